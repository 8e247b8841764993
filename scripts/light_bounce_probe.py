#!/usr/bin/env python3
"""What rm_shade_rays_indirect and rm_light_probes_indirect cost beside the calls without a grid, and beside the composition a caller
writes without them.  One GPU, one build.  Per input a child process of its own under a time limit of its own; the first one that
fails ends the run, and what the earlier ones measured stays in --out.  In a child the routes are interleaved round by round, HIP
events around whole calls (the protocol of profiles/light_grid.md and light_depth.md): `launches` calls per event pair, `rounds`
rounds, ms per call as median [min – max] over the rounds, after one untimed call of every route.

(a) Frames (inputs frame_c2: the 1080p frame of directional_light_2.json; frame_bulb: the 4K Mandelbulb): camera_rays in
    tile_order, on the device before the clock starts; a 32³ grid with depth records baked by light_grid_visible (64 directions).
  fused        Renderer.shade_rays_indirect into a tensor allocated before: ONE launch.
  bare         Renderer.shade_rays on the same rays: the price of the term is fused − bare.
  composition  what a caller has without the entry: shade_rays + trace_rays (tMax = far) + grid.irradiance on the hit points and
               normals + the torch albedo kd · cDiffuse[object] · max(e, 0) · strength / π added to the colour.  It has no texture and
               no palette in its albedo: on the Mandelbulb it computes another, poorer picture.
(b) Bakes (inputs bake_c2, bake_bulb): 32³ probes over mesh_bounds, 256 directions, one set, reading a 32³ grid baked before.
  fused        Renderer.light_probes_indirect: ONE launch.
  bare         Renderer.light_probes at the same positions.
  composition  the n·K rays built on the device, the frame composition above on them, and the projection as one torch matmul per
               probe batch (colour and hit flag times the basis), in slices of 2²¹ rays so that it fits.
(c) Peak extra device memory of a route: torch.cuda.max_memory_allocated around one call minus what was allocated before it.

  python scripts/light_bounce_probe.py [--rounds 5] [--launches 4] [--out profiles/light_bounce.md] [--limit 420]"""
import argparse
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
NAMES = ("frame_c2", "frame_bulb", "bake_c2", "bake_bulb")


def child(args):
    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, light_grid_positions, scenes, sphere_directions
    from raymarcher_amd.render import tile_order

    r = Renderer(0)
    dev = r.device
    lines = []
    mib = 1.0 / (1 << 20)

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(args.section, "w") as f:  # as it goes: a child that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    def timed(variants, launches):
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / launches)
        return times

    def show(v):
        return f"{statistics.median(v):.3f} [{min(v):.3f} – {max(v):.3f}]"

    def med(v):
        return statistics.median(v)

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        keep = fn()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - before
        del keep
        return extra

    bulb = args.scene.endswith("bulb")
    frame = args.scene.startswith("frame")
    W, H = (3840, 2160) if bulb else (1920, 1080)
    if bulb:
        t, s = scenes.mandelbulb(W, H), abi.default_settings()
    else:
        t, s = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H), abi.default_settings()
    far = t.camera.initialFar
    grid = r.light_grid_visible(t, s, (32, 32, 32), directions=64)
    albedo = torch.tensor([list(t.objects[i].cDiffuse) for i in range(t.num_objects)], dtype=torch.float32, device=dev)
    scale = float(t.globals_.kd) / math.pi

    def composition(rays, out=None):
        """shade_rays + trace_rays + irradiance + the torch albedo → colours (n, 4)."""
        colour = r.shade_rays(t, s, rays, far=far, out=out)
        probe = rays.clone()
        probe[:, 3] = far
        normal, _, point, obj = r.trace_rays(t, s, probe)
        n = rays.shape[0]
        p4, n4 = torch.zeros((n, 4), device=dev), torch.zeros((n, 4), device=dev)
        p4[:, 0:3], n4[:, 0:3] = point, normal
        e, _, probes = grid.irradiance(p4, n4)
        on = (obj >= 0) & (probes > 0)
        ind = albedo[obj.clamp(min=0).long()] * e[:, 0:3].clamp(min=0) * scale
        colour[:, 0:3] += torch.where(on[:, None], ind, torch.zeros_like(ind))
        return colour

    title = "the Mandelbulb" if bulb else "c2 (directional_light_2.json)"
    if frame:
        rays = torch.from_numpy(camera_rays(t.camera, W, H)[tile_order(W, H)]).to(dev)
        n = rays.shape[0]
        out = torch.empty((n, 4), dtype=torch.float32, device=dev)
        emit(f"## (a) The {W}×{H} frame of {title}: {n} camera rays in tile order, a 32³ grid with depth records")
        emit()
        head = ("| rays | fused, ms | bare shade_rays, ms | composition, ms | fused − bare, ms | fused / bare | composition / fused | "
                "fused: peak extra MiB | composition: peak extra MiB | 16 B · n, MiB | rays with a term | max abs(fused − composition) |")
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        tm = timed({"fused": lambda: r.shade_rays_indirect(t, s, rays, grid, far=far, out=out),
                    "bare": lambda: r.shade_rays(t, s, rays, far=far, out=out),
                    "composed": lambda: composition(rays, out)}, args.launches)
        a = r.shade_rays_indirect(t, s, rays, grid, far=far).clone()
        bare = r.shade_rays(t, s, rays, far=far).clone()
        b = composition(rays)
        lit = int((a.view(torch.int32) != bare.view(torch.int32)).any(dim=1).sum())
        delta = float((a - b).abs().max())
        del a, b, bare
        mem_fused = peak_extra(lambda: r.shade_rays_indirect(t, s, rays, grid, far=far))
        mem_composed = peak_extra(lambda: composition(rays))
        emit(f"| {n} | {show(tm['fused'])} | {show(tm['bare'])} | {show(tm['composed'])} | {med(tm['fused']) - med(tm['bare']):.3f} | "
             f"{med(tm['fused']) / med(tm['bare']):.3f} | {med(tm['composed']) / med(tm['fused']):.2f} | {mem_fused * mib:.1f} | "
             f"{mem_composed * mib:.1f} | {16.0 * n * mib:.1f} | {lit} | {delta:.3e} |")
        torch.cuda.synchronize()
        return 0

    g, K = 32, 256
    n = g ** 3
    pos = torch.from_numpy(light_grid_positions(grid.origin, grid.step, grid.dims)).to(dev)
    table = torch.from_numpy(sphere_directions(K, 1)).to(dev)
    out = torch.empty((n, 40), dtype=torch.float32, device=dev)
    emit(f"## (b) The bake on {title}: {g}³ probes at the grid's own positions, {K} directions, reading the 32³ grid with depth records")
    emit()
    head = ("| probes | rays | fused, ms | bare light_probes, ms | composition, ms | fused − bare, ms | fused / bare | composition / fused | "
            "fused: peak extra MiB | composition: peak extra MiB | 160 B · n, MiB | max abs(fused − composition) band 0 |")
    emit(head)
    emit("|" + "---|" * (head.count("|") - 1))
    chunk = (1 << 21) // K  # probes per slice of the composition

    def composed_bake():
        rec = torch.empty((n, 9, 4), dtype=torch.float32, device=dev)
        basis = table[:, 4:13]  # (K, 9)
        for lo in range(0, n, chunk):
            m = min(chunk, n - lo)
            rays = torch.zeros((m, K, 8), dtype=torch.float32, device=dev)
            rays[:, :, 0:3] = pos[lo:lo + m, None, 0:3]
            rays[:, :, 3] = far
            rays[:, :, 4:7] = table[None, :, 0:3]
            rays = rays.view(m * K, 8)
            colour = composition(rays)
            hit = r.trace_rays(t, s, rays, normals=False)[3] >= 0
            colour[:, 3] = hit.float()
            rec[lo:lo + m] = torch.einsum("kj,mkc->mjc", basis, colour.view(m, K, 4))
        return rec

    tm = timed({"fused": lambda: r.light_probes_indirect(t, s, pos, grid, directions=K, far=far, table=table, out=out),
                "bare": lambda: r.light_probes(t, s, pos, directions=K, far=far, table=table, out=out),
                "composed": composed_bake}, args.bake_launches)
    a = r.light_probes_indirect(t, s, pos, grid, directions=K, far=far, table=table)[0].clone()
    b = composed_bake()
    delta = float((a[:, 0, 0:3] - b[:, 0, 0:3]).abs().max())
    del a, b
    mem_fused = peak_extra(lambda: r.light_probes_indirect(t, s, pos, grid, directions=K, far=far, table=table))
    mem_composed = peak_extra(composed_bake)
    emit(f"| {g}³ = {n} | {n * K} | {show(tm['fused'])} | {show(tm['bare'])} | {show(tm['composed'])} | {med(tm['fused']) - med(tm['bare']):.3f} | "
         f"{med(tm['fused']) / med(tm['bare']):.3f} | {med(tm['composed']) / med(tm['fused']):.2f} | {mem_fused * mib:.1f} | {mem_composed * mib:.1f} | "
         f"{160.0 * n * mib:.1f} | {delta:.3e} |")
    torch.cuda.synchronize()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=4, help="calls per event pair of the frames")
    ap.add_argument("--bake-launches", type=int, default=2, help="calls per event pair of the bakes")
    ap.add_argument("--limit", type=int, default=420, help="seconds an input's child process may take")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    ap.add_argument("--scene", default=None, choices=NAMES, help="(internal) measure this input in this process")
    ap.add_argument("--section", default=None, help="(internal) where the child writes its section")
    args = ap.parse_args()
    if args.scene:
        return child(args)
    import tempfile
    text = ["# rm_shade_rays_indirect and rm_light_probes_indirect beside the calls without a grid and beside the composition", "",
            f"{args.rounds} interleaved rounds, HIP events around the calls ({args.launches} calls per pair for the frames, {args.bake_launches} for "
            "the bakes); ms per call, median [min – max] over the rounds.  The routes and the columns are in the head of "
            "scripts/light_bounce_probe.py.", ""]
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for scene in NAMES:
            section = os.path.join(tmp, scene + ".md")
            cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--section", section, "--rounds", str(args.rounds), "--launches",
                   str(args.launches), "--bake-launches", str(args.bake_launches)]
            try:
                status = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                status = 124
            if os.path.exists(section):
                text += open(section).read().splitlines() + [""]
            if status != 0:
                text += [f"{scene}: ended with status {status}; nothing after it was run.", ""]
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(text))
            if status != 0:
                break
    return status


if __name__ == "__main__":
    sys.exit(main())
