#!/usr/bin/env python3
"""What rm_light_probes_depth buys beside the composition a caller writes without it, and what the visibility term costs a lookup.
One GPU, one build.  Per input a child process of its own under a time limit of its own; the first one that fails ends the run,
and what the earlier ones measured stays in --out.  In a child the routes are interleaved round by round, HIP events around whole
calls (the protocol of profiles/light_grid.md): `launches` calls per event pair, `rounds` rounds, ms per call as median [min – max]
over the rounds, after one untimed call of every route.

The bake (inputs bake_c2, bake_bulb): 32³ probes on a grid over the box of the scene's cull ball, 256 directions, one set,
probe_depth_weights at sharpness 50, max_distance = 1.5 × the length of the grid's step.
  fused        Renderer.light_probes_depth into a tensor allocated before: ONE launch of rm_light_probes_depth.
  composition  on the same commit, from the same table and weights: the n·K RmRay rows built on the device with torch,
               rm_trace_rays (closest, no normals) on them, and two torch matmuls of t and t·t (n, K) with the weights (K, 64).
               Timed end to end; the projection is a GEMM and fast.
  trace alone  the bare rm_trace_rays call in the middle, on rays already built.
The routes' moments differ by the order of the sums only; the largest difference relative to the largest moment is reported.

The lookup (inputs look_c2, look_bulb): the points (a), (b) and (d) of scripts/light_grid_probe.py on its grids, baked with
light_grid_visible.
  visible      LightGrid.irradiance_visible(visible=True): ONE launch of rm_light_grid_irradiance_visible.
  plain        the same grid, visible=False: ONE launch of rm_light_grid_irradiance, whose unit this commit does not touch —
               the parent commit's code object.
Peak extra device memory of a route: torch.cuda.max_memory_allocated around one call minus what was allocated before it.

  python scripts/light_depth_probe.py [--rounds 5] [--launches 20] [--out profiles/light_depth.md] [--limit 420]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
NAMES = ("bake_c2", "bake_bulb", "look_c2", "look_bulb")


def child(args):
    import torch
    from raymarcher_amd import Renderer, Scene, abi, lib, probe_depth_weights, scenes, sphere_directions

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

    def c2(W, H):
        return Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H), abi.default_settings()

    if args.scene.startswith("bake"):
        t, s = c2(64, 36) if args.scene == "bake_c2" else (scenes.mandelbulb(64, 36), abi.default_settings())
        title = "c2 (directional_light_2.json)" if args.scene == "bake_c2" else "the Mandelbulb"
        bounds = (C.c_float * 14)()
        assert lib().rm_debug_cull_bounds(t.objects, t.num_objects, C.byref(t.globals_), bounds) == 0
        centre, radius = ((bounds[1], bounds[2], bounds[3]), bounds[4] ** 0.5) if bounds[0] != 0.0 and bounds[4] > 0.0 else ((0.0, 0.0, 0.0), 3.0)
        g, K = 32, 256
        n = g ** 3
        dist = 1.5 * (3.0 ** 0.5) * (2.0 * radius / (g - 1))
        emit(f"## The bake on {title}: {g}³ probes on a grid over the box of the cull ball (centre {centre[0]:.2f} {centre[1]:.2f} {centre[2]:.2f}, "
             f"radius {radius:.2f}), {K} directions, max_distance {dist:.4f}")
        emit()
        head = ("| probes | rays | fused, ms | composition, ms | its rm_trace_rays alone, ms | composition / fused | trace alone / fused | "
                "fused: peak extra MiB | composition: peak extra MiB | 512 B · n, MiB | 64 B · n · K, MiB | max Δ moment / max moment | rays that hit |")
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        axis = torch.linspace(-1.0, 1.0, g, device=dev) * radius
        pos = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        pos[:, 0:3] = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=3).reshape(n, 3) + torch.tensor(centre, device=dev)
        host_table = sphere_directions(K, 1)
        table = torch.from_numpy(host_table).to(dev)
        weights = torch.from_numpy(probe_depth_weights(host_table, 1, 50.0)).to(dev)
        out = torch.empty((n, 64, 2), dtype=torch.float32, device=dev)
        rays = torch.empty((n * K, 8), dtype=torch.float32, device=dev)
        hits = torch.empty((n * K, 8), dtype=torch.float32, device=dev)

        def fused(into=out):
            return r.light_probes_depth(t, s, pos, directions=K, sets=1, max_distance=dist, table=table, weights=weights, out=into)

        def build(into):
            v = into.view(n, K, 8)
            v[:, :, 0:3] = pos[:, None, 0:3]
            v[:, :, 3] = dist
            v[:, :, 4:7] = table[None, :, 0:3]
            v[:, :, 7] = 0.0
            return into

        def trace(src, into):
            return r.trace_rays(t, s, src, normals=False, out=into)

        def composed(own_memory=False):
            src = build(torch.empty((n * K, 8), dtype=torch.float32, device=dev) if own_memory else rays)
            d = trace(src, None if own_memory else hits)[1].view(n, K)
            return torch.stack([d @ weights, (d * d) @ weights], dim=2)

        build(rays)
        tm = timed({"fused": fused, "composed": composed, "trace": lambda: trace(rays, hits)}, args.bake_launches)
        rec = fused()
        ref = composed()
        scale = float(ref.abs().max())
        delta = float((rec - ref).abs().max()) / scale if scale > 0 else 0.0
        share = float((trace(rays, hits)[3] >= 0).sum()) / (n * K)
        mem_fused = peak_extra(lambda: fused(None))
        del rays, hits, ref
        mem_composed = peak_extra(lambda: composed(True))
        emit(f"| {g}³ = {n} | {n * K} | {show(tm['fused'])} | {show(tm['composed'])} | {show(tm['trace'])} | "
             f"{statistics.median(tm['composed']) / statistics.median(tm['fused']):.2f} | "
             f"{statistics.median(tm['trace']) / statistics.median(tm['fused']):.2f} | {mem_fused * mib:.1f} | {mem_composed * mib:.1f} | "
             f"{512.0 * n * mib:.1f} | {64.0 * n * K * mib:.1f} | {delta:.2e} | {share:.3f} |")
        torch.cuda.synchronize()
        return 0

    head = ("| points | n | facing | visible, ms | plain, ms | visible / plain | visible: peak extra MiB | 32 B · n, MiB | "
            "points whose record differs | mean e.rgb visible / plain |")

    def measure(grid, pts, nrm, label, facings=(True, False)):
        n = pts.shape[0]
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        for facing in facings:
            tm = timed({"visible": lambda: grid.irradiance_visible(pts, nrm, facing=facing, out=out, visible=True),
                        "plain": lambda: grid.irradiance_visible(pts, nrm, facing=facing, out=out, visible=False)}, args.launches)
            a = grid.irradiance_visible(pts, nrm, facing=facing, visible=True)[0].clone()
            b = grid.irradiance_visible(pts, nrm, facing=facing, visible=False)[0]
            differ = int((a.view(torch.int32) != b.view(torch.int32)).any(dim=1).sum())
            ratio = float(a[:, 0:3].sum() / b[:, 0:3].sum())
            del a, b
            mem = peak_extra(lambda: grid.irradiance_visible(pts, nrm, facing=facing, visible=True))
            emit(f"| {label} | {n} | {'on' if facing else 'off'} | {show(tm['visible'])} | {show(tm['plain'])} | "
                 f"{statistics.median(tm['visible']) / statistics.median(tm['plain']):.2f} | {mem * mib:.1f} | {32.0 * n * mib:.1f} | {differ} | {ratio:.4f} |")
            torch.cuda.synchronize()

    if args.scene == "look_c2":
        W, H = 1920, 1080
        t, s = c2(W, H)
        grid = r.light_grid_visible(t, s, (32, 32, 32), directions=64)
        nd, ids, pos = r.render_gbuffer(t, s, W, H, position=True)
        hit = ids.reshape(-1) >= 0
        pts, nrm = pos.reshape(-1, 4)[hit].contiguous(), nd.reshape(-1, 4)[hit].contiguous()
        del nd, ids, pos
        emit(f"## The lookup on c2: the {pts.shape[0]} primary hit points of the {W}×{H} G-buffer, a 32³ grid over mesh_bounds with depth records "
             f"(16 MiB beside 5 MiB of SH), step {grid.step[0]:.4f} {grid.step[1]:.4f} {grid.step[2]:.4f}, normal_bias {0.25 * float(grid.step.min()):.4f}")
        emit()
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        measure(grid, pts, nrm, "(a) pixel order")
        perm = torch.randperm(pts.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        measure(grid, pts[perm].contiguous(), nrm[perm].contiguous(), "(b) shuffled")
    else:
        t, s = scenes.mandelbulb(64, 36), abi.default_settings(fractalIters=12)
        grid = r.light_grid_visible(t, s, (64, 64, 64), directions=64)
        verts, _quads, _vobj = r.scene_mesh_pruned(t, s, 1025)
        normal = r.shade_points(t, s, verts, colour=False)[0]
        nrm = torch.zeros_like(verts)
        nrm[:, 0:3] = normal
        del normal, _quads, _vobj
        emit(f"## The lookup on the Mandelbulb (12 iterations): the {verts.shape[0]} vertices of scene_mesh_pruned at 1025, a 64³ grid over "
             f"mesh_bounds with depth records (128 MiB beside 40 MiB of SH), step {grid.step[0]:.4f}")
        emit()
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        measure(grid, verts, nrm, "(d) mesh vertices, surface-nets order")
    torch.cuda.synchronize()
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="calls per event pair of the lookups")
    ap.add_argument("--bake-launches", type=int, default=2, help="calls per event pair of the bakes")
    ap.add_argument("--limit", type=int, default=420, help="seconds an input's child process may take")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    ap.add_argument("--scene", default=None, choices=NAMES, help="(internal) measure this input in this process")
    ap.add_argument("--section", default=None, help="(internal) where the child writes its section")
    args = ap.parse_args()
    if args.scene:
        return child(args)
    import tempfile
    text = ["# rm_light_probes_depth beside rm_trace_rays and torch; rm_light_grid_irradiance_visible beside rm_light_grid_irradiance", "",
            f"{args.rounds} interleaved rounds, HIP events around the calls ({args.bake_launches} calls per pair for the bakes, {args.launches} for "
            "the lookups); ms per call, median [min – max] over the rounds.  The routes and the columns are in the head of "
            "scripts/light_depth_probe.py.", ""]
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
