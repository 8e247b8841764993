#!/usr/bin/env python3
"""What rm_light_grid_irradiance buys beside the composition a caller writes without it.  One GPU, one build.  Per input a child
process of its own under a time limit of its own; the first one that fails ends the run, and what the earlier ones measured stays in
--out.  In a child the routes are interleaved round by round, HIP events around whole calls (scripts/light_probes_probe.py's
pattern): `launches` calls per event pair, `rounds` rounds, ms per call as median [min – max] over the rounds, after one
untimed call of every route.

  fused        LightGrid.irradiance into a tensor allocated before: ONE launch of rm_light_grid_irradiance.
  composition  on the same commit, from the same records, in torch: the cell and the trilinear weights, a gather of the eight
               probes' hits and coefficients ((n, 8, 9, 4) floats, 1152 B per point), the same facing weights, sh_irradiance per
               corner and the weighted blend.  Timed end to end.

Peak extra device memory of a route: torch.cuda.max_memory_allocated around one call minus what was allocated before it; the fused
route's includes its (n, 8) result.  The two routes differ by rounding only (torch fuses nothing but orders its sums its own way);
the largest difference of e relative to the largest |e| is reported.

Inputs: c2 — the primary hit points of directional_light_2.json's 1920×1080 G-buffer against a 32³ grid over mesh_bounds, facing on
and off, in pixel order, shuffled, and the first 10⁴ —; bulb — the vertices of scene_mesh_pruned of the Mandelbulb (12 iterations)
at 1025 with shade_points' normals, against a 64³ grid.  The grids are Renderer.light_grid's, 64 directions, probes inside geometry
masked.

The calls of an event pair repeat on the same buffers: points, normals and result (64 B per point) stay in the Infinity Cache from one
call to the next, as the grid does, for both routes alike.  A fused call of 10⁴ points is at the floor of one launch from Python.

  python scripts/light_grid_probe.py [--rounds 5] [--launches 20] [--out profiles/light_grid.md] [--limit 420]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
NAMES = ("c2", "bulb")


def child(args):
    import torch
    from raymarcher_amd import Renderer, Scene, abi, scenes, sh_irradiance

    r = Renderer(0)
    dev = r.device
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(args.section, "w") as f:  # as it goes: a child that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

    def timed(variants):
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.launches)
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

    def composition(grid, pts, nrm, facing):
        """The lookup in torch, with the entry's weights."""
        nx, ny, nz = grid.dims
        o, s = torch.from_numpy(grid.origin).to(dev), torch.from_numpy(grid.step).to(dev)
        top = torch.tensor([nx - 1, ny - 1, nz - 1], dtype=torch.float32, device=dev)
        p, n = pts[:, 0:3], nrm[:, 0:3]
        u = torch.minimum(((p - o) / s).clamp(min=0.0), top)
        cell = torch.minimum(u.floor(), top - 1.0)
        f = u - cell
        bits = torch.tensor([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)], dtype=torch.float32, device=dev)
        at = cell[:, None, :] + bits[None, :, :]                                     # (n, 8, 3)
        index = (at[..., 0] + nx * (at[..., 1] + ny * at[..., 2])).long()            # (n, 8)
        w = torch.where(bits[None, :, :] > 0, f[:, None, :], 1.0 - f[:, None, :]).prod(dim=2)
        valid = grid.probes[:, 36].view(torch.int32)[index] >= 0
        if facing:
            d = (o + at * s) - p[:, None, :]
            length = d.norm(dim=2)
            b = ((d * n[:, None, :]).sum(dim=2) / length + 1.0) * 0.5
            w = w * torch.where(length == 0, torch.ones_like(b), b * b + 0.2)
        w = torch.where(valid, w, torch.zeros_like(w))
        sh = grid.probes[:, 0:36][index].view(-1, 8, 9, 4)                           # the gather: 1152 B per point
        E = sh_irradiance(sh, n[:, None, :])                                         # (n, 8, 4)
        E = torch.where(valid[:, :, None], E, torch.zeros_like(E))
        return (w[:, :, None] * E).sum(dim=1) / w.sum(dim=1, keepdim=True)

    head = ("| points | n | facing | fused, ms | composition, ms | composition / fused | fused: peak extra MiB | composition: peak extra MiB | "
            "32 B · n, MiB | 1152 B · n, MiB | max Δe / max e | points with 8 probes | with none |")

    def measure(grid, pts, nrm, label, facings=(True, False)):
        n = pts.shape[0]
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        mib = 1.0 / (1 << 20)
        for facing in facings:
            tm = timed({"fused": lambda: grid.irradiance(pts, nrm, facing=facing, out=out),
                        "composed": lambda: composition(grid, pts, nrm, facing)})
            e, _w, probes = grid.irradiance(pts, nrm, facing=facing, out=out)
            ref = composition(grid, pts, nrm, facing)
            lit = probes > 0
            scale = float(e[lit].abs().max())
            delta = float((e[lit] - ref[lit]).abs().max()) / scale
            del ref
            mem_fused = peak_extra(lambda: grid.irradiance(pts, nrm, facing=facing))
            mem_composed = peak_extra(lambda: composition(grid, pts, nrm, facing))
            emit(f"| {label} | {n} | {'on' if facing else 'off'} | {show(tm['fused'])} | {show(tm['composed'])} | "
                 f"{statistics.median(tm['composed']) / statistics.median(tm['fused']):.2f} | {mem_fused * mib:.1f} | {mem_composed * mib:.1f} | "
                 f"{32.0 * n * mib:.1f} | {1152.0 * n * mib:.1f} | {delta:.2e} | {int((probes == 8).sum())} | {int((probes == 0).sum())} |")
            torch.cuda.synchronize()

    if args.scene == "c2":
        W, H = 1920, 1080
        t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
        s = abi.default_settings()
        grid = r.light_grid(t, s, (32, 32, 32), directions=64)
        masked = int((grid.probes[:, 36].view(torch.int32) < 0).sum())
        nd, ids, pos = r.render_gbuffer(t, s, W, H, position=True)
        hit = ids.reshape(-1) >= 0
        pts, nrm = pos.reshape(-1, 4)[hit].contiguous(), nd.reshape(-1, 4)[hit].contiguous()
        del nd, ids, pos
        emit(f"## c2 (directional_light_2.json): the {pts.shape[0]} primary hit points of the {W}×{H} G-buffer, a 32³ grid over mesh_bounds "
             f"({masked} of 32768 probes masked), step {grid.step[0]:.4f} {grid.step[1]:.4f} {grid.step[2]:.4f}")
        emit()
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        measure(grid, pts, nrm, "(a) pixel order")
        perm = torch.randperm(pts.shape[0], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        measure(grid, pts[perm].contiguous(), nrm[perm].contiguous(), "(b) shuffled")
        measure(grid, pts[:10000].contiguous(), nrm[:10000].contiguous(), "(c) the first 10 000")
    else:
        t, s = scenes.mandelbulb(64, 36), abi.default_settings(fractalIters=12)
        grid = r.light_grid(t, s, (64, 64, 64), directions=64)
        masked = int((grid.probes[:, 36].view(torch.int32) < 0).sum())
        verts, _quads, _vobj = r.scene_mesh_pruned(t, s, 1025)
        normal = r.shade_points(t, s, verts, colour=False)[0]
        nrm = torch.zeros_like(verts)
        nrm[:, 0:3] = normal
        del normal, _quads, _vobj
        emit(f"## Mandelbulb (12 iterations): the {verts.shape[0]} vertices of scene_mesh_pruned at 1025 with shade_points' normals, a 64³ grid "
             f"over mesh_bounds ({masked} of 262144 probes masked), step {grid.step[0]:.4f}")
        emit()
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        measure(grid, verts, nrm, "(d) mesh vertices, surface-nets order")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--limit", type=int, default=420, help="seconds an input's child process may take")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    ap.add_argument("--scene", default=None, choices=NAMES, help="(internal) measure this input in this process")
    ap.add_argument("--section", default=None, help="(internal) where the child writes its section")
    args = ap.parse_args()
    if args.scene:
        return child(args)
    import tempfile
    text = ["# rm_light_grid_irradiance beside a torch gather and blend", "",
            f"{args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the calls; ms per call, median [min – max] over "
            "the rounds.  The routes and the columns are in the head of scripts/light_grid_probe.py.  Mapping: one lane per point, 256-lane "
            "workgroups, eight hits words and then nine float4 per valid corner, two 16-byte stores.", ""]
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for scene in NAMES:
            section = os.path.join(tmp, scene + ".md")
            cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--section", section, "--rounds", str(args.rounds), "--launches",
                   str(args.launches)]
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
