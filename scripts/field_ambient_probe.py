#!/usr/bin/env python3
"""What rm_field_ambient buys beside the composition a caller writes without it.  One GPU, one build.  Per shape a child process of
its own under a time limit of its own; the first one that fails ends the run, and what the earlier ones measured stays in --out.
In a child the two routes are interleaved round by round, HIP events around whole calls (scripts/field_handle_probe.py's pattern,
DESIGN §7): `launches` calls per event pair, `rounds` rounds, ms per call as median [min – max] over the rounds, after one untimed
call of every route.

  fused        LatticeField.ambient into a tensor allocated before: ONE launch of rm_field_ambient.
  composition  on the same commit, from the same table and the same normals: the frame of Duff et al. and the n·K RmRay rows built
               on the device with torch, rm_field_trace RM_TRACE_OCCLUSION on them, and a torch reduction of the n·K RmRayHit rows
               to (bent, visibility, hits).  Timed end to end, and the rm_field_trace call in the middle alone.

Peak extra device memory of a route: torch.cuda.max_memory_allocated around one call minus what was allocated before it; the fused
route's includes its (n, 8) result.  The two routes' visibility differ by the order of the sum only (the composition's torch.sum has
its own); the largest difference and whether the hit counts are equal are reported.

Shapes:
  c2-dense     c2 (directional_light_2.json, 1920×1080): the primary hit points in 8×8-tile order with their normals, on the DENSE
               lattice of --dense points, SOFT, 16 and 64 directions; and the first 10 000 of them at 64, the small-count case.
  bulb-sparse  the vertices of scene_mesh_pruned of the Mandelbulb (12 iterations) at --sparse, on scene_field_pruned's lattice of the
               same resolution, normals from the lattice's own gradient, SOFT, 16 and 64 directions.

  python scripts/field_ambient_probe.py [--rounds 5] [--launches 3] [--dense 513] [--sparse 1025] [--out profiles/field_ambient.md]
                                        [--limit 420]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
SHAPES = ("c2-dense", "bulb-sparse")
ISO, STEPS = 0.001, 64


def child(args):
    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, hemisphere_directions, scenes, tile_order

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

    def measure(field, pts, nrm, K, bias, far, label):
        n = pts.shape[0]
        table = torch.from_numpy(hemisphere_directions(K, 1)).to(dev)
        out = torch.empty((n, 8), dtype=torch.float32, device=dev)
        rays = torch.empty((n * K, 8), dtype=torch.float32, device=dev)
        hits = torch.empty((n * K, 8), dtype=torch.float32, device=dev)

        def fused(into=out):
            return field.ambient(pts, nrm, directions=table, sets=1, max_distance=far, bias=bias, iso=ISO, max_steps=STEPS, soft=True, out=into)

        def build(into):
            nx, ny, nz = nrm[:, 0], nrm[:, 1], nrm[:, 2]
            s = torch.copysign(torch.ones_like(nz), nz)
            a = -1.0 / (s + nz)
            b = nx * ny * a
            T = torch.stack([1.0 + s * nx * nx * a, s * b, -s * nx], dim=1)
            B = torch.stack([b, s + ny * ny * a, -ny], dim=1)
            d = table[None, :, 0:1] * T[:, None, :] + table[None, :, 1:2] * B[:, None, :] + table[None, :, 2:3] * nrm[:, None, 0:3]
            v = into.view(n, K, 8)
            v[:, :, 0:3] = (pts[:, 0:3] + nrm[:, 0:3] * bias)[:, None, :]
            v[:, :, 3] = far
            v[:, :, 4:7] = d
            v[:, :, 7] = 0.0
            return into

        def trace(src, into):
            return field.trace(src, iso=ISO, max_steps=STEPS, mode="occlusion", out=into)

        def reduce(src, from_hits):
            h = from_hits.view(n, K, 8)
            oid = h[:, :, 7].view(torch.int32)
            c = table[None, :, 3] * torch.where(oid == -1, h[:, :, 3].clamp(min=0.0), torch.zeros((), device=dev))
            bent = (c[:, :, None] * src.view(n, K, 8)[:, :, 4:7]).sum(dim=1)
            return bent, c.sum(dim=1), ((oid != -1) & (oid != abi.RM_RAY_INVALID)).sum(dim=1)

        def composed(own_memory=False):
            src = build(torch.empty((n * K, 8), dtype=torch.float32, device=dev) if own_memory else rays)
            dst = torch.empty((n * K, 8), dtype=torch.float32, device=dev) if own_memory else hits
            trace(src, dst)
            return reduce(src, dst)

        build(rays)
        tm = timed({"fused": fused, "composed": composed, "trace": lambda: trace(rays, hits)})
        fused()
        bent, vis, count = composed()
        ok = out[:, 7].view(torch.int32) >= 0
        dv = float((out[:, 3] - vis)[ok].abs().max())
        same_hits = bool((out[:, 7].view(torch.int32)[ok] == count[ok]).all())
        mem_fused = peak_extra(lambda: fused(None))
        rays = hits = None  # the timed routes' buffers: the composition below allocates its own
        mem_composed = peak_extra(lambda: composed(True))
        mib = 1.0 / (1 << 20)
        emit(f"| {label} | {n} | {K} | {show(tm['fused'])} | {show(tm['composed'])} | {show(tm['trace'])} | "
             f"{statistics.median(tm['composed']) / statistics.median(tm['fused']):.2f} | "
             f"{statistics.median(tm['trace']) / statistics.median(tm['fused']):.2f} | {mem_fused * mib:.1f} | {mem_composed * mib:.1f} | "
             f"{32.0 * n * mib:.1f} | {64.0 * n * K * mib:.1f} | {dv:.2e} | {'equal' if same_hits else 'DIFFER'} | "
             f"{float(out[:, 3][ok].mean()):.3f} |")

    head = ("| shape | points | directions | fused, ms | composition, ms | its rm_field_trace alone, ms | composition / fused | trace alone / fused | "
            "fused: peak extra MiB | composition: peak extra MiB | 32 B · n, MiB | 64 B · n · K, MiB | max abs Δ visibility | hit counts | "
            "mean visibility |")
    if args.shape == "c2-dense":
        W, H = 1920, 1080
        t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
        s = abi.default_settings()
        rays = torch.from_numpy(camera_rays(t.camera, W, H)[tile_order(W, H)]).to(dev).contiguous()
        nrm, _tt, pos, oid = r.trace_rays(t, s, rays)
        hit = oid >= 0
        pts = torch.zeros((int(hit.sum()), 4), dtype=torch.float32, device=dev)
        nrm4 = torch.zeros_like(pts)
        pts[:, 0:3], nrm4[:, 0:3] = pos[hit], nrm[hit]
        del rays, pos, nrm, oid
        origin, step, dims = r._scene_lattice(t, args.dense, None)
        dense, ids = r.sdf_grid(t, s, origin, (step,) * 3, dims, ids=True)
        far = float(sum((step * (d - 1)) ** 2 for d in dims) ** 0.5)
        emit(f"## c2 (directional_light_2.json, {W}×{H}): the {pts.shape[0]} primary hit points in 8×8-tile order, the dense lattice of "
             f"{dims[0]}×{dims[1]}×{dims[2]} points, step {step:.5f}")
        emit()
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        with r.lattice_field(dense, origin, (step,) * 3, ids=ids) as field:
            for K in (16, 64):
                measure(field, pts, nrm4, K, 2.0 * step, far, "all hit points")
            measure(field, pts[:10000].contiguous(), nrm4[:10000].contiguous(), 64, 2.0 * step, far, "the first 10 000")
            torch.cuda.synchronize()
    else:
        W, H = 64, 36
        t, s = scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12)
        verts, _quads, _vobj = r.scene_mesh_pruned(t, s, args.sparse, iso=ISO)
        grid, ids, bl, blocks, origin, step = r.scene_field_pruned(t, s, args.sparse, iso=ISO)
        far = float(sum((step[a] * 8 * blocks[a]) ** 2 for a in range(3)) ** 0.5)
        emit(f"## Mandelbulb (12 iterations): the {verts.shape[0]} vertices of scene_mesh_pruned at {args.sparse}, scene_field_pruned's lattice "
             f"({bl.shape[0]} listed of {blocks[0] * blocks[1] * blocks[2]} blocks), step {step[0]:.5f}")
        emit()
        emit(head)
        emit("|" + "---|" * (head.count("|") - 1))
        with r.lattice_field_blocks(grid, bl, blocks, origin, step, ids=ids) as field:
            g, _v, _c, code = field.sample(verts)
            length = g.norm(dim=1)
            good = (code > abi.RM_RAY_INVALID) & (length > 0) & torch.isfinite(length)
            pts = verts[good].contiguous()
            nrm4 = torch.zeros_like(pts)
            nrm4[:, 0:3] = g[good] / length[good][:, None]
            emit(f"<!-- {int(good.sum())} of {verts.shape[0]} vertices have a gradient in a listed block -->")
            for K in (16, 64):
                measure(field, pts, nrm4, K, 2.0 * step[0], far, "mesh vertices, surface-nets order")
            torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--dense", type=int, default=513)
    ap.add_argument("--sparse", type=int, default=1025)
    ap.add_argument("--limit", type=int, default=420, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    ap.add_argument("--shape", default=None, choices=SHAPES, help="(internal) measure this shape in this process")
    ap.add_argument("--section", default=None, help="(internal) where the child writes its section")
    args = ap.parse_args()
    if args.shape:
        return child(args)
    import tempfile
    text = ["# rm_field_ambient beside rm_field_trace and torch", "",
            f"{args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the calls; ms per call, median [min – max] over "
            f"the rounds.  SOFT, iso {ISO}, {STEPS} samples, bias twice the step, maxDistance the lattice's diagonal, one set of directions.  "
            "The routes and the columns are in the head of scripts/field_ambient_probe.py.  Mapping: (point, direction) pairs flattened "
            "over lanes, a segment of numDirs lanes per point, xor-shuffle tree.", ""]
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for shape in SHAPES:
            section = os.path.join(tmp, shape + ".md")
            cmd = [sys.executable, os.path.abspath(__file__), "--shape", shape, "--section", section, "--rounds", str(args.rounds), "--launches",
                   str(args.launches), "--dense", str(args.dense), "--sparse", str(args.sparse)]
            try:
                status = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                status = 124
            if os.path.exists(section):
                text += open(section).read().splitlines() + [""]
            if status != 0:
                text += [f"{shape}: ended with status {status}; nothing after it was run.", ""]
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(text))
            if status != 0:
                break
    return status


if __name__ == "__main__":
    sys.exit(main())
