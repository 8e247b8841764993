#!/usr/bin/env python3
"""The block-sparse lattice (rm_sdf_blocks_select, rm_sdf_grid_blocks, rm_sdf_mesh_blocks) measured.  One process, one GPU, the
routes of a table interleaved round by round, outputs compared before anything is timed.

  A  lane mapping: rm_sdf_blocks_select of this build (runs of 64 in x-fastest order) and of --variant-lib (a build with
     -DRM_BLOCKS_MAP=1: 9×3×2 sub-boxes) on a lattice of --map-blocks³ blocks, beside rm_sdf_grid on the same 8·m + 1 points per axis —
     the parent's kernel on the same points; evaluations per second (729 per block against one per point) and the ratio
  B  dense against sparse where dense exists (--dense, points per axis): sdf_grid + extract_mesh against sdf_active_blocks +
     sdf_grid_blocks + extract_mesh_blocks, ms per step and bytes (tensors held by the route + the library's workspace, from the
     sizes the header states)
  C  sparse alone (--sparse, points per axis): blocks kept, vertices, quads, bytes, ms per step

Scenes: the headline Mandelbulb (12 iterations, iso 0.001) and c5's sponge (unit_mengersponge.json, 5 levels, iso 0.001), each over
its mesh_bounds.  HIP events around each step, a warm-up round, then --rounds interleaved rounds; median [min – max].

  python scripts/bench_sdf_blocks.py [--variant-lib PATH] [--map-blocks 64] [--dense 257,513,1025] [--sparse 2049,4097]
                                     [--rounds 5] [--scenes bulb,sponge] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant-lib", default=None, help="a second build of the library whose rm_sdf_blocks_select is timed as route V")
    ap.add_argument("--variant-name", default="9×3×2 sub-boxes, fifteen waves")
    ap.add_argument("--map-blocks", type=int, default=64)
    ap.add_argument("--dense", default="257,513,1025")
    ap.add_argument("--sparse", default="2049,4097")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scenes", default="bulb,sponge")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import numpy as np
    import torch
    import torch.nn.functional as F
    from raymarcher_amd import Renderer, Scene, abi, lib, mesh_bounds, scenes
    from raymarcher_amd._lib import SIGNATURES

    r = Renderer(0)
    dev = r.device
    L = lib()
    variant = None
    if args.variant_lib:
        variant = C.CDLL(os.path.abspath(args.variant_lib)).rm_sdf_blocks_select
        variant.restype, variant.argtypes = SIGNATURES["rm_sdf_blocks_select"]

    def timed(routes, rounds):
        for fn in routes.values():  # the warm-up round
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(rounds):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        return times

    def fmt(v):
        return f"{statistics.median(v):.3f} [{min(v):.3f} – {max(v):.3f}]"

    def spread(v):
        return (max(v) - min(v)) / statistics.median(v)

    def vec(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def table(name):
        if name == "bulb":
            return scenes.mandelbulb(64, 36), abi.default_settings(fractalIters=12), "the headline Mandelbulb, 12 iterations"
        if name == "sponge":
            t = Scene(path=os.path.join(SCENES, "simple", "unit_mengersponge.json")).tables(64, 36)
            return t, abi.default_settings(mengerLevels=5), "c5's sponge: unit_mengersponge.json, 5 levels"
        raise KeyError(name)

    def lattice(t, points):
        """origin, step and blocks per axis of the cubic lattice of `points` = 8·m + 1 points per axis over the table's bounds."""
        lo, hi = mesh_bounds(t)
        step = float((hi.astype(np.float64) - lo).max()) / (points - 1)
        return lo.astype(np.float32), (step,) * 3, [(points - 1) // 8] * 3

    def tensor_bytes(*ts):
        return sum(x.numel() * x.element_size() for x in ts if x is not None)

    iso = 0.001
    emit("# Block-sparse SDF lattices: rm_sdf_blocks_select, rm_sdf_grid_blocks, rm_sdf_mesh_blocks")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; HIP events around each step, a warm-up round, then {args.rounds} interleaved rounds; ms per "
         "step, median [min – max] over the rounds; iso 0.001; every lattice is cubic over the table's mesh_bounds.")
    for name in args.scenes.split(","):
        t, s, title = table(name)

        # ---- A: the lane mapping
        m = args.map_blocks
        n = 8 * m + 1
        origin, step, blocks = lattice(t, n)
        o3, s3 = vec(origin), vec(step)
        dist = r.sdf_grid(t, s, origin, step, (n, n, n))
        inside = (dist < iso).to(torch.float16).view(1, 1, n, n, n)
        want = (F.max_pool3d(inside, 9, 8).view(-1) > 0) & (F.max_pool3d(1 - inside, 9, 8).view(-1) > 0)  # linear order (bk·m + bj)·m + bi
        del inside
        cap = int(want.sum())
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        out_a, out_v = (torch.full((cap, 4), -1, dtype=torch.int32, device=dev) for _ in range(2))

        def select(fn, out):
            st = fn(t.objects, t.num_objects, C.byref(t.globals_), C.byref(s), o3, s3, m, m, m, iso, cap, ptr(out), ptr(count), r._stream())
            assert st == abi.RM_OK, st

        def grid():
            r.sdf_grid(t, s, origin, step, (n, n, n), ids=False)

        routes = {"G": grid, "S": lambda: select(L.rm_sdf_blocks_select, out_a)}
        select(L.rm_sdf_blocks_select, out_a)
        assert int(count.item()) == cap, f"{name}: {int(count.item())} blocks selected, {cap} active in rm_sdf_grid's lattice"
        lin = (out_a[:, 2].long() * m + out_a[:, 1]) * m + out_a[:, 0]
        assert torch.equal(lin, want.nonzero().view(-1)) and bool((out_a[:, 3] == 0).all()), f"{name}: the selected list differs"
        if variant:
            routes["V"] = lambda: select(variant, out_v)
            select(variant, out_v)
            assert int(count.item()) == cap and torch.equal(out_v, out_a), f"{name}: the lane mapping changes the list"
        times = timed(routes, args.rounds)
        emit()
        emit(f"## {title}")
        emit()
        emit(f"### A. Lane mapping on {m}³ blocks ({n}³ points); {cap} of {m ** 3} blocks are active; the lists agree with rm_sdf_grid's "
             "lattice" + (" and with each other" if variant else "") + ": yes")
        emit()
        emit("G = rm_sdf_grid without ids on the same lattice; S = rm_sdf_blocks_select, runs of 64 in x-fastest order, twelve waves"
             + (f"; V = rm_sdf_blocks_select, {args.variant_name}" if variant else "") + ".")
        emit()
        emit("| route | ms per call | evaluations | 10⁹ evaluations/s | rate against G |")
        emit("|---|---|---|---|---|")
        g_rate = n ** 3 / statistics.median(times["G"]) / 1e6
        for k, v in times.items():
            evals = n ** 3 if k == "G" else 729 * m ** 3
            rate = evals / statistics.median(v) / 1e6
            emit(f"| {k} | {fmt(v)} | {evals} | {rate:.2f} | {rate / g_rate:.3f} |")
        emit()
        emit("Spread over the rounds, (max − min) / median: " + ", ".join(f"{k} {spread(v) * 100:.1f} %" for k, v in times.items()) + ".")
        if variant:
            sm, vm, tol = statistics.median(times["S"]), statistics.median(times["V"]), max(spread(times["S"]), spread(times["V"]))
            verdict = "within this run's spread" if abs(vm / sm - 1) <= tol else ("runs of 64 are faster" if sm < vm else "sub-boxes are faster")
            emit(f"V / S = {vm / sm:.3f}, this run's spread {tol * 100:.1f} %: {verdict}.")
        del dist, out_a, out_v, want
        flush()

        # ---- B and C: dense against sparse, sparse alone
        def sparse_route(points):
            origin, step, blocks = lattice(t, points)
            state = {}

            def sel():
                state["bl"] = r.sdf_active_blocks(t, s, origin, step, blocks, iso)

            def grd():
                state["d"], state["i"] = r.sdf_grid_blocks(t, s, origin, step, blocks, state["bl"], ids=True)

            def msh():
                state["v"], state["q"], state["vo"], state["open"] = r.extract_mesh_blocks(state["d"], state["bl"], blocks, origin, step, iso, state["i"])

            def held():
                nb, nblocks = state["bl"].shape[0], blocks[0] * blocks[1] * blocks[2]
                ws = max(4 * nblocks + 8 * (nblocks // 1024 + 2), 4 * nblocks + 88 * nb)  # the header's workspace sizes
                return tensor_bytes(state["bl"], state["d"], state["i"], state["v"], state["q"], state["vo"]) + ws
            return {"select": sel, "grid_blocks": grd, "mesh_blocks": msh}, state, held

        def dense_route(points):
            origin, step, _ = lattice(t, points)
            state = {}

            def grd():
                state["d"], state["i"] = r.sdf_grid(t, s, origin, step, (points,) * 3, ids=True)

            def msh():
                state["v"], state["q"], state["vo"] = r.extract_mesh(state["d"], origin, step, iso, state["i"])

            def held():
                ws = 4 * (points - 1) ** 3 + 12 * (points ** 3 // 1024 + 1)  # rm_sdf_mesh's workspace
                return tensor_bytes(state["d"], state["i"], state["v"], state["q"], state["vo"]) + ws
            return {"sdf_grid": grd, "extract_mesh": msh}, state, held

        def report(label, steps, state, held, rounds, extra=""):
            times = timed(steps, rounds)
            total = [sum(times[k][i] for k in steps) for i in range(rounds)]
            row = f"| {label} | " + " + ".join(f"{k} {fmt(times[k])}" for k in steps) + f" | {fmt(total)} | {held() / 2 ** 20:.0f} MiB | {extra}"
            return row, state, statistics.median(total)

        emit()
        emit("### B. Dense against sparse (ms per step: every step includes its Python layer's counting call and read-back)")
        emit()
        emit("| lattice | steps, ms | total ms | bytes held | mesh |")
        emit("|---|---|---|---|---|")
        for points in [int(x) for x in args.dense.split(",") if x]:
            torch.cuda.empty_cache()
            L.rm_release_workspaces(None)
            steps, st, held = dense_route(points)
            row, st, d_ms = report(f"{points}³ dense", steps, st, held, args.rounds)
            dv, dq = st["v"], st["q"]
            emit(row + f"{len(dv)} vertices, {len(dq)} quads |")
            key = torch.sort(dv[:, 0].double() * 7 + dv[:, 1].double() * 13 + dv[:, 2].double() * 29).values  # an order-free checksum
            nvd, nqd = len(dv), len(dq)
            del st, dv, dq, steps, held
            torch.cuda.empty_cache()
            L.rm_release_workspaces(None)
            steps, st, held = sparse_route(points)
            row, st, s_ms = report(f"{points}³ sparse", steps, st, held, args.rounds)
            key2 = torch.sort(st["v"][:, 0].double() * 7 + st["v"][:, 1].double() * 13 + st["v"][:, 2].double() * 29).values
            assert (len(st["v"]), len(st["q"]), st["open"]) == (nvd, nqd, 0) and torch.equal(key, key2), f"{name} {points}: the meshes differ"
            emit(row + f"{len(st['v'])} vertices, {len(st['q'])} quads, {st['bl'].shape[0]} of {((points - 1) // 8) ** 3} blocks; equals the dense mesh: yes; "
                 f"sparse / dense = {s_ms / d_ms:.2f} |")
            del st, steps, held, key, key2
            flush()
        emit()
        emit("### C. Sparse alone")
        emit()
        emit("| lattice | steps, ms | total ms | bytes held | mesh |")
        emit("|---|---|---|---|---|")
        for points in [int(x) for x in args.sparse.split(",") if x]:
            torch.cuda.empty_cache()
            L.rm_release_workspaces(None)
            steps, st, held = sparse_route(points)
            try:
                row, st, _ = report(f"{points}³ sparse", steps, st, held, min(args.rounds, 3))
            except Exception as e:  # a list beyond RM_MAX_BLOCK_LIST: recorded, not hidden
                emit(f"| {points}³ sparse | not run: {type(e).__name__}: {e} | | | |")
                flush()
                continue
            emit(row + f"{len(st['v'])} vertices, {len(st['q'])} quads, {st['bl'].shape[0]} of {((points - 1) // 8) ** 3} blocks, "
                 f"{st['open']} open vertices |")
            del st, steps, held
            flush()
    flush()


if __name__ == "__main__":
    main()
