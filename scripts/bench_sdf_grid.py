#!/usr/bin/env python3
"""rm_sdf_grid against the only other way to get its values, rm_probe_sdscene over the same points in x-fastest order, and the time
of rm_sdf_mesh beside it.  One process, one GPU, the routes of a case interleaved round by round.

  (i)  the headline Mandelbulb (12 iterations) on a 256³ lattice over its bounds (mesh_bounds)
  (ii) c2's five-primitive table (directional_light_2.json) on a 256³ lattice over its bounds
        P    rm_probe_sdscene: reads 12 B per point, writes 16 B per point, point i on lane i % 64 — 64 neighbours along x
        G    rm_sdf_grid with d_objectId (4 + 4 B per point written), the library's brick shape
        Gd   rm_sdf_grid without d_objectId
        V    rm_sdf_grid of --variant-lib (a build with the other brick shape, -DRM_SDF_BRICK=1: 8×8×1), when given
        Mc   rm_sdf_mesh, the counting call, on G's lattice at iso 0.001
        Me   rm_sdf_mesh, the emitting call with exact capacities

Before timing, G's and V's lattices are checked against P's components 0 and 1 in every bit.  Every route is timed with HIP events
around `--launches` calls, `--rounds` times, after a warm-up round; the table gives the median and the range over the rounds.  The
verdict compares G with P: slower by more than the spread this run itself shows (the larger of the two routes' (max − min) / median)
is a failure and the exit status is 1.  No figure was fixed in advance.

  python scripts/bench_sdf_grid.py [--n 256] [--rounds 7] [--launches 3] [--cases bulb,c2] [--variant-lib PATH] [--out FILE]"""
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
    ap.add_argument("--n", type=int, default=256, help="lattice points per axis")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--cases", default="bulb,c2")
    ap.add_argument("--variant-lib", default=None, help="a second build of the library whose rm_sdf_grid is timed as route V")
    ap.add_argument("--variant-name", default="8×8×1 bricks")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, lib, mesh_bounds, scenes
    from raymarcher_amd._lib import SIGNATURES

    r = Renderer(0)
    dev = r.device
    L = lib()
    variant = None
    if args.variant_lib:
        variant = C.CDLL(os.path.abspath(args.variant_lib)).rm_sdf_grid
        variant.restype, variant.argtypes = SIGNATURES["rm_sdf_grid"]

    def timed(routes):
        for fn in routes.values():  # the warm-up round
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.launches)
        return times

    def same(x, y):
        return bool((x.contiguous().view(torch.int32) == y.contiguous().view(torch.int32)).all())

    def vec(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    n = args.n
    emit("# rm_sdf_grid against rm_probe_sdscene, and rm_sdf_mesh beside it")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; a {n}³ lattice ({n ** 3} points) over the table's bounds; a warm-up round, then {args.rounds} "
         f"interleaved rounds of {args.launches} calls per route, HIP events around the calls; ms per call, median [min – max] over the "
         "rounds.  P = rm_probe_sdscene over the same points in x-fastest order; G / Gd = rm_sdf_grid with / without d_objectId"
         + (f"; V = rm_sdf_grid with {args.variant_name}" if variant else "") + "; Mc / Me = rm_sdf_mesh counting / emitting at iso 0.001.")
    failed = False
    for name in args.cases.split(","):
        if name == "bulb":
            t, s = scenes.mandelbulb(64, 36), abi.default_settings(fractalIters=12)
            title = "(i) the headline Mandelbulb, 12 iterations"
        elif name == "c2":
            t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(64, 36)
            s = abi.default_settings()
            title = "(ii) c2: directional_light_2.json, five primitives"
        else:
            raise KeyError(name)
        lo, hi = mesh_bounds(t)
        origin = lo.astype(np.float32)
        step = ((hi.astype(np.float64) - lo) / (n - 1)).astype(np.float32)
        ax = [origin[a] + np.arange(n, dtype=np.float32) * step[a] for a in range(3)]
        zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        pts = torch.from_numpy(np.ascontiguousarray(np.stack([xx, yy, zz], axis=-1).reshape(-1, 3))).to(dev)
        del zz, yy, xx
        probe = torch.empty((n ** 3, 4), dtype=torch.float32, device=dev)
        dist, ids = (torch.empty((n, n, n), dtype=dt, device=dev) for dt in (torch.float32, torch.int32))
        dist_alone, dist_v, ids_v = torch.empty_like(dist), torch.empty_like(dist), torch.empty_like(ids)
        o3, s3 = vec(origin), vec(step)

        def grid(fn, d, i):
            st = fn(t.objects, t.num_objects, C.byref(t.globals_), C.byref(s), o3, s3, n, n, n, ptr(d), ptr(i), r._stream())
            assert st == abi.RM_OK, st

        routes = {"P": lambda: r.probe_sdscene(t, s, pts, out=probe),
                  "G": lambda: grid(L.rm_sdf_grid, dist, ids),
                  "Gd": lambda: grid(L.rm_sdf_grid, dist_alone, None)}
        if variant:
            routes["V"] = lambda: grid(variant, dist_v, ids_v)
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        assert same(dist.view(-1), probe[:, 0]) and bool((ids.view(-1) == probe[:, 1].to(torch.int32)).all()), f"{name}: G differs from P"
        assert same(dist_alone, dist), f"{name}: d_dist changes without d_objectId"
        if variant:
            assert same(dist_v, dist) and bool((ids_v == ids).all()), f"{name}: the brick shape changes a bit"
        # the mesh of G's lattice: counts first, then exact capacities
        counts = torch.zeros(2, dtype=torch.int32, device=dev)

        def mesh(mv, mq, v, vo, q):
            st = L.rm_sdf_mesh(ptr(dist), ptr(ids), n, n, n, o3, s3, 0.001, mv, mq, ptr(v), ptr(vo), ptr(q), ptr(counts), r._stream())
            assert st == abi.RM_OK, st

        mesh(0, 0, None, None, None)
        nv, nq = (int(x) for x in counts.cpu().numpy().view(np.uint32))
        verts = torch.empty((max(nv, 1), 4), dtype=torch.float32, device=dev)
        vobj = torch.empty((max(nv, 1),), dtype=torch.int32, device=dev)
        quads = torch.empty((max(nq, 1), 4), dtype=torch.int32, device=dev)
        routes["Mc"] = lambda: mesh(0, 0, None, None, None)
        routes["Me"] = lambda: mesh(nv, nq, verts if nv else None, vobj if nv else None, quads if nq else None)
        times = timed(routes)
        p_med = statistics.median(times["P"])
        emit()
        emit(f"## {title}: bounds {np.round(lo, 4).tolist()} … {np.round(hi, 4).tolist()}; outputs agree in every bit: yes; "
             f"the mesh at iso 0.001 has {nv} vertices and {nq} quads")
        emit()
        emit("| route | ms per call, median [min – max] | 10⁹ evaluations/s | ratio to P |")
        emit("|---|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            rate = f"{n ** 3 / med / 1e6:.2f}" if k in ("P", "G", "Gd", "V") else "—"
            emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {rate} | {med / p_med:.3f} |")
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in times.items()}
        emit()
        emit("Spread over the rounds, (max − min) / median: " + ", ".join(f"{k} {v * 100:.1f} %" for k, v in spread.items()) + ".")
        g_med, tol = statistics.median(times["G"]), max(spread["G"], spread["P"])
        ok = g_med <= p_med * (1.0 + tol)
        failed = failed or not ok
        emit(f"Verdict: G / P = {g_med / p_med:.3f}, this run's spread {tol * 100:.1f} %: " +
             ("rm_sdf_grid is not slower than the probe path." if ok else "rm_sdf_grid is SLOWER than the probe path."))
        del pts, probe, dist, ids, dist_alone, dist_v, ids_v, verts, vobj, quads
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
