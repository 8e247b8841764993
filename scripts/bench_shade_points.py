#!/usr/bin/env python3
"""rm_shade_points against rm_shade_rays on the same surface points, and bake_mesh beside rm_sdf_grid.  One process, one GPU, the
routes of a case interleaved round by round.

The headline camera's rays (in 8×8 tile order, as a frame's waves hold them) are traced once; the rays that hit, and their hit
positions, are the workload of
  (i)  the headline Mandelbulb (12 iterations, 3 directional lights, hard shadows, Perlin bump: the shadow pool's case)
  (ii) c2's five-primitive table (directional_light_2.json, soft shadows + ambient occlusion)
        R    rm_shade_rays on the hit rays: the primary march, then the shading
        P    rm_shade_points, d_rgba alone, on those rays' hit positions with view = dir, in the same order: the same shading, no march
        Q    P of --variant-lib (a build of rm_points.hip with -DRM_POINTS_POOL=0: getPhong's per-lane queue), when given
        Ps   rm_shade_points, d_surface alone          Psa  d_surface and d_ao          Pall  all three outputs
  (iii) bake_mesh's steps on the Mandelbulb's --n³ lattice: G rm_sdf_grid, M rm_sdf_mesh (counting + emitting), B rm_shade_points on
        the mesh's vertices with every output and two projection steps

Before timing: P's colour equals R's in every bit on c2 (on the bulb the orbit trap of a hit point is not the march's, so there P's
normal is checked against rm_trace_rays' instead), Q's colour equals P's, and every mode of rm_shade_points holds the same bits.
Every route is timed with HIP events around `--launches` calls, `--rounds` times, after a warm-up round; the table gives the median
and the range over the rounds.  The verdict compares P with R per element: slower by more than the spread this run itself shows (the
larger of the two routes' (max − min) / median) is a failure and the exit status is 1.  No figure was fixed in advance.

  python scripts/bench_shade_points.py [--size 1920x1080] [--n 256] [--rounds 7] [--launches 5] [--cases bulb,c2,bake]
                                       [--variant-lib PATH] [--ply FILE] [--out FILE]"""
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
    ap.add_argument("--size", default="1920x1080", help="the frame whose primary rays are traced")
    ap.add_argument("--n", type=int, default=256, help="lattice points along the longest side for the bake")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--cases", default="bulb,c2,bake")
    ap.add_argument("--variant-lib", default=None, help="a second build of the library whose rm_shade_points is timed as route Q")
    ap.add_argument("--ply", default=None, help="write the baked Mandelbulb (colours and normals) to this PLY file")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, lib, scenes, tile_order, write_ply_ex
    from raymarcher_amd._lib import SIGNATURES

    r = Renderer(0)
    dev = r.device
    L = lib()
    variant = None
    if args.variant_lib:
        variant = C.CDLL(os.path.abspath(args.variant_lib)).rm_shade_points
        variant.restype, variant.argtypes = SIGNATURES["rm_shade_points"]

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

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def table(times, per, unit):
        emit(f"| route | ms per call, median [min – max] | ns per {unit} |")
        emit("|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            emit(f"| {k} | {med:.4f} [{min(v):.4f} – {max(v):.4f}] | {med * 1e6 / per[k]:.2f} |")
        spread = {k: (max(v) - min(v)) / statistics.median(v) for k, v in times.items()}
        emit()
        emit("Spread over the rounds, (max − min) / median: " + ", ".join(f"{k} {v * 100:.1f} %" for k, v in spread.items()) + ".")
        return spread

    def scene_of(name):
        if name == "c2":
            return (Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H),
                    abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1))
        return scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12)

    emit("# rm_shade_points against rm_shade_rays on the same surface points")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; the primary rays of a {W}×{H} frame in 8×8 tile order, traced once; a warm-up round, then "
         f"{args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the calls; ms per call, median [min – "
         "max] over the rounds.  R = rm_shade_rays on the rays that hit; P = rm_shade_points (d_rgba alone) on their hit positions with "
         "view = dir" + ("; Q = P with getPhong's per-lane queue in place of the shadow pool" if variant else "") +
         "; Ps / Psa / Pall = rm_shade_points with d_surface alone, with d_ao too, with all three outputs.")
    failed = False
    for name in [c for c in args.cases.split(",") if c in ("bulb", "c2")]:
        t, s = scene_of(name)
        title = "(ii) c2: directional_light_2.json, soft shadows + ambient occlusion" if name == "c2" else \
            "(i) the headline Mandelbulb, 12 iterations, hard shadows from three directional lights"
        far = t.camera.initialFar
        rays = torch.from_numpy(camera_rays(t.camera, W, H)[tile_order(W, H)]).to(dev)
        normal, _, position, oid = r.trace_rays(t, s, rays)
        hit = oid >= 0
        rays = rays[hit].contiguous()
        n = rays.shape[0]
        assert n >= 100000, f"{name}: {n} hits: take a larger --size"
        pts = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        pts[:, 0:3] = position[hit]
        view = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        view[:, 0:3] = rays[:, 4:7]
        trace_normal = normal[hit].contiguous()
        res, _keep = r._resources(t)
        ps = abi.RmPointsSettings(far, 0.001, float("inf"), 0)
        col_r = torch.empty((n, 4), dtype=torch.float32, device=dev)
        col = {k: torch.empty((n, 4), dtype=torch.float32, device=dev) for k in ("P", "Q", "Pall")}
        sf = {k: torch.empty((n, 8), dtype=torch.float32, device=dev) for k in ("Ps", "Psa", "Pall")}
        ao = {k: torch.empty((n,), dtype=torch.float32, device=dev) for k in ("Psa", "Pall")}

        def points(fn, k):
            st = fn(ptr(pts), ptr(view), n, C.byref(ps), t.objects, t.num_objects, t.lights, t.num_lights, C.byref(t.globals_), C.byref(s),
                    C.byref(res), ptr(sf.get(k)), ptr(ao.get(k)), ptr(col.get(k)), r._stream())
            assert st == abi.RM_OK, st

        routes = {"R": lambda: r.shade_rays(t, s, rays, far=far, out=col_r), "P": lambda: points(L.rm_shade_points, "P")}
        if variant:
            routes["Q"] = lambda: points(variant, "Q")
        for k in ("Ps", "Psa", "Pall"):
            routes[k] = lambda k=k: points(L.rm_shade_points, k)
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        assert same(col["Pall"], col["P"]) and same(sf["Psa"], sf["Ps"]) and same(sf["Pall"], sf["Ps"]) and same(ao["Pall"], ao["Psa"]), \
            f"{name}: an output changes with the others"
        if variant:
            assert same(col["Q"], col["P"]), f"{name}: the queue and the pool differ"
        ids_same = bool((sf["Ps"][:, 7].view(torch.int32) == oid[hit]).all())
        if name == "c2":
            assert ids_same and same(col["P"], col_r), "c2: P's colour differs from R's"
            checked = "P's colour equals R's in every bit"
        else:
            assert ids_same and same(sf["Ps"][:, 0:3], trace_normal), "bulb: P's normal differs from rm_trace_rays'"
            checked = "P's normal equals rm_trace_rays' in every bit (the orbit trap of the hit point is not the march's: the colours differ)"
        times = timed(routes)
        emit()
        emit(f"## {title}: {n} of {W * H} rays hit; {checked}; every mode of rm_shade_points holds the same bits"
             + ("; Q's colour equals P's" if variant else ""))
        emit()
        spread = table(times, {k: n for k in times}, "ray or point")
        r_med, p_med, tol = statistics.median(times["R"]), statistics.median(times["P"]), max(spread["R"], spread["P"])
        ok = p_med <= r_med * (1.0 + tol)
        failed = failed or not ok
        emit(f"Verdict: P / R = {p_med / r_med:.3f} per element, this run's spread {tol * 100:.1f} %: " +
             ("rm_shade_points is not slower than rm_shade_rays." if ok else "rm_shade_points is SLOWER than rm_shade_rays."))
        if variant:
            emit(f"Queue against pool: Q / P = {statistics.median(times['Q']) / p_med:.3f} "
                 f"(spread {max(spread['Q'], spread['P']) * 100:.1f} %).")
        del rays, pts, view, col, sf, ao, col_r
    if "bake" in args.cases.split(","):
        t, s = scene_of("bulb")
        verts, quads, _vobj, step = r._scene_mesh(t, s, args.n, 0.001, None)
        nv, nq = verts.shape[0], quads.shape[0]
        from raymarcher_amd import mesh_bounds
        lo, hi = (np.asarray(b, dtype=np.float64) for b in mesh_bounds(t))
        dims = [min(args.n, int(np.ceil(sd / step)) + 3) for sd in hi - lo]
        origin = lo - step
        move = 0.5 * step * 3.0 ** 0.5
        routes = {"G": lambda: r.sdf_grid(t, s, origin, (step,) * 3, dims, ids=True),
                  "B": lambda: r.shade_points(t, s, verts, colour=True, ao=True, project=2, iso=0.001, max_move=move)}
        dist, obj = r.sdf_grid(t, s, origin, (step,) * 3, dims, ids=True)
        routes["M"] = lambda: r.extract_mesh(dist, origin, (step,) * 3, 0.001, obj)
        times = timed(routes)
        emit()
        emit(f"## (iii) bake_mesh of the headline Mandelbulb on a {dims[0]}×{dims[1]}×{dims[2]} lattice: {nv} vertices, {nq} quads")
        emit()
        table(times, {"G": dims[0] * dims[1] * dims[2], "M": dims[0] * dims[1] * dims[2], "B": max(nv, 1)}, "lattice point (G, M) or vertex (B)")
        emit()
        emit("M includes extract_mesh's read-back of the two counts between its counting and its emitting call.")
        if args.ply:
            bv, bq, _o, bn, _ao, rgb = r.bake_mesh(t, s, args.n)
            write_ply_ex(args.ply, bv, bq, colours=rgb, normals=bn)
            emit(f"The baked mesh as a PLY with colours and normals: {bv.shape[0]} vertices, {bq.shape[0]} quads, "
                 f"{os.path.getsize(args.ply)} bytes.")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
