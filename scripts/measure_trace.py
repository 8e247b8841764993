#!/usr/bin/env python3
"""rm_trace_rays against rm_render_gbuffer on a frame's own primary rays, and the price of incoherent rays.  One process, one GPU,
the routes of a case interleaved round by round.

  (i)  c3's frame (the Mandelbulb, 12 iterations, 3840×2160)
  (ii) c2's scene (directional_light_2.json, 1920×1080)
        G    rm_render_gbuffer with d_position (its kernels are byte-identical to the build before rm_trace_rays: DESIGN §6.12)
        T    rm_trace_rays, closest, the frame's rays laid out so that each run of 64 is one 8×8 pixel tile: the G-buffer's wave shape
        TN   the same with RM_TRACE_NO_NORMAL
        TO   the same rays, RM_TRACE_OCCLUSION
        R    closest, the rays in row-major order (a wave is 64 pixels of one row)
        S    closest, the rays of T in a seeded shuffle: what incoherence costs (nothing here tries to remove it)

Before timing, the outputs are checked against each other: T holds G's bits pixel for pixel, R and S hold T's rays' results in
their own order, TN holds T's ids and t.  Every route is timed with HIP events around `--launches` calls, `--rounds` times; the
table gives the median and the range over the rounds.  No figure was fixed in advance.

The file it writes starts with a section that needs no GPU: the accuracy of the specification's normals on lone spheres, which
tests/test_trace_spec.py asserts at twice the figures measured here.

  python scripts/measure_trace.py [--rounds 5] [--launches 3] [--cases c3,c2] [--no-gpu] [--out profiles/trace_rays.md]"""
import argparse
import os
import platform
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def spec_section(emit):
    """The specification (tests/trace_spec/rm_trace_spec.c) on lone spheres against the analytic intersection, on the CPU."""
    import numpy as np
    import helpers as h
    import test_trace_spec as S
    import trace_helpers as T
    from raymarcher_amd import abi

    emit("## The specification on lone spheres (CPU, no GPU involved)")
    emit()
    emit(f"tests/trace_spec/rm_trace_spec.c, built with oracle/Makefile's flags, on {platform.machine()} ({platform.system()}); binary32 "
         "throughout, so the figures are the same on any IEEE machine.  RM_SPHERE of radius R = 0.5·scale, 20 000 seeded rays per scale "
         "from distance 3 to 8 with impact parameter <= 0.9 R (the seeds and centres of tests/test_trace_spec.py), no bump.  "
         "The normal is compared with the radial direction through the returned position; its error is binary32 cancellation in "
         "getNormal's 5e-4 taps and grows as the sphere shrinks.  The test asserts t and position at the derived bounds "
         "(4·SURFACE_DIST + 1e-5·t, 2·SURFACE_DIST + 1e-5) and the normal at twice the figure in the last column.")
    emit()
    emit("| scale | centre | max abs(t − t_analytic) / SURFACE_DIST | max abs(abs(p − c) − R) | max abs(normal − radial), any component |")
    emit("|---|---|---|---|---|")
    for scale, centre, seed, _ in S.SPHERES:
        R, c = 0.5 * scale, np.array(centre, dtype=np.float64)
        objs, n = T.sphere_table(scale, centre)
        rays, o, d = T.sphere_rays(np.random.default_rng(seed), 20000, centre, R, 0.0, 0.9)
        hits = T.spec_trace(objs, n, h.make_globals(), abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND), rays)
        oc = o - c
        a, b, cc = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - R * R
        t = (-b - np.sqrt(b * b - a * cc)) / a
        p = hits[:, 4:7].astype(np.float64)
        rad = (p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
        emit(f"| {scale} | {centre} | {np.abs(hits[:, 3] - t).max() / S.SURFACE_DIST:.3f} | "
             f"{np.abs(np.linalg.norm(p - c, axis=1) - R).max():.4e} | {np.abs(hits[:, 0:3] - rad).max():.4e} |")
    emit()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--cases", default="c3,c2")
    ap.add_argument("--no-gpu", action="store_true", help="write the CPU section only and say that no GPU run is recorded")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def finish():
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    emit("# rm_trace_rays: the specification's accuracy, and the kernel against rm_render_gbuffer")
    emit()
    spec_section(emit)
    emit("## rm_trace_rays against rm_render_gbuffer on a frame's own primary rays")
    emit()
    if args.no_gpu:
        emit("NOT MEASURED YET: no GPU run of scripts/measure_trace.py is recorded here.")
        finish()
        return

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, scenes

    r = Renderer(0)
    dev = r.device

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

    def same(x, y):
        return bool((x.contiguous().view(torch.int32) == y.contiguous().view(torch.int32)).all())

    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per call, median [min – max] over the rounds.  G = rm_render_gbuffer with position (its code object is "
         "byte-identical to the build before this entry point existed); T / TN / TO = rm_trace_rays closest / without normals / "
         "occlusion on the frame's rays in 8×8-tile order; R = closest in row-major order; S = closest on a seeded shuffle of T's rays.")
    for name in args.cases.split(","):
        if name == "c3":
            W, H = 3840, 2160
            t, s = scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12)
            title = f"(i) c3: Mandelbulb, 12 iterations, {W}×{H}"
        elif name == "c2":
            W, H = 1920, 1080
            t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
            s = abi.default_settings()
            title = f"(ii) c2: directional_light_2.json, {W}×{H}"
        else:
            raise KeyError(name)
        n = W * H
        # pixel index of every ray in 8×8-tile order (partial tiles at the frame's edges keep their pixels, in tile order)
        ty, tx, ly, lx = np.meshgrid(np.arange((H + 7) // 8), np.arange((W + 7) // 8), np.arange(8), np.arange(8), indexing="ij")
        px, py = (tx * 8 + lx).reshape(-1), (ty * 8 + ly).reshape(-1)
        keep = (px < W) & (py < H)
        tile = (py[keep] * W + px[keep]).astype(np.int64)
        row_rays = camera_rays(t.camera, W, H)
        rays_r = torch.from_numpy(row_rays).to(dev)
        tile_t = torch.from_numpy(tile).to(dev)
        rays_t = rays_r[tile_t].contiguous()
        perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
        rays_s = rays_t[perm].contiguous()
        nd = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
        ids = torch.empty((1, H, W), dtype=torch.int32, device=dev)
        pos = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
        out = {k: torch.empty((n, 8), dtype=torch.float32, device=dev) for k in ("T", "TN", "TO", "R", "S")}
        routes = {
            "G": lambda: r.render_gbuffer(t, s, W, H, out_normal_depth=nd, out_object_id=ids, out_position=pos),
            "T": lambda: r.trace_rays(t, s, rays_t, out=out["T"]),
            "TN": lambda: r.trace_rays(t, s, rays_t, normals=False, out=out["TN"]),
            "TO": lambda: r.trace_rays(t, s, rays_t, mode="occlusion", out=out["TO"]),
            "R": lambda: r.trace_rays(t, s, rays_r, out=out["R"]),
            "S": lambda: r.trace_rays(t, s, rays_s, out=out["S"]),
        }
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        g_rows = torch.cat([nd.view(n, 4), pos.view(n, 4)[:, 0:3], ids.view(n, 1).view(torch.float32)], dim=1)
        assert same(out["R"], g_rows), f"{name}: rm_trace_rays on the camera's rays differs from rm_render_gbuffer"
        assert same(out["T"], out["R"][tile_t]) and same(out["S"], out["T"][perm]), f"{name}: a ray's result depends on its neighbours"
        assert same(out["TN"][:, 3], out["T"][:, 3]) and same(out["TN"][:, 7], out["T"][:, 7]), f"{name}: NO_NORMAL changes id or t"
        times = timed(routes)
        g_med = statistics.median(times["G"])
        hit = float((ids >= 0).float().mean()) * 100
        emit()
        emit(f"## {title}: {n} rays, {hit:.1f} % hit (outputs agree: yes)")
        emit()
        emit("| route | ms per call, median [min – max] | Mrays/s | ratio to G |")
        emit("|---|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {n / med / 1e3:.0f} | {med / g_med:.3f} |")
        emit()
        emit("Spread over the rounds, (max − min) / median: " +
             ", ".join(f"{k} {(max(v) - min(v)) / statistics.median(v) * 100:.1f} %" for k, v in times.items()) + ".")
        del nd, ids, pos, out, rays_r, rays_t, rays_s
    finish()


if __name__ == "__main__":
    main()
