#!/usr/bin/env python3
"""rm_shade_rays against rm_render_batch on a frame's own primary rays, and the price of incoherent rays.  One process, one GPU,
the routes of a case interleaved round by round.

  (i)  c3's frame (the Mandelbulb, 12 iterations, 3840×2160)
  (ii) c2's scene (directional_light_2.json, 1920×1080)
        B    rm_render_batch of that ONE frame with its bright output: the one-lane-per-pixel kernel of the class over raster 8×8
             tiles, no tuner and no tile-order feedback — the schedule rm_shade_rays has
        T    rm_shade_rays with bright, the frame's rays (rm_camera_rays) laid out so that each run of 64 is one 8×8 pixel tile:
             the render kernel's wave shape (tile_order)
        R    the rays in row-major order (a wave is 64 pixels of one row)
        S    the rays of T in a seeded shuffle: what incoherence costs (nothing here tries to remove it)

Before timing, the outputs are checked against each other: R holds B's bits pixel for pixel, colour and bright; T and S hold R's
rays' results in their own order.  Every route is timed with HIP events around `--launches` calls, `--rounds` times; the table gives
the median and the range over the rounds.  No ratio was fixed in advance: rm_shade_rays swaps primaryRay's divisions and normalise
for 32 bytes of load per ray, so the tiled case is expected near the batch kernel's time, and that is a prediction, not an assertion.

  python scripts/measure_shade.py [--rounds 5] [--launches 3] [--cases c3,c2] [--out profiles/shade_rays.md]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--cases", default="c3,c2")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, scenes, tile_order

    r = Renderer(0)  # raises without a GPU: there is nothing to measure elsewhere
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

    emit("# rm_shade_rays against rm_render_batch on a frame's own primary rays")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per call, median [min – max] over the rounds.  B = rm_render_batch of the one frame, colour and bright (raster 8×8 "
         "tiles, no tuner); T = rm_shade_rays, colour and bright, on the frame's rays in 8×8-tile order; R = the rays in row-major "
         "order; S = a seeded shuffle of T's rays.")
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
        far = t.camera.initialFar
        rays_r = torch.from_numpy(camera_rays(t.camera, W, H)).to(dev)
        tile_t = torch.from_numpy(tile_order(W, H)).to(dev)
        rays_t = rays_r[tile_t].contiguous()
        perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
        rays_s = rays_t[perm].contiguous()
        frame = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
        frame_b = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
        out = {k: (torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev))
               for k in ("T", "R", "S")}
        routes = {
            "B": lambda: r.render_batch(t, s, W, H, [t.camera], out=frame, out_bright=frame_b),
            "T": lambda: r.shade_rays(t, s, rays_t, far=far, out=out["T"][0], out_bright=out["T"][1]),
            "R": lambda: r.shade_rays(t, s, rays_r, far=far, out=out["R"][0], out_bright=out["R"][1]),
            "S": lambda: r.shade_rays(t, s, rays_s, far=far, out=out["S"][0], out_bright=out["S"][1]),
        }
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        for k in (0, 1):
            assert same(out["R"][k], (frame, frame_b)[k].view(n, 4)), f"{name}: rm_shade_rays on the camera's rays differs from rm_render_batch"
            assert same(out["T"][k], out["R"][k][tile_t]) and same(out["S"][k], out["T"][k][perm]), f"{name}: a ray's result depends on its neighbours"
        times = timed(routes)
        b_med = statistics.median(times["B"])
        hit = float((frame[..., 0:3] != frame[0, 0, 0, 0:3]).any(dim=-1).float().mean()) * 100
        emit()
        emit(f"## {title}: {n} rays, {hit:.1f} % of the pixels differ from the corner's background (outputs agree: yes)")
        emit()
        emit("| route | ms per call, median [min – max] | Mrays/s | ratio to B |")
        emit("|---|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {n / med / 1e3:.0f} | {med / b_med:.3f} |")
        emit()
        emit("Spread over the rounds, (max − min) / median: " +
             ", ".join(f"{k} {(max(v) - min(v)) / statistics.median(v) * 100:.1f} %" for k, v in times.items()) + ".")
        del frame, frame_b, out, rays_r, rays_t, rays_s
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
