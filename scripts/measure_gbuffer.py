#!/usr/bin/env python3
"""rm_render_gbuffer against the colour render of the same frames.  One process, one GPU, the routes of a case interleaved round by
round.

  (i)   c3's frame (the Mandelbulb, 12 iterations, 3840×2160)             one frame per call
  (ii)  c2's scene (directional_light_2.json, soft shadows + AO, 1920×1080) one frame per call
  (iii) c1's scene (unit_sphere.json, 64 steps), 64 frames at 256×256     one call
        G    rm_render_gbuffer, normalDepth + objectId
        GP   rm_render_gbuffer with d_position too
        C    rm_render_batch of the same cameras, fragColor alone (the colour render: march, normal, shading)

Before timing, the outputs are checked against each other: G's two outputs are GP's bit for bit, a pixel has objectId >= 0 exactly
where its position flag is 1 and its depth is below initialFar, and (iii)'s frame 0 is the one-frame call's.  Every route is timed
with HIP events around `--launches` calls, `--rounds` times; the table gives the median and the range over the rounds.  No figure
was fixed in advance: the table records ms per frame and the ratio to the colour render.

  python scripts/measure_gbuffer.py [--rounds 7] [--launches 10] [--cases c3,c2,c1] [--out profiles/gbuffer.md]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--cases", default="c3,c2,c1")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()

    import torch
    from raymarcher_amd import Renderer, Scene, abi, scenes

    r = Renderer(0)
    dev = r.device
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def timed(variants):
        for fn in variants.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / args.launches)
        return times

    def bit_equal(x, y):
        return bool((x.view(torch.int32) == y.view(torch.int32)).all())

    emit("# rm_render_gbuffer against the colour render of the same frames")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per frame, median [min – max] over the rounds.  G = normalDepth + objectId, GP = G + position, C = rm_render_batch "
         "of the same cameras (fragColor alone).")
    for name in args.cases.split(","):
        if name == "c3":
            W, H, n = 3840, 2160, 1
            t, s = scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12)
            title = f"(i) c3: Mandelbulb, 12 iterations, {W}×{H}"
        elif name == "c2":
            W, H, n = 1920, 1080, 1
            t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
            s = abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)
            title = f"(ii) c2: directional_light_2.json, soft shadows + AO, {W}×{H}"
        elif name == "c1":
            W, H, n = 256, 256, 64
            t = Scene(path=os.path.join(SCENES, "simple", "unit_sphere.json")).tables(W, H)
            s = abi.default_settings(maxSteps=64)
            title = f"(iii) c1: unit_sphere.json, 64 steps, {n} frames of {W}×{H} in one call"
        else:
            raise KeyError(name)
        cams = [t.camera] * n
        nd, ndp = (torch.empty((n, H, W, 4), dtype=torch.float32, device=dev) for _ in range(2))
        ids, idsp = (torch.empty((n, H, W), dtype=torch.int32, device=dev) for _ in range(2))
        pos, col = (torch.empty((n, H, W, 4), dtype=torch.float32, device=dev) for _ in range(2))

        def run_g():
            r.render_gbuffer(t, s, W, H, cameras=cams, out_normal_depth=nd, out_object_id=ids)

        def run_gp():
            r.render_gbuffer(t, s, W, H, cameras=cams, out_normal_depth=ndp, out_object_id=idsp, out_position=pos)

        def run_c():
            r.render_batch(t, s, W, H, cams, out=col)

        run_g()
        run_gp()
        run_c()
        torch.cuda.synchronize()
        assert bit_equal(nd, ndp) and bool((ids == idsp).all()), f"{name}: the outputs change with d_position"
        hit = ids >= 0
        assert bool(((pos[..., 3] == 1.0) == hit).all()) and bool(((nd[..., 3] < t.camera.initialFar) == hit).all()), f"{name}: hit flags disagree"
        if n > 1:
            one = r.render_gbuffer(t, s, W, H, cameras=cams[:1])
            assert bit_equal(one[0][0], nd[0]) and bool((one[1][0] == ids[0]).all()), f"{name}: frame 0 differs from a one-frame call"
        times = timed({"G": run_g, "GP": run_gp, "C": run_c})
        c_med = statistics.median(times["C"])
        emit()
        emit(f"## {title}: {float(hit.float().mean()) * 100:.1f} % hit pixels (outputs agree: yes)")
        emit()
        emit("| route | ms per frame, median [min – max] | Mpixels/s | ratio to C |")
        emit("|---|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            emit(f"| {k} | {med / n:.4f} [{min(v) / n:.4f} – {max(v) / n:.4f}] | {n * W * H / med / 1e3:.0f} | {med / c_med:.3f} |")
        emit()
        emit("Spread over the rounds, (max − min) / median: " +
             ", ".join(f"{k} {(max(v) - min(v)) / statistics.median(v) * 100:.1f} %" for k, v in times.items()) + ".")
        del nd, ndp, ids, idsp, pos, col
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
