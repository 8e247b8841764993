#!/usr/bin/env python3
"""A/B of rm_render_supersampled against the only thing a caller could do before it: rm_render of the ss·W × ss·H frame (and a
reduction of their own, not timed here).  One process, one GPU, the variants interleaved round by round:

  A   rm_render_supersampled at 1920×1080 with ss = 2 and at 960×540 with ss = 4 (both 3840×2160 samples)
  B   rm_render of the 3840×2160 frame in raster tile order (rm_set_tile_order(0)): the same marches in the same tile order, but
      16 B stored per sample (32 B with BrightColor).  For c2's scene B is also pinned to 8×8 tiles and no light split, so that A
      and B run the same schedule.
  T   (c3 only) rm_render of the 3840×2160 frame with the library's defaults (measured tile order): what the raster order of A
      leaves on the table, the baseline of a heavy-first order for supersampled launches.

for the c3 (Mandelbulb) and c2 (directional_light_2.json, soft shadows + AO) scenes of bench.py, with and without BrightColor.
Every variant is timed as a host clock around `--launches` launches that end in a device synchronise, `--rounds` times; the table
gives the median and the range over the rounds.  The spread of B's own rounds is what a difference between A and B has to exceed.
Before timing, A is compared bit for bit with B reduced on the host by the tree of include/raymarcher_amd.h.

  python scripts/measure_supersample.py [--rounds 7] [--launches 100] [--out profiles/supersample.md]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def resolve(S, ss):
    import numpy as np
    level = 1
    while level < ss:
        a = S[:, 0::2] + S[:, 1::2]
        S = a[0::2] + a[1::2]
        level *= 2
    return S * np.float32(1 / ss ** 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, lib, scenes

    L = lib()
    r = Renderer(0)
    SW, SH = 3840, 2160
    configs = {
        "c3": (lambda W, H: scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12), False),
        "c2": (lambda W, H: Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H),
               abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1), True),
    }
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit(f"# rm_render_supersampled against rm_render of the {SW}×{SH} sample frame")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} launches per variant, host clock around "
         "launches + synchronise; ms per launch, median [min – max] over the rounds.")
    for name, (build, s, pin) in configs.items():
        big = build(SW, SH)
        for bright in (False, True):
            bufs = {}

            def out_for(key, shape):
                if key not in bufs:
                    bufs[key] = (torch.empty(shape, dtype=torch.float32, device=r.device),
                                 torch.empty(shape, dtype=torch.float32, device=r.device) if bright else None)
                return bufs[key]

            def run_a(ss):
                W, H = SW // ss, SH // ss
                o, b = out_for(("a", ss), (1, H, W, 4))
                r.render_supersampled(big, s, W, H, [big.camera], ss, out=o, out_bright=b)
                return o, b

            def run_b(tuned=False):
                o, b = out_for(("b", tuned), (SH, SW, 4))
                L.rm_set_tile_order(-1 if tuned else 0)
                if pin and not tuned:
                    L.rm_debug_set_tile_shape(3)
                    L.rm_debug_set_light_split(0)
                try:
                    r.render(big, s, SW, SH, out=o, out_bright=b)
                finally:
                    L.rm_set_tile_order(-1)
                    L.rm_debug_set_tile_shape(-1)
                    L.rm_debug_set_light_split(-1)
                return o, b

            variants = {"A ss=2 1920×1080": lambda: run_a(2), "A ss=4 960×540": lambda: run_a(4), "B raster 3840×2160": run_b}
            if name == "c3":
                variants["T tuned 3840×2160"] = lambda: run_b(tuned=True)
            # same results first (and every shape warmed up)
            Sb, Sbb = run_b()
            Sn = Sb.cpu().numpy()
            Sbn = Sbb.cpu().numpy() if bright else None
            for ss in (2, 4):
                o, b = run_a(ss)
                assert (o[0].cpu().numpy().view(np.uint32) == resolve(Sn, ss).view(np.uint32)).all(), f"{name} ss {ss} differs from B reduced"
                if bright:
                    assert (b[0].cpu().numpy().view(np.uint32) == resolve(Sbn, ss).view(np.uint32)).all(), f"{name} ss {ss} bright differs"
            for fn in variants.values():
                for _ in range(12 if name == "c3" else 30):  # the tuned variant settles its tile order; clocks ramp up
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    fn()  # the variant's own state (tile order of T) after the others ran
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.launches):
                        fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) / args.launches * 1e3)
            emit()
            emit(f"## {name}, {'fragColor + BrightColor' if bright else 'fragColor only'} (A bit-equal to B reduced on the host: yes)")
            emit()
            emit("| variant | ms per launch, median [min – max] | Msamples/s | bytes stored per output pixel at 1080p / 540p |")
            emit("|---|---|---|---|")
            per = 32 if bright else 16
            for k, v in times.items():
                med = statistics.median(v)
                stored = f"{per}" if k.startswith("A") else f"{4 * per} / {16 * per} (the ss·W × ss·H intermediate)"
                emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {SW * SH / med / 1e3:.0f} | {stored} |")
            b = times["B raster 3840×2160"]
            emit()
            emit(f"B's own spread over its rounds: {(max(b) - min(b)) / statistics.median(b) * 100:.1f} % of its median.  "
                 + "  ".join(f"{k}: {(statistics.median(v) / statistics.median(b) - 1) * 100:+.1f} % against B." for k, v in times.items()
                             if not k.startswith("B")))
    emit()
    emit(f"Peak extra memory of B: the {SW}×{SH} float4 intermediate, {SW * SH * 16 / 2**20:.0f} MiB for fragColor and as much again for "
         "BrightColor (k²·32 B per output pixel with both), plus a reduction pass over it that the library does not have.  A: none.")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
