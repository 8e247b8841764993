#!/usr/bin/env python3
"""rm_render_adaptive against the two entry points it is composed of.  One process, one GPU, the variants interleaved round by round:

  B1   rm_render_batch of one W×H frame                  (what an unflagged pixel costs)
  Bss  rm_render_supersampled of the same frame at ss    (what refining every pixel costs)
  A    rm_render_adaptive at ss and thresholds 0.05 / 0.1 / 0.25 / +inf / −1, with d_mask and d_refined
  C    a device-to-device copy of 21 B per pixel (what the classify pass moves), E: two launches of a one-element fill (the
       closest thing to an empty kernel the host has), both on the same stream

for the c3 (Mandelbulb) and c2 (directional_light_2.json, soft shadows + AO) pictures of bench.py at 1920×1080, ss = 2 and 4.
Every variant is timed as a host clock around `--launches` launches that end in a device synchronise, `--rounds` times; the tables
give the median and the range over the rounds.  The spread of a baseline's own rounds (max − min) is the resolution of a comparison
with it.  Before timing, A is compared bit for bit with the composite of B1 and Bss by the definition of include/raymarcher_amd.h.

  python scripts/measure_adaptive.py [--rounds 7] [--launches 50] [--out profiles/adaptive.md]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
THRESHOLDS = [0.05, 0.1, 0.25, float("inf"), -1.0]


def contrast_mask(F, thr):
    import numpy as np
    c = F[..., :3]
    dx = (~(np.abs(c[:, 1:] - c[:, :-1]) <= np.float32(thr))).any(-1)
    dy = (~(np.abs(c[1:] - c[:-1]) <= np.float32(thr))).any(-1)
    m = np.zeros(F.shape[:2], dtype=bool)
    m[:, 1:] |= dx
    m[:, :-1] |= dx
    m[1:] |= dy
    m[:-1] |= dy
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, scenes

    r = Renderer(0)
    W, H = args.width, args.height
    configs = {
        "c3": (scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12)),
        "c2": (Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H),
               abi.default_settings(enableSoftShadow=1, enableAmbientOcclusion=1)),
    }
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    def fmt(v):
        return f"{statistics.median(v):.3f} [{min(v):.3f} – {max(v):.3f}]"

    med = statistics.median
    emit(f"# rm_render_adaptive at {W}×{H} against rm_render_batch (B1) and rm_render_supersampled (Bss)")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} launches per variant, host clock around "
         "launches + synchronise; ms per launch, median [min – max] over the rounds.  fragColor only; A writes d_mask and d_refined.")
    out = torch.empty((1, H, W, 4), dtype=torch.float32, device=r.device)
    mask = torch.empty((1, H, W), dtype=torch.uint8, device=r.device)
    cnt = torch.empty((1,), dtype=torch.int32, device=r.device)
    src, dst = (torch.empty(21 * W * H, dtype=torch.uint8, device=r.device) for _ in range(2))
    one = torch.zeros(1, dtype=torch.float32, device=r.device)
    for name, (t, s) in configs.items():
        cams = [t.camera]
        for ss in (2, 4):
            variants = {"B1": lambda: r.render_batch(t, s, W, H, cams, out=out),
                        "Bss": lambda: r.render_supersampled(t, s, W, H, cams, ss, out=out),
                        "C copy 21 B/pixel": lambda: dst.copy_(src),
                        "E two tiny launches": lambda: (one.zero_(), one.zero_())}
            for thr in THRESHOLDS:
                variants[f"A thr {thr}"] = lambda thr=thr: r.render_adaptive(t, s, W, H, cams, ss, thr, out=out, mask=mask, counts=cnt)
            # the same results first (and every shape warmed up)
            F = r.render_batch(t, s, W, H, cams).cpu().numpy()[0]
            R = r.render_supersampled(t, s, W, H, cams, ss).cpu().numpy()[0]
            shares = {}
            for thr in THRESHOLDS:
                variants[f"A thr {thr}"]()
                m = contrast_mask(F, thr)
                assert (mask[0].cpu().numpy().astype(bool) == m).all() and int(cnt[0]) == int(m.sum()), (name, ss, thr)
                assert (out[0].cpu().numpy().view(np.uint32) == np.where(m[..., None], R, F).view(np.uint32)).all(), (name, ss, thr)
                shares[thr] = int(cnt[0]) / (W * H)
            for fn in variants.values():
                for _ in range(10):
                    fn()
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for _ in range(args.rounds):
                for k, fn in variants.items():
                    fn()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.launches):
                        fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) / args.launches * 1e3)
            b1, bss = times["B1"], times["Bss"]
            emit()
            emit(f"## {name}, ss = {ss} (A bit-equal to the composite of B1 and Bss: yes)")
            emit()
            emit("| variant | refined share (d_refined) | ms per launch, median [min – max] | B1 + share·Bss |")
            emit("|---|---|---|---|")
            for k, v in times.items():
                if k.startswith("A"):
                    sh = shares[float(k.split()[-1])]
                    emit(f"| {k} | {100 * sh:.1f} % | {fmt(v)} | {med(b1) + sh * med(bss):.3f} |")
                else:
                    emit(f"| {k} | | {fmt(v)} | |")
            sp1, spss = max(b1) - min(b1), max(bss) - min(bss)
            a_inf, a_neg, a_01 = times["A thr inf"], times["A thr -1.0"], times["A thr 0.1"]
            bound = sp1 + med(times["C copy 21 B/pixel"]) + med(times["E two tiny launches"])
            emit()
            emit(f"Spread of B1's rounds: {sp1:.3f} ms, of Bss's: {spss:.3f} ms.")
            emit(f"- threshold +inf: A − B1 = {med(a_inf) - med(b1):.3f} ms; bound (B1's spread + C + E) = {bound:.3f} ms: "
                 f"{'inside' if med(a_inf) - med(b1) < bound else 'OUTSIDE'}.")
            emit(f"- threshold 0.1: Bss − A = {med(bss) - med(a_01):.3f} ms against Bss's spread {spss:.3f} ms: "
                 f"{'A < Bss by more than the spread' if med(bss) - med(a_01) > spss else 'NOT below Bss by more than the spread'}.")
            emit(f"- threshold −1: A = {med(a_neg):.3f} ms against B1 + Bss = {med(b1) + med(bss):.3f} ms "
                 f"({(med(a_neg) / (med(b1) + med(bss)) - 1) * 100:+.1f} %: the refine kernel's gather and list traffic over render_ss_kernel).")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
