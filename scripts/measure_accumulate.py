#!/usr/bin/env python3
"""rm_render_accumulated against the only way to the same picture before it: rm_render_batch of every sub-frame into a
numFrames·n-frame buffer, then the sequential reduction of the header with torch operations on the same stream.  One process, one
GPU, the two routes interleaved round by round:

  A   rm_render_accumulated                                   (one launch, no n-sized image)
  B   rm_render_batch of the numFrames·n sub-frames + torch   (acc = S_0; acc += S_j, j = 1 … n − 1; acc *= 1/n — fragColor and
                                                               BrightColor)

for three cases, all with BrightColor:

  small   c1's scene (unit_sphere.json, 64 steps) at 256×256, n = 16 lens samples, 16 frames
  dof     depth_of_field.json at 1920×1080, n = 16, its own focus distance (the lens three times the file's), reflection on
  bulb4k  c3's Mandelbulb at 3840×2160, n = 8

Before timing, A is compared bit for bit with B.  Every variant is timed with HIP events around `--launches` calls, `--rounds`
times; the table gives the median and the range over the rounds.  The spread of B's own rounds is what a difference between A and B
has to exceed.  For bulb4k the peak device memory of each route is recorded too (torch's allocator, which owns every image of
either route; the library adds its scene blocks, ≈9.7 KB per sub-frame, to both).

  python scripts/measure_accumulate.py [--rounds 7] [--launches 10] [--out profiles/accumulate.md]"""
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
    ap.add_argument("--cases", default="small,dof,bulb4k")
    ap.add_argument("--out", default=None, help="also write the table (markdown) to this file")
    args = ap.parse_args()

    import torch
    from raymarcher_amd import Renderer, Scene, abi, scenes
    from raymarcher_amd.render import lens_cameras

    r = Renderer(0)
    dev = r.device

    def case(name):
        if name == "small":
            W = H = 256
            sc = Scene(path=os.path.join(SCENES, "simple", "unit_sphere.json"))
            cd = sc.camera_data()
            cams = []
            for f in range(16):  # 16 frames: the camera steps sideways, each frame through its own lens
                cd.pos[0] += 0.02
                cams += lens_cameras(cd, W, H, 0.05, 4.0, 16)
            return sc.tables(W, H), abi.default_settings(maxSteps=64), W, H, 16, cams
        if name == "dof":
            W, H = 1920, 1080
            sc = Scene(path=os.path.join(SCENES, "lighting", "depth_of_field.json"))
            radius, focus = sc.lens()
            return sc.tables(W, H), abi.default_settings(enableReflection=1), W, H, 16, lens_cameras(sc.camera_data(), W, H, 3.0 * radius, focus, 16)
        if name == "bulb4k":
            W, H = 3840, 2160
            cd = abi.RmCameraData()
            cd.pos[:] = (0.0, 0.0, 4.5, 1.0)
            cd.look[:] = (0.0, 0.0, -4.5, 0.0)
            cd.up[:] = (0.0, 1.0, 0.0, 0.0)
            cd.heightAngle = 30.0 * 3.14159265358979323846 / 180.0
            return scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12), W, H, 8, lens_cameras(cd, W, H, 0.05, 3.6, 8)
        raise KeyError(name)

    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    emit("# rm_render_accumulated against rm_render_batch of every sub-frame + a sequential reduction")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per call, median [min – max] over the rounds.  fragColor + BrightColor in both routes.")
    for name in args.cases.split(","):
        t, s, W, H, n, cams = case(name)
        frames = len(cams) // n
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        a_out = torch.empty((frames, H, W, 4), dtype=torch.float32, device=dev)
        a_br = torch.empty_like(a_out)

        def run_a():
            r.render_accumulated(t, s, W, H, cams, n, out=a_out, out_bright=a_br)

        run_a()
        torch.cuda.synchronize()
        peak_a = torch.cuda.max_memory_allocated() - base
        torch.cuda.reset_peak_memory_stats()
        b_sub = torch.empty((frames * n, H, W, 4), dtype=torch.float32, device=dev)
        b_subbr = torch.empty_like(b_sub)
        b_out = torch.empty_like(a_out)
        b_br = torch.empty_like(a_out)
        scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))

        def run_b():
            r.render_batch(t, s, W, H, cams, out=b_sub, out_bright=b_subbr)
            for src, dst in ((b_sub, b_out), (b_subbr, b_br)):
                v = src.view(frames, n, H, W, 4)
                dst.copy_(v[:, 0])
                for j in range(1, n):
                    dst.add_(v[:, j])
                dst.mul_(scale)

        run_b()
        torch.cuda.synchronize()
        peak_b = torch.cuda.max_memory_allocated() - base - 2 * a_out.numel() * 4  # without A's outputs, which are still alive
        same = bool((a_out.view(torch.int32) == b_out.view(torch.int32)).all()) and bool((a_br.view(torch.int32) == b_br.view(torch.int32)).all())
        assert same, f"{name}: rm_render_accumulated differs from rm_render_batch reduced"
        variants = {"A accumulated": run_a, "B batch + reduction": run_b}
        for fn in variants.values():
            for _ in range(5):
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
        emit()
        emit(f"## {name}: {W}×{H}, n = {n}, {frames} frame{'s' if frames > 1 else ''} (A bit-equal to B: yes)")
        emit()
        emit("| route | ms per call, median [min – max] | Msub-frame-pixels/s | peak device memory of the route's images |")
        emit("|---|---|---|---|")
        for (k, v), peak in zip(times.items(), (peak_a, peak_b)):
            med = statistics.median(v)
            emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {frames * n * W * H / med / 1e3:.0f} | {peak / 2**20:.1f} MiB |")
        a, b = times["A accumulated"], times["B batch + reduction"]
        emit()
        emit(f"B's own spread over its rounds: {(max(b) - min(b)) / statistics.median(b) * 100:.1f} % of its median; A's: "
             f"{(max(a) - min(a)) / statistics.median(a) * 100:.1f} %.  A against B: {(statistics.median(a) / statistics.median(b) - 1) * 100:+.1f} %.")
        del a_out, a_br, b_sub, b_subbr, b_out, b_br
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
