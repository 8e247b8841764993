#!/usr/bin/env python3
"""rm_render_animated measured two ways.  One process, one GPU, the routes of a case interleaved round by round.

  (i)  restage overhead: depth_of_field.json at 1920×1080, n = 16 lens samples, reflection on, the tables shared
         A   rm_render_animated, numObjectTables = numLightTables = 1     (render_anim_kernel, no restage bit set)
         B   rm_render_accumulated of the same call                       (render_acc_kernel: rm_accumulate.hip's code object and the
                                                                            staging it goes through are byte-for-byte the parent
                                                                            commit's, DESIGN §6.10, so B is the parent's route)
  (ii) what the feature buys: c1's scene (unit_sphere.json, 64 steps) plus a second sphere that translates per block, 256×256,
       64 frames, with n = 1 and with n = 8
         A   rm_render_animated with one object table per block           (one launch)
         B   one rm_render_res per block into a blocks-sized buffer + the sequential reduction of the header as torch operations
             on the same stream — the only route there was

Before timing, A is compared bit for bit with B.  Every route is timed with HIP events around `--launches` calls, `--rounds` times;
the table gives the median and the range over the rounds.  The spread of B's own rounds is what a difference has to exceed.

  python scripts/measure_animated.py [--rounds 7] [--launches 10] [--cases dof,move1,move8] [--out profiles/animated.md]"""
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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--cases", default="dof,move1,move8")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()

    import torch
    from raymarcher_amd import Renderer, Scene, SceneTables, abi, translated_objects
    from raymarcher_amd.render import lens_cameras

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

    def report(title, times, work):
        emit()
        emit(f"## {title} (A bit-equal to B: yes)")
        emit()
        emit("| route | ms per call, median [min – max] | Msub-frame-pixels/s |")
        emit("|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {work / med / 1e3:.0f} |")
        (ka, a), (kb, b) = times.items()
        emit()
        emit(f"B's own spread over its rounds: {(max(b) - min(b)) / statistics.median(b) * 100:.1f} % of its median; A's: "
             f"{(max(a) - min(a)) / statistics.median(a) * 100:.1f} %.  A / B = {statistics.median(a) / statistics.median(b):.3f}.")

    def bit_equal(x, y):
        return bool((x.view(torch.int32) == y.view(torch.int32)).all())

    emit("# rm_render_animated: the restage overhead, and one launch against one rm_render_res per block")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per call, median [min – max] over the rounds.  fragColor + BrightColor in every route.")
    for name in args.cases.split(","):
        if name == "dof":
            W, H, n = 1920, 1080, 16
            sc = Scene(path=os.path.join(SCENES, "lighting", "depth_of_field.json"))
            radius, focus = sc.lens()
            t, s = sc.tables(W, H), abi.default_settings(enableReflection=1)
            cams = lens_cameras(sc.camera_data(), W, H, 3.0 * radius, focus, n)
            outs = [torch.empty((1, H, W, 4), dtype=torch.float32, device=dev) for _ in range(4)]

            def run_a():
                r.render_animated(t, s, W, H, cams, n, out=outs[0], out_bright=outs[1])

            def run_b():
                r.render_accumulated(t, s, W, H, cams, n, out=outs[2], out_bright=outs[3])

            run_a()
            run_b()
            torch.cuda.synchronize()
            assert bit_equal(outs[0], outs[2]) and bit_equal(outs[1], outs[3]), "rm_render_animated differs from rm_render_accumulated"
            times = timed({"A animated, shared tables": run_a, "B accumulated": run_b})
            report(f"(i) depth_of_field.json {W}×{H}, n = {n}, shared tables", times, n * W * H)
            del outs
        elif name in ("move1", "move8"):
            W = H = 256
            n, frames = (1 if name == "move1" else 8), 64
            blocks = n * frames
            sc = Scene(path=os.path.join(SCENES, "simple", "unit_sphere.json"))
            base = sc.tables(W, H)
            mover = abi.RmObject()
            C.memmove(C.byref(mover), C.byref(base.objects[0]), C.sizeof(abi.RmObject))
            objs = [base.objects[i] for i in range(base.num_objects)] + [mover]
            t = SceneTables(base.camera, (abi.RmObject * len(objs))(*objs), len(objs), base.lights, base.num_lights, base.globals_)
            s = abi.default_settings(maxSteps=64)
            stacked = translated_objects(objs, len(objs) - 1, [(-1.5 + 3.0 * b / (blocks - 1), 0.6, 0.0) for b in range(blocks)])
            per_block = [SceneTables(base.camera, (abi.RmObject * len(objs))(*stacked[b * len(objs):(b + 1) * len(objs)]), len(objs),
                                     base.lights, base.num_lights, base.globals_) for b in range(blocks)]
            cams = [base.camera] * blocks
            a_out = torch.empty((frames, H, W, 4), dtype=torch.float32, device=dev)
            a_br, b_out, b_br = torch.empty_like(a_out), torch.empty_like(a_out), torch.empty_like(a_out)
            b_sub = torch.empty((blocks, H, W, 4), dtype=torch.float32, device=dev)
            b_subbr = torch.empty_like(b_sub)
            scale = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32))

            def run_a():
                r.render_animated(t, s, W, H, cams, n, objects=stacked, out=a_out, out_bright=a_br)

            def run_b():
                for b in range(blocks):
                    r.render(per_block[b], s, W, H, out=b_sub[b], out_bright=b_subbr[b])
                for src, dst in ((b_sub, b_out), (b_subbr, b_br)):
                    v = src.view(frames, n, H, W, 4)
                    dst.copy_(v[:, 0])
                    for j in range(1, n):
                        dst.add_(v[:, j])
                    dst.mul_(scale)

            run_a()
            run_b()
            torch.cuda.synchronize()
            assert bit_equal(a_out, b_out) and bit_equal(a_br, b_br), f"{name}: rm_render_animated differs from rm_render_res per block reduced"
            times = timed({"A animated": run_a, "B rm_render_res per block + reduction": run_b})
            report(f"(ii) unit_sphere.json + a translating sphere, {W}×{H}, {frames} frames, n = {n}", times, blocks * W * H)
            del a_out, a_br, b_out, b_br, b_sub, b_subbr
        else:
            raise KeyError(name)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
