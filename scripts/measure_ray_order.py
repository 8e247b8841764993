#!/usr/bin/env python3
"""What rm_rays_order costs and what it buys: incoherent rays traced and shaded as they come, against order → the same call on the
sorted rays → restore.  One process, one GPU, the routes of a table interleaved round by round (scripts/measure_trace.py's pattern).

  cases      c3 (the Mandelbulb, 12 iterations, 3840×2160) and c2 (directional_light_2.json, 1920×1080): DESIGN §6.12 / §6.13
  workloads  (a) the frame's primary rays in a seeded shuffle (§6.12's and §6.13's route S); the 8×8-tile order is the floor
             (b) AO-style rays: the hit points of the frame in tile order, pushed 0.002 along the normal, each with a seeded
                 direction in the hemisphere about its normal, tMax 1 — origins that are neighbours, directions that are not
  calls      rm_trace_rays (closest) and rm_shade_rays
  routes     U      the call on the rays as they come (the baseline: the kernels of rm_trace.hip and rm_shade.hip, whose code
                    objects this feature does not change)
             F      (a) only: the call on the rays in tile order
             per bit pair (originBits, dirBits) of --bits:
             O      rm_rays_order with d_sorted
             X      the call on d_sorted
             R      rm_rays_restore of the call's output
             E      O, X and R back to back: the end-to-end time a caller of trace_rays_sorted / shade_rays_sorted pays

Before anything is timed, the restored output of every bit pair is compared with U's output, bit for bit.  "Pays" means: the
median of E is below the median of U by more than the larger of the two routes' ranges (max − min over the rounds).  No ratio was
fixed in advance.  The sort is also held against its own byte traffic at the achievable HBM rate of 6.3 TB/s: per ray 32 B (bounds)
+ 44 B (keys: the ray again, key and index out) + 32 B per pass that runs (the histogram reads the key, 8 B; the scatter reads
key and index, 12 B, and writes them, 12 B) + 72 B (the index, d_order, and the gather of d_sorted).  A skipped pass reads and
writes nothing.

  python scripts/measure_ray_order.py [--rounds 5] [--launches 3] [--cases c3,c2] [--bits 0:11,7:8,8:10,10:11] [--out profiles/ray_order.md]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--cases", default="c3,c2")
    ap.add_argument("--bits", default="0:11,7:8,8:10,10:11")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    pairs = [tuple(int(v) for v in p.split(":")) for p in args.bits.split(",")]
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, lib, scenes, tile_order

    r = Renderer(0)
    dev = r.device
    L = lib()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

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

    def show(v):
        return f"{statistics.median(v):.3f} [{min(v):.3f} – {max(v):.3f}]"

    def passes_run(keys, ob, db):
        """How many of the sort's passes run, from the keys themselves: the digits on which not all keys agree."""
        k = keys.cpu().numpy().view(np.uint64)
        differ = int(np.bitwise_or.reduce(k)) ^ int(np.bitwise_and.reduce(k))
        total = (3 * ob + 2 * db + 1 + 7) // 8
        return sum(1 for p in range(total) if (differ >> (8 * p)) & 0xff), total

    def workload(title, t, s, rays, floor_rays, far):
        n = rays.shape[0]
        order = torch.empty((n,), dtype=torch.int32, device=dev)
        srt = torch.empty((n, 8), dtype=torch.float32, device=dev)
        keys = torch.empty((n,), dtype=torch.int64, device=dev)

        def do_order(ob, db, with_keys=False):
            st = L.rm_rays_order(ptr(rays), n, ob, db, ptr(order), ptr(srt), ptr(keys) if with_keys else None, r._stream())
            assert st == 0, L.rm_last_error().decode()

        for call in ("trace", "shade"):
            words = 8 if call == "trace" else 4
            out_u, out_x, out_r, out_f = (torch.empty((n, words), dtype=torch.float32, device=dev) for _ in range(4))
            if call == "trace":
                run = lambda src, dst: r.trace_rays(t, s, src, out=dst)  # noqa: E731
            else:
                run = lambda src, dst: r.shade_rays(t, s, src, far=far, out=dst)  # noqa: E731

            def do_restore():
                assert L.rm_rays_restore(ptr(out_x), ptr(order), n, 4 * words, ptr(out_r), r._stream()) == 0

            run(rays, out_u)
            info = {}
            for ob, db in pairs:  # every bit pair gives U's bits back, checked before anything is timed
                out_r.fill_(-1.0)
                do_order(ob, db, with_keys=True)
                run(srt, out_x)
                do_restore()
                torch.cuda.synchronize()
                assert same(out_r, out_u), f"{title} {call} bits {(ob, db)}: the sorted route differs from the unsorted call"
                info[(ob, db)] = passes_run(keys, ob, db)
            routes = {"U": lambda: run(rays, out_u)}
            if floor_rays is not None:
                routes["F"] = lambda: run(floor_rays, out_f)
            for ob, db in pairs:
                tag = f"{ob}/{db}"

                def end_to_end(ob=ob, db=db):
                    do_order(ob, db)
                    run(srt, out_x)
                    do_restore()

                routes[f"O {tag}"] = lambda ob=ob, db=db: do_order(ob, db)
                routes[f"X {tag}"] = lambda: run(srt, out_x)  # srt holds this pair's order: O of the same pair ran just before
                routes[f"R {tag}"] = do_restore
                routes[f"E {tag}"] = end_to_end
            times = timed(routes)
            u = times["U"]
            emit()
            emit(f"### {title}, rm_{call}_rays: {n} rays")
            emit()
            emit(f"U (as they come) {show(u)} ms" + (f"; F (tile order, the floor) {show(times['F'])} ms; U / F = "
                                                    f"{statistics.median(u) / statistics.median(times['F']):.2f}" if "F" in times else "") + ".")
            emit()
            emit("| bits | passes run / of | O order | X call on sorted | R restore | O + X + R | E end to end | U / E | pays | "
                 "sort traffic at 6.3 TB/s | O / that |")
            emit("|---|---|---|---|---|---|---|---|---|---|---|")
            for ob, db in pairs:
                tag = f"{ob}/{db}"
                o, x, rs, e = (times[f"{k} {tag}"] for k in "OXRE")
                ran, total = info[(ob, db)]
                ideal = n * (32 + 44 + 32 * ran + 72) / HBM * 1e3
                gain = statistics.median(u) - statistics.median(e)
                pays = gain > max(max(u) - min(u), max(e) - min(e))
                emit(f"| {tag} | {ran} / {total} | {show(o)} | {show(x)} | {show(rs)} | "
                     f"{statistics.median(o) + statistics.median(x) + statistics.median(rs):.3f} | {show(e)} | "
                     f"{statistics.median(u) / statistics.median(e):.2f} | {'yes' if pays else 'no'} | {ideal:.3f} ms | "
                     f"{statistics.median(o) / ideal:.1f}× |")
            summary.append((title, call, u, {p: times[f"E {p[0]}/{p[1]}"] for p in pairs}))
            del out_u, out_x, out_r, out_f

    summary = []
    emit("# rm_rays_order: the sort's cost, and incoherent rays with and without it")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per call, median [min – max] over the rounds.  The routes, the workloads and what \"pays\" means are in the head of "
         "scripts/measure_ray_order.py.  Every sorted route's restored output equals the unsorted call's in every bit, checked before "
         "the timing.  The baseline U runs the kernels of rm_trace.hip and rm_shade.hip, which this feature leaves as they were "
         "(DESIGN §6.19).")
    for name in args.cases.split(","):
        if name == "c3":
            W, H = 3840, 2160
            t, s = scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12)
            title = f"c3 (Mandelbulb, 12 iterations, {W}×{H})"
        elif name == "c2":
            W, H = 1920, 1080
            t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
            s = abi.default_settings()
            title = f"c2 (directional_light_2.json, {W}×{H})"
        else:
            raise KeyError(name)
        n = W * H
        far = t.camera.initialFar
        rays_t = torch.from_numpy(camera_rays(t.camera, W, H)[tile_order(W, H)]).to(dev).contiguous()
        perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
        rays_s = rays_t[perm].contiguous()
        emit()
        emit(f"## {title}")
        workload(f"{name} (a) shuffled primary rays", t, s, rays_s, rays_t, far)
        # (b): the hit points in tile order, a seeded direction in the hemisphere about each normal
        hits = torch.empty((n, 8), dtype=torch.float32, device=dev)
        r.trace_rays(t, s, rays_t, out=hits)
        hit = hits[hits[:, 7].view(torch.int32) >= 0]
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        d = torch.randn((hit.shape[0], 3), generator=gen, device=dev, dtype=torch.float32)
        d = d / d.norm(dim=1, keepdim=True)
        d = torch.where((d * hit[:, 0:3]).sum(1, keepdim=True) < 0, -d, d)
        ao = torch.zeros((hit.shape[0], 8), dtype=torch.float32, device=dev)
        ao[:, 0:3] = hit[:, 4:7] + 0.002 * hit[:, 0:3]
        ao[:, 3] = 1.0
        ao[:, 4:7] = d
        del hits, hit, d
        workload(f"{name} (b) AO-style rays from the hit points", t, s, ao.contiguous(), None, far)
        del rays_t, rays_s, ao
    # which key the Python layer should default to: per table the pair with the lowest end-to-end median, and how the default and
    # the finest key stand beside it ("same": the medians differ by no more than the larger of the two ranges)
    import inspect
    sig = inspect.signature(Renderer.order_rays).parameters
    default, finest = (sig["origin_bits"].default, sig["dir_bits"].default), (10, 11)
    med, rng = statistics.median, lambda v: max(v) - min(v)  # noqa: E731

    def beside(e, best):
        return f"{med(e):.3f} ({med(e) / med(best):.2f}, {'same' if abs(med(e) - med(best)) <= max(rng(e), rng(best)) else 'apart'})"

    emit()
    emit("## Summary: end to end (E), ms, per bit pair")
    emit()
    emit(f"The Python default is {default[0]}/{default[1]}.  In brackets: the ratio to the table's best pair, and whether the two are "
         "told apart by the rounds' ranges.")
    emit()
    emit("| workload | call | U | best pair | its E | U / E | default's E | finest key's E |")
    emit("|---|---|---|---|---|---|---|---|")
    for title, call, u, e in summary:
        best = min(e, key=lambda p: med(e[p]))
        emit(f"| {title} | {call} | {med(u):.3f} | {best[0]}/{best[1]} | {med(e[best]):.3f} | {med(u) / med(e[best]):.2f} | "
             f"{beside(e[default], e[best]) if default in e else 'not swept'} | {beside(e[finest], e[best]) if finest in e else 'not swept'} |")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
