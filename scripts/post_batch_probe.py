#!/usr/bin/env python3
"""What does the post step of an exported sequence cost, per frame, as a host loop of rm_post_process + rm_frame_to_rgba8 against one
rm_post_process_batch + rm_frames_to_rgba8?  torch.cuda.Event times on one stream after warm-up, the two ways alternated in one
process, every timed output compared word for word with the per-frame path; plus the end-to-end export (render_sequence against
render_batch followed by per-frame post).  GPU box only.

Usage: python scripts/post_batch_probe.py --out DIR            the whole probe → DIR/post_batch_probe.json
       python scripts/post_batch_probe.py --out DIR --single   rm_post_process single-frame times only → DIR/post_single.json;
                                                               with --root TREE, of the package and library built in another
                                                               checkout (e.g. the parent commit's)
       python scripts/post_batch_probe.py --trace              one per-frame loop and one batch at 256², N = 64, bloom + HDR +
                                                               FXAA, for a rocprofv3 --kernel-trace --stats run"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--single", action="store_true")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose raymarcher_amd package (and built library) is measured; default: this one")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
import torch  # noqa: E402
from raymarcher_amd import Renderer, abi  # noqa: E402

SIZES = [(256, 256, 64), (256, 256, 256), (1920, 1080, 8), (3840, 2160, 4)]
CASES = {"bloom+hdr+fxaa": dict(enableBloom=1, enableHDR=1, enableFXAA=1, exposure=0.8), "hdr+fxaa": dict(enableHDR=1, enableFXAA=1, exposure=1.2)}


def frames(r, N, W, H, seed=0):
    """N different random frames (values up to 1.6) and their sparse BrightColor planes, on the device."""
    g = torch.Generator(device=r.device).manual_seed(seed)
    frag = torch.rand((N, H, W, 4), generator=g, device=r.device) * 1.6
    frag[..., 3] = 1.0
    luma = (frag[..., :3] * torch.tensor([0.2126, 0.7152, 0.0722], device=r.device)).sum(-1, keepdim=True)
    bright = torch.where(luma > 1.0, frag, torch.zeros_like(frag))
    bright[..., 3] = 1.0
    return frag.contiguous(), bright.contiguous()


def timed(fn, reps):
    """ms per call of fn, device events around reps calls on the current stream."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(ways, reps, rounds=7):
    """{name: median ms per call} of the ways timed in turn, `rounds` times over (each warmed up first)."""
    for fn in ways.values():
        fn()
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in ways}
    for _ in range(rounds):
        for k, fn in ways.items():
            ms[k].append(timed(fn, reps))
    return {k: statistics.median(v) for k, v in ms.items()}, {k: [min(v), max(v)] for k, v in ms.items()}


def mismatches(a, b):
    return int((a.view(torch.int32) != b.view(torch.int32)).sum()) if a.dtype == torch.float32 else int((a != b).sum())


def post_probe(r):
    rows = []
    for W, H, N in SIZES:
        fd, bd = frames(r, N, W, H)
        for name, kw in CASES.items():
            posts = [abi.RmPostSettings(**{**kw, "exposure": kw["exposure"] * (0.6 + 0.8 * f / N)}) for f in range(N)]  # a fade
            o, o8 = torch.empty_like(fd), torch.empty((N, H, W, 4), dtype=torch.uint8, device=r.device)
            b, b8 = torch.empty_like(fd), torch.empty_like(o8)

            def loop():
                for f in range(N):
                    r.post_process(fd[f], bd[f], posts[f], out=o[f])
                    r.to_rgba8(o[f], out=o8[f])

            def batch():
                r.post_process_batch(fd, bd, posts, out=b)
                r.to_rgba8_batch(b, out=b8)

            reps = max(2, 256 // N)
            med, spread = alternate({"per_frame": loop, "batch": batch}, reps)
            row = dict(W=W, H=H, N=N, passes=name, ms_per_frame_loop=med["per_frame"] / N, ms_per_frame_batch=med["batch"] / N,
                       ratio=med["batch"] / med["per_frame"], spread_ms_per_call=spread,
                       mismatched_words=mismatches(b, o), mismatched_bytes=mismatches(b8, o8))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del fd, bd
        torch.cuda.empty_cache()
    return rows


def e2e_probe(r):
    import bench
    rows = []
    for cfg, N in (("c1", 64), ("c2", 8)):
        t, s, W, H = bench.build_config(cfg)[:4]
        cams = [t.camera] * N  # the configuration's view, iTime advancing
        globs = []
        for f in range(N):
            g = abi.RmGlobals.from_buffer_copy(bytes(t.globals_))
            g.iTime = 0.1 * f
            globs.append(g)
        post = abi.RmPostSettings(**CASES["bloom+hdr+fxaa"])
        outs = {}

        def seq():
            outs["seq"] = r.render_sequence(t, s, W, H, cams, globals_=globs, post=post)

        def per_frame_post():
            fr, br = r.render_batch(t, s, W, H, cams, globals_=globs, bright=True)
            o8 = torch.empty((N, H, W, 4), dtype=torch.uint8, device=r.device)
            for f in range(N):
                r.to_rgba8(r.post_process(fr[f], br[f], post), out=o8[f])
            outs["loop"] = o8

        med, spread = alternate({"render_batch+per_frame_post": per_frame_post, "render_sequence": seq}, max(2, 64 // N), rounds=5)
        row = dict(config=cfg, W=W, H=H, N=N, passes="bloom+hdr+fxaa", ms_per_frame_loop=med["render_batch+per_frame_post"] / N,
                   ms_per_frame_sequence=med["render_sequence"] / N, spread_ms_per_call=spread,
                   mismatched_bytes=mismatches(outs["seq"], outs["loop"]))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def single_probe(r):
    """rm_post_process of one frame, ms per call, at every probe size and pass set (the library's single-frame path)."""
    rows = []
    for W, H, _ in SIZES[:1] + SIZES[2:]:
        fd, bd = frames(r, 1, W, H)
        o = torch.empty_like(fd[0])
        for name, kw in CASES.items():
            ps = abi.RmPostSettings(**kw)
            med, spread = alternate({"single": lambda: r.post_process(fd[0], bd[0], ps, out=o)}, max(4, 2048 * 2048 // (W * H)), rounds=9)
            rows.append(dict(W=W, H=H, passes=name, ms=med["single"], spread_ms=spread["single"]))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    a = ARGS
    if not a.trace and not a.out:
        ap.error("--out DIR is required (except with --trace)")
    r = Renderer(0)
    if a.trace:
        W, H, N = SIZES[0]
        fd, bd = frames(r, N, W, H)
        ps = abi.RmPostSettings(**CASES["bloom+hdr+fxaa"])
        for _ in range(2):
            for f in range(N):
                r.to_rgba8(r.post_process(fd[f], bd[f], ps))
            torch.cuda.synchronize()
            r.to_rgba8_batch(r.post_process_batch(fd, bd, ps))
            torch.cuda.synchronize()
        return
    os.makedirs(a.out, exist_ok=True)
    if a.single:
        import raymarcher_amd
        res = {"package": os.path.abspath(raymarcher_amd.__file__), "single": single_probe(r)}
        name = "post_single.json"
    else:
        res = {"device": torch.cuda.get_device_name(0), "post": post_probe(r), "end_to_end": e2e_probe(r)}
        name = "post_batch_probe.json"
    with open(os.path.join(a.out, name), "w") as f:
        json.dump(res, f, indent=1)
    bad = sum(row.get("mismatched_words", 0) + row.get("mismatched_bytes", 0) for k in ("post", "end_to_end") for row in res.get(k, []))
    if bad:
        print(f"{bad} mismatched words/bytes", flush=True)
        sys.exit(1)


if __name__ == "__main__":
    main()
