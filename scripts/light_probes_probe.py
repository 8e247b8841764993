#!/usr/bin/env python3
"""What rm_light_probes buys beside the composition a caller writes without it.  One GPU, one build.  Per scene a child process of
its own under a time limit of its own; the first one that fails ends the run, and what the earlier ones measured stays in --out.
In a child the routes are interleaved round by round, HIP events around whole calls (scripts/field_ambient_probe.py's pattern,
DESIGN §7): `launches` calls per event pair, `rounds` rounds, ms per call as median [min – max] over the rounds, after one untimed
call of every route.

  fused        Renderer.light_probes into a tensor allocated before: ONE launch of rm_light_probes.
  composition  on the same commit, from the same table: the n·K RmRay rows built on the device with torch, rm_shade_rays on them,
               and a torch projection (one einsum) of the n·K colours onto the table's nine basis values.  It has no hit channel:
               that would take an rm_trace_rays call on the same rays on top.  Timed end to end.
  shade alone  the bare rm_shade_rays call in the middle, on rays already built.

Peak extra device memory of a route: torch.cuda.max_memory_allocated around one call minus what was allocated before it; the fused
route's includes its (n, 40) result.  The two routes' coefficients differ by the order of the sum only (the einsum has its own);
the largest difference relative to the largest coefficient is reported.

Scenes: c2 (directional_light_2.json) and the Mandelbulb of raymarcher_amd.scenes, reference settings.  Shapes: a g×g×g grid of
probes over the box of the table's cull ball, 32³ probes × 256 directions and 10³ × 64.

  python scripts/light_probes_probe.py [--rounds 5] [--launches 2] [--out profiles/light_probes.md] [--limit 420]"""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
NAMES = ("c2", "bulb")
SHAPES = ((32, 256), (10, 64))


def child(args):
    import torch
    from raymarcher_amd import Renderer, Scene, abi, lib, scenes, sphere_directions

    r = Renderer(0)
    dev = r.device
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)
        with open(args.section, "w") as f:  # as it goes: a child that is cut short leaves what it measured
            f.write("\n".join(lines) + "\n")

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

    def show(v):
        return f"{statistics.median(v):.3f} [{min(v):.3f} – {max(v):.3f}]"

    def peak_extra(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        keep = fn()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated(dev) - before
        del keep
        return extra

    if args.scene == "c2":
        t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(64, 36)
        title = "c2 (directional_light_2.json)"
    else:
        t = scenes.mandelbulb(64, 36)
        title = "the Mandelbulb"
    s = abi.default_settings()
    far = float(t.camera.initialFar)
    bounds = (C.c_float * 14)()
    assert lib().rm_debug_cull_bounds(t.objects, t.num_objects, C.byref(t.globals_), bounds) == 0
    centre, radius = ((bounds[1], bounds[2], bounds[3]), bounds[4] ** 0.5) if bounds[0] != 0.0 and bounds[4] > 0.0 else ((0.0, 0.0, 0.0), 3.0)
    emit(f"## {title}: probes on a grid over the box of the cull ball (centre {centre[0]:.2f} {centre[1]:.2f} {centre[2]:.2f}, radius {radius:.2f}), "
         f"far {far:g}")
    emit()
    head = ("| probes | directions | rays | fused, ms | composition, ms | its rm_shade_rays alone, ms | composition / fused | shade alone / fused | "
            "fused: peak extra MiB | composition: peak extra MiB | 160 B · n, MiB | 48 B · n · K, MiB | max Δ coefficient / max coefficient | "
            "rays that hit |")
    emit(head)
    emit("|" + "---|" * (head.count("|") - 1))
    for g, K in SHAPES:
        n = g ** 3
        axis = torch.linspace(-1.0, 1.0, g, device=dev) * radius
        pos = torch.zeros((n, 4), dtype=torch.float32, device=dev)
        pos[:, 0:3] = torch.stack(torch.meshgrid(axis, axis, axis, indexing="ij"), dim=3).reshape(n, 3) + torch.tensor(centre, device=dev)
        table = torch.from_numpy(sphere_directions(K, 1)).to(dev)
        out = torch.empty((n, 40), dtype=torch.float32, device=dev)
        rays = torch.empty((n * K, 8), dtype=torch.float32, device=dev)
        colours = torch.empty((n * K, 4), dtype=torch.float32, device=dev)

        def fused(into=out):
            return r.light_probes(t, s, pos, directions=K, sets=1, far=far, table=table, out=into)

        def build(into):
            v = into.view(n, K, 8)
            v[:, :, 0:3] = pos[:, None, 0:3]
            v[:, :, 3] = far
            v[:, :, 4:7] = table[None, :, 0:3]
            v[:, :, 7] = 0.0
            return into

        def shade(src, into):
            return r.shade_rays(t, s, src, far=far, out=into)

        def project(c):
            return torch.einsum("nkc,kj->njc", c.view(n, K, 4)[:, :, 0:3], table[:, 4:13])

        def composed(own_memory=False):
            src = build(torch.empty((n * K, 8), dtype=torch.float32, device=dev) if own_memory else rays)
            return project(shade(src, None if own_memory else colours))

        build(rays)
        tm = timed({"fused": fused, "composed": composed, "shade": lambda: shade(rays, colours)})
        sh, hits = fused()
        ref = composed()
        scale = float(ref.abs().max())
        delta = float((sh[:, :, 0:3] - ref).abs().max()) / scale if scale > 0 else 0.0
        share = float(hits.clamp(min=0).sum()) / (n * K)
        mem_fused = peak_extra(lambda: fused(None))
        del rays, colours, ref
        mem_composed = peak_extra(lambda: composed(True))
        mib = 1.0 / (1 << 20)
        emit(f"| {g}³ = {n} | {K} | {n * K} | {show(tm['fused'])} | {show(tm['composed'])} | {show(tm['shade'])} | "
             f"{statistics.median(tm['composed']) / statistics.median(tm['fused']):.2f} | "
             f"{statistics.median(tm['shade']) / statistics.median(tm['fused']):.2f} | {mem_fused * mib:.1f} | {mem_composed * mib:.1f} | "
             f"{160.0 * n * mib:.1f} | {48.0 * n * K * mib:.1f} | {delta:.2e} | {share:.3f} |")
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="seconds a scene's child process may take")
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    ap.add_argument("--scene", default=None, choices=NAMES, help="(internal) measure this scene in this process")
    ap.add_argument("--section", default=None, help="(internal) where the child writes its section")
    args = ap.parse_args()
    if args.scene:
        return child(args)
    import tempfile
    text = ["# rm_light_probes beside rm_shade_rays and torch", "",
            f"{args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the calls; ms per call, median [min – max] over "
            "the rounds.  Reference settings, one set of rm_sphere_directions' directions.  The routes and the columns are in the head of "
            "scripts/light_probes_probe.py.  Mapping: (probe, direction) pairs flattened over lanes, a segment of numDirs lanes per probe, "
            "xor-shuffle tree; 256 directions are four passes of 64 by one wave.", ""]
    status = 0
    with tempfile.TemporaryDirectory() as tmp:
        for scene in NAMES:
            section = os.path.join(tmp, scene + ".md")
            cmd = [sys.executable, os.path.abspath(__file__), "--scene", scene, "--section", section, "--rounds", str(args.rounds), "--launches",
                   str(args.launches)]
            try:
                status = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                status = 124
            if os.path.exists(section):
                text += open(section).read().splitlines() + [""]
            if status != 0:
                text += [f"{scene}: ended with status {status}; nothing after it was run.", ""]
            if args.out:
                with open(args.out, "w") as f:
                    f.write("\n".join(text))
            if status != 0:
                break
    return status


if __name__ == "__main__":
    sys.exit(main())
