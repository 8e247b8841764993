#!/usr/bin/env python3
"""What a march through a baked lattice costs beside the march through the scene, and what the lattice queries cost by themselves.
One process, one GPU; the routes of a table interleaved round by round, HIP events around whole calls (scripts/measure_ray_order.py's
pattern): `launches` calls per event pair, `rounds` rounds, ms per call as median [min – max] over the rounds, after one untimed call
of every route.

  (a) c3, the headline Mandelbulb frame (12 iterations, 3840×2160): its camera rays in 8×8-tile order through rm_trace_rays
      (RM_TRACE_NO_NORMAL) and through rm_sdf_trace_blocks (RM_TRACE_NO_NORMAL, 256 steps, iso 0.001) on scene_field_sparse at each
      resolution of --resolutions.  Per resolution: ms per call, the share of rays whose hit-or-miss agrees with the direct march, the
      median and 99th percentile of |Δt| in cells over the rays both routes hit — and, once, the same rays SHUFFLED through the
      lattice march as they come and through rm_rays_order (0/11 bits) + march + rm_rays_restore.
  (b) the same for c2 (directional_light_2.json, 1920×1080) on the DENSE lattice of --dense points (rm_sdf_grid + rm_sdf_trace).
  (c) the block map's share of a sparse call: rm_sdf_trace_blocks with ONE ray — the map's fill and scatter and a launch of one
      workgroup — beside the whole call of (a), per resolution; at resolutions the Mandelbulb's list does not fit
      (RM_MAX_BLOCK_LIST) the c2 table stands in, and the row says so.
  (d) rm_sdf_sample_blocks on --points random points inside listed blocks of the first resolution's lattice: points per second and
      effective GB/s at 88 B per point (16 B point, 32 B record, eight values, one id, one map word).

  python scripts/field_trace_probe.py [--rounds 5] [--launches 3] [--resolutions 1025,2049] [--map-resolutions 1025,2049,4097]
                                      [--dense 513] [--points 1000000] [--out profiles/field_trace.md]"""
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
    ap.add_argument("--resolutions", default="1025,2049")
    ap.add_argument("--map-resolutions", default="1025,2049,4097")
    ap.add_argument("--dense", type=int, default=513)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)
        if args.out:  # as it goes: a run that is cut short leaves what it measured
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    import numpy as np
    import torch
    from raymarcher_amd import RaymarcherError, Renderer, Scene, abi, camera_rays, scenes, tile_order

    r = Renderer(0)
    dev = r.device
    ISO, STEPS = 0.001, 256

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

    def agreement(direct, lattice, cell):
        """(share of rays whose hit-or-miss agrees, median and 99th percentile of |Δt| in cells over the rays both hit)"""
        hd, hl = direct[:, 7].view(torch.int32) >= 0, lattice[:, 7].view(torch.int32) >= 0
        both = hd & hl
        dt = ((direct[:, 3] - lattice[:, 3]).abs()[both] / cell).double()
        q = lambda p: float(torch.quantile(dt[:: max(1, dt.numel() // 4000000)], p)) if dt.numel() else float("nan")  # noqa: E731
        return float((hd == hl).double().mean()), q(0.5), q(0.99), int(hd.sum()), int(hl.sum())

    def table(name):
        if name == "c3":
            W, H = 3840, 2160
            return scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12), W, H, f"c3 (Mandelbulb, 12 iterations, {W}×{H})"
        W, H = 1920, 1080
        t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
        return t, abi.default_settings(), W, H, f"c2 (directional_light_2.json, {W}×{H})"

    def rays_of(t, W, H):
        return torch.from_numpy(camera_rays(t.camera, W, H)[tile_order(W, H)]).to(dev).contiguous()

    emit("# rm_sdf_trace / rm_sdf_sample: a march through the baked lattice beside the march through the scene")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the calls; "
         "ms per call, median [min – max] over the rounds.  The routes are in the head of scripts/field_trace_probe.py.  Both marches: "
         f"RM_TRACE_NO_NORMAL; the lattice's: iso {ISO}, {STEPS} steps, with object ids.")

    # ---- (a) and (c) on the Mandelbulb, (d) on its first lattice
    t, s, W, H, title = table("c3")
    rays = rays_of(t, W, H)
    n = rays.shape[0]
    direct, lat = (torch.empty((n, 8), dtype=torch.float32, device=dev) for _ in range(2))
    one = rays[n // 2:n // 2 + 1].contiguous()
    one_out = torch.empty((1, 8), dtype=torch.float32, device=dev)
    emit()
    emit(f"## (a) {title}: {n} camera rays in 8×8-tile order")
    emit()
    emit("| resolution | listed blocks | lattice MiB | bake ms (select + grid_blocks, one call) | rm_trace_rays | rm_sdf_trace_blocks | "
         "direct / lattice | hit-or-miss agrees | hits direct / lattice | median abs Δt, cells | 99th percentile |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|")
    map_rows, first_field, shuffled = {}, None, None
    for res in sorted({int(v) for v in args.resolutions.split(",")} | {int(v) for v in args.map_resolutions.split(",")}):
        try:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            field = r.scene_field_sparse(t, s, res, iso=ISO)
            e1.record()
            e1.synchronize()
        except RaymarcherError as err:
            map_rows[res] = f"c3: {err}"
            continue
        grid, ids, bl, blocks, origin, step = field
        march = lambda src=rays, dst=lat: r.trace_lattice_blocks(grid, bl, blocks, origin, step, src, iso=ISO, max_steps=STEPS, ids=ids,  # noqa: E731
                                                                 normals=False, out=dst)
        routes = {"direct": lambda: r.trace_rays(t, s, rays, normals=False, out=direct), "lattice": march,
                  "map": lambda: march(one, one_out)}
        times = timed(routes)
        share, med, p99, nd, nl = agreement(direct, lat, step[0])
        mib = (grid.numel() + ids.numel()) * 4 / 2 ** 20
        if str(res) in args.resolutions.split(","):
            emit(f"| {res} | {bl.shape[0]} of {int(np.prod(blocks))} | {mib:.0f} | {e0.elapsed_time(e1):.1f} | {show(times['direct'])} | "
                 f"{show(times['lattice'])} | {statistics.median(times['direct']) / statistics.median(times['lattice']):.2f} | {share:.4%} | "
                 f"{nd} / {nl} | {med:.3f} | {p99:.3f} |")
        map_rows[res] = (f"c3, {bl.shape[0]} listed of {int(np.prod(blocks))} blocks", times["map"], times["lattice"])
        if first_field is None:
            first_field = field
            perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
            mixed = rays[perm].contiguous()
            out_u, out_x = (torch.empty((n, 8), dtype=torch.float32, device=dev) for _ in range(2))

            def sorted_route():
                order, srt = r.order_rays(mixed, 0, 11)
                march(srt, out_x)
                r.restore_order(out_x, order, out=out_u)

            tm = timed({"as they come": lambda: march(mixed, out_x), "order + march + restore": sorted_route})
            shuffled = (res, tm)
            del mixed, out_u, out_x, perm
        else:
            del field, grid, ids, bl
        torch.cuda.empty_cache()
    if shuffled:
        res, tm = shuffled
        emit()
        emit(f"The same rays in a seeded shuffle through the lattice march at resolution {res}: as they come {show(tm['as they come'])} ms; "
             f"rm_rays_order (0/11 bits) + march + rm_rays_restore {show(tm['order + march + restore'])} ms.")

    # ---- (d)
    if first_field is not None:
        grid, ids, bl, blocks, origin, step = first_field
        gen = torch.Generator(device=dev)
        gen.manual_seed(5)
        k = args.points
        pick = bl[torch.randint(0, bl.shape[0], (k,), generator=gen, device=dev).long(), :3].float()
        u = pick * 8.0 + torch.rand((k, 3), generator=gen, device=dev) * 8.0
        pts = torch.zeros((k, 4), dtype=torch.float32, device=dev)
        pts[:, :3] = torch.tensor(list(origin), dtype=torch.float32, device=dev) + u * step[0]
        got = r.sample_lattice_blocks(grid, bl, blocks, origin, step, pts, ids=ids)
        listed = float((got[3] >= 0).double().mean())
        tm = timed({"sample": lambda: r.sample_lattice_blocks(grid, bl, blocks, origin, step, pts, ids=ids),
                    "map": lambda: r.sample_lattice_blocks(grid, bl, blocks, origin, step, pts[:1], ids=ids)})
        ms, mp = statistics.median(tm["sample"]), statistics.median(tm["map"])
        emit()
        emit(f"## (d) rm_sdf_sample_blocks: {k} random points inside listed blocks ({listed:.2%} of them sampled), c3 at {shuffled[0]}")
        emit()
        emit(f"{show(tm['sample'])} ms per call, of which the block map and a one-point launch {show(tm['map'])} ms: {k / ms / 1e6 * 1e3:.0f} M points/s "
             f"and {k * 88 / ms / 1e6:.1f} GB/s effective for the whole call, {k / max(ms - mp, 1e-6) / 1e6 * 1e3:.0f} M points/s and "
             f"{k * 88 / max(ms - mp, 1e-6) / 1e6:.1f} GB/s behind the map (the allocation of the output included in both).")
        del first_field, grid, ids, bl, pts, got
        torch.cuda.empty_cache()
    del direct, lat

    # ---- (b)
    t2, s2, W2, H2, title2 = table("c2")
    rays2 = rays_of(t2, W2, H2)
    n2 = rays2.shape[0]
    d2, l2 = (torch.empty((n2, 8), dtype=torch.float32, device=dev) for _ in range(2))
    origin, step, dims = r._scene_lattice(t2, args.dense, None)
    dense, dids = r.sdf_grid(t2, s2, origin, (step,) * 3, dims, ids=True)
    tm = timed({"direct": lambda: r.trace_rays(t2, s2, rays2, normals=False, out=d2),
                "lattice": lambda: r.trace_lattice(dense, origin, (step,) * 3, rays2, iso=ISO, max_steps=STEPS, ids=dids, normals=False, out=l2)})
    share, med, p99, nd, nl = agreement(d2, l2, step)
    emit()
    emit(f"## (b) {title2}: {n2} camera rays in 8×8-tile order, the dense lattice of {dims[0]}×{dims[1]}×{dims[2]} points "
         f"({(dense.numel() + dids.numel()) * 4 / 2 ** 20:.0f} MiB)")
    emit()
    emit("| rm_trace_rays | rm_sdf_trace | direct / lattice | hit-or-miss agrees | hits direct / lattice | median abs Δt, cells | 99th percentile |")
    emit("|---|---|---|---|---|---|---|")
    emit(f"| {show(tm['direct'])} | {show(tm['lattice'])} | {statistics.median(tm['direct']) / statistics.median(tm['lattice']):.2f} | {share:.4%} | "
         f"{nd} / {nl} | {med:.3f} | {p99:.3f} |")
    del dense, dids
    torch.cuda.empty_cache()

    # ---- (c)
    for res in (int(v) for v in args.map_resolutions.split(",")):
        if isinstance(map_rows.get(res), str):  # the Mandelbulb's list does not fit: the c2 table stands in
            why = map_rows[res]
            try:
                grid, ids, bl, blocks, origin, step = r.scene_field_sparse(t2, s2, res, iso=ISO)
            except RaymarcherError as err:
                map_rows[res] = f"{why}; c2: {err}"
                continue
            march2 = lambda src, dst: r.trace_lattice_blocks(grid, bl, blocks, origin, step, src, iso=ISO, max_steps=STEPS, ids=ids,  # noqa: E731
                                                             normals=False, out=dst)
            tm = timed({"map": lambda: march2(rays2[:1], l2[:1]), "lattice": lambda: march2(rays2, l2)})
            map_rows[res] = (f"c2 ({n2} rays), {bl.shape[0]} listed of {int(np.prod(blocks))} blocks — {why}", tm["map"], tm["lattice"])
            del grid, ids, bl
            torch.cuda.empty_cache()
    emit()
    emit("## (c) the block map's share of a sparse call")
    emit()
    emit("| resolution | table | one-ray call (map + one workgroup) | whole call | share |")
    emit("|---|---|---|---|---|")
    for res in (int(v) for v in args.map_resolutions.split(",")):
        row = map_rows.get(res)
        if isinstance(row, tuple):
            emit(f"| {res} | {row[0]} | {show(row[1])} | {show(row[2])} | {statistics.median(row[1]) / statistics.median(row[2]):.1%} |")
        else:
            emit(f"| {res} | not run: {row} | | | |")


if __name__ == "__main__":
    main()
