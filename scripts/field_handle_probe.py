#!/usr/bin/env python3
"""What an RmField handle buys beside the entry points it stands in for.  One process, one GPU, one build; the routes of a table
interleaved round by round, HIP events around whole calls (scripts/field_trace_probe.py's pattern): `launches` calls per
event pair, `rounds` rounds, ms per call as median [min – max] over the rounds, after one untimed call of every route.

  (a) c3, the headline Mandelbulb frame (12 iterations, 3840×2160): its camera rays in 8×8-tile order through rm_trace_rays,
      through rm_sdf_trace_blocks and through rm_field_trace (all RM_TRACE_NO_NORMAL; the lattice's: 256 steps, iso 0.001) on
      scene_field_sparse at each resolution of --resolutions, and the same rays in a seeded shuffle through the two lattice
      routes.  Per resolution: ms per call, and the share of rays whose hit-or-miss agrees with the direct march, per lattice route.
      rm_field_trace counts samples only, so at the same number it does more than rm_sdf_trace_blocks, whose iterations run out among
      the skips: the tile-ordered rows also time rm_sdf_trace_blocks with 256 + mx + my + mz iterations, which lacks none the handle's
      march has, and give the share of records on which the two are equal in every word.
      With --fine-lib (a build of the library with -DRM_FIELD_COARSE=0, loaded beside the first into this process) a handle of
      that build is a route of the same rounds: the coarse level on against off.
  (b) rm_sdf_sample_blocks against rm_field_sample on --points random points inside listed blocks of the first resolution's
      lattice, each beside its one-point call.  A one-point call is a launch of one workgroup, the allocation of its output and
      the host's part of a call; the old entry's also builds the block map, so the difference of the two one-point calls is the
      map build, and "old − map build" is what the handle's call is held against.
  (c) c2 (directional_light_2.json, 1920×1080) on the DENSE lattice of --dense points: rm_sdf_trace against rm_field_trace on the
      camera rays; then SHADOW rays — from each camera ray's hit, lifted 0.01 along the normal, towards the scene's first light —
      through rm_trace_rays RM_TRACE_OCCLUSION and through rm_field_trace RM_TRACE_OCCLUSION, with the share of rays on which the
      two agree about an occluder and the median |Δ visibility| where both see none.
  (d) what rm_field_create_blocks costs once, per resolution of --create-resolutions: wall time around the call (it synchronises).

  python scripts/field_handle_probe.py [--rounds 5] [--launches 3] [--resolutions 1025,2049] [--create-resolutions 1025,2049,4097]
                                       [--dense 513] [--points 1000000] [--fine-lib PATH] [--out profiles/field_handle.md]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--resolutions", default="1025,2049")
    ap.add_argument("--create-resolutions", default="1025,2049,4097")
    ap.add_argument("--dense", type=int, default=513)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--fine-lib", default=None, help="a build with -DRM_FIELD_COARSE=0, measured beside the loaded one")
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
    from raymarcher_amd._lib import SIGNATURES

    r = Renderer(0)
    dev = r.device
    ISO, STEPS = 0.001, 256
    fine = None
    if args.fine_lib:
        fine = C.CDLL(os.path.abspath(args.fine_lib))
        for name in ("rm_field_create_blocks", "rm_field_destroy", "rm_field_trace", "rm_set_device"):
            getattr(fine, name).restype, getattr(fine, name).argtypes = SIGNATURES[name]
        assert fine.rm_set_device(0) == abi.RM_OK

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

    def ratio(a, b):
        return f"{statistics.median(a) / statistics.median(b):.2f}"

    def agrees(direct, lattice):
        return float(((direct[:, 7].view(torch.int32) >= 0) == (lattice[:, 7].view(torch.int32) >= 0)).double().mean())

    def table(name):
        if name == "c3":
            W, H = 3840, 2160
            return scenes.mandelbulb(W, H), abi.default_settings(fractalIters=12), W, H, f"c3 (Mandelbulb, 12 iterations, {W}×{H})"
        W, H = 1920, 1080
        t = Scene(path=os.path.join(SCENES, "lighting", "directional_light_2.json")).tables(W, H)
        return t, abi.default_settings(), W, H, f"c2 (directional_light_2.json, {W}×{H})"

    def rays_of(t, W, H):
        return torch.from_numpy(camera_rays(t.camera, W, H)[tile_order(W, H)]).to(dev).contiguous()

    def vec(v):
        return (C.c_float * 3)(*[float(x) for x in v])

    emit("# RmField handles beside rm_sdf_sample_blocks / rm_sdf_trace_blocks / rm_sdf_trace / rm_trace_rays")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the calls; "
         "ms per call, median [min – max] over the rounds.  The routes are in the head of scripts/field_handle_probe.py.  The marches of "
         f"(a) and of (c)'s first table: RM_TRACE_NO_NORMAL; the lattice's: iso {ISO}, {STEPS} steps / samples, with object ids.")

    # ---- (a), (b), (d) on the Mandelbulb
    t, s, W, H, title = table("c3")
    rays = rays_of(t, W, H)
    n = rays.shape[0]
    perm = torch.from_numpy(np.random.default_rng(7).permutation(n)).to(dev)
    mixed = rays[perm].contiguous()
    del perm
    direct, old, new, off, raised = (torch.empty((n, 8), dtype=torch.float32, device=dev) for _ in range(5))
    r.trace_rays(t, s, rays, normals=False, out=direct)
    emit()
    emit(f"## (a) {title}: {n} camera rays through the sparse lattice")
    emit()
    emit("| resolution | listed blocks | order | rm_trace_rays | rm_sdf_trace_blocks | rm_field_trace | old / handle | handle, coarse level off | "
         "off / on | agrees with rm_trace_rays: old | handle | rm_sdf_trace_blocks with 256 + mx + my + mz iterations | raised / handle | "
         "its records equal to the handle's |")
    emit("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    create_rows, first = {}, None
    wanted = [int(v) for v in args.resolutions.split(",")]
    for res in sorted(set(wanted) | {int(v) for v in args.create_resolutions.split(",")}):
        try:
            grid, ids, bl, blocks, origin, step = r.scene_field_sparse(t, s, res, iso=ISO)
        except RaymarcherError as err:
            create_rows[res] = f"not run: {err}"
            continue
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        field = r.lattice_field_blocks(grid, bl, blocks, origin, step, ids=ids)
        create_ms = [(time.perf_counter() - w0) * 1e3]
        for _ in range(4):
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            again = r.lattice_field_blocks(grid, bl, blocks, origin, step, ids=ids)
            create_ms.append((time.perf_counter() - w0) * 1e3)
            again.close()
        create_rows[res] = f"{bl.shape[0]} listed of {int(np.prod(blocks))} blocks | {create_ms[0]:.3f} | {show(create_ms[1:])}"
        if res in wanted:
            fh = C.c_void_p()
            if fine is not None:
                st = fine.rm_field_create_blocks(C.c_void_p(grid.data_ptr()), C.c_void_p(ids.data_ptr()), C.c_void_p(bl.data_ptr()), bl.shape[0],
                                                 *blocks, vec(origin), vec(step), r._stream(), C.byref(fh))
                assert st == abi.RM_OK and fh.value
            for order, src in (("8×8 tiles", rays), ("shuffled", mixed)):
                routes = {"old": lambda: r.trace_lattice_blocks(grid, bl, blocks, origin, step, src, iso=ISO, max_steps=STEPS, ids=ids, normals=False, out=old),
                          "new": lambda: field.trace(src, iso=ISO, max_steps=STEPS, normals=False, out=new)}
                if order == "8×8 tiles":
                    routes["direct"] = lambda: r.trace_rays(t, s, rays, normals=False, out=direct)
                    routes["raised"] = lambda: r.trace_lattice_blocks(grid, bl, blocks, origin, step, src, iso=ISO, max_steps=STEPS + sum(blocks),
                                                                      ids=ids, normals=False, out=raised)
                if fine is not None:
                    routes["off"] = lambda: fine.rm_field_trace(fh, C.c_void_p(src.data_ptr()), n, ISO, STEPS, abi.RM_TRACE_NO_NORMAL,
                                                                C.c_void_p(off.data_ptr()), r._stream())
                tm = timed(routes)
                same = "" if fine is None else ("same bits" if torch.equal(new.view(torch.int32), off.view(torch.int32)) else "BITS DIFFER")
                emit(f"| {res} | {bl.shape[0]} of {int(np.prod(blocks))} | {order} | {show(tm['direct']) if 'direct' in tm else ''} | {show(tm['old'])} | "
                     f"{show(tm['new'])} | {ratio(tm['old'], tm['new'])} | {show(tm['off']) + ', ' + same if fine is not None else 'not built'} | "
                     f"{ratio(tm['off'], tm['new']) if fine is not None else ''} | "
                     + (f"{agrees(direct, old):.4%} | {agrees(direct, new):.4%} | {show(tm['raised'])} | {ratio(tm['raised'], tm['new'])} | "
                        f"{float((raised.view(torch.int32) == new.view(torch.int32)).all(dim=1).double().mean()):.4%} |"
                        if order == "8×8 tiles" else " | | | | |"))
            if fh.value:
                torch.cuda.synchronize()
                fine.rm_field_destroy(fh)
        if first is None and res in wanted:
            first = res
            gen = torch.Generator(device=dev)
            gen.manual_seed(5)
            k = args.points
            pick = bl[torch.randint(0, bl.shape[0], (k,), generator=gen, device=dev).long(), :3].float()
            u = pick * 8.0 + torch.rand((k, 3), generator=gen, device=dev) * 8.0
            pts = torch.zeros((k, 4), dtype=torch.float32, device=dev)
            pts[:, :3] = torch.tensor(list(origin), dtype=torch.float32, device=dev) + u * step[0]
            a, b = r.sample_lattice_blocks(grid, bl, blocks, origin, step, pts, ids=ids), field.sample(pts)
            same = all(torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)) for x, y in zip(a, b))
            sample_tm = timed({"old": lambda: r.sample_lattice_blocks(grid, bl, blocks, origin, step, pts, ids=ids),
                               "map": lambda: r.sample_lattice_blocks(grid, bl, blocks, origin, step, pts[:1], ids=ids),
                               "new": lambda: field.sample(pts), "new one point": lambda: field.sample(pts[:1])})
            sample_row = (k, res, same, sample_tm)
            del pts, a, b, pick, u
        field.close()
        del field, grid, ids, bl
        torch.cuda.empty_cache()
    del mixed, old, new, off, raised, direct, rays
    torch.cuda.empty_cache()

    if first is not None:
        k, res, same, tm = sample_row
        emit()
        emit(f"## (b) {k} random points inside listed blocks, c3 at {res} ({'the same bits from both' if same else 'BITS DIFFER'})")
        emit()
        med = {k: statistics.median(v) for k, v in tm.items()}
        build = med["map"] - med["new one point"]  # both one-point calls launch one workgroup and allocate one record: what is left is the map
        emit("| rm_sdf_sample_blocks | its one-point call | rm_field_sample | its one-point call | the map build (difference of the one-point "
             "calls) | old − map build | old / handle | (old − map build) / handle |")
        emit("|---|---|---|---|---|---|---|---|")
        emit(f"| {show(tm['old'])} | {show(tm['map'])} | {show(tm['new'])} | {show(tm['new one point'])} | {build:.3f} | {med['old'] - build:.3f} | "
             f"{ratio(tm['old'], tm['new'])} | {(med['old'] - build) / med['new']:.2f} |")

    # ---- (c)
    t2, s2, W2, H2, title2 = table("c2")
    rays2 = rays_of(t2, W2, H2)
    n2 = rays2.shape[0]
    d2, o2, h2 = (torch.empty((n2, 8), dtype=torch.float32, device=dev) for _ in range(3))
    origin, step, dims = r._scene_lattice(t2, args.dense, None)
    dense, dids = r.sdf_grid(t2, s2, origin, (step,) * 3, dims, ids=True)
    field = r.lattice_field(dense, origin, (step,) * 3, ids=dids)
    tm = timed({"direct": lambda: r.trace_rays(t2, s2, rays2, normals=False, out=d2),
                "old": lambda: r.trace_lattice(dense, origin, (step,) * 3, rays2, iso=ISO, max_steps=STEPS, ids=dids, normals=False, out=o2),
                "new": lambda: field.trace(rays2, iso=ISO, max_steps=STEPS, normals=False, out=h2)})
    same = torch.equal(o2.view(torch.int32), h2.view(torch.int32))
    emit()
    emit(f"## (c) {title2}: {n2} camera rays in 8×8-tile order, the dense lattice of {dims[0]}×{dims[1]}×{dims[2]} points")
    emit()
    emit("| rm_trace_rays | rm_sdf_trace | rm_field_trace | old / handle | bits |")
    emit("|---|---|---|---|---|")
    emit(f"| {show(tm['direct'])} | {show(tm['old'])} | {show(tm['new'])} | {ratio(tm['old'], tm['new'])} | {'the same' if same else 'DIFFER'} |")
    # shadow rays: from the direct march's hits towards the first light
    nrm, tt, pos, oid = r.trace_rays(t2, s2, rays2)
    light = t2.lights[0]
    hit = oid >= 0
    shadow = torch.zeros((n2, 8), dtype=torch.float32, device=dev)
    shadow[:, 0:3] = pos + 0.01 * nrm
    shadow[:, 3] = float(t2.camera.initialFar)
    if light.type == abi.RM_LIGHT_DIRECTIONAL:
        to_light = -torch.tensor(list(light.dir), dtype=torch.float32, device=dev)
        shadow[:, 4:7] = to_light / to_light.norm()
    else:
        to_light = torch.tensor(list(light.pos), dtype=torch.float32, device=dev) - shadow[:, 0:3]
        shadow[:, 3] = to_light.norm(dim=1)
        shadow[:, 4:7] = to_light / shadow[:, 3:4]
    shadow = shadow[hit].contiguous()  # in the camera rays' tile order
    ns = shadow.shape[0]
    sd, sl = (torch.empty((ns, 8), dtype=torch.float32, device=dev) for _ in range(2))
    tm = timed({"direct": lambda: r.trace_rays(t2, s2, shadow, mode="occlusion", out=sd),
                "new": lambda: field.trace(shadow, iso=ISO, max_steps=STEPS, mode="occlusion", out=sl)})
    od, ol = sd[:, 7].view(torch.int32) >= 0, sl[:, 7].view(torch.int32) >= 0
    free = ~od & ~ol
    dv = float((sd[:, 3] - sl[:, 3]).abs()[free].double().median()) if bool(free.any()) else float("nan")
    emit()
    emit(f"Shadow rays of the same frame ({ns}, towards light 0, tMax {'far' if light.type == abi.RM_LIGHT_DIRECTIONAL else 'the light'}), RM_TRACE_OCCLUSION:")
    emit()
    emit("| rm_trace_rays | rm_field_trace | direct / handle | occluded direct / handle | agree on occluded-or-not | median abs Δ penumbra factor where both see none |")
    emit("|---|---|---|---|---|---|")
    emit(f"| {show(tm['direct'])} | {show(tm['new'])} | {ratio(tm['direct'], tm['new'])} | {int(od.sum())} / {int(ol.sum())} | "
         f"{float((od == ol).double().mean()):.4%} | {dv:.4f} |")
    field.close()

    # ---- (d)
    emit()
    emit("## (d) rm_field_create_blocks, once: the block map and the coarse level, wall ms around the call (it synchronises its stream)")
    emit()
    emit("| resolution | c3's list | first call | four more, median [min – max] |")
    emit("|---|---|---|---|")
    for res in (int(v) for v in args.create_resolutions.split(",")):
        emit(f"| {res} | {create_rows.get(res, 'not run')} |")


if __name__ == "__main__":
    main()
