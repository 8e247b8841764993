#!/usr/bin/env python3
"""rm_shade_rays_layers and rm_trace_rays_layers on the landscape frame's own primary rays against rm_render_batch of that frame,
and a landscape panorama.  One process, one GPU, the routes interleaved round by round.

  c4's frame (scenefiles/simple/volumetric.json + TERRAIN | CLOUD | SKY_BACKGROUND | PERLIN_BUMP, 3840×2160)
        B    rm_render_batch of that ONE frame with its bright output: the one-lane-per-pixel kernel of the env class over raster
             8×8 tiles, no tuner and no tile-order feedback — the schedule rm_shade_rays_layers has
        T    rm_shade_rays_layers with bright, the frame's rays (rm_camera_rays) laid out so that each run of 64 is one 8×8 pixel
             tile: the render kernel's wave shape (tile_order); imageWidth = W
        R    the rays in row-major order (a wave is 64 pixels of one row)
        Xt   rm_trace_rays_layers on T's rays (the terrain's surface; the cloud is ignored), with normals
        Xr   rm_trace_rays_layers on R's rays
  P     render_panorama_layers, 4096×2048, from the c4 camera's position: the rays, their upload and the scatter included
  Pd    the device's share of P: rm_shade_rays_layers on the panorama's rays, already uploaded in tile order

Before timing, the outputs are checked against each other: R holds B's bits pixel for pixel, colour and bright; T holds R's rays'
results in tile order; Xt holds Xr's.  Every route is timed with HIP events around `--launches` calls, `--rounds` times; the table
gives the median and the range over the rounds.  No ratio was fixed in advance.

  python scripts/measure_layers.py [--rounds 5] [--launches 3] [--out profiles/layers_rays.md]"""
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
    ap.add_argument("--out", default=None, help="also write the tables (markdown) to this file")
    args = ap.parse_args()
    lines = []

    def emit(s=""):
        print(s, flush=True)
        lines.append(s)

    import torch
    from raymarcher_amd import Renderer, Scene, abi, camera_rays, panorama_rays, tile_order

    r = Renderer(0)  # raises without a GPU: there is nothing to measure elsewhere
    dev = r.device

    def timed(variants, launches):
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) / launches)
        return times

    def same(x, y):
        return bool((x.contiguous().view(torch.int32) == y.contiguous().view(torch.int32)).all())

    def table(times, n, base):
        emit("| route | ms per call, median [min – max] | Mrays/s | ratio to B |")
        emit("|---|---|---|---|")
        for k, v in times.items():
            med = statistics.median(v)
            emit(f"| {k} | {med:.3f} [{min(v):.3f} – {max(v):.3f}] | {n[k] / med / 1e3:.0f} | {med / base:.3f} |")
        emit()
        emit("Spread over the rounds, (max − min) / median: " +
             ", ".join(f"{k} {(max(v) - min(v)) / statistics.median(v) * 100:.1f} %" for k, v in times.items()) + ".")

    W, H = 3840, 2160
    t = Scene(path=os.path.join(SCENES, "simple", "volumetric.json")).tables(W, H, far=2000.0)
    s = abi.default_settings(features=abi.RM_FEAT_SKY_BACKGROUND | abi.RM_FEAT_TERRAIN | abi.RM_FEAT_CLOUD | abi.RM_FEAT_PERLIN_BUMP)
    n = W * H
    far = t.camera.initialFar
    emit("# rm_shade_rays_layers and rm_trace_rays_layers on the landscape frame (c4)")
    emit()
    emit(f"{torch.cuda.get_device_name(0)}; {args.rounds} interleaved rounds of {args.launches} calls per route, HIP events around the "
         "calls; ms per call, median [min – max] over the rounds.  B = rm_render_batch of the one frame, colour and bright (raster 8×8 "
         "tiles, no tuner); T = rm_shade_rays_layers, colour and bright, on the frame's rays in 8×8-tile order; R = the rays in "
         "row-major order; Xt / Xr = rm_trace_rays_layers with normals on the same two arrays; P = render_panorama_layers.")
    rays_np = camera_rays(t.camera, W, H)
    rays_r = torch.from_numpy(rays_np).to(dev)
    tile_t = torch.from_numpy(tile_order(W, H)).to(dev)
    rays_t = rays_r[tile_t].contiguous()
    frame = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
    frame_b = torch.empty((1, H, W, 4), dtype=torch.float32, device=dev)
    out = {k: (torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n, 4), dtype=torch.float32, device=dev)) for k in "TR"}
    hits = {k: torch.empty((n, 8), dtype=torch.float32, device=dev) for k in ("Xt", "Xr")}
    routes = {
        "B": lambda: r.render_batch(t, s, W, H, [t.camera], out=frame, out_bright=frame_b),
        "T": lambda: r.shade_rays_layers(t, s, rays_t, W, far=far, out=out["T"][0], out_bright=out["T"][1]),
        "R": lambda: r.shade_rays_layers(t, s, rays_r, W, far=far, out=out["R"][0], out_bright=out["R"][1]),
        "Xt": lambda: r.trace_rays_layers(t, s, rays_t, W, out=hits["Xt"]),
        "Xr": lambda: r.trace_rays_layers(t, s, rays_r, W, out=hits["Xr"]),
    }
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    for k in (0, 1):
        assert same(out["R"][k], (frame, frame_b)[k].view(n, 4)), "rm_shade_rays_layers on the camera's rays differs from rm_render_batch"
        assert same(out["T"][k], out["R"][k][tile_t]), "a ray's colour depends on its neighbours"
    assert same(hits["Xt"], hits["Xr"][tile_t]), "a ray's hit depends on its neighbours"
    ids = hits["Xr"][:, 7].view(torch.int32)
    kinds = {name: float((ids == v).float().mean()) * 100 for name, v in (("terrain", abi.RM_HIT_TERRAIN), ("sea", abi.RM_HIT_SEA),
                                                                           ("miss", -1))}
    kinds["object"] = float((ids >= 0).float().mean()) * 100
    times = timed(routes, args.launches)
    b_med = statistics.median(times["B"])
    emit()
    emit(f"## c4: volumetric.json + TERRAIN | CLOUD | SKY, {W}×{H}: {n} rays (outputs agree: yes); the trace names " +
         ", ".join(f"{v:.1f} % {k}" for k, v in kinds.items()))
    emit()
    table(times, {k: n for k in times}, b_med)
    del frame, frame_b, out, hits, rays_r, rays_t

    PW, PH = 4096, 2048
    # the camera's position: the common origin of its rays, to within the near plane
    pos = tuple(float(v) for v in rays_np[:, 0:3].astype("float64").mean(axis=0))
    rays_p = torch.from_numpy(panorama_rays(pos, PW, PH)[tile_order(PW, PH)]).to(dev)
    out_p = torch.empty((PW * PH, 4), dtype=torch.float32, device=dev)
    pano = timed({"P": lambda: r.render_panorama_layers(t, s, PW, PH, pos),
                  "Pd": lambda: r.shade_rays_layers(t, s, rays_p, PW, out=out_p)}, 1)
    img = r.render_panorama_layers(t, s, PW, PH, pos)
    back = torch.empty_like(out_p)
    back[torch.from_numpy(tile_order(PW, PH)).to(dev)] = out_p
    assert same(img.view(-1, 4), back), "render_panorama_layers differs from rm_shade_rays_layers on its rays"
    emit()
    emit(f"## render_panorama_layers {PW}×{PH} from ({pos[0]:.1f}, {pos[1]:.1f}, {pos[2]:.1f}): {PW * PH} rays, host work included "
         "(panorama_rays, the upload, the scatter back to pixels) in P, the one launch alone in Pd")
    emit()
    table(pano, {"P": PW * PH, "Pd": PW * PH}, b_med)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
