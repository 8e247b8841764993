"""What the query entry points (rm_queries.hip) owe the launcher's one staging call, stage_block_launch (rm_launcher.hip), behind
every launch: the path rm_debug_last_path reports, one timed launch per call under rm_set_timing(1) — none and no path for a probe —
and a slot of the batch ring that is not handed out again while its upload may still be in flight.  One sphere, 64 rays, 64 points,
a 9×9×9 lattice (one block), 64 probe points; each entry once."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as h
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

N = 64


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _scene():
    objs, no = h.table([h.make_object(abi.RM_SPHERE)])
    lights, nl = h.table([h.make_light(abi.RM_LIGHT_DIRECTIONAL, direction=(0.3, -1.0, 0.5))], struct=abi.RmLight)
    return objs, no, lights, nl, h.make_globals(), abi.default_settings()


def _rays(device):
    r = np.zeros((N, 8), dtype=np.float32)
    r[:, 0] = np.linspace(-0.7, 0.7, N)  # some hit the sphere, some pass it
    r[:, 1] = 0.1
    r[:, 2] = -3.0
    r[:, 3] = 100.0
    r[:, 6] = 1.0
    return torch.from_numpy(r).to(device)


def test_every_entry_records_its_path_and_one_timed_launch(renderer):
    L, dev, stream = lib(), renderer.device, renderer._stream()
    objs, no, lights, nl, g, s = _scene()
    rays = _rays(dev)
    hits = torch.empty((N, 8), dtype=torch.float32, device=dev)
    rgba = torch.empty((N, 4), dtype=torch.float32, device=dev)
    pts4 = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    pts4[:, 0] = torch.linspace(-0.6, 0.6, N, device=dev)
    surface = torch.empty((N, 8), dtype=torch.float32, device=dev)
    ps = abi.RmPointsSettings()
    L.rm_points_settings_default(C.byref(ps))
    origin, step = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.25, 0.25, 0.25)
    dist = torch.empty((9, 9, 9), dtype=torch.float32, device=dev)
    blocks = torch.zeros((4, 4), dtype=torch.int32, device=dev)
    count = torch.zeros((2,), dtype=torch.int32, device=dev)
    block_dist = torch.empty((1, 729), dtype=torch.float32, device=dev)
    pts3 = pts4[:, :3].contiguous()
    probe = torch.empty((N, 4), dtype=torch.float32, device=dev)
    G, S = C.byref(g), C.byref(s)

    def select_is_one_block():
        torch.cuda.synchronize()
        assert int(count[0]) == 1 and blocks[0].tolist() == [0, 0, 0, 0]

    # (the call, the path behind it or None for "unchanged", an optional check of what it stored)
    calls = [
        ("rm_trace_rays closest", lambda: L.rm_trace_rays(_ptr(rays), N, objs, no, G, S, abi.RM_TRACE_CLOSEST, _ptr(hits), stream), 12, None),
        ("rm_trace_rays occlusion", lambda: L.rm_trace_rays(_ptr(rays), N, objs, no, G, S, abi.RM_TRACE_OCCLUSION, _ptr(hits), stream), 12, None),
        ("rm_shade_rays", lambda: L.rm_shade_rays(_ptr(rays), N, 100.0, objs, no, lights, nl, G, S, None, _ptr(rgba), None, stream), 13, None),
        ("rm_shade_rays_layers", lambda: L.rm_shade_rays_layers(_ptr(rays), N, 100.0, 8, objs, no, lights, nl, G, S, None, _ptr(rgba), None,
                                                                stream), 14, None),
        ("rm_trace_rays_layers", lambda: L.rm_trace_rays_layers(_ptr(rays), N, 8, objs, no, G, S, abi.RM_TRACE_CLOSEST, _ptr(hits), stream), 15,
         None),
        ("rm_shade_points with d_rgba", lambda: L.rm_shade_points(_ptr(pts4), None, N, C.byref(ps), objs, no, lights, nl, G, S, None,
                                                                  _ptr(surface), None, _ptr(rgba), stream), 17, None),
        ("rm_shade_points without d_rgba", lambda: L.rm_shade_points(_ptr(pts4), None, N, C.byref(ps), objs, no, lights, nl, G, S, None,
                                                                     _ptr(surface), None, None, stream), 17, None),
        ("rm_sdf_grid", lambda: L.rm_sdf_grid(objs, no, G, S, origin, step, 9, 9, 9, _ptr(dist), None, stream), 16, None),
        ("rm_sdf_blocks_select", lambda: L.rm_sdf_blocks_select(objs, no, G, S, origin, step, 1, 1, 1, 0.0, 4, _ptr(blocks), _ptr(count), stream),
         18, select_is_one_block),
        ("rm_sdf_blocks_select_pruned", lambda: L.rm_sdf_blocks_select_pruned(objs, no, G, S, origin, step, 1, 1, 1, 0.0, 1.0, 1.0, 4, _ptr(blocks),
                                                                              _ptr(count), stream), 20, select_is_one_block),
        ("rm_sdf_grid_blocks", lambda: L.rm_sdf_grid_blocks(objs, no, G, S, origin, step, 1, 1, 1, _ptr(blocks), 1, _ptr(block_dist), None, stream),
         19, None),
        ("rm_probe_sdscene", lambda: L.rm_probe_sdscene(objs, no, G, S, _ptr(pts3), _ptr(probe), N, stream), None, None),
    ]
    ms, launches = C.c_double(), C.c_int()
    assert L.rm_set_timing(1) == abi.RM_OK
    try:
        for name, call, path, check in calls:
            before = L.rm_debug_last_path()
            assert call() == abi.RM_OK, f"{name}: {L.rm_last_error()}"
            assert L.rm_debug_last_path() == (before if path is None else path), name
            assert L.rm_get_timing(C.byref(ms), C.byref(launches)) == abi.RM_OK  # hands out, and forgets, the launches timed since the last call
            assert launches.value == (0 if path is None else 1), name
            if check:
                check()
        torch.cuda.synchronize()
        assert torch.isfinite(probe).all()
    finally:
        L.rm_set_timing(0)


def test_light_and_lattice_entries_record_their_path_and_timed_launches(renderer):
    """The sibling of the test above for the light family, the lattice queries and rm_field_ambient.  The four bakes and shades stage
    a scene: their path and one timed launch.  The two grid lookups, the handle queries, rm_field_ambient and the handle-free
    lattice queries are "not render launches": rm_debug_last_path() keeps its value and rm_set_timing does not time them."""
    from raymarcher_amd import hemisphere_directions, probe_depth_weights, sphere_directions
    L, dev, stream = lib(), renderer.device, renderer._stream()
    objs, no, lights, nl, g, s = _scene()
    G, S = C.byref(g), C.byref(s)
    rays = _rays(dev)
    pts4 = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    pts4[:, 0] = torch.linspace(-0.9, 0.9, N, device=dev)
    pts4[:, 1] = 0.2
    nrm4 = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    nrm4[:, 1] = 1.0
    K, P = 8, 8  # eight probes on the corners of one cell around the sphere, eight directions each
    table_h = sphere_directions(K, 1)
    table = torch.from_numpy(table_h).to(dev)
    weights = torch.from_numpy(probe_depth_weights(table_h, 1)).to(dev)
    dims, origin, step = (C.c_int * 3)(2, 2, 2), (C.c_float * 3)(-1.5, -1.5, -1.5), (C.c_float * 3)(3.0, 3.0, 3.0)
    pos = torch.tensor([[-1.5 + 3.0 * (i & 1), -1.5 + 3.0 * (i >> 1 & 1), -1.5 + 3.0 * (i >> 2), 1.0] for i in range(P)], dtype=torch.float32, device=dev)
    probes = torch.empty((P, 40), dtype=torch.float32, device=dev)
    second = torch.empty((P, 40), dtype=torch.float32, device=dev)
    depth = torch.empty((P, 64, 2), dtype=torch.float32, device=dev)
    light = torch.empty((N, 8), dtype=torch.float32, device=dev)
    rgba = torch.empty((N, 4), dtype=torch.float32, device=dev)
    ref = abi.RmLightGridRef(probes.data_ptr(), depth.data_ptr(), (C.c_int32 * 3)(2, 2, 2), (C.c_float * 3)(-1.5, -1.5, -1.5), (C.c_float * 3)(3.0, 3.0, 3.0),
                             1.0, abi.RM_LIGHT_GRID_FACING, 0.1)
    # a 9×9×9 lattice of the sphere, dense and as one block, a handle on each
    lo, st = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.25, 0.25, 0.25)
    dist = torch.empty((9, 9, 9), dtype=torch.float32, device=dev)
    blocks = torch.zeros((1, 4), dtype=torch.int32, device=dev)
    block_dist = torch.empty((1, 729), dtype=torch.float32, device=dev)
    assert L.rm_sdf_grid(objs, no, G, S, lo, st, 9, 9, 9, _ptr(dist), None, stream) == abi.RM_OK
    assert L.rm_sdf_grid_blocks(objs, no, G, S, lo, st, 1, 1, 1, _ptr(blocks), 1, _ptr(block_dist), None, stream) == abi.RM_OK
    dense, sparse = C.c_void_p(), C.c_void_p()
    assert L.rm_field_create(_ptr(dist), None, 9, 9, 9, lo, st, C.byref(dense)) == abi.RM_OK
    assert L.rm_field_create_blocks(_ptr(block_dist), None, _ptr(blocks), 1, 1, 1, 1, lo, st, stream, C.byref(sparse)) == abi.RM_OK
    hemi = torch.from_numpy(hemisphere_directions(K, 1)).to(dev)
    samples = torch.empty((N, 8), dtype=torch.float32, device=dev)
    hits = torch.empty((N, 8), dtype=torch.float32, device=dev)
    ambient = torch.empty((N, 8), dtype=torch.float32, device=dev)

    # (the call, the path behind it or None for "unchanged and not timed")
    calls = [
        ("rm_light_probes", lambda: L.rm_light_probes(_ptr(pos), P, _ptr(table), K, 1, 100.0, objs, no, lights, nl, G, S, None, _ptr(probes), stream), 21),
        ("rm_light_probes_depth", lambda: L.rm_light_probes_depth(_ptr(pos), P, _ptr(table), _ptr(weights), K, 1, 4.0, objs, no, G, S, _ptr(depth), stream), 22),
        ("rm_shade_rays_indirect", lambda: L.rm_shade_rays_indirect(_ptr(rays), N, 100.0, objs, no, lights, nl, G, S, None, C.byref(ref), _ptr(rgba), stream), 23),
        ("rm_light_probes_indirect", lambda: L.rm_light_probes_indirect(_ptr(pos), P, _ptr(table), K, 1, 100.0, objs, no, lights, nl, G, S, None, C.byref(ref),
                                                                        _ptr(second), stream), 24),
        ("rm_light_grid_irradiance", lambda: L.rm_light_grid_irradiance(_ptr(probes), dims, origin, step, _ptr(pts4), _ptr(nrm4), N, abi.RM_LIGHT_GRID_FACING,
                                                                        _ptr(light), stream), None),
        ("rm_light_grid_irradiance_visible", lambda: L.rm_light_grid_irradiance_visible(_ptr(probes), _ptr(depth), dims, origin, step, _ptr(pts4), _ptr(nrm4), N,
                                                                                        abi.RM_LIGHT_GRID_FACING, 0.1, _ptr(light), stream), None),
        ("rm_field_sample dense", lambda: L.rm_field_sample(dense, _ptr(pts4), N, _ptr(samples), stream), None),
        ("rm_field_sample blocks", lambda: L.rm_field_sample(sparse, _ptr(pts4), N, _ptr(samples), stream), None),
        ("rm_field_trace dense", lambda: L.rm_field_trace(dense, _ptr(rays), N, 0.0, 64, abi.RM_TRACE_CLOSEST, _ptr(hits), stream), None),
        ("rm_field_trace blocks, occlusion", lambda: L.rm_field_trace(sparse, _ptr(rays), N, 0.0, 64, abi.RM_TRACE_OCCLUSION, _ptr(hits), stream), None),
        ("rm_field_ambient dense", lambda: L.rm_field_ambient(dense, _ptr(pts4), _ptr(nrm4), N, _ptr(hemi), K, 1, 0.5, 2.0, 0.0, 64, abi.RM_AMBIENT_SOFT,
                                                              _ptr(ambient), stream), None),
        ("rm_field_ambient blocks, hard", lambda: L.rm_field_ambient(sparse, _ptr(pts4), None, N, _ptr(hemi), K, 1, 0.5, 2.0, 0.0, 64, abi.RM_AMBIENT_HARD,
                                                                     _ptr(ambient), stream), None),
        ("rm_sdf_sample", lambda: L.rm_sdf_sample(_ptr(pts4), N, _ptr(dist), None, 9, 9, 9, lo, st, _ptr(samples), stream), None),
        ("rm_sdf_trace", lambda: L.rm_sdf_trace(_ptr(rays), N, _ptr(dist), None, 9, 9, 9, lo, st, 0.0, 64, 0, _ptr(hits), stream), None),
        ("rm_sdf_sample_blocks", lambda: L.rm_sdf_sample_blocks(_ptr(pts4), N, _ptr(block_dist), None, _ptr(blocks), 1, 1, 1, 1, lo, st, _ptr(samples), stream), None),
        ("rm_sdf_trace_blocks", lambda: L.rm_sdf_trace_blocks(_ptr(rays), N, _ptr(block_dist), None, _ptr(blocks), 1, 1, 1, 1, lo, st, 0.0, 64, 0, _ptr(hits),
                                                              stream), None),
    ]
    ms, launches = C.c_double(), C.c_int()
    assert L.rm_set_timing(1) == abi.RM_OK
    try:
        assert L.rm_get_timing(C.byref(ms), C.byref(launches)) == abi.RM_OK  # forgets what was timed before
        for name, call, path in calls:
            before = L.rm_debug_last_path()
            assert call() == abi.RM_OK, f"{name}: {L.rm_last_error()}"
            assert L.rm_debug_last_path() == (before if path is None else path), name
            assert L.rm_get_timing(C.byref(ms), C.byref(launches)) == abi.RM_OK
            assert launches.value == (0 if path is None else 1), name
        torch.cuda.synchronize()
        assert (probes[:, 36].view(torch.int32) >= 0).all() and torch.isfinite(light).all() and torch.isfinite(ambient[:, 3]).all()
    finally:
        L.rm_set_timing(0)
        torch.cuda.synchronize()
        L.rm_field_destroy(dense)
        L.rm_field_destroy(sparse)


def test_multi_frame_renders_and_the_entries_that_are_no_render_launches(renderer):
    """A third table of the same form.  The multi-frame renders record their path and count as ONE timed launch per call, as the
    header states for each (7 to 11).  rm_rays_order, rm_rays_restore, rm_sdf_mesh and rm_sdf_mesh_blocks are "not a render launch";
    the conversions, the de-interleaves, the post passes and the probes are no `rm_render*` launches, which is all that
    rm_get_timing averages and rm_debug_last_path reports: the path unchanged, nothing timed."""
    from raymarcher_amd.render import batch_arrays
    L, dev, stream = lib(), renderer.device, renderer._stream()
    objs, no, lights, nl, g, s = _scene()
    G, S = C.byref(g), C.byref(s)
    W, H = 16, 8
    cams, globs = batch_arrays([h.make_camera((0.2 * k, 0.1, 3.0), (0, 0, -1), (0, 1, 0), 45.0, W, H) for k in range(2)], g)
    f32, i32 = torch.float32, torch.int32
    frames, bright = torch.empty((2, H, W, 4), dtype=f32, device=dev), torch.empty((2, H, W, 4), dtype=f32, device=dev)
    posted = torch.empty((2, H, W, 4), dtype=f32, device=dev)
    mask, counts = torch.empty((2, H, W), dtype=torch.uint8, device=dev), torch.empty((2,), dtype=i32, device=dev)
    ids, position = torch.empty((2, H, W), dtype=i32, device=dev), torch.empty((2, H, W, 4), dtype=f32, device=dev)
    bytes8, bytes8b = torch.empty((2, H, W, 4), dtype=torch.uint8, device=dev), torch.empty((2, H, W, 4), dtype=torch.uint8, device=dev)
    rays = _rays(dev)
    hits = torch.zeros((N, 8), dtype=f32, device=dev)
    order, ordered, restored = torch.empty((N,), dtype=i32, device=dev), torch.empty((N, 8), dtype=f32, device=dev), torch.empty((N, 8), dtype=f32, device=dev)
    origin, step = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.25, 0.25, 0.25)
    dist = torch.empty((9, 9, 9), dtype=f32, device=dev)
    blocks = torch.zeros((1, 4), dtype=i32, device=dev)
    block_dist = torch.empty((1, 729), dtype=f32, device=dev)
    assert L.rm_sdf_grid(objs, no, G, S, origin, step, 9, 9, 9, _ptr(dist), None, stream) == abi.RM_OK
    assert L.rm_sdf_grid_blocks(objs, no, G, S, origin, step, 1, 1, 1, _ptr(blocks), 1, _ptr(block_dist), None, stream) == abi.RM_OK
    verts, quads = torch.empty((512, 4), dtype=f32, device=dev), torch.empty((1536, 4), dtype=i32, device=dev)
    found = torch.zeros((4,), dtype=i32, device=dev)
    pts3 = torch.zeros((N, 3), dtype=f32, device=dev)
    pts3[:, 0] = torch.linspace(-0.6, 0.6, N, device=dev)
    probe4, probe8 = torch.empty((N, 4), dtype=f32, device=dev), torch.empty((N, 8), dtype=f32, device=dev)
    x = torch.linspace(0.1, 2.0, N, device=dev)
    _, bulb, nb, bulb_lights, nbl, bulb_g = h.scene_mandelbulb(W, H)
    ps = abi.RmPostSettings(1, 0, 1, 1, 0.8)  # the post passes and the conversions read what the renders above them have written

    calls = [
        ("rm_render_supersampled", lambda: L.rm_render_supersampled(cams, globs, 1, 2, objs, no, lights, nl, S, None, W, H, 2, _ptr(frames), _ptr(bright), stream), 7),
        ("rm_render_adaptive", lambda: L.rm_render_adaptive(cams, globs, 1, 2, objs, no, lights, nl, S, None, W, H, 2, 0.05, _ptr(frames), _ptr(bright), _ptr(mask),
                                                            _ptr(counts), stream), 8),
        ("rm_render_accumulated", lambda: L.rm_render_accumulated(cams, globs, 1, 1, 2, objs, no, lights, nl, S, None, W, H, _ptr(frames), _ptr(bright), stream), 9),
        ("rm_render_animated", lambda: L.rm_render_animated(cams, globs, 1, objs, no, 1, lights, nl, 1, 1, 2, S, None, W, H, _ptr(frames), _ptr(bright), stream), 10),
        ("rm_render_gbuffer", lambda: L.rm_render_gbuffer(cams, globs, 1, 2, objs, no, S, W, H, _ptr(frames), _ptr(ids), _ptr(position), stream), 11),
        ("rm_rays_order", lambda: L.rm_rays_order(_ptr(rays), N, 4, 5, _ptr(order), _ptr(ordered), None, stream), None),
        ("rm_rays_restore", lambda: L.rm_rays_restore(_ptr(hits), _ptr(order), N, 32, _ptr(restored), stream), None),
        ("rm_sdf_mesh", lambda: L.rm_sdf_mesh(_ptr(dist), None, 9, 9, 9, origin, step, 0.0, 512, 1536, _ptr(verts), None, _ptr(quads), _ptr(found), stream), None),
        ("rm_sdf_mesh_blocks", lambda: L.rm_sdf_mesh_blocks(_ptr(block_dist), None, _ptr(blocks), 1, 1, 1, 1, origin, step, 0.0, 512, 1536, _ptr(verts), None,
                                                            _ptr(quads), _ptr(found), stream), None),
        ("rm_frame_to_rgba8", lambda: L.rm_frame_to_rgba8(_ptr(bright), _ptr(bytes8), W, H, stream), None),
        ("rm_frames_to_rgba8", lambda: L.rm_frames_to_rgba8(_ptr(bright), _ptr(bytes8), W, H, 2, stream), None),
        ("rm_tiles_to_rgba8", lambda: L.rm_tiles_to_rgba8(_ptr(bright), _ptr(bytes8), W, H, stream), None),
        ("rm_deinterleave", lambda: L.rm_deinterleave(_ptr(bright), _ptr(posted), W, H, 4, 2, 0, stream), None),
        ("rm_deinterleave_rgba8", lambda: L.rm_deinterleave_rgba8(_ptr(bytes8), _ptr(bytes8b), W, H, 4, 2, 0, 1, stream), None),
        ("rm_post_process", lambda: L.rm_post_process(_ptr(bright), _ptr(bright[1]), _ptr(posted), W, H, C.byref(ps), stream), None),
        ("rm_post_process_batch", lambda: L.rm_post_process_batch(_ptr(frames), _ptr(bright), _ptr(posted), W, H, 2, C.byref(ps), 1, stream), None),
        ("rm_probe_math", lambda: L.rm_probe_math(abi.RM_FN_SQRT, _ptr(x), _ptr(x), _ptr(x), _ptr(probe4), N, stream), None),
        ("rm_probe_bump", lambda: L.rm_probe_bump(_ptr(pts3), _ptr(probe4), N, stream), None),
        ("rm_probe_sdscene_variant", lambda: L.rm_probe_sdscene_variant(objs, no, G, S, 0, 0, 1, 0, 0, -1, _ptr(pts3), None, _ptr(probe8), N, stream), None),
        ("rm_probe_pool_cull", lambda: L.rm_probe_pool_cull(bulb, nb, bulb_lights, nbl, C.byref(bulb_g), S, 1, 0, 100.0, _ptr(pts3), _ptr(probe8), N, stream), None),
    ]
    ms, launches = C.c_double(), C.c_int()
    assert L.rm_set_timing(1) == abi.RM_OK
    try:
        assert L.rm_get_timing(C.byref(ms), C.byref(launches)) == abi.RM_OK  # forgets what was timed before
        for name, call, path in calls:
            before = L.rm_debug_last_path()
            assert call() == abi.RM_OK, f"{name}: {L.rm_last_error()}"
            assert L.rm_debug_last_path() == (before if path is None else path), name
            assert L.rm_get_timing(C.byref(ms), C.byref(launches)) == abi.RM_OK
            assert launches.value == (0 if path is None else 1), name
        torch.cuda.synchronize()
        assert 0 < int(found[0]) <= 512 and torch.isfinite(posted).all() and sorted(order.tolist()) == list(range(N))
    finally:
        L.rm_set_timing(0)


def test_more_calls_in_flight_than_the_batch_ring_has_slots(renderer):
    """Six rm_trace_rays calls back to back on one stream, no synchronise between them: the batch ring has four slots, so the fifth
    call must wait for the first slot's launch instead of overwriting its pinned block.  Every result is the first call's."""
    L, dev, stream = lib(), renderer.device, renderer._stream()
    objs, no, _, _, g, s = _scene()
    rays = _rays(dev)
    torch.cuda.synchronize()
    outs = [torch.full((N, 8), float("nan"), dtype=torch.float32, device=dev) for _ in range(6)]
    torch.cuda.synchronize()
    for out in outs:
        assert L.rm_trace_rays(_ptr(rays), N, objs, no, C.byref(g), C.byref(s), abi.RM_TRACE_CLOSEST, _ptr(out), stream) == abi.RM_OK
    torch.cuda.synchronize()
    first = outs[0].cpu().numpy().view(np.uint32)
    ids = first[:, 7].view(np.int32)
    assert (ids == 0).any() and (ids == -1).any(), "the rays should hold hits and misses"
    for k, out in enumerate(outs[1:], 1):
        assert (out.cpu().numpy().view(np.uint32) == first).all(), f"call {k} differs from call 0"
