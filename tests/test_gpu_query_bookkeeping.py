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
