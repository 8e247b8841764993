"""The batch ring of scene blocks (DeviceState::batches, acquire_slot in rm_launcher.hip) with all of its four slots busy: a slot
is not handed out again while the upload or the launch that reads its pinned block is still in flight.  The older ring tests
(test_gpu_query_bookkeeping, batch_slot_case of test_gpu_write_coverage) stage the same bytes in the calls that would collide, so
an early reuse overwrites a block with itself.  Here every call stages a table of its own and the stream is held by a gate —
torch.cuda._sleep — until the host has issued every call: the fifth call finds four busy slots and has to wait for the oldest,
and a slot rewritten too early gives its launch the table of a later call, which the expectations tell apart.

The ring only grows, once per process: each case runs in a fresh child process under a time limit of its own.  After a child that
was killed, ran into its limit or met a HIP error the module starts nothing further."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import tables_of
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE_CYCLES = 50_000_000  # test_gpu_write_coverage's gate: tens of milliseconds at least
SLOTS = 4                 # the batch ring's maximum
N, K, P = 64, 8, 8        # rays or points, directions per probe, probes
_ABANDONED = []           # why the module stopped starting processes


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def query_ring_case(renderer):
    """Ten staged calls behind the gate on one stream, one of each entry that takes a slot of the batch ring.  Call j stages one
    sphere at x = 0.15·j under a light of its own colour and marches to far = 50 + j."""
    import torch
    from raymarcher_amd import probe_depth_weights, sphere_directions
    L, dev, stream = lib(), renderer.device, renderer._stream()
    s = abi.default_settings()
    g = h.make_globals()
    G, S = C.byref(g), C.byref(s)

    def scene(j):
        objs, no = h.table([h.make_object(abi.RM_SPHERE, model=h.translate(0.15 * j, 0.0, 0.0))])
        lights, nl = h.table([h.make_light(abi.RM_LIGHT_DIRECTIONAL, color=(1.0 - 0.07 * j, 0.3 + 0.06 * j, 0.5 + 0.04 * (j % 3)), direction=(0.3, -1.0, 0.5))],
                             struct=abi.RmLight)
        return objs, no, lights, nl, 50.0 + j

    def rays(far):
        r = np.zeros((N, 8), dtype=np.float32)
        r[:, 0] = np.linspace(-0.7, 1.9, N)  # every sphere of the ten is hit by some and passed by others
        r[:, 1], r[:, 2], r[:, 3], r[:, 6] = 0.1, -3.0, far, 1.0
        return torch.from_numpy(r).to(dev)

    pts = torch.zeros((N, 4), dtype=torch.float32, device=dev)
    pts[:, 0] = torch.linspace(-0.6, 2.0, N, device=dev)
    pts[:, 1] = 0.45
    table_h = sphere_directions(K, 1)
    table = torch.from_numpy(table_h).to(dev)
    weights = torch.from_numpy(probe_depth_weights(table_h, 1)).to(dev)
    corners = [[-1.0 + 3.4 * (i & 1), -1.5 + 3.0 * (i >> 1 & 1), -1.5 + 3.0 * (i >> 2), 1.0] for i in range(P)]
    pos = torch.tensor(corners, dtype=torch.float32, device=dev)
    # the grid that calls 4 and 5 read: the eight probes of scene 0, baked alone
    grid = torch.empty((P, 40), dtype=torch.float32, device=dev)
    o0 = scene(0)
    assert L.rm_light_probes(_ptr(pos), P, _ptr(table), K, 1, 50.0, o0[0], o0[1], o0[2], o0[3], G, S, None, _ptr(grid), stream) == abi.RM_OK
    ref = abi.RmLightGridRef(grid.data_ptr(), None, (C.c_int32 * 3)(2, 2, 2), (C.c_float * 3)(-1.0, -1.5, -1.5), (C.c_float * 3)(3.4, 3.0, 3.0), 1.0,
                             abi.RM_LIGHT_GRID_FACING, 0.0)
    lo, st = (C.c_float * 3)(-1.0, -1.0, -1.0), (C.c_float * 3)(0.3, 0.25, 0.25)
    torch.cuda.synchronize()

    # entry → (shapes of its outputs, call(scene, rays, outputs)); every call takes the stream
    def ps_of(far):
        ps = abi.RmPointsSettings()
        L.rm_points_settings_default(C.byref(ps))
        ps.far = far
        return ps

    entries = [
        ("rm_trace_rays", [(N, 8)], lambda sc, r, o: L.rm_trace_rays(_ptr(r), N, sc[0], sc[1], G, S, abi.RM_TRACE_CLOSEST, _ptr(o[0]), stream)),
        ("rm_shade_rays", [(N, 4)], lambda sc, r, o: L.rm_shade_rays(_ptr(r), N, sc[4], sc[0], sc[1], sc[2], sc[3], G, S, None, _ptr(o[0]), None, stream)),
        ("rm_light_probes", [(P, 40)], lambda sc, r, o: L.rm_light_probes(_ptr(pos), P, _ptr(table), K, 1, sc[4], sc[0], sc[1], sc[2], sc[3], G, S, None, _ptr(o[0]), stream)),
        ("rm_light_probes_depth", [(P, 128)], lambda sc, r, o: L.rm_light_probes_depth(_ptr(pos), P, _ptr(table), _ptr(weights), K, 1, sc[4], sc[0], sc[1], G, S, _ptr(o[0]),
                                                                                        stream)),
        ("rm_shade_rays_indirect", [(N, 4)], lambda sc, r, o: L.rm_shade_rays_indirect(_ptr(r), N, sc[4], sc[0], sc[1], sc[2], sc[3], G, S, None, C.byref(ref), _ptr(o[0]),
                                                                                      stream)),
        ("rm_light_probes_indirect", [(P, 40)], lambda sc, r, o: L.rm_light_probes_indirect(_ptr(pos), P, _ptr(table), K, 1, sc[4], sc[0], sc[1], sc[2], sc[3], G, S, None,
                                                                                           C.byref(ref), _ptr(o[0]), stream)),
        ("rm_shade_points", [(N, 8), (N, 4)], lambda sc, r, o: L.rm_shade_points(_ptr(pts), None, N, C.byref(ps_of(sc[4])), sc[0], sc[1], sc[2], sc[3], G, S, None,
                                                                                _ptr(o[0]), None, _ptr(o[1]), stream)),
        ("rm_sdf_grid", [(9, 9, 9)], lambda sc, r, o: L.rm_sdf_grid(sc[0], sc[1], G, S, lo, st, 9, 9, 9, _ptr(o[0]), None, stream)),
        ("rm_shade_rays_layers", [(N, 4)], lambda sc, r, o: L.rm_shade_rays_layers(_ptr(r), N, sc[4], 8, sc[0], sc[1], sc[2], sc[3], G, S, None, _ptr(o[0]), None, stream)),
        ("rm_trace_rays_layers", [(N, 8)], lambda sc, r, o: L.rm_trace_rays_layers(_ptr(r), N, 8, sc[0], sc[1], G, S, abi.RM_TRACE_CLOSEST, _ptr(o[0]), stream)),
    ]
    scenes = [scene(j) for j in range(len(entries))]
    ray_sets = [rays(sc[4]) for sc in scenes]

    def alone(j, with_scene):
        """Entry j with the table, light and far of call `with_scene`, made alone and synchronised → its outputs' words."""
        name, shapes, call = entries[j]
        outs = [torch.full(shape, float("nan"), dtype=torch.float32, device=dev) for shape in shapes]
        assert call(scenes[with_scene], ray_sets[with_scene], outs) == abi.RM_OK, f"{name}: {L.rm_last_error()}"
        torch.cuda.synchronize()
        return [h.bits(o.cpu().numpy()) for o in outs]

    # every table, buffer and expected result first: nothing but the calls themselves between the gate and the last of them
    expect = [alone(j, j) for j in range(len(entries))]
    for j in range(len(entries) - SLOTS):
        # an early reuse of call j's slot by call j + SLOTS would show: the same entry on that call's table gives other words.
        # That is the assertion that counts.  The second one is the condition as the issue words it — the expectations of calls j
        # and j + SLOTS differ —, which holds trivially where the two entries store records of different kinds.
        later = alone(j, j + SLOTS)
        assert any((a != b).any() for a, b in zip(expect[j], later)), f"{entries[j][0]}: the table of call {j + SLOTS} gives the words of call {j}'s own"
        assert b"".join(a.tobytes() for a in expect[j]) != b"".join(a.tobytes() for a in expect[j + SLOTS]), (j, j + SLOTS)
    bufs = [[h.guarded(shape, device=dev) for shape in shapes] for _, shapes, _ in entries]
    torch.cuda.synchronize()

    torch.cuda._sleep(GATE_CYCLES)
    busy = None
    for j, (name, _, call) in enumerate(entries):
        assert call(scenes[j], ray_sets[j], [out for out, _ in bufs[j]]) == abi.RM_OK, f"{name}: {L.rm_last_error()}"
        if j == SLOTS - 1:
            busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    print(f"stream.query() after call {SLOTS}: {not busy}")
    assert busy, "the gate had ended before the fifth call was issued: the four slots were not busy together"
    for j, (name, _, _) in enumerate(entries):
        for k, (out, check) in enumerate(bufs[j]):
            check()
            got = h.bits(out.cpu().numpy())
            assert (got == expect[j][k]).all(), f"call {j}, {name}, output {k}: {(got != expect[j][k]).sum()} words differ from the same call made alone"


def batch_ring_case(renderer):
    """Six render_batch calls behind the gate, batch j with cameras and globals that no other batch has: an orbit that starts j
    steps further round and iTime offset by j.  Every frame against the oracle, as batch_slot_case holds its own."""
    import torch
    W, H = 64, 40
    scene = h.scene_mandelbulb(W, H)
    s = abi.default_settings(fractalIters=8, maxSteps=96)
    t = tables_of(scene)
    sizes = [3, 2, 3, 1, 3, 2]
    orbit = SB.orbit((0, 0, 4.5), (0, 0, -1), 30.0, W, H, 40, deg=3.0)
    cams = [orbit[5 * j:5 * j + k] for j, k in enumerate(sizes)]
    globs = [[h.with_globals(scene[5], iTime=float(j) + 0.1 * f) for f in range(k)] for j, k in enumerate(sizes)]
    refs = [[h.oracle_render((cams[j][f],) + tuple(scene[1:5]) + (globs[j][f],), s, W, H, bright=True, threads=16) for f in range(k)] for j, k in enumerate(sizes)]
    for j in range(len(sizes) - SLOTS):
        assert (h.bits(refs[j][0][0]) != h.bits(refs[j + SLOTS][0][0])).any(), f"batches {j} and {j + SLOTS} show the same first frame"
    bufs = [(h.guarded((k, H, W, 4), device=renderer.device), h.guarded((k, H, W, 4), device=renderer.device)) for k in sizes]
    torch.cuda.synchronize()
    torch.cuda._sleep(GATE_CYCLES)
    busy = None
    for j, ((out, _), (br, _)) in enumerate(bufs):
        renderer.render_batch(t, s, W, H, cams[j], globals_=globs[j], out=out, out_bright=br)
        if j == SLOTS - 1:
            busy = not torch.cuda.current_stream().query()
    torch.cuda.synchronize()
    print(f"stream.query() after batch {SLOTS}: {not busy}")
    assert busy, "the gate had ended before the fifth batch was issued: the four slots were not busy together"
    for j, (k, ((out, c1), (br, c2))) in enumerate(zip(sizes, bufs)):
        c1()
        c2()
        for f in range(k):
            h.assert_bit_equal(out[f].cpu().numpy(), refs[j][f][0], f"batch {j}, frame {f}")
            h.assert_bit_equal(br[f].cpu().numpy(), refs[j][f][1], f"batch {j}, frame {f} bright")


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_query_ring as t
from raymarcher_amd import Renderer
getattr(t, sys.argv[2])(Renderer(0))
print("ok")
'''


def run_case(case, limit):
    if _ABANDONED:
        pytest.fail(f"not started: {_ABANDONED[0]}")
    t0 = time.perf_counter()
    try:
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, case], capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        _ABANDONED.append(f"{case} did not end within {limit} s")
        pytest.fail(_ABANDONED[0])
    print(f"{case}: process {time.perf_counter() - t0:.2f} s; {p.stdout.strip()[-200:]}")
    if p.returncode < 0 or p.returncode in (134, 139):
        _ABANDONED.append(f"{case} was ended by signal {abs(p.returncode) if p.returncode < 0 else p.returncode - 128}: {p.stderr[-600:]}")
        pytest.fail(_ABANDONED[0])
    if "HIP error" in p.stderr or "hipError" in p.stderr or "RM_ERR_DEVICE" in p.stderr or "device error" in p.stderr:
        _ABANDONED.append(f"{case} met a device error: {p.stderr[-800:]}")
        pytest.fail(_ABANDONED[0])
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-3000:])


def test_ten_staged_queries_in_flight_on_four_slots():
    run_case("query_ring_case", 120)


def test_six_batches_of_their_own_cameras_in_flight_on_four_slots():
    run_case("batch_ring_case", 180)
