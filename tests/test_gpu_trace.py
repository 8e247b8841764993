"""rm_trace_rays / Renderer.trace_rays on the GPU: all eight words of every RmRayHit bit for bit against the specification
(tests/trace_spec/rm_trace_spec.c: the oracle's own raymarch, getNormal, bumpNormal and softshadow) — closest hit, closest hit
without normals and occlusion, for the three march classes, the sponge prologue, a Sierpinski, wide random tables, an empty table,
the bump bit and maxSteps = 0, on seeded rays from inside, on and far outside the cull ball, with invalid rays among them, at ray
counts around the wave and workgroup sizes, into poisoned, guarded buffers.  Then: a shuffled call gives the shuffled results; a
camera's own rays give rm_render_gbuffer's bits; four launches back to back keep their tables apart; the schedule is path 12 and
the single-frame state is left alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as h
import scene_builders as SB
import trace_helpers as T
from raymarcher_amd import abi, camera_rays, lib
from raymarcher_amd.render import SceneTables

pytestmark = pytest.mark.gpu

N = 4099
SIZES = (1, 63, 64, 65, 257, N)
BUMP, PLAIN = abi.RM_FEAT_WHITE_BACKGROUND | abi.RM_FEAT_PERLIN_BUMP, abi.RM_FEAT_WHITE_BACKGROUND


def _random(seed, max_objects=30):
    return h.table(h.random_tablewalk_objects(np.random.default_rng(seed), max_objects=max_objects, materials=False))


# name → (object table, count, globals, settings).  The random seeds: 7 = 30 objects with scaleFactors 0.14 … 3.6, 0 = 25 objects,
# 9 = 5 objects, 11 = 2 objects (nested and coincident copies among them: helpers.random_tablewalk_objects).
@functools.lru_cache(maxsize=None)
def case(name):
    g = h.make_globals()
    s = abi.default_settings(features=BUMP)
    if name.startswith("random_"):
        objs, n = _random(int(name.split("_")[1]))
        if name.endswith("_nobump"):
            s = abi.default_settings(features=PLAIN)
        if name.endswith("_nosteps"):
            s = abi.default_settings(maxSteps=0)
    elif name == "one_object":
        objs, n = _random(3, max_objects=1)
    elif name in ("plain_bulb", "plain_bulb_nobump"):
        objs, n = h.scene_mandelbulb(8, 8)[1:3]
        s = abi.default_settings(features=PLAIN if name.endswith("_nobump") else BUMP, fractalIters=12)
        assert lib().rm_debug_bulb_plain(objs, 1, C.byref(g)) == 1
    elif name == "moved_bulb":
        objs, n = SB.moved_bulb_scene(8, 8)[1:3]
        s = abi.default_settings(fractalIters=12)
        assert lib().rm_debug_bulb_plain(objs, 1, C.byref(g)) == 0
    elif name == "menger":
        objs, n = SB.menger_scene(8, 8)[1:3]
        g = h.make_globals(itime=7.5)
        s = abi.default_settings(mengerLevels=3)
    elif name == "sierpinski":
        objs, n = h.table([h.make_object(abi.RM_SIERPINSKI, model=h.scale(0.8, 0.8, 0.8), scale_factor=0.8),
                           h.make_object(abi.RM_CUBE, model=h.translate(1.2, 0.1, -0.3) @ h.scale(0.6, 0.6, 0.6), scale_factor=0.6)])
    elif name == "empty":
        objs, n = h.table([])
    else:
        raise KeyError(name)
    return objs, n, g, s


CASES = ["random_7", "random_0", "random_9", "random_11", "one_object", "plain_bulb", "moved_bulb", "menger", "sierpinski", "empty",
         "random_9_nobump", "plain_bulb_nobump", "random_9_nosteps"]


@functools.lru_cache(maxsize=None)
def rays_of(name):
    objs, n, g, _ = case(name)
    centre, radius = T.cull_bounds(objs, n, g)
    rays = T.seeded_rays(np.random.default_rng(1000 + CASES.index(name)), N, centre, radius)
    rays.setflags(write=False)
    return rays


@functools.lru_cache(maxsize=None)
def spec_of(name, mode):
    """The specification's hits of the case's N rays, computed once and shared (read-only)."""
    objs, n, g, s = case(name)
    hits = T.spec_trace(objs, n, g, s, rays_of(name), mode)
    hits.setflags(write=False)
    return hits


def case_tables(name):
    objs, n, g, _ = case(name)
    return h.tables_of((abi.RmCamera(), objs, n, None, 0, g))


def trace_guarded(renderer, name, rays, mode):
    """Renderer.trace_rays into a poisoned, guarded (n, 8) buffer, checked → numpy (n, 8)."""
    out, check = h.guarded((len(rays), 8), device=renderer.device)
    kw = dict(mode="occlusion") if mode == "occlusion" else dict(normals=mode == "closest")
    got = renderer.trace_rays(case_tables(name), case(name)[3], np.array(rays), out=out, **kw)  # a writable copy of the shared rays
    assert len(got) == 4 and got[0].data_ptr() == out.data_ptr() and got[3].dtype == torch.int32
    assert lib().rm_debug_last_path() == 12 and lib().rm_debug_last_split() == 0
    check()
    return out.cpu().numpy()


# ---------------------------------------------------------------- 6. the kernel equals the specification in every bit
@pytest.mark.parametrize("mode", ["closest", "no_normal", "occlusion"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_spec_in_every_bit(renderer, name, mode):
    rays, want = rays_of(name), spec_of(name, mode)
    ids = T.ids_of(want)
    if name not in ("empty", "random_9_nosteps"):
        assert (ids >= 0).sum() >= 40 and (ids == -1).sum() >= 40, "the case should hold hits and misses"
    else:
        assert not (ids >= 0).any()
    assert (ids == abi.RM_RAY_INVALID).sum() >= 100
    for n in SIZES:
        got = trace_guarded(renderer, name, rays[:n], mode)
        T.assert_bits(got, want[:n], f"{name} {mode} {n} rays")
    if mode != "closest":
        assert (T.bits(want[:, 0:3]) == 0).all() and (T.bits(want[:, 4:7]) == 0).all()


def test_rays_may_be_a_device_tensor_and_normals_off_keeps_id_and_t(renderer):
    name = "random_9"
    rays = torch.from_numpy(np.array(rays_of(name)[:257])).to(renderer.device)
    t = case_tables(name)
    nrm, tt, pos, ids = renderer.trace_rays(t, case(name)[3], rays)
    want = spec_of(name, "closest")[:257]
    T.assert_bits(nrm.cpu().numpy(), want[:, 0:3], "normal view")
    T.assert_bits(tt.cpu().numpy(), want[:, 3], "t view")
    T.assert_bits(pos.cpu().numpy(), want[:, 4:7], "position view")
    assert (ids.cpu().numpy() == T.ids_of(want)).all()
    with pytest.raises(ValueError):
        renderer.trace_rays(t, case(name)[3], rays[:, :7])
    with pytest.raises(ValueError):
        renderer.trace_rays(t, case(name)[3], rays, mode="nearest")


# ---------------------------------------------------------------- 7. grouping: a shuffled call gives the shuffled results
@pytest.mark.parametrize("mode", ["closest", "occlusion"])
@pytest.mark.parametrize("name", ["random_7", "random_9", "plain_bulb"])
def test_a_shuffled_call_gives_the_shuffled_results(renderer, name, mode):
    """The table walk is where the wave-uniform single-object path switches on what the lanes of a wave agree on: another set of
    neighbours must not change a bit of any ray's result."""
    rays = rays_of(name)
    perm = np.random.default_rng(77).permutation(N)
    straight = trace_guarded(renderer, name, rays, mode)
    shuffled = trace_guarded(renderer, name, rays[perm], mode)
    T.assert_bits(shuffled, straight[perm], f"{name} {mode} shuffled")
    T.assert_bits(straight, spec_of(name, mode), f"{name} {mode}")


# ---------------------------------------------------------------- 8. a camera's rays give the G-buffer
@pytest.mark.parametrize("W,H", [(64, 36), (37, 23)])
@pytest.mark.parametrize("scene_name", ["directional_light_2", "plain_bulb", "moved_bulb"])
def test_camera_rays_traced_equal_the_gbuffer(renderer, scene_name, W, H):
    scene = {"directional_light_2": SB.directional_light_2, "plain_bulb": h.scene_mandelbulb, "moved_bulb": SB.moved_bulb_scene}[scene_name](W, H)
    t = SceneTables(*scene)
    s = abi.default_settings()
    nd, ids, pos = renderer.render_gbuffer(t, s, W, H, position=True)
    nd, ids, pos = nd.cpu().numpy().reshape(-1, 4), ids.cpu().numpy().reshape(-1), pos.cpu().numpy().reshape(-1, 4)
    out, check = h.guarded((W * H, 8), device=renderer.device)
    renderer.trace_rays(t, s, camera_rays(scene[0], W, H), out=out)
    check()
    got = out.cpu().numpy()
    assert 0 < (ids >= 0).sum() < W * H
    assert (T.ids_of(got) == ids).all()
    T.assert_bits(got[:, 0:4], nd, f"{scene_name} normal and depth")  # a miss: zeros and far = tMax
    T.assert_bits(got[:, 4:7], pos[:, 0:3], f"{scene_name} position")


# ---------------------------------------------------------------- 9. launch state
def test_four_launches_back_to_back_keep_their_tables_apart(renderer):
    names = ["random_7", "plain_bulb", "menger", "random_9"]
    n = 257
    outs = [h.guarded((n, 8), device=renderer.device) for _ in names]
    dev = [torch.from_numpy(np.array(rays_of(name)[:n])).to(renderer.device) for name in names]
    torch.cuda.synchronize()
    for name, (out, _), rays in zip(names, outs, dev):  # nothing waits between the four
        renderer.trace_rays(case_tables(name), case(name)[3], rays, out=out)
    assert lib().rm_debug_last_path() == 12
    for name, (out, check) in zip(names, outs):
        check()
        T.assert_bits(out.cpu().numpy(), spec_of(name, "closest")[:n], f"{name} among four launches")


def test_single_frames_before_and_after_are_the_same_bits(renderer):
    W, H = 64, 36
    t = SceneTables(*SB.directional_light_2(W, H))
    s = abi.default_settings(enableSoftShadow=1)
    before = renderer.render(t, s, W, H).cpu().numpy()
    path = lib().rm_debug_last_path()
    for mode in ("closest", "occlusion"):
        trace_guarded(renderer, "random_9", rays_of("random_9")[:257], mode)
    assert lib().rm_debug_last_path() == 12
    after = renderer.render(t, s, W, H).cpu().numpy()
    assert lib().rm_debug_last_path() == path
    T.assert_bits(after, before, "a single frame around rm_trace_rays")


def test_pick_agrees_with_the_gbuffers_centre_pixel(renderer):
    W, H = 64, 36
    scene = SB.directional_light_2(W, H)
    t = SceneTables(*scene)
    s = abi.default_settings()
    nd, ids, pos = renderer.render_gbuffer(t, s, W, H, position=True)
    nd, ids, pos = nd.cpu().numpy()[0], ids.cpu().numpy()[0], pos.cpu().numpy()[0]
    hit = np.argwhere(ids >= 0)
    miss = np.argwhere(ids < 0)
    for y, x in [(H // 2, W // 2), tuple(hit[len(hit) // 2]), tuple(miss[0])]:
        oid, p, nrm, tt = renderer.pick(t, s, W, H, int(x), int(y))
        assert oid == ids[y, x]
        assert np.float32(tt).view(np.uint32) == nd[y, x, 3].view(np.uint32)
        T.assert_bits(np.array(p, dtype=np.float32), pos[y, x, 0:3], "picked position")
        T.assert_bits(np.array(nrm, dtype=np.float32), nd[y, x, 0:3], "picked normal")
    assert ids[H // 2, W // 2] >= 0 or len(hit) > 0
    # another camera than the scene's own
    cam = h.make_camera((0.5, 1.0, 6.0), (-0.5, -1.0, -6.0), (0, 1, 0), 35.0, W, H)
    nd2, ids2 = renderer.render_gbuffer(t, s, W, H, cameras=[cam])
    oid, p, nrm, tt = renderer.pick(t, s, W, H, W // 2, H // 2, camera=cam)
    assert oid == int(ids2[0, H // 2, W // 2]) and np.float32(tt).view(np.uint32) == nd2[0, H // 2, W // 2, 3].cpu().numpy().view(np.uint32)
