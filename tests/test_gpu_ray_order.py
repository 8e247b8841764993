"""rm_rays_order and rm_rays_restore on the GPU against the NumPy specification (tests/ray_order_spec.py) in every bit: keys, order
and sorted rays for every ray family and bit pair at counts around the wave and the sort's tile, into poisoned, guarded buffers,
with each optional output also left out; the same call twice and two streams at once; the restore and its skipped entries; the
sorted trace and shade entries against the unsorted ones; and the library state an ordering must leave alone."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as h
import layers_helpers as L
import ray_order_helpers as R
import ray_order_spec as S
import scene_builders as SB
from raymarcher_amd import abi, camera_rays, lib

pytestmark = pytest.mark.gpu

T = abi.RM_RAYS_ORDER_TILE
COUNTS = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 70001)  # the last: more than 65 536, in case a counter is 16 bits wide
W, H = R.FRAME_W, R.FRAME_H


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@functools.lru_cache(maxsize=None)
def spec_of(name, n, bits):
    """(keys uint64, order int32) of the family's first n rays by the specification, shared and read-only."""
    rays = R.family(name, max(COUNTS))[:n]
    k, o = S.keys(rays, *bits), S.order(rays, *bits)
    k.setflags(write=False)
    o.setflags(write=False)
    return k, o


def order_guarded(renderer, rays, bits, want_sorted=True, want_keys=True):
    """rm_rays_order on a device copy of `rays` into poisoned, guarded buffers, checked → (order, sorted or None, keys or None)
    as numpy arrays."""
    n = len(rays)
    d_rays = torch.from_numpy(np.array(rays)).to(renderer.device)  # a copy: the shared families are read-only
    order, c1 = h.guarded((n,), torch.int32, device=renderer.device)
    srt, c2 = h.guarded((n, 8), device=renderer.device) if want_sorted else (None, None)
    keys, c3 = h.guarded((n,), torch.int64, device=renderer.device) if want_keys else (None, None)
    st = lib().rm_rays_order(ptr(d_rays), n, bits[0], bits[1], ptr(order), ptr(srt), ptr(keys), renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    for c in (c1, c2, c3):
        if c:
            c()
    assert (d_rays.cpu().numpy().view(np.uint32) == np.ascontiguousarray(rays).view(np.uint32)).all(), "the input was written"
    return (order.cpu().numpy(), srt.cpu().numpy() if want_sorted else None,
            keys.cpu().numpy().view(np.uint64) if want_keys else None)


def assert_order(got, rays, want_keys, want_order, what):
    order, srt, keys = got
    if keys is not None:
        bad = keys != want_keys
        assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} keys differ, the first at {np.argwhere(bad)[:5].ravel().tolist()}"
    bad = order != want_order
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} order entries differ, the first at {np.argwhere(bad)[:5].ravel().tolist()}"
    if srt is not None:
        h.assert_bit_equal(srt, np.ascontiguousarray(rays)[want_order], f"{what}: sorted rays")


# ---------------------------------------------------------------- 1. keys, order and sorted rays equal the specification
@pytest.mark.parametrize("bits", S.BIT_PAIRS)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_keys_order_and_sorted_rays_equal_the_spec_in_every_bit(renderer, name, bits):
    rays = R.family(name, max(COUNTS))
    for n in COUNTS:
        want = spec_of(name, n, bits)
        assert_order(order_guarded(renderer, rays[:n], bits), rays[:n], *want, f"{name} {bits} n={n}")


@pytest.mark.parametrize("bits", [(7, 8), (10, 11)])
@pytest.mark.parametrize("name", ["box", "specials"])
def test_each_optional_output_may_be_null(renderer, name, bits):
    rays = R.family(name, max(COUNTS))
    for n in (65, T + 1, 70001):
        want = spec_of(name, n, bits)
        for want_sorted, want_keys in ((False, False), (True, False), (False, True)):
            got = order_guarded(renderer, rays[:n], bits, want_sorted, want_keys)
            assert_order(got, rays[:n], *want, f"{name} {bits} n={n} sorted={want_sorted} keys={want_keys}")


def test_more_tiles_than_one_round_of_the_scan_and_more_rays_than_the_strided_grids(renderer):
    """1025 tiles and a bit: the scan's workgroups take a second round of 1024 tiles, and the bounds' and the keys' kernels (at most
    512 and 2048 workgroups) stride over the rays more than once."""
    n = 1025 * T + 3
    rng = np.random.default_rng(77)
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(-2, 2, (n, 3))
    rays[:, 4:7] = rng.normal(size=(n, 3))
    rays[n - 5, 4:7] = 0.0   # the extremes and a ray that is not valid in the last, partial tile
    rays[n - 2, 0:3] = (9.0, -9.0, 9.0)
    rays[n - 1, 0:3] = (-9.0, 9.0, -9.0)
    assert_order(order_guarded(renderer, rays, (7, 8)), rays, S.keys(rays, 7, 8), S.order(rays, 7, 8), f"n={n}")


def test_the_whole_shuffled_frame_through_the_python_layer(renderer):
    rays, pixels = R.camera_frame()
    rays = np.array(rays)  # a copy: the shared frame is read-only, and the renderer hands the array to torch
    order, srt, keys = renderer.order_rays(rays, 10, 11, keys=True)
    assert order.dtype == torch.int32 and srt.dtype == torch.float32 and keys.dtype == torch.int64
    assert_order((order.cpu().numpy(), srt.cpu().numpy(), keys.cpu().numpy().view(np.uint64)), rays, S.keys(rays, 10, 11), S.order(rays, 10, 11),
                 "camera frame")
    assert S.median_wave_box(order.cpu().numpy(), pixels) <= 512
    alone = renderer.order_rays(rays, sorted_rays=False)  # the default key: 7 and 8 bits
    assert torch.is_tensor(alone) and (alone.cpu().numpy() == S.order(rays, 7, 8)).all()
    o2, k2 = renderer.order_rays(torch.from_numpy(np.array(rays)).to(renderer.device), 0, 11, sorted_rays=False, keys=True)
    assert (o2.cpu().numpy() == S.order(rays, 0, 11)).all() and (k2.cpu().numpy().view(np.uint64) == S.keys(rays, 0, 11)).all()
    empty = renderer.order_rays(np.zeros((0, 8), np.float32))
    assert tuple(empty[0].shape) == (0,) and tuple(empty[1].shape) == (0, 8)


# ---------------------------------------------------------------- 2. repeatable, and streams keep their workspaces apart
def test_the_same_call_twice_gives_the_same_bits(renderer):
    rays = R.family("specials", max(COUNTS))
    a = order_guarded(renderer, rays, (10, 11))
    b = order_guarded(renderer, rays, (10, 11))
    for x, y in zip(a, b):
        assert (x.view(np.uint32) == y.view(np.uint32)).all()


def test_two_streams_with_different_inputs_keep_their_workspaces_apart(renderer):
    a, b = R.family("box", max(COUNTS)), R.family("specials", max(COUNTS))[:3 * T + 5]
    s1, s2 = torch.cuda.Stream(device=renderer.device), torch.cuda.Stream(device=renderer.device)
    da, db = torch.from_numpy(np.array(a)).to(renderer.device), torch.from_numpy(np.array(b)).to(renderer.device)
    torch.cuda.synchronize(renderer.device)
    got = []
    for _ in range(3):  # enqueued alternately, nothing waits in between
        with torch.cuda.stream(s1):
            got.append(("box", a, renderer.order_rays(da, 10, 11, keys=True)))
        with torch.cuda.stream(s2):
            got.append(("specials", b, renderer.order_rays(db, 7, 8, keys=True)))
    torch.cuda.synchronize(renderer.device)
    for name, rays, (order, srt, keys) in got:
        bits = (10, 11) if name == "box" else (7, 8)
        assert_order((order.cpu().numpy(), srt.cpu().numpy(), keys.cpu().numpy().view(np.uint64)), rays, S.keys(rays, *bits), S.order(rays, *bits),
                     f"{name} on its own stream")


# ---------------------------------------------------------------- 3. rm_rays_restore
def _rows(n, words, seed):
    """Seeded rows of every bit pattern but the poison's → float32 (n, words)."""
    a = np.random.default_rng(seed).integers(0, 2 ** 32, (n, words), dtype=np.uint64).astype(np.uint32)
    a[a == h.FLOAT_POISON] = 0
    return a.view(np.float32)


@pytest.mark.parametrize("words", [4, 8])
def test_restore_inverts_the_order(renderer, words):
    for n in (1, 63, 65, T + 1, 70001):
        order = spec_of("box", n, (10, 11))[1]
        rows = _rows(n, words, n + words)
        out, check = h.guarded((n, words), device=renderer.device)
        d_rows, d_order = torch.from_numpy(rows).to(renderer.device), torch.from_numpy(np.array(order)).to(renderer.device)
        st = lib().rm_rays_restore(ptr(d_rows), ptr(d_order), n, 4 * words, ptr(out), renderer._stream())
        assert st == abi.RM_OK, lib().rm_last_error().decode()
        check()
        h.assert_bit_equal(out.cpu().numpy()[order], rows, f"{words} words n={n}")
        back = renderer.restore_order(d_rows, d_order)
        h.assert_bit_equal(back.cpu().numpy(), S.restore(rows, order)[0], f"restore_order, {words} words n={n}")


@pytest.mark.parametrize("words", [4, 8])
def test_restore_skips_entries_out_of_range_and_writes_nothing_past_the_end(renderer, words):
    n = 2 * T + 1
    order = np.array(spec_of("box", n, (7, 8))[1])
    for k, v in ((0, -1), (5, n), (64, n + 1), (T, 2 ** 31 - 1), (T + 1, -2 ** 31), (n - 1, -7)):
        order[k] = v
    rows = _rows(n, words, 99 + words)
    want, written = S.restore(rows, order)
    assert (~written).sum() == 6
    g = h.Guarded((n, words), torch.float32, h.FLOAT_POISON, renderer.device)
    d_rows, d_order = torch.from_numpy(rows).to(renderer.device), torch.from_numpy(order).to(renderer.device)
    assert lib().rm_rays_restore(ptr(d_rows), ptr(d_order), n, 4 * words, ptr(g.payload), renderer._stream()) == abi.RM_OK
    whole = g.buf.cpu().numpy().view(np.uint32)
    lo, hi = g.guard // 4, (g.guard + g.nbytes) // 4
    assert (whole[:lo] == h.FLOAT_POISON).all() and (whole[hi:] == h.FLOAT_POISON).all(), "a guard band was written"
    got = whole[lo:hi].reshape(n, words)
    assert (got[~written] == h.FLOAT_POISON).all(), "a skipped row was written"
    assert (got[written] == want.view(np.uint32)[written]).all()


# ---------------------------------------------------------------- 4. the sorted entries give the unsorted entries' bits
def _scene(name):
    """(tables, settings, shuffled primary rays of the scene's own 96×64 camera, image_width or None)."""
    if name == "sea_terrain":
        scene, s, res = L.case("sea_terrain", W, H)
        tables, iw = h.tables_of(scene, res), W
    else:
        scene = {"primitives": SB.all_primitives_scene, "bulb": h.scene_mandelbulb}[name](W, H)
        tables, s, iw = h.tables_of(scene), abi.default_settings(), None
    rays = camera_rays(scene[0], W, H)[np.random.default_rng(5).permutation(W * H)]
    rays[::97, 4:7] = 0.0      # and a few rays that are not valid, which the sort moves to the end
    rays[::89, 0] = np.nan
    return tables, s, rays, iw


@pytest.mark.parametrize("mode", ["closest", "no_normal", "occlusion"])
@pytest.mark.parametrize("name", ["primitives", "bulb", "sea_terrain"])
def test_trace_rays_sorted_equals_trace_rays_in_every_bit(renderer, name, mode):
    tables, s, rays, iw = _scene(name)
    kw = dict(mode="occlusion") if mode == "occlusion" else dict(normals=mode == "closest")
    if iw is not None and mode == "occlusion":
        with pytest.raises(ValueError):
            renderer.trace_rays_sorted(tables, s, rays, image_width=iw, **kw)
        return
    want = renderer.trace_rays(tables, s, rays, **kw) if iw is None else renderer.trace_rays_layers(tables, s, rays, iw, **kw)
    got = renderer.trace_rays_sorted(tables, s, rays, image_width=iw, **kw)
    for part, a, b in zip(("normal", "t", "position", "object id"), got, want):
        h.assert_bit_equal(a.cpu().numpy(), b.cpu().numpy(), f"{name} {mode}: {part}")
    ids = got[3].cpu().numpy()
    assert (ids == abi.RM_RAY_INVALID).sum() >= len(rays) // 97 and (ids >= 0).sum() > 100, "the frame should hit something"
    coarse = renderer.trace_rays_sorted(tables, s, rays, image_width=iw, origin_bits=0, dir_bits=5, **kw)
    h.assert_bit_equal(coarse[1].cpu().numpy(), want[1].cpu().numpy(), f"{name} {mode}: t with a coarse key")


@pytest.mark.parametrize("name", ["primitives", "bulb", "sea_terrain"])
def test_shade_rays_sorted_equals_shade_rays_in_every_bit(renderer, name):
    tables, s, rays, iw = _scene(name)
    if iw is None:
        want, want_bright = renderer.shade_rays(tables, s, rays, bright=True)
    else:
        want, want_bright = renderer.shade_rays_layers(tables, s, rays, iw, bright=True)
    got, got_bright = renderer.shade_rays_sorted(tables, s, rays, bright=True, image_width=iw)
    h.assert_bit_equal(got.cpu().numpy(), want.cpu().numpy(), f"{name}: colour")
    h.assert_bit_equal(got_bright.cpu().numpy(), want_bright.cpu().numpy(), f"{name}: bright")
    alone = renderer.shade_rays_sorted(tables, s, rays, image_width=iw, origin_bits=7, dir_bits=8)
    h.assert_bit_equal(alone.cpu().numpy(), want.cpu().numpy(), f"{name}: colour alone, a coarser key")
    assert len(np.unique(want.cpu().numpy().view(np.uint32), axis=0)) > 100, "the frame should show something"


# ---------------------------------------------------------------- 5. what an ordering leaves alone
def test_ordering_is_not_a_render_launch(renderer):
    tables, s, rays, _ = _scene("primitives")
    renderer.trace_rays(tables, s, rays[:100])
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    assert path == abi.RM_PATH_TRACE_RAYS
    order, srt = renderer.order_rays(rays)
    renderer.restore_order(srt, order)
    torch.cuda.synchronize(renderer.device)
    assert (lib().rm_debug_last_path(), lib().rm_debug_last_split()) == (path, split)


def test_a_workspace_limit_below_the_need_is_refused_and_the_next_call_works(renderer):
    rays = R.family("box", max(COUNTS))[:3 * T]
    torch.cuda.synchronize(renderer.device)
    assert lib().rm_release_workspaces(C.byref(C.c_ulonglong(0))) == abi.RM_OK  # no buffer of an earlier test that is large enough already
    d_rays = torch.from_numpy(np.array(rays)).to(renderer.device)
    order = torch.full((len(rays),), -5, dtype=torch.int32, device=renderer.device)
    call = lambda: lib().rm_rays_order(ptr(d_rays), len(rays), 10, 11, ptr(order), None, None, renderer._stream())  # noqa: E731
    assert lib().rm_set_workspace_limit(24 * len(rays)) == abi.RM_OK  # the four buffers alone: the histograms do not fit
    try:
        assert call() == abi.RM_ERR_DEVICE and "rm_set_workspace_limit" in lib().rm_last_error().decode()
        assert (order == -5).all(), "a refused call wrote"
        assert lib().rm_set_workspace_limit(24 * len(rays) + (1 << 16)) == abi.RM_OK
        assert call() == abi.RM_OK, lib().rm_last_error().decode()
        assert (order.cpu().numpy() == S.order(rays, 10, 11)).all()
    finally:
        lib().rm_set_workspace_limit(0)
    assert call() == abi.RM_OK and (order.cpu().numpy() == S.order(rays, 10, 11)).all()
