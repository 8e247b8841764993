"""The HIP post passes (rm_post.hip) and the three RGBA8 conversions (rm_kernels.hip) on the values and at the sizes where they can
be wrong without the rest of the suite noticing: the value atlas of test_post_values.py (NaN, ±inf, negatives, the binary16 range
and its ties, every 8-bit store tie) through every pass selection; containment of a NaN or +inf texel; no bleed between the frames
of a batch; every frame size around the 64×32 blur tiles (4-texel apron), the 256-pixel row blocks of the fused last pass and the
16×16 FXAA blocks, with bright texels on the seams; and the bloom impulse response against float64.

GPU against the oracle is bit for bit.  The one allowance, wherever a float output can be NaN: a NaN on both sides counts as equal
(the contract does not fix the sign or payload of a NaN that arithmetic produces).  Byte outputs get no allowance and
are held to exact arithmetic (test_post_values.store8_exact), not to the oracle."""
import functools

import numpy as np
import pytest

import helpers as h
import test_post_values as V
from helpers import assert_bit_equal as assert_bits
from scene_builders import POST_CASES
from raymarcher_amd import abi

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = np.array([0x7FC00000], dtype=np.uint32).view(F32)[0]


def post_of(name):
    return abi.RmPostSettings(**{"exposure": 1.0, **POST_CASES[name]})


def device(renderer, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(renderer.device) for a in arrays]


def assert_same(got, ref, what):
    """Bit equality, a NaN on both sides counting as equal."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == F32, what
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {i}: got {got[i]!r} "
                             f"({int(got.view(np.uint32)[i]):#010x}), expected {ref[i]!r} ({int(ref.view(np.uint32)[i]):#010x})")


def ordinary(W, H, seed=0, N=None):
    """Random frames with values up to 1.6 and their sparse BrightColor planes, as the existing synthetic post tests build them."""
    rng = np.random.default_rng(seed * 7919 + W * 1000 + H)
    shape = (H, W, 4) if N is None else (N, H, W, 4)
    frag = rng.random(shape, dtype=F32) * F32(1.6)
    frag[..., 3] = 1.0
    luma = (frag[..., :3] * np.array([0.2126, 0.7152, 0.0722], dtype=F32)).sum(-1, keepdims=True)
    bright = np.where(luma > 1.0, frag, F32(0.0)).astype(F32)
    bright[..., 3] = 1.0
    return frag, bright


# ---------------------------------------------------------------- 1. the atlas through every pass selection
@pytest.mark.parametrize("plane", ["frag", "bright"])
@pytest.mark.parametrize("name", list(POST_CASES))
def test_atlas_through_every_pass_selection(renderer, name, plane):
    frag, bright = ordinary(V.ATLAS_W, V.ATLAS_H, seed=3)
    if plane == "frag":
        frag = V.value_atlas()
    else:
        bright = V.value_atlas()
    post = post_of(name)
    fd, bd = device(renderer, frag, bright)
    out = renderer.post_process(fd, bd, post)
    got = out.cpu().numpy()
    ref = h.oracle_post(frag, bright, post)
    assert_same(got, ref, f"{name}, atlas in {plane}")
    img = renderer.to_rgba8(out).cpu().numpy()
    exp = V.store8_exact(ref[::-1])
    assert (img == exp).all(), (name, plane, np.argwhere(img != exp)[:4])


# ---------------------------------------------------------------- 2. the three RGBA8 conversions
def test_rgba8_conversions_on_the_atlas_and_the_ties(renderer):
    """rm_frame_to_rgba8, rm_frames_to_rgba8 (N = 3) and rm_tiles_to_rgba8 on the atlas (all four channels: every tie triple,
    NaN → 0, ±inf, negatives) against exact arithmetic; the first two flip each frame within itself, the third does not."""
    import torch
    a = V.value_atlas()
    t = np.zeros((24, 33, 4), dtype=F32)  # the tie triples once more, in order, at an odd width
    t.reshape(-1)[:765] = V.tie_triples()
    for frame in (a, t):
        d, = device(renderer, frame)
        assert (renderer.to_rgba8(d).cpu().numpy() == V.store8_exact(frame[::-1])).all()
        assert (renderer.tiles_to_rgba8(d).cpu().numpy() == V.store8_exact(frame)).all()
    frames = np.stack([a, a[::-1, ::-1], np.roll(a, 7, axis=1)])
    d, = device(renderer, frames)
    got = renderer.to_rgba8_batch(d).cpu().numpy()
    assert (got == V.store8_exact(frames[:, ::-1])).all()
    assert torch.equal(renderer.to_rgba8_batch(d)[1], renderer.to_rgba8(d[1]))


# ---------------------------------------------------------------- 3. containment
CONTAIN_W, CONTAIN_H = 200, 80


@pytest.mark.parametrize("x,y", [(0, 0), (CONTAIN_W - 1, CONTAIN_H - 1), (64, 32)])
def test_a_nonfinite_texel_stays_inside_its_footprint(renderer, x, y):
    """Bloom + HDR without FXAA.  A NaN or +inf texel of BrightColor can reach 5 horizontal passes × 4 texels = 20 columns and
    4 vertical passes × 4 texels = 16 rows: every output texel farther away than that in either axis equals, bit for bit, the
    output of the same frame with that texel 0.  A NaN texel of the frame itself changes that output texel only."""
    frag, bright = ordinary(CONTAIN_W, CONTAIN_H, seed=5)
    post = post_of("bloom")
    post.enableHDR = 1
    bright[y, x] = 0
    frag0 = frag.copy()
    frag0[y, x] = 0
    fd, bd = device(renderer, frag0, bright)
    base = renderer.post_process(fd, bd, post).cpu().numpy()
    assert np.isfinite(base).all()
    yy, xx = np.mgrid[0:CONTAIN_H, 0:CONTAIN_W]
    outside = (np.abs(xx - x) > 20) | (np.abs(yy - y) > 16)
    for v in (NAN, F32(np.inf)):
        b = bright.copy()
        b[y, x, :3] = v
        got = renderer.post_process(fd, device(renderer, b)[0], post).cpu().numpy()
        assert_bits(got[outside], base[outside], f"bright texel {v} at ({x}, {y})")
        assert not (got[y, x, :3] == base[y, x, :3]).all()  # it did reach its own texel: 1 − exp2(NaN) = 1 − exp(−inf) = 1
        assert (got[y, x, :3] == 1).all()
    f = frag0.copy()
    f[y, x] = NAN
    got = renderer.post_process(device(renderer, f)[0], bd, post).cpu().numpy()
    elsewhere = np.ones((CONTAIN_H, CONTAIN_W), dtype=bool)
    elsewhere[y, x] = False
    assert_bits(got[elsewhere], base[elsewhere], f"frag NaN at ({x}, {y})")
    assert (got[y, x] == 1).all()


# ---------------------------------------------------------------- 4. no bleed between the frames of a batch
BATCH_W, BATCH_H = 70, 40


@functools.lru_cache(maxsize=None)
def batch_frames():
    return ordinary(BATCH_W, BATCH_H, seed=9, N=66)


_single = {}


def single_outputs(renderer, name):
    """rm_post_process of each of the 66 ordinary frames, once per settings."""
    if name not in _single:
        import torch
        fd, bd = device(renderer, *batch_frames())
        _single[name] = torch.stack([renderer.post_process(fd[f], bd[f], post_of(name)) for f in range(66)]).cpu().numpy()
    return _single[name]


@pytest.mark.parametrize("name", ["bloom_hdr_fxaa", "bloom", "gamma_fxaa"])
@pytest.mark.parametrize("N,at", [(3, 0), (3, 2), (66, 0), (66, 65), (66, 63), (66, 64)])
def test_a_nan_frame_does_not_bleed_into_its_batch(renderer, N, at, name):
    """One frame NaN in both planes, first, last, or on either side of the 64-frame chunk edge: every other frame's output equals
    its own rm_post_process bit for bit, out of place and in place; the NaN frame equals its own rm_post_process too."""
    frag, bright = (p[:N].copy() for p in batch_frames())
    frag[at] = NAN
    bright[at] = NAN
    want = single_outputs(renderer, name)[:N]
    post = post_of(name)
    fd, bd = device(renderer, frag, bright)
    nan_single = renderer.post_process(fd[at], bd[at], post).cpu().numpy()
    others = np.arange(N) != at
    for in_place in (False, True):
        out = renderer.post_process_batch(fd, bd, post, out=fd if in_place else None).cpu().numpy()
        assert_bits(out[others], want[others], f"{name} N={N} NaN frame {at} in_place={in_place}")
        assert_same(out[at], nan_single, f"{name} N={N}: the NaN frame itself, in_place={in_place}")


# ---------------------------------------------------------------- 5. seam sweep
SEAM_W = [1, 2, 4, 5, 8, 9, 15, 16, 17, 63, 64, 65, 68, 69, 127, 128, 129, 255, 256, 257, 260, 261, 264, 265]
SEAM_H = [1, 2, 4, 5, 9, 15, 16, 17, 31, 32, 33, 36, 37, 64, 65]


def seam_frame(W, H):
    """A random frame as ordinary(), with bright texels (colour 1..3 per channel, so they pass the bright threshold) forced onto
    every corner, the last row and column, columns 63, 64, 255, 256 and rows 31, 32 — wherever the frame has them."""
    frag, bright = ordinary(W, H, seed=11)
    rng = np.random.default_rng(W * 131 + H)
    hot = np.zeros((H, W), dtype=bool)
    hot[[0, 0, -1, -1], [0, -1, 0, -1]] = True
    hot[-1, :] = True
    hot[:, -1] = True
    for x in (63, 64, 255, 256):
        if x < W:
            hot[:, x] = True
    for y in (31, 32):
        if y < H:
            hot[y, :] = True
    v = (F32(1.0) + rng.random((H, W, 4), dtype=F32) * F32(2.0))
    v[..., 3] = 1.0
    frag[hot] = v[hot]
    bright[hot] = v[hot]
    return frag, bright


@pytest.mark.parametrize("W", sorted(SEAM_W, reverse=True))  # largest first: the grow-only post workspace is allocated once
def test_seam_sweep(renderer, W):
    for H in sorted(SEAM_H, reverse=True):
        frag, bright = seam_frame(W, H)
        fd, bd = device(renderer, frag, bright)
        for name in ("bloom_hdr_fxaa", "bloom"):
            post = post_of(name)
            got = renderer.post_process(fd, bd, post).cpu().numpy()
            assert_same(got, h.oracle_post(frag, bright, post), f"{name} {W}x{H}")


# ---------------------------------------------------------------- 6. the bloom impulse response
@pytest.mark.parametrize("x,y", V.IMPULSE_POSITIONS)
def test_bloom_impulse_response(renderer, x, y):
    """The impulse frames of test_post_values.py: the HIP passes within the derived float64 tolerance of the documented kernel
    (impulse_expected), and bit-equal to the oracle."""
    frag, bright = V.impulse_frames(x, y)
    post = V.post_of(enableBloom=1, enableHDR=1, exposure=1.0)
    fd, bd = device(renderer, frag, bright)
    got = renderer.post_process(fd, bd, post).cpu().numpy()
    V.check_impulse(got, x, y, "HIP")
    assert_bits(got, h.oracle_post(frag, bright, post), f"impulse at ({x}, {y})")
