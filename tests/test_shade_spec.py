"""The specification of rm_shade_rays (tests/shade_spec/rm_shade_spec.c: the oracle's shadePixel from the background colour on,
restated for a given ray with the oracle's own functions) on the CPU, before the GPU tests compare the kernel with it: on a camera's
own primary rays, with far = the camera's, it equals rmo_render_res in every bit of colour and bright, on one scene or more per
kernel class — which pins the restated lines — and it keeps the invariants of the definition.  Then the two host generators that
ship with the entry point, panorama_rays and tile_order."""
import numpy as np
import pytest

import helpers as h
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import abi, panorama_rays, tile_order


# ---------------------------------------------------------------- (a) the spec on a camera's rays is the oracle's frame
@pytest.mark.parametrize("W,H", [(64, 36), (37, 23)])
@pytest.mark.parametrize("name", list(S.CASES))
def test_spec_on_primary_rays_equals_the_oracles_frame_in_every_bit(name, W, H):
    scene, s, res = S.case(name, W, H)
    assert S.class_of(scene, s) == S.CASES[name][0], "the case is not of the class it is listed under"
    rays = T.spec_primary_rays(scene[0], W, H)
    col, br = S.spec_shade(scene, s, rays, scene[0].initialFar, res)
    ref, ref_b = h.oracle_render(scene, s, W, H, bright=True, **res)
    S.assert_bits(col, ref.reshape(-1, 4), f"{name} {W}x{H} colour")
    S.assert_bits(br, ref_b.reshape(-1, 4), f"{name} {W}x{H} bright")
    if name != "empty":
        assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 10, "the frame should not be constant"
    if S.CASES[name][0][3] and name != "env_sec":
        assert ref[..., 3].max() >= 2.0, "a class with secondary rays should show a bounce in its alpha"


# ---------------------------------------------------------------- invariants of the specification
def test_spec_invalid_rays_give_zeros_in_both_outputs():
    scene, s, res = S.case("generic_nosec")
    rays, n_invalid = T.invalid_rays()
    rays = rays[[i for i in range(len(rays)) if not (i < n_invalid and np.isfinite(rays[i, [0, 1, 2, 4, 5, 6]]).all() and
                                                      rays[i, 4:7].any())]]  # tMax is not read: a bad tMax alone is a valid ray
    bad = ~np.isfinite(rays[:, [0, 1, 2, 4, 5, 6]]).all(axis=1) | ~rays[:, 4:7].any(axis=1)
    assert bad.sum() == 20 and (~bad).sum() == 2
    col, br = S.spec_shade(scene, s, rays, 100.0, res)
    assert (T.bits(col[bad]) == 0).all() and (T.bits(br[bad]) == 0).all()
    assert (col[~bad, 3] >= 1.0).all() and (br[~bad, 3] == 1.0).all(), "a valid ray's alpha is >= 1"
    # a ray whose tMax is NaN, negative or −inf is valid here and gives what tMax = 0 gives
    odd, _ = T.invalid_rays()
    odd = odd[n_invalid - 3:n_invalid]
    assert not np.isfinite(odd[:, 3]).all()
    plain = odd.copy()
    plain[:, 3] = 0.0
    for a, b in zip(S.spec_shade(scene, s, odd, 100.0, res), S.spec_shade(scene, s, plain, 100.0, res)):
        S.assert_bits(a, b, "tMax is not read")
        assert (a[:, 3] >= 1.0).all()


@pytest.mark.parametrize("name", ["generic_sec", "plain_bulb_nosec", "tex_sec"])
def test_spec_of_a_shuffled_array_is_the_shuffled_result(name):
    scene, s, res = S.case(name)
    centre, radius = T.cull_bounds(scene[1], scene[2], scene[5])
    rays = T.seeded_rays(np.random.default_rng(5), 600, centre, radius)
    perm = np.random.default_rng(6).permutation(len(rays))
    col, br = S.spec_shade(scene, s, rays, 100.0, res)
    col2, br2 = S.spec_shade(scene, s, rays[perm], 100.0, res)
    S.assert_bits(col2, col[perm], name)
    S.assert_bits(br2, br[perm], name + " bright")
    assert (col[:, 3] == 0).sum() >= 20 and len(np.unique(col, axis=0)) > 50


@pytest.mark.parametrize("feat,what", [(abi.RM_FEAT_WHITE_BACKGROUND, "white"), (abi.RM_FEAT_DARK_BACKGROUND, "dark"),
                                       (abi.RM_FEAT_SKY_BACKGROUND, "sky"),
                                       (abi.RM_FEAT_SKY_BACKGROUND | abi.RM_FEAT_WHITE_BACKGROUND, "white over sky"),
                                       (abi.RM_FEAT_WHITE_BACKGROUND | abi.RM_FEAT_DARK_BACKGROUND, "dark over white")])
def test_spec_of_a_ray_aimed_away_is_exactly_the_background(feat, what):
    scene, _, res = S.case("generic_sec")
    s = abi.default_settings(features=feat, enableReflection=1, enableRefraction=1)
    rng = np.random.default_rng(8)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = T.make_rays(50.0 * d, d, 0.0)  # from 50 units out, pointing outwards: nothing lies ahead
    col, br = S.spec_shade(scene, s, rays, 100.0, res)
    if what in ("white", "white over sky"):
        want = np.ones((200, 3), dtype=np.float32)
    elif what in ("dark", "dark over white"):
        want = np.zeros((200, 3), dtype=np.float32)
    else:
        # getSky through the one-object-free frame of the oracle: an empty table renders the background for every pixel
        empty, _ = h.table([])
        want = S.spec_shade((None, empty, 0, None, 0, scene[5]), s, rays, 100.0)[0][:, 0:3]
        assert len(np.unique(want, axis=0)) > 100, "the sky varies with the direction"
    S.assert_bits(col[:, 0:3], want, what)
    assert (col[:, 3] == 1.0).all()
    S.assert_bits(br, np.tile(np.float32([0, 0, 0, 1]), (200, 1)), what + " bright")


def test_sky_background_of_the_spec_is_the_oracles_sky():
    """The sky of the previous test, pinned to the oracle: an empty table's frame is getSky of every primary ray."""
    W, H = 37, 23
    scene, _, _ = S.case("empty", W, H)
    s = abi.default_settings(features=abi.RM_FEAT_SKY_BACKGROUND)
    col, _ = S.spec_shade(scene, s, T.spec_primary_rays(scene[0], W, H), scene[0].initialFar)
    S.assert_bits(col, h.oracle_render(scene, s, W, H).reshape(-1, 4), "sky")


def test_spec_refuses_what_the_entry_point_refuses():
    scene, s, res = S.case("generic_nosec")
    rays = T.make_rays([[0, 0, 5]], [[0, 0, -1]], 0.0)
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA):
        S.spec_shade(scene, abi.default_settings(features=feat), rays, 100.0, expect=abi.RM_ERR_UNSUPPORTED)
    for far in (np.nan, -1.0, np.inf):
        S.spec_shade(scene, s, rays, far, expect=abi.RM_ERR_INVALID_ARGUMENT)


# ---------------------------------------------------------------- (c) panorama_rays and tile_order
def test_panorama_rays_are_unit_and_laid_out_as_documented():
    W, H = 64, 32
    pos = (0.25, -1.5, 3.0)
    rays = panorama_rays(pos, W, H)
    assert rays.shape == (W * H, 8) and rays.dtype == np.float32
    assert (rays[:, 0:3] == np.float32(pos)).all() and (T.bits(rays[:, 3]) == 0).all() and (T.bits(rays[:, 7]) == 0).all()
    d = rays[:, 4:7].astype(np.float64)
    # rounding three components to float32 costs at most 1.5 · 2^-24 of the length: 2^-22 is a bound with room
    assert np.abs(np.linalg.norm(d, axis=1) - 1.0).max() <= 2.0 ** -22
    d = d.reshape(H, W, 3)
    f, r, u = np.array([0.0, 0.0, -1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
    # the four centre pixels straddle forward symmetrically: the same forward part, right and up parts of opposite sign
    c = d[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1]
    assert (c @ f > 0.99).all() and np.ptp(c @ f) <= 2.0 ** -22
    assert np.abs(c[:, 0] @ r + c[:, 1] @ r).max() <= 2.0 ** -22 and (c[:, 1] @ r > 0).all()
    assert np.abs(c[0] @ u + c[1] @ u).max() <= 2.0 ** -22 and (c[1] @ u > 0).all(), "row 0 is the bottom"
    # column 0 and column W − 1 mirror across −forward: both point backwards, with opposite right parts
    assert (d[:, 0] @ f < 0).all() and np.abs(d[:, 0] @ r + d[:, W - 1] @ r).max() <= 2.0 ** -22
    assert np.abs(d[:, 0] @ f - d[:, W - 1] @ f).max() <= 2.0 ** -22 and (d[:, 0] @ r < 0).all()
    # the rows run from straight down to straight up
    assert (d[0] @ u < -0.99).all() and (d[H - 1] @ u > 0.99).all()


def test_panorama_rays_orient_a_non_axis_basis_as_stated():
    W, H = 40, 20
    fwd, up = np.array([1.0, 0.5, -2.0]), np.array([0.2, 1.0, 0.1])
    rays = panorama_rays((0, 0, 0), W, H, forward=fwd, up=up)
    d = rays[:, 4:7].astype(np.float64).reshape(H, W, 3)
    f = fwd / np.linalg.norm(fwd)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    assert np.abs(np.linalg.norm(d, axis=2) - 1.0).max() <= 2.0 ** -22
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    theta, phi = ((x + 0.5) / W - 0.5) * 2 * np.pi, ((y + 0.5) / H - 0.5) * np.pi
    assert np.abs(d @ r - np.cos(phi) * np.sin(theta)).max() <= 2.0 ** -22
    assert np.abs(d @ u - np.sin(phi)).max() <= 2.0 ** -22
    assert np.abs(d @ f - np.cos(phi) * np.cos(theta)).max() <= 2.0 ** -22
    with pytest.raises(ValueError):
        panorama_rays((0, 0, 0), 8, 4, forward=(0, 2, 0), up=(0, 1, 0))


def test_tile_order_is_a_permutation_of_8x8_tiles():
    order = tile_order(64, 32)
    assert order.dtype == np.int64 and sorted(order.tolist()) == list(range(64 * 32))
    for k in range(0, 64 * 32, 64):
        y, x = np.divmod(order[k:k + 64], 64)
        assert x.min() % 8 == 0 and y.min() % 8 == 0 and np.ptp(x) == 7 and np.ptp(y) == 7, "a run of 64 is one 8×8 tile"
        assert (y * 64 + x == order[k:k + 64]).all() and (np.diff(order[k:k + 8]) == 1).all()
    assert (order[:64:8] == np.arange(8) * 64).all() and order[64] == 8, "tiles in raster order, rows inside a tile"
    ragged = tile_order(37, 23)
    assert sorted(ragged.tolist()) == list(range(37 * 23))
    y, x = np.divmod(ragged, 37)
    tile = (y // 8) * 5 + x // 8
    assert (np.diff(tile) >= 0).all(), "the pixels of a tile stay together, ragged edges included"
    assert sorted(tile_order(5, 3, tile=2).tolist()) == list(range(15))
