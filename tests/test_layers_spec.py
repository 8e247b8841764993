"""The specification of rm_shade_rays_layers and rm_trace_rays_layers (tests/layers_spec/rm_layers_spec.c) without a GPU: on a
camera's primary rays with imageWidth = W it is the oracle's frame in every bit, for every layer scene and mask; without a layer bit
it is the specification of rm_shade_rays and rm_trace_rays; the two specs agree on what a ray sees; every kind of surface is
present in the scenes the GPU tests use; terrain hits lie on the terrain; invalid rays, shuffles and the one role of imageWidth."""
import numpy as np
import pytest

import helpers as h
import layers_helpers as L
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import abi


@pytest.fixture(scope="module")
def frames():
    """name, W, H → the oracle's (colour | bright) rows of the frame, computed once per case and size."""
    cache = {}

    def get(name, W, H):
        if (name, W, H) not in cache:
            scene, s, res = L.case(name, W, H)
            col, br = h.oracle_render(scene, s, W, H, bright=True, **res)
            cache[name, W, H] = np.concatenate([col.reshape(-1, 4), br.reshape(-1, 4)], axis=1)
        return cache[name, W, H]
    return get


def shade(name, W, H, rays, s=None, image_width=None, scene=None):
    sc, s0, res = L.case(name, W, H)
    sc = sc if scene is None else scene
    return np.concatenate(L.spec_shade_layers(sc, s0 if s is None else s, rays, sc[0].initialFar, W if image_width is None else image_width,
                                              res), axis=1)


def trace(name, W, H, rays, s=None, image_width=None, mode="closest", empty=False):
    sc, s0, _ = L.case(name, W, H)
    objs, no = (h.table([])) if empty else (sc[1], sc[2])
    return L.spec_trace_layers(objs, no, sc[5], s0 if s is None else s, rays, W if image_width is None else image_width, mode)


# ---------------------------------------------------------------- (a) the primary rays give the oracle's frame
@pytest.mark.parametrize("W,H", L.SIZES_WH)
@pytest.mark.parametrize("name", L.NAMES)
def test_primary_rays_give_the_oracles_frame(frames, name, W, H):
    want = frames(name, W, H)
    got = shade(name, W, H, L.primary_rays(name, W, H))
    L.assert_bits(got, want, f"{name} {W}x{H}")
    assert np.isfinite(want).all() and len(np.unique(want[:, 0:3], axis=0)) > 50


# ---------------------------------------------------------------- (b) without a layer bit: the specs of rm_shade_rays / rm_trace_rays
@pytest.mark.parametrize("name", ["env_all", "sea_sky"])
def test_without_a_layer_bit_it_is_the_old_specification(name):
    scene, s, res = L.case(name)
    s = L.without_layers(s)
    rays = L.seeded_rays(name)[:1024]
    got = np.concatenate(L.spec_shade_layers(scene, s, rays, 100.0, 7, res), axis=1)
    L.assert_bits(got, np.concatenate(S.spec_shade(scene, s, rays, 100.0, res), axis=1), f"{name} shade")
    for mode in T.MODES:
        L.assert_bits(L.spec_trace_layers(scene[1], scene[2], scene[5], s, rays, 7, mode),
                      T.spec_trace(scene[1], scene[2], scene[5], s, rays, mode), f"{name} trace {mode}")
    # CLOUD alone is accepted by the trace and ignored; occlusion with a layer bit is refused
    cloudy = L.with_features(s, s.features | L.CLOUD)
    L.assert_bits(L.spec_trace_layers(scene[1], scene[2], scene[5], cloudy, rays, 7), T.spec_trace(scene[1], scene[2], scene[5], s, rays),
                  f"{name} trace with CLOUD")
    L.spec_trace_layers(scene[1], scene[2], scene[5], cloudy, rays, 7, "occlusion", expect=abi.RM_ERR_UNSUPPORTED)


# ---------------------------------------------------------------- (c) the two specs agree on what a ray sees
@pytest.mark.parametrize("name", ["env_all", "sea_sky"])
def test_classification_agrees_between_the_two_specs(name):
    W, H = 64, 36
    scene, s, _ = L.case(name, W, H)
    s = L.with_features(s, L.SKY | L.TERRAIN | L.SEA)
    rays = L.primary_rays(name, W, H)
    empty = (scene[0], h.table([])[0], 0, None, 0, scene[5])
    col = np.concatenate(L.spec_shade_layers(empty, s, rays, scene[0].initialFar, W, {"noise": L.shared_noise()}), axis=1)[:, 0:3]
    ids = L.ids_of(trace(name, W, H, rays, s=s, empty=True))
    sky = L.sky_of(rays)
    differs = (L.bits(col) != L.bits(sky)).any(axis=1)
    assert set(np.unique(ids)) <= {-1, L.HIT_SEA, L.HIT_TERRAIN}
    assert (differs == ((ids == L.HIT_SEA) | (ids == L.HIT_TERRAIN))).all()
    assert ((ids == -1) == ~differs).all()
    assert differs.sum() >= 500
    if name == "env_all":  # sea_scene's camera stands below the terrain's height: there every ray ends on a layer
        assert (~differs).sum() >= 100 and (ids == L.HIT_TERRAIN).sum() >= 500
    else:
        assert (ids == L.HIT_SEA).sum() >= 100 and (ids == L.HIT_TERRAIN).sum() >= 100


# ---------------------------------------------------------------- (d) every kind of surface is present
def test_every_kind_is_present(frames):
    """Counted on the CPU oracle at 64×36.  env_scene under SKY | TERRAIN: 1333 pixels that are not sky, of which the trace names
    1303 terrain and 30 the torus; CLOUD changes 566 more pixels' colour.  sea_scene under SKY | SEA: 1920 pixels that are not sky,
    1838 sea and 82 the sphere; 384 sky.  At least half of each must be there (half of the larger figure where two are known: 1333
    terrain, 581 cloud, 1920 sea)."""
    W, H = 64, 36
    rays = L.primary_rays("env_sky_terrain", W, H)
    ids = L.ids_of(trace("env_sky_terrain", W, H, rays))
    clouded = shade("env_sky_terrain", W, H, rays, s=L.with_features(L.case("env_sky_terrain")[1], L.SKY | L.TERRAIN | L.CLOUD))
    changed = (L.bits(clouded) != L.bits(frames("env_sky_terrain", W, H))).any(axis=1)
    print("env_scene: terrain", (ids == L.HIT_TERRAIN).sum(), "cloud-changed", changed.sum(), "objects", (ids >= 0).sum())
    assert (ids == L.HIT_TERRAIN).sum() >= 1333 // 2 + 1 and changed.sum() >= 581 // 2 + 1 and (ids >= 0).sum() >= 30 // 2
    rays = L.primary_rays("sea_sky", W, H)
    ids = L.ids_of(trace("sea_sky", W, H, rays))
    print("sea_scene: sea", (ids == L.HIT_SEA).sum(), "objects", (ids >= 0).sum(), "sky", (ids == -1).sum())
    assert (ids == L.HIT_SEA).sum() >= 1920 // 2 and (ids >= 0).sum() >= 82 // 2 and (ids == -1).sum() >= 384 // 2
    assert (ids == L.HIT_SEA).sum() + (ids >= 0).sum() + (ids == -1).sum() == W * H


# ---------------------------------------------------------------- (e) terrain hits lie on the terrain
# |position.y − height(position.xz)| over the terrain hits of (d)'s rays (env_scene under SKY | TERRAIN, 64×36), measured on the CPU:
# maximum 26.26, median 0.629, over 1303 hits with t up to 1379.  The march stops where the ray is within 0.001·t above the surface
# and interpolates linearly between its last two steps (frag:2060-2090), so the typical gap is of the order of 0.001·t; the largest
# ones are grazing rays on ridges, where the last step dives deep and the chord leaves the surface.  A wrong tmin or bound puts the
# point a march step away: the steps are 0.8 of the height above ground, hundreds of units from this camera.
TERRAIN_GAP_MEASURED, TERRAIN_GAP_MEDIAN_MEASURED = 26.26, 0.629


def test_terrain_hits_lie_on_the_terrain():
    W, H = 64, 36
    hits = trace("env_sky_terrain", W, H, L.primary_rays("env_sky_terrain", W, H))
    on = L.ids_of(hits) == L.HIT_TERRAIN
    p = hits[on, 4:7].astype(np.float64)
    gap = np.abs(p[:, 1] - L.terrain_height(p[:, 0], p[:, 2]).astype(np.float64))
    print("terrain gap: max", gap.max(), "median", np.median(gap), "t max", hits[on, 3].max())
    assert gap.max() <= 4.0 * TERRAIN_GAP_MEASURED and np.median(gap) <= 4.0 * TERRAIN_GAP_MEDIAN_MEASURED
    n = hits[on, 0:3].astype(np.float64)
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5) and (n[:, 1] > 0).all(), "the surface normal points up and is unit"
    assert (hits[on, 3] >= 15.0).all(), "the terrain march starts at tmin = 15"


# ---------------------------------------------------------------- (f) invalid rays and shuffles
@pytest.mark.parametrize("name", ["env_all_sea", "sea_terrain"])
def test_invalid_rays_and_shuffles(name):
    W = 64
    scene, s, res = L.case(name)
    bad, n_invalid = T.invalid_rays()
    hits = trace(name, W, 36, bad)
    assert (L.ids_of(hits)[:n_invalid] == abi.RM_RAY_INVALID).all() and (L.bits(hits[:n_invalid, 0:7]) == 0).all()
    assert (L.ids_of(hits)[n_invalid:] != abi.RM_RAY_INVALID).all()
    col = shade(name, W, 36, bad)
    shade_invalid = np.array([not (np.isfinite(r[0:3]).all() and np.isfinite(r[4:7]).all() and (r[4:7] != 0).any()) for r in bad])
    assert (L.bits(col[shade_invalid]) == 0).all() and (col[~shade_invalid, 3] >= 1.0).all()
    rays = L.seeded_rays(name)[:1024]
    perm = np.random.default_rng(9).permutation(len(rays))
    L.assert_bits(shade(name, W, 36, rays[perm]), shade(name, W, 36, rays)[perm], f"{name} shade shuffled")
    L.assert_bits(trace(name, W, 36, rays[perm]), trace(name, W, 36, rays)[perm], f"{name} trace shuffled")
    ids = L.ids_of(trace(name, W, 36, rays))
    assert (ids == abi.RM_RAY_INVALID).sum() >= 16 and ((ids == L.HIT_SEA) | (ids == L.HIT_TERRAIN)).sum() >= 100
    # without normals: the same id and t, zeros elsewhere
    full, lean = trace(name, W, 36, rays), trace(name, W, 36, rays, mode="no_normal")
    L.assert_bits(lean[:, [3, 7]], full[:, [3, 7]], f"{name} id and t without normals")
    assert (L.bits(lean[:, [0, 1, 2, 4, 5, 6]]) == 0).all()


# ---------------------------------------------------------------- (g) imageWidth matters only for the sea
def test_image_width_matters_only_for_the_sea():
    W, H = 64, 36
    rays = L.primary_rays("env_all", W, H)
    L.assert_bits(shade("env_all", W, H, rays, image_width=1), shade("env_all", W, H, rays, image_width=4096), "TERRAIN | CLOUD colour")
    L.assert_bits(trace("env_all", W, H, rays, image_width=1), trace("env_all", W, H, rays, image_width=4096), "TERRAIN | CLOUD trace")
    rays = L.primary_rays("sea_sky", W, H)
    a, b = shade("sea_sky", W, H, rays, image_width=W), shade("sea_sky", W, H, rays, image_width=4 * W)
    assert (L.bits(a) != L.bits(b)).any(axis=1).sum() >= 500, "the sea's colour reads imageWidth"
    ta, tb = trace("sea_sky", W, H, rays, image_width=W), trace("sea_sky", W, H, rays, image_width=4 * W)
    sea = L.ids_of(ta) == L.HIT_SEA
    L.assert_bits(ta[:, 3:8], tb[:, 3:8], "t, position and id do not read imageWidth")
    assert (L.bits(ta[sea, 0:3]) != L.bits(tb[sea, 0:3])).any(axis=1).sum() >= 500, "the sea's normal reads imageWidth"
    L.assert_bits(ta[~sea], tb[~sea], "object hits and misses do not read imageWidth")
