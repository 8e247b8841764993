"""The lattice queries' definition without a GPU.  First the library's own arithmetic (raymarcher_amd/csrc/rm_field_march.h, the
code the kernels call), run serially by a stand-alone CPU program under the address and undefined-behaviour sanitizers, against the
NumPy specification (tests/field_spec.py) in every bit.  Then properties of the specification alone: the sparse march with every
block listed is the dense march, the list of active blocks loses no hit, the march on a sphere's lattice finds the sphere, and a
sample on a lattice point returns that point's value."""
import numpy as np
import pytest

import field_helpers as Q
import field_spec as F
import sdf_blocks_helpers as K
import sdf_blocks_spec as B

f32 = np.float32


@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    return Q.build_cpu_program(tmp_path_factory.mktemp("field_cpu"))


# ---------------------------------------------------------------- (a) the shared header on the CPU
@pytest.mark.parametrize("name", Q.DENSE_CASES[::2] + list(Q.HANDMADE_DENSE))
def test_the_shared_header_on_the_cpu_equals_the_spec_dense(cpu_program, tmp_path, name):
    dist, ids, origin, step, iso = Q.dense_case(name)
    points, rays = Q.points_for(dist, origin, step, 1500), Q.rays_for(dist, origin, step, iso, 1500)
    for with_ids, steps, normals in ((True, 64, True), (False, 3, False)):
        use = ids if with_ids else None
        got_s, got_h = Q.run_cpu_program(cpu_program, tmp_path, dist, use, origin, step, iso, points, rays, steps, normals)
        Q.assert_records_equal(got_s, F.sample(dist, origin, step, points, use), f"{name}: samples, ids {with_ids}")
        Q.assert_records_equal(got_h, F.trace(dist, origin, step, rays, iso, steps, use, normals=normals), f"{name}: hits, {steps} steps")


@pytest.mark.parametrize("name", Q.BLOCK_CASES)
def test_the_shared_header_on_the_cpu_equals_the_spec_blocks(cpu_program, tmp_path, name):
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    points, rays = Q.points_for(dense, origin, step, 1500), Q.rays_for(dense, origin, step, iso, 1500)
    for label, bl in Q.block_lists(dense, iso).items():
        packed = B.pack_blocks(dense, bl, f32(np.nan))
        packed_ids = B.pack_blocks(ids, bl, np.int32(-9)) if ids is not None else None
        got_s, got_h = Q.run_cpu_program(cpu_program, tmp_path, packed, packed_ids, origin, step, iso, points, rays, 64, True, bl, blocks)
        Q.assert_records_equal(got_s, F.sample(dense, origin, step, points, ids, bl), f"{name}, {label} list: samples")
        Q.assert_records_equal(got_h, F.trace(dense, origin, step, rays, iso, 64, ids, bl), f"{name}, {label} list: hits")


# ---------------------------------------------------------------- (b) the specification alone
@pytest.mark.parametrize("name", Q.BLOCK_CASES)
def test_with_every_block_listed_the_sparse_queries_are_the_dense_ones(name):
    dense, ids, origin, step, iso = K.case(name)
    points, rays = Q.points_for(dense, origin, step, 1500), Q.rays_for(dense, origin, step, iso, 1500)
    for bl in (B.all_blocks(B.blocks_of(dense)), K.messy_list(B.blocks_of(dense))):
        Q.assert_records_equal(F.sample(dense, origin, step, points, ids, bl), F.sample(dense, origin, step, points, ids), f"{name}: samples")
        for steps in (64, 3):
            Q.assert_records_equal(F.trace(dense, origin, step, rays, iso, steps, ids, bl), F.trace(dense, origin, step, rays, iso, steps, ids),
                                   f"{name}: hits, {steps} steps")


def test_an_unlisted_block_is_reported_and_listed_blocks_sample_as_the_dense_lattice():
    dense, ids, origin, step, iso = K.case("bulb_33")  # 64 blocks, some of them without surface
    bl = B.active_blocks(dense, iso)
    points = Q.points_for(dense, origin, step)
    sparse, full = F.sample(dense, origin, step, points, ids, bl), F.sample(dense, origin, step, points, ids)
    unlisted = sparse["objectId"] == F.UNLISTED
    assert unlisted.any() and (~unlisted).sum() > 500
    Q.assert_records_equal(sparse[~unlisted], full[~unlisted], "listed blocks")
    assert (sparse["cell"][unlisted] == full["cell"][unlisted]).all() and (full["objectId"][unlisted] >= 0).all()
    assert (sparse[unlisted].view(np.uint32).reshape(-1, 8)[:, 0:4] == 0).all(), "value and gradient of an unlisted sample are zeros"
    none = F.sample(dense, origin, step, points, ids, np.zeros((0, 4), np.int32))
    assert ((none["objectId"] == F.UNLISTED) == (full["objectId"] >= -1)).all()
    for code in (F.INVALID, F.OUTSIDE):
        rows = full["objectId"] == code
        assert rows.any() and (full[rows].view(np.uint32).reshape(-1, 8)[:, :7] == 0).all()
    misses = F.trace(dense, origin, step, Q.rays_for(dense, origin, step, iso), iso, 64, ids, np.zeros((0, 4), np.int32))
    assert np.isin(misses["objectId"], (F.MISS, F.INVALID)).all(), "with an empty list every valid ray misses"


@pytest.mark.parametrize("blocks", (2, 4, 8))
def test_on_the_active_blocks_a_ray_from_outside_the_surface_gets_the_dense_marchs_hit_or_miss(blocks):
    """Sphere lattices of 2³, 4³ and 8³ blocks; unit directions, so that the march's step is the distance; 256 steps, which no ray
    comes near (asserted), so the budget decides nothing."""
    dense, origin, step = Q.sphere_lattice(8 * blocks + 1)
    iso = 0.001
    bl = B.active_blocks(dense, iso)
    assert 0 < len(bl) < blocks ** 3 or blocks == 2
    rays = Q.rays_for(dense, origin, step, iso, 3000, seed=blocks)
    d = rays[:, 4:7].astype(np.float64)
    length = np.linalg.norm(d, axis=1)
    with np.errstate(all="ignore"):
        rays[:, 4:7] = np.where(length[:, None] > 0, d / length[:, None], d).astype(f32)
        outside = np.linalg.norm(rays[:, 0:3].astype(np.float64), axis=1) - 0.5 > iso  # outside the surface {d = iso}
    stats_s, stats_d = {}, {}
    sparse = F.trace(dense, origin, step, rays, iso, 256, None, bl, stats=stats_s)
    full = F.trace(dense, origin, step, rays, iso, 256, None, None, stats=stats_d)
    assert stats_s["iterations"].max() < 256 and stats_d["iterations"].max() < 256, "every ray terminates within the budget"
    assert stats_s["skips"].max() <= 3 * blocks + 2
    valid = full["objectId"] != F.INVALID
    assert ((sparse["objectId"] == F.INVALID) == ~valid).all()
    rows = valid & outside
    assert rows.sum() > 1500
    assert ((sparse["objectId"][rows] >= 0) == (full["objectId"][rows] >= 0)).all()
    assert (full["objectId"][rows] >= 0).sum() > 200 and (full["objectId"][rows] < 0).sum() > 200


def test_the_march_on_a_spheres_lattice_finds_the_sphere():
    """The 33³ lattice of |p| − 0.5 across ±0.8, iso 0.001; rays from |o| = 3 aimed at uniform targets in ±0.7.  A ray whose closest
    approach to the centre differs from 0.5 by more than one lattice step agrees with the analytic sphere on hit or miss, and a hit's
    t is within 2 cells of the analytic one; the grazing rays left out are at most 20 %."""
    dense, origin, step = Q.sphere_lattice(33)
    rng = np.random.default_rng(11)
    n = 4000
    o = rng.normal(size=(n, 3))
    o = 3.0 * o / np.linalg.norm(o, axis=1)[:, None]
    d = rng.uniform(-0.7, 0.7, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = o, 10.0, d
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    along = -(o * d).sum(axis=1) / (d * d).sum(axis=1)
    closest = np.linalg.norm(o + d * along[:, None], axis=1)
    cell = float(step[0])
    judged = np.abs(closest - 0.5) > cell
    assert (~judged).mean() <= 0.20, f"{(~judged).mean():.1%} of the rays graze the sphere"
    hits = F.trace(dense, origin, step, rays, 0.001, 256)
    hit = hits["objectId"] >= 0
    assert (hit[judged] == (closest[judged] < 0.5)).all()
    rows = judged & hit
    analytic = along[rows] - np.sqrt(0.25 - closest[rows] ** 2) / np.linalg.norm(d[rows], axis=1)
    err = np.abs(hits["t"][rows].astype(np.float64) - analytic) / cell
    assert rows.sum() > 1000 and err.max() <= 2.0, f"|Δt| up to {err.max():.2f} cells"
    # the normal of a hit points out of the sphere, the position is on the ray
    p = hits["position"][rows].astype(np.float64)
    cosine = (hits["normal"][rows] * p).sum(axis=1) / np.linalg.norm(p, axis=1)
    assert cosine.min() > 0.9
    assert np.abs(p - (o[rows] + d[rows] * hits["t"][rows][:, None])).max() < 1e-5


def test_a_sample_on_a_lattice_point_returns_its_stored_bits():
    """origin and step are binary fractions, so u is the integer exactly; the point's own cell has f = 0 on every axis and every lerp
    returns its first argument.  (At u = N the point is corner 1 of the last cell, f = 1, and a + 1·(b − a) is b only up to
    rounding: those points are left out.)"""
    rng = np.random.default_rng(5)
    dist = rng.uniform(-1, 1, (9, 12, 17)).astype(f32)
    origin, step = np.array([-1.0, 0.5, 2.0], f32), np.array([0.25, 0.5, 0.125], f32)
    k, j, i = np.meshgrid(np.arange(8), np.arange(11), np.arange(16), indexing="ij")
    cells = np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1)
    got = F.sample(dist, origin, step, (origin + cells.astype(f32) * step).astype(f32))
    assert (got["cell"] == cells).all() and (got["objectId"] == -1).all()
    assert got["value"].tobytes() == dist[:8, :11, :16].ravel().tobytes()
