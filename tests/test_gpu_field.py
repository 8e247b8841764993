"""rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace and rm_sdf_trace_blocks on the GPU against the NumPy specification
(tests/field_spec.py) in every bit: the oracle's lattices and hand-made ones with NaN, infinities and values equal to iso, points and
rays that reach every branch of the definition, every output between guard words; then cross-checks on the device and the Python
layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_helpers as Q
import field_spec as F
import helpers as h
import sdf_blocks_helpers as K
import sdf_blocks_spec as B
import sdf_helpers as V
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu
f32 = np.float32


def vec(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def up(renderer, a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to(renderer.device) if a is not None else None  # a copy: shared arrays are read-only


class Lattice:
    """A lattice on the device: dense (dist (nz, ny, nx)), or with a block list the packed slots of that dense lattice — void slots
    hold NaN and the id −9, which no query may read."""

    def __init__(self, renderer, dense, ids, origin, step, block_list=None):
        self.r, self.origin, self.step = renderer, origin, step
        self.sparse = block_list is not None
        if self.sparse:
            self.dims = B.blocks_of(dense)
            self.bl = up(renderer, block_list, np.int32)
            self.dist = up(renderer, B.pack_blocks(dense, block_list, f32(np.nan)), f32)
            self.ids = up(renderer, B.pack_blocks(ids, block_list, np.int32(-9)), np.int32) if ids is not None else None
        else:
            self.dims, self.bl = dense.shape[::-1], None
            self.dist, self.ids = up(renderer, dense, f32), up(renderer, ids, np.int32)

    def _head(self, with_ids):
        ids = ptr(self.ids) if with_ids else None
        if self.sparse:
            return (ptr(self.dist), ids, ptr(self.bl), len(self.bl), *self.dims, vec(self.origin), vec(self.step))
        return (ptr(self.dist), ids, *self.dims, vec(self.origin), vec(self.step))

    def sample(self, points, with_ids=True):
        """The C entry point into a poisoned, guarded output → SAMPLE records; every word written, no guard word touched."""
        pts = points if torch.is_tensor(points) else up(self.r, points, f32)
        g = h.Guarded((len(pts), 8), torch.float32, h.FLOAT_POISON, self.r.device)
        fn = lib().rm_sdf_sample_blocks if self.sparse else lib().rm_sdf_sample
        path = lib().rm_debug_last_path()
        st = fn(ptr(pts), len(pts), *self._head(with_ids), ptr(g.payload), self.r._stream())
        assert st == abi.RM_OK, lib().rm_last_error().decode()
        g.check()
        assert lib().rm_debug_last_path() == path, "not a render launch"
        return g.payload.cpu().numpy().view(F.SAMPLE).reshape(-1)

    def trace(self, rays, iso, steps, with_ids=True, normals=True):
        rs = rays if torch.is_tensor(rays) else up(self.r, rays, f32)
        g = h.Guarded((len(rs), 8), torch.float32, h.FLOAT_POISON, self.r.device)
        fn = lib().rm_sdf_trace_blocks if self.sparse else lib().rm_sdf_trace
        path = lib().rm_debug_last_path()
        st = fn(ptr(rs), len(rs), *self._head(with_ids), float(iso), steps, abi.RM_TRACE_CLOSEST if normals else abi.RM_TRACE_NO_NORMAL,
                ptr(g.payload), self.r._stream())
        assert st == abi.RM_OK, lib().rm_last_error().decode()
        g.check()
        assert lib().rm_debug_last_path() == path, "not a render launch"
        return g.payload.cpu().numpy().view(F.HIT).reshape(-1)


# ---------------------------------------------------------------- against the specification
@pytest.mark.parametrize("name", Q.DENSE_CASES + list(Q.HANDMADE_DENSE))
def test_dense_queries_equal_the_spec(renderer, name):
    dist, ids, origin, step, iso = Q.dense_case(name)
    points, rays = Q.points_for(dist, origin, step), Q.rays_for(dist, origin, step, iso)
    lat = Lattice(renderer, dist, ids, origin, step)
    for with_ids in (True, False) if ids is not None else (False,):
        use = ids if with_ids else None
        Q.assert_records_equal(lat.sample(points, with_ids), F.sample(dist, origin, step, points, use), f"{name}: samples, ids {with_ids}")
        Q.assert_records_equal(lat.trace(rays, iso, 64, with_ids), F.trace(dist, origin, step, rays, iso, 64, use), f"{name}: hits, ids {with_ids}")


@pytest.mark.parametrize("name", Q.BLOCK_CASES)
def test_block_queries_equal_the_spec(renderer, name):
    dense, ids, origin, step, iso = K.case(name)
    points, rays = Q.points_for(dense, origin, step), Q.rays_for(dense, origin, step, iso)
    for label, bl in Q.block_lists(dense, iso).items():
        lat = Lattice(renderer, dense, ids, origin, step, bl)
        want_s, want_h = F.sample(dense, origin, step, points, ids, bl), F.trace(dense, origin, step, rays, iso, 64, ids, bl)
        Q.assert_records_equal(lat.sample(points, ids is not None), want_s, f"{name}, {label} list: samples")
        Q.assert_records_equal(lat.trace(rays, iso, 64, ids is not None), want_h, f"{name}, {label} list: hits")
        if label == "active" and name == "bulb_33":
            assert (want_s["objectId"] == F.UNLISTED).any() and (want_h["objectId"] >= 0).sum() > 100
        if label == "empty":
            assert np.isin(want_h["objectId"], (F.MISS, F.INVALID)).all()


@pytest.mark.parametrize("name", ("bulb_plain_33x25x17", "bulb_33"))
def test_a_budget_of_three_steps_binds(renderer, name):
    sparse = name in Q.BLOCK_CASES
    dense, ids, origin, step, iso = K.case(name) if sparse else Q.dense_case(name)
    bl = B.active_blocks(dense, iso) if sparse else None
    rays = Q.rays_for(dense, origin, step, iso)
    lat = Lattice(renderer, dense, ids, origin, step, bl)
    want = F.trace(dense, origin, step, rays, iso, 3, ids, bl)
    assert ((want["objectId"] >= 0) != (F.trace(dense, origin, step, rays, iso, 64, ids, bl)["objectId"] >= 0)).sum() > 50, "the budget decides"
    Q.assert_records_equal(lat.trace(rays, iso, 3), want, f"{name}: three steps")
    none = lat.trace(rays, iso, 0)
    assert np.isin(none["objectId"], (F.MISS, F.INVALID)).all()
    Q.assert_records_equal(none, F.trace(dense, origin, step, rays, iso, 0, ids, bl), f"{name}: no step")


@pytest.mark.parametrize("name", ("sphere_cube_17x13x9", "menger_33"))
def test_no_normal_changes_only_normal_and_position_and_one_record_is_a_call(renderer, name):
    sparse = name in Q.BLOCK_CASES
    dense, ids, origin, step, iso = K.case(name) if sparse else Q.dense_case(name)
    bl = B.active_blocks(dense, iso) if sparse else None
    points, rays = Q.points_for(dense, origin, step), Q.rays_for(dense, origin, step, iso)
    lat = Lattice(renderer, dense, ids, origin, step, bl)
    full, bare = lat.trace(rays, iso, 64), lat.trace(rays, iso, 64, normals=False)
    assert (full["objectId"] >= 0).sum() > 100
    Q.assert_records_equal(bare, F.trace(dense, origin, step, rays, iso, 64, ids, bl, normals=False), f"{name}: without normals")
    assert (h.bits(bare["t"]) == h.bits(full["t"])).all() and (bare["objectId"] == full["objectId"]).all()
    assert (h.bits(bare["normal"]) == 0).all() and (h.bits(bare["position"]) == 0).all()
    # one point, one ray: the first of each kind that does something
    hit = int(np.nonzero(full["objectId"] >= 0)[0][0])
    Q.assert_records_equal(lat.trace(rays[hit:hit + 1], iso, 64), full[hit:hit + 1], f"{name}: one ray")
    samples = lat.sample(points)
    inside = int(np.nonzero(samples["objectId"] >= 0)[0][0])
    Q.assert_records_equal(lat.sample(points[inside:inside + 1]), samples[inside:inside + 1], f"{name}: one point")


# ---------------------------------------------------------------- cross-checks on the device
def test_the_sparse_entries_against_the_dense_ones_and_a_permuted_input(renderer):
    dense, ids, origin, step, iso = K.case("bulb_33")
    points, rays = Q.points_for(dense, origin, step), Q.rays_for(dense, origin, step, iso)
    d = Lattice(renderer, dense, ids, origin, step)
    act = Lattice(renderer, dense, ids, origin, step, B.active_blocks(dense, iso))
    every = Lattice(renderer, dense, ids, origin, step, K.messy_list(B.blocks_of(dense)))
    ds, ss = d.sample(points), act.sample(points)
    listed = ss["objectId"] != F.UNLISTED
    assert (~listed).any() and listed.sum() > 1000
    Q.assert_records_equal(ss[listed], ds[listed], "sample_blocks against sample where the block is listed")
    Q.assert_records_equal(every.sample(points), ds, "sample_blocks with every block listed")
    dh = d.trace(rays, iso, 64)
    Q.assert_records_equal(every.trace(rays, iso, 64), dh, "trace_blocks with every block listed against trace")
    # a point's or ray's result does not depend on its neighbours
    perm = np.random.default_rng(9).permutation(Q.NUM)
    ah = act.trace(rays, iso, 64)
    Q.assert_records_equal(act.trace(rays[perm], iso, 64), ah[perm], "permuted rays, sparse")
    Q.assert_records_equal(d.trace(rays[perm], iso, 64), dh[perm], "permuted rays, dense")
    Q.assert_records_equal(act.sample(points[perm]), ss[perm], "permuted points, sparse")
    Q.assert_records_equal(d.sample(points[perm]), ds[perm], "permuted points, dense")


# ---------------------------------------------------------------- the Python layer
def test_the_renderers_methods_and_scene_field_sparse(renderer):
    objs, no, g, s = V.scene("bulb_plain")
    t = h.tables_of((abi.RmCamera(), objs, no, None, 0, g))
    lo, hi = V.BOXES["bulb_plain"]
    grid, gids, bl, blocks, origin, step = renderer.scene_field_sparse(t, s, 36, iso=0.001, bounds=(lo, hi))
    n = bl.shape[0]
    assert tuple(grid.shape) == (n, 9, 9, 9) and tuple(gids.shape) == (n, 9, 9, 9) and 0 < n < int(np.prod(blocks)) and len(step) == 3
    dims = tuple(8 * m + 1 for m in blocks)
    dense, dids = renderer.sdf_grid(t, s, origin, step, dims, ids=True)
    o32, s32 = np.asarray(origin, f32), np.asarray(step, f32)
    points = Q.points_for(dense.cpu().numpy(), o32, s32, 1500)
    rays = Q.rays_for(dense.cpu().numpy(), o32, s32, 0.001, 1500)
    gs, vs, cs, os_ = renderer.sample_lattice_blocks(grid, bl, blocks, origin, step, points, ids=gids)
    gd, vd, cd, od = renderer.sample_lattice(dense, origin, step, points[:, :3], ids=dids)
    assert gs.shape == (1500, 3) and vs.shape == (1500,) and cs.shape == (1500, 3) and cs.dtype == torch.int32 and os_.dtype == torch.int32
    listed = (os_ != abi.RM_FIELD_UNLISTED).cpu().numpy()
    assert listed.sum() > 300 and (~listed).any() and (od.cpu().numpy()[~listed] >= 0).all()
    for a, b, what in ((gs, gd, "gradient"), (vs, vd, "value"), (cs, cd, "cell"), (os_, od, "object")):
        h.assert_bit_equal(a.cpu().numpy()[listed], b.cpu().numpy()[listed], f"sample_lattice_blocks against sample_lattice: {what}")
    rows = torch.cat([gd, vd[:, None], cd.view(torch.float32), od.view(torch.float32)[:, None]], dim=1).cpu().numpy()
    Q.assert_records_equal(rows.view(F.SAMPLE), F.sample(dense.cpu().numpy(), o32, s32, points, dids.cpu().numpy()), "sample_lattice against the spec")
    out = torch.empty((1500, 8), dtype=torch.float32, device=renderer.device)
    nrm, tt, pos, oid = renderer.trace_lattice_blocks(grid, bl, blocks, origin, step, rays, iso=0.001, max_steps=64, ids=gids, out=out)
    assert nrm.data_ptr() == out.data_ptr() and oid.dtype == torch.int32 and tt.shape == (1500,)
    want = F.trace(dense.cpu().numpy(), o32, s32, rays, 0.001, 64, dids.cpu().numpy(), bl.cpu().numpy())
    Q.assert_records_equal(out.cpu().numpy().view(F.HIT), want, "trace_lattice_blocks against the spec")
    assert (want["objectId"] >= 0).sum() > 100
    dn, dt, dp, do = renderer.trace_lattice(dense, origin, step, rays, max_steps=64, normals=False)
    want = F.trace(dense.cpu().numpy(), o32, s32, rays, 0.001, 64, None, normals=False)
    h.assert_bit_equal(dt.cpu().numpy(), want["t"], "trace_lattice: t")
    assert (do.cpu().numpy() == want["objectId"]).all() and not dn.any() and not dp.any()
    # no points, no rays
    assert renderer.sample_lattice(dense, origin, step, np.zeros((0, 3), f32))[1].shape == (0,)
    assert renderer.trace_lattice_blocks(grid, bl, blocks, origin, step, np.zeros((0, 8), f32))[1].shape == (0,)
