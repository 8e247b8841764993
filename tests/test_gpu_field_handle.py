"""RmField handles on the GPU: rm_field_sample and the three modes of rm_field_trace against the NumPy specifications
(tests/field_spec.py, tests/field_handle_spec.py) in every bit, every output between guard words, on dense and block handles; the
handle against the entry points it stands in for, on the device; the skip campaign; what a handle owns and borrows; the query
refusals, which need a live handle; and the Python layer."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import field_handle_helpers as H
import field_handle_spec as S
import field_helpers as Q
import field_spec as F
import helpers as h
import sdf_blocks_helpers as K
import sdf_blocks_spec as B
import sdf_helpers as V
from raymarcher_amd import abi, lib
from test_gpu_field import Lattice, ptr, up, vec

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID = abi.RM_ERR_INVALID_ARGUMENT
MODE = {S.CLOSEST: abi.RM_TRACE_CLOSEST, S.NO_NORMAL: abi.RM_TRACE_NO_NORMAL, S.OCCLUSION: abi.RM_TRACE_OCCLUSION}


class Field(Lattice):
    """test_gpu_field's lattice on the device with an RmField handle on it; sample and trace go through the handle (old_sample and
    old_trace: through rm_sdf_sample … rm_sdf_trace_blocks)."""

    def __init__(self, renderer, dense, ids, origin, step, block_list=None, with_ids=True):
        super().__init__(renderer, dense, ids, origin, step, block_list)
        self.handle = C.c_void_p()
        use = ptr(self.ids) if with_ids else None
        if self.sparse:
            st = lib().rm_field_create_blocks(ptr(self.dist), use, ptr(self.bl), len(self.bl), *self.dims, vec(origin), vec(step),
                                              renderer._stream(), C.byref(self.handle))
        else:
            st = lib().rm_field_create(ptr(self.dist), use, *self.dims, vec(origin), vec(step), C.byref(self.handle))
        assert st == abi.RM_OK and self.handle.value, lib().rm_last_error().decode()

    old_sample, old_trace = Lattice.sample, Lattice.trace

    def close(self):
        torch.cuda.synchronize()
        lib().rm_field_destroy(self.handle)
        self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _query(self, fn, src, args, dtype):
        g = h.Guarded((len(src), 8), torch.float32, h.FLOAT_POISON, self.r.device)
        path = lib().rm_debug_last_path()
        st = fn(self.handle, ptr(src), len(src), *args, ptr(g.payload), self.r._stream())
        assert st == abi.RM_OK, lib().rm_last_error().decode()
        g.check()
        assert lib().rm_debug_last_path() == path, "not a render launch"
        return g.payload.cpu().numpy().view(dtype).reshape(-1)

    def sample(self, points):
        return self._query(lib().rm_field_sample, points if torch.is_tensor(points) else up(self.r, points, f32), (), F.SAMPLE)

    def trace(self, rays, iso, steps, mode=S.CLOSEST):
        return self._query(lib().rm_field_trace, rays if torch.is_tensor(rays) else up(self.r, rays, f32), (float(iso), steps, MODE[mode]), F.HIT)


# ---------------------------------------------------------------- against the specification and the existing entry points
@pytest.mark.parametrize("name", Q.DENSE_CASES + list(Q.HANDMADE_DENSE))
def test_a_dense_handle_equals_the_spec_and_rm_sdf_sample_and_rm_sdf_trace(renderer, name):
    dist, ids, origin, step, iso = Q.dense_case(name)
    points, rays = Q.points_for(dist, origin, step), Q.rays_for(dist, origin, step, iso)
    with Field(renderer, dist, ids, origin, step) as f:
        got = f.sample(points)
        Q.assert_records_equal(got, F.sample(dist, origin, step, points, ids), f"{name}: samples")
        Q.assert_records_equal(got, f.old_sample(points), f"{name}: samples against rm_sdf_sample")
        for mode, steps in ((S.CLOSEST, 64), (S.NO_NORMAL, 3), (S.OCCLUSION, 64), (S.OCCLUSION, 3)):
            got = f.trace(rays, iso, steps, mode)
            Q.assert_records_equal(got, S.trace(dist, origin, step, rays, iso, steps, ids, None, mode), f"{name}: mode {mode}, {steps} samples")
            if mode != S.OCCLUSION:
                Q.assert_records_equal(got, f.old_trace(rays, iso, steps, normals=mode == S.CLOSEST), f"{name}: against rm_sdf_trace, {steps}")
        Q.assert_records_equal(f.trace(rays, iso, 0), f.old_trace(rays, iso, 0), f"{name}: no sample")
    if ids is not None:
        with Field(renderer, dist, ids, origin, step, with_ids=False) as f:
            Q.assert_records_equal(f.sample(points), F.sample(dist, origin, step, points, None), f"{name}: samples without ids")
            Q.assert_records_equal(f.trace(rays, iso, 64, S.OCCLUSION), S.trace(dist, origin, step, rays, iso, 64, None, None, S.OCCLUSION),
                                   f"{name}: occlusion without ids")


@pytest.mark.parametrize("name", Q.BLOCK_CASES)
def test_a_block_handle_equals_the_spec_and_the_block_entries(renderer, name):
    dense, ids, origin, step, iso = K.case(name)
    points, rays = Q.points_for(dense, origin, step), Q.rays_for(dense, origin, step, iso)
    with Field(renderer, dense, ids, origin, step) as whole:
        dense_hits = whole.trace(rays, iso, 64)
        dense_samples = whole.sample(points)
    for label, bl in Q.block_lists(dense, iso).items():
        with Field(renderer, dense, ids, origin, step, bl) as f:
            got = f.sample(points)
            Q.assert_records_equal(got, F.sample(dense, origin, step, points, ids, bl), f"{name}, {label} list: samples")
            Q.assert_records_equal(got, f.old_sample(points), f"{name}, {label} list: samples against rm_sdf_sample_blocks")
            for mode, steps in ((S.CLOSEST, 64), (S.OCCLUSION, 64), (S.NO_NORMAL, 3), (S.OCCLUSION, 3), (S.CLOSEST, 0)):
                want = S.trace(dense, origin, step, rays, iso, steps, ids, bl, mode)
                got = f.trace(rays, iso, steps, mode)
                Q.assert_records_equal(got, want, f"{name}, {label} list: mode {mode}, {steps} samples")
                if (mode, steps) == (S.CLOSEST, 64):
                    closest = got
            # rm_sdf_trace_blocks with all the iterations it can have against the handle at 256 samples.  Left out: the rays that
            # use 256 samples up WITHOUT having reached a state that repeats (the spec's never_ends: such a ray runs out in both
            # marches, the same miss, and is compared) — the only rays a larger budget could end otherwise; under 5 % of a case.
            stats = {}
            want = S.trace(dense, origin, step, rays, iso, 256, ids, bl, S.CLOSEST, stats)
            left_out = stats["exhausted"] & ~stats["never_ends"]
            assert left_out.mean() < 0.05, f"{name}, {label} list: {left_out.mean():.1%} of the rays left out"
            at256 = f.trace(rays, iso, 256)
            Q.assert_records_equal(at256, want, f"{name}, {label} list: 256 samples")
            Q.assert_records_equal(at256[~left_out], f.old_trace(rays, iso, 65536)[~left_out], f"{name}, {label} list: against rm_sdf_trace_blocks")
            if label in ("full", "messy"):
                Q.assert_records_equal(closest, dense_hits, f"{name}, {label} list: every block listed is the dense handle")
                Q.assert_records_equal(f.sample(points), dense_samples, f"{name}, {label} list: samples, every block listed")
            if label == "empty":
                occ = f.trace(rays, iso, 64, S.OCCLUSION)
                assert np.isin(occ["objectId"], (F.MISS, F.INVALID)).all() and (occ["t"][occ["objectId"] == F.MISS] == 1).all()


def _campaign_field(blocks, field):
    return (H.campaign_lattice(blocks), H.CAMPAIGN_ISO, 256) if field == "sphere" else (H.negative_lattice(blocks), H.NEGATIVE_ISO, 24)


@functools.lru_cache(maxsize=None)
def _campaign_want(blocks, label, field, mode):
    (dense, origin, step), iso, steps = _campaign_field(blocks, field)
    want = S.trace(dense, origin, step, H.campaign_rays(blocks)[:Q.NUM], iso, steps, None, H.campaign_list(blocks, label), mode)
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("label", H.CAMPAIGN_LISTS)
@pytest.mark.parametrize("blocks", H.CAMPAIGN_BLOCKS, ids=lambda b: "x".join(map(str, b)))
def test_the_skip_campaign(renderer, blocks, label):
    """4 099 rays of the campaign (field_handle_helpers.campaign_rays: ties, faces, edges, ragged groups, tiny and huge directions)
    through lattices of 9×5×6 and 16×16×16 blocks with each list, on the sphere's field and on the negative one, where t falls
    below 0."""
    rays = H.campaign_rays(blocks)[:Q.NUM]
    for field in ("sphere", "negative"):
        (dense, origin, step), iso, steps = _campaign_field(blocks, field)
        with Field(renderer, dense, None, origin, step, H.campaign_list(blocks, label)) as f:
            for mode in (S.CLOSEST, S.OCCLUSION):
                Q.assert_records_equal(f.trace(rays, iso, steps, mode), _campaign_want(blocks, label, field, mode),
                                       f"{blocks}, {label} list, {field} field, mode {mode}")


# ---------------------------------------------------------------- what a handle owns, borrows and survives
def test_one_point_one_ray_two_handles_a_second_stream_and_a_freed_list(renderer):
    dense, ids, origin, step, iso = K.case("bulb_33")
    points, rays = Q.points_for(dense, origin, step), Q.rays_for(dense, origin, step, iso)
    bl = B.active_blocks(dense, iso)
    a = Field(renderer, dense, ids, origin, step, bl)
    a.bl = None  # the handle consumed the list: free it, and churn the allocator over where it was
    gc.collect()
    torch.cuda.empty_cache()
    junk = torch.full((1 << 16,), -1, dtype=torch.int32, device=renderer.device)
    b = Field(renderer, dense, ids, origin, step)  # a second handle, alive beside the first
    want_a = S.trace(dense, origin, step, rays, iso, 64, ids, bl)
    want_b = S.trace(dense, origin, step, rays, iso, 64, ids, None)
    Q.assert_records_equal(a.trace(rays, iso, 64), want_a, "the block handle after its list is gone")
    Q.assert_records_equal(b.trace(rays, iso, 64), want_b, "the dense handle beside it")
    Q.assert_records_equal(a.sample(points), F.sample(dense, origin, step, points, ids, bl), "the block handle's samples")
    hit = int(np.nonzero(want_a["objectId"] >= 0)[0][0])
    Q.assert_records_equal(a.trace(rays[hit:hit + 1], iso, 64), want_a[hit:hit + 1], "one ray")
    Q.assert_records_equal(a.trace(rays[hit:hit + 1], iso, 64, S.OCCLUSION), S.trace(dense, origin, step, rays[hit:hit + 1], iso, 64, ids, bl, S.OCCLUSION),
                           "one ray, occlusion")
    inside = int(np.nonzero(F.sample(dense, origin, step, points, ids, bl)["objectId"] >= 0)[0][0])
    Q.assert_records_equal(a.sample(points[inside:inside + 1]), F.sample(dense, origin, step, points[inside:inside + 1], ids, bl), "one point")
    # a stream the handle was not built on
    side = torch.cuda.Stream(device=renderer.device)
    side.wait_stream(torch.cuda.current_stream(renderer.device))
    with torch.cuda.stream(side):
        on_side = a.trace(rays, iso, 64), b.sample(points)
    side.synchronize()
    Q.assert_records_equal(on_side[0], want_a, "a second stream, block handle")
    Q.assert_records_equal(on_side[1], F.sample(dense, origin, step, points, ids), "a second stream, dense handle")
    a.close(), b.close()
    a.close()  # a closed handle is NULL here: destroying it again is the no-op
    del junk


def test_values_rewritten_in_place_are_seen_by_the_next_call(renderer):
    dense, ids, origin, step, iso = K.case("sphere_25")
    rays, points = Q.rays_for(dense, origin, step, iso), Q.points_for(dense, origin, step)
    bl = B.all_blocks(B.blocks_of(dense))
    moved = (dense + f32(0.05)).astype(f32)  # the sphere shrinks
    for block_list in (None, bl):
        with Field(renderer, dense, ids, origin, step, block_list) as f:
            before = f.trace(rays, iso, 64, S.OCCLUSION)
            Q.assert_records_equal(before, S.trace(dense, origin, step, rays, iso, 64, ids, block_list, S.OCCLUSION), "before")
            f.dist.copy_(up(renderer, moved if block_list is None else B.pack_blocks(moved, bl, f32(np.nan)), f32))  # in place: the same memory
            after = f.trace(rays, iso, 64, S.OCCLUSION)
            Q.assert_records_equal(after, S.trace(moved, origin, step, rays, iso, 64, ids, block_list, S.OCCLUSION), "after")
            assert (F.as_words(before) != F.as_words(after)).any(axis=1).sum() > 100
            Q.assert_records_equal(f.sample(points), F.sample(moved, origin, step, points, ids, block_list), "samples after")


def test_query_refusals_in_order(renderer):
    dense, ids, origin, step, iso = K.case("iso_ties_9")
    nan, inf = float("nan"), float("inf")
    host = np.zeros(4096, f32)
    hp = C.c_void_p(host.ctypes.data)
    assert host.ctypes.data % 16 == 0
    buf = torch.zeros((64, 8), dtype=torch.float32, device=renderer.device)
    dev = C.c_void_p(buf.data_ptr())
    fake = C.c_void_p(0x1000)

    def refused(status, text):
        return status == INVALID and text in lib().rm_last_error().decode()

    for block_list in (None, B.all_blocks(B.blocks_of(dense))):
        with Field(renderer, dense, ids, origin, step, block_list) as f:
            sample = lambda n=5, p=fake, o=fake: lib().rm_field_sample(f.handle, p, n, o, None)  # noqa: E731
            trace = lambda n=5, r=fake, iso=0.0, steps=64, mode=0, o=fake: lib().rm_field_trace(f.handle, r, n, iso, steps, mode, o, None)  # noqa: E731
            for n in (-1, -2 ** 31):
                assert refused(sample(n=n), "negative numPoints") and refused(trace(n=n, iso=nan), "negative numRays")
            for v in (nan, inf, -inf):
                assert refused(trace(iso=v, steps=-1), "iso must be finite")
            for steps in (-1, 65537, 2 ** 31 - 1):
                assert refused(trace(steps=steps, mode=4), "maxSteps must be 0 … RM_MAX_FIELD_STEPS")
            for mode in (4, 8, 0x80000000, 5):
                assert refused(trace(mode=mode, n=0), "mode bits other than")
            assert refused(trace(mode=3), "RM_TRACE_NO_NORMAL is a flag on RM_TRACE_CLOSEST") and refused(trace(mode=3, n=0, r=None), "flag on")
            assert sample(n=0) == abi.RM_OK and sample(n=0, p=None, o=None) == abi.RM_OK
            for mode in (0, 1, 2):
                assert trace(n=0, mode=mode) == abi.RM_OK and trace(n=0, mode=mode, r=None, o=None, steps=65536) == abi.RM_OK
            assert refused(sample(p=None), "null d_points or d_samples") and refused(sample(o=None), "null d_points or d_samples")
            assert refused(trace(r=None), "null d_rays or d_hits") and refused(trace(o=None, mode=2), "null d_rays or d_hits")
            assert refused(sample(p=None, o=C.c_void_p(0x1008)), "null")  # null comes before misaligned
            for k in ("p", "o"):
                assert refused(sample(**{k: C.c_void_p(0x1008)}), "misaligned")
            for k in ("r", "o"):
                assert refused(trace(**{k: C.c_void_p(0x1008)}), "misaligned")
            assert refused(sample(p=hp, o=dev), "d_points is not device-accessible") and refused(sample(p=dev, o=hp), "d_samples is not device-accessible")
            assert refused(trace(r=hp, o=dev), "d_rays is not device-accessible") and refused(trace(r=dev, o=hp), "d_hits is not device-accessible")
            assert refused(trace(r=hp, o=C.c_void_p(host.ctypes.data + 8)), "misaligned")  # misaligned comes before the device-memory check
            if torch.cuda.device_count() > 1:
                try:
                    assert lib().rm_set_device(1) == abi.RM_OK
                    assert refused(sample(p=dev, o=dev), "another device") and refused(trace(r=dev, o=dev), "another device")
                finally:
                    assert lib().rm_set_device(0) == abi.RM_OK
                    torch.cuda.set_device(renderer.device)
            assert sample(p=dev, o=dev) == abi.RM_OK and trace(r=dev, o=dev, mode=2) == abi.RM_OK  # the handle still works
        assert refused(lib().rm_field_sample(None, dev, 5, dev, None), "null or stale RmField handle")


# ---------------------------------------------------------------- the Python layer
def test_the_python_layer_and_scene_field(renderer):
    from raymarcher_amd import LatticeField
    objs, no, g, s = V.scene("bulb_plain")
    t = h.tables_of((abi.RmCamera(), objs, no, None, 0, g))
    lo, hi = V.BOXES["bulb_plain"]
    grid, gids, bl, blocks, origin, step = renderer.scene_field_sparse(t, s, 36, iso=0.001, bounds=(lo, hi))
    dims = tuple(8 * m + 1 for m in blocks)
    dense, dids = renderer.sdf_grid(t, s, origin, step, dims, ids=True)
    o32, s32 = np.asarray(origin, f32), np.asarray(step, f32)
    dn, di, bn = dense.cpu().numpy(), dids.cpu().numpy(), bl.cpu().numpy()
    points, rays = Q.points_for(dn, o32, s32, 1500), Q.rays_for(dn, o32, s32, 0.001, 1500)

    def rows(parts, dtype):
        return torch.cat([p.view(torch.float32).reshape(len(p), -1) for p in parts], dim=1).cpu().numpy().view(dtype).reshape(-1)

    with renderer.scene_field(t, s, 36, iso=0.001, bounds=(lo, hi)) as field:
        assert isinstance(field, LatticeField)
        Q.assert_records_equal(rows(field.sample(points), F.SAMPLE), F.sample(dn, o32, s32, points, di, bn), "scene_field: samples")
        Q.assert_records_equal(rows(field.trace(rays, max_steps=64), F.HIT), S.trace(dn, o32, s32, rays, 0.001, 64, di, bn), "scene_field: closest")
        out = torch.empty((1500, 8), dtype=torch.float32, device=renderer.device)
        nrm, tt, pos, oid = field.trace(rays, max_steps=64, mode="occlusion", out=out)
        assert nrm.data_ptr() == out.data_ptr() and oid.dtype == torch.int32 and tt.shape == (1500,)
        want = S.trace(dn, o32, s32, rays, 0.001, 64, di, bn, S.OCCLUSION)
        Q.assert_records_equal(out.cpu().numpy().view(F.HIT).reshape(-1), want, "scene_field: occlusion")
        assert (want["objectId"] >= 0).sum() > 100 and ((want["objectId"] == F.MISS) & (want["t"] < 1)).sum() > 20
        with pytest.raises(ValueError):
            field.trace(rays, mode="shadow")
    with renderer.lattice_field_blocks(grid, bl, blocks, origin, step, ids=gids) as sparse, renderer.lattice_field(dense, origin, step, ids=dids) as whole:
        Q.assert_records_equal(rows(sparse.trace(rays, max_steps=64, normals=False), F.HIT), S.trace(dn, o32, s32, rays, 0.001, 64, di, bn, S.NO_NORMAL),
                               "lattice_field_blocks: without normals")
        Q.assert_records_equal(rows(whole.trace(rays, max_steps=64), F.HIT), F.trace(dn, o32, s32, rays, 0.001, 64, di), "lattice_field: closest")
        Q.assert_records_equal(rows(whole.sample(points[:, :3]), F.SAMPLE), F.sample(dn, o32, s32, points, di), "lattice_field: samples")
        assert whole.sample(np.zeros((0, 3), f32))[1].shape == (0,) and sparse.trace(np.zeros((0, 8), f32))[1].shape == (0,)
    sparse.close()
    sparse.close()  # idempotent
    with pytest.raises(ValueError):
        sparse.sample(points)
    empty = renderer.lattice_field_blocks(grid[:0], bl[:0], blocks, origin, step)
    assert (empty.sample(points)[3].cpu().numpy() != abi.RM_FIELD_UNLISTED).sum() == (F.sample(dn, o32, s32, points)["objectId"] < -1).sum()
    del empty  # destroyed on garbage collection
    gc.collect()
