"""rm_field_trace's definition without a GPU.  The library's own march (raymarcher_amd/csrc/rm_field_skip.h, the code the kernels call),
run serially by a stand-alone CPU program under the address and undefined-behaviour sanitizers — built twice, with and without the
coarse level —, against the NumPy specification (tests/field_handle_spec.py) in every bit; the specification against
rm_sdf_trace_blocks' (tests/field_spec.py) wherever the budget decides nothing; the coarse level against the fine march on the skip
campaign; and the properties of the occlusion mode."""
import numpy as np
import pytest

import field_handle_helpers as H
import field_handle_spec as S
import field_helpers as Q
import field_spec as F
import sdf_blocks_helpers as K
import sdf_blocks_spec as B

f32 = np.float32
EQUIVALENCE_BUDGET = 256  # check 2: the samples the handle's march gets; field_spec.trace shows there how few rays need more and end
EQUIVALENCE_RAYS = 600


@pytest.fixture(scope="module")
def cpu_programs(tmp_path_factory):
    """(the march that reads the coarse level, the march that does not)"""
    d = tmp_path_factory.mktemp("field_handle_cpu")
    return H.build_cpu_program(d, 1), H.build_cpu_program(d, 0)


def _packed(dense, ids, bl):
    return B.pack_blocks(dense, bl, f32(np.nan)), (B.pack_blocks(ids, bl, np.int32(-9)) if ids is not None else None)


# ---------------------------------------------------------------- 1. the shared header on the CPU equals the specification
@pytest.mark.parametrize("name", Q.BLOCK_CASES)
def test_the_shared_header_on_the_cpu_equals_the_spec_blocks(cpu_programs, tmp_path, name):
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    rays = Q.rays_for(dense, origin, step, iso, 1500)
    for label, bl in Q.block_lists(dense, iso).items():
        packed, packed_ids = _packed(dense, ids, bl)
        for steps in (64, 3):
            for mode in (S.CLOSEST, S.OCCLUSION):
                want = S.trace(dense, origin, step, rays, iso, steps, ids, bl, mode)
                for exe in cpu_programs:
                    got = H.run_cpu_program(exe, tmp_path, packed, packed_ids, origin, step, iso, rays, steps, mode, bl, blocks)
                    Q.assert_records_equal(got, want, f"{name}, {label} list, {steps} samples, mode {mode}")


# ---------------------------------------------------------------- 2. the handle's march is rm_sdf_trace_blocks' where no budget bites
@pytest.mark.parametrize("name", Q.BLOCK_CASES)
def test_where_the_budget_decides_nothing_the_march_is_rm_sdf_trace_blocks(cpu_programs, tmp_path, name):
    """The reference is field_spec.trace with all the iterations rm_sdf_trace_blocks can have, 65536, whose statistics say how many
    samples (iterations − skips) each ray took.  A ray is LEFT OUT iff the reference ended it — a hit, the box, the lattice or tMax
    left — after more samples than the handle's march is given here: only then can the two differ.  That is a subset of the rays
    "whose samples exceed the budget", and it is under 5 % of each case and list, asserted from the reference's statistics alone.
    The other rays whose samples exceed the budget are those the reference itself gives up on after 65536 iterations: rays that
    converge on a surface at iso = 0 and never get below it, and rays whose t became a NaN (7 %, 28 % and 57 % of the rays of the
    sphere, the sponge and the non-finite lattice, at any budget).  They are KEPT in the comparison: running out is the same miss
    record in both marches, so they must be equal too, and are.  The price is 65536 passes of the NumPy loop where such rays
    exist, which is why this test has fewer rays than its neighbours and is the slowest of the file."""
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    rays = Q.rays_for(dense, origin, step, iso, EQUIVALENCE_RAYS)
    for label, bl in Q.block_lists(dense, iso).items():
        ref = {}
        old = F.trace(dense, origin, step, rays, iso, 65536, ids, bl, stats=ref)
        needed = ref["iterations"] - ref["skips"]
        gave_up = ref["iterations"] >= 65536
        left_out = (needed > EQUIVALENCE_BUDGET) & ~gave_up
        print(f"{name}, {label} list: {left_out.mean():.2%} of the rays left out, {gave_up.mean():.1%} never end")
        assert left_out.mean() < 0.05, f"{name}, {label} list: {left_out.mean():.1%} of the rays need more than {EQUIVALENCE_BUDGET} samples"
        judged = ~left_out
        want = S.trace(dense, origin, step, rays, iso, EQUIVALENCE_BUDGET, ids, bl, S.CLOSEST)
        Q.assert_records_equal(want[judged], old[judged], f"{name}, {label} list: the specification against rm_sdf_trace_blocks'")
        packed, packed_ids = _packed(dense, ids, bl)
        got = H.run_cpu_program(cpu_programs[0], tmp_path, packed, packed_ids, origin, step, iso, rays, EQUIVALENCE_BUDGET, S.CLOSEST, bl, blocks)
        Q.assert_records_equal(got[judged], old[judged], f"{name}, {label} list: the library's march against rm_sdf_trace_blocks'")


# ---------------------------------------------------------------- 3. the skip campaign: coarse equals fine, on every ray
@pytest.mark.parametrize("label", H.CAMPAIGN_LISTS)
@pytest.mark.parametrize("blocks", H.CAMPAIGN_BLOCKS, ids=lambda b: "x".join(map(str, b)))
def test_on_the_skip_campaign_the_coarse_level_changes_no_bit(cpu_programs, tmp_path, blocks, label):
    """Two fields per lattice and list: the sphere at iso 0.001, where t only grows, and negative values over a negative iso, where
    every sample moves t down, through 0 and below — there t = max(ta, t) takes a ta, zeros of either sign among them, and the sign
    of a zero t decides the sign of the occlusion mode's infinite q."""
    bl, rays = H.campaign_list(blocks, label), H.campaign_rays(blocks)
    assert len(rays) * len(H.CAMPAIGN_BLOCKS) * len(H.CAMPAIGN_LISTS) >= 200_000
    if (blocks, label) == ((9, 5, 6), "corner"):
        _the_campaign_reaches_what_it_is_built_for(blocks, rays)
    sub = slice(0, Q.NUM)
    for (dense, origin, step), iso, budgets in ((H.campaign_lattice(blocks), H.CAMPAIGN_ISO, ((S.CLOSEST, 256), (S.OCCLUSION, 256), (S.NO_NORMAL, 2))),
                                                (H.negative_lattice(blocks), H.NEGATIVE_ISO, ((S.CLOSEST, 24), (S.OCCLUSION, 24), (S.OCCLUSION, 2)))):
        packed, _ = _packed(dense, None, bl)
        for mode, steps in budgets:
            coarse, fine = (H.run_cpu_program(exe, tmp_path, packed, None, origin, step, iso, rays, steps, mode, bl, blocks) for exe in cpu_programs)
            Q.assert_records_equal(coarse, fine, f"{blocks}, {label} list, iso {iso}, mode {mode}: coarse against fine")  # no ray is left out
            stats = {}
            want = S.trace(dense, origin, step, rays[sub], iso, steps, None, bl, mode, stats)
            Q.assert_records_equal(coarse[sub], want, f"{blocks}, {label} list, iso {iso}, mode {mode}: against the specification")
            if iso < 0 and mode == S.OCCLUSION and steps == 24 and label in ("checker", "groups", "full"):
                assert (want["objectId"] == F.MISS).sum() > 1000 and (want["t"][want["objectId"] == F.MISS] < 0).sum() > 300, "t went below 0"
                assert np.isinf(want["t"]).sum() > 20, "a sample at t = ±0"


def _the_campaign_reaches_what_it_is_built_for(blocks, rays):
    """Long runs of skips, ties on all three axes, every octant, tiny and huge directions, origins on edges and corners."""
    dense, origin, step = H.campaign_lattice(blocks)
    d = rays[:, 4:7]
    octant = (d[:, 0] > 0) * 1 + (d[:, 1] > 0) * 2 + (d[:, 2] > 0) * 4
    full = (d != 0).all(axis=1)
    assert all((octant[full] == k).sum() > 500 for k in range(8))
    length = np.linalg.norm(d.astype(np.float64), axis=1)
    assert (length < 1e-29).sum() > 500 and (length > 1e29).sum() > 500
    assert ((d != 0).sum(axis=1) == 1).sum() > 2000, "axis-parallel rays"
    diag = (np.abs(d[:, 0]) == np.abs(d[:, 1])) & (np.abs(d[:, 1]) == np.abs(d[:, 2])) & full
    assert diag.sum() > 2000
    u = (rays[:, 0:3].astype(np.float64) - origin) / step
    on_face = (u == np.round(u)) & (np.round(u) % 8 == 0)
    assert (on_face.sum(axis=1) >= 2).sum() > 1000, "origins on block edges and corners"
    stats = {}
    S.trace(dense, origin, step, rays[:Q.NUM], H.CAMPAIGN_ISO, 256, None, H.campaign_list(blocks, "corner"), S.CLOSEST, stats)
    assert stats["skips"].max() >= 9 and (stats["skips"] >= 4).sum() > 500, "runs of skips longer than a group"
    assert stats["skips"].max() <= sum(blocks) * (stats["samples"].max() + 1)


def test_a_run_of_skips_keeps_the_first_of_several_zero_ta(cpu_programs, tmp_path):
    """8×8×1 blocks of −6 everywhere, iso −10, one listed block; the ray enters the box at t = 5 exactly on the edge x = 8, y = 32 of
    an empty group, samples nothing there — the block is unlisted — but after its first listed sample t has fallen below 0, and the
    next run of skips crosses an inner face at ta = +0 before it leaves the group at ta = −0 (or the other way round): t = ta > t ?
    ta : t keeps the first.  The occlusion factor then divides by that zero."""
    blocks = (8, 8, 1)
    dense = np.full((9, 65, 65), -6.0, f32)
    origin, step = np.zeros(3, f32), np.ones(3, f32)
    bl = np.array([[1, 3, 0, 0]], np.int32)
    rays = np.zeros((8, 8), f32)
    rays[:, 3] = 100.0
    for i, (o, d) in enumerate((((8, 32, -5), (0.1, -0.1, 1)), ((8, 32, -5), (-0.1, 0.1, 1)), ((16, 32, -5), (0.1, -0.1, 1)), ((16, 24, -5), (-0.1, -0.1, 1)),
                                ((8, 32, 13), (0.1, -0.1, -1)), ((32, 32, -5), (0.1, -0.1, 1)), ((8, 32, -5), (0.1, -0.1, 2)), ((8, 24, -5), (0.1, 0.1, 1)))):
        rays[i, 0:3], rays[i, 4:7] = o, d
    packed, _ = _packed(dense, None, bl)
    seen = []
    for mode in (S.OCCLUSION, S.CLOSEST):
        for steps in (1, 2, 3, 8):
            want = S.trace(dense, origin, step, rays, -10.0, steps, None, bl, mode)
            for exe in cpu_programs:
                got = H.run_cpu_program(exe, tmp_path, packed, None, origin, step, -10.0, rays, steps, mode, bl, blocks)
                Q.assert_records_equal(got, want, f"mode {mode}, {steps} samples")
            seen.append(want["t"][0])
    assert np.isneginf(seen[1]) and np.isneginf(seen[2]), "the first ray's factor is −inf after its second sample"


# ---------------------------------------------------------------- 4. a dense handle's march is rm_sdf_trace
@pytest.mark.parametrize("name", Q.DENSE_CASES[::2] + list(Q.HANDMADE_DENSE))
def test_the_dense_march_is_rm_sdf_trace(cpu_programs, tmp_path, name):
    dist, ids, origin, step, iso = Q.dense_case(name)
    rays = Q.rays_for(dist, origin, step, iso, 1500)
    for use, steps, mode in ((ids, 64, S.CLOSEST), (None, 3, S.NO_NORMAL), (ids, 0, S.CLOSEST)):
        old = F.trace(dist, origin, step, rays, iso, steps, use, normals=mode == S.CLOSEST)
        Q.assert_records_equal(S.trace(dist, origin, step, rays, iso, steps, use, None, mode), old, f"{name}: the specification, {steps} steps")
        got = H.run_cpu_program(cpu_programs[0], tmp_path, dist, use, origin, step, iso, rays, steps, mode)
        Q.assert_records_equal(got, old, f"{name}: the library's march, {steps} steps")
    want = S.trace(dist, origin, step, rays, iso, 64, ids, None, S.OCCLUSION)
    got = H.run_cpu_program(cpu_programs[0], tmp_path, dist, ids, origin, step, iso, rays, 64, S.OCCLUSION)
    Q.assert_records_equal(got, want, f"{name}: occlusion")


# ---------------------------------------------------------------- 5. the occlusion mode
@pytest.mark.parametrize("name", ("sphere_25", "bulb_33", "nonfinite_17x9x9"))
def test_occlusion_hits_iff_closest_hits_and_the_factor_is_at_most_one(cpu_programs, tmp_path, name):
    """On the records of the library's march (the CPU program), and on the specification's: occlusion hits iff closest hits, with the
    same ids; normal and position are zero words; the factor is never a NaN and at most 1; 1 for a ray that never sampled."""
    dense, ids, origin, step, iso = K.case(name)
    blocks = B.blocks_of(dense)
    rays = Q.rays_for(dense, origin, step, iso, 3000)
    for label, bl in list(Q.block_lists(dense, iso).items()) + [("dense", None)]:
        stats = {}
        spec = S.trace(dense, origin, step, rays, iso, 64, ids, bl, S.OCCLUSION, stats), S.trace(dense, origin, step, rays, iso, 64, ids, bl, S.NO_NORMAL)
        if bl is None:
            lib = tuple(H.run_cpu_program(cpu_programs[0], tmp_path, dense, ids, origin, step, iso, rays, 64, m) for m in (S.OCCLUSION, S.NO_NORMAL))
        else:
            packed, packed_ids = _packed(dense, ids, bl)
            lib = tuple(H.run_cpu_program(cpu_programs[0], tmp_path, packed, packed_ids, origin, step, iso, rays, 64, m, bl, blocks)
                        for m in (S.OCCLUSION, S.NO_NORMAL))
        for who, (occ, near) in (("the library", lib), ("the specification", spec)):
            assert (occ["objectId"] == near["objectId"]).all(), f"{name}, {label}, {who}: the same hits, misses, invalid rays and ids"
            words = occ.view(np.uint32).reshape(-1, 8)
            assert (words[:, [0, 1, 2, 4, 5, 6]] == 0).all(), f"{who}: normal and position are zeros"
            valid = occ["objectId"] != F.INVALID
            assert not np.isnan(occ["t"]).any() and (occ["t"][valid] <= 1).all() and (occ["t"][~valid] == 0).all(), who
            never = valid & (stats["samples"] == 0)
            assert (occ["t"][never] == 1).all(), f"{who}: a ray that never sampled stores 1"
            moved = valid & (stats["samples"] >= 2) & (occ["objectId"] == F.MISS)
            if label in ("full", "dense") and name != "nonfinite_17x9x9":
                assert moved.sum() > 100 and (occ["t"][moved] < 1).any(), who
            if label == "empty":
                assert (occ["t"][occ["objectId"] == F.MISS] == 1).all() and np.isin(occ["objectId"], (F.MISS, F.INVALID)).all(), who
