"""rm_sdf_blocks_select_pruned's rule without a GPU: what the eight-corner rule keeps and loses on the oracle's lattices of the seven
tables (the table the header's remarks about the two constants rest on), the rule on hand-made corner values a distance function
would not produce, and the library's own classification (raymarcher_amd/csrc/rm_blocks_prune.h) in a stand-alone CPU program under
the host sanitizers, which equals the NumPy specification in every word."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as h
import sdf_blocks_spec as B
import sdf_helpers as V
import sdf_prune_spec as P

f32 = np.float32
inf, nan = f32(np.inf), f32(np.nan)
SCENES = ("sphere", "primitives", "menger", "bulb_plain", "bulb_moved", "bulb_power6", "julia")
ISO = {"sphere": 0.0, "primitives": 0.0, "menger": 0.0, "bulb_plain": 0.001, "bulb_moved": 0.001, "bulb_power6": 0.001, "julia": 0.001}
BLOCKS = (16, 16, 16)
CPU_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sdf_prune_spec", "rm_blocks_prune_cpu.cpp")


def lattice(name):
    """(dense, step, iso) of a table's oracle lattice of 16³ blocks."""
    dist, _ids, _origin, step = V.oracle_lattice(name, tuple(8 * m + 1 for m in BLOCKS))
    return dist, step, ISO[name]


def lost(name, l_out, l_in):
    """The active blocks that the rule discards → int32 (n, 4), with the exhaustive list and the number of candidates."""
    dense, step, iso = lattice(name)
    every = B.active_blocks(dense, iso)
    kept, cand = P.pruned_blocks(dense, step, iso, l_out, l_in)
    as_set = lambda a: {tuple(r) for r in a.tolist()}  # noqa: E731
    assert as_set(kept) <= as_set(every) and len(kept) <= cand <= int(np.prod(BLOCKS))
    return np.array(sorted(as_set(every) - as_set(kept)), np.int32).reshape(-1, 4), every, cand


# ---------------------------------------------------------------- (a) the oracle's lattices
@pytest.mark.parametrize("name", SCENES)
def test_outside_bound_one_loses_no_active_block(name):
    gone, every, cand = lost(name, 1.0, inf)
    assert len(every) > 50, "the lattice does not cross the surface"
    assert len(gone) == 0, f"{name}: (1, inf) lost {gone[:5].tolist()}"
    # and it prunes: not the whole lattice is evaluated, never fewer blocks than are active
    assert len(every) <= cand < int(np.prod(BLOCKS)), (len(every), cand)


@pytest.mark.parametrize("name", SCENES)
def test_inside_bound_one_loses_only_the_julia_sets_interior_pockets(name):
    gone, _every, _cand = lost(name, 1.0, 1.0)
    if name != "julia":
        assert len(gone) == 0, f"{name}: (1, 1) lost {gone[:5].tolist()}"
        return
    assert len(gone) == 4, gone.tolist()
    dense, _step, iso = lattice(name)
    corners = np.stack([B.block_values(dense, bi, bj, bk)[::8, ::8, ::8].reshape(8) for bi, bj, bk, _ in gone])
    # every lost block sits in the set's interior, where the estimator reports one constant that is no distance: all eight corners
    # hold it, and the block is active only through a pocket of escaping points between them
    assert (h.bits(corners) == h.bits(corners)[0, 0]).all(), corners
    assert abs(float(corners[0, 0]) + 0.1827376) < 1e-6
    for bi, bj, bk, _ in gone:
        escaping = int((B.block_values(dense, bi, bj, bk) >= f32(iso)).sum())
        assert 1 <= escaping < 729 // 2, escaping


def test_an_eighth_of_the_bound_loses_blocks():
    """The rule has teeth: with lipschitzOut = 0.125 an active block of the primitives goes."""
    gone, _every, _cand = lost("primitives", 0.125, inf)
    assert len(gone) >= 1


def test_infinite_constants_keep_every_block_and_zero_keeps_the_sign_changes():
    dense, step, iso = lattice("primitives")
    assert P.candidates(dense, step, iso, inf, inf).all()
    kept, cand = P.pruned_blocks(dense, step, iso, inf, inf)
    assert (kept == B.active_blocks(dense, iso)).all() and cand == int(np.prod(BLOCKS))
    c = dense[::8, ::8, ::8]
    zero = P.candidates(dense, step, iso, 0.0, 0.0)
    out = c > f32(iso)
    same = np.ones(zero.shape, bool)
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                same &= out[cz:16 + cz, cy:16 + cy, cx:16 + cx] == out[:16, :16, :16]
    assert not (c == f32(iso)).any() and (zero == ~same).all()


# ---------------------------------------------------------------- (b) hand-made corners
STEP = np.array([0.25, 0.5, 0.125], f32)  # h = 4 · sqrt(0.328125)


def one_block(values):
    return np.array(values, f32).reshape(2, 2, 2)


def handmade():
    """name → (corners, step, iso, l_out, l_in, the candidate flags expected or None).  The expectations are worked out here, from
    the definition's words, not computed by the specification."""
    iso = f32(0.25)
    b1 = f32(f32(4) * np.sqrt(f32(0.328125)))  # the bound of a constant of 1
    far = f32(iso + f32(2) * b1)
    out = {}
    up, down = np.nextafter(b1, inf), np.nextafter(b1, -inf)
    # iso = 0 makes c − iso exact: a corner at the bound ties and is not far, one ulp beyond it is
    out["all_just_beyond_out"] = (one_block([up] * 8), STEP, 0.0, 1.0, inf, [0])
    out["one_tie_out"] = (one_block([up] * 7 + [b1]), STEP, 0.0, 1.0, inf, [1])
    out["all_ties_out"] = (one_block([b1] * 8), STEP, 0.0, 1.0, 1.0, [1])
    out["all_just_beyond_in"] = (one_block([-up] * 8), STEP, 0.0, inf, 1.0, [0])
    out["one_tie_in"] = (one_block([-up] * 3 + [-b1] + [-up] * 4), STEP, 0.0, 1.0, 1.0, [1])
    out["one_short_in"] = (one_block([-up] * 7 + [-down]), STEP, 0.0, 1.0, 1.0, [1])
    out["far_in_but_inside_is_inf"] = (one_block([-far] * 8), STEP, iso, 1.0, inf, [1])
    out["far_out_but_outside_is_inf"] = (one_block([far] * 8), STEP, iso, inf, 1.0, [1])
    out["far_on_both_sides_mixed"] = (one_block([far, -far] * 4), STEP, iso, 1.0, 1.0, [1])  # far everywhere, on no single side
    out["one_nan"] = (one_block([far] * 5 + [nan] + [far] * 2), STEP, iso, 1.0, 1.0, [1])
    out["all_nan"] = (one_block([nan] * 8), STEP, iso, 0.0, 0.0, [1])
    out["plus_inf"] = (one_block([inf] * 8), STEP, iso, 1.0, 1.0, [0])
    out["minus_inf"] = (one_block([-inf] * 8), STEP, iso, 1.0, 1.0, [0])
    out["minus_inf_one_plus_inf"] = (one_block([-inf] * 7 + [inf]), STEP, iso, 1.0, 1.0, [1])
    out["plus_inf_under_an_infinite_constant"] = (one_block([inf] * 8), STEP, iso, inf, inf, [1])  # inf > inf is false
    out["minus_inf_under_an_infinite_constant"] = (one_block([-inf] * 8), STEP, iso, inf, inf, [1])
    # a constant of 0: the bound is 0, any corner strictly beyond iso is far, one equal to iso is not
    out["zero_all_above"] = (one_block([np.nextafter(iso, inf)] * 8), STEP, iso, 0.0, 0.0, [0])
    out["zero_all_below"] = (one_block([np.nextafter(iso, -inf)] * 8), STEP, iso, 0.0, 0.0, [0])
    out["zero_one_at_iso"] = (one_block([f32(1)] * 7 + [iso]), STEP, iso, 0.0, 0.0, [1])
    out["zero_sign_change"] = (one_block([f32(1)] * 7 + [f32(-1)]), STEP, iso, 0.0, 0.0, [1])
    # a step whose square overflows: h = +inf, the bound of a positive constant +inf, of a zero constant NaN — nothing is discarded
    huge = np.array([1e20, 1.0, 1.0], f32)
    out["overflow_positive_constant"] = (one_block([inf] * 8), huge, iso, 0.5, 0.5, [1])
    out["overflow_zero_constant"] = (one_block([inf] * 8), huge, iso, 0.0, 0.0, [1])
    out["overflow_zero_constant_inside"] = (one_block([-inf] * 8), huge, iso, 0.0, 0.0, [1])
    # three blocks along x, the middle one's corners far out, its neighbours each hold a near corner: (mz, my, mx) = (1, 1, 3)
    row = np.full((2, 2, 4), far, f32)
    row[0, 0, 0], row[1, 1, 3] = iso, iso
    out["three_blocks_middle_discarded"] = (row, STEP, iso, 1.0, 1.0, [1, 0, 1])
    # 5×4×3 blocks of random values with every special value sprinkled in, against the CPU program and the block-by-block rule
    rng = np.random.default_rng(47)
    big = rng.choice(np.array([-3 * b1, -up, -b1, -down, -0.0, 0.0, down, b1, up, 3 * b1], f32), (4, 5, 6))
    pick = rng.uniform(size=big.shape)
    big[pick < 0.03], big[(pick >= 0.03) & (pick < 0.06)], big[(pick >= 0.06) & (pick < 0.09)] = nan, inf, -inf
    big[2:, 2:, 3:] = up
    big[:2, :2, :2] = -up
    out["random_5x4x3"] = (big, STEP, 0.0, 1.0, 1.0, None)
    return out


def by_the_words(corners, step, iso, l_out, l_in):
    """The rule block by block and corner by corner, in Python's float64 on float32 values: a second reading of the definition."""
    b_out, b_in = P.bounds(step, l_out, l_in)
    mz, my, mx = (n - 1 for n in corners.shape)
    flags = np.ones((mz, my, mx), bool)
    for bk in range(mz):
        for bj in range(my):
            for bi in range(mx):
                with np.errstate(invalid="ignore"):
                    d = [f32(corners[bk + cz, bj + cy, bi + cx] - f32(iso)) for cz in (0, 1) for cy in (0, 1) for cx in (0, 1)]
                flags[bk, bj, bi] = not (all(float(x) > float(b_out) for x in d) or all(float(x) < -float(b_in) for x in d))
    return flags


@pytest.mark.parametrize("name", sorted(handmade()))
def test_handmade_corners(name):
    corners, step, iso, l_out, l_in, want = handmade()[name]
    got = P.candidates_of_corners(corners, step, iso, l_out, l_in)
    assert got.shape == tuple(n - 1 for n in corners.shape)
    if want is not None:
        assert got.reshape(-1).tolist() == [bool(w) for w in want], name
    assert (got == by_the_words(corners, step, iso, l_out, l_in)).all(), name


def test_the_bounds():
    b_out, b_in = P.bounds(STEP, 1.0, 0.5)
    assert h.bits(b_out) == h.bits(f32(f32(4) * np.sqrt(f32(0.328125)))) and h.bits(b_in) == h.bits(f32(f32(0.5) * b_out))
    assert abs(float(b_out) - 4 * (0.25 ** 2 + 0.5 ** 2 + 0.125 ** 2) ** 0.5) < 1e-6
    assert P.bounds(STEP, inf, 0.0) == (inf, f32(0))
    huge = P.bounds((1e20, 1.0, 1.0), 0.5, 0.0)
    assert huge[0] == inf and np.isnan(huge[1])
    # half a block's diagonal: no point of a block is farther from its nearest corner
    assert float(b_out) >= np.linalg.norm(4 * STEP.astype(np.float64)) * (1 - 1e-7)


# ---------------------------------------------------------------- (c) the library's header on the CPU
@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    """As sdf_helpers.build_cpu_program builds its program: g++, the address and undefined-behaviour sanitizers linked in statically,
    -ffp-contract=off."""
    exe = os.path.join(str(tmp_path_factory.mktemp("sdf_prune_cpu")), "rm_blocks_prune_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, corners, step, iso, l_out, l_in):
    mz, my, mx = (n - 1 for n in corners.shape)
    src, dst = os.path.join(str(directory), "corners.bin"), os.path.join(str(directory), "flags.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<3i", mx, my, mz))
        f.write(np.asarray(step, f32).tobytes() + np.array([iso, l_out, l_in], f32).tobytes())
        f.write(np.ascontiguousarray(corners, f32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 8 + 4 * mx * my * mz
    return np.frombuffer(raw, f32, 2), np.frombuffer(raw, np.uint32, mx * my * mz, 8).reshape(mz, my, mx)


def assert_cpu_equals_spec(exe, directory, corners, step, iso, l_out, l_in, what):
    bounds, flags = run_cpu_program(exe, directory, corners, step, iso, l_out, l_in)
    h.assert_bit_equal(bounds, np.array(P.bounds(step, l_out, l_in), f32), f"{what}: the bounds")
    want = P.candidates_of_corners(corners, step, iso, l_out, l_in).astype(np.uint32)
    assert (flags == want).all(), f"{what}: {int((flags != want).sum())} flags differ, first at {np.argwhere(flags != want)[:5].tolist()}"


@pytest.mark.parametrize("name", SCENES)
def test_the_shared_header_on_the_cpu_equals_the_spec_on_the_oracles_lattices(cpu_program, tmp_path, name):
    dense, step, iso = lattice(name)
    for l_out, l_in in ((1.0, inf), (1.0, 1.0), (0.125, inf), (0.0, 0.0), (inf, inf)):
        assert_cpu_equals_spec(cpu_program, tmp_path, dense[::8, ::8, ::8], step, iso, l_out, l_in, f"{name} ({l_out}, {l_in})")


def test_the_shared_header_on_the_cpu_equals_the_spec_on_the_handmade_corners(cpu_program, tmp_path):
    for name, (corners, step, iso, l_out, l_in, _want) in handmade().items():
        assert_cpu_equals_spec(cpu_program, tmp_path, corners, step, iso, l_out, l_in, name)
