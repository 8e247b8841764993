"""rm_rays_order without a GPU: the library's key header (raymarcher_amd/csrc/rm_ray_key.h), compiled into a stand-alone CPU program
under the host sanitizers and run as a child process, against the NumPy specification (tests/ray_order_spec.py) in every bit; then
the properties of the specification itself, and that the ordering does what it is for."""
import numpy as np
import pytest

import ray_order_helpers as R
import ray_order_spec as S


@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    return R.build_cpu_program(tmp_path_factory.mktemp("ray_order_cpu"))


@pytest.mark.parametrize("bits", S.BIT_PAIRS)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_the_key_header_equals_the_specification_in_every_bit(cpu_program, tmp_path, name, bits):
    rays = R.family(name)
    got = R.run_cpu_program(cpu_program, tmp_path, rays, *bits)
    want = S.keys(rays, *bits)
    bad = got["keys"] != want
    assert not bad.any(), f"{name} {bits}: {bad.sum()} keys differ, the first at {np.argwhere(bad)[:5].ravel().tolist()}"
    assert (got["order"] == S.order(rays, *bits)).all(), f"{name} {bits}: order"
    lo, hi = S.bounds(rays)
    assert (got["lo"] == lo).all() and (got["hi"] == hi).all(), f"{name} {bits}: bounds by value (the sign of a zero is free)"


def test_the_whole_camera_frame_and_tiny_arrays(cpu_program, tmp_path):
    rays = R.camera_frame()[0]
    got = R.run_cpu_program(cpu_program, tmp_path, rays, 10, 11)
    assert (got["keys"] == S.keys(rays, 10, 11)).all() and (got["order"] == S.order(rays, 10, 11)).all()
    for n in (0, 1, 2):
        got = R.run_cpu_program(cpu_program, tmp_path, R.family("box")[:n], 7, 8)
        assert (got["keys"] == S.keys(R.family("box")[:n], 7, 8)).all() and got["order"].tolist() == S.order(R.family("box")[:n], 7, 8).tolist()
    none = R.specials()[:20]  # not one valid ray: every key is the invalid key, the order the identity
    assert not S.valid(none).any()
    got = R.run_cpu_program(cpu_program, tmp_path, none, 10, 11)
    assert (got["keys"] == np.uint64(1 << 52)).all() and (S.keys(none, 10, 11) == np.uint64(1 << 52)).all()
    assert got["order"].tolist() == list(range(20))


@pytest.mark.parametrize("bits", S.BIT_PAIRS)
@pytest.mark.parametrize("name", R.FAMILIES)
def test_order_is_a_permutation_with_the_invalid_rays_last_in_input_order(name, bits):
    rays = R.family(name)
    order, keys, valid = S.order(rays, *bits), S.keys(rays, *bits), S.valid(rays)
    assert sorted(order.tolist()) == list(range(len(rays)))
    nv = int(valid.sum())
    assert valid[order[:nv]].all() and order[nv:].tolist() == np.nonzero(~valid)[0].tolist()
    top = np.uint64(1) << np.uint64(3 * bits[0] + 2 * bits[1])
    assert (keys[valid] < top).all() and (keys[~valid] == top).all()
    assert (np.diff(keys[order].astype(np.int64)) >= 0).all()
    ties = np.diff(keys[order].astype(np.int64)) == 0
    assert (np.diff(order)[ties] > 0).all(), "equal keys keep their input order"


def test_validity_reads_the_geometry_only():
    sp = R.specials()
    valid = S.valid(sp)
    assert not valid[:20].any() and valid[20:].all()  # 18 non-finite rows, 2 zero directions; tMax NaN or negative does not matter
    again = sp.copy()
    again[:, 3], again[:, 7] = np.nan, np.inf
    for bits in S.BIT_PAIRS:
        assert (S.keys(again, *bits) == S.keys(sp, *bits)).all()


@pytest.mark.parametrize("name", R.FAMILIES)
def test_no_bits_give_the_identity_on_the_valid_rays(name):
    rays = R.family(name)
    valid = S.valid(rays)
    assert (S.keys(rays, 0, 0)[valid] == 0).all()
    nv = int(valid.sum())
    assert S.order(rays, 0, 0)[:nv].tolist() == np.nonzero(valid)[0].tolist()


@pytest.mark.parametrize("name", ["specials", "flat", "box"])
def test_the_sign_of_a_zero_bound_changes_no_key(cpu_program, tmp_path, name):
    rays = np.array(R.family(name))
    if name == "box":  # bounds that ARE zeros: the smallest x and the largest z of the origins, and a direction along −x … +x
        rays[:, 0] -= rays[:, 0].min()
        rays[:, 2] -= rays[:, 2].max()
    lo, hi = S.bounds(rays)
    assert name != "box" or (lo[0] == 0 and hi[2] == 0)
    flip = lambda b: np.where(b == 0, -b, b).astype(np.float32)  # noqa: E731
    for bits in S.BIT_PAIRS:
        want = S.keys(rays, *bits)
        assert (S.keys(rays, *bits, lo_hi=(flip(lo), flip(hi))) == want).all(), bits
        assert (S.keys(rays, *bits, lo_hi=(flip(lo), hi)) == want).all() and (S.keys(rays, *bits, lo_hi=(lo, flip(hi))) == want).all(), bits
        assert (R.run_cpu_program(cpu_program, tmp_path, rays, *bits, flip_zeros=True)["keys"] == want).all(), bits


def test_quantisation_edges():
    f = np.float32
    x = np.array([0.0, 1.0, 0.5, np.nextafter(f(1), f(0)), np.nextafter(f(0), f(1)), -0.0, 0.25], f)
    assert S.quantise(x, f(0), f(1), 11).tolist() == [0, 2047, 1024, 2047, 0, 0, 512]
    assert S.quantise(x, f(0), f(1), 0).tolist() == [0] * 7
    assert S.quantise(x, f(1), f(1), 8).tolist() == [0] * 7 and S.quantise(x, f(np.inf), f(-np.inf), 8).tolist() == [0] * 7
    big = np.array([3e38, -3e38, 0.0], f)  # hi − lo = +inf: t is inf / inf = NaN at the top, 0 below
    assert S.quantise(big, f(-3e38), f(3e38), 10).tolist() == [0, 0, 0]


def test_the_order_makes_waves_coherent_on_a_shuffled_camera_frame():
    """The usefulness condition, on the specification alone: runs of 64 consecutive rays of the ordered, shuffled 96×64 frame
    cover a median pixel bounding box of at most 512 px (the ideal is 64; the shuffled input gives thousands)."""
    rays, pixels = R.camera_frame()
    shuffled = S.median_wave_box(np.arange(len(rays)), pixels)
    ordered = S.median_wave_box(S.order(rays, 10, 11), pixels)
    print(f"median pixel bounding box of a wave: ordered {ordered:.0f} px, shuffled {shuffled:.0f} px")
    assert shuffled > 2000
    assert ordered <= 512
