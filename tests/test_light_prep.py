"""The per-light constants the launcher stages for the bulb kernels' shadow pool (rm_debug_light_prep, no GPU needed): L =
normalize(−dir), pd = invModel·L (3×3) and a = dot(pd, pd), word for word what the oracle's normalize3 and the cull's products
written with the oracle's rm_fma give (tests/light_prep_spec).  The host code stands in for arithmetic the kernels did per ray, so
every word counts: random directions, magnitudes where the square root takes its scaled path and the reciprocal its IEEE form,
signed zeros, rotated and non-uniformly scaled models, and the directions the table check admits although no light has them
(zero, infinite, NaN)."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from raymarcher_amd import abi, lib

P = C.POINTER
SIGNATURES = {"rmo_spec_light_prep": (C.c_int, [P(abi.RmObject), C.c_int, P(abi.RmLight), C.c_int, P(C.c_float)])}

MODELS = {
    "identity": None,
    "rotated": h.rotation((1, 2, 0.5), 0.6),
    "scaled": h.scale(0.7, 1.9, 1.1),
    "rotated_scaled_moved": h.translate(0.3, -0.2, 0.1) @ h.rotation((0.2, -1, 0.4), 2.1) @ h.scale(1.3, 0.45, 2.2),
    "tiny": h.scale(1e-3, 1e-3, 1e-3),
}


def both(objs, no, dirs):
    """(staged, specified) constants, (n, 8) each, of directional lights with the float32 directions `dirs`, RM_MAX_LIGHTS at a time."""
    dirs = np.asarray(dirs, dtype=np.float32).reshape(-1, 3)
    got, want = np.zeros((len(dirs), 8), np.float32), np.full((len(dirs), 8), 7.0, np.float32)
    spec = h.load_spec("light_prep", SIGNATURES)
    for at in range(0, len(dirs), abi.RM_MAX_LIGHTS):
        part = dirs[at:at + abi.RM_MAX_LIGHTS]
        lights = (abi.RmLight * len(part))()
        for li, d in zip(lights, part):
            li.type = abi.RM_LIGHT_DIRECTIONAL
            for k in range(3):
                li.dir[k] = d[k]  # a c_float field takes the binary32 value as it is
        g, w = got[at:at + len(part)], want[at:at + len(part)]
        assert lib().rm_debug_light_prep(objs, no, lights, len(part), h.fptr(g)) == 0
        assert spec.rmo_spec_light_prep(objs, no, lights, len(part), h.fptr(w)) == 0
    return got, want


def bulb(model):
    return (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=model))


def same(got, want, what):
    """Word for word; a NaN word may be any NaN (the kernels read a NaN direction through comparisons and min / max only, and the
    sign and payload of an invalid operation's NaN are the processor's)."""
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN words differ"
    h.assert_bit_equal(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), what)


@pytest.mark.parametrize("model", sorted(MODELS))
def test_random_directions(model):
    rng = np.random.default_rng(20)
    dirs = rng.standard_normal((400, 3)).astype(np.float32) * rng.choice(np.float32([0.01, 1, 1, 300]), (400, 1))
    got, want = both(bulb(MODELS[model]), 1, dirs)
    assert not np.isnan(want).any()
    h.assert_bit_equal(got, want, f"random directions, {model} model")
    assert (np.abs(np.linalg.norm(got[:, :3].astype(np.float64), axis=1) - 1) < 1e-6).all()


@pytest.mark.parametrize("mag", [1e-20, 3e-23, 1e-38, 1e19, 3e18, 1.5e19, 2e38])
def test_extreme_magnitudes(mag):
    """|dir|² below 2^-96 (the square root's scaled path, denormal squares), and |dir| where the length or its reciprocal leaves
    the fast reciprocal's range or the dot product overflows."""
    rng = np.random.default_rng(21)
    with np.errstate(over="ignore"):  # 2e38: some components are infinite, which is the point
        dirs = (rng.standard_normal((100, 3)) * mag).astype(np.float32)
    for name in ("identity", "rotated_scaled_moved"):
        got, want = both(bulb(MODELS[name]), 1, dirs)
        same(got, want, f"|dir| ~ {mag}, {name} model")


def test_axis_directions_and_signed_zeros():
    z = np.float32(0.0)
    dirs = [(sx * a, sy * b, sz * c) for a, b, c in ((1, z, z), (z, 1, z), (z, z, 1), (2.5, z, z), (z, -0.3, z), (1, 1, z))
            for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    for name in ("identity", "scaled", "rotated"):
        got, want = both(bulb(MODELS[name]), 1, dirs)
        h.assert_bit_equal(got, want, f"axis directions, {name} model")
    got, _ = both(bulb(None), 1, [(0.0, 0.0, 1.0), (-0.0, -0.0, 1.0)])
    # L = −dir·(1 / len): the zeros keep the sign the negation gives them
    assert h.bits(got[0, :3]).tolist() == [0x80000000, 0x80000000, 0xbf800000]
    assert h.bits(got[1, :3]).tolist() == [0x00000000, 0x00000000, 0xbf800000]


def test_directions_no_light_has():
    """validate_scene does not look at a light's direction: zero, infinite and NaN ones reach the kernels, which take what
    normalize gives for them (NaN, zeros) and leave the pool's shared first step."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    dirs = [(0, 0, 0), (-0.0, 0, 0), (inf, 0, 0), (1, -inf, 2), (nan, 1, 0), (1, 1, nan), (3e38, 3e38, 0)]
    for name in ("identity", "rotated_scaled_moved"):
        got, want = both(bulb(MODELS[name]), 1, dirs)
        same(got, want, f"degenerate directions, {name} model")
    assert np.isnan(got[0, :3]).all() and np.isnan(got[4, :3]).all()


def test_other_lights_and_empty_tables():
    lights = (abi.RmLight * 3)(h.make_light(abi.RM_LIGHT_POINT, pos=(1, 2, 3), direction=(0, 1, 0)),
                               h.make_light(abi.RM_LIGHT_DIRECTIONAL, direction=(0.3, -1, 0.2)),
                               h.make_light(abi.RM_LIGHT_SPOT, pos=(1, 2, 3), direction=(0, 1, 0), angle=0.5, penumbra=0.1))
    objs = bulb(MODELS["rotated"])
    got, want = np.full((3, 8), 5.0, np.float32), np.zeros((3, 8), np.float32)
    assert lib().rm_debug_light_prep(objs, 1, lights, 3, h.fptr(got)) == 0
    assert h.load_spec("light_prep", SIGNATURES).rmo_spec_light_prep(objs, 1, lights, 3, h.fptr(want)) == 0
    h.assert_bit_equal(got, want, "mixed table")
    assert not got[0].any() and not got[2].any() and got[1, :7].all()
    none = np.full((3, 8), 5.0, np.float32)
    assert lib().rm_debug_light_prep(None, 0, lights, 3, h.fptr(none)) == 0
    h.assert_bit_equal(none[1, :3], got[1, :3], "L without an object table")
    assert not none[1, 3:].any()
    assert lib().rm_debug_light_prep(objs, 1, None, 0, h.fptr(none)) == 0
    for bad in ((None, 1, lights, 3), (objs, 1, None, 2), (objs, -1, lights, 3), (objs, 1, lights, abi.RM_MAX_LIGHTS + 1),
                (objs, abi.RM_MAX_OBJECTS + 1, lights, 3)):
        assert lib().rm_debug_light_prep(*bad, h.fptr(none)) == abi.RM_ERR_INVALID_ARGUMENT
    assert lib().rm_debug_light_prep(objs, 1, lights, 3, None) == abi.RM_ERR_INVALID_ARGUMENT
