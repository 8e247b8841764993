"""rm_probe_sdscene_variant without a GPU: the header declares it, the library exports it, and it accepts exactly the scene
evaluator instantiations that production kernels compile, refusing everything else before the first HIP call.  Also the CPU
oracle's Mandelbulb against the binary64 arbiter, where the value is well conditioned and where binary32 overflows."""
import ctypes as C
import itertools

import numpy as np

import abi_helpers as ah
import helpers as h
from abi_helpers import FAKE
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

# (bulbClass, count, trap, skip, track, one) of every production instantiation, from the call sites in rm_device.hip.h and
# rm_wavefront.hip.h: march (TRAP = !SHADOW, SKIP = TRACK = CULL && !BULB && COUNT != 1, sdSceneOne on its fast path), getNormal
# and calcAO (TRAP 0, SKIP the same), the shadow pools and refraction march (no SKIP), the wavefront march (COUNT 0, TRAP 2 / 0,
# SKIP either, no TRACK); the plain bulb form only in the COUNT 0 kernels.
ACCEPTED = set()
for count in (0, 1, 2):
    for trap in (0, 1):
        ACCEPTED.add((0, count, trap, 0, 0, 0))
        ACCEPTED.add((1, count, trap, 0, 0, 0))
        if count != 1:
            ACCEPTED.add((0, count, trap, 1, 1, 0))
            ACCEPTED.add((0, count, trap, 1, 1, 1))
    if count != 1:
        ACCEPTED.add((0, count, 0, 1, 0, 0))
ACCEPTED |= {(2, 0, 0, 0, 0, 0), (2, 0, 1, 0, 0, 0), (0, 0, 2, 0, 0, 0), (0, 0, 2, 1, 0, 0)}

NOT_INSTANTIATED = b"no production kernel instantiates this sdScene variant"


def _tables(kind):
    if kind == "bulb":
        return (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB)), 1, h.make_globals()
    objs = [h.make_object(abi.RM_CUBE), h.make_object(abi.RM_SPHERE, model=h.translate(1, 0, 0)),
            h.make_object(abi.RM_MENGERSPONGE, model=h.translate(-2, 0, 0)), h.make_object(abi.RM_MANDELBULB, model=h.translate(0, 3, 0))]
    return (abi.RmObject * len(objs))(*objs), len(objs), h.make_globals()


def call(objs, no, g, cls, count, trap, skip, track, one, pts=None, out=None, n=1, s=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_probe_sdscene_variant(objs, no, C.byref(g), C.byref(s), cls, count, trap, skip, track, one, pts, None, out, n,
                                          None)


def test_header_declares_and_library_exports_the_variant_probe():
    assert ah.params("rm_probe_sdscene_variant")
    assert ah.params("rm_probe_sdscene")  # the original probe stays
    assert "rm_probe_sdscene_variant" in SIGNATURES
    ah.assert_exported(["rm_probe_sdscene_variant"])


def test_exactly_the_production_instantiations_are_accepted():
    """Every combination in a grid around the legal ones: the accepted ones get as far as the (null) point pointer, every other
    one is refused for its combination.  Nothing reaches a HIP call (null pointers fail before require_device_pointers)."""
    L = lib()
    bulb, walk = _tables("bulb"), _tables("walk")
    seen = set()
    for cls, count, trap, skip, track, one in itertools.product((-1, 0, 1, 2, 3), (-1, 0, 1, 2, 3), (-1, 0, 1, 2, 3), (0, 1, 2),
                                                                 (0, 1), (0, 1)):
        objs, no, g = bulb if cls in (1, 2) else walk
        st = call(objs, no, g, cls, count, trap, skip, track, 0 if one else -1)
        assert st == abi.RM_ERR_INVALID_ARGUMENT
        err = L.rm_last_error()
        key = (cls, count, trap, skip, track, one)
        if key in ACCEPTED:
            assert err == b"bad probe arguments", (key, err)
            seen.add(key)
        else:
            assert err == NOT_INSTANTIATED, (key, err)
    assert seen == ACCEPTED


def test_bulb_classes_need_a_single_mandelbulb():
    L = lib()
    walk = _tables("walk")
    cube = ((abi.RmObject * 1)(h.make_object(abi.RM_CUBE)), 1, h.make_globals())
    two = ((abi.RmObject * 2)(h.make_object(abi.RM_MANDELBULB), h.make_object(abi.RM_MANDELBULB)), 2, h.make_globals())
    for objs, no, g in (walk, cube, two):
        for cls in (1, 2):
            assert call(objs, no, g, cls, 0, 1, 0, 0, -1) == abi.RM_ERR_INVALID_ARGUMENT
            assert L.rm_last_error() == b"a bulb class needs a table of one Mandelbulb"


def test_plain_bulb_refused_where_bulb_plain_rejects_the_table():
    L = lib()
    bulb = h.make_object(abi.RM_MANDELBULB)
    cases = [
        ((abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=h.translate(0.5, 0, 0))), h.make_globals()),
        ((abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, scale_factor=0.5)), h.make_globals()),
        ((abi.RmObject * 1)(bulb), h.make_globals(power=7.0)),
        ((abi.RmObject * 1)(bulb), h.make_globals(julia=(0.25, 0.0))),
    ]
    for objs, g in cases:
        assert L.rm_debug_bulb_plain(objs, 1, C.byref(g)) == 0
        assert call(objs, 1, g, 2, 0, 1, 0, 0, -1) == abi.RM_ERR_INVALID_ARGUMENT
        assert L.rm_last_error() == b"the plain bulb form does not apply to this table"
        # the general form takes the same table as far as the pointers
        assert call(objs, 1, g, 1, 0, 1, 0, 0, -1) == abi.RM_ERR_INVALID_ARGUMENT
        assert L.rm_last_error() == b"bad probe arguments"
    # and the plain table itself, with -0 off the diagonal (what the scenefile loader writes), is accepted
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB))
    objs[0].invModel[1] = -0.0
    assert call(objs, 1, h.make_globals(), 2, 0, 1, 0, 0, -1) == abi.RM_ERR_INVALID_ARGUMENT
    assert L.rm_last_error() == b"bad probe arguments"


def test_single_object_path_needs_a_primitive_in_range():
    L = lib()
    objs, no, g = _tables("walk")  # cube, sphere, Menger sponge, Mandelbulb
    for one in (-2, no, no + 5, 2, 3):
        assert call(objs, no, g, 0, 0, 1, 1, 1, one) == abi.RM_ERR_INVALID_ARGUMENT
        assert L.rm_last_error() == b"`one` must name a primitive of the table", one
    for one in (0, 1):
        assert call(objs, no, g, 0, 0, 1, 1, 1, one) == abi.RM_ERR_INVALID_ARGUMENT
        assert L.rm_last_error() == b"bad probe arguments"


def test_scene_and_pointer_errors():
    L = lib()
    objs, no, g = _tables("walk")
    s = abi.default_settings()
    assert lib().rm_probe_sdscene_variant(objs, no, None, C.byref(s), 0, 0, 1, 0, 0, -1, None, None, None, 1, None) \
        == abi.RM_ERR_INVALID_ARGUMENT
    assert lib().rm_probe_sdscene_variant(objs, abi.RM_MAX_OBJECTS + 1, C.byref(g), C.byref(s), 0, 0, 1, 0, 0, -1, None, None,
                                          None, 1, None) == abi.RM_ERR_CAPACITY
    assert call(objs, no, g, 0, 0, 1, 0, 0, -1, pts=FAKE, out=None) == abi.RM_ERR_INVALID_ARGUMENT
    assert call(objs, no, g, 0, 0, 1, 0, 0, -1, pts=FAKE, out=FAKE, n=-1) == abi.RM_ERR_INVALID_ARGUMENT
    assert L.rm_last_error() == b"bad probe arguments"


# ---------------------------------------------------------------- the bulb: binary32 oracle against the binary64 arbiter
def _oracle32(objs, g, s, pts):
    p = np.ascontiguousarray(pts, dtype=np.float32)
    out = np.empty((len(p), 6), dtype=np.float32)
    assert h.oracle().rmo_probe_sdscene_trap4(objs, len(objs), C.byref(g), C.byref(s), h.fptr(p), h.fptr(out), len(p)) == 0
    return out


def _arbiter64(objs, g, s, pts):
    p = np.ascontiguousarray(pts, dtype=np.float64)
    out = np.empty((len(p), 4), dtype=np.float64)
    dp = C.POINTER(C.c_double)
    st = h.arbiter().rmo_probe_sdscene(h._to_f64(objs), len(objs), C.byref(h._to_f64(g)), C.byref(s), p.ctypes.data_as(dp),
                                       out.ctypes.data_as(dp), len(p))
    assert st == 0
    return out


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def test_oracle_bulb_matches_the_binary64_arbiter_where_one_step_bails_out():
    """|p| in [2, 240] of the unit Mandelbulb: the first iteration takes |w| to about |p|^8 > sqrt(2), the loop stops, and the
    distance estimate 0.5·ln|w|·|w| / dz is well conditioned.  Measured over these 1e5 points: max relative difference 8.9e-7
    (the 99.9th percentile 7.2e-7); the bound 2e-6 leaves a margin of 2.25x."""
    rng = np.random.default_rng(20261016)
    n = 100_000
    r = np.exp(rng.uniform(np.log(2.0), np.log(240.0), n))
    pts = (_directions(rng, n) * r[:, None]).astype(np.float32)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB))
    g, s = h.make_globals(), abi.default_settings()
    a, b = _oracle32(objs, g, s, pts), _arbiter64(objs, g, s, pts.astype(np.float64))
    assert (a[:, 1] == 0).all() and (b[:, 1] == 0).all()
    assert np.isfinite(b[:, 0]).all() and (b[:, 0] > 0).all()
    rel = np.abs(a[:, 0].astype(np.float64) - b[:, 0]) / b[:, 0]
    assert rel.max() < 2e-6, (rel.max(), r[rel.argmax()])


def test_oracle_bulb_overflow_radius_gives_the_initial_minimum():
    """Beyond |p| ≈ 256 (2^(128/16): m = |w|² ≈ |p|^16 overflows binary32 after the first iteration) the bulb's value is inf
    or NaN, never below the initial minimum, and sdScene returns (1e6, −1) — the binary32 contract's value, while
    the arbiter still gives a finite distance.  Below 255 no direction overflows."""
    rng = np.random.default_rng(7)
    d = _directions(rng, 4000)
    objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB))
    g, s = h.make_globals(), abi.default_settings()
    for R in (2.0, 100.0, 240.0, 254.9):
        o = _oracle32(objs, g, s, (d * R).astype(np.float32))
        assert (o[:, 1] == 0).all() and np.isfinite(o[:, 0]).all(), R
    for R in (257.0, 266.0, 1000.0, 1e6, 1e19):
        pts = (d * R).astype(np.float32)
        o = _oracle32(objs, g, s, pts)
        assert (o[:, 0] == np.float32(1e6)).all() and (o[:, 1] == -1).all(), R
        if R < 1e3:
            b = _arbiter64(objs, g, s, pts.astype(np.float64))
            assert np.isfinite(b[:, 0]).all() and (b[:, 1] == 0).all(), R
    # in world space the radius scales with the object: a model scaled by 1e-2 (scaleFactor 1e-2) overflows from |p| ≈ 2.57
    M = h.scale(0.01, 0.01, 0.01)
    small = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=M, scale_factor=0.01))
    o = _oracle32(small, g, s, (d * 2.6).astype(np.float32))
    assert (o[:, 0] == np.float32(1e6)).all() and (o[:, 1] == -1).all()
