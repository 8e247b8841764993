"""The shared comparator, table builder and spec loader of tests/helpers.py, without a GPU: assert_bit_equal must fail on everything
the bit-exactness tests rely on it to catch (signed zeros, NaN payloads, a broadcast, a conversion by value), tables_of must copy
exactly the arrays that are not writeable, and load_spec must compile a specification once."""
import ctypes as C
import os

import numpy as np
import pytest

import gbuffer_helpers as G
import helpers as h

F32 = np.float32


def f32_of(*words):
    return np.array(words, dtype=np.uint32).view(F32)


def test_equal_words_pass():
    a = f32_of(0x00000000, 0x80000000, 0x7FC00000, 0x7FA5A5A5, 0x3F800000).reshape(1, 5)
    h.assert_bit_equal(a, a.copy(), "same words")
    h.assert_bit_equal(a[:, ::2], a.copy()[:, ::2], "same words, not contiguous")


def test_signed_zeros_differ():
    with pytest.raises(AssertionError, match="1 of 2 words differ"):
        h.assert_bit_equal(np.array([0.0, 1.0], F32), np.array([-0.0, 1.0], F32), "zeros")


def test_nan_payloads_differ():
    a, b = f32_of(0x7FC00000), f32_of(0xFFC00000)  # the host's and the GPU's arithmetic NaN
    assert np.isnan(a).all() and np.isnan(b).all()
    with pytest.raises(AssertionError, match="words differ"):
        h.assert_bit_equal(a, b, "sign of a NaN")
    with pytest.raises(AssertionError, match="words differ"):
        h.assert_bit_equal(f32_of(0x7FC00000), f32_of(0x7FC00001), "payload of a NaN")


def test_shapes_are_not_broadcast():
    a = np.arange(4, dtype=F32)
    with pytest.raises(AssertionError, match="shape"):
        h.assert_bit_equal(a.reshape(1, 4), a, "(1, 4) against (4,)")


def test_float64_is_refused_not_converted():
    a = np.array([1.0, 2.0], F32)
    for got, want in ((a.astype(np.float64), a), (a, a.astype(np.float64))):
        with pytest.raises(AssertionError, match="4-byte"):
            h.assert_bit_equal(got, want, "float64 operand")
    with pytest.raises(AssertionError, match="4-byte"):
        h.bits(a.astype(np.float64))


def test_int32_against_float32_compares_words_not_values():
    with pytest.raises(AssertionError, match="words differ"):
        h.assert_bit_equal(np.array([1], np.int32), np.array([1.0], F32), "int32 1 against float32 1.0")
    ids = np.array([-4, -1, 0, 7, 2 ** 31 - 1], np.int32)
    h.assert_bit_equal(h.bits(ids), h.bits(ids.view(F32)), "an int32 array against its own float32 view")
    h.assert_bit_equal(ids, ids.view(F32), "… and without bits()")


def test_tables_of_copies_exactly_the_read_only_arrays():
    scene = h.scene_mandelbulb(8, 8)
    shared = np.zeros((4, 4, 4), np.uint8)
    shared.setflags(write=False)
    fresh = np.ones((4, 4, 4), np.uint8)
    faces = [fresh] * 6
    t = h.tables_of(scene + ("ignored",), {"noise": shared}, ltc1=fresh, skybox=faces)
    assert t.noise is not shared and t.noise.flags.writeable and (t.noise == shared).all()
    assert t.ltc1 is fresh and t.skybox is faces
    assert t.camera is scene[0] and t.objects is scene[1] and t.num_lights == 3 and t.globals_ is scene[5]
    assert h.tables_of(scene).noise is None


def test_load_spec_compiles_once_and_hands_out_one_handle():
    lib = G.spec()
    so = os.path.join(h.ROOT, "tests", "gbuffer_spec", "_build", "librm_gbuffer_spec.so")
    stamp = os.stat(so).st_mtime_ns
    again = h.load_spec("gbuffer", G.SIGNATURES)
    assert again is lib and G.spec() is lib
    assert os.stat(so).st_mtime_ns == stamp
    assert lib.rmo_spec_gbuffer.restype is C.c_int and len(lib.rmo_spec_gbuffer.argtypes) == 10
