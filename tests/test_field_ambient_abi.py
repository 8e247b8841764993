"""rm_field_ambient and rm_hemisphere_directions without a GPU: the header declares them and the library exports them under the
unchanged ABI version, RmAmbient has 32 bytes, every refusal that comes before the handle is looked at or needs no live handle is
returned before the first HIP call — with pointers that would fault if read —, the table of directions is what the header says, and
the Python layer has its methods.  What needs a live handle is in tests/test_gpu_field_ambient.py."""
import ctypes as C
import inspect
import re

import numpy as np

import abi_helpers as ah
from abi_helpers import FAKE, HEADER, refused
from raymarcher_amd import abi, hemisphere_directions, lib
from raymarcher_amd._lib import SIGNATURES

f32 = np.float32
NAMES = {"rm_hemisphere_directions": 3, "rm_field_ambient": 14}


def test_header_declares_and_library_exports_the_symbols():
    assert ah.params("rm_hemisphere_directions") == ["int numDirs", "int numSets", "float *out4"]
    assert ah.params("rm_field_ambient") == [
        "const RmField *field", "const float *d_points", "const float *d_normals", "int numPoints", "const float *d_dirs", "int numDirs",
        "int numSets", "float bias", "float maxDistance", "float iso", "int maxSteps", "unsigned mode", "RmAmbient *d_out", "void *stream"]
    assert HEADER.index("typedef struct RmAmbient {") > HEADER.index("int  rm_field_trace(")
    assert HEADER.index("int rm_field_ambient(") < HEADER.index("rm_shade_points —")
    ah.assert_exported(NAMES)
    for name, n in NAMES.items():
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == n == len(ah.params(name)) and SIGNATURES[name][0] is C.c_int


def test_abi_version_stays_and_the_record_has_32_bytes():
    ah.assert_abi_version()
    assert C.sizeof(abi.RmAmbient) == 32
    assert [f[0] for f in abi.RmAmbient._fields_] == ["bent", "visibility", "normal", "hits"]
    assert abi.RmAmbient.visibility.offset == 12 and abi.RmAmbient.normal.offset == 16 and abi.RmAmbient.hits.offset == 28
    assert re.search(r"typedef struct RmAmbient \{ float bent\[3\]; float visibility; float normal\[3\]; int32_t hits; \} RmAmbient;\s*/\* 32 bytes \*/",
                     HEADER)
    for name, value in (("RM_AMBIENT_SOFT", "0u"), ("RM_AMBIENT_HARD", "1u"), ("RM_MAX_AMBIENT_DIRS", "256"), ("RM_MAX_AMBIENT_TABLE", "1024")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", HEADER), name
    assert (abi.RM_AMBIENT_SOFT, abi.RM_AMBIENT_HARD, abi.RM_MAX_AMBIENT_DIRS, abi.RM_MAX_AMBIENT_TABLE) == (0, 1, 256, 1024)
    ah.assert_comment_has("RmAmbient", (
        "ONE binary32 operation", "copysign(1, n.z)", "a = −1 / (s + n.z)", "n.z = −1 gives a = 0.5", "s[j] = s[2j] + s[2j + 1]",
        "i mod numSets", "h.t > 0 ? h.t : 0", "sign and payload", "Then numPoints == 0: RM_OK", "d_normals included when it is given",
        "No device", "0.6180339887498949", "0.7548776662466927", "rm_debug_last_path() keeps its value"))


def ambient(field=None, points=FAKE, normals=FAKE, n=5, dirs=FAKE, num_dirs=16, num_sets=1, bias=0.05, max_distance=1.0, iso=0.001, steps=64,
            mode=0, out=FAKE):
    return lib().rm_field_ambient(field, points, normals, n, dirs, num_dirs, num_sets, bias, max_distance, iso, steps, mode, out, None)


def test_a_null_handle_is_refused_before_anything_else():
    assert refused(ambient(), "null or stale RmField handle")
    assert refused(ambient(n=-1, num_dirs=3, num_sets=0, bias=float("nan"), steps=-1, mode=7), "handle")
    assert refused(ambient(n=0, points=None, normals=None, dirs=None, out=None), "handle")  # before the empty call
    # a pointer that is not a handle: misaligned ones are refused unread
    assert refused(ambient(field=C.c_void_p(0x1001)), "null or stale RmField handle")


BAD_DIRS = (0, -1, 3, 6, 12, 24, 96, 255, 257, 512, 1024, 2 ** 31 - 1, -2 ** 31)
GOOD_SHAPES = ((1, 1), (1, 1024), (2, 512), (16, 64), (64, 16), (256, 4), (256, 1), (128, 8))
BAD_SETS = ((1, 0), (1, -1), (1, 1025), (256, 5), (16, 65), (64, 17), (2, 2 ** 30), (4, 2 ** 31 - 1), (1, -2 ** 31))


def test_hemisphere_directions_refusals():
    buf = np.zeros((1024, 4), f32)
    out = C.c_void_p(buf.ctypes.data)
    for k in BAD_DIRS:
        assert refused(lib().rm_hemisphere_directions(k, 1, out), "numDirs must be a power of two"), k
        assert refused(lib().rm_hemisphere_directions(k, 0, None), "numDirs"), k  # numDirs comes first
    for k, s in BAD_SETS:
        assert refused(lib().rm_hemisphere_directions(k, s, out), "numSets"), (k, s)
        assert refused(lib().rm_hemisphere_directions(k, s, None), "numSets"), (k, s)  # and numSets before out4
    assert (buf == 0).all()
    for k, s in GOOD_SHAPES:
        assert refused(lib().rm_hemisphere_directions(k, s, None), "null out4"), (k, s)
        assert lib().rm_hemisphere_directions(k, s, out) == abi.RM_OK, (k, s)


def test_hemisphere_directions_is_the_headers_table():
    for k, s in GOOD_SHAPES + ((64, 3), (4, 3)):
        t = hemisphere_directions(k, s)
        assert t.shape == (k * s, 4) and t.dtype == f32
        again = hemisphere_directions(k, s)
        assert (t.view(np.uint32) == again.view(np.uint32)).all(), "two calls, the same bits"
        # unit to within 2 ulp of 1: the components are rounded from a double unit vector, the length is taken in double
        length = np.sqrt((t[:, 0:3].astype(np.float64) ** 2).sum(axis=1))
        assert (np.abs(length - 1.0) <= 2 * 2.0 ** -23).all(), (k, s, np.abs(length - 1.0).max())
        assert (t[:, 2] > 0).all() and (t[:, 3] == f32(1.0 / k)).all() and f32(1.0 / k) * k == 1
        sets = t.reshape(s, k, 4)
        for a in range(s):
            kk = np.arange(k, dtype=np.float64)
            u = (kk + 0.5) / k
            turn = kk * 0.6180339887498949 + a * 0.7548776662466927
            phi = 2 * np.pi * (turn - np.floor(turn))
            want = np.stack([np.sqrt(u) * np.cos(phi), np.sqrt(u) * np.sin(phi), np.sqrt(1 - u)], axis=1)
            assert np.abs(sets[a, :, 0:3] - want).max() <= 2.0 ** -23, (k, s, a)  # libm against NumPy: rounding and an ulp of the double
            assert (sets[a, :, 2] == np.sqrt(1 - u).astype(f32)).all()           # sqrt is correctly rounded in both
            for b in sorted({0, a // 2, a - 1} - {a, -1}):
                assert (sets[a, :, 0:2] != sets[b, :, 0:2]).any(), "the sets differ"
                assert (sets[a, :, 2:4] == sets[b, :, 2:4]).all(), "by a rotation about the normal"


def test_python_signatures():
    from raymarcher_amd import LatticeField
    from raymarcher_amd.render import Renderer
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(hemisphere_directions) == ["num_dirs", "num_sets"] and inspect.signature(hemisphere_directions).parameters["num_sets"].default == 1
    assert sig(LatticeField.ambient) == ["self", "points", "normals", "directions", "sets", "max_distance", "bias", "iso", "max_steps", "soft", "out"]
    p = inspect.signature(LatticeField.ambient).parameters
    assert ([p[k].default for k in ("normals", "directions", "sets", "max_distance", "bias", "iso", "max_steps", "soft", "out")]
            == [None, 16, 1, None, None, 0.001, 64, True, None])
    assert "bias" in LatticeField.ambient.__doc__ and "must exceed" in LatticeField.ambient.__doc__
    assert sig(Renderer.bake_mesh_pruned_ambient) == (sig(Renderer.bake_mesh_pruned)[:4] + ["ambient"] + sig(Renderer.bake_mesh_pruned)[4:])
    assert inspect.signature(Renderer.bake_mesh_pruned_ambient).parameters["ambient"].default == 16
    for f in (Renderer.bake_mesh, Renderer.bake_mesh_sparse, Renderer.bake_mesh_pruned):  # as they were
        assert "ambient" not in inspect.signature(f).parameters
    # the Python wrapper raises what the library refuses
    import pytest
    from raymarcher_amd import RaymarcherError
    with pytest.raises(RaymarcherError):
        hemisphere_directions(3)
    with pytest.raises(RaymarcherError):
        hemisphere_directions(256, 5)
