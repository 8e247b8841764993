"""rm_render_animated and rm_object_translated without a GPU: the header declares them, the library exports them under the unchanged
ABI version, every argument error — the table counts and an invalid table in a block other than the first among them — returns its
status before the first HIP call, and the translation helper is invModel · T(−t) in float64, rounded once."""
import ctypes as C
import inspect

import numpy as np
import pytest

import abi_helpers as ah
import helpers as h
from abi_helpers import FAKE, INT_MAX, refused
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES


# ---------------------------------------------------------------- the entry points
def test_header_declares_and_library_exports_both_symbols():
    assert ah.params("rm_render_animated") == [
        "const RmCamera *cams", "const RmGlobals *globals", "int numGlobals", "const RmObject *objs", "int numObjects",
        "int numObjectTables", "const RmLight *lights", "int numLights", "int numLightTables", "int numFrames",
        "int subFrames", "const RmSettings *s", "const RmResources *res", "int W", "int H", "float *d_rgba", "float *d_bright", "void *stream"]
    res, args = SIGNATURES["rm_render_animated"]
    P = C.POINTER
    assert res is C.c_int and args == [P(abi.RmCamera), P(abi.RmGlobals), C.c_int, P(abi.RmObject), C.c_int, C.c_int, P(abi.RmLight),
                                       C.c_int, C.c_int, C.c_int, C.c_int, P(abi.RmSettings), P(abi.RmResources), C.c_int, C.c_int,
                                       C.c_void_p, C.c_void_p, C.c_void_p]
    assert ah.params("rm_object_translated") == ["const RmObject *in", "const float t[3]", "RmObject *out"]
    assert SIGNATURES["rm_object_translated"] == (C.c_int, [P(abi.RmObject), P(C.c_float), P(abi.RmObject)])
    ah.assert_exported(["rm_render_animated", "rm_object_translated"])


def test_abi_version_stays():
    ah.assert_abi_version()
    assert lib().rm_abi_sizeof(0) == C.sizeof(abi.RmObject) == 176


def test_header_comment_carries_the_definition():
    ah.assert_comment_has("rm_render_animated", (
        "b = f·subFrames + j", "objs + b·numObjects", "lights + b·numLights", "rm_render_res writes for block b", "in that order",
        "binary32", "1.0f / (float)n", "is rm_render_accumulated, exactly", "names the block", "before any HIP call",
        "rm_debug_last_path() = 10", "symbol lookup"))


def test_python_signatures():
    from raymarcher_amd import translated_objects
    from raymarcher_amd.render import Renderer
    sig = inspect.signature(Renderer.render_animated)
    assert list(sig.parameters) == ["self", "tables", "settings", "W", "H", "cameras", "sub_frames", "objects", "lights", "globals_",
                                    "bright", "out", "out_bright"]
    assert sig.parameters["sub_frames"].default == 1 and sig.parameters["objects"].default is None
    seq = inspect.signature(Renderer.render_sequence).parameters
    for name in ("objects", "lights"):
        assert seq[name].kind is inspect.Parameter.KEYWORD_ONLY and seq[name].default is None
    assert list(seq)[:11] == ["self", "tables", "settings", "W", "H", "cameras", "globals_", "post", "supersample", "adaptive", "accumulate"]
    assert list(inspect.signature(translated_objects).parameters) == ["objs", "index", "offsets"]


# ---------------------------------------------------------------- refusals, all without a device
def _scene(blocks, W=32, H=24):
    """Three primitives and two lights, with `blocks` copies of both tables stacked."""
    objs = [h.make_object(abi.RM_SPHERE, model=h.translate(-1, 0, 0)), h.make_object(abi.RM_CUBE, model=h.translate(1, 0, 0)),
            h.make_object(abi.RM_TORUS, model=h.translate(0, 1, 0))]
    lights = [h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (0, -1, -1)), h.make_light(abi.RM_LIGHT_POINT, (1, 1, 1), pos=(0, 3, 3))]
    n = max(blocks, 1)
    cams = (abi.RmCamera * n)(*[h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, W, H) for _ in range(n)])
    globs = (abi.RmGlobals * n)(*[h.make_globals(itime=0.1 * i) for i in range(n)])

    def copies(struct, items):
        arr = (struct * (n * len(items)))()
        for b in range(n):
            for i, it in enumerate(items):
                C.memmove(C.byref(arr[b * len(items) + i]), C.byref(it), C.sizeof(struct))
        return arr
    return cams, globs, copies(abi.RmObject, objs), 3, copies(abi.RmLight, lights), 2


def call(cams, globs, ng, objs, no, not_, lights, nl, nlt, n, sub, W=32, H=24, out=None, s=None, res=None):
    s = s if s is not None else abi.default_settings()
    return lib().rm_render_animated(cams, globs, ng, objs, no, not_, lights, nl, nlt, n, sub, C.byref(s), res, W, H, out, None, None)


def test_table_counts_are_one_or_blocks():
    cams, globs, objs, no, lights, nl = _scene(12)
    for n, sub in ((12, 1), (4, 3), (3, 4), (1, 12)):
        for bad in (0, 2, 5, 13, -1) + ((n,) if sub > 1 and n > 1 else ()):  # numFrames alone is not enough
            assert refused(call(cams, globs, 1, objs, no, bad, lights, nl, 1, n, sub, out=FAKE), "numObjectTables"), (n, sub, bad)
            assert refused(call(cams, globs, 1, objs, no, 12, lights, nl, bad, n, sub, out=FAKE), "numLightTables"), (n, sub, bad)
        # null tables where the count needs them, fine where it does not
        assert refused(call(cams, globs, 1, None, no, 12, lights, nl, 12, n, sub, out=FAKE)), (n, sub)
        assert refused(call(cams, globs, 1, objs, no, 12, None, nl, 12, n, sub, out=FAKE)), (n, sub)
        assert refused(call(cams, globs, 1, None, no, 1, lights, nl, 1, n, sub, out=FAKE)), (n, sub)
        # valid counts get as far as the output pointer
        for not_, nlt in ((1, 1), (12, 1), (1, 12), (12, 12)):
            assert refused(call(cams, globs, 12, objs, no, not_, lights, nl, nlt, n, sub, out=None), "null output"), (n, sub, not_, nlt)
    assert refused(call(cams, globs, 1, None, 0, 12, None, 0, 12, 4, 3, out=None), "null output")  # empty tables need no pointer


def test_everything_rm_render_accumulated_refuses():
    L = lib()
    cams, globs, objs, no, lights, nl = _scene(12)
    for sub in (0, -1, abi.RM_MAX_SUBFRAMES + 1, INT_MAX):
        assert refused(call(cams, globs, 1, objs, no, 1, lights, nl, 1, 1, sub, out=FAKE), "subFrames"), sub
    for n, sub in ((abi.RM_MAX_BATCH_FRAMES + 1, 1), (abi.RM_MAX_BATCH_FRAMES // 64 + 1, 64), (513, 2), (INT_MAX, 64)):
        assert refused(call(cams, globs, 1, objs, no, 1, lights, nl, 1, n, sub, out=FAKE), "RM_MAX_BATCH_FRAMES", want=abi.RM_ERR_CAPACITY), (n, sub)
    for sub in (1, 3, 4):
        n = 12 // sub
        # numFrames == 0: RM_OK whatever the table counts say, nothing is read
        for not_, nlt in ((1, 1), (12, 12), (7, 5)):
            assert call(cams, globs, 1, objs, no, not_, lights, nl, nlt, 0, sub, out=None) == abi.RM_OK, sub
        assert call(None, None, 0, None, 0, 1, None, 0, 1, 0, sub, out=None) == abi.RM_OK, sub
        assert refused(call(cams, globs, 1, objs, no, 12, lights, nl, 12, -1, sub, out=FAKE)), sub
        for ng in (0, 2, 13, -1) + ((n,) if sub > 1 else ()):
            assert refused(call(cams, globs, ng, objs, no, 12, lights, nl, 12, n, sub, out=FAKE), "numGlobals"), (sub, ng)
        assert refused(call(None, globs, 1, objs, no, 12, lights, nl, 12, n, sub, out=FAKE)), sub
        assert refused(call(cams, None, 1, objs, no, 12, lights, nl, 12, n, sub, out=FAKE)), sub
        for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1), (INT_MAX // 8 + 1, 8), (8, 65536 * 8)):
            assert refused(call(cams, globs, 12, objs, no, 12, lights, nl, 12, n, sub, W=W, H=H, out=FAKE)), (sub, W, H)
        many = (abi.RmObject * (abi.RM_MAX_OBJECTS + 1))(*[h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
        assert refused(call(cams, globs, 12, many, abi.RM_MAX_OBJECTS + 1, 1, lights, nl, 12, n, sub, out=FAKE), want=abi.RM_ERR_CAPACITY), sub
        assert refused(L.rm_render_animated(cams, globs, 12, objs, no, 12, lights, nl, 12, n, sub, None, None, 32, 24, FAKE, None, None)), sub
        assert refused(call(cams, globs, 12, objs, no, 12, lights, nl, 12, n, sub, out=None), "null output"), sub


@pytest.mark.parametrize("n,sub", [(12, 1), (4, 3), (2, 6)])
def test_every_block_is_validated_and_the_error_names_it(n, sub):
    """An invalid entry in a table that is not table 0: validate_scene runs per block, ahead of any HIP call."""
    L = lib()
    blocks = n * sub
    # a CUSTOM object in table 5
    cams, globs, objs, no, lights, nl = _scene(blocks)
    objs[5 * no + 1].type = abi.RM_CUSTOM
    assert refused(call(cams, globs, 1, objs, no, blocks, lights, nl, 1, n, sub, out=FAKE), want=abi.RM_ERR_UNSUPPORTED)
    assert "block 5" in L.rm_last_error().decode() and "object 1" in L.rm_last_error().decode()
    # with one shared table the same bytes are never read as table 5
    assert refused(call(cams, globs, 1, objs, no, 1, lights, nl, 1, n, sub, out=None)) and "null output" in L.rm_last_error().decode()
    # a texLoc beyond numTextures in table 3 (one texture supplied, texLoc 1)
    cams, globs, objs, no, lights, nl = _scene(blocks)
    objs[3 * no + 0].texLoc = 1
    px = np.zeros((2, 2, 4), dtype=np.uint8)
    tex = (abi.RmTexture * 1)()
    tex[0].pixels, tex[0].width, tex[0].height = px.ctypes.data, 2, 2
    res = abi.RmResources()
    res.textures, res.numTextures = tex, 1
    assert refused(call(cams, globs, 1, objs, no, blocks, lights, nl, blocks, n, sub, out=FAKE, res=C.byref(res)), want=abi.RM_ERR_UNSUPPORTED)
    assert "block 3" in L.rm_last_error().decode() and "texLoc" in L.rm_last_error().decode()
    # an area light without LTC tables in the last light table only
    cams, globs, objs, no, lights, nl = _scene(blocks)
    lights[(blocks - 1) * nl + 1].type = abi.RM_LIGHT_AREA
    assert refused(call(cams, globs, 1, objs, no, 1, lights, nl, blocks, n, sub, out=FAKE), want=abi.RM_ERR_UNSUPPORTED)
    assert f"block {blocks - 1}" in L.rm_last_error().decode() and "LTC" in L.rm_last_error().decode()
    # an unknown light type in table 1
    cams, globs, objs, no, lights, nl = _scene(blocks)
    lights[1 * nl + 0].type = 77
    assert refused(call(cams, globs, 1, objs, no, blocks, lights, nl, blocks, n, sub, out=FAKE), "block 1", want=abi.RM_ERR_UNSUPPORTED)


# ---------------------------------------------------------------- rm_object_translated
def _translated(o, t):
    out = abi.RmObject()
    st = lib().rm_object_translated(C.byref(o), (C.c_float * 3)(*t), C.byref(out))
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    return out


def _rotated_scaled():
    model = h.translate(0.7, -1.3, 2.1) @ h.rotation((0.3, 1.0, -0.2), 0.9) @ h.scale(1.7, 0.6, 2.3)
    o = h.make_object(abi.RM_CYLINDER, model=model, scale_factor=0.6, ambient=(.1, .2, .3), diffuse=(.4, .5, .6), specular=(.7, .8, .9),
                      shininess=17.0, reflective=(.2, .1, .3), transparent=(.5, .4, .6), ior=1.3)
    o.texLoc, o.repeatU, o.repeatV, o.blend, o.isEmissive, o.lightIdx = 2, 3.0, 4.0, 0.25, 1, 3
    o.color[0], o.color[1], o.color[2] = 0.9, 0.8, 0.7
    return o


@pytest.mark.parametrize("t", [(6.0, 0.0, 0.0), (0.1, -0.2, 0.3), (-17.25, 3.5e-3, 1.0e4), (1e-20, 0.0, -0.0)])
def test_object_translated_is_inv_model_times_t_in_float64_rounded_once(t):
    o = _rotated_scaled()
    got = _translated(o, t)
    M = np.array(o.invModel[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T  # column-major storage
    T = np.eye(4)
    T[:3, 3] = -np.array(t, dtype=np.float32).astype(np.float64)
    want = (M @ T).astype(np.float32).T.reshape(-1)
    assert (np.array(got.invModel[:], dtype=np.float32).view(np.uint32) == want.view(np.uint32)).all()
    # every other field is copied
    a, b = bytearray(bytes(o)), bytearray(bytes(got))
    off = abi.RmObject.invModel.offset
    a[off:off + 64] = b[off:off + 64] = bytes(64)
    assert a == b
    # the object really moved: its world-space centre −A⁻¹b is t further
    def centre(obj):
        m = np.array(obj.invModel[:], dtype=np.float64).reshape(4, 4).T
        return -np.linalg.inv(m[:3, :3]) @ m[:3, 3]
    tt = np.array(t, dtype=np.float32).astype(np.float64)
    assert np.abs(centre(got) - centre(o) - tt).max() <= 1e-5 * max(1.0, np.abs(tt).max())


def test_object_translated_by_zero_is_the_object_and_bad_arguments_are_refused():
    L = lib()
    o = _rotated_scaled()
    o.invModel[12], o.invModel[13] = -0.0, 1e-42  # a signed zero and a denormal in the column that moves
    for t in ((0.0, 0.0, 0.0), (-0.0, 0.0, -0.0)):
        assert bytes(_translated(o, t)) == bytes(o)
    same = _rotated_scaled()  # in place
    assert L.rm_object_translated(C.byref(same), (C.c_float * 3)(1.0, 2.0, 3.0), C.byref(same)) == abi.RM_OK
    assert bytes(same) == bytes(_translated(_rotated_scaled(), (1.0, 2.0, 3.0)))
    out = abi.RmObject()
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(3):
            t = [0.5, 0.5, 0.5]
            t[k] = bad
            assert refused(L.rm_object_translated(C.byref(o), (C.c_float * 3)(*t), C.byref(out))), (bad, k)
    t = (C.c_float * 3)(1, 2, 3)
    assert refused(L.rm_object_translated(None, t, C.byref(out)))
    assert refused(L.rm_object_translated(C.byref(o), None, C.byref(out)))
    assert refused(L.rm_object_translated(C.byref(o), t, None))


# ---------------------------------------------------------------- the Python layer
def test_python_wrappers_check_before_any_device_is_touched():
    from raymarcher_amd import translated_objects
    from raymarcher_amd.render import Renderer, SceneTables
    W, H = 32, 24
    cams_a, globs, objs, no, lights, nl = _scene(1)
    t = SceneTables(cams_a[0], objs, no, lights, nl, globs[0])
    cams = [cams_a[0]] * 6
    r = Renderer.__new__(Renderer)  # no device is touched before the checks
    s = abi.default_settings()
    for sub in (0, -1, 65, 2.0, None, True):
        with pytest.raises(ValueError):
            r.render_animated(t, s, W, H, cams, sub)
    with pytest.raises(ValueError):
        r.render_animated(t, s, W, H, cams, 4)  # 6 cameras are not frames of 4
    stacked = translated_objects(list(objs), 0, [(0.1 * b, 0, 0) for b in range(6)])
    with pytest.raises(ValueError):
        r.render_animated(t, s, W, H, cams[:5], 1, objects=stacked)  # 6 tables for 5 cameras
    with pytest.raises(ValueError):
        r.render_animated(t, s, W, H, cams, 2, lights=[list(lights)] * 5)
    with pytest.raises(ValueError):
        r.render_animated(t, s, W, H, cams, 2, lights=[list(lights)[:1]] * 6)
    for kw in (dict(supersample=2), dict(adaptive=0.1)):
        with pytest.raises(ValueError):
            r.render_sequence(t, s, W, H, cams, objects=stacked, **kw)
    # translated_objects: table b is the table with entry `index` moved by offsets[b] through the C helper
    assert len(stacked) == 6 * no
    for b in range(6):
        assert bytes(stacked[b * no + 0]) == bytes(_translated(objs[0], (0.1 * b, 0, 0)))
        assert bytes(stacked[b * no + 1]) == bytes(objs[1]) and bytes(stacked[b * no + 2]) == bytes(objs[2])
    for bad in (dict(index=3), dict(index=-1), dict(index=1.0), dict(offsets=[]), dict(offsets=[(1, 2)])):
        kw = dict(index=0, offsets=[(0, 0, 0)])
        kw.update(bad)
        with pytest.raises(ValueError):
            translated_objects(list(objs), kw["index"], kw["offsets"])
