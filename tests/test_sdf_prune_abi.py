"""rm_sdf_blocks_select_pruned without a GPU: the header declares it and the library exports it under the unchanged ABI version, the
header's comment carries the definition, the Python layer has its methods, and every refusal returns its status before the first
HIP call — with pointers that would fault if read — in rm_sdf_blocks_select's order, the two constants between iso and maxBlocks."""
import ctypes as C
import inspect
import os
import re

import numpy as np

import helpers as h
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import LIB_PATH, SIGNATURES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "raymarcher_amd.h")).read()
INVALID, CAPACITY, UNSUPPORTED = abi.RM_ERR_INVALID_ARGUMENT, abi.RM_ERR_CAPACITY, abi.RM_ERR_UNSUPPORTED
FAKE = C.c_void_p(0x1000)  # never dereferenced: every call that gets it fails its checks first
inf, nan = float("inf"), float("nan")
NAME = "rm_sdf_blocks_select_pruned"


def test_header_declares_and_library_exports_the_symbol():
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^)]*)\)", body)
    assert m, f"include/raymarcher_amd.h does not declare {NAME}"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["const RmObject *objs", "int numObjects", "const RmGlobals *g", "const RmSettings *s", "const float origin[3]",
                      "const float step[3]", "int mx", "int my", "int mz", "float iso", "float lipschitzOut", "float lipschitzIn",
                      "int maxBlocks", "int32_t *d_blocks", "uint32_t *d_count", "void *stream"]
    assert body.index("int rm_sdf_blocks_select(") < body.index("int " + NAME + "(") < body.index("int rm_sdf_grid_blocks(")
    assert "uint32_t *d_count /* 2 words */" in HEADER
    lib()
    assert hasattr(C.CDLL(LIB_PATH), NAME), f"the library does not export {NAME}"
    assert NAME in SIGNATURES and SIGNATURES[NAME][0] is C.c_int and len(SIGNATURES[NAME][1]) == 16
    floats = [n for n, ty in enumerate(SIGNATURES[NAME][1]) if ty is C.c_float]
    assert floats == [9, 10, 11]


def test_abi_version_stays_and_the_header_carries_the_definition():
    assert abi.RM_ABI_VERSION == 5 and lib().rm_abi_version() == 5
    assert re.search(r"#define\s+RM_ABI_VERSION\s+5\b", HEADER)
    assert abi.RM_PATH_SDF_BLOCKS_SELECT_PRUNED == 20
    assert re.search(r"19 = a launch of rm_sdf_grid_blocks,\s*\*?\s*20 = a launch of rm_sdf_blocks_select_pruned", HEADER)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int " + NAME + r"\b", HEADER, flags=re.S)
    assert m, f"no comment in front of {NAME}"
    text = re.sub(r"\s*\n\s*\*\s?", " ", m.group(1))
    for w in ("lattice point (8i, 8j, 8k)", "h = 4 · sqrt((sx·sx + sy·sy) + sz·sz)", "correctly rounded", "computed on the host",
              "bOut = lipschitzOut · h", "bIn = lipschitzIn · h", "a NaN bound (0 · inf) discards nothing", "d = c − iso", "farOut = d > bOut",
              "farIn = d < −bIn", "a NaN c is neither", "DISCARDED iff farOut holds at all eight", "CANDIDATE", "(bk·my + bj)·mx + bi",
              "FULL number", "the counting call", "d_count[1] receives the number of candidates, saturated at 2^32 − 1",
              "sub-sequence of rm_sdf_blocks_select's list", "With both constants +INFINITY the two lists and d_count[0] are equal in every word",
              "v(p) ≥ v(q) − lipschitzOut·|p − q|", "A true distance function honours this with 1", "lipschitzIn = +INFINITY",
              "before any HIP call", "NaN or below 0", "+INFINITY and 0 are valid", "rm_debug_last_path() = 20", "counts as one launch",
              "4 B per corner + 8 B per block", "at most 12 B per block", "rm_set_workspace_limit", "rm_release_workspaces",
              "no host synchronisation", "does not depend on its wave", "length they read from device memory", "RM_ABI_VERSION"):
        assert w in text, f"the comment of {NAME} lacks: {w}"


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    default = lambda f, p: inspect.signature(f).parameters[p].default  # noqa: E731
    assert sig(Renderer.sdf_active_blocks_pruned) == sig(Renderer.sdf_active_blocks) + ["outside", "inside"]
    assert sig(Renderer.scene_mesh_pruned) == sig(Renderer.scene_mesh_sparse) + ["outside", "inside"]
    assert sig(Renderer.bake_mesh_pruned) == sig(Renderer.bake_mesh_sparse) + ["outside", "inside"]
    assert sig(Renderer.scene_field_pruned) == sig(Renderer.scene_field_sparse) + ["outside", "inside"]
    # outside: twice the smallest value of the measured ladder that lost no block of the headline bulb at 4097 points per axis (1
    # lost 16 there, 2 none: profiles/sdf_prune.md); inside: None, +inf — the fractals' interior honours no constant
    for f in (Renderer.sdf_active_blocks_pruned, Renderer.scene_mesh_pruned, Renderer.bake_mesh_pruned, Renderer.scene_field_pruned):
        assert default(f, "outside") == 4.0 and default(f, "inside") is None, f
    for f in (Renderer.scene_mesh_pruned, Renderer.bake_mesh_pruned, Renderer.scene_field_pruned):
        assert default(f, "iso") == 0.001 and default(f, "bounds") is None
    # the existing methods are as they were
    assert sig(Renderer.sdf_active_blocks) == ["self", "tables", "settings", "origin", "step", "blocks", "iso"]
    assert sig(Renderer.scene_field_sparse) == ["self", "tables", "settings", "resolution", "iso", "bounds"]


def refused(status, want=INVALID, text=None):
    msg = lib().rm_last_error().decode()
    return status == want and len(msg) > 0 and (text is None or text in msg)


def vec(*v):
    return (C.c_float * 3)(*v)


def _scene():
    objs, no = h.table([h.make_object(abi.RM_SPHERE, model=h.translate(-1, 0, 0)), h.make_object(abi.RM_CUBE, model=h.translate(1, 0, 0)),
                        h.make_object(abi.RM_TORUS)])
    return objs, no, h.make_globals()


def pruned(objs, no, g, s="default", origin=(0, 0, 0), step=(0.1, 0.1, 0.1), blocks=(2, 2, 2), iso=0.0, l_out=1.0, l_in=inf, max_blocks=8,
           out=FAKE, count=FAKE):
    s = abi.default_settings() if s == "default" else s
    return lib().rm_sdf_blocks_select_pruned(objs, no, C.byref(g) if g is not None else None, C.byref(s) if s is not None else None,
                                             vec(*origin) if origin is not None else None, vec(*step) if step is not None else None,
                                             blocks[0], blocks[1], blocks[2], iso, l_out, l_in, max_blocks, out, count, None)


BAD_STEPS = ((nan, 1, 1), (1, inf, 1), (1, 1, 0.0), (-0.5, 1, 1), (1, -0.0, 1), (1, 1, -inf))
BAD_ORIGINS = ((nan, 0, 0), (0, inf, 0), (0, 0, -inf))
BAD_BLOCKS = ((0, 2, 2), (2, -1, 2), (2, 2, 0), (513, 1, 1), (1, 513, 1), (1, 1, 2 ** 31 - 1), (-2 ** 31, 2, 2))
BIG_BLOCKS = ((512, 512, 512), (1, 1, 1), (512, 1, 1), (1, 1, 512))
BAD_CONSTANTS = (nan, -0.5, -inf)


def test_refusals_in_rm_sdf_blocks_selects_order():
    objs, no, g = _scene()
    assert refused(pruned(objs, no, None), text="null g, s, origin or step")
    assert refused(pruned(objs, no, g, s=None), text="null g, s, origin or step")
    assert refused(pruned(objs, no, g, origin=None), text="null g, s, origin or step")
    assert refused(pruned(objs, no, g, step=None), text="null g, s, origin or step")
    assert refused(pruned(None, no, g), text="null object table")
    assert refused(pruned(objs, -1, g), text="null object table")
    assert refused(pruned(None, no, None), text="null g, s")  # the pointers come before the table
    for o in BAD_ORIGINS:
        assert refused(pruned(objs, no, g, origin=o), text="origin must be finite"), o
        assert refused(pruned(None, no, g, origin=o), text="null object table"), o  # the table comes before the lattice
    for st in BAD_STEPS:
        assert refused(pruned(objs, no, g, step=st), text="step must be finite and greater than 0"), st
        assert refused(pruned(objs, no, g, origin=(nan, 0, 0), step=st), text="origin"), st
    for b in BAD_BLOCKS:
        assert refused(pruned(objs, no, g, blocks=b), text="block dimension"), b
        assert refused(pruned(objs, no, g, step=(0, 1, 1), blocks=b), text="step"), b
    for b in BIG_BLOCKS:  # no INT_MAX rule: these get as far as the outputs
        assert refused(pruned(objs, no, g, blocks=b, count=None), text="null d_count"), b
    for iso in (nan, inf, -inf):
        assert refused(pruned(objs, no, g, iso=iso), text="iso must be finite"), iso
        assert refused(pruned(objs, no, g, iso=iso, blocks=(0, 1, 1)), text="block dimension"), iso  # the lattice comes before iso
        assert refused(pruned(objs, no, g, iso=iso, l_out=nan), text="iso"), iso                     # iso before the constants
        assert refused(pruned(objs, no, g, iso=iso, max_blocks=-1), text="iso"), iso
    for bad in BAD_CONSTANTS:
        for kw in (dict(l_out=bad), dict(l_in=bad), dict(l_out=bad, l_in=bad)):
            assert refused(pruned(objs, no, g, **kw), text="lipschitzOut and lipschitzIn must not be NaN or negative"), kw
            assert refused(pruned(objs, no, g, max_blocks=-1, **kw), text="lipschitz"), kw             # the constants before maxBlocks
            assert refused(pruned(objs, no, g, blocks=(0, 1, 1), **kw), text="block dimension"), kw  # the lattice before the constants
            assert refused(pruned(objs, no, g, s=abi.default_settings(features=abi.RM_FEAT_SEA), **kw), text="lipschitz"), kw  # before the layers
    # +inf, 0 and −0 are valid constants: these get as far as the outputs
    for l_out, l_in in ((inf, inf), (0.0, 0.0), (-0.0, inf), (inf, 0.0), (1e-45, 3e38)):
        assert refused(pruned(objs, no, g, l_out=l_out, l_in=l_in, count=None), text="null d_count"), (l_out, l_in)
    assert refused(pruned(objs, no, g, max_blocks=-1), text="negative maxBlocks")
    assert refused(pruned(objs, no, g, max_blocks=-2 ** 31, out=None), text="negative maxBlocks")
    # maxBlocks comes before the layers, the layers before the 2-D mode, that before the table, the table before the outputs
    assert refused(pruned(objs, no, g, max_blocks=-1, s=abi.default_settings(features=abi.RM_FEAT_SEA)), text="negative maxBlocks")
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_SEA | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(pruned(objs, no, g, s=abi.default_settings(features=feat)), UNSUPPORTED, "TERRAIN / CLOUD / SEA"), feat
        assert refused(pruned(objs, no, h.make_globals(two_d=1), s=abi.default_settings(features=feat)), UNSUPPORTED, "TERRAIN"), feat
        assert refused(pruned(objs, no, g, out=None, s=abi.default_settings(features=feat)), UNSUPPORTED, "TERRAIN / CLOUD / SEA"), feat
    assert refused(pruned(objs, no, h.make_globals(two_d=1)), UNSUPPORTED, "isTwoD")
    many, nm = h.table([h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(pruned(many, nm, g), CAPACITY, "RM_MAX_OBJECTS")
    assert refused(pruned(many, nm, h.make_globals(two_d=1)), UNSUPPORTED, "isTwoD")
    assert refused(pruned(many, nm, g, count=None), CAPACITY, "RM_MAX_OBJECTS")
    assert refused(pruned(many, abi.RM_MAX_OBJECTS, g, count=None), text="null d_count")
    for field in ("fractalIters", "mengerLevels", "maxSteps"):
        assert refused(pruned(objs, no, g, s=abi.default_settings(**{field: -1})), text="loop bound"), field
    objs[1].type = abi.RM_CUSTOM
    assert refused(pruned(objs, no, g), UNSUPPORTED, "object 1") and "CUSTOM" in lib().rm_last_error().decode()
    objs[1].type = abi.RM_CUBE
    assert refused(pruned(None, 0, g, count=None), text="null d_count")  # an empty table needs no pointer
    assert refused(pruned(objs, no, g, out=None), text="null d_blocks with maxBlocks above 0")
    assert refused(pruned(objs, no, g, count=None), text="null d_count")
    # the counting call takes a null list: it gets as far as the device-memory check of a count that is host memory
    host = np.zeros(64, dtype=np.int32)
    hp = C.c_void_p(host.ctypes.data)
    assert refused(pruned(objs, no, g, max_blocks=0, out=None, count=hp), text="d_count is not device-accessible")
    assert refused(pruned(objs, no, g, out=hp, count=hp), text="d_blocks is not device-accessible")
