"""rm_sdf_blocks_select_pruned without a GPU: the header declares it and the library exports it under the unchanged ABI version, the
header's comment carries the definition, the Python layer has its methods, and every refusal returns its status before the first
HIP call — with pointers that would fault if read — in rm_sdf_blocks_select's order, the two constants between iso and maxBlocks."""
import ctypes as C
import inspect
import re

import abi_helpers as ah
import helpers as h
import scene_builders as SB
from abi_helpers import BAD_BLOCKS, BAD_ORIGINS, BAD_STEPS, BIG_BLOCKS, CAPACITY, FAKE, HEADER, HP, inf, nan, refused, vec3
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES

UNSUPPORTED = abi.RM_ERR_UNSUPPORTED
NAME = "rm_sdf_blocks_select_pruned"


def test_header_declares_and_library_exports_the_symbol():
    body = ah.HEADER_CODE
    assert ah.params(NAME) == [
        "const RmObject *objs", "int numObjects", "const RmGlobals *g", "const RmSettings *s", "const float origin[3]",
        "const float step[3]", "int mx", "int my", "int mz", "float iso", "float lipschitzOut", "float lipschitzIn",
        "int maxBlocks", "int32_t *d_blocks", "uint32_t *d_count", "void *stream"]
    assert body.index("int rm_sdf_blocks_select(") < body.index("int " + NAME + "(") < body.index("int rm_sdf_grid_blocks(")
    assert "uint32_t *d_count /* 2 words */" in HEADER
    ah.assert_exported([NAME])
    assert NAME in SIGNATURES and SIGNATURES[NAME][0] is C.c_int and len(SIGNATURES[NAME][1]) == 16
    floats = [n for n, ty in enumerate(SIGNATURES[NAME][1]) if ty is C.c_float]
    assert floats == [9, 10, 11]


def test_abi_version_stays_and_the_header_carries_the_definition():
    ah.assert_abi_version()
    assert abi.RM_PATH_SDF_BLOCKS_SELECT_PRUNED == 20
    assert re.search(r"19 = a launch of rm_sdf_grid_blocks,\s*\*?\s*20 = a launch of rm_sdf_blocks_select_pruned", HEADER)
    ah.assert_comment_has(NAME, (
        "lattice point (8i, 8j, 8k)", "h = 4 · sqrt((sx·sx + sy·sy) + sz·sz)", "correctly rounded", "computed on the host",
        "bOut = lipschitzOut · h", "bIn = lipschitzIn · h", "a NaN bound (0 · inf) discards nothing", "d = c − iso", "farOut = d > bOut",
        "farIn = d < −bIn", "a NaN c is neither", "DISCARDED iff farOut holds at all eight", "CANDIDATE", "(bk·my + bj)·mx + bi",
        "FULL number", "the counting call", "d_count[1] receives the number of candidates, saturated at 2^32 − 1",
        "sub-sequence of rm_sdf_blocks_select's list", "With both constants +INFINITY the two lists and d_count[0] are equal in every word",
        "v(p) ≥ v(q) − lipschitzOut·|p − q|", "A true distance function honours this with 1", "lipschitzIn = +INFINITY",
        "before any HIP call", "NaN or below 0", "+INFINITY and 0 are valid", "rm_debug_last_path() = 20", "counts as one launch",
        "4 B per corner + 8 B per block", "at most 12 B per block", "rm_set_workspace_limit", "rm_release_workspaces",
        "no host synchronisation", "does not depend on its wave", "length they read from device memory", "RM_ABI_VERSION"))


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


def pruned(objs, no, g, s="default", origin=(0, 0, 0), step=(0.1, 0.1, 0.1), blocks=(2, 2, 2), iso=0.0, l_out=1.0, l_in=inf, max_blocks=8,
           out=FAKE, count=FAKE):
    s = abi.default_settings() if s == "default" else s
    return lib().rm_sdf_blocks_select_pruned(objs, no, C.byref(g) if g is not None else None, C.byref(s) if s is not None else None,
                                             vec3(origin), vec3(step), blocks[0], blocks[1], blocks[2], iso, l_out, l_in, max_blocks, out, count, None)


BAD_CONSTANTS = (nan, -0.5, -inf)


def test_refusals_in_rm_sdf_blocks_selects_order():
    objs, no, g = SB.three_primitives_table()
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
        assert refused(pruned(objs, no, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
        assert refused(pruned(objs, no, h.make_globals(two_d=1), s=abi.default_settings(features=feat)), "TERRAIN", want=UNSUPPORTED), feat
        assert refused(pruned(objs, no, g, out=None, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
    assert refused(pruned(objs, no, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    many, nm = h.table([h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(pruned(many, nm, g), "RM_MAX_OBJECTS", want=CAPACITY)
    assert refused(pruned(many, nm, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    assert refused(pruned(many, nm, g, count=None), "RM_MAX_OBJECTS", want=CAPACITY)
    assert refused(pruned(many, abi.RM_MAX_OBJECTS, g, count=None), text="null d_count")
    for field in ("fractalIters", "mengerLevels", "maxSteps"):
        assert refused(pruned(objs, no, g, s=abi.default_settings(**{field: -1})), text="loop bound"), field
    objs[1].type = abi.RM_CUSTOM
    assert refused(pruned(objs, no, g), "object 1", want=UNSUPPORTED) and "CUSTOM" in lib().rm_last_error().decode()
    objs[1].type = abi.RM_CUBE
    assert refused(pruned(None, 0, g, count=None), text="null d_count")  # an empty table needs no pointer
    assert refused(pruned(objs, no, g, out=None), text="null d_blocks with maxBlocks above 0")
    assert refused(pruned(objs, no, g, count=None), text="null d_count")
    # the counting call takes a null list: it gets as far as the device-memory check of a count that is host memory
    assert refused(pruned(objs, no, g, max_blocks=0, out=None, count=HP), text="d_count is not device-accessible")
    assert refused(pruned(objs, no, g, out=HP, count=HP), text="d_blocks is not device-accessible")
