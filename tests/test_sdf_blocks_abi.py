"""rm_sdf_blocks_select, rm_sdf_grid_blocks and rm_sdf_mesh_blocks without a GPU: the header declares them and the library exports
them under the unchanged ABI version, the Python layer has its methods, and every refusal returns its status before the first HIP
call — with pointers that would fault if read — in the order the header states."""
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
NAMES = ("rm_sdf_blocks_select", "rm_sdf_grid_blocks", "rm_sdf_mesh_blocks")


SCENE = ["const RmObject *objs", "int numObjects", "const RmGlobals *g", "const RmSettings *s", "const float origin[3]", "const float step[3]",
         "int mx", "int my", "int mz"]


def test_header_declares_and_library_exports_the_three_symbols():
    assert ah.params("rm_sdf_blocks_select") == SCENE + ["float iso", "int maxBlocks", "int32_t *d_blocks", "uint32_t *d_count", "void *stream"]
    assert ah.params("rm_sdf_grid_blocks") == SCENE + ["const int32_t *d_blocks", "int numBlocks", "float *d_dist", "int32_t *d_objectId",
                                                     "void *stream"]
    assert ah.params("rm_sdf_mesh_blocks") == [
        "const float *d_dist", "const int32_t *d_objectId", "const int32_t *d_blocks", "int numBlocks",
        "int mx", "int my", "int mz", "const float origin[3]", "const float step[3]", "float iso",
        "int maxVertices", "int maxQuads", "float *d_vertices", "int32_t *d_vertexObject",
        "int32_t *d_quads", "uint32_t *d_counts", "void *stream"]
    ah.assert_exported(NAMES)
    for name, n in zip(NAMES, (14, 14, 17)):
        assert name in SIGNATURES and SIGNATURES[name][0] is C.c_int and len(SIGNATURES[name][1]) == n


def test_abi_version_stays_and_the_header_carries_the_definitions():
    ah.assert_abi_version()
    assert re.search(r"#define\s+RM_MAX_LATTICE_BLOCKS\s+512\b", HEADER) and abi.RM_MAX_LATTICE_BLOCKS == 512
    assert re.search(r"#define\s+RM_MAX_BLOCK_LIST\s+\(1 << 22\)", HEADER) and abi.RM_MAX_BLOCK_LIST == 1 << 22
    assert (abi.RM_PATH_SDF_BLOCKS_SELECT, abi.RM_PATH_SDF_GRID_BLOCKS) == (18, 19)
    assert re.search(r"18 = a launch of rm_sdf_blocks_select,\s*\*?\s*19 = a launch of rm_sdf_grid_blocks", HEADER)
    words = {"rm_sdf_blocks_select": ("not the same for all 729", "one of its 512 cells is active in rm_sdf_mesh's sense", "(bk·my + bj)·mx + bi",
                                      "FULL number", "the counting call", "before any HIP call", "rm_debug_last_path() = 18",
                                      "rm_set_workspace_limit", "leaves before the evaluation"),
             "rm_sdf_grid_blocks": ("(c·9 + b)·9 + a", "the bits rm_sdf_grid stores", "A void entry's slot is not written", "numBlocks = 0: RM_OK",
                                    "rm_debug_last_path() = 19", "before any HIP call"),
             "rm_sdf_mesh_blocks": ("GLOBAL cell index", "(c·8 + b)·8 + a", "that cell's block owns the edge", "OPEN vertices",
                                    "stored vertex numbers stay below d_counts[0]", "before any HIP call", "88 B per list entry")}
    for name, ws in words.items():
        ah.assert_comment_has(name, ws)
    assert "of equal entries the first counts" in re.sub(r"\s*\n\s*\*\s?", " ", HEADER)


def test_python_signatures():
    from raymarcher_amd.render import Renderer
    sig = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert sig(Renderer.sdf_active_blocks) == ["self", "tables", "settings", "origin", "step", "blocks", "iso"]
    assert sig(Renderer.sdf_grid_blocks) == ["self", "tables", "settings", "origin", "step", "blocks", "block_list", "ids"]
    assert inspect.signature(Renderer.sdf_grid_blocks).parameters["ids"].default is False
    assert sig(Renderer.extract_mesh_blocks) == ["self", "grid_blocks", "block_list", "blocks", "origin", "step", "iso", "ids"]
    assert inspect.signature(Renderer.extract_mesh_blocks).parameters["iso"].default == 0.0
    assert sig(Renderer.scene_mesh_sparse) == sig(Renderer.scene_mesh)
    assert inspect.signature(Renderer.scene_mesh_sparse).parameters["iso"].default == 0.001
    assert sig(Renderer.bake_mesh_sparse) == sig(Renderer.bake_mesh)


def _head(objs, no, g, s, origin, step, blocks):
    s = abi.default_settings() if s == "default" else s
    return (objs, no, C.byref(g) if g is not None else None, C.byref(s) if s is not None else None,
            vec3(origin), vec3(step), blocks[0], blocks[1], blocks[2])


def select(objs, no, g, s="default", origin=(0, 0, 0), step=(0.1, 0.1, 0.1), blocks=(2, 2, 2), iso=0.0, max_blocks=8, out=FAKE, count=FAKE):
    return lib().rm_sdf_blocks_select(*_head(objs, no, g, s, origin, step, blocks), iso, max_blocks, out, count, None)


def grid(objs, no, g, s="default", origin=(0, 0, 0), step=(0.1, 0.1, 0.1), blocks=(2, 2, 2), bl=FAKE, n=3, dist=FAKE, ids=FAKE):
    return lib().rm_sdf_grid_blocks(*_head(objs, no, g, s, origin, step, blocks), bl, n, dist, ids, None)


def _shared_refusals(call, null_output):
    """What the two staged entry points refuse alike, in order; null_output: keyword arguments that get a call past everything but
    its outputs, and the text of that refusal."""
    objs, no, g = SB.three_primitives_table()
    kw, text = null_output
    assert refused(call(objs, no, None), text="null g, s, origin or step")
    assert refused(call(objs, no, g, s=None), text="null g, s, origin or step")
    assert refused(call(objs, no, g, origin=None), text="null g, s, origin or step")
    assert refused(call(objs, no, g, step=None), text="null g, s, origin or step")
    assert refused(call(None, no, g), text="null object table")
    assert refused(call(objs, -1, g), text="null object table")
    assert refused(call(None, no, None), text="null g, s")  # the pointers come before the table
    for o in BAD_ORIGINS:
        assert refused(call(objs, no, g, origin=o), text="origin must be finite"), o
        assert refused(call(None, no, g, origin=o), text="null object table"), o  # the table comes before the lattice
    for st in BAD_STEPS:
        assert refused(call(objs, no, g, step=st), text="step must be finite and greater than 0"), st
        assert refused(call(objs, no, g, origin=(nan, 0, 0), step=st), text="origin"), st
    for b in BAD_BLOCKS:
        assert refused(call(objs, no, g, blocks=b), text="block dimension"), b
        assert refused(call(objs, no, g, step=(0, 1, 1), blocks=b), text="step"), b
    for b in BIG_BLOCKS:  # no INT_MAX rule: these get as far as the outputs
        assert refused(call(objs, no, g, blocks=b, **kw), text=text), b
    for feat in (abi.RM_FEAT_TERRAIN, abi.RM_FEAT_CLOUD, abi.RM_FEAT_SEA, abi.RM_FEAT_SEA | abi.RM_FEAT_PERLIN_BUMP):
        assert refused(call(objs, no, g, s=abi.default_settings(features=feat)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED), feat
        assert refused(call(objs, no, g, s=abi.default_settings(features=feat), blocks=(0, 1, 1)), text="block dimension"), feat
        assert refused(call(objs, no, h.make_globals(two_d=1), s=abi.default_settings(features=feat)), "TERRAIN", want=UNSUPPORTED), feat
    assert refused(call(objs, no, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)
    many, nm = h.table([h.make_object(abi.RM_SPHERE) for _ in range(abi.RM_MAX_OBJECTS + 1)])
    assert refused(call(many, nm, g), "RM_MAX_OBJECTS", want=CAPACITY)
    assert refused(call(many, nm, h.make_globals(two_d=1)), "isTwoD", want=UNSUPPORTED)  # the 2-D mode comes before the table
    assert refused(call(many, nm, g, **kw), "RM_MAX_OBJECTS", want=CAPACITY)              # and the table before the outputs
    assert refused(call(many, abi.RM_MAX_OBJECTS, g, **kw), text=text)
    for field in ("fractalIters", "mengerLevels", "maxSteps"):
        assert refused(call(objs, no, g, s=abi.default_settings(**{field: -1})), text="loop bound"), field
    objs[1].type = abi.RM_CUSTOM
    assert refused(call(objs, no, g), "object 1", want=UNSUPPORTED) and "CUSTOM" in lib().rm_last_error().decode()
    objs[1].type = 99
    assert refused(call(objs, no, g, **kw), "object 1", want=UNSUPPORTED)
    objs[1].type = abi.RM_CUBE
    assert refused(call(objs, no, g, **kw), text=text)
    assert refused(call(None, 0, g, **kw), text=text)  # an empty table needs no pointer


def test_select_refusals_in_order():
    _shared_refusals(select, (dict(count=None), "null d_count"))
    objs, no, g = SB.three_primitives_table()
    for iso in (nan, inf, -inf):
        assert refused(select(objs, no, g, iso=iso), text="iso must be finite"), iso
        assert refused(select(objs, no, g, iso=iso, blocks=(0, 1, 1)), text="block dimension"), iso  # the lattice comes before iso
        assert refused(select(objs, no, g, iso=iso, max_blocks=-1), text="iso"), iso                 # iso before maxBlocks
    assert refused(select(objs, no, g, max_blocks=-1), text="negative maxBlocks")
    assert refused(select(objs, no, g, max_blocks=-2 ** 31, out=None), text="negative maxBlocks")
    # maxBlocks comes before the layers, the layers before the outputs
    assert refused(select(objs, no, g, max_blocks=-1, s=abi.default_settings(features=abi.RM_FEAT_SEA)), text="negative maxBlocks")
    assert refused(select(objs, no, g, out=None, s=abi.default_settings(features=abi.RM_FEAT_SEA)), "TERRAIN / CLOUD / SEA", want=UNSUPPORTED)
    assert refused(select(objs, no, g, out=None), text="null d_blocks with maxBlocks above 0")
    assert refused(select(objs, no, g, count=None), text="null d_count")
    # the counting call takes a null list: it gets as far as the device-memory check of a count that is host memory
    assert refused(select(objs, no, g, max_blocks=0, out=None, count=HP), text="d_count is not device-accessible")
    assert refused(select(objs, no, g, out=HP, count=HP), text="d_blocks is not device-accessible")


def test_grid_blocks_refusals_in_order_and_the_empty_list():
    _shared_refusals(grid, (dict(dist=None), "null d_blocks or d_dist"))
    objs, no, g = SB.three_primitives_table()
    for n in (-1, -2 ** 31, (1 << 22) + 1, 2 ** 31 - 1):
        assert refused(grid(objs, no, g, n=n), text="numBlocks must be 0 … RM_MAX_BLOCK_LIST"), n
        assert refused(grid(objs, no, g, n=n, blocks=(0, 1, 1)), text="block dimension"), n  # the lattice comes before numBlocks
        assert refused(grid(objs, no, g, n=n, s=abi.default_settings(features=abi.RM_FEAT_SEA)), text="numBlocks"), n  # numBlocks before the layers
    assert refused(grid(objs, no, g, n=1 << 22, bl=None), text="null d_blocks or d_dist")  # the longest list is a list
    assert refused(grid(objs, no, g, bl=None), text="null d_blocks or d_dist")
    assert refused(grid(objs, no, g, dist=None), text="null d_blocks or d_dist")
    # an empty list: RM_OK with nothing read, but only for a call that is otherwise in order
    assert grid(objs, no, g, n=0, bl=None, dist=None, ids=None) == abi.RM_OK
    assert grid(objs, no, g, n=0) == abi.RM_OK
    assert refused(grid(objs, no, g, n=0, blocks=(0, 1, 1)), text="block dimension")
    assert refused(grid(objs, no, h.make_globals(two_d=1), n=0), "isTwoD", want=UNSUPPORTED)
    assert refused(grid(objs, no, g, bl=HP, ids=None), text="d_blocks is not device-accessible")


def mesh(blocks=(2, 2, 2), origin=(0, 0, 0), step=(0.1, 0.1, 0.1), iso=0.0, n=3, max_v=10, max_q=10, dist=FAKE, ids=FAKE, bl=FAKE, verts=FAKE,
         vobj=FAKE, quads=FAKE, counts=FAKE):
    return lib().rm_sdf_mesh_blocks(dist, ids, bl, n, blocks[0], blocks[1], blocks[2], vec3(origin), vec3(step), iso, max_v, max_q, verts,
                                    vobj, quads, counts, None)


def test_mesh_blocks_refusals_in_order():
    assert refused(mesh(origin=None), text="null origin or step")
    assert refused(mesh(step=None), text="null origin or step")
    for o in BAD_ORIGINS:
        assert refused(mesh(origin=o), text="origin must be finite"), o
    for st in BAD_STEPS:
        assert refused(mesh(step=st), text="step must be finite and greater than 0"), st
        assert refused(mesh(origin=(0, nan, 0), step=st), text="origin"), st
    for b in BAD_BLOCKS:
        assert refused(mesh(blocks=b), text="block dimension"), b
        assert refused(mesh(blocks=b, step=(1, 1, nan)), text="step"), b
    for iso in (nan, inf, -inf):
        assert refused(mesh(iso=iso), text="iso must be finite"), iso
        assert refused(mesh(iso=iso, blocks=(0, 1, 1)), text="block dimension"), iso  # the lattice comes before iso
        assert refused(mesh(iso=iso, n=-1), text="iso"), iso                          # iso before numBlocks
    for n in (-1, (1 << 22) + 1, 2 ** 31 - 1):
        assert refused(mesh(n=n), text="numBlocks must be 0 … RM_MAX_BLOCK_LIST"), n
        assert refused(mesh(n=n, max_v=-1), text="numBlocks"), n                      # numBlocks before the capacities
    assert refused(mesh(max_v=-1), text="negative capacity")
    assert refused(mesh(max_q=-5), text="negative capacity")
    assert refused(mesh(max_q=-2 ** 31, verts=None), text="negative capacity")        # the capacities before the outputs
    assert refused(mesh(verts=None), text="null d_vertices or d_quads")
    assert refused(mesh(quads=None), text="null d_vertices or d_quads")
    assert refused(mesh(verts=None, dist=None), text="null d_vertices or d_quads")     # the outputs before the inputs and d_counts
    assert refused(mesh(dist=None), text="null d_dist, d_blocks or d_counts")
    assert refused(mesh(bl=None), text="null d_dist, d_blocks or d_counts")
    assert refused(mesh(counts=None), text="null d_dist, d_blocks or d_counts")
    assert refused(mesh(n=0, dist=None, bl=None, counts=None), text="null d_dist, d_blocks or d_counts")  # an empty list still has counts
    for b in BIG_BLOCKS:
        assert refused(mesh(blocks=b, n=1 << 22, counts=None), text="null d_dist, d_blocks or d_counts"), b
    # the counting call takes null outputs, d_vertexObject and d_objectId may be null, an empty list needs neither d_dist nor
    # d_blocks: each of these gets as far as the device-memory check of an array that is host memory
    assert refused(mesh(max_v=0, max_q=0, verts=None, vobj=None, quads=None, ids=None, dist=HP), text="d_dist is not device-accessible")
    assert refused(mesh(max_q=0, quads=None, dist=HP), text="d_dist is not device-accessible")
    assert refused(mesh(n=0, dist=None, bl=None, ids=None, max_v=0, max_q=0, verts=None, vobj=None, quads=None, counts=HP),
                   text="d_counts is not device-accessible")
