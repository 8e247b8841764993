"""tests/abi_helpers.py on small literal headers, not on the real one: what the parser returns for a declaration with array
parameters and line breaks, for a comment with #define lines behind it and for a typedef's comment, how it fails for a name that
is not declared, and the three conditions of refused() against a stubbed status and message."""
import pytest

import abi_helpers as ah

HEADER = """
/* The version. */
#define RM_ABI_VERSION 5

/* An earlier entry point: not the comment of rm_bake. */
int rm_first(void);

/* Bakes the lattice.
 * origin and step: three floats each,
 *   read on the host before any HIP call.
 */
#define RM_MAX_BAKE 4096
#define RM_BAKE_TILE (1 << 3)
int rm_bake(const float *d_dist,   const int32_t *d_objectId,
            const float origin[3], const float step[3],
            int nx, RmBake **out /* one handle */, void *stream);

/* A sample of the lattice:
 * the value, then the cell. */
typedef struct RmBakeSample { float value; int32_t cell[3]; } RmBakeSample; /* 16 bytes */

/* An opaque handle. */
typedef struct RmBake RmBake;
void rm_bake_destroy(RmBake *bake);
"""
CODE = ah.strip_comments(HEADER)


def test_params_keep_arrays_and_squeeze_line_breaks():
    assert "one handle" not in CODE and "Bakes" not in CODE
    assert ah.params("rm_bake", code=CODE) == ["const float *d_dist", "const int32_t *d_objectId", "const float origin[3]",
                                               "const float step[3]", "int nx", "RmBake **out", "void *stream"]
    assert ah.params("rm_first", code=CODE) == ["void"]
    assert ah.params("rm_bake_destroy", "void", code=CODE) == ["RmBake *bake"]
    assert ah.declared_functions(CODE) == ["rm_bake", "rm_bake_destroy", "rm_first"]


def test_an_undeclared_name_or_another_return_type_asserts_with_the_header_named():
    for name, returns in (("rm_missing", "int"), ("rm_bak", "int"), ("rm_bake_destroy", "int"), ("rm_bake", "void")):
        with pytest.raises(AssertionError) as e:
            ah.params(name, returns, code=CODE)
        assert str(e.value).startswith(f"include/raymarcher_amd.h does not declare {name}")


def test_comment_before_a_declaration_skips_define_lines_and_joins_the_lines():
    text = ah.comment_before("rm_bake", HEADER)
    # every "newline, blanks, star" is one blank; the newline in front of a closing */ on a line of its own stays
    assert text == " Bakes the lattice. origin and step: three floats each,   read on the host before any HIP call.\n "
    ah.assert_comment_has("rm_bake", ("three floats each,   read on the host", "before any HIP call"), HEADER)
    assert ah.comment_before("rm_first", HEADER) == " An earlier entry point: not the comment of rm_bake. "
    with pytest.raises(AssertionError) as e:
        ah.assert_comment_has("rm_bake", ("Bakes the lattice", "an earlier entry point"), HEADER)
    assert str(e.value).startswith("the comment of rm_bake lacks: an earlier entry point")
    # a declaration with another declaration between it and the nearest comment has no comment of its own
    with pytest.raises(AssertionError) as e:
        ah.comment_before("rm_bake_destroy", HEADER)
    assert str(e.value).startswith("no comment in front of rm_bake_destroy")


def test_comment_before_a_typedef_struct():
    assert ah.comment_before("RmBakeSample", HEADER) == " A sample of the lattice: the value, then the cell. "
    assert ah.comment_before("RmBake", HEADER) == " An opaque handle. "  # the whole name: not RmBakeSample's
    assert ah.comment_before("RmBake RmBake;", HEADER) == " An opaque handle. "
    with pytest.raises(AssertionError):
        ah.comment_before("RmBak", HEADER)


class _Stub:
    def __init__(self, message):
        self.message = message

    def rm_last_error(self):
        return self.message


def test_refused_needs_the_status_a_message_and_the_text(monkeypatch):
    stub = _Stub(b"negative numRays")
    monkeypatch.setattr(ah, "lib", lambda: stub)
    assert ah.refused(ah.INVALID) and ah.refused(ah.INVALID, "numRays") and ah.refused(ah.INVALID, text="negative")
    assert ah.refused(ah.CAPACITY, "numRays", want=ah.CAPACITY)
    # the status
    assert not ah.refused(0) and not ah.refused(ah.CAPACITY) and not ah.refused(ah.INVALID, want=ah.CAPACITY)
    # the text
    assert not ah.refused(ah.INVALID, "numPoints") and not ah.refused(ah.CAPACITY, "numPoints", want=ah.CAPACITY)
    # a message at all
    stub.message = b""
    assert not ah.refused(ah.INVALID) and not ah.refused(ah.CAPACITY, want=ah.CAPACITY)
    assert not ah.refused(ah.INVALID, "")


def test_walk_reports_the_step_the_mend_the_status_and_the_message(monkeypatch):
    stub = _Stub(b"bad frame size")
    monkeypatch.setattr(ah, "lib", lambda: stub)
    seen = []

    def call(a):
        seen.append(dict(a))
        return ah.INVALID if a["W"] <= 0 else 0

    start = dict(W=0, H=0)
    ah.walk(call, start, [(dict(), ah.INVALID, "frame size"), (dict(H=4), ah.INVALID, "bad"), (dict(W=8), 0, None)])
    assert seen == [dict(W=0, H=0), dict(W=0, H=4), dict(W=8, H=4)] and start == dict(W=0, H=0)
    with pytest.raises(AssertionError) as e:
        ah.walk(call, start, [(dict(), ah.INVALID, "frame size"), (dict(W=8), ah.INVALID, "frame size")])
    assert e.value.args[0] == (1, dict(W=8), 0, "bad frame size")
    with pytest.raises(AssertionError) as e:
        ah.walk(call, start, [(dict(), ah.INVALID, "null output")])
    assert e.value.args[0] == (0, dict(), "bad frame size")


def test_pointers_and_vectors():
    assert ah.FAKE.value == 0x1000 and ah.fake(0x1008).value == 0x1008
    assert ah.HP.value % 16 == 0 and ah.HOST.ctypes.data <= ah.HP.value
    assert ah.vec3(None) is None and list(ah.vec3((1, 2.5, -0.0))) == [1.0, 2.5, -0.0]
