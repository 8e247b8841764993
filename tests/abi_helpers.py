"""What test_abi.py and the test_*_abi.py modules share: the public header and its parser, the library handle, the ABI version, the
refusal check, pointers that are never read, the order-of-checks walk and the lattice argument tables.  Each is written once here;
a value or builder that only one module uses stays in that module.  Imported as `import abi_helpers as ah`."""
import ctypes as C
import os
import re

import numpy as np

from raymarcher_amd import abi, lib
from raymarcher_amd._lib import LIB_PATH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "raymarcher_amd.h")).read()
INT_MAX = 2 ** 31 - 1
INVALID, CAPACITY = abi.RM_ERR_INVALID_ARGUMENT, abi.RM_ERR_CAPACITY
ABI_VERSION = 5  # the one place the tests write the number


# ---------------------------------------------------------------- the header's parser
def strip_comments(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


HEADER_CODE = strip_comments(HEADER)


def declared_functions(code=HEADER_CODE):
    return sorted(set(re.findall(r"\b(rm_[a-z0-9_]+)\s*\(", code)))


def params(name, returns="int", code=HEADER_CODE):
    """The parameters of `returns name(...)` as written, blanks squeezed: arrays stay arrays ("const float origin[3]")."""
    m = re.search(r"\b" + returns + r"\s+" + name + r"\s*\(([^)]*)\)", code)
    assert m, f"include/raymarcher_amd.h does not declare {name}"
    return [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]


def comment_before(name, header=HEADER):
    """The comment right in front of the declaration of function `name` or of `typedef struct name` (a name or a regex), joined
    into one line.  #define lines may stand between the comment and the declaration."""
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*(?:#define[^\n]*\n\s*)*(?:(?:int|void)\s+|typedef struct )" + name + r"(?!\w)", header,
                  flags=re.S)
    assert m, f"no comment in front of {name}"
    return re.sub(r"\s*\n\s*\*\s?", " ", m.group(1))


def assert_comment_has(name, words, header=HEADER):
    text = comment_before(name, header)
    for w in words:
        assert w in text, f"the comment of {name} lacks: {w}"


# ---------------------------------------------------------------- the library
def library():
    """A plain ctypes handle of the library: hasattr() on it is a symbol lookup."""
    # the package's loader first: a bare dlopen of the library would bind the system HIP runtime, and the GPU tests later in
    # the same process would then find no device through torch's (_lib._share_torchs_hip_runtime); this handle is the same library
    lib()
    return C.CDLL(LIB_PATH)


def assert_exported(names):
    L = library()
    for n in names:
        assert hasattr(L, n), f"the library does not export {n}"


def assert_abi_version():
    assert abi.RM_ABI_VERSION == ABI_VERSION and lib().rm_abi_version() == ABI_VERSION
    assert re.search(rf"#define\s+RM_ABI_VERSION\s+{ABI_VERSION}\b", HEADER)


def refused(status, text=None, want=INVALID):
    """The status is `want`, rm_last_error() says why, and says `text` where one is given."""
    msg = lib().rm_last_error().decode()
    return status == want and len(msg) > 0 and (text is None or text in msg)


def walk(call, start, steps):
    """The order of the checks: `start` fails every check, each step (mend, status, word) mends one argument, and call(arguments)
    must then return `status` with `word` in rm_last_error() — the earliest check still violated."""
    a = dict(start)
    for step, (mend, status, word) in enumerate(steps):
        a.update(mend)
        got = call(a)
        assert got == status, (step, mend, got, lib().rm_last_error().decode())
        if word is not None:
            assert word in lib().rm_last_error().decode(), (step, mend, lib().rm_last_error().decode())


# ---------------------------------------------------------------- pointers and vectors
def fake(addr):
    """A device pointer that is never dereferenced: every call that gets it fails its checks first."""
    return C.c_void_p(addr)


FAKE = fake(0x1000)  # 16-byte aligned
HOST = np.zeros(4096 + 4, dtype=np.float32)
HP = C.c_void_p(HOST.ctypes.data + (-HOST.ctypes.data) % 16)  # aligned host memory: it gets as far as the device-memory check
assert HP.value % 16 == 0 and HP.value + 4096 * 4 <= HOST.ctypes.data + HOST.nbytes


def vec3(v):
    return (C.c_float * 3)(*v) if v is not None else None


# ---------------------------------------------------------------- the lattice arguments that rm_lattice.h refuses
inf, nan = float("inf"), float("nan")
BAD_STEPS = ((nan, 1, 1), (1, inf, 1), (1, 1, 0.0), (-0.5, 1, 1), (1, -0.0, 1), (1, 1, -inf))
BAD_ORIGINS = ((nan, 0, 0), (0, inf, 0), (0, 0, -inf))
BAD_DIMS = ((0, 2, 2), (2, -1, 2), (4097, 2, 2), (2, 2, 2 ** 31 - 1), (-2 ** 31, 2, 2))  # of a lattice that is sampled: 2 is valid
ONE_DIMS = ((1, 2, 2), (2, 1, 2), (2, 2, 1), (1, 1, 1), (4096, 4096, 1))
BAD_BLOCKS = ((0, 2, 2), (2, -1, 2), (2, 2, 0), (513, 1, 1), (1, 513, 1), (1, 1, 2 ** 31 - 1), (-2 ** 31, 2, 2))
BIG_BLOCKS = ((512, 512, 512), (1, 1, 1), (512, 1, 1), (1, 1, 512))  # 4097³ points and more than INT_MAX of them: a lattice here
BAD_COUNTS = (-1, -2 ** 31, (1 << 22) + 1, 2 ** 31 - 1)


def lattice_refusals(call, dense, still):
    """What the sampled-lattice entries (rm_sdf_sample / rm_sdf_trace, their _blocks forms and the two rm_field creates) refuse
    about the lattice, in order and with their messages.  call(origin=, step=, dims=, nb=) is the module's wrapper; `still`: keyword
    arguments that fail a later check, or make the call one of nothing — the lattice's refusal still comes first."""
    assert refused(call(origin=None), "null origin or step") and refused(call(step=None), "null origin or step")
    assert refused(call(origin=None, **still), "null origin or step")
    for o in BAD_ORIGINS:
        assert refused(call(origin=o), "origin must be finite"), o
    for st in BAD_STEPS:
        assert refused(call(step=st), "step must be finite and greater than 0"), st
        assert refused(call(origin=(nan, 0, 0), step=st), "origin"), st
    if dense:
        for d in BAD_DIMS:
            assert refused(call(dims=d), "lattice dimension must be 1 … RM_MAX_LATTICE_DIM"), d
            assert refused(call(dims=d, step=(0, 1, 1)), "step"), d
        assert refused(call(dims=(4096, 4096, 4096)), "more than INT_MAX lattice points")
        for d in ONE_DIMS:
            assert refused(call(dims=d), "at least 2"), d
            assert refused(call(dims=d, **still), "at least 2"), d
    else:
        for b in BAD_BLOCKS:
            assert refused(call(dims=b), "block dimension"), b
            assert refused(call(dims=b, step=(0, 1, 1)), "step"), b
        for nb in BAD_COUNTS:
            assert refused(call(nb=nb), "numBlocks must be 0 … RM_MAX_BLOCK_LIST"), nb
            assert refused(call(nb=nb, dims=(0, 1, 1)), "block dimension"), nb  # the lattice comes before numBlocks
            assert refused(call(nb=nb, **still), "numBlocks"), nb
