"""Shared test helpers: oracle loader, an independent numpy camera, scene builders."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from raymarcher_amd import abi  # noqa: E402

_ORACLE = None


def oracle():
    """ctypes handle of oracle/_build/librm_oracle.so (built on demand with make)."""
    global _ORACLE
    if _ORACLE is None:
        so = os.environ.get("RM_ORACLE_SO")  # a sanitizer build of the oracle for a one-off check (with LD_PRELOAD=libasan.so)
        if not so:
            so = os.path.join(ROOT, "oracle", "_build", "librm_oracle.so")
            if not os.path.exists(so):
                subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
        lib = C.CDLL(so)
        lib.rmo_const_bits.restype = C.c_uint32
        _ORACLE = lib
    return _ORACLE


def fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


# ------------------------------------------------------------------ the specification libraries (tests/<name>_spec)
# oracle/Makefile's CFLAGS (-ffp-contract=off: the numeric contract fuses only where rm_fma() is written)
SPEC_CFLAGS = ["-O3", "-std=c99", "-fPIC", "-mfma", "-mavx2", "-mf16c", "-ffp-contract=off", "-fno-fast-math", "-fopenmp", "-Wall",
               "-Wextra", "-Wno-unused-function"]
_SPECS = {}


def load_spec(name, signatures):
    """ctypes handle of tests/<name>_spec/_build/librm_<name>_spec.so, built from tests/<name>_spec/rm_<name>_spec.c when that file,
    the oracle's sources or the public header are newer, and loaded once per process.  signatures: {symbol: (restype, argtypes)}."""
    if name not in _SPECS:
        here = os.path.join(ROOT, "tests", f"{name}_spec")
        src, so = os.path.join(here, f"rm_{name}_spec.c"), os.path.join(here, "_build", f"librm_{name}_spec.so")
        deps = [src] + [os.path.join(ROOT, "oracle", f) for f in ("rm_oracle.c", "rm_oracle.h", "rm_math.h")] + \
               [os.path.join(ROOT, "include", "raymarcher_amd.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            tmp = f"{so}.{os.getpid()}.tmp"  # two test processes may build at once: each links its own file, then renames
            subprocess.check_call([os.environ.get("CC", "gcc")] + SPEC_CFLAGS + ["-shared", "-o", tmp, src, "-lm"])
            os.replace(tmp, so)
        lib = C.CDLL(so)
        for symbol, (restype, argtypes) in signatures.items():
            fn = getattr(lib, symbol)
            fn.restype, fn.argtypes = restype, argtypes
        _SPECS[name] = lib
    return _SPECS[name]


# ------------------------------------------------------------------ tables for the renderer, the one bit comparator
def tables_of(scene, res=None, **resources):
    """SceneTables of the tests' scene tuple (camera, objects, count, lights, count, globals, …) with the resources of `res` (a
    dict) and of the keywords set on it.  A NumPy array that is not writeable (a shared, cached one) is copied first:
    Renderer._upload hands the array to torch.from_numpy.  A writeable one is passed on as it is."""
    from raymarcher_amd.render import SceneTables
    t = SceneTables(*scene[:6])
    for k, v in {**(res or {}), **resources}.items():
        setattr(t, k, v.copy() if isinstance(v, np.ndarray) and not v.flags.writeable else v)
    return t


def bits(a):
    """The words of an array of 4-byte elements as they are: never a conversion by value."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, f"bits() of {a.dtype}: not a 4-byte type"
    return a.view(np.uint32)


def assert_bit_equal(got, want, what):
    """Word-for-word equality of two arrays of 4-byte elements with the same shape (+0 is not −0, a NaN equals only itself)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype.itemsize == 4 and want.dtype.itemsize == 4, f"{what}: {got.dtype} against {want.dtype}: not 4-byte types"
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    bad = bits(got) != bits(want)
    if bad.any():
        delta = ""
        if got.dtype.kind == "f" and want.dtype.kind == "f":
            with np.errstate(all="ignore"):
                diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
            diff = diff[~np.isnan(diff)]
            delta = f" max |Δ| = {diff.max() if diff.size else np.nan:.3e};"
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} words differ;{delta} first at {np.argwhere(bad)[:5].tolist()}")


def with_globals(g, **over):
    """A copy of an RmGlobals with fields replaced (julia=(x, y) sets juliaSeed)."""
    g2 = abi.RmGlobals()
    C.memmove(C.byref(g2), C.byref(g), C.sizeof(g))
    for k, v in over.items():
        if k == "julia":
            g2.juliaSeed[0], g2.juliaSeed[1] = v
        else:
            setattr(g2, k, v)
    return g2


def table(items, struct=abi.RmObject):
    """(ctypes array of at least one element, count) of a list of structs."""
    items = list(items)
    return (struct * max(len(items), 1))(*items), len(items)


# ------------------------------------------------------------------ numpy camera (camera.cpp:74-133)
def camera_numpy(pos, look, up, height_angle_rad, W, H, near=0.1, far=100.0):
    f = np.float32
    pos, look, up = (np.asarray(v, dtype=f)[:3] for v in (pos, look, up))
    T = np.eye(4, dtype=f)
    T[:3, 3] = -pos
    w = -look / np.linalg.norm(look).astype(f)
    v = up - np.dot(up, w) * w
    v = v / np.linalg.norm(v).astype(f)
    u = np.cross(v, w)
    R = np.eye(4, dtype=f)
    R[0, :3], R[1, :3], R[2, :3] = u, v, w
    view = (R @ T).astype(f)
    aspect = f(W) / f(H)
    vh = f(2) * f(far) * np.tan(f(height_angle_rad) / f(2)).astype(f)
    vw = aspect * vh
    S = np.diag([f(2) / vw, f(2) / vh, f(1) / f(far), f(1)]).astype(f)
    c = -f(near) / f(far)
    U = np.eye(4, dtype=f)
    U[2, 2] = f(1) / (f(1) + c)
    U[2, 3] = -c / (f(1) + c)
    U[3, 2] = f(-1)
    U[3, 3] = f(0)
    G = np.eye(4, dtype=f)
    G[2, 2] = f(-2)
    G[2, 3] = f(-1)
    proj = (G @ U @ S).astype(f)
    inv = np.linalg.inv((proj @ view).astype(np.float64)).astype(f)
    return view, proj, inv


def make_camera(pos, look, up, height_angle_deg, W, H, near=0.1, far=100.0):
    _, _, inv = camera_numpy(pos, look, up, np.deg2rad(height_angle_deg), W, H, near, far)
    cam = abi.RmCamera()
    colmajor = inv.T.reshape(-1)  # column-major storage
    for i in range(16):
        cam.invProjView[i] = float(colmajor[i])
    cam.initialFar = far
    for i in range(3):
        cam.eyePosition[i] = float(pos[i])
    cam.eyePosition[3] = 1.0
    return cam


def make_object(type_, model=None, scale_factor=1.0, ambient=(0, 0, 0), diffuse=(1, 1, 1), specular=(0, 0, 0),
                shininess=0.0, reflective=(0, 0, 0), transparent=(0, 0, 0), ior=0.0):
    o = abi.RmObject()
    o.type = type_
    M = np.eye(4) if model is None else np.asarray(model, dtype=np.float64)
    inv = np.linalg.inv(M).astype(np.float32).T.reshape(-1)
    for i in range(16):
        o.invModel[i] = float(inv[i])
    o.scaleFactor = scale_factor
    o.shininess = shininess
    o.ior = ior
    for i in range(3):
        o.cAmbient[i], o.cDiffuse[i], o.cSpecular[i] = ambient[i], diffuse[i], specular[i]
        o.cReflective[i], o.cTransparent[i] = reflective[i], transparent[i]
    o.texLoc = -1
    o.lightIdx = -1
    return o


def make_light(type_, color=(1, 1, 1), direction=(0, 0, 0), pos=(0, 0, 0), func=(1, 0, 0), angle=0.0, penumbra=0.0):
    li = abi.RmLight()
    li.type = type_
    for i in range(3):
        li.color[i], li.dir[i], li.pos[i], li.func[i] = color[i], direction[i], pos[i], func[i]
    li.angle, li.penumbra = angle, penumbra
    return li


def make_globals(ka=0.5, kd=0.5, ks=0.5, kt=0.5, power=8.0, julia=(0, 0), itime=0.0, two_d=0):
    g = abi.RmGlobals(ka, kd, ks, kt, power)
    g.juliaSeed[0], g.juliaSeed[1] = julia
    g.iTime = itime
    g.isTwoD = two_d
    return g


def translate(x, y, z):
    M = np.eye(4)
    M[:3, 3] = (x, y, z)
    return M


def scale(x, y, z):
    return np.diag([x, y, z, 1.0])


def scene_mandelbulb(W, H):
    """scenefiles/simple/unit_mandelbulb.json as constants."""
    cam = make_camera((0, 0, 4.5), (0, 0, -4.5), (0, 1, 0), 30.0, W, H)
    objs = (abi.RmObject * 1)(make_object(abi.RM_MANDELBULB, ambient=(.3, .3, .3), diffuse=(1, 1, 1),
                                          specular=(1, 1, 1), shininess=100.0, ior=1.5))
    lights = (abi.RmLight * 3)(
        make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (0, 0, 1)),
        make_light(abi.RM_LIGHT_DIRECTIONAL, (1.5, 1.1, 0.7), (0, -1, 0)),
        make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (0, 0, -1)))
    return cam, objs, 1, lights, 3, make_globals()


def host_resources(textures=None, noise=None, skybox=None, ltc1=None, ltc2=None):
    """RmResources over HOST arrays (for the oracle); returns (struct, keep-alive)."""
    res = abi.RmResources()
    keep = []

    def fill(slot, a):
        assert a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"] and a.shape[2] == 4
        slot.pixels = a.ctypes.data
        slot.height, slot.width = a.shape[0], a.shape[1]
        keep.append(a)

    if textures:
        tex = (abi.RmTexture * len(textures))()
        for i, a in enumerate(textures):
            fill(tex[i], a)
        res.textures = tex
        res.numTextures = len(textures)
        keep.append(tex)
    if noise is not None:
        fill(res.noise, noise)
    if skybox:
        for f in range(6):
            fill(res.skybox[f], skybox[f])
    for name, a in (("ltc1", ltc1), ("ltc2", ltc2)):
        if a is not None:
            assert a.dtype == np.uint8 and a.shape == (64, 64, 4) and a.flags["C_CONTIGUOUS"]
            setattr(res, name, a.ctypes.data)
            keep.append(a)
    return res, keep


def oracle_render(scene, settings, W, H, row0=0, row1=None, threads=8, bright=False, counters=False, textures=None,
                  expect=0, **resources):
    """textures: list of uint8 (H, W, 4) arrays, rows bottom-up, indexed by RmObject.texLoc; resources: noise=, skybox=,
    ltc1=, ltc2= (see host_resources)."""
    cam, objs, no, lights, nl, g = scene[:6]
    row1 = H if row1 is None else row1
    out = np.zeros((row1 - row0, W, 4), dtype=np.float32)
    br = np.zeros_like(out) if bright else None
    cnt = abi.RmCounters()
    res, _keep = host_resources(textures=textures, **resources)
    st = oracle().rmo_render_res(C.byref(cam), objs, no, lights, nl, C.byref(g), C.byref(settings), C.byref(res), W, H,
                                 row0, row1, fptr(out), fptr(br) if bright else None, C.byref(cnt), threads)
    assert st == expect, f"oracle status {st}"
    res = [out]
    if bright:
        res.append(br)
    if counters:
        res.append(cnt)
    return res[0] if len(res) == 1 else tuple(res)


# ------------------------------------------------------------------ the binary64 arbiter (oracle/rm_oracle_f64.c)
_ARBITER = None
_F64_TYPES = {}


def arbiter():
    """ctypes handle of oracle/_build/librm_oracle_f64.so: the same restatement with every float a double and libm
    built-ins.  Compared with tolerances only."""
    global _ARBITER
    if _ARBITER is None:
        so = os.path.join(ROOT, "oracle", "_build", "librm_oracle_f64.so")
        if not os.path.exists(so):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle")], stdout=subprocess.DEVNULL)
        _ARBITER = C.CDLL(so)
    return _ARBITER


def _f64_type(t):
    """The ctypes twin of an ABI type with every c_float a c_double (what `#define float double` makes of the header)."""
    if t is C.c_float:
        return C.c_double
    if t in _F64_TYPES:
        return _F64_TYPES[t]
    if isinstance(t, type) and issubclass(t, C.Array):
        r = _f64_type(t._type_) * t._length_
    elif isinstance(t, type) and issubclass(t, C.Structure):
        r = type(t.__name__ + "F64", (C.Structure,), {"_fields_": [(n, _f64_type(ft)) for n, ft in t._fields_]})
    else:
        r = t
    _F64_TYPES[t] = r
    return r


def _to_f64(src):
    """Copy an ABI struct / array into its binary64 twin, field by field (exact: every binary32 is a binary64)."""
    dst = _f64_type(type(src))()

    def copy(d, s_):
        if isinstance(s_, C.Array):
            for i in range(len(s_)):
                if isinstance(s_[i], (C.Array, C.Structure)):
                    copy(d[i], s_[i])
                else:
                    d[i] = s_[i]
        else:
            for n, _ in s_._fields_:
                v = getattr(s_, n)
                if isinstance(v, (C.Array, C.Structure)):
                    copy(getattr(d, n), v)
                else:
                    setattr(d, n, v)
    copy(dst, src)
    return dst


def arbiter_render(scene, settings, W, H, row0=0, row1=None, threads=8, textures=None, **resources):
    """The frame in binary64 (float64 array, rows × W × 4)."""
    cam, objs, no, lights, nl, g = scene[:6]
    row1 = H if row1 is None else row1
    out = np.zeros((row1 - row0, W, 4), dtype=np.float64)
    res, _keep = host_resources(textures=textures, **resources)  # pointers and ints only: same layout in both builds
    cam64, objs64, lights64, g64 = _to_f64(cam), _to_f64(objs), _to_f64(lights), _to_f64(g)
    st = arbiter().rmo_render_res(C.byref(cam64), objs64, no, lights64, nl, C.byref(g64), C.byref(settings), C.byref(res), W, H,
                                  row0, row1, out.ctypes.data_as(C.POINTER(C.c_double)), None, None, threads)
    assert st == 0, f"arbiter status {st}"
    return out


def oracle_ltc_quantise(table):
    t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1, 4)
    out = np.empty(t.shape, dtype=np.uint8)
    oracle().rmo_ltc_quantise(fptr(t), out.ctypes.data_as(C.c_void_p), t.shape[0])
    return out.reshape(np.shape(table))


def oracle_post(frag, bright, post):
    """rmo_post_process on host arrays (H, W, 4)."""
    H, W = frag.shape[:2]
    out = np.empty((H, W, 4), dtype=np.float32)
    frag = np.ascontiguousarray(frag, dtype=np.float32)
    b = None if bright is None else np.ascontiguousarray(bright, dtype=np.float32)
    st = oracle().rmo_post_process(fptr(frag), fptr(b) if b is not None else None, fptr(out), W, H, C.byref(post))
    assert st == 0, f"oracle post status {st}"
    return out


# ------------------------------------------------------------------ wide random tables for the table walk's exact shortcuts
PRIMITIVES = [abi.RM_CUBE, abi.RM_CONE, abi.RM_CYLINDER, abi.RM_SPHERE, abi.RM_OCTAHEDRON, abi.RM_TORUS, abi.RM_CAPSULE,
              abi.RM_DEATHSTAR, abi.RM_RECTANGLE]


def rotation(axis, angle):
    """Rotation by `angle` about an arbitrary axis (Rodrigues), 4×4."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    return M


def random_tablewalk_objects(rng, max_objects=30, materials=True):
    """A random all-primitive table drawn WIDE — what the pass-over test, the runner-up tracking and the ball ∩ box culls of the
    table walk (rm_device.hip.h sdSceneImpl / march, rm_frame.cpp scene_cull_ball) must survive without changing a bit:
    arbitrary-axis rotations, shear, anisotropy 0.2–5, a scaleFactor that is deliberately NOT the smallest scale (the ABI accepts
    any: the distance values are then not 1-Lipschitz, which the launcher's `lip` must account for), objects inside objects,
    coincident copies (ties: the lower index wins), tables of up to 30.  Returns a list of RmObject."""
    f = rng.uniform
    n = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 12, 20, 25, max_objects]))
    n = min(n, max_objects)
    spread = 2.2 if n <= 8 else 4.0
    objs, models = [], []

    def material():
        if not materials:
            return {}
        return dict(ambient=tuple(f(0, .3, 3)), diffuse=tuple(f(.2, 1, 3)), specular=tuple(f(0, 1, 3)),
                    shininess=float(rng.choice([0, 1, 7.5, 25, 100])), reflective=tuple(f(0, .8, 3)) if f() < 0.4 else (0, 0, 0),
                    transparent=tuple(f(0, .8, 3)) if f() < 0.3 else (0, 0, 0), ior=float(f(1.05, 1.6)))

    while len(objs) < n:
        ty = int(rng.choice(PRIMITIVES))
        kind = f()
        if objs and kind < 0.12:      # a coincident copy of an earlier object (same shape or another one, other material)
            M, sc = models[int(rng.integers(0, len(models)))]
            if f() < 0.5:
                ty = objs[-1].type
        elif objs and kind < 0.27:    # nested: inside an earlier object, smaller, same centre or slightly off
            P, psc = models[int(rng.integers(0, len(models)))]
            k = float(f(0.2, 0.7))
            M = P @ translate(*(f(-0.1, 0.1, 3))) @ rotation(rng.normal(size=3), f(-3, 3)) @ scale(k, k, k)
            sc = psc * k
        else:
            base = float(f(0.5, 1.8)) if n <= 8 else float(f(0.4, 1.0))
            an = np.ones(3) if f() < 0.4 else np.exp(f(np.log(0.2), np.log(5.0), 3)) ** 0.5  # pairwise ratio up to 5 (25 at the extremes)
            if f() < 0.15:
                an = np.exp(f(np.log(0.2), np.log(5.0), 3))
            sx, sy, sz = base * an
            S = scale(sx, sy, sz)
            sh = np.eye(4)
            if f() < 0.3:             # shear
                i, j = rng.choice(3, 2, replace=False)
                sh[i, j] = float(f(-0.8, 0.8))
                if f() < 0.3:
                    sh[j, (i + 1) % 3 if (i + 1) % 3 != j else (i + 2) % 3] = float(f(-0.5, 0.5))
            M = translate(f(-spread, spread), f(-1.0, 1.4), f(-2.8, 1.0)) @ rotation(rng.normal(size=3), f(-3.2, 3.2)) @ sh @ S
            sc = min(sx, sy, sz)
        sf = sc
        if f() < 0.25:                # a scaleFactor the loader would not have produced
            sf = sc * float(rng.choice([0.3, 0.5, 0.8, 1.3, 2.0, 3.0]))
        objs.append(make_object(ty, model=M, scale_factor=float(sf), **material()))
        models.append((M, sc))
    return objs


# ------------------------------------------------------------------ guarded, poisoned output buffers (write coverage)
FLOAT_POISON = 0x7FA5A5A5      # a signalling NaN with a fixed payload: GPU arithmetic only ever produces quiet NaNs
U8_POISONS = (0xA5, 0x5A)      # a byte poison can be a real value: uint8 outputs are produced twice, once under each


def _i32(v):
    return v - (1 << 32) if v >= 1 << 31 else v


class Guarded:
    """One device allocation: a guard band, the payload, a guard band, all filled with `poison` (see guarded)."""

    def __init__(self, shape, dtype, poison, device):
        import torch
        self.shape, self.dtype, self.poison = tuple(int(d) for d in shape), dtype, poison
        item = torch.empty((), dtype=dtype).element_size()
        row = item * (self.shape[-2] * self.shape[-1] if len(self.shape) >= 2 else 1)
        self.nbytes = item * int(np.prod(self.shape, dtype=np.int64))
        self.guard = max(4096, -(-row // 256) * 256)  # >= one output row, >= 4 KB, a multiple of 256 bytes
        tail = self.guard + (-self.nbytes) % 256  # the back guard starts right at the payload's end
        self.buf = torch.empty(self.guard + self.nbytes + tail, dtype=torch.uint8, device=device)
        if item == 1:
            self.buf.fill_(poison)
        else:
            self.buf.view(torch.int32).fill_(_i32(poison))  # through an integer view: a float fill would lose the NaN's payload
        self.payload = self.buf[self.guard:self.guard + self.nbytes].view(dtype).view(self.shape)

    def _unwritten(self, region):
        """Mask of the words (bytes for uint8) of a region of buf that still hold the poison."""
        import torch
        return region == self.poison if self.dtype.itemsize == 1 else region.view(torch.int32) == _i32(self.poison)

    def check(self):
        """Both guards still hold the poison bit for bit, and (float payloads) no payload word still holds it; a uint8 payload can
        hold its poison legitimately: see guarded_u8.  Synchronises through the comparisons."""
        end = self.guard + self.nbytes
        for name, lo, hi in (("front", 0, self.guard), ("back", end, self.buf.numel())):
            kept = self._unwritten(self.buf[lo:hi])
            if not bool(kept.all()):
                w = int((~kept).nonzero()[0, 0]) * (hi - lo) // kept.numel()  # byte offset in the guard
                off = f"{self.guard - w} bytes before the payload" if name == "front" else f"{w} bytes past its end"
                raise AssertionError(f"{name} guard written: {int((~kept).sum())} of {kept.numel()} guard words changed, "
                                     f"the first {off}")
        if self.dtype.itemsize == 1:
            return
        left = self._unwritten(self.buf[self.guard:end])
        if bool(left.any()):
            i = int(left.nonzero()[0, 0]) * 4 // self.dtype.itemsize
            where = tuple(int(v) for v in np.unravel_index(i, self.shape))
            raise AssertionError(f"{int(left.sum())} of {left.numel()} payload words never written; the first at {where} "
                                 f"(row, column, channel) of {self.shape}")


def guarded(shape, dtype=None, poison=FLOAT_POISON, device="cuda"):
    """A freshly poisoned output between two guard bands → (payload view, check).  check() asserts that both guards still hold
    the poison and that no payload word does (the names of the first offending element or guard byte are in the message)."""
    import torch
    g = Guarded(shape, torch.float32 if dtype is None else dtype, poison, device)
    return g.payload, g.check


def guarded_u8(shape, produce, device="cuda"):
    """Produce a uint8 output twice, into buffers poisoned with 0xA5 and with 0x5A: `produce(out)` writes `out`.  Both results
    equal and both guards intact → the result (a byte the launch never wrote would differ between the two)."""
    import torch
    got = []
    for p in U8_POISONS:
        out, check = guarded(shape, torch.uint8, p, device)
        produce(out)
        check()
        got.append(out)
    bad = got[0] != got[1]
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} bytes differ under the two poisons (never written); the first at {i}")
    return got[0]


def render_guarded(renderer, tables, settings, W, H, row_begin=0, row_end=None, bright=False):
    """Renderer.render into freshly poisoned, guarded buffers (and the bright one too with bright=True), checked before it
    returns: a pixel the launch never wrote, or a write past either end of the rows, fails here."""
    row_end = H if row_end is None else row_end
    out, c1 = guarded((row_end - row_begin, W, 4), device=renderer.device)
    br, c2 = guarded((row_end - row_begin, W, 4), device=renderer.device) if bright else (None, None)
    renderer.render(tables, settings, W, H, row_begin, row_end, bright=bright, out=out, out_bright=br)
    c1()
    if bright:
        c2()
        return out, br
    return out


def render_tiles_guarded(renderer, tables, settings, W, H, tile_rows, shard, num_shards):
    """Renderer.render_tiles into a freshly poisoned, guarded buffer of exactly the shard's rows, checked before it returns."""
    from raymarcher_amd import lib
    out, check = guarded((lib().rm_shard_rows(H, tile_rows, shard, num_shards), W, 4), device=renderer.device)
    renderer.render_tiles(tables, settings, W, H, tile_rows, shard, num_shards, out=out)
    check()
    return out
