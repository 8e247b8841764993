"""Every production instantiation of the scene evaluator (rm_device.hip.h sdSceneImpl / sdSceneOne), point by point, on waves
built to trip its wave-uniform shortcuts, against the CPU oracle bit for bit (rm_probe_sdscene_variant; point i runs on lane
i % 64 of wave i / 64).

Compared bit for bit: d and idx always; the orbit trap where the variant defines it (TRAP 1: all four components, TRAP 2: .z
alone, TRAP 0: none).  The one allowance: a trap component that is NaN on both sides counts as equal, because DESIGN §3 does not
define the bits of a NaN produced by arithmetic (the oracle's host NaN and the GPU's differ in sign and payload); d and idx can
never be NaN (the minimum starts at 1e6 and takes a value only through a strict <).  Every evaluated point must also give the
same bits (NaN trap components included) in every wave context it is put in."""
import ctypes as C
import types

import numpy as np
import pytest

import helpers as h
from raymarcher_amd import abi

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
WALK = [(c, t, s, k) for (c, t, s, k) in [  # (count, trap, skip, track) of the table walk (tests/test_sdscene_variant_abi.py)
    (0, 0, 0, 0), (0, 0, 1, 0), (0, 0, 1, 1), (1, 0, 0, 0), (2, 0, 0, 0), (2, 0, 1, 0), (2, 0, 1, 1),
    (0, 1, 0, 0), (0, 1, 1, 1), (1, 1, 0, 0), (2, 1, 0, 0), (2, 1, 1, 1), (0, 2, 0, 0), (0, 2, 1, 0)]]
BULB_GENERAL = [(c, t) for c in (0, 1, 2) for t in (0, 1)]
BULB_PLAIN = [(0, 0), (0, 1)]
TRAP_COLS = {0: [], 1: [2, 3, 4, 5], 2: [4]}


@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from raymarcher_amd import Renderer
    return Renderer(0)


def tables(objs, g):
    arr = (abi.RmObject * len(objs))(*objs)
    return types.SimpleNamespace(objects=arr, num_objects=len(objs), globals_=g)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def run(R, t, s, pts, ub=None, **variant):
    p = torch.from_numpy(np.ascontiguousarray(pts, dtype=F32)).to(R.device)
    u = None if ub is None else torch.from_numpy(np.ascontiguousarray(ub, dtype=F32)).to(R.device)
    out = R.probe_sdscene_variant(t, s, p, ub=u, **variant)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def oracle(t, s, pts):
    p = np.ascontiguousarray(pts, dtype=F32)
    out = np.empty((len(p), 6), dtype=F32)
    assert h.oracle().rmo_probe_sdscene_trap4(t.objects, t.num_objects, C.byref(t.globals_), C.byref(s), h.fptr(p), h.fptr(out),
                                              len(p)) == 0
    return out


def same(a, b, nan_equal):
    """Bitwise equality; with nan_equal, two NaNs of any bits also count as equal."""
    eq = bits(a) == bits(b)
    if nan_equal:
        eq |= np.isnan(a) & np.isnan(b)
    return eq


def check_against_oracle(dev, ref, trap, what):
    for col, name in ((0, "d"), (1, "idx")):
        bad = ~same(dev[:, col], ref[:, col], False)
        assert not bad.any(), f"{what}: {name} differs at {np.flatnonzero(bad)[:8]}: dev {dev[bad, col][:4]} oracle {ref[bad, col][:4]}"
    for col in TRAP_COLS[trap]:
        bad = ~same(dev[:, col], ref[:, col], True)
        assert not bad.any(), f"{what}: trap[{col - 2}] differs at {np.flatnonzero(bad)[:8]}: dev {dev[bad, col][:4]} oracle {ref[bad, col][:4]}"


def check_contexts(dev, ids, what):
    """Rows of dev that evaluate the same point (ids[i] = the point's number) carry the same bits in columns 0-6."""
    order = np.argsort(ids, kind="stable")
    d, k = dev[order][:, :7], ids[order]
    first = np.r_[True, k[1:] != k[:-1]]
    rep = d[np.maximum.accumulate(np.where(first, np.arange(len(k)), 0))]
    bad = (bits(d) != bits(rep)).any(axis=1)
    assert not bad.any(), f"{what}: a point gives other bits in another wave context (points {np.unique(k[bad])[:8]})"


def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf) if k > 0 else F32(-np.inf), dtype=F32)
    return F32(x)


# ---------------------------------------------------------------- the single-Mandelbulb class
def _bulb_edge_points(rng):
    z = [0.0, -0.0]
    P = [(x, y, w) for x in z for y in z for w in z]                                   # the origin, every sign of zero
    P += [(sx, sy * 0.7, sw) for sx in z for sw in z for sy in (1, -1)]                 # the y axis
    P += [(0.5, -0.0, 0.6), (-0.0, 0.3, 0.8), (0.6, 0.4, -0.0), (-0.0, -0.9, 0.0)]      # one zero coordinate
    t = F32(2.0 ** -48)
    for k in (-2, -1, 0, 1, 2):                                                         # mx at the RAW guard's threshold
        v = _step(t, k)
        P += [(v, 0.8, 0.0), (0.0, 0.8, -v), (-v, 0.3, 0.0)]
    tiny = [np.finfo(F32).tiny, F32(1e-40), F32(2.0 ** -149)]                           # FLT_MIN, a denormal, the smallest
    P += [(v, 0.5, 0.0) for v in tiny] + [(0.0, 0.5, -v) for v in tiny] + [(v, v, v) for v in tiny]
    d = rng.normal(size=(3, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for R_ in (250.0, 255.0, 256.0, 257.0, 266.0):                                      # m overflows after one step from ~256
        P += [tuple(R_ * d[i]) for i in range(3)]
    big = np.finfo(F32).max
    P += [(1e19, 1e19, 1e19), (1.1e19, 1.1e19, 1.1e19), (2e19, 0.5, 0.5), (0.5, -2e19, 0.5), (big, 0, 0), (-big, big, big)]
    inf, nan = np.inf, np.nan
    P += [(inf, 0.5, 0.5), (0.5, -inf, 0.5), (0.5, 0.5, inf), (inf, inf, -inf), (nan, 0.5, 0.5), (0.5, nan, 0.5), (0.5, 0.5, nan)]
    pts = np.array(P, dtype=F32)
    snan = np.array([0x7FA00001, 0xFFA12345, 0x7FC54321, 0xFFFFFFFF], np.uint32).view(F32)  # signalling and quiet NaN payloads
    extra = np.array([[snan[0], 0.5, 0.5], [0.5, snan[1], 0.5], [0.5, 0.5, snan[2]], [snan[3], 0.2, 0.1]], F32)
    extra[0, 0], extra[1, 1], extra[2, 2], extra[3, 0] = snan[0], snan[1], snan[2], snan[3]
    return np.concatenate([pts, extra])


def _bulb_ordinary_points(rng, n=63):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[:, 1] *= 0.9                                                    # away from the y axis: every lane would take the RAW step
    return (d * rng.uniform(0.35, 1.3, (n, 1))).astype(F32)


def _bulb_layout(E, O, tail):
    """Point numbers (0 … len(O)-1 ordinary, len(O) … edge) in wave order: per edge point four waves of the 63 ordinary points
    with the edge point at lane 0, 31, 32 or 63 (contexts a and c); the edge points alone, padded to whole waves (b); the
    ordinary points alone; and a partial last wave of `tail` lanes (1, or 63 with an edge point at lane 31)."""
    nO, nE = len(O), len(E)
    assert nO == 63
    ids = []
    for e in range(nE):
        for lane in (0, 31, 32, 63):
            w = list(range(nO))
            w.insert(lane, nO + e)
            ids += w
    edge = [nO + e for e in range(nE)]
    ids += edge + edge[:(-nE) % 64]
    ids += list(range(nO)) + [0]
    ids += [nO + nE - 1] if tail == 1 else list(range(31)) + [nO + 3] + list(range(31, 62))
    ids = np.array(ids)
    assert len(ids) % 64 == tail
    return ids


def _bulb_tables(rng):
    g = h.make_globals
    bulb = lambda **kw: h.make_object(abi.RM_MANDELBULB, **kw)  # noqa: E731
    out = []
    plain = bulb()
    signed = bulb()
    for i in (1, 2, 4, 6, 8, 9, 12, 13, 14):                                       # −0 off the diagonal, where the loader puts it
        signed.invModel[i] = -0.0 if rng.uniform() < 0.5 else 0.0
    out += [("plain", [plain], g(), True), ("plain-signed-zeros", [signed], g(), True)]
    # general forms: a model with exact zeros of random sign in invModel (an axis permutation with a translation and a scale)
    M = np.array([[0, 0, 2, 0.25], [0, -2, 0, -0.5], [2, 0, 0, 0.125], [0, 0, 0, 1]], dtype=np.float64)
    moved = bulb(model=M, scale_factor=2.0)
    for i in range(16):
        if moved.invModel[i] == 0.0 and rng.uniform() < 0.5:
            moved.invModel[i] = -0.0
    rot = bulb(model=h.translate(0.1, -0.2, 0.05) @ h.rotation((1, 2, 3), 0.7) @ h.scale(1.5, 1.5, 1.5), scale_factor=1.5)
    out += [("moved", [moved], g(), False), ("rotated", [rot], g(), False), ("julia", [plain], g(julia=(0.35, -0.2)), False),
            ("small-scale", [bulb(model=h.scale(0.01, 0.01, 0.01), scale_factor=0.01)], g(), False)]
    for pw in (6.0, 7.5, 3.0, 1.0, 0.0, -2.0, 200.0, 2e6):
        out.append((f"power{pw}", [plain], g(power=pw), False))
    return out


def _settings(**kw):
    s = abi.default_settings()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def test_bulb_variants_on_adversarial_waves(R):
    rng = np.random.default_rng(11)
    E, O = _bulb_edge_points(rng), _bulb_ordinary_points(rng)
    P = np.concatenate([O, E])
    algebraic = abi.RM_FEAT_BULB_POWER8_ALGEBRAIC
    runs = 0
    for ti, (name, objs, g, plain_ok) in enumerate(_bulb_tables(rng)):
        t = tables(objs, g)
        settings = [_settings()]
        if g.power == 8.0:
            settings.append(_settings(features=abi.default_settings().features | algebraic))
        if name == "plain":
            settings += [_settings(fractalIters=k) for k in (0, 1, 2, 12)]
        for si, s in enumerate(settings):
            ref = oracle(t, s, P)
            variants = [(1, c, tr) for c, tr in BULB_GENERAL] + ([(2, c, tr) for c, tr in BULB_PLAIN] if plain_ok else [])
            for vi, (cls, count, trap) in enumerate(variants):
                ids = _bulb_layout(E, O, 1 if (ti + si + vi) % 2 else 63)
                dev = run(R, t, s, P[ids], bulb_class=cls, count=count, trap=trap)
                what = f"{name} settings#{si} class {cls} count {count} trap {trap}"
                check_against_oracle(dev, ref[ids], trap, what)
                check_contexts(dev, ids, what)
                assert (dev[:, 6] == np.inf).all()
                assert (dev[:, 7] == (1.0 if count else 0.0)).all(), what
                runs += 1
    assert runs >= 100


# ---------------------------------------------------------------- the Menger sponge
def _menger_points(rng):
    P = list(rng.uniform(-1.6, 1.6, (120, 3)))
    grid = [0.0, -0.0, 1.0, -1.0, 2.0, 0.5, -1.5, 1.5]
    for m in range(1, 8):                                          # multiples of 2 / 3^m: p·hs at or next to an integer
        grid += [F32(2.0 * k / 3 ** m) for k in (1, 2, 4, -5)]
    for i in range(100):
        P.append(tuple(rng.choice(grid, 3)))
    big, inf, nan = np.finfo(F32).max, np.inf, np.nan
    P += [(1e30, 0.2, 0.3), (-3e38, 3e38, 0.1), (big, big, big), (inf, 0.3, 0.1), (0.3, -inf, 0.1), (0.1, 0.3, inf),
          (nan, 0.3, 0.1), (0.3, nan, 0.1), (0.1, 0.3, nan), (inf, -inf, nan), (1e7, 1e7, -1e7), (6561.0, 0.5, 2187.0)]
    return np.array(P, dtype=F32)


def test_menger_variants_every_level_still_and_animated(R):
    rng = np.random.default_rng(12)
    P = _menger_points(rng)
    ids = np.r_[np.arange(len(P)), rng.permutation(len(P))[:63]]  # every point twice, in two wave contexts, partial last wave
    for it in (0.0, 3.0, 4.0):
        for model in (None, h.translate(0.2, -0.1, 0.3) @ h.rotation((0, 1, 1), 0.4)):
            t = tables([h.make_object(abi.RM_MENGERSPONGE, model=model)], h.make_globals(itime=it))
            for levels in range(11):
                s = _settings(mengerLevels=levels)
                ref = oracle(t, s, P)[ids]
                for count, trap, skip, track in WALK:
                    dev = run(R, t, s, P[ids], count=count, trap=trap, skip=skip, track=track)
                    what = f"Menger iTime {it} levels {levels} count {count} trap {trap} skip {skip} track {track}"
                    check_against_oracle(dev, ref, trap, what)
                    check_contexts(dev, ids, what)


# ---------------------------------------------------------------- the table walk: SKIP, TRACK, COUNT, and sdSceneOne
def _walk_tables(rng):
    out = []
    prims = h.PRIMITIVES
    for ty in prims:
        out.append((f"type{ty}", [h.make_object(ty, model=h.translate(0.2, 0.1, -0.3) @ h.rotation((1, 1, 0), 0.5) @ h.scale(1.2, 0.8, 1.0),
                                                scale_factor=0.8)]))
    allp = [h.make_object(ty, model=h.translate(1.3 * (i % 3) - 1.3, 1.3 * (i // 3) - 1.3, 0.2 * i), scale_factor=1.0)
            for i, ty in enumerate(prims)]
    out.append(("all-primitives", allp))
    for seed in range(5):
        out.append((f"random{seed}", h.random_tablewalk_objects(np.random.default_rng(100 + seed))))
    M = h.translate(0.3, 0, 0)
    out.append(("duplicates", [h.make_object(abi.RM_SPHERE, model=M), h.make_object(abi.RM_SPHERE, model=M),
                               h.make_object(abi.RM_CUBE, model=M), h.make_object(abi.RM_SPHERE, model=M)]))
    out.append(("unbounded-scale", [h.make_object(abi.RM_CUBE, model=h.translate(1, 0, 0)),
                                    h.make_object(abi.RM_SPHERE, model=h.scale(1e-7, 1e-7, 1e-7), scale_factor=1e-7),
                                    h.make_object(abi.RM_TORUS, model=h.scale(2e6, 2e6, 2e6), scale_factor=2e6),
                                    h.make_object(abi.RM_CAPSULE, model=h.translate(-1, 0, 0))]))
    out.append(("fractals-between", [h.make_object(abi.RM_CUBE, model=h.translate(2, 0, 0)),
                                     h.make_object(abi.RM_MENGERSPONGE, model=h.translate(-2, 0, 0)),
                                     h.make_object(abi.RM_SPHERE, model=h.translate(0, 2, 0)),
                                     h.make_object(abi.RM_MANDELBULB, model=h.translate(0, -2, 0)),
                                     h.make_object(abi.RM_TORUS, model=h.translate(0, 0, 2)),
                                     h.make_object(abi.RM_MENGERSPONGE, model=h.translate(0, 0, -2) @ h.scale(0.5, 0.5, 0.5), scale_factor=0.5),
                                     h.make_object(abi.RM_CAPSULE, model=h.translate(1, 1, 1))]))
    return out


def _single_values(t, s, pts):
    """Each object's own binary32 value d·scaleFactor at every point (one-object oracle tables), NaN where it is not below 1e6."""
    vals = []
    for o in t.objects[:t.num_objects]:
        r = oracle(tables([o], t.globals_), s, pts)
        vals.append(np.where(r[:, 1] == 0, r[:, 0], np.nan))
    return np.stack(vals, axis=1)


def test_table_walk_variants_with_valid_bounds(R):
    rng = np.random.default_rng(13)
    s = abi.default_settings()
    ones = 0
    exact_lanes = [0]
    for name, objs in _walk_tables(rng):
        g = h.make_globals()
        t = tables(objs, g)
        P = np.concatenate([rng.uniform(-3, 3, (192, 3)), rng.uniform(-0.6, 0.6, (63, 3))]).astype(F32)
        ref = oracle(t, s, P)
        d0 = ref[:, 0]
        inside = d0 <= 0
        ubs = {"exact": d0, "ulp": np.nextafter(d0, F32(np.inf), dtype=F32),
               "margin": (np.abs(d0) * F32(1e-4) + d0 + F32(1e-5)).astype(F32), "inf": np.full_like(d0, np.inf),
               "nan": np.full_like(d0, np.nan), "zero": np.where(inside, F32(0.0), d0).astype(F32),
               "negzero": np.where(inside, F32(-0.0), d0).astype(F32)}
        vals = _single_values(t, s, P)
        for count, trap, skip, track in WALK:
            for ubn, ub in (ubs.items() if skip else [("none", None)]):
                dev = run(R, t, s, P, ub=ub, count=count, trap=trap, skip=skip, track=track)
                what = f"{name} count {count} trap {trap} skip {skip} track {track} ub {ubn}"
                check_against_oracle(dev, ref, trap, what)
                if count == 2 and not skip:
                    assert (dev[:, 7] == t.num_objects).all(), what
                if count == 1:
                    assert (dev[:, 7] == t.num_objects).all(), what
                if track:
                    # the runner-up property the single-object fast path rests on: second <= every other object's value
                    idx = dev[:, 1].astype(int)
                    others = vals.copy()
                    rows = np.flatnonzero(idx >= 0)
                    others[rows, idx[rows]] = np.nan
                    bad = (dev[:, 6:7] > others) & ~np.isnan(others)
                    assert not bad.any(), f"{what}: second above another object's value at {np.flatnonzero(bad.any(axis=1))[:8]}"
                    if count == 2:
                        # and on lanes whose wave passed over nothing, it IS the runner-up: the smallest of the other objects'
                        # values and the initial minimum 1e6 (a walk that put the minimum itself there would still be a bound)
                        full = (dev[:, 7] == t.num_objects) & (idx >= 0) & np.isfinite(vals).all(axis=1)
                        runner = np.minimum(np.nanmin(np.where(np.isnan(others), np.inf, others), axis=1), F32(1e6))
                        assert (dev[full, 6] == runner[full]).all(), f"{what}: second is not the runner-up"
                        exact_lanes[0] += int(full.sum())
        # sdSceneOne: where object j is strictly nearest, it returns the full walk's d and idx
        for j in range(t.num_objects):
            if objs[j].type > abi.RM_RECTANGLE:
                continue
            rest = np.delete(vals, j, axis=1)
            lanes = ~np.isnan(vals[:, j]) & (np.isnan(rest) | (rest > vals[:, j:j + 1])).all(axis=1)
            for count, trap in ((0, 0), (0, 1), (2, 0), (2, 1)):
                dev = run(R, t, s, P, count=count, trap=trap, skip=1, track=1, one=j)
                assert (dev[:, 1] == j).all() and (dev[:, 7] == (1.0 if count else 0.0)).all()
                assert (bits(dev[lanes, 0]) == bits(ref[lanes, 0])).all(), f"{name}: sdSceneOne({j}) differs from the walk"
                assert (ref[lanes, 1] == j).all()
            ones += int(lanes.sum())
    assert ones > 1000, ones
    assert exact_lanes[0] > 1000, exact_lanes


def test_skip_shell_waves_pass_over_exactly_when_predicted(R):
    """A cube at the origin, then sphere K at c (scale 2^k: its transform is exact in binary32), points on the axis line from c
    towards the cube.  Every lane's minimum is the cube's value dA, so after the cube the walk's bound is dA whatever valid ub
    came in, and K's pass-over test is far = |p_K|² > RN(RN(lim²)·1.00003) with lim = RN(dA·2^-k + boundR): computed here in
    binary32 exactly as the device does (ub comes in as the exact minimum, a few ulp above it, +inf or NaN: the walk's
    min_(ub, cur) after the cube makes it dA in every case).  Waves of 64 lanes within a few ulp of that threshold, on one side or straddling it:
    the shapes counter (COUNT 2) must say "passed over" exactly on the waves whose every lane is far — including a far wave
    with one near lane, which must not pass — and every lane must equal the oracle and the walk without SKIP."""
    s = abi.default_settings()
    passed = kept = 0
    for ksc, c, axis, sign in ((1.0, 3.0, 0, 1), (0.5, 2.5, 1, -1), (0.25, 4.0, 2, 1), (2.0, 5.0, 0, -1)):
        cvec = np.zeros(3)
        cvec[axis] = sign * c
        K = h.make_object(abi.RM_SPHERE, model=h.translate(*cvec) @ h.scale(ksc, ksc, ksc), scale_factor=ksc)
        cube = h.make_object(abi.RM_CUBE)
        t = tables([cube, K], h.make_globals())
        inv, boundR, cs = F32(1.0 / ksc), F32(0.5001), F32(sign * c)
        assert K.invModel[5 * axis] == inv and K.invModel[12 + axis] == -cs * inv

        def threshold(P):
            dA = oracle(tables([cube], t.globals_), s, P)[:, 0]
            pK = ((P[:, axis] - cs) * inv).astype(F32)  # K's object coordinate: one rounding, as the device's fma
            lim = (dA * inv + boundR).astype(F32)
            return (pK * pK).astype(np.float64) - ((lim * lim) * F32(1.00003)).astype(np.float64), lim

        # locate the threshold on a coarse line, then take every binary32 coordinate within 300 ulp of it
        line = np.zeros((4000, 3), F32)
        line[:, axis] = (sign * (c - np.linspace(0.3, c - 0.6, 4000))).astype(F32)
        gap, _ = threshold(line)
        k0 = int(np.flatnonzero(np.diff(np.sign(gap)))[0])
        lo, hi = line[k0].copy(), line[k0 + 1].copy()
        for _ in range(60):  # bisection down to neighbouring binary32 coordinates
            mid = lo.copy()
            mid[axis] = F32((np.float64(lo[axis]) + np.float64(hi[axis])) / 2)
            if mid[axis] in (lo[axis], hi[axis]):
                break
            if np.sign(threshold(mid[None])[0][0]) == np.sign(gap[k0]):
                lo = mid
            else:
                hi = mid
        x0 = F32(lo[axis])
        P = np.zeros((301, 3), F32)
        P[:, axis] = [_step(x0, k) for k in range(-150, 151)]
        ref = oracle(t, s, P)
        P, ref = P[ref[:, 1] == 0], ref[ref[:, 1] == 0]  # lanes whose minimum is the cube's (K is nearer a little way in)
        gap, lim = threshold(P)
        far = (lim >= 0) & (gap > 0)
        order = np.argsort(gap, kind="stable")  # nearest first … farthest last
        i0 = int((~far).sum())
        assert 64 <= i0 <= len(P) - 80, (i0, len(P))
        starts = [i0 - 64, i0 - 40, i0 - 32, i0 - 8, i0 - 1, i0, i0 + 16]
        waves = [order[a:a + 64] for a in starts]
        one_near = order[i0:i0 + 64].copy()
        one_near[17] = order[i0 - 1]  # the lane just inside the threshold
        waves += [one_near, order[i0:i0 + 1]]  # and a far lane alone in a partial last wave
        ids = np.concatenate(waves)
        for extra in (0, 1, 3, np.inf, np.nan):  # ub: the exact minimum, a few ulp above it, +inf, NaN
            ub = np.full(len(P), extra, F32) if not np.isfinite(extra) else np.array([_step(v, int(extra)) for v in ref[:, 0]], F32)
            dev = run(R, t, s, P[ids], ub=ub[ids], count=2, trap=1, skip=1, track=1)
            what = f"shell axis {axis} scale {ksc} ub +{extra} ulp"
            check_against_oracle(dev, ref[ids], 1, what)
            plainw = run(R, t, s, P[ids], count=2, trap=1)
            assert (bits(dev[:, :6]) == bits(plainw[:, :6])).all(), what
            for wi, w in enumerate(waves):
                sl = slice(64 * wi, 64 * wi + len(w))
                expect = 1.0 if far[w].all() else 2.0
                assert (dev[sl, 7] == expect).all(), (what, wi, int(far[w].sum()), dev[sl, 7][:4])
                passed += expect == 1.0
                kept += expect == 2.0
    assert passed >= 8 and kept >= 8, (passed, kept)
