"""rm_probe_bump — the device function the production kernels call for bumpNormal's four Perlin samples — against values built
from the oracle's pnoise, word for word.  The function takes an offset sample from the base sample's lattice when every lane of
the wave stays in its cell on that axis and from pnoise itself otherwise, so the waves here are built lane by lane (point i runs
on lane i % 64 of wave i / 64): nobody crossing, everybody crossing, one lane crossing, the knife edge of the float32 sum, the
mod-256 wrap, absorbed offsets, zeros, denormals and non-finite lanes.

The expected words are exact: ps = pos * float32(10), ps_k + float32(0.1) (the other two + float32(0)) and the float32 difference
are one IEEE operation each in numpy, and pnoise is the oracle's (the function tests/test_gpu_parity.py holds RM_FN_PNOISE3 to).
"""
import numpy as np
import pytest

import helpers as h
from raymarcher_amd import abi

pytestmark = pytest.mark.gpu

F = np.float32
TENTH = F(0.1)


def scaled(p):
    return (p.astype(F) * F(10)).astype(F)


def crossing(p):
    """(n, 3) bool: floor(ps_k + 0.1f) != floor(ps_k) with the float32 sum."""
    ps = scaled(p)
    return np.floor((ps + TENTH).astype(F)) != np.floor(ps)


def oracle_pnoise(q):
    q = np.ascontiguousarray(q, dtype=F)
    x, y, z = (np.ascontiguousarray(q[:, i]) for i in range(3))
    out = np.empty(len(q), dtype=F)
    assert h.oracle().rmo_probe_math(abi.RM_FN_PNOISE3, h.fptr(x), h.fptr(y), h.fptr(z), h.fptr(out), len(q)) == 0
    return out


def expected(p):
    """(n, 4): nv, g0, g1, g2 as bumpNormal forms them."""
    ps = scaled(p)
    with np.errstate(invalid="ignore", over="ignore"):
        nv = oracle_pnoise(ps)
        out = [nv]
        for k in range(3):
            off = np.zeros(3, dtype=F)
            off[k] = TENTH
            out.append((oracle_pnoise((ps + off).astype(F)) - nv).astype(F))
    return np.stack(out, axis=1)


def find_p(target):
    """A float32 p with float32(p * 10) == target, or None (10 p skips some values where its ulp is 1.25 steps of p)."""
    p = F(F(target) / F(10))
    lo = hi = p
    for _ in range(6):
        for q in (lo, hi):
            if F(q * F(10)) == F(target) and np.signbit(F(q * F(10))) == np.signbit(F(target)):
                return q
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
    return None


class Pools:
    """Points of [-30, 30]^3 that cross on exactly the axes of a mask (bit k: axis k crosses): the fraction of 10 p is drawn from
    [0.92, 0.98] on a crossing axis and from [0.05, 0.85] on the others, and crossing() has the last word."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)

    def take(self, mask, n):
        want = np.array([(mask >> k) & 1 for k in range(3)], dtype=bool)
        cell = self.rng.integers(-300, 300, (4 * n + 16, 3))
        frac = np.where(want, self.rng.uniform(0.92, 0.98, cell.shape), self.rng.uniform(0.05, 0.85, cell.shape))
        p = ((cell + frac) / 10.0).astype(F)
        p = p[(crossing(p) == want).all(axis=1)]
        assert len(p) >= n, f"pool {mask} too small"
        return p[:n]


def build():
    """→ (points (n, 3), {name: (first point, count, lanes whose words are compared as numbers-or-NaN only)})."""
    pools = Pools(11)
    rng = np.random.default_rng(12)
    segs, names = [], {}

    def add(name, pts, loose=()):
        pts = np.ascontiguousarray(pts, dtype=F)
        assert pts.shape == (64, 3) or name == "partial last wave", (name, pts.shape)
        names[name] = (sum(len(s) for s in segs), len(pts), tuple(loose))
        segs.append(pts)

    add("no lane crossing", pools.take(0, 64))
    for k, ax in enumerate("xyz"):
        add(f"every lane crossing on {ax}", pools.take(1 << k, 64))
    for lane in (0, 31, 63):
        for k, ax in enumerate("xyz"):
            w = pools.take(0, 64).copy()
            w[lane] = pools.take(1 << k, 1)[0]
            add(f"lane {lane} alone crossing on {ax}", w)
    add("mixed axes", np.concatenate([pools.take(m, 8) for m in range(8)]))
    add("all axes crossing", pools.take(7, 64))
    neg = np.concatenate([-np.abs(pools.take(0, 40)), -np.abs(pools.take(1, 8)), -np.abs(pools.take(2, 8)), -np.abs(pools.take(4, 8))])
    add("negative coordinates", neg)

    # the knife edge of the float32 sum: 10 p an exact integer; 10 p = n - 0.1f exactly, and one ulp either side of it
    ints, edges = [], []
    for n in list(range(-300, 301, 7)) + [0, 1, -1, 255, 256, -256, -255]:
        q = find_p(F(n))
        if q is not None:
            ints.append(q)
        t = F(F(n) - TENTH)
        for cand in (t, np.nextafter(t, F(-np.inf)), np.nextafter(t, F(np.inf))):
            q = find_p(cand)
            if q is not None:
                edges.append(q)
    assert len(ints) >= 32 and len(edges) >= 96, (len(ints), len(edges))
    ints, edges = np.array(ints, dtype=F), np.array(edges, dtype=F)
    for k, ax in enumerate("xyz"):
        w = pools.take(0, 64).copy()
        w[:32, k] = ints[rng.permutation(len(ints))[:32]]
        w[32:, (k + 1) % 3] = ints[rng.permutation(len(ints))[:32]]
        add(f"exact integers on {ax}", w)
        w = pools.take(0, 64).copy()
        w[:, k] = edges[rng.permutation(len(edges))[:64]]
        add(f"integer - 0.1f and its neighbours on {ax}", w)
    w = np.stack([edges[rng.permutation(len(edges))[:64]] for _ in range(3)], axis=1)
    add("integer - 0.1f on all axes", w)

    # the wrap of mod(., 256): cells 255 -> 0 (p around 25.6) and -1 -> -256 (p around -0.005 and around -25.6)
    for k, ax in enumerate("xyz"):
        w = pools.take(0, 64).copy()
        w[:22, k] = rng.uniform(25.585, 25.605, 22)
        w[22:44, k] = rng.uniform(-25.605, -25.585, 22)
        w[44:, k] = rng.uniform(-0.015, 0.005, 20)
        add(f"mod 256 wrap on {ax}", w)
    w = np.concatenate([rng.uniform(25.58, 25.6, (32, 3)), rng.uniform(-25.61, -25.59, (32, 3))])
    add("mod 256 wrap, one side per half wave", w)

    # ps >= 2^21, ps <= -2^22: + 0.1f is absorbed (the sum lands in a binade of ulp 0.25 and more)
    big = rng.uniform(2.0 ** 22 / 10, 2.0 ** 24, (64, 3)) * rng.choice([-1.0, 1.0], (64, 3))
    big[:8] = [[209715.2, 1.0, 2.0], [-419430.4, 1.0, 2.0], [1e6, -1e6, 1e6], [1e7, 1e7, -1e7], [3e5, 0.5, -3e5], [1e30, 0.3, 0.2],
               [0.3, -1e30, 0.2], [1e9, 1e12, 1e20]]
    add("offset absorbed", big)
    w = pools.take(0, 64).copy()
    w[5] = [4e5, 0.25, -0.75]
    w[40] = [0.1, -2.5e6, 1e30]
    add("absorbed lanes in an ordinary wave", w)

    zeros = pools.take(0, 64).copy()
    tiny = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, 1e-39]
    for i, t in enumerate(tiny):
        zeros[i, i % 3] = t
        zeros[10 + i] = [t, -t, t]
        zeros[20 + i] = [tiny[(i + 1) % 10], t, tiny[(i + 3) % 10]]
    add("zeros and denormals", zeros)

    for name, v in (("NaN", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for lane, k in ((17, 0), (0, 1), (63, 2)):
            w = pools.take(0, 64).copy()
            w[lane, k] = v
            add(f"a {name} lane (lane {lane}, axis {'xyz'[k]})", w, loose=(lane,))
    w = pools.take(0, 64).copy()
    w[9] = [3.4e38, 0.0, 0.0]  # finite p, 10 p overflows
    add("10 p overflows on one lane", w, loose=(9,))

    add("random 1", rng.uniform(-30, 30, (64, 3)))
    rnd = rng.uniform(-30, 30, (64 * 60, 3)).astype(F)
    first_rnd = sum(len(s) for s in segs)
    segs.append(rnd)
    add("partial last wave", np.concatenate([pools.take(0, 20), pools.take(2, 1), pools.take(0, 16)]))
    pts = np.concatenate(segs)
    names["random points"] = (first_rnd, len(rnd), ())
    return pts, names


@pytest.fixture(scope="module")
def case(renderer):
    import torch
    pts, names = build()
    n = len(pts)
    assert n % 64 == 37  # the last wave is partial
    # poisoned rows behind the n the probe is given: it writes 4 n floats and nothing past them
    buf = torch.full((n + 64, 4), float("nan"), dtype=torch.float32, device=renderer.device)
    poison = buf[n:].clone()
    got = renderer.probe_bump(torch.from_numpy(pts).to(renderer.device), out=buf[:n]).cpu().numpy()
    assert torch.equal(buf[n:].view(torch.int32), poison.view(torch.int32)), "rm_probe_bump wrote past 4 n floats"
    return pts, names, got, expected(pts)


def test_the_waves_are_what_their_names_say():
    pts, names = build()
    c = crossing(pts)

    def wave(name):
        a, n, _ = names[name]
        return c[a:a + n]
    assert not wave("no lane crossing").any()
    for k, ax in enumerate("xyz"):
        w = wave(f"every lane crossing on {ax}")
        assert w[:, k].all() and not np.delete(w, k, axis=1).any()
        for lane in (0, 31, 63):
            w = wave(f"lane {lane} alone crossing on {ax}")
            assert w.sum() == 1 and w[lane, k]
        # the knife edge holds lanes on both sides of it
        w = wave(f"integer - 0.1f and its neighbours on {ax}")[:, k]
        assert 8 <= w.sum() <= 56
        assert not wave(f"exact integers on {ax}")[:32, k].any()
        w = wave(f"mod 256 wrap on {ax}")[:, k]
        assert w[:22].any() and w[22:44].any() and w[44:].any() and not w.all()
    assert wave("all axes crossing").all()
    w = wave("mixed axes")
    assert all(0 < w[:, k].sum() < 64 for k in range(3))
    a, n, _ = names["offset absorbed"]
    ps = scaled(pts[a:a + n])
    far = (ps >= 2.0 ** 21) | (ps <= -2.0 ** 22)
    assert far.any(axis=1).all() and ((ps + TENTH).astype(F) == ps)[far].all() and not wave("offset absorbed")[far].any()
    a, n, _ = names["negative coordinates"]
    assert (pts[a:a + n] < 0).all() and c[a:a + n].any() and not c[a:a + n].all(axis=0).any()
    a, n, _ = names["partial last wave"]
    assert n == 37 and a + n == len(pts) and c[a:a + n].sum() == 1
    a, n, _ = names["random points"]
    r = c[a:a + n].reshape(-1, 64, 3)
    assert n >= 3000 and (~r.any(axis=1)).any() and r.any(axis=1).any()  # waves of both kinds among the random ones


def _names():
    return list(build()[1])


@pytest.mark.parametrize("name", _names())
def test_bump_probe_matches_the_oracle(case, name):
    pts, names, got, ref = case
    a, n, loose = names[name]
    g, r = got[a:a + n].view(np.uint32), ref[a:a + n].view(np.uint32)
    strict = np.ones(n, dtype=bool)
    strict[list(loose)] = False
    bad = (g != r).any(axis=1) & strict
    assert not bad.any(), (f"{name}: {bad.sum()} of {n} points differ, first at lane {np.argmax(bad)}: p = {pts[a + np.argmax(bad)]}, "
                           f"device {got[a + np.argmax(bad)]}, oracle {ref[a + np.argmax(bad)]}")
    for lane in loose:  # a non-finite lane: NaN where the oracle has NaN (its payload is not part of the contract), the same words elsewhere
        gn, rn = got[a + lane], ref[a + lane]
        assert (np.isnan(gn) == np.isnan(rn)).all() and (g[lane] == r[lane])[~np.isnan(rn)].all(), (name, lane, gn, rn)
