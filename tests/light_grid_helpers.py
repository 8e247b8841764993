"""What the rm_light_grid_irradiance test modules share: the stand-alone CPU program of raymarcher_amd/csrc/rm_light_grid.h (built
under the host sanitizers and run as a program), and the fixture — the three grids, their seeded probe records with one invalid
probe whose coefficients are NaN, and the points with their edge cases."""
import functools
import os
import struct
import subprocess

import numpy as np

import helpers as h
import light_grid_spec as G

f32 = np.float32
CPU_SRC = os.path.join(h.ROOT, "tests", "light_grid_spec", "rm_light_grid_cpu.cpp")
# name → (dims, origin, step, index of the invalid probe, its hits).  One cell; a grid where a stride mistake shows (nx != ny != nz);
# an anisotropic step — 0.5 and 0.25 also make u of a coordinate of 3e38 infinite — and a negative origin.  The third grid's invalid
# probe has hits = −1: a probe is valid iff hits >= 0, whatever the negative value.
GRIDS = {
    "one_cell": ((2, 2, 2), (0.0, -0.5, 1.0), (1.0, 1.0, 1.0), 5, G.INVALID),
    "strides": ((3, 2, 4), (0.25, 0.5, -1.0), (0.75, 0.75, 0.75), 10, G.INVALID),
    "anisotropic": ((5, 4, 3), (-2.0, -1.5, -0.75), (0.5, 0.25, 1.5), 27, -1),
}
COUNTS = (1, 64, 65, 257)  # one lane, a full wave, a wave with one live lane, a second workgroup


def build_cpu_program(directory):
    """g++, the address and undefined-behaviour sanitizers linked in statically, -ffp-contract=off: as light_probes_helpers builds its own."""
    exe = os.path.join(str(directory), "rm_light_grid_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, probes, dims, origin, step, points, normals, facing):
    """PROBE records, the grid, points and normals (n, 4) float32 → GRIDLIGHT records (n) of the program."""
    points, normals = np.ascontiguousarray(points, f32), np.ascontiguousarray(normals, f32)
    probes = np.ascontiguousarray(probes)
    n = len(points)
    assert points.shape == (n, 4) and normals.shape == (n, 4) and probes.dtype == G.PROBE
    src, dst = os.path.join(str(directory), "grid_query.bin"), os.path.join(str(directory), "grid_result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<5i", *(int(d) for d in dims), n, G.FACING if facing else 0))
        f.write(np.asarray(origin, f32).tobytes() + np.asarray(step, f32).tobytes())
        f.write(probes.tobytes() + points.tobytes() + normals.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 32 * n
    return np.frombuffer(raw, G.GRIDLIGHT, n)


# ---------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def records(name, all_invalid=False):
    """The seeded probe records of grid `name` → read-only PROBE (nx·ny·nz): finite coefficients of both signs, some denormal, some
    zeros of either sign, hits in 0 … 255, `reserved` junk that is not read; ONE invalid probe whose forty-odd other words are NaN.
    all_invalid: every probe is that."""
    dims, _, _, bad, code = GRIDS[name]
    count = int(np.prod(dims))
    rng = np.random.default_rng(4100 + sorted(GRIDS).index(name))
    rec = np.zeros(count, G.PROBE)
    sh = rng.uniform(-2, 2, (count, 9, 4)).astype(f32)
    kind = rng.integers(0, 12, (count, 9, 4))
    sh[kind == 0] *= f32(1e-38)   # around the smallest normal: denormal products
    sh[kind == 1] = f32(1e-42)    # denormal themselves
    sh[kind == 2] = f32(-0.0)
    sh[kind == 3] = f32(0.0)
    rec["sh"], rec["hits"] = sh, rng.integers(0, 256, count)
    rec["reserved"] = rng.integers(-5, 5, (count, 3))
    which = np.arange(count) if all_invalid else np.array([bad])
    rec["sh"][which] = f32(np.nan)
    rec["hits"][which] = code
    rec["reserved"][which] = 0x7FC00000
    assert np.isfinite(rec["sh"][rec["hits"] >= 0]).all() and (rec["hits"] < 0).sum() == len(which)
    rec.setflags(write=False)
    return rec


def _unit(rng, m):
    v = rng.normal(size=(m, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


@functools.lru_cache(maxsize=None)
def points(name, n):
    """The points and normals of grid `name` for a call of n points → two read-only float32 (n, 4), w = junk that is not read (a NaN
    and an infinity).  Seeded points in and around the box with unit normals; from 64 points on, behind the first point: points
    exactly on probes (the invalid one among them), on faces and on edges of cells; outside the box on every side and beyond a
    corner; at +3e38 and −3e38 along one axis (unit normals there: the facing term overflows to a clean infinity, not to a NaN); a
    −0 coordinate; a NaN and an infinite position, a zero and a NaN normal — neither first nor last —; normals of length 2.5 and
    0.01.  A call of one point has one good point."""
    dims, origin, step, bad, _ = GRIDS[name]
    rng = np.random.default_rng(5200 + 7 * n + sorted(GRIDS).index(name))
    pos = G.positions(origin, step, dims)
    lo, hi = pos[0], pos[-1]
    side = hi - lo
    p = np.zeros((n, 4), f32)
    v = np.zeros((n, 4), f32)
    p[:, 0:3] = lo + rng.uniform(-0.3, 1.3, (n, 3)).astype(f32) * side
    v[:, 0:3] = _unit(rng, n)
    p[:, 3], v[:, 3] = f32(np.nan), f32(np.inf)
    if n >= 64:
        s = np.asarray(step, f32)
        inside = lambda: lo + rng.uniform(0.1, 0.9, 3).astype(f32) * side  # noqa: E731
        special = [pos[0], pos[-1], pos[bad], pos[len(pos) // 2]]                                      # on probes
        for a in range(3):                                                                             # on a face, then on an edge
            q = inside(); q[a] = pos[bad][a]; special.append(q)
            q = inside(); q[a], q[(a + 1) % 3] = pos[-1][a], pos[0][(a + 1) % 3]; special.append(q)
        for a in range(3):                                                                             # outside, every side
            for sign in (-1, 1):
                q = inside(); q[a] = (lo[a] - f32(1.3) * s[a]) if sign < 0 else (hi[a] + f32(2.7) * s[a]); special.append(q)
        special.append(hi + s * f32(3.0))                                                              # beyond a corner
        special.append(lo - s * f32(0.5))
        q = inside(); q[0] = f32(3e38); special.append(q)
        q = inside(); q[1] = f32(-3e38); special.append(q)
        q = inside(); q[0] = f32(-0.0); special.append(q)
        k = len(special)
        assert 1 + k + 6 < 64
        p[1:1 + k, 0:3] = np.array(special, f32)
        at = 1 + k
        p[at, 1] = f32(np.nan)
        p[at + 1, 2] = f32(-np.inf)
        v[at + 2, 0:3] = (0.0, -0.0, 0.0)
        v[at + 3, 2] = f32(np.nan)
        v[at + 4, 0:3] *= f32(2.5)
        v[at + 5, 0:3] *= f32(0.01)
        assert (~G.valid_points(p, v)).sum() == 4 and G.valid_points(p[:1], v[:1]).all() and G.valid_points(p[-1:], v[-1:]).all()
    else:
        assert G.valid_points(p, v).all()
    p.setflags(write=False)
    v.setflags(write=False)
    return p, v
