"""What the probe-depth test modules share: the stand-alone CPU program of raymarcher_amd/csrc/rm_light_depth.h and of the visible
step of rm_light_grid.h (built under the host sanitizers and run as a program), and the fixtures — the bake's shapes, positions,
tables and weights, and the seeded depth records of light_grid_helpers' three grids."""
import functools
import os
import struct
import subprocess

import numpy as np

import helpers as h
import light_depth_spec as D
import light_grid_helpers as MG
import light_grid_spec as G
import light_probes_helpers as MP
import light_probes_spec as L

f32 = np.float32
CPU_SRC = os.path.join(h.ROOT, "tests", "light_depth_spec", "rm_light_depth_cpu.cpp")
# The bake's shapes.  K = 1: 64 probes per wave, a tree of one leaf.  K = 2: segments of two.  K = 64: one probe per wave, the whole
# serial fold.  K = 128: the smallest that loops — two passes, one pending level.  n = 1: one live segment; n = 3: a non-finite probe
# between two finite ones; n = 65: a second wave at K = 1, a second workgroup from K = 64 on.
DIRS = (1, 2, 64, 128)
PROBES = (1, 3, 65)
SETS = (1, 3)
BIASES = (0.0, 0.1)


def build_cpu_program(directory):
    """g++, the address and undefined-behaviour sanitizers linked in statically, -ffp-contract=off: as light_grid_helpers builds its own."""
    exe = os.path.join(str(directory), "rm_light_depth_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
           "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, directory, mode, query, size, dtype, n):
    src, dst = os.path.join(str(directory), f"{mode}_query.bin"), os.path.join(str(directory), f"{mode}_result.bin")
    with open(src, "wb") as f:
        f.write(query)
    r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == size * n
    return np.frombuffer(raw, dtype, n)


def run_cpu_bake(exe, directory, positions, table, weights, K, sets, t):
    """positions (n, 4), table (sets·K, 16), weights (sets·K, 64), t (n·K) float32 → DEPTH records (n) of the program."""
    positions, table = np.ascontiguousarray(positions, f32), np.ascontiguousarray(table, f32)
    weights, t = np.ascontiguousarray(weights, f32), np.ascontiguousarray(t, f32)
    n = len(positions)
    assert positions.shape == (n, 4) and table.shape == (sets * K, 16) and weights.shape == (sets * K, 64) and t.shape == (n * K,)
    query = struct.pack("<3i", n, K, sets) + positions.tobytes() + table.tobytes() + weights.tobytes() + t.tobytes()
    return _run(exe, directory, "bake", query, 512, D.DEPTH, n)


def run_cpu_look(exe, directory, probes, depth, dims, origin, step, points, normals, facing, normal_bias):
    """PROBE and DEPTH records, the grid, points and normals (n, 4) float32 → GRIDLIGHT records (n) of the program."""
    points, normals = np.ascontiguousarray(points, f32), np.ascontiguousarray(normals, f32)
    probes, depth = np.ascontiguousarray(probes), np.ascontiguousarray(depth)
    n = len(points)
    assert points.shape == (n, 4) and normals.shape == (n, 4) and probes.dtype == G.PROBE and depth.dtype == D.DEPTH
    query = (struct.pack("<5i", *(int(d) for d in dims), n, G.FACING if facing else 0) + np.asarray(origin, f32).tobytes() +
             np.asarray(step, f32).tobytes() + f32(normal_bias).tobytes() + probes.tobytes() + depth.tobytes() + points.tobytes() +
             normals.tobytes())
    return _run(exe, directory, "look", query, 32, G.GRIDLIGHT, n)


# ---------------------------------------------------------------- the bake's fixture
def bake_positions(centre, radius, n, seed):
    """n seeded probe positions in and around a ball → float32 (n, 4), w = junk that is not read; from three probes on ONE has a
    non-finite coordinate, neither first nor last."""
    rng = np.random.default_rng(8100 + seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = np.zeros((n, 4), f32)
    p[:, 0:3] = np.asarray(centre) + u * (rng.uniform(0.2, 1.6, (n, 1)) * radius)
    p[:, 3] = rng.uniform(-5, 5, n)
    if n >= 3:
        p[n // 2, rng.integers(0, 3)] = f32(np.nan) if n == 3 else f32(np.inf)
        assert L.valid_positions(p).sum() == n - 1 and L.valid_positions(p[[0, -1]]).all()
    return p


tables = MP.tables  # rm_sphere_directions' with a zero and a NaN row; a table of one or two rows also with its rows bad


def seeded_weights(K, sets, seed):
    """float32 (sets·K, 64): finite weights of both signs, denormals, values around the smallest normal, zeros of either sign."""
    rng = np.random.default_rng(8300 + 17 * K + sets + seed)
    w = rng.uniform(-1, 1, (sets * K, 64)).astype(f32)
    kind = rng.integers(0, 12, w.shape)
    w[kind == 0] *= f32(1e-38)
    w[kind == 1] = f32(1e-42)
    w[kind == 2] = f32(-0.0)
    w[kind == 3] = f32(0.0)
    return w


# ---------------------------------------------------------------- the lookup's fixture
@functools.lru_cache(maxsize=None)
def depth_records(name, far=False):
    """The seeded depth records of grid `name` (light_grid_helpers.GRIDS) → read-only DEPTH (nx·ny·nz).  Means and mean squares
    around the grid's step, so that points lie on both sides of them: of both signs, some denormal, some with m2 < m², some with
    m2 = m² exactly (no variance), some zeros; the invalid probe's words are NaN.  far: every mean is 1e30, above every r of the
    fixture's finite points but those at ±3e38, mean squares 1e35."""
    dims, _, step, bad, _ = MG.GRIDS[name]
    count = int(np.prod(dims))
    rng = np.random.default_rng(9400 + sorted(MG.GRIDS).index(name))
    rec = np.zeros(count, D.DEPTH)
    if far:
        rec["moments"][:, :, 0], rec["moments"][:, :, 1] = f32(1e30), f32(1e35)
    else:
        scale = float(np.linalg.norm(np.asarray(step, np.float64)))
        m = rng.uniform(0.05, 1.2, (count, 64)).astype(f32) * f32(scale)
        spread = rng.uniform(0.0, 0.3, (count, 64)).astype(f32) * f32(scale)
        m2 = m * m + spread * spread
        kind = rng.integers(0, 16, (count, 64))
        m2[kind == 0] = (m * m)[kind == 0]                       # no variance
        m2[kind == 1] = (m * m)[kind == 1] * f32(0.5)            # m2 < m²
        m[kind == 2] = -m[kind == 2]                             # a negative mean
        m[kind == 3], m2[kind == 3] = f32(1e-42), f32(1e-43)     # denormals
        m[kind == 4], m2[kind == 4] = f32(0.0), f32(-0.0)
        m2[kind == 5] = -m2[kind == 5]
        rec["moments"][:, :, 0], rec["moments"][:, :, 1] = m, m2
    rec["moments"][bad] = f32(np.nan)
    rec.setflags(write=False)
    return rec
