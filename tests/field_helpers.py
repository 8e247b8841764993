"""What the lattice-query tests share (rm_sdf_sample, rm_sdf_sample_blocks, rm_sdf_trace, rm_sdf_trace_blocks): the lattices, the
points and rays that reach every branch of the definition, and the CPU program that runs the library's own arithmetic
(tests/field_spec/rm_field_cpu.cpp over raymarcher_amd/csrc/rm_field_march.h) under the host sanitizers."""
import functools
import os
import struct
import subprocess

import numpy as np

import field_spec as F
import sdf_blocks_helpers as K
import sdf_blocks_spec as B
import sdf_helpers as V

f32 = np.float32
CPU_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "field_spec", "rm_field_cpu.cpp")
NUM = 4099  # points and rays per case: not a multiple of 64, seventeen workgroups

DENSE_ISO = {"sphere_cube": 0.0, "menger": 0.0, "bulb_plain": 0.001}
DENSE_DIMS = ((17, 13, 9), (33, 25, 17))
DENSE_CASES = [f"{t}_{d[0]}x{d[1]}x{d[2]}" for t in DENSE_ISO for d in DENSE_DIMS]
HANDMADE_DENSE = ("iso_ties_4x4x4", "nonfinite_3x5x4", "infinities_4x4x4")
BLOCK_CASES = ("sphere_25", "menger_33", "bulb_33", "nonfinite_17x9x9", "iso_ties_9")  # 3×2×2, 4×4×4, 2×1×1 and 1×1×1 blocks


def _readonly(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def dense_case(name):
    """(dist (nz, ny, nx), ids or None, origin, step, iso) of a dense case: the oracle's sdScene, or hand-made values."""
    if name in HANDMADE_DENSE:
        return V.handmade()[name]
    table, dims = name.rsplit("_", 1)
    dims = tuple(int(d) for d in dims.split("x"))
    dist, ids, origin, step = V.oracle_lattice(table, dims)
    return dist, ids, origin, step, DENSE_ISO[table]


@functools.lru_cache(maxsize=None)
def sphere_lattice(n, radius=0.5, half=0.8):
    """|p| − radius on n³ points across the box ±half → (dist, origin, step), float32."""
    origin = np.full(3, -half, f32)
    step = np.full(3, f32(2 * half / (n - 1)), f32)
    x = origin[0] + np.arange(n, dtype=f32) * step[0]
    z, y, xx = np.meshgrid(x, x, x, indexing="ij")
    dist = (np.sqrt(xx.astype(np.float64) ** 2 + y.astype(np.float64) ** 2 + z.astype(np.float64) ** 2) - radius).astype(f32)
    return _readonly(dist, origin, step)


def block_lists(dense, iso):
    """label → int32 (n, 4): every block, the specification's active blocks, the shuffled list with voids and duplicates, none."""
    blocks = B.blocks_of(dense)
    return {"full": B.all_blocks(blocks), "active": B.active_blocks(dense, iso), "messy": K.messy_list(blocks),
            "empty": np.zeros((0, 4), np.int32)}


# ---------------------------------------------------------------- points and rays
def _world(origin, step, u):
    """origin + u · step in float32, u in lattice units."""
    return (origin + np.asarray(u, f32) * step).astype(f32)


def points_for(dist, origin, step, n=NUM, seed=3):
    """float32 (n, 4): random in and around the box, exactly on lattice points, on the box's faces (u = 0 and u = N), on block
    faces (multiples of 8), non-finite.  w holds a NaN: it is not read."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = dist.shape
    N = np.array([nx - 1, ny - 1, nz - 1], np.int64)
    parts = [_world(origin, step, rng.uniform(-0.25, 1.25, (n, 3)) * N)]
    on = rng.integers(0, N + 1, (600, 3))
    parts.append(_world(origin, step, on))
    face = rng.uniform(0, 1, (600, 3)) * N
    axis, side = rng.integers(0, 3, 600), rng.integers(0, 2, 600)
    face[np.arange(600), axis] = np.where(side == 1, N[axis], 0)
    parts.append(_world(origin, step, face))
    blockface = rng.uniform(0, 1, (400, 3)) * N
    axis = rng.integers(0, 3, 400)
    blockface[np.arange(400), axis] = np.minimum(8 * rng.integers(0, 4, 400), N[axis])
    parts.append(_world(origin, step, blockface))
    parts.append(_world(origin, step, np.array([N, N * [1, 0, 1], [0, 0, 0], N * [0, 1, 0]])))  # corners: u = N on every axis
    bad = _world(origin, step, rng.uniform(0, 1, (12, 3)) * N)
    for r, v in enumerate((np.nan, np.inf, -np.inf) * 4):
        bad[r, r % 3] = v
    parts.append(bad)
    p = np.concatenate(parts)
    p = p[rng.permutation(len(p))[:n]] if len(p) > n else p
    p[:12] = bad  # the permutation may not drop them
    out = np.full((len(p), 4), np.nan, f32)
    out[:, :3] = p
    assert len(out) == n
    return out


def rays_for(dist, origin, step, iso, n=NUM, seed=4):
    """float32 (n, 8) rows of RmRay: from outside aimed at the box, from inside the box, from inside the surface, from exactly on a
    face, axis-parallel inside and outside the slabs, missing the box, tMax shorter than the entry, tMax = +inf, invalid."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = dist.shape
    N = np.array([nx - 1, ny - 1, nz - 1], np.float64)
    lo, hi = origin.astype(np.float64), origin + N * step
    mid, half = (lo + hi) / 2, (hi - lo) / 2
    radius = float(np.linalg.norm(half))

    def sphere_dirs(k):
        d = rng.normal(size=(k, 3))
        return d / np.linalg.norm(d, axis=1)[:, None]

    def rows(o, d, tmax):
        r = np.zeros((len(o), 8), f32)
        r[:, 0:3], r[:, 3], r[:, 4:7] = o, tmax, d
        r[:, 7] = f32(np.nan)  # reserved: not read
        return r

    parts = []
    k = n // 4  # from outside, aimed at targets in the box; a third of them with a dir that is not unit
    o = mid + sphere_dirs(k) * radius * rng.uniform(1.2, 3.0, (k, 1))
    d = (lo + rng.uniform(0, 1, (k, 3)) * (hi - lo)) - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    d[::3] *= rng.uniform(0.3, 2.5, (len(d[::3]), 1))
    parts.append(rows(o, d, 100.0))
    k = n // 6  # from inside the box
    parts.append(rows(lo + rng.uniform(0, 1, (k, 3)) * (hi - lo), sphere_dirs(k), 50.0))
    with np.errstate(invalid="ignore"):
        inside = np.argwhere(dist < f32(iso))[:, ::-1]  # (i, j, k) of lattice points below iso
    if len(inside):  # from inside the surface
        pick = inside[rng.integers(0, len(inside), n // 12)]
        parts.append(rows(_world(origin, step, pick), sphere_dirs(len(pick)), 50.0))
    k = n // 12  # from exactly on a face of the box, inwards and outwards
    u = rng.uniform(0, 1, (k, 3)) * N
    axis, side = rng.integers(0, 3, k), rng.integers(0, 2, k)
    u[np.arange(k), axis] = np.where(side == 1, N[axis], 0)
    parts.append(rows(_world(origin, step, u), sphere_dirs(k), 50.0))
    k = n // 8  # axis-parallel: two components of dir are zero; origins inside and outside the other two slabs
    o = lo + rng.uniform(-0.3, 1.3, (k, 3)) * (hi - lo)
    d = np.zeros((k, 3))
    d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0, 0.5, -2.0], k)
    d[::7] = np.where(d[::7] == 0, -0.0, d[::7])  # negative zeros are zeros
    parts.append(rows(o, d, 50.0))
    k = n // 16  # one zero component
    d = sphere_dirs(k)
    d[np.arange(k), rng.integers(0, 3, k)] = 0.0
    parts.append(rows(lo + rng.uniform(-0.3, 1.3, (k, 3)) * (hi - lo), d, 50.0))
    k = n // 16  # pointing away from the box
    dirs = sphere_dirs(k)
    parts.append(rows(mid + dirs * radius * 1.5, dirs, 50.0))
    k = n // 16  # tMax shorter than the way to the box, and tMax = 0
    dirs = sphere_dirs(k)
    parts.append(rows(mid - dirs * radius * 2.0, dirs, np.where(rng.uniform(size=k) < 0.2, 0.0, 0.3 * radius)))
    k = n // 16  # tMax = +inf
    dirs = sphere_dirs(k)
    parts.append(rows(mid - dirs * radius * rng.uniform(0.0, 2.0, (k, 1)), dirs, np.inf))
    bad = rows(np.tile(mid, (10, 1)), np.tile([0.0, 0.0, 1.0], (10, 1)), 10.0)
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    bad[3, 4], bad[4, 5], bad[5, 6] = np.nan, np.inf, -np.inf
    bad[6, 4:7] = 0.0
    bad[7, 4:7] = (-0.0, 0.0, -0.0)
    bad[8, 3], bad[9, 3] = np.nan, -1.0
    parts.append(bad)
    r = np.concatenate(parts)
    fill = n - len(r)
    assert fill >= 0
    o = lo + rng.uniform(-0.5, 1.5, (fill, 3)) * (hi - lo)
    r = np.concatenate([r, rows(o, sphere_dirs(fill) * rng.uniform(0.5, 1.5, (fill, 1)), 30.0)])
    r = r[rng.permutation(n)]
    return np.ascontiguousarray(r, f32)


# ---------------------------------------------------------------- the library's arithmetic on the CPU
def build_cpu_program(directory):
    """As sdf_helpers.build_cpu_program builds its twin: g++, the address and undefined-behaviour sanitizers linked in statically,
    -ffp-contract=off."""
    exe = os.path.join(str(directory), "rm_field_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, dist, ids, origin, step, iso, points, rays, max_steps, normals=True, block_list=None, blocks=None):
    """dist: the dense lattice (nz, ny, nx), or with block_list the packed slots (n, 9, 9, 9) → (SAMPLE records, HIT records)."""
    sparse = block_list is not None
    dims = blocks if sparse else dist.shape[::-1]
    nb = len(block_list) if sparse else 0
    src, dst = os.path.join(str(directory), "query.bin"), os.path.join(str(directory), "result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<10i", int(sparse), dims[0], dims[1], dims[2], nb, 0 if ids is None else 1, len(points), len(rays), max_steps,
                            0 if normals else 1))
        f.write(np.asarray(origin, f32).tobytes() + np.asarray(step, f32).tobytes() + f32(iso).tobytes())
        if sparse:
            f.write(np.ascontiguousarray(block_list, np.int32).tobytes())
        f.write(np.ascontiguousarray(dist, f32).tobytes())
        if ids is not None:
            f.write(np.ascontiguousarray(ids, np.int32).tobytes())
        f.write(np.ascontiguousarray(points, f32).tobytes() + np.ascontiguousarray(rays, f32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 32 * (len(points) + len(rays))
    return np.frombuffer(raw, F.SAMPLE, len(points)), np.frombuffer(raw, F.HIT, len(rays), 32 * len(points))


def assert_records_equal(got, want, what):
    """SAMPLE or HIT record arrays equal in every bit (field_spec.as_words: a NaN equals any NaN); the message shows the first rows
    that differ."""
    got, want = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1)
    g, w = F.as_words(got), F.as_words(want)
    assert got.dtype == want.dtype and g.shape == w.shape, f"{what}: {got.dtype} {g.shape} against {want.dtype} {w.shape}"
    bad = (g != w).any(axis=1)
    if bad.any():
        detail = "; ".join(f"row {r}: got {got[r]} want {want[r]}" for r in np.nonzero(bad)[0][:3])
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(g)} records differ; {detail}")
