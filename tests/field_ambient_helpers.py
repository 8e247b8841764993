"""What the rm_field_ambient tests share: the CPU program that runs the library's own arithmetic
(tests/field_ambient_spec/rm_field_ambient_cpu.cpp over raymarcher_amd/csrc/rm_field_ambient.h) under the host sanitizers, and the
FIXTURE — two spheres over a floor on the skip campaign's small box, as a dense lattice and over its active blocks, with about 600
points on the floor, on the spheres and off every surface, their normals, and the edge points."""
import functools
import os
import struct
import subprocess

import numpy as np

import field_ambient_spec as A
import field_handle_helpers as H
import sdf_blocks_spec as B

f32 = np.float32
CPU_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "field_ambient_spec", "rm_field_ambient_cpu.cpp")
BLOCKS = (9, 5, 6)
ISO = 0.001
BIAS = 2.0 / 32.0      # twice the step, the Python layer's default
MAX_DISTANCE = 0.8
MAX_STEPS = 64
CENTRE_1, RADIUS_1 = np.array([0.09, -0.05, 0.07]), 0.22   # campaign_lattice's sphere
CENTRE_2, RADIUS_2 = np.array([0.50, -0.05, -0.08]), 0.15  # beside it, its lowest point 0.07 above the floor
FLOOR = -0.30
NUM_POINTS = 600


# ---------------------------------------------------------------- the library's arithmetic on the CPU
def build_cpu_program(directory):
    """Exactly as field_handle_helpers.build_cpu_program builds its twin: g++, the address and undefined-behaviour sanitizers linked
    in statically, -ffp-contract=off."""
    exe = os.path.join(str(directory), "rm_field_ambient_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, dense, origin, step, points, normals, table, num_dirs, num_sets, bias, max_distance, iso, max_steps,
                    mode, ids=None, block_list=None):
    """dense: the dense lattice (nz, ny, nx); with block_list its packed slots are what the program gets → AMBIENT records."""
    sparse = block_list is not None
    dims = B.blocks_of(dense) if sparse else dense.shape[::-1]
    nb = len(block_list) if sparse else 0
    points = np.ascontiguousarray(points, f32)
    assert points.shape[1] == 4 and (normals is None or normals.shape == points.shape)
    src, dst = os.path.join(str(directory), "ambient_query.bin"), os.path.join(str(directory), "ambient_result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<12i", int(sparse), dims[0], dims[1], dims[2], nb, 0 if ids is None else 1, len(points), 0 if normals is None else 1,
                            num_dirs, num_sets, max_steps, mode))
        f.write(np.asarray(origin, f32).tobytes() + np.asarray(step, f32).tobytes() + np.array([bias, max_distance, iso], f32).tobytes())
        if sparse:
            f.write(np.ascontiguousarray(block_list, np.int32).tobytes())
            f.write(np.ascontiguousarray(B.pack_blocks(dense, block_list, f32(np.nan)), f32).tobytes())
        else:
            f.write(np.ascontiguousarray(dense, f32).tobytes())
        if ids is not None:
            f.write(np.ascontiguousarray(B.pack_blocks(ids, block_list, np.int32(-9)) if sparse else ids, np.int32).tobytes())
        f.write(points.tobytes())
        if normals is not None:
            f.write(np.ascontiguousarray(normals, f32).tobytes())
        f.write(np.ascontiguousarray(table, f32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 32 * len(points)
    return np.frombuffer(raw, A.AMBIENT, len(points))


def assert_records_equal(got, want, what):
    g, w = A.as_words(got), A.as_words(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero((g != w).any(axis=1))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(g)} records differ, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


# ---------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def lattice():
    """(dense, origin, step) on campaign_lattice(BLOCKS)'s box, step 1/32: min(sphere 1, floor z + 0.30, sphere 2) in float64,
    rounded to float32."""
    first, origin, step = H.campaign_lattice(BLOCKS)
    x, y, z = (origin[a].astype(np.float64) + np.arange(8 * m + 1, dtype=np.float64) * np.float64(step[a]) for a, m in enumerate(BLOCKS))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")

    def sphere(c, r):
        return np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) - r

    dense = np.minimum(np.minimum(sphere(CENTRE_1, RADIUS_1), zz - FLOOR), sphere(CENTRE_2, RADIUS_2)).astype(f32)
    assert dense.shape == first.shape
    dense.setflags(write=False)
    return dense, origin, step


@functools.lru_cache(maxsize=None)
def block_list():
    bl = np.ascontiguousarray(B.active_blocks(lattice()[0], ISO), np.int32)
    assert 0 < len(bl) < len(B.all_blocks(BLOCKS))
    bl.setflags(write=False)
    return bl


def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


@functools.lru_cache(maxsize=None)
def points():
    """(points (600, 4), normals (600, 4)) float32: 300 on the floor within 0.4 of the spheres' axes, 120 on each sphere above the
    floor, 60 off every surface with any unit normal.  w holds a NaN: it is not read."""
    rng = np.random.default_rng(41)
    parts, normals = [], []
    k = 300
    axis = np.where(rng.integers(0, 2, k)[:, None] == 0, CENTRE_1[:2], CENTRE_2[:2])
    radius, angle = 0.4 * np.sqrt(rng.uniform(0, 1, k)), rng.uniform(0, 2 * np.pi, k)
    xy = axis + radius[:, None] * np.stack([np.cos(angle), np.sin(angle)], axis=1)
    parts.append(np.concatenate([xy, np.full((k, 1), FLOOR)], axis=1))
    normals.append(np.tile([0.0, 0.0, 1.0], (k, 1)))
    for c, r in ((CENTRE_1, RADIUS_1), (CENTRE_2, RADIUS_2)):
        d = _unit(rng.normal(size=(120, 3)))
        parts.append(c + r * d)
        normals.append(d)
    k = NUM_POINTS - sum(len(p) for p in parts)
    lo, hi = -np.array(BLOCKS) * 8 / 64, np.array(BLOCKS) * 8 / 64
    parts.append(rng.uniform(0.9 * lo, 0.9 * hi, (k, 3)))
    normals.append(_unit(rng.normal(size=(k, 3))))
    order = rng.permutation(NUM_POINTS)
    p, n = np.full((NUM_POINTS, 4), np.nan, f32), np.full((NUM_POINTS, 4), np.nan, f32)
    p[:, 0:3], n[:, 0:3] = np.concatenate(parts)[order], np.concatenate(normals)[order]
    p.setflags(write=False)
    n.setflags(write=False)
    return p, n


OVERHANG_POINT = np.array([CENTRE_2[0] + 0.06, CENTRE_2[1], FLOOR, 0.0], f32)  # on the floor under the second sphere
OPEN_POINT = np.array([-0.9, 0.4, FLOOR, 0.0], f32)                           # on the floor far from both


def edge_points():
    """(points (m, 4), normals (m, 4), labels): what step a and b refuse and what the frame must survive, between valid points.  The
    unlisted one lies high above the spheres, in a block the surface does not pass through."""
    p, n = points()
    valid = np.nonzero(np.isfinite(p[:, 0:3]).all(axis=1))[0][:6]
    nan, inf = np.nan, np.inf
    s = 1.0 / np.sqrt(2.0)
    rows = [
        ("valid 0", p[valid[0], 0:3], n[valid[0], 0:3]),
        ("NaN coordinate", (nan, 0.0, 0.0), (0, 0, 1)),
        ("inf coordinate", (0.0, -inf, 0.0), (0, 0, 1)),
        ("valid 1", p[valid[1], 0:3], n[valid[1], 0:3]),
        ("zero normal", OPEN_POINT[0:3], (0, 0, 0)),
        ("negative zero normal", OPEN_POINT[0:3], (-0.0, 0.0, -0.0)),
        ("NaN normal", OPEN_POINT[0:3], (0, nan, 1)),
        ("n = +z", OPEN_POINT[0:3], (0, 0, 1)),
        ("n = -z", (0.3, 0.3, 0.5), (0, 0, -1)),
        ("n.z = -0", OPEN_POINT[0:3], (s, s, -0.0)),
        ("n.z = +0", OPEN_POINT[0:3], (s, -s, 0.0)),
        ("valid 2", p[valid[2], 0:3], n[valid[2], 0:3]),
        ("non-unit normal", OVERHANG_POINT[0:3], (0.0, 0.6, 2.5)),
        ("tiny normal", OPEN_POINT[0:3], (0.0, 0.0, 1e-30)),
        ("outside the box", (5.0, 0.0, 0.0), (0, 0, 1)),
        ("just outside the box", (0.0, 0.0, 0.7500001), (0, 0, -1)),
        ("unlisted block", (-0.9, 0.4, 0.6), (0, 0, 1)),
        ("valid 3", p[valid[3], 0:3], n[valid[3], 0:3]),
    ]
    pts, nrm = np.zeros((len(rows), 4), f32), np.zeros((len(rows), 4), f32)
    for i, (_label, a, b) in enumerate(rows):
        pts[i, 0:3], nrm[i, 0:3] = a, b
    return pts, nrm, [r[0] for r in rows]
