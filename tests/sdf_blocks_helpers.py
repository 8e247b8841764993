"""What the block-sparse lattice tests share: dense lattices of 8·m + 1 points per axis (the oracle's sdScene, and hand-made values a
distance function would not produce), block lists with voids, and the CPU program that runs the library's block-local arithmetic
(tests/sdf_blocks_spec/rm_sdf_blocks_cpu.cpp) under the host sanitizers."""
import functools
import os
import struct
import subprocess

import numpy as np

import helpers as h
import sdf_blocks_spec as B
import sdf_helpers as V

f32 = np.float32
CPU_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sdf_blocks_spec", "rm_sdf_blocks_cpu.cpp")

# name → (table, dims, iso): lattices of 3×2×2 and 4×4×4 blocks across the tables' surfaces
ORACLE_CASES = {"sphere_25": ("sphere", (25, 17, 17), 0.0), "primitives_25": ("primitives", (25, 17, 17), 0.0),
                "sphere_cube_25_iso": ("sphere_cube", (25, 17, 17), 0.07), "menger_33": ("menger", (33, 33, 33), 0.0),
                "bulb_33": ("bulb_plain", (33, 33, 33), 0.001)}


@functools.lru_cache(maxsize=None)
def handmade():
    """name → (dense (nz, ny, nx), ids or None, origin, step, iso) at 9³ and 17×9×9 points: one block and two blocks along x."""
    inf, nan = f32(np.inf), f32(np.nan)
    rng = np.random.default_rng(31)
    origin, step = np.array([-1.0, 0.5, 2.0], f32), np.array([0.25, 0.5, 0.125], f32)
    out = {}
    a = rng.uniform(-1, 1, (9, 9, 9)).astype(f32)
    a[rng.uniform(size=a.shape) < 0.1] = 0.25  # values exactly equal to iso: outside
    out["iso_ties_9"] = (a, rng.integers(0, 5, a.shape).astype(np.int32), origin, step, 0.25)
    b = rng.uniform(-1, 1, (9, 9, 17)).astype(f32)
    pick = rng.uniform(size=b.shape)
    b[pick < 0.05], b[(pick >= 0.05) & (pick < 0.1)], b[(pick >= 0.1) & (pick < 0.15)] = nan, inf, -inf
    b[4, 4, 8], b[3, 5, 8], b[0, 0, 8] = nan, -inf, inf  # on the face the two blocks share
    out["nonfinite_17x9x9"] = (b, rng.integers(0, 3, b.shape).astype(np.int32), origin, step, 0.0)
    c = np.full((9, 9, 17), inf, f32)  # every crossing runs between infinities; the box spans both blocks
    c[2:7, 3:6, 5:12] = -inf
    out["infinities_17x9x9"] = (c, None, origin, step, 0.0)
    out["all_inside_9"] = (np.full((9, 9, 9), -1.0, f32), None, origin, step, 0.0)
    out["all_outside_17x9x9"] = (np.full((9, 9, 17), 2.0, f32), np.zeros((9, 9, 17), np.int32), origin, step, 0.0)
    d = np.full((9, 9, 17), 1.0, f32)  # a slab that leaves the lattice through four of its faces and crosses the shared face
    d[3:6, :, :] = -1.0
    out["touches_boundary_17x9x9"] = (d, None, origin, step, 0.0)
    e = np.full((9, 9, 17), 1.0, f32)
    e[:, :, 8] = -0.5  # inside points only on the face the two blocks share
    out["shared_face_only_17x9x9"] = (e, None, origin, step, 0.0)
    for v in out.values():
        for x in v[:4]:
            if x is not None:
                x.setflags(write=False)
    return out


def case(name):
    """(dense, ids, origin, step, iso) of an oracle or hand-made case."""
    if name in ORACLE_CASES:
        table, dims, iso = ORACLE_CASES[name]
        dist, ids, origin, step = V.oracle_lattice(table, dims)
        return dist, ids, origin, step, iso
    return handmade()[name]


def messy_list(blocks, order_seed=7):
    """Every block of the lattice once, shuffled, with duplicates (before and after their originals' places) and entries outside
    the lattice interleaved; the fourth word is not zero everywhere → int32 (n, 4)."""
    mx, my, mz = blocks
    rng = np.random.default_rng(order_seed)
    good = B.all_blocks(blocks)[rng.permutation(mx * my * mz)]
    outside = ((-1, 0, 0), (mx, 0, 0), (0, my, 0), (0, 0, -5), (0, 0, mz), (2 ** 31 - 1, -2 ** 31, 0))
    rows = []
    for n, row in enumerate(good.tolist()):
        rows.append(row[:3] + [n % 3])
        if n % 3 == 0:
            rows.append(good[rng.integers(0, len(good))].tolist()[:3] + [9])  # a duplicate of an entry before or after this place
        if n % 4 == 1:
            rows.append(list(outside[(n // 4) % len(outside)]) + [0])
    rows.append(list(outside[1]) + [0])  # and one more void at the very end
    return np.array(rows, np.int32).reshape(-1, 4)


# ---------------------------------------------------------------- the library's block-local arithmetic on the CPU
def build_cpu_program(directory):
    """As sdf_helpers.build_cpu_program builds its twin: g++, the address and undefined-behaviour sanitizers linked in statically,
    -ffp-contract=off."""
    exe = os.path.join(str(directory), "rm_sdf_blocks_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, packed, packed_ids, block_list, blocks, origin, step, iso):
    n = len(block_list)
    src, dst = os.path.join(str(directory), "blocks.bin"), os.path.join(str(directory), "mesh.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<5i", blocks[0], blocks[1], blocks[2], n, 0 if packed_ids is None else 1))
        f.write(np.asarray(origin, f32).tobytes() + np.asarray(step, f32).tobytes() + f32(iso).tobytes())
        f.write(np.ascontiguousarray(block_list, np.int32).tobytes())
        f.write(np.ascontiguousarray(packed, f32).tobytes())
        if packed_ids is not None:
            f.write(np.ascontiguousarray(packed_ids, np.int32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    nv, nq, no = struct.unpack_from("<3I", raw, 0)
    off = 12
    verts = np.frombuffer(raw, f32, nv * 4, off).reshape(nv, 4)
    off += nv * 16
    vobj = np.frombuffer(raw, np.int32, nv, off)
    off += nv * 4
    quads = np.frombuffer(raw, np.int32, nq * 4, off).reshape(nq, 4)
    off += nq * 16
    active = np.frombuffer(raw, np.int32, n, off)
    assert off + n * 4 == len(raw)
    return dict(vertices=verts, vertex_object=vobj, quads=quads, counts=(nv, nq, no), active=active)


def assert_mesh_equal(got, want, what):
    assert tuple(got["counts"]) == tuple(want["counts"]), f"{what}: counts {got['counts']} against {want['counts']}"
    h.assert_bit_equal(got["vertices"], want["vertices"], f"{what}: vertices")
    assert (got["vertex_object"] == want["vertex_object"]).all(), f"{what}: vertex ids"
    assert (got["quads"] == want["quads"]).all(), f"{what}: quads"
