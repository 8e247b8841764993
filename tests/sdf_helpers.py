"""What the rm_sdf_grid / rm_sdf_mesh tests share: the object tables and lattices (the oracle's sdScene on the lattice points of the
specification, computed once per process), the hand-made lattices, the mesh's geometric properties, and the CPU program that runs
the library's own per-cell and per-edge functions (tests/sdf_mesh_spec/rm_sdf_mesh_cpu.cpp) under the host sanitizers."""
import ctypes as C
import functools
import os
import struct
import subprocess

import numpy as np

import helpers as h
import sdf_mesh_spec as S
from raymarcher_amd import abi

f32 = np.float32
bits, assert_bits = h.bits, h.assert_bit_equal
HERE = os.path.dirname(os.path.abspath(__file__))
CPU_SRC = os.path.join(HERE, "sdf_mesh_spec", "rm_sdf_mesh_cpu.cpp")
CPU_DEPS = [CPU_SRC, os.path.join(h.ROOT, "raymarcher_amd", "csrc", "rm_surface_nets.h")]


# ---------------------------------------------------------------- object tables
def scene(name):
    """(objs, numObjects, globals, settings) of a named table."""
    s = abi.default_settings()
    g = h.make_globals()
    rot = h.rotation
    if name == "sphere":
        objs = [h.make_object(abi.RM_SPHERE)]
    elif name == "sphere_cube":
        objs = [h.make_object(abi.RM_SPHERE, model=h.translate(-0.8, 0, 0)), h.make_object(abi.RM_CUBE, model=h.translate(0.8, 0, 0))]
    elif name == "primitives":  # one of each primitive type, rotated and scaled, spread over a 3 × 3 arrangement
        objs = []
        for n, ty in enumerate(h.PRIMITIVES):
            sc = 0.6 + 0.1 * (n % 4)
            M = h.translate(1.5 * (n % 3 - 1), 1.5 * (n // 3 - 1), 0.2 * (n % 2)) @ rot((1, n + 1, 2), 0.4 + 0.3 * n) @ h.scale(sc, sc * 1.2, sc * 0.9)
            objs.append(h.make_object(ty, model=M, scale_factor=sc * 0.9))
    elif name == "menger":
        objs = [h.make_object(abi.RM_MENGERSPONGE, model=rot((0, 1, 0), 0.3))]
        g = h.make_globals(itime=1.7)
    elif name == "sierpinski":
        objs = [h.make_object(abi.RM_SIERPINSKI)]
    elif name == "julia":
        objs = [h.make_object(abi.RM_MANDELBULB)]
        g = h.make_globals(julia=(0.3, -0.2))
    elif name == "bulb_plain":
        objs = [h.make_object(abi.RM_MANDELBULB)]
    elif name == "bulb_moved":
        objs = [h.make_object(abi.RM_MANDELBULB, model=h.translate(0.1, -0.05, 0.2) @ rot((1, 1, 0), 0.5))]
    elif name == "bulb_power6":
        objs = [h.make_object(abi.RM_MANDELBULB)]
        g = h.make_globals(power=6.0)
    else:
        raise KeyError(name)
    objs, no = h.table(objs)
    return objs, no, g, s


# the box each table's lattices span: they cross the objects' surfaces and, for the bulbs, hold points inside the set
BOXES = {"sphere": ((-0.8, -0.8, -0.8), (0.8, 0.8, 0.8)), "sphere_cube": ((-1.6, -0.8, -0.8), (1.6, 0.8, 0.8)),
         "primitives": ((-2.3, -2.3, -0.9), (2.3, 2.3, 1.1)), "menger": ((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7)),
         "sierpinski": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "julia": ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)),
         "bulb_plain": ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)), "bulb_moved": ((-1.1, -1.25, -1.0), (1.3, 1.15, 1.4)),
         "bulb_power6": ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2))}


def lattice_of(name, dims):
    """origin and step (float32 arrays of 3) of the dims = (nx, ny, nz) lattice that spans the table's box; a dimension of 1 sits
    at the box's lower face."""
    lo, hi = (np.array(v, dtype=np.float64) for v in BOXES[name])
    step = np.array([(hi[a] - lo[a]) / max(dims[a] - 1, 1) for a in range(3)])
    return lo.astype(f32), step.astype(f32)


@functools.lru_cache(maxsize=None)
def oracle_lattice(name, dims):
    """The oracle's sdScene on the lattice → (dist float32 (nz, ny, nx), ids int32 (nz, ny, nx), origin, step), read-only."""
    objs, no, g, s = scene(name)
    origin, step = lattice_of(name, dims)
    pts = S.lattice_points(origin, step, dims)
    out = np.empty((len(pts), 4), dtype=f32)
    assert h.oracle().rmo_probe_sdscene(objs, no, C.byref(g), C.byref(s), h.fptr(pts), h.fptr(out), len(pts)) == 0
    nx, ny, nz = dims
    dist = np.ascontiguousarray(out[:, 0]).reshape(nz, ny, nx)
    ids = out[:, 1].astype(np.int32).reshape(nz, ny, nx)
    for a in (dist, ids, origin, step):
        a.setflags(write=False)
    return dist, ids, origin, step


# ---------------------------------------------------------------- hand-made lattices
def handmade():
    """name → (dist (nz, ny, nx), ids or None, origin, step, iso): the values a distance function would not produce."""
    inf, nan = f32(np.inf), f32(np.nan)
    rng = np.random.default_rng(20)
    out = {}
    origin, step = np.array([-1.0, 0.5, 2.0], f32), np.array([0.25, 0.5, 0.125], f32)
    a = rng.uniform(-1, 1, (4, 4, 4)).astype(f32)
    a[1, 2, 1], a[2, 2, 2], a[0, 0, 0], a[3, 3, 3] = 0.25, 0.25, 0.25, 0.25  # values exactly equal to iso: outside
    out["iso_ties_4x4x4"] = (a, rng.integers(0, 5, a.shape).astype(np.int32), origin, step, 0.25)
    b = rng.uniform(-1, 1, (4, 5, 3)).astype(f32)  # 3 × 5 × 4 as (nx, ny, nz)
    b[1, 1, 1], b[1, 2, 1], b[2, 3, 1], b[2, 1, 1], b[1, 3, 1] = nan, inf, -inf, -inf, inf
    b[2, 2, 1] = nan
    out["nonfinite_3x5x4"] = (b, rng.integers(0, 3, b.shape).astype(np.int32), origin, step, 0.0)
    c = np.full((4, 4, 4), inf, f32)  # every crossing runs between infinities: t is NaN, the fallback 0.5 places the vertices
    c[1:3, 1:3, 1:3] = -inf
    out["infinities_4x4x4"] = (c, None, origin, step, 0.0)
    out["all_inside_4x4x4"] = (np.full((4, 4, 4), -1.0, f32), None, origin, step, 0.0)
    out["all_outside_3x5x4"] = (np.full((4, 5, 3), 2.0, f32), np.zeros((4, 5, 3), np.int32), origin, step, 0.0)
    d = np.full((4, 5, 3), 1.0, f32)  # a slab that runs out of the lattice through four of its faces: boundary edges give no quad
    d[1:3, :, :] = -1.0
    out["touches_boundary_3x5x4"] = (d, None, origin, step, 0.0)
    e = np.full((4, 4, 4), 1.0, f32)
    e[0, :, :] = -0.5  # inside points only on the lattice's own face
    out["face_only_4x4x4"] = (e, None, origin, step, 0.0)
    return out


# ---------------------------------------------------------------- the mesh's geometry
def directed_edges(quads):
    q = np.asarray(quads, dtype=np.int64)
    return np.concatenate([np.stack([q[:, n], q[:, (n + 1) % 4]], axis=1) for n in range(4)])


def assert_closed_oriented(quads, what):
    """Every mesh edge is shared by exactly two quads, which run along it in opposite directions.  Returns the number of edges."""
    de = directed_edges(quads)
    assert (de[:, 0] != de[:, 1]).all(), f"{what}: a degenerate edge"
    key = de[:, 0] * (de.max() + 1) + de[:, 1]
    uniq, counts = np.unique(key, return_counts=True)
    assert (counts == 1).all(), f"{what}: a directed edge used twice (two quads with the same orientation on one edge)"
    rev = de[:, 1] * (de.max() + 1) + de[:, 0]
    assert np.isin(rev, uniq).all(), f"{what}: an edge without its opposite (a hole, or a flipped quad)"
    return len(uniq) // 2


def components(num_vertices, quads):
    """Labels of the connected components of the mesh's vertices (union-find over the quads' edges)."""
    parent = np.arange(num_vertices)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in directed_edges(quads):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    return np.array([find(x) for x in range(num_vertices)])


def signed_volume(vertices, quads):
    """The volume the mesh encloses by the divergence theorem, each quad cut along (v0, v2); positive with outward normals."""
    v = np.asarray(vertices, dtype=np.float64)[:, :3]
    q = np.asarray(quads)
    a, b, c, d = (v[q[:, n]] for n in range(4))
    return float((np.einsum("ij,ij->i", a, np.cross(b, c)) + np.einsum("ij,ij->i", a, np.cross(c, d))).sum() / 6.0)


# ---------------------------------------------------------------- the library's per-cell and per-edge functions on the CPU
def build_cpu_program(directory):
    """g++ with the address and undefined-behaviour sanitizers linked in statically: a stand-alone program that needs nothing
    preloaded.  -ffp-contract=off: the definition's operations one by one."""
    exe = os.path.join(str(directory), "rm_sdf_mesh_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, dist, ids, origin, step, iso):
    nz, ny, nx = dist.shape
    src, dst = os.path.join(str(directory), "lattice.bin"), os.path.join(str(directory), "mesh.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4i", nx, ny, nz, 0 if ids is None else 1))
        f.write(np.asarray(origin, f32).tobytes() + np.asarray(step, f32).tobytes() + f32(iso).tobytes())
        f.write(np.ascontiguousarray(dist, f32).tobytes())
        if ids is not None:
            f.write(np.ascontiguousarray(ids, np.int32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    nv, nq = struct.unpack_from("<2I", raw, 0)
    off = 8
    verts = np.frombuffer(raw, f32, nv * 4, off).reshape(nv, 4)
    off += nv * 16
    vobj = np.frombuffer(raw, np.int32, nv, off)
    off += nv * 4
    quads = np.frombuffer(raw, np.int32, nq * 4, off).reshape(nq, 4)
    assert off + nq * 16 == len(raw)
    return dict(vertices=verts, vertex_object=vobj, quads=quads)


def read_ply(path):
    """A few lines of PLY reader for what rm_write_ply writes → (vertices (n, 3) float32, colours (n, 3) uint8 or None, quads (m, 4))."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([ln for ln in lines if ln.startswith("element vertex")][0].split()[2])
    nq = int([ln for ln in lines if ln.startswith("element face")][0].split()[2])
    assert "property list uchar int vertex_indices" in lines
    rgb = "property uchar red" in lines
    vt = np.dtype([("xyz", "<f4", 3)] + ([("rgb", "u1", 3)] if rgb else []))
    ft = np.dtype([("n", "u1"), ("idx", "<i4", 4)])
    v = np.frombuffer(raw, vt, nv, end)
    fc = np.frombuffer(raw, ft, nq, end + nv * vt.itemsize)
    assert end + nv * vt.itemsize + nq * ft.itemsize == len(raw) and (fc["n"] == 4).all()
    return v["xyz"].copy(), (v["rgb"].copy() if rgb else None), fc["idx"].copy()
