"""What the rm_light_probes test modules share: the stand-alone CPU program of raymarcher_amd/csrc/rm_light_probes.h (built under the
host sanitizers and run as a program), and the fixture of the GPU tests — the shapes, the probe positions of a case and the
direction tables with their bad rows."""
import functools
import os
import struct
import subprocess

import numpy as np

import helpers as h
import light_probes_spec as L
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import sphere_directions

f32 = np.float32
CPU_SRC = os.path.join(h.ROOT, "tests", "light_probes_spec", "rm_light_probes_cpu.cpp")
FAR = 100.0
# (K, n): the smallest shapes at which each mechanism of the kernel can go wrong.
#   K = 1, n = 65: one ray per probe, 64 probes per wave, two waves.  K = 2, n = 33: the last wave has one live segment of 32.
#   K = 64, n = 5: one probe per wave, a full butterfly, two workgroups.  K = 128, n = 3: two passes and one pending level.
#   K = 1024, n = 2: sixteen passes and four pending levels.
# Up to 64 directions the two probes with a non-finite position are among the n, so the calls have exactly 65, 33 and 5 probes.
# With more (n = 3 and n = 2) they would leave one finite probe or none, so they are added on top — calls of 5 and 4 probes, a wave
# each: the passes and levels of the finite probes are what they are with n probes.  n·K finite rays <= 2048 in every shape.
SHAPES = ((1, 65), (2, 33), (64, 5), (128, 3), (1024, 2))
SETS = (1, 3)


def build_cpu_program(directory):
    """g++, the address and undefined-behaviour sanitizers linked in statically, -ffp-contract=off: as the field tests build theirs."""
    exe = os.path.join(str(directory), "rm_light_probes_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, positions, table, K, sets, colours, hit):
    """positions (n, 4), table (sets·K, 16), colours (n·K, 4) float32 and hit (n·K) → PROBE records (n) of the program."""
    positions, table = np.ascontiguousarray(positions, f32), np.ascontiguousarray(table, f32)
    colours, hit = np.ascontiguousarray(colours, f32), np.ascontiguousarray(hit, np.uint8)
    n = len(positions)
    assert positions.shape == (n, 4) and table.shape == (sets * K, 16) and colours.shape == (n * K, 4) and hit.shape == (n * K,)
    src, dst = os.path.join(str(directory), "probes_query.bin"), os.path.join(str(directory), "probes_result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<3i", n, K, sets))
        f.write(positions.tobytes() + table.tobytes() + colours.tobytes() + hit.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 160 * n
    return np.frombuffer(raw, L.PROBE, n)


# ---------------------------------------------------------------- the GPU tests' fixture
def tables(K, sets):
    """The direction tables a shape is run with → [(label, float32 (sets·K, 16))]: rm_sphere_directions' with one row whose
    direction is zero and one whose direction has a NaN — their basis values stay, reserved and pad hold junk that is not read.  A
    table of one or two rows has no room for both beside a valid row: it is run as it is, and again with its rows bad."""
    clean = sphere_directions(K, sets)
    clean[:, 3] = f32(np.nan)          # reserved: not read
    clean[:, 13:16] = f32(-np.inf)     # pad: not read
    rows = K * sets
    if rows >= 3:
        t = clean.copy()
        t[1, 0:3] = (0.0, -0.0, 0.0)
        t[rows - 1, 1] = f32(np.nan)
        return [("bad rows", t)]
    zero, nan = clean.copy(), clean.copy()
    zero[:, 0:3] = (-0.0, 0.0, 0.0)
    nan[:, 0] = f32(np.nan)
    if rows == 2:
        nan[0, 0:3] = (0.0, 0.0, 0.0)
    return [("clean", clean), ("zero rows", zero), ("zero and NaN rows" if rows == 2 else "NaN rows", nan)]


@functools.lru_cache(maxsize=None)
def positions(name, K, n):
    """The probe positions of case `name` for shape (K, n) → read-only float32 (m, 4), w = junk that is not read.  Seeded points
    inside and around the cull ball of the case's table; one inside an object — a little behind the first hit of a ray towards the
    ball's centre, where the case has objects —; one with a NaN and one with an infinite coordinate, neither first nor last."""
    scene, s, _ = S.case(name)
    centre, radius = T.cull_bounds(scene[1], scene[2], scene[5])
    rng = np.random.default_rng(7000 + 31 * K + sorted(S.CASES).index(name))
    extra = 2 if K > 64 else 0
    m = n + extra
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    p = np.zeros((m, 4), f32)
    p[:, 0:3] = np.asarray(centre) + u * (rng.uniform(0.2, 1.6, (m, 1)) * radius)
    p[:, 3] = rng.uniform(-5, 5, m)
    if scene[2] > 0:
        v = rng.normal(size=(64, 3))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        rec = T.spec_trace(scene[1], scene[2], scene[5], s, T.make_rays(np.asarray(centre) + v * 3.0 * radius, -v, 1000.0), "closest")
        found = np.nonzero(T.ids_of(rec) >= 0)[0]
        assert len(found), f"{name}: no ray towards the cull ball's centre hits an object"
        p[0, 0:3] = rec[found[0], 4:7] + f32(0.02 * radius) * (-v[found[0]]).astype(f32)
    bad = (1, m - 2) if m >= 4 else ()
    assert len(bad) == 2 and bad[0] != bad[1]
    p[bad[0], 1] = f32(np.nan)
    p[bad[1], 2] = f32(-np.inf)
    assert L.valid_positions(p).sum() == m - 2 == (n if extra else n - 2)
    p.setflags(write=False)
    return p
