"""What the rm_rays_order tests share: the seeded ray families, the shuffled camera frame with its pixels, and the CPU program that
runs the library's key header (tests/ray_order_spec/rm_ray_order_cpu.cpp) under the host sanitizers as a child process."""
import functools
import os
import struct
import subprocess

import numpy as np

import helpers as h
from raymarcher_amd import camera_rays

f32 = np.float32
CPU_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ray_order_spec", "rm_ray_order_cpu.cpp")
FRAME_W, FRAME_H = 96, 64


@functools.lru_cache(maxsize=None)
def camera_frame(W=FRAME_W, H=FRAME_H, seed=11):
    """(rays float32 (W·H, 8), pixels int (W·H, 2)) of a 60° pinhole camera's frame from rm_camera_rays, in a seeded shuffle;
    pixels[i] = the (x, y) of ray i.  Read-only, shared."""
    cam = h.make_camera((0.5, 0.25, 6.0), (-0.1, 0.05, -1.0), (0, 1, 0), 60.0, W, H)
    rays = camera_rays(cam, W, H)
    y, x = np.divmod(np.arange(W * H), W)
    perm = np.random.default_rng(seed).permutation(W * H)
    rays, pixels = np.ascontiguousarray(rays[perm]), np.stack([x, y], 1)[perm]
    rays.setflags(write=False)
    pixels.setflags(write=False)
    return rays, pixels


def specials():
    """NaN and ±inf in each component of origin and dir, a zero dir of either sign, −0 components, denormals, components of 3e38
    (their sum overflows), −0 and +0 both present in every coordinate, unusual tMax and `reserved` words → float32 (n, 8)."""
    inf, nan, tiny, big = np.inf, np.nan, 1e-42, 3e38
    rows = []
    for k in (0, 1, 2, 4, 5, 6):
        for bad in (nan, inf, -inf):
            r = [0.1, 0.2, 5.0, 10.0, 0.3, -0.4, -1.0, 0.0]
            r[k] = bad
            rows.append(r)
    rows += [[0.1, 0.2, 5.0, 10.0, 0.0, 0.0, 0.0, 0.0], [0.1, 0.2, 5.0, 10.0, -0.0, 0.0, -0.0, 0.0]]   # dir all zeros: not valid
    rows += [[0.0, -0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0], [-0.0, 0.0, -0.0, 1.0, -0.0, -0.0, 1.0, 0.0],   # zeros of both signs, u = v = ±0
             [0.0, 0.0, 0.0, 1.0, -0.0, 0.0, -1.0, 0.0], [0.0, 0.0, 0.0, 1.0, 0.0, -0.0, -1.0, 0.0],    # … through the lower half's fold
             [1.0, -1.0, 2.0, nan, 1.0, 0.0, 0.0, 0.0], [1.0, -1.0, 2.0, -5.0, 0.0, -1.0, -0.0, 0.0],   # tMax NaN or negative: valid here
             [tiny, -tiny, tiny, 1.0, tiny, -tiny, tiny, 0.0], [tiny, tiny, -tiny, 1.0, -tiny, 2 * tiny, -3 * tiny, 0.0],
             [big, -big, big, 1.0, big, big, big, 0.0], [-big, big, -big, 1.0, -big, big, -big, 0.0],    # s = +inf, x − lo = +inf
             [big, 0.0, 0.0, 1.0, big, -tiny, 0.0, 0.0], [0.5, 0.5, 0.5, 1.0, 1.0, 1.0, 1.0, 0.0],
             [0.5, 0.5, 0.5, 1.0, -1.0, -1.0, -1.0, 0.0], [0.25, 0.75, -0.5, 1.0, 0.0, 0.0, -2.0, 0.0]]
    a = np.array(rows, dtype=f32)
    a[:, 7].view(np.uint32)[::3] = 0xDEADBEEF  # `reserved` is not read, and is copied verbatim
    return a


@functools.lru_cache(maxsize=None)
def family(name, n=700):
    """A seeded ray family → float32 (n, 8), read-only.  camera: the shuffled frame's first n rays (ONE origin); box: random origins
    in a box with random directions; identical: one ray n times; flat: all origins share one coordinate; one_origin: all origins
    are one point, a few directions are zero; specials: the special values, cycled and mixed with box rays so that every wave of
    64 holds them."""
    rng = np.random.default_rng(sum(map(ord, name)) + n)
    box = np.zeros((n, 8), f32)
    box[:, 0:3] = rng.uniform((-3, -1, 2), (4, 5, 9), (n, 3))
    box[:, 3] = rng.uniform(0.1, 100.0, n)
    box[:, 4:7] = rng.normal(size=(n, 3)) * rng.uniform(0.2, 3.0, (n, 1))
    if name == "camera":
        rays = camera_frame()[0]
        a = np.array(rays[np.arange(n) % len(rays)])
    elif name == "box":
        a = box
    elif name == "identical":
        a = np.repeat(box[:1], n, axis=0)
    elif name == "flat":
        a = box
        a[:, 1] = f32(0.75)
    elif name == "one_origin":  # every origin digit is the same in all keys; the few rays that are not valid differ in the top bit,
        a = box                 # so with origin bits the sort skips passes in the middle and runs one after them
        a[:, 0:3] = (f32(0.5), f32(-1.25), f32(3.0))
        a[5::211, 4:7] = 0.0
    elif name == "specials":
        sp = specials()
        a = box
        where = np.arange(n) % 3 != 0
        a[where] = sp[np.arange(where.sum()) % len(sp)]
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a, f32)
    a.setflags(write=False)
    return a


FAMILIES = ("camera", "box", "identical", "flat", "one_origin", "specials")


# ---------------------------------------------------------------- the library's key header on the CPU
def build_cpu_program(directory):
    """As sdf_blocks_helpers.build_cpu_program builds its twin: g++, the address and undefined-behaviour sanitizers linked in
    statically, -ffp-contract=off."""
    exe = os.path.join(str(directory), "rm_ray_order_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, rays, origin_bits, dir_bits, flip_zeros=False):
    """→ dict(keys uint64 (n,), order int32 (n,), lo, hi float32 (5,))."""
    rays = np.ascontiguousarray(rays, f32)
    n = len(rays)
    src, dst = os.path.join(str(directory), "rays.bin"), os.path.join(str(directory), "order.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<4i", n, origin_bits, dir_bits, 1 if flip_zeros else 0))
        f.write(rays.tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 12 * n + 40, len(raw)
    return dict(keys=np.frombuffer(raw, np.uint64, n, 0), order=np.frombuffer(raw, np.int32, n, 8 * n),
                lo=np.frombuffer(raw, f32, 5, 12 * n), hi=np.frombuffer(raw, f32, 5, 12 * n + 20))
