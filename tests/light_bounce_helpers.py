"""What the light-bounce test modules share: the stand-alone CPU program of raymarcher_amd/csrc/rm_indirect.h over rm_light_grid.h
(built under the host sanitizers and run as a program), and the fixtures — light_grid_helpers' three grids with light_depth_helpers'
depth records, and seeded per-ray inputs of the term (shaded colours, diffuse colours, palette colours and kinds)."""
import os
import struct
import subprocess

import numpy as np

import helpers as h
import light_bounce_spec as B
import light_depth_helpers as MD
import light_depth_spec as D
import light_grid_helpers as MG
import light_grid_spec as G
import shade_helpers as S
from raymarcher_amd import abi

f32 = np.float32
CPU_SRC = os.path.join(h.ROOT, "tests", "light_bounce_spec", "rm_light_bounce_cpu.cpp")
COUNTS = MG.COUNTS    # 1, 64, 65, 257
BIASES = MD.BIASES    # 0 and 0.1
STRENGTHS = (1.0, 0.37)


def build_cpu_program(directory):
    """g++, the address and undefined-behaviour sanitizers linked in statically, -ffp-contract=off: as light_grid_helpers builds its own."""
    exe = os.path.join(str(directory), "rm_light_bounce_cpu")
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-Wall", "-Wno-unknown-pragmas", "-Wno-maybe-uninitialized",
           "-o", exe, CPU_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run_cpu_program(exe, directory, probes, depth, dims, origin, step, facing, normal_bias, k, points, normals, colour, dif, c, palette,
                    has_term):
    """PROBE records, DEPTH records or None, the grid, the lookup's flags and bias, k, and per ray the hit point, the normal, the
    shaded colour, the diffuse and the palette colour (n, 4) float32, the palette kind and has_term (n) → float32 (n, 4)."""
    arrays = [np.ascontiguousarray(a, f32) for a in (points, normals, colour, dif, c)]
    n = len(arrays[0])
    assert all(a.shape == (n, 4) for a in arrays) and probes.dtype == G.PROBE and (depth is None or depth.dtype == D.DEPTH)
    src, dst = os.path.join(str(directory), "bounce_query.bin"), os.path.join(str(directory), "bounce_result.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<6i", *(int(d) for d in dims), n, G.FACING if facing else 0, 0 if depth is None else 1))
        f.write(np.asarray(origin, f32).tobytes() + np.asarray(step, f32).tobytes() + f32(normal_bias).tobytes() + f32(k).tobytes())
        f.write(np.ascontiguousarray(probes).tobytes() + (b"" if depth is None else np.ascontiguousarray(depth).tobytes()))
        for a in arrays:
            f.write(a.tobytes())
        f.write(np.ascontiguousarray(palette, np.int32).tobytes() + np.ascontiguousarray(has_term, np.int32).tobytes())
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    raw = open(dst, "rb").read()
    assert len(raw) == 16 * n
    return np.frombuffer(raw, f32).reshape(n, 4)


def ray_inputs(name, n):
    """Seeded inputs of the term for the n points of light_grid_helpers.points(name, n) → (colour, dif, c, palette, has_term): shaded
    colours of both signs with alpha 1 to 3, a −0 and a denormal among them; diffuse colours in [0, 1] with zeros; palette colours in
    [0, 1]; every palette kind; and rays without a term (misses, emissive hits, invalid rays), neither first nor last from 64 on."""
    rng = np.random.default_rng(9900 + 13 * n + sorted(MG.GRIDS).index(name))
    colour = np.zeros((n, 4), f32)
    colour[:, 0:3] = rng.uniform(-0.5, 2.0, (n, 3))
    colour[:, 3] = rng.integers(1, 4, n)
    dif = np.zeros((n, 4), f32)
    dif[:, 0:3] = rng.uniform(0, 1, (n, 3))
    c = np.zeros((n, 4), f32)
    c[:, 0:3] = rng.uniform(0, 1, (n, 3))
    palette = rng.integers(0, 3, n).astype(np.int32)
    has_term = np.ones(n, np.int32)
    if n >= 64:
        colour[3, 0], colour[4, 1], dif[5, 0:3], dif[6, 2] = f32(-0.0), f32(1e-42), f32(0.0), f32(-0.0)
        has_term[rng.choice(np.arange(1, n - 1), n // 8, replace=False)] = 0
        palette[0:3] = (B.PLAIN, B.BULB, B.SPONGE)
    return colour, dif, c, palette, has_term


# ---------------------------------------------------------------- shade_rays_indirect through the shipped entries
def object_fields(scene):
    _, objs, no = scene[:3]
    m = max(no, 1)
    return {"cDiffuse": np.array([list(objs[i].cDiffuse) for i in range(m)], f32), "type": np.array([objs[i].type for i in range(m)]),
            "isEmissive": np.array([objs[i].isEmissive for i in range(m)]), "texLoc": np.array([objs[i].texLoc for i in range(m)]),
            "repeatU": np.array([objs[i].repeatU for i in range(m)], np.float64), "repeatV": np.array([objs[i].repeatV for i in range(m)], np.float64),
            "blend": np.array([objs[i].blend for i in range(m)], np.float64),
            "invModel": np.array([np.array(list(objs[i].invModel), np.float64).reshape(4, 4).T for i in range(m)])}


def palette_tables(scene, s, res):
    """The copy of the tables whose shade_rays colour is the palette factor alone: no lights, ka = 1, cAmbient = 1, AO, reflection
    and refraction off — Phong is (1·1)·1 = 1 exactly, so the colour of a hit is 8c on the bulb, c on the sponge, 1 elsewhere."""
    cam, objs, no, _, _, g = scene[:6]
    o = (abi.RmObject * max(no, 1))(*[abi.RmObject.from_buffer_copy(bytes(objs[i])) for i in range(no)])
    for i in range(no):
        for k in range(3):
            o[i].cAmbient[k] = 1.0
    g2 = abi.RmGlobals.from_buffer_copy(bytes(g))
    g2.ka = 1.0
    s2 = abi.RmSettings.from_buffer_copy(bytes(s))
    s2.enableAmbientOcclusion = s2.enableReflection = s2.enableRefraction = 0
    return S.tables_of((cam, o, no, None, 0, g2), res), s2


def composed_indirect(renderer, scene, s, res, rays, grid, facing, bias, strength, far):
    """shade_rays_indirect through the shipped entries — shade_rays, trace_rays with tMax = far, the grid's lookup, a second
    shade_rays call for the palette factor and the NumPy term — → (want (n, 4), on (n): the rays with a term, textured (n): the
    hits of textured objects, whose dif the composition does not have bit for bit, parts: what went into it).  scene, s, res: a
    case of shade_helpers.CASES or any other tables; grid: a LightGrid."""
    t = S.tables_of(scene, res)
    rays = np.array(rays)
    n = len(rays)
    colour = renderer.shade_rays(t, s, rays, far=far).cpu().numpy()
    probe = rays.copy()
    probe[:, 3] = f32(far)
    normal, _, point, obj = (a.cpu().numpy() for a in renderer.trace_rays(t, s, probe))
    o = object_fields(scene)
    k = np.maximum(obj, 0)
    has_term = (obj >= 0) & (o["isEmissive"][k] == 0)
    p4, n4 = np.zeros((n, 4), f32), np.zeros((n, 4), f32)
    p4[:, 0:3], n4[:, 0:3] = point, normal
    e, _, probes = grid.irradiance_visible(p4, n4, facing=facing, visible=grid.depth is not None, normal_bias=bias)
    e, probes = e.cpu().numpy(), probes.cpu().numpy()
    tp, sp = palette_tables(scene, s, res)
    pal = renderer.shade_rays(tp, sp, rays, far=far).cpu().numpy()[:, 0:3]
    kind = np.where(o["type"][k] == abi.RM_MANDELBULB, B.BULB, np.where(o["type"][k] == abi.RM_MENGERSPONGE, B.SPONGE, B.PLAIN))
    plain = has_term & (kind == B.PLAIN)
    assert (pal[plain] == f32(1)).all(), "the palette call's colour is exactly 1 on a hit of anything but the two fractals"
    c = np.where((kind == B.BULB)[:, None], pal * f32(0.125), pal).astype(f32)  # 8c → c, exact
    dif = (f32(scene[5].kd) * o["cDiffuse"][k]).astype(f32)
    want = B.term(colour, has_term, probes, e, dif, B.scale_of(strength), kind, c)
    on = has_term & (probes > 0)
    textured = on & (o["texLoc"][k] != -1)
    return want, on, textured, dict(colour=colour, obj=obj, point=point, e=e, probes=probes, kind=kind, c=c, o=o, k=k)
