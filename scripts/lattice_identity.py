#!/usr/bin/env python3
"""The bits of the lattice family and of rm_rays_order, for comparing two builds of the library: every entry on fixed small inputs,
the SHA-256 of every output buffer and the bytes rm_release_workspaces frees after each entry, into one JSON file.  Run it in a
checkout of each build and compare the files (--compare): every kernel involved is deterministic — integer atomics, a stable sort —
so two builds that compute the same give the same file.

Scenes: a sphere beside a cube (the table walk), the headline Mandelbulb (the plain bulb class, 12 iterations) and a Menger sponge
(5 levels).  Lattices: dense, 33 points per axis over the scene's box, and block-sparse, 11 × 10 × 10 blocks over the same box
(1100 flags: two shares of the compaction).  Entries per scene: rm_sdf_blocks_select; rm_sdf_blocks_select_pruned at (4, +inf) and
(1, 1); rm_sdf_grid; rm_sdf_grid_blocks; rm_sdf_mesh; rm_sdf_mesh_blocks; rm_sdf_sample and rm_sdf_trace, dense and block form;
RmField handles, dense and block form: sample, closest, closest without normals, occlusion.  Then rm_rays_order on 70 000 shuffled
rays at the default key bits, with keys.

  python scripts/lattice_identity.py --out FILE
  python scripts/lattice_identity.py --compare FILE_A FILE_B"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ISO = 0.001
BLOCKS = (11, 10, 10)
DENSE = 33

TWO_SOLIDS = json.dumps({
    "name": "root",
    "globalData": {"ambientCoeff": 0.5, "diffuseCoeff": 0.5, "specularCoeff": 0.5, "transparentCoeff": 0.5},
    "cameraData": {"position": [0, 0, 5], "up": [0, 1, 0], "heightAngle": 30.0, "focus": [0, 0, 0]},
    "groups": [{"lights": [{"type": "directional", "color": [1, 1, 1], "direction": [0, -1, -1]}]},
               {"translate": [-0.8, 0, 0], "primitives": [{"type": "sphere", "diffuse": [1, 1, 1]}]},
               {"translate": [0.8, 0, 0], "primitives": [{"type": "cube", "diffuse": [1, 1, 1]}]}]})


def compare(a, b):
    records = []
    for path in (a, b):
        with open(path) as f:
            records.append(json.load(f))
    x, y = records
    keys = sorted(set(x) | set(y))
    differ = [k for k in keys if x.get(k) != y.get(k)]
    for k in differ:
        print(f"DIFFERS {k}: {x.get(k)} | {y.get(k)}")
    print(f"{len(keys)} records, {len(differ)} differ")
    return 1 if differ else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        return compare(*args.compare)
    if not args.out:
        ap.error("--out FILE or --compare A B")

    import ctypes as C

    import numpy as np
    import torch
    from raymarcher_amd import Renderer, Scene, abi, lib, scenes

    r = Renderer(0)
    L = lib()
    record = {}

    def digest(t):
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def done(entry, **buffers):
        """The entry's output buffers and what its workspaces held."""
        torch.cuda.synchronize()
        for name, t in buffers.items():
            record[f"{entry}/{name}"] = {"shape": list(t.shape), "sha256": digest(t)}
        freed = C.c_ulonglong(0)
        assert L.rm_release_workspaces(C.byref(freed)) == abi.RM_OK
        record[f"{entry}/workspace_bytes"] = int(freed.value)

    def queries(box, rng):
        """Points in and around the box, and rays from around it towards it; a few that no lattice can serve."""
        lo, hi = (np.asarray(v, np.float64) for v in box)
        mid, half = (lo + hi) / 2, (hi - lo) / 2
        pts = (mid + rng.uniform(-1.1, 1.1, (4096, 3)) * half).astype(np.float32)
        pts[7] = np.nan
        start = mid + rng.normal(size=(4096, 3)) * half * 1.6
        aim = mid + rng.uniform(-0.8, 0.8, (4096, 3)) * half
        d = aim - start
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays = np.zeros((4096, 8), np.float32)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7] = start, 50.0, d
        rays[5, 4:7] = 0.0
        rays[9, 0] = np.inf
        rays[11, 3] = 0.5
        return pts, rays

    def field_entries(entry, field, pts, rays):
        with field as f:
            done(f"{entry}/sample", **dict(zip(("gradient", "value", "cell", "object"), f.sample(pts))))
            for mode, kw in (("closest", {}), ("no_normal", dict(normals=False)), ("occlusion", dict(mode="occlusion"))):
                done(f"{entry}/{mode}", **dict(zip(("normal", "t", "position", "object"), f.trace(rays, ISO, 200, **kw))))
            torch.cuda.synchronize()

    def scene(tag, t, s, box):
        rng = np.random.default_rng(11)
        lo, hi = (np.asarray(v, np.float64) for v in box)
        pts, rays = queries(box, rng)
        # the block-sparse lattice
        step = tuple(float(x) for x in (hi - lo) / (8 * np.asarray(BLOCKS)))
        bl = r.sdf_active_blocks(t, s, lo, step, BLOCKS, ISO)
        done(f"{tag}/select", list=bl)
        for constants in ((4.0, None), (1.0, 1.0)):
            pl, cand = r.sdf_active_blocks_pruned(t, s, lo, step, BLOCKS, ISO, *constants)
            record[f"{tag}/select_pruned{constants}/candidates"] = cand
            done(f"{tag}/select_pruned{constants}", list=pl)
        gb, ib = r.sdf_grid_blocks(t, s, lo, step, BLOCKS, bl, ids=True)
        done(f"{tag}/grid_blocks", dist=gb, ids=ib)
        v, q, vo, nopen = r.extract_mesh_blocks(gb, bl, BLOCKS, lo, step, ISO, ib)
        record[f"{tag}/mesh_blocks/open"] = nopen
        done(f"{tag}/mesh_blocks", vertices=v, quads=q, vertex_object=vo)
        done(f"{tag}/sample_blocks", **dict(zip(("gradient", "value", "cell", "object"), r.sample_lattice_blocks(gb, bl, BLOCKS, lo, step, pts, ib))))
        done(f"{tag}/trace_blocks", **dict(zip(("normal", "t", "position", "object"), r.trace_lattice_blocks(gb, bl, BLOCKS, lo, step, rays, ISO, 200, ib))))
        field_entries(f"{tag}/field_blocks", r.lattice_field_blocks(gb, bl, BLOCKS, lo, step, ib), pts, rays)
        # the dense lattice
        step = tuple(float(x) for x in (hi - lo) / (DENSE - 1))
        g, i = r.sdf_grid(t, s, lo, step, (DENSE,) * 3, ids=True)
        done(f"{tag}/grid", dist=g, ids=i)
        v, q, vo = r.extract_mesh(g, lo, step, ISO, i)
        done(f"{tag}/mesh", vertices=v, quads=q, vertex_object=vo)
        done(f"{tag}/sample", **dict(zip(("gradient", "value", "cell", "object"), r.sample_lattice(g, lo, step, pts, i))))
        done(f"{tag}/trace", **dict(zip(("normal", "t", "position", "object"), r.trace_lattice(g, lo, step, rays, ISO, 200, i))))
        field_entries(f"{tag}/field", r.lattice_field(g, lo, step, i), pts, rays)

    L.rm_release_workspaces(None)
    two = Scene(text=TWO_SOLIDS)
    scene("two_solids", two.tables(64, 36), abi.default_settings(), ((-1.6, -0.8, -0.8), (1.6, 0.8, 0.8)))
    two.close()
    scene("bulb", scenes.mandelbulb(64, 36), abi.default_settings(fractalIters=12), ((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)))
    scene("sponge", scenes.mengersponge(64, 36), abi.default_settings(mengerLevels=5), ((-0.7, -0.7, -0.7), (0.7, 0.7, 0.7)))

    rng = np.random.default_rng(12)
    n = 70000
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = rng.uniform(-3, 3, (n, 3))
    rays[:, 3] = 100.0
    d = rng.normal(size=(n, 3))
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[::997, 4:7] = 0.0  # invalid rays sort last
    order, srt, keys = r.order_rays(rays, keys=True)
    done("rays_order", order=order, sorted=srt, keys=keys)

    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
    print(f"{len(record)} records → {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
