"""rm_render on frames whose 8×8 tiles (one wave each) exercise every branch of the lattice-sharing bump gradient, fragColor and
BrightColor against the oracle, word for word.  An offset sample of bumpNormal is taken from the base sample's noise lattice when
no hit lane of the wave leaves its cell on that axis, and from pnoise otherwise: the frames below hold tiles where no lane, some
lanes and every lane crosses, on each axis, and the coverage is asserted from the oracle's own hit points (the position plane of
the G-buffer specification, tests/gbuffer_helpers.py), not from the device.

The two zoomed frames have the pixel pitch of the 3840×2160 headline frame (30° over 2160 rows ≈ 1.8° over 128).  The general
class (a rotated, translated bulb; it runs the same pooled surface phase) brings whole tiles across a z lattice plane — the plain
bulb's front is too curved for that at this pitch — and, moved to x ≈ 25.6, the wrap of the lattice's mod 256.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import gbuffer_helpers as gh
import helpers as h
from helpers import assert_bit_equal, tables_of
from raymarcher_amd import abi, scenes

pytestmark = pytest.mark.gpu

ROOT = h.ROOT
F = np.float32
GENERAL = dict(rot=((0, 0, 1), 0.3), tz=0.015, angle=0.6)
# name: (W, H, camera position, look-at point, height angle in degrees, model matrix of the bulb or None for the scene's own)
FRAMES = {
    "zoom on the origin": (256, 128, (0, 0, 4.5), (0, 0, 0), 1.8, None),
    "zoom on the shoulder": (256, 128, (0, 0, 4.5), (0.55, 0.6, 0), 1.8, None),
    "whole bulb": (128, 64, (0, 0, 4.5), (0, 0, 0), 30.0, None),
    "ragged": (130, 70, (0, 0, 4.5), (0, 0, 0), 30.0, None),
    "general class at a z plane": (64, 32, (0, 0, 4.5), (0, 0, 0), GENERAL["angle"], (0.0, 0.0, GENERAL["tz"])),
    "general class at the x wrap": (64, 32, (25.6, 0, 4.5), (25.6, 0, 0), GENERAL["angle"], (25.6, 0.0, GENERAL["tz"])),
}
BULB_FRAMES = ("zoom on the origin", "zoom on the shoulder", "whole bulb")


def scene_of(name):
    W, H, pos, target, angle, move = FRAMES[name]
    t = scenes.mandelbulb(W, H)
    cam = h.make_camera(pos, tuple(np.subtract(target, pos)), (0, 1, 0), angle, W, H)
    objs = t.objects
    if move is not None:
        model = h.translate(*move) @ h.rotation(*GENERAL["rot"])
        objs = (abi.RmObject * 1)(h.make_object(abi.RM_MANDELBULB, model=model, ambient=(.3, .3, .3), diffuse=(1, 1, 1),
                                                specular=(1, 1, 1), shininess=100.0, ior=1.5))
    return (cam, objs, 1, t.lights, t.num_lights, t.globals_), W, H


def tile_classes(name):
    """(3, 3) counts over the frame's 8×8 tiles that hold a hit: [axis][no hit lane crosses, some do, all do], and the scaled hit
    points — crossing = floor(ps_k + 0.1f) != floor(ps_k) with ps = 10 p in float32, p the oracle's hit point."""
    scene, W, H = scene_of(name)
    _, ids, pos = gh.spec_gbuffer(scene[0], scene[1], 1, scene[5], abi.default_settings(), W, H)
    ps = (pos[..., :3] * F(10)).astype(F)
    cross = np.floor((ps + F(0.1)).astype(F)) != np.floor(ps)
    hit = ids >= 0
    out = np.zeros((3, 3), dtype=int)
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            m = hit[ty:ty + 8, tx:tx + 8]
            if m.any():
                c = cross[ty:ty + 8, tx:tx + 8][m]
                for k in range(3):
                    n = c[:, k].sum()
                    out[k, 0 if n == 0 else (2 if n == len(c) else 1)] += 1
    return out, ps[hit]


def check(renderer, name):
    scene, W, H = scene_of(name)
    s = abi.default_settings()
    assert s.features & abi.RM_FEAT_PERLIN_BUMP
    ref, ref_bright = h.oracle_render(scene, s, W, H, bright=True)
    out, bright = h.render_guarded(renderer, tables_of(scene), s, W, H, bright=True)
    assert_bit_equal(out.cpu().numpy(), ref, f"{name}: fragColor")
    assert_bit_equal(bright.cpu().numpy(), ref_bright, f"{name}: BrightColor")


def test_the_frames_hold_every_class_of_tile():
    total = np.zeros((3, 3), dtype=int)
    for name in BULB_FRAMES:
        total += tile_classes(name)[0]
    assert (total[:, 0] >= 4).all() and (total[:, 1] >= 4).all(), total.tolist()  # none and mixed, every axis
    assert total[0, 2] >= 4 and total[1, 2] >= 4, total.tolist()                   # every lane crossing, x and y
    z, ps = tile_classes("general class at a z plane")
    assert z[2, 2] >= 4 and z[2, 1] >= 4, z.tolist()                                # every lane crossing on z, and mixed
    w, ps = tile_classes("general class at the x wrap")
    cells = np.floor(ps[:, 0])
    assert (cells == 255).any() and (cells == 256).any() and w[0, 1] + w[0, 2] >= 4, (w.tolist(), np.unique(cells).tolist())
    assert w[2, 2] >= 4, w.tolist()


@pytest.mark.parametrize("name", list(FRAMES))
def test_frame_matches_the_oracle(renderer, name):
    check(renderer, name)


_CHILD = r'''
import sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_bump_lattice as t
from raymarcher_amd import Renderer
r = Renderer(0)
for name in ("whole bulb", "ragged", "general class at a z plane"):
    t.check(r, name)
print("ok")
'''


@pytest.mark.parametrize("wpb", [2, 4])
def test_waves_per_block(wpb):
    """Two and four waves per workgroup: the ballots are per wave whatever the workgroup holds (the environment is read once per
    process, hence the child)."""
    env = dict(os.environ, RM_WAVES_PER_BLOCK=str(wpb))
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout[-1000:], p.stderr[-2000:])
