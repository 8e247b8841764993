"""The single-Mandelbulb kernel's two forms — plain (invModel 1 on the diagonal and ±0 elsewhere, scaleFactor 1, power 8, no
Julia seed: no object transform, ·scaleFactor or Julia select per evaluation) and general — and the iteration's single range
guard (mx = max(|w.x|, |w.z|) >= 2^-48 and m < inf selects the unguarded step), bit for bit against the oracle: the headline bulb with the identity and with translated, rotated and scaled models, Julia on and
off, views whose rays and iterates run along the coordinate axes (w.x = w.z = 0, ±0 coordinates), with and without secondary
rays, soft shadows and ambient occlusion."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
from helpers import assert_bit_equal, tables_of
from scene_builders import bulb_scene
from raymarcher_amd import abi, lib

pytestmark = pytest.mark.gpu


CASES = {
    "identity": dict(),
    "translated": dict(model=h.translate(0.25, -0.1, 0.0)),
    "rotated": dict(model=h.rotation((1, 2, 0.5), 0.6)),
    "scaled": dict(model=h.scale(1.3, 1.3, 1.3), sf=1.3),
    "julia": dict(julia=(0.35, -0.2)),
    "julia_translated": dict(model=h.translate(0.0, 0.2, 0.0), julia=(0.4, -0.3)),
    # views along the axes: the centre rays (odd frame sizes) and their iterates have x = z = 0 or ±0 coordinates
    "down_the_y_axis": dict(pos=(0, 4.5, 0), look=(0, -1, 0), up=(0, 0, -1)),
    "down_the_x_axis": dict(pos=(-4.5, 0, 0), look=(1, 0, 0)),
    "along_the_z_axis_from_behind": dict(pos=(0, 0, -4.5), look=(0, 0, 1)),
}


PLAIN = ("identity", "down_the_y_axis", "down_the_x_axis", "along_the_z_axis_from_behind")


@pytest.mark.parametrize("name", sorted(CASES))
def test_bulb_forms_bit_exact(renderer, name):
    W, H = 63, 35
    scene = bulb_scene(W, H, **CASES[name])
    assert lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5])) == int(name in PLAIN)
    s = abi.default_settings()
    assert_bit_equal(renderer.render(tables_of(scene), s, W, H).cpu().numpy(), h.oracle_render(scene, s, W, H), name)


@pytest.mark.parametrize("name", ["identity", "julia", "rotated"])
def test_bulb_forms_with_secondary_rays_and_soft_shadows(renderer, name):
    """The secondary-ray instantiation, and the soft-shadow / AO marches (not the hard-shadow queue)."""
    W, H = 47, 33
    scene = bulb_scene(W, H, refl=(.4, .4, .4), **CASES[name])
    for over in ({"enableReflection": 1, "numReflection": 1}, {"enableSoftShadow": 1, "enableAmbientOcclusion": 1}):
        s = abi.default_settings(**over)
        assert_bit_equal(renderer.render(tables_of(scene), s, W, H).cpu().numpy(), h.oracle_render(scene, s, W, H),
                         f"{name} {over}")


def _signed_zero_identity(scene, seed):
    """The same bulb with random signs on the zeros of invModel (the plain form; the transform returns −0 or +0 per coordinate
    depending on the signs of the other coordinates)."""
    rng = np.random.default_rng(seed)
    o = scene[1][0]
    for i in (1, 2, 4, 6, 8, 9, 12, 13, 14):
        o.invModel[i] = -0.0 if rng.random() < 0.5 else 0.0
    return scene


@pytest.mark.parametrize("seed", range(4))
def test_plain_form_with_signed_zeros_on_the_axes(renderer, seed):
    """Views down each axis, so that pixels' rays, march points, normal taps and shadow origins have zero coordinates, with the
    zeros of invModel of either sign: the plain kernel (which reads p itself) against the oracle (which runs the transform)."""
    W, H = 63, 35
    for k, view in enumerate((dict(), dict(pos=(0, 4.5, 0), look=(0, -1, 0), up=(0, 0, -1)), dict(pos=(-4.5, 0, 0), look=(1, 0, 0)))):
        scene = _signed_zero_identity(bulb_scene(W, H, **view), 10 * seed + k)
        assert lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5])) == 1
        for s in (abi.default_settings(), abi.default_settings(features=abi.RM_FEAT_REFERENCE_DEFAULT | abi.RM_FEAT_BULB_POWER8_ALGEBRAIC)):
            assert_bit_equal(renderer.render(tables_of(scene), s, W, H).cpu().numpy(), h.oracle_render(scene, s, W, H),
                             f"seed {seed} view {k} features {s.features}")
