"""The HIP kernels' resource-reading paths — random-byte textures through the uv maps, random-byte sky-box faces, area lights with the
reference's 8-bit LTC tables, emissive rectangles, BrightColor — held DIRECTLY to the independent NumPy float64 arbiter, with the same
margins and assertions as tests/test_resource_arbiter.py, on the shapes where the launch code differs: ragged frames, guarded whole
frames, a row range off the tile grid, rm_render_batch with per-frame cameras, bright output on.  Every frame is also bit-equal to
the oracle (cheap, and it says which side moved if the arbiter check fails).  Inputs come from tests/golden or a seed."""
import numpy as np
import pytest

import arbiter_numpy as an
import helpers as h
import test_resource_arbiter as ra
from raymarcher_amd import abi

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(case, tables, settings, W, H, res, got, got_b, rows=(0, None), max_exc=3):
    r0, r1 = rows[0], H if rows[1] is None else rows[1]
    scene = (tables.camera, tables.objects, tables.num_objects, tables.lights, tables.num_lights, tables.globals_)
    kw = {k: v for k, v in res.items() if k != "textures"}
    o32, b32 = h.oracle_render(scene, settings, W, H, row0=r0, row1=r1, bright=True, textures=res.get("textures"), **kw)
    assert (_bits(got) == _bits(o32)).all() and (_bits(got_b) == _bits(b32)).all(), f"{case}: the HIP frame differs from the oracle"
    f64, _hit, info = an.render_frame_table(tables, settings, W, H, resources=res, diag=True)
    fj = an.render_frame_table(tables, settings, W, H, resources=res, jitter=ra.JITTER)[0]
    c64 = h.arbiter_render(scene, settings, W, H, row0=r0, row1=r1, textures=res.get("textures"), **kw)
    sl = slice(r0, r1)
    info = {k: v[sl] for k, v in info.items()}
    ra.explain(case, f64[sl], info, np.abs(fj - f64).max(-1)[sl], got, got_b, c64, max_exc)


def _tables_with(t, res):
    t.textures, t.skybox = res.get("textures"), res.get("skybox")
    t.ltc1, t.ltc2 = res.get("ltc1"), res.get("ltc2")
    return t


def _textured(W, H):
    t = ra.textured_scene(W, H, (7.0, -3.0), 1.0)
    res = {"textures": [ra.random_image(64, 64, 90 + i) if i % 2 == 0 else ra.random_image(3, 7, 90 + i) for i in range(5)]}
    return _tables_with(t, res), res


def _sky(W, H):
    t = ra.skybox_scene(W, H, (0, 0, 0), (1, 1, 1), 100.0)
    res = {"skybox": ra.random_faces(5, 3)}
    return _tables_with(t, res), res


def _area(W, H, two_sided=0):
    t = ra.area_scene(W, H, two_sided)
    l1, l2 = ra.fixture_ltc()
    res = {"ltc1": l1, "ltc2": l2}
    return _tables_with(t, res), res


@pytest.mark.parametrize("shape", [(203, 117), (5, 3)])
@pytest.mark.parametrize("kind", ["textures", "sky", "area"])
def test_ragged_guarded_frames_against_the_arbiter(renderer, kind, shape):
    """Whole frames of ragged sizes into poisoned, guarded buffers (render_guarded), bright on."""
    W, H = shape
    t, res = {"textures": _textured, "sky": _sky, "area": _area}[kind](W, H)
    s = {"textures": abi.default_settings(enableSoftShadow=1),
         "sky": abi.default_settings(enableSkyBox=1, enableReflection=1, features=abi.RM_FEAT_WHITE_BACKGROUND),
         "area": abi.default_settings(enableReflection=1)}[kind]
    out, br = h.render_guarded(renderer, t, s, W, H, bright=True)
    # measured on 203×117: 0 / 23 / 0 explained exceptions (the sky seen in the mirrors: ill-conditioned)
    _check(f"{kind} {W}x{H}", t, s, W, H, res, out.cpu().numpy(), br.cpu().numpy(), max_exc={"textures": 4, "sky": 30, "area": 4}[kind])


@pytest.mark.parametrize("kind", ["textures", "area"])
def test_row_range_off_the_tile_grid(renderer, kind):
    W, H = 80, 48
    t, res = _textured(W, H) if kind == "textures" else _area(W, H, two_sided=1)
    s = abi.default_settings(enableAmbientOcclusion=1)
    out, br = h.render_guarded(renderer, t, s, W, H, row_begin=7, row_end=30, bright=True)
    _check(f"{kind} rows 7-30", t, s, W, H, res, out.cpu().numpy(), br.cpu().numpy(), rows=(7, 30))


def test_batch_cameras_across_a_seam_and_a_cube_edge(renderer):
    """rm_render_batch: one scene with random-byte textures and sky-box faces, four cameras that sweep across the side maps' seam and
    the cube map's x/y/z corner; each frame against the oracle bit for bit and against the arbiter."""
    W, H = 48, 32
    t, res = _textured(W, H)
    res["skybox"] = ra.random_faces(5, 4)
    t.skybox = res["skybox"]
    s = abi.default_settings(enableSkyBox=1, features=abi.RM_FEAT_WHITE_BACKGROUND)
    poses = [((0.4, 1.9, 5.0), (0, -0.35, -1)), ((2.5, 1.5, 4.0), (-0.4, -0.3, -1)), ((-2.0, 2.5, 3.0), (0.5, -0.6, -1)),
             ((0.0, 0.5, 3.5), (1, 1, -1))]
    cams = [h.make_camera(p, l, (0, 1, 0), 60.0, W, H) for p, l in poses]
    out, br = renderer.render_batch(t, s, W, H, cams, bright=True)
    out, br = out.cpu().numpy(), br.cpu().numpy()
    for i, cam in enumerate(cams):
        t.camera = cam
        _check(f"batch frame {i}", t, s, W, H, res, out[i], br[i], max_exc=4)
