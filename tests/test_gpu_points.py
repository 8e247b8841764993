"""rm_shade_points / Renderer.shade_points on the GPU: the eight words of the surface point, the ambient occlusion and the four words
of the colour of every point bit for bit against the specification (tests/points_spec/rm_points_spec.c: the header's definition
restated with the oracle's own functions and tied to the shade and trace specs by tests/test_points_spec.py) — for each of the four
kernel classes, on hit points, surface-nets vertices, points deep inside and far outside, with every kind of invalid point and view
in every wave, at point counts around the wave and workgroup sizes, into poisoned, guarded buffers.  Then: projection, every subset
of outputs, two streams, other neighbours, and bake_mesh through the Python layer."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

import helpers as h
import points_helpers as PH
import scene_builders as SB
import sdf_helpers as F
import shade_helpers as S
from raymarcher_amd import abi, lib, mesh_bounds, write_ply_ex

pytestmark = pytest.mark.gpu

N = 257
SIZES = (1, 63, 64, 65, N)
FAR = 100.0
INF = float("inf")
ds = abi.default_settings


def _bulb_sponge(W, H):
    """A bulb, then a sponge beside it: UB3, the trap every hit reads is the sponge's, the last fractal evaluated."""
    cam = h.make_camera((0, 0.3, 5.5), (0, -0.05, -1), (0, 1, 0), 40.0, W, H)
    mat = dict(ambient=(.3, .3, .3), diffuse=(1, 1, 1), specular=(1, 1, 1), shininess=30.0)
    objs = (abi.RmObject * 2)(h.make_object(abi.RM_MANDELBULB, model=h.translate(-1.1, 0, 0), **mat),
                              h.make_object(abi.RM_MENGERSPONGE, model=h.translate(1.1, 0, 0) @ h.rotation((0, 1, 0), 0.4), **mat))
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.4, -1, -0.6)),
                               h.make_light(abi.RM_LIGHT_POINT, (.8, .8, 1), pos=(2, 3, 4), func=(0.6, 0.05, 0.0)))
    return cam, objs, 2, lights, 2, h.make_globals(itime=2.5)


def _bulb_lights(builder, W, H):
    """The builder's bulb under a directional and a point light: the bulb classes off the shadow pool."""
    sc = builder(W, H)
    lights = (abi.RmLight * 2)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (0.2, -1, -0.5)),
                               h.make_light(abi.RM_LIGHT_POINT, (1, .9, .8), pos=(1.5, 2.0, 3.0), func=(0.7, 0.05, 0.0)))
    return sc[:3] + (lights, 2) + sc[5:]


def _empty(W, H):
    objs, _ = h.table([])
    return h.make_camera((0, 0, 4.5), (0, 0, -1), (0, 1, 0), 30.0, W, H), objs, 0, None, 0, h.make_globals()


# name → (kernel class, builder(W, H) → (scene, settings, resources)).  Class: 0 the table walk, 1 the general bulb, 2 the plain bulb,
# "tex" the samplers' kernel.  The bulb classes: hard shadows from directional lights (the pool), with bump and AO on top, and soft
# shadows with a point light (getPhong).
BUMP = abi.RM_FEAT_PERLIN_BUMP | abi.RM_FEAT_REFERENCE_DEFAULT
CASES = {
    "walk_soft_ao": (0, lambda W, H: (SB.directional_light_2(W, H), ds(enableSoftShadow=1, enableAmbientOcclusion=1), {})),
    "walk_bump": (0, lambda W, H: (SB.all_primitives_scene(W, H), ds(features=BUMP, mengerLevels=3, fractalIters=6), {})),
    "bulb_sponge": (0, lambda W, H: (_bulb_sponge(W, H), ds(mengerLevels=3, fractalIters=6), {})),
    "plain_bulb": (2, lambda W, H: (h.scene_mandelbulb(W, H), ds(fractalIters=8), {})),
    "plain_bulb_bump_ao": (2, lambda W, H: (h.scene_mandelbulb(W, H), ds(fractalIters=8, features=BUMP, enableAmbientOcclusion=1), {})),
    "plain_bulb_soft": (2, lambda W, H: (_bulb_lights(h.scene_mandelbulb, W, H), ds(fractalIters=8, enableSoftShadow=1), {})),
    "moved_bulb": (1, lambda W, H: (SB.moved_bulb_scene(W, H), ds(fractalIters=8), {})),
    "moved_bulb_point": (1, lambda W, H: (_bulb_lights(SB.moved_bulb_scene, W, H), ds(fractalIters=8, enableAmbientOcclusion=1), {})),
    "tex": ("tex", lambda W, H: (SB.textured_scene(W, H), ds(features=abi.RM_FEAT_WHITE_BACKGROUND),
                                 {"textures": SB.synthetic_textures()})),
    "area_light": ("tex", lambda W, H: SB.resource_case("area_light_bump_ao", W, H)),
    "empty": (0, lambda W, H: (_empty(W, H), ds(), {})),
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name][1](40, 40)


@functools.lru_cache(maxsize=None)
def points_of(name):
    """The case's N seeded points and views (read-only, shared)."""
    scene, s, _ = case(name)
    pts, views = PH.point_set(scene, s, N, 3000 + NAMES.index(name))
    pts.setflags(write=False)
    views.setflags(write=False)
    return pts, views


@functools.lru_cache(maxsize=None)
def spec_of(name, view, project=0, max_move=INF):
    """The specification's three outputs for the case's points, computed once and shared (read-only)."""
    scene, s, res = case(name)
    pts, views = points_of(name)
    out = PH.spec_points(scene, s, pts, view=views if view else None, far=FAR, project=project, max_move=max_move, res=res)
    for a in out:
        a.setflags(write=False)
    return out


def points_guarded(renderer, scene, s, res, pts, views=None, outputs="sac", project=0, max_move=INF, iso=0.001, far=FAR, stream=None):
    """rm_shade_points into poisoned, guarded buffers → (surface, ao, colour, check): device tensors (None where not asked for) and
    the function that checks every guard and that every word was written, then returns the three as numpy."""
    dev = renderer.device
    p = torch.from_numpy(np.array(pts)).to(dev)
    v = None if views is None else torch.from_numpy(np.array(views)).to(dev)
    n = len(pts)
    bufs = {"s": h.guarded((n, 8), device=dev), "a": h.guarded((n,), device=dev), "c": h.guarded((n, 4), device=dev)}
    ptr = lambda k: C.c_void_p(bufs[k][0].data_ptr()) if k in outputs else None  # noqa: E731
    t = S.tables_of(scene, res)
    r, _keep = renderer._resources(t)
    ps = abi.RmPointsSettings(far, iso, max_move, project)
    if stream is not None:  # the uploads and the poison fills above ran on the current stream
        stream.wait_stream(torch.cuda.current_stream(dev))
    st = lib().rm_shade_points(C.c_void_p(p.data_ptr()), C.c_void_p(v.data_ptr()) if v is not None else None, n, C.byref(ps), t.objects,
                               t.num_objects, t.lights, t.num_lights, C.byref(t.globals_), C.byref(s), C.byref(r), ptr("s"), ptr("a"),
                               ptr("c"), C.c_void_p(stream.cuda_stream) if stream is not None else renderer._stream())
    assert st == abi.RM_OK, lib().rm_last_error().decode()
    assert lib().rm_debug_last_path() == PH.PATH_POINTS == abi.RM_PATH_SHADE_POINTS and lib().rm_debug_last_split() == 0

    alive = (p, v, t, r, _keep)  # the caching allocator orders reuse on the CURRENT stream only: the inputs live until the check

    def check():
        if stream is not None:
            stream.synchronize()
        assert alive
        got = []
        for k in "sac":
            if k in outputs:
                bufs[k][1]()
                got.append(bufs[k][0].cpu().numpy())
            else:
                assert bool((bufs[k][0].view(torch.int32) == h._i32(h.FLOAT_POISON)).all()), f"output {k} was not asked for"
                got.append(None)
        return got
    return check


def assert_outputs(got, want, what):
    """Word for word, but for a NaN the arithmetic GENERATES in a colour: the contract (oracle/rm_math.h) fixes no sign or payload
    for it — x86 writes the default NaN with the sign bit set, gfx950 with it clear — so where the spec's colour word is a NaN the
    kernel's must be one, and every other word is compared in every bit.  (The area light seen head-on: LTC_Evaluate's tangent
    frame normalises V − N·(N·V), a zero vector where V = N exactly.)  The markers −1 and RM_RAY_INVALID are stored, not generated."""
    for a, b, name in zip(got, want, ("surface", "ao", "colour")):
        if a is None:
            continue
        if name == "colour" and np.isnan(b).any():
            nan = np.isnan(b)
            assert (np.isnan(a) == nan).all(), f"{what} colour: NaN words at other places than the spec's"
            a, b = np.where(nan, np.float32(0), a), np.where(nan, np.float32(0), b)
        h.assert_bit_equal(a, b, f"{what} {name}")


# ---------------------------------------------------------------- the kernel equals the specification in every word
@pytest.mark.parametrize("view", [True, False], ids=["view", "head_on"])
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_spec_in_every_bit(renderer, name, view):
    scene, s, res = case(name)
    cls = CASES[name][0]
    if cls != "tex":
        kind = 0 if scene[2] != 1 or scene[1][0].type != abi.RM_MANDELBULB else (2 if lib().rm_debug_bulb_plain(scene[1], 1, C.byref(scene[5])) else 1)
        assert kind == cls, "the case is not of the class it is listed under"
    else:
        assert S.class_of(scene, s)[2] == 1
    pts, views = points_of(name)
    want = spec_of(name, view)
    ids = PH.ids_of(want[0])
    assert (ids == abi.RM_RAY_INVALID).sum() >= (32 if view else 14), "invalid points in every wave"
    if name != "empty":
        assert (ids >= 0).sum() >= 150 and len(np.unique(want[2], axis=0)) > 50 and len(np.unique(want[1])) > 20
        assert (want[0][ids >= 0, 3] < -0.05).any() and (want[0][ids >= 0, 3] > 10.0).any(), "points deep inside and far outside"
    else:
        assert (ids[ids != abi.RM_RAY_INVALID] == -1).all()
    for n in SIZES:
        got = points_guarded(renderer, scene, s, res, pts[:n], views[:n] if view else None)()
        assert_outputs(got, [w[:n] for w in want], f"{name} {n} points")


# ---------------------------------------------------------------- projection
@pytest.mark.parametrize("max_move", [INF, 0.02], ids=["unbounded", "max_move"])
@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("name", ["walk_soft_ao", "walk_bump", "plain_bulb", "moved_bulb_point", "tex", "empty"])
def test_projection_equals_the_spec(renderer, name, steps, max_move):
    scene, s, res = case(name)
    pts, views = points_of(name)
    want = spec_of(name, True, steps, max_move)
    got = points_guarded(renderer, scene, s, res, pts, views, project=steps, max_move=max_move)()
    assert_outputs(got, want, f"{name} {steps} steps")
    if name != "empty":
        moved = np.linalg.norm(want[0][:, 4:7].astype(np.float64) - pts[:, 0:3].astype(np.float64), axis=1)
        ok = PH.ids_of(want[0]) >= 0
        assert (moved[ok] > 0).sum() > 100 and (max_move == INF or moved[ok].max() <= max_move * (1 + 1e-6))


# ---------------------------------------------------------------- every subset of outputs
@pytest.mark.parametrize("name", ["walk_soft_ao", "plain_bulb_bump_ao", "moved_bulb", "area_light"])
def test_every_subset_of_outputs_holds_the_same_bits(renderer, name):
    scene, s, res = case(name)
    pts, views = points_of(name)
    want = spec_of(name, True, 1)
    for k in (1, 2, 3):
        for outs in itertools.combinations("sac", k):
            got = points_guarded(renderer, scene, s, res, pts, views, outputs="".join(outs), project=1)()
            assert [g is not None for g in got] == [c in outs for c in "sac"]
            assert_outputs(got, want, f"{name} outputs {outs}")


# ---------------------------------------------------------------- launch state: two streams, other neighbours
def test_two_streams_keep_their_tables_apart(renderer):
    names = ["walk_soft_ao", "plain_bulb", "tex", "moved_bulb_point"]
    streams = [torch.cuda.Stream(device=renderer.device) for _ in range(2)]
    torch.cuda.synchronize()
    checks = []
    for i, name in enumerate(names):  # nothing waits between the four
        scene, s, res = case(name)
        pts, views = points_of(name)
        checks.append(points_guarded(renderer, scene, s, res, pts, views, stream=streams[i % 2]))
    for name, check in zip(names, checks):
        assert_outputs(check(), spec_of(name, True), f"{name} among four calls on two streams")


@pytest.mark.parametrize("name", ["plain_bulb", "plain_bulb_bump_ao", "walk_soft_ao", "bulb_sponge"])
def test_a_points_result_does_not_depend_on_its_neighbours(renderer, name):
    """The pooled bulb class marches a point's shadow rays on whichever lane of the wave is idle, and the table walk switches
    wave-uniform paths on what the lanes of a wave agree on: other neighbours must not change a bit of any point's result."""
    scene, s, res = case(name)
    pts, views = points_of(name)
    want = spec_of(name, True)
    perm = np.random.default_rng(77).permutation(N)
    got = points_guarded(renderer, scene, s, res, pts[perm], views[perm])()
    assert_outputs(got, [w[perm] for w in want], f"{name} shuffled")
    # the first 40 points alone, and among far-away and invalid points only
    got = points_guarded(renderer, scene, s, res, pts[:40], views[:40])()
    assert_outputs(got, [w[:40] for w in want], f"{name} alone")
    other = np.concatenate([pts[:40], pts[(np.arange(N) % 8 == 5) | (np.arange(N) % 8 == 6)]])
    other_v = np.concatenate([views[:40], views[(np.arange(N) % 8 == 5) | (np.arange(N) % 8 == 6)]])
    got = points_guarded(renderer, scene, s, res, other, other_v)()
    assert_outputs([g[:40] for g in got], [w[:40] for w in want], f"{name} among strangers")


# ---------------------------------------------------------------- the Python layer
def test_shade_points_takes_arrays_and_tensors_of_three_or_four(renderer):
    name = "walk_soft_ao"
    scene, s, res = case(name)
    pts, views = points_of(name)
    t = S.tables_of(scene, res)
    want = spec_of(name, True)
    normal, dist, pos, oid, ao, col = renderer.shade_points(t, s, np.array(pts[:, 0:3]), view=torch.from_numpy(np.array(views)).to(renderer.device),
                                                            far=FAR, ao=True)
    assert lib().rm_debug_last_path() == abi.RM_PATH_SHADE_POINTS
    assert normal.shape == (N, 3) and dist.shape == (N,) and pos.shape == (N, 3) and oid.dtype == torch.int32 and col.shape == (N, 4)
    got = np.concatenate([normal.cpu().numpy(), dist.cpu().numpy()[:, None], pos.cpu().numpy()], axis=1)
    h.assert_bit_equal(got, want[0][:, 0:7], "surface")
    assert (oid.cpu().numpy() == PH.ids_of(want[0])).all()
    h.assert_bit_equal(ao.cpu().numpy(), want[1], "ao")
    h.assert_bit_equal(col.cpu().numpy(), want[2], "colour")
    out = renderer.shade_points(t, s, np.array(pts), colour=False)
    assert out[4] is None and out[5] is None
    h.assert_bit_equal(out[1].cpu().numpy(), spec_of(name, False)[0][:, 3], "distance alone")
    with pytest.raises(ValueError):
        renderer.shade_points(t, s, np.zeros((4, 2), dtype=np.float32))
    with pytest.raises(ValueError):
        renderer.shade_points(t, s, np.array(pts), view=np.array(views[:5]))


def test_bake_mesh_of_a_sphere_and_a_cube(renderer, tmp_path):
    objs, no, g, s = F.scene("sphere_cube")
    lights = (abi.RmLight * 1)(h.make_light(abi.RM_LIGHT_DIRECTIONAL, (1, 1, 1), (-0.3, -1, -0.5)))
    for i in range(no):
        for k in range(3):
            objs[i].cAmbient[k], objs[i].cDiffuse[k] = 0.3, 0.8
    scene = (h.make_camera((0, 0, 5), (0, 0, -1), (0, 1, 0), 40.0, 8, 8), objs, no, lights, 1, g)
    t = S.tables_of(scene)
    v0, q0, o0 = renderer.scene_mesh(t, s, 12)
    verts, quads, oid, normals, ao, rgb = renderer.bake_mesh(t, s, 12)
    n = v0.shape[0]
    assert n > 50 and verts.shape == (n, 4) and normals.shape == (n, 3) and ao.shape == (n,) and rgb.shape == (n, 3)
    assert rgb.dtype == torch.uint8 and oid.dtype == torch.int32
    assert torch.equal(quads, q0) and torch.equal(oid, o0), "the mesh is scene_mesh's, and no vertex changed its object"
    nn, d0 = normals.cpu().numpy().astype(np.float64), v0.cpu().numpy()
    assert np.abs(np.linalg.norm(nn, axis=1) - 1.0).max() <= 2.0 ** -22, "unit normals (one float32 normalize)"
    # the projected vertices are the spec's, nearer the surface than surface nets left them, and within half a cell's diagonal
    lo, hi = (np.asarray(b, dtype=np.float64) for b in mesh_bounds(t))
    step = float((hi - lo).max()) / 9
    want = PH.spec_points(scene, s, d0, far=scene[0].initialFar, project=2, max_move=0.5 * step * 3.0 ** 0.5)
    h.assert_bit_equal(verts.cpu().numpy()[:, 0:3], want[0][:, 4:7], "projected vertices")
    h.assert_bit_equal(normals.cpu().numpy(), want[0][:, 0:3], "normals")
    h.assert_bit_equal(ao.cpu().numpy(), want[1], "ao")
    before = np.abs(PH.spec_points(scene, s, d0, outputs="s")[0][:, 3] - np.float32(0.001))
    after = np.abs(want[0][:, 3] - np.float32(0.001))
    assert after.max() < before.max() / 4 and (np.linalg.norm(want[0][:, 4:7] - d0[:, 0:3], axis=1) <= 0.5 * step * 3.0 ** 0.5 * (1 + 1e-6)).all()
    # the colours are to_rgba8's of the spec's colours
    col8 = renderer.to_rgba8(torch.from_numpy(want[2]).to(renderer.device).view(1, n, 4))[0, :, 0:3]
    assert torch.equal(rgb, col8) and len(torch.unique(rgb, dim=0)) > 10
    # PLY round trip
    path = write_ply_ex(tmp_path / "baked.ply", verts, quads, colours=rgb, normals=normals)
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + 11
    head = raw[:end].decode()
    assert f"element vertex {n}\n" in head and f"element face {quads.shape[0]}\n" in head and "property float nx" in head
    rec = np.frombuffer(raw, dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]), count=n, offset=end)
    h.assert_bit_equal(rec["p"], verts.cpu().numpy()[:, 0:3], "ply positions")
    h.assert_bit_equal(rec["n"], normals.cpu().numpy(), "ply normals")
    assert (rec["c"] == rgb.cpu().numpy()).all()
    faces = np.frombuffer(raw, dtype=np.dtype([("k", "u1"), ("i", "<i4", 4)]), count=quads.shape[0], offset=end + n * 27)
    assert (faces["i"] == quads.cpu().numpy()).all() and end + n * 27 + quads.shape[0] * 17 == len(raw)


# ---------------------------------------------------------------- refusals that need the device
def test_host_pointers_are_refused_and_nothing_is_written(renderer):
    scene, s, res = case("walk_soft_ao")
    _, objs, no, lights, nl, g = scene
    n = 64
    dev = renderer.device
    pts = torch.from_numpy(np.array(points_of("walk_soft_ao")[0][:n])).to(dev)
    sf, check_s = h.guarded((n, 8), device=dev)
    ao, check_a = h.guarded((n,), device=dev)
    col, check_c = h.guarded((n, 4), device=dev)
    host = np.zeros(n * 8 + 8, dtype=np.float32)
    hp = (host.ctypes.data + 15) & ~15
    ps = abi.RmPointsSettings(FAR, 0.001, INF, 0)

    def call(p, v, a, b, c):
        q = lambda x: C.c_void_p(x) if x else None  # noqa: E731
        return lib().rm_shade_points(q(p), q(v), n, C.byref(ps), objs, no, lights, nl, C.byref(g), C.byref(s), None, q(a), q(b), q(c), None)

    good = (pts.data_ptr(), 0, sf.data_ptr(), ao.data_ptr(), col.data_ptr())
    for k, word in enumerate(("d_points", "d_view", "d_surface", "d_ao", "d_rgba")):
        args = list(good)
        args[k] = hp
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    torch.cuda.synchronize()
    for buf in (sf, ao, col):
        assert bool((buf.view(torch.int32) == h._i32(h.FLOAT_POISON)).all()), "a refused call wrote something"
    assert call(*good) == abi.RM_OK
    check_s(), check_a(), check_c()
