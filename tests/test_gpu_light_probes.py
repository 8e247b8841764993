"""rm_light_probes / Renderer.light_probes on the GPU: all forty words of every record bit for bit against two references — the NumPy
definition (tests/light_probes_spec.py: spec_shade's colours, spec_trace's hit flags, the leaves and the tree) and the composition
through the shipped entries (rm_shade_rays on the n·K rays, rm_trace_rays NO_NORMAL with tMax = far, the NumPy tree) — for every
case of shade_helpers.CASES, which covers the twelve kernel classes, at the smallest shapes at which each mechanism of the kernel can
go wrong (light_probes_helpers.SHAPES), with one and three sets, two probes with a non-finite position and one inside an object, a
table row with a zero and one with a NaN direction, into poisoned, guarded buffers.  Then: a caller's own table, probes asked alone,
the path, the memory the call allocates, and the refusals that need the device.

The shapes of more than 64 directions (n = 3 and n = 2 finite probes) carry their two non-finite probes on top of n: among two or
three probes they would leave one finite probe or none (light_probes_helpers.SHAPES)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers as h
import light_probes_helpers as M
import light_probes_spec as L
import shade_helpers as S
import trace_helpers as T
from raymarcher_amd import RaymarcherError, abi, lib, sphere_directions

pytestmark = pytest.mark.gpu

FAR = M.FAR
NAMES = list(S.CASES)
f32 = np.float32


@functools.lru_cache(maxsize=None)
def spec_of(name, K, n, sets, variant):
    """The definition's records of a case, shape, set count and table variant, computed once and shared (read-only)."""
    scene, s, res = S.case(name)
    want = L.probes(scene, s, res, M.positions(name, K, n), M.tables(K, sets)[variant][1], K, sets, FAR)
    want.setflags(write=False)
    return want


def probes_guarded(renderer, scene, s, res, positions, table, K, sets, far=FAR):
    """Renderer.light_probes into a poisoned, guarded buffer, checked → PROBE records."""
    out, check = h.guarded((len(positions), 40), device=renderer.device)
    sh, hits = renderer.light_probes(S.tables_of(scene, res), s, np.array(positions), directions=K, sets=sets, far=far, table=np.array(table), out=out)
    assert lib().rm_debug_last_path() == abi.RM_PATH_LIGHT_PROBES == 21 and lib().rm_debug_last_split() == 0
    check()
    assert sh.data_ptr() == out.data_ptr() and tuple(sh.shape) == (len(positions), 9, 4) and hits.dtype == torch.int32
    rec = np.frombuffer(out.cpu().numpy().tobytes(), L.PROBE, len(positions))
    assert (rec["hits"] == hits.cpu().numpy()).all() and (rec["sh"].view(np.uint32) == sh.cpu().numpy().view(np.uint32)).all()
    return rec


def composed(renderer, scene, s, res, positions, table, K, sets, far=FAR, first=0):
    """The same records through the shipped entries: rm_shade_rays and rm_trace_rays on the n·K rays, then the NumPy leaves and tree."""
    t = S.tables_of(scene, res)
    shade = lambda rays: renderer.shade_rays(t, s, rays, far=far).cpu().numpy()  # noqa: E731
    trace = lambda rays: renderer.trace_rays(t, s, rays, normals=False)[3].cpu().numpy()  # noqa: E731
    return L.probes(scene, s, res, positions, table, K, sets, far, shade=shade, trace=trace, first=first)


# ---------------------------------------------------------------- the kernel equals the definition and the composition in every word
@pytest.mark.parametrize("K, n", M.SHAPES)
@pytest.mark.parametrize("name", NAMES)
def test_kernel_equals_the_spec_and_the_composition_in_every_word(renderer, name, K, n):
    scene, s, res = S.case(name)
    assert S.class_of(scene, s) == S.CASES[name][0], "the case is not of the class it is listed under"
    positions = M.positions(name, K, n)
    assert (~L.valid_positions(positions)).sum() == 2
    for sets in M.SETS:
        for variant, (label, table) in enumerate(M.tables(K, sets)):
            what = f"{name}, K = {K}, {len(positions)} probes, {sets} sets, {label}"
            want = spec_of(name, K, n, sets, variant)
            got = probes_guarded(renderer, scene, s, res, positions, table, K, sets)
            L.assert_records_equal(got, want, what + ": against the definition")
            L.assert_records_equal(got, composed(renderer, scene, s, res, positions, table, K, sets), what + ": against the composition")
            bad = ~L.valid_positions(positions)
            assert (want["hits"][bad] == abi.RM_RAY_INVALID).all() and not L.as_words(want[bad])[:, :36].any()
            assert (want["reserved"] == 0).all() and (want["hits"][~bad] >= 0).all() and (want["hits"][~bad] <= K).all()
            if label == "bad rows" and name != "empty" and K >= 64:
                assert 0 < want["hits"][~bad].sum() < K * (~bad).sum(), "the case should hold hits and misses"
                assert len(np.unique(L.as_words(want[~bad])[:, 0])) == (~bad).sum(), "every probe should see another radiance"


def test_every_kernel_class_is_covered():
    assert S.CLASSES == sorted((b, e, t, c) for b, e, t in ((0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 0, 1), (0, 1, 1)) for c in (0, 1))


# ---------------------------------------------------------------- a caller's own table
@pytest.mark.parametrize("name, K, n, sets", [("generic_sec", 8, 19, 3), ("plain_bulb_nosec", 128, 3, 2), ("tex_sec", 64, 4, 1)])
def test_a_callers_own_table_of_other_basis_values(renderer, name, K, n, sets):
    """An ambient cube's clamped axes, negative and tiny weights, directions of other lengths: the kernel only multiplies and adds."""
    scene, s, res = S.case(name)
    rng = np.random.default_rng(31 + K)
    d = rng.normal(size=(K * sets, 3))
    d *= rng.uniform(0.3, 3.0, (K * sets, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    table = np.zeros((K * sets, 16), f32)
    table[:, 0:3] = d
    table[:, 4:7], table[:, 7:10] = np.maximum(d, 0), np.maximum(-d, 0)    # the six faces of an ambient cube
    table[:, 10], table[:, 11], table[:, 12] = -1.0 / K, 1e-38, rng.uniform(-2, 2, K * sets)
    table[:, 3], table[:, 13:16] = 7.0, np.nan
    positions = np.array(M.positions(name, 64 if K <= 64 else K, n + 2 if K <= 64 else n))
    want = L.probes(scene, s, res, positions, table, K, sets, FAR)
    got = probes_guarded(renderer, scene, s, res, positions, table, K, sets)
    L.assert_records_equal(got, want, f"{name}: a table of the caller's against the definition")
    L.assert_records_equal(got, composed(renderer, scene, s, res, positions, table, K, sets), f"{name}: … against the composition")


# ---------------------------------------------------------------- a probe does not depend on the probes it shares a call with
@pytest.mark.parametrize("name, K, n, sets", [("plain_bulb_sec", 2, 33, 1), ("generic_nosec", 16, 9, 3), ("moved_bulb_nosec", 128, 3, 1)])
def test_probes_asked_alone_equal_the_same_probes_of_a_call(renderer, name, K, n, sets):
    scene, s, res = S.case(name)
    positions = np.array(M.positions(name, K if K != 16 else 64, n if K != 16 else 5))
    if K == 16:
        positions = np.concatenate([positions, positions[::-1] * f32(0.5)])[:n]
    table = sphere_directions(K, sets)
    together = probes_guarded(renderer, scene, s, res, positions, table, K, sets)
    for i in range(len(positions)):
        own = table[(i % sets) * K:(i % sets + 1) * K]  # alone the probe is probe 0 and takes set 0: hand it its own set
        alone = probes_guarded(renderer, scene, s, res, positions[i:i + 1], own, K, 1)
        L.assert_records_equal(alone, together[i:i + 1], f"{name}: probe {i} alone")


# ---------------------------------------------------------------- the built table, the defaults, the memory
def test_the_built_table_defaults_and_memory(renderer):
    name, K, n = "generic_nosec", 64, 16
    scene, s, res = S.case(name)
    t = S.tables_of(scene, res)
    rng = np.random.default_rng(5)
    centre, radius = T.cull_bounds(scene[1], scene[2], scene[5])
    pos = np.zeros((n, 4), f32)
    pos[:, 0:3] = np.asarray(centre) + rng.uniform(-1, 1, (n, 3)) * radius
    dev = torch.from_numpy(pos).to(renderer.device)
    sh, hits = renderer.light_probes(t, s, dev, directions=K, far=FAR)  # builds and keeps the table
    assert tuple(sh.shape) == (n, 9, 4) and sh.dtype == torch.float32 and tuple(hits.shape) == (n,) and hits.dtype == torch.int32
    rec = np.zeros(n, L.PROBE)
    rec["sh"], rec["hits"] = sh.cpu().numpy(), hits.cpu().numpy()
    L.assert_records_equal(rec, L.probes(scene, s, res, pos, sphere_directions(K, 1), K, 1, FAR), "the built table")
    # (n, 3) positions and far=None: the scene camera's initialFar
    sh3, hits3 = renderer.light_probes(t, s, pos[:, 0:3], directions=K)
    rec["sh"], rec["hits"] = sh3.cpu().numpy(), hits3.cpu().numpy()
    L.assert_records_equal(rec, L.probes(scene, s, res, pos, sphere_directions(K, 1), K, 1, scene[0].initialFar), "far=None")
    del sh, hits, sh3, hits3
    # the call allocates its result and nothing else: n·160 B = 2560 B, five of the allocator's 512-byte blocks
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(renderer.device)
    sh, hits = renderer.light_probes(t, s, dev, directions=K, far=FAR)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated(renderer.device) - before == n * 160 == sh.numel() * 4 + hits.numel() * 4 * 4
    assert lib().rm_debug_last_path() == abi.RM_PATH_LIGHT_PROBES
    # no probes: nothing is launched, empty views come back
    sh0, hits0 = renderer.light_probes(t, s, np.zeros((0, 4), f32), directions=K)
    assert tuple(sh0.shape) == (0, 9, 4) and tuple(hits0.shape) == (0,)
    with pytest.raises(ValueError):
        renderer.light_probes(t, s, dev, directions=K, table=np.zeros((K, 15), f32))
    with pytest.raises(ValueError):
        renderer.light_probes(t, s, dev, directions=K, out=torch.empty((n, 36), device=renderer.device))
    with pytest.raises(RaymarcherError):
        renderer.light_probes(t, s, dev, directions=48)
    with pytest.raises(RaymarcherError):
        renderer.light_probes(t, s, dev, directions=K, far=float("nan"))


def test_single_frames_before_and_after_are_the_same_bits(renderer):
    W, H = 64, 36
    scene, s, res = S.case("generic_nosec", W, H)
    t = S.tables_of(scene, res)
    before = renderer.render(t, s, W, H).cpu().numpy()
    path, split = lib().rm_debug_last_path(), lib().rm_debug_last_split()
    for name in ("generic_sec", "plain_bulb_nosec"):
        sc, ss, rr = S.case(name)
        probes_guarded(renderer, sc, ss, rr, M.positions(name, 64, 5), sphere_directions(64, 1), 64, 1)
    after = renderer.render(t, s, W, H).cpu().numpy()
    assert lib().rm_debug_last_path() == path and lib().rm_debug_last_split() == split
    S.assert_bits(after, before, "a single frame around rm_light_probes")


# ---------------------------------------------------------------- refusals that need the device
def test_host_pointers_and_misaligned_tensors_are_refused(renderer):
    scene, s, res = S.case("generic_nosec")
    _, objs, no, lights, nl, g = scene
    n, K = 8, 16
    pos = torch.zeros((n + 1, 4), device=renderer.device)
    table = torch.from_numpy(sphere_directions(K, 1)).to(renderer.device)
    spare = torch.zeros((K + 1, 16), device=renderer.device)
    out, check = h.guarded((n, 40), device=renderer.device)  # refused calls touch nothing: the guards and the poison hold to the end
    host = np.zeros(4096, f32)
    hp = (host.ctypes.data + 15) & ~15

    def call(p, d, o):
        return lib().rm_light_probes(C.c_void_p(p), n, C.c_void_p(d), K, 1, FAR, objs, no, lights, nl, C.byref(g), C.byref(s), None, C.c_void_p(o), None)

    for args, word in (((hp, table.data_ptr(), out.data_ptr()), "d_positions"), ((pos.data_ptr(), hp, out.data_ptr()), "d_dirs"),
                       ((pos.data_ptr(), table.data_ptr(), hp), "d_out")):
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and word in lib().rm_last_error().decode(), word
    for args in ((pos.data_ptr() + 4, table.data_ptr(), out.data_ptr()), (pos.data_ptr(), spare.data_ptr() + 8, out.data_ptr()),
                 (pos.data_ptr(), table.data_ptr(), out.data_ptr() + 4)):
        assert call(*args) == abi.RM_ERR_INVALID_ARGUMENT and "16-byte aligned" in lib().rm_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out.view(torch.int32) == h._i32(h.FLOAT_POISON)).all()), "a refused call wrote into d_out"
    assert call(pos.data_ptr(), table.data_ptr(), out.data_ptr()) == abi.RM_OK
    torch.cuda.synchronize()
    check()
