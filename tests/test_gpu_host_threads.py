"""The threads-and-streams contract of include/raymarcher_amd.h held on real host threads: "Calls on different streams or devices
may be issued concurrently from different host threads; calls on ONE stream must come from one thread at a time", "Queries of one
handle may run concurrently from several threads and streams" (RmField), "a render launch or post pass that another thread is
enqueuing on the device at the time finishes its enqueue first" (rm_release_workspaces).

tests/host_threads/gpu_threads.cpp is the driver: a stand-alone C++ host (std::thread, the C ABI, the HIP runtime) that makes every
call alone first and then from threads that start at one barrier, each on a non-blocking stream of its own, and memcmp's every
output — between guard bands of a poison word — against the serial bytes.  One child process per case, under a time limit, so a
deadlock in the library is a failed test; once a child was killed, timed out or met a HIP error the module's remaining tests fail without
starting anything.  The serial pass dumps the whole frames it rendered, and this module holds them to the oracle: "serial" is itself the
pinned result.  The bar is bit equality everywhere; what is new is that it does not depend on who else is calling.

The cases `light` and `lattice` cover the light family, the layer queries, rm_field_ambient and the handle-free lattice queries;
their serial pass dumps its inputs and records, and this module holds every record to the definition its entry's own test module
uses (check_light_dumps, check_lattice_dumps): "equal to serial" means "equal to the definition" there too.

The last two tests share the session's Renderer between four Python threads (Renderer._upload's cache, the probe tables)."""
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import threading
import time

import numpy as np
import pytest

import field_ambient_spec as FA
import field_spec as FS
import helpers as h
import light_bounce_helpers as MB
import light_depth_spec as D
import light_grid_spec as G
import light_probes_spec as L
import scene_builders as SB
import trace_helpers as T
from helpers import tables_of
from raymarcher_amd import LightGrid, abi, sphere_directions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case → (threads, calls, whether the case must show that its threads contended: overlap >= 0.5)
CASES = {"frames": (4, 128, True), "entries": (8, 193, True), "field": (4, 200, True), "release": (4, 130, False),
         "counted": (3, 40, False), "timing": (4, 100, False), "light": (8, 148, True), "lattice": (4, 220, True)}
_ABANDONED = []  # why the module stopped starting processes: a child ended by a signal or at its time limit


@pytest.fixture(scope="module")
def program(renderer, tmp_path_factory):
    """gpu_threads, built by hipcc against libraymarcher_amd.so exactly as test_cxx_host_without_python builds its host."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this box")
    exe = tmp_path_factory.mktemp("gpu_threads") / "gpu_threads"
    libdir = os.path.join(ROOT, "raymarcher_amd", "lib")
    cmd = [hipcc, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "host_threads", "gpu_threads.cpp"), "-o",
           str(exe), "-L", libdir, "-lraymarcher_amd", f"-Wl,-rpath,{libdir}"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return str(exe)


def read_tables(path):
    """The tables of one dump of gpu_threads → (scene tuple, settings, W, H, whether a noise texture goes with them)."""
    raw = open(path, "rb").read()
    W, H, no, nl, has_noise, _ = np.frombuffer(raw, np.int32, 6)
    at = 24

    def take(t):
        nonlocal at
        v = t.from_buffer_copy(raw, at)
        at += C.sizeof(t)
        return v
    cam, g, s = take(abi.RmCamera), take(abi.RmGlobals), take(abi.RmSettings)
    objs, lights = take(abi.RmObject * max(int(no), 1)) if no else (abi.RmObject * 1)(), take(abi.RmLight * max(int(nl), 1)) if nl else (abi.RmLight * 1)()
    assert at == len(raw), f"{path}: {len(raw)} bytes, {at} read"
    return (cam, objs, int(no), lights, int(nl), g), s, int(W), int(H), bool(has_noise)


def read_dump(base, ext=".scene"):
    """NAME.scene + NAME.rgba (+ NAME.noise) of gpu_threads' serial pass → (scene tuple, settings, W, H, resources, pixels)."""
    scene, s, W, H, has_noise = read_tables(base + ext)
    res = {"noise": np.fromfile(base + ".noise", np.uint8).reshape(256, 256, 4)} if has_noise else {}
    px = np.fromfile(base + ".rgba", np.float32).reshape(H, W, 4)
    return scene, s, W, H, res, px


# ---------------------------------------------------------------- the serial records of `light` and `lattice` against the definitions
def words_equal(got, want, what):
    """Two record arrays of any dtype, every 32-bit word."""
    g, w = np.ascontiguousarray(got).view(np.uint32).reshape(-1), np.ascontiguousarray(want).view(np.uint32).reshape(-1)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.nonzero(g != w)[0]
    assert not len(bad), f"{what}: {len(bad)} of {len(g)} words differ, the first is word {int(bad[0])}: got {g[bad[0]]:#010x}, want {w[bad[0]]:#010x}"


def check_light_dumps(renderer, tmp):
    """The serial records of gpu_threads' case `light`, each against the definition that its entry's own module is held to, on the
    dumped inputs: rm_light_probes against light_probes_spec.probes (spec_shade's colours, spec_trace's hit flags, the tree);
    rm_light_probes_depth against light_depth_spec.moments over spec_trace's t; the two lookups against light_grid_spec.grid_light
    and light_depth_spec.grid_light_visible; rm_shade_rays_indirect against light_bounce_helpers.composed_indirect;
    rm_light_probes_indirect against the tree over that composition's colours; the frame against the oracle."""
    def load(name, dtype, shape=None):
        a = np.fromfile(os.path.join(tmp, f"light_{name}.bin"), dtype)
        return a if shape is None else a.reshape(shape)

    n, count, packed = (int(v) for v in load("head", np.int32)[:3])
    par = load("params", np.float32)
    origin, step, far, dist, bias, strength = par[0:3], par[3:6], float(par[6]), float(par[7]), float(par[8]), float(par[9])
    dims = (packed & 255, packed >> 8 & 255, packed >> 16 & 255)
    assert dims == (5, 4, 3) and count == 60 and n == 4096
    positions, points, normals = load("positions", np.float32, (count, 4)), load("points", np.float32, (n, 4)), load("normals", np.float32, (n, 4))
    dirs64, dirs128, weights = load("dirs64", np.float32, (192, 16)), load("dirs128", np.float32, (128, 16)), load("weights64", np.float32, (192, 64))
    assert np.allclose(np.linalg.norm(normals[:, 0:3], axis=1), 1.0, atol=1e-6)
    words_equal(positions[:, 0:3], G.positions(origin, step, dims), "the grid's positions")
    words_equal(dirs64, sphere_directions(64, 3), "the table of 64 directions, three sets")
    words_equal(dirs128, sphere_directions(128, 1), "the table of 128 directions")
    words_equal(weights, D.depth_weights(dirs64, 64, 3, 50.0), "the depth weights")
    for v in range(2):
        scene, s, _, _, _ = read_tables(os.path.join(tmp, f"light_scene_v{v}.tables"))
        objs, no, g = scene[1], scene[2], scene[5]
        rays = load(f"rays_v{v}", np.float32, (n, 8))
        grid, depth = load(f"grid_v{v}", G.PROBE), load(f"depth_v{v}", D.DEPTH)

        def lit(rows, probes, depth_records):
            lg = LightGrid(renderer, np.array(probes).view(np.float32).reshape(-1, 40), origin, step, dims)
            lg.set_depth(None if depth_records is None else np.array(depth_records["moments"]))
            return MB.composed_indirect(renderer, scene, s, None, rows, lg, True, bias, strength, far)

        def bake_lit(probes, depth_records):
            return L.probes(scene, s, None, positions, dirs64, 64, 3, far, shade=lambda rows: lit(rows, probes, depth_records)[0],
                            trace=lambda rows: T.ids_of(T.spec_trace(objs, no, g, s, rows, "no_normal")))

        def moments():
            t = T.spec_trace(objs, no, g, s, L.rays(positions, dirs64, 64, 3, dist), "no_normal")[:, 3]
            return D.moments(positions, dirs64, weights, 64, 3, t)

        what = f"light, scene {v}: "
        baked = L.probes(scene, s, None, positions, dirs64, 64, 3, far)
        L.assert_records_equal(grid, baked, what + "the shared grid")
        L.assert_records_equal(load(f"probes_64_v{v}_b0", L.PROBE), baked, what + "probes_64")
        L.assert_records_equal(load(f"probes_128_v{v}_b0", L.PROBE), L.probes(scene, s, None, positions, dirs128, 128, 1, far), what + "probes_128")
        assert 0 < baked["hits"].sum() < 64 * count, "the probes should hold hits and misses"
        D.assert_depth_equal(depth, moments(), what + "the shared depth records")
        D.assert_depth_equal(load(f"depth_v{v}_b0", D.DEPTH), depth, what + "depth, the bake")
        visible = D.grid_light_visible(grid, depth, dims, origin, step, points, normals, True, bias)
        G.assert_records_equal(load(f"depth_v{v}_b1", G.GRIDLIGHT), visible, what + "depth, the lookup behind the bake")
        G.assert_records_equal(load(f"lookups_v{v}_b0", G.GRIDLIGHT), G.grid_light(grid, dims, origin, step, points, normals, True), what + "lookups, facing")
        G.assert_records_equal(load(f"lookups_v{v}_b1", G.GRIDLIGHT), G.grid_light(grid, dims, origin, step, points, normals, False), what + "lookups, plain")
        G.assert_records_equal(load(f"lookups_v{v}_b2", G.GRIDLIGHT), visible, what + "lookups, visible")
        assert (visible["probes"] > 0).any() and (G.as_words(visible) != G.as_words(load(f"lookups_v{v}_b0", G.GRIDLIGHT))).any(), "the depth records should matter"
        for with_depth in (0, 1):
            d = depth if with_depth else None
            name = f"indirect_v{v + 2 * with_depth}"
            want, on, textured, _ = lit(rays, grid, d)
            assert on.any() and not textured.any(), "the grid should light some hits, none of them textured"
            words_equal(load(name + "_b0", np.float32, (n, 4)), want, what + f"rm_shade_rays_indirect, depth {with_depth}")
            L.assert_records_equal(load(name + "_b1", L.PROBE), bake_lit(grid, d), what + f"rm_light_probes_indirect, depth {with_depth}")
        first, second = load(f"bounce_chain_v{v}_b0", L.PROBE), load(f"bounce_chain_v{v}_b1", L.PROBE)
        L.assert_records_equal(first, baked, what + "bounce_chain, the first bake")
        L.assert_records_equal(second, bake_lit(first, None), what + "bounce_chain, the second bounce")
        words_equal(load(f"bounce_chain_v{v}_b2", np.float32, (n, 4)), lit(rays, second, None)[0], what + "bounce_chain, the rays")
    scene, s, W, H, res, px = read_dump(os.path.join(tmp, "light_render"), ".tables")
    h.assert_bit_equal(px, h.oracle_render(scene, s, W, H, threads=16, **res), "light_render: the serial frame against the oracle")
    # the render family's other buffers against that frame: rm_render_ex without textures, the two shards de-interleaved, and the
    # two ways to the 8-bit frame against each other (the conversions and the post pass have their definitions in their own modules)
    frame = lambda b: load(f"render_v0_b{b}", np.float32, (H, W, 4))  # noqa: E731
    h.assert_bit_equal(frame(1), px, "light_render: rm_render_ex against rm_render_res")
    h.assert_bit_equal(frame(4), px, "light_render: the two shards of rm_render_tiles, de-interleaved")
    eight = load("render_v0_b7", np.uint8)
    assert (eight == load("render_v0_b6", np.uint8)).all(), "light_render: rm_deinterleave_rgba8 of rm_tiles_to_rgba8 against rm_frame_to_rgba8"


def check_lattice_dumps(tmp):
    """The serial records of gpu_threads' case `lattice` against field_ambient_spec and field_spec on the dumped lattices: the block
    entries against the definition on the dense form of their virtual lattice with the list they were given.  The records of
    rm_sdf_blocks_select_pruned (buffers 10 and 11) are held to the serial pass only: tests/test_gpu_sdf_prune.py has its definition."""
    def load(name, dtype, shape=None):
        a = np.fromfile(os.path.join(tmp, f"lattice_{name}.bin"), dtype)
        return a if shape is None else a.reshape(shape)

    n, n_amb, full, shorter, nx, ny, nz, max_blocks = (int(v) for v in load("head", np.int32))
    assert (n, n_amb, nx, ny, nz) == (4096, 256, 17, 13, 9) and shorter == full - 1 >= 1
    points, normals, rays = load("points", np.float32, (n, 4)), load("normals", np.float32, (n, 4)), load("rays", np.float32, (n, 8))
    hemi64, hemi256 = load("hemi64", np.float32, (192, 4)), load("hemi256", np.float32, (256, 4))
    par = load("params", np.float32)
    lo, step, blo, bstep, bias, reach = par[0:3], par[3:6], par[6:9], par[9:12], float(par[12]), float(par[13])
    dense, ids = load("dense", np.float32, (nz, ny, nx)), load("dense_ids", np.int32, (nz, ny, nx))
    virtual, vids = load("virtual", np.float32, (9, 17, 17)), load("virtual_ids", np.int32, (9, 17, 17))
    blocks = load("blocks", np.int32, (full, 4))
    rec = lambda b, dtype: load(f"lattice_v0_b{b}", dtype)  # noqa: E731
    iso = 0.0  # every march of the case
    amb_p, amb_n = points[:n_amb], normals[:n_amb]
    for b, (lattice, o, st, i, bl, what) in enumerate(((dense, lo, step, ids, None, "dense"), (virtual, blo, bstep, vids, blocks, "blocks"))):
        soft = FA.ambient(lattice, o, st, amb_p, amb_n, hemi64, 64, 3, bias, reach, iso, 64, FA.SOFT, ids=i, block_list=bl)
        words_equal(rec(b, FA.AMBIENT), soft, f"lattice: rm_field_ambient, soft, {what}")
        hard = FA.ambient(lattice, o, st, amb_p, None, hemi256, 256, 1, bias, reach, iso, 64, FA.HARD, ids=i, block_list=bl)
        words_equal(rec(2 + b, FA.AMBIENT), hard, f"lattice: rm_field_ambient, hard, {what}")
        assert (soft["hits"] > 0).any() and (hard["hits"] >= 0).any() and (hard["visibility"] > 0).any()
    words_equal(rec(4, FS.SAMPLE), FS.sample(dense, lo, step, points, ids), "lattice: rm_sdf_sample")
    words_equal(rec(5, FS.HIT), FS.trace(dense, lo, step, rays, iso, 128, ids), "lattice: rm_sdf_trace")
    for b, count in ((6, full), (7, shorter)):
        words_equal(rec(b, FS.SAMPLE), FS.sample(virtual, blo, bstep, points, vids, blocks[:count]), f"lattice: rm_sdf_sample_blocks, {count} blocks")
        words_equal(rec(b + 2, FS.HIT), FS.trace(virtual, blo, bstep, rays, iso, 128, vids, blocks[:count]), f"lattice: rm_sdf_trace_blocks, {count} blocks")
    assert (rec(6, FS.SAMPLE)["objectId"] != rec(7, FS.SAMPLE)["objectId"]).any(), "the two lists should give different samples"
    assert (rec(9, FS.HIT)["objectId"] >= 0).any() and (rec(5, FS.HIT)["objectId"] == -1).any()


@pytest.mark.parametrize("case", list(CASES))
def test_library_called_from_real_threads(program, renderer, tmp_path, case):
    threads, calls, must_contend = CASES[case]
    if _ABANDONED:
        pytest.fail(f"not started: {_ABANDONED[0]}")
    t0 = time.perf_counter()
    try:
        r = subprocess.run([program, case, SB.SCENES, str(tmp_path)], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _ABANDONED.append(f"gpu_threads {case} did not end within its time limit (a deadlock?)")
        pytest.fail(_ABANDONED[0])
    wall = time.perf_counter() - t0
    if r.returncode < 0 or r.returncode in (134, 139):
        _ABANDONED.append(f"gpu_threads {case} was ended by signal {abs(r.returncode) if r.returncode < 0 else r.returncode - 128}: {r.stderr[-600:]}")
        pytest.fail(_ABANDONED[0])
    if r.returncode == 3:  # a HIP call failed in the child: nothing more is started on the device from this module
        _ABANDONED.append(f"gpu_threads {case} met a device error: {r.stdout[-600:]} {r.stderr[-600:]}")
        pytest.fail(_ABANDONED[0])
    lines = r.stdout.strip().splitlines()
    assert lines, (r.returncode, r.stderr[-800:])
    line = json.loads(lines[-1])
    print(f"gpu_threads {case}: process {wall:.2f} s, threads' wall {line['wall_ms']:.1f} ms, {line['threads']} threads, {line['calls']} calls, "
          f"overlap {line['overlap']:.3f}, first_mismatch {line['first_mismatch']!r}")
    assert line["case"] == case
    assert line["ok"] and line["first_mismatch"] is None and r.returncode == 0, (line["first_mismatch"], r.returncode, r.stderr[-800:])
    assert (line["threads"], line["calls"]) == (threads, calls)
    if must_contend:
        assert line["overlap"] >= 0.5, f"{case} did not contend: only {line['overlap']:.3f} of its calls ran beside a call of another thread"
    # "serial" is itself pinned: every whole frame the serial pass rendered equals the oracle's, bit for bit
    dumps = sorted(glob.glob(os.path.join(str(tmp_path), f"{case}_*.scene")))
    assert len(dumps) == {"frames": 4, "timing": 4, "counted": 3, "release": 1}.get(case, 0)
    for d in dumps:
        scene, s, W, H, res, px = read_dump(d[:-len(".scene")])
        h.assert_bit_equal(px, h.oracle_render(scene, s, W, H, threads=16, **res), f"{os.path.basename(d)}: the serial frame against the oracle")
    if case == "light":
        check_light_dumps(renderer, str(tmp_path))
    if case == "lattice":
        check_lattice_dumps(str(tmp_path))


def resource_scenes(W, H):
    """Four scenes that read samplers, each with arrays of its own: textured primitives, a sky box, an area light with its LTC
    tables, the sea with the noise texture."""
    out = [(SB.textured_scene(W, H), abi.default_settings(features=abi.RM_FEAT_WHITE_BACKGROUND), {"textures": SB.synthetic_textures()})]
    out += [SB.resource_case(name, W, H) for name in ("skybox_reflect", "area_light", "sea_sky")]
    return out


def test_one_renderer_shared_by_python_threads(renderer):
    """Four threads, one Renderer, a torch stream each, a resource scene each; the first calls leave one barrier together, so the
    first uploads — and, before the cache was made in __init__ and put behind a lock, its creation — race.  Every one of the 12 frames
    of every thread equals the frame the same call gives alone."""
    import torch
    if _ABANDONED:
        pytest.fail(f"not started: {_ABANDONED[0]}")
    W, H, frames, n = 64, 40, 12, 4
    cases = resource_scenes(W, H)
    tables = [tables_of(scene, res) for scene, _, res in cases]
    barrier = threading.Barrier(n)
    got, errors = [None] * n, [None] * n

    def work(i):
        try:
            stream = torch.cuda.Stream(device=renderer.device)
            outs = []
            barrier.wait(timeout=60)
            with torch.cuda.stream(stream):
                for _ in range(frames):
                    outs.append(renderer.render(tables[i], cases[i][1], W, H))
            stream.synchronize()
            got[i] = [o.cpu().numpy() for o in outs]
        except BaseException as e:  # noqa: BLE001 — reported by the main thread
            errors[i] = e

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(n)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + 120
    for t in threads:
        t.join(timeout=max(deadline - time.monotonic(), 0.1))
    if any(t.is_alive() for t in threads):
        pytest.exit("threads that share one Renderer did not end within 120 s: the library or the Python layer deadlocked", returncode=1)
    assert errors == [None] * n, errors
    torch.cuda.synchronize(renderer.device)
    for i in range(n):
        alone = h.render_guarded(renderer, tables[i], cases[i][1], W, H).cpu().numpy()
        assert len(got[i]) == frames
        for k, frame in enumerate(got[i]):
            h.assert_bit_equal(frame, alone, f"thread {i}, frame {k} against the same call made alone")


def test_one_renderer_shared_by_python_threads_making_light_calls(renderer):
    """Four threads, one Renderer, a torch stream each, eight rounds each of one light call: light_probes with the renderer's built
    table, light_probes_depth with its built weights, shade_rays_indirect on a LightGrid that all share, and that grid's
    irradiance_visible.  The first calls leave one barrier together, so the renderer's table and weight caches are filled under
    contention.  Every result equals the same call made alone."""
    import torch
    if _ABANDONED:
        pytest.fail(f"not started: {_ABANDONED[0]}")
    W, H, rounds, n, K = 64, 40, 8, 4, 32  # K: a table no other test of the session has built
    scene = SB.all_primitives_scene(W, H)
    s = abi.default_settings(maxSteps=96)
    t = tables_of(scene)
    lo, hi = np.array([-3.0, -1.5, -3.0], np.float32), np.array([3.0, 2.5, 3.0], np.float32)
    grid = renderer.light_grid_visible(t, s, (4, 3, 4), bounds=(lo, hi), directions=16)
    rng = np.random.default_rng(11)
    pos = np.ones((24, 4), np.float32)
    pos[:, 0:3] = rng.uniform(lo, hi, (24, 3))
    rays = np.array(T.make_rays(rng.uniform(lo, hi, (256, 3)) + (0, 0, 6), rng.normal(size=(256, 3)) * 0.2 + (0, 0, -1), 100.0))
    pts, nrm = np.ones((256, 4), np.float32), np.zeros((256, 4), np.float32)
    pts[:, 0:3] = rng.uniform(lo, hi, (256, 3))
    u = rng.normal(size=(256, 3))
    nrm[:, 0:3] = u / np.linalg.norm(u, axis=1, keepdims=True)
    dev = {k: torch.from_numpy(v).to(renderer.device) for k, v in (("pos", pos), ("rays", rays), ("pts", pts), ("nrm", nrm))}
    torch.cuda.synchronize(renderer.device)
    calls = [lambda: torch.cat([a.reshape(len(pos), -1).view(torch.int32) for a in renderer.light_probes(t, s, dev["pos"], directions=K, sets=2, far=50.0)], dim=1),
             lambda: renderer.light_probes_depth(t, s, dev["pos"], directions=K, sets=2, max_distance=4.0),
             lambda: renderer.shade_rays_indirect(t, s, dev["rays"], grid, far=50.0, strength=0.7),
             lambda: torch.cat([a.reshape(256, -1).view(torch.int32) for a in grid.irradiance_visible(dev["pts"], dev["nrm"])], dim=1)]
    barrier = threading.Barrier(n)
    got, errors = [None] * n, [None] * n

    def work(i):
        try:
            stream = torch.cuda.Stream(device=renderer.device)
            outs = []
            barrier.wait(timeout=60)
            with torch.cuda.stream(stream):
                for _ in range(rounds):
                    outs.append(calls[i]())
            stream.synchronize()
            got[i] = [o.cpu().numpy() for o in outs]
        except BaseException as e:  # noqa: BLE001 — reported by the main thread
            errors[i] = e

    threads = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(n)]
    for th in threads:
        th.start()
    deadline = time.monotonic() + 120
    for th in threads:
        th.join(timeout=max(deadline - time.monotonic(), 0.1))
    if any(th.is_alive() for th in threads):
        pytest.exit("threads that share one Renderer did not end within 120 s: the library or the Python layer deadlocked", returncode=1)
    assert errors == [None] * n, errors
    torch.cuda.synchronize(renderer.device)
    for i in range(n):
        alone = calls[i]().cpu().numpy()
        assert len(got[i]) == rounds and (h.bits(alone) != 0).any()
        for k, out in enumerate(got[i]):
            h.assert_bit_equal(out, alone, f"thread {i}, round {k} against the same call made alone")
