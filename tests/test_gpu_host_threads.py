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

The last test shares the session's Renderer between four Python threads (Renderer._upload's cache)."""
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

import helpers as h
import scene_builders as SB
from helpers import tables_of
from raymarcher_amd import abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# case → (threads, calls, whether the case must show that its threads contended: overlap >= 0.5)
CASES = {"frames": (4, 128, True), "entries": (8, 193, True), "field": (4, 200, True), "release": (4, 130, False),
         "counted": (3, 40, False), "timing": (4, 100, False)}
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


def read_dump(base):
    """NAME.scene + NAME.rgba (+ NAME.noise) of gpu_threads' serial pass → (scene tuple, settings, W, H, resources, pixels)."""
    raw = open(base + ".scene", "rb").read()
    W, H, no, nl, has_noise, _ = np.frombuffer(raw, np.int32, 6)
    at = 24

    def take(t):
        nonlocal at
        v = t.from_buffer_copy(raw, at)
        at += C.sizeof(t)
        return v
    cam, g, s = take(abi.RmCamera), take(abi.RmGlobals), take(abi.RmSettings)
    objs, lights = take(abi.RmObject * max(int(no), 1)) if no else (abi.RmObject * 1)(), take(abi.RmLight * max(int(nl), 1)) if nl else (abi.RmLight * 1)()
    assert at == len(raw), f"{base}.scene: {len(raw)} bytes, {at} read"
    res = {"noise": np.fromfile(base + ".noise", np.uint8).reshape(256, 256, 4)} if has_noise else {}
    px = np.fromfile(base + ".rgba", np.float32).reshape(int(H), int(W), 4)
    return (cam, objs, int(no), lights, int(nl), g), s, int(W), int(H), res, px


@pytest.mark.parametrize("case", list(CASES))
def test_library_called_from_real_threads(program, tmp_path, case):
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
