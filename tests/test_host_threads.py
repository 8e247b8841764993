"""The host-only half of the threads contract of include/raymarcher_amd.h — "calls … may be issued concurrently from different host
threads", "Thread-local text of the last failure in this thread" — on eight real threads under ThreadSanitizer, on the CPU (the GPU
build cannot run under a sanitizer on this pool): tests/host_threads/host_threads.cpp, a stand-alone program over the scenefile
loader, the camera builders, the image readers, the rm_debug_* functions that share a static SceneBlock behind a static mutex
(rm_frame.cpp) and rm_last_error.  Every threaded result is memcmp'd against the same call made alone; a lock or a thread_local
that went missing is a TSan report, which halts the program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "raymarcher_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("host_threads") / "host_threads"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-o", str(out), os.path.join(ROOT, "tests", "host_threads", "host_threads.cpp")]
    cmd += [os.path.join(CSRC, f) for f in ("rm_host.cpp", "rm_scene.cpp", "rm_jpeg.cpp", "rm_gif.cpp", "rm_frame.cpp")] + ["-lz"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find -ltsan" in r.stderr:
        pytest.skip("ThreadSanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    return str(out)


def test_host_entries_from_eight_threads_under_tsan(program):
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([program, os.path.join(ROOT, "tests", "golden", "scenes")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert "51 of 52 scenefiles loaded" in r.stdout, r.stdout  # unit_terrain.json is invalid in the reference itself
    assert lines[-1] == "host_threads ok", r.stdout[-2000:]
