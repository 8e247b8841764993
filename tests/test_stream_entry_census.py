"""A census of the entry points that take a stream, so that a new one is not forgotten by the tests that hold the header's
concurrency and bookkeeping promises: every function of include/raymarcher_amd.h whose last parameter is `void *stream` is called
by the threads driver (tests/host_threads/gpu_threads.cpp) and named in one of the tables of tests/test_gpu_query_bookkeeping.py,
or stands in a short exemption set with its reason.  No GPU: the header's parser and a search of the two files' text."""
import os
import re

import abi_helpers as ah

DRIVER = os.path.join(ah.ROOT, "tests", "host_threads", "gpu_threads.cpp")
BOOKKEEPING = os.path.join(ah.ROOT, "tests", "test_gpu_query_bookkeeping.py")

# not called by the threads driver, and why
DRIVER_EXEMPT = {
    "rm_probe_math": "a tests-only probe of one device function: no scene block, no library state",
    "rm_probe_sdscene": "a tests-only probe; its untimed staging call is held by test_gpu_query_bookkeeping",
    "rm_probe_sdscene_variant": "a tests-only probe, staged as rm_probe_sdscene is",
    "rm_probe_bump": "a tests-only probe of one device function: no scene block, no library state",
    "rm_probe_pool_cull": "a tests-only probe, staged as rm_probe_sdscene is",
}
# in no bookkeeping table, and why: the single-frame and batch renders, whose path depends on the picture and the tuner
BOOKKEEPING_EXEMPT = {
    "rm_render": "path 1, 2 … 5 by picture and tuner: test_gpu_parity, test_gpu_wavefront and test_gpu_write_coverage pin it; its timed launches: gpu_threads' case timing",
    "rm_render_ex": "rm_render with textures: the same launch path, pinned with rm_render",
    "rm_render_res": "rm_render with every sampler: the same launch path, pinned with rm_render",
    "rm_render_tiles": "rm_render of a shard's rows: the same launch path (test_gpu_parity)",
    "rm_render_tiles_res": "rm_render_tiles with the samplers: the same launch path",
    "rm_render_batch": "path 6 or, frame by frame, the wavefront pipeline: test_gpu_batch pins both",
}


def census():
    """The functions of the header whose last parameter is `void *stream`."""
    out = []
    for name in ah.declared_functions():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", ah.HEADER_CODE)
        if m and re.sub(r"\s+", " ", m.group(1).split(",")[-1].strip()) == "void *stream":
            out.append(name)
    return out


def missing(names, text, exempt):
    """The names that `text` never calls (`name(`) and that are not exempt."""
    return [n for n in names if n not in exempt and not re.search(r"\b" + n + r"\(", text)]


def test_the_census_finds_the_stream_taking_entries():
    names = census()
    assert len(names) >= 49 and len(set(names)) == len(names)
    for n in ("rm_render", "rm_light_probes", "rm_light_grid_irradiance_visible", "rm_field_ambient", "rm_sdf_trace_blocks", "rm_post_process_batch"):
        assert n in names, n
    for n in ("rm_field_create_blocks", "rm_render_counted", "rm_set_timing", "rm_camera_rays"):  # a stream that is not last, or none
        assert n not in names, n


def test_every_stream_taking_entry_is_called_by_the_threads_driver():
    names, text = census(), open(DRIVER).read()
    assert set(DRIVER_EXEMPT) <= set(names), sorted(set(DRIVER_EXEMPT) - set(names))
    lacking = missing(names, text, DRIVER_EXEMPT)
    assert not lacking, f"tests/host_threads/gpu_threads.cpp calls none of: {', '.join(lacking)}"
    stale = [n for n in DRIVER_EXEMPT if re.search(r"\b" + n + r"\(", text)]
    assert not stale, f"exempt, but called by the driver: {', '.join(stale)}"
    # the check can fail: a driver without one of its families names that family's entry
    for gone in ("rm_field_ambient", "rm_light_grid_irradiance", "rm_sdf_trace_blocks"):
        assert missing(names, text.replace(gone + "(", "("), DRIVER_EXEMPT) == [gone]


def test_every_stream_taking_entry_is_in_a_bookkeeping_table():
    names, text = census(), open(BOOKKEEPING).read()
    assert set(BOOKKEEPING_EXEMPT) <= set(names), sorted(set(BOOKKEEPING_EXEMPT) - set(names))
    lacking = missing(names, text, BOOKKEEPING_EXEMPT)
    assert not lacking, f"tests/test_gpu_query_bookkeeping.py has no row for: {', '.join(lacking)}"
    stale = [n for n in BOOKKEEPING_EXEMPT if re.search(r"\b" + n + r"\(", text)]
    assert not stale, f"exempt, but in a table: {', '.join(stale)}"


def test_the_exemption_sets_stay_short():
    names = census()
    assert all(DRIVER_EXEMPT.values()) and all(BOOKKEEPING_EXEMPT.values()), "every exemption has its reason"
    assert len(DRIVER_EXEMPT) + len(BOOKKEEPING_EXEMPT) <= len(names) // 4, (len(DRIVER_EXEMPT), len(BOOKKEEPING_EXEMPT), len(names))
