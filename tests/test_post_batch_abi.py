"""rm_post_process_batch / rm_frames_to_rgba8 without a GPU: the header declares them, the library exports them, and every argument
error returns its status before the first HIP call; Renderer.post_process_batch / to_rgba8_batch / render_sequence check lengths,
shapes and types in Python."""
import pytest

import abi_helpers as ah
from abi_helpers import FAKE
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import SIGNATURES


def test_header_declares_and_library_exports_the_post_batch_entry_points():
    assert ah.params("rm_post_process_batch") and ah.params("rm_frames_to_rgba8")
    assert "rm_post_process_batch" in SIGNATURES and "rm_frames_to_rgba8" in SIGNATURES
    ah.assert_exported(["rm_post_process_batch", "rm_frames_to_rgba8"])
    ah.assert_abi_version()


def posts(*flag_sets, exposure=1.0):
    return (abi.RmPostSettings * len(flag_sets))(*[abi.RmPostSettings(exposure=exposure, **f) for f in flag_sets])


def post_batch(n, ps, num_post, frag=FAKE, bright=None, out=FAKE, W=32, H=24):
    return lib().rm_post_process_batch(frag, bright, out, W, H, n, ps, num_post, None)


def test_post_batch_argument_errors_return_before_any_hip_call():
    L = lib()
    hdr = dict(enableHDR=1)
    one = posts(hdr)
    three = posts(hdr, hdr, hdr)
    # numFrames == 0: nothing to write, null pointers are fine
    assert post_batch(0, one, 1, frag=None, out=None) == abi.RM_OK
    assert post_batch(0, None, 0, frag=None, out=None) == abi.RM_OK
    # negative numFrames
    assert post_batch(-1, one, 1) == abi.RM_ERR_INVALID_ARGUMENT
    # over the cap
    assert post_batch(abi.RM_MAX_BATCH_FRAMES + 1, one, 1) == abi.RM_ERR_CAPACITY
    # numPost neither 1 nor numFrames
    for np_ in (0, 2, 4, -1):
        assert post_batch(3, three, np_) == abi.RM_ERR_INVALID_ARGUMENT, np_
    # null frames, output or settings
    assert post_batch(3, three, 3, frag=None) == abi.RM_ERR_INVALID_ARGUMENT
    assert post_batch(3, three, 3, out=None) == abi.RM_ERR_INVALID_ARGUMENT
    assert post_batch(3, None, 3) == abi.RM_ERR_INVALID_ARGUMENT
    # bad frame size
    for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1)):
        assert post_batch(3, three, 3, W=W, H=H) == abi.RM_ERR_INVALID_ARGUMENT, (W, H)
    # enable flags that differ between entries (each flag in turn); differing exposures alone are not an error (see below)
    for flag in ("enableFXAA", "enableGammaCorrection", "enableHDR", "enableBloom"):
        mixed = posts(hdr, {**hdr, flag: 0 if flag == "enableHDR" else 1}, hdr)
        assert post_batch(3, mixed, 3, bright=FAKE) == abi.RM_ERR_INVALID_ARGUMENT, flag
        assert "flags" in L.rm_last_error().decode()
    # bloom without the BrightColor planes
    assert post_batch(3, posts(dict(enableBloom=1)), 1) == abi.RM_ERR_INVALID_ARGUMENT
    assert "BrightColor" in L.rm_last_error().decode()


def test_frames_to_rgba8_argument_errors_return_before_any_hip_call():
    L = lib()
    assert L.rm_frames_to_rgba8(None, None, 32, 24, 0, None) == abi.RM_OK
    assert L.rm_frames_to_rgba8(FAKE, FAKE, 32, 24, -1, None) == abi.RM_ERR_INVALID_ARGUMENT
    assert L.rm_frames_to_rgba8(FAKE, FAKE, 32, 24, abi.RM_MAX_BATCH_FRAMES + 1, None) == abi.RM_ERR_CAPACITY
    assert L.rm_frames_to_rgba8(None, FAKE, 32, 24, 2, None) == abi.RM_ERR_INVALID_ARGUMENT
    assert L.rm_frames_to_rgba8(FAKE, None, 32, 24, 2, None) == abi.RM_ERR_INVALID_ARGUMENT
    for W, H in ((0, 24), (32, 0), (-5, 24), (32, -1)):
        assert L.rm_frames_to_rgba8(FAKE, FAKE, W, H, 2, None) == abi.RM_ERR_INVALID_ARGUMENT, (W, H)


def test_python_wrappers_check_lengths_shapes_and_types():
    import torch
    from raymarcher_amd.render import Renderer, post_array
    hdr = abi.RmPostSettings(enableHDR=1, exposure=1.0)
    fade = [abi.RmPostSettings(enableHDR=1, exposure=0.5 + 0.1 * i) for i in range(3)]
    assert len(post_array(hdr, 3)) == 1
    a = post_array(fade, 3)
    assert len(a) == 3 and abs(a[2].exposure - 0.7) < 1e-6
    with pytest.raises(ValueError):
        post_array(fade[:2], 3)
    with pytest.raises(ValueError):
        post_array(fade + fade[:1], 3)
    with pytest.raises(ValueError):
        post_array([fade[0], abi.RmPostSettings(enableHDR=1, enableFXAA=1), fade[2]], 3)
    with pytest.raises(ValueError):
        post_array([abi.default_settings()], 1)
    r = Renderer.__new__(Renderer)  # no device is touched before the checks
    r.torch, r.device = torch, torch.device("cuda", 0)
    cpu = torch.zeros((3, 4, 5, 4), dtype=torch.float32)
    with pytest.raises(ValueError):  # not on the renderer's device
        r.post_process_batch(cpu, None, hdr)
    with pytest.raises(ValueError):
        r.to_rgba8_batch(cpu)
    with pytest.raises(ValueError):  # not (N, H, W, 4)
        r.post_process_batch(cpu[0], None, hdr)
    with pytest.raises(ValueError):
        r.to_rgba8_batch(cpu[..., :3])
    with pytest.raises(ValueError):  # not a tensor
        r.post_process_batch(cpu.numpy(), None, hdr)
    with pytest.raises(ValueError):  # wrong number of settings, caught before the device check
        r.post_process_batch(cpu, None, fade[:2])
    with pytest.raises(ValueError):  # render_sequence checks the settings before it renders
        r.render_sequence(None, abi.default_settings(), 5, 4, [abi.RmCamera()] * 3, post=fade[:2])
