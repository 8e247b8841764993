"""rm_post_process_batch / rm_frames_to_rgba8 and Renderer.post_process_batch / to_rgba8_batch / render_sequence on the GPU: every
frame of a batch bit for bit against the oracle's post passes and against rm_post_process / rm_frame_to_rgba8 of that frame, with
one settings entry or one per frame (exposure fades); guarded outputs; chunks of 64 frames and chunks cut by the workspace limit;
in place; two streams at once; and the whole export path from the batched raymarch to the finished 8-bit images."""
import ctypes as C

import numpy as np
import pytest

import helpers as h
import scene_builders as SB
from helpers import assert_bit_equal, tables_of, with_globals
from scene_builders import orbit
from raymarcher_amd import abi, lib
from raymarcher_amd._lib import RaymarcherError

pytestmark = pytest.mark.gpu

POST_BYTES_PER_PIXEL = 20  # the post workspace: two binary16 ping-pong images and the 8-bit FXAA source


def synthetic_frames(N, W, H, seed=0):
    """N different random frames (values up to 1.6, so some pass the bright threshold) and their sparse BrightColor planes, the
    way test_post_passes_bit_exact_on_wide_synthetic_frames builds one."""
    rng = np.random.default_rng(seed * 7919 + W * 1000 + H)
    frag = rng.random((N, H, W, 4), dtype=np.float32) * np.float32(1.6)
    frag[..., 3] = 1.0
    luma = (frag[..., :3] * np.array([0.2126, 0.7152, 0.0722], dtype=np.float32)).sum(-1, keepdims=True)
    bright = np.where(luma > 1.0, frag, np.float32(0.0)).astype(np.float32)
    bright[..., 3] = 1.0
    return frag, bright


def post_of(name, exposure=None):
    kw = {"exposure": 1.0, **SB.POST_CASES[name]}
    if exposure is not None:
        kw["exposure"] = exposure
    return abi.RmPostSettings(**kw)


def fade(name, N):
    """One settings entry per frame: the case's flags, a different exposure for every frame."""
    base = post_of(name).exposure
    return [post_of(name, base * (0.55 + 0.1 * f)) for f in range(N)]


def device(renderer, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(renderer.device) for a in arrays]


def per_frame(renderer, fd, bd, posts):
    """rm_post_process of every frame with its own settings, stacked."""
    import torch
    N = fd.shape[0]
    return torch.stack([renderer.post_process(fd[f], bd[f], posts[f if len(posts) == N else 0]) for f in range(N)])


# ---------------------------------------------------------------- 1. oracle equality
@pytest.mark.parametrize("W,H", [(150, 90), (700, 45), (257, 33), (3, 70), (1, 1)])
@pytest.mark.parametrize("N", [1, 3, 17])
def test_every_frame_equals_the_oracle(renderer, W, H, N):
    frag, bright = synthetic_frames(N, W, H)
    fd, bd = device(renderer, frag, bright)
    oracle = {}

    def ref(f, p):
        key = (f, p.exposure)
        if key not in oracle:
            oracle[key] = h.oracle_post(frag[f], bright[f], p)
        return oracle[key]

    for name in SB.POST_CASES:
        oracle.clear()
        for posts in ([post_of(name)], fade(name, N)):
            got = renderer.post_process_batch(fd, bd, posts if len(posts) > 1 else posts[0]).cpu().numpy()
            for f in range(N):
                p = posts[f if len(posts) == N else 0]
                assert_bit_equal(got[f], ref(f, p), f"{name} {W}x{H} N={N} numPost={len(posts)} frame {f}")


# ---------------------------------------------------------------- 2. guarded writes
@pytest.mark.parametrize("W,H", [(257, 33), (3, 70)])
def test_every_word_of_every_frame_is_written_and_nothing_else(renderer, W, H):
    N = 5
    frag, bright = synthetic_frames(N, W, H, seed=2)
    fd, bd = device(renderer, frag, bright)
    for name in SB.POST_CASES:
        posts = fade(name, N)
        out, check = h.guarded((N, H, W, 4), device=renderer.device)
        renderer.post_process_batch(fd, bd if posts[0].enableBloom else None, posts, out=out)
        check()
        assert SB.ieq(out, per_frame(renderer, fd, bd, posts)), name


# ---------------------------------------------------------------- 3. chunk boundaries
@pytest.mark.parametrize("N", [65, 130])
def test_batches_across_the_64_frame_chunk(renderer, N):
    W, H = 33, 17
    frag, bright = synthetic_frames(N, W, H, seed=3)
    fd, bd = device(renderer, frag, bright)
    posts = fade("bloom_hdr_fxaa", N)
    out, check = h.guarded((N, H, W, 4), device=renderer.device)
    renderer.post_process_batch(fd, bd, posts, out=out)
    check()
    assert SB.ieq(out, per_frame(renderer, fd, bd, posts))
    got = out.cpu().numpy()
    for f in (0, 63, 64, N - 1):
        assert_bit_equal(got[f], h.oracle_post(frag[f], bright[f], posts[f]), f"frame {f} of {N}")


def test_workspace_limit_cuts_the_chunks(renderer):
    W, H, N = 61, 37, 5
    need = POST_BYTES_PER_PIXEL * W * H  # one frame's post workspace
    frag, bright = synthetic_frames(N, W, H, seed=4)
    fd, bd = device(renderer, frag, bright)
    posts = fade("bloom_hdr_fxaa", N)
    expect = per_frame(renderer, fd, bd, posts)
    L = lib()
    freed = C.c_ulonglong()
    try:
        assert L.rm_set_workspace_limit(2 * need) == abi.RM_OK
        assert L.rm_release_workspaces(C.byref(freed)) == abi.RM_OK
        out, check = h.guarded((N, H, W, 4), device=renderer.device)
        renderer.post_process_batch(fd, bd, posts, out=out)  # chunks of 2, 2, 1
        check()
        assert SB.ieq(out, expect)
        assert L.rm_release_workspaces(C.byref(freed)) == abi.RM_OK
        assert 0 < freed.value <= 2 * need, freed.value
        # below one frame's need: the workspace cannot be allocated, as for rm_post_process
        assert L.rm_set_workspace_limit(need - 1) == abi.RM_OK
        with pytest.raises(RaymarcherError) as e:
            renderer.post_process_batch(fd, bd, posts)
        assert e.value.status == abi.RM_ERR_DEVICE
        assert "rm_set_workspace_limit" in L.rm_last_error().decode()
    finally:
        L.rm_set_workspace_limit(0)
    assert SB.ieq(renderer.post_process_batch(fd, bd, posts), expect)


# ---------------------------------------------------------------- 4. in place
def test_in_place_equals_out_of_place(renderer):
    W, H, N = 150, 90, 6
    frag, bright = synthetic_frames(N, W, H, seed=5)
    fd, bd = device(renderer, frag, bright)
    for name in ("bloom_hdr_fxaa", "bloom", "hdr", "fxaa_only", "none"):
        posts = fade(name, N)
        ref = renderer.post_process_batch(fd, bd, posts).clone()
        inplace = fd.clone()
        assert renderer.post_process_batch(inplace, bd, posts, out=inplace).data_ptr() == inplace.data_ptr()
        assert SB.ieq(inplace, ref), name


# ---------------------------------------------------------------- 5. two streams
def test_two_streams_use_their_own_workspaces(renderer):
    import torch
    W, H, N = 256, 256, 16
    fa, ba = synthetic_frames(N, W, H, seed=6)
    fb, bb = synthetic_frames(N, W, H, seed=7)
    fad, bad, fbd, bbd = device(renderer, fa, ba, fb, bb)
    posts = fade("bloom_hdr_fxaa", N)
    ref_a, ref_b = per_frame(renderer, fad, bad, posts), per_frame(renderer, fbd, bbd, posts[::-1])
    torch.cuda.synchronize(renderer.device)
    s1, s2 = torch.cuda.Stream(renderer.device), torch.cuda.Stream(renderer.device)
    for _ in range(2):  # the second round reuses both streams' workspaces
        with torch.cuda.stream(s1):
            out_a = renderer.post_process_batch(fad, bad, posts)
        with torch.cuda.stream(s2):
            out_b = renderer.post_process_batch(fbd, bbd, posts[::-1])
        torch.cuda.synchronize(renderer.device)
        assert SB.ieq(out_a, ref_a) and SB.ieq(out_b, ref_b)


# ---------------------------------------------------------------- 6. to_rgba8_batch
@pytest.mark.parametrize("W,H,N", [(257, 33, 3), (3, 70, 5), (1, 1, 2), (33, 17, 70)])
def test_to_rgba8_batch_flips_every_frame_in_itself(renderer, W, H, N):
    rng = np.random.default_rng(W * 31 + H * 7 + N)
    frames = (rng.random((N, H, W, 4), dtype=np.float32) * np.float32(1.4) - np.float32(0.2)).astype(np.float32)
    (fd,) = device(renderer, frames)
    got = h.guarded_u8((N, H, W, 4), lambda o: renderer.to_rgba8_batch(fd, out=o), device=renderer.device)
    for f in range(N):
        one = h.guarded_u8((H, W, 4), lambda o: renderer.to_rgba8(fd[f], out=o), device=renderer.device)
        assert bool((got[f] == one).all()), f"frame {f}"
    exp = (np.clip(frames[:, ::-1], 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    assert (got.cpu().numpy() == exp).all()


# ---------------------------------------------------------------- 7. end to end
def test_render_sequence_equals_the_per_frame_export(renderer, tmp_path):
    W, H, N = 150, 90, 8
    scene = SB.reflect_refract_scene(W, H)
    for li in scene[3]:
        li.color[0] *= 2.5; li.color[1] *= 2.5; li.color[2] *= 2.5  # over-exposed: BrightColor is populated
    s = abi.default_settings(enableReflection=1)
    cams = orbit((0, 1.2, 5), (0, -0.2, -1), 40.0, W, H, N)
    globs = [with_globals(scene[5], iTime=0.25 * f) for f in range(N)]
    post = post_of("bloom_hdr_fxaa")
    imgs = renderer.render_sequence(tables_of(scene), s, W, H, cams, globals_=globs, post=post)
    assert tuple(imgs.shape) == (N, H, W, 4) and imgs.dtype == renderer.torch.uint8
    for f in range(N):
        tf = tables_of((cams[f],) + tuple(scene[1:5]) + (globs[f],))
        frag, bright = renderer.render(tf, s, W, H, bright=True)
        if f == 0:
            assert float(bright[..., :3].max()) > 1.0
        one = renderer.to_rgba8(renderer.post_process(frag, bright, post))
        assert bool((imgs[f] == one).all()), f"frame {f}"
    assert not bool((imgs[0] == imgs[N - 1]).all())
    # frame 0 through the oracle: raymarch, post passes, 8-bit read-back
    frag0, bright0 = h.oracle_render((cams[0],) + tuple(scene[1:5]) + (globs[0],), s, W, H, bright=True)
    ref = h.oracle_post(frag0, bright0, post)
    exp = (np.clip(ref[::-1], 0, 1) * np.float32(255.0) + np.float32(0.5)).astype(np.uint8)
    assert (imgs[0].cpu().numpy() == exp).all()
    # post=None: the raw frames, quantised
    raw = renderer.render_sequence(tables_of(scene), s, W, H, cams[:2], globals_=globs[:2])
    assert bool((raw == renderer.to_rgba8_batch(renderer.render_batch(tables_of(scene), s, W, H, cams[:2], globals_=globs[:2]))).all())
    # and the images written as a numbered PNG sequence
    from raymarcher_amd.render import load_image, save_png_sequence
    paths = save_png_sequence(imgs[:3], str(tmp_path / "frame_{:04d}.png"))
    assert [p.rsplit("/", 1)[1] for p in paths] == ["frame_0000.png", "frame_0001.png", "frame_0002.png"]
    for f, p in enumerate(paths):
        assert (load_image(p, flip_vertical=False) == imgs[f].cpu().numpy()).all()


def test_host_pointers_are_refused(renderer):
    """Plain host memory is refused before any launch, as rm_post_process and rm_frame_to_rgba8 refuse it."""
    import torch
    L = lib()
    host = np.zeros((2, 4, 5, 4), dtype=np.float32)
    host8 = np.zeros((2, 4, 5, 4), dtype=np.uint8)
    dev = torch.zeros((2, 4, 5, 4), dtype=torch.float32, device=renderer.device)
    ps = (abi.RmPostSettings * 1)(post_of("hdr"))
    assert L.rm_post_process_batch(C.c_void_p(host.ctypes.data), None, C.c_void_p(dev.data_ptr()), 5, 4, 2, ps, 1, None) == \
        abi.RM_ERR_INVALID_ARGUMENT
    assert "d_frag" in L.rm_last_error().decode()
    assert L.rm_post_process_batch(C.c_void_p(dev.data_ptr()), None, C.c_void_p(host.ctypes.data), 5, 4, 2, ps, 1, None) == \
        abi.RM_ERR_INVALID_ARGUMENT
    assert "d_out" in L.rm_last_error().decode()
    assert L.rm_frames_to_rgba8(C.c_void_p(dev.data_ptr()), C.c_void_p(host8.ctypes.data), 5, 4, 2, None) == abi.RM_ERR_INVALID_ARGUMENT
    assert "d_out" in L.rm_last_error().decode()
