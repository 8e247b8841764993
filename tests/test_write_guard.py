"""The guarded, poisoned output buffers of the write-coverage tests (helpers.guarded), on CPU tensors: a writer that skips one
word and a writer that writes one word past the end must both fail check(); a writer that fills the payload exactly must pass."""
import numpy as np
import pytest
import torch

import helpers as h

SHAPES = [(1, 1, 4), (3, 70, 4), (9, 65, 4), (2, 5, 7, 4)]


def payload_words(out):
    return out.reshape(-1).view(torch.int32)


def whole_buffer(out):
    """The word view of the payload's allocation, with the index of the payload's first word in it."""
    base = out.untyped_storage()
    words = torch.empty(0, dtype=torch.int32).set_(base, 0, (base.nbytes() // 4,))
    return words, out.storage_offset() * out.element_size() // 4


@pytest.mark.parametrize("shape", SHAPES)
def test_guard_fails_a_skipped_word_and_passes_a_full_write(shape):
    out, check = h.guarded(shape, device="cpu")
    assert out.shape == shape and out.dtype == torch.float32
    assert out.storage_offset() * out.element_size() % 256 == 0  # the payload keeps the kernels' float4 alignment
    assert bool((payload_words(out) == h._i32(h.FLOAT_POISON)).all())
    n = out.numel()
    for skip in sorted({0, n // 2, n - 1}):
        out, check = h.guarded(shape, device="cpu")
        w = payload_words(out)
        w.copy_(torch.arange(n, dtype=torch.int32))  # every word written …
        w[skip] = h._i32(h.FLOAT_POISON)              # … but one: it still holds the poison
        with pytest.raises(AssertionError, match="never written") as e:
            check()
        where = tuple(int(v) for v in np.unravel_index(skip, shape))
        assert str(where) in str(e.value)
    out, check = h.guarded(shape, device="cpu")
    out.copy_(torch.rand(shape))
    check()


@pytest.mark.parametrize("shape", SHAPES)
def test_guard_fails_a_write_past_either_end(shape):
    for before in (True, False):
        out, check = h.guarded(shape, device="cpu")
        out.copy_(torch.rand(shape))
        words, first = whole_buffer(out)
        words[first - 1 if before else first + out.numel()] = 0  # one word in front of the payload, or one past its end
        with pytest.raises(AssertionError, match="front guard" if before else "back guard") as e:
            check()
        assert ("4 bytes before" if before else "0 bytes past") in str(e.value)


def test_guard_bands_are_at_least_a_row_and_4k_and_256_byte_multiples():
    for shape in [(1, 1, 4), (2, 636, 4), (1, 4000, 4), (0, 17, 4)]:
        g = h.Guarded(shape, torch.float32, h.FLOAT_POISON, "cpu")
        assert g.guard % 256 == 0 and g.guard >= 4096 and g.guard >= shape[1] * 16
        assert g.buf.numel() - g.guard - g.nbytes >= g.guard
    out, check = h.guarded((0, 17, 4), device="cpu")  # an empty payload: only the guards are checked
    check()


def test_float_poison_is_a_signalling_nan_no_arithmetic_produces():
    p = np.array([h.FLOAT_POISON], dtype=np.uint32).view(np.float32)
    assert np.isnan(p[0]) and not (h.FLOAT_POISON >> 22) & 1  # quiet bit clear
    # what torch produces from it is a quiet NaN: a finished output word cannot equal the poison by accident
    q = (torch.from_numpy(p.copy()) * 1.0).view(torch.int32)
    assert int(q[0]) != h._i32(h.FLOAT_POISON)


def test_uint8_outputs_are_produced_under_two_poisons():
    shape = (3, 5, 4)
    ref = torch.randint(0, 256, shape, dtype=torch.uint8)
    ref[0, 0, 0] = 0xA5  # a real byte equal to one of the poisons is no error

    def full(out):
        out.copy_(ref)
    assert torch.equal(h.guarded_u8(shape, full, device="cpu"), ref)

    def skips(out):  # every byte but one: that one keeps whichever poison the buffer was filled with
        keep = out.view(-1)[7].clone()
        out.copy_(ref)
        out.view(-1)[7] = keep
    with pytest.raises(AssertionError, match="differ under the two poisons"):
        h.guarded_u8(shape, skips, device="cpu")

    def past(out):  # every byte, and one more past the end
        out.copy_(ref)
        raw = torch.empty(0, dtype=torch.uint8).set_(out.untyped_storage(), 0, (out.untyped_storage().nbytes(),))
        raw[out.storage_offset() + out.numel()] = 0
    with pytest.raises(AssertionError, match="back guard"):
        h.guarded_u8(shape, past, device="cpu")
