"""The guard checker of tests/guarded.py sees damage: the negative control of the memory-contract tests, on CPU tensors.

The GPU tests never break a kernel to prove themselves; this file flips single bytes instead.
"""
import numpy as np
import pytest

from guarded import ALIGN, Guarded


@pytest.mark.parametrize("misalign", [0, 1, 4, 255])
def test_layout(misalign):
    w, h = 37, 50
    dtype, shape = (np.uint8, (h, w)) if misalign % 4 else (np.float32, (h, w))
    nbytes = w * h * np.dtype(dtype).itemsize
    g = Guarded(nbytes, dtype, shape, misalign=misalign, plane=w * h, device="cpu")
    guard = 8192                                               # 4 * 37 * 50 = 7400, rounded up to 4096
    assert g.view.data_ptr() % ALIGN == misalign and g.ptr.value == g.view.data_ptr()
    assert tuple(g.view.shape) == shape and g.view.numel() * g.view.element_size() == nbytes
    assert g.front >= guard and g.buf.numel() - g.front - nbytes >= guard
    assert bool((g.buf == 0xA5).all())                         # guards and payload alike
    assert Guarded(16, np.uint8, (16,), device="cpu").front >= 4096
    g.check("fresh")
    g.check_untouched("fresh")


def test_a_flipped_guard_byte_is_seen_and_a_payload_byte_is_not():
    n = 1000
    g = Guarded(n, np.uint8, (n,), misalign=1, device="cpu")
    g.load(np.arange(n, dtype=np.uint8))
    g.check_unchanged("loaded")
    assert g.damage() is None
    # the payload is the call's to write: no guard damage
    g.view[0] ^= 1
    g.view[n - 1] ^= 1
    g.check("payload written")
    with pytest.raises(AssertionError, match="input was modified, first at byte 0, last at 999"):
        g.check_unchanged("payload written")
    with pytest.raises(AssertionError, match="written although nothing ran"):
        g.check_untouched("payload written")
    # one byte in the front guard: the byte just before the payload
    g.buf[g.front - 1] ^= 0x10
    assert g.damage() == (-1, -1)
    with pytest.raises(AssertionError, match="first damaged byte at offset -1, last at -1"):
        g.check("front")
    g.buf[g.front - 1] = g.fill
    g.check("front repaired")
    # one byte in the back guard: the byte just behind the payload, then also the very last one
    g.buf[g.front + n] = 0
    assert g.damage() == (n, n)
    with pytest.raises(AssertionError, match=f"first damaged byte at offset {n}, last at {n}"):
        g.check("back")
    last = g.buf.numel() - 1 - g.front
    g.buf[-1] = 0
    assert g.damage() == (n, last)
    # both guards: first in the front one, last in the back one
    g.buf[0] = 0
    assert g.damage() == (-g.front, last)
    with pytest.raises(AssertionError, match=f"offset {-g.front}, last at {last}"):
        g.check("both")


@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_other_fills(fill):
    g = Guarded(64, np.int64, (8,), misalign=8, fill=fill, device="cpu")
    assert bool((g.buf == fill).all())
    g.check_untouched("fresh")
    g.buf[g.front + 64 + 5] = 0xA5
    assert g.damage() == (69, 69)
