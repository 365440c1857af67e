"""Guarded buffers for the buffer contract of the C ABI (include/cvtt_mi355x.h, "Buffers").

A result read back from the tensor a call returned says what the call computed, not where it wrote: the caching allocator
hands a loop the previous, correct answer in its "empty" buffer, and nothing looks past the end.  The buffers here are one
allocation  [front guard | offset gap | payload | back guard]  filled with a poison byte; after the call the guards and the
gap must still be poison and the payload must equal the expected bytes exactly, so a byte the call did not write (it still
holds poison) and a byte it wrote outside its buffer are both reported, with their offsets relative to the payload.

A helper, not a conftest: tests import it.  device_* need torch and a GPU; host_buffer and the checks are plain numpy."""
import numpy as np

GUARD = 4096  # bytes of each guard band: at least this, and a multiple of 256


def _round_guard(nbytes):
    return max(GUARD, (int(nbytes) + 255) // 256 * 256)


def _span(bad):
    """first / last offending index and count of a boolean array"""
    idx = np.flatnonzero(bad)
    return int(idx[0]), int(idx[-1]), int(idx.size)


def verify(raw, front, offset, nbytes, poison, expected, what="buffer"):
    """raw: the whole allocation as uint8 numpy; the payload is raw[front + offset : front + offset + nbytes].  Asserts, in
    this order: both guards hold `poison`; the offset gap holds `poison`; the payload equals `expected` (bytes-like or
    array, exactly nbytes).  Offsets in the messages are relative to the payload's first byte."""
    raw = np.asarray(raw, np.uint8).reshape(-1)
    start = front + offset
    end = start + nbytes
    assert end <= raw.size
    for name, lo, hi in (("front guard", 0, front), ("back guard", end, raw.size), ("offset gap", front, start)):
        bad = raw[lo:hi] != poison
        if bad.any():
            first, last, count = _span(bad)
            raise AssertionError("%s: %d byte(s) of the %s overwritten, payload offsets %d .. %d (payload is %d bytes)"
                                 % (what, count, name, lo + first - start, lo + last - start, nbytes))
    exp = np.frombuffer(np.ascontiguousarray(expected).tobytes(), np.uint8) if not isinstance(expected, (bytes, bytearray)) \
        else np.frombuffer(bytes(expected), np.uint8)
    assert exp.size == nbytes, "%s: expected %d bytes, the payload has %d" % (what, exp.size, nbytes)
    bad = raw[start:end] != exp
    if bad.any():
        first, last, count = _span(bad)
        unwritten = int((bad & (raw[start:end] == poison)).sum())
        raise AssertionError("%s: %d payload byte(s) differ from the expected bytes, offsets %d .. %d (%d of them still hold "
                             "the poison 0x%02X: not written)" % (what, count, first, last, unwritten, poison))


def verify_no_poison_blocks(raw, front, offset, nbytes, poison, block_bytes, what="buffer"):
    """the payload holds no block of `block_bytes` poison bytes (for parts of a large result no reference is computed for)"""
    payload = np.asarray(raw, np.uint8).reshape(-1)[front + offset: front + offset + nbytes].reshape(-1, block_bytes)
    bad = (payload == poison).all(axis=1)
    if bad.any():
        first, last, count = _span(bad)
        raise AssertionError("%s: %d block(s) still hold the poison 0x%02X, payload offsets %d .. %d"
                             % (what, count, poison, first * block_bytes, (last + 1) * block_bytes - 1))


class _Checker:
    def __init__(self, snapshot, front, offset, nbytes, poison, what):
        self._snapshot, self.front, self.offset, self.nbytes, self.poison, self.what = snapshot, front, offset, nbytes, poison, what

    def __call__(self, expected_bytes):
        verify(self._snapshot(), self.front, self.offset, self.nbytes, self.poison, expected_bytes, self.what)

    check = __call__

    def untouched(self):
        """the call wrote nothing at all: guards, gap and payload still hold the poison"""
        verify(self._snapshot(), self.front, self.offset, self.nbytes, self.poison,
               np.full(self.nbytes, self.poison, np.uint8), self.what)

    def payload(self):
        return self._snapshot()[self.front + self.offset: self.front + self.offset + self.nbytes].copy()

    def no_poison_blocks(self, block_bytes):
        verify_no_poison_blocks(self._snapshot(), self.front, self.offset, self.nbytes, self.poison, block_bytes, self.what)


def host_buffer(nbytes, offset=0, poison=0xA5, back=GUARD, what="host buffer"):
    """numpy form: (payload view, checker).  The allocation starts on a 256-byte boundary, so the payload's address is
    256-aligned + offset; any byte offset is allowed (host pointers need no alignment)."""
    front, back = GUARD, _round_guard(back)
    total = front + offset + nbytes + back
    store = np.empty(total + 256, np.uint8)
    skew = (-store.ctypes.data) % 256
    raw = store[skew: skew + total]
    raw[:] = poison
    view = raw[front + offset: front + offset + nbytes]
    assert view.ctypes.data == raw.ctypes.data + front + offset
    return view, _Checker(lambda: raw, front, offset, nbytes, poison, what)


def device_buffer(nbytes, offset=0, poison=0xA5, back=GUARD, what="device buffer"):
    """one uint8 CUDA tensor of front + offset + nbytes + back bytes, every byte `poison`; returns (payload view, checker)
    with view.data_ptr() == base + front + offset.  checker(expected_bytes) synchronises and reads the allocation back."""
    import torch
    front, back = GUARD, _round_guard(back)
    raw = torch.full((front + offset + nbytes + back,), poison, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 256 == 0
    view = raw[front + offset: front + offset + nbytes]
    assert view.data_ptr() == raw.data_ptr() + front + offset

    def snapshot():
        torch.cuda.synchronize()
        return raw.cpu().numpy()
    return view, _Checker(snapshot, front, offset, nbytes, poison, what)


def device_input(array, offset=0, poison=0x3C, what="input"):
    """the bytes of `array` placed `offset` bytes into a larger poisoned CUDA allocation: returns (view, unchanged) where
    unchanged() asserts that neither the input bytes nor the poison around them were modified"""
    import torch
    data = np.frombuffer(np.ascontiguousarray(array).tobytes(), np.uint8)
    front = GUARD
    image = np.full(front + offset + data.size + GUARD, poison, np.uint8)
    image[front + offset: front + offset + data.size] = data
    raw = torch.from_numpy(image).cuda()
    assert raw.data_ptr() % 256 == 0
    view = raw[front + offset: front + offset + data.size]

    def unchanged():
        torch.cuda.synchronize()
        now = raw.cpu().numpy()
        bad = now != image
        if bad.any():
            first, last, count = _span(bad)
            raise AssertionError("%s: the call modified %d byte(s) of its input allocation, input offsets %d .. %d (input is %d bytes)"
                                 % (what, count, first - front - offset, last - front - offset, data.size))
    return view, unchanged
