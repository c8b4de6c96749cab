"""Guard bands and poisoned memory for tests that call the C ABI with raw pointers (tests/test_gpu_memory_contract.py; shown to
bite on CPU tensors by tests/test_guarded_cpu.py).  A `Guard` places every tensor of one call in the middle of a larger 1-D
allocation whose flanks hold a poison pattern, poisons the interior of the outputs as well, and `check()` asserts afterwards,
on raw bytes, that no flank has changed.  Three defects of a hand-tiled kernel then show:

  * a store outside the output (a ragged tile that is not clipped) changes a flank                          -> check() fails
  * an output element that is never written keeps the poison                                                 -> the bit compare fails
  * a load outside an input (a halo masked by multiplication, not by select) brings the poison into the sum  -> the bit compare fails

The float32 poison words are a quiet NaN with a payload, +FLT_MAX and -FLT_MAX, and a test runs under each of them: a ReLU
written as max(x, 0) turns the NaN into the 0 that zero padding would have given, while behind a BatchNorm scale of either sign
one of +-FLT_MAX survives it as a huge value.  Every other type is poisoned with the byte 0xA5; the flanks of a `mask` input
hold 1, the only code that changes what the kernels do with a pixel.  Works on any torch device."""
import numpy as np
import torch

QNAN, PLUS_MAX, MINUS_MAX = 0x7FC0A5A5, 0x7F7FFFFF, 0xFF7FFFFF
FLOAT_WORDS = (QNAN, PLUS_MAX, MINUS_MAX)
BYTE = 0xA5
BYTE_WORD = 0xA5A5A5A5
MASK_WORD = 0x01010101          # flanks of a `mask` input: code 1 ("use this pixel") in every byte
MIN_FLANK = 4096                # elements


def word_id(word):
    return {QNAN: "qnan", PLUS_MAX: "+fltmax", MINUS_MAX: "-fltmax"}.get(word, hex(word))


def _torch_dtype(np_dtype):
    return torch.from_numpy(np.empty(0, np_dtype)).dtype


class _Buffer:
    def __init__(self, name, raw, pattern, lo, nbytes, itemsize, view):
        self.name, self.raw, self.pattern, self.lo, self.nbytes, self.itemsize, self.view = name, raw, pattern, lo, nbytes, itemsize, view


class Guard:
    """The guarded buffers of one call.  word: the poison of float32 flanks and output interiors; skew = 1 starts every tensor
    one element past the aligned base (unless align16 is asked for), so that the tensor base has element alignment only."""

    def __init__(self, device, word=QNAN, skew=0):
        assert skew in (0, 1)
        self.device, self.word, self.skew = torch.device(device), int(word), int(skew)
        self.buffers = []

    # ---- placement -----------------------------------------------------------------------------
    def _alloc(self, shape, np_dtype, plane, align16, word, name):
        np_dtype = np.dtype(np_dtype)
        shape = tuple(int(s) for s in shape)
        n = int(np.prod(shape, dtype=np.int64))
        if plane is None:       # one H x W plane of the tensor: a ragged tile's overrun in y lands a row pitch past the end
            plane = shape[-1] * shape[-2] if len(shape) >= 2 else n
        item = np_dtype.itemsize
        flank = -(-max(MIN_FLANK, int(plane)) * item // 256) * 256            # bytes, a multiple of 256: the base stays aligned
        lo = flank + (0 if align16 else self.skew * item)
        nbytes = n * item
        total = -(-(lo + nbytes + flank) // 4) * 4
        if word is None:
            word = self.word if np_dtype == np.float32 else BYTE_WORD
        pattern = torch.from_numpy(np.full(total // 4, word, np.uint32).view(np.uint8).copy()).to(self.device)
        raw = pattern.clone()
        view = raw[lo:lo + nbytes].view(_torch_dtype(np_dtype)).view(shape)
        assert view.is_contiguous() and view.data_ptr() == raw.data_ptr() + lo
        if align16:
            assert view.data_ptr() % 16 == 0, "the allocator's base is not 16-byte aligned"
        elif self.skew and item < 16:
            assert view.data_ptr() % 16 != 0
        self.buffers.append(_Buffer(name or f"buffer {len(self.buffers)}", raw, pattern, lo, nbytes, item, view))
        return view

    def place(self, array, plane=None, align16=False, word=None, name=None):
        """An input: a contiguous view holding `array`, flanks poisoned (word: the flank pattern, MASK_WORD for a mask)."""
        array = np.ascontiguousarray(array)
        view = self._alloc(array.shape, array.dtype, plane, align16, word, name)
        view.copy_(torch.from_numpy(array.copy()))
        return view

    def empty(self, shape, dtype=np.float32, plane=None, align16=False, word=None, name=None):
        """An output (or a workspace): flanks AND interior poisoned, so that an element the call never writes keeps the poison."""
        return self._alloc(shape, dtype, plane, align16, word, name)

    # ---- checking ------------------------------------------------------------------------------
    def check(self):
        """Every flank of every buffer still holds its pattern, compared byte by byte; the first offending offset is reported
        in elements relative to the tensor (negative: before its start, >= numel: past its end)."""
        for b in self.buffers:
            hi = b.lo + b.nbytes
            for base, got, want in ((0, b.raw[:b.lo], b.pattern[:b.lo]), (hi, b.raw[hi:], b.pattern[hi:])):
                if torch.equal(got, want):
                    continue
                bad = torch.nonzero(got != want).reshape(-1)
                first = base + int(bad[0])
                off = (first - b.lo) // b.itemsize              # floor: byte -1 belongs to element -1
                side = "before the start" if first < b.lo else "past the end"
                raise AssertionError(f"{b.name}: {int(bad.numel())} guard byte(s) changed, the first at element offset {off} "
                                     f"({side} of a tensor of {b.nbytes // b.itemsize} elements)")


def as_bits(a):
    """A numpy array as integers of its element width: comparisons never go through float semantics (NaN != NaN, -0 == 0)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
    return a


def assert_bits(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = as_bits(got) != as_bits(want)
    if diff.any():
        first = int(np.flatnonzero(diff.reshape(-1))[0])
        raise AssertionError(f"{what}: {int(diff.sum())}/{want.size} elements differ, the first at flat index {first}: "
                             f"got {got.reshape(-1)[first]!r}, want {want.reshape(-1)[first]!r}")
