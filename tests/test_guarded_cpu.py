"""tests/guarded.py bites: on CPU tensors, small Python stand-ins for a kernel -- one correct, the others each with ONE of the
defects the guard bands and the poison are for -- and the check meant for each defect catches it, under every poison word
where the word matters.  (No defect is ever planted in a HIP kernel: the harness is proven here, the kernels are held to it in
tests/test_gpu_memory_contract.py.)  Also the host-side errors of lws_debug_fill_workspace, which need no GPU."""
import ctypes

import numpy as np
import pytest

import guarded as G

torch = pytest.importorskip("torch")

H, W = 6, 10
WORDS = pytest.mark.parametrize("word", G.FLOAT_WORDS, ids=G.word_id)
SKEWS = pytest.mark.parametrize("skew", [0, 1])


def _raw(g, t):
    """(flat view of the whole allocation as the tensor's type, index of the tensor's first element in it) -- what a kernel
    with a wrong index reaches through the pointer it was given."""
    b = next(b for b in g.buffers if b.view is t)
    return b.raw[:b.raw.numel() // b.itemsize * b.itemsize].view(t.dtype), b.lo // b.itemsize


def want(x):
    return (x.astype(np.float32) * np.float32(2.0) + np.float32(1.0)).astype(np.float32)


def k_correct(g, x, out):
    out.copy_(x * 2.0 + 1.0)


def k_one_past_the_end(g, x, out):
    k_correct(g, x, out)
    flat, first = _raw(g, out)
    flat[first + out.numel()] = 3.0


def k_one_before_the_start(g, x, out):
    k_correct(g, x, out)
    flat, first = _raw(g, out)
    flat[first - 1] = 3.0


def k_one_row_pitch_past_the_end(g, x, out):
    """A ragged tile in y that is not clipped: row H of an H-row plane."""
    k_correct(g, x, out)
    flat, first = _raw(g, out)
    flat[first + out.numel() + (W - 1)] = 3.0              # (row H, last column: one pitch past the last element)


def k_skips_an_interior_element(g, x, out):
    y = x * 2.0 + 1.0
    keep = out.reshape(-1)[H * W // 2 + 3].clone()
    out.copy_(y)
    out.reshape(-1)[H * W // 2 + 3] = keep


def k_sum_reads_the_flank(g, x, out):
    """A 2-tap row sum whose right tap at the last element of the tensor is not masked: it reads the element past the end."""
    flat, first = _raw(g, x)
    n = x.numel()
    out.reshape(-1).copy_(flat[first:first + n] + flat[first + 1:first + n + 1])


def want_sum(x):
    f = x.reshape(-1)
    return (f + np.concatenate([f[1:], np.zeros(1, np.float32)])).reshape(x.shape)


def run(kernel, word, skew, ref=want):
    x_np = np.random.default_rng(1).standard_normal((2, H, W)).astype(np.float32)
    g = G.Guard("cpu", word, skew)
    x, out = g.place(x_np, name="x"), g.empty(x_np.shape, name="out")
    kernel(g, x, out)
    return g, out, ref(x_np)


@WORDS
@SKEWS
def test_correct_writer_passes(word, skew):
    g, out, ref = run(k_correct, word, skew)
    G.assert_bits(out, ref, "out")
    g.check()


@WORDS
@SKEWS
@pytest.mark.parametrize("kernel,offset", [(k_one_past_the_end, H * W * 2), (k_one_before_the_start, -1),
                                           (k_one_row_pitch_past_the_end, H * W * 2 + W - 1)])
def test_a_store_outside_the_output_changes_a_flank(word, skew, kernel, offset):
    g, out, ref = run(kernel, word, skew)
    G.assert_bits(out, ref, "out")                         # the values inside are right: only the flank tells
    with pytest.raises(AssertionError, match=rf"out: 4 guard byte\(s\) changed, the first at element offset {offset} "):
        g.check()


@WORDS
@SKEWS
def test_an_element_never_written_keeps_the_poison(word, skew):
    g, out, ref = run(k_skips_an_interior_element, word, skew)
    g.check()                                              # no flank was touched: only the bit compare tells
    with pytest.raises(AssertionError, match=rf"1/{2 * H * W} elements differ, the first at flat index {H * W // 2 + 3}:"):
        G.assert_bits(out, ref, "out")
    assert int(G.as_bits(out.numpy()).reshape(-1)[H * W // 2 + 3]) == word


@WORDS
@SKEWS
def test_a_load_from_the_flank_reaches_the_result(word, skew):
    g, out, ref = run(k_sum_reads_the_flank, word, skew, want_sum)
    g.check()
    with pytest.raises(AssertionError, match=rf"1/{2 * H * W} elements differ, the first at flat index {2 * H * W - 1}:"):
        G.assert_bits(out, ref, "out")


def test_all_three_words_are_needed_behind_a_relu():
    """The halo tap of a BatchNorm(scale s) -> ReLU -> sum stand-in, read from the flank instead of being zero: with the ReLU
    written as max(v, 0) (fmaxf drops a NaN) the quiet NaN gives the very 0 that padding gives, and of +-FLT_MAX exactly the
    one whose sign matches the scale survives.  Every defect is caught by at least one word; no single word catches both signs."""
    x_np = np.abs(np.random.default_rng(2).standard_normal((1, H, W))).astype(np.float32)
    caught = {}
    for scale in (1.0, -1.0):
        ref = np.maximum(x_np * np.float32(scale), 0) + 0.0                      # the halo tap contributes max(0 * s, 0) = 0
        for word in G.FLOAT_WORDS:
            g = G.Guard("cpu", word)
            x = g.place(x_np)
            flat, first = _raw(g, x)
            halo = flat[first + x.numel()] * scale                               # the unmasked tap
            halo = torch.where(halo > 0, halo, torch.zeros(()))                  # max(v, 0) the way fmaxf computes it: NaN -> 0
            out = torch.clamp(x * scale, min=0) + halo
            caught[scale, word] = not np.array_equal(G.as_bits(out.numpy()), G.as_bits(ref.astype(np.float32)))
            g.check()
    assert caught == {(1.0, G.QNAN): False, (1.0, G.PLUS_MAX): True, (1.0, G.MINUS_MAX): False,
                      (-1.0, G.QNAN): False, (-1.0, G.PLUS_MAX): False, (-1.0, G.MINUS_MAX): True}


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32, np.int64, np.float64])
@SKEWS
def test_other_types_are_poisoned_with_the_byte(dtype, skew):
    g = G.Guard("cpu", G.PLUS_MAX, skew)
    a = np.arange(35, dtype=dtype).reshape(5, 7)
    t = g.place(a, name="in")
    o = g.empty((5, 7), dtype, name="out")
    assert np.array_equal(t.numpy(), a)
    assert (o.numpy().view(np.uint8) == G.BYTE).all()
    for b in g.buffers:
        assert (b.raw[:b.lo].numpy() == G.BYTE).all() and (b.raw[b.lo + b.nbytes:].numpy() == G.BYTE).all()
    g.check()
    flat, first = _raw(g, o)
    flat[first + 35] = 0
    with pytest.raises(AssertionError, match="out: .* the first at element offset 35 "):
        g.check()


def test_placement_flanks_alignment_and_mask_word():
    g = G.Guard("cpu", G.QNAN, skew=1)
    small = g.place(np.zeros((2, 1, 3, 5), np.float32))
    big = g.place(np.zeros((2, 1, 100, 90), np.float32))
    rgb = g.place(np.zeros((2, 9, 11, 3), np.uint8), plane=9 * 11 * 3)
    rec = g.empty((2, 50 * 70, 16), np.uint8, plane=50 * 70 * 16, align16=True)
    mask = g.place(np.zeros((1, 1, 4, 4), np.uint8), word=G.MASK_WORD)
    for t, flank, item in ((small, G.MIN_FLANK, 4), (big, 9000, 4), (rgb, G.MIN_FLANK, 1), (rec, 50 * 70 * 16, 1), (mask, G.MIN_FLANK, 1)):
        b = next(b for b in g.buffers if b.view is t)
        assert b.lo >= flank * item and b.raw.numel() - b.lo - b.nbytes >= flank * item
        assert t.is_contiguous() and t.data_ptr() % item == 0
    assert small.data_ptr() % 16 == 4 and big.data_ptr() % 16 == 4 and rgb.data_ptr() % 16 == 1      # element alignment only
    assert rec.data_ptr() % 16 == 0                                                                  # where the header demands it
    b = next(b for b in g.buffers if b.view is mask)
    assert (b.raw[:b.lo].numpy() == 1).all() and (b.raw[b.lo + b.nbytes:].numpy() == 1).all()
    b = next(b for b in g.buffers if b.view is small)
    assert (b.raw[b.lo + b.nbytes:].view(torch.int32).numpy().view(np.uint32) == G.QNAN).all()
    g.check()


def test_fill_workspace_hook_validates_on_host(hip_lib):
    """lws_debug_fill_workspace (include/lwsnet_hip.h): the device rule of every handle call, then LWS_ERR_STATE while the handle
    has no workspace -- both before any HIP work, so without a GPU."""
    from lwsnet_amd import _lib
    from lwsnet_amd.weights import default_args
    a = default_args()
    cfg = _lib.LwsConfig((ctypes.c_int32 * 3)(*a.maxdisplist), a.layers_3d, a.channels_3d, (ctypes.c_int32 * 3)(*a.growth_rate), 0,
                         a.interp_align_mode)
    h = ctypes.c_void_p()
    assert hip_lib.lws_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    assert hip_lib.lws_debug_fill_workspace(None, G.QNAN, None) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_debug_fill_workspace(h, G.QNAN, None) == _lib.LWS_ERR_STATE
    assert b"no workspace yet" in hip_lib.lws_last_error()
    assert hip_lib.lws_set_option(h, b"device", 5) == 0
    assert hip_lib.lws_debug_fill_workspace(h, G.QNAN, None) == _lib.LWS_ERR_INVALID
    assert b"belongs to HIP device 5" in hip_lib.lws_last_error()
    assert hip_lib.lws_destroy(h) == 0
