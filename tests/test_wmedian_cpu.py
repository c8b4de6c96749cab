"""The weighted median filter without a GPU: the sort-based restatement (tests/wmedian_reference.py) against an independent brute
force and against np.median, the weight table, the exported symbol, the argument errors of lws_wmedian_filter through the C ABI
and the CLI flags."""
import numpy as np
import pytest

import speckle_inputs as I
import wmedian_reference as R
from lwsnet_amd import _lib


def brute_force(disp, mask, rgb, wlut, radius, fill_min):
    """Per pixel, in plain Python: for every candidate value the weights of the candidates <= it are summed, and the smallest
    value whose doubled sum reaches the total is the answer.  No sort, no cumulative sum."""
    B, _, H, W = disp.shape
    out = np.zeros_like(disp)
    counts = np.zeros((B, 2), np.int64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                def ok(qy, qx):
                    v = disp[b, 0, qy, qx]
                    return bool(np.isfinite(v)) and v > 0 and (mask is None or mask[b, 0, qy, qx] == 1)

                cand = []
                for qy in range(max(0, y - radius), min(H, y + radius + 1)):
                    for qx in range(max(0, x - radius), min(W, x + radius + 1)):
                        if not ok(qy, qx):
                            continue
                        w = 1
                        if rgb is not None:
                            w = int(wlut[sum(abs(int(rgb[b, y, x, c]) - int(rgb[b, qy, qx, c])) for c in range(3))])
                        if w > 0:
                            cand.append((disp[b, 0, qy, qx], w))
                total = sum(w for _, w in cand)
                best = None
                for v, _ in cand:
                    if 2 * sum(w for u, w in cand if u <= v) >= total and (best is None or v < best):
                        best = v
                d = disp[b, 0, y, x]
                if ok(y, x):
                    o = d if total == 0 else best
                    counts[b, 0] += int(np.float32(o).view(np.uint32) != np.float32(d).view(np.uint32))
                elif fill_min > 0 and len(cand) >= fill_min:
                    o = best
                    counts[b, 1] += 1
                else:
                    o = np.float32(0.0)
                out[b, 0, y, x] = o
    return out, counts


def guide(B, H, W, seed):
    """A few constant colour regions plus noise of a few grey levels: s covers 0, small values and values in the hundreds."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    K = 5
    cy, cx = rng.uniform(0, H, K), rng.uniform(0, W, K)
    region = np.argmin((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2, axis=0)
    colour = rng.integers(0, 256, (K, 3))
    g = colour[region][None] + rng.integers(-3, 4, (B, H, W, 3)) * (rng.uniform(size=(B, H, W, 1)) < 0.5)
    return np.clip(g, 0, 255).astype(np.uint8)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("seed", range(12))
def test_reference_equals_brute_force(seed):
    from lwsnet_amd import ops
    rng = np.random.default_rng(seed)
    B, H, W = 1 + seed % 2, int(rng.integers(1, 13)), int(rng.integers(1, 17))
    radius = 1 + seed % 3
    if seed % 3 == 0:                                       # a few levels only: ties everywhere
        d = (np.round(rng.uniform(1, 4, (B, 1, H, W))) * 0.75).astype(np.float32)
    else:
        d = rng.uniform(0.5, 60.0, (B, 1, H, W)).astype(np.float32)
    d = I.plant_specials(d, rng)
    d.reshape(-1)[rng.integers(0, d.size, max(1, d.size // 6))] = 0.0       # holes
    mask = I.random_mask(B, H, W, seed + 50) if seed % 4 != 1 else None
    rgb = guide(B, H, W, seed) if seed % 4 != 2 else None
    tables = [ops.wmedian_lut(2.0), ops.wmedian_lut(40.0), np.concatenate([[0], np.full(765, 7)]).astype(np.uint16)]
    wlut = tables[seed % 3] if rgb is not None else None
    for fill_min in (0, 1, 4):
        want, wc = brute_force(d, mask, rgb, wlut, radius, fill_min)
        got, gc = R.wmedian_filter(d, radius, rgb, wlut, mask, fill_min)
        assert np.array_equal(bits(got), bits(want)), (seed, fill_min)
        assert np.array_equal(gc, wc), (seed, fill_min)


def test_unweighted_interior_is_the_ordinary_median():
    rng = np.random.default_rng(3)
    d = rng.uniform(1.0, 50.0, (2, 1, 17, 23)).astype(np.float32)
    out, counts = R.wmedian_filter(d, 1)
    win = np.lib.stride_tricks.sliding_window_view(d[:, 0], (3, 3), axis=(1, 2)).reshape(2, 15, 21, 9)
    assert np.array_equal(bits(out[:, 0, 1:-1, 1:-1]), bits(np.median(win, axis=-1).astype(np.float32)))
    # the clipped corner window has four values: the lower of the two middle ones
    assert out[0, 0, 0, 0] == np.sort(d[0, 0, :2, :2].reshape(-1))[1]
    assert counts[:, 1].tolist() == [0, 0] and (counts[:, 0] > 0).all()


def test_all_ones_table_equals_no_guide():
    rng = np.random.default_rng(4)
    d = I.plant_specials(rng.uniform(1.0, 50.0, (2, 1, 19, 31)).astype(np.float32), rng)
    mask = I.random_mask(2, 19, 31, 5)
    ones = np.ones(R.LUT_SIZE, np.uint16)
    for radius in (1, 2, 3):
        a, ac = R.wmedian_filter(d, radius, guide(2, 19, 31, 6), ones, mask, 4)
        b, bc = R.wmedian_filter(d, radius, None, None, mask, 4)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(ac, bc)


def test_table_with_zero_self_weight_keeps_a_lonely_pixel():
    """wlut[0] == 0 on a constant guide: no candidate anywhere, T == 0, every valid pixel keeps its value and no hole is filled."""
    d = np.array([[5, 0, 7], [np.nan, 3, 9]], np.float32)[None, None]
    wlut = np.concatenate([[0], np.full(765, 9)]).astype(np.uint16)
    out, counts = R.wmedian_filter(d, 1, np.full((1, 2, 3, 3), 80, np.uint8), wlut, None, 1)
    assert out[0, 0].tolist() == [[5, 0, 7], [0, 3, 9]] and counts.tolist() == [[0, 0]]


def test_wmedian_lut():
    from lwsnet_amd import ops
    for sigma, scale in ((2.0, 4096), (10.0, 4096), (40.0, 65535), (0.3, 1)):
        t = ops.wmedian_lut(sigma, scale)
        assert t.dtype == np.uint16 and t.shape == (766,)
        assert t[0] == scale and (np.diff(t.astype(np.int64)) <= 0).all()
    # exp(-30 / 30) = 0.36787944...: 4096 * 0.36787944 = 1506.83
    assert ops.wmedian_lut(10.0)[30] == 1507
    assert ops.wmedian_lut(2.0)[60] == 0 and ops.wmedian_lut(2.0)[6] == 1507        # many zero weights at a small sigma
    assert ops.wmedian_lut(10.0, scale=np.int64(100))[0] == 100
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "3"):
        with pytest.raises(ValueError, match="sigma"):
            ops.wmedian_lut(bad)
    for bad in (0, 65536, -5, 1.5, None):
        with pytest.raises(ValueError, match="scale"):
            ops.wmedian_lut(10.0, bad)


def test_library_exports_the_entry_point(hip_lib):
    assert "lws_wmedian_filter" in _lib.PROTOTYPES
    assert hip_lib.lws_wmedian_filter.argtypes == _lib.PROTOTYPES["lws_wmedian_filter"][1]
    assert hip_lib.lws_abi_version() == 8


def _call(lib, disp=1 << 20, mask=None, rgb=None, wlut=None, B=1, H=8, W=8, radius=2, fill_min=0, out=1 << 21, counts=None):
    """lws_wmedian_filter with made-up (never dereferenced) device addresses: every argument error returns before any GPU call."""
    return lib.lws_wmedian_filter(disp, mask, rgb, wlut, B, H, W, radius, fill_min, out, counts, None)


def test_argument_errors_through_the_c_abi(hip_lib):
    lib = hip_lib
    bad = [dict(radius=0), dict(radius=4), dict(radius=-1), dict(fill_min=-1), dict(rgb=1 << 22), dict(disp=None), dict(out=None),
           dict(B=0), dict(B=65536), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(out=(1 << 20)), dict(out=(1 << 20) + 64),
           dict(mask=(1 << 21) + 8), dict(rgb=(1 << 21) + 100, wlut=1 << 23), dict(rgb=1 << 22, wlut=(1 << 21) + 16),
           dict(counts=(1 << 21) + 32), dict(counts=(1 << 20) + 32), dict(mask=1 << 22, counts=(1 << 22) + 8),
           dict(rgb=1 << 22, wlut=1 << 23, counts=(1 << 22) + 8), dict(rgb=1 << 22, wlut=1 << 23, counts=(1 << 23) + 1000),
           dict(disp=(1 << 20) + 2), dict(counts=(1 << 24) + 4), dict(rgb=1 << 22, wlut=(1 << 23) + 1)]
    for kw in bad:
        assert _call(lib, **kw) == _lib.LWS_ERR_INVALID, kw
        assert lib.lws_last_error().startswith(b"wmedian_filter:"), (kw, lib.lws_last_error())
        with pytest.raises(ValueError, match="wmedian_filter"):
            _lib.check(_lib.LWS_ERR_INVALID)
    assert _call(lib, radius=4) == _lib.LWS_ERR_INVALID and b"radius" in lib.lws_last_error()
    assert _call(lib, fill_min=-1) == _lib.LWS_ERR_INVALID and b"fill_min" in lib.lws_last_error()
    assert _call(lib, rgb=1 << 22) == _lib.LWS_ERR_INVALID and b"wlut" in lib.lws_last_error()
    assert _call(lib, H=65536, W=32768) == _lib.LWS_ERR_INVALID and b"2^31" in lib.lws_last_error()
    assert _call(lib, out=(1 << 20) + 64) == _lib.LWS_ERR_INVALID and b"disp and out overlap" in lib.lws_last_error()


# (moved buffer, the written buffer it is moved 8 bytes into, the whole error): every written / any pair, each alone
_OVERLAPS = [
    ("counts", "out", b"wmedian_filter: counts and out overlap"), ("disp", "out", b"wmedian_filter: disp and out overlap"),
    ("mask", "out", b"wmedian_filter: mask and out overlap"), ("rgb", "out", b"wmedian_filter: rgb and out overlap"),
    ("wlut", "out", b"wmedian_filter: wlut and out overlap"), ("disp", "counts", b"wmedian_filter: disp and counts overlap"),
    ("mask", "counts", b"wmedian_filter: mask and counts overlap"), ("rgb", "counts", b"wmedian_filter: rgb and counts overlap"),
    ("wlut", "counts", b"wmedian_filter: wlut and counts overlap"),
]


def test_every_overlapping_pair_is_named(hip_lib):
    base = dict(disp=1 << 20, out=1 << 21, mask=1 << 22, wlut=1 << 23, counts=1 << 24, rgb=1 << 25)
    for moved, onto, msg in _OVERLAPS:
        assert _call(hip_lib, **{**base, moved: base[onto] + 8}) == _lib.LWS_ERR_INVALID, (moved, onto)
        assert hip_lib.lws_last_error() == msg


def test_shared_checks_keep_their_whole_text(hip_lib):
    cases = [(dict(B=0), b"wmedian_filter: bad shape B=0 H=8 W=8"), (dict(B=65536), b"wmedian_filter: bad shape B=65536 H=8 W=8"),
             (dict(H=0), b"wmedian_filter: bad shape B=1 H=0 W=8"), (dict(W=-1), b"wmedian_filter: bad shape B=1 H=8 W=-1"),
             (dict(H=65536, W=32768), b"wmedian_filter: H*W = 65536x32768 must be < 2^31"),
             (dict(disp=(1 << 20) + 2), b"wmedian_filter: disp / out must be 4-byte, counts 8-byte, wlut 2-byte aligned"),
             (dict(counts=(1 << 24) + 4), b"wmedian_filter: disp / out must be 4-byte, counts 8-byte, wlut 2-byte aligned"),
             (dict(rgb=1 << 22, wlut=(1 << 23) + 1), b"wmedian_filter: disp / out must be 4-byte, counts 8-byte, wlut 2-byte aligned")]
    for kw, msg in cases:
        assert _call(hip_lib, **kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw


def test_ops_validates_before_the_library():
    from lwsnet_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.wmedian_filter(np.zeros((1, 1, 8, 8), np.float32), 1)


ARGV_ERRORS = [["--wmedian_sigma", "5"], ["--wmedian_fill", "4"], ["--wmedian", "0"], ["--wmedian", "4"], ["--wmedian", "-1"],
               ["--wmedian", "2", "--wmedian_sigma", "nan"], ["--wmedian", "2", "--wmedian_sigma", "-1"],
               ["--wmedian", "2", "--wmedian_sigma", "inf"], ["--wmedian", "2", "--wmedian_fill", "-1"], ["--wmedian", "2", "--workers", "4"]]


@pytest.mark.parametrize("argv", ARGV_ERRORS)
def test_cli_argument_errors(argv, capsys, monkeypatch):
    from lwsnet_amd import evaluate, inference
    loaded = []
    monkeypatch.setattr(inference, "load_model", lambda *a, **k: loaded.append("inference"))
    monkeypatch.setattr(evaluate, "load_model", lambda *a, **k: loaded.append("evaluate"))
    monkeypatch.setattr(evaluate, "load_dataset", lambda *a, **k: loaded.append("dataset"))
    for mod in (inference, evaluate):
        p = mod.build_parser()
        args = p.parse_args(argv)
        with pytest.raises(SystemExit) as e:
            inference.check_wmedian_arguments(p, args)
        assert e.value.code == 2
        assert "--wmedian" in capsys.readouterr().err
    for main, extra in ((inference.main, ["--synthetic_weights", "--left_img", "nowhere/left.png"]), (evaluate.main, ["--synthetic_weights"])):
        with pytest.raises(SystemExit) as e:
            main(extra + argv)
        assert e.value.code == 2
        assert "--wmedian" in capsys.readouterr().err
    assert loaded == [], "a parser error must come before any model or dataset work"


def test_cli_defaults():
    from lwsnet_amd import evaluate, inference
    for mod in (inference, evaluate):
        p = mod.build_parser()
        args = p.parse_args(["--wmedian", "2"])
        inference.check_wmedian_arguments(p, args)
        assert args.wmedian == 2 and args.wmedian_sigma == 10.0 and args.wmedian_fill == 0
        args = p.parse_args(["--wmedian", "3", "--wmedian_sigma", "0", "--wmedian_fill", "4"])
        inference.check_wmedian_arguments(p, args)
        assert args.wmedian == 3 and args.wmedian_sigma == 0.0 and args.wmedian_fill == 4
        args = p.parse_args([])
        inference.check_wmedian_arguments(p, args)
        assert args.wmedian is None and args.wmedian_sigma is None and args.wmedian_fill is None
