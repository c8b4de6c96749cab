"""The left-right consistency check without a GPU: the numpy restatement (tests/lr_reference.py) on constructed rows, the host-side
argument checks of lws_lr_check / lws_lr_pairs, and the CLIs' refusal of --lr_check with --workers."""
import ctypes

import numpy as np
import pytest

import lr_reference as R
from lwsnet_amd import _lib


def _row(vals):
    return np.asarray(vals, np.float32).reshape(1, 1, 1, -1)


def forward_warp_right(dl):
    """z-buffered forward warp of a left-view row: right pixel x - d takes the largest disparity that lands there (the nearest
    surface); holes get the background value min(dl).  Returns the mirrored right-view row dRm."""
    W = dl.shape[-1]
    right = np.full(W, -np.inf, np.float32)
    for x in range(W):
        xr = x - int(dl[x])
        if 0 <= xr < W:
            right[xr] = max(right[xr], dl[x])
    right[np.isinf(right)] = dl.min()
    return right[::-1].copy()


def test_constant_disparity_is_out_of_view_left_of_d0():
    W, d0 = 64, 7
    dl = _row(np.full(W, d0))
    out, code, right, kept = R.lr_check(dl, dl, 1.0, fill=False)
    x = np.arange(W)
    assert np.array_equal(code[0, 0, 0], np.where(x < d0, 2, 1))
    assert np.array_equal(out[0, 0, 0], np.where(x < d0, 0, d0).astype(np.float32))
    assert kept.tolist() == [[W - d0]]
    # fill: the out-of-view band has only a right neighbour
    out, _, _, _ = R.lr_check(dl, dl, 1.0, fill=True)
    assert np.all(out == d0)


def test_occlusion_band_left_of_foreground_is_inconsistent_and_filled_with_background():
    W, x0, x1 = 200, 100, 140
    d = np.full(W, 10.0, np.float32)
    d[x0:x1] = 40.0
    drm = forward_warp_right(d)
    out, code, _, _ = R.lr_check(_row(d), _row(drm), 1.0, fill=False)
    c = code[0, 0, 0]
    assert np.all(c[:10] == 2) and np.all(c[10:x0 - 30] == 1)
    assert np.all(c[x0 - 30:x0] == 0), "the band of width 30 left of the block is occluded in the right view"
    assert np.all(c[x0:] == 1)
    assert np.all(out[0, 0, 0, x0 - 30:x0] == 0)
    filled, _, _, _ = R.lr_check(_row(d), _row(drm), 1.0, fill=True)
    f = filled[0, 0, 0]
    assert np.all(f[x0 - 30:x0] == 10.0) and np.all(f[x0:x1] == 40.0) and np.all(f[:10] == 10.0)


def test_difference_equal_to_tau_is_consistent():
    W = 32
    dl, drm = _row(np.full(W, 5.0)), _row(np.full(W, 5.5))
    code = R.lr_codes(dl, drm, 0.5)[0, 0, 0]
    assert np.all(code[5:] == 1) and np.all(code[:5] == 2)
    code = R.lr_codes(dl, drm, np.nextafter(np.float32(0.5), np.float32(0)))[0, 0, 0]
    assert np.all(code[5:] == 0)


def test_nan_is_inconsistent_and_inf_out_of_view():
    W = 16
    d = np.full(W, 2.0, np.float32)
    d[4], d[6], d[8] = np.nan, np.inf, -np.inf
    drm = np.full(W, 2.0, np.float32)
    drm[3] = np.nan                                          # t = 3 at x = 14; at x = 15, t = 2 and a = 0, but r = R[2] + 0 * NaN
    out, code, _, kept = R.lr_check(_row(d), _row(drm), 1.0, fill=True)
    c = code[0, 0, 0]
    assert c[4] == 0 and c[6] == 2 and c[8] == 2 and c[14] == 0 and c[15] == 0 and c[13] == 1
    assert np.all(np.isfinite(out))
    assert kept[0, 0] == W - 2 - 5                           # x < 2 out of view, plus 4, 6, 8, 14, 15


def test_fill_takes_the_smaller_neighbour_and_zero_for_an_empty_row():
    dl = _row([3, 9, 9, 9, 5, 9])
    code = np.array([1, 0, 0, 0, 1, 0], np.uint8).reshape(dl.shape)
    assert R.background_fill(dl, code)[0, 0, 0].tolist() == [3, 3, 3, 3, 5, 5]
    assert np.all(R.background_fill(dl, np.zeros_like(code)) == 0)


def test_lr_pairs_restatement():
    a = np.arange(2 * 3 * 2 * 5, dtype=np.float32).reshape(2, 3, 2, 5)
    b = -a
    l2, r2 = R.lr_pairs(a, b)
    assert l2.shape == (4, 3, 2, 5) and np.array_equal(l2[:2], a) and np.array_equal(l2[2:, ..., 0], b[..., 4])
    assert np.array_equal(r2[:2], b) and np.array_equal(r2[2:], a[..., ::-1])


# ---- host-side argument checks of the C ABI (no GPU call is reached) ----
_P = ctypes.c_void_p(256)                                    # never dereferenced: every call below is refused first


def _arr(n=4, p=_P):
    return (ctypes.c_void_p * 4)(*([p] * n + [None] * (4 - n)))


def test_lr_check_rejects_bad_arguments(hip_lib):
    def call(dl=None, drm=None, nmaps=4, B=1, H=8, W=16, tau=1.0, fill=0, out=None, mask=None):
        return hip_lib.lws_lr_check(dl if dl is not None else _arr(), drm if drm is not None else _arr(), nmaps, B, H, W, tau, fill,
                                    out if out is not None else _arr(), mask if mask is not None else _arr(), _arr(0), None, None)

    cases = [
        (dict(dl=_arr(0)), b"null"),
        (dict(mask=_arr(3)), b"null"),
        (dict(nmaps=0), b"nmaps"), (dict(nmaps=5), b"nmaps"),
        (dict(B=0), b"shape"), (dict(H=0), b"shape"), (dict(W=-1), b"shape"),
        (dict(W=8193), b"8192"),
        (dict(tau=-0.5), b"tau"), (dict(tau=float("inf")), b"tau"), (dict(tau=float("nan")), b"tau"),
        (dict(fill=2), b"fill"),
    ]
    for kw, msg in cases:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert msg in hip_lib.lws_last_error(), (kw, hip_lib.lws_last_error())
    texts = [
        (dict(nmaps=5), b"lr_check: nmaps 5 outside 1..4"), (dict(B=0), b"lr_check: bad shape B=0 H=8 W=16"),
        (dict(B=65536), b"lr_check: bad shape B=65536 H=8 W=16"), (dict(W=-1), b"lr_check: bad shape B=1 H=8 W=-1"),
        (dict(W=8193), b"lr_check: W=8193 exceeds 8192 (the row is staged in LDS)"),
        (dict(tau=-0.5), b"lr_check: tau must be finite and >= 0, got -0.5"), (dict(tau=float("inf")), b"lr_check: tau must be finite and >= 0, got inf"),
        (dict(tau=float("nan")), b"lr_check: tau must be finite and >= 0, got nan"),
        (dict(fill=2), b"lr_check: fill 2 (0 = zero, 1 = background fill)"), (dict(mask=_arr(3)), b"lr_check: map 3 has a null pointer"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw
    null4 = _arr(0)
    assert hip_lib.lws_lr_check(null4, _arr(), 1, 1, 8, 16, 1.0, 0, _arr(), _arr(), null4, None, None) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_lr_check(_arr(), _arr(), 1, 1, 8, 16, 1.0, 0, null4, _arr(), null4, None, None) == _lib.LWS_ERR_INVALID


def test_lr_pairs_rejects_bad_arguments(hip_lib):
    assert hip_lib.lws_lr_pairs(None, _P, _P, _P, 1, 8, 16, None) == _lib.LWS_ERR_INVALID
    assert b"null" in hip_lib.lws_last_error()
    assert hip_lib.lws_lr_pairs(_P, _P, _P, None, 1, 8, 16, None) == _lib.LWS_ERR_INVALID
    for B, H, W in ((0, 8, 16), (1, 0, 16), (1, 8, 0), (-2, 8, 16)):
        assert hip_lib.lws_lr_pairs(_P, _P, _P, _P, B, H, W, None) == _lib.LWS_ERR_INVALID
        assert b"shape" in hip_lib.lws_last_error()


# ---- CLIs: the check is sequential only, refused before any model or GPU work ----
@pytest.mark.parametrize("module", ["inference", "evaluate"])
def test_cli_rejects_lr_check_with_workers(module, capsys):
    import importlib
    mod = importlib.import_module(f"lwsnet_amd.{module}")
    with pytest.raises(SystemExit) as e:
        mod.main(["--lr_check", "1", "--workers", "2", "--synthetic_weights"])
    assert e.value.code != 0
    assert "--lr_check runs in the sequential mode only" in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--lr_fill"], ["--lr_check", "-1"], ["--lr_check", "nan"]])
def test_cli_rejects_bad_lr_flags(argv, capsys):
    from lwsnet_amd import evaluate, inference
    for mod in (inference, evaluate):
        with pytest.raises(SystemExit) as e:
            mod.main(argv + ["--synthetic_weights"])
        assert e.value.code != 0
        assert "--lr_" in capsys.readouterr().err


def test_lr_flags_default_off():
    from lwsnet_amd import evaluate, inference
    for mod in (inference, evaluate):
        a = mod.build_parser().parse_args([])
        assert a.lr_check is None and a.lr_fill is False
