"""The one-forward occlusion check without a GPU: the numpy restatement (tests/occ_reference.py) against a per-pixel brute force
and on constructed rows, the host-side argument checks of lws_occlusion_check, the CLIs' flags, and the facts
postprocess.Options derives with the check on against a table written out by hand."""
import ctypes
import itertools
import math

import numpy as np
import pytest

import lr_reference as LR
import occ_reference as R
from lwsnet_amd import _lib
from lwsnet_amd.postprocess import Options

F = np.float32


def _row(vals):
    return np.asarray(vals, np.float32).reshape(1, 1, 1, -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the restatement against the contract, pixel by pixel in plain Python ----
def _less(a, b):
    """a < b in the order of the keys: the float order, with -0.0 below +0.0."""
    return a < b or (a == b and math.copysign(1.0, a) < math.copysign(1.0, b))


def brute_force(row, tau, fill):
    """One row (a list of float32 values) -> (out, code, right, kept) by the contract's words, no keys: Z holds floats or None."""
    W = len(row)
    Z = [None] * W
    t = [None] * W
    for x, d in enumerate(row):
        if math.isnan(d):
            continue
        tx = float(F(x) - F(d))
        if not (0.0 <= tx <= float(W - 1)):
            continue
        t[x] = tx
        lo, hi = math.floor(tx), math.ceil(tx)
        for j in ((lo,) if hi == lo else (lo, lo + 1)):
            if Z[j] is None or _less(Z[j], d):
                Z[j] = d
    code = []
    for x, d in enumerate(row):
        if math.isnan(d):
            code.append(0)
        elif t[x] is None:
            code.append(2)
        else:
            j = round(t[x])                                            # Python's round: half to even
            code.append(1 if F(Z[j]) - F(d) <= F(tau) else 0)
    out = []
    for x, d in enumerate(row):
        if code[x] == 1:
            out.append(d)
        elif not fill:
            out.append(0.0)
        else:
            left = next((row[i] for i in range(x - 1, -1, -1) if code[i] == 1), None)
            right = next((row[i] for i in range(x + 1, W) if code[i] == 1), None)
            both = [v for v in (left, right) if v is not None]
            out.append(0.0 if not both else (right if len(both) == 2 and right < left else both[0]))
    return out, code, [0.0 if z is None else z for z in Z], sum(c == 1 for c in code)


@pytest.mark.parametrize("W", [1, 2, 5, 33, 96])
def test_restatement_equals_the_brute_force(W):
    rng = np.random.default_rng(W)
    rows = []
    for kind in range(6):
        d = rng.uniform(-3.0, W + 3.0, W)
        if kind == 1:
            d = np.round(d)                                             # integer targets: one tap
        if kind == 2:
            d = np.round(d * 2) / 2                                     # targets at k + 0.5
        if kind == 3:
            d = np.cumsum(rng.uniform(-0.2, 1.2, W))                    # a slanted surface with folds
        d = d.astype(np.float32)
        if kind >= 4:
            for v in (np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30):
                d[rng.integers(W)] = v
        rows.append(d)
    dl = np.stack(rows).reshape(2, 1, 3, W)
    for tau in (0.0, 0.5, 1.0):
        for fill in (0, 1):
            out, code, right, kept = R.occlusion_check(dl, tau, fill)
            for i, d in enumerate(rows):
                b, y = divmod(i, 3)
                wo, wc, wr, wk = brute_force([float(v) for v in d], tau, fill)
                what = f"W={W} row {i} tau={tau} fill={fill}"
                assert code[b, 0, y].tolist() == wc, what
                assert np.array_equal(_bits(out[b, 0, y]), _bits(wo)), what
                assert np.array_equal(_bits(right[b, 0, y]), _bits(wr)), what
                assert kept[b, y] == wk, what


def test_key_is_order_preserving_and_never_empty():
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.standard_normal(200) * 50, [-np.inf, -3.0, -2.0, -1e-45, -0.0, 0.0, 1e-45, 2.0, 1e30, np.inf]]).astype(np.float32)
    k = R.key(v)
    assert np.all(k != 0) and np.array_equal(_bits(R.unkey(k)), _bits(v))
    order = np.argsort(k, kind="stable")
    assert np.all(np.diff(v[order].astype(np.float64)) >= 0), "unsigned order of the keys is the float order"
    assert R.key(F(-0.0)) < R.key(F(0.0)) and R.key(F(-2.0)) < R.key(F(-1.0)) < R.key(F(-0.0))
    assert R.key(np.uint32(0xffffffff).view(np.float32)) == 0, "the one word that keys to 0 is a NaN, and NaNs are never keyed"


def test_constant_disparity_is_out_of_view_left_of_d0():
    W, d0 = 64, 7
    dl = _row(np.full(W, d0))
    out, code, right, kept = R.occlusion_check(dl, 1.0, fill=False)
    x = np.arange(W)
    assert np.array_equal(code[0, 0, 0], np.where(x < d0, 2, 1))
    assert np.array_equal(out[0, 0, 0], np.where(x < d0, 0, d0).astype(np.float32))
    assert np.array_equal(right[0, 0, 0], np.where(x < W - d0, d0, 0).astype(np.float32))
    assert kept.tolist() == [[W - d0]]
    out, _, _, _ = R.occlusion_check(dl, 1.0, fill=True)
    assert np.all(out == d0)


@pytest.mark.parametrize("db,df", [(10, 40), (0, 3), (5, 7)])
def test_plateau_gives_the_occluded_band_and_agrees_with_the_left_right_check(db, df):
    """An ideal integer scene: the band of width df - db immediately left of the plateau is occluded, and the codes are those of
    the left-right check given the scene's true right-view map.  `right` is that true map wherever a left pixel landed; its holes
    are exactly what the left camera does not see: the band the plateau uncovers and the df / db columns past the right edge."""
    W, x0, x1 = 200, 100, 150
    d = np.full(W, db, np.float32)
    d[x0:x1] = df
    true_right = np.full(W, db, np.float32)                             # the right camera: the plateau stands df columns further left
    true_right[x0 - df:x1 - df] = df
    out, code, right, kept = R.occlusion_check(_row(d), 1.0, fill=False)
    wo, wc, wr, wk = LR.lr_check(_row(d), _row(true_right[::-1]), 1.0, fill=False)
    assert np.array_equal(code, wc) and np.array_equal(out, wo) and np.array_equal(kept, wk)
    c = code[0, 0, 0]
    assert np.all(c[:db] == 2) and np.all(c[db:x0 - (df - db)] == 1)
    assert np.all(c[x0 - (df - db):x0] == 0) and np.all(c[x0:] == 1)
    r = right[0, 0, 0]
    x = np.arange(W)
    hole = ((x >= x1 - df) & (x < x1 - db)) | (x >= W - db)
    assert np.array_equal(r == 0, hole | (wr[0, 0, 0] == 0))
    assert np.array_equal(r[~hole], wr[0, 0, 0][~hole])
    filled, _, _, _ = R.occlusion_check(_row(d), 1.0, fill=True)
    f = filled[0, 0, 0]
    assert np.all(f[x0 - (df - db):x0] == db) and np.all(f[x0:x1] == df) and np.all(f[:x0] == db)
    assert np.array_equal(filled, LR.lr_check(_row(d), _row(true_right[::-1]), 1.0, fill=True)[0])


def test_difference_equal_to_tau_is_visible():
    d = np.full(16, np.nan, np.float32)
    d[10], d[11] = 5.0, 5.5                                             # t = 5 and 5.5: both touch column 5, z - d = 0.5 at x = 10
    assert R.occlusion_check(_row(d), 0.5, False)[1][0, 0, 0, 10:12].tolist() == [1, 1]
    assert R.occlusion_check(_row(d), np.nextafter(F(0.5), F(0)), False)[1][0, 0, 0, 10:12].tolist() == [0, 1]


def test_nan_is_code_0_and_inf_out_of_view():
    W = 16
    d = np.full(W, 2.0, np.float32)
    d[4], d[6], d[8], d[9] = np.nan, np.inf, -np.inf, 1e30
    out, code, right, kept = R.occlusion_check(_row(d), 1.0, fill=True)
    c = code[0, 0, 0]
    assert c[4] == 0 and c[6] == 2 and c[8] == 2 and c[9] == 2 and np.all(c[:2] == 2)
    assert np.all(np.isfinite(out)) and np.all(np.isfinite(right))
    assert kept[0, 0] == W - 2 - 4
    assert right[0, 0, 0].tolist() == [2, 2, 0, 2, 0, 2, 0, 0, 2, 2, 2, 2, 2, 2, 0, 0]


def test_negative_disparities_and_minus_zero_are_ordered_by_the_key():
    d = np.full(8, np.nan, np.float32)
    d[3], d[4], d[5] = -2.0, -1.0, -0.0                                 # all three land on column 5
    out, code, right, _ = R.occlusion_check(_row(d), 1.0, False)
    assert _bits(right[0, 0, 0, 5]) == 0x80000000, "-0.0 is the nearest of the three, and is no hole"
    assert code[0, 0, 0, 3:6].tolist() == [0, 1, 1]
    d[2] = 0.0                                                          # +0.0 above -0.0 on column 2 ...
    d[1] = -1.0
    assert _bits(R.occlusion_check(_row(d), 1.0, False)[2][0, 0, 0, 2]) == 0
    d[2], d[1] = -0.0, np.nan                                           # ... and a lone -0.0 there is not a hole
    assert _bits(R.occlusion_check(_row(d), 1.0, False)[2][0, 0, 0, 2]) == 0x80000000


@pytest.mark.parametrize("x,cols", [(11, (5, 6)), (12, (6, 7))])
def test_half_way_target_tests_the_even_column_and_finds_it_splatted(x, cols):
    d = np.full(16, np.nan, np.float32)
    d[x] = 5.5                                                          # t = 5.5 / 6.5: rint gives 6 both times (the ceil / the floor)
    _, code, right, _ = R.occlusion_check(_row(d), 0.0, False)
    assert code[0, 0, 0, x] == 1
    assert np.flatnonzero(right[0, 0, 0]).tolist() == list(cols) and 6 in cols


def test_a_row_without_a_visible_pixel_fills_to_zero():
    for vals in ([np.nan] * 9, [1e30] * 9, [np.nan, 100.0, -np.inf, np.inf, -50.0]):
        out, code, right, kept = R.occlusion_check(_row(vals), 1.0, fill=True)
        assert not np.any(code == 1) and kept.tolist() == [[0]]
        assert not _bits(out).any() and not _bits(right).any()


# ---- host-side argument checks of the C ABI (no GPU call is reached) ----
_P = ctypes.c_void_p(256)                                    # never dereferenced: every call below is refused first


def _arr(n=4, p=_P):
    return (ctypes.c_void_p * 4)(*([p] * n + [None] * (4 - n)))


def test_occlusion_check_rejects_bad_arguments(hip_lib):
    def call(dl=None, nmaps=4, B=1, H=8, W=16, tau=1.0, fill=0, out=None, mask=None):
        return hip_lib.lws_occlusion_check(dl if dl is not None else _arr(), nmaps, B, H, W, tau, fill,
                                           out if out is not None else _arr(), mask if mask is not None else _arr(), _arr(0), None, None)

    cases = [
        (dict(dl=_arr(0)), b"null"), (dict(out=_arr(2)), b"null"), (dict(mask=_arr(3)), b"null"),
        (dict(nmaps=0), b"nmaps"), (dict(nmaps=5), b"nmaps"),
        (dict(B=0), b"shape"), (dict(H=0), b"shape"), (dict(W=0), b"shape"), (dict(W=-1), b"shape"),
        (dict(W=8193), b"8192"),
        (dict(tau=-0.5), b"tau"), (dict(tau=float("inf")), b"tau"), (dict(tau=float("nan")), b"tau"),
        (dict(fill=2), b"fill"),
    ]
    for kw, msg in cases:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        err = hip_lib.lws_last_error()
        assert msg in err and b"occlusion_check" in err, (kw, err)
    texts = [
        (dict(nmaps=5), b"occlusion_check: nmaps 5 outside 1..4"), (dict(B=0), b"occlusion_check: bad shape B=0 H=8 W=16"),
        (dict(B=65536), b"occlusion_check: bad shape B=65536 H=8 W=16"), (dict(W=-1), b"occlusion_check: bad shape B=1 H=8 W=-1"),
        (dict(tau=-0.5), b"occlusion_check: tau must be finite and >= 0, got -0.5"),
        (dict(tau=float("inf")), b"occlusion_check: tau must be finite and >= 0, got inf"),
        (dict(tau=float("nan")), b"occlusion_check: tau must be finite and >= 0, got nan"),
        (dict(fill=2), b"occlusion_check: fill 2 (0 = zero, 1 = background fill)"), (dict(out=_arr(2)), b"occlusion_check: map 2 has a null pointer"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw
    # dL, out, mask themselves NULL: through a second handle of the library, whose prototype takes the arrays as plain pointers
    _, args = _lib.PROTOTYPES["lws_occlusion_check"]
    fn = ctypes.CDLL(_lib.LIB_PATH).lws_occlusion_check
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p if a is ctypes.c_void_p * 4 else a for a in args]
    arrays = [_arr(), _arr(), _arr()]
    for k in range(3):
        ptrs = [ctypes.addressof(a) for a in arrays]
        ptrs[k] = None
        assert fn(ptrs[0], 1, 1, 8, 16, 1.0, 0, ptrs[1], ptrs[2], None, None, None) == _lib.LWS_ERR_INVALID
        assert b"null" in hip_lib.lws_last_error()


# ---- CLIs ----
@pytest.mark.parametrize("module", ["inference", "evaluate"])
@pytest.mark.parametrize("argv,msg", [(["--occ_fill"], "--occ_fill needs --occ_check"),
                                      (["--occ_check", "1", "--lr_check", "1"], "--occ_check and --lr_check are alternatives"),
                                      (["--occ_check", "1", "--workers", "2"], "--occ_check runs in the sequential mode only"),
                                      (["--occ_check", "-1"], "--occ_check TAU must be finite"),
                                      (["--occ_check", "nan"], "--occ_check TAU must be finite")])
def test_cli_rejects_bad_occ_flags(module, argv, msg, capsys):
    import importlib
    mod = importlib.import_module(f"lwsnet_amd.{module}")
    with pytest.raises(SystemExit) as e:
        mod.main(argv + ["--synthetic_weights"])
    assert e.value.code != 0
    assert msg in capsys.readouterr().err


def test_occ_flags_default_off():
    from lwsnet_amd import evaluate, inference
    for mod in (inference, evaluate):
        p = mod.build_parser()
        a = p.parse_args([])
        assert Options.from_args(a) == Options()
        mod.post.check_occ_arguments(p, a)
        assert a.occ_check is None and a.occ_fill is False
        assert Options.from_args(a) == Options()
        a = p.parse_args(["--occ_check", "0.5", "--occ_fill"])
        mod.post.check_occ_arguments(p, a)
        assert a.occ_check == 0.5 and a.occ_fill is True
        assert Options.from_args(a) == Options(occ_check=0.5, occ_fill=True)
    assert Options().occ_check is None and Options().occ_fill is False and Options().has_codes is False


def test_options_refuse_both_checks_and_bad_tau():
    for bad in (dict(occ_check=1.0, lr_check=1.0), dict(occ_check=-1.0), dict(occ_check=float("nan")), dict(occ_check=float("inf"))):
        with pytest.raises(ValueError, match="occ_check"):
            Options.make(**bad).check()
    Options.make(occ_check=0.0, occ_fill=True, speckle=10, wmedian=1).check()


def test_evaluate_refuses_the_check_with_workers():
    from lwsnet_amd import evaluate
    with pytest.raises(ValueError, match="occlusion check runs in the sequential mode only"):
        evaluate.evaluate(None, [None], "kitti", workers=2, occ_check=1.0)


# ---- the facts of the chain with the occlusion check on ----
FACTS = ("forward_fills", "speckle_fills", "row_filled", "filled", "needs_guide", "wmedian_takes_codes", "geometry_takes_codes",
         "has_codes")

# (occlusion check, speckle filter, weighted median at sigma 10) -> FACTS in their order, T = true.  "fill": --occ_fill /
# --speckle_fill; "fill0" / "fill4": --wmedian_fill 0 / 4.  By hand, the occlusion check standing where the left-right check
# stands: the check fills its own maps only without a speckle filter behind it; the speckle filter fills for either row-fill
# flag; the guide goes with the median; the median takes the codes while no row was filled; the geometry files take them when, in
# addition, the median filled no hole; there are codes in every row.
TABLE = {
    ('on',   'off',  'off'):   "......TT",
    ('on',   'off',  'fill0'): "....TTTT",
    ('on',   'off',  'fill4'): "...TTT.T",
    ('on',   'on',   'off'):   "......TT",
    ('on',   'on',   'fill0'): "....TTTT",
    ('on',   'on',   'fill4'): "...TTT.T",
    ('on',   'fill', 'off'):   ".TTT...T",
    ('on',   'fill', 'fill0'): ".TTTT..T",
    ('on',   'fill', 'fill4'): ".TTTT..T",
    ('fill', 'off',  'off'):   "T.TT...T",
    ('fill', 'off',  'fill0'): "T.TTT..T",
    ('fill', 'off',  'fill4'): "T.TTT..T",
    ('fill', 'on',   'off'):   ".TTT...T",
    ('fill', 'on',   'fill0'): ".TTTT..T",
    ('fill', 'on',   'fill4'): ".TTTT..T",
    ('fill', 'fill', 'off'):   ".TTT...T",
    ('fill', 'fill', 'fill0'): ".TTTT..T",
    ('fill', 'fill', 'fill4'): ".TTTT..T",
}


def test_the_table_has_every_combination():
    assert set(TABLE) == set(itertools.product(("on", "fill"), ("off", "on", "fill"), ("off", "fill0", "fill4")))


@pytest.mark.parametrize("key", list(TABLE), ids=lambda k: "-".join(k))
def test_derived_facts_with_the_occlusion_check(key):
    occ, sp, wm = key
    options = Options.make(occ_check=1.0, occ_fill=occ == "fill", speckle=None if sp == "off" else 60, speckle_fill=sp == "fill",
                           wmedian=None if wm == "off" else 2, wmedian_sigma=10.0, wmedian_fill=4 if wm == "fill4" else 0)
    options.check()
    got = {name: getattr(options, name) for name in FACTS}
    assert all(type(v) is bool for v in got.values()), got
    assert got == {name: c == "T" for name, c in zip(FACTS, TABLE[key])}
    want_stages = ["occlusion check"] + ["speckle filter"] * (sp != "off") + ["weighted median filter"] * (wm != "off")
    assert options.stages_on == want_stages
    # the same switches on the left-right check give the same facts: the occlusion check stands exactly where it stands
    lr = Options.make(lr_check=1.0, lr_fill=occ == "fill", speckle=options.speckle, speckle_fill=options.speckle_fill,
                      wmedian=options.wmedian, wmedian_sigma=10.0, wmedian_fill=options.wmedian_fill)
    assert {name: getattr(lr, name) for name in FACTS} == got
