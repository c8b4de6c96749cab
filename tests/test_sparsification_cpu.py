"""The host side of the sparsification curves: metrics.spars_bin against an independent np.frexp formulation, the curves and AUSE
of metrics.sparsification_curves on histograms worked out by hand, the host-side argument errors of lws_sparsification, and what
evaluate() and the evaluation CLI refuse to combine with --sparsification."""
import ctypes

import numpy as np
import pytest

import sparsification_reference as REF
from lwsnet_amd import _lib
from lwsnet_amd import metrics as M


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


# ---- bins ----
def test_bins_at_the_edges():
    lo = np.float32(2.0 ** -24)
    vals = np.array([lo, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(1)), 255.99998, 256.0, 0.0, -0.0, -3.5,
                     np.inf, -np.inf, np.nan, 1.0, np.nextafter(np.float32(1), np.float32(0))], np.float32)
    want = [1, 0, 1, 1024, 1025, 0, 0, 0, 1025, 0, 1025, 1 + 24 * 32, 24 * 32]
    assert M.spars_bin(vals).tolist() == want
    assert REF.bin_frexp(vals).tolist() == want
    assert M.spars_bin(np.float32(255.99998)) == 1024 and np.float32(255.99998) == np.nextafter(np.float32(256), np.float32(0))
    assert M.spars_bin(vals.reshape(13, 1)).shape == (13, 1) and M.spars_bin(vals).dtype == np.int64


def test_bins_of_random_bit_patterns():
    bits = np.random.default_rng(5).integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32)
    v = _f32(bits)
    got = M.spars_bin(v)
    assert np.array_equal(got, REF.bin_frexp(v))
    assert np.array_equal(got, REF.bin_frexp_fast(v))
    assert got.min() == 0 and got.max() == 1025 and len(np.unique(got)) > 900        # the patterns reach the whole range


def test_bin_edges_are_the_lower_edges():
    edges = M.spars_bin_edges()
    assert edges.dtype == np.float64 and edges.shape == (1025,)
    assert edges[0] == 2.0 ** -24 and edges[-1] == 256.0 and np.all(np.diff(edges) > 0)
    e32 = edges.astype(np.float32)
    assert np.array_equal(e32.astype(np.float64), edges)                              # every edge is a float32
    assert np.array_equal(M.spars_bin(e32), np.arange(1, 1026))
    assert np.array_equal(M.spars_bin(np.nextafter(e32, np.float32(0))), np.arange(0, 1025))


# ---- curves ----
def _hist(unc_rows, oracle_rows):
    """{bin: (pixels, bad, q sum)} per ranking -> [2,1026,3] int64."""
    h = np.zeros((2, 1026, 3), np.int64)
    for r, rows in enumerate((unc_rows, oracle_rows)):
        for j, row in rows.items():
            h[r, j] = row
    return h


def test_hand_computed_case_3_bins_6_pixels():
    """Ranking: bins 0 / 5 / 1025 hold 3 / 2 / 1 pixels, 0 / 1 / 1 of them bad.  Points (removed fraction, error of the rest):
    (1/2, 0), (1/6, 1/5), (0, 1/3).  Oracle: 4 good pixels, then the 2 bad ones: (1/3, 0), (0, 1/3).  At f = 0, 1/4, 1/2 the ranking
    gives 1/3, 0.2 * (1 - (1/4 - 1/6) / (1/3)) = 0.15, 0 and the oracle 1/3, 1/3 * (1 - 3/4) = 1/12, 0 (flat beyond its last point)."""
    h = _hist({0: (3, 0, 3 * 512), 5: (2, 1, 2 * 2048), 1025: (1, 1, 8192)}, {0: (4, 0, 0), 1000: (2, 2, 0)})
    c = M.sparsification_curves(h, "kitti", fractions=[0.0, 0.25, 0.5])
    np.testing.assert_allclose(c["unc"], [1 / 3, 0.15, 0.0], rtol=1e-14, atol=1e-16)
    np.testing.assert_allclose(c["oracle"], [1 / 3, 1 / 12, 0.0], rtol=1e-14, atol=1e-16)
    assert c["all"] == 2 / 6
    np.testing.assert_allclose(c["ause"], (0.15 - 1 / 12) / 3, rtol=1e-13)
    np.testing.assert_allclose(c["ause_rel"], (0.15 - 1 / 12), rtol=1e-13)
    assert np.array_equal(c["fractions"], [0.0, 0.25, 0.5])
    np.testing.assert_allclose(c["ause"], REF.ause_loop(h, "kitti", [0.0, 0.25, 0.5]), rtol=1e-13)
    # the same pixels as EPE: the q sums are 1.5, 4 and 8 px, so the rest after 1/2 has mean 0.5 px and all six 13.5 / 6
    e = M.sparsification_curves(h, "epe", fractions=[0.0, 0.5])
    assert e["all"] == 13.5 / 6 and e["unc"].tolist() == [13.5 / 6, 0.5]


def test_a_ranking_equal_to_the_oracle_has_ause_exactly_zero():
    rng = np.random.default_rng(1)
    rows = np.zeros((1026, 3), np.int64)
    rows[:, 0] = rng.integers(0, 50, 1026) * (rng.random(1026) < 0.3)
    rows[:, 1] = (rows[:, 0] * np.linspace(0, 1, 1026)).astype(np.int64)
    rows[:, 2] = rows[:, 0] * np.arange(1026) * 37
    h = np.stack([rows, rows])
    for metric in ("kitti", "epe"):
        c = M.sparsification_curves(h, metric)
        assert c["ause"] == 0.0 and c["ause_rel"] == 0.0 and np.array_equal(c["unc"], c["oracle"])
        assert c["fractions"].shape == (100,) and c["fractions"][0] == 0 and c["fractions"][-1] == 0.99
        if metric == "epe":
            assert np.all(np.diff(c["oracle"]) <= 0)            # the error per pixel ascends with the bin: removing bins helps


def test_a_reversed_ranking_has_positive_ause():
    rows = np.zeros((1026, 3), np.int64)
    rows[100:200, 0] = 10
    rows[100:200, 1] = np.arange(100) // 10                     # the error grows with the bin
    rows[100:200, 2] = np.arange(100) * 1024
    rev = rows.copy()
    rev[100:200] = rows[100:200][::-1]                          # the most trusted bins hold the worst pixels
    for metric in ("kitti", "epe"):
        c = M.sparsification_curves(np.stack([rev, rows]), metric)
        assert c["ause"] > 0 and c["ause_rel"] > 0 and c["unc"][0] == c["oracle"][0] == c["all"]
        np.testing.assert_allclose(c["ause"], REF.ause_loop(np.stack([rev, rows]), metric), rtol=1e-12)


def test_no_valid_pixel_and_bad_arguments_raise():
    with pytest.raises(ValueError, match="no valid pixel"):
        M.sparsification_curves(np.zeros((2, 1026, 3), np.int64), "kitti")
    with pytest.raises(ValueError):
        M.sparsification_curves(np.ones((2, 1026, 3), np.int64), "rmse")
    with pytest.raises(ValueError):
        M.sparsification_curves(np.ones((2, 1025, 3), np.int64), "epe")
    with pytest.raises(ValueError):
        M.sparsification_curves(np.ones((2, 1026, 3), np.float64), "epe")
    h = _hist({3: (5, 0, 0)}, {0: (5, 0, 0)})                   # no error at all: `all` is 0, so there is no relative value
    c = M.sparsification_curves(h, "epe")
    assert c["all"] == 0.0 and c["ause"] == 0.0 and c["ause_rel"] is None


# ---- the C entry point's argument errors: host side, before any GPU call ----
_P = 0x10000                                                    # a non-null address that is never dereferenced


def _arr(n=4, p=_P):
    return (ctypes.c_void_p * 4)(*([p] * n + [None] * (4 - n)))


def test_sparsification_rejects_bad_arguments(hip_lib):
    hist = 0x40000000

    def call(pred=None, unc=None, nmaps=4, kind=0, B=1, Hp=8, W=16, off=0, gt=_P, Hg=8, maxdisp=192.0, mode=0, hist=hist):
        return hip_lib.lws_sparsification(pred if pred is not None else _arr(), unc if unc is not None else _arr(), nmaps, kind, B, Hp,
                                          W, off, gt, Hg, maxdisp, mode, hist, None)

    hist_bytes = 4 * 2 * 1026 * 3 * 8
    cases = [
        (dict(pred=_arr(3)), b"null"), (dict(unc=_arr(0)), b"null"), (dict(gt=None), b"null"), (dict(hist=None), b"null"),
        (dict(nmaps=0), b"nmaps"), (dict(nmaps=5), b"nmaps"),
        (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"), (dict(mode=2), b"mode"), (dict(mode=-1), b"mode"),
        (dict(off=-1, Hp=7), b"row_offset"), (dict(Hp=9), b"Hp"), (dict(off=2), b"Hp"),
        (dict(maxdisp=0.0), b"maxdisp"), (dict(maxdisp=-1.0), b"maxdisp"), (dict(maxdisp=float("nan")), b"maxdisp"),
        (dict(B=0), b"shape"), (dict(B=65536), b"shape"),
        (dict(gt=hist + hist_bytes - 4), b"overlap"), (dict(gt=hist - 8 * 16 * 4 + 4), b"overlap"),
        (dict(pred=_arr(4, hist + 64)), b"overlap"), (dict(unc=_arr(4, hist)), b"overlap"),
    ]
    for kw, msg in cases:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        err = hip_lib.lws_last_error()
        assert msg in err and b"sparsification" in err, (kw, err)
    # the checks shared with lws_stage_metrics and every pair of the written histogram with a buffer that is read: the whole text
    def one(s, p):
        a = _arr()
        a[s] = p
        return a

    texts = [
        (dict(B=0), b"sparsification: bad shape B=0 Hg=8 W=16"), (dict(B=65536), b"sparsification: bad shape B=65536 Hg=8 W=16"),
        (dict(Hg=0, Hp=0), b"sparsification: bad shape B=1 Hg=0 W=16"), (dict(W=-1), b"sparsification: bad shape B=1 Hg=8 W=-1"),
        (dict(off=-1, Hp=7), b"sparsification: row_offset -1 < 0"),
        (dict(Hp=9), b"sparsification: Hp=9 must be Hg + row_offset = 8 + 0"),
        (dict(off=2), b"sparsification: Hp=8 must be Hg + row_offset = 8 + 2"),
        (dict(mode=2), b"sparsification: mode 2 (0 = KITTI 3-px, 1 = EPE)"),
        (dict(maxdisp=0.0), b"sparsification: maxdisp must be > 0, got 0"),
        (dict(maxdisp=float("nan")), b"sparsification: maxdisp must be > 0, got nan"),
        (dict(Hg=1048577, Hp=1048577, W=1048576), b"sparsification: 1048577x1048576 is too large"),
        (dict(nmaps=5), b"sparsification: nmaps 5 outside 1..4"), (dict(kind=2), b"sparsification: kind 2 (0 = sigma, 1 = conf)"),
        (dict(gt=hist + 8), b"sparsification: hist and gt overlap"),
        (dict(pred=one(0, hist + 8)), b"sparsification: hist and pred[0] overlap"),
        (dict(pred=one(1, hist + 8)), b"sparsification: hist and pred[1] overlap"),
        (dict(pred=one(2, hist + 8)), b"sparsification: hist and pred[2] overlap"),
        (dict(pred=one(3, hist + 8)), b"sparsification: hist and pred[3] overlap"),
        (dict(unc=one(0, hist + 8)), b"sparsification: hist and unc[0] overlap"),
        (dict(unc=one(1, hist + 8)), b"sparsification: hist and unc[1] overlap"),
        (dict(unc=one(2, hist + 8)), b"sparsification: hist and unc[2] overlap"),
        (dict(unc=one(3, hist + 8)), b"sparsification: hist and unc[3] overlap"),
    ]
    for kw, msg in texts:
        assert call(**kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw
    # maps beyond nmaps are not looked at
    assert call(nmaps=2, pred=one(1, hist + 8)) == _lib.LWS_ERR_INVALID and hip_lib.lws_last_error() == b"sparsification: hist and pred[1] overlap"
    # pred, unc themselves NULL: through a second handle of the library, whose prototype takes the arrays as plain pointers
    _, args = _lib.PROTOTYPES["lws_sparsification"]
    fn = ctypes.CDLL(_lib.LIB_PATH).lws_sparsification
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p if a is ctypes.c_void_p * 4 else a for a in args]
    arrays = [_arr(), _arr()]
    for k in range(2):
        ptrs = [ctypes.addressof(a) for a in arrays]
        ptrs[k] = None
        assert fn(ptrs[0], ptrs[1], 4, 0, 1, 8, 16, 0, _P, 8, 192.0, 0, hist, None) == _lib.LWS_ERR_INVALID
        assert b"null" in hip_lib.lws_last_error()
    assert _lib.LWS_SPARS_BINS == M.SPARS_BINS == REF.BINS == 1026


# ---- evaluate() and the CLI ----
@pytest.mark.parametrize("kw,msg", [(dict(workers=2), "sequential mode only"), (dict(lr_check=1.0), "left-right check"),
                                    (dict(occ_check=1.0), "occlusion check"), (dict(speckle=100), "speckle filter"),
                                    (dict(wmedian=1), "weighted median filter")])
def test_evaluate_refuses_what_sparsification_does_not_combine_with(kw, msg):
    from lwsnet_amd import evaluate
    with pytest.raises(ValueError, match=msg):
        evaluate.evaluate(None, [None], "kitti", sparsification=True, **kw)


def test_host_accumulator_pools_integers_and_marks_empty_images():
    """evaluate.Sparsification: two batches, the second image of the first one without a valid pixel."""
    from lwsnet_amd.evaluate import Sparsification
    rng = np.random.default_rng(3)

    def image():
        rows = np.zeros((2, 1026, 3), np.int64)
        for r in range(2):
            bins = rng.choice(1026, 40, replace=False)
            rows[r, bins, 0] = 5
            rows[r, bins, 1] = rng.integers(0, 6, 40)
            rows[r, bins, 2] = rng.integers(0, 5000, 40)
        return rows

    batches = [np.stack([np.stack([image(), np.zeros((2, 1026, 3), np.int64)]) for _ in range(4)]),
               np.stack([np.stack([image()]) for _ in range(4)])]
    acc = Sparsification("kitti")
    for h in batches:
        acc.update({"conf": h, "sigma": h[::-1]})
    res = acc.result()
    assert sorted(res) == ["all", "conf", "fractions", "oracle", "per_image_ause", "sigma"]
    assert res["per_image_ause"]["conf"][1] == [None] * 4 and len(res["per_image_ause"]["sigma"]) == 3
    for s in range(4):
        pooled = batches[0][s].sum(axis=0) + batches[1][s].sum(axis=0)
        want = M.sparsification_curves(pooled, "kitti")
        assert res["conf"]["ause"][s] == want["ause"] and res["conf"]["curve"][s] == want["unc"].tolist()
        assert res["oracle"]["curve"][s] == want["oracle"].tolist() and res["all"][s] == want["all"]
        assert res["per_image_ause"]["conf"][0][s] == M.sparsification_curves(batches[0][s, 0], "kitti")["ause"]
        assert res["per_image_ause"]["sigma"][2][s] == res["per_image_ause"]["conf"][2][3 - s]
    lines = acc.lines(res)
    assert lines[0].startswith("Sparsification (conf): AUSE Stage 0=") and lines[1].startswith("Sparsification (sigma): AUSE Stage 0=")
    import json
    json.dumps(res)                                             # plain lists, floats and None


@pytest.mark.parametrize("argv,msg", [(["--workers", "2"], "--sparsification runs in the sequential mode only"),
                                      (["--lr_check", "1"], "does not combine with --lr_check"),
                                      (["--occ_check", "1"], "does not combine with --occ_check"),
                                      (["--speckle", "100"], "does not combine with --speckle"),
                                      (["--wmedian", "1"], "does not combine with --wmedian")])
def test_cli_rejects_bad_combinations_before_any_model_work(argv, msg, capsys):
    from lwsnet_amd import evaluate
    with pytest.raises(SystemExit) as e:
        evaluate.main(["--sparsification", "--synthetic_weights", *argv])
    assert e.value.code != 0
    assert msg in capsys.readouterr().err


@pytest.mark.parametrize("argv", [[], ["--workers", "2"], ["--lr_check", "1", "--lr_fill"], ["--dataset", "sceneflow", "--maxdisp", "100"]])
def test_a_command_line_without_the_flag_parses_as_before(argv):
    from lwsnet_amd import evaluate
    p = evaluate.build_parser()
    without = vars(p.parse_args(argv))
    assert "sparsification" not in without
    assert vars(p.parse_args(argv + ["--sparsification"])) == {**without, "sparsification": True}
    args = p.parse_args(argv)
    if not argv:
        evaluate.check_sparsification_argument(p, args)         # writes the default, like the occlusion flags' check
        assert args.sparsification is False and vars(args) == {**without, "sparsification": False}
