"""The confidence contract without a GPU: tests/confidence_reference.py against the C oracle's soft-argmin and against a float64
evaluation of the same formulas, its exact cases, ops.confidence_codes' truth table on CPU tensors, the C ABI's argument
checks and the inference CLI's flag-exclusion errors."""
import ctypes

import numpy as np
import pytest

import confidence_reference as CR
from conftest import golden

F = np.float32


def seeded_cost(seed, shape, scale=12.0):
    return (np.random.default_rng(seed).random(shape) * scale).astype(F)


# (cost, start): the committed soft-argmin fixtures, a seeded D = 7 case (the kernel's generic path) and D = 32
def cases():
    out = []
    for name in ("softargmin_d9.npz", "softargmin_d24.npz"):
        g = golden(name)
        out.append((name, g["cost"], float(g["start"]), g["low"]))
    out.append(("seeded D=7", seeded_cost(71, (2, 7, 6, 9)), -3.0, None))
    out.append(("seeded D=32", seeded_cost(72, (1, 32, 5, 11), 3.0), 0.0, None))       # a flatter volume: many hypotheses carry mass
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_reference_disparity_is_the_oracles_softargmin():
    from oracle import c_oracle as C
    for name, cost, start, low in cases():
        d, _, _ = CR.low_maps(cost, start)
        assert np.array_equal(bits(d), bits(C.softargmin(cost, start))), name
        if low is not None:                     # (the fixture's own map is the literal restatement's: float32 noise apart)
            assert float(np.abs(d - low).max()) < 1e-5, name


def test_one_hot_volume_is_certain():
    """One cost 0, the others 1e4: every other e_k is exactly 0, so p = 1 on that hypothesis, d = v_k, peak = 1 and sig = 0."""
    for D, start, k in ((9, -4.0, 0), (24, 0.0, 17), (7, -3.0, 6)):
        cost = np.full((1, D, 2, 3), 1e4, F)
        cost[:, k] = 0.0
        d, peak, sig = CR.low_maps(cost, start)
        assert np.all(d == F(start) + F(k)) and np.all(peak == F(1.0)) and np.all(bits(sig) == 0)


def test_flat_volume_spreads_over_the_range():
    """All costs equal (odd D): e_k = 1, p_k = fl(1 / D), d at the centre, and the window holds the three hypotheses around it."""
    for D, start in ((9, -4.0), (7, -3.0), (33, 0.0)):
        cost = np.full((2, D, 3, 2), 2.5, F)
        d, peak, sig = CR.low_maps(cost, start)
        centre = F(start) + F((D - 1) // 2)
        assert np.all(np.abs(d - centre) < 1e-5)
        p = F(1.0) / F(D)                       # S = D exactly (a small integer)
        assert np.all(peak == (F(0.0) + p) + p + p)
        assert np.allclose(sig, np.sqrt((D * D - 1) / 12.0), rtol=1e-5)


def test_reference_against_float64():
    """peak and sig against the float64 evaluation.  Measured on these inputs (CPU, the oracle's expf against numpy's exp): the
    largest distance is 2.83e-07 for peak and 1.24e-06 for sig (sig reaches 9 hypothesis steps on the flatter D = 32 volume, so
    that is about one ulp of it).  The gate is four times the measured value: float32 summation of <= 32 non-negative terms
    accumulates a few ulp of the result, and the polynomial expf is within an ulp of exp."""
    worst_peak = worst_sig = 0.0
    for name, cost, start, _ in cases():
        d, peak, sig = CR.low_maps(cost, start)
        peak64, sig64 = CR.low_maps_f64(cost, start, d)
        worst_peak = max(worst_peak, float(np.abs(peak - peak64).max()))
        worst_sig = max(worst_sig, float(np.abs(sig - sig64).max()))
    print(f"max |peak - peak64| = {worst_peak:.3e}, max |sig - sig64| = {worst_sig:.3e}")
    assert worst_peak <= 4 * 2.83e-07 and worst_sig <= 4 * 1.24e-06


def test_full_maps_are_the_oracles_resizes():
    from oracle import c_oracle as C
    cost = seeded_cost(5, (2, 9, 5, 11))
    r = CR.softargmin_conf(cost, -4.0, 40, 88)
    assert r["conf"].shape == r["sigma"].shape == (2, 1, 40, 88)
    assert np.array_equal(bits(r["conf"][:, 0]), bits(C.resize_bilinear(r["peak_low"], 40, 88)))
    scaled = (r["sigma_low"] * F(40)) * (F(1.0) / F(5))
    assert np.array_equal(bits(r["sigma"][:, 0]), bits(C.resize_bilinear(scaled, 40, 88)))
    assert float(r["conf"].min()) >= 0.0 and float(r["conf"].max()) <= 1.0 + 1e-6


def test_confidence_codes_truth_table():
    torch = pytest.importorskip("torch")
    from lwsnet_amd import ops

    def maps(vals):
        return [torch.tensor(v, dtype=torch.float32).view(1, 1, 1, -1) for v in vals]

    #            pixel:  0     1     2     3     4
    conf = maps([[0.9, 0.9, 0.2, 0.9, float("nan")], [0.9, 0.4, 0.9, 0.9, 0.9], [0.9, 0.9, 0.9, 0.5, 0.9]])
    sigma = maps([[0.5, 3.0, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5, 0.5], [0.5, 0.5, 0.5, 2.0, 0.5]])

    def codes(**kw):
        c = ops.confidence_codes(conf, sigma, **kw)
        assert c.dtype == torch.uint8 and tuple(c.shape) == (1, 1, 1, 5)
        return c.view(-1).tolist()

    assert codes() == [1, 1, 1, 1, 1]                                        # no threshold: everything passes
    assert codes(min_conf=0.5) == [1, 0, 0, 1, 0]                            # every stage must pass; NaN fails; 0.5 >= 0.5 passes
    assert codes(max_sigma=2.0) == [1, 0, 1, 1, 1]                           # 2.0 <= 2.0 passes
    assert codes(min_conf=0.5, max_sigma=1.0) == [1, 0, 0, 0, 0]
    assert codes(min_conf=0.5, stages=(2,)) == [1, 1, 1, 1, 1]
    assert codes(min_conf=0.6, stages=(2,)) == [1, 1, 1, 0, 1]
    assert codes(min_conf=0.5, max_sigma=1.0, stages=(0, 1)) == [1, 0, 0, 1, 0]
    assert ops.confidence_codes(None, sigma, max_sigma=1.0).view(-1).tolist() == [1, 0, 1, 0, 1]
    for bad in ((), (3,), (-1, 0)):
        with pytest.raises(ValueError):
            ops.confidence_codes(conf, sigma, min_conf=0.5, stages=bad)
    with pytest.raises(ValueError):
        ops.confidence_codes(None, sigma, min_conf=0.5)
    with pytest.raises(ValueError):
        ops.confidence_codes(None, None)


def test_abi_validates_arguments_on_the_host(hip_lib):
    """lws_softargmin_conf and lws_forward_conf refuse bad arguments before any HIP work (no GPU needed)."""
    from lwsnet_amd import _lib
    z = np.zeros(64, F)
    p = ctypes.c_void_p(z.ctypes.data)
    call = hip_lib.lws_softargmin_conf
    assert call(None, 1, 9, 2, 2, 0.0, 4, 4, p, p, p, p, p, None) == _lib.LWS_ERR_INVALID
    assert call(p, 1, 9, 2, 2, 0.0, 4, 4, None, None, None, None, None, None) == _lib.LWS_ERR_INVALID
    assert b"every output is null" in hip_lib.lws_last_error()
    assert call(p, 0, 9, 2, 2, 0.0, 4, 4, p, p, p, p, p, None) == _lib.LWS_ERR_INVALID
    assert call(p, 1, 9, 2, 2, 0.0, 1, 4, p, p, p, p, p, None) == _lib.LWS_ERR_INVALID          # H < h
    assert call(p, 1, 9, 1, 1, 0.0, 2000, 4, p, p, p, p, p, None) == _lib.LWS_ERR_INVALID       # factor above 1024
    assert b"upsampling factor" in hip_lib.lws_last_error()
    outs = (ctypes.c_void_p * 4)(*[z.ctypes.data] * 4)
    three = (ctypes.c_void_p * 3)()
    assert hip_lib.lws_forward_conf(None, p, p, 1, 64, 256, outs, three, three, None) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_kernel_class_name(_lib.LWS_KC_COUNT - 1) == b"softargmin_conf"


@pytest.mark.parametrize("extra,msg", [
    (["--save_conf", "--lr_check", "1"], "do not combine with --lr_check or --occ_check"),
    (["--conf_min", "0.5", "--save_disp16", "--occ_check", "1"], "do not combine with --lr_check or --occ_check"),
    (["--sigma_max_keep", "2", "--save_disp16", "--lr_check", "1"], "do not combine with --lr_check or --occ_check"),
    (["--save_conf", "--workers", "2"], "sequential mode only"),
    (["--conf_min", "0.5"], "give one of them"),
    (["--sigma_max", "4"], "--sigma_max needs --save_conf"),
    (["--save_conf", "--sigma_max", "0"], "--sigma_max MAX must be finite and > 0"),
])
def test_cli_refuses_flag_combinations(extra, msg, capsys):
    """Before any model or GPU work: a clear SystemExit with the reason on stderr."""
    from lwsnet_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main(["--left_img", "nowhere/left_test.png", "--synthetic_weights", *extra])
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_cli_png_encodings():
    from lwsnet_amd import inference
    conf = np.array([[-0.1, 0.0, 0.5, 0.998, 1.0, 1.2]], F)
    assert inference.conf_to_u8(conf).tolist() == [[0, 0, 128, 254, 255, 255]]             # rint: 127.5 -> 128 (half to even)
    sigma = np.array([[0.0, 1.0, 4.0, 8.0, 9.0, 0.1]], F)
    assert inference.sigma_to_u8(sigma, 8.0).tolist() == [[0, 32, 128, 255, 255, 3]]
    assert inference.conf_to_u8(conf).dtype == np.uint8


CONF_FLAGS = "--save_conf / --conf_min / --sigma_max_keep"
OUTPUT_FLAGS = "--save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh"


@pytest.mark.parametrize("extra,text", [
    (["--sigma_max", "4"], "--sigma_max needs --save_conf"),
    (["--save_conf", "--sigma_max", "0"], "--sigma_max MAX must be finite and > 0, got 0.0"),
    (["--save_conf", "--sigma_max", "inf"], "--sigma_max MAX must be finite and > 0, got inf"),
    (["--conf_min", "nan"], "--conf_min must be a number, got nan"),
    (["--sigma_max_keep", "nan"], "--sigma_max_keep must be a number, got nan"),
    (["--save_conf", "--occ_check", "1"], CONF_FLAGS + " use the network's own confidence and do not combine with --lr_check or --occ_check"),
    (["--save_conf", "--workers", "2"], CONF_FLAGS + " run in the sequential mode only: use --workers 0"),
    (["--conf_min", "0.5"], "--conf_min and --sigma_max_keep mask " + OUTPUT_FLAGS + ": give one of them"),
    # two apply: the earlier check wins
    (["--sigma_max", "0", "--conf_min", "nan"], "--sigma_max needs --save_conf"),
    (["--save_conf", "--sigma_max", "0", "--conf_min", "nan"], "--sigma_max MAX must be finite and > 0, got 0.0"),
    (["--conf_min", "nan", "--lr_check", "1"], "--conf_min must be a number, got nan"),
    (["--conf_min", "0.5", "--lr_check", "1", "--workers", "2"], "--lr_check runs in the sequential mode only: use --workers 0"),
    (["--sigma_max_keep", "2", "--workers", "2"], CONF_FLAGS + " run in the sequential mode only: use --workers 0"),
])
def test_cli_conf_error_texts(extra, text, capsys):
    from lwsnet_amd import inference
    with pytest.raises(SystemExit) as e:
        inference.main(["--left_img", "nowhere/left_test.png", "--synthetic_weights", *extra])
    assert e.value.code == 2
    assert capsys.readouterr().err.endswith(": error: " + text + "\n")
