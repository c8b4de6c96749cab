"""The speckle filter without a GPU: the union-find restatement (tests/speckle_reference.py) against an independent flood fill and
against hand-written cases, the argument errors of lws_speckle_filter / lws_speckle_workspace through the C ABI, the CLI flags,
and the properties the GPU tests ask of their inputs."""
import ctypes
from collections import deque

import numpy as np
import pytest

import speckle_inputs as I
import speckle_reference as R
from lwsnet_amd import _lib


def flood_fill(d, mask, max_diff):
    """Breadth-first flood fill in raster order, written without the reference's helpers: labels [H,W] int32 (first pixel of the
    component in raster order, -1 invalid) and the size of each pixel's component."""
    H, W = d.shape
    md = np.float32(max_diff)
    lab = np.full((H, W), -1, np.int32)
    size = np.zeros((H, W), np.int64)

    def ok(y, x):
        v = d[y, x]
        return bool(np.isfinite(v)) and v > 0 and (mask is None or mask[y, x] == 1)

    for y0 in range(H):
        for x0 in range(W):
            if lab[y0, x0] >= 0 or not ok(y0, x0):
                continue
            lab[y0, x0] = y0 * W + x0
            todo, members = deque([(y0, x0)]), [(y0, x0)]
            while todo:
                y, x = todo.popleft()
                for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                    if 0 <= ny < H and 0 <= nx < W and lab[ny, nx] < 0 and ok(ny, nx):
                        with np.errstate(invalid="ignore", over="ignore"):
                            joined = np.abs(np.float32(d[y, x] - d[ny, nx])) <= md
                        if joined:
                            lab[ny, nx] = y0 * W + x0
                            todo.append((ny, nx))
                            members.append((ny, nx))
            for y, x in members:
                size[y, x] = len(members)
    return lab, size


@pytest.mark.parametrize("seed", range(20))
def test_union_find_equals_flood_fill(seed):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 49)), int(rng.integers(1, 65))
    kind = I.KINDS[seed % len(I.KINDS)] if seed % 2 else "plateaus"
    d = I.make(kind, 1, H, W, seed)[0, 0]
    if seed % 3 == 0:                                       # coarse levels: components of many sizes at max_diff 0 .. 1
        d = np.round(rng.uniform(1, 4, (H, W))).astype(np.float32) * np.float32(0.75)
    d = I.plant_specials(d.copy(), rng)
    mask = I.random_mask(1, H, W, seed + 100)[0, 0] if seed % 4 != 1 else None
    for max_diff in (0.0, 0.5, 1.0):
        valid, lab, size = R.label_image(d, mask, max_diff)
        want_lab, want_size = flood_fill(d, mask, max_diff)
        assert np.array_equal(lab, want_lab), (seed, max_diff)
        assert np.array_equal(size, want_size), (seed, max_diff)
        assert np.array_equal(valid, want_lab >= 0)


def _filter(rows, max_size, max_diff=1.0, mask=None, fill=0):
    d = np.array(rows, np.float32)[None, None]
    m = None if mask is None else np.array(mask, np.uint8)[None, None]
    out, code, lab, counts = R.speckle_filter(d, m, max_diff, max_size, fill)
    return out[0, 0], code[0, 0], lab[0, 0], counts[0]


def test_size_threshold_is_inclusive():
    rows = [[5, 5, 5, 0, 9, 9, 9, 9]]                       # a component of 3 pixels and one of 4
    out, code, lab, counts = _filter(rows, 3)
    assert code.tolist() == [[3, 3, 3, 0, 1, 1, 1, 1]]      # exactly max_size: removed; max_size + 1: kept
    assert out.tolist() == [[0, 0, 0, 0, 9, 9, 9, 9]]
    assert lab.tolist() == [[0, 0, 0, -1, 4, 4, 4, 4]]      # a speckle keeps its label
    assert counts.tolist() == [7, 4, 1]
    assert _filter(rows, 2)[1].tolist() == [[1, 1, 1, 0, 1, 1, 1, 1]]
    assert _filter(rows, 4)[1].tolist() == [[3, 3, 3, 0, 3, 3, 3, 3]]


def test_diagonal_neighbours_are_not_joined():
    out, code, lab, counts = _filter([[5, 0], [0, 5]], 1)
    assert lab.tolist() == [[0, -1], [-1, 3]] and code.tolist() == [[3, 0], [0, 3]] and counts.tolist() == [2, 0, 2]


def test_joining_is_transitive():
    out, code, lab, counts = _filter([[10.0, 10.75, 11.5]], 2)       # a-b and b-c within 1, a-c not: one component of 3
    assert lab.tolist() == [[0, 0, 0]] and code.tolist() == [[1, 1, 1]] and counts.tolist() == [3, 3, 0]
    out, code, lab, counts = _filter([[10.0, 10.75, 11.5]], 2, max_diff=0.5)
    assert lab.tolist() == [[0, 1, 2]] and code.tolist() == [[3, 3, 3]] and counts.tolist() == [3, 0, 3]


def test_max_size_zero_removes_nothing():
    rows = [[5, 0, 7, 7], [np.nan, 3, 0, -1]]
    out, code, lab, counts = _filter(rows, 0)
    assert code.tolist() == [[1, 0, 1, 1], [0, 1, 0, 0]] and counts.tolist() == [4, 4, 0]
    assert out.tolist() == [[5, 0, 7, 7], [0, 3, 0, 0]]


def test_masked_pixel_splits_a_component_and_keeps_its_code():
    rows = [[5, 5, 5, 5, 5]]
    out, code, lab, counts = _filter(rows, 2, mask=[[1, 1, 2, 1, 1]])
    assert lab.tolist() == [[0, 0, -1, 3, 3]] and code.tolist() == [[3, 3, 2, 3, 3]] and counts.tolist() == [4, 0, 2]
    out, code, lab, counts = _filter(rows, 1, mask=[[1, 1, 0, 1, 1]])
    assert code.tolist() == [[1, 1, 0, 1, 1]] and counts.tolist() == [4, 4, 0]
    # a pixel the mask trusts but whose value is not a disparity: code 0, not the mask's 1
    out, code, lab, counts = _filter([[5, np.inf, 5]], 0, mask=[[1, 1, 1]])
    assert code.tolist() == [[1, 0, 1]]


def test_fill_is_the_background_fill_of_the_codes():
    out, code, lab, counts = _filter([[8, 8, 8, 0, 2, 0, 6, 6, 6]], 1, fill=1)
    assert code.tolist() == [[1, 1, 1, 0, 3, 0, 1, 1, 1]]
    assert out.tolist() == [[8, 8, 8, 6, 6, 6, 6, 6, 6]]    # the smaller of the nearest kept values left and right


@pytest.mark.parametrize("H,W", [(63, 255), (256, 512)])
def test_plateau_inputs_reach_every_code(H, W):
    """What tests/test_gpu_speckle.py asserts of its inputs at the middle parameter values, checked here on the CPU as well."""
    d, m = I.plateaus(2, H, W, 11), I.random_mask(2, H, W, 12)
    out, code, lab, counts = R.speckle_filter(d, m, 0.5, 50, 0)
    assert set(np.unique(code)) == {0, 1, 2, 3}
    assert (counts[:, 2] > 0).all() and (counts[:, 1] > 0).all()
    assert np.unique(R.speckle_filter(I.serpentine(1, H, W, 0), None, 0.5, 50, 0)[2]).tolist() == [-1, 0]      # one component
    assert np.unique(R.speckle_filter(I.spiral(1, H, W, 0), None, 0.5, 50, 0)[2]).tolist() == [-1, 0]
    assert np.unique(R.speckle_filter(I.comb(1, H, W, 0), None, 0.5, 50, 0)[2]).tolist() == [-1, 0]
    assert R.speckle_filter(I.checkerboard(1, H, W, 0), None, 1.0, 50, 0)[3].tolist() == [[H * W, 0, H * W]]
    assert R.speckle_filter(I.constant(1, H, W, 0), None, 0.0, 50, 0)[3].tolist() == [[H * W, H * W, 0]]


def test_edge_case_inputs_are_pairs_and_blocks():
    d = I.edge_cases()
    lab = R.labelling(d, None, 1.0)
    for b, want in enumerate([2, 2] + [4] * 9):
        sizes = np.unique(lab[b][2][lab[b][0]])
        assert sizes.tolist() == [want], (b, sizes)
    starts = {int(l) % d.shape[3] for l in np.unique(lab[0][1]) if l >= 0}
    assert starts == set(range(d.shape[3] - 1))             # a horizontal pair starts at every column


def _call(lib, disp=1 << 20, mask=None, B=1, H=8, W=8, max_diff=1.0, max_size=4, fill=0, workspace=1 << 24, out=1 << 21,
          mask_out=1 << 22, labels=None, counts=None):
    """lws_speckle_filter with made-up (never dereferenced) device addresses: every argument error returns before any GPU call."""
    return lib.lws_speckle_filter(disp, mask, B, H, W, max_diff, max_size, fill, workspace, out, mask_out, labels, counts, None)


def test_argument_errors_through_the_c_abi(hip_lib):
    lib = hip_lib
    bad = [dict(max_diff=-0.5), dict(max_diff=float("nan")), dict(max_diff=float("inf")), dict(max_size=-1), dict(fill=2), dict(B=0),
           dict(B=65536), dict(H=0), dict(W=0), dict(H=65536, W=32768), dict(disp=None), dict(workspace=None), dict(out=None),
           dict(mask_out=None), dict(fill=1, W=8193, H=1), dict(out=(1 << 20) + 64), dict(mask_out=(1 << 20) + 8),
           dict(labels=1 << 20), dict(workspace=(1 << 21) - 256), dict(mask=1 << 22, mask_out=(1 << 22) + 4)]
    for kw in bad:
        assert _call(lib, **kw) == _lib.LWS_ERR_INVALID, kw
        assert lib.lws_last_error().startswith(b"speckle_filter:"), (kw, lib.lws_last_error())
        with pytest.raises(ValueError, match="speckle_filter"):
            _lib.check(_lib.LWS_ERR_INVALID)
    assert _call(lib, max_diff=float("nan")) == _lib.LWS_ERR_INVALID and b"max_diff" in lib.lws_last_error()
    assert _call(lib, H=65536, W=32768) == _lib.LWS_ERR_INVALID and b"2^31" in lib.lws_last_error()
    assert _call(lib, out=(1 << 20) + 64) == _lib.LWS_ERR_INVALID and b"disp and out overlap" in lib.lws_last_error()


# (moved buffer, the buffer it is moved 16 bytes into, the whole error): every pair of the seven buffers, each alone
_OVERLAPS = [
    ("mask", "disp", b"speckle_filter: disp and mask overlap"), ("out", "disp", b"speckle_filter: disp and out overlap"),
    ("mask_out", "disp", b"speckle_filter: disp and mask_out overlap"), ("labels", "disp", b"speckle_filter: disp and labels overlap"),
    ("counts", "disp", b"speckle_filter: disp and counts overlap"), ("disp", "workspace", b"speckle_filter: disp and workspace overlap"),
    ("out", "mask", b"speckle_filter: mask and out overlap"), ("mask_out", "mask", b"speckle_filter: mask and mask_out overlap"),
    ("labels", "mask", b"speckle_filter: mask and labels overlap"), ("counts", "mask", b"speckle_filter: mask and counts overlap"),
    ("mask", "workspace", b"speckle_filter: mask and workspace overlap"), ("mask_out", "out", b"speckle_filter: out and mask_out overlap"),
    ("labels", "out", b"speckle_filter: out and labels overlap"), ("counts", "out", b"speckle_filter: out and counts overlap"),
    ("out", "workspace", b"speckle_filter: out and workspace overlap"), ("labels", "mask_out", b"speckle_filter: mask_out and labels overlap"),
    ("counts", "mask_out", b"speckle_filter: mask_out and counts overlap"),
    ("mask_out", "workspace", b"speckle_filter: mask_out and workspace overlap"),
    ("counts", "labels", b"speckle_filter: labels and counts overlap"), ("labels", "workspace", b"speckle_filter: labels and workspace overlap"),
    ("counts", "workspace", b"speckle_filter: counts and workspace overlap"),
]


def test_every_overlapping_pair_is_named(hip_lib):
    base = dict(disp=1 << 20, mask=1 << 23, workspace=1 << 24, out=1 << 21, mask_out=1 << 22, labels=1 << 25, counts=1 << 26)
    assert len({frozenset(c[:2]) for c in _OVERLAPS}) == 7 * 6 // 2
    for moved, onto, msg in _OVERLAPS:
        assert _call(hip_lib, **{**base, moved: base[onto] + 16}) == _lib.LWS_ERR_INVALID, (moved, onto)
        assert hip_lib.lws_last_error() == msg


def test_shared_checks_keep_their_whole_text(hip_lib):
    cases = [(dict(B=0), b"speckle_filter: bad shape B=0 H=8 W=8"), (dict(B=65536), b"speckle_filter: bad shape B=65536 H=8 W=8"),
             (dict(H=0), b"speckle_filter: bad shape B=1 H=0 W=8"), (dict(W=-1), b"speckle_filter: bad shape B=1 H=8 W=-1"),
             (dict(H=65536, W=32768), b"speckle_filter: H*W = 65536x32768 must be < 2^31"),
             (dict(max_diff=-0.5), b"speckle_filter: max_diff must be finite and >= 0, got -0.5"),
             (dict(max_diff=float("inf")), b"speckle_filter: max_diff must be finite and >= 0, got inf"),
             (dict(max_diff=float("nan")), b"speckle_filter: max_diff must be finite and >= 0, got nan"),
             (dict(fill=2), b"speckle_filter: fill 2 (0 = zero, 1 = background fill)"),
             (dict(fill=-1), b"speckle_filter: fill -1 (0 = zero, 1 = background fill)"),
             (dict(fill=1, W=8193, H=1), b"speckle_filter: fill needs W <= 8192 (the row is staged in LDS), got 8193"),
             (dict(disp=(1 << 20) + 2), b"speckle_filter: disp / out / labels must be 4-byte, counts 8-byte, workspace 16-byte aligned"),
             (dict(counts=(1 << 26) + 4), b"speckle_filter: disp / out / labels must be 4-byte, counts 8-byte, workspace 16-byte aligned"),
             (dict(workspace=(1 << 24) + 8), b"speckle_filter: disp / out / labels must be 4-byte, counts 8-byte, workspace 16-byte aligned")]
    for kw, msg in cases:
        assert _call(hip_lib, **kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error() == msg, kw
    for shape, msg in (((0, 8, 8), b"speckle_workspace: bad shape B=0 H=8 W=8"), ((1, 8, 0), b"speckle_workspace: bad shape B=1 H=8 W=0"),
                       ((1, 65536, 32768), b"speckle_workspace: H*W = 65536x32768 must be < 2^31")):
        assert hip_lib.lws_speckle_workspace(*shape) == _lib.LWS_ERR_INVALID
        assert hip_lib.lws_last_error() == msg


def test_workspace_size(hip_lib):
    lib = hip_lib
    sizes = [lib.lws_speckle_workspace(B, 368, 1232) for B in (1, 2, 3, 8)]
    assert all(s > 0 for s in sizes) and sizes == sorted(set(sizes))
    assert 8 * 368 * 1232 <= sizes[0] <= 8 * 368 * 1232 + 12 * 368 + 3 * 256          # 8 bytes per pixel + 12 per row
    assert lib.lws_speckle_workspace(1, 8, 1) >= 8 * 8
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (65536, 8, 8), (1, 65536, 32768)):
        assert lib.lws_speckle_workspace(B, H, W) == _lib.LWS_ERR_INVALID
        assert lib.lws_last_error().startswith(b"speckle_workspace:")


def test_ops_validates_before_the_library():
    from lwsnet_amd import ops
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.speckle_filter(np.zeros((1, 1, 8, 8), np.float32), 4)


def test_grey_table_keeps_its_first_three_values():
    from lwsnet_amd import imageio as io
    assert io.LR_MASK_GREY[:3].tolist() == [0, 255, 128] and len(io.LR_MASK_GREY) == 4
    assert io.LR_MASK_GREY[3] not in (0, 255, 128)


@pytest.mark.parametrize("argv", [["--speckle_fill"], ["--speckle_diff", "0.5"], ["--speckle", "0"], ["--speckle", "-3"],
                                  ["--speckle", "10", "--speckle_diff", "nan"], ["--speckle", "10", "--speckle_diff", "-1"],
                                  ["--speckle", "10", "--workers", "4"]])
def test_cli_argument_errors(argv, capsys):
    from lwsnet_amd import evaluate, inference
    for mod in (inference, evaluate):
        p = mod.build_parser()
        args = p.parse_args(argv)
        with pytest.raises(SystemExit) as e:
            inference.check_speckle_arguments(p, args)
        assert e.value.code == 2
        assert "--speckle" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        inference.main(["--synthetic_weights", "--left_img", "nowhere/left.png"] + argv)


def test_cli_defaults():
    from lwsnet_amd import inference
    p = inference.build_parser()
    args = p.parse_args(["--speckle", "50"])
    inference.check_speckle_arguments(p, args)
    assert args.speckle == 50 and args.speckle_diff == 1.0 and args.speckle_fill is False
    args = p.parse_args([])
    inference.check_speckle_arguments(p, args)
    assert args.speckle is None
