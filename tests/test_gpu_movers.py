"""lws_movers on the device against the numpy restatement (tests/movers_reference.py): every output bit for bit.  The shapes are the
smallest that can still go wrong -- 37 x 83 and 64 x 129, no multiple of the 32 x 64 labelling tile, the 4 x 64 evidence tile or the
2048-pixel numbering block, with a one-pixel spiral through every tile and a ring on all four image borders; 2 x 4 and 4 x 4 around
the photometric term's W >= 4 rule; projections that land exactly on u = W - 1, v = 0 and half-way between pixels; windows of radius
0, 1, 2 at the corners; NaN, +-inf and tiny disparities and sigmas in both frames; a motion that puts points behind the camera;
components of exactly min_pixels and one less; more movers than slots; grow 0, 1, 8 against the borders.  Then: mask_out in place,
a permuted batch, poisoned guard bands and workspace, argument errors that launch nothing, a captured graph, MoverSegmenter over the
four scenes of tests/test_movers_cpu.py, and the CLI."""
import ctypes
import os

import numpy as np
import pytest

import guarded
import movers_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, cu  # noqa: E402

F = np.float32
OUTPUTS = ("evidence", "mask", "labels", "rows", "vals", "info")
INPUTS = ("rgb_prev", "disp_prev", "sigma_prev", "mask_prev", "rgb_cur", "disp_cur", "sigma_cur", "mask_cur", "cam", "pose")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def cameras(rows):
    """The Camera objects whose float32 rows are `rows`, bit for bit."""
    from lwsnet_amd.geometry import Camera, camera_rows
    cams = [Camera(*(float(v) for v in r[:4]), float(r[4]) / float(r[0])) for r in rows]
    assert np.array_equal(camera_rows(cams, len(cams)), np.asarray(rows, F))
    return cams


def run_op(dev, case, **kw):
    """ops.movers on a case of tests/movers_reference.py: the six outputs as numpy arrays."""
    from lwsnet_amd import ops
    t = {k: None if case.get(k) is None else cu(case[k], dev) for k in INPUTS}
    res = ops.movers(t["rgb_prev"], t["disp_prev"], t["rgb_cur"], t["disp_cur"], cameras(case["cam"]), t["pose"], sigma_prev=t["sigma_prev"],
                     mask_prev=t["mask_prev"], sigma_cur=t["sigma_cur"], mask_cur=t["mask_cur"], **kw)
    return {k: v.cpu().numpy() for k, v in res._asdict().items()}


def compare(got, want, what):
    for k in OUTPUTS:
        guarded.assert_bits(got[k], want[k], f"{what} {k}")


def check_case(dev, case, what, **kw):
    want = R.run_case(case, **kw)
    compare(run_op(dev, case, **kw), want, what)
    return want


# ---- the pattern cases: a spiral through every tile, a ring on the four borders, blobs of chosen sizes ----
def pattern(H, W):
    """(want uint8 [H,W], near bool [H,W]): static everywhere but a ring of `appeared` on the four borders, a spiral of `changed`
    inside it (two pixels in), and in the spiral's free middle nothing; the spiral's first arm is `uncovered` for its first 9 pixels."""
    want = np.full((H, W), R.STATIC, np.uint8)
    want[[0, H - 1], :] = R.APPEARED
    want[:, [0, W - 1]] = R.APPEARED
    sp = R.spiral(H, W)
    want[sp] = R.CHANGED
    want[2, 2:11] = R.UNCOVERED
    return want, np.zeros((H, W), bool)


def blobs(H, W, sizes):
    """want with one horizontal run of `appeared` per size, every other row, from column 1; the rest static."""
    want = np.full((H, W), R.STATIC, np.uint8)
    for k, n in enumerate(sizes):
        assert n <= W - 2 and 1 + 2 * k < H
        want[1 + 2 * k, 1:1 + n] = R.APPEARED
    return want


@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("H,W", ((37, 83), (64, 129)))
def test_spiral_and_border_ring_bit_for_bit(dev, hip_lib, H, W, radius):
    want, near = pattern(H, W)
    case = R.pattern_case(want, near, seed=H)
    kw = dict(radius=radius, cand_bits=28, min_pixels=8, grow=1, max_movers=8)
    ref = check_case(dev, case, f"{H}x{W} radius {radius}", **kw)
    if radius == 0:                                         # the construction gives the evidence it was made for; a window then softens it
        assert np.array_equal(ref["evidence"][0, 0], want)
        rows = ref["rows"][0]
        assert ref["info"][0, 6] == 2 and rows[0].tolist()[:5] == [2 * (H + W) - 4, 0, W - 1, 0, H - 1]       # the ring touches all four borders
        n_spiral = int(R.spiral(H, W).sum())
        assert rows[1, 0] == n_spiral and rows[1, 6] == 9 and rows[1, 7] == n_spiral - 9          # one component through every tile
        tiles = {(y // 32, x // 64) for y, x in zip(*np.nonzero(ref["labels"][0, 0] == 1))}
        assert len(tiles) >= 4


@pytest.mark.parametrize("H,W", ((2, 4), (4, 4)))
def test_the_photometric_term_is_on_from_four_by_four(dev, hip_lib, H, W):
    """Every pixel's grey changes by 80 levels and its disparity agrees: `changed` where the photometric test is on -- the four
    middle pixels of 4 x 4 -- and `static` everywhere else, and on all of 2 x 4."""
    case = R.pattern_case(np.full((H, W), R.CHANGED, np.uint8))
    ref = check_case(dev, case, f"{H}x{W}", min_pixels=1, grow=0, max_movers=4)
    changed = ref["evidence"][0, 0] == R.CHANGED
    assert int(changed.sum()) == (4 if H == 4 else 0) and (ref["evidence"][0, 0][~changed] == R.STATIC).all()
    assert ref["info"][0, 6] == (1 if H == 4 else 0)


@pytest.mark.parametrize("sx,sy", ((1.0, -1.0), (0.5, -0.5), (-0.5, 1.5), (0.0, 0.0)))
def test_projections_on_the_last_column_the_first_row_and_half_way(dev, hip_lib, sx, sy):
    H, W = 9, 14
    case = R.shift_case(H, W, sx, sy, seed=3)
    okc = np.ones((H, W), bool)
    _, _, _, _, (iv, iu, u, v) = R.residuals(case["rgb_prev"][0], case["disp_prev"][0, 0], None, okc, case["rgb_cur"][0], case["disp_cur"][0, 0], None,
                                             okc, case["cam"][0], case["pose"][0], R.params())
    xs, ys = np.arange(W, dtype=F)[None, :], np.arange(H, dtype=F)[:, None]
    assert np.array_equal(u, np.broadcast_to(xs + F(sx), (H, W))) and np.array_equal(v, np.broadcast_to(ys + F(sy), (H, W)))      # exact
    if sx == 1.0:
        assert (u[:, W - 2] == W - 1).all() and (v[1] == 0).all()
    for radius in (0, 2):
        ref = check_case(dev, case, f"shift {sx},{sy} radius {radius}", radius=radius, min_pixels=2, grow=1, cand_bits=28)
        tested = ref["evidence"][0, 0] != 0
        inside = (u >= 0) & (u <= W - 1) & (v >= 0) & (v <= H - 1)
        assert np.array_equal(tested, inside)               # a projection exactly on the last column or the first row is inside
    if sx == 0.5:                                           # ties go to the even column and row
        assert iu[1, :4].tolist() == [0, 2, 2, 4] and iv[1:5, 0].tolist() == [0, 2, 2, 4]


@pytest.mark.parametrize("radius", (0, 1, 2))
@pytest.mark.parametrize("H,W,B", ((37, 83, 1), (64, 129, 2), (5, 7, 3)))
def test_messy_inputs_with_nan_inf_and_tiny_values_in_both_frames(dev, hip_lib, H, W, B, radius):
    case = R.stack_cases([R.messy_case(H, W, seed=10 * b + radius) for b in range(B)])
    for k in ("disp_prev", "disp_cur", "sigma_prev", "sigma_cur"):
        assert H <= 5 or (np.isnan(case[k]).any() and np.isinf(case[k]).any())
    ref = check_case(dev, case, f"messy {H}x{W} B{B} radius {radius}", radius=radius, min_pixels=3, grow=radius, cand_bits=(20, 28, 4)[radius],
                     max_diff=(1.0, 0.25, float("inf"))[radius], sigma0=0.3, max_movers=16)
    if H > 5:
        assert (np.bincount(ref["evidence"].reshape(-1), minlength=5) > 0).all() and (ref["info"][:, 6] > 0).all()


def test_without_sigma_maps_and_masks_and_without_labels(dev, hip_lib):
    from lwsnet_amd import ops
    case = R.messy_case(37, 83, seed=5, specials=False)
    for k in ("sigma_prev", "sigma_cur", "mask_prev", "mask_cur"):
        case[k] = None
    want = R.run_case(case, min_pixels=3, gate_p=float("inf"))
    got = run_op(dev, case, min_pixels=3, gate_p=float("inf"))
    compare(got, want, "no optional maps")
    assert want["info"][0, 4] == 0                          # an infinite photometric gate: nothing is `changed`
    t = {k: None if case.get(k) is None else cu(case[k], dev) for k in INPUTS}
    res = ops.movers(t["rgb_prev"], t["disp_prev"], t["rgb_cur"], t["disp_cur"], cameras(case["cam"]), t["pose"], min_pixels=3, gate_p=float("inf"),
                     labels=False)
    assert res.labels is None
    guarded.assert_bits(res.mask, want["mask"], "mask without labels")


def test_a_pose_that_looks_backwards_and_one_that_drives_through_the_scene(dev, hip_lib):
    H, W = 37, 83
    back = R.messy_case(H, W, seed=7, specials=False)
    back["pose"] = np.array([[[-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0]] * 2], F)      # half a turn about y: every Qz < 0
    ref = check_case(dev, back, "backwards", min_pixels=3)
    assert (ref["evidence"] == 0).all() and ref["info"][0].tolist() == [0] * 8
    through = R.messy_case(H, W, seed=8, specials=False, tz=-5.0)       # pose[1] moves the points 5 m towards the previous camera and past it
    ref = check_case(dev, through, "through", min_pixels=3)
    okc = through["mask_cur"][0, 0] == 1
    fb, d = through["cam"][0, 4], through["disp_cur"][0, 0]
    behind = okc & (d > 0) & (fb / d < 4.5)
    assert behind.sum() > 50 and (ref["evidence"][0, 0][behind] == 0).all() and (ref["evidence"] != 0).sum() > 20


def test_a_component_of_min_pixels_is_a_mover_and_one_less_is_not(dev, hip_lib):
    H, W = 12, 20
    case = R.pattern_case(blobs(H, W, (7, 6, 8, 5, 6)))
    ref = check_case(dev, case, "sizes", min_pixels=6, grow=0, max_movers=8)
    assert ref["info"][0, 5:7].tolist() == [5, 4] and ref["rows"][0, :5, 0].tolist() == [7, 6, 8, 6, 0]
    assert (ref["labels"][0, 0][7] == -1).all() and (ref["mask"][0, 0][7] == 1).all()                 # the run of five


def test_more_movers_than_slots(dev, hip_lib):
    H, W = 12, 20
    case = R.pattern_case(blobs(H, W, (4, 5, 6, 7, 8)))
    ref = check_case(dev, case, "cap", min_pixels=4, grow=0, max_movers=3)
    assert ref["info"][0, 6] == 5 and ref["info"][0, 7] == 30 and ref["rows"].shape == (1, 3, 8) and ref["rows"][0, :, 0].tolist() == [4, 5, 6]
    lab, mask = ref["labels"][0, 0], ref["mask"][0, 0]
    assert (lab[7, 1:8] == -1).all() and (lab[9, 1:9] == -1).all() and (mask[7, 1:8] == 4).all() and (mask[9, 1:9] == 4).all()
    assert sorted(np.unique(lab).tolist()) == [-1, 0, 1, 2]


@pytest.mark.parametrize("grow", (0, 1, 8))
def test_grow_against_the_borders(dev, hip_lib, grow):
    H, W = 21, 30
    want = np.full((H, W), R.STATIC, np.uint8)
    want[0, 0:3] = want[H - 1, W - 4:W] = want[10, 13:17] = R.APPEARED
    want[3, 20] = R.UNTESTED                               # an untested pixel keeps its own code unless a mover grows over it
    case = R.pattern_case(want)
    ref = check_case(dev, case, f"grow {grow}", min_pixels=3, grow=grow, max_movers=4)
    member = ref["labels"][0, 0] >= 0
    ys, xs = np.nonzero(member)
    dist = np.min(np.maximum(np.abs(np.arange(H)[:, None, None] - ys), np.abs(np.arange(W)[None, :, None] - xs)), -1)
    assert np.array_equal(ref["mask"][0, 0] == 4, dist <= grow) and ref["info"][0, 7] == (dist <= grow).sum()
    assert ref["mask"][0, 0][3, 20] == (4 if dist[3, 20] <= grow else 0)


def test_two_blobs_that_touch_at_different_depths_are_two_components(dev, hip_lib):
    H, W = 12, 20
    want = np.full((H, W), R.STATIC, np.uint8)
    want[3:7, 2:14] = R.APPEARED
    near = np.zeros((H, W), bool)
    near[3:7, 8:14] = True                                  # disparity 16 beside 8: not joined at max_diff 1, joined at 8
    case = R.pattern_case(want, near)
    ref = check_case(dev, case, "split", min_pixels=4, grow=0)
    assert ref["info"][0, 6] == 2 and ref["vals"][0, :2].tolist() == [[8.0, 8.0], [16.0, 4.0]]
    ref = check_case(dev, case, "joined", min_pixels=4, grow=0, max_diff=8.0)
    assert ref["info"][0, 6] == 1 and ref["rows"][0, 0, 0] == 48 and ref["vals"][0, 0].tolist() == [12.0, F(64.0) / F(12.0)]


# ---- raw calls: in place, guard bands, argument errors, a graph ----
SCALARS = dict(min_disp=1.0, sigma0=0.3, sigma_min=0.05, gate_g=3.0, gate_p=25.0, radius=1, cand_bits=28, max_diff=1.0, min_pixels=3, grow=2,
               max_movers=16)


def output_buffers(make, B, H, W, K, hip_lib):
    ws = hip_lib.lws_movers_workspace(B, H, W, K)
    assert ws > 0
    return dict(work=make((ws,), np.uint8, "work"), evidence=make((B, 1, H, W), np.uint8, "evidence"), mask=make((B, 1, H, W), np.uint8, "mask"),
                labels=make((B, 1, H, W), np.int32, "labels"), rows=make((B, K, 8), np.int32, "rows"), vals=make((B, K, 2), F, "vals"),
                info=make((B, 8), np.int32, "info"))


def raw_call(hip_lib, dev, b, shape, **kw):
    s = {**SCALARS, **kw}
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    return hip_lib.lws_movers(*(ptr(b.get(k)) for k in INPUTS), *shape, s["min_disp"], s["sigma0"], s["sigma_min"], s["gate_g"], s["gate_p"],
                              s["radius"], s["cand_bits"], s["max_diff"], s["min_pixels"], s["grow"], s["max_movers"], ptr(b["work"]),
                              ptr(b["evidence"]), ptr(b["mask"]), ptr(b.get("labels")), ptr(b["rows"]), ptr(b["vals"]), ptr(b["info"]), stream)


def plain_buffers(dev, case, hip_lib, K=SCALARS["max_movers"]):
    B, _, H, W = case["disp_cur"].shape
    b = {k: None if case.get(k) is None else cu(case[k], dev) for k in INPUTS}
    b.update(output_buffers(lambda shape, dt, name: torch.full(shape, 77, dtype=torch.from_numpy(np.empty(0, dt)).dtype, device=dev), B, H, W, K, hip_lib))
    return b, (B, H, W)


def test_mask_out_in_place_over_mask_cur(dev, hip_lib):
    case = R.stack_cases([R.messy_case(37, 83, seed=20 + b) for b in range(2)])
    want = R.run_case(case, **SCALARS)
    b, shape = plain_buffers(dev, case, hip_lib)
    b["mask"] = b["mask_cur"]
    assert raw_call(hip_lib, dev, b, shape) == 0, hip_lib.lws_last_error()
    torch.cuda.synchronize(dev)
    for k in OUTPUTS:
        guarded.assert_bits(b[k], want[k], f"in place {k}")
    assert (want["mask"] == 4).any() and (want["mask"] == 3).any()          # movers, and codes of mask_cur that came through


def test_an_image_gives_the_same_bytes_at_any_place_in_a_batch(dev, hip_lib):
    H, W = 37, 83
    singles = [R.messy_case(H, W, seed=30 + b, tz=0.1 * b) for b in range(3)]
    kw = dict(radius=1, min_pixels=3, cand_bits=28)
    alone = [run_op(dev, c, **kw) for c in singles]
    for order in ((0, 1, 2), (2, 0, 1), (1, 2, 0)):
        got = run_op(dev, R.stack_cases([singles[i] for i in order]), **kw)
        for place, i in enumerate(order):
            for k in OUTPUTS:
                guarded.assert_bits(got[k][place], alone[i][k][0], f"order {order} image {i} {k}")
    again = run_op(dev, singles[0], **kw)
    for k in OUTPUTS:
        guarded.assert_bits(again[k], alone[0][k], f"second run {k}")


@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Every tensor between poisoned flanks and one element past a 16-byte boundary (the workspace keeps its alignment), outputs and
    workspace poisoned inside: the same bytes as from plain memory, and no flank changed."""
    case = R.stack_cases([R.messy_case(37, 83, seed=40 + b) for b in range(2)])
    want = R.run_case(case, **SCALARS)
    gd = guarded.Guard(dev, word, skew=1)
    b = {k: gd.place(case[k], word=guarded.MASK_WORD if k.startswith("mask") else None, name=k) for k in INPUTS}
    B, _, H, W = case["disp_cur"].shape
    b.update(output_buffers(lambda shape, dt, name: gd.empty(shape, dt, align16=name == "work", name=name), B, H, W, SCALARS["max_movers"], hip_lib))
    assert raw_call(hip_lib, dev, b, (B, H, W)) == 0, hip_lib.lws_last_error()
    torch.cuda.synchronize(dev)
    gd.check()
    for k in OUTPUTS:
        guarded.assert_bits(b[k], want[k], f"guarded {k}")


def test_argument_errors_launch_nothing(dev, hip_lib):
    from lwsnet_amd import _lib
    case = R.messy_case(12, 20, seed=50)
    b, shape = plain_buffers(dev, case, hip_lib)
    bad = [dict(radius=3), dict(radius=-1), dict(cand_bits=1), dict(cand_bits=2), dict(cand_bits=32), dict(grow=9), dict(grow=-1), dict(min_pixels=0),
           dict(max_movers=0), dict(max_movers=65537), dict(gate_g=0.0), dict(gate_g=float("inf")), dict(gate_p=0.0), dict(gate_p=float("nan")),
           dict(max_diff=-1.0), dict(max_diff=float("nan")), dict(min_disp=0.0), dict(sigma0=-1.0), dict(sigma_min=0.0)]
    for kw in bad:
        assert raw_call(hip_lib, dev, b, shape, **kw) == _lib.LWS_ERR_INVALID, kw
        assert hip_lib.lws_last_error().startswith(b"movers: "), kw
    for k in ("rgb_prev", "disp_prev", "rgb_cur", "disp_cur", "cam", "pose", "work", "evidence", "mask", "rows", "vals", "info"):
        assert raw_call(hip_lib, dev, {**b, k: None}, shape) == _lib.LWS_ERR_INVALID, k
        assert hip_lib.lws_last_error().endswith(b"must not be null"), k
    assert raw_call(hip_lib, dev, b, (0, 12, 20)) == _lib.LWS_ERR_INVALID and raw_call(hip_lib, dev, b, (1, 1 << 16, 1 << 15)) == _lib.LWS_ERR_INVALID
    assert raw_call(hip_lib, dev, {**b, "mask": b["evidence"]}, shape) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_last_error() == b"movers: mask_out and evidence overlap"
    assert raw_call(hip_lib, dev, {**b, "evidence": b["mask_cur"]}, shape) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_last_error() == b"movers: mask_cur and evidence overlap"
    assert raw_call(hip_lib, dev, {**b, "mask": b["mask_cur"].view(-1)[1:]}, shape) == _lib.LWS_ERR_INVALID          # in place means the same pointer
    assert raw_call(hip_lib, dev, {**b, "disp_cur": b["disp_cur"].view(torch.uint8).view(-1)[2:]}, shape) == _lib.LWS_ERR_INVALID
    assert hip_lib.lws_last_error().endswith(b"workspace 16-byte aligned")
    torch.cuda.synchronize(dev)
    # nothing was launched: every output and the workspace hold what they held
    assert (b["evidence"] == 77).all() and (b["mask"] == 77).all() and (b["labels"] == 77).all() and (b["rows"] == 77).all() and (b["info"] == 77).all()
    assert (b["vals"] == 77).all() and (b["work"] == 77).all()


def test_graph_capture_replays_on_changed_inputs(dev, hip_lib):
    H, W, B = 37, 83, 2
    first = R.stack_cases([R.messy_case(H, W, seed=60 + b) for b in range(B)])
    second = R.stack_cases([R.messy_case(H, W, seed=70 + b, tz=0.2) for b in range(B)])
    want = {id(c): R.run_case(c, **SCALARS) for c in (first, second)}
    b, shape = plain_buffers(dev, first, hip_lib)
    assert raw_call(hip_lib, dev, b, shape) == 0            # the code object is loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert raw_call(hip_lib, dev, b, shape) == 0
    for c in (first, second, first):
        for k in INPUTS:
            b[k].copy_(cu(c[k], dev))
        for k in ("work", "evidence", "mask", "labels", "rows", "vals", "info"):
            b[k].fill_(77)
        graph.replay()
        torch.cuda.synchronize(dev)
        for k in OUTPUTS:
            guarded.assert_bits(b[k], want[id(c)][k], f"replay {k}")


# ---- the state-holding class ----
@pytest.mark.parametrize("name", ("static", "approaching", "receding", "lateral"))
def test_mover_segmenter_over_the_scenes(dev, hip_lib, name):
    from lwsnet_amd.movers import MoverSegmenter
    boxes = R.BOX.get(name, (None, None))
    case, inside = R.scene_pair(*boxes, noise=0.2, seed=1)
    kw = dict(min_disp=0.5, cand_bits=28 if name == "receding" else 20)
    want = R.run_case(case, **kw)
    seg = MoverSegmenter(cameras(case["cam"])[0], **kw)
    first = seg.step(cu(case["rgb_prev"], dev), cu(case["disp_prev"], dev), None, mask=cu(case["mask_prev"], dev))
    assert first is None and seg.prev is not None
    res = seg.step(cu(case["rgb_cur"], dev), cu(case["disp_cur"], dev), cu(case["pose"], dev), mask=cu(case["mask_cur"], dev))
    compare({k: v.cpu().numpy() for k, v in res._asdict().items()}, want, name)
    assert (want["info"][0, 6] > 0) == (name != "static")
    assert seg.step(cu(case["rgb_cur"], dev), cu(case["disp_cur"], dev), None) is None                # no trusted motion: not segmented
    host = seg.step(cu(case["rgb_cur"], dev), cu(case["disp_cur"], dev), case["pose"][0])             # a host [2,12], as geometry.relative_pose gives
    assert host is not None and int(host.info[0, 0]) > 0


# ---- the CLI ----
def write_sequence(root, n, H=375, W=1242):
    """n frames of one synthetic pair with a textured square pasted 14 columns further right in each (30 columns of disparity)."""
    from PIL import Image
    from lwsnet_amd import synth
    left, right, _ = synth.make_pair(H, W, 0)
    patch = synth.to_rgb8(synth.make_pair(H, W, 1)[0])
    left, right = synth.to_rgb8(left), synth.to_rgb8(right)
    for side in ("image_2", "image_3"):
        os.makedirs(os.path.join(root, side), exist_ok=True)
    for k in range(n):
        l, r = left.copy(), right.copy()
        x = 500 + 14 * k
        l[200:260, x:x + 60] = patch[200:260, 500:560]
        r[200:260, x - 30:x + 30] = patch[200:260, 500:560]
        Image.fromarray(l).save(os.path.join(root, "image_2", f"{k:06d}_10.png"))
        Image.fromarray(r).save(os.path.join(root, "image_3", f"{k:06d}_10.png"))


def test_inference_cli_movers_files(dev, model, tmp_path, caplog):
    """Six frames with --egomotion --movers --tsdf --save_movers: the files exist, every log line is what Odometry and MoverSegmenter
    give composed by hand, and the volume takes fewer voxels than in the same run without --movers.  The weights are synthetic, so
    the maps are rough and a component is a few pixels: the run asks for movers of 4 pixels grown by 8, which is what the wiring
    needs to show; what the segmentation finds in a scene is the matter of tests/test_movers_cpu.py."""
    import logging
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, outputs
    from lwsnet_amd import postprocess as post
    from lwsnet_amd.egomotion import Odometry
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.movers import MoverSegmenter
    n = 6
    root = str(tmp_path / "kitti")
    write_sequence(root, n)
    calib = tmp_path / "calib.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    out, plain_out = tmp_path / "out", tmp_path / "plain"
    common = ["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--egomotion", "--ego_levels", "3", "--ego_iters", "4",
              "--tsdf", "--tsdf_voxel", "0.4", "--tsdf_extent", "-8", "8", "-3.2", "3.2", "0", "32"]
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(common + ["--save_path", str(out), "--movers", "--save_movers", "--movers_min_pixels", "4", "--movers_grow", "8"])
    lines = [r.getMessage() for r in caplog.records]
    stems = [f"{k:06d}_10" for k in range(n)]
    assert sorted(os.listdir(out)) == sorted(s + e for s in stems for e in (".png", "_movers.png", "_movers.csv"))
    assert len(written) == 3 * n
    got = [line for line in lines if line.startswith("Movers: tested = ")]
    opts = post.Options.make()
    odo = seg = None
    expected, csv_lines = [], []
    for k, stem in enumerate(stems):
        full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
        left = io.crop_bottom_right(full)
        r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
        cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
        res = post.run_chain(model, io.to_input(left)[None], r_in, opts)
        assert res.keep is None                             # a run without checks: --movers gives the stages behind it their codes
        rgb, d = outputs.rgb_on_device(left, dev), res.disp[3].as_subclass(torch.Tensor)
        odo = odo or Odometry(cam, levels=3, iters=4, huber=10.0, min_disp=1.0)
        seg = seg or MoverSegmenter(cam, gate_g=3.0, gate_p=25.0, radius=0, min_pixels=4, grow=8, cand_bits=ops.MOVER_CANDIDATES, min_disp=1.0)
        ego = odo.step(rgb, d, None)
        pose = None if ego is None or int(ego.status[0]) & ops.EGO_UNTRUSTED else ego.pose
        mv = seg.step(rgb, d, pose)
        png = np.asarray(Image.open(out / (stem + "_movers.png")))
        if mv is None:
            assert not png.any()
            continue
        info = mv.info[0].cpu().tolist()
        expected.append(outputs.movers_line(info, mv.rows[0].cpu().numpy(), mv.vals[0].cpu().numpy()))
        assert expected[-1].startswith("Movers: tested = {}, static = {}, appeared = {}, uncovered = {}, changed = {}, components = {}, movers = {}, "
                                       "masked pixels = {}".format(*info))
        assert np.array_equal(png, outputs.movers_to_rgb(mv.evidence[0, 0].cpu().numpy(), mv.labels[0, 0].cpu().numpy())), stem
        csv_lines.append(len((out / (stem + "_movers.csv")).read_text().splitlines()) - 1)
        assert csv_lines[-1] == min(info[6], 64)
    print("\n".join(got))
    assert got == expected and len(got) >= 1
    assert sum(csv_lines) >= 1, "the pasted square is found in no frame"
    with_movers = [int(line.split("=")[1]) for line in lines if line.startswith("TSDF: voxels updated = ")]
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        inference.main(common + ["--save_path", str(plain_out)])
    without = [int(r.getMessage().split("=")[1]) for r in caplog.records if r.getMessage().startswith("TSDF: voxels updated = ")]
    assert sorted(os.listdir(plain_out)) == sorted(s + ".png" for s in stems)
    print("voxels updated with --movers:", with_movers, "without:", without)
    assert len(with_movers) == len(without) == n and with_movers[0] == without[0] and sum(with_movers) < sum(without)
