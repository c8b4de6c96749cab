"""The one-forward occlusion check on the device: lws_occlusion_check bit for bit against the numpy restatement
(tests/occ_reference.py) at every width where the kernel takes another path (a scalar tail, one quad, more than one quad per
thread, the LDS limit), on every kind of input, at skewed addresses and in place, between poisoned guard bands, in any batch, and
replayed from a captured graph; LWSNet.forward_occ against a plain forward plus the restatement; postprocess.run_chain with the
check on against the same steps composed by hand.  The shapes are a few rows of each width: the kernel shares nothing between rows."""
import ctypes

import numpy as np
import pytest

import guarded as G
import occ_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WIDTHS = [1, 3, 4, 5, 63, 64, 65, 257, 1023, 1232, 8189, 8192]
TAUS = (0.0, 0.5, 1.0)
_REF = {}


def ref(key, fn):
    """References are computed once per case and shared; never modified."""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def cu(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def host(t):
    return t.detach().cpu().numpy()


# ---- inputs ----
def ramps(B, H, W, seed):
    """Smooth ramps with jumps: slanted surfaces (targets 0..2 columns apart) and plateaus in front of them."""
    rng = np.random.default_rng(seed)
    slope = rng.uniform(-0.3, 0.6, (B, 1, H, 1))
    d = rng.uniform(0.0, min(40.0, W / 2.0), (B, 1, H, 1)) + slope * np.arange(W)
    for _ in range(1 + W // 64):
        x0 = int(rng.integers(W))
        d[..., x0:x0 + int(rng.integers(1, max(2, W // 8)))] += rng.uniform(-20.0, 20.0)
    return d.astype(np.float32)


def noise(B, H, W, seed):
    return np.random.default_rng(seed).uniform(-3.0, W + 3.0, (B, 1, H, W)).astype(np.float32)


def sprinkled(B, H, W, seed):
    d = ramps(B, H, W, seed)
    rng = np.random.default_rng(seed + 1)
    flat = d.reshape(-1)
    for v in (np.nan, np.inf, -np.inf, -0.0, 1e30):
        flat[rng.choice(flat.size, size=max(1, flat.size // 40), replace=False)] = v
    return d


def halves(B, H, W, seed):
    """Integer and half-integer disparities: one-tap splats, and targets at k + 0.5 that rint sends to the even column."""
    return (np.round(np.random.default_rng(seed).uniform(-3.0, W + 3.0, (B, 1, H, W)) * 2) / 2).astype(np.float32)


def stage_maps(B, H, W):
    return ref(("in", B, H, W), lambda: [ramps(B, H, W, W), noise(B, H, W, W + 1), sprinkled(B, H, W, W + 2), halves(B, H, W, W + 3)])


def special_rows(W):
    """[1,1,3,W]: d = x (every pixel lands on column 0: one LDS word takes all W maxima), constant 0, all NaN."""
    d = np.zeros((1, 1, 3, W), np.float32)
    d[0, 0, 0] = np.arange(W)
    d[0, 0, 2] = np.nan
    return d


def want(name, d, tau, fill):
    return ref((name, tau, fill), lambda: R.occlusion_check(d, tau, fill))


# ---- the raw call ----
def raw_call(lib, dev, dl, tau, fill, out, mask, right=None, kept=None):
    """lws_occlusion_check on torch's current stream; right: None, or a list with None for the maps whose right view is skipped."""
    from lwsnet_amd import _lib
    arr = ctypes.c_void_p * 4
    p = lambda ts: arr(*[t.data_ptr() if t is not None else None for t in ts])      # noqa: E731
    B, _, H, W = dl[0].shape
    with torch.cuda.device(dev):
        _lib.check(lib.lws_occlusion_check(p(dl), len(dl), B, H, W, float(tau), int(fill), p(out), p(mask), p(right) if right is not None else arr(),
                                           ctypes.c_void_p(kept.data_ptr()) if kept is not None else None,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_occlusion_check")


def check_outputs(what, wants, out, mask, right, kept):
    for s, (wo, wm, wr, wk) in enumerate(wants):
        G.assert_bits(out[s], wo, f"{what} out {s}")
        G.assert_bits(mask[s], wm, f"{what} mask {s}")
        if right is not None and right[s] is not None:
            G.assert_bits(right[s], wr, f"{what} right {s}")
        if kept is not None:
            G.assert_bits(kept[s], wk, f"{what} row_kept {s}")


@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("W", WIDTHS)
def test_occlusion_check_bitexact(dev, hip_lib, W, B, H):
    stages = stage_maps(B, H, W)
    dls = [cu(d, dev) for d in stages]
    codes = set()
    for nmaps in (1, 4):
        for tau in TAUS:
            for fill in (0, 1):
                k = nmaps + fill + int(2 * tau)                          # the optional outputs every way over the loop
                dl = dls[:nmaps]
                out = [torch.empty_like(d) for d in dl]
                mask = [torch.empty(d.shape, dtype=torch.uint8, device=dev) for d in dl]
                right = [torch.empty_like(d) for d in dl] if k % 3 else None
                if right is not None and nmaps == 4 and k % 3 == 1:
                    right[1] = None                                      # one right[s] NULL among the others
                kept = torch.empty((nmaps, B, H), dtype=torch.int32, device=dev) if k % 2 else None
                raw_call(hip_lib, dev, dl, tau, fill, out, mask, right, kept)
                wants = [want(("maps", B, H, W, s), stages[s], tau, fill) for s in range(nmaps)]
                check_outputs(f"B={B} {H}x{W} nmaps={nmaps} tau={tau} fill={fill}", wants, out, mask, right, kept)
                codes |= set(np.unique(np.concatenate([w[1].ravel() for w in wants])).tolist())
    assert codes <= {0, 1, 2}
    if W >= 63:
        assert codes == {0, 1, 2}, "the inputs should reach every code"


@pytest.mark.parametrize("W", WIDTHS)
def test_ramp_onto_one_column_constant_zero_and_all_nan_rows(dev, hip_lib, W):
    from lwsnet_amd import ops
    d = special_rows(W)
    for tau in (0.0, 1.0):
        for fill in (0, 1):
            out, mask, right, kept = ops.occlusion_check([cu(d, dev)], tau, fill)
            wo, wm, wr, wk = want(("special", W), d, tau, fill)
            check_outputs(f"W={W} tau={tau} fill={fill}", [(wo, wm, wr, wk)], out, mask, right, kept)
            assert wr[0, 0, 0, 0] == W - 1 and not wr[0, 0, 0, 1:].any(), "d = x: the nearest pixel of the row on column 0, nothing else"
            assert wk[0].tolist() == [1 if tau < 1 or W == 1 else 2, W, 0]


@pytest.mark.parametrize("W", [5, 64, 1232, 8189])
def test_addresses_offset_by_one_float_and_in_place(dev, hip_lib, W):
    """Every tensor one float past a 16-byte boundary (the scalar load / store path of an aligned width too), and out[s] == dL[s]."""
    B, H = 2, 3
    stages = stage_maps(B, H, W)[:2]
    n = B * H * W

    def skewed(dtype):
        return torch.empty(n + 4, dtype=dtype, device=dev)[1:1 + n].view(B, 1, H, W)

    for fill in (0, 1):
        dl = [skewed(torch.float32) for _ in stages]
        for t, d in zip(dl, stages):
            t.copy_(cu(d, dev))
            assert t.data_ptr() % 16 == 4
        mask, right = [skewed(torch.uint8) for _ in stages], [skewed(torch.float32) for _ in stages]
        kept = torch.empty((2, B, H), dtype=torch.int32, device=dev)
        raw_call(hip_lib, dev, dl, 0.5, fill, dl, mask, right, kept)          # in place
        wants = [want(("maps", B, H, W, s), stages[s], 0.5, fill) for s in range(2)]
        check_outputs(f"W={W} fill={fill} skewed, in place", wants, dl, mask, right, kept)


@pytest.mark.parametrize("word", G.FLOAT_WORDS + (G.BYTE_WORD,), ids=G.word_id)
@pytest.mark.parametrize("skew", [0, 1], ids=["aligned", "skewed"])
@pytest.mark.parametrize("optional", [True, False], ids=["right+row_kept", "no-optional"])
@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("B,H,W", [(2, 3, 7), (1, 1, 65)])
def test_memory_contract(dev, hip_lib, B, H, W, fill, optional, skew, word):
    """Inputs between poisoned flanks, outputs between poisoned flanks with a poisoned interior: no flank changes, no poison is
    read into a result, and every output element is written."""
    stages = stage_maps(B, H, W)[1:3]
    wants = [want(("maps", B, H, W, s + 1), stages[s], 1.0, fill) for s in range(2)]
    g = G.Guard(dev, word, skew)
    dl = [g.place(d, name=f"dL{s}") for s, d in enumerate(stages)]
    out = [g.empty((B, 1, H, W), name=f"out{s}") for s in range(2)]
    mask = [g.empty((B, 1, H, W), np.uint8, name=f"mask{s}") for s in range(2)]
    right = [g.empty((B, 1, H, W), name=f"right{s}") for s in range(2)] if optional else None
    kept = g.empty((2, B, H), np.int32, name="row_kept") if optional else None
    raw_call(hip_lib, dev, dl, 1.0, fill, out, mask, right, kept)
    check_outputs("guarded", wants, out, mask, right, kept)
    for s, d in enumerate(stages):
        G.assert_bits(dl[s], d, f"dL{s} is an input")
    g.check()


def test_occlusion_check_is_batch_independent(dev, hip_lib):
    from lwsnet_amd import ops
    H, W = 3, 257
    d = sprinkled(2, H, W, 5)
    other = noise(2, H, W, 6)
    alone = ops.occlusion_check([cu(d[1:2], dev)], 0.5, 1)
    batch = ops.occlusion_check([cu(d, dev)], 0.5, 1)
    for k, what in ((0, "out"), (1, "mask"), (2, "right")):
        G.assert_bits(batch[k][0][1:2], host(alone[k][0]), what)
    G.assert_bits(batch[3][:, 1:2], host(alone[3]), "row_kept")
    other[0] = d[1]                                                     # the same image first of two, beside other content, as map 2 of 2
    first = ops.occlusion_check([cu(noise(2, H, W, 7), dev), cu(other, dev)], 0.5, 1)
    for k, what in ((0, "out"), (1, "mask"), (2, "right")):
        G.assert_bits(first[k][1][0:1], host(alone[k][0]), what + " at position 0 of map 1")


def test_graph_capture_replays_the_call(dev, hip_lib):
    from lwsnet_amd import ops
    B, H, W = 2, 3, 1232
    sets = [[sprinkled(B, H, W, 31), noise(B, H, W, 32)], [halves(B, H, W, 33), ramps(B, H, W, 34)]]
    dl = [cu(d, dev) for d in sets[0]]
    out, right = [torch.empty_like(d) for d in dl], [torch.empty_like(d) for d in dl]
    mask = [torch.empty(d.shape, dtype=torch.uint8, device=dev) for d in dl]
    kept = torch.empty((2, B, H), dtype=torch.int32, device=dev)
    raw_call(hip_lib, dev, dl, 1.0, 1, out, mask, right, kept)          # the code object is loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_call(hip_lib, dev, dl, 1.0, 1, out, mask, right, kept)
    for maps in reversed(sets):                                         # new inputs first
        for t, d in zip(dl, maps):
            t.copy_(cu(d, dev))
        for t in out + right + mask + [kept]:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize(dev)
        eo, em, er, ek = ops.occlusion_check([cu(d, dev) for d in maps], 1.0, 1)
        check_outputs("replay against the eager call", [(host(eo[s]), host(em[s]), host(er[s]), host(ek[s])) for s in range(2)],
                      out, mask, right, kept)
        check_outputs("replay against the reference", [R.occlusion_check(d, 1.0, 1) for d in maps], out, mask, right, kept)


def test_forward_occ(dev, model):
    from lwsnet_amd.synth import make_pair
    H, W = 64, 256
    left, right = (a[None] for a in make_pair(H, W, 0)[:2])
    plain = [p.numpy() for p in model(left, right)]
    for tau, fill in ((1.0, True), (0.5, False)):
        res = model.forward_occ(left, right, tau=tau, fill=fill)
        assert type(res).__name__ == "OccResult" and res._fields == ("left", "right", "disp", "mask", "density")
        assert res.density.shape == (4, 1)
        for s in range(4):
            assert type(res.left[s]).__name__ == "DisparityTensor"
            G.assert_bits(res.left[s], plain[s], f"left stage {s + 1}")
            wo, wm, wr, wk = R.occlusion_check(plain[s], tau, fill)
            G.assert_bits(res.disp[s], wo, f"disp stage {s + 1}")
            G.assert_bits(res.mask[s], wm, f"mask stage {s + 1}")
            G.assert_bits(res.right[s], wr, f"right stage {s + 1}")
            assert np.array_equal(res.density[s], wk.sum(axis=1) / float(H * W))
        print(f"forward_occ tau={tau}: density {res.density[:, 0].tolist()}")
        assert 0.0 < res.density.min() and res.density.max() <= 1.0


@pytest.mark.parametrize("occ_fill", [False, True], ids=["unfilled", "occ_fill"])
def test_chain_with_the_occlusion_check(dev, model, occ_fill):
    """run_chain with --occ_check -> speckle filter -> weighted median, and the point cloud of its result, against the same steps
    composed by hand.  Unfilled, the codes reach the median and the point cloud; with --occ_fill the check runs unfilled, the
    speckle filter does the one row fill, and neither takes codes."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.postprocess import Options, run_chain
    from lwsnet_amd.synth import make_pair, to_rgb8
    H, W = 64, 256
    pairs = [make_pair(H, W, seed)[:2] for seed in (0, 1)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    guide = cu(np.stack([to_rgb8(img) for img in left]), dev)
    cam = Camera(721.5, 721.5, 127.5, 31.5, 0.54)
    options = Options.make(occ_check=1.0, occ_fill=occ_fill, speckle=1, speckle_diff=1.0, wmedian=2, wmedian_sigma=10.0, wmedian_fill=0)
    got = run_chain(model, left, right, options, guide)
    occ = model.forward_occ(left, right, tau=1.0, fill=False)
    wlut = ops.wmedian_lut(10.0)
    sp = [ops.speckle_filter(occ.disp[s], 1, 1.0, mask=occ.mask[s], fill=occ_fill) for s in range(4)]
    wm = [ops.wmedian_filter(sp[s].disp, 2, rgb=guide, wlut=wlut, mask=None if occ_fill else sp[s].mask, fill_min=0) for s in range(4)]
    visible = sum(int((host(m) == 1).sum()) for m in occ.mask)
    kept = sum(int((host(r.mask) == 1).sum()) for r in sp)
    print(f"chain: visible {visible}, kept {kept} of {4 * 2 * H * W}")
    assert 0 < kept <= visible < 4 * 2 * H * W, "the check must drop pixels and the chain keep some, or the comparison shows nothing"
    for s in range(4):
        G.assert_bits(got.disp[s], host(wm[s].disp), f"final map, stage {s + 1}")
        G.assert_bits(got.occ_masks[s], host(occ.mask[s]), f"occlusion codes, stage {s + 1}")
        G.assert_bits(got.speckle_masks[s], host(sp[s].mask), f"speckle codes, stage {s + 1}")
    assert got.lr_masks is None and got.lr_density is None
    G.assert_bits(got.occ_density, occ.density, "density")
    G.assert_bits(got.speckle_counts, np.stack([host(r.counts) for r in sp]), "speckle counts")
    G.assert_bits(got.wmedian_counts, np.stack([host(r.counts) for r in wm]), "median counts")
    if occ_fill:
        assert got.keep is None
        keep = None
    else:
        for s in range(4):
            G.assert_bits(got.keep[s], host(sp[s].mask), f"codes kept for geometry, stage {s + 1}")
        keep = got.keep[3]
    points, counts = ops.point_cloud(got.disp[3], cam, keep, guide)
    want_points, want_counts = ops.point_cloud(wm[3].disp, cam, None if occ_fill else sp[3].mask, guide)
    G.assert_bits(counts, host(want_counts), "point count")
    assert int(counts.sum()) > 0
    for b in range(2):
        n = int(counts[b])
        assert torch.equal(points[b, :n].view(torch.uint8), want_points[b, :n].view(torch.uint8)), f"points of image {b}"
