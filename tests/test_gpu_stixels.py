"""lws_stixels on the device, bit for bit against the numpy restatement (tests/stixel_reference.py): random maps at the smallest
shapes that reach each path (a last strip of one column, more rows than threads, the widest strip and the largest histogram, strips
that straddle quads), views one element past a 16-byte boundary, the hand-made columns of tests/test_stixels_cpu.py, the road
scenes behind ops.ground, batch independence, poisoned guard bands, a captured graph, real maps of the model and the inference
CLI's files."""
import ctypes
import os

import numpy as np
import pytest

import guarded
import stixel_reference as X

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, assert_bits, cam_rows, cu, misaligned  # noqa: E402
from test_gpu_ground import ROAD, SPECIAL, all_buffers, reference, road_cameras, roads, run_ops, run_raw  # noqa: E402
from test_stixels_cpu import COL, HAND_MADE, STIX, hole_map  # noqa: E402

F = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def ref(d, rows, codes, height, p):
    return X.stixels(d, rows, codes, height, p["min_disp"], p["max_depth"], p["code_bits"], p["width"], p["sub"], p["nbins"], p["tol_bins"],
                     p["min_count"], p["min_row"], p["max_gap"], p["layers"])


def stix_ops(d, cams, codes, height, p, dev, udisp=True):
    from lwsnet_amd import ops
    t = lambda a: a if isinstance(a, torch.Tensor) else cu(a, dev)              # noqa: E731
    return ops.stixels(t(d), cams, t(codes), t(height), p["min_disp"], p["max_depth"], p["code_bits"], p["width"], sub=p["sub"], nbins=p["nbins"],
                       tol_bins=p["tol_bins"], min_count=p["min_count"], min_row=p["min_row"], max_gap=p["max_gap"], layers=p["layers"],
                       udisp=udisp)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_stixels(lib, dev, b, shape, p):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_stixels(P(b["disp"]), P(b["cam"]), P(b["codes"]), P(b["height"]), *shape, p["min_disp"], p["max_depth"], p["code_bits"],
                                   p["width"], p["sub"], p["nbins"], p["tol_bins"], p["min_count"], p["min_row"], p["max_gap"], p["layers"],
                                   P(b["rows"]), P(b["vals"]), P(b.get("udisp")), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "lws_stixels")


def check(got, want, what, udisp=True):
    assert_bits(got[0], want[0], f"{what} rows")
    assert_bits(got[1], want[1], f"{what} vals")
    if udisp:
        assert_bits(got[2], want[2], f"{what} udisp")
    else:
        assert got[2] is None


# ---- random maps ----
def random_maps(B, H, W, sub, nbins, seed):
    """Disparities up to a fifth past the last bin -- half of them uniform, half near three values per image, so that bins fill,
    rows hold several members and counts tie -- with the specials planted; codes drawn from {0..5, 6, 255} independently of the
    disparities; heights of either sign."""
    rng = np.random.default_rng(seed)
    top = nbins / sub
    near = (rng.random((B, 1, 1, 3)) * top).astype(F)
    pick = np.take_along_axis(np.broadcast_to(near, (B, 1, H, 3)), rng.integers(0, 3, (B, 1, H, W)), axis=3)
    d = np.where(rng.random((B, 1, H, W)) < 0.5, pick + (rng.random((B, 1, H, W)) * (1.5 / sub)).astype(F),
                 (rng.random((B, 1, H, W)) * 1.2 * top).astype(F)).astype(F)
    flat = d.reshape(-1)
    idx = rng.choice(flat.size, size=max(1, flat.size // 20), replace=False)
    flat[idx] = np.concatenate([SPECIAL, [F(top), np.nextafter(F(top), F(0))]]).astype(F)[np.arange(len(idx)) % (len(SPECIAL) + 2)]
    codes = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 255, 2, 2, 3, 2], np.uint8), size=d.shape)
    height = (rng.random(d.shape) * 4.0 - 1.0).astype(F)
    return d, codes, height


@pytest.mark.parametrize("code_bits", [1 << 2, (1 << 2) | (1 << 3)])
@pytest.mark.parametrize("B,H,W,width,sub,nbins,tol_bins,layers,min_disp,counts", [
    (1, 1, 1, 1, 4, 1, 0, 1, 1.0, (1, 1, 0)),               # one pixel, one bin: nothing can take part
    (2, 300, 13, 4, 4, 70, 1, 2, 1.0, (12, 1, 3)),          # the last strip is one column; more rows than threads
    (1, 5, 130, 64, 16, 4096, 8, 4, 1.0, (6, 3, 1)),        # the widest strip, the largest histogram, a last strip of 2 columns
    (3, 37, 61, 7, 1, 70, 2, 4, 1.0, (10, 2, 2)),           # strips straddle quads
    (2, 3, 5, 3, 3, 1, 0, 1, 0.01, (2, 1, 0))])
def test_random_maps_bitexact(dev, hip_lib, B, H, W, width, sub, nbins, tol_bins, layers, min_disp, counts, code_bits):
    d, codes, height = random_maps(B, H, W, sub, nbins, 7 * H + W + nbins + code_bits)
    cams = road_cameras(B)
    rows = cam_rows(cams)
    p = dict(min_disp=min_disp, max_depth=INF, code_bits=code_bits, width=width, sub=sub, nbins=nbins, tol_bins=tol_bins, min_count=counts[0],
             min_row=counts[1], max_gap=counts[2], layers=layers)
    want = ref(d, rows, codes, height, p)
    what = f"B={B} {H}x{W} width={width} sub={sub} nbins={nbins} bits={code_bits}"
    found = want[0][..., 0] > 0
    print(f"{what}: {found.sum(axis=(0, 1)).tolist()} stixels per layer, {int((want[0][..., 3] >= 0).sum() - found.sum())} holes, "
          f"{int(want[2].sum())} of {d.size} pixels take part")
    if H * W > 16:
        assert found.any() and 0 < want[2].sum() < d.size
    for udisp in (True, False):
        check(stix_ops(d, cams, codes, height, p, dev, udisp), want, what, udisp)
        # every buffer a view one element past a 16-byte boundary, the outputs included
        S = -(-W // width)
        b = dict(disp=misaligned(d, dev), cam=misaligned(rows, dev), codes=misaligned(codes, dev), height=misaligned(height, dev),
                 rows=misaligned(np.full((B, S, layers, 4), 77, np.int32), dev), vals=misaligned(np.full((B, S, layers, 4), 7.0, F), dev),
                 udisp=misaligned(np.full((B, S, nbins), 77, np.uint32), dev) if udisp else None)
        raw_stixels(hip_lib, dev, b, (B, H, W), p)
        check((b["rows"], b["vals"], b["udisp"]), want, "misaligned " + what, udisp)


# ---- the hand-made columns of the CPU test ----
def hand_camera():
    from lwsnet_amd.geometry import Camera
    return [Camera(100.0, 100.0, 7.5, 15.5, 0.5)]           # fb = 50: CAM1 of the CPU test


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made_columns(dev, hip_lib, name):
    kw, want_rows = HAND_MADE[name]
    kw = dict(kw)
    p = {**COL, **{k: v for k, v in kw.items() if k != "strips"}}
    d, codes, height = X.column_map(32, 16, p["width"], kw["strips"])
    cams = hand_camera()
    want = ref(d, cam_rows(cams), codes, height, p)
    for s, slots in want_rows.items():
        assert want[0][0, s].tolist() == slots
    check(stix_ops(d, cams, codes, height, p, dev), want, name)


def test_hole_then_a_real_layer(dev, hip_lib):
    d, codes, height = hole_map()
    cams = hand_camera()
    for min_row, slots in ((2, [[0, -1, -1, 12], [12, 14, 19, 6]]), (1, [[8, 0, 7, 12], [12, 14, 19, 6]])):
        p = {**COL, "min_row": min_row}
        want = ref(d, cam_rows(cams), codes, height, p)
        assert want[0][0, 3].tolist() == slots
        check(stix_ops(d, cams, codes, height, p, dev), want, f"hole min_row={min_row}")


# ---- the road scenes ----
def ground_then_stixels(d, mask, cams, dev, p=STIX):
    """ops.ground with ROAD, then ops.stixels on its codes and heights -> (GroundResult, StixelResult)."""
    g = run_ops(d, mask, cams, ROAD, dev)
    return g, stix_ops(d, cams, g.codes, g.height, p, dev)


def test_road_scenes_and_batch_independence(dev, hip_lib):
    B = 2
    d, mask, cams = roads(B, 31)
    g, got = ground_then_stixels(d, mask, cams, dev)
    assert g.info[:, 0].cpu().tolist() == [0, 0]
    codes, height = g.codes.cpu().numpy(), g.height.cpu().numpy()
    ground = reference(d, mask, cam_rows(cams), ROAD)
    assert_bits(g.codes, ground["codes"], "road codes")
    assert_bits(g.height, ground["height"], "road height")
    want = ref(d, cam_rows(cams), codes, height, STIX)
    found = want[0][..., 0] > 0
    print(f"roads: {found.sum(axis=1).tolist()} stixels per image and layer")
    assert (found[:, :, 0].sum(axis=1) >= 8).all() and found[:, :, 1].any()
    check(got, want, "roads")

    def same(res, b, rb, what):
        for a, r, key in zip(res, got, ("rows", "vals", "udisp")):
            assert np.array_equal(guarded.as_bits(a[b].cpu().numpy()), guarded.as_bits(r[rb].cpu().numpy())), f"{what} {key}"

    for b in range(B):
        same(ground_then_stixels(d[b:b + 1], mask[b:b + 1], [cams[b]], dev)[1], 0, b, f"image {b} alone")
    d2, m2, _ = roads(B, 32)
    d2[0], m2[0] = d[1], mask[1]
    same(ground_then_stixels(d2, m2, [cams[1], cams[1]], dev)[1], 0, 1, "image 1 moved to the front")


# ---- the memory contract ----
@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Inputs and outputs between poisoned flanks, the outputs poisoned inside: nothing outside the outputs changes and every element
    the header promises is written -- empty slots and the histogram's zero bins included.  Strips of 7 columns: the last holds 6."""
    B = 2
    d, mask, cams = roads(B, 8)
    H, W = d.shape[2:]
    rows = cam_rows(cams)
    ground = reference(d, mask, rows, ROAD)
    p = {**STIX, "width": 7}
    want = ref(d, rows, ground["codes"], ground["height"], p)
    assert (want[0][..., 0] == 0).any() and (want[0][..., 0] > 0).any() and (want[2] == 0).any()
    S = -(-W // p["width"])
    g = guarded.Guard(dev, word, skew=1)
    b = dict(disp=g.place(d, name="disp"), cam=g.place(rows, name="cam"), codes=g.place(ground["codes"], name="codes"),
             height=g.place(ground["height"], name="height"), rows=g.empty((B, S, p["layers"], 4), np.int32, name="rows"),
             vals=g.empty((B, S, p["layers"], 4), F, name="vals"), udisp=g.empty((B, S, p["nbins"]), np.uint32, name="udisp"))
    raw_stixels(hip_lib, dev, b, (B, H, W), p)
    for key, w in zip(("rows", "vals", "udisp"), want):
        guarded.assert_bits(b[key], w, f"guarded {key}")
    g.check()


# ---- a captured graph ----
def test_graph_capture_replays_ground_and_stixels(dev, hip_lib):
    B = 2
    first, second = roads(B, 41), roads(B, 42, plain=True)
    H, W = first[0].shape[2:]
    rows = cam_rows(first[2])
    S = -(-W // STIX["width"])
    b = all_buffers(dev, hip_lib, B, H, W, ROAD, first[0], first[1], rows)
    b.update(rows=torch.empty((B, S, STIX["layers"], 4), dtype=torch.int32, device=dev),
             vals=torch.empty((B, S, STIX["layers"], 4), dtype=torch.float32, device=dev),
             udisp=torch.empty((B, S, STIX["nbins"]), dtype=torch.uint32, device=dev))
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream: the capture stream
        run_raw(hip_lib, dev, b, (B, H, W), ROAD)
        raw_stixels(hip_lib, dev, b, (B, H, W), STIX)
    for d_np, m_np, _ in (first, second):
        b["disp"].copy_(cu(d_np, dev))
        b["mask"].copy_(cu(m_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        ground = reference(d_np, m_np, rows, ROAD)
        want = ref(d_np, rows, ground["codes"], ground["height"], STIX)
        assert (want[0][..., 0] > 0).any()
        check((b["rows"], b["vals"], b["udisp"]), want, "replay")


# ---- real maps ----
def test_stixels_of_model_maps(dev, model):
    """The seeded model at 64 x 256 behind forward_occ, each stage through ops.ground and ops.stixels with their defaults -- bit-equal
    whatever the maps hold."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.synth import make_pair
    H, W = 64, 256
    left, right = (a[None] for a in make_pair(H, W, 0)[:2])
    cams = [Camera(721.5, 721.5, 127.5, 31.5, 0.54)]
    res = model.forward_occ(left, right, tau=1.0, fill=False)
    p = dict(min_disp=1.0, max_depth=INF, code_bits=1 << 2, width=8, sub=4, nbins=768, tol_bins=1, min_count=16, min_row=4, max_gap=2, layers=2)
    for s in range(4):
        g = ops.ground(res.disp[s], cams, res.mask[s])
        got = ops.stixels(res.disp[s], cams, g.codes, g.height, udisp=True)     # the defaults are these parameters
        want = ref(res.disp[s].numpy(), cam_rows(cams), g.codes.cpu().numpy(), g.height.cpu().numpy(), p)
        print(f"forward_occ stage {s + 1}: {(want[0][..., 0] > 0).sum(axis=(0, 1)).tolist()} stixels per layer, {int(want[2].sum())} pixels take part")
        check(got, want, f"forward_occ stage {s + 1}")


def test_inference_cli_stixel_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, synth
    from lwsnet_amd.geometry import Camera
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, 1)
    calib = tmp_path / "000000.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    out = tmp_path / "out"
    written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path",
                              str(out), "--save_stixels", "--stixel_width", "16", "--stixel_layers", "3"])
    stem = "000000_10"
    assert sorted(os.listdir(out)) == sorted(stem + s for s in (".png", "_occ.png", "_stixels.png", "_stixels.csv"))
    assert len(written) == 4
    full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
    left = io.crop_bottom_right(full)
    l_in = io.to_input(left)[None]
    r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
    cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
    res = model.forward_occ(l_in, r_in, tau=1.0, fill=False)
    g = ops.ground(res.disp[3], cam, res.mask[3])
    st = ops.stixels(res.disp[3], cam, g.codes, g.height, width=16, layers=3)
    rows, vals = st.rows[0].cpu().numpy(), st.vals[0].cpu().numpy()
    assert rows.shape == (77, 3, 4)
    assert np.array_equal(np.asarray(Image.open(out / (stem + "_stixels.png"))),
                          inference.stixels_to_rgb(rows, vals, left, 16, inference.STIXEL_COLOUR_DEPTH))
    assert (out / (stem + "_stixels.csv")).read_text() == inference.stixels_to_csv(rows, vals, 16, left.shape[1])
