"""lws_objects on the device, bit for bit against the numpy restatement (tests/object_reference.py): random maps at the smallest
shapes that reach each path (one pixel, a last strip of one column, the widest strip with the largest histogram, a cell grid of
more than two tiles with ragged last tiles in both directions, three images), views one element past a 16-byte boundary,
adversarial components across every tile edge, the hand-made cells of tests/test_objects_cpu.py, the road scenes behind ops.ground
and ops.stixels, batch independence, poisoned guard bands, a captured graph, real maps of the model and the inference CLI's files.
The tile of the labelling kernel, T_s strips x T_k bins, is read from its source (test_objects_cpu.tile); the shapes follow."""
import ctypes
import os

import numpy as np
import pytest

import guarded
import object_reference as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, assert_bits, cam_rows, cu, misaligned  # noqa: E402
from test_gpu_ground import ROAD, all_buffers, reference, road_cameras, roads, run_ops, run_raw  # noqa: E402
from test_gpu_stixels import random_maps, raw_stixels, stix_ops  # noqa: E402
from test_objects_cpu import CAM1, OBJ, PATTERNS, pattern, road_objects, second_round_case, tile  # noqa: E402
from test_stixels_cpu import STIX  # noqa: E402

F = np.float32
INF = float("inf")
T_S, T_K = tile()
KEYS = ("rows", "vals", "labels", "info")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def stix_params(p):
    """The stixel call that writes the udisp of the object parameters p (its own thresholds do not reach the histogram)."""
    return dict(min_disp=p["min_disp"], max_depth=p["max_depth"], code_bits=p["code_bits"] & ~0x33, width=p["width"], sub=p["sub"], nbins=p["nbins"],
                tol_bins=1, min_count=8, min_row=2, max_gap=2, layers=1)


def obj_ops(d, cams, codes, udisp, p, dev, labels=True):
    from lwsnet_amd import ops
    t = lambda a: a if isinstance(a, torch.Tensor) else cu(a, dev)              # noqa: E731
    return ops.objects(t(d), cams, t(codes), t(udisp), p["min_disp"], p["max_depth"], p["code_bits"], p["width"], p["sub"], p["min_count"],
                       p["min_pixels"], p["max_objects"], labels=labels)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_objects(lib, dev, b, shape, p):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_objects(P(b["disp"]), P(b["cam"]), P(b["codes"]), P(b["udisp"]), *shape, p["min_disp"], p["max_depth"], p["code_bits"],
                                   p["width"], p["sub"], p["nbins"], p["min_count"], p["min_pixels"], p["max_objects"], P(b["work"]), P(b["rows"]),
                                   P(b["vals"]), P(b.get("labels")), P(b["info"]), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "lws_objects")


def check(got, want, what, labels=True):
    for g, w, key in zip(got, want, KEYS):
        if key == "labels" and not labels:
            assert g is None
        else:
            assert_bits(g, w, f"{what} {key}")


def workspace(lib, dev, B, W, p):
    nbytes = int(lib.lws_objects_workspace(B, W, p["width"], p["nbins"]))
    assert nbytes > 0
    return torch.empty((nbytes,), dtype=torch.uint8, device=dev)


def summary(want):
    info = want[3]
    return f"info {info.tolist()}, {int((want[2] >= 0).sum())} labelled pixels"


# ---- random maps ----
@pytest.mark.parametrize("B,H,W,width,sub,nbins,min_disp,min_count,min_pixels,max_objects,code_bits", [
    (1, 1, 1, 1, 4, 1, 1.0, 1, 1, 2, 1 << 2),                                   # one pixel, one bin: nothing can take part
    (2, 60, 13, 4, 4, 70, 1.0, 3, 12, 5, 1 << 2),                               # the last strip is one column
    (1, 24, 130, 64, 16, 4096, 1.0, 2, 10, 16, (1 << 2) | (1 << 3)),            # the widest strip, the largest histogram, a last strip of 2 columns
    (1, 40, 3 * (2 * T_S + 3) - 1, 3, 2, 2 * T_K + 22, 1.0, 2, 9, 300, 0x3f),   # S = 2 T_s + 3, nbins = 2 T_k + 22: 3 x 3 tiles, the last ones ragged
    (3, 37, 61, 7, 1, 70, 0.01, 2, 8, 4, (1 << 2) | (1 << 1))])                 # three images; more kept components than slots
def test_random_maps_bitexact(dev, hip_lib, B, H, W, width, sub, nbins, min_disp, min_count, min_pixels, max_objects, code_bits):
    """udisp comes from ops.stixels(udisp=True) where its code_bits are allowed there, else from the restatement."""
    d, codes, height = random_maps(B, H, W, sub, nbins, 7 * H + W + nbins + code_bits)
    cams = road_cameras(B)
    rows = cam_rows(cams)
    p = dict(min_disp=min_disp, max_depth=INF, code_bits=code_bits, width=width, sub=sub, nbins=nbins, min_count=min_count, min_pixels=min_pixels,
             max_objects=max_objects)
    udisp = O.udisp_of(d, rows, codes, p)
    if not code_bits & 0x33:
        u_dev = stix_ops(d, cams, codes, height, stix_params(p), dev).udisp
        assert_bits(u_dev, udisp, "udisp")
    want = O.run(d, rows, codes, udisp, p)
    what = f"B={B} {H}x{W} width={width} sub={sub} nbins={nbins} bits={code_bits}"
    print(f"{what}: {summary(want)}")
    if H * W > 16:                                          # at least one kept object and one dropped component, in every image
        assert (want[3][:, 2] >= 1).all() and (want[3][:, 1] > want[3][:, 2]).all() and (want[2] >= 0).any()
    for labels in (True, False):
        check(obj_ops(d, cams, codes, udisp, p, dev, labels), want, what, labels)
    # every buffer a view one element past a 16-byte boundary, the outputs included (the workspace is 16-byte aligned by contract)
    b = dict(disp=misaligned(d, dev), cam=misaligned(rows, dev), codes=misaligned(codes, dev), udisp=misaligned(udisp, dev),
             work=workspace(hip_lib, dev, B, W, p), rows=misaligned(np.full((B, max_objects, 8), 77, np.int32), dev),
             vals=misaligned(np.full((B, max_objects, 8), 7.0, F), dev), labels=misaligned(np.full((B, 1, H, W), 77, np.int32), dev),
             info=misaligned(np.full((B, 4), 77, np.int32), dev))
    raw_objects(hip_lib, dev, b, (B, H, W), p)
    check([b[k] for k in KEYS], want, "misaligned " + what)


# ---- adversarial components: S = 2 T_s + 3 strips of 3 columns, 2 T_k + 22 bins, one row of a strip per cell ----
ADV_S, ADV_K = 2 * T_S + 3, 2 * T_K + 22
ADV = dict(min_disp=0.25, max_depth=INF, code_bits=1 << 2, width=3, sub=1, nbins=ADV_K, min_count=3, min_pixels=3, max_objects=ADV_K)


def staircase():
    """A slanted wall: one cell per strip, the bin one up or down per strip (bouncing between the first and the last bin), so that
    the cells are joined only diagonally, from the first to the last strip across every tile edge."""
    cells, k, step = {}, 5, 1
    for s in range(ADV_S):
        cells[(s, k)] = 3
        if not 0 <= k + step < ADV_K:
            step = -step
        k += step
    return cells


def serpentine():
    """Every fourth bin filled over all strips, the runs joined in turn at the grid's right and left border: one component whose
    unions chain through every tile in both directions."""
    cells = {}
    for i, k in enumerate(range(1, ADV_K, 4)):
        for s in range(ADV_S):
            cells[(s, k)] = 3
        if k + 4 < ADV_K:
            s = ADV_S - 1 if i % 2 == 0 else 0
            for kk in (k + 1, k + 2, k + 3):
                cells[(s, kk)] = 3
    return cells


def checkerboard():
    return {(s, k): 3 for s in range(ADV_S) for k in range(ADV_K) if (s + k) % 2 == 0}


def bin_rows():
    return {(s, k): 3 for s in range(ADV_S) for k in range(0, ADV_K, 2)}


ADVERSARIAL = {"staircase": (staircase, 1), "serpentine": (serpentine, 1), "checkerboard": (checkerboard, 1), "bin_rows": (bin_rows, ADV_K // 2)}


@pytest.mark.parametrize("name", sorted(ADVERSARIAL))
def test_adversarial_components(dev, hip_lib, name):
    make, components = ADVERSARIAL[name]
    cells = make()
    H = max(sum(1 for (s, _) in cells if s == strip) for strip in range(ADV_S))   # one row per cell: cells per strip * min_count / width
    assert H <= ADV_K
    p, cam = ADV, CAM1
    d, codes = O.cell_map(H, 3 * ADV_S, 3, 1, cells)
    udisp = O.udisp_of(d, cam, codes, p)
    want = O.run(d, cam, codes, udisp, p)
    print(f"{name}: {H} rows, {len(cells)} cells, {summary(want)}")
    assert want[3][0].tolist() == [len(cells), components, components, int(sum(cells.values()))]
    from lwsnet_amd.geometry import Camera
    check(obj_ops(d, [Camera(100.0, 100.0, 7.5, 15.5, 0.5)], codes, udisp, p, dev), want, name)


# ---- the hand-made cells of the CPU test ----
@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_hand_made_cells(dev, hip_lib, name):
    from lwsnet_amd.geometry import Camera
    d, codes, udisp, p, want_rows, want_info = pattern(name)
    want = O.run(d, CAM1, codes, udisp, p)
    assert want[3][0].tolist() == want_info and want[0][0, :len(want_rows)].tolist() == want_rows
    check(obj_ops(d, [Camera(100.0, 100.0, 7.5, 15.5, 0.5)], codes, udisp, p, dev), want, name)


def test_numbering_scan_second_round(dev, hip_lib):
    """S * nbins = 524 352 cells: the per-image scan of the numbering goes round twice, and kept roots stand in the first block,
    in the last block of round one, in the first block of round two and in the last cell."""
    from lwsnet_amd.geometry import Camera
    d, codes, udisp, p, want_rows, want_info = second_round_case()
    want = O.run(d, CAM1, codes, udisp, p)
    assert want[3][0].tolist() == want_info and want[0][0, :len(want_rows)].tolist() == want_rows
    check(obj_ops(d, [Camera(100.0, 100.0, 7.5, 15.5, 0.5)], codes, udisp, p, dev), want, "second round")


def test_a_foreign_udisp_is_followed_as_it_is(dev, hip_lib):
    """The call is a pure function of its inputs: a histogram that is not the map's own -- a bridge cell no pixel stands in, a cell
    emptied under its pixels, and random counts over a random map -- gives what the restatement gives."""
    from lwsnet_amd.geometry import Camera
    d, codes, udisp, p, _, _ = pattern("two_apart")
    udisp[0, 1, 6], udisp[0, 1, 7] = 9, 0
    want = O.run(d, CAM1, codes, udisp, p)
    assert want[3][0].tolist() == [2, 1, 1, 4]
    check(obj_ops(d, [Camera(100.0, 100.0, 7.5, 15.5, 0.5)], codes, udisp, p, dev), want, "bridge")
    B, H, W = 2, 30, 50
    d, codes, _ = random_maps(B, H, W, 2, 40, 5)
    p = dict(min_disp=1.0, max_depth=INF, code_bits=0x3f, width=5, sub=2, nbins=40, min_count=3, min_pixels=4, max_objects=32)
    udisp = np.random.default_rng(6).integers(0, 6, (B, 10, 40)).astype(np.uint32)
    cams = road_cameras(B)
    want = O.run(d, cam_rows(cams), codes, udisp, p)
    print(f"random counts: {summary(want)}")
    assert (want[3][:, 2] >= 1).all() and (want[3][:, 1] > want[3][:, 2]).all()
    check(obj_ops(d, cams, codes, udisp, p, dev), want, "random counts")


# ---- the road scenes ----
def ground_stixels_objects(d, mask, cams, dev, labels=True):
    """ops.ground with ROAD, ops.stixels with STIX on its codes and heights, ops.objects with OBJ on the histogram."""
    g = run_ops(d, mask, cams, ROAD, dev)
    st = stix_ops(d, cams, g.codes, g.height, STIX, dev)
    return g, st, obj_ops(d, cams, g.codes, st.udisp, OBJ, dev, labels)


def test_road_scenes_and_batch_independence(dev, hip_lib):
    B = 2
    d, mask, cams = roads(B, 31)
    g, st, got = ground_stixels_objects(d, mask, cams, dev)
    assert g.info[:, 0].cpu().tolist() == [0, 0]
    want = O.run(d, cam_rows(cams), g.codes.cpu().numpy(), st.udisp.cpu().numpy(), OBJ)
    print(f"roads: {summary(want)}")
    assert (want[3][:, 2] >= 3).all()
    check(got, want, "roads")
    check(ground_stixels_objects(d, mask, cams, dev, labels=False)[2], want, "roads without labels", labels=False)

    def same(res, b, rb, what):
        for a, r, key in zip(res, got, KEYS):
            assert np.array_equal(guarded.as_bits(a[b].cpu().numpy()), guarded.as_bits(r[rb].cpu().numpy())), f"{what} {key}"

    for b in range(B):
        same(ground_stixels_objects(d[b:b + 1], mask[b:b + 1], [cams[b]], dev)[2], 0, b, f"image {b} alone")
    d2, m2, _ = roads(B, 32)
    d2[0], m2[0] = d[1], mask[1]
    same(ground_stixels_objects(d2, m2, [cams[1], cams[1]], dev)[2], 0, 1, "image 1 moved to the front")


def test_clean_road_scene_matches_the_cpu_expectation(dev, hip_lib):
    """The scene the CPU test describes (three boxes at 5, 7 and 11 m), its restatement computed there."""
    from test_stixels_cpu import CAM
    s, rows, vals, labels, info = road_objects(1.4)
    got = obj_ops(s["d"], [CAM], s["codes"], s["udisp"][None], OBJ, dev)
    check(got, (rows[None], vals[None], labels[None, None], info[None]), "clean road")


# ---- the memory contract ----
@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Inputs, outputs and the workspace between poisoned flanks, the outputs and the workspace poisoned inside: nothing outside
    them changes and every element the header promises is written -- the empty slots and the -1 labels included.  Strips of 7
    columns: the last holds 6."""
    B = 2
    d, mask, cams = roads(B, 8)
    H, W = d.shape[2:]
    rows = cam_rows(cams)
    ground = reference(d, mask, rows, ROAD)
    p = {**OBJ, "width": 7, "min_count": 7}
    udisp = O.udisp_of(d, rows, ground["codes"], p)
    want = O.run(d, rows, ground["codes"], udisp, p)
    assert (want[0][..., 0] == 0).any() and (want[3][:, 2] >= 1).all() and (want[2] < 0).any() and (want[2] >= 0).any()
    nbytes = int(hip_lib.lws_objects_workspace(B, W, p["width"], p["nbins"]))
    g = guarded.Guard(dev, word, skew=1)
    b = dict(disp=g.place(d, name="disp"), cam=g.place(rows, name="cam"), codes=g.place(ground["codes"], name="codes"),
             udisp=g.place(udisp, name="udisp"), work=g.empty((nbytes,), np.uint8, align16=True, word=g.word, name="workspace"),
             rows=g.empty((B, p["max_objects"], 8), np.int32, name="rows"), vals=g.empty((B, p["max_objects"], 8), F, name="vals"),
             labels=g.empty((B, 1, H, W), np.int32, name="labels"), info=g.empty((B, 4), np.int32, name="info"))
    raw_objects(hip_lib, dev, b, (B, H, W), p)
    for key, w in zip(KEYS, want):
        guarded.assert_bits(b[key], w, f"guarded {key}")
    g.check()


# ---- a captured graph ----
def test_graph_capture_replays_ground_stixels_and_objects(dev, hip_lib):
    B = 2
    first, second = roads(B, 41), roads(B, 42, plain=True)
    H, W = first[0].shape[2:]
    rows = cam_rows(first[2])
    S = -(-W // STIX["width"])
    b = all_buffers(dev, hip_lib, B, H, W, ROAD, first[0], first[1], rows)
    stix = dict(b, rows=torch.empty((B, S, STIX["layers"], 4), dtype=torch.int32, device=dev),
                vals=torch.empty((B, S, STIX["layers"], 4), dtype=torch.float32, device=dev),
                udisp=torch.empty((B, S, STIX["nbins"]), dtype=torch.uint32, device=dev))
    obj = dict(disp=b["disp"], cam=b["cam"], codes=b["codes"], udisp=stix["udisp"], work=workspace(hip_lib, dev, B, W, OBJ),
               rows=torch.empty((B, OBJ["max_objects"], 8), dtype=torch.int32, device=dev),
               vals=torch.empty((B, OBJ["max_objects"], 8), dtype=torch.float32, device=dev),
               labels=torch.empty((B, 1, H, W), dtype=torch.int32, device=dev), info=torch.empty((B, 4), dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                           # one stream: the capture stream
        run_raw(hip_lib, dev, b, (B, H, W), ROAD)
        raw_stixels(hip_lib, dev, stix, (B, H, W), STIX)
        raw_objects(hip_lib, dev, obj, (B, H, W), OBJ)
    for d_np, m_np, _ in (first, second):
        b["disp"].copy_(cu(d_np, dev))
        b["mask"].copy_(cu(m_np, dev))
        graph.replay()
        torch.cuda.synchronize(dev)
        ground = reference(d_np, m_np, rows, ROAD)
        want = O.run(d_np, rows, ground["codes"], O.udisp_of(d_np, rows, ground["codes"], OBJ), OBJ)
        assert (want[3][:, 2] >= 1).all()
        check([obj[k] for k in KEYS], want, "replay")


# ---- real maps ----
def test_objects_of_model_maps(dev, model):
    """The seeded model at 64 x 256 behind forward_occ, each stage through ops.ground, ops.stixels and ops.objects with their defaults
    but min_pixels (16: the maps of random weights hold small blobs only) -- bit-equal whatever the maps hold."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from lwsnet_amd.synth import make_pair
    H, W = 64, 256
    left, right = (a[None] for a in make_pair(H, W, 0)[:2])
    cams = [Camera(721.5, 721.5, 127.5, 31.5, 0.54)]
    res = model.forward_occ(left, right, tau=1.0, fill=False)
    p = dict(min_disp=1.0, max_depth=INF, code_bits=1 << 2, width=8, sub=4, nbins=768, min_count=8, min_pixels=16, max_objects=256)
    for s in range(4):
        g = ops.ground(res.disp[s], cams, res.mask[s])
        st = ops.stixels(res.disp[s], cams, g.codes, g.height, udisp=True)
        got = ops.objects(res.disp[s], cams, g.codes, st.udisp, min_pixels=16)         # the other defaults are these parameters
        want = O.run(res.disp[s].numpy(), cam_rows(cams), g.codes.cpu().numpy(), st.udisp.cpu().numpy(), p)
        print(f"forward_occ stage {s + 1}: {summary(want)}")
        check(got, want, f"forward_occ stage {s + 1}")


def test_inference_cli_object_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, outputs, synth
    from lwsnet_amd.geometry import Camera
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, 1)
    calib = tmp_path / "000000.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    out = tmp_path / "out"
    written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path",
                              str(out), "--save_objects", "--object_min_pixels", "16"])
    stem = "000000_10"
    assert sorted(os.listdir(out)) == sorted(stem + s for s in (".png", "_occ.png", "_objects.png", "_objects.csv"))
    assert len(written) == 4
    full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
    left = io.crop_bottom_right(full)
    l_in = io.to_input(left)[None]
    r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
    cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
    res = model.forward_occ(l_in, r_in, tau=1.0, fill=False)
    g = ops.ground(res.disp[3], cam, res.mask[3])
    st = ops.stixels(res.disp[3], cam, g.codes, g.height, udisp=True)
    ob = ops.objects(res.disp[3], cam, g.codes, st.udisp, min_pixels=16)
    rows, vals, labels = ob.rows[0].cpu().numpy(), ob.vals[0].cpu().numpy(), ob.labels[0, 0].cpu().numpy()
    assert np.array_equal(np.asarray(Image.open(out / (stem + "_objects.png"))), outputs.objects_to_rgb(rows, labels, left))
    assert (out / (stem + "_objects.csv")).read_text() == outputs.objects_to_csv(rows, vals)
