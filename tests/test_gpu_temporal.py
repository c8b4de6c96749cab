"""lws_temporal_step on the device, bit for bit against the numpy restatement (tests/temporal_reference.py).  Rows interact here --
the four taps of the previous state and the target of the hold lie in other rows -- so the shapes start at one and two rows; the
widths are one pixel, the quad and its neighbours, the 64-lane wave and its neighbours, more than one workgroup per row, and the
workload's 1232.  Five motions (identity, forward, backward: the image shrinks and many sources land on one target, a yaw with a
lateral step, a turn that takes most of the scene out of view) meet five kinds of input (the scene, uniform noise, maps sprinkled
with NaN, +-inf, -0.0 and 1e30, integer and half-integer disparities, a constant map whose z-buffer ties the source index decides)
with sigma and mask given or not and hold off and on; together they reach every code.  Then: views one element past a 16-byte
boundary, poisoned guard bands, batch independence, a captured graph, TemporalFilter, the chain in front of it, and the CLI."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import guarded
import temporal_reference as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import KITTI15_CALIB, cam_rows, cu, misaligned  # noqa: E402

F = np.float32
HS, WS, BS = (1, 2, 5, 17), (1, 3, 4, 5, 63, 64, 65, 257, 1232), (1, 2)
KINDS = ("scene", "uniform", "special", "halves", "constant")
# camera-to-world pose of the second frame (the first is the identity): dz, yaw, dx
MOTIONS = {"identity": (0.0, 0.0, 0.0), "forward": (0.5, 0.0, 0.0), "backward": (-6.0, 0.0, 0.0), "yaw_and_step": (0.3, 0.05, 0.2),
           "out_of_view": (0.2, 0.6, 3.0)}
PARAMS = dict(sigma0=0.5, min_disp=0.5, sigma_min=0.05, gate=3.0, q=0.01, max_jump=1.0, q_hold=0.05, max_var=4.0)
KEYS = ("D", "V", "A", "code", "counts")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


def camera(H, W):
    """A camera for an H x W view of the scene: the wall fills the middle, the road the rows below the principal point."""
    from lwsnet_amd.geometry import Camera
    return Camera(max(1.25 * W, 8.0), max(1.25 * W, 8.0), (W - 1) / 2.0, 0.4 * (H - 1), 0.5)


def frame(kind, H, W, cam, pose, rng):
    """One [H,W] float32 map of `kind` seen from the camera-to-world `pose`."""
    truth = T.render(pose, H, W, tuple(float(v) for v in cam.row()))
    if kind == "scene":
        return np.where(truth > 0, truth + rng.normal(0, 0.2, truth.shape), 0).astype(F)
    if kind == "uniform":
        return rng.uniform(0.3, 40.0, (H, W)).astype(F)
    if kind == "halves":
        return (np.rint(rng.uniform(1.0, 12.0, (H, W)) * 2) / 2).astype(F)
    if kind == "constant":
        return np.full((H, W), 8.0, F)
    m = np.where(truth > 0, truth + rng.normal(0, 0.2, truth.shape), 0).astype(F).reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 1e30, -3.0], F)
    idx = rng.choice(m.size, size=max(1, m.size // 6), replace=False)
    m[idx] = special[np.arange(len(idx)) % len(special)]
    return m.reshape(H, W)


def two_frames(H, W, B, motion, kind, seed):
    """(cams, the first maps, the second maps with holes, sigma of both, mask of the second, pose [B,2,12]): image b moves by the
    motion b places behind `motion` in MOTIONS, so the images of a batch differ in pose as well."""
    rng = np.random.default_rng(seed)
    cams = [camera(H, W)] * B
    names = list(MOTIONS)
    m0, m1, pose = np.empty((B, 1, H, W), F), np.empty((B, 1, H, W), F), np.empty((B, 2, 12), F)
    for b in range(B):
        dz, yaw, dx = MOTIONS[names[(names.index(motion) + b) % len(names)]]
        T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, dz, yaw, dx)
        m0[b, 0], m1[b, 0] = frame(kind, H, W, cams[b], T0, rng), frame(kind, H, W, cams[b], T1, rng)
        pose[b] = T.relative(T0, T1)
    m1[rng.random(m1.shape) < 0.2] = np.nan                 # what a check dropped: the hold's pixels
    sigma = [rng.uniform(0.0, 1.0, m0.shape).astype(F) for _ in range(2)]
    sigma[1].reshape(-1)[::11] = np.nan
    sigma[1].reshape(-1)[5::13] = -0.25
    mask = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=m1.shape)
    return cams, m0, m1, sigma, mask, pose


def step_ops(dev, m, cams, pose, prev, sigma, mask, counts=True, **kw):
    from lwsnet_amd import ops
    t = lambda a: None if a is None else a if isinstance(a, torch.Tensor) else cu(a, dev)     # noqa: E731
    return ops.temporal_step(t(m), cams, pose=pose, prev=None if prev is None else tuple(t(a) for a in prev), sigma=t(sigma), mask=t(mask),
                             counts=counts, **kw)


def check(got, want, what):
    for g, w, key in zip(got, want, KEYS):
        guarded.assert_bits(g, w, f"{what} {key}")


_WANT = {}                                                  # the restatement of a case, computed once


def case_reference(H, W, B):
    """Per motion: the inputs of the case, the state after the first frame, and per hold the restatement of the second."""
    if (H, W, B) not in _WANT:
        out = []
        for i, motion in enumerate(MOTIONS):
            kind = KINDS[(i + H + W + B) % len(KINDS)]
            with_sigma, with_mask = (i + W) % 2 == 0, (i // 2 + H) % 2 == 0
            cams, m0, m1, sigma, mask, pose = two_frames(H, W, B, motion, kind, 1000 * H + 10 * W + B + i)
            rows = cam_rows(cams)
            s0 = T.step(m0, rows, None, None, sigma[0] if with_sigma else None, None, **PARAMS)
            s1 = [T.step(m1, rows, pose, s0[:3], sigma[1] if with_sigma else None, mask if with_mask else None, hold=hold, **PARAMS)
                  for hold in (0, 1)]
            out.append(dict(motion=motion, kind=kind, cams=cams, m0=m0, m1=m1, sigma=sigma if with_sigma else (None, None),
                            mask=mask if with_mask else None, pose=pose, s0=s0, s1=s1))
        _WANT[(H, W, B)] = out
    return _WANT[(H, W, B)]


@pytest.mark.parametrize("H,W,B", list(itertools.product(HS, WS, BS)))
def test_shapes_motions_and_inputs_bitexact(dev, hip_lib, H, W, B):
    for c in case_reference(H, W, B):
        what = f"B={B} {H}x{W} {c['motion']} {c['kind']} sigma={c['sigma'][0] is not None} mask={c['mask'] is not None}"
        first = step_ops(dev, c["m0"], c["cams"], None, None, c["sigma"][0], None, hold=True, **PARAMS)      # a first frame with hold: one fuse launch
        check(first, c["s0"], what + " first frame")
        for hold in (0, 1):
            got = step_ops(dev, c["m1"], c["cams"], c["pose"], first[:3], c["sigma"][1], c["mask"], hold=bool(hold), **PARAMS)
            check(got, c["s1"][hold], f"{what} hold={hold}")
        none = step_ops(dev, c["m1"], c["cams"], c["pose"], first[:3], c["sigma"][1], c["mask"], hold=True, counts=False, **PARAMS)
        assert none.counts is None
        check(none[:4], c["s1"][1][:4], what + " counts NULL")


def test_the_cases_reach_every_code():
    """Over all the cases above (their restatements; computed here where that test did not run): every code 0 .. 4 occurs, held
    pixels under every motion but the one that leaves nothing in view, and ties of the z-buffer's disparity half under the constant map."""
    total, held = np.zeros(5, np.int64), {m: 0 for m in MOTIONS}
    ties = 0
    for H, W, B in itertools.product(HS, WS, BS):
        for c in case_reference(H, W, B):
            cnt = c["s1"][1][4].sum(axis=0)
            total += cnt + c["s1"][0][4].sum(axis=0)
            held[c["motion"]] += int(c["s1"][1][4][0, 4])
            if c["kind"] == "constant" and c["motion"] == "backward":
                ties += int(c["s1"][1][4][0, 4])
    print("pixels per code over all cases:", total.tolist(), "held per motion (image 0):", held, "held on constant maps moving backward:", ties)
    assert (total > 0).all() and all(n > 0 for m, n in held.items() if m != "out_of_view") and ties > 0


# ---- the raw call ----
def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def raw_step(lib, dev, b, shape, hold, p=PARAMS):
    from lwsnet_amd import _lib
    with torch.cuda.device(dev):
        _lib.check(lib.lws_temporal_step(P(b["meas"]), P(b.get("sigma")), P(b.get("mask")), P(b["cam"]), P(b.get("pose")), P(b.get("Dp")), P(b.get("Vp")),
                                         P(b.get("Ap")), *shape, p["sigma0"], p["min_disp"], p["sigma_min"], p["gate"], p["q"], p["max_jump"], hold,
                                         p["q_hold"], p["max_var"], P(b.get("work")), P(b["D"]), P(b["V"]), P(b["A"]), P(b["code"]), P(b.get("counts")),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "lws_temporal_step")


def full_case(H, W, B, motion, kind, seed):
    """Two frames with sigma and mask given, and the restatement of both steps with hold."""
    cams, m0, m1, sigma, mask, pose = two_frames(H, W, B, motion, kind, seed)
    rows = cam_rows(cams)
    s0 = T.step(m0, rows, None, None, sigma[0], None, **PARAMS)
    s1 = T.step(m1, rows, pose, s0[:3], sigma[1], mask, hold=1, **PARAMS)
    return dict(rows=rows, cams=cams, m0=m0, m1=m1, sigma=sigma, mask=mask, pose=pose, s0=s0, s1=s1)


@pytest.mark.parametrize("H,W,motion,kind", [(5, 65, "backward", "special"), (17, 257, "yaw_and_step", "special"), (2, 3, "identity", "uniform")])
def test_one_element_past_a_16_byte_boundary(dev, hip_lib, H, W, motion, kind):
    B = 2
    c = full_case(H, W, B, motion, kind, 77)
    assert H * W < 16 or ((c["s1"][3] == 4).any() and (c["s1"][3] == 2).any())
    b = dict(meas=misaligned(c["m1"], dev), sigma=misaligned(c["sigma"][1], dev), mask=misaligned(c["mask"], dev), cam=misaligned(c["rows"], dev),
             pose=misaligned(c["pose"], dev), Dp=misaligned(c["s0"][0], dev), Vp=misaligned(c["s0"][1], dev), Ap=misaligned(c["s0"][2], dev),
             work=torch.empty((B * H * W,), dtype=torch.int64, device=dev),
             D=misaligned(np.full((B, 1, H, W), 7.0, F), dev), V=misaligned(np.full((B, 1, H, W), 7.0, F), dev),
             A=misaligned(np.full((B, 1, H, W), 77, np.uint16), dev), code=misaligned(np.full((B, 1, H, W), 77, np.uint8), dev),
             counts=torch.full((B, 5), 77, dtype=torch.int64, device=dev))
    raw_step(hip_lib, dev, b, (B, H, W), 1)
    check([b[k] for k in KEYS], c["s1"], f"misaligned {H}x{W}")


@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
@pytest.mark.parametrize("hold", [0, 1])
def test_memory_contract(dev, hip_lib, word, hold):
    """Inputs, outputs and the workspace between poisoned flanks, the outputs and the workspace poisoned inside: no flank changes and
    every output element is written.  17 x 65: a last quad of one pixel, two rows of workgroups' worth of quads."""
    B, H, W = 2, 17, 65
    c = full_case(H, W, B, "backward", "scene", 5)
    want = c["s1"] if hold else T.step(c["m1"], c["rows"], c["pose"], c["s0"][:3], c["sigma"][1], c["mask"], hold=0, **PARAMS)
    assert (want[3] == 4).any() == bool(hold) and (want[3] == 0).any() and (want[3] == 2).any()
    g = guarded.Guard(dev, word, skew=1)
    b = dict(meas=g.place(c["m1"], name="meas"), sigma=g.place(c["sigma"][1], name="sigma"), mask=g.place(c["mask"], word=guarded.MASK_WORD, name="mask"),
             cam=g.place(c["rows"], name="cam"), pose=g.place(c["pose"], name="pose"), Dp=g.place(c["s0"][0], name="Dp"), Vp=g.place(c["s0"][1], name="Vp"),
             Ap=g.place(c["s0"][2], name="Ap"), work=g.empty((B * H * W,), np.int64, align16=True, word=g.word, name="workspace"),
             D=g.empty((B, 1, H, W), F, name="D"), V=g.empty((B, 1, H, W), F, name="V"), A=g.empty((B, 1, H, W), np.uint16, name="A"),
             code=g.empty((B, 1, H, W), np.uint8, name="code"), counts=g.empty((B, 5), np.int64, align16=True, name="counts"))
    raw_step(hip_lib, dev, b, (B, H, W), hold)
    for key, w in zip(KEYS, want):
        guarded.assert_bits(b[key], w, f"guarded {key}")
    g.check()


def test_batch_independence(dev, hip_lib):
    """The same image alone, first of two and second of two gives the same bytes."""
    H, W = 17, 257
    c = full_case(H, W, 2, "backward", "halves", 9)

    def run(order):
        idx = list(order)
        sel = lambda a: np.ascontiguousarray(a[idx])        # noqa: E731
        prev = tuple(sel(a) for a in c["s0"][:3])
        return step_ops(dev, sel(c["m1"]), [c["cams"][i] for i in idx], sel(c["pose"]), prev, sel(c["sigma"][1]), sel(c["mask"]), hold=True, **PARAMS)

    both, swapped, alone = run((0, 1)), run((1, 0)), run((1,))
    check(both, c["s1"], "both")
    for g, s, a, key in zip(both, swapped, alone, KEYS):
        bits = guarded.as_bits(g[1].cpu().numpy())
        assert np.array_equal(bits, guarded.as_bits(s[0].cpu().numpy())) and np.array_equal(bits, guarded.as_bits(a[0].cpu().numpy())), key


def test_graph_capture_replays_on_two_input_sets(dev, hip_lib):
    B, H, W = 2, 17, 257
    first, second = full_case(H, W, B, "forward", "scene", 21), full_case(H, W, B, "backward", "special", 22)
    keys = ("meas", "sigma", "mask", "pose", "Dp", "Vp", "Ap")

    def inputs(c):
        return dict(zip(keys, (c["m1"], c["sigma"][1], c["mask"], c["pose"], *c["s0"][:3])))

    b = {k: cu(v, dev) for k, v in inputs(first).items()}
    b.update(cam=cu(first["rows"], dev), work=torch.empty((B * H * W,), dtype=torch.int64, device=dev),
             D=torch.empty((B, 1, H, W), dtype=torch.float32, device=dev), V=torch.empty((B, 1, H, W), dtype=torch.float32, device=dev),
             A=torch.empty((B, 1, H, W), dtype=torch.uint16, device=dev), code=torch.empty((B, 1, H, W), dtype=torch.uint8, device=dev),
             counts=torch.empty((B, 5), dtype=torch.int64, device=dev))
    raw_step(hip_lib, dev, b, (B, H, W), 1)                 # the code object is loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        raw_step(hip_lib, dev, b, (B, H, W), 1)
    for c in (first, second, first):
        for k, v in inputs(c).items():
            b[k].copy_(cu(v, dev))
        for k in ("D", "V", "A", "code", "counts", "work"):
            b[k].fill_(77)
        graph.replay()
        torch.cuda.synchronize(dev)
        check([b[k] for k in KEYS], c["s1"], "replay")


# ---- the state-holding class ----
def test_filter_over_four_frames(dev, hip_lib):
    from lwsnet_amd.temporal import TemporalFilter
    H, W = 48, 96
    rng = np.random.default_rng(4)
    from lwsnet_amd.geometry import Camera, relative_pose
    cam = Camera(120.0, 120.0, 47.5, 20.0, 0.5)
    assert tuple(cam.row()) == tuple(F(v) for v in T.SCENE_CAM)
    poses = [T.forward_pose(k, 0.6, yaw=0.01) for k in range(4)]
    frames = []
    for k, p in enumerate(poses):
        t = T.render(p)
        m = np.where(t > 0, t + rng.normal(0, 0.3, t.shape), 0).astype(F)
        if k >= 2:
            m[rng.random(t.shape) < 0.1] = np.nan
        frames.append(m[None, None])
    kw = dict(gate=3.0, q=0.0, sigma0=0.3, max_jump=1.0, hold=True, q_hold=0.05, max_var=4.0, min_disp=0.5)
    want = T.run_sequence(frames, T.SCENE_CAM, poses, **{**kw, "hold": 1})
    filt = TemporalFilter(cam, **kw)
    kept = []
    for k, m in enumerate(frames):
        got = filt.step(cu(m, dev), None if k == 0 else relative_pose(poses[k - 1], poses[k]))
        check(got, want[k], f"frame {k}")
        kept.append(got)
    assert (want[3][3] == 4).any() and (want[3][3] == 2).any() and filt.frames == 4
    assert kept[3].disp.data_ptr() == kept[1].disp.data_ptr() != kept[2].disp.data_ptr()       # two state sets, written in turn
    first = filt.step(cu(frames[0], dev))                   # pose None: a reset
    check(first, want[0], "after the reset")
    assert filt.frames == 1


def test_chain_then_filter(dev, model):
    """run_chain with the occlusion check, its `keep` codes the filter's mask, against the same steps composed by hand and against
    the restatement on what the chain returned."""
    from lwsnet_amd import ops
    from lwsnet_amd import postprocess as post
    from lwsnet_amd.geometry import Camera, relative_pose
    from lwsnet_amd.synth import make_pair
    from lwsnet_amd.temporal import TemporalFilter
    H, W = 64, 256
    cam = Camera(721.5, 721.5, 127.5, 31.5, 0.54)
    opts = post.Options.make(occ_check=1.0)
    filt = TemporalFilter(cam, hold=True, min_disp=0.25)
    poses = [T.forward_pose(k, 0.2) for k in range(2)]
    prev = prev_np = None
    for k in range(2):
        left, right = (a[None] for a in make_pair(H, W, k)[:2])
        res = post.run_chain(model, left, right, opts)
        assert res.keep is not None
        d, keep = res.disp[3].as_subclass(torch.Tensor), res.keep[3]
        pose = None if k == 0 else relative_pose(poses[0], poses[1])
        got = filt.step(d, pose, mask=keep)
        by_hand = ops.temporal_step(d, cam, pose=pose, prev=prev, mask=keep, hold=True, min_disp=0.25)
        want = T.step(d.cpu().numpy(), cam.row()[None], None if k == 0 else pose[None], prev_np, None, keep.cpu().numpy(), hold=1, min_disp=0.25)
        print(f"frame {k}: pixels per code {want[4][0].tolist()}")
        check(got, want, f"frame {k}")
        check(by_hand, want, f"frame {k} by hand")
        prev, prev_np = tuple(t.clone() for t in got[:3]), want[:3]


# ---- the CLI ----
def test_inference_cli_temporal_files(dev, model, tmp_path):
    from PIL import Image
    from lwsnet_amd import imageio as io
    from lwsnet_amd import inference, ops, outputs, synth
    from lwsnet_amd import postprocess as post
    from lwsnet_amd.geometry import Camera, relative_pose
    n = 4
    root = str(tmp_path / "kitti")
    synth.write_kitti_tree(root, n)
    calib = tmp_path / "calib.txt"
    calib.write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
    poses = np.stack([T.forward_pose(k, 0.3, yaw=0.002) for k in range(n)])
    pose_file = tmp_path / "poses.txt"
    pose_file.write_text("".join(" ".join(repr(float(v)) for v in p.reshape(12)) + "\n" for p in poses))
    out = tmp_path / "out"
    written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(calib), "--occ_check", "1", "--save_path", str(out),
                              "--temporal", "--poses", str(pose_file), "--temporal_hold", "--save_temporal", "--save_disp16"])
    stems = [f"{k:06d}_10" for k in range(n)]
    assert sorted(os.listdir(out)) == sorted(s + e for s in stems for e in (".png", "_occ.png", "_disp16.png", "_tcode.png", "_tsigma.png"))
    assert len(written) == 5 * n
    opts = post.Options.make(occ_check=1.0)
    prev = None
    for k, stem in enumerate(stems):
        full = io.load_rgb(os.path.join(root, "image_2", stem + ".png"))
        l_in = io.to_input(io.crop_bottom_right(full))[None]
        r_in = io.to_input(io.crop_bottom_right(io.load_rgb(os.path.join(root, "image_3", stem + ".png"))))[None]
        cam = Camera.from_kitti(str(calib)).crop_bottom_right(*full.shape[:2])
        res = post.run_chain(model, l_in, r_in, opts)
        fused = ops.temporal_step(res.disp[3].as_subclass(torch.Tensor), cam, pose=None if k == 0 else relative_pose(poses[k - 1], poses[k]), prev=prev,
                                  mask=res.keep[3], hold=True)
        prev = fused[:3]
        assert np.array_equal(np.asarray(Image.open(out / (stem + ".png"))), io.disparity_to_color(fused.disp[0, 0].cpu().numpy()))
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_tcode.png"))), outputs.temporal_to_rgb(fused.code[0, 0].cpu().numpy()))
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_tsigma.png"))),
                              outputs.sigma_to_u8(np.sqrt(fused.var[0, 0].cpu().numpy().astype(np.float64)), 8.0))
        _, _, d16 = ops.depth_maps(fused.disp, cam, (fused.code != 0).to(torch.uint8), depth=False, depth16=False, disp16=True)
        assert np.array_equal(np.asarray(Image.open(out / (stem + "_disp16.png"))), d16[0, 0].cpu().numpy())
    assert (fused.code == 2).any()
