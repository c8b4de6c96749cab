"""Every stream-ordering promise of the project, held under a stalled device (tests/stream_stall.py).

The technique, always the same: the destination is poisoned, the producer's stream is stalled with a bounded device-side delay, the
real producer is queued behind the delay, then the consumer is queued.  A consumer that lacks its wait runs at once on an otherwise
idle stream and reads the poison, so the bits differ.  Expected values are the same call run calmly on the same inputs, compared bit
for bit (guarded.assert_bits); the other test modules tie those bits to the references.  The forwards are held to the C oracle's maps
directly, calm and stalled: a fork without its wait is wrong in a calm run as well.  Every case runs once per stream of stream_stall.caller_streams, because a stream that happens to share a
hardware queue with the library's side stream is ordered by accident.

What is held:
  a. every C-ABI function whose prototype ends in `void *stream` runs all of its kernels, clears and memsets on that stream (TABLE);
  b. the forks of lws_forward / lws_forward_conf, on every launch plan: a side branch that starts before its producer reads the
     quiet NaN the workspace and the input buffers hold;
  c. two forwards back to back behind one stall: the forks of call n + 1 against the tail of call n on the shared workspace;
  d. a captured graph replayed behind a stall;
  e. lws_pool: a job starts behind everything queued on `after_stream`; lws_pool_wait returns only once the outputs are final;
  f. dist.StagedGather(multi_stream=True): a gather runs behind the writers of its slots, a step on another stream behind the
     gather that still reads the buffer it is handed;
  g. the pipelined CLIs (inference.inference_pipelined, evaluate._pipelined) with their device-side I/O kernels held back: the
     pool's jobs behind the upload stream, the read-back behind the colour map, the metric's sums behind its kernel.

A missing JOIN -- the caller's stream waiting for the side branch -- cannot be forced from here: the side stream belongs to the
handle.  tests/test_gpu_side_delay.py holds the joins, with lws_debug_delay_side making the side branch late from inside."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import guarded as G
import stream_stall as SS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H, W = 64, 256                      # the smallest valid frame, maxdisplist (24, 5, 5)
RESERVE = (4, H, W)
OPTION_DEFAULTS = dict(side_streams=1, ref_chunk_mb=72, ref_pipe=-1, fork2_after=-1, host_joins=-1, host_join_budget_us=900)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def streams(dev):
    SS.ticks_per_ms(dev)
    a = torch.zeros((2, 8), device=dev)                 # the fills and copies the cases queue behind their stalls, once calmly:
    poison_(a.clone().fill_(1.0)).copy_(a)              # loading a kernel for its first launch can take longer than a stall
    poison_(torch.zeros(8, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    return SS.caller_streams(dev)


def new_net(dev, reserve=RESERVE):
    from lwsnet_amd import _lib
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    m = LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()
    with torch.cuda.device(dev):
        _lib.call("lws_reserve", m._h, *reserve)
    return m


@pytest.fixture(scope="module")
def net(dev, hip_lib):
    return new_net(dev)


@pytest.fixture(scope="module")
def pairs(dev):
    """Eight pairs on the device: set A is [:B], set B is [4:4 + B]."""
    from lwsnet_amd.synth import make_batch
    left, right = make_batch(8, H, W, 4242)
    return cu(left, dev), cu(right, dev), left, right


_ORACLE = []


@pytest.fixture(scope="module")
def oracle(net, pairs):
    """The C oracle's four stage maps of the eight pairs, [8,1,H,W] each (pairs are independent of their batch)."""
    if not _ORACLE:         # once per process: tests/test_gpu_side_delay.py borrows this fixture, and the pairs and weights are fixed
        from oracle import c_oracle
        _ORACLE.extend(c_oracle.forward(pairs[2], pairs[3], net.state_dict()))
    return list(_ORACLE)


def maps_of(oracle, lo, B):
    return [m[lo:lo + B] for m in oracle]


def cu(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def sp(stream):
    return ctypes.c_void_p(stream.cuda_stream)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def arr(n, ts):
    return (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])


def poison_(t):
    """Fills t on the current stream: float32 with the quiet-NaN word of guarded.FLOAT_WORDS, every other type with the byte 0xA5."""
    if t.numel():
        if t.dtype == torch.float32:
            t.view(torch.int32).fill_(G.QNAN)
        else:
            t.view(torch.uint8).fill_(G.BYTE)
    return t


def poisoned(shape, dtype, dev):
    return poison_(torch.empty(tuple(shape), dtype=dtype, device=dev))


def still_poison(a):
    """A numpy array that holds nothing but what poison_ wrote."""
    if a.dtype == np.float32:
        return bool((G.as_bits(a) == G.QNAN).all())
    return bool((np.ascontiguousarray(a).reshape(-1).view(np.uint8) == G.BYTE).all())


def host(ts):
    return [None if t is None else t.cpu().numpy() for t in ts]


def assert_all_bits(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert (g is None) == (w is None), (what, i)
        if g is not None:
            G.assert_bits(g, w, f"{what}: output {i}")


@contextlib.contextmanager
def plan(net, options):
    """The launch-plan options of one case, the defaults restored afterwards."""
    try:
        for k, v in options.items():
            net.set_option(k, v)
        yield
    finally:
        for k, v in OPTION_DEFAULTS.items():
            net.set_option(k, v)


# ================================================================== the stall itself
def test_a_stall_holds_its_stream_about_as_long_as_asked(dev, streams):
    """The tick rate is measured once and every stall scaled from it: a stall of STALL_MS must then last between half and twice
    that (the counter behind torch.cuda._sleep runs at about the shader clock, which power management moves by less than a factor
    of two between the probe and a stall), and what is queued behind it runs behind it, while another stream is not held.  Prints
    the figures profiles/NOTES.md quotes."""
    flag = torch.zeros(1, device=dev)
    flag.fill_(0.0).clone()             # calmly first, as everywhere in this file: loading a kernel can take longer than the stall
    torch.cuda.synchronize()
    with torch.cuda.stream(streams[0]):
        ev = SS.stall(streams[0])
        flag.fill_(1.0)
    SS.assert_still_stalled(ev)
    with torch.cuda.stream(streams[1]):
        early = flag.clone()            # another stream is not held
        streams[1].synchronize()
    SS.assert_still_stalled(ev)
    ms = ev.stalled_ms()
    torch.cuda.synchronize()
    print(f"torch.cuda._sleep: {SS.ticks_per_ms(dev):.0f} ticks per ms; a stall of {SS.STALL_MS} ms held its stream for {ms:.2f} ms")
    assert float(early) == 0.0 and float(flag) == 1.0
    assert 0.5 * SS.STALL_MS <= ms <= 2.0 * SS.STALL_MS, ms


# ================================================================== a. every entry point honours its stream
class Recorder:
    """Listens at the two places lwsnet_amd.ops hands tensors to the library (ops._call, ops._arr) while a case runs calmly through
    the Python wrappers, which size every buffer.  A recorded call can then be made again through the C ABI on buffers of this
    module's own: `const` pointers of the prototype are inputs, everything else is an output or a workspace."""

    def __init__(self):
        self.calls, self.arrays, self.fresh_workspaces, self.inout = {}, {}, [], set()

    def io(self, *tensors):
        """Declares tensors a call of the case updates in place: their contents before the call are inputs as well."""
        self.inout.update(t.data_ptr() for t in tensors if t is not None)

    @contextlib.contextmanager
    def listening(self):
        from lwsnet_amd import ops
        real_call, real_arr, real_work = ops._call, ops._arr, ops._workspace

        def arr_(ts, n=4):
            a = real_arr(ts, n)
            self.arrays[id(a)] = (a, list(ts) + [None] * (n - len(ts)))
            return a

        def work_(name, device, *dims):
            t = real_work(name, device, *dims)
            self.fresh_workspaces.append(t)                 # alive until the call that uses it: its address is not handed out again
            return t

        def call_(name, device, *args):
            items = []
            for a in args:
                if isinstance(a, torch.Tensor):
                    items.append(("tensor", a, a.clone()))
                elif id(a) in self.arrays:
                    ts = self.arrays[id(a)][1]
                    items.append(("array", ts, [None if t is None else t.clone() for t in ts]))
                else:
                    items.append(("raw", a, None))
            self.calls[name] = (device, items, {t.data_ptr() for t in self.fresh_workspaces})      # the latest call of a name is replayed
            self.fresh_workspaces = []
            return real_call(name, device, *args)

        ops._call, ops._arr, ops._workspace = call_, arr_, work_
        try:
            yield self
        finally:
            ops._call, ops._arr, ops._workspace = real_call, real_arr, real_work


def replay(rec, name, stream, stall_ms):
    """The recorded call `name` made through the C ABI on `stream`: inputs hold poison until the copies queued behind the stall
    (stall_ms, None for the calm run) bring the real data; outputs and workspaces, the handle's included, are poisoned before the
    stall, the caller's once more behind it, so that a clear or memset that runs early on another stream is overwritten.  Returns the outputs as numpy arrays, in
    parameter order, the workspaces left out (their contents are undefined)."""
    from lwsnet_amd import _lib
    device, items, workspaces = rec.calls[name]
    spell = _lib.merge_headers({h: t[1] for h, t in _lib.ABI.items()})[name][1]
    assert len(spell) == len(items) + 1 and spell[-1] == "void *", (name, spell)
    bufs, order = {}, []

    def buffer(t, before, const):
        key = t.data_ptr()
        if key not in bufs:
            src = before if const or key in rec.inout else None
            bufs[key] = (poisoned(t.shape, t.dtype, t.device), src)
            if not const and key not in workspaces:
                order.append(key)
        return bufs[key][0]

    args = []
    for (kind, value, before), c_type in zip(items, spell):
        const = c_type.startswith("const ")
        if kind == "tensor":
            args.append(P(buffer(value, before, const)))
        elif kind == "array":
            args.append(arr(len(value), [None if t is None else buffer(t, b, const) for t, b in zip(value, before)]))
        else:
            args.append(value)
    handle = items[0][1] if spell[0] == "lws_handle" else None
    with torch.cuda.device(device), torch.cuda.stream(stream):
        if handle is not None:          # what an earlier call left in the handle's workspace is gone before the stall begins
            _lib.call("lws_debug_fill_workspace", handle, ctypes.c_uint32(G.QNAN), sp(stream))
        torch.cuda.synchronize()
        ev = SS.stall(stream, stall_ms) if stall_ms else None
        for buf, src in bufs.values():
            if src is not None:
                buf.copy_(src, non_blocking=True)
            else:
                poison_(buf)
        if ev is None:
            stream.synchronize()        # the calm run: the inputs have landed whatever stream a kernel of the call is on
        _lib.call(name, *args, sp(stream))
    if ev is not None:
        SS.assert_still_stalled(ev, name)
    stream.synchronize()
    return host([bufs[k][0] for k in order])


def cases_network(dev, net, io):
    """The per-op entry points of the network at the shapes of tests/test_gpu_memory_contract.py, and the whole forwards."""
    from conftest import golden
    from lwsnet_amd import imageio, ops
    from lwsnet_amd.synth import make_batch
    from test_gpu_confidence import START, op_case
    from test_gpu_parity import _warp_case
    rng = np.random.default_rng(11)
    L, R = (rng.standard_normal((3, 16, 5, 24)).astype(np.float32) for _ in range(2))
    ops.volume_l1_shift(cu(L, dev), cu(R, dev), 24)
    L, R, prev, _, _ = _warp_case(np.random.default_rng(5), 2, 8, 19, 65, 2, 0)
    ops.volume_l1_warp(cu(L, dev), cu(R, dev), cu(prev, dev), 5, return_wflow=True)
    ops.conv3d_stack(net._h, 1, cu((rng.random((1, 4, 9, 31)) * 12.0).astype(np.float32), dev))
    ops.softargmin(cu((rng.random((1, 24, 2, 67)) * 12.0).astype(np.float32), dev), 0.0)
    ops.softargmin_conf(cu(op_case(3, 9, (5, 11), (40, 88))[0], dev), START[9], 40, 88)
    ops.upsample_add(cu((rng.random((2, 3, 5)) * 20.0).astype(np.float32), dev), cu((rng.random((2, 1, 24, 40)) * 150.0).astype(np.float32), dev), 24, 40)
    ops.feature_extraction(net._h, cu(rng.standard_normal((3, 3, 32, 48)).astype(np.float32), dev))
    ops.refine(net._h, cu(rng.standard_normal((2, 3, 17, 15)).astype(np.float32), dev), cu((rng.random((2, 1, 17, 15)) * 150.0).astype(np.float32), dev))
    gold = golden("e2e_64x256.npz")
    ops.disparity_stages(net._h, [cu(gold[f"featL{i}"], dev) for i in range(3)], [cu(gold[f"featR{i}"], dev) for i in range(3)], H, W)
    left, right = (cu(a, dev) for a in make_batch(1, H, W, 61))
    ops.forward(net._h, left, right)
    ops.forward_conf(net._h, left, right)
    img = rng.integers(0, 256, size=(2, 37, 53, 3), dtype=np.uint8)
    ops.preprocess_rgb8(cu(img, dev))
    ops.apply_lut8(cu((rng.random((61, 47)) * 300.0 - 20.0).astype(np.float32), dev), cu(imageio.jet_lut(), dev))


def cases_checks(dev, net, io):
    """The checks and scores of stage maps: 17 x 65 maps at B = 2, 37 x 61 against ground truth."""
    from lwsnet_amd import ops
    from test_gpu_lrcheck import maps
    from test_gpu_occlusion import stage_maps
    from test_gpu_photometric import case
    from test_gpu_sparsification import make_inputs
    B, h, w = 2, 17, 65
    rng = np.random.default_rng(3)
    ops.lr_pairs(*(cu(rng.standard_normal((B, 3, h, w)).astype(np.float32), dev) for _ in range(2)))
    stages = [maps(B, h, w, 10 * s + w) for s in range(2)]
    ops.lr_check([cu(s[0], dev) for s in stages], [cu(s[1], dev) for s in stages], 1.0, True)
    ops.occlusion_check([cu(d, dev) for d in stage_maps(B, h, w)], 0.5, True)
    preds, unc, gt = make_inputs(B, 37, 61, 3, 0, seed=2101)
    ops.stage_metrics([cu(p, dev) for p in preds], cu(gt, dev), 3, 192, 0)
    ops.sparsification([cu(p, dev) for p in preds], [cu(u, dev) for u in unc], cu(gt, dev), 3, 192, 0, 0)
    c = case(B, h, w)
    ops.photometric([cu(d, dev) for d in c["disp"]], cu(c["left"], dev), cu(c["right"], dev), [cu(m, dev) for m in c["mask"]], cu(c["rvalid"], dev),
                    0.85, want_err=True, want_scored=True, want_warped=True)


def cases_maps(dev, net, io):
    """What is made of one disparity map: geometry, mesh, filters, the rectifier in front of it."""
    import speckle_inputs as SI
    from lwsnet_amd import ops
    from test_gpu_geometry import cameras, maps
    from test_gpu_mesh import scene
    from test_gpu_rectify import raw_images, records, run
    from test_gpu_wmedian import inputs
    B, h, w = 2, 17, 65
    d, m, rgb = maps(B, h, w, 5)
    ops.depth_maps(cu(d, dev), cameras(B), cu(m, dev), 1.0, 80.0)
    ops.point_cloud(cu(d, dev), cameras(B), cu(m, dev), cu(rgb, dev), 1.0, 80.0)
    d, m, rgb = scene(B, h, w, 7)
    ops.surface_mesh(cu(d, dev), cameras(B), cu(m, dev), cu(rgb, dev), 1.0, 80.0, 1.0, with_normals=True, want_index=True)     # normals, then the mesh
    ops.speckle_filter(cu(SI.make("plateaus", B, h, w, 3 * h + w), dev), 50, 0.5, mask=cu(SI.random_mask(B, h, w, h + 7 * w), dev), fill=True, want_labels=True)
    d, m, g = inputs(B, h, w)
    ops.wmedian_filter(cu(d, dev), 2, rgb=cu(g, dev), wlut=cu(ops.wmedian_lut(2.0), dev), mask=cu(m, dev), fill_min=4)
    run(dev, raw_images(B, 37, 53, 1), records(B, 37, 53, 29, 45, 3, 2, seed=2), (29, 45), (3, 2), 0)


def cases_road(dev, net, io):
    """The 96 x 160 road scenes through ground, stixels and objects."""
    from test_gpu_ground import roads
    from test_gpu_objects import ground_stixels_objects
    ground_stixels_objects(*roads(2, 31), dev)


def cases_sequence(dev, net, io):
    """Over frames: the temporal filter's second step, one linearisation and the three-level estimate of the ego-motion at 17 x 65,
    the 33 x 4 x 5 volume."""
    import temporal_reference as T
    import tsdf_reference as R
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    from test_gpu_egomotion import HUBER, MIN_DISP, images, level_camera, normal_cases
    from test_gpu_temporal import PARAMS, step_ops, two_frames
    B, h, w = 2, 17, 65
    cams, m0, m1, sigma, mask, pose = two_frames(h, w, B, "forward", "scene", 1765)
    first = step_ops(dev, m0, cams, None, None, sigma[0], None, hold=True, **PARAMS)
    step_ops(dev, m1, cams, pose, first[:3], sigma[1], mask, hold=True, **PARAMS)
    c = normal_cases(h, w, B)[1]
    ops.ego_normal(cu(c["g0"], dev), cu(c["d0"], dev), cu(c["g1"], dev), c["cams"], c["M"], level=c["level"], mask=cu(c["mask"], dev), min_disp=MIN_DISP,
                   huber=HUBER, terms=True)
    rng = np.random.default_rng(11)
    full, cam_l = level_camera(h, w, 0)
    T0, T1 = T.forward_pose(0, 0.0), T.forward_pose(1, 0.3, 0.01)
    rgb = [np.stack([np.repeat(np.clip(images("scene", h, w, cam_l, t, rng)[0], 0, 255).astype(np.uint8)[..., None], 3, -1) for _ in range(B)]) for t in (T0, T1)]
    d = np.stack([images("special", h, w, cam_l, T0, rng)[1] for _ in range(B)])[:, None]
    mask = rng.choice(np.array([0, 1, 1, 1, 2], np.uint8), size=(B, 1, h, w))
    ops.egomotion(cu(rgb[0], dev), cu(d, dev), cu(rgb[1], dev), [full] * B, mask=cu(mask, dev), levels=3, iters=2, min_disp=0.5, max_jump=1.0, huber=10.0,
                  damping=0.0, min_pixels=16, trace=True, resid=True)
    v = R.integrate_case((33, 4, 5), (5, 7), 3)
    f = v["cam"][0]
    vcams = [Camera(float(f[0]), float(f[1]), float(f[2]), float(f[3]), 4.0)] * 3
    kw = {**{k: x for k, x in v["kw"].items() if k != "wmode"}, "weight": ("unit", "sigma")[v["kw"]["wmode"]]}
    Tv, Wv, Cv = cu(v["T0"], dev), cu(v["W0"], dev), cu(v["C0"], dev)
    io(Tv, Wv, Cv)
    ops.tsdf_integrate(Tv, Wv, v["origin"], v["vs"], cu(v["disp"], dev), vcams, v["pose"], C=Cv, sigma=cu(v["sigma"], dev), mask=cu(v["mask"], dev),
                       normals=cu(v["normals"], dev), rgb=cu(v["rgb"], dev), **kw)
    Tc, Wc, origin, vs = R.crafted_volume()
    cam, pose = R.raycast_views()
    views = [Camera(*(float(x) for x in row[:4]), float(row[4] / row[0])) for row in cam]
    ops.tsdf_raycast(cu(Tc, dev), cu(Wc, dev), origin, vs, views, np.ascontiguousarray(pose, np.float32), 24, 40, **R.RAYCASTS[0])
    Tp, Wp, Cp, origin, vs = R.points_volume((33, 4, 5), 1)
    ops.tsdf_points(cu(Tp, dev), cu(Wp, dev), origin, vs, 4096, C=cu(Cp, dev))


SCENARIOS = {"network": cases_network, "checks": cases_checks, "maps": cases_maps, "road": cases_road, "sequence": cases_sequence}
# one row per C-ABI function whose prototype ends in `void *stream`: the scenario whose calm run makes the call that is replayed
TABLE = {
    "lws_volume_l1_shift": "network", "lws_volume_l1_warp": "network", "lws_conv3d_stack": "network", "lws_softargmin": "network",
    "lws_softargmin_conf": "network", "lws_upsample_add": "network", "lws_feature_extraction": "network", "lws_refine": "network",
    "lws_disparity_stages": "network", "lws_forward": "network", "lws_forward_conf": "network", "lws_preprocess_rgb8": "network",
    "lws_apply_lut8": "network",
    "lws_lr_pairs": "checks", "lws_lr_check": "checks", "lws_occlusion_check": "checks", "lws_stage_metrics": "checks",
    "lws_sparsification": "checks", "lws_photometric": "checks",
    "lws_depth_maps": "maps", "lws_point_cloud": "maps", "lws_surface_normals": "maps", "lws_surface_mesh": "maps",
    "lws_speckle_filter": "maps", "lws_wmedian_filter": "maps", "lws_rectify_pair": "maps",
    "lws_vdisparity": "road", "lws_ground_fit": "road", "lws_ground_classify": "road", "lws_bev_grid": "road", "lws_stixels": "road",
    "lws_objects": "road",
    "lws_temporal_step": "sequence", "lws_ego_normal": "sequence", "lws_egomotion": "sequence", "lws_tsdf_integrate": "sequence",
    "lws_tsdf_raycast": "sequence", "lws_tsdf_points": "sequence",
}
# functions with a `void *stream` that have no row, and why
EXCLUDED = {"lws_debug_fill_workspace": "the tool that poisons the handle's workspace behind the stall in the rows of the handle's entry points and in every "
                                        "forward case below; a fill on the wrong stream lets the workspace reach them clean, which no bit compare can see"}

_RECORDED = {}


def recorded(scenario, dev, net):
    """The scenario run once, calmly, through the wrappers, every call to the library noted."""
    if scenario not in _RECORDED:
        rec = Recorder()
        with rec.listening(), torch.cuda.device(dev):
            SCENARIOS[scenario](dev, net, rec.io)
        torch.cuda.synchronize()
        _RECORDED[scenario] = rec
    return _RECORDED[scenario]


@pytest.mark.parametrize("name", sorted(TABLE))
def test_entry_point_runs_on_the_stream_it_is_given(dev, net, streams, name):
    rec = recorded(TABLE[name], dev, net)
    assert name in rec.calls, f"the scenario {TABLE[name]!r} never called {name}"
    want = replay(rec, name, streams[0], None)
    assert want and not all(still_poison(w) for w in want), f"{name}: the calm call wrote nothing"
    for i, s in enumerate(streams):
        assert_all_bits(replay(rec, name, s, SS.STALL_MS), want, f"{name} on caller stream {i}")


# ================================================================== b. the forks of the forward
def forward_call(net, left, right, outs, stream, conf=None, sigma=None):
    from lwsnet_amd import _lib
    B = left.shape[0]
    if conf is None:
        _lib.call("lws_forward", net._h, P(left), P(right), B, H, W, arr(4, outs), sp(stream))
    else:
        _lib.call("lws_forward_conf", net._h, P(left), P(right), B, H, W, arr(4, outs), arr(3, conf), arr(3, sigma), sp(stream))


def stalled_forward(net, dev, lt, rt, stream, stall_ms, conf=False, blocking=False):
    """One forward of the pairs lt, rt on `stream` by the pattern of the module docstring: the handle's workspace filled with quiet
    NaN on the stream, the input buffers holding the same until the copies behind the stall.  Returns the 4 (10 with conf) maps."""
    from lwsnet_amd import _lib
    B = lt.shape[0]
    left, right = poisoned(lt.shape, torch.float32, dev), poisoned(rt.shape, torch.float32, dev)
    outs = [poisoned((B, 1, H, W), torch.float32, dev) for _ in range(10 if conf else 4)]
    torch.cuda.synchronize()
    with torch.cuda.device(dev), torch.cuda.stream(stream):
        _lib.call("lws_debug_fill_workspace", net._h, ctypes.c_uint32(G.QNAN), sp(stream))
        stream.synchronize()
        ev = SS.stall(stream, stall_ms) if stall_ms else None
        left.copy_(lt, non_blocking=True)
        right.copy_(rt, non_blocking=True)
        for o in outs:
            poison_(o)
        _, seconds = SS.timed(forward_call, net, left, right, outs[:4], stream, *((outs[4:7], outs[7:]) if conf else ()))
    if ev is not None and blocking:
        SS.assert_host_was_held(ev, seconds, "a forward whose joins the host resolves")
    elif ev is not None:
        SS.assert_still_stalled(ev, "forward")
    stream.synchronize()
    return host(outs)


# id -> (batch, options)
PLANS = {
    "defaults-b1": (1, {}), "defaults-b2": (2, {}),
    "defaults-b4": (4, {}),                                               # the second plan: the right-image head on its own side stream
    "four-chunks-b4": (4, dict(ref_chunk_mb=1, ref_pipe=1)),              # four chunks of one pair, alternating streams
    "fork2-after-0": (1, dict(fork2_after=0)), "fork2-after-2": (1, dict(fork2_after=2)), "fork2-after-2-b4": (4, dict(fork2_after=2)),
    "queued-joins": (1, dict(host_joins=0)), "polled-joins-budget-0": (1, dict(host_joins=1, host_join_budget_us=0)),
    "single-stream": (1, dict(side_streams=0)),                           # the control: no forks at all
}


@pytest.mark.parametrize("plan_id", list(PLANS))
def test_forward_forks_wait_for_their_producers(dev, net, streams, pairs, oracle, plan_id):
    """Expected: the C oracle's maps.  The same call run calmly must give them too, but it is not what the stalled runs are compared
    with: a fork without its wait can read the poisoned workspace in a calm run as well, and two equally wrong runs would agree."""
    from test_gpu_host_joins import stats
    B, options = PLANS[plan_id]
    lt, rt, _, _ = pairs
    want = maps_of(oracle, 0, B)
    with plan(net, options):
        assert_all_bits(stalled_forward(net, dev, lt[:B], rt[:B], streams[0], None), want, f"{plan_id}: the calm forward against the C oracle")
        for i, s in enumerate(streams):
            stats(net)
            got = stalled_forward(net, dev, lt[:B], rt[:B], s, SS.STALL_MS)
            st = stats(net)
            assert_all_bits(got, want, f"{plan_id} on caller stream {i}")
            if "host_joins" in options:         # with the device stalled no join can have been seen complete by the host
                assert (st[:, 0] == 0).all() and (st[:, 1] == 1).all(), (plan_id, i, st.tolist())


def test_forward_with_host_resolved_joins_holds_the_host(dev, net, streams, pairs, oracle):
    """"host_joins" = 1 with a budget of one second blocks by contract: the host polls the first join until the stalled head has run."""
    lt, rt, _, _ = pairs
    want = maps_of(oracle, 0, 1)
    with plan(net, dict(host_joins=1, host_join_budget_us=1000000)):
        for i, s in enumerate(streams):
            assert_all_bits(stalled_forward(net, dev, lt[:1], rt[:1], s, SS.STALL_MS, blocking=True), want, f"caller stream {i}")


@pytest.mark.parametrize("B", [1, 4])
def test_forward_conf_forks_wait_for_their_producers(dev, net, streams, pairs, oracle, B):
    """All four stage maps and the six confidence outputs.  Expected: the C oracle's stage maps, and the confidence maps of the
    single-stream plan, which has no fork to miss (every plan gives the same bits)."""
    lt, rt, _, _ = pairs
    with plan(net, dict(side_streams=0)):
        want = stalled_forward(net, dev, lt[:B], rt[:B], streams[0], None, conf=True)
    assert_all_bits(want[:4], maps_of(oracle, 0, B), "the single-stream forward_conf against the C oracle")
    assert not any(still_poison(w) for w in want[4:])
    assert_all_bits(stalled_forward(net, dev, lt[:B], rt[:B], streams[0], None, conf=True), want, f"B={B}: the calm call")
    for i, s in enumerate(streams):
        assert_all_bits(stalled_forward(net, dev, lt[:B], rt[:B], s, SS.STALL_MS, conf=True), want, f"B={B} on caller stream {i}")


# ================================================================== c. two forwards back to back
@pytest.mark.parametrize("B", [1, 4])
def test_two_forwards_back_to_back_behind_one_stall(dev, net, streams, pairs, oracle, B):
    """Forward n + 1 is queued while the device is still stalled: its forks must wait for the tail of forward n, which still owns
    the workspace the side branches write."""
    lt, rt, _, _ = pairs
    sets = [(lt[:B], rt[:B]), (lt[4:4 + B], rt[4:4 + B])]
    want = [maps_of(oracle, 0, B), maps_of(oracle, 4, B)]
    for k, (l, r) in enumerate(sets):
        assert_all_bits(stalled_forward(net, dev, l, r, streams[0], None), want[k], f"B={B}: the calm forward of set {k}")
    from lwsnet_amd import _lib
    for i, s in enumerate(streams):
        ins = [(poisoned(l.shape, torch.float32, dev), poisoned(r.shape, torch.float32, dev)) for l, r in sets]
        outs = [[poisoned((B, 1, H, W), torch.float32, dev) for _ in range(4)] for _ in sets]
        torch.cuda.synchronize()
        with torch.cuda.device(dev), torch.cuda.stream(s):
            _lib.call("lws_debug_fill_workspace", net._h, ctypes.c_uint32(G.QNAN), sp(s))
            s.synchronize()
            ev = SS.stall(s)
            for (l, r), (lb, rb), o in zip(sets, ins, outs):
                lb.copy_(l, non_blocking=True)
                rb.copy_(r, non_blocking=True)
                forward_call(net, lb, rb, o, s)
        SS.assert_still_stalled(ev, "two forwards")
        s.synchronize()
        for k in range(2):
            assert_all_bits(host(outs[k]), want[k], f"B={B} caller stream {i} forward {'n' if k == 0 else 'n + 1'}")


# ================================================================== d. a captured graph
@pytest.mark.parametrize("B", [1, 3])
def test_captured_graph_replayed_behind_a_stall(dev, hip_lib, streams, pairs, oracle, B):
    """Captured as tests/test_gpu_parity.py::test_graph_capture_replays_the_forward captures it.  The inputs arrive behind the stall;
    the workspace is not poisoned (include/lwsnet_hip.h forbids lws_debug_fill_workspace around a captured stream)."""
    lt, rt, _, _ = pairs
    m = new_net(dev, (B, H, W))
    want = maps_of(oracle, 0, B)
    assert_all_bits(host(m(lt[:B].clone(), rt[:B].clone())), want, f"B={B}: the eager forward")
    left, right = lt[4:4 + B].clone(), rt[4:4 + B].clone()             # captured on other pairs than the ones replayed
    outs = [torch.empty((B, 1, H, W), device=dev) for _ in range(4)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m(left, right, out=outs)
    g.replay()                                                          # once calmly: the graph is instantiated and loaded
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        for t in (left, right, *outs):
            poison_(t)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ev = SS.stall(s)
            left.copy_(lt[:B], non_blocking=True)
            right.copy_(rt[:B], non_blocking=True)
            g.replay()
        SS.assert_still_stalled(ev, "graph replay")
        s.synchronize()
        assert_all_bits(host(outs), want, f"B={B} replay on caller stream {i}")


# ================================================================== e. lws_pool
@pytest.fixture(scope="module", params=[False, True], ids=["one-stream-workers", "side-stream-workers"])
def pool(request, dev, net):
    with net.pool(workers=3, side_streams=request.param) as p:
        p.reserve(1, H, W)
        yield p


@pytest.fixture(scope="module")
def calm_maps(dev, net, pairs, oracle):
    """lws_forward's maps of each of the eight pairs alone, which are the C oracle's."""
    lt, rt, _, _ = pairs
    maps = [host(net(lt[k:k + 1], rt[k:k + 1])) for k in range(8)]
    for k in range(8):
        assert_all_bits(maps[k], maps_of(oracle, k, 1), f"lws_forward of pair {k}")
    return maps


def test_pool_job_starts_behind_after_stream_and_wait_means_complete(dev, net, pool, streams, pairs, calm_maps):
    """The inputs are produced on `after_stream` behind a stall.  submit returns at once; lws_pool_wait returns only after the stall,
    and the outputs, read right then through a fresh stream with no other synchronisation, are final."""
    lt, rt, _, _ = pairs
    for i, s in enumerate(streams):
        left, right = poisoned((1, 3, H, W), torch.float32, dev), poisoned((1, 3, H, W), torch.float32, dev)
        outs = [poisoned((1, 1, H, W), torch.float32, dev) for _ in range(4)]
        reader = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ev = SS.stall(s)
            left.copy_(lt[i:i + 1], non_blocking=True)
            right.copy_(rt[i:i + 1], non_blocking=True)
            job = pool.submit(left, right, out=outs)
        SS.assert_still_stalled(ev, "lws_pool_submit")
        _, seconds = SS.timed(job.result)
        with torch.cuda.stream(reader):
            got = host(outs)
        assert_all_bits(got, calm_maps[i], f"after_stream = caller stream {i}")
        SS.assert_host_was_held(ev, seconds, "lws_pool_wait")


def test_pool_twelve_jobs_from_a_ring_of_three_input_buffers(dev, net, pool, streams, pairs, calm_maps):
    """Twelve tickets, each with the bits of its own input.  The producers are queued on `after_stream` only and the host never
    waits for them; it does wait for ticket t - 3 before the producer of ticket t reuses that job's buffers, as the header demands,
    so the stall covers the first three jobs and the later ones meet producers that have only just been queued."""
    lt, rt, _, _ = pairs
    for i, s in enumerate(streams):
        ring = [(poisoned((1, 3, H, W), torch.float32, dev), poisoned((1, 3, H, W), torch.float32, dev)) for _ in range(3)]
        outs = [[poisoned((1, 1, H, W), torch.float32, dev) for _ in range(4)] for _ in range(12)]
        jobs = []
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            ev = SS.stall(s)
            for t in range(12):
                if t == 3:
                    SS.assert_still_stalled(ev, "three submits")
                if t >= 3:
                    jobs[t - 3].result()
                k = (t + i) % 8
                ring[t % 3][0].copy_(lt[k:k + 1], non_blocking=True)
                ring[t % 3][1].copy_(rt[k:k + 1], non_blocking=True)
                jobs.append(pool.submit(*ring[t % 3], out=outs[t]))
        for t in range(12):
            jobs[t].result()
            assert_all_bits(host(outs[t]), calm_maps[(t + i) % 8], f"caller stream {i} ticket {t}")


# ================================================================== f. dist.StagedGather on several streams
GH, GW = 64, 256
SHORT_MS = SS.STALL_MS / 2      # the committing step's stall: its stream is ahead of the slot writers', so a gather without its wait runs first


def gather_steps(dev, sa, sb):
    """Six steps alternating between two streams, no process group: the gather is the device copy into recv[b][0].  Every step stalls
    its stream, writes step + 1 into its slot and commits; the steps that gather are on the stream with the shorter stalls."""
    from lwsnet_amd.dist import StagedGather
    sg = StagedGather(1, GH, GW, 2, dev, multi_stream=True)
    for t in (*sg.staging, *sg.recv[0], *sg.recv[1]):
        poison_(t)
    torch.cuda.synchronize()
    seen = []
    for step in range(6):
        st = sb if step & 1 else sa
        with torch.cuda.stream(st):
            ev = SS.stall(st, SHORT_MS if step & 1 else SS.STALL_MS)
            sg.slot().fill_(float(step + 1))
            if sg.commit():
                SS.assert_still_stalled(ev, f"commit of step {step}")
                seen.append((step, sg.gathered(0)[0].clone()))         # queued behind the gather on its own stream
    torch.cuda.synchronize()
    for step, t in seen:
        got = t.cpu().numpy()
        want = np.stack([np.full((1, GH, GW), v, np.float32) for v in (step, step + 1)])
        G.assert_bits(got, want, f"the buffer gathered at step {step}")
    assert [s for s, _ in seen] == [1, 3, 5]


@pytest.mark.parametrize("first", [0, 2])
def test_staged_gather_orders_gathers_behind_slot_writers(dev, hip_lib, streams, first):
    gather_steps(dev, streams[first], streams[first + 1])
    gather_steps(dev, streams[first + 1], streams[first])


def test_staged_gather_case_fails_without_its_waits(dev, hip_lib, streams, monkeypatch):
    """The test of the test: with Stream.wait_event a no-op the gather runs before the other stream's slot has been written, and the
    case above must fail on the gathered bits.  If it passes, the stall is too short or the two streams share a hardware queue."""
    monkeypatch.setattr(torch.cuda.Stream, "wait_event", lambda self, event: None)
    failed = 0
    for a, b in ((0, 1), (2, 3)):
        try:
            gather_steps(dev, streams[a], streams[b])
        except AssertionError as e:
            assert "the buffer gathered at step" in str(e), e
            failed += 1
    assert failed > 0, "a gather without its waits still gave the right bits"


@pytest.mark.parametrize("first", [0, 2])
def test_staged_gather_flush_then_a_step_on_the_other_stream(dev, hip_lib, streams, first):
    """flush() gathers a partly filled buffer on a stalled stream; after reset() a step on the OTHER stream is handed the same
    buffer and must not overwrite the slot the tail gather still has to read."""
    from lwsnet_amd.dist import StagedGather
    sa, sb = streams[first], streams[first + 1]
    sg = StagedGather(1, GH, GW, 2, dev, multi_stream=True)
    for t in (*sg.staging, *sg.recv[0], *sg.recv[1]):
        poison_(t)
    torch.cuda.synchronize()
    with torch.cuda.stream(sa):
        sg.slot().fill_(1.0)
        assert not sg.commit()
    with torch.cuda.stream(sb):
        ev = SS.stall(sb)
        sg.flush()
        SS.assert_still_stalled(ev, "flush")
        tail, n = sg.gathered(0)
        tail = tail.clone()
    sg.reset()
    with torch.cuda.stream(sa):
        sg.slot().fill_(2.0)                    # the same slot of the same buffer, from the stream that is not stalled
        sg.commit()
    SS.assert_still_stalled(ev, "the step behind flush")
    torch.cuda.synchronize()
    assert n == 1
    G.assert_bits(tail[:1], np.full((1, 1, GH, GW), 1.0, np.float32), "the slot gathered by flush()")


# ================================================================== g. the pipelined CLIs
IO_STALL_MS = SS.STALL_MS / 2       # six stalls a run: three pairs or batches, two kernels each


def stalling(monkeypatch, names, ms=IO_STALL_MS):
    """lwsnet_amd.ops.<name>, for every name, first stalls the current stream and then calls through; the op itself is
    asynchronous, so the stall must still hold when it returns.  Returns the calls counted per name."""
    from lwsnet_amd import ops
    calls = {n: 0 for n in names}

    def held(name, real):
        def op(*args, **kwargs):
            ev = SS.stall(torch.cuda.current_stream(), ms)
            out = real(*args, **kwargs)
            SS.assert_still_stalled(ev, f"ops.{name}")
            calls[name] += 1
            return out
        return op

    for n in names:
        monkeypatch.setattr(ops, n, held(n, getattr(ops, n)))
    return calls


def test_inference_pipeline_with_its_io_kernels_held_back(dev, hip_lib, tmp_path, monkeypatch):
    """The directory of tests/test_gpu_parity.py::test_cli_directory_pipeline_writes_identical_files, three pairs of it: the files
    written with lws_preprocess_rgb8 and lws_apply_lut8 behind stalls are, byte for byte, those of a calm run."""
    from PIL import Image
    from lwsnet_amd import inference as inf
    kp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_pair")
    l0 = np.asarray(Image.open(os.path.join(kp, "left_test.png")).convert("RGB"))
    r0 = np.asarray(Image.open(os.path.join(kp, "right_test.png")).convert("RGB"))
    src = tmp_path / "kitti"
    for d in ("image_2", "image_3"):
        (src / d).mkdir(parents=True)
    for i in range(3):
        Image.fromarray(np.roll(l0, 7 * i, axis=1)).save(src / "image_2" / f"{i:06d}_10.png")
        Image.fromarray(np.roll(r0, 7 * i, axis=1)).save(src / "image_3" / f"{i:06d}_10.png")

    def run(tag):
        out = tmp_path / tag
        written = inf.main(["--img_path", str(src), "--save_path", str(out), "--synthetic_weights", "--workers", "2", "--gpu_workers", "2"])
        assert len(written) == 3
        return {n: (out / n).read_bytes() for n in sorted(os.listdir(out))}

    calm = run("calm")
    assert len(set(calm.values())) == 3
    calls = stalling(monkeypatch, ("preprocess_rgb8", "apply_lut8"))
    assert run("stalled") == calm, "the files differ from the calm run's"
    assert calls == {"preprocess_rgb8": 3, "apply_lut8": 3}, calls


def test_evaluate_pipeline_with_its_io_kernels_held_back(dev, hip_lib, tmp_path, monkeypatch):
    """The synthetic KITTI set of tests/test_gpu_evaluate.py with --workers: five pairs in three batches.  With lws_preprocess_rgb8
    and lws_stage_metrics behind stalls every per-batch, per-image and average figure equals the calm run's exactly."""
    from lwsnet_amd import evaluate, synth
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, 5)
    argv = ["--synthetic_weights", "--test_batch_size", "2", "--dataset", "kitti2015", "--datapath", root, "--val_set", split, "--workers", "2"]
    calm = evaluate.main(argv)
    assert calm["pairs"] == 5 and calm["batches"] == 3
    calls = stalling(monkeypatch, ("preprocess_rgb8", "stage_metrics"))
    got = evaluate.main(argv)
    for k in ("average", "per_batch", "per_image"):
        assert got[k] == calm[k], k
    assert calls == {"preprocess_rgb8": 3, "stage_metrics": 3}, calls
