"""lws_tsdf_window on the device, bit for bit against the numpy restatement (tests/tsdf_window_reference.py), and the volume that
follows the camera on top of it.  The quad edges: rows of 13 voxels under every shift -5 .. 5 along x (every residue mod 4, both
signs) crossed with shifts along y and z; rows of 2 .. 9 voxels; rows of 16 voxels, where whole quads are loaded and stored as
16-byte words, with the source and the destination one element past a 16-byte boundary independently; more quads than the capped
grid has threads.  A shift of G or more, a shift of 0, a slab, a larger destination; NaN, +inf, -0.0 and negative weights, poison
under Wt == 0; C and counts given or NULL; the refusals, which leave the destination alone; guard bands; a stalled stream; a
captured graph.  Then TsdfVolume.shift: the conservation of the mesh, integration across a shift against the numpy pipeline, the
ray-cast after a shift, the bookkeeping, follow(); and the inference CLI with --tsdf_follow."""
import ctypes
import itertools

import numpy as np
import pytest

import guarded
import stream_stall as SS
import temporal_reference as TR
import tsdf_reference as R
import tsdf_window_reference as WR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_geometry import cu, misaligned  # noqa: E402
from test_gpu_tsdf import P, check_volume, grid, put_colour, raw_raycast, stream  # noqa: E402
from test_tsdf_window_cpu import G as G_MESH, SHIFTS, whole_mesh  # noqa: E402

F = np.float32
T_FILL, W_FILL, C_FILL, N_FILL = 7.0, -3.0, 0xA5, 77       # what an unwritten destination holds


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def raw_window(lib, dev, b, G, s, D, st=None):
    with torch.cuda.device(dev):
        return lib.lws_tsdf_window(P(b["T"]), P(b["Wt"]), P(b.get("C")), *G, *s, P(b["T2"]), P(b["Wt2"]), P(b.get("C2")), *D, P(b.get("counts")),
                                   st or stream())


def past_boundary(shape, dtype, fill, dev):
    """A filled tensor whose data starts one element past a 16-byte boundary (C: one 4-byte word past it)."""
    n = int(np.prod(shape))
    if dtype == torch.uint8:
        buf = torch.full((n + 4,), fill, dtype=dtype, device=dev)
        v = buf[4:].view(shape)
    else:
        buf = torch.full((n + 1,), fill, dtype=dtype, device=dev)
        v = buf[1:].view(shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def destination(dev, D, colour=True, counts=True, skew=False):
    shape = tuple(D)[::-1]
    make = (lambda sh, dt, fill: past_boundary(sh, dt, fill, dev)) if skew else (lambda sh, dt, fill: torch.full(sh, fill, dtype=dt, device=dev))
    b = dict(T2=make(shape, torch.float32, T_FILL), Wt2=make(shape, torch.float32, W_FILL))
    if colour:
        b["C2"] = make((*shape, 4), torch.uint8, C_FILL)
    if counts:
        b["counts"] = torch.full((2,), N_FILL, dtype=torch.int64, device=dev)
    return b


def source(dev, T, Wt, C, skew=False):
    put = (lambda a: misaligned(a, dev)) if skew else (lambda a: cu(a, dev))
    b = dict(T=put(T), Wt=put(Wt))
    if C is not None:
        b["C"] = put_colour(C, lambda a, name: put(a))
    return b


def check(b, want, what):
    guarded.assert_bits(b["Wt2"], want[1], what + " Wt2")
    guarded.assert_bits(b["T2"], want[0], what + " T2")
    if want[2] is not None and "C2" in b:
        guarded.assert_bits(b["C2"], want[2], what + " C2")
    if "counts" in b:
        assert b["counts"].tolist() == list(want[3]), (what, b["counts"].tolist(), want[3])


def run(lib, dev, vol, s, D=None, src=None, skew_dst=False, colour=True, counts=True, what=""):
    """One call on fresh, filled destinations, held to the restatement; src: the device source to reuse.  Returns the buffers."""
    from lwsnet_amd import _lib
    T, Wt, C = vol[:3]
    G = T.shape[::-1]
    D = G if D is None else D
    b = dict(src or source(dev, T, Wt, C if colour else None), **destination(dev, D, colour, counts, skew_dst))
    if not colour:
        b.pop("C", None)
    _lib.check(raw_window(lib, dev, b, G, s, D), "lws_tsdf_window")
    check(b, WR.window(T, Wt, C if colour else None, s, D), f"{what} G={G} s={s} D={D}")
    return b


# ---- 1. the quad edges ----
@pytest.mark.parametrize("sx", range(-5, 6))
def test_rows_of_13_voxels_under_every_shift_along_x(dev, hip_lib, sx):
    """Every residue of sx mod 4 with both signs, crossed with sy and sz in {-2, 0, 3}: quads that straddle the source's border at
    either end, rows that come from inside and from outside.  Rows of 13 voxels begin at every alignment: both paths are taken."""
    vol = WR.noise_volume((13, 6, 5), 20 + sx, holes=0.15, special=True)
    src = source(dev, *vol[:3])
    for sy, sz in itertools.product((-2, 0, 3), repeat=2):
        b = run(hip_lib, dev, vol, (sx, sy, sz), src=src)
    assert int(b["counts"].sum()) == 13 * 6 * 5


@pytest.mark.parametrize("Gx", [2, 3, 4, 5, 7, 8, 9])
def test_short_rows(dev, hip_lib, Gx):
    vol = WR.noise_volume((Gx, 3, 4), Gx, holes=0.2)
    src = source(dev, *vol[:3])
    for sx in (0, 1, -1, 2, 4, -4, Gx - 1, 1 - Gx):
        run(hip_lib, dev, vol, (sx, 1, -1), src=src)
        run(hip_lib, dev, vol, (sx, 0, 0), src=src, colour=False)


@pytest.mark.parametrize("skew_src,skew_dst", list(itertools.product((False, True), repeat=2)))
@pytest.mark.parametrize("Gx", [16, 13])
def test_bases_one_element_past_a_16_byte_boundary(dev, hip_lib, Gx, skew_src, skew_dst):
    """Rows of 16 voxels on aligned bases: every quad is a 16-byte word on both sides for sx = 0, 4, -8.  A source one element past
    the boundary is loaded voxel by voxel and stored as words, a destination there the other way round, and sx = 1, -3 undo or
    double the skew.  The bytes do not depend on the path."""
    vol = WR.noise_volume((Gx, 5, 4), 31, holes=0.1, special=True)
    src = source(dev, *vol[:3], skew=skew_src)
    assert src["T"].data_ptr() % 16 == (4 if skew_src else 0) and src["C"].data_ptr() % 16 == (4 if skew_src else 0)
    for sx in (0, 4, -8, 1, -3, 3):
        run(hip_lib, dev, vol, (sx, 1, 0), src=src, skew_dst=skew_dst, what=f"src skew {skew_src} dst skew {skew_dst}")


def test_more_quads_than_the_capped_grid_has_threads(dev, hip_lib):
    """132 x 128 x 128 voxels are 540672 quads, the grid 2048 workgroups of 256 threads = 524288: the last quads are a thread's second."""
    dims = (132, 128, 128)
    rng = np.random.default_rng(8)
    Wt = rng.choice(np.array([0.0, 1.0, 2.0], F), size=dims[::-1])
    T = rng.uniform(-1, 1, dims[::-1]).astype(F)
    C = rng.integers(0, 256, (*dims[::-1], 4), dtype=np.uint8)
    assert (dims[0] // 4) * dims[1] * dims[2] > 2048 * 256
    for s in ((4, -1, 2), (-3, 0, 0)):
        b = run(hip_lib, dev, (T, Wt, C), s)
        assert b["counts"][0] > 0


# ---- 2. shifts and shapes ----
@pytest.mark.parametrize("s", [(13, 0, 0), (-13, 0, 0), (0, 6, 0), (0, 0, -5), (4096, -4096, 4096), (12, 5, 4)])
def test_a_shift_of_the_volume_or_more_clears_everything(dev, hip_lib, s):
    vol = WR.noise_volume((13, 6, 5), 3)
    b = run(hip_lib, dev, vol, s)
    if s != (12, 5, 4):                                     # (one voxel stays: the far corner)
        assert b["counts"].tolist() == [0, 13 * 6 * 5] and not b["T2"].view(torch.int32).any() and not b["Wt2"].view(torch.int32).any() and not b["C2"].any()


def test_a_shift_of_zero_is_a_copy_that_scrubs_the_poison(dev, hip_lib):
    T, Wt, C, _, _ = vol = WR.noise_volume((13, 6, 5), 4, holes=0.3)
    b = run(hip_lib, dev, vol, (0, 0, 0))
    got_T, got_C = b["T2"].cpu().numpy(), b["C2"].cpu().numpy()
    dead = Wt == 0
    assert dead.any() and np.isnan(T[dead]).all() and (C[dead] == 0xA5).all()
    assert not got_T[dead].view(np.uint32).any() and not got_C[dead].any()
    assert got_T[~dead].tobytes() == T[~dead].tobytes() and (got_C[~dead] == C[~dead]).all()


@pytest.mark.parametrize("D,s", [((4, 6, 5), (0, 0, 0)), ((4, 6, 5), (9, 0, 0)), ((4, 6, 5), (11, 0, 0)), ((13, 2, 5), (0, 4, 0)), ((13, 6, 3), (0, 0, -1)),
                                 ((17, 9, 8), (0, 0, 0)), ((17, 9, 8), (-2, -1, -2)), ((20, 6, 5), (-3, 0, 0)), ((2, 2, 2), (5, 3, 2))])
def test_a_destination_of_another_size(dev, hip_lib, D, s):
    """Slabs and boxes cut out of the volume (what spill_boxes asks for) and destinations larger than the source."""
    vol = WR.noise_volume((13, 6, 5), 5, special=True)
    run(hip_lib, dev, vol, s, D=D)
    run(hip_lib, dev, vol, s, D=D, colour=False, counts=False)


# ---- 3. contents and arguments ----
def test_special_weights_and_what_lies_under_a_zero_weight(dev, hip_lib):
    """Wt of NaN, +inf and a negative number is live and moves with its bits; -0.0 is dead and leaves as +0.0; T = NaN and C = 0xA5
    under Wt == 0 come out as zeros."""
    dims = (9, 3, 2)
    Wt = np.ones(dims[::-1], F)
    T = np.arange(Wt.size, dtype=F).reshape(Wt.shape) - 20
    C = np.random.default_rng(1).integers(0, 256, (*Wt.shape, 4), dtype=np.uint8)
    row = Wt[0, 1]
    row[:5] = np.array([np.nan, np.inf, -0.0, 0.0, -2.5], F)
    row.view(np.uint32)[5] = 0x7FC00123                      # a NaN with a payload
    T[0, 1, 2:4] = WR.POISON_T
    C[0, 1, 2:4] = 0xA5
    for s in ((0, 0, 0), (1, 0, 0), (-2, 0, 0)):
        b = run(hip_lib, dev, (T, Wt, C), s)
    got = run(hip_lib, dev, (T, Wt, C), (0, 0, 0))
    w = got["Wt2"].cpu().numpy()[0, 1].view(np.uint32)
    assert w[:6].tolist() == [0x7FC00000, 0x7F800000, 0, 0, 0xC0200000, 0x7FC00123]
    assert got["T2"].cpu().numpy()[0, 1, 2:4].view(np.uint32).tolist() == [0, 0] and not got["C2"][0, 1, 2:4].any()
    assert got["counts"].tolist() == [Wt.size - 2, 2]
    del b


@pytest.mark.parametrize("colour,counts", [(True, False), (False, True), (False, False)])
def test_colour_and_counts_are_optional(dev, hip_lib, colour, counts):
    vol = WR.noise_volume((33, 4, 5), 6)
    for s in ((0, 0, 0), (4, 1, -1), (-5, 0, 2)):
        run(hip_lib, dev, vol, s, colour=colour, counts=counts)


def test_refusals_leave_the_destination_alone(dev, hip_lib):
    from lwsnet_amd import _lib, ops
    G = (13, 6, 5)
    vol = WR.noise_volume(G, 7)
    b = dict(source(dev, *vol[:3]), **destination(dev, G))
    flat = torch.full((2 * 13 * 6 * 5,), T_FILL, device=dev)
    n = 13 * 6 * 5
    cases = [
        (dict(C=None), G, (1, 0, 0), G, "C and C2 must be given together"), (dict(C2=None), G, (1, 0, 0), G, "C and C2 must be given together"),
        (dict(T2=b["T"]), G, (1, 0, 0), G, "T and T2 overlap"), (dict(Wt2=b["Wt"]), G, (0, 0, 0), G, "Wt and Wt2 overlap"),
        (dict(C2=b["C"]), G, (0, 0, 1), G, "C and C2 overlap"), (dict(T=flat[:n].view(5, 6, 13), T2=flat[n - 1:2 * n - 1].view(5, 6, 13)), G, (1, 0, 0), G, "T and T2 overlap"),
        (dict(Wt2=b["T2"]), G, (1, 0, 0), G, "Wt2 and T2 overlap"), (dict(counts=b["T2"].view(-1)[:4].view(torch.int64)), G, (1, 0, 0), G, "counts and T2 overlap"),
        ({}, (1, 6, 5), (0, 0, 0), G, "bad source volume 1x6x5"), ({}, G, (0, 0, 0), (13, 6, 4097), "bad destination volume 13x6x4097"),
        ({}, G, (4097, 0, 0), G, "bad shift (4097, 0, 0)"), ({}, G, (0, 0, -4097), G, "bad shift (0, 0, -4097)"),
        ({}, (2048, 1024, 1024), (0, 0, 0), G, "the source volume 2048x1024x1024 must hold fewer than 2^31 voxels"),
    ]
    for change, g, s, d, msg in cases:
        rc = raw_window(hip_lib, dev, {**b, **change}, g, s, d)
        assert rc == _lib.LWS_ERR_INVALID, (msg, rc)
        assert hip_lib.lws_last_error().decode().startswith("tsdf_window: " + msg), (msg, hip_lib.lws_last_error())
    torch.cuda.synchronize(dev)
    assert (b["T2"] == T_FILL).all() and (b["Wt2"] == W_FILL).all() and (b["C2"] == C_FILL).all() and (b["counts"] == N_FILL).all()
    guarded.assert_bits(b["T"], vol[0], "the source after the refusals")
    with pytest.raises(ValueError, match="tsdf_window: T and T2 overlap"):
        ops.tsdf_window(b["T"], b["Wt"], (1, 0, 0), C=b["C"], out=(b["T"], b["Wt2"], b["C2"]))


# ---- 4. the contract ----
@pytest.mark.parametrize("word", guarded.FLOAT_WORDS, ids=guarded.word_id)
def test_memory_contract(dev, hip_lib, word):
    """Every buffer between poisoned flanks and one element past a 16-byte boundary, the outputs poisoned inside; T holds the poison
    word wherever Wt == 0.  A box, a shift and a larger destination; two runs give the same bytes."""
    from lwsnet_amd import _lib
    G = (33, 7, 9)
    T, Wt, C, _, _ = WR.noise_volume(G, 9, holes=0.2)
    T = np.where(Wt == 0, np.array([word], np.uint32).view(F)[0], T).astype(F)
    for s, D in (((4, -2, 3), G), ((-1, 0, 0), G), ((30, 0, 0), (4, 7, 9)), ((-3, -1, -1), (40, 9, 11))):
        runs = []
        for _ in range(2):
            gd = guarded.Guard(dev, word, skew=1)
            b = dict(T=gd.place(T, name="T"), Wt=gd.place(Wt, name="Wt"), C=put_colour(C, lambda a, name: gd.place(a, name=name)),
                     T2=gd.empty(D[::-1], F, name="T2"), Wt2=gd.empty(D[::-1], F, name="Wt2"),
                     C2=gd.empty(D[::-1], np.int32, name="C2").view(torch.uint8).view(*D[::-1], 4), counts=gd.empty((2,), np.int64, align16=True, name="counts"))
            _lib.check(raw_window(hip_lib, dev, b, G, s, D), "lws_tsdf_window")
            check(b, WR.window(T, Wt, C, s, D), f"guarded s={s} D={D}")
            gd.check()
            runs.append([b[k].cpu().numpy().tobytes() for k in ("T2", "Wt2", "C2", "counts")])
        assert runs[0] == runs[1]


def test_the_call_runs_on_the_stream_it_is_given(dev, hip_lib):
    """The scenario of tests/test_gpu_tsdf_mesh.py restated for this call: source and destination hold poison, the caller's stream is
    stalled, the copies that bring the real volume are queued behind the stall and the call behind them.  The call returns while the
    stream is still held; read from another stream meanwhile, no output byte has changed; once the stall ends the outputs are the
    calm run's.  A reading stream that shares a hardware queue with the caller's waits for the stall itself and is not judged, but
    on one caller stream at least the read must fall inside the stall."""
    from lwsnet_amd import _lib
    from test_gpu_stream_order import poison_, poisoned, still_poison
    G, s = (33, 4, 5), (4, 1, -1)
    vol = WR.noise_volume(G, 10)
    want = WR.window(*vol[:3], s)
    src = source(dev, *vol[:3])
    SS.ticks_per_ms(dev)
    calm = dict(src, **destination(dev, G))
    _lib.check(raw_window(hip_lib, dev, calm, G, s, G), "lws_tsdf_window")       # calmly first: the kernels are loaded
    poison_(torch.empty_like(src["T"])).copy_(src["T"])
    poison_(torch.empty((8,), dtype=torch.uint8, device=dev)).clone()
    torch.cuda.synchronize()
    check(calm, want, "calm")
    names = ("T2", "Wt2", "C2", "counts")
    other, seen_held = torch.cuda.Stream(device=dev), 0
    for i, st in enumerate(SS.caller_streams(dev)):
        b = {k: poisoned(v.shape, v.dtype, dev) for k, v in calm.items()}
        torch.cuda.synchronize()
        with torch.cuda.device(dev), torch.cuda.stream(st):
            ev = SS.stall(st)
            for k in ("T", "Wt", "C"):
                b[k].copy_(src[k], non_blocking=True)
            _lib.check(raw_window(hip_lib, dev, b, G, s, G, st=ctypes.c_void_p(st.cuda_stream)), "lws_tsdf_window")
        SS.assert_still_stalled(ev, f"lws_tsdf_window on caller stream {i}")
        with torch.cuda.stream(other):
            early = [b[k].clone() for k in names]
            other.synchronize()
        if not ev.query():                                  # the read ran while the caller's stream was held
            assert all(still_poison(e.cpu().numpy()) for e in early), f"caller stream {i}: an output changed while the stream was held"
            seen_held += 1
        st.synchronize()
        check(b, want, f"caller stream {i}")
    assert seen_held > 0, "the reading stream shared a hardware queue with every caller stream: no read fell inside a stall"


def test_graph_capture_replays_against_the_direct_call(dev, hip_lib):
    from lwsnet_amd import _lib
    G, s, D = (33, 7, 9), (5, -1, 2), (33, 7, 9)
    first, second = WR.noise_volume(G, 11), WR.noise_volume(G, 12, holes=0.3)
    b = dict(source(dev, *first[:3]), **destination(dev, D))
    _lib.check(raw_window(hip_lib, dev, b, G, s, D), "lws_tsdf_window")           # the code objects are loaded before the capture
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lib.check(raw_window(hip_lib, dev, b, G, s, D), "lws_tsdf_window")
    for T, Wt, C, _, _ in (first, second, first):
        b["T"].copy_(cu(T, dev))
        b["Wt"].copy_(cu(Wt, dev))
        b["C"].copy_(put_colour(C, lambda a, name: cu(a, dev)))
        for k, fill in (("T2", T_FILL), ("Wt2", W_FILL), ("C2", C_FILL), ("counts", N_FILL)):
            b[k].fill_(fill)
        graph.replay()
        torch.cuda.synchronize(dev)
        check(b, WR.window(T, Wt, C, s, D), "replay")
        direct = dict(b, **destination(dev, D))
        _lib.check(raw_window(hip_lib, dev, direct, G, s, D), "lws_tsdf_window")
        for k in ("T2", "Wt2", "C2", "counts"):
            assert torch.equal(direct[k].view(torch.uint8), b[k].view(torch.uint8)), k


# ---- 5. the volume that moves ----
def volume_of(dev, T, Wt, C, origin, vs, **kw):
    from lwsnet_amd.tsdf import TsdfVolume
    vol = TsdfVolume(origin, vs, T.shape[::-1], colour=C is not None, device=dev, **{"mu0": 3 * vs, **kw})
    vol.T.copy_(cu(T, dev))
    vol.Wt.copy_(cu(Wt, dev))
    if C is not None:
        vol.C.copy_(cu(C, dev))
    return vol


@pytest.mark.parametrize("shift", SHIFTS)
def test_the_mesh_is_conserved_on_the_device(dev, hip_lib, shift):
    """TsdfVolume.shift(spill="mesh"): the triangles the chunks hold plus those of the shifted volume are the triangles of the whole
    volume (computed once, on the CPU), as triples of 16-byte vertex records, bit for bit."""
    from lwsnet_amd.tsdf import spill_boxes
    w = whole_mesh()
    T, Wt, C, origin, vs = w["volume"]
    vol = volume_of(dev, T, Wt, C, origin, vs)
    before = vol.T.data_ptr()
    chunks = vol.shift(*shift, spill="mesh", max_points=4096, max_faces=4096)
    assert len(chunks) == len(spill_boxes(G_MESH, shift)) and vol.T.data_ptr() != before
    assert vol.offset.tolist() == list(shift) and np.array(vol.origin, F).tobytes() == np.array(WR.moved_origin(origin, shift, vs), F).tobytes()
    want = WR.window(T, Wt, C, shift)
    check(dict(T2=vol.T, Wt2=vol.Wt, C2=vol.C, counts=vol.kept), want, f"shift {shift}")
    parts = []
    for c in chunks + [vol.chunk("mesh", max_points=4096, max_faces=4096)]:
        assert c.points.shape[1:] == (16,) and c.vnormals.shape == (len(c.points), 4) and c.faces.dtype == np.int32
        assert len(c.faces) == 0 or (c.faces.min() >= 0 and c.faces.max() < len(c.points))
        parts += WR.triangles(c.points, c.faces)
    assert sorted(parts) == w["triangles"]
    # the points alone: every chunk's records are those of its mesh
    again = volume_of(dev, T, Wt, C, origin, vs)
    for c, m in zip(again.shift(*shift, spill="points", max_points=4096), chunks):
        assert c.points.tobytes() == m.points.tobytes() and len(c.faces) == 0
    with pytest.raises(ValueError, match="more than max_points"):
        volume_of(dev, T, Wt, C, origin, vs).shift(*shift, spill="mesh", max_points=3, max_faces=4096)


def test_shifting_does_not_disturb_what_stays(dev, hip_lib):
    """On a grid whose voxel centres are exact floats: two frames of tsdf_reference.integrate_case, a shift by (2, -1, 3), a third
    frame -- the numpy pipeline in bits.  And on the voxels whose source was inside, integrating the third frame and then windowing
    equals windowing and then integrating."""
    from lwsnet_amd import ops
    from lwsnet_amd.geometry import Camera
    dims, hw, s = (65, 7, 9), (48, 96), (2, -1, 3)
    c = R.integrate_case(dims, hw, 3, i=3)                           # the case of this volume and map with every optional input given
    origin, vs = c["origin"], c["vs"]
    assert all(float(F(o)) == o for o in origin) and vs == 0.125 and all(c[k] is not None for k in ("rgb", "sigma", "mask", "normals"))
    f = c["cam"][0]
    cams = Camera(float(f[0]), float(f[1]), float(f[2]), float(f[3]), 4.0)          # one camera for every frame
    assert np.array_equal(cams.row(), f)
    kw = {**{k: v for k, v in c["kw"].items() if k != "wmode"}, "weight": ("unit", "sigma")[c["kw"]["wmode"]]}
    part = lambda a, i: None if a is None else a[i]                  # noqa: E731
    dv = lambda a: None if a is None else cu(a, dev)                 # noqa: E731

    def integrate_on_device(vol, i):
        return ops.tsdf_integrate(vol.T, vol.Wt, vol.origin, vol.voxel, dv(c["disp"][i]), cams, c["pose"][i], C=vol.C, sigma=dv(part(c["sigma"], i)),
                                  mask=dv(part(c["mask"], i)), normals=dv(part(c["normals"], i)), rgb=dv(part(c["rgb"], i)), **kw)

    def integrate_in_numpy(state, o, i):
        return R.integrate(*state, o, vs, c["disp"][i], c["cam"][i], c["pose"][i], part(c["sigma"], i), part(c["mask"], i), part(c["normals"], i),
                           part(c["rgb"], i), **c["kw"])

    vol = volume_of(dev, c["T0"], c["W0"], c["C0"], origin, vs, **{k: v for k, v in kw.items() if k in ("mu0", "mu_d", "weight", "w_max")})
    integrate_on_device(vol, slice(0, 2))
    two = integrate_in_numpy((c["T0"], c["W0"], c["C0"]), origin, slice(0, 2))
    check_volume(dict(T=vol.T, Wt=vol.Wt, C=vol.C), two, "two frames")
    early = volume_of(dev, *two[:3], origin, vs)                     # the other order: the third frame first, then the window
    assert vol.shift(*s) == []
    moved = WR.window(*two[:3], s)
    check(dict(T2=vol.T, Wt2=vol.Wt, C2=vol.C, counts=vol.kept), moved, "the shift")
    upd = integrate_on_device(vol, slice(2, 3))
    want = integrate_in_numpy(moved[:3], WR.moved_origin(origin, s, vs), slice(2, 3))
    assert int(upd[0]) == int(want[3][0]) > 0
    check_volume(dict(T=vol.T, Wt=vol.Wt, C=vol.C), want, "a third frame after the shift")
    integrate_on_device(early, slice(2, 3))
    early.shift(*s)
    inside = np.zeros(dims[::-1], bool)
    inside[:dims[2] - s[2], 1:, :dims[0] - s[0]] = True             # the destination voxels whose source lay inside the volume
    assert inside.sum() == (65 - 2) * (7 - 1) * (9 - 3)
    for a, b in ((early.T, vol.T), (early.Wt, vol.Wt), (early.C.view(torch.int32).squeeze(-1), vol.C.view(torch.int32).squeeze(-1))):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        assert a[inside].tobytes() == b[inside].tobytes()
    assert (vol.Wt.cpu().numpy()[~inside] != 0).sum() == 339          # the third frame wrote into what had come in: the orders differ there


def test_the_raycast_after_a_shift(dev, hip_lib):
    T, Wt, origin, vs = R.crafted_volume()
    cam, pose = R.raycast_views()
    H, W, s, kw = 24, 40, (2, -1, 3), R.RAYCASTS[0]
    assert all(float(F(o)) == o for o in origin)
    vol = volume_of(dev, T, Wt, None, origin, vs)
    vol.shift(*s)
    T2, Wt2, _, _ = WR.window(T, Wt, None, s)
    want = R.raycast(T2, Wt2, WR.moved_origin(origin, s, vs), vs, cam, pose, H, W, **kw)
    assert (want[0] > 0).any()
    b = dict(T=vol.T, Wt=vol.Wt, cam=cu(cam, dev), pose=cu(pose, dev), disp=torch.full((3, 1, H, W), 7.0, device=dev),
             weight=torch.full((3, 1, H, W), 7.0, device=dev), normals=torch.full((3, 3, H, W), 7.0, device=dev))
    raw_raycast(hip_lib, dev, b, (3, H, W), grid(vol.dims, vol.origin, vs), kw["z_near"], kw["step"], kw["nsteps"])
    for key, w in zip(("disp", "weight", "normals"), want):
        guarded.assert_bits(b[key], w, key + " after the shift")


def test_the_bookkeeping_of_a_volume_that_follows(dev, hip_lib):
    """Two sets of tensors, swapped by each move; origin0 and the integer offset; a move and its reverse restore the origin's bits
    (and clear what had left); follow() moves once the anchor is `step` voxels from the centre, by the rounded difference."""
    T, Wt, C, _, _ = WR.noise_volume((13, 6, 5), 13)
    origin, vs = (-1.3, 0.7, 0.1), 0.2
    vol = volume_of(dev, T, Wt, C, origin, vs)
    first = np.array(vol.origin, F).tobytes()
    sets = [(vol.T.data_ptr(), vol.Wt.data_ptr(), vol.C.data_ptr())]
    assert vol.shift(0, 0, 0, spill="mesh") == [] and vol.T.data_ptr() == sets[0][0] and vol.kept is None
    for s in ((3, 0, 1), (-3, 0, -1), (1, 1, 1)):
        vol.shift(*s)
        sets.append((vol.T.data_ptr(), vol.Wt.data_ptr(), vol.C.data_ptr()))
    assert sets[0] != sets[1] and sets[2] == sets[0] and sets[3] == sets[1]
    assert vol.offset.tolist() == [1, 1, 1] and vol.grid[:3] == (13, 6, 5) and tuple(vol.grid[3:6]) == vol.origin
    want = WR.window(*WR.window(*WR.window(T, Wt, C, (3, 0, 1))[:3], (-3, 0, -1))[:3], (1, 1, 1))
    check(dict(T2=vol.T, Wt2=vol.Wt, C2=vol.C, counts=vol.kept), want, "three moves")
    vol.shift(-1, -1, -1)
    assert np.array(vol.origin, F).tobytes() == first and vol.offset.tolist() == [0, 0, 0]
    assert np.allclose(vol.centre(), np.array(origin) + np.array([6.0, 2.5, 2.0]) * vs, rtol=0, atol=1e-12)
    pose = np.hstack([np.eye(3), [[0.0], [0.0], [0.0]]])
    anchor = vol.centre()
    assert vol.follow(pose, anchor, 2) == ((0, 0, 0), [])
    pose[:, 3] = (0.39, 0.0, -0.1)                                  # 1.95 voxels: not yet
    assert vol.follow(pose, anchor, 2) == ((0, 0, 0), [])
    pose[:, 3] = (0.41, 0.0, -0.11)                                 # 2.05, 0, -0.55 voxels
    s, chunks = vol.follow(pose, anchor, 2, spill="points", max_points=4096)
    assert s == (2, 0, -1) and len(chunks) == 2 and vol.offset.tolist() == [2, 0, -1]
    assert vol.follow(pose, anchor, 2)[0] == (0, 0, 0)              # the centre has caught up
    for bad in (dict(spill="cloud"), dict(max_points=0, spill="points")):
        with pytest.raises(ValueError):
            vol.shift(1, 0, 0, **bad)
    with pytest.raises(ValueError, match=r"offset\[0\]"):
        vol.shift(5000, 0, 0)
    assert vol.offset.tolist() == [2, 0, -1]


# ---- 6. the CLI ----
CLI_VOLUME = ["--tsdf_voxel", "0.4", "--tsdf_extent", "-8", "8", "-3.2", "3.2", "0", "32"]          # 41 x 17 x 81 voxels


def cli_run(tmp_path, name, zs, more, caplog):
    """inference.main over a synthetic sequence of len(zs) pairs whose camera stands zs[k] metres ahead of the first, with both TSDF
    files; -> (the log lines, the point file, the mesh file)."""
    import logging
    import os
    from lwsnet_amd import inference, synth
    from test_gpu_geometry import KITTI15_CALIB
    root = str(tmp_path / "kitti")
    if not os.path.isdir(root):
        synth.write_kitti_tree(root, len(zs))
        (tmp_path / "calib.txt").write_text(KITTI15_CALIB.format(fx=721.5377, cx=609.5593, cy=172.854, t3=44.85728 - 0.54 * 721.5377))
        (tmp_path / "poses.txt").write_text("".join(" ".join(repr(float(v)) for v in TR.forward_pose(1, z).reshape(12)) + "\n" for z in zs))
    ply, mesh = tmp_path / f"{name}_points.ply", tmp_path / f"{name}_mesh.ply"
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="lwsnet_amd.inference"):
        written = inference.main(["--img_path", root + "/", "--synthetic_weights", "--calib", str(tmp_path / "calib.txt"), "--occ_check", "1",
                                  "--save_path", str(tmp_path / f"out_{name}"), "--tsdf", "--poses", str(tmp_path / "poses.txt"), *CLI_VOLUME,
                                  "--save_tsdf_ply", str(ply), "--save_tsdf_mesh", str(mesh), *more])
    assert written[-2:] == [str(ply), str(mesh)]
    return [r.getMessage() for r in caplog.records], ply, mesh


def updated_per_frame(lines):
    import re
    return [int(m[1]) for m in (re.fullmatch(r"TSDF: voxels updated = (\d+)", line) for line in lines) if m]


def test_inference_cli_follows_the_camera_out_of_the_box(dev, hip_lib, tmp_path, caplog):
    """Three frames 0.3 m apart (what the mesh's own CLI test integrates: enough for faces), a jump of 20 m, three more, a jump of
    20 m and a last frame: the jumps are 52 and 51 voxels of a volume 81 long.  Without the flag the last frame stands 9 m past
    the volume's far end and takes no voxel; with --tsdf_follow 2 the volume has moved twice, each time spilling a slab as a mesh,
    the frame takes voxels, and both files hold the three chunks."""
    import re
    from lwsnet_amd.geometry import read_mesh_ply
    zs = [0.0, 0.3, 0.6, 20.7, 21.0, 21.3, 41.3]
    n = len(zs)
    lines, ply, mesh = cli_run(tmp_path, "follow", zs, ["--tsdf_follow", "2"], caplog)
    moves = [tuple(int(v) for v in m.groups()) for m in
             (re.fullmatch(r"TSDF: followed by \((-?\d+), (-?\d+), (-?\d+)\) voxels, kept = (\d+), spilled vertices = (\d+), faces = (\d+)", line) for line in lines) if m]
    assert [m[:3] for m in moves] == [(0, 0, 52), (0, 0, 51)] and all(m[4] > 0 for m in moves) and moves[0][5] > 0, moves
    assert any(re.fullmatch(r"TSDF: 3 chunks, vertices at a place an earlier vertex holds \(the seams\) = \d+", line) for line in lines), lines
    updated = updated_per_frame(lines)
    assert len(updated) == n and all(u > 0 for u in updated), updated
    cloud, none = read_mesh_ply(str(ply))
    verts, faces = read_mesh_ply(str(mesh))
    assert len(none) == 0 and len(verts) > 0 and len(faces) > 0 and verts.tobytes() == cloud.tobytes()
    assert faces.min() >= 0 and faces.max() < len(verts)
    assert len(verts) >= sum(m[4] for m in moves) and len(faces) >= sum(m[5] for m in moves)
    logged = [(int(m[1]), int(m[2])) for m in (re.fullmatch(r"Save TSDF mesh = .*, vertices = (\d+), faces = (\d+)", line) for line in lines) if m]
    assert logged == [(len(verts), len(faces))]
    z = verts["z"]
    assert z.max() > 32.0 + 0.4                                     # the map reaches past the far end of the first box
    lines, _, _ = cli_run(tmp_path, "fixed", zs, [], caplog)
    fixed = updated_per_frame(lines)
    assert len(fixed) == n and fixed[0] > 0 and fixed[-1] == 0, fixed
    assert not any(line.startswith("TSDF: followed") for line in lines)


def test_inference_cli_a_step_too_large_to_move_changes_no_file(dev, hip_lib, tmp_path, caplog):
    """0.3 m a frame is less than a voxel: with N = 14 nothing moves, and every file is the file of the run without the flag."""
    import os
    lines, ply, mesh = cli_run(tmp_path, "still", [0.0, 0.3], ["--tsdf_follow", "14"], caplog)
    assert not any(line.startswith("TSDF: followed") for line in lines) and all(u > 0 for u in updated_per_frame(lines))
    _, ply0, mesh0 = cli_run(tmp_path, "plain", [0.0, 0.3], [], caplog)
    assert ply.read_bytes() == ply0.read_bytes() and mesh.read_bytes() == mesh0.read_bytes() and ply.stat().st_size > 1000
    a, b = tmp_path / "out_still", tmp_path / "out_plain"
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and len(os.listdir(a)) > 0
    for name in os.listdir(a):
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
