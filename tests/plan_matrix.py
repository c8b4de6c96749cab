"""The launch plans of lws_forward crossed with the shapes and batches at which its host predicates flip, and a host-side model
of which launches each cell makes.

lws_forward has a family of launch lists.  Options choose among them (include/lwsnet_hip.h, lws_set_option) and so do host
predicates on the shape (lwsnet_amd/csrc/lws_forward.hip): defers(), the integer-ratio test of stage_map(), the automatic
"fuse_ref_last", the refinement's chunk count and its `pipe`.  The header promises the same bits for every setting; this module
says at which (plan, shape, batch) cells that promise is checked (tests/test_gpu_plan_matrix.py), and `expected_launches`
restates the host logic so that the library's own profiler (lws_profile_read) shows which side of each predicate a cell took.
tests/test_plan_matrix_cpu.py keeps the matrix from shrinking: every predicate must keep cells on both sides, per cause.

Pure Python: nothing here imports torch or the library.
"""

# tests/test_gpu_parity.py::test_forward_schedule_options runs these at 64x256 (it imports the list from here)
OPTION_PLANS = [{"fuse_first": 0}, {"fuse_first": 1}, {"fuse_first": 2}, {"defer_upsample": 0}, {"ref_chunk_mb": 0}, {"ref_chunk_mb": 1},
                {"side_streams": 0}, {"side_streams": 0, "fuse_first": 0}, {"warp_form": 0}, {"warp_form": 0, "defer_upsample": 0},
                {"fuse_last1": 0}, {"fuse_last1": 1, "warp_form": 0}, {"fuse_ref_last": 0}, {"fuse_ref_last": 1},
                {"fork2_after": 0}, {"fork2_after": 2}, {"fork2_after": 1, "side_streams": 0}, {"ref_pipe": 1, "ref_chunk_mb": 1},
                {"ref_pipe": 0, "ref_chunk_mb": 1},
                {"fuse_first": 0, "defer_upsample": 0, "fuse_last1": 0, "fuse_ref_last": 0, "fork2_after": 0, "warp_form": 0}]
ALL_OFF_PLAN = OPTION_PLANS[-1]

PLANS = OPTION_PLANS + [{"host_joins": 0}, {"host_joins": 1}, {"host_joins": 1, "host_join_budget_us": 0},
                        {"fuse_ref_last": 1, "ref_chunk_mb": 1}, {"fuse_ref_last": 0, "fuse_last1": 0},
                        {"ref_pipe": 1, "ref_chunk_mb": 1, "fork2_after": 1},
                        {"side_streams": 0, "ref_pipe": 1, "ref_chunk_mb": 1},        # (the pipe must stay off)
                        {"defer_upsample": 0, "fuse_ref_last": 1}, {}]

# the options' defaults (lws_common.h, lws_ctx::opt; documented in include/lwsnet_hip.h)
OPTION_DEFAULTS = {"fuse_first": 3, "defer_upsample": 1, "side_streams": 1, "ref_chunk_mb": 72, "ref_pipe": -1, "warp_form": 1,
                   "fuse_last1": 1, "fork2_after": -1, "fuse_ref_last": -1, "host_joins": -1, "host_join_budget_us": 900}

# The smallest legal sizes of each class (legal: ceil(H/2) % 4 == 0, ceil(W/2) % 4 == 0, ceil(W/2) / 4 >= maxdisplist[0] = 24)
SHAPES = [(8, 192),       # one row of stage-1 tiles, the smallest input
          (16, 192),      # even, every resize ratio an integer
          (24, 200),      # even, 25 / 50 / 100 columns: partial tiles, deferral allowed
          (15, 191),      # both sides odd
          (16, 199),      # W odd only
          (23, 200),      # H odd only
          (63, 255),      # odd, several tile rows
          (40, 264)]      # even, 33 / 66 / 132 columns
LARGE_SHAPES = ((63, 255), (40, 264))          # batches 1, 2, 3 only: the C oracle takes 0.6 - 0.9 s per pair there
# With "ref_chunk_mb" = 1 one [H,W,32] map of 15x191 is 0.367 MB, so a chunk is CH = 2 pairs: batch 8 is four chunks (the
# automatic "ref_pipe" switches on), batch 3 a chunk of two and a ragged chunk of one.
BATCHES = {shape: (1, 2, 3) if shape in LARGE_SHAPES else (1, 2, 3, 5) + ((8,) if shape == (15, 191) else ())
           for shape in SHAPES}

# The order one handle walks the shapes in: large, small, large (a slab sized for the largest is reused, stale, by the smallest,
# and the geometry changes under whatever plan the handle carries)
WALK = [(63, 255), (8, 192), (40, 264), (15, 191), (24, 200), (16, 199), (16, 192), (23, 200)]

MODELLED_CLASSES = ("volume_l1_shift+conv3d_first", "volume_l1_warp", "conv3d_mid16", "conv3d_mid8", "conv3d_last", "softargmin",
                    "upsample_add", "feature_conv2d", "ref_first", "ref_dws", "ref_conv64", "ref_last", "softargmin_conf")


def plan_id(plan):
    return ",".join(f"{k}={v}" for k, v in plan.items()) or "default"


def half_up(v):
    return (v + 1) // 2


def size_ok(H, W, maxdisp0=24):
    """check_size (lws_forward.hip)"""
    return H > 0 and W > 0 and half_up(H) % 4 == 0 and half_up(W) % 4 == 0 and half_up(W) // 4 >= maxdisp0


def refine_chunk(ref_chunk_mb, B, H, W):
    """refine_chunk (lws_forward.hip): pairs per refinement chunk, the same double arithmetic"""
    if ref_chunk_mb <= 0:
        return B
    map_mb = float(H) * W * 128.0 / 1e6
    c = max(int(float(ref_chunk_mb) / map_mb), 1)
    return min(c, B)


def _last_can_fuse(c3, D):
    """conv3d_last_can_fuse (lws_conv3d.hip)"""
    return (D == 9 and c3 in (8, 16)) or (c3 == 32 and D in (24, 32))


def expected_launches(plan, args, B, H, W, conf=False):
    """Per-class launch counts of ONE lws_forward (conf: lws_forward_conf) under `plan` for the model `args` describes, and the
    host predicates they follow from.  Restated from include/lwsnet_hip.h (the options) and the host code of run_forward,
    stage_volume, stage_map, refine_left and refine_rest in lws_forward.hip; the *_can_fuse predicates from lws_conv3d.hip /
    lws_refine.hip.  Keys: the profiler's class names (lws_kernel_class_name), "volume_l1_shift" and "conv3d_first" as their sum
    (which of the two builds the stage-1 volume depends on the packed weights, not on the plan), and the derived
    "defers" / "integer_ratio" / "fused" (per stage), "fuse_ref_last", "CH", "nchunks", "ragged", "pipe", "total"."""
    o = dict(OPTION_DEFAULTS)
    o.update(plan)
    L3 = int(args.layers_3d)
    c3 = [int(args.channels_3d) * int(g) for g in args.growth_rate]
    n = {k: 0 for k in MODELLED_CLASSES}
    n["feature_conv2d"] = 8                                   # feature_head 4 pair launches, feature_tail 1 + 3
    # the refinement's first block evaluates (and writes out) a deferred stage-3 map: dilation 2 always fuses
    ref_evaluates = bool(o["fuse_first"] & 1)
    even = H % 2 == 0 and W % 2 == 0
    defers, integer, fused = [], [], []
    written = [False, False, False]
    for s in range(3):
        m = int(args.maxdisplist[s])
        D = m if s == 0 else 2 * m - 1
        div = 4 >> s
        hh, ww = half_up(H) // div, half_up(W) // div
        keep = s < 2 or ref_evaluates
        d = (not conf) and keep and o["defer_upsample"] != 0 and B <= 2 and even and (s > 0 or o["fuse_last1"] != 0)
        defers.append(d)
        integer.append(H % hh == 0 and W % ww == 0)
        # stage_volume
        n["volume_l1_shift+conv3d_first"] += 1
        if s > 0:
            n["volume_l1_warp"] += 1
            # k_volume_l1_warp writes a deferred map (and a deferred map before it) out where the stage is at half resolution
            if not written[s - 1] and H == 2 * hh and W == 2 * ww:
                written[s - 1] = True
                if s == 2:
                    written[0] = True
        n["conv3d_mid16" if c3[s] != 8 else "conv3d_mid8"] += L3
        n["conv3d_last"] += 1
        f = (not conf) and (s > 0 or d) and _last_can_fuse(c3[s], D)
        fused.append(f)
        # stage_map
        if not (f and d):
            if s > 0 and not written[s - 1]:
                n["upsample_add"] += 1
                written[s - 1] = True
            if not f:
                n["softargmin"] += 1
                if not integer[s]:
                    n["upsample_add"] += 1
            else:
                n["upsample_add"] += 1
            written[s] = True
        if conf:
            n["softargmin_conf"] += 1
    # refine_left: every chunk runs refinement1_left's five layers
    CH_left = refine_chunk(o["ref_chunk_mb"], B, H, W)
    chunks_left = -(-B // CH_left)
    n["ref_dws"] += 4 * chunks_left
    if not o["fuse_first"] & 2:
        n["ref_first"] += chunks_left
    # refine_rest: a deferred stage-3 map is one chunk
    CH = refine_chunk(o["ref_chunk_mb"], B, H, W) if written[2] else B
    nchunks = -(-B // CH)
    fuse_ref_last = o["fuse_ref_last"] != 0 if o["fuse_ref_last"] >= 0 else B <= 1
    want = o["ref_pipe"] if o["ref_pipe"] >= 0 else (1 if nchunks >= 4 else 0)
    pipe = want != 0 and o["side_streams"] != 0 and nchunks >= 2 and 2 * CH <= B
    n["ref_dws"] += (4 + 3 + (0 if fuse_ref_last else 1)) * nchunks
    if not o["fuse_first"] & 1:
        n["ref_first"] += nchunks
    n["ref_conv64"] += nchunks
    n["ref_last"] += nchunks
    n["total"] = sum(n[k] for k in MODELLED_CLASSES)
    n.update(defers=defers, integer_ratio=integer, fused=fused, fuse_ref_last=fuse_ref_last, CH=CH, nchunks=nchunks,
             ragged=B % CH != 0, pipe=pipe)
    return n


def cells(plans=None, shapes=None, batches=None):
    plans = PLANS if plans is None else plans
    shapes = SHAPES if shapes is None else shapes
    batches = BATCHES if batches is None else batches
    for plan in plans:
        for shape in shapes:
            for B in batches[shape]:
                yield plan, shape, B


def coverage(plans, shapes, batches, args):
    """For every host predicate, the cells (plan id, shape, B) on each side of it, split by cause.  Keys are
    "<predicate>:<side or cause>"; tests/test_plan_matrix_cpu.py requires every list to be non-empty."""
    cov = {k: [] for k in (
        "defers:off by defer_upsample=0", "defers:off by B>=3", "defers:off by odd H", "defers:off by odd W",
        "defers:stage 1 off by fuse_last1=0", "defers:on at B=1", "defers:on at B=2", "defers:stage 3 off by fuse_first bit 0",
        "integer_ratio:yes", "integer_ratio:no",
        "fuse_ref_last:automatic on", "fuse_ref_last:automatic off", "fuse_ref_last:forced on at B>=2",
        "fuse_ref_last:forced on at an odd size", "fuse_ref_last:forced off at B=1",
        "nchunks:1", "nchunks:2", "nchunks:>=4", "nchunks:ragged last chunk",
        "pipe:on by option", "pipe:on automatically", "pipe:refused by side_streams=0", "pipe:refused by 2*CH>B")}
    for plan, (H, W), B in cells(plans, shapes, batches):
        o = dict(OPTION_DEFAULTS)
        o.update(plan)
        e = expected_launches(plan, args, B, H, W)
        cell = (plan_id(plan), (H, W), B)
        even = H % 2 == 0 and W % 2 == 0

        def hit(key, cond):
            if cond:
                cov[key].append(cell)
        # deferral: each "off" cause alone (everything else would have allowed it)
        hit("defers:off by defer_upsample=0", o["defer_upsample"] == 0 and B <= 2 and even and not any(e["defers"]))
        hit("defers:off by B>=3", o["defer_upsample"] != 0 and B >= 3 and even and not any(e["defers"]))
        hit("defers:off by odd H", o["defer_upsample"] != 0 and B <= 2 and H % 2 == 1 and W % 2 == 0 and not any(e["defers"]))
        hit("defers:off by odd W", o["defer_upsample"] != 0 and B <= 2 and H % 2 == 0 and W % 2 == 1 and not any(e["defers"]))
        hit("defers:stage 1 off by fuse_last1=0", o["fuse_last1"] == 0 and not e["defers"][0] and e["defers"][1])
        hit("defers:stage 3 off by fuse_first bit 0", not (o["fuse_first"] & 1) and e["defers"][1] and not e["defers"][2])
        hit("defers:on at B=1", B == 1 and all(e["defers"]))
        hit("defers:on at B=2", B == 2 and all(e["defers"]))
        hit("integer_ratio:yes", all(e["integer_ratio"]))
        hit("integer_ratio:no", not any(e["integer_ratio"]))
        auto = o["fuse_ref_last"] < 0
        hit("fuse_ref_last:automatic on", auto and e["fuse_ref_last"])
        hit("fuse_ref_last:automatic off", auto and not e["fuse_ref_last"])
        hit("fuse_ref_last:forced on at B>=2", o["fuse_ref_last"] == 1 and B >= 2)
        hit("fuse_ref_last:forced on at an odd size", o["fuse_ref_last"] == 1 and H % 2 == 1 and W % 2 == 1)
        hit("fuse_ref_last:forced off at B=1", o["fuse_ref_last"] == 0 and B == 1)
        hit("nchunks:1", e["nchunks"] == 1)
        hit("nchunks:2", e["nchunks"] == 2)
        hit("nchunks:>=4", e["nchunks"] >= 4)
        hit("nchunks:ragged last chunk", e["nchunks"] >= 2 and e["ragged"])
        hit("pipe:on by option", e["pipe"] and o["ref_pipe"] == 1 and e["nchunks"] < 4)
        hit("pipe:on automatically", e["pipe"] and o["ref_pipe"] < 0)
        hit("pipe:refused by side_streams=0", not e["pipe"] and o["ref_pipe"] == 1 and o["side_streams"] == 0
            and e["nchunks"] >= 2 and 2 * e["CH"] <= B)
        hit("pipe:refused by 2*CH>B", not e["pipe"] and o["ref_pipe"] == 1 and o["side_streams"] != 0
            and e["nchunks"] >= 2 and 2 * e["CH"] > B)
    return cov
