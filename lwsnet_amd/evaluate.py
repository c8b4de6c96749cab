#!/usr/bin/env python3
"""Dataset evaluation with the loops of the reference's `finetune.py --evaluate` (test + error_estimating, finetune.py:115-117,
184-219: KITTI 2015, 3-pixel error) and `train.py`'s test() (train.py:169-199: SceneFlow, end-point error), running the MI355X-native
model and reducing the metric on the device.

    python -m lwsnet_amd.evaluate --dataset kitti2015 --datapath dataset/kitti2015/training/ --model checkpoint.pdparams
    python -m lwsnet_amd.evaluate --dataset sceneflow --datapath dataset/sceneflow/ --synthetic_weights --workers 8

What is reproduced exactly: the batches (`--test_batch_size` pairs in list order, the last one partial), one AverageMeter update
per batch and stage (the average is over BATCHES, not pixels), the per-batch value (KITTI: sum(bad) / sum(valid) over the batch's
images, i.e. error_estimating on the stacked batch; SceneFlow: the mean |d - gt| over the batch's mask, with the 4 padded rows of
the 544-row crop dropped, train.py:189) and the log lines.  Two reference quirks are kept: error_estimating is called with its
default maxdisp=192 whatever --maxdisp says, and SceneFlow's mask `gt < maxdisp` admits gt <= 0.  A KITTI batch without a valid
pixel raises ValueError naming its files (the reference divides by zero there).

The per-pixel work -- |d - gt|, the masks, the counts and the sums -- is lws_stage_metrics (lwsnet_amd/csrc/lws_metrics.hip):
float32 as numpy computes it, counts exact, sums in fp64, deterministic; only 4 x B x 3 numbers come back per batch.

`--workers N` (not in the reference): N spawned host processes (numpy + PIL, never the GPU) decode and crop `StereoPairs.raw(i)`
into shared-memory slots; a copy stream uploads the bytes and normalises them on the device (lws_preprocess_rgb8, bit for bit
StereoPairs[i]); every batch is one lws_pool job of B pairs; the metric kernel runs behind it (lwsnet_amd/pipeline.py, as for
`lwsnet_amd.inference --workers N`).  Same numbers as `--workers 0`.

`--lr_check` (or `--occ_check`), `--speckle` and `--wmedian` (not in the reference; sequential mode only) put the post-processing chain in front of
the metric; how its steps combine is stated once, in the docstring of lwsnet_amd/postprocess.py.

`--lr_check TAU [--lr_fill]`: the lines score LWSNet.forward_lr's checked maps, and one more line gives the per-stage mean density
of consistent pixels.

`--occ_check TAU [--occ_fill]`: the one-forward alternative -- the lines score LWSNet.forward_occ's checked maps, and one more line
gives the per-stage mean density of visible pixels.

`--speckle SIZE [--speckle_diff D] [--speckle_fill]`: the lines score the maps after lws_speckle_filter, and one more line gives the
per-stage mean density of kept pixels.

`--wmedian R [--wmedian_sigma S] [--wmedian_fill N]`: the lines score the maps after lws_wmedian_filter, the last step in front of
the metric; the guide is the batch's uint8 left images, uploaded once and normalised on the device (lws_preprocess_rgb8), and one
more line gives the per-stage mean fraction of pixels the filter changed or filled.

`--sparsification` (not in the reference; sequential mode only, without the post-processing chain) scores the confidence maps: the
batch runs LWSNet.forward_conf, whose stage maps are the forward's bits, so every line above and every other field of the result
is what it is without the flag.  Behind the metric, lws_sparsification (lwsnet_amd/csrc/lws_sparsification.hip) bins every valid
pixel of every stage map twice, by its uncertainty and by its error, once with sigma and once with 1 - conf as the uncertainty
(the refined map goes by stage 3's maps, the rule of `--conf_min`); the integer histograms are summed on the host over the
dataset, and lwsnet_amd.metrics.sparsification_curves turns them into the sparsification curve (the error of the pixels left
after the least trusted fraction is removed), the oracle curve (removal by the true error) and the area between the two (AUSE,
Ilg et al. 2018), for the run's metric.  Two more log lines give the per-stage AUSE of either ranking, and the result gains the key
"sparsification".  Its curves, and "all", their value at fraction 0, are pooled over the PIXELS of the dataset: "all" is therefore
not the reference's average over batches that the lines above print.

`--photometric [--photo_alpha A]` (not in the reference; sequential mode only) scores the maps WITHOUT the ground truth, by the
photometric reprojection error (lws_photometric, lwsnet_amd/csrc/lws_photometric.hip: the right image warped into the left view
with the map against the left image, A * DSSIM + (1 - A) * L1, A = 0.85 by default).  The batch is read as bytes
(StereoPairs.raw), as for the guided median; the maps scored are the ones the metric scores, the chain's final maps when the chain
is on, and only the pixels the chain's codes keep are scored, under the rule of the geometry outputs (lwsnet_amd/postprocess.py: the
codes count while nothing has been filled).  One more log line gives the per-stage mean error and density, pooled over the pixels
of the dataset, and the result gains the key "photometric"; nothing else in it changes.
"""
import argparse
import contextlib
import functools
import json
import logging
import os
import time

import numpy as np

from . import pipeline
from . import postprocess as post
from .inference import add_model_arguments, load_model, start_logging

STAGES = 4
KITTI_MAXDISP = 192                     # error_estimating's default (finetune.py:212), which test() never overrides


class AverageMeter:
    """Running value / average with the update rule of the reference's utils/utils.py: sum += val * n, avg = sum / count."""

    def __init__(self):
        self.val, self.avg, self.sum, self.count = 0, 0, 0, 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class Meters:
    """The bookkeeping of the reference's two test loops, fed one batch at a time IN ORDER: `update` turns the batch's per-image
    device sums into the per-stage values, updates the meters and returns the log line the reference prints (or None)."""

    def __init__(self, metric, n_batches):
        if metric not in ("kitti", "epe"):
            raise ValueError(f"metric must be 'kitti' or 'epe', got {metric!r}")
        self.metric, self.n_batches = metric, n_batches
        self.meters = [AverageMeter() for _ in range(STAGES)]
        self.values = []                                    # per batch: 4 values (None = stage skipped, SceneFlow only)

    def update(self, batch_id, counts, abs_sum, files=()):
        """counts [4,b,2] = {valid, bad}, abs_sum [4,b] of one batch (host arrays)."""
        counts = np.asarray(counts, dtype=np.int64)
        abs_sum = np.asarray(abs_sum, dtype=np.float64)
        vals = []
        for s in range(STAGES):
            valid = int(counts[s, :, 0].sum())
            if self.metric == "kitti":                          # float(err3) / float(mask.sum()), finetune.py:219
                if valid == 0:
                    raise ValueError(f"KITTI batch {batch_id} has no ground-truth pixel with 0 < gt < {KITTI_MAXDISP} "
                                     f"(the reference divides by zero here): {', '.join(map(str, files))}")
                v = float(int(counts[s, :, 1].sum())) / float(valid)
            else:                                               # float(np.mean(|d - gt|[mask])), train.py:186-190
                if valid == 0:
                    vals.append(None)
                    continue
                v = float(abs_sum[s].sum()) / valid
            self.meters[s].update(v)
            vals.append(v)
        self.values.append(vals)
        return self.line(batch_id)

    def line(self, batch_id):
        m = self.meters
        if self.metric == "kitti":                              # finetune.py:206-208, every batch
            info = "\t".join("Stage {} = {:.4f}({:.4f})".format(x, m[x].val, m[x].avg) for x in range(STAGES))
            return "Test [{}/{}] {}".format(batch_id, self.n_batches, info)
        if batch_id % 5 == 0:                                   # train.py:192-194
            info = "\t".join("Stage {} = {:.2f}({:.2f})".format(x, m[x].val, m[x].avg) for x in range(STAGES))
            return "Test: [{}/{}] {}".format(batch_id, self.n_batches, info)
        return None

    def averages(self):
        return [float(m.avg) for m in self.meters]

    def final_line(self):
        if self.metric == "kitti":                              # finetune.py:210-211
            return "Average test 3-Pixel Error: " + ", ".join("Stage {}={:.4f}".format(x, m.avg) for x, m in enumerate(self.meters))
        return "Average test EPE = " + ", ".join("Stage {}={:.2f}".format(x, m.avg) for x, m in enumerate(self.meters))   # train.py:196-197


def aggregate(batches, metric, batch_files=None):
    """Pure host form of the reference loops: batches = [(counts [4,b,2], abs_sum [4,b]), ...] in order.  Returns
    (averages [4], per-batch values [[4], ...], log lines)."""
    meters = Meters(metric, len(batches))
    lines = []
    for i, (counts, abs_sum) in enumerate(batches):
        ln = meters.update(i, counts, abs_sum, batch_files[i] if batch_files else ())
        if ln is not None:
            lines.append(ln)
    lines.append(meters.final_line())
    return meters.averages(), meters.values, lines


def batch_ranges(n, batch_size):
    """The reference's DataLoader(shuffle=False, drop_last=False): consecutive index ranges, the last one partial."""
    return [range(i, min(i + batch_size, n)) for i in range(0, n, batch_size)]


def _row_offset(H, Hg):
    if Hg > H:
        raise ValueError(f"the ground truth has {Hg} rows, more than the {H}-row crop")
    return H - Hg


def _sequential(model, dataset, mode, batches, maxdisp, options, sparsification=False, photo_alpha=None):
    """StereoPairs[i] -> postprocess.run_chain on the batch -> lws_stage_metrics, one batch after the other.  A generator: "start"
    after a warm-up forward, then (counts, abs_sum, stats) per batch.  stats has a [4,b] array per stage of `options` that is on:
    lr_density (the check's consistent pixels / (H*W)), occ_density (the occlusion check's visible pixels / (H*W)), speckle_density (the speckle filter's kept pixels / (H*W)) and
    wmedian_changed (the median's changed + filled pixels / (H*W)).  When the median needs a guide the batch is read as bytes
    (StereoPairs.raw), uploaded once and normalised on the device, and its left images are the guide.  With `sparsification` (no
    stage of the chain is on then) the batch runs LWSNet.forward_conf instead and stats has "sparsification": per kind ("conf",
    "sigma") the host copy of ops.sparsification's histogram [4,b,2,1026,3].  With photo_alpha = A the batch is read as bytes too
    and stats has "photometric": the host copy of ops.photometric's sums [4,b,4] for the maps the metric scores, masked by the
    chain's `keep` codes (None: every pixel), and H * W."""
    import torch
    from . import ops
    dev = model.device
    H, W = dataset[batches[0][0]][0].shape[1:]
    x = np.zeros((len(batches[0]), 3, H, W), np.float32)
    if options.lr_check is not None:                    # warm-up outside the clock: workspace for the largest batch
        model.forward_lr(x, x, options.lr_check, options.forward_fills)
    elif options.occ_check is not None:
        model.forward_occ(x, x, options.occ_check, options.forward_fills)
    elif sparsification:
        model.forward_conf(x, x)
    else:
        model(x, x)
    torch.cuda.synchronize(dev)
    yield "start"
    for rng in batches:
        guide = keep = None
        if options.needs_guide or photo_alpha is not None:
            items = [dataset.raw(i) for i in rng]
            with torch.cuda.device(dev):
                u8 = torch.from_numpy(np.stack([it[0] for it in items] + [it[1] for it in items])).to(dev)
                both = ops.preprocess_rgb8(u8)                  # bit for bit StereoPairs[i]
            left, right, guide = both[:len(items)], both[len(items):], u8[:len(items)] if options.needs_guide else None
        else:
            items = [dataset[i] for i in rng]
            left = np.stack([it[0] for it in items])
            right = np.stack([it[1] for it in items])
        gt = torch.from_numpy(np.ascontiguousarray(np.stack([it[2] for it in items]), dtype=np.float32)).to(dev)
        stats = {}
        if sparsification:
            conf_res = model.forward_conf(left, right)
            disp = conf_res.preds
        else:
            res = post.run_chain(model, left, right, options, guide)
            disp, keep = res.disp, res.keep
            if res.lr_density is not None:
                stats["lr_density"] = res.lr_density
            if res.occ_density is not None:
                stats["occ_density"] = res.occ_density
            if res.speckle_counts is not None:
                stats["speckle_density"] = res.speckle_counts[:, :, 1].cpu().numpy() / float(H * W)
            if res.wmedian_counts is not None:
                stats["wmedian_changed"] = res.wmedian_counts.sum(dim=2).cpu().numpy() / float(H * W)
        with torch.cuda.device(dev):
            row_offset = _row_offset(left.shape[2], gt.shape[1])
            counts, sums = ops.stage_metrics(disp, gt, row_offset, maxdisp, mode)
            if sparsification:                              # the refined map goes by stage 3's uncertainty
                unc = {"conf": conf_res.conf, "sigma": conf_res.sigma}
                hists = {kind: ops.sparsification(disp, [*u, u[2]], gt, row_offset, maxdisp, mode, kind) for kind, u in unc.items()}
                stats["sparsification"] = {kind: h.cpu().numpy() for kind, h in hists.items()}
            if photo_alpha is not None:
                photo = ops.photometric(list(disp), u8[:len(items)], u8[len(items):], mask=keep, alpha=photo_alpha, want_err=False)
                stats["photometric"] = photo.sums.cpu().numpy(), H * W
            yield counts.cpu().numpy(), sums.cpu().numpy(), stats


def _decode_pair(dataset, shape, views, j, index):
    """Host worker handler of the pipelined mode (lwsnet_amd/pipeline.py: a spawned process, numpy and PIL only):
    StereoPairs.raw(index) into position j of the slot, views = [left, right (2,B,H,W,3) uint8 | ground truth (B,Hg,W) float32]."""
    left, right, gt = dataset.raw(index)
    H, W, Hg = shape
    if left.shape != (H, W, 3) or gt.shape != (Hg, W):
        raise ValueError(f"{dataset.left[index]}: crop {left.shape[:2]} / ground truth {gt.shape} differ from the first pair's "
                         f"{(H, W)} / {(Hg, W)}")
    img, g = views
    np.copyto(img[0, j], left)
    np.copyto(img[1, j], right)
    np.copyto(g[j], gt)
    return "decoded", None


class _Slot(pipeline.Slot):
    """One batch in flight: the shared block of _decode_pair, its device copies, the normalised inputs [left B | right B] and
    the four stage maps."""

    def __init__(self, dev, B, H, W, Hg):
        import torch
        super().__init__([((2, B, H, W, 3), np.uint8), ((B, Hg, W), np.float32)], dev)
        self.dev_img = torch.empty((2, B, H, W, 3), dtype=torch.uint8, device=dev)
        self.dev_gt = torch.empty((B, Hg, W), dtype=torch.float32, device=dev)
        self.dev_lr = torch.empty((2 * B, 3, H, W), dtype=torch.float32, device=dev)
        self.outs = [torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) for _ in range(STAGES)]
        self.batch, self.filled = -1, 0

    def upload(self, b):
        """Host -> device, then lws_preprocess_rgb8 for the first b pairs, on the current stream; returns (left, right, gt)."""
        from . import ops
        for i, dst in enumerate((self.dev_img, self.dev_gt)):
            self.stage(i)
            dst.copy_(self.pinned(i), non_blocking=True)
        H, W = self.dev_img.shape[2:4]
        lr = self.dev_lr[:2 * b]
        ops.preprocess_rgb8(self.dev_img[:, :b].reshape(2 * b, H, W, 3), out=lr)
        return lr[:b], lr[b:], self.dev_gt[:b]


def _pipelined(model, dataset, mode, batches, maxdisp, workers, gpu_workers):
    """Host workers decode into slots; every batch is one lws_pool job; the metric kernel runs behind it (see the module
    docstring).  A generator: yields "start" once everything is up, then (counts, abs_sum) per batch in order."""
    import torch
    from . import ops
    from .datasets import StereoPairs
    dev = model.device
    N, P = max(1, int(workers)), max(1, int(gpu_workers))
    B = max(len(r) for r in batches)
    first = dataset.raw(batches[0][0])
    H, W, Hg = first[0].shape[0], first[0].shape[1], first[2].shape[0]
    row_offset = _row_offset(H, Hg)
    torch.cuda.set_device(dev)
    pairs = StereoPairs(dataset.left, dataset.right, dataset.disp, training=False, kitti_set=dataset.kitti_set, rng=None)  # picklable
    copy = torch.cuda.Stream(device=dev)
    next_batch = 0

    def assign(sid):                                    # a free slot takes the next batch
        nonlocal next_batch
        if next_batch < len(batches):
            slots[sid].batch, slots[sid].filled = next_batch, 0
            for j, i in enumerate(batches[next_batch]):
                host.put(sid, f"pair {i}", j, i)
            next_batch += 1

    def handle(kind, sid, _):
        sl = slots[sid]
        sl.filled += 1
        b = len(batches[sl.batch])
        if sl.filled < b:
            return None
        with torch.cuda.stream(copy):
            left, right, gt = sl.upload(b)
            return sl.batch, sid, gpool.submit(left, right, out=[o[:b] for o in sl.outs]), gt     # starts behind the upload

    def retire(item):
        k, sid, job, gt = item
        preds = job.result()                            # the four stage maps are complete in device memory
        with torch.cuda.stream(copy):
            counts, sums = ops.stage_metrics(preds, gt, row_offset, maxdisp, mode)
            res = counts.cpu().numpy(), sums.cpu().numpy()
        assign(sid)
        return k, res

    with contextlib.ExitStack() as stack:
        slots = [stack.enter_context(_Slot(dev, B, H, W, Hg)) for _ in range(min(len(batches), P + 2))]
        host = stack.enter_context(pipeline.HostWorkers(N, functools.partial(_decode_pair, pairs, (H, W, Hg)), slots))
        gpool = stack.enter_context(model.pool(workers=P))
        sl = slots[0]                                   # warm-up outside the clock: library, pool workers and their workspaces
        gpool.submit(sl.dev_lr[:B].zero_(), sl.dev_lr[B:].zero_(), out=sl.outs).result()
        torch.cuda.synchronize(dev)
        host.wait_ready()
        yield "start"
        for sid in range(len(slots)):
            assign(sid)
        done, emitted = {}, 0
        for k, res in pipeline.schedule(host, P, handle, retire, lambda: host.pending > 0):
            done[k] = res
            while emitted in done:                      # in batch order
                yield done.pop(emitted)
                emitted += 1


def _stage_reports(o):
    """Per stage of the options `o` that is on: (its key in _sequential's stats and in the result, the prefix of its log line, the
    settings the result records in front of it)."""
    reports = []
    if o.lr_check is not None:
        reports.append(("lr_density", "LR check (tau = {:g}{}): mean density ".format(o.lr_check, ", filled" if o.lr_fill else ""),
                        {"lr_tau": o.lr_check}))
    if o.occ_check is not None:
        reports.append(("occ_density", "Occlusion check (tau = {:g}{}): mean density ".format(o.occ_check, ", filled" if o.occ_fill else ""),
                        {"occ_tau": o.occ_check}))
    if o.speckle is not None:
        reports.append(("speckle_density", "Speckle filter (size <= {}, diff <= {:g}{}): mean kept density ".format(
            o.speckle, o.speckle_diff, ", filled" if o.speckle_fills else ""), {"speckle_size": o.speckle, "speckle_diff": o.speckle_diff}))
    if o.wmedian is not None:
        reports.append(("wmedian_changed", "Weighted median (radius {}, sigma {:g}, fill {}): mean changed fraction ".format(
            o.wmedian, o.wmedian_sigma, o.wmedian_fill),
            {"wmedian_radius": o.wmedian, "wmedian_sigma": o.wmedian_sigma, "wmedian_fill": o.wmedian_fill}))
    return reports


class Sparsification:
    """The host side of `--sparsification`, fed one batch at a time in order: per kind ("conf", "sigma") the per-image AUSE of the
    four stage maps and the histograms' sum over the dataset (integers: pooling is exact)."""
    KINDS = ("conf", "sigma")

    def __init__(self, metric):
        self.metric = metric
        self.pooled = {}
        self.per_image = {kind: [] for kind in self.KINDS}

    def update(self, hists):
        """hists: per kind, the int64 [4,b,2,1026,3] histograms of one batch."""
        from .metrics import sparsification_curves
        for kind in self.KINDS:
            h = np.asarray(hists[kind], dtype=np.int64)
            self.pooled[kind] = self.pooled.get(kind, 0) + h.sum(axis=1)
            for b in range(h.shape[1]):
                if h[0, b, 0, :, 0].sum() == 0:             # no valid pixel: the same for every stage, it depends on gt alone
                    self.per_image[kind].append([None] * STAGES)
                else:
                    self.per_image[kind].append([sparsification_curves(h[s, b], self.metric)["ause"] for s in range(STAGES)])

    def result(self):
        """The "sparsification" entry of evaluate()'s result (ValueError when the dataset has no valid pixel at all)."""
        from .metrics import sparsification_curves
        curves = {kind: [sparsification_curves(self.pooled[kind][s], self.metric) for s in range(STAGES)] for kind in self.KINDS}
        first = curves[self.KINDS[0]]                       # fractions, the oracle curve and `all` do not depend on the kind
        res = {"fractions": first[0]["fractions"].tolist()}
        for kind in self.KINDS:
            res[kind] = {"ause": [c["ause"] for c in curves[kind]], "ause_rel": [c["ause_rel"] for c in curves[kind]],
                         "curve": [c["unc"].tolist() for c in curves[kind]]}
        res["oracle"] = {"curve": [c["oracle"].tolist() for c in first]}
        res["all"] = [c["all"] for c in first]
        res["per_image_ause"] = self.per_image
        return res

    def lines(self, res):
        return ["Sparsification ({}): AUSE ".format(kind) + ", ".join("Stage {}={:.4f}".format(x, a) for x, a in enumerate(res[kind]["ause"]))
                for kind in self.KINDS]


class Photometric:
    """The host side of `--photometric`, fed one batch at a time in order: ops.photometric's integer sums of every image."""

    def __init__(self, alpha):
        self.alpha, self.pixels, self.sums = float(alpha), None, []

    def update(self, sums, pixels):
        """sums: the int64 [4,b,4] of one batch; pixels: H * W of its images."""
        self.sums.append(np.asarray(sums, dtype=np.int64))
        self.pixels = int(pixels)

    def result(self):
        """The "photometric" entry of evaluate()'s result: alpha, the per-stage means pooled over the pixels of the dataset
        (metrics.photometric_means: pe, l1, dssim, scored, density; None for a stage without a scored pixel) and per_image, the same
        four means per image."""
        from .metrics import photometric_means
        sums = np.concatenate(self.sums, axis=1)
        res = {"alpha": self.alpha, **photometric_means(sums, self.pixels)}
        each = [photometric_means(sums[:, i:i + 1], self.pixels) for i in range(sums.shape[1])]
        res["per_image"] = {key: [m[key] for m in each] for key in ("pe", "l1", "dssim", "density")}
        return res

    def line(self, res):
        fmt = lambda v: "none" if v is None else "{:.4f}".format(v)     # noqa: E731
        return "Photometric (alpha = {:g}): mean error ".format(self.alpha) + ", ".join(
            "Stage {}={} (density {:.4f})".format(x, fmt(e), d) for x, (e, d) in enumerate(zip(res["pe"], res["density"])))


def evaluate(model, dataset, metric, batch_size=8, maxdisp=KITTI_MAXDISP, workers=0, gpu_workers=2, log=None, lr_check=None,
             lr_fill=False, speckle=None, speckle_diff=1.0, speckle_fill=False, wmedian=None, wmedian_sigma=10.0, wmedian_fill=0,
             occ_check=None, occ_fill=False, sparsification=False, photometric=False, photo_alpha=0.85):
    """Runs the reference's test loop for `metric` ("kitti": finetune.py's 3-pixel error, "epe": train.py's EPE) over
    `dataset` (a StereoPairs with training=False).  maxdisp is the mask bound (the KITTI loop uses 192, see KITTI_MAXDISP).
    Returns a dict: per-stage averages at full precision, per-batch values, per-image counts and sums, pairs, wall time, pairs/s.
    lr_check = TAU (or occ_check = TAU, the one-forward alternative), speckle = SIZE and wmedian = R (sequential mode only) switch on the stages of postprocess.run_chain in front of
    the metric, with the flags named after them (postprocess.Options; the module docstring there says how they combine); a value
    a stage does not support is a ValueError.  Per stage the dict gains its settings and a per-stage mean over the pairs: lr_tau
    and lr_density (consistent pixels / (H*W)); occ_tau and occ_density (visible pixels / (H*W)); speckle_size, speckle_diff and speckle_density (kept pixels / (H*W));
    wmedian_radius, wmedian_sigma, wmedian_fill and wmedian_changed ((changed + filled pixels) / (H*W)).
    sparsification = True (sequential mode only, with no stage of the chain: a ValueError otherwise) adds the key "sparsification",
    the curves and AUSE of the confidence and sigma maps (the module docstring; Sparsification.result).
    photometric = True (sequential mode only; photo_alpha in [0, 1]: a ValueError otherwise) adds the key "photometric", the
    photometric reprojection error of the maps the metric scores (the module docstring; Photometric.result)."""
    if metric not in ("kitti", "epe"):
        raise ValueError(f"metric must be 'kitti' or 'epe', got {metric!r}")
    options = post.Options.make(lr_check=lr_check, lr_fill=lr_fill, speckle=speckle, speckle_diff=speckle_diff, speckle_fill=speckle_fill,
                                wmedian=wmedian, wmedian_sigma=wmedian_sigma, wmedian_fill=wmedian_fill, occ_check=occ_check,
                                occ_fill=occ_fill)
    if options.stages_on and workers > 0:
        raise ValueError(f"the {options.stages_on[0]} runs in the sequential mode only (workers = 0)")
    options.check()
    if sparsification and workers > 0:
        raise ValueError("the sparsification curves run in the sequential mode only (workers = 0)")
    if sparsification and options.stages_on:
        raise ValueError(f"the sparsification curves score the forward's own maps: they do not combine with the {options.stages_on[0]}")
    if photometric and workers > 0:
        raise ValueError("the photometric error runs in the sequential mode only (workers = 0)")
    if photometric and not (isinstance(photo_alpha, (int, float)) and 0.0 <= photo_alpha <= 1.0):
        raise ValueError(f"photo_alpha must be in [0, 1], got {photo_alpha!r}")
    if batch_size < 1:
        raise ValueError("batch_size must be >= 1")
    n = len(dataset)
    if n == 0:
        raise ValueError("the dataset is empty")
    log = log or logging.getLogger("lwsnet_amd.evaluate")
    batches = batch_ranges(n, batch_size)
    files = [[os.path.basename(dataset.left[i]) for i in r] for r in batches]
    meters = Meters(metric, len(batches))
    per_image = {"valid": [], "bad": [], "abs_sum": []}
    stats = {}
    if workers > 0:
        it = _pipelined(model, dataset, metric, batches, maxdisp, workers, gpu_workers)
    else:
        it = _sequential(model, dataset, metric, batches, maxdisp, options, sparsification, float(photo_alpha) if photometric else None)
    spars = Sparsification(metric) if sparsification else None
    photo = Photometric(photo_alpha) if photometric else None
    if next(it) != "start":
        raise RuntimeError("the evaluation did not start")
    t0 = time.perf_counter()
    for k, (counts, sums, *batch_stats) in enumerate(it):               # _pipelined runs no stage and yields no stats
        for key, value in (batch_stats[0].items() if batch_stats else ()):
            if key == "sparsification":
                spars.update(value)
            elif key == "photometric":
                photo.update(*value)
            else:
                stats.setdefault(key, []).append(value)
        line = meters.update(k, counts, sums, files[k])
        if line is not None:
            log.info(line)
        per_image["valid"] += counts[:, :, 0].T.tolist()
        per_image["bad"] += counts[:, :, 1].T.tolist()
        per_image["abs_sum"] += sums.T.tolist()
    wall = time.perf_counter() - t0
    log.info(meters.final_line())
    res = {"metric": metric, "maxdisp": maxdisp, "batch_size": batch_size, "pairs": n, "batches": len(batches),
           "average": meters.averages(), "per_batch": meters.values,
           "per_image": dict(files=[os.path.basename(p) for p in dataset.left], **per_image),
           "wall_s": wall, "pairs_per_s": n / wall if wall > 0 else float("inf"),
           "workers": int(workers), "gpu_workers": int(gpu_workers) if workers > 0 else 0}
    for key, prefix, settings in _stage_reports(options):
        mean = np.concatenate(stats[key], axis=1).mean(axis=1)             # [4]: mean over the pairs
        log.info(prefix + ", ".join("Stage {}={:.4f}".format(x, d) for x, d in enumerate(mean)))
        res.update(settings)
        res[key] = [float(d) for d in mean]
    if spars is not None:
        res["sparsification"] = spars.result()
        for line in spars.lines(res["sparsification"]):
            log.info(line)
    if photo is not None:
        res["photometric"] = photo.result()
        log.info(photo.line(res["photometric"]))
    return res


DEFAULT_DATAPATH = {"kitti2015": "dataset/kitti2015/training/", "sceneflow": "dataset/sceneflow/"}   # finetune.py:22, train.py:23


def build_parser():
    p = argparse.ArgumentParser(description="Evaluation of LWSNet on KITTI 2015 (3-pixel error) or SceneFlow (EPE)")
    p.add_argument("--dataset", choices=["kitti2015", "sceneflow"], default="kitti2015")
    p.add_argument("--datapath", type=str, default=None, help="default: dataset/kitti2015/training/ or dataset/sceneflow/")
    p.add_argument("--val_set", type=str, default="val_set.txt", help="KITTI: the split file of the validation frames")
    p.add_argument("--test_batch_size", type=int, default=8)
    p.add_argument("--maxdisp", type=int, default=192, help="SceneFlow: the mask bound gt < maxdisp (the KITTI loop always uses 192)")
    p.add_argument("--model", type=str, default="checkpoint")
    add_model_arguments(p)
    p.add_argument("--workers", type=int, default=0,
                   help="host worker processes decoding into a pipelined GPU path (0 = the reference's sequential loop; not in the reference)")
    p.add_argument("--gpu_workers", type=int, default=2, help="with --workers: batches kept in flight by lws_pool")
    p.add_argument("--json", type=str, default=None, help="write the result (full-precision numbers) to this file")
    post.add_lr_arguments(p)
    post.add_occ_arguments(p)
    post.add_speckle_arguments(p)
    post.add_wmedian_arguments(p)
    add_sparsification_argument(p)
    post.add_photometric_arguments(p)
    return p


def add_sparsification_argument(p):
    """--sparsification (not in the reference).  A command line without it parses to the namespace it parsed to before the flag
    existed (argparse.SUPPRESS); check_sparsification_argument writes its default, False."""
    p.add_argument("--sparsification", action="store_true", default=argparse.SUPPRESS,
                   help="score the confidence and sigma maps: sparsification curves and AUSE per stage (sequential mode only, without "
                        "the post-processing flags; not in the reference)")


def check_sparsification_argument(p, args):
    """Rejects what --sparsification does not combine with, before any model or GPU work; sets the flag's default."""
    args.sparsification = getattr(args, "sparsification", False)
    if not args.sparsification:
        return
    post.sequential_only(p, args, "--sparsification")
    for flag in ("lr_check", "occ_check", "speckle", "wmedian"):
        if getattr(args, flag, None) is not None:
            p.error(f"--sparsification scores the forward's own maps: it does not combine with --{flag}")


def load_dataset(args):
    """The evaluation lists and crops of finetune.py (KITTI: validation frames of the split file) or train.py (SceneFlow TEST)."""
    from .datasets import StereoPairs, kitti2015_lists, sceneflow_lists
    datapath = args.datapath or DEFAULT_DATAPATH[args.dataset]
    if args.dataset == "kitti2015":
        if not os.path.isfile(args.val_set):                    # evaluation never falls back to a shuffled split
            raise FileNotFoundError(f"--val_set {args.val_set} does not exist")
        _, _, _, left, right, disp = kitti2015_lists(datapath, args.val_set)
        return StereoPairs(left, right, disp, training=False, kitti_set=True), "kitti", KITTI_MAXDISP
    _, _, _, left, right, disp = sceneflow_lists(datapath)
    return StereoPairs(left, right, disp, training=False, kitti_set=False), "epe", args.maxdisp


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    post.check_lr_arguments(parser, args)
    post.check_occ_arguments(parser, args)
    post.check_speckle_arguments(parser, args)
    post.check_wmedian_arguments(parser, args)
    check_sparsification_argument(parser, args)
    post.check_photometric_arguments(parser, args)
    log = start_logging("lwsnet_amd.evaluate", args)
    dataset, metric, maxdisp = load_dataset(args)
    model = load_model(args, log, missing_status=1)
    res = evaluate(model, dataset, metric, batch_size=args.test_batch_size, maxdisp=maxdisp, workers=args.workers,
                   gpu_workers=args.gpu_workers, log=log, lr_check=args.lr_check, lr_fill=args.lr_fill, speckle=args.speckle,
                   speckle_diff=args.speckle_diff, speckle_fill=args.speckle_fill, wmedian=args.wmedian,
                   wmedian_sigma=args.wmedian_sigma, wmedian_fill=args.wmedian_fill, occ_check=args.occ_check, occ_fill=args.occ_fill,
                   sparsification=args.sparsification, photometric=args.photometric, photo_alpha=args.photo_alpha)
    res["dataset"] = args.dataset
    log.info("%d pairs in %.3f s: %.2f pairs/s", res["pairs"], res["wall_s"], res["pairs_per_s"])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
