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
StereoPairs[i]); every batch is one lws_pool job of B pairs; the metric kernel runs behind it.  Same numbers as `--workers 0`.

`--lr_check TAU [--lr_fill]` (not in the reference; sequential mode only): the lines score LWSNet.forward_lr's checked maps, and one
more line gives the per-stage mean density of consistent pixels.
"""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

from .inference import add_lr_arguments, check_lr_arguments

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


def _sequential(model, dataset, mode, batches, maxdisp, lr=None):
    """StereoPairs[i] -> model(left, right) on the batch -> lws_stage_metrics, one batch after the other.  A generator like
    _pipelined: "start" after a warm-up forward, then (counts, abs_sum) per batch.  lr = (tau, fill): the metric scores the
    checked maps of LWSNet.forward_lr instead, and each item gains the batch's density [4,b]."""
    import torch
    from . import ops
    dev = model.device
    H, W = dataset[batches[0][0]][0].shape[1:]
    x = np.zeros((len(batches[0]), 3, H, W), np.float32)
    if lr is None:
        model(x, x)                                     # warm-up outside the clock: workspace for the largest batch
    else:
        model.forward_lr(x, x, *lr)
    torch.cuda.synchronize(dev)
    yield "start"
    for rng in batches:
        items = [dataset[i] for i in rng]
        left = np.stack([it[0] for it in items])
        right = np.stack([it[1] for it in items])
        gt = torch.from_numpy(np.ascontiguousarray(np.stack([it[2] for it in items]), dtype=np.float32)).to(dev)
        if lr is None:
            preds, density = model(left, right), None
        else:
            res = model.forward_lr(left, right, *lr)
            preds, density = res.disp, res.density
        with torch.cuda.device(dev):
            counts, sums = ops.stage_metrics(preds, gt, _row_offset(left.shape[2], gt.shape[1]), maxdisp, mode)
            if density is None:
                yield counts.cpu().numpy(), sums.cpu().numpy()
            else:
                yield counts.cpu().numpy(), sums.cpu().numpy(), density


def _gt_offset(n_img):
    return (2 * n_img + 255) // 256 * 256


def _host_worker(task_q, done_q, lists, kitti_set, slot_names, B, H, W, Hg):
    """Body of a host worker PROCESS of the pipelined mode (spawned: numpy and PIL only, never the GPU).  Task (slot, j, index):
    StereoPairs.raw(index) into position j of the slot's shared memory [left B,H,W,3 | right B,H,W,3 | gt B,Hg,W float32]
    (the ground truth at _gt_offset)."""
    from multiprocessing import shared_memory

    from lwsnet_amd.datasets import StereoPairs
    ds = StereoPairs(*lists, training=False, kitti_set=kitti_set)
    n_img = B * H * W * 3
    shms = {}

    def views(sid):
        if sid not in shms:
            shm = shared_memory.SharedMemory(name=slot_names[sid])
            img = np.ndarray((2, B, H, W, 3), np.uint8, buffer=shm.buf)
            gt = np.ndarray((B, Hg, W), np.float32, buffer=shm.buf, offset=_gt_offset(n_img))
            shms[sid] = (shm, img, gt)
        return shms[sid]

    done_q.put(("ready", -1, -1, None))
    while True:
        task = task_q.get()
        if task is None:
            break
        sid, j, index = task
        try:
            left, right, gt = ds.raw(index)
            if left.shape != (H, W, 3) or gt.shape != (Hg, W):
                raise ValueError(f"{ds.left[index]}: crop {left.shape[:2]} / ground truth {gt.shape} differ from the first pair's "
                                 f"{(H, W)} / {(Hg, W)}")
            _, img, g = views(sid)
            np.copyto(img[0, j], left)
            np.copyto(img[1, j], right)
            np.copyto(g[j], gt)
            done_q.put(("decoded", sid, j, None))
        except Exception as e:                                          # noqa: BLE001 (reported to the parent, which raises)
            done_q.put(("error", sid, j, f"pair {index}: {type(e).__name__}: {e}"))
    for shm, _, _ in shms.values():
        shm.close()


class _Slot:
    """One batch in flight: the shared-memory block the host workers fill, a pinned staging copy of it, the device copies, the
    normalised inputs [left B | right B] and the four stage maps."""

    def __init__(self, dev, B, H, W, Hg):
        from multiprocessing import shared_memory

        import torch
        self.n_img = B * H * W * 3
        self.gt_off = _gt_offset(self.n_img)
        size = self.gt_off + 4 * B * Hg * W
        self.shm = shared_memory.SharedMemory(create=True, size=size)
        self.host = torch.frombuffer(self.shm.buf, dtype=torch.uint8)
        self.pinned = torch.empty((size,), dtype=torch.uint8).pin_memory()
        self.dev_raw = torch.empty((size,), dtype=torch.uint8, device=dev)
        self.dev_lr = torch.empty((2 * B, 3, H, W), dtype=torch.float32, device=dev)
        self.outs = [torch.empty((B, 1, H, W), dtype=torch.float32, device=dev) for _ in range(STAGES)]
        self.shape = (B, H, W, Hg)
        self.batch, self.filled = -1, 0

    def upload(self, b):
        """Host -> device for the first b pairs, then lws_preprocess_rgb8, on the current stream; returns (left, right, gt)."""
        import torch
        from . import ops
        B, H, W, Hg = self.shape
        self.pinned.copy_(self.host)
        self.dev_raw.copy_(self.pinned, non_blocking=True)
        img = self.dev_raw[:2 * self.n_img].view(2, B, H, W, 3)[:, :b].reshape(2 * b, H, W, 3)
        lr = self.dev_lr[:2 * b]
        ops.preprocess_rgb8(img, out=lr)
        gt = self.dev_raw[self.gt_off:].view(torch.float32).view(B, Hg, W)[:b]
        return lr[:b], lr[b:], gt

    def close(self):
        self.host = None
        try:
            self.shm.close()
        except BufferError:                                             # a view is still alive somewhere: unlink anyway
            pass
        self.shm.unlink()


def _pipelined(model, dataset, mode, batches, maxdisp, workers, gpu_workers):
    """Host workers decode into slots; every batch is one lws_pool job; the metric kernel runs behind it (see the module
    docstring).  A generator: yields "start" once everything is up, then (counts, abs_sum) per batch in order.  submit() and
    result() of the pool are called on this thread only."""
    import collections
    import multiprocessing as mp
    import queue

    import torch
    from . import ops
    dev = model.device
    N, P = max(1, int(workers)), max(1, int(gpu_workers))
    B = max(len(r) for r in batches)
    first = dataset.raw(batches[0][0])
    H, W, Hg = first[0].shape[0], first[0].shape[1], first[2].shape[0]
    row_offset = _row_offset(H, Hg)
    torch.cuda.set_device(dev)
    slots = [_Slot(dev, B, H, W, Hg) for _ in range(min(len(batches), P + 2))]
    ctx = mp.get_context("spawn")                       # fresh interpreters: a forked child of a process that holds HIP state is not safe
    task_q, done_q = ctx.Queue(), ctx.Queue()
    lists = (dataset.left, dataset.right, dataset.disp)
    procs = [ctx.Process(target=_host_worker, args=(task_q, done_q, lists, dataset.kitti_set, [sl.shm.name for sl in slots],
                                                    B, H, W, Hg), daemon=True) for _ in range(N)]
    for pr in procs:
        pr.start()
    copy = torch.cuda.Stream(device=dev)
    try:
        with model.pool(workers=P) as gpool:
            gpool.reserve(B, H, W)
            sl = slots[0]                                   # warm-up outside the clock: library, pool workers and their workspaces
            gpool.submit(sl.dev_lr[:B].zero_(), sl.dev_lr[B:].zero_(), out=sl.outs).result()
            torch.cuda.synchronize(dev)
            ready, t_wait = 0, time.perf_counter()
            while ready < N:                                # every worker has started (spawn + imports: ~1 s, once)
                try:
                    msg = done_q.get(timeout=5.0)
                except queue.Empty:
                    if not all(pr.is_alive() for pr in procs) or time.perf_counter() - t_wait > 120.0:
                        raise RuntimeError("the host worker processes did not start")
                    continue
                if msg[0] != "ready":
                    raise RuntimeError(f"unexpected message from a host worker before its start-up: {msg}")
                ready += 1
            yield "start"
            next_batch = 0

            def assign(sid):
                nonlocal next_batch
                slots[sid].batch, slots[sid].filled = next_batch, 0
                for j, i in enumerate(batches[next_batch]):
                    task_q.put((sid, j, i))
                next_batch += 1

            for sid in range(len(slots)):
                assign(sid)
            inflight = collections.deque()                  # (batch, slot id, job, gt) in submission order
            done, emitted = {}, 0
            while emitted < len(batches):
                decoding = any(sl.batch >= 0 and sl.filled < len(batches[sl.batch]) for sl in slots)
                if inflight and (len(inflight) >= P or not decoding):
                    k, sid, job, gt = inflight.popleft()
                    preds = job.result()                    # the four stage maps are complete in device memory
                    with torch.cuda.stream(copy):
                        counts, sums = ops.stage_metrics(preds, gt, row_offset, maxdisp, mode)
                        done[k] = (counts.cpu().numpy(), sums.cpu().numpy())
                    slots[sid].batch = -1
                    if next_batch < len(batches):
                        assign(sid)
                    while emitted in done:
                        yield done.pop(emitted)
                        emitted += 1
                    continue
                try:
                    kind, sid, j, val = done_q.get(timeout=5.0)
                except queue.Empty:
                    if not all(pr.is_alive() for pr in procs):
                        raise RuntimeError("a host worker process died")
                    continue
                if kind != "decoded":
                    raise RuntimeError(val)
                sl = slots[sid]
                sl.filled += 1
                k = sl.batch
                b = len(batches[k])
                if sl.filled == b:
                    with torch.cuda.stream(copy):
                        left, right, gt = sl.upload(b)
                        job = gpool.submit(left, right, out=[o[:b] for o in sl.outs])     # starts behind the upload (after_stream = copy)
                    inflight.append((k, sid, job, gt))
    finally:
        for _ in procs:
            task_q.put(None)
        for pr in procs:
            pr.join(timeout=10.0)
            if pr.is_alive():
                pr.terminate()                              # (the exact children started above)
        torch.cuda.synchronize(dev)
        for sl in slots:
            sl.close()


def evaluate(model, dataset, metric, batch_size=8, maxdisp=KITTI_MAXDISP, workers=0, gpu_workers=2, log=None, lr_check=None,
             lr_fill=False):
    """Runs the reference's test loop for `metric` ("kitti": finetune.py's 3-pixel error, "epe": train.py's EPE) over
    `dataset` (a StereoPairs with training=False).  maxdisp is the mask bound (the KITTI loop uses 192, see KITTI_MAXDISP).
    Returns a dict: per-stage averages at full precision, per-batch values, per-image counts and sums, pairs, wall time, pairs/s.
    lr_check = TAU (sequential mode only): the metric scores the maps of LWSNet.forward_lr(tau=TAU, fill=lr_fill), and the dict
    gains lr_tau and lr_density, the per-stage mean over the pairs of the fraction of consistent pixels."""
    if metric not in ("kitti", "epe"):
        raise ValueError(f"metric must be 'kitti' or 'epe', got {metric!r}")
    if lr_check is not None and workers > 0:
        raise ValueError("the left-right check runs in the sequential mode only (workers = 0)")
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
    lr = None if lr_check is None else (float(lr_check), bool(lr_fill))
    densities = []
    if workers > 0:
        it = _pipelined(model, dataset, metric, batches, maxdisp, workers, gpu_workers)
    else:
        it = _sequential(model, dataset, metric, batches, maxdisp, lr)
    if next(it) != "start":
        raise RuntimeError("the evaluation did not start")
    t0 = time.perf_counter()
    for k, item in enumerate(it):
        counts, sums = item[0], item[1]
        if lr is not None:
            densities.append(item[2])
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
    if lr is not None:
        density = np.concatenate(densities, axis=1).mean(axis=1)           # [4]: mean over the pairs
        log.info("LR check (tau = {:g}{}): mean density ".format(lr[0], ", filled" if lr[1] else "")
                 + ", ".join("Stage {}={:.4f}".format(x, d) for x, d in enumerate(density)))
        res["lr_tau"] = lr[0]
        res["lr_density"] = [float(d) for d in density]
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
    p.add_argument("--synthetic_weights", action="store_true",
                   help="use the seeded synthetic weights instead of --model (the reference ships no checkpoint)")
    p.add_argument("--maxdisplist", type=int, nargs="+", default=[24, 5, 5])
    p.add_argument("--channels_3d", type=int, default=8)
    p.add_argument("--layers_3d", type=int, default=4)
    p.add_argument("--growth_rate", type=int, nargs="+", default=[4, 1, 1])
    p.add_argument("--gpu_id", type=int, default=0)
    p.add_argument("--workers", type=int, default=0,
                   help="host worker processes decoding into a pipelined GPU path (0 = the reference's sequential loop; not in the reference)")
    p.add_argument("--gpu_workers", type=int, default=2, help="with --workers: batches kept in flight by lws_pool")
    p.add_argument("--json", type=str, default=None, help="write the result (full-precision numbers) to this file")
    add_lr_arguments(p)
    return p


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
    check_lr_arguments(parser, args)
    logging.basicConfig(stream=sys.stderr, level=logging.INFO,
                        format="[%(asctime)s %(filename)s:%(lineno)s] %(levelname)s: %(message)s")
    log = logging.getLogger("lwsnet_amd.evaluate")
    for k, v in vars(args).items():
        log.info("%s: %s", k, v)
    dataset, metric, maxdisp = load_dataset(args)
    import torch
    from .checkpoint import load_state_dict
    from .models import LWSNet
    from .weights import make_state_dict
    torch.cuda.set_device(args.gpu_id)
    model = LWSNet(args, device=torch.device("cuda", args.gpu_id))
    if args.synthetic_weights:
        model.set_state_dict(make_state_dict(7, args))
        log.info("Using seeded synthetic weights")
    elif not os.path.isfile(args.model):
        log.info("No model load")
        raise SystemExit(1)
    else:
        model.set_state_dict(load_state_dict(args.model))
        log.info("Successful load model")
    model.eval()
    res = evaluate(model, dataset, metric, batch_size=args.test_batch_size, maxdisp=maxdisp, workers=args.workers,
                   gpu_workers=args.gpu_workers, log=log, lr_check=args.lr_check, lr_fill=args.lr_fill)
    res["dataset"] = args.dataset
    log.info("%d pairs in %.3f s: %.2f pairs/s", res["pairs"], res["wall_s"], res["pairs_per_s"])
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return res


if __name__ == "__main__":
    main()
