"""The host worker pipeline of the CLIs' `--workers N` modes (lwsnet_amd/pipeline.py) without a GPU: spawned workers running
the real inference and evaluation handlers on plain shared-memory slots, errors and a dead worker reported to the parent, and
a teardown that leaves no process and no shared memory behind (checked after every pool here)."""
import contextlib
import functools
import os
import signal
from multiprocessing import shared_memory

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT
from lwsnet_amd import imageio as io
from lwsnet_amd import pipeline
from lwsnet_amd.evaluate import _decode_pair
from lwsnet_amd.inference import _pair_task

KITTI_PAIR = [os.path.join(ROOT, "tests", "golden", "kitti_pair", f) for f in ("left_test.png", "right_test.png")]
PAIR_LAYOUT = [((2, io.CROP_H, io.CROP_W, 3), np.uint8), ((io.CROP_H, io.CROP_W, 3), np.uint8)]    # inference's _Slot


@contextlib.contextmanager
def _workers(handler, layouts, n=2):
    with contextlib.ExitStack() as stack:
        slots = [stack.enter_context(pipeline.Slot(layout)) for layout in layouts]
        host = stack.enter_context(pipeline.HostWorkers(n, handler, slots))
        host.wait_ready()
        yield host, slots
    assert len(host.procs) == n and not any(pr.is_alive() for pr in host.procs)
    for sl in slots:
        with pytest.raises(FileNotFoundError):
            shared_memory.SharedMemory(name=sl.name)


def test_inference_handler_decodes_and_encodes(tmp_path):
    small = str(tmp_path / "small.png")
    Image.fromarray(np.zeros((300, 1300, 3), np.uint8)).save(small)              # 300 rows < 368: skipped
    with _workers(_pair_task, [PAIR_LAYOUT] * 2) as (host, slots):
        host.put(0, "decode of pair 0", "decode", *KITTI_PAIR)
        host.put(1, "decode of pair 1", "decode", small, KITTI_PAIR[1])
        assert host.pending == 2
        assert sorted(host.get()[:2] for _ in range(2)) == [("decoded", 0), ("skipped", 1)]
        pair = slots[0].views[0]
        for k in range(2):
            assert np.array_equal(pair[k], io.crop_bottom_right(io.load_rgb(KITTI_PAIR[k])))
        rgb = io.disparity_to_color(pair[0, :, :, 0].astype(np.float32) / 4)
        np.copyto(slots[0].views[1], rgb)
        host.put(0, "encode of pair 0", "encode", str(tmp_path / "got.png"))
        kind, sid, seconds = host.get()
        assert (kind, sid) == ("encoded", 0) and seconds > 0 and host.pending == 0
        io.save_png(str(tmp_path / "want.png"), rgb)
        assert (tmp_path / "got.png").read_bytes() == (tmp_path / "want.png").read_bytes()


def _kitti_pairs(tmp_path, n):
    from lwsnet_amd import datasets as D
    from lwsnet_amd import synth
    root = str(tmp_path / "kitti") + "/"
    split = synth.write_kitti_tree(root, n)
    ds = D.StereoPairs(*D.kitti2015_lists(root, split)[3:], training=False, kitti_set=True, rng=None)
    left, _, gt = ds.raw(0)
    return ds, (left.shape[0], left.shape[1], gt.shape[0])


def test_evaluation_handler_decodes_raw_pairs(tmp_path):
    ds, (H, W, Hg) = _kitti_pairs(tmp_path, 3)
    layout = [((2, 2, H, W, 3), np.uint8), ((2, Hg, W), np.float32)]                 # evaluate's _Slot, batch of 2
    with _workers(functools.partial(_decode_pair, ds, (H, W, Hg)), [layout]) as (host, slots):
        for j, index in enumerate((2, 1)):
            host.put(0, f"pair {index}", j, index)
        assert [host.get() for _ in range(2)] == [("decoded", 0, None)] * 2
        img, gt = slots[0].views
        for j, index in enumerate((2, 1)):
            left, right, g = ds.raw(index)
            assert np.array_equal(img[0, j], left) and np.array_equal(img[1, j], right) and np.array_equal(gt[j], g)


def test_a_handler_error_comes_back_naming_the_task(tmp_path):
    with _workers(_pair_task, [PAIR_LAYOUT]) as (host, _):
        host.put(0, "decode of pair 7", "decode", str(tmp_path / "missing.png"), KITTI_PAIR[1])
        with pytest.raises(RuntimeError, match=r"^decode of pair 7: FileNotFoundError: .*missing\.png"):
            host.get()
    ds, (H, W, Hg) = _kitti_pairs(tmp_path, 1)
    layout = [((2, 1, H, W, 3), np.uint8), ((1, Hg, W), np.float32)]
    with _workers(functools.partial(_decode_pair, ds, (H, W, Hg + 1)), [layout]) as (host, _):   # not the first pair's shape
        host.put(0, "pair 0", 0, 0)
        with pytest.raises(RuntimeError, match=r"^pair 0: ValueError: .*differ from the first pair's"):
            host.get()


def test_a_dead_worker_is_reported_instead_of_waited_for():
    with _workers(_pair_task, [PAIR_LAYOUT]) as (host, _):
        os.kill(host.procs[0].pid, signal.SIGKILL)
        host.procs[0].join(timeout=30.0)
        with pytest.raises(RuntimeError, match="a host worker process died"):
            host.get()
