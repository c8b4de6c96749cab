"""postprocess.run_chain on the device, bit for bit against the same steps composed by hand, stage by stage, from
LWSNet.forward_lr, ops.speckle_filter and ops.wmedian_filter.  The batch is two synth.make_pair(64, 256, seed) pairs, the smallest
shape the model's tests use: B = 2 is what a wrong slice of the maps concatenated along the batch would mix up.  On the first pair
(tests/test_gpu_wmedian.py, above test_forward_lr_speckle_wmedian_point_cloud_chain) tau = 2 keeps 363 pixels of stage 4, the
speckle filter at size 1 keeps 83 of them, and the 5 x 5 median with fill_min 4 changes 26 and fills 74: nothing is vacuous."""
import numpy as np
import pytest

import guarded as G

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

H, W = 64, 256
FLAGS = dict(lr_check=2.0, speckle=1, speckle_diff=1.0, wmedian=2, wmedian_sigma=10.0, wmedian_fill=4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev, hip_lib):
    from lwsnet_amd.models import LWSNet
    from lwsnet_amd.weights import default_args, make_state_dict
    return LWSNet(default_args(), device=dev).set_state_dict(make_state_dict(7)).eval()


@pytest.fixture(scope="module")
def batch(dev):
    """(left, right) float32 [2,3,H,W] and the guide, the uint8 [2,H,W,3] images the left inputs were normalised from, on the device."""
    from lwsnet_amd.synth import make_pair, to_rgb8
    pairs = [make_pair(H, W, seed)[:2] for seed in (0, 1)]
    left, right = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    return left, right, torch.from_numpy(np.stack([to_rgb8(img) for img in left])).to(dev)


def host(t):
    return t.detach().cpu().numpy()


def assert_maps(got, want, what):
    assert len(got) == len(want) == 4
    for s in range(4):
        G.assert_bits(got[s], host(want[s]), f"{what}, stage {s + 1}")


def test_chain_with_every_stage_on(model, batch):
    from lwsnet_amd import ops
    from lwsnet_amd.postprocess import Options, run_chain
    left, right, guide = batch
    got = run_chain(model, left, right, Options.make(**FLAGS), guide)
    lr = model.forward_lr(left, right, tau=2.0, fill=False)
    wlut = ops.wmedian_lut(10.0)
    sp = [ops.speckle_filter(lr.disp[s], 1, 1.0, mask=lr.mask[s], fill=False) for s in range(4)]
    wm = [ops.wmedian_filter(sp[s].disp, 2, rgb=guide, wlut=wlut, mask=sp[s].mask, fill_min=4) for s in range(4)]
    kept = sum(int((host(r.mask) == 1).sum()) for r in sp)
    holes_filled = sum(int(host(r.counts)[:, 1].sum()) for r in wm)
    print(f"chain: kept {kept} of {4 * 2 * H * W}, filled {holes_filled}; stage 4 of pair 0: checked "
          f"{int((host(lr.mask[3])[0] == 1).sum())}, kept {int((host(sp[3].mask)[0] == 1).sum())}, changed and filled {host(wm[3].counts)[0].tolist()}")
    assert kept > 0 and holes_filled > 0, "the chain must keep pixels and fill holes, or the comparison shows nothing"
    assert_maps(got.disp, [r.disp for r in wm], "final map")
    assert_maps(got.lr_masks, lr.mask, "left-right codes")
    assert_maps(got.speckle_masks, [r.mask for r in sp], "speckle codes")
    assert got.keep is None, "fill_min 4 fills holes: the geometry outputs get no codes"
    G.assert_bits(got.lr_density, lr.density, "density")
    G.assert_bits(got.speckle_counts, np.stack([host(r.counts) for r in sp]), "speckle counts")
    G.assert_bits(got.wmedian_counts, np.stack([host(r.counts) for r in wm]), "median counts")
    # fill_min 0 fills nothing: the same codes reach the median, and the geometry outputs keep the speckle filter's
    unfilled = run_chain(model, left, right, Options.make(**dict(FLAGS, wmedian_fill=0)), guide)
    assert_maps(unfilled.keep, [r.mask for r in sp], "codes kept for geometry")
    assert_maps(unfilled.disp, [ops.wmedian_filter(sp[s].disp, 2, rgb=guide, wlut=wlut, mask=sp[s].mask, fill_min=0).disp for s in range(4)],
                "final map without hole filling")


def test_chain_with_lr_fill(model, batch):
    """--lr_fill with the speckle filter on: the check runs unfilled, the speckle filter does the one row fill, the median
    filters the whole map without codes, and the geometry outputs get none."""
    from lwsnet_amd import ops
    from lwsnet_amd.postprocess import Options, run_chain
    left, right, guide = batch
    got = run_chain(model, left, right, Options.make(lr_fill=True, **FLAGS), guide)
    lr = model.forward_lr(left, right, tau=2.0, fill=False)
    wlut = ops.wmedian_lut(10.0)
    sp = [ops.speckle_filter(lr.disp[s], 1, 1.0, mask=lr.mask[s], fill=True) for s in range(4)]
    wm = [ops.wmedian_filter(sp[s].disp, 2, rgb=guide, wlut=wlut, mask=None, fill_min=4) for s in range(4)]
    dropped = sum(int((host(r.mask) != 1).sum()) for r in sp)
    changed = sum(int(host(r.counts)[:, 0].sum()) for r in wm)
    print(f"chain with the row fill: dropped and filled {dropped} of {4 * 2 * H * W}, the median changed {changed}")
    assert 0 < dropped < 4 * 2 * H * W and changed > 0, "the fill and the median must both do something"
    assert_maps(got.disp, [r.disp for r in wm], "final map")
    assert_maps(got.lr_masks, lr.mask, "left-right codes")
    assert_maps(got.speckle_masks, [r.mask for r in sp], "speckle codes")
    assert got.keep is None
    G.assert_bits(got.lr_density, lr.density, "density")
    G.assert_bits(got.speckle_counts, np.stack([host(r.counts) for r in sp]), "speckle counts")
    G.assert_bits(got.wmedian_counts, np.stack([host(r.counts) for r in wm]), "median counts")


def test_chain_with_every_stage_off(model, batch):
    from lwsnet_amd.postprocess import Options, run_chain
    left, right, _ = batch
    got = run_chain(model, left, right, Options())
    assert_maps(got.disp, model(left, right), "stage map")
    assert got[1:] == (None,) * 6, "no stage ran: no codes, no density, no counts"


def test_ops_call_runs_on_the_current_stream(dev, hip_lib):
    """ops._call, the one path every wrapper takes into the library: the launch goes to the stream that is current at the call, on
    the tensor's device, and a None argument arrives as NULL (prev).  The result of a fresh stream is complete once THAT stream
    is synchronised -- nothing device-wide is waited for, so an output computed on another stream would be read early."""
    from lwsnet_amd import ops
    low = torch.tensor([[[0.5, 1.25, 2.0], [3.0, 0.75, 1.5]]], device=dev)
    want = host(ops.upsample_add(low, None, 4, 6))                          # default stream; the copy waits for it, and for `low`
    assert want.shape == (1, 1, 4, 6) and want.min() > 0
    s = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(s):
        got = ops.upsample_add(low, None, 4, 6)
        got_host = got.cpu()                                                # queued on s, behind the launch if the launch is on s
    s.synchronize()
    G.assert_bits(got_host, want, "upsample_add on a fresh stream")
