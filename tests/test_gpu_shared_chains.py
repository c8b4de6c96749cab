"""The arithmetic chains that several kernels share (lws_device_math.h: the soft-argmin, the bilinear blend), through every entry
point that has one of its own: k_softargmin, k_softargmin_conf and k_upsample_add give the C oracle's bits.  The kernels without an
entry point (k_softargmin_upsample, k_volume_l1_warp, the deferred maps) are held by the forward's bit-exact tests."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, LOW_H, LOW_W = 2, 5, 11          # ragged against the 64-thread block of k_softargmin and both tiles (4 x 8, 2 x 4) of k_softargmin_conf


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def cu(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def assert_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    bad = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert bad == 0, f"{what}: {bad}/{want.size} elements differ, max abs {np.abs(got - want).max():.3e}"


@functools.lru_cache(maxsize=None)
def softargmin_case(D, start):
    """cost [B,D,5,11] and the C oracle's soft-argmin of it (computed once, read-only)."""
    from oracle import c_oracle as C
    cost = np.random.default_rng(100 + D).uniform(0.0, 12.0, (B, D, LOW_H, LOW_W)).astype(np.float32)
    cost[0, :, 0, :] = np.linspace(0, 300, D, dtype=np.float32)[:, None]      # exp underflows on all but one hypothesis
    cost[0, :, 1, :] = 1e4
    cost[0, D // 3, 1, :] = -1e4                                               # one-hot
    want = C.softargmin(cost, start)
    cost.setflags(write=False)
    want.setflags(write=False)
    return cost, want


@pytest.mark.parametrize("centred", [False, True], ids=["start0", "centred"])
@pytest.mark.parametrize("D", [9, 24, 32, 7])       # the three register forms and the generic one
def test_softargmin_entry_points_share_one_chain(dev, hip_lib, D, centred):
    from lwsnet_amd import ops
    start = float(-(D // 2)) if centred else 0.0
    cost, want = softargmin_case(D, start)
    assert want[0, 1, 0] == np.float32(start + D // 3)
    c = cu(cost, dev)
    low = ops.softargmin(c, start)
    conf = ops.softargmin_conf(c, start, 8 * LOW_H, 8 * LOW_W).disp_low
    assert_bits(low, want, f"softargmin D={D} start={start}")
    assert_bits(conf, want, f"softargmin_conf.disp_low D={D} start={start}")
    assert torch.equal(low, conf)


@pytest.mark.parametrize("h,w,H,W", [(5, 11, 40, 88), (8, 32, 63, 255)], ids=["x8", "non_integer_ratio"])
def test_upsample_add_matches_c_oracle(dev, hip_lib, h, w, H, W):
    from lwsnet_amd import ops
    from oracle import c_oracle as C
    rng = np.random.default_rng(7)
    low = rng.uniform(-6.0, 30.0, (B, h, w)).astype(np.float32)
    prev = rng.uniform(0.0, 190.0, (B, 1, H, W)).astype(np.float32)
    assert_bits(ops.upsample_add(cu(low, dev), cu(prev, dev), H, W), C.upsample_add(low, prev, H, W), f"upsample_add {h}x{w} -> {H}x{W}")
    assert_bits(ops.upsample_add(cu(low, dev), None, H, W), C.upsample_add(low, None, H, W), f"upsample {h}x{w} -> {H}x{W}")
