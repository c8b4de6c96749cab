"""Per-op wrappers over the C ABI for torch ROCm tensors (device memory + stream plumbing only).

Each function mirrors one reference symbol (see include/lwsnet_hip.h for file:line) and
launches the hand-written HIP kernel on torch's current stream.  No CPU path exists:
tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes
import math
from collections import namedtuple

import torch

from . import _lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a torch tensor on a HIP device (the disparity path has no CPU fallback)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _arr(ts, n=4):
    """The device pointers of up to n tensors as the void *[n] of the C ABI (a None and the missing entries: NULL)."""
    return (ctypes.c_void_p * n)(*[t.data_ptr() if t is not None else None for t in ts])


def _call(name, dev, *args):
    """The library's `name` on device `dev` and torch's current stream there, which goes last: a tensor or None among args becomes
    its device pointer, everything else passes through unchanged."""
    with torch.cuda.device(dev):
        _lib.call(name, *[_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args], _stream())


def _imagenet_stats():
    """The (mean, std) float[3] arguments of the kernels that normalise an image for the network."""
    from .synth import IMAGENET_MEAN, IMAGENET_STD
    return tuple((ctypes.c_float * 3)(*[float(v) for v in a]) for a in (IMAGENET_MEAN, IMAGENET_STD))


def _disp_map(t, name):
    """t as a contiguous float32 device tensor that must be [B,1,H,W]."""
    t = _dev(t, name)
    if t.dim() != 4 or t.shape[1] != 1:
        raise ValueError(f"{name} must be [B,1,H,W]; got {tuple(t.shape)}")
    return t


def _stage_maps(like=None, **lists):
    """name = list of 1-4 stage maps: every map float32 on one device and of the shape [B,1,H,W] of the first, or of the (shape,
    device) `like`.  Returns the lists of contiguous tensors, that shape and the device."""
    ts = {name: [_dev(t, f"{name}[{s}]") for s, t in enumerate(v)] for name, v in lists.items()}
    first = next(iter(lists))
    shape, dev = like or (tuple(_disp_map(ts[first][0], f"{first}[0]").shape), ts[first][0].device)
    for name, v in ts.items():
        for s, t in enumerate(v):
            if tuple(t.shape) != shape or t.device != dev:
                raise ValueError(f"{name}[{s}] must be {shape} on {dev}; got {tuple(t.shape)} on {t.device}")
    return list(ts.values()), shape, dev


def _check_outputs(n, shape, dev, want_right):
    """The (out, mask, right, row_kept) outputs of a check of n maps of `shape` = [B,1,H,W]; right is None unless want_right."""
    out = [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(n)]
    mask = [torch.empty(shape, device=dev, dtype=torch.uint8) for _ in range(n)]
    right = [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(n)] if want_right else None
    return out, mask, right, torch.empty((n, shape[0], shape[2]), device=dev, dtype=torch.int32)


def _tensor_of(t, name, dt, shape, device, tail=""):
    """t made contiguous: it must be a tensor of dtype dt and exactly `shape` on `device`; `tail` ends the message."""
    if not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{name} must be a {str(dt).split('.')[-1]} {tuple(shape)} tensor on {device}{tail}")
    return t.contiguous()


def _code_map(mask, d):
    """mask: None, or the uint8 code map of the maps d (same shape and device), made contiguous."""
    return None if mask is None else _tensor_of(mask, "mask", torch.uint8, d.shape, d.device, " (the lws_lr_check code map)")


def _guide(rgb, d):
    """rgb: the uint8 [B,H,W,3] images that go with the maps d [B,1,H,W], made contiguous."""
    B, _, H, W = d.shape
    return _tensor_of(rgb, "rgb", torch.uint8, (B, H, W, 3), d.device)


def _ground_codes(codes, d):
    """codes: the uint8 codes ground_classify returns for the maps d (same shape and device), made contiguous."""
    return _tensor_of(codes, "codes", torch.uint8, d.shape, d.device, " (what ground_classify returns)")


def _height_map(height, d):
    """height: the float32 heights ground_classify returns for the maps d (same shape and device), made contiguous."""
    height = _disp_map(height, "height")
    if tuple(height.shape) != tuple(d.shape) or height.device != d.device:
        raise ValueError(f"height must be {tuple(d.shape)} on {d.device}")
    return height


def _int_in(name, v, lo, hi, what=None):
    """v as an int that must lie in lo .. hi; `what` words the range where the default wording does not serve."""
    if isinstance(v, bool) or int(v) != v or not lo <= v <= hi:
        raise ValueError(f"{name} must be {what or f'an integer in {lo} .. {hi}'}, got {v}")
    return int(v)


def _finite_nonneg(name, v):
    if not (math.isfinite(v) and v >= 0):
        raise ValueError(f"{name} must be finite and >= 0, got {v}")
    return float(v)


def _finite_pos(name, v):
    if not (math.isfinite(v) and v > 0):
        raise ValueError(f"{name} must be finite and > 0, got {v}")
    return float(v)


def _int_indexed(H, W, name, op, what="maps", sides=False):
    """Refuses images of 2^31 pixels or more, which the kernels of `op` index with an int; with `sides`, also a side above 2^24."""
    if H * W >= 1 << 31 or (sides and max(H, W) > 1 << 24):
        raise ValueError(f"{name + ' is ' if name else ''}{H}x{W}: {op} takes {what} of fewer than 2^31 pixels"
                         f"{' and at most 2^24 a side' if sides else ''}")


def _device_rows(t, name, shape, device, host_rows):
    """t as a float32 device tensor of `shape`: a device tensor (egomotion's pose block, say) is taken as it is and nothing is read
    back; anything else is what host_rows() makes of it, the op's own reading of host numbers as a numpy array, uploaded."""
    if isinstance(t, torch.Tensor) and t.is_cuda:
        return _tensor_of(t, name, torch.float32, shape, device)
    return torch.from_numpy(host_rows()).to(device)


def _workspace(name, device, *dims):
    """The uint8 workspace of the size the library's `name`(*dims) asks for."""
    return torch.empty((_lib.nbytes(name, *dims),), device=device, dtype=torch.uint8)


def volume_l1_shift(feat_l, feat_r, maxdisp):
    """LWSNet._build_volume_2d (models/models.py:58-76)."""
    L, R = _dev(feat_l, "feat_l"), _dev(feat_r, "feat_r")
    if L.shape != R.shape or L.dim() != 4:
        raise ValueError(f"feat_l/feat_r must both be [B,C,h,w]; got {tuple(L.shape)} and {tuple(R.shape)}")
    B, C, h, w = L.shape
    cost = torch.empty((B, maxdisp, h, w), device=L.device, dtype=torch.float32)
    _call("lws_volume_l1_shift", L.device, L, R, cost, B, C, h, w, int(maxdisp))
    return cost


def volume_l1_warp(feat_l, feat_r, prev_disp, maxdisp, return_wflow=False):
    """forward() glue (models/models.py:119-121) + _build_volume_2d3 (:78-104) + warp (:28-55)."""
    L, R, P = _dev(feat_l, "feat_l"), _dev(feat_r, "feat_r"), _dev(prev_disp, "prev_disp")
    if L.shape != R.shape or L.dim() != 4:
        raise ValueError(f"feat_l/feat_r must both be [B,C,h,w]; got {tuple(L.shape)} and {tuple(R.shape)}")
    B, C, h, w = L.shape
    if P.dim() != 4 or P.shape[0] != B or P.shape[1] != 1:
        raise ValueError(f"prev_disp must be [B,1,H,W]; got {tuple(P.shape)}")
    H, W = P.shape[2], P.shape[3]
    cost = torch.empty((B, 2 * maxdisp - 1, h, w), device=L.device, dtype=torch.float32)
    wflow = torch.empty((B, h, w), device=L.device, dtype=torch.float32) if return_wflow else None
    _call("lws_volume_l1_warp", L.device, L, R, P, cost, wflow, B, C, h, w, H, W, int(maxdisp))
    return (cost, wflow) if return_wflow else cost


def conv3d_stack(handle, stage, cost):
    """volume_postprocess[stage](cost) + cost (models/models.py:136-138)."""
    c = _dev(cost, "cost")
    if c.dim() != 4:
        raise ValueError(f"cost must be [B,D,h,w]; got {tuple(c.shape)}")
    B, D, h, w = c.shape
    out = torch.empty_like(c)
    _call("lws_conv3d_stack", c.device, handle, int(stage), c, out, B, D, h, w)
    return out


def softargmin(cost, start):
    """F.softmax(-cost, 1) + disparity_regression (models/models.py:142,151-152,167-179)."""
    c = _dev(cost, "cost")
    B, D, h, w = c.shape
    low = torch.empty((B, h, w), device=c.device, dtype=torch.float32)
    _call("lws_softargmin", c.device, c, low, B, D, h, w, float(start))
    return low


SoftargminConf = namedtuple("SoftargminConf", ["disp_low", "peak_low", "sigma_low", "conf", "sigma"])


def softargmin_conf(cost, start, H, W, disp_low=True, peak_low=True, sigma_low=True, conf=True, sigma=True):
    """lws_softargmin_conf (include/lwsnet_hip.h): the soft-argmin of cost [B,D,h,w] with the confidence and the standard deviation of
    its distribution.  Returns a SoftargminConf: disp_low (bit-equal to softargmin), peak_low, sigma_low [B,h,w] and conf, sigma
    [B,1,H,W]; an output switched off by its keyword is None and is not computed."""
    c = _dev(cost, "cost")
    if c.dim() != 4:
        raise ValueError(f"cost must be [B,D,h,w]; got {tuple(c.shape)}")
    B, D, h, w = c.shape
    outs = [torch.empty((B, h, w), device=c.device, dtype=torch.float32) if on else None for on in (disp_low, peak_low, sigma_low)]
    outs += [torch.empty((B, 1, int(H), int(W)), device=c.device, dtype=torch.float32) if on else None for on in (conf, sigma)]
    _call("lws_softargmin_conf", c.device, c, B, D, h, w, float(start), int(H), int(W), *outs)
    return SoftargminConf(*outs)


def upsample_add(disp_low, prev, H, W):
    """models/models.py:145-148,153-156."""
    low = _dev(disp_low, "disp_low")
    B, h, w = low.shape
    prev = _dev(prev, "prev") if prev is not None else None
    out = torch.empty((B, 1, H, W), device=low.device, dtype=torch.float32)
    _call("lws_upsample_add", low.device, low, prev, out, B, h, w, int(H), int(W))
    return out


def disparity_stages(handle, feats_l, feats_r, H, W):
    """The body of `for scale in range(3)` (models/models.py:115-156): returns [pred1, pred2, pred3]."""
    fl = [_dev(t, f"feats_l[{i}]") for i, t in enumerate(feats_l)]
    fr = [_dev(t, f"feats_r[{i}]") for i, t in enumerate(feats_r)]
    if len(fl) != 3 or len(fr) != 3:
        raise ValueError("feats_l / feats_r must hold the three feature maps (1/8, 1/4, 1/2)")
    B = fl[0].shape[0]
    h2, w2 = (H + 1) // 2, (W + 1) // 2                 # the stem convolution gives ceil(H/2) (submodules.py:118-125)
    want = [(B, 16, h2 // 4, w2 // 4), (B, 16, h2 // 2, w2 // 2), (B, 8, h2, w2)]
    for i in range(3):
        if tuple(fl[i].shape) != want[i] or tuple(fr[i].shape) != want[i]:
            raise ValueError(f"stage {i + 1} features must be {want[i]}; got {tuple(fl[i].shape)} / {tuple(fr[i].shape)}")
    preds = [torch.empty((B, 1, H, W), device=fl[0].device, dtype=torch.float32) for _ in range(3)]
    _call("lws_disparity_stages", fl[0].device, handle, _arr(fl, 3), _arr(fr, 3), B, int(H), int(W), _arr(preds, 3))
    return preds


def feature_extraction(handle, img):
    """feature_extraction (models/submodules.py:113-188): [N,3,H,W] -> [1/8 (16 ch), 1/4 (16 ch), 1/2 (8 ch)]."""
    x = _dev(img, "img")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"img must be [N,3,H,W]; got {tuple(x.shape)}")
    N, _, H, W = x.shape
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    f8 = torch.empty((N, 16, h2 // 4, w2 // 4), device=x.device, dtype=torch.float32)
    f4 = torch.empty((N, 16, h2 // 2, w2 // 2), device=x.device, dtype=torch.float32)
    f2 = torch.empty((N, 8, h2, w2), device=x.device, dtype=torch.float32)
    _call("lws_feature_extraction", x.device, handle, x, N, H, W, f8, f4, f2)
    return [f8, f4, f2]


def refine(handle, left, pred3):
    """models/models.py:158-162: pred4 = pred3 + refinement2(cat(refinement1_left(left), refinement1_disp(pred3)))."""
    l, p3 = _dev(left, "left"), _dev(pred3, "pred3")
    B, _, H, W = l.shape
    if tuple(p3.shape) != (B, 1, H, W):
        raise ValueError(f"pred3 must be {(B, 1, H, W)}; got {tuple(p3.shape)}")
    out = torch.empty_like(p3)
    _call("lws_refine", l.device, handle, l, p3, B, H, W, out)
    return out


def stage_outputs(out, B, H, W, device):
    """The four [B,1,H,W] destinations of a forward: `out` is None or a list of four entries, each None (allocated here) or
    a contiguous float32 tensor of exactly that shape on `device` -- a raw pointer is handed to the library, so a strided or
    wrong-sized tensor would be an out-of-bounds device write (shared by ops.forward and ForwardPool.submit)."""
    if out is not None and (not isinstance(out, (list, tuple)) or len(out) != 4):
        raise ValueError("out must be a list of four tensors (or None entries), one per stage")
    preds = []
    for s in range(4):
        t = out[s] if out is not None else None
        if t is None:
            t = torch.empty((B, 1, H, W), device=device, dtype=torch.float32)
        elif not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == torch.device(device) and t.dtype == torch.float32
                  and t.is_contiguous() and tuple(t.shape) == (B, 1, H, W)):
            raise ValueError(f"out[{s}] must be a contiguous float32 tensor of shape {(B, 1, H, W)} on {device}")
        preds.append(t)
    return preds


def forward(handle, left, right, out=None):
    """LWSNet.forward (models/models.py:106-164): list of 4 x [B,1,H,W].  `out` (optional): a list of four destinations;
    entries that are None are allocated here, the others must be contiguous float32 [B,1,H,W] device tensors (a slot of
    a staging buffer, say) and are written in place."""
    l, r = _dev(left, "left"), _dev(right, "right")
    B, _, H, W = l.shape
    preds = stage_outputs(out, B, H, W, l.device)
    _call("lws_forward", l.device, handle, l, r, B, H, W, _arr(preds))
    return preds


def forward_conf(handle, left, right, conf=True, sigma=True):
    """lws_forward_conf (include/lwsnet_hip.h): the forward plus the confidence and sigma maps of the three volume stages.  Returns
    (preds, conf, sigma): four, three and three [B,1,H,W] maps; conf / sigma is None when switched off by its keyword."""
    l, r = _dev(left, "left"), _dev(right, "right")
    B, _, H, W = l.shape
    preds = stage_outputs(None, B, H, W, l.device)
    cs, ss = ([torch.empty((B, 1, H, W), device=l.device, dtype=torch.float32) for _ in range(3)] if on else None for on in (conf, sigma))
    _call("lws_forward_conf", l.device, handle, l, r, B, H, W, _arr(preds), _arr(cs or [], 3), _arr(ss or [], 3))
    return preds, cs, ss


def confidence_codes(conf, sigma, min_conf=None, max_sigma=None, stages=(0, 1, 2)):
    """A uint8 code map with lws_lr_check's meaning from forward_conf's maps: 1 where every stage in `stages` has conf >= min_conf and
    sigma <= max_sigma (a threshold that is None is not applied; NaN fails both), else 0.  Plain comparisons on the device;
    speckle_filter, wmedian_filter, depth_maps and point_cloud take the result as their `mask`."""
    stages = tuple(int(s) for s in stages)
    if not stages or any(s < 0 or s > 2 for s in stages):
        raise ValueError(f"stages must be a non-empty selection of 0, 1, 2; got {stages}")
    if (min_conf is not None and conf is None) or (max_sigma is not None and sigma is None):
        raise ValueError("a threshold was given for maps that are None")
    maps = conf if conf is not None else sigma
    if maps is None:
        raise ValueError("conf and sigma are both None")
    first = maps[stages[0]]

    def stage_map(ts, name, s):                 # plain torch on whatever device the maps live on
        t = ts[s]
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 1 or t.shape != first.shape \
                or t.device != first.device:
            raise ValueError(f"{name}[{s}] must be a float32 [B,1,H,W] tensor of the shape and device of the other maps")
        return t.as_subclass(torch.Tensor)

    ok = torch.ones(first.shape, device=first.device, dtype=torch.bool)
    for s in stages:
        if min_conf is not None:
            ok &= stage_map(conf, "conf", s) >= float(min_conf)
        if max_sigma is not None:
            ok &= stage_map(sigma, "sigma", s) <= float(max_sigma)
    return ok.to(torch.uint8)


def preprocess_rgb8(rgb_u8, out=None):
    """ToTensor + Normalize(imagenet) of inference.py:83-85,102-103 on the device: rgb_u8 [B,H,W,3] uint8 -> [B,3,H,W] float32,
    bit for bit lwsnet_amd.imageio.to_input (numpy)."""
    if not isinstance(rgb_u8, torch.Tensor) or not rgb_u8.is_cuda or rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 4 or rgb_u8.shape[3] != 3:
        raise ValueError("rgb_u8 must be a [B,H,W,3] uint8 tensor on a HIP device")
    rgb_u8 = rgb_u8.contiguous()
    B, H, W, _ = rgb_u8.shape
    if out is None:
        out = torch.empty((B, 3, H, W), device=rgb_u8.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, 3, H, W) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous [B,3,H,W] float32 device tensor")
    mean, std = _imagenet_stats()
    _call("lws_preprocess_rgb8", rgb_u8.device, rgb_u8, out, B, H, W, mean, std)
    return out


def apply_lut8(disp, lut_dev, out=None):
    """`.astype(np.uint8)` + colour map of inference.py:114-115 on the device: disp (any shape) float32 -> [...,3] uint8 through
    lut_dev ([256,3] uint8 on the device), bit for bit lwsnet_amd.imageio.disparity_to_color."""
    d = _dev(disp, "disp")
    if not isinstance(lut_dev, torch.Tensor) or not lut_dev.is_cuda or lut_dev.dtype != torch.uint8 or lut_dev.numel() != 768:
        raise ValueError("lut_dev must be a [256,3] uint8 tensor on a HIP device")
    if out is None:
        out = torch.empty(tuple(d.shape) + (3,), device=d.device, dtype=torch.uint8)
    elif out.numel() != 3 * d.numel() or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 device tensor with 3 bytes per disparity value")
    _call("lws_apply_lut8", d.device, d, lut_dev.contiguous(), out, ctypes.c_int64(d.numel()))
    return out


METRIC_MODES = {"kitti": 0, "epe": 1}


def _gt_maps(gt, row_offset, mode, **lists):
    """The inputs the evaluation ops share: mode as 0 / 1, gt [B,Hg,W], row_offset >= 0 and, per name, a list of maps that must
    be [B,1,Hg + row_offset,W] on gt's device.  Returns mode, the contiguous gt, row_offset and the lists of contiguous maps."""
    mode = METRIC_MODES.get(mode, mode)
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 / 'kitti' or 1 / 'epe', got {mode!r}")
    g = _dev(gt, "gt")
    if g.dim() != 3:
        raise ValueError(f"gt must be [B,Hg,W]; got {tuple(g.shape)}")
    B, Hg, W = g.shape
    row_offset = int(row_offset)
    if row_offset < 0:
        raise ValueError(f"row_offset must be >= 0, got {row_offset}")
    return mode, g, row_offset, _stage_maps(like=((B, 1, Hg + row_offset, W), g.device), **lists)[0]


def stage_metrics(preds, gt, row_offset, maxdisp, mode):
    """The per-image sums behind the reference's test loops (finetune.py:184-219 error_estimating, mode 0 / "kitti";
    train.py:169-199, mode 1 / "epe") on the device.  preds: the four [B,1,Hp,W] float32 stage maps; gt: [B,Hg,W] float32 with
    Hp = Hg + row_offset.  Returns device tensors counts [4,B,2] int64 = {valid, bad} and abs_sum [4,B] float64 (include/lwsnet_hip.h,
    lws_stage_metrics), allocated on the current stream."""
    if not isinstance(preds, (list, tuple)) or len(preds) != 4:
        raise ValueError("preds must be the four stage maps")
    mode, g, row_offset, (ps,) = _gt_maps(gt, row_offset, mode, preds=preds)
    B, Hg, W = g.shape
    work = _workspace("lws_stage_metrics_workspace", g.device, B, Hg, W)
    counts = torch.empty((4, B, 2), device=g.device, dtype=torch.int64)
    abs_sum = torch.empty((4, B), device=g.device, dtype=torch.float64)
    _call("lws_stage_metrics", g.device, _arr(ps), B, Hg + row_offset, W, row_offset, g, Hg, float(maxdisp), int(mode), work, counts,
          abs_sum)
    return counts, abs_sum


SPARS_KINDS = {"sigma": 0, "conf": 1}


def sparsification(preds, unc, gt, row_offset, maxdisp, mode, kind):
    """The integer histograms behind the sparsification curves (include/lwsnet_hip.h, lws_sparsification; the curves and AUSE:
    lwsnet_amd.metrics.sparsification_curves).  preds, unc: 1-4 [B,1,Hp,W] float32 maps each, unc[s] the uncertainty that ranks the
    pixels of preds[s]: kind 0 / "sigma" (lower = more trusted) or 1 / "conf" (ranked by 1 - conf); gt, row_offset, maxdisp and
    mode as for stage_metrics.  Returns the device tensor hist [nmaps,B,2,1026,3] int64 = per map, image, ranking (0: by unc, 1: the
    oracle, by the error itself) and bin {pixels, bad pixels, error sum in 1/1024 px}, allocated on the current stream."""
    kind = SPARS_KINDS.get(kind, kind)
    if kind not in (0, 1):
        raise ValueError(f"kind must be 0 / 'sigma' or 1 / 'conf', got {kind!r}")
    if not isinstance(preds, (list, tuple)) or not isinstance(unc, (list, tuple)) or not 1 <= len(preds) <= 4 or len(unc) != len(preds):
        raise ValueError("preds and unc must be lists of the same 1-4 maps")
    mode, g, row_offset, (ps, us) = _gt_maps(gt, row_offset, mode, preds=preds, unc=unc)
    B, Hg, W = g.shape
    hist = torch.empty((len(ps), B, 2, _lib.LWS_SPARS_BINS, 3), device=g.device, dtype=torch.int64)
    _call("lws_sparsification", g.device, _arr(ps), _arr(us), len(ps), int(kind), B, Hg + row_offset, W, row_offset, g, Hg,
          float(maxdisp), int(mode), hist)
    return hist


def lr_pairs(left, right):
    """The input of the left-right check's one forward of 2B pairs (include/lwsnet_hip.h, lws_lr_pairs): left, right [B,3,H,W]
    float32 -> left2 = [left; mirror_w(right)], right2 = [right; mirror_w(left)], each [2B,3,H,W], bit copies."""
    l, r = _dev(left, "left"), _dev(right, "right")
    if l.dim() != 4 or l.shape[1] != 3 or l.shape != r.shape or l.device != r.device:
        raise ValueError(f"left/right must both be [B,3,H,W] on one device; got {tuple(l.shape)} and {tuple(r.shape)}")
    B, _, H, W = l.shape
    left2 = torch.empty((2 * B, 3, H, W), device=l.device, dtype=torch.float32)
    right2 = torch.empty_like(left2)
    _call("lws_lr_pairs", l.device, l, r, left2, right2, B, H, W)
    return left2, right2


def lr_check(dl, drm, tau, fill, want_right=True):
    """Left-right consistency check of 1-4 stage maps (include/lwsnet_hip.h, lws_lr_check): dl[s] the left-view maps, drm[s] the
    mirrored right-view maps, each [B,1,H,W] float32.  Returns (out, mask, right, row_kept): lists of [B,1,H,W] float32 checked
    (filled if `fill`) maps, uint8 codes (1 consistent, 0 inconsistent, 2 out of view) and un-mirrored right-view maps (None
    unless want_right), and an int32 [nmaps,B,H] device tensor of the consistent pixels per row."""
    if not isinstance(dl, (list, tuple)) or not isinstance(drm, (list, tuple)) or len(dl) != len(drm) or not 1 <= len(dl) <= 4:
        raise ValueError("dl and drm must be lists of the same 1-4 stage maps")
    (ls, rs), shape, dev = _stage_maps(dl=dl, drm=drm)
    B, _, H, W = shape
    out, mask, right, row_kept = _check_outputs(len(ls), shape, dev, want_right)
    _call("lws_lr_check", dev, _arr(ls), _arr(rs), len(ls), B, H, W, float(tau), int(bool(fill)), _arr(out), _arr(mask), _arr(right or []),
          row_kept)
    return out, mask, right, row_kept


def occlusion_check(dl, tau, fill, want_right=True):
    """One-forward occlusion check of 1-4 stage maps (include/lwsnet_hip.h, lws_occlusion_check): dl[s] the left-view maps,
    each [B,1,H,W] float32, splatted into the right view with a z-buffer.  Returns (out, mask, right, row_kept) as lr_check does:
    lists of [B,1,H,W] float32 checked (filled if `fill`) maps, uint8 codes (1 visible, 0 occluded by a nearer surface, 2 out of
    view) and right-view maps in the right camera's frame with 0 in the holes (None unless want_right), and an int32
    [nmaps,B,H] device tensor of the visible pixels per row."""
    if not isinstance(dl, (list, tuple)) or not 1 <= len(dl) <= 4:
        raise ValueError("dl must be a list of 1-4 stage maps")
    (ls,), shape, dev = _stage_maps(dl=dl)
    B, _, H, W = shape
    out, mask, right, row_kept = _check_outputs(len(ls), shape, dev, want_right)
    _call("lws_occlusion_check", dev, _arr(ls), len(ls), B, H, W, float(tau), int(bool(fill)), _arr(out), _arr(mask), _arr(right or []),
          row_kept)
    return out, mask, right, row_kept


def _geometry_inputs(disp, mask, cameras, min_disp, max_depth):
    """Shared checks of depth_maps / point_cloud: disp [B,1,H,W] float32, mask None or uint8 of that shape, cameras (None, one
    Camera or a list of B) -> (disp, mask, cam [B,5] float32 device tensor or None)."""
    from .geometry import camera_rows
    d = _disp_map(disp, "disp")
    mask = _code_map(mask, d)
    _finite_pos("min_disp", min_disp)
    if not max_depth > 0:
        raise ValueError(f"max_depth must be > 0 (inf allowed), got {max_depth}")
    cam = None
    if cameras is not None:
        cam = torch.from_numpy(camera_rows(cameras, d.shape[0])).to(d.device)
    return d, mask, cam


def depth_maps(disp, cameras=None, mask=None, min_disp=1.0, max_depth=float("inf"), depth=True, depth16=True, disp16=True):
    """Metric depth and KITTI's 16-bit disparity / depth PNG values of disparity maps (include/lwsnet_hip.h, lws_depth_maps).
    disp [B,1,H,W] float32; cameras: one lwsnet_amd.geometry.Camera or a list of B (needed for depth / depth16); mask: None or the
    uint8 lws_lr_check code map (only code-1 pixels count).  Returns (depth float32, depth16 uint16, disp16 uint16), each
    [B,1,H,W] or None where not asked for."""
    if not (depth or depth16 or disp16):
        raise ValueError("depth_maps: ask for at least one of depth, depth16, disp16")
    if (depth or depth16) and cameras is None:
        raise ValueError("depth_maps: depth and depth16 need cameras")
    d, mask, cam = _geometry_inputs(disp, mask, cameras if (depth or depth16) else None, min_disp, max_depth)
    outs = [torch.empty(d.shape, device=d.device, dtype=dt) if want else None
            for want, dt in ((depth, torch.float32), (depth16, torch.uint16), (disp16, torch.uint16))]
    B, _, H, W = d.shape
    _call("lws_depth_maps", d.device, d, mask, cam, B, H, W, float(min_disp), float(max_depth), *outs)
    return tuple(outs)


def point_cloud(disp, cameras, mask=None, rgb=None, min_disp=1.0, max_depth=float("inf")):
    """The valid pixels of disparity maps as coloured 3-D points (include/lwsnet_hip.h, lws_point_cloud).  disp [B,1,H,W] float32;
    cameras: one Camera or a list of B; mask: None or the uint8 lws_lr_check code map; rgb: None (white) or the uint8 [B,H,W,3]
    cropped left images.  Returns (points uint8 [B,H*W,16], counts int64 [B]): image b's counts[b] records
    {float X, Y, Z; uint8 r, g, b, 255} (lwsnet_amd.geometry.POINT_DTYPE) in raster order from points[b]; the rest is unwritten."""
    if cameras is None:
        raise ValueError("point_cloud needs cameras")
    d, mask, cam = _geometry_inputs(disp, mask, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    if rgb is not None:
        rgb = _guide(rgb, d)
    work = _workspace("lws_point_cloud_workspace", d.device, B, H)
    points = torch.empty((B, H * W, 16), device=d.device, dtype=torch.uint8)
    counts = torch.empty((B,), device=d.device, dtype=torch.int64)
    _call("lws_point_cloud", d.device, d, mask, rgb, cam, B, H, W, float(min_disp), float(max_depth), work, points, counts)
    return points, counts


def surface_normals(disp, cameras, mask=None, min_disp=1.0, max_depth=float("inf"), max_jump=1.0, normals=True, normals8=False):
    """Per-pixel surface normals of disparity maps from the 3 x 3 stencil of the pixel grid (include/lwsnet_hip.h,
    lws_surface_normals).  disp, cameras, mask, min_disp, max_depth as point_cloud; max_jump: the largest disparity step between
    two neighbouring pixels of one surface.  Returns (normals float32 [B,3,H,W], normals8 uint8 [B,H,W,3] -- the bytes of an
    OpenGL-convention normal map), each None where not asked for; an invalid pixel and one without two connected neighbours has
    the zero normal (128, 128, 128)."""
    if not (normals or normals8):
        raise ValueError("surface_normals: ask for at least one of normals, normals8")
    if cameras is None:
        raise ValueError("surface_normals needs cameras")
    d, mask, cam = _geometry_inputs(disp, mask, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    n = torch.empty((B, 3, H, W), device=d.device, dtype=torch.float32) if normals else None
    n8 = torch.empty((B, H, W, 3), device=d.device, dtype=torch.uint8) if normals8 else None
    max_jump = _finite_nonneg("max_jump", max_jump)
    _call("lws_surface_normals", d.device, d, mask, cam, B, H, W, float(min_disp), float(max_depth), max_jump, n, n8)
    return n, n8


SurfaceMesh = namedtuple("SurfaceMesh", ["points", "vnormals", "faces", "index", "counts"])
SurfaceMesh.__doc__ = """What surface_mesh returns: points uint8 [B,H*W,16] (the records of point_cloud), vnormals float32 [B,H*W,4]
{n.x, n.y, n.z, 0} per vertex (None without normals), faces int32 [B,max(1, 2*(H-1)*(W-1)),3], index int32 [B,1,H,W] (a pixel's
vertex index or -1; None unless want_index) and counts, an int64 [B,2] device tensor {vertices, faces}: image b's vertices are
points[b, :counts[b,0]], its faces faces[b, :counts[b,1]]; the rest is unwritten."""


def surface_mesh(disp, cameras, mask=None, rgb=None, min_disp=1.0, max_depth=float("inf"), max_jump=1.0, with_normals=True,
                 want_index=False):
    """An indexed triangle mesh of disparity maps that does not span depth discontinuities (include/lwsnet_hip.h,
    lws_surface_mesh): the vertices are point_cloud's records, two triangles per grid cell whose corners are connected (disparity
    steps <= max_jump).  with_normals: surface_normals runs first and its normals are gathered per vertex.  Returns a SurfaceMesh."""
    if cameras is None:
        raise ValueError("surface_mesh needs cameras")
    d, mask, cam = _geometry_inputs(disp, mask, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    if rgb is not None:
        rgb = _guide(rgb, d)
    dev = d.device
    work = _workspace("lws_surface_mesh_workspace", dev, B, H)
    n = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32) if with_normals else None
    vn = torch.empty((B, H * W, 4), device=dev, dtype=torch.float32) if with_normals else None
    points = torch.empty((B, H * W, 16), device=dev, dtype=torch.uint8)
    faces = torch.empty((B, max(1, 2 * (H - 1) * (W - 1)), 3), device=dev, dtype=torch.int32)
    index = torch.empty((B, 1, H, W), device=dev, dtype=torch.int32) if want_index else None
    counts = torch.empty((B, 2), device=dev, dtype=torch.int64)
    args = (B, H, W, float(min_disp), float(max_depth), _finite_nonneg("max_jump", max_jump))
    if with_normals:
        _call("lws_surface_normals", dev, d, mask, cam, *args, n, None)
    _call("lws_surface_mesh", dev, d, mask, rgb, cam, n, *args, work, points, vn, faces, index, counts)
    return SurfaceMesh(points, vn, faces, index, counts)


GROUND_STATUS = ("ok", "no ground", "degenerate")                     # info[b, 0] of ground_fit
GROUND_CODES = ("invalid", "ground", "obstacle", "overhead", "below", "no plane")      # the codes of ground_classify


def _hist_args(min_disp, sub, nbins, maxdisp):
    """(min_disp, sub, nbins) of vdisparity / ground_fit; nbins None: min(1024, sub * maxdisp)."""
    min_disp, sub = _finite_pos("min_disp", min_disp), _int_in("sub", sub, 1, 16)
    if nbins is None:
        nbins = min(1024, sub * _int_in("maxdisp", maxdisp, 1, 1 << 20), 256 * sub)
    return min_disp, sub, _int_in("nbins", nbins, 1, min(4096, 256 * sub))


def vdisparity(disp, mask=None, min_disp=1.0, sub=4, nbins=None, maxdisp=192):
    """The v-disparity image of disparity maps: per row, a histogram of the disparities in bins of 1 / sub pixels
    (include/lwsnet_hip.h, lws_vdisparity).  disp [B,1,H,W] float32; mask: None or the uint8 code map (only code-1 pixels count);
    nbins: None for min(1024, sub * maxdisp).  Returns hist uint32 [B,H,nbins]."""
    min_disp, sub, nbins = _hist_args(min_disp, sub, nbins, maxdisp)
    d = _disp_map(disp, "disp")
    mask = _code_map(mask, d)
    B, _, H, W = d.shape
    hist = torch.empty((B, H, nbins), device=d.device, dtype=torch.uint32)
    _call("lws_vdisparity", d.device, d, mask, B, H, W, min_disp, sub, nbins, hist)
    return hist


def ground_fit(disp, hist, mask=None, min_disp=1.0, sub=4, yh_range=None, qb_range=None, tol_bins=1, min_score=0, tol0=1.0, tol=1.0,
               iters=3):
    """The road's plane d = a*x + b*y + c of disparity maps: a Hough vote on their v-disparity image `hist` (vdisparity with the same
    mask, min_disp and sub), then iters + 1 least-squares passes on the maps (include/lwsnet_hip.h, lws_ground_fit).  yh_range: the
    horizon rows tried, (lo, hi), None for H/4 .. 3H/4; qb_range: the bottom row's bins tried, None for the upper two thirds of the
    bins; tol0 / tol: the inlier tolerance in pixels of pass 0 (against the voted line) and of the later passes.  Returns
    (plane float32 [B,4] = {a, b, c, 0}, NaN unless info[b,0] is 0; info int32 [B,8] = {status, yh, qB, score, inliers, 0, 0, 0}),
    both on the device; status: GROUND_STATUS."""
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.uint32 or hist.dim() != 3:
        raise ValueError("hist must be the uint32 [B,H,nbins] tensor vdisparity returns")
    nbins = int(hist.shape[2])
    min_disp, sub, nbins = _hist_args(min_disp, sub, nbins, 1)
    H = int(hist.shape[1])
    if yh_range is None:
        yh_hi = min(3 * H // 4, H - 2)
        yh_range = (min(H // 4, yh_hi), yh_hi)
    if qb_range is None:
        qb_range = (max(1, nbins // 3), nbins - 1)
    yh_lo, yh_hi = (_int_in("yh_range", v, -65536, H - 2) for v in yh_range)
    qb_lo, qb_hi = (_int_in("qb_range", v, 1, nbins - 1) for v in qb_range)
    if yh_lo > yh_hi or qb_lo > qb_hi:
        raise ValueError(f"yh_range {tuple(yh_range)} and qb_range {tuple(qb_range)} must each be (lo, hi) with lo <= hi")
    if (yh_hi - yh_lo + 1) * (qb_hi - qb_lo + 1) > 1 << 22:
        raise ValueError("yh_range x qb_range holds more than 2^22 candidates")
    tol_bins, iters = _int_in("tol_bins", tol_bins, 0, 8), _int_in("iters", iters, 0, 8)
    min_score = _int_in("min_score", min_score, 0, 2 ** 31 - 1)
    tol0, tol = _finite_nonneg("tol0", tol0), _finite_nonneg("tol", tol)
    d = _disp_map(disp, "disp")
    mask = _code_map(mask, d)
    B, _, _, W = d.shape
    if tuple(hist.shape[:2]) != (B, d.shape[2]) or hist.device != d.device:
        raise ValueError(f"hist must be [{B},{d.shape[2]},nbins] on {d.device}; got {tuple(hist.shape)} on {hist.device}")
    hist = hist.contiguous()
    work = _workspace("lws_ground_workspace", d.device, B, H, nbins)
    plane = torch.empty((B, 4), device=d.device, dtype=torch.float32)
    info = torch.empty((B, 8), device=d.device, dtype=torch.int32)
    _call("lws_ground_fit", d.device, d, mask, hist, B, H, W, min_disp, sub, nbins, yh_lo, yh_hi, qb_lo, qb_hi, tol_bins, min_score, tol0, tol,
          iters, work, plane, info)
    return plane, info


def _heights(ground_tol, max_height):
    ground_tol, max_height = _finite_nonneg("ground_tol", ground_tol), _finite_nonneg("max_height", max_height)
    if ground_tol > max_height:
        raise ValueError(f"ground_tol {ground_tol} must be <= max_height {max_height}")
    return ground_tol, max_height


def ground_classify(disp, cameras, plane, mask=None, min_disp=1.0, max_depth=float("inf"), ground_tol=0.2, max_height=3.0, height=True,
                    codes=True, counts=True):
    """The height of every valid pixel's point over the plane and a code per pixel (include/lwsnet_hip.h, lws_ground_classify;
    GROUND_CODES).  plane: the float32 [B,4] device tensor ground_fit returns; ground_tol, max_height in metres.  Returns
    (height float32 [B,1,H,W], codes uint8 [B,1,H,W], counts int64 [B,6]), each None where not asked for."""
    if not (height or codes):
        raise ValueError("ground_classify: ask for at least one of height, codes")
    if cameras is None:
        raise ValueError("ground_classify needs cameras")
    ground_tol, max_height = _heights(ground_tol, max_height)
    d, mask, cam = _geometry_inputs(disp, mask, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    plane = _tensor_of(plane, "plane", torch.float32, (B, 4), d.device, " (what ground_fit returns)")
    h = torch.empty(d.shape, device=d.device, dtype=torch.float32) if height else None
    c = torch.empty(d.shape, device=d.device, dtype=torch.uint8) if codes else None
    n = torch.empty((B, 6), device=d.device, dtype=torch.int64) if counts else None
    _call("lws_ground_classify", d.device, d, mask, cam, plane, B, H, W, float(min_disp), float(max_depth), ground_tol, max_height, h, c, n)
    return h, c, n


def _bev_args(code_bits, x_min, cell, grid, hmax):
    code_bits = _int_in("code_bits", code_bits, 0, 63)
    if hmax and code_bits & 0x33:
        raise ValueError(f"code_bits {code_bits} selects a code other than 2 and 3, whose heights are not positive: ask for no hmax")
    if not math.isfinite(x_min):
        raise ValueError(f"x_min must be finite, got {x_min}")
    cell = _finite_pos("cell", cell)
    if len(grid) != 2:
        raise ValueError(f"grid must be (Gx, Gz), got {grid}")
    return code_bits, float(x_min), cell, _int_in("grid", grid[0], 1, 4096), _int_in("grid", grid[1], 1, 4096)


def bev_grid(disp, cameras, codes, height=None, min_disp=1.0, max_depth=float("inf"), code_bits=1 << 2, x_min=-20.0, cell=0.2,
             grid=(200, 300), count=True, hmax=True):
    """An occupancy grid seen from above (include/lwsnet_hip.h, lws_bev_grid): the valid pixels whose code's bit is set in code_bits
    (default: obstacles), dropped into cells of `cell` metres; grid = (Gx, Gz): Gx cells across from x_min, Gz cells deep from the
    camera.  codes, height: what ground_classify returns.  Returns (count uint32 [B,Gz,Gx], hmax float32 [B,Gz,Gx] -- the largest
    height in the cell, 0 for an empty one), each None where not asked for."""
    if not (count or hmax):
        raise ValueError("bev_grid: ask for at least one of count, hmax")
    if cameras is None:
        raise ValueError("bev_grid needs cameras")
    if hmax and height is None:
        raise ValueError("bev_grid: hmax needs height")
    code_bits, x_min, cell, Gx, Gz = _bev_args(code_bits, x_min, cell, grid, hmax)
    d, _, cam = _geometry_inputs(disp, None, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    codes = _ground_codes(codes, d)
    if height is not None:
        height = _height_map(height, d)
    n = torch.empty((B, Gz, Gx), device=d.device, dtype=torch.uint32) if count else None
    top = torch.empty((B, Gz, Gx), device=d.device, dtype=torch.float32) if hmax else None
    _call("lws_bev_grid", d.device, d, cam, codes, height if hmax else None, B, H, W, float(min_disp), float(max_depth), code_bits, x_min, cell,
          Gx, Gz, n, top)
    return n, top


GroundResult = namedtuple("GroundResult", ["hist", "plane", "info", "height", "codes", "counts", "bev_count", "bev_hmax"])
GroundResult.__doc__ = """What ground returns, all on the device: hist uint32 [B,H,nbins] (vdisparity), plane float32 [B,4] and info
int32 [B,8] (ground_fit), height float32 [B,1,H,W], codes uint8 [B,1,H,W] and counts int64 [B,6] (ground_classify), bev_count uint32
and bev_hmax float32 [B,Gz,Gx] (bev_grid)."""


def ground(disp, cameras, mask=None, min_disp=1.0, max_depth=float("inf"), maxdisp=192, sub=4, nbins=None, yh_range=None, qb_range=None,
           tol_bins=1, min_score=0, tol0=1.0, tol=1.0, iters=3, ground_tol=0.2, max_height=3.0, code_bits=1 << 2, x_min=-20.0, cell=0.2,
           grid=(200, 300)):
    """Where the road is and what stands on it: vdisparity, ground_fit, ground_classify and bev_grid on the current stream, nothing
    read back in between.  Defaults: bins of a quarter pixel up to min(1024, 4 * maxdisp), horizon rows H/4 .. 3H/4, three passes
    after the voted line at 1 px, ground within 0.2 m, obstacles up to 3 m, a grid of 0.2 m cells 40 m wide and 60 m deep.
    Returns a GroundResult; lwsnet_amd.geometry.GroundPlane turns a plane row into camera height, pitch and roll."""
    if cameras is None:
        raise ValueError("ground needs cameras")
    _heights(ground_tol, max_height)
    _bev_args(code_bits, x_min, cell, grid, True)
    hist = vdisparity(disp, mask, min_disp, sub, nbins, maxdisp)
    plane, info = ground_fit(disp, hist, mask, min_disp, sub, yh_range, qb_range, tol_bins, min_score, tol0, tol, iters)
    height, codes, counts = ground_classify(disp, cameras, plane, mask, min_disp, max_depth, ground_tol, max_height)
    n, top = bev_grid(disp, cameras, codes, height, min_disp, max_depth, code_bits, x_min, cell, grid)
    return GroundResult(hist, plane, info, height, codes, counts, n, top)


StixelResult = namedtuple("StixelResult", ["rows", "vals", "udisp"])
StixelResult.__doc__ = """What stixels returns, all on the device, S = ceil(W / width) strips: rows int32 [B,S,layers,4] = {n, y_top,
y_base, k_peak}, vals float32 [B,S,layers,4] = {disparity, z, X, height}, udisp uint32 [B,S,nbins] (None unless asked for).  A slot
with n = 0 is empty: y_top = y_base = -1 and four zeros."""


def _stixel_args(min_disp, code_bits, width, maxdisp, sub, nbins, tol_bins, min_count, min_row, max_gap, layers):
    """The validated scalar arguments of stixels, defaults resolved: min_count None is 2 * width, min_row None max(1, width // 2)."""
    min_disp, sub, nbins = _hist_args(min_disp, sub, nbins, maxdisp)
    code_bits = _int_in("code_bits", code_bits, 0, 63)
    if code_bits & 0x33:
        raise ValueError(f"code_bits {code_bits} selects a code other than 2 and 3, whose heights are not positive")
    width = _int_in("width", width, 1, 64)
    top = 2 ** 31 - 1
    min_count = _int_in("min_count", 2 * width if min_count is None else min_count, 1, top)
    min_row = _int_in("min_row", max(1, width // 2) if min_row is None else min_row, 1, top)
    return (min_disp, code_bits, width, sub, nbins, _int_in("tol_bins", tol_bins, 0, 8), min_count, min_row,
            _int_in("max_gap", max_gap, 0, top), _int_in("layers", layers, 1, 4))


def stixels(disp, cameras, codes, height, min_disp=1.0, max_depth=float("inf"), code_bits=1 << 2, width=8, maxdisp=192, sub=4, nbins=None,
            tol_bins=1, min_count=None, min_row=None, max_gap=2, layers=2, udisp=False):
    """The stixel world of disparity maps (include/lwsnet_hip.h, lws_stixels): per strip of `width` columns and per layer, nearest
    first, the obstacle that stands there -- its rows, disparity, depth z, lateral position X and height -- from the u-disparity
    histogram of the strip's pixels whose code's bit is set in code_bits (default: obstacles).  codes, height: what ground_classify
    (or ground) returns for the same maps.  Bins of 1 / sub pixels, nbins None for min(1024, sub * maxdisp) as in vdisparity; a layer is
    the nearest bin whose window of +-tol_bins holds min_count pixels (None: 2 * width); a row belongs to it with min_row members
    (None: max(1, width // 2)), and it ends above the first max_gap + 1 rows without.  Returns a StixelResult."""
    if cameras is None:
        raise ValueError("stixels needs cameras")
    min_disp, code_bits, width, sub, nbins, tol_bins, min_count, min_row, max_gap, layers = _stixel_args(
        min_disp, code_bits, width, maxdisp, sub, nbins, tol_bins, min_count, min_row, max_gap, layers)
    d, _, cam = _geometry_inputs(disp, None, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    if H > 16384 or W > 16384:
        raise ValueError(f"disp is {H}x{W}: stixels takes maps up to 16384x16384")
    codes, height = _ground_codes(codes, d), _height_map(height, d)
    S = -(-W // width)
    rows = torch.empty((B, S, layers, 4), device=d.device, dtype=torch.int32)
    vals = torch.empty((B, S, layers, 4), device=d.device, dtype=torch.float32)
    u = torch.empty((B, S, nbins), device=d.device, dtype=torch.uint32) if udisp else None
    _call("lws_stixels", d.device, d, cam, codes, height, B, H, W, min_disp, float(max_depth), code_bits, width, sub, nbins, tol_bins, min_count,
          min_row, max_gap, layers, rows, vals, u)
    return StixelResult(rows, vals, u)


ObjectResult = namedtuple("ObjectResult", ["rows", "vals", "labels", "info"])
ObjectResult.__doc__ = """What objects returns, all on the device: rows int32 [B,max_objects,8] = {n, x_min, x_max, y_min, y_max, k_min, k_max,
cells}, vals float32 [B,max_objects,8] = {disparity, z, X_min, X_max, Y_min, Y_max, Z_min, Z_max}, labels int32 [B,1,H,W] (the object's
number per pixel, -1 for none; None unless asked for) and info int32 [B,4] = {occupied cells, components, kept components, member
pixels of the kept ones}.  A slot with n = 0 is empty: -1 in the boxes and eight zeros."""


def _object_args(min_disp, code_bits, width, sub, min_count, min_pixels, max_objects):
    """The validated scalar arguments of objects, defaults resolved: min_count None is width."""
    min_disp = _finite_pos("min_disp", min_disp)
    width = _int_in("width", width, 1, 64)
    top = 2 ** 31 - 1
    return (min_disp, _int_in("code_bits", code_bits, 0, 63), width, _int_in("sub", sub, 1, 16),
            _int_in("min_count", width if min_count is None else min_count, 1, top), _int_in("min_pixels", min_pixels, 1, top),
            _int_in("max_objects", max_objects, 1, 65536))


def objects(disp, cameras, codes, udisp, min_disp=1.0, max_depth=float("inf"), code_bits=1 << 2, width=8, sub=4, min_count=None,
            min_pixels=64, max_objects=256, labels=True):
    """The obstacle objects of disparity maps (include/lwsnet_objects.h, lws_objects): the connected components (8-neighbours) of the
    cells of the u-disparity image that hold at least min_count pixels, each pixel mapped back to its cell's component, and per
    component of at least min_pixels pixels -- nearest first -- its pixel box, bins, disparity, depth and box in camera coordinates.
    codes: what ground_classify (or ground) returns for the same maps; udisp: what stixels(udisp=True) returns for them with the same
    min_disp, max_depth, code_bits, width and sub (nbins is udisp.shape[2]).  min_count None means width: a cell counts once it holds
    as many pixels as one row of its strip.  That default and min_pixels = 64 were chosen on synthetic road scenes only; they have
    not met real data.  Returns an ObjectResult."""
    if cameras is None:
        raise ValueError("objects needs cameras")
    min_disp, code_bits, width, sub, min_count, min_pixels, max_objects = _object_args(min_disp, code_bits, width, sub, min_count, min_pixels,
                                                                                      max_objects)
    d, _, cam = _geometry_inputs(disp, None, cameras, min_disp, max_depth)
    B, _, H, W = d.shape
    if H > 16384 or W > 16384:
        raise ValueError(f"disp is {H}x{W}: objects takes maps up to 16384x16384")
    S = -(-W // width)
    if not isinstance(udisp, torch.Tensor) or udisp.dim() != 3:
        raise ValueError("udisp must be a uint32 [B,S,nbins] tensor (what stixels(udisp=True) returns)")
    nbins = _int_in("nbins = udisp.shape[2]", udisp.shape[2], 1, min(4096, 256 * sub))
    if S * nbins > 1 << 22:
        raise ValueError(f"{S} strips x {nbins} bins: objects takes up to 2^22 cells")
    codes = _ground_codes(codes, d)
    udisp = _tensor_of(udisp, "udisp", torch.uint32, (B, S, nbins), d.device, " (what stixels(udisp=True) returns)")
    work = _workspace("lws_objects_workspace", d.device, B, W, width, nbins)
    rows = torch.empty((B, max_objects, 8), device=d.device, dtype=torch.int32)
    vals = torch.empty((B, max_objects, 8), device=d.device, dtype=torch.float32)
    lab = torch.empty(d.shape, device=d.device, dtype=torch.int32) if labels else None
    info = torch.empty((B, 4), device=d.device, dtype=torch.int32)
    _call("lws_objects", d.device, d, cam, codes, udisp, B, H, W, min_disp, float(max_depth), code_bits, width, sub, nbins, min_count,
          min_pixels, max_objects, work, rows, vals, lab, info)
    return ObjectResult(rows, vals, lab, info)


TemporalResult = namedtuple("TemporalResult", ["disp", "var", "age", "code", "counts"])
TemporalResult.__doc__ = """What temporal_step returns: the new state -- disp float32 [B,1,H,W] the fused disparity, var float32 its variance
in px^2, age uint16 the frames fused (0: no state) --, code uint8 [B,1,H,W] (0 nothing, 1 new, 2 fused, 3 reset by the gate, 4 held)
and counts, an int64 [B,5] device tensor of the pixels per code (None unless asked for)."""


def _temporal_args(sigma0, min_disp, sigma_min, gate, q, max_jump, hold, q_hold, max_var):
    """The validated scalar arguments of temporal_step, in the order of the C call."""
    if not (max_jump >= 0):
        raise ValueError(f"max_jump must be >= 0 (inf allowed), got {max_jump}")
    if not (max_var > 0):
        raise ValueError(f"max_var must be > 0 (inf allowed), got {max_var}")
    if isinstance(hold, float) or hold not in (0, 1):
        raise ValueError(f"hold must be False or True, got {hold}")
    return (_finite_nonneg("sigma0", sigma0), _finite_pos("min_disp", min_disp), _finite_pos("sigma_min", sigma_min), _finite_pos("gate", gate),
            _finite_nonneg("q", q), float(max_jump), int(hold), _finite_nonneg("q_hold", q_hold), float(max_var))


def temporal_pose_rows(pose, B):
    """pose as the float32 [B,2,12] rows of lws_temporal_step: one [2][12] (lwsnet_amd.geometry.relative_pose) for every image, or
    B of them."""
    import numpy as np
    p = np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose, np.float32)
    if p.shape == (2, 12):
        p = np.broadcast_to(p, (B, 2, 12))
    if p.shape != (B, 2, 12) or not np.isfinite(p).all():
        raise ValueError(f"pose must be a finite float32 [2,12] or [{B},2,12] (geometry.relative_pose), got shape {p.shape}")
    return np.array(p, np.float32, order="C")              # (a copy: a broadcast view is read-only)


def temporal_step(disp, cameras, pose=None, prev=None, sigma=None, mask=None, sigma0=0.5, min_disp=1.0, sigma_min=0.05, gate=3.0, q=0.0,
                  max_jump=1.0, hold=False, q_hold=0.05, max_var=4.0, counts=True, out=None):
    """One step of the temporal filter on disparity maps (include/lwsnet_temporal.h, lws_temporal_step): the previous state is carried
    into the current left camera with a known pose, gated against the new maps and fused with them; with hold, a pixel without a
    measurement keeps what was seen there before.  disp [B,1,H,W] float32; cameras: one Camera or a list of B; pose: what
    geometry.relative_pose returns, [2,12] or [B,2,12], or the float32 [B,2,12] device tensor egomotion returns; prev: the (disp, var, age) of the previous step's TemporalResult, or None on
    the first frame (pose is then not read); sigma: None (sigma0 px everywhere) or float32 [B,1,H,W] in px; mask: None or the uint8
    lws_lr_check code map (only code-1 pixels are measurements).  The defaults of gate, q, sigma0, sigma_min, max_jump, q_hold and
    max_var were chosen on a synthetic scene only; they have not met real data.  out: None (new tensors) or the four tensors (disp, var, age, code) to write, which may not be
    prev's.  Returns a TemporalResult."""
    if cameras is None:
        raise ValueError("temporal_step needs cameras")
    scalars = _temporal_args(sigma0, min_disp, sigma_min, gate, q, max_jump, hold, q_hold, max_var)
    if prev is not None and (len(prev) != 3 or any(t is None for t in prev)):
        raise ValueError("prev must be the (disp, var, age) of the previous step, or None")
    if prev is not None and pose is None:
        raise ValueError("temporal_step: a previous state needs pose")
    d, mask, cam = _geometry_inputs(disp, mask, cameras, scalars[1], float("inf"))
    B, _, H, W = d.shape
    _int_indexed(H, W, "disp", "temporal_step")
    if sigma is not None:
        sigma = _disp_map(sigma, "sigma")
        if tuple(sigma.shape) != tuple(d.shape) or sigma.device != d.device:
            raise ValueError(f"sigma must be {tuple(d.shape)} on {d.device}")
    pose_dev = None
    if prev is not None:
        prev = (_tensor_of(prev[0], "prev disp", torch.float32, d.shape, d.device), _tensor_of(prev[1], "prev var", torch.float32, d.shape, d.device),
                _tensor_of(prev[2], "prev age", torch.uint16, d.shape, d.device))
        pose_dev = _device_rows(pose, "pose", (B, 2, 12), d.device, lambda: temporal_pose_rows(pose, B))
    else:
        prev = (None, None, None)
    hold = scalars[6]
    work = _workspace("lws_temporal_workspace", d.device, B, H, W, hold) if hold else None
    dts = (torch.float32, torch.float32, torch.uint16, torch.uint8)
    if out is None:
        out = [torch.empty(d.shape, device=d.device, dtype=dt) for dt in dts]
    elif len(out) != 4:
        raise ValueError("out must be four tensors (disp, var, age, code)")
    else:
        out = [_tensor_of(t, f"out[{i}]", dt, d.shape, d.device) for i, (t, dt) in enumerate(zip(out, dts))]
    cnt =torch.empty((B, 5), device=d.device, dtype=torch.int64) if counts else None
    _call("lws_temporal_step", d.device, d, sigma, mask, cam, pose_dev, *prev, B, H, W, *scalars, work, *out, cnt)
    return TemporalResult(*out, cnt)


EgoResult = namedtuple("EgoResult", ["pose", "status", "info", "trace", "resid"])
EgoResult.__doc__ = """What egomotion returns, all on the device: pose float32 [B,2,12], the block temporal_step reads (pose[b][0] maps the
previous camera's frame into the current one, pose[b][1] is its inverse); status int32 [B], a bit set (1 a level had too few pixels,
2 a singular step, 4 a non-finite step, 8 the final linearisation had too few pixels: do not trust the pose, 16 a step below the
pose's float32 resolution was not taken); info float64 [B,4]: pixels used and weighted rms residual at level 0 for the final pose,
|delta| of the last step taken, steps taken; trace float64 [B,levels*iters,48] and resid float32 [B,1,H,W] (None unless asked for)."""
EGO_UNTRUSTED = 8                                           # the status bit that says the pose is not to be trusted


def ego_args(levels, iters, min_disp, max_jump, huber, damping, min_pixels):
    """The validated scalar arguments of egomotion, in the order of the C call (lwsnet_amd.egomotion.Odometry checks its own with it)."""
    if not (max_jump >= 0):
        raise ValueError(f"max_jump must be >= 0 (inf allowed), got {max_jump}")
    return (_int_in("levels", levels, 1, 8), _int_in("iters", iters, 1, 64), _finite_pos("min_disp", min_disp), float(max_jump),
            _finite_pos("huber", huber), _finite_nonneg("damping", damping), _int_in("min_pixels", min_pixels, 1, (1 << 31) - 1))


def _motion_rows(M, B, name, dt):
    """M as [B,12] rows of numpy dtype dt: one row-major 3 x 4 [R|t] (12 numbers or 3 x 4) for every image, or B of them."""
    import numpy as np
    m = np.asarray(M.detach().cpu().numpy() if isinstance(M, torch.Tensor) else M, np.float64)
    if m.shape in ((12,), (3, 4)):
        m = np.broadcast_to(m.reshape(1, 12), (B, 12))
    elif m.shape == (B, 3, 4):
        m = m.reshape(B, 12)
    if m.shape != (B, 12) or not np.isfinite(m).all():
        raise ValueError(f"{name} must be a finite [12] or [{B},12] (row-major 3x4 [R|t]), got shape {m.shape}")
    return np.array(m, dt, order="C")


def ego_normal(grey_ref, disp_ref, grey_cur, cameras, M, level=0, mask=None, min_disp=1.0, huber=10.0, terms=False):
    """One linearisation of the photometric error at one pyramid level (include/lwsnet_egomotion.h, lws_ego_normal).  grey_ref,
    disp_ref, grey_cur float32 [B,1,H,W], the images of this level (disp_ref in full-resolution pixels); cameras: the full-resolution
    Camera or a list of B; M: the motion to linearise at, [12] or [B,12] (float64); level 0..7 scales the camera; mask: None or the
    uint8 lws_lr_check code map.  Returns (sums float64 [B,29], terms float32 [B,H,W,8] or None)."""
    if cameras is None:
        raise ValueError("ego_normal needs cameras")
    level = _int_in("level", level, 0, 7)
    huber = _finite_pos("huber", huber)
    d, mask, cam = _geometry_inputs(disp_ref, mask, cameras, min_disp, float("inf"))
    B, _, H, W = d.shape
    _int_indexed(H, W, "disp_ref", "ego_normal")
    g0, g1 = (_tensor_of(g, name, torch.float32, d.shape, d.device) for g, name in ((grey_ref, "grey_ref"), (grey_cur, "grey_cur")))
    m_dev = torch.from_numpy(_motion_rows(M, B, "M", "float64")).to(d.device)
    work = _workspace("lws_egomotion_workspace", d.device, B, H, W, 1)
    sums = torch.empty((B, 29), device=d.device, dtype=torch.float64)
    tm = torch.empty((B, H, W, 8), device=d.device, dtype=torch.float32) if terms else None
    _call("lws_ego_normal", d.device, g0, d, mask, g1, cam, m_dev, B, H, W, level, float(min_disp), huber, work, sums, tm)
    return sums, tm


def egomotion(rgb_ref, disp_ref, rgb_cur, cameras, mask=None, init=None, levels=4, iters=8, min_disp=1.0, max_jump=1.0, huber=10.0,
              damping=0.0, min_pixels=256, trace=False, resid=False):
    """The motion of the camera between two frames by dense direct alignment (include/lwsnet_egomotion.h, lws_egomotion): the pixels
    of the previous left image, with their disparity, are warped into the current one and the intensity difference is minimised over
    the six motion parameters, coarse to fine.  rgb_ref, rgb_cur uint8 [B,H,W,3], the previous and the current left image; disp_ref
    float32 [B,1,H,W] and mask (None or the uint8 lws_lr_check code map) the previous frame's disparity; cameras: one Camera or a
    list of B; init: None (the identity), a float32 [B,12] device tensor (such as pose[:, 0] of the previous estimate) or [12] /
    [B,12] host numbers.  The defaults of levels, iters, huber, max_jump and min_pixels were chosen on a synthetic scene only; they
    have not met real data.  Returns an EgoResult; nothing is read back, and its pose is what temporal_step takes as `pose`."""
    if cameras is None:
        raise ValueError("egomotion needs cameras")
    scalars = ego_args(levels, iters, min_disp, max_jump, huber, damping, min_pixels)
    d, mask, cam = _geometry_inputs(disp_ref, mask, cameras, scalars[2], float("inf"))
    B, _, H, W = d.shape
    _int_indexed(H, W, "disp_ref", "egomotion")
    r0, r1 = (_tensor_of(r, name, torch.uint8, (B, H, W, 3), d.device) for r, name in ((rgb_ref, "rgb_ref"), (rgb_cur, "rgb_cur")))
    if init is not None:
        init = _device_rows(init, "init", (B, 12), d.device, lambda: _motion_rows(init, B, "init", "float32"))
    levels, iters = scalars[:2]
    work = _workspace("lws_egomotion_workspace", d.device, B, H, W, levels)
    pose = torch.empty((B, 2, 12), device=d.device, dtype=torch.float32)
    status = torch.empty((B,), device=d.device, dtype=torch.int32)
    info = torch.empty((B, 4), device=d.device, dtype=torch.float64)
    tr = torch.empty((B, levels * iters, 48), device=d.device, dtype=torch.float64) if trace else None
    rs = torch.empty(d.shape, device=d.device, dtype=torch.float32) if resid else None
    _call("lws_egomotion", d.device, r0, d, mask, r1, cam, init, B, H, W, *scalars, work, pose, status, info, tr, rs)
    return EgoResult(pose, status, info, tr, rs)


TrackResult = namedtuple("TrackResult", ["pose", "status", "info", "trace", "resid", "sums", "terms"])
TrackResult.__doc__ = """What track and track_normal return, all on the device.  track: pose float32 [B,2,12] as egomotion's; status int32
[B], egomotion's bits (8: do not trust the pose) and 32: the final linearisation had fewer than min_pixels geometric terms, the model
did not constrain the pose; info float64 [B,6]: n_p, photometric rms (grey levels), n_g, geometric rms (standard deviations), |delta| of
the last step taken, steps taken; trace float64 [B,iters,51] and resid float32 [B,2,H,W] (None unless asked for); sums, terms None.
track_normal: sums float64 [B,32] and terms float32 [B,H,W,16] (None unless asked for); the rest None."""
TRACK_UNTRUSTED, TRACK_NO_MODEL = 8, 32


def track_args(min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g):
    """The validated scalars of track_normal, in the order of the C call."""
    huber_g = _finite_pos("huber_g", huber_g)
    if not (gate_g >= huber_g):
        raise ValueError(f"gate_g must be >= huber_g (inf allowed), got {gate_g} < {huber_g}")
    return (_finite_pos("min_disp", min_disp), _finite_pos("huber_p", huber_p), _finite_pos("sigma_p", sigma_p), huber_g, float(gate_g),
            _finite_nonneg("sigma0", sigma0), _finite_pos("sigma_min", sigma_min), _finite_nonneg("lambda_g", lambda_g))


def _track_maps(who, disp_ref, normals_ref, mask_ref, disp_cur, sigma_cur, mask_cur, cameras, min_disp):
    """The model maps and the current maps of track / track_normal, checked: (disp_ref, normals, mask_ref, disp_cur, sigma, mask_cur, cam)."""
    if cameras is None:
        raise ValueError(f"{who} needs cameras")
    d, mask_ref, cam = _geometry_inputs(disp_ref, mask_ref, cameras, min_disp, float("inf"))
    B, _, H, W = d.shape
    _int_indexed(H, W, "disp_ref", who, sides=True)
    dc = _tensor_of(disp_cur, "disp_cur", torch.float32, d.shape, d.device)
    if normals_ref is not None:
        normals_ref = _tensor_of(normals_ref, "normals_ref", torch.float32, (B, 3, H, W), d.device, " (what tsdf_raycast returns)")
    if sigma_cur is not None:
        sigma_cur = _tensor_of(sigma_cur, "sigma_cur", torch.float32, d.shape, d.device)
    if mask_cur is not None:
        mask_cur = _tensor_of(mask_cur, "mask_cur", torch.uint8, d.shape, d.device, " (the lws_lr_check code map)")
    return d, normals_ref, mask_ref, dc, sigma_cur, mask_cur, cam


def track_normal(grey_ref, disp_ref, grey_cur, disp_cur, cameras, M, normals_ref=None, mask_ref=None, sigma_cur=None, mask_cur=None,
                 min_disp=1.0, huber_p=10.0, sigma_p=4.0, huber_g=1.5, gate_g=4.0, sigma0=0.5, sigma_min=0.05, lambda_g=1.0, terms=False):
    """One linearisation of the joint photometric + point-to-plane cost (include/lwsnet_track.h, lws_track_normal).  grey_ref,
    grey_cur, disp_ref (the model's view), disp_cur float32 [B,1,H,W]; normals_ref float32 [B,3,H,W] or None; the masks uint8 or
    None; sigma_cur float32 [B,1,H,W] or None; M [12] or [B,12] (float64).  Returns a TrackResult with sums and terms."""
    scalars = track_args(min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g)
    d, nr, mr, dc, sc, mc, cam = _track_maps("track_normal", disp_ref, normals_ref, mask_ref, disp_cur, sigma_cur, mask_cur, cameras, scalars[0])
    B, _, H, W = d.shape
    g0, g1 = (_tensor_of(g, name, torch.float32, d.shape, d.device) for g, name in ((grey_ref, "grey_ref"), (grey_cur, "grey_cur")))
    m_dev = torch.from_numpy(_motion_rows(M, B, "M", "float64")).to(d.device)
    work = _workspace("lws_track_workspace", d.device, B, H, W)
    sums = torch.empty((B, 32), device=d.device, dtype=torch.float64)
    tm = torch.empty((B, H, W, 16), device=d.device, dtype=torch.float32) if terms else None
    _call("lws_track_normal", d.device, g0, d, nr, mr, g1, dc, sc, mc, cam, m_dev, B, H, W, *scalars, work, sums, tm)
    return TrackResult(None, None, None, None, None, sums, tm)


def track(rgb_ref, disp_ref, rgb_cur, disp_cur, cameras, normals_ref=None, mask_ref=None, sigma_cur=None, mask_cur=None, init=None, iters=6,
          min_disp=1.0, huber_p=10.0, sigma_p=4.0, huber_g=1.5, gate_g=4.0, sigma0=0.5, sigma_min=0.05, lambda_g=1.0, damping=0.0,
          min_pixels=256, trace=False, resid=False):
    """The motion of the camera from a reference view of the TSDF model to the current frame (include/lwsnet_track.h, lws_track):
    `iters` Gauss-Newton steps on the joint photometric + point-to-plane cost at full resolution.  rgb_ref, rgb_cur uint8 [B,H,W,3];
    disp_ref, normals_ref, mask_ref: the model's view in the reference camera (what tsdf_raycast returns); disp_cur, sigma_cur,
    mask_cur: the current frame's own maps; init as egomotion takes it (the frame-to-frame estimate).  The defaults were chosen on a
    synthetic scene only; they have not met real data.  Returns a TrackResult; nothing is read back."""
    scalars = track_args(min_disp, huber_p, sigma_p, huber_g, gate_g, sigma0, sigma_min, lambda_g)
    iters = _int_in("iters", iters, 1, 64)
    damping = _finite_nonneg("damping", damping)
    min_pixels = _int_in("min_pixels", min_pixels, 1, (1 << 31) - 1)
    d, nr, mr, dc, sc, mc, cam = _track_maps("track", disp_ref, normals_ref, mask_ref, disp_cur, sigma_cur, mask_cur, cameras, scalars[0])
    B, _, H, W = d.shape
    r0, r1 = (_tensor_of(r, name, torch.uint8, (B, H, W, 3), d.device) for r, name in ((rgb_ref, "rgb_ref"), (rgb_cur, "rgb_cur")))
    if init is not None:
        init = _device_rows(init, "init", (B, 12), d.device, lambda: _motion_rows(init, B, "init", "float32"))
    work = _workspace("lws_track_workspace", d.device, B, H, W)
    pose = torch.empty((B, 2, 12), device=d.device, dtype=torch.float32)
    status = torch.empty((B,), device=d.device, dtype=torch.int32)
    info = torch.empty((B, 6), device=d.device, dtype=torch.float64)
    tr = torch.empty((B, iters, 51), device=d.device, dtype=torch.float64) if trace else None
    rs = torch.empty((B, 2, H, W), device=d.device, dtype=torch.float32) if resid else None
    _call("lws_track", d.device, r0, d, nr, mr, r1, dc, sc, mc, cam, init, B, H, W, iters, *scalars, damping, min_pixels, work, pose, status, info,
          tr, rs)
    return TrackResult(pose, status, info, tr, rs, None, None)


TSDF_WEIGHTS = {"unit": 0, "sigma": 1}                      # wmode of lws_tsdf_integrate


def tsdf_volume_args(origin, voxel, dims):
    """The validated (Gx, Gy, Gz, ox, oy, oz, vs) of a volume, in the order of the C calls: origin three finite numbers (the centre
    of voxel (0, 0, 0)), voxel finite and > 0, dims = (Gx, Gy, Gz), each in 2 .. 4096 with a product below 2^31."""
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"origin must be three finite numbers, got {origin}")
    if len(dims) != 3:
        raise ValueError(f"dims must be (Gx, Gy, Gz), got {dims}")
    g = [_int_in(f"dims[{i}]", v, 2, 4096) for i, v in enumerate(dims)]
    if g[0] * g[1] * g[2] >= 1 << 31:
        raise ValueError(f"dims {tuple(g)}: a volume holds fewer than 2^31 voxels")
    return (*g, *(float(v) for v in origin), _finite_pos("voxel", voxel))


def tsdf_pose_rows(poses_c2w, B):
    """Camera-to-world poses, float64 [3,4] (one for every image) or [B,3,4] -> the float32 [B,2,12] rows of lws_tsdf_integrate and
    lws_tsdf_raycast: world -> camera, the inverse taken in float64 as geometry.relative_pose takes it, and camera -> world."""
    import numpy as np
    p = np.asarray(poses_c2w, np.float64)
    if p.shape == (3, 4):
        p = np.broadcast_to(p, (B, 3, 4))
    if p.shape != (B, 3, 4) or not np.isfinite(p).all():
        raise ValueError(f"poses must be finite camera-to-world [3,4] or [{B},3,4] float64 [R|t], got shape {p.shape}")
    m = np.concatenate([p, np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (B, 1, 4))], axis=1)
    inv = np.stack([np.linalg.solve(m[b], np.eye(4)) for b in range(B)])
    return np.stack([inv[:, :3].reshape(B, 12), m[:, :3].reshape(B, 12)], axis=1).astype(np.float32)


def _tsdf_pose(pose, B, device):
    def host_rows():
        import numpy as np
        p = np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose)
        if p.dtype != np.float32 or p.shape != (B, 2, 12) or not np.isfinite(p).all():
            raise ValueError(f"pose must be the finite float32 [{B},2,12] of tsdf_pose_rows, got {p.dtype} {p.shape}")
        return np.ascontiguousarray(p)
    return _device_rows(pose, "pose", (B, 2, 12), device, host_rows)


def _tsdf_volume(T, Wt, C, g):
    """The tensors of a volume of g = (Gx, Gy, Gz): T, Wt float32 [Gz,Gy,Gx], C None or uint8 [Gz,Gy,Gx,4], contiguous on one HIP
    device (the calls write them in place, so nothing is copied)."""
    shape = (g[2], g[1], g[0])
    for name, t, dt, sh in (("T", T, torch.float32, shape), ("Wt", Wt, torch.float32, shape), ("C", C, torch.uint8, (*shape, 4))):
        if t is None and name == "C":
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} must be a torch tensor on a HIP device (the volume has no CPU fallback)")
        if t.dtype != dt or tuple(t.shape) != sh or not t.is_contiguous() or t.device != T.device:
            raise ValueError(f"{name} must be a contiguous {str(dt).split('.')[-1]} {sh} tensor on {T.device}")
    return T.device


def _tsdf_integrate_args(sigma0, min_disp, max_depth, mu0, mu_d, sigma_min, weight, w_max):
    """The validated scalar arguments of tsdf_integrate, in the order of the C call."""
    if not (max_depth > 0):
        raise ValueError(f"max_depth must be > 0 (inf allowed), got {max_depth}")
    if not (w_max > 0):
        raise ValueError(f"w_max must be > 0 (inf allowed), got {w_max}")
    if weight not in TSDF_WEIGHTS:
        raise ValueError(f"weight must be one of {sorted(TSDF_WEIGHTS)}, got {weight!r}")
    return (_finite_nonneg("sigma0", sigma0), _finite_pos("min_disp", min_disp), float(max_depth), _finite_pos("mu0", mu0), _finite_nonneg("mu_d", mu_d),
            _finite_pos("sigma_min", sigma_min), TSDF_WEIGHTS[weight], float(w_max))


def tsdf_integrate(T, Wt, origin, voxel, disp, cameras, pose, C=None, sigma=None, mask=None, normals=None, rgb=None, sigma0=0.5, min_disp=1.0,
                   max_depth=float("inf"), mu0=0.25, mu_d=0.0, sigma_min=0.05, weight="unit", w_max=float("inf"), updated=True):
    """Integrates B frames into a TSDF volume, in place (include/lwsnet_tsdf.h, lws_tsdf_integrate).  T, Wt float32 [Gz,Gy,Gx] and
    C uint8 [Gz,Gy,Gx,4] or None: the volume, whose voxel (0, 0, 0) has its centre at `origin` and whose voxels are `voxel` metres
    wide; disp [B,1,H,W] float32; cameras: one Camera or a list of B; pose: tsdf_pose_rows(camera-to-world poses, B), or that block
    as a float32 [B,2,12] device tensor; sigma: None (sigma0 px everywhere) or float32 [B,1,H,W]; mask: None or the uint8
    lws_lr_check code map; normals: None (the distance along the ray) or the float32 [B,3,H,W] of surface_normals (the distance to
    the pixel's tangent plane); rgb: the uint8 [B,H,W,3] images, required iff C is given.  Returns the voxels taken per frame, an
    int64 [B] device tensor (None unless asked for)."""
    if cameras is None:
        raise ValueError("tsdf_integrate needs cameras")
    g = tsdf_volume_args(origin, voxel, T.shape[::-1] if isinstance(T, torch.Tensor) and T.dim() == 3 else ())
    scalars = _tsdf_integrate_args(sigma0, min_disp, max_depth, mu0, mu_d, sigma_min, weight, w_max)
    dev = _tsdf_volume(T, Wt, C, g)
    if (C is None) != (rgb is None):
        raise ValueError("tsdf_integrate: rgb and C go together (a volume with colour needs the images, one without takes none)")
    d, mask, cam = _geometry_inputs(disp, mask, cameras, scalars[1], scalars[2])
    if d.device != dev:
        raise ValueError(f"disp is on {d.device}, the volume on {dev}")
    B, _, H, W = d.shape
    _int_indexed(H, W, "disp", "tsdf_integrate", sides=True)
    if sigma is not None:
        sigma = _tensor_of(sigma, "sigma", torch.float32, d.shape, dev)
    if normals is not None:
        normals = _tensor_of(normals, "normals", torch.float32, (B, 3, H, W), dev, " (what surface_normals returns)")
    if rgb is not None:
        rgb = _guide(rgb, d)
    pose = _tsdf_pose(pose, B, dev)
    upd = torch.empty((B,), device=dev, dtype=torch.int64) if updated else None
    _call("lws_tsdf_integrate", dev, d, sigma, mask, normals, rgb, cam, pose, B, H, W, T, Wt, C, *g, *scalars, upd)
    return upd


TsdfView = namedtuple("TsdfView", ["disp", "weight", "normals"])
TsdfView.__doc__ = """What tsdf_raycast returns: disp float32 [B,1,H,W], the disparity of the surface the pixel's ray meets, 0 where it
meets none; weight float32 [B,1,H,W], the volume's weight there; normals float32 [B,3,H,W] in the camera's frame, the convention of
surface_normals (weight and normals: None unless asked for)."""


def _tsdf_w_min(w_min):
    return _finite_nonneg("w_min", w_min)


def tsdf_raycast(T, Wt, origin, voxel, cameras, pose, H, W, z_near=0.5, step=None, nsteps=None, z_far=None, w_min=0.0, weight=True, normals=True):
    """Casts B views of H x W from a TSDF volume (include/lwsnet_tsdf.h, lws_tsdf_raycast).  cameras: one Camera or a list of B
    (B = 1 for one Camera and one pose); pose as tsdf_integrate takes it; the rays are sampled at the camera depths
    z_near + k * step, k < nsteps.  step defaults to half a voxel; nsteps to what reaches z_far, and z_far to z_near plus the volume's
    diagonal, which no ray that starts inside the volume outruns.  Returns a TsdfView."""
    import numpy as np
    from .geometry import Camera, camera_rows
    g = tsdf_volume_args(origin, voxel, T.shape[::-1] if isinstance(T, torch.Tensor) and T.dim() == 3 else ())
    dev = _tsdf_volume(T, Wt, None, g)
    if cameras is None:
        raise ValueError("tsdf_raycast needs cameras")
    if isinstance(pose, torch.Tensor) or (isinstance(pose, np.ndarray) and pose.ndim == 3):
        B = int(pose.shape[0])
    else:
        raise ValueError("pose must be the float32 [B,2,12] of tsdf_pose_rows")
    if not isinstance(cameras, Camera) and len(cameras) != B:
        raise ValueError(f"cameras must be one Camera or a list of {B}")
    B = _int_in("B", B, 1, 65535)
    H, W = _int_in("H", H, 1, 1 << 24), _int_in("W", W, 1, 1 << 24)
    _int_indexed(H, W, "", "tsdf_raycast", what="views")
    z_near = _finite_pos("z_near", z_near)
    step = _finite_pos("step", 0.5 * g[6] if step is None else step)
    if nsteps is None:
        far = z_near + g[6] * math.sqrt(sum((n - 1) ** 2 for n in g[:3])) if z_far is None else _finite_pos("z_far", z_far)
        nsteps = min(max(int(math.ceil((far - z_near) / step)) + 1, 2), 65535)
    nsteps = _int_in("nsteps", nsteps, 2, 65535)
    w_min = _tsdf_w_min(w_min)
    cam = torch.from_numpy(camera_rows(cameras, B)).to(dev)
    pose = _tsdf_pose(pose, B, dev)
    d = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32)
    wt = torch.empty((B, 1, H, W), device=dev, dtype=torch.float32) if weight else None
    n = torch.empty((B, 3, H, W), device=dev, dtype=torch.float32) if normals else None
    _call("lws_tsdf_raycast", dev, T, Wt, *g, cam, pose, B, H, W, z_near, step, nsteps, w_min, d, wt, n)
    return TsdfView(d, wt, n)


TsdfPoints = namedtuple("TsdfPoints", ["points", "vnormals", "counts"])
TsdfPoints.__doc__ = """What tsdf_points returns: points uint8 [max_points,16], the records of point_cloud (geometry.POINT_DTYPE) in world
coordinates; vnormals float32 [max_points,4] {n.x, n.y, n.z, 0} (None unless asked for); counts, an int64 [1] device tensor: the
crossings found, of which the first min(counts, max_points) records are written and the rest is unwritten."""


def tsdf_points(T, Wt, origin, voxel, max_points, C=None, w_min=0.0, with_normals=True):
    """The zero crossings of a TSDF volume on the edges of its voxel grid as oriented, coloured points in a fixed order
    (include/lwsnet_tsdf.h, lws_tsdf_points).  max_points: the capacity in records.  Returns a TsdfPoints."""
    g = tsdf_volume_args(origin, voxel, T.shape[::-1] if isinstance(T, torch.Tensor) and T.dim() == 3 else ())
    max_points = _int_in("max_points", max_points, 1, (1 << 31) - 1)
    w_min = _tsdf_w_min(w_min)
    dev = _tsdf_volume(T, Wt, C, g)
    work = _workspace("lws_tsdf_points_workspace", dev, g[1], g[2])
    points = torch.empty((max_points, 16), device=dev, dtype=torch.uint8)
    vn = torch.empty((max_points, 4), device=dev, dtype=torch.float32) if with_normals else None
    counts = torch.empty((1,), device=dev, dtype=torch.int64)
    _call("lws_tsdf_points", dev, T, Wt, C, *g, w_min, ctypes.c_int64(max_points), work, points, vn, counts)
    return TsdfPoints(points, vn, counts)


TsdfMesh = namedtuple("TsdfMesh", ["points", "vnormals", "faces", "counts"])
TsdfMesh.__doc__ = """What tsdf_mesh returns: points uint8 [max_points,16] and vnormals float32 [max_points,4] (None unless asked for), the
records and normals of tsdf_points; faces int32 [max_faces,3], indices into the records; counts, an int64 [2] device tensor: the
vertices and the faces found.  The first min(counts[0], max_points) records are written, and the first min(counts[1], max_faces)
faces unless counts[0] > max_points, which leaves every face unwritten."""


def tsdf_mesh(T, Wt, origin, voxel, max_points, max_faces, C=None, w_min=0.0, with_normals=True):
    """The zero level set of a TSDF volume as an indexed triangle mesh: marching cubes whose vertices are the records of tsdf_points
    in their order (include/lwsnet_tsdf_mesh.h, lws_tsdf_mesh).  max_points, max_faces: the capacities.  Returns a TsdfMesh."""
    g = tsdf_volume_args(origin, voxel, T.shape[::-1] if isinstance(T, torch.Tensor) and T.dim() == 3 else ())
    max_points = _int_in("max_points", max_points, 1, (1 << 31) - 1)
    max_faces = _int_in("max_faces", max_faces, 1, (1 << 31) - 1)
    w_min = _tsdf_w_min(w_min)
    dev = _tsdf_volume(T, Wt, C, g)
    work = _workspace("lws_tsdf_mesh_workspace", dev, g[1], g[2])
    points = torch.empty((max_points, 16), device=dev, dtype=torch.uint8)
    vn = torch.empty((max_points, 4), device=dev, dtype=torch.float32) if with_normals else None
    faces = torch.empty((max_faces, 3), device=dev, dtype=torch.int32)
    counts = torch.empty((2,), device=dev, dtype=torch.int64)
    _call("lws_tsdf_mesh", dev, T, Wt, C, *g, w_min, ctypes.c_int64(max_points), ctypes.c_int64(max_faces), work, points, vn, faces, counts)
    return TsdfMesh(points, vn, faces, counts)


TsdfWindow = namedtuple("TsdfWindow", ["T", "Wt", "C", "counts"])
TsdfWindow.__doc__ = """What tsdf_window returns: the second volume T, Wt float32 [Dz,Dy,Dx] and C uint8 [Dz,Dy,Dx,4] (None without colour), every
element written; counts, an int64 [2] device tensor {live, not live} voxels (None unless asked for)."""
TSDF_MAX_SHIFT = 4096                                       # |offset| per axis of lws_tsdf_window


def tsdf_window_args(dims, offset, out_dims=None):
    """The validated (Gx, Gy, Gz, sx, sy, sz, Dx, Dy, Dz) of tsdf_window: dims and out_dims (default: dims) each in 2 .. 4096 with a
    product below 2^31, offset three integers in -4096 .. 4096."""
    def volume(name, d):
        if len(d) != 3:
            raise ValueError(f"{name} must be (Gx, Gy, Gz), got {tuple(d)}")
        g = [_int_in(f"{name}[{i}]", v, 2, 4096) for i, v in enumerate(d)]
        if g[0] * g[1] * g[2] >= 1 << 31:
            raise ValueError(f"{name} {tuple(g)}: a volume holds fewer than 2^31 voxels")
        return g
    if len(offset) != 3:
        raise ValueError(f"offset must be (sx, sy, sz), got {tuple(offset)}")
    g = volume("dims", dims)
    s = [_int_in(f"offset[{i}]", v, -TSDF_MAX_SHIFT, TSDF_MAX_SHIFT) for i, v in enumerate(offset)]
    return (*g, *s, *(g if out_dims is None else volume("out_dims", out_dims)))


def tsdf_window(T, Wt, offset, dims=None, C=None, out=None, counts=True):
    """A TSDF volume seen through an integer offset, written to a second volume (include/lwsnet_tsdf_window.h, lws_tsdf_window):
    voxel (ix, iy, iz) of the result is voxel (ix, iy, iz) + offset of T, Wt, C where that lies inside them and is observed, and
    cleared (T = Wt = 0, C = 0) elsewhere.  dims = (Dx, Dy, Dz): the result's, default the source's.  out: (T2, Wt2, C2) to write into
    (C2 None iff C is), which must not share memory with the source; default: new tensors.  Returns a TsdfWindow."""
    a = tsdf_window_args(T.shape[::-1] if isinstance(T, torch.Tensor) and T.dim() == 3 else (), offset, dims)
    dev = _tsdf_volume(T, Wt, C, a[:3])
    shape = (a[8], a[7], a[6])
    if out is None:
        out = (torch.empty(shape, device=dev, dtype=torch.float32), torch.empty(shape, device=dev, dtype=torch.float32),
               None if C is None else torch.empty((*shape, 4), device=dev, dtype=torch.uint8))
    if len(out) != 3 or (out[2] is None) != (C is None):
        raise ValueError("out must be (T2, Wt2, C2), C2 given iff C is")
    T2, Wt2, C2 = out
    if _tsdf_volume(T2, Wt2, C2, a[6:]) != dev:
        raise ValueError(f"out is on {T2.device}, the volume on {dev}")
    n = torch.empty((2,), device=dev, dtype=torch.int64) if counts else None
    _call("lws_tsdf_window", dev, T, Wt, C, *a[:6], T2, Wt2, C2, *a[6:], n)
    return TsdfWindow(T2, Wt2, C2, n)


MoversResult = namedtuple("MoversResult", ["evidence", "mask", "labels", "rows", "vals", "info"])
MoversResult.__doc__ = """What movers returns, all on the device and in the current frame: evidence uint8 [B,1,H,W] (MOVER_EVIDENCE: 0 untested,
1 static, 2 appeared, 3 uncovered, 4 changed); mask uint8 [B,1,H,W], the current code map with MOVER_CODE = 4 on every mover and
`grow` pixels around it; labels int32 [B,1,H,W] (None unless asked for), the mover's number or -1; rows int32 [B,max_movers,8] =
{n, x_min, x_max, y_min, y_max, n2, n3, n4}; vals float32 [B,max_movers,2] = {disparity, depth}; info int32 [B,8] = {tested, static,
appeared, uncovered, changed pixels, components, movers before the cap, pixels of code 4 in mask}."""
MOVER_EVIDENCE = ("untested", "static", "appeared", "uncovered", "changed")
MOVER_CODE = 4                                              # the code of a mover's pixel in MoversResult.mask
MOVER_CANDIDATES = 1 << 2 | 1 << 4                          # cand_bits: appeared and changed; 1 << 3 adds the uncovered pixels
MOVERS_DEFAULTS = dict(min_disp=1.0, sigma0=0.5, sigma_min=0.05, gate_g=3.0, gate_p=25.0, radius=0, cand_bits=MOVER_CANDIDATES, max_diff=1.0,
                       min_pixels=64, grow=2, max_movers=64)           # the scalars of movers, in the order of movers_args


def movers_args(min_disp, sigma0, sigma_min, gate_g, gate_p, radius, cand_bits, max_diff, min_pixels, grow, max_movers):
    """The validated scalars of movers, in the order of the C call."""
    if not gate_p > 0:
        raise ValueError(f"gate_p must be > 0 (inf: no photometric test), got {gate_p}")
    cand_bits = _int_in("cand_bits", cand_bits, 0, 31)
    if cand_bits & 3:
        raise ValueError(f"cand_bits must leave bits 0 and 1 clear (untested and static pixels are no candidates), got {cand_bits}")
    if not max_diff >= 0:
        raise ValueError(f"max_diff must be >= 0 (inf allowed), got {max_diff}")
    return (_finite_pos("min_disp", min_disp), _finite_nonneg("sigma0", sigma0), _finite_pos("sigma_min", sigma_min), _finite_pos("gate_g", gate_g),
            float(gate_p), _int_in("radius", radius, 0, 2), cand_bits, float(max_diff), _int_in("min_pixels", min_pixels, 1, 2 ** 31 - 1),
            _int_in("grow", grow, 0, 8), _int_in("max_movers", max_movers, 1, 65536))


def movers(rgb_prev, disp_prev, rgb_cur, disp_cur, cameras, pose, sigma_prev=None, mask_prev=None, sigma_cur=None, mask_cur=None, min_disp=1.0,
           sigma0=0.5, sigma_min=0.05, gate_g=3.0, gate_p=25.0, radius=0, cand_bits=MOVER_CANDIDATES, max_diff=1.0, min_pixels=64, grow=2,
           max_movers=64, labels=True, mask_out=None):
    """The moving objects between two consecutive frames (include/lwsnet_movers.h, lws_movers): per pixel of the current frame the
    evidence against a rigid scene under the camera motion `pose`, the connected components of the candidate pixels, and per
    component of at least min_pixels pixels -- a mover -- its box, disparity and depth.  rgb uint8 [B,H,W,3]; disp float32 [B,1,H,W];
    sigmas float32 [B,1,H,W] in px or None (sigma0 everywhere); masks uint8 lws_lr_check code maps or None; pose: the float32
    [B,2,12] device tensor egomotion or track returns, or what geometry.relative_pose returns.  mask_out: None (a new tensor) or the
    tensor to write, which may be mask_cur itself.  The defaults were chosen on synthetic scenes only; they have not met real data.
    Returns a MoversResult; nothing is read back."""
    scalars = movers_args(min_disp, sigma0, sigma_min, gate_g, gate_p, radius, cand_bits, max_diff, min_pixels, grow, max_movers)
    if cameras is None:
        raise ValueError("movers needs cameras")
    if pose is None:
        raise ValueError("movers needs pose, the motion between the two frames")
    d, mask_cur, cam = _geometry_inputs(disp_cur, mask_cur, cameras, scalars[0], float("inf"))
    B, _, H, W = d.shape
    _int_indexed(H, W, "disp_cur", "movers", sides=True)
    dp = _tensor_of(disp_prev, "disp_prev", torch.float32, d.shape, d.device)
    r0, r1 = (_tensor_of(r, name, torch.uint8, (B, H, W, 3), d.device) for r, name in ((rgb_prev, "rgb_prev"), (rgb_cur, "rgb_cur")))
    sp, sc = (None if s is None else _tensor_of(s, name, torch.float32, d.shape, d.device) for s, name in ((sigma_prev, "sigma_prev"), (sigma_cur, "sigma_cur")))
    if mask_prev is not None:
        mask_prev = _tensor_of(mask_prev, "mask_prev", torch.uint8, d.shape, d.device, " (the lws_lr_check code map)")
    pose_dev = _device_rows(pose, "pose", (B, 2, 12), d.device, lambda: temporal_pose_rows(pose, B))
    max_movers = scalars[-1]
    work = _workspace("lws_movers_workspace", d.device, B, H, W, max_movers)
    evidence = torch.empty(d.shape, device=d.device, dtype=torch.uint8)
    if mask_out is None:
        mask_out = torch.empty(d.shape, device=d.device, dtype=torch.uint8)
    elif not (isinstance(mask_out, torch.Tensor) and mask_out.dtype == torch.uint8 and tuple(mask_out.shape) == tuple(d.shape)
              and mask_out.device == d.device and mask_out.is_contiguous()):
        raise ValueError(f"mask_out must be a contiguous uint8 {tuple(d.shape)} tensor on {d.device}")
    lab = torch.empty(d.shape, device=d.device, dtype=torch.int32) if labels else None
    rows = torch.empty((B, max_movers, 8), device=d.device, dtype=torch.int32)
    vals = torch.empty((B, max_movers, 2), device=d.device, dtype=torch.float32)
    info = torch.empty((B, 8), device=d.device, dtype=torch.int32)
    _call("lws_movers", d.device, r0, dp, sp, mask_prev, r1, d, sc, mask_cur, cam, pose_dev, B, H, W, *scalars, work, evidence, mask_out, lab,
          rows, vals, info)
    return MoversResult(evidence, mask_out, lab, rows, vals, info)


SpeckleResult = namedtuple("SpeckleResult", ["disp", "mask", "labels", "counts"])
SpeckleResult.__doc__ = """What speckle_filter returns: the filtered (filled if asked) maps float32 [B,1,H,W], the uint8 code map (1 kept,
3 speckle, the input code or 0 for an invalid pixel), labels int32 [B,1,H,W] (None unless want_labels) and counts, an int64
[B,3] device tensor {valid pixels, kept pixels, removed components}."""


def speckle_filter(disp, max_size, max_diff=1.0, mask=None, fill=False, want_labels=False):
    """Removes the connected blobs of at most `max_size` pixels from disparity maps (include/lwsnet_hip.h, lws_speckle_filter:
    4-neighbours are joined iff their float32 disparities differ by <= max_diff).  disp [B,1,H,W] float32 (four stage maps:
    torch.cat them along B, every image is filtered on its own); mask: None or the uint8 lws_lr_check code map (only code-1
    pixels are valid); fill: give the removed and invalid pixels the background value of their row.  The workspace (8 bytes per
    pixel) and the outputs are allocated per call on the current stream.  Returns a SpeckleResult."""
    d = _disp_map(disp, "disp")
    mask = _code_map(mask, d)
    max_diff = _finite_nonneg("max_diff", max_diff)
    max_size = _int_in("max_size", max_size, 0, 2 ** 31 - 1, "an integer in 0 .. 2^31 - 1")
    B, _, H, W = d.shape
    work = _workspace("lws_speckle_workspace", d.device, B, H, W)
    out = torch.empty_like(d)
    mask_out = torch.empty(d.shape, device=d.device, dtype=torch.uint8)
    labels = torch.empty(d.shape, device=d.device, dtype=torch.int32) if want_labels else None
    counts = torch.empty((B, 3), device=d.device, dtype=torch.int64)
    _call("lws_speckle_filter", d.device, d, mask, B, H, W, max_diff, max_size, int(bool(fill)), work, out, mask_out, labels, counts)
    return SpeckleResult(out, mask_out, labels, counts)


WMEDIAN_LUT_SIZE = 766                  # s = |dr| + |dg| + |db| between two uint8 colours: 0 .. 765


def wmedian_lut(sigma, scale=4096):
    """The weight table of wmedian_filter: numpy uint16 [766], wlut[s] = rint(scale * exp(-s / (3 * sigma))) in float64, s the sum
    of the absolute colour differences to the window's centre (so sigma is in grey levels per channel).  sigma finite and > 0,
    scale an integer in 1 .. 65535 (the weight of equal colours).  The only transcendental of the filter: the table is data."""
    import numpy as np
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not (math.isfinite(sigma) and sigma > 0):
        raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= scale <= 65535:
        raise ValueError(f"scale must be an integer in 1 .. 65535, got {scale!r}")
    s = np.arange(WMEDIAN_LUT_SIZE, dtype=np.float64)
    return np.rint(np.float64(scale) * np.exp(-s / (3.0 * np.float64(sigma)))).astype(np.uint16)


WMedianResult = namedtuple("WMedianResult", ["disp", "counts"])
WMedianResult.__doc__ = """What wmedian_filter returns: the filtered maps float32 [B,1,H,W] and counts, an int64 [B,2] device tensor {valid
pixels whose value changed, invalid pixels that were filled}."""


def wmedian_filter(disp, radius, rgb=None, wlut=None, mask=None, fill_min=0):
    """Edge-aware weighted median of disparity maps (include/lwsnet_hip.h, lws_wmedian_filter): every pixel takes the lower weighted
    median of the valid disparities in its (2 radius + 1)^2 window, weighted by wlut[colour distance to the centre in rgb].  disp
    [B,1,H,W] float32 (four stage maps: torch.cat them along B and repeat the guide, every image is filtered on its own); radius
    1, 2 or 3; rgb: None (the unweighted median) or the uint8 [B,H,W,3] cropped left images; wlut: with rgb, the 766 uint16 weights
    as a numpy array (wmedian_lut; uploaded here) or a device tensor; mask: None or the uint8 lws_lr_check / lws_speckle_filter
    code map (only code-1 pixels are valid); fill_min: an invalid pixel with at least this many candidates takes their median (0:
    never).  The outputs are allocated per call on the current stream.  Returns a WMedianResult."""
    import numpy as np
    d = _disp_map(disp, "disp")
    radius = _int_in("radius", radius, 1, 3, "1, 2 or 3")
    fill_min = _int_in("fill_min", fill_min, 0, 2 ** 31 - 1, "an integer in 0 .. 2^31 - 1")
    B, _, H, W = d.shape
    mask = _code_map(mask, d)
    if rgb is None:
        if wlut is not None:
            raise ValueError("wlut is the weight table of a guide: give rgb with it")
    else:
        rgb = _guide(rgb, d)
        if isinstance(wlut, np.ndarray):
            if wlut.dtype != np.uint16 or wlut.shape != (WMEDIAN_LUT_SIZE,):
                raise ValueError(f"wlut must hold {WMEDIAN_LUT_SIZE} uint16 weights; got {wlut.dtype} {wlut.shape}")
            wlut = torch.from_numpy(np.ascontiguousarray(wlut)).to(d.device)
        elif not (isinstance(wlut, torch.Tensor) and wlut.dtype == torch.uint16 and tuple(wlut.shape) == (WMEDIAN_LUT_SIZE,)
                  and wlut.device == d.device):
            raise ValueError(f"rgb needs wlut: a numpy array or a tensor on {d.device} of {WMEDIAN_LUT_SIZE} uint16 weights (wmedian_lut)")
        wlut = wlut.contiguous()
    out = torch.empty_like(d)
    counts = torch.empty((B, 2), device=d.device, dtype=torch.int64)
    _call("lws_wmedian_filter", d.device, d, mask, rgb, wlut, B, H, W, radius, fill_min, out, counts)
    return WMedianResult(out, counts)


def rectify_pair(raw_left, raw_right, params, out_hw, origin=(0, 0), border=0, want_rect=True, want_input=True, want_valid=True,
                 want_map=False):
    """Undistorts and rectifies raw stereo pairs and normalises them for the network in one launch (include/lwsnet_hip.h,
    lws_rectify_pair).  raw_left, raw_right: uint8 [B,Hs,Ws,3] device tensors of one size; params: the float32 [B,2,18] records
    (lwsnet_amd.geometry.rectify_params; numpy, uploaded here, or a device tensor; [2,18] serves every image); out_hw = (H, W) and
    origin = (y0, x0): the window of the rectified frame to compute; border: the grey level 0..255 of the taps outside the raw image.
    Returns a dict with the outputs asked for, each a (left, right) pair of device tensors: "rect" uint8 [B,H,W,3], "input" float32
    [B,3,H,W] (the bits of preprocess_rgb8(rect)), "valid" uint8 [B,1,H,W], "map" float32 [B,H,W,2].  The outputs are allocated per
    call on the current stream."""
    import numpy as np
    for name, t in (("raw_left", raw_left), ("raw_right", raw_right)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"{name} must be a torch tensor on a HIP device (the rectification has no CPU fallback)")
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[3] != 3:
            raise ValueError(f"{name} must be a [B,Hs,Ws,3] uint8 tensor; got {t.dtype} {tuple(t.shape)}")
    if raw_left.shape != raw_right.shape or raw_left.device != raw_right.device:
        raise ValueError(f"raw_left and raw_right must share one shape and device; got {tuple(raw_left.shape)} and {tuple(raw_right.shape)}")
    if not (want_rect or want_input or want_valid or want_map):
        raise ValueError("rectify_pair: ask for at least one of rect, input, valid, map")
    raw_left, raw_right = raw_left.contiguous(), raw_right.contiguous()
    dev = raw_left.device
    B, Hs, Ws, _ = raw_left.shape
    if isinstance(params, np.ndarray):
        params = torch.from_numpy(np.ascontiguousarray(params, dtype=np.float32)).to(dev)
    if not isinstance(params, torch.Tensor) or params.dtype != torch.float32 or params.device != dev:
        raise ValueError(f"params must be a float32 numpy array or a float32 tensor on {dev}")
    if tuple(params.shape) == (2, 18):
        params = params.expand(B, 2, 18)
    if tuple(params.shape) != (B, 2, 18):
        raise ValueError(f"params must be [{B},2,18] or [2,18]; got {tuple(params.shape)}")
    params = params.contiguous()
    (H, W), (y0, x0) = (int(v) for v in out_hw), (int(v) for v in origin)
    border = _int_in("border", border, 0, 255)
    if H < 1 or W < 1:
        raise ValueError(f"out_hw must be positive, got {(H, W)}")
    res, arrays = {}, []
    for key, want, shape, dt in (("rect", want_rect, (H, W, 3), torch.uint8), ("input", want_input, (3, H, W), torch.float32),
                                 ("valid", want_valid, (1, H, W), torch.uint8), ("map", want_map, (H, W, 2), torch.float32)):
        pair = torch.empty((2, B) + shape, device=dev, dtype=dt) if want else None     # one allocation for both cameras
        if want:
            res[key] = (pair[0], pair[1])
        arrays.append(_arr(res.get(key, ()), 2))
    mean, std = _imagenet_stats()
    _call("lws_rectify_pair", dev, _arr([raw_left, raw_right], 2), params, B, Hs, Ws, H, W, x0, y0, border, mean, std, *arrays)
    return res


PhotometricResult = namedtuple("PhotometricResult", ["err", "scored", "warped", "sums"])
PhotometricResult.__doc__ = """What photometric returns: per map the error maps float32 [B,1,H,W] (0 where not scored), the uint8 [B,1,H,W]
scored maps and the uint8 [B,H,W,3] right images warped into the left view -- each a list like `disp`, or one tensor when `disp` was
one tensor, or None when not asked for -- and sums, an int64 [nmaps,B,4] device tensor {scored pixels, sum q(pe), sum q(l1),
sum q(dssim)}, q(v) = rint(v * 2^20) (lwsnet_amd.metrics.photometric_means turns it into means)."""


def photometric(disp, left_u8, right_u8, mask=None, rvalid=None, alpha=0.85, want_err=True, want_scored=False, want_warped=False):
    """Photometric reprojection error of disparity maps, a score that needs no ground truth (include/lwsnet_hip.h, lws_photometric):
    the right image warped into the left view with the map against the left image, alpha * DSSIM (3 x 3) + (1 - alpha) * L1.  disp: one
    [B,1,H,W] float32 map or a list of 1-4; left_u8, right_u8: the uint8 [B,H,W,3] images; mask: None, one uint8 [B,1,H,W]
    lws_lr_check code map for every map, or a list with one (or None) per map: only code-1 pixels are scored; rvalid: None or the
    uint8 [B,1,H,W] valid map of the right camera (rectify_pair): a tap outside it cannot be used; alpha in [0, 1].  The outputs are
    allocated per call on the current stream.  Returns a PhotometricResult."""
    single = isinstance(disp, torch.Tensor)
    maps = [disp] if single else disp
    if not isinstance(maps, (list, tuple)) or not 1 <= len(maps) <= 4:
        raise ValueError("disp must be one map or a list of 1-4 maps")
    (ds,), shape, dev = _stage_maps(disp=[d.as_subclass(torch.Tensor) if isinstance(d, torch.Tensor) else d for d in maps])
    B, _, H, W = shape
    left, right = (_guide(t, ds[0]) for t in (left_u8, right_u8))
    if mask is None or isinstance(mask, torch.Tensor):
        mask = [mask] * len(ds)
    if not isinstance(mask, (list, tuple)) or len(mask) != len(ds):
        raise ValueError("mask must be None, one code map or a list with one entry per map")
    masks = [_code_map(k, ds[0]) for k in mask]
    rvalid = _code_map(rvalid, ds[0])
    if isinstance(alpha, bool) or not (math.isfinite(alpha) and 0.0 <= alpha <= 1.0):
        raise ValueError(f"alpha must be in [0, 1], got {alpha!r}")
    n = len(ds)
    err = [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(n)] if want_err else None
    scored = [torch.empty(shape, device=dev, dtype=torch.uint8) for _ in range(n)] if want_scored else None
    warped = [torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8) for _ in range(n)] if want_warped else None
    sums = torch.empty((n, B, 4), device=dev, dtype=torch.int64)
    _call("lws_photometric", dev, _arr(ds), n, left, right, _arr(masks), rvalid, B, H, W, float(alpha), _arr(err or []), _arr(scored or []),
          _arr(warped or []), sums)
    if single:
        err, scored, warped = (v[0] if v is not None else None for v in (err, scored, warped))
    return PhotometricResult(err, scored, warped, sums)
