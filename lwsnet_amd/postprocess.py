"""The disparity post-processing chain of both CLIs (lwsnet_amd.inference and lwsnet_amd.evaluate, sequential mode): the
left-right check (`--lr_check`, LWSNet.forward_lr) or, in its place, the one-forward occlusion check (`--occ_check`,
LWSNet.forward_occ), the speckle filter (`--speckle`, ops.speckle_filter) and the edge-aware
weighted median (`--wmedian`, ops.wmedian_filter), in this order, each one optional.  This module alone knows how they combine:

- The occlusion check stands exactly where the left-right check stands, with `--occ_fill` for `--lr_fill`: every rule below
  that names "the check" holds for whichever of the two is on.  They are alternatives (one run of the network against two; the
  occlusion check finds no mismatches), and asking for both is an error.
- With the speckle filter on, the check runs unfilled, and ONE row fill by the speckle filter (`--speckle_fill`, `--lr_fill` or
  `--occ_fill`) then covers what either step dropped.  Without it, `--lr_fill` / `--occ_fill` is the check's own fill.
- The code map handed to the next step is the speckle filter's when it ran, otherwise the check's.
- The weighted median takes that code map only while no row fill has happened (only trusted pixels vote; with `--wmedian_fill N`
  a dropped pixel with at least N voting neighbours takes their median).  A row-filled map is filtered as a whole.
- The guide (the uint8 left images) is needed only when sigma > 0; sigma = 0 is the unweighted median.
- The geometry outputs of the inference CLI (`_disp16`, `_depth16`, `.ply`) take the code map only while NOTHING has been filled:
  a row fill and `--wmedian_fill N > 0` both count as filling.
- The four stage maps go through each filter as one call, concatenated along the batch dimension (every image is filtered on its
  own), with the guide repeated four times.

Options holds the flags and names these facts; run_chain runs one batch; the add_* / check_* functions are the CLIs' flags.
"""
import dataclasses
from collections import namedtuple

import numpy as np


@dataclasses.dataclass(frozen=True)
class Options:
    """The flags of the stages, named as the CLIs and evaluate.evaluate name them.  A stage is off while its main flag
    (lr_check = TAU, occ_check = TAU, speckle = SIZE, wmedian = R) is None."""
    lr_check: float = None
    lr_fill: bool = False
    speckle: int = None
    speckle_diff: float = 1.0
    speckle_fill: bool = False
    wmedian: int = None
    wmedian_sigma: float = 10.0
    wmedian_fill: int = 0
    occ_check: float = None
    occ_fill: bool = False

    @classmethod
    def make(cls, **flags):
        """From keyword arguments named as the fields, converted to the fields' types; a flag that is None keeps its default."""
        types = {f.name: f.type for f in dataclasses.fields(cls)}
        return cls(**{k: types[k](v) for k, v in flags.items() if v is not None})

    @classmethod
    def from_args(cls, args):
        """From parsed arguments; a flag the namespace does not have is off."""
        return cls.make(**{f.name: getattr(args, f.name, None) for f in dataclasses.fields(cls)})

    def check(self):
        """Raises ValueError for every value a stage that is on does not support."""
        if self.lr_check is not None:
            in_range(_invalid, "--lr_check TAU", self.lr_check)
        if self.occ_check is not None:
            in_range(_invalid, "--occ_check TAU", self.occ_check)
            if self.lr_check is not None:
                raise ValueError("--occ_check and --lr_check are alternatives: give one of them")
        if self.speckle is not None:
            if self.speckle <= 0 or self.speckle >= 2 ** 31:
                raise ValueError(f"--speckle SIZE must be an integer > 0, got {self.speckle}")
            in_range(_invalid, "--speckle_diff D", self.speckle_diff)
        if self.wmedian is not None:
            if not 1 <= self.wmedian <= 3:
                raise ValueError(f"--wmedian R must be 1, 2 or 3, got {self.wmedian}")
            in_range(_invalid, "--wmedian_sigma S", self.wmedian_sigma)
            if self.wmedian_fill < 0 or self.wmedian_fill >= 2 ** 31:
                raise ValueError(f"--wmedian_fill N must be an integer >= 0, got {self.wmedian_fill}")

    @property
    def stages_on(self):
        """The names of the stages that are on, in the chain's order."""
        names = (("lr_check", "left-right check"), ("occ_check", "occlusion check"), ("speckle", "speckle filter"), ("wmedian", "weighted median filter"))
        return [name for flag, name in names if getattr(self, flag) is not None]

    @property
    def forward_fills(self):
        """The left-right check (or the occlusion check) fills its own maps: only without the speckle filter behind it."""
        return ((self.lr_check is not None and self.lr_fill) or (self.occ_check is not None and self.occ_fill)) and self.speckle is None

    @property
    def speckle_fills(self):
        """The speckle filter's row fill, which also covers what the check dropped."""
        return self.speckle is not None and (self.speckle_fill or self.lr_fill or self.occ_fill)

    @property
    def row_filled(self):
        return self.forward_fills or self.speckle_fills

    @property
    def filled(self):
        """Anything was filled, by a row fill or by the median's hole filling."""
        return self.row_filled or (self.wmedian is not None and self.wmedian_fill > 0)

    @property
    def has_codes(self):
        return self.lr_check is not None or self.occ_check is not None or self.speckle is not None

    @property
    def needs_guide(self):
        return self.wmedian is not None and self.wmedian_sigma > 0

    @property
    def wmedian_takes_codes(self):
        return self.wmedian is not None and self.has_codes and not self.row_filled

    @property
    def geometry_takes_codes(self):
        return self.has_codes and not self.filled


class ChainResult(namedtuple("ChainResult", ["disp", "lr_masks", "speckle_masks", "keep", "lr_density", "speckle_counts", "wmedian_counts"])):
    """What run_chain returns: the four final stage maps; the left-right check's four code maps and the speckle filter's
    (None when the stage is off); keep, the four code maps the geometry outputs keep code 1 of (None once anything was filled);
    lr_density, the check's numpy [4,B]; speckle_counts [4,B,3] and wmedian_counts [4,B,2], int64 on the device (ops.speckle_filter,
    ops.wmedian_filter).  Behind these seven, as attributes that default to None and are no part of the tuple (a caller that
    unpacks or slices the seven sees what it saw before the occlusion check existed): occ_masks and occ_density, the occlusion
    check's four code maps and its numpy [4,B]."""

    def __new__(cls, disp, lr_masks, speckle_masks, keep, lr_density, speckle_counts, wmedian_counts, occ_masks=None, occ_density=None):
        self = super().__new__(cls, disp, lr_masks, speckle_masks, keep, lr_density, speckle_counts, wmedian_counts)
        self.occ_masks, self.occ_density = occ_masks, occ_density
        return self

    def with_stage4(self, disp, keep):
        """This result with another stage-4 map and, where there are `keep` codes, another stage-4 code map."""
        new = self._replace(disp=list(self.disp[:3]) + [disp], keep=None if self.keep is None else list(self.keep[:3]) + [keep])
        new.occ_masks, new.occ_density = self.occ_masks, self.occ_density      # (_replace copies the tuple's seven only)
        return new

    def with_stage4_keep(self, keep):
        """This result with another stage-4 code map, also where there were no `keep` codes: the other stages then keep every pixel
        (all 1), which is what having no codes meant for them."""
        import torch
        new = self._replace(keep=(list(self.keep[:3]) if self.keep is not None else [torch.ones_like(keep) for _ in range(3)]) + [keep])
        new.occ_masks, new.occ_density = self.occ_masks, self.occ_density
        return new


def run_chain(model, left, right, options, guide=None):
    """One batch through the forward (or forward_lr, or forward_occ), the speckle filter and the weighted median, as `options` has them on (the
    module docstring has the rules).  guide: the uint8 [B,H,W,3] left images on the device, needed when options.needs_guide.
    Returns a ChainResult."""
    o = options
    lr_masks = occ_masks = sp_masks = density = occ_density = sp_counts = wm_counts = None
    if o.lr_check is not None:
        res = model.forward_lr(left, right, tau=o.lr_check, fill=o.forward_fills)
        disp, lr_masks, density = res.disp, res.mask, res.density
    elif o.occ_check is not None:
        res = model.forward_occ(left, right, tau=o.occ_check, fill=o.forward_fills)
        disp, occ_masks, occ_density = res.disp, res.mask, res.density
    else:
        disp = model(left, right)
    codes = lr_masks if lr_masks is not None else occ_masks
    if o.speckle is not None:
        disp, sp_masks, sp_counts = speckle_stages(disp, codes, o.speckle, o.speckle_diff, o.speckle_fills)
        codes = sp_masks
    if o.wmedian is not None:
        disp, wm_counts = wmedian_stages(disp, codes if o.wmedian_takes_codes else None, guide, o.wmedian, o.wmedian_sigma, o.wmedian_fill)
    return ChainResult(disp, lr_masks, sp_masks, codes if o.geometry_takes_codes else None, density, sp_counts, wm_counts, occ_masks,
                       occ_density)


def speckle_stages(disp, masks, size, diff, fill):
    """ops.speckle_filter on the four stage maps of one forward ([B,1,H,W] each, concatenated along B: every image is filtered on
    its own) with the left-right (or occlusion) check's masks (or None).  Returns (filtered maps, code maps, counts [4,B,3] on the device)."""
    import torch
    from . import ops
    from .models import DisparityTensor
    B = disp[0].shape[0]
    with torch.cuda.device(disp[0].device):
        res = ops.speckle_filter(torch.cat([d.as_subclass(torch.Tensor) for d in disp]), size, diff,
                                 torch.cat(list(masks)) if masks is not None else None, fill=fill)
    return ([DisparityTensor.wrap(res.disp[s * B:(s + 1) * B]) for s in range(4)], [res.mask[s * B:(s + 1) * B] for s in range(4)],
            res.counts.view(4, B, 3))


def wmedian_stages(disp, masks, rgb, radius, sigma, fill_min):
    """ops.wmedian_filter on the four stage maps of one forward ([B,1,H,W] each, concatenated along B: every image is filtered on
    its own) with their code maps (or None) and the guide rgb (uint8 [B,H,W,3] on the device, repeated per stage; unused when
    sigma == 0).  Returns (filtered maps, counts [4,B,2] on the device)."""
    import torch
    from . import ops
    from .models import DisparityTensor
    B = disp[0].shape[0]
    guided = sigma > 0
    with torch.cuda.device(disp[0].device):
        res = ops.wmedian_filter(torch.cat([d.as_subclass(torch.Tensor) for d in disp]), radius,
                                 rgb=rgb.repeat(4, 1, 1, 1) if guided else None, wlut=ops.wmedian_lut(sigma) if guided else None,
                                 mask=torch.cat(list(masks)) if masks is not None else None, fill_min=fill_min)
    return [DisparityTensor.wrap(res.disp[s * B:(s + 1) * B]) for s in range(4)], res.counts.view(4, B, 2)


def add_lr_arguments(p):
    """--lr_check TAU / --lr_fill (not in the reference): LWSNet.forward_lr."""
    p.add_argument("--lr_check", type=float, default=None, metavar="TAU",
                   help="left-right consistency check: keep the pixels whose left- and right-view disparities differ by <= TAU "
                        "(sequential mode only; not in the reference)")
    p.add_argument("--lr_fill", action="store_true", help="with --lr_check: fill the dropped pixels with their row's background value")


def add_occ_arguments(p):
    """--occ_check TAU / --occ_fill (not in the reference): LWSNet.forward_occ.  A command line without them parses to the
    namespace it parsed to before they existed (argparse.SUPPRESS); check_occ_arguments writes their defaults, None and False."""
    import argparse
    p.add_argument("--occ_check", type=float, default=argparse.SUPPRESS, metavar="TAU",
                   help="one-forward occlusion check, the alternative to --lr_check: splat the left-view disparities into the right "
                        "view and drop the pixels behind a surface more than TAU nearer (sequential mode only; not in the reference)")
    p.add_argument("--occ_fill", action="store_true", default=argparse.SUPPRESS, help="with --occ_check: fill the dropped pixels with their row's background value")


def add_speckle_arguments(p):
    """--speckle SIZE / --speckle_diff D / --speckle_fill (not in the reference): ops.speckle_filter."""
    p.add_argument("--speckle", type=int, default=None, metavar="SIZE",
                   help="speckle filter: remove the connected blobs of at most SIZE pixels from the disparity maps (sequential mode "
                        "only; not in the reference)")
    p.add_argument("--speckle_diff", type=float, default=None, metavar="D",
                   help="with --speckle: neighbours are connected when their disparities differ by <= D (default 1.0)")
    p.add_argument("--speckle_fill", action="store_true",
                   help="with --speckle: fill the removed pixels with their row's background value")


def add_wmedian_arguments(p):
    """--wmedian R / --wmedian_sigma S / --wmedian_fill N (not in the reference): ops.wmedian_filter."""
    p.add_argument("--wmedian", type=int, default=None, metavar="R",
                   help="edge-aware weighted median filter of the disparity maps over a (2R + 1)^2 window, R in 1..3, weighted by "
                        "the left image (sequential mode only; not in the reference)")
    p.add_argument("--wmedian_sigma", type=float, default=None, metavar="S",
                   help="with --wmedian: colour scale of the weights in grey levels per channel (default 10.0; 0 = the unweighted "
                        "median, no guide)")
    p.add_argument("--wmedian_fill", type=int, default=None, metavar="N",
                   help="with --wmedian: a dropped pixel with at least N trusted neighbours in its window takes their median "
                        "(default 0 = holes are not filled)")


def sequential_only(p, args, flag, verb="runs"):
    """The stages run in the CLIs' sequential mode: a parser error for `flag` (several flags: verb="run") with --workers N > 0."""
    if args.workers > 0:
        p.error(f"{flag} {verb} in the sequential mode only: use --workers 0")


def needs_camera(p, args, flags):
    """A parser error for `flags` (their names as the sentence's subject) when nothing gives a camera: --calib, --camera or --rectify."""
    if args.calib is None and args.camera is None and getattr(args, "rectify", None) is None:
        p.error(f"{flags} need a camera: --calib PATH or --camera FX FY CX CY BASELINE")


def in_range(fail, name, v, lo=0, hi=None, strict=False):
    """The one wording of a flag's range: fail(sentence) -- a parser's error, or _invalid -- unless v is finite and >= lo (> lo
    when strict) or, with hi, in lo .. hi."""
    if hi is not None:
        if not lo <= v <= hi:
            fail(f"{name} must be in {lo} .. {hi}, got {v}")
    elif not (np.isfinite(v) and (v > lo if strict else v >= lo)):
        fail(f"{name} must be finite and {'>' if strict else '>='} {lo}, got {v}")


def _invalid(sentence):
    raise ValueError(sentence)


def set_defaults(args, **defaults):
    """Writes the default of every flag that the parser left out of the namespace (argparse.SUPPRESS) or at None."""
    for flag, value in defaults.items():
        if getattr(args, flag, None) is None:
            setattr(args, flag, value)


# main flag -> (the flags that depend on it, the error when one of them comes without it)
_DEPENDENT = {"lr_check": (("lr_fill",), "--lr_fill needs --lr_check TAU"),
              "occ_check": (("occ_fill",), "--occ_fill needs --occ_check TAU"),
              "speckle": (("speckle_diff", "speckle_fill"), "--speckle_fill and --speckle_diff need --speckle SIZE"),
              "wmedian": (("wmedian_sigma", "wmedian_fill"), "--wmedian_sigma and --wmedian_fill need --wmedian R")}


def _check_stage(p, args, main):
    """One stage's flags, before any model or GPU work: a dependent flag without the main one, Options.check on the stage's values
    (the defaults of its dependent flags are written back into args), --workers."""
    dependent, lonely = _DEPENDENT[main]
    if getattr(args, main) is None:
        if any(getattr(args, f) is not None and getattr(args, f) is not False for f in dependent):
            p.error(lonely)
        return
    options = Options.make(**{f: getattr(args, f) for f in (main, *dependent)})
    for f in dependent:
        setattr(args, f, getattr(options, f))
    try:
        options.check()
    except ValueError as e:
        p.error(str(e))
    sequential_only(p, args, "--" + main)


def check_lr_arguments(p, args):
    """Rejects what the left-right check does not support."""
    _check_stage(p, args, "lr_check")


OCC_DEFAULTS = dict(occ_check=None, occ_fill=False)


def check_occ_arguments(p, args):
    """Rejects what the occlusion check does not support, --lr_check beside it included; sets the flags' defaults."""
    set_defaults(args, **OCC_DEFAULTS)
    if args.occ_check is not None and getattr(args, "lr_check", None) is not None:
        p.error("--occ_check and --lr_check are alternatives: give one of them")
    _check_stage(p, args, "occ_check")


def check_speckle_arguments(p, args):
    """Rejects what the speckle filter does not support; sets the default of --speckle_diff."""
    _check_stage(p, args, "speckle")


def check_wmedian_arguments(p, args):
    """Rejects what the weighted median filter does not support; sets the defaults of --wmedian_sigma and --wmedian_fill."""
    _check_stage(p, args, "wmedian")


def add_photometric_arguments(p, save=False):
    """--photometric / --photo_alpha A (and, for the inference CLI, --save_photo; not in the reference): ops.photometric.  A command
    line without them parses to the namespace it parsed to before they existed (argparse.SUPPRESS); check_photometric_arguments
    writes their defaults."""
    import argparse
    p.add_argument("--photometric", action="store_true", default=argparse.SUPPRESS,
                   help="score the disparity maps without ground truth: the photometric reprojection error of the right image warped "
                        "into the left view (sequential mode only; not in the reference)")
    p.add_argument("--photo_alpha", type=float, default=argparse.SUPPRESS, metavar="A",
                   help="with --photometric: the error is A * DSSIM + (1 - A) * L1, A in [0, 1] (default 0.85)")
    if save:
        p.add_argument("--save_photo", action="store_true", default=argparse.SUPPRESS,
                       help="with --photometric: write <stem>_pe.png, the error map as rint(pe * 255), and <stem>_warp.png, the warped right image")


def photometric_defaults(args, save=False):
    set_defaults(args, photometric=False, **({"save_photo": False} if save else {}), photo_alpha=0.85)


def check_photometric_arguments(p, args, save=False):
    """Rejects what the photometric error does not support, before any model or GPU work; sets the flags' defaults (False, 0.85
    and, for the CLI that has --save_photo, False)."""
    alpha_given = getattr(args, "photo_alpha", None) is not None
    photometric_defaults(args, save)
    if not args.photometric and (alpha_given or (save and args.save_photo)):
        p.error("--photo_alpha and --save_photo need --photometric" if save else "--photo_alpha needs --photometric")
    if not 0.0 <= args.photo_alpha <= 1.0:                              # (false for NaN)
        p.error(f"--photo_alpha A must be in [0, 1], got {args.photo_alpha}")
    if args.photometric:
        sequential_only(p, args, "--photometric")
