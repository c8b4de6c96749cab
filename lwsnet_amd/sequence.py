"""The stages of the inference CLI that treat the frames of directory mode as a sequence -- `--egomotion`, `--tsdf_track`,
`--movers`, `--temporal`, `--tsdf` (lwsnet_amd/inference.py's docstring describes the flags) -- and the one source of their poses.

A stage is an object with four methods, and the run's stages are a tuple that inference.inference() walks with a `for`, in the
order ego-motion (on the chain's own map), model tracking (the estimate refined against the volume), movers (what disagrees with
that motion leaves the `keep` codes), filter, volume (on what the
filter left): step(s, log) takes the record of a processed
pair -- index, frame, res (the ChainResult), conf, and what the stages of this frame made so far: ego (the ops.EgoResult, None on a
first frame), track (the ops.TrackResult of --tsdf_track, None on a first frame), movers (the ops.MoversResult of --movers, None on a frame that
was not segmented), fused (the ops.TemporalResult; res then holds the fused map in the chain's place), view (the ops.TsdfView of
--save_tsdf) -- and leaves what it made in it; skip(path, log) hears of a pair that was skipped; save(s, stem, log) writes the stage's own
per-frame file beside the colour file and finish(log) the file at the end of the run, both returning the paths.  A new stage is a
class like these, its flags' add_* / *_DEFAULTS / check_* beside it, its name in begin(), and its check called by inference.main().

PoseSource is the only code that maps a pair's index to a pose and the only one that knows of skipped pairs.  It is backed by the
file of --poses (read once, by the argument check), by the run's Odometry or, with --tsdf_track, by the run's ModelTracker, and answers what the stages ask: the camera-to-world
pose of the current pair, the motion from the pair processed before it, the lines of --save_poses.  Each answer is computed as it
was before there was one source -- geometry.relative_pose for the file, the estimate's own block, the Odometry's accumulated
float64 poses -- because the files written are compared bit for bit.
"""
import argparse
import glob
import os

import numpy as np

from . import outputs as out
from . import postprocess as post


def list_pairs(args):
    """The (left, right) image paths of directory mode (inference.py:50-60), in sorted order: pair i is frame i of the sequence."""
    if os.path.isdir(args.img_path):
        return tuple(sorted(glob.glob(os.path.join(args.img_path, side + "/*.png"))) for side in ("image_2", "image_3"))
    base, name = os.path.dirname(os.path.dirname(args.img_path)), os.path.basename(args.img_path)
    return [os.path.join(base, "image_2", name)], [os.path.join(base, "image_3", name)]


def _a_sequence(p, args, flag, save, verb):
    """What every sequence stage needs, refused in this order: a camera, the sequential mode, directory mode."""
    post.needs_camera(p, args, f"--{flag} and --{save}")
    post.sequential_only(p, args, f"--{flag} / --{save}", "run")
    if args.left_img:
        p.error(f"--{flag} {verb} a sequence: use directory mode (--img_path), not --left_img")


def read_poses(p, args):
    """--poses: the file's float64 [N,3,4], read once for the run; a parser error when it cannot be read or is shorter than the pairs."""
    from .geometry import read_kitti_poses
    try:
        poses = read_kitti_poses(args.poses)
    except (OSError, ValueError) as e:
        p.error(f"--poses: cannot read {args.poses}: {e}")
    pairs = len(list_pairs(args)[0])
    if len(poses) < pairs:
        p.error(f"--poses: {args.poses} holds {len(poses)} poses for {pairs} pairs (line i belongs to the i-th pair in sorted order)")
    return poses


TSDF_FOLLOW_STEP = 16                                       # --tsdf_follow without a number, in voxels


def add_sequence_arguments(p):
    """--temporal, --egomotion, --tsdf and their flags (not in the reference).  A command line without them parses to the namespace it
    parsed to before they existed (argparse.SUPPRESS); the check_* functions write their defaults."""
    S = argparse.SUPPRESS
    p.add_argument("--temporal", action="store_true", default=S,
                   help="fuse the stage-4 maps of the sequence over time with the poses of --poses (directory mode, sequential only; "
                        "needs a camera; not in the reference)")
    p.add_argument("--poses", type=str, default=S, metavar="PATH",
                   help="with --temporal: a KITTI odometry poses.txt, 12 numbers per line (camera-to-world), line i for the i-th pair in sorted order")
    p.add_argument("--temporal_gate", type=float, default=S, metavar="G", help="temporal: the gate in standard deviations (default 3)")
    p.add_argument("--temporal_q", type=float, default=S, metavar="Q", help="temporal: process noise in px^2 per frame (default 0)")
    p.add_argument("--temporal_sigma", type=str, default=S, metavar="S|net",
                   help="temporal: the measurement's sigma in px (default 0.5), or `net` for the network's own stage-3 sigma")
    p.add_argument("--temporal_hold", action="store_true", default=S, help="temporal: a pixel the checks dropped holds what was seen there in earlier frames")
    p.add_argument("--save_temporal", action="store_true", default=S,
                   help="--temporal, and write <stem>_tcode.png (the codes in colour) and <stem>_tsigma.png (the fused sigma, scaled as --save_conf's)")
    p.add_argument("--egomotion", action="store_true", default=S,
                   help="estimate the left camera's motion from frame to frame by dense direct alignment (directory mode, sequential "
                        "only; needs a camera; not in the reference)")
    p.add_argument("--ego_levels", type=int, default=S, metavar="N", help="egomotion: pyramid levels, 1 .. 8 (default 4)")
    p.add_argument("--ego_iters", type=int, default=S, metavar="N", help="egomotion: Gauss-Newton steps per level, 1 .. 64 (default 8)")
    p.add_argument("--ego_huber", type=float, default=S, metavar="K", help="egomotion: the Huber threshold in grey levels (default 10)")
    p.add_argument("--save_poses", type=str, default=S, metavar="PATH", help="egomotion: write the accumulated camera-to-world poses as a KITTI odometry poses.txt")
    p.add_argument("--save_ego", action="store_true", default=S, help="egomotion: write <stem>_ego.png, the magnitude of the residual at the final pose")
    p.add_argument("--tsdf", action="store_true", default=S,
                   help="integrate the stage-4 maps of the sequence into a TSDF volume with the poses of --poses or --egomotion (directory "
                        "mode, sequential only; needs a camera; not in the reference)")
    p.add_argument("--tsdf_voxel", type=float, default=S, metavar="V", help="tsdf: the voxel's side in metres (default 0.2)")
    p.add_argument("--tsdf_extent", type=float, nargs=6, default=S, metavar=("X0", "X1", "Y0", "Y1", "Z0", "Z1"),
                   help="tsdf: the volume's extent in metres in the first camera's frame, y down, z forward (default -12.8 12.8 -3.2 3.2 0 51.2)")
    p.add_argument("--tsdf_trunc", type=float, default=S, metavar="MU0", help="tsdf: the truncation band in metres (default 3 voxels)")
    p.add_argument("--tsdf_trunc_px", type=float, default=S, metavar="MU_D",
                   help="tsdf: the band in pixels of disparity, so that it grows as z^2: max(MU0, MU_D * z^2 / fb) (default 0)")
    p.add_argument("--tsdf_weight", type=str, default=S, choices=("unit", "sigma"),
                   help="tsdf: a frame counts 1, or 1 / sigma_z^2 with the sigma of --temporal (0.5 px without it) (default unit)")
    p.add_argument("--tsdf_sdf", type=str, default=S, choices=("plane", "ray"),
                   help="tsdf: the distance to the pixel's tangent plane (surface normals with --max_jump) or along the ray (default plane)")
    p.add_argument("--save_tsdf_ply", type=str, default=S, metavar="PATH",
                   help="tsdf: at the end, write the volume's zero crossings as a binary PLY of vertices with normals and colours")
    p.add_argument("--save_tsdf_mesh", type=str, default=S, metavar="PATH",
                   help="tsdf: at the end, write the volume's zero level set as a binary PLY of the same vertices and the triangles between them")
    p.add_argument("--tsdf_follow", type=int, nargs="?", const=TSDF_FOLLOW_STEP, default=S, metavar="N",
                   help="tsdf: the volume follows the camera, moving by whole voxels once the view's centre is N voxels from its own (default 16; "
                        "at least 1, below the smallest dimension minus 2); what leaves is spilled to --save_tsdf_mesh / --save_tsdf_ply in chunks "
                        "first.  A seam vertex is in both chunks that meet there, a normal at a chunk's border is zero, what re-enters the "
                        "volume is mapped afresh (a loop gives two surfaces), and after a sharp turn what lies behind the camera is spilled")
    p.add_argument("--save_tsdf", action="store_true", default=S, help="tsdf: write <stem>_tsdf.png, the volume ray-cast into the frame's own pose, coloured as the stage maps")
    p.add_argument("--tsdf_track", action="store_true", default=S,
                   help="refine each frame's --egomotion estimate against the --tsdf volume (joint photometric + point-to-plane cost); the "
                        "filter, the volume and --save_poses then get the tracked poses (needs --tsdf and --egomotion, not --poses)")
    p.add_argument("--track_iters", type=int, default=S, metavar="N", help="tsdf_track: Gauss-Newton steps, 1 .. 64 (default 6)")
    p.add_argument("--track_lambda", type=float, default=S, metavar="L", help="tsdf_track: the weight of the point-to-plane term, 0 switches it off (default 1)")
    p.add_argument("--track_gate", type=float, default=S, metavar="G", help="tsdf_track: the gate of the point-to-plane residual in standard deviations (default 4)")
    p.add_argument("--save_track", action="store_true", default=S, help="tsdf_track: write <stem>_track.png, the point-to-plane residual at the final pose in standard deviations, coloured")
    p.add_argument("--movers", action="store_true", default=S,
                   help="segment what moves between consecutive frames under the motion of --poses or --egomotion (--tsdf_track: the tracked one) "
                        "and take it out of the `keep` codes, so that --temporal and --tsdf never fuse it (directory mode, sequential only; "
                        "needs a camera; not in the reference)")
    p.add_argument("--movers_gate", type=float, default=S, metavar="G", help="movers: the gate of the disparity residual in standard deviations (default 3)")
    p.add_argument("--movers_gate_p", type=float, default=S, metavar="P", help="movers: the gate of the grey-level residual (default 25; inf switches the term off)")
    p.add_argument("--movers_radius", type=int, default=S, metavar="R", help="movers: the window of taps in the previous frame, 0 .. 2 (default 0: one tap)")
    p.add_argument("--movers_min_pixels", type=int, default=S, metavar="N", help="movers: the smallest component that is a mover (default 64)")
    p.add_argument("--movers_grow", type=int, default=S, metavar="N", help="movers: pixels around a mover that leave the `keep` codes with it, 0 .. 8 (default 2)")
    p.add_argument("--movers_uncovered", action="store_true", default=S,
                   help="movers: uncovered pixels are candidates too -- a receding mover is then found, and so is every disocclusion")
    p.add_argument("--save_movers", action="store_true", default=S,
                   help="movers: write <stem>_movers.png (the evidence codes in colour, movers outlined) and <stem>_movers.csv (one line per mover)")


TEMPORAL_DEFAULTS = dict(temporal=False, poses=None, temporal_gate=3.0, temporal_q=0.0, temporal_sigma="0.5", temporal_hold=False, save_temporal=False)


def temporal_sigma(args):
    """--temporal_sigma as (the scalar sigma0 in px, or None for the network's stage-3 sigma)."""
    return None if args.temporal_sigma == "net" else float(args.temporal_sigma)


def check_temporal_arguments(p, args):
    """Rejects what the temporal filter does not support, before any model or GPU work; sets the defaults.  Returns read_poses' or None."""
    given = [f for f in ("temporal_gate", "temporal_q", "temporal_sigma", "temporal_hold") if getattr(args, f, None) not in (None, False)]
    post.set_defaults(args, **TEMPORAL_DEFAULTS)
    args.temporal = args.temporal or args.save_temporal
    if not args.temporal:
        if given or (args.poses is not None and not getattr(args, "tsdf", False) and not getattr(args, "movers", False)):
            p.error("--poses, --temporal_gate, --temporal_q, --temporal_sigma and --temporal_hold need --temporal")
        return None
    ego = bool(getattr(args, "egomotion", False))
    if ego and args.poses is not None:
        p.error("--temporal --egomotion takes the filter's poses from the estimate: do not give --poses as well")
    if args.poses is None and not ego:
        p.error("--temporal needs --poses PATH, the camera-to-world pose of every pair")
    _a_sequence(p, args, "temporal", "save_temporal", "fuses")
    try:
        if temporal_sigma(args) is not None and not (np.isfinite(temporal_sigma(args)) and temporal_sigma(args) >= 0):
            raise ValueError
    except ValueError:
        p.error(f"--temporal_sigma must be a finite number of pixels >= 0 or `net`, got {args.temporal_sigma}")
    if temporal_sigma(args) is None and (args.lr_check is not None or getattr(args, "occ_check", None) is not None):
        p.error("--temporal_sigma net uses the network's own sigma and does not combine with --lr_check or --occ_check")
    post.in_range(p.error, "--temporal_gate", args.temporal_gate, strict=True)
    post.in_range(p.error, "--temporal_q", args.temporal_q)
    return None if ego else read_poses(p, args)


EGO_DEFAULTS = dict(egomotion=False, ego_levels=4, ego_iters=8, ego_huber=10.0, save_poses=None, save_ego=False)


def check_egomotion_arguments(p, args):
    """Rejects what the ego-motion estimate does not support, before any model or GPU work; sets the defaults."""
    given = [f for f in ("ego_levels", "ego_iters", "ego_huber", "save_poses", "save_ego") if hasattr(args, f)]   # (SUPPRESS: there only if given)
    post.set_defaults(args, **EGO_DEFAULTS)
    if not args.egomotion:
        if given:
            p.error("--ego_levels, --ego_iters, --ego_huber, --save_poses and --save_ego need --egomotion")
        return
    _a_sequence(p, args, "egomotion", "save_ego", "follows")
    post.in_range(p.error, "--ego_levels", args.ego_levels, 1, 8)
    post.in_range(p.error, "--ego_iters", args.ego_iters, 1, 64)
    post.in_range(p.error, "--ego_huber", args.ego_huber, strict=True)


TSDF_DEFAULTS = dict(tsdf=False, tsdf_voxel=0.2, tsdf_extent=(-12.8, 12.8, -3.2, 3.2, 0.0, 51.2), tsdf_trunc=None, tsdf_trunc_px=0.0,
                     tsdf_weight="unit", tsdf_sdf="plane", save_tsdf_ply=None, save_tsdf=False)
TSDF_MAX_POINTS = 1 << 22                                   # the capacity of --save_tsdf_ply, in records of 32 bytes


def tsdf_grid(args):
    """(origin, dims) of the volume --tsdf_extent and --tsdf_voxel describe: voxel centres from X0, Y0, Z0 on, as many as reach the far ends."""
    e, v = args.tsdf_extent, args.tsdf_voxel
    return (e[0], e[2], e[4]), tuple(int(np.floor((e[2 * k + 1] - e[2 * k]) / v + 0.5)) + 1 for k in range(3))


def check_tsdf_arguments(p, args):
    """Rejects what the volume does not support, before any model or GPU work; sets the defaults.  Returns read_poses' or None."""
    from . import ops
    given = [f for f in TSDF_DEFAULTS if f != "tsdf" and hasattr(args, f)]      # (SUPPRESS: there only if given)
    post.set_defaults(args, **TSDF_DEFAULTS)
    if not args.tsdf:
        if given:
            p.error("--tsdf_voxel, --tsdf_extent, --tsdf_trunc, --tsdf_trunc_px, --tsdf_weight, --tsdf_sdf, --save_tsdf_ply and --save_tsdf need --tsdf")
        return None
    _a_sequence(p, args, "tsdf", "save_tsdf", "maps")
    if getattr(args, "poses", None) is None and not getattr(args, "egomotion", False):
        p.error("--tsdf needs the pose of every pair: --poses PATH or --egomotion")
    post.in_range(p.error, "--tsdf_voxel", args.tsdf_voxel, strict=True)
    e = args.tsdf_extent
    if not (np.isfinite(e).all() and e[0] < e[1] and e[2] < e[3] and e[4] < e[5]):
        p.error(f"--tsdf_extent must be finite X0 < X1, Y0 < Y1, Z0 < Z1, got {' '.join(str(v) for v in e)}")
    try:
        ops.tsdf_volume_args(tsdf_grid(args)[0], args.tsdf_voxel, tsdf_grid(args)[1])
    except ValueError as err:
        p.error(f"--tsdf_extent / --tsdf_voxel: {err}")
    if args.tsdf_trunc is None:
        args.tsdf_trunc = 3.0 * args.tsdf_voxel
    post.in_range(p.error, "--tsdf_trunc", args.tsdf_trunc, strict=True)
    post.in_range(p.error, "--tsdf_trunc_px", args.tsdf_trunc_px)
    read = getattr(args, "temporal", False) or getattr(args, "egomotion", False)      # check_temporal_arguments read the file, or there is none
    return None if read else read_poses(p, args)


TSDF_MESH_DEFAULTS = dict(save_tsdf_mesh=None)             # a table of its own: TSDF_DEFAULTS is the flags --tsdf came with
TSDF_MAX_FACES = 1 << 23                                    # the capacity of --save_tsdf_mesh, in triangles of 13 bytes


def check_tsdf_mesh_arguments(p, args):
    """--save_tsdf_mesh, behind check_tsdf_arguments: sets the default; the flag without --tsdf is refused."""
    post.set_defaults(args, **TSDF_MESH_DEFAULTS)
    if args.save_tsdf_mesh is not None and not getattr(args, "tsdf", False):
        p.error("--save_tsdf_mesh needs --tsdf")


TSDF_FOLLOW_DEFAULTS = dict(tsdf_follow=None)              # a table of its own, as TSDF_MESH_DEFAULTS


def check_tsdf_follow_arguments(p, args):
    """--tsdf_follow, behind check_tsdf_arguments: sets the default; the flag without --tsdf or with N out of range is refused."""
    post.set_defaults(args, **TSDF_FOLLOW_DEFAULTS)
    if args.tsdf_follow is None:
        return
    if not getattr(args, "tsdf", False):
        p.error("--tsdf_follow needs --tsdf")
    top = min(tsdf_grid(args)[1]) - 2
    if not 1 <= args.tsdf_follow < top:
        p.error(f"--tsdf_follow must be at least 1 and below the volume's smallest dimension minus 2 = {top} voxels, got {args.tsdf_follow}")


TRACK_DEFAULTS = dict(tsdf_track=False, track_iters=6, track_lambda=1.0, track_gate=4.0, save_track=False)
TRACK_HUBER_G = 1.5                                         # the Huber threshold of the point-to-plane term: the gate may not lie below it


def check_track_arguments(p, args):
    """--tsdf_track, behind check_tsdf_arguments: rejects what the tracker does not support, before any model or GPU work; sets the defaults."""
    given = [f for f in TRACK_DEFAULTS if f != "tsdf_track" and hasattr(args, f)]      # (SUPPRESS: there only if given)
    post.set_defaults(args, **TRACK_DEFAULTS)
    if not args.tsdf_track:
        if given:
            p.error("--track_iters, --track_lambda, --track_gate and --save_track need --tsdf_track")
        return
    if getattr(args, "left_img", None):
        p.error("--tsdf_track follows a sequence: use directory mode (--img_path), not --left_img")
    if getattr(args, "poses", None) is not None:
        p.error("--tsdf_track estimates the poses: do not give --poses as well")
    if not getattr(args, "tsdf", False):
        p.error("--tsdf_track needs --tsdf, the volume it tracks against")
    if not getattr(args, "egomotion", False):
        p.error("--tsdf_track needs --egomotion, the frame-to-frame estimate it starts from")
    post.in_range(p.error, "--track_iters", args.track_iters, 1, 64)
    post.in_range(p.error, "--track_lambda", args.track_lambda)
    post.in_range(p.error, "--track_gate", args.track_gate, TRACK_HUBER_G, float("inf"))


MOVERS_DEFAULTS = dict(movers=False, movers_gate=3.0, movers_gate_p=25.0, movers_radius=0, movers_min_pixels=64, movers_grow=2,
                       movers_uncovered=False, save_movers=False)


def check_movers_arguments(p, args):
    """--movers, behind the checks of the other sequence flags: rejects what the segmentation does not support, before any model or
    GPU work; sets the defaults.  Returns read_poses' where neither --temporal nor --tsdf read the file of --poses, else None."""
    given = [f for f in MOVERS_DEFAULTS if f != "movers" and hasattr(args, f)]      # (SUPPRESS: there only if given)
    post.set_defaults(args, **MOVERS_DEFAULTS)
    if not args.movers:
        if given:
            p.error("--movers_gate, --movers_gate_p, --movers_radius, --movers_min_pixels, --movers_grow, --movers_uncovered and --save_movers need --movers")
        return None
    _a_sequence(p, args, "movers", "save_movers", "follows")
    if getattr(args, "poses", None) is None and not getattr(args, "egomotion", False):
        p.error("--movers needs the motion between the frames: --poses PATH or --egomotion")
    post.in_range(p.error, "--movers_gate", args.movers_gate, strict=True)
    if not args.movers_gate_p > 0:
        p.error(f"--movers_gate_p must be > 0 (inf switches the term off), got {args.movers_gate_p}")
    post.in_range(p.error, "--movers_radius", args.movers_radius, 0, 2)
    post.in_range(p.error, "--movers_min_pixels", args.movers_min_pixels, 1, 2 ** 31 - 1)
    post.in_range(p.error, "--movers_grow", args.movers_grow, 0, 8)
    read = getattr(args, "temporal", False) or getattr(args, "tsdf", False) or getattr(args, "egomotion", False)     # an earlier check read the file, or there is none
    return None if read else read_poses(p, args)


class PoseSource:
    """The poses of a run's pairs.  poses: the float64 [N,3,4] of --poses, line i for pair i; None: they are estimated, and `odometry`
    is the run's egomotion.Odometry from the ego-motion stage's first frame on, its k-th pose that of the k-th pair processed; with
    --tsdf_track, `tracker` is the run's tracking.ModelTracker from the tracking stage's first frame on, and answers in its place.
    frame(index) announces each processed pair, in order; one never announced was skipped, and the next motion spans the gap."""

    def __init__(self, pairs, poses=None):
        self.pairs, self.poses, self.odometry, self.seen = pairs, poses, None, []      # seen: the indices of the pairs processed so far
        self.tracker = None

    def frame(self, index):
        self.seen.append(index)

    def world(self):
        """The camera-to-world pose [3,4] of the current pair."""
        if self.tracker is not None:
            return self.tracker.poses()[-1]
        return self.poses[self.seen[-1]] if self.poses is not None else self.odometry.poses()[-1]

    def relative(self, s, log, warn=True):
        """TemporalFilter.step's motion from the pair processed before to the current one (the record s); None: the filter starts anew.
        warn=False: an untrusted motion is answered with None and no line in the log (the movers stage asks before the filter does and
        says its own)."""
        from . import ops
        if self.poses is not None:
            from .geometry import relative_pose
            return None if len(self.seen) < 2 else relative_pose(self.poses[self.seen[-2]], self.poses[self.seen[-1]])
        if self.tracker is not None:
            if s.track is not None and int(s.track.status[0]) & ops.TRACK_UNTRUSTED:
                if warn:
                    log.warning("Temporal: the tracked pose of %s is not to be trusted (status %d): the filter starts anew", s.frame.path,
                                int(s.track.status[0]))
                return None
            return None if s.track is None else s.track.pose
        if s.ego is not None and int(s.ego.status[0]) & ops.EGO_UNTRUSTED:
            if warn:
                log.warning("Temporal: the ego-motion estimate of %s is not to be trusted (status %d): the filter starts anew", s.frame.path,
                            int(s.ego.status[0]))
            return None
        return None if s.ego is None else s.ego.pose

    def lines(self):
        """The float64 [pairs,3,4] of --save_poses: a skipped pair repeats the last pair processed before it, else the identity."""
        identity = np.hstack([np.eye(3), np.zeros((3, 1))])
        estimator = self.tracker if self.tracker is not None else self.odometry
        poses = estimator.poses() if estimator is not None else np.zeros((0, 3, 4))
        at = np.searchsorted(self.seen, np.arange(self.pairs), side="right") - 1       # per pair: its pose among the estimator's, -1 before the first
        return np.stack([poses[k] if k >= 0 else identity for k in at]) if self.pairs else poses


def _stage4(res):
    """(the stage-4 map as a plain tensor, its `keep` codes or None) of a ChainResult."""
    import torch
    return res.disp[3].as_subclass(torch.Tensor), res.keep[3] if res.keep is not None else None


class _Stage:
    """What a stage does where it has nothing of its own to do: nothing for a skipped pair, no files."""

    def __init__(self, args, source):
        self.args, self.source = args, source

    def skip(self, path, log):
        pass

    def save(self, s, stem, log):
        return []

    def finish(self, log):
        return []


class _Odometry(_Stage):
    """--egomotion: step() estimates the motion from the pair processed before to this one from the chain's own stage-4 map and `keep`
    codes with the source's Odometry (made on the first frame) and leaves the ops.EgoResult in s.ego; it reads back, once, for the log."""

    def skip(self, path, log):
        log.warning("Egomotion: %s was skipped; its line of the poses file repeats the pose of the pair before it", path)

    def step(self, s, log):
        import torch
        from .egomotion import Odometry, motion_summary
        a, src = self.args, self.source
        if src.odometry is None:
            src.odometry = Odometry(s.frame.cam, levels=a.ego_levels, iters=a.ego_iters, huber=a.ego_huber, min_disp=a.min_disp)
        disp, keep = _stage4(s.res)
        with torch.cuda.device(disp.device):
            s.ego = src.odometry.step(out.rgb_on_device(s.frame.left, disp.device), disp, keep, resid=a.save_ego)
        if s.ego is not None:
            t, deg = motion_summary(s.ego.pose[0, 0].cpu().numpy())
            n, rms = s.ego.info[0, :2].cpu().tolist()
            log.info("Egomotion: t = {:.4f} m, rotation = {:.4f} deg, pixels = {}, rms = {:.3f}, status = {}".format(
                t, deg, int(n), rms, int(src.odometry.status[-1][0])))

    def save(self, s, stem, log):
        return out.save_ego(stem, s.frame, log, s.ego) if self.args.save_ego else []

    def finish(self, log):
        from .geometry import write_kitti_poses
        path = self.args.save_poses
        if path is not None:
            write_kitti_poses(path, self.source.lines())
            log.info("Save poses = {}".format(path))
        return [] if path is None else [path]


class _Tracker(_Stage):
    """--tsdf_track: step() refines the frame's ego-motion estimate against the volume stage's TsdfVolume with the source's
    ModelTracker (made on the first frame) and leaves the ops.TrackResult in s.track; it reads back, once, for the log.  The volume
    holds the frames before this one, integrated at their tracked poses: the volume stage runs after this one."""
    volume = None                                           # the volume stage's TsdfVolume: begin() hands it over

    def skip(self, path, log):
        log.warning("Tracking: %s was skipped; the next frame is aligned with the volume's view of the pair before it", path)

    def step(self, s, log):
        import torch
        from . import ops
        from .tracking import ModelTracker
        a, src = self.args, self.source
        disp, keep = _stage4(s.res)
        if src.tracker is None:
            src.tracker = ModelTracker(self.volume, s.frame.cam, iters=a.track_iters, lambda_g=a.track_lambda, gate_g=a.track_gate, huber_g=TRACK_HUBER_G,
                                       min_disp=a.min_disp, z_near=max(a.tsdf_voxel, 0.5))
        init = None
        if s.ego is not None and not int(s.ego.status[0]) & ops.EGO_UNTRUSTED:
            init = s.ego.pose[:, 0].contiguous()
        with torch.cuda.device(disp.device):
            s.track = src.tracker.step(out.rgb_on_device(s.frame.left, disp.device), disp, keep, init=init, resid=a.save_track)
        if s.track is not None:
            n_p, rms_p, n_g, rms_g = s.track.info[0, :4].cpu().tolist()
            log.info("Tracking: photometric pixels = {}, rms = {:.3f}, model pixels = {}, rms = {:.3f} sigma, status = {}".format(
                int(n_p), rms_p, int(n_g), rms_g, int(src.tracker.status[-1][0])))

    def save(self, s, stem, log):
        return out.save_track(stem, s.frame, log, s.track) if self.args.save_track else []


class _Movers(_Stage):
    """--movers: step() segments what moved between the pair processed before and this one, on the chain's own stage-4 map and `keep`
    codes under the source's motion, with a MoverSegmenter (made on the first frame); it leaves the ops.MoversResult in s.movers and
    its code map in the place of the stage-4 `keep` of s.res -- a run without checks gets a `keep` where there was none -- so that
    the filter and the volume behind it never take a mover.  A frame without a trusted motion is not segmented and keeps its codes.
    It reads back, once, for the log."""
    segmenter = None

    def step(self, s, log):
        import torch
        from . import ops
        from .movers import MoverSegmenter
        a = self.args
        if self.segmenter is None:
            bits = ops.MOVER_CANDIDATES | (1 << 3 if a.movers_uncovered else 0)
            self.segmenter = MoverSegmenter(s.frame.cam, gate_g=a.movers_gate, gate_p=a.movers_gate_p, radius=a.movers_radius,
                                            min_pixels=a.movers_min_pixels, grow=a.movers_grow, cand_bits=bits, min_disp=a.min_disp)
        first = self.segmenter.prev is None
        (disp, keep), pose = _stage4(s.res), self.source.relative(s, log, warn=False)
        with torch.cuda.device(disp.device):
            s.movers = self.segmenter.step(out.rgb_on_device(s.frame.left, disp.device), disp, pose, mask=keep)
        if s.movers is None:
            if not first:
                log.warning("Movers: %s has no trusted motion from the pair before it: the frame is not segmented", s.frame.path)
            return
        log.info(out.movers_line(s.movers.info[0].cpu().tolist(), s.movers.rows[0].cpu().numpy(), s.movers.vals[0].cpu().numpy()))
        s.res = s.res.with_stage4_keep(s.movers.mask)

    def save(self, s, stem, log):
        return out.save_movers(stem, s.frame, log, s.movers) if self.args.save_movers else []


class _Sequence(_Stage):
    """--temporal: step() fuses one frame's stage-4 map under the chain's `keep` codes and puts the fused map in the chain's place:
    later stages and writers get s.res, whose stage-4 `keep` (where there is one) is 1 where the filter left a value."""
    filter = None

    def step(self, s, log):
        import torch
        from .models import DisparityTensor
        from .temporal import TemporalFilter
        a, sigma0 = self.args, temporal_sigma(self.args)
        if self.filter is None:
            self.filter = TemporalFilter(s.frame.cam, gate=a.temporal_gate, q=a.temporal_q, sigma0=0.5 if sigma0 is None else sigma0,
                                         hold=a.temporal_hold, min_disp=a.min_disp)
        (disp, keep), pose = _stage4(s.res), self.source.relative(s, log)
        with torch.cuda.device(disp.device):
            s.fused = self.filter.step(disp, pose, sigma=s.conf.sigma[2] if sigma0 is None else None, mask=keep)
        log.info("Temporal: " + ", ".join("{} = {}".format(n, c) for n, c in zip(out.TEMPORAL_CODES, s.fused.counts[0].cpu().tolist())))
        s.res = s.res.with_stage4(DisparityTensor.wrap(s.fused.disp), None if keep is None else (s.fused.code != 0).to(torch.uint8))


class _Volume(_Stage):
    """--tsdf: step() integrates one frame's stage-4 map (with --temporal the fused map and its sigma) under the `keep` codes, at the
    source's pose expressed in the frame of the first camera integrated; with --save_tsdf it leaves that pose's ray-cast in s.view."""
    first = None

    def __init__(self, args, source, device, log):
        import torch
        from .tsdf import MeshChunks, TsdfVolume, volume_bytes
        super().__init__(args, source)
        origin, dims = tsdf_grid(args)
        need, free = volume_bytes(dims, colour=True), torch.cuda.mem_get_info(device)[0]
        if need > free:
            raise RuntimeError(f"--tsdf: a volume of {dims[0]} x {dims[1]} x {dims[2]} voxels takes {need} bytes, the device has {free} free "
                               "(a larger --tsdf_voxel or a smaller --tsdf_extent)")
        self.volume = TsdfVolume(origin, args.tsdf_voxel, dims, mu0=args.tsdf_trunc, mu_d=args.tsdf_trunc_px, weight=args.tsdf_weight, colour=True,
                                 min_disp=args.min_disp, max_depth=args.max_depth, device=device)
        log.info("TSDF: volume {} x {} x {} voxels of {:g} m from ({:g}, {:g}, {:g}), {} bytes".format(*dims, args.tsdf_voxel, *origin, need))
        # --tsdf_follow: the volume's centre in the first camera's frame is what the volume keeps near its centre, so the first frame
        # never moves it; the chunks that left wait on the host for finish()
        self.anchor, self.chunks = self.volume.centre(), MeshChunks()
        self.spill = "mesh" if args.save_tsdf_mesh is not None else "points" if args.save_tsdf_ply is not None else None

    def step(self, s, log):
        import torch
        from . import ops
        a, frame = self.args, s.frame
        pose = np.vstack([self.source.world(), [0.0, 0.0, 0.0, 1.0]])
        if self.first is None:
            self.first = pose
        pose = np.linalg.solve(self.first, pose)[:3]        # camera -> the first camera integrated
        disp, keep = _stage4(s.res)
        keep = out.merge_keep(keep, frame.valid_left)
        with torch.cuda.device(disp.device):
            if a.tsdf_follow is not None:
                self.follow(pose, log)
            kw = dict(mask=keep, min_disp=a.min_disp, max_depth=a.max_depth, max_jump=a.max_jump)
            normals = ops.surface_normals(disp, frame.cam, **kw)[0] if a.tsdf_sdf == "plane" else None
            sigma = None if s.fused is None else torch.sqrt(s.fused.var)
            updated = self.volume.integrate(disp, frame.cam, pose, sigma=sigma, mask=keep, normals=normals,
                                            rgb=out.rgb_on_device(frame.left, disp.device))
            log.info("TSDF: voxels updated = {}".format(int(updated[0])))
            if a.save_tsdf:
                s.view = self.volume.raycast(frame.cam, pose, *disp.shape[2:], z_near=max(a.tsdf_voxel, 0.5), weight=False, normals=False)

    def follow(self, pose, log):
        """--tsdf_follow, before a frame is integrated at `pose` (camera -> the first camera): moves the volume once the anchor is N
        voxels from its centre, keeps what the move spilled and logs the move."""
        shift, chunks = self.volume.follow(pose, self.anchor, self.args.tsdf_follow, spill=self.spill, max_points=TSDF_MAX_POINTS,
                                           max_faces=TSDF_MAX_FACES)
        if not any(shift):
            return
        for c in chunks:
            self.chunks.append(c)
        log.info("TSDF: followed by ({}, {}, {}) voxels, kept = {}, spilled vertices = {}, faces = {}".format(
            *shift, int(self.volume.kept[0]), sum(len(c.points) for c in chunks), sum(len(c.faces) for c in chunks)))

    def save(self, s, stem, log):
        return out.save_tsdf(stem, log, s.view) if s.view is not None else []

    def finish_chunks(self, log):
        """finish() with --tsdf_follow: the volume is the last chunk; the point file gets the chunks' vertices, the mesh file the same
        vertices in the same order and the faces."""
        path, mesh = self.args.save_tsdf_ply, self.args.save_tsdf_mesh
        if self.spill is not None:
            self.chunks.append(self.volume.chunk(self.spill, max_points=TSDF_MAX_POINTS, max_faces=TSDF_MAX_FACES))
            pts = np.concatenate(self.chunks.points)
            twice = len(pts) - len(np.unique(np.ascontiguousarray(pts[:, :12]).view("V12")))
            log.info("TSDF: {} chunks, vertices at a place an earlier vertex holds (the seams) = {}".format(len(self.chunks.points), twice))
        if path is not None:
            log.info("Save TSDF points = {}, vertices = {}".format(path, self.chunks.write(path, faces=False)[0]))
        if mesh is not None:
            log.info("Save TSDF mesh = {}, vertices = {}, faces = {}".format(mesh, *self.chunks.write(mesh)))
        return [f for f in (path, mesh) if f is not None]

    def finish(self, log):
        if self.args.tsdf_follow is not None:
            return self.finish_chunks(log)
        path = self.args.save_tsdf_ply
        if path is not None:
            log.info("Save TSDF points = {}, vertices = {}".format(path, self.volume.write_ply(path, max_points=TSDF_MAX_POINTS)))
        mesh = self.args.save_tsdf_mesh
        if mesh is not None:
            log.info("Save TSDF mesh = {}, vertices = {}, faces = {}".format(
                mesh, *self.volume.write_mesh_ply(mesh, max_points=TSDF_MAX_POINTS, max_faces=TSDF_MAX_FACES)))
        return [f for f in (path, mesh) if f is not None]


def begin(args, pairs, device, log, poses=None):
    """(the PoseSource, the stages that are on, in the order they run) of a run over `pairs` pairs.  poses: what the checks read;
    a namespace that skipped the checks gets the flags' defaults and its --poses file read here."""
    post.set_defaults(args, **TEMPORAL_DEFAULTS, **EGO_DEFAULTS, **TSDF_DEFAULTS, **TSDF_MESH_DEFAULTS, **TSDF_FOLLOW_DEFAULTS, **TRACK_DEFAULTS,
                      **MOVERS_DEFAULTS)
    if poses is None and args.poses is not None and not args.egomotion:
        from .geometry import read_kitti_poses
        poses = read_kitti_poses(args.poses)
    source = PoseSource(pairs, None if args.egomotion else poses)
    on = ((args.egomotion, _Odometry, ()), (args.tsdf_track, _Tracker, ()), (args.movers, _Movers, ()), (args.temporal, _Sequence, ()), (args.tsdf, _Volume, (device, log)))
    stages = tuple(cls(args, source, *more) for flag, cls, more in on if flag)
    for st in stages:
        if isinstance(st, _Tracker):
            st.volume = next(v.volume for v in stages if isinstance(v, _Volume))
    return source, stages
