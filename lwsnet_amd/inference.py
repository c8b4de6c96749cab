#!/usr/bin/env python3
"""Inference CLI with the I/O contract of /root/reference/inference.py (same flags, crop rule, normalisation,
per-stage colour-mapped PNG outputs and log line), running the MI355X-native model.

    python -m lwsnet_amd.inference --left_img path/left_test.png --model checkpoint.pdparams
    python -m lwsnet_amd.inference --left_img path/left_test.png --synthetic_weights      # no checkpoint needed

Differences from the reference, all on the host side: PIL instead of cv2 (absent in this image); timing is taken
after a device synchronise and excludes the first (warm-up) call; `--vis` is accepted and ignored (no display).

`--workers N` (not in the reference; directory mode only): the reference's loop (inference.py:88-137) is one pair at a time --
decode, forward, colour-map, encode, all on one thread, which is what its published "10 FPS" measures.  With N > 0 the same
per-pair work is pipelined: N host worker PROCESSES (spawned, numpy + PIL only, no GPU) PNG-decode and crop into shared-memory
slots that are registered with HIP as pinned memory; a copy stream uploads the uint8 pixels and normalises them on the device
(lws_preprocess_rgb8: bit for bit the host transform), the forwards run through lws_pool (several batch-1 forwards in flight), a
second stream casts and colour-maps the stage-4 map on the device (lws_apply_lut8) and brings 3 bytes per pixel back into the
slot, and the same workers PNG-encode them (the processes, the slots and the one-thread scheduling loop: lwsnet_amd/pipeline.py).
The files written are byte-identical to the sequential loop's (tests/test_gpu_parity.py::test_cli_directory_pipeline_writes_identical_files);
the end-to-end rate and where the time goes are logged and returned (profiles/r06/e2e_cli.txt).

The flags below are not in the reference and run in the sequential mode only; their files are written by lwsnet_amd/outputs.py, one
writer per group of files, in the order of its write_stage.  `--lr_check` (or `--occ_check`), `--speckle` and `--wmedian` are the
post-processing chain; the order of its steps, which step fills, and which code map the median and the geometry files are given
are stated once, in the docstring of lwsnet_amd/postprocess.py.

`--lr_check TAU [--lr_fill]`: the colour files come from LWSNet.forward_lr's checked maps and each gets a grey mask `<stem>_lr.png`
beside it (consistent 255, inconsistent 0, out of the right view 128).

`--occ_check TAU [--occ_fill]`: the alternative that runs the network once -- the colour files come from LWSNet.forward_occ's
checked maps (lws_occlusion_check: the left-view map splatted into the right view with a z-buffer) and each gets a grey mask
`<stem>_occ.png` beside it (visible 255, occluded 0, out of the right view 128).

`--save_disp16`, `--save_depth`, `--save_ply` write KITTI's 16-bit disparity PNG `<stem>_disp16.png`, the 16-bit depth PNG
`<stem>_depth16.png` and a binary PLY point cloud `<stem>.ply` beside each colour file (lws_depth_maps / lws_point_cloud).  Depth and
points need a camera: `--calib` (a KITTI calibration file, or in directory mode a folder of them named after the frames) or
`--camera FX FY CX CY BASELINE` in the uncropped image's pixels; it is cropped as the images are.

`--save_normals`, `--save_mesh [--max_jump J]`: an OpenGL-convention normal map `<stem>_normals.png` and a binary PLY triangle mesh
`<stem>_mesh.ply` (the vertices of `<stem>.ply` with their normals, two triangles per grid cell) beside each colour file
(lws_surface_normals / lws_surface_mesh).  Two neighbouring pixels belong to one surface when their disparities differ by <= J
(default 1), so no triangle spans a depth discontinuity.  Both need a camera and the sequential mode, as `--save_ply` does, and keep
the pixels it keeps.

`--ground [--ground_tol M] [--max_height M] [--save_ground]`: the road under each map, on the device (lwsnet_amd.ops.ground: lws_vdisparity,
lws_ground_fit, lws_ground_classify, lws_bev_grid) -- one log line with the fit's status, the camera's height over the road, its pitch
and roll, the share of inliers and the pixels per code (invalid, ground, obstacle, overhead, below, no plane).  `--save_ground` also
writes `<stem>_ground.png`, the codes through a fixed six-colour table averaged with the left image's grey, and `<stem>_bev.png`, the
largest obstacle height per 0.2 m cell of a grid 40 m wide and 60 m deep as rint(min(h / max_height, 1) * 255), row 0 the farthest.
Both need a camera and the sequential mode, as `--save_ply` does, and take the code map it takes.

`--stixels [--stixel_width N] [--stixel_layers N] [--save_stixels]`: the stixel world of each map, on the device (lwsnet_amd.ops.stixels:
lws_stixels on the codes and heights of `--ground`, which it implies) -- per strip of N columns (default 8) and per layer (default 2,
nearest first) the obstacle that stands there; one log line with the number of stixels and the nearest one's depth z and lateral
position X.  `--save_stixels` also writes `<stem>_stixels.png`, the left image's grey with each stixel's rectangle tinted by a fixed
depth ramp (near red, far blue, 60 m and beyond the same), and `<stem>_stixels.csv`, one line per stixel:
strip,layer,x0,x1,y_top,y_base,n,disparity,z,x,height.  Camera and mode as for `--ground`.

`--objects [--object_min_pixels N] [--save_objects]`: the obstacle objects of each map, on the device (lwsnet_amd.ops.objects: lws_objects
on the codes of `--ground` and the u-disparity histogram of `--stixels`, which it implies) -- the connected cells of that histogram
that hold at least a strip's row of pixels, each pixel mapped back to its cell's object, objects of fewer than N pixels (default 64)
dropped; one log line with the number of objects, components and member pixels and the nearest object's depth z, lateral extent and
size.  `--save_objects` also writes `<stem>_objects.png`, the left image's grey with each object's pixels tinted with a fixed palette
colour by its number and its pixel box outlined, and `<stem>_objects.csv`, one line per object, nearest first:
object,n,x_min,x_max,y_min,y_max,k_min,k_max,cells,disparity,z,X_min,X_max,Y_min,Y_max,Z_min,Z_max.  Camera and mode as for `--ground`.

`--speckle SIZE [--speckle_diff D] [--speckle_fill]`: the connected blobs of at most SIZE pixels (4-neighbours joined when their
disparities differ by <= D, default 1) are removed from the stage maps on the device (lws_speckle_filter) before the colour, 16-bit
and point-cloud files are written, and each colour file gets a grey code map `<stem>_sp.png` beside it (kept 255, speckle 64, the
left-right check's 0 / 128 where it dropped the pixel).

`--wmedian R [--wmedian_sigma S] [--wmedian_fill N]`: the stage maps go through the edge-aware weighted median filter
(lws_wmedian_filter: a (2R + 1)^2 window, R in 1..3, weights rint(4096 exp(-s / 3S)) of the colour distance s to the window's centre
in the cropped left image; S = 0: the unweighted median, no guide) as the last step before the colour, 16-bit and point-cloud files
are made.  No code map is written: the `_lr` / `_sp` files are what they were.

`--rectify PATH [--save_rect]`: the inputs are RAW pairs -- a camera driver's frames,
KITTI's unsynced "extract" recordings -- and PATH is the rig's calibration, a KITTI raw `calib_cam_to_cam.txt` with S_, K_, D_,
R_rect_, P_rect_ and S_rect_ lines (or, in directory mode, a folder of such files named after the frames, as for `--calib`).  Both
images are undistorted, rectified and normalised on the device in one launch (lws_rectify_pair), which computes only the
bottom-right 368 x 1232 window of the rectified frame: its float planes feed the forward directly, its left uint8 image is the guide
of `--wmedian` and the colour of `--save_ply`, and the pixels whose taps fall outside the raw left image are dropped from the depth
and point-cloud files (code 2 in the mask they are given).  A frame whose size is not the calibration's S_xx is an error for that
frame (logged, nothing written); a rectified frame smaller than the crop is skipped, by the reference's rule.  Without `--calib` /
`--camera` the geometry outputs use the calibration's own rectified left camera.  `--save_rect` writes the two rectified crops as
`<left stem>_rect_left.png` and `<left stem>_rect_right.png` into the output folder.

`--save_conf [--sigma_max MAX]`, `--conf_min C`, `--sigma_max_keep S`: the forward is LWSNet.forward_conf, which also returns each volume
stage's confidence (the probability mass its soft-argmin puts within one hypothesis step of the disparity) and sigma (the standard
deviation of that distribution in pixels).  `--save_conf` writes the finest stage's (stage 3's) two maps as 8-bit grey files, two per
pair, beside the colour file (with `--left_img` beside `3.png`): `<stem>_conf.png` = rint(clip(conf, 0, 1) * 255) and `<stem>_sigma.png` = rint(min(sigma, MAX) * 255 / MAX), MAX = 8 px by
default.  `--conf_min C` and `--sigma_max_keep S` keep a pixel in the `_disp16`, `_depth16`, `.ply`, `_normals` and `_mesh.ply` files only where its stage's
conf >= C and sigma <= S (ops.confidence_codes; stage 4, the refined map, goes by stage 3's), on top of what the speckle filter's
codes drop.  They are not part of the post-processing chain, and not available with `--lr_check`, `--occ_check` or `--workers`.

`--photometric [--photo_alpha A] [--save_photo]`: every frame's four final maps are scored without ground truth by the photometric
reprojection error (lws_photometric: the right crop warped into the left view with the map against the left crop, A * DSSIM +
(1 - A) * L1, A = 0.85 by default), and one log line per frame gives the four stages' mean error and the density of scored pixels.
Only the pixels the chain's codes keep are scored, under the rule of the geometry files (the codes count while nothing has been
filled); with `--rectify` the left valid map merges into those codes as it does for the geometry files, and a right tap outside the
right valid map cannot be used.  `--save_photo` writes two files beside each colour file: `<stem>_pe.png`, the error map as 8-bit
grey rint(pe * 255) (0 where the pixel is not scored), and `<stem>_warp.png`, the warped right image.

`--temporal --poses PATH [--temporal_gate G] [--temporal_q Q] [--temporal_sigma S|net] [--temporal_hold] [--save_temporal]`: directory
mode only; the frames are a sequence in sorted order and line i of PATH (a KITTI odometry `poses.txt`: 12 numbers, camera-to-world) is
the pose of pair i; fewer lines than pairs is an error.  The stage-4 map of each frame goes through lwsnet_amd.temporal.TemporalFilter
(lws_temporal_step) behind the post-processing chain, with the chain's `keep` codes as the filter's mask, so `--temporal_hold` fills
what the checks dropped with what earlier frames saw; the fused map is what the colour file and every geometry or ground step
receive.  The measurement's sigma is the constant S px (default 0.5) or, with `net`, LWSNet.forward_conf's stage-3 sigma.  One log
line per frame gives the pixels per code (nothing, new, fused, reset, held).  `--save_temporal` writes `<stem>_tcode.png`, the codes
through a fixed five-colour table, and `<stem>_tsigma.png`, sqrt of the fused variance scaled as `--save_conf`'s sigma image.  Needs a
camera; the poses are taken as the left camera's.

`--egomotion [--ego_levels N] [--ego_iters N] [--ego_huber K] [--save_poses PATH] [--save_ego]`: directory mode only, sequential, needs
a camera; the frames are a sequence in sorted order.  The motion of the left camera from each frame to the next is estimated by dense
direct alignment (lwsnet_amd.egomotion.Odometry, lws_egomotion) from the previous frame's left crop, the chain's own stage-4 map and
`keep` codes of that frame (not a fused state) and the current left crop.  One log line per frame gives the translation in metres, the
rotation in degrees, the pixels used, the rms residual in grey levels and the status bits.  `--save_poses PATH` writes the accumulated
camera-to-world poses as a KITTI odometry `poses.txt` (line 0 the identity); `--save_ego` writes `<stem>_ego.png`, the magnitude of
the residual at the final pose as 8-bit grey (all 0 for the first frame): what does not move with the scene shows there.  A pair that
is skipped keeps its line of the poses file (line i belongs to pair i): it repeats the pose before it, with a warning, and the next
estimate spans the gap.  The op reads nothing back; the CLI reads the estimate's pose, info and status back once per frame.  With
`--temporal`, the filter takes its pose from the estimate and `--poses` may not be given; an estimate whose status says it is not to
be trusted (bit 3) resets the filter for that frame, with a warning.

`--tsdf [--tsdf_voxel V] [--tsdf_extent X0 X1 Y0 Y1 Z0 Z1] [--tsdf_trunc MU0] [--tsdf_trunc_px MU_D] [--tsdf_weight unit|sigma]
[--tsdf_sdf plane|ray] [--save_tsdf_ply PATH] [--save_tsdf_mesh PATH] [--save_tsdf]`: directory mode only, sequential, needs a camera and the pose of every
pair, from `--poses PATH` or `--egomotion`.  The stage-4 map of each frame -- with `--temporal` the fused map and its sigma -- is
integrated behind the chain into a dense TSDF volume (lwsnet_amd.tsdf.TsdfVolume, lws_tsdf_integrate) under the chain's `keep` codes
and with the left crop's colours.  The volume's frame is the first camera integrated (y down, z forward); the extent is in metres
there, the voxel V metres wide (default 0.2 over -12.8 12.8 -3.2 3.2 0 51.2).  `plane` (the default) measures the distance to each
pixel's tangent plane, with the normals of lws_surface_normals at `--max_jump`; `ray` measures it along the ray, which starves a road
seen at a grazing angle of updates.  One log line per frame gives the voxels updated.  `--save_tsdf` writes `<stem>_tsdf.png`, the
volume ray-cast into the frame's own pose and coloured as the stage maps: the denoised model view of that frame.  At the end
`--save_tsdf_ply PATH` writes the volume's zero crossings as a PLY of vertices with normals and colours and logs their number;
`--save_tsdf_mesh PATH` writes the same vertices, in the same order, with the marching-cubes triangles between them
(lws_tsdf_mesh, include/lwsnet_tsdf_mesh.h) and logs vertices and faces.  A volume that does not fit the device's free memory is an error before the first frame.  What leaves the volume is not mapped; movers
smear unless `--movers` takes them out; the poses are taken as given.

`--tsdf_follow [N]`: needs `--tsdf`.  The volume follows the camera (lwsnet_amd.tsdf.TsdfVolume.follow, lws_tsdf_window,
include/lwsnet_tsdf_window.h): before a frame is integrated, the centre of `--tsdf_extent`, carried along with the camera, is compared
with the volume's centre, and once they are N voxels apart on some axis (default 16; at least 1 and below the smallest dimension
minus 2) the volume moves by the rounded difference, in whole voxels.  What the move loses is extracted first -- as a mesh with
`--save_tsdf_mesh`, else as points with `--save_tsdf_ply`, else it is dropped -- and kept on the host; one log line per move gives
the shift, the voxels kept and the vertices and faces spilled.  At the end the volume itself is the last chunk: `--save_tsdf_ply`
gets every chunk's vertices and `--save_tsdf_mesh` the same vertices in the same order with the faces.  Limits: a vertex on the
seam of two chunks is in both (the total is logged); a vertex normal at a chunk's border is zero, as at any volume border; what
re-enters the volume after leaving is mapped afresh, so a loop gives two surfaces; after a sharp turn the volume swings with the
view, and what lies behind the camera is spilled.  Without the flag no output changes by a byte.

`--tsdf_track [--track_iters N] [--track_lambda L] [--track_gate G] [--save_track]`: needs `--tsdf` and `--egomotion`, refused with
`--poses`.  Each frame's ego-motion estimate is refined against the volume (lwsnet_amd.tracking.ModelTracker, lws_track,
include/lwsnet_track.h): the volume is ray-cast at the previous frame's tracked pose and the frame is aligned with that view by
one joint photometric + point-to-plane cost.  While it is on, the filter, the volume and `--save_poses` get the tracked poses.  One
log line per frame gives the terms of both kinds, their rms and the status.  `--save_track` writes `<stem>_track.png`, the
point-to-plane residual in standard deviations (white 0, red / blue +-4, black: no model there).

`--movers [--movers_gate G] [--movers_gate_p P] [--movers_radius R] [--movers_min_pixels N] [--movers_grow N] [--movers_uncovered]
[--save_movers]`: needs a pose source, `--poses` or `--egomotion`.  Between tracking and the filter, each frame is compared with
the pair processed before it under the run's motion (lwsnet_amd.movers.MoverSegmenter, lws_movers, include/lwsnet_movers.h): the
pixels whose disparity or grey level disagrees with a rigid scene are grouped, a group of N pixels or more is a mover, and the movers
(grown by `--movers_grow` pixels) get code 4 in the stage-4 `keep` codes, so that `--temporal` and `--tsdf` never take them; a run
without checks gets `keep` codes where it had none.  A frame whose motion is not to be trusted is not segmented.  One log line per
frame gives the pixels per evidence code, the movers and the nearest mover's box and depth.  `--save_movers` writes
`<stem>_movers.png` (untested black, static grey, appeared red, uncovered blue, changed yellow, movers outlined in white) and
`<stem>_movers.csv`, one line per mover.  A receding mover looks like a disocclusion and is found with `--movers_uncovered` only.
"""
import argparse
import contextlib
import logging
import os
import shutil
import sys
import time
import types

import numpy as np

from . import imageio as io
from . import outputs as out
from . import pipeline
from . import postprocess as post
from . import sequence as seq
from .outputs import (STIXEL_COLOUR_DEPTH, bev_to_u8, conf_to_u8, ground_to_rgb, objects_to_csv, objects_to_rgb, photo_to_u8,  # noqa: F401
                      sigma_to_u8, stixels_to_csv, stixels_to_rgb, geometry_requested as _geometry_requested)      # these stay this module's names
from .postprocess import (add_lr_arguments, add_occ_arguments, add_speckle_arguments, add_wmedian_arguments, check_lr_arguments,
                          check_occ_arguments, check_speckle_arguments, check_wmedian_arguments)
from .sequence import (TSDF_DEFAULTS, TSDF_FOLLOW_DEFAULTS, TSDF_MESH_DEFAULTS, check_egomotion_arguments, check_temporal_arguments,  # noqa: F401
                       check_tsdf_arguments, check_tsdf_follow_arguments, check_tsdf_mesh_arguments, check_track_arguments, check_movers_arguments, list_pairs as _list_pairs, temporal_sigma, tsdf_grid)


def build_parser():
    p = argparse.ArgumentParser(description="Model Inference")        # inference.py:17-29
    p.add_argument("--max_disparity", type=int, default=192)
    p.add_argument("--img_path", type=str, default="dataset/kitti2015/testing/")
    p.add_argument("--left_img", type=str, default="")
    p.add_argument("--model", type=str, default="results/finetune/checkpoint.pdparams")
    p.add_argument("--save_path", type=str, default="results/inference")
    add_model_arguments(p)
    p.add_argument("--vis", action="store_true", default=False)
    p.add_argument("--split_bf16", action="store_true",
                   help="opt-in numerics mode of this build (not in the reference): MFMA convolutions on split-bf16 operands, "
                        "float32-level accuracy, +20-25 %% speed, not bit-identical to the default (include/lwsnet_hip.h)")
    p.add_argument("--workers", type=int, default=0,
                   help="directory mode: host worker processes for decode and encode around a pipelined GPU path (0 = the "
                        "reference's sequential loop; not in the reference)")
    p.add_argument("--gpu_workers", type=int, default=3, help="with --workers: forwards kept in flight by lws_pool")
    add_lr_arguments(p)
    add_occ_arguments(p)
    add_speckle_arguments(p)
    add_wmedian_arguments(p)
    add_geometry_arguments(p)
    add_rectify_arguments(p)
    add_conf_arguments(p)
    post.add_photometric_arguments(p, save=True)
    seq.add_sequence_arguments(p)
    return p


def add_conf_arguments(p):
    """--save_conf / --sigma_max MAX / --conf_min C / --sigma_max_keep S (not in the reference): LWSNet.forward_conf.  A command line
    without them parses to the namespace it parsed to before they existed (argparse.SUPPRESS); check_conf_arguments writes their
    defaults."""
    p.add_argument("--save_conf", action="store_true", default=argparse.SUPPRESS,
                   help="write <stem>_conf.png and <stem>_sigma.png, the finest stage's confidence and disparity sigma as 8-bit grey "
                        "maps (sequential mode only; not in the reference)")
    p.add_argument("--sigma_max", type=float, default=argparse.SUPPRESS, metavar="MAX", help="with --save_conf: the sigma, in pixels, that maps to 255 (default 8)")
    p.add_argument("--conf_min", type=float, default=argparse.SUPPRESS, metavar="C",
                   help="--save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh keep only the pixels whose confidence is >= C")
    p.add_argument("--sigma_max_keep", type=float, default=argparse.SUPPRESS, metavar="S",
                   help="--save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh keep only the pixels whose disparity sigma is <= S pixels")


def conf_requested(args):
    return bool(getattr(args, "save_conf", False)) or getattr(args, "conf_min", None) is not None or getattr(args, "sigma_max_keep", None) is not None


CONF_DEFAULTS = dict(save_conf=False, sigma_max=8.0, conf_min=None, sigma_max_keep=None)


def check_conf_arguments(p, args):
    """Rejects what the confidence outputs do not support, before any model or GPU work; sets the flags' defaults (--sigma_max: 8)."""
    sigma_max_given = getattr(args, "sigma_max", None) is not None
    post.set_defaults(args, **CONF_DEFAULTS)
    if sigma_max_given and not args.save_conf:
        p.error("--sigma_max needs --save_conf")
    post.in_range(p.error, "--sigma_max MAX", args.sigma_max, strict=True)
    for flag in ("conf_min", "sigma_max_keep"):
        v = getattr(args, flag)
        if v is not None and np.isnan(v):
            p.error(f"--{flag} must be a number, got {v}")
    if not conf_requested(args):
        return
    flags = "--save_conf / --conf_min / --sigma_max_keep"
    if args.lr_check is not None or getattr(args, "occ_check", None) is not None:
        p.error(f"{flags} use the network's own confidence and do not combine with --lr_check or --occ_check")
    post.sequential_only(p, args, flags, "run")
    if (args.conf_min is not None or args.sigma_max_keep is not None) and not _geometry_requested(args):
        p.error("--conf_min and --sigma_max_keep mask --save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh: give one of them")


class _ConfModel:
    """What the chain calls as model(left, right) when the confidence outputs are on: LWSNet.forward_conf, whose ConfResult stays
    in `last` for the files written after the chain."""

    def __init__(self, model):
        self.model, self.last = model, None

    def __call__(self, left, right):
        self.last = self.model.forward_conf(left, right)
        return self.last.preds


def add_rectify_arguments(p):
    """--rectify PATH / --save_rect (not in the reference): ops.rectify_pair in front of the forward."""
    p.add_argument("--rectify", type=str, default=None, metavar="PATH",
                   help="the inputs are raw pairs: undistort and rectify them on the device with this KITTI raw calib_cam_to_cam.txt "
                        "(in directory mode also a folder of <frame>.txt files; sequential mode only; not in the reference)")
    p.add_argument("--save_rect", action="store_true",
                   help="with --rectify: write <left stem>_rect_left.png and <left stem>_rect_right.png, the rectified crops")


def check_rectify_arguments(p, args):
    """Rejects what the rectifying front end does not support, before any model or GPU work; reads every calibration file."""
    from .geometry import RectifyCalib
    if args.rectify is None:
        if args.save_rect:
            p.error("--save_rect needs --rectify PATH")
        return
    post.sequential_only(p, args, "--rectify")
    _check_calibration_files(p, args, "rectify", args.rectify, RectifyCalib.from_kitti)


def add_geometry_arguments(p):
    """--calib / --camera, --min_disp / --max_depth and --save_disp16 / --save_depth / --save_ply (not in the reference)."""
    cam = p.add_mutually_exclusive_group()
    cam.add_argument("--calib", type=str, default=None, metavar="PATH",
                     help="KITTI calibration file (P_rect_02/03 or P2/P3); in directory mode also a folder of <frame>.txt files")
    cam.add_argument("--camera", type=float, nargs=5, default=None, metavar=("FX", "FY", "CX", "CY", "BASELINE"),
                     help="camera in the uncropped image's pixels, baseline in metres")
    p.add_argument("--min_disp", type=float, default=1.0, help="depth and points: smallest disparity kept (pixels)")
    p.add_argument("--max_depth", type=float, default=float("inf"), help="depth and points: largest depth kept (metres)")
    p.add_argument("--save_disp16", action="store_true", help="write <stem>_disp16.png, KITTI's 16-bit disparity PNG (d * 256)")
    p.add_argument("--save_depth", action="store_true", help="write <stem>_depth16.png, a 16-bit depth PNG (metres * 256); needs a camera")
    p.add_argument("--save_ply", action="store_true", help="write <stem>.ply, a binary point cloud of the kept pixels; needs a camera")
    # a command line without the next three parses to the namespace it parsed to before they existed; check_geometry_arguments
    # writes their defaults
    p.add_argument("--save_normals", action="store_true", default=argparse.SUPPRESS,
                   help="write <stem>_normals.png, the surface normals of the kept pixels as an OpenGL-convention normal map; needs a camera")
    p.add_argument("--save_mesh", action="store_true", default=argparse.SUPPRESS,
                   help="write <stem>_mesh.ply, a binary triangle mesh of the kept pixels with vertex normals; needs a camera")
    p.add_argument("--max_jump", type=float, default=argparse.SUPPRESS, metavar="J",
                   help="normals and mesh: the largest disparity step between two neighbouring pixels of one surface (default 1)")
    # the ground flags likewise
    p.add_argument("--ground", action="store_true", default=argparse.SUPPRESS,
                   help="fit the road's plane and log camera height, pitch, roll and the pixels per code for each map; needs a camera")
    p.add_argument("--save_ground", action="store_true", default=argparse.SUPPRESS,
                   help="--ground, and write <stem>_ground.png (the codes in colour over the left image's grey) and <stem>_bev.png (the "
                        "obstacles' heights seen from above)")
    p.add_argument("--ground_tol", type=float, default=argparse.SUPPRESS, metavar="M",
                   help="ground: a pixel within M metres of the plane is road (default 0.2)")
    p.add_argument("--max_height", type=float, default=argparse.SUPPRESS, metavar="M",
                   help="ground: a pixel up to M metres above the road is an obstacle, above that overhead (default 3)")
    # the stixel flags likewise
    p.add_argument("--stixels", action="store_true", default=argparse.SUPPRESS,
                   help="--ground, and log the number of stixels (obstacles per column strip) and the nearest one's depth and lateral position")
    p.add_argument("--save_stixels", action="store_true", default=argparse.SUPPRESS,
                   help="--stixels, and write <stem>_stixels.png (the stixels tinted by depth over the left image's grey) and <stem>_stixels.csv")
    p.add_argument("--stixel_width", type=int, default=argparse.SUPPRESS, metavar="N", help="stixels: columns per strip, 1 .. 64 (default 8)")
    p.add_argument("--stixel_layers", type=int, default=argparse.SUPPRESS, metavar="N", help="stixels: obstacles per strip, nearest first, 1 .. 4 (default 2)")
    # the object flags likewise
    p.add_argument("--objects", action="store_true", default=argparse.SUPPRESS,
                   help="--stixels, and log the number of objects (connected obstacles in strip and disparity) and the nearest one's depth, lateral "
                        "extent and size")
    p.add_argument("--save_objects", action="store_true", default=argparse.SUPPRESS,
                   help="--objects, and write <stem>_objects.png (each object's pixels tinted and its box outlined over the left image's grey) and "
                        "<stem>_objects.csv")
    p.add_argument("--object_min_pixels", type=int, default=argparse.SUPPRESS, metavar="N", help="objects: the fewest pixels of an object (default 64)")


def _frame_file(path, left_path):
    """The calibration file of a frame: `path` itself, or for a folder the KITTI naming 000123_10.png -> 000123.txt."""
    if not os.path.isdir(path):
        return path
    return os.path.join(path, os.path.splitext(os.path.basename(left_path))[0].split("_")[0] + ".txt")


def _geometry_defaults(args):
    """The surface, stixel, ground and object flags' defaults, in the order in which the log's argument lines have shown them;
    --save_objects implies --objects, both and --save_stixels imply --stixels, and those and --save_ground imply --ground."""
    post.set_defaults(args, save_normals=False, save_mesh=False, max_jump=1.0, save_ground=False, save_stixels=False, stixels=False,
                      stixel_width=8, stixel_layers=2, ground=False, ground_tol=0.2, max_height=3.0, save_objects=False, objects=False,
                      object_min_pixels=64)
    args.objects = args.objects or args.save_objects
    args.stixels = args.stixels or args.save_stixels or args.objects
    args.ground = args.ground or args.save_ground or args.stixels


def _check_calibration_files(p, args, flag, path, read):
    """--calib / --rectify PATH: a parser error unless `read` reads the file or, for a folder, the file of every frame."""
    paths = [path]
    if os.path.isdir(path):
        if args.left_img:
            p.error(f"--{flag}: a folder of calibration files needs directory mode (--img_path); give a file with --left_img")
        paths = [_frame_file(path, li) for li in _list_pairs(args)[0]]
    for f in paths:
        try:
            read(f)
        except (OSError, ValueError) as e:
            p.error(f"--{flag}: cannot read {f}: {e}")


def check_geometry_arguments(p, args):
    """Rejects what the geometry outputs do not support, before any model or GPU work; reads every calibration file."""
    from .geometry import Camera
    _geometry_defaults(args)
    surface = args.save_normals or args.save_mesh
    outputs = args.save_disp16 or args.save_depth or args.save_ply or surface
    if not (np.isfinite(args.ground_tol) and np.isfinite(args.max_height) and 0 <= args.ground_tol <= args.max_height):
        p.error(f"--ground_tol and --max_height must be finite with 0 <= ground_tol <= max_height, got {args.ground_tol} and {args.max_height}")
    post.in_range(p.error, "--max_jump", args.max_jump)
    post.in_range(p.error, "--min_disp", args.min_disp, strict=True)
    if not args.max_depth > 0:
        p.error(f"--max_depth must be > 0, got {args.max_depth}")
    if args.save_depth or args.save_ply or surface:
        post.needs_camera(p, args, "--save_depth, --save_ply, --save_normals and --save_mesh")
    post.in_range(p.error, "--stixel_width", args.stixel_width, 1, 64)
    post.in_range(p.error, "--stixel_layers", args.stixel_layers, 1, 4)
    if args.object_min_pixels < 1:
        p.error(f"--object_min_pixels must be >= 1, got {args.object_min_pixels}")
    for name in ("objects", "stixels", "ground"):
        if getattr(args, name):
            post.needs_camera(p, args, f"--{name} and --save_{name}")
            post.sequential_only(p, args, f"--{name} / --save_{name}", "run")
    if outputs:
        post.sequential_only(p, args, "--save_disp16 / --save_depth / --save_ply / --save_normals / --save_mesh", "run")
    if args.camera is not None:
        try:
            Camera(*args.camera).check()
        except ValueError as e:
            p.error(f"--camera: {e}")
    if args.calib is not None:
        _check_calibration_files(p, args, "calib", args.calib, Camera.from_kitti)


def add_model_arguments(p):
    """The model's shape flags, --gpu_id and --synthetic_weights (shared with lwsnet_amd.evaluate; --model is per CLI)."""
    p.add_argument("--maxdisplist", type=int, nargs="+", default=[24, 5, 5])
    p.add_argument("--channels_3d", type=int, default=8)
    p.add_argument("--layers_3d", type=int, default=4)
    p.add_argument("--growth_rate", type=int, nargs="+", default=[4, 1, 1])
    p.add_argument("--gpu_id", type=int, default=0)
    p.add_argument("--synthetic_weights", action="store_true",
                   help="use the seeded synthetic weights instead of --model (the reference ships no checkpoint)")


def start_logging(name, args):
    """The CLIs' log lines on stderr, opened with one line per argument; returns the logger `name`."""
    logging.basicConfig(stream=sys.stderr, level=logging.INFO,
                        format="[%(asctime)s %(filename)s:%(lineno)s] %(levelname)s: %(message)s")
    log = logging.getLogger(name)
    for k, v in vars(args).items():
        log.info("%s: %s", k, v)
    return log


def load_model(args, log, missing_status=None):
    """LWSNet on cuda:<gpu_id> in eval mode, with the seeded synthetic weights or the checkpoint --model.  When --model names
    no file: "No model load" and SystemExit(missing_status) (inference.py:41-43 exits with None)."""
    import torch
    from .checkpoint import load_state_dict
    from .models import LWSNet
    from .weights import make_state_dict
    torch.cuda.set_device(args.gpu_id)                                  # inference.py:38
    model = LWSNet(args, device=torch.device("cuda", args.gpu_id))
    if args.synthetic_weights:
        model.set_state_dict(make_state_dict(7, args))
        log.info("Using seeded synthetic weights")
    elif not os.path.isfile(args.model):                                # inference.py:41-43
        log.info("No model load")
        raise SystemExit(missing_status)
    else:
        model.set_state_dict(load_state_dict(args.model))
        log.info("Successful load model")
    return model.eval()


def _pair_task(views, op, *paths):
    """Host worker handler of the pipelined directory mode (lwsnet_amd/pipeline.py: a spawned process, numpy and PIL only).
    views = [left, right (2,H,W,3) | colour-mapped stage-4 map (H,W,3)], uint8 RGB.  ("decode", left path, right path): PNG
    decode + crop of both images into the slot (inference.py:90-100; the normalisation of :102-103 runs on the GPU,
    lws_preprocess_rgb8); ("encode", out path): PNG of the slot's colour-mapped map (inference.py:136; the uint8 cast and the
    JET table of :114-115 run on the GPU, lws_apply_lut8).  Returns (kind, seconds spent)."""
    t0 = time.perf_counter()
    if op == "encode":
        io.save_png(paths[0], views[1])
        return "encoded", time.perf_counter() - t0
    left = io.crop_bottom_right(io.load_rgb(paths[0]))
    right = io.crop_bottom_right(io.load_rgb(paths[1]))
    if left is None or right is None:                                   # inference.py:96-97
        return "skipped", 0.0
    np.copyto(views[0][0], left)
    np.copyto(views[0][1], right)
    return "decoded", time.perf_counter() - t0


class _Slot(pipeline.Slot):
    """One pair in flight: the shared block of _pair_task, the device copies of its three images, the normalised device
    inputs [left | right], the four stage maps and the copy timing events."""

    def __init__(self, dev, H, W):
        import torch
        super().__init__([((2, H, W, 3), np.uint8), ((H, W, 3), np.uint8)], dev)
        self.dev_in = torch.empty((2, H, W, 3), dtype=torch.uint8, device=dev)
        self.dev_rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
        self.dev_lr = torch.empty((2, 3, H, W), dtype=torch.float32, device=dev)
        self.outs = [torch.empty((1, 1, H, W), dtype=torch.float32, device=dev) for _ in range(4)]
        self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]      # h2d begin / end, d2h begin / end
        self.pair, self.t0 = -1, 0.0


def inference_pipelined(model, left_imgs, right_imgs, args, log):
    """The loop of inference.py:88-137 in directory mode, pipelined (see the module docstring).  Returns (written, stats)."""
    import torch
    from . import ops
    dev = model.device
    N, P = max(1, int(args.workers)), max(1, int(args.gpu_workers))
    H, W = io.CROP_H, io.CROP_W
    total = len(left_imgs)
    torch.cuda.set_device(dev)
    lut_dev = torch.from_numpy(io.jet_lut()).to(dev)
    h2d, d2h = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    written = {}
    acc = {"decode_s": 0.0, "encode_s": 0.0, "h2d_ms": 0.0, "d2h_ms": 0.0, "pairs": 0, "skipped": 0, "latency_s": 0.0}
    nxt = decoding = 0

    def out_path(i):
        return os.path.join(args.save_path, os.path.basename(left_imgs[i]))

    def feed(sid):                                                      # a free slot takes the next pair
        nonlocal nxt, decoding
        if nxt < total:
            slots[sid].pair, slots[sid].t0 = nxt, time.perf_counter()
            host.put(sid, f"decode of pair {nxt}", "decode", left_imgs[nxt], right_imgs[nxt])
            nxt += 1
            decoding += 1

    def handle(kind, sid, seconds):
        nonlocal decoding
        sl = slots[sid]
        if kind == "decoded":
            decoding -= 1
            acc["decode_s"] += seconds
            sl.stage(0)
            with torch.cuda.stream(h2d):
                sl.ev[0].record()
                sl.dev_in.copy_(sl.pinned(0), non_blocking=True)
                ops.preprocess_rgb8(sl.dev_in, out=sl.dev_lr)               # inference.py:102-103 (ToTensor + Normalize)
                sl.ev[1].record()
                return sid, gpool.submit(sl.dev_lr[:1], sl.dev_lr[1:], out=sl.outs)    # starts behind them (after_stream = h2d)
        if kind == "skipped":
            decoding -= 1
            acc["skipped"] += 1
        else:                                                           # encoded: the slot's pair is on disk
            acc["encode_s"] += seconds
            acc["h2d_ms"] += sl.ev[0].elapsed_time(sl.ev[1])
            acc["d2h_ms"] += sl.ev[2].elapsed_time(sl.ev[3])
            acc["pairs"] += 1
            acc["latency_s"] += time.perf_counter() - sl.t0
            written[sl.pair] = out_path(sl.pair)
        feed(sid)
        return None

    def retire(item):
        sid, job = item
        sl = slots[sid]
        job.result()                                                    # the four stage maps are complete in device memory
        with torch.cuda.stream(d2h):
            sl.ev[2].record()
            ops.apply_lut8(sl.outs[3][0, 0], lut_dev, out=sl.dev_rgb)   # inference.py:114-115; directory mode keeps stage 4 (:133-137)
            sl.pinned(1).copy_(sl.dev_rgb, non_blocking=True)
            sl.ev[3].record()
        sl.ev[3].synchronize()
        sl.unstage(1)
        host.put(sid, f"encode of pair {sl.pair}", "encode", out_path(sl.pair))

    with contextlib.ExitStack() as stack:
        slots = [stack.enter_context(_Slot(dev, H, W)) for _ in range(2 * P + 2 * N)]
        host = stack.enter_context(pipeline.HostWorkers(N, _pair_task, slots))
        gpool = stack.enter_context(model.pool(workers=P))
        # warm-up outside the clock (the reference times its first call; this build never does): library, pool and workers up
        gpool.submit(slots[0].dev_lr[:1].zero_(), slots[0].dev_lr[1:].zero_(), out=slots[0].outs).result()
        torch.cuda.synchronize(dev)
        host.wait_ready()
        t_begin = time.perf_counter()
        for sid in range(len(slots)):
            feed(sid)
        for _ in pipeline.schedule(host, P, handle, retire, lambda: decoding > 0):
            pass
        wall = time.perf_counter() - t_begin
    registered = all(sl.registered for sl in slots)
    n = max(acc["pairs"], 1)
    stats = {"pairs": acc["pairs"], "skipped": acc["skipped"], "wall_s": round(wall, 4), "pairs_per_s": round(acc["pairs"] / wall, 2),
             "host_processes": N, "gpu_workers": P, "shared_memory_pinned": registered,
             "decode_ms_per_pair": round(1e3 * acc["decode_s"] / n, 3), "encode_ms_per_pair": round(1e3 * acc["encode_s"] / n, 3),
             "h2d_ms_per_pair": round(acc["h2d_ms"] / n, 3), "d2h_ms_per_pair": round(acc["d2h_ms"] / n, 3),
             "latency_ms_per_pair": round(1e3 * acc["latency_s"] / n, 2)}
    paths = [written[i] for i in sorted(written)]
    for pth in paths:
        log.info("Inference 4 stages cost = {:.3f} sec, FPS = {:.1f}\t\tSave img = {}".format(wall / n, n / wall, pth))
    log.info("pipelined: %s", stats)
    return paths, stats


def default_arguments(args):
    """The defaults that main()'s check_* calls write, in their order, for a namespace that did not go through them (build_parser()'s
    own, or one made by hand): the code below main() reads every flag as args.flag."""
    post.set_defaults(args, rectify=None, save_rect=False, **post.OCC_DEFAULTS)
    _geometry_defaults(args)
    post.set_defaults(args, **CONF_DEFAULTS)
    post.photometric_defaults(args, save=True)


def inference(model, left_imgs, right_imgs, args, log, poses=None):
    """inference.py:78-138.  poses: the file of --poses as main()'s checks read it."""
    import torch
    default_arguments(args)
    written, warm = [], False
    opts = post.Options.from_args(args)
    source, stages = seq.begin(args, min(len(left_imgs), len(right_imgs)), model.device, log, poses)
    geo = _geometry_requested(args) or bool(stages)
    conf_on = conf_requested(args) or (args.temporal and temporal_sigma(args) is None)
    chain_model = _ConfModel(model) if conf_on else model
    for index, (li, ri) in enumerate(zip(left_imgs, right_imgs)):
        frame = _load_frame(args, li, ri, model.device, geo, log)
        if frame is None:
            for st in stages:
                st.skip(li, log)
            continue
        if args.rectify is not None and args.save_rect:
            folder = os.path.dirname(args.left_img) if args.left_img else args.save_path
            written += out.save_rect(frame, os.path.join(folder, os.path.splitext(os.path.basename(frame.path))[0]), args, log)
        for _ in range(1 if warm else 2):                   # the first frame runs twice: one warm-up in all (the reference times its first call)
            torch.cuda.synchronize(model.device)
            t0 = time.time()
            guide = out.rgb_on_device(frame.left, model.device) if opts.needs_guide else None
            res = post.run_chain(chain_model, frame.l_in, frame.r_in, opts, guide)
            torch.cuda.synchronize(model.device)
            cost = time.time() - t0
        warm = True
        ss = "Inference 4 stages cost = {:.3f} sec, FPS = {:.1f}".format(cost, 1 / cost)
        if res.wmedian_counts is not None:
            for stage, (changed, refilled) in enumerate(res.wmedian_counts[:, 0].cpu().tolist()):
                log.info("Weighted median (radius {}, sigma {:g}, fill {}): stage {} changed = {}, filled = {}".format(
                    opts.wmedian, opts.wmedian_sigma, opts.wmedian_fill, stage + 1, changed, refilled))
        conf = chain_model.last if conf_on else None
        step = types.SimpleNamespace(index=index, frame=frame, res=res, conf=conf, ego=None, track=None, movers=None, fused=None, view=None)   # (lwsnet_amd/sequence.py)
        source.frame(index)
        for st in stages:                                   # ego-motion on the chain's own map and codes, the filter, the volume on what it left
            st.step(step, log)
        res = step.res
        photo = out.photometric(frame, res, args, log) if args.photometric else None
        for stage in range(4):
            disp = res.disp[stage].squeeze(axis=[0, 1]).numpy()         # :114 (the uint8 cast is inside disparity_to_color)
            color = io.disparity_to_color(disp)
            if args.left_img:                                           # :117-122
                written += out.write_stage(os.path.join(os.path.dirname(args.left_img), str(stage + 1) + ".png"), color, ss, frame, stage, args, log, res, conf, photo)
        if not args.left_img:                                           # :133-137 (stage-4 map only)
            path = os.path.join(args.save_path, os.path.basename(frame.path))
            written += out.write_stage(path, color, ss, frame, 3, args, log, res, conf, photo, step.fused)
            for st in stages:
                written += st.save(step, os.path.splitext(path)[0], log)
    for st in stages:
        written += st.finish(log)
    return written


def _load_frame(args, left_path, right_path, device, geo, log):
    """One pair decoded and cropped (inference.py:90-103) or, with --rectify, rectified on the device, as the Frame of
    lwsnet_amd/outputs.py; None when the frame is skipped (:96-97).  geo: a geometry output is on, so the frame needs its camera."""
    full = io.load_rgb(left_path)
    if args.rectify is not None:
        return _rectify_frame(args, left_path, full, io.load_rgb(right_path), device, geo, log)
    left = io.crop_bottom_right(full)
    right = io.crop_bottom_right(io.load_rgb(right_path))
    if left is None or right is None:                                   # :96-97
        return None
    cam = _frame_camera(args, left_path, *full.shape[:2]) if geo else None
    return out.Frame(left_path, io.to_input(left)[None], io.to_input(right)[None], left, right, cam=cam)


def _rectify_frame(args, left_path, raw_left, raw_right, device, geo, log):
    """--rectify: one raw pair -> the Frame of its rectified crops, all on the device (network inputs, uint8 crops [1,H,W,3], valid
    maps of the two views, camera of the crop or None); None when the frame is skipped (rectified frame smaller than the crop) or in
    error (image size other than the calibration's)."""
    import torch
    from . import ops
    from .geometry import RectifyCalib
    calib = RectifyCalib.from_kitti(_frame_file(args.rectify, left_path))
    for name, img in (("left", raw_left), ("right", raw_right)):
        if tuple(img.shape[:2]) != calib.raw_hw:
            log.error("%s: the %s image is %dx%d but the calibration's raw size is %dx%d; frame not processed", left_path, name,
                      img.shape[0], img.shape[1], *calib.raw_hw)
            return None
    hr, wr = calib.rect_hw
    if hr < io.CROP_H or wr < io.CROP_W:                                # :96-97, on the rectified frame
        return None
    raws = [torch.from_numpy(np.ascontiguousarray(img)[None]).to(device) for img in (raw_left, raw_right)]
    with torch.cuda.device(device):
        r = ops.rectify_pair(raws[0], raws[1], calib.params(), (io.CROP_H, io.CROP_W), origin=(hr - io.CROP_H, wr - io.CROP_W))
    cam = (_frame_camera(args, left_path, hr, wr) or calib.camera().crop_bottom_right(hr, wr, io.CROP_H, io.CROP_W)) if geo else None
    return out.Frame(left_path, *r["input"], *r["rect"], *r["valid"], cam)


def _frame_camera(args, left_path, h, w):
    """The camera of a frame's cropped maps (None without --calib / --camera)."""
    from .geometry import Camera
    if args.calib is not None:
        cam = Camera.from_kitti(_frame_file(args.calib, left_path))
    elif args.camera is not None:
        cam = Camera(*args.camera)
    else:
        return None
    return cam.crop_bottom_right(h, w, io.CROP_H, io.CROP_W)


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    check_lr_arguments(parser, args)
    check_occ_arguments(parser, args)
    check_speckle_arguments(parser, args)
    check_wmedian_arguments(parser, args)
    check_geometry_arguments(parser, args)
    check_rectify_arguments(parser, args)
    check_conf_arguments(parser, args)
    post.check_photometric_arguments(parser, args, save=True)
    check_egomotion_arguments(parser, args)
    poses = check_temporal_arguments(parser, args)
    alone = check_tsdf_arguments(parser, args)              # the file of --poses comes from the one of the two checks that read it
    check_tsdf_mesh_arguments(parser, args)
    check_tsdf_follow_arguments(parser, args)
    check_track_arguments(parser, args)
    mine = check_movers_arguments(parser, args)
    log = start_logging("lwsnet_amd.inference", args)
    model = load_model(args, log)
    if getattr(args, "split_bf16", False):
        model.set_option("split_bf16", 7)
        log.info("split-bf16 numerics mode")
    if not args.left_img:                                               # :50-63
        lefts, rights = _list_pairs(args)
        if os.path.exists(args.save_path):
            shutil.rmtree(args.save_path)
        os.makedirs(args.save_path)
    else:                                                               # :65-70
        lefts = [args.left_img]
        rights = [os.path.join(os.path.dirname(args.left_img), "right_test.png")]
    log.info("Begin inference!")
    if args.workers > 0 and not args.left_img:
        written, stats = inference_pipelined(model, lefts, rights, args, log)
        main.last_stats = stats
    else:
        written = inference(model, lefts, rights, args, log, next((f for f in (poses, alone, mine) if f is not None), None))
    log.info("End inference!")
    return written


if __name__ == "__main__":
    main()
