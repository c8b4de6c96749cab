"""The optional outputs of the inference CLI's sequential mode (lwsnet_amd/inference.py; its docstring describes the flags): what
one pair brings to them (Frame), the rule for the code map the geometry and photometric outputs are given (merge_keep), the pure
host converters behind the files, and one writer per group of files.

The writers share one shape: writer(frame, stage, stem, args, log, <the group's device results>) writes the group's files as
`<stem><suffix>`, logs its lines and returns the paths it wrote.  write_stage runs them, in their fixed order, for one colour file.
`args` is a namespace that went through the CLI's check_* functions, or through inference.default_arguments."""
import dataclasses
import os

import numpy as np

from . import imageio as io


@dataclasses.dataclass
class Frame:
    """One pair as the outputs see it.  left, right: the uint8 crops, numpy [H,W,3] or, with --rectify, device [1,H,W,3];
    valid_left, valid_right: --rectify's valid maps of the two views; cam: the camera of the crop when a geometry file is asked for."""
    path: str                   # of the left image
    l_in: object                # the network's inputs
    r_in: object
    left: object
    right: object
    valid_left: object = None
    valid_right: object = None
    cam: object = None


def rgb_on_device(rgb, device):
    """A uint8 [H,W,3] image (numpy) or [1,H,W,3] device tensor as the [1,H,W,3] device tensor the kernels take."""
    import torch
    if isinstance(rgb, torch.Tensor):
        return rgb
    return torch.from_numpy(np.ascontiguousarray(rgb)[None]).to(device)


def _rgb_on_host(rgb):
    return rgb if isinstance(rgb, np.ndarray) else rgb[0].cpu().numpy()


def merge_keep(keep, valid_left=None, conf_low=None):
    """The code map (only code-1 pixels are kept) an output is given: the chain's `keep` (or None) with, first, code 0 where the
    confidence codes conf_low are 0 and, next, code 2 (out of view) where --rectify's valid_left is 0; a map merged into no `keep`
    is the code map itself.  The geometry files pass both, the photometric error valid_left only."""
    import torch
    for low, code in ((conf_low, 0), (valid_left, 2)):
        if low is not None:
            keep = low if keep is None else torch.where(low == 0, torch.full_like(keep, code), keep)
    return keep


# ---- the pure host converters ----
def conf_to_u8(conf):
    """[H,W] confidence -> the bytes of <stem>_conf.png: rint(clip(conf, 0, 1) * 255)."""
    return np.rint(np.clip(np.asarray(conf, np.float64), 0.0, 1.0) * 255.0).astype(np.uint8)


def sigma_to_u8(sigma, sigma_max):
    """[H,W] sigma in pixels -> the bytes of <stem>_sigma.png: rint(min(sigma, MAX) * 255 / MAX)."""
    return np.rint(np.minimum(np.asarray(sigma, np.float64), float(sigma_max)) * 255.0 / float(sigma_max)).astype(np.uint8)


def photo_to_u8(err):
    """[H,W] photometric error in [0, 1] -> the bytes of <stem>_pe.png: rint(pe * 255)."""
    return np.rint(np.asarray(err, np.float64) * 255.0).astype(np.uint8)


def _grey(rgb):
    """The grey of a uint8 RGB image under the tinted files, as uint32: (77 r + 150 g + 29 b + 128) >> 8."""
    rgb = np.asarray(rgb).astype(np.uint32)
    return (77 * rgb[..., 0] + 150 * rgb[..., 1] + 29 * rgb[..., 2] + 128) >> 8


GROUND_COLOURS = np.array([[0, 0, 0], [0, 200, 0], [255, 0, 0], [0, 128, 255], [255, 0, 255], [128, 128, 128]], np.uint8)   # by code


def ground_to_rgb(codes, left_rgb):
    """<stem>_ground.png: the colour of each pixel's code (GROUND_COLOURS: invalid black, ground green, obstacle red, overhead blue,
    below magenta, no plane grey) averaged with the left image's grey (_grey); integers throughout."""
    return ((GROUND_COLOURS[np.asarray(codes)].astype(np.uint32) + _grey(left_rgb)[..., None] + 1) >> 1).astype(np.uint8)


def bev_to_u8(hmax, max_height):
    """<stem>_bev.png: [Gz,Gx] largest heights -> rint(min(h / max_height, 1) * 255), 0 for an empty cell, row 0 the farthest."""
    h = np.asarray(hmax, np.float64)[::-1]
    with np.errstate(all="ignore"):
        v = np.where(h > 0, np.minimum(h / float(max_height), 1.0), 0.0)
    return np.rint(v * 255.0).astype(np.uint8)


STIXEL_COLOUR_DEPTH = 60.0          # metres: the far end of the depth ramp of <stem>_stixels.png


def stixels_to_rgb(rows, vals, left_rgb, width, max_depth_for_colour):
    """<stem>_stixels.png: the left image's grey (_grey) with each stixel's rectangle x0 .. x1 by y_top ..
    y_base averaged with the colour of its depth: t = min(z / max_depth_for_colour, 1), (r, g, b) = rint(255 * (1 - t, 2 min(t, 1 - t),
    t)) -- near red, far blue.  rows, vals: one image's [S,layers,4]; the layers are drawn far to near, so the nearest shows."""
    grey = _grey(left_rgb)
    out = np.repeat(grey[..., None], 3, axis=2)
    rows, vals = np.asarray(rows), np.asarray(vals, np.float64)
    W = grey.shape[1]
    for layer in range(rows.shape[1] - 1, -1, -1):
        for s in range(rows.shape[0]):
            n, y_top, y_base, _ = (int(v) for v in rows[s, layer])
            if n <= 0:
                continue
            t = min(max(vals[s, layer, 1] / float(max_depth_for_colour), 0.0), 1.0)
            colour = np.rint(255.0 * np.array([1.0 - t, 2.0 * min(t, 1.0 - t), t])).astype(np.uint32)
            x0, x1 = s * width, min((s + 1) * width, W) - 1
            out[y_top:y_base + 1, x0:x1 + 1] = (colour + grey[y_top:y_base + 1, x0:x1 + 1, None] + 1) >> 1
    return out.astype(np.uint8)


STIXEL_CSV_HEADER = "strip,layer,x0,x1,y_top,y_base,n,disparity,z,x,height"


def stixels_to_csv(rows, vals, width, W):
    """<stem>_stixels.csv as a string: STIXEL_CSV_HEADER, then one line per non-empty slot of one image's [S,layers,4] rows and vals,
    strips left to right, layers nearest first; the four values with six decimals."""
    rows, vals = np.asarray(rows), np.asarray(vals)
    lines = [STIXEL_CSV_HEADER]
    for s in range(rows.shape[0]):
        for layer in range(rows.shape[1]):
            n, y_top, y_base, _ = (int(v) for v in rows[s, layer])
            if n > 0:
                x0, x1 = s * width, min((s + 1) * width, W) - 1
                lines.append(",".join([str(v) for v in (s, layer, x0, x1, y_top, y_base, n)] + ["{:.6f}".format(float(v)) for v in vals[s, layer]]))
    return "\n".join(lines) + "\n"


# by object number, cycled: distinct hues that stay apart from the grey underneath
OBJECT_COLOURS = np.array([[230, 25, 75], [60, 180, 75], [255, 225, 25], [0, 130, 200], [245, 130, 48], [145, 30, 180], [70, 240, 240],
                           [240, 50, 230], [210, 245, 60], [250, 190, 212], [0, 128, 128], [170, 110, 40]], np.uint8)


def objects_to_rgb(rows, labels, left_rgb):
    """<stem>_objects.png: the left image's grey (_grey) with each object's pixels averaged with the colour of its number
    (OBJECT_COLOURS, cycled) and its pixel box x_min .. x_max by y_min .. y_max outlined in that colour.  rows: one image's [N,8];
    labels: its [H,W]; the boxes are drawn far to near, so the nearest shows."""
    grey = _grey(left_rgb)
    out = np.repeat(grey[..., None], 3, axis=2)
    rows, labels = np.asarray(rows), np.asarray(labels)
    colours = OBJECT_COLOURS.astype(np.uint32)
    member = labels >= 0
    out[member] = (colours[labels[member] % len(colours)] + grey[member][:, None] + 1) >> 1
    for j in range(rows.shape[0] - 1, -1, -1):
        n, x_min, x_max, y_min, y_max = (int(v) for v in rows[j, :5])
        if n <= 0:
            continue
        colour = colours[j % len(colours)]
        out[[y_min, y_max], x_min:x_max + 1] = colour
        out[y_min:y_max + 1, [x_min, x_max]] = colour
    return out.astype(np.uint8)


OBJECT_CSV_HEADER = "object,n,x_min,x_max,y_min,y_max,k_min,k_max,cells,disparity,z,X_min,X_max,Y_min,Y_max,Z_min,Z_max"


def objects_to_csv(rows, vals):
    """<stem>_objects.csv as a string: OBJECT_CSV_HEADER, then one line per non-empty slot of one image's [N,8] rows and vals, nearest
    first; the eight values with six decimals."""
    rows, vals = np.asarray(rows), np.asarray(vals)
    lines = [OBJECT_CSV_HEADER]
    for j in range(rows.shape[0]):
        if rows[j, 0] > 0:
            lines.append(",".join([str(j)] + [str(int(v)) for v in rows[j]] + ["{:.6f}".format(float(v)) for v in vals[j]]))
    return "\n".join(lines) + "\n"


# ---- the writers ----
def save_png_gray8(path, img):
    with open(path, "wb") as f:
        f.write(io.encode_png_gray(img))


def save_rect(frame, stem, args, log):
    """--save_rect: the two rectified crops as <stem>_rect_left.png and <stem>_rect_right.png."""
    for side, img in (("left", frame.left), ("right", frame.right)):
        io.save_png(f"{stem}_rect_{side}.png", img[0].cpu().numpy())
        log.info("Save rectified %s image = %s_rect_%s.png", side, stem, side)
    return [f"{stem}_rect_left.png", f"{stem}_rect_right.png"]


def save_code_mask(frame, stage, stem, args, log, masks, suffix, text, codes):
    """One stage's code map of the left-right check, the occlusion check or the speckle filter as the grey PNG <stem><suffix>;
    text: the log line, formatted with the share of the pixels of each code in `codes` and the path."""
    code = masks[stage][0, 0].cpu().numpy()
    io.save_lr_mask_png(stem + suffix, code)
    log.info(text.format(*(float((code == c).mean()) for c in codes), stem + suffix))
    return [stem + suffix]


def save_conf(frame, stage, stem, args, log, conf):
    """The finest stage's confidence and sigma of the pair (a ConfResult) as <stem>_conf.png and <stem>_sigma.png."""
    c, sigma = conf.conf[2][0, 0].cpu().numpy(), conf.sigma[2][0, 0].cpu().numpy()
    save_png_gray8(stem + "_conf.png", conf_to_u8(c))
    save_png_gray8(stem + "_sigma.png", sigma_to_u8(sigma, args.sigma_max))
    log.info("Confidence: mean = {:.4f}, sigma: median = {:.3f} px\t\tSave maps = {}_conf.png, {}_sigma.png".format(
        float(c.mean()), float(np.median(sigma)), stem, stem))
    return [stem + "_conf.png", stem + "_sigma.png"]


def _save_depth_maps(frame, stage, stem, args, log, disp, mask):
    from . import ops
    _, depth16, disp16 = ops.depth_maps(disp, frame.cam, mask, args.min_disp, args.max_depth, depth=False, depth16=args.save_depth,
                                        disp16=args.save_disp16)
    written = []
    for t, suffix in ((disp16, "_disp16.png"), (depth16, "_depth16.png")):
        if t is not None:
            io.save_png_gray16(stem + suffix, t[0, 0].cpu().numpy())
            written.append(stem + suffix)
            log.info("Save {} = {}".format(suffix[1:-4], stem + suffix))
    return written


def _save_ply(frame, stage, stem, args, log, disp, mask):
    from . import ops
    from .geometry import write_ply
    points, counts = ops.point_cloud(disp, frame.cam, mask, rgb_on_device(frame.left, disp.device), args.min_disp, args.max_depth)
    n = int(counts[0])
    write_ply(stem + ".ply", points[0, :n].cpu().numpy(), n)
    log.info("Save point cloud ({} points) = {}".format(n, stem + ".ply"))
    return [stem + ".ply"]


def _save_normals(frame, stage, stem, args, log, disp, mask):
    from . import ops
    _, n8 = ops.surface_normals(disp, frame.cam, mask, args.min_disp, args.max_depth, args.max_jump, normals=False, normals8=True)
    io.save_png(stem + "_normals.png", n8[0].cpu().numpy())
    log.info("Save normal map = {}".format(stem + "_normals.png"))
    return [stem + "_normals.png"]


def _save_mesh(frame, stage, stem, args, log, disp, mask):
    from . import ops
    from .geometry import write_mesh_ply
    mesh = ops.surface_mesh(disp, frame.cam, mask, rgb_on_device(frame.left, disp.device), args.min_disp, args.max_depth, args.max_jump)
    n, m = (int(v) for v in mesh.counts[0].cpu())
    write_mesh_ply(stem + "_mesh.ply", mesh.points[0, :n].cpu().numpy(), n, mesh.faces[0, :m].cpu().numpy(), mesh.vnormals[0, :n].cpu().numpy())
    log.info("Save mesh ({} vertices, {} faces) = {}".format(n, m, stem + "_mesh.ply"))
    return [stem + "_mesh.ply"]


def _save_ground(frame, stage, stem, args, log, disp, mask):
    """--ground: the road of one map (ops.ground) as a log line; --save_ground: <stem>_ground.png and <stem>_bev.png; --stixels: the
    stixels of the same map behind them, on this GroundResult; --objects: the objects behind those, on the stixels' histogram."""
    from . import ops
    from .geometry import GroundPlane
    res = ops.ground(disp, frame.cam, mask, args.min_disp, args.max_depth, maxdisp=args.max_disparity, ground_tol=args.ground_tol,
                     max_height=args.max_height)
    info, counts = res.info[0].cpu().tolist(), res.counts[0].cpu().tolist()
    gp = GroundPlane.from_plane(res.plane[0].cpu().numpy(), frame.cam) if info[0] == 0 else None
    pose = "height = {:.3f} m, pitch = {:.2f} deg, roll = {:.2f} deg".format(gp.height, gp.pitch_deg, gp.roll_deg) if gp else "no plane"
    valid = max(sum(counts[1:]), 1)
    log.info("Ground: status = {}, {}, inliers = {:.4f} of the valid pixels, {}".format(
        ops.GROUND_STATUS[info[0]], pose, info[4] / valid, ", ".join("{} = {}".format(n, c) for n, c in zip(ops.GROUND_CODES, counts))))
    written = []
    if args.save_ground:
        io.save_png(stem + "_ground.png", ground_to_rgb(res.codes[0, 0].cpu().numpy(), _rgb_on_host(frame.left)))
        save_png_gray8(stem + "_bev.png", bev_to_u8(res.bev_hmax[0].cpu().numpy(), args.max_height))
        written += [stem + "_ground.png", stem + "_bev.png"]
        log.info("Save ground codes = {}, bird's-eye heights = {}".format(stem + "_ground.png", stem + "_bev.png"))
    if args.stixels:
        paths, stixels = _save_stixels(frame, stage, stem, args, log, disp, res)
        written += paths
        if args.objects:
            written += _save_objects(frame, stage, stem, args, log, disp, res, stixels)
    return written


def _save_stixels(frame, stage, stem, args, log, disp, ground):
    """--stixels: the stixels of one map (ops.stixels on the codes and heights of its GroundResult) as a log line; --save_stixels:
    <stem>_stixels.png and <stem>_stixels.csv.  Returns the paths and the StixelResult (with --objects: its u-disparity histogram)."""
    from . import ops
    res = ops.stixels(disp, frame.cam, ground.codes, ground.height, args.min_disp, args.max_depth, width=args.stixel_width,
                      maxdisp=args.max_disparity, layers=args.stixel_layers, udisp=args.objects)
    rows, vals = res.rows[0].cpu().numpy(), res.vals[0].cpu().numpy()
    found = rows[..., 0] > 0
    nearest = "none"
    if found.any():
        s, layer = np.unravel_index(np.argmin(np.where(found, vals[..., 1], np.inf)), found.shape)
        nearest = "z = {:.2f} m, X = {:.2f} m".format(float(vals[s, layer, 1]), float(vals[s, layer, 2]))
    log.info("Stixels: {} in {} strips of {} columns x {} layers, nearest: {}".format(int(found.sum()), rows.shape[0], args.stixel_width,
                                                                                     rows.shape[1], nearest))
    if not args.save_stixels:
        return [], res
    io.save_png(stem + "_stixels.png", stixels_to_rgb(rows, vals, _rgb_on_host(frame.left), args.stixel_width, STIXEL_COLOUR_DEPTH))
    with open(stem + "_stixels.csv", "w", encoding="ascii", newline="") as f:
        f.write(stixels_to_csv(rows, vals, args.stixel_width, disp.shape[3]))
    log.info("Save stixels = {}, {}".format(stem + "_stixels.png", stem + "_stixels.csv"))
    return [stem + "_stixels.png", stem + "_stixels.csv"], res


def _save_objects(frame, stage, stem, args, log, disp, ground, stixels):
    """--objects: the objects of one map (ops.objects on the codes of its GroundResult and the histogram of its StixelResult) as a
    log line; --save_objects: <stem>_objects.png and <stem>_objects.csv."""
    from . import ops
    res = ops.objects(disp, frame.cam, ground.codes, stixels.udisp, args.min_disp, args.max_depth, width=args.stixel_width,
                      min_pixels=args.object_min_pixels, labels=args.save_objects)
    rows, vals, info = res.rows[0].cpu().numpy(), res.vals[0].cpu().numpy(), res.info[0].cpu().tolist()
    nearest = "none"
    if rows[0, 0] > 0:                                      # object 0 is the one whose nearest cell is nearest
        nearest = "z = {:.2f} m, X = {:.2f} .. {:.2f} m, {} pixels in {} cells".format(float(vals[0, 1]), float(vals[0, 2]), float(vals[0, 3]),
                                                                                      int(rows[0, 0]), int(rows[0, 7]))
    log.info("Objects: {} of {} components in {} cells, {} member pixels, nearest: {}".format(info[2], info[1], info[0], info[3], nearest))
    if not args.save_objects:
        return []
    io.save_png(stem + "_objects.png", objects_to_rgb(rows, res.labels[0, 0].cpu().numpy(), _rgb_on_host(frame.left)))
    with open(stem + "_objects.csv", "w", encoding="ascii", newline="") as f:
        f.write(objects_to_csv(rows, vals))
    log.info("Save objects = {}, {}".format(stem + "_objects.png", stem + "_objects.csv"))
    return [stem + "_objects.png", stem + "_objects.csv"]


# the geometry outputs in the order they are written: (the flags that ask for one, its writer); --save_ground, --stixels and
# --save_stixels imply --ground, whose writer makes their files; --objects and --save_objects imply --stixels and ride on it
GEOMETRY = ((("save_disp16", "save_depth"), _save_depth_maps), (("save_ply",), _save_ply), (("save_normals",), _save_normals),
            (("save_mesh",), _save_mesh), (("ground", "save_ground", "stixels", "save_stixels"), _save_ground))


def geometry_requested(args):
    """One of the outputs of GEOMETRY is asked for (a flag the namespace does not have yet is off)."""
    return any(getattr(args, flag, False) for flags, _ in GEOMETRY for flag in flags)


def save_geometry(frame, stage, stem, args, log, disp, mask):
    """The geometry files of one map, <stem>_disp16.png, <stem>_depth16.png, <stem>.ply, <stem>_normals.png, <stem>_mesh.ply,
    <stem>_ground.png, <stem>_bev.png, <stem>_stixels.png, <stem>_stixels.csv, <stem>_objects.png, <stem>_objects.csv; with --ground the
    road's log line, with --stixels the stixels', with --objects the objects'.  mask: the code map of merge_keep (only code-1 pixels kept) or None."""
    written = []
    for flags, writer in GEOMETRY:
        if any(getattr(args, flag) for flag in flags):
            written += writer(frame, stage, stem, args, log, disp, mask)
    return written


def photometric(frame, res, args, log):
    """--photometric: ops.photometric on the chain's four final maps of one frame, masked by the codes the geometry files keep (with
    --rectify: merged with the left valid map as for them; the right valid map is rvalid); logs the frame's line."""
    import torch

    from . import ops
    from .metrics import photometric_means
    device = res.disp[0].device
    keep = res.keep
    if keep is not None or frame.valid_left is not None:
        keep = [merge_keep(k, frame.valid_left) for k in (keep or [None] * 4)]
    with torch.cuda.device(device):
        photo = ops.photometric(list(res.disp), rgb_on_device(frame.left, device), rgb_on_device(frame.right, device),
                                mask=keep, rvalid=frame.valid_right, alpha=args.photo_alpha,
                                want_err=args.save_photo, want_warped=args.save_photo)
    H, W = res.disp[0].shape[2:]
    m = photometric_means(photo.sums, H * W)
    log.info("Photometric (alpha = {:g}): ".format(args.photo_alpha) + ", ".join(
        "Stage {} = {} (density {:.4f})".format(s + 1, "none" if e is None else "{:.4f}".format(e), d)
        for s, (e, d) in enumerate(zip(m["pe"], m["density"]))))
    return photo


def save_photo(frame, stage, stem, args, log, photo):
    """The photometric error and the warped right image of one stage, as <stem>_pe.png and <stem>_warp.png."""
    save_png_gray8(stem + "_pe.png", photo_to_u8(photo.err[stage][0, 0].cpu().numpy()))
    io.save_png(stem + "_warp.png", photo.warped[stage][0].cpu().numpy())
    log.info("Save photometric maps = {}_pe.png, {}_warp.png".format(stem, stem))
    return [stem + "_pe.png", stem + "_warp.png"]


TEMPORAL_CODES = ("nothing", "new", "fused", "reset", "held")                     # lws_temporal_step's codes 0 .. 4
TEMPORAL_COLOURS = np.array([[0, 0, 0], [0, 130, 200], [60, 180, 75], [230, 25, 75], [255, 225, 25]], np.uint8)   # by code


def temporal_to_rgb(code):
    """<stem>_tcode.png: the colour of each pixel's temporal code (TEMPORAL_COLOURS: nothing black, new blue, fused green, reset by
    the gate red, held yellow)."""
    return TEMPORAL_COLOURS[np.asarray(code)]


def save_temporal(frame, stage, stem, args, log, fused):
    """--save_temporal: the temporal filter's codes and fused sigma of one frame (an ops.TemporalResult) as <stem>_tcode.png and
    <stem>_tsigma.png = sigma_to_u8(sqrt(var), --sigma_max)."""
    io.save_png(stem + "_tcode.png", temporal_to_rgb(fused.code[0, 0].cpu().numpy()))
    save_png_gray8(stem + "_tsigma.png", sigma_to_u8(np.sqrt(fused.var[0, 0].cpu().numpy().astype(np.float64)), args.sigma_max))
    log.info("Save temporal codes = {}_tcode.png, fused sigma = {}_tsigma.png".format(stem, stem))
    return [stem + "_tcode.png", stem + "_tsigma.png"]


def ego_to_u8(resid):
    """[H,W] residual of lws_egomotion in grey levels -> the bytes of <stem>_ego.png: min(rint(|r|), 255)."""
    return np.minimum(np.rint(np.abs(np.asarray(resid, np.float64))), 255.0).astype(np.uint8)


def save_ego(stem, frame, log, ego):
    """--save_ego: <stem>_ego.png, the residual magnitude at the final pose of the frame's ops.EgoResult; all 0 for a first frame
    (ego None), which has no previous frame to align with."""
    h, w = _rgb_on_host(frame.left).shape[:2]
    save_png_gray8(stem + "_ego.png", np.zeros((h, w), np.uint8) if ego is None else ego_to_u8(ego.resid[0, 0].cpu().numpy()))
    log.info("Save ego-motion residual = {}_ego.png".format(stem))
    return [stem + "_ego.png"]


TRACK_FULL_SCALE = 4.0                                      # standard deviations at which <stem>_track.png saturates


def track_to_rgb(resid_g):
    """[H,W] point-to-plane residual of lws_track in standard deviations -> the uint8 [H,W,3] of <stem>_track.png: black where the
    pixel carried no geometric term (0), else white at a residual near 0 running to red at +TRACK_FULL_SCALE (the model lies behind
    the frame's surface along the normal) and to blue at -TRACK_FULL_SCALE."""
    r = np.asarray(resid_g, np.float64)
    t = np.clip(np.abs(r) / TRACK_FULL_SCALE, 0.0, 1.0)
    fade = np.rint(255.0 * (1.0 - t))
    full = np.full(r.shape, 255.0)
    rgb = np.stack([np.where(r > 0, full, fade), fade, np.where(r < 0, full, fade)], -1)
    return np.where((r != 0)[..., None], rgb, 0.0).astype(np.uint8)


def save_track(stem, frame, log, track):
    """--save_track: <stem>_track.png, the point-to-plane residual at the final pose of the frame's ops.TrackResult (track_to_rgb);
    all black for a first frame (track None), which has no model to align with."""
    h, w = _rgb_on_host(frame.left).shape[:2]
    io.save_png(stem + "_track.png", np.zeros((h, w, 3), np.uint8) if track is None else track_to_rgb(track.resid[0, 1].cpu().numpy()))
    log.info("Save tracking residual = {}_track.png".format(stem))
    return [stem + "_track.png"]


MOVERS_CODES = ("untested", "static", "appeared", "uncovered", "changed")          # lws_movers' evidence codes 0 .. 4
MOVERS_COLOURS = np.array([[0, 0, 0], [90, 90, 90], [230, 25, 75], [0, 130, 200], [255, 225, 25]], np.uint8)   # by code
MOVERS_OUTLINE = np.array([255, 255, 255], np.uint8)


def movers_line(info, rows, vals):
    """The log line of one frame's ops.MoversResult (info [8], rows [K,8], vals [K,2] of one image, on the host): the pixels per
    evidence code, the movers, and the box and depth of the nearest mover that has a slot."""
    text = "Movers: " + ", ".join("{} = {}".format(n, c) for n, c in zip(("tested",) + MOVERS_CODES[1:], info[:5]))
    text += ", components = {}, movers = {}, masked pixels = {}".format(info[5], info[6], info[7])
    held = np.flatnonzero(np.asarray(rows)[:, 0] > 0)
    if len(held):
        j = held[np.argmin(np.asarray(vals)[held, 1])]
        n, x0, x1, y0, y1 = (int(v) for v in rows[j][:5])
        text += ", nearest = #{} x {}..{} y {}..{} ({} px) at {:.2f} m".format(j, x0, x1, y0, y1, n, float(vals[j][1]))
    return text


def movers_to_rgb(evidence, labels):
    """<stem>_movers.png: the colour of each pixel's evidence code (MOVERS_COLOURS: untested black, static grey, appeared red,
    uncovered blue, changed yellow); a mover's pixel with a 4-neighbour that is not of the same mover (or at the image's edge) is
    drawn in MOVERS_OUTLINE."""
    rgb = MOVERS_COLOURS[np.asarray(evidence)]
    lab = np.asarray(labels)
    pad = np.pad(lab, 1, constant_values=-2)
    edge = np.zeros(lab.shape, bool)
    for dy, dx in ((0, 1), (2, 1), (1, 0), (1, 2)):
        edge |= pad[dy:dy + lab.shape[0], dx:dx + lab.shape[1]] != lab
    rgb[(lab >= 0) & edge] = MOVERS_OUTLINE
    return rgb


def save_movers(stem, frame, log, movers):
    """--save_movers: <stem>_movers.png (movers_to_rgb) and <stem>_movers.csv, one line per mover that has a slot, of the frame's
    ops.MoversResult; all black and the header alone for a frame that was not segmented (movers None)."""
    h, w = _rgb_on_host(frame.left).shape[:2]
    lines = ["mover,pixels,x_min,x_max,y_min,y_max,appeared,uncovered,changed,disparity,depth"]
    if movers is None:
        rgb = np.zeros((h, w, 3), np.uint8)
    else:
        rgb = movers_to_rgb(movers.evidence[0, 0].cpu().numpy(), movers.labels[0, 0].cpu().numpy())
        rows, vals = movers.rows[0].cpu().numpy(), movers.vals[0].cpu().numpy()
        lines += ["{},{},{:.4f},{:.4f}".format(j, ",".join(str(int(v)) for v in rows[j]), vals[j][0], vals[j][1]) for j in np.flatnonzero(rows[:, 0] > 0)]
    io.save_png(stem + "_movers.png", rgb)
    with open(stem + "_movers.csv", "w") as f:
        f.write("\n".join(lines) + "\n")
    log.info("Save movers = {}_movers.png, {}_movers.csv".format(stem, stem))
    return [stem + "_movers.png", stem + "_movers.csv"]


def save_tsdf(stem, log, view):
    """--save_tsdf: <stem>_tsdf.png, the volume ray-cast into the frame's own pose (an ops.TsdfView), coloured as the stage maps."""
    io.save_png(stem + "_tsdf.png", io.disparity_to_color(view.disp[0, 0].cpu().numpy()))
    log.info("Save TSDF view = {}_tsdf.png".format(stem))
    return [stem + "_tsdf.png"]


# the code maps beside a colour file: (the ChainResult's field, suffix, log line, the codes whose shares it gives)
CODE_MASKS = (("lr_masks", "_lr.png", "LR check: density = {:.4f}\t\tSave mask = {}", (1,)),
              ("occ_masks", "_occ.png", "Occlusion check: density = {:.4f}\t\tSave mask = {}", (1,)),
              ("speckle_masks", "_sp.png", "Speckle filter: kept = {:.4f}, removed = {:.4f}\t\tSave codes = {}", (1, 3)))


def write_stage(path, color, cost_line, frame, stage, args, log, res, conf=None, photo=None, temporal=None):
    """One colour file and everything beside it: the colour-mapped map `color` of stage `stage` to `path`, then the lr, occ and
    speckle code maps, the confidence maps, the geometry files, the photometric maps and the temporal maps that are on.  res: the
    ChainResult; conf: the ConfResult of the same forward when a confidence flag is on; photo: the result of photometric();
    temporal: the frame's ops.TemporalResult with --temporal.  Returns the paths."""
    io.save_png(path, color)
    log.info("{}\t\tSave img = {}".format(cost_line, path))
    written, stem = [path], os.path.splitext(path)[0]
    for field, suffix, text, codes in CODE_MASKS:
        if getattr(res, field) is not None:
            written += save_code_mask(frame, stage, stem, args, log, getattr(res, field), suffix, text, codes)
    if args.save_conf and (stage == 2 or not args.left_img):            # --left_img: beside 3.png, the stage they belong to
        written += save_conf(frame, stage, stem, args, log, conf)
    if geometry_requested(args):
        low = None
        if args.conf_min is not None or args.sigma_max_keep is not None:        # each map by its own stage's confidence, the refined one by stage 3's
            from . import ops
            low = ops.confidence_codes(conf.conf, conf.sigma, args.conf_min, args.sigma_max_keep, stages=(min(stage, 2),))
        keep = merge_keep(res.keep[stage] if res.keep is not None else None, frame.valid_left, low)
        written += save_geometry(frame, stage, stem, args, log, res.disp[stage], keep)
    if photo is not None and args.save_photo:
        written += save_photo(frame, stage, stem, args, log, photo)
    if temporal is not None and args.save_temporal and stage == 3:      # the filter runs on the stage-4 map
        written += save_temporal(frame, stage, stem, args, log, temporal)
    return written
