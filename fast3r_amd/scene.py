"""Scene assembly and PLY export on the GPU: the last step after the forward pass, turning a prediction into a point cloud to look at
or hand on.  In the reference this is the body of `fast3r/viz/viser_visualizer.py::start_visualization` (:343-427 frame processing,
:115-165 `update_points_filtering`, :168-254 `collect_visible_points` / `safe_color_conversion` / `generate_ply_bytes`), all
single-threaded numpy; here every per-point step is a HIP kernel (fast3r_amd/csrc/f3r_scene.hip):

* `assemble_scene` -> `Scene`: per view and per head the confidence order (`np.argsort(-conf, kind='stable')`; the reference uses
  numpy's default unstable sort, of which the stable order is one valid output and the only deterministic one) and, in the same
  kernel, the four gathers and the image / confidence colourings; the per-view maximum confidence; the 20th / 80th percentile extent.
* `Scene.collect_points`: the prefix cut `num = max(1, int(total * (100 - p) / 100))`, the sky-mask compaction and the concatenation.
* `generate_ply_bytes` / `save_ply`: the reference's header and 15-byte records, packed on the device.

Deviations, all stated in DESIGN.md section 7: colours are stored as uint8 (for RGB the reference's float arrays are these / 255.0 and
the round trip through `safe_color_conversion` is the identity; for the other two colourings the uint8 values are exactly what reaches
the PLY); image values outside [-1, 1] saturate where the reference's uint8 cast wraps; the sky mask is an input (`not_sky`), like
`valid_mask` elsewhere, or `not_sky="detect"` computes it as the reference does (`detect_sky_mask`: fast3r_amd/sky.py) -- the default,
None, still means no sky anywhere; `sample` selects the batch row where the reference's `squeeze()` only works at B = 1.
"""
import colorsys
import os
import struct

import numpy as np
import torch

from . import post_ops
from ._frontend import check_inputs, fp32_on, on_work_device, preds_and_views, read_back
from ._lib import work_device

TURBO_LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "turbo_lut_u8.bin")
EXTENT_PERCENTILE = 80  # viser_visualizer.py:421
PLY_RECORD_BYTES = 15
_LUT = {}


def turbo_lut_u8():
    """(256, 3) uint8 numpy array: trunc(matplotlib.cm.turbo's table * 255), shipped as data (tools/make_golden_scene.py writes and checks it)"""
    b = open(TURBO_LUT_PATH, "rb").read()
    if len(b) != 768:
        raise ValueError(f"{TURBO_LUT_PATH}: expected 768 bytes, found {len(b)}")
    return np.frombuffer(b, dtype=np.uint8).reshape(256, 3)


def _lut_on(dev):
    key = str(dev)
    if key not in _LUT:
        _LUT[key] = torch.from_numpy(turbo_lut_u8().copy()).to(dev)
    return _LUT[key]


# ------------------------------------------------------------------------------------------------------------------- host logic
def num_to_show(total, percentile):
    """viser_visualizer.py:122: how many of the sorted entries the percentile slider keeps"""
    return max(1, int(total * (100 - percentile) / 100))


def view_contributes(i, is_high_confidence, upto_timestep, show_high_conf, show_low_conf):
    """does view i contribute to the export: it is on the timeline and its confidence class is switched on"""
    return i <= upto_timestep and bool((is_high_confidence and show_high_conf) or (not is_high_confidence and show_low_conf))


def rainbow_color(i, num_frames):
    """viser_visualizer.py:380-384"""
    return colorsys.hsv_to_rgb(i / num_frames, 1.0, 1.0)


def rainbow_u8(rgb):
    """what safe_color_conversion makes of a rainbow colour (float64 in [0, 1]): trunc(c * 255)"""
    return tuple(int(np.clip(np.float64(c) * 255, 0, 255).astype(np.uint8)) for c in rgb)


def is_outdoor_scene(sky_ratios):
    """viser_visualizer.py:74-81: at least a quarter of the views with more than 20 % sky"""
    significant = sum(1 for r in sky_ratios if r > 0.2)
    return significant >= len(sky_ratios) / 4


def percentile_indexes(n, percent):
    """What np.percentile(x fp32 of length n, percent) (method 'linear') reads: (previous index, next index, gamma).  numpy divides the
    percentage by float32(100) and forms the virtual index (n - 1) * q in float32 when the data are float32; this does the same."""
    q = np.true_divide(percent, np.float32(100))
    virtual = np.asanyarray((n - 1) * q)
    previous = np.asanyarray(np.floor(virtual))
    nxt = np.asanyarray(previous + 1)
    if virtual >= n - 1:
        previous, nxt = np.asanyarray(previous.dtype.type(-1)), np.asanyarray(previous.dtype.type(-1))
    if virtual < 0:
        previous, nxt = np.asanyarray(previous.dtype.type(0)), np.asanyarray(previous.dtype.type(0))
    prev_i, next_i = previous.astype(np.intp), nxt.astype(np.intp)
    gamma = np.asanyarray(np.asanyarray(virtual - prev_i), dtype=virtual.dtype)
    return int(prev_i) % n, int(next_i) % n, gamma


def percentile_finish(previous, nxt, gamma):
    """numpy's _lerp on the two order statistics (fp32 arrays over the axes)"""
    diff = np.subtract(nxt, previous)
    out = np.asanyarray(np.add(previous, diff * gamma))
    np.subtract(nxt, diff * (1 - gamma), out=out, where=gamma >= 0.5, casting="unsafe", dtype=type(out.dtype))
    return out


def _conf_of_key(k):
    """inverse of the sort key (f3r.h f3r_scene_sort): uint32 key -> the fp32 confidence"""
    k = (~k) & 0xffffffff
    u = (k & 0x7fffffff) if k & 0x80000000 else (~k) & 0xffffffff
    return struct.unpack("<f", struct.pack("<I", u))[0]


def _double_of_key(k):
    u = (k & 0x7fffffffffffffff) if k >> 63 else (~k) & 0xffffffffffffffff
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def color_rule(lo, hi):
    """which of safe_color_conversion's three range rules applies (viser_visualizer.py:205-221)"""
    if lo >= 0 and hi <= 1:
        return 0
    if lo >= -1 and hi <= 1:
        return 1
    return 2


# ------------------------------------------------------------------------------------------------------------------- the scene
class Scene:
    """What `assemble_scene` returns.  `frames[i]` carries the reference's `frame_data` keys as device tensors; see the module text."""

    def __init__(self, frames, scene_extent, is_outdoor, global_conf_threshold):
        self.frames = frames
        self.scene_extent = scene_extent                  # (3,) fp32 numpy: percentile 80 - percentile 20 per axis
        self.max_extent = float(np.max(scene_extent))     # np.max: NaN if any
        self.is_outdoor = is_outdoor
        self.global_conf_threshold = global_conf_threshold

    @property
    def num_frames(self):
        return len(self.frames)

    def frustum_scale(self, percent=2.0):
        """viser_visualizer.py:456"""
        return self.max_extent * (percent / 100.0)

    def set_global_conf_threshold(self, value):
        """the "High/Low Conf Threshold" slider (:655-659)"""
        self.global_conf_threshold = value
        for fd in self.frames:
            fd["is_high_confidence"] = fd["max_conf_global"] >= value

    def collect_points(self, *, min_conf_thr_percentile=10, mask_sky=None, color="rgb", show_global=False, show_local=True,
                       show_high_conf=True, show_low_conf=False, upto_timestep=None):
        """The visible points and their colours, as the reference's "Download PLY" collects them: (points (M, 3) fp32, colors (M, 3)
        uint8) on the device, or (None, None) when nothing is visible.  Defaults are the reference's GUI defaults after its
        "Show High-Conf Views" handler has run; mask_sky=None means `is_outdoor`."""
        if not 0 <= min_conf_thr_percentile <= 100:
            raise ValueError(f"collect_points: min_conf_thr_percentile = {min_conf_thr_percentile} outside [0, 100]")
        if color not in ("rgb", "confidence", "rainbow"):
            raise ValueError(f"collect_points: color must be 'rgb', 'confidence' or 'rainbow', got {color!r}")
        if mask_sky is None:
            mask_sky = self.is_outdoor
        if upto_timestep is None:
            upto_timestep = len(self.frames) - 1
        pts, cols, masks, nums, consts = [], [], [], [], []
        for i, fd in enumerate(self.frames):
            if not view_contributes(i, fd["is_high_confidence"], upto_timestep, show_high_conf, show_low_conf):
                continue
            for head, shown in (("global", show_global), ("local", show_local)):
                if not shown:
                    continue
                p = fd[f"sorted_pts3d_{head}"]
                pts.append(p)
                nums.append(num_to_show(p.shape[0], min_conf_thr_percentile))
                masks.append(fd[f"sorted_not_sky_{head}"] if mask_sky else None)
                if color == "rainbow":
                    cols.append(None)
                    consts.append(rainbow_u8(fd["rainbow_color"]))
                else:
                    cols.append(fd[f"colors_{color}_{head}"])
                    consts.append(None)
        if not pts:
            return None, None
        return post_ops.scene_collect(pts, cols, masks, nums, consts)

    def save_ply(self, path, **kwargs):
        """collect_points(**kwargs) -> save_ply; returns the number of points written (0: nothing visible, no file)"""
        p, c = self.collect_points(**kwargs)
        if p is None:
            return 0
        save_ply(path, p, c)
        return p.shape[0]


def assemble_scene(output_or_preds, views=None, *, sample=0, not_sky=None, global_conf_thr_value_to_drop_view=1.5, niter_PnP=100, poses=True):
    """Everything `start_visualization` prepares before it draws (viser_visualizer.py:279-282, :343-427).  Takes what `inference()` returns
    ({'preds', 'views'}, host tensors: uploaded here) or (preds, views) with device tensors; views may differ in H x W; `sample` selects
    the batch row.  `not_sky`: None (no sky anywhere), a list of per-view (H, W) bool / int8 masks, nonzero = keep (what `detect_sky_mask`
    returns), or "detect": run fast3r_amd.sky's batched detection on the images already on the device and proceed as if given those masks.
    Results stay on the device."""
    preds, views = preds_and_views(output_or_preds, views, "assemble_scene", "image colours")
    check_inputs(preds, views, sample, not_sky, what="assemble_scene")
    V = len(preds)
    dev = work_device(preds[0]["conf"], "preds")

    def mask_of(m):
        m = torch.as_tensor(m)
        if m.device != dev:
            m = m.to(dev)
        if m.dtype == torch.bool:
            m = m.view(torch.int8)   # 0 / 1 bytes as they are
        elif m.dtype != torch.int8:
            m = (m != 0).to(torch.int8)
        return m.reshape(-1)

    detect = isinstance(not_sky, str)
    conf, pts, img, mask, shapes = [], [], [], [], []
    for head in ("global", "local"):
        for i, (pred, view) in enumerate(zip(preds, views)):
            H, W = pred["conf"].shape[1:3]
            if head == "global":
                shapes.append((int(H), int(W)))
                if tuple(view["img"].shape[1:]) != (3, H, W):
                    raise ValueError(f"assemble_scene: views[{i}]['img'] is {tuple(view['img'].shape)}; expected (B, 3, {H}, {W})")
                img.append(fp32_on(view["img"][sample], dev, (3, H * W)))   # the (3, H, W) planes as stored: nothing is permuted
                mask.append(None if (not_sky is None or detect) else mask_of(not_sky[i]))
                conf.append(fp32_on(pred["conf"][sample], dev, (H * W,)))
                pts.append(fp32_on(pred["pts3d_in_other_view"][sample], dev, (H * W, 3)))
            else:
                if detect and i == 0:   # every view's planes are on the device now: one batched detection, no host synchronisation
                    from .sky import detect_sky_planes
                    mask[:V] = [m.reshape(-1) for m in detect_sky_planes(img[:V], shapes)[0]]
                img.append(img[i])
                mask.append(mask[i])
                conf.append(fp32_on(pred["conf_local"][sample], dev, (H * W,)))
                pts.append(fp32_on(pred["pts3d_local_aligned_to_global"][sample], dev, (H * W, 3)))
    out = post_ops.scene_sort(conf, pts, img, mask, _lut_on(dev))
    offs = out["offsets"] + [out["order"].shape[0]]
    n_global = offs[V]

    # the scene extent: np.percentile(all global points, 20 / 80, axis=0); the sorted global points are the same multiset, contiguous
    lo_prev, lo_next, lo_gamma = percentile_indexes(n_global, 100 - EXTENT_PERCENTILE)
    hi_prev, hi_next, hi_gamma = percentile_indexes(n_global, EXTENT_PERCENTILE)
    ranks = sorted({lo_prev, lo_next, hi_prev, hi_next})
    ranks4 = (ranks + [ranks[-1]] * 4)[:4]
    ext_dev = post_ops.scene_extent_stats(out["pts"][:n_global], ranks4)

    poses_dev = focals_dev = None
    if poses:
        from .pose import estimate_camera_poses_device
        poses_dev, focals_dev = estimate_camera_poses_device(preds, niter_PnP, "first_view_from_global_head")

    stats = out["stats"].cpu().numpy().view(np.uint32)   # one small readback: 4 words per (view, head)
    ext = ext_dev.cpu().numpy()
    vals = ext[:12].view(np.float32).reshape(3, 4)
    at = {r: vals[:, j] for j, r in enumerate(ranks4)}
    with np.errstate(invalid="ignore"):
        min_coords = percentile_finish(at[lo_prev], at[lo_next], lo_gamma)
        max_coords = percentile_finish(at[hi_prev], at[hi_next], hi_gamma)
        min_coords[ext[12:15] != 0] = np.nan   # np.percentile: a NaN in the axis gives NaN
        max_coords[ext[12:15] != 0] = np.nan
        scene_extent = max_coords - min_coords

    frames, sky_ratios = [], []
    rainbows = [rainbow_color(i, V) for i in range(V)]
    rb_dev = torch.tensor([rainbow_u8(rb) for rb in rainbows], dtype=torch.uint8).to(dev)   # one upload
    lengths = [offs[s + 1] - offs[s] for s in range(2 * V)]
    parts = {k: out[k].split(lengths) for k in ("pts", "conf", "order", "rgb", "conf_rgb", "mask")}   # views, one call per output
    for i in range(V):
        H, W = shapes[i]
        rb = rainbows[i]
        rb_i = rb_dev[i]
        fd = {}
        for head, s in (("global", i), ("local", V + i)):
            fd[f"sorted_pts3d_{head}"] = parts["pts"][s]
            fd[f"sorted_conf_{head}"] = parts["conf"][s]
            fd[f"order_{head}"] = parts["order"][s]
            fd[f"colors_rgb_{head}"] = parts["rgb"][s]
            fd[f"colors_confidence_{head}"] = parts["conf_rgb"][s]
            fd[f"colors_rainbow_{head}"] = rb_i.expand(lengths[s], 3)
            fd[f"sorted_not_sky_{head}"] = parts["mask"][s]
        kmax, _, n_nan, n_mask = (int(x) for x in stats[i])
        max_conf = float("nan") if n_nan else _conf_of_key(kmax)   # np.max: NaN if any NaN
        fd["max_conf_global"] = max_conf
        fd["is_high_confidence"] = max_conf >= global_conf_thr_value_to_drop_view
        fd["height"], fd["width"], fd["rainbow_color"] = H, W, rb
        if poses:
            fd["c2w"] = poses_dev[sample, i]
            fd["focal_length"] = focals_dev[sample, i]
        frames.append(fd)
        sky_ratios.append(1.0 - n_mask / (H * W))
    return Scene(frames, scene_extent, is_outdoor_scene(sky_ratios), global_conf_thr_value_to_drop_view)


# ------------------------------------------------------------------------------------------------------------------- PLY
def ply_header(n):
    """viser_visualizer.py:230-242"""
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n}", "property float x", "property float y", "property float z",
             "property uchar red", "property uchar green", "property uchar blue", "end_header"]
    return "\n".join(lines).encode("ascii") + b"\n"


def colors_to_uint8(colors):
    """`safe_color_conversion` (viser_visualizer.py:205-226) on the device: uint8 passes through; float32 / float64 take one of the three
    range rules, evaluated in the input's own dtype.  ValueError where the reference would divide by zero (rule 3 on a constant input)
    or meets a NaN."""
    if colors.dtype == torch.uint8:
        return colors
    if colors.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"generate_ply_bytes: colors must be uint8, float32 or float64, got {colors.dtype}")
    kmin, kmax, n_nan = (int(x) & 0xffffffffffffffff for x in post_ops.color_range(colors).cpu().tolist())
    if n_nan:
        raise ValueError("generate_ply_bytes: colors contain NaN")
    lo, hi = _double_of_key(kmin), _double_of_key(kmax)
    rule = color_rule(lo, hi)
    if rule == 2 and hi == lo:
        raise ValueError(f"generate_ply_bytes: constant colors {lo} outside [-1, 1]: the reference's linear scaling divides by zero")
    return post_ops.color_to_u8(colors, rule, lo, hi)


def generate_ply_bytes(points, colors):
    """The reference's binary PLY (`generate_ply_bytes`, :228-254): its header, then 15-byte little-endian records, packed on the device
    and brought back with one copy through pinned memory.  points (M, 3); colors (M, 3) uint8 or float32 / float64; torch or numpy."""
    points, colors = (on_work_device(x, "generate_ply_bytes", name)[0] for x, name in ((points, "points"), (colors, "colors")))
    n = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or tuple(colors.shape) != (n, 3):
        raise ValueError(f"generate_ply_bytes: points (M, 3) and colors (M, 3), got {tuple(points.shape)} and {tuple(colors.shape)}")
    if colors.device != points.device:
        colors = colors.to(points.device)
    header = ply_header(n)
    if n == 0:
        return header
    rec = post_ops.ply_pack(points.to(torch.float32), colors_to_uint8(colors))
    return header + read_back(rec)


def save_ply(path, points, colors):
    with open(path, "wb") as f:
        f.write(generate_ply_bytes(points, colors))
