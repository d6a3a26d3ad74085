"""Map pictures on the GPU: the first things the reference's multi-view notebook (`notebooks/demo_multiview.ipynb`) shows after
`inference()` -- `plot_rgb_images`, `plot_confidence_maps`, `maybe_plot_local_depth_and_conf` -- and the dump that goes with them,
`save_pointmaps_and_camera_parameters_to_folder`.  There every map is copied to the host, normalised and colour-mapped by matplotlib and
laid out by plotly; here the maps stay on the device, one batched kernel call (fast3r_amd/csrc/f3r_maps.hip) normalises and colours all
maps of a sheet, and only finished RGBA bytes cross to the host, for PNG encoding.

* `colorize_maps(maps, cmap)`: any list of scalar fields -> RGBA8 pictures, byte for byte what `matplotlib.pylab.imsave(path, map,
  cmap=cmap)` writes: fp32 `vmin = min`, `vmax = max` (numpy's: a NaN makes the whole picture transparent), `x = (a - vmin) / (vmax -
  vmin)` (0 for a constant map) -- the subtraction in fp32, the division in fp64 by the fp64 range and rounded to fp32, as numpy 2 runs
  matplotlib's lines --, `trunc(x * 256)` with 256 -> 255, the colormap's table `* 255` truncated to bytes, alpha 255, and (0, 0, 0, 0)
  where the quotient is NaN.  tests/maps_ref.py restates it in numpy.
* The three plot functions, with the notebook's names, argument order, defaults and file names.  Where the notebook builds a plotly
  figure they return a contact sheet: one (rows Hc, cols Wc, 4) uint8 device tensor, the cell (Hc, Wc) the largest height and the
  largest width of any view, views left to right wrapping after `max_columns`, each map in the top left corner of its cell, every other
  byte 0.  The kernel writes each map straight into its cell; the per-view pictures (and the PNGs) are windows of the sheet.
* `save_pointmaps_and_camera_parameters_to_folder`: `pointmaps_and_camera_params.npz` with the notebook's seven keys.

The two tables are data files (fast3r_amd/data/turbo_lut_u8.bin and, as text, greys_lut_u8.txt; tools/make_golden_maps.py writes and checks them against
matplotlib, which nothing in this package imports).

Deviations, stated in DESIGN.md section 7 and docs/rows_f.md: a contact sheet instead of a plotly figure; `max_columns` (the notebook puts
all views in one row); `sample` selects the batch row where the notebook's `squeeze()` only works at B = 1; an image value that is NaN
reads as 0 (numpy's cast of it is undefined).
"""
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import post_ops, render
from ._frontend import fp32_on
from ._lib import F3R_MAPS_LUT, F3R_MAPS_RGB, require_gpu, work_device
from .pose import estimate_camera_poses
from .scene import turbo_lut_u8

GREYS_LUT_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "greys_lut_u8.txt")
CMAPS = {"turbo": "turbo", "Turbo": "turbo", "Greys": "Greys"}   # as the notebook writes them -> the table
NPZ_NAME = "pointmaps_and_camera_params.npz"
NPZ_KEYS = {"global_pointmaps": "pts3d_in_other_view", "global_confidence_maps": "conf", "local_pointmaps": "pts3d_local",
            "local_aligned_to_global_pointmaps": "pts3d_local_aligned_to_global", "local_confidence_maps": "conf_local"}
_LUT = {}


def grey_levels_u8(path):
    """a text file of 256 grey levels (integers in [0, 255] separated by white space, '#' starts a comment) -> (256, 3) uint8, R = G = B"""
    words = [w for line in open(path) for w in line.split("#", 1)[0].split()]
    levels = [int(w) for w in words]
    if len(levels) != 256 or any(not 0 <= v <= 255 for v in levels):
        raise ValueError(f"{path}: expected 256 grey levels in [0, 255], found {len(levels)} entries")
    return np.repeat(np.array(levels, dtype=np.uint8)[:, None], 3, axis=1)


def greys_lut_u8():
    """(256, 3) uint8 numpy array: trunc(matplotlib.cm.Greys' table * 255), shipped as a text file of grey levels, since the table is pure grey
    (tools/make_golden_maps.py writes and checks it)"""
    return grey_levels_u8(GREYS_LUT_PATH)


def cmap_table(cmap):
    """'turbo', 'Turbo' or 'Greys' -> the name of its table; ValueError for anything else"""
    if not isinstance(cmap, str) or cmap not in CMAPS:
        raise ValueError(f"cmap = {cmap!r}; accepted values are 'turbo' and 'Greys'")
    return CMAPS[cmap]


def _lut_on(dev, name):
    key = (str(dev), name)
    if key not in _LUT:
        _LUT[key] = torch.from_numpy((turbo_lut_u8() if name == "turbo" else greys_lut_u8()).copy()).to(dev)
    return _LUT[key]


# ------------------------------------------------------------------------------------------------------------------- host logic
def sheet_layout(shapes, max_columns=8, rows_per_view=1):
    """The contact sheet of views with those (H, W) shapes (None: a view without a map): -> (sheet height, sheet width, (Hc, Wc), origins)
    with origins[i][k] = (y, x), the top left corner of view i's k-th cell.  cols = min(len(shapes), max_columns); view i sits in column
    i % cols, and its k-th cell in cell row rows_per_view (i // cols) + k."""
    n, max_columns = len(shapes), int(max_columns)
    if max_columns < 1:
        raise ValueError(f"max_columns = {max_columns}; need >= 1")
    known = [s for s in shapes if s is not None]
    if n == 0 or not known:
        return 0, 0, (0, 0), [[(0, 0)] * rows_per_view for _ in range(n)]
    Hc, Wc = max(int(s[0]) for s in known), max(int(s[1]) for s in known)
    cols = min(n, max_columns)
    bands = (n + cols - 1) // cols
    origins = [[((rows_per_view * (i // cols) + k) * Hc, (i % cols) * Wc) for k in range(rows_per_view)] for i in range(n)]
    return bands * rows_per_view * Hc, cols * Wc, (Hc, Wc), origins


def title_file_name(title):
    return title.replace(" ", "_") + ".png"


def _save_pictures(sheet, windows, folder, title):
    """the windows (file name, y, x, H, W) of the device sheet, and with a title the sheet itself, as PNGs in folder: one copy to the host,
    then `render._save_png` on the bounded pool of `render_cumulative_pts3d_viz`"""
    os.makedirs(folder, exist_ok=True)
    host = sheet.cpu().numpy()
    jobs = [(np.ascontiguousarray(host[y:y + H, x:x + W]), os.path.join(folder, name)) for name, y, x, H, W in windows]
    if title:
        jobs.append((host, os.path.join(folder, title_file_name(title))))
    if not jobs:
        return
    pending = deque()
    with ThreadPoolExecutor(max_workers=min(render.PNG_WORKERS, len(jobs))) as pool:
        for array, path in jobs:
            pending.append(pool.submit(render._save_png, array, path))
            while len(pending) > 2 * render.PNG_WORKERS:
                pending.popleft().result()
        for f in pending:
            f.result()


def _preds_of(output_or_preds, key="preds"):
    return output_or_preds[key] if isinstance(output_or_preds, dict) else output_or_preds


def _row(t, sample, who, name):
    """batch row `sample` of a (B, ...) prediction"""
    if not torch.is_tensor(t):
        t = torch.as_tensor(t)
    if not 0 <= sample < t.shape[0]:
        raise ValueError(f"{who}: sample = {sample} outside [0, {t.shape[0]}) of {name}")
    return t[sample]


# ------------------------------------------------------------------------------------------------------------------- pictures
def colorize_maps(maps, cmap="turbo", *, channel=None, return_ranges=False):
    """A list of scalar maps -- (H, W) fp32 device tensors, or (H, W, C) with `channel`, read in place -- as a list of (H, W, 4) uint8
    device pictures: what `matplotlib.pylab.imsave(path, map, cmap=cmap)` writes, byte for byte (the module text).  One kernel call for
    the whole list; maps may differ in size.  cmap: 'turbo' ('Turbo') or 'Greys'.  With return_ranges also the (n, 2) fp32 device tensor of
    each map's (vmin, vmax), NaN for a map with a NaN.  CPU tensors raise F3RError; inputs are never written."""
    name = cmap_table(cmap)
    maps = list(maps)
    if not maps:
        return ([], torch.empty((0, 2), dtype=torch.float32)) if return_ranges else []
    srcs = []
    for i, m in enumerate(maps):
        if not torch.is_tensor(m):
            raise ValueError(f"colorize_maps: maps[{i}] must be a torch tensor on a ROCm device, got {type(m).__name__}")
        require_gpu(m, f"maps[{i}]")
        if m.dtype != torch.float32 or m.dim() != (2 if channel is None else 3):
            raise ValueError(f"colorize_maps: maps[{i}] must be {'(H, W)' if channel is None else '(H, W, C)'} fp32, got {tuple(m.shape)} {m.dtype}")
        if channel is not None:
            if not -m.shape[2] <= channel < m.shape[2]:
                raise ValueError(f"colorize_maps: channel = {channel} outside the {m.shape[2]} channels of maps[{i}]")
            m = m[..., channel]
        srcs.append(m)
    dsts = [torch.empty((m.shape[0], m.shape[1], 4), dtype=torch.uint8, device=m.device) for m in srcs]
    ranges = post_ops.maps_colorize(srcs, dsts, _lut_on(srcs[0].device, name), mode=F3R_MAPS_LUT)
    return (dsts, ranges) if return_ranges else dsts


def _sheet_of(rows, save_image_to_folder, title, max_columns):
    """rows: per view a list over cell rows of None or (map, table name or 'rgb', file name): the sheet, filled by one kernel call per
    table, and its files"""
    shapes = [next((tuple(c[0].shape[-2:]) for c in cells if c is not None), None) for cells in rows]
    per_view = len(rows[0]) if rows else 1
    height, width, _, origins = sheet_layout(shapes, max_columns, per_view)
    filled = [c[0] for cells in rows for c in cells if c is not None]
    if not filled:
        return torch.zeros((0, 0, 4), dtype=torch.uint8)
    dev = filled[0].device
    sheet = torch.zeros((height, width, 4), dtype=torch.uint8, device=dev)
    calls, windows = {}, []
    for i, cells in enumerate(rows):
        for k, c in enumerate(cells):
            if c is None:
                continue
            m, table, name = c
            H, W = (int(x) for x in m.shape[-2:])
            y, x = origins[i][k]
            srcs, dsts = calls.setdefault(table, ([], []))
            srcs.append(m)
            dsts.append(sheet[y:y + H, x:x + W])
            windows.append((name, y, x, H, W))
    for table, (srcs, dsts) in calls.items():
        if table == "rgb":
            post_ops.maps_colorize(srcs, dsts, mode=F3R_MAPS_RGB)
        else:
            post_ops.maps_colorize(srcs, dsts, _lut_on(dev, table), mode=F3R_MAPS_LUT)
    if save_image_to_folder:
        _save_pictures(sheet, windows, save_image_to_folder, title)
    return sheet


def plot_rgb_images(views, title="RGB Images", save_image_to_folder=None, *, max_columns=8, sample=0):
    """The notebook's `plot_rgb_images`: per view `((img + 1) * 127.5).astype(int).clip(0, 255)` -- two rounded fp32 operations,
    truncated -- with alpha 255; with `save_image_to_folder` written to `view_{i}.png`, whose pixels are those of the notebook's `imsave`.
    `views` may be the dict `inference()` returns; host tensors are uploaded.  -> the contact sheet (the module text)."""
    views = _preds_of(views, "views")
    rows = []
    for i, view in enumerate(views):
        img = _row(view["img"], sample, "plot_rgb_images", f"views[{i}]['img']")
        if img.dim() != 3 or img.shape[0] != 3:
            raise ValueError(f"plot_rgb_images: views[{i}]['img'] is {tuple(view['img'].shape)}; expected (B, 3, H, W)")
        rows.append([(fp32_on(img, work_device(img, "views"), tuple(img.shape)), "rgb", f"view_{i}.png")])
    return _sheet_of(rows, save_image_to_folder, title, max_columns)


def _scalar_cell(pred, key, sample, who, i, table, name, channel=None):
    t = _row(pred[key], sample, who, f"preds[{i}]['{key}']")
    want = 2 if channel is None else 3
    if t.dim() != want:
        raise ValueError(f"{who}: preds[{i}]['{key}'] is {tuple(pred[key].shape)}; expected (B, H, W{', 3' if channel is not None else ''})")
    t = fp32_on(t, work_device(t, "preds"), tuple(t.shape))
    return (t if channel is None else t[..., channel], table, name)


def plot_confidence_maps(preds, title="Confidence Maps", save_image_to_folder=None, *, max_columns=8, sample=0):
    """The notebook's `plot_confidence_maps`: per view the turbo picture of `conf`, each view normalised by its own minimum and maximum;
    with `save_image_to_folder` written to `view_{i}_conf.png` as `imsave(path, conf, cmap='turbo')` writes it.  `preds` may be the dict
    `inference()` returns; host tensors are uploaded.  -> the contact sheet (the module text)."""
    preds = _preds_of(preds)
    rows = [[_scalar_cell(p, "conf", sample, "plot_confidence_maps", i, "turbo", f"view_{i}_conf.png")] for i, p in enumerate(preds)]
    return _sheet_of(rows, save_image_to_folder, title, max_columns)


def maybe_plot_local_depth_and_conf(preds, title="Local Depth and Confidence Maps", save_image_to_folder=None, *, max_columns=8, sample=0):
    """The notebook's `maybe_plot_local_depth_and_conf`: per view the turbo picture of `conf_local` and, in the cell below it, the Greys
    picture of the z channel of `pts3d_local` (read in place); a view lacking either key leaves that cell empty, as the notebook skips it.
    With `save_image_to_folder`: `view_{i}_conf_local.png` and `view_{i}_depth_local.png`.  -> the contact sheet (the module text)."""
    who = "maybe_plot_local_depth_and_conf"
    preds = _preds_of(preds)
    rows = []
    for i, p in enumerate(preds):
        conf = _scalar_cell(p, "conf_local", sample, who, i, "turbo", f"view_{i}_conf_local.png") if "conf_local" in p else None
        depth = _scalar_cell(p, "pts3d_local", sample, who, i, "Greys", f"view_{i}_depth_local.png", channel=2) if "pts3d_local" in p else None
        rows.append([conf, depth])
    return _sheet_of(rows, save_image_to_folder, title, max_columns)


# ------------------------------------------------------------------------------------------------------------------- the dump
def save_pointmaps_and_camera_parameters_to_folder(preds, save_folder, niter_PnP=100, focal_length_estimation_method="individual"):
    """The notebook's function: `estimate_camera_poses` of this package, batch row 0, and `save_folder/pointmaps_and_camera_params.npz`
    with its seven arrays: the five stacked per-view maps as stored, `estimated_focals` (n,) float64 (NaN where the solve failed) and
    `estimated_poses_c2w` (n, 4, 4) float64.  `preds` may be the dict `inference()` returns.  -> the file's path."""
    preds = _preds_of(preds)
    for i, pred in enumerate(preds):
        if "pts3d_local_aligned_to_global" not in pred:
            raise KeyError(f"'pts3d_local_aligned_to_global' not in preds[{i}]: call align_local_pts3d_to_global(preds, views) first")
        for key in NPZ_KEYS.values():
            if key not in pred:
                raise KeyError(f"'{key}' not in preds[{i}]")
    poses_c2w, focals = estimate_camera_poses(preds, niter_PnP=niter_PnP, focal_length_estimation_method=focal_length_estimation_method)
    poses_c2w, focals = poses_c2w[0], focals[0]   # batch row 0, as the notebook
    arrays = {name: np.stack([torch.as_tensor(pred[key])[0].detach().cpu().numpy() for pred in preds]) for name, key in NPZ_KEYS.items()}
    arrays["estimated_focals"] = np.array([float("nan") if f is None else float(f) for f in focals], dtype=np.float64)
    arrays["estimated_poses_c2w"] = np.stack([np.asarray(p, dtype=np.float64) for p in poses_c2w])
    os.makedirs(save_folder, exist_ok=True)
    save_file = os.path.join(save_folder, NPZ_NAME)
    np.savez(save_file, **arrays)
    return save_file


__all__ = ["colorize_maps", "maybe_plot_local_depth_and_conf", "plot_confidence_maps", "plot_rgb_images",
           "save_pointmaps_and_camera_parameters_to_folder", "sheet_layout"]
