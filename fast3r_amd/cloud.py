"""Point-cloud export on the GPU: `export_combined_ply` of the reference's multi-view notebook (`notebooks/demo_multiview.ipynb`), the
sibling for points of the `as_mesh=True` branch that fast3r_amd/mesh.py took from the same notebook.  Per view `np.percentile(conf, p)`,
`conf > thr`, `((img + 1) * 127.5).astype(np.uint8).clip(0, 255)`, the views stacked; then, if the cloud has more than `max_num_points`
points, one of three ways to bound it: `np.random.choice`, Open3D's `voxel_down_sample` with a voxel size derived from the bounding box,
or Open3D's `farthest_point_down_sample`.  There all of it runs single-threaded on the host after a D2H copy of every pointmap; here it is
HIP kernels (fast3r_amd/csrc/f3r_cloud.hip) on a cloud that stays on the device.

* `export_combined_ply(preds, views, ...)`: the notebook's function, names, order and defaults.
* `combine_points(...)`: its first half alone.
* `voxel_down_sample(points, colors, voxel_size)` -> `(points, colors, counts)`: Open3D's `VoxelDownSample` arithmetic in fp64 -- index
  `floor((p - (min_bound - 0.5 voxel_size)) / voxel_size)` per axis, per voxel the sequential sum of the widened coordinates and of
  `colour / 255.0` in original index order, the mean, `trunc(mean colour * 255.0)` -- with the voxels in ascending key order (x-major).
  The colour line keeps the notebook's quirk: a voxel of k equal colours c can come out as c - 1, where `c / 255.0` summed k times,
  divided by k and multiplied by 255.0 lands just below c.
* `farthest_point_down_sample(points, num_samples, start_index=0)` -> `selected`: Open3D's `FarthestPointDownSample`.  It is O(n k) -- the
  reference's own algorithm, which its notebook comments as "may be slow" -- and is not capped.
* `downsample_cloud(points, colors, max_num_points, sampling_strategy, ...)`: the notebook's `if max_num_points is not None and
  len(all_points) > max_num_points:` block on any device cloud, for instance what `Scene.collect_points` returns.

Deviations, stated in DESIGN.md section 7 and docs/rows_f.md: image values outside [-1, 1] saturate where the notebook's uint8 cast
wraps, and NaN reads as 0; `sample` selects the batch row where the notebook's `squeeze()` only works at B = 1; the voxels come in
ascending key order (Open3D's order is its hash map's, unspecified); a voxel key has at most 63 bits and 31 per axis (Open3D's own limit is
INT_MAX cells per axis), beyond which `ValueError`; a NaN or inf coordinate raises `ValueError` (Open3D's `floor` of it is undefined
behaviour); `'uniform'` draws with `torch.randperm` on the device (the notebook draws from NumPy's global RNG: no values to pin); the file
is this project's PLY (`generate_ply_bytes`), since the notebook hands the file to `trimesh`.

Known cost: a voxel's points are added by one thread, so a voxel holding millions of points is walked serially.  The heuristic voxel size
produces this when far outliers inflate the bounding box; an explicit `voxel_size=` is the remedy.
"""
import torch

from . import post_ops
from ._frontend import check_inputs, fp32_on, preds_and_views
from ._lib import F3R_FPS_AUTO, require_gpu, work_device
from .post_ops import heuristic_voxel_size, voxel_key_bits, voxel_sort_passes  # noqa: F401  (host arithmetic, public here)
from .scene import percentile_indexes, save_ply

SAMPLING_STRATEGIES = ("uniform", "voxel", "farthest_point")


def combine_points(output_or_preds, views=None, *, pts3d_key_to_visualize="pts3d_local_aligned_to_global", conf_key_to_visualize="conf_local",
                   min_conf_thr_percentile=0, flip_axes=False, sample=0, return_offsets=False):
    """The first half of `export_combined_ply`: per view the pixels with conf > np.percentile(conf, min_conf_thr_percentile) -- strictly:
    at percentile 0 the minimum pixels drop, and a view of constant confidence keeps nothing; a view with a NaN confidence gets a NaN
    threshold and contributes nothing -- their colours trunc((img + 1.0f) * 127.5f) (two rounded fp32 operations, saturated), with
    `flip_axes` (x, y, z) -> (x, z, -y), stacked in view order then pixel order.  Takes what `inference()` returns ({'preds', 'views'}, host
    tensors: uploaded here) or (preds, views) with device tensors; views may differ in H x W.  -> (points (M, 3) fp32, colors (M, 3)
    uint8) on the device, or (None, None) when nothing is kept.  With return_offsets a third entry follows: the end offset of every view in
    the cloud (ascending Python ints; a view that keeps nothing repeats its predecessor's).  Input tensors are never written."""
    preds, views = preds_and_views(output_or_preds, views, "combine_points", "point colours")
    if not 0 <= min_conf_thr_percentile <= 100:
        raise ValueError(f"combine_points: min_conf_thr_percentile = {min_conf_thr_percentile} outside [0, 100]")
    pts_key, conf_key = pts3d_key_to_visualize, conf_key_to_visualize
    check_inputs(preds, views, sample, None, what="combine_points", keys=(pts_key, conf_key))
    dev = work_device(preds[0][conf_key], "preds")
    conf, pts, img, shapes, ranks = [], [], [], [], []
    for i, (pred, view) in enumerate(zip(preds, views)):
        H, W = (int(x) for x in pred[conf_key].shape[1:3])
        if tuple(view["img"].shape[1:]) != (3, H, W):
            raise ValueError(f"combine_points: views[{i}]['img'] is {tuple(view['img'].shape)}; expected (B, 3, {H}, {W})")
        if tuple(pred[pts_key].shape[1:]) != (H, W, 3):
            raise ValueError(f"combine_points: preds[{i}]['{pts_key}'] is {tuple(pred[pts_key].shape)}; expected (B, {H}, {W}, 3)")
        shapes.append((H, W))
        conf.append(fp32_on(pred[conf_key][sample], dev, (H * W,)))
        pts.append(fp32_on(pred[pts_key][sample], dev, (H * W, 3)))
        img.append(fp32_on(view["img"][sample], dev, (3, H * W)))   # the (3, H, W) planes as stored: nothing is permuted
        ranks.append(percentile_indexes(H * W, min_conf_thr_percentile))
    return post_ops.cloud_combine(conf, pts, img, [None] * len(pts), shapes, ranks, flip_axes=flip_axes, return_offsets=return_offsets)


def _device_cloud(points, colors, who):
    if not torch.is_tensor(points) or (colors is not None and not torch.is_tensor(colors)):
        raise ValueError(f"{who}: points and colors must be torch tensors on a ROCm device")
    require_gpu(points, "points")
    if colors is not None:
        require_gpu(colors, "colors")
    return points, colors


def voxel_down_sample(points, colors, voxel_size):
    """Open3D's `VoxelDownSample` (the module text) -> (points (M, 3) fp32, colors (M, 3) uint8, counts (M,) int32) on the device, voxels in
    ascending key order; colors may be None (then None comes back).  ValueError on NaN / inf coordinates, voxel_size <= 0, or a voxel_size
    too small for the extent (more than 63 key bits)."""
    points, colors = _device_cloud(points, colors, "voxel_down_sample")
    out = post_ops.cloud_voxel_down_sample(points, colors, voxel_size)
    return out["points"], out["colors"], out["counts"]


def farthest_point_down_sample(points, num_samples, start_index=0, *, mode=F3R_FPS_AUTO):
    """Open3D's `FarthestPointDownSample` -> `selected`, int32 (num_samples,) on the device in selection order.  d[j] = inf; far =
    start_index; num_samples times: record far; d[j] = min(d[j], |p[j] - p[far]|^2) in fp64; far = the smallest index attaining max d if
    that maximum is > 0, otherwise unchanged -- a cloud that has run out of distinct points selects the same point again.  The cost is
    O(n num_samples): the reference's own algorithm, not capped.  ValueError on non-finite input, num_samples outside [1, n] and
    start_index outside [0, n).  `mode` forces the one-workgroup or the tiled kernel (fast3r_amd._lib.F3R_FPS_*); both give the same bits."""
    points, _ = _device_cloud(points, None, "farthest_point_down_sample")
    n = points.shape[0] if points.dim() == 2 else 0
    if not 1 <= int(num_samples) <= n:
        raise ValueError(f"farthest_point_down_sample: num_samples = {num_samples} outside [1, {n}]")
    if not 0 <= int(start_index) < n:
        raise ValueError(f"farthest_point_down_sample: start_index = {start_index} outside [0, {n})")
    bad = post_ops.cloud_bounds(points)[2]
    if bad:
        raise ValueError(f"farthest_point_down_sample: {bad} coordinates are NaN or inf")
    return post_ops.cloud_fps(points, num_samples, start_index, mode)


def downsample_cloud(points, colors, max_num_points, sampling_strategy="uniform", *, voxel_size=None, generator=None, order="index"):
    """The notebook's downsampling block on a device cloud (points (n, 3) fp32, colors (n, 3) uint8): unchanged when max_num_points is
    None or n <= max_num_points; otherwise
      'uniform': `torch.randperm(n, generator=generator)[:max_num_points]` on the device, gathered in drawn order;
      'voxel': `voxel_down_sample` with `voxel_size`, or the notebook's heuristic (extent_x extent_y extent_z / max_num_points) ** (1/3) --
          which bounds the cloud near, not at, max_num_points, as there;
      'farthest_point': `farthest_point_down_sample(points, max_num_points)`, then order="index": the selected points in original index order
          with repeats collapsed (Open3D's `SelectByIndex` builds a mask), or order="selection": in selection order, repeats kept.
    Anything else raises the notebook's ValueError.  -> (points, colors) on the device."""
    if order not in ("index", "selection"):
        raise ValueError(f"downsample_cloud: order must be 'index' or 'selection', got {order!r}")
    if points is None:
        return None, None
    points, colors = _device_cloud(points, colors, "downsample_cloud")
    if max_num_points is None or len(points) <= max_num_points:
        return points, colors
    if sampling_strategy not in SAMPLING_STRATEGIES:   # inside the block, as in the notebook: a cloud that is small enough never gets here
        raise ValueError(f"Unsupported sampling strategy: {sampling_strategy}")
    if max_num_points < 1:
        raise ValueError(f"downsample_cloud: max_num_points = {max_num_points}; need >= 1")
    n = points.shape[0]
    if sampling_strategy == "uniform":
        index = torch.randperm(n, device=points.device, generator=generator)[:max_num_points]
        return post_ops.cloud_gather(points, colors, index)
    if sampling_strategy == "voxel":
        bounds = post_ops.cloud_bounds(points)
        if bounds[2]:
            raise ValueError(f"downsample_cloud: {bounds[2]} coordinates are NaN or inf")
        if voxel_size is None:
            voxel_size = heuristic_voxel_size(bounds[0], bounds[1], max_num_points)
        out = post_ops.cloud_voxel_down_sample(points, colors, voxel_size, bounds)
        return out["points"], out["colors"]
    selected = farthest_point_down_sample(points, max_num_points)
    if order == "selection":
        return post_ops.cloud_gather(points, colors, selected)
    mask = post_ops.cloud_mark(selected, n)
    u8 = colors if colors is not None else torch.zeros((n, 3), dtype=torch.uint8, device=points.device)
    out_p, out_c = post_ops.cloud_combine([None], [points], [u8], [mask], [(1, n)], [None])
    return out_p, (out_c if colors is not None else None)


def export_combined_ply(preds, views, export_ply_path=None, pts3d_key_to_visualize="pts3d_local_aligned_to_global",
                        conf_key_to_visualize="conf_local", min_conf_thr_percentile=0, flip_axes=False, max_num_points=None,
                        sampling_strategy="uniform", *, sample=0, voxel_size=None, generator=None):
    """The notebook's `export_combined_ply`, names, order and defaults: `combine_points`, then `downsample_cloud` when the cloud has more than
    `max_num_points` points, then -- with `export_ply_path` -- the file, written through `save_ply`.  `preds` may also be the dict
    `inference()` returns (then `views` may be None).  Keyword-only: `sample`, the batch row; `voxel_size`, overriding the heuristic of
    'voxel'; `generator`, a torch.Generator on the device for 'uniform'.  -> (points (M, 3) fp32, colors (M, 3) uint8) on the device;
    (None, None), and no file, when nothing is kept."""
    points, colors = combine_points(preds, views, pts3d_key_to_visualize=pts3d_key_to_visualize, conf_key_to_visualize=conf_key_to_visualize,
                                    min_conf_thr_percentile=min_conf_thr_percentile, flip_axes=flip_axes, sample=sample)
    if points is None:
        return None, None
    points, colors = downsample_cloud(points, colors, max_num_points, sampling_strategy, voxel_size=voxel_size, generator=generator)
    if export_ply_path:
        save_ply(export_ply_path, points, colors)
    return points, colors


__all__ = ["combine_points", "downsample_cloud", "export_combined_ply", "farthest_point_down_sample", "heuristic_voxel_size",
           "voxel_down_sample", "voxel_key_bits", "voxel_sort_passes"]
