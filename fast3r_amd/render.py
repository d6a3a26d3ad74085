"""Pictures of a point cloud on the GPU: `render_cumulative_pts3d_viz` of the reference's multi-view notebook
(`notebooks/demo_multiview.ipynb`), the last consumer of a prediction in that notebook.  There every frame is a fresh `pyrender` scene and
EGL context over host copies of every pointmap; here the cloud stays on the device and the renderer is a z-buffered point splat
(fast3r_amd/csrc/f3r_render.hip): integer `atomicMin` on a packed (fp32 depth, point index) key per pixel.  Frame i of the cumulative
pictures is the key buffer after view i's points went in, so all frames together take one pass over the cloud.

* `Camera`: `view` (3 x 4 fp64 world-to-eye; the eye frame is OpenGL's: x right, y up, looking along -z), `sx`, `sy` (the diagonal of
  pyrender's perspective matrix: 1 / (aspect tan(yfov / 2)) and 1 / tan(yfov / 2)), `cx`, `cy` (the principal point's offset in normalised
  device coordinates, 0 for a centred camera) and `znear` (0.05, pyrender's default).  The projection is infinite, as `zfar=None` gives.
* `birdseye_camera(center, min_bound, max_bound)`: the notebook's stationary camera as the notebook computes it, quirk included (below).
* `pinhole_camera(c2w, focal, pp, H, W)`: a camera `estimate_camera_poses` predicted (OpenCV convention, pixels).
* `render_points(points, colors, camera, ...)`: one frame, or with `segments=` a generator of one frame per segment.
* `render_cumulative_pts3d_viz(preds, views, output_dir, point_size, min_conf_thr_percentile)`: the notebook's function, names, order and
  defaults; writes `cumulative_{i:03d}.png`.

The per-point arithmetic is the header comment of include/f3r.h ("point-splat renderer"); tests/render_ref.py restates it in numpy.

The bird's-eye quirk.  The notebook builds a camera-to-world pose at center + (0, 0, 2 max_extent) looking at center with up = (0, 1, 0),
turns it into a view matrix (inverse, then y and z flipped), and hands that *view* matrix to pyrender as the camera's *pose*.  pyrender
inverts the pose to get its view matrix.  The camera therefore sits at (c_x, -c_y, c_z + 2 max_extent) with axes diag(-1, -1, 1): it looks
down -z as intended, but the picture is turned by 180 degrees and is centred on the cloud only when c_y is near 0.  This project
reproduces the reference's arithmetic, so the quirk stays; pass `camera=` for another view.  A cloud whose bounding box has no extent has
no such camera (the notebook divides 0 by 0): `ValueError`.

Deviations, stated in DESIGN.md section 7 and docs/rows_f.md: one sample per pixel at its centre (pyrender's offscreen target is
multisampled, which softens the rim of each square); the depth compared is the fp32 eye distance, not a 24-bit window depth; the centre
is an fp64 sum in a fixed order where numpy adds fp32 rows; colours saturate as in `combine_points`; the PNG bytes are PIL's.
"""
import math
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np
import torch

from . import post_ops
from .cloud import combine_points

PNG_WORKERS = 16  # host threads that encode PNGs, at most


@dataclass(frozen=True)
class Camera:
    view: tuple          # 12 floats: the 3 x 4 world-to-eye matrix, row-major
    sx: float
    sy: float
    cx: float = 0.0
    cy: float = 0.0
    znear: float = 0.05

    def words(self):
        """the 17 doubles of f3r_render_splat"""
        return list(self.view) + [self.sx, self.sy, self.cx, self.cy, self.znear]


def _camera(view, sx, sy, cx, cy, znear, who):
    view = np.asarray(view, dtype=np.float64)
    cam = Camera(tuple(float(v) for v in view[:3].reshape(-1)), float(sx), float(sy), float(cx), float(cy), float(znear))
    if not all(math.isfinite(w) for w in cam.words()):
        raise ValueError(f"{who}: the camera is not finite: {cam}")
    if not cam.znear > 0:
        raise ValueError(f"{who}: znear = {cam.znear}; need > 0")
    return cam


def look_at_pose(position, target, up):
    """A camera-to-world matrix at `position` whose third column points at `target` and whose first column is up x forward (normalised);
    when up is parallel to forward, up becomes (0, 0, 1), or (1, 0, 0) if up's y component is 1.  fp64."""
    position, target, up = (np.asarray(a, dtype=np.float64) for a in (position, target, up))
    with np.errstate(invalid="ignore", divide="ignore"):
        forward = target - position
        forward = forward / np.linalg.norm(forward)
        right = np.cross(up, forward)
        if np.linalg.norm(right) < 1e-6:
            up = np.array([0.0, 0.0, 1.0]) if up[1] != 1 else np.array([1.0, 0.0, 0.0])
            right = np.cross(up, forward)
        right = right / np.linalg.norm(right)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = right, np.cross(forward, right), forward, position
    return pose


def opengl_view_of(c2w):
    """inverse(c2w) with its y and z columns negated: what the notebook calls the OpenGL view matrix of a camera-to-world pose"""
    return np.linalg.inv(np.asarray(c2w, dtype=np.float64)) @ np.diag([1.0, -1.0, -1.0, 1.0])


def birdseye_camera(center, min_bound, max_bound, yfov=math.pi / 3, aspect=16 / 9, znear=0.05):
    """The notebook's camera for a cloud with that centre and bounding box (the module text has the quirk).  max_extent is the largest
    fp32 difference max - min, as numpy computes it on the fp32 cloud; the rest is host fp64."""
    center = np.asarray(center, dtype=np.float64).reshape(3)
    extent = np.asarray(max_bound, dtype=np.float32).reshape(3) - np.asarray(min_bound, dtype=np.float32).reshape(3)
    distance = np.float32(np.max(extent)) * 2
    position = center + np.array([0.0, 0.0, float(distance)])
    with np.errstate(invalid="ignore"):
        given_as_pose = opengl_view_of(look_at_pose(position, center, (0.0, 1.0, 0.0)))
    if not np.isfinite(given_as_pose).all():
        raise ValueError(f"birdseye_camera: no camera for centre {center.tolist()} and extent {extent.tolist()}: the reference divides 0 by 0 "
                         "when the camera's distance, twice the largest extent, does not move it off the centre")
    view = np.linalg.inv(given_as_pose)   # pyrender's view matrix is the inverse of the node's pose
    t = math.tan(0.5 * float(yfov))
    return _camera(view, 1.0 / (float(aspect) * t), 1.0 / t, 0.0, 0.0, znear, "birdseye_camera")


def pinhole_camera(c2w, focal, pp, H, W, znear=0.05):
    """The camera of a predicted pose: c2w (4 x 4 or 3 x 4 camera-to-world, OpenCV convention: x right, y down, z forward), focal and
    principal point pp = (x, y) in pixels of an H x W image whose pixel (u, v) has its centre at (u, v) -- the pixel grid
    `estimate_camera_poses` and the pointmaps use.  A point that projects to (u, v) lands at window position (u + 0.5, H - 0.5 - v): in
    the middle of pixel (row v, column u) of a width = W, height = H picture."""
    if torch.is_tensor(c2w):
        c2w = c2w.detach().cpu().numpy()
    m = np.eye(4)
    m[:3] = np.asarray(c2w, dtype=np.float64).reshape(-1, 4)[:3]
    view = np.diag([1.0, -1.0, -1.0, 1.0]) @ np.linalg.inv(m)
    focal, H, W = float(focal), int(H), int(W)
    ppx, ppy = (float(v) for v in pp)
    return _camera(view, 2.0 * focal / W, 2.0 * focal / H, (2.0 * ppx + 1.0) / W - 1.0, 1.0 - (2.0 * ppy + 1.0) / H, znear, "pinhole_camera")


def cloud_camera(points, **kwargs):
    """`birdseye_camera` of a device cloud: the centre from f3r_render_center, the box from f3r_cloud_bounds.  ValueError on a NaN or inf
    coordinate: such a cloud has no centre."""
    lo, hi, bad = post_ops.cloud_bounds(points)
    if bad:
        raise ValueError(f"render: {bad} coordinates are NaN or inf, so the cloud has no centre to derive a camera from; pass camera=")
    return birdseye_camera(post_ops.render_center(points), lo, hi, **kwargs)


def _checked(width, height, point_size, camera, who):
    width, height = post_ops._render_viewport(width, height, who)
    point_size = float(point_size)
    if not (math.isfinite(point_size) and point_size > 0):
        raise ValueError(f"{who}: point_size = {point_size}; need a finite value > 0")
    if not isinstance(camera, Camera):
        raise ValueError(f"{who}: camera must be a fast3r_amd.render.Camera or None, got {type(camera).__name__}")
    return width, height, point_size


def _frames(points, colors, camera, ends, width, height, point_size, background, return_depth, wanted=None):
    keys = post_ops.render_keys(width, height, points.device)
    start = 0
    for i, end in enumerate(ends):
        if end > start:
            post_ops.render_splat(points, start, end, camera.words(), point_size, keys)
        start = end
        if wanted is None or i in wanted:
            yield post_ops.render_resolve(keys, colors, background, return_depth=return_depth)


def render_points(points, colors, camera=None, *, width=1920, height=1080, point_size=5.0, background=(255, 255, 255), segments=None,
                  return_depth=False):
    """A device cloud (points (n, 3) fp32, colors (n, 3) uint8: what `combine_points`, `export_combined_ply` or `Scene.collect_points`
    return) as a (height, width, 3) uint8 device picture, row 0 at the top, through `camera` (None: `cloud_camera(points)`, the notebook's).
    Every point is a square of point_size pixels, drawn iff its centre is inside the frustum and not nearer than znear; the nearest point
    shows, at equal depth the one with the lowest index; `background` elsewhere.  segments: ascending end offsets into the cloud -- then
    the call returns a generator of one frame per segment, frame i showing points [0, segments[i]) (a generator keeps memory bounded:
    1500 frames of 1080p are 9 GB).  return_depth: (picture, (height, width) fp32 eye distance, +inf where empty) instead of the picture.
    A point with a NaN or inf coordinate is not drawn; with camera=None it is a ValueError.  Inputs are never written."""
    points, colors, n = post_ops._cloud_points(points, "render_points", colors, bits=32)
    if colors is None:
        raise ValueError("render_points: colors must be an (n, 3) uint8 device tensor")
    if camera is None:
        camera = cloud_camera(points)
    width, height, point_size = _checked(width, height, point_size, camera, "render_points")
    if segments is None:
        return next(_frames(points, colors, camera, [n], width, height, point_size, background, return_depth))
    ends = [int(e) for e in segments]
    if any(b < a for a, b in zip([0] + ends, ends)) or (ends and ends[-1] > n):
        raise ValueError(f"render_points: segments must be ascending end offsets within [0, {n}], got {ends}")
    return _frames(points, colors, camera, ends, width, height, point_size, background, return_depth)


def _save_png(array, path):
    from PIL import Image
    Image.fromarray(array).save(path)


def render_cumulative_pts3d_viz(preds, views, output_dir="./output", point_size=5.0, min_conf_thr_percentile=0, *, sample=0, width=1920,
                                height=1080, camera=None, frames=None, return_frames=False):
    """The notebook's `render_cumulative_pts3d_viz`, names, order and defaults: per view the pixels of `pts3d_in_other_view` with conf >
    np.percentile(conf, min_conf_thr_percentile) and their colours (`combine_points` with those two keys), the notebook's stationary
    bird's-eye camera over the whole cloud, and per view i the picture of views 0 .. i, written to output_dir/cumulative_{i:03d}.png.  A
    view that keeps nothing repeats the previous picture; when no view keeps anything, nothing is written (the notebook's "No points to
    render").  `preds` may be the dict `inference()` returns (then `views` may be None).  Keyword-only: `sample`, the batch row; `width`,
    `height` (the notebook's 1920 x 1080); `camera`, a `Camera` instead of the bird's-eye one; `frames`, the view indices to resolve and
    write (None: all); `return_frames`: also return the pictures as a list of (height, width, 3) uint8 device tensors (1080p: 6 MB each).
    The pictures are copied to the host one at a time and encoded by up to 16 threads through PIL.  -> None, or the list."""
    os.makedirs(output_dir, exist_ok=True)
    points, colors, ends = combine_points(preds, views, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                          min_conf_thr_percentile=min_conf_thr_percentile, sample=sample, return_offsets=True)
    if points is None:
        return [] if return_frames else None
    wanted = None if frames is None else {int(f) for f in frames}
    if wanted is not None and any(not 0 <= f < len(ends) for f in wanted):
        raise ValueError(f"render_cumulative_pts3d_viz: frames = {sorted(wanted)} outside [0, {len(ends)})")
    if camera is None:
        camera = cloud_camera(points)
    order = [i for i in range(len(ends)) if wanted is None or i in wanted]
    if not order:
        return [] if return_frames else None
    width, height, point_size = _checked(width, height, point_size, camera, "render_cumulative_pts3d_viz")
    pictures = _frames(points, colors, camera, ends[:order[-1] + 1], width, height, point_size, (255, 255, 255), False, set(order))
    kept, pending = [], deque()
    with ThreadPoolExecutor(max_workers=min(PNG_WORKERS, len(order))) as pool:
        for i, picture in zip(order, pictures):
            pending.append(pool.submit(_save_png, picture.cpu().numpy(), os.path.join(output_dir, f"cumulative_{i:03d}.png")))
            if return_frames:
                kept.append(picture)
            while len(pending) > 2 * PNG_WORKERS:  # host pictures waiting for a thread stay bounded
                pending.popleft().result()
        for f in pending:
            f.result()
    return kept if return_frames else None


__all__ = ["Camera", "birdseye_camera", "cloud_camera", "pinhole_camera", "render_cumulative_pts3d_viz", "render_points"]
