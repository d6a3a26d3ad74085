"""Ground-truth views from posed RGB-D frames, on the GPU: what the reference's datasets (7-Scenes, NRGBD, DTU, ScanNet++ ...) hand to
`evaluate_reconstruction`, `evaluate_camera_poses` and the validation loss, made here without OpenCV or torchvision and without a trip
through the host.

The reference's recipe, per frame (`BaseStereoViewDataset.__getitem__`, fast3r/dust3r/datasets/base/base_stereo_view_dataset.py:78-142):
`_crop_resize_if_necessary` (:165-221: a crop centred on the rounded principal point, a LANCZOS or BICUBIC resize of the image with a
nearest-neighbour resize of the depth, a second crop to the resolution, the intrinsics carried along), `ImgNorm`,
`depthmap_to_absolute_camera_coordinates` (dust3r/utils/geometry.py:186-243), the validity mask, `transpose_to_landscape` (:243-261).

* `plan_view` is the host part: the reference's arithmetic on sizes and intrinsics with the reference's dtypes, no pixel touched.  Views
  with equal plans form a launch group.
* Per group two kernel calls (fast3r_amd/csrc/f3r_views.hip): `f3r_gtview_resample` (both Pillow passes, the crops, ImgNorm, the
  transposition of portrait views) and `f3r_gtview_unproject` (the depth gather, the fp64 unprojection, the pose, the mask).  A group's
  tensors are one allocation each; the views hold slices.
* `build_gt_views` returns the views as the reference's `__getitem__` returns them after default collation of one sample (B = 1), on the
  device, plus `img_u8`, an addition: the cropped RGB bytes before normalisation, (h, w, 3), in the orientation of `img`.
* `crop_resize_if_necessary`, `depthmap_to_camera_coordinates`, `depthmap_to_absolute_camera_coordinates`: the reference's functions, on
  device tensors.

Bit for bit the reference's `img`, `depthmap`, `valid_mask`, `camera_intrinsics`, `true_shape` and camera-frame points; `pts3d` within
8 * 2^-24 * (sum_k |R_ik X_k| + |t_i|) per component, because numpy's einsum fixes no summation order (docs/rows_f.md).

Deviations, stated in DESIGN.md section 7 and docs/rows_f.md: the reference draws the orientation of a near-square frame from its RNG,
here the caller states it (`square_portrait`); `aug_crop`, a training augmentation, is not offered; the `rng` key is not returned; the
reference's asserts are ValueErrors.  There is no CPU path.
"""
import math

import numpy as np
import torch

from . import post_ops
from ._lib import GTVIEW_CAM_WORDS, F3RError
from .image import resample_tables

__all__ = ["build_gt_views", "crop_resize_if_necessary", "depthmap_to_absolute_camera_coordinates", "depthmap_to_camera_coordinates",
           "nearest_table", "plan_view"]


# ------------------------------------------------------------------------------------------------------------------- host plan
def _resolution(resolution):
    """an int or (width, height) with width >= height, as `_set_resolutions` (:144-163)"""
    if isinstance(resolution, (int, np.integer)) and not isinstance(resolution, bool):
        width = height = int(resolution)
    else:
        try:
            width, height = resolution
        except (TypeError, ValueError):
            raise ValueError(f"resolution = {resolution!r}; need an int or (width, height)") from None
        if not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in (width, height)):
            raise ValueError(f"resolution = {resolution!r}; width and height must be ints")
        width, height = int(width), int(height)
    if height < 1 or width < height:
        raise ValueError(f"resolution = {resolution!r}; need width >= height >= 1")
    return width, height


def nearest_table(src, dst):
    """cv2.resize(..., dsize, interpolation=INTER_NEAREST)'s source index of every destination index along one axis: with the scale
    inverted as OpenCV inverts it, `min(floor(x * (1.0 / (dst / src))), src - 1)`, all in double (fx and fy are ignored when dsize is
    given).  -> int32 (dst,)"""
    src, dst = int(src), int(dst)
    inv = 1.0 / (float(dst) / float(src))
    return np.array([min(int(math.floor(x * inv)), src - 1) for x in range(dst)], dtype=np.int32)


def _opencv_to_colmap(K):
    K = K.copy()
    K[0, 2] += 0.5
    K[1, 2] += 0.5
    return K


def _colmap_to_opencv(K):
    K = K.copy()
    K[0, 2] -= 0.5
    K[1, 2] -= 0.5
    return K


def _camera_matrix_of_crop(K, input_resolution, output_resolution, scaling=1, offset_factor=0.5):
    """cropping.py:93-106, operation for operation: the fp32 matrix is scaled in place by `scaling` (a float64 scalar in the rescale, the
    int 1 in the crop) and shifted by a float64 offset, every result rounded into the fp32 matrix"""
    margins = np.asarray(input_resolution) * scaling - output_resolution
    if not np.all(margins >= 0.0):
        raise ValueError(f"the {tuple(output_resolution)} target does not fit the {tuple(input_resolution)} picture")
    offset = offset_factor * margins
    Kc = _opencv_to_colmap(K)
    Kc[:2, :] *= scaling
    Kc[:2, 2] -= offset
    return _colmap_to_opencv(Kc)


def _crop_intrinsics(K, l, t):
    K = K.copy()
    K[0, 2] -= l
    K[1, 2] -= t
    return K


def plan_view(size_wh, intrinsics, resolution, square_portrait=False):
    """Everything `_crop_resize_if_necessary` does to ONE frame, as numbers.  size_wh: (W, H) of the frame; intrinsics: 3 x 3 (read as
    fp32, the dtype the reference's datasets hand over); resolution: int or (width, height), width >= height; square_portrait: the
    choice the reference draws from its RNG for a near-square crop when the resolution is not square.  -> dict:
      box1 (l, t, r, b): the crop around the rounded principal point (numpy rounds half to even);
      portrait: whether the target is flipped; target (w, h); scale_final; resized (w, h) = floor(cropped size * scale_final);
      filter: 'lanczos' when scale_final < 1, else 'bicubic';
      box2 (l, t, r, b): the second crop, in the resized picture; intrinsics: fp32 3 x 3 of the cropped picture (before transposition);
      true_shape (h, w); transpose: whether `transpose_to_landscape` turns the view (w < h).
    ValueError for the reference's asserts: a principal point with min_margin_x <= W / 5 or min_margin_y <= H / 5."""
    W, H = (int(v) for v in size_wh)
    res = _resolution(resolution)
    K = np.array(intrinsics, dtype=np.float32).reshape(3, 3)
    if not np.isfinite(K).all():
        raise ValueError("camera_intrinsics are not finite")
    cx, cy = K[:2, 2].round().astype(int)
    cx, cy = int(cx), int(cy)
    min_margin_x, min_margin_y = min(cx, W - cx), min(cy, H - cy)
    if not min_margin_x > W / 5 or not min_margin_y > H / 5:
        raise ValueError(f"bad principal point ({K[0, 2]}, {K[1, 2]}) in a {W} x {H} frame: the margins ({min_margin_x}, {min_margin_y}) must "
                         f"exceed a fifth of the size")
    l, t, r, b = cx - min_margin_x, cy - min_margin_y, cx + min_margin_x, cy + min_margin_y
    K1 = _crop_intrinsics(K, l, t)
    W1, H1 = r - l, b - t
    portrait = False
    if H1 > 1.1 * W1:
        portrait = True
    elif 0.9 < H1 / W1 < 1.1 and res[0] != res[1]:
        portrait = bool(square_portrait)
    target = res[::-1] if portrait else res
    # rescale_image_depthmap (cropping.py:62-90)
    input_resolution = np.array((W1, H1))
    scale_final = max(np.array(target) / (W1, H1)) + 1e-8
    output_resolution = np.floor(input_resolution * scale_final).astype(int)
    K2 = _camera_matrix_of_crop(K1, input_resolution, output_resolution, scaling=scale_final)
    W2, H2 = (int(v) for v in output_resolution)
    # the second crop (:211-219)
    K3 = _camera_matrix_of_crop(K2, (W2, H2), target, offset_factor=0.5)
    l2, t2 = np.int32(np.round(K2[:2, 2] - K3[:2, 2]))
    l2, t2 = int(l2), int(t2)
    if l2 < 0 or t2 < 0 or l2 + target[0] > W2 or t2 + target[1] > H2:
        raise ValueError(f"the second crop ({l2}, {t2}) + {target} leaves the resized {W2} x {H2} picture")
    K_out = _crop_intrinsics(K2, np.int32(l2), np.int32(t2))
    return {"size": (W, H), "box1": (l, t, r, b), "portrait": portrait, "target": (int(target[0]), int(target[1])), "scale_final": float(scale_final),
            "resized": (W2, H2), "filter": "lanczos" if scale_final < 1 else "bicubic", "box2": (l2, t2, l2 + int(target[0]), t2 + int(target[1])),
            "intrinsics": K_out, "true_shape": (int(target[1]), int(target[0])), "transpose": bool(target[0] < target[1])}


def _group_key(plan):
    return plan["box1"], plan["resized"], plan["filter"], plan["box2"], plan["transpose"]


def _returned_intrinsics(plan):
    """the intrinsics as the view returns them: rows [1, 0, 2] for a transposed view (`transpose_to_landscape`, :261)"""
    return plan["intrinsics"][[1, 0, 2]] if plan["transpose"] else plan["intrinsics"]


def _check_skew(K, who):
    K = np.float32(K)
    if K[0, 1] != 0.0 or K[1, 0] != 0.0:
        raise ValueError(f"{who}: camera_intrinsics have a skew term ({K[0, 1]}, {K[1, 0]}); the unprojection assumes none")


# ------------------------------------------------------------------------------------------------------------------- device side
def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise F3RError(f"fast3r_amd.gt_views runs on the ROCm GPU (device={device}); there is no CPU fallback")
    if dev.index is None:
        if not torch.cuda.is_available():
            raise F3RError("fast3r_amd.gt_views: no ROCm device is available; the HIP kernels need one (there is no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def _frame(x, dev, dtype, ndim, what):
    """a host or device array as a device tensor of `dtype` (no copy when it already is one)"""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if not torch.is_tensor(x):
        raise ValueError(f"{what} must be a torch tensor or a numpy array, got {type(x).__name__}")
    if x.dim() != ndim or (ndim == 3 and x.shape[2] != 3):
        raise ValueError(f"{what} must be {'(H, W, 3)' if ndim == 3 else '(H, W)'}, got {tuple(x.shape)}")
    if dtype == torch.uint8 and x.dtype != torch.uint8:
        raise ValueError(f"{what} must be uint8, got {x.dtype}")
    if dtype == torch.float32 and not x.dtype.is_floating_point:
        raise ValueError(f"{what} must be a floating-point map, got {x.dtype}")
    return x.to(dev, dtype)


def _small(x, shape, what):
    """a small host or device matrix as a float64 numpy array (values of an fp32 input are kept exactly)"""
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    a = np.asarray(x, dtype=np.float64)
    if a.shape != shape:
        raise ValueError(f"{what} must be {shape}, got {a.shape}")
    return a


class _Tables:
    """the device tables of a plan: Pillow's filter tables for both passes (made for the cropped size), the row span the kept rows read,
    and OpenCV's nearest tables; shared by the views of a group, cached over a call"""

    def __init__(self, plan, dev):
        l, t, r, b = plan["box1"]
        (W1, H1), (W2, H2) = (r - l, b - t), plan["resized"]
        self.window = (l, t, W1, H1)
        l2, t2, r2, b2 = plan["box2"]
        self.crop = (l2, t2, r2 - l2, b2 - t2)
        kh, bh, wh = resample_tables(W1, W2, plan["filter"])
        kv, bv, wv = resample_tables(H1, H2, plan["filter"])
        kept = bv[t2:b2].astype(np.int64)
        self.row_span = (int(kept[:, 0].min()), int((kept[:, 0] + kept[:, 1]).max()))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.tables_h, self.tables_v = (kh, up(bh), up(wh)), (kv, up(bv), up(wv))
        self.nearest = (up(nearest_table(W1, W2)), up(nearest_table(H1, H2)))


def _run_group(plan, tables, images, depthmaps, cams, flag):
    img_u8, img = post_ops.gtview_resample(images, tables.window, tables.tables_h, tables.tables_v, plan["resized"], tables.crop, tables.row_span,
                                           plan["transpose"])
    depth, pts, valid = post_ops.gtview_unproject(depthmaps, cams, tables.window, tables.nearest, plan["resized"], tables.crop, plan["transpose"],
                                                  flag=flag)
    return img_u8, img, depth, pts, valid


def _per_view(x, n, what):
    if isinstance(x, (bool, np.bool_)):
        return [bool(x)] * n
    x = list(x)
    if len(x) != n:
        raise ValueError(f"{what} has {len(x)} entries for {n} views")
    return x


def build_gt_views(images, depthmaps, camera_intrinsics, camera_poses=None, *, resolution, dataset="unknown", labels=None, instances=None,
                   square_portrait=False, device="cuda", check_finite=True):
    """N posed RGB-D frames -> the N ground-truth views the reference's datasets return (the module text), collated with B = 1, on `device`.
    images: N (H, W, 3) uint8 arrays or tensors, host or device, sizes may differ; depthmaps: N (H, W) fp32; camera_intrinsics: N 3 x 3;
    camera_poses: N 4 x 4 cam-to-world, or None: a NaN pose, `pts3d` NaN and `valid_mask` all False (:114-115); resolution: int or
    (width, height), width >= height; square_portrait: a bool or N bools; labels, instances: N strings (default: the view's number).
    Each view: img (1, 3, h, w) fp32, depthmap (1, h, w) fp32, pts3d (1, h, w, 3) fp32, valid_mask (1, h, w) bool, camera_pose (1, 4, 4)
    fp32, camera_intrinsics (1, 3, 3) fp32, true_shape (1, 2) int32 (before the transposition, as in the reference), dataset / label /
    instance (one-element lists), idx (the collated triple (0, 0, view number)), and img_u8 (h, w, 3) uint8.  Portrait views come back
    transposed with intrinsics rows [1, 0, 2].  Views with equal plans are one launch group: their tensors are slices of one allocation.
    ValueError: a bad principal point, a skew term, a pose that is not finite, and with check_finite a depth that is not finite (one
    flag word read back once, at the end of the call)."""
    dev = _device(device)
    images, depthmaps, camera_intrinsics = list(images), list(depthmaps), list(camera_intrinsics)
    n = len(images)
    if n < 1 or len(depthmaps) != n or len(camera_intrinsics) != n or (camera_poses is not None and len(camera_poses) != n):
        raise ValueError(f"build_gt_views: need one depthmap, one camera_intrinsics (and one camera_pose) per image and at least one image; got "
                         f"{n} images, {len(depthmaps)} depthmaps, {len(camera_intrinsics)} intrinsics"
                         + ("" if camera_poses is None else f", {len(camera_poses)} poses"))
    res = _resolution(resolution)
    portrait = _per_view(square_portrait, n, "square_portrait")
    labels = [str(i) for i in range(n)] if labels is None else [str(s) for s in _per_view(labels, n, "labels")]
    instances = [str(i) for i in range(n)] if instances is None else [str(s) for s in _per_view(instances, n, "instances")]
    # host: shapes, intrinsics, poses, plans
    cams = np.full((n, GTVIEW_CAM_WORDS), np.nan, dtype=np.float32)
    shapes = np.zeros((n, 2), dtype=np.int32)
    plans, groups = [], {}
    for i in range(n):
        img, dep = images[i], depthmaps[i]
        if not hasattr(img, "shape") or not hasattr(dep, "shape") or len(img.shape) != 3 or tuple(dep.shape) != tuple(img.shape[:2]):
            raise ValueError(f"build_gt_views: view {i}: the image must be (H, W, 3) and the depthmap (H, W) of the same frame, got "
                             f"{tuple(getattr(img, 'shape', ()))} and {tuple(getattr(dep, 'shape', ()))}")
        K = _small(camera_intrinsics[i], (3, 3), f"build_gt_views: camera_intrinsics[{i}]")
        _check_skew(K, f"build_gt_views: view {i}")
        plan = plan_view((img.shape[1], img.shape[0]), K, res, portrait[i])
        plans.append(plan)
        groups.setdefault(_group_key(plan), []).append(i)
        cams[i, :9] = _returned_intrinsics(plan).reshape(-1)
        shapes[i] = plan["true_shape"]
        if camera_poses is not None:
            pose = _small(camera_poses[i], (4, 4), f"build_gt_views: camera_poses[{i}]")
            if not np.isfinite(pose).all():
                raise ValueError(f"build_gt_views: NaN in camera pose for view {i}")
            cams[i, 9:] = pose.astype(np.float32).reshape(-1)
    views = [None] * n
    with torch.cuda.device(dev):
        order = [i for members in groups.values() for i in members]   # group-major, so that a group's cameras are one run of the table
        cams_dev = torch.from_numpy(cams[order]).to(dev)
        shapes_dev = torch.from_numpy(shapes[order]).to(dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev) if check_finite else None
        at = 0
        for members in groups.values():
            plan, m = plans[members[0]], len(members)
            tables = _Tables(plan, dev)
            imgs = [_frame(images[i], dev, torch.uint8, 3, f"build_gt_views: images[{i}]") for i in members]
            deps = [_frame(depthmaps[i], dev, torch.float32, 2, f"build_gt_views: depthmaps[{i}]") for i in members]
            img_u8, img, depth, pts, valid = _run_group(plan, tables, imgs, deps, cams_dev[at:at + m], flag)
            for k, i in enumerate(members):
                row = cams_dev[at + k]
                views[i] = {"img": img[k:k + 1], "depthmap": depth[k:k + 1], "pts3d": pts[k:k + 1], "valid_mask": valid[k:k + 1],
                            "camera_pose": row[9:].view(1, 4, 4), "camera_intrinsics": row[:9].view(1, 3, 3),
                            "true_shape": shapes_dev[at + k:at + k + 1], "dataset": [str(dataset)], "label": [labels[i]], "instance": [instances[i]],
                            "idx": [torch.tensor([0]), torch.tensor([0]), torch.tensor([i])], "img_u8": img_u8[k]}
            at += m
        if check_finite and int(flag.item()) != 0:
            raise ValueError("build_gt_views: NaN or infinity in a depthmap (check_finite=False skips this check)")
    return views


# ------------------------------------------------------------------------------------------------------------------- the reference's names
def _device_tensor(x, dtype, ndim, who, name):
    if not torch.is_tensor(x):
        raise ValueError(f"{who}: {name} must be a torch tensor on a ROCm device, got {type(x).__name__}")
    if not x.is_cuda:
        raise F3RError(f"fast3r_amd: {name} lives on {x.device}; the HIP kernels need a ROCm device (there is no CPU fallback)")
    return _frame(x, x.device, dtype, ndim, f"{who}: {name}")


def _cams_row(K, pose, dev):
    row = np.full((1, GTVIEW_CAM_WORDS), np.nan, dtype=np.float32)
    row[0, :9] = np.float32(K).reshape(-1)
    if pose is not None:
        row[0, 9:] = np.float32(pose).reshape(-1)
    return torch.from_numpy(row).to(dev)


def crop_resize_if_necessary(image, depthmap, intrinsics, resolution, *, square_portrait=False):
    """`BaseStereoViewDataset._crop_resize_if_necessary` (:165-221) of one frame on the device.  image (H, W, 3) uint8 and depthmap (H, W)
    fp32 device tensors; intrinsics 3 x 3 (host or device).  -> (img_u8 (h, w, 3) uint8, depthmap (h, w) fp32, intrinsics2 (3, 3) fp32 on
    the device), not transposed, as the reference returns them."""
    who = "crop_resize_if_necessary"
    image = _device_tensor(image, torch.uint8, 3, who, "image")
    depthmap = _device_tensor(depthmap, torch.float32, 2, who, "depthmap")
    if tuple(depthmap.shape) != tuple(image.shape[:2]) or depthmap.device != image.device:
        raise ValueError(f"{who}: image {tuple(image.shape)} on {image.device} and depthmap {tuple(depthmap.shape)} on {depthmap.device} are not one frame")
    dev = image.device
    plan = dict(plan_view((image.shape[1], image.shape[0]), _small(intrinsics, (3, 3), f"{who}: intrinsics"), resolution, square_portrait), transpose=False)
    with torch.cuda.device(dev):
        tables = _Tables(plan, dev)
        cams = _cams_row(plan["intrinsics"], None, dev)
        img_u8, _ = post_ops.gtview_resample([image], tables.window, tables.tables_h, tables.tables_v, plan["resized"], tables.crop, tables.row_span, False)
        depth, _, _ = post_ops.gtview_unproject([depthmap], cams, tables.window, tables.nearest, plan["resized"], tables.crop, False, want_points=False)
    return img_u8[0], depth[0], cams[0, :9].view(3, 3)


def _unproject(depthmap, camera_intrinsics, camera_pose, who):
    depthmap = _device_tensor(depthmap, torch.float32, 2, who, "depthmap")
    K = _small(camera_intrinsics, (3, 3), f"{who}: camera_intrinsics")
    _check_skew(K, who)
    pose = None
    if camera_pose is not None:
        rows = 3 if tuple(camera_pose.shape) == (3, 4) else 4   # a 3 x 4 pose is accepted, as by the reference; only R and t are read
        pose = np.vstack([_small(camera_pose, (rows, 4), f"{who}: camera_pose")[:3], [[0.0, 0.0, 0.0, 1.0]]])
    H, W = (int(v) for v in depthmap.shape)
    dev = depthmap.device
    with torch.cuda.device(dev):
        _, pts, valid = post_ops.gtview_unproject([depthmap], _cams_row(K, pose, dev), (0, 0, W, H), None, (W, H), (0, 0, W, H), False,
                                                  pose=pose is not None, finite_mask=False)
    return pts[0], valid[0]


def depthmap_to_camera_coordinates(depthmap, camera_intrinsics):
    """dust3r/utils/geometry.py:186-218 on the device: depthmap (H, W) fp32 device tensor, camera_intrinsics 3 x 3 -> (X_cam (H, W, 3) fp32,
    valid_mask (H, W) bool = depthmap > 0).  x = (u - cu) z / fu and y = (v - cv) z / fv in fp64, rounded once to fp32: bit for bit
    numpy's result.  ValueError for a skew term (the reference's assert)."""
    return _unproject(depthmap, camera_intrinsics, None, "depthmap_to_camera_coordinates")


def depthmap_to_absolute_camera_coordinates(depthmap, camera_intrinsics, camera_pose):
    """dust3r/utils/geometry.py:221-243 on the device: the camera-frame points moved by the 4 x 4 (or 3 x 4) cam-to-world pose in fp32 ->
    (X_world (H, W, 3) fp32, valid_mask (H, W) bool = depthmap > 0)."""
    return _unproject(depthmap, camera_intrinsics, camera_pose, "depthmap_to_absolute_camera_coordinates")
