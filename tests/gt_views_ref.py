"""TEST INFRASTRUCTURE: the reference's ground-truth view recipe restated with numpy and Pillow alone -- `BaseStereoViewDataset.__getitem__`
(fast3r/dust3r/datasets/base/base_stereo_view_dataset.py:78-142) with `_crop_resize_if_necessary` (:165-221), cropping.py, `ImgNorm`,
`depthmap_to_absolute_camera_coordinates` (dust3r/utils/geometry.py:186-243) and `transpose_to_landscape` -- without OpenCV, torchvision or
the reference.  Pillow does the image work (crop, resize, crop); the depth resize is OpenCV's nearest rule written as one index
expression.  It is the yardstick where the reference does not exist (the GPU tests), and tools/make_golden_gt_views.py asserts that it
reproduces what the reference itself returns.  Written apart from fast3r_amd/gt_views.py: it shares no code with it."""
import numpy as np
import PIL.Image

try:
    LANCZOS, BICUBIC = PIL.Image.Resampling.LANCZOS, PIL.Image.Resampling.BICUBIC
except AttributeError:
    LANCZOS, BICUBIC = PIL.Image.LANCZOS, PIL.Image.BICUBIC

KEYS_EXACT = ("img", "depthmap", "valid_mask", "camera_intrinsics", "true_shape")


def nearest_indices(src, dst):
    return np.array([min(int(np.floor(x * (1.0 / (dst / src)))), src - 1) for x in range(dst)], dtype=np.int64)


def shifted(K, dx, dy):
    K = K.copy()
    K[0, 2] += dx
    K[1, 2] += dy
    return K


def matrix_of_crop(K, size_in, size_out, scaling=1):
    margins = np.asarray(size_in) * scaling - size_out
    assert np.all(margins >= 0.0)
    M = shifted(K, 0.5, 0.5)
    M[:2, :] *= scaling
    M[:2, 2] -= 0.5 * margins
    return shifted(M, -0.5, -0.5)


def crop_resize(image, depthmap, K, resolution, square_portrait=False):
    """-> (PIL image, depthmap, intrinsics, trace): what `_crop_resize_if_necessary` returns, and the numbers it passed through"""
    K = np.float32(K)
    pic = PIL.Image.fromarray(image)
    W, H = pic.size
    cx, cy = K[:2, 2].round().astype(int)
    mx, my = min(cx, W - cx), min(cy, H - cy)
    if not (mx > W / 5 and my > H / 5):
        raise ValueError("bad principal point")
    box1 = (int(cx - mx), int(cy - my), int(cx + mx), int(cy + my))
    pic, depthmap, K = pic.crop(box1), depthmap[box1[1]:box1[3], box1[0]:box1[2]], shifted(K, -box1[0], -box1[1])
    W, H = pic.size
    resolution = tuple(resolution)
    assert resolution[0] >= resolution[1]
    if H > 1.1 * W or (0.9 < H / W < 1.1 and resolution[0] != resolution[1] and square_portrait):
        resolution = resolution[::-1]
    scale = max(np.array(resolution) / pic.size) + 1e-8
    size_in = np.array(pic.size)
    size_out = np.floor(size_in * scale).astype(int)
    pic = pic.resize(tuple(int(v) for v in size_out), resample=LANCZOS if scale < 1 else BICUBIC)
    ys, xs = nearest_indices(H, int(size_out[1])), nearest_indices(W, int(size_out[0]))
    depthmap = depthmap[ys[:, None], xs[None, :]]
    K = matrix_of_crop(K, size_in, size_out, scaling=scale)
    K2 = matrix_of_crop(K, pic.size, resolution)
    l, t = np.int32(np.round(K[:2, 2] - K2[:2, 2]))
    box2 = (int(l), int(t), int(l) + resolution[0], int(t) + resolution[1])
    pic, depthmap = pic.crop(box2), depthmap[box2[1]:box2[3], box2[0]:box2[2]]
    K = K.copy()
    K[0, 2] -= l
    K[1, 2] -= t
    trace = {"box1": box1, "box2": box2, "resized": (int(size_out[0]), int(size_out[1])), "scale_final": float(scale),
             "filter": "lanczos" if scale < 1 else "bicubic", "nearest_x": xs.astype(np.int32), "nearest_y": ys.astype(np.int32)}
    return pic, np.ascontiguousarray(depthmap), K, trace


def img_norm(pic):
    a = np.asarray(pic).astype(np.float32).transpose(2, 0, 1) / np.float32(255)
    return ((a - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)


def camera_points(depthmap, K):
    K = np.float32(K)
    assert K[0, 1] == 0.0 and K[1, 0] == 0.0
    H, W = depthmap.shape
    u, v = np.meshgrid(np.arange(W), np.arange(H))
    x = (u - K[0, 2]) * depthmap / K[0, 0]
    y = (v - K[1, 2]) * depthmap / K[1, 1]
    with np.errstate(over="ignore"):
        return np.stack((x, y, depthmap), axis=-1).astype(np.float32), depthmap > 0.0


def world_points(X, pose):
    """R X + t as three fp32 products and three fp32 sums per component, in index order (numpy's einsum fixes no order)"""
    R, t = pose[:3, :3].astype(np.float32), pose[:3, 3].astype(np.float32)
    with np.errstate(all="ignore"):
        return np.stack([(R[i, 0] * X[..., 0] + R[i, 1] * X[..., 1]) + R[i, 2] * X[..., 2] + t[i] for i in range(3)], axis=-1).astype(np.float32)


def pts3d_bound(X, pose):
    """8 * 2^-24 * (sum_k |R_ik X_k| + |t_i|) per component, in fp64"""
    R, t = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    with np.errstate(all="ignore"):
        S = np.abs(X.astype(np.float64))[..., None, :] * np.abs(R)[None, None]
        return 8.0 * 2.0 ** -24 * (S.sum(-1) + np.abs(t))


def make_view(image, depthmap, K, pose, resolution, square_portrait=False):
    """one frame -> the view dict of `__getitem__` (numpy arrays, not collated), plus img_u8, X_cam and the trace"""
    pic, depth, K2, trace = crop_resize(np.asarray(image), np.asarray(depthmap, dtype=np.float32), K, resolution, square_portrait)
    width, height = pic.size
    if pose is None:
        pose = np.full((4, 4), np.nan, dtype=np.float32)
    else:
        pose = np.float32(pose)
        if not np.isfinite(pose).all():
            raise ValueError("NaN in camera pose")
    if not np.isfinite(depth).all():
        raise ValueError("NaN in depthmap")
    X, positive = camera_points(depth, K2)
    pts = world_points(X, pose)
    view = {"img": img_norm(pic), "img_u8": np.asarray(pic).copy(), "depthmap": depth, "camera_intrinsics": K2, "camera_pose": pose,
            "pts3d": pts, "valid_mask": positive & np.isfinite(pts).all(axis=-1), "true_shape": np.int32((height, width)), "X_cam": X,
            "trace": trace}
    if width < height:
        view["img"] = view["img"].swapaxes(1, 2)
        for key in ("img_u8", "valid_mask", "depthmap", "pts3d", "X_cam"):
            view[key] = view[key].swapaxes(0, 1)
        view["camera_intrinsics"] = view["camera_intrinsics"][[1, 0, 2]]
    return view


def build(images, depthmaps, intrinsics, poses, resolution, square_portrait=False):
    n = len(images)
    flags = [square_portrait] * n if isinstance(square_portrait, bool) else list(square_portrait)
    return [make_view(images[i], depthmaps[i], intrinsics[i], None if poses is None else poses[i], resolution, flags[i]) for i in range(n)]


def pts3d_close(got, ref_view):
    """got within the derived bound of the reference's pts3d wherever that is finite, and non-finite exactly where it is not"""
    ref = ref_view["pts3d"]
    fin = np.isfinite(ref)
    if not np.array_equal(np.isfinite(got), fin):
        return False, float("inf")
    if not fin.any():
        return True, 0.0
    bound = pts3d_bound(ref_view["X_cam"], ref_view["camera_pose"])
    with np.errstate(all="ignore"):
        ratio = np.abs(got.astype(np.float64) - ref.astype(np.float64))[fin] / bound[fin]
    ratio = ratio[np.isfinite(ratio)]   # a bound of 0 (a point at the origin of a pure rotation): the difference must be 0 too
    zero = (bound[fin] == 0) & (got[fin] != ref[fin])
    worst = float(ratio.max()) if ratio.size else 0.0
    return bool(worst <= 1.0 and not zero.any()), worst
