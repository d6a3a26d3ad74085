"""TEST INFRASTRUCTURE: a stand-in for the one `cv2` call of the reference's dataset path, `cv2.resize(src, dsize, fx=, fy=,
interpolation=cv2.INTER_NEAREST)` (fast3r/dust3r/datasets/utils/cropping.py:83-84), and for the names cropping.py and what it imports touch at import, so
that tools/make_golden_gt_views.py can run `BaseStereoViewDataset.__getitem__` unmodified where OpenCV is not installed.

OpenCV's nearest-neighbour rule (modules/imgproc/src/resize.cpp, resizeNN): with dsize given, fx and fy are ignored and recomputed as
`inv_scale_x = (double)dsize.width / ssize.width`; then `ifx = 1. / inv_scale_x` and, per destination column x,
`sx = cvFloor(x * ifx)`, `x_ofs[x] = min(sx, ssize.width - 1)`; rows the same with `ify`.  No half-pixel shift, all in double.

OpenCV's binary never ran here, so this file is pinned on that definition (tests/test_gt_views.py checks the index rule against its
closed form for all sizes up to 64), not on OpenCV's output.  Written apart from fast3r_amd/gt_views.py and tests/gt_views_ref.py on
purpose: the golden generator asserts that they agree."""
import numpy as np

INTER_NEAREST = 0
INTER_LINEAR = 1
INTER_CUBIC = 2
INTER_AREA = 3
INTER_LANCZOS4 = 4
IMREAD_COLOR = 1          # a default argument of the reference's imread_cv2 (dust3r/utils/image.py:35), evaluated at import
IMREAD_ANYDEPTH = 2
COLOR_BGR2RGB = 4


def nn_indices(src, dst):
    """x_ofs of resizeNN: the source index of each of `dst` destination indices over `src` source indices"""
    inv_scale = float(dst) / float(src)
    ifx = 1.0 / inv_scale
    ofs = np.floor(np.arange(dst, dtype=np.float64) * ifx).astype(np.int64)
    return np.minimum(ofs, src - 1)


def resize(src, dsize, dst=None, fx=0, fy=0, interpolation=INTER_LINEAR):
    if interpolation != INTER_NEAREST:
        raise NotImplementedError(f"cv2_resize_stub.resize: interpolation {interpolation}; only INTER_NEAREST")
    src = np.asarray(src)
    if src.ndim != 2:
        raise ValueError(f"cv2_resize_stub.resize: single-channel maps only, got shape {src.shape}")
    width, height = (int(v) for v in dsize)
    if width <= 0 or height <= 0:
        raise ValueError("cv2_resize_stub.resize: dsize must be positive (fx / fy alone are not supported)")
    ys, xs = nn_indices(src.shape[0], height), nn_indices(src.shape[1], width)
    return np.ascontiguousarray(src[ys[:, None], xs[None, :]])
