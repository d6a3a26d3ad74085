"""TEST INFRASTRUCTURE: a stand-in for the four `cv2` calls of the reference's `detect_sky_mask` (fast3r/viz/viser_visualizer.py:33-57),
with OpenCV's uint8 semantics, so that tools/make_golden_sky.py can run that function unmodified where OpenCV is not installed:

* `cvtColor(img, COLOR_RGB2BGR)` and `cvtColor(img, COLOR_BGR2HSV)` for 8-bit images: H in [0, 180), the integer code of OpenCV's
  RGB2HSV_b (12-bit fixed-point tables, `cvRound`, the branch-free h selection with the -1 / 0 masks `vr`, `vg`);
* `inRange(src, lower, upper)`: 255 where every channel is inside its inclusive range, else 0;
* `dilate(src, kernel, iterations=1)` / `morphologyEx(src, MORPH_OPEN, kernel)`: the maximum / minimum over the kernel's footprint,
  anchor at the centre, with OpenCV's default morphology border (pixels outside the image never win: they are ignored).  The filters
  work on the uint8 VALUES (the reference's mask holds 0, 1 and 255 at that point), not on a boolean view of them.

OpenCV's binary never ran here, so this file is pinned on the definition (tests/test_sky.py: the HSV it computes lies within one unit of
the real-valued HSV over all 2^24 colours), not on OpenCV's output.  Written apart from tests/sky_ref.py on purpose: the golden generator
asserts that the two agree."""
import numpy as np

COLOR_RGB2BGR = 4
COLOR_BGR2HSV = 40
MORPH_OPEN = 2
HSV_SHIFT = 12


def _tables():
    sdiv = np.zeros(256, dtype=np.int32)
    hdiv = np.zeros(256, dtype=np.int32)
    for i in range(1, 256):
        sdiv[i] = int(np.rint((255 << HSV_SHIFT) / (1.0 * i)))
        hdiv[i] = int(np.rint((180 << HSV_SHIFT) / (6.0 * i)))
    return sdiv, hdiv


_SDIV, _HDIV = _tables()


def _bgr2hsv(bgr):
    b, g, r = (bgr[..., c].astype(np.int32) for c in range(3))
    v = np.maximum(np.maximum(b, g), r)
    vmin = np.minimum(np.minimum(b, g), r)
    diff = v - vmin
    vr = np.where(v == r, -1, 0).astype(np.int32)
    vg = np.where(v == g, -1, 0).astype(np.int32)
    s = (diff * _SDIV[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = (vr & (g - b)) + (~vr & ((vg & (b - r + 2 * diff)) + (~vg & (r - g + 4 * diff))))
    h = (h * _HDIV[diff] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = h + np.where(h < 0, 180, 0)
    return np.stack([np.clip(h, 0, 255), np.clip(s, 0, 255), v], axis=-1).astype(np.uint8)


def cvtColor(src, code):
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError(f"cv2_sky_stub.cvtColor: 8-bit 3-channel images only, got {src.dtype} {src.shape}")
    if code == COLOR_RGB2BGR:
        return np.ascontiguousarray(src[..., ::-1])
    if code == COLOR_BGR2HSV:
        return _bgr2hsv(src)
    raise NotImplementedError(f"cv2_sky_stub.cvtColor: code {code}")


def inRange(src, lowerb, upperb):
    src = np.asarray(src)
    lo, hi = np.asarray(lowerb), np.asarray(upperb)
    inside = np.all((src >= lo) & (src <= hi), axis=-1)
    return np.where(inside, 255, 0).astype(np.uint8)


def _rank_filter(src, kernel, want_max):
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 2:
        raise ValueError(f"cv2_sky_stub: morphology on 8-bit single-channel images only, got {src.dtype} {src.shape}")
    kernel = np.asarray(kernel)
    kh, kw = kernel.shape
    ay, ax = kh // 2, kw // 2
    H, W = src.shape
    border = 0 if want_max else 255   # morphologyDefaultBorderValue: the value that can never win
    pad = np.full((H + kh - 1, W + kw - 1), border, dtype=np.uint8)
    pad[ay:ay + H, ax:ax + W] = src
    out = np.full((H, W), border, dtype=np.uint8)
    for dy in range(kh):
        for dx in range(kw):
            if kernel[dy, dx]:
                win = pad[dy:dy + H, dx:dx + W]
                out = np.maximum(out, win) if want_max else np.minimum(out, win)
    return out


def dilate(src, kernel, iterations=1):
    for _ in range(iterations):
        src = _rank_filter(src, kernel, True)
    return src


def erode(src, kernel, iterations=1):
    for _ in range(iterations):
        src = _rank_filter(src, kernel, False)
    return src


def morphologyEx(src, op, kernel):
    if op != MORPH_OPEN:
        raise NotImplementedError(f"cv2_sky_stub.morphologyEx: op {op}")
    return dilate(erode(src, kernel), kernel)
