"""TEST INFRASTRUCTURE: the plain numpy restatement of the reference's `detect_sky_mask` (fast3r/viz/viser_visualizer.py:24-72) that the
sky kernels are compared with: the 8-bit conversion, OpenCV's integer HSV, the colour ranges, binary 7 x 7 OR / AND box filters with
ignored borders, ONE 4-connected labelling (scipy.ndimage.label) and the top-row / 1 % rule.  tools/make_golden_sky.py asserts that it
equals the reference's own function (run around tests/cv2_sky_stub.py) on every golden case."""
import numpy as np
from scipy import ndimage

BRANCHES = ("empty", "no_top", "top")

# OpenCV's tables (hsv_shift = 12): cvRound = rint, 0 at i = 0
with np.errstate(divide="ignore"):
    SDIV = np.rint((255 << 12) / np.arange(256, dtype=np.float64))
    HDIV = np.rint((180 << 12) / (6.0 * np.arange(256, dtype=np.float64)))
SDIV[0] = HDIV[0] = 0
SDIV, HDIV = SDIV.astype(np.int32), HDIV.astype(np.int32)   # every product below stays under 2^31


def to_u8(img):
    """((img + 1) * 127.5).astype(uint8) for fp32 values in [-1, 1]: an fp32 add, an fp32 multiply, truncation"""
    img = np.asarray(img, dtype=np.float32)
    return ((img + np.float32(1)) * np.float32(127.5)).astype(np.uint8)


def to_u8_saturating(img):
    """the product's stated deviation outside [-1, 1]: saturate where the cast wraps, NaN -> 0"""
    img = np.asarray(img, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        y = (img + np.float32(1)) * np.float32(127.5)
        y = np.where(y > 0, np.minimum(y, np.float32(255)), np.float32(0))
    return y.astype(np.uint8)


def hsv_u8(r, g, b):
    """OpenCV's 8-bit RGB -> HSV (H in [0, 180)) on integer arrays: (h, s, v) as int32"""
    r, g, b = (np.asarray(x).astype(np.int32) for x in (r, g, b))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = (d * SDIV[v] + 2048) >> 12
    h0 = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h0 * HDIV[d] + 2048) >> 12   # numpy's >> on signed integers is arithmetic
    h = np.where(h < 0, h + 180, h)
    return h, s, v


def sky_coloured(h, s, v, in_upper):
    blue = (h >= 105) & (h <= 135) & (s >= 50) & (s <= 255) & (v >= 140) & (v <= 255)
    light = (h >= 95) & (h <= 145) & (s >= 5) & (s <= 100) & (v >= 150) & (v <= 255)
    white = (h >= 0) & (h <= 180) & (s >= 0) & (s <= 10) & (v >= 235) & (v <= 255)
    return blue | light | white | (in_upper & (s < 50) & (v > 150))


def classify_u8(u8):
    """(H, W, 3) uint8 RGB -> the bool bitmap before morphology"""
    H = u8.shape[0]
    h, s, v = hsv_u8(u8[..., 0], u8[..., 1], u8[..., 2])
    in_upper = (np.arange(H) < int(H * 0.4))[:, None]
    return sky_coloured(h, s, v, in_upper)


def classify(img_hw3, saturate=False):
    return classify_u8(to_u8_saturating(img_hw3) if saturate else to_u8(img_hw3))


def _box(mask, k, want_all):
    """k x k box OR (want_all False) / AND (True), anchor at the centre, pixels outside the image ignored"""
    H, W = mask.shape
    r = k // 2
    fill = bool(want_all)
    pad = np.full((H + 2 * r, W + 2 * r), fill, dtype=bool)
    pad[r:r + H, r:r + W] = mask
    out = np.full((H, W), fill, dtype=bool)
    for dy in range(k):
        for dx in range(k):
            win = pad[dy:dy + H, dx:dx + W]
            out = (out & win) if want_all else (out | win)
    return out


def dilate7(mask):
    return _box(np.asarray(mask, dtype=bool), 7, False)


def erode7(mask):
    return _box(np.asarray(mask, dtype=bool), 7, True)


def morphology(mask):
    """dilate 7 x 7, then MORPH_OPEN 7 x 7 = erode, dilate"""
    return dilate7(erode7(dilate7(mask)))


def label_roots(mask):
    """(roots int32 (H, W): the smallest linear index of each pixel's 4-connected component, -1 background; count)"""
    mask = np.asarray(mask, dtype=bool)
    labels, n = ndimage.label(mask)
    roots = np.full(mask.shape, -1, dtype=np.int32)
    if n:
        idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
        mins = ndimage.minimum(idx, labels, np.arange(1, n + 1)).astype(np.int64)
        roots[mask] = mins[labels[mask] - 1]
    return roots, int(n)


def select(mask):
    """step 5 on the bool bitmap after morphology -> (sky bool (H, W), stats dict)"""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    labels, n = ndimage.label(mask)
    stats = {"sky_pixels": int(mask.sum()), "components": int(n), "components_top": 0, "components_kept": 0, "branch": "empty"}
    if n == 0:
        return mask, stats
    top = sorted(set(labels[0, :].tolist()) - {0})
    stats["components_top"] = len(top)
    if not top:
        stats["branch"], stats["components_kept"] = "no_top", int(n)
        return mask, stats
    stats["branch"] = "top"
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    kept = [l for l in top if sizes[l] > mask.size * 0.01]
    stats["components_kept"] = len(kept)
    return np.isin(labels, kept), stats


def detect_sky_mask(img_hw3, saturate=False):
    """the whole function: (not_sky int8 (H, W), stats)"""
    sky, stats = select(morphology(classify(img_hw3, saturate)))
    return (~sky).astype(np.int8), stats


def pack_bits(mask):
    """the kernels' bitmap layout: (H, ceil(W / 64)) uint64, pixel x = bit x % 64 of word x / 64"""
    mask = np.asarray(mask, dtype=bool)
    H, W = mask.shape
    WW = (W + 63) // 64
    pad = np.zeros((H, WW * 64), dtype=np.uint64)
    pad[:, :W] = mask
    return (pad.reshape(H, WW, 64) << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64)
