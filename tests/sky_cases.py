"""TEST INFRASTRUCTURE: the seeded procedural scenes of the sky-detection golden (tests/golden/sky_cases.pt, tools/make_golden_sky.py) and
the stress bitmaps of the labelling tests.  A scene is painted as 8-bit RGB and normalised the way ImgNorm does ((u / 255 - 0.5) / 0.5 in
fp32), which is what real inputs look like; the recipes are seeded, so the golden stores results and checksums, never images."""
import hashlib

import numpy as np

SHAPES = ((48, 64), (64, 48), (37, 53), (1, 64), (64, 1), (7, 7), (96, 128), (224, 288))
SCENES = ("indoor", "outdoor", "outdoor_lake", "top_pixel", "lake_only", "all_sky", "noise", "bluish_noise", "partial_top")
CASES = tuple((scene, H, W) for H, W in SHAPES for scene in SCENES)

SKY_BLUE = (100, 150, 230)
WARM = ((150, 100, 60), (120, 80, 50), (170, 130, 90), (90, 70, 60), (60, 50, 45))
GROUND = ((70, 110, 50), (110, 90, 60), (85, 120, 65))


def case_name(scene, H, W):
    return f"{scene}_{H}x{W}"


def case_seed(scene, H, W):
    return int.from_bytes(hashlib.sha256(case_name(scene, H, W).encode()).digest()[:4], "little")


def _blocks(rng, H, W, palette):
    """a patchwork of palette colours with +-4 of noise"""
    u = np.empty((H, W, 3), dtype=np.int64)
    bh, bw = max(1, H // 4), max(1, W // 5)
    for y0 in range(0, H, bh):
        for x0 in range(0, W, bw):
            u[y0:y0 + bh, x0:x0 + bw] = palette[rng.integers(len(palette))]
    return u + rng.integers(-4, 5, size=(H, W, 3))


def _paint_sky(u, rng, ys, xs):
    region = u[ys, xs]
    region[...] = np.asarray(SKY_BLUE) + rng.integers(-6, 7, size=region.shape)


def paint(scene, H, W):
    """the scene as (H, W, 3) uint8"""
    rng = np.random.default_rng(case_seed(scene, H, W))
    if scene == "noise":
        return rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8)
    if scene == "bluish_noise":
        u = rng.integers(0, 256, size=(H, W, 3))
        u[..., 2] = np.maximum(u[..., 2], rng.integers(128, 256, size=(H, W)))
        return u.astype(np.uint8)
    u = _blocks(rng, H, W, WARM)
    horizon = max(1, int(H * 0.45))
    if scene in ("outdoor", "outdoor_lake"):
        u[horizon:] = _blocks(rng, H, W, GROUND)[horizon:]
        _paint_sky(u, rng, slice(0, horizon), slice(0, W))
    if scene in ("outdoor_lake", "lake_only"):
        y0, y1 = min(H - 1, int(H * 0.7)), max(min(H - 1, int(H * 0.7)) + 1, int(H * 0.85))
        _paint_sky(u, rng, slice(y0, y1), slice(W // 5, max(W // 5 + 1, W // 2)))
    if scene == "top_pixel":
        u[0, W // 2] = SKY_BLUE
    if scene == "all_sky":
        _paint_sky(u, rng, slice(0, H), slice(0, W))
    if scene == "partial_top":   # a large sky region on the left of the top rows, and one sky pixel on row 0 far to its right
        _paint_sky(u, rng, slice(0, horizon), slice(0, max(1, W // 2)))
        if W - 5 > W // 2 + 8:
            u[0, W - 5] = SKY_BLUE
    return np.clip(u, 0, 255).astype(np.uint8)


def normalise(u8):
    """ImgNorm: ToTensor + Normalize(0.5, 0.5) in fp32"""
    return ((u8.astype(np.float32) / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)


def build(scene, H, W):
    """the case's input: (H, W, 3) float32 in [-1, 1]"""
    return normalise(paint(scene, H, W))


def checksum(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------------- labelling stress bitmaps
def spiral(H, W):
    """a one-pixel-wide rectangular spiral with one-pixel gaps, walked inwards from (0, 0): ONE component that is a single long path across
    every tile border"""
    m = np.zeros((H, W), dtype=bool)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = True

    def free(yy, xx):
        return not (0 <= yy < H and 0 <= xx < W) or not m[yy, xx]
    while True:
        for _ in range(2):
            ny, nx = y + dy, x + dx
            if 0 <= ny < H and 0 <= nx < W and not m[ny, nx] and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy   # turn right
        else:
            return m
        y, x = ny, nx
        m[y, x] = True


def serpentine(H, W):
    """full rows on even lines joined alternately at the right and the left end: one component, a path of H * W / 2 pixels"""
    m = np.zeros((H, W), dtype=bool)
    m[0::2] = True
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = True
    return m


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (y + x) % 2 == 0


def comb(H, W):
    """teeth on even columns from row 0 down, joined only by the full last row"""
    m = np.zeros((H, W), dtype=bool)
    m[:, 0::2] = True
    m[H - 1] = True
    return m


def diagonal_pair(H, W):
    """two squares that touch only at a corner: two components under 4-connectivity"""
    m = np.zeros((H, W), dtype=bool)
    cy, cx = H // 2, W // 2
    m[max(0, cy - 3):cy, max(0, cx - 3):cx] = True
    m[cy:cy + 3, cx:cx + 3] = True
    return m


def noise(H, W, density, seed):
    return np.random.default_rng(seed).random((H, W)) < density


def stress_bitmaps():
    """name -> bool bitmap: shapes morphology never emits"""
    H, W = 96, 128
    out = {
        "spiral": spiral(H, W), "serpentine": serpentine(H, W), "checkerboard": checkerboard(H, W), "comb": comb(H, W),
        "full": np.ones((H, W), dtype=bool), "empty": np.zeros((H, W), dtype=bool),
        "diagonal_pair": diagonal_pair(H, W), "noise40": noise(H, W, 0.40, 40), "noise60": noise(H, W, 0.60, 60),
        "row_1xW": noise(1, 200, 0.6, 1), "col_Hx1": noise(200, 1, 0.6, 2),
        "spiral_odd": spiral(37, 131), "serpentine_odd": serpentine(45, 65), "noise60_odd": noise(67, 193, 0.60, 3),
    }
    r0 = np.zeros((H, W), dtype=bool)
    r0[0] = True
    c0 = np.zeros((H, W), dtype=bool)
    c0[:, 0] = True
    out["row0_only"], out["col0_only"] = r0, c0
    return out
