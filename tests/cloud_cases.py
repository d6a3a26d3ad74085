"""Seeded recipes for the point-cloud export tests (tests/test_cloud.py, tests/test_cloud_gpu.py): everything is numpy, built from a
RandomState, so the CPU self-checks and the GPU comparisons see the same inputs."""
import functools

import numpy as np

import cloud_ref as R
from fast3r_amd import _lib

T = _lib.CLOUD_TILE
ST = _lib.CLOUD_SORT_TILE
FT = _lib.CLOUD_FPS_TILE
F32 = np.float32

PTS_KEY, CONF_KEY = "pts3d_local_aligned_to_global", "conf_local"


def shape_of(n):
    """(H, W) with H W = n, H the largest divisor not above sqrt(n)"""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


COMBINE_PIXELS = (1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17)
COMBINE_SPECIAL = ("constant", "nan", "zeros_inf")


def combine_case(seed=5, B=2):
    """views of COMBINE_PIXELS pixels with different (H, W), then three special views: constant confidence, one NaN confidence, and
    -0.0 / +0.0 / +inf confidences.  Image values leave [-1, 1] in places and hold one NaN.  -> (preds, views) of numpy arrays with batch B"""
    rs = np.random.RandomState(seed)
    preds, views = [], []
    shapes = [shape_of(n) for n in COMBINE_PIXELS] + [(6, 11), (8, 9), (9, 8)]
    for v, (H, W) in enumerate(shapes):
        conf = (1.0 + np.exp(rs.randn(B, H, W))).astype(F32)
        conf = np.round(conf, 1) if v % 2 else conf                  # rounded: ties at the threshold
        kind = COMBINE_SPECIAL[v - len(COMBINE_PIXELS)] if v >= len(COMBINE_PIXELS) else None
        if kind == "constant":
            conf[:] = F32(2.5)
        elif kind == "nan":
            conf[:, 3, 4] = np.nan
        elif kind == "zeros_inf":
            flat = conf.reshape(B, -1)
            flat[:, 0:20:2] = F32(-0.0)
            flat[:, 1:20:2] = F32(0.0)
            flat[:, 30:33] = np.inf
        img = (rs.rand(B, 3, H, W) * 2.0 - 1.0).astype(F32)
        if H * W >= 63:
            flat = img.reshape(B, 3, -1)
            flat[:, 0, 5], flat[:, 1, 6], flat[:, 2, 7], flat[:, 0, 8], flat[:, 1, 9] = -1.5, 1.25, 3.0, -1.0, 1.0
            flat[:, 2, 10] = np.nan
        preds.append({PTS_KEY: rs.randn(B, H, W, 3).astype(F32), CONF_KEY: conf})
        views.append({"img": img})
    return preds, views


# ------------------------------------------------------------------------------------------------------------------- voxel
def random_cloud(n, seed, box=(4.0, 3.0, 2.0)):
    rs = np.random.RandomState(seed)
    return (rs.rand(n, 3) * np.asarray(box)).astype(F32), rs.randint(0, 256, (n, 3)).astype(np.uint8)


VOXEL_SIZES = (1, 2, 63, 64, 65, ST - 1, ST, ST + 1, 3 * ST + 211)


def one_voxel(n=5000, seed=11):
    """every point in one voxel of size 1: a run that spans sort tiles"""
    rs = np.random.RandomState(seed)
    return (10.0 + 0.4 * rs.rand(n, 3)).astype(F32), rs.randint(0, 256, (n, 3)).astype(np.uint8), 1.0


def own_voxels(seed=12, n=None):
    """the 12 x 11 x 10 integer lattice, shuffled (its first n points): with voxel size 1 every point is its own voxel"""
    rs = np.random.RandomState(seed)
    g = np.stack(np.meshgrid(np.arange(12), np.arange(11), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
    g = g[rs.permutation(len(g))][:n]
    return g.astype(F32), rs.randint(0, 256, (len(g), 3)).astype(np.uint8), 1.0


# as many voxels as points, around the T = 1024 heads of one tile of the head compaction
assert T == 1024
own_voxels_1023 = functools.partial(own_voxels, n=1023)
own_voxels_1024 = functools.partial(own_voxels, n=1024)
own_voxels_1025 = functools.partial(own_voxels, n=1025)


def on_boundaries(seed=13, n=700):
    """coordinates that are multiples of 1 / 8 with voxel size 1 / 4 and the minimum at 0: (p - vmin) / voxel_size is exactly an integer
    or an integer and a half"""
    rs = np.random.RandomState(seed)
    p = rs.randint(0, 33, (n, 3)).astype(F32) / F32(8.0)
    p[0] = 0.0
    return p, rs.randint(0, 256, (n, 3)).astype(np.uint8), 0.25


def duplicates(seed=14, n=900):
    rs = np.random.RandomState(seed)
    base = (rs.rand(40, 3) * 3.0).astype(F32)
    return base[rs.randint(0, 40, n)], rs.randint(0, 256, (n, 3)).astype(np.uint8), 0.3


def small_integers(seed=15, n=1500):
    """small integer coordinates and voxel size 2: no fp64 sum rounds, so any grouping gives the same sums"""
    rs = np.random.RandomState(seed)
    return rs.randint(0, 16, (n, 3)).astype(F32), rs.randint(0, 256, (n, 3)).astype(np.uint8), 2.0


def quirk_colors():
    """one voxel per (c, k): k points of one colour c in cell j + 1 of a row of unit voxels -- the colours 0 and 255, and every quirk pair
    with k <= 8 (cloud_ref.quirk_pairs); a point of colour 7 at the origin anchors the grid and is voxel 0.
    -> (points, colors, voxel_size, [(c, k)] of voxels 1, 2, ..)"""
    pairs = [(0, 3), (255, 1), (255, 7)] + R.quirk_pairs(8)
    pts, cols = [[0.0, 0.0, 0.0]], [[7, 7, 7]]
    for j, (c, k) in enumerate(pairs):
        for i in range(k):
            pts.append([j + 0.5 + 0.05 * i, 0.75, 0.75])              # index floor(x + 0.5) = j + 1
            cols.append([c, c, c])
    return np.asarray(pts, dtype=F32), np.asarray(cols, dtype=np.uint8), 1.0, pairs


BIT_CASES = {8: (3, 3, 2), 9: (3, 3, 3), 16: (6, 5, 5), 17: (6, 6, 5), 24: (8, 8, 8), 25: (9, 8, 8), 40: (14, 13, 13), 41: (14, 14, 13)}


def bits_cloud(bits, seed=16, n=600):
    """an anisotropic box whose axis a spans 2^bits[a] - 1 unit voxels: the key has exactly sum(bits) bits.  Both corners are present,
    and a third of the points repeat earlier ones with a small shift, so voxels hold several points."""
    rs = np.random.RandomState(seed + sum(bits))
    top = np.asarray([2 ** b - 1 for b in bits], dtype=np.float64)
    p = np.floor(rs.rand(n, 3) * (top + 1.0)) + 0.1 * rs.rand(n, 3)
    p = np.minimum(p, top)
    p[n // 3 * 2:] = p[:n - n // 3 * 2] + 0.01
    p = np.minimum(p, top)
    p[0], p[1] = 0.0, top
    return p.astype(F32), rs.randint(0, 256, (n, 3)).astype(np.uint8), 1.0


# ------------------------------------------------------------------------------------------------------------------- farthest point
FPS_SIZES = ((1, 1), (64, 64), (65, 65), (1025, 100))


def lattice():
    """the 5 x 5 x 5 integer lattice: most iterations have several points at the maximum distance"""
    return np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(5), indexing="ij"), -1).reshape(-1, 3).astype(F32)


def few_distinct(seed=21, n=500, distinct=10):
    rs = np.random.RandomState(seed)
    base = rs.randn(distinct, 3).astype(F32)
    pick = rs.randint(0, distinct, n)
    pick[:distinct] = rs.permutation(distinct)                        # every one of them occurs
    return base[pick], rs.randint(0, 256, (n, 3)).astype(np.uint8)
