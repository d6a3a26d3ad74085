"""Seeded inputs of the view-matching tests, shared by tests/test_matching.py (CPU), tests/test_matching_gpu.py and
tools/make_golden_matches.py.  A case is a dict: pts (a list of (H, W, 3) fp32 pointmaps), confs / masks (lists or None), pairs (a graph string
or rows (i, j)), pct, subsample.  numpy only."""
import numpy as np

F32 = np.float32
GOLDEN_PATCHES = ((24, 32), (17, 40), (31, 9))  # the three surface patches of the golden file
GOLDEN_CLOUDS = (500, 777)                        # its two unrelated random clouds
GRAPHS = ("complete", "swin", "swin-1", "swin-2", "swin-5", "oneref", "oneref-1")
PREFILTERS = (None, "seq1", "seq3", "cyc1", "cyc2")
GRAPH_SIZES = (1, 2, 5, 8)
COUNTS = (0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 5000)  # candidates per view: the wave, the sort tile of 2048, more than two tiles


def surface(H, W, seed, shift=(0.0, 0.0), step=0.05, noise=0.004):
    """an (H, W, 3) pointmap of one smooth surface z = f(x, y) in a common frame, sampled on a grid moved by `shift`, with noise: two patches
    with overlapping footprints have reciprocal neighbours where they overlap"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    x = xx * step + shift[0] + 0.3 * step * rs.uniform(-1, 1, (H, W))
    y = yy * step + shift[1] + 0.3 * step * rs.uniform(-1, 1, (H, W))
    z = 2.0 + 0.3 * np.sin(1.7 * x) * np.cos(1.3 * y) + noise * rs.standard_normal((H, W))
    return np.stack([x, y, z], -1).astype(F32)


def golden_inputs(seed):
    """the golden file's inputs for one seed: three patches seen from shifted poses, two unrelated clouds"""
    rs = np.random.RandomState(seed)
    shifts = [(0.0, 0.0), (0.11, 0.07), (0.31, -0.12)]
    patches = [surface(H, W, seed * 10 + k, shifts[k]) for k, (H, W) in enumerate(GOLDEN_PATCHES)]
    clouds = [rs.uniform(-1, 1, (n, 3)).astype(F32) for n in GOLDEN_CLOUDS]
    return patches, clouds


def first_n_mask(H, W, n, seed):
    """a bool (H, W) mask with exactly n true pixels at seeded places"""
    m = np.zeros(H * W, bool)
    m[np.random.RandomState(seed).permutation(H * W)[:n]] = True
    return m.reshape(H, W)


def counts_case():
    """ten views of different sizes whose masks leave COUNTS candidates, every pair: the empty view, the one-point view, the wave and tile edges"""
    sizes = {0: (5, 7), 1: (3, 4), 2: (4, 4), 63: (9, 8), 64: (8, 9), 65: (7, 11), 2047: (41, 53), 2048: (50, 44), 2049: (33, 70), 5000: (50, 101)}
    pts, masks = [], []
    for k, n in enumerate(COUNTS):
        H, W = sizes[n]
        pts.append(surface(H, W, 100 + k, (0.013 * k, -0.017 * k), step=2.0 / max(H, W)))
        masks.append(first_n_mask(H, W, n, 200 + k))
    return {"pts": pts, "masks": masks, "pairs": "complete"}


def views_case(n_views, H=12, W=15, pairs="complete", seed=300):
    return {"pts": [surface(H, W, seed + v, (0.02 * v, 0.01 * v)) for v in range(n_views)], "pairs": pairs}


def many_views_case():
    """257 views of 3 points: the view number crosses an 8-bit digit of the sort key"""
    rs = np.random.RandomState(400)
    return {"pts": [rs.uniform(-1, 1, (1, 3, 3)).astype(F32) for _ in range(257)], "pairs": "swin-2"}


def degenerate_cases():
    rs = np.random.RandomState(500)
    base = surface(20, 25, 501)
    same = np.tile(np.array([0.3, -0.2, 1.5], F32), (6, 9, 1))
    plane = surface(21, 23, 502)
    plane[..., 2] = 1.25
    line = np.zeros((1, 300, 3), F32)
    line[0, :, 0] = np.sort(rs.uniform(-1, 1, 300)).astype(F32)
    far = surface(20, 25, 503) + np.array([1e4, -2e4, 3e4], F32)
    out = surface(50, 100, 504, step=0.01)                      # 5000 points, 1 % of them 1000 extents away: the grid is stretched
    flat = out.reshape(-1, 3)
    sel = rs.permutation(5000)[:50]
    flat[sel] += (1000.0 * rs.choice([-1.0, 1.0], (50, 3))).astype(F32)
    dup = surface(16, 16, 505)
    dflat = dup.reshape(-1, 3)
    dflat[rs.permutation(256)[:128]] = dflat[rs.permutation(256)[:128]]  # exact duplicates: ties go to the smaller index
    dup2 = dup.copy()                                                   # and a second view with the same points in another order
    dup2 = dup2.reshape(-1, 3)[rs.permutation(256)].reshape(16, 16, 3)
    return {
        "identical": {"pts": [same, base, same.copy()], "pairs": [(0, 1), (1, 0), (0, 2), (0, 0)]},
        "plane": {"pts": [plane, base], "pairs": "complete"},
        "line": {"pts": [line, base, line[:, ::-1].copy()], "pairs": "complete"},
        "disjoint": {"pts": [base, far], "pairs": [(0, 1), (1, 0)]},
        "outliers": {"pts": [out, surface(40, 60, 506, step=0.012)], "pairs": [(0, 1), (1, 1), (0, 0)]},
        "duplicates": {"pts": [dup, dup2, base], "pairs": [(0, 1), (1, 0), (0, 0), (1, 2)]},
    }


def candidate_cases():
    rs = np.random.RandomState(600)
    pts = [surface(7, 10, 601), surface(7, 10, 602, (0.02, 0.01)), surface(9, 6, 603, (0.01, 0.03), step=0.06)]
    conf = [rs.uniform(1, 5, p.shape[:2]).astype(F32) for p in pts]
    shared = [c.copy() for c in conf]
    for c in shared:  # the threshold value is shared by several pixels: rank 0.5 (n - 1) lands on a run of equal values
        flat = c.reshape(-1)
        order = np.argsort(flat)
        flat[order[len(flat) // 2 - 3:len(flat) // 2 + 4]] = flat[order[len(flat) // 2]]
    nan_conf = [c.copy() for c in conf]
    nan_conf[1][3, 4] = np.nan
    masks = [rs.uniform(0, 1, p.shape[:2]) < 0.6 for p in pts]
    one = [m.copy() for m in masks]
    one[2][:] = False
    one[2][4, 5] = True
    cases = {f"subsample{s}": {"pts": pts, "confs": conf, "pairs": "complete", "subsample": s} for s in (1, 2, 3)}
    cases["shared_threshold"] = {"pts": pts, "confs": shared, "pairs": "complete", "pct": 50}
    cases["percentile"] = {"pts": pts, "confs": conf, "pairs": "complete", "pct": 37.5, "subsample": 2}
    cases["nan_conf"] = {"pts": pts, "confs": nan_conf, "pairs": "complete", "pct": 10}
    cases["nan_conf_pct0"] = {"pts": pts, "confs": nan_conf, "pairs": "complete"}
    cases["mask"] = {"pts": pts, "confs": conf, "masks": masks, "pairs": "complete", "pct": 20}
    cases["one_pixel"] = {"pts": pts, "masks": one, "pairs": "complete"}
    return cases


def chunk_case():
    return views_case(6, 20, 30, "complete", seed=700)
