"""Plain-numpy restatement of the point-cloud export (fast3r_amd/cloud.py), in this project's own words: the notebook's
`export_combined_ply` (notebooks/demo_multiview.ipynb) and the two Open3D algorithms it calls, VoxelDownSample and FarthestPointDownSample,
as include/f3r.h describes them.  Every floating-point operation is written out in the order the kernels use, so comparisons are bit for
bit.  Open3D and trimesh have never run here: Open3D's binary is unpinned (docs/rows_f.md)."""
import warnings

import numpy as np

F32 = np.float32


def color_u8(img):
    """trunc((img + 1.0f) * 127.5f) as two rounded fp32 operations, saturated to [0, 255], NaN -> 0 (the notebook's cast wraps instead)"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = (np.asarray(img, dtype=F32) + F32(1.0)) * F32(127.5)
        out = np.zeros(y.shape, dtype=np.uint8)
        mid = (y > 0) & (y < 255)
        out[mid] = y[mid].astype(np.int32).astype(np.uint8)
        out[y >= 255] = 255
    return out


def threshold(conf, percentile):
    """np.percentile of the fp32 confidences (method 'linear'); NaN if any confidence is NaN"""
    with np.errstate(invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.percentile(np.asarray(conf, dtype=F32), percentile)


def combine(preds, views, pts_key="pts3d_local_aligned_to_global", conf_key="conf_local", percentile=0, flip_axes=False, sample=0):
    """the notebook's loop over views: (points (M, 3) fp32, colors (M, 3) uint8), or (None, None) when nothing is kept.  preds / views hold
    numpy arrays with a batch axis: pts (B, H, W, 3), conf (B, H, W), img (B, 3, H, W)."""
    all_p, all_c = [], []
    for pred, view in zip(preds, views):
        pts = np.asarray(pred[pts_key][sample], dtype=F32).reshape(-1, 3)
        conf = np.asarray(pred[conf_key][sample], dtype=F32).reshape(-1)
        img = np.asarray(view["img"][sample], dtype=F32).reshape(3, -1).T
        with np.errstate(invalid="ignore"):
            mask = conf > threshold(conf, percentile)
        p = pts[mask].copy()
        if flip_axes:
            p = p[:, [0, 2, 1]]
            p[:, 2] = -p[:, 2]
        all_p.append(p)
        all_c.append(color_u8(img[mask]))
    p, c = np.vstack(all_p), np.vstack(all_c)
    if len(p) == 0:
        return None, None
    return np.ascontiguousarray(p, dtype=F32), np.ascontiguousarray(c, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- voxel
def heuristic_voxel_size(points, max_num_points):
    p = np.asarray(points, dtype=np.float64)
    extent = p.max(axis=0) - p.min(axis=0)
    return (float(extent[0]) * float(extent[1]) * float(extent[2]) / max_num_points) ** (1 / 3)


def voxel_indices(points, voxel_size):
    """floor((p - (min_bound - 0.5 voxel_size)) / voxel_size) per axis in fp64 -> int64 (n, 3)"""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    vmin = p.min(axis=0) - 0.5 * float(voxel_size)
    return np.floor((p - vmin) / float(voxel_size)).astype(np.int64)


def voxel_down_sample(points, colors, voxel_size):
    """-> (points (M, 3) fp32, colors (M, 3) uint8 or None, counts (M,) int32), voxels in ascending (x, y, z) index order.  Per voxel the
    sums run over its points in original index order, one addition after the other, as Open3D's accumulator does."""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    idx = voxel_indices(points, voxel_size)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))           # stable: equal keys stay in index order
    sidx = idx[order]
    head = np.ones(len(order), dtype=bool)
    head[1:] = (sidx[1:] != sidx[:-1]).any(axis=1)
    group = np.cumsum(head) - 1
    m = int(group[-1]) + 1
    starts = np.flatnonzero(head)
    counts = np.diff(np.append(starts, len(order)))
    rank = np.arange(len(order)) - starts[group]
    c64 = None if colors is None else np.asarray(colors, dtype=np.uint8).astype(np.float64) / 255.0
    sp, sc = np.zeros((m, 3)), np.zeros((m, 3))
    for r in range(int(counts.max())):                              # round r adds every voxel's r-th point: sequential within a voxel
        sel = rank == r
        g, i = group[sel], order[sel]
        sp[g] += p[i]
        if c64 is not None:
            sc[g] += c64[i]
    cnt = counts.astype(np.float64)[:, None]
    out_p = (sp / cnt).astype(F32)
    out_c = None if c64 is None else (sc / cnt * 255.0).astype(np.int32).astype(np.uint8)
    return out_p, out_c, counts.astype(np.int32)


def voxel_down_sample_loop(points, colors, voxel_size):
    """the same with one Python loop over the points in index order and a dict, the way Open3D's hash map accumulates: a check of the
    vectorised form above"""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    idx = voxel_indices(points, voxel_size)
    acc = {}
    for i in range(len(p)):
        a = acc.setdefault(tuple(idx[i]), [np.zeros(3), np.zeros(3), 0])
        a[0] = a[0] + p[i]
        if colors is not None:
            a[1] = a[1] + np.asarray(colors[i], dtype=np.uint8).astype(np.float64) / 255.0
        a[2] += 1
    keys = sorted(acc)
    out_p = np.array([acc[k][0] / float(acc[k][2]) for k in keys]).astype(F32)
    out_c = None if colors is None else np.array([acc[k][1] / float(acc[k][2]) * 255.0 for k in keys]).astype(np.int32).astype(np.uint8)
    return out_p, out_c, np.array([acc[k][2] for k in keys], dtype=np.int32)


def quirk_pairs(k_max=8):
    """(c, k): k equal colours c whose fp64 mean, formed as above, truncates to c - 1"""
    out = []
    for k in range(1, k_max + 1):
        for c in range(256):
            s = 0.0
            for _ in range(k):
                s += c / 255.0
            if int(s / float(k) * 255.0) != c:
                out.append((c, k))
    return out


def key_bits(points, voxel_size):
    """per axis ceil(log2(cells)), cells = floor(extent / voxel_size + 0.5) + 1 (Python floats on the fp64-widened bounds)"""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    bits = []
    for a in range(3):
        extent = float(p[:, a].max()) - float(p[:, a].min())
        cells = int(np.floor(extent / float(voxel_size) + 0.5)) + 1
        bits.append(int(cells - 1).bit_length())
    return bits


# ------------------------------------------------------------------------------------------------------------------- farthest point
def farthest_point_down_sample(points, num_samples, start_index=0):
    """-> selected int32 (num_samples,) in selection order"""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    d = np.full(len(p), np.inf)
    far = int(start_index)
    selected = []
    for _ in range(int(num_samples)):
        selected.append(far)
        diff = p - p[far]
        d = np.minimum(d, (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        if d.max() > 0:
            far = int(np.argmax(d))                                  # the first = smallest index attaining the maximum
    return np.array(selected, dtype=np.int32)


def fps_ties(points, num_samples, start_index=0):
    """in how many of the iterations more than one point attains the maximum distance"""
    p = np.asarray(points, dtype=F32).astype(np.float64)
    d = np.full(len(p), np.inf)
    far, ties = int(start_index), 0
    for _ in range(int(num_samples)):
        d = np.minimum(d, ((p - p[far]) ** 2).sum(axis=1))
        if d.max() > 0:
            ties += int((d == d.max()).sum() > 1)
            far = int(np.argmax(d))
    return ties


def select_by_index(points, colors, selected, order="index"):
    """Open3D's SelectByIndex builds a mask: original index order, repeats collapsed; order='selection': a gather, repeats kept"""
    sel = np.unique(selected) if order == "index" else np.asarray(selected)
    return points[sel], (None if colors is None else colors[sel])


def downsample(points, colors, max_num_points, strategy, voxel_size=None, order="index"):
    if max_num_points is None or len(points) <= max_num_points:
        return points, colors
    if strategy == "voxel":
        vs = heuristic_voxel_size(points, max_num_points) if voxel_size is None else voxel_size
        return voxel_down_sample(points, colors, vs)[:2]
    if strategy == "farthest_point":
        return select_by_index(points, colors, farthest_point_down_sample(points, max_num_points), order)
    raise ValueError(f"Unsupported sampling strategy: {strategy}")


# ------------------------------------------------------------------------------------------------------------------- PLY
def parse_ply(raw):
    """reader of fast3r_amd.scene's layout -> (points (M, 3) fp32, colors (M, 3) uint8)"""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n = int(lines[2].split()[2])
    assert lines[3:9] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                          "property uchar blue"]
    rec = np.frombuffer(raw, np.dtype([("p", "<f4", 3), ("c", "u1", 3)]), n, end)
    assert len(raw) == end + 15 * n
    return rec["p"].copy(), rec["c"].copy()
