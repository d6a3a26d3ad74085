"""Plain-numpy restatement of the triangle rasteriser (fast3r_amd/csrc/f3r_raster.hip; the rule is the "triangle rasteriser" section of
include/f3r.h): fp64, every operation a numpy operation of its own, painter-free -- per pixel the minimum over the triangles that cover
its centre of (bits of the fp32 depth, index_base + face).  Keys are window rows (row 0 at the bottom) as in tests/render_ref.py, whose
splat and resolve compose with `raster`.  Also the host side of camera_meshes and auto_cam_size, written from their description."""
import numpy as np

import render_ref as R

EMPTY = R.EMPTY


def first_center_ge(t, hi):
    """the smallest i with i + 0.5 >= t, within [0, hi]: a binary search over the centres is the comparison's own answer"""
    return np.searchsorted(np.arange(hi) + 0.5, t, "left")


def project(vertices, cam, W, H):
    """-> (ok, x_w, y_w, d) per vertex"""
    V = np.asarray(cam.view, dtype=np.float64).reshape(3, 4)
    p = vertices.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        e = [((V[r, 0] * x + V[r, 1] * y) + V[r, 2] * z) + V[r, 3] for r in range(3)]
        d = -e[2]
        px = np.float64(cam.sx) * e[0] + np.float64(cam.cx) * d
        py = np.float64(cam.sy) * e[1] + np.float64(cam.cy) * d
        xw = (px / d + 1.0) * (W * 0.5)
        yw = (py / d + 1.0) * (H * 0.5)
        ok = (d >= cam.znear) & np.isfinite(xw) & np.isfinite(yw)
    return ok, xw, yw, d


class Setup:
    """the triangles of faces[f0:f1] that are not skipped: .f (their face numbers), window corners, r, dmin, dmax, A and the pixel box"""

    def __init__(self, vertices, faces, f0, f1, cam, W, H):
        nv = len(vertices)
        fc = np.asarray(faces[f0:f1]).astype(np.int64)
        inside = ((fc >= 0) & (fc < nv)).all(axis=1)                                      # the indices first: nothing is gathered before
        ok, xw, yw, d = project(vertices, cam, W, H)
        safe = np.where(inside[:, None], fc, 0)
        keep = inside & ok[safe].all(axis=1)
        x, y, dd = xw[safe], yw[safe], d[safe]
        with np.errstate(all="ignore"):
            A = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
            keep &= (A != 0) & np.isfinite(A)
        sel = np.flatnonzero(keep)
        self.f = sel + f0
        self.x, self.y, d3, self.A = x[sel], y[sel], dd[sel], A[sel]
        self.r = 1.0 / d3
        self.dmin, self.dmax = d3.min(axis=1, initial=np.inf), d3.max(axis=1, initial=-np.inf)
        self.i0 = first_center_ge(self.x.min(axis=1, initial=np.inf), W)
        self.i1 = np.minimum(first_center_ge(self.x.max(axis=1, initial=-np.inf), W) + 1, W)
        self.j0 = first_center_ge(self.y.min(axis=1, initial=np.inf), H)
        self.j1 = np.minimum(first_center_ge(self.y.max(axis=1, initial=-np.inf), H) + 1, H)
        self.pixels = np.where((self.i1 > self.i0) & (self.j1 > self.j0), (self.i1 - self.i0) * (self.j1 - self.j0), 0)

    def shade(self, t, i, j):
        """triangles t (an index array, or one index) at pixels (i, j), broadcast against each other -> (covered, fp32 depth)"""
        x, y, r = self.x[t], self.y[t], self.r[t]
        x0, x1, x2, y0, y1, y2 = x[..., 0], x[..., 1], x[..., 2], y[..., 0], y[..., 1], y[..., 2]
        cx, cy = i + 0.5, j + 0.5
        with np.errstate(all="ignore"):
            w0 = (x2 - x1) * (cy - y1) - (y2 - y1) * (cx - x1)
            w1 = (x0 - x2) * (cy - y2) - (y0 - y2) * (cx - x2)
            w2 = (x1 - x0) * (cy - y0) - (y1 - y0) * (cx - x0)
            covered = np.where(self.A[t] > 0, (w0 >= 0) & (w1 >= 0) & (w2 >= 0), (w0 <= 0) & (w1 <= 0) & (w2 <= 0))
            inv = (w0 * r[..., 0] + w1 * r[..., 1]) + w2 * r[..., 2]
            dd = ((w0 + w1) + w2) / inv
            dd = np.where(dd >= self.dmin[t], dd, self.dmin[t])
            dd = np.where(dd > self.dmax[t], self.dmax[t], dd)
            return covered, dd.astype(np.float32)


def _key(df, index):
    return (df.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index.astype(np.uint64)


def raster(keys, vertices, faces, cam, f0=0, f1=None, index_base=0, small=64):
    """faces [f0, f1) into keys (H, W) uint64, window rows.  -> the Setup (its .pixels tells which path the kernel takes per triangle).
    `small` only chooses how the loops below are arranged -- the keys do not depend on it."""
    H, W = keys.shape
    f1 = len(faces) if f1 is None else f1
    s = Setup(vertices, faces, f0, f1, cam, W, H)
    flat = keys.reshape(-1)
    lo = np.flatnonzero((s.pixels > 0) & (s.pixels <= small))
    if len(lo):                                                                           # all small boxes at once, pixel offset by pixel offset
        bw, bh = s.i1[lo] - s.i0[lo], s.j1[lo] - s.j0[lo]
        for dj in range(int(bh.max())):
            for di in range(int(bw.max())):
                m = (dj < bh) & (di < bw)
                if not m.any():
                    continue
                t, i, j = lo[m], s.i0[lo][m] + di, s.j0[lo][m] + dj
                covered, df = s.shade(t, i.astype(np.float64), j.astype(np.float64))
                key = _key(df, index_base + s.f[t])
                np.minimum.at(flat, (j * W + i)[covered], key[covered])
    for t in np.flatnonzero(s.pixels > small):                                            # a large box: all its pixels at once
        j, i = np.mgrid[s.j0[t]:s.j1[t], s.i0[t]:s.i1[t]]
        covered, df = s.shade(t, i.astype(np.float64), j.astype(np.float64))
        key = _key(df, np.full(df.shape, index_base + s.f[t]))
        np.minimum.at(flat, (j * W + i)[covered], key[covered])
    return s


def render(vertices, faces, face_colors, cam, W, H, points=None, colors=None, point_size=5.0, background=(255, 255, 255)):
    """render_mesh restated: points take indices [0, n), faces n + f; resolve over the concatenated colours.  -> (image, depth, keys)"""
    keys = np.full((H, W), EMPTY, dtype=np.uint64)
    n = 0 if points is None else len(points)
    if n:
        R.splat(keys, points, 0, n, cam, point_size)
    raster(keys, vertices, faces, cam, index_base=n)
    table = face_colors if n == 0 else np.concatenate([colors, face_colors])
    image, depth = R.resolve(keys, table, background)
    return image, depth, keys[::-1]


# ------------------------------------------------------------------------------------------------------------------- cameras of a scene
def pdist(x):
    """the condensed Euclidean distance vector of scipy.spatial.distance.pdist: pairs (i, j), i < j, row-major; sqrt of the sum of the
    squared differences added in coordinate order"""
    x = np.asarray(x, dtype=np.float64)
    i, j = np.triu_indices(len(x), k=1)
    d = x[i] - x[j]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
