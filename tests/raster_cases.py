"""Seeded recipes for the triangle rasteriser's tests (tests/test_raster.py on the restatement, tests/test_raster_gpu.py on the GPU).
Triangles are given in window coordinates (x_w, y_w, depth) of the identity camera below and turned into fp32 vertices: x = (2 x_w / W
- 1) d, y = (2 y_w / H - 1) d, z = -d.  On 64 x 48 with d a power of two, x_w any multiple of 1 / 2 and y_w = j + 0.5 with j = 1 (mod 3)
come back exactly: the cases that put a vertex on a pixel centre or an edge through a row of centres use those."""
import numpy as np

import render_ref as R

F32 = np.float32
IDENTITY = R.Cam((1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0), 1.0, 1.0, 0.0, 0.0, 0.05)
VIEWPORTS = [(37, 23), (64, 48)]


def window_mesh(tris, W, H):
    """tris: a list of triangles, each three (x_w, y_w, d) -> (vertices (3 T, 3) fp32, faces (T, 3) int64), three vertices per triangle"""
    t = np.asarray(tris, dtype=np.float64).reshape(-1, 3)
    d = t[:, 2]
    v = np.stack([(2.0 * t[:, 0] / W - 1.0) * d, (2.0 * t[:, 1] / H - 1.0) * d, -d], axis=1).astype(F32)
    return v, np.arange(len(v), dtype=np.int64).reshape(-1, 3)


def colors_of(n, seed=0):
    """distinct colours, none of them white"""
    return np.stack([np.arange(n) % 251, (np.arange(n) // 251) % 251, (np.arange(n) * 7 + seed) % 251], axis=1).astype(np.uint8)


def single_triangles(W, H):
    """name -> one triangle in window coordinates.  On 64 x 48 the named properties hold exactly (test_raster.py asserts them)."""
    c = {
        "no centre": [(10.1, 7.1, 1), (10.4, 7.1, 1), (10.1, 7.4, 1)],
        "one centre": [(10.2, 7.2, 1), (10.9, 7.3, 2), (10.4, 7.9, 1)],
        "vertex on a centre": [(10.5, 7.5, 1), (14.25, 8.0, 1), (11.0, 12.5, 2)],
        "edge through a row of centres": [(3.5, 4.5, 1), (20.5, 4.5, 1), (10.0, 12.0, 1)],
        "edge through a column of centres": [(6.5, 1.5, 2), (6.5, 19.5, 2), (15.0, 9.0, 2)],
        "wholly outside": [(W + 5.0, 3.0, 1), (W + 9.0, 4.0, 1), (W + 6.0, 9.0, 1)],
        "a million pixels outside": [(-1e6, -1e6, 1), (1e6, -5e5, 2), (W / 2, 1e6, 1)],
        "whole viewport": [(-5.0, -5.0, 2), (2.0 * W + 10, -5.0, 2), (-5.0, 2.0 * H + 10, 2)],
    }
    for name, (ex, ey) in {"left": (0, H / 2), "right": (W, H / 2), "bottom": (W / 2, 0), "top": (W / 2, H), "bottom left": (0, 0),
                           "top left": (0, H), "bottom right": (W, 0), "top right": (W, H)}.items():
        c["across " + name] = [(ex - 4.3, ey - 3.1, 1), (ex + 5.2, ey - 2.4, 2), (ex + 0.6, ey + 4.7, 1)]
    return c


def skipped_mesh(W, H):
    """-> (vertices, faces, number of faces that draw): one good triangle first, then triangles that must be skipped -- each would cover
    pixels if it were drawn as given"""
    good = [(5.0, 5.0, 1), (15.0, 6.0, 1), (8.0, 14.0, 1)]
    v, f = window_mesh([good,
                        [(2.0, 2.0, 0.04), (20.0, 3.0, 1), (9.0, 18.0, 1)],                # one vertex nearer than znear
                        [(2.0, 6.0, 1), (10.0, 6.0, 1), (18.0, 6.0, 1)],                   # collinear: one y_w, so A is exactly 0 on any viewport
                        [(2.0, 2.0, 1), (2.0, 2.0, 1), (18.0, 10.0, 1)],                   # a repeated vertex
                        [(2.0, 2.0, 1), (20.0, 3.0, 1), (9.0, 18.0, 1)],                   # gets a NaN below
                        [(2.0, 2.0, 1), (20.0, 3.0, 1), (9.0, 18.0, 1)],                   # gets an inf below
                        [(2.0, 2.0, 1), (20.0, 3.0, 1), (9.0, 18.0, 1)],                   # index -1 below
                        [(2.0, 2.0, 1), (20.0, 3.0, 1), (9.0, 18.0, 1)]], W, H)            # index nv below
    v[4 * 3 + 1, 0] = np.nan
    v[5 * 3 + 2, 1] = np.inf
    f[3] = [9, 9, 11]                                                                      # repeated by index as well as by value
    f[6, 1] = -1
    f[7, 2] = len(v)
    return v, f, 1


def box_recipe(W, H, small):
    """triangles whose pixel boxes hold small - 1, small, small + 1 pixels (63 = 9 x 7, 64 = 8 x 8, 65 = 13 x 5 for small = 64), each
    covering most of its box -> (vertices, faces, the three counts)"""
    assert small == 64 and W >= 30 and H >= 21
    tris, want = [], []
    for (bw, bh), (x, y) in zip([(9, 7), (8, 8), (13, 5)], [(1, 1), (12, 2), (22, 12)]):
        x0, x1, y0, y1 = x + 0.2, x + bw - 1 + 0.3, y + 0.2, y + bh - 1 + 0.3
        tris.append([(x0, y0, 1), (x1, y0 + 0.1, 2), (x0 + 0.1, y1, 1)])
        want.append(bw * bh)
    v, f = window_mesh(tris, W, H)
    return v, f, want


def random_triangles(n, seed, W, H, size=3.0, far=4.0):
    """n triangles around random centres in and slightly beyond the viewport, corners within +-size pixels, depths in [1, far] per vertex"""
    rs = np.random.RandomState(seed)
    centre = np.stack([rs.uniform(-2, W + 2, n), rs.uniform(-2, H + 2, n)], axis=1)
    corners = centre[:, None, :] + rs.uniform(-size, size, (n, 3, 2))
    depth = rs.uniform(1.0, far, (n, 3, 1))
    return window_mesh(np.concatenate([corners, depth], axis=2), W, H)


def synthetic_views(n_views=3, H=32, W=48, seed=7, focal=60.0):
    """pointmaps of a wavy surface seen by a pinhole at the origin, with a depth step in the middle (rubber-sheet triangles across it),
    shifted per view -> (preds, views) as numpy, B = 1"""
    rs = np.random.RandomState(seed)
    preds, views = [], []
    v, u = np.mgrid[0:H, 0:W]
    for k in range(n_views):
        z = 2.0 + 0.3 * np.sin(u / 5.0 + k) + 0.2 * np.cos(v / 4.0) + np.where(u > W // 2 + k, 0.8, 0.0)
        pts = np.stack([(u - W / 2 + 0.5 + 3 * k) * z / focal, (v - H / 2 + 0.5) * z / focal, z], axis=-1).astype(F32)
        preds.append({"pts3d_in_other_view": pts[None], "conf": rs.uniform(1, 10, (1, H, W)).astype(F32)})
        views.append({"img": rs.uniform(-0.9, 0.9, (1, 3, H, W)).astype(F32)})
    return preds, views


def pose_sets():
    """five seeded sets of camera-to-world poses (only the centres matter to auto_cam_size), odd and even numbers of pairs"""
    out = []
    for seed, n in enumerate([2, 3, 4, 7, 12]):
        rs = np.random.RandomState(100 + seed)
        poses = np.tile(np.eye(4), (n, 1, 1))
        poses[:, :3, 3] = rs.randn(n, 3) * [2.0, 0.5, 3.0]
        out.append(poses)
    return out


def look_from(c2w, back):
    """a camera-to-world pose `back` behind c2w along its optical axis, looking the same way"""
    m = np.array(c2w, dtype=np.float64)
    m[:3, 3] = m[:3, 3] - back * m[:3, 2]
    return m
