"""The cases of the map pictures (fast3r_amd/maps.py), as recipes: seeded numpy inputs, sized to break the kernel, not to load it.  A tile
of the kernels is 1024 pixels and a thread takes four consecutive ones, so 37 x 53 is ragged for any vector width, and 1 x 1025 and
130 x 257 need more than one workgroup per map.  tools/make_golden_maps.py runs matplotlib's imsave on these and stores inputs and decoded
pictures in tests/golden/map_cases.npz; tests/test_maps.py checks that the recipes still give the stored inputs."""
import os

import numpy as np

F32 = np.float32
CMAPS = ("turbo", "Greys")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_cases.npz")


def _rand(seed, shape, lo=0.0, hi=1.0):
    return np.random.RandomState(seed).uniform(lo, hi, shape).astype(F32)


def scalar_cases():
    """name -> the list of (H, W) fp32 maps of one call"""
    c = {}
    c["one_by_one"] = [np.array([[3.5]], F32)]
    c["constant_5x7"] = [np.full((5, 7), 2.25, F32)]
    c["ragged_37x53"] = [_rand(1, (37, 53), 1.0, 20.0)]
    c["row_1x1025"] = [_rand(2, (1, 1025), -3.0, 3.0)]
    c["blocks_130x257"] = [(1 + np.round(np.exp(_rand(3, (130, 257), -2.0, 3.0)) * 64) / 64).astype(F32)]   # on a grid of 1 / 64: the file stays small
    a = _rand(4, (37, 53))
    a[0, 0], a[-1, -1] = 2.0, -1.0
    c["max_first_min_last"] = [a]
    b = _rand(5, (37, 53))
    b[0, 0], b[-1, -1] = -1.0, 2.0
    c["min_first_max_last"] = [b]
    c["steps_0_to_256"] = [np.arange(257, dtype=F32).reshape(1, 257)]          # x * 256 lands on every integer: truncation, 256 -> 255
    c["ulp_steps"] = [(1 + np.arange(3) * 2.0 ** -23).astype(F32).reshape(1, 3)]   # quotients 0, 1/2, 1: the division's rounding
    c["ulp_steps_7"] = [(1 + np.arange(8) * 2.0 ** -23).astype(F32).reshape(2, 4)]  # sevenths: quotients that do round
    # at pixel (3, 2) fp32(t / fp32(vmax - vmin)) * 256 truncates to 217 where matplotlib's fp32(fp64(t) / (fp64(vmax) - fp64(vmin))) gives 218
    c["fp64_divisor"] = [np.random.RandomState(409).uniform(1, 20, (4, 5)).astype(F32)]
    c["huge_1e30"] = [(_rand(6, (9, 11), -1.0, 1.0) * F32(1e30)).astype(F32)]
    d = _rand(7, (5, 7), -1e38, 1e38)
    d[1, 2], d[3, 4] = 3e38, -3e38
    c["overflow_3e38"] = [d]                                                   # vmax - vmin is +inf in fp32 and 6e38 in fp64
    c["subnormal"] = [(np.random.RandomState(8).randint(0, 1000, (6, 9)) * np.float64(2.0 ** -149)).astype(F32)]
    e = _rand(9, (12, 10), -5.0, -0.1)
    e[3, 3] = 0.7
    c["negative_depths"] = [e]
    left, mid, right = _rand(10, (9, 11), 1, 5), _rand(11, (8, 13), 1, 5), _rand(12, (9, 11), 1, 5)
    mid[4, 6] = np.nan
    c["nan_in_the_middle_map"] = [left, mid, right]
    f = _rand(13, (7, 9), 0, 4)
    f[2, 5] = np.inf
    c["one_pos_inf"] = [f]
    g = _rand(14, (7, 9), 0, 4)
    g[6, 0] = -np.inf
    c["one_neg_inf"] = [g]
    c["portrait_and_landscape"] = [_rand(15, (40, 24), 1, 9), _rand(16, (24, 40), 1, 9)]
    return c


def pointmap_case():
    """an (H, W, 3) pointmap whose z channel is read in place (element stride 3, starting at element 2)"""
    p = _rand(17, (20, 33, 3), -2.0, 2.0)
    p[..., 2] = _rand(18, (20, 33), 0.3, 6.0)
    return p


VIEW_SHAPES = [(20, 12), (12, 20), (9, 13)]         # a portrait view, a landscape view and a ragged one
NO_CONF_LOCAL, NO_PTS3D_LOCAL = 1, 2               # the views that lack one of the local keys


def views_case():
    """(preds, views) of three views, B = 2, as numpy: conf, conf_local (B, H, W), pts3d_local (B, H, W, 3), img (B, 3, H, W) with values
    slightly outside [-1, 1]; view 1 has no conf_local and view 2 no pts3d_local"""
    preds, views = [], []
    for v, (H, W) in enumerate(VIEW_SHAPES):
        pred = {"conf": (1 + np.exp(_rand(20 + v, (2, H, W), -1.0, 2.5))).astype(F32)}
        if v != NO_CONF_LOCAL:
            pred["conf_local"] = (1 + np.exp(_rand(30 + v, (2, H, W), -2.0, 1.0))).astype(F32)
        if v != NO_PTS3D_LOCAL:
            pts = _rand(40 + v, (2, H, W, 3), -1.5, 1.5)
            pts[..., 2] = _rand(50 + v, (2, H, W), -0.2, 4.0)
            pred["pts3d_local"] = pts
        preds.append(pred)
        img = _rand(60 + v, (2, 3, H, W), -1.02, 1.02)
        img[:, :, 0, 0], img[:, :, -1, -1] = (-1.0, 1.0, -1.004), (1.004, 0.0, -0.0)
        views.append({"img": img})
    return preds, views


def scalar_pictures(golden):
    """(label, input map, cmap, matplotlib's bytes) of every scalar picture of the loaded golden file"""
    for name, maps in scalar_cases().items():
        for i in range(len(maps)):
            for cmap in CMAPS:
                yield f"{name}/{i}/{cmap}", golden[f"s/{name}/{i}/in"], cmap, golden[f"s/{name}/{i}/{cmap}"]
    for cmap in CMAPS:
        yield f"z/{cmap}", golden["z/in"][..., 2], cmap, golden[f"z/{cmap}"]
