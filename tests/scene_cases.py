"""Seeded recipes of the scene-assembly cases, shared by tools/make_golden_scene.py (which runs the reference on them) and the tests
(which rebuild the same inputs).  Only numpy's legacy RandomState and exactly rounded arithmetic are used, so the inputs are the
same bits on every machine; the golden stores a checksum of each and the tests compare it.

Segment lengths are expressed from T, the tile length of the segmented sort (fast3r_amd._lib.SCENE_TILE): 1, 63, 64, 65, T - 1, T,
T + 1 and 2 T + 18 in one scene run through the reference, each view with its own (H, W); 1 and 2 T + 17 in a scene of their own.
(T = 4096 is more than 48 x 64 pixels, so the views around T are as large as they have to be and no larger.)"""
import hashlib

import numpy as np
import torch

from fast3r_amd import _lib

T = _lib.SCENE_TILE
DEFAULT_THRESHOLD = 1.5
FIVE_VALUES = (1.0, 1.5, 2.0, 3.0, 7.5)


def shape_of(n):
    """the most nearly square (H, W) with H * W == n, H <= W"""
    h = int(np.floor(np.sqrt(n)))
    while n % h:
        h -= 1
    return h, n // h


# name -> lengths, batch, sample, seed, per-view kind of the global conf, of the local conf, of the sky mask (None: no masks: all ones)
SCENES = {
    "lengths": dict(lengths=[63, 64, 65, T - 1, T, T + 1, 2 * T + 18], B=1, sample=0, seed=11,
                    conf=["random", "constant", "low", "special", "random", "random", "five"],
                    conf_local=["five", "random", "special", "random", "constant", "low", "random"],
                    mask=["zeros", "random", "random", "random", "ones", "random", "random"]),
    # the reference cannot take a view with H = 1 or W = 1 (its squeeze() drops the axis), and 2 T + 17 is prime: these lengths are
    # pinned on tests/scene_ref.py alone, which the other scenes pin on the reference
    "edge": dict(lengths=[1, 2 * T + 17, 63], B=1, sample=0, seed=14, conf=["random", "five", "random"], conf_local=["random", "special", "low"],
                 mask=["ones", "random", "random"], reference=False),
    "batch2": dict(lengths=[42, 45, 64], B=2, sample=1, seed=12, conf=["random", "low", "five"], conf_local=["five", "random", "random"],
                   mask=None),
    "indoor": dict(lengths=[48, 130], B=1, sample=0, seed=13, conf=["random", "special"], conf_local=["random", "random"],
                   mask=["ones", "ones"]),
}

# (percentile, mask_sky (None: is_outdoor), colouring, show_global, show_local, show_high_conf, show_low_conf, timestep = last - this,
#  high / low threshold).  At most one of the two confidence switches is on: with both on the reference's handlers hide whichever class
#  the handler that ran first had shown, so that state has no single meaning there.
STATES = [
    (10, None, "rgb", False, True, True, False, 0, DEFAULT_THRESHOLD),          # the GUI defaults
    (0, True, "rgb", True, True, True, False, 0, DEFAULT_THRESHOLD),
    (50, False, "confidence", True, False, True, False, 0, DEFAULT_THRESHOLD),
    (100, True, "rainbow", False, True, True, False, 0, DEFAULT_THRESHOLD),
    (100, False, "confidence", True, True, False, True, 0, DEFAULT_THRESHOLD),  # the low-confidence views alone
    (10, True, "confidence", True, True, True, False, 2, DEFAULT_THRESHOLD),    # a timestep below the last
    (50, True, "rgb", True, False, False, True, 1, DEFAULT_THRESHOLD),
    (10, False, "rainbow", True, True, True, False, 0, DEFAULT_THRESHOLD),
    (10, True, "rgb", False, False, True, False, 0, DEFAULT_THRESHOLD),         # both heads off: nothing to save
    (0, False, "rgb", True, True, False, False, 0, DEFAULT_THRESHOLD),          # both confidence classes off: nothing to save
    (10, None, "rgb", True, True, True, False, 0, 3.0),                         # the threshold slider moved
]
STATE_KEYS = ("percentile", "mask_sky", "color", "show_global", "show_local", "show_high_conf", "show_low_conf", "back", "threshold")


def _conf(rs, kind, n):
    if kind == "random":
        c = 1.0 + 8.0 * rs.rand(n) ** 2
    elif kind == "five":
        c = np.asarray(FIVE_VALUES)[rs.randint(0, 5, n)]
    elif kind == "constant":
        c = np.full(n, 2.5)
    elif kind == "low":
        c = 1.0 + 0.4 * rs.rand(n)
    elif kind == "special":
        c = 1.0 + 8.0 * rs.rand(n) ** 2
        c = c.astype(np.float32)
        idx = rs.permutation(n)[:min(n, 24)]
        special = [0.0, -0.0, np.inf, np.nan, np.nan, -0.0, 0.0, np.nan, np.inf, -1.5, np.nan, 0.0]
        for j, i in enumerate(idx[:min(len(special), max(1, n // 4))]):
            c[i] = special[j]
        c[idx[len(special):]] = 2.0   # ties around them
        return c
    else:
        raise KeyError(kind)
    return c.astype(np.float32)


def _mask(rs, kind, h, w):
    if kind == "ones":
        return np.ones((h, w), np.int8)
    if kind == "zeros":
        return np.zeros((h, w), np.int8)
    return (rs.rand(h, w) < 0.7).astype(np.int8)


def build(name):
    """-> dict(preds, views: lists over views of dicts of (B, ...) torch tensors on the CPU; masks: list of (H, W) int8 numpy or None;
    B, sample, shapes)"""
    r = SCENES[name]
    rs = np.random.RandomState(r["seed"])
    B = r["B"]
    preds, views, masks, shapes = [], [], [], []
    for i, n in enumerate(r["lengths"]):
        h, w = shape_of(n)
        shapes.append((h, w))
        img = (rs.rand(B, 3, h, w) * 2.0 - 1.0).astype(np.float32)
        img.reshape(-1)[:: max(1, img.size // 7)] = 1.0    # the ends of the range: 255 and 0 exactly
        img.reshape(-1)[1:: max(1, img.size // 5)] = -1.0
        pred = {"pts3d_in_other_view": (rs.randn(B, h, w, 3) * 2.0).astype(np.float32),
                "pts3d_local": rs.randn(B, h, w, 3).astype(np.float32),
                "pts3d_local_aligned_to_global": (rs.randn(B, h, w, 3) * 2.0 + 0.25).astype(np.float32),
                "conf": np.stack([_conf(rs, r["conf"][i], n).reshape(h, w) for _ in range(B)]),
                "conf_local": np.stack([_conf(rs, r["conf_local"][i], n).reshape(h, w) for _ in range(B)])}
        preds.append({k: torch.from_numpy(v) for k, v in pred.items()})
        views.append({"img": torch.from_numpy(img)})
        if r["mask"] is not None:
            masks.append(_mask(rs, r["mask"][i], h, w))
    return dict(preds=preds, views=views, masks=masks if r["mask"] is not None else None, B=B, sample=r["sample"], shapes=shapes)


def single_sample(scene):
    """the {'preds', 'views'} dict the reference can take: batch row `sample` alone (its squeeze() needs B = 1)"""
    s = scene["sample"]
    return {"preds": [{k: v[s:s + 1] for k, v in p.items()} for p in scene["preds"]],
            "views": [{k: v[s:s + 1] for k, v in vw.items()} for vw in scene["views"]]}


def checksum(scene):
    h = hashlib.sha256()
    for p, v in zip(scene["preds"], scene["views"]):
        for k in sorted(p):
            h.update(p[k].numpy().tobytes())
        h.update(v["img"].numpy().tobytes())
    for m in scene["masks"] or []:
        h.update(m.tobytes())
    return h.hexdigest()


# generate_ply_bytes cases: name -> (n, colour dtype, range kind)
PLY_CASES = {
    "u8": (33, "uint8", "u8"),
    "unit_f32": (37, "float32", "unit"),
    "unit_f64": (5, "float64", "unit"),
    "sym_f32": (64, "float32", "sym"),
    "sym_f64": (65, "float64", "sym"),
    "wide_f32": (129, "float32", "wide"),
    "wide_f64": (31, "float64", "wide"),
}


def ply_case(name):
    """-> (points (n, 3) float32, colors (n, 3)) numpy"""
    n, dtype, kind = PLY_CASES[name]
    rs = np.random.RandomState(1000 + sorted(PLY_CASES).index(name))
    pts = (rs.randn(n, 3) * 3.0).astype(np.float32)
    if kind == "u8":
        col = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    else:
        u = rs.rand(n, 3)
        col = {"unit": u, "sym": u * 2.0 - 1.0, "wide": u * 300.0 - 20.0}[kind].astype(dtype)
        if kind == "unit":
            col[0, 0], col[1, 1] = 0.0, 1.0
        if kind == "sym":
            col[0, 0], col[1, 1] = -1.0, 1.0
    return pts, col
