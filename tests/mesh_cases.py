"""Seeded recipes of the mesh-export cases, shared by tools/make_golden_mesh.py (which runs the reference on them) and the tests (which
rebuild the same inputs).  Only numpy's legacy RandomState is used, and every draw is rounded to fp32 (which absorbs a last-bit difference
of a double exp or log between machines), so the inputs are the same bits everywhere; the golden stores a checksum of each and the tests
compare it.

The shapes are the smallest at which each piece of fast3r_amd/csrc/f3r_mesh.hip can go wrong.  T = fast3r_amd._lib.MESH_TILE quads (or
pixels) are one workgroup's, 64 one wave step's: 2 x 2 is one quad; 1 x 5 and 5 x 1 have none; 2 x 9 and 9 x 2 are one quad row and one
quad per row; in 3 x 65 and 5 x 67 the quad index crosses a wave step inside a row and W - 1 does not divide the tile; 26 x 42 has T + 1
quads and 33 x 33 exactly T.  Image values lie in [-1, 1]; confidences are lognormal unless the kind says otherwise."""
import hashlib

import numpy as np
import torch

from fast3r_amd import _lib

T = _lib.MESH_TILE
assert 25 * 41 == T + 1 and 32 * 32 == T

MASK_SHAPE = (6, 7)
MASK_KINDS = ("all", "none", "checker", "interior", "edge", "corner_tl", "corner_tr")
# how many triangles (of one winding) the single invalid pixel removes: its incident triangles
MASK_REMOVES = {"all": 0, "interior": 6, "edge": 3, "corner_tl": 1, "corner_tr": 2}

# name -> shapes, batch, sample, seed, percentile, per-view kind of the confidence, per-view kind of the `valid` mask (None: no masks)
CASES = {
    "quad": dict(shapes=[(2, 2)], seed=21, pct=0, conf=["lognormal"]),
    "no_quads": dict(shapes=[(1, 5), (5, 1)], seed=22, pct=80, conf=["lognormal", "lognormal"]),
    "one_quad_row": dict(shapes=[(2, 9), (9, 2)], seed=23, pct=10, conf=["lognormal", "lognormal"]),
    "wave_crossing": dict(shapes=[(3, 65), (5, 67)], seed=24, pct=10, conf=["lognormal", "lognormal"]),
    "tile_plus_one": dict(shapes=[(26, 42)], seed=25, pct=10, conf=["lognormal"]),
    "tile_exact": dict(shapes=[(33, 33)], seed=26, pct=10, conf=["lognormal"]),
    # the vertex and face bases carry over a middle view without a kept face (all confidences equal) and views of three sizes
    "three_views": dict(shapes=[(7, 9), (4, 6), (6, 11)], seed=27, pct=10, conf=["lognormal", "equal", "lognormal"],
                        mask=["random", "all", "random"]),
    "masks": dict(shapes=[MASK_SHAPE] * len(MASK_KINDS), seed=28, pct=10, conf=["lognormal"] * len(MASK_KINDS), mask=list(MASK_KINDS)),
    # all equal: the threshold equals every value; ties that straddle it; one NaN (that view has no faces, the next is unaffected); +inf
    "confs": dict(shapes=[(5, 6)] * 5, seed=29, pct=80, conf=["equal", "ties", "nan", "inf", "lognormal"]),
    "pct0": dict(shapes=[(6, 7), (5, 9)], seed=30, pct=0, conf=["lognormal", "ties"]),
    "pct10": dict(shapes=[(6, 7), (5, 9)], seed=30, pct=10, conf=["lognormal", "ties"]),
    "pct80": dict(shapes=[(6, 7), (5, 9)], seed=30, pct=80, conf=["lognormal", "ties"]),
    "pct99_5": dict(shapes=[(6, 7), (5, 9)], seed=30, pct=99.5, conf=["lognormal", "ties"]),
    "pct100": dict(shapes=[(6, 7), (5, 9)], seed=30, pct=100, conf=["lognormal", "ties"]),
    "batch2": dict(shapes=[(4, 5), (6, 5)], B=2, sample=1, seed=31, pct=50, conf=["lognormal", "lognormal"]),
}


def _conf(rs, kind, n):
    if kind == "lognormal":
        c = 1.0 + np.exp(rs.randn(n))
    elif kind == "equal":
        c = np.full(n, 2.5)
    elif kind == "ties":
        c = np.asarray([1.0, 1.5, 2.0, 3.0, 7.5])[rs.randint(0, 5, n)]
    elif kind == "nan":
        c = 1.0 + np.exp(rs.randn(n))
        c[rs.randint(0, n)] = np.nan
    elif kind == "inf":
        c = 1.0 + np.exp(rs.randn(n))
        c[rs.permutation(n)[:2]] = np.inf
    else:
        raise KeyError(kind)
    return c.astype(np.float32)


def _mask(rs, kind, h, w):
    m = np.ones((h, w), bool)
    if kind == "none":
        m[:] = False
    elif kind == "checker":
        m = (np.add.outer(np.arange(h), np.arange(w)) % 2) == 0
    elif kind == "interior":
        m[h // 2, w // 2] = False
    elif kind == "edge":
        m[0, w // 2] = False
    elif kind == "corner_tl":
        m[0, 0] = False
    elif kind == "corner_tr":
        m[0, w - 1] = False
    elif kind == "random":
        m = rs.rand(h, w) < 0.85
    elif kind != "all":
        raise KeyError(kind)
    return m


def build(name):
    """-> dict(preds, views: lists over views of dicts of (B, ...) torch tensors on the CPU; masks: list of (H, W) bool numpy or None;
    B, sample, shapes, pct)"""
    r = CASES[name]
    rs = np.random.RandomState(r["seed"])
    B = r.get("B", 1)
    preds, views, masks = [], [], []
    for i, (h, w) in enumerate(r["shapes"]):
        n = h * w
        img = (rs.rand(B, 3, h, w) * 2.0 - 1.0).astype(np.float32)
        img.reshape(-1)[:: max(1, img.size // 7)] = 1.0    # the ends of the range: 255 and 0 exactly
        img.reshape(-1)[1:: max(1, img.size // 5)] = -1.0
        pred = {"pts3d_in_other_view": (rs.randn(B, h, w, 3) * 2.0).astype(np.float32),
                "pts3d_local": rs.randn(B, h, w, 3).astype(np.float32),
                "conf": np.stack([_conf(rs, r["conf"][i], n).reshape(h, w) for _ in range(B)]),
                "conf_local": np.stack([_conf(rs, "lognormal", n).reshape(h, w) for _ in range(B)])}
        preds.append({k: torch.from_numpy(v) for k, v in pred.items()})
        views.append({"img": torch.from_numpy(img)})
        if r.get("mask") is not None:
            masks.append(_mask(rs, r["mask"][i], h, w))
    return dict(preds=preds, views=views, masks=masks if r.get("mask") is not None else None, B=B, sample=r.get("sample", 0),
                shapes=list(r["shapes"]), pct=r["pct"])


def numpy_views(case, head="global"):
    """per view (img (3, H, W), pts (H, W, 3), conf (H, W)) of batch row `sample`, as numpy"""
    s = case["sample"]
    pk, ck = ("pts3d_in_other_view", "conf") if head == "global" else ("pts3d_local", "conf_local")
    return [(v["img"][s].numpy(), p[pk][s].numpy(), p[ck][s].numpy()) for p, v in zip(case["preds"], case["views"])]


def checksum(case):
    h = hashlib.sha256()
    for p, v in zip(case["preds"], case["views"]):
        for k in sorted(p):
            h.update(p[k].numpy().tobytes())
        h.update(v["img"].numpy().tobytes())
    for m in case["masks"] or []:
        h.update(m.tobytes())
    return h.hexdigest()
