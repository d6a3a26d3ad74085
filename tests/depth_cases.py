"""Case recipes of the multi-view depth metrics (include/f3r.h "multi-view depth metrics"), shared by tests/test_depth_metric.py (CPU) and
tests/test_depth_metric_gpu.py, and the guarded launch through the C ABI.  Every recipe is seeded; inputs are built in float64 and rounded
to fp32 once.  A case is a dict: segs = a list of dict(g, p, conf, mask) of flat fp32 arrays (mask: bytes or None) and the parameters of
depth_ref.segment under "kw"."""
import ctypes
import functools

import numpy as np
import torch

import depth_ref as R

SHAPES = ((1, 1), (1, 2), (1, 3), (7, 9), (8, 8), (5, 13), (31, 33), (32, 32), (25, 41), (64, 65))   # 1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4160 pixels
THRESHOLDS4 = (1.03125, 1.25, 1.5, 2.0)        # exact in fp32: a prediction of exactly t against a ground truth of 1 has the ratio t
KW = dict(alignment="median", thresholds=(1.03,), clip=None, pct=0, uncertainty=True, n_bins=100)


def _rng(*key):
    return np.random.default_rng([20261020] + [int(k) for k in key])


def f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64).astype(np.float32))


def plain(n, seed, scale=0.5, noise=0.05, mask_share=0.9, dirty=True):
    """depths in [0.5, 5], a prediction of scale * g * (1 + noise), confidences in (0, 1), a mask that keeps mask_share; dirty: some pixels
    with g in {0, -1, inf, NaN} and p in {NaN, 0, -p}"""
    r = _rng(n, seed)
    g = r.uniform(0.5, 5.0, n)
    p = scale * g * (1.0 + noise * r.standard_normal(n))
    conf = r.uniform(0.01, 1.0, n)
    mask = (r.uniform(0, 1, n) < mask_share).astype(np.uint8) if mask_share < 1 else None
    if dirty and n >= 63:
        at = r.permutation(n)[:14]
        g[at[0:2]], g[at[2:4]], g[at[4:6]], g[at[6:8]] = 0.0, -1.0, np.inf, np.nan
        p[at[8:10]], p[at[10:12]] = np.nan, 0.0
        p[at[12:14]] = -p[at[12:14]]
    return dict(g=f32(g), p=f32(p), conf=f32(conf), mask=mask)


@functools.lru_cache(maxsize=None)
def case(name):
    kw = dict(KW)
    if name == "shapes":                       # every size in one call: n < K, n not a multiple of K, ragged tile ends
        segs = [plain(h * w, i) for i, (h, w) in enumerate(SHAPES)]
    elif name == "valid_counts":               # 0, 1, 2, 3 and all pixels valid
        segs = []
        for i, k in enumerate((0, 1, 2, 3, 64)):
            s = plain(64, 100 + i, mask_share=1, dirty=False)
            s["mask"] = np.zeros(64, np.uint8)
            s["mask"][_rng(7, i).permutation(64)[:k]] = 1
            segs.append(s)
    elif name == "med_p_zero":                 # the median of p is 0: s = 1
        s = plain(65, 3, dirty=False)
        s["p"][_rng(8).permutation(65)[:40]] = 0.0
        s["mask"] = None
        segs = [s]
    elif name == "negative_p":                 # s < 0 is kept: the metrics of -p
        s = plain(1025, 4, dirty=False)
        s["p"] = -s["p"]
        segs = [s]
    elif name == "positive_p":                 # its mirror
        segs = [plain(1025, 4, dirty=False)]
    elif name == "clip":                       # pixels below, inside and above [1, 3]
        segs, kw["clip"] = [plain(1023, 5), plain(65, 6)], (1.0, 3.0)
    elif name in ("pct50", "pct100"):          # ten pixels with conf == thr
        n = 1025
        r = _rng(9)
        conf = np.concatenate([r.uniform(0.01, 0.49, 507), np.full(10, 0.5), r.uniform(0.51, 0.89, 498), np.full(10, 0.9)])
        s = plain(n, 10)
        s["conf"] = f32(conf[r.permutation(n)])
        segs, kw["pct"] = [s, plain(64, 11)], 50 if name == "pct50" else 100
    elif name == "conf_equal":                 # every confidence equal: the sparsification order is the pixel order
        s = plain(1024, 12)
        s["conf"] = np.full(1024, 0.25, np.float32)
        segs = [s, plain(3, 13)]
    elif name == "ties_bin_cut":               # 100 equal confidences across the cut of bins 4 | 5 (K = 10, all 1000 + 24 pixels valid)
        s = plain(1024, 14, mask_share=1, dirty=False)
        conf = np.concatenate([np.linspace(0.01, 0.4, 462), np.full(100, 0.5), np.linspace(0.6, 0.99, 462)])
        s["conf"] = f32(conf[_rng(15).permutation(1024)])
        segs, kw["n_bins"] = [s], 10
    elif name == "conf_special":               # NaNs of both signs, -0.0 and +0.0, infinities
        s = plain(1025, 16)
        c = s["conf"].view(np.uint32).copy()
        at = _rng(17).permutation(1025)
        c[at[0:3]], c[at[3:6]], c[at[6:9]], c[at[9:12]] = 0x7fc00000, 0xffc00000, 0x80000000, 0x00000000
        c[at[12:14]], c[at[14:16]] = 0x7f800000, 0xff800000
        s["conf"] = c.view(np.float32)
        segs = [s]
    elif name == "k1":
        segs, kw["n_bins"] = [plain(65, 18), plain(2, 19)], 1
    elif name == "four_thresholds":            # one pixel exactly on each threshold: r = p / g = t with g = 1, alignment none
        s = plain(64, 20, scale=1.0, mask_share=1, dirty=False)
        s["g"][:4], s["p"][:4] = 1.0, np.asarray(THRESHOLDS4, np.float32)
        s["g"][4:8], s["p"][4:8] = np.asarray(THRESHOLDS4, np.float32), 1.0        # and g / p = t
        segs = [s]
        kw.update(alignment="none", thresholds=THRESHOLDS4)
    elif name == "huge_error":                 # one huge error among tiny ones: total - prefix loses the tiny ones
        g = np.ones(64)
        p = 1.0 + np.arange(64) * 2.0 ** -20
        p[17] = 1e30
        segs = [dict(g=f32(g), p=f32(p), conf=f32(_rng(21).uniform(0.1, 1, 64)), mask=None)]
        kw.update(alignment="none")
    elif name == "even_two":                   # two pixels, g = (1, 2), p = (2, 4): s = 0.5 and every metric 0
        segs = [dict(g=f32([1, 2]), p=f32([2, 4]), conf=f32([0.5, 0.25]), mask=None)]
    else:
        raise KeyError(name)
    return dict(name=name, segs=segs, kw=kw)


CASES = ("shapes", "valid_counts", "med_p_zero", "negative_p", "positive_p", "clip", "pct50", "pct100", "conf_equal", "ties_bin_cut", "conf_special", "k1",
         "four_thresholds", "huge_error", "even_two")
# the cases a wrong reading of the definitions must miss
DISCRIMINATES = {"lower_median": ("even_two", "valid_counts"), "le_threshold": ("four_thresholds",), "unstable_ties": ("conf_equal", "ties_bin_cut"),
                 "total_minus_prefix": ("huge_error",), "conf_gt_thr": ("pct50", "pct100")}


@functools.lru_cache(maxsize=None)
def reference(name, wrong=None):
    """the restatement of every segment of a case: computed once, shared, and left unchanged"""
    c = case(name)
    return tuple(R.segment(s["g"], s["p"], s["conf"], s["mask"], wrong=wrong, **c["kw"]) for s in c["segs"])


def on_threshold(c):
    """the (segment, pixel) pairs a recipe places exactly on a threshold"""
    return {(0, i) for i in range(8)} if c["name"] == "four_thresholds" else set()


# ================================================================================================ the guarded launch (GPU)
def run(lib, dev, c, *, pointmap=False, misalign=False, what="depth"):
    """The three entry points on a case through the C ABI: operands inside 0xFF bytes, outputs and workspace between sentinel words, the
    guards asserted before any value is read.  pointmap: the prediction as channel 2 of an (n, 3) pointmap whose other channels are NaN.
    misalign: every operand starts 4 bytes past a 16-byte boundary.  -> dict(out (S, 16 + 2 K) float64 numpy, order_conf, order_err, starts,
    inputs_unchanged)."""
    from fast3r_amd import _lib
    from post_cases import Bufs, _p, _stream
    kw, segs = c["kw"], c["segs"]
    S, K = len(segs), kw["n_bins"]
    b = Bufs(dev)
    rows, base, tiles, placed = [], 0, [0], []

    def place(a):
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a))
        if misalign:                                    # one more element in front: the operand proper starts 4 (or 1) bytes later
            pad = torch.full((4 // t.element_size(),), 255 if t.dtype == torch.uint8 else float("nan"), dtype=t.dtype)
            view = b.op(torch.cat([pad, t.reshape(-1)]))[pad.numel():]
            assert t.dtype == torch.uint8 or view.data_ptr() % 16 == 4
        else:
            view = b.op(t)
        placed.append((view, t))
        return view
    for s in segs:
        n = s["g"].size
        g, conf, mask = place(s["g"]), place(s["conf"]), place(s["mask"])
        if pointmap:
            pm = np.full((n, 3), np.nan, np.float32)
            pm[:, 2] = s["p"]
            p, stride, chan = place(pm), 3, 2
        else:
            p, stride, chan = place(s["p"]), 1, 0
        rows.append([g.data_ptr(), p.data_ptr(), stride, chan, _p(conf) or 0, _p(mask) or 0, n, base])
        base += n
        tiles.append(tiles[-1] + (n + _lib.DEPTH_TILE - 1) // _lib.DEPTH_TILE)
    words = [x for r in rows for x in r] + tiles
    host = (ctypes.c_int64 * len(words))(*words)
    table = b.op(torch.tensor(words, dtype=torch.int64))
    T, total = tiles[-1], base
    ld = _lib.DEPTH_OUT_WORDS + 2 * K
    out = b.out(2 * S * ld, torch.int32)
    use_thr = int(kw["pct"] > 0)
    clip = kw["clip"]
    tt = (ctypes.c_double * 4)(*kw["thresholds"])
    align = _lib.F3R_DEPTH_ALIGN_MEDIAN if kw["alignment"] == "median" else _lib.F3R_DEPTH_ALIGN_NONE
    _lib.check(lib.f3r_depth_medians(_p(table), host, S, T, align, use_thr, kw["pct"] / 100.0, _p(out), ld, _stream()), "f3r_depth_medians")
    nb0 = lib.f3r_depth_workspace_bytes(S, T, total, 0, 0)
    ws0 = b.out(nb0 // 4, torch.int32)
    _lib.check(lib.f3r_depth_errors(_p(table), host, S, T, use_thr, int(clip is not None), *(clip or (0.0, 0.0)), tt, len(kw["thresholds"]), _p(ws0), nb0,
                                    _p(out), ld, _stream()), "f3r_depth_errors")
    nb1 = lib.f3r_depth_workspace_bytes(S, T, total, 1, K)
    assert nb0 > 0 and nb1 > nb0 and nb0 % 256 == 0 and nb1 % 256 == 0
    ws1, oc, oe, st = b.out(nb1 // 4, torch.int32), b.out(total, torch.int32), b.out(total, torch.int32), b.out(S + 1, torch.int32)
    _lib.check(lib.f3r_depth_sparsify(_p(table), host, S, T, use_thr, int(clip is not None), *(clip or (0.0, 0.0)), K, _p(ws1), nb1, _p(oc), _p(oe),
                                      _p(st), _p(out), ld, _stream()), "f3r_depth_sparsify")
    b.intact(what)
    unchanged = all(v.cpu().numpy().tobytes() == t.numpy().tobytes() for v, t in placed)
    return dict(out=out.view.cpu().numpy().reshape(-1).view(np.float64).reshape(S, ld), order_conf=oc.view.cpu().numpy().reshape(-1),
                order_err=oe.view.cpu().numpy().reshape(-1), starts=st.view.cpu().numpy().reshape(-1), inputs_unchanged=unchanged)
