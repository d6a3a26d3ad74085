"""The float64 restatement of the multi-view depth metrics (fast3r_amd/depth_metric.py, include/f3r.h "multi-view depth metrics"; the
definitions: docs/rows_f.md), in plain numpy on the CPU: np.median on the widened values, math.fsum for every sum, np.argsort(kind="stable")
on the integer keys.  `segment` scores one (view, sample); its keyword `wrong` swaps in one deliberately wrong reading of the definitions,
for the tests that show the cases tell them apart."""
import math

import numpy as np

WRONG = ("lower_median", "le_threshold", "unstable_ties", "total_minus_prefix", "conf_gt_thr")


def fkey(x):
    """the order-preserving 32-bit key of f3r_prims.h: -0.0 below +0.0, NaNs beyond the infinities"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def quantile_rule(conf, q):
    """torch.quantile(conf, q) as block_quantile computes it: the rank q (n - 1) in fp32, the two order statistics by key, at::lerp in fp32"""
    c = np.ascontiguousarray(conf, dtype=np.float32).reshape(-1)
    srt = c[np.argsort(fkey(c), kind="stable")]
    rank = np.float32(np.float32(q) * np.float32(c.size - 1))
    rlo = np.floor(rank)
    vlo, vhi = srt[int(rlo)], srt[int(np.ceil(rank))]
    with np.errstate(all="ignore"):
        w, d = np.float32(rank - rlo), np.float32(vhi - vlo)
        return np.float32(vlo + np.float32(w * d)) if w < np.float32(0.5) else np.float32(vhi - np.float32(d * np.float32(np.float32(1.0) - w)))


def valid_pixels(g, p, conf=None, mask=None, thr=None, wrong=None):
    g, p = np.asarray(g, np.float32).reshape(-1), np.asarray(p, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        v = (g > 0) & np.isfinite(g) & np.isfinite(p)
        if mask is not None:
            v &= np.asarray(mask).reshape(-1) != 0
        if thr is not None:
            c = np.asarray(conf, np.float32).reshape(-1)
            v &= (c > thr) if wrong == "conf_gt_thr" else (c >= thr)
    return v


def _median(x, wrong):
    if x.size and wrong == "lower_median":
        return float(np.sort(x)[(x.size - 1) // 2])
    return float(np.median(x))


def segment(g, p, conf=None, mask=None, *, alignment="median", thresholds=(1.03,), clip=None, pct=0, uncertainty=False, n_bins=100, wrong=None):
    """-> dict(n_valid, thr, median_gt, median_pred, scale, absrel, rmse, inliers, counts, ratios; with uncertainty also order_conf, order_err,
    s, o, ause).  g, p, conf: fp32 arrays of one size (p: the depth); mask: bytes or bools."""
    assert wrong is None or wrong in WRONG
    g32, p32 = np.asarray(g, np.float32).reshape(-1), np.asarray(p, np.float32).reshape(-1)
    thr = quantile_rule(conf, np.float32(pct / 100.0)) if pct > 0 else None
    v = valid_pixels(g32, p32, conf, mask, thr, wrong)
    pix = np.flatnonzero(v)
    n = int(pix.size)
    gv, pv = g32[pix].astype(np.float64), p32[pix].astype(np.float64)
    nan = float("nan")
    T = len(thresholds)
    res = {"n_valid": n, "thr": nan if thr is None else float(thr), "median_gt": nan, "median_pred": nan, "scale": nan, "absrel": nan, "rmse": nan,
           "inliers": [nan] * T, "counts": [0] * T, "ratios": np.zeros(0)}
    K = int(n_bins)
    if uncertainty:
        res.update(order_conf=np.zeros(0, np.int64), order_err=np.zeros(0, np.int64), s=[nan] * K, o=[nan] * K, ause=nan)
    if n == 0:
        return res
    with np.errstate(all="ignore"):
        mg, mp = _median(gv, wrong), _median(pv, wrong)
        s = 1.0
        if alignment == "median":
            s = np.float64(mg) / np.float64(mp)
            s = float(s) if np.isfinite(s) else 1.0
        sp = s * pv
        if clip is not None:
            sp = np.minimum(np.maximum(sp, clip[0]), clip[1])
        d = sp - gv
        e = np.abs(d) / gv
        ratios = np.maximum(gv / sp, sp / gv)
        counts = [int(((ratios <= t) if wrong == "le_threshold" else (ratios < t)).sum()) for t in thresholds]
    res.update(median_gt=mg, median_pred=mp, scale=s, absrel=100.0 * math.fsum(e) / n, rmse=math.sqrt(math.fsum(d * d) / n), counts=counts,
               inliers=[100.0 * c / n for c in counts], ratios=ratios)
    if not uncertainty:
        return res
    kc = fkey(np.asarray(conf, np.float32).reshape(-1)[pix]).astype(np.int64) if conf is not None else np.zeros(n, np.int64)
    ke = (~fkey(e.astype(np.float32))).astype(np.int64)
    if wrong == "unstable_ties":    # ties in reverse pixel order
        oc, oe = np.lexsort((-np.arange(n), kc)), np.lexsort((-np.arange(n), ke))
    else:
        oc, oe = np.argsort(kc, kind="stable"), np.argsort(ke, kind="stable")

    def curve(order):
        es = e[order]
        if wrong == "total_minus_prefix":
            total = float(np.sum(es))
            return [(total - float(np.sum(es[:n * k // K]))) / (n - n * k // K) for k in range(K)]
        return [math.fsum(es[n * k // K:]) / (n - n * k // K) for k in range(K)]
    sc, oc_curve = curve(oc), curve(oe)
    ause = 0.0
    if sc[0] != 0.0:
        dk = [(a - b) / sc[0] for a, b in zip(sc, oc_curve)]
        ause = math.fsum((dk[k] + dk[k + 1]) / (2.0 * K) for k in range(K - 1))
    res.update(order_conf=pix[oc], order_err=pix[oe], s=sc, o=oc_curve, ause=ause)
    return res


def tolerance(n, ref):
    """|got - ref| allowed for absrel, rmse and each s_k, o_k: a float64 sum of n non-negative terms in any order is within (n - 1) 2^-53
    relative, the division, the scaling and the square root add a few units, and the reference sum is exact"""
    return (n + 8) * 2.0 ** -53 * abs(ref)


def ause_tolerance(n, s):
    """a weighted sum, of total weight below 1, of differences of quantities that each carry `tolerance`, over s_0"""
    return 4 * (n + 8) * 2.0 ** -53 * max(s) / s[0] if s[0] else 0.0
