"""Multi-view depth evaluation on the GPU: the counterpart of the reference's scripts/robustmvd_eval.py, whose wrapper takes a view's
pointmap z as depth and 1 - conf as uncertainty (:136-216) and hands them to an external benchmark library with alignment="median"
(:276-277), per sample, in numpy, after a copy to the host.  Here every (view, sample) of a forward pass is scored in one call on tensors
that stay on the device (f3r_depth.hip, include/f3r.h "multi-view depth metrics"): a masked median of two maps, a streaming error pass, a
segmented stable sort for the sparsification curves, fixed-order fp64 sums.

The benchmark library is installed nowhere this project runs, so its defaults cannot be pinned: the definitions are this project's own,
stated in docs/rows_f.md and pinned by a float64 restatement (tests/depth_ref.py).  Deviations from the reference's wrapper: depth is +z
(the wrapper negates it; the median ratio undoes the sign either way), prediction and ground truth must have the same H x W (the library
resizes), and the ground truth comes from the views (`build_gt_views`), not from the library's datasets.

* `depth_metrics(gt_depths, pred, ...)`: the building block, on lists of device tensors -> per-segment numpy arrays.
* `evaluate_multiview_depth(views, preds, ...)`: the views / preds form -> per sample the per-view metrics, their means and the scene.
"""
import numpy as np
import torch

from . import _lib, post_ops
from ._lib import work_device

_ALIGNMENTS = {"none": _lib.F3R_DEPTH_ALIGN_NONE, "median": _lib.F3R_DEPTH_ALIGN_MEDIAN}


def _arguments(alignment, inlier_thresholds, clip_pred_depth, min_conf_thr_percentile, eval_uncertainty, n_bins):
    if alignment not in _ALIGNMENTS:
        raise ValueError(f"depth_metrics: alignment must be 'median' or 'none', got {alignment!r}")
    thresholds = tuple(float(t) for t in inlier_thresholds)
    if len(thresholds) > _lib.DEPTH_MAX_THRESHOLDS or any(t != t for t in thresholds):
        raise ValueError(f"depth_metrics: at most {_lib.DEPTH_MAX_THRESHOLDS} inlier thresholds, none of them NaN; got {inlier_thresholds!r}")
    clip = None
    if clip_pred_depth is not None:
        clip = tuple(float(v) for v in clip_pred_depth)
        if len(clip) != 2 or not clip[0] <= clip[1]:
            raise ValueError(f"depth_metrics: clip_pred_depth must be (lo, hi) with lo <= hi, got {clip_pred_depth!r}")
    pct = float(min_conf_thr_percentile)
    if not 0.0 <= pct <= 100.0:
        raise ValueError(f"depth_metrics: min_conf_thr_percentile must lie in [0, 100], got {min_conf_thr_percentile!r}")
    K = int(n_bins)
    if eval_uncertainty and not 1 <= K <= 65536:
        raise ValueError(f"depth_metrics: n_bins must lie in [1, 65536], got {n_bins!r}")
    return thresholds, clip, pct, K


def depth_metrics(gt_depths, pred, confs=None, valid_masks=None, *, alignment="median", inlier_thresholds=(1.03,), clip_pred_depth=None,
                  min_conf_thr_percentile=0, eval_uncertainty=False, n_bins=100):
    """Depth metrics of every (view, sample) segment in one call.  Lists over views of device tensors: gt_depths (B, H, W) fp32; pred
    (B, H, W, 3) pointmaps, whose channel 2 is read in place, or (B, H, W) depth maps; confs (B, H, W) fp32 or None; valid_masks (B, H, W)
    bool or uint8 or None.  (H, W) may differ between views; a prediction must have its ground truth's.  Segment s = view * B + sample.
    -> dict of numpy arrays over segments: n_valid (int64), thr, median_gt, median_pred, scale, absrel, rmse, inliers (S, T), inlier_counts
    (S, T) and, with eval_uncertainty, ause, sparsification (S, n_bins), oracle (S, n_bins); plus "thresholds" and "segments" = (views, B).
    A segment without a valid pixel has n_valid 0 and NaN everywhere else.  One device-to-host copy."""
    thresholds, clip, pct, K = _arguments(alignment, inlier_thresholds, clip_pred_depth, min_conf_thr_percentile, eval_uncertainty, n_bins)
    V = len(gt_depths)
    if V < 1 or len(pred) != V or (confs is not None and len(confs) != V) or (valid_masks is not None and len(valid_masks) != V):
        raise ValueError("depth_metrics: every list must have one entry per view, and at least one view")
    use_thr = pct > 0
    if (use_thr or eval_uncertainty) and (confs is None or any(c is None for c in confs)):
        raise ValueError("depth_metrics: min_conf_thr_percentile > 0 and eval_uncertainty need a confidence map for every view")
    B = gt_depths[0].shape[0]
    g_list, p_list, c_list, m_list = [], [], [], []
    for v in range(V):
        g, p = gt_depths[v], pred[v]
        if g.dim() != 3 or g.shape[0] != B:
            raise ValueError(f"depth_metrics: view {v}: the ground-truth depth must be (B = {B}, H, W), got {tuple(g.shape)}")
        if tuple(p.shape) not in (tuple(g.shape), tuple(g.shape) + (3,)):
            raise ValueError(f"depth_metrics: view {v}: the prediction {tuple(p.shape)} must have the ground truth's size {tuple(g.shape)} "
                             "(a pointmap with a last dimension of 3, or a depth map); resize one of them first")
        c = None if confs is None else confs[v]
        m = None if valid_masks is None else valid_masks[v]
        for name, t in (("confidence", c), ("valid mask", m)):
            if t is not None and tuple(t.shape) != tuple(g.shape):
                raise ValueError(f"depth_metrics: view {v}: the {name} {tuple(t.shape)} must have the ground truth's size {tuple(g.shape)}")
        g, p = g.contiguous(), p.contiguous()
        c = None if c is None else c.contiguous()
        m = None if m is None else (m.contiguous().view(torch.uint8) if m.dtype == torch.bool else m.contiguous())
        for b in range(B):
            g_list.append(g[b])
            p_list.append(p[b])
            c_list.append(None if c is None else c[b])
            m_list.append(None if m is None else m[b])
    plan = post_ops.depth_plan(g_list, p_list, c_list, m_list, n_bins=K if eval_uncertainty else 0)
    post_ops.depth_medians(plan, _ALIGNMENTS[alignment], pct / 100.0 if use_thr else None)
    post_ops.depth_errors(plan, thresholds, clip, use_thr)
    if eval_uncertainty:
        post_ops.depth_sparsify(plan, clip, use_thr)
    rows = plan["out"].cpu().numpy()  # the one copy; it also orders the launches before the inputs can be freed
    W, T = _lib.DEPTH_OUT_WORDS, len(thresholds)
    res = {"n_valid": rows[:, 0].astype(np.int64), "thr": rows[:, 1].copy(), "median_gt": rows[:, 2].copy(), "median_pred": rows[:, 3].copy(),
           "scale": rows[:, 4].copy(), "absrel": rows[:, 5].copy(), "rmse": rows[:, 6].copy(), "inliers": rows[:, 7:7 + T].copy(),
           "inlier_counts": rows[:, 11:11 + T].copy(), "thresholds": thresholds, "segments": (V, B)}
    if eval_uncertainty:
        res.update(ause=rows[:, 15].copy(), sparsification=rows[:, W:W + K].copy(), oracle=rows[:, W + K:W + 2 * K].copy())
    return res


def _nanmean(values):
    values = [v for v in values if v == v]
    return float(np.mean(values)) if values else float("nan")


def evaluate_multiview_depth(views, preds, *, head="local", keyviews=None, **kw):
    """Depth metrics of a forward pass against `views[v]["depthmap"]` (and `valid_mask`, where a view has one), as `build_gt_views` leaves
    them.  head="local" scores every view (or the views listed in keyviews) from `pts3d_local` / `conf_local`, each in its own camera;
    head="global" scores view 0 only, from `pts3d_in_other_view` / `conf`, as the active lines of the reference's wrapper do.  The
    keywords of `depth_metrics` pass through.  -> a list over samples of {"scene", "views": the scored view numbers, "per_view": {metric:
    array over those views}, and the means over the views with n_valid > 0: "absrel", "rmse", "inliers_<t>" per threshold, "ause" with
    eval_uncertainty}."""
    if head not in ("local", "global"):
        raise ValueError(f"evaluate_multiview_depth: head must be 'local' or 'global', got {head!r}")
    if len(views) != len(preds) or len(views) < 1:
        raise ValueError("evaluate_multiview_depth: need one pred per view, and at least one view")
    key = list(range(len(views))) if keyviews is None else [int(k) for k in keyviews]
    if head == "global":
        key = [0] if keyviews is None else key
        if key != [0]:
            raise ValueError(f"evaluate_multiview_depth: head='global' scores view 0 only, got keyviews {key}: pts3d_in_other_view lives in view "
                             "0's camera, so its z is a depth for that view alone (use head='local' for the others)")
    if not key or any(not 0 <= k < len(views) for k in key):
        raise ValueError(f"evaluate_multiview_depth: keyviews {key} are not views of this pass (0 .. {len(views) - 1})")
    pts_key, conf_key = ("pts3d_local", "conf_local") if head == "local" else ("pts3d_in_other_view", "conf")
    for k in key:
        if "depthmap" not in views[k]:
            raise ValueError(f"evaluate_multiview_depth: views[{k}] has no 'depthmap'; build the ground-truth views with build_gt_views")
        if pts_key not in preds[k]:
            raise KeyError(f"evaluate_multiview_depth: preds[{k}] has no '{pts_key}' (head={head!r})")
    dev = work_device(preds[key[0]][pts_key], "preds")
    to = lambda t: t.to(dev) if t.device != dev else t  # noqa: E731
    gt = [to(views[k]["depthmap"]).to(torch.float32) for k in key]
    pts = [to(preds[k][pts_key]).to(torch.float32) for k in key]
    conf = [to(preds[k][conf_key]).to(torch.float32) for k in key] if all(conf_key in preds[k] for k in key) else None
    masks = None
    if any("valid_mask" in views[k] for k in key):
        masks = [to(views[k]["valid_mask"]) if "valid_mask" in views[k] else torch.ones_like(gt[i], dtype=torch.uint8) for i, k in enumerate(key)]
    res = depth_metrics(gt, pts, conf, masks, **kw)
    V, B = res["segments"]
    names = ["n_valid", "scale", "absrel", "rmse"] + (["ause"] if "ause" in res else [])
    out = []
    for b in range(B):
        seg = [v * B + b for v in range(V)]
        scene = "/".join(views[b]["label"][0].split("/")[:-1]) if b < len(views) and "label" in views[b] else "unknown"  # sample index, as evaluate_reconstruction
        per_view = {n: res[n][seg] for n in names}
        for t, thr in enumerate(res["thresholds"]):
            per_view[f"inliers_{thr:g}"] = res["inliers"][seg, t]
        if "ause" in res:
            per_view["sparsification"], per_view["oracle"] = res["sparsification"][seg], res["oracle"][seg]
        ok = per_view["n_valid"] > 0
        sample = {"scene": scene, "views": list(key), "per_view": per_view}
        for n in per_view:
            if n not in ("n_valid", "scale", "sparsification", "oracle"):
                sample[n] = _nanmean(per_view[n][ok].tolist())
        out.append(sample)
    return out
