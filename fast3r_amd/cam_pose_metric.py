"""Relative camera-pose metrics on the GPU: `camera_to_rel_deg` and `calculate_auc` (fast3r/eval/cam_pose_metric.py:17-40,73-100) and
the metric body of `MultiViewDUSt3RLitModule.evaluate_camera_poses` (fast3r/models/multiview_dust3r_module.py:761-783): RRA@tau,
RTA@tau and mAA(30) over all view pairs.

The reference gathers (pairs, 4, 4) tensors four times over on the CPU; here one launch of f3r_pose_pair_metrics
(fast3r_amd/csrc/f3r_pose_metric.hip, docs/rows_f.md) tiles the upper triangle of (i, j) and returns integer counts, and the metrics
are finished from those counts alone.

One deviation from the reference: it evaluates every pair in the dtype of the ground-truth poses (normally fp32); the kernel evaluates
in fp64 on the same values, widened exactly.  The two can differ only for pairs whose error lies within fp32 rounding (about 1e-3
degrees) of a threshold or of a histogram edge k * 30 / 31; the reference's own fp32 and fp64 runs differ in the same way.
"""
import numpy as np
import torch

from . import post_ops
from ._lib import work_device

N_BINS_EXTRA = 1  # calculate_auc asks torch.histc for max_threshold + 1 bins over [0, max_threshold] (cam_pose_metric.py:93)


def _pair_inputs(pred, gt, what):
    if not torch.is_tensor(pred) or not torch.is_tensor(gt):
        raise ValueError(f"{what}: poses must be torch tensors")
    if pred.shape != gt.shape or tuple(pred.shape[-2:]) != (4, 4):
        raise ValueError(f"{what}: predicted and ground-truth poses must have one shape (..., 4, 4); got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.dtype != gt.dtype or pred.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{what}: poses must both be float32 or both float64; got {pred.dtype} and {gt.dtype}")
    dev = gt.device if gt.is_cuda else work_device(pred, "poses")
    return pred.to(dev), gt.to(dev)


def camera_to_rel_deg(pred_cameras_c2w, gt_cameras_c2w, device=None, batch_size=None):
    """cam_pose_metric.py:17-40: (rel_rangle_deg, rel_tangle_deg) of every pair i < j of the (N, 4, 4) cam-to-world matrices, one entry
    per pair in torch.combinations order, in the input dtype, on the caller's device (CPU inputs go up to the current ROCm device and
    come back).  `device` and `batch_size` are accepted for the reference's signature; the pair set is all pairs of the N poses.
    Computed in fp64 on the input values (see the module docstring).  Raises the reference's ValueError when a relative rotation has
    its trace outside [-1 - 1e-4, 3 + 1e-4] (so3_utils.py:102-103)."""
    home = pred_cameras_c2w.device if torch.is_tensor(pred_cameras_c2w) else None
    pred, gt = _pair_inputs(pred_cameras_c2w, gt_cameras_c2w, "camera_to_rel_deg")
    if pred.dim() != 3:
        raise ValueError(f"camera_to_rel_deg: poses must be (N, 4, 4); got {tuple(pred.shape)}")
    counts, rel_r, rel_t = post_ops.pose_pair_metrics(pred[None], gt[None], (), (), 1, 1.0, want_pairs=True)
    if int(counts[0, 1]) != 0:
        raise ValueError("A matrix has trace outside valid range [-1-eps,3+eps].")
    return rel_r[0].to(home), rel_t[0].to(home)


def _auc_from_bins(bins, n, dtype):
    """The last three operations of calculate_auc (cam_pose_metric.py:96-100) on the histogram, in `dtype`, on the host (a few dozen
    numbers): bit-identical to the reference whenever the bin counts are."""
    histogram = bins.to(device="cpu", dtype=dtype)
    num_pairs = float(n)
    normalized_histogram = histogram / num_pairs
    return torch.cumsum(normalized_histogram, dim=0).mean()


def calculate_auc(r_error, t_error, max_threshold=30):
    """cam_pose_metric.py:73-100: the mean of the cumulative normalised torch.histc(max(r, t), bins = max_threshold + 1, min = 0,
    max = max_threshold) -- the bin width is max_threshold / (max_threshold + 1), as in the reference.  The histogram is counted by
    f3r_pose_error_stats; a 0-d tensor of the input dtype on the caller's device."""
    if r_error.dim() != 1 or r_error.shape != t_error.shape or r_error.dtype != t_error.dtype:
        raise ValueError(f"calculate_auc: r_error and t_error must be 1-D, of one length and dtype; got {tuple(r_error.shape)} and {tuple(t_error.shape)}")
    home, dev = r_error.device, work_device(r_error, "r_error")
    n_bins = int(max_threshold) + N_BINS_EXTRA
    counts = post_ops.pose_error_stats(r_error.to(dev), t_error.to(dev), (), (), n_bins, float(max_threshold))
    return _auc_from_bins(counts[:n_bins], r_error.shape[0], r_error.dtype).to(home)


def camera_pose_metrics(pred_c2w, gt_c2w, rra_thresholds=(5, 15, 30), rta_thresholds=(5, 15, 30), max_threshold=30):
    """The metric body of evaluate_camera_poses (multiview_dust3r_module.py:761-783) for (B, N, 4, 4) predicted and ground-truth
    cam-to-world poses: one dict per sample with `RRA_at_<tau>`, `RTA_at_<tau>` and `mAA_<max_threshold>` as Python floats.  Computed from
    the kernel's counts alone; nothing per pair is materialised.  `RRA_at_tau` is count / pairs in fp32, which is what the reference's
    `(x < tau).float().mean()` gives -- exactly so below 2**24 pairs (N <= 5793), where fp32 still holds every count; mAA is finished in
    the poses' dtype as in `calculate_auc`.  Pairs are evaluated in fp64 (see the module docstring).  Raises the reference's ValueError
    when a relative rotation has its trace out of range."""
    pred, gt = _pair_inputs(pred_c2w, gt_c2w, "camera_pose_metrics")
    if pred.dim() != 4:
        raise ValueError(f"camera_pose_metrics: poses must be (B, N, 4, 4); got {tuple(pred.shape)}")
    B, N = pred.shape[:2]
    n_r, n_t, n_bins = len(rra_thresholds), len(rta_thresholds), int(max_threshold) + N_BINS_EXTRA
    counts, _, _ = post_ops.pose_pair_metrics(pred, gt, rra_thresholds, rta_thresholds, n_bins, float(max_threshold))
    counts = counts.cpu()
    if int(counts[:, n_r + n_t + n_bins].sum()) != 0:
        raise ValueError("A matrix has trace outside valid range [-1-eps,3+eps].")
    n_pairs = N * (N - 1) // 2
    results = []
    for b in range(B):
        c = counts[b]
        res = {}
        for k, tau in enumerate(rra_thresholds):
            res[f"RRA_at_{tau}"] = float(np.float32(int(c[k])) / np.float32(n_pairs))
        for k, tau in enumerate(rta_thresholds):
            res[f"RTA_at_{tau}"] = float(np.float32(int(c[n_r + k])) / np.float32(n_pairs))
        res[f"mAA_{max_threshold}"] = _auc_from_bins(c[n_r + n_t: n_r + n_t + n_bins], n_pairs, pred.dtype).item()
        results.append(res)
    return results
