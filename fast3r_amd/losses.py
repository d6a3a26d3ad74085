"""The validation criterion of the reference (fast3r/dust3r/losses.py), forward only, on the GPU.

Every released config validates with `ConfLossMultiviewV2(Regr3DMultiviewV4(L21Loss, norm_mode="avg_dis"), alpha=0.2)` (data_scaling and
model_scaling: `Regr3DMultiviewV3`).  The classes here carry the reference's names and constructor signatures, so such a config line
builds the same object; calling it runs one HIP kernel family (f3r_loss.hip, `post_ops.mv_conf_loss`) instead of the reference's chain of
concatenations, NaN fills, boolean gathers and einsums, and returns the reference's `(loss, details)`:

    loss      0-dim fp32 tensor on the device, without grad (there is no backward here)
    details   dict of Python floats, the reference's keys in the reference's insertion order:
              Regr3DMultiviewV3_pts3d_loss_global/00.., Regr3DMultiviewV3_pts3d_loss_local/00.. (with a local head),
              ConfLossMultiviewV2_conf_loss_global/00.., ConfLossMultiviewV2_conf_loss_local/00..
              (Regr3DMultiviewV4 uses the prefix `Regr3DMultiviewV3` too: the reference's quirk, kept.)

The arithmetic is fp64 on the fp32 inputs (the reference: fp32 throughout), so the values differ from the reference's by its own fp32
rounding (docs/rows_f.md).

What raises, and what the reference does in the same place:
  * `median_*` with Regr3DMultiviewV4: ValueError at construction (reference: AttributeError on `nanmedian(...).clip` at the first call);
  * any `*_warp-log1p`: ValueError at construction (reference: a shape error at the first call in every configuration, B = 1 included);
  * an empty `norm_mode`: ValueError at construction (reference: fails on `split("_")`);
  * `median_*` with Regr3DMultiviewV3: NotImplementedError at construction (works in the reference; not built here);
  * calling a Regr3DMultiview* object directly: NotImplementedError (reference: its `Sum` fails on the 3-tuples); it is the argument of
    ConfLossMultiviewV2 only;
  * `loss + loss2`: NotImplementedError (no second loss exists here); `k * loss` works;
  * CPU tensors in `preds`: F3RError, as on the other device paths.  Entries of `views` on the CPU are moved to the device.
"""
from copy import copy, deepcopy

import torch
from torch import nn

from . import _lib, post_ops


class LLoss(nn.Module):
    """L-norm loss between (..., 3) point tensors (reference :44-66)."""

    def __init__(self, reduction="mean"):
        super().__init__()
        self.reduction = reduction

    def forward(self, a, b):
        assert a.shape == b.shape and a.ndim >= 2 and 1 <= a.shape[-1] <= 3, f"Bad shape = {a.shape}"
        dist = self.distance(a, b)
        if self.reduction == "none":
            return dist
        if self.reduction == "sum":
            return dist.sum()
        if self.reduction == "mean":
            return dist.mean() if dist.numel() > 0 else dist.new_zeros(())
        raise ValueError(f"bad {self.reduction=} mode")

    def distance(self, a, b):
        raise NotImplementedError()


class L21Loss(LLoss):
    """Euclidean distance between 3-D points (reference :69-73); inside the multi-view losses the kernels compute it."""

    def distance(self, a, b):
        return torch.norm(a - b, dim=-1)


L21 = L21Loss()


class MultiLoss(nn.Module):
    """The reference's combinable loss (:99-157), without the chain: `k * loss` scales, `loss + loss2` raises NotImplementedError."""

    def __init__(self):
        super().__init__()
        self._alpha = 1
        self._loss2 = None

    def compute_loss(self, *args, **kwargs):
        raise NotImplementedError()

    def get_name(self):
        raise NotImplementedError()

    def __mul__(self, alpha):
        assert isinstance(alpha, (int, float))
        res = copy(self)
        res._alpha = alpha
        return res

    __rmul__ = __mul__

    def __add__(self, loss2):
        raise NotImplementedError("fast3r_amd.losses: sums of losses are not built (the validation criterion is a single ConfLossMultiviewV2)")

    def __repr__(self):
        name = self.get_name()
        return f"{self._alpha:g}*{name}" if self._alpha != 1 else name

    def forward(self, *args, **kwargs):
        loss, details = self.compute_loss(*args, **kwargs)
        return loss * self._alpha, details


def _parse_norm_mode(norm_mode, version):
    """-> post_ops dis_mode; raises what the module docstring lists."""
    name = f"Regr3DMultiviewV{version}"
    if not norm_mode:
        raise ValueError(f"{name}: an empty norm_mode is not supported (the reference fails on it too); use 'avg_dis' or 'avg_log1p'")
    parts = str(norm_mode).split("_")
    if len(parts) != 2:
        raise ValueError(f"{name}: norm_mode {norm_mode!r} is not of the form '<avg|median>_<dis|log1p>'")
    norm, dis = parts
    if dis == "warp-log1p":
        raise ValueError(f"{name}: norm_mode {norm_mode!r}: the warp-log1p distance fails in the reference with a shape error in every "
                         "configuration, so there is nothing to reproduce")
    if dis not in ("dis", "log1p"):
        raise ValueError(f"{name}: Unsupported distance mode: {dis}")
    if norm == "median":
        if version == 4:
            raise ValueError(f"{name}: norm_mode {norm_mode!r}: the reference fails on median norms here (nanmedian(dim) returns a tuple, "
                             "which has no .clip)")
        raise NotImplementedError(f"{name}: norm_mode {norm_mode!r}: median norms are not built; use 'avg_dis' or 'avg_log1p'")
    if norm != "avg":
        raise ValueError(f"{name}: Unsupported normalization mode: {norm}")
    return _lib.F3R_LOSS_LOG1P if dis == "log1p" else _lib.F3R_LOSS_DIS


class _Regr3DMultiviewBase(MultiLoss):
    _version = 0

    def __init__(self, criterion, norm_mode, gt_scale, local_scale_consistent):
        super().__init__()
        assert isinstance(criterion, LLoss), f"{criterion} is not a proper criterion!"
        if not isinstance(criterion, L21Loss):
            raise NotImplementedError(f"{type(self).__name__}: only L21Loss is built, got {type(criterion).__name__}")
        self.criterion = copy(criterion)
        self._dis_mode = _parse_norm_mode(norm_mode, self._version)
        self.norm_mode = norm_mode
        self.gt_scale = gt_scale
        self.local_scale_consistent = local_scale_consistent

    def get_name(self):
        return f"{type(self).__name__}({self.criterion})"

    def with_reduction(self, mode):
        res = deepcopy(self)
        res.criterion.reduction = "none"  # as in the reference, whatever `mode` says (:90-96)
        return res

    def forward(self, *args, **kwargs):
        raise NotImplementedError(f"{type(self).__name__} is the pixel loss of ConfLossMultiviewV2 and is not called on its own "
                                  "(in the reference the direct call fails in Sum())")


class Regr3DMultiviewV3(_Regr3DMultiviewBase):
    """Reference :404-568: one global factor over the whole batch (`.mean()`, NaN-propagating), one local factor per view."""
    _version = 3

    def __init__(self, criterion, norm_mode="avg_dis", gt_scale=False):
        super().__init__(criterion, norm_mode, gt_scale, False)


class Regr3DMultiviewV4(_Regr3DMultiviewBase):
    """Reference :570-742: one global factor per sample over all views (`nanmean`), local factors per (sample, view) or, with
    `local_scale_consistent`, the global ones."""
    _version = 4

    def __init__(self, criterion, norm_mode="avg_dis", gt_scale=False, local_scale_consistent=False):
        super().__init__(criterion, norm_mode, gt_scale, local_scale_consistent)


class ConfLossMultiviewV2(MultiLoss):
    """Reference :789-848: per view the mean of `L conf - alpha log conf` over the valid pixels (0 for a view without any), summed over
    the global and the local terms and divided by their number.  `criterion(views, preds, dist_clip=None)` -> (loss, details)."""

    def __init__(self, pixel_loss, alpha=1):
        super().__init__()
        assert alpha > 0
        if not isinstance(pixel_loss, _Regr3DMultiviewBase):
            raise TypeError(f"ConfLossMultiviewV2: pixel_loss must be Regr3DMultiviewV3 or Regr3DMultiviewV4, got {type(pixel_loss).__name__}")
        self.alpha = alpha
        self.pixel_loss = pixel_loss.with_reduction("none")

    def get_name(self):
        return f"ConfLossMultiviewV2({self.pixel_loss})"

    def compute_loss(self, gts, preds, dist_clip=None):
        if len(gts) != len(preds) or len(preds) < 1:
            raise ValueError(f"ConfLossMultiviewV2: {len(gts)} views and {len(preds)} preds")
        local = "pts3d_local" in preds[0]
        keys = ["pts3d_in_other_view", "conf"] + (["pts3d_local", "conf_local"] if local else [])
        for i, p in enumerate(preds):
            for k in keys:
                _lib.require_gpu(p[k], f"preds[{i}]['{k}']")
        dev = preds[0]["pts3d_in_other_view"].device
        pl = self.pixel_loss
        out = post_ops.mv_conf_loss(
            [g["pts3d"].to(dev) for g in gts], [g["valid_mask"].to(dev) for g in gts], [g["camera_pose"].to(dev) for g in gts],
            [p["pts3d_in_other_view"] for p in preds], [p["conf"] for p in preds],
            [p["pts3d_local"] for p in preds] if local else None, [p["conf_local"] for p in preds] if local else None,
            version=pl._version, dis_mode=pl._dis_mode, gt_scale=pl.gt_scale, local_scale_consistent=pl.local_scale_consistent,
            dist_clip=dist_clip, alpha=self.alpha)
        host = out.cpu().tolist()  # the one device-to-host copy
        V = len(preds)
        details = {}
        for part, (prefix, kind) in enumerate((("Regr3DMultiviewV3_pts3d_loss", "global"), ("Regr3DMultiviewV3_pts3d_loss", "local"),
                                               ("ConfLossMultiviewV2_conf_loss", "global"), ("ConfLossMultiviewV2_conf_loss", "local"))):
            if kind == "local" and not local:
                continue
            for v in range(V):
                details[f"{prefix}_{kind}/{v:02d}"] = host[1 + part * V + v]
        return out[0].float(), details
