"""Seeded recipes of the validation-loss cases (tests/golden/loss_cases.pt holds the reference's outputs for them, written by
tools/make_golden_loss.py).  Inputs come from a torch.Generator on the CPU and are built in float64 with elementwise +, -, *, / and sqrt only
(no matmul, no exp / log / sin / cos: the noise is a sum of uniforms, not torch.randn) and rounded to fp32 once at the end, so that a
host whose vector units round an intermediate differently still rebuilds the same fp32 bits; the fixture stores a checksum per input
tensor to prove it.
"""
import torch

F64 = torch.float64
ALPHA = 0.2  # the released configs

# name -> recipe.  shapes: (H, W) per view; B samples; depth_scale: per-sample factor on the scene's depth (V3 normalises the batch as one,
# V4 every sample on its own: they differ once the samples differ in scale).
CASES = {
    "b1_v2_global":       dict(seed=1, B=1, shapes=[(8, 12)] * 2, local=False, version=4),
    "released_local":     dict(seed=2, B=2, shapes=[(12, 16)] * 3, local=True, version=4, holes=0.3),
    "odd_shape":          dict(seed=3, B=2, shapes=[(7, 9)] * 2, local=True, version=4, holes=0.2),  # samples not 16-byte aligned, tail pixels
    "mixed_heights":      dict(seed=4, B=2, shapes=[(8, 16), (12, 16), (10, 16)], local=True, version=4, holes=0.2),
    "avg_log1p":          dict(seed=5, B=2, shapes=[(12, 16)] * 3, local=True, version=4, norm_mode="avg_log1p", holes=0.2),
    "local_scale_consistent": dict(seed=6, B=2, shapes=[(12, 16)] * 3, local=True, version=4, local_scale_consistent=True, holes=0.2),
    "gt_scale":           dict(seed=7, B=2, shapes=[(12, 16)] * 3, local=True, version=4, gt_scale=True, holes=0.2),
    "dist_clip":          dict(seed=8, B=2, shapes=[(12, 16)] * 3, local=True, version=4, dist_clip=3.1, holes=0.2),
    "empty_view":         dict(seed=9, B=2, shapes=[(12, 16)] * 3, local=True, version=4, holes=0.2, empty_view=1),
    "empty_sample":       dict(seed=10, B=2, shapes=[(12, 16)] * 3, local=True, version=4, holes=0.2, empty_sample=1),
    "v3_b2":              dict(seed=11, B=2, shapes=[(12, 16)] * 3, local=True, version=3, holes=0.2, depth_scale=(1.0, 2.5)),
    "v4_b2_same_inputs":  dict(seed=11, B=2, shapes=[(12, 16)] * 3, local=True, version=4, holes=0.2, depth_scale=(1.0, 2.5)),  # what v3_b2 must differ from
    "v3_log1p_gt_scale":  dict(seed=12, B=2, shapes=[(10, 16)] * 2, local=True, version=3, norm_mode="avg_log1p", gt_scale=True, holes=0.2),
    "pose_fp64":          dict(seed=13, B=2, shapes=[(12, 16)] * 3, local=True, version=4, holes=0.2, pose_fp64=True),
    "nan_pred_v4":        dict(seed=14, B=2, shapes=[(12, 16)] * 3, local=True, version=4, holes=0.2, nan_pred=(1, 0, 5, 7)),
    "nan_pred_v3":        dict(seed=14, B=2, shapes=[(12, 16)] * 3, local=True, version=3, holes=0.2, nan_pred=(1, 0, 5, 7)),
    "large":              dict(seed=15, B=1, shapes=[(224, 288)] * 8, local=True, version=4, holes=0.1),
}


def criterion_kwargs(recipe):
    """the keyword arguments of Regr3DMultiviewV3 / V4 for a recipe"""
    kw = dict(norm_mode=recipe.get("norm_mode", "avg_dis"), gt_scale=recipe.get("gt_scale", False))
    if recipe["version"] == 4:
        kw["local_scale_consistent"] = recipe.get("local_scale_consistent", False)
    return kw


def call_kwargs(recipe):
    return {"dist_clip": recipe["dist_clip"]} if "dist_clip" in recipe else {}


def _noise(g, *shape):
    """zero-mean noise of standard deviation about 1 from uniforms alone"""
    u = torch.rand(*shape, 4, generator=g, dtype=F64)
    return ((u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3]) - 2.0) * 1.7


def _poses(g, B):
    """(B, 4, 4) fp64 camera-to-world: a moderate rotation from a normalised quaternion (polynomial in its entries), a translation"""
    q = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=F64) + 0.35 * _noise(g, B, 4)
    q = q / (((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]).sqrt()[:, None]
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(B, 3, 3)
    P = torch.zeros(B, 4, 4, dtype=F64)
    P[:, :3, :3] = R
    P[:, :3, 3] = 0.8 * _noise(g, B, 3)
    P[:, 3, 3] = 1.0
    return P


def _apply(R, t, x):
    """R x + t per sample with elementwise products only; R (B, 3, 3), t (B, 3), x (B, H, W, 3)"""
    out = []
    for i in range(3):
        acc = R[:, None, None, i, 0] * x[..., 0]
        acc = acc + R[:, None, None, i, 1] * x[..., 1]
        acc = acc + R[:, None, None, i, 2] * x[..., 2]
        out.append(acc + t[:, None, None, i])
    return torch.stack(out, dim=-1)


def build(name):
    """-> (views, preds) on the CPU for the recipe `name`.  Ground truth: camera-frame points at depth 1..4 carried to the world by the
    view's pose; global prediction: the ground truth in view 0's frame, scaled by 1.7, plus noise; local prediction: the camera-frame
    points scaled by 0.6 plus noise; conf = 1 + 4 u^2 >= 1."""
    r = CASES[name]
    g = torch.Generator().manual_seed(1000 + r["seed"])
    B = r["B"]
    poses = [_poses(g, B) for _ in r["shapes"]]
    R0, t0 = poses[0][:, :3, :3], poses[0][:, :3, 3]
    views, preds = [], []
    for v, (H, W) in enumerate(r["shapes"]):
        z = (1.0 + 3.0 * torch.rand(B, H, W, generator=g, dtype=F64)) * torch.tensor(r.get("depth_scale", (1.0,) * B), dtype=F64)[:, None, None]
        xy = (torch.rand(B, H, W, 2, generator=g, dtype=F64) - 0.5) * 1.2 * z[..., None]
        cam = torch.cat([xy, z[..., None]], dim=-1)
        P = poses[v]
        world = _apply(P[:, :3, :3], P[:, :3, 3], cam)
        anchor = _apply(R0.transpose(1, 2), torch.zeros(B, 3, dtype=F64), world - t0[:, None, None, :])
        valid = torch.rand(B, H, W, generator=g, dtype=F64) >= r.get("holes", 0.0)
        def conf():
            u = torch.rand(B, H, W, generator=g, dtype=F64)
            return (1.0 + 4.0 * (u * u)).float()

        pred = {"pts3d_in_other_view": (1.7 * anchor + 0.05 * _noise(g, B, H, W, 3)).float(), "conf": conf()}
        if r["local"]:
            pred["pts3d_local"] = (0.6 * cam + 0.05 * _noise(g, B, H, W, 3)).float()
            pred["conf_local"] = conf()
        if r.get("empty_view") == v:
            valid[:] = False
        if "empty_sample" in r:
            valid[r["empty_sample"]] = False
        if "nan_pred" in r and r["nan_pred"][0] == v:
            _, b, i, j = r["nan_pred"]
            valid[b, i, j] = True
            pred["pts3d_in_other_view"][b, i, j, 1] = float("nan")
            if r["local"]:
                pred["pts3d_local"][b, i, j, 0] = float("nan")
        # pose_fp64: the pose stays fp64, not representable in fp32, so the criterion's .float() must round it
        P = P + 1e-9 * _noise(g, B, 4, 4) if r.get("pose_fp64") else P.float()
        views.append({"pts3d": world.float(), "valid_mask": valid, "camera_pose": P})
        preds.append(pred)
    return views, preds


def checksum(t):
    """position-weighted fp64 sum (NaN counted as 0 and bools as 0 / 1)"""
    x = torch.nan_to_num(t.double().reshape(-1), nan=0.0)
    return float((x * torch.arange(1, x.numel() + 1, dtype=torch.float64)).sum())


def checksums(views, preds):
    out = {}
    for v, (view, pred) in enumerate(zip(views, preds)):
        for k in ("pts3d", "valid_mask", "camera_pose"):
            out[f"{v}/{k}"] = checksum(view[k])
        for k, t in pred.items():
            out[f"{v}/{k}"] = checksum(t)
    return out


def to_device(views, preds, device):
    return ([{k: t.to(device) for k, t in view.items()} for view in views], [{k: t.to(device) for k, t in pred.items()} for pred in preds])
