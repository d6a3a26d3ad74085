"""A float64 restatement of the validation criterion, ConfLossMultiviewV2 around Regr3DMultiviewV3 / V4 with L21Loss, in plain formulas
(test infrastructure; no reference code).  It works view by view on whatever device the inputs are on, so the same function checks the
golden cases on the CPU and the size case on the GPU.

Per view v and sample b, with x the ground-truth points, P the camera-to-world poses rounded to fp32, all widened to float64:
    g_glob = inv(P[0, b]) x,  g_loc = inv(P[v, b]) x          (rotation part times x, plus the translation part)
    valid  = valid_mask [& |g| <= dist_clip], per set
    f      = identity (avg_dis) or log1p (avg_log1p)
    V4:  n(b)   = sum over the views' valid pixels of sample b of f(|.|), NaN values left out, / their number     (global)
         n(b,v) = the same over one view                                                                         (local, or n(b) with
                                                                                                                  local_scale_consistent)
    V3:  n      = mean of f(|.|) over all valid pixels of the batch (NaN if any is NaN)                          (global)
         n(v)   = the same over one view                                                                         (local)
    every n is clipped to >= 1e-8 (NaN stays); gt_scale: the ground truth's n is 1
    L = |pred / n_pred - g / n_gt|
    pts3d_loss(v) = mean of L over the valid pixels of view v (NaN without any)
    conf_loss(v)  = mean of L conf - alpha log conf over them (0 without any)
    loss = sum of all conf_loss / their number
"""
import torch

F64 = torch.float64


def _inverse_poses(pose, device):
    return torch.linalg.inv(pose.float().to(F64).cpu()).to(device)  # 4 x 4: on the host, whatever the device


def _transform(inv, x):
    return (inv[:, None, None, :3, :3] * x[..., None, :]).sum(-1) + inv[:, None, None, :3, 3]


def _clip_min(f):
    return torch.where(f < 1e-8, torch.full_like(f, 1e-8), f)  # NaN stays NaN


def _moments(d, mask, log1p):
    """per sample: number of valid pixels, number of non-NaN f(d) among them, their sum"""
    f = torch.log1p(d) if log1p else d
    good = mask & ~torch.isnan(f)
    B = d.shape[0]
    return (mask.reshape(B, mask[0].numel()).sum(1).to(F64), good.reshape(B, mask[0].numel()).sum(1).to(F64),
            torch.where(good, f, torch.zeros_like(f)).reshape(B, mask[0].numel()).sum(1))  # not -1: a view may have no pixels


def _factor(cnt, nn, s, version):
    """from summed moments (any shape): V4 nanmean, V3 NaN-propagating mean"""
    if version == 4:
        return _clip_min(s / nn)
    return _clip_min(torch.where(nn != cnt, torch.full_like(s, float("nan")), s / cnt))


def multiview_conf_loss(views, preds, version=4, norm_mode="avg_dis", gt_scale=False, local_scale_consistent=False, dist_clip=None, alpha=1.0,
                        inv=None):
    """-> (loss, details): Python floats, details with the reference's keys in the reference's order.  inv: the (B, 4, 4) float64 inverse
    poses per view, for a caller that inverts them another way (default: torch.linalg.inv)."""
    assert version in (3, 4) and norm_mode in ("avg_dis", "avg_log1p")
    log1p = norm_mode == "avg_log1p"
    V = len(views)
    dev = preds[0]["pts3d_in_other_view"].device
    local = "pts3d_local" in preds[0]
    inv = [_inverse_poses(v["camera_pose"], dev) for v in views] if inv is None else [m.to(dev) for m in inv]
    sets = [("global", "pts3d_in_other_view", "conf")] + ([("local", "pts3d_local", "conf_local")] if local else [])

    def geometry(v, kind):
        x = views[v]["pts3d"].to(dev).to(F64)
        g = _transform(inv[0] if kind == "global" else inv[v], x)
        mask = views[v]["valid_mask"].to(dev).bool()
        if dist_clip is not None:
            mask = mask & (g.norm(dim=-1) <= dist_clip)
        return g, mask

    # moments[kind][who]: (cnt, nn, sum), each (V, B)
    mom = {}
    for kind, pkey, _ in sets:
        rows = {"gt": [], "pred": []}
        for v in range(V):
            g, mask = geometry(v, kind)
            rows["gt"].append(torch.stack(_moments(g.norm(dim=-1), mask, log1p)))
            rows["pred"].append(torch.stack(_moments(preds[v][pkey].to(F64).norm(dim=-1), mask, log1p)))
        mom[kind] = {who: torch.stack(r, dim=1) for who, r in rows.items()}  # (3, V, B)

    def factors(kind, who):
        """(V, B)"""
        cnt, nn, s = mom[kind][who]
        if who == "gt" and gt_scale:
            return torch.ones_like(s)
        if kind == "local" and version == 4 and local_scale_consistent:
            return factors("global", who)
        if kind == "global":
            red = (lambda t: t.sum(0, keepdim=True)) if version == 4 else (lambda t: t.sum().reshape(1, 1))
        else:
            red = (lambda t: t) if version == 4 else (lambda t: t.sum(1, keepdim=True))
        return _factor(red(cnt), red(nn), red(s), version).expand_as(s)

    details_pts, details_conf, terms = {}, {}, []
    for kind, pkey, ckey in sets:
        n_gt, n_pr = factors(kind, "gt"), factors(kind, "pred")
        for v in range(V):
            g, mask = geometry(v, kind)
            p = preds[v][pkey].to(F64)
            L = (p / n_pr[v][:, None, None, None] - g / n_gt[v][:, None, None, None]).norm(dim=-1)[mask]
            c = preds[v][ckey].to(F64)[mask]
            details_pts[f"Regr3DMultiviewV3_pts3d_loss_{kind}/{v:02d}"] = float(L.mean()) if L.numel() else float("nan")
            term = float((L * c - alpha * torch.log(c)).mean()) if L.numel() else 0.0
            details_conf[f"ConfLossMultiviewV2_conf_loss_{kind}/{v:02d}"] = term
            terms.append(term)
    return sum(terms) / len(terms), {**details_pts, **details_conf}
