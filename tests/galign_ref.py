"""The global-alignment kernel's contract (include/f3r.h "global alignment", docs/rows_f.md) restated in plain torch on the CPU, as separate
operations, in the dtype asked for (fp64: the witness; fp32: what the same formulas give in the reference's precision).  Test infrastructure
only: the product never imports it.

* `loss_and_grads(problem, dist, dtype)`: the closed forms, pixel by pixel as tensors -- no autograd.
* `loss_only(...)`: the loss as a differentiable function of the matrices, for finite differences.
* `RefLoss`: an autograd function around `loss_and_grads`, to put under the torch chain from the raw parameters."""
import numpy as np
import torch


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def tensors(problem, dtype=torch.float64):
    """the numpy problem of galign_cases.matrix_problem as torch tensors of `dtype`"""
    p = problem
    return {"shapes": p["shapes"], "edges": p["edges"], "poses": _t(p["poses"], dtype), "focals": _t(p["focals"], dtype), "pp": _t(p["pp"], dtype),
            "log_depth": [_t(d, dtype) for d in p["log_depth"]], "pw": _t(p["pw"], dtype), "adapt": _t(p["adapt"], dtype),
            "pts": [_t(x, dtype) for x in p["pts"]], "w": [_t(x, dtype) for x in p["w"]]}


def _areas(shapes, edges):
    return (sum(shapes[i][0] * shapes[i][1] for i, j in edges), sum(shapes[j][0] * shapes[j][1] for i, j in edges))


def _view_points(T, v):
    """q (H, W, 3) and X = R q + t of view v"""
    H, W = T["shapes"][v]
    dt = T["poses"].dtype
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    d = T["log_depth"][v].exp()
    f, c = T["focals"][v], T["pp"][v]
    q = torch.stack((d * (xs - c[0]) / f, d * (ys - c[1]) / f, d), dim=-1)
    R, t = T["poses"][v][:, :3], T["poses"][v][:, 3]
    X = torch.stack([(R[r, 0] * q[..., 0] + R[r, 1] * q[..., 1]) + R[r, 2] * q[..., 2] + t[r] for r in range(3)], dim=-1)
    return q, X


def loss_and_grads(T, dist="l1"):
    """T: tensors(problem, dtype).  -> dict(loss, d_log_depth (list per view), d_poses (N, 3, 4), d_focals (N,), d_pp (N, 2), d_pw (E, 3, 4),
    d_adapt (E, 3)) in T's dtype."""
    shapes, edges = T["shapes"], T["edges"]
    N, E, dt = len(shapes), len(edges), T["poses"].dtype
    k = [1.0 / a for a in _areas(shapes, edges)]
    loss = torch.zeros((), dtype=dt)
    G = [torch.zeros(H, W, 3, dtype=dt) for H, W in shapes]
    QX = [_view_points(T, v) for v in range(N)]
    d_pw, d_adapt = torch.zeros(E, 3, 4, dtype=dt), torch.zeros(E, 3, dtype=dt)
    for e, (i, j) in enumerate(edges):
        S, m, a = T["pw"][e][:, :3], T["pw"][e][:, 3], T["adapt"][e]
        for side, v in enumerate((i, j)):
            P, w = T["pts"][2 * e + side], T["w"][2 * e + side]
            b = a * P
            A = torch.stack([(S[r, 0] * b[..., 0] + S[r, 1] * b[..., 1]) + S[r, 2] * b[..., 2] + m[r] for r in range(3)], dim=-1)
            r = QX[v][1] - A
            rr = (r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1]) + r[..., 2] * r[..., 2]
            if dist == "l2":
                cost = w * rr
                s = 2.0 * (k[side] * w)
            else:
                n = rr.sqrt()
                cost = w * n
                s = torch.where(n == 0, torch.zeros_like(n), (k[side] * w) / n)
            g = s[..., None] * r
            live = (w != 0)  # a weight of exactly 0 contributes exactly nothing
            g = torch.where(live[..., None], g, torch.zeros_like(g))
            cost = torch.where(live, cost, torch.zeros_like(cost))
            loss = loss + k[side] * cost.sum()
            G[v] = G[v] + g
            d_pw[e, :, :3] -= torch.einsum("hwi,hwj->ij", g, b)
            d_pw[e, :, 3] -= g.sum(dim=(0, 1))
            d_adapt[e] -= (torch.einsum("ri,hwr->hwi", S, g) * P).sum(dim=(0, 1))
    d_l, d_poses, d_f, d_c = [], torch.zeros(N, 3, 4, dtype=dt), torch.zeros(N, dtype=dt), torch.zeros(N, 2, dtype=dt)
    for v in range(N):
        q, _ = QX[v]
        R, f = T["poses"][v][:, :3], T["focals"][v]
        Rq = torch.einsum("ij,hwj->hwi", R, q)
        d_l.append((G[v] * Rq).sum(dim=-1))
        d_poses[v, :, :3] = torch.einsum("hwi,hwj->ij", G[v], q)
        d_poses[v, :, 3] = G[v].sum(dim=(0, 1))
        u = torch.einsum("ji,hwj->hwi", R, G[v])
        d_f[v] = (-(u[..., 0] * q[..., 0] + u[..., 1] * q[..., 1]) / f).sum()
        d_c[v, 0] = (-(q[..., 2] / f) * u[..., 0]).sum()
        d_c[v, 1] = (-(q[..., 2] / f) * u[..., 1]).sum()
    return {"loss": loss, "d_log_depth": d_l, "d_poses": d_poses, "d_focals": d_f, "d_pp": d_c, "d_pw": d_pw, "d_adapt": d_adapt}


def loss_only(T, dist="l1"):
    """the loss alone, from the formulas of the contract, differentiable by autograd and by finite differences"""
    k = [1.0 / a for a in _areas(T["shapes"], T["edges"])]
    loss = 0
    for e, (i, j) in enumerate(T["edges"]):
        S, m, a = T["pw"][e][:, :3], T["pw"][e][:, 3], T["adapt"][e]
        for side, v in enumerate((i, j)):
            P, w = T["pts"][2 * e + side], T["w"][2 * e + side]
            r = _view_points(T, v)[1] - ((a * P) @ S.T + m)
            cost = r.square().sum(dim=-1) if dist == "l2" else r.norm(dim=-1)
            loss = loss + k[side] * (w * cost).sum()
    return loss


def flat(out):
    """the outputs under the names of galign_cases.MATRIX_NAMES, the per-view log-depth gradients one after another"""
    return {"d_log_depth": torch.cat([d.reshape(-1) for d in out["d_log_depth"]]), "d_poses": out["d_poses"], "d_focals": out["d_focals"],
            "d_pp": out["d_pp"], "d_pw": out["d_pw"], "d_adapt": out["d_adapt"]}


class RefLoss(torch.autograd.Function):
    """alignment_loss's signature with the restatement inside: im_poses (N, 4, 4), focals (N, 1), pp (N, 2), log_depths (total,), pw_poses
    (E, 4, 4), adaptors (E, 3); meta = (shapes, edges, pts, w, dist)"""

    @staticmethod
    def forward(ctx, im_poses, focals, pp, log_depths, pw_poses, adaptors, meta):
        shapes, edges, pts, w, dist = meta
        off, ld = 0, []
        for H, W in shapes:
            ld.append(log_depths.detach()[off:off + H * W].view(H, W))
            off += H * W
        T = {"shapes": shapes, "edges": edges, "poses": im_poses.detach()[:, :3], "focals": focals.detach().reshape(-1), "pp": pp.detach(),
             "log_depth": ld, "pw": pw_poses.detach()[:, :3], "adapt": adaptors.detach(), "pts": pts, "w": w}
        out = loss_and_grads(T, dist)
        f = flat(out)
        pad = lambda g: torch.cat((g, torch.zeros_like(g[:, :1])), dim=1)  # noqa: E731
        ctx.save_for_backward(pad(f["d_poses"]), f["d_focals"].reshape(focals.shape), f["d_pp"], f["d_log_depth"], pad(f["d_pw"]), f["d_adapt"])
        return out["loss"]

    @staticmethod
    def backward(ctx, go):
        return tuple(g * go for g in ctx.saved_tensors) + (None,)


def rel_err(got, ref):
    """max |got - ref| / max |ref| (0 / 0 = 0); NaNs must sit at the same places"""
    got, ref = torch.as_tensor(got).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    assert torch.equal(got.isnan(), ref.isnan())
    ok = ~ref.isnan()
    if not ok.any():
        return 0.0
    top = float(ref[ok].abs().max())
    diff = float((got[ok] - ref[ok]).abs().max())
    return 0.0 if diff == 0.0 else diff / top if top > 0 else float("inf")


CONF_TRF = {"log": torch.log, "sqrt": torch.sqrt, "m1": lambda x: x - 1, "id": lambda x: x}


def golden_problem(golden, name, case):
    """the kernel-level problem of a golden recipe: the matrices the reference's fp32 run computed (stored), the recipe's log depths and
    pointmaps, and the weights conf_trf(conf) in fp32 as the reference computes them"""
    trf = CONF_TRF[case["conf"]]
    pts, w = [], []
    for e in range(len(case["edges"])):
        for p, c in ((case["pts_i"][e], case["conf_i"][e]), (case["pts_j"][e], case["conf_j"][e])):
            pts.append(p)
            w.append(trf(torch.from_numpy(c)).numpy())
    return {"shapes": case["shapes"], "edges": case["edges"], "poses": golden[f"{name}_in_poses"], "focals": golden[f"{name}_in_focals"],
            "pp": golden[f"{name}_in_pp"], "log_depth": case["im_depthmaps"], "pw": golden[f"{name}_in_pw"], "adapt": golden[f"{name}_in_adapt"],
            "pts": pts, "w": w}
