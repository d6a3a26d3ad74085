"""Writes tests/golden/galign_cases.npz (CPU only; needs the reference checkout).  `--check` regenerates it in memory and compares it with
the committed file array for array.

The golden is what the reference's own `PointCloudOptimizer` (fast3r/dust3r/cloud_opt/optimizer.py, base_opt.py) computes on the recipes of
tests/galign_cases.py, behind the stub list of tools/make_golden_clean.py.  The class touches two names of `roma`, which is installed
nowhere this project runs: `RigidUnitQuat(q, t).normalize().to_homogeneous()` and `rotmat_to_unitquat`.  This tool puts its own stand-in
for the two into the reference's module at run time (oracle/roma_stub.py stays as it is).

Per recipe, with `allow_pw_adaptors=True` and `optimize_pp=True` so that every parameter has a gradient, four runs of the reference's
`forward()` and `backward()`:
* raw32 / raw64: the class as it is, in fp32, and after `.double()` on the widened fp32 values -> the loss and the gradient of every raw
  parameter (`im_depthmaps` without the reference's padding to the largest area);
* mat32 / mat64: the same forward with its five getters (`get_im_poses`, `get_focals`, `get_principal_points`, `get_pw_poses`,
  `get_adaptors`) handing out leaves that hold the fp32 run's matrices, in fp32 and widened -> the loss and the gradients at the level of
  matrices, at exactly the inputs the kernel is given.
Stored: those, the matrices themselves, the recipes' names and seeds, the reference's constructor signature, and for the loop case the start
loss, the start gradients, the parameters after the reference's first iteration and the final loss of its own 100-iteration loop.

Margin conditions, asserted here on the reference alone and stored:
* in l1 cases no residual norm (fp64 run, pixels of weight 0 aside) is below 1e-3 of the case's median residual norm;
* every depth is positive and finite;
* every gradient tensor has a nonzero maximum.
A recipe that breaks one fails loudly: pick another seed in tests/galign_cases.py, never a wider cap."""
import argparse
import contextlib
import importlib.util
import inspect
import io
import json
import os
import re
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import galign_cases as C  # noqa: E402
from oracle import cv2_stub, ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "galign_cases.npz")
MIN_RESIDUAL_SHARE = 1e-3
GETTERS = ("get_im_poses", "get_focals", "get_principal_points", "get_pw_poses", "get_adaptors")


# ------------------------------------------------------------------------------------------------------------------- the roma stand-in
def _unitquat_to_rotmat(q):
    x, y, z, w = q.unbind(-1)
    rows = [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]
    return torch.stack(rows, dim=-1).reshape(q.shape[:-1] + (3, 3))


class RigidUnitQuat:
    """what `_get_poses` (base_opt.py:190-195) calls: quaternions in (x, y, z, w) order"""

    def __init__(self, linear, translation):
        self.linear, self.translation = linear, translation

    def normalize(self):
        return RigidUnitQuat(self.linear / torch.norm(self.linear, dim=-1, keepdim=True), self.translation)

    def to_homogeneous(self):
        R = _unitquat_to_rotmat(self.linear)
        top = torch.cat((R, self.translation[..., None]), dim=-1)
        bottom = torch.zeros(top.shape[:-2] + (1, 4), dtype=top.dtype, device=top.device)
        bottom[..., 0, 3] = 1
        return torch.cat((top, bottom), dim=-2)


def _rotmat_to_unitquat(R):
    """one rotation (3, 3) -> (x, y, z, w); the largest of the four pivots decides the form"""
    m = R.double()
    piv = [1 + m[0, 0] - m[1, 1] - m[2, 2], 1 - m[0, 0] + m[1, 1] - m[2, 2], 1 - m[0, 0] - m[1, 1] + m[2, 2], 1 + m[0, 0] + m[1, 1] + m[2, 2]]
    k = int(np.argmax([float(p) for p in piv]))
    q = [torch.stack((piv[0], m[0, 1] + m[1, 0], m[0, 2] + m[2, 0], m[2, 1] - m[1, 2])),
         torch.stack((m[0, 1] + m[1, 0], piv[1], m[1, 2] + m[2, 1], m[0, 2] - m[2, 0])),
         torch.stack((m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], piv[2], m[1, 0] - m[0, 1])),
         torch.stack((m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], piv[3]))][k]
    q = q / q.norm()
    return (q if q[3] >= 0 else -q).to(R.dtype)


def load_reference():
    """(PointCloudOptimizer, the base_opt module, geotrf) of the reference, with the roma stand-in in place"""
    sys.modules["cv2"] = cv2_stub
    extra = ("roma", "torchmetrics", "pl_bolts", "open3d", "rerun", "matplotlib", "trimesh", "viser", "wandb", "sklearn", "imageio")
    if importlib.util.find_spec("tqdm") is None:
        extra += ("tqdm",)
    ref_loader._STUB_ROOTS = tuple(r for r in ref_loader._STUB_ROOTS if r != "cv2") + extra
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        from fast3r.dust3r.cloud_opt import base_opt
        from fast3r.dust3r.cloud_opt.optimizer import PointCloudOptimizer
        from fast3r.dust3r.utils.geometry import geotrf
    roma = types.ModuleType("roma_stand_in")
    roma.RigidUnitQuat, roma.rotmat_to_unitquat = RigidUnitQuat, _rotmat_to_unitquat
    base_opt.roma = roma
    return PointCloudOptimizer, base_opt, geotrf


def default_repr(x):
    """repr without the address a built-in's repr ends with (`rand_pose=torch.randn`)"""
    return re.sub(r" at 0x[0-9a-f]+", "", repr(x))


def signature(cls, base_opt):
    """the constructor's parameters: `_init_from_views` of the base class, then the keyword-only ones the class adds"""
    base = [p for p in inspect.signature(base_opt.BasePCOptimizer._init_from_views).parameters.values() if p.name != "self"]
    own = [p for p in inspect.signature(cls.__init__).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    return [[p.name, None if p.default is inspect.Parameter.empty else default_repr(p.default)] for p in base + own]


# ------------------------------------------------------------------------------------------------------------------- runs
def build(cls, c, **kw):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    view1, view2, pred1, pred2 = C.optimizer_inputs(c, t)
    net = cls(view1, view2, pred1, pred2, dist=c["dist"], conf=c["conf"], base_scale=C.BASE_SCALE, pw_break=C.PW_BREAK,
              focal_break=C.FOCAL_BREAK, verbose=False, **kw)
    with torch.no_grad():
        for name in ("pw_poses", "pw_adaptors", "im_poses", "im_focals", "im_pp"):
            getattr(net, name).data[:] = t(c[name])
        net.im_depthmaps.data.zero_()
        for v, d in enumerate(c["im_depthmaps"]):
            net.im_depthmaps.data[v, :d.size] = t(d).reshape(-1)
    return net


def unpad(net, x):
    """(N, max_area, ...) -> the views one after another"""
    return torch.cat([x[v, :h * w] for v, (h, w) in enumerate(net.imshapes)])


def raw_run(net):
    net.zero_grad()
    loss = net()
    loss.backward()
    g = {n: getattr(net, n).grad.detach().clone() for n in C.RAW_NAMES if getattr(net, n).grad is not None}
    g["im_depthmaps"] = unpad(net, g["im_depthmaps"])
    return loss.detach(), g


def matrices_of(net):
    with torch.no_grad():
        return {n: getattr(net, n)().detach().clone() for n in GETTERS}


def mat_run(net, mats, dtype):
    """forward() with the five getters handing out leaves that hold `mats` in `dtype`"""
    leaves = {n: m.detach().clone().to(dtype).requires_grad_() for n, m in mats.items()}
    for n in GETTERS:
        setattr(net, n, (lambda leaf: (lambda *a, **k: leaf))(leaves[n]))
    try:
        net.zero_grad()
        loss = net()
        loss.backward()
    finally:
        for n in GETTERS:
            delattr(net, n)
    g = {"d_log_depth": unpad(net, net.im_depthmaps.grad.detach()), "d_poses": leaves["get_im_poses"].grad[:, :3],
         "d_focals": leaves["get_focals"].grad.reshape(-1), "d_pp": leaves["get_principal_points"].grad,
         "d_pw": leaves["get_pw_poses"].grad[:, :3], "d_adapt": leaves["get_adaptors"].grad}
    return loss.detach(), {k: v.detach().clone() for k, v in g.items()}


def residual_norms(net, geotrf):
    """the residual norms of the reference's own forward, pixels of weight 0 and the padding aside"""
    with torch.no_grad():
        pw, ad, proj = net.get_pw_poses(), net.get_adaptors().unsqueeze(1), net.get_pts3d(raw=True)
        out = []
        for pred, w, idx in ((net._stacked_pred_i, net._weight_i, net._ei), (net._stacked_pred_j, net._weight_j, net._ej)):
            r = (proj[idx] - geotrf(pw, ad * pred)).norm(dim=-1)
            for e, v in enumerate(idx.tolist()):
                h, wd = net.imshapes[v]
                keep = w[e, :h * wd] != 0
                out.append(r[e, :h * wd][keep])
        return torch.cat(out)


def case(cls, base_opt, geotrf, name):
    c = C.golden_case(name)
    kw = dict(allow_pw_adaptors=True, optimize_pp=True)
    net32 = build(cls, c, **kw)
    net64 = build(cls, c, **kw).double()
    l32, g32 = raw_run(net32)
    l64, g64 = raw_run(net64)
    mats = matrices_of(net32)
    ml32, mg32 = mat_run(net32, mats, torch.float32)
    ml64, mg64 = mat_run(net64, mats, torch.float64)
    # margin conditions
    depths = torch.cat([d.reshape(-1) for d in net64.get_depthmaps()])
    assert bool(torch.isfinite(depths).all()) and bool((depths > 0).all()), f"{name}: a depth is not positive and finite"
    rn = residual_norms(net64, geotrf)
    share = float(rn.min() / rn.median())
    if c["dist"] == "l1":
        assert share >= MIN_RESIDUAL_SHARE, f"{name}: the smallest residual is {share:.2e} of the median (floor {MIN_RESIDUAL_SHARE}): pick another seed"
    for tag, g in (("raw", g64), ("matrix", mg64)):
        for k, v in g.items():
            assert float(v.abs().max()) > 0 and bool(torch.isfinite(v).all()), f"{name}: the {tag} gradient {k} vanishes or is not finite"
    n_zero = int(sum((w == 0).sum() for w in (net32._weight_i, net32._weight_j)))
    print(f"{name}: loss {float(l64):.6f} (fp32 {float(l32):.6f}), smallest residual {share:.2e} of the median {float(rn.median()):.3f}, "
          f"{len(c['edges'])} edges, {n_zero} padded or zero weights")
    data = {f"{name}_seed": np.int64(C.GOLDEN[name][4]), f"{name}_residual_share": np.float64(share), f"{name}_residual_median": np.float64(rn.median()),
            f"{name}_loss32": np.float32(l32), f"{name}_loss64": np.float64(l64), f"{name}_mat_loss32": np.float32(ml32),
            f"{name}_mat_loss64": np.float64(ml64)}
    for k in C.RAW_NAMES:
        data[f"{name}_raw32_{k}"], data[f"{name}_raw64_{k}"] = g32[k].numpy(), g64[k].numpy()
    for k in C.MATRIX_NAMES:
        data[f"{name}_mat32_{k}"], data[f"{name}_mat64_{k}"] = mg32[k].numpy(), mg64[k].numpy()
    data[f"{name}_in_poses"] = mats["get_im_poses"][:, :3].contiguous().numpy()
    data[f"{name}_in_focals"] = mats["get_focals"].reshape(-1).numpy()
    data[f"{name}_in_pp"] = mats["get_principal_points"].numpy()
    data[f"{name}_in_pw"] = mats["get_pw_poses"][:, :3].contiguous().numpy()
    data[f"{name}_in_adapt"] = mats["get_adaptors"].numpy()
    return data


def loop_case(cls, base_opt):
    """the reference's defaults (adaptors and principal points fixed) on exact pairwise pointmaps"""
    c = C.loop_case()
    net = build(cls, c)
    l0, g0 = raw_run(net)
    first = build(cls, c)
    base_opt.global_alignment_loop(first, lr=C.LOOP_LR, niter=1, schedule="cosine", lr_min=1e-6)
    full = build(cls, c)
    lf = base_opt.global_alignment_loop(full, lr=C.LOOP_LR, niter=C.LOOP_NITER, schedule="cosine", lr_min=1e-6)
    trained = ("pw_poses", "im_poses", "im_focals", "im_depthmaps")
    assert sorted(n for n, p in net.named_parameters() if p.requires_grad) == sorted(trained)
    assert float(lf) < 0.5 * float(l0), (float(l0), float(lf))
    print(f"loop: loss {float(l0):.6f} -> {float(lf):.6f} after {C.LOOP_NITER} iterations of the reference's loop")
    data = {"loop_seed": np.int64(C.LOOP[4]), "loop_l0": np.float64(l0), "loop_lf": np.float64(lf)}
    for k in trained:
        p1 = getattr(first, k).detach()
        data[f"loop_grad0_{k}"] = g0[k].numpy()
        data[f"loop_first_{k}"] = (unpad(first, p1) if k == "im_depthmaps" else p1).numpy().copy()
    return data


def schedules(base_opt):
    import fast3r.dust3r.cloud_opt.commons as commons
    ts = np.linspace(0.0, 1.0, 11)
    return {"schedule_t": ts, "schedule_cosine": np.asarray([commons.cosine_schedule(t, 0.01, 1e-6) for t in ts], np.float64),
            "schedule_linear": np.asarray([commons.linear_schedule(t, 0.01, 1e-6) for t in ts], np.float64)}


def generate():
    torch.set_num_threads(1)
    cls, base_opt, geotrf = load_reference()
    data = {"conditions_ok": np.bool_(True), "min_residual_share": np.float64(MIN_RESIDUAL_SHARE),
            "signature": np.asarray(json.dumps(signature(cls, base_opt))), "names": np.asarray(json.dumps(list(C.GOLDEN)))}
    for name in C.GOLDEN:
        data.update(case(cls, base_opt, geotrf, name))
    data.update(loop_case(cls, base_opt))
    data.update(schedules(base_opt))
    return data


def same(a, b):
    return sorted(a) == sorted(b) and all(np.asarray(a[k]).dtype == np.asarray(b[k]).dtype and np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
                                          for k in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed file array for array")
    args = ap.parse_args()
    data = generate()
    if args.check:
        with np.load(OUT) as f:
            ok = same(data, {k: f[k] for k in f.files})
        print("galign_cases.npz reproduced array for array" if ok else "galign_cases.npz DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size < 1000 * 1000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
