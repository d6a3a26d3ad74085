"""Writes tests/golden/recon_cases.pt: the reference's reconstruction metrics on inputs rebuilt from recipes (CPU only; needs the
reference checkout).  `--check` regenerates the fixture in memory and compares it with the committed file bit for bit.

* metric cases: recipes (kind, sizes, seeds) of two clouds + seeded random unit normals -> the reference's own `accuracy`,
  `completion` (with normals) and `completion_ratio` (fast3r/eval/recon_metric.py:14-49);
* normals: the restated Open3D normals (tests/recon_ref.py) of one ~20 k-point cloud, with the points where the two smallest
  covariance eigenvalues are separated by more than 1e-3 relative;
* evaluate cases: the output of the reference's own MultiViewDUSt3RLitModule.evaluate_reconstruction
  (fast3r/models/multiview_dust3r_module.py:551-735), imported through oracle.ref_loader, with `open3d` and `roma` resolved to the
  stand-ins of tests/recon_ref.py (the reference's align_local_pts3d_to_global runs on the same roma stand-in, unweighted).
"""
import argparse
import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recon_ref  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "recon_cases.pt")

# name: (gt kind, n_gt, gt seed, rec kind, n_rec, rec seed, dist_th)
METRIC_CASES = {
    "uniform": ("uniform", 20000, 1, "uniform", 15000, 2, 0.01),
    "surface": ("surface", 30000, 3, "surface", 25000, 4, 0.005),
    "outliers": ("outliers", 20000, 5, "outliers", 20000, 6, 0.02),
    "duplicates": ("duplicates", 8000, 7, "duplicates", 6000, 8, 0.05),
    "outside": ("uniform", 10000, 9, "outside", 5000, 10, 0.05),
}
NORMALS_CASE = ("surface", 20000, 11)
# name: (B, view sizes, seed, icp percentile, metric percentile)
EVAL_CASES = {
    "b1_p0": (1, [(24, 32), (24, 32), (16, 20)], 21, 0, 0),
    "b1_p85_50": (1, [(24, 32), (16, 20), (24, 32)], 22, 85, 50),
    "b2_p0": (2, [(20, 24), (24, 16), (20, 24)], 23, 0, 0),
    "b2_p85_50": (2, [(20, 24), (24, 16), (20, 24)], 24, 85, 50),
}


def load_reference():
    sys.modules["roma"] = recon_ref.roma
    sys.modules["open3d"] = recon_ref.open3d
    ref_loader._STUB_ROOTS = tuple(ref_loader._STUB_ROOTS) + ("torchmetrics", "pl_bolts", "rerun", "matplotlib", "trimesh", "viser", "wandb",
                                                              "imageio")
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.eval.recon_metric as rm
        import fast3r.models.multiview_dust3r_module as mm
    assert mm.roma is recon_ref.roma and mm.o3d is recon_ref.open3d
    return rm, mm.MultiViewDUSt3RLitModule


def metric_inputs(case):
    gk, ng, gs, rk, nr, rs, th = case
    gt, rec = recon_ref.make_cloud(gk, ng, gs), recon_ref.make_cloud(rk, nr, rs)
    return gt, rec, recon_ref.unit_normals(ng, gs + 1000), recon_ref.unit_normals(nr, rs + 1000), th


def run_reference_eval(cls, case):
    B, sizes, seed, p_icp, p_metric = case
    views, preds = recon_ref.make_eval_case(B, sizes, seed)
    obj = types.SimpleNamespace(reconstruction_metrics_per_epoch={})
    obj.align_local_pts3d_to_global = types.MethodType(cls.align_local_pts3d_to_global, obj)
    with contextlib.redirect_stdout(io.StringIO()):
        cls.evaluate_reconstruction(obj, views, preds, "golden", min_conf_thr_percentile_for_local_alignment_and_icp=p_icp,
                                    min_conf_thr_percentile_for_metric_cacluation=p_metric, use_pts3d_from_local_head=True)
    return {scene: {k: float(v) for k, v in d.items()} for scene, d in obj.reconstruction_metrics_per_epoch["golden"].items()}


def generate():
    warnings.filterwarnings("ignore")
    torch.set_num_threads(8)
    rm, cls = load_reference()
    metric = {}
    for name, case in METRIC_CASES.items():
        gt, rec, ngt, nrec, th = metric_inputs(case)
        acc = rm.accuracy(gt, rec, ngt, nrec)
        comp = rm.completion(gt, rec, ngt, nrec)
        ratio = rm.completion_ratio(gt, rec, th)
        metric[name] = {"recipe": case, "accuracy": torch.tensor([float(v) for v in acc], dtype=torch.float64),
                        "completion": torch.tensor([float(v) for v in comp], dtype=torch.float64),
                        "completion_ratio": torch.tensor(float(ratio), dtype=torch.float32)}
    kind, n, seed = NORMALS_CASE
    pts = recon_ref.make_cloud(kind, n, seed)
    nrm, ev = recon_ref.normals_and_eigenvalues(pts, 30)
    separated = (ev[:, 1] - ev[:, 0]) > 1e-3 * np.abs(ev[:, 1])
    normals = {"recipe": NORMALS_CASE, "normals": torch.from_numpy(nrm.astype(np.float32)), "separated": torch.from_numpy(separated)}
    evals = {name: {"recipe": case, "metrics": run_reference_eval(cls, case)} for name, case in EVAL_CASES.items()}
    return {"metric": metric, "normals": normals, "eval": evals}


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and bool((a.view(-1).view(torch.uint8) == b.view(-1).view(torch.uint8)).all())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return isinstance(b, float) and np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed fixture bit for bit")
    args = ap.parse_args()
    data = generate()
    if args.check:
        old = torch.load(OUT, weights_only=False)
        ok = same(data, old)
        print("recon_cases.pt reproduced bit for bit" if ok else "recon_cases.pt DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    torch.save(data, OUT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
