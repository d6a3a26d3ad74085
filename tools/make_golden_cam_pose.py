"""Writes tests/golden/cam_pose_cases.pt: what the reference returns for the camera-pose metrics on inputs rebuilt from the recipes of
tests/cam_pose_cases.py (CPU only; needs the reference checkout).  `--check` regenerates the fixture in memory and compares it with
the committed file bit for bit.

* metric cases: the reference's own `camera_to_rel_deg`, the threshold means of `evaluate_camera_poses` and `calculate_auc`
  (fast3r/eval/cam_pose_metric.py), run in fp32 and in fp64 on the widened fp32 values, for seeded pose sets and the special sets;
* margin conditions, asserted here on the reference alone and stored: for the sets of up to 12 views, d = max |fp32 run - fp64 run|
  over pairs, and every fp64 pair error and pair maximum at least 10 d from every threshold and every histogram edge k * 30 / 31
  (then fp32 reference, fp64 reference and the kernel must count identically); for 64 and 1500 views no fp64 pair error within 1e-9
  degrees of one;
* evaluate cases: the reference's own MultiViewDUSt3RLitModule.evaluate_camera_poses, unmodified, around oracle/cv2_stub.py, driven
  through a SimpleNamespace carrier with no-op `log` and metric attributes; for 'first_view_from_global_head' every pair error of the
  reference result at least 0.05 degrees from every threshold and edge (tests/test_pnp.py allows 2e-5 on pose entries, which moves an
  angle by at most about 2e-3 degrees at these baselines: 0.05 is 20 x that); and what its `correct_preds_orientation` did to the
  mixed landscape / portrait batch (shapes and a checksum per tensor).
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

import cam_pose_cases as C  # noqa: E402
from oracle import cv2_stub, fixture_io, ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "cam_pose_cases.pt")
POSE_FIXTURE = os.path.join(ROOT, "tests", "golden", "pose_cases.pt")
EXACT_MARGIN_FACTOR = 10.0
LARGE_MARGIN_DEG = 1e-9
EVAL_MARGIN_DEG = 0.05


def load_reference():
    """(fast3r.eval.cam_pose_metric, MultiViewDUSt3RLitModule) of the reference, with oracle/cv2_stub.py as cv2"""
    sys.modules["cv2"] = cv2_stub
    ref_loader._STUB_ROOTS = tuple(r for r in ref_loader._STUB_ROOTS if r != "cv2") + (
        "roma", "torchmetrics", "pl_bolts", "open3d", "rerun", "matplotlib", "trimesh", "viser", "wandb", "sklearn", "imageio")
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.dust3r.cloud_opt.init_im_poses as ip
        import fast3r.eval.cam_pose_metric as cpm
        import fast3r.models.multiview_dust3r_module as mm
    assert ip.cv2 is cv2_stub and mm.camera_to_rel_deg is cpm.camera_to_rel_deg
    return cpm, mm.MultiViewDUSt3RLitModule


def reference_metrics(cpm, pred, gt, dtype, keep_pairs):
    """The metric body of evaluate_camera_poses (:765-783) for one sample in `dtype`, plus the integer counts behind it."""
    pred, gt = pred.to(dtype), gt.to(dtype)
    try:
        r, t = cpm.camera_to_rel_deg(pred, gt, "cpu", len(pred))
    except ValueError as e:
        return {"raises": "ValueError", "message": str(e)}
    out = {"RRA": [(r < tau).float().mean().item() for tau in C.RRA_THRESHOLDS],
           "RTA": [(t < tau).float().mean().item() for tau in C.RTA_THRESHOLDS],
           "mAA": cpm.calculate_auc(r, t, max_threshold=C.MAX_THRESHOLD).item()}
    hist = torch.histc(torch.max(torch.stack((r, t), dim=1), dim=1)[0], bins=C.N_BINS, min=0, max=C.MAX_THRESHOLD)
    out["counts"] = torch.cat([torch.tensor([int((r < tau).sum()) for tau in C.RRA_THRESHOLDS] + [int((t < tau).sum()) for tau in C.RTA_THRESHOLDS]),
                               hist.round().to(torch.int64)])
    out["n_default"] = int((t > 1e5).sum())
    if keep_pairs:
        out["rel_r"], out["rel_t"] = r, t
    return out, r, t


def metric_case(cpm, pred, gt, keep_pairs):
    res = {}
    pairs = {}
    for name, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
        got = reference_metrics(cpm, pred, gt, dtype, keep_pairs)
        if isinstance(got, dict):
            res[name] = got
        else:
            res[name], pairs[name + "_r"], pairs[name + "_t"] = got
    if len(pairs) == 4:
        finite = torch.isfinite(pairs["fp64_r"]) & torch.isfinite(pairs["fp32_r"])
        d_r = float((pairs["fp32_r"].double() - pairs["fp64_r"])[finite].abs().max()) if finite.any() else 0.0
        res["d"] = max(d_r, float((pairs["fp32_t"].double() - pairs["fp64_t"]).abs().max()))
        r, t = pairs["fp64_r"], pairs["fp64_t"]
        res["edge_distance"] = C.edge_distance(r, t, torch.max(r, t))
        res["n_within_1e-9"] = int(sum(((x[torch.isfinite(x) & (x < 1e5), None] - C.edges()[None, :]).abs() < LARGE_MARGIN_DEG).any(1).sum()
                                       for x in (r, t, torch.max(r, t))))
    return res


def carrier(cls):
    """what evaluate_camera_poses touches on `self`: device, thresholds, no-op metrics and log, and the two static methods"""
    obj = types.SimpleNamespace(device="cpu", RRA_thresholds=list(C.RRA_THRESHOLDS), RTA_thresholds=list(C.RTA_THRESHOLDS),
                                log=lambda *a, **k: None, val_mAA=lambda *a, **k: None)
    for tau in set(C.RRA_THRESHOLDS + C.RTA_THRESHOLDS):
        setattr(obj, f"val_RRA_{tau}", lambda *a, **k: None)
        setattr(obj, f"val_RTA_{tau}", lambda *a, **k: None)
    obj.correct_preds_orientation = cls.correct_preds_orientation
    obj.estimate_camera_poses = cls.estimate_camera_poses
    return obj


def checksum(t):
    """position-weighted fp64 sum of the tensor read in its own (possibly transposed) index order"""
    x = t.double().reshape(-1)
    return float((x * torch.arange(1, x.numel() + 1, dtype=torch.float64)).sum())


def eval_case(cpm, cls, name, pose_cases):
    out = {"metrics": {}}
    for mode in C.EVAL_MODES:
        views, preds = C.eval_scene(name, pose_cases)
        captured = {}
        obj = carrier(cls)

        def estimate(preds, views=None, niter_PnP=10, focal_length_estimation_method="individual", _c=captured):
            _c["poses"], _c["focals"] = cls.estimate_camera_poses(preds=preds, views=views, niter_PnP=niter_PnP,
                                                                  focal_length_estimation_method=focal_length_estimation_method)
            return _c["poses"], _c["focals"]
        obj.estimate_camera_poses = estimate  # records what the unmodified method returned, for the margin condition below
        with contextlib.redirect_stdout(io.StringIO()):
            res = cls.evaluate_camera_poses(obj, views, preds, niter_PnP=C.EVAL_NITER_PNP, focal_length_estimation_method=mode)
        out["metrics"][mode] = [{k: float(v) for k, v in d.items()} for d in res]
        if mode == "first_view_from_global_head":
            gt = torch.stack([v["camera_pose"] for v in views]).transpose(0, 1)
            pred = torch.tensor(np.stack(captured["poses"]), dtype=gt.dtype)
            dist = float("inf")
            for b in range(gt.shape[0]):
                r, t = cpm.camera_to_rel_deg(pred[b].double(), gt[b].double(), "cpu", gt.shape[1])
                dist = min(dist, C.edge_distance(r, t, torch.max(r, t)))
            assert dist >= EVAL_MARGIN_DEG, f"evaluate case {name}: a pair error lies {dist:.4f} degrees from a threshold or edge; pick another scene"
            out["edge_distance"] = dist
            out["poses"] = pred
    if C.EVAL_CASES[name][0] == "mixed":
        views, preds = C.eval_scene(name, pose_cases)
        cls.correct_preds_orientation(preds, views)
        out["oriented"] = [{k: {"shapes": [tuple(x.shape) for x in p[k]], "checksums": [checksum(x) for x in p[k]]} for k in p} for p in preds]
    return out


def generate():
    warnings.filterwarnings("ignore")
    torch.set_num_threads(8)
    cpm, cls = load_reference()
    metric = {}
    for name, (n_views, seed) in C.POSE_SETS.items():
        pred, gt = C.pose_set(n_views, seed)
        res = metric_case(cpm, pred, gt, keep_pairs=name in C.PER_PAIR_SETS)
        if name in C.EXACT_SETS:
            assert res["edge_distance"] >= EXACT_MARGIN_FACTOR * res["d"], (name, res["edge_distance"], res["d"])
            assert torch.equal(res["fp32"]["counts"], res["fp64"]["counts"]), name
        else:
            assert res["n_within_1e-9"] == 0, (name, res["edge_distance"])
            if name not in C.PER_PAIR_SETS:
                del res["fp32"]  # the large set pins the fp64 counts and mAA only
        res["recipe"] = (n_views, seed)
        metric[name] = res
    special = {name: metric_case(cpm, *C.special_set(name), keep_pairs=True) for name in C.SPECIAL_SETS}
    pose_cases = fixture_io.load(POSE_FIXTURE)["cases"]
    evals = {name: eval_case(cpm, cls, name, pose_cases) for name in C.EVAL_CASES}
    return {"metric": metric, "special": special, "eval": evals}


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and bool(
            (a.contiguous().view(-1).view(torch.uint8) == b.contiguous().view(-1).view(torch.uint8)).all())
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
        print("cam_pose_cases.pt reproduced bit for bit" if ok else "cam_pose_cases.pt DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    torch.save(data, OUT)
    size = os.path.getsize(OUT)
    assert size < 500 * 1000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
