"""Writes tests/golden/loss_cases.pt: what the reference's validation criterion returns for the recipes of tests/loss_cases.py (CPU only;
needs the reference checkout).  `--check` regenerates the fixture in memory and compares it with the committed file bit for bit.

Per case the file holds outputs only:
  * ref32: loss and details of the reference's own classes, ConfLossMultiviewV2(Regr3DMultiviewV3 | V4(L21Loss, ...), alpha), in fp32 as
    the reference runs them;
  * ref64: the same outputs from the float64 restatement tests/loss_ref.py (plain formulas, no reference code);
  * d: |ref32 - ref64| per output (0 where both are NaN), the reference's own fp32 error, which the GPU test allows twice on top of its bound;
  * checksums of the rebuilt inputs.
Asserted here: both have the same keys in the same order and NaN in the same places; the empty view's confidence term is exactly 0 in
both; d stays below 1e-5 relative; the dist_clip case has different global and local masks and no pixel within 1e-4 of the clip distance;
V3 differs from V4 on the same inputs.
"""
import argparse
import contextlib
import io
import math
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loss_cases as C  # noqa: E402
import loss_ref  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loss_cases.pt")
MAX_REL_D = 1e-5
CLIP_MARGIN = 1e-4


def load_reference():
    """the reference's fast3r.dust3r.losses; it imports `dust3r.*`, which lives in the reference's fast3r/ directory"""
    extra = ("roma", "torchmetrics", "pl_bolts", "open3d", "rerun", "matplotlib", "trimesh", "viser", "wandb", "sklearn", "imageio", "scipy", "tqdm",
             "PIL", "huggingface_hub", "einops")
    ref_loader._STUB_ROOTS = tuple(ref_loader._STUB_ROOTS) + tuple(r for r in extra if not _importable(r))  # stand-ins only for what is not installed
    ref_loader.install()
    inner = os.path.join(ref_loader.REFERENCE_ROOT, "fast3r")
    if inner not in sys.path:
        sys.path.insert(0, inner)
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.dust3r.losses as L
    return L


def _importable(name):
    """really installed (the path finder alone: an earlier ref_loader.install() answers for its stubs through sys.meta_path)"""
    import importlib.machinery
    return importlib.machinery.PathFinder.find_spec(name) is not None


def reference_run(L, recipe, views, preds):
    cls = L.Regr3DMultiviewV4 if recipe["version"] == 4 else L.Regr3DMultiviewV3
    crit = L.ConfLossMultiviewV2(cls(L.L21, **C.criterion_kwargs(recipe)), alpha=C.ALPHA)
    with torch.no_grad():
        loss, details = crit(views, preds, **C.call_kwargs(recipe))
    return {"loss": float(loss), "details": {k: float(v) for k, v in details.items()}}


def restatement_run(recipe, views, preds):
    loss, details = loss_ref.multiview_conf_loss(views, preds, version=recipe["version"], alpha=C.ALPHA, **C.criterion_kwargs(recipe),
                                                 **C.call_kwargs(recipe))
    return {"loss": float(loss), "details": details}


def flat(res):
    return {"loss": res["loss"], **res["details"]}


def clip_margin(recipe, views):
    """(smallest relative distance of a valid pixel's |g| from dist_clip over both sets, number of pixels where the two masks differ)"""
    clip, margin, differ = recipe["dist_clip"], math.inf, 0
    inv = [torch.linalg.inv(v["camera_pose"].float().double()) for v in views]
    for v, view in enumerate(views):
        x = view["pts3d"].double()
        norms = [loss_ref._transform(m, x).norm(dim=-1) for m in (inv[0], inv[v])]
        for n in norms:
            margin = min(margin, float(((n - clip).abs() / clip)[view["valid_mask"]].min()))
        differ += int((((norms[0] <= clip) != (norms[1] <= clip)) & view["valid_mask"]).sum())
    return margin, differ


def generate():
    warnings.filterwarnings("ignore")
    torch.set_num_threads(8)
    L = load_reference()
    data = {}
    for name, recipe in C.CASES.items():
        views, preds = C.build(name)
        before = C.checksums(views, preds)
        ref32 = reference_run(L, recipe, views, preds)
        assert C.checksums(views, preds) == before, f"{name}: the reference changed its inputs"
        ref64 = restatement_run(recipe, views, preds)
        a, b = flat(ref32), flat(ref64)
        assert list(a) == list(b), (name, list(a), list(b))
        d = {}
        for k in a:
            assert math.isnan(a[k]) == math.isnan(b[k]), (name, k, a[k], b[k])
            d[k] = 0.0 if math.isnan(a[k]) else abs(a[k] - b[k])
            assert d[k] == 0.0 or d[k] <= MAX_REL_D * max(abs(b[k]), 1e-2), (name, k, a[k], b[k])
        case = {"ref32": ref32, "ref64": ref64, "d": d, "checksums": before, "recipe": dict(recipe)}
        if "dist_clip" in recipe:
            margin, differ = clip_margin(recipe, views)
            assert margin >= CLIP_MARGIN and differ > 0, (name, margin, differ)
            case["clip_margin"], case["masks_differ_at"] = margin, differ
        if "empty_view" in recipe:
            v = recipe["empty_view"]
            for res in (ref32, ref64):
                assert res["details"][f"ConfLossMultiviewV2_conf_loss_global/{v:02d}"] == 0.0
                assert math.isnan(res["details"][f"Regr3DMultiviewV3_pts3d_loss_global/{v:02d}"])
        data[name] = case
    assert abs(data["v3_b2"]["ref64"]["loss"] - data["v4_b2_same_inputs"]["ref64"]["loss"]) > 1e-4, "V3 and V4 agree at B = 2: pick another seed"
    assert math.isnan(data["nan_pred_v4"]["ref64"]["loss"]) and math.isnan(data["nan_pred_v3"]["ref64"]["loss"])
    finite_v4 = [k for k, v in data["nan_pred_v4"]["ref64"]["details"].items() if not math.isnan(v)]
    finite_v3 = [k for k, v in data["nan_pred_v3"]["ref64"]["details"].items() if not math.isnan(v)]
    assert len(finite_v4) > len(finite_v3), "the NaN prediction must spread further under V3 (one factor for the batch) than under V4"
    return data


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a.keys()) == list(b.keys()) and all(same(a[k], b[k]) for k in a)
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
        print("loss_cases.pt reproduced bit for bit" if ok else "loss_cases.pt DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    torch.save(data, OUT)
    for name, case in data.items():
        rel = max(case["d"][k] / max(abs(v), 1e-2) for k, v in flat(case["ref64"]).items() if not math.isnan(v)) if any(
            not math.isnan(v) for v in flat(case["ref64"]).values()) else 0.0
        print(f"{name:24s} loss {case['ref64']['loss']:.9g}  worst relative d {rel:.2e}")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
