"""Writes tests/golden/sky_cases.pt (CPU only; needs the reference checkout and scipy).  `--check` regenerates it in memory and compares it
with the committed file bit for bit.

The golden is what the reference's own `detect_sky_mask` (fast3r/viz/viser_visualizer.py:24-72), unmodified, returns for the seeded
procedural scenes of tests/sky_cases.py, with
* the module's `cv2` replaced by tests/cv2_sky_stub.py (the four OpenCV calls restated with OpenCV's uint8 semantics; OpenCV itself is not
  installed, so that stand-in is pinned on the definition of the HSV conversion by tests/test_sky.py, not on OpenCV's binary);
* real `scipy.ndimage`;
* the module loaded the way tools/make_golden_scene.py loads it (`viser` resolving to tests/viser_stub.py).

Stored per case: the checksum of the input, the reference's result packed to bits, and the stats and the branch of the restatement
(tests/sky_ref.py).  Asserted here and stored as `restatement_matches`: the restatement's result equals the reference's on every case,
and the cases reach every branch: empty, no_top, top with all / none / some of the top components kept, and a component that does not
touch row 0 dropped."""
import argparse
import contextlib
import io
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cv2_sky_stub  # noqa: E402
import sky_cases as C  # noqa: E402
import sky_ref as R  # noqa: E402
import viser_stub  # noqa: E402
from oracle import cv2_stub, ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sky_cases.pt")
BRANCH_KINDS = ("empty", "no_top", "top_all", "top_none", "top_some")


def load_reference():
    sys.modules["cv2"] = cv2_stub   # what the rest of the package touches at import time
    v, t = viser_stub.modules()
    sys.modules["viser"], sys.modules["viser.transforms"] = v, t
    ref_loader._STUB_ROOTS = tuple(r for r in ref_loader._STUB_ROOTS if r != "cv2") + (
        "roma", "torchmetrics", "pl_bolts", "open3d", "rerun", "trimesh", "wandb", "imageio")
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.viz.viser_visualizer as vv
    vv.cv2 = cv2_sky_stub           # the four calls of detect_sky_mask
    from scipy import ndimage
    assert vv.ndimage is ndimage
    return vv


def branch_kind(stats):
    if stats["branch"] != "top":
        return stats["branch"]
    if stats["components_kept"] == stats["components_top"]:
        return "top_all"
    return "top_none" if stats["components_kept"] == 0 else "top_some"


def generate():
    warnings.filterwarnings("ignore")
    vv = load_reference()
    cases, kinds, non_top_dropped = {}, set(), False
    for scene, H, W in C.CASES:
        img = C.build(scene, H, W)
        ref = vv.detect_sky_mask(img)
        assert ref.dtype == np.int8 and ref.shape == (H, W)
        mine, stats = R.detect_sky_mask(img)
        assert np.array_equal(ref, mine), f"tests/sky_ref.py differs from the reference on {C.case_name(scene, H, W)}"
        kinds.add(branch_kind(stats))
        non_top_dropped |= stats["branch"] == "top" and stats["components"] > stats["components_top"]
        cases[C.case_name(scene, H, W)] = {
            "input_sha256": C.checksum(img), "not_sky_bits": torch.from_numpy(np.packbits(ref.astype(bool))),
            "stats": [stats[k] for k in ("sky_pixels", "components", "components_top", "components_kept")], "branch": stats["branch"]}
    assert kinds == set(BRANCH_KINDS) and non_top_dropped, (kinds, non_top_dropped)
    return {"cases": cases, "restatement_matches": True, "branch_kinds": sorted(kinds), "non_top_component_dropped": True}


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a == b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="regenerate in memory and compare with the committed file bit for bit")
    args = ap.parse_args()
    data = generate()
    if args.check:
        ok = same(data, torch.load(OUT, weights_only=False))
        print("sky_cases.pt reproduced bit for bit" if ok else "sky_cases.pt DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    torch.save(data, OUT)
    size = os.path.getsize(OUT)
    assert size < 200 * 1000, size
    print(f"wrote {OUT} ({size} bytes, {len(data['cases'])} cases)")


if __name__ == "__main__":
    main()
