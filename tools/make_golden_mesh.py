"""Writes tests/golden/mesh_cases.pt (CPU only; needs the reference checkout).  `--check` regenerates it in memory and compares it
with the committed file bit for bit.

The golden is what the reference's own `pts3d_to_trimesh` and `cat_meshes` (fast3r/dust3r/viz.py), imported unmodified through
oracle/ref_loader with `trimesh` resolving to a permissive stand-in (numpy and scipy are real), make of the cases of tests/mesh_cases.py
after the three preparation lines of notebooks/demo_multiview.ipynb::plot_3d_points_with_colors (as_mesh=True):

    conf_thr = np.percentile(conf, min_conf_thr_percentile)
    mask = conf > conf_thr
    img_rgb = ((img_rgb + 1) * 127.5).astype(np.uint8).clip(0, 255)

(a case with `valid` masks passes `mask & valid`; the case "masks" is also run with `valid` alone).  Stored per case: the input
checksum, the thresholds, the per-view face counts, and vertices / faces / face_colors whole where they are small, as length and
SHA-256 otherwise.  Asserted here and stored as `restatement_matches`: tests/mesh_ref.py reproduces all of it bit for bit."""
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

import mesh_cases as C  # noqa: E402
import mesh_ref as R  # noqa: E402
from oracle import ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mesh_cases.pt")
WHOLE = 2048   # arrays of up to this many elements are stored whole


def load_reference():
    ref_loader._STUB_ROOTS = tuple(ref_loader._STUB_ROOTS) + tuple(r for r in ("trimesh", "roma") if r not in ref_loader._STUB_ROOTS)
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.dust3r.viz as viz
    assert viz.np is np
    return viz


def stored(a):
    a = np.ascontiguousarray(a)
    if a.size <= WHOLE:
        return torch.from_numpy(a.copy())
    return {"dtype": str(a.dtype), "shape": tuple(a.shape), "sha256": R.digest(a)[1]}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def run_reference(viz, views, pct, masks):
    """the notebook's loop -> (cat_meshes dict, thresholds, faces per view)"""
    meshes, thr = [], []
    for i, (img, pts3d, conf) in enumerate(views):
        img_rgb = img.transpose(1, 2, 0)
        mask = None
        if pct is not None:
            with np.errstate(invalid="ignore"):
                conf_thr = np.percentile(conf, pct)
                mask = conf > conf_thr
            thr.append(conf_thr)
        if masks is not None:
            mask = masks[i] if mask is None else mask & masks[i]
        img_rgb = ((img_rgb + 1) * 127.5).astype(np.uint8).clip(0, 255)
        meshes.append(viz.pts3d_to_trimesh(img_rgb, pts3d, valid=mask))
    per_view = [len(m["faces"]) for m in meshes]
    return viz.cat_meshes(meshes), np.asarray(thr, np.float32), np.asarray(per_view, np.int64)


def record(viz, views, pct, masks):
    ref, thr, per_view = run_reference(viz, views, pct, masks)
    mine = R.build(views, pct, masks)
    assert ref["vertices"].dtype == np.float32 and ref["faces"].dtype == np.int64 and ref["face_colors"].dtype == np.uint8
    ok = all(same_bits(ref[k], mine[k]) for k in ("vertices", "faces", "face_colors"))
    ok = ok and same_bits(thr, mine["thresholds"]) and same_bits(per_view, mine["faces_per_view"])
    assert ok, "tests/mesh_ref.py does not reproduce the reference"
    return {"vertices": stored(ref["vertices"]), "faces": stored(ref["faces"]), "face_colors": stored(ref["face_colors"]),
            "thresholds": torch.from_numpy(thr.copy()), "faces_per_view": torch.from_numpy(per_view.copy()), "restatement_matches": ok}


def generate():
    warnings.filterwarnings("ignore")
    viz = load_reference()
    cases = {}
    for name in C.CASES:
        case = C.build(name)
        views = C.numpy_views(case)
        out = {"checksum": C.checksum(case), "shapes": [tuple(s) for s in case["shapes"]], "pct": case["pct"],
               "mesh": record(viz, views, case["pct"], case["masks"])}
        if name == "masks":
            out["mask_only"] = record(viz, views, None, case["masks"])
        out["restatement_matches"] = all(out[k]["restatement_matches"] for k in ("mesh", "mask_only") if k in out)
        cases[name] = out
    return {"tile": C.T, "cases": cases}


def same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()
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
        print("mesh_cases.pt reproduced bit for bit" if ok else "mesh_cases.pt DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    torch.save(data, OUT)
    size = os.path.getsize(OUT)
    assert size < 500 * 1000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
