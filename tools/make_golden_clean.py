"""Writes tests/golden/clean_cases.npz (CPU only; needs the reference checkout).  `--check` regenerates it in memory and compares it with
the committed file array for array.

The golden is what the reference's own `BasePCOptimizer.clean_pointcloud` (fast3r/dust3r/cloud_opt/base_opt.py:279-317) returns on the
recipes of tests/clean_cases.py, run in fp32 and in fp64 on the widened fp32 values.  The method is called unbound on a small carrier that
supplies what it touches: n_imgs, imshapes, im_conf, get_im_poses, get_intrinsics, get_depthmaps, depth_to_pts3d and a __deepcopy__.  Only
the recipes' names and results are stored: the fp32 result, and of the fp64 run the mask of changed pixels (its values are the inputs and
min(input, max_bad_conf): asserted here).

Margin conditions, asserted here on the reference alone and stored (tests/clean_ref.py `margins` has the definitions):
* d = the largest |u or v of the fp32 run - of the fp64 run| over the near-cone triples, by the reference's own geotrf and inv, rounded up to
  a multiple of 1e-7 px;
* a pixel is fragile if one of its triples has u or v within 16 d of a half-integer, or |z - (1 - tol) d_j| < 1e-5 |z|, or |z| < 16 d; it
  is tainted if it is fragile or lands, in fp64, in front of a tainted pixel of an earlier view;
* the two runs agree on every untainted pixel; at most 5 % of a case is tainted; every view but possibly the first has at least 8 lowered
  pixels; at least 2 % of all pixels are lowered.
A recipe that breaks a condition fails loudly: pick another seed in tests/clean_cases.py, never a wider cap."""
import argparse
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import clean_cases as C  # noqa: E402
import clean_ref as R  # noqa: E402
from oracle import cv2_stub, ref_loader  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "clean_cases.npz")
TAINTED_CAP = 0.05
D_STEP = 1e-7
MIN_LOWERED_PER_VIEW = 8
MIN_LOWERED_SHARE = 0.02


def load_reference():
    """(BasePCOptimizer, geotrf, inv) of the reference, behind the stub list of tools/make_golden_cam_pose.py"""
    sys.modules["cv2"] = cv2_stub
    ref_loader._STUB_ROOTS = tuple(r for r in ref_loader._STUB_ROOTS if r != "cv2") + (
        "roma", "torchmetrics", "pl_bolts", "open3d", "rerun", "matplotlib", "trimesh", "viser", "wandb", "sklearn", "imageio")
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        from fast3r.dust3r.cloud_opt.base_opt import BasePCOptimizer
        from fast3r.dust3r.utils.geometry import geotrf, inv
    return BasePCOptimizer, geotrf, inv


class Carrier:
    """what clean_pointcloud touches on `self`"""

    def __init__(self, s, dtype):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)  # noqa: E731
        self.n_imgs = len(s["shapes"])
        self.imshapes = [tuple(sh) for sh in s["shapes"]]
        self.im_conf = [t(c) for c in s["conf"]]
        self._poses = t(s["poses"])
        K = torch.zeros((self.n_imgs, 3, 3), dtype=dtype)
        intr = t(s["intr"])
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = intr[:, 0], intr[:, 1], intr[:, 2], intr[:, 3], 1.0
        self._K = K
        self._depth = [t(d) for d in s["depth"]]
        self._pts = [t(p) for p in s["world"]]

    def get_im_poses(self):
        return self._poses

    def get_intrinsics(self):
        return self._K

    def get_depthmaps(self):
        return self._depth

    def depth_to_pts3d(self):
        return self._pts

    def __deepcopy__(self, memo):
        other = copy.copy(self)
        other.im_conf = [c.clone() for c in self.im_conf]
        return other


def reference_run(cls, s, dtype):
    car = Carrier(s, dtype)
    res = cls.clean_pointcloud(car, tol=s["tol"], max_bad_conf=s["max_bad_conf"])
    assert all(torch.equal(a, torch.from_numpy(c).to(dtype)) for a, c in zip(car.im_conf, s["conf"]))  # the inputs are untouched
    return [c.numpy() for c in res.im_conf]


def reference_uv(geotrf, inv, s, dtype):
    """{(i, j): (u, v)} before rounding, by the reference's own inv and geotrf calls (base_opt.py:285, :298-300)"""
    car = Carrier(s, dtype)
    cams, K, out = inv(car.get_im_poses()), car.get_intrinsics(), {}
    for i, pts in enumerate(car.depth_to_pts3d()):
        for j in range(car.n_imgs):
            if i != j:
                with np.errstate(all="ignore"):
                    uv = geotrf(K[j], geotrf(cams[j], pts), norm=1, ncol=2).numpy()
                out[(i, j)] = (uv[:, 0], uv[:, 1])
    return out


def case(cls, geotrf, inv, name):
    s = C.golden_scene(name)
    r32, r64 = reference_run(cls, s, torch.float32), reference_run(cls, s, torch.float64)
    c64 = [c.astype(np.float64) for c in s["conf"]]
    changed32 = [a != c for a, c in zip(r32, s["conf"])]
    changed64 = [a != c for a, c in zip(r64, c64)]
    for a, c, ch in zip(r64, c64, changed64):  # the fp64 result holds nothing but the inputs and the clip: the mask loses nothing
        assert np.array_equal(a, np.where(ch, np.minimum(c, float(s["max_bad_conf"])), c)), name
    d = R.pixel_shift(s, reference_uv(geotrf, inv, s, torch.float32), reference_uv(geotrf, inv, s, torch.float64))
    d = float(np.ceil(d / D_STEP) * D_STEP)  # rounded up to a multiple of 1e-7 px: a last-bit difference of a BLAS does not move the file
    m = R.margins(s, d)
    tainted = [t.numpy() for t in m["tainted"]]
    total = sum(h * w for h, w in s["shapes"])
    share = sum(int(t.sum()) for t in tainted) / total
    lowered = [int(ch.sum()) for ch in changed32]
    assert d > 0 and all(np.array_equal(a[~t], b[~t]) for a, b, t in zip(changed32, changed64, tainted)), f"{name}: the fp32 and fp64 runs differ on an untainted pixel"
    assert share <= TAINTED_CAP, f"{name}: {share:.2%} of the pixels are tainted (cap {TAINTED_CAP:.0%}): pick another seed"
    assert all(n >= MIN_LOWERED_PER_VIEW for n in lowered[1:]), f"{name}: lowered per view {lowered}: pick another seed"
    assert sum(lowered) >= MIN_LOWERED_SHARE * total, f"{name}: {sum(lowered)} of {total} pixels lowered: pick another seed"
    cat = lambda xs, dt: np.concatenate([np.asarray(x).reshape(-1) for x in xs]).astype(dt)  # noqa: E731
    print(f"{name}: d = {d:.2e} px, tainted {share:.2%}, lowered {lowered} ({sum(lowered) / total:.1%})")
    return {f"{name}_seed": np.int64(C.GOLDEN[name][1]), f"{name}_conf32": cat(r32, np.float32), f"{name}_changed64": np.packbits(cat(changed64, bool)),
            f"{name}_d": np.float64(d), f"{name}_tainted": np.packbits(cat(tainted, bool)), f"{name}_tainted_share": np.float64(share),
            f"{name}_lowered": np.asarray(lowered, np.int64)}


def generate():
    torch.set_num_threads(4)
    cls, geotrf, inv = load_reference()
    data = {"conditions_ok": np.bool_(True), "tainted_cap": np.float64(TAINTED_CAP)}
    for name in C.GOLDEN:
        data.update(case(cls, geotrf, inv, name))
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
        print("clean_cases.npz reproduced array for array" if ok else "clean_cases.npz DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    np.savez_compressed(OUT, **data)
    size = os.path.getsize(OUT)
    assert size < 1000 * 1000, size
    print(f"wrote {OUT} ({size} bytes)")


if __name__ == "__main__":
    main()
