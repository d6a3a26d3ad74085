"""Writes tests/golden/gt_views_cases.pt (CPU only; needs the reference checkout).  `--check` regenerates it in memory and compares it with
the committed file bit for bit.

The golden is what the reference's own dataset path returns: a subclass of `BaseStereoViewDataset` whose `_get_views` feeds seeded frames
through the reference's `_crop_resize_if_necessary`, and the class's unmodified `__getitem__` (ImgNorm, the unprojection, the mask,
`transpose_to_landscape`), with
* `cv2` replaced by tests/cv2_resize_stub.py (the one OpenCV call of that path, `resize(..., INTER_NEAREST)`, restated from OpenCV's
  definition; OpenCV is not installed, so the stand-in is pinned on that definition by tests/test_gt_views.py, not on OpenCV's binary);
* `torchvision` replaced by oracle/torchvision_stub.py plus a `ColorJitter` placeholder (the dataset package builds a jitter transform at
  import; nothing here applies it);
* `oracle.ref_loader.install()` for everything else the reference imports.
Where the reference draws the orientation of a near-square frame from its RNG, a stub `rng` forces the stored choice.

Stored: the frames (inputs), and per case the frame names, poses, resolution, the forced choices, what `__getitem__` returned per view,
and the numbers the reference passed through on the way -- the two crop boxes handed to `crop_image_depthmap`, the size handed to
`cv2.resize` and the stand-in's index tables.  Only data.  Asserted here and stored as `restatement_matches`: tests/gt_views_ref.py
reproduces every field bit for bit except `pts3d`, which it meets within the derived bound (docs/rows_f.md)."""
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

import cv2_resize_stub  # noqa: E402
import gt_views_ref as R  # noqa: E402
from oracle import ref_loader, torchvision_stub  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "gt_views_cases.pt")
VIEW_KEYS = ("img", "depthmap", "pts3d", "valid_mask", "camera_pose", "camera_intrinsics", "true_shape")


# ------------------------------------------------------------------------------------------------------------------- seeded inputs
def intrinsics(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dtype=np.float32)


def pose(rs):
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, rs.uniform(-2, 2, 3)
    return T.astype(np.float32)


def frame(seed, W, H, K):
    """random bytes everywhere (reading outside a crop window changes output bytes) and a smooth positive depth with noise"""
    rs = np.random.RandomState(seed)
    image = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1.5 + 0.5 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + 0.05 * rs.standard_normal((H, W))).astype(np.float32)
    return {"image": image, "depthmap": depth, "intrinsics": K}


def frames_and_cases():
    F = {
        "a0": frame(10, 80, 60, intrinsics(70.0, 70.5, 40.0, 30.0)),
        "a1": frame(11, 80, 60, intrinsics(70.0, 70.5, 40.0, 30.0)),
        "a2": frame(12, 80, 60, intrinsics(71.0, 69.0, 40.0, 30.0)),
        "b0": frame(20, 80, 60, intrinsics(66.0, 67.0, 40.5, 29.7)),
        "c0": frame(30, 161, 97, intrinsics(120.0, 121.0, 77.2, 50.1)),
        "p0": frame(40, 60, 80, intrinsics(55.0, 56.0, 27.0, 40.0)),
        "p1": frame(41, 60, 80, intrinsics(54.0, 57.0, 27.0, 40.0)),
        "u0": frame(50, 20, 16, intrinsics(18.0, 18.5, 10.0, 8.0)),
        "s0": frame(60, 64, 64, intrinsics(60.0, 60.0, 32.0, 32.0)),
    }
    # case 7: zeros, negatives, and one pixel of 3.0e38 where |u - cu| / fu > 2: x_cam overflows in the fp32 cast
    wide = frame(70, 80, 60, intrinsics(5.0, 5.0, 40.0, 30.0))
    d = wide["depthmap"]
    d[5:9, 10:30] = 0.0
    d[20:24, 40:70] = -1.0
    xs, ys = cv2_resize_stub.nn_indices(80, 32), cv2_resize_stub.nn_indices(60, 24)
    d[ys[12], xs[30]] = 3.0e38   # lands at output pixel (12, 30): cu is 15.7 there and fu 2, so |u - cu| / fu = 7.15
    F["w0"] = wide
    rs = np.random.RandomState(7)
    P = {name: pose(rs) for name in F}
    cases = {
        "1_plain_lanczos": (["a0"], True, (32, 24), [False]),
        "2_half_even_square_target": (["b0"], True, (32, 32), [False]),
        "3_odd_sizes": (["c0"], True, (70, 38), [False]),
        "4_portrait": (["p0"], True, (32, 24), [False]),
        "5_upscale_bicubic": (["u0"], True, (32, 24), [False]),
        "6_square_landscape": (["s0"], True, (32, 24), [False]),
        "6_square_portrait": (["s0"], True, (32, 24), [True]),
        "7_depth_edge_values": (["w0"], True, (32, 24), [False]),
        "8_three_views_one_geometry": (["a0", "a1", "a2"], True, (32, 24), [False] * 3),
        "8_four_views_two_geometries": (["a1", "p0", "a2", "p1"], True, (32, 24), [False] * 4),
        "9_no_pose": (["a0"], False, (32, 24), [False]),
    }
    return F, P, cases


# ------------------------------------------------------------------------------------------------------------------- the reference
class ForcedRng:
    """stands in for the generator `_crop_resize_if_necessary` draws the orientation of a near-square frame from"""

    def __init__(self, choice):
        self.choice, self.draws = int(bool(choice)), 0

    def integers(self, *args, **kwargs):
        self.draws += 1
        return self.choice


def load_reference(record):
    cv2 = types.ModuleType("cv2")
    for name in dir(cv2_resize_stub):
        if name.isupper():
            setattr(cv2, name, getattr(cv2_resize_stub, name))

    def resize(src, dsize, *args, **kwargs):
        dsize = tuple(int(v) for v in dsize)
        record.append(("resize", tuple(src.shape), dsize))
        return cv2_resize_stub.resize(src, dsize, *args, **kwargs)

    cv2.resize = resize
    sys.modules["cv2"] = cv2
    torchvision_stub.install()
    sys.modules["torchvision.transforms"].ColorJitter = lambda *a, **k: (lambda x: x)   # built at import by datasets/utils/transforms.py, never applied
    ref_loader.install()
    with contextlib.redirect_stdout(io.StringIO()):
        import fast3r.dust3r.datasets.base.base_stereo_view_dataset as base
        import fast3r.dust3r.datasets.utils.cropping as cropping
    assert cropping.cv2 is cv2
    crop = cropping.crop_image_depthmap

    def recording_crop(image, depthmap, camera_intrinsics, crop_bbox):
        record.append(("crop", tuple(int(v) for v in crop_bbox)))
        return crop(image, depthmap, camera_intrinsics, crop_bbox)

    cropping.crop_image_depthmap = recording_crop
    return base


def dataset_class(base):
    class GoldenFrames(base.BaseStereoViewDataset):
        def __init__(self, frames, poses, choices, **kw):
            super().__init__(**kw)
            self.frames, self.poses, self.choices, self.scenes = frames, poses, choices, [0]

        def _get_views(self, idx, resolution, rng):
            views = []
            for i, f in enumerate(self.frames):
                forced = ForcedRng(self.choices[i])
                img, depth, K = self._crop_resize_if_necessary(f["image"].copy(), f["depthmap"].copy(), f["intrinsics"].copy(), resolution, rng=forced,
                                                               info=str(i))
                view = dict(img=img, depthmap=depth, camera_intrinsics=K, dataset="golden", label=f"scene/{i}", instance=str(i))
                if self.poses is not None:
                    view["camera_pose"] = self.poses[i].copy()
                views.append(view)
            return views

    return GoldenFrames


def to_tensor(x):
    if isinstance(x, torch.Tensor):
        return x.clone()
    return torch.from_numpy(np.ascontiguousarray(x))


def generate():
    warnings.filterwarnings("ignore")
    record = []
    base = load_reference(record)
    Dataset = dataset_class(base)
    F, P, cases = frames_and_cases()
    out = {"frames": {k: {kk: to_tensor(vv) for kk, vv in f.items()} for k, f in F.items()}, "poses": {k: to_tensor(v) for k, v in P.items()},
           "cases": {}}
    worst = 0.0
    for name, (names, with_pose, resolution, choices) in cases.items():
        frames = [F[k] for k in names]
        poses = [P[k] for k in names] if with_pose else None
        del record[:]
        views = Dataset(frames, poses, choices, split="test", resolution=resolution, seed=1)[0]
        assert len(views) == len(names) and len(record) == 3 * len(names), (name, record)
        mine = R.build([f["image"] for f in frames], [f["depthmap"] for f in frames], [f["intrinsics"] for f in frames], poses, resolution, choices)
        stored = []
        for i, (view, ref) in enumerate(zip(views, mine)):
            (_, box1), (_, src_shape, dsize), (_, box2) = record[3 * i:3 * i + 3]
            trace = {"box1": box1, "box2": box2, "resized": dsize, "nearest_x": to_tensor(cv2_resize_stub.nn_indices(src_shape[1], dsize[0]).astype(np.int32)),
                     "nearest_y": to_tensor(cv2_resize_stub.nn_indices(src_shape[0], dsize[1]).astype(np.int32))}
            assert view["idx"] == (0, 0, i) and view["true_shape"].dtype == np.int32 and view["img"].dtype == torch.float32
            for key in R.KEYS_EXACT:
                got = view[key].numpy() if torch.is_tensor(view[key]) else np.asarray(view[key])
                assert got.dtype == ref[key].dtype and got.shape == ref[key].shape and got.tobytes() == ref[key].tobytes(), \
                    f"tests/gt_views_ref.py differs from the reference on {name}, view {i}, {key}"
            assert np.array_equal(view["camera_pose"], ref["camera_pose"], equal_nan=True)
            ok, ratio = R.pts3d_close(np.asarray(view["pts3d"]), ref)
            assert ok, (name, i, ratio)
            worst = max(worst, ratio)
            for key in ("box1", "box2", "resized"):
                assert tuple(ref["trace"][key]) == tuple(trace[key]), (name, i, key)
            assert np.array_equal(ref["trace"]["nearest_x"], trace["nearest_x"].numpy()) and np.array_equal(ref["trace"]["nearest_y"], trace["nearest_y"].numpy())
            stored.append(dict({key: to_tensor(view[key]) for key in VIEW_KEYS}, trace=trace))
        out["cases"][name] = {"frames": list(names), "with_pose": with_pose, "resolution": tuple(resolution), "square_portrait": list(choices),
                              "views": stored}
    edge = out["cases"]["7_depth_edge_values"]["views"][0]
    assert not torch.isfinite(edge["pts3d"][12, 30]).all() and not edge["valid_mask"][12, 30] and edge["depthmap"][12, 30] == 3.0e38
    assert (edge["depthmap"] == 0).any() and (edge["depthmap"] < 0).any()
    assert tuple(out["cases"]["4_portrait"]["views"][0]["true_shape"].tolist()) == (32, 24)
    assert out["cases"]["2_half_even_square_target"]["views"][0]["trace"]["box2"][0] > 0
    assert out["cases"]["3_odd_sizes"]["views"][0]["trace"]["box1"][1] > 0
    out["restatement_matches"] = True
    return out, worst


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
    data, worst = generate()
    print(f"tests/gt_views_ref.py: every exact field reproduced; pts3d at most {worst:.3f} of the derived bound from the reference")
    if args.check:
        ok = same(data, torch.load(OUT, weights_only=False))
        print("gt_views_cases.pt reproduced bit for bit" if ok else "gt_views_cases.pt DIFFERS from a fresh generation")
        sys.exit(0 if ok else 1)
    torch.save(data, OUT)
    size = os.path.getsize(OUT)
    assert size < 1000 * 1000, size
    print(f"wrote {OUT} ({size} bytes, {len(data['cases'])} cases)")


if __name__ == "__main__":
    main()
