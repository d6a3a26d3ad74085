"""Camera-pose metrics, CPU side: the new C entry points are declared, exported, bound and reject bad arguments before any launch; the
committed fixture satisfies its own margin conditions and is reproduced by its generator; `correct_preds_orientation` and the
list-valued input checks of `estimate_camera_poses` (no kernel is launched here)."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cam_pose_cases as C  # noqa: E402
from oracle import fixture_io, ref_loader  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cam_pose_cases.pt")


def golden():
    return torch.load(GOLDEN, weights_only=False)


def checksum(t):
    x = t.double().reshape(-1)
    return float((x * torch.arange(1, x.numel() + 1, dtype=torch.float64)).sum())


def test_pose_metric_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f3r.h")).read(), flags=re.S)
    for name in ("f3r_pose_pair_metrics", "f3r_pose_error_stats"):
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in include/f3r.h"
        assert hasattr(built_lib, name) and name in _lib.SYMBOLS
    assert built_lib.f3r_version() >= 370 and _lib.ABI_VERSION >= 370
    import fast3r_amd
    for name in ("camera_to_rel_deg", "calculate_auc", "camera_pose_metrics"):
        assert callable(getattr(fast3r_amd, name))
    lit = fast3r_amd.MultiViewDUSt3RLitModule(net=None)
    assert lit.RRA_thresholds == [5, 15, 30] and lit.RTA_thresholds == [5, 15, 30] and lit.camera_pose_metrics_per_epoch == []


def test_pose_metric_entry_points_reject_bad_arguments(built_lib):
    l = built_lib
    F = 0x10000  # a fake device address: every call below must fail its argument checks before touching it
    thr = (ctypes.c_double * 9)(*range(1, 10))

    def pair(pred=F, gt=F, dtype=0, n_samples=1, n_views=4, n_r=3, n_t=3, n_bins=31, mx=30.0, rel_r=None, rel_t=None, counts=F, r_thr=thr, t_thr=thr):
        return l.f3r_pose_pair_metrics(pred, gt, dtype, n_samples, n_views, r_thr, n_r, t_thr, n_t, n_bins, mx, rel_r, rel_t, counts, None)

    def err():
        return l.f3r_last_error_string()

    assert pair(n_views=1) == -1 and b"n_views" in err()
    assert pair(n_views=0) == -1 and pair(n_views=-3) == -1
    assert pair(n_samples=0) == -1 and b"n_samples" in err()
    assert pair(pred=None) == -1 and b"null" in err()
    assert pair(gt=None) == -1 and b"null" in err()
    assert pair(counts=None) == -1 and b"null" in err()
    assert pair(n_r=9) == -1 and b"thresholds" in err()
    assert pair(n_t=9) == -1 and b"thresholds" in err()
    assert pair(r_thr=None) == -1 and b"threshold" in err()
    assert pair(n_bins=0) == -1 and b"n_bins" in err()
    assert pair(n_bins=257) == -1 and b"n_bins" in err()
    assert pair(dtype=2) == -1 and b"dtype" in err()
    assert pair(rel_r=F) == -1 and b"rel_r" in err()
    assert pair(mx=0.0) == -1 and b"max_threshold" in err()

    def stats(r=F, t=F, n=10, dtype=0, n_r=3, n_t=3, n_bins=31, mx=30.0, counts=F):
        return l.f3r_pose_error_stats(r, t, n, dtype, thr, n_r, thr, n_t, n_bins, mx, counts, None)

    assert stats(r=None) == -1 and b"null" in err()
    assert stats(counts=None) == -1 and b"null" in err()
    assert stats(n=-1) == -1
    assert stats(n_t=9) == -1 and b"thresholds" in err()
    assert stats(n_bins=300) == -1 and b"n_bins" in err()
    assert stats(dtype=7) == -1 and b"dtype" in err()


def test_fixture_satisfies_its_margin_conditions():
    g = golden()
    assert set(g["metric"]) == set(C.POSE_SETS) and set(g["special"]) == set(C.SPECIAL_SETS) and set(g["eval"]) == set(C.EVAL_CASES)
    assert os.path.getsize(GOLDEN) < 500 * 1000
    for name in C.EXACT_SETS:
        m = g["metric"][name]
        r, t = m["fp64"]["rel_r"], m["fp64"]["rel_t"]
        assert r.dtype == torch.float64 and m["fp32"]["rel_r"].dtype == torch.float32
        d = max(float((m["fp32"]["rel_r"].double() - r).abs().max()), float((m["fp32"]["rel_t"].double() - t).abs().max()))
        assert d == m["d"] and d > 0
        assert C.edge_distance(r, t, torch.max(r, t)) == m["edge_distance"] >= 10 * d
        assert torch.equal(m["fp32"]["counts"], m["fp64"]["counts"])
    for name in ("v64", "v1500"):
        assert g["metric"][name]["n_within_1e-9"] == 0 and g["metric"][name]["edge_distance"] >= 1e-9
    assert "rel_r" not in g["metric"]["v1500"]["fp64"] and "fp32" not in g["metric"]["v1500"]
    m = g["metric"]["v64"]
    assert C.edge_distance(m["fp64"]["rel_r"], m["fp64"]["rel_t"], torch.max(m["fp64"]["rel_r"], m["fp64"]["rel_t"])) == m["edge_distance"]
    # counts are what the per-pair arrays say
    for name in C.PER_PAIR_SETS:
        m = g["metric"][name]["fp64"]
        n = m["rel_r"].numel()
        assert n == C.POSE_SETS[name][0] * (C.POSE_SETS[name][0] - 1) // 2
        assert [int((m["rel_r"] < tau).sum()) for tau in C.RRA_THRESHOLDS] == m["counts"][:3].tolist()
        assert int(m["counts"][6:].sum()) == int((torch.max(m["rel_r"], m["rel_t"]) <= C.MAX_THRESHOLD).sum())
    for name, e in g["eval"].items():
        assert e["edge_distance"] >= 0.05, name
        assert set(e["metrics"]) == set(C.EVAL_MODES)
    assert g["special"]["trace_out_of_range"]["fp64"]["raises"] == "ValueError"
    assert g["special"]["nan_translation"]["fp64"]["n_default"] > 0


@needs_reference
def test_golden_generator_reproduces_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_cam_pose.py"), "--check"], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout + r.stderr


def test_correct_preds_orientation_matches_the_reference_and_takes_views():
    from fast3r_amd import MultiViewDUSt3RLitModule
    stored = golden()["eval"]["mixed_b2"]["oriented"]
    views, preds = C.eval_scene("mixed_b2")
    for p in preds:  # the local head's outputs too: they must be corrected when present
        p["pts3d_local"] = p["pts3d_in_other_view"] + 1.0
        p["conf_local"] = p["conf"] + 1.0
        p["pts3d_local_aligned_to_global"] = p["pts3d_in_other_view"] * 2.0
    before = [{k: v for k, v in p.items()} for p in preds]
    assert MultiViewDUSt3RLitModule.correct_preds_orientation(preds, views) is None
    H, W = C.MIXED_SCENE["H"], C.MIXED_SCENE["W"]
    for p, b, s in zip(preds, before, stored):
        assert set(p) == set(b)
        for k in p:
            assert isinstance(p[k], list) and len(p[k]) == 2
            assert tuple(p[k][0].shape[:2]) == (H, W) and tuple(p[k][1].shape[:2]) == (W, H)  # sample 1 is portrait
            for i in range(2):
                assert p[k][i].untyped_storage().data_ptr() == b[k].untyped_storage().data_ptr()  # a view: nothing copied
                assert torch.equal(p[k][i], b[k][i].transpose(0, 1) if i == 1 else b[k][i])
        for k in s:  # what the reference's method did to the same scene
            assert [tuple(x.shape) for x in p[k]] == [tuple(x) for x in s[k]["shapes"]]
            assert [checksum(x) for x in p[k]] == s[k]["checksums"]
    # views=None: untouched (reference :878)
    views, preds = C.eval_scene("mixed_b2")
    MultiViewDUSt3RLitModule.correct_preds_orientation(preds, None)
    assert torch.is_tensor(preds[0]["conf"])


def test_estimate_camera_poses_rejects_malformed_list_preds():
    from fast3r_amd import estimate_camera_poses
    pts, conf = torch.zeros(8, 12, 3), torch.ones(8, 12)
    good = {"pts3d_in_other_view": [pts, pts.transpose(0, 1)], "conf": [conf, conf.t()]}
    bad = [
        [good, {"pts3d_in_other_view": [pts], "conf": [conf]}],                                 # another number of samples
        [good, {"pts3d_in_other_view": [pts, pts], "conf": torch.stack([conf, conf])}],         # a list next to a tensor
        [good, {"pts3d_in_other_view": [pts, pts], "conf": [conf, conf.t()]}],                  # conf not the pointmap's shape
        [good, {"pts3d_in_other_view": [pts, pts[..., :2]], "conf": [conf, conf]}],             # not (H, W, 3)
        [good, {"pts3d_in_other_view": [pts, None], "conf": [conf, conf]}],                     # not a tensor
    ]
    for preds in bad:
        with pytest.raises(ValueError):
            estimate_camera_poses(preds, focal_length_estimation_method="individual")
    with pytest.raises(ValueError):
        estimate_camera_poses([good, good], focal_length_estimation_method="nope")
