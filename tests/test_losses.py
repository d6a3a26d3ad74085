"""The validation loss, CPU side: the new C entry points are declared, exported, bound and reject bad arguments before any launch; the
loss classes have the reference's constructor signatures, raise what their docstring lists and name their outputs as the reference does;
the committed fixture is reproduced by its generator; model_step / validation_step keep their books (no kernel is launched here)."""
import ctypes
import inspect
import math
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loss_cases as C  # noqa: E402
import loss_ref  # noqa: E402
from oracle import ref_loader  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss_cases.pt")
NAMES = ("f3r_mv_conf_loss", "f3r_mv_conf_loss_workspace_bytes")


def test_loss_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f3r.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} not declared in include/f3r.h"
        assert hasattr(built_lib, name) and name in _lib.SYMBOLS
    assert built_lib.f3r_version() >= 380 and _lib.ABI_VERSION >= 380
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert "f3r_mv_conf_loss" in open(os.path.join(ROOT, doc)).read(), doc
    import fast3r_amd
    for name in ("L21Loss", "L21", "Regr3DMultiviewV3", "Regr3DMultiviewV4", "ConfLossMultiviewV2"):
        assert hasattr(fast3r_amd, name) and hasattr(fast3r_amd.losses, name)


def test_workspace_is_independent_of_the_pixel_count(built_lib):
    l = built_lib
    assert l.f3r_mv_conf_loss_workspace_bytes(0, 1) == 0 and l.f3r_mv_conf_loss_workspace_bytes(1, 0) == 0
    small, big = l.f3r_mv_conf_loss_workspace_bytes(2, 1), l.f3r_mv_conf_loss_workspace_bytes(320, 1)
    assert 0 < small < big < 1 << 20  # O(workgroups + views x samples): under 1 MiB for 320 views of any size


def test_loss_entry_point_rejects_bad_arguments(built_lib):
    l = built_lib
    F = 0x10000  # a fake device address: every call below must fail its argument checks before touching it

    def call(gt=F, valid=F, pose=F, pose_dtype=0, pred=F, conf=F, pred_l=F, conf_l=F, npix=F, V=3, B=2, version=4, dis=0, gt_scale=0, lsc=0,
             use_clip=0, clip=0.0, alpha=0.2, ws=F, ws_bytes=None, out=F):
        if ws_bytes is None:
            ws_bytes = l.f3r_mv_conf_loss_workspace_bytes(max(V, 1), max(B, 1))
        return l.f3r_mv_conf_loss(gt, valid, pose, pose_dtype, pred, conf, pred_l, conf_l, npix, V, B, version, dis, gt_scale, lsc, use_clip, clip,
                                  alpha, ws, ws_bytes, out, None)

    def err():
        return l.f3r_last_error_string()

    for table in ("gt", "valid", "pose", "pred", "conf", "npix"):
        assert call(**{table: None}) == -1 and b"null table" in err(), table
    assert call(ws=None) == -1 and b"null" in err()
    assert call(out=None) == -1 and b"null" in err()
    assert call(V=0) == -1 and b"n_views" in err()
    assert call(V=-2) == -1 and call(B=0) == -1 and b"n_samples" in err()
    assert call(alpha=0.0) == -1 and b"alpha" in err()
    assert call(alpha=-1.0) == -1 and call(alpha=float("nan")) == -1 and b"alpha" in err()
    assert call(version=2) == -1 and b"unknown mode" in err()
    assert call(version=5) == -1 and b"unknown mode" in err()
    assert call(dis=2) == -1 and b"unknown mode" in err()
    assert call(version=3, lsc=1) == -1 and b"local_scale_consistent" in err()
    assert call(pose_dtype=2) == -1 and b"pose_dtype" in err()
    assert call(pred_l=None) == -1 and b"local confidence table without a local points table" in err()
    assert call(conf_l=None) == -1 and b"local" in err()
    assert call(use_clip=1, clip=float("nan")) == -1 and b"dist_clip" in err()
    assert call(ws_bytes=64) == -1 and b"workspace" in err()


def test_constructor_signatures_match_the_reference():
    from fast3r_amd import losses as L

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]

    assert sig(L.Regr3DMultiviewV3) == [("criterion", inspect.Parameter.empty), ("norm_mode", "avg_dis"), ("gt_scale", False)]
    assert sig(L.Regr3DMultiviewV4) == [("criterion", inspect.Parameter.empty), ("norm_mode", "avg_dis"), ("gt_scale", False),
                                        ("local_scale_consistent", False)]
    assert sig(L.ConfLossMultiviewV2) == [("pixel_loss", inspect.Parameter.empty), ("alpha", 1)]
    assert sig(L.L21Loss) == [("reduction", "mean")] and isinstance(L.L21, L.L21Loss)


SIGNATURE_PROBE = """
import inspect, json, sys
sys.path.insert(0, sys.argv[1])
import make_golden_loss
R = make_golden_loss.load_reference()
names = ("L21Loss", "Regr3DMultiviewV3", "Regr3DMultiviewV4", "ConfLossMultiviewV2")
sigs = {n: [(p.name, None if p.default is inspect.Parameter.empty else repr(p.default)) for p in inspect.signature(getattr(R, n)).parameters.values()] for n in names}
crit = R.ConfLossMultiviewV2(R.Regr3DMultiviewV4(R.L21, norm_mode="avg_dis"), alpha=0.2)
print(json.dumps({"sigs": sigs, "repr": repr(crit), "repr3": repr(3 * crit)}))
"""


@needs_reference
def test_constructor_signatures_are_the_reference_s_own():
    """asked of the reference in a child process: loading it changes sys.path and the import stubs"""
    import json
    r = subprocess.run([sys.executable, "-c", SIGNATURE_PROBE, os.path.join(ROOT, "tools")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    theirs = json.loads(r.stdout.strip().splitlines()[-1])
    from fast3r_amd import losses as L
    for name, want in theirs["sigs"].items():
        ours = [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(getattr(L, name)).parameters.values()]
        assert ours == want, name
    released = L.ConfLossMultiviewV2(L.Regr3DMultiviewV4(L.L21, norm_mode="avg_dis"), alpha=0.2)
    assert repr(released) == theirs["repr"] and repr(3 * released) == theirs["repr3"]


def test_construction_time_errors_and_operators():
    from fast3r_amd import losses as L
    for cls in (L.Regr3DMultiviewV3, L.Regr3DMultiviewV4):
        for mode in ("avg_warp-log1p", "median_warp-log1p"):
            with pytest.raises(ValueError, match="warp-log1p"):
                cls(L.L21, norm_mode=mode)
        for mode in ("", None):
            with pytest.raises(ValueError, match="empty"):
                cls(L.L21, norm_mode=mode)
        with pytest.raises(ValueError):
            cls(L.L21, norm_mode="mean_dis")
        with pytest.raises(ValueError):
            cls(L.L21, norm_mode="avg_sqrt")
    for mode in ("median_dis", "median_log1p"):
        with pytest.raises(ValueError, match="median"):
            L.Regr3DMultiviewV4(L.L21, norm_mode=mode)
        with pytest.raises(NotImplementedError, match="median"):
            L.Regr3DMultiviewV3(L.L21, norm_mode=mode)
    with pytest.raises(AssertionError):
        L.ConfLossMultiviewV2(L.Regr3DMultiviewV4(L.L21), alpha=0)
    with pytest.raises(AssertionError):
        L.Regr3DMultiviewV4("L21")
    pixel = L.Regr3DMultiviewV4(L.L21, norm_mode="avg_log1p", gt_scale=True, local_scale_consistent=True)
    with pytest.raises(NotImplementedError):
        pixel([], [])
    crit = L.ConfLossMultiviewV2(pixel, alpha=0.2)
    assert crit.pixel_loss.criterion.reduction == "none" and pixel.criterion.reduction == "mean"  # with_reduction copies
    assert (crit.alpha, crit.pixel_loss.norm_mode, crit.pixel_loss.gt_scale, crit.pixel_loss.local_scale_consistent) == (0.2, "avg_log1p", True, True)
    assert (2 * crit)._alpha == 2 and (crit * 0.5)._alpha == 0.5 and crit._alpha == 1
    with pytest.raises(NotImplementedError):
        crit + crit
    assert repr(crit) == "ConfLossMultiviewV2(Regr3DMultiviewV4(L21Loss()))" and repr(2 * crit).startswith("2*")


def test_cpu_preds_raise():
    from fast3r_amd import _lib, losses as L
    views, preds = C.build("b1_v2_global")
    with pytest.raises(_lib.F3RError):
        L.ConfLossMultiviewV2(L.Regr3DMultiviewV4(L.L21), alpha=0.2)(views, preds)


def expected_keys(n_views, local):
    kinds = ["global", "local"] if local else ["global"]
    return ([f"Regr3DMultiviewV3_pts3d_loss_{k}/{v:02d}" for k in kinds for v in range(n_views)]
            + [f"ConfLossMultiviewV2_conf_loss_{k}/{v:02d}" for k in kinds for v in range(n_views)])


def test_fixture_holds_every_case_with_the_reference_s_key_order():
    g = torch.load(GOLDEN, weights_only=False)
    assert list(g) == list(C.CASES) and os.path.getsize(GOLDEN) < 200 * 1000
    for name, case in g.items():
        r = C.CASES[name]
        want = expected_keys(len(r["shapes"]), r["local"])
        assert list(case["ref32"]["details"]) == want and list(case["ref64"]["details"]) == want, name  # the reference's own insertion order
        assert list(case["d"]) == ["loss"] + want
        for k in want:
            a, b = case["ref32"]["details"][k], case["ref64"]["details"][k]
            assert math.isnan(a) == math.isnan(b) and (math.isnan(a) or abs(a - b) == case["d"][k])
    e = g["empty_view"]["ref32"]["details"]
    assert e["ConfLossMultiviewV2_conf_loss_global/01"] == 0.0 and math.isnan(e["Regr3DMultiviewV3_pts3d_loss_local/01"])
    assert math.isfinite(g["empty_sample"]["ref32"]["loss"])
    assert abs(g["v3_b2"]["ref32"]["loss"] - g["v4_b2_same_inputs"]["ref32"]["loss"]) > 1e-4
    assert g["dist_clip"]["masks_differ_at"] > 0 and g["dist_clip"]["clip_margin"] >= 1e-4
    assert g["pose_fp64"]["recipe"]["pose_fp64"] and C.build("pose_fp64")[0][1]["camera_pose"].dtype == torch.float64


@pytest.mark.parametrize("name", ["released_local", "v3_b2", "dist_clip", "nan_pred_v4"])
def test_restatement_reproduces_its_recorded_outputs(name):
    """tests/loss_ref.py against what the generator stored from it (to 1e-12: fp64 sums may be ordered differently on another host) and,
    through the recorded d, against the reference's fp32 run; the inputs rebuild to the recorded checksums"""
    case = torch.load(GOLDEN, weights_only=False)[name]
    views, preds = C.build(name)
    for k, v in C.checksums(views, preds).items():
        assert v == pytest.approx(case["checksums"][k], rel=1e-12, abs=1e-12), k
    r = C.CASES[name]
    loss, details = loss_ref.multiview_conf_loss(views, preds, version=r["version"], alpha=C.ALPHA, **C.criterion_kwargs(r), **C.call_kwargs(r))
    got, want = {"loss": loss, **details}, {"loss": case["ref64"]["loss"], **case["ref64"]["details"]}
    assert list(got) == list(want)
    for k in want:
        assert math.isnan(got[k]) == math.isnan(want[k]), k
        if not math.isnan(want[k]):
            assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), k


@needs_reference
def test_golden_generator_reproduces_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_loss.py"), "--check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ model_step / validation_step
class StubNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def forward(self, views):
        self.seen.append(views)
        return [{"pts3d_in_other_view": v["pts3d"] + self.w, "conf": torch.ones(v["pts3d"].shape[:3])} for v in views]


class StubCriterion:
    def __init__(self):
        self.calls = []

    def __call__(self, views, preds):
        self.calls.append((views, preds))
        n = len(self.calls)
        return torch.tensor(0.5 * n), {"Regr3DMultiviewV3_pts3d_loss_global/00": 1.0 * n, "Regr3DMultiviewV3_pts3d_loss_global/01": 3.0 * n,
                                       "ConfLossMultiviewV2_conf_loss_global/00": -1.0 * n, "no_view_number": 7.0}


def stub_batch(dataset):
    return [{"img": torch.zeros(1, 3, 4, 6), "pts3d": torch.ones(1, 4, 6, 3), "valid_mask": torch.ones(1, 4, 6, dtype=torch.bool),
             "camera_pose": torch.eye(4)[None], "dataset": [dataset], "true_shape": torch.tensor([[4, 6]])} for _ in range(2)]


def make_lit(criterion="stub"):
    from fast3r_amd import MultiViewDUSt3RLitModule
    crit = StubCriterion() if criterion == "stub" else criterion
    lit = MultiViewDUSt3RLitModule(net=StubNet(), validation_criterion=crit)
    lit.pose_calls, lit.recon_calls = [], []
    lit.evaluate_camera_poses = lambda views, preds, **kw: lit.pose_calls.append(kw)
    lit.evaluate_reconstruction = lambda views, preds, **kw: lit.recon_calls.append(kw)
    return lit, crit


def test_model_step_runs_forward_and_criterion():
    lit, crit = make_lit()
    assert lit.current_epoch == 0 and lit.val_losses == [] and lit.val_loss_details_per_epoch == {} and lit.device == torch.device("cpu")
    batch = stub_batch("Co3d_v2")
    views, preds, loss, details = lit.model_step(batch, crit)
    assert views is batch and len(preds) == 2 and crit.calls[0][0] is batch and crit.calls[0][1] is preds
    assert float(loss) == 0.5 and details["no_view_number"] == 7.0
    views, preds, loss, details = lit.model_step(stub_batch("x"), None)
    assert loss is None and details is None and len(preds) == 2
    got = lit.model_step(stub_batch("x"), lambda v, p: ("any", {"callable": 1.0}))
    assert got[2] == "any" and got[3] == {"callable": 1.0}


def test_validation_step_bookkeeping_routing_and_epoch_gating():
    from fast3r_amd import MultiViewDUSt3RLitModule
    with pytest.raises(ValueError, match="validation_criterion"):
        MultiViewDUSt3RLitModule.load_for_inference(StubNet()).validation_step(stub_batch("dtu"), 0)
    lit, crit = make_lit()
    assert lit.validation_step(stub_batch("Co3d_v2"), 0) == 0.5
    assert lit.pose_calls == [{"niter_PnP": 100, "focal_length_estimation_method": "first_view_from_global_head"}] and lit.recon_calls == []
    assert lit.validation_step(stub_batch("dtu"), 1, dataloader_idx=1) == 1.0
    recon_kw = {"dataset_name": "dtu", "use_pts3d_from_local_head": True, "min_conf_thr_percentile_for_local_alignment_and_icp": 85,
                "min_conf_thr_percentile_for_metric_cacluation": 0}
    assert lit.recon_calls == [recon_kw] and len(lit.pose_calls) == 1
    assert lit.validation_step(stub_batch("scannetpp"), 2) == 1.5  # neither evaluation
    assert len(lit.recon_calls) == 1 and len(lit.pose_calls) == 1
    assert lit.val_losses == [0.5, 1.0, 1.5]
    d = lit.val_loss_details_per_epoch
    assert list(d) == ["Co3d_v2", "dtu", "scannetpp"]
    assert d["dtu"] == {"val_detail_dtu_Regr3DMultiviewV3_pts3d_loss_global/00": [2.0], "val/dtu_Regr3DMultiviewV3_pts3d_loss_global": [2.0, 6.0],
                        "val_detail_dtu_Regr3DMultiviewV3_pts3d_loss_global/01": [6.0], "val_detail_dtu_ConfLossMultiviewV2_conf_loss_global/00": [-2.0],
                        "val/dtu_ConfLossMultiviewV2_conf_loss_global": [-2.0], "val_detail_dtu_no_view_number": [7.0]}
    # epoch gating of the reconstruction metrics: epochs 0, 4, 9, ... only; 7scenes and nrgbd are routed like dtu
    for epoch, name, expect in ((1, "dtu", False), (3, "7scenes", False), (4, "7scenes", True), (5, "nrgbd", False), (9, "nrgbd", True), (0, "nrgbd", True)):
        lit.current_epoch, before = epoch, len(lit.recon_calls)
        lit.validation_step(stub_batch(name), 0)
        assert (len(lit.recon_calls) == before + 1) == expect, (epoch, name)
        if expect:
            assert lit.recon_calls[-1]["dataset_name"] == name
    lit.eval_use_pts3d_from_local_head = False
    lit.current_epoch = 0
    lit.validation_step(stub_batch("dtu"), 0)
    assert lit.recon_calls[-1]["use_pts3d_from_local_head"] is False
    out = lit.on_validation_epoch_end()
    assert out["val/loss"] == pytest.approx(sum(0.5 * n for n in range(1, 11)) / 10)
    assert out["val_detail_Co3d_v2_Regr3DMultiviewV3_pts3d_loss_global/01"] == 3.0 and out["val/Co3d_v2_Regr3DMultiviewV3_pts3d_loss_global"] == 2.0
    assert lit.val_losses == [] and lit.val_loss_details_per_epoch == {}
    assert math.isnan(lit.on_validation_epoch_end()["val/loss"])
