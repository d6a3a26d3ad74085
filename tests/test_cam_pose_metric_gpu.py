"""Camera-pose metrics on the GPU against tests/golden/cam_pose_cases.pt (tools/make_golden_cam_pose.py: the reference's own
camera_to_rel_deg / calculate_auc in fp32 and fp64, and its evaluate_camera_poses around oracle/cv2_stub.py).

Tolerances, none of them taken from the code under test:
* per-pair errors against the fp64 golden: 1e-5 degrees.  The worst-conditioned step is acos(sqrt(1 - x)) at the clamp x = 1e-15,
  where its slope is 1.6e7: an fp64 rounding of x moves the angle by about 2e-7 degrees; 1e-5 is 50 x that;
* per-pair errors against the fp32 golden: 2 d of that case, d = the stored max |fp32 reference - fp64 reference|;
* counts, RRA, RTA and mAA: bit for bit -- against both goldens up to 12 views (the fixture's margin of 10 d makes the three runs count
  alike), against the fp64 golden at 64 and 1500 views (no pair within 1e-9 degrees of a threshold or edge)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cam_pose_cases as C  # noqa: E402
from oracle import fixture_io  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_FP64_DEG = 1e-5
N_R, N_T = len(C.RRA_THRESHOLDS), len(C.RTA_THRESHOLDS)


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(ROOT, "tests", "golden", "cam_pose_cases.pt"), weights_only=False)


def bits(x):
    return np.float64(x).tobytes()


def metrics(pred, gt):
    from fast3r_amd import camera_pose_metrics
    return camera_pose_metrics(pred, gt, C.RRA_THRESHOLDS, C.RTA_THRESHOLDS, C.MAX_THRESHOLD)


def counts_of(pred, gt, want_pairs=False):
    from fast3r_amd import post_ops
    return post_ops.pose_pair_metrics(pred, gt, C.RRA_THRESHOLDS, C.RTA_THRESHOLDS, C.N_BINS, float(C.MAX_THRESHOLD), want_pairs=want_pairs)


def assert_dict_equals_golden(res, ref, what):
    want = {f"RRA_at_{tau}": ref["RRA"][k] for k, tau in enumerate(C.RRA_THRESHOLDS)}
    want.update({f"RTA_at_{tau}": ref["RTA"][k] for k, tau in enumerate(C.RTA_THRESHOLDS)})
    want["mAA_30"] = ref["mAA"]
    assert set(res) == set(want), what
    for k in want:
        print(what, k, res[k], want[k])
        assert isinstance(res[k], float) and bits(res[k]) == bits(want[k]), (what, k, res[k], want[k])


@pytest.mark.parametrize("name", C.PER_PAIR_SETS)
def test_per_pair_errors_match_both_reference_runs(built_lib, golden, name):
    from fast3r_amd import camera_to_rel_deg
    m = golden["metric"][name]
    pred, gt = C.pose_set(*C.POSE_SETS[name])
    for dtype in (torch.float32, torch.float64):
        r, t = camera_to_rel_deg(pred.to(dtype).cuda(), gt.to(dtype).cuda(), "cuda", len(pred))
        assert r.is_cuda and r.dtype == t.dtype == dtype and r.shape == t.shape == m["fp64"]["rel_r"].shape
        r, t = r.cpu().double(), t.cpu().double()
        e64 = max(float((r - m["fp64"]["rel_r"]).abs().max()), float((t - m["fp64"]["rel_t"]).abs().max()))
        e32 = max(float((r - m["fp32"]["rel_r"].double()).abs().max()), float((t - m["fp32"]["rel_t"].double()).abs().max()))
        print(name, dtype, "max |kernel - fp64 golden| =", e64, " max |kernel - fp32 golden| =", e32, " d =", m["d"])
        assert e64 <= TOL_FP64_DEG  # also for fp32 output: half an fp32 ulp below 256 degrees is 7.6e-6
        assert e32 <= 2 * m["d"]


@pytest.mark.parametrize("name", list(C.POSE_SETS))
def test_counts_and_metrics_equal_the_goldens_bit_for_bit(built_lib, golden, name):
    m = golden["metric"][name]
    pred, gt = C.pose_set(*C.POSE_SETS[name])
    for dtype in (torch.float32, torch.float64):
        p, g = pred.to(dtype).cuda()[None], gt.to(dtype).cuda()[None]
        counts, rel_r, rel_t = counts_of(p, g)
        assert rel_r is None and rel_t is None
        c = counts[0].cpu()
        print(name, dtype, c.tolist())
        assert torch.equal(c[:N_R + N_T + C.N_BINS], m["fp64"]["counts"]) and c[-2:].tolist() == [0, 0]
        res = metrics(p, g)
        assert len(res) == 1
        if dtype == torch.float64:
            assert_dict_equals_golden(res[0], m["fp64"], f"{name} fp64")
        elif name in C.EXACT_SETS:
            assert torch.equal(c[:N_R + N_T + C.N_BINS], m["fp32"]["counts"])
            assert_dict_equals_golden(res[0], m["fp32"], f"{name} fp32")


def test_v1500_counts_only_equals_counts_of_own_pairs_and_pair_order(built_lib):
    from fast3r_amd import post_ops
    V = 1500
    pred, gt = C.pose_set(*C.POSE_SETS["v1500"])
    p, g = pred.cuda()[None], gt.cuda()[None]
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    counts, _, _ = counts_of(p, g)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < 64 * 1024  # nothing of size O(pairs) = 4.5 MB per array was allocated
    counts2, rel_r, rel_t = counts_of(p, g, want_pairs=True)
    assert torch.equal(counts, counts2)
    assert rel_r.shape == (1, V * (V - 1) // 2)
    # fp32 per-pair output rounds the fp64 errors, so the recount runs on the fp64 input's own pairs
    c64, r64, t64 = counts_of(p.double(), g.double(), want_pairs=True)
    recount = post_ops.pose_error_stats(r64[0], t64[0], C.RRA_THRESHOLDS, C.RTA_THRESHOLDS, C.N_BINS, float(C.MAX_THRESHOLD))
    assert torch.equal(c64, counts) and torch.equal(recount[:-2], counts[0, :-2])
    r_cpu, t_cpu = r64[0].cpu(), t64[0].cpu()
    host = [int((r_cpu < tau).sum()) for tau in C.RRA_THRESHOLDS] + [int((t_cpu < tau).sum()) for tau in C.RTA_THRESHOLDS]
    assert host == counts[0, :N_R + N_T].tolist()
    # pair (i, j) sits where torch.combinations puts it
    comb = torch.combinations(torch.arange(V), 2)
    from fast3r_amd import camera_to_rel_deg
    for idx in (0, 1, V - 2, V - 1, 123456, 777777, comb.shape[0] - 2, comb.shape[0] - 1):
        i, j = comb[idx].tolist()
        r2, t2 = camera_to_rel_deg(pred[[i, j]].double().cuda(), gt[[i, j]].double().cuda())
        assert float(r2[0]) == float(r_cpu[idx]) and float(t2[0]) == float(t_cpu[idx]), (idx, i, j)


@pytest.mark.parametrize("name", C.SPECIAL_SETS)
def test_special_sets_behave_as_recorded(built_lib, golden, name):
    from fast3r_amd import camera_to_rel_deg
    s = golden["special"][name]
    pred, gt = C.special_set(name)
    if "raises" in s["fp64"]:
        for dtype in (torch.float32, torch.float64):
            with pytest.raises(ValueError, match="trace outside valid range"):
                camera_to_rel_deg(pred.to(dtype).cuda(), gt.to(dtype).cuda())
            with pytest.raises(ValueError, match="trace outside valid range"):
                metrics(pred.to(dtype).cuda()[None], gt.to(dtype).cuda()[None])
        counts, _, _ = counts_of(pred.cuda()[None], gt.cuda()[None])
        assert int(counts[0, -2]) > 0
        return
    ref = s["fp64"]
    r, t = camera_to_rel_deg(pred.double().cuda(), gt.double().cuda())
    r, t = r.cpu(), t.cpu()
    assert torch.equal(torch.isnan(r), torch.isnan(ref["rel_r"])) and not torch.isnan(t).any()
    ok = ~torch.isnan(r)
    e = max(float((r - ref["rel_r"])[ok].abs().max()), float((t - ref["rel_t"]).abs().max()))
    print(name, "max |kernel - fp64 golden| =", e, r[:4].tolist(), t[:4].tolist())
    assert e <= TOL_FP64_DEG
    for dtype in (torch.float32, torch.float64):
        counts, _, _ = counts_of(pred.to(dtype).cuda()[None], gt.to(dtype).cuda()[None])
        c = counts[0].cpu()
        assert torch.equal(c[:N_R + N_T + C.N_BINS], ref["counts"]), (name, c.tolist())
        assert int(c[-2]) == 0 and int(c[-1]) == ref["n_default"]
        assert_dict_equals_golden(metrics(pred.to(dtype).cuda()[None], gt.to(dtype).cuda()[None])[0], s["fp64" if dtype == torch.float64 else "fp32"], name)
    if name == "pred_is_gt":
        assert float((r - 0.4051).abs().max()) < 1e-3      # identical rotations score 0.4051 degrees, not 0
    if name == "opposite_translation":
        assert float(t.max()) < 1e-5                         # blind to sign
    if name == "identity_pred":
        assert float((t - 90.0).abs().max()) < 1e-9
    if name == "half_turn":
        assert float(r.max()) > 179.5                        # the lower extrapolation branch
    if name == "nan_translation":
        assert float(t.max()) == 1e6 * 180.0 / np.pi and ref["n_default"] == 4


def test_batches_dtypes_and_cpu_resident_inputs(built_lib, golden):
    from fast3r_amd import calculate_auc, camera_to_rel_deg
    names = ("v8", "v12", "v3")
    # B = 3 of one size: three seeds of 8 views against single-sample launches
    sets = [C.pose_set(8, s) for s in (0, 1, 2)]
    pred, gt = torch.stack([p for p, _ in sets]), torch.stack([g for _, g in sets])
    for dtype in (torch.float32, torch.float64):
        batched = metrics(pred.to(dtype).cuda(), gt.to(dtype).cuda())
        single = [metrics(pred[b:b + 1].to(dtype).cuda(), gt[b:b + 1].to(dtype).cuda())[0] for b in range(3)]
        assert batched == single and len(batched) == 3
        assert_dict_equals_golden(batched[0], golden["metric"]["v8"]["fp64" if dtype == torch.float64 else "fp32"], f"B=3 sample 0 {dtype}")
    assert batched[0] != batched[1]
    # CPU-resident inputs go up and come back
    for name in names:
        m = golden["metric"][name]
        p, g = C.pose_set(*C.POSE_SETS[name])
        assert_dict_equals_golden(metrics(p[None], g[None])[0], m["fp32"], f"{name} cpu")
        r, t = camera_to_rel_deg(p.double(), g.double(), "cpu", len(p))
        assert not r.is_cuda and r.dtype == torch.float64
        assert float((r - m["fp64"]["rel_r"]).abs().max()) <= TOL_FP64_DEG and float((t - m["fp64"]["rel_t"]).abs().max()) <= TOL_FP64_DEG
        # calculate_auc on the reference's own per-pair arrays: bit-identical in both dtypes, on either device
        for key, dtype in (("fp32", torch.float32), ("fp64", torch.float64)):
            for dev in ("cpu", "cuda"):
                auc = calculate_auc(m[key]["rel_r"].to(dev), m[key]["rel_t"].to(dev), max_threshold=C.MAX_THRESHOLD)
                assert auc.dtype == dtype and auc.dim() == 0 and auc.device.type == dev
                assert bits(auc.item()) == bits(m[key]["mAA"]), (name, key, dev)
    with pytest.raises(ValueError):
        metrics(torch.eye(4)[None, None].cuda(), torch.eye(4)[None, None].cuda())  # one view: no pair


def _lit():
    from fast3r_amd import MultiViewDUSt3RLitModule
    return MultiViewDUSt3RLitModule(net=None)


@pytest.mark.parametrize("name", list(C.EVAL_CASES))
def test_evaluate_camera_poses_returns_the_reference_dicts(built_lib, golden, name):
    pose_cases = fixture_io.load(os.path.join(ROOT, "tests", "golden", "pose_cases.pt"))["cases"]
    e = golden["eval"][name]
    lit = _lit()
    for resident in ("cuda", "cpu"):
        views, preds = C.eval_scene(name, pose_cases)
        if resident == "cuda":
            preds = [{k: v.cuda() for k, v in p.items()} for p in preds]
            views = [dict(v, camera_pose=v["camera_pose"].cuda()) for v in views]
        res = lit.evaluate_camera_poses(views, preds, niter_PnP=C.EVAL_NITER_PNP, focal_length_estimation_method="first_view_from_global_head")
        ref = e["metrics"]["first_view_from_global_head"]
        print(name, resident, res, ref)
        assert isinstance(preds[0]["conf"], list)  # corrected in place, as in the reference
        assert len(res) == len(ref)
        for a, b in zip(res, ref):
            assert set(a) == set(b)
            for k in b:
                assert bits(a[k]) == bits(b[k]), (name, resident, k, a[k], b[k])
    assert len(lit.camera_pose_metrics_per_epoch) == 2 * len(ref)
    # 'individual': the focal search is not comparable by construction (docs/rows_f.md): keys and range only
    views, preds = C.eval_scene(name, pose_cases)
    res = lit.evaluate_camera_poses(views, [{k: v.cuda() for k, v in p.items()} for p in preds], niter_PnP=C.EVAL_NITER_PNP,
                                    focal_length_estimation_method="individual")
    ref = e["metrics"]["individual"]
    assert len(res) == len(ref)
    for a, b in zip(res, ref):
        assert set(a) == set(b)
        assert all(np.isfinite(v) and 0.0 <= v <= 1.0 for v in a.values())


def test_evaluate_camera_poses_from_the_local_head_on_the_mixed_batch(built_lib, golden):
    """'first_view_from_local_head' aligns first, then corrects the orientation of the local head's outputs too and takes the focal from
    them.  With the local head's outputs set to copies of the global ones the alignment is the identity up to fp32 rounding (poses move
    by far less than the 2e-5 that tests/test_pnp.py allows), so the fixture's 0.05 degree margin makes the reference's
    'first_view_from_global_head' dicts the expected result."""
    views, preds = C.eval_scene("mixed_b2")
    preds = [{k: v.cuda() for k, v in p.items()} for p in preds]
    for p in preds:
        p["pts3d_local"], p["conf_local"] = p["pts3d_in_other_view"].clone(), p["conf"].clone()
    res = _lit().evaluate_camera_poses(views, preds, niter_PnP=C.EVAL_NITER_PNP, focal_length_estimation_method="first_view_from_local_head")
    assert all(isinstance(preds[0][k], list) for k in ("conf", "pts3d_in_other_view", "conf_local", "pts3d_local", "pts3d_local_aligned_to_global"))
    assert tuple(preds[0]["pts3d_local_aligned_to_global"][1].shape) == (C.MIXED_SCENE["W"], C.MIXED_SCENE["H"], 3)
    ref = golden["eval"]["mixed_b2"]["metrics"]["first_view_from_global_head"]
    print(res, ref)
    assert len(res) == len(ref)
    for a, b in zip(res, ref):
        assert {k: bits(v) for k, v in a.items()} == {k: bits(v) for k, v in b.items()}


def test_evaluate_camera_poses_with_one_view_warns_and_returns_nothing(built_lib, caplog):
    views, preds = C.eval_scene("mixed_b2")
    with caplog.at_level("WARNING"):
        assert _lit().evaluate_camera_poses(views[:1], preds[:1]) == []
    assert "Not enough camera poses" in caplog.text
