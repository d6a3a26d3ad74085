"""The validation loss on the GPU (f3r_loss.hip through fast3r_amd.losses): every golden case against the reference's own fp32 run and the
float64 restatement, a size case checked by the same restatement on the device, determinism, untouched inputs, and validation_step
end to end.

Bounds.  The kernels and tests/loss_ref.py both work in fp64 on the same widened inputs, so they differ by fp64 rounding only (another
4 x 4 inverse, another order of the sums).  Measured on an MI355X over every output of every golden case and of the size case, as
|got - ref64| / max(|ref64|, 1e-2): worst REL_F64_MEASURED (docs/rows_f.md); the tests assert 10 x that.  `loss` is returned as an
fp32 tensor, so it alone gets half an fp32 ulp (2^-24 relative) on top.  Against the reference's fp32 run the allowance is 2 d plus the
same bound, d being the case's recorded |fp32 reference - fp64 restatement|.
"""
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cam_pose_cases as PC  # noqa: E402
import loss_cases as C  # noqa: E402
import loss_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "loss_cases.pt")
REL_F64_MEASURED = 5.3e-15  # worst figure of the measurement run (the size case under V3 + log1p + dist_clip; golden cases: 3.3e-15)
REL_F64 = 10 * REL_F64_MEASURED
FP32_HALF_ULP = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def criterion(recipe, alpha=C.ALPHA):
    from fast3r_amd import losses as L
    cls = L.Regr3DMultiviewV4 if recipe["version"] == 4 else L.Regr3DMultiviewV3
    return L.ConfLossMultiviewV2(cls(L.L21, **C.criterion_kwargs(recipe)), alpha=alpha)


def run_case(name, device="cuda"):
    recipe = C.CASES[name]
    views, preds = C.to_device(*C.build(name), device)
    loss, details = criterion(recipe)(views, preds, **C.call_kwargs(recipe))
    return views, preds, loss, details


def scale(x):
    return max(abs(x), 1e-2)


def check_outputs(got, ref64, ref32=None, d=None, what=""):
    """NaN exactly where the reference has it; the bounds of the module docstring.  Prints the worst figure before asserting."""
    assert list(got) == list(ref64), what
    worst = 0.0
    failures = []
    for k, want in ref64.items():
        extra = FP32_HALF_ULP * abs(want) if k == "loss" and not math.isnan(want) else 0.0
        if math.isnan(want):
            if not math.isnan(got[k]):
                failures.append(f"{what} {k}: {got[k]} where the reference has NaN")
            continue
        if math.isnan(got[k]):
            failures.append(f"{what} {k}: NaN where the reference has {want}")
            continue
        if math.isinf(want) or math.isinf(got[k]):  # equal infinities pass, anything else fails (max(0.0, nan) below would let them through)
            if got[k] != want:
                failures.append(f"{what} {k}: {got[k]!r} vs fp64 {want!r}")
            continue
        err = max(0.0, abs(got[k] - want) - extra)
        worst = max(worst, err / scale(want))
        if err > REL_F64 * scale(want):
            failures.append(f"{what} {k}: {got[k]!r} vs fp64 {want!r}: {err / scale(want):.3e} relative")
        if ref32 is not None and abs(got[k] - ref32[k]) > 2 * d[k] + REL_F64 * scale(want) + extra:
            failures.append(f"{what} {k}: {got[k]!r} vs the reference's fp32 {ref32[k]!r}: off by {abs(got[k] - ref32[k]):.3e}, d = {d[k]:.3e}")
    print(f"LOSS-MEASURE {what}: worst |got - ref64| / max(|ref64|, 1e-2) = {worst:.3e}")
    assert not failures, "\n".join(failures)
    return worst


@pytest.mark.parametrize("name", list(C.CASES))
def test_golden_case_matches_both_reference_runs(built_lib, golden, name):
    case = golden[name]
    views, preds, loss, details = run_case(name)
    for k, v in C.checksums(*C.to_device(views, preds, "cpu")).items():
        assert v == pytest.approx(case["checksums"][k], rel=1e-12, abs=1e-12), f"input {k} does not rebuild"
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.is_cuda and not loss.requires_grad
    assert all(type(v) is float for v in details.values())
    got = {"loss": float(loss), **details}
    ref64 = {"loss": case["ref64"]["loss"], **case["ref64"]["details"]}
    ref32 = {"loss": case["ref32"]["loss"], **case["ref32"]["details"]}
    check_outputs(got, ref64, ref32, case["d"], name)
    if "empty_view" in C.CASES[name]:
        v = C.CASES[name]["empty_view"]
        for kind in ("global", "local"):
            term = details[f"ConfLossMultiviewV2_conf_loss_{kind}/{v:02d}"]
            assert term == 0.0 and math.copysign(1.0, term) == 1.0  # the reference's literal 0
            assert math.isnan(details[f"Regr3DMultiviewV3_pts3d_loss_{kind}/{v:02d}"])


def device_scene(n_views, H, W, seed):
    """inputs generated on the device: pinhole-like depth maps seen from moving cameras, holes in the masks, local heads present"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device="cuda")  # noqa: E731
    views, preds = [], []
    for v in range(n_views):
        z = 1.0 + 3.0 * rnd(1, H, W)
        cam = torch.cat([(rnd(1, H, W, 2) - 0.5) * 1.2 * z[..., None], z[..., None]], dim=-1)
        a = 0.3 * (rnd(1) - 0.5) * v
        c, s = torch.cos(a), torch.sin(a)
        P = torch.eye(4, device="cuda")[None].clone()
        P[0, 0, 0], P[0, 0, 2], P[0, 2, 0], P[0, 2, 2] = c[0], s[0], -s[0], c[0]
        P[0, :3, 3] = (rnd(3) - 0.5) * (2.0 if v else 0.0)
        world = cam @ P[0, :3, :3].T + P[0, :3, 3]
        views.append({"pts3d": world, "valid_mask": rnd(1, H, W) >= 0.15, "camera_pose": P})
        preds.append({"pts3d_in_other_view": 1.4 * world + 0.05 * (rnd(1, H, W, 3) - 0.5), "conf": 1.0 + 4.0 * rnd(1, H, W) ** 2,
                      "pts3d_local": 0.7 * cam + 0.05 * (rnd(1, H, W, 3) - 0.5), "conf_local": 1.0 + 4.0 * rnd(1, H, W) ** 2})
    return views, preds


def raw_bytes(t):
    return t.contiguous().view(-1).view(torch.uint8).clone()


def test_size_case_against_the_restatement_on_the_device(built_lib):
    """N = 100 views of 384 x 512 with local heads (19.7 M pixels per set), V4 and V3 + log1p + dist_clip: the same float64 restatement,
    evaluated view by view on the GPU; the inputs are left as they were"""
    views, preds = device_scene(100, 384, 512, seed=5)
    before = [raw_bytes(t) for d in views + preds for t in d.values()]
    for recipe, kw in ((dict(version=4), {}), (dict(version=3, norm_mode="avg_log1p"), {"dist_clip": 4.0})):
        loss, details = criterion(recipe)(views, preds, **kw)
        want_loss, want = loss_ref.multiview_conf_loss(views, preds, version=recipe["version"], alpha=C.ALPHA, **C.criterion_kwargs(recipe), **kw)
        assert all(math.isfinite(v) for v in want.values()) and len(want) == 400
        check_outputs({"loss": float(loss), **details}, {"loss": want_loss, **want}, what=f"size case V{recipe['version']}")
    after = [raw_bytes(t) for d in views + preds for t in d.values()]
    assert all(torch.equal(a, b) for a, b in zip(before, after))


@pytest.mark.parametrize("name", ["released_local", "odd_shape", "nan_pred_v4", "large"])
def test_two_runs_give_the_same_bits_and_leave_the_inputs_alone(built_lib, name):
    recipe = C.CASES[name]
    views, preds = C.to_device(*C.build(name), "cuda")
    before = [raw_bytes(t) for d in views + preds for t in d.values()]
    crit = criterion(recipe)
    runs = []
    for run in range(2):
        if run:  # the second run gets a workspace full of NaN: whatever the kernels read there they must have written themselves
            junk = torch.full((built_lib.f3r_mv_conf_loss_workspace_bytes(len(views), recipe["B"]) // 8,), float("nan"), dtype=torch.float64, device="cuda")
            del junk  # back to the caching allocator, which hands the block to the next request of that size
        loss, details = crit(views, preds, **C.call_kwargs(recipe))
        runs.append(torch.tensor([float(loss)] + list(details.values()), dtype=torch.float64))
    assert torch.equal(raw_bytes(runs[0]), raw_bytes(runs[1]))
    after = [raw_bytes(t) for d in views + preds for t in d.values()]
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_host_views_uint8_masks_strided_inputs_and_scaling(built_lib):
    name = "released_local"
    recipe = C.CASES[name]
    views, preds, loss, details = run_case(name)
    crit = criterion(recipe)
    # views on the host are moved to the device
    cpu_views = [{k: t.cpu() for k, t in v.items()} for v in views]
    loss2, details2 = crit(cpu_views, preds)
    assert float(loss2) == float(loss) and details2 == details
    # uint8 masks, and non-contiguous predictions (made contiguous by the wrapper)
    u8_views = [dict(v, valid_mask=v["valid_mask"].to(torch.uint8)) for v in views]
    strided = [{k: (t.transpose(1, 2).contiguous().transpose(1, 2) if t.dim() >= 3 else t) for k, t in p.items()} for p in preds]
    assert not strided[0]["conf"].is_contiguous()
    loss3, details3 = crit(u8_views, strided)
    assert float(loss3) == float(loss) and details3 == details
    # k * loss
    loss4, details4 = (2 * crit)(views, preds)
    assert float(loss4) == 2 * float(loss) and details4 == details
    # without the local head's outputs only the global terms exist
    loss5, details5 = crit(views, [{k: p[k] for k in ("pts3d_in_other_view", "conf")} for p in preds])
    assert list(details5) == [k for k in details if "_global/" in k] and all(details5[k] == details[k] for k in details5)
    V = len(views)
    assert float(loss5) == pytest.approx(sum(details[f"ConfLossMultiviewV2_conf_loss_global/{v:02d}"] for v in range(V)) / V, rel=1e-6)


# ------------------------------------------------------------------------------------------------ validation_step end to end
class SyntheticNet(torch.nn.Module):
    """A tiny stand-in for the model: predicts the ground truth in view 0's frame (global head) and in the view's own frame (local head),
    scaled by learnable factors, so the pose and reconstruction evaluations downstream see a consistent scene."""

    def __init__(self):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.tensor([1.3, 0.8]))

    def forward(self, views):
        with torch.no_grad():
            inv = [torch.linalg.inv(v["camera_pose"].float().cpu()).to(v["pts3d"].device) for v in views]
            preds = []
            for v, view in enumerate(views):
                x = view["pts3d"]
                glob = torch.einsum("bij,bhwj->bhwi", inv[0][:, :3, :3], x) + inv[0][:, None, None, :3, 3]
                loc = torch.einsum("bij,bhwj->bhwi", inv[v][:, :3, :3], x) + inv[v][:, None, None, :3, 3]
                conf = 1.0 + loc[..., 2].abs()
                preds.append({"pts3d_in_other_view": (self.scale[0] * glob).contiguous(), "conf": conf.contiguous(),
                              "pts3d_local": (self.scale[1] * loc).contiguous(), "conf_local": (conf + 0.5).contiguous()})
        return preds


def e2e_batch(dataset, n_views=3, H=48, W=64):
    g = torch.Generator().manual_seed(21)
    batch = []
    for v in range(n_views):
        Xw, _, T = PC.make_view(g, H, W, 60.0, 0.0, 0, anchor=(v == 0))
        batch.append({"img": torch.zeros(1, 3, H, W), "pts3d": Xw[None].contiguous(), "valid_mask": torch.ones(1, H, W, dtype=torch.bool),
                      "camera_pose": T.float()[None], "true_shape": torch.tensor([[H, W]]), "dataset": [dataset],
                      "label": [f"scene_{dataset}/seq"], "instance": [str(v)]})
    return batch


@pytest.mark.parametrize("dataset", ["Co3d_v2", "dtu"])
def test_validation_step_end_to_end(built_lib, dataset):
    from fast3r_amd import MultiViewDUSt3RLitModule
    from fast3r_amd import losses as L
    crit = L.ConfLossMultiviewV2(L.Regr3DMultiviewV4(L.L21, norm_mode="avg_dis"), alpha=0.2)
    lit = MultiViewDUSt3RLitModule(net=SyntheticNet().cuda(), validation_criterion=crit)
    assert lit.device.type == "cuda"
    views, preds, loss, details = lit.model_step(e2e_batch(dataset), crit)
    assert all(views[0][k].is_cuda for k in ("img", "pts3d", "valid_mask", "camera_pose")) and loss.is_cuda
    value = lit.validation_step(e2e_batch(dataset), 0)
    print(f"LOSS-MEASURE validation_step {dataset}: loss {value!r}")
    assert type(value) is float and math.isfinite(value) and value == float(loss)
    assert lit.val_losses == [value]
    store = lit.val_loss_details_per_epoch[dataset]
    assert store[f"val_detail_{dataset}_Regr3DMultiviewV3_pts3d_loss_local/02"] == [details["Regr3DMultiviewV3_pts3d_loss_local/02"]]
    assert len(store[f"val/{dataset}_ConfLossMultiviewV2_conf_loss_global"]) == 3
    # the prediction is the ground truth up to one scale per head, which the normalisation removes: L is rounding noise
    assert all(abs(v) < 1e-5 for k, v in details.items() if "pts3d_loss" in k)
    if dataset == "Co3d_v2":
        assert len(lit.camera_pose_metrics_per_epoch) == 1 and lit.reconstruction_metrics_per_epoch == {}
        m = lit.camera_pose_metrics_per_epoch[0]
        assert set(m) == {"RRA_at_5", "RRA_at_15", "RRA_at_30", "RTA_at_5", "RTA_at_15", "RTA_at_30", "mAA_30"}
        assert all(math.isfinite(float(x)) for x in m.values())
    else:
        assert lit.camera_pose_metrics_per_epoch == [] and list(lit.reconstruction_metrics_per_epoch) == ["dtu"]
        scenes = lit.reconstruction_metrics_per_epoch["dtu"]
        metrics = scenes["scene_dtu"]
        assert math.isfinite(float(metrics["accuracy"])) and math.isfinite(float(metrics["completion"]))
        lit.current_epoch = 2  # not an evaluation epoch: the loss is still computed, the metrics are not
        lit.reconstruction_metrics_per_epoch = {}
        assert lit.validation_step(e2e_batch(dataset), 1) == value and lit.reconstruction_metrics_per_epoch == {}
    out = lit.on_validation_epoch_end()
    assert out["val/loss"] == pytest.approx(value) and lit.val_losses == []
