"""Global alignment, the parts that need no GPU: the fp64 restatement (tests/galign_ref.py) against the reference's own PointCloudOptimizer
(tests/golden/galign_cases.npz, written by tools/make_golden_galign.py) and against finite differences, the torch chain from the raw
parameters to the matrices, the constructor signature, the schedules, parameter freezing, pairs_from_passes, and every refusal of
fast3r_amd/global_align.py and of the C entry point."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import galign_cases as C
import galign_ref as R
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "galign_cases.npz")
NEW_SYMBOLS = {"f3r_galign_workspace_bytes": 2, "f3r_galign_loss_grad": 27}
# the restatement against the reference's fp64 autograd: the largest max|a - b| / max|b| over all stored gradients of all recipes was
# 4.7e-15 (d_log_depth of sym3_l1_m1: a sum of up to 8 products against autograd's order); asserted at ten times that
FP64_ROUNDING = 4.7e-15
# the same through the chain from the raw parameters (quaternion normalisation, expm1, the scale normalisation): 7.3e-15 measured
# (im_depthmaps of mixed4_l1_log)
FP64_CHAIN_ROUNDING = 7.3e-15


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")
def test_golden_generator_reproduces_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_galign.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_golden_holds_data_only_and_its_margins(golden):
    assert os.path.getsize(GOLDEN) < 400 * 1000
    assert all(v.dtype.kind in "bfiuU" for v in golden.values())
    assert json.loads(str(golden["names"])) == list(C.GOLDEN) and bool(golden["conditions_ok"])
    for name, rec in C.GOLDEN.items():
        assert int(golden[f"{name}_seed"]) == rec[4]
        if rec[2] == "l1":
            assert float(golden[f"{name}_residual_share"]) >= float(golden["min_residual_share"]) == 1e-3
        assert float(golden[f"{name}_residual_median"]) > 0.05                 # scene-sized residuals
        for k in C.RAW_NAMES:
            assert np.abs(golden[f"{name}_raw64_{k}"]).max() > 0
        for k in C.MATRIX_NAMES:
            assert np.abs(golden[f"{name}_mat64_{k}"]).max() > 0
    assert {rec[2] for rec in C.GOLDEN.values()} == {"l1", "l2"} and {rec[3] for rec in C.GOLDEN.values()} == {"log", "sqrt", "m1", "id"}


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_restatement_equals_the_reference_fp64_autograd(golden, name):
    c = C.golden_case(name)
    P = R.golden_problem(golden, name, c)
    if c["conf"] in ("log", "m1"):
        assert sum(int((w == 0).sum()) for w in P["w"]) > 0                    # confidences exactly 1: weights exactly 0
    out = R.loss_and_grads(R.tensors(P), c["dist"])
    f = R.flat(out)
    errs = {k: R.rel_err(f[k], golden[f"{name}_mat64_{k}"]) for k in C.MATRIX_NAMES}
    errs["loss"] = abs(float(out["loss"]) - float(golden[f"{name}_mat_loss64"])) / float(golden[f"{name}_mat_loss64"])
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 10 * FP64_ROUNDING, errs
    # the matrix-level and the raw runs of the reference are the same forward
    assert abs(float(golden[f"{name}_mat_loss64"]) - float(golden[f"{name}_loss64"])) <= 1e-6 * float(golden[f"{name}_loss64"])


@pytest.mark.parametrize("dist", ["l1", "l2"])
def test_restatement_gradients_equal_central_differences(dist):
    P = C.matrix_problem([(3, 4), (4, 3), (3, 4)], [(0, 1), (2, 0), (1, 2)], 7)
    T = R.tensors(P)
    f = R.flat(R.loss_and_grads(T, dist))
    h = 1e-6
    rs = np.random.RandomState(0)
    groups = {"d_poses": ("poses", None), "d_focals": ("focals", None), "d_pp": ("pp", None), "d_pw": ("pw", None), "d_adapt": ("adapt", None)}
    for gname, (key, _) in groups.items():
        x = T[key]
        for idx in [tuple(rs.randint(0, s) for s in x.shape) for _ in range(6)]:
            old = float(x[idx])
            x[idx] = old + h
            up = float(R.loss_only(T, dist))
            x[idx] = old - h
            dn = float(R.loss_only(T, dist))
            x[idx] = old
            fd, an = (up - dn) / (2 * h), float(f[gname][idx])
            assert abs(fd - an) <= 1e-6 * max(1.0, float(f[gname].abs().max())), (gname, idx, fd, an)
    off = 0
    for v, (H, W) in enumerate(P["shapes"]):
        x = T["log_depth"][v]
        for idx in [(rs.randint(0, H), rs.randint(0, W)) for _ in range(4)]:
            old = float(x[idx])
            x[idx] = old + h
            up = float(R.loss_only(T, dist))
            x[idx] = old - h
            dn = float(R.loss_only(T, dist))
            x[idx] = old
            an = float(f["d_log_depth"][off + idx[0] * W + idx[1]])
            assert abs((up - dn) / (2 * h) - an) <= 1e-6 * max(1.0, float(f["d_log_depth"].abs().max())), (v, idx)
        off += H * W


def build_optimizer(c, **kw):
    from fast3r_amd import PointCloudOptimizer
    view1, view2, pred1, pred2 = C.optimizer_inputs(c, lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    net = PointCloudOptimizer(view1, view2, pred1, pred2, dist=c["dist"], conf=c["conf"], base_scale=C.BASE_SCALE, pw_break=C.PW_BREAK,
                              focal_break=C.FOCAL_BREAK, **kw)
    with torch.no_grad():
        for name in ("pw_poses", "pw_adaptors", "im_poses", "im_focals", "im_pp"):
            getattr(net, name).data[:] = torch.from_numpy(c[name])
        net.im_depthmaps.data[:] = torch.cat([torch.from_numpy(d).reshape(-1) for d in c["im_depthmaps"]])
    return net


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_torch_chain_with_the_restatement_equals_the_reference_raw_gradients(golden, name):
    c = C.golden_case(name)
    net = build_optimizer(c, allow_pw_adaptors=True, optimize_pp=True).double()
    assert net.edges == c["edges"] and net.imshapes == c["shapes"] and net.im_depthmaps.dtype == torch.float64
    # the matrices of the fp32 chain are the reference's, to fp32 rounding of the chain
    net32 = build_optimizer(c)
    for got, key in ((net32.get_im_poses()[:, :3], "poses"), (net32.get_focals().reshape(-1), "focals"), (net32.get_principal_points(), "pp"),
                     (net32.get_pw_poses()[:, :3], "pw"), (net32.get_adaptors(), "adapt")):
        assert R.rel_err(got.detach(), golden[f"{name}_in_{key}"]) <= 4e-7, key
    meta = (net.imshapes, net.edges, net._pts, net._weight, net.dist)
    loss = R.RefLoss.apply(net.get_im_poses(), net.get_focals(), net.get_principal_points(), net.im_depthmaps, net.get_pw_poses(),
                           net.get_adaptors(), meta)
    loss.backward()
    errs = {k: R.rel_err(getattr(net, k).grad, golden[f"{name}_raw64_{k}"]) for k in C.RAW_NAMES}
    errs["loss"] = abs(float(loss.detach()) - float(golden[f"{name}_loss64"])) / float(golden[f"{name}_loss64"])
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 10 * FP64_CHAIN_ROUNDING, errs


# ------------------------------------------------------------------------------------------------------------------- the interface
def test_constructor_signature_is_the_reference_s(golden):
    """the reference's own signature is stored by the golden tool: `_init_from_views` of the base class and the keyword-only parameters the
    class adds.  Two of its parameters are left out here: `iterationsCount`, which nothing reads, and `verbose`, which only prints."""
    import fast3r_amd
    theirs = [tuple(x) for x in json.loads(str(golden["signature"]))]
    rep = lambda x: re.sub(r" at 0x[0-9a-f]+", "", repr(x))  # noqa: E731
    ours = [(p.name, None if p.default is inspect.Parameter.empty else rep(p.default))
            for p in inspect.signature(fast3r_amd.PointCloudOptimizer).parameters.values()]
    assert [n for n, _ in ours] == ["view1", "view2", "pred1", "pred2", "dist", "conf", "min_conf_thr", "base_scale", "allow_pw_adaptors", "pw_break",
                                    "optimize_pp", "focal_break", "rand_pose"]
    assert sorted(ours) == sorted(x for x in theirs if x[0] not in ("iterationsCount", "verbose"))
    assert [n for n, _ in theirs[:10]] == [n for n, _ in ours[:10]]           # the positional order of the shared parameters
    sig = inspect.signature(fast3r_amd.PointCloudOptimizer.compute_global_alignment)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("init", None), ("niter", 300), ("schedule", "cosine"), ("lr", 0.01),
                                                                                 ("lr_min", 1e-6)]
    assert isinstance(fast3r_amd.MultiViewDUSt3RLitModule.__dict__["global_aligner"], staticmethod)
    assert [m.value for m in fast3r_amd.GlobalAlignerMode] == ["PointCloudOptimizer", "ModularPointCloudOptimizer", "PairViewer"]


def test_schedules_equal_the_reference_s(golden):
    from fast3r_amd import global_align as G
    for t, c, l in zip(golden["schedule_t"], golden["schedule_cosine"], golden["schedule_linear"]):
        assert G.cosine_schedule(float(t), 0.01, 1e-6) == c and G.linear_schedule(float(t), 0.01, 1e-6) == l


def test_parameters_and_freezing():
    c = C.loop_case()
    net = build_optimizer(c)
    trainable = lambda n: sorted(k for k, p in n.named_parameters() if p.requires_grad)  # noqa: E731
    assert trainable(net) == ["im_depthmaps", "im_focals", "im_poses", "pw_poses"]
    assert trainable(build_optimizer(c, allow_pw_adaptors=True, optimize_pp=True)) == sorted(C.RAW_NAMES)
    assert net.pw_poses.shape == (6, 8) and net.pw_adaptors.shape == (6, 2) and net.im_poses.shape == (3, 7) and net.im_focals.shape == (3, 1)
    assert net.im_pp.shape == (3, 2) and net.im_depthmaps.shape == (3 * 48,) and net.total_area_i == net.total_area_j == 6 * 48
    assert net.norm_pw_scale and net.is_symmetrized and net.n_imgs == 3 and net.n_edges == 6 and net.str_edges[1] == "1_0"
    # the getters
    assert torch.allclose(net.get_focals(), (net.im_focals / 20).exp()) and net.get_focals().shape == (3, 1)
    assert torch.equal(net.get_principal_points(), torch.tensor([[4.0, 3.0]] * 3) + 10 * net.im_pp)
    K = net.get_intrinsics()
    assert K.shape == (3, 3, 3) and torch.equal(K[:, 0, 0], net.get_focals()[:, 0]) and torch.equal(K[:, :2, 2], net.get_principal_points())
    ad = build_optimizer(c, allow_pw_adaptors=True).get_adaptors()
    assert ad.shape == (6, 3) and torch.allclose(ad.log().sum(dim=1), torch.zeros(6), atol=1e-6) and torch.equal(ad[:, 0], ad[:, 1])
    pw = net.get_pw_poses()
    scale = torch.linalg.det(pw[:, :3, :3]).abs() ** (1 / 3)
    assert torch.allclose(scale.log().mean(), torch.tensor(np.log(0.5), dtype=torch.float32), atol=1e-5)       # norm_pw_scale: the mean log scale is log base_scale
    assert [d.shape for d in net.get_depthmaps()] == [(6, 8)] * 3 and [p.shape for p in net.get_pts3d()] == [(6, 8, 3)] * 3
    assert all(m.dtype == torch.bool for m in net.get_masks()) and torch.equal(net.get_conf()[0], net.im_conf[0].log())
    want = torch.maximum(torch.from_numpy(c["conf_i"][0]), torch.from_numpy(c["conf_i"][2]))                      # view 0: edges (0, 1), (1, 0), (0, 2), (2, 0)
    want = torch.maximum(torch.maximum(want, torch.from_numpy(c["conf_j"][1])), torch.from_numpy(c["conf_j"][3]))
    assert torch.equal(net.im_conf[0], want)
    # _set_* write through, and only while the parameter is free
    pose = torch.eye(4)
    pose[:3, :3] = torch.from_numpy(C.quat_to_rotmat([0.1, -0.2, 0.05, 1.0])).float()
    pose[:3, 3] = torch.tensor([0.3, -1.5, 2.0])
    net._set_pose(net.im_poses, 1, pose)
    assert torch.allclose(net.get_im_poses()[1], pose, atol=1e-6)
    net._set_focal(2, 11.5)
    assert abs(float(net.get_focals()[2].detach()) - 11.5) < 1e-5
    net._set_depthmap(0, torch.full((6, 8), 2.5))
    assert torch.allclose(net.get_depthmaps()[0], torch.full((6, 8), 2.5))
    net.preset_pose([pose] * 3)
    assert not net.im_poses.requires_grad and not net.norm_pw_scale and torch.allclose(net.get_im_poses()[0], pose, atol=1e-6)
    assert float(net.get_pw_norm_scale_factor()) == 1
    net.preset_focal([7.0, 8.0, 9.0])
    assert not net.im_focals.requires_grad and torch.allclose(net.get_focals()[:, 0], torch.tensor([7.0, 8.0, 9.0])) and bool(net.get_known_focal_mask().all())
    net2 = build_optimizer(c, optimize_pp=True)
    net2.preset_principal_point([(4.5, 2.5)] * 3)
    assert not net2.im_pp.requires_grad and torch.allclose(net2.get_principal_points(), torch.tensor([[4.5, 2.5]] * 3))
    assert trainable(net) == ["im_depthmaps", "pw_poses"]
    before = net.im_poses.detach().clone()
    net._set_pose(net.im_poses, 0, torch.eye(4))                               # frozen: no modification
    assert torch.equal(net.im_poses.detach(), before)
    with pytest.raises(ValueError, match="incomplete mask"):
        build_optimizer(c).preset_focal([1.0], msk=[0])


def test_quaternion_round_trip():
    from fast3r_amd import global_align as G
    rs = np.random.RandomState(3)
    q = torch.from_numpy(rs.normal(size=(64, 4)))
    q = q / q.norm(dim=-1, keepdim=True)
    Rm = G.unitquat_to_rotmat(q)
    assert torch.allclose(Rm @ Rm.transpose(1, 2), torch.eye(3, dtype=torch.float64).expand(64, 3, 3), atol=1e-12)
    assert torch.allclose(torch.linalg.det(Rm), torch.ones(64, dtype=torch.float64))
    back = G.rotmat_to_unitquat(Rm)
    assert torch.allclose(back, torch.where(q[:, 3:] < 0, -q, q), atol=1e-12)
    for k in range(4):
        assert np.allclose(Rm[k].numpy(), C.quat_to_rotmat(q[k].numpy()), atol=1e-12)
    x = torch.tensor([-3.0, -0.5, 0.0, 0.2, 4.0])
    assert torch.allclose(G.signed_expm1(G.signed_log1p(x)), x, atol=1e-6)


def synthetic_pass(order, H=4, W=5, B=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"preds": [{"pts3d_in_other_view": torch.rand(B, H, W, 3, generator=g) + v, "conf": 1 + torch.rand(B, H, W, generator=g),
                       "pts3d_local": torch.rand(B, H, W, 3, generator=g) + 1, "conf_local": 1 + torch.rand(B, H, W, generator=g)} for v in order],
            "views": [{} for _ in order]}


def test_pairs_from_passes():
    import fast3r_amd
    out0, out2 = synthetic_pass([0, 1, 2, 3]), synthetic_pass([2, 0, 1, 3], seed=1)
    view1, view2, pred1, pred2 = fast3r_amd.pairs_from_passes([out0, out2], [0, 2])
    assert view1["idx"] == [0, 0, 0, 2, 2, 2] and view2["idx"] == [1, 2, 3, 0, 1, 3]
    # orientation: pred1 is the anchor's map, pred2 view v's, both of the pass that the edge comes from
    assert torch.equal(pred1["pts3d"][0], out0["preds"][0]["pts3d_in_other_view"][0]) and torch.equal(pred1["pts3d"][3], out2["preds"][0]["pts3d_in_other_view"][0])
    assert torch.equal(pred2["pts3d_in_other_view"][1], out0["preds"][2]["pts3d_in_other_view"][0])
    assert torch.equal(pred2["pts3d_in_other_view"][3], out2["preds"][1]["pts3d_in_other_view"][0])          # view 0 is position 1 of pass 1
    assert torch.equal(pred2["conf"][4], out2["preds"][2]["conf"][0]) and torch.equal(pred1["conf"][5], out2["preds"][0]["conf"][0])
    # shared storage: one object per anchor, and no copy of the passes' own memory
    assert pred1["pts3d"][0] is pred1["pts3d"][1] is pred1["pts3d"][2] and pred1["pts3d"][3] is pred1["pts3d"][5] and pred1["conf"][0] is pred1["conf"][2]
    assert pred1["pts3d"][0].data_ptr() == out0["preds"][0]["pts3d_in_other_view"].data_ptr()
    assert pred2["pts3d_in_other_view"][5].data_ptr() == out2["preds"][3]["pts3d_in_other_view"].data_ptr()
    # an explicit order, and preds lists in place of output dicts
    v1, v2, _, p2 = fast3r_amd.pairs_from_passes([out2["preds"]], [[2, 3, 1, 0]])
    assert v1["idx"] == [2, 2, 2] and v2["idx"] == [3, 1, 0] and torch.equal(p2["pts3d_in_other_view"][0], out2["preds"][1]["pts3d_in_other_view"][0])
    # the optimizer keeps one tensor per distinct map
    net = fast3r_amd.PointCloudOptimizer(view1, view2, pred1, pred2)
    assert net.edges == [(0, 1), (0, 2), (0, 3), (2, 0), (2, 1), (2, 3)] and not net.is_symmetrized
    assert net._pts[0] is net._pts[2] is net._pts[4] and net._weight[0] is net._weight[4] and net._pts[6] is net._pts[10]
    assert len({id(t) for t in net._pts}) == 8 and net._passes["edge_pass"] == [0, 0, 0, 1, 1, 1]
    for bad, anchors, word in (([out0], [0, 1], "equal lengths"), ([], [], "one pass"), ([out0, synthetic_pass([0, 1, 2])], [0, 1], "pass 1 has 3 views"),
                               ([out0], [4], "permutation"), ([out0], [[0, 1, 1, 3]], "permutation"), ([synthetic_pass([0])], [0], "two at least")):
        with pytest.raises(ValueError, match=word):
            fast3r_amd.pairs_from_passes(bad, anchors)
    with pytest.raises(KeyError, match="conf"):
        fast3r_amd.pairs_from_passes([[{"pts3d_in_other_view": torch.zeros(1, 2, 2, 3)}] * 2], [0])


def test_refusals_before_any_device_work():
    import fast3r_amd
    from fast3r_amd import GlobalAlignerMode, global_align as G
    c = C.loop_case()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    args = lambda: C.optimizer_inputs(c, t)  # noqa: E731
    make = fast3r_amd.PointCloudOptimizer
    with pytest.raises(ValueError, match="dist"):
        make(*args(), dist="l3")
    with pytest.raises(ValueError, match="conf"):
        make(*args(), conf="exp")
    v1, v2, p1, p2 = args()
    with pytest.raises(ValueError, match="equal lengths"):
        make({"idx": v1["idx"][:-1]}, v2, p1, p2)
    with pytest.raises(ValueError, match="one edge"):
        make({"idx": []}, {"idx": []}, p1, p2)
    with pytest.raises(ValueError, match="missing values"):                    # view indices with gaps
        make({"idx": [0, 3]}, {"idx": [3, 0]}, {k: v[:2] for k, v in p1.items()}, {k: v[:2] for k, v in p2.items()})
    with pytest.raises(ValueError, match="itself"):
        make({"idx": [0, 1]}, {"idx": [1, 1]}, {k: v[:2] for k, v in p1.items()}, {k: v[:2] for k, v in p2.items()})
    with pytest.raises(ValueError, match=r"pred1\['pts3d'\] has 5 entries"):
        make(v1, v2, dict(p1, pts3d=p1["pts3d"][:5]), p2)
    with pytest.raises(ValueError, match=r"pred2\['conf'\] has 7 entries"):
        make(v1, v2, p1, dict(p2, conf=p2["conf"] + p2["conf"][:1]))
    with pytest.raises(ValueError, match="incorrect shape for image"):
        make(v1, v2, dict(p1, pts3d=[torch.zeros(5, 8, 3)] + p1["pts3d"][1:], conf=[torch.ones(5, 8)] + p1["conf"][1:]), p2)
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        make(v1, v2, dict(p1, conf=[torch.ones(6, 7)] + p1["conf"][1:]), p2)
    net = make(*args())
    for kw, word in (({"schedule": "step"}, "schedule"), ({"niter": -1}, "niter"), ({"init": "random"}, "init")):
        with pytest.raises(ValueError, match=word):
            net.compute_global_alignment(**kw)
    for init in ("mst", "known_poses"):
        with pytest.raises(NotImplementedError, match="fast_pnp"):
            net.compute_global_alignment(init=init)
    with pytest.raises(ValueError, match="pairs_from_passes"):
        net.compute_global_alignment(init="passes")
    out = dict(zip(("view1", "view2", "pred1", "pred2"), args()))
    for mode in (GlobalAlignerMode.ModularPointCloudOptimizer, GlobalAlignerMode.PairViewer):
        with pytest.raises(NotImplementedError, match=mode.value):
            fast3r_amd.global_aligner(out, "cpu", mode=mode)
    assert isinstance(fast3r_amd.global_aligner(out, "cpu"), make)
    # the loss: shapes and observations are checked first, and a CPU problem has no fallback
    shapes, edges = [(2, 3), (3, 2)], [(0, 1)]
    maps = lambda: ([torch.zeros(2, 3, 3), torch.zeros(3, 2, 3)], [torch.ones(2, 3), torch.ones(3, 2)])  # noqa: E731
    for change, word in ((lambda p, w: (shapes, [(0, 2)], p, w), "outside the 2 views"), (lambda p, w: (shapes, [(1, 1)], p, w), "itself"),
                         (lambda p, w: (shapes, edges, p[:1], w), "2 pointmaps"), (lambda p, w: (shapes, edges, [p[1], p[0]], w), "against view 0"),
                         (lambda p, w: (shapes, edges, p, [w[0], torch.ones(2, 3)]), "against view 1"), (lambda p, w: (shapes, edges, [None, p[1]], w), "no pointmap"),
                         (lambda p, w: (shapes, edges, [p[0].double(), p[1]], w), "contiguous fp32"), (lambda p, w: (shapes[:1], edges, p, w), "two views"),
                         (lambda p, w: (shapes, [], [], []), "one edge")):
        with pytest.raises(ValueError, match=word):
            G.Observations(*change(*maps()))
    from fast3r_amd import _lib
    with pytest.raises(_lib.F3RError):
        G.Observations(shapes, edges, *maps())
    with pytest.raises(ValueError, match="dist"):
        fast3r_amd.alignment_loss(None, None, None, None, None, None, None, dist="huber")
    with pytest.raises(ValueError, match="Observations"):
        fast3r_amd.alignment_loss(None, None, None, None, None, None, object())


# ------------------------------------------------------------------------------------------------------------------- the library
def test_library_side(built_lib):
    from fast3r_amd import _lib, post_ops
    for name, arity in NEW_SYMBOLS.items():
        assert len(_lib.SYMBOLS[name][1]) == arity and _lib.symbol_since(name) == 0 and _lib.if_present(name)
        assert name in _lib.SYMBOL_IF_PRESENT_GALIGN and name not in _lib.SYMBOL_IF_PRESENT_CLEAN and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_IF_PRESENT_GALIGN) == set(NEW_SYMBOLS)
    assert built_lib.f3r_version() == 430                                     # unchanged
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_galign ] && extra="-ffp-contract=off"' in build and "obj/f3r_galign.o" in build
    size = built_lib.f3r_galign_workspace_bytes
    assert size(1, 1) == 0 and size(2, 0) == 0 and size(65536, 1) == 0 and size(-1, 5) == 0
    assert size(2, 1) == 2 * (2 * 64 * 16 * 8) + 256                           # 64 rows of 16 doubles per view and per observation, whatever the image size
    assert size(100, 600) == 100 * 64 * 16 * 8 + 1200 * 64 * 16 * 8 + 1024
    assert post_ops.galign_dist_id("l1") == 0 and post_ops.galign_dist_id("l2") == 1
    tb = post_ops.galign_tables([(2, 3), (3, 2), (2, 3)], [(0, 1), (2, 0)], [(0x1000, 0x2000, 2, 3), (0x3000, 0x4000, 3, 2), (0x5000, 0x6000, 2, 3),
                                                                            (0x1000, 0x2000, 2, 3)])
    assert tb["view_table_host"][0].tolist() == [2, 3, 0, 3, 2, 6, 2, 3, 12, 0, 2, 3, 4] and tb["obs_list_host"][0].tolist() == [0, 3, 1, 2]
    assert tb["edges_host"][0].tolist() == [0, 1, 2, 0] and tb["total"] == 18 and tb["obs_table_host"][0].tolist()[:4] == [0x1000, 0x2000, 2, 3]


def test_entry_point_refuses_before_any_launch(built_lib):
    """every refusal of f3r_galign_loss_grad with pointers that are never dereferenced: the host tables decide"""
    from fast3r_amd import post_ops
    err = lambda: built_lib.f3r_last_error_string()  # noqa: E731
    shapes, edges = [(2, 3), (3, 2), (2, 3)], [(0, 1), (2, 0)]
    maps = [(0x1000, 0x2000, 2, 3), (0x3000, 0x4000, 3, 2), (0x5000, 0x6000, 2, 3), (0x1000, 0x2000, 2, 3)]

    def call(shapes=shapes, edges=edges, maps=maps, dist=0, ws=1 << 22, ptrs=0x1000, ws_ptr=0x1000, vt=None, ol=None, N=None, E=None):
        tb = post_ops.galign_tables(shapes, edges, maps)
        vt_a = tb["view_table_host"][0] if vt is None else np.asarray(vt, dtype=np.int64)
        ol_a = tb["obs_list_host"][0] if ol is None else np.asarray(ol, dtype=np.int32)
        p64, p32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
        return built_lib.f3r_galign_loss_grad(ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, vt_a.ctypes.data_as(p64), len(shapes) if N is None else N, ptrs,
                                              tb["edges_host"][1], len(edges) if E is None else E, ptrs, tb["obs_table_host"][1], ptrs,
                                              ol_a.ctypes.data_as(p32), dist, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, ws_ptr, ws, None)
    assert call(N=1) == -1 and b"n_views = 1" in err()
    assert call(E=0) == -1 and b"n_edges = 0" in err()
    assert call(ptrs=None) == -1 and b"null pointer" in err()
    assert call(dist=2) == -1 and b"dist = 2" in err()
    assert call(shapes=[(0, 3), (3, 2), (2, 3)]) == -1 and b"view 0 is 0 x 3" in err()
    assert call(shapes=[(1 << 16, 1 << 15), (3, 2), (2, 3)]) == -1 and b"2^31 - 1" in err()
    assert call(vt=[2, 3, 0, 3, 2, 5, 2, 3, 12, 0, 2, 3, 4]) == -1 and b"running sum" in err()
    assert call(edges=[(0, 3), (2, 0)]) == -1 and b"edge 0 = (0, 3) lies outside the 3 views" in err()
    assert call(edges=[(0, 1), (-1, 0)]) == -1 and b"edge 1 = (-1, 0)" in err()
    assert call(edges=[(0, 1), (2, 2)]) == -1 and b"edge 1 joins view 2 with itself" in err()
    assert call(maps=[maps[0], (0, 0x4000, 3, 2)] + maps[2:]) == -1 and b"null pointmap or weight map of edge 0, side 1" in err()
    assert call(maps=maps[:3] + [(0x1000, 0, 2, 3)]) == -1 and b"null pointmap or weight map of edge 1, side 1" in err()
    assert call(maps=[(0x1002, 0x2000, 2, 3)] + maps[1:]) == -1 and b"misaligned pointmap" in err()
    assert call(maps=[(0x1000, 0x2000, 3, 2)] + maps[1:]) == -1 and b"edge 0, side 0 is 3 x 2, its view 0 is 2 x 3" in err()
    assert call(vt=[2, 3, 0, 3, 2, 6, 2, 3, 12, 1, 2, 3, 4]) == -1 and b"start at 0" in err()
    assert call(vt=[2, 3, 0, 3, 2, 6, 2, 3, 12, 0, 2, 3, 5]) == -1 and b"end at 2 n_edges" in err()
    assert call(vt=[2, 3, 0, 3, 2, 6, 2, 3, 12, 0, 2, 1, 4]) == -1 and b"observation list of view 1" in err()
    assert call(ol=[0, 1, 3, 2]) == -1 and b"observation 1 in the list of view 0 is not one of its own" in err()
    assert call(ol=[3, 0, 1, 2]) == -1 and b"must ascend" in err()
    assert call(ol=[0, 0, 1, 2]) == -1 and b"must ascend" in err()             # an observation twice
    assert call(ol=[0, 7, 1, 2]) == -1 and b"observation 7" in err()
    assert call(ws=255) == -1 and b"workspace" in err()
    assert call(ws_ptr=0x1010) == -1 and b"workspace" in err()
    assert call(ptrs=0x1002) == -1 and b"misaligned" in err()
