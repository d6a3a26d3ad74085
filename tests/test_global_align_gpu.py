"""Global alignment on a real MI355X.  The bar of every comparison: for an output tensor T, err(T) = max|got - ref64| / max|ref64| must not
exceed max(4 d(T), 2^-20), where d(T) is the same quantity for the fp32 run of the reference (golden cases) or of the restatement
tests/galign_ref.py (geometry cases), and 2^-20 is 16 fp32 ulps of the largest entry.  Measured on an MI355X over the golden cases: the
largest err of a matrix-level output was 9.8e-8 (dL/dl of two_l1_log: the fp32 rounding of the stored result; d between 6e-8 and 2.8e-6), of
a raw-parameter gradient 3.9e-6 against d = 3.6e-6 (im_focals of star5_l2_log: the fp32 rounding of the matrices the kernel is given);
docs/rows_f.md has the table."""
import os

import numpy as np
import pytest
import torch

import galign_cases as C
import galign_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
FLOOR = 2.0 ** -20
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "galign_cases.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def upload(P):
    """the numpy problem on the device; arrays that are one object become one tensor, so that shared maps stay shared"""
    seen = {}

    def one(a):
        if id(a) not in seen:
            seen[id(a)] = gpu(a)
        return seen[id(a)]
    from fast3r_amd import Observations
    pts, w = [one(p) for p in P["pts"]], [one(x) for x in P["w"]]
    obs = Observations(P["shapes"], P["edges"], pts, w)
    args = [gpu(P["poses"]), gpu(P["focals"]), gpu(P["pp"]), torch.cat([gpu(d).reshape(-1) for d in P["log_depth"]]), gpu(P["pw"]), gpu(P["adapt"])]
    return args, obs, pts, w


def run(P, dist):
    from fast3r_amd import post_ops
    args, obs, pts, w = upload(P)
    out = post_ops.galign_loss_grad(*args, obs.tables, dist)
    assert out[0].dtype == torch.float64 and out[0].dim() == 0 and all(o.is_cuda for o in out)
    assert all(o.dtype == torch.float32 and o.shape == a.shape for o, a in zip(out[1:], [args[3], args[0], args[1], args[2], args[4], args[5]]))
    return dict(zip(("loss",) + C.MATRIX_NAMES, [o.cpu() for o in out]))


def compare(got, ref64, ref32, names, what):
    """the bar of the module docstring on every tensor; prints err and d before it asserts"""
    rows = {}
    for k in names:
        rows[k] = (R.rel_err(got[k], ref64[k]), R.rel_err(ref32[k], ref64[k]))
    print(what, {k: f"err {e:.1e} d {d:.1e}" for k, (e, d) in rows.items()})
    for k, (e, d) in rows.items():
        assert e <= max(4 * d, FLOOR), (what, k, e, d)
    return rows


def against_restatement(P, dist, what):
    got = run(P, dist)
    o64, o32 = R.loss_and_grads(R.tensors(P), dist), R.loss_and_grads(R.tensors(P, torch.float32), dist)
    r64, r32 = dict(R.flat(o64), loss=o64["loss"]), dict(R.flat(o32), loss=o32["loss"])
    compare(got, r64, r32, ("loss",) + C.MATRIX_NAMES, what)
    return got, r64


def build_optimizer(c, **kw):
    from fast3r_amd import PointCloudOptimizer
    view1, view2, pred1, pred2 = C.optimizer_inputs(c, lambda a: torch.from_numpy(np.ascontiguousarray(a)))
    net = PointCloudOptimizer(view1, view2, pred1, pred2, dist=c["dist"], conf=c["conf"], base_scale=C.BASE_SCALE, pw_break=C.PW_BREAK,
                              focal_break=C.FOCAL_BREAK, **kw)
    with torch.no_grad():
        for name in ("pw_poses", "pw_adaptors", "im_poses", "im_focals", "im_pp"):
            getattr(net, name).data[:] = torch.from_numpy(c[name])
        net.im_depthmaps.data[:] = torch.cat([torch.from_numpy(d).reshape(-1) for d in c["im_depthmaps"]])
    return net.to(DEV)


# ------------------------------------------------------------------------------------------------------------------- accuracy on the golden cases
@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_golden_matrix_level_outputs(built_lib, golden, name):
    c = C.golden_case(name)
    got = run(R.golden_problem(golden, name, c), c["dist"])
    ref64 = dict({k: golden[f"{name}_mat64_{k}"] for k in C.MATRIX_NAMES}, loss=golden[f"{name}_mat_loss64"])
    ref32 = dict({k: golden[f"{name}_mat32_{k}"] for k in C.MATRIX_NAMES}, loss=golden[f"{name}_mat_loss32"])
    compare(got, ref64, ref32, ("loss",) + C.MATRIX_NAMES, name)


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_golden_raw_parameter_gradients(built_lib, golden, name):
    c = C.golden_case(name)
    net = build_optimizer(c, allow_pw_adaptors=True, optimize_pp=True)
    loss = net()
    assert loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
    loss.backward()
    got = dict({k: getattr(net, k).grad.cpu() for k in C.RAW_NAMES}, loss=loss.detach().cpu())
    ref64 = dict({k: golden[f"{name}_raw64_{k}"] for k in C.RAW_NAMES}, loss=golden[f"{name}_loss64"])
    ref32 = dict({k: golden[f"{name}_raw32_{k}"] for k in C.RAW_NAMES}, loss=golden[f"{name}_loss32"])
    compare(got, ref64, ref32, ("loss",) + C.RAW_NAMES, name + " raw")


# ------------------------------------------------------------------------------------------------------------------- geometry
def test_one_pixel_views(built_lib):
    for dist in ("l1", "l2"):
        against_restatement(C.matrix_problem([(1, 1), (1, 1)], [(0, 1), (1, 0)], 3, zero_share=0.0), dist, f"1 x 1 {dist}")


# a chunk is 512 pixels, two per thread of a workgroup.  35, 323 and 256 pixels: less than a wave, a partial last wave, half a chunk; 512 and
# 513: one whole chunk, a chunk and one pixel; 1024 and 1025: two chunks on two workgroups, and one pixel on a third; 2049: five; 65792: 129
# chunks on the 64 workgroups a view gets at the most, so that each takes a second chunk, one a third, and adds to its partial rows
@pytest.mark.parametrize("shape", [(5, 7), (17, 19), (16, 16), (16, 32), (19, 27), (32, 32), (25, 41), (3, 683), (257, 256)])
def test_pixel_counts_around_the_chunk(built_lib, shape):
    dist = "l1" if (shape[0] * shape[1]) % 2 else "l2"
    against_restatement(C.matrix_problem([shape, shape, shape], [(0, 1), (1, 2), (2, 0), (0, 2)], 10 + shape[0]), dist, f"{shape} {dist}")


def test_shapes_that_differ_across_an_edge(built_lib):
    against_restatement(C.matrix_problem([(6, 8), (8, 6), (5, 7), (33, 32)], [(0, 1), (1, 2), (2, 3), (3, 0), (1, 0)], 41), "l1", "mixed shapes")


def test_one_observation_next_to_forty(built_lib):
    shapes = [(5, 7)] * 41
    got, _ = against_restatement(C.matrix_problem(shapes, [(0, v) for v in range(1, 41)], 42), "l1", "view 0 with 40 observations")
    assert got["d_poses"].abs().max() > 0


def test_three_hundred_edges_over_25_views(built_lib):
    edges = [(i, j) for i in range(25) for j in range(i + 1, 25)]
    assert len(edges) == 300
    against_restatement(C.matrix_problem([(4, 5)] * 25, edges, 43), "l2", "300 edges")


def test_many_edges_share_one_pointer(built_lib):
    shapes, edges = [(9, 11)] * 5, C.STAR5 + [(1, 2), (2, 3)]
    P = C.matrix_problem(shapes, edges, 44, share_maps=True)
    args, obs, pts, w = upload(P)
    table = obs.tables["obs_table_host"][0].reshape(-1, 4)
    assert len({int(a) for a in table[:, 0]}) == 5 and len({int(a) for a in table[:, 1]}) == 5 and len(table) == 20   # one map per view, 20 observations
    against_restatement(P, "l1", "shared maps")


# ------------------------------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("dist", ["l1", "l2"])
def test_zero_residual_gives_zero_not_nan(built_lib, dist):
    got = run(C.exact_problem(), dist)
    assert float(got["loss"]) == 0.0
    for k in C.MATRIX_NAMES:
        assert not torch.isnan(got[k]).any() and float(got[k].abs().max()) == 0.0, k


def test_all_weights_zero(built_lib):
    P = C.matrix_problem([(6, 8), (8, 6), (6, 8)], C.SYM3, 45)
    P["w"] = [np.zeros_like(x) for x in P["w"]]
    for dist in ("l1", "l2"):
        got = run(P, dist)
        assert float(got["loss"]) == 0.0 and all(float(got[k].abs().max()) == 0.0 for k in C.MATRIX_NAMES)


def test_a_nan_stays_with_its_view_and_edge(built_lib):
    P = C.matrix_problem([(6, 8), (8, 6), (6, 8)], [(0, 1), (1, 2), (2, 0)], 46)
    P["pts"][1] = P["pts"][1].copy()
    P["w"][1] = P["w"][1].copy()
    P["pts"][1][3, 2, 1] = np.nan                                              # edge 0, side 1: view 1, pixel (3, 2)
    P["w"][1][3, 2] = 1.0
    got, ref = against_restatement(P, "l1", "NaN")                            # NaNs at the same places, everything else within the bar
    assert torch.isnan(got["loss"])
    dl = got["d_log_depth"]
    assert int(torch.isnan(dl).sum()) == 1 and bool(torch.isnan(dl[48 + 3 * 6 + 2]))
    for k in ("d_poses", "d_focals", "d_pp"):
        assert torch.isnan(got[k][1]).all() and not torch.isnan(got[k][[0, 2]]).any(), k
    for k in ("d_pw", "d_adapt"):
        assert torch.isnan(got[k][0]).all() and not torch.isnan(got[k][[1, 2]]).any(), k
    # a NaN under a weight of exactly 0 reaches nothing
    P["w"][1][3, 2] = 0.0
    clean = run(P, "l1")
    assert not any(torch.isnan(clean[k]).any() for k in ("loss",) + C.MATRIX_NAMES)


# ------------------------------------------------------------------------------------------------------------------- other checks
def test_two_runs_give_the_same_bits_and_leave_the_inputs(built_lib):
    from fast3r_amd import post_ops
    P = C.matrix_problem([(33, 32), (25, 41), (257, 256)], C.SYM3, 47)
    args, obs, pts, w = upload(P)
    before = [a.clone() for a in args + pts + w]
    a = post_ops.galign_loss_grad(*args, obs.tables, "l1")
    b = post_ops.galign_loss_grad(*args, obs.tables, "l1")
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(before, args + pts + w))


def test_grad_output_scales_the_gradients(built_lib):
    import fast3r_amd
    P = C.matrix_problem([(6, 8), (8, 6), (6, 8)], C.SYM3, 48)
    args, obs, _, _ = upload(P)
    grads = []
    for factor in (1.0, -2.5):
        leaves = [a.clone().requires_grad_() for a in args]
        loss = fast3r_amd.alignment_loss(*leaves, obs, "l1")
        assert loss.dim() == 0 and loss.is_cuda and loss.requires_grad
        (factor * loss).backward()
        grads.append([x.grad for x in leaves])
    for g1, g2 in zip(*grads):
        assert torch.equal(g2, g1 * -2.5) and g1.abs().max() > 0
    # 4 x 4 poses and (N, 1) focals pass, the bottom row gets a zero gradient
    poses44 = torch.cat((args[0], torch.tensor([[[0.0, 0, 0, 1]]], device=DEV).expand(3, 1, 4)), dim=1).requires_grad_()
    f1 = args[1].reshape(-1, 1).clone().requires_grad_()
    fast3r_amd.alignment_loss(poses44, f1, args[2], args[3], args[4], args[5], obs, "l1").backward()
    assert torch.equal(poses44.grad[:, :3], grads[0][0]) and float(poses44.grad[:, 3].abs().max()) == 0 and torch.equal(f1.grad[:, 0], grads[0][1])


# ------------------------------------------------------------------------------------------------------------------- the loop
def test_first_iteration_moves_every_parameter_as_the_reference(built_lib, golden):
    c = C.loop_case()
    net = build_optimizer(c)
    start = {k: getattr(net, k).detach().clone() for k in ("pw_poses", "im_poses", "im_focals", "im_depthmaps")}
    assert abs(float(net().detach()) - float(golden["loop_l0"])) <= 1e-5 * float(golden["loop_l0"])
    net.compute_global_alignment(niter=1, lr=C.LOOP_LR)
    for k, before in start.items():
        g0, want = golden[f"loop_grad0_{k}"], golden[f"loop_first_{k}"]
        mask = torch.from_numpy(np.abs(g0) > 1e-3 * np.abs(g0).max())
        got = getattr(net, k).detach().cpu()
        moved = (got - before.cpu()).abs()
        diff = (got - torch.from_numpy(want)).abs()
        print(k, f"{int(mask.sum())} of {mask.numel()} entries, worst |ours - reference| = {float(diff[mask].max()):.2e}, steps {float(moved[mask].min()):.2e} .. {float(moved[mask].max()):.2e}")
        assert int(mask.sum()) > 0 and float(diff[mask].max()) <= 1e-3 * C.LOOP_LR, k
        assert float(moved[mask].min()) > 0.5 * C.LOOP_LR                       # the first Adam step is lr g / (|g| + eps)
    assert torch.equal(net.im_pp.cpu(), torch.from_numpy(c["im_pp"])) and torch.equal(net.pw_adaptors.cpu(), torch.from_numpy(c["pw_adaptors"]))


def test_hundred_iterations_reach_the_reference_s_decrease_with_one_read(built_lib, golden, monkeypatch):
    """measured on an MI355X: the loss falls from 0.50041 to 0.01931 (the reference's CPU loop: 0.01932)"""
    from fast3r_amd import PointCloudOptimizer
    net = build_optimizer(C.loop_case())
    reads = {"read_back": 0, "other": 0}
    real = PointCloudOptimizer._read_back

    def read_back(history):
        assert history.is_cuda and history.shape == (C.LOOP_NITER,) and history.dtype == torch.float32
        reads["read_back"] += 1
        reads["other"] -= 1                                                       # its own .cpu() is the one allowed read
        return real(history)

    def counting(fn):
        def wrapped(self, *a, **k):
            if self.is_cuda:
                reads["other"] += 1
            return fn(self, *a, **k)
        return wrapped
    monkeypatch.setattr(PointCloudOptimizer, "_read_back", staticmethod(read_back))
    for name in ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__"):
        monkeypatch.setattr(torch.Tensor, name, counting(getattr(torch.Tensor, name)))
    final = net.compute_global_alignment(niter=C.LOOP_NITER, lr=C.LOOP_LR)
    monkeypatch.undo()
    assert reads == {"read_back": 1, "other": 0}, reads
    hist = net.loss_history
    assert isinstance(final, float) and not hist.is_cuda and hist.shape == (C.LOOP_NITER,) and final == float(hist[-1])
    l0, lf = float(golden["loop_l0"]), float(golden["loop_lf"])
    print(f"loss {float(hist[0]):.5f} -> {final:.5f}; the reference's loop: {l0:.5f} -> {lf:.5f}")
    assert abs(float(hist[0]) - l0) <= 1e-5 * l0
    assert final <= lf + 0.1 * (l0 - lf)


def test_niter_zero_and_linear_schedule(built_lib):
    net = build_optimizer(C.loop_case())
    assert net.compute_global_alignment(niter=0) == float("inf") and net.loss_history.numel() == 0
    first = float(net().detach())
    last = net.compute_global_alignment(niter=5, schedule="linear", lr=0.01)
    assert np.isfinite(last) and net.loss_history.shape == (5,) and abs(float(net.loss_history[0]) - first) <= 1e-6 * first


# ------------------------------------------------------------------------------------------------------------------- end to end
def scene_passes(anchors, H=48, W=64, seed=5):
    """a synthetic scene as forward passes with different anchor views: four cameras near the origin (the poses and focals of
    tests/galign_cases.py) look down +z at a surface with strong relief -- depths between 2 and 4, so that focal and distance are not
    confused as they are in front of a plane; pass k holds every view's points in the frame of its first view, and every view's local points"""
    tr = C.raw_case(((H, W),) * 4, [(0, 1)], "l1", "log", seed, 0.0)["true"]
    N = 4
    rs = np.random.RandomState(seed)
    local, world = [], []
    for v in range(N):
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        ray = np.stack([(xs - W / 2) / tr["f"][v], (ys - H / 2) / tr["f"][v], np.ones((H, W))], -1)
        depth = 3.0 + np.sin(3 * np.pi * xs / W + v) * np.cos(2 * np.pi * ys / H + 0.5 * v)
        local.append(ray * depth[..., None])
        world.append(local[v] @ tr["R"][v].T + tr["t"][v])
    conf = [rs.uniform(1.5, 6.0, (H, W)).astype(np.float32) for _ in range(N)]
    outputs = []
    for a in anchors:
        order = [a] + [v for v in range(N) if v != a]
        preds = []
        for v in order:
            in_anchor = (world[v] - tr["t"][a]) @ tr["R"][a]
            preds.append({"pts3d_in_other_view": gpu(in_anchor.astype(np.float32)[None]), "conf": gpu(conf[v][None]),
                          "pts3d_local": gpu(local[v].astype(np.float32)[None]), "conf_local": gpu(conf[v][None])})
        outputs.append({"preds": preds, "views": [{"img": gpu(rs.uniform(-1, 1, (1, 3, H, W)).astype(np.float32))} for _ in order]})
    return outputs, tr


def test_two_passes_end_to_end(built_lib):
    import fast3r_amd
    outputs, tr = scene_passes([0, 2])
    view1, view2, pred1, pred2 = fast3r_amd.pairs_from_passes(outputs, [0, 2])
    net = fast3r_amd.MultiViewDUSt3RLitModule.global_aligner(dict(view1=view1, view2=view2, pred1=pred1, pred2=pred2), DEV)
    assert isinstance(net, fast3r_amd.PointCloudOptimizer) and net.edges == [(0, 1), (0, 2), (0, 3), (2, 0), (2, 1), (2, 3)]
    assert net._observations().tables["obs_table_host"][0].reshape(-1, 4)[0, 0] == net._observations().tables["obs_table_host"][0].reshape(-1, 4)[2, 0]
    final = net.compute_global_alignment(init="passes", niter=50)
    hist = net.loss_history
    print(f"init='passes': loss {float(hist[0]):.5f} -> {final:.5f}")
    # a consistent scene: the start from pass 0 and one registration per pass is already close (residuals are of the order of the scene, 1.5,
    # without it), and the loop does not leave it
    assert np.isfinite(final) and float(hist[0]) < 0.1 and final < 0.1
    focals = net.get_focals().detach().flatten().cpu().numpy()
    assert np.all(np.abs(focals / np.asarray(tr["f"]) - 1) < 0.2)
    cleaned = net.clean_pointcloud()
    assert cleaned is not net and len(cleaned.im_conf) == 4 and all(c.shape == (48, 64) and c.is_cuda for c in cleaned.im_conf)
    assert all(bool((a <= b).all()) for a, b in zip(cleaned.im_conf, net.im_conf))
    pts = [p.detach() for p in cleaned.get_pts3d()]
    p0 = outputs[0]["preds"]
    preds = [{"pts3d_in_other_view": pts[v][None].contiguous(), "conf": cleaned.im_conf[v][None].contiguous(), "pts3d_local": p0[v]["pts3d_local"],
              "conf_local": p0[v]["conf_local"], "pts3d_local_aligned_to_global": pts[v][None].contiguous()} for v in range(4)]
    scene = fast3r_amd.assemble_scene(preds, outputs[0]["views"], poses=False)
    assert scene is not None
