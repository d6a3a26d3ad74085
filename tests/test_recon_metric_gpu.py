"""Reconstruction metrics on the GPU (fast3r_amd/recon_metric.py, csrc/f3r_recon.hip): exact 1-NN and k-NN against a chunked fp64 brute
force, the metrics against the reference's numbers (tests/golden/recon_cases.pt, tools/make_golden_recon.py), normals against the
restatement, evaluate_reconstruction against the reference method, determinism, a real-size sample."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recon_ref  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "recon_cases.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def brute_d2(q, db):
    """fp64 ((dx^2 + dy^2) + dz^2) of every (query, database) pair, one elementwise op at a time (no contraction)"""
    q, db = q.double(), db.double()
    dx = q[:, None, 0] - db[None, :, 0]
    d2 = dx * dx
    dy = q[:, None, 1] - db[None, :, 1]
    d2 = d2 + dy * dy
    dz = q[:, None, 2] - db[None, :, 2]
    return d2 + dz * dz


def brute_nn(q, db, chunk=None):
    chunk = chunk or max(1, (1 << 25) // max(db.shape[0], 1))
    ds, ids = [], []
    ar = torch.arange(db.shape[0], device=db.device)
    for c in range(0, q.shape[0], chunk):
        d2 = brute_d2(q[c:c + chunk], db)
        mn = d2.min(1).values
        ids.append(torch.where(d2 == mn[:, None], ar, db.shape[0]).min(1).values)  # ties -> the smaller index
        ds.append(mn.sqrt())
    return torch.cat(ds), torch.cat(ids)


def check_nn(q, db):
    from fast3r_amd import nearest_neighbors
    d, i = nearest_neighbors(q, db)
    bd, bi = brute_nn(q, db)
    rel = ((d - bd).abs() / bd.clamp_min(1e-300)).max().item()
    assert rel <= 1e-14, rel
    assert bool((i == bi).all())  # both resolve exact ties to the smaller index, so the indices agree everywhere
    return d, i


DISTS = {  # (query kind, n, seed, database kind, m, seed)
    "uniform": ("uniform", 20000, 1, "uniform", 30000, 2),
    "surface": ("surface", 20000, 3, "surface", 40000, 4),
    "outliers": ("outliers", 20000, 5, "outliers", 30000, 6),
    "duplicates": ("duplicates", 10000, 7, "duplicates", 20000, 8),
    "outside": ("outside", 5000, 9, "uniform", 20000, 10),
}


@pytest.mark.parametrize("name", list(DISTS))
def test_nn_exact_vs_brute_force(dev, name):
    qk, n, qs, dk, m, ds = DISTS[name]
    q = torch.from_numpy(recon_ref.make_cloud(qk, n, qs)).to(dev)
    db = torch.from_numpy(recon_ref.make_cloud(dk, m, ds)).to(dev)
    check_nn(q, db)
    check_nn(db, db)  # every point finds itself (or an exact duplicate with a smaller index)


@pytest.mark.parametrize("m", [63, 64, 65, 2047, 2048, 2049])
def test_nn_database_sizes_at_wave_and_tile_boundaries(dev, m):
    """the sort of the index walks its 2048-element tiles in 64-element steps: one short of, at and one over each"""
    q = torch.from_numpy(recon_ref.make_cloud("uniform", 200, 61)).to(dev)
    db = torch.from_numpy(recon_ref.make_cloud("uniform", m, 62 + m)).to(dev)
    check_nn(q, db)


def test_nn_small_and_degenerate(dev):
    from fast3r_amd import nearest_neighbors
    one = torch.tensor([[1.0, 2.0, 3.0]], device=dev)
    q = torch.rand((100, 3), device=dev)
    d, i = nearest_neighbors(q, one)
    assert bool((i == 0).all()) and torch.allclose(d, (q.double() - one.double()).norm(dim=1), rtol=1e-14)
    same = torch.ones((50, 3), device=dev)  # all points identical: one cell, every query ties -> index 0
    d, i = nearest_neighbors(q, same)
    assert bool((i == 0).all())
    d, i = nearest_neighbors(q, torch.zeros((0, 3), device=dev))
    assert bool(torch.isinf(d).all()) and bool((i == 0).all())
    d, i = nearest_neighbors(torch.zeros((0, 3), device=dev), q)
    assert d.numel() == 0


def test_non_finite_inputs_are_rejected(dev):
    """cKDTree raises ValueError for NaN / inf data or queries; so does this path, before anything searches (no corrupt index)"""
    from fast3r_amd import accuracy, completion_ratio, estimate_normals, nearest_neighbors
    db = torch.from_numpy(recon_ref.make_cloud("surface", 20000, 51)).to(dev)
    q = torch.from_numpy(recon_ref.make_cloud("surface", 5000, 52)).to(dev)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for which in (0, 1, 2):
            d = db.clone()
            d[1234, which] = bad
            with pytest.raises(ValueError, match="non-finite"):
                nearest_neighbors(q, d)
            with pytest.raises(ValueError, match="non-finite"):
                estimate_normals(d)
            with pytest.raises(ValueError, match="non-finite"):
                accuracy(d, q)
            qq = q.clone()
            qq[77, which] = bad
            with pytest.raises(ValueError, match="non-finite"):
                nearest_neighbors(qq, db)
            with pytest.raises(ValueError, match="non-finite"):
                completion_ratio(qq, db)
    two = db.clone()
    two[5, 0], two[9, 2] = float("nan"), float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        nearest_neighbors(q, two)
    d, i = nearest_neighbors(q, db)  # the library still works after the rejections
    bd, bi = brute_nn(q, db)
    assert bool((d == bd).all()) and bool((i == bi).all())


def test_evaluate_reconstruction_with_inf_prediction_raises(dev, golden):
    views, preds, p_icp, p_metric = _gpu_case(golden["eval"]["b1_p0"]["recipe"], dev)
    preds[1]["pts3d_in_other_view"][0, 3, 4, 0] = float("inf")
    views[1]["valid_mask"][0, 3, 4] = True  # a kept pixel (percentile 0 keeps every valid one)
    with pytest.raises(ValueError, match="non-finite"):
        _Lit().m.evaluate_reconstruction(views, preds, "x", p_icp, p_metric, use_pts3d_from_local_head=False)


def _ngrid(ix):
    return int(ix.buf.view(torch.int32)[44].item())  # NNHeader.ngrid: after the two 88-byte grids


INDEX_CASES = [("uniform", m, 80 + k) for k, m in enumerate((1, 63, 64, 65, 2047, 2048, 2049, 4097, 6145))] + [
    ("duplicates", 20000, 8),   # long runs of equal keys across the sort's tiles
    ("outliers", 30000, 6),     # two grids, one key space
    ("uniform", 1025000, 90),   # more than 65,536 cells: the smallest uniform size (in steps of 5000) whose keys take 17 bits, three passes
]


def test_index_bytes_vs_numpy_restatement(dev):
    """The index itself, not the answers it gives (an exact search hides a mis-sorted or mis-tabulated index while some ring still finds
    the point): the sorted keys, the records' order and coordinates and the dense cell starts equal recon_ref.check_nn_index's numpy
    restatement from the header the build wrote.  Database sizes at the wave and the 2048-key tile of the shared sort, a third tile
    with a one-key tail, and 0 .. 3 sort passes ((key_bits + 7) // 8)."""
    from fast3r_amd.recon_metric import NNIndex
    passes = {}
    for kind, m, seed in INDEX_CASES:
        pts = recon_ref.make_cloud(kind, m, seed)
        raw = NNIndex(torch.from_numpy(pts).to(dev)).buf.view(torch.uint8).cpu().numpy()
        H = recon_ref.check_nn_index(raw, pts)
        assert (1 << H["key_bits"]) >= H["ncells"] and (H["key_bits"] == 0 or (1 << (H["key_bits"] - 1)) < H["ncells"])
        passes[(kind, m)] = (H["key_bits"] + 7) // 8
        print(f"{kind} {m}: ngrid {H['ngrid']}, dense {H['dense']}, {H['ncells']} cells, {H['occupied']} occupied, {H['key_bits']} key bits")
        if kind == "outliers":
            assert H["ngrid"] == 2
        if m == 1025000:
            assert H["key_bits"] >= 17
    assert {1, 2, 3} <= set(passes.values()), passes


def test_far_outliers_get_their_own_grid_and_stay_exact(dev):
    """1 M points in two clusters + 0.1 % outliers at 1e4 x the scene: the outliers go to a second grid; 1-NN of every outlier and
    of 4096 sampled inliers, and k-NN of sampled points (outliers included), equal the brute force"""
    from fast3r_amd import nearest_neighbors
    from fast3r_amd.recon_metric import NNIndex
    db = torch.from_numpy(recon_ref.make_cloud("outliers", 1 << 20, 61)).to(dev)
    q = torch.from_numpy(recon_ref.make_cloud("outliers", 1 << 20, 62)).to(dev)
    ix = NNIndex(db)
    assert _ngrid(ix) == 2
    assert _ngrid(NNIndex(torch.from_numpy(recon_ref.make_cloud("surface", 50000, 63)).to(dev))) == 1
    d, i = nearest_neighbors(q, db)
    far = (q.abs().max(1).values > 10).nonzero().flatten()
    g = torch.Generator(device="cpu").manual_seed(3)
    sel = torch.cat([far, torch.randperm(q.shape[0], generator=g)[:4096].to(dev)])
    bd, bi = brute_nn(q[sel], db, chunk=16)
    assert bool((d[sel] == bd).all()) and bool((i[sel] == bi).all())
    _, ki, _ = ix.knn(30, normals=False, neighbours=True)
    far_db = (db.abs().max(1).values > 10).nonzero().flatten()
    ps = torch.cat([far_db[:256], torch.randperm(db.shape[0], generator=g)[:256].to(dev)])
    for c in range(0, ps.numel(), 16):
        rows = ps[c:c + 16]
        d2 = brute_d2(db[rows], db)
        kth = d2.topk(30, dim=1, largest=False).values[:, -1]
        got = d2.gather(1, ki[rows].long())
        assert bool((got <= kth[:, None]).all())
        hit = torch.zeros_like(d2, dtype=torch.bool).scatter_(1, ki[rows].long(), True)
        assert bool((hit | ~(d2 < kth[:, None])).all())


def test_knn_sets_vs_brute_force(dev):
    from fast3r_amd.recon_metric import NNIndex
    for kind, m, seed in (("surface", 20000, 12), ("duplicates", 6000, 13), ("outliers", 10000, 14)):
        p = torch.from_numpy(recon_ref.make_cloud(kind, m, seed)).to(dev)
        _, ki, kd = NNIndex(p).knn(30, normals=False, neighbours=True)
        sel = torch.arange(0, m, max(1, m // 1500), device=dev)
        d2 = brute_d2(p[sel], p)
        kth = d2.topk(30, dim=1, largest=False).values[:, -1]
        got = brute_d2(p[sel], p).gather(1, ki[sel].long())
        assert bool((got <= kth[:, None]).all()), kind                                   # nothing beyond the k-th distance
        assert bool(((d2 < kth[:, None]).sum(1) <= 30).all())
        inner = (d2 < kth[:, None])
        hit = torch.zeros_like(inner).scatter_(1, ki[sel].long(), True)
        assert bool((hit | ~inner).all()), kind                                           # everything strictly inside is there
        assert bool((kd[sel] == got.sqrt()).all()), kind
        # (distance, index) order
        k2 = got
        ordered = (k2[:, 1:] > k2[:, :-1]) | ((k2[:, 1:] == k2[:, :-1]) & (ki[sel][:, 1:] > ki[sel][:, :-1]))
        assert bool(ordered.all()), kind


def _rel(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / max(abs(b), 1e-300) if a != b else 0.0


def test_metrics_vs_reference_golden(dev, golden):
    from fast3r_amd import accuracy, completion, completion_ratio
    for name, g in golden["metric"].items():
        gk, ng, gs, rk, nr, rs, th = g["recipe"]
        gt = torch.from_numpy(recon_ref.make_cloud(gk, ng, gs)).to(dev)
        rec = torch.from_numpy(recon_ref.make_cloud(rk, nr, rs)).to(dev)
        ngt, nrec = recon_ref.unit_normals(ng, gs + 1000), recon_ref.unit_normals(nr, rs + 1000)
        acc = accuracy(gt, rec, ngt, nrec)
        comp = completion(gt, rec, ngt, nrec)
        # exact distance ties (the duplicates case) pick a tree-order-dependent index in cKDTree and the smaller one here, so the
        # normal terms are only comparable where no query ties
        n_terms = 2 if name == "duplicates" else 4
        for ours, ref in ((acc, g["accuracy"]), (comp, g["completion"])):
            for a, b in zip(ours[:n_terms], ref.tolist()[:n_terms]):
                assert _rel(a, b) <= 1e-12, (name, a, b)
        r = completion_ratio(gt, rec, th)
        assert isinstance(r, np.float32) and r == g["completion_ratio"].item(), (name, r)


def test_numpy_inputs_return_reference_types(dev, golden):
    from fast3r_amd import accuracy, completion, completion_ratio
    gk, ng, gs, rk, nr, rs, th = golden["metric"]["uniform"]["recipe"]
    gt, rec = recon_ref.make_cloud(gk, ng, gs), recon_ref.make_cloud(rk, nr, rs)
    ngt, nrec = recon_ref.unit_normals(ng, gs + 1000), recon_ref.unit_normals(nr, rs + 1000)
    for out in (accuracy(gt, rec, ngt, nrec), completion(gt, rec, ngt, nrec), accuracy(gt, rec), completion(gt.astype(np.float64), rec)):
        assert isinstance(out, tuple) and all(type(v) is np.float64 for v in out)
    for a, b in zip(accuracy(gt, rec, ngt, nrec), golden["metric"]["uniform"]["accuracy"].tolist()):
        assert _rel(a, b) <= 1e-12
    assert type(completion_ratio(gt, rec, th)) is np.float32
    # edge cases of the reference: empty database -> inf, empty queries -> nan, normals with an empty database -> IndexError
    e = np.zeros((0, 3), np.float32)
    a = accuracy(e, rec)
    assert np.isinf(a[0]) and np.isinf(a[1])
    a = accuracy(gt, e)
    assert np.isnan(a[0]) and np.isnan(a[1])
    with pytest.raises(IndexError):
        accuracy(e, rec, np.zeros((0, 3)), nrec)


def test_normals_vs_restatement(dev, golden):
    from fast3r_amd import estimate_normals
    g = golden["normals"]
    kind, n, seed = g["recipe"]
    p = recon_ref.make_cloud(kind, n, seed)
    nrm = estimate_normals(torch.from_numpy(p).to(dev)).cpu()
    assert nrm.dtype == torch.float64 and nrm.shape == (n, 3)
    dot = (nrm * g["normals"].double()).sum(1).abs()
    sep = g["separated"]
    assert sep.float().mean() > 0.9
    assert dot[sep].min().item() >= 1 - 1e-6, dot[sep].min().item()
    # fewer than 3 points: +z, as Open3D
    two = estimate_normals(torch.rand((2, 3), device=dev)).cpu()
    assert two.tolist() == [[0.0, 0.0, 1.0]] * 2


class _Lit:
    def __init__(self):
        from fast3r_amd import MultiViewDUSt3RLitModule
        self.m = MultiViewDUSt3RLitModule(net=torch.nn.Identity())


def _gpu_case(recipe, dev):
    B, sizes, seed, p_icp, p_metric = recipe
    views, preds = recon_ref.make_eval_case(B, sizes, seed)
    views = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in views]
    preds = [{k: v.to(dev) for k, v in d.items()} for d in preds]
    return views, preds, p_icp, p_metric


# measured margins against the reference method (docs/rows_f.md): the asserted bounds below
EVAL_REL_DIST, EVAL_ABS_NC = 5e-5, 1e-4  # measured: 1.1e-5, 2.7e-5


@pytest.mark.parametrize("case", ["b1_p0", "b1_p85_50", "b2_p0", "b2_p85_50"])
def test_evaluate_reconstruction_vs_reference(dev, golden, case):
    g = golden["eval"][case]
    views, preds, p_icp, p_metric = _gpu_case(g["recipe"], dev)
    lit = _Lit().m
    out = lit.evaluate_reconstruction(views, preds, "golden", min_conf_thr_percentile_for_local_alignment_and_icp=p_icp,
                                      min_conf_thr_percentile_for_metric_cacluation=p_metric)
    got = lit.reconstruction_metrics_per_epoch["golden"]
    assert out is got and got.keys() == g["metrics"].keys()
    worst = {"dist": 0.0, "nc": 0.0}
    for scene, ref in g["metrics"].items():
        assert got[scene].keys() == ref.keys()
        for k, v in ref.items():
            assert type(got[scene][k]) is np.float64
            if k.startswith("nc"):
                worst["nc"] = max(worst["nc"], abs(float(got[scene][k]) - v))
            else:
                worst["dist"] = max(worst["dist"], _rel(got[scene][k], v))
    print(f"{case}: worst rel dist {worst['dist']:.3e}, worst abs nc {worst['nc']:.3e}")
    assert worst["dist"] <= EVAL_REL_DIST and worst["nc"] <= EVAL_ABS_NC, worst


def _restated_eval(views, preds, i, p_icp, p_metric):
    """evaluate_reconstruction of sample i on the CPU from the pieces of tests/recon_ref.py, global head: per view the two
    torch.quantile thresholds, the masks, torch.cat over the views, the weighted registration, normals, accuracy / completion"""
    x, y, w, gt_all = [], [], [], []
    for view, pred in zip(views, preds):
        conf, valid = pred["conf"][i].cpu(), view["valid_mask"][i].cpu()
        keep = valid & (conf >= torch.quantile(conf.reshape(-1), p_metric / 100.0))
        x.append(pred["pts3d_in_other_view"][i].cpu()[keep])
        y.append(view["pts3d"][i].cpu()[keep])
        w.append(conf[keep] >= torch.quantile(conf.reshape(-1), p_icp / 100.0))
        gt_all.append(view["pts3d"][i].cpu()[valid])
    x, y, w, gt_all = torch.cat(x), torch.cat(y), torch.cat(w), torch.cat(gt_all)
    R, t, s = recon_ref.rigid_points_registration(x, y, weights=w, compute_scaling=True)
    rec = (s * (x @ R.T) + t).numpy().astype(np.float64)
    gt = gt_all.numpy().astype(np.float64)
    n_rec, n_gt = recon_ref.estimate_normals(rec), recon_ref.estimate_normals(gt)
    acc = recon_ref.accuracy(gt, rec, n_gt, n_rec)
    comp = recon_ref.completion(gt, rec, n_gt, n_rec)
    return {"accuracy": acc[0], "accuracy_median": acc[1], "completion": comp[0], "completion_median": comp[1],
            "nc1": acc[2], "nc1_median": acc[3], "nc2": comp[2], "nc2_median": comp[3]}, len(x), len(gt)


def test_evaluate_reconstruction_at_wave_and_tile_boundaries(dev):
    """Two views of 130 and 3072 pixels with exactly 65 and 2049 valid ones: the first segment ends inside a 64-pixel step of the first
    2048-pixel compaction tile, the kept GT points run one past a wave and one past a tile.  The bounds are those of
    test_evaluate_reconstruction_vs_reference: the same fp32 registration and transform against the same CPU method."""
    views, preds = recon_ref.make_eval_case(1, [(5, 26), (48, 64)], 71)
    g = torch.Generator().manual_seed(72)
    for view, n_valid in zip(views, (65, 2049)):
        vm = torch.zeros(view["valid_mask"].numel(), dtype=torch.bool)
        vm[torch.randperm(vm.numel(), generator=g)[:n_valid]] = True
        view["valid_mask"] = vm.reshape(view["valid_mask"].shape)
    want, n_pred, n_gt = _restated_eval(views, preds, 0, 50, 10)
    assert n_gt == 65 + 2049 and 0 < n_pred < n_gt
    views = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in views]
    preds = [{k: v.to(dev) for k, v in d.items()} for d in preds]
    got = _Lit().m.evaluate_reconstruction(views, preds, "edge", 50, 10, use_pts3d_from_local_head=False)["scene71/view0"]
    assert got.keys() == want.keys()
    worst = {"dist": 0.0, "nc": 0.0}
    for k, v in want.items():
        if k.startswith("nc"):
            worst["nc"] = max(worst["nc"], abs(float(got[k]) - v))
        else:
            worst["dist"] = max(worst["dist"], _rel(got[k], v))
    print(f"edge: worst rel dist {worst['dist']:.3e}, worst abs nc {worst['nc']:.3e}")
    assert worst["dist"] <= EVAL_REL_DIST and worst["nc"] <= EVAL_ABS_NC, worst


def test_evaluate_reconstruction_asserts_percentiles(dev, golden):
    views, preds, _, _ = _gpu_case(golden["eval"]["b1_p0"]["recipe"], dev)
    with pytest.raises(AssertionError):
        _Lit().m.evaluate_reconstruction(views, preds, "x", min_conf_thr_percentile_for_local_alignment_and_icp=10,
                                         min_conf_thr_percentile_for_metric_cacluation=20)


def test_deterministic(dev, golden):
    from fast3r_amd import estimate_normals, nearest_neighbors
    q = torch.from_numpy(recon_ref.make_cloud("surface", 30000, 31)).to(dev)
    db = torch.from_numpy(recon_ref.make_cloud("surface", 40000, 32)).to(dev)
    a, b = nearest_neighbors(q, db), nearest_neighbors(q, db)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(estimate_normals(db), estimate_normals(db))
    outs = []
    for _ in range(2):
        views, preds, p_icp, p_metric = _gpu_case(golden["eval"]["b2_p85_50"]["recipe"], dev)
        lit = _Lit().m
        lit.evaluate_reconstruction(views, preds, "d", p_icp, p_metric)
        outs.append({s: {k: np.float64(v).tobytes() for k, v in d.items()} for s, d in lit.reconstruction_metrics_per_epoch["d"].items()})
    assert outs[0] == outs[1]


def test_realsize_sample(dev):
    """One 20 x 512x384 sample: evaluate_reconstruction runs, and the 1-NN of 4096 sampled queries in both directions is exact."""
    from fast3r_amd import nearest_neighbors
    views, preds, _, _ = _gpu_case((1, [(384, 512)] * 20, 41, 0, 0), dev)
    lit = _Lit().m
    res = lit.evaluate_reconstruction(views, preds, "real", 50, 10)
    vals = [float(v) for d in res.values() for v in d.values()]
    assert len(vals) == 8 and all(np.isfinite(vals))
    gt = torch.cat([v["pts3d"][0].reshape(-1, 3) for v in views])
    pr = torch.cat([p["pts3d_local_aligned_to_global"][0].reshape(-1, 3) for p in preds]).float()
    g = torch.Generator(device="cpu").manual_seed(5)
    for q, db in ((pr, gt), (gt, pr)):
        sel = torch.randperm(q.shape[0], generator=g)[:4096].to(dev)
        d, i = nearest_neighbors(q, db)
        bd, bi = brute_nn(q[sel], db, chunk=8)
        assert bool((d[sel] == bd).all()) and bool((i[sel] == bi).all())
