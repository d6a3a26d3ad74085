"""Multi-view depth metrics on a real MI355X, through the C ABI (guarded placement: tests/depth_cases.py run) and through the Python API,
against the float64 restatement (tests/depth_ref.py).  Bit-equal: n_valid, thr, both medians, scale, the inlier counts and percentages, both
orders; two runs; the inputs.  Within (n + 8) 2^-53 relative: absrel, rmse and every s_k, o_k (a float64 sum of n non-negative terms in any
order is within (n - 1) 2^-53 of the exact sum the restatement takes; the division, scaling and square root add a few units); ause within
4 (n + 8) 2^-53 max_k(s_k) / s_0."""
import math

import numpy as np
import pytest
import torch

import depth_cases as C
import depth_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")


def bits(x):
    return np.float64(x).tobytes()


def check_against_reference(c, got, what):
    """one launch of a case against the restatement of each of its segments"""
    K, T = c["kw"]["n_bins"], len(c["kw"]["thresholds"])
    assert got["inputs_unchanged"], what
    starts = got["starts"]
    for i, ref in enumerate(C.reference(c["name"])):
        row, n, w = got["out"][i], ref["n_valid"], f"{what} segment {i}"
        assert row[0] == n and int(starts[i + 1]) - int(starts[i]) == n, w
        for col, key in ((1, "thr"), (2, "median_gt"), (3, "median_pred"), (4, "scale")):
            assert bits(row[col]) == bits(ref[key]) or (math.isnan(row[col]) and math.isnan(ref[key])), (w, key, row[col], ref[key])
        assert np.isnan(row[11 + T:15]).all() and np.isnan(row[7 + T:11]).all(), w
        assert row[11:11 + T].tolist() == [float(x) for x in ref["counts"]], (w, row[11:15], ref["counts"])
        s_k, o_k = row[16:16 + K], row[16 + K:16 + 2 * K]
        if n == 0:                                                       # NaN exactly where the restatement has it
            assert np.isnan(row[2:11]).all() and math.isnan(row[15]) and np.isnan(s_k).all() and np.isnan(o_k).all(), w
            continue
        assert not np.isnan(row[2:7]).any() and not np.isnan(row[15:]).any() and math.isnan(row[1]) == math.isnan(ref["thr"]), w
        assert [bits(x) for x in row[7:7 + T]] == [bits(x) for x in ref["inliers"]], w
        assert got["order_conf"][starts[i]:starts[i + 1]].tolist() == ref["order_conf"].tolist(), w
        assert got["order_err"][starts[i]:starts[i + 1]].tolist() == ref["order_err"].tolist(), w
        for col, key in ((5, "absrel"), (6, "rmse")):
            print(f"{w}: {key} got {row[col]!r} ref {ref[key]!r} n {n}")
            assert abs(row[col] - ref[key]) <= R.tolerance(n, ref[key]), (w, key, row[col], ref[key])
        for k in range(K):
            assert abs(s_k[k] - ref["s"][k]) <= R.tolerance(n, ref["s"][k]), (w, "s", k, s_k[k], ref["s"][k])
            assert abs(o_k[k] - ref["o"][k]) <= R.tolerance(n, ref["o"][k]), (w, "o", k, o_k[k], ref["o"][k])
        print(f"{w}: ause got {row[15]!r} ref {ref['ause']!r}")
        assert abs(row[15] - ref["ause"]) <= R.ause_tolerance(n, ref["s"]), (w, "ause", row[15], ref["ause"])


@pytest.fixture(scope="module")
def launched(built_lib):
    """every case through the guarded launch once: shared, never changed"""
    out = {name: C.run(built_lib, DEV, C.case(name), what=name) for name in C.CASES}
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", C.CASES)
def test_case_against_the_restatement(launched, name):
    check_against_reference(C.case(name), launched[name], name)


@pytest.mark.parametrize("name", ("shapes", "pct50", "conf_special"))
def test_placement_does_not_change_a_bit(launched, built_lib, name):
    """a second run, the prediction as channel 2 of a pointmap, and every operand 4 bytes past a 16-byte boundary (scalar loads)"""
    c, base = C.case(name), launched[name]
    for kw in (dict(), dict(pointmap=True), dict(misalign=True), dict(pointmap=True, misalign=True)):
        again = C.run(built_lib, DEV, c, what=f"{name} {kw}", **kw)
        assert again["inputs_unchanged"]
        for key in ("out", "order_conf", "order_err", "starts"):
            a, b = again[key], base[key]
            if key.startswith("order"):                                  # the slots past the valid pixels hold nothing
                a, b = a[:int(base["starts"][-1])], b[:int(base["starts"][-1])]
            assert a.tobytes() == b.tobytes(), (name, kw, key)


def test_special_confidences_sort_as_their_keys(launched):
    c, got = C.case("conf_special"), launched["conf_special"]
    conf = c["segs"][0]["conf"][got["order_conf"][:int(got["starts"][1])]]
    keys = R.fkey(conf).astype(np.int64)
    assert (np.diff(keys) >= 0).all() and np.isnan(conf[0]) and np.isnan(conf[-1])          # a negative NaN first, a positive one last
    zeros = np.flatnonzero(conf == 0)
    assert zeros.size and (np.diff(np.signbit(conf[zeros]).astype(int)) <= 0).all() and np.signbit(conf[zeros[0]])     # -0.0 before +0.0


# ------------------------------------------------------------------------------------------------------------------- the Python API
def _views_b2():
    """three views of different sizes, B = 2: per view (gt, depth, conf, mask) tensors and the restatement per (view, sample)"""
    data, refs = [], []
    kw = dict(C.KW, thresholds=(1.03, 1.25), n_bins=7)
    for v, (h, w) in enumerate(((5, 13), (31, 33), (32, 32))):
        segs = [C.plain(h * w, 500 + 2 * v + b) for b in range(2)]
        for s in segs:
            if s["mask"] is None:
                s["mask"] = np.ones(h * w, np.uint8)
        stack = lambda key, dt: torch.from_numpy(np.stack([s[key] for s in segs]).reshape(2, h, w).astype(dt))   # noqa: E731
        data.append((stack("g", np.float32), stack("p", np.float32), stack("conf", np.float32), stack("mask", np.uint8).bool()))
        refs += [R.segment(s["g"], s["p"], s["conf"], s["mask"], **kw) for s in segs]
    return data, refs, kw


def test_depth_metrics_three_views_of_different_sizes_b2(built_lib):
    import fast3r_amd
    data, refs, kw = _views_b2()
    gt, depth, conf, mask = ([d[i].to(DEV) for d in data] for i in range(4))
    pm = []
    for d in depth:
        p = torch.full(tuple(d.shape) + (3,), float("nan"), device=DEV)
        p[..., 2] = d
        pm.append(p)
    call = dict(inlier_thresholds=kw["thresholds"], eval_uncertainty=True, n_bins=kw["n_bins"])
    keep = [t.clone() for t in gt + pm + conf]
    a = fast3r_amd.depth_metrics(gt, pm, conf, mask, **call)
    b = fast3r_amd.depth_metrics(gt, depth, conf, [m.to(torch.uint8) for m in mask], **call)
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(keep, gt + pm + conf))     # inputs are not written to
    assert a["segments"] == (3, 2) and a["inliers"].shape == (6, 2) and a["sparsification"].shape == (6, 7)
    for key in ("n_valid", "thr", "median_gt", "median_pred", "scale", "absrel", "rmse", "inliers", "inlier_counts", "ause", "sparsification", "oracle"):
        assert a[key].tobytes() == b[key].tobytes(), key                                                          # a pointmap and a depth map: the same bits
    for i, ref in enumerate(refs):
        n = ref["n_valid"]
        assert a["n_valid"][i] == n > 0 and bits(a["scale"][i]) == bits(ref["scale"]) and bits(a["median_pred"][i]) == bits(ref["median_pred"])
        assert a["inlier_counts"][i].tolist() == ref["counts"] and [bits(x) for x in a["inliers"][i]] == [bits(x) for x in ref["inliers"]]
        assert abs(a["absrel"][i] - ref["absrel"]) <= R.tolerance(n, ref["absrel"]) and abs(a["rmse"][i] - ref["rmse"]) <= R.tolerance(n, ref["rmse"])
        for k in range(kw["n_bins"]):
            assert abs(a["sparsification"][i][k] - ref["s"][k]) <= R.tolerance(n, ref["s"][k])
            assert abs(a["oracle"][i][k] - ref["o"][k]) <= R.tolerance(n, ref["o"][k])
        assert abs(a["ause"][i] - ref["ause"]) <= R.ause_tolerance(n, ref["s"])
    plain = fast3r_amd.depth_metrics(gt, pm, None, None, alignment="none")
    assert "ause" not in plain and plain["inliers"].shape == (6, 1) and (plain["scale"] == 1.0).all() and np.isnan(plain["thr"]).all()


def _gt_views(n=3):
    import fast3r_amd
    rs = np.random.RandomState(5)
    images = [rs.randint(0, 256, (60, 80, 3)).astype(np.uint8) for _ in range(n)]
    depths = [(1.0 + 3.0 * rs.rand(60, 80)).astype(np.float32) for _ in range(n)]
    depths[1][:7, :9] = 0.0                                              # pixels without a depth: not valid
    K = np.array([[70, 0, 40], [0, 70, 30], [0, 0, 1]], dtype=np.float32)
    return fast3r_amd.build_gt_views(images, depths, [K] * n, [np.eye(4, dtype=np.float32)] * n, resolution=(32, 24), dataset="syn",
                                     labels=[f"room/seq/{i}" for i in range(n)])


def test_end_to_end_on_build_gt_views_output(built_lib):
    """predictions = the ground-truth camera points times 3 (identity poses: pts3d is in the camera's frame).  fl32(3 g) is within 2^-24 of
    3 g, so under "median" scale = 1/3 within 2^-23 and every |sp / g - 1| < 2^-22; under "none" every e = 2 within 2^-22."""
    import fast3r_amd
    views = _gt_views()
    assert all(bool((v["pts3d"][..., 2] == v["depthmap"])[v["valid_mask"]].all()) for v in views)
    preds = [{"pts3d_local": v["pts3d"] * 3.0, "conf_local": torch.rand(v["depthmap"].shape, device=DEV) + 0.5,
              "pts3d_in_other_view": v["pts3d"] * 3.0, "conf": torch.ones_like(v["depthmap"])} for v in views]
    (res,) = fast3r_amd.evaluate_multiview_depth(views, preds, eval_uncertainty=True, n_bins=10)
    assert res["scene"] == "room/seq" and res["views"] == [0, 1, 2] and set(res) >= {"absrel", "inliers_1.03", "rmse", "ause", "per_view"}
    pv = res["per_view"]
    assert pv["n_valid"].tolist() == [int(v["valid_mask"].sum()) for v in views] and pv["n_valid"][1] < 32 * 24
    assert (np.abs(pv["scale"] * 3.0 - 1.0) <= 2.0 ** -23).all() and 0.0 <= res["absrel"] <= 100 * 2.0 ** -22
    assert res["inliers_1.03"] == 100.0 and (pv["inliers_1.03"] == 100.0).all() and pv["sparsification"].shape == (3, 10)
    assert res["absrel"] == pytest.approx(float(np.mean(pv["absrel"])), rel=1e-15)
    (none,) = fast3r_amd.evaluate_multiview_depth(views, preds, alignment="none")
    assert abs(none["absrel"] - 200.0) <= 100 * 2.0 ** -22 and none["inliers_1.03"] == 0.0 and (none["per_view"]["scale"] == 1.0).all()
    (glob,) = fast3r_amd.evaluate_multiview_depth(views, preds, head="global")
    assert glob["views"] == [0] and glob["per_view"]["n_valid"].tolist() == [int(views[0]["valid_mask"].sum())]
    assert bits(glob["per_view"]["scale"][0]) == bits(pv["scale"][0]) and bits(glob["absrel"]) == bits(pv["absrel"][0])
    cpu_preds = [{k: t.cpu() for k, t in p.items()} for p in preds]     # preds as inference() hands them back: uploaded, same bits
    (back,) = fast3r_amd.evaluate_multiview_depth(views, cpu_preds, eval_uncertainty=True, n_bins=10)
    assert bits(back["absrel"]) == bits(res["absrel"]) and bits(back["ause"]) == bits(res["ause"])


def test_lit_module_fills_its_dict(built_lib):
    from fast3r_amd.multiview_dust3r_module import MultiViewDUSt3RLitModule
    views = _gt_views(2)
    preds = [{"pts3d_local": v["pts3d"] * 2.0, "conf_local": torch.ones_like(v["depthmap"])} for v in views]
    lit = MultiViewDUSt3RLitModule.load_for_inference(None)
    got = lit.evaluate_multiview_depth(views, preds, "syn", inlier_thresholds=(1.03, 1.25))
    assert got is lit.depth_metrics_per_epoch["syn"] and list(got) == ["room/seq"]
    sample = got["room/seq"]
    assert sample["inliers_1.03"] == 100.0 and sample["inliers_1.25"] == 100.0 and sample["absrel"] == 0.0 and sample["rmse"] == 0.0
    assert (sample["per_view"]["scale"] == 0.5).all() and "ause" not in sample
    lit.evaluate_multiview_depth(views, preds, "other", alignment="none")
    assert set(lit.depth_metrics_per_epoch) == {"syn", "other"} and lit.depth_metrics_per_epoch["other"]["room/seq"]["absrel"] == 100.0
