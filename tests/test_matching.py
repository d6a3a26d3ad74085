"""View matching, the parts that need no GPU: the numpy restatement (tests/match_ref.py) against the reference's own find_reciprocal_matches
and make_pairs (tests/golden/matches_cases.npz, written by tools/make_golden_matches.py), the case recipes (tests/match_cases.py) against
the properties they claim, and the host-only logic of fast3r_amd/matching.py: pair parsing, chunk planning against a byte budget, refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import match_cases as C
import match_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "matches_cases.npz")
CLOUD_PAIRS = {"patch01": ("patch0", "patch1"), "patch12": ("patch1", "patch2"), "patch20": ("patch2", "patch0"), "clouds": ("cloud0", "cloud1")}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.skipif(not os.path.isdir(os.path.join(os.environ.get("FAST3R_REFERENCE_ROOT", "/root/reference"), "fast3r")),
                    reason="needs the reference checkout")
def test_golden_generator_reproduces_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_matches.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_golden_holds_data_only_and_its_conditions(golden):
    assert bool(golden["margins_ok"]) and bool(golden["restatement_matches"]) and float(golden["margin"]) == 1e-9
    assert os.path.getsize(GOLDEN) < 1000 * 1000
    assert all(v.dtype.kind in "biuf" for v in golden.values())  # arrays and index lists, nothing else
    patches, clouds = C.golden_inputs(int(golden["seed"]))
    for k, p in enumerate(patches):
        assert p.shape[:2] == C.GOLDEN_PATCHES[k] and np.array_equal(p, golden[f"patch{k}"])
    for k, c in enumerate(clouds):
        assert c.shape == (C.GOLDEN_CLOUDS[k], 3) and np.array_equal(c, golden[f"cloud{k}"])


@pytest.mark.parametrize("name", sorted(CLOUD_PAIRS))
def test_restatement_reproduces_the_reference(golden, name):
    a, b = (golden[k].reshape(-1, 3) for k in CLOUD_PAIRS[name])
    rec, nn2, num, d2 = R.find_reciprocal_matches(a, b)
    assert rec.dtype == bool and np.array_equal(rec, golden[f"{name}_reciprocal_in_P2"])
    assert np.array_equal(nn2, golden[f"{name}_nn2_in_P1"]) and num == int(golden[f"{name}_num_matches"]) == int(rec.sum())
    best, second = R.best_two(b, a)
    assert np.array_equal(best, d2) and (second > best * (1 + 1e-9)).all()  # the condition the file records
    if name.startswith("patch"):
        assert num > 20  # overlapping patches of one surface do match
    # the other direction gives the same number of matches (the reference asserts it)
    assert R.find_reciprocal_matches(b, a)[2] == num


def test_restatement_reproduces_the_pair_lists(golden):
    keys = [k for k in golden if k.startswith("pairs_")]
    assert len(keys) > 200
    for key in keys:
        _, n, g, f, sym = key.split("_")
        want = golden[key]
        for fn in (R.scene_graph_pairs, __import__("fast3r_amd").scene_graph_pairs):
            got = fn(int(n[1:]), g, None if f == "None" else f, bool(int(sym)))
            assert got.dtype == np.int64 and got.shape == want.shape, key
            if g.startswith("swin"):  # the reference walks a set there
                assert sorted(map(tuple, got.tolist())) == sorted(map(tuple, want.tolist())), key
                half = len(got) // 2 if int(sym) else len(got)
                assert got[:half].tolist() == sorted(got[:half].tolist()) and (not int(sym) or np.array_equal(got[half:], got[:half, ::-1])), key
            else:
                assert np.array_equal(got, want), key


def test_ties_go_to_the_smaller_index_and_order():
    D = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0]], np.float32)
    idx, d2 = R.nearest(np.zeros((1, 3), np.float32), D)
    assert idx.tolist() == [0] and d2.tolist() == [1.0]
    rec, nn2, num, _ = R.find_reciprocal_matches(D, D)
    assert nn2.tolist() == [0, 1, 0, 3] and rec.tolist() == [True, True, False, True] and num == 3
    x, y, z = np.float32(1e-3), np.float32(3e-3), np.float32(7e-3)
    want = (np.float64(x) * np.float64(x) + np.float64(y) * np.float64(y)) + np.float64(z) * np.float64(z)
    assert R.sq_dists(np.array([[x, y, z]]), np.zeros((1, 3)))[0, 0] == want
    empty = np.zeros((0, 3), np.float32)
    rec, nn2, num, d2 = R.find_reciprocal_matches(empty, D)
    assert not rec.any() and nn2.tolist() == [0] * 4 and num == 0 and np.isinf(d2).all()
    assert R.find_reciprocal_matches(D, empty)[0].shape == (0,)
    with pytest.raises(ValueError):
        R.find_reciprocal_matches(np.array([[np.nan, 0, 0]], np.float32), D)


def test_quantile_restatement():
    """the project's quantile rule: rank q (n - 1) in fp32, at::lerp with every operation rounded.  torch.quantile itself may fuse the
    multiply and the add of its lerp, so it agrees to one unit in the last place, and exactly where the rank is an integer"""
    rs = np.random.RandomState(0)
    for n in (1, 2, 7, 70, 1001):
        v = rs.uniform(1, 5, n).astype(np.float32)
        for q in (0.0, 0.1, 0.375, 0.5, 0.99, 1.0):
            got, ref = R.quantile_f32(v, q), torch.quantile(torch.from_numpy(v), q).numpy()
            assert abs(np.float64(got) - np.float64(ref)) <= np.spacing(np.float32(ref)), (n, q)
            if q in (0.0, 1.0):
                assert got == (v.min() if q == 0.0 else v.max())
    assert R.quantile_f32(np.array([1, 2, 4, 8], np.float32), 0.5) == np.float32(3.0)       # rank 1.5: 4 - 2 * 0.5
    assert R.quantile_f32(np.array([1, 2, 4, 8], np.float32), 0.25) == np.float32(1.75)     # rank 0.75: 2 - 1 * 0.25
    v[3] = np.nan
    assert np.isnan(R.quantile_f32(v, 0.0)) and np.isnan(R.quantile_f32(v, 0.7)) and torch.isnan(torch.from_numpy(v).amin())
    from fast3r_amd.matching import _threshold
    for n in (1, 2, 7, 70, 1001):                                                          # the product's own threshold is that rule, bit for bit
        v = rs.uniform(1, 5, n).astype(np.float32)
        for q in (0.0, 0.1, 0.375, 0.5, 0.99, 1.0):
            assert _threshold(torch.from_numpy(v), q).numpy().tobytes() == R.quantile_f32(v, q).tobytes(), (n, q)
    v[0] = np.nan
    assert torch.isnan(_threshold(torch.from_numpy(v), 0.3)) and torch.isnan(_threshold(torch.from_numpy(v), 0.0))


# ------------------------------------------------------------------------------------------------------------------- the recipes
def test_recipes_have_the_properties_they_claim():
    c = C.counts_case()
    assert tuple(int(m.sum()) for m in c["masks"]) == C.COUNTS and len({p.shape[:2] for p in c["pts"]}) == len(C.COUNTS)
    assert R.match_views(c["pts"], None, c["masks"])["n_candidates"] == list(C.COUNTS)
    m = C.many_views_case()
    assert len(m["pts"]) == 257 and all(p.shape == (1, 3, 3) for p in m["pts"])
    d = C.degenerate_cases()
    assert len(np.unique(d["identical"]["pts"][0].reshape(-1, 3), axis=0)) == 1
    assert np.ptp(d["plane"]["pts"][0][..., 2]) == 0 and np.ptp(d["line"]["pts"][0][..., 1:]) == 0
    a, b = (p.reshape(-1, 3) for p in d["disjoint"]["pts"])
    assert (np.abs(b.mean(0) - a.mean(0)) > 100 * np.ptp(a, axis=0).max()).all()
    o = d["outliers"]["pts"][0].reshape(-1, 3)
    med = np.median(o, 0)
    ext = np.ptp(o[np.abs(o - med).max(1) < 10], axis=0).max()
    assert o.shape[0] == 5000 and (np.abs(o - med).max(1) > 900 * ext).sum() == 50
    u = d["duplicates"]["pts"][0].reshape(-1, 3)
    assert len(np.unique(u, axis=0)) < len(u)
    rec, nn2, _, d2 = R.find_reciprocal_matches(u, d["duplicates"]["pts"][1].reshape(-1, 3))
    assert (d2 == 0).all() and not rec.all()  # every point has an exact copy in the other view; among copies only the smallest index is mutual
    k = C.candidate_cases()
    assert [R.match_views(**_kw(k[f"subsample{s}"]))["n_candidates"][0] for s in (1, 2, 3)] == [70, 20, 12]
    sh = k["shared_threshold"]
    thr = R.quantile_f32(sh["confs"][0], 0.5)
    assert (sh["confs"][0] == thr).sum() >= 5 and R.match_views(**_kw(sh))["n_candidates"][0] == int((sh["confs"][0] >= thr).sum()) > 35
    assert R.match_views(**_kw(k["nan_conf"]))["n_candidates"][1] == 0 == R.match_views(**_kw(k["nan_conf_pct0"]))["n_candidates"][1]
    assert R.match_views(**_kw(k["one_pixel"]))["n_candidates"][2] == 1


def _kw(case):
    return {"pts": case["pts"], "confs": case.get("confs"), "masks": case.get("masks"), "pairs": case["pairs"], "pct": case.get("pct", 0),
            "subsample": case.get("subsample", 1)}


def test_match_views_restatement_order_and_transpose():
    c = C.views_case(3, 9, 11)
    res = R.match_views(c["pts"], pairs=[(0, 1), (1, 0), (0, 1)])
    o = res["offsets"]
    assert res["counts"][0] == res["counts"][1] == res["counts"][2] > 0
    fwd = (res["xy_i"][o[0]:o[1]], res["xy_j"][o[0]:o[1]])
    bwd = (res["xy_i"][o[1]:o[2]], res["xy_j"][o[1]:o[2]])
    key = lambda a, b: sorted(map(tuple, np.concatenate([a, b], 1).tolist()))  # noqa: E731
    assert key(fwd[0], fwd[1]) == key(bwd[1], bwd[0])                        # the transposed pair holds the same matches
    lin = fwd[1][:, 1] * 11 + fwd[1][:, 0]
    assert (np.diff(lin) > 0).all()                                            # ascending candidate order of view j
    assert np.array_equal(res["xy_i"][o[2]:o[3]], fwd[0])
    cv = R.covisibility(res, 3)
    assert cv[0, 1] == cv[1, 0] == 3 * res["counts"][0] and cv[2].sum() == 0


# ------------------------------------------------------------------------------------------------------------------- host logic
def test_pair_parsing_and_refusals():
    from fast3r_amd import matching as M, scene_graph_pairs
    assert scene_graph_pairs(4).tolist() == [[1, 0], [2, 0], [2, 1], [3, 0], [3, 1], [3, 2]] + [[0, 1], [0, 2], [1, 2], [0, 3], [1, 3], [2, 3]]
    assert scene_graph_pairs(5, "swin-1", symmetrize=False).tolist() == [[0, 1], [0, 4], [1, 2], [2, 3], [3, 4]]
    assert scene_graph_pairs(2, "swin", symmetrize=False).tolist() == [[0, 0], [0, 1], [1, 1]]    # the window wraps onto the view itself
    assert scene_graph_pairs(4, "oneref-2", symmetrize=False).tolist() == [[2, 0], [2, 1], [2, 3]]
    assert scene_graph_pairs(6, "complete", "cyc1", False).tolist() == [[1, 0], [2, 1], [3, 2], [4, 3], [5, 0], [5, 4]]
    assert scene_graph_pairs(0).shape == (0, 2) and scene_graph_pairs(1).shape == (0, 2)
    for bad in ("star", "", "swin-x", "oneref-9", "swinx"):
        with pytest.raises(ValueError, match="scene"):
            scene_graph_pairs(5, bad)
    with pytest.raises(ValueError, match="prefilter"):
        scene_graph_pairs(5, "complete", "near2")
    with pytest.raises(ValueError, match="prefilter"):
        scene_graph_pairs(5, "complete", "seqx")
    assert M._pair_list("swin-1", 5).tolist() == [[0, 1], [0, 4], [1, 2], [2, 3], [3, 4]]
    assert M._pair_list([], 3).shape == (0, 2) and M._pair_list(torch.tensor([[2, 2], [0, 1], [0, 1]]), 3).tolist() == [[2, 2], [0, 1], [0, 1]]
    for bad in ([(0, 3)], [(-1, 0)], [(0, 1, 2)], [(0.0, 1.0)], [0, 1]):
        with pytest.raises(ValueError, match="pairs"):
            M._pair_list(bad, 3)


def test_chunk_planning_against_a_byte_budget():
    from fast3r_amd import matching as M
    counts, index_bytes = [100, 200, 300, 0], 1000
    pairs = [(0, 1), (1, 0), (1, 2), (2, 2), (0, 1), (3, 0)]
    one = M.plan_chunks(counts, pairs, index_bytes, 1 << 30)
    assert len(one) == 1 and one[0]["directed"] == [(0, 1), (1, 0), (1, 2), (2, 1), (2, 2), (3, 0), (0, 3)]   # each directed pair once
    assert one[0]["rows"] == [(0, 1), (1, 0), (2, 3), (4, 4), (0, 1), (5, 6)] and one[0]["queries"] == 100 + 200 + 200 + 300 + 300 + 0 + 100
    assert one[0]["bytes"] == index_bytes + 12 * one[0]["queries"] and (one[0]["start"], one[0]["stop"]) == (0, 6)
    tight = index_bytes + 12 * 500                                             # the largest single pair, (1, 2), exactly
    chunks = M.plan_chunks(counts, pairs, index_bytes, tight)
    assert len(chunks) >= 3 and [(c["start"], c["stop"]) for c in chunks][0][0] == 0 and chunks[-1]["stop"] == 6
    assert all(a["stop"] == b["start"] for a, b in zip(chunks, chunks[1:])) and all(c["bytes"] <= tight for c in chunks)
    assert all(c["bytes"] == index_bytes + 12 * sum(counts[a] for a, _ in c["directed"]) for c in chunks)
    with pytest.raises(ValueError, match="subsample"):
        M.plan_chunks(counts, pairs, index_bytes, tight - 1)
    assert M.plan_chunks(counts, [], index_bytes, 10) == []
    # a chunk also ends where one launch ends: directed queries and tiles of the second views
    by_queries = M.plan_chunks(counts, pairs, index_bytes, 1 << 30, max_queries=600)
    assert len(by_queries) >= 3 and all(c["queries"] <= 600 for c in by_queries) and by_queries[-1]["stop"] == 6
    by_tiles = M.plan_chunks(counts, pairs, index_bytes, 1 << 30, max_tiles=2)
    assert [c["tiles"] for c in by_tiles] == [2, 2, 2] and [(c["start"], c["stop"]) for c in by_tiles] == [(0, 2), (2, 4), (4, 6)]
    assert one[0]["tiles"] == 6 and M.MAX_CHUNK_QUERIES == (1 << 31) - 1 and M.MAX_CHUNK_TILES == (1 << 21) - 1


def test_match_views_refuses_bad_arguments_before_any_launch():
    import fast3r_amd
    p = [{"pts3d_in_other_view": torch.zeros(1, 4, 5, 3), "conf": torch.ones(1, 4, 5)} for _ in range(2)]
    for kw, exc, word in (({"subsample": 0}, ValueError, "subsample"), ({"subsample": 1.5}, ValueError, "subsample"),
                          ({"min_conf_thr_percentile": 101}, ValueError, "percentile"), ({"pairs": "ring"}, ValueError, "scene graph"),
                          ({"pairs": [(0, 2)]}, ValueError, "pairs"), ({"masks": [None]}, ValueError, "masks"),
                          ({"pts3d_key": "pts3d_local"}, KeyError, "pts3d_local")):
        with pytest.raises(exc, match=word):
            fast3r_amd.match_views(p, **kw)
    with pytest.raises(ValueError, match="one view"):
        fast3r_amd.match_views([])
    with pytest.raises(ValueError, match="preds"):
        fast3r_amd.match_views({"views": []})
    with pytest.raises(ValueError, match=r"\(n, 3\)"):
        fast3r_amd.find_reciprocal_matches(torch.zeros(4, 2), torch.zeros(4, 3))
    assert hasattr(fast3r_amd.MultiViewDUSt3RLitModule, "match_views") and fast3r_amd.ViewMatches is fast3r_amd.matching.ViewMatches


def test_library_side(built_lib):
    from fast3r_amd import _lib, post_ops
    new = {"f3r_match_index_bytes": 2, "f3r_match_workspace_bytes": 2, "f3r_match_index": 9, "f3r_match_search": 11, "f3r_match_count": 16,
           "f3r_match_write": 21}
    for name, arity in new.items():
        assert len(_lib.SYMBOLS[name][1]) == arity and _lib.if_present(name) and _lib.entry(name) is getattr(built_lib, name)
    assert built_lib.f3r_version() == 430                                     # unchanged
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_match ] && extra="-ffp-contract=off"' in build and "obj/f3r_match.o" in build
    # sizes need no GPU: 256 header bytes, the unit table, then per view a 256-byte-aligned slice of 512 + 36 m bytes
    assert post_ops.match_index_bytes([0]) == 256 + 256 + 512 and post_ops.match_index_bytes([3, 100]) == 256 + 256 + 768 + 4352
    assert post_ops.match_index_bytes([1] * 65537) == 0 and post_ops.match_index_bytes([1 << 31]) == 0 and post_ops.match_index_bytes([-1]) == 0
    assert built_lib.f3r_match_workspace_bytes(1 << 32, 1) == 0 and built_lib.f3r_match_workspace_bytes(10, 0) == 0
    with pytest.raises(_lib.F3RError):
        post_ops.match_index(torch.zeros(4, 3), [4])                          # a CPU tensor: no fallback
