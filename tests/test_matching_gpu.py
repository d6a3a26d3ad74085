"""View matching on a real MI355X against the numpy restatement (tests/match_ref.py): masks, indices, counts, pixel coordinates and their
order exactly; `dist` bit-equal to the square root of the restatement's fp64 squared distance.  The cases are tests/match_cases.py's."""
import ctypes

import numpy as np
import pytest
import torch

import match_cases as C
import match_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
_REFERENCES = {}


def preds_of(case):
    confs = case.get("confs") or [None] * len(case["pts"])
    out = []
    for p, c in zip(case["pts"], confs):
        d = {"pts3d_in_other_view": torch.from_numpy(np.ascontiguousarray(p))[None].to(DEV)}
        if c is not None:
            d["conf"] = torch.from_numpy(np.ascontiguousarray(c))[None].to(DEV)
        out.append(d)
    return out


def run(case, **kw):
    import fast3r_amd
    masks = None if case.get("masks") is None else [None if m is None else torch.from_numpy(m).to(DEV) for m in case["masks"]]
    return fast3r_amd.match_views(preds_of(case), pairs=case["pairs"], min_conf_thr_percentile=case.get("pct", 0), masks=masks,
                                  subsample=case.get("subsample", 1), **kw)


def reference(name, case):
    """the restatement of a case, computed once and shared"""
    if name not in _REFERENCES:
        _REFERENCES[name] = R.match_views(case["pts"], case.get("confs"), case.get("masks"), case["pairs"], case.get("pct", 0), case.get("subsample", 1))
    return _REFERENCES[name]


def host(vm):
    return {k: getattr(vm, k).cpu().numpy() for k in ("pairs", "offsets", "xy_i", "xy_j", "dist", "counts")}


def assert_same(got, ref, what):
    assert got["pairs"].dtype == np.int64 and np.array_equal(got["pairs"], ref["pairs"]), what
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref["counts"]), (what, got["counts"], ref["counts"])
    assert got["offsets"].dtype == np.int64 and np.array_equal(got["offsets"], ref["offsets"]), what
    assert got["xy_i"].dtype == np.int32 and got["xy_i"].shape == ref["xy_i"].shape and np.array_equal(got["xy_i"], ref["xy_i"]), what
    assert got["xy_j"].dtype == np.int32 and np.array_equal(got["xy_j"], ref["xy_j"]), what
    assert got["dist"].dtype == np.float64 and got["dist"].tobytes() == np.sqrt(ref["d2"]).tobytes(), what


def check(name, case, **kw):
    vm = run(case, **kw)
    got, ref = host(vm), reference(name, case)
    print(f"{name}: {len(case['pts'])} views, candidates {ref['n_candidates'][:12]}, {len(ref['pairs'])} pairs, {int(ref['counts'].sum())} matches, "
          f"{vm.n_chunks} chunk(s)")
    assert_same(got, ref, name)
    return vm, got, ref


# ------------------------------------------------------------------------------------------------------------------- golden
@pytest.fixture(scope="module")
def golden():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matches_cases.npz")) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("name,a,b", [("patch01", "patch0", "patch1"), ("patch12", "patch1", "patch2"), ("patch20", "patch2", "patch0"),
                                      ("clouds", "cloud0", "cloud1")])
def test_find_reciprocal_matches_reproduces_the_reference(built_lib, golden, name, a, b):
    import fast3r_amd
    P1, P2 = (torch.from_numpy(golden[k].reshape(-1, 3)).to(DEV) for k in (a, b))
    rec, nn2, num = fast3r_amd.find_reciprocal_matches(P1, P2)
    assert rec.dtype == torch.bool and nn2.dtype == torch.int64 and isinstance(num, int) and rec.is_cuda and nn2.is_cuda
    assert np.array_equal(rec.cpu().numpy(), golden[f"{name}_reciprocal_in_P2"]) and np.array_equal(nn2.cpu().numpy(), golden[f"{name}_nn2_in_P1"])
    assert num == int(golden[f"{name}_num_matches"])
    rec64, nn64, num64 = fast3r_amd.find_reciprocal_matches(P1.double(), P2.cpu().numpy())  # other float types and hosts are converted
    assert torch.equal(rec64, rec) and torch.equal(nn64, nn2) and num64 == num


def test_match_views_reproduces_the_reference_on_the_golden_patches(built_lib, golden):
    case = {"pts": [golden[f"patch{k}"] for k in range(3)], "pairs": [(0, 1), (1, 2), (2, 0)]}
    vm, got, _ = check("golden_patches", case)
    for p, name in enumerate(("patch01", "patch12", "patch20")):
        i, j = case["pairs"][p]
        rec, nn2 = golden[f"{name}_reciprocal_in_P2"], golden[f"{name}_nn2_in_P1"]
        Wi, Wj = case["pts"][i].shape[1], case["pts"][j].shape[1]
        pj, pi = np.flatnonzero(rec), nn2[rec]
        xi, xj, _ = vm.pair(p)
        assert int(got["counts"][p]) == int(golden[f"{name}_num_matches"])
        assert np.array_equal(xj.cpu().numpy(), np.stack([pj % Wj, pj // Wj], 1)) and np.array_equal(xi.cpu().numpy(), np.stack([pi % Wi, pi // Wi], 1))


# ------------------------------------------------------------------------------------------------------------------- sizes
def test_candidate_counts_across_the_wave_and_the_sort_tile(built_lib):
    """0, 1, 2, 63, 64, 65, 2047, 2048, 2049 and 5000 candidates in views of ten different sizes, every pair"""
    _, _, ref = check("counts", C.counts_case())
    assert ref["n_candidates"] == list(C.COUNTS) and ref["counts"].max() > 100 and not ref["counts"][(ref["pairs"] == 0).any(1)].any()  # pairs with the empty view


def test_per_view_index_bytes_vs_numpy_restatement(built_lib):
    """The per-view indexes f3r_match_index writes, not the matches they give: three views of 0, 65 and 2049 candidates (an empty slice, one
    past a wave, one past a sort tile); each slice's records and dense cell starts equal recon_ref.check_nn_index's numpy restatement from
    that view's own header.  A slice starts 256 bytes + the (V + 1)-word unit table (rounded to 256) + 256 x its scanned unit count in."""
    import recon_ref
    from fast3r_amd import post_ops
    counts = [0, 65, 2049]
    pts = np.concatenate([recon_ref.make_cloud("uniform", 65, 21), recon_ref.make_cloud("surface", 2049, 22)])
    raw = post_ops.match_index(torch.from_numpy(pts).to(DEV), counts)["index"].cpu().numpy()
    assert raw[:4].view(np.uint32)[0] == 0                                      # no view with a NaN / inf coordinate
    units = raw[256:256 + 4 * (len(counts) + 1)].view(np.uint32)
    assert units.tolist() == np.concatenate([[0], np.cumsum([(512 + 36 * m + 255) // 256 for m in counts])]).tolist()
    seg = np.concatenate([[0], np.cumsum(counts)])
    for v, m in enumerate(counts):
        H = recon_ref.check_nn_index(raw[512 + 256 * int(units[v]):512 + 256 * int(units[v + 1])], pts[seg[v]:seg[v + 1]], stored_keys=False)
        print(f"view {v}: {m} candidates, {H['ncells']} cells, {H['occupied']} occupied")
        assert H["ngrid"] == 1 and H["dense"] == 1 and 1 <= H["ncells"] <= 4 * m + 63


def test_one_view_matches_itself(built_lib):
    case = C.views_case(1, 12, 15, [(0, 0)])
    _, got, _ = check("one_view", case)
    assert got["counts"].tolist() == [12 * 15] and np.array_equal(got["xy_i"], got["xy_j"]) and not got["dist"].any()


@pytest.mark.parametrize("n", [2, 5])
def test_some_views(built_lib, n):
    check(f"views{n}", C.views_case(n))


def test_257_views_of_three_points(built_lib):
    """the view number crosses an 8-bit digit of the (view, cell) sort key"""
    _, _, ref = check("views257", C.many_views_case())
    assert len(ref["pairs"]) == 2 * 257 and ref["counts"].sum() > 257


# ------------------------------------------------------------------------------------------------------------------- pair lists
def test_no_pairs(built_lib):
    _, got, _ = check("no_pairs", dict(C.views_case(3), pairs=[]))
    assert got["pairs"].shape == (0, 2) and got["offsets"].tolist() == [0] and got["xy_i"].shape == (0, 2) and got["dist"].shape == (0,)


def test_both_directions_are_transposes_and_repeats_repeat(built_lib):
    vm, got, _ = check("directions", dict(C.views_case(3), pairs=[(0, 1), (1, 0), (0, 1), (2, 2), (1, 0)]))
    o = got["offsets"]
    assert got["counts"][0] == got["counts"][1] == got["counts"][2] == got["counts"][4] > 0
    fwd = np.concatenate([got["xy_i"][o[0]:o[1]], got["xy_j"][o[0]:o[1]], got["dist"][o[0]:o[1], None].view(np.int64).astype(np.int64)], 1)
    bwd = np.concatenate([got["xy_j"][o[1]:o[2]], got["xy_i"][o[1]:o[2]], got["dist"][o[1]:o[2], None].view(np.int64).astype(np.int64)], 1)
    assert sorted(map(tuple, fwd.tolist())) == sorted(map(tuple, bwd.tolist()))      # the same matches, each as its transpose
    for a, b in ((0, 2), (1, 4)):                                                      # a repeated pair repeats its result
        assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(vm.pair(a), vm.pair(b)))


@pytest.mark.parametrize("graph", C.GRAPHS)
def test_every_graph_string_at_five_views(built_lib, graph):
    import fast3r_amd
    _, got, _ = check(f"graph_{graph}", C.views_case(5, 8, 9, graph))
    assert np.array_equal(got["pairs"], fast3r_amd.scene_graph_pairs(5, graph, symmetrize=False)) and len(got["pairs"]) >= 4


# ------------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("name", ["identical", "plane", "line", "disjoint", "outliers", "duplicates"])
def test_degenerate_geometry(built_lib, name):
    _, got, ref = check(f"degenerate_{name}", C.degenerate_cases()[name])
    if name == "identical":  # every point of a one-point cloud is at distance 0 of the others' first: one mutual match per pair of such views
        assert got["counts"].tolist()[2:] == [1, 1]
    if name == "disjoint":
        assert got["counts"][0] == got["counts"][1] >= 1  # far apart: the closest pair of all is mutual


# ------------------------------------------------------------------------------------------------------------------- candidates
@pytest.mark.parametrize("name", ["subsample1", "subsample2", "subsample3", "shared_threshold", "percentile", "nan_conf", "nan_conf_pct0", "mask",
                                  "one_pixel"])
def test_candidate_rule(built_lib, name):
    _, got, ref = check(f"candidates_{name}", C.candidate_cases()[name])
    if name.startswith("nan_conf"):
        assert ref["n_candidates"][1] == 0 and got["counts"][[0, 2]].tolist() == [0, 0]  # pairs (1, 0) and (2, 1): the NaN view keeps nothing
    if name.startswith("subsample"):
        s = int(name[-1])
        assert (got["xy_i"] % s == 0).all() and (got["xy_j"] % s == 0).all()


# ------------------------------------------------------------------------------------------------------------------- chunks
def test_chunked_run_is_bit_equal(built_lib):
    from fast3r_amd import matching as M, post_ops
    case = C.chunk_case()
    one, got_one, ref = check("chunks", case)
    counts = ref["n_candidates"]
    index_bytes = post_ops.match_index_bytes(counts)
    budget = index_bytes + 12 * 4 * 600                                         # two pairs of 600-point views at a time
    assert len(M.plan_chunks(counts, ref["pairs"], index_bytes, budget)) >= 3 and one.n_chunks == 1
    many, got_many, _ = check("chunks", case, max_workspace_bytes=budget)
    assert many.n_chunks >= 3 and many.workspace_bytes <= budget
    for k in got_one:
        assert got_one[k].tobytes() == got_many[k].tobytes(), k
    with pytest.raises(ValueError, match="subsample"):
        run(case, max_workspace_bytes=index_bytes + 12 * 1200 - 1)              # below one pair


# ------------------------------------------------------------------------------------------------------------------- errors, determinism
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_candidates_raise_and_masked_ones_do_not(built_lib, bad):
    import fast3r_amd
    case = C.views_case(3, 9, 11)
    case["pts"][1][4, 5, 2] = bad
    with pytest.raises(ValueError, match="NaN or inf"):
        run(case)
    with pytest.raises(ValueError, match="NaN or inf"):
        fast3r_amd.find_reciprocal_matches(torch.from_numpy(case["pts"][0].reshape(-1, 3)).to(DEV), torch.from_numpy(case["pts"][1].reshape(-1, 3)).to(DEV))
    mask = np.ones((9, 11), bool)
    mask[4, 5] = False
    case["masks"] = [None, mask, None]
    clean = {"pts": [p.copy() for p in case["pts"]], "masks": case["masks"], "pairs": case["pairs"]}
    clean["pts"][1][4, 5, 2] = 0.0                                               # the restatement of the same call without the masked value
    assert_same(host(run(case)), R.match_views(clean["pts"], None, clean["masks"], clean["pairs"]), "masked non-finite")


def test_two_runs_give_the_same_bits(built_lib):
    case = C.counts_case()
    a, b = host(run(case)), host(run(case))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_covisibility(built_lib):
    vm, got, ref = check("covis", dict(C.views_case(4), pairs=[(0, 1), (1, 0), (2, 1), (3, 3), (0, 3)]))
    assert np.array_equal(vm.covisibility().cpu().numpy(), R.covisibility(ref, 4)) and vm.covisibility().dtype == torch.int64
    assert np.array_equal(vm.covisibility(n_views=6).cpu().numpy()[:4, :4], R.covisibility(ref, 4)) and vm.covisibility(6).shape == (6, 6)
    d = np.sort(got["dist"])
    cut = float(d[len(d) // 2])
    want = R.covisibility(ref, 4, cut)
    assert np.array_equal(vm.covisibility(max_dist=cut).cpu().numpy(), want) and 0 < want.sum() < R.covisibility(ref, 4).sum()


# ------------------------------------------------------------------------------------------------------------------- hostile arguments
def test_hostile_argument_tuples_return_the_error_code(built_lib):
    """null, misaligned, too small, over the limits: F3R_ERR_ARG (-1) before any launch.  Every buffer handed over is real and large enough
    for the sizes named, so nothing here depends on a refusal to stay inside its memory."""
    i64, i32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    L = built_lib
    seg_h = np.array([0, 4, 10], np.int64)
    seg_p = seg_h.ctypes.data_as(i64)
    V, total = 2, 10
    nb, wb = L.f3r_match_index_bytes(seg_p, V), L.f3r_match_workspace_bytes(total, V)
    assert nb > 0 and wb > 0
    pts = torch.zeros((total, 3), device=DEV)
    seg = torch.from_numpy(seg_h).to(DEV)
    index = torch.zeros(nb + 512, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(wb + 512, dtype=torch.uint8, device=DEV)
    assert index.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
    ok = [pts.data_ptr(), seg.data_ptr(), seg_p, V, index.data_ptr(), nb, ws.data_ptr(), wb, None]

    def index_call(**change):
        names = ["pts", "seg", "seg_host", "V", "index", "index_bytes", "ws", "ws_bytes", "stream"]
        a = list(ok)
        for k, v in change.items():
            a[names.index(k)] = v
        return L.f3r_match_index(*a)

    bad_seg = np.array([0, 6, 4], np.int64)
    big_seg = np.array([0, 1 << 31, 1 << 31], np.int64)
    many = np.zeros(65538, np.int64)
    for change in ({"pts": None}, {"seg": None}, {"seg_host": None}, {"index": None}, {"ws": None}, {"V": 0}, {"V": -1},
                   {"V": 65537, "seg_host": many.ctypes.data_as(i64)}, {"seg_host": bad_seg.ctypes.data_as(i64)}, {"seg_host": big_seg.ctypes.data_as(i64)},
                   {"index": index.data_ptr() + 16}, {"ws": ws.data_ptr() + 64}, {"seg": seg.data_ptr() + 4}, {"pts": pts.data_ptr() + 2},
                   {"index_bytes": nb - 1}, {"ws_bytes": wb - 1}, {"index_bytes": 0}):
        assert index_call(**change) == -1, change
        assert b"f3r_match_index" in L.f3r_last_error_string()
    assert L.f3r_match_index_bytes(None, 2) == 0 and L.f3r_match_index_bytes(bad_seg.ctypes.data_as(i64), 2) == 0
    assert L.f3r_match_workspace_bytes(-1, 2) == 0 and L.f3r_match_workspace_bytes(10, 65537) == 0

    dir_h = np.array([0, 1, 1, 0], np.int32)
    qoff_h = np.array([0, 4, 10], np.int64)
    directed, qoff = torch.from_numpy(dir_h).to(DEV), torch.from_numpy(qoff_h).to(DEV)
    nn_idx, nn_dist = torch.zeros(16, dtype=torch.int32, device=DEV), torch.zeros(16, dtype=torch.float64, device=DEV)
    s_ok = [index.data_ptr(), seg_p, V, directed.data_ptr(), dir_h.ctypes.data_as(i32), qoff.data_ptr(), qoff_h.ctypes.data_as(i64), 2, nn_idx.data_ptr(),
            nn_dist.data_ptr(), None]
    s_names = ["index", "seg_host", "V", "directed", "directed_host", "qoff", "qoff_host", "D", "nn_idx", "nn_dist", "stream"]
    out_of_views = np.array([0, 2, 1, 0], np.int32)
    wrong_qoff = np.array([0, 5, 10], np.int64)
    for change in ({"index": None}, {"seg_host": None}, {"qoff_host": None}, {"directed": None}, {"directed_host": None}, {"qoff": None},
                   {"nn_idx": None}, {"nn_dist": None}, {"D": -1}, {"V": 0}, {"directed_host": out_of_views.ctypes.data_as(i32)},
                   {"qoff_host": wrong_qoff.ctypes.data_as(i64)}, {"index": index.data_ptr() + 16}, {"qoff": qoff.data_ptr() + 4},
                   {"nn_dist": nn_dist.data_ptr() + 4}, {"nn_idx": nn_idx.data_ptr() + 2}):
        a = list(s_ok)
        for k, v in change.items():
            a[s_names.index(k)] = v
        assert L.f3r_match_search(*a) == -1, change
        assert b"f3r_match_search" in L.f3r_last_error_string()

    pair_h = np.array([0, 1, 0, 1], np.int32)
    toff_h = np.array([0, 1], np.int64)
    pairs, toff = torch.from_numpy(pair_h).to(DEV), torch.from_numpy(toff_h).to(DEV)
    tile_counts, offsets = torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.int64, device=DEV)
    c_ok = [index.data_ptr(), seg.data_ptr(), seg_p, V, pairs.data_ptr(), pair_h.ctypes.data_as(i32), toff.data_ptr(), toff_h.ctypes.data_as(i64), 1,
            qoff.data_ptr(), qoff_h.ctypes.data_as(i64), 2, nn_idx.data_ptr(), tile_counts.data_ptr(), offsets.data_ptr(), None]
    c_names = ["index", "seg", "seg_host", "V", "pairs", "pairs_host", "tile_off", "tile_off_host", "P", "qoff", "qoff_host", "D", "nn_idx", "tile_counts",
               "offsets", "stream"]
    bad_rows = np.array([0, 1, 0, 2], np.int32)
    bad_view = np.array([0, 3, 0, 1], np.int32)
    swapped = np.array([0, 1, 1, 0], np.int32)          # the forward row has view 1's size
    bad_tiles = np.array([0, 2], np.int64)
    for change in ({"index": None}, {"seg": None}, {"seg_host": None}, {"pairs": None}, {"pairs_host": None}, {"tile_off": None}, {"tile_off_host": None},
                   {"qoff": None}, {"qoff_host": None}, {"nn_idx": None}, {"tile_counts": None}, {"offsets": None}, {"P": -1}, {"D": -1},
                   {"pairs_host": bad_rows.ctypes.data_as(i32)}, {"pairs_host": bad_view.ctypes.data_as(i32)}, {"pairs_host": swapped.ctypes.data_as(i32)},
                   {"tile_off_host": bad_tiles.ctypes.data_as(i64)}, {"offsets": offsets.data_ptr() + 4}, {"tile_counts": tile_counts.data_ptr() + 2}):
        a = list(c_ok)
        for k, v in change.items():
            a[c_names.index(k)] = v
        assert L.f3r_match_count(*a) == -1, change
        assert b"f3r_match_count" in L.f3r_last_error_string()

    pix, widths = torch.zeros(total, dtype=torch.int32, device=DEV), torch.ones(V, dtype=torch.int32, device=DEV)
    xy_i, xy_j = torch.zeros((8, 2), dtype=torch.int32, device=DEV), torch.zeros((8, 2), dtype=torch.int32, device=DEV)
    dist = torch.zeros(8, dtype=torch.float64, device=DEV)
    w_ok = [seg.data_ptr(), seg_p, V, pairs.data_ptr(), pair_h.ctypes.data_as(i32), toff.data_ptr(), toff_h.ctypes.data_as(i64), 1, qoff.data_ptr(),
            qoff_h.ctypes.data_as(i64), 2, nn_idx.data_ptr(), nn_dist.data_ptr(), tile_counts.data_ptr(), pix.data_ptr(), widths.data_ptr(), xy_i.data_ptr(),
            xy_j.data_ptr(), dist.data_ptr(), 4, None]
    w_names = ["seg", "seg_host", "V", "pairs", "pairs_host", "tile_off", "tile_off_host", "P", "qoff", "qoff_host", "D", "nn_idx", "nn_dist", "tile_counts",
               "pix", "widths", "xy_i", "xy_j", "dist", "M", "stream"]
    for change in ({"seg": None}, {"seg_host": None}, {"pairs": None}, {"tile_off": None}, {"qoff": None}, {"nn_idx": None}, {"nn_dist": None},
                   {"tile_counts": None}, {"pix": None}, {"widths": None}, {"xy_i": None}, {"xy_j": None}, {"dist": None}, {"M": -1}, {"M": 1 << 32},
                   {"pairs_host": bad_view.ctypes.data_as(i32)}, {"dist": dist.data_ptr() + 4}, {"xy_i": xy_i.data_ptr() + 2}):
        a = list(w_ok)
        for k, v in change.items():
            a[w_names.index(k)] = v
        assert L.f3r_match_write(*a) == -1, change
        assert b"f3r_match_write" in L.f3r_last_error_string()
    torch.cuda.synchronize()
