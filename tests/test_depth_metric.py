"""Multi-view depth metrics, the parts that need no GPU: the float64 restatement (tests/depth_ref.py) against hand-computed cases and against
torch.quantile, the case recipes (tests/depth_cases.py) against deliberately wrong readings of the definitions, the refusals of the Python
layer, and the library side (symbols, presence gate, build flag, argument errors)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import depth_cases as C
import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"f3r_depth_workspace_bytes": 5, "f3r_depth_medians": 10, "f3r_depth_errors": 15, "f3r_depth_sparsify": 17}


# ------------------------------------------------------------------------------------------------------------------- the restatement
def test_two_pixels_by_hand():
    r = C.reference("even_two")[0]
    assert r["n_valid"] == 2 and r["median_gt"] == 1.5 and r["median_pred"] == 3.0 and r["scale"] == 0.5
    assert r["absrel"] == 0.0 and r["rmse"] == 0.0 and r["inliers"] == [100.0] and r["ause"] == 0.0
    assert r["s"] == [0.0] * 100 and r["o"] == [0.0] * 100
    assert r["order_conf"].tolist() == [1, 0] and r["order_err"].tolist() == [0, 1]       # ascending confidence; equal errors in pixel order


def test_the_ratio_is_compared_strictly():
    on = R.segment(C.f32([1.25]), C.f32([1.0]), alignment="none", thresholds=(1.25,))
    assert on["ratios"].tolist() == [1.25] and on["counts"] == [0] and on["inliers"] == [0.0]
    below = R.segment(np.nextafter(np.float32(1.25), np.float32(0), dtype=np.float32).reshape(1), C.f32([1.0]), alignment="none", thresholds=(1.25,))
    assert below["ratios"][0] < 1.25 and below["counts"] == [1] and below["inliers"] == [100.0]
    assert on["absrel"] == 100.0 * (0.25 / 1.25) and on["rmse"] == 0.25


def test_sums_by_hand():
    g, p = C.f32([1, 2, 4, 0, -1]), C.f32([1.5, 2, 2, 9, 9])
    r = R.segment(g, p, C.f32([.5, .4, .3, .2, .1]), alignment="none", thresholds=(1.5, 2.5), uncertainty=True, n_bins=3)
    assert r["n_valid"] == 3 and r["median_gt"] == 2.0 and r["median_pred"] == 2.0 and r["scale"] == 1.0
    assert r["absrel"] == 100.0 * (0.5 + 0.0 + 0.5) / 3 and r["rmse"] == math.sqrt((0.25 + 0 + 4) / 3)
    assert r["counts"] == [1, 3]                                                          # ratios 1.5 (not below 1.5), 1, 2
    assert r["order_conf"].tolist() == [2, 1, 0] and r["order_err"].tolist() == [0, 2, 1]  # errors .5, 0, .5: the tie in pixel order
    assert r["s"] == [1.0 / 3, 0.25, 0.5] and r["o"] == [1.0 / 3, 0.25, 0.0]
    d = [0.0, 0.0, 0.5 / (1.0 / 3)]
    assert r["ause"] == pytest.approx((d[0] + d[1]) / 6 + (d[1] + d[2]) / 6, rel=1e-15)


def test_empty_segment_is_nan():
    r = R.segment(C.f32([0, -1]), C.f32([1, 1]), C.f32([1, 1]), uncertainty=True, n_bins=4)
    assert r["n_valid"] == 0 and all(math.isnan(r[k]) for k in ("scale", "absrel", "rmse", "ause", "median_gt")) and math.isnan(r["s"][0])


def test_negative_scale_gives_the_metrics_of_the_mirror():
    neg, pos = C.reference("negative_p")[0], C.reference("positive_p")[0]
    assert neg["scale"] == -pos["scale"] < 0
    for k in ("n_valid", "absrel", "rmse", "inliers", "s", "o", "ause"):
        assert neg[k] == pos[k], k


def test_median_of_zero_predictions_leaves_the_scale_at_one():
    r = C.reference("med_p_zero")[0]
    assert r["median_pred"] == 0.0 and r["scale"] == 1.0 and r["n_valid"] == 65


def test_quantile_rule_is_torch_quantile():
    for n in (1, 2, 3, 64, 1025):
        conf = C._rng(n, 77).uniform(0, 1, n).astype(np.float32)
        conf[: n // 3] = conf[0]
        for pct in (1, 15, 50, 85, 99.5, 100):
            q = pct / 100.0
            assert np.float32(R.quantile_rule(conf, q)).tobytes() == torch.quantile(torch.from_numpy(conf), q).numpy().tobytes(), (n, pct)
    c = C.case("pct50")["segs"][0]["conf"]
    assert R.quantile_rule(c, 0.5) == np.float32(0.5) and int((c == np.float32(0.5)).sum()) == 10
    assert R.quantile_rule(c, 1.0) == np.float32(0.9) and int((c == np.float32(0.9)).sum()) == 10
    assert [C.reference("pct50")[0]["thr"], C.reference("pct100")[0]["thr"]] == [0.5, float(np.float32(0.9))]


def test_keys_order_floats_as_stated():
    v = np.array([0xffc00000, 0xff800000, 0xbf800000, 0x80000000, 0x00000000, 0x3f800000, 0x7f800000, 0x7fc00000], np.uint32).view(np.float32)
    k = R.fkey(v).astype(np.int64)
    assert (np.diff(k) > 0).all()                      # negative NaN, -inf, -1, -0.0, +0.0, 1, +inf, NaN


# ------------------------------------------------------------------------------------------------------------------- the recipes
def test_recipes_hold_what_they_were_built_for():
    assert [s["g"].size for s in C.case("shapes")["segs"]] == [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4160]
    assert [r["n_valid"] for r in C.reference("valid_counts")] == [0, 1, 2, 3, 64]
    big = C.case("shapes")["segs"][-1]
    assert (big["g"] == 0).any() and (big["g"] < 0).any() and np.isinf(big["g"]).any() and np.isnan(big["g"]).any()
    assert np.isnan(big["p"]).any() and (big["p"] == 0).any() and (big["p"] < 0).any()
    refs = C.reference("shapes")
    assert any(0 < r["n_valid"] < 100 for r in refs) and any(r["n_valid"] > 100 and r["n_valid"] % 100 for r in refs)
    cl = C.reference("clip")[0]
    seg = C.case("clip")["segs"][0]
    sp = cl["scale"] * seg["p"][R.valid_pixels(seg["g"], seg["p"], None, seg["mask"])].astype(np.float64)
    assert (sp < 1.0).any() and (sp > 3.0).any() and ((sp > 1.0) & (sp < 3.0)).any()
    sp_c = C.case("conf_special")["segs"][0]["conf"]
    assert np.isnan(sp_c).sum() == 6 and (sp_c.view(np.uint32) == 0x80000000).sum() == 3 and np.isinf(sp_c).sum() == 4
    tb, ref = C.case("ties_bin_cut")["segs"][0], C.reference("ties_bin_cut")[0]
    rank = np.flatnonzero(tb["conf"][ref["order_conf"]] == np.float32(0.5))
    assert ref["n_valid"] == 1024 and rank.size == 100 and rank[0] < 1024 * 5 // 10 < rank[-1]
    assert C.reference("four_thresholds")[0]["counts"] != C.reference("four_thresholds", "le_threshold")[0]["counts"]
    assert C.reference("k1")[0]["ause"] == 0.0 and len(C.reference("k1")[0]["s"]) == 1


@pytest.mark.parametrize("name", C.CASES)
def test_ratios_keep_away_from_the_thresholds(name):
    c = C.case(name)
    for i, r in enumerate(C.reference(name)):
        pix = np.flatnonzero(R.valid_pixels(c["segs"][i]["g"], c["segs"][i]["p"], c["segs"][i]["conf"], c["segs"][i]["mask"],
                                            None if np.isnan(r["thr"]) else np.float32(r["thr"])))
        assert pix.size == r["n_valid"]
        for t in c["kw"]["thresholds"]:
            for j, ratio in zip(pix, r["ratios"]):
                if (i, int(j)) in C.on_threshold(c):
                    continue
                assert not abs(ratio - t) < 1e-9 * t, (name, i, j, ratio, t)
    if name == "four_thresholds":
        r = C.reference(name)[0]["ratios"]
        assert r[:4].tolist() == list(C.THRESHOLDS4) and r[4:8].tolist() == list(C.THRESHOLDS4)


def _differs(a, b):
    for k in ("n_valid", "median_gt", "median_pred", "scale", "counts"):
        if not (a[k] == b[k] or (a[k] != a[k] and b[k] != b[k])):
            return True
    if a["n_valid"] == 0:
        return False
    if "order_conf" in a and (a["order_conf"].tolist() != b["order_conf"].tolist() or a["order_err"].tolist() != b["order_err"].tolist()):
        return True
    n = a["n_valid"]
    pairs = [(a["absrel"], b["absrel"]), (a["rmse"], b["rmse"])] + list(zip(a.get("s", []), b.get("s", []))) + list(zip(a.get("o", []), b.get("o", [])))
    return any(abs(x - y) > R.tolerance(n, x) for x, y in pairs)


@pytest.mark.parametrize("wrong", R.WRONG)
def test_the_cases_discriminate(wrong):
    """each deliberately wrong restatement misses every case listed for it, by more than the tolerance the GPU is held to"""
    for name in C.DISCRIMINATES[wrong]:
        good, bad = C.reference(name), C.reference(name, wrong)
        assert any(_differs(g, b) for g, b in zip(good, bad)), (wrong, name)
    assert not any(_differs(g, b) for g, b in zip(C.reference("shapes"), C.reference("shapes")))


# ------------------------------------------------------------------------------------------------------------------- the Python layer
def test_refusals_of_the_python_layer():
    import fast3r_amd
    from fast3r_amd import _lib
    g, p = torch.ones(1, 4, 5), torch.ones(1, 4, 5, 3)
    views, preds = [{"depthmap": g, "label": ["a/b/0"]}], [{"pts3d_local": p, "conf_local": g, "pts3d_in_other_view": p, "conf": g}]
    with pytest.raises(ValueError, match="same|size"):
        fast3r_amd.depth_metrics([g], [torch.ones(1, 5, 4, 3)])
    with pytest.raises(ValueError, match="alignment"):
        fast3r_amd.depth_metrics([g], [p], alignment="lsq")
    with pytest.raises(ValueError, match="at most 4"):
        fast3r_amd.depth_metrics([g], [p], inlier_thresholds=(1.1, 1.2, 1.3, 1.4, 1.5))
    with pytest.raises(ValueError, match="n_bins"):
        fast3r_amd.depth_metrics([g], [p], [g], eval_uncertainty=True, n_bins=0)
    with pytest.raises(ValueError, match="clip_pred_depth"):
        fast3r_amd.depth_metrics([g], [p], clip_pred_depth=(3.0, 1.0))
    with pytest.raises(ValueError, match="min_conf_thr_percentile"):
        fast3r_amd.depth_metrics([g], [p], [g], min_conf_thr_percentile=101)
    with pytest.raises(ValueError, match="confidence"):
        fast3r_amd.depth_metrics([g], [p], eval_uncertainty=True)
    with pytest.raises(ValueError, match="one entry per view"):
        fast3r_amd.depth_metrics([g], [p, p])
    with pytest.raises(ValueError, match="view 0's camera"):
        fast3r_amd.evaluate_multiview_depth(views * 2, preds * 2, head="global", keyviews=[1])
    with pytest.raises(ValueError, match="build_gt_views"):
        fast3r_amd.evaluate_multiview_depth([{"label": ["a/b/0"]}], preds)
    with pytest.raises(ValueError, match="head"):
        fast3r_amd.evaluate_multiview_depth(views, preds, head="both")
    with pytest.raises(_lib.F3RError, match="ROCm device"):                  # no CPU path
        fast3r_amd.depth_metrics([g], [p])
    if not torch.cuda.is_available():
        with pytest.raises(_lib.F3RError, match="no ROCm device"):
            fast3r_amd.evaluate_multiview_depth(views, preds)


def test_signatures_are_the_stated_ones():
    import inspect
    import fast3r_amd
    from fast3r_amd.multiview_dust3r_module import MultiViewDUSt3RLitModule
    sig = inspect.signature(fast3r_amd.depth_metrics)
    assert [(p.name, p.default) for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD] == [
        ("gt_depths", inspect.Parameter.empty), ("pred", inspect.Parameter.empty), ("confs", None), ("valid_masks", None)]
    assert {p.name: p.default for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY} == dict(
        alignment="median", inlier_thresholds=(1.03,), clip_pred_depth=None, min_conf_thr_percentile=0, eval_uncertainty=False, n_bins=100)
    sig = inspect.signature(fast3r_amd.evaluate_multiview_depth)
    assert {p.name: p.default for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY} == dict(head="local", keyviews=None)
    assert list(inspect.signature(MultiViewDUSt3RLitModule.evaluate_multiview_depth).parameters)[:4] == ["self", "views", "preds", "dataset_name"]
    assert MultiViewDUSt3RLitModule(net=None).depth_metrics_per_epoch == {}


# ------------------------------------------------------------------------------------------------------------------- the library side
def test_new_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    raw = open(os.path.join(ROOT, "include", "f3r.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity, name
        assert _lib.symbol_since(name) == 0 and _lib.if_present(name) and name in _lib.SYMBOL_IF_PRESENT_DEPTH
        assert name not in _lib.SYMBOL_IF_PRESENT and name not in _lib.SYMBOL_IF_PRESENT_MAPS and name not in _lib.SYMBOL_IF_PRESENT_VIEWS
        assert getattr(built_lib, name).argtypes == _lib.SYMBOLS[name][1] and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_IF_PRESENT_DEPTH) == set(NEW_SYMBOLS) and not _lib.if_present("f3r_gemm") and _lib.if_present("f3r_gtview_resample")
    for macro, const in (("F3R_DEPTH_TILE", _lib.DEPTH_TILE), ("F3R_DEPTH_ROW_WORDS", _lib.DEPTH_ROW_WORDS), ("F3R_DEPTH_OUT_WORDS", _lib.DEPTH_OUT_WORDS),
                         ("F3R_DEPTH_MAX_THRESHOLDS", _lib.DEPTH_MAX_THRESHOLDS)):
        assert int(re.search(r"#define %s (\d+)" % macro, raw).group(1)) == const
    assert re.search(r"F3R_DEPTH_ALIGN_NONE = 0, F3R_DEPTH_ALIGN_MEDIAN = 1", raw) and (_lib.F3R_DEPTH_ALIGN_NONE, _lib.F3R_DEPTH_ALIGN_MEDIAN) == (0, 1)
    assert "multi-view depth metrics" in raw.lower() and built_lib.f3r_version() == 430


def test_build_script_carries_the_file_the_flag_and_the_shared_sort():
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_depth ] && extra="-ffp-contract=off"' in build and '"$here"/obj/f3r_depth.o' in build
    assert re.search(r"^for f in .*\bf3r_depth\b.*; do$", build, flags=re.M) and "f3r_sort.h" in build
    csrc = os.path.join(ROOT, "fast3r_amd", "csrc")
    depth, cloud, sort = (open(os.path.join(csrc, f)).read() for f in ("f3r_depth.hip", "f3r_cloud.hip", "f3r_sort.h"))
    for src in (depth, cloud):                         # both users take the LSD passes from the one header
        assert '#include "f3r_sort.h"' in src and "sort_pairs_lsd(" in src and "void sort_scatter_kernel" not in src
    assert "void sort_scatter_kernel" in sort and "void sort_hist_kernel" in sort
    assert "select_kth_key<" in depth and "block_quantile<" in depth and "atomicAdd(&sh_cnt" in depth
    assert not re.search(r"atomicAdd\([^)]*(double|float)", depth)


def test_the_index_builders_share_the_sort_the_sizing_rules_and_the_search():
    """f3r_recon.hip and f3r_match.hip take the LSD passes from f3r_sort.h and the grid-sizing rules from f3r_nn.h; no second copy anywhere"""
    csrc = os.path.join(ROOT, "fast3r_amd", "csrc")
    files = {os.path.relpath(os.path.join(d, f), csrc): open(os.path.join(d, f)).read() for d, _, fs in os.walk(csrc) if os.path.basename(d) != "obj"
             for f in sorted(fs) if f.endswith((".hip", ".h", ".cpp", ".py", ".sh"))}
    for f in ("f3r_recon.hip", "f3r_match.hip"):
        assert '#include "f3r_sort.h"' in files[f] and '#include "f3r_nn.h"' in files[f] and "sort_pairs_lsd(" in files[f], f
    for gone in ("radix_scatter_kernel", "set_grid_dev", "box_volume_dev"):
        assert not [f for f, src in files.items() if gone in src], gone
    for name, home in (("set_grid", "f3r_nn.h"), ("first_ge", "f3r_prims.h"), ("key_bits_of", "f3r_nn.h")):
        defined = [f for f, src in files.items() if re.search(r"^[\w \t]*\b(?:void|double|int|int64_t|bool) %s\(" % name, src, flags=re.M)]
        assert defined == [home], (name, defined)


def test_a_library_without_the_depth_metrics_still_loads(tmp_path, monkeypatch):
    from fast3r_amd import _lib, post_ops
    names = [n for n in _lib.SYMBOLS if n not in _lib.SYMBOL_IF_PRESENT_DEPTH and n not in ("f3r_version", "f3r_sizeof")]
    src, so = tmp_path / "stub.c", tmp_path / "libf3r_hip.so"
    sizes = (ctypes.sizeof(_lib.GemmArgs), ctypes.sizeof(_lib.AttnArgs), ctypes.sizeof(_lib.AttnF32Args))
    src.write_text("int f3r_version(void) { return 430; }\nunsigned long f3r_sizeof(int w) { return w == 0 ? %d : w == 1 ? %d : w == 2 ? %d : 0; }\n"
                   % sizes + "".join("int %s(void) { return 0; }\n" % n for n in names))
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    l = _lib.lib()
    assert _lib.entry("f3r_gtview_unproject") is l.f3r_gtview_unproject and _lib.entry("f3r_maps_colorize") is l.f3r_maps_colorize
    for name in NEW_SYMBOLS:
        with pytest.raises(_lib.F3RError, match=f"does not export {name}: rebuild it"):
            _lib.entry(name)
    plan = {"out": torch.zeros(1, 16, dtype=torch.float64), "n_bins": 0}
    for call in (post_ops.depth_medians, post_ops.depth_errors, post_ops.depth_sparsify):
        with pytest.raises(_lib.F3RError, match="rebuild it"):
            call(plan)


def test_argument_errors_are_codes_before_any_launch(built_lib):
    l, err = built_lib, built_lib.f3r_last_error_string
    P = 0x1000

    def table(n=(5, 2000), **kw):
        rows, base, tiles = [], 0, [0]
        for k in n:
            rows += [P, P, 3, 2, P, P, k, base]
            base += k
            tiles.append(tiles[-1] + (k + 1023) // 1024)
        words = rows + tiles
        for at, v in kw.items():
            words[int(at[1:])] = v
        return (ctypes.c_int64 * len(words))(*words), len(n), tiles[-1]

    def medians(host, S, T, **kw):
        a = dict(table=P, host=host, n_seg=S, n_tiles=T, alignment=1, use_thr=0, q=0.0, out=P, out_ld=16, stream=None)
        a.update(kw)
        return l.f3r_depth_medians(*a.values())

    def errors(host, S, T, **kw):
        a = dict(table=P, host=host, n_seg=S, n_tiles=T, use_thr=0, clip=0, lo=0.0, hi=0.0, thr=(ctypes.c_double * 8)(), n_thr=1, ws=P, ws_bytes=1 << 20,
                 out=P, out_ld=16, stream=None)
        a.update(kw)
        return l.f3r_depth_errors(*a.values())

    def sparsify(host, S, T, **kw):
        a = dict(table=P, host=host, n_seg=S, n_tiles=T, use_thr=0, clip=0, lo=0.0, hi=0.0, n_bins=100, ws=P, ws_bytes=1 << 30, oc=P, oe=P, st=P, out=P,
                 out_ld=216, stream=None)
        a.update(kw)
        return l.f3r_depth_sparsify(*a.values())

    host, S, T = table()
    assert T == 3
    for call in (medians, errors, sparsify):
        assert call(host, S, T, table=None) == -1 and b"null table" in err()
        assert call(None, S, T) == -1 and b"null table" in err()
        assert call(host, S, T, out=None) == -1 and b"null out" in err()
        assert call(host, 0, T) == -1 and b"segments" in err()
        assert call(host, S, T + 1) == -1 and b"tile starts" in err()
        assert call(table(n=(5, 2 ** 31))[0], 2, 1 + 2 ** 21) == -1 and b"2^31 pixels or more" in err()
        assert call(table(n=(0, 7, 7))[0], 3, 3) == -1 and b"fewer than 1" in err()
        assert call(table(w0=0)[0], S, T) == -1 and b"null depth or prediction" in err()
        assert call(table(w2=2)[0], S, T) == -1 and b"neither 1 nor 3" in err()
        assert call(table(w9=P + 2)[0], S, T) == -1 and b"multiple of 4 bytes" in err()
        assert call(table(w15=4)[0], S, T) == -1 and b"pixel base" in err()
        assert call(host, S, T, out_ld=15) == -1 and b"out_ld" in err()
    assert medians(host, S, T, alignment=2) == -1 and b"unknown alignment" in err()
    assert medians(host, S, T, use_thr=1, q=1.5) == -1 and b"outside [0, 1]" in err()
    assert errors(host, S, T, n_thr=5) == -1 and b"5 thresholds; at most 4" in err()
    assert errors(host, S, T, thr=None) == -1 and b"thresholds" in err()
    assert errors(host, S, T, clip=1, lo=2.0, hi=1.0) == -1 and b"not an interval" in err()
    assert errors(host, S, T, clip=1, lo=float("nan"), hi=1.0) == -1 and b"not an interval" in err()
    assert errors(host, S, T, ws=None) == -1 and b"null workspace" in err()
    assert errors(host, S, T, ws_bytes=255) == -1 and b"workspace too small" in err()
    for k in (0, -1, 65537):
        assert sparsify(host, S, T, n_bins=k) == -1 and b"n_bins" in err()
        assert l.f3r_depth_workspace_bytes(S, T, 2005, 1, k) == 0
    assert sparsify(host, S, T, oc=None) == -1 and sparsify(host, S, T, st=None) == -1 and b"null workspace, order or starts" in err()
    assert sparsify(host, S, T, out_ld=215) == -1 and b"out_ld" in err()
    assert sparsify(host, S, T, ws_bytes=1 << 10) == -1 and b"workspace too small" in err()
    big, Sb, Tb = table(n=(2 ** 30, 2 ** 30))
    assert sparsify(big, Sb, Tb) == -1 and b"fewer than 2^31" in err() and l.f3r_depth_workspace_bytes(Sb, Tb, 2 ** 31, 1, 100) == 0
    # sizes: 48 bytes per tile without the curves; with them of the order of the pixel count
    assert l.f3r_depth_workspace_bytes(S, T, 2005, 0, 0) == 256 and l.f3r_depth_workspace_bytes(320, 320 * 256, 320 * 2 ** 18, 0, 0) == 320 * 256 * 48
    assert l.f3r_depth_workspace_bytes(320, 320 * 256, 320 * 2 ** 18, 1, 100) > 32 * 320 * 2 ** 18
    assert l.f3r_depth_workspace_bytes(0, 1, 5, 0, 0) == 0 and l.f3r_depth_workspace_bytes(2, 1, 5, 0, 0) == 0
