"""Point-cloud export, the parts that need no GPU: the signature is the notebook's, the numpy restatement (tests/cloud_ref.py) checks
itself by brute force, the recipes (tests/cloud_cases.py) hold the edge cases they promise, the host arithmetic of the voxel grid, and
the library side: symbols, sizing functions, the version gate of the later entry points, argument errors before anything is launched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import cloud_cases as C
import cloud_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"f3r_cloud_combine_count": 6, "f3r_cloud_combine_write": 9, "f3r_cloud_bounds": 4, "f3r_cloud_voxel_workspace_bytes": 1,
               "f3r_cloud_voxel_sort": 9, "f3r_cloud_voxel_sums": 10, "f3r_cloud_fps_workspace_bytes": 1, "f3r_cloud_fps": 9,
               "f3r_cloud_mark": 5, "f3r_cloud_gather": 9}


def test_signature_is_the_notebooks():
    import fast3r_amd
    want = [("preds", inspect.Parameter.empty), ("views", inspect.Parameter.empty), ("export_ply_path", None),
            ("pts3d_key_to_visualize", "pts3d_local_aligned_to_global"), ("conf_key_to_visualize", "conf_local"),
            ("min_conf_thr_percentile", 0), ("flip_axes", False), ("max_num_points", None), ("sampling_strategy", "uniform")]
    params = list(inspect.signature(fast3r_amd.export_combined_ply).parameters.values())
    positional = [p for p in params if p.kind == p.POSITIONAL_OR_KEYWORD]
    assert [(p.name, p.default) for p in positional] == want
    keyword_only = {p.name: p.default for p in params if p.kind == p.KEYWORD_ONLY}
    assert keyword_only == {"sample": 0, "voxel_size": None, "generator": None} and len(params) == len(want) + 3
    for name in ("combine_points", "downsample_cloud", "voxel_down_sample", "farthest_point_down_sample"):
        assert callable(getattr(fast3r_amd, name))
    sig = inspect.signature(fast3r_amd.downsample_cloud)
    assert list(sig.parameters)[:4] == ["points", "colors", "max_num_points", "sampling_strategy"] and sig.parameters["order"].default == "index"
    assert list(inspect.signature(fast3r_amd.farthest_point_down_sample).parameters)[:3] == ["points", "num_samples", "start_index"]


def test_no_cpu_path_and_the_notebooks_error_text():
    import fast3r_amd
    from fast3r_amd._lib import F3RError
    p, c = torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8)
    for call in (lambda: fast3r_amd.downsample_cloud(p, c, 2, "voxel"), lambda: fast3r_amd.voxel_down_sample(p, c, 1.0),
                 lambda: fast3r_amd.farthest_point_down_sample(p, 2)):
        with pytest.raises(F3RError, match="ROCm device"):
            call()
    if not torch.cuda.is_available():
        preds = [{C.PTS_KEY: torch.zeros(1, 2, 2, 3), C.CONF_KEY: torch.ones(1, 2, 2)}]
        with pytest.raises(F3RError, match="no ROCm device"):
            fast3r_amd.export_combined_ply(preds, [{"img": torch.zeros(1, 3, 2, 2)}])
    src = open(os.path.join(ROOT, "fast3r_amd", "cloud.py")).read()
    assert 'raise ValueError(f"Unsupported sampling strategy: {sampling_strategy}")' in src
    assert not re.search(r"^\s*(import|from)\s+(open3d|trimesh|sklearn|scipy)", src, flags=re.M)


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["random", "lattice", "few_distinct"])
def test_fps_restatement_by_brute_force(name):
    """every selected point attains the maximum, over all points, of the minimum distance to the earlier selections"""
    p = {"random": C.random_cloud(300, 1)[0], "lattice": C.lattice(), "few_distinct": C.few_distinct()[0]}[name]
    k = 40
    sel = R.farthest_point_down_sample(p, k, start_index=3)
    assert sel[0] == 3 and sel.dtype == np.int32
    p64 = p.astype(np.float64)
    for i in range(1, k):
        d = np.full(len(p), np.inf)
        for s in sel[:i]:
            diff = p64 - p64[s]
            d = np.minimum(d, (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        if d.max() > 0:
            assert d[sel[i]] == d.max() and sel[i] == np.flatnonzero(d == d.max())[0]
        else:
            assert sel[i] == sel[i - 1]


def test_lattice_has_tied_maxima_and_few_distinct_repeats():
    assert R.fps_ties(C.lattice(), 40) >= 30
    p, _ = C.few_distinct()
    sel = R.farthest_point_down_sample(p, 40)
    assert len(np.unique(p, axis=0)) == 10 and len(np.unique(sel)) == 10 and len(set(sel[10:].tolist())) == 1
    assert len(R.select_by_index(p, None, sel)[0]) == 10 and len(R.select_by_index(p, None, sel, "selection")[0]) == 40


def test_voxel_restatement_against_unique_grouping():
    """small integer coordinates: no fp64 sum rounds, so np.unique + np.add.at (any order) must give the same bits"""
    p, c, vs = C.small_integers()
    got_p, got_c, got_n = R.voxel_down_sample(p, c, vs)
    idx = R.voxel_indices(p, vs)
    uniq, inv, cnt = np.unique(idx, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    sums = np.zeros((len(uniq), 3))
    np.add.at(sums, inv, p.astype(np.float64))
    assert np.array_equal(got_n, cnt.astype(np.int32)) and cnt.max() > 3
    assert got_p.dtype == np.float32 and got_p.tobytes() == (sums / cnt[:, None]).astype(np.float32).tobytes()
    csum = np.zeros((len(uniq), 3))
    np.add.at(csum, inv, c.astype(np.float64))                       # integer sums are exact; the restatement's are of c / 255.0
    assert np.abs(got_c.astype(np.int64) - np.floor(csum / cnt[:, None]).astype(np.int64)).max() <= 1


@pytest.mark.parametrize("recipe", ["on_boundaries", "duplicates", "small_integers", "own_voxels", "own_voxels_1023", "own_voxels_1024",
                                    "own_voxels_1025"])
def test_vectorised_voxel_restatement_equals_the_point_loop(recipe):
    p, c, vs = getattr(C, recipe)()
    a, b = R.voxel_down_sample(p, c, vs), R.voxel_down_sample_loop(p, c, vs)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    if recipe.startswith("own_voxels"):
        assert len(a[0]) == len(p) and (a[2] == 1).all()


def test_colour_quirk_is_in_the_recipes():
    pairs = R.quirk_pairs(8)
    assert len(pairs) == 173 and (9, 6) in pairs and (11, 3) in pairs
    p, c, vs, listed = C.quirk_colors()
    out_p, out_c, counts = R.voxel_down_sample(p, c, vs)
    assert counts.tolist() == [1] + [k for _, k in listed] and out_c[0].tolist() == [7, 7, 7]
    want = [cc if (cc, k) not in pairs else cc - 1 for cc, k in listed]
    assert out_c[1:, 0].tolist() == want and sum(w != cc for w, (cc, _) in zip(want, listed)) == 173
    assert out_c[1, 0] == 0 and out_c[2, 0] == 255 and out_c[3, 0] == 255


def test_combine_recipe_and_restatement():
    preds, views = C.combine_case()
    pix = [p[C.CONF_KEY].shape[1] * p[C.CONF_KEY].shape[2] for p in preds]
    assert pix[:8] == list(C.COMBINE_PIXELS) and len({p[C.CONF_KEY].shape[1:] for p in preds}) == len(preds)
    n = len(C.COMBINE_PIXELS)
    for pct in (0, 50, 80, 100):
        for i in (n, n + 1):                                         # the constant and the NaN view keep nothing
            assert R.combine(preds[i:i + 1], views[i:i + 1], percentile=pct) == (None, None)
    p0, c0 = R.combine(preds, views, percentile=0, sample=1)
    kept = sum(int((p[C.CONF_KEY][1] > p[C.CONF_KEY][1].min()).sum()) for i, p in enumerate(preds) if i not in (n, n + 1))
    assert len(p0) == kept and c0.dtype == np.uint8
    assert R.color_u8(np.array([-1.5, -1.0, 1.0, 1.25, 3.0, np.nan, 0.0], np.float32)).tolist() == [0, 0, 255, 255, 255, 0, 127]
    pf, _ = R.combine(preds, views, percentile=50, flip_axes=True)
    pn, _ = R.combine(preds, views, percentile=50)
    assert np.array_equal(pf[:, 0], pn[:, 0]) and np.array_equal(pf[:, 1], pn[:, 2]) and np.array_equal(pf[:, 2], -pn[:, 1])


# ------------------------------------------------------------------------------------------------------------------- host arithmetic
def test_voxel_grid_host_arithmetic():
    from fast3r_amd import cloud
    lo, hi = [0.0, -1.0, 2.0], [4.0, 2.0, 3.0]
    vs = cloud.heuristic_voxel_size(lo, hi, 1000)
    assert vs == (4.0 * 3.0 * 1.0 / 1000) ** (1 / 3)
    p, _ = C.random_cloud(500, 3)
    assert cloud.heuristic_voxel_size(p.min(0), p.max(0), 77) == R.heuristic_voxel_size(p, 77)
    # cells = floor(extent / voxel_size + 0.5) + 1; bits = ceil(log2(cells))
    assert cloud.voxel_key_bits([0, 0, 0], [0, 0, 0], 1.0) == [0, 0, 0]          # one cell per axis: no bits, no passes
    assert cloud.voxel_key_bits([0, 0, 0], [1.0, 1.4, 1.5], 1.0) == [1, 1, 2]    # 2, 2 and 3 cells
    assert cloud.voxel_key_bits([0, 0, 0], [255, 256, 3], 1.0) == [8, 9, 2]
    assert cloud.voxel_key_bits([-3, 5, 0], [4, 5.4, 1e-3], 0.5) == [4, 1, 0]
    for total, bits in C.BIT_CASES.items():
        p, _, vs = C.bits_cloud(bits)
        got = cloud.voxel_key_bits(p.min(0), p.max(0), vs)
        assert got == list(bits) == R.key_bits(p, vs) and sum(got) == total
        assert cloud.voxel_sort_passes(got) == -(-total // 8)
        assert int(R.voxel_indices(p, vs).max(0)[0]) == 2 ** bits[0] - 1
    assert sorted({cloud.voxel_sort_passes(b) for b in C.BIT_CASES.values()}) == [1, 2, 3, 4, 5, 6]
    assert cloud.voxel_sort_passes([0, 0, 0]) == 0 and cloud.voxel_sort_passes([21, 21, 21]) == 8
    with pytest.raises(ValueError, match="voxel_size too small for this extent"):
        cloud.voxel_key_bits([0, 0, 0], [1e6, 1e6, 1e6], 1e-1)                    # 24 bits per axis: 72 in all
    with pytest.raises(ValueError, match="voxel_size too small for this extent"):
        cloud.voxel_key_bits([0, 0, 0], [1.0, 0, 0], 1e-12)                       # 40 bits on one axis
    with pytest.raises(ValueError, match="voxel_size too small for this extent"):
        cloud.voxel_key_bits([0, 0, 0], [3e38, 0, 0], 1e-300)                     # the quotient overflows
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cloud.voxel_key_bits([0, 0, 0], [1, 1, 1], bad)
    # the cell count never falls below the largest index of the kernel's own expression
    rs = np.random.RandomState(0)
    for _ in range(2000):
        lo1, ext, v = rs.randn() * 10, abs(rs.randn()) * 50, abs(rs.randn()) + 1e-3
        top = np.floor((np.float64(lo1 + ext) - (np.float64(lo1) - 0.5 * v)) / v)
        assert 2 ** cloud.voxel_key_bits([lo1, 0, 0], [lo1 + ext, 0, 0], v)[0] > top


# ------------------------------------------------------------------------------------------------------------------- the library
def test_new_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f3r.h")).read(), flags=re.S)
    assert built_lib.f3r_version() >= 420 and _lib.ABI_VERSION == 410
    for name, arity in NEW_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity, name
        assert _lib.SYMBOL_SINCE[name] == 420 and getattr(built_lib, name).argtypes == _lib.SYMBOLS[name][1]
        assert _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_SINCE) == set(NEW_SYMBOLS)
    raw = open(os.path.join(ROOT, "include", "f3r.h")).read()
    for macro, const in (("F3R_CLOUD_TILE", _lib.CLOUD_TILE), ("F3R_CLOUD_SORT_TILE", _lib.CLOUD_SORT_TILE),
                         ("F3R_CLOUD_FPS_TILE", _lib.CLOUD_FPS_TILE), ("F3R_CLOUD_FPS_ONE_MAX", _lib.CLOUD_FPS_ONE_MAX)):
        assert int(re.search(r"#define %s (\d+)" % macro, raw).group(1)) == const
    assert _lib.CLOUD_FPS_ONE_MAX >= 4096
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_cloud ] && extra="-ffp-contract=off"' in build and "obj/f3r_cloud.o" in build


def test_later_entry_points_ask_an_older_library_to_rebuild(built_lib, monkeypatch):
    from fast3r_amd import _lib, post_ops
    monkeypatch.setattr(_lib, "library_version", lambda: 410)
    for name in NEW_SYMBOLS:
        with pytest.raises(_lib.F3RError, match="version 410.*needs >= 420.*rebuild it"):
            _lib.entry(name)
    assert _lib.entry("f3r_mesh_count") is built_lib.f3r_mesh_count               # an entry point of the gated version itself
    with pytest.raises(_lib.F3RError, match="rebuild it"):
        post_ops.cloud_fps(torch.zeros(4, 3), 2)                                  # a wrapper asks for its entry points before it looks at a tensor
    monkeypatch.undo()
    assert _lib.entry("f3r_cloud_fps") is built_lib.f3r_cloud_fps


def test_a_410_library_still_loads_without_the_later_symbols(tmp_path, monkeypatch):
    """lib() binds a symbol of SYMBOL_SINCE only when the library reports that version: its gate stays on ABI_VERSION"""
    import subprocess
    from fast3r_amd import _lib
    names = [n for n in _lib.SYMBOLS if n not in _lib.SYMBOL_SINCE and n not in ("f3r_version", "f3r_sizeof")]
    src, so = tmp_path / "stub.c", tmp_path / "libf3r_hip.so"
    sizes = (ctypes.sizeof(_lib.GemmArgs), ctypes.sizeof(_lib.AttnArgs), ctypes.sizeof(_lib.AttnF32Args))
    src.write_text("int f3r_version(void) { return 410; }\nunsigned long f3r_sizeof(int w) { return w == 0 ? %d : w == 1 ? %d : w == 2 ? %d : 0; }\n"
                   % sizes + "".join("int %s(void) { return 0; }\n" % n for n in names))
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    l = _lib.lib()
    assert l.f3r_version() == 410
    with pytest.raises(_lib.F3RError, match="version 410.*f3r_cloud_bounds needs >= 420.*rebuild it"):
        _lib.entry("f3r_cloud_bounds")


def test_sizing_functions(built_lib):
    for fn in (built_lib.f3r_cloud_voxel_workspace_bytes, built_lib.f3r_cloud_fps_workspace_bytes):
        for bad in (0, -1, 2 ** 31, 2 ** 40):
            assert fn(bad) == 0
        sizes = [fn(n) for n in (1, 2, 63, 64, 65, 1000, 2047, 2048, 2049, 10 ** 6, 10 ** 6 + 1, 84 * 10 ** 6, 2 ** 31 - 1)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert all(s % 256 == 0 for s in sizes)
    n = 10 ** 6
    # two (key, index) buffers, the digit-major histograms, the head scan and the voxel starts
    assert built_lib.f3r_cloud_voxel_workspace_bytes(n) >= 2 * 8 * n + 2 * 4 * n + 4 * 256 * -(-n // 2048) + 4 * (n + 1)
    assert built_lib.f3r_cloud_fps_workspace_bytes(n) >= 8 * n + 2 * 1024 * 12
    assert built_lib.f3r_cloud_voxel_workspace_bytes(n) < 40 * n and built_lib.f3r_cloud_fps_workspace_bytes(n) < 9 * n


def test_argument_errors_are_codes_before_any_launch(built_lib):
    l, err = built_lib, built_lib.f3r_last_error_string
    P = 0x1000
    assert l.f3r_cloud_combine_count(None, 1, 1, None, P, None) == -1 and b"null" in err()
    assert l.f3r_cloud_combine_count(P, 0, 1, None, P, None) == -1 and b"at least one view" in err()
    assert l.f3r_cloud_combine_write(P, 1, 1, None, P, 0, None, P, None) == -1
    assert l.f3r_cloud_bounds(P, 0, P, None) == -1 and l.f3r_cloud_bounds(P, 2 ** 31, P, None) == -1 and b"2^31" in err()
    mb, bits = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_int * 3)(8, 8, 8)
    assert l.f3r_cloud_voxel_sort(P, 10, mb, 0.0, bits, P, 1 << 20, P, None) == -1 and b"voxel_size" in err()
    assert l.f3r_cloud_voxel_sort(P, 10, mb, 1.0, (ctypes.c_int * 3)(22, 21, 21), P, 1 << 20, P, None) == -1 and b"at most 63" in err()
    assert l.f3r_cloud_voxel_sort(P, 10, mb, 1.0, (ctypes.c_int * 3)(32, 1, 1), P, 1 << 20, P, None) == -1
    assert l.f3r_cloud_voxel_sort(P, 10, mb, 1.0, bits, P, 16, P, None) == -1 and b"workspace too small" in err()
    assert l.f3r_cloud_voxel_sort(P, 10, (ctypes.c_double * 3)(0, float("nan"), 0), 1.0, bits, P, 1 << 20, P, None) == -1
    assert l.f3r_cloud_voxel_sums(P, None, 10, 11, P, 1 << 20, P, None, P, None) == -1 and b"n_voxels" in err()
    assert l.f3r_cloud_voxel_sums(P, P, 10, 5, P, 1 << 20, P, None, P, None) == -1
    assert l.f3r_cloud_fps(P, 10, 0, 0, 0, None, 0, P, None) == -1 and b"num_samples" in err()
    assert l.f3r_cloud_fps(P, 10, 11, 0, 0, None, 0, P, None) == -1
    assert l.f3r_cloud_fps(P, 10, 5, 10, 0, None, 0, P, None) == -1 and b"start_index" in err()
    assert l.f3r_cloud_fps(P, 10, 5, 0, 3, None, 0, P, None) == -1 and b"mode" in err()
    assert l.f3r_cloud_fps(P, 10 ** 5, 5, 0, 1, None, 0, P, None) == -1 and b"one-workgroup" in err()
    assert l.f3r_cloud_fps(P, 10 ** 5, 5, 0, 2, P, 16, P, None) == -1 and b"workspace too small" in err()
    assert l.f3r_cloud_mark(P, 0, 10, P, None) == -1 and l.f3r_cloud_mark(P, 11, 10, P, None) == -1
    assert l.f3r_cloud_gather(P, None, P, 0, 10, 0, P, None, None) == -1 and l.f3r_cloud_gather(P, P, P, 0, 10, 3, P, None, None) == -1
