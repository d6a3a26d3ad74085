"""The map pictures, the parts that need no GPU: the numpy restatement (tests/maps_ref.py) against matplotlib's own bytes -- the golden
file, and live matplotlib where it imports --, the two table files, the sheet's geometry, the colormap names, the npz's structure
against a key list kept as data, and the library side (symbol, presence gate, build flag, argument errors, no CPU path)."""
import ctypes
import inspect
import io
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

import map_cases as C
import maps_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"f3r_maps_colorize": 9}


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def test_recipes_give_the_stored_inputs(golden):
    for name, maps in C.scalar_cases().items():
        for i, a in enumerate(maps):
            assert a.dtype == np.float32 and golden[f"s/{name}/{i}/in"].tobytes() == a.tobytes(), name
    assert golden["z/in"].tobytes() == C.pointmap_case().tobytes()
    preds, views = C.views_case()
    for v, (pred, view) in enumerate(zip(preds, views)):
        assert golden[f"v/{v}/img/in"].tobytes() == view["img"].tobytes()
        for key, stored in (("conf", "conf"), ("conf_local", "conf_local"), ("pts3d_local", "depth_local")):
            assert (f"v/{v}/{stored}/in" in golden.files) == (key in pred)
            if key in pred:
                assert golden[f"v/{v}/{stored}/in"].tobytes() == pred[key].tobytes()
    assert "conf_local" not in preds[C.NO_CONF_LOCAL] and "pts3d_local" not in preds[C.NO_PTS3D_LOCAL]


def test_cases_have_their_stated_properties():
    c = C.scalar_cases()
    assert c["one_by_one"][0].shape == (1, 1) and np.ptp(c["constant_5x7"][0]) == 0
    assert c["row_1x1025"][0].size > 1024 and c["blocks_130x257"][0].size > 32 * 1024       # more than one 1024-pixel tile
    assert all(c["ragged_37x53"][0].size % k for k in (2, 4, 8)) and 53 % 4 and 257 % 4
    a, b = c["max_first_min_last"][0], c["min_first_max_last"][0]
    assert a.argmax() == 0 and a.argmin() == a.size - 1 and b.argmin() == 0 and b.argmax() == b.size - 1
    x = R.normalize(c["steps_0_to_256"][0]) * np.float32(256)
    assert np.array_equal(x[0], np.arange(257, dtype=np.float32))                        # every integer, 256 included
    assert R.normalize(c["ulp_steps"][0]).tolist() == [[0.0, 0.5, 1.0]]
    assert np.abs(c["huge_1e30"][0]).max() > 1e29
    d = c["overflow_3e38"][0]
    with np.errstate(over="ignore"):
        assert np.isinf(d.max() - d.min()) and np.isfinite(np.float64(d.max()) - np.float64(d.min()))
    s = c["subnormal"][0]
    assert 0 < s.max() < np.finfo(np.float32).tiny
    assert (c["negative_depths"][0] < 0).sum() == c["negative_depths"][0].size - 1
    left, mid, right = c["nan_in_the_middle_map"]
    assert np.isnan(mid).sum() == 1 and not np.isnan(left).any() and not np.isnan(right).any()
    assert np.isposinf(c["one_pos_inf"][0]).sum() == 1 and np.isneginf(c["one_neg_inf"][0]).sum() == 1
    p, l = c["portrait_and_landscape"]
    assert p.shape[0] > p.shape[1] and l.shape[0] < l.shape[1]
    _, views = C.views_case()
    assert all((v["img"] > 1).any() and (v["img"] < -1).any() for v in views)            # the clip has work to do


def test_restatement_equals_matplotlibs_bytes(golden):
    tables = {cmap: R.table(cmap) for cmap in C.CMAPS}
    n = 0
    for label, a, cmap, want in C.scalar_pictures(golden):
        got = R.colorize(a, tables[cmap])
        assert got.dtype == np.uint8 and got.shape == a.shape + (4,) and got.tobytes() == want.tobytes(), label
        n += 1
    assert n == 2 * (sum(len(m) for m in C.scalar_cases().values()) + 1)
    preds, views = C.views_case()
    for v, (pred, view) in enumerate(zip(preds, views)):
        for b in range(2):
            assert R.rgb_picture(view["img"][b]).tobytes() == golden[f"v/{v}/img/{b}"].tobytes()
            assert R.colorize(pred["conf"][b], tables["turbo"]).tobytes() == golden[f"v/{v}/conf/{b}"].tobytes()
            if "conf_local" in pred:
                assert R.colorize(pred["conf_local"][b], tables["turbo"]).tobytes() == golden[f"v/{v}/conf_local/{b}"].tobytes()
            if "pts3d_local" in pred:
                assert R.colorize(pred["pts3d_local"][b][..., 2], tables["Greys"]).tobytes() == golden[f"v/{v}/depth_local/{b}"].tobytes()


def test_what_the_golden_pictures_show(golden):
    """the NaN map is transparent throughout and its neighbours are not touched by it; an inf pixel is transparent among index-0 pixels;
    the fp32 subtraction equals numpy's fp64 one rounded; the fp64 divisor matters"""
    assert not golden["s/nan_in_the_middle_map/1/turbo"].any() and not golden["s/nan_in_the_middle_map/1/Greys"].any()
    for i in (0, 2):
        assert (golden[f"s/nan_in_the_middle_map/{i}/turbo"][..., 3] == 255).all()
    turbo = R.table("turbo")
    pic, a = golden["s/one_pos_inf/0/turbo"], golden["s/one_pos_inf/0/in"]
    assert not pic[np.isinf(a)].any() and (pic[~np.isinf(a)] == np.append(turbo[0], 255)).all()
    assert not golden["s/one_neg_inf/0/turbo"].any()                                      # inf - inf and inf / inf everywhere
    over, d = golden["s/overflow_3e38/0/turbo"], golden["s/overflow_3e38/0/in"]
    assert (over[..., 3] == 255).all() and tuple(over[d == d.max()][0][:3]) == tuple(turbo[255]) and tuple(over[d == d.min()][0][:3]) == tuple(turbo[0])
    assert len({tuple(p) for p in over.reshape(-1, 4).tolist()}) > 10                    # the fp64 range keeps the picture: not two colours
    assert (golden["s/constant_5x7/0/Greys"] == 255).all() and (golden["s/one_by_one/0/turbo"] == np.append(turbo[0], 255)).all()
    for name, maps in C.scalar_cases().items():
        for a in maps:
            with np.errstate(invalid="ignore", over="ignore"):
                vmin = a.min()
                in64 = (a.astype(np.float64) - np.float64(vmin)).astype(np.float32)
                assert (a - vmin).tobytes() == in64.tobytes() or np.isnan(vmin), name
    a = C.scalar_cases()["fp64_divisor"][0]
    all_fp32 = ((a - a.min()) / (a.max() - a.min()) * np.float32(256)).astype(int)
    as_matplotlib = (R.normalize(a) * np.float32(256)).astype(int)
    assert all_fp32[3, 2] == 217 and as_matplotlib[3, 2] == 218 and (all_fp32 != as_matplotlib).sum() == 1
    assert tuple(golden["s/fp64_divisor/0/turbo"][3, 2][:3]) == tuple(turbo[218]) != tuple(turbo[217])


def test_restatement_equals_live_matplotlib():
    pytest.importorskip("matplotlib")
    from matplotlib import colormaps, pylab
    from PIL import Image

    def imsave(a, **kw):
        buf = io.BytesIO()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            pylab.imsave(buf, a, format="png", **kw)
        buf.seek(0)
        return np.asarray(Image.open(buf).convert("RGBA"))

    for cmap in C.CMAPS:
        m = colormaps[cmap]
        m._init()
        assert ((m._lut[:256, :3] * 255).astype(np.uint8)).tobytes() == R.table(cmap).tobytes()
    rs = np.random.RandomState(77)
    maps = [m for ms in C.scalar_cases().values() for m in ms]
    maps += [(rs.randn(11, 13) * 10.0 ** rs.randint(-30, 30)).astype(np.float32) for _ in range(20)]
    for a in maps:
        for cmap in ("turbo", "Greys"):
            assert R.colorize(a, R.table(cmap)).tobytes() == imsave(a, cmap=cmap).tobytes()
    img = rs.uniform(-1.05, 1.05, (3, 9, 14)).astype(np.float32)
    u8 = ((img.transpose(1, 2, 0) + 1) * 127.5).astype(int).clip(0, 255).astype(np.uint8)
    assert R.rgb_picture(img).tobytes() == imsave(u8).tobytes()


# ------------------------------------------------------------------------------------------------------------------- tables and names
def test_the_two_table_files():
    from fast3r_amd import maps, scene
    greys, turbo = maps.greys_lut_u8(), scene.turbo_lut_u8()
    assert greys.shape == turbo.shape == (256, 3) and greys.dtype == np.uint8
    assert os.path.getsize(scene.TURBO_LUT_PATH) == 768 and maps.GREYS_LUT_PATH.endswith(".txt") and open(maps.GREYS_LUT_PATH).read().isascii()
    g = greys.astype(int)
    assert (g[:, 0] == g[:, 1]).all() and (g[:, 0] == g[:, 2]).all() and g[0, 0] == 255 and g[255, 0] == 0 and (np.diff(g[:, 0]) <= 0).all()
    assert tuple(turbo[0]) == (48, 18, 59) and tuple(turbo[255]) == (122, 4, 2)          # matplotlib's turbo ends, * 255 truncated
    assert R.table("Greys").tobytes() == greys.tobytes() and R.table("turbo").tobytes() == turbo.tobytes()


def test_cmap_names_are_the_notebooks():
    import fast3r_amd
    from fast3r_amd import maps
    assert maps.cmap_table("turbo") == maps.cmap_table("Turbo") == "turbo" and maps.cmap_table("Greys") == "Greys"
    for bad in ("viridis", "greys", "TURBO", "", None, 3):
        with pytest.raises(ValueError, match="'turbo' and 'Greys'"):
            maps.cmap_table(bad)
        with pytest.raises(ValueError, match="'turbo' and 'Greys'"):
            fast3r_amd.colorize_maps([], cmap=bad)
    assert fast3r_amd.colorize_maps([]) == []


def test_signatures_are_the_notebooks():
    import fast3r_amd
    want = {"plot_rgb_images": [("views", inspect.Parameter.empty), ("title", "RGB Images"), ("save_image_to_folder", None)],
            "plot_confidence_maps": [("preds", inspect.Parameter.empty), ("title", "Confidence Maps"), ("save_image_to_folder", None)],
            "maybe_plot_local_depth_and_conf": [("preds", inspect.Parameter.empty), ("title", "Local Depth and Confidence Maps"),
                                                ("save_image_to_folder", None)],
            "save_pointmaps_and_camera_parameters_to_folder": [("preds", inspect.Parameter.empty), ("save_folder", inspect.Parameter.empty),
                                                               ("niter_PnP", 100), ("focal_length_estimation_method", "individual")]}
    for name, params in want.items():
        sig = inspect.signature(getattr(fast3r_amd, name))
        positional = [(p.name, p.default) for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD]
        assert positional == params, name
        extra = {p.name: p.default for p in sig.parameters.values() if p.kind == p.KEYWORD_ONLY}
        assert extra == ({} if name.startswith("save_") else {"max_columns": 8, "sample": 0}), name
    sig = inspect.signature(fast3r_amd.colorize_maps)
    assert [(p.name, p.default, p.kind == p.KEYWORD_ONLY) for p in sig.parameters.values()] == [
        ("maps", inspect.Parameter.empty, False), ("cmap", "turbo", False), ("channel", None, True), ("return_ranges", False, True)]
    for f in os.listdir(os.path.join(ROOT, "fast3r_amd")):
        if f.endswith(".py"):
            src = open(os.path.join(ROOT, "fast3r_amd", f)).read()
            assert not re.search(r"^\s*(import|from)\s+(matplotlib|plotly)", src, flags=re.M), f


# ------------------------------------------------------------------------------------------------------------------- sheet geometry
def test_sheet_layout():
    from fast3r_amd.maps import sheet_layout, title_file_name
    shapes = [(20, 12), (12, 20), (9, 13)]
    h, w, cell, origins = sheet_layout(shapes)
    assert (h, w, cell) == (20, 60, (20, 20)) and origins == [[(0, 0)], [(0, 20)], [(0, 40)]]
    h, w, cell, origins = sheet_layout(shapes, max_columns=2)
    assert (h, w, cell) == (40, 40, (20, 20)) and origins == [[(0, 0)], [(0, 20)], [(20, 0)]]
    h, w, cell, origins = sheet_layout(shapes, max_columns=2, rows_per_view=2)                # conf above depth, band after band
    assert (h, w) == (80, 40) and origins == [[(0, 0), (20, 0)], [(0, 20), (20, 20)], [(40, 0), (60, 0)]]
    h, w, cell, origins = sheet_layout([None, (3, 5), None], rows_per_view=2)                 # views without a map still own their column
    assert (h, w, cell) == (6, 15, (3, 5)) and origins[1] == [(0, 5), (3, 5)]
    assert sheet_layout([(4, 4)] * 17)[:3] == (12, 32, (4, 4))                                # 8 columns, three bands
    assert sheet_layout([], 8)[:2] == (0, 0) and sheet_layout([None, None])[:2] == (0, 0)
    with pytest.raises(ValueError, match="max_columns"):
        sheet_layout(shapes, max_columns=0)
    assert title_file_name("Local Depth and Confidence Maps") == "Local_Depth_and_Confidence_Maps.png"
    # the restatement's sheet uses the same geometry
    pics = [[np.full(s + (4,), 10 + i, np.uint8), None if i == 1 else np.full(s + (4,), 20 + i, np.uint8)] for i, s in enumerate(shapes)]
    sheet = R.sheet(pics, max_columns=2)
    h, w, _, origins = sheet_layout(shapes, max_columns=2, rows_per_view=2)
    assert sheet.shape == (h, w, 4)
    filled = np.zeros((h, w), bool)
    for i, (s, row) in enumerate(zip(shapes, pics)):
        for k, p in enumerate(row):
            if p is not None:
                y, x = origins[i][k]
                assert (sheet[y:y + s[0], x:x + s[1]] == p).all()
                filled[y:y + s[0], x:x + s[1]] = True
    assert not sheet[~filled].any()


# ------------------------------------------------------------------------------------------------------------------- the npz
def test_npz_structure_from_host_logic(tmp_path, monkeypatch):
    """the writer with the pose solve replaced (that part needs a GPU; tests/test_maps_gpu.py runs the real one)"""
    import fast3r_amd
    from fast3r_amd import maps
    spec = R.npz_spec()
    assert [e["key"] for e in spec] == list(maps.NPZ_KEYS) + ["estimated_focals", "estimated_poses_c2w"] and len(spec) == 7
    n, B, H, W = 3, 2, 6, 8
    rs = np.random.RandomState(0)
    preds = [{"pts3d_in_other_view": torch.from_numpy(rs.rand(B, H, W, 3).astype(np.float32)), "conf": torch.from_numpy(rs.rand(B, H, W).astype(np.float32)),
              "pts3d_local": torch.from_numpy(rs.rand(B, H, W, 3).astype(np.float32)), "conf_local": torch.from_numpy(rs.rand(B, H, W).astype(np.float32)),
              "pts3d_local_aligned_to_global": torch.from_numpy(rs.rand(B, H, W, 3).astype(np.float32))} for _ in range(n)]
    seen = {}

    def solve(p, niter_PnP=10, focal_length_estimation_method="individual"):
        seen.update(niter=niter_PnP, method=focal_length_estimation_method, preds=p)
        return [[np.eye(4) * (b + 1) for _ in range(n)] for b in range(B)], [[100.0 + b, None, 300.0 + b] for b in range(B)]

    monkeypatch.setattr(maps, "estimate_camera_poses", solve)
    path = fast3r_amd.save_pointmaps_and_camera_parameters_to_folder({"preds": preds, "views": None}, str(tmp_path / "out"))
    assert path == str(tmp_path / "out" / "pointmaps_and_camera_params.npz") and seen["niter"] == 100 and seen["method"] == "individual"
    data = R.check_npz(path, n, H, W)
    assert data["global_confidence_maps"].tobytes() == np.stack([p["conf"][0].numpy() for p in preds]).tobytes()   # batch row 0
    assert data["local_pointmaps"].tobytes() == np.stack([p["pts3d_local"][0].numpy() for p in preds]).tobytes()
    f = data["estimated_focals"]
    assert f[0] == 100.0 and np.isnan(f[1]) and f[2] == 300.0 and np.array_equal(data["estimated_poses_c2w"][2], np.eye(4))
    fast3r_amd.save_pointmaps_and_camera_parameters_to_folder(preds, str(tmp_path / "again"), 7, "first_view_from_global_head")
    assert seen["niter"] == 7 and seen["method"] == "first_view_from_global_head"
    del preds[1]["pts3d_local_aligned_to_global"]
    with pytest.raises(KeyError, match=r"preds\[1\].*call align_local_pts3d_to_global"):
        fast3r_amd.save_pointmaps_and_camera_parameters_to_folder(preds, str(tmp_path / "missing"))
    assert not os.path.exists(tmp_path / "missing")


# ------------------------------------------------------------------------------------------------------------------- the library side
def test_new_symbol_is_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    raw = open(os.path.join(ROOT, "include", "f3r.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity, name
        assert _lib.symbol_since(name) == 0 and _lib.if_present(name) and name in _lib.SYMBOL_IF_PRESENT_MAPS
        assert getattr(built_lib, name).argtypes == _lib.SYMBOLS[name][1] and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_IF_PRESENT_MAPS) == set(NEW_SYMBOLS) and not _lib.if_present("f3r_gemm") and _lib.if_present("f3r_raster_triangles")
    assert int(re.search(r"#define F3R_MAPS_TILE (\d+)", raw).group(1)) == _lib.MAPS_TILE == 1024
    assert re.search(r"F3R_MAPS_LUT = 0, F3R_MAPS_RGB = 1", raw) and (_lib.F3R_MAPS_LUT, _lib.F3R_MAPS_RGB) == (0, 1)
    assert "map pictures" in raw.lower()


def test_build_script_carries_the_file_and_the_flag():
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_maps ] && extra="-ffp-contract=off"' in build and '"$here"/obj/f3r_maps.o' in build
    assert re.search(r"^for f in .*\bf3r_maps\b.*; do$", build, flags=re.M)
    src = open(os.path.join(ROOT, "fast3r_amd", "csrc", "f3r_maps.hip")).read()
    assert '#include "f3r_prims.h"' in src and "block_min_max" in src


def test_a_library_without_the_map_pictures_still_loads(tmp_path, monkeypatch):
    from fast3r_amd import _lib, post_ops
    import fast3r_amd
    names = [n for n in _lib.SYMBOLS if n not in _lib.SYMBOL_IF_PRESENT_MAPS and n not in ("f3r_version", "f3r_sizeof")]
    src, so = tmp_path / "stub.c", tmp_path / "libf3r_hip.so"
    sizes = (ctypes.sizeof(_lib.GemmArgs), ctypes.sizeof(_lib.AttnArgs), ctypes.sizeof(_lib.AttnF32Args))
    src.write_text("int f3r_version(void) { return 430; }\nunsigned long f3r_sizeof(int w) { return w == 0 ? %d : w == 1 ? %d : w == 2 ? %d : 0; }\n"
                   % sizes + "".join("int %s(void) { return 0; }\n" % n for n in names))
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    l = _lib.lib()
    assert _lib.entry("f3r_raster_triangles") is l.f3r_raster_triangles
    with pytest.raises(_lib.F3RError, match="does not export f3r_maps_colorize: rebuild it"):
        _lib.entry("f3r_maps_colorize")
    cpu = torch.zeros(4, 4)
    with pytest.raises(_lib.F3RError, match="rebuild it"):
        post_ops.maps_colorize([cpu], [cpu])
    with pytest.raises(_lib.F3RError):
        fast3r_amd.colorize_maps([cpu])


def test_no_cpu_path(built_lib):
    import fast3r_amd
    from fast3r_amd import _lib, post_ops
    a = torch.zeros(4, 5)
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.colorize_maps([a])
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        post_ops.maps_colorize([a], [torch.zeros(4, 5, 4, dtype=torch.uint8)], torch.zeros(256, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="torch tensor"):
        fast3r_amd.colorize_maps([np.zeros((4, 5), np.float32)])
    if not torch.cuda.is_available():
        with pytest.raises(_lib.F3RError, match="no ROCm device"):
            fast3r_amd.plot_confidence_maps([{"conf": torch.zeros(1, 4, 5)}])
        with pytest.raises(_lib.F3RError, match="no ROCm device"):
            fast3r_amd.plot_rgb_images([{"img": torch.zeros(1, 3, 4, 5)}])


def test_argument_errors_are_codes_before_any_launch(built_lib):
    l, err = built_lib, built_lib.f3r_last_error_string
    P = 0x1000

    def call(rows=((P, 1, 4, 5, 2 * P, 20),), **kw):
        flat = [x for r in rows for x in r]
        tiles = sum((r[2] * r[3] + 1023) // 1024 for r in rows if r[2] > 0 and r[3] > 0)
        a = dict(table=P, host_rows=(ctypes.c_int64 * len(flat))(*flat), n_maps=len(rows), n_tiles=tiles, mode=0, lut=P, keys=P, ranges=P, stream=None)
        a.update(kw)
        return l.f3r_maps_colorize(*a.values())

    for name in ("table", "host_rows"):
        assert call(**{name: None}) == -1 and b"null table or host_rows" in err(), name
    for name in ("lut", "keys", "ranges"):
        assert call(**{name: None}) == -1 and b"null lut, keys or ranges" in err(), name
    assert call(n_maps=0) == -1 and b"n_maps" in err()
    for mode in (2, -1):
        assert call(mode=mode) == -1 and b"unknown mode" in err()
    for H, W in ((0, 5), (4, 0), (-1, 5), (2 ** 15 + 1, 2 ** 15), (2 ** 31, 1)):
        assert call(rows=((P, 1, H, W, 2 * P, 4 * max(W, 1)),)) == -1 and b"H W <= 2^30" in err(), (H, W)
    assert call(rows=((P, 1, 4, 5, 2 * P, 16),)) == -1 and b"pitch 16 is smaller than 4 W = 20" in err()
    assert call(rows=((P, 1, 4, 5, 2 * P, 20), (P, 1, 4, 5, 2 * P, 19))) == -1 and b"map 1: pitch" in err()
    assert call(rows=((0, 1, 4, 5, 2 * P, 20),)) == -1 and b"null source or destination" in err()
    assert call(rows=((P, 1, 4, 5, 0, 20),)) == -1 and b"null source or destination" in err()
    for stride in (0, -3, 2 ** 31):
        assert call(rows=((P, stride, 4, 5, 2 * P, 20),)) == -1 and b"stride" in err()
    assert call(rows=((P + 2, 1, 4, 5, 2 * P, 20),)) == -1 and b"4-byte aligned" in err()
    assert call(rows=((P, 1, 4, 5, 2 * P + 1, 20),)) == -1 and b"4-byte aligned" in err()
    assert call(rows=((P, 1, 4, 5, 2 * P, 22),)) == -1 and b"4-byte aligned" in err()
    assert call(n_tiles=2) == -1 and b"n_tiles" in err()
    assert call(rows=((P, 1, 33, 32, 2 * P, 128),), n_tiles=1) == -1 and b"n_tiles" in err()   # 1056 pixels are two tiles
