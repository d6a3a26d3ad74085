"""Ground-truth views, the parts that need no GPU: the host plan (fast3r_amd/gt_views.py plan_view, nearest_table) and the numpy / Pillow
restatement (tests/gt_views_ref.py) against what the reference's own dataset path returned (tests/golden/gt_views_cases.pt, written by
tools/make_golden_gt_views.py), the OpenCV stand-in against the closed form of its index rule, the error conditions, and the library side
(symbols, presence gate, build flag, argument errors, no CPU path)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import cv2_resize_stub
import gt_views_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gt_views_cases.pt")
NEW_SYMBOLS = {"f3r_gtview_workspace_bytes": 3, "f3r_gtview_resample": 26, "f3r_gtview_unproject": 22}
CASES = ("1_plain_lanczos", "2_half_even_square_target", "3_odd_sizes", "4_portrait", "5_upscale_bicubic", "6_square_landscape",
         "6_square_portrait", "7_depth_edge_values", "8_three_views_one_geometry", "8_four_views_two_geometries", "9_no_pose")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def case_inputs(golden, name):
    c = golden["cases"][name]
    frames = [golden["frames"][k] for k in c["frames"]]
    poses = [golden["poses"][k].numpy() for k in c["frames"]] if c["with_pose"] else None
    return ([f["image"].numpy() for f in frames], [f["depthmap"].numpy() for f in frames], [f["intrinsics"].numpy() for f in frames], poses,
            c["resolution"], c["square_portrait"], c["views"])


def test_the_fixture_holds_the_cases_and_only_data(golden):
    assert tuple(golden["cases"]) == CASES and golden["restatement_matches"] is True
    assert os.path.getsize(GOLDEN) < 1000 * 1000
    for f in golden["frames"].values():
        assert f["image"].dtype == torch.uint8 and f["image"].shape[0] <= 97 and f["image"].shape[1] <= 161
        assert f["depthmap"].dtype == torch.float32 and f["intrinsics"].dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------------- the host plan
@pytest.mark.parametrize("name", CASES)
def test_plan_view_equals_the_reference_numbers(golden, name):
    from fast3r_amd import gt_views
    images, _, Ks, _, resolution, choices, views = case_inputs(golden, name)
    for i, view in enumerate(views):
        plan = gt_views.plan_view((images[i].shape[1], images[i].shape[0]), Ks[i], resolution, choices[i])
        trace = view["trace"]
        assert plan["box1"] == tuple(trace["box1"]) and plan["box2"] == tuple(trace["box2"]) and plan["resized"] == tuple(trace["resized"])
        assert plan["true_shape"] == tuple(view["true_shape"].tolist())
        K = gt_views._returned_intrinsics(plan)
        assert K.dtype == np.float32 and K.tobytes() == view["camera_intrinsics"].numpy().tobytes()
        W1, H1 = plan["box1"][2] - plan["box1"][0], plan["box1"][3] - plan["box1"][1]
        nx, ny = gt_views.nearest_table(W1, plan["resized"][0]), gt_views.nearest_table(H1, plan["resized"][1])
        assert nx.dtype == np.int32 and np.array_equal(nx, trace["nearest_x"].numpy()) and np.array_equal(ny, trace["nearest_y"].numpy())
        assert plan["filter"] == ("lanczos" if plan["scale_final"] < 1 else "bicubic")
        assert plan["transpose"] == (plan["true_shape"][1] < plan["true_shape"][0])


def test_plan_view_on_the_facts_the_cases_were_chosen_for(golden):
    from fast3r_amd import gt_views
    def plan(name, i=0):
        images, _, Ks, _, resolution, choices, _ = case_inputs(golden, name)
        return gt_views.plan_view((images[i].shape[1], images[i].shape[0]), Ks[i], resolution, choices[i])

    p = plan("1_plain_lanczos")
    assert p["box1"] == (0, 0, 80, 60) and p["resized"] == (32, 24) and p["box2"] == (0, 0, 32, 24) and p["filter"] == "lanczos"
    p = plan("2_half_even_square_target")     # cx = 40.5 rounds to 40 (half to even): 41 would give the window (2, 0, 80, 60)
    assert p["box1"] == (0, 0, 80, 60) and p["resized"] == (42, 32) and p["box2"][0] == 5
    p = plan("3_odd_sizes")
    assert p["box1"] == (0, 3, 154, 97) and p["resized"][0] % 4 and (p["box2"][2] - p["box2"][0], p["box2"][3] - p["box2"][1]) == (70, 38)
    p = plan("4_portrait")
    assert p["portrait"] and p["transpose"] and p["target"] == (24, 32) and p["box2"][1] > 0 and p["true_shape"] == (32, 24)
    p = plan("5_upscale_bicubic")
    assert p["filter"] == "bicubic" and p["scale_final"] > 1
    assert not plan("6_square_landscape")["portrait"] and plan("6_square_portrait")["portrait"]
    assert plan("6_square_portrait")["true_shape"] == (32, 24) and plan("6_square_landscape")["true_shape"] == (24, 32)
    assert gt_views._group_key(plan("8_four_views_two_geometries", 0)) == gt_views._group_key(plan("8_four_views_two_geometries", 2))
    assert gt_views._group_key(plan("8_four_views_two_geometries", 0)) != gt_views._group_key(plan("8_four_views_two_geometries", 1))


def test_resolution_follows_the_reference_rule():
    from fast3r_amd import gt_views
    assert gt_views._resolution(224) == (224, 224) and gt_views._resolution((512, 384)) == (512, 384) and gt_views._resolution([32, 32]) == (32, 32)
    for bad in ((24, 32), (32.0, 24), "512", (32,), (0, 0), None, True):
        with pytest.raises(ValueError, match="resolution"):
            gt_views._resolution(bad)


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_golden(golden, name):
    images, depths, Ks, poses, resolution, choices, views = case_inputs(golden, name)
    mine = R.build(images, depths, Ks, poses, resolution, choices)
    assert len(mine) == len(views)
    for got, want in zip(mine, views):
        for key in R.KEYS_EXACT:
            w = want[key].numpy()
            assert got[key].dtype == w.dtype and got[key].shape == w.shape and got[key].tobytes() == w.tobytes(), key
        assert np.array_equal(got["camera_pose"], want["camera_pose"].numpy(), equal_nan=True)
        ok, ratio = R.pts3d_close(want["pts3d"].numpy(), got)    # the reference's einsum against the restatement's fixed order
        assert ok, ratio
        assert np.array_equal(np.isfinite(got["pts3d"]), np.isfinite(want["pts3d"].numpy()))
        # the camera-frame points are the fp64 expression rounded once: the golden's z channel and, for an identity pose, everything
        assert got["X_cam"][..., 2].tobytes() == np.ascontiguousarray(got["depthmap"]).tobytes()


def test_the_edge_case_holds_what_it_was_built_for(golden):
    v = golden["cases"]["7_depth_edge_values"]["views"][0]
    assert v["depthmap"][12, 30] == 3.0e38 and not torch.isfinite(v["pts3d"][12, 30]).all() and not v["valid_mask"][12, 30]
    assert (v["depthmap"] == 0).any() and (v["depthmap"] < 0).any()
    assert not v["valid_mask"][v["depthmap"] <= 0].any() and v["valid_mask"][(v["depthmap"] > 0) & (v["depthmap"] < 10)].all()
    K = v["camera_intrinsics"]
    assert abs(30 - float(K[0, 2])) / float(K[0, 0]) > 2
    n = golden["cases"]["9_no_pose"]["views"][0]
    assert torch.isnan(n["camera_pose"]).all() and torch.isnan(n["pts3d"]).all() and not n["valid_mask"].any()


def test_pts3d_bound_is_the_derived_one():
    X = np.array([[[1.0, -2.0, 4.0]]], dtype=np.float32)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, :3] = [[0.5, -0.5, 0.25], [0, 1, 0], [0, 0, -1]]
    pose[:3, 3] = [1, -3, 0]
    b = R.pts3d_bound(X, pose)
    assert np.allclose(b[0, 0], 8 * 2.0 ** -24 * np.array([0.5 + 1.0 + 1.0 + 1, 2.0 + 3, 4.0]), rtol=1e-12)


# ------------------------------------------------------------------------------------------------------------------- the OpenCV stand-in
def test_the_stub_index_rule_is_the_closed_form():
    from fast3r_amd import gt_views
    differs_from_rational = 0
    for src in range(1, 65):
        for dst in range(1, 65):
            closed = [min(int(math.floor(x * (1.0 / (dst / src)))), src - 1) for x in range(dst)]
            assert cv2_resize_stub.nn_indices(src, dst).tolist() == closed, (src, dst)
            assert gt_views.nearest_table(src, dst).tolist() == closed and R.nearest_indices(src, dst).tolist() == closed
            assert closed[0] == 0 and all(b >= a for a, b in zip(closed, closed[1:])) and closed[-1] <= src - 1
            differs_from_rational += closed != [min((x * src) // dst, src - 1) for x in range(dst)]
    # the double product rounds below an integer for some sizes (49 -> 7 ... ): the rule is OpenCV's double arithmetic, not the exact quotient
    assert differs_from_rational > 0


def test_the_stub_resize_gathers_by_the_rule():
    a = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    out = cv2_resize_stub.resize(a, (10, 3), fx=9.0, fy=9.0, interpolation=cv2_resize_stub.INTER_NEAREST)   # fx, fy are ignored
    ys, xs = cv2_resize_stub.nn_indices(5, 3), cv2_resize_stub.nn_indices(7, 10)
    assert out.shape == (3, 10) and out.dtype == np.float32 and np.array_equal(out, a[ys][:, xs])
    with pytest.raises(NotImplementedError):
        cv2_resize_stub.resize(a, (10, 3))


# ------------------------------------------------------------------------------------------------------------------- errors
def test_error_conditions_raise_before_any_device_work(golden):
    import fast3r_amd
    from fast3r_amd import _lib, gt_views
    K = np.array([[70, 0, 40], [0, 70, 30], [0, 0, 1]], dtype=np.float32)
    for cx, cy in ((16.0, 30.0), (64.4, 30.0), (40.0, 12.0), (40.0, 48.0)):      # min_margin_x <= W / 5 = 16 or min_margin_y <= H / 5 = 12
        bad = K.copy()
        bad[0, 2], bad[1, 2] = cx, cy
        with pytest.raises(ValueError, match="principal point"):
            gt_views.plan_view((80, 60), bad, (32, 24))
    ok = K.copy()
    ok[0, 2] = 17.0
    gt_views.plan_view((80, 60), ok, (32, 24))
    img, dep = np.zeros((60, 80, 3), np.uint8), np.ones((60, 80), np.float32)
    with pytest.raises(_lib.F3RError, match="no CPU fallback"):
        fast3r_amd.build_gt_views([torch.from_numpy(img)], [torch.from_numpy(dep)], [K], resolution=(32, 24), device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.F3RError, match="no ROCm device"):
            fast3r_amd.build_gt_views([img], [dep], [K], resolution=(32, 24))
        return
    skew = K.copy()
    skew[0, 1] = 0.5
    with pytest.raises(ValueError, match="skew"):
        fast3r_amd.build_gt_views([img], [dep], [skew], resolution=(32, 24))
    pose = np.eye(4, dtype=np.float32)
    pose[1, 3] = np.inf
    with pytest.raises(ValueError, match="camera pose"):
        fast3r_amd.build_gt_views([img], [dep], [K], [pose], resolution=(32, 24))
    with pytest.raises(ValueError, match="one depthmap"):
        fast3r_amd.build_gt_views([img], [dep, dep], [K], resolution=(32, 24))
    with pytest.raises(ValueError, match="resolution"):
        fast3r_amd.build_gt_views([img], [dep], [K], resolution=(24, 32))


def test_no_cpu_path_for_the_named_functions():
    import fast3r_amd
    from fast3r_amd import _lib
    K = np.array([[70, 0, 40], [0, 70, 30], [0, 0, 1]], dtype=np.float32)
    dep, img = torch.ones(60, 80), torch.zeros(60, 80, 3, dtype=torch.uint8)
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.depthmap_to_camera_coordinates(dep, K)
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.depthmap_to_absolute_camera_coordinates(dep, K, np.eye(4))
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.crop_resize_if_necessary(img, dep, K, (32, 24))
    with pytest.raises(ValueError, match="torch tensor"):
        fast3r_amd.depthmap_to_camera_coordinates(dep.numpy(), K)


# ------------------------------------------------------------------------------------------------------------------- the library side
def test_new_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    raw = open(os.path.join(ROOT, "include", "f3r.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity, name
        assert _lib.symbol_since(name) == 0 and _lib.if_present(name) and name in _lib.SYMBOL_IF_PRESENT_VIEWS
        assert name not in _lib.SYMBOL_IF_PRESENT and name not in _lib.SYMBOL_IF_PRESENT_MAPS
        assert getattr(built_lib, name).argtypes == _lib.SYMBOLS[name][1] and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_IF_PRESENT_VIEWS) == set(NEW_SYMBOLS) and not _lib.if_present("f3r_gemm")
    assert _lib.if_present("f3r_raster_triangles") and _lib.if_present("f3r_maps_colorize")
    assert int(re.search(r"#define F3R_GTVIEW_CAM_WORDS (\d+)", raw).group(1)) == _lib.GTVIEW_CAM_WORDS == 25
    assert re.search(r"F3R_GTVIEW_POSE = 1, F3R_GTVIEW_FINITE_MASK = 2", raw) and (_lib.F3R_GTVIEW_POSE, _lib.F3R_GTVIEW_FINITE_MASK) == (1, 2)
    assert "ground-truth views" in raw.lower()


def test_the_version_did_not_move(built_lib):
    from fast3r_amd import _lib
    assert built_lib.f3r_version() == 430 and _lib.ABI_VERSION == 410


def test_build_script_carries_the_file_and_the_flag():
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_views ] && extra="-ffp-contract=off"' in build and '"$here"/obj/f3r_views.o' in build
    assert re.search(r"^for f in .*\bf3r_views\b.*; do$", build, flags=re.M)
    src = open(os.path.join(ROOT, "fast3r_amd", "csrc", "f3r_views.hip")).read()
    assert '#include "f3r_prims.h"' in src and "1 << 21" in src and ">>= 22" in src


def test_a_library_without_the_views_still_loads(tmp_path, monkeypatch):
    from fast3r_amd import _lib, post_ops
    import fast3r_amd
    names = [n for n in _lib.SYMBOLS if n not in _lib.SYMBOL_IF_PRESENT_VIEWS and n not in ("f3r_version", "f3r_sizeof")]
    src, so = tmp_path / "stub.c", tmp_path / "libf3r_hip.so"
    sizes = (ctypes.sizeof(_lib.GemmArgs), ctypes.sizeof(_lib.AttnArgs), ctypes.sizeof(_lib.AttnF32Args))
    src.write_text("int f3r_version(void) { return 430; }\nunsigned long f3r_sizeof(int w) { return w == 0 ? %d : w == 1 ? %d : w == 2 ? %d : 0; }\n"
                   % sizes + "".join("int %s(void) { return 0; }\n" % n for n in names))
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    l = _lib.lib()
    assert _lib.entry("f3r_maps_colorize") is l.f3r_maps_colorize and _lib.entry("f3r_raster_triangles") is l.f3r_raster_triangles
    for name in NEW_SYMBOLS:
        with pytest.raises(_lib.F3RError, match=f"does not export {name}: rebuild it"):
            _lib.entry(name)
    cpu = torch.zeros(4, 4)
    with pytest.raises(_lib.F3RError, match="rebuild it"):
        post_ops.gtview_unproject([cpu], torch.zeros(1, 25), (0, 0, 4, 4), None, (4, 4), (0, 0, 4, 4))
    with pytest.raises(_lib.F3RError, match="rebuild it"):
        post_ops.gtview_resample([torch.zeros(4, 4, 3, dtype=torch.uint8)], (0, 0, 4, 4), None, None, (4, 4), (0, 0, 4, 4), (0, 4))
    with pytest.raises(_lib.F3RError):
        fast3r_amd.depthmap_to_camera_coordinates(cpu, np.eye(3))


def test_argument_errors_are_codes_before_any_launch(built_lib):
    l, err = built_lib, built_lib.f3r_last_error_string
    P = 0x1000

    def resample(**kw):
        a = dict(src_table=P, n_views=1, win_x=0, win_y=0, win_w=80, win_h=60, bounds_h=P, kk_h=P, ksize_h=17, res_w=42, bounds_v=P, kk_v=P,
                 ksize_v=13, res_h=32, row0=0, rows=60, crop_x=5, crop_y=0, out_w=32, out_h=32, transpose=0, img_u8=P, img=P, workspace=P,
                 workspace_bytes=1 << 20, stream=None)
        a.update(kw)
        return l.f3r_gtview_resample(*a.values())

    def unproject(**kw):
        a = dict(src_table=P, cams=P, n_views=1, win_x=0, win_y=0, win_w=80, win_h=60, nx=P, ny=P, res_w=42, res_h=32, crop_x=5, crop_y=0, out_w=32,
                 out_h=32, transpose=0, flags=3, depthmap=P, pts3d=P, valid_mask=P, flag=None, stream=None)
        a.update(kw)
        return l.f3r_gtview_unproject(*a.values())

    assert l.f3r_gtview_workspace_bytes(2, 60, 32) == 2 * 60 * 32 * 3 and l.f3r_gtview_workspace_bytes(1, 3, 5) == 48
    assert l.f3r_gtview_workspace_bytes(0, 60, 32) == 0 and l.f3r_gtview_workspace_bytes(1, 0, 32) == 0
    for name in ("src_table", "bounds_h", "kk_h", "bounds_v", "kk_v", "img_u8", "img", "workspace"):
        assert resample(**{name: None}) == -1 and b"null pointer" in err(), name
    for call in (resample, unproject):
        for n in (0, -1, 2 ** 20 + 1):
            assert call(n_views=n) == -1 and b"n_views" in err()
        for kw in (dict(win_x=-1), dict(win_y=-1), dict(win_w=0), dict(win_h=0), dict(win_x=2 ** 24)):
            assert call(**kw) == -1 and b"is not a box of a frame" in err(), kw
        for kw in (dict(crop_x=11), dict(crop_y=1), dict(out_w=0), dict(out_h=0), dict(crop_x=-1), dict(crop_y=-1), dict(out_w=38)):
            assert call(**kw) == -1 and b"leaves the resized 42 x 32 picture" in err(), kw
        for t in (2, -1):
            assert call(transpose=t) == -1 and b"transpose" in err()
    for kw in (dict(row0=-1), dict(rows=0), dict(row0=1), dict(rows=61)):
        assert resample(**kw) == -1 and b"leave the window's 60 rows" in err(), kw
    assert resample(workspace_bytes=60 * 32 * 3 - 1) == -1 and b"f3r_gtview_workspace_bytes" in err()
    assert resample(workspace=P + 8) == -1 and b"16-byte aligned" in err()
    assert resample(res_w=0) == -1 and resample(ksize_v=0) == -1
    assert unproject(src_table=None) == -1 and unproject(cams=None) == -1 and b"null src_table or cams" in err()
    assert unproject(depthmap=None, pts3d=None, valid_mask=None) == -1 and b"no output" in err()
    assert unproject(nx=None) == -1 and b"given together" in err()
    assert unproject(nx=None, ny=None) == -1 and b"without nearest tables" in err()
    for flags in (4, 8, -1):
        assert unproject(flags=flags) == -1 and b"unknown flags" in err()
