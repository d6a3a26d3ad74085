"""The point-splat renderer, the parts that need no GPU: the signature is the notebook's, the numpy restatement (tests/render_ref.py)
against pictures worked out by hand, its sx / sy form against pyrender's 4 x 4 matrix multiplied out, the two cameras (the notebook's
bird's-eye quirk, the pinhole's pixel convention), and the library side: symbols, the version gate, build flags, argument errors."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"f3r_render_clear": 4, "f3r_render_splat": 10, "f3r_render_resolve": 9, "f3r_render_center": 5}
IDENTITY = R.Cam((1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0), 1.0, 1.0, 0.0, 0.0, 0.05)


def test_signature_is_the_notebooks():
    import fast3r_amd
    want = [("preds", inspect.Parameter.empty), ("views", inspect.Parameter.empty), ("output_dir", "./output"), ("point_size", 5.0),
            ("min_conf_thr_percentile", 0)]
    params = list(inspect.signature(fast3r_amd.render_cumulative_pts3d_viz).parameters.values())
    assert [(p.name, p.default) for p in params if p.kind == p.POSITIONAL_OR_KEYWORD] == want
    assert {p.name: p.default for p in params if p.kind == p.KEYWORD_ONLY} == {"sample": 0, "width": 1920, "height": 1080, "camera": None,
                                                                              "frames": None, "return_frames": False}
    sig = inspect.signature(fast3r_amd.render_points)
    assert list(sig.parameters)[:3] == ["points", "colors", "camera"]
    assert {k: p.default for k, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY} == {
        "width": 1920, "height": 1080, "point_size": 5.0, "background": (255, 255, 255), "segments": None, "return_depth": False}
    for name in ("Camera", "birdseye_camera", "pinhole_camera"):
        assert callable(getattr(fast3r_amd, name))
    assert list(inspect.signature(fast3r_amd.pinhole_camera).parameters)[:5] == ["c2w", "focal", "pp", "H", "W"]
    sig = inspect.signature(fast3r_amd.birdseye_camera)
    assert list(sig.parameters)[:3] == ["center", "min_bound", "max_bound"]
    assert sig.parameters["yfov"].default == math.pi / 3 and sig.parameters["aspect"].default == 16 / 9


def test_no_cpu_path(built_lib):
    import fast3r_amd
    from fast3r_amd._lib import F3RError
    p, c = torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.uint8)
    cam = fast3r_amd.birdseye_camera([0, 0, 0], [-1, -1, -1], [1, 1, 1])
    with pytest.raises(F3RError, match="ROCm device"):
        fast3r_amd.render_points(p, c, cam, width=8, height=8)
    src = open(os.path.join(ROOT, "fast3r_amd", "render.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(pyrender|OpenGL|trimesh)", src, flags=re.M)


# ------------------------------------------------------------------------------------------------------------------- the restatement
def square(rows, cols, H=5, W=7):
    want = np.full((H, W, 3), 255, np.uint8)
    want[rows[0]:rows[1], cols[0]:cols[1]] = (10, 20, 30)
    return want


@pytest.mark.parametrize("size,rows,cols", [(1, (2, 3), (3, 4)), (4, (1, 5), (1, 5)), (5, (0, 5), (1, 6)), (2.5, (1, 4), (2, 5))])
def test_restatement_against_hand_computed_pictures(size, rows, cols):
    """One point on the axis of an identity camera, 7 x 5 viewport: x_w = 3.5, y_w = 2.5.  A pixel is covered iff x_w - s / 2 <= centre <
    x_w + s / 2.  s = 1: [3, 4) x [2, 3) holds the centres 3.5 and 2.5.  s = 4: [1.5, 5.5) holds 1.5 .. 4.5 -- columns 1 .. 4 -- and [0.5,
    4.5) the window rows 0 .. 3, which are image rows 4 .. 1: the half-open test puts the even square on the lower-left side.  s = 5:
    [1, 6) -> columns 1 .. 5, [0, 5) -> every row.  s = 2.5: [2.25, 4.75) -> columns 2 .. 4, [1.25, 3.75) -> window rows 1 .. 3."""
    p, c = np.array([[0, 0, -1]], np.float32), np.array([[10, 20, 30]], np.uint8)
    image, depth = R.render(p, c, IDENTITY, 7, 5, size)
    assert np.array_equal(image, square(rows, cols))
    assert np.array_equal(np.isinf(depth), (image == 255).all(-1)) and set(depth[np.isfinite(depth)].tolist()) == {1.0}


def test_restatement_rules():
    c = np.array([[1, 1, 1], [2, 2, 2], [3, 3, 3]], np.uint8)
    pic = lambda p, **kw: R.render(np.array(p, np.float32), c[:len(p)], IDENTITY, 7, 5, 1, **kw)[0]   # noqa: E731
    assert pic([[0, 0, -2], [0, 0, -1]])[2, 3].tolist() == [2, 2, 2]                     # the nearer point, whatever the order
    assert pic([[0, 0, -1], [0, 0, -2]])[2, 3].tolist() == [1, 1, 1]
    assert pic([[0, 0, -1], [0, 0, -1]])[2, 3].tolist() == [1, 1, 1]                     # a tie: the lowest index
    assert (pic([[0, 0, 1], [0, 0, -0.04], [np.nan, 0, -1]]) == 255).all()               # behind, nearer than znear, NaN
    assert (pic([[0, 0, -0.05]]) != 255).any()                                           # d = fp64(fp32(0.05)) >= 0.05
    assert (pic([[1.01, 0, -1]]) == 255).all() and (pic([[1.0, 0, -1]])[:, 6] == 1).any()   # |p_x| <= d: the frustum's side is inside
    assert pic([[-0.9, -0.9, -1]])[4, 0].tolist() == [1, 1, 1]                           # (-1, -1) is the lower left: the last image row
    assert (pic([[-1.0, -1.0, -1]]) == 255).all()                                        # [-0.5, 0.5) holds no pixel centre: half-open
    frames = R.render(np.array([[0, 0, -2], [0, 0, -1]], np.float32), c[:2], IDENTITY, 7, 5, 1, segments=[1, 1, 2])
    assert [f[0][2, 3, 0] for f in frames] == [1, 1, 2]
    assert R.render(np.array([[0, 0, -1]], np.float32), c[:1], IDENTITY, 7, 5, 1, background=(1, 2, 3))[0][0, 0].tolist() == [1, 2, 3]


def test_sx_sy_form_against_the_projection_matrix():
    """the sx / sy arithmetic and pyrender's 4 x 4 matrices multiplied out agree on what is inside and on where it lands"""
    rs = np.random.RandomState(0)
    p = (rs.randn(4000, 3) * [3, 3, 4] + [0.5, -1, 0]).astype(np.float32)
    lo, hi = p.min(0), p.max(0)
    cam = R.birdseye(R.center(p), lo / 8, hi / 8)                                         # a camera inside the cloud: points on every side of it
    W, H = 64, 36
    drawn, xw, yw, df = R.project(p, cam, W, H)
    inside, mx, my, w = R.window_by_matrices(p, cam.view, R.perspective_matrix(np.pi / 3, 16 / 9, 0.05), W, H)
    assert 100 < drawn.sum() < len(p) and np.array_equal(drawn, inside)                   # no point of this cloud sits on a frustum plane
    assert np.abs(xw[drawn] - mx[drawn]).max() < 1e-9 and np.abs(yw[drawn] - my[drawn]).max() < 1e-9
    assert np.array_equal(df[drawn], w[drawn].astype(np.float32))
    assert cam.sx == 1 / (16 / 9 * np.tan(np.pi / 6)) and cam.sy == 1 / np.tan(np.pi / 6)


# ------------------------------------------------------------------------------------------------------------------- cameras
def test_birdseye_camera_keeps_the_notebooks_quirk():
    import fast3r_amd
    center, lo, hi = np.array([1.0, 2.0, 3.0]), np.array([-1.0, 0.0, 2.0], np.float32), np.array([3.0, 3.0, 3.5], np.float32)
    pose = R.notebook_node_pose(center, lo, hi)                                           # what pyrender is given as the camera's pose
    assert np.array_equal(pose[:3, :3], np.diag([-1.0, -1.0, 1.0]))                       # its axes: turned by 180 degrees about z
    assert pose[:3, 3].tolist() == [1.0, -2.0, 3.0 + 2 * 4.0]                             # it sits at (c_x, -c_y, c_z + 2 max_extent)
    cam = fast3r_amd.birdseye_camera(center, lo, hi)
    want = R.birdseye(center, lo, hi)
    assert np.array_equal(np.array(cam.view), np.array(want.view)) and (cam.sx, cam.sy, cam.cx, cam.cy, cam.znear) == want[1:]
    V = np.array(cam.view).reshape(3, 4)
    assert np.array_equal(V, np.array([[-1.0, 0, 0, 1.0], [0, -1.0, 0, -2.0], [0, 0, 1.0, -11.0]]))
    # the cloud's centre lands 2 c_y off the picture's middle and world +x points to the left
    _, xw, yw, df = R.project(np.array([[1, 2, 3], [2, 2, 3]], np.float32), want, 64, 36)
    assert xw[0] == 32.0 and yw[0] == (want.sy * -4.0 / 8.0 + 1.0) * 18.0 and xw[1] < xw[0] and df[0] == 8.0
    centred = fast3r_amd.birdseye_camera([1.0, 0.0, 3.0], lo, hi)
    assert R.project(np.array([[1, 0, 3]], np.float32), centred, 64, 36)[1:3] == (32.0, 18.0)
    assert fast3r_amd.birdseye_camera(center, lo, hi, yfov=1.0, aspect=2.0).sx == 1 / (2.0 * math.tan(0.5))


def test_birdseye_camera_of_a_cloud_without_extent():
    """max_extent = 0 puts the camera on the centre: the notebook's forward vector is 0 / 0 and every entry of its matrix NaN"""
    import fast3r_amd
    assert np.isnan(R.notebook_node_pose([1.0, 2.0, 3.0], [1, 2, 3], [1, 2, 3])).any()
    with pytest.raises(ValueError, match="divides 0 by 0"):
        fast3r_amd.birdseye_camera([1.0, 2.0, 3.0], [1, 2, 3], [1, 2, 3])
    with pytest.raises(ValueError, match="divides 0 by 0"):                               # an extent that the centre's magnitude swallows
        fast3r_amd.birdseye_camera([0.0, 0.0, 1e30], [0, 0, 0], [1, 1, 1])


def test_pinhole_camera_puts_the_optical_axis_on_the_principal_point():
    import fast3r_amd
    H, W, f, pp = 8, 12, 10.0, (7.0, 2.0)
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])                           # a rotation, and a position
    c2w[:3, 3] = [0.5, -2.0, 1.0]
    cam = fast3r_amd.pinhole_camera(c2w, f, pp, H, W)
    on_axis = (c2w[:3, 3] + 3.0 * c2w[:3, 2]).astype(np.float32)[None]                    # 3 units along the camera's z
    drawn, xw, yw, df = R.project(on_axis, cam, W, H)
    assert drawn[0] and df[0] == 3.0 and abs(xw[0] - (pp[0] + 0.5)) < 1e-12 and abs(yw[0] - (H - 0.5 - pp[1])) < 1e-12
    image, _ = R.render(on_axis, np.array([[9, 9, 9]], np.uint8), cam, W, H, 1)
    assert np.argwhere((image == 9).all(-1)).tolist() == [[2, 7]]                         # row pp_y, column pp_x
    # a point one pixel to the right and two down in the image: x_cam = 1 * z / f, y_cam = 2 * z / f (y down)
    off = (c2w[:3, 3] + 3.0 * c2w[:3, 2] + 0.3 * c2w[:3, 0] + 0.6 * c2w[:3, 1]).astype(np.float32)[None]
    image, _ = R.render(off, np.array([[9, 9, 9]], np.uint8), cam, W, H, 1)
    assert np.argwhere((image == 9).all(-1)).tolist() == [[4, 8]]
    assert fast3r_amd.pinhole_camera(torch.eye(4)[:3], f, (W / 2 - 0.5, H / 2 - 0.5), H, W).cx == 0.0
    with pytest.raises(ValueError, match="not finite"):
        fast3r_amd.pinhole_camera(np.eye(4), float("nan"), pp, H, W)


# ------------------------------------------------------------------------------------------------------------------- the library
def test_new_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "f3r.h")).read(), flags=re.S)
    assert built_lib.f3r_version() == 430 and _lib.ABI_VERSION == 410
    for name, arity in NEW_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity, name
        assert _lib.SYMBOL_SINCE_430[name] == 430 and name not in _lib.SYMBOL_SINCE and _lib.symbol_since(name) == 430
        assert getattr(built_lib, name).argtypes == _lib.SYMBOLS[name][1] and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_SINCE_430) == set(NEW_SYMBOLS) and _lib.symbol_since("f3r_cloud_fps") == 420 and _lib.symbol_since("f3r_gemm") == 0
    raw = open(os.path.join(ROOT, "include", "f3r.h")).read()
    assert int(re.search(r"#define F3R_RENDER_CENTER_PARTS (\d+)", raw).group(1)) == _lib.RENDER_CENTER_PARTS


def test_build_script_carries_the_file_and_the_flag():
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_render ] && extra="-ffp-contract=off"' in build and '"$here"/obj/f3r_render.o' in build
    assert re.search(r"^for f in .*\bf3r_render\b.*; do$", build, flags=re.M)
    assert os.path.exists(os.path.join(ROOT, "fast3r_amd", "csrc", "f3r_render.hip"))


def test_render_entry_points_ask_a_420_library_to_rebuild(built_lib, monkeypatch):
    from fast3r_amd import _lib, post_ops
    monkeypatch.setattr(_lib, "library_version", lambda: 420)
    for name in NEW_SYMBOLS:
        with pytest.raises(_lib.F3RError, match=f"version 420, {name} needs >= 430: rebuild it"):
            _lib.entry(name)
    assert _lib.entry("f3r_cloud_fps") is built_lib.f3r_cloud_fps                         # an entry point of the gated version itself
    cpu = torch.zeros(4, 3)
    for call in (lambda: post_ops.render_splat(cpu, 0, 4, [0.0] * 17, 1.0, cpu), lambda: post_ops.render_resolve(cpu, cpu),
                 lambda: post_ops.render_center(cpu), lambda: post_ops.render_keys(4, 4, "cpu")):
        with pytest.raises(_lib.F3RError, match="rebuild it"):                            # before the wrapper looks at a tensor
            call()
    monkeypatch.undo()
    assert _lib.entry("f3r_render_splat") is built_lib.f3r_render_splat


def test_a_420_library_still_loads_without_the_renderer(tmp_path, monkeypatch):
    import subprocess
    from fast3r_amd import _lib
    names = [n for n in _lib.SYMBOLS if n not in _lib.SYMBOL_SINCE_430 and n not in ("f3r_version", "f3r_sizeof")]
    src, so = tmp_path / "stub.c", tmp_path / "libf3r_hip.so"
    sizes = (ctypes.sizeof(_lib.GemmArgs), ctypes.sizeof(_lib.AttnArgs), ctypes.sizeof(_lib.AttnF32Args))
    src.write_text("int f3r_version(void) { return 420; }\nunsigned long f3r_sizeof(int w) { return w == 0 ? %d : w == 1 ? %d : w == 2 ? %d : 0; }\n"
                   % sizes + "".join("int %s(void) { return 0; }\n" % n for n in names))
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    l = _lib.lib()
    assert l.f3r_version() == 420 and _lib.entry("f3r_cloud_bounds") is l.f3r_cloud_bounds
    with pytest.raises(_lib.F3RError, match="version 420, f3r_render_splat needs >= 430: rebuild it"):
        _lib.entry("f3r_render_splat")


def test_argument_errors_are_codes_before_any_launch(built_lib):
    l, err = built_lib, built_lib.f3r_last_error_string
    P = 0x1000
    cam = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 1.0, 1.0, 0.0, 0.0, 0.05]
    C = lambda v=cam: (ctypes.c_double * 17)(*v)   # noqa: E731
    changed = lambda k, v: C(cam[:k] + [v] + cam[k + 1:])   # noqa: E731
    assert l.f3r_render_clear(None, 4, 4, None) == -1 and b"null" in err()
    for W, H in ((0, 4), (4, 0), (-1, 4), (2 ** 16, 2 ** 15), (2 ** 30, 2)):
        assert l.f3r_render_clear(P, W, H, None) == -1 and b"W H < 2^31" in err()
        assert l.f3r_render_splat(P, 10, 0, 10, C(), 1.0, W, H, P, None) == -1 and b"W H < 2^31" in err()
        assert l.f3r_render_resolve(P, P, 10, W, H, 0, P, None, None) == -1 and b"W H < 2^31" in err()
    for args in ((None, 10, 0, 10, C(), 1.0, 4, 4, P, None), (P, 10, 0, 10, None, 1.0, 4, 4, P, None),
                 (P, 10, 0, 10, C(), 1.0, 4, 4, None, 1, None)):
        assert l.f3r_render_splat(*args) == -1 and b"null" in err()
    for n in (0, -1, 2 ** 32, 2 ** 40):
        assert l.f3r_render_splat(P, n, 0, 0, C(), 1.0, 4, 4, P, None) == -1 and b"2^32" in err()
        assert l.f3r_render_resolve(P, P, n, 4, 4, 0, P, None, None) == -1 and b"2^32" in err()
        assert l.f3r_render_center(P, n, P, P, None) == -1 and b"2^32" in err()
    for n0, n1 in ((5, 4), (-1, 4), (0, 11)):
        assert l.f3r_render_splat(P, 10, n0, n1, C(), 1.0, 4, 4, P, None) == -1 and b"n0 <= n1" in err()
    for size in (0.0, -1.0, float("nan"), float("inf")):
        assert l.f3r_render_splat(P, 10, 0, 10, C(), size, 4, 4, P, None) == -1 and b"point_size" in err()
    for znear in (0.0, -0.05):
        assert l.f3r_render_splat(P, 10, 0, 10, changed(16, znear), 1.0, 4, 4, P, None) == -1 and b"znear" in err()
    for k in (0, 3, 11, 12, 13, 14, 15, 16):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert l.f3r_render_splat(P, 10, 0, 10, changed(k, bad), 1.0, 4, 4, P, None) == -1 and b"camera[%d] is not finite" % k in err()
    assert l.f3r_render_splat(P, 10, 3, 3, C(), 1.0, 4, 4, P, None) == 0              # an empty range launches nothing
    assert l.f3r_render_resolve(None, P, 10, 4, 4, 0, P, None, None) == -1 and l.f3r_render_resolve(P, None, 10, 4, 4, 0, P, None, None) == -1
    assert l.f3r_render_resolve(P, P, 10, 4, 4, 0, None, None, None) == -1 and b"null" in err()
    assert l.f3r_render_resolve(P, P, 10, 4, 4, 1 << 24, P, None, None) == -1 and b"background" in err()
    assert l.f3r_render_center(None, 10, P, P, None) == -1 and l.f3r_render_center(P, 10, None, P, None) == -1
    assert l.f3r_render_center(P, 10, P, None, None) == -1 and b"null" in err()


def test_wrappers_refuse_before_the_library_is_asked_for_work(built_lib):
    """host-side refusals of render_points that need no device: they come after the device check, so they are exercised through the
    camera constructors and the segment check's arithmetic here and on the GPU in tests/test_render_gpu.py"""
    import fast3r_amd
    from fast3r_amd import render
    cam = fast3r_amd.birdseye_camera([0, 0, 0], [-1, -1, -1], [1, 1, 1])
    assert len(cam.words()) == 17 and cam.words()[12:] == [cam.sx, cam.sy, 0.0, 0.0, 0.05]
    for bad in ((0, 4, 1.0), (4, 0, 1.0), (2 ** 16, 2 ** 15, 1.0), (4, 4, 0.0), (4, 4, float("inf")), (4, 4, float("nan"))):
        with pytest.raises(ValueError):
            render._checked(*bad, cam, "t")
    with pytest.raises(ValueError, match="Camera"):
        render._checked(4, 4, 1.0, (1, 2, 3), "t")
    with pytest.raises(ValueError, match="znear"):
        fast3r_amd.birdseye_camera([0, 0, 0], [-1, -1, -1], [1, 1, 1], znear=0.0)
