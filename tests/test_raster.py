"""The triangle rasteriser, the parts that need no GPU: the numpy restatement (tests/raster_ref.py) against pictures worked out by hand,
the recipes' stated properties, the library side (symbols, the presence gate, build flags, argument errors), and the host geometry of
the scene's cameras (auto_cam_size against scipy, the pyramid's invariants)."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import raster_cases as C
import raster_ref as RR
import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"f3r_raster_workspace_bytes": 1, "f3r_raster_triangles": 16}


def keys_of(v, f, W, H, cam=C.IDENTITY, **kw):
    keys = np.full((H, W), RR.EMPTY, dtype=np.uint64)
    s = RR.raster(keys, v, f, cam, **kw)
    return keys, s


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("n", [4, 7])
def test_quad_split_along_a_diagonal_through_pixel_centres(n):
    """The square [0, n]^2 at depth 2, split along the diagonal from (0, 0) to (n, n), which passes through the centres (i + 0.5, i + 0.5):
    every centre of the n x n pixels is covered, the diagonal's by both triangles (edges are inclusive), the others by one; the depth is
    exactly 2 (the clamp); both windings cover the same pixels."""
    W = H = 8
    quad = [[(0, 0, 2), (n, 0, 2), (n, n, 2)], [(0, 0, 2), (n, n, 2), (0, n, 2)]]
    v, f = C.window_mesh(quad, W, H)
    per_face = []
    for k in range(2):
        keys, s = keys_of(v, f, W, H, f0=k, f1=k + 1)
        per_face.append(keys != RR.EMPTY)
        assert set((keys[keys != RR.EMPTY] >> np.uint64(32)).tolist()) == {int(np.float32(2.0).view(np.uint32))}
    inside = np.zeros((H, W), bool)
    inside[:n, :n] = True
    assert np.array_equal(per_face[0] | per_face[1], inside)
    assert np.array_equal(per_face[0] & per_face[1], np.eye(H, W, dtype=bool) & inside)
    keys, _ = keys_of(v, f, W, H)
    assert np.array_equal((keys & np.uint64(0xffffffff))[np.eye(H, W, dtype=bool) & inside], np.zeros(n, np.uint64))   # the lower face wins the tie
    flipped, _ = keys_of(v, f[:, ::-1].copy(), W, H)
    assert np.array_equal(flipped, keys)
    image, depth = R.resolve(keys, C.colors_of(2))
    assert image.shape == (H, W, 3) and set(depth[np.isfinite(depth)].tolist()) == {2.0}
    assert (image[H - n:, :n] != 255).any(-1).all() and (image[:H - n] == 255).all()      # window row 0 is the last image row


def test_single_triangle_recipes_have_their_stated_properties():
    W, H = 64, 48
    cases = C.single_triangles(W, H)
    covered = {}
    for name, tri in cases.items():
        v, f = C.window_mesh([tri], W, H)
        keys, s = keys_of(v, f, W, H)
        covered[name] = keys != RR.EMPTY
        assert len(s.f) == 1, name
    assert covered["no centre"].sum() == 0 and covered["wholly outside"].sum() == 0
    assert covered["one centre"].sum() == 1 and covered["one centre"][7, 10]
    assert covered["whole viewport"].all() and covered["a million pixels outside"].sum() > 0
    v, f = C.window_mesh([cases["vertex on a centre"]], W, H)
    s = RR.Setup(v, f, 0, 1, C.IDENTITY, W, H)
    assert (s.x[0, 0], s.y[0, 0]) == (10.5, 7.5) and covered["vertex on a centre"][7, 10]  # exactly on the centre, and covered: inclusive
    v, f = C.window_mesh([cases["edge through a row of centres"]], W, H)
    s = RR.Setup(v, f, 0, 1, C.IDENTITY, W, H)
    assert s.y[0, 0] == s.y[0, 1] == 4.5 and covered["edge through a row of centres"][4, 3:21].all()
    assert not covered["edge through a row of centres"][3].any()
    assert covered["edge through a column of centres"][2:19, 6].all() and not covered["edge through a column of centres"][:, 5].any()
    for name in cases:
        if name.startswith("across"):
            assert 0 < covered[name].sum() < 60, name                                     # clipped by the viewport, not dropped
    for W, H in C.VIEWPORTS:
        v, f, drawn = C.skipped_mesh(W, H)
        keys, s = keys_of(v, f, W, H)
        assert s.f.tolist() == [0] and drawn == 1 and set((keys[keys != RR.EMPTY] & np.uint64(0xffffffff)).tolist()) == {0}


def test_box_recipe_straddles_the_threshold_and_both_loops_agree():
    from fast3r_amd import _lib
    small = _lib.RASTER_SMALL_PIXELS
    for W, H in C.VIEWPORTS:
        v, f, want = C.box_recipe(W, H, small)
        keys, s = keys_of(v, f, W, H, small=small)
        assert s.pixels.tolist() == want == [small - 1, small, small + 1]
        for other in (0, 10 ** 6):                                                        # the restatement's two loop arrangements
            again, _ = keys_of(v, f, W, H, small=other)
            assert np.array_equal(again, keys)
    v, f = C.random_triangles(300, 3, 37, 23, size=6.0)
    a, s = keys_of(v, f, 37, 23, small=0)
    b, _ = keys_of(v, f, 37, 23, small=10 ** 6)
    assert np.array_equal(a, b) and (s.pixels > small).any() and (s.pixels <= small).any() and (a != RR.EMPTY).mean() > 0.5


def test_depth_is_perspective_correct_and_sub_ranges_compose():
    """the midpoint in the window of an edge from depth 1 to depth 3 lies at depth 1 / ((1 / 1 + 1 / 3) / 2) = 1.5, not 2"""
    W, H = 64, 48
    v, f = C.window_mesh([[(2.5, 4.5, 1), (22.5, 4.5, 3), (12.5, 20.5, 1)]], W, H)
    keys, _ = keys_of(v, f, W, H)
    depth = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert abs(depth[4, 12] - 1.5) < 1e-6 and depth[4, 2] == 1.0 and depth[4, 22] == 3.0
    v, f = C.random_triangles(100, 5, W, H, size=5.0)
    whole, _ = keys_of(v, f, W, H, index_base=7)
    parts = np.full((H, W), RR.EMPTY, dtype=np.uint64)
    for f0, f1 in ((60, 100), (0, 1), (1, 60)):
        RR.raster(parts, v, f, C.IDENTITY, f0=f0, f1=f1, index_base=7)
    assert np.array_equal(parts, whole) and (whole[whole != RR.EMPTY] & np.uint64(0xffffffff)).min() >= 7


# ------------------------------------------------------------------------------------------------------------------- the library
def test_signatures():
    import fast3r_amd
    sig = inspect.signature(fast3r_amd.render_mesh)
    assert list(sig.parameters)[:2] == ["mesh", "camera"] and sig.parameters["camera"].default is None
    assert {k: p.default for k, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY} == {
        "points": None, "colors": None, "point_size": 5.0, "width": 1920, "height": 1080, "background": (255, 255, 255), "return_depth": False}
    sig = inspect.signature(fast3r_amd.plot_3d_points_with_estimated_camera_poses)
    assert [(p.name, p.default) for p in sig.parameters.values() if p.kind == p.POSITIONAL_OR_KEYWORD][2:] == [
        ("title", "3D Points and Camera Poses"), ("flip_axes", False), ("min_conf_thr_percentile", 80), ("export_ply_path", None),
        ("export_html_path", None)]
    assert {k: p.default for k, p in sig.parameters.items() if p.kind == p.KEYWORD_ONLY} == {
        "sample": 0, "output_path": None, "camera": None, "width": 1920, "height": 1080, "point_size": 1.0, "niter_PnP": 10}
    sig = inspect.signature(fast3r_amd.camera_meshes)
    assert list(sig.parameters)[:2] == ["poses_c2w", "focals"] and sig.parameters["cam_size"].default == 0.03
    assert sig.parameters["image_cells"].default == 64
    assert list(inspect.signature(fast3r_amd.SceneViz.add_camera).parameters) == ["self", "pose_c2w", "focal", "color", "image", "imsize", "cam_size"]
    assert list(inspect.signature(fast3r_amd.SceneViz.add_pointcloud).parameters) == ["self", "pts3d", "color", "mask"]
    assert len(fast3r_amd.CAM_COLORS) == 11 and fast3r_amd.CAM_COLORS[4] == (255, 204, 0)
    with pytest.raises(NotImplementedError, match="render"):
        fast3r_amd.SceneViz().show()
    with pytest.raises(ValueError, match="HTML"):
        fast3r_amd.plot_3d_points_with_estimated_camera_poses([], [], export_html_path="scene.html")
    src = open(os.path.join(ROOT, "fast3r_amd", "viz.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(pyrender|OpenGL|trimesh|scipy|plotly)", src, flags=re.M)


def test_new_symbols_are_declared_exported_and_bound(built_lib):
    from fast3r_amd import _lib
    raw = open(os.path.join(ROOT, "include", "f3r.h")).read()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert built_lib.f3r_version() == 430 and _lib.ABI_VERSION == 410
    for name, arity in NEW_SYMBOLS.items():
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity, name
        assert _lib.symbol_since(name) == 0 and name in _lib.SYMBOL_IF_PRESENT
        assert getattr(built_lib, name).argtypes == _lib.SYMBOLS[name][1] and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_IF_PRESENT) == set(NEW_SYMBOLS)
    assert int(re.search(r"#define F3R_RASTER_SMALL_PIXELS (\d+)", raw).group(1)) == _lib.RASTER_SMALL_PIXELS
    assert "triangle rasteriser" in raw.lower()
    assert built_lib.f3r_raster_workspace_bytes(1000) >= 4000 and built_lib.f3r_raster_workspace_bytes(0) == 0
    assert built_lib.f3r_raster_workspace_bytes(-1) == 0 and built_lib.f3r_raster_workspace_bytes(2 ** 31) == 0


def test_build_script_carries_the_file_and_the_flag():
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_raster ] && extra="-ffp-contract=off"' in build and '"$here"/obj/f3r_raster.o' in build
    assert re.search(r"^for f in .*\bf3r_raster\b.*; do$", build, flags=re.M) and "f3r_pixel.h" in build
    csrc = os.path.join(ROOT, "fast3r_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "f3r_raster.hip"))
    for name in ("f3r_raster.hip", "f3r_render.hip"):                                     # one first_center_ge, in the shared header
        src = open(os.path.join(csrc, name)).read()
        assert '#include "f3r_pixel.h"' in src and not re.search(r"int\s+first_center_ge\s*\(", src), name
    assert len(re.findall(r"int\s+first_center_ge\s*\(", open(os.path.join(csrc, "f3r_pixel.h")).read())) == 1


def test_a_library_without_the_rasteriser_still_loads(tmp_path, monkeypatch):
    """a library built before the rasteriser: version 430, every other symbol.  lib() loads it, an older entry point works, and the
    rasteriser's names ask for a rebuild -- also through the wrappers, before they look at a tensor"""
    from fast3r_amd import _lib, post_ops
    import fast3r_amd
    names = [n for n in _lib.SYMBOLS if n not in _lib.SYMBOL_IF_PRESENT and n not in ("f3r_version", "f3r_sizeof")]
    src, so = tmp_path / "stub.c", tmp_path / "libf3r_hip.so"
    sizes = (ctypes.sizeof(_lib.GemmArgs), ctypes.sizeof(_lib.AttnArgs), ctypes.sizeof(_lib.AttnF32Args))
    src.write_text("int f3r_version(void) { return 430; }\nunsigned long f3r_sizeof(int w) { return w == 0 ? %d : w == 1 ? %d : w == 2 ? %d : 0; }\n"
                   % sizes + "".join("int %s(void) { return 0; }\n" % n for n in names))
    subprocess.run(["gcc", "-shared", "-fPIC", str(src), "-o", str(so)], check=True)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(so))
    l = _lib.lib()
    assert l.f3r_version() == 430 and _lib.entry("f3r_cloud_bounds") is l.f3r_cloud_bounds
    assert _lib.entry("f3r_render_splat") is l.f3r_render_splat
    for name in NEW_SYMBOLS:
        with pytest.raises(_lib.F3RError, match=f"does not export {name}: rebuild it"):
            _lib.entry(name)
    cpu = torch.zeros(4, 3)
    for call in (lambda: post_ops.raster_triangles(cpu, cpu, [0.0] * 17, cpu), lambda: fast3r_amd.render_mesh({}),
                 lambda: fast3r_amd.camera_meshes([np.eye(4)]), lambda: post_ops.raster_workspace("cpu", 10)):
        with pytest.raises(_lib.F3RError, match="rebuild it"):
            call()


def test_no_cpu_path(built_lib):
    from fast3r_amd import _lib, post_ops
    import fast3r_amd
    v, f, c = torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 3, dtype=torch.uint8)
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        post_ops.raster_triangles(v, f, [0.0] * 17, torch.zeros(4, 4, dtype=torch.int64))
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.render_mesh(dict(vertices=v, faces=f, face_colors=c), width=8, height=8)
    with pytest.raises(ValueError, match="Mesh or a dict"):
        fast3r_amd.render_mesh([1, 2, 3])


def test_argument_errors_are_codes_before_any_launch(built_lib):
    l, err = built_lib, built_lib.f3r_last_error_string
    P = 0x1000
    cam = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 1.0, 1.0, 0.0, 0.0, 0.05]
    C17 = lambda v=cam: (ctypes.c_double * 17)(*v)   # noqa: E731
    changed = lambda k, v: C17(cam[:k] + [v] + cam[k + 1:])   # noqa: E731
    need = l.f3r_raster_workspace_bytes(100)

    def call(**kw):
        a = dict(vertices=P, nv=10, faces=P, index_dtype=1, nf=20, f0=0, f1=20, index_base=0, camera=C17(), W=4, H=4, keys=P, workspace=P,
                 workspace_bytes=need, faces_per_launch=100, stream=None)
        a.update(kw)
        return l.f3r_raster_triangles(*a.values())

    for name in ("vertices", "faces", "camera", "keys", "workspace"):
        assert call(**{name: None}) == -1 and b"null" in err(), name
    for W, H in ((0, 4), (4, 0), (-1, 4), (2 ** 16, 2 ** 15), (2 ** 30, 2)):
        assert call(W=W, H=H) == -1 and b"W H < 2^31" in err()
    for f0, f1, nf in ((5, 4, 20), (-1, 4, 20), (0, 21, 20), (0, 0, -1)):
        assert call(f0=f0, f1=f1, nf=nf) == -1 and b"f0 <= f1 <= nf" in err()
    for base, nf in ((2 ** 32 - 20, 20), (-1, 20), (2 ** 32, 0), (0, 2 ** 32)):
        assert call(index_base=base, nf=nf, f1=0) == -1 and b"index_base" in err()
    assert call(index_base=2 ** 32 - 21, f1=0) == 0                                       # the largest base that fits, and an empty range
    assert call(nv=0) == -1 and b"nv" in err()
    assert call(index_dtype=2) == -1 and b"index_dtype" in err()
    for znear in (0.0, -0.05):
        assert call(camera=changed(16, znear)) == -1 and b"znear" in err()
    for k in (0, 3, 11, 12, 13, 14, 15, 16):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert call(camera=changed(k, bad)) == -1 and b"camera[%d] is not finite" % k in err()
    for fpl in (0, -5, 2 ** 31):
        assert call(faces_per_launch=fpl) == -1 and b"faces_per_launch" in err()
    assert call(workspace_bytes=need - 1) == -1 and b"workspace" in err()
    assert call(faces_per_launch=101) == -1 and b"workspace" in err()                     # sized for 100 faces a launch
    assert call(workspace=P + 4) == -1 and b"aligned" in err()
    assert call(f0=7, f1=7) == 0                                                          # an empty range launches nothing


# ------------------------------------------------------------------------------------------------------------------- cameras of a scene
def test_auto_cam_size_matches_scipy_to_the_last_bit():
    """pdist's Euclidean distance is sqrt of the squared differences added in coordinate order, and np.median of the condensed vector is
    what the reference calls: the same fp64 operations in the same order, so the comparison is exact -- no ulp of slack."""
    from scipy.spatial.distance import pdist
    import fast3r_amd
    for poses in C.pose_sets():
        want = 0.1 * np.median(pdist([p[:3, 3] for p in poses]))
        assert fast3r_amd.auto_cam_size(poses) == want
        assert fast3r_amd.auto_cam_size([torch.from_numpy(p) for p in poses]) == want
        assert np.array_equal(RR.pdist(poses[:, :3, 3]), pdist(poses[:, :3, 3]))
    assert np.isnan(fast3r_amd.auto_cam_size([np.eye(4)]))


def random_pose(seed):
    rs = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rs.randn(3, 3))
    pose = np.eye(4)
    pose[:3, :3] = q * np.sign(np.linalg.det(q))
    pose[:3, 3] = rs.randn(3)
    return pose


def test_camera_vertices_and_faces_invariants():
    from fast3r_amd import viz
    for seed, (H, W, focal, cam_size) in enumerate([(6, 8, 7.0, 0.03), (48, 64, 70.0, 0.2), (9, 5, 4.0, 1.0), (5, 5, 5.5, 0.05)]):
        pose = random_pose(seed)
        grid = viz.image_grid(H, W, 4)
        v = viz.camera_vertices(pose, H, W, focal, cam_size, grid)
        assert v.shape == (15 + (grid[0] + 1) * (grid[1] + 1), 3) and v.dtype == np.float64
        assert np.allclose(v[0], pose[:3, 3], atol=1e-15) and np.allclose(v[10], pose[:3, 3], atol=1e-15)   # the apex is the camera centre
        local = (v - pose[:3, 3]) @ pose[:3, :3]                                          # back into the camera's frame
        u, w = focal * local[1:5, 0] / local[1:5, 2] + W / 2, focal * local[1:5, 1] / local[1:5, 2] + H / 2
        assert np.allclose(u, [0, W, W, 0], atol=1e-9) and np.allclose(w, [0, 0, H, H], atol=1e-9)   # corners onto the image's corners
        assert np.allclose(local[1:5, 2], focal * cam_size / H) and np.allclose(np.ptp(local[1:5, 1]), cam_size)
        centre = np.array([0, 0, focal * cam_size / H])
        assert np.allclose(local[5:10] - centre, 0.95 * (local[0:5] - centre), atol=1e-12)
        # the turned copy: 2 degrees about the optical axis once the aspect ratio's stretch of x is undone; the apex stays
        unstretch = np.array([H / W, 1.0, 1.0])
        a, b = local[1:5] * unstretch, local[11:15] * unstretch
        cos = (a[:, :2] * b[:, :2]).sum(1) / np.linalg.norm(a[:, :2], axis=1) / np.linalg.norm(b[:, :2], axis=1)
        assert np.allclose(np.degrees(np.arccos(cos)), 2.0, atol=1e-6) and np.allclose(a[:, 2], b[:, 2])
        # the grid's corners are the base's corners
        g = local[15:].reshape(grid[0] + 1, grid[1] + 1, 3)
        assert np.allclose([g[0, 0], g[0, -1], g[-1, -1], g[-1, 0]], local[1:5], atol=1e-12)
        f = viz.camera_faces(grid)
        assert f.shape == (24 + 2 * grid[0] * grid[1], 3) and f.dtype == np.int64 and f.min() == 0 and f.max() == len(v) - 1
        sl = f[:24]
        assert len({tuple(sorted(t)) for t in sl.tolist()}) == 24                         # no reversed duplicates
        assert all(len(set(t)) == 3 for t in sl.tolist()) and (sl < 15).all()
        assert viz.camera_faces(None).shape == (viz.SLIVER_FACES, 3) and viz.camera_vertices(pose, H, W, focal).shape == (15, 3)
    assert viz.image_grid(6, 8, 64) == (48, 64) and viz.image_grid(8, 6, 64) == (64, 48) and viz.image_grid(1, 1000, 8) == (1, 8)


def test_camera_defaults_follow_the_references_branches():
    from fast3r_amd import viz
    assert viz.camera_image_size((6, 8, 3), (100, 50), 7.0) == (6.0, 8.0, 7.0)            # the image decides
    assert viz.camera_image_size((6, 8, 3), None, None) == (6.0, 8.0, 6 * 1.1)
    assert viz.camera_image_size(None, (100, 50), None) == (50.0, 100.0, 50 * 1.1)        # imsize is (W, H)
    assert viz.camera_image_size(None, None, 11.0) == (11.0 / 1.1, 11.0 / 1.1, 11.0)
    assert viz.camera_image_size(None, None, None) == (1.0, 1.0, 1.1)
