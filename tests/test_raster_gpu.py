"""The triangle rasteriser on a real MI355X against the numpy restatement (tests/raster_ref.py), bit for bit on keys, picture and depth:
the arithmetic order is specified, so there are no tolerances.  Single-triangle geometry, the viewport's edges and corners, triangles that
must be skipped (bad indices among them), both index dtypes and sub-ranges, both size paths, launch geometry, contention, composition with
points, a real mesh, the scene's cameras, and the notebook's function end to end."""
import numpy as np
import pytest
import torch

import raster_cases as C
import raster_ref as RR
import render_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def camera_of(cam):
    from fast3r_amd import Camera
    return Camera(tuple(float(v) for v in cam.view), cam.sx, cam.sy, cam.cx, cam.cy, cam.znear)


def queue_total(device, faces_per_launch):
    """the number of triangles stage 1 handed to stage 2 over all launches of the last call"""
    from fast3r_amd import post_ops
    ws, _ = post_ops.raster_workspace(device, faces_per_launch)
    return int(ws[1].item())


def check(v, f, W, H, cam=C.IDENTITY, *, index_dtype=np.int64, ranges=None, index_base=0, faces_per_launch=None, what=""):
    """raster_triangles against the restatement: keys, then picture and depth through the resolve.  -> (restated keys in image order, Setup)"""
    from fast3r_amd import post_ops
    dv, df = dev(v), dev(f.astype(index_dtype))
    colors = C.colors_of(index_base + len(f))
    keys = post_ops.render_keys(W, H, dv.device)
    kw = {} if faces_per_launch is None else {"faces_per_launch": faces_per_launch}
    queued = 0
    for f0, f1 in ranges or [(0, None)]:
        post_ops.raster_triangles(dv, df, camera_of(cam).words(), keys, f0=f0, f1=f1, index_base=index_base, **kw)
        if f1 is None or f1 > f0:                                                         # an empty range launches nothing and leaves the counters
            queued += queue_total(dv.device, faces_per_launch or post_ops.RASTER_FACES_PER_LAUNCH)
    from fast3r_amd import _lib
    want, large = np.full((H, W), RR.EMPTY, dtype=np.uint64), 0
    for f0, f1 in ranges or [(0, None)]:                                                  # the same ranges into the restatement's keys
        s = RR.raster(want, v, f, cam, f0=f0, f1=f1, index_base=index_base)
        large += int((s.pixels > _lib.RASTER_SMALL_PIXELS).sum())
    got = keys.cpu().numpy().view(np.uint64)
    assert got.shape == (H, W) and np.array_equal(got, want[::-1]), (what, int((got != want[::-1]).sum()))
    assert queued == large, what                                                          # each triangle took the path its box says
    image, depth = post_ops.render_resolve(keys, dev(colors), return_depth=True)
    wi, wd = R.resolve(want, colors)
    assert image.cpu().numpy().tobytes() == wi.tobytes() and depth.cpu().numpy().tobytes() == wd.tobytes(), what
    assert dv.cpu().numpy().tobytes() == v.tobytes() and df.cpu().numpy().tobytes() == f.astype(index_dtype).tobytes(), what   # inputs unchanged
    return want[::-1], s


# ------------------------------------------------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("W,H", C.VIEWPORTS)
def test_single_triangles_edges_corners_and_outside(built_lib, W, H):
    cases = C.single_triangles(W, H)
    for name, tri in cases.items():
        v, f = C.window_mesh([tri], W, H)
        keys, s = check(v, f, W, H, what=name)
        for g in (f[:, ::-1].copy(), f[:, [1, 2, 0]].copy()):                             # the other winding, another first vertex
            if name != "a million pixels outside":                                        # there the edge functions round differently per order
                flipped, _ = check(v, g, W, H, what=name + " rewound")
                assert np.array_equal(flipped != RR.EMPTY, keys != RR.EMPTY), name
    v, f = C.window_mesh(list(cases.values()), W, H)                                      # and all of them in one mesh
    check(v, f, W, H, what="all")


@pytest.mark.parametrize("W,H", C.VIEWPORTS)
@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
def test_skipped_triangles_and_bad_indices(built_lib, W, H, index_dtype):
    """one vertex nearer than znear, collinear and repeated vertices, NaN, inf, a vertex index of -1 and of nv: nothing of them is drawn,
    nothing is read out of range (the kernel checks the three indices before it gathers), and the inputs come back unchanged"""
    v, f, drawn = C.skipped_mesh(W, H)
    keys, s = check(v, f, W, H, index_dtype=index_dtype, what="skipped")
    assert len(s.f) == drawn and set((keys[keys != RR.EMPTY] & np.uint64(0xffffffff)).tolist()) == {0}
    torch.cuda.synchronize()


@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
def test_sub_ranges_compose_to_the_whole(built_lib, index_dtype):
    W, H = 37, 23
    v, f = C.random_triangles(300, 21, W, H, size=6.0)
    check(v, f, W, H, index_dtype=index_dtype, ranges=[(200, 300), (0, 1), (1, 1), (1, 200)], index_base=11, what="ranges")


# ------------------------------------------------------------------------------------------------------------------- the two size paths
@pytest.mark.parametrize("W,H", C.VIEWPORTS)
def test_boxes_at_the_threshold(built_lib, W, H):
    from fast3r_amd import _lib
    small = _lib.RASTER_SMALL_PIXELS
    v, f, want = C.box_recipe(W, H, small)
    _, s = check(v, f, W, H, what="boxes")
    assert s.pixels.tolist() == want == [small - 1, small, small + 1]
    for k in range(3):                                                                    # each alone: 0, 0 and 1 triangles queued
        check(v, f, W, H, ranges=[(k, k + 1)], what=f"box {k}")


@pytest.mark.parametrize("W,H", C.VIEWPORTS)
@pytest.mark.parametrize("depth", [0.5, 9.0])
def test_a_triangle_over_the_whole_viewport_with_small_ones(built_lib, W, H, depth):
    """in front of the small triangles (depth 0.5) it hides them all; behind them (depth 9) it fills what they leave"""
    v, f = C.random_triangles(200, 8, W, H, size=2.0)
    big, _ = C.window_mesh([[(-5.0, -5.0, depth), (2.0 * W + 10, -5.0, depth), (-5.0, 2.0 * H + 10, depth)]], W, H)
    for at in (0, 100, 200):                                                              # first, in the middle, last
        vv = np.concatenate([v[:3 * at], big, v[3 * at:]])
        ff = np.arange(len(vv), dtype=np.int64).reshape(-1, 3)
        keys, _ = check(vv, ff, W, H, what=f"big at {at}")
        assert (keys != RR.EMPTY).all()
        shows = ((keys & np.uint64(0xffffffff)) == np.uint64(at))
        assert shows.all() if depth < 1 else 0 < shows.sum() < W * H


# ------------------------------------------------------------------------------------------------------------------- launch geometry
@pytest.mark.parametrize("n", [255, 256, 257])
def test_face_counts_around_a_workgroup(built_lib, n):
    v, f = C.random_triangles(n, n, 37, 23, size=5.0)
    check(v, f, 37, 23, what=f"{n} faces")


@pytest.mark.parametrize("n,faces_per_launch", [(257, 100), (5, 1), (257, 256)])
def test_chunked_launches_and_the_queue_reset(built_lib, n, faces_per_launch):
    v, f = C.random_triangles(n, 40 + n, 64, 48, size=9.0)
    _, s = check(v, f, 64, 48, faces_per_launch=faces_per_launch, what=f"{n} faces by {faces_per_launch}")
    assert (s.pixels > 64).sum() >= 2 and (s.pixels <= 64).any()                          # both paths ran in the chunks


# ------------------------------------------------------------------------------------------------------------------- contention
def test_contention_is_deterministic(built_lib):
    """4 096 random triangles on 16 x 16: every pixel is fought over; two runs give the same bits, and they are the restatement's"""
    from fast3r_amd import post_ops
    W = H = 16
    v, f = C.random_triangles(4096, 2, W, H, size=10.0)
    want, s = check(v, f, W, H, what="contention")
    assert (want != RR.EMPTY).all() and (s.pixels > 64).sum() > 1000
    dv, df = dev(v), dev(f)
    runs = []
    for _ in range(2):
        keys = post_ops.render_keys(W, H, dv.device)
        post_ops.raster_triangles(dv, df, camera_of(C.IDENTITY).words(), keys)
        runs.append(keys.cpu().numpy().view(np.uint64))
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], want)


# ------------------------------------------------------------------------------------------------------------------- with points
def mesh_dict(v, f, colors, index_dtype=np.int64):
    return dict(vertices=dev(v), faces=dev(f.astype(index_dtype)), face_colors=dev(colors))


def check_render_mesh(v, f, fc, cam, W, H, p=None, pc=None, size=3.0, index_dtype=np.int64):
    import fast3r_amd
    from fast3r_amd import post_ops
    mesh = mesh_dict(v, f, fc, index_dtype)
    kw = {} if p is None else dict(points=dev(p), colors=dev(pc))
    image, depth = fast3r_amd.render_mesh(mesh, camera_of(cam), width=W, height=H, point_size=size, return_depth=True, **kw)
    wi, wd, wk = RR.render(v, f, fc, cam, W, H, p, pc, size)
    assert image.dtype == torch.uint8 and tuple(image.shape) == (H, W, 3) and depth.dtype == torch.float32
    assert image.cpu().numpy().tobytes() == wi.tobytes() and depth.cpu().numpy().tobytes() == wd.tobytes()
    # the same by hand: splat, raster, resolve
    keys = post_ops.render_keys(W, H, mesh["vertices"].device)
    n = 0 if p is None else len(p)
    if n:
        post_ops.render_splat(kw["points"], 0, n, camera_of(cam).words(), size, keys)
    post_ops.raster_triangles(mesh["vertices"], mesh["faces"], camera_of(cam).words(), keys, index_base=n)
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), wk)
    table = mesh["face_colors"] if n == 0 else torch.cat((kw["colors"], mesh["face_colors"]))
    assert torch.equal(post_ops.render_resolve(keys, table), image)
    return wi, wd


def test_points_and_faces_in_one_picture(built_lib):
    W, H = 64, 48
    face = lambda d, x=20.0: [(x, 10.0, d), (x + 20, 12.0, d), (x + 8, 34.0, d)]   # noqa: E731
    v, f = C.window_mesh([face(2.0), face(2.0, 24.0), face(4.0, 30.0)], W, H)             # two overlapping faces at depth 2, one behind
    fc = np.array([[10, 0, 0], [20, 0, 0], [30, 0, 0]], np.uint8)
    at = lambda xw, yw, d: ((2 * xw / W - 1) * d, (2 * yw / H - 1) * d, -d)   # noqa: E731
    p = np.array([at(28.5, 16.5, 1.0), at(33.5, 16.5, 3.0), at(30.5, 22.5, 2.0), at(60.5, 40.5, 2.0)], F32)
    pc = np.array([[0, 1, 0], [0, 2, 0], [0, 3, 0], [0, 4, 0]], np.uint8)
    image, depth = check_render_mesh(v, f, fc, C.IDENTITY, W, H, p, pc, size=1.0)
    row = lambda yw: H - 1 - int(yw)   # noqa: E731
    assert image[row(16.5), 28].tolist() == [0, 1, 0] and depth[row(16.5), 28] == 1.0     # a point in front of a face
    assert image[row(16.5), 33].tolist() == [10, 0, 0] and depth[row(16.5), 33] == 2.0    # a point behind a face: the lower of the two faces
    assert image[row(22.5), 30].tolist() == [0, 3, 0] and depth[row(22.5), 30] == 2.0     # equal fp32 depth: the point shows
    assert image[row(20.5), 30].tolist() == [10, 0, 0]                                    # two faces at equal depth: the lower index
    assert image[row(40.5), 60].tolist() == [0, 4, 0]
    only, _ = check_render_mesh(v, f, fc, C.IDENTITY, W, H)                               # without points
    assert only[row(22.5), 30].tolist() == [10, 0, 0]
    check_render_mesh(v, f[::-1].copy(), fc, C.IDENTITY, W, H, p, pc, size=4.0, index_dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------- a real mesh
def on_device(preds, views):
    return [{k: dev(v) for k, v in p.items()} for p in preds], [{k: dev(v) for k, v in vw.items()} for vw in views]


def test_build_mesh_through_a_pinhole(built_lib):
    """three synthetic 32 x 48 views with a depth step (rubber-sheet triangles over it), about 17 k faces, double-sided, at 160 x 120"""
    import fast3r_amd
    preds, views = C.synthetic_views()
    mesh = fast3r_amd.build_mesh(*on_device(preds, views), min_conf_thr_percentile=5)
    v, f, fc = (t.cpu().numpy() for t in (mesh.vertices, mesh.faces, mesh.face_colors))
    assert 12000 < len(f) < 18000
    W, H = 160, 120
    cam = fast3r_amd.pinhole_camera(np.eye(4), 150.0, (W / 2 - 0.5, H / 2 - 0.5), H, W)
    image, depth = fast3r_amd.render_mesh(mesh, cam, width=W, height=H, return_depth=True)
    wi, wd, _ = RR.render(v, f, fc, cam, W, H)
    assert image.cpu().numpy().tobytes() == wi.tobytes() and depth.cpu().numpy().tobytes() == wd.tobytes()
    assert 0.3 < np.isfinite(wd).mean() < 1.0
    single = fast3r_amd.build_mesh(*on_device(preds, views), min_conf_thr_percentile=5, double_sided=False, index_dtype=torch.int32)
    assert 2 * len(single.faces) == len(f)
    again, d2 = fast3r_amd.render_mesh(single, cam, width=W, height=H, return_depth=True)  # nothing is culled: the same surface
    assert torch.equal(d2, depth)
    # and with the cloud of the same views in the picture, through the camera the function derives
    p, pc = fast3r_amd.combine_points(*on_device(preds, views), pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                      min_conf_thr_percentile=50)
    got = fast3r_amd.render_mesh(mesh.as_dict(), points=p, colors=pc, width=96, height=54, point_size=2.0)
    from fast3r_amd import render
    want, _, _ = RR.render(v, f, fc, render.cloud_camera(p), 96, 54, p.cpu().numpy(), pc.cpu().numpy(), 2.0)
    assert got.cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------------- cameras
def test_camera_meshes_through_a_fourth_camera(built_lib):
    import fast3r_amd
    from fast3r_amd import viz
    rs = np.random.RandomState(9)
    poses = []
    for k in range(3):
        pose = np.eye(4)
        t = 0.4 * (k - 1)
        pose[:3, :3] = np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])
        pose[:3, 3] = [0.5 * (k - 1), 0.1 * k, 0.0]
        poses.append(pose)
    images = [rs.randint(0, 255, (6, 8, 3)).astype(np.uint8), rs.uniform(0, 1, (6, 8, 3)).astype(F32), rs.uniform(-1, 1, (3, 6, 8)).astype(F32)]
    mesh = fast3r_amd.camera_meshes(poses, [9.0, None, 7.5], images=images, cam_size=0.3, image_cells=8)
    v, f, fc = (t.cpu().numpy() for t in (mesh["vertices"], mesh["faces"], mesh["face_colors"]))
    per = 24 + 2 * 8 * 6
    assert f.shape == (3 * per, 3) and fc.shape == f.shape and v.shape == (3 * (15 + 9 * 7), 3) and v.dtype == F32
    for k in range(3):                                                                    # the host geometry, rounded once; the edge colours
        assert np.array_equal(v[k * 78:(k + 1) * 78], viz.camera_vertices(poses[k], 6, 8, [9.0, 6 * 1.1, 7.5][k], 0.3, (6, 8)).astype(F32))
        assert np.array_equal(f[k * per:(k + 1) * per], viz.camera_faces((6, 8)) + k * 78)
        assert (fc[k * per:k * per + 24] == fast3r_amd.CAM_COLORS[k]).all()
    u8 = [images[0], (images[1] * F32(255.0)).astype(np.uint8), R.color_u8(np.transpose(images[2], (1, 2, 0)))]
    for k in range(3):                                                                    # an 8 x 6 grid on an 8 x 6 image: cell = pixel
        assert np.array_equal(fc[k * per + 24:(k + 1) * per].reshape(6, 8, 2, 3), np.repeat(u8[k][:, :, None], 2, axis=2)), k
    W, H = 64, 48
    viewer = C.look_from(poses[1], 1.5)
    viewer[:3, 3] += [0.05, -0.2, 0.0]
    cam = fast3r_amd.pinhole_camera(viewer, 50.0, (W / 2 - 0.5, H / 2 - 0.5), H, W)
    image, depth = fast3r_amd.render_mesh(mesh, cam, width=W, height=H, return_depth=True)
    wi, wd, _ = RR.render(v, f, fc, cam, W, H)
    assert image.cpu().numpy().tobytes() == wi.tobytes() and depth.cpu().numpy().tobytes() == wd.tobytes()
    seen = {tuple(c) for c in wi.reshape(-1, 3).tolist()}
    assert all(fast3r_amd.CAM_COLORS[k] in seen for k in range(3)) and len(seen) > 20     # the three pyramids' edges and their images
    # the same through SceneViz, with a cloud
    p = rs.uniform(-1, 1, (500, 3)).astype(F32) * [1.0, 0.5, 0.3] + [0, 0, 1.0]
    scene = fast3r_amd.SceneViz().add_pointcloud([p[:200], p[200:]], (0, 128, 255)).add_cameras(poses, [9.0, None, 7.5], images=images, cam_size=0.3)
    got = scene.render(cam, width=W, height=H, point_size=2, image_cells=8)
    want, _, _ = RR.render(v, f, fc, cam, W, H, p.astype(F32), np.tile(np.array([[0, 128, 255]], np.uint8), (500, 1)), 2.0)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(NotImplementedError, match="render"):
        scene.show()


def scene_camera_case():
    import fast3r_amd
    rs = np.random.RandomState(13)
    pose = np.eye(4)
    pose[:3, 3] = [0.1, -0.1, 0.0]
    image = rs.randint(0, 255, (6, 8, 3)).astype(np.uint8)
    W, H = 64, 48
    viewer = C.look_from(pose, 1.2)
    cam = fast3r_amd.pinhole_camera(viewer, 50.0, (W / 2 - 0.5, H / 2 - 0.5), H, W)
    return rs, pose, image, cam, W, H


@pytest.mark.parametrize("kind", ["uint8", "float"])
def test_scene_pointcloud_with_per_view_colours_and_masks(built_lib, kind):
    """per-view device tensors of different H x W, colours as a list like the points (uint8, or float in [0, 1] as the reference's
    uint8()), boolean masks selecting on the device: the picture is the restatement's of the masked, concatenated cloud and the camera"""
    import fast3r_amd
    rs, pose, image, cam, W, H = scene_camera_case()
    shapes = [(5, 7), (9, 4), (1, 1), (6, 6)]
    pts = [(rs.uniform(-1, 1, s + (3,)) * [0.8, 0.5, 0.3] + [0, 0, 1.0]).astype(F32) for s in shapes]
    masks = [rs.rand(*s) < 0.7 for s in shapes]
    masks[2][:] = False                                                                   # a view that keeps nothing
    if kind == "uint8":
        cols = [rs.randint(0, 255, s + (3,)).astype(np.uint8) for s in shapes]
        want_cols = cols
    else:
        cols = [rs.uniform(0, 1, s + (3,)).astype(F32) for s in shapes]
        want_cols = [(c * F32(255.0)).astype(np.uint8) for c in cols]
    mesh = fast3r_amd.camera_meshes([pose], [9.0], images=[image], cam_size=0.3, image_cells=8)
    v, f, fc = (t.cpu().numpy() for t in (mesh["vertices"], mesh["faces"], mesh["face_colors"]))
    p = np.concatenate([a[m] for a, m in zip(pts, masks)])
    pc = np.concatenate([a[m] for a, m in zip(want_cols, masks)])
    want, _, _ = RR.render(v, f, fc, cam, W, H, p, pc, 2.0)
    for lift in (dev, lambda a: a, lambda a: torch.from_numpy(a)):                        # device tensors, host arrays, host tensors
        scene = fast3r_amd.SceneViz().add_pointcloud([lift(a) for a in pts], [lift(c) for c in cols], mask=[lift(m) for m in masks])
        scene.add_camera(pose, 9.0, color=fast3r_amd.CAM_COLORS[0], image=image, cam_size=0.3)
        got = scene.render(cam, width=W, height=H, point_size=2, image_cells=8)
        assert got.cpu().numpy().tobytes() == want.tobytes()
    # without masks, and one view given as it is instead of a list
    scene = fast3r_amd.SceneViz().add_pointcloud(dev(pts[0]), dev(cols[0])).add_pointcloud([dev(pts[1])], [dev(cols[1])])
    scene.add_camera(pose, 9.0, color=fast3r_amd.CAM_COLORS[0], image=image, cam_size=0.3)
    got = scene.render(cam, width=W, height=H, point_size=2, image_cells=8)
    want, _, _ = RR.render(v, f, fc, cam, W, H, np.concatenate([pts[0].reshape(-1, 3), pts[1].reshape(-1, 3)]),
                           np.concatenate([want_cols[0].reshape(-1, 3), want_cols[1].reshape(-1, 3)]), 2.0)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="views"):
        fast3r_amd.SceneViz().add_pointcloud([dev(pts[0]), dev(pts[1])], [dev(cols[0])])


def test_scene_pointcloud_colour_triples(built_lib):
    """one (r, g, b) for all points, whatever holds it: a tuple, a list, a numpy array, a host or device tensor, floats in [0, 1]"""
    import fast3r_amd
    rs, pose, image, cam, W, H = scene_camera_case()
    pts = [(rs.uniform(-1, 1, (4, 5, 3)) * [0.8, 0.5, 0.3] + [0, 0, 1.0]).astype(F32), (rs.uniform(-1, 1, (3, 3)) * 0.5 + [0, 0, 1.0]).astype(F32)]
    p = np.concatenate([a.reshape(-1, 3) for a in pts])
    mesh = fast3r_amd.camera_meshes([pose], [9.0], images=[image], cam_size=0.3, image_cells=8)
    v, f, fc = (t.cpu().numpy() for t in (mesh["vertices"], mesh["faces"], mesh["face_colors"]))
    want, _, _ = RR.render(v, f, fc, cam, W, H, p, np.tile(np.array([[0, 128, 255]], np.uint8), (len(p), 1)), 2.0)
    triple = np.array([0, 128, 255], np.uint8)
    forms = [(0, 128, 255), [0, 128, 255], triple, torch.from_numpy(triple), dev(triple), dev(triple.astype(np.int64)),
             (np.uint8(0), np.int64(128), 255)]
    for color in forms:
        scene = fast3r_amd.SceneViz().add_pointcloud([dev(a) for a in pts], color)
        scene.add_camera(pose, 9.0, color=fast3r_amd.CAM_COLORS[0], image=image, cam_size=0.3)
        got = scene.render(cam, width=W, height=H, point_size=2, image_cells=8)
        assert got.cpu().numpy().tobytes() == want.tobytes(), type(color)
    # floats are 255 * c, as the reference's uint8(): (0, 0.5, 1) -> (0, 127, 255)
    want, _, _ = RR.render(v, f, fc, cam, W, H, p, np.tile(np.array([[0, 127, 255]], np.uint8), (len(p), 1)), 2.0)
    for color in ((0.0, 0.5, 1.0), dev(np.array([0.0, 0.5, 1.0], F32))):
        scene = fast3r_amd.SceneViz().add_pointcloud([dev(a) for a in pts], color)
        scene.add_camera(pose, 9.0, color=fast3r_amd.CAM_COLORS[0], image=image, cam_size=0.3)
        assert scene.render(cam, width=W, height=H, point_size=2, image_cells=8).cpu().numpy().tobytes() == want.tobytes()
    # a single view of three points given as it is, with colours of its own shape (3, 3): per point, not a triple
    one, its = pts[1], np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.uint8)
    got = fast3r_amd.SceneViz().add_pointcloud(dev(one), dev(its)).render(cam, width=W, height=H, point_size=2)
    assert got.cpu().numpy().tobytes() == R.render(one, its, cam, W, H, 2.0)[0].tobytes()
    # a (3,) colour beside a (3,)-shaped single point: either reading is the same cloud
    got = fast3r_amd.SceneViz().add_pointcloud(dev(one[0]), dev(its[0])).render(cam, width=W, height=H, point_size=2)
    assert got.cpu().numpy().tobytes() == R.render(one[:1], its[:1], cam, W, H, 2.0)[0].tobytes()


def test_render_mesh_of_an_empty_mesh_with_points_and_on_a_side_stream(built_lib):
    import fast3r_amd
    from fast3r_amd import post_ops
    W, H = 37, 23
    p = np.array([[0.0, 0.0, -1.0], [0.3, 0.2, -2.0]], F32)
    pc = np.array([[1, 2, 3], [4, 5, 6]], np.uint8)
    for nv in (0, 3):                                                                     # no faces, with and without vertices: the points alone
        empty = dict(vertices=torch.zeros((nv, 3), device="cuda"), faces=torch.zeros((0, 3), dtype=torch.int64, device="cuda"),
                     face_colors=torch.zeros((0, 3), dtype=torch.uint8, device="cuda"))
        got = fast3r_amd.render_mesh(empty, camera_of(C.IDENTITY), points=dev(p), colors=dev(pc), point_size=3.0, width=W, height=H)
        assert got.cpu().numpy().tobytes() == R.render(p, pc, C.IDENTITY, W, H, 3.0)[0].tobytes()
    with pytest.raises(ValueError, match="nothing to draw"):
        fast3r_amd.render_mesh(empty, camera_of(C.IDENTITY), width=W, height=H)
    # a side stream gets a workspace of its own and the same bits
    v, f = C.random_triangles(300, 77, W, H, size=6.0)
    want = np.full((H, W), RR.EMPTY, dtype=np.uint64)
    RR.raster(want, v, f, C.IDENTITY)
    dv, df = dev(v), dev(f)
    main_ws, _ = post_ops.raster_workspace(dv.device, post_ops.RASTER_FACES_PER_LAUNCH)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        keys = post_ops.render_keys(W, H, dv.device)
        post_ops.raster_triangles(dv, df, camera_of(C.IDENTITY).words(), keys)
        side_ws, _ = post_ops.raster_workspace(dv.device, post_ops.RASTER_FACES_PER_LAUNCH)
    side.synchronize()
    assert side_ws.data_ptr() != main_ws.data_ptr()
    assert np.array_equal(keys.cpu().numpy().view(np.uint64), want[::-1])


@pytest.fixture(scope="module")
def tiny_output():
    from fast3r_amd import Fast3R, MultiViewDUSt3RLitModule, inference
    from fast3r_amd.synthetic import make_views, synth_state_dict, tiny_args
    enc, dec, head = tiny_args()
    m = Fast3R(enc, dec, head).eval()
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0), strict=True)
    lit = MultiViewDUSt3RLitModule.load_for_inference(m.cuda())
    torch.manual_seed(3)
    return inference(make_views(3, 64, 64, batch=2), lit, torch.device("cuda"), dtype=torch.float16, verbose=False)


def test_plot_3d_points_with_estimated_camera_poses_end_to_end(built_lib, tiny_output, tmp_path):
    """what inference() returns goes in as it is; the PNG holds the returned picture, which is the restatement's picture of the same
    cloud and cameras; seen from just behind the first estimated camera, its pyramid's edges show in its colour"""
    import fast3r_amd
    from PIL import Image
    out = tiny_output
    W, H, pct = 192, 108, 80
    png, ply = tmp_path / "scene.png", tmp_path / "scene.ply"
    picture = fast3r_amd.plot_3d_points_with_estimated_camera_poses(out["preds"], out["views"], min_conf_thr_percentile=pct,
                                                                    export_ply_path=str(ply), output_path=str(png), width=W, height=H)
    host = picture.cpu().numpy()
    assert host.shape == (H, W, 3) and host.dtype == np.uint8
    assert np.array_equal(np.asarray(Image.open(png).convert("RGB")), host) and ply.stat().st_size > 1000
    # the same scene restated: the cloud, the poses, the cameras' mesh
    p, pc = fast3r_amd.combine_points(out, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf", min_conf_thr_percentile=pct)
    preds = [{k: q[k].cuda() for k in ("pts3d_in_other_view", "conf")} for q in out["preds"]]
    poses, focals = fast3r_amd.estimate_camera_poses(preds, niter_PnP=10)
    size = max(fast3r_amd.auto_cam_size(poses[0]), 0.05)
    mesh = fast3r_amd.camera_meshes(poses[0], focals[0], images=[v["img"][0] for v in out["views"]], cam_size=size)
    v, f, fc = (t.cpu().numpy() for t in (mesh["vertices"], mesh["faces"], mesh["face_colors"]))
    from fast3r_amd import render
    want, _, keys = RR.render(v, f, fc, render.cloud_camera(p), W, H, p.cpu().numpy(), pc.cpu().numpy(), 1.0)
    assert host.tobytes() == want.tobytes()
    # at least one pixel of the written picture carries a camera colour: a pixel whose key names a sliver face shows that camera's colour
    index = (keys & np.uint64(0xffffffff)).astype(np.int64) - len(p)
    per_camera = len(f) // 3
    sliver = (keys != RR.EMPTY) & (index >= 0) & (index % per_camera < 24)
    assert sliver.any()
    for r, c in np.argwhere(sliver):
        assert tuple(host[r, c]) == fast3r_amd.CAM_COLORS[index[r, c] // per_camera]
    # from 4 camera sizes behind camera 0, looking its way: its pyramid is straight ahead and nearer than anything it looks at
    viewer = fast3r_amd.pinhole_camera(C.look_from(poses[0][0], 4 * size), 100.0, (W / 2 - 0.5, H / 2 - 0.5), H, W)
    close = fast3r_amd.plot_3d_points_with_estimated_camera_poses(out, None, min_conf_thr_percentile=pct, camera=viewer, width=W, height=H)
    want, _, _ = RR.render(v, f, fc, viewer, W, H, p.cpu().numpy(), pc.cpu().numpy(), 1.0)
    assert close.cpu().numpy().tobytes() == want.tobytes()
    assert (close.cpu().numpy() == np.array(fast3r_amd.CAM_COLORS[0], np.uint8)).all(-1).sum() >= 1
    flipped = fast3r_amd.plot_3d_points_with_estimated_camera_poses(out, None, flip_axes=True, min_conf_thr_percentile=pct, width=W, height=H)
    assert tuple(flipped.shape) == (H, W, 3) and not torch.equal(flipped, picture)
    with pytest.raises(ValueError, match="HTML"):
        fast3r_amd.plot_3d_points_with_estimated_camera_poses(out, None, export_html_path=str(tmp_path / "scene.html"))
