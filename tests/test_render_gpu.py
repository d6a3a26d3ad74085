"""The point-splat renderer on a real MI355X against the numpy restatement (tests/render_ref.py), byte for byte: the arithmetic order is
specified, so there are no tolerances except the centre's (two fp64 sums of the same values in different orders).  Clipped squares at
the viewport's edges and corners, culling at every frustum plane, point sizes and viewports, ties, the cumulative frames, contention on
a 4 x 4 viewport, the whole function on a tiny model, a pinhole round trip, the centre and the depth output."""
import os

import numpy as np
import pytest
import torch

import render_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
NEXT_UP = float(np.nextafter(F32(1), F32(2)))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def identity_camera(**kw):
    from fast3r_amd import Camera
    return Camera((1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0), kw.pop("sx", 1.0), kw.pop("sy", 1.0), **kw)


def colors_of(n, seed=0):
    """distinct colours, none of them the background's"""
    c = np.stack([np.arange(n) % 251, (np.arange(n) // 251) % 251, (np.arange(n) * 7 + seed) % 251], axis=1).astype(np.uint8)
    return c


def check(points, colors, camera, W, H, size, segments=None, background=(255, 255, 255)):
    """the product's pictures and depths against the restatement's: dtype, shape and bytes.  -> the restatement's (image, depth), or their list with segments"""
    import fast3r_amd
    dp, dc = dev(points), dev(colors)
    got = fast3r_amd.render_points(dp, dc, camera, width=W, height=H, point_size=size, segments=segments, return_depth=True,
                                   background=background)
    want = R.render(points, colors, camera, W, H, size, background, segments)
    got, want = ([got], [want]) if segments is None else (list(got), want)
    assert len(got) == len(want)
    for i, ((gi, gd), (wi, wd)) in enumerate(zip(got, want)):
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        assert gi.dtype == np.uint8 and gi.shape == (H, W, 3) and gd.dtype == F32 and gd.shape == (H, W)
        assert gi.tobytes() == wi.tobytes(), (i, int((gi != wi).any(-1).sum()))
        assert gd.tobytes() == wd.tobytes(), i                                            # bit for bit, +inf where the pixel is empty
    assert dp.cpu().numpy().tobytes() == points.tobytes() and dc.cpu().numpy().tobytes() == colors.tobytes()   # inputs are not written
    return want[0] if segments is None else want


def random_cloud(n, seed, spread=1.3):
    """points around the frustum of an identity camera with sx = sy = 1: most inside, some beyond every side, some behind"""
    rs = np.random.RandomState(seed)
    d = rs.uniform(0.2, 4.0, n)
    p = np.stack([rs.uniform(-spread, spread, n) * d, rs.uniform(-spread, spread, n) * d, -d], axis=1).astype(F32)
    p[rs.rand(n) < 0.05, 2] *= -1
    return p


# ------------------------------------------------------------------------------------------------------------------- edges and culling
EDGE_POINTS = [(-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1)]      # the four edges, the four corners


@pytest.mark.parametrize("size", [1, 4, 5, 2.5, 33])
def test_squares_clipped_at_edges_and_corners_and_centres_outside(built_lib, size):
    """64 x 36.  Points exactly on the frustum's sides are drawn and their squares clipped to the viewport; a centre one ulp outside any
    side is dropped, although its square would reach in."""
    W, H = 64, 36
    on = np.array([(x * 2.0, y * 2.0, -2.0) for x, y in EDGE_POINTS], F32)
    out = np.array([(x * NEXT_UP * 2.0, y * 2.0, -2.0) for x, y in EDGE_POINTS if x] +
                   [(x * 2.0, y * NEXT_UP * 2.0, -2.0) for x, y in EDGE_POINTS if y], F32)
    p = np.concatenate([on, out, np.array([[0.1, 0.2, -3.0]], F32)])
    c = colors_of(len(p))
    image, depth = check(p, c, identity_camera(), W, H, size)
    seen = {tuple(v) for v in image.reshape(-1, 3).tolist()}
    assert not any(tuple(v) in seen for v in c[len(on):len(on) + len(out)].tolist())      # no centre outside left a pixel
    if size >= 2.5:
        assert all(tuple(v) in seen for v in c[:len(on)].tolist())                        # every edge and corner point shows, clipped
        assert tuple(image[H - 1, 0]) == tuple(c[4]) and tuple(image[0, W - 1]) == tuple(c[7])   # (-1, -1): bottom left; (1, 1): top right
    else:   # s = 1: [x_w - 0.5, x_w + 0.5) holds the centre W - 0.5 at x_w = W but no centre at x_w = 0 -- half-open
        assert tuple(c[1]) in seen and tuple(c[0]) not in seen


def test_depth_culling_and_non_finite_points(built_lib):
    W, H = 7, 5
    near = F32(0.05)                                                                      # fp64(fp32(0.05)) = 0.05000000074... >= 0.05
    rows = [(0, 0, -near), (0.01, 0, -np.nextafter(near, F32(0))), (0, 0, 1.0), (0, 0, 0.0), (0, 0, -0.0),
            (np.nan, 0, -1), (0, np.nan, -1), (0, 0, np.nan), (np.inf, 0, -1), (0, -np.inf, -1), (0, 0, -np.inf), (0, 0, np.inf),
            (np.inf, np.inf, -np.inf), (0.5, 0.5, -1.0)]
    p = np.array(rows, F32)
    c = colors_of(len(p))
    image, depth = check(p, c, identity_camera(), W, H, 1)
    seen = {tuple(v) for v in image.reshape(-1, 3).tolist()}
    assert seen == {tuple(c[0]), tuple(c[-1]), (255, 255, 255)} and depth[2, 3] == near   # d = znear is drawn; everything else here is not
    # d beyond the fp32 range: finite in fp64, +inf as a float -- not drawn; one ulp lower it is
    from fast3r_amd import Camera
    far = Camera((1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 2.0, 0.0), 1.0, 1.0)
    big = float(np.finfo(F32).max)
    p = np.array([(0, 0, -big), (0, 0, -big / 2), (0, 0, -np.nextafter(F32(big / 2), F32(0)))], F32)
    image, depth = check(p, colors_of(3), far, W, H, 1)
    assert tuple(image[2, 3]) == tuple(colors_of(3)[2]) and depth[2, 3] == np.nextafter(F32(big / 2), F32(0)) * F32(2)


# ------------------------------------------------------------------------------------------------------------------- sizes and viewports
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (64, 36)])
@pytest.mark.parametrize("size", [1, 4, 5, 2.5, 33])
def test_sizes_and_viewports(built_lib, W, H, size):
    p = random_cloud(3000, seed=W * 100 + int(size * 10))
    image, _ = check(p, colors_of(len(p)), identity_camera(sx=0.9, sy=1.1, cx=0.05, cy=-0.1), W, H, size, background=(0, 10, 200))
    assert (image != np.array([0, 10, 200], np.uint8)).any()


def test_full_hd_once(built_lib):
    """1920 x 1080, about 10^5 points in several workgroups, through the cloud's own bird's-eye camera"""
    from fast3r_amd import render
    rs = np.random.RandomState(5)
    p = (rs.randn(100003, 3) * [2.0, 1.0, 0.5] + [0.3, 0.02, 1.0]).astype(F32)
    cam = render.cloud_camera(dev(p))
    image, _ = check(p, colors_of(len(p)), cam, 1920, 1080, 5.0)
    assert 0.02 < (image != 255).any(-1).mean() < 0.9


# ------------------------------------------------------------------------------------------------------------------- ties
def test_ties_go_to_the_lowest_index(built_lib):
    W, H = 7, 5
    spot = (0.0, 0.0, -1.0)
    p = np.array([(0.5, 0.5, -3.0), spot, spot, spot, (0.3, 0, -1.0), (-0.3, 0, -1.0), spot], F32)   # equal depth at three x as well
    c = colors_of(len(p))
    (image, depth), = check(p, c, identity_camera(), W, H, 1, segments=[len(p)])
    assert tuple(image[2, 3]) == tuple(c[1]) and depth[2, 3] == 1.0
    frames = check(p, c, identity_camera(), W, H, 4, segments=[1, 2, 3, 3, 5, 7])        # across segments: the earlier segment's point stays
    assert all(tuple(f[0][2, 3]) == tuple(c[1]) for f in frames[1:])
    q = p[::-1].copy()                                                                    # the same cloud reversed: now the last copy is index 0
    (image, _), = check(q, c, identity_camera(), W, H, 1, segments=[len(q)])
    assert tuple(image[2, 3]) == tuple(c[0])


# ------------------------------------------------------------------------------------------------------------------- cumulative frames
VIEW_SHAPES = [(1, 1), (8, 12), (17, 3), (5, 7), (40, 30)]
CONSTANT_VIEW = 3


def cumulative_case(empty=False):
    """five views, B = 2; view 3 has constant confidence and the 1 x 1 view is its own minimum: both keep nothing at any percentile.  View 1
    holds a far red point and view 4 a nearer green one straight above it."""
    rs = np.random.RandomState(11)
    preds, views = [], []
    for v, (H, W) in enumerate(VIEW_SHAPES):
        pts = np.stack([rs.uniform(-1, 1, (2, H, W)), rs.uniform(-0.5, 0.5, (2, H, W)), rs.uniform(0, 0.5, (2, H, W))], axis=-1).astype(F32)
        conf = rs.uniform(1, 10, (2, H, W)).astype(F32)
        img = rs.uniform(-0.9, 0.9, (2, 3, H, W)).astype(F32)
        if v == 1:                                                                        # above every random point (z <= 0.5)
            pts[:, 2, 5], conf[:, 2, 5], img[:, :, 2, 5] = (0.31, 0.12, 0.6), 100.0, (1.0, -1.0, -1.0)
        if v == 4:
            pts[:, 7, 9], conf[:, 7, 9], img[:, :, 7, 9] = (0.31, 0.12, 0.9), 100.0, (-1.0, 1.0, -1.0)
        if v == CONSTANT_VIEW or empty:
            conf[:] = 3.0
        preds.append({"pts3d_in_other_view": pts, "conf": conf})
        views.append({"img": img})
    return preds, views


def on_device(preds, views):
    return [{k: dev(v) for k, v in p.items()} for p in preds], [{k: dev(v) for k, v in vw.items()} for vw in views]


def test_cumulative_frames(built_lib, tmp_path):
    import fast3r_amd
    from fast3r_amd import post_ops, render
    preds, views = cumulative_case()
    dp, dv = on_device(preds, views)
    W, H, size, pct = 64, 36, 3.0, 20
    p, c, ends = R.combine(preds, views, pct)
    gp, gc, gends = fast3r_amd.combine_points(dp, dv, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                              min_conf_thr_percentile=pct, return_offsets=True)
    assert gends == ends and ends[0] == 0 and ends[CONSTANT_VIEW] == ends[CONSTANT_VIEW - 1] and gp.cpu().numpy().tobytes() == p.tobytes()
    lo, hi, bad = post_ops.cloud_bounds(gp)
    cam = render.cloud_camera(gp)                                                         # the camera the function derives by itself
    assert bad == 0 and cam == fast3r_amd.birdseye_camera(post_ops.render_center(gp), lo, hi)
    assert np.array_equal(np.array(lo, F32), p.min(0)) and (np.abs(np.array(post_ops.render_center(gp)) - R.center(p)) <= R.center_bound(p)).all()
    want = R.render(p, c, cam, W, H, size, segments=ends)
    frames = fast3r_amd.render_cumulative_pts3d_viz(dp, dv, str(tmp_path), size, pct, width=W, height=H, return_frames=True)
    assert len(frames) == 5 and sorted(os.listdir(tmp_path)) == [f"cumulative_{i:03d}.png" for i in range(5)]
    for i, (f, (wi, _)) in enumerate(zip(frames, want)):
        assert f.is_cuda and f.dtype == torch.uint8 and f.cpu().numpy().tobytes() == wi.tobytes(), i
    assert (want[0][0] == 255).all()                                                      # the 1 x 1 view keeps nothing: a blank first picture
    assert torch.equal(frames[CONSTANT_VIEW], frames[CONSTANT_VIEW - 1]) and not torch.equal(frames[2], frames[1])
    # the green point of view 4 is nearer than the red one of view 1 below it: red until frame 3, green from frame 4
    _, xw, yw, _ = R.project(np.array([[0.31, 0.12, 0.9]], F32), cam, W, H)
    row, col = H - 1 - int(np.floor(yw[0])), int(np.floor(xw[0]))
    shown = [tuple(f[row, col].tolist()) for f in frames]
    assert shown[0] == (255, 255, 255) and shown[1:4] == [(255, 0, 0)] * 3 and shown[4] == (0, 255, 0)
    # every frame equals a from-scratch picture of the segments up to it
    for i, end in enumerate(ends):
        if end:
            scratch = fast3r_amd.render_points(gp[:end], gc[:end], cam, width=W, height=H, point_size=size)
            assert torch.equal(scratch, frames[i]), i
    # the generator form on the same cloud, and a subset of frames
    again = list(fast3r_amd.render_points(gp, gc, cam, width=W, height=H, point_size=size, segments=ends))
    assert all(torch.equal(a, b) for a, b in zip(again, frames))
    sub = tmp_path / "sub"
    some = fast3r_amd.render_cumulative_pts3d_viz(dp, dv, str(sub), size, pct, width=W, height=H, frames=[4, 1], return_frames=True)
    assert sorted(os.listdir(sub)) == ["cumulative_001.png", "cumulative_004.png"] and len(some) == 2
    assert torch.equal(some[0], frames[1]) and torch.equal(some[1], frames[4])
    with pytest.raises(ValueError, match="frames"):
        fast3r_amd.render_cumulative_pts3d_viz(dp, dv, str(sub), frames=[5])
    with pytest.raises(ValueError, match="segments"):
        fast3r_amd.render_points(gp, gc, cam, segments=[3, 2])


def test_nothing_kept_means_no_files_and_no_frames(built_lib, tmp_path):
    import fast3r_amd
    dp, dv = on_device(*cumulative_case(empty=True))
    out = tmp_path / "none"
    assert fast3r_amd.render_cumulative_pts3d_viz(dp, dv, str(out), width=16, height=9, return_frames=True) == []
    assert fast3r_amd.render_cumulative_pts3d_viz(dp, dv, str(out), width=16, height=9) is None
    assert os.listdir(out) == []


def test_a_cloud_with_non_finite_points_needs_an_explicit_camera(built_lib):
    import fast3r_amd
    p = random_cloud(500, 3)
    p[7, 1], p[9, 0] = np.nan, np.inf
    c = colors_of(len(p))
    with pytest.raises(ValueError, match="NaN or inf"):
        fast3r_amd.render_points(dev(p), dev(c), width=16, height=9)
    check(p, c, identity_camera(), 16, 9, 2.0)                                            # with a camera such points are simply not drawn


# ------------------------------------------------------------------------------------------------------------------- contention
def test_contention_on_a_small_viewport_is_deterministic(built_lib):
    """50 000 points with random depths, each covering most of a 4 x 4 viewport: every pixel is fought over by all of them"""
    import fast3r_amd
    rs = np.random.RandomState(2)
    d = rs.uniform(1, 2, 50000)
    p = np.stack([rs.uniform(-0.6, 0.6, 50000) * d, rs.uniform(-0.6, 0.6, 50000) * d, -d], axis=1).astype(F32)
    p[rs.randint(0, 50000, 200)] = p[123]                                                 # and coincident copies of one point
    c = colors_of(len(p))
    want = check(p, c, identity_camera(), 4, 4, 5.0)
    dp, dc = dev(p), dev(c)
    a = fast3r_amd.render_points(dp, dc, identity_camera(), width=4, height=4, point_size=5.0, return_depth=True)
    b = fast3r_amd.render_points(dp, dc, identity_camera(), width=4, height=4, point_size=5.0, return_depth=True)
    assert torch.equal(a[0], b[0]) and a[1].cpu().numpy().tobytes() == b[1].cpu().numpy().tobytes() == want[1].tobytes()
    assert (want[0] != 255).all()


# ------------------------------------------------------------------------------------------------------------------- whole function
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


@pytest.mark.parametrize("sample", [0, 1])
def test_render_cumulative_pts3d_viz_end_to_end(built_lib, tiny_output, tmp_path, sample):
    """what inference() returns goes in as it is; the PNGs hold the returned pictures, which equal the restatement's"""
    import fast3r_amd
    from fast3r_amd import post_ops
    from PIL import Image
    out = tiny_output
    preds = [{k: p[k].float().cpu().numpy() for k in ("pts3d_in_other_view", "conf")} for p in out["preds"]]
    views = [{"img": v["img"].float().cpu().numpy()} for v in out["views"]]
    W, H, pct = 96, 54, 10
    p, c, ends = R.combine(preds, views, pct, sample=sample)
    assert len(p) > 10000 and np.isfinite(p).all()
    gp, gc = fast3r_amd.combine_points(out, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                       min_conf_thr_percentile=pct, sample=sample)
    assert gp.cpu().numpy().tobytes() == p.tobytes() and gc.cpu().numpy().tobytes() == c.tobytes()
    center = post_ops.render_center(gp)
    assert (np.abs(np.array(center) - R.center(p)) <= R.center_bound(p)).all()
    want = R.render(p, c, R.birdseye(center, p.min(0), p.max(0)), W, H, 5.0, segments=ends)
    frames = fast3r_amd.render_cumulative_pts3d_viz(out, None, str(tmp_path), min_conf_thr_percentile=pct, sample=sample, width=W, height=H,
                                                    return_frames=True)
    assert sorted(os.listdir(tmp_path)) == ["cumulative_000.png", "cumulative_001.png", "cumulative_002.png"] and len(frames) == 3
    for i, f in enumerate(frames):
        host = f.cpu().numpy()
        assert host.tobytes() == want[i][0].tobytes(), i
        assert np.array_equal(np.asarray(Image.open(tmp_path / f"cumulative_{i:03d}.png").convert("RGB")), host)
    assert (want[-1][0] != 255).any()
    sub = tmp_path / "sub"
    assert fast3r_amd.render_cumulative_pts3d_viz(out["preds"], out["views"], str(sub), 5.0, pct, sample=sample, width=W, height=H,
                                                  frames=[2]) is None
    assert os.listdir(sub) == ["cumulative_002.png"]
    assert np.array_equal(np.asarray(Image.open(sub / "cumulative_002.png").convert("RGB")), frames[2].cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------- pinhole round trip
def test_pinhole_round_trip(built_lib):
    """an 8 x 12 depth map unprojected with a known focal and the identity pose, drawn at 12 x 8 with one-pixel points through the same
    camera: every pixel gets its own colour back"""
    import fast3r_amd
    H, W, f, pp = 8, 12, 10.0, (5.0, 4.5)
    rs = np.random.RandomState(4)
    z = rs.uniform(1.0, 3.0, (H, W))
    v, u = np.mgrid[0:H, 0:W]
    p = np.stack([(u - pp[0]) * z / f, (v - pp[1]) * z / f, z], axis=-1).reshape(-1, 3).astype(F32)
    c = np.stack([v, u, np.full_like(u, 7)], axis=-1).reshape(-1, 3).astype(np.uint8)
    cam = fast3r_amd.pinhole_camera(np.eye(4), f, pp, H, W)
    image, depth = check(p, c, cam, W, H, 1)
    assert np.array_equal(image, c.reshape(H, W, 3)) and np.array_equal(depth, z.astype(F32))


# ------------------------------------------------------------------------------------------------------------------- centre
@pytest.mark.parametrize("n", [1, 63, 2049, 300007, 2200001])
def test_center_is_within_the_bound_of_two_fp64_sums(built_lib, n):
    """|got - np.sum(p, 0, dtype=float64) / M| <= 2 (M - 1) 2^-53 sum |p_i| / M per axis; one workgroup, several, and more tiles than the
    1024 partials (each first-stage workgroup then strides)"""
    from fast3r_amd import post_ops
    rs = np.random.RandomState(n % 1000)
    p = (rs.randn(n, 3) * [1.0, 30.0, 1e-3] + [100.0, -0.5, 7.0]).astype(F32)
    p[:, 1] *= (10.0 ** rs.uniform(-6, 6, n)).astype(F32)                                 # twelve decades on one axis: sums that do round
    dp = dev(p)
    got = post_ops.render_center(dp)
    err, bound = np.abs(np.array(got) - R.center(p)), R.center_bound(p)
    print(f"centre n = {n}: error {err.tolist()}, bound {bound.tolist()}")
    assert (err <= bound).all()
    assert post_ops.render_center(dp) == got and dp.cpu().numpy().tobytes() == p.tobytes()
