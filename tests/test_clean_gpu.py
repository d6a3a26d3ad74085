"""Confidence cleaning on a real MI355X against the torch restatement (tests/clean_ref.py): the cleaned confidences bit for bit on every
pixel, with no exclusions, and n_lowered exactly -- both are IEEE fp32 in the same order.  The cases are tests/clean_cases.py's and the
smallest shapes at which the kernel can still go wrong."""
import numpy as np
import pytest
import torch

import clean_cases as C
import clean_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
F32 = np.float32


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(s, pairs="complete", frame="world"):
    import fast3r_amd
    pts = [gpu(p) for p in (s["local"] if frame == "camera" else s["world"])]
    conf, lowered = fast3r_amd.clean_confidences(pts, [gpu(c) for c in s["conf"]], [gpu(d) for d in s["depth"]], gpu(s["poses"]),
                                                 gpu(s["intr"][:, :2]), gpu(s["intr"][:, 2:]), tol=s["tol"], max_bad_conf=s["max_bad_conf"],
                                                 pairs=pairs, frame=frame, return_lowered=True)
    assert all(c.is_cuda and c.dtype == torch.float32 for c in conf) and lowered.dtype == np.int64
    return [c.cpu().numpy() for c in conf], lowered.tolist()


def check(s, pairs="complete", nbrs=None, frame="world", what=""):
    got, lowered = run(s, pairs, frame)
    ref, ref_lowered = R.clean_ref(s, nbrs, frame=frame)
    print(f"{what}: {len(s['shapes'])} views, lowered {lowered[:12]}")
    assert lowered == ref_lowered, (what, lowered, ref_lowered)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == tuple(s["shapes"][i]) and g.tobytes() == r.numpy().tobytes(), (what, i, int((g != r.numpy()).sum()))
    return got, lowered


def small_scene(shapes, seed, tol=0.001, max_bad_conf=0.0, **kw):
    s = C.scene(shapes, seed, **kw)
    s["tol"], s["max_bad_conf"] = tol, max_bad_conf
    return s


# ------------------------------------------------------------------------------------------------------------------- golden recipes, shapes
@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_golden_recipes_match_the_restatement(built_lib, name):
    s = C.golden_scene(name)
    _, lowered = check(s, what=name)
    assert sum(lowered) >= 0.02 * sum(h * w for h, w in s["shapes"])


def test_one_view_changes_nothing(built_lib):
    s = small_scene([(5, 7)], 1)
    got, lowered = check(s, what="one view")
    assert lowered == [0] and got[0].tobytes() == s["conf"][0].tobytes()


def test_two_views_of_one_pixel(built_lib):
    """focal 1, principal point (0, 0), identity poses: both pixels lie on the axis.  View 0's point at depth 2 hangs in front of view 1's
    depth 4 with the lower confidence"""
    one = lambda v: np.full((1, 1), v, dtype=F32)  # noqa: E731
    s = {"world": [np.array([[0, 0, 2]], dtype=F32), np.array([[0, 0, 4]], dtype=F32)], "conf": [one(1.5), one(3.0)], "depth": [one(2), one(4)],
         "shapes": [(1, 1)] * 2, "poses": np.stack([np.eye(4, dtype=F32)] * 2), "intr": np.array([[1, 1, 0, 0]] * 2, dtype=F32), "tol": 0.001,
         "max_bad_conf": 0.0}
    got, lowered = check(s, what="1 x 1")
    assert lowered == [1, 0] and got[0][0, 0] == 0.0 and got[1][0, 0] == 3.0


@pytest.mark.parametrize("shape", [(5, 7), (17, 19), (16, 16)])
def test_less_than_a_wave_one_block_and_a_partial_wave(built_lib, shape):
    _, lowered = check(small_scene([shape] * 3, 21 + shape[0]), what=f"{shape}")
    assert sum(lowered) > 0


def test_mixed_landscape_and_portrait(built_lib):
    _, lowered = check(small_scene([(6, 8), (8, 6), (6, 8), (8, 6)], 31, floaters=0.2), what="6 x 8 with 8 x 6")
    assert sum(lowered) > 0


# ------------------------------------------------------------------------------------------------------------------- the order of the views
def test_order_case_sequential_not_jacobi(built_lib):
    s = C.order_case()
    got, lowered = check(s, what="order")
    assert lowered == [1, 0, 0] and got[0][0, 0] == 0.0 and got[1][0, 0] == 1.0           # the sequential answer keeps view 1's pixel
    jac, jac_lowered = R.clean_ref(s, jacobi=True)
    assert jac_lowered == [1, 1, 0] and float(jac[1][0, 0]) == 0.0                           # a Jacobi evaluation lowers it: the case has teeth
    rev, rev_lowered = check(C.reversed_views(s), what="order reversed")
    assert rev_lowered == [0, 1, 1] and rev[1][0, 0] == 0.0 and rev[2][0, 0] == 0.0          # reversed, the same pixel is lowered


# ------------------------------------------------------------------------------------------------------------------- exact boundary values
def boundary_scene():
    """Identity cameras, focal 2, principal point (0, 0), tol = 0.5 (so (float)(1 - tol) = 0.5 and the limit of depth 4 is exactly 2).  A point
    (X, Y, 1) projects to u = 2 X, v = 2 Y exactly.  View 0 is a 1 x 10 strip of test points with confidence 1 (point 6: 5); views 1 (2 x 4)
    and 2 (2 x 5) show depth 4 with confidence 5 everywhere."""
    pts = np.array([[-0.25, 0, 1],    # 0: u = -0.5 rounds to -0: in the image, lowered
                    [1.75, 0, 1],     # 1: u = 3.5 rounds to 4 (even): outside W = 4, inside W = 5
                    [2.25, 0, 1],     # 2: u = 4.5 rounds to 4 (even): outside W = 4, inside W = 5
                    [1.25, 0, 1],     # 3: u = 2.5 rounds to 2: inside both
                    [0, 0, 2],        # 4: z == (1 - tol) d exactly: not in front (strict <)
                    [0, 0, np.nextafter(F32(2), F32(0))],  # 5: one ulp nearer: in front
                    [0.5, 0.5, 1],    # 6: equal confidences (5 against 5): kept
                    [0.5, 0.5, 0],    # 7: z = 0: u = inf
                    [0.5, 0.5, -1],   # 8: behind the camera
                    [0, 0.75, 1]],    # 9: v = 1.5 rounds to 2: outside H = 2
                   dtype=F32)
    conf0 = np.ones((1, 10), dtype=F32)
    conf0[0, 6] = 5.0
    far = lambda H, W: np.stack([np.zeros(H * W), np.zeros(H * W), np.full(H * W, 4.0)], 1).astype(F32)  # noqa: E731
    shapes = [(1, 10), (2, 4), (2, 5)]
    return {"world": [pts, far(2, 4), far(2, 5)], "conf": [conf0, np.full((2, 4), 5, F32), np.full((2, 5), 5, F32)],
            "depth": [pts[:, 2].reshape(1, 10).copy(), np.full((2, 4), 4, F32), np.full((2, 5), 4, F32)], "shapes": shapes,
            "poses": np.stack([np.eye(4, dtype=F32)] * 3), "intr": np.array([[2, 2, 0, 0]] * 3, dtype=F32), "tol": 0.5, "max_bad_conf": 0.0}


@pytest.mark.parametrize("other,expect", [(1, [0, 3, 5]), (2, [0, 1, 2, 3, 5])])
def test_boundary_values_exact_in_fp32(built_lib, other, expect):
    s = boundary_scene()
    got, lowered = check(s, pairs=[(0, other)], nbrs=C.lists_of([(0, other)], 3), what=f"boundaries against W = {s['shapes'][other][1]}")
    assert np.flatnonzero(got[0][0] == 0.0).tolist() == expect and lowered == [len(expect), 0, 0]


# ------------------------------------------------------------------------------------------------------------------- values and arguments
def test_nan_and_inf_never_lower_and_never_raise(built_lib):
    s = small_scene([(8, 9)] * 3, 41, floaters=0.2)
    rs = np.random.RandomState(3)
    for i in range(3):
        w, c, d = s["world"][i], s["conf"][i].reshape(-1), s["depth"][i].reshape(-1)
        for arr, vals in ((w[:, 0], (np.nan, np.inf)), (w[:, 2], (np.nan, -np.inf, np.inf)), (c, (np.nan, np.inf, -np.inf)), (d, (np.nan, np.inf, -np.inf))):
            for val in vals:
                arr[rs.randint(0, arr.shape[0], 3)] = val
    got, lowered = check(s, what="NaN and inf")
    for i in range(3):
        nan = np.isnan(s["conf"][i])
        assert nan.any() and np.isnan(got[i][nan]).all() and not np.isnan(got[i][~nan]).any()
    assert sum(lowered) > 0


def test_tol_zero_and_max_bad_conf_above_some_confidences(built_lib):
    _, lowered = check(small_scene([(9, 11)] * 3, 51, tol=0.0, floaters=0.2), what="tol = 0")
    assert sum(lowered) > 0
    s = small_scene([(9, 11)] * 3, 52, max_bad_conf=3.0, slope=0.0, rot=0.05, floaters=0.3)
    got, lowered = check(s, what="max_bad_conf = 3")
    flagged_below = sum(int(((g == c) & (c < 3.0) & f).sum()) for g, c, f in zip(got, s["conf"], s["floater"]))
    assert sum(lowered) > 0 and flagged_below > 0 and all((g[g != c] == 3.0).all() for g, c in zip(got, s["conf"]))


def test_sparse_graphs_against_the_same_lists(built_lib):
    from fast3r_amd import scene_graph_pairs
    s = small_scene([(7, 9)] * 5, 61, floaters=0.2)
    nbrs = C.lists_of(scene_graph_pairs(5, "swin-1", symmetrize=False).tolist(), 5)
    assert nbrs == [[1, 4], [0, 2], [1, 3], [2, 4], [0, 3]]
    _, lowered = check(s, pairs="swin-1", nbrs=nbrs, what="swin-1")
    assert sum(lowered) > 0
    got, lowered = check(s, pairs=[], nbrs=[[]] * 5, what="no pairs")
    assert lowered == [0] * 5 and all(g.tobytes() == c.tobytes() for g, c in zip(got, s["conf"]))


def test_three_hundred_views(built_lib):
    """more views than any staging of the table would hold, and 300 launches"""
    _, lowered = check(small_scene([(2, 3)] * 300, 71, floaters=0.2), what="300 views")
    assert sum(lowered) > 100


def test_camera_frame_equals_world_frame_on_transformed_points(built_lib):
    """frame='camera' applies the pose in fp32 in the fixed order: fed the restatement's transformed points, frame='world' gives the same bits"""
    s = small_scene([(10, 12)] * 4, 81, slope=0.2, rot=0.15, floaters=0.2)
    got_cam, low_cam = check(s, frame="camera", what="camera frame")
    t = dict(s)
    poses = torch.from_numpy(s["poses"])
    t["world"] = [torch.stack(R._affine(poses[i], *torch.from_numpy(p).unbind(1)), 1).numpy() for i, p in enumerate(s["local"])]
    got_world, low_world = check(t, frame="world", what="world frame, transformed points")
    assert low_cam == low_world and sum(low_cam) > 0 and all(a.tobytes() == b.tobytes() for a, b in zip(got_cam, got_world))


def test_inputs_are_unchanged_and_stacked_inputs_come_back_stacked(built_lib):
    import fast3r_amd
    s = small_scene([(6, 7)] * 3, 91, floaters=0.3)
    args = [torch.stack([gpu(p) for p in s["world"]]), torch.stack([gpu(c) for c in s["conf"]]), torch.stack([gpu(d) for d in s["depth"]]),
            gpu(s["poses"]), gpu(s["intr"][:, :2]), gpu(s["intr"][:, 2:])]
    before = [a.clone() for a in args]
    out = fast3r_amd.clean_confidences(*args, tol=s["tol"], max_bad_conf=0)
    ref, _ = R.clean_ref(s)
    assert torch.is_tensor(out) and out.shape == (3, 6, 7) and out.data_ptr() != args[1].data_ptr()
    assert out.cpu().numpy().tobytes() == torch.stack(ref).numpy().tobytes() and not torch.equal(out, args[1])
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(args, before))
    # numpy in, the same numbers out, on the host
    host = fast3r_amd.clean_confidences(s["world"], s["conf"], s["depth"], s["poses"], s["intr"][:, 0], s["intr"][:, 2:], tol=s["tol"])
    same_f = dict(s, intr=np.concatenate([s["intr"][:, :1], s["intr"][:, :1], s["intr"][:, 2:]], 1))
    assert all(not h.is_cuda for h in host) and all(h.numpy().tobytes() == r.numpy().tobytes() for h, r in zip(host, R.clean_ref(same_f)[0]))


def test_singular_pose_raises(built_lib):
    import fast3r_amd
    s = small_scene([(4, 5)] * 3, 95)
    s["poses"] = s["poses"].copy()
    s["poses"][1, :3, 2] = 0.0
    with pytest.raises(ValueError, match="no inverse"):
        run(s)
    s["poses"][1] = np.nan
    with pytest.raises(ValueError, match="no inverse"):
        run(s)
    assert hasattr(fast3r_amd.MultiViewDUSt3RLitModule, "clean_pointcloud")


# ------------------------------------------------------------------------------------------------------------------- a forward pass
def test_clean_pointcloud_end_to_end(built_lib):
    """synthetic preds at N = 4, 16 x 24 with known poses and focals: both heads against the restatement, and the result through the consumers"""
    import fast3r_amd
    H, W, N = 16, 24, 4
    s = small_scene([(H, W)] * N, 97, slope=0.2, rot=0.15, floaters=0.15, focal=22.0)
    s["intr"][:, 1] = s["intr"][:, 0]
    s["intr"][:, 2:] = [W / 2, H / 2]   # what clean_pointcloud assumes: one focal, the principal point at the centre
    rs = np.random.RandomState(5)
    other = rs.uniform(1, 6, (N, H, W)).astype(F32)
    preds = []
    for i in range(N):
        preds.append({"pts3d_local": gpu(s["local"][i].reshape(1, H, W, 3)), "conf_local": gpu(s["conf"][i][None]),
                      "pts3d_in_other_view": gpu(s["world"][i].reshape(1, H, W, 3)), "conf": gpu(other[i][None]),
                      "pts3d_local_aligned_to_global": gpu(s["world"][i].reshape(1, H, W, 3))})
    views = [{"img": gpu(rs.uniform(-1, 1, (1, 3, H, W)).astype(F32))} for _ in range(N)]
    poses, focals = gpu(s["poses"]), gpu(s["intr"][:, 0])
    before = [{k: v.clone() for k, v in p.items()} for p in preds]
    local = fast3r_amd.MultiViewDUSt3RLitModule.clean_pointcloud(preds, views, poses=poses, focals=focals)
    ref, ref_lowered = R.clean_ref(s, frame="camera")
    assert isinstance(local, fast3r_amd.CleanedCloud) and local.n_lowered.tolist() == ref_lowered and sum(ref_lowered) > 0
    for i in range(N):
        assert local.conf[i].cpu().numpy().tobytes() == ref[i].numpy().tobytes()
        assert torch.equal(local.kept[i].cpu(), ref[i] == torch.from_numpy(s["conf"][i])) and local.kept[i].dtype == torch.bool
        assert local.preds[i]["conf_local"].shape == (1, H, W) and torch.equal(local.preds[i]["conf_local"][0], local.conf[i])
        assert local.preds[i]["conf"] is preds[i]["conf"] and local.preds[i] is not preds[i]
        assert all(torch.equal(preds[i][k], before[i][k]) for k in preds[i])
    g = dict(s, conf=list(other))
    glob = fast3r_amd.clean_pointcloud({"preds": preds, "views": views}, poses=poses, focals=focals, head="global", tol=0.01, max_bad_conf=1.0)
    g["tol"], g["max_bad_conf"] = 0.01, 1.0
    gref, gref_lowered = R.clean_ref(g, frame="world")
    assert glob.n_lowered.tolist() == gref_lowered and all(glob.conf[i].cpu().numpy().tobytes() == gref[i].numpy().tobytes() for i in range(N))
    assert all(torch.equal(glob.preds[i]["conf"][0], glob.conf[i]) and glob.preds[i]["conf_local"] is preds[i]["conf_local"] for i in range(N))
    # the consumers take the preds unchanged and the masks as theirs
    scene = fast3r_amd.assemble_scene(glob.preds, views, not_sky=glob.kept, poses=False)
    assert scene is not None
    assert fast3r_amd.build_mesh(glob.preds, views, head="global", min_conf_thr_percentile=10).faces.shape[0] > 0
    # on the same confidences (the same per-view thresholds) the masks take away the faces that touch a lowered pixel
    masked = fast3r_amd.build_mesh(preds, views, head="global", min_conf_thr_percentile=10, valid=glob.kept)
    plain = fast3r_amd.build_mesh(preds, views, head="global", min_conf_thr_percentile=10)
    assert 0 < masked.faces.shape[0] < plain.faces.shape[0]
    # without poses the solve of estimate_camera_poses_device supplies them: it runs, and nothing it lowers is a NaN
    solved = fast3r_amd.clean_pointcloud(preds, head="global", pairs="swin-1")
    assert len(solved.conf) == N and all(c.shape == (H, W) and not torch.isnan(c).any() for c in solved.conf)
