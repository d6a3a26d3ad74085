"""Seeded inputs of the global-alignment tests, shared by tests/test_global_align.py (CPU), tests/test_global_align_gpu.py and
tools/make_golden_galign.py.  numpy only; everything is built in float64 and rounded to float32 once.

Two kinds of input:
* `matrix_problem`: the kernel's own inputs (poses, focals, principal points, log depths, pairwise matrices, adaptors, one pointmap and one
  weight map per (edge, side)) drawn at scene size, for the geometry tests;
* `raw_case`: what the reference's `PointCloudOptimizer` takes -- (view1, view2, pred1, pred2) -- and a full set of its raw parameters, the
  true ones of a synthetic scene moved by a seeded perturbation, for the golden file and the loop tests."""
import numpy as np

F32 = np.float32

SYM3 = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)]
STAR5 = [(0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (2, 0), (3, 0), (4, 0)]  # view 0 has 8 observations, the others 2
MIXED4 = [(0, 1), (0, 2), (1, 2), (3, 0), (2, 3)]  # not symmetrised
MIXED4_SHAPES = ((24, 32), (32, 24), (24, 32), (32, 24))

# name -> (shapes, edges, dist, conf, seed, noise of the pairwise pointmaps).  A recipe that breaks a margin condition of
# tools/make_golden_galign.py gets another seed, never a wider cap.
GOLDEN = {
    "two_l1_log": (((6, 8),) * 2, [(0, 1)], "l1", "log", 101, 0.02),
    "two_l2_id": (((6, 8),) * 2, [(0, 1)], "l2", "id", 102, 0.02),
    "sym3_l1_m1": (((6, 8),) * 3, SYM3, "l1", "m1", 103, 0.02),
    "sym3_l2_sqrt": (((6, 8),) * 3, SYM3, "l2", "sqrt", 104, 0.02),
    "mixed4_l1_log": (MIXED4_SHAPES, MIXED4, "l1", "log", 105, 0.02),
    "mixed4_l2_m1": (MIXED4_SHAPES, MIXED4, "l2", "m1", 106, 0.02),
    "star5_l1_sqrt": (((6, 8),) * 5, STAR5, "l1", "sqrt", 107, 0.02),
    "star5_l2_log": (((6, 8),) * 5, STAR5, "l2", "log", 108, 0.02),
}
# the loop case: exact pairwise pointmaps, the reference's default switches (no adaptors, fixed principal points)
LOOP = (((6, 8),) * 3, SYM3, "l1", "log", 201, 0.0)
LOOP_NITER, LOOP_LR = 100, 0.01
BASE_SCALE, PW_BREAK, FOCAL_BREAK = 0.5, 20, 20
CONF_ONE_SHARE = 0.1  # confidences exactly 1: weight 0 under conf="log" and "m1"


# ------------------------------------------------------------------------------------------------------------------- rotations
def quat_to_rotmat(q):
    """(x, y, z, w), normalised here"""
    x, y, z, w = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def small_quat(rs, angle):
    """a rotation by at most about `angle` radians around a random axis, as (x, y, z, w)"""
    v = rs.uniform(-1, 1, 3) * angle / 2
    return np.array([v[0], v[1], v[2], 1.0])


def signed_log1p(x):
    return np.sign(x) * np.log1p(np.abs(x))


# ------------------------------------------------------------------------------------------------------------------- kernel-level problems
def observation_lists(n_views, edges):
    """per view the observations o = 2 e + side that belong to it, ascending"""
    lists = [[] for _ in range(n_views)]
    for e, (i, j) in enumerate(edges):
        lists[i].append(2 * e)
        lists[j].append(2 * e + 1)
    return lists


def matrix_problem(shapes, edges, seed, zero_share=0.1, share_maps=False):
    """The kernel's inputs at scene size: cameras near the origin looking down +z at depths around 3, pairwise matrices close to the pose of the
    edge's first view with scales around 0.5, pointmaps that land near the world points up to 10 % noise, weights in [0, 2] with a seeded share
    exactly 0.  share_maps: every observation of a view uses one pointmap and one weight map (the same arrays, by identity)."""
    rs = np.random.RandomState(seed)
    N, E = len(shapes), len(edges)
    poses = np.zeros((N, 3, 4))
    for v in range(N):
        poses[v, :, :3] = quat_to_rotmat(small_quat(rs, 0.3))
        poses[v, :, 3] = rs.uniform(-0.5, 0.5, 3)
    focals = np.array([0.9 * max(H, W, 2) * rs.uniform(0.9, 1.2) for H, W in shapes])
    pp = np.array([[W / 2 + rs.uniform(-0.4, 0.4), H / 2 + rs.uniform(-0.4, 0.4)] for H, W in shapes])
    log_depth = [np.log(rs.uniform(2.0, 4.0, (H, W))) for H, W in shapes]
    poses, focals, pp, log_depth = poses.astype(F32), focals.astype(F32), pp.astype(F32), [d.astype(F32) for d in log_depth]
    world = []
    for v, (H, W) in enumerate(shapes):
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        d = np.exp(log_depth[v].astype(np.float64))
        q = np.stack([d * (xs - pp[v, 0]) / focals[v], d * (ys - pp[v, 1]) / focals[v], d], -1)
        world.append(q @ poses[v, :, :3].astype(np.float64).T + poses[v, :, 3].astype(np.float64))
    pw, adapt = np.zeros((E, 3, 4)), np.zeros((E, 3))
    for e, (i, j) in enumerate(edges):
        s = 0.5 * np.exp(rs.uniform(-0.2, 0.2))
        R = poses[i, :, :3].astype(np.float64) @ quat_to_rotmat(small_quat(rs, 0.05))
        pw[e, :, :3], pw[e, :, 3] = s * R, poses[i, :, 3] + rs.uniform(-0.05, 0.05, 3)
        adapt[e] = np.exp(rs.uniform(-0.05, 0.05, 3))
    pw, adapt = pw.astype(F32), adapt.astype(F32)
    pts, w, own = [], [], {}
    for e, (i, j) in enumerate(edges):
        for v in (i, j):
            if share_maps and v in own:
                p, ww = own[v]
            else:
                H, W = shapes[v]
                S, m = pw[e, :, :3].astype(np.float64), pw[e, :, 3].astype(np.float64)
                p = ((world[v] - m) @ np.linalg.inv(S).T) / adapt[e].astype(np.float64)
                p = (p * (1 + 0.1 * rs.uniform(-1, 1, p.shape))).astype(F32)
                ww = rs.uniform(0.0, 2.0, (H, W))
                ww[rs.uniform(0, 1, (H, W)) < zero_share] = 0.0
                ww = ww.astype(F32)
                own[v] = (p, ww)
            pts.append(p)
            w.append(ww)
    return {"shapes": [tuple(s) for s in shapes], "edges": [tuple(e) for e in edges], "poses": poses, "focals": focals, "pp": pp,
            "log_depth": log_depth, "pw": pw, "adapt": adapt, "pts": pts, "w": w}


def exact_problem():
    """identity pose, f = 1, principal point on the pixel, l = 0, prediction (0, 0, 1), identity pairwise pose: r = 0 exactly.  Two views of
    1 x 1 with one edge."""
    z = lambda *s: np.zeros(s, dtype=F32)  # noqa: E731
    eye = np.concatenate([np.eye(3, dtype=F32), z(3, 1)], axis=1)
    one = np.array([[[0, 0, 1]]], dtype=F32)
    return {"shapes": [(1, 1), (1, 1)], "edges": [(0, 1)], "poses": np.stack([eye, eye]), "focals": np.ones(2, F32), "pp": z(2, 2),
            "log_depth": [z(1, 1), z(1, 1)], "pw": eye[None].copy(), "adapt": np.ones((1, 3), F32), "pts": [one, one.copy()],
            "w": [np.full((1, 1), 1.5, F32), np.full((1, 1), 0.5, F32)]}


# ------------------------------------------------------------------------------------------------------------------- optimizer-level cases
def raw_case(shapes, edges, dist, conf, seed, noise):
    """A synthetic scene -- cameras near the origin looking at a slanted plane -- as the optimizer's inputs and a full set of raw parameters.
    Edge e = (i, j) predicts view i's and view j's points in camera i's frame, divided by the edge's scale sigma_e = base_scale exp(delta_e -
    mean delta) (the scale its pairwise pose has after the reference's normalisation), times 1 + noise u, u uniform in [-1, 1].  The raw
    parameters are the true ones plus a seeded perturbation of a few per cent, so that residuals are scene-sized."""
    rs = np.random.RandomState(seed)
    N, E = len(shapes), len(edges)
    n = np.array([-0.2, -0.1, 1.0])  # the plane n . X = 3
    R, t, f, depth, world = [], [], [], [], []
    for v, (H, W) in enumerate(shapes):
        Rv = quat_to_rotmat(small_quat(rs, 0.3 if v else 0.0))
        tv = rs.uniform(-0.5, 0.5, 3) * np.array([1.0, 1.0, 0.3]) * (1 if v else 0)
        fv = 0.9 * max(H, W) * rs.uniform(0.95, 1.15)
        ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
        ray = np.stack([(xs - W / 2) / fv, (ys - H / 2) / fv, np.ones((H, W))], -1)
        d = (3.0 - n @ tv) / (ray @ Rv.T @ n)
        R.append(Rv), t.append(tv), f.append(fv), depth.append(d)
        world.append((ray * d[..., None]) @ Rv.T + tv)
    delta = rs.uniform(-0.3, 0.3, E)
    sigma = BASE_SCALE * np.exp(delta - delta.mean())
    pts_i, pts_j, conf_i, conf_j = [], [], [], []
    for e, (i, j) in enumerate(edges):
        for v, pts, cf in ((i, pts_i, conf_i), (j, pts_j, conf_j)):
            H, W = shapes[v]
            p = ((world[v] - t[i]) @ R[i]) / sigma[e]
            p = p * (1 + noise * rs.uniform(-1, 1, p.shape))
            c = 1.0 + rs.uniform(0.1, 5.0, (H, W))
            c[rs.uniform(0, 1, (H, W)) < CONF_ONE_SHARE] = 1.0
            pts.append(p.astype(F32)), cf.append(c.astype(F32))
    # the true raw parameters, then the perturbation
    quat = lambda Rm: _rotmat_to_quat(Rm)  # noqa: E731
    pw_poses = np.stack([np.concatenate([quat(R[i]), signed_log1p(t[i] / sigma[e]), [delta[e]]]) for e, (i, j) in enumerate(edges)])
    im_poses = np.stack([np.concatenate([quat(R[v]), signed_log1p(t[v])]) for v in range(N)])
    im_focals = np.array([[FOCAL_BREAK * np.log(f[v])] for v in range(N)])
    pw_poses[:, :4] += rs.uniform(-0.03, 0.03, (E, 4))
    pw_poses[:, 4:7] += rs.uniform(-0.05, 0.05, (E, 3))
    pw_poses[:, 7] += rs.uniform(-0.05, 0.05, E)
    im_poses[:, :4] += rs.uniform(-0.03, 0.03, (N, 4))
    im_poses[:, 4:7] += rs.uniform(-0.05, 0.05, (N, 3))
    im_focals += rs.uniform(-0.5, 0.5, (N, 1))
    return {"shapes": [tuple(s) for s in shapes], "edges": [tuple(e) for e in edges], "dist": dist, "conf": conf,
            "pts_i": pts_i, "pts_j": pts_j, "conf_i": conf_i, "conf_j": conf_j,
            "pw_poses": pw_poses.astype(F32), "pw_adaptors": rs.uniform(-1.0, 1.0, (E, 2)).astype(F32), "im_poses": im_poses.astype(F32),
            "im_focals": im_focals.astype(F32), "im_pp": rs.uniform(-0.05, 0.05, (N, 2)).astype(F32),
            "im_depthmaps": [(np.log(d) + rs.uniform(-0.05, 0.05, d.shape)).astype(F32) for d in depth],
            "true": {"R": R, "t": t, "f": f, "depth": depth, "sigma": sigma}}


def _rotmat_to_quat(R):
    """(x, y, z, w) with w > 0: the test rotations are small"""
    w = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-12)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])


def golden_case(name):
    return raw_case(*GOLDEN[name])


def loop_case():
    return raw_case(*LOOP)


def optimizer_inputs(c, wrap=lambda a: a):
    """(view1, view2, pred1, pred2) of a raw case; wrap turns every array into what the optimizer under test takes"""
    view1 = {"idx": [i for i, j in c["edges"]]}
    view2 = {"idx": [j for i, j in c["edges"]]}
    pred1 = {"pts3d": [wrap(p) for p in c["pts_i"]], "conf": [wrap(x) for x in c["conf_i"]]}
    pred2 = {"pts3d_in_other_view": [wrap(p) for p in c["pts_j"]], "conf": [wrap(x) for x in c["conf_j"]]}
    return view1, view2, pred1, pred2


RAW_NAMES = ("pw_poses", "pw_adaptors", "im_poses", "im_focals", "im_pp", "im_depthmaps")
MATRIX_NAMES = ("d_log_depth", "d_poses", "d_focals", "d_pp", "d_pw", "d_adapt")
