"""Seeded inputs of the confidence-cleaning tests, shared by tests/test_clean.py (CPU), tests/test_clean_gpu.py and
tools/make_golden_clean.py.  A scene is a dict of per-view lists: local (H W, 3) points in the view's own camera, world (H W, 3) points, conf
and depth (H, W), plus poses (N, 4, 4) camera-to-world, intr (N, 4) = fx, fy, cx, cy and shapes; everything is built in float64 and rounded
to float32 once.  numpy only."""
import numpy as np

F32 = np.float32

# the golden recipes: name -> (shapes, seed, tol, max_bad_conf, surface slope, camera rotation in radians).  Three scenes of 6 views at
# 24 x 32 and one of 5 views mixing landscape and portrait; tol 0.03 twice and the default 0.001 twice; max_bad_conf 1.2 once, so that some
# flagged pixels lie below it and keep their value.  With tol = 0.001 the surface faces the cameras: across half a pixel its depth then moves
# by less than tol, and what is lowered is a floater or hidden, not a slope.
GOLDEN = {
    "six_tol3": (((24, 32),) * 6, 11, 0.03, 0.0, 0.2, 0.15),
    "six_tol3_keep": (((24, 32),) * 6, 12, 0.03, 1.2, 0.2, 0.15),
    "six_default": (((24, 32),) * 6, 13, 0.001, 0.0, 0.0, 0.01),
    "mixed_default": (((24, 32), (32, 24), (24, 32), (32, 24), (24, 32)), 14, 0.001, 0.0, 0.0, 0.01),
}
FLOATER_SHARE = 0.08


def _rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def scene(shapes, seed, slope=0.2, rot=0.15, floaters=FLOATER_SHARE, focal=None):
    """N cameras near the origin looking down +z at the plane z = 3 + slope x + slope / 2 y.  Pixel (u, v) of a view holds the point where its
    ray meets the plane; a seeded share of the pixels is pulled towards the camera along the ray (to 40 % .. 80 % of the depth) with a low
    confidence in [1, 1.4]: the floaters.  The other confidences lie in [1.5, 6].  View 0 has the identity pose."""
    rs = np.random.RandomState(seed)
    n = np.array([-slope, -slope / 2, 1.0])  # n . X = 3
    out = {"local": [], "world": [], "conf": [], "depth": [], "shapes": [tuple(s) for s in shapes], "floater": []}
    poses, intr = [], []
    for i, (H, W) in enumerate(shapes):
        T = np.eye(4)
        if i:
            T[:3, :3] = _rotation(*(rot * rs.uniform(-1, 1, 3)))
            T[:3, 3] = rs.uniform(-0.5, 0.5, 3) * np.array([1.0, 1.0, 0.3])
        f = float(focal) if focal is not None else 0.9 * max(H, W) * rs.uniform(0.95, 1.15)
        fx, fy, cx, cy = f, f * rs.uniform(0.97, 1.03), W / 2 + rs.uniform(-0.4, 0.4), H / 2 + rs.uniform(-0.4, 0.4)
        vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
        ray = np.stack([(uu - cx) / fx, (vv - cy) / fy, np.ones((H, W))], -1).reshape(-1, 3)  # z = 1 in the camera
        t = (3.0 - n @ T[:3, 3]) / (ray @ T[:3, :3].T @ n)
        fl = rs.uniform(0, 1, H * W) < floaters
        t = np.where(fl, t * rs.uniform(0.4, 0.8, H * W), t)
        conf = np.where(fl, rs.uniform(1.0, 1.4, H * W), rs.uniform(1.5, 6.0, H * W))
        local = ray * t[:, None]
        T32 = T.astype(F32)
        local32 = local.astype(F32)
        world = local32.astype(np.float64) @ T32[:3, :3].astype(np.float64).T + T32[:3, 3].astype(np.float64)
        out["local"].append(local32)
        out["world"].append(world.astype(F32))
        out["conf"].append(conf.astype(F32).reshape(H, W))
        out["depth"].append(local32[:, 2].reshape(H, W).copy())
        out["floater"].append(fl.reshape(H, W))
        poses.append(T32)
        intr.append([fx, fy, cx, cy])
    out["poses"] = np.stack(poses)
    out["intr"] = np.asarray(intr, dtype=F32)
    return out


def golden_scene(name):
    shapes, seed, tol, max_bad, slope, rot = GOLDEN[name]
    s = scene(shapes, seed, slope, rot)
    s["tol"], s["max_bad_conf"] = tol, max_bad
    return s


def complete(n):
    return [[j for j in range(n) if j != i] for i in range(n)]


def lists_of(pairs, n):
    """neighbour lists of explicit rows (i, j): both directions, no self, ascending"""
    sets = [set() for _ in range(n)]
    for i, j in pairs:
        if i != j:
            sets[i].add(j)
            sets[j].add(i)
    return [sorted(s) for s in sets]


def order_case():
    """Three views of 2 x 2, focal 1, principal point (1, 1): pixel (u, v) is the ray (u - 1, v - 1, 1).  Views 0 and 1 have the identity pose,
    view 2 stands at (-2, 0, 0).  Every pixel holds its ray's point at depth 4 with confidence 5, except pixel (0, 0) of
      view 0: P0 = (-2, -2, 2), confidence 2.  In view 2 it lands on (u, v) = (1, 0), depth 4, confidence 5: view 2 lowers it to 0.  In view 1
              it lands on (0, 0), whose depth 1 lies in front of it;
      view 1: P1 = (-1, -1, 1), confidence 1.  In view 0 it lands on (0, 0) in front of P0's depth 2; in view 2 on u = 2, outside the image.
    A point at depth 4 is in front of nothing here.  Sequentially view 1 meets view 0's cleaned confidence 0 and keeps its 1; a Jacobi
    evaluation compares with view 0's input 2 and lowers it.  With the views reversed view 1 comes before view 0, meets the input 2 and
    is lowered.  Every number is exact in fp32."""
    H = W = 2
    vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
    ray = np.stack([uu - 1.0, vv - 1.0, np.ones((H, W))], -1).reshape(-1, 3)
    depth = [np.full(4, 4.0) for _ in range(3)]
    conf = [np.full(4, 5.0) for _ in range(3)]
    depth[0][0], conf[0][0] = 2.0, 2.0
    depth[1][0], conf[1][0] = 1.0, 1.0
    poses = np.stack([np.eye(4, dtype=F32)] * 3)
    poses[2, 0, 3] = -2.0
    local = [(ray * d[:, None]).astype(F32) for d in depth]
    world = [x + poses[i, :3, 3][None, :] for i, x in enumerate(local)]
    return {"local": local, "world": world, "conf": [c.astype(F32).reshape(H, W) for c in conf],
            "depth": [d.astype(F32).reshape(H, W) for d in depth], "shapes": [(H, W)] * 3, "poses": poses,
            "intr": np.asarray([[1.0, 1.0, 1.0, 1.0]] * 3, dtype=F32), "tol": 0.001, "max_bad_conf": 0.0}


def reversed_views(s):
    r = dict(s)
    for k in ("local", "world", "conf", "depth", "shapes"):
        r[k] = list(s[k])[::-1]
    r["poses"], r["intr"] = s["poses"][::-1].copy(), s["intr"][::-1].copy()
    return r
