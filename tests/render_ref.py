"""Plain-numpy restatement of the point-splat renderer (fast3r_amd/render.py, fast3r_amd/csrc/f3r_render.hip), in this project's own
words: fp64, every operation a numpy operation of its own (numpy never fuses a multiply with an add), painter-free -- per pixel the
minimum over the points that cover it of (bits of the fp32 eye distance, point index).  Also the two camera helpers of the reference's
notebook, written from their description, pyrender's use of a node pose, and its infinite perspective matrix multiplied out the long way.
A camera is anything with .view (12 floats, the 3 x 4 world-to-eye matrix row-major), .sx, .sy, .cx, .cy, .znear."""
import collections

import numpy as np

Cam = collections.namedtuple("Cam", "view sx sy cx cy znear")
EMPTY = np.uint64(0xffffffffffffffff)


# ------------------------------------------------------------------------------------------------------------------- cameras
def create_camera_pose(position, target, up):
    """camera-to-world: columns right, up, forward, position; forward points from the camera to the target, right = up x forward"""
    position, target, up = (np.array(a, dtype=np.float64) for a in (position, target, up))
    with np.errstate(all="ignore"):
        fwd = target - position
        fwd /= np.linalg.norm(fwd)
        right = np.cross(up, fwd)
        if np.linalg.norm(right) < 1e-6:
            up = np.array([0, 0, 1]) if up[1] != 1 else np.array([1, 0, 0])
            right = np.cross(up, fwd)
        right /= np.linalg.norm(right)
        up = np.cross(fwd, right)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, up, fwd, position
    return m


def convert_c2w_to_opengl_view(c2w):
    """world-to-camera, then the y and z axes flipped on the right"""
    flip = np.array([[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 0], [0, 0, 0, 1]], dtype=np.float64)
    with np.errstate(all="ignore"):
        return np.linalg.inv(c2w) @ flip


def notebook_node_pose(center, min_bound, max_bound):
    """what the notebook hands to pyrender as the camera node's pose: the 'OpenGL view matrix' of a camera 2 max_extent above the centre"""
    center = np.asarray(center, dtype=np.float64)
    extent = np.asarray(max_bound, np.float32) - np.asarray(min_bound, np.float32)          # fp32, as numpy subtracts the fp32 cloud's bounds
    distance = np.max(extent) * 2
    position = center + np.array([0, 0, distance])
    return convert_c2w_to_opengl_view(create_camera_pose(position, center, np.array([0, 1, 0])))


def birdseye(center, min_bound, max_bound, yfov=np.pi / 3, aspect=16 / 9, znear=0.05):
    pose = notebook_node_pose(center, min_bound, max_bound)
    view = np.linalg.inv(pose)                                                              # pyrender: view matrix = inverse of the node's pose
    t = np.tan(yfov / 2)
    return Cam(tuple(view[:3].reshape(-1).tolist()), 1.0 / (aspect * t), 1.0 / t, 0.0, 0.0, znear)


def perspective_matrix(yfov, aspect, znear):
    """pyrender's PerspectiveCamera.get_projection_matrix with zfar = None"""
    t = np.tan(yfov / 2)
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[2, 2], P[2, 3], P[3, 2] = 1.0 / (aspect * t), 1.0 / t, -1.0, -2.0 * znear, -1.0
    return P


def window_by_matrices(points, view34, P, W, H):
    """GL's pipeline the long way: clip = P (V p); inside iff -w <= x, y, z <= w; window = (ndc + 1) size / 2.  -> (inside, x_w, y_w, w)"""
    V = np.vstack([np.asarray(view34, np.float64).reshape(3, 4), [0, 0, 0, 1]])
    hom = np.concatenate([points.astype(np.float64), np.ones((len(points), 1))], axis=1)
    clip = (P @ (V @ hom.T)).T
    w = clip[:, 3]
    with np.errstate(all="ignore"):
        inside = np.all((clip[:, :3] >= -w[:, None]) & (clip[:, :3] <= w[:, None]), axis=1)
        ndc = clip[:, :2] / w[:, None]
    return inside, (ndc[:, 0] + 1) * (W / 2), (ndc[:, 1] + 1) * (H / 2), w


# ------------------------------------------------------------------------------------------------------------------- the renderer
def project(points, cam, W, H):
    """-> (drawn, x_w, y_w, fp32 depth) per point, in the written order of include/f3r.h"""
    V = np.asarray(cam.view, dtype=np.float64).reshape(3, 4)
    p = points.astype(np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        e = [((V[r, 0] * x + V[r, 1] * y) + V[r, 2] * z) + V[r, 3] for r in range(3)]
        d = -e[2]
        px = np.float64(cam.sx) * e[0] + np.float64(cam.cx) * d
        py = np.float64(cam.sy) * e[1] + np.float64(cam.cy) * d
        df = d.astype(np.float32)
        drawn = (d >= cam.znear) & (np.abs(px) <= d) & (np.abs(py) <= d) & np.isfinite(df)
        xw = (px / d + 1.0) * (W * 0.5)
        yw = (py / d + 1.0) * (H * 0.5)
    return drawn, xw, yw, df


def splat(keys, points, n0, n1, cam, point_size):
    """points [n0, n1) into keys (H, W) uint64, window rows (row 0 at the bottom)"""
    H, W = keys.shape
    drawn, xw, yw, df = project(points[n0:n1], cam, W, H)
    idx = np.flatnonzero(drawn)
    if len(idx) == 0:
        return
    h = np.float64(point_size) * 0.5
    cx_, cy_ = np.arange(W) + 0.5, np.arange(H) + 0.5
    # the first pixel centre >= t: exactly the comparisons x_w - h <= i + 0.5 and i + 0.5 < x_w + h, by binary search over the centres
    i0, i1 = np.searchsorted(cx_, xw[idx] - h, "left"), np.searchsorted(cx_, xw[idx] + h, "left")
    j0, j1 = np.searchsorted(cy_, yw[idx] - h, "left"), np.searchsorted(cy_, yw[idx] + h, "left")
    key = (df[idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (idx + n0).astype(np.uint64)
    flat = keys.reshape(-1)
    for dj in range(int((j1 - j0).max(initial=0))):
        for di in range(int((i1 - i0).max(initial=0))):
            m = (j0 + dj < j1) & (i0 + di < i1)
            if m.any():
                np.minimum.at(flat, (j0[m] + dj) * W + (i0[m] + di), key[m])


def resolve(keys, colors, background=(255, 255, 255)):
    """-> (image (H, W, 3) uint8 with row 0 at the top, depth (H, W) fp32 with +inf where empty)"""
    k = keys[::-1]
    empty = k == EMPTY
    image = np.empty(k.shape + (3,), np.uint8)
    image[:] = np.asarray(background, np.uint8)
    image[~empty] = colors[(k[~empty] & np.uint64(0xffffffff)).astype(np.int64)]
    depth = (k >> np.uint64(32)).astype(np.uint32).view(np.float32).copy()
    depth[empty] = np.inf
    return image, depth


def render(points, colors, cam, W, H, point_size, background=(255, 255, 255), segments=None):
    """one (image, depth), or with segments (ascending end offsets) the list of them, frame i after segments <= i went in"""
    keys = np.full((H, W), EMPTY, dtype=np.uint64)
    out, start = [], 0
    for end in [len(points)] if segments is None else segments:
        splat(keys, points, start, end, cam, point_size)
        start = end
        out.append(resolve(keys, colors, background))
    return out[0] if segments is None else out


def center(points):
    return np.sum(points, axis=0, dtype=np.float64) / len(points)


def center_bound(points):
    """2 (M - 1) 2^-53 sum |p_i| / M per axis: two fp64 sums of the same fp32 values, each within (M - 1) 2^-53 sum |p_i| of the exact sum"""
    M = len(points)
    return 2 * (M - 1) * 2.0 ** -53 * np.sum(np.abs(points.astype(np.float64)), axis=0) / M


def cloud_camera(points):
    """the notebook's camera of a finite cloud, with the fp64 centre"""
    return birdseye(center(points), points.min(0), points.max(0))


# ------------------------------------------------------------------------------------------------------------------- the notebook's loop
def color_u8(img):
    """trunc((img + 1) * 127.5) in fp32, saturated, NaN -> 0 (the project's colour line)"""
    with np.errstate(all="ignore"):
        y = (img.astype(np.float32) + np.float32(1.0)) * np.float32(127.5)
    y = np.where(y > 0, np.minimum(y, np.float32(255.0)), np.float32(0.0))                 # NaN > 0 is false
    return y.astype(np.uint8)


def combine(preds, views, percentile, sample=0, pts_key="pts3d_in_other_view", conf_key="conf"):
    """-> (points, colors, end offsets); points None when nothing is kept"""
    pts, cols, ends, total = [], [], [], 0
    for pred, view in zip(preds, views):
        conf = np.asarray(pred[conf_key][sample], np.float32).reshape(-1)
        p = np.asarray(pred[pts_key][sample], np.float32).reshape(-1, 3)
        rgb = np.transpose(np.asarray(view["img"][sample], np.float32), (1, 2, 0)).reshape(-1, 3)
        with np.errstate(all="ignore"):
            mask = conf > np.percentile(conf, percentile)
        pts.append(p[mask])
        cols.append(color_u8(rgb[mask]))
        total += int(mask.sum())
        ends.append(total)
    if total == 0:
        return None, None, ends
    return np.concatenate(pts), np.concatenate(cols), ends
