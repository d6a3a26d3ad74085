"""A numpy restatement of the reference's mesh export, in this project's words: the notebook's three preparation lines
(`np.percentile`, `conf > thr`, the colour line) and `fast3r/dust3r/viz.py::pts3d_to_trimesh` / `cat_meshes`.  tools/make_golden_mesh.py
asserts that it reproduces the reference's own functions bit for bit on every case of tests/mesh_cases.py.  It also defines what has no
reference counterpart: `drop_unreferenced`, `double_sided=False`, `flip_axes` and the PLY bytes."""
import hashlib

import numpy as np


def threshold(conf, pct):
    """np.percentile(conf fp32, pct), method 'linear', spelt out: the virtual index in fp32, two order statistics, numpy's two-sided lerp"""
    c = np.sort(np.asarray(conf, np.float32).reshape(-1))   # NaNs last
    n = c.size
    if np.isnan(c[-1]):
        return c[-1]
    q = np.float32(pct) / np.float32(100)
    virtual = np.float32(n - 1) * q
    lo = int(np.floor(virtual))
    if virtual >= n - 1:      # numpy reads element -1 twice and keeps the weight virtual - (-1)
        a = b = c[-1]
        g = np.float32(virtual - np.float32(-1))
    else:
        a, b = c[lo], c[lo + 1]
        g = np.float32(virtual - np.float32(lo))
    with np.errstate(invalid="ignore"):
        d = np.float32(b - a)
        if g >= 0.5:
            return np.float32(b - np.float32(d * np.float32(np.float32(1) - g)))
        return np.float32(a + np.float32(d * g))


def colors_u8(img_chw):
    """(3, H, W) fp32 in [-1, 1] -> (H, W, 3) uint8: an fp32 add, an fp32 multiply, truncation"""
    x = np.asarray(img_chw, np.float32).transpose(1, 2, 0)
    return np.clip((x + np.float32(1)) * np.float32(127.5), 0, 255).astype(np.uint8)


def view_mesh(img_u8, pts, valid, double_sided=True):
    """one view: (vertices (H W, 3), faces (F, 3) int64 local indices, face_colors (F, 3) uint8, kept A, kept B)"""
    H, W = pts.shape[:2]
    v = np.ones((H, W), bool) if valid is None else np.asarray(valid, bool).reshape(H, W)
    tl = (np.arange(H)[:, None] * W + np.arange(W)[None, :])[:H - 1, :W - 1]
    keep_a = v[:-1, :-1] & v[:-1, 1:] & v[1:, :-1]
    keep_b = v[:-1, 1:] & v[1:, :-1] & v[1:, 1:]
    ia, ib = tl[keep_a].astype(np.int64), tl[keep_b].astype(np.int64)   # boolean indexing keeps the quad order
    a = np.stack([ia, ia + 1, ia + W], axis=1).reshape(-1, 3)
    b = np.stack([ib + 1, ib + W, ib + W + 1], axis=1).reshape(-1, 3)
    flat = img_u8.reshape(-1, 3)
    ca, cb = flat[ia], flat[ib + W + 1]
    if double_sided:
        faces, cols = [a, a[:, ::-1], b, b[:, ::-1]], [ca, ca, cb, cb]
    else:
        faces, cols = [a, b], [ca, cb]
    return pts.reshape(-1, 3), np.concatenate(faces, axis=0), np.concatenate(cols, axis=0), len(ia), len(ib)


def build(views, pct, masks=None, *, double_sided=True, drop_unreferenced=False, flip_axes=False):
    """views: list of (img (3, H, W) fp32, pts (H, W, 3) fp32, conf (H, W) fp32); pct None: validity is the mask alone.
    -> dict(vertices, faces int64, face_colors, thresholds fp32 (V,), faces_per_view, vertices_per_view)"""
    vs, fs, cs, thr, nf, nv = [], [], [], [], [], []
    base = 0
    for i, (img, pts, conf) in enumerate(views):
        valid = None
        if pct is not None:
            t = threshold(conf, pct)
            thr.append(t)
            with np.errstate(invalid="ignore"):
                valid = conf > t
        if masks is not None:
            valid = masks[i] if valid is None else valid & np.asarray(masks[i], bool)
        v, f, c, _, _ = view_mesh(colors_u8(img), pts, valid, double_sided)
        if drop_unreferenced:
            used = np.unique(f)
            remap = np.full(len(v), -1, np.int64)
            remap[used] = np.arange(len(used))
            v, f = v[used], remap[f]
        vs.append(v)
        fs.append(f + base)
        cs.append(c)
        nf.append(len(f))
        nv.append(len(v))
        base += len(v)
    vertices = np.concatenate(vs, axis=0).astype(np.float32)
    if flip_axes:
        vertices = np.stack([vertices[:, 0], vertices[:, 2], -vertices[:, 1]], axis=1)
    return dict(vertices=np.ascontiguousarray(vertices), faces=np.concatenate(fs, axis=0).astype(np.int64).reshape(-1, 3),
                face_colors=np.concatenate(cs, axis=0).astype(np.uint8).reshape(-1, 3), thresholds=np.asarray(thr, np.float32),
                faces_per_view=np.asarray(nf, np.int64), vertices_per_view=np.asarray(nv, np.int64))


def ply_bytes(vertices, faces, face_colors):
    """the mesh PLY of fast3r_amd/mesh.py: its header, 12-byte vertex records, 16-byte face records"""
    nv, nf = len(vertices), len(faces)
    head = ("ply\nformat binary_little_endian 1.0\n"
            f"element vertex {nv}\nproperty float x\nproperty float y\nproperty float z\n"
            f"element face {nf}\nproperty list uchar int vertex_indices\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "end_header\n").encode("ascii")
    rec = np.zeros(nf, dtype=[("n", "u1"), ("idx", "<i4", 3), ("rgb", "u1", 3)])
    rec["n"] = 3
    rec["idx"] = np.asarray(faces).reshape(-1, 3)
    rec["rgb"] = np.asarray(face_colors, np.uint8).reshape(-1, 3)
    assert rec.dtype.itemsize == 16
    return head + np.asarray(vertices, "<f4").tobytes() + rec.tobytes()


def digest(a):
    """None, or (length, SHA-256) of bytes / of an array's bytes"""
    if a is None:
        return None
    b = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
    return (len(b), hashlib.sha256(b).hexdigest())
