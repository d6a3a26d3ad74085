"""TEST INFRASTRUCTURE ONLY -- the CPU side of the reconstruction metrics (fast3r_amd/recon_metric.py):

* `accuracy`, `completion`, `completion_ratio`: the reference's metric functions (fast3r/eval/recon_metric.py:14-49) restated on scipy's
  cKDTree -- pinned bit for bit against the live reference by tests/test_recon_metric.py;
* `open3d`: a stand-in module for what evaluate_reconstruction uses of Open3D (multiview_dust3r_module.py:668-690): PointCloud with
  `points` / `colors` / `normals` and `estimate_normals()` restating Open3D's defaults (KNN 30, fast_normal_computation): the k nearest
  points by (distance, index), one-pass cumulant covariance E[x x^T] - mu mu^T in fp64, eigenvector of the smallest eigenvalue
  (numpy.linalg.eigh); (0, 0, 1) below 3 neighbours;
* `roma`: a stand-in whose `rigid_points_registration` honours `weights` (Umeyama in fp64), which oracle/roma_stub.py does not.

tools/make_golden_recon.py runs the reference's own evaluate_reconstruction around these two stand-ins.  Pure numpy / scipy / torch.
"""
import types

import numpy as np
import torch
from scipy.spatial import cKDTree

KNN_MARGIN = 8  # extra neighbours fetched before the (distance, index) re-sort, so that ties at the k-th distance resolve by index
WORKERS = 16  # cKDTree query threads (the reference asks for 24)


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    distances, _ = cKDTree(rec_points).query(gt_points, workers=WORKERS)
    return np.mean((distances < dist_th).astype(np.float32))


def accuracy(gt_points, rec_points, gt_normals=None, rec_normals=None, device=None):
    distances, idx = cKDTree(gt_points).query(rec_points, workers=WORKERS)
    acc, acc_median = np.mean(distances), np.median(distances)
    if gt_normals is not None and rec_normals is not None:
        normal_dot = np.abs(np.sum(gt_normals[idx] * rec_normals, axis=-1))
        return acc, acc_median, np.mean(normal_dot), np.median(normal_dot)
    return acc, acc_median


def completion(gt_points, rec_points, gt_normals=None, rec_normals=None, device=None):
    distances, idx = cKDTree(rec_points).query(gt_points, workers=WORKERS)
    comp, comp_median = np.mean(distances), np.median(distances)
    if gt_normals is not None and rec_normals is not None:
        normal_dot = np.abs(np.sum(gt_normals * rec_normals[idx], axis=-1))
        return comp, comp_median, np.mean(normal_dot), np.median(normal_dot)
    return comp, comp_median


def knn_sorted(points, k=30):
    """(idx [m, k'], dist [m, k']) of the k' = min(k, m) nearest points of every point (itself included) in (distance, index) order."""
    pts = np.asarray(points, dtype=np.float64)
    m = len(pts)
    kk = min(k, m)
    kq = min(kk + KNN_MARGIN, m)
    d, i = cKDTree(pts).query(pts, k=kq, workers=WORKERS)
    d, i = d.reshape(m, kq), i.reshape(m, kq)
    order = np.lexsort((i, d), axis=-1)[:, :kk]
    return np.take_along_axis(i, order, -1), np.take_along_axis(d, order, -1)


def normals_and_eigenvalues(points, k=30):
    """Restated Open3D normals [m, 3] and the covariance eigenvalues [m, 3] (ascending)."""
    pts = np.asarray(points, dtype=np.float64)
    m = len(pts)
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (m, 1))
    ev = np.zeros((m, 3))
    if m < 3 or k < 3:
        return nrm, ev
    idx, _ = knn_sorted(pts, k)
    for c0 in range(0, m, 100000):  # in chunks: the neighbour coordinates of a chunk are [chunk][k][3] fp64
        sl = slice(c0, min(c0 + 100000, m))
        nrm[sl], ev[sl] = _normals_of(pts, idx[sl])
    return nrm, ev


def _normals_of(pts, idx):
    m, kk = idx.shape
    nrm = np.tile(np.array([0.0, 0.0, 1.0]), (m, 1))
    P = pts[idx]
    c = np.zeros((m, 9))
    for s in range(kk):  # one neighbour at a time, in (distance, index) order
        x, y, z = P[:, s, 0], P[:, s, 1], P[:, s, 2]
        c[:, 0] += x
        c[:, 1] += y
        c[:, 2] += z
        c[:, 3] += x * x
        c[:, 4] += x * y
        c[:, 5] += x * z
        c[:, 6] += y * y
        c[:, 7] += y * z
        c[:, 8] += z * z
    c /= float(kk)
    cov = np.empty((m, 3, 3))
    cov[:, 0, 0] = c[:, 3] - c[:, 0] * c[:, 0]
    cov[:, 0, 1] = cov[:, 1, 0] = c[:, 4] - c[:, 0] * c[:, 1]
    cov[:, 0, 2] = cov[:, 2, 0] = c[:, 5] - c[:, 0] * c[:, 2]
    cov[:, 1, 1] = c[:, 6] - c[:, 1] * c[:, 1]
    cov[:, 1, 2] = cov[:, 2, 1] = c[:, 7] - c[:, 1] * c[:, 2]
    cov[:, 2, 2] = c[:, 8] - c[:, 2] * c[:, 2]
    w, v = np.linalg.eigh(cov)
    n = v[:, :, 0]
    norm = np.linalg.norm(n, axis=-1)
    ok = norm > 0
    nrm[ok] = n[ok] / norm[ok, None]
    return nrm, w


def estimate_normals(points, k=30):
    return normals_and_eigenvalues(points, k)[0]


# ---- the open3d stand-in ------------------------------------------------------------------------------------------------------
class _PointCloud:
    def __init__(self):
        self.points = np.zeros((0, 3))
        self.colors = np.zeros((0, 3))
        self.normals = np.zeros((0, 3))

    def estimate_normals(self, *a, **k):
        self.normals = estimate_normals(np.asarray(self.points), 30)


open3d = types.ModuleType("open3d")
open3d.geometry = types.SimpleNamespace(PointCloud=_PointCloud)
open3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a, dtype=np.float64))


# ---- the roma stand-in ---------------------------------------------------------------------------------------------------------
def rigid_points_registration(x, y, weights=None, compute_scaling=False):
    """Weighted Umeyama in fp64: argmin sum_i w_i |s R x_i + t - y_i|^2 (roma's contract); results in the dtype of x."""
    X, Y = x.double(), y.double()
    w = torch.ones(X.shape[0], dtype=torch.float64) if weights is None else weights.double()
    wn = w / w.sum()
    mx, my = (wn[:, None] * X).sum(0), (wn[:, None] * Y).sum(0)
    Xc, Yc = X - mx, Y - my
    M = (wn[:, None] * Yc).T @ Xc
    U, S, Vt = torch.linalg.svd(M)
    d = torch.sign(torch.det(U) * torch.det(Vt))
    D = torch.diag(torch.stack([torch.ones((), dtype=torch.float64), torch.ones((), dtype=torch.float64), d]))
    R = U @ D @ Vt
    if not compute_scaling:
        return R.to(x.dtype), (my - R @ mx).to(x.dtype)
    s = (S * torch.diagonal(D)).sum() / (wn * (Xc * Xc).sum(1)).sum()
    t = my - s * (R @ mx)
    return R.to(x.dtype), t.to(x.dtype), s.to(x.dtype)


roma = types.ModuleType("roma")
roma.rigid_points_registration = rigid_points_registration


# ---- inputs rebuilt from recipes (tools/make_golden_recon.py stores recipes, not clouds) ------------------------------------------
def make_cloud(kind, n, seed):
    """(n, 3) float32 numpy cloud of a named distribution, from a CPU torch.Generator."""
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":
        p = torch.rand((n, 3), generator=g)
    elif kind == "surface":  # a pointmap-like height field with noise
        uv = torch.rand((n, 2), generator=g) * 2 - 1
        z = 2.0 + 0.3 * torch.sin(3 * uv[:, 0]) * torch.cos(2 * uv[:, 1]) + 0.002 * torch.randn(n, generator=g)
        p = torch.stack([uv[:, 0] * z, uv[:, 1] * z, z], 1)
    elif kind == "outliers":  # two clusters + 0.1 % far outliers at 1e4 x the scene scale
        c = torch.randint(0, 2, (n,), generator=g).float()
        p = torch.randn((n, 3), generator=g) * 0.05 + torch.stack([c * 2.0, c * 0.5, 1.0 + 0 * c], 1)
        k = max(1, n // 1000)
        sel = torch.randperm(n, generator=g)[:k]
        p[sel] = (torch.rand((k, 3), generator=g) * 2 - 1) * 2e4
    elif kind == "duplicates":  # exact duplicates of a coarse lattice
        p = torch.randint(0, 12, (n, 3), generator=g).float() * 0.1
    elif kind == "outside":  # a cloud wholly outside the unit cube (paired with "uniform" databases)
        p = torch.rand((n, 3), generator=g) * 0.5 + torch.tensor([3.0, -2.0, 1.5])
    else:
        raise ValueError(kind)
    return p.float().numpy()


def unit_normals(n, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((n, 3), generator=g, dtype=torch.float64)
    return (v / v.norm(dim=1, keepdim=True)).numpy()


def make_eval_case(B, sizes, seed, holes=True):
    """views / preds (CPU tensors) for evaluate_reconstruction: per view (H, W) of `sizes`, a GT height-field pointmap, a prediction
    that is a similarity transform of it plus noise (global and local heads), confidences, valid_mask holes, labels per view."""
    g = torch.Generator().manual_seed(seed)
    views, preds = [], []
    ang = float(torch.rand((), generator=g)) * 1.0
    c, s_ = np.cos(ang), np.sin(ang)
    R = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    scale, t = 0.7, torch.tensor([0.2, -0.1, 0.3])
    for j, (H, W) in enumerate(sizes):
        yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
        gts, prs, loc, cfs, cls, vms = [], [], [], [], [], []
        for i in range(B):
            z = 2.0 + 0.2 * j + 0.3 * torch.sin(3 * xx + i) * torch.cos(2 * yy) + 0.01 * torch.randn((H, W), generator=g)
            gt = torch.stack([xx * z, yy * z, z], -1)
            pr = scale * (gt @ R.T) + t + 0.01 * torch.randn((H, W, 3), generator=g)
            lo = pr * 1.3 + 0.05 + 0.005 * torch.randn((H, W, 3), generator=g)  # the local head: another similarity of the same points
            gts.append(gt)
            prs.append(pr)
            loc.append(lo)
            cfs.append(1.0 + torch.rand((H, W), generator=g) * 5)
            cls.append(1.0 + torch.rand((H, W), generator=g) * 5)
            vm = torch.rand((H, W), generator=g) > (0.15 if holes else -1.0)
            vms.append(vm)
        views.append({"img": torch.rand((B, 3, H, W), generator=g) * 2 - 1, "pts3d": torch.stack(gts).float(), "valid_mask": torch.stack(vms),
                      "label": [f"scene{seed}/view{j}/img{i:03d}.png" for i in range(B)]})
        preds.append({"pts3d_in_other_view": torch.stack(prs).float(), "conf": torch.stack(cfs).float(),
                      "pts3d_local": torch.stack(loc).float(), "conf_local": torch.stack(cls).float()})
    return views, preds


# ---- the bytes of one nearest-neighbour index (csrc/f3r_nn.h), restated: header fields, fp64 cell keys, the stable order ------------
NN_HDR_BYTES = 256


def nn_header(raw):
    """the NNHeader at the start of `raw` (uint8): two 88-byte grids {lo[3], hi[3], h, inv_h: fp64; dims[3]: int32; base: uint32; ncells:
    int64}, then ngrid, dense: int32 (byte 176), m, ncells, occupied: int64, key_bits: int32"""
    grids = []
    for k in range(2):
        b = raw[88 * k:88 * (k + 1)]
        f = b[:64].view(np.float64)
        grids.append({"lo": f[0:3].copy(), "hi": f[3:6].copy(), "h": float(f[6]), "inv_h": float(f[7]), "dims": b[64:76].view(np.int32).astype(np.int64),
                      "base": int(b[76:80].view(np.uint32)[0]), "ncells": int(b[80:88].view(np.int64)[0])})
    ngrid, dense = (int(v) for v in raw[176:184].view(np.int32))
    m, ncells, occupied = (int(v) for v in raw[184:208].view(np.int64))
    return {"g": grids, "ngrid": ngrid, "dense": dense, "m": m, "ncells": ncells, "occupied": occupied, "key_bits": int(raw[208:212].view(np.int32)[0])}


def nn_cell_keys(H, pts):
    """point_key of every fp32 point in fp64, one operation at a time: cell_coord's clamp, the grid choice, the grids' base"""
    p = pts.astype(np.float64)

    def keys_of(g):
        c = []
        for a in range(3):
            f = np.floor((p[:, a] - g["lo"][a]) * g["inv_h"])
            c.append(np.where(f >= 0.0, np.minimum(f, float(g["dims"][a] - 1)), 0.0).astype(np.int64))
        return g["base"] + (c[2] * g["dims"][1] + c[1]) * g["dims"][0] + c[0]

    k = keys_of(H["g"][0])
    if H["ngrid"] == 2:
        g = H["g"][0]
        inside = np.all((p >= g["lo"]) & (p <= g["hi"]), axis=1)
        k = np.where(inside, k, keys_of(H["g"][1]))
    return k


def check_nn_index(raw, pts, stored_keys=True):
    """asserts that the index in `raw` (uint8, from its header on) over the fp32 points `pts` holds what its own header implies: records
    = the points in the stable order of their cell keys with their original indices, the sorted keys after them (f3r_nn_build; the
    per-view indexes of f3r_match_index leave that region unused), and with `dense` the first sorted position of every cell.  -> header"""
    H = nn_header(raw)
    m = H["m"]
    assert m == len(pts) and H["ngrid"] in (1, 2) and H["ncells"] == H["g"][0]["ncells"] + (H["g"][1]["ncells"] if H["ngrid"] == 2 else 0)
    assert all(int(np.prod(g["dims"])) == g["ncells"] for g in H["g"][:H["ngrid"]]) and H["g"][0]["base"] == 0
    keys = nn_cell_keys(H, pts)
    assert m == 0 or (keys.min() >= 0 and keys.max() < H["ncells"])
    order = np.argsort(keys, kind="stable")
    want = keys[order]
    recs = raw[NN_HDR_BYTES:NN_HDR_BYTES + 16 * m].view(np.uint32).reshape(m, 4)
    if stored_keys:
        assert np.array_equal(raw[NN_HDR_BYTES + 16 * m:NN_HDR_BYTES + 20 * m].view(np.uint32), want), "sorted keys"
    assert np.array_equal(recs[:, 3], order), "record order"
    assert np.array_equal(recs[:, :3], np.ascontiguousarray(pts[order]).view(np.uint32)), "record coordinates"
    if H["dense"]:
        table = raw[NN_HDR_BYTES + 20 * m:NN_HDR_BYTES + 20 * m + 4 * (H["ncells"] + 1)].view(np.uint32)
        assert np.array_equal(table, np.searchsorted(want, np.arange(H["ncells"] + 1), "left")), "cell starts"
    return H
