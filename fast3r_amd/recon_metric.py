"""Reconstruction metrics on the GPU: `accuracy`, `completion`, `completion_ratio` (fast3r/eval/recon_metric.py:14-49) and the body
of `MultiViewDUSt3RLitModule.evaluate_reconstruction` (fast3r/models/multiview_dust3r_module.py:551-735).

The reference builds scipy cKDTrees on the CPU and estimates normals with Open3D; here the nearest-neighbour index, the exact 1-NN
and k-NN queries, the normals and the statistics are HIP kernels (fast3r_amd/csrc/f3r_recon.hip, see docs/rows_f.md).  What is
exact: 1-NN distances (fp64 of the fp32 coordinates, as cKDTree computes them on its float64 copies) and indices (ties to the smaller
index), means up to fp64 summation order, medians (np.median), the completion ratio.  What is restated: Open3D's normals (same
neighbour set and covariance, a different 3x3 eigen-solver: the sign is arbitrary and every metric takes |dot|).
"""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr, work_device


def _points(x, dev, what):
    """(n, 3) fp32 contiguous on `dev`.  fp64 inputs are rounded to fp32 coordinates (the reference's flow only holds fp32 values)."""
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    if t.ndim != 2 or t.shape[-1] != 3:
        raise ValueError(f"{what}: expected an (n, 3) point array, got shape {tuple(t.shape)}")
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _normals(x, dev):
    if x is None:
        return None
    t = torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x)
    return t.to(device=dev, dtype=torch.float64).reshape(-1, 3).contiguous()


def _device_of(*xs):
    for x in xs:
        if torch.is_tensor(x) and x.is_cuda:
            return x.device
    probe = xs[0] if torch.is_tensor(xs[0]) else torch.empty(0)
    return work_device(probe, "points")


class NNIndex:
    """Exact nearest-neighbour index over an (m, 3) fp32 device tensor (the kernels' grid; keeps `points` alive for the normals)."""

    def __init__(self, points):
        self.points = points
        self.m = points.shape[0]
        l = _lib.lib()
        nb = l.f3r_nn_index_bytes(self.m)
        self.buf = torch.empty((nb + 15) // 16 * 4, dtype=torch.float32, device=points.device)
        ws = _workspace(l.f3r_nn_workspace_bytes(self.m), points.device)
        with torch.cuda.device(points.device):
            check(l.f3r_nn_build(ptr(points) if self.m else None, self.m, ptr(self.buf), nb, ptr(ws), ws.numel(), stream_ptr()), "f3r_nn_build")

    def query(self, q):
        """(dist fp64 [n], idx int64 [n]) of the nearest indexed point of every row of q ((n, 3) fp32 on the same device)."""
        l = _lib.lib()
        n = q.shape[0]
        dist = torch.empty(n, dtype=torch.float64, device=q.device)
        idx = torch.empty(n, dtype=torch.int32, device=q.device)
        ws = _workspace(l.f3r_nn_workspace_bytes(n), q.device)
        with torch.cuda.device(q.device):
            check(l.f3r_nn_query(ptr(self.buf), ptr(q) if n else None, n, ptr(dist), ptr(idx), ptr(ws), ws.numel(), stream_ptr()), "f3r_nn_query")
        return dist, idx

    def knn(self, k=30, normals=True, neighbours=False):
        """Normals [m, 3] fp64 and / or the min(k, m) nearest indexed points of every indexed point ((idx int32, dist fp64) [m, k'])."""
        l = _lib.lib()
        kk = min(k, self.m)
        dev = self.points.device
        nrm = torch.empty((self.m, 3), dtype=torch.float64, device=dev) if normals else None
        ki = torch.empty((self.m, kk), dtype=torch.int32, device=dev) if neighbours else None
        kd = torch.empty((self.m, kk), dtype=torch.float64, device=dev) if neighbours else None
        if self.m:
            with torch.cuda.device(dev):
                check(l.f3r_estimate_normals(ptr(self.buf), ptr(self.points), kk, ptr(nrm), ptr(ki), ptr(kd), stream_ptr()), "f3r_estimate_normals")
        return nrm, ki, kd


def _workspace(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def nearest_neighbors(query, database):
    """Exact 1-NN of every query point in `database` (both (n, 3) device tensors): (dist fp64 [n], idx int64 [n]), as
    scipy.spatial.cKDTree(database).query(query) returns them (fp32 coordinates; ties to the smaller index).  NaN / inf coordinates
    raise ValueError, as in cKDTree."""
    dev = _device_of(database, query)
    db, q = _points(database, dev, "database"), _points(query, dev, "query")
    dist, idx = NNIndex(db).query(q)
    return dist, idx.long()


def estimate_normals(points, knn=30):
    """Open3D's PointCloud.estimate_normals() (KDTreeSearchParamKNN(knn), fast_normal_computation=True) on the GPU: (m, 3) fp64 unit
    normals with an arbitrary sign; (0, 0, 1) where fewer than 3 neighbours exist."""
    if not 1 <= knn <= 64:
        raise ValueError(f"estimate_normals: knn = {knn} outside 1..64")
    dev = _device_of(points)
    p = _points(points, dev, "points")
    return NNIndex(p).knn(knn)[0]


def _stats(dist, idx, nq, ndb, dist_th=0.0):
    m_db = 0 if ndb is None else ndb.shape[0]
    l = _lib.lib()
    n = dist.shape[0]
    if n == 0:
        nq = ndb = None  # empty queries: NaN statistics (empty tensors carry no device address)
    out = torch.empty(5, dtype=torch.float64, device=dist.device)
    ws = _workspace(l.f3r_recon_stats_workspace_bytes(n), dist.device)
    with torch.cuda.device(dist.device):
        check(l.f3r_recon_stats(ptr(dist), ptr(idx), ptr(nq), ptr(ndb), n, m_db, float(dist_th), ptr(out), ptr(ws), ws.numel(), stream_ptr()),
              "f3r_recon_stats")
    return out.cpu().numpy()


def _one_way(query, database, nq, ndb, dist_th=0.0):
    """query -> database 1-NN statistics; nq / ndb are the normals of query / database (or None)."""
    dev = _device_of(database, query, nq, ndb)
    db, q = _points(database, dev, "database"), _points(query, dev, "query")
    nq, ndb = _normals(nq, dev), _normals(ndb, dev)
    if nq is not None and ndb is not None and db.shape[0] == 0 and q.shape[0] > 0:
        # the reference indexes the database's normals with cKDTree's "no neighbour" index (= 0 = len)
        raise IndexError("index 0 is out of bounds for axis 0 with size 0")
    dist, idx = NNIndex(db).query(q)
    use_n = nq is not None and ndb is not None
    return _stats(dist, idx, nq if use_n else None, ndb if use_n else None, dist_th), use_n


def accuracy(gt_points, rec_points, gt_normals=None, rec_normals=None, device=None):
    """recon_metric.py:21-34: (mean, median) of the distance of every reconstructed point to the nearest GT point, plus (mean, median)
    of |n_gt[nn] . n_rec| when both normal sets are given.  numpy.float64 scalars.  `device` is ignored, as in the reference.
    Points may be numpy arrays or tensors (CPU ones are uploaded to the current GPU); fp64 coordinates are rounded to fp32."""
    s, use_n = _one_way(rec_points, gt_points, rec_normals, gt_normals)
    if use_n:
        return np.float64(s[0]), np.float64(s[1]), np.float64(s[2]), np.float64(s[3])
    return np.float64(s[0]), np.float64(s[1])


def completion(gt_points, rec_points, gt_normals=None, rec_normals=None, device=None):
    """recon_metric.py:37-49: accuracy with the roles swapped (GT points queried against the reconstruction)."""
    s, use_n = _one_way(gt_points, rec_points, gt_normals, rec_normals)
    if use_n:
        return np.float64(s[0]), np.float64(s[1]), np.float64(s[2]), np.float64(s[3])
    return np.float64(s[0]), np.float64(s[1])


def completion_ratio(gt_points, rec_points, dist_th=0.05):
    """recon_metric.py:14-18: fraction of GT points within dist_th of the reconstruction, as numpy.float32."""
    s, _ = _one_way(gt_points, rec_points, None, None, dist_th)
    return np.float32(s[4])


# ------------------------------------------------------------------------------------------------------------------------------
# evaluate_reconstruction (multiview_dust3r_module.py:551-735)

def _metrics_of_sample(pred_pts, gt_pts):
    """Both clouds on the GPU: normals of each (k = 30), then accuracy / completion with normals (:673-704)."""
    ip, ig = NNIndex(pred_pts), NNIndex(gt_pts)
    npred, ngt = ip.knn(30)[0], ig.knn(30)[0]
    if gt_pts.shape[0] == 0 and pred_pts.shape[0] > 0 or pred_pts.shape[0] == 0 and gt_pts.shape[0] > 0:
        raise IndexError("evaluate_reconstruction: one of the two clouds is empty")
    d, i = ig.query(pred_pts)
    acc = _stats(d, i, npred, ngt)
    d, i = ip.query(gt_pts)
    comp = _stats(d, i, ngt, npred)
    f = np.float64
    return {"accuracy": f(acc[0]), "accuracy_median": f(acc[1]), "completion": f(comp[0]), "completion_median": f(comp[1]),
            "nc1": f(acc[2]), "nc1_median": f(acc[3]), "nc2": f(comp[2]), "nc2_median": f(comp[3])}


def reconstruction_metrics(views, preds, min_conf_thr_percentile_for_local_alignment_and_icp=0,
                           min_conf_thr_percentile_for_metric_cacluation=0, use_pts3d_from_local_head=True):
    """The per-sample metric dicts of evaluate_reconstruction after the (optional) local-to-global alignment: a list of
    {scene_name: {accuracy, accuracy_median, completion, completion_median, nc1, nc1_median, nc2, nc2_median}}, one per sample."""
    pts_key = "pts3d_local_aligned_to_global" if use_pts3d_from_local_head else "pts3d_in_other_view"
    conf_key = "conf_local" if use_pts3d_from_local_head else "conf"
    B = len(views[0]["img"])
    V = len(preds)
    dev = work_device(preds[0][pts_key], "preds")
    # sample-major concatenation of every view (the reference's torch.cat order per sample, :640-646)
    order = [(i, j) for i in range(B) for j in range(V)]
    conf = torch.cat([preds[j][conf_key][i].reshape(-1).to(dev, torch.float32) for i, j in order]).contiguous()
    pred = torch.cat([preds[j][pts_key][i].reshape(-1, 3).to(dev, torch.float32) for i, j in order]).contiguous()
    gt = torch.cat([views[j]["pts3d"][i].reshape(-1, 3).to(dev, torch.float32) for i, j in order]).contiguous()
    valid = torch.cat([views[j]["valid_mask"][i].reshape(-1).to(dev) for i, j in order]).to(torch.uint8).contiguous()
    sizes = [preds[j][conf_key][i].numel() for i, j in order]
    seg = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    L = sum(sizes[:V])
    q_metric = float(min_conf_thr_percentile_for_metric_cacluation) / 100.0
    q_icp = float(min_conf_thr_percentile_for_local_alignment_and_icp) / 100.0
    l = _lib.lib()
    pred_out = torch.empty((B * L, 3), dtype=torch.float32, device=dev)
    gt_out = torch.empty((B * L, 3), dtype=torch.float32, device=dev)
    counts = torch.empty((2, B), dtype=torch.int32, device=dev)
    rts = torch.empty((B, 13), dtype=torch.float32, device=dev)
    ws = _workspace(l.f3r_recon_prepare_workspace_bytes(B, V, L), dev)
    with torch.cuda.device(dev):
        check(l.f3r_recon_prepare(ptr(conf), ptr(pred), ptr(gt), ptr(valid), ptr(seg), B, V, L, q_metric, q_icp, ptr(pred_out), ptr(gt_out),
                                  ptr(counts), ptr(rts), ptr(ws), ws.numel(), stream_ptr()), "f3r_recon_prepare")
    counts = counts.cpu().tolist()
    results = []
    with torch.cuda.device(dev):
        for i in range(B):
            scene_name = "/".join(views[i]["label"][0].split("/")[:-1]) if "label" in views[i] else "unknown"  # sic: sample index i (:566)
            pp = pred_out[i * L: i * L + counts[0][i]]
            gg = gt_out[i * L: i * L + counts[1][i]]
            results.append({scene_name: _metrics_of_sample(pp, gg)})
    return results
