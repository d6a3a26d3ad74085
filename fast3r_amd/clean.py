"""Cross-view occlusion filter for confidences on the GPU: the reference's `BasePCOptimizer.clean_pointcloud`
(fast3r/dust3r/cloud_opt/base_opt.py:279-317).  Every view's points are projected into the other cameras; a point that lies in front of a
camera's depth map and is less confident than the pixel it lands on -- a floater -- has its confidence clipped to `max_bad_conf`.

The kernel (fast3r_amd/csrc/f3r_clean.hip, include/f3r.h "cross-view occlusion filter", docs/rows_f.md) runs one launch per target view in
ascending order: view i is tested against the working copy, cleaned already for j < i and still the input for j > i, as the reference's loop
does, so the result depends on the order of the views exactly as the reference's.

* `clean_confidences(pts3d, conf, depthmaps, im_poses, focals, pp)`: the five inputs of the reference method -> the cleaned confidences.
* `clean_pointcloud(preds, ...)` -> `CleanedCloud`: a forward pass with its poses and focals, the depth from `pts3d_local[..., 2]`.
* `pairs=`: test view i against its neighbours in a scene graph only (a pair connects both ways); `frame="camera"`: the points are given in
  their own camera's frame and the kernel applies the pose.  Both are additions to the reference.
"""
import dataclasses

import numpy as np
import torch

from . import post_ops
from ._lib import work_device
from .matching import _pair_list, _preds_of

HEADS = {"local": ("pts3d_local", "conf_local", "camera"), "global": ("pts3d_in_other_view", "conf", "world")}


# ------------------------------------------------------------------------------------------------------------------- neighbour lists
def neighbour_lists(pairs, n_views):
    """The CSR of the views each view is tested against: (starts: N + 1 Python ints, nbr: int32 numpy).  pairs: 'complete' (every other view),
    any other graph string of scene_graph_pairs, or explicit rows (i, j).  A pair connects both ways; a view is never its own neighbour;
    every list ascends and holds a view once."""
    N = int(n_views)
    if isinstance(pairs, str) and pairs == "complete":
        nbr = np.asarray([j for i in range(N) for j in range(N) if j != i], dtype=np.int32)
        return [i * (N - 1) for i in range(N + 1)], nbr
    try:
        rows = _pair_list(pairs, N)
    except ValueError as e:
        raise ValueError(str(e).replace("match_views", "clean_confidences")) from None
    sets = [set() for _ in range(N)]
    for i, j in rows.tolist():
        if i != j:
            sets[i].add(j)
            sets[j].add(i)
    starts, nbr = [0], []
    for s in sets:
        nbr += sorted(s)
        starts.append(len(nbr))
    return starts, np.asarray(nbr, dtype=np.int32)


# ------------------------------------------------------------------------------------------------------------------- arguments
def _tol_arg(tol, who):
    tol = float(tol)
    if not 0.0 <= tol < 1.0:  # NaN fails
        raise ValueError(f"{who}: tol must lie in [0, 1), got {tol}")
    return tol


def _max_bad_arg(max_bad_conf, who):
    m = float(max_bad_conf)
    if m != m:
        raise ValueError(f"{who}: max_bad_conf is NaN")
    return m


def _views_of(x, n, what):
    """a list of per-view tensors or arrays, or a stacked one -> a list of torch tensors (numpy is wrapped, nothing is copied yet)"""
    if torch.is_tensor(x) or isinstance(x, np.ndarray):
        x = list(x)
    x = [torch.as_tensor(t) for t in x]
    if n is not None and len(x) != n:
        raise ValueError(f"clean_confidences: {what} has {len(x)} entries for {n} views")
    return x


def _intrinsics(focals, pp, shapes):
    """(N, 4) fp32 on the host: fx, fy, cx, cy.  focals per view: a scalar or (fx, fy); pp per view (cx, cy), default (W / 2, H / 2)"""
    N = len(shapes)
    f = torch.as_tensor(np.asarray([torch.as_tensor(v).detach().cpu().numpy() for v in focals]) if isinstance(focals, (list, tuple)) else focals)
    f = f.detach().cpu().to(torch.float32)
    if f.dim() == 2 and f.shape[1] == 1:
        f = f[:, 0]
    if f.shape[0] != N or f.dim() not in (1, 2) or (f.dim() == 2 and f.shape[1] != 2):
        raise ValueError(f"clean_confidences: focals must be one scalar or (fx, fy) per view ({N} views), got shape {tuple(f.shape)}")
    if f.dim() == 1:
        f = torch.stack([f, f], dim=1)
    if pp is None:
        c = torch.tensor([[W / 2, H / 2] for H, W in shapes], dtype=torch.float32)
    else:
        c = torch.as_tensor(np.asarray([torch.as_tensor(v).detach().cpu().numpy() for v in pp]) if isinstance(pp, (list, tuple)) else pp)
        c = c.detach().cpu().to(torch.float32)
        if tuple(c.shape) != (N, 2):
            raise ValueError(f"clean_confidences: pp must be (cx, cy) per view ({N} views), got shape {tuple(c.shape)}")
    return torch.cat([f, c], dim=1).contiguous()


def clean_confidences(pts3d, conf, depthmaps, im_poses, focals, pp=None, *, tol=0.001, max_bad_conf=0, pairs="complete", frame="world",
                      return_lowered=False):
    """`BasePCOptimizer.clean_pointcloud` on its five inputs.  Per view i, as lists of per-view tensors or stacked ones, numpy or torch: pts3d
    (H_i, W_i, 3) or (H_i W_i, 3) points -- in the world frame, or with frame="camera" in camera i's own (the kernel applies the pose) --,
    conf and depthmaps (H_i, W_i), im_poses (4, 4) camera-to-world, focals a scalar or (fx, fy); pp (cx, cy), default (W / 2, H / 2), the
    convention of estimate_focal.  Views may differ in size.  pairs: 'complete', a graph string of scene_graph_pairs or explicit rows (i, j): view
    i is tested against its neighbours only, in both directions of a pair; the ascending order of i stays.  -> the cleaned confidences, new
    tensors shaped and placed like `conf` (a list for a list, stacked for a stacked tensor); with return_lowered also the per-view counts of
    lowered pixels (int64 numpy).  Argument errors are ValueErrors raised before any device work."""
    who = "clean_confidences"
    tol, max_bad = _tol_arg(tol, who), _max_bad_arg(max_bad_conf, who)
    post_ops.clean_frame_id(frame)
    stacked = torch.is_tensor(conf) or isinstance(conf, np.ndarray)
    conf_l = _views_of(conf, None, "conf")
    N = len(conf_l)
    if N < 1:
        raise ValueError(f"{who}: need at least one view")
    pts_l, depth_l, pose_l = _views_of(pts3d, N, "pts3d"), _views_of(depthmaps, N, "depthmaps"), _views_of(im_poses, N, "im_poses")
    shapes = []
    for i in range(N):
        c = conf_l[i]
        if c.dim() != 2 or c.numel() < 1:
            raise ValueError(f"{who}: conf of view {i} must be (H, W), got {tuple(c.shape)}")
        H, W = c.shape
        if tuple(depth_l[i].shape) != (H, W):
            raise ValueError(f"{who}: depthmap of view {i} is {tuple(depth_l[i].shape)}, its confidence {(H, W)}")
        if tuple(pts_l[i].shape) not in ((H, W, 3), (H * W, 3)):
            raise ValueError(f"{who}: pts3d of view {i} is {tuple(pts_l[i].shape)}; need {(H, W, 3)} or {(H * W, 3)}")
        if tuple(pose_l[i].shape) != (4, 4):
            raise ValueError(f"{who}: im_poses of view {i} is {tuple(pose_l[i].shape)}; need (4, 4)")
        shapes.append((H, W))
    intr = _intrinsics(focals, pp, shapes)
    starts, nbr = neighbour_lists(pairs, N)
    home = conf_l[0].device
    dev = work_device(conf_l[0], "conf")
    f32 = torch.float32
    up = lambda ts, shape: torch.cat([t.to(dev, f32).reshape(shape) for t in ts]).contiguous()  # noqa: E731
    out, lowered = post_ops.clean_confidence(up(pts_l, (-1, 3)), up(conf_l, (-1,)), up(depth_l, (-1,)),
                                             torch.stack([t.to(dev, f32) for t in pose_l]).contiguous(), intr.to(dev), shapes, starts, nbr,
                                             tol=tol, max_bad_conf=max_bad, frame=frame)
    res, off = [], 0
    for H, W in shapes:
        res.append(out[off:off + H * W].view(H, W).to(home))
        off += H * W
    if stacked:
        res = torch.stack(res)
    return (res, lowered) if return_lowered else res


# ------------------------------------------------------------------------------------------------------------------- forward passes
@dataclasses.dataclass
class CleanedCloud:
    """conf: per view the cleaned (H, W) confidence; kept: bool masks, true where the value did not change (they fit
    assemble_scene(not_sky=...) and build_mesh(valid=...)); n_lowered: int64 numpy per view; preds: shallow copies of the pred dicts with the
    one confidence entry replaced, for every consumer of preds."""
    conf: list
    kept: list
    n_lowered: np.ndarray
    preds: list


def _sample_map(t, sample, trailing, what):
    """(B, H, W, ...) -> (H, W, ...) of one sample; a map without the batch dimension passes"""
    if t.dim() == 3 + trailing:
        if not 0 <= sample < t.shape[0]:
            raise ValueError(f"clean_pointcloud: sample = {sample} outside the batch of {t.shape[0]} ({what})")
        t = t[sample]
    if t.dim() != 2 + trailing or (trailing and t.shape[-1] != 3):
        raise ValueError(f"clean_pointcloud: {what} must be (H, W{', 3' if trailing else ''}) with or without a batch dimension, got {tuple(t.shape)}")
    return t


def clean_pointcloud(output_or_preds, views=None, *, poses=None, focals=None, head="local", tol=0.001, max_bad_conf=0, pairs="complete", sample=0):
    """`clean_pointcloud` on a forward pass: output_or_preds is the output dict of inference() or its preds list.  head="local": the points are
    `pts3d_local` in their own cameras (frame="camera"), the confidence `conf_local`; head="global": `pts3d_in_other_view` in view 0's frame
    with `conf`.  The depth of view j is `pts3d_local[..., 2]`.  poses (N, 4, 4) camera-to-world relative to view 0 and focals (N,) default to
    estimate_camera_poses_device(preds) for that sample; the principal point is the image centre.  -> CleanedCloud."""
    who = "clean_pointcloud"
    if head not in HEADS:
        raise ValueError(f"{who}: head must be 'local' or 'global', got {head!r}")
    pts_key, conf_key, frame = HEADS[head]
    tol, max_bad = _tol_arg(tol, who), _max_bad_arg(max_bad_conf, who)
    try:
        preds, views = _preds_of(output_or_preds, views)
    except ValueError as e:
        raise ValueError(str(e).replace("match_views", who)) from None
    N = len(preds)
    if N < 1:
        raise ValueError(f"{who}: need at least one view")
    sample = int(sample)
    pts_l, conf_l, depth_l = [], [], []
    for v, p in enumerate(preds):
        for key in {pts_key, conf_key, "pts3d_local"}:
            if key not in p:
                raise KeyError(f"{who}: preds[{v}] has no '{key}'")
        x = _sample_map(p[pts_key], sample, 1, f"preds[{v}]['{pts_key}']")
        c = _sample_map(p[conf_key], sample, 0, f"preds[{v}]['{conf_key}']")
        d = _sample_map(p["pts3d_local"], sample, 1, f"preds[{v}]['pts3d_local']")[..., 2]
        if c.shape != x.shape[:2] or d.shape != c.shape:
            raise ValueError(f"{who}: view {v}: points {tuple(x.shape)}, confidence {tuple(c.shape)} and depth {tuple(d.shape)} differ in size")
        pts_l.append(x)
        conf_l.append(c)
        depth_l.append(d)
    neighbour_lists(pairs, N)  # refuses a bad graph before the solve below
    if (poses is None) != (focals is None):
        raise ValueError(f"{who}: give poses and focals together, or neither")
    if poses is None:
        from .pose import estimate_camera_poses_device
        all_poses, all_focals = estimate_camera_poses_device(preds)
        if not 0 <= sample < all_poses.shape[0]:
            raise ValueError(f"{who}: sample = {sample} outside the batch of {all_poses.shape[0]}")
        poses, focals = all_poses[sample], all_focals[sample]
    conf, lowered = clean_confidences(pts_l, conf_l, depth_l, poses, focals, tol=tol, max_bad_conf=max_bad, pairs=pairs, frame=frame,
                                      return_lowered=True)
    kept, new_preds = [], []
    for v, p in enumerate(preds):
        old = conf_l[v]
        new = conf[v].to(old.dtype)
        kept.append((new == old) | (new.isnan() & old.isnan()))
        entry = p[conf_key].clone()
        if entry.dim() == 3:
            entry[sample] = new
        else:
            entry = new
        q = dict(p)
        q[conf_key] = entry
        new_preds.append(q)
    return CleanedCloud(conf=conf, kept=kept, n_lowered=lowered, preds=new_preds)
