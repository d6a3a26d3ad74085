"""Global alignment on the GPU: the reference's `global_aligner(...)` -> `PointCloudOptimizer` -> `compute_global_alignment(niter=300)`
(fast3r/dust3r/cloud_opt/{__init__,base_opt,optimizer,commons}.py).  Pairwise pointmaps -- edge (i, j) holds view i's and view j's pointmap
in view i's frame -- are fused into one set of poses, focals and depth maps by minimising, with Adam, the confidence-weighted distance
between every pairwise pointmap, moved by its own similarity, and the world points of its view.

The loss and all its gradients are one kernel call (fast3r_amd/csrc/f3r_galign.hip, include/f3r.h "global alignment", docs/rows_f.md) at the
level of matrices; the chain from the raw parameters (quaternions, `signed_expm1`, log scales, log focals) to those few N- and E-sized
matrices is ordinary torch autograd around it.

* `alignment_loss(im_poses, focals, pp, log_depths, pw_poses, adaptors, observations, dist)`: the autograd function.
* `PointCloudOptimizer`, `global_aligner`, `GlobalAlignerMode`: the reference's names and meaning.  `compute_global_alignment` is the
  reference's loop without its per-iteration read-back of the loss.
* `pairs_from_passes(outputs, anchors)`: K forward passes with different anchor views -> the reference's (view1, view2, pred1, pred2);
  `compute_global_alignment(init="passes")` starts from pass 0.  Both are additions to the reference.
Out of scope: `init="mst"` / `"known_poses"`, `ModularPointCloudOptimizer`, `PairViewer`, `show()`, `mask_sky()`.
"""
import copy
import enum

import numpy as np
import torch
import torch.nn as nn

from . import _lib, post_ops
from ._lib import check, ptr, stream_ptr

DISTS = ("l1", "l2")
CONFS = ("log", "sqrt", "m1", "id", "none")
SCHEDULES = ("cosine", "linear")


class GlobalAlignerMode(enum.Enum):
    PointCloudOptimizer = "PointCloudOptimizer"
    ModularPointCloudOptimizer = "ModularPointCloudOptimizer"
    PairViewer = "PairViewer"


# ------------------------------------------------------------------------------------------------------------------- small functions
def edge_str(i, j):
    return f"{i}_{j}"


def get_conf_trf(mode):
    """commons.py:54-77"""
    if mode == "log":
        return lambda x: x.log()
    if mode == "sqrt":
        return lambda x: x.sqrt()
    if mode == "m1":
        return lambda x: x - 1
    if mode in ("id", "none"):
        return lambda x: x
    raise ValueError(f"PointCloudOptimizer: conf must be one of {CONFS}, got {mode!r}")


def signed_log1p(x):
    return torch.sign(x) * torch.log1p(torch.abs(x))


def signed_expm1(x):
    return torch.sign(x) * torch.expm1(torch.abs(x))


def cosine_schedule(t, lr_start, lr_end):
    assert 0 <= t <= 1
    return lr_end + (lr_start - lr_end) * (1 + np.cos(t * np.pi)) / 2


def linear_schedule(t, lr_start, lr_end):
    assert 0 <= t <= 1
    return lr_start + (lr_end - lr_start) * t


def unitquat_to_rotmat(q):
    """(..., 4) unit quaternions in (x, y, z, w) order -> (..., 3, 3)"""
    x, y, z, w = q.unbind(-1)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = torch.ones_like(x)
    return torch.stack((one - (tyy + tzz), txy - twz, txz + twy,
                        txy + twz, one - (txx + tzz), tyz - twx,
                        txz - twy, tyz + twx, one - (txx + tyy)), dim=-1).reshape(q.shape[:-1] + (3, 3))


def rotmat_to_unitquat(R):
    """(..., 3, 3) rotations -> (..., 4) unit quaternions in (x, y, z, w) order, w >= 0 up to rounding.  Branch-free on the device: the four
    candidate forms are computed and the one with the largest pivot is taken."""
    m = R.reshape(R.shape[:-2] + (9,))
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = m.unbind(-1)
    piv = torch.stack((1 + m00 - m11 - m22, 1 - m00 + m11 - m22, 1 - m00 - m11 + m22, 1 + m00 + m11 + m22), dim=-1)
    cand = torch.stack((torch.stack((piv[..., 0], m01 + m10, m02 + m20, m21 - m12), dim=-1),
                        torch.stack((m01 + m10, piv[..., 1], m12 + m21, m02 - m20), dim=-1),
                        torch.stack((m02 + m20, m12 + m21, piv[..., 2], m10 - m01), dim=-1),
                        torch.stack((m21 - m12, m02 - m20, m10 - m01, piv[..., 3]), dim=-1)), dim=-2)
    best = piv.argmax(dim=-1)
    q = torch.gather(cand, -2, best[..., None, None].expand(best.shape + (1, 4))).squeeze(-2)
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.where(q[..., 3:4] < 0, -q, q)


def poses_from_params(poses):
    """`_get_poses` (base_opt.py:190-195): rows (quaternion xyzw, signed-log translation, ...) -> (n, 4, 4) camera-to-world"""
    Q = poses[:, :4]
    Q = Q / Q.norm(dim=-1, keepdim=True)
    T = signed_expm1(poses[:, 4:7])
    RT = torch.zeros((poses.shape[0], 4, 4), dtype=poses.dtype, device=poses.device)
    RT[:, :3, :3] = unitquat_to_rotmat(Q)
    RT[:, :3, 3] = T
    RT[:, 3, 3] = 1
    return RT


# ------------------------------------------------------------------------------------------------------------------- the loss
class Observations:
    """What `alignment_loss` needs beside the parameters: the views' shapes, the edges and per (edge, side) a pointmap (H, W, 3), a weight map
    (H, W) -- fp32 on one ROCm device, contiguous; edges may share one tensor, which is then stored once -- and the device tables of the
    kernel.  Built once per problem.  Argument errors are ValueErrors raised before any device work."""

    def __init__(self, shapes, edges, pointmaps, weights):
        self.shapes = [(int(H), int(W)) for H, W in shapes]
        self.edges = [(int(i), int(j)) for i, j in edges]
        N, E = len(self.shapes), len(self.edges)
        if N < 2 or E < 1:
            raise ValueError(f"alignment_loss: need at least two views and one edge, got {N} and {E}")
        if len(pointmaps) != 2 * E or len(weights) != 2 * E:
            raise ValueError(f"alignment_loss: {E} edges need {2 * E} pointmaps and weight maps (edge-major, side i then side j), got "
                             f"{len(pointmaps)} and {len(weights)}")
        dev = next((p.device for p in pointmaps if p is not None), None)
        maps = []
        for o, (p, w) in enumerate(zip(pointmaps, weights)):
            e, side = divmod(o, 2)
            i, j = self.edges[e]
            if not (0 <= i < N and 0 <= j < N):
                raise ValueError(f"alignment_loss: edge {e} = ({i}, {j}) lies outside the {N} views")
            if i == j:
                raise ValueError(f"alignment_loss: edge {e} joins view {i} with itself")
            H, W = self.shapes[j if side else i]
            if p is None or w is None:
                raise ValueError(f"alignment_loss: edge {e}, side {side} has no pointmap or no weight map")
            if tuple(p.shape) != (H, W, 3) or tuple(w.shape) != (H, W):
                raise ValueError(f"alignment_loss: edge {e}, side {side}: pointmap {tuple(p.shape)} and weights {tuple(w.shape)} against view "
                                 f"{j if side else i} of {(H, W)}")
            for t, what in ((p, "pointmap"), (w, "weight map")):
                if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
                    raise ValueError(f"alignment_loss: the {what} of edge {e}, side {side} must be contiguous fp32 on {dev}")
            maps.append((p, w, H, W))
        _lib.require_gpu(pointmaps[0], "pointmaps")
        self.device = dev
        self.tables = post_ops.galign_tables(self.shapes, self.edges, maps, dev)
        self.total = self.tables["total"]


class _AlignmentLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im_poses, focals, pp, log_depths, pw_poses, adaptors, observations, dist):
        f32 = torch.float32
        prep = lambda t: t.detach().to(f32).contiguous()  # noqa: E731
        loss, *grads = post_ops.galign_loss_grad(prep(im_poses[:, :3]), prep(focals.reshape(-1)), prep(pp), prep(log_depths.reshape(-1)),
                                                 prep(pw_poses[:, :3]), prep(adaptors), observations.tables, dist)
        ctx.save_for_backward(*grads)
        ctx.meta = [(tuple(t.shape), t.dtype) for t in (log_depths, im_poses, focals, pp, pw_poses, adaptors)]
        return loss.to(f32)

    @staticmethod
    def backward(ctx, grad_output):
        out = []
        for g, (shape, dtype) in zip(ctx.saved_tensors, ctx.meta):
            g = g * grad_output
            if len(shape) == 3 and shape[1] == 4:  # a (n, 4, 4) pose: the bottom row has no gradient
                g = torch.cat((g, torch.zeros_like(g[:, :1])), dim=1)
            out.append(g.reshape(shape).to(dtype))
        d_l, d_T, d_f, d_c, d_M, d_a = out
        return d_T, d_f, d_c, d_l, d_M, d_a, None, None


def alignment_loss(im_poses, focals, pp, log_depths, pw_poses, adaptors, observations, dist="l1"):
    """The loss of `PointCloudOptimizer.forward` as a 0-dim fp32 device tensor with a backward: one kernel call computes it and every
    gradient; backward hands them out times grad_output.  im_poses (N, 4, 4) or (N, 3, 4) camera-to-world, focals (N,) or (N, 1), pp (N, 2),
    log_depths (total,): the views' log depths one after another, pw_poses (E, 4, 4) or (E, 3, 4) scaled pairwise poses, adaptors (E, 3),
    observations: an `Observations`.  No host synchronisation."""
    if dist not in DISTS:
        raise ValueError(f"alignment_loss: dist must be 'l1' or 'l2', got {dist!r}")
    if not isinstance(observations, Observations):
        raise ValueError("alignment_loss: observations must be an Observations")
    N, E = len(observations.shapes), len(observations.edges)
    for t, name, shapes in ((im_poses, "im_poses", ((N, 4, 4), (N, 3, 4))), (focals, "focals", ((N,), (N, 1))), (pp, "pp", ((N, 2),)),
                            (log_depths, "log_depths", ((observations.total,),)), (pw_poses, "pw_poses", ((E, 4, 4), (E, 3, 4))),
                            (adaptors, "adaptors", ((E, 3),))):
        if tuple(t.shape) not in shapes:
            raise ValueError(f"alignment_loss: {name} must be {' or '.join(map(str, shapes))}, got {tuple(t.shape)}")
    return _AlignmentLoss.apply(im_poses, focals, pp, log_depths, pw_poses, adaptors, observations, dist)


# ------------------------------------------------------------------------------------------------------------------- the optimizer
def _entries(x, n, what):
    if torch.is_tensor(x) or isinstance(x, np.ndarray):
        x = list(x)
    x = [torch.as_tensor(t) for t in x]
    if len(x) != n:
        raise ValueError(f"PointCloudOptimizer: {what} has {len(x)} entries for {n} edges")
    return x


def _idx_list(idx):
    return [int(i) for i in (idx.tolist() if hasattr(idx, "tolist") else idx)]


class PointCloudOptimizer(nn.Module):
    """The reference's `PointCloudOptimizer` (optimizer.py, base_opt.py): graph nodes are images, edges are observations (pred1, pred2).
    Parameters, under the reference's names: pw_poses (E, 8) = quaternion xyzw, signed-log translation, log scale; pw_adaptors (E, 2);
    im_poses (N, 7); im_focals (N, 1) = focal_break log f; im_pp (N, 2) in tenths of a pixel around (W / 2, H / 2); im_depthmaps: the log
    depths of the views one after another (total,), where the reference pads every view to the largest area."""
    POSE_DIM = 7

    def __init__(self, view1, view2, pred1, pred2, dist="l1", conf="log", min_conf_thr=3, base_scale=0.5, allow_pw_adaptors=False,
                 pw_break=20, optimize_pp=False, focal_break=20, rand_pose=torch.randn):
        super().__init__()
        if dist not in DISTS:
            raise ValueError(f"PointCloudOptimizer: dist must be 'l1' or 'l2', got {dist!r}")
        self.conf_trf = get_conf_trf(conf)
        i1, i2 = _idx_list(view1["idx"]), _idx_list(view2["idx"])
        if len(i1) != len(i2) or len(i1) < 1:
            raise ValueError(f"PointCloudOptimizer: view1 has {len(i1)} indices, view2 {len(i2)}; need one edge at least and equal lengths")
        self.edges = list(zip(i1, i2))
        self.is_symmetrized = set(self.edges) == {(j, i) for i, j in self.edges}
        self.dist = dist
        self.n_imgs = self._check_edges()
        E = self.n_edges
        pts_i, pts_j = _entries(pred1["pts3d"], E, "pred1['pts3d']"), _entries(pred2["pts3d_in_other_view"], E, "pred2['pts3d_in_other_view']")
        conf_i, conf_j = _entries(pred1["conf"], E, "pred1['conf']"), _entries(pred2["conf"], E, "pred2['conf']")
        self.imshapes = [None] * self.n_imgs
        for e, (i, j) in enumerate(self.edges):
            for v, p, c, side in ((i, pts_i[e], conf_i[e], "i"), (j, pts_j[e], conf_j[e], "j")):
                if p.dim() != 3 or p.shape[-1] != 3 or tuple(c.shape) != tuple(p.shape[:2]):
                    raise ValueError(f"PointCloudOptimizer: edge {e}, side {side}: pointmap {tuple(p.shape)} and confidence {tuple(c.shape)}; need "
                                     "(H, W, 3) and (H, W)")
                if self.imshapes[v] is not None and self.imshapes[v] != tuple(p.shape[:2]):
                    raise ValueError(f"PointCloudOptimizer: incorrect shape for image {v}: {tuple(p.shape[:2])} on edge {e}, {self.imshapes[v]} before")
                self.imshapes[v] = tuple(p.shape[:2])
        # one stored tensor per distinct input map: edges of one pass share their anchor's pointmap and confidence
        self._unique, self._pts, self._conf, self._weight = {}, [], [], []
        for e in range(E):
            for p, c in ((pts_i[e], conf_i[e]), (pts_j[e], conf_j[e])):
                self._pts.append(self._keep(p))
                cc = self._keep(c)
                self._conf.append(cc)
                self._weight.append(self._keep(cc, trf=True))
        self.pred_i = {edge_str(i, j): self._pts[2 * e] for e, (i, j) in enumerate(self.edges)}
        self.pred_j = {edge_str(i, j): self._pts[2 * e + 1] for e, (i, j) in enumerate(self.edges)}
        self.conf_i = {edge_str(i, j): self._conf[2 * e] for e, (i, j) in enumerate(self.edges)}
        self.conf_j = {edge_str(i, j): self._conf[2 * e + 1] for e, (i, j) in enumerate(self.edges)}
        self.min_conf_thr = min_conf_thr
        self.im_conf = self._compute_img_conf()
        self.base_scale, self.norm_pw_scale, self.pw_break, self.focal_break = base_scale, True, pw_break, focal_break
        self.rand_pose, self.has_im_poses, self.verbose, self.imgs = rand_pose, True, False, None
        self.pw_poses = nn.Parameter(rand_pose((E, 1 + self.POSE_DIM)))
        self.pw_adaptors = nn.Parameter(torch.zeros((E, 2)))
        self.pw_adaptors.requires_grad_(allow_pw_adaptors)
        areas = [h * w for h, w in self.imshapes]
        self._offsets = [0]
        for a in areas:
            self._offsets.append(self._offsets[-1] + a)
        self.imshape, self.max_area = self.imshapes[0], max(areas)
        self.im_depthmaps = nn.Parameter(torch.cat([(torch.randn(H, W) / 10 - 3).reshape(-1) for H, W in self.imshapes]))
        self.im_poses = nn.Parameter(torch.stack([rand_pose(self.POSE_DIM) for _ in range(self.n_imgs)]))
        self.im_focals = nn.Parameter(torch.tensor([[focal_break * np.log(max(H, W))] for H, W in self.imshapes], dtype=torch.float32))
        self.im_pp = nn.Parameter(torch.zeros((self.n_imgs, 2)))
        self.im_pp.requires_grad_(optimize_pp)
        self.register_buffer("_pp", torch.tensor([(w / 2, h / 2) for h, w in self.imshapes], dtype=torch.float32))
        self.total_area_i = sum(areas[i] for i, j in self.edges)
        self.total_area_j = sum(areas[j] for i, j in self.edges)
        self._passes = view1.get("passes") if isinstance(view1, dict) else None
        self._obs, self.loss_history = None, None

    # ---- storage
    def _keep(self, t, trf=False):
        key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), str(t.device), trf)
        if key not in self._unique:
            s = t.detach().to(torch.float32).contiguous()
            self._unique[key] = self.conf_trf(s) if trf else s
        return self._unique[key]

    def _apply(self, fn, *a, **kw):
        super()._apply(fn, *a, **kw)
        moved = {}

        def mv(t):
            if id(t) not in moved:
                moved[id(t)] = fn(t)
            return moved[id(t)]
        for name in ("_pts", "_conf", "_weight", "im_conf"):
            setattr(self, name, [mv(t) for t in getattr(self, name)])
        for name in ("pred_i", "pred_j", "conf_i", "conf_j"):
            setattr(self, name, {k: mv(t) for k, t in getattr(self, name).items()})
        self._unique, self._obs = {}, None
        return self

    def _observations(self):
        if self._obs is None:
            self._obs = Observations(self.imshapes, self.edges, self._pts, self._weight)
        return self._obs

    @property
    def n_edges(self):
        return len(self.edges)

    @property
    def str_edges(self):
        return [edge_str(i, j) for i, j in self.edges]

    @property
    def imsizes(self):
        return [(w, h) for h, w in self.imshapes]

    @property
    def device(self):
        return self.pw_poses.device

    def _check_edges(self):
        indices = sorted({i for edge in self.edges for i in edge})
        if indices != list(range(len(indices))):
            raise ValueError(f"PointCloudOptimizer: bad pair indices: missing values (the views must be 0 .. n - 1 without gaps, got {indices})")
        if any(i == j for i, j in self.edges):
            raise ValueError("PointCloudOptimizer: an edge joins a view with itself")
        if len(indices) < 2:
            raise ValueError("PointCloudOptimizer: need at least two views")
        return len(indices)

    @torch.no_grad()
    def _compute_img_conf(self):
        im_conf = [None] * self.n_imgs
        for e, (i, j) in enumerate(self.edges):
            for v, c in ((i, self._conf[2 * e]), (j, self._conf[2 * e + 1])):
                if im_conf[v] is None:
                    im_conf[v] = torch.maximum(torch.zeros_like(c), c)
                elif im_conf[v] is not c:
                    im_conf[v] = torch.maximum(im_conf[v], c)
        return im_conf

    # ---- pairwise parameters
    def get_adaptors(self, _raw=None):
        adapt = self.pw_adaptors if _raw is None else _raw
        adapt = torch.cat((adapt[:, 0:1], adapt), dim=-1)  # (scale_xy, scale_xy, scale_z)
        if self.norm_pw_scale:  # normalize so that the product == 1
            adapt = adapt - adapt.mean(dim=1, keepdim=True)
        return (adapt / self.pw_break).exp()

    def _get_poses(self, poses):
        return poses_from_params(poses)

    def _set_pose(self, poses, idx, R, T=None, scale=None, force=False):
        pose = poses[idx]
        if not (pose.requires_grad or force):
            return pose
        if R is not None and tuple(R.shape) == (4, 4):
            assert T is None
            T = R[:3, 3]
            R = R[:3, :3]
        if R is not None:
            pose.data[0:4] = rotmat_to_unitquat(torch.as_tensor(R).to(pose.device, pose.dtype))
        if T is not None:
            pose.data[4:7] = signed_log1p(torch.as_tensor(T).to(pose.device, pose.dtype) / (scale or 1))
        if scale is not None:
            assert poses.shape[-1] in (8, 13)
            pose.data[-1] = np.log(float(scale))
        return pose

    def get_pw_norm_scale_factor(self, _raw=None):
        if self.norm_pw_scale:
            return (np.log(self.base_scale) - (self.pw_poses if _raw is None else _raw)[:, -1].mean()).exp()
        return 1

    def get_pw_scale(self, _raw=None):
        return (self.pw_poses if _raw is None else _raw)[:, -1].exp() * self.get_pw_norm_scale_factor(_raw)

    def get_pw_poses(self, _raw=None):
        RT = self._get_poses(self.pw_poses if _raw is None else _raw)
        scaled = RT.clone()
        scaled[:, :3] *= self.get_pw_scale(_raw).view(-1, 1, 1)
        return scaled

    # ---- image parameters
    def _get_msk_indices(self, msk):
        if msk is None:
            return range(self.n_imgs)
        if isinstance(msk, int):
            return [msk]
        if isinstance(msk, (tuple, list)):
            return self._get_msk_indices(np.array(msk))
        if msk.dtype in (bool, torch.bool, np.bool_):
            assert len(msk) == self.n_imgs
            return np.where(msk)[0]
        if np.issubdtype(msk.dtype, np.integer):
            return msk
        raise ValueError(f"bad {msk=}")

    def _check_all_imgs_are_selected(self, msk):
        if not np.all(np.asarray(self._get_msk_indices(msk)) == np.arange(self.n_imgs)):
            raise ValueError("incomplete mask!")

    def _no_grad(self, tensor):
        assert tensor.requires_grad, "it must be True at this point, otherwise no modification occurs"

    def preset_pose(self, known_poses, pose_msk=None):
        self._check_all_imgs_are_selected(pose_msk)
        if isinstance(known_poses, torch.Tensor) and known_poses.ndim == 2:
            known_poses = [known_poses]
        for idx, pose in zip(self._get_msk_indices(pose_msk), known_poses):
            self._no_grad(self._set_pose(self.im_poses, idx, torch.as_tensor(pose)))
        self.im_poses.requires_grad_(False)
        self.norm_pw_scale = False

    def preset_focal(self, known_focals, msk=None):
        self._check_all_imgs_are_selected(msk)
        for idx, focal in zip(self._get_msk_indices(msk), known_focals):
            self._no_grad(self._set_focal(idx, focal))
        self.im_focals.requires_grad_(False)

    def preset_principal_point(self, known_pp, msk=None):
        self._check_all_imgs_are_selected(msk)
        for idx, pp in zip(self._get_msk_indices(msk), known_pp):
            self._no_grad(self._set_principal_point(idx, pp))
        self.im_pp.requires_grad_(False)

    def _set_focal(self, idx, focal, force=False):
        param = self.im_focals[idx]
        if param.requires_grad or force:
            param.data[:] = self.focal_break * torch.log(torch.as_tensor(focal, dtype=param.dtype).to(param.device))
        return param

    def get_focals(self):
        return (self.im_focals / self.focal_break).exp()

    def get_known_focal_mask(self):
        return torch.tensor([not self.im_focals.requires_grad] * self.n_imgs)

    def _set_principal_point(self, idx, pp, force=False):
        param = self.im_pp[idx]
        H, W = self.imshapes[idx]
        if param.requires_grad or force:
            pp = torch.as_tensor(pp, dtype=param.dtype).to(param.device)
            param.data[:] = (pp - torch.tensor((W / 2, H / 2), dtype=param.dtype, device=param.device)) / 10
        return param

    def get_principal_points(self):
        return self._pp + 10 * self.im_pp

    def get_intrinsics(self):
        K = torch.zeros((self.n_imgs, 3, 3), device=self.device)
        focals = self.get_focals().flatten()
        K[:, 0, 0] = K[:, 1, 1] = focals
        K[:, :2, 2] = self.get_principal_points()
        K[:, 2, 2] = 1
        return K

    def get_im_poses(self):
        return self._get_poses(self.im_poses)

    def _view_slice(self, idx):
        return slice(self._offsets[idx], self._offsets[idx + 1])

    def _set_depthmap(self, idx, depth, force=False):
        param = self.im_depthmaps[self._view_slice(idx)]
        if param.requires_grad or force:
            depth = torch.as_tensor(depth).to(param.device, param.dtype).reshape(-1)
            param.data[:] = depth.log().nan_to_num(neginf=0)
        return param

    def get_depthmaps(self, raw=False):
        res = self.im_depthmaps.exp()
        if raw:
            return res
        return [res[self._view_slice(v)].view(h, w) for v, (h, w) in enumerate(self.imshapes)]

    def depth_to_pts3d(self):
        """the world points of every view (optimizer.py:219-229), as plain torch operations: an accessor, not the loss's path"""
        focals, pp, poses, out = self.get_focals(), self.get_principal_points(), self.get_im_poses(), []
        for v, d in enumerate(self.get_depthmaps()):
            H, W = self.imshapes[v]
            ys, xs = torch.meshgrid(torch.arange(H, device=d.device, dtype=d.dtype), torch.arange(W, device=d.device, dtype=d.dtype), indexing="ij")
            q = torch.stack((d * (xs - pp[v, 0]) / focals[v, 0], d * (ys - pp[v, 1]) / focals[v, 0], d), dim=-1)
            out.append(q @ poses[v, :3, :3].T + poses[v, :3, 3])
        return out

    def get_pts3d(self, raw=False):
        res = self.depth_to_pts3d()
        if raw:
            return torch.cat([p.reshape(-1, 3) for p in res])
        return res

    def get_masks(self):
        return [(conf > self.min_conf_thr) for conf in self.im_conf]

    def get_conf(self, mode=None):
        trf = self.conf_trf if mode is None else get_conf_trf(mode)
        return [trf(c) for c in self.im_conf]

    # ---- the loss and the loop
    def forward(self):
        """The chain from the raw parameters to the kernel's matrices runs in fp64 here (a few N- and E-sized tensors; the getters keep the
        parameters' precision): the gradients of the focals and the adaptors are sums that cancel, and an fp32 `exp` of the device, a last
        bit or two off, moved them by several times what the reference's own fp32 run is off (docs/rows_f.md).  The matrices are rounded to
        fp32 once, for the kernel."""
        d = torch.float64
        return alignment_loss(self._get_poses(self.im_poses.to(d)), (self.im_focals.to(d) / self.focal_break).exp(),
                              self._pp.to(d) + 10 * self.im_pp.to(d), self.im_depthmaps, self.get_pw_poses(self.pw_poses.to(d)),
                              self.get_adaptors(self.pw_adaptors.to(d)), self._observations(), self.dist)

    @torch.no_grad()
    def clean_pointcloud(self, tol=0.001, max_bad_conf=0):
        """`BasePCOptimizer.clean_pointcloud` on the object's own poses, intrinsics, depths and im_conf (fast3r_amd/clean.py) -> a shallow
        copy of the object with `im_conf` replaced; the parameters are shared with it."""
        from .clean import clean_confidences
        conf = clean_confidences(self.get_pts3d(), self.im_conf, self.get_depthmaps(), self.get_im_poses(), self.get_focals().flatten(),
                                 self.get_principal_points(), tol=tol, max_bad_conf=max_bad_conf)
        res = copy.copy(self)
        res.im_conf = list(conf)
        return res

    @staticmethod
    def _read_back(history):
        """the loop's one device-to-host read"""
        return history.cpu()

    def compute_global_alignment(self, init=None, niter=300, schedule="cosine", lr=0.01, lr_min=1e-6):
        """base_opt.py:348-453 without the per-iteration `float(loss)`: the losses land in a device tensor that is read once.  -> the final
        loss as a float; `.loss_history` keeps all of them (fp32, host)."""
        if schedule not in SCHEDULES:
            raise ValueError(f"compute_global_alignment: schedule must be 'cosine' or 'linear', got {schedule!r}")
        niter = int(niter)
        if niter < 0:
            raise ValueError(f"compute_global_alignment: niter = {niter}; need niter >= 0")
        if init is None:
            pass
        elif init == "passes":
            self._init_from_passes()
        elif init in ("mst", "msp", "known_poses"):
            raise NotImplementedError(f"compute_global_alignment: init={init!r} needs fast_pnp and one registration per edge on pairwise "
                                      "predictions (init_minimum_spanning_tree / init_from_known_poses), which this project does not have yet")
        else:
            raise ValueError(f"compute_global_alignment: bad value for init={init!r}")
        params = [p for p in self.parameters() if p.requires_grad]
        if not params:
            return self
        sched = cosine_schedule if schedule == "cosine" else linear_schedule
        optimizer = torch.optim.Adam(params, lr=lr, betas=(0.9, 0.9))
        history = torch.empty(niter, dtype=torch.float32, device=self.device)
        for n in range(niter):
            cur = float(sched(n / niter, lr, lr_min))
            for group in optimizer.param_groups:
                group["lr"] = cur
            optimizer.zero_grad()
            loss = self()
            loss.backward()
            optimizer.step()
            history[n] = loss.detach()
        self.loss_history = self._read_back(history)
        return float(self.loss_history[-1]) if niter else float("inf")

    @torch.no_grad()
    def _init_from_passes(self):
        """The start of `init="passes"`: poses, focals and depths of pass 0; every edge of pass k from the one similarity that registers pass k's
        anchor pointmap onto the initial world points of that view (f3r_align_local_to_global, quantile 0: every pixel)."""
        from .pose import estimate_camera_poses_device
        who = "compute_global_alignment(init='passes')"
        if self._passes is None:
            raise ValueError(f"{who}: the optimizer was not built from pairs_from_passes(...)")
        preds, orders, edge_pass = self._passes["preds"], self._passes["orders"], self._passes["edge_pass"]
        dev = self.device
        poses, focals = estimate_camera_poses_device(preds[0])
        poses, focals = poses[0].to(dev), focals[0].to(dev)
        default = (self.im_focals.data[:, 0] / self.focal_break).exp()
        for p, v in enumerate(orders[0]):
            self._set_pose(self.im_poses, v, poses[p])
            self._set_focal(v, torch.where(torch.isfinite(focals[p]), focals[p], default[v]))
            self._set_depthmap(v, _sample0(preds[0][p]["pts3d_local"])[..., 2])
        world = self.depth_to_pts3d()
        lib = _lib.lib()
        rows = torch.empty((len(preds), 8), dtype=torch.float32, device=dev)
        for k, order in enumerate(orders):
            a = order[0]
            H, W = self.imshapes[a]
            loc = _sample0(preds[k][0]["pts3d_in_other_view"]).to(dev, torch.float32).contiguous()
            conf = _sample0(preds[k][0]["conf"]).to(dev, torch.float32).contiguous()
            glo = world[a].to(torch.float32).contiguous()
            out, rts = torch.empty_like(loc), torch.empty((1, 13), dtype=torch.float32, device=dev)
            nbytes = lib.f3r_align_workspace_bytes(1)
            ws = torch.empty((max(nbytes // 8, 1),), dtype=torch.float64, device=dev)
            with torch.cuda.device(dev):
                check(lib.f3r_align_local_to_global(ptr(conf), ptr(loc), ptr(glo), None, ptr(out), ptr(rts), None, ptr(ws), nbytes, 1, H * W, 0.0,
                                                    stream_ptr()), "f3r_align_local_to_global")
            R, t, s = rts[0, :9].view(3, 3), rts[0, 9:12], rts[0, 12]
            rows[k, :4], rows[k, 4:7], rows[k, 7] = rotmat_to_unitquat(R), signed_log1p(t / s), s.log()
        if self.pw_poses.requires_grad:
            self.pw_poses.data[:] = rows[torch.as_tensor(edge_pass, device=dev)]
        if self.norm_pw_scale:  # the world is rescaled with the pairwise scales (init_im_poses.py does the same after its spanning tree)
            factor = self.get_pw_norm_scale_factor()
            if self.im_poses.requires_grad:
                self.im_poses.data[:, 4:7] = signed_log1p(signed_expm1(self.im_poses.data[:, 4:7]) * factor)
            if self.im_depthmaps.requires_grad:
                self.im_depthmaps.data += factor.log()


def _sample0(t):
    """(B, H, W, ...) -> sample 0; a map without the batch dimension passes"""
    t = torch.as_tensor(t)
    return t[0] if t.dim() in (4,) or (t.dim() == 3 and t.shape[-1] != 3) else t


def global_aligner(dust3r_output, device, mode=GlobalAlignerMode.PointCloudOptimizer, **optim_kw):
    """cloud_opt/__init__.py:26-45: builds the optimizer from dict(view1, view2, pred1, pred2) and moves it to `device`."""
    view1, view2, pred1, pred2 = [dust3r_output[k] for k in "view1 view2 pred1 pred2".split()]
    if mode == GlobalAlignerMode.PointCloudOptimizer:
        return PointCloudOptimizer(view1, view2, pred1, pred2, **optim_kw).to(device)
    if mode in (GlobalAlignerMode.ModularPointCloudOptimizer, GlobalAlignerMode.PairViewer):
        raise NotImplementedError(f"global_aligner: mode {mode.value} is not implemented (PointCloudOptimizer only)")
    raise NotImplementedError(f"Unknown mode {mode}")


def pairs_from_passes(outputs, anchors):
    """K forward passes over the same N images with different anchor views -> (view1, view2, pred1, pred2) in the reference's layout.
    outputs[k]: an `inference()` output (or its preds list) whose first view is view anchors[k] of the common numbering and whose other
    views follow in ascending order of that numbering; anchors[k] may also be the pass's whole order, a permutation of 0 .. N - 1.  Pass k
    gives the edges (a_k, v) for every other view v: pred1['pts3d'] = the anchor's global-head pointmap, pred2['pts3d_in_other_view'] = view
    v's, and the two `conf` maps, of sample 0.  No pointmap is copied: the anchor's tensor is one object shared by its edges."""
    who = "pairs_from_passes"
    if len(outputs) != len(anchors) or len(outputs) < 1:
        raise ValueError(f"{who}: {len(outputs)} passes for {len(anchors)} anchors; need one pass at least and equal lengths")
    preds_all, orders = [], []
    for k, (out, a) in enumerate(zip(outputs, anchors)):
        preds = out["preds"] if isinstance(out, dict) else out
        N = len(preds)
        if k and N != len(preds_all[0]):
            raise ValueError(f"{who}: pass {k} has {N} views, pass 0 has {len(preds_all[0])}")
        if N < 2:
            raise ValueError(f"{who}: pass {k} has {N} views; need two at least")
        order = [int(x) for x in a] if isinstance(a, (list, tuple, np.ndarray)) else [int(a)] + [v for v in range(N) if v != int(a)]
        if sorted(order) != list(range(N)):
            raise ValueError(f"{who}: the order of pass {k} is {order}: not a permutation of 0 .. {N - 1}")
        for p in preds:
            for key in ("pts3d_in_other_view", "conf"):
                if key not in p:
                    raise KeyError(f"{who}: a pred of pass {k} has no '{key}'")
        preds_all.append(preds)
        orders.append(order)
    idx1, idx2, p1, c1, p2, c2, edge_pass = [], [], [], [], [], [], []
    for k, (preds, order) in enumerate(zip(preds_all, orders)):
        pts = [_sample0(p["pts3d_in_other_view"]) for p in preds]
        conf = [_sample0(p["conf"]) for p in preds]
        for pos in range(1, len(order)):
            idx1.append(order[0])
            idx2.append(order[pos])
            p1.append(pts[0])
            c1.append(conf[0])
            p2.append(pts[pos])
            c2.append(conf[pos])
            edge_pass.append(k)
    view1 = {"idx": idx1, "passes": {"preds": preds_all, "orders": orders, "edge_pass": edge_pass}}
    return view1, {"idx": idx2}, {"pts3d": p1, "conf": c1}, {"pts3d_in_other_view": p2, "conf": c2}
