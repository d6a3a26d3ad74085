"""Tensor-level wrappers over the C ABI (include/f3r.h) for what runs after the forward pass: the camera-pose metrics, the multi-view
loss, scene assembly, sky detection, mesh export, point-cloud export, the point-splat renderer, the map pictures, the ground-truth views, the depth metrics, view matching, confidence cleaning and global alignment.  Like fast3r_amd/ops.py (the model's operators), these only check arguments, lay
out the per-view device tables and launch: every arithmetic op is a HIP kernel in fast3r_amd/csrc/, and CPU tensors raise F3RError.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require_gpu, stream_ptr


def _thresholds(ts):
    ts = [float(t) for t in ts]
    return (ctypes.c_double * max(1, len(ts)))(*ts), len(ts)


def _real_id(dt):
    if dt == torch.float32:
        return _lib.F3R_REAL_F32
    if dt == torch.float64:
        return _lib.F3R_REAL_F64
    raise ValueError(f"fast3r_amd: camera-pose metrics take torch.float32 or torch.float64, got {dt}")


def pose_pair_metrics(pred, gt, r_thresholds, t_thresholds, n_bins, max_threshold, want_pairs=False):
    """Relative-pose errors of every view pair i < j of every sample (cam_pose_metric.py:17-40) and their counts.  pred, gt: (B, N, 4, 4)
    cam-to-world, fp32 or fp64, same dtype, on the GPU.  -> (counts int64 (B, n_r + n_t + n_bins + 2) = thresholds passed | histc bins of
    max(r, t) | pairs with a trace out of range | pairs with the 1e6 default, rel_r, rel_t): the per-pair errors in degrees, (B, N (N - 1) / 2)
    in the input dtype in torch.combinations order, only with want_pairs (otherwise None: nothing per pair is allocated or written)."""
    require_gpu(pred, "pred")
    require_gpu(gt, "gt")
    if pred.dim() != 4 or tuple(pred.shape[2:]) != (4, 4) or pred.shape != gt.shape or pred.dtype != gt.dtype:
        raise ValueError(f"pred and gt must both be (B, N, 4, 4) of one dtype; got {tuple(pred.shape)} {pred.dtype} and {tuple(gt.shape)} {gt.dtype}")
    B, N = pred.shape[:2]
    pred, gt = pred.contiguous(), gt.contiguous()
    rt, n_r = _thresholds(r_thresholds)
    tt, n_t = _thresholds(t_thresholds)
    counts = torch.empty((B, n_r + n_t + int(n_bins) + 2), dtype=torch.int64, device=pred.device)
    rel_r = torch.empty((B, N * (N - 1) // 2), dtype=pred.dtype, device=pred.device) if want_pairs else None
    rel_t = torch.empty_like(rel_r) if want_pairs else None
    with torch.cuda.device(pred.device):
        check(_lib.lib().f3r_pose_pair_metrics(ptr(pred), ptr(gt), _real_id(pred.dtype), B, N, rt, n_r, tt, n_t, int(n_bins), float(max_threshold),
                                               ptr(rel_r), ptr(rel_t), ptr(counts), stream_ptr()), "f3r_pose_pair_metrics")
    return counts, rel_r, rel_t


def pose_error_stats(r_error, t_error, r_thresholds, t_thresholds, n_bins, max_threshold):
    """The counts of pose_pair_metrics from given per-pair errors (1-D, same length and dtype, on the GPU): int64 (n_r + n_t + n_bins + 2)."""
    require_gpu(r_error, "r_error")
    require_gpu(t_error, "t_error")
    if r_error.dim() != 1 or r_error.shape != t_error.shape or r_error.dtype != t_error.dtype:
        raise ValueError(f"r_error and t_error must be 1-D, of one length and dtype; got {tuple(r_error.shape)} {r_error.dtype} and "
                         f"{tuple(t_error.shape)} {t_error.dtype}")
    r_error, t_error = r_error.contiguous(), t_error.contiguous()
    n = r_error.numel()
    rt, n_r = _thresholds(r_thresholds)
    tt, n_t = _thresholds(t_thresholds)
    counts = torch.empty(n_r + n_t + int(n_bins) + 2, dtype=torch.int64, device=r_error.device)
    with torch.cuda.device(r_error.device):
        check(_lib.lib().f3r_pose_error_stats(ptr(r_error) if n else None, ptr(t_error) if n else None, n, _real_id(r_error.dtype), rt, n_r, tt, n_t,
                                              int(n_bins), float(max_threshold), ptr(counts), stream_ptr()), "f3r_pose_error_stats")
    return counts


def mv_conf_loss(gt_pts, valid_mask, camera_pose, pred_pts, pred_conf, pred_pts_local=None, pred_conf_local=None, *, version=4, dis_mode=0,
                 gt_scale=False, local_scale_consistent=False, dist_clip=None, alpha=1.0):
    """ConfLossMultiviewV2(Regr3DMultiviewV3 | V4(L21Loss, avg_dis | avg_log1p), alpha) on the device (f3r_mv_conf_loss, include/f3r.h).
    Lists over views of GPU tensors: gt_pts / pred_pts / pred_pts_local (B, H, W, 3) fp32, valid_mask (B, H, W) bool or uint8, camera_pose
    (B, 4, 4) fp32 or fp64, pred_conf / pred_conf_local (B, H, W) fp32; (H, W) may differ between views.  Nothing is concatenated: the
    kernels read every tensor where it lies (a non-contiguous one is made contiguous first).  -> fp64 device tensor (1 + 4 V):
    total | pts3d_loss_global | pts3d_loss_local | conf_loss_global | conf_loss_local (the local parts only with a local head)."""
    V = len(gt_pts)
    local = pred_pts_local is not None
    lists = [gt_pts, valid_mask, camera_pose, pred_pts, pred_conf] + ([pred_pts_local, pred_conf_local] if local else [])
    if V < 1 or any(x is None or len(x) != V for x in lists):
        raise ValueError("mv_conf_loss: every per-view list must have one entry per view (at least one view); pred_pts_local and "
                         "pred_conf_local are given together")
    dev = gt_pts[0].device
    B = gt_pts[0].shape[0]
    keep, rows, npix = [], [[] for _ in range(7)], []
    pose_dtype = camera_pose[0].dtype
    for v in range(V):
        g = gt_pts[v]
        if g.dim() != 4 or g.shape[-1] != 3 or g.shape[0] != B:
            raise ValueError(f"mv_conf_loss: view {v}: pts3d must be (B = {B}, H, W, 3), got {tuple(g.shape)}")
        want = {0: (g.shape, torch.float32), 3: (g.shape, torch.float32), 5: (g.shape, torch.float32), 1: (g.shape[:3], None),
                4: (g.shape[:3], torch.float32), 6: (g.shape[:3], torch.float32), 2: ((B, 4, 4), pose_dtype)}
        for i, lst in enumerate(lists):
            t = lst[v]
            require_gpu(t, f"view {v} of input {i}")
            shape, dt = want[i]
            if i == 1:
                if t.dtype not in (torch.bool, torch.uint8):
                    raise ValueError(f"mv_conf_loss: view {v}: valid_mask must be bool or uint8, got {t.dtype}")
            elif t.dtype != dt:
                raise ValueError(f"mv_conf_loss: view {v}, input {i}: expected {dt}, got {t.dtype}")
            if tuple(t.shape) != tuple(shape) or t.device != dev:
                raise ValueError(f"mv_conf_loss: view {v}, input {i}: expected shape {tuple(shape)} on {dev}, got {tuple(t.shape)} on {t.device}")
            t = t.contiguous()
            keep.append(t)
            rows[i].append(t.data_ptr())
        npix.append(g.shape[1] * g.shape[2])
    if not local:
        rows[5] = rows[6] = [0] * V
    table = torch.tensor(rows + [npix], dtype=torch.int64).to(dev)  # one small upload: 7 pointer tables and the pixel counts
    l = _lib.lib()
    ws_bytes = l.f3r_mv_conf_loss_workspace_bytes(V, B)
    if ws_bytes == 0:
        raise ValueError(f"mv_conf_loss: {V} views x {B} samples is not a supported shape")
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty(1 + 4 * V, dtype=torch.float64, device=dev)
    row = lambda i: table[i].data_ptr()  # noqa: E731
    with torch.cuda.device(dev):
        check(l.f3r_mv_conf_loss(row(0), row(1), row(2), _real_id(pose_dtype), row(3), row(4), row(5) if local else None, row(6) if local else None,
                                 row(7), V, B, int(version), int(dis_mode), int(bool(gt_scale)), int(bool(local_scale_consistent)),
                                 int(dist_clip is not None), float(dist_clip) if dist_clip is not None else 0.0, float(alpha), ptr(ws), ws_bytes,
                                 ptr(out), stream_ptr()), "f3r_mv_conf_loss")
    del keep  # the launches are stream-ordered before the caching allocator can hand these blocks out again
    return out


def tile_starts(lengths, tile, at_least_one=False):
    """the n + 1 running tile counts of a list of lengths: ceil(length / tile) each, with at_least_one never fewer than one (an entry
    without work still owns a workgroup)"""
    floor = int(at_least_one)
    return [0] + list(itertools.accumulate(max(floor, (n + tile - 1) // tile) for n in lengths))


def table_words(rows, *starts):
    """rows (one list of int64 per entry) followed by the lists of tile starts, as one host int64 tensor: the caller's one small upload"""
    return torch.tensor([x for r in rows for x in r] + [x for st in starts for x in st], dtype=torch.int64)


def scene_sort(conf, pts, img, mask, lut):
    """The segmented stable confidence sort with its fused gathers (f3r_scene_sort, include/f3r.h).  Lists over segments of GPU tensors:
    conf (L,) fp32, pts (L, 3) fp32, img (3, L) fp32 planes, mask (L,) int8 or None; lut (256, 3) uint8 on the device.
    -> dict(order int32, pts, conf, rgb uint8, conf_rgb uint8, mask int8: concatenated over segments; offsets: the segments' first slots;
    stats (S, 4) int32 bit patterns of the uint32 words)."""
    S = len(conf)
    if S < 1 or len(pts) != S or len(img) != S or len(mask) != S:
        raise ValueError("scene_sort: need one conf, pts, img and mask entry per segment, and at least one segment")
    dev = conf[0].device
    require_gpu(lut, "lut")
    if lut.dtype != torch.uint8 or lut.numel() != 768:
        raise ValueError("scene_sort: lut must be 256 x 3 uint8")
    rows, lengths, keep, off = [], [], [lut.contiguous()], 0
    f32, i8 = torch.float32, torch.int8
    for s in range(S):
        c, p, g, m = conf[s], pts[s], img[s], mask[s]
        L = c.numel()
        for t in (c, p, g, m):
            if t is not None and not t.is_cuda:
                require_gpu(t, f"segment {s}")
        if (c.dtype != f32 or p.dtype != f32 or g.dtype != f32 or c.dim() != 1 or p.shape != (L, 3) or g.shape != (3, L)
                or p.device != dev or g.device != dev or c.device != dev):
            raise ValueError(f"scene_sort: segment {s}: conf (L,), pts (L, 3), img (3, L), all fp32 on {dev}; got {tuple(c.shape)} {c.dtype}, "
                             f"{tuple(p.shape)} {p.dtype}, {tuple(g.shape)} {g.dtype}")
        if m is not None and (m.dtype != i8 or m.shape != (L,) or m.device != dev):
            raise ValueError(f"scene_sort: segment {s}: mask must be ({L},) int8 on {dev}, got {tuple(m.shape)} {m.dtype} on {m.device}")
        if not 1 <= L < 2 ** 31:
            raise ValueError(f"scene_sort: segment {s} has {L} keys; need 1 <= L < 2^31")
        c, p, g = c.contiguous(), p.contiguous(), g.contiguous()
        m = None if m is None else m.contiguous()
        keep += [c, p, g, m]
        rows.append([c.data_ptr(), p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), L, off])
        lengths.append(L)
        off += L
    total = off
    starts = tile_starts(lengths, _lib.SCENE_TILE)
    table, n_tiles = table_words(rows, starts).to(dev), starts[-1]
    l = _lib.lib()
    ws_bytes = l.f3r_scene_sort_workspace_bytes(total, n_tiles)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = {"order": torch.empty(total, dtype=torch.int32, device=dev), "pts": torch.empty((total, 3), dtype=torch.float32, device=dev),
           "conf": torch.empty(total, dtype=torch.float32, device=dev), "rgb": torch.empty((total, 3), dtype=torch.uint8, device=dev),
           "conf_rgb": torch.empty((total, 3), dtype=torch.uint8, device=dev), "mask": torch.empty(total, dtype=torch.int8, device=dev),
           "stats": torch.empty((S, 4), dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        check(l.f3r_scene_sort(ptr(table), S, n_tiles, total, ptr(keep[0]), ptr(ws), ws_bytes, ptr(out["order"]), ptr(out["pts"]), ptr(out["conf"]),
                               ptr(out["rgb"]), ptr(out["conf_rgb"]), ptr(out["mask"]), ptr(out["stats"]), stream_ptr()), "f3r_scene_sort")
    del keep, ws  # the launches are stream-ordered before the caching allocator can hand these blocks out again
    out["offsets"] = [r[5] for r in rows]
    return out


def scene_extent_stats(pts, ranks):
    """Order statistics `ranks` (four 0-based ranks in ascending order) of each axis of pts (M, 3) fp32 on the GPU (f3r_scene_extent).
    -> int32 (15,) on the device: 12 fp32 bit patterns [axis][rank], then the NaN count of each axis."""
    require_gpu(pts, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype != torch.float32 or not pts.is_contiguous() or pts.shape[0] < 1:
        raise ValueError(f"scene_extent_stats: pts must be a contiguous (M >= 1, 3) fp32 tensor, got {tuple(pts.shape)} {pts.dtype}")
    if len(ranks) != 4:
        raise ValueError("scene_extent_stats: four ranks")
    l = _lib.lib()
    ws_bytes = l.f3r_scene_extent_workspace_bytes()
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=pts.device)
    out = torch.empty(15, dtype=torch.int32, device=pts.device)
    rk = (ctypes.c_int64 * 4)(*[int(r) for r in ranks])
    with torch.cuda.device(pts.device):
        check(l.f3r_scene_extent(ptr(pts), pts.shape[0], rk, ptr(ws), ws_bytes, ptr(out), stream_ptr()), "f3r_scene_extent")
    return out


def scene_collect(pts, colors, masks, nums, const_colors):
    """The prefix cut and stable mask compaction of collect_points (f3r_scene_collect_count / _write).  Lists over segments: pts (L, 3) fp32
    sorted points, colors (L, 3) uint8 or None (then const_colors[s] = (r, g, b) is used), masks (L,) int8 or None (keep all), nums = how
    many entries to take from the front (1 <= num <= L).  -> (points (M, 3) fp32, colors (M, 3) uint8) on the device, or (None, None) when
    nothing is kept.  The host reads back one word: the total."""
    S = len(pts)
    if S < 1:
        return None, None
    dev = pts[0].device
    rows, keep = [], []
    for s in range(S):
        p, c, m, n = pts[s], colors[s], masks[s], int(nums[s])
        require_gpu(p, f"segment {s} pts")
        L = p.shape[0]
        if p.dim() != 2 or p.shape[1] != 3 or p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"scene_collect: segment {s}: pts must be contiguous (L, 3) fp32")
        if not 1 <= n <= L:
            raise ValueError(f"scene_collect: segment {s}: num = {n} outside [1, {L}]")
        if c is not None and (tuple(c.shape) != (L, 3) or c.dtype != torch.uint8 or not c.is_contiguous() or c.device != dev):
            raise ValueError(f"scene_collect: segment {s}: colors must be contiguous ({L}, 3) uint8 on {dev}")
        if m is not None and (tuple(m.shape) != (L,) or m.dtype != torch.int8 or not m.is_contiguous() or m.device != dev):
            raise ValueError(f"scene_collect: segment {s}: mask must be contiguous ({L},) int8 on {dev}")
        cc = (0, 0, 0) if const_colors[s] is None else const_colors[s]
        rows.append([p.data_ptr(), 0 if c is None else c.data_ptr(), 0 if m is None else m.data_ptr(), n,
                     int(cc[0]) | int(cc[1]) << 8 | int(cc[2]) << 16])
        keep += [p, c, m]
    starts = tile_starts([r[3] for r in rows], _lib.COLLECT_TILE)
    table, n_tiles = table_words(rows, starts).to(dev), starts[-1]
    l = _lib.lib()
    scan = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(l.f3r_scene_collect_count(ptr(table), S, n_tiles, ptr(scan), stream_ptr()), "f3r_scene_collect_count")
        total = int(scan[n_tiles].item()) & 0xffffffff
        if total == 0:
            return None, None
        out_p = torch.empty((total, 3), dtype=torch.float32, device=dev)
        out_c = torch.empty((total, 3), dtype=torch.uint8, device=dev)
        check(l.f3r_scene_collect_write(ptr(table), S, n_tiles, ptr(scan), ptr(out_p), ptr(out_c), stream_ptr()), "f3r_scene_collect_write")
    del keep
    return out_p, out_c


def ply_pack(points, colors_u8):
    """(M, 3) fp32 points and (M, 3) uint8 colours on the GPU -> uint8 device tensor of the 15 M record bytes (f3r_ply_pack)"""
    require_gpu(points, "points")
    require_gpu(colors_u8, "colors")
    n = points.shape[0]
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or tuple(colors_u8.shape) != (n, 3) or colors_u8.dtype != torch.uint8:
        raise ValueError(f"ply_pack: points (M, 3) fp32 and colors (M, 3) uint8, got {tuple(points.shape)} {points.dtype}, "
                         f"{tuple(colors_u8.shape)} {colors_u8.dtype}")
    points, colors_u8 = points.contiguous(), colors_u8.contiguous()
    out = torch.empty((n * 15 + 3) // 4, dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        check(_lib.lib().f3r_ply_pack(ptr(points), ptr(colors_u8), n, ptr(out), stream_ptr()), "f3r_ply_pack")
    return out.view(torch.uint8)[:n * 15]


def color_range(colors):
    """int64 (3,) on the device: the bit patterns of {key of the minimum, key of the maximum, NaN count} of a float32 / float64 GPU tensor
    (f3r_color_range; fast3r_amd/scene.py decodes the keys)"""
    require_gpu(colors, "colors")
    colors = colors.contiguous()
    out = torch.empty(3, dtype=torch.int64, device=colors.device)
    with torch.cuda.device(colors.device):
        check(_lib.lib().f3r_color_range(ptr(colors), colors.numel(), _real_id(colors.dtype), ptr(out), stream_ptr()), "f3r_color_range")
    return out


def color_to_u8(colors, rule, lo=0.0, hi=1.0):
    """safe_color_conversion's rule 0 / 1 / 2 in the tensor's own dtype (f3r_color_to_u8) -> uint8 tensor of the same shape"""
    require_gpu(colors, "colors")
    colors = colors.contiguous()
    out = torch.empty(colors.shape, dtype=torch.uint8, device=colors.device)
    with torch.cuda.device(colors.device):
        check(_lib.lib().f3r_color_to_u8(ptr(colors), colors.numel(), _real_id(colors.dtype), int(rule), float(lo), float(hi), ptr(out),
                                         stream_ptr()), "f3r_color_to_u8")
    return out


# ------------------------------------------------------------------------------------------------------------------- sky detection
def sky_row_words(W):
    """64-bit words per row of the bit-packed bitmap (include/f3r.h f3r_sky_detect)"""
    return (W + 63) // 64


def sky_detect(src, shapes, stages, *, want_not_sky=True, want_roots=False, want_bits=False):
    """f3r_sky_detect (include/f3r.h) on a list of views in one call.  src[i]: with F3R_SKY_CLASSIFY in `stages` the (3, H * W) fp32
    planes of view i, otherwise its (H, W) int8 bitmap, on the GPU; shapes[i] = (H, W).
    -> dict(not_sky: list of (H, W) int8, roots: list of (H, W) int32, stats: (V, 5) int32 on the device, bits: uint64 words as int64
    (V concatenated), word_offsets) with the entries that were asked for and that the stages produce."""
    V = len(src)
    if V < 1 or len(shapes) != V:
        raise ValueError(f"sky_detect: need one shape per view and at least one view (got {V} views, {len(shapes)} shapes)")
    classify, label = bool(stages & _lib.F3R_SKY_CLASSIFY), bool(stages & _lib.F3R_SKY_LABEL)
    dev = src[0].device
    keep, rows, hw, words = [], [], [], []
    word_off = pix_off = width_off = 0
    not_sky, roots = [], []
    for i, (t, (H, W)) in enumerate(zip(src, shapes)):
        H, W = int(H), int(W)
        if H < 1 or W < 1 or H * W >= 2 ** 31:
            raise ValueError(f"sky_detect: view {i} is {H} x {W}; need H, W >= 1 and H * W < 2^31")
        require_gpu(t, f"view {i}")
        want = ((3, H * W), torch.float32) if classify else ((H, W), torch.int8)
        if tuple(t.shape) != want[0] or t.dtype != want[1] or t.device != dev:
            raise ValueError(f"sky_detect: view {i} must be {want[0]} {want[1]} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        t = t.contiguous()
        keep.append(t)
        ns = torch.empty((H, W), dtype=torch.int8, device=dev) if (label and want_not_sky) else None
        rt = torch.empty((H, W), dtype=torch.int32, device=dev) if (label and want_roots) else None
        not_sky.append(ns)
        roots.append(rt)
        n_words = H * sky_row_words(W)
        # mask.size * 0.01 and int(height * 0.4) are Python doubles in the reference; an integer size exceeds the first iff it exceeds its floor
        rows.append([t.data_ptr(), 0 if ns is None else ns.data_ptr(), 0 if rt is None else rt.data_ptr(), H, W, word_off, pix_off, width_off,
                     int(math.floor(H * W * 0.01)), int(H * 0.4)])
        hw += [H, W]
        words.append(n_words)
        word_off += n_words
        pix_off += H * W
        width_off += W
    pix_starts, word_starts = tile_starts(words, _lib.SKY_PIX_TILE), tile_starts(words, _lib.SKY_WORD_TILE)
    table = table_words(rows, pix_starts, word_starts).to(dev)
    host_hw = (ctypes.c_int64 * len(hw))(*hw)
    l = _lib.lib()
    ws_bytes = l.f3r_sky_workspace_bytes(word_off, pix_off, width_off, stages)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stats = torch.empty((V, 5), dtype=torch.int32, device=dev) if label else None
    bits = torch.empty(word_off, dtype=torch.int64, device=dev) if (want_bits or not label) else None
    with torch.cuda.device(dev):
        check(l.f3r_sky_detect(ptr(table), host_hw, V, pix_starts[-1], word_starts[-1], word_off, pix_off, width_off, stages, ptr(ws), ws_bytes,
                               ptr(stats), ptr(bits), stream_ptr()), "f3r_sky_detect")
    del keep, ws, table  # the launches are stream-ordered before the caching allocator can hand these blocks out again
    return {"not_sky": not_sky, "roots": roots, "stats": stats, "bits": bits, "word_offsets": [r[5] for r in rows]}


# ------------------------------------------------------------------------------------------------------------------- mesh export
def mesh_index_id(index_dtype):
    if index_dtype == torch.int32:
        return _lib.F3R_INDEX_I32
    if index_dtype == torch.int64:
        return _lib.F3R_INDEX_I64
    raise ValueError(f"mesh: index_dtype must be torch.int32 or torch.int64, got {index_dtype}")


def _view_count(who, conf, pts, img, mask, shapes, ranks):
    V = len(pts)
    if V < 1 or not (len(conf) == len(img) == len(mask) == len(shapes) == len(ranks) == V):
        raise ValueError(f"{who}: need one conf, pts, img, mask, shape and rank entry per view, and at least one view")
    return V


def _view_rows(who, conf, pts, img, mask, shapes, ranks, pixel_bits=None):
    """The per-view checks of mesh_build and cloud_combine (who: the caller's name for the messages) and the rows of their device table
    (ViewRow, csrc/f3r_view_row.h), after _view_count.  pixel_bits: a view must have fewer than 2^pixel_bits pixels.  -> (rows, pixels
    per view, the contiguous tensors the rows point into, the total number of pixels)"""
    V = len(pts)
    dev = pts[0].device
    f32, u8 = torch.float32, torch.uint8
    rows, pix, keep, vbase = [], [], [], 0
    for i in range(V):
        H, W = int(shapes[i][0]), int(shapes[i][1])
        if H < 1 or W < 1 or (pixel_bits and H * W >= 2 ** pixel_bits):
            raise ValueError(f"{who}: view {i} is {H} x {W}; need H, W >= 1" + (f" and H * W < 2^{pixel_bits}" if pixel_bits else ""))
        n = H * W
        c, p, g, m = conf[i], pts[i], img[i], mask[i]
        for t in (c, p, g, m):
            if t is not None:
                require_gpu(t, f"view {i}")
                if t.device != dev:
                    raise ValueError(f"{who}: view {i}: tensors on {t.device} and {dev}")
        if p.dtype != f32 or tuple(p.shape) != (n, 3):
            raise ValueError(f"{who}: view {i}: pts must be ({n}, 3) fp32, got {tuple(p.shape)} {p.dtype}")
        if c is not None and (c.dtype != f32 or tuple(c.shape) != (n,)):
            raise ValueError(f"{who}: view {i}: conf must be ({n},) fp32, got {tuple(c.shape)} {c.dtype}")
        img_u8 = g.dtype == u8
        if not ((img_u8 and tuple(g.shape) == (n, 3)) or (g.dtype == f32 and tuple(g.shape) == (3, n))):
            raise ValueError(f"{who}: view {i}: img must be (3, {n}) fp32 planes or ({n}, 3) uint8, got {tuple(g.shape)} {g.dtype}")
        if m is not None and (m.dtype != u8 or tuple(m.shape) != (n,)):
            raise ValueError(f"{who}: view {i}: mask must be ({n},) uint8, got {tuple(m.shape)} {m.dtype}")
        c = None if c is None else c.contiguous()
        m = None if m is None else m.contiguous()
        p, g = p.contiguous(), g.contiguous()
        keep += [c, p, g, m]
        k_lo, k_hi, gamma = (0, 0, 0.0) if c is None else ranks[i]
        gamma_bits = int(np.asarray(gamma, dtype=np.float32).reshape(1).view(np.uint32)[0])
        rows.append([0 if c is None else c.data_ptr(), p.data_ptr(), g.data_ptr(), 0 if m is None else m.data_ptr(), H, W, vbase,
                     int(img_u8), int(k_lo), int(k_hi), gamma_bits, 0])
        pix.append(n)
        vbase += n
    return rows, pix, keep, vbase


def mesh_build(conf, pts, img, mask, shapes, ranks, *, double_sided=True, drop_unreferenced=False, flip_axes=False, index_dtype=torch.int64):
    """The triangle mesh of a list of views in one pass (f3r_mesh_threshold / _count / _write, include/f3r.h).  Lists over views of GPU
    tensors: conf (H W,) fp32 or None (validity is the mask alone), pts (H W, 3) fp32, img (3, H W) fp32 planes or (H W, 3) uint8 colours,
    mask (H W,) uint8 or None; shapes[i] = (H, W); ranks[i] = (k_lo, k_hi, gamma) as scene.percentile_indexes gives them (ignored without
    conf).  -> dict(vertices (Nv, 3) fp32, faces (F, 3) index_dtype, face_colors (F, 3) uint8 on the device; thresholds (V,) fp32 and
    nan_counts (V,) numpy, or None without any conf; counts (V, 3) int64 numpy: kept A, kept B, vertices per view).  The host reads back
    the per-view counts once, between the count and the write."""
    V = _view_count("mesh_build", conf, pts, img, mask, shapes, ranks)
    idx_id = mesh_index_id(index_dtype)
    rows, pix, keep, total = _view_rows("mesh_build", conf, pts, img, mask, shapes, ranks)
    dev = pts[0].device
    f32, u8 = torch.float32, torch.uint8
    hw = [x for r in rows for x in r[4:6]]
    quads = [(r[4] - 1) * (r[5] - 1) for r in rows]
    if total >= 2 ** 31:
        raise ValueError(f"mesh_build: {total} vertices; the indices are 32-bit: need fewer than 2^31 in all")
    tsv = tile_starts(pix, _lib.MESH_TILE)
    tsq = tile_starts(quads, _lib.MESH_TILE, at_least_one=True)   # a view of one row or column has no quads and still one tile
    nvt, nqt = tsv[-1], tsq[-1]
    table = table_words(rows, tsv, tsq).to(dev)
    host_hw = (ctypes.c_int64 * len(hw))(*hw)
    drop, ds, flip = int(bool(drop_unreferenced)), int(bool(double_sided)), int(bool(flip_axes))
    have_conf = any(c is not None for c in conf)
    l = _lib.lib()
    ws_bytes = l.f3r_mesh_workspace_bytes(nvt, nqt, total, drop)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    # one block: thresholds as fp32 bits, NaN counts, then the (V, 3) counts -- one readback
    small = torch.empty(V * 5, dtype=torch.int32, device=dev)
    thr, nans, counts = small[:V], small[V:2 * V], small[2 * V:]
    with torch.cuda.device(dev):
        if have_conf:
            check(l.f3r_mesh_threshold(ptr(table), V, ptr(thr), ptr(nans), stream_ptr()), "f3r_mesh_threshold")
        check(l.f3r_mesh_count(ptr(table), host_hw, V, nvt, nqt, total, ptr(thr) if have_conf else None, drop, ptr(ws), ws_bytes, ptr(counts),
                               stream_ptr()), "f3r_mesh_count")
        host = small.cpu().numpy()
        cnt = host[2 * V:].view(np.uint32).reshape(V, 3).astype(np.int64)
        n_faces = int((ds + 1) * (cnt[:, 0].sum() + cnt[:, 1].sum()))
        n_vert = int(cnt[:, 2].sum())
        vertices = torch.empty((n_vert, 3), dtype=f32, device=dev)
        faces = torch.empty((n_faces, 3), dtype=index_dtype, device=dev)
        colors = torch.empty((n_faces, 3), dtype=u8, device=dev)
        check(l.f3r_mesh_write(ptr(table), host_hw, V, nvt, nqt, total, ds, drop, flip, idx_id, ptr(ws), ws_bytes,
                               ptr(vertices) if n_vert else None, ptr(faces) if n_faces else None, ptr(colors) if n_faces else None,
                               stream_ptr()), "f3r_mesh_write")
    del keep, ws, table  # the launches are stream-ordered before the caching allocator can hand these blocks out again
    return {"vertices": vertices, "faces": faces, "face_colors": colors, "counts": cnt,
            "thresholds": host[:V].view(np.float32).copy() if have_conf else None,
            "nan_counts": host[V:2 * V].view(np.uint32).copy() if have_conf else None}


def mesh_ply_pack(vertices, faces, face_colors):
    """(Nv, 3) fp32 vertices, (F, 3) int32 / int64 faces and (F, 3) uint8 face colours on the GPU -> uint8 device tensor of the 12 Nv + 16 F
    record bytes (f3r_mesh_ply_pack)"""
    for t, name in ((vertices, "vertices"), (faces, "faces"), (face_colors, "face_colors")):
        require_gpu(t, name)
    nv, nf = vertices.shape[0], faces.shape[0]
    if (vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or tuple(faces.shape) != (nf, 3)
            or tuple(face_colors.shape) != (nf, 3) or face_colors.dtype != torch.uint8):
        raise ValueError(f"mesh_ply_pack: vertices (Nv, 3) fp32, faces (F, 3) and face_colors (F, 3) uint8, got {tuple(vertices.shape)} "
                         f"{vertices.dtype}, {tuple(faces.shape)} {faces.dtype}, {tuple(face_colors.shape)} {face_colors.dtype}")
    idx_id = mesh_index_id(faces.dtype)
    if nv >= 2 ** 31:
        raise ValueError(f"mesh_ply_pack: {nv} vertices; the file's indices are 32-bit: need fewer than 2^31")
    vertices, faces, face_colors = vertices.contiguous(), faces.contiguous(), face_colors.contiguous()
    out = torch.empty(nv * 3 + nf * 4, dtype=torch.int32, device=vertices.device)
    with torch.cuda.device(vertices.device):
        check(_lib.lib().f3r_mesh_ply_pack(ptr(vertices) if nv else None, nv, ptr(faces) if nf else None, ptr(face_colors) if nf else None, nf,
                                           idx_id, ptr(out), stream_ptr()), "f3r_mesh_ply_pack")
    return out.view(torch.uint8)


# ------------------------------------------------------------------------------------------------------------------- point-cloud export
def cloud_combine(conf, pts, img, mask, shapes, ranks, *, flip_axes=False, thresholds=None, return_offsets=False):
    """The kept pixels of a list of views as one cloud (f3r_mesh_threshold, then f3r_cloud_combine_count / _write, include/f3r.h).  Lists
    over views of GPU tensors, as mesh_build takes them: conf (H W,) fp32 or None (no threshold test), pts (H W, 3) fp32, img (3, H W) fp32
    planes or (H W, 3) uint8 colours, mask (H W,) uint8 (nonzero = keep) or None; shapes[i] = (H, W); ranks[i] = (k_lo, k_hi, gamma) of
    scene.percentile_indexes (ignored without conf).  A pixel is kept iff conf > the view's threshold and its mask byte is nonzero.
    thresholds: a (V,) fp32 device tensor to use instead of computing them.  -> (points (M, 3) fp32, colors (M, 3) uint8) on the device
    in view order then pixel order, or (None, None) when nothing is kept.  The host reads back one word: the total.  With return_offsets a
    third entry follows: the V end offsets of the views in the cloud (ascending Python ints, read from the tile scan: V words read back
    instead of one)."""
    V = _view_count("cloud_combine", conf, pts, img, mask, shapes, ranks)
    count, write = _lib.entry("f3r_cloud_combine_count"), _lib.entry("f3r_cloud_combine_write")
    rows, pix, keep, _ = _view_rows("cloud_combine", conf, pts, img, mask, shapes, ranks, pixel_bits=31)
    dev = pts[0].device
    f32, u8 = torch.float32, torch.uint8
    starts = tile_starts(pix, _lib.CLOUD_TILE)
    n_tiles = starts[-1]
    if n_tiles >= 2 ** 31:
        raise ValueError(f"cloud_combine: {n_tiles} tiles; need fewer than 2^31")
    table = table_words(rows, starts).to(dev)
    have_conf = any(c is not None for c in conf)
    if thresholds is not None:
        require_gpu(thresholds, "thresholds")
        if thresholds.dtype != f32 or tuple(thresholds.shape) != (V,) or thresholds.device != dev:
            raise ValueError(f"cloud_combine: thresholds must be ({V},) fp32 on {dev}, got {tuple(thresholds.shape)} {thresholds.dtype}")
        thr = thresholds.contiguous()
    else:
        small = torch.empty(2 * V, dtype=torch.int32, device=dev)
        thr = small[:V].view(f32)
    scan = torch.empty(n_tiles + 1, dtype=torch.int32, device=dev)
    l = _lib.lib()
    with torch.cuda.device(dev):
        if have_conf and thresholds is None:
            check(l.f3r_mesh_threshold(ptr(table), V, ptr(thr), ptr(small[V:]), stream_ptr()), "f3r_mesh_threshold")
        thr_ptr = ptr(thr) if have_conf else None
        check(count(ptr(table), V, n_tiles, thr_ptr, ptr(scan), stream_ptr()), "f3r_cloud_combine_count")
        if return_offsets:  # the scan at a view's first tile is the view's first slot: the next view's is its end
            ends = [int(e) & 0xffffffff for e in scan[torch.tensor(starts[1:], device=dev)].tolist()]
            total = ends[-1]
        else:
            total = int(scan[n_tiles].item()) & 0xffffffff
        if total == 0:
            return (None, None, ends) if return_offsets else (None, None)
        out_p = torch.empty((total, 3), dtype=f32, device=dev)
        out_c = torch.empty((total, 3), dtype=u8, device=dev)
        check(write(ptr(table), V, n_tiles, thr_ptr, ptr(scan), int(bool(flip_axes)), ptr(out_p), ptr(out_c), stream_ptr()),
              "f3r_cloud_combine_write")
    del keep, table  # the launches are stream-ordered before the caching allocator can hand these blocks out again
    return (out_p, out_c, ends) if return_offsets else (out_p, out_c)


def _cloud_points(points, who, colors=None, bits=31):
    """the (n, 3) fp32 cloud and its optional (n, 3) uint8 colours, contiguous, and n < 2^bits (31: the exporters, 32: the renderer)"""
    require_gpu(points, "points")
    n = points.shape[0] if points.dim() == 2 else -1
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32 or not 1 <= n < 2 ** bits:
        raise ValueError(f"{who}: points must be (1 <= n < 2^{bits}, 3) fp32, got {tuple(points.shape)} {points.dtype}")
    if colors is not None:
        require_gpu(colors, "colors")
        if tuple(colors.shape) != (n, 3) or colors.dtype != torch.uint8 or colors.device != points.device:
            raise ValueError(f"{who}: colors must be ({n}, 3) uint8 on {points.device}, got {tuple(colors.shape)} {colors.dtype} on {colors.device}")
        colors = colors.contiguous()
    return points.contiguous(), colors, n


def _float_of_key(k):
    k = int(k) & 0xffffffff
    u = (k & 0x7fffffff) if k & 0x80000000 else (~k) & 0xffffffff
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])


def cloud_bounds(points):
    """(min (3,), max (3,)) as Python floats over the finite coordinates, and the count of non-finite ones (f3r_cloud_bounds): one
    readback of eight words"""
    fn = _lib.entry("f3r_cloud_bounds")
    points, _, n = _cloud_points(points, "cloud_bounds")
    out = torch.empty(8, dtype=torch.int32, device=points.device)
    with torch.cuda.device(points.device):
        check(fn(ptr(points), n, ptr(out), stream_ptr()), "f3r_cloud_bounds")
    w = out.cpu().tolist()
    return [_float_of_key(k) for k in w[:3]], [_float_of_key(k) for k in w[3:6]], int(w[6]) & 0xffffffff


def heuristic_voxel_size(min_bound, max_bound, max_num_points):
    """the notebook's voxel size for a target count: the cube root of the bounding box's volume per point, as Python floats"""
    extent = [float(hi) - float(lo) for lo, hi in zip(min_bound, max_bound)]
    return (extent[0] * extent[1] * extent[2] / max_num_points) ** (1 / 3)


def voxel_key_bits(min_bound, max_bound, voxel_size):
    """Bits of the voxel key per axis: ceil(log2(c_a)) for c_a = floor(extent_a / voxel_size + 0.5) + 1 cells -- and never fewer cells than
    the largest index the kernel's own expression floor((max_a - (min_a - 0.5 voxel_size)) / voxel_size) reaches, which rounding can put one
    past that count.  ValueError when an axis needs more than 31 bits or the key more than 63."""
    voxel_size = float(voxel_size)
    if not (voxel_size > 0.0 and math.isfinite(voxel_size)):
        raise ValueError(f"voxel_size = {voxel_size}; need a finite value > 0")
    bits = []
    for lo, hi in zip(min_bound, max_bound):
        lo, hi = float(lo), float(hi)
        cells = (hi - lo) / voxel_size + 0.5
        top = (hi - (lo - 0.5 * voxel_size)) / voxel_size
        if not (math.isfinite(cells) and math.isfinite(top)):
            raise ValueError(f"voxel_size too small for this extent ({voxel_size} for {hi - lo})")
        c = max(math.floor(cells) + 1, math.floor(top) + 1)
        bits.append((c - 1).bit_length())
    if max(bits) > 31 or sum(bits) > 63:
        raise ValueError(f"voxel_size too small for this extent: {bits} key bits per axis; at most 31 each and 63 in all")
    return bits


def voxel_sort_passes(bits):
    """8-bit LSD passes over a key of that many bits"""
    return (sum(bits) + 7) // 8


def cloud_voxel_down_sample(points, colors, voxel_size, bounds=None):
    """Open3D's VoxelDownSample in a fixed order (f3r_cloud_voxel_sort / _sums, include/f3r.h).  points (n, 3) fp32, colors (n, 3) uint8 or
    None, on the GPU; bounds: what cloud_bounds(points) returned, if the caller has it.  -> dict(points (M, 3) fp32, colors (M, 3) uint8 or
    None, counts (M,) int32: voxels in ascending key order; bits: key bits per axis; passes: sort passes run).  ValueError on a NaN or inf
    coordinate, voxel_size <= 0 and a key of more than 63 bits.  The host reads back the bounds and one word: the voxel count."""
    sort, sums, sizer = _lib.entry("f3r_cloud_voxel_sort"), _lib.entry("f3r_cloud_voxel_sums"), _lib.entry("f3r_cloud_voxel_workspace_bytes")
    points, colors, n = _cloud_points(points, "cloud_voxel_down_sample", colors)
    lo, hi, bad = cloud_bounds(points) if bounds is None else bounds
    if bad:
        raise ValueError(f"cloud_voxel_down_sample: {bad} coordinates are NaN or inf")
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError(f"cloud_voxel_down_sample: voxel_size = {voxel_size}; need > 0")
    bits = voxel_key_bits(lo, hi, voxel_size)
    dev = points.device
    ws_bytes = sizer(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    n_vox = torch.empty(1, dtype=torch.int32, device=dev)
    mb, cb = (ctypes.c_double * 3)(*lo), (ctypes.c_int * 3)(*bits)
    with torch.cuda.device(dev):
        check(sort(ptr(points), n, mb, voxel_size, cb, ptr(ws), ws_bytes, ptr(n_vox), stream_ptr()), "f3r_cloud_voxel_sort")
        m = int(n_vox.item()) & 0xffffffff
        out_p = torch.empty((m, 3), dtype=torch.float32, device=dev)
        out_c = None if colors is None else torch.empty((m, 3), dtype=torch.uint8, device=dev)
        counts = torch.empty(m, dtype=torch.int32, device=dev)
        check(sums(ptr(points), ptr(colors), n, m, ptr(ws), ws_bytes, ptr(out_p), ptr(out_c), ptr(counts), stream_ptr()), "f3r_cloud_voxel_sums")
    del ws  # the launches are stream-ordered before the caching allocator can hand this block out again
    return {"points": out_p, "colors": out_c, "counts": counts, "bits": bits, "passes": voxel_sort_passes(bits)}


def cloud_fps(points, num_samples, start_index=0, mode=_lib.F3R_FPS_AUTO):
    """Open3D's FarthestPointDownSample (f3r_cloud_fps, include/f3r.h): points (n, 3) fp32 on the GPU, finite (the caller's check:
    cloud_bounds counts) -> selected int32 (num_samples,) in selection order.  mode: F3R_FPS_AUTO, F3R_FPS_ONE (one workgroup, n <=
    CLOUD_FPS_ONE_MAX) or F3R_FPS_TILED (one launch per sample).  O(n num_samples), as the reference's."""
    fn, sizer = _lib.entry("f3r_cloud_fps"), _lib.entry("f3r_cloud_fps_workspace_bytes")
    points, _, n = _cloud_points(points, "cloud_fps")
    num_samples, start_index, mode = int(num_samples), int(start_index), int(mode)
    if not 1 <= num_samples <= n:
        raise ValueError(f"cloud_fps: num_samples = {num_samples} outside [1, {n}]")
    if not 0 <= start_index < n:
        raise ValueError(f"cloud_fps: start_index = {start_index} outside [0, {n})")
    if mode not in (_lib.F3R_FPS_AUTO, _lib.F3R_FPS_ONE, _lib.F3R_FPS_TILED) or (mode == _lib.F3R_FPS_ONE and n > _lib.CLOUD_FPS_ONE_MAX):
        raise ValueError(f"cloud_fps: mode = {mode} for n = {n}; F3R_FPS_ONE takes n <= {_lib.CLOUD_FPS_ONE_MAX}")
    dev = points.device
    tiled = mode == _lib.F3R_FPS_TILED or (mode == _lib.F3R_FPS_AUTO and n > _lib.CLOUD_FPS_ONE_MAX)
    ws_bytes = sizer(n) if tiled else 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev) if tiled else None
    selected = torch.empty(num_samples, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(fn(ptr(points), n, num_samples, start_index, mode, ptr(ws), ws_bytes, ptr(selected), stream_ptr()), "f3r_cloud_fps")
    del ws  # the launches are stream-ordered before the caching allocator can hand this block out again
    return selected


def cloud_mark(selected, n):
    """uint8 (n,) on the device: 1 at every index in selected (int32, every entry in [0, n)), 0 elsewhere (f3r_cloud_mark)"""
    require_gpu(selected, "selected")
    k, n = selected.numel(), int(n)
    if selected.dim() != 1 or selected.dtype != torch.int32 or not 1 <= k <= n < 2 ** 31:
        raise ValueError(f"cloud_mark: selected must be int32 (1 <= k <= n = {n} < 2^31,), got {tuple(selected.shape)} {selected.dtype}")
    fn = _lib.entry("f3r_cloud_mark")
    selected = selected.contiguous()
    mask = torch.empty(n, dtype=torch.uint8, device=selected.device)
    with torch.cuda.device(selected.device):
        check(fn(ptr(selected), k, n, ptr(mask), stream_ptr()), "f3r_cloud_mark")
    return mask


def cloud_gather(points, colors, index):
    """(points[index], colors[index]) in the order of index (int32 or int64, every entry in [0, n): the caller's contract) (f3r_cloud_gather);
    colors may be None"""
    points, colors, n = _cloud_points(points, "cloud_gather", colors)
    require_gpu(index, "index")
    m = index.numel()
    if index.dim() != 1 or index.dtype not in (torch.int32, torch.int64) or index.device != points.device or not 1 <= m < 2 ** 31:
        raise ValueError(f"cloud_gather: index must be int32 or int64 (1 <= m < 2^31,) on {points.device}, got {tuple(index.shape)} {index.dtype}")
    fn = _lib.entry("f3r_cloud_gather")
    index = index.contiguous()
    out_p = torch.empty((m, 3), dtype=torch.float32, device=points.device)
    out_c = None if colors is None else torch.empty((m, 3), dtype=torch.uint8, device=points.device)
    with torch.cuda.device(points.device):
        check(fn(ptr(points), ptr(colors), ptr(index), int(index.dtype == torch.int64), n, m, ptr(out_p), ptr(out_c), stream_ptr()),
              "f3r_cloud_gather")
    return out_p, out_c


# ------------------------------------------------------------------------------------------------------------------- point-splat renderer
def _render_viewport(width, height, who):
    width, height = int(width), int(height)
    if width < 1 or height < 1 or width * height >= 2 ** 31:
        raise ValueError(f"{who}: viewport {width} x {height}; need width, height >= 1 and width * height < 2^31")
    return width, height


def _keys_ok(keys, device):
    return keys.dim() == 2 and keys.dtype == torch.int64 and keys.is_contiguous() and keys.device == device


def _render_keys(keys, device, who):
    """`keys` as render_keys made it, on `device` -> (width, height)"""
    if not _keys_ok(keys, device):
        raise ValueError(f"{who}: keys must be a contiguous (height, width) int64 tensor on {device}, got {tuple(keys.shape)} "
                         f"{keys.dtype} on {keys.device}")
    height, width = keys.shape
    return _render_viewport(width, height, who)


def _camera(camera, who):
    """the 17 doubles of include/f3r.h (V row-major, sx, sy, cx, cy, znear) as a C array"""
    cam = [float(c) for c in camera]
    if len(cam) != 17:
        raise ValueError(f"{who}: camera must hold 17 numbers (V, sx, sy, cx, cy, znear), got {len(cam)}")
    return (ctypes.c_double * 17)(*cam)


def render_keys(width, height, device):
    """A cleared key buffer (f3r_render_clear): int64 (height, width) on `device`, every word all ones -- no point anywhere"""
    fn = _lib.entry("f3r_render_clear")
    width, height = _render_viewport(width, height, "render_keys")
    keys = torch.empty((height, width), dtype=torch.int64, device=device)
    require_gpu(keys, "keys")
    with torch.cuda.device(keys.device):
        check(fn(ptr(keys), width, height, stream_ptr()), "f3r_render_clear")
    return keys


def render_splat(points, n0, n1, camera, point_size, keys):
    """Points [n0, n1) of the cloud (n, 3) fp32 go into `keys` (what render_keys returned; written in place) through `camera`, the 17
    doubles of include/f3r.h (V row-major, sx, sy, cx, cy, znear) (f3r_render_splat).  Calls accumulate."""
    fn = _lib.entry("f3r_render_splat")
    points, _, n = _cloud_points(points, "render_splat", bits=32)
    require_gpu(keys, "keys")
    width, height = _render_keys(keys, points.device, "render_splat")
    cam = _camera(camera, "render_splat")
    with torch.cuda.device(points.device):
        check(fn(ptr(points), n, int(n0), int(n1), cam, float(point_size), width, height, ptr(keys),
                 stream_ptr()), "f3r_render_splat")


def render_resolve(keys, colors, background=(255, 255, 255), *, return_depth=False):
    """keys (height, width) int64 and the cloud's colours (n, 3) uint8 -> the (height, width, 3) uint8 picture, row 0 at the top, and with
    return_depth the (height, width) fp32 depth, +inf where no point landed (f3r_render_resolve)"""
    fn = _lib.entry("f3r_render_resolve")
    require_gpu(keys, "keys")
    require_gpu(colors, "colors")
    n = colors.shape[0] if colors.dim() == 2 else -1
    if (not _keys_ok(keys, keys.device) or colors.dim() != 2 or colors.shape[1] != 3
            or colors.dtype != torch.uint8 or colors.device != keys.device or not 1 <= n < 2 ** 32):
        raise ValueError(f"render_resolve: keys contiguous (height, width) int64 and colors (1 <= n < 2^32, 3) uint8 on one device, got "
                         f"{tuple(keys.shape)} {keys.dtype} on {keys.device}, {tuple(colors.shape)} {colors.dtype} on {colors.device}")
    bg = [int(b) for b in background]
    if len(bg) != 3 or any(not 0 <= b <= 255 for b in bg):
        raise ValueError(f"render_resolve: background = {background!r}; need three values in [0, 255]")
    height, width = keys.shape
    _render_viewport(width, height, "render_resolve")
    colors = colors.contiguous()
    image = torch.empty((height, width, 3), dtype=torch.uint8, device=keys.device)
    depth = torch.empty((height, width), dtype=torch.float32, device=keys.device) if return_depth else None
    with torch.cuda.device(keys.device):
        check(fn(ptr(keys), ptr(colors), n, width, height, bg[0] | bg[1] << 8 | bg[2] << 16, ptr(image), ptr(depth), stream_ptr()),
              "f3r_render_resolve")
    return (image, depth) if return_depth else image


def render_center(points):
    """The mean of the cloud's coordinates as three Python floats: the fp64 sums of f3r_render_center (a fixed order: two runs give the same
    bits), each divided by n on the host.  One readback of three doubles."""
    fn = _lib.entry("f3r_render_center")
    points, _, n = _cloud_points(points, "render_center", bits=32)
    buf = torch.empty((_lib.RENDER_CENTER_PARTS + 1) * 3, dtype=torch.float64, device=points.device)
    with torch.cuda.device(points.device):
        check(fn(ptr(points), n, ptr(buf[3:]), ptr(buf), stream_ptr()), "f3r_render_center")
    return [s / n for s in buf[:3].tolist()]


# ------------------------------------------------------------------------------------------------------------------- triangle rasteriser
RASTER_FACES_PER_LAUNCH = 1 << 24  # faces of one launch pair of f3r_raster_triangles: a 64 MB queue, whatever the mesh
_raster_workspaces = {}  # (device index, stream, bytes) -> the int64 workspace tensor; launches on one stream run in order, so one serves every call on it


def raster_workspace(device, faces_per_launch):
    """The workspace of f3r_raster_triangles for launches of `faces_per_launch` faces on `device`, cached per device, current stream and size.  After a
    call, word 0 holds the last launch's queue length (its low 32 bits) and word 1 the queue length over all launches of the call."""
    sizer = _lib.entry("f3r_raster_workspace_bytes")
    faces_per_launch = int(faces_per_launch)
    nbytes = sizer(faces_per_launch) if 1 <= faces_per_launch < 2 ** 31 else 0
    if nbytes == 0:
        raise ValueError(f"raster_triangles: faces_per_launch = {faces_per_launch}; need 1 <= faces_per_launch < 2^31")
    device = torch.device(device)
    index = device.index if device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(index):
        key = (index, stream_ptr(), nbytes)   # per stream: calls on two streams of one device must not share the queue and its counter
    if key not in _raster_workspaces:
        _raster_workspaces[key] = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=device)
    return _raster_workspaces[key], nbytes


def raster_triangles(vertices, faces, camera, keys, *, f0=0, f1=None, index_base=0, faces_per_launch=RASTER_FACES_PER_LAUNCH):
    """Triangles [f0, f1) of the mesh (vertices (nv, 3) fp32, faces (nf, 3) int32 or int64) go into `keys` (what render_keys returned;
    written in place) through `camera`, the 17 doubles of include/f3r.h, as keys (fp32 depth << 32) | (index_base + f)
    (f3r_raster_triangles).  Calls accumulate, with each other and with render_splat.  f1 = None: nf."""
    fn = _lib.entry("f3r_raster_triangles")
    require_gpu(vertices, "vertices")
    require_gpu(faces, "faces")
    require_gpu(keys, "keys")
    nv = vertices.shape[0] if vertices.dim() == 2 else -1
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.dtype != torch.float32 or nv < 1:
        raise ValueError(f"raster_triangles: vertices must be (nv >= 1, 3) fp32, got {tuple(vertices.shape)} {vertices.dtype}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype not in (torch.int32, torch.int64) or faces.device != vertices.device:
        raise ValueError(f"raster_triangles: faces must be (nf, 3) int32 or int64 on {vertices.device}, got {tuple(faces.shape)} {faces.dtype} "
                         f"on {faces.device}")
    width, height = _render_keys(keys, vertices.device, "raster_triangles")
    nf = faces.shape[0]
    f1 = nf if f1 is None else int(f1)
    cam = _camera(camera, "raster_triangles")
    if nf == 0 and int(f0) == 0 and f1 == 0:
        return
    vertices, faces = vertices.contiguous(), faces.contiguous()
    ws, nbytes = raster_workspace(vertices.device, faces_per_launch)
    with torch.cuda.device(vertices.device):
        check(fn(ptr(vertices), nv, ptr(faces), mesh_index_id(faces.dtype), nf, int(f0), f1, int(index_base), cam,
                 width, height, ptr(keys), ptr(ws), nbytes, int(faces_per_launch), stream_ptr()), "f3r_raster_triangles")


# ------------------------------------------------------------------------------------------------------------------- map pictures
def _map_source(t):
    """a (H, W) fp32 view as (tensor to keep alive, element stride): read where it lies when its elements are evenly spaced in row-major
    order -- a dense map, or one channel of an (H, W, C) tensor -- and from a dense copy otherwise"""
    H, W = t.shape
    step = t.stride(1) if W > 1 else (t.stride(0) if H > 1 else 1)
    if step < 1 or (W > 1 and H > 1 and t.stride(0) != W * step):
        return t.contiguous(), 1
    return t, step


def maps_table(srcs, dsts, mode=_lib.F3R_MAPS_LUT):
    """The checked per-map table of f3r_maps_colorize for lists of sources and destinations (as `maps_colorize` takes them): -> dict(table:
    the device words, host_rows: the rows for the argument checks, n, n_tiles, mode, device, keep: the tensors the table points into).
    One small upload."""
    n = len(srcs)
    if n < 1 or len(dsts) != n:
        raise ValueError(f"maps_colorize: need one destination per map and at least one map (got {n} maps, {len(dsts)} destinations)")
    if mode not in (_lib.F3R_MAPS_LUT, _lib.F3R_MAPS_RGB):
        raise ValueError(f"maps_colorize: unknown mode {mode}")
    rgb = mode == _lib.F3R_MAPS_RGB
    for i, t in enumerate(list(srcs) + list(dsts)):
        require_gpu(t, f"map {i % n}")
    dev = srcs[0].device
    rows, pixels, keep = [], [], []
    for i, (s, d) in enumerate(zip(srcs, dsts)):
        if s.dtype != torch.float32 or s.dim() != (3 if rgb else 2) or (rgb and s.shape[0] != 3) or s.device != dev:
            raise ValueError(f"maps_colorize: map {i} must be {'(3, H, W)' if rgb else '(H, W)'} fp32 on {dev}, got {tuple(s.shape)} {s.dtype} "
                             f"on {s.device}")
        H, W = (int(x) for x in s.shape[-2:])
        if H < 1 or W < 1 or H * W > 2 ** 30:
            raise ValueError(f"maps_colorize: map {i} is {H} x {W}; need H, W >= 1 and H * W <= 2^30")
        if d.dtype != torch.uint8 or tuple(d.shape) != (H, W, 4) or d.device != dev or d.stride(2) != 1 or d.stride(1) != 4:
            raise ValueError(f"maps_colorize: destination {i} must be ({H}, {W}, 4) uint8 on {dev} with dense pixels, got {tuple(d.shape)} "
                             f"{d.dtype} on {d.device}, strides {d.stride()}")
        pitch = d.stride(0) if H > 1 else 4 * W
        s, step = (s.contiguous(), 1) if rgb else _map_source(s)
        keep += [s, d]
        rows.append([s.data_ptr(), step, H, W, d.data_ptr(), pitch])
        pixels.append(H * W)
    starts = tile_starts(pixels, _lib.MAPS_TILE)
    host = table_words(rows, starts)
    return {"table": host.to(dev), "host_rows": (ctypes.c_int64 * (6 * n))(*host[:6 * n].tolist()), "n": n, "n_tiles": starts[-1], "mode": int(mode),
            "device": dev, "keep": keep}


def maps_launch(plan, lut=None):
    """f3r_maps_colorize on a table `maps_table` built: launches only.  -> the (n, 2) fp32 device ranges, or None for F3R_MAPS_RGB"""
    fn = _lib.entry("f3r_maps_colorize")
    n, dev, rgb = plan["n"], plan["device"], plan["mode"] == _lib.F3R_MAPS_RGB
    if not rgb:
        require_gpu(lut, "lut")
        if lut.dtype != torch.uint8 or lut.numel() != 768 or lut.device != dev or not lut.is_contiguous():
            raise ValueError(f"maps_colorize: lut must be a contiguous 256 x 3 uint8 tensor on {dev}")
    small = None if rgb else torch.empty((2, n, 2), dtype=torch.int32, device=dev)   # the keys, then the ranges
    with torch.cuda.device(dev):
        check(fn(ptr(plan["table"]), plan["host_rows"], n, plan["n_tiles"], plan["mode"], None if rgb else ptr(lut),
                 None if rgb else small[0].data_ptr(), None if rgb else small[1].data_ptr(), stream_ptr()), "f3r_maps_colorize")
    return None if rgb else small[1].view(torch.float32)


def maps_colorize(srcs, dsts, lut=None, *, mode=_lib.F3R_MAPS_LUT):
    """f3r_maps_colorize (include/f3r.h) on a list of maps in one call.  srcs[i]: with F3R_MAPS_LUT an (H, W) fp32 GPU tensor, which may be
    a view of one channel of an (H, W, C) tensor (read in place); with F3R_MAPS_RGB the (3, H, W) fp32 planes.  dsts[i]: the (H, W, 4)
    uint8 picture it lands in, which may be a window of a larger picture (its row stride is the pitch); written in place, only inside the
    window.  lut: (256, 3) uint8 on the device (F3R_MAPS_LUT).  -> the (n, 2) fp32 device tensor of (vmin, vmax) per map, or None for
    F3R_MAPS_RGB."""
    _lib.entry("f3r_maps_colorize")   # a library without it: say so before looking at a tensor
    plan = maps_table(srcs, dsts, mode)
    out = maps_launch(plan, lut)
    del plan  # the launches are stream-ordered before the caching allocator can hand the table and the copies out again
    return out


# ------------------------------------------------------------------------------------------------------------------- ground-truth views
def _gtview_geometry(window, resized, crop, who):
    """the checked ints of a launch group's geometry: window (x, y, w, h) in the frame, resized (w, h), crop (x, y, w, h) in the resized picture"""
    wx, wy, ww, wh = (int(v) for v in window)
    rw, rh = (int(v) for v in resized)
    cx, cy, cw, ch = (int(v) for v in crop)
    if min(wx, wy) < 0 or min(ww, wh) < 1 or max(wx + ww, wy + wh) > 2 ** 24:
        raise ValueError(f"{who}: window {window} is not a box of a frame")
    if min(rw, rh) < 1 or max(rw, rh) > 2 ** 24 or min(cx, cy) < 0 or min(cw, ch) < 1 or cx + cw > rw or cy + ch > rh:
        raise ValueError(f"{who}: crop {crop} leaves the resized {rw} x {rh} picture")
    return (wx, wy, ww, wh), (rw, rh), (cx, cy, cw, ch)


def _gtview_sources(frames, window, dtype, channels, who):
    """frames: per view a GPU tensor (H, W[, 3]) of `dtype` that contains the window, with dense pixels (rows may be pitched) -> (device
    int64 table [n][2] = pointer, row pitch in elements, the tensors it points into)"""
    wx, wy, ww, wh = window
    n = len(frames)
    if n < 1:
        raise ValueError(f"{who}: need at least one view")
    dev, keep, rows = frames[0].device, [], []
    for i, t in enumerate(frames):
        require_gpu(t, f"view {i}")
        want = 3 if channels else 2
        if t.dtype != dtype or t.dim() != want or (channels and t.shape[2] != channels) or t.device != dev:
            raise ValueError(f"{who}: view {i} must be (H, W{', 3' if channels else ''}) {dtype} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
        H, W = int(t.shape[0]), int(t.shape[1])
        if wx + ww > W or wy + wh > H:
            raise ValueError(f"{who}: view {i} is {H} x {W}; the window (x {wx}, y {wy}, {ww} x {wh}) leaves it")
        dense = t.stride(1) == (channels or 1) and (not channels or t.stride(2) == 1) and t.stride(0) >= W * (channels or 1)
        if not dense:
            t = t.contiguous()
        keep.append(t)
        rows.append([t.data_ptr(), t.stride(0)])
    return torch.tensor(rows, dtype=torch.int64).to(dev), keep


def gtview_resample(images, window, tables_h, tables_v, resized, crop, row_span, transpose=False):
    """f3r_gtview_resample (include/f3r.h) on one launch group.  images: per view an (H, W, 3) uint8 GPU tensor.  window: crop box 1 (x, y, w,
    h).  tables_h / tables_v: (ksize, bounds int32 (res, 2), kk int32 (res, ksize)) device tensors of the two passes, made for the window's
    size (`image.resample_tables`).  resized: (w, h).  crop: box 2 (x, y, w, h).  row_span: (first, end) of the window rows the kept output rows
    read (from the host copy of tables_v: the intermediate holds only those).  -> (img_u8 (n, h, w, 3) uint8, img (n, 3, h, w) fp32),
    h and w swapped when transpose."""
    fn, size_fn = _lib.entry("f3r_gtview_resample"), _lib.entry("f3r_gtview_workspace_bytes")
    window, resized, crop = _gtview_geometry(window, resized, crop, "gtview_resample")
    table, keep = _gtview_sources(images, window, torch.uint8, 3, "gtview_resample")
    dev, n = table.device, len(images)
    (kh, bh, wh_), (kv, bv, wv_) = tables_h, tables_v
    for name, (k, b, w), res in (("tables_h", (kh, bh, wh_), resized[0]), ("tables_v", (kv, bv, wv_), resized[1])):
        for t in (b, w):
            require_gpu(t, name)
        if b.dtype != torch.int32 or w.dtype != torch.int32 or tuple(b.shape) != (res, 2) or tuple(w.shape) != (res, int(k)) or not b.is_contiguous() \
                or not w.is_contiguous() or b.device != dev or w.device != dev:
            raise ValueError(f"gtview_resample: {name} must be (ksize, int32 ({res}, 2), int32 ({res}, ksize)) contiguous on {dev}")
    cx, cy, cw, ch = crop
    row0, row1 = (int(v) for v in row_span)
    if row0 < 0 or row1 > window[3] or row1 <= row0:
        raise ValueError(f"gtview_resample: row_span [{row0}, {row1}) is not a run of rows of a window of {window[3]} rows")
    rows = row1 - row0
    oh, ow = (cw, ch) if transpose else (ch, cw)
    img_u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
    img = torch.empty((n, 3, oh, ow), dtype=torch.float32, device=dev)
    nbytes = size_fn(n, rows, cw)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(fn(ptr(table), n, *window, ptr(bh), ptr(wh_), int(kh), resized[0], ptr(bv), ptr(wv_), int(kv), resized[1], row0, rows, cx, cy, cw, ch,
                 int(bool(transpose)), ptr(img_u8), ptr(img), ptr(ws), nbytes, stream_ptr()), "f3r_gtview_resample")
    del keep, ws  # the launches are stream-ordered before the caching allocator can hand these out again
    return img_u8, img


def gtview_unproject(depthmaps, cams, window, nearest, resized, crop, transpose=False, *, pose=True, finite_mask=True, want_points=True, flag=None):
    """f3r_gtview_unproject (include/f3r.h) on one launch group.  depthmaps: per view an (H, W) fp32 GPU tensor.  cams: (n, 25) fp32 device
    tensor, per view the intrinsics as returned (rows [1, 0, 2] when transpose) and the pose.  nearest: None (no resize) or (nx int32
    (res_w,), ny int32 (res_h,)) device tensors.  flag: None or a zeroed int32 device word, raised for a depth that is not finite.
    -> (depthmap (n, h, w) fp32, pts3d (n, h, w, 3) fp32 or None, valid_mask (n, h, w) bool or None), h and w swapped when transpose."""
    fn = _lib.entry("f3r_gtview_unproject")
    window, resized, crop = _gtview_geometry(window, resized, crop, "gtview_unproject")
    table, keep = _gtview_sources(depthmaps, window, torch.float32, 0, "gtview_unproject")
    dev, n = table.device, len(depthmaps)
    require_gpu(cams, "cams")
    if cams.dtype != torch.float32 or tuple(cams.shape) != (n, _lib.GTVIEW_CAM_WORDS) or not cams.is_contiguous() or cams.device != dev:
        raise ValueError(f"gtview_unproject: cams must be a contiguous ({n}, {_lib.GTVIEW_CAM_WORDS}) fp32 tensor on {dev}")
    nx = ny = None
    if nearest is not None:
        nx, ny = nearest
        for name, t, res in (("nx", nx, resized[0]), ("ny", ny, resized[1])):
            require_gpu(t, name)
            if t.dtype != torch.int32 or tuple(t.shape) != (res,) or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"gtview_unproject: {name} must be a contiguous int32 ({res},) tensor on {dev}")
    elif resized != (window[2], window[3]):
        raise ValueError(f"gtview_unproject: without nearest tables the resized size {resized} must be the window's")
    if flag is not None:
        require_gpu(flag, "flag")
        if flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != dev:
            raise ValueError(f"gtview_unproject: flag must be one int32 word on {dev}")
    cx, cy, cw, ch = crop
    oh, ow = (cw, ch) if transpose else (ch, cw)
    depth = torch.empty((n, oh, ow), dtype=torch.float32, device=dev)
    pts = torch.empty((n, oh, ow, 3), dtype=torch.float32, device=dev) if want_points else None
    valid = torch.empty((n, oh, ow), dtype=torch.uint8, device=dev) if want_points else None
    flags = (_lib.F3R_GTVIEW_POSE if pose else 0) | (_lib.F3R_GTVIEW_FINITE_MASK if finite_mask else 0)
    with torch.cuda.device(dev):
        check(fn(ptr(table), ptr(cams), n, *window, ptr(nx), ptr(ny), resized[0], resized[1], cx, cy, cw, ch, int(bool(transpose)), flags, ptr(depth),
                 ptr(pts), ptr(valid), ptr(flag), stream_ptr()), "f3r_gtview_unproject")
    del keep
    return depth, pts, None if valid is None else valid.view(torch.bool)


# ------------------------------------------------------------------------------------------------------------------- multi-view depth metrics
def depth_plan(gt, pred, conf=None, mask=None, *, n_bins=0):
    """The table of the depth-metric entry points (include/f3r.h) and the result rows they fill.  Lists over segments of GPU tensors: gt fp32
    of n elements; pred fp32 of n elements (a depth map) or of shape (..., 3) with 3 n elements (a pointmap: channel 2 is read in place);
    conf fp32 of n elements or None; mask bool or uint8 of n elements or None (conf and mask may be None as a whole).  Nothing is stacked:
    a tensor that is not contiguous is made so first.  n_bins > 0 leaves room for the curves.  -> dict(table, host, n_seg, n_tiles, total,
    lengths, out fp64 (n_seg, 16 + 2 n_bins), keep)."""
    S = len(gt)
    conf = [None] * S if conf is None else conf
    mask = [None] * S if mask is None else mask
    if S < 1 or len(pred) != S or len(conf) != S or len(mask) != S:
        raise ValueError("depth_plan: need one gt, pred, conf and mask entry per segment, and at least one segment")
    dev, keep, rows, lengths, base = gt[0].device, [], [], [], 0
    for s in range(S):
        g, p, c, m = gt[s], pred[s], conf[s], mask[s]
        for t in (g, p, c, m):
            if t is not None:
                require_gpu(t, f"segment {s}")
                if t.device != dev:
                    raise ValueError(f"depth_plan: segment {s}: every tensor must be on {dev}, got {t.device}")
        n = g.numel()
        if g.dtype != torch.float32 or p.dtype != torch.float32 or not 1 <= n < 2 ** 31:
            raise ValueError(f"depth_plan: segment {s}: gt and pred must be fp32 with 1 <= n < 2^31 pixels, got {g.dtype}, {p.dtype}, n = {n}")
        if p.numel() == n:
            stride, chan = 1, 0
        elif p.dim() >= 1 and p.shape[-1] == 3 and p.numel() == 3 * n:
            stride, chan = 3, 2
        else:
            raise ValueError(f"depth_plan: segment {s}: pred {tuple(p.shape)} is neither a depth map nor a pointmap of gt's {n} pixels")
        if c is not None and (c.dtype != torch.float32 or c.numel() != n):
            raise ValueError(f"depth_plan: segment {s}: conf must be fp32 with {n} elements, got {tuple(c.shape)} {c.dtype}")
        if m is not None:
            if m.dtype not in (torch.bool, torch.uint8) or m.numel() != n:
                raise ValueError(f"depth_plan: segment {s}: mask must be bool or uint8 with {n} elements, got {tuple(m.shape)} {m.dtype}")
        g, p = g.contiguous(), p.contiguous()
        c = None if c is None else c.contiguous()
        m = None if m is None else m.contiguous()
        keep += [g, p, c, m]
        rows.append([g.data_ptr(), p.data_ptr(), stride, chan, 0 if c is None else c.data_ptr(), 0 if m is None else m.data_ptr(), n, base])
        lengths.append(n)
        base += n
    starts = tile_starts(lengths, _lib.DEPTH_TILE)
    words = table_words(rows, starts)
    host = (ctypes.c_int64 * words.numel())(*words.tolist())
    out = torch.empty((S, _lib.DEPTH_OUT_WORDS + 2 * int(n_bins)), dtype=torch.float64, device=dev)
    return {"table": words.to(dev), "host": host, "n_seg": S, "n_tiles": starts[-1], "total": base, "lengths": lengths, "out": out, "keep": keep,
            "n_bins": int(n_bins)}


def _depth_clip(clip):
    if clip is None:
        return 0, 0.0, 0.0
    lo, hi = (float(v) for v in clip)
    return 1, lo, hi


def depth_medians(plan, alignment=_lib.F3R_DEPTH_ALIGN_MEDIAN, q=None):
    """f3r_depth_medians on a plan: n_valid, thr, both medians and the scale into columns 0 .. 4 of plan["out"].  q: None (no threshold)
    or the quantile in [0, 1] of each segment's confidence below which a pixel is not valid."""
    fn = _lib.entry("f3r_depth_medians")
    out = plan["out"]
    with torch.cuda.device(out.device):
        check(fn(ptr(plan["table"]), plan["host"], plan["n_seg"], plan["n_tiles"], int(alignment), int(q is not None), 0.0 if q is None else float(q),
                 ptr(out), out.shape[1], stream_ptr()), "f3r_depth_medians")
    return out


def depth_errors(plan, thresholds=(1.03,), clip=None, use_thr=False):
    """f3r_depth_errors on a plan whose medians are taken: absrel, rmse, inlier percentages and counts into columns 5 .. 14 of plan["out"]."""
    fn, size_fn = _lib.entry("f3r_depth_errors"), _lib.entry("f3r_depth_workspace_bytes")
    out = plan["out"]
    tt, n_t = _thresholds(thresholds)
    on, lo, hi = _depth_clip(clip)
    nbytes = size_fn(plan["n_seg"], plan["n_tiles"], plan["total"], 0, 0)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=out.device)
    with torch.cuda.device(out.device):
        check(fn(ptr(plan["table"]), plan["host"], plan["n_seg"], plan["n_tiles"], int(bool(use_thr)), on, lo, hi, tt, n_t, ptr(ws), nbytes, ptr(out),
                 out.shape[1], stream_ptr()), "f3r_depth_errors")
    del ws  # the launches are stream-ordered before the caching allocator can hand the block out again
    return out


def depth_sparsify(plan, clip=None, use_thr=False, return_order=False):
    """f3r_depth_sparsify on a plan made with n_bins > 0 whose medians are taken: ause into column 15 of plan["out"], the sparsification and
    the oracle curve into the 2 n_bins columns after it.  With return_order also (order_conf, order_err, starts): int32 device tensors of the
    two orders as pixel indices inside their segments, segment s at [starts[s], starts[s + 1])."""
    fn, size_fn = _lib.entry("f3r_depth_sparsify"), _lib.entry("f3r_depth_workspace_bytes")
    out, K = plan["out"], plan["n_bins"]
    on, lo, hi = _depth_clip(clip)
    nbytes = size_fn(plan["n_seg"], plan["n_tiles"], plan["total"], 1, K)
    if nbytes == 0:
        raise ValueError(f"depth_sparsify: n_bins = {K} with {plan['total']} pixels is not a supported shape (1 <= n_bins <= 65536, fewer than 2^31 pixels)")
    dev = out.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    orders = torch.empty((2, plan["total"]), dtype=torch.int32, device=dev)
    starts = torch.empty(plan["n_seg"] + 1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(fn(ptr(plan["table"]), plan["host"], plan["n_seg"], plan["n_tiles"], int(bool(use_thr)), on, lo, hi, K, ptr(ws), nbytes, ptr(orders[0]),
                 ptr(orders[1]), ptr(starts), ptr(out), out.shape[1], stream_ptr()), "f3r_depth_sparsify")
    del ws
    return (out, orders[0], orders[1], starts) if return_order else out


# ------------------------------------------------------------------------------------------------------------------- view matching
def _host_i64(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int64).reshape(-1))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


def _host_i32(values):
    a = np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _table(host, dev):
    """the device copy of a host table (one word at least, so that an empty table still has an address)"""
    return torch.from_numpy(host if host.size else np.zeros(1, host.dtype)).to(dev)


def match_index_bytes(counts):
    """bytes of the index f3r_match_index builds over views of `counts` candidates (0: not a supported shape).  Needs no GPU."""
    seg, seg_p = _host_i64(np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]))
    return int(_lib.entry("f3r_match_index_bytes")(seg_p, len(counts)))


def match_index(points, counts):
    """f3r_match_index: one exact nearest-neighbour index per view.  points: fp32 (total, 3) on the GPU, the candidates of the views one
    after another; counts: candidates per view.  -> dict(index, seg, seg_host, n_views, counts, total).  Launches only."""
    fn, size_fn, ws_fn = _lib.entry("f3r_match_index"), _lib.entry("f3r_match_index_bytes"), _lib.entry("f3r_match_workspace_bytes")
    require_gpu(points, "points")
    counts = [int(c) for c in counts]
    V, total = len(counts), int(sum(counts))
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] != total or not points.is_contiguous():
        raise ValueError(f"match_index: points must be contiguous fp32 ({total}, 3), got {tuple(points.shape)} {points.dtype}")
    seg, seg_p = _host_i64(np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))]))
    nbytes, wbytes = size_fn(seg_p, V), ws_fn(total, V)
    if nbytes == 0 or wbytes == 0:
        raise ValueError(f"match_index: {V} views with {total} candidates is not a supported shape (1 .. 65536 views, fewer than 2^31 candidates "
                         "per view and 2^32 in all)")
    dev = points.device
    index = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(wbytes, dtype=torch.uint8, device=dev)
    seg_dev = _table(seg, dev)
    with torch.cuda.device(dev):
        check(fn(ptr(points) if total else None, ptr(seg_dev), seg_p, V, ptr(index), nbytes, ptr(ws), wbytes, stream_ptr()), "f3r_match_index")
    del ws  # the launches are stream-ordered before the caching allocator can hand the block out again
    return {"index": index, "seg": seg_dev, "seg_host": (seg, seg_p), "n_views": V, "counts": counts, "total": total, "points": points}


def match_search(ix, directed):
    """f3r_match_search on an index: directed = rows (a, b).  -> dict(directed, qoff (device and host), nn_idx int32 [Q], nn_dist fp64 [Q]):
    for candidate q of a, entry qoff[d] + q holds its nearest candidate of b (local to b) and the distance.  One launch."""
    fn = _lib.entry("f3r_match_search")
    dev, V = ix["index"].device, ix["n_views"]
    dh, dh_p = _host_i32(directed)
    D = dh.size // 2
    if dh.size != 2 * D or (D and (dh.min() < 0 or dh.max() >= V)):
        raise ValueError(f"match_search: directed pairs must be rows (a, b) of views 0 .. {V - 1}")
    qoff, qoff_p = _host_i64(np.concatenate([[0], np.cumsum(np.asarray([ix["counts"][a] for a in dh[0::2]], dtype=np.int64))]))
    Q = int(qoff[-1])
    d_dev, q_dev = _table(dh, dev), _table(qoff, dev)
    nn_idx = torch.empty(max(Q, 1), dtype=torch.int32, device=dev)
    nn_dist = torch.empty(max(Q, 1), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(fn(ptr(ix["index"]), ix["seg_host"][1], V, ptr(d_dev), dh_p, ptr(q_dev), qoff_p, D, ptr(nn_idx), ptr(nn_dist), stream_ptr()),
              "f3r_match_search")
    return {"directed": d_dev, "directed_host": (dh, dh_p), "qoff": q_dev, "qoff_host": (qoff, qoff_p), "n_directed": D, "n_queries": Q,
            "nn_idx": nn_idx[:Q], "nn_dist": nn_dist[:Q]}


def match_count(ix, found, pairs):
    """f3r_match_count: pairs = rows (i, j, directed row of i -> j, directed row of j -> i) over the rows of `found` (match_search).
    -> dict with offsets: device int64 [P + 2] = matches before each pair, the total, the index's flag word (views with a NaN / inf
    coordinate).  Launches only: the caller reads offsets back once."""
    fn = _lib.entry("f3r_match_count")
    dev, V, D = ix["index"].device, ix["n_views"], found["n_directed"]
    ph, ph_p = _host_i32(pairs)
    P = ph.size // 4
    if ph.size != 4 * P:
        raise ValueError("match_count: pairs must be rows (i, j, forward, backward)")
    tiles = [-(-ix["counts"][j] // _lib.MATCH_TILE) for j in ph[1::4]]
    toff, toff_p = _host_i64(np.concatenate([[0], np.cumsum(np.asarray(tiles, dtype=np.int64))]))
    p_dev, t_dev = _table(ph, dev), _table(toff, dev)
    tile_counts = torch.empty(int(toff[-1]) + 1, dtype=torch.int32, device=dev)
    offsets = torch.empty(P + 2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(fn(ptr(ix["index"]), ptr(ix["seg"]), ix["seg_host"][1], V, ptr(p_dev), ph_p, ptr(t_dev), toff_p, P, ptr(found["qoff"]),
                 found["qoff_host"][1], D, ptr(found["nn_idx"]) if found["n_queries"] else None, ptr(tile_counts), ptr(offsets), stream_ptr()),
              "f3r_match_count")
    return {"pairs": p_dev, "pairs_host": (ph, ph_p), "tile_off": t_dev, "tile_off_host": (toff, toff_p), "n_pairs": P, "tile_counts": tile_counts,
            "offsets": offsets}


def match_write(ix, found, counted, n_matches, pix, widths):
    """f3r_match_write after match_count: pix int32 [total] = every candidate's row-major pixel index in its view, widths int32 [V].
    -> (xy_i int32 [M, 2], xy_j int32 [M, 2], dist fp64 [M]) in pair order, ascending candidates of j inside a pair."""
    fn = _lib.entry("f3r_match_write")
    dev, V, M = ix["index"].device, ix["n_views"], int(n_matches)
    if pix.dtype != torch.int32 or pix.numel() != ix["total"] or widths.dtype != torch.int32 or widths.numel() != V:
        raise ValueError(f"match_write: pix must be int32 [{ix['total']}] and widths int32 [{V}]")
    xy_i = torch.empty((M, 2), dtype=torch.int32, device=dev)
    xy_j = torch.empty((M, 2), dtype=torch.int32, device=dev)
    dist = torch.empty(M, dtype=torch.float64, device=dev)
    if M:
        with torch.cuda.device(dev):
            check(fn(ptr(ix["seg"]), ix["seg_host"][1], V, ptr(counted["pairs"]), counted["pairs_host"][1], ptr(counted["tile_off"]),
                     counted["tile_off_host"][1], counted["n_pairs"], ptr(found["qoff"]), found["qoff_host"][1], found["n_directed"],
                     ptr(found["nn_idx"]), ptr(found["nn_dist"]), ptr(counted["tile_counts"]), ptr(pix.contiguous()), ptr(widths.contiguous()),
                     ptr(xy_i), ptr(xy_j), ptr(dist), M, stream_ptr()), "f3r_match_write")
    return xy_i, xy_j, dist


# ------------------------------------------------------------------------------------------------------------------- confidence cleaning
def clean_frame_id(frame):
    if frame == "world":
        return _lib.F3R_CLEAN_WORLD
    if frame == "camera":
        return _lib.F3R_CLEAN_CAMERA
    raise ValueError(f"clean_confidence: frame must be 'world' or 'camera', got {frame!r}")


def _shape_rows(shapes):
    """rows (H, W, first element) of views that lie one after another, and the total number of elements"""
    rows, off = [], 0
    for H, W in shapes:
        rows.append([int(H), int(W), off])
        off += int(H) * int(W)
    return rows, off


def clean_table(shapes, starts):
    """the host table of f3r_clean_confidence: rows (H, W, first element) of the views, then the starts of the neighbour lists"""
    rows, off = _shape_rows(shapes)
    return table_words(rows, [int(s) for s in starts]), off


def clean_confidence(pts, conf, depth, poses, intrinsics, shapes, starts, nbr, *, tol=0.001, max_bad_conf=0.0, frame="world"):
    """f3r_clean_confidence (include/f3r.h): the views one after another in pts (total, 3), conf and depth (total,), all fp32 on the GPU; poses
    (N, 4, 4) fp32 camera-to-world, intrinsics (N, 4) fp32 = fx, fy, cx, cy; shapes[i] = (H, W); starts (N + 1) and nbr: the neighbour lists
    (ascending, without the view itself).  -> (out_conf fp32 (total,), n_lowered int64 numpy (N,)).  Inputs are not written to.  One
    read-back: the counts and the flag word (ValueError on a pose without an inverse)."""
    fn, size_fn = _lib.entry("f3r_clean_confidence"), _lib.entry("f3r_clean_workspace_bytes")
    N = len(shapes)
    table_t, total = clean_table(shapes, starts)
    frame_id = clean_frame_id(frame)
    f32 = torch.float32
    for t, name, shape in ((pts, "pts", (total, 3)), (conf, "conf", (total,)), (depth, "depth", (total,)), (poses, "poses", (N, 4, 4)),
                           (intrinsics, "intrinsics", (N, 4))):
        require_gpu(t, name)
        if t.dtype != f32 or tuple(t.shape) != shape or t.device != pts.device or not t.is_contiguous():
            raise ValueError(f"clean_confidence: {name} must be contiguous fp32 {shape} on {pts.device}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    if len(starts) != N + 1:
        raise ValueError(f"clean_confidence: {len(starts)} neighbour-list starts for {N} views")
    dev = pts.device
    table = table_t.numpy()
    table_p = table.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    nh, nh_p = _host_i32(nbr)
    nbytes = size_fn(N)
    if nbytes == 0:
        raise ValueError(f"clean_confidence: {N} views is not a supported shape (at least one view)")
    t_dev, n_dev = _table(table, dev), _table(nh, dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(total, dtype=f32, device=dev)
    small = torch.empty(N + 1, dtype=torch.int32, device=dev)  # the counts, then the flag word: one read-back
    with torch.cuda.device(dev):
        check(fn(ptr(pts), ptr(conf), ptr(depth), ptr(poses), ptr(intrinsics), ptr(t_dev), table_p, N, ptr(n_dev), nh_p, nh.size, float(tol),
                 float(max_bad_conf), frame_id, ptr(out), ptr(small), small.data_ptr() + 4 * N, ptr(ws), nbytes, stream_ptr()), "f3r_clean_confidence")
        host = small.cpu().numpy()
    del ws, t_dev, n_dev  # the launches are stream-ordered before the caching allocator can hand these blocks out again
    if host[N] != 0:
        raise ValueError("clean_confidence: a camera pose has no inverse (its 3 x 3 block is singular, NaN or inf)")
    return out, host[:N].view(np.uint32).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- global alignment
def galign_dist_id(dist):
    if dist == "l1":
        return _lib.F3R_GALIGN_L1
    if dist == "l2":
        return _lib.F3R_GALIGN_L2
    raise ValueError(f"alignment_loss: dist must be 'l1' or 'l2', got {dist!r}")


def galign_tables(shapes, edges, maps, device=None):
    """The tables of f3r_galign_loss_grad, built once per problem.  shapes[v] = (H, W); edges: rows (i, j); maps[2 e + side] = (pointmap,
    weight map, H, W): contiguous fp32 device tensors (H, W, 3) and (H, W), or (address, address, H, W) when device is None (host checks
    only).  Edges may share a map: only its address is stored.  -> dict with the host arrays (kept alive for the calls), their device copies
    and the maps themselves."""
    N, E = len(shapes), len(edges)
    rows, off = _shape_rows(shapes)
    eh, eh_p = _host_i32([x for e in edges for x in e])
    lists = [[] for _ in range(N)]
    for o, v in enumerate(eh.tolist()):
        if 0 <= v < N:  # an edge outside the views is refused by the entry point, which reads these host copies
            lists[v].append(o)
    starts = [0]
    for ls in lists:
        starts.append(starts[-1] + len(ls))
    vt, vt_p = _host_i64([x for r in rows for x in r] + starts)
    ol, ol_p = _host_i32([o for ls in lists for o in ls])
    addr = lambda t: t.data_ptr() if torch.is_tensor(t) else int(t)  # noqa: E731
    ot, ot_p = _host_i64([x for (p, w, H, W) in maps for x in (addr(p), addr(w), int(H), int(W))])
    tb = {"n_views": N, "n_edges": E, "total": off, "shapes": [(int(H), int(W)) for H, W in shapes], "maps": maps,
          "view_table_host": (vt, vt_p), "edges_host": (eh, eh_p), "obs_table_host": (ot, ot_p), "obs_list_host": (ol, ol_p), "device": device}
    if device is not None:
        tb.update(view_table=_table(vt, device), edges=_table(eh, device), obs_table=_table(ot, device), obs_list=_table(ol, device))
    return tb


def galign_loss_grad(poses, focals, pp, log_depth, pw_poses, adaptors, tables, dist="l1"):
    """f3r_galign_loss_grad (include/f3r.h): poses (N, 3, 4), focals (N,), pp (N, 2), log_depth (total,), pw_poses (E, 3, 4), adaptors (E, 3),
    contiguous fp32 on the device of the tables (galign_tables).  -> (loss: 0-dim fp64, d_log_depth, d_poses, d_focals, d_pp, d_pw_poses,
    d_adaptors: fp32 shaped like the inputs), all on the device.  Launches only: nothing is read back.  Inputs are not written to."""
    fn, size_fn = _lib.entry("f3r_galign_loss_grad"), _lib.entry("f3r_galign_workspace_bytes")
    N, E, total, dev = tables["n_views"], tables["n_edges"], tables["total"], tables["device"]
    dist_id = galign_dist_id(dist)
    f32 = torch.float32
    for t, name, shape in ((poses, "poses", (N, 3, 4)), (focals, "focals", (N,)), (pp, "pp", (N, 2)), (log_depth, "log_depth", (total,)),
                           (pw_poses, "pw_poses", (E, 3, 4)), (adaptors, "adaptors", (E, 3))):
        require_gpu(t, name)
        if t.dtype != f32 or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
            raise ValueError(f"galign_loss_grad: {name} must be contiguous fp32 {shape} on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    nbytes = size_fn(N, E)
    if nbytes == 0:
        raise ValueError(f"galign_loss_grad: {N} views with {E} edges is not a supported shape (2 .. 65535 views, at least one edge)")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    outs = [torch.empty_like(t) for t in (log_depth, poses, focals, pp, pw_poses, adaptors)]
    with torch.cuda.device(dev):
        check(fn(ptr(poses), ptr(focals), ptr(pp), ptr(log_depth), ptr(pw_poses), ptr(adaptors), ptr(tables["view_table"]),
                 tables["view_table_host"][1], N, ptr(tables["edges"]), tables["edges_host"][1], E, ptr(tables["obs_table"]),
                 tables["obs_table_host"][1], ptr(tables["obs_list"]), tables["obs_list_host"][1], dist_id, ptr(loss), *[ptr(t) for t in outs],
                 ptr(ws), nbytes, stream_ptr()), "f3r_galign_loss_grad")
    del ws  # the launches are stream-ordered before the caching allocator can hand the block out again
    return (loss, *outs)
