"""Triangle-mesh export on the GPU: the `as_mesh=True` branch of the reference's multi-view notebook
(`notebooks/demo_multiview.ipynb::plot_3d_points_with_colors`), which turns a prediction into one coloured mesh: per view
`np.percentile(conf, p)`, `conf > thr`, `((img + 1) * 127.5).astype(np.uint8).clip(0, 255)`, then `fast3r/dust3r/viz.py::pts3d_to_trimesh`
(:43-90; every pixel a vertex, every 2 x 2 block of pixels two triangles, each written twice with opposite winding, a triangle kept iff
its three vertices are valid) and `cat_meshes` (:93-104).  There it is single-threaded numpy after a D2H copy of every pointmap; here it
is HIP kernels (fast3r_amd/csrc/f3r_mesh.hip): one exact radix selection per view, one count pass, one scan, one write pass.

* `build_mesh(out)` -> `Mesh`: all views in one pass; no per-view dicts, nothing concatenated.
* `pts3d_to_trimesh(img, pts3d, valid=None)`, `cat_meshes(meshes)`: the reference's names, argument order and assertions, on device tensors.
* `generate_mesh_ply_bytes` / `save_mesh_ply` / `Mesh.save_ply`: a binary PLY packed on the device.

Face order (the reference's): view after view; per view the kept A triangles `(i1, i2, i3)` in quad order, the same as `(i3, i2, i1)`,
the kept B triangles `(i2, i3, i4)`, the same as `(i4, i3, i2)`, with `i1..i4` the top-left, top-right, bottom-left and bottom-right
pixel of a quad plus the vertices of the views before.  A faces take the colour of the top-left pixel, B faces of the bottom-right.

Deviations, stated in DESIGN.md section 7 and docs/rows_f.md: image values outside [-1, 1] saturate where the reference's uint8 cast
wraps; `cat_meshes` does not write to its inputs (the reference adds the vertex offsets into the callers' face arrays in place);
`sample` selects the batch row where the reference's `squeeze()` only works at B = 1; a view with a NaN confidence gets the quiet NaN
as its threshold (np.percentile hands back the data's own NaN) and, as there, no faces.  `double_sided=False`, `drop_unreferenced=True`
and `index_dtype=torch.int32` have no reference counterpart; `flip_axes=True` is the notebook's two assignments.

The PLY layout is this project's own (the reference hands the file to `trimesh`): the header of `mesh_ply_header`,

    ply
    format binary_little_endian 1.0
    element vertex <Nv>
    property float x
    property float y
    property float z
    element face <F>
    property list uchar int vertex_indices
    property uchar red
    property uchar green
    property uchar blue
    end_header

then Nv records of 12 bytes (x, y, z as little-endian fp32) and F records of 16 bytes (the byte 3, three little-endian int32 vertex
indices, red, green, blue).
"""
import numpy as np
import torch

from . import post_ops
from ._frontend import check_inputs, fp32_on, on_work_device, preds_and_views, read_back
from ._lib import require_gpu, work_device
from .scene import percentile_indexes

MESH_VERTEX_BYTES = 12
MESH_FACE_BYTES = 16


def mesh_ply_header(n_vertices, n_faces):
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {n_vertices}", "property float x", "property float y",
             "property float z", f"element face {n_faces}", "property list uchar int vertex_indices", "property uchar red",
             "property uchar green", "property uchar blue", "end_header"]
    return "\n".join(lines).encode("ascii") + b"\n"


def generate_mesh_ply_bytes(vertices, faces, face_colors):
    """The binary PLY of a mesh (layout: the module text), packed on the device and brought back with one copy through pinned memory.
    vertices (Nv, 3) fp32, faces (F, 3) int32 / int64, face_colors (F, 3) uint8; torch or numpy."""
    vertices, faces, face_colors = (on_work_device(x, "generate_mesh_ply_bytes", name)[0]
                                    for x, name in ((vertices, "vertices"), (faces, "faces"), (face_colors, "face_colors")))
    nv, nf = vertices.shape[0], faces.shape[0]
    if vertices.dim() != 2 or vertices.shape[1] != 3 or tuple(faces.shape) != (nf, 3) or tuple(face_colors.shape) != (nf, 3):
        raise ValueError(f"generate_mesh_ply_bytes: vertices (Nv, 3), faces (F, 3) and face_colors (F, 3), got {tuple(vertices.shape)}, "
                         f"{tuple(faces.shape)} and {tuple(face_colors.shape)}")
    if vertices.dtype != torch.float32 or face_colors.dtype != torch.uint8:
        raise ValueError(f"generate_mesh_ply_bytes: vertices must be float32 and face_colors uint8, got {vertices.dtype} and {face_colors.dtype}")
    header = mesh_ply_header(nv, nf)
    if nv == 0 and nf == 0:
        return header
    rec = post_ops.mesh_ply_pack(vertices, faces.to(vertices.device), face_colors.to(vertices.device))
    return header + read_back(rec)


def save_mesh_ply(path, vertices, faces, face_colors):
    with open(path, "wb") as f:
        f.write(generate_mesh_ply_bytes(vertices, faces, face_colors))


class Mesh:
    """What `build_mesh` returns: `vertices` (Nv, 3) fp32, `faces` (F, 3) int64 or int32, `face_colors` (F, 3) uint8 on the device;
    `thresholds` (V,) fp32 numpy, the per-view confidence thresholds; `faces_per_view`, `vertices_per_view` (V,) int64 numpy."""

    def __init__(self, vertices, faces, face_colors, thresholds, faces_per_view, vertices_per_view):
        self.vertices, self.faces, self.face_colors = vertices, faces, face_colors
        self.thresholds, self.faces_per_view, self.vertices_per_view = thresholds, faces_per_view, vertices_per_view

    def as_dict(self):
        """the reference's `cat_meshes` dict"""
        return dict(vertices=self.vertices, face_colors=self.face_colors, faces=self.faces)

    def save_ply(self, path):
        """-> (vertices, faces) written"""
        save_mesh_ply(path, self.vertices, self.faces, self.face_colors)
        return self.vertices.shape[0], self.faces.shape[0]


def pts3d_to_trimesh(img, pts3d, valid=None):
    """viz.py:43-90 on device tensors: img (H, W, 3) uint8, pts3d (H, W, 3) fp32, valid (H, W) bool / uint8 or None (every face kept)
    -> dict(vertices (H W, 3) fp32, face_colors (F, 3) uint8, faces (F, 3) int64) on the device, in the reference's order."""
    for t, name in ((img, "img"), (pts3d, "pts3d")) + (((valid, "valid"),) if valid is not None else ()):
        if not torch.is_tensor(t):
            raise ValueError(f"pts3d_to_trimesh: {name} must be a torch tensor on a ROCm device, got {type(t).__name__}")
        require_gpu(t, name)
    H, W, THREE = img.shape
    assert THREE == 3
    assert img.shape == pts3d.shape
    if img.dtype != torch.uint8 or pts3d.dtype != torch.float32:
        raise ValueError(f"pts3d_to_trimesh: img must be uint8 and pts3d float32, got {img.dtype} and {pts3d.dtype}")
    mask = None
    if valid is not None:
        assert valid.shape == (H, W)
        if valid.dtype == torch.bool:
            mask = valid.contiguous().view(torch.uint8).reshape(-1)   # 0 / 1 bytes as they are
        elif valid.dtype == torch.uint8:
            mask = valid.reshape(-1)
        else:
            raise ValueError(f"pts3d_to_trimesh: valid must be bool or uint8, got {valid.dtype}")
    out = post_ops.mesh_build([None], [pts3d.reshape(-1, 3)], [img.reshape(-1, 3)], [mask], [(H, W)], [None])
    return dict(vertices=out["vertices"], face_colors=out["face_colors"], faces=out["faces"])


def cat_meshes(meshes):
    """viz.py:93-104 on device tensors.  Unlike the reference, which adds the vertex offsets into the callers' face arrays in place, the
    inputs are left as they are."""
    vertices, faces, colors = zip(*[(m["vertices"], m["faces"], m["face_colors"]) for m in meshes])
    n_vertices = np.cumsum([0] + [len(v) for v in vertices])
    faces = [f + int(n_vertices[i]) for i, f in enumerate(faces)]
    return dict(vertices=torch.cat(vertices), face_colors=torch.cat(colors), faces=torch.cat(faces))


def build_mesh(output_or_preds, views=None, *, sample=0, head="global", min_conf_thr_percentile=80, valid=None, double_sided=True,
               drop_unreferenced=False, flip_axes=False, index_dtype=torch.int64):
    """The `as_mesh=True` branch of `plot_3d_points_with_colors` for all views in one pass -> `Mesh`.  Takes what `inference()` returns
    ({'preds', 'views'}, host tensors: uploaded here) or (preds, views) with device tensors; views may differ in H x W; `sample` selects
    the batch row.  head="global" reads `pts3d_in_other_view` / `conf` (the notebook's), head="local" `pts3d_local` / `conf_local`, or
    `pts3d_local_aligned_to_global` where `align_local_pts3d_to_global` has put it.  A vertex is valid iff conf > np.percentile(conf of
    its view, min_conf_thr_percentile) and, with `valid` (a list of per-view (H, W) bool / uint8 masks), valid there too.
    `double_sided=False` leaves the backward-wound copies out; `drop_unreferenced=True` keeps only the vertices that a face uses, in
    their order, and renumbers the faces; `flip_axes=True` maps (x, y, z) to (x, z, -y); `index_dtype`: torch.int64 (the reference's)
    or torch.int32.  Input tensors are never written.  Results stay on the device."""
    preds, views = preds_and_views(output_or_preds, views, "build_mesh", "face colours")
    if head not in ("global", "local"):
        raise ValueError(f"build_mesh: head must be 'global' or 'local', got {head!r}")
    if not 0 <= min_conf_thr_percentile <= 100:
        raise ValueError(f"build_mesh: min_conf_thr_percentile = {min_conf_thr_percentile} outside [0, 100]")
    if isinstance(valid, str):
        raise ValueError(f"build_mesh: valid = {valid!r}; accepted values are None or a list of per-view (H, W) masks")
    post_ops.mesh_index_id(index_dtype)
    conf_key = "conf" if head == "global" else "conf_local"
    pts_key = "pts3d_in_other_view"
    if head == "local":
        pts_key = "pts3d_local_aligned_to_global" if len(preds) and all("pts3d_local_aligned_to_global" in p for p in preds) else "pts3d_local"
    check_inputs(preds, views, sample, valid, what="build_mesh", keys=(pts_key, conf_key), mask_name="valid")
    dev = work_device(preds[0][conf_key], "preds")

    conf, pts, img, mask, shapes, ranks = [], [], [], [], [], []
    for i, (pred, view) in enumerate(zip(preds, views)):
        H, W = (int(x) for x in pred[conf_key].shape[1:3])
        if tuple(view["img"].shape[1:]) != (3, H, W):
            raise ValueError(f"build_mesh: views[{i}]['img'] is {tuple(view['img'].shape)}; expected (B, 3, {H}, {W})")
        if tuple(pred[pts_key].shape[1:]) != (H, W, 3):
            raise ValueError(f"build_mesh: preds[{i}]['{pts_key}'] is {tuple(pred[pts_key].shape)}; expected (B, {H}, {W}, 3)")
        shapes.append((H, W))
        conf.append(fp32_on(pred[conf_key][sample], dev, (H * W,)))
        pts.append(fp32_on(pred[pts_key][sample], dev, (H * W, 3)))
        img.append(fp32_on(view["img"][sample], dev, (3, H * W)))   # the (3, H, W) planes as stored: nothing is permuted
        ranks.append(percentile_indexes(H * W, min_conf_thr_percentile))
        m = None
        if valid is not None:
            m = torch.as_tensor(valid[i])
            if m.device != dev:
                m = m.to(dev)
            m = m.contiguous().view(torch.uint8) if m.dtype in (torch.bool, torch.int8) else m
            m = m.reshape(-1)
        mask.append(m)
    out = post_ops.mesh_build(conf, pts, img, mask, shapes, ranks, double_sided=double_sided, drop_unreferenced=drop_unreferenced,
                              flip_axes=flip_axes, index_dtype=index_dtype)
    cnt = out["counts"]
    return Mesh(out["vertices"], out["faces"], out["face_colors"], out["thresholds"], (2 if double_sided else 1) * (cnt[:, 0] + cnt[:, 1]),
                cnt[:, 2].copy())


__all__ = ["Mesh", "build_mesh", "cat_meshes", "generate_mesh_ply_bytes", "mesh_ply_header", "pts3d_to_trimesh", "save_mesh_ply"]
