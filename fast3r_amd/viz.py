"""Pictures with triangles in them: a mesh (`render_mesh`), and the cloud with the estimated cameras in it
(`plot_3d_points_with_estimated_camera_poses` of the reference's multi-view notebook, which goes through `SceneViz`, `auto_cam_size` and
`add_scene_cam` of fast3r/dust3r/viz.py:133-305).  The reference shows both with trimesh / plotly viewers; here the renderer is the
project's own: the point splat of fast3r_amd/render.py and a z-buffered triangle rasteriser (fast3r_amd/csrc/f3r_raster.hip) write the
same packed (fp32 depth, index) keys into one buffer, and the splat's resolve turns them into colours.

* `render_mesh(mesh, camera, points=, colors=)`: a `Mesh` or a dict of `vertices` / `faces` / `face_colors`, optionally with a cloud.
* `auto_cam_size`, `CAM_COLORS`: the reference's.
* `camera_meshes(poses_c2w, focals, images=...)`: the pyramids of `add_scene_cam` for all cameras at once, as one mesh dict.
* `SceneViz`: the reference's method names; `render` / `save_png` instead of a viewer.
* `plot_3d_points_with_estimated_camera_poses(preds, views, ...)`: the notebook's function; returns the picture.

The per-triangle arithmetic is the "triangle rasteriser" section of include/f3r.h; tests/raster_ref.py restates it in numpy.

Deviations, stated in DESIGN.md section 7 and docs/rows_f.md: no near-plane clipping (a triangle with a vertex nearer than znear is
dropped whole); no textures (a camera's image is a grid of flat-coloured cells); one sample per pixel; the cameras' colours come from
`CAM_COLORS` where the notebook draws random ones; there is no HTML export and no interactive viewer.
"""
import math

import numpy as np
import torch

from . import _lib, post_ops
from .cloud import combine_points
from .mesh import Mesh
from .pose import estimate_camera_poses
from .render import _checked, _save_png, cloud_camera, render_points
from .scene import save_ply

CAM_COLORS = [(255, 0, 0), (0, 0, 255), (0, 255, 0), (255, 0, 255), (255, 204, 0), (0, 204, 204), (128, 255, 255), (255, 128, 255),
              (255, 255, 128), (0, 0, 0), (128, 128, 128)]
SLIVER_FACES = 24         # per camera: 4 side faces x 2 copies x 3 pseudo-edges
PYRAMID_VERTICES = 15     # per camera: apex and four base corners; their 0.95 copy; their copy turned by 2 degrees


# ------------------------------------------------------------------------------------------------------------------- a mesh as a picture
def _mesh_parts(mesh, who):
    if isinstance(mesh, Mesh):
        mesh = mesh.as_dict()
    try:
        vertices, faces, face_colors = mesh["vertices"], mesh["faces"], mesh["face_colors"]
    except (TypeError, KeyError):
        raise ValueError(f"{who}: mesh must be a fast3r_amd.Mesh or a dict with 'vertices', 'faces' and 'face_colors'") from None
    for t, name in ((vertices, "vertices"), (faces, "faces"), (face_colors, "face_colors")):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: mesh['{name}'] must be a torch tensor on a ROCm device, got {type(t).__name__}")
        _lib.require_gpu(t, name)
    nf = faces.shape[0]
    if tuple(face_colors.shape) != (nf, 3) or face_colors.dtype != torch.uint8 or face_colors.device != vertices.device:
        raise ValueError(f"{who}: face_colors must be ({nf}, 3) uint8 on {vertices.device}, got {tuple(face_colors.shape)} "
                         f"{face_colors.dtype} on {face_colors.device}")
    return vertices, faces, face_colors


def render_mesh(mesh, camera=None, *, points=None, colors=None, point_size=5.0, width=1920, height=1080, background=(255, 255, 255),
                return_depth=False):
    """A device mesh -- a `Mesh`, or a dict with `vertices` (nv, 3) fp32, `faces` (nf, 3) int32 / int64 and `face_colors` (nf, 3) uint8
    such as `pts3d_to_trimesh` or `cat_meshes` return -- as a (height, width, 3) uint8 device picture, row 0 at the top; with `points` (n,
    3) fp32 and `colors` (n, 3) uint8, the cloud is drawn into the same picture as squares of `point_size` pixels.  Points and triangles
    go into one key buffer: points take the indices [0, n) and face f takes n + f, so the nearest surface shows, at equal depth a point
    wins over a face and a lower face over a higher one.  `camera` None: the bird's-eye camera (`cloud_camera`) of the points if given,
    otherwise of the vertices.  Every face is flat-coloured and drawn whatever its winding: nothing is culled, so
    `build_mesh(double_sided=False)` gives the same picture for half the work.  A triangle with a vertex nearer than the camera's znear, a
    NaN or inf coordinate or an index outside the vertices is not drawn.  return_depth: (picture, (height, width) fp32 depth, +inf where
    empty).  Inputs are never written."""
    _lib.entry("f3r_raster_triangles")
    vertices, faces, face_colors = _mesh_parts(mesh, "render_mesh")
    n = 0
    if points is not None:
        points, colors, n = post_ops._cloud_points(points, "render_mesh", colors, bits=32)
        if colors is None:
            raise ValueError("render_mesh: points need colors, an (n, 3) uint8 device tensor")
    if n == 0 and faces.shape[0] == 0:
        raise ValueError("render_mesh: nothing to draw: no faces and no points")
    if camera is None:
        camera = cloud_camera(points if n else vertices)
    width, height, point_size = _checked(width, height, point_size, camera, "render_mesh")
    keys = post_ops.render_keys(width, height, vertices.device)
    if n:
        post_ops.render_splat(points, 0, n, camera.words(), point_size, keys)
    if faces.shape[0]:                                                                    # a mesh without faces (and perhaps without vertices) adds nothing
        post_ops.raster_triangles(vertices, faces, camera.words(), keys, index_base=n)
    table = torch.cat((colors, face_colors)) if n else face_colors
    return post_ops.render_resolve(keys, table, background, return_depth=return_depth)


# ------------------------------------------------------------------------------------------------------------------- cameras
def _centres(poses_c2w):
    out = []
    for p in poses_c2w:
        p = p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)
        out.append(np.asarray(p, dtype=np.float64).reshape(-1, 4)[:3, 3])
    return np.stack(out) if out else np.zeros((0, 3))


def auto_cam_size(poses_c2w):
    """viz.py:133: 0.1 * the median distance between the camera centres (`get_med_dist_between_poses`: np.median of scipy's pdist).  Host
    fp64.  The condensed distances are the square roots of (dx dx + dy dy) + dz dz over the pairs i < j, and the median is np.median's
    (the mean of the two middle values of an even count).  Fewer than two cameras have no distance: nan, as the reference."""
    c = _centres(poses_c2w)
    i, j = np.triu_indices(len(c), k=1)
    d = c[i] - c[j]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    with np.errstate(all="ignore"):
        return float(0.1 * np.median(dist)) if len(dist) else float("nan")


def camera_image_size(image_shape=None, imsize=None, focal=None):
    """add_scene_cam's branches (viz.py:239-254) -> (H, W, focal): H, W from the image (H, W, 3), else imsize = (W, H), else focal / 1.1,
    else 1; focal defaults to 1.1 * min(H, W)."""
    if image_shape is not None:
        H, W = image_shape[0], image_shape[1]
    elif imsize is not None:
        W, H = imsize
    elif focal is not None:
        H = W = focal / 1.1
    else:
        H = W = 1
    if focal is None:
        focal = min(H, W) * 1.1
    return float(H), float(W), float(focal)


def image_grid(H, W, image_cells):
    """cells (rows, columns) of a camera's image plane: image_cells on the long side, the other in proportion and at least 1"""
    image_cells = int(image_cells)
    if image_cells < 1:
        raise ValueError(f"camera_meshes: image_cells = {image_cells}; need >= 1")
    if W >= H:
        return max(1, int(round(image_cells * H / W))), image_cells
    return image_cells, max(1, int(round(image_cells * W / H)))


def camera_vertices(pose_c2w, H, W, focal, cam_size=0.03, grid=None):
    """The vertices of one camera, host fp64, (15 + (gy + 1)(gx + 1), 3) in world coordinates.  In the camera's OpenCV frame (x right, y
    down, z forward) the apex is the optical centre and the base corners are (+-cam_size W / (2 H), +-cam_size / 2, focal cam_size / H),
    in the order top-left, top-right, bottom-right, bottom-left of the image: what the reference's pose_c2w @ OPENGL @ aspect_ratio @
    rot45 makes of its 4-section cone, so the pyramid opens by the camera's field of view.  Rows 0 .. 4: apex, corners.  Rows 5 .. 9:
    their copy scaled by 0.95 about the base's centre (the cone's own origin).  Rows 10 .. 14: their copy turned by 2 degrees about the
    optical axis in the cone's frame, that is before the aspect ratio stretches x.  Then, with grid = (gy, gx), the (gy + 1) x (gx + 1)
    corners of the image plane's cells, row-major from the top-left corner."""
    pose = np.asarray(pose_c2w, dtype=np.float64).reshape(-1, 4)[:3]
    hx, hy, hz = cam_size * W / (2.0 * H), cam_size / 2.0, focal * cam_size / H
    cone = np.array([[0.0, 0.0, 0.0], [-hx, -hy, hz], [hx, -hy, hz], [hx, hy, hz], [-hx, hy, hz]])
    centre = np.array([0.0, 0.0, hz])
    smaller = centre + 0.95 * (cone - centre)
    a, t = W / H, math.radians(2.0)
    c, s = math.cos(t), math.sin(t)
    # OPENGL (y and z negated) turns the cone frame's rotation by +2 degrees about z into one by -2 degrees in the x, y of this frame
    turned = np.stack([c * cone[:, 0] + a * s * cone[:, 1], -s * cone[:, 0] / a + c * cone[:, 1], cone[:, 2]], axis=1)
    parts = [cone, smaller, turned]
    if grid is not None:
        gy, gx = grid
        v, u = np.meshgrid(np.arange(gy + 1) / gy, np.arange(gx + 1) / gx, indexing="ij")
        parts.append(np.stack([-hx + 2.0 * hx * u, -hy + 2.0 * hy * v, np.full(u.shape, hz)], axis=-1).reshape(-1, 3))
    local = np.concatenate(parts)
    return local @ pose[:, :3].T + pose[:, 3]


def camera_faces(grid=None):
    """The faces of one camera over the rows of `camera_vertices`, int64: the 24 sliver triangles that draw the pyramid's edges -- per
    side face (a, b, c) = (apex, corner k, corner k + 1) the reference's (a, b, b2), (a, a2, c), (c2, b, c) with 2 = the 0.95 copy, and
    the same with the turned copy; the reversed duplicates are left out, since nothing is culled -- then two triangles per image cell."""
    faces = []
    for k in range(4):
        a, b, c = 0, 1 + k, 1 + (k + 1) % 4
        for off in (5, 10):
            faces += [(a, b, b + off), (a, a + off, c), (c + off, b, c)]
    if grid is not None:
        gy, gx = grid
        r, q = np.mgrid[0:gy, 0:gx]
        v00 = PYRAMID_VERTICES + (r * (gx + 1) + q).reshape(-1)
        cells = np.stack([np.stack([v00, v00 + 1, v00 + gx + 1], axis=1), np.stack([v00 + 1, v00 + gx + 2, v00 + gx + 1], axis=1)], axis=1)
        return np.concatenate([np.array(faces, dtype=np.int64), cells.reshape(-1, 3)])
    return np.array(faces, dtype=np.int64)


def _image_u8(image, dev):
    """-> (H, W, 3) uint8 on dev from (H, W, 3) uint8, float (H, W, 3) in [0, 1] (the reference's np.uint8(255 * image); values outside
    saturate), or a view's (3, H, W) float `img` in [-1, 1] (the project's colour rule, trunc((img + 1) * 127.5) saturated)"""
    t = torch.as_tensor(image)
    if t.dim() != 3 or 3 not in (t.shape[0], t.shape[2]):
        raise ValueError(f"camera_meshes: an image must be (H, W, 3) or (3, H, W), got {tuple(t.shape)}")
    t = t.to(dev)
    if t.shape[2] == 3 and (t.shape[0] != 3 or t.dtype == torch.uint8):                 # (H, W, 3); a float (3, W, 3) reads as planes
        if t.dtype == torch.uint8:
            return t.contiguous()
        if not t.is_floating_point():
            raise ValueError(f"camera_meshes: an (H, W, 3) image must be uint8 or float in [0, 1], got {t.dtype}")
        return post_ops.color_to_u8(t.float(), 0)
    if not t.is_floating_point():
        raise ValueError(f"camera_meshes: a (3, H, W) image must be float in [-1, 1], got {t.dtype}")
    return post_ops.color_to_u8(t.float().permute(1, 2, 0).contiguous(), 1)


def _get(seq, i):
    return None if seq is None else seq[i]


def _scalar(v):
    if v is None:
        return None
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    v = float(np.asarray(v, dtype=np.float64).reshape(-1)[0])   # the reference takes focal[0] of an array
    return None if math.isnan(v) else v


def camera_meshes(poses_c2w, focals=None, *, images=None, imsizes=None, colors=None, cam_size=0.03, image_cells=64, device=None):
    """The geometry of the reference's `add_scene_cam` for all cameras at once -> dict(vertices (nv, 3) fp32, faces (nf, 3) int64,
    face_colors (nf, 3) uint8) on the device, what `render_mesh` and `cat_meshes` take.  poses_c2w: camera-to-world matrices (OpenCV
    convention); focals, images, imsizes, colors: per camera or None, entries may be None (a focal of NaN counts as None).  Per camera:
    `camera_image_size` decides H, W and the focal; `camera_vertices` / `camera_faces` give a pyramid whose apex is the optical centre
    and whose base is the image plane cam_size high, drawn as 24 sliver triangles along its edges in colors[i], or CAM_COLORS[i % 11];
    with an image the base is a grid of `image_cells` cells on the long side, each two triangles in the colour of the image pixel
    nearest the cell's centre (the reference textures one quad; without an image there are no plane faces).  The vertex positions are
    host fp64, rounded to fp32 once; the cell colours are gathered on the device."""
    _lib.entry("f3r_raster_triangles")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    vertices, faces, face_colors, base = [], [], [], 0
    for i, pose in enumerate(poses_c2w):
        pose = pose.detach().cpu().numpy() if torch.is_tensor(pose) else np.asarray(pose)
        image = _get(images, i)
        image = None if image is None else _image_u8(image, dev)
        H, W, focal = camera_image_size(None if image is None else image.shape, _get(imsizes, i), _scalar(_get(focals, i)))
        grid = None if image is None else image_grid(H, W, image_cells)
        v, f = camera_vertices(pose, H, W, focal, float(cam_size), grid), camera_faces(grid)
        color = _get(colors, i)
        color = CAM_COLORS[i % len(CAM_COLORS)] if color is None else tuple(int(c) for c in np.asarray(color).reshape(-1)[:3])
        vertices.append(torch.from_numpy(v.astype(np.float32)).to(dev))
        faces.append(torch.from_numpy(f + base).to(dev))
        face_colors.append(torch.tensor([color] * SLIVER_FACES, dtype=torch.uint8, device=dev))
        if grid is not None:
            gy, gx = grid
            rows = torch.clamp(((torch.arange(gy, device=dev, dtype=torch.float64) + 0.5) * (image.shape[0] / gy)).floor().long(), max=image.shape[0] - 1)
            cols = torch.clamp(((torch.arange(gx, device=dev, dtype=torch.float64) + 0.5) * (image.shape[1] / gx)).floor().long(), max=image.shape[1] - 1)
            cells = image[rows][:, cols].reshape(-1, 3)                                   # the pixel nearest each cell's centre
            face_colors.append(cells.repeat_interleave(2, dim=0))
        base += len(v)
    if not vertices:
        raise ValueError("camera_meshes: no cameras")
    return dict(vertices=torch.cat(vertices), faces=torch.cat(faces), face_colors=torch.cat(face_colors))


# ------------------------------------------------------------------------------------------------------------------- the scene
def _device_tensor(x, dev):
    return torch.as_tensor(x).to(dev)


def _cloud_colors(col, dev):
    """the reference's uint8(): floats are 255 * c (saturated here), integers as they are"""
    col = _device_tensor(col, dev)
    if col.is_floating_point():
        return post_ops.color_to_u8(col.float().contiguous(), 0)
    return col.to(torch.uint8)


def _is_triple(color, one_view=None):
    """whether `color` is one (r, g, b) for all points rather than colours per point, decided without converting a list of views: a
    list or tuple of three scalars; or an array / tensor of shape (3,), unless the points are a single array of that same shape (one
    point: then both readings give the same cloud)"""
    if torch.is_tensor(color) or isinstance(color, np.ndarray):
        if one_view is not None and tuple(color.shape) == tuple(one_view.shape):
            return False
        return tuple(color.shape) == (3,)
    if isinstance(color, (list, tuple)):
        return len(color) == 3 and all(isinstance(c, (int, float, np.number)) or (hasattr(c, "shape") and tuple(c.shape) == ())
                                       for c in color)
    raise ValueError(f"SceneViz.add_pointcloud: color must be an (r, g, b) triple or per-view colours, got {type(color).__name__}")


class SceneViz:
    """The reference's SceneViz (viz.py:137-192) over device tensors: `add_pointcloud`, `add_camera` and `add_cameras` collect, `render`
    draws everything collected through one camera.  There is no display here: `show` raises."""

    def __init__(self, device=None):
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None and torch.cuda.is_available() else device
        self.points, self.colors, self.cameras = [], [], []

    def _dev(self):
        if self.device is None:
            raise _lib.F3RError("fast3r_amd: SceneViz needs a ROCm device (there is no CPU fallback)")
        return torch.device(self.device)

    def add_pointcloud(self, pts3d, color, mask=None):
        """pts3d: a list over views of (..., 3) arrays or tensors (or one such); mask: per view, boolean, selecting on the device; color: a
        list like pts3d (uint8, or float in [0, 1]) or one (r, g, b) triple for all points"""
        dev = self._dev()
        single = torch.is_tensor(pts3d) or isinstance(pts3d, np.ndarray)
        pts3d = [pts3d] if single else list(pts3d)
        masks = [None] * len(pts3d) if mask is None else ([mask] if single else list(mask))
        per_view = not _is_triple(color, pts3d[0] if single else None)
        cols = ([color] if single else list(color)) if per_view else [None] * len(pts3d)
        if len(masks) != len(pts3d) or len(cols) != len(pts3d):
            raise ValueError(f"SceneViz.add_pointcloud: {len(pts3d)} views of points, {len(cols)} of colours, {len(masks)} of masks")
        triple = None
        if not per_view:                                                                  # through torch on the device, whatever holds the three
            rgb = torch.tensor([c.item() if hasattr(c, "item") else c for c in color]) if isinstance(color, (list, tuple)) else color
            triple = _cloud_colors(rgb, dev).reshape(1, 3)
        for p, m, c in zip(pts3d, masks, cols):
            p = _device_tensor(p, dev).float()
            m = None if m is None else _device_tensor(m, dev).bool()
            pts = (p if m is None else p[m]).reshape(-1, 3)
            if per_view:
                c = _cloud_colors(c, dev)
                col = (c if m is None else c[m]).reshape(-1, 3)
                assert col.shape == pts.shape
            else:
                col = triple.expand(pts.shape[0], 3)
            self.points.append(pts)
            self.colors.append(col)
        return self

    def add_camera(self, pose_c2w, focal=None, color=(0, 0, 0), image=None, imsize=None, cam_size=0.03):
        self.cameras.append(dict(pose=pose_c2w, focal=focal, color=color, image=image, imsize=imsize, cam_size=cam_size))
        return self

    def add_cameras(self, poses, focals=None, images=None, imsizes=None, colors=None, **kw):
        for i, pose_c2w in enumerate(poses):
            self.add_camera(pose_c2w, _get(focals, i), image=_get(images, i), color=_get(colors, i), imsize=_get(imsizes, i), **kw)
        return self

    def geometry(self, image_cells=64):
        """-> (points or None, colors or None, mesh dict or None) on the device"""
        dev = self._dev()
        points = torch.cat(self.points).contiguous() if self.points else None
        colors = torch.cat(self.colors).contiguous() if self.colors else None
        if points is not None and points.shape[0] == 0:
            points = colors = None
        meshes = [camera_meshes([c["pose"]], [c["focal"]], images=[c["image"]], imsizes=[c["imsize"]],
                                colors=[CAM_COLORS[i % len(CAM_COLORS)] if c["color"] is None else c["color"]],
                                cam_size=c["cam_size"], image_cells=image_cells, device=dev) for i, c in enumerate(self.cameras)]
        mesh = None
        if meshes:
            offsets = np.cumsum([0] + [len(m["vertices"]) for m in meshes])
            mesh = dict(vertices=torch.cat([m["vertices"] for m in meshes]), face_colors=torch.cat([m["face_colors"] for m in meshes]),
                        faces=torch.cat([m["faces"] + int(o) for m, o in zip(meshes, offsets)]))
        return points, colors, mesh

    def render(self, camera=None, *, width=1920, height=1080, point_size=2, background=(255, 255, 255), return_depth=False, image_cells=64):
        """the picture of everything added, (height, width, 3) uint8 on the device; camera None: the bird's-eye camera of the points, or
        of the cameras' vertices when there are no points"""
        points, colors, mesh = self.geometry(image_cells)
        if mesh is None:
            if points is None:
                raise ValueError("SceneViz.render: nothing was added")
            return render_points(points, colors, camera, width=width, height=height, point_size=point_size, background=background,
                                 return_depth=return_depth)
        return render_mesh(mesh, camera, points=points, colors=colors, point_size=point_size, width=width, height=height,
                           background=background, return_depth=return_depth)

    def save_png(self, path, camera=None, **kw):
        picture = self.render(camera, **kw)
        _save_png((picture[0] if isinstance(picture, tuple) else picture).cpu().numpy(), path)
        return picture

    def show(self, point_size=2, viewer=None):
        raise NotImplementedError("SceneViz.show: there is no display or viewer here; use SceneViz.render(camera, width=, height=) for the "
                                  "picture or SceneViz.save_png(path) for a file")


FLIP = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0], [0, -1.0, 0, 0], [0, 0, 0, 1.0]])   # the notebook's two assignments: (x, y, z) -> (x, z, -y)


def plot_3d_points_with_estimated_camera_poses(preds, views, title="3D Points and Camera Poses", flip_axes=False, min_conf_thr_percentile=80,
                                               export_ply_path=None, export_html_path=None, *, sample=0, output_path=None, camera=None,
                                               width=1920, height=1080, point_size=1.0, niter_PnP=10):
    """The notebook's function, names, order and defaults: per view the pixels of `pts3d_in_other_view` with conf > np.percentile(conf,
    min_conf_thr_percentile) and their colours (`combine_points`), the poses and focals of `estimate_camera_poses(preds, niter_PnP=10)`,
    cam_size = max(auto_cam_size(poses), 0.05), and one camera per view carrying its image.  `flip_axes` maps (x, y, z) to (x, z, -y) --
    the notebook's two assignments -- for points and poses alike.  `export_ply_path`: the kept cloud as a PLY (`save_ply`).  -> the
    (height, width, 3) uint8 device picture, also written as a PNG when `output_path` is given.  `preds` may be the dict `inference()`
    returns (then `views` may be None).  Deviations: the cameras are coloured from CAM_COLORS in view order (the notebook draws random
    colours); `title` is accepted and unused (a picture has none); `export_html_path` other than None is a ValueError, because there is
    no HTML viewer; the picture is returned where the notebook opens a viewer."""
    if export_html_path is not None:
        raise ValueError("plot_3d_points_with_estimated_camera_poses: export_html_path is not supported: there is no HTML viewer here; "
                         "use output_path= for a PNG or export_ply_path= for the cloud")
    _lib.entry("f3r_raster_triangles")
    if isinstance(preds, dict) and "preds" in preds:
        preds, views = preds["preds"], (preds["views"] if views is None else views)
    points, colors = combine_points(preds, views, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                    min_conf_thr_percentile=min_conf_thr_percentile, flip_axes=flip_axes, sample=sample)
    dev = _lib.work_device(preds[0]["conf"], "preds")
    on_dev = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in p.items() if k in ("pts3d_in_other_view", "conf")} for p in preds]
    poses_c2w, focals = estimate_camera_poses(on_dev, niter_PnP=niter_PnP)
    poses_c2w, focals = poses_c2w[sample], focals[sample]
    if flip_axes:
        poses_c2w = [FLIP @ np.asarray(p, dtype=np.float64) for p in poses_c2w]
    cam_size = auto_cam_size(poses_c2w)
    cam_size = 0.05 if not cam_size >= 0.05 else cam_size                                 # max(auto, 0.05); a lone camera's nan gives 0.05
    viz = SceneViz(dev)
    if points is not None:
        viz.points.append(points)
        viz.colors.append(colors)
        if export_ply_path:
            save_ply(export_ply_path, points, colors)
    for i, pose in enumerate(poses_c2w):
        viz.add_camera(pose, focals[i], color=CAM_COLORS[i % len(CAM_COLORS)], image=views[i]["img"][sample], cam_size=cam_size)
    picture = viz.render(camera, width=width, height=height, point_size=point_size)
    if output_path is not None:
        _save_png(picture.cpu().numpy(), output_path)
    return picture


__all__ = ["CAM_COLORS", "SceneViz", "auto_cam_size", "camera_faces", "camera_image_size", "camera_meshes", "camera_vertices", "image_grid",
           "plot_3d_points_with_estimated_camera_poses", "render_mesh"]
