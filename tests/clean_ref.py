"""The restatement of the confidence cleaning (fast3r_amd/csrc/f3r_clean.hip, include/f3r.h "cross-view occlusion filter") in torch on the
CPU, in our own words.  `clean_ref` performs the kernel's arithmetic as separate elementwise tensor operations in the kernel's order, so in
float32 every intermediate is the kernel's, bit for bit; with dtype=torch.float64 it is the witness.  `margins` measures in float64 how far
every decision lies from its boundary.  The pose inverse is the closed form of the kernel in float64 numpy."""
import numpy as np
import torch


def pose_inverse(poses):
    """(N, 4, 4) camera-to-world -> (N, 3, 4) float64 world-to-camera: the cofactor inverse of the 3 x 3 block and -A^-1 t, every operation
    in the kernel's order"""
    P = np.asarray(poses).astype(np.float64)
    out = np.zeros((len(P), 3, 4))
    for n, M in enumerate(P):
        a, t = M[:3, :3], M[:3, 3]
        co = np.empty((3, 3))
        co[0, 0] = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]
        co[0, 1] = a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]
        co[0, 2] = a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]
        co[1, 0] = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]
        co[1, 1] = a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]
        co[1, 2] = a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]
        co[2, 0] = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]
        co[2, 1] = a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]
        co[2, 2] = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
        det = (a[0, 0] * co[0, 0] + a[0, 1] * co[1, 0]) + a[0, 2] * co[2, 0]
        with np.errstate(all="ignore"):
            for r in range(3):
                inv = [co[r, c] / det for c in range(3)]
                out[n, r, :3] = inv
                out[n, r, 3] = -((inv[0] * t[0] + inv[1] * t[1]) + inv[2] * t[2])
    return out


def _affine(m, x, y, z):
    """((m0 x + m1 y) + m2 z) + m3 for the three rows of m (.., 3, 4): each product and sum a tensor operation of its own.  With m (J, 3, 4)
    and x, y, z (n, 1) the result is (n, J): the same operations on every (pixel, neighbour) couple"""
    return [((m[..., r, 0] * x + m[..., r, 1] * y) + m[..., r, 2] * z) + m[..., r, 3] for r in range(3)]


def _project(m, k, x, y, z):
    X, Y, Z = _affine(m, x, y, z)
    u = (k[..., 0] * X + k[..., 2] * Z) / Z
    v = (k[..., 1] * Y + k[..., 3] * Z) / Z
    return X, Y, Z, u, v


def _setup(s, dtype, frame):
    f64 = dtype == torch.float64
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    inv = pose_inverse(s["poses"])
    cams = torch.from_numpy(inv if f64 else inv.astype(np.float32)).to(dtype)
    poses, intr = t(s["poses"]), t(s["intr"])
    pts = []
    for i, p in enumerate(s["local"] if frame == "camera" else s["world"]):
        x, y, z = t(p).reshape(-1, 3).unbind(1)
        if frame == "camera":
            x, y, z = _affine(poses[i], x, y, z)
        pts.append((x, y, z))
    omt = 1.0 - float(s["tol"])
    omt = torch.tensor(omt if f64 else float(np.float32(omt)), dtype=dtype)
    return cams, intr, pts, [t(c).reshape(-1) for c in s["conf"]], [t(d).reshape(-1) for d in s["depth"]], omt


def clean_ref(s, nbrs=None, *, frame="world", dtype=torch.float32, jacobi=False):
    """s: a scene of tests/clean_cases.py with tol and max_bad_conf; nbrs: neighbour lists (default: every other view).  frame="camera" reads
    s["local"] and applies the pose first.  jacobi: compare with the input confidences only (NOT the contract: the order case shows the
    difference).  The views are taken in ascending order; inside a view every (pixel, neighbour) couple is one element of the same tensor
    operations.  -> (the cleaned (H, W) confidences in `dtype`, n_lowered per view)."""
    N = len(s["shapes"])
    nbrs = [[j for j in range(N) if j != i] for i in range(N)] if nbrs is None else nbrs
    cams, intr, pts, conf, depth, omt = _setup(s, dtype, frame)
    max_bad = torch.tensor(float(s["max_bad_conf"]), dtype=dtype)
    Hs, Ws = (torch.tensor([sh[k] for sh in s["shapes"]], dtype=torch.int64) for k in (0, 1))
    off = torch.cumsum(Hs * Ws, 0) - Hs * Ws
    depth_all, conf_all = torch.cat(depth), torch.cat(conf)
    res_all = conf_all.clone()
    lowered = []
    for i in range(N):
        if len(nbrs[i]) == 0:
            lowered.append(0)
            continue
        J = torch.tensor(nbrs[i], dtype=torch.int64)
        x, y, z = (a[:, None] for a in pts[i])
        c = conf[i]
        _, _, Z, u, v = _project(cams[J], intr[J], x, y, z)
        ur, vr = torch.round(u), torch.round(v)  # half to even, as rintf
        cone = (Z > 0) & (ur >= 0) & (ur < Ws[J].to(dtype)) & (vr >= 0) & (vr < Hs[J].to(dtype))
        zero = torch.zeros_like(ur)
        e = off[J] + torch.where(cone, vr, zero).to(torch.int64) * Ws[J] + torch.where(cone, ur, zero).to(torch.int64)
        other = conf_all if jacobi else res_all
        bad = (cone & (Z < omt * depth_all[e]) & (c[:, None] < other[e])).any(1)
        new = torch.where(bad, torch.minimum(c, max_bad), c)
        lowered.append(int((bad & (new != c)).sum()))
        res_all[off[i]:off[i] + c.numel()] = new
    return [res_all[off[i]:off[i] + h * w].reshape(h, w).clone() for i, (h, w) in enumerate(s["shapes"])], lowered


def pixel_shift(s, ref_uv32, ref_uv64):
    """d of the margin conditions: the largest |u or v of the fp32 run - of the fp64 run| over the near-cone triples, from two lists
    {(i, j): (u, v)} of projections"""
    d = 0.0
    for key, (u64, v64) in ref_uv64.items():
        H, W = s["shapes"][key[1]]
        u32, v32 = ref_uv32[key]
        near = np.isfinite(u64) & np.isfinite(v64) & (u64 >= -1) & (u64 <= W) & (v64 >= -1) & (v64 <= H)
        if near.any():
            d = max(d, float(np.abs(u32.astype(np.float64) - u64)[near].max()), float(np.abs(v32.astype(np.float64) - v64)[near].max()))
    return d


def projections(s, dtype):
    """{(i, j): (u, v, Z)} as numpy, by the restatement in `dtype` over the complete graph"""
    cams, intr, pts, _, _, _ = _setup(s, dtype, "world")
    out = {}
    N = len(s["shapes"])
    for i in range(N):
        for j in range(N):
            if i != j:
                with np.errstate(all="ignore"):
                    _, _, Z, u, v = _project(cams[j], intr[j], *pts[i])
                out[(i, j)] = (u.numpy(), v.numpy(), Z.numpy())
    return out


def margins(s, d, nbrs=None, factor=16.0, rel_depth=1e-5):
    """In float64, per view: `px`: per pixel the smallest distance of u or v of any of its near-cone triples (Z > 0, -1 <= u <= W, -1 <= v <= H)
    to a half-integer; `rel`: the smallest |Z - (1 - tol) d_j| / |Z| over its in-cone triples; `absz`: the smallest |Z| over all its triples;
    `fragile`: px < factor d, or rel < rel_depth, or absz < factor d (in depth units); `tainted`: fragile, or in front (in cone and
    Z < (1 - tol) d_j) of a tainted pixel of an earlier view."""
    N = len(s["shapes"])
    nbrs = [[j for j in range(N) if j != i] for i in range(N)] if nbrs is None else nbrs
    cams, intr, pts, _, depth, omt = _setup(s, torch.float64, "world")
    out = {"px": [], "rel": [], "absz": [], "fragile": [], "tainted": []}
    for i in range(N):
        n = pts[i][0].numel()
        px, rel, absz = torch.full((n,), np.inf, dtype=torch.float64), torch.full((n,), np.inf, dtype=torch.float64), torch.full((n,), np.inf, dtype=torch.float64)
        hit = torch.zeros(n, dtype=torch.bool)
        for j in nbrs[i]:
            H, W = s["shapes"][j]
            _, _, Z, u, v = _project(cams[j], intr[j], *pts[i])
            absz = torch.minimum(absz, torch.nan_to_num(Z.abs(), nan=0.0))
            near = (Z > 0) & (u >= -1) & (u <= W) & (v >= -1) & (v <= H)
            half = lambda a: ((a - 0.5) - torch.round(a - 0.5)).abs()  # noqa: E731
            px = torch.where(near, torch.minimum(px, torch.minimum(half(u), half(v))), px)
            ur, vr = torch.round(u), torch.round(v)
            cone = (Z > 0) & (ur >= 0) & (ur < W) & (vr >= 0) & (vr < H)
            e = torch.where(cone, vr * W + ur, torch.zeros_like(ur)).to(torch.int64)
            lim = omt * depth[j][e]
            rel = torch.where(cone, torch.minimum(rel, torch.nan_to_num((Z - lim).abs() / Z.abs(), nan=0.0)), rel)
            if j < i:
                hit |= cone & (Z < lim) & out["tainted"][j].reshape(-1)[e]
        fragile = (px < factor * d) | (rel < rel_depth) | (absz < factor * d)
        shape = s["shapes"][i]
        for k, a in (("px", px), ("rel", rel), ("absz", absz), ("fragile", fragile), ("tainted", fragile | hit)):
            out[k].append(a.reshape(shape))
    return out
