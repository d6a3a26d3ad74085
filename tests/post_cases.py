"""Seeded cases of the three oldest post-forward kernels at the edges of their geometry -- the quantile threshold and the similarity solve of
f3r_align_local_to_global, f3r_estimate_focal (csrc/f3r_post.hip, f3r_post_common.h, f3r_linalg.h) and f3r_estimate_poses (csrc/f3r_pnp.hip,
f3r_sqpnp.h) -- with their float64 references and the guarded placement of their device buffers; shared by tests/test_post_cases.py (no GPU:
the references meet the tolerances, the cases reach the branches they are there for, wrong restatements miss) and
tests/test_post_geometry_gpu.py (the kernels, through the C ABI, against the references).

The references are the ones the project already trusts: torch.quantile, oracle/align_oracle.py and oracle/align_pin.horn_similarity in
float64 on the fp32 inputs the kernel sees, oracle/focal_oracle.py, oracle/pnp_oracle.py, oracle/sqpnp.py and oracle/cv2_stub.py.  A builder
returns CPU tensors only.  The `run_*` functions at the end own every device buffer of a launch: operands inside 0xFF bytes (NaN as fp32, true as
a mask byte), outputs and workspaces between sentinel words; they assert the guards before they hand any value back.
"""
import dataclasses
import functools
import math

import numpy as np
import torch

from conv_cases import guarded_operand
from gemm_cases import Guarded, guards_intact, strided_out
from oracle import align_oracle, focal_oracle, pnp_oracle, sqpnp
from oracle.align_pin import horn_similarity

F32, F64 = torch.float32, torch.float64
PNT = 1024                                   # threads of a problem workgroup (f3r_post.hip: PNT, f3r_pnp.hip: PT)
ORTHO_TOL = 1e-5                             # |R^T R - I|, fp32 rts: the rounding of a 3 x 3 product of fp32 entries
HORN_R_TOL, HORN_S_TOL, HORN_T_TOL = 2e-6, 2e-6, 1e-5     # test_hip_alignment_matches_the_independent_pin
ALIGN_PTS_TOL = 2e-5                         # aligned points over the output scale
FOCAL_TOL = 5e-5                             # tests/test_focal.py
POSE_TOL = 1e-4                              # tests/test_pnp.py: HIP vs pnp_oracle
REPROJ_THR = 5.0


def _gen(*key):
    s = 54321
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def f32(x):
    """a Python number as the float the C ABI hands to the kernel"""
    return float(np.float32(x))


def same_f32(a, b):
    """bit-equal, or both a zero (-0.0 == +0.0), or both NaN (inf - inf inside the lerp: the payload is the machine's)"""
    a, b = a.reshape(-1).float().cpu(), b.reshape(-1).float().cpu()
    bits = a.view(torch.int32) == b.view(torch.int32)
    return bool((bits | ((a == 0) & (b == 0)) | (torch.isnan(a) & torch.isnan(b))).all())


def random_rotation(g):
    q, _ = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=F64))
    if torch.det(q) < 0:
        q[:, 0] *= -1
    return q


def ortho_err(R):
    R = R.double()
    return float((R.t() @ R - torch.eye(3, dtype=F64)).abs().max())


# ================================================================================================ quantile threshold
Q_NPIX = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2049)
Q_ROWS = ("rand", "equal", "ties100", "low10", "mid11", "top11", "negative", "zeros", "subnormal", "inf")


def quantile_qs(n):
    """q = 0, 1 / (n - 1), 0.5, 0.85, 1 - 2^-20, 1, and one whose rank q (n - 1) is a whole number inside the row (n - 1 a multiple of 4)"""
    qs = [0.0, 0.5, 0.85, 1.0 - 2.0 ** -20, 1.0]
    if n > 1:
        qs.append(1.0 / (n - 1))
    if n > 4 and (n - 1) % 4 == 0:
        qs.append(0.25)
    return sorted({f32(q) for q in qs})


def _from_bits(b):
    return b.to(torch.int32).view(F32)


def quantile_row(kind, n, q=0.5):
    """one confidence row of n values.  The three radix passes of select_kth take bits 31..21, 20..10 and 9..0 of the order-preserving key, so
    'top11' / 'mid11' / 'low10' hold values that differ in that field only: a pass that mishandles its field returns another order statistic."""
    g = _gen(1, Q_ROWS.index(kind), n)
    base = torch.full((n,), 1.5).view(torch.int32)
    if kind == "rand":
        return 1 + torch.exp(torch.randn(n, generator=g))
    if kind == "equal":
        return torch.full((n,), 1.5)
    if kind == "ties100":                      # up to 100 equal values whose run straddles the cut at rank q (n - 1)
        x = (1 + torch.rand(n, generator=g)).sort().values
        k = int(q * (n - 1))
        lo = max(0, k - 50)
        x[lo:lo + 100] = x[k]
        return x[torch.randperm(n, generator=g)]
    if kind == "low10":
        return _from_bits(base | torch.randint(0, 1 << 10, (n,), generator=g, dtype=torch.int32))
    if kind == "mid11":
        return _from_bits(base | (torch.randint(0, 1 << 11, (n,), generator=g, dtype=torch.int32) << 10))
    if kind == "top11":                        # sign, exponent (1 .. 190: finite, and no overflow in vhi - vlo), two mantissa bits
        sign = torch.randint(0, 2, (n,), generator=g, dtype=torch.int64) << 31
        expo = torch.randint(1, 191, (n,), generator=g, dtype=torch.int64) << 23
        mant = torch.randint(0, 4, (n,), generator=g, dtype=torch.int64) << 21
        v = sign | expo | mant
        return _from_bits(torch.where(v >= 2 ** 31, v - 2 ** 32, v))
    if kind == "negative":
        return torch.randn(n, generator=g) * 3 - 1
    if kind == "zeros":                        # -0.0 next to +0.0 around the cut, a few other values at either end
        x = torch.zeros(n)
        x[torch.rand(n, generator=g) < 0.5] = -0.0
        m = max(n // 8, 0)
        x[:m] = -1 - torch.rand(m, generator=g)
        x[n - m:] = 1 + torch.rand(m, generator=g)
        return x[torch.randperm(n, generator=g)]
    if kind == "subnormal":
        return _from_bits(torch.randint(1, 1 << 23, (n,), generator=g, dtype=torch.int32))
    if kind == "inf":
        x = 1 + torch.exp(torch.randn(n, generator=g))
        x[torch.rand(n, generator=g) < 0.25] = float("inf")
        return x
    raise ValueError(kind)


def quantile_rows(n, q):
    """[len(Q_ROWS)][n]: every kind of row, solved as the problems of ONE launch"""
    return torch.stack([quantile_row(k, n, q) for k in Q_ROWS])


def quantile_ref(rows, q, interpolation="linear"):
    return torch.quantile(rows, f32(q), dim=1, interpolation=interpolation)


# ================================================================================================ alignment
@dataclasses.dataclass(frozen=True)
class AlignCase:
    id: str
    npix: int
    n_prob: int = 1
    masked: bool = False
    q: float = 0.0
    kind: str = "shape"       # "shape" | a fall-back | a cloud
    path: str = ""            # expected route per problem: "A" conf & valid, "B" valid only, "I" identity ("" = whatever the data give)


ALIGN_SHAPES = [AlignCase(f"n{n}-p{p}-{'mask' if m else 'all'}-q{q:g}", n, p, m, q) for n in (1, 2, 3, 4, 1023, 1025) for p in (1, 3) for m in (False, True)
                for q in (0.0, 0.85)]
ALIGN_FALLBACKS = [AlignCase("two-confident", 64, 1, True, 0.85, "two-confident", "B"), AlignCase("three-confident", 64, 1, True, 0.85, "three-confident", "A"),
                   AlignCase("two-valid", 64, 1, True, 0.0, "two-valid", "I"), AlignCase("none-valid", 64, 1, True, 0.0, "none-valid", "I"),
                   AlignCase("tie-at-threshold", 65, 1, False, 0.5, "tie", "A")]
CLOUD_N, CLOUD_OFF = 400, 40                 # masked points of a cloud, and pixels outside the mask that lie off its plane / line
ALIGN_CLOUDS = ("plane", "plane-offset", "line", "line-offset", "mirrored", "axis-planar", "far")
ROTATION_DETERMINED = ("plane", "plane-offset", "mirrored", "axis-planar", "far")
FAR_OFFSETS = (10.0, 100.0, 1000.0)
CLOUD_SEED = {"plane": 1}          # seeds at which the parent commit's header fails every tilted cloud (docs/parity.md)
FAR_OFFSET = 1000.0                          # the largest of FAR_OFFSETS at which the float64 raw-moment restatement meets the Horn bounds (test_post_cases.py)


def build_align(c):
    """conf [P][n], loc / glob [P][n][3] fp32, valid [P][n] bool or None"""
    g = _gen(2, c.npix, c.n_prob, c.masked, int(c.q * 100), len(c.kind))
    P, n = c.n_prob, c.npix
    glob = torch.randn(P, n, 3, generator=g) * 2.0 + torch.tensor([0.5, -1.0, 4.0])
    loc = torch.empty_like(glob)
    for p in range(P):
        R, s, t = random_rotation(g).float(), float(0.5 + 2 * torch.rand(1, generator=g)), torch.randn(3, generator=g)
        loc[p] = ((glob[p] - t) @ R) / s + 0.02 * torch.randn(n, 3, generator=g)
    conf = 1 + torch.exp(torch.randn(P, n, generator=g))
    valid = (torch.rand(P, n, generator=g) > 0.3) if c.masked else None
    if c.kind in ("two-confident", "three-confident"):
        keep = 2 if c.kind == "two-confident" else 3
        thr = torch.quantile(conf[0], f32(c.q))
        top = torch.nonzero(conf[0] >= thr).reshape(-1)
        valid[0, top] = False
        valid[0, top[:keep]] = True
    elif c.kind == "two-valid":
        valid[:] = False
        valid[0, [5, 40]] = True
    elif c.kind == "none-valid":
        valid[:] = False
    elif c.kind == "tie":                      # rank 32 of 65 is a whole number: thr = 2.0 exactly, held by ten pixels whose points pull the solve
        conf[0, :30], conf[0, 30:40], conf[0, 40:] = 1.0, 2.0, 3.0
        loc[0, 30:40] += 0.5 * torch.randn(10, 3, generator=g)
        perm = torch.randperm(n, generator=g)
        conf, loc, glob = conf[:, perm], loc[:, perm], glob[:, perm]
    return dict(conf=conf.contiguous(), loc=loc.contiguous(), glob=glob.contiguous(), valid=valid)


def align_path(conf, valid, q, strict=False):
    """the route of one problem: 'A' (>= 3 confident and valid points), 'B' (>= 3 valid), 'I'.  strict: the mask with > (what the kernel must NOT do)"""
    thr = torch.quantile(conf, f32(q))
    v = torch.ones_like(conf, dtype=torch.bool) if valid is None else valid
    a = ((conf > thr) if strict else (conf >= thr)) & v
    return "A" if int(a.sum()) >= 3 else ("B" if int(v.sum()) >= 3 else "I")


def align_ref(d, q):
    """oracle/align_oracle.py in float64 on the fp32 inputs -> aligned points [P][n][3] float64 (the reference takes a percentile: q * 100)"""
    P, n = d["conf"].shape
    preds = [{"pts3d_local": d["loc"].double().view(P, 1, n, 3), "conf_local": d["conf"].view(P, 1, n),
              "pts3d_in_other_view": d["glob"].double().view(P, 1, n, 3), "conf": d["conf"].view(P, 1, n)}]
    views = [{} if d["valid"] is None else {"valid_mask": d["valid"].view(P, 1, n)}]
    pct = round(q * 100)
    assert f32(pct / 100.0) == f32(q)
    return align_oracle.align_local_pts3d_to_global(preds, views, min_conf_thr_percentile=pct)[0]["pts3d_local_aligned_to_global"].view(P, n, 3)


def align_restate(d, q, strict=False, skip_valid_fallback=False, solver=None):
    """the method's control flow on one launch's data, float64; strict / skip_valid_fallback are the two wrong variants"""
    solver = solver or align_oracle.rigid_points_registration
    outs = []
    for p in range(d["conf"].shape[0]):
        conf, x, y = d["conf"][p], d["loc"][p].double(), d["glob"][p].double()
        v = torch.ones_like(conf, dtype=torch.bool) if d["valid"] is None else d["valid"][p]
        thr = torch.quantile(conf, f32(q))
        m = ((conf > thr) if strict else (conf >= thr)) & v
        if int(m.sum()) < 3 and not skip_valid_fallback:
            m = v
        if int(m.sum()) < 3:
            outs.append(x.clone())
            continue
        R, t, s = solver(x[m], y[m])
        outs.append(s * (x @ R.t()) + t)
    return torch.stack(outs)


def cloud(kind, offset=None, seed=None):
    """(x, y, mask): CLOUD_N masked fp32 points with y = 1.3 R x + t exactly in float64 before the rounding, followed by CLOUD_OFF pixels outside
    the mask that lie off the plane / line -- the kernel transforms them too, and a rank-2 'rotation' would flatten them"""
    g = _gen(3, ALIGN_CLOUDS.index(kind), CLOUD_SEED.get(kind, 0) if seed is None else seed)
    n = CLOUD_N + CLOUD_OFF
    Q = random_rotation(g)                     # tilts the plane / line out of the axes
    R = random_rotation(g)
    ab = torch.randn(n, 3, generator=g, dtype=F64) * torch.tensor([2.0, 1.0, 0.5], dtype=F64)
    if kind.startswith("plane") or kind == "axis-planar":
        ab[:CLOUD_N, 2] = 0.0
    if kind.startswith("line"):
        ab[:CLOUD_N, 1:] = 0.0
    x = ab if kind == "axis-planar" else ab @ Q.t()
    if kind.endswith("-offset"):
        x = x + torch.tensor([30.0, -32.0, 24.0], dtype=F64)   # |offset| = 50
    if kind == "far":
        off = FAR_OFFSET if offset is None else offset
        x = x + off * torch.tensor([0.6, -0.64, 0.48], dtype=F64)
    y = 1.3 * x @ R.t() + torch.tensor([0.4, -1.0, 3.0], dtype=F64)
    if kind == "mirrored":                     # the unconstrained optimum is a reflection: the determinant correction decides
        y = 0.7 * (x * torch.tensor([1.0, 1.0, -1.0], dtype=F64)) @ R.t() + 0.01 * torch.randn(n, 3, generator=g, dtype=F64)
    mask = torch.zeros(n, dtype=torch.bool)
    mask[:CLOUD_N] = True
    return x.float(), y.float(), mask


def umeyama_raw_moments(x, y, det_correction=True):
    """similarity_from_moments restated in float64 with torch's SVD: RAW moments (sum y x^T - n ym xm^T), results rounded to fp32 as rts is.
    det_correction=False: plain Procrustes, what the kernel must NOT do (a mirrored cloud then gets a reflection)"""
    x, y = x.double(), y.double()
    n = x.shape[0]
    xm, ym = x.sum(0) / n, y.sum(0) / n
    M = y.t() @ x - n * torch.outer(ym, xm)
    sx2 = (x * x).sum() - n * (xm * xm).sum()
    U, S, Vh = torch.linalg.svd(M)
    d = float(torch.sign(torch.linalg.det(U) * torch.linalg.det(Vh))) if det_correction else 1.0
    D = torch.tensor([1.0, 1.0, d], dtype=F64)
    R = U @ torch.diag(D) @ Vh
    s = (S * D).sum() / sx2
    t = ym - s * (R @ xm)
    return R.float().double(), t.float().double(), s.float().double()


def umeyama_plain(x, y):
    return umeyama_raw_moments(x, y, det_correction=False)


def horn_misses(R, t, s, x, y, mask, kind):
    """which of the bounds a solve (R, t, s) of cloud (x, y, mask) misses -> list of (name, figure, bound); empty = all met"""
    Rh, th, sh = horn_similarity(x[mask], y[mask])
    R, t, s = R.double(), t.double(), float(s)
    out = [("ortho", ortho_err(R), ORTHO_TOL), ("det", abs(float(torch.det(R)) - 1.0), ORTHO_TOL), ("scale", abs(s - float(sh)) / float(sh), HORN_S_TOL)]
    if kind in ROTATION_DETERMINED:
        out += [("R", float((R - Rh).abs().max()), HORN_R_TOL), ("t", float((t - th).abs().max()), HORN_T_TOL)]
        ref, got = sh * x.double() @ Rh.t() + th, s * x.double() @ R.t() + t           # ALL pixels, the off-plane ones included
    else:
        ref, got = (sh * x.double() @ Rh.t() + th)[mask], (s * x.double() @ R.t() + t)[mask]
    out.append(("points", float((got - ref).abs().max()) / float(ref.abs().max()), ALIGN_PTS_TOL))
    return [(k, v, b) for k, v, b in out if not v <= b]


# ================================================================================================ focal
@dataclasses.dataclass(frozen=True)
class FocalCase:
    id: str
    H: int
    W: int
    q: float = 0.1
    n_iter: int = 10
    pp: tuple = None          # None: (W / 2, H / 2)
    rng: tuple = (0.0, 3.0e38)   # (min_focal, max_focal)
    kind: str = "scene"       # "scene" | "nan-thr" | "z0-all" | "z0-some"
    frac: float = 0.9         # scene focal / focal_base

    @property
    def ppxy(self):
        return (self.W / 2, self.H / 2) if self.pp is None else self.pp

    @property
    def base(self):
        return max(self.H, self.W) / (2 * math.tan(math.radians(30)))


FOCAL_HW = ((1, 1), (1, 9), (9, 1), (5, 7), (31, 33))
FOCAL = ([FocalCase(f"{h}x{w}-it{it}", h, w, n_iter=it) for h, w in FOCAL_HW for it in (0, 1, 10)]
         + [FocalCase(f"{h}x{w}-q0", h, w, q=0.0) for h, w in FOCAL_HW] + [FocalCase(f"{h}x{w}-q1", h, w, q=1.0) for h, w in FOCAL_HW]
         + [FocalCase("5x7-pp", 5, 7, pp=(2.25, 3.5)), FocalCase("31x33-pp", 31, 33, pp=(20.5, 11.25)),
            FocalCase("31x33-bounded", 31, 33, rng=(0.5, 1.5)), FocalCase("31x33-clamp-lo", 31, 33, rng=(1.2, 2.0)), FocalCase("31x33-clamp-hi", 31, 33, rng=(0.25, 0.75)),
            FocalCase("5x7-nan-thr", 5, 7, q=1.0, kind="nan-thr"), FocalCase("5x7-z0-all", 5, 7, kind="z0-all"), FocalCase("31x33-z0-all", 31, 33, kind="z0-all"),
            FocalCase("5x7-z0-some", 5, 7, kind="z0-some"), FocalCase("31x33-z0-some", 31, 33, kind="z0-some")])
FOCAL_BATCH = ("31x33-it10", "31x33-z0-some", "31x33-pp")     # three views of one launch (the third one's principal point is the launch's)


def build_focal(c, pp=None):
    g = _gen(4, c.H, c.W, int(c.q * 100), c.n_iter, len(c.kind), int(c.frac * 100))
    ppx, ppy = c.ppxy if pp is None else pp
    f = c.frac * c.base
    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=F32), torch.arange(c.W, dtype=F32), indexing="ij")
    z = 2 + 3 * torch.rand(c.H, c.W, generator=g)
    pts = torch.stack([(xs - ppx) * z / f, (ys - ppy) * z / f, z], -1) + 0.01 * torch.randn(c.H, c.W, 3, generator=g)
    conf = 1 + 4 * torch.rand(c.H, c.W, generator=g)
    if c.kind == "nan-thr":                    # the largest key is a NaN: rank n - 1 (q = 1) picks it, and nothing is >= NaN
        conf[2, 3] = float("nan")
    if c.kind == "z0-all":
        pts[..., 2] = 0.0
    if c.kind == "z0-some":                    # x / 0 = +-inf and 0 / 0 = NaN among kept points: nan_to_num makes them 0
        idx = torch.randperm(c.H * c.W, generator=g)[:max(3, c.H * c.W // 10)]
        pts.view(-1, 3)[idx, 2] = 0.0
        pts.view(-1, 3)[idx[0], :2] = 0.0
        conf.view(-1)[idx] = 5.5               # above every threshold but q = 1's
    return dict(pts=pts.contiguous(), conf=conf.contiguous())


def focal_ref(c, d, pp=None, nan_to_num=True):
    """(focal, threshold): torch.quantile + oracle/focal_oracle.py on the fp32 inputs.  nan_to_num=False: the ratios as they come (what the kernel
    must NOT do: one Z == 0 poisons the estimate)"""
    thr = torch.quantile(d["conf"].reshape(-1), f32(c.q))
    mask = (d["conf"] >= thr)[None]
    ppt = torch.tensor([c.ppxy if pp is None else pp], dtype=F32)
    lo, hi = c.rng
    hi = math.inf if hi >= 3.0e38 else hi
    if nan_to_num:
        return float(focal_oracle.estimate_focal_knowing_depth_and_confidence_mask(d["pts"][None], ppt, mask, lo, hi, c.n_iter)), thr
    orig = torch.Tensor.nan_to_num
    try:
        torch.Tensor.nan_to_num = lambda self, *a, **k: self
        return float(focal_oracle.estimate_focal_knowing_depth_and_confidence_mask(d["pts"][None], ppt, mask, lo, hi, c.n_iter)), thr
    finally:
        torch.Tensor.nan_to_num = orig


# ================================================================================================ PnP
@dataclasses.dataclass(frozen=True)
class PnpCase:
    id: str
    H: int
    W: int
    mask: object = "all"       # "all" | int (that many random pixels) | "first10" | "last-row"
    focal: str = "given"       # "given" | "search"
    n_iter: int = 100
    n_focals: int = 100
    k_focal: int = 40          # the scene focal is np.geomspace(S / 2, 3 S, n_focals)[k_focal]
    pp: tuple = None
    conf_thr: float = 1.0
    n_out: int = 0             # gross outliers among the masked points
    seed: int = 0

    @property
    def S(self):
        return max(self.H, self.W)

    @property
    def grid(self):
        return np.geomspace(self.S / 2, self.S * 3, self.n_focals)

    @property
    def f(self):
        return float(self.grid[min(self.k_focal, self.n_focals - 1)])

    @property
    def ppxy(self):
        return (self.W / 2, self.H / 2) if self.pp is None else self.pp

    @property
    def few(self):
        return isinstance(self.mask, int) and self.mask in (4, 5)


PNP_HW = ((5, 7), (7, 5), (1, 40), (31, 33), (48, 64))


def _pnp_cases():
    out = []
    for h, w in PNP_HW:
        for m in (4, 5, 6, 7, 8, 12, "all"):
            if isinstance(m, int) and m > h * w:
                continue
            out.append(PnpCase(f"{h}x{w}-m{m}-given", h, w, m))
    out += [PnpCase(f"{h}x{w}-m{m}-search", h, w, m, "search") for h, w in ((5, 7), (31, 33), (48, 64)) for m in (4, 5)]
    out += [PnpCase(f"{h}x{w}-all-search", h, w, "all", "search") for h, w in ((31, 33), (48, 64))]
    out += [PnpCase("48x64-first10", 48, 64, "first10"), PnpCase("48x64-last-row", 48, 64, "last-row"), PnpCase("31x33-last-row", 31, 33, "last-row")]
    out += [PnpCase(f"31x33-iter{it}", 31, 33, n_iter=it) for it in (1, 2, 32)] + [PnpCase(f"31x33-iter{it}-search", 31, 33, focal="search", n_iter=it) for it in (1, 2)]
    out += [PnpCase(f"31x33-nf{nf}-search", 31, 33, focal="search", n_focals=nf, k_focal=0) for nf in (1, 2)]
    out += [PnpCase("31x33-m4-nf2-search", 31, 33, 4, "search", n_focals=2, k_focal=1), PnpCase("5x7-m5-nf1-search", 5, 7, 5, "search", n_focals=1, k_focal=0)]
    out += [PnpCase("31x33-pp", 31, 33, pp=(20.5, 11.25)), PnpCase("31x33-pp-search", 31, 33, focal="search", pp=(20.5, 11.25)), PnpCase("31x33-m5-pp", 31, 33, 5, pp=(20.5, 11.25))]
    out += [PnpCase("31x33-thr2.5", 31, 33, 12, conf_thr=2.5), PnpCase("31x33-m4-thr0", 31, 33, 4, conf_thr=0.0)]
    out += [PnpCase(f"{h}x{w}-outliers", h, w, n_out=h * w // 10, seed=1) for h, w in ((31, 33), (48, 64))]
    out += [PnpCase(f"31x33-m{m}-fails", 31, 33, m) for m in (0, 1, 3)]
    return out


PNP = _pnp_cases()
PNP_BATCH = ("31x33-m3-fails", "31x33-mall-given", "31x33-m4-given", "31x33-outliers")     # failing, ordinary, four points, outliers: one launch
PNP_MIXED = ("31x33-mall-given", "31x33-all-search", "31x33-m5-given")                      # focal_in: positive | <= 0 | positive


def pnp_case(case_id):
    return next(c for c in PNP if c.id == case_id)


def build_pnp(c):
    """a world pointmap seen by a camera of focal c.f.  conf is conf_thr + 1 on the mask and EXACTLY conf_thr elsewhere, on points that fit the camera
    as well as the masked ones: a mask taken with >= counts them all"""
    g = _gen(5, c.H, c.W, c.seed, c.mask if isinstance(c.mask, int) else 1000 + ("all", "first10", "last-row").index(c.mask), int(c.f * 100))
    ppx, ppy = c.ppxy
    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=F64), torch.arange(c.W, dtype=F64), indexing="ij")
    z = 2 + 3 * torch.rand(c.H, c.W, generator=g, dtype=F64)
    Xc = torch.stack([(xs - ppx) * z / c.f, (ys - ppy) * z / c.f, z], -1)
    R, t = random_rotation(g), torch.randn(3, generator=g, dtype=F64)
    Xw = (Xc - t) @ R
    npix = c.H * c.W
    if c.mask == "all":
        m = torch.ones(npix, dtype=torch.bool)
    elif c.mask == "first10":
        m = torch.arange(npix) < 10
    elif c.mask == "last-row":
        m = torch.arange(npix) >= npix - c.W
    else:
        m = torch.zeros(npix, dtype=torch.bool)
        m[torch.randperm(npix, generator=g)[:c.mask]] = True
    if c.n_out:
        idx = torch.nonzero(m).reshape(-1)
        idx = idx[torch.randperm(len(idx), generator=g)[:c.n_out]]
        Xw.view(-1, 3)[idx] += torch.randn(c.n_out, 3, generator=g, dtype=F64)
    T = torch.eye(4, dtype=F64)
    T[:3, :3], T[:3, 3] = R.t(), -R.t() @ t
    conf = torch.where(m, torch.tensor(c.conf_thr + 1.0), torch.tensor(float(c.conf_thr))).view(c.H, c.W).float()
    return dict(pts=Xw.float().contiguous(), conf=conf.contiguous(), T=T, mask=m.view(c.H, c.W))


@functools.lru_cache(maxsize=None)
def pnp_ref(case_id, ge_mask=False):
    """(focal | None, cam-to-world | None, inliers): oracle/pnp_oracle.fast_pnp on the fp32 inputs + the float64 recount.  ge_mask: the mask taken
    with >= (what the kernel must NOT do)"""
    c = pnp_case(case_id)
    d = build_pnp(c)
    msk = (d["conf"] >= c.conf_thr) if ge_mask else (d["conf"] > c.conf_thr)
    f, T = pnp_oracle.fast_pnp(d["pts"], c.f if c.focal == "given" else None, msk, pp=c.ppxy, num_guessed_focals=c.n_focals, niter_PnP=c.n_iter)
    if T is None:
        return None, None, 0
    return f, T, recount(c, d["pts"], msk, T, f)[0]


def recount(c, pts, msk, T, f):
    """float64: (masked points within 5 px and in front of the camera under cam-to-world T and focal f, largest reprojection error of the masked points, min z)"""
    T = T.double()
    R, t = T[:3, :3].t(), -T[:3, :3].t() @ T[:3, 3]
    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=F64), torch.arange(c.W, dtype=F64), indexing="ij")
    m = msk.reshape(-1)
    Xc = pts.double().reshape(-1, 3)[m] @ R.t() + t
    u, v = float(f) * Xc[:, 0] / Xc[:, 2] - (xs.reshape(-1)[m] - c.ppxy[0]), float(f) * Xc[:, 1] / Xc[:, 2] - (ys.reshape(-1)[m] - c.ppxy[1])
    e = (u * u + v * v).sqrt()
    return int(((e <= REPROJ_THR) & (Xc[:, 2] > 0)).sum()), float(e.max()), float(Xc[:, 2].min())


def sqpnp_on_mask(c, d):
    """cam-to-world of oracle/sqpnp.py on ALL masked points at the scene focal (what cv2_stub.solvePnPRansac returns for 4 or 5 points)"""
    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=F64), torch.arange(c.W, dtype=F64), indexing="ij")
    m = d["mask"].reshape(-1)
    xy = torch.stack([(xs.reshape(-1)[m] - c.ppxy[0]) / c.f, (ys.reshape(-1)[m] - c.ppxy[1]) / c.f], 1)
    R, t, _ = sqpnp.solve(d["pts"].double().reshape(-1, 3)[m].numpy(), xy.numpy())
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ t
    return torch.from_numpy(T)


def cv2_route(c, d):
    """the reference's route for a given focal: cv2.solvePnPRansac(SQPNP) of oracle/cv2_stub.py -> cam-to-world, or None"""
    from oracle import cv2_stub as cv2
    ys, xs = torch.meshgrid(torch.arange(c.H, dtype=F64), torch.arange(c.W, dtype=F64), indexing="ij")
    m = d["mask"].reshape(-1)
    uv = torch.stack([xs.reshape(-1)[m], ys.reshape(-1)[m]], 1).numpy()
    K = np.array([[c.f, 0, c.ppxy[0]], [0, c.f, c.ppxy[1]], [0, 0, 1]])
    ok, rvec, tvec, inl = cv2.solvePnPRansac(d["pts"].double().reshape(-1, 3)[m].numpy(), uv, K, None, iterationsCount=10, reprojectionError=5, flags=cv2.SOLVEPNP_SQPNP)
    if not ok:
        return None
    R = cv2.Rodrigues(rvec)[0]
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R.T, -R.T @ tvec[:, 0]
    return torch.from_numpy(T)


# ================================================================================================ guarded placement and the launches
class Bufs:
    """the device buffers of one launch"""

    def __init__(self, dev):
        self.dev, self.keep, self.outs = dev, [], []

    def op(self, t, margin=4096):
        """an operand inside 0xFF bytes: NaN for fp32, true for a mask byte"""
        if t is None:
            return None
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        view, buf = guarded_operand(t.contiguous(), self.dev, margin)
        self.keep.append(buf)
        return view

    def out(self, n, dtype=F32, want=True):
        """n 32-bit outputs between sentinel words, 16-byte aligned"""
        if not want:
            return None
        g = strided_out(1, n, n, dtype, self.dev)
        self.outs.append(g)
        return g

    def intact(self, what):
        torch.cuda.synchronize()
        for g in self.outs:
            assert guards_intact(g), f"{what}: a store outside an output of {g.width} words"


def _p(x):
    if x is None:
        return None
    return (x.view if isinstance(x, Guarded) else x).data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_align(lib, dev, d, q, want_thr=True, what="align"):
    """f3r_align_local_to_global on guarded buffers -> out [P][n][3], rts [P][13], thr [P] | None (CPU)"""
    from fast3r_amd import _lib
    P, n = d["conf"].shape
    b = Bufs(dev)
    conf, loc, glob, valid = b.op(d["conf"]), b.op(d["loc"]), b.op(d["glob"]), b.op(d["valid"])
    out, rts, thr = b.out(P * n * 3), b.out(P * 13), b.out(P, want=want_thr)
    ws_bytes = lib.f3r_align_workspace_bytes(P)
    assert ws_bytes == P * 40 * 8
    ws = b.out(ws_bytes // 4)
    _lib.check(lib.f3r_align_local_to_global(_p(conf), _p(loc), _p(glob), _p(valid), _p(out), _p(rts), _p(thr), _p(ws), ws_bytes, P, n, f32(q), _stream()),
               "f3r_align_local_to_global")
    b.intact(what)
    return out.view.cpu().view(P, n, 3), rts.view.cpu().view(P, 13), None if thr is None else thr.view.cpu().view(P)


def run_focal(lib, dev, pts, conf, q, pp, n_iter, rng, want_thr=True, what="focal"):
    """f3r_estimate_focal on guarded buffers; pts [V][H][W][3], conf [V][H][W] -> focal [V], thr [V] | None (CPU)"""
    from fast3r_amd import _lib
    V, H, W = conf.shape
    b = Bufs(dev)
    p, c = b.op(pts), b.op(conf)
    focal, thr = b.out(V), b.out(V, want=want_thr)
    ws_bytes = lib.f3r_focal_workspace_bytes(V, H, W)
    assert ws_bytes == V * H * W * 16
    ws = b.out(ws_bytes // 4)
    _lib.check(lib.f3r_estimate_focal(_p(p), _p(c), _p(focal), _p(thr), _p(ws), ws_bytes, V, H, W, f32(q), float(pp[0]), float(pp[1]), int(n_iter), float(rng[0]),
                                      float(rng[1]), _stream()), "f3r_estimate_focal")
    b.intact(what)
    return focal.view.cpu().view(V), None if thr is None else thr.view.cpu().view(V)


def run_pnp(lib, dev, pts, conf, focal_in, pp, conf_thr, n_focals, n_iter, what="pnp"):
    """f3r_estimate_poses on guarded buffers; pts [V][H][W][3], conf [V][H][W], focal_in [V] | None -> cam_to_world [V][4][4], focal [V], inliers [V] (CPU)"""
    from fast3r_amd import _lib
    V, H, W = conf.shape
    b = Bufs(dev)
    p, c, fin = b.op(pts), b.op(conf), b.op(focal_in)
    pose, fout, inl = b.out(V * 16), b.out(V), b.out(V, torch.int32)
    _lib.check(lib.f3r_estimate_poses(_p(p), _p(c), _p(fin), _p(fout), _p(pose), _p(inl), V, H, W, float(conf_thr), float(pp[0]), float(pp[1]), int(n_focals),
                                      int(n_iter), _stream()), "f3r_estimate_poses")
    b.intact(what)
    return pose.view.cpu().view(V, 4, 4), fout.view.cpu().view(V), inl.view.cpu().view(V)
