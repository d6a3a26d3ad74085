"""Seeded cases of the HBM-bound kernels (csrc/f3r_elem.hip) and of the fp32 kernels of precision "exact" (csrc/f3r_exact.hip) at the edges of
their geometry, their float64 references, float32 restatements of the kernels' arithmetic and the guarded placement of their device tensors
-- shared by tests/test_elem_cases.py (no GPU: the references against independent statements, the case lists against the structural
properties they are there for, and wrong restatements that must miss) and tests/test_elem_geometry_gpu.py (the kernels against the references).

One dataclass per kernel family; every case has an `id`.  A builder returns CPU tensors only: the operands exactly as the launch takes them
(already rounded to the case's dtype where the kernel reads 16-bit planes) and `ref`, float64 of the same operation on those operands.
"""
import dataclasses
import math

import torch
import torch.nn.functional as F

from conv_cases import BF16, H16, guarded_operand                       # noqa: F401  (the guard helpers: used by tests/test_elem_geometry_gpu.py)
from gemm_cases import guarded_rows, guards_intact, strided_out       # noqa: F401  (strided_out / guards_intact cover fp32 and 16-bit outputs alike)
from fast3r_amd import ops

F32 = torch.float32
DTYPES = (H16, BF16)
XQ, XK = 256, 32     # queries of a workgroup / keys of an LDS tile of attn_f32_kernel
LN_WAVE = 256        # floats one pass of a wave covers in layernorm_kernel (64 lanes x float4): MAXV = 4 | 8 | 32 from ceil(D / 256)


def _dt(dt):
    return "f16" if dt == H16 else "bf16"


def _gen(*key):
    s = 12345
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def rel_err(got, ref):
    """max |got - ref| over the output scale: the figure every check of the project asserts"""
    ref = ref.double()
    return float((got.double() - ref).abs().max()) / float(ref.abs().max().clamp_min(1e-6))


# ================================================================================================ LayerNorm / RMSNorm
@dataclasses.dataclass(frozen=True)
class LnCase:
    D: int
    rows: int
    outs: str = "both"        # "lp" | "f32" | "both"
    rms: bool = False
    dtype: torch.dtype = H16
    data: str = "randn"       # "randn": randn * 3 + 0.5 | "mean100": mean 100, std 1 | "equal": x == 0.5

    @property
    def eps(self):
        return 1e-5 if self.rms else 1e-6

    @property
    def id(self):
        return f"D{self.D}-r{self.rows}-{self.outs}-{'rms' if self.rms else 'ln'}-{_dt(self.dtype)}-{self.data}"


LN_D = (4, 8, 252, 260, 1024, 1028, 2048, 2052, 8188, 8192)


def _ln_cases():
    out = []
    for D in LN_D:
        for rows in ((1, 3, 4, 5) if D < 2052 else (3,)):
            for outs in ("lp", "f32", "both"):
                for rms in (False, True):
                    for dt in DTYPES:
                        out.append(LnCase(D, rows, outs, rms, dt))
    for D in (260, 2052):
        for rms in (False, True):
            for dt in DTYPES:
                out.append(LnCase(D, 3, "both", rms, dt, "mean100"))
    for dt in DTYPES:
        out.append(LnCase(256, 3, "both", False, dt, "equal"))
    return out


LN = _ln_cases()


def ln_maxv(D):
    """the instantiation f3r_layernorm picks: float4 per lane"""
    nv = (D // 4 + 63) // 64
    return 4 if nv <= 4 else (8 if nv <= 8 else 32)


def ln_math(x, g, b, eps, rms, one_pass=False):
    """the operation in x's own precision; one_pass: the variance as E[x^2] - mean^2 (what the kernel must NOT do)"""
    if rms:
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * g
    mu = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mu * mu if one_pass else (x - mu).pow(2).mean(-1, keepdim=True)
    y = (x - mu) * torch.rsqrt(var + eps) * g
    return y if b is None else y + b


def build_ln(c):
    g = _gen(1, c.D, c.rows, c.rms, {"randn": 0, "mean100": 1, "equal": 2}[c.data])
    if c.data == "randn":
        x = torch.randn((c.rows, c.D), generator=g) * 3 + 0.5
    elif c.data == "mean100":
        x = torch.randn((c.rows, c.D), generator=g) + 100.0
    else:
        x = torch.full((c.rows, c.D), 0.5)
    gamma = torch.randn(c.D, generator=g)
    beta = None if c.rms else torch.randn(c.D, generator=g)
    ref = ln_math(x.double(), gamma.double(), None if beta is None else beta.double(), c.eps, c.rms)
    return dict(x=x, gamma=gamma, beta=beta, ref=ref)


# ------------------------------------------------------------------------------------------------ LayerNorm -> rows [D fp16 | D fp8]
@dataclasses.dataclass(frozen=True)
class LnF8Case:
    D: int
    rows: int
    pad: int            # ld_out = 3 D / 2 + pad (fp16 elements)
    rms: bool = False
    seed: int = 0

    @property
    def ld(self):
        return 3 * self.D // 2 + self.pad

    @property
    def eps(self):
        return 1e-5 if self.rms else 1e-6

    @property
    def id(self):
        return f"D{self.D}-r{self.rows}-ld{self.ld}-{'rms' if self.rms else 'ln'}"


# The entry point wants ld_out % 8 == 0 (16-byte rows for the GEMM that reads them), so 3 D / 2 must be a multiple of 8 and D one of 16: the
# widths 8, 1032 and 2056 (the first multiples of 8 behind 0 and behind the two register switches) are refused at either stride, and the
# first multiples of 16 there -- 16, 1040 (MAXV 8), 2064 (MAXV 32) -- are the ones that run.
LN_F8_D_REFUSED, LN_F8_D = (8, 1032, 2056), (16, 1040, 2064)
# seeds: the first per (D, rms) for which no output lies within F8_TIE_MARGIN of an e4m3 rounding boundary (test_elem_cases.py holds them to it)
LN_F8_SEEDS = {(16, False): 0, (16, True): 0, (1040, False): 0, (1040, True): 0, (2064, False): 1, (2064, True): 0}
LN_F8 = [LnF8Case(D, 5, pad, rms, LN_F8_SEEDS[(D, rms)]) for D in LN_F8_D for pad in (0, 8) for rms in (False, True)]
LN_F8_REFUSED = [LnF8Case(D, 5, pad) for D in LN_F8_D_REFUSED for pad in (0, 8)]
F8_TIE_MARGIN = 2.0 ** -18   # relative: 32 fp32 ulps, far beyond what two fp32 evaluations of the same row differ by


def build_ln_f8(c):
    g = _gen(2, c.D, c.rms, c.seed)
    x = torch.randn((c.rows, c.D), generator=g) * 3.0
    gamma = 1 + 0.1 * torch.randn(c.D, generator=g)
    beta = None if c.rms else 0.1 * torch.randn(c.D, generator=g)
    if c.D > 40:
        gamma[40] = 2000.0   # a channel whose output leaves the fp8 range: the clamp comes before the conversion
    ref = ln_math(x.double(), gamma.double(), None if beta is None else beta.double(), c.eps, c.rms)
    return dict(x=x, gamma=gamma, beta=beta, ref=ref)


def e4m3(y):
    """clamp(+-448) -> e4m3 codes (uint8), as the kernels convert"""
    return y.float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def f8_ties(y64, margin=F8_TIE_MARGIN):
    """how many values change their e4m3 code when moved by the relative margin either way"""
    lo, hi = e4m3(y64 * (1 - margin)), e4m3(y64 * (1 + margin))
    return int((lo != hi).sum())


# ================================================================================================ bilinear
@dataclasses.dataclass(frozen=True)
class BilCase:
    B: int
    h: int
    w: int
    C: int
    full: tuple              # the interpolation's own output size
    out: tuple               # the (cropped) extent written
    dtype: torch.dtype = H16
    form: str = "plain"      # "plain" | "planes" (hi + lo in, hi + lo out) | "f8" (planes and the fp8 planes)

    @property
    def x2(self):
        """takes the f3r_upsample2x entry point"""
        return self.full == (2 * self.h, 2 * self.w) and self.form != "f8"

    @property
    def id(self):
        return f"{self.B}x{self.h}x{self.w}x{self.C}-to{self.full[0]}x{self.full[1]}-crop{self.out[0]}x{self.out[1]}-{self.form}-{_dt(self.dtype)}"


def _bil_cases():
    shapes = [((1, 1, 7, 8), (2, 14), (2, 14)), ((1, 5, 1, 8), (10, 2), (10, 2)), ((2, 3, 3, 24), (1, 1), (1, 1)), ((1, 9, 6, 8), (4, 3), (4, 3)),
              ((1, 3, 2, 16), (5, 4), (5, 4)), ((3, 4, 5, 64), (8, 10), (7, 10)), ((3, 4, 5, 64), (8, 10), (8, 9)), ((3, 4, 5, 64), (8, 10), (1, 1)),
              ((1, 2, 2, 8), (4, 4), (4, 4))]
    out = [BilCase(*s, full, crop, dt) for s, full, crop in shapes for dt in DTYPES]
    out += [BilCase(2, 4, 5, 64, (8, 10), (8, 10), dt, "planes") for dt in DTYPES]
    out += [BilCase(1, 1, 1, 128, (2, 2), (2, 2), H16, "f8"), BilCase(1, 3, 2, 128, (6, 4), (5, 3), H16, "f8")]
    return out


BIL = _bil_cases()


def bil_ref(x64, full, out):
    """F.interpolate(size=full, bilinear, align_corners=True) on the float64 NHWC input, cropped"""
    y = F.interpolate(x64.permute(0, 3, 1, 2), size=tuple(full), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    return y[:, :out[0], :out[1]].contiguous()


def bil_restate(x, full, out, dtype=F32, edge_clamp=True):
    """upsample2x_kernel's arithmetic in `dtype` on the plane as it lies in memory: pixels [B * h * w][C] followed by w + 2 pixels of NaN (the
    guard of the device buffer).  edge_clamp=False: x1 = x0 + 1, y1 = y0 + 1 without the `< w - 1` / `< h - 1` test (what the kernel must NOT do)."""
    B, h, w, C = x.shape
    (fh, fw), (oh, ow) = full, out
    flat = torch.cat([x.reshape(-1, C).to(dtype), torch.full((w + 2, C), float("nan"), dtype=dtype)])
    one = torch.ones((), dtype=dtype)
    sy = (one * (h - 1)) / (fh - 1) if fh > 1 else one * 0
    sx = (one * (w - 1)) / (fw - 1) if fw > 1 else one * 0
    fy, fx = sy * torch.arange(oh, dtype=dtype), sx * torch.arange(ow, dtype=dtype)
    y0, x0 = fy.long().clamp(max=h - 1), fx.long().clamp(max=w - 1)
    y1 = y0 + ((y0 < h - 1).long() if edge_clamp else 1)
    x1 = x0 + ((x0 < w - 1).long() if edge_clamp else 1)
    ly, lx = (fy - y0.to(dtype))[None, :, None, None], (fx - x0.to(dtype))[None, None, :, None]
    hy, hx = 1 - ly, 1 - lx
    b = torch.arange(B)[:, None, None]

    def px(yy, xx):
        return flat[(b * h + yy[None, :, None]) * w + xx[None, None, :]]
    return hy * (hx * px(y0, x0) + lx * px(y0, x1)) + ly * (hx * px(y1, x0) + lx * px(y1, x1))


def build_bil(c):
    g = _gen(3, c.B, c.h, c.w, c.C, c.out[0], c.out[1])
    x32 = torch.randn((c.B, c.h, c.w, c.C), generator=g) * (3.0 if c.form == "f8" else 1.0)
    if c.form == "plain":
        x, x_lo = x32.to(c.dtype), None
        xin = x.double()
    else:
        x, x_lo = ops.split_planes(x32, c.dtype)
        xin = x.double() + x_lo.double()
    return dict(x=x, x_lo=x_lo, xin=xin, ref=bil_ref(xin, c.full, c.out))


# ================================================================================================ head tail
@dataclasses.dataclass(frozen=True)
class DptCase:
    Cin: int
    npix: int
    lo: bool = False
    dtype: torch.dtype = H16
    n_out: int = 4
    depth: str = "exp"
    conf: tuple = ("exp", 1.0, math.inf)      # ignored with n_out == 3
    special: str = ""                         # "zero": pixel 0 has x = 0 and the bias is 0 | "saturate": the logit reaches +-60

    @property
    def id(self):
        cm = "noconf" if self.n_out == 3 else f"{self.conf[0]}{self.conf[1]:g}-{self.conf[2]:g}"
        return f"c{self.Cin}-p{self.npix}-{'pair' if self.lo else 'one'}-{_dt(self.dtype)}-{self.depth}-{cm}" + (f"-{self.special}" if self.special else "")


DPT128_NPIX = (1, 63, 64, 65, 129)


def _dpt_cases():
    out = []
    for dt in DTYPES:
        out += [DptCase(128, n, lo, dt) for lo in (False, True) for n in DPT128_NPIX]
        out += [DptCase(cin, n, False, dt) for cin in (8, 24) for n in (1, 255, 257)]
        out += [DptCase(24, 257, True, dt), DptCase(2048, 257, False, dt)]
        out += [DptCase(128, 65, False, dt, n_out=3), DptCase(24, 257, False, dt, n_out=3)]
        out += [DptCase(128, 65, True, dt, depth=m, special="zero") for m in ("exp", "linear", "square")]
        out += [DptCase(8, 257, False, dt, depth=m, special="zero") for m in ("exp", "linear", "square")]
        out += [DptCase(cin, 129, False, dt, conf=("sigmoid", 0.5, 3.0), special="saturate") for cin in (128, 8)]
    return out


DPT = _dpt_cases()
SATURATED = 30.0    # |logit| from which fp32 1 / (1 + exp(-z)) is exactly 1 or (times 2.5, plus 0.5) exactly vmin: exp(-30) = 9e-14 < 2^-25


def dpt_math(xin, w, b, depth, conf):
    """x (npix, Cin) @ w^T + b -> reg_dense_depth / reg_dense_conf (heads/postprocess.py:27-64) in xin's precision -> (pts, conf | None)"""
    z = xin @ w.t() + b
    xyz = z[:, :3]
    if depth == "linear":
        pts = xyz
    else:
        d = xyz.norm(dim=-1, keepdim=True)
        pts = xyz / d.clamp_min(1e-8) * (torch.expm1(d) if depth == "exp" else d * d)
    if w.shape[0] == 3:
        return pts, None
    mode, vmin, vmax = conf
    cf = vmin + z[:, 3].exp().clamp(max=vmax - vmin) if mode == "exp" else (vmax - vmin) * torch.sigmoid(z[:, 3]) + vmin
    return pts, cf


def build_dpt(c):
    g = _gen(4, c.Cin, c.npix, c.lo, c.n_out)
    x32 = torch.randn((c.npix, c.Cin), generator=g)
    w = torch.randn((c.n_out, c.Cin), generator=g) * c.Cin ** -0.5     # unit-variance outputs at every width
    b = torch.randn(c.n_out, generator=g) * 0.1
    if c.special == "zero":
        x32[0] = 0.0
        b = torch.zeros(c.n_out)
    x, x_lo = ops.split_planes(x32, c.dtype) if c.lo else (x32.to(c.dtype), None)
    xin = x.double() + (x_lo.double() if c.lo else 0.0)
    if c.special == "saturate":
        b[3] = 0.0
        z3 = xin @ w[3].double()
        w[3] *= 60.0 / float(z3.abs().max())
        z3 = xin @ w[3].double()
        assert float(z3.max()) >= SATURATED and float(z3.min()) <= -SATURATED, "the case must saturate on both sides"
    pts, cf = dpt_math(xin, w.double(), b.double(), c.depth, c.conf)
    return dict(x=x, x_lo=x_lo, xin=xin, w=w, b=b, pts=pts, conf=cf)


def dpt128_staged_rows(npix, group, clamp_to_last=True):
    """the pixel rows dpt_final128_kernel stages for 64-pixel group `group`: rows past the end are clamped to npix - 1 (clamp_to_last=False: to
    npix, the row behind the plane -- what the kernel must NOT read)"""
    rows = torch.arange(group * 64, group * 64 + 64)
    return rows.clamp(max=npix - 1 if clamp_to_last else npix)


# ================================================================================================ cast, patchify, SwiGLU gate, row add
@dataclasses.dataclass(frozen=True)
class CastCase:
    n: int
    lo: bool
    dtype: torch.dtype

    @property
    def id(self):
        return f"n{self.n}-{'pair' if self.lo else 'one'}-{_dt(self.dtype)}"


CAST = [CastCase(n, lo, dt) for n in (8, 8 * 257) for lo in (False, True) for dt in DTYPES]


def build_cast(c):
    x = torch.randn(c.n, generator=_gen(5, c.n)) * 3
    hi = x.to(c.dtype)
    return dict(x=x, hi=hi, lo=(x - hi.float()).to(c.dtype))


@dataclasses.dataclass(frozen=True)
class PatchCase:
    B: int
    H: int
    W: int
    ps: int
    ld: int = 0                  # 0: the entry point's default, K
    dtype: torch.dtype = H16

    @property
    def K(self):
        return 3 * self.ps * self.ps

    @property
    def ld_eff(self):
        return self.ld or self.K

    @property
    def vector_path(self):
        """f3r_patchify's switch: patchify_kernel (16 bytes per lane) or patchify_any_kernel"""
        return self.ps % 8 == 0 and self.ld_eff == self.K

    @property
    def patches(self):
        return self.B * (self.H // self.ps) * (self.W // self.ps)

    @property
    def id(self):
        return f"{self.B}x{self.H}x{self.W}-ps{self.ps}-ld{self.ld}-{_dt(self.dtype)}"


PATCH = [PatchCase(*a, dt) for dt in DTYPES for a in
         [(1, 16, 16, 16, 0), (2, 16, 48, 16, 768), (2, 16, 24, 8, 0), (1, 24, 48, 24, 0), (2, 8, 12, 4, 48), (2, 14, 28, 14, 592), (2, 14, 28, 14, 640),
          (1, 16, 32, 16, 776)]]


def patch_ref(img, ps):
    """F.unfold rows in (c, dy, dx) order = the patch-embed Conv2d's weight order"""
    return F.unfold(img, kernel_size=ps, stride=ps).transpose(1, 2).reshape(-1, 3 * ps * ps)


def patch_explicit(img, ps):
    B, _, H, W = img.shape
    return img.reshape(B, 3, H // ps, ps, W // ps, ps).permute(0, 2, 4, 1, 3, 5).reshape(-1, 3 * ps * ps)


def build_patch(c):
    img = torch.rand((c.B, 3, c.H, c.W), generator=_gen(6, c.B, c.H, c.W, c.ps)) * 2 - 1
    return dict(img=img, ref=patch_ref(img, c.ps).to(c.dtype))


@dataclasses.dataclass(frozen=True)
class SiluCase:
    rows: int
    hidden: int
    dtype: torch.dtype

    @property
    def id(self):
        return f"r{self.rows}-h{self.hidden}-{_dt(self.dtype)}"


SILU = [SiluCase(r, h, dt) for r, h in ((1, 8), (3, 200), (257, 8)) for dt in DTYPES]
SILU_F32 = [SiluCase(r, h, dt) for r, h in ((1, 4), (3, 100), (257, 4)) for dt in DTYPES]


def build_silu(c, f32=False):
    """ab [rows][2 hidden] = a | b; a holds +30 and -30 (exp(30) = 1e13 in the gate), their b is 1/16 so they do not set the output scale"""
    g = _gen(7, c.rows, c.hidden, f32)
    ab = torch.randn((c.rows, 2 * c.hidden), generator=g) * 2.0
    ab[0, 0], ab[0, 1], ab[-1, c.hidden - 1] = 30.0, -30.0, -30.0
    ab[0, c.hidden], ab[0, c.hidden + 1], ab[-1, 2 * c.hidden - 1] = 0.0625, 0.0625, 0.0625
    if not f32:
        ab = ab.to(c.dtype)
    ref = F.silu(ab[:, :c.hidden].double()) * ab[:, c.hidden:].double()
    return dict(ab=ab, ref=ref)


@dataclasses.dataclass(frozen=True)
class RowsAddCase:
    D: int
    total: int
    rows: int

    @property
    def id(self):
        return f"D{self.D}-{self.rows}of{self.total}"


ROWS_ADD = [RowsAddCase(D, 5, r) for D in (4, 260) for r in (0, 1, 5)]


def build_rows_add(c):
    g = _gen(8, c.D, c.rows)
    x, vec = torch.randn((c.total, c.D), generator=g), torch.randn(c.D, generator=g)
    ref = x.clone()
    ref[:c.rows] += vec
    return dict(x=x, vec=vec, ref=ref)


# ================================================================================================ fp32 attention
@dataclasses.dataclass(frozen=True)
class AttnCase:
    HD: int
    tq: int
    tk: int
    H: int = 2
    kv_group: int = 1
    n_seq: int = 1
    causal: bool = False
    q_pos0: int = 0
    k_pos0: int = 0
    pad: int = 0               # ldq, ldkv, ldo = their width + pad
    outs: str = "all"          # "f32" | "hi" (no low plane, no fp32) | "all"
    dtype: torch.dtype = H16
    entry: str = "ex"          # "ex": f3r_attn_f32_ex | "plain": f3r_attn_f32 (q | k | v column blocks of one buffer, tq == tk)

    @property
    def Hkv(self):
        return self.H // self.kv_group

    @property
    def scale(self):
        return self.HD ** -0.5

    @property
    def id(self):
        ca = f"-causal{self.q_pos0}.{self.k_pos0}" if self.causal else ""
        return (f"hd{self.HD}-q{self.tq}-k{self.tk}-h{self.H}g{self.kv_group}-s{self.n_seq}{ca}-pad{self.pad}-{self.outs}-{_dt(self.dtype)}"
                + ("-plain" if self.entry == "plain" else ""))


ATTN_HD = (16, 32, 48, 64, 80, 96, 112, 128)
ATTN_TQ_EDGE, ATTN_TK_EDGE = (1, 255, 256, 257), (1, 31, 32, 33)
ATTN_CAUSAL = ((0, 3, 8, 8), (0, 300, 257, 64), (100, 90, 64, 200))    # (q_pos0, k_pos0, tq, tk)


def _attn_cases():
    out = []
    for dt in DTYPES:
        out += [AttnCase(hd, 33, 65, kv_group=2, n_seq=2, dtype=dt) for hd in ATTN_HD]
        for hd in (64, 128):
            out += [AttnCase(hd, tq, 40, dtype=dt) for tq in ATTN_TQ_EDGE]
            out += [AttnCase(hd, 5, tk, dtype=dt) for tk in ATTN_TK_EDGE]
        out.append(AttnCase(64, 257, 40, n_seq=3, dtype=dt))
        out += [AttnCase(hd, 33, 65, kv_group=2, n_seq=2, pad=8, outs=o, dtype=dt) for hd in (64, 80) for o in ("f32", "hi", "all")]
        out += [AttnCase(64, 33, 65, outs=o, dtype=dt) for o in ("f32", "hi")]
        out += [AttnCase(64, tq, tk, kv_group=2, n_seq=2, causal=True, q_pos0=qp, k_pos0=kp, outs=o, dtype=dt)
                for qp, kp, tq, tk in ATTN_CAUSAL for o in ("f32", "hi", "all")]
        out.append(AttnCase(128, 8, 8, causal=True, q_pos0=0, k_pos0=3, pad=8, dtype=dt))
        out.append(AttnCase(64, 33, 33, n_seq=2, dtype=dt, entry="plain"))
    return out


ATTN = _attn_cases()


def attn_visible(c):
    """[tq][tk] bool: key j is visible to query i"""
    if not c.causal:
        return torch.ones((c.tq, c.tk), dtype=torch.bool)
    return (c.k_pos0 + torch.arange(c.tk))[None, :] <= (c.q_pos0 + torch.arange(c.tq))[:, None]


def _heads(c, q, k, v):
    qh = q.reshape(c.n_seq, c.tq, c.H, c.HD).permute(0, 2, 1, 3)
    kh = k.reshape(c.n_seq, c.tk, c.Hkv, c.HD).permute(0, 2, 1, 3).repeat_interleave(c.kv_group, dim=1)
    vh = v.reshape(c.n_seq, c.tk, c.Hkv, c.HD).permute(0, 2, 1, 3).repeat_interleave(c.kv_group, dim=1)
    return qh, kh, vh


def attn_ref(c, q, k, v):
    """softmax(q k^T scale [masked]) v in the inputs' precision -> [n_seq * tq][H * HD]; a row that sees no key is zeros (the kernel's contract,
    f3r_exact.hip: `inv = l > 0 ? 1 / l : 0`), where softmax itself would give NaN"""
    qh, kh, vh = _heads(c, q, k, v)
    vis = attn_visible(c)
    s = (qh @ kh.transpose(-1, -2) * c.scale).masked_fill(~vis, float("-inf"))
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isinf(m), torch.zeros_like(m), m))
    l = p.sum(-1, keepdim=True)
    o = torch.where(l > 0, (p @ vh) / l.clamp_min(1e-300), torch.zeros_like(l))
    return o.permute(0, 2, 1, 3).reshape(c.n_seq * c.tq, c.H * c.HD)


def attn_restate_f32(c, q, k, v, use_k_pos0=True):
    """attn_f32_kernel's algorithm in float32: 32-key tiles, running maximum and online rescale, 1 / l at the end (not its fmaf order).
    use_k_pos0=False: the causal mask as if the keys started at position 0 (what the kernel must NOT do)."""
    qh, kh, vh = _heads(c, q.float(), k.float(), v.float())
    qh = qh * torch.tensor(c.scale, dtype=F32)
    vis = attn_visible(c if use_k_pos0 else dataclasses.replace(c, k_pos0=0))
    m = torch.full(qh.shape[:-1] + (1,), float("-inf"))
    l = torch.zeros_like(m)
    o = torch.zeros_like(qh)
    for k0 in range(0, c.tk, XK):
        s = (qh @ kh[:, :, k0:k0 + XK].transpose(-1, -2)).masked_fill(~vis[:, k0:k0 + XK], float("-inf"))
        m_new = torch.maximum(m, s.amax(-1, keepdim=True))
        safe = torch.where(torch.isinf(m_new), torch.zeros_like(m_new), m_new)     # rows that have seen no key yet: p = exp(-inf) = 0
        alpha = torch.exp(m - safe)
        p = torch.exp(s - safe)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + p @ vh[:, :, k0:k0 + XK]
        m = m_new
    inv = torch.where(l > 0, 1.0 / l.clamp_min(1e-37), torch.zeros_like(l))
    return (o * inv).permute(0, 2, 1, 3).reshape(c.n_seq * c.tq, c.H * c.HD)


def build_attn(c):
    g = _gen(9, c.HD, c.tq, c.tk, c.H, c.kv_group, c.n_seq)
    q = torch.randn((c.n_seq * c.tq, c.H * c.HD), generator=g)
    k = torch.randn((c.n_seq * c.tk, c.Hkv * c.HD), generator=g)
    v = torch.randn((c.n_seq * c.tk, c.Hkv * c.HD), generator=g)
    return dict(q=q, k=k, v=v, ref=attn_ref(c, q.double(), k.double(), v.double()), no_key=~attn_visible(c).any(-1))


def attn_tol(c, what):
    """the project's figures (test_exact_mode_rope_and_fp32_attention): 3e-6 for the fp32 output and the fp16 planes' sum, 3e-5 for the bf16 planes' sum;
    one lowp plane alone: its rounding"""
    if what == "f32":
        return 3e-6
    if what == "planes":
        return 3e-6 if c.dtype == H16 else 3e-5
    return 2.0 ** -9 if c.dtype == H16 else 2.0 ** -6


# ================================================================================================ fp32 rotary embedding
@dataclasses.dataclass(frozen=True)
class RopeCase:
    mode: int
    rows: int
    seq_len: int
    rope_w: int
    n_rot: int = 3             # rotated 64-wide column groups (2 q heads + 1 k head)
    tail: int = 128            # columns behind them (k's / v's part): must come out bit-unchanged
    pad: int = 0               # ld = n_rot * 64 + tail + pad

    @property
    def width(self):
        return self.n_rot * 64 + self.tail

    @property
    def id(self):
        return f"mode{self.mode}-r{self.rows}-s{self.seq_len}-w{self.rope_w}-rot{self.n_rot}-pad{self.pad}"


ROPE = [RopeCase(0, 1, 1, 1), RopeCase(0, 30, 15, 5, n_rot=4, tail=128, pad=8),    # 4 x 64 = 2 D, D = 128: ld = 3 D + 8
        RopeCase(1, 5, 5, 1), RopeCase(1, 12, 12, 5), RopeCase(1, 12, 12, 5, pad=8)]


def rope_math(c, x, cos, sin, pair=16):
    """rope_f32_kernel in x's precision, out of place: column head * 64 + half * 32 + i (i < 16) rotates with the column `pair` further on"""
    out = x.clone()
    row = torch.arange(c.rows)
    for half in (0, 1):
        if c.mode == 1:
            t = (row // c.rope_w) * 32 + half * 16
        else:
            pos = row % c.seq_len
            t = (pos // c.rope_w if half == 0 else pos % c.rope_w) * 16
        idx = t[:, None] + torch.arange(16)[None, :]
        cs, sn = cos.reshape(-1)[idx], sin.reshape(-1)[idx]
        for head in range(c.n_rot):
            c0 = head * 64 + half * 32
            a, b = x[:, c0:c0 + 16], x[:, c0 + pair:c0 + pair + 16]
            out[:, c0:c0 + 16] = a * cs - b * sn
            out[:, c0 + pair:c0 + pair + 16] = b * cs + a * sn
    return out


def rope_complex(c, x, cos, sin):
    """the same rotation as a complex product (a + i b)(cos + i sin), float64"""
    out = x.clone().double()
    for r in range(c.rows):
        for head in range(c.n_rot):
            for half in (0, 1):
                if c.mode == 1:
                    ang = torch.complex(cos.double(), sin.double()).reshape(-1, 32)[r // c.rope_w, half * 16:half * 16 + 16]
                else:
                    pos = r % c.seq_len
                    ang = torch.complex(cos.double(), sin.double()).reshape(-1, 16)[pos // c.rope_w if half == 0 else pos % c.rope_w]
                c0 = head * 64 + half * 32
                z = torch.complex(out[r, c0:c0 + 16], out[r, c0 + 16:c0 + 32]) * ang
                out[r, c0:c0 + 16], out[r, c0 + 16:c0 + 32] = z.real, z.imag
    return out


def build_rope(c):
    g = _gen(10, c.mode, c.rows, c.rope_w, c.n_rot)
    x = torch.randn((c.rows, c.width), generator=g)
    if c.mode == 0:
        n_pos = max(-(-c.seq_len // c.rope_w), c.rope_w)
        cos, sin = ops.rope_tables(n_pos, 100.0, "cpu")
    else:
        ang = torch.rand((-(-c.rows // c.rope_w), 32), generator=g) * 6.28
        cos, sin = ang.cos().contiguous(), ang.sin().contiguous()
    return dict(x=x, cos=cos, sin=sin, ref=rope_math(c, x.double(), cos.double(), sin.double()))
