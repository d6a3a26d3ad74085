"""Seeded cases of the plain-operand launches of f3r_gemm -- the generic epilogue, the QKV projection and ConvT -- at the edges of their geometry,
their float64 references and the guarded placement of their device tensors: shared by tests/test_gemm_cases.py (no GPU: the references against a
direct product on the materialised batch, the case lists against the properties they are there for, the eligibility restated here against the
library) and tests/test_gemm_geometry_gpu.py (the kernels against the references).

A case names its shape, role, split, dtype, row strides and a period P: row m of a periodic case carries the content of row m mod (P tiles), so the
reference is computed for one period and compared against all M rows.

What the reference is, by split (float64 throughout):
  None    the product of the operands rounded to the case's dtype
  "w2"    the rounded activation against the UNROUNDED fp32 weights (the kernel carries the weights as hi + lo planes)
  "x3"    the unrounded fp32 operands (the kernel drops only lo x lo)
  "w2f8"  the decoded planes: fp16 x fp16 hi + e4m3 copy of the activation x e4m3 low plane of the weights with its power-of-two scales
"""
import dataclasses

import torch
import torch.nn.functional as F

from conv_cases import BF16, CU_NOMINAL, H16, SENTINEL, guarded_operand, periodic  # noqa: F401  (re-exported: one owner)
from fast3r_amd import _lib, ops
from test_kernels_gpu import _rope_ref

BM = 256   # output rows of a tile of the 256-tile kernel (and of the hand-scheduled one)

# what a role of the generic epilogue passes: bias, activation, outputs, additive terms
ROLES = {
    "f32": dict(bias=True, act=None, f32=True, lp=False),                     # fp32 out + bias
    "gelu": dict(bias=True, act="gelu", f32=False, lp=True),                  # lowp out + GELU
    "relu2res": dict(bias=True, act="relu", f32=False, lp=True, res_lp=True),  # lowp out + ReLU + two lowp residuals
    "resf32": dict(bias=True, act=None, f32=True, lp=False, res_f32=True),    # fp32 residual, in place
    "rowadd": dict(bias=True, act=None, f32=True, lp=False, rowadd=True),     # image-id rows
    "both": dict(bias=True, act=None, f32=True, lp=True),                     # both outputs at once
    "nobias": dict(bias=False, act=None, f32=False, lp=True),                 # no bias at all
}


def _dt(dt):
    return "f16" if dt == H16 else "bf16"


@dataclasses.dataclass(frozen=True)
class GemmCase:
    M: int
    N: int
    K: int
    role: str = "f32"
    split: object = None          # None | "w2" | "x3" | "w2f8"
    dtype: torch.dtype = H16
    div: int = 0                  # rowadd_div of the "rowadd" role
    lda: int = 0                  # row strides in elements; 0: the row's width
    ldo_f32: int = 0
    ldo_lp: int = 0
    ldr_f32: int = 0
    ldr_lp: int = 0
    ldr_lp2: int = 0
    P: int = 0                    # period of the rows' content in 256-row tiles (0: every row its own)
    f8_rows: bool = False         # "w2f8": out_lp rows are [N fp16 | N fp8]

    kind = "gemm"

    @property
    def period(self):
        return self.P or -(-self.M // BM)

    @property
    def rows(self):
        """rows of one period"""
        return self.P * BM if self.P else self.M

    @property
    def spec(self):
        return ROLES[self.role]

    @property
    def a_width(self):
        """elements of an operand row that the kernel reads"""
        return 3 * self.K // 2 if self.split == "w2f8" else self.K

    @property
    def lp_width(self):
        return 3 * self.N // 2 if self.f8_rows else self.N

    def ld(self, name):
        width = {"lda": self.a_width, "ldo_lp": self.lp_width}.get(name, self.N)
        return getattr(self, name) or width

    @property
    def want_lo(self):
        return self.split == "x3" and self.spec["lp"]

    @property
    def id(self):
        lds = "".join(f"-{n}{getattr(self, n)}" for n in ("lda", "ldo_f32", "ldo_lp", "ldr_f32", "ldr_lp", "ldr_lp2") if getattr(self, n))
        return (f"{self.M}x{self.N}x{self.K}{f'p{self.P}' if self.P else ''}-{self.role}{self.div or ''}-{self.split or 'one'}-{_dt(self.dtype)}"
                f"{lds}{'-f8rows' if self.f8_rows else ''}")


@dataclasses.dataclass(frozen=True)
class QkvCase:
    n_seq: int
    S: int
    Dq: int
    Dkv: int
    K: int
    dtype: torch.dtype = H16
    grid: object = None           # (gh, gw) with gh * gw == S: RoPE-2D, or None
    q_scale: float = 0.0
    ldvt: int = 0                 # 0: ops.vt_ld(S)
    P: int = 0                    # period of the sequences' content, in sequences

    kind = "qkv"

    @property
    def M(self):
        return self.n_seq * self.S

    @property
    def N(self):
        return self.Dq + 2 * self.Dkv

    @property
    def period(self):
        return self.P or self.n_seq

    @property
    def vt_stride(self):
        return self.ldvt or ops.vt_ld(self.S)

    @property
    def id(self):
        g = f"-rope{self.grid[0]}x{self.grid[1]}" if self.grid else ""
        return (f"qkv-{self.n_seq}x{self.S}{f'p{self.P}' if self.P else ''}-q{self.Dq}-kv{self.Dkv}-k{self.K}-{_dt(self.dtype)}{g}"
                f"{'-qs' if self.q_scale else ''}{f'-ldvt{self.ldvt}' if self.ldvt else ''}")


@dataclasses.dataclass(frozen=True)
class ConvTCase:
    B: int
    h: int
    w: int
    Ci: int
    Co: int
    s: int
    split: object = None          # None | "x3"
    dtype: torch.dtype = H16

    kind = "convt"

    @property
    def M(self):
        return self.B * self.h * self.w

    @property
    def N(self):
        return self.s * self.s * self.Co

    @property
    def K(self):
        return self.Ci

    @property
    def id(self):
        return f"convt-{self.B}x{self.h}x{self.w}-c{self.Ci}-n{self.Co}-s{self.s}-{self.split or 'one'}-{_dt(self.dtype)}"


# ------------------------------------------------------------------------------------------------ which kernel forms take a case
def planes(c):
    return 1 if getattr(c, "split", None) is None else 2


def eligible256(c):
    """f3r_gemm256_eligible restated for these cases: whole 128-column tiles, no K tail (the LDS-DMA staging cannot zero-fill one), QKV parts of
    whole 256-wide tiles, and of the additive terms only the fp32 residual or the image-id rows, without an activation"""
    if c.N % 128 or c.K % 64:
        return False
    if c.kind == "qkv":
        return c.Dq % 256 == 0 and c.Dkv % 256 == 0
    if c.kind == "gemm":
        if c.split == "w2f8" or c.spec.get("res_lp"):
            return False
        assert not ((c.spec.get("res_f32") or c.spec.get("rowadd")) and c.spec["act"])   # (no role of these lists has both)
    return True


def eligible_asm(c):
    """f3r_gemm_asm_eligible / f3r_gemm_asm_qkv_eligible restated: whole 256 x 256 tiles, at least four K-tiles over all planes, one plane or w2, ONE
    output (fp32 + bias + fp32 residual, or lowp + bias + activation), 16-byte row strides; QKV: equal parts of whole tiles, sequences of whole
    tiles"""
    if c.kind == "convt" or c.M % 256 or c.K % 64:
        return False
    if c.kind == "qkv":
        return c.Dq == c.Dkv and c.Dq % 256 == 0 and c.S % 256 == 0 and c.K // 64 >= 4 and c.vt_stride % 8 == 0
    if c.N % 256 or c.split not in (None, "w2") or planes(c) * c.K // 64 < 4:
        return False
    if c.role not in ("f32", "gelu", "resf32", "nobias"):
        return False
    return c.ld("ldo_lp") % 8 == 0 if c.spec["lp"] else (c.ld("ldo_f32") % 4 == 0 and c.ld("ldr_f32") % 4 == 0)


def kernel_sels(c):
    """the kernel forms that take the case: 1 = 128-tile kernel; 2 / 3 = 256-tile kernel staggered / lock-step, 4 = its 256 x 128 tile form, 5 = one
    tile per workgroup (QKV has the wide tile only: no 4); 6 = the hand-scheduled kernel; 0 = by shape.  "w2f8" has one kernel family: 0 only."""
    if getattr(c, "split", None) == "w2f8":
        return [0]
    sels = [1]
    if eligible256(c):
        sels += [2, 3, 5] if c.kind == "qkv" else [2, 3, 4, 5]
    if eligible_asm(c):
        sels.append(6)
    return sels + [0]


def tile_width(c, sel):
    """columns of an output tile of the form (tile_halves in csrc/f3r_gemm256_impl.h: a 256-wide tile only where N fills it)"""
    if sel == 1:
        return 128
    if sel == 6 or c.kind == "qkv":
        return 256
    return 128 if (c.N % 256 or sel == 4) else 256


def tiles(c, sel):
    bm = 128 if sel == 1 else BM
    return -(-c.M // bm) * -(-c.N // tile_width(c, sel))


def legal(c):
    """f3r_gemm's argument rules (csrc/f3r_gemm.hip) restated: None, or the first rule the case breaks"""
    if c.M <= 0 or c.N <= 0 or c.N % 4:
        return "M / N"
    if c.K <= 0 or c.K % 8:
        return "K"
    if c.kind == "qkv":
        if c.Dq % 64 or c.Dkv % 64 or (2 * c.Dkv) % 128 or c.Dq <= 0 or c.Dkv <= 0:
            return "QKV parts must be whole heads"
        if c.S <= 0 or c.vt_stride < c.S or (c.grid and c.grid[0] * c.grid[1] != c.S):
            return "seq_len / ldvt / grid"
        return None
    if c.kind == "convt":
        return "ConvT cout" if c.Co % 4 or c.s <= 0 else None
    if c.split == "w2f8":
        if c.dtype != H16 or c.K % 128 or c.M % 256 or c.N % 256 or c.K // 64 + c.K // 128 < 4:
            return "w2f8 shape"
        if c.ld("lda") % 8 or c.ld("lda") * 2 < 3 * c.K or c.role not in ("f32", "gelu", "resf32"):
            return "w2f8 rows"
        if c.f8_rows and (c.role != "gelu" or c.ld("ldo_lp") * 2 < 3 * c.N):
            return "w2f8 output rows"
    elif c.f8_rows:
        return "f8 rows without w2f8"
    if c.ld("lda") % 8 or c.ld("lda") < c.a_width:
        return "lda"
    for name, width in (("ldo_f32", c.N), ("ldo_lp", c.lp_width)):
        if c.ld(name) % 4 or c.ld(name) < width:
            return name
    for name in ("ldr_f32", "ldr_lp", "ldr_lp2"):
        if c.ld(name) % 4 or c.ld(name) < c.N:     # (the library asks only % 4 of a residual's stride; a shorter row would alias the next)
            return name
    if c.spec.get("res_f32") and c.ld("ldr_f32") != c.ld("ldo_f32"):
        return "the fp32 residual is updated in place: one stride"
    if bool(c.spec.get("rowadd")) != bool(c.div):
        return "rowadd_div"
    if c.P and (c.M < c.rows or c.div):
        return "period"
    return None


def stand_in_args(c, sel=0, M=None):
    """the f3r_gemm_args the GPU test's launch of the case builds, with stand-in addresses (argument checks and eligibility read no memory)"""
    g = _lib.GemmArgs()
    at = 0x10000
    g.A = g.W = at
    split = getattr(c, "split", None)
    p = planes(c)
    g.M, g.N, g.K = c.M if M is None else M, c.N, c.K
    g.Kpad = c.K if split == "w2f8" else p * ops.round_up(c.K, 64)
    g.a_mode, g.dtype, g.split, g.kernel_sel = _lib.F3R_A_PLAIN, _lib.dtype_id(c.dtype), ops.SPLIT[split], sel
    if split == "x3":
        g.A_lo = at
    if c.kind == "qkv":
        g.epi, g.lda, g.bias = _lib.F3R_EPI_QKV, c.K, at
        g.q = g.k = g.vt = at
        g.seq_len, g.ldvt, g.q_scale = c.S, c.vt_stride, c.q_scale
        g.qkv_dq = 0 if c.Dq == c.Dkv else c.Dq
        if c.grid:
            g.rope_cos = g.rope_sin = at
            g.rope_w = c.grid[1]
    elif c.kind == "convt":
        g.epi, g.lda, g.bias, g.out_lp, g.ldo_lp = _lib.F3R_EPI_CONVT, c.Ci, at, at, c.Co
        g.ct_s, g.ct_h, g.ct_w, g.ct_cout = c.s, c.h, c.w, c.Co
        if split == "x3":
            g.out_lp_lo = at
    else:
        spec = c.spec
        g.epi, g.lda, g.act = _lib.F3R_EPI_GENERIC, c.ld("lda"), ops.ACT[spec["act"]]
        if spec["bias"]:
            g.bias = at
        if spec["f32"]:
            g.out_f32, g.ldo_f32 = at, c.ld("ldo_f32")
        if spec["lp"]:
            g.out_lp, g.ldo_lp = at, c.ld("ldo_lp")
            if c.want_lo:
                g.out_lp_lo = at
        if spec.get("res_f32"):
            g.res_f32, g.ldr_f32 = at, c.ld("ldr_f32")
        if spec.get("rowadd"):
            g.rowadd, g.rowadd_div = at, c.div
        if spec.get("res_lp"):
            g.res_lp, g.ldr_lp, g.res_lp2, g.ldr_lp2 = at, c.ld("ldr_lp"), at, c.ld("ldr_lp2")
            if split == "x3":
                g.res_lp_lo = g.res_lp2_lo = at
        if split == "w2f8":
            g.w_scale, g.out_lp_f8 = at, int(c.f8_rows)
    return g


# ------------------------------------------------------------------------------------------------ 1. the edges of the generic epilogue
EDGE_M = (1, 15, 16, 17, 63, 65, 127, 129, 255, 257, 321, 513)
EDGE_N128 = (4, 60, 68, 124, 132, 260)        # the 128-tile kernel alone
EDGE_N256 = (128, 256, 384, 640)              # where the 256-tile forms apply
EDGE_K = (8, 72, 64, 128, 192)                # 72: a K tail (Kpad 128); 8: one 16-byte chunk
EDGE_K256 = (64, 128, 192)                    # no K tail: what the 256-tile kernel stages by LDS-DMA
EDGE_ROLES = tuple(ROLES)
EDGE_SPLITS = (None, "w2", "x3")
ROWADD_DIVS = (1, 70, "M")


def _edges():
    """every M meets every role twice: with an N (and any K) of the 128-tile kernel, and with an N (and a K without tail) that the 256-tile forms
    take.  The other values rotate against (M, role) so that every N meets every role as well, both dtypes and the three splits meet every role,
    and the three rowadd_div values meet narrow and wide N."""
    out = []
    for i, M in enumerate(EDGE_M):
        for j, role in enumerate(EDGE_ROLES):
            for wide in (False, True):
                ns, ks = (EDGE_N256, EDGE_K256) if wide else (EDGE_N128, EDGE_K)
                N, K = ns[(i + j) % len(ns)], ks[(i + 2 * j + wide) % len(ks)]
                dt = (H16, BF16)[(i + j + wide) % 2]
                split = EDGE_SPLITS[(i + 2 * j + 2 * wide) % 3]
                div = 0
                if role == "rowadd":
                    div = ROWADD_DIVS[(i + wide) % 3]
                    div = M if div == "M" else div
                out.append(GemmCase(M, N, K, role, split, dt, div))
    return out


EDGES = _edges()


# ------------------------------------------------------------------------------------------------ 2. row strides
def _strides():
    out = []
    # interior (every wave sub-tile inside the matrix; K = 256: four K-tiles, what the hand-scheduled kernel needs) and ragged
    for M, N, K in ((512, 256, 128), (512, 256, 256), (300, 132, 128)):
        wide = (3 * N // 2 + 7) // 8 * 8
        for dt in (H16, BF16):
            out += [
                GemmCase(M, N, K, "f32", None, dt, lda=K + 8, ldo_f32=N + 4),
                GemmCase(M, N, K, "f32", "w2", dt, lda=K + 64, ldo_f32=N + 4),
                GemmCase(M, N, K, "gelu", None, dt, lda=K + 64, ldo_lp=N + 8),
                GemmCase(M, N, K, "gelu", None, dt, ldo_lp=wide),                 # hid aliased onto the [N fp16 | N fp8] rows of hid8
                GemmCase(M, N, K, "nobias", "w2", dt, lda=K + 8, ldo_lp=wide),
                GemmCase(M, N, K, "resf32", None, dt, lda=K + 8, ldo_f32=N + 4, ldr_f32=N + 4),
                GemmCase(M, N, K, "relu2res", None, dt, ldo_lp=N + 8, ldr_lp=N + 4, ldr_lp2=N + 12),
                GemmCase(M, N, K, "relu2res", "x3", dt, lda=K + 8, ldo_lp=N + 8, ldr_lp=N + 4, ldr_lp2=N + 12),
                GemmCase(M, N, K, "rowadd", None, dt, 70, lda=K + 64, ldo_f32=N + 4),
                GemmCase(M, N, K, "both", None, dt, lda=K + 8, ldo_f32=N + 4, ldo_lp=N + 8),
                GemmCase(M, N, K, "both", "x3", dt, lda=K + 64, ldo_f32=N + 4, ldo_lp=wide),
            ]
    return out


STRIDES = _strides()
# rows [K fp16 | K fp8] with a gap behind them in, rows [N fp16 | N fp8] with a gap behind them out
STRIDE_F8 = GemmCase(512, 256, 256, "gelu", "w2f8", H16, lda=3 * 256 // 2 + 8, ldo_lp=3 * 256 // 2 + 8, f8_rows=True)


# ------------------------------------------------------------------------------------------------ 3. QKV
QS = 0.160192 * ops.LOG2E


def _qkv():
    out = []
    for dt in (H16, BF16):
        # the 128-tile kernel: D an odd multiple of 64 -- a 128-wide tile straddles two parts, its two wave columns run in different roles
        out.append(QkvCase(2, 70, 64, 64, 128, dt, (7, 10)))            # M = 140: the tile boundary in the middle of the second sequence
        out.append(QkvCase(2, 70, 64, 64, 128, dt))
        out.append(QkvCase(3, 50, 192, 192, 72, dt, (5, 10)))           # a K tail (staged through registers)
        out.append(QkvCase(3, 50, 192, 192, 128, dt, None, QS))
        out.append(QkvCase(2, 70, 320, 320, 64, dt, (7, 10), QS))
        out.append(QkvCase(2, 70, 192, 64, 128, dt, (7, 10)))           # grouped: N = 192 + 64 + 64, k ends and v begins inside one tile
        out.append(QkvCase(2, 70, 192, 64, 128, dt, None, QS))
        out.append(QkvCase(260, 1, 320, 320, 128, dt))                  # S = 1: every row its own sequence
        out.append(QkvCase(260, 1, 64, 64, 64, dt, (1, 1)))
        # the 256-tile kernel: seq_len % 4 != 0 -- the 4 tokens of a lane's V^T store span two sequences; tiles end inside sequences
        out.append(QkvCase(8, 70, 256, 256, 128, dt, (7, 10), QS))
        out.append(QkvCase(8, 70, 256, 256, 64, dt, None, QS))
        out.append(QkvCase(8, 70, 256, 256, 192, dt, (7, 10), 0.0, ldvt=136))   # ldvt > vt_ld(S) = 128
        out.append(QkvCase(260, 1, 256, 256, 128, dt, None, QS))
        out.append(QkvCase(260, 1, 256, 256, 64, dt, (1, 1)))
    return out


QKV = _qkv()


# ------------------------------------------------------------------------------------------------ 4. ConvT
CONVT_HW = ((1, 1), (1, 3), (3, 1), (5, 7))


def _convt():
    """per grid: M = 1 (or one image), M below 128, M just above 256; s = 2 and 4 with N = s s Co = 128 or 256 (every form) and once N = 96 / K = 72 (the
    128-tile kernel alone)"""
    batches = {(1, 1): (1, 100, 257), (1, 3): (1, 20, 86), (3, 1): (1, 33, 87), (5, 7): (1, 3, 8)}
    out = []
    for gi, (h, w) in enumerate(CONVT_HW):
        for bi, B in enumerate(batches[(h, w)]):
            for s in (2, 4):
                co = (32, 64)[(gi + bi) % 2] if s == 2 else (8, 16)[(gi + bi) % 2]
                ci = (64, 128, 192)[(gi + bi + s) % 3]
                for split, dt in ((None, H16), (None, BF16), ("x3", H16), ("x3", BF16)):
                    out.append(ConvTCase(B, h, w, ci, co, s, split, dt))
    for dt in (H16, BF16):
        out.append(ConvTCase(9, 5, 7, 72, 24, 2, None, dt))       # N = 96, K tail: M = 315
        out.append(ConvTCase(86, 1, 3, 96, 12, 4, "x3", dt))      # N = 192, K = 96 (Kpad 128)
    return out


CONVT = _convt()


# ------------------------------------------------------------------------------------------------ 5. a persistent workgroup's second tile
def second_tile_M(n_cu, extra=4):
    return BM * (n_cu + extra)


def second_tile_cases(n_cu):
    """more 256-row tiles than CUs (rows of period 3 or 5 tiles); K = 256 / 320: four and five K-tiles through the five-slot ring of the
    hand-scheduled kernel"""
    M = second_tile_M(n_cu)
    out = []
    for dt in (H16, BF16):
        for N, K, P in ((256, 64, 5), (512, 192, 3), (128, 64, 5), (256, 256, 3), (256, 320, 5), (512, 320, 3)):
            out.append(GemmCase(M, N, K, "resf32", None, dt, P=P))
            out.append(GemmCase(M, N, K, "gelu", None, dt, P=P))
            if K < 256:
                out.append(GemmCase(M, N, K, "both", "x3", dt, P=P))
            else:
                out.append(GemmCase(M, N, K, "f32", "w2", dt, P=P))
        for K, P in ((64, 5), (192, 3)):
            out.append(QkvCase(n_cu + 4, 256, 256, 256, K, dt, (16, 16), QS, P=P))
        for K, P in ((256, 5), (320, 3)):
            out.append(QkvCase(n_cu + 4, 256, 256, 256, K, dt, (16, 16) if P == 5 else None, QS, P=P))
    return out


def second_tile_sels(c):
    """the persistent forms a second-tile case runs on, and the one-tile-per-workgroup form (5) they must equal bit for bit"""
    if c.kind == "gemm" and c.N == 128:
        sels = [4, 5]
    else:
        sels = [2, 3, 5]
    return sels + ([6] if eligible_asm(c) else [])


def period_hides_a_stale_tile(c, n_cu):
    """as conv_cases.period_hides_a_stale_tile: a workgroup's second tile lies n_cu tiles after its first (the hand-scheduled kernel: n_cu rounded
    down to a multiple of 8)"""
    return n_cu % c.period == 0 or (n_cu // 8 * 8) % c.period == 0


# every case that does not depend on the device
STATIC = EDGES + STRIDES + [STRIDE_F8] + QKV + CONVT


# ------------------------------------------------------------------------------------------------ float64 references
def _seed(c):
    return 2000 + c.M * 7 + c.N * 3 + c.K + sum(map(ord, c.id)) % 1000


def build_gemm(c):
    """Operands of one period (CPU), packed weights and the float64 reference.  Keys: a, a_lo, w, w_scale, bias, rowadd, x (the fp32 residual), pre_act (A W^T + bias), res
    ([(hi, lo), (hi, lo)] or None), ref: {"f32", "lp"} -> what the fp32 output / the lowp output planes must (sum to) [, "f8": see f8 rows]"""
    g = torch.Generator().manual_seed(_seed(c))
    R, dt, spec = c.rows, c.dtype, c.spec
    d = dict(a_lo=None, w_scale=None, bias=None, rowadd=None, x=None, res=None)
    if c.split == "w2f8":
        from test_gemm_asm_gpu import _f8_operands
        d["a"], d["w"], d["w_scale"], y, _, _ = _f8_operands(R, c.K, c.N, _seed(c))
        a32 = w32 = None
    else:
        a32 = torch.randn((R, c.K), generator=g)
        w32 = torch.randn((c.N, c.K), generator=g) * c.K ** -0.5
        d["w"] = ops.pack_linear_weight(w32, dt, split=c.split is not None)
        if c.split == "x3":
            d["a"], d["a_lo"] = ops.split_planes(a32, dt)
            y = a32.double() @ w32.double().t()
        else:
            d["a"] = a32.to(dt)
            y = d["a"].double() @ (w32.double() if c.split == "w2" else w32.to(dt).double()).t()
    d["a32"], d["w32"] = a32, w32
    if spec["bias"]:
        d["bias"] = torch.randn(c.N, generator=g)
        y = y + d["bias"].double()
    d["pre_act"] = y
    if spec["act"] == "gelu":
        y = F.gelu(y)
    elif spec["act"] == "relu":
        y = F.relu(y)
    if spec.get("rowadd"):
        d["rowadd"] = torch.randn((-(-c.M // c.div), c.N), generator=g)
        y = y + d["rowadd"].double().repeat_interleave(c.div, 0)[:R]
    if spec.get("res_f32"):
        d["x"] = torch.randn((R, c.N), generator=g)
        y = y + d["x"].double()
    if spec.get("res_lp"):
        r32 = torch.randn((2, R, c.N), generator=g)
        d["res"] = [ops.split_planes(r32[i], dt) if c.split == "x3" else (r32[i].to(dt), None) for i in range(2)]
        y = y + sum(hi.double() + (lo.double() if lo is not None else 0.0) for hi, lo in d["res"])
    d["ref"] = y
    return d


def build_qkv(c):
    """-> a, w (packed [q | k | v] rows), bias, cos / sin (or None), ref: {"q", "k", "v"} ([rows][D] each, v not transposed) for one period"""
    g = torch.Generator().manual_seed(_seed(c))
    R, dt = c.period * c.S, c.dtype
    a = torch.randn((R, c.K), generator=g).to(dt)
    w = (torch.randn((c.N, c.K), generator=g) * c.K ** -0.5).to(dt)
    bias = torch.randn(c.N, generator=g) * 0.1
    y = a.double() @ w.double().t() + bias.double()
    rq, rk, rv = y[:, :c.Dq], y[:, c.Dq:c.Dq + c.Dkv], y[:, c.Dq + c.Dkv:]
    cos = sin = None
    if c.grid:
        gh, gw = c.grid
        cos, sin = ops.rope_tables(max(gh, gw), 100.0, "cpu")
        p = torch.arange(R) % c.S
        rq = _rope_ref(rq.reshape(R, c.Dq // 64, 64), p // gw, p % gw, cos, sin).reshape(R, c.Dq)
        rk = _rope_ref(rk.reshape(R, c.Dkv // 64, 64), p // gw, p % gw, cos, sin).reshape(R, c.Dkv)
    if c.q_scale:
        rq = rq * c.q_scale
    return dict(a=a, w=ops.pack_linear_weight(w.float(), dt), w_rows=w, bias=bias, cos=cos, sin=sin, ref=dict(q=rq, k=rk, v=rv))


def pixel_shuffle(y, c):
    """[M][(dy s + dx) Co + co] -> (B, h s, w s, Co): every output pixel gets exactly one tap"""
    return y.reshape(c.B, c.h, c.w, c.s, c.s, c.Co).permute(0, 1, 3, 2, 4, 5).reshape(c.B, c.h * c.s, c.w * c.s, c.Co)


def build_convt(c):
    """-> x, x_lo (NHWC), w (packed), bias (tiled), wt / bias32 (the ConvTranspose2d parameters), ref (B, h s, w s, Co)"""
    g = torch.Generator().manual_seed(_seed(c))
    dt = c.dtype
    x32 = torch.randn((c.B, c.h, c.w, c.Ci), generator=g)
    wt = torch.randn((c.Ci, c.Co, c.s, c.s), generator=g) * c.Ci ** -0.5
    bias = torch.randn(c.Co, generator=g)
    wp, bt = ops.pack_convT_weight(wt, bias, dt, split=c.split is not None)
    rows = wt.permute(2, 3, 1, 0).reshape(c.N, c.Ci)
    if c.split == "x3":
        x, x_lo = ops.split_planes(x32, dt)
        y = x32.double().reshape(c.M, c.Ci) @ rows.double().t()
    else:
        x, x_lo = x32.to(dt), None
        y = x.double().reshape(c.M, c.Ci) @ rows.to(dt).double().t()
    y = y + bt.double()
    return dict(x=x, x_lo=x_lo, w=wp, bias=bt, wt=wt, bias32=bias, x32=x32, ref=pixel_shuffle(y, c))


# ------------------------------------------------------------------------------------------------ guarded placement
SENTINEL32 = (SENTINEL << 16) | SENTINEL   # finite as fp32: what an fp32 output buffer holds outside its outputs


def guarded_rows(t, ld, dev, margin_rows=2):
    """t [rows][width] as a view with row stride ld >= width inside a 0xFF-filled buffer (conv_cases.guarded_operand): the gap columns of every row
    are NaN patterns as well"""
    rows, width = t.shape
    assert ld >= width
    if ld == width:
        view, buf = guarded_operand(t, dev, margin_rows * ld * t.element_size())
        return view, buf
    full = torch.full((rows, ld * t.element_size()), 0xFF, dtype=torch.uint8).view(t.dtype)
    full[:, :width] = t
    view, buf = guarded_operand(full, dev, margin_rows * ld * t.element_size())
    return view[:, :width], buf


@dataclasses.dataclass
class Guarded:
    view: torch.Tensor    # [rows][width], row stride ld
    buf: torch.Tensor     # the whole buffer, as sentinel-sized integers
    lead: int
    rows: int
    width: int
    ld: int


def strided_out(rows, width, ld, dtype, dev):
    """an output view [rows][width] with row stride ld >= width inside a buffer of sentinel words (32-bit ones for a 32-bit dtype): three rows and
    16 bytes before and behind, 16-byte aligned"""
    assert ld >= width
    wide = torch.empty((), dtype=dtype).element_size() == 4
    per16 = 4 if wide else 8
    lead = (3 * ld + per16 - 1) // per16 * per16 + per16
    buf = torch.full((lead + rows * ld + lead,), SENTINEL32 if wide else SENTINEL, dtype=torch.int32 if wide else torch.int16, device=dev)
    view = buf[lead:lead + rows * ld].view(dtype).view(rows, ld)[:, :width]
    assert view.data_ptr() % 16 == 0 and view.stride(0) == ld
    return Guarded(view, buf, lead, rows, width, ld)


def guards_intact(g):
    """the words before and behind the outputs AND in the gap columns [width, ld) of every row are the bits written there"""
    s = SENTINEL32 if g.buf.dtype == torch.int32 else SENTINEL
    body = g.buf[g.lead:g.lead + g.rows * g.ld].view(g.rows, g.ld)
    return bool((g.buf[:g.lead] == s).all()) and bool((g.buf[g.lead + g.rows * g.ld:] == s).all()) and bool((body[:, g.width:] == s).all())
