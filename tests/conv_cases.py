"""Seeded cases of the 3x3 implicit-GEMM convolution at the edges of its geometry, their float64 references and the guarded placement of
their device tensors -- shared by tests/test_conv_cases.py (no GPU: the references against F.conv2d, the case lists against the structural
properties they are there for) and tests/test_conv_geometry_gpu.py (the kernels against the references).

A case names (B, H, W, Ci, Co, stride, split, dtype, extras) and a period P: image b carries the content of image b mod P, so the reference is
computed for P images and compared against all B (the cases that need more output tiles than the chip has CUs stay cheap on the host).

What the reference is, by split (the float64 sum of exactly the products the kernel forms):
  None    the operands rounded to the case's dtype
  "x3"    (x_hi + x_lo) against the unrounded fp32 weights (the kernel drops only lo x lo)
  "x3f8"  the decoded planes: fp16 hi x hi + e4m3 hi8 x lo8 + lo8 x hi8 with their power-of-two scales (planes_ref)
"""
import dataclasses
import math

import torch
import torch.nn.functional as F

from fast3r_amd import ops

H16, BF16 = torch.float16, torch.bfloat16
BM = 256             # output rows of a tile of the 256-tile kernel
TAB_ENTRIES = 512    # records of its K-tile table (TileCfg::TAB_ENTRIES in csrc/f3r_gemm256_impl.h)
CU_NOMINAL = 256     # CUs of an MI355X: what the shape-only checks of the second-tile cases assume


@dataclasses.dataclass(frozen=True)
class ConvCase:
    B: int
    H: int
    W: int
    Ci: int
    Co: int
    stride: int = 1
    split: object = None          # None | "x3" | "x3f8"
    dtype: torch.dtype = H16
    extras: tuple = ()            # "skips": two lowp skip connections + the relu copy; "fin": the fused head tail; "a_relu": ReLU on the operand
    P: int = 0                    # period of the batch's content (0: every image its own)

    @property
    def period(self):
        return self.P or self.B

    @property
    def out_hw(self):
        return (self.H - 1) // self.stride + 1, (self.W - 1) // self.stride + 1

    @property
    def per_img(self):
        oh, ow = self.out_hw
        return oh * ow

    @property
    def M(self):
        return self.B * self.per_img

    @property
    def id(self):
        dt = "f16" if self.dtype == H16 else "bf16"
        ex = "".join("+" + e for e in self.extras)
        per = f"p{self.P}" if self.P else ""
        return f"{self.B}x{self.H}x{self.W}{per}-c{self.Ci}-n{self.Co}-s{self.stride}-{self.split or 'one'}-{dt}{ex}"


# ------------------------------------------------------------------------------------------------ shape arithmetic (what the kernels do with a case)
def k_tiles(c):
    """K-tiles of the 256-tile kernel = records it writes into its table (gemm256_body's nk): 9 C / 64 per plane product"""
    nk1 = 9 * ((c.Ci + 63) // 64)
    return {None: nk1, "w2": 2 * nk1, "x3": 3 * nk1, "x3f8": nk1 + 2 * (nk1 // 2)}[c.split]


def eligible256(c):
    """f3r_gemm256_eligible restated for these cases (no additive term together with an activation occurs in them)"""
    if c.Co % 128 or c.Ci % 64 or "a_relu" in c.extras or k_tiles(c) > TAB_ENTRIES:
        return False
    if c.split == "x3f8" and (c.Ci % 128 or c.dtype != H16):
        return False
    return "fin" not in c.extras or c.Co == 128


def kernel_sels(c):
    """the kernel forms that take the case: 1 = 128-tile kernel, 2 / 3 = 256-tile kernel staggered / lock-step, 4 = its 256 x 128 tile form,
    0 = by shape.  "x3f8" and the fused tail have one kernel family and no second path: 0 only."""
    if c.split == "x3f8" or "fin" in c.extras:
        return [0]
    return [1, 2, 3, 4, 0] if eligible256(c) else [1, 0]


def m_tiles(c):
    return (c.M + BM - 1) // BM


def tiles(c, bn):
    return m_tiles(c) * ((c.Co + bn - 1) // bn)


def images_in_tile(c, t):
    """how many images have output rows in m-tile t"""
    lo, hi = t * BM, min(c.M, (t + 1) * BM) - 1
    return hi // c.per_img - lo // c.per_img + 1


def second_tile_B(n_cu, per_img=255, extra=4):
    """the batch that gives about n_cu + extra m-tiles"""
    return -(-(n_cu + extra) * BM // per_img)


# ------------------------------------------------------------------------------------------------ the case lists
def _tiny():
    # (B, H, W): H and W of 1 .. 5 (and the 1 x 7 strip), M below 256 and just above it at either stride
    shapes = [(300, 1, 1), (7, 2, 3), (37, 1, 7), (60, 1, 5), (52, 5, 1), (65, 2, 2), (90, 3, 1), (3, 4, 5), (30, 3, 3), (11, 5, 5), (260, 2, 2),
              (130, 3, 1), (87, 5, 2)]
    cn = [(64, 128), (128, 256), (192, 128), (64, 256), (128, 128), (192, 256)]
    out = []
    for i, (b, h, w) in enumerate(shapes):
        for stride in (1, 2):
            ci, co = cn[(i + stride) % len(cn)]
            for dt in (H16, BF16):
                out.append(ConvCase(b, h, w, ci, co, stride, None, dt, ("bias",)))
                out.append(ConvCase(b, h, w, ci, co, stride, "x3", dt, ("bias",)))
            out.append(ConvCase(b, h, w, 128, co, stride, "x3f8", H16, ("bias",)))
    for dt in (H16, BF16):  # two skip connections and the relu copy: a tile of six whole images and a ragged end, one of 43 and a ragged end
        out.append(ConvCase(37, 1, 7, 192, 128, 1, None, dt, ("bias", "skips")))
        out.append(ConvCase(43, 2, 3, 64, 256, 1, "x3", dt, ("bias", "skips")))
    return out


TINY = _tiny()

# stride 2 with both parities of H and W: the bottom / right taps leave the image only for odd sizes
STRIDE2 = [ConvCase(3, h, w, ci, co, 2, split, dt, ("bias",))
           for (h, w), (ci, co) in zip([(4, 4), (5, 4), (4, 5), (5, 5), (8, 7)], [(64, 128), (128, 256), (192, 128), (128, 128), (64, 256)])
           for split, dt in ((None, H16), (None, BF16), ("x3", H16), ("x3", BF16))] + \
          [ConvCase(3, h, w, 128, co, 2, "x3f8", H16, ("bias",)) for (h, w), co in zip([(4, 4), (5, 4), (4, 5), (5, 5), (8, 7)], [128, 256, 128, 256, 128])]

# the 128-tile kernel's channel tails (C % 64 != 0 down to one 16-byte chunk), with and without the ReLU on the operand
TAILS = [ConvCase(3, h, w, ci, co, stride, None, dt, ("bias", "a_relu") if relu else ("bias",))
         for ci in (8, 24, 72, 136) for (h, w, co) in ((3, 3, 64), (5, 6, 40)) for stride in (1, 2) for relu in (False, True) for dt in (H16, BF16)]


def second_tile_cases(n_cu):
    """more output tiles than CUs: a persistent workgroup walks a second tile.  15 x 17 images = 255 pixels (every tile straddles images), content of
    period 5"""
    B = second_tile_B(n_cu)
    out = []
    for split, dt in ((None, H16), (None, BF16), ("x3", H16), ("x3", BF16), ("x3f8", H16)):
        for fin in (False, True):
            out.append(ConvCase(B, 15, 17, 128, 128, 1, split, dt, ("bias", "fin") if fin else ("bias",), P=5))
    out.append(ConvCase(B, 30, 34, 128, 128, 2, "x3", H16, ("bias",), P=5))      # stride 2, the same output size
    out.append(ConvCase(B, 30, 34, 128, 128, 2, "x3f8", H16, ("bias",), P=5))
    out.append(ConvCase(B, 15, 17, 64, 256, 1, None, H16, ("bias",), P=5))       # the 256 x 256 tile form with an odd K-tile count (9)
    out.append(ConvCase(B, 15, 17, 1152, 128, 1, "x3", H16, ("bias",), P=5))     # the fullest table (486 records) walked twice
    return out


def period_hides_a_stale_tile(c, n_cu):
    """a workgroup's second tile lies n_cu tiles after its first: when P divides the CU count a tile computed from the first one's operands could
    carry identical content, and the case proves nothing on that device (the tests skip it)"""
    return n_cu % c.period == 0


# the K-tile table guard: x3 at C = 1216 needs 513 records, x3f8 at C = 1920 needs 540; C = 1152 x3 (486) is the largest x3 shape that fits
GUARD_OVER_X3 = ConvCase(1, 8, 8, 1216, 128, 1, "x3", H16, ("bias",))
GUARD_OVER_F8 = ConvCase(1, 8, 8, 1920, 128, 1, "x3f8", H16, ("bias",))
GUARD_FITS_X3 = ConvCase(1, 8, 8, 1152, 128, 1, "x3", H16, ("bias",))


# ------------------------------------------------------------------------------------------------ float64 references
def dec8(b):
    return b.view(torch.float8_e4m3fn).double()


def decode_weight_f8(wp, sc, co, ci):
    """pack_conv3x3_weight_f8 rows -> (w_hi, w_lo8 decoded, w_hi8 decoded) as float64 (Cout, Cin, 3, 3)"""
    kp = 9 * ci
    raw = wp.view(torch.uint8).view(co, 4 * kp)
    hi = raw[:, :2 * kp].contiguous().view(torch.float16).double()
    e_lo = (sc.long() & 0xff).double()
    e_hi = ((sc.long() >> 8) & 0xff).double()
    lo8 = dec8(raw[:, 2 * kp:3 * kp].contiguous()) * torch.exp2(e_lo - 127)[:, None]
    hi8 = dec8(raw[:, 3 * kp:].contiguous()) * torch.exp2(e_hi - 127)[:, None]
    cv = lambda t: t.view(co, 3, 3, ci).permute(0, 3, 1, 2).contiguous()
    return cv(hi), cv(lo8), cv(hi8)


def conv64(x_nhwc, w, stride=1):
    return F.conv2d(x_nhwc.double().permute(0, 3, 1, 2), w.double(), None, padding=1, stride=stride).permute(0, 2, 3, 1)


def planes_ref(x32, wp, sc, co, ci, stride=1):
    """what split "x3f8" computes, in float64, from the planes the kernel reads -> (sum, x_hi, fp8 planes of x)"""
    x_hi = x32.to(H16)
    p8 = ops.f8_planes(x32)
    a_hi8 = dec8(p8[..., :ci].contiguous())
    a_lo8 = dec8(p8[..., ci:].contiguous()) / 4096.0
    w_hi, w_lo8, w_hi8 = decode_weight_f8(wp, sc, co, ci)
    return conv64(x_hi, w_hi, stride) + conv64(a_hi8, w_lo8, stride) + conv64(a_lo8, w_hi8, stride), x_hi, p8


def periodic(t, B):
    """the (B, ...) batch whose image b is t[b mod P]"""
    P = t.shape[0]
    return t if P == B else t[torch.arange(B) % P].contiguous()


def build(c):
    """Operands (one period of them, on the CPU), packed weights, planes and the float64 reference of a case.
    Keys: x (the operand the launch takes as `x`: the rounded operand / the high plane), x_lo, x_f8, w (packed), w_scale, bias, res (two skip tensors
    or None), fin (dpt_fin_args of the fused tail, or None), ref: {"out": what the output planes must sum to, "relu", "pts", "conf"}."""
    g = torch.Generator().manual_seed(1000 + c.H * 131 + c.W * 17 + c.Ci + c.Co + c.stride)
    P, dt = c.period, c.dtype
    x32 = torch.randn((P, c.H, c.W, c.Ci), generator=g)
    w32 = torch.randn((c.Co, c.Ci, 3, 3), generator=g) * (9 * c.Ci) ** -0.5
    bias = torch.randn(c.Co, generator=g) if "bias" in c.extras else None
    d = dict(x_lo=None, x_f8=None, w_scale=None, bias=bias, res=None, fin=None)
    if c.split is None:
        d["x"], d["w"] = x32.to(dt), ops.pack_conv3x3_weight(w32, dt)
        xin = F.relu(d["x"].double()) if "a_relu" in c.extras else d["x"].double()
        y = conv64(xin, w32.to(dt), c.stride)
    elif c.split == "x3":
        d["x"], d["x_lo"] = ops.split_planes(x32, dt)
        d["w"] = ops.pack_conv3x3_weight(w32, dt, split=True)
        y = conv64(d["x"].double() + d["x_lo"].double(), w32, c.stride)
    else:
        assert c.split == "x3f8" and dt == H16
        d["w"], d["w_scale"] = ops.pack_conv3x3_weight_f8(w32)
        y, d["x"], d["x_f8"] = planes_ref(x32, d["w"], d["w_scale"], c.Co, c.Ci, c.stride)
    if bias is not None:
        y = y + bias.double()
    ref = {}
    if "skips" in c.extras:
        oh, ow = c.out_hw
        r32 = torch.randn((2, P, oh, ow, c.Co), generator=g)
        if c.split is None:
            d["res"] = [(r32[i].to(dt), None) for i in range(2)]
            y = y + d["res"][0][0].double() + d["res"][1][0].double()
        else:
            d["res"] = [ops.split_planes(r32[i], dt) for i in range(2)]
            y = y + sum(hi.double() + lo.double() for hi, lo in d["res"])
        ref["relu"] = F.relu(y)
    if "fin" in c.extras:
        w4 = torch.randn((4, c.Co), generator=g) * 0.08
        b4 = torch.randn(4, generator=g) * 0.1
        d["fin"] = (w4, b4, ("exp", 1.0, math.inf))
        z = F.relu(y) @ w4.double().t() + b4.double()
        n = z[..., :3].norm(dim=-1, keepdim=True)
        ref["pts"] = z[..., :3] / n.clamp_min(1e-8) * torch.expm1(n)
        ref["conf"] = 1.0 + torch.exp(z[..., 3])
    ref["out"] = y
    d["ref"] = ref
    d["x32"], d["w32"] = x32, w32
    return d


# ------------------------------------------------------------------------------------------------ guarded placement
SENTINEL = 0x5A7B   # a finite 16-bit pattern in both formats: what the output buffer holds outside the M * N outputs


def _offset16(nbytes):
    """a 16-byte aligned (and no better) offset of at least nbytes"""
    return ((nbytes + 15) // 16 * 16) | 16


def guarded_operand(t, dev, margin_bytes):
    """t as a contiguous view at a 16-byte aligned offset inside a larger device buffer whose other bytes are 0xFF (NaN in fp16, bf16 and e4m3):
    a load before or behind the plane poisons the output"""
    nb = t.numel() * t.element_size()
    off = _offset16(margin_bytes)
    buf = torch.full((off + nb + _offset16(margin_bytes),), 0xFF, dtype=torch.uint8, device=dev)
    view = buf[off:off + nb].view(t.dtype).view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 32 == 16
    return view, buf


def guarded_out(shape, dtype, dev):
    """an output view inside a buffer of SENTINEL words, three output rows and 16 bytes from either end -> (view, buffer, first, last + 1 element of the view)"""
    n = math.prod(shape)
    lead = 3 * shape[-1] + 8
    buf = torch.full((lead + n + lead,), SENTINEL, dtype=torch.int16, device=dev)
    view = buf[lead:lead + n].view(dtype).view(shape)
    assert view.data_ptr() % 16 == 0
    return view, buf, lead, lead + n


def guards_intact(buf, lo, hi):
    """the words before and behind the outputs are the bits written there"""
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all())
