"""The DPT head on the HIP kernels (heads/dpt_head.py:42-129 of the reference), its packed weights and the views per launch.  `fmt` is the
model's OperandFormat (fast3r.py); read here: `lp`, `planes`, `head_f8` and the two per-view row thresholds."""
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import ops
from .packing import _f32
from .params import PixelwiseTaskWithDPT


class _PackedHead:
    pass


class _ConvW:
    """A packed 3x3 convolution weight: `w` for split None / "x3" (ops.pack_conv3x3_weight) and, when the head runs its correction products on the
    fp8 MFMA (Fast3R.head_corrections = "fp8") and Cin % 128 == 0, `w8` / `scale` for split "x3f8" (ops.pack_conv3x3_weight_f8)."""
    __slots__ = ("w", "w8", "scale")

    def __init__(self, w, w8=None, scale=None):
        self.w, self.w8, self.scale = w, w8, scale


def _pack_head(head: PixelwiseTaskWithDPT, fmt):
    d = head.dpt
    h = _PackedHead()
    ap = d.act_postprocess
    lp, split = fmt.lp, fmt.planes
    lin = lambda w: ops.pack_linear_weight(w.detach().float(), lp, split)

    def c33(w):
        w = w.detach().float()
        if fmt.head_f8 and w.shape[1] % 128 == 0:
            return _ConvW(ops.pack_conv3x3_weight(w, lp, split), *ops.pack_conv3x3_weight_f8(w))
        return _ConvW(ops.pack_conv3x3_weight(w, lp, split))
    h.a_w = [lin(ap[i][0].weight) for i in range(4)]
    h.a_b = [_f32(ap[i][0].bias) for i in range(4)]
    # The transposed convolutions write their output with the channel count rounded up to 64 (layer_dims[0] = 96 -> 128 zero-weight / zero-bias
    # channels, matched by zero input channels in layer1_rn's weight: exact): the 3x3 convolution behind them then has a channel count the
    # 256-tile kernel's LDS-DMA staging takes (a ragged one ran on the 128-tile kernel through registers: 13.8 of 126 ms of head convolutions at N = 100).
    def convT_padded(m):
        w, b = m.weight.detach().float(), m.bias.detach().float()
        pad = ops.round_up(w.shape[1], 64) - w.shape[1]
        if pad:
            w, b = nn.functional.pad(w, (0, 0, 0, 0, 0, pad)), nn.functional.pad(b, (0, pad))
        return ops.pack_convT_weight(w, b, lp, split) + (w.shape[1],)

    def rn(i):
        w = getattr(d.scratch, f"layer{i + 1}_rn").weight.detach().float()
        pad = ops.round_up(w.shape[1], 64) - w.shape[1] if i < 2 else 0   # (levels 0 / 1 read the transposed convolutions' padded outputs)
        return c33(nn.functional.pad(w, (0, 0, 0, 0, 0, pad)) if pad else w)
    h.t0_w, h.t0_b, h.t0_cout = convT_padded(ap[0][1])
    h.t1_w, h.t1_b, h.t1_cout = convT_padded(ap[1][1])
    h.c3_w, h.c3_b = c33(ap[3][1].weight), _f32(ap[3][1].bias)
    h.rn_w = [rn(i) for i in range(4)]
    h.ref = []
    for i in range(1, 5):
        r = getattr(d.scratch, f"refinenet{i}")
        convs = dict(u1c1=r.resConfUnit1.conv1, u1c2=r.resConfUnit1.conv2, u2c1=r.resConfUnit2.conv1, u2c2=r.resConfUnit2.conv2)
        h.ref.append(dict({k: (c33(c.weight), _f32(c.bias)) for k, c in convs.items()}, out=(lin(r.out_conv.weight), _f32(r.out_conv.bias))))
    h.h0_w, h.h0_b = c33(d.head[0].weight), _f32(d.head[0].bias)
    h.h2_w, h.h2_b = c33(d.head[2].weight), _f32(d.head[2].bias)
    h.h4_w = d.head[4].weight.detach().float().reshape(d.num_channels, -1).contiguous()
    h.h4_b = _f32(d.head[4].bias)
    h.dims = d.layer_dims
    h.feature_dim, h.last_dim, h.num_channels, h.patch_size = d.feature_dim, d.last_dim, d.num_channels, d.patch_size
    h.depth_mode, h.conf_mode = head.depth_mode, head.conf_mode
    h.fin = None
    if d.last_dim == 128 and h.h4_w.shape[1] == 128:  # the fused tail (f3r_gemm_args.fin_w): head[4] as a zero-padded [4][128] matrix
        try:
            h.fin = ops.dpt_fin_args(h.h4_w, h.h4_b, h.conf_mode, tuple(h.depth_mode))
        except (ValueError, AssertionError):
            h.fin = None  # an unsupported mode raises where the reference raises: in the head's own call (ops.dpt_final)
    return h


# ======================================================================================= launch forms
# (the `rows * channels * 2 < 2^32` clauses depend on the chunk, and head[2]'s Cin is feature_dim // 2, not last_dim: ADVICE.md item 3, kept as they are)
def use_f8(on, has_w8, rows_per_view, rows, cin, min_rows):
    """Does a 3x3 convolution run split "x3f8"?  on: OperandFormat.head_f8; has_w8: its weight has an fp8 pack (_ConvW.w8)."""
    # decided by the pixels of ONE view (rows_per_view), so that a forward computes the same numbers whatever max_parallel_views_for_head is;
    # the operand of a launch must stay below 4 GiB (32-bit lane offsets of the 256-tile kernel: 63 views of 512 x 512 x 128 channels)
    return bool(on and has_w8 and cin % 128 == 0 and rows_per_view >= min_rows and rows * cin * 2 < (1 << 32))


def tail_fused(has_fin, rows_per_view, rows, last_dim, min_rows):
    """head[2] + head[3] + head[4] + postprocess in one launch (when the 256 x 128 tile kernel takes it)?  has_fin: _PackedHead.fin was built."""
    return has_fin and rows_per_view >= min_rows and last_dim % 64 == 0 and rows * last_dim * 2 < (1 << 32)


# ======================================================================================= activations
class Act(NamedTuple):
    """An NHWC activation: the fp16 / bf16 high plane, the 16-bit low plane (None = not carried) and the fp8 planes (None = not carried)."""
    hi: torch.Tensor
    lo: Optional[torch.Tensor] = None
    f8: Optional[torch.Tensor] = None


class Feat(NamedTuple):
    """A convolution's output and, when a ResidualConvUnit follows, the pre-activated copy relu(x) its first convolution reads."""
    x: Act
    relu: Optional[Act] = None


# Which planes a producer writes beside `hi` follows from its CONSUMER: a residual add, a 1x1 conv, an upsample or an "x3" convolution read
# hi + lo (lo only in the formats that carry planes); a 3x3 convolution that runs split "x3f8" (to_f8) reads hi + f8 and needs no lo.
def _writes(fmt, to_f8):
    """-> (write lo, write f8) for a producer whose consumer is (to_f8) / is not an "x3f8" convolution."""
    return fmt.planes and not to_f8, to_f8


def _linear(fmt, hi, lo, w, b, shape):
    """1x1 convolution of the planes (hi, lo) -> Act viewed as `shape`."""
    C = hi.shape[-1]
    r = ops.gemm(hi.view(-1, C), w, bias=b, want_lp=True, want_lo=fmt.planes, split="x3" if fmt.planes else None,
                 a_lo=None if lo is None else lo.view(-1, C))
    return Act(*(t.view(shape) for t in r[1:]))


def _convT(fmt, x, w, b, s, cout):
    r = ops.convT(x.hi, w, b, s, cout, split="x3" if fmt.planes else None, x_lo=x.lo, want_lo=fmt.planes)
    return Act(*r) if fmt.planes else Act(r)


def _conv_operands(fmt, x, w):
    """-> (packed weight, operand arguments) of a 3x3 convolution over x."""
    if x.f8 is not None:  # the producer wrote fp8 planes because this launch takes them
        return w.w8, dict(split="x3f8", x_f8=x.f8, w_scale=w.scale)
    return w.w, dict(split="x3" if fmt.planes else None, x_lo=x.lo)


def _conv(fmt, x, w, bias=None, stride=1, act=None, res=None, res2=None, to_f8=False, relu_to_f8=None):
    """3x3 convolution (+ residuals res, res2).  to_f8: the output's consumer is an "x3f8" convolution; relu_to_f8: None = no relu copy, else
    whether the copy's consumer is one (_writes)."""
    wt, kw = _conv_operands(fmt, x, w)
    want_lo, want_f8 = _writes(fmt, to_f8)
    want_relu_lo, want_relu_f8 = _writes(fmt, bool(relu_to_f8))
    r = ops.conv3x3(x.hi, wt, stride=stride, bias=bias, act=act,
                    res_lp=None if res is None else res.hi, res_lp_lo=None if res is None else res.lo,
                    res_lp2=None if res2 is None else res2.hi, res_lp2_lo=None if res2 is None else res2.lo,
                    want_lo=want_lo, want_relu=relu_to_f8 is not None, want_f8=want_f8, want_relu_lo=want_relu_lo, want_relu_f8=want_relu_f8, **kw)
    if not isinstance(r, dict):
        return Feat(Act(r))
    return Feat(Act(r["out"], r.get("out_lo"), r.get("out_f8")),
                None if relu_to_f8 is None else Act(r["relu"], r.get("relu_lo"), r.get("relu_f8")))


def _resize(fmt, fn, x, size, to_f8=False):
    """fn: ops.upsample2x (size: crop or None) or ops.interp_bilinear (size: output size)."""
    want_lo, want_f8 = _writes(fmt, to_f8)
    r = fn(x.hi, size, x_lo=x.lo, want_lo=want_lo, want_f8=want_f8)
    return Act(*r) if (want_lo or want_f8) else Act(r)


def _rows(t):
    return t.shape[0] * t.shape[1] * t.shape[2]


# ======================================================================================= the head
def dpt(fmt, hk, toks, nv, gh, gw):
    """DPTOutputAdapter_fix.forward + postprocess (heads/dpt_head.py:42-129) for nv same-size views.
    toks: the 4 hooked token matrices as (lowp [nv*gh*gw][C], low plane or None) pairs.  Activations stay NHWC lowp (two planes
    each in "high" precision, every conv then runs split="x3"); accumulation fp32.  A ResidualConvUnit reads relu(x) for its first
    conv and x for its skip add (dpt_block.py:143-154): the PRODUCER of x writes both (f3r_gemm_args.out_relu), so no conv
    pre-activates its operand while staging it and all of them can use LDS-DMA."""
    ld, F = hk.dims, hk.feature_dim

    def f8(rows, cin, w):
        return use_f8(fmt.head_f8, w.w8 is not None, rows // nv, rows, cin, fmt.head_f8_min_rows)

    def c1(i):  # act_postprocess[i][0]: 1x1 conv on the tokens
        return _linear(fmt, *toks[i], hk.a_w[i], hk.a_b[i], (nv, gh, gw, ld[i]))

    l0 = _convT(fmt, c1(0), hk.t0_w, hk.t0_b, 4, hk.t0_cout)                          # dpt_block.py:416-434 (channels padded to 64: _pack_head)
    l1 = _convT(fmt, c1(1), hk.t1_w, hk.t1_b, 2, hk.t1_cout)                          # :436-454
    l2 = c1(2)                                                                      # :456-464
    l3 = _conv(fmt, c1(3), hk.c3_w, bias=hk.c3_b, stride=2).x                         # :466-481
    # scratch.layer_rn (no bias); the relu copy feeds the first RCU convolution of its level
    ls = [_conv(fmt, l, hk.rn_w[i], relu_to_f8=f8(_rows(l.hi), F, hk.ref[i]["u2c1" if i == 3 else "u1c1"][0]))
          for i, l in enumerate((l0, l1, l2, l3))]
    del l0, l1, l2, l3

    def rcu(x, c1w, c2w, extra=None, relu_to_f8=None):
        # x + conv2(relu(conv1(relu(x)))) (+ extra); x: Feat
        t = _conv(fmt, x.relu, c1w[0], bias=c1w[1], act="relu", to_f8=f8(_rows(x.x.hi), F, c2w[0])).x
        return _conv(fmt, t, c2w[0], bias=c2w[1], res=x.x, res2=extra, relu_to_f8=relu_to_f8)

    def fusion(r, path, skip=None, crop=None, out_f8=False):
        # out_conv(up2(RCU2(path + RCU1(skip)))); the 1x1 out_conv commutes exactly with the bilinear
        # interpolation (both linear, weights sum to 1), so it runs BEFORE the upsample on 4x fewer pixels.
        if skip is not None:
            path = rcu(skip, r["u1c1"], r["u1c2"], extra=path, relu_to_f8=f8(_rows(skip.x.hi), F, r["u2c1"][0]))
        y = rcu(path, r["u2c1"], r["u2c2"]).x
        return _resize(fmt, ops.upsample2x, _linear(fmt, y.hi, y.lo, *r["out"], y.hi.shape), crop, to_f8=out_f8)

    p4 = fusion(hk.ref[3], ls[3], None, crop=(ls[2].x.hi.shape[1], ls[2].x.hi.shape[2]))  # dpt_head.py:69-71
    p3 = fusion(hk.ref[2], p4, ls[2])
    p2 = fusion(hk.ref[1], p3, ls[1])
    B1, h1, w1 = ls[0].x.hi.shape[:3]
    p1 = fusion(hk.ref[0], p2, ls[0], out_f8=f8(B1 * 4 * h1 * w1, F, hk.h0_w))
    del ls, p4, p3, p2
    y = _conv(fmt, p1, hk.h0_w, bias=hk.h0_b).x                                       # head[0]
    # head[1]: Interpolate(scale_factor = patch_size / 8, bilinear, align_corners=True) (dpt_block.py:374): x2 for patch 16, x1.75 for 14
    full = (y.hi.shape[1] * hk.patch_size // 8, y.hi.shape[2] * hk.patch_size // 8)
    rows2 = y.hi.shape[0] * full[0] * full[1]
    u = _resize(fmt, ops.interp_bilinear, y, full, to_f8=f8(rows2, hk.last_dim, hk.h2_w))
    # head[2], head[3] (+ head[4] and postprocess in the same launch when the 256 x 128 tile kernel takes it)
    if tail_fused(hk.fin is not None, rows2 // nv, rows2, hk.last_dim, fmt.head_tail_fused_min_rows):
        wt, kw = _conv_operands(fmt, u, hk.h2_w)
        return ops.conv3x3(u.hi, wt, bias=hk.h2_b, act="relu", fin=hk.fin, **kw)
    y = _conv(fmt, u, hk.h2_w, bias=hk.h2_b, act="relu").x
    return ops.dpt_final(y.hi, hk.h4_w, hk.h4_b, hk.conf_mode, x_lo=y.lo, depth_mode=tuple(hk.depth_mode))  # head[4] + postprocess


def chunk_views(limit, gh, gw, cus=256):
    """Views per head launch: the count in (limit / 2, limit] whose convolution launches fill the chip's rounds best.  max_parallel_views_for_head
    (the reference's 25, fast3r.py:68) bounds the head's memory; the results do not depend on the chunking (tested bit for bit), so inside that
    bound the chunk is chosen for the 256-row output tiles of the big 3x3 convolutions: at 512 x 512, 25 views are 1 600 tiles = 6.25 rounds of 256
    workgroups at the 128 x 128 level and 1.56 at 64 x 64 (11 % / 22 % of those launches idle), 16 views are 4 and 1 round exactly.  Cost model:
    sum over the levels of (FLOPs per pixel) x rounds(c) / c."""
    if limit <= 2:
        return limit
    t = gh * gw   # pixels per view at the token grid; levels at 1/4, 1, 4, 16 (RCU convolutions), 64 (head[0]), 256 (head[2]) times that
    levels = [(t // 4, 2 * 256 * 256), (t, 4 * 256 * 256), (4 * t, 4 * 256 * 256), (16 * t, 4 * 256 * 256), (64 * t, 256 * 128), (256 * t, 128 * 128)]
    best, best_cost = limit, None
    for c in range(limit, max(1, limit // 2), -1):
        cost = sum(w * (-(-(-(-c * max(px, 1) // 256)) // cus)) for px, w in levels) / c
        if best_cost is None or cost < best_cost * 0.995:   # (ties and near-ties: the larger chunk = fewer launches)
            best, best_cost = c, cost
    return best
