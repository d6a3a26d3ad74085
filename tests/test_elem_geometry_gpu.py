"""The HBM-bound kernels (csrc/f3r_elem.hip) and the fp32 kernels of precision "exact" (csrc/f3r_exact.hip) at the edges of their geometry, on a
real MI355X through the C ABI: both sides of every dispatch switch (LayerNorm's three register counts, the staged head tail's ragged group,
the vector / scalar patchify), the sizes at which a row, a tile or a workgroup ends (256 queries, 32 keys, 64 pixels), every head width of
the fp32 attention, row strides wider than the rows, causal rows that see no key, and data that tells the right arithmetic from a cheaper
one (cases, float64 references and what each case is there for: tests/elem_cases.py; that they discriminate: tests/test_elem_cases.py).

The module owns every buffer: each input plane lies inside a buffer of 0xFF bytes (NaN in fp16, bf16, e4m3 and fp32), each output inside a
buffer of sentinel words with sentinel gap columns where the entry point takes a row stride.  After each launch: synchronise, guards intact,
then the comparison, at the tolerance the project already holds that kind of output to (fp32 outputs 2e-5, lowp lp_tol, hi + lo planes
split_tol, the head tail 1e-5, fp32 attention 3e-6 / 3e-5, fp32 rotary embedding 2e-6); the measured figure is printed before it is asserted.
"""
import ctypes

import pytest
import torch

import elem_cases as ec
from elem_cases import BF16, F32, H16
from fast3r_amd import _lib, ops
from gemm_cases import Guarded
from test_gemm256_gpu import split_tol
from test_kernels_gpu import DEV, lp_tol

pytestmark = pytest.mark.gpu
ID = dict(ids=lambda c: c.id)


def check(kind, got, ref, tol, what):
    """test_kernels_gpu.assert_close, with the figure printed before it is asserted"""
    got, ref = got.detach().double().cpu().reshape(ref.shape), ref.double()
    scale = float(ref.abs().max().clamp_min(1e-6))
    err = float((got - ref).abs().max())
    print(f"[elem-geometry] kind={kind} rel_err={err / scale:.3e} tol={tol:.1e} {what}")
    assert err == err and err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol:.1e})"


class Bufs:
    """the device buffers of one launch: operands in guarded placement, outputs in sentinel buffers"""

    def __init__(self):
        self.keep, self.outs = [], []

    def op(self, t, margin=64):
        if t is None:
            return None
        view, buf = ec.guarded_operand(t, DEV, margin)
        self.keep.append(buf)
        return view

    def rows(self, t, ld):
        view, buf = ec.guarded_rows(t, ld, DEV)
        self.keep.append(buf)
        return view

    def out(self, rows, width, ld, dtype, want=True):
        if not want:
            return None
        g = ec.strided_out(rows, width, ld, dtype, DEV)
        self.outs.append(g)
        return g

    def intact(self, what):
        torch.cuda.synchronize()
        for g in self.outs:
            assert ec.guards_intact(g), f"{what}: a store outside the {g.rows} x {g.width} outputs (row stride {g.ld})"


def P(g):
    """device address of a tensor or of a guarded output (None -> NULL)"""
    if g is None:
        return None
    return ops.ptr(g.view if isinstance(g, Guarded) else g)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def dt_name(dt):
    return "f16" if dt == H16 else "bf16"


# ================================================================================================ LayerNorm / RMSNorm
def _layernorm(lib, b, d, c_rows, D, eps, rms, dtype, want_lp, want_f32):
    x, g, beta = b.op(d["x"], 2 * D * 4), b.op(d["gamma"]), b.op(d["beta"])
    lp, f32 = b.out(c_rows, D, D, dtype, want_lp), b.out(c_rows, D, D, F32, want_f32)
    _lib.check(lib.f3r_layernorm(P(x), P(g), P(beta), P(lp), P(f32), c_rows, D, float(eps), int(rms), ops.dtype_id(dtype), ops.stream_ptr()), "f3r_layernorm")
    return lp, f32


@pytest.mark.parametrize("c", ec.LN, **ID)
def test_layernorm(built_lib, c):
    """three instantiations (4 / 8 / 32 float4 per lane) on both sides of their switches, widths at which only some lanes hold a vector, 1 .. 5
    rows of a 4-row workgroup, every output combination; rows of mean 100 (a one-pass variance loses them) and constant rows (output == beta)"""
    d, b = ec.build_ln(c), Bufs()
    lp, f32 = _layernorm(built_lib, b, d, c.rows, c.D, c.eps, c.rms, c.dtype, c.outs in ("lp", "both"), c.outs in ("f32", "both"))
    b.intact(c.id)
    kind = f"{'rms' if c.rms else 'ln'}-{c.data}"
    if f32 is not None:
        check(f"{kind}-f32", f32.view, d["ref"], 2e-5, c.id)
    if lp is not None:
        check(f"{kind}-{dt_name(c.dtype)}", lp.view.float(), d["ref"], lp_tol(c.dtype), c.id)
    if c.data == "equal":
        want = d["beta"].expand(c.rows, c.D)
        assert torch.equal(bits(f32.view), bits(want)) and torch.equal(bits(lp.view), bits(want.to(c.dtype))), f"{c.id}: a constant row must give beta"


@pytest.mark.parametrize("c", ec.LN_F8, **ID)
def test_layernorm_f8_rows(built_lib, c):
    """rows [D fp16 | D e4m3 | pad]: the fp16 part is f3r_layernorm's output bit for bit, the fp8 part e4m3(clamp(y, +-448)) of its fp32 output
    (the cap 1e-4 of test_layernorm_f8_rows; these seeds hold no value near a rounding boundary), the pad columns keep their sentinel"""
    d, b = ec.build_ln_f8(c), Bufs()
    lp, f32 = _layernorm(built_lib, b, d, c.rows, c.D, c.eps, c.rms, H16, True, True)
    x, g, beta = b.op(d["x"], 2 * c.D * 4), b.op(d["gamma"]), b.op(d["beta"])
    rows = b.out(c.rows, 3 * c.D // 2, c.ld, H16)
    _lib.check(built_lib.f3r_layernorm_f8(P(x), P(g), P(beta), P(rows), c.ld, c.rows, c.D, float(c.eps), int(c.rms), ops.stream_ptr()), "f3r_layernorm_f8")
    b.intact(c.id)
    check("ln-f8-f32", f32.view, d["ref"], 2e-5, c.id)
    check("ln-f8-f16", rows.view[:, :c.D].float(), d["ref"], lp_tol(H16), c.id)
    assert torch.equal(bits(rows.view[:, :c.D]), bits(lp.view)), f"{c.id}: the fp16 part differs from f3r_layernorm"
    got8 = rows.view[:, c.D:].contiguous().view(torch.uint8).cpu()
    want8 = ec.e4m3(f32.view.cpu())
    assert got8.shape == want8.shape == (c.rows, c.D)
    share = float((got8 != want8).float().mean())
    print(f"[elem-geometry] kind=ln-f8-codes mismatch_share={share:.3e} cap=1.0e-04 {c.id}")
    assert not ((got8 & 0x7F) == 0x7F).any(), f"{c.id}: NaN codes"
    assert share < 1e-4
    if c.D > 40:
        assert int((got8[:, 40] & 0x7F).max()) == 0x7E     # 448: the clamp came before the conversion


@pytest.mark.parametrize("c", ec.LN_F8_REFUSED, **ID)
def test_layernorm_f8_refuses_rows_that_are_not_16_byte_multiples(built_lib, c):
    """D = 8, 1032, 2056: 3 D / 2 (+ 8) is not a multiple of 8, and the entry point says so before it launches anything"""
    x, g = torch.zeros((c.rows, c.D), device=DEV), torch.ones(c.D, device=DEV)
    rows = torch.zeros((c.rows, c.ld + 8), dtype=H16, device=DEV)
    with pytest.raises(ValueError, match="multiple of 8"):
        _lib.check(built_lib.f3r_layernorm_f8(P(x), P(g), None, P(rows), c.ld, c.rows, c.D, 1e-6, 0, ops.stream_ptr()), "f3r_layernorm_f8")


# ================================================================================================ bilinear
def _bilinear(lib, c, d, entry, want_f8=False):
    b = Bufs()
    margin = (c.w + 2) * c.C * 2
    x, x_lo = b.op(d["x"], margin), b.op(d["x_lo"], margin)
    npx = c.B * c.out[0] * c.out[1]
    out = b.out(npx, c.C, c.C, c.dtype)
    out_lo = b.out(npx, c.C, c.C, c.dtype, c.form != "plain")
    out_f8 = b.out(npx, c.C, c.C, H16, want_f8)       # [C e4m3 | C e4m3] per pixel = C 16-bit words
    sizes = (c.B, c.h, c.w, c.C)
    tail = (*c.out, ops.dtype_id(c.dtype), ops.stream_ptr())
    if entry == "x2":
        st = lib.f3r_upsample2x(P(x), P(x_lo), P(out), P(out_lo), *sizes, *tail)
    elif entry == "f8":
        st = lib.f3r_interp_bilinear_f8(P(x), P(x_lo), P(out), P(out_lo), P(out_f8), *sizes, *c.full, *tail)
    else:
        st = lib.f3r_interp_bilinear(P(x), P(x_lo), P(out), P(out_lo), *sizes, *c.full, *tail)
    _lib.check(st, "f3r_interp_bilinear")
    b.intact(f"{c.id} {entry}")
    return out, out_lo, out_f8


@pytest.mark.parametrize("c", ec.BIL, **ID)
def test_bilinear(built_lib, c):
    """one-row and one-column inputs, a nominal size of 1, downscaling, coordinates that land on integers, crops down to 1 x 1, one 16-byte item
    per pixel, planes in and out, the fp8 planes"""
    d = ec.build_bil(c)
    out, out_lo, out_f8 = _bilinear(built_lib, c, d, "f8" if c.form == "f8" else "general", want_f8=c.form == "f8")
    if c.form == "plain":
        check(f"bilinear-{dt_name(c.dtype)}", out.view.float(), d["ref"], lp_tol(c.dtype), c.id)
    else:
        check(f"bilinear-planes-{dt_name(c.dtype)}", out.view.double() + out_lo.view.double(), d["ref"], split_tol(c.dtype), c.id)
    if c.x2:     # f3r_upsample2x is the same launch with the nominal size 2 h x 2 w
        o2, o2_lo, _ = _bilinear(built_lib, c, d, "x2")
        assert torch.equal(bits(o2.view), bits(out.view)) and (out_lo is None or torch.equal(bits(o2_lo.view), bits(out_lo.view)))
    if c.form == "f8":
        plain, plain_lo, _ = _bilinear(built_lib, c, d, "general")
        assert torch.equal(bits(plain.view), bits(out.view)) and torch.equal(bits(plain_lo.view), bits(out_lo.view)), f"{c.id}: out_f8 changes the fp16 planes"
        p = out_f8.view.contiguous().view(torch.uint8).cpu()
        assert p.shape == (c.B * c.out[0] * c.out[1], 2 * c.C)
        dec = lambda t: t.contiguous().view(torch.float8_e4m3fn).double()
        hi8, lo8 = dec(p[:, :c.C]), dec(p[:, c.C:]) / 4096.0
        val = out.view.double().cpu() + out_lo.view.double().cpu()
        rest = out_lo.view.double().cpu()
        e_hi = float(((hi8 - val).abs() - (val.abs() * 2.0 ** -4 + 2.0 ** -10)).max())
        e_lo = float(((lo8 - rest).abs() - (rest.abs() * 2.0 ** -4 + 2.0 ** -22)).max())
        print(f"[elem-geometry] kind=bilinear-f8 excess_hi={e_hi:.3e} excess_lo={e_lo:.3e} {c.id}")
        assert e_hi <= 0.0 and e_lo <= 1e-9       # the bounds of test_interp_bilinear_f8_planes


def test_bilinear_f8_goes_with_fp16_only(built_lib):
    x = torch.zeros((1, 1, 1, 128), dtype=BF16, device=DEV)
    out, f8 = torch.zeros((1, 2, 2, 128), dtype=BF16, device=DEV), torch.zeros((1, 2, 2, 256), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="fp16"):
        _lib.check(built_lib.f3r_interp_bilinear_f8(P(x), None, P(out), None, P(f8), 1, 1, 1, 128, 2, 2, 2, 2, ops.dtype_id(BF16), ops.stream_ptr()), "f3r_interp_bilinear_f8")


# ================================================================================================ head tail
@pytest.mark.parametrize("c", ec.DPT, **ID)
def test_dpt_final(built_lib, c):
    """Cin == 128 (LDS-DMA staged, the ragged last group clamped to the last pixel) at 1 / 63 / 64 / 65 / 129 pixels with and without the low plane;
    the one-pixel-per-lane kernel at its smallest and largest width; a 3-row weight inside NaN; the d == 0 pixel; a saturated sigmoid"""
    d, b = ec.build_dpt(c), Bufs()
    margin = 2 * c.Cin * 2
    x, x_lo, w, bias = b.op(d["x"], margin), b.op(d["x_lo"], margin), b.op(d["w"], margin), b.op(d["b"])
    pts, conf = b.out(c.npix, 3, 3, F32), b.out(c.npix, 1, 1, F32, c.n_out == 4)
    cmode, vmin, vmax = (ops.CONF_MODES[c.conf[0]], float(c.conf[1]), float(c.conf[2])) if c.n_out == 4 else (0, 1.0, float("inf"))
    _lib.check(built_lib.f3r_dpt_final(P(x), P(x_lo), P(w), P(bias), c.n_out, P(pts), P(conf), c.npix, c.Cin, ops.DEPTH_MODES[c.depth], cmode, vmin, vmax,
                                       ops.dtype_id(c.dtype), ops.stream_ptr()), "f3r_dpt_final")
    b.intact(c.id)
    kind = f"dpt{'128' if c.Cin == 128 else ''}-{dt_name(c.dtype)}"
    assert torch.isfinite(pts.view).all()
    check(f"{kind}-pts", pts.view, d["pts"], 1e-5, c.id)
    if conf is not None:
        assert torch.isfinite(conf.view).all()
        check(f"{kind}-conf", conf.view, d["conf"].reshape(-1, 1), 1e-5, c.id)
    if c.special == "zero":
        assert bool((pts.view[0] == 0).all()), f"{c.id}: the d == 0 pixel must be exactly 0, got {pts.view[0].tolist()}"
    if c.special == "saturate":
        z = d["xin"] @ d["w"][3].double() + d["b"][3].double()
        got = conf.view[:, 0].cpu()
        assert bool((got[z >= ec.SATURATED] == c.conf[2]).all()) and bool((got[z <= -ec.SATURATED] == c.conf[1]).all()), f"{c.id}: a saturated sigmoid is vmax / vmin"


# ================================================================================================ cast, patchify, SwiGLU gate, row add
@pytest.mark.parametrize("c", ec.CAST, **ID)
def test_cast(built_lib, c):
    d, b = ec.build_cast(c), Bufs()
    x = b.op(d["x"])
    hi, lo = b.out(1, c.n, c.n, c.dtype), b.out(1, c.n, c.n, c.dtype, c.lo)
    _lib.check(built_lib.f3r_cast_f32_to_lp(P(x), P(hi), P(lo), c.n, ops.dtype_id(c.dtype), ops.stream_ptr()), "f3r_cast_f32_to_lp")
    b.intact(c.id)
    assert torch.equal(bits(hi.view[0]), bits(d["hi"])), f"{c.id}: hi != x.to(dtype)"
    assert lo is None or torch.equal(bits(lo.view[0]), bits(d["lo"])), f"{c.id}: lo != (x - hi).to(dtype)"


@pytest.mark.parametrize("c", ec.PATCH, **ID)
def test_patchify(built_lib, c):
    """both sides of `ps % 8 == 0 && ld_out == K`: the 16-byte kernel at patch 8 / 16 / 24, the pair kernel at patch 4 and 14 and at patch 16 with a
    padded row; rows equal F.unfold bit for bit, pad columns exactly zero"""
    d, b = ec.build_patch(c), Bufs()
    img = b.op(d["img"], 2 * c.W * 4)
    out = b.out(c.patches, c.ld_eff, c.ld_eff, c.dtype)
    _lib.check(built_lib.f3r_patchify(P(img), P(out), c.B, c.H, c.W, c.ps, c.ld, ops.dtype_id(c.dtype), ops.stream_ptr()), "f3r_patchify")
    b.intact(c.id)
    assert torch.equal(bits(out.view[:, :c.K]), bits(d["ref"])), f"{c.id}: rows differ from F.unfold"
    assert c.ld_eff == c.K or bool((bits(out.view[:, c.K:]) == 0).all()), f"{c.id}: pad columns must be zero"


@pytest.mark.parametrize("c", ec.SILU, **ID)
def test_silu_mul(built_lib, c):
    d, b = ec.build_silu(c), Bufs()
    ab = b.op(d["ab"], 2 * 2 * c.hidden * 2)
    out = b.out(c.rows, c.hidden, c.hidden, c.dtype)
    _lib.check(built_lib.f3r_silu_mul(P(ab), P(out), c.rows, c.hidden, ops.dtype_id(c.dtype), ops.stream_ptr()), "f3r_silu_mul")
    b.intact(c.id)
    assert torch.isfinite(out.view.float()).all()
    check(f"silu-{dt_name(c.dtype)}", out.view.float(), d["ref"], lp_tol(c.dtype), c.id)


@pytest.mark.parametrize("c", ec.ROWS_ADD, **ID)
def test_rows_add(built_lib, c):
    d, b = ec.build_rows_add(c), Bufs()
    x = b.out(c.total, c.D, c.D, F32)
    x.view.copy_(d["x"])
    vec = b.op(d["vec"])
    _lib.check(built_lib.f3r_rows_add_f32(P(x), P(vec), c.rows, c.D, ops.stream_ptr()), "f3r_rows_add_f32")
    b.intact(c.id)
    assert torch.equal(bits(x.view), bits(d["ref"])), f"{c.id}: touched rows must be x + vec bit for bit, the others unchanged"


# ================================================================================================ fp32 attention
def _attention(lib, c, d):
    b = Bufs()
    D, Dkv = c.H * c.HD, c.Hkv * c.HD
    T = c.n_seq * c.tq
    a = _lib.AttnF32Args()
    if c.entry == "plain":
        assert c.tq == c.tk and c.kv_group == 1 and not c.causal
        qkv = b.rows(torch.cat([d["q"], d["k"], d["v"]], dim=1), 3 * D + c.pad)
        ld = qkv.stride(0)
    else:
        q, k, v = b.rows(d["q"], D + c.pad), b.rows(d["k"], Dkv + c.pad), b.rows(d["v"], Dkv + c.pad)
        a.q, a.k, a.v, a.ldq, a.ldkv = P(q), P(k), P(v), D + c.pad, Dkv + c.pad
        assert q.stride(0) == a.ldq and k.stride(0) == v.stride(0) == a.ldkv
    ldo = D + c.pad
    o32 = b.out(T, D, ldo, F32, c.outs in ("f32", "all"))
    hi = b.out(T, D, ldo, c.dtype, c.outs in ("hi", "all"))
    lo = b.out(T, D, ldo, c.dtype, c.outs == "all")
    if c.entry == "plain":
        base = qkv.data_ptr()
        st = lib.f3r_attn_f32(base, base + D * 4, base + 2 * D * 4, ld, P(hi), P(lo), P(o32), ldo, c.n_seq, c.tq, c.H, float(c.scale), ops.dtype_id(c.dtype), c.HD,
                              ops.stream_ptr())
    else:
        a.o_hi, a.o_lo, a.o_f32, a.ldo = P(hi), P(lo), P(o32), ldo
        a.n_seq, a.tq, a.tk, a.q_pos0, a.k_pos0 = c.n_seq, c.tq, c.tk, c.q_pos0, c.k_pos0
        a.n_heads, a.kv_group, a.causal, a.dtype, a.head_dim, a.scale = c.H, c.kv_group, int(c.causal), ops.dtype_id(c.dtype), c.HD, float(c.scale)
        st = lib.f3r_attn_f32_ex(ctypes.byref(a), ops.stream_ptr())
    _lib.check(st, "f3r_attn_f32")
    b.intact(c.id)
    return o32, hi, lo


@pytest.mark.parametrize("c", ec.ATTN, **ID)
def test_attn_f32(built_lib, c):
    """every head width; 1 / 255 / 256 / 257 queries (the workgroup edge) and 1 / 31 / 32 / 33 keys (the tile edge); three sequences whose workgroup
    edges lie inside them; row strides wider than the rows; each output form; causal masks on absolute positions with k_pos0 != 0, where a row
    -- or a whole workgroup -- without a visible key gives exact zeros"""
    assert c.tk < ops.ATTN_F32_MFMA_MIN_KEYS
    d = ec.build_attn(c)
    o32, hi, lo = _attention(built_lib, c, d)
    kind = f"attn-hd{c.HD}"
    if o32 is not None:
        check(f"{kind}-f32", o32.view, d["ref"], ec.attn_tol(c, "f32"), c.id)
    if lo is not None:
        check(f"{kind}-planes-{dt_name(c.dtype)}", hi.view.double() + lo.view.double(), d["ref"], ec.attn_tol(c, "planes"), c.id)
    elif hi is not None:
        check(f"{kind}-hi-{dt_name(c.dtype)}", hi.view.float(), d["ref"], ec.attn_tol(c, "hi"), c.id)
    dark = d["no_key"].repeat(c.n_seq).to(DEV)
    if bool(dark.any()):
        for name, g in (("o_f32", o32), ("o_hi", hi), ("o_lo", lo)):
            assert g is None or bool((g.view[dark] == 0).all()), f"{c.id}: a row without a visible key must be zeros in {name}"


# ================================================================================================ fp32 rotary embedding and gate
@pytest.mark.parametrize("c", ec.ROPE, **ID)
def test_rope_f32(built_lib, c):
    """RoPE-2D on one token and on a 3 x 5 grid x 2 sequences with a padded row stride; the per-view form with one row per group and with a partial
    last group; the columns behind the rotated heads come out bit-unchanged, the gap columns keep their sentinel"""
    d, b = ec.build_rope(c), Bufs()
    buf = b.out(c.rows, c.width, c.width + c.pad, F32)
    buf.view.copy_(d["x"])
    cos, sin = b.op(d["cos"]), b.op(d["sin"])
    _lib.check(built_lib.f3r_rope_f32(P(buf), c.rows, c.width + c.pad, c.n_rot, c.seq_len, c.rope_w, c.mode, P(cos), P(sin), ops.stream_ptr()), "f3r_rope_f32")
    b.intact(c.id)
    n = c.n_rot * 64
    check(f"rope-mode{c.mode}", buf.view[:, :n], d["ref"][:, :n], 2e-6, c.id)
    assert torch.equal(bits(buf.view[:, n:]), bits(d["x"][:, n:])), f"{c.id}: columns behind the rotated heads changed"


@pytest.mark.parametrize("c", ec.SILU_F32, **ID)
def test_silu_mul_f32(built_lib, c):
    d, b = ec.build_silu(c, f32=True), Bufs()
    ab = b.op(d["ab"], 2 * 2 * c.hidden * 4)
    hi, lo = b.out(c.rows, c.hidden, c.hidden, c.dtype), b.out(c.rows, c.hidden, c.hidden, c.dtype)
    _lib.check(built_lib.f3r_silu_mul_f32(P(ab), P(hi), P(lo), c.rows, c.hidden, ops.dtype_id(c.dtype), ops.stream_ptr()), "f3r_silu_mul_f32")
    b.intact(c.id)
    check(f"silu-f32-planes-{dt_name(c.dtype)}", hi.view.double() + lo.view.double(), d["ref"], 3e-6 if c.dtype == H16 else 3e-5, c.id)
