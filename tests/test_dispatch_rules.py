"""Every refusal rule of f3r_gemm and f3r_attn_fwd, one argument block each: a block the library accepts with exactly one thing broken, the status it
must return and a distinctive part of f3r_last_error_string().  No GPU: a refusal returns before any launch, and the accepted blocks are called
with M = 0 / tq = 0 only.  A rule that the F3R_SPLIT_W2F8 launches share with the other splits appears twice, once per split ("w2f8 ..." rows): the
two must keep the same status, and the part of the message named here."""
import ctypes

import pytest

import gemm_cases as gc
from conv_cases import ConvCase
from gemm_cases import BF16, H16, ConvTCase, GemmCase, QkvCase
from fast3r_amd import _lib, ops

ARG, UNSUPPORTED = -1, -2
AT = 0x10000            # a 16-byte aligned stand-in address (argument checks read no memory)


# ------------------------------------------------------------------------------------------------ f3r_gemm: the blocks the rules are broken in
def _gemm(role="f32", split=None, dt=H16, sel=1):
    return lambda: gc.stand_in_args(GemmCase(512, 256, 256, role, split, dt, 70 if role == "rowadd" else 0), sel, M=0)


def _qkv(rope=True, sel=1):
    return lambda: gc.stand_in_args(QkvCase(2, 256, 256, 256, 256, H16, (16, 16) if rope else None), sel, M=0)


def _convt():
    return gc.stand_in_args(ConvTCase(2, 5, 7, 64, 32, 2), 1, M=0)


def _conv(split=None, fin=False, Ci=128, Co=128, sel=0):
    """the f3r_gemm_args of a 3x3 convolution (what ops.conv3x3 builds), M = 0"""
    def make():
        c = ConvCase(2, 8, 8, Ci, Co, 1, split)
        g = _lib.GemmArgs()
        planes = 1 if split is None else 2
        g.A = g.W = g.out_lp = g.bias = AT
        g.M, g.N, g.Kpad = 0, c.Co, planes * 9 * ((c.Ci + 63) // 64) * 64
        g.a_mode, g.conv_H, g.conv_W, g.conv_C, g.conv_stride, g.conv_OH, g.conv_OW = _lib.F3R_A_CONV3X3, c.H, c.W, c.Ci, 1, 8, 8
        g.epi, g.dtype, g.split, g.ldo_lp, g.kernel_sel = _lib.F3R_EPI_GENERIC, _lib.F3R_F16, ops.SPLIT[split], c.Co, sel
        if split is not None:
            g.A_lo = AT
        if split == "x3f8":
            g.w_scale = AT
        if fin:
            g.fin_w = g.fin_b = g.fin_pts = AT
            g.fin_n_out, g.out_lp = 3, None
        return g
    return make


def _w2f8(role="gelu"):
    """rows [K fp16 | K fp8] on both operands, the generic epilogue (gemm_cases.STRIDE_F8 without its gaps)"""
    return lambda: gc.stand_in_args(GemmCase(512, 256, 256, role, "w2f8", H16, f8_rows=role == "gelu"), 0, M=0)


def _w2f8_qkv(rope=True):
    def make():
        g = _qkv(rope, 0)()
        g.split, g.Kpad, g.lda = _lib.F3R_SPLIT_W2F8, g.K, 3 * g.K // 2
        g.w_scale = g.W_aux = AT
        return g
    return make


def _f8_outputs():
    g = _gemm("gelu")()
    g.out_f8 = g.out_relu_f8 = AT
    return g


def _set(**kw):
    def f(g):
        for k, v in kw.items():
            setattr(g, k, v)
    return f


# (id, block, what breaks, status, part of the message)
GEMM_RULES = [
    ("null operand", _gemm(), _set(A=None), ARG, "null operand"),
    ("null weight", _gemm(), _set(W=None), ARG, "null operand"),
    ("negative M", _gemm(), _set(M=-1), ARG, "bad M/N"),
    ("N zero", _gemm(), _set(N=0), ARG, "bad M/N"),
    ("split out of range", _gemm(), _set(split=5), ARG, "bad split 5"),
    ("split negative", _gemm(), _set(split=-1), ARG, "bad split -1"),
    ("fp8 planes beside QKV", _qkv(), _set(out_f8=AT), ARG, "need the generic epilogue"),
    ("fused tail beside ConvT", _convt, _set(fin_w=AT), ARG, "need the generic epilogue"),
    ("Kpad not a multiple of 64", _gemm(), _set(Kpad=264), ARG, "Kpad 264 must be a positive multiple of 64"),
    ("Kpad of two planes", _gemm(split="w2"), _set(Kpad=576), ARG, "Kpad 576 must be a positive multiple of 128"),
    ("x3 without A_lo", _gemm("both", "x3"), _set(A_lo=None), ARG, "needs A_lo"),
    ("x3 with a_relu", _gemm("both", "x3"), _set(a_relu=1), ARG, "needs A_lo"),
    ("x3f8 without w_scale", _conv("x3f8"), _set(w_scale=None), ARG, "X3F8 needs a 3x3 convolution"),
    ("x3f8 in bf16", _conv("x3f8"), _set(dtype=_lib.F3R_BF16), ARG, "X3F8 needs a 3x3 convolution"),
    ("kernel_sel 8", _gemm(), _set(kernel_sel=8), ARG, "bad kernel_sel 8"),
    ("kernel_sel 12", _gemm(), _set(kernel_sel=12), ARG, "bad kernel_sel 12"),
    ("kernel_sel negative", _gemm(), _set(kernel_sel=-1), ARG, "bad kernel_sel -1"),
    ("w2f8 kernel_sel 8", _w2f8(), _set(kernel_sel=8), ARG, "bad kernel_sel 8"),
    ("w2f8 kernel_sel 16", _w2f8(), _set(kernel_sel=16), ARG, "bad kernel_sel 16"),
    ("N not a multiple of 4", _gemm(), _set(N=254), ARG, "N 254 must be a multiple of 4"),
    ("w2f8 N not a multiple of 4", _w2f8(), _set(N=254), ARG, "N 254 must be a multiple of 4"),
    ("A misaligned", _gemm(), _set(A=AT + 8), ARG, "A/W must be 16-byte aligned"),
    ("W misaligned", _gemm(), _set(W=AT + 8), ARG, "A/W must be 16-byte aligned"),
    ("dtype", _gemm(), _set(dtype=2), ARG, "bad dtype 2"),
    ("K not a multiple of 8", _gemm(), _set(K=252), ARG, "K 252 must be a multiple of 8"),
    ("K beyond Kpad", _gemm(), _set(K=264, lda=264), ARG, "K 264 must be a multiple of 8 and <= Kpad"),
    ("lda below K", _gemm(), _set(lda=248), ARG, "lda 248 must be a multiple of 8 and >= K"),
    ("lda not a multiple of 8", _gemm(), _set(lda=260), ARG, "lda 260 must be a multiple of 8"),
    ("conv_C", _conv(), _set(conv_C=132), ARG, "conv_C 132 must be a multiple of 8"),
    ("conv Kpad", _conv(), _set(Kpad=1152 + 64), ARG, "conv Kpad 1216 != 9*roundup(C,64)"),
    ("conv with ConvT epilogue", _conv(), _set(epi=_lib.F3R_EPI_CONVT), ARG, "conv3x3 supports only the generic epilogue"),
    ("conv stride", _conv(), _set(conv_stride=3), ARG, "conv stride 3"),
    ("conv output dims", _conv(), _set(conv_OH=7), ARG, "conv output dims inconsistent"),
    ("conv M", _conv(), _set(M=65), ARG, "conv M not a multiple of OH*OW"),
    ("a_mode", _gemm(), _set(a_mode=2), ARG, "bad a_mode 2"),
    ("no output", _gemm(), _set(out_f32=None), ARG, "no output"),
    ("w2f8 no output", _w2f8(), _set(out_lp=None), ARG, "no output"),
    ("out_f32 misaligned", _gemm(), _set(out_f32=AT + 8), ARG, "out_f32 alignment/ld"),
    ("out_f32 stride below N", _gemm(), _set(ldo_f32=252), ARG, "out_f32 alignment/ld"),
    ("w2f8 out_f32 misaligned", _w2f8("f32"), _set(out_f32=AT + 8), ARG, "out_f32 alignment/ld"),
    ("w2f8 out_f32 stride below N", _w2f8("f32"), _set(ldo_f32=252), ARG, "out_f32 alignment/ld"),
    ("out_lp misaligned", _gemm("gelu"), _set(out_lp=AT + 4), ARG, "out_lp alignment/ld"),
    ("out_lp stride below N", _gemm("gelu"), _set(ldo_lp=252), ARG, "out_lp alignment/ld"),
    ("w2f8 out_lp misaligned", _w2f8(), _set(out_lp=AT + 8), ARG, "out_lp alignment/ld"),
    ("w2f8 out_lp stride", _w2f8(), _set(ldo_lp=388), ARG, "out_lp alignment/ld"),
    ("w2f8 out_lp stride below N", _w2f8(), _set(ldo_lp=248, out_lp_f8=0), ARG, "out_lp alignment/ld"),
    ("fp8 planes in bf16", _f8_outputs, _set(dtype=_lib.F3R_BF16), ARG, "out_f8 / out_relu_f8 need fp16"),
    ("fp8 planes beside out_lp_f8", _f8_outputs, _set(out_lp_f8=1), ARG, "out_f8 / out_relu_f8 need fp16"),
    ("fp8 plane alone", _f8_outputs, _set(out_relu_f8=AT + 4), ARG, "out_f8 / out_relu_f8 need fp16"),
    ("fused tail without fin_b", _conv(fin=True), _set(fin_b=None), ARG, "fin_w needs fin_b"),
    ("fused tail fin_n_out", _conv(fin=True), _set(fin_n_out=5), ARG, "fin_w needs fin_b"),
    ("fused tail confidence of 3 channels", _conv(fin=True), _set(fin_conf=AT), ARG, "fin_w needs fin_b"),
    ("fused tail depth mode", _conv(fin=True), _set(fin_depth_mode=3), ARG, "bad fin_depth_mode / fin_conf_mode"),
    ("fused tail conf mode", _conv(fin=True), _set(fin_conf_mode=2), ARG, "bad fin_depth_mode / fin_conf_mode"),
    ("fused tail with a second output", _conv(fin=True), _set(out_relu=AT), ARG, "the fused head tail writes fin_pts / fin_conf only"),
    ("res_f32 misaligned", _gemm("resf32"), _set(res_f32=AT + 8), ARG, "res_f32 alignment/ld"),
    ("res_f32 stride", _gemm("resf32"), _set(ldr_f32=258), ARG, "res_f32 alignment/ld"),
    ("w2f8 res_f32 misaligned", _w2f8("resf32"), _set(res_f32=AT + 8), ARG, "res_f32 alignment/ld"),
    ("w2f8 res_f32 stride", _w2f8("resf32"), _set(ldr_f32=258), ARG, "res_f32 alignment/ld"),
    ("w2f8 res_f32 stride below N", _w2f8("resf32"), _set(ldr_f32=252), ARG, "res_f32 alignment/ld"),
    ("res_lp misaligned", _gemm("relu2res"), _set(res_lp=AT + 4), ARG, "res_lp alignment/ld"),
    ("res_lp2 stride", _gemm("relu2res"), _set(ldr_lp2=258), ARG, "res_lp2 alignment/ld"),
    ("low residual plane alone", _gemm("gelu"), _set(res_lp_lo=AT), ARG, "low residual planes need their high planes"),
    ("second low residual plane alone", _gemm("gelu"), _set(res_lp2_lo=AT), ARG, "low residual planes need their high planes"),
    ("out_lp_lo alone", _gemm(), _set(out_lp_lo=AT), ARG, "out_lp_lo / out_relu alignment"),
    ("out_relu misaligned", _gemm("gelu"), _set(out_relu=AT + 4), ARG, "out_lp_lo / out_relu alignment"),
    ("out_relu_lo alone", _gemm("gelu"), _set(out_relu_lo=AT), ARG, "out_lp_lo / out_relu alignment"),
    ("rowadd_div", _gemm("rowadd"), _set(rowadd_div=0), ARG, "rowadd alignment/div"),
    ("rowadd misaligned", _gemm("rowadd"), _set(rowadd=AT + 8), ARG, "rowadd alignment/div"),
    ("row stride 2^26", _gemm(), _set(ldo_f32=1 << 26), ARG, "row strides must be < 2^26 elements"),
    ("negative residual stride", _gemm("resf32"), _set(ldr_f32=-4), ARG, "row strides must be < 2^26 elements"),
    ("bias misaligned", _gemm(), _set(bias=AT + 8), ARG, "bias alignment"),
    ("w2f8 bias misaligned", _w2f8(), _set(bias=AT + 8), ARG, "bias"),
    ("QKV thirds", _qkv(), _set(N=772), ARG, "QKV with three equal parts needs N % 3 == 0 (got 772)"),
    ("w2f8 QKV thirds", _w2f8_qkv(), _set(N=772), ARG, "QKV with three equal parts needs N % 3 == 0 (got 772)"),
    ("QKV heads", _qkv(), _set(qkv_dq=288), ARG, "QKV parts must be whole 64-wide heads (N 768, q 288)"),
    ("w2f8 QKV heads", _w2f8_qkv(), _set(qkv_dq=288), ARG, "QKV parts must be whole 64-wide heads (N 768, q 288)"),
    ("QKV without q", _qkv(), _set(q=None), ARG, "QKV outputs null/misaligned"),
    ("QKV vt misaligned", _qkv(), _set(vt=AT + 4), ARG, "QKV outputs null/misaligned"),
    ("w2f8 QKV without q", _w2f8_qkv(), _set(q=None), ARG, "QKV"),
    ("w2f8 QKV without vt", _w2f8_qkv(), _set(vt=None), ARG, "QKV"),
    ("QKV seq_len", _qkv(), _set(seq_len=0), ARG, "QKV seq_len/ldvt"),
    ("QKV seq_len does not divide M", _qkv(), _set(M=300), ARG, "QKV seq_len/ldvt"),
    ("QKV ldvt", _qkv(), _set(ldvt=248), ARG, "QKV seq_len/ldvt"),
    ("w2f8 QKV seq_len", _w2f8_qkv(), _set(seq_len=0), ARG, "seq_len"),
    ("w2f8 QKV seq_len does not divide M", _w2f8_qkv(), _set(M=300), ARG, "seq_len"),
    ("w2f8 QKV ldvt", _w2f8_qkv(), _set(ldvt=248), ARG, "seq_len"),
    ("QKV activation", _qkv(), _set(act=_lib.F3R_ACT_GELU), ARG, "QKV has no activation"),
    ("w2f8 QKV activation", _w2f8_qkv(), _set(act=_lib.F3R_ACT_GELU), ARG, "no activation"),
    ("QKV bias", _qkv(), _set(bias=AT + 8), ARG, "bias alignment"),
    ("w2f8 QKV bias", _w2f8_qkv(), _set(bias=AT + 8), ARG, "bias"),
    ("QKV RoPE tables", _qkv(), _set(rope_sin=None), ARG, "RoPE tables"),
    ("QKV RoPE width", _qkv(), _set(rope_w=0), ARG, "RoPE tables"),
    ("w2f8 QKV RoPE tables", _w2f8_qkv(), _set(rope_sin=None), ARG, "RoPE tables"),
    ("w2f8 QKV RoPE width", _w2f8_qkv(), _set(rope_w=0), ARG, "RoPE tables"),
    ("ConvT without out_lp", _convt, _set(out_lp=None), ARG, "CONVT needs out_lp"),
    ("ConvT N", _convt, _set(ct_cout=28), ARG, "CONVT N != s*s*cout"),
    ("ConvT grid", _convt, _set(ct_h=0), ARG, "CONVT M not a multiple of h*w"),
    ("ConvT M", _convt, _set(M=36), ARG, "CONVT M not a multiple of h*w"),
    ("ConvT bias", _convt, _set(bias=AT + 8), ARG, "bias alignment"),
    # ---- what W2F8 alone asks
    ("w2f8 A misaligned", _w2f8(), _set(A=AT + 8), ARG, "W2F8 needs 16-byte aligned A / W and w_scale"),
    ("w2f8 without w_scale", _w2f8(), _set(w_scale=None), ARG, "W2F8 needs 16-byte aligned A / W and w_scale"),
    ("w2f8 w_scale misaligned", _w2f8(), _set(w_scale=AT + 2), ARG, "W2F8 needs 16-byte aligned A / W and w_scale"),
    ("w2f8 K", _w2f8(), _set(K=192, Kpad=192), ARG, "W2F8 needs K = Kpad, a multiple of 128 (got 192 / 192)"),
    ("w2f8 Kpad", _w2f8(), _set(Kpad=512), ARG, "W2F8 needs K = Kpad, a multiple of 128 (got 256 / 512)"),
    ("w2f8 rows", _w2f8(), _set(lda=376), ARG, "W2F8 rows are [K fp16 | K fp8]: lda 376 must be >= 3 K / 2"),
    ("w2f8 second output", _w2f8(), _set(out_f8=AT), ARG, "W2F8 launches write one output"),
    ("w2f8 fused tail", _w2f8(), _set(fin_w=AT), ARG, "W2F8 launches write one output"),
    ("w2f8 bf16", _w2f8(), _set(dtype=_lib.F3R_BF16), ARG, "W2F8 corrects fp16 planes only (dtype 1)"),
    ("w2f8 act", _w2f8(), _set(act=3), ARG, "bad act 3"),
    ("w2f8 QKV without W_aux", _w2f8_qkv(), _set(W_aux=None), ARG, "W_aux"),
    ("w2f8 QKV W_aux misaligned", _w2f8_qkv(), _set(W_aux=AT + 8), ARG, "W_aux"),
    # ---- refused at selection
    ("lab form in a product build", _gemm(dt=BF16), _set(kernel_sel=16), ARG, "kernel_sel 16 is not available in this build"),
    ("x3f8 over the K-tile table", _conv("x3f8", Ci=1920), _set(), UNSUPPORTED, "split X3F8 / fin_w but the launch is not eligible for the 256-tile kernel"),
    ("x3f8 ragged channels", _conv("x3f8"), _set(N=192, ldo_lp=192), UNSUPPORTED, "split X3F8 / fin_w but the launch is not eligible for the 256-tile kernel"),
    ("fused tail of 256 channels", _conv(fin=True, Co=256), _set(), UNSUPPORTED, "split X3F8 / fin_w but the launch is not eligible for the 256-tile kernel"),
    ("kernel_sel 6 without rows", _gemm(sel=6), _set(), UNSUPPORTED, "kernel_sel 6 (hand-scheduled kernel) but the launch is not eligible: M or N not a multiple of 256"),
    ("kernel_sel 9 without rows", _gemm(sel=9), _set(), UNSUPPORTED, "kernel_sel 6 (hand-scheduled kernel) but the launch is not eligible: M or N not a multiple of 256"),
    ("kernel_sel 6 on two outputs", _gemm("both", sel=6), _set(M=512), UNSUPPORTED, "but the launch is not eligible: both an fp32 and a lowp output"),
    ("kernel_sel 6 on a convolution", _conv(sel=6), _set(), UNSUPPORTED, "but the launch is not eligible: not a plain GEMM operand (convolution)"),
    ("kernel_sel 6 on ConvT", _convt, _set(kernel_sel=6), UNSUPPORTED, "but the launch is not eligible: QKV / ConvT epilogue"),
    ("kernel_sel 6 on grouped QKV", _qkv(sel=6), _set(M=512, qkv_dq=384), UNSUPPORTED, "but the launch is not eligible: grouped-query widths (q and k segments differ)"),
    ("kernel_sel 6 on QKV without rows", _qkv(sel=6), _set(), UNSUPPORTED, "but the launch is not eligible: D, M or seq_len not a multiple of 256"),
    ("kernel_sel 2 on a ragged N", _gemm(sel=2), _set(N=132, ldo_f32=132), ARG, "kernel_sel 2 but the shape is not eligible for the 256-tile kernel"),
    ("kernel_sel 4 on a K tail", _gemm(sel=4), _set(K=248), ARG, "kernel_sel 4 but the shape is not eligible for the 256-tile kernel"),
    ("kernel_sel 5 on lowp residuals", _gemm("relu2res"), _set(kernel_sel=5), ARG, "kernel_sel 5 but the shape is not eligible for the 256-tile kernel"),
    ("w2f8 without rows", _w2f8(), _set(), UNSUPPORTED, "split W2F8 (fp8 low plane) but the launch is not eligible for the hand-scheduled kernel: M or N not a multiple of 256"),
    ("w2f8 with a lowp residual", _w2f8(), _set(M=512, res_lp=AT, ldr_lp=256), UNSUPPORTED,
     "but the launch is not eligible for the hand-scheduled kernel: additive rows / lowp residuals / second outputs / A_lo"),
    ("w2f8 on a convolution", _w2f8(), _set(M=512, a_mode=_lib.F3R_A_CONV3X3), UNSUPPORTED, "not a plain GEMM with the generic epilogue"),
    ("w2f8 on ConvT", _w2f8(), _set(M=512, epi=_lib.F3R_EPI_CONVT), UNSUPPORTED, "not a plain GEMM with the generic epilogue"),
    ("w2f8 QKV without rows", _w2f8_qkv(), _set(), UNSUPPORTED, "split W2F8 QKV but the launch is not eligible for the hand-scheduled kernel: D, M or seq_len not a multiple of 256"),
    ("w2f8 QKV outputs at 8 bytes", _w2f8_qkv(), _set(M=512, k=AT + 8), UNSUPPORTED, "split W2F8 QKV but the launch is not eligible for the hand-scheduled kernel: outputs not 16-byte aligned"),
    ("unknown epilogue on the 128-tile kernel", _gemm(), _set(epi=3), ARG, "bad epi 3"),
]

# accepted with M = 0: every rule met, nothing to launch
GEMM_ACCEPTED = [
    ("f32", _gemm()), ("f32 by shape", _gemm(sel=0)), ("f32 automatic without the hand-scheduled kernel", _gemm(sel=7)), ("gelu 256-tile", _gemm("gelu", sel=2)),
    ("w2", _gemm(split="w2")), ("x3 both", _gemm("both", "x3", BF16)), ("relu2res", _gemm("relu2res")), ("rowadd", _gemm("rowadd", sel=3)), ("resf32 256 x 128", _gemm("resf32", sel=4)),
    ("qkv", _qkv()), ("qkv without rope by shape", _qkv(False, 0)), ("qkv one tile per workgroup", _qkv(sel=5)), ("convt", _convt), ("conv", _conv()), ("conv x3", _conv("x3", sel=1)),
    ("conv x3f8", _conv("x3f8")), ("conv fused tail", _conv(fin=True)), ("conv x3f8 fused tail", _conv("x3f8", fin=True)), ("conv x3f8 merged schedule", _conv("x3f8", fin=True, sel=5)),
    ("fp8 planes", _f8_outputs),
]


def _last_error(lib):
    return lib.f3r_last_error_string().decode()


@pytest.mark.parametrize("block,breaks,status,text", [r[1:] for r in GEMM_RULES], ids=[r[0] for r in GEMM_RULES])
def test_f3r_gemm_refuses(built_lib, block, breaks, status, text):
    g = block()
    breaks(g)
    assert built_lib.f3r_gemm(ctypes.byref(g), None) == status, _last_error(built_lib)
    assert text in _last_error(built_lib)


@pytest.mark.parametrize("block", [b[1] for b in GEMM_ACCEPTED], ids=[b[0] for b in GEMM_ACCEPTED])
def test_f3r_gemm_accepts_the_unbroken_blocks(built_lib, block):
    g = block()
    assert g.M == 0
    assert built_lib.f3r_gemm(ctypes.byref(g), None) == 0, _last_error(built_lib)


def test_every_block_of_the_table_is_accepted_before_it_is_broken(built_lib):
    """(a row whose block were refused for another reason would prove nothing about its rule); the selection rows' blocks are whole launches that
    only lack rows, or a form: their refusal is the row itself"""
    for name, block, breaks, status, text in GEMM_RULES:
        g = block()
        rc = built_lib.f3r_gemm(ctypes.byref(g), None)
        assert g.M == 0 and (rc == 0 or (rc == UNSUPPORTED and "not eligible" in _last_error(built_lib))), (name, _last_error(built_lib))
    for name, block, breaks, status, text in ATTN_RULES:
        a = block()
        assert a.tq == 0 and built_lib.f3r_attn_fwd(ctypes.byref(a), None) == 0, (name, _last_error(built_lib))


def test_null_argument_blocks(built_lib):
    assert built_lib.f3r_gemm(None, None) == ARG and "f3r_gemm: null args" in _last_error(built_lib)
    assert built_lib.f3r_attn_fwd(None, None) == ARG and "f3r_attn_fwd: null args" in _last_error(built_lib)


# ------------------------------------------------------------------------------------------------ f3r_attn_fwd
def _attn(heads=2, hd=64, planes=1, sel=1, keys=128, segs=1):
    """one launch of `heads` heads over `segs` segments of `keys` keys, tq = 0"""
    def make():
        a = _lib.AttnArgs()
        a.q = a.o = AT
        a.ldq, a.ldo = heads * hd * (2 if planes >= 2 else 1), heads * hd
        a.tq, a.batch, a.n_heads, a.n_seg, a.dtype = 0, 1, heads, segs, _lib.F3R_F16
        for s in range(segs):
            a.k_seg[s] = a.vt_seg[s] = AT
            a.seg_len[s], a.ldvt[s], a.seg_pos0[s] = keys, ops.vt_ld(keys), s * keys
        a.ldk, a.q_prescaled, a.kernel_sel, a.head_dim, a.qk_planes = a.ldq, 1, sel, hd, planes
        return a
    return make


def _seg(field, s, v):
    def f(a):
        getattr(a, field)[s] = v
    return f


def _both(*fs):
    def f(a):
        for x in fs:
            x(a)
    return f


ATTN_RULES = [
    ("null q", _attn(), _set(q=None), ARG, "null q/o"),
    ("null o", _attn(), _set(o=None), ARG, "null q/o"),
    ("dtype", _attn(), _set(dtype=2), ARG, "bad dtype 2"),
    ("no heads", _attn(), _set(n_heads=0), ARG, "bad sizes"),
    ("no batch", _attn(), _set(batch=0), ARG, "bad sizes"),
    ("negative tq", _attn(), _set(tq=-1), ARG, "bad sizes"),
    ("no segments", _attn(), _set(n_seg=0), ARG, "n_seg 0 out of range"),
    ("too many segments", _attn(), _set(n_seg=9), ARG, "n_seg 9 out of range"),
    ("head_dim not a multiple of 16", _attn(), _set(head_dim=24), ARG, "head_dim 24 (a multiple of 16 up to 128)"),
    ("head_dim above 128", _attn(), _set(head_dim=144), ARG, "head_dim 144 (a multiple of 16 up to 128)"),
    ("ldq not a multiple of 8", _attn(), _set(ldq=132), ARG, "ldq/ldk must be multiples of 8, ldo of 4"),
    ("ldk not a multiple of 8", _attn(), _set(ldk=132), ARG, "ldq/ldk must be multiples of 8, ldo of 4"),
    ("ldo not a multiple of 4", _attn(), _set(ldo=130), ARG, "ldq/ldk must be multiples of 8, ldo of 4"),
    ("qk_planes", _attn(), _set(qk_planes=4), ARG, "qk_planes 4"),
    ("reserve_cus", _attn(), _set(reserve_cus=-1), ARG, "reserve_cus -1"),
    ("ldq below the heads", _attn(), _set(ldq=120), ARG, "row strides < heads*head_dim"),
    ("ldq below the planes", _attn(planes=2, sel=0), _set(ldq=128), ARG, "row strides < heads*head_dim"),
    ("ldo below the heads", _attn(), _set(ldo=124), ARG, "row strides < heads*head_dim"),
    ("q misaligned", _attn(), _set(q=AT + 8), ARG, "q/o alignment"),
    ("o misaligned", _attn(), _set(o=AT + 4), ARG, "q/o alignment"),
    ("q batch stride", _attn(), _set(q_batch_stride=4), ARG, "batch strides alignment"),
    ("o batch stride", _attn(), _set(o_batch_stride=2), ARG, "batch strides alignment"),
    ("negative segment", _attn(), _seg("seg_len", 0, -64), ARG, "negative segment length"),
    ("null K segment", _attn(segs=2), _seg("k_seg", 1, None), ARG, "null K/V^T segment 1"),
    ("null V^T segment", _attn(), _seg("vt_seg", 0, None), ARG, "null K/V^T segment 0"),
    ("K misaligned", _attn(), _seg("k_seg", 0, AT + 8), ARG, "K/V^T alignment"),
    ("ldvt not a multiple of 64", _attn(), _seg("ldvt", 0, 160), ARG, "ldvt[0]=160 must be a multiple of 64 covering the segment"),
    ("ldvt below the segment", _attn(segs=2), _seg("ldvt", 1, 64), ARG, "ldvt[1]=64 must be a multiple of 64 covering the segment"),
    ("K batch stride", _attn(), _seg("k_batch_stride", 0, 4), ARG, "K/V^T batch stride alignment"),
    ("V^T batch stride", _attn(), _seg("vt_batch_stride", 0, 4), ARG, "K/V^T batch stride alignment"),
    ("ldk beyond 32-bit tile offsets", _attn(), _set(ldk=1 << 25), ARG, "ldk / ldvt too large for 32-bit tile offsets"),
    ("ldvt beyond 32-bit tile offsets", _attn(), _seg("ldvt", 0, 1 << 25), ARG, "ldk / ldvt too large for 32-bit tile offsets"),
    ("no keys", _attn(), _seg("seg_len", 0, 0), ARG, "no keys"),
    ("causal launch that starts behind its queries", _attn(), _both(_set(causal=1, q_pos0=10), _seg("seg_pos0", 0, 11)), ARG,
     "causal launch without carried state whose first key (seg_pos0[0] = 11) lies after its first query (q_pos0 = 10)"),
    ("kv_group", _attn(), _set(kv_group=3), ARG, "kv_group 3 does not divide n_heads 2"),
    ("negative kv_group", _attn(), _set(kv_group=-1), ARG, "kv_group -1 does not divide n_heads 2"),
    ("ldk below the kv heads", _attn(), _set(ldk=120), ARG, "ldk < kv heads * head_dim"),
    ("state without buffers", _attn(), _set(state_out=1), ARG, "state buffers null/misaligned"),
    ("state misaligned", _attn(), _set(state_in=1, st_o=AT, st_ml=AT + 8), ARG, "state buffers null/misaligned"),
    ("kernel_sel 3", _attn(), _set(kernel_sel=3), ARG, "kernel_sel 3"),
    ("kernel_sel negative", _attn(), _set(kernel_sel=-1), ARG, "kernel_sel -1"),
    # ---- refused at selection (tq > 0; no kernel is launched)
    ("planes on the general kernel", _attn(planes=2, sel=0), _set(tq=128, kernel_sel=1), UNSUPPORTED,
     "qk_planes 2 / 3 but the launch is not eligible for the hand-scheduled three-product kernel: kernel_sel 1"),
    ("planes without a pre-scaled q", _attn(planes=3, sel=0), _set(tq=128, q_prescaled=0), UNSUPPORTED,
     "qk_planes 2 / 3 but the launch is not eligible for the hand-scheduled three-product kernel: q not pre-scaled"),
    ("planes at head_dim 128", _attn(hd=128, planes=2, sel=2), _set(tq=128), UNSUPPORTED, "three-product kernel: qk_planes 2 / 3 need head_dim 64 and fp16"),
    ("kernel_sel 2 with a causal mask", _attn(sel=2), _set(tq=128, causal=1), UNSUPPORTED, "kernel_sel 2 (hand-scheduled kernel) but the launch is not eligible: causal mask"),
    ("kernel_sel 2 below a wave's rows", _attn(sel=2), _set(tq=127), UNSUPPORTED,
     "kernel_sel 2 (hand-scheduled kernel) but the launch is not eligible: fewer query rows than one wave takes"),
    ("kernel_sel 2 at head_dim 96", _attn(hd=96, sel=2), _set(tq=128), UNSUPPORTED, "but the launch is not eligible: no generated kernel for this head_dim (64, 80, 128)"),
    ("kernel_sel 2 on ragged keys", _attn(sel=2, keys=100), _set(tq=128), UNSUPPORTED, "but the launch is not eligible: a K/V segment is not a multiple of 64 keys"),
]


@pytest.mark.parametrize("block,breaks,status,text", [r[1:] for r in ATTN_RULES], ids=[r[0] for r in ATTN_RULES])
def test_f3r_attn_fwd_refuses(built_lib, block, breaks, status, text):
    a = block()
    breaks(a)
    assert built_lib.f3r_attn_fwd(ctypes.byref(a), None) == status, _last_error(built_lib)
    assert text in _last_error(built_lib)


@pytest.mark.parametrize("block", [_attn(), _attn(sel=0), _attn(sel=2), _attn(4, 80, sel=0), _attn(4, 128, sel=2), _attn(2, 64, 2, 0), _attn(2, 64, 3, 2), _attn(3, 48, segs=8)],
                         ids=["hip", "auto", "asm", "d80", "d128", "qk3", "qk3f8", "generic"])
def test_f3r_attn_fwd_accepts_the_unbroken_blocks(built_lib, block):
    a = block()
    assert a.tq == 0
    assert built_lib.f3r_attn_fwd(ctypes.byref(a), None) == 0, _last_error(built_lib)
