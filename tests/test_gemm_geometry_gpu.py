"""The plain-operand launches of f3r_gemm at the edges of their geometry, on a real MI355X through the C ABI: the generic epilogue with M and N next
to every tile and fragment boundary, row strides wider than the rows on every operand and output, QKV parts that straddle a tile and sequences that
straddle a lane's four tokens, ConvT on grids of one to 35 pixels, and persistent workgroups that walk a second tile (cases and float64 references:
tests/gemm_cases.py).

Every case runs on every kernel form that the eligibility restated in gemm_cases lists for it -- a form the library refuses is a failure, never a
skip -- and is held to the tolerance the project already uses for that kind of output: fp32 outputs 2e-5, lowp outputs lp_tol, w2 / x3 against the
unrounded operands split_tol (a single lowp plane of a w2 launch: lp_tol), w2f8 against its decoded planes as test_gemm_asm_fp8_low_plane.  Every
operand lies inside a buffer of NaN patterns (the gap columns of a strided row included) and every output inside a buffer of sentinel words: a
load outside a plane poisons the result, a store outside the M x N outputs -- into the gap of a strided row, behind row M, into the V^T padding --
changes a sentinel.  After each launch the guards are asserted before any value is compared.
"""
import ctypes

import pytest
import torch

import gemm_cases as gc
from gemm_cases import H16
from fast3r_amd import _lib, ops
from test_gemm256_gpu import split_tol
from test_kernels_gpu import DEV, lp_tol

pytestmark = pytest.mark.gpu


def check(kind, got, ref, tol, what):
    """test_kernels_gpu.assert_close, with the figure printed before it is asserted"""
    got, ref = got.detach().double().cpu(), ref.double()
    scale = float(ref.abs().max().clamp_min(1e-6))
    err = float((got - ref).abs().max())
    print(f"[gemm-geometry] kind={kind} rel_err={err / scale:.3e} tol={tol:.1e} {what}")
    assert err == err and err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol:.1e})"


def _dt(c):
    return "f16" if c.dtype == H16 else "bf16"


def _intact(g, what):
    assert gc.guards_intact(g), f"{what}: a store outside the {g.rows} x {g.width} outputs (row stride {g.ld})"


class Placed:
    """operands in guarded placement: every buffer is kept alive with the launcher"""

    def __init__(self):
        self.keep = []

    def rows(self, t, ld=0, M=None):
        if t is None:
            return None
        t = t if M is None else gc.periodic(t, M)
        view, buf = gc.guarded_rows(t, ld or t.shape[1], DEV)
        self.keep.append(buf)
        return view

    def flat(self, t, margin=256):
        if t is None:
            return None
        view, buf = gc.guarded_operand(t, DEV, margin)
        self.keep.append(buf)
        return view


# ------------------------------------------------------------------------------------------------ the generic epilogue
class GemmLauncher(Placed):
    def __init__(self, c):
        super().__init__()
        self.c, self.d = c, gc.build_gemm(c)
        d, M = self.d, c.M
        self.a, self.a_lo = self.rows(d["a"], c.ld("lda"), M), self.rows(d["a_lo"], c.ld("lda"), M)
        self.w = self.rows(d["w"])
        self.bias, self.w_scale = self.flat(d["bias"]), self.flat(d["w_scale"])
        self.rowadd = self.rows(d["rowadd"])
        self.x = None if d["x"] is None else gc.periodic(d["x"], M).to(DEV)
        self.res = None
        if d["res"] is not None:
            lds = (c.ld("ldr_lp"), c.ld("ldr_lp2"))
            self.res = [(self.rows(hi, ld, M), self.rows(lo, ld, M)) for (hi, lo), ld in zip(d["res"], lds)]
        self.ref = d["ref"]   # one period

    def run(self, sel):
        """-> ({"f32" / "lp": the output (planes summed) as float64 on the device}, the raw output tensors)"""
        c, spec = self.c, self.c.spec
        what = f"{c.id} sel={sel}"
        kw = dict(bias=self.bias, act=spec["act"], kernel_sel=sel, split=c.split)
        outs = {}
        if spec["f32"]:
            outs["f32"] = gc.strided_out(c.M, c.N, c.ld("ldo_f32"), torch.float32, DEV)
            kw["out_f32"] = outs["f32"].view
            if spec.get("res_f32"):   # in place: the residual IS the output buffer
                outs["f32"].view.copy_(self.x)
                kw["res_f32"] = outs["f32"].view
        if spec["lp"]:
            outs["lp"] = gc.strided_out(c.M, c.lp_width, c.ld("ldo_lp"), c.dtype, DEV)
            kw["out_lp"] = outs["lp"].view
            if c.want_lo:
                outs["lp_lo"] = gc.strided_out(c.M, c.N, c.ld("ldo_lp"), c.dtype, DEV)
                kw["out_lp_lo"] = outs["lp_lo"].view
        if c.split == "x3":
            kw["a_lo"] = self.a_lo
        if c.split == "w2f8":
            kw.update(w_scale=self.w_scale, out_f8_rows=c.f8_rows)
        if spec.get("rowadd"):
            kw.update(rowadd=self.rowadd, rowadd_div=c.div)
        if self.res is not None:
            (r1, r1lo), (r2, r2lo) = self.res
            kw.update(res_lp=r1, res_lp2=r2, res_lp_lo=r1lo, res_lp2_lo=r2lo)
        ops.gemm(self.a, self.w, **kw)
        torch.cuda.synchronize()
        for name, g in outs.items():
            _intact(g, f"{what} {name}")
        got = {}
        if "f32" in outs:
            got["f32"] = outs["f32"].view
        if "lp" in outs:
            got["lp"] = outs["lp"].view[:, :c.N].double() + outs["lp_lo"].view.double() if c.want_lo else outs["lp"].view[:, :c.N]
        return got, [outs[k].view for k in sorted(outs)]

    def tol(self, name):
        c = self.c
        if c.split in ("w2", "x3") and (name == "f32" or c.want_lo):
            return split_tol(c.dtype)
        return 2e-5 if name == "f32" else lp_tol(c.dtype)

    def kind(self, name):
        planes = "+lo" if (name == "lp" and self.c.want_lo) else ""
        return f"gemm-{name}{planes}-{self.c.split or 'one'}-{_dt(self.c)}"


def _check_rows(L, got, sel, missed, rows=None):
    """the first `rows` rows (one period) of every output against the reference: figures printed, misses collected"""
    for name, g in got.items():
        try:
            check(L.kind(name), g[:rows] if rows else g, L.ref if isinstance(L.ref, torch.Tensor) else L.ref[name], L.tol(name), f"{L.c.id} {name} sel={sel}")
        except AssertionError as e:
            missed.append(str(e).splitlines()[0])


def _run_gemm(c):
    L = GemmLauncher(c)
    missed = []
    for sel in gc.kernel_sels(c):
        got, _ = L.run(sel)
        _check_rows(L, got, sel, missed)
    assert not missed, "; ".join(missed)


@pytest.mark.parametrize("c", gc.EDGES, ids=lambda c: c.id)
def test_generic_epilogue_edges(built_lib, c):
    """M and N next to multiples of 16, 64, 128 and 256: the wave-uniform interior / edge switch, the clamped loads (mc = M - 1, nbc = N - 4), rows and
    columns past the matrix, K tails; every role of the epilogue on every form"""
    _run_gemm(c)


@pytest.mark.parametrize("c", gc.STRIDES, ids=lambda c: c.id)
def test_row_strides(built_lib, c):
    """lda, ldo and ldr wider than the rows: the interior epilogues fold the stride into one 32-bit lane offset; the gaps must stay untouched (the
    model aliases hid onto the rows of hid8 and h onto rows8)"""
    _run_gemm(c)


def test_row_strides_fp8_rows(built_lib):
    """w2f8: rows [K fp16 | K fp8] with a gap behind them in, rows [N fp16 | N fp8] with a gap behind them out"""
    c = gc.STRIDE_F8
    L = GemmLauncher(c)
    assert gc.kernel_sels(c) == [0]
    g = gc.strided_out(c.M, c.lp_width, c.ld("ldo_lp"), c.dtype, DEV)
    ops.gemm(L.a, L.w, bias=L.bias, act="gelu", split="w2f8", w_scale=L.w_scale, out_lp=g.view, out_f8_rows=True)
    torch.cuda.synchronize()
    _intact(g, c.id)
    h16 = g.view[:, :c.N]
    check("gemm-lp-w2f8-f16", h16, L.ref, lp_tol(H16), f"{c.id} fp16 part")
    h8 = g.view.contiguous().view(torch.uint8).view(c.M, 3 * c.N)[:, 2 * c.N:].contiguous().view(torch.float8_e4m3fn).float().cpu()
    want8 = h16.float().clamp(max=448).to(torch.float8_e4m3fn).float().cpu()
    off = float(((h8 - want8).abs() > 0.13 * want8.abs().clamp_min(2.0 ** -9)).float().mean())   # as test_mlp_chain_on_fp8_rows
    print(f"[gemm-geometry] kind=gemm-f8copy-w2f8-f16 off_fraction={off:.3e} tol=2.0e-03 {c.id} fp8 part")
    assert off < 2e-3
    f = gc.strided_out(c.M, c.N, c.N + 4, torch.float32, DEV)   # the fp32 role of the same kernel family, strided
    ops.gemm(L.a, L.w, bias=L.bias, split="w2f8", w_scale=L.w_scale, out_f32=f.view)
    torch.cuda.synchronize()
    _intact(f, c.id + " f32")
    check("gemm-f32-w2f8-f16", f.view, L.d["pre_act"], 2e-5, f"{c.id} f32 role")


# ------------------------------------------------------------------------------------------------ QKV
class QkvLauncher(Placed):
    def __init__(self, c):
        super().__init__()
        self.c, self.d = c, gc.build_qkv(c)
        d = self.d
        a = d["a"]
        if c.P:
            a = gc.periodic(a.view(c.P, c.S, c.K), c.n_seq).reshape(c.M, c.K)
        self.a, self.w, self.bias = self.rows(a), self.rows(d["w"]), self.flat(d["bias"])
        self.rope = (self.flat(d["cos"], 64), self.flat(d["sin"], 64), c.grid[1]) if c.grid else None
        self.ref = d["ref"]

    def run(self, sel):
        c = self.c
        what = f"{c.id} sel={sel}"
        q = gc.strided_out(c.M, c.Dq, c.Dq, c.dtype, DEV)
        k = gc.strided_out(c.M, c.Dkv, c.Dkv, c.dtype, DEV)
        vt = gc.strided_out(c.n_seq * c.Dkv, c.S, c.vt_stride, c.dtype, DEV)   # the columns [S, ldvt) are gap columns: they must stay untouched
        vt3 = vt.view.unflatten(0, (c.n_seq, c.Dkv))
        assert vt3.stride() == (c.Dkv * c.vt_stride, c.vt_stride, 1)
        ops.gemm_qkv(self.a, self.w, self.bias, q.view, k.view, vt3, c.S, self.rope, q_scale=c.q_scale, kernel_sel=sel, q_dim=0 if c.Dq == c.Dkv else c.Dq)
        torch.cuda.synchronize()
        for name, g in (("q", q), ("k", k), ("vt", vt)):
            _intact(g, f"{what} {name}")
        return dict(q=q.view, k=k.view, v=vt3.permute(0, 2, 1).reshape(c.M, c.Dkv)), [q.view, k.view, vt3]

    def tol(self, name):
        return lp_tol(self.c.dtype)

    def kind(self, name):
        return f"qkv-{name}-{_dt(self.c)}"


@pytest.mark.parametrize("c", gc.QKV, ids=lambda c: c.id)
def test_qkv_parts_and_sequences(built_lib, c):
    """the 128-tile kernel with a tile that holds the end of one part and the start of the next (two waves of a workgroup in different operand
    roles); both kernels with seq_len % 4 != 0 (a lane's four V^T tokens span two sequences), S = 1 and tiles that end inside a sequence.
    With N an odd multiple of 64 the last tile hangs 64 columns over N: the wave that holds them once stored V^T channels d >= Dkv into the next
    sequence's rows and behind the buffer (the vt guard of every such case; gemm_epilogue_vt now skips columns n >= N)."""
    L = QkvLauncher(c)
    missed = []
    for sel in gc.kernel_sels(c):
        got, _ = L.run(sel)
        _check_rows(L, got, sel, missed)
    assert not missed, "; ".join(missed)


# ------------------------------------------------------------------------------------------------ ConvT
class ConvTLauncher(Placed):
    def __init__(self, c):
        super().__init__()
        self.c, self.d = c, gc.build_convt(c)
        d = self.d
        self.x = self.rows(d["x"].reshape(c.M, c.Ci))
        self.x_lo = None if d["x_lo"] is None else self.rows(d["x_lo"].reshape(c.M, c.Ci))
        self.w, self.bias = self.rows(d["w"]), self.flat(d["bias"])
        self.ref = d["ref"].reshape(-1, c.Co)

    def run(self, sel):
        """ops.convT with the output (and its low plane) placed by the caller"""
        c = self.c
        n_pix = c.M * c.s * c.s
        out = gc.strided_out(n_pix, c.Co, c.Co, c.dtype, DEV)
        lo = gc.strided_out(n_pix, c.Co, c.Co, c.dtype, DEV) if c.split else None
        g = _lib.GemmArgs()
        g.kernel_sel, g.split = sel, ops.SPLIT[c.split]
        g.A, g.W, g.bias = _lib.ptr(self.x), _lib.ptr(self.w), _lib.ptr(self.bias)
        if c.split:
            g.A_lo, g.out_lp_lo = _lib.ptr(self.x_lo), _lib.ptr(lo.view)
        g.M, g.N, g.K, g.Kpad, g.lda = c.M, c.N, c.Ci, self.w.shape[1], c.Ci
        g.a_mode, g.epi, g.act = _lib.F3R_A_PLAIN, _lib.F3R_EPI_CONVT, _lib.F3R_ACT_NONE
        g.out_lp, g.ldo_lp = _lib.ptr(out.view), c.Co
        g.ct_s, g.ct_h, g.ct_w, g.ct_cout = c.s, c.h, c.w, c.Co
        g.dtype = _lib.dtype_id(c.dtype)
        _lib.check(_lib.lib().f3r_gemm(ctypes.byref(g), _lib.stream_ptr()), "f3r_gemm(convT)")
        torch.cuda.synchronize()
        _intact(out, f"{c.id} sel={sel}")
        if lo is not None:
            _intact(lo, f"{c.id} sel={sel} low plane")
        return dict(out=out.view.double() + lo.view.double() if lo is not None else out.view), [out.view]

    def tol(self, name):
        return split_tol(self.c.dtype) if self.c.split else lp_tol(self.c.dtype)

    def kind(self, name):
        return f"convt-{self.c.split or 'one'}-{_dt(self.c)}"


@pytest.mark.parametrize("c", gc.CONVT, ids=lambda c: c.id)
def test_conv_transpose_small_grids(built_lib, c):
    """grids of 1 x 1 to 5 x 7 pixels, M = 1, below one tile and just above 256: the pixel-shuffle scatter at the image and batch boundaries"""
    L = ConvTLauncher(c)
    missed = []
    for sel in gc.kernel_sels(c):
        got, _ = L.run(sel)
        _check_rows(L, got, sel, missed)
    assert not missed, "; ".join(missed)


# ------------------------------------------------------------------------------------------------ the restatement on the device
def test_restated_eligibility_of_the_hand_scheduled_kernel(built_lib):
    """with its code object loaded: the library takes exactly the launches gemm_cases.eligible_asm lists (the CPU test can only see the rules
    about the launch)"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 0
    for c in gc.STATIC + gc.second_tile_cases(n_cu):
        if getattr(c, "split", None) == "w2f8":
            continue
        qkv = c.kind == "qkv"
        f = built_lib._Z25f3r_gemm_asm_qkv_eligibleRK13f3r_gemm_argsPPKc if qkv else built_lib._Z21f3r_gemm_asm_eligibleRK13f3r_gemm_argsPPKc
        f.restype, f.argtypes = ctypes.c_bool, [ctypes.POINTER(_lib.GemmArgs), ctypes.POINTER(ctypes.c_char_p)]
        why = ctypes.c_char_p()
        assert bool(f(ctypes.byref(gc.stand_in_args(c)), ctypes.byref(why))) == gc.eligible_asm(c), (c.id, why.value)
        n += gc.eligible_asm(c)
    assert n > 20


# ------------------------------------------------------------------------------------------------ a persistent workgroup's second tile
N_SECOND = len(gc.second_tile_cases(gc.CU_NOMINAL))


def _periods_equal(t, rows):
    """every period of `rows` rows of t [M][...] is the same bits as the first (the last one may be cut short)"""
    M = t.shape[0]
    full = M // rows
    first = t[:rows]
    ok = bool((t[:full * rows].unflatten(0, (full, rows)) == first).all())
    return ok and (M == full * rows or bool((t[full * rows:] == first[:M - full * rows]).all()))


@pytest.mark.parametrize("i", range(N_SECOND), ids=[c.id for c in gc.second_tile_cases(gc.CU_NOMINAL)])   # (ids: at the nominal CU count)
def test_second_tile_of_a_persistent_workgroup(built_lib, i):
    """more 256-row tiles than CUs: the first workgroups compute a second tile whose opening K-tile loads were issued before the first one's
    epilogue stores.  (a) one period against float64, (b) the one-tile-per-workgroup grid (kernel_sel 5) runs the same instructions per tile: the
    same bits as the persistent forms, (c) rows of period P tiles: every period of the output is the same bits as the first.  The
    hand-scheduled kernel (6; four and five K-tiles through its five-slot ring) has no other grid: (a) and (c)."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = gc.second_tile_cases(n_cu)[i]
    if gc.period_hides_a_stale_tile(c, n_cu):
        pytest.skip(f"content of period {c.period} tiles on {n_cu} CUs: a stale tile would carry identical content")
    sels = gc.second_tile_sels(c)
    for sel in sels:
        assert sel in gc.kernel_sels(c) and gc.tiles(c, sel) >= n_cu + 4
    L = GemmLauncher(c) if c.kind == "gemm" else QkvLauncher(c)
    rows = c.rows if c.kind == "gemm" else c.P * c.S
    missed, raws = [], {}
    for sel in sels:
        got, raw = L.run(sel)
        _check_rows(L, got, sel, missed, rows)                                                     # (a)
        for name, g in got.items():
            assert _periods_equal(g, rows), f"{c.id} {name} sel={sel}: a period of the output differs from the first"   # (c)
        raws[sel] = raw
    for sel in sels:                                                                               # (b)
        if sel in (5, 6):
            continue
        for a, b in zip(raws[sel], raws[5]):
            assert torch.equal(a, b), f"{c.id}: the persistent grid (kernel_sel {sel}) and one tile per workgroup differ"
    assert not missed, "; ".join(missed)
