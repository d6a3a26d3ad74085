"""The plain-operand GEMM geometry cases without a GPU: the references of tests/gemm_cases.py against a direct float64 product on the materialised
batch, the case lists against the properties tests/test_gemm_geometry_gpu.py relies on (computed from shapes alone), the strided sentinel helper, and
the eligibility restated in gemm_cases against the library's own rules through host-side calls."""
import ctypes
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import gemm_cases as gc
from gemm_cases import BF16, H16, ConvTCase, GemmCase, QkvCase
from fast3r_amd import _lib, ops

STATIC = gc.STATIC
ALL = STATIC + gc.second_tile_cases(gc.CU_NOMINAL)


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("role,split,dt", [("resf32", None, H16), ("gelu", None, BF16), ("both", "x3", H16), ("f32", "w2", BF16), ("relu2res", "x3", BF16)])
def test_periodic_reference_equals_the_direct_product_on_the_full_batch(role, split, dt):
    c = GemmCase(7 * 256, 132, 72, role, split, dt, P=3)
    d = gc.build_gemm(c)
    assert d["a"].shape == (768, 72) and d["ref"].shape == (768, 132)
    a = gc.periodic(d["a"], c.M).double()
    if split == "x3":
        a = a + gc.periodic(d["a_lo"], c.M).double()
    w = d["w32"].double() if split else d["w32"].to(dt).double()
    full = a @ w.t()
    if d["bias"] is not None:
        full = full + d["bias"].double()
    full = {"gelu": F.gelu, "relu": F.relu, None: lambda t: t}[c.spec["act"]](full)
    if d["x"] is not None:
        full = full + gc.periodic(d["x"], c.M).double()
    for hi, lo in d["res"] or []:
        full = full + gc.periodic(hi, c.M).double() + gc.periodic(lo, c.M).double()
    ref = gc.periodic(d["ref"], c.M)
    assert full.shape == (7 * 256, 132)
    # x3: the reference takes the unrounded operand, hi + lo carries it to the planes' precision; float64 against float64 otherwise
    tol = {None: 1e-12, "w2": 1e-12, "x3": 2.0 ** -20 if dt == H16 else 2.0 ** -14}[split]
    assert float((full - ref).abs().max()) <= tol * float(ref.abs().max())
    assert torch.equal(ref[768:1536], ref[:768]) and torch.equal(ref[1536:], ref[:256]) and not torch.equal(ref[:256], ref[256:512])


def test_rowadd_reference_indexes_rows_by_the_divisor():
    c = GemmCase(321, 68, 72, "rowadd", None, H16, 70)
    d = gc.build_gemm(c)
    assert d["rowadd"].shape == (5, 68)
    base = d["a"].double() @ d["w32"].to(H16).double().t() + d["bias"].double()
    for m in (0, 69, 70, 279, 280, 320):
        assert torch.allclose(d["ref"][m], base[m] + d["rowadd"][m // 70].double(), rtol=0, atol=1e-12)
    assert gc.build_gemm(GemmCase(17, 4, 8, "rowadd", None, H16, 17))["rowadd"].shape == (1, 4)
    assert gc.build_gemm(GemmCase(17, 4, 8, "rowadd", None, H16, 1))["rowadd"].shape == (17, 4)


def test_k_tail_of_the_packed_weight_is_zero():
    c = GemmCase(15, 60, 72, "f32", "w2", BF16)
    d = gc.build_gemm(c)
    assert d["w"].shape == (60, 256) and float(d["w"][:, 72:128].abs().sum()) == 0.0 and float(d["w"][:, 200:].abs().sum()) == 0.0


def _rope_direct(t, S, gw, heads):
    """RoPE-2D row by row: dims [0, 32) of a head rotate by the token's grid row, [32, 64) by its grid column, dim i paired with i + 16, angle
    pos * 100^(-i / 16)"""
    out = t.clone()
    freq = 100.0 ** (-torch.arange(16, dtype=torch.float64) / 16.0)
    for m in range(t.shape[0]):
        pos = m % S
        for h in range(heads):
            for half, p in ((0, pos // gw), (1, pos % gw)):
                o = h * 64 + half * 32
                a, b = t[m, o:o + 16], t[m, o + 16:o + 32]
                ang = p * freq
                out[m, o:o + 16] = a * ang.cos() - b * ang.sin()
                out[m, o + 16:o + 32] = b * ang.cos() + a * ang.sin()
    return out


@pytest.mark.parametrize("c", [QkvCase(5, 12, 192, 64, 72, BF16, (3, 4), gc.QS, P=2), QkvCase(4, 6, 64, 64, 64, H16, None, 0.0, P=3)], ids=lambda c: c.id)
def test_qkv_reference_equals_the_direct_product_with_rope(c):
    d = gc.build_qkv(c)
    assert d["a"].shape[0] == c.P * c.S
    a = gc.periodic(d["a"].view(c.P, c.S, c.K), c.n_seq).reshape(c.M, c.K).double()
    y = a @ d["w_rows"].double().t() + d["bias"].double()
    q, k, v = y[:, :c.Dq], y[:, c.Dq:c.Dq + c.Dkv], y[:, c.Dq + c.Dkv:]
    if c.grid:
        q, k = _rope_direct(q, c.S, c.grid[1], c.Dq // 64), _rope_direct(k, c.S, c.grid[1], c.Dkv // 64)
    q = q * (c.q_scale or 1.0)
    for name, full in (("q", q), ("k", k), ("v", v)):
        ref = gc.periodic(d["ref"][name].view(c.P, c.S, -1), c.n_seq).reshape(c.M, -1)
        assert full.shape == ref.shape
        assert float((full - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), name   # (the tables are fp32: cos / sin to 6e-8)
    assert d["w"].shape == (c.N, 128 if c.K == 72 else c.K)


@pytest.mark.parametrize("c", [ConvTCase(3, 5, 7, 72, 24, 2, None, BF16), ConvTCase(2, 1, 3, 64, 8, 4, "x3", H16), ConvTCase(1, 1, 1, 64, 32, 2, None, H16)], ids=lambda c: c.id)
def test_convt_reference_is_conv_transpose2d(c):
    d = gc.build_convt(c)
    if c.split == "x3":
        x, wt = d["x32"].double(), d["wt"].double()
    else:
        x, wt = d["x"].double(), d["wt"].to(c.dtype).double()
    full = F.conv_transpose2d(x.permute(0, 3, 1, 2), wt, d["bias32"].double(), stride=c.s).permute(0, 2, 3, 1)
    assert full.shape == d["ref"].shape == (c.B, c.h * c.s, c.w * c.s, c.Co)
    assert float((full - d["ref"]).abs().max()) <= 1e-12 * float(full.abs().max())


# ------------------------------------------------------------------------------------------------ the case lists
def test_case_ids_are_unique():
    for cases in (gc.EDGES, gc.STRIDES, gc.QKV, gc.CONVT, gc.second_tile_cases(gc.CU_NOMINAL), STATIC):
        ids = [c.id for c in cases]
        assert len(set(ids)) == len(ids)


def test_every_case_is_a_legal_launch():
    for c in ALL:
        assert gc.legal(c) is None, (c.id, gc.legal(c))
        sels = gc.kernel_sels(c)
        assert sels == [0] or (sels[0] == 1 and sels[-1] == 0)
    # the restated rules notice what the library would refuse
    assert gc.legal(GemmCase(16, 6, 64)) and gc.legal(GemmCase(16, 8, 12)) and gc.legal(GemmCase(16, 8, 64, lda=60))
    assert gc.legal(GemmCase(16, 8, 64, "gelu", ldo_lp=6)) and gc.legal(GemmCase(16, 8, 64, "resf32", ldo_f32=12)) and gc.legal(GemmCase(16, 8, 64, "rowadd"))
    assert gc.legal(QkvCase(2, 70, 96, 96, 64)) and gc.legal(QkvCase(2, 70, 64, 64, 64, H16, (7, 9))) and gc.legal(ConvTCase(1, 1, 1, 64, 6, 2))
    assert gc.legal(dataclasses.replace(gc.STRIDE_F8, lda=380)) and gc.legal(dataclasses.replace(gc.STRIDE_F8, M=300))


def test_edge_lists_contain_the_named_values():
    e = gc.EDGES
    assert gc.EDGE_M == (1, 15, 16, 17, 63, 65, 127, 129, 255, 257, 321, 513) and {c.M for c in e} == set(gc.EDGE_M)
    assert {c.N for c in e} == {4, 60, 68, 124, 132, 260, 128, 256, 384, 640} and {c.K for c in e} == {8, 72, 64, 128, 192}
    assert set(gc.ROLES) == {"f32", "gelu", "relu2res", "resf32", "rowadd", "both", "nobias"}
    for role in gc.ROLES:
        mine = [c for c in e if c.role == role]
        for M in gc.EDGE_M:   # every M meets the role on the 128-tile kernel alone and on every form that accepts the role
            forms = [tuple(gc.kernel_sels(c)) for c in mine if c.M == M]
            assert (1, 0) in forms and (role == "relu2res" or (1, 2, 3, 4, 5, 0) in forms), (role, M)
        assert {c.N for c in mine} == {c.N for c in e}, role
        for N in gc.EDGE_N256:   # ... and so does every N that the 256-tile forms take
            assert all(gc.eligible256(c) == (role != "relu2res") for c in mine if c.N == N), (role, N)
        assert {c.dtype for c in mine} == {H16, BF16} and {c.split for c in mine} == {None, "w2", "x3"}, role
        assert {c.K for c in mine} == {8, 72, 64, 128, 192}, role
    assert all(c.K in gc.EDGE_K256 for c in e if c.N in gc.EDGE_N256) and not any(gc.eligible256(c) for c in e if c.N in gc.EDGE_N128)
    assert not any(gc.eligible_asm(c) for c in e)   # (no edge M is a whole number of 256-row tiles)
    rows = [c for c in e if c.role == "rowadd"]
    assert {("M" if c.div == c.M else c.div) for c in rows if c.M > 70} == {1, 70, "M"}
    for wide in (False, True):
        assert {("M" if c.div == c.M else c.div) for c in rows if (c.N in gc.EDGE_N256) == wide and c.M > 70} == {1, 70, "M"}
    assert all(bool(c.div) == (c.role == "rowadd") for c in e)
    assert any(c.want_lo and c.role == "both" for c in e) and any(c.split == "x3" and c.role == "relu2res" for c in e)


def test_stride_cases_cover_the_named_strides():
    s = gc.STRIDES
    assert {(c.M, c.N) for c in s} == {(512, 256), (300, 132)}
    for M, N in ((512, 256), (300, 132)):
        mine = [c for c in s if (c.M, c.N) == (M, N)]
        K = 128
        assert {c.lda for c in mine if c.K == K} >= {K + 8, K + 64} and {c.ldo_f32 for c in mine} >= {N + 4}
        assert {c.ldo_lp for c in mine} >= {N + 8, (3 * N // 2 + 7) // 8 * 8} and {c.ldr_f32 for c in mine} >= {N + 4}
        assert any(c.ldr_lp == N + 4 and c.ldr_lp2 not in (0, c.ldr_lp) for c in mine)
        assert {c.dtype for c in mine} == {H16, BF16} and {c.role for c in mine} == set(gc.ROLES)
    assert (3 * 256 // 2 + 7) // 8 * 8 == 3 * 256 // 2
    six = [c for c in s if 6 in gc.kernel_sels(c)]
    assert six and all(c.M % 256 == 0 and c.N % 256 == 0 and c.K >= 128 * (1 if c.split else 2) for c in six)
    assert {c.role for c in six} >= {"f32", "gelu", "resf32"} and any(c.lda for c in six) and any(c.ldo_lp > c.N for c in six) and any(c.ldr_f32 > c.N for c in six)
    f8 = gc.STRIDE_F8
    assert (f8.M, f8.N, f8.K) == (512, 256, 256) and f8.lda * 2 > 3 * f8.K and f8.f8_rows and f8.ldo_lp * 2 > 3 * f8.N and gc.kernel_sels(f8) == [0]


def test_qkv_cases_cover_straddled_tiles_and_ragged_sequences():
    q = gc.QKV
    narrow = [c for c in q if not gc.eligible256(c)]
    assert {c.Dq for c in narrow if c.Dq == c.Dkv} == {64, 192, 320} and any((c.Dq, c.Dkv) == (192, 64) for c in narrow)
    # a 128-wide tile of the 128-tile kernel holds the end of one part and the start of the next
    assert all(c.Dq % 128 == 64 or (c.Dq + c.Dkv) % 128 == 64 for c in narrow)
    wide = [c for c in q if gc.eligible256(c)]
    assert all(gc.kernel_sels(c) == [1, 2, 3, 5, 0] and c.Dq == 256 for c in wide)
    assert any(c.S == 70 and c.n_seq == 8 and c.grid == (7, 10) for c in wide) and any(c.S == 70 and c.n_seq == 8 and c.grid is None for c in wide)
    for group in (narrow, wide):
        assert {c.dtype for c in group} == {H16, BF16}
        assert any(c.S == 1 and c.n_seq == 260 for c in group)
        assert any(c.S % 4 and c.S > 1 for c in group)
        # a tile boundary (128 / 256 rows) inside a sequence
        assert any(c.M > 256 and 256 % c.S for c in group if c.S > 1) or any(c.M > 128 and 128 % c.S for c in group if c.S > 1)
    assert any(c.ldvt > ops.vt_ld(c.S) for c in q) and any(c.K % 64 for c in narrow)


def test_convt_cases_cover_the_small_grids():
    t = gc.CONVT
    for hw in gc.CONVT_HW:
        for s in (2, 4):
            mine = [c for c in t if (c.h, c.w) == hw and c.s == s and gc.eligible256(c)]
            assert min(c.M for c in mine) == (1 if hw == (1, 1) else hw[0] * hw[1])
            assert any(c.M < 128 for c in mine) and any(256 < c.M <= 300 for c in mine), (hw, s)
            for M in {c.M for c in mine}:
                assert {(c.split, c.dtype) for c in mine if c.M == M} == {(None, H16), (None, BF16), ("x3", H16), ("x3", BF16)}
            assert all(gc.kernel_sels(c) == [1, 2, 3, 4, 5, 0] for c in mine)
    assert any(c.M == 1 for c in t) and any(gc.kernel_sels(c) == [1, 0] for c in t) and {c.N for c in t} >= {96, 128, 256}


def test_second_tile_cases_need_more_tiles_than_cus():
    n_cu = gc.CU_NOMINAL
    cases = gc.second_tile_cases(n_cu)
    for c in cases:
        assert c.M == 256 * (n_cu + 4) and c.P in (3, 5) and not gc.period_hides_a_stale_tile(c, n_cu)
        for sel in gc.second_tile_sels(c):
            assert sel in gc.kernel_sels(c) and gc.tiles(c, sel) >= n_cu + 4, (c.id, sel)   # workgroups 0 .. 3 (at least) walk a second tile
        assert 5 in gc.second_tile_sels(c)
    g = [c for c in cases if c.kind == "gemm"]
    assert {(c.N, c.K) for c in g} >= {(256, 64), (512, 192), (128, 64), (256, 256), (256, 320)}
    assert all(gc.second_tile_sels(c) == [4, 5] for c in g if c.N == 128)
    for dt in (H16, BF16):
        small = {(c.role, c.split) for c in g if c.dtype == dt and c.K < 256}
        assert small == {("resf32", None), ("gelu", None), ("both", "x3")}
        six = [c for c in cases if c.dtype == dt and 6 in gc.second_tile_sels(c)]
        assert {c.K for c in six} == {256, 320} and {getattr(c, "role", "qkv") for c in six} >= {"resf32", "gelu", "qkv"}
        assert any(c.kind == "qkv" and c.K < 256 and c.Dq == 256 for c in cases if c.dtype == dt)
    assert gc.period_hides_a_stale_tile(cases[0], 255) and gc.second_tile_M(256) == 66560


# ------------------------------------------------------------------------------------------------ guarded placement
@pytest.mark.parametrize("dt", [H16, BF16, torch.float32])
def test_strided_out_notices_stores_into_the_gap_and_behind_the_last_row(dt):
    g = gc.strided_out(5, 12, 20, dt, "cpu")
    assert g.view.shape == (5, 12) and g.view.stride() == (20, 1) and g.view.data_ptr() % 16 == 0
    es = g.view.element_size()
    assert g.buf.element_size() == es and g.lead >= 3 * 20 and g.buf.numel() == 2 * g.lead + 5 * 20
    g.view.fill_(1.5)
    assert gc.guards_intact(g)
    assert bool(torch.isfinite(g.buf.view(dt).float()).all())
    first = g.lead
    for at in (first - 1, first + 12, first + 19, first + 4 * 20 + 12, first + 5 * 20 - 1,   # before; gap of row 0, of the last row
               first + 5 * 20, first + 5 * 20 + 11, 0, g.buf.numel() - 1):                  # the row behind the last one; either end
        b2 = dataclasses.replace(g, buf=g.buf.clone())
        b2.buf[at] = 0
        assert not gc.guards_intact(b2), at
    b2 = dataclasses.replace(g, buf=g.buf.clone())
    b2.buf[first + 3 * 20 + 11] = 0     # (the last column of a row is an output)
    assert gc.guards_intact(b2)
    dense = gc.strided_out(3, 8, 8, dt, "cpu")
    dense.view.zero_()
    assert gc.guards_intact(dense)


@pytest.mark.parametrize("dt", [H16, torch.float32])
def test_guarded_rows_fills_the_gap_columns_with_nan_patterns(dt):
    t = (torch.arange(7 * 24) % 100).to(dt).view(7, 24)
    view, buf = gc.guarded_rows(t, 32, "cpu")
    assert torch.equal(view, t) and view.stride() == (32, 1) and view.data_ptr() % 16 == 0
    es = t.element_size()
    off = view.data_ptr() - buf.data_ptr()
    whole = buf[off:off + 7 * 32 * es].view(dt).view(7, 32)
    assert bool(whole[:, 24:].isnan().all()) and bool(buf[:off].eq(0xFF).all()) and bool(buf[off + 7 * 32 * es:].eq(0xFF).all())
    assert off >= 2 * 32 * es
    dense, _ = gc.guarded_rows(t, 24, "cpu")
    assert dense.is_contiguous() and torch.equal(dense, t)


# ------------------------------------------------------------------------------------------------ the restated eligibility against the library
def _eligible256(lib, g):
    f = lib._Z20f3r_gemm256_eligibleRK13f3r_gemm_args   # bool f3r_gemm256_eligible(const f3r_gemm_args&): csrc/f3r_common.h
    f.restype, f.argtypes = ctypes.c_bool, [ctypes.POINTER(_lib.GemmArgs)]
    return bool(f(ctypes.byref(g)))


NOT_LOADED = b"the embedded code object could not be loaded"   # the last obstacle f3r_gemm_asm_eligible names: every rule about the launch is met


def asm_rules_met(lib, g, qkv):
    """f3r_gemm_asm_eligible / f3r_gemm_asm_qkv_eligible(const f3r_gemm_args&, const char** why): eligible, or refused only because no device is there
    to load the kernel on"""
    f = lib._Z25f3r_gemm_asm_qkv_eligibleRK13f3r_gemm_argsPPKc if qkv else lib._Z21f3r_gemm_asm_eligibleRK13f3r_gemm_argsPPKc
    f.restype, f.argtypes = ctypes.c_bool, [ctypes.POINTER(_lib.GemmArgs), ctypes.POINTER(ctypes.c_char_p)]
    why = ctypes.c_char_p()
    ok = bool(f(ctypes.byref(g), ctypes.byref(why)))
    return ok or (why.value or b"").startswith(NOT_LOADED)


def test_restated_eligibility_is_the_librarys(built_lib):
    n256 = nasm = 0
    for c in ALL:
        if getattr(c, "split", None) == "w2f8":
            continue
        g = gc.stand_in_args(c)
        assert _eligible256(built_lib, g) == gc.eligible256(c), c.id
        assert asm_rules_met(built_lib, g, c.kind == "qkv") == gc.eligible_asm(c), c.id
        n256 += gc.eligible256(c)
        nasm += gc.eligible_asm(c)
    assert n256 > 100 and nasm > 20


def test_the_library_accepts_the_arguments_of_every_case(built_lib):
    """f3r_gemm's own argument checks on the arguments of every case and form: with M = 0 the call validates everything (the rules about M are
    restated in gemm_cases.legal) and returns before it launches"""
    for c in ALL:
        if getattr(c, "split", None) == "w2f8":
            continue
        for sel in gc.kernel_sels(c):
            if sel == 6:
                continue   # (the hand-scheduled kernel refuses M = 0: asm_rules_met holds it to its rules)
            g = gc.stand_in_args(c, sel, M=0)
            status = built_lib.f3r_gemm(ctypes.byref(g), None)
            assert status == 0, (c.id, sel, built_lib.f3r_last_error_string())
    bad = gc.stand_in_args(GemmCase(16, 6, 64), 1, M=0)
    assert built_lib.f3r_gemm(ctypes.byref(bad), None) != 0
    bad = gc.stand_in_args(GemmCase(16, 8, 64, "gelu", ldo_lp=6), 1, M=0)
    assert built_lib.f3r_gemm(ctypes.byref(bad), None) != 0
    bad = gc.stand_in_args(GemmCase(17, 132, 72), 2, M=0)     # a forced form on a shape it cannot take
    assert built_lib.f3r_gemm(ctypes.byref(bad), None) != 0
