"""f3r_gemm_plan_name / f3r_attn_kernel_name: the launch plan of csrc/f3r_dispatch.h as text, held to the eligibility that gemm_cases / conv_cases
restate.  Nothing is launched.  Without a device the hand-scheduled kernels cannot be loaded and are never planned: the test marked `gpu` covers them."""
import ctypes

import pytest

import conv_cases as cc
import gemm_cases as gc
from gemm_cases import ConvTCase, GemmCase, QkvCase
from fast3r_amd import _lib, ops
from test_dispatch_rules import _attn, _set

AT = 0x10000
FORM = {2: "staggered", 3: "lock-step", 4: "staggered", 5: "staggered, one tile per workgroup"}


def plan_name(lib, g):
    f = lib._Z18f3r_gemm_plan_nameRK13f3r_gemm_args   # const char* f3r_gemm_plan_name(const f3r_gemm_args&): csrc/f3r_dispatch.h
    f.restype, f.argtypes = ctypes.c_char_p, [ctypes.POINTER(_lib.GemmArgs)]
    return f(ctypes.byref(g)).decode()


def conv_args(c, sel):
    """the f3r_gemm_args ops.conv3x3 builds for a conv_cases.ConvCase, with stand-in addresses"""
    g = _lib.GemmArgs()
    oh, ow = c.out_hw
    planes = 1 if c.split is None else 2
    g.A = g.W = g.out_lp = AT
    g.M, g.N, g.Kpad = c.M, c.Co, planes * 9 * ((c.Ci + 63) // 64) * 64
    g.a_mode, g.conv_H, g.conv_W, g.conv_C, g.conv_stride, g.conv_OH, g.conv_OW = _lib.F3R_A_CONV3X3, c.H, c.W, c.Ci, c.stride, oh, ow
    g.epi, g.dtype, g.split, g.ldo_lp, g.kernel_sel = _lib.F3R_EPI_GENERIC, _lib.dtype_id(c.dtype), ops.SPLIT[c.split], c.Co, sel
    g.a_relu = int("a_relu" in c.extras)
    if "bias" in c.extras:
        g.bias = AT
    if c.split is not None:
        g.A_lo = AT
    if c.split == "x3f8":
        g.w_scale = AT
    if "skips" in c.extras:
        g.res_lp = g.res_lp2 = g.out_relu = AT
        g.ldr_lp = g.ldr_lp2 = c.Co
    if "fin" in c.extras:
        g.fin_w = g.fin_b = g.fin_pts = AT
        g.fin_n_out, g.out_lp = 3, None
    return g


def check_256(name, width, sel):
    assert name.startswith("gemm256_kernel") and f" 256x{width} " in name and name.endswith(FORM[sel]), (name, width, sel)


def test_forced_forms_name_their_family_and_form_or_nothing(built_lib):
    n = 0
    for c in gc.STATIC + gc.second_tile_cases(gc.CU_NOMINAL):
        if getattr(c, "split", None) == "w2f8":
            continue   # (one family, hand-scheduled: needs a device)
        assert gc.legal(c) is None
        assert plan_name(built_lib, gc.stand_in_args(c, 1)) == "gemm_kernel 128x128 (f3r_gemm.hip)", c.id
        for sel in (2, 3, 4, 5):
            name = plan_name(built_lib, gc.stand_in_args(c, sel))
            if gc.eligible256(c):
                check_256(name, gc.tile_width(c, sel), sel)
                n += 1
            else:
                assert name == "", (c.id, sel, name)
    assert n > 400
    # what gemm_cases.legal refuses has no plan
    for c in (GemmCase(16, 6, 64), GemmCase(16, 8, 12), GemmCase(16, 8, 64, lda=60), GemmCase(16, 8, 64, "gelu", ldo_lp=6), QkvCase(2, 70, 96, 96, 64), ConvTCase(1, 1, 1, 64, 6, 2)):
        assert gc.legal(c) and plan_name(built_lib, gc.stand_in_args(c, 1)) == "", c.id


def by_shape(name, c, eligible256, width128):
    """kernel_sel 0 / 7: a family whose restated eligibility holds"""
    if name.startswith("f3r_gemm_asm"):
        assert gc.eligible_asm(c), (c.id, name)
    elif name.startswith("gemm256_kernel"):
        assert eligible256 and ((" 256x128 " in name) if width128 else (" 256x" in name)) and name.endswith("staggered"), (c.id, name)
    else:
        assert name == "gemm_kernel 128x128 (f3r_gemm.hip)", (c.id, name)


def test_selection_by_shape_names_an_eligible_family(built_lib):
    n128 = 0
    for c in gc.STATIC + gc.second_tile_cases(gc.CU_NOMINAL):
        if getattr(c, "split", None) == "w2f8":
            continue
        for sel in (0, 7):
            name = plan_name(built_lib, gc.stand_in_args(c, sel))
            by_shape(name, c, gc.eligible256(c), c.kind != "qkv" and c.N % 256 != 0)
            assert sel == 0 or not name.startswith("f3r_gemm_asm")
            if not gc.eligible256(c) and not gc.eligible_asm(c):
                assert name == "gemm_kernel 128x128 (f3r_gemm.hip)", c.id
                n128 += 1
    assert n128 > 100


CONV = cc.TINY + cc.STRIDE2 + cc.TAILS + cc.second_tile_cases(cc.CU_NOMINAL) + [cc.GUARD_OVER_X3, cc.GUARD_OVER_F8, cc.GUARD_FITS_X3]


def test_convolutions_name_their_family_and_form_or_nothing(built_lib):
    seen = set()
    for c in CONV:
        one_family = c.split == "x3f8" or "fin" in c.extras     # no second path: every kernel_sel plans that family, or nothing
        ok = cc.eligible256(c)
        for sel in (0, 1, 2, 3, 4, 5):
            name = plan_name(built_lib, conv_args(c, sel))
            if one_family:
                assert name.startswith("gemm256_kernel (x3f8 / fused tail) 256x") == ok and (ok or name == ""), (c.id, sel, name)
                assert ("merged schedule" in name) == (ok and sel == 5 and c.split == "x3f8" and "fin" in c.extras), (c.id, sel, name)
            elif sel == 1:
                assert name == "gemm_kernel 128x128 (f3r_gemm.hip)", c.id
            elif sel == 0:
                by_shape(name, c, ok, c.Co % 256 != 0)
                assert ok or name == "gemm_kernel 128x128 (f3r_gemm.hip)", (c.id, name)
            elif ok:
                check_256(name, 128 if (c.Co % 256 or sel == 4) else 256, sel)
            else:
                assert name == "", (c.id, sel, name)
            seen.add(name.split(" 256x")[0])
    assert seen == {"", "gemm_kernel 128x128 (f3r_gemm.hip)", "gemm256_kernel", "gemm256_kernel (x3f8 / fused tail)"}
    assert plan_name(built_lib, conv_args(cc.GUARD_OVER_F8, 0)) == "" and plan_name(built_lib, conv_args(cc.GUARD_OVER_X3, 0)).startswith("gemm_kernel 128x128")


def attn_name(lib, a):
    return lib.f3r_attn_kernel_name(ctypes.byref(a)).decode()


def test_attention_names_nothing_for_a_call_that_selection_refuses(built_lib):
    """the HIP kernels by their instance; "" where f3r_attn_fwd returns F3R_ERR_UNSUPPORTED (before the plan, the name function named the three-product
    kernel for qk_planes >= 2 with kernel_sel 1, and the general kernel for kernel_sel 2 on an ineligible launch)"""
    for block, kw in ((_attn(planes=2, sel=1), {}), (_attn(planes=3, sel=1), {}), (_attn(sel=2), dict(causal=1)), (_attn(sel=2), dict(q_prescaled=0)),
                      (_attn(hd=96, sel=2), {}), (_attn(planes=2, sel=0), dict(q_prescaled=0))):
        a = block()
        _set(tq=128, **kw)(a)
        assert attn_name(built_lib, a) == "" and built_lib.f3r_attn_fwd(ctypes.byref(a), None) == -2, kw
    for block, kw, want in ((_attn(), {}, "attn_kernel (f3r_attn.hip)"), (_attn(), dict(batch=2), "attn_kernel<batched> (f3r_attn.hip)"),
                            (_attn(sel=0), dict(causal=1), "attn_kernel<causal> (f3r_attn.hip)"), (_attn(hd=96, sel=0), {}, "attn_generic_kernel (f3r_attn_generic.hip)"),
                            (_attn(hd=80), {}, "attn_generic_kernel (f3r_attn_generic.hip)")):
        a = block()
        _set(**kw)(a)     # (tq = 0: named, never launched)
        assert attn_name(built_lib, a) == want and built_lib.f3r_attn_fwd(ctypes.byref(a), None) == 0


@pytest.mark.gpu
def test_hand_scheduled_family_is_planned_exactly_where_it_is_eligible(built_lib):
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n6 = 0
    for c in gc.STATIC + gc.second_tile_cases(n_cu):
        if getattr(c, "split", None) == "w2f8":
            assert plan_name(built_lib, gc.stand_in_args(c, 0)) == "f3r_gemm_asm (w2f8)", c.id
            continue
        want = "f3r_gemm_asm (qkv pair)" if c.kind == "qkv" else "f3r_gemm_asm"
        ok = gc.eligible_asm(c)
        assert plan_name(built_lib, gc.stand_in_args(c, 6)) == (want if ok else ""), c.id
        assert plan_name(built_lib, gc.stand_in_args(c, 9)) == (want + ", start skew" if ok else ""), c.id
        name = plan_name(built_lib, gc.stand_in_args(c, 0))
        by_shape(name, c, gc.eligible256(c), c.kind != "qkv" and c.N % 256 != 0)
        n6 += ok
    assert n6 > 20
    # by shape: one full round of 256 x 256 tiles goes to the hand-scheduled kernel, a round and a bit (the last round under 80 % full) does not
    cus = n_cu // 8 * 8
    assert plan_name(built_lib, gc.stand_in_args(GemmCase(256 * cus, 256, 256, "gelu"), 0)) == "f3r_gemm_asm"
    assert plan_name(built_lib, gc.stand_in_args(GemmCase(256 * (cus + 8), 256, 256, "gelu"), 0)).startswith("gemm256_kernel 256x")
    assert plan_name(built_lib, gc.stand_in_args(GemmCase(256 * cus, 256, 256, "gelu"), 7)).startswith("gemm256_kernel 256x")
