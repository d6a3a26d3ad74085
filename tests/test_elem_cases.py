"""The elementwise / resize / fp32-attention edge cases without a GPU: the float64 references of tests/elem_cases.py against independent
statements of the same operations, the case lists against the structural properties tests/test_elem_geometry_gpu.py relies on (computed from
shapes alone), and -- per family -- a correct float32 restatement of the kernel that meets the family's tolerance next to a deliberately wrong
one that misses it on a listed case: the cases discriminate, shown here and never by seeding a fault into a kernel."""
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import elem_cases as ec
from elem_cases import BF16, H16
from fast3r_amd.params import CroCoEncoder, LlamaDecoder

LP_TOL = {H16: 2.0 ** -9, BF16: 2.0 ** -6}     # test_kernels_gpu.lp_tol (that module needs no GPU to import, but is a GPU module)


def _agree(a, b, tol=1e-12):
    return float((a - b).abs().max()) <= tol * float(b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ references against independent statements
@pytest.mark.parametrize("c", [ec.LnCase(260, 5), ec.LnCase(2052, 3, data="mean100"), ec.LnCase(8, 1), ec.LnCase(256, 3, data="equal")], ids=lambda c: c.id)
def test_layernorm_reference_is_F_layer_norm(c):
    d = ec.build_ln(c)
    want = F.layer_norm(d["x"].double(), (c.D,), d["gamma"].double(), d["beta"].double(), c.eps)
    assert _agree(d["ref"], want)
    if c.data == "equal":
        assert torch.equal(d["ref"], d["beta"].double().expand(c.rows, c.D))     # x - mean == 0 exactly: the output is beta
    r = ec.build_ln(dataclasses.replace(c, rms=True))
    x = r["x"].double()
    assert _agree(r["ref"], x / torch.sqrt((x * x).mean(-1, keepdim=True) + 1e-5) * r["gamma"].double())


@pytest.mark.parametrize("c", ec.BIL, ids=lambda c: c.id)
def test_bilinear_reference_is_the_explicit_gather(c):
    """F.interpolate on NCHW (the reference) against the four-tap formula on the NHWC plane as it lies in memory, float64 both"""
    d = ec.build_bil(c)
    assert d["ref"].shape == (c.B, *c.out, c.C)
    assert _agree(ec.bil_restate(d["xin"], c.full, c.out, torch.float64), d["ref"])


@pytest.mark.parametrize("c", [c for c in ec.ATTN if c.dtype == H16 and c.outs in ("all", "f32")], ids=lambda c: c.id)
def test_attention_reference_is_sdpa_with_zero_filled_rows(c):
    d = ec.build_attn(c)
    qh, kh, vh = ec._heads(c, d["q"].double(), d["k"].double(), d["v"].double())
    vis = ec.attn_visible(c)
    some = vis.any(-1)
    mask = vis | ~some[:, None]          # rows without a key attend to everything inside SDPA (no NaN) and are zero-filled behind it
    o = F.scaled_dot_product_attention(qh, kh, vh, attn_mask=mask, scale=c.scale)
    o = torch.where(some[None, None, :, None], o, torch.zeros_like(o)).permute(0, 2, 1, 3).reshape(c.n_seq * c.tq, c.H * c.HD)
    assert _agree(o, d["ref"])
    assert torch.equal(d["no_key"], ~some)
    rows = d["ref"].reshape(c.n_seq, c.tq, -1)
    assert bool((rows[:, d["no_key"]] == 0).all()) and bool((rows[:, ~d["no_key"]].abs().amax(-1) > 0).all())


@pytest.mark.parametrize("c", [c for c in ec.PATCH if c.dtype == H16], ids=lambda c: c.id)
def test_patchify_reference_is_the_explicit_reshape(c):
    d = ec.build_patch(c)
    assert d["ref"].shape == (c.patches, c.K) and torch.equal(ec.patch_ref(d["img"], c.ps), ec.patch_explicit(d["img"], c.ps))


@pytest.mark.parametrize("c", ec.ROPE, ids=lambda c: c.id)
def test_rope_reference_is_the_complex_product(c):
    d = ec.build_rope(c)
    assert _agree(ec.rope_complex(c, d["x"], d["cos"], d["sin"]), d["ref"])
    assert torch.equal(d["ref"][:, c.n_rot * 64:], d["x"].double()[:, c.n_rot * 64:])


def test_dpt_reference_is_postprocess_on_the_matrix_product():
    c = ec.DptCase(24, 257, True, BF16, depth="square", conf=("sigmoid", 0.5, 3.0))
    d = ec.build_dpt(c)
    z = torch.einsum("pc,oc->po", d["x"].double() + d["x_lo"].double(), d["w"].double()) + d["b"].double()
    n = z[:, :3].pow(2).sum(-1, keepdim=True).sqrt()
    assert _agree(z[:, :3] * n, d["pts"]) and _agree(0.5 + 2.5 / (1 + torch.exp(-z[:, 3])), d["conf"])


# ------------------------------------------------------------------------------------------------ the cases discriminate
@pytest.mark.parametrize("D", [260, 2052])
def test_mean_100_rows_tell_two_pass_from_one_pass_variance(D):
    c = ec.LnCase(D, 3, data="mean100")
    assert c in ec.LN
    d = ec.build_ln(c)
    two = ec.ln_math(d["x"], d["gamma"], d["beta"], c.eps, False)
    one = ec.ln_math(d["x"], d["gamma"], d["beta"], c.eps, False, one_pass=True)
    print(f"[elem-cases] ln mean100 D={D}: two-pass {ec.rel_err(two, d['ref']):.3e}, one-pass {ec.rel_err(one, d['ref']):.3e} (tol 2e-5)")
    assert ec.rel_err(two, d["ref"]) <= 2e-5 < ec.rel_err(one, d["ref"])
    plain = ec.build_ln(ec.LnCase(D, 3))     # on the zero-mean data of the other cases the one-pass form passes: only this row tells them apart
    assert ec.rel_err(ec.ln_math(plain["x"], plain["gamma"], plain["beta"], 1e-6, False, one_pass=True), plain["ref"]) <= 2e-5


def _bil_errs(fn):
    """per plain case: the rounded float32 result of fn against the reference, over the case's lowp tolerance (NaN counts as a miss)"""
    out = {}
    for c in ec.BIL:
        if c.form != "plain":
            continue
        d = ec.build_bil(c)
        e = ec.rel_err(fn(c, d).to(c.dtype), d["ref"])
        out[c.id] = (e / LP_TOL[c.dtype]) if e == e else float("inf")
    return out


def test_bilinear_cases_tell_align_corners_and_the_edge_clamp():
    good = _bil_errs(lambda c, d: ec.bil_restate(d["x"], c.full, c.out))
    assert max(good.values()) <= 1.0, good

    def half_pixel(c, d):
        y = F.interpolate(d["x"].float().permute(0, 3, 1, 2), size=c.full, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
        return y[:, :c.out[0], :c.out[1]]
    assert max(_bil_errs(half_pixel).values()) > 1.0
    no_clamp = _bil_errs(lambda c, d: ec.bil_restate(d["x"], c.full, c.out, edge_clamp=False))
    missed = [k for k, v in no_clamp.items() if v > 1.0]
    print(f"[elem-cases] bilinear without the edge clamp misses: {missed}")
    # the tap behind the last pixel carries weight 0: only the NaN guard behind the plane shows it (0 * NaN), and only where the output reaches
    # the plane's last row and column -- the uncropped cases
    assert missed and all("crop1x1" not in k or "to1x1" in k for k in missed)


def test_causal_cases_tell_a_mask_that_ignores_k_pos0():
    worst_good, worst_bad = 0.0, 0.0
    for c in ec.ATTN:
        if not (c.causal and c.outs == "f32" and c.dtype == H16):
            continue
        d = ec.build_attn(c)
        good = ec.rel_err(ec.attn_restate_f32(c, d["q"], d["k"], d["v"]), d["ref"])
        bad = ec.rel_err(ec.attn_restate_f32(c, d["q"], d["k"], d["v"], use_k_pos0=False), d["ref"])
        print(f"[elem-cases] {c.id}: restatement {good:.3e}, mask without k_pos0 {bad:.3e}")
        assert good <= ec.attn_tol(c, "f32") < bad
        worst_good, worst_bad = max(worst_good, good), max(worst_bad, bad)
    assert worst_bad > 1e-2


@pytest.mark.parametrize("hd", ec.ATTN_HD)
def test_float32_restatement_of_the_attention_meets_the_tolerance_at_every_width(hd):
    """the figure docs/parity.md records per head width: 32-key tiles and the online rescale in float32 against float64"""
    c = ec.AttnCase(hd, 33, 65, kv_group=2, n_seq=2)
    assert c in ec.ATTN
    d = ec.build_attn(c)
    e = ec.rel_err(ec.attn_restate_f32(c, d["q"], d["k"], d["v"]), d["ref"])
    print(f"[elem-cases] attention restatement hd={hd}: {e:.3e} (tol {ec.attn_tol(c, 'f32'):.1e})")
    assert e <= ec.attn_tol(c, "f32")


def test_rope_cases_tell_the_pair_offset():
    for c in ec.ROPE:
        d = ec.build_rope(c)
        good = ec.rel_err(ec.rope_math(c, d["x"], d["cos"], d["sin"]), d["ref"])
        bad = ec.rel_err(ec.rope_math(c, d["x"], d["cos"], d["sin"], pair=32), d["ref"])
        print(f"[elem-cases] rope {c.id}: restatement {good:.3e}, pair offset 32 {bad:.3e}")
        assert good <= 2e-6
        assert bad > 2e-6 or (c.mode == 0 and c.rows == 1)     # (position 0 rotates by the angle 0: the one-token case is there for the indexing)


def test_dpt128_cases_reach_the_clamp_of_the_ragged_group():
    """the staged rows of the last 64-pixel group, gathered from the plane followed by its guard: clamped to npix - 1 they are finite, clamped to
    npix (one row too far) they hold the guard's NaN -- except where npix is a multiple of 64 and nothing is clamped"""
    for npix in ec.DPT128_NPIX:
        c = ec.DptCase(128, npix)
        d = ec.build_dpt(c)
        plane = torch.cat([d["x"].float(), torch.full((1, 128), float("nan"))])
        last = (npix - 1) // 64
        good = plane[ec.dpt128_staged_rows(npix, last)]
        bad = plane[ec.dpt128_staged_rows(npix, last, clamp_to_last=False)]
        assert torch.isfinite(good).all()
        assert bool(torch.isnan(bad).any()) == (npix % 64 != 0)
    x = ec.build_dpt(ec.DptCase(128, 65, True))
    got = ec.dpt_math((x["x"].float() + x["x_lo"].float()), x["w"], x["b"], "exp", ("exp", 1.0, float("inf")))
    assert ec.rel_err(got[0], x["pts"]) <= 1e-5 and ec.rel_err(got[1], x["conf"]) <= 1e-5


@pytest.mark.parametrize("cin", [8, 128, 2048])
def test_float32_head_tail_meets_1e5_at_every_width(cin):
    """weights of size Cin^-1/2 keep the four outputs at unit variance, so the 1e-5 the project holds the head tail to is reachable by an fp32 sum
    over 2048 channels (the exp depth mode turns an absolute error of the norm into a relative one of the point)"""
    c = ec.DptCase(cin, 257 if cin != 128 else 129)
    d = ec.build_dpt(c)
    pts, cf = ec.dpt_math(d["x"].float(), d["w"], d["b"], c.depth, c.conf)
    print(f"[elem-cases] head tail fp32 Cin={cin}: pts {ec.rel_err(pts, d['pts']):.3e} conf {ec.rel_err(cf, d['conf']):.3e}")
    assert ec.rel_err(pts, d["pts"]) <= 1e-5 and ec.rel_err(cf, d["conf"]) <= 1e-5


# ------------------------------------------------------------------------------------------------ special data
def test_zero_pixel_and_saturation_cases_are_what_they_say():
    for c in ec.DPT:
        d = ec.build_dpt(c)
        assert torch.isfinite(d["pts"]).all() and (d["conf"] is None) == (c.n_out == 3)
        if c.special == "zero":
            assert float(d["xin"][0].abs().max()) == 0.0 and bool((d["pts"][0] == 0).all())
        if c.special == "saturate":
            z = d["xin"] @ d["w"][3].double() + d["b"][3].double()
            assert float(z.max()) >= ec.SATURATED and float(z.min()) <= -ec.SATURATED and abs(float(z.abs().max()) - 60.0) < 1e-3
            f = torch.sigmoid(z.float())     # fp32: exactly 1 / below 2^-43 from the threshold on
            assert bool((f[z >= ec.SATURATED] == 1).all()) and bool(((2.5 * f[z <= -ec.SATURATED] + 0.5) == 0.5).all())


@pytest.mark.parametrize("c", ec.LN_F8, ids=lambda c: c.id)
def test_fp8_row_seeds_have_no_value_on_a_rounding_boundary(c):
    """the GPU module compares the fused kernel's e4m3 codes with codes made from the plain kernel's fp32 output: two fp32 evaluations of one row
    differ by an ulp or two, so with no value within 32 ulps of a boundary the expected number of differing codes is zero"""
    d = ec.build_ln_f8(c)
    assert ec.f8_ties(d["ref"]) == 0
    assert c.D <= 40 or float(d["ref"].abs().max()) > 448.0      # the clamp is exercised
    assert c.ld % 8 == 0 and c.ld * 2 >= 3 * c.D


def test_fp8_row_widths_sit_behind_the_register_switches():
    """3 D / 2 is a multiple of 8 only for D % 16 == 0: the multiples of 8 right behind 0, 1024 and 2048 are refused by the entry point at either
    stride (the GPU module asserts the refusal), the next multiples of 16 take the three instantiations"""
    assert all(c.ld % 8 for c in ec.LN_F8_REFUSED) and {c.D for c in ec.LN_F8_REFUSED} == {8, 1032, 2056}
    assert [ec.ln_maxv(D) for D in ec.LN_F8_D] == [4, 8, 32] and [ec.ln_maxv(D - 16) for D in ec.LN_F8_D[1:]] == [4, 8]
    assert {c.pad for c in ec.LN_F8} == {0, 8} and {c.rows for c in ec.LN_F8} == {5}


# ------------------------------------------------------------------------------------------------ structure, from shapes alone
def test_layernorm_list_has_both_sides_of_each_register_switch():
    by_maxv = {}
    for c in ec.LN:
        by_maxv.setdefault(ec.ln_maxv(c.D), set()).add(c.D)
    assert {1024} <= by_maxv[4] and {1028, 2048} <= by_maxv[8] and {2052, 8192} <= by_maxv[32]
    passes = {-(-D // ec.LN_WAVE) for D in ec.LN_D}
    assert {4, 5, 8, 9} <= passes and max(passes) == 32 and 1 in passes
    assert {4, 252, 260} <= set(ec.LN_D)      # only some lanes hold a vector: 1, 63 and 65 float4
    assert {c.rows for c in ec.LN if c.D == 4} == {1, 3, 4, 5} and {c.rows for c in ec.LN if c.D >= 2052} == {3}
    assert {(c.outs, c.rms, c.dtype) for c in ec.LN if c.D == 1028} == {(o, r, t) for o in ("lp", "f32", "both") for r in (False, True) for t in ec.DTYPES}
    assert len({c.id for c in ec.LN}) == len(ec.LN)


def test_head_tail_list_has_the_ragged_groups():
    n128 = {c.npix % 64 for c in ec.DPT if c.Cin == 128 and not c.special and c.n_out == 4}
    assert {0, 1, 63} <= n128
    assert {(c.lo, c.npix) for c in ec.DPT if c.Cin == 128 and not c.special and c.n_out == 4} == {(lo, n) for lo in (False, True) for n in ec.DPT128_NPIX}
    assert {c.Cin for c in ec.DPT} == {8, 24, 128, 2048} and {c.npix for c in ec.DPT if c.Cin == 2048} == {257}
    assert {c.depth for c in ec.DPT if c.special == "zero"} == {"exp", "linear", "square"}
    assert any(c.n_out == 3 for c in ec.DPT) and any(c.special == "saturate" for c in ec.DPT)
    assert len({c.id for c in ec.DPT}) == len(ec.DPT)


def test_attention_lists_have_both_sides_of_the_workgroup_and_tile_edges():
    tq = {c.tq for c in ec.ATTN if c.HD in (64, 128) and not c.causal}
    tk = {c.tk for c in ec.ATTN if c.HD in (64, 128) and not c.causal}
    assert {1, ec.XQ - 1, ec.XQ, ec.XQ + 1} <= tq and {1, ec.XK - 1, ec.XK, ec.XK + 1} <= tk
    assert {c.HD for c in ec.ATTN} == set(ec.ATTN_HD)
    assert all(c.tk < 8192 for c in ec.ATTN)                                # below ops.ATTN_F32_MFMA_MIN_KEYS: the FMA kernel
    assert any(c.n_seq == 3 and c.tq == ec.XQ + 1 for c in ec.ATTN)         # workgroup edges inside a sequence
    assert {c.outs for c in ec.ATTN if c.pad} == {"f32", "hi", "all"}
    ca = {(c.q_pos0, c.k_pos0, c.tq, c.tk) for c in ec.ATTN if c.causal and c.HD == 64}
    assert ca == set(ec.ATTN_CAUSAL)
    for c in ec.ATTN:
        if not c.causal:
            continue
        vis = ec.attn_visible(c)
        for q0 in range(0, c.tq, ec.XQ):                                     # k_end of the workgroup, as the kernel computes it
            last_q = min(q0 + ec.XQ, c.tq) - 1
            k_end = max(0, min(c.tk, c.q_pos0 + last_q - c.k_pos0 + 1))
            assert k_end == int(vis[q0:last_q + 1].any(0).sum())
        if (c.q_pos0, c.k_pos0) == (0, 300):
            assert not vis.any() and c.tq > ec.XQ                           # k_end == 0 in both workgroups
        if (c.q_pos0, c.k_pos0, c.tq) == (0, 3, 8):
            assert vis.any(-1).tolist() == [False] * 3 + [True] * 5
    assert len({c.id for c in ec.ATTN}) == len(ec.ATTN)


def test_patchify_list_has_both_sides_of_the_vector_switch():
    vec = [c for c in ec.PATCH if c.vector_path]
    assert {c.ps for c in vec} == {8, 16, 24}
    rest = [c for c in ec.PATCH if not c.vector_path]
    assert any(c.ps == 16 and c.ld_eff > c.K for c in rest) and any(c.ps % 8 and c.ld_eff == c.K for c in rest) and any(c.ps == 14 for c in rest)
    assert all(c.ld_eff % 8 == 0 and c.ld_eff >= c.K for c in ec.PATCH)
    assert any(c.patches == 1 for c in ec.PATCH)


def test_bilinear_list_has_the_degenerate_sizes():
    plain = [c for c in ec.BIL if c.form == "plain"]
    assert any(c.h == 1 and c.w > 1 for c in plain) and any(c.w == 1 and c.h > 1 for c in plain)
    assert any(c.full == (1, 1) and c.h > 1 for c in plain) and any(c.full[0] < c.h and c.full[1] < c.w for c in plain)
    assert any(c.out == (1, 1) and c.full != (1, 1) for c in plain) and {8, 16, 24, 64} <= {c.C for c in plain}
    assert any(c.x2 for c in ec.BIL) and any(not c.x2 for c in plain)
    assert all(c.dtype == H16 for c in ec.BIL if c.form == "f8")


# ------------------------------------------------------------------------------------------------ rotary embedding and head widths
def test_a_rotary_embedding_cannot_meet_a_head_width_other_than_64():
    """rope_f32_kernel (and the QKV epilogue) rotate 64-wide heads, pairs (i, i + 16); f3r_attn_f32_ex takes eight widths.  The two meet in
    Fast3R._block_exact only for models whose blocks carry a rotary embedding: the CroCo encoder (RoPE-2D) and the Llama decoder (per view).
    Both constructors refuse another width; the Fast3R decoder, which takes any multiple of 16, has no rotary embedding."""
    with pytest.raises(ValueError, match="head_dim 64"):
        CroCoEncoder(img_size=64, embed_dim=160, num_heads=2, depth=1)
    with pytest.raises(ValueError, match="head_dim 64"):
        LlamaDecoder(False, 128, embed_dim=160, n_layers=1, n_heads=2)
