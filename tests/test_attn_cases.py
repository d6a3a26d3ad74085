"""tests/attn_cases.py without a GPU: the float64 references against a per-row softmax written out in Python, the case lists against what they
claim to cover (every form meets every edge class), the launch rules restated there against the figures csrc/f3r_attn_asm.hip documents, the zero
padding of V^T against ops.vt_ld, and the guarded placement against itself."""
import dataclasses
import math

import pytest
import torch

import attn_cases as ac
from attn_cases import BF16, CU_NOMINAL, H16
from fast3r_amd import ops

N_CU = CU_NOMINAL


def all_cases(n_cu=N_CU):
    return ac.STATIC + ac.asm_cases("asm512", n_cu) + ac.steal_cases(n_cu) + ac.split_cases(n_cu)


def by_form(n_cu=N_CU):
    out = {}
    for c in all_cases(n_cu):
        for form, _ in ac.forms(c, n_cu):
            out.setdefault(form, []).append(c)
    return out


# ------------------------------------------------------------------------------------------------ the references
def naive_row(q, k, v, log_scale, hidden=None):
    """one query row of one head: plain Python floats"""
    s = [sum(float(a) * float(b) for a, b in zip(q, kr)) * log_scale for kr in k]
    s = [x for j, x in enumerate(s) if not (hidden and hidden[j])]
    vv = [vr for j, vr in enumerate(v) if not (hidden and hidden[j])]
    m = max(s)
    p = [math.exp(x - m) for x in s]
    z = sum(p)
    return [sum(pj * float(vr[d]) for pj, vr in zip(p, vv)) / z for d in range(len(v[0]))]


@pytest.mark.parametrize("c", [ac.AttnCase(3, (5,), 64, H16, 2, 2), ac.AttnCase(4, (3, 0, 2), 16, BF16, 3, 1, 2, q_prescaled=False, scale=0.25),
                               ac.AttnCase(5, (2, 4), 64, H16, 2, 1, causal=True, q_pos0=3, seg_pos0=(2, 6)), ac.AttnCase(2, (7,), 48, H16, 4, 2, q_prescaled=False)],
                         ids=lambda c: c.id)
def test_reference_is_a_per_row_softmax(c):
    d = ac.build(c)
    ref = ac.reference(c, d)
    hd, ls = c.head_dim, (math.log(2.0) if c.q_prescaled else c.scale)
    pos = [p + i for p, n in zip(c.positions, c.segs) for i in range(n)]
    for b in range(c.batch):
        k = torch.cat([x[b] for x in d["k"]]).double().tolist()
        v = torch.cat([x[b] for x in d["v"]]).double().tolist()
        for r in range(c.tq):
            hidden = [p > c.q_pos0 + r for p in pos] if c.causal else None
            for h in range(c.n_heads):
                kv = h // c.kv_group
                want = naive_row(d["q"][b, r, h * hd:(h + 1) * hd].double().tolist(), [row[kv * hd:(kv + 1) * hd] for row in k],
                                 [row[kv * hd:(kv + 1) * hd] for row in v], ls, hidden)
                got = ref[b, r, h * hd:(h + 1) * hd].tolist()
                assert max(abs(a - w) for a, w in zip(got, want)) < 1e-12
    rows = torch.tensor([c.tq - 1, 0])
    assert torch.equal(ac.reference(c, d, rows), ref[:, rows])


@pytest.mark.parametrize("planes", [2, 3])
def test_reference_on_planes_is_a_per_row_softmax_of_the_kernels_products(planes):
    """rows as f3r_qkv_planes writes them, made here in Python: [hi 64 | lo 64] fp16, or [hi 64 fp16 | e4m3(hi) 64 B | e4m3(lo 2^12) 64 B]"""
    c = ac.AttnCase(3, (6,), 64, H16, 2, 2, qk_planes=planes)
    g = torch.Generator().manual_seed(5)

    def rows_of(x32, heads):
        n = x32.shape[0]
        hi = x32.to(H16)
        lo32 = x32 - hi.float()
        if planes == 2:
            lo = lo32.to(H16)
        else:
            b = torch.cat([ac.e4m3(hi.double()).float().to(torch.float8_e4m3fn).view(torch.uint8).reshape(n, heads, 64),
                           ac.e4m3(lo32.double() * 4096.0).float().to(torch.float8_e4m3fn).view(torch.uint8).reshape(n, heads, 64)], 2)
            lo = b.contiguous().view(H16).reshape(n, heads * 64)
        return torch.stack([hi.reshape(n, heads, 64), lo.reshape(n, heads, 64)], 2).reshape(n, heads * 128), hi, lo32

    q32, k32 = torch.randn((3, 128), generator=g), torch.randn((6, 64), generator=g)
    v = torch.randn((6, 64), generator=g).to(H16)
    qp, q_hi, q_lo = rows_of(q32, 2)
    kp, k_hi, k_lo = rows_of(k32, 1)
    got = ac.reference_planes(c, qp, kp, v)
    for r in range(3):
        for h in range(2):
            sl = slice(h * 64, (h + 1) * 64)
            if planes == 2:
                s = ((q_hi[r, sl].double() + q_lo[r, sl].to(H16).double()) * (k_hi.double() + k_lo.to(H16).double())).sum(1)
            else:
                s = ((q_hi[r, sl].double() * k_hi.double()).sum(1) + (ac.e4m3(q_lo[r, sl].double() * 4096.0) / 4096.0 * ac.e4m3(k_hi.double())).sum(1)
                     + (ac.e4m3(q_hi[r, sl].double()) * ac.e4m3(k_lo.double() * 4096.0) / 4096.0).sum(1))
            p = torch.exp2(s - s.max())
            want = (p[:, None] * v.double()).sum(0) / p.sum()
            assert float((got[r, sl] - want).abs().max()) < 1e-12


def test_exact_reference_is_a_per_row_softmax():
    c = ac.ExactCase(3, 5, 80, 2, 2, n_seq=2, causal=True, q_pos0=2, k_pos0=1)
    d = ac.build_exact(c)
    for z in range(2):
        for r in range(3):
            hidden = [c.k_pos0 + j > c.q_pos0 + r for j in range(5)]
            for h in range(2):
                want = naive_row(d["q"][z * 3 + r, h * 80:(h + 1) * 80].tolist(), d["k"][z * 5:(z + 1) * 5, :80].tolist(), d["v"][z * 5:(z + 1) * 5, :80].tolist(),
                                 80 ** -0.5, hidden)
                assert max(abs(a - w) for a, w in zip(d["ref"][z * 3 + r, h * 80:(h + 1) * 80].tolist(), want)) < 1e-12


# ------------------------------------------------------------------------------------------------ the lists
def test_every_case_is_legal_and_named_once():
    cases = all_cases()
    for c in cases:
        assert ac.legal(c) is None, (c.id, ac.legal(c))
        assert ac.forms(c, N_CU), c.id
    ids = [c.id for c in cases] + [c.id for c in ac.EXACT]
    assert len(ids) == len(set(ids))
    assert ac.legal(ac.CAUSAL_REFUSED) == "a fresh causal launch whose first key lies after its first query"


def test_every_case_runs_on_the_forms_it_is_there_for():
    """at the nominal CU count.  The 512-query form cannot take fewer than 257 rows under ANY heads x batch: one 256-query item per 512-query item
    at 0.64 of its time always wins (use_q256), so its tq = 128 / 129 cases run on the 256-query form; the emulator (test_attn_asm_emu.py) runs
    the 512-query generator at tq = 128."""
    for c in all_cases():
        listed = {f for f, _ in ac.forms(c, N_CU)}
        for f in c.forms:
            if f == "asm512" and c.tq <= 256:
                assert "q256" in listed and all(ac.use_q256(dataclasses.replace(c, n_heads=h), c.tq, n) for h in (4, 64, 132, 256, 1024) for n in (64, 256, 304))
            else:
                assert f in listed, (c.id, listed)


# (rows of a wave, rows of a workgroup) per form
ROWS = {"hip": (64, 256), "asm512": (128, 512), "q256": (64, 256), "d80": (64, 256), "d128": (64, 256), "qk3": (64, 256), "qk3f8": (64, 256)}


def test_every_form_meets_every_edge_class():
    forms = by_form()
    assert set(forms) >= {"hip", "hip-batched", "hip-causal", "generic", "asm512", "q256", "split", "d80", "d128", "qk3", "qk3f8", "cross"}
    for form, (wave, wg) in ROWS.items():
        tqs = {c.tq for c in forms[form] + (forms["hip-batched"] if form == "hip" else [])}
        assert {wg - 1, wg, wg + 1} <= tqs or (form != "hip" and {wg - 1, wg, wg + 1, 300} & tqs >= {wg - 1, wg, wg + 1}), (form, sorted(tqs))
        if form == "hip":
            assert {1, 31, 32, 33, wave - 1, wave, wave + 1, 127, 128, 129} <= tqs
        elif form != "asm512":      # (a hand-scheduled launch needs a wave's rows; the 512-query form more than 256: see above)
            assert {wave, wave + 1} <= tqs or {128, 129} <= tqs, (form, sorted(tqs))
    hand = ("asm512", "q256", "d80", "d128", "qk3", "qk3f8")
    for form in hand:
        cs = forms[form]
        assert {1, 2, 3, 5} <= {c.keys // 64 for c in cs if len(c.segs) == 1}, form
        assert any(0 in c.segs for c in cs) and any(len(c.segs) == 8 for c in cs), form
        assert any(c.ld("ldvt") >= ops.vt_ld(min(n for n in c.segs if n)) + 128 for c in cs), form      # columns a prefetch past a short segment would read
        assert any(c.batch > 1 and c.q_bs and c.o_bs and c.ldq and c.ldk and c.ldo and c.k_pad_rows and c.vt_pad_rows for c in cs), form
        assert any(c.state for c in cs) and {1, 2, 4} <= {c.kv_group for c in cs}, form
    assert any(c.state and c.batch == 3 for c in forms["qk3"]) and any(c.state and c.batch == 3 for c in forms["qk3f8"])
    hip = forms["hip"] + forms["hip-batched"]
    assert set(ac.HIP_KEYS) <= {c.keys for c in hip if len(c.segs) == 1}
    for dt in (H16, BF16):
        sub = [c for c in hip if c.dtype == dt]
        assert {c.segs for c in sub} >= set(ac.HIP_SEGS)
        assert {True, False} == {c.q_prescaled for c in sub} and {1, 2, 3} <= {c.kv_group for c in sub} and {1, 3} <= {c.n_heads for c in sub}
        assert {c.state[1] for c in sub if c.state} == {1, 2}
        assert any(c.batch == 3 and c.ldq and c.ldk and c.ldo and c.q_bs and c.o_bs and c.ld("ldvt") == ops.vt_ld(max(c.segs)) + 64 for c in sub)
    assert len(ac.HIP_SEGS[-1]) == ac.MAX_SEG and min(ac.HIP_SEGS[-1]) == 1 and max(ac.HIP_SEGS[-1]) == 65
    gen = forms["generic"]
    for hd in ac.GENERIC_HDS:
        sub = [c for c in gen if c.head_dim == hd and not c.cross]
        assert {c.tq for c in sub} >= set(ac.GENERIC_TQ), hd
        assert any(0 in c.segs for c in sub) and any(c.state for c in sub) and any(c.batch > 1 and c.ldq and c.q_bs for c in sub) and any(c.kv_group > 1 for c in sub)
    assert {48, 112} <= {c.head_dim for c in gen}
    assert {c.keys for c in gen if len(c.segs) == 1} >= set(ac.GENERIC_KEYS)
    cau = forms["hip-causal"]
    assert {c.tq for c in cau if c.q_pos0 == 0 and not c.state and c.tq == c.keys} >= set(ac.CAUSAL_T)
    assert any(c.tq != c.keys and c.q_pos0 == c.keys - c.tq for c in cau)
    assert {c.q_pos0 for c in cau if c.state} == {0, 63, 64, 65}
    assert {(c.head_dim, c.cross) for c in forms["cross"]} == {(hd, x) for hd in (64, 80, 128) for x in ((1, 2), (2, 1))}


def test_exact_cases_cover_their_edges():
    for mfma in (False, True):
        sub = [c for c in ac.EXACT if c.mfma == mfma and not c.causal]
        assert {c.tq for c in sub} >= set(ac.EXACT_T) and {c.tk for c in sub} >= set(ac.EXACT_T) and {c.kv_group for c in sub} == {1, 2}
    assert all(c.head_dim == 64 and not c.causal for c in ac.EXACT if c.mfma)
    fma = [c for c in ac.EXACT if not c.mfma]
    assert {c.head_dim for c in fma} == {64, 80} and any(c.causal and c.q_pos0 for c in fma) and any(c.causal and c.k_pos0 for c in fma)
    assert {c.tq for c in fma if c.causal and c.tq == c.tk} >= set(ac.EXACT_T)


# ------------------------------------------------------------------------------------------------ the launch rules
def _shape(tq, h, b=1, hd=64):
    return ac.AttnCase(tq, (2048,), hd, H16, h, 1, b)


@pytest.mark.parametrize("tq,h,expect", [(3072, 16, "q256"), (20480, 16, "split"), (8192, 16, "asm512"), (40960, 16, "asm512"), (3000, 5, "q256"), (4096, 16, "q256"),
                                         (6144, 16, "asm512"), (20480 - 300, 16, "split"), (20480 + 300, 16, "asm512"), (24576, 16, "asm512"), (102400, 16, "asm512"),
                                         (50 * 512, 16, "split"), (9 * 512, 32, "split")])
def test_restated_rules_give_the_forms_the_library_is_tested_for(tq, h, expect):
    """the shapes and forms of tests/test_attn_asm_gpu.py::test_small_launches_take_256_query_work_items, on 256 CUs"""
    assert ac.asm_form(_shape(tq, h), 256) == expect


def test_the_split_gives_no_launch_fewer_rows_than_a_wave():
    """tq = g 512 + r at heads x batch = 16: the last block alone is the tail.  Below 64 rows the 256-query form cannot take it (its waves clamp
    their first row with tq - 64, which wraps): the rule now keeps ONE launch there, and without that check (guarded=False) it split"""
    for n_cu in (256, 304, 64):
        assert ac.split_possible(n_cu)
        for c in ac.split_cases(n_cu):
            r = c.tq - ac.split_g(n_cu) * 512
            assert c.n_heads * c.batch == 16 and r in ac.SPLIT_R and c.keys in (64, 128)
            assert (ac.tail_split_rows(c, n_cu) > 0) == (r >= 64), (n_cu, c.id)
            assert ac.tail_split_rows(c, n_cu, guarded=False) == ac.split_g(n_cu) * 512
            assert (c.forms == ("split",)) == (r >= 64) and c.forms[0] in ("split", "asm512", "q256")
    # every launch the rules derive has a wave's rows, whatever the shape
    for n_cu in (256, 304):
        for hb in (1, 3, 16, 24, 48, 100):
            for tq in list(range(128, 700)) + [512 * k + r for k in (4, 16, 17, 19, 33) for r in (1, 63, 64, 127, 128, 200)]:
                c = _shape(tq, hb)
                rows = ac.tail_split_rows(c, n_cu)
                if rows:
                    tail = tq - rows
                    assert rows % 512 == 0 and not ac.use_q256(c, rows, n_cu) and tail >= (64 if ac.use_q256(c, tail, n_cu) else 128)


def test_steal_cases_are_the_smallest_that_steal():
    for n_cu in (256, 304):
        for c in ac.steal_cases(n_cu):
            assert ac.steals(c, n_cu) and ac.asm_form(c, n_cu) == c.forms[0]
            wg = 4 * ac.wave_rows(c)
            assert not ac.steals(dataclasses.replace(c, tq=c.tq - wg), n_cu)


# ------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_vt_image_is_zero_padded_to_vt_ld(n):
    c = ac.AttnCase(8, (n, 192), 80, BF16, 2, 2, 2, ldvt=320)
    v = ac.build(c)["v"][0]
    img = ac.vt_image(v, c)
    assert img.shape == (2, 80, 320) and ops.vt_ld(n) == -(-n // 64) * 64
    assert torch.equal(img[:, :, :n], v.transpose(1, 2))
    assert not img[:, :, n:ops.vt_ld(n)].any()
    assert bool((img[:, :, ops.vt_ld(n):].contiguous().view(torch.uint8) == 0xFF).all())


def test_guarded_placement_round_trips():
    t = torch.randn((3, 5, 16)).to(H16)
    view, buf = ac.place(t, 24, 5 * 24 + 48, "cpu", 7)
    assert torch.equal(view, t) and view.stride() == (168, 24, 1) and view.data_ptr() % 16 == 0
    view.view(torch.int16).zero_()
    assert int((buf == 0).sum()) == 3 * 5 * 16 * 2 and int((buf == 0xFF).sum()) == buf.numel() - 3 * 5 * 16 * 2   # everything but the values is a NaN pattern
    lead = (view.data_ptr() - buf.data_ptr()) // 2
    assert lead >= 7 * 24 and buf.numel() // 2 - lead - (2 * 168 + 4 * 24 + 16) >= 7 * 24    # a margin of 7 rows on either side
    one, b1 = ac.place(t[:1], 16, 0, "cpu", 2)
    rows, b2 = ac.guarded_rows(t[0], 16, "cpu")                    # the tight single-sequence form is gemm_cases' placement
    assert torch.equal(one[0], rows) and torch.equal(b1, b2)
    for dtype in (H16, torch.float32):
        g = ac.place_out(3, 5, 16, 24, 5 * 24 + 48, dtype, "cpu", 7)
        assert g.view.shape == (3, 5, 16) and ac.out_intact(g) and ac.untouched(g)
        g.view.fill_(1.0)
        assert ac.out_intact(g) and not ac.untouched(g)
        for where in (g.lead - 1, g.lead + 16, g.lead + 5 * 24, g.lead + 2 * 168 + 5 * 24):   # margin, gap column, a row between sequences, behind
            saved = int(g.buf[where])
            g.buf[where] = 0
            assert not ac.out_intact(g), where
            g.buf[where] = saved
        assert ac.out_intact(g)
    g = ac.place_out(1, 5, 16, 24, 0, H16, "cpu", 3)
    assert ac.out_intact(g) and ac.guards_intact(g)
    g.buf[g.lead + 17] = 0
    assert not ac.out_intact(g) and not ac.guards_intact(g)
