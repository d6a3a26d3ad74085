"""The attention family at the edges of its geometry, on a real MI355X through the C ABI: f3r_attn_fwd on every kernel form -- the HIP head_dim-64
kernel (plain, batched, causal), the generic kernel at every built head_dim, the hand-scheduled kernels (512- and 256-query items, the split of
the last round, work stealing, head_dim 80 / 128, the three-product forms) -- and the exact mode's f3r_attn_f32_ex / f3r_attn_f32_mfma, with tq
and the key counts next to every tile, wave and workgroup boundary, row and batch strides wider than what they span, empty and one-key segments,
and the softmax state parked and resumed at every cut (cases, float64 references and the restated launch rules: tests/attn_cases.py).

Every case runs on every form attn_cases.forms lists for it at this device's CU count; f3r_attn_kernel_name must name that form BEFORE the launch
goes out, and a form the library refuses is a failure, never a skip.  Every operand lies inside a buffer of NaN patterns and every output inside a
buffer of sentinel words, with a margin of a whole work item on either side (attn_cases: guarded placement): a load outside the planes poisons
the result, a store outside rows [0, tq) x the heads' columns changes a sentinel.  The guards are asserted before any value is compared.

Tolerances are the ones the project already holds these kernels to: 2 lp_tol for one-plane kernels (test_kernels_gpu.py, test_attn_asm_gpu.py),
2^-9 for the three-product kernels against their planes and 2^-10 between their one- and two-launch forms (test_robust_gpu.py), 3e-6 rel-L2 for
the exact kernels (docs/parity.md); bit equality for one launch against park + resume on the HIP and generic kernels and for work stealing
against the static launch."""
import ctypes

import pytest
import torch

import attn_cases as ac
from attn_cases import H16
from fast3r_amd import _lib, ops
from test_kernels_gpu import DEV, lp_tol

pytestmark = pytest.mark.gpu


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def check(kind, got, ref, tol, what, missed):
    """test_kernels_gpu.assert_close with the figure printed before it is judged; a miss is collected"""
    got, ref = got.detach().double().cpu(), ref.double()
    scale = float(ref.abs().max().clamp_min(1e-6))
    err = float((got - ref).abs().max())
    print(f"[attn-geometry] kind={kind} rel_err={err / scale:.3e} tol={tol:.1e} {what}")
    if not (err == err and err <= tol * scale):
        missed.append(f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol:.1e})")


def check_l2(kind, got, ref, tol, what, missed):
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    err = float((got - ref).norm() / ref.norm().clamp_min(1e-30))
    print(f"[attn-geometry] kind={kind} rel_err={err:.3e} tol={tol:.1e} {what}")
    if not (err == err and err <= tol):
        missed.append(f"{what}: rel-L2 {err:.3e} (tol {tol:.1e})")


class Launcher:
    """the operands of a case in guarded placement, its float64 reference, and launches of it through f3r_attn_fwd"""

    def __init__(self, c):
        self.c, self.keep = c, []
        d = ac.build(c)
        if c.qk_planes >= 2:
            d = self._planes(d)
        self.q = self._place(d["q"], c.ld("ldq"), c.bs("q"), ac.MARGIN_ROWS)
        self.k, self.vt = [], []
        for k, v, n in zip(d["k"], d["v"], c.segs):
            if n == 0:     # never read: one row of NaN patterns
                k = torch.full((c.batch, 1, c.k_width), float("nan"), dtype=c.dtype)
            self.k.append(self._place(k, c.ld("ldk"), c.bs("k"), ac.K_MARGIN_ROWS))
            self.vt.append(self._place(ac.vt_image(v, c), c.ld("ldvt"), c.bs("vt"), ac.VT_MARGIN_ROWS))
        # big launches: the last 600 rows and 64 sampled rows of the rest
        self.rows = None
        if c.tq > 2000:
            g = torch.Generator().manual_seed(c.tq)
            self.rows = torch.cat([torch.randperm(c.tq - 600, generator=g)[:64].sort().values, torch.arange(c.tq - 600, c.tq)])
        if c.qk_planes >= 2:
            self.ref = torch.stack([ac.reference_planes(c, d["q"][b], torch.cat([k[b] for k in d["k"]]), torch.cat([v[b] for v in d["v"]])) for b in range(c.batch)])
        else:
            self.ref = ac.reference(c, d, self.rows)

    def _place(self, t, ld, bs, margin):
        view, buf = ac.place(t, ld, bs, DEV, margin)
        self.keep.append(buf)
        return view

    def _planes(self, d):
        """q and K rows as f3r_qkv_planes writes them (the values of build(c) are already scaled: q_scale 1), V rounded to fp16 -- read back to the
        CPU, where the reference is computed from the planes themselves and the guarded images are made"""
        c = self.c
        H, kvh = c.n_heads, c.kv_heads

        def planes(q, k, v, seq_len):
            rows = c.batch * seq_len
            z = lambda x, w: torch.zeros((rows, w)) if x is None else x.reshape(rows, w)   # noqa: E731
            qkv = torch.cat([z(q, H * 64), z(k, kvh * 64), z(v, kvh * 64)], 1).to(DEV)
            qp, kp, vt = ops.qkv_planes(qkv, H, kvh, c.batch, seq_len, 1.0, c.dtype, planes=c.qk_planes)
            return qp.cpu().view(c.batch, seq_len, H * 128), kp.cpu().view(c.batch, seq_len, kvh * 128), vt.cpu()[:, :, :seq_len].transpose(1, 2).contiguous()

        out = dict(q=planes(d["q"], None, None, c.tq)[0], k=[], v=[])
        for k, v, n in zip(d["k"], d["v"], c.segs):
            if n == 0:
                out["k"].append(torch.zeros((c.batch, 0, kvh * 128), dtype=c.dtype))
                out["v"].append(torch.zeros((c.batch, 0, kvh * 64), dtype=c.dtype))
                continue
            _, kp, v16 = planes(None, k, v, n)
            out["k"].append(kp)
            out["v"].append(v16)
        return out

    def out(self):
        c = self.c
        return ac.place_out(c.batch, c.tq, c.o_width, c.ld("ldo"), c.bs("o"), c.dtype, DEV)

    def state(self):
        c = self.c
        T = c.batch * c.tq
        return (ac.place_out(1, T, c.o_width, c.o_width, 0, torch.float32, DEV), ac.place_out(1, T, c.n_heads * 4, c.n_heads * 4, 0, torch.float32, DEV))

    def launch(self, sel, o, expect, segs=None, state=None, state_in=False, state_out=False, refused=None):
        """f3r_attn_kernel_name first -- it must name `expect` -- then f3r_attn_fwd over the segments `segs` (default: all)"""
        c = self.c
        idx = list(range(len(c.segs))) if segs is None else list(segs)
        a = _lib.AttnArgs()
        a.q, a.o = _lib.ptr(self.q), _lib.ptr(o.view)
        a.ldq, a.ldo, a.q_batch_stride, a.o_batch_stride = c.ld("ldq"), c.ld("ldo"), c.bs("q"), c.bs("o")
        a.tq, a.batch, a.n_heads, a.n_seg, a.dtype = c.tq, c.batch, c.n_heads, len(idx), _lib.dtype_id(c.dtype)
        for i, s in enumerate(idx):
            a.k_seg[i], a.vt_seg[i], a.seg_len[i], a.ldvt[i] = _lib.ptr(self.k[s]), _lib.ptr(self.vt[s]), c.segs[s], c.ld("ldvt")
            a.k_batch_stride[i], a.vt_batch_stride[i], a.seg_pos0[i] = c.bs("k"), c.bs("vt"), c.positions[s]
        a.ldk, a.scale, a.q_prescaled = c.ld("ldk"), c.scale, int(c.q_prescaled)
        a.kv_group, a.causal, a.q_pos0 = c.kv_group, int(c.causal), c.q_pos0
        a.kernel_sel, a.head_dim, a.qk_planes = sel, c.head_dim, c.qk_planes
        if state is not None:
            a.st_o, a.st_ml, a.state_in, a.state_out = _lib.ptr(state[0].view), _lib.ptr(state[1].view), int(state_in), int(state_out)
        if ops.ATTN_WORK_STEALING:
            a.sched_counter = _lib.ptr(ops._sched_counter(self.q.device))
        name = _lib.lib().f3r_attn_kernel_name(ctypes.byref(a)).decode()
        assert expect in name, f"{c.id} kernel_sel={sel}: f3r_attn_kernel_name says {name!r}, the restated launch rule expects {expect!r}"
        rc = _lib.lib().f3r_attn_fwd(ctypes.byref(a), _lib.stream_ptr())
        if refused is not None:
            assert rc == -1 and refused in _lib.lib().f3r_last_error_string().decode(), (rc, _lib.lib().f3r_last_error_string())
            return name
        _lib.check(rc, f"f3r_attn_fwd({c.id}, kernel_sel={sel})")
        torch.cuda.synchronize()
        return name

    def got(self, o):
        return o.view if self.rows is None else o.view[:, self.rows.to(DEV)]


def _expect(form, c):
    return ac.expected_name(form, c)


def _sel_form(c, sel, n_cu):
    return ac.hip_form(c) if sel == 1 else ac.asm_form(c, n_cu)


def _finish(L, st):
    """the parked state -> O as the sum of the hi + lo planes f3r_attn_state_finish writes (what the three-product kernels' callers read)"""
    c = L.c
    T = c.batch * c.tq
    hi, lo = ops.attention_state_finish((st[0].view[0], st[1].view[0].view(T, c.n_heads, 4)), c.n_heads, c.head_dim, c.dtype)
    torch.cuda.synchronize()
    return (hi.double() + lo.double()).view(c.batch, c.tq, c.o_width)


def _state_intact(st, what):
    assert ac.out_intact(st[0]), f"{what}: a store outside the st_o rows"
    assert ac.out_intact(st[1]), f"{what}: a store outside the st_ml rows"


def run_form(L, form, sel, n_cu, missed):
    c = L.c
    dt = ac._dt(c.dtype)
    tol = 2 * lp_tol(c.dtype)
    if c.cross:
        s1, s2 = c.cross
        f1, f2 = _sel_form(c, s1, n_cu), _sel_form(c, s2, n_cu)
        what = f"{c.id} {f1} -> {f2}"
        cut = c.state[1]
        o, st = L.out(), L.state()
        L.launch(s1, o, _expect(f1, c), range(cut), st, state_out=True)
        assert ac.untouched(o), f"{what}: the parking launch wrote o"
        _state_intact(st, what)
        L.launch(s2, o, _expect(f2, c), range(cut, len(c.segs)), st, state_in=True)
        assert ac.out_intact(o), f"{what}: a store outside the {c.batch} x {c.tq} x {c.o_width} outputs"
        _state_intact(st, what)
        check(f"cross-{f1}-{f2}-{dt}", L.got(o), L.ref, tol, what, missed)
        return
    what = f"{c.id} on {form}"
    expect = _expect(form, c)
    if c.qk_planes >= 2:    # the three-product kernels' callers always park the state and read O from f3r_attn_state_finish
        o, st = L.out(), L.state()
        L.launch(sel, o, expect, None, st, state_out=True)
        assert ac.untouched(o), f"{what}: a launch with state_out wrote o"
        _state_intact(st, what)
        one = _finish(L, st)
        check(f"{form}-state-{dt}", one, L.ref, 2.0 ** -9, what, missed)
        if c.state:
            cut = c.state[1]
            st2 = L.state()
            L.launch(sel, o, expect, range(cut), st2, state_out=True)
            _state_intact(st2, what + " parked")
            L.launch(sel, o, expect, range(cut, len(c.segs)), st2, state_in=True, state_out=True)
            assert ac.untouched(o), f"{what}: a launch with state_out wrote o"
            _state_intact(st2, what + " resumed")
            two = _finish(L, st2)
            check(f"{form}-resumed-{dt}", two, L.ref, 2.0 ** -9, what + " park + resume", missed)
            check(f"{form}-resumed-vs-one-{dt}", two, one.cpu(), 2.0 ** -10, what + " park + resume against one launch", missed)
        return
    o = L.out()
    name = L.launch(sel, o, expect)
    assert ac.out_intact(o), f"{what} ({name}): a store outside the {c.batch} x {c.tq} x {c.o_width} outputs (row stride {c.ld('ldo')})"
    check(f"{form}-{dt}", L.got(o), L.ref, tol, what, missed)
    if L.rows is not None:
        assert bool(torch.isfinite(o.view.float()).all()), f"{what}: a row nobody computed"
    if c.state:
        cut = c.state[1]
        o2, st = L.out(), L.state()
        L.launch(sel, o2, expect, range(cut), st, state_out=True)
        assert ac.untouched(o2), f"{what}: the parking launch wrote o"
        _state_intact(st, what + " parked")
        L.launch(sel, o2, expect, range(cut, len(c.segs)), st, state_in=True)
        assert ac.out_intact(o2), f"{what}: the resumed launch stored outside the outputs"
        _state_intact(st, what + " resumed")
        check(f"{form}-resumed-{dt}", L.got(o2), L.ref, tol, what + " park + resume", missed)
        if sel == 1 and not c.causal:   # the HIP and generic kernels: same tiles in the same order, the state kept in fp32 (test_attention_state_carried_across_launches)
            assert torch.equal(o.view, o2.view), f"{what}: park + resume differs from one launch"
    return o


def run_case(c, n_cu=None):
    n_cu = n_cu or n_cus()
    listed = ac.forms(c, n_cu)
    assert listed, c.id
    for f in c.forms:
        if f not in [x for x, _ in listed]:
            print(f"[attn-geometry] {c.id}: form {f} cannot occur at tq={c.tq} on {n_cu} CUs, the launch rule takes {[x for x, _ in listed]}")
    L = Launcher(c)
    missed = []
    for form, sel in listed:
        run_form(L, form, sel, n_cu, missed)
    assert not missed, "; ".join(missed)


# ------------------------------------------------------------------------------------------------ the cases that do not depend on the device
@pytest.mark.parametrize("c", ac.HIP, ids=lambda c: c.id)
def test_hip_head_dim_64(built_lib, c):
    """attn_kernel and attn_kernel<batched>: tq next to a query block, a wave's and a workgroup's rows; one to 191 keys (clamped K rows, the zero
    padding of V^T); scaled and pre-scaled q; grouped heads; empty and one-key segments; wide strides; park and resume at every cut"""
    run_case(c)


@pytest.mark.parametrize("c", ac.CAUSAL, ids=lambda c: c.id)
def test_causal_head_dim_64(built_lib, c):
    """attn_kernel<causal>: the diagonal inside one tile and across tiles, queries that are the last rows of a longer sequence, and the sharded
    form -- the rank's own shard first (parked), the other shards resumed -- with shard edges at 63, 64 and 65"""
    run_case(c)


def test_causal_launch_whose_first_key_is_hidden_is_refused(built_lib):
    """a fresh causal launch must see its first key from every row (f3r.h): the kernel's first softmax reference comes from tile 0"""
    c = ac.CAUSAL_REFUSED
    L = Launcher(c)
    o = L.out()
    L.launch(1, o, "attn_kernel<causal>", refused="lies after its first query")
    torch.cuda.synchronize()
    assert ac.untouched(o)


@pytest.mark.parametrize("c", ac.GENERIC, ids=lambda c: c.id)
def test_generic_kernel(built_lib, c):
    """attn_generic_kernel at every built head_dim (48 and 112 run nowhere else): both workgroup sizes, partial key tiles, an empty segment,
    grouped heads, park and resume, a batch with wide strides"""
    run_case(c)


@pytest.mark.parametrize("c", ac.ASM_STATIC, ids=lambda c: c.id)
def test_hand_scheduled_forms(built_lib, c):
    """f3r_attn_asm_q256_*, _d80_*, _d128_*, _qk3_f16 and _qk3f8_f16 (and the HIP / generic kernel on the same guarded operands): a wave's rows,
    a workgroup's rows and one more; 1, 2, 3 and 5 key tiles; segments with an empty one, eight segments, a 64-key segment under ldvt = 256; grouped
    heads; a batch with wide strides; park and resume"""
    run_case(c)


N_ASM512 = len(ac.asm_cases("asm512"))


@pytest.mark.parametrize("i", range(N_ASM512), ids=[f"{i}-q{c.tq}-k{'_'.join(map(str, c.segs))}-b{c.batch}" for i, c in enumerate(ac.asm_cases("asm512"))])
def test_hand_scheduled_512_query_form(built_lib, i):
    """f3r_attn_asm_*: heads x batch come from the CU count so that the launch rule keeps 512-query items (more than half a round of them).  Up to
    256 rows the rule takes the 256-query form whatever the heads: those cases run on it (printed)"""
    run_case(ac.asm_cases("asm512", n_cus())[i])


@pytest.mark.parametrize("c", ac.CROSS, ids=lambda c: c.id)
def test_state_parked_by_one_kernel_is_resumed_by_another(built_lib, c):
    """f3r.h promises ONE state layout: HIP <-> hand-scheduled at head_dim 64, generic <-> _d80 / _d128"""
    run_case(c)


# ------------------------------------------------------------------------------------------------ work stealing, the split of the last round
@pytest.mark.parametrize("i", range(len(ac.steal_cases())), ids=[f"{i}-hd{c.head_dim}" for i, c in enumerate(ac.steal_cases())])
def test_work_stealing_against_the_static_launch(built_lib, i):
    """the smallest launch that runs as persistent workgroups (two rounds of them on this device): bit for bit the static launch's output"""
    n_cu = n_cus()
    c = ac.steal_cases(n_cu)[i]
    assert ac.steals(c, n_cu) and ops.ATTN_WORK_STEALING
    form = ac.asm_form(c, n_cu)
    assert (form,) == c.forms
    L = Launcher(c)
    missed = []
    stolen = run_form(L, form, 2, n_cu, missed)
    ops.ATTN_WORK_STEALING = False
    try:
        static = run_form(L, form, 2, n_cu, missed)
    finally:
        ops.ATTN_WORK_STEALING = True
    assert torch.equal(stolen.view.view(torch.int16), static.view.view(torch.int16)), f"{c.id}: work stealing and the static launch differ"
    assert not missed, "; ".join(missed)


N_SPLIT = len(ac.split_cases())


@pytest.mark.parametrize("i", range(N_SPLIT), ids=[f"{i}-r{ac.SPLIT_R[i // 2]}-k{(64, 128)[i % 2]}" for i in range(N_SPLIT)])
def test_split_of_the_last_round(built_lib, i):
    """tq = g 512 + r at heads x batch = 16: from r = 64 on the last block goes out as a second launch on 256-query items; below, a wave of that
    form would take more rows than the launch has, and the launch stays one.  f3r_attn_kernel_name must agree with the restated rule before
    anything is launched; the float64 reference covers the last 600 rows and 64 sampled rows of the main part, the guards everything."""
    n_cu = n_cus()
    if not ac.split_possible(n_cu):
        print(f"[attn-geometry] the last-round split cannot occur at heads x batch = 16 on {n_cu} CUs")
        pytest.skip(f"no split of the last round at heads x batch = 16 on {n_cu} CUs")
    c = ac.split_cases(n_cu)[i]
    r = c.tq - ac.split_g(n_cu) * 512
    assert (c.forms == ("split",)) == (r >= 64)
    L = Launcher(c)
    missed = []
    run_form(L, c.forms[0], 2, n_cu, missed)     # (the name "... for the last round" is asserted, or asserted absent, before the launch)
    assert not missed, "; ".join(missed)


# ------------------------------------------------------------------------------------------------ the exact mode
@pytest.mark.parametrize("c", ac.EXACT, ids=lambda c: c.id)
def test_exact_mode_kernels(built_lib, c):
    """f3r_attn_f32_ex (head_dim 64 and 80, causal by q_pos0 / k_pos0) and f3r_attn_f32_mfma, called directly: q, k and v as three separate fp32
    tensors between NaN patterns with wide row strides, the three outputs between sentinels"""
    d = ac.build_exact(c)
    D, Dk = c.n_heads * c.head_dim, c.n_heads // c.kv_group * c.head_dim
    wide = (c.tq + c.tk) % 2 == 0
    ldq, ldkv, ldo = (D + 4, Dk + 8, D + 4) if wide else (D, Dk, D)
    keep = []

    def put(t, ld, margin):
        view, buf = ac.place(t[None], ld, 0, DEV, margin)
        keep.append(buf)
        return view

    q, k, v = put(d["q"], ldq, ac.MARGIN_ROWS), put(d["k"], ldkv, 256), put(d["v"], ldkv, 256)
    T = c.n_seq * c.tq
    o_hi, o_lo, o32 = (ac.place_out(1, T, D, ldo, 0, dt, DEV) for dt in (c.dtype, c.dtype, torch.float32))
    a = _lib.AttnF32Args()
    a.q, a.k, a.v, a.ldq, a.ldkv = _lib.ptr(q), _lib.ptr(k), _lib.ptr(v), ldq, ldkv
    a.o_hi, a.o_lo, a.o_f32, a.ldo = _lib.ptr(o_hi.view), _lib.ptr(o_lo.view), _lib.ptr(o32.view), ldo
    a.n_seq, a.tq, a.tk, a.q_pos0, a.k_pos0 = c.n_seq, c.tq, c.tk, c.q_pos0, c.k_pos0
    a.n_heads, a.kv_group, a.causal, a.dtype, a.head_dim, a.scale = c.n_heads, c.kv_group, int(c.causal), _lib.dtype_id(c.dtype), c.head_dim, d["scale"]
    if c.mfma:
        nbytes = int(_lib.lib().f3r_attn_f32_mfma_workspace(ctypes.byref(a)))
        assert nbytes > 0, c.id
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        _lib.check(_lib.lib().f3r_attn_f32_mfma(ctypes.byref(a), _lib.ptr(ws), nbytes, _lib.stream_ptr()), "f3r_attn_f32_mfma")
    else:
        _lib.check(_lib.lib().f3r_attn_f32_ex(ctypes.byref(a), _lib.stream_ptr()), "f3r_attn_f32_ex")
    torch.cuda.synchronize()
    for name, g in (("o_hi", o_hi), ("o_lo", o_lo), ("o_f32", o32)):
        assert ac.out_intact(g), f"{c.id}: a store outside the {T} x {D} rows of {name} (row stride {ldo})"
    missed = []
    kind = f"exact-{'mfma' if c.mfma else 'fma'}"
    check_l2(f"{kind}-f32", o32.view[0], d["ref"], 3e-6, c.id, missed)
    planes = o_hi.view[0].double() + o_lo.view[0].double()
    check_l2(f"{kind}-planes-{ac._dt(c.dtype)}", planes, o32.view[0], 2e-6 if c.dtype == H16 else 1e-4, c.id + " hi + lo against the fp32 output", missed)   # test_exact_mfma_gpu.py
    assert not missed, "; ".join(missed)
