"""f3r_attn_asm_{f16,bf16}_grp on a real MI355X through the C ABI: from F3R_ATTN_GROUPED_MIN_KEYS keys on, a head_dim-64 launch on 512-query items
meets at one s_barrier per group of key tiles on an 8-slot LDS ring (csrc/asm/attn_gen.py, "The LDS ring"; tests/test_attn_grouped_emu.py holds the
instruction stream bit for bit to the one-barrier-per-tile kernel in the emulator).  Here: the launch rule at the threshold -- the name
f3r_attn_kernel_name gives BEFORE the launch goes out -- every remainder of the tile count mod the group, a ring that wraps, segments with an
empty one, a batch with wide strides, park and resume, partial workgroups, and the work-stealing form.

Cases, guarded placement and the float64 reference are tests/attn_cases.py's; the bar is the one tests/test_attn_geometry_gpu.py holds the 512-query
form to (2 lp_tol on the largest reference value); guards are asserted before any value is compared; kernel_sel 0 and 2 must agree bit for bit.
The reference covers every head on the first and last rows of the launch (the re-aimed waves of a partial workgroup) and a sample of the rest."""
import os
import re

import pytest
import torch

import attn_cases as ac
from attn_cases import AttnCase, BF16, H16
from fast3r_amd import ops
from test_attn_geometry_gpu import Launcher, check
from test_kernels_gpu import lp_tol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "f3r.h")) as _f:
    TH = int(re.search(r"#define\s+F3R_ATTN_GROUPED_MIN_KEYS\s+(\d+)", _f.read()).group(1))
GRP = "f3r_attn_asm_{dt}_grp (hand-scheduled"
PLAIN = ac.FORM_NAMES["asm512"]


def n_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def group():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "fast3r_amd", "csrc", "asm"))
    import attn_gen
    return attn_gen.GROUPED_RING["tiles_per_barrier"]


class SampledLauncher(Launcher):
    """Launcher with the float64 reference on a sample of the query rows at any tq (all heads)"""

    def __init__(self, c):
        self.c, self.keep = c, []
        d = ac.build(c)
        self.q = self._place(d["q"], c.ld("ldq"), c.bs("q"), ac.MARGIN_ROWS)
        self.k, self.vt = [], []
        for k, v, n in zip(d["k"], d["v"], c.segs):
            if n == 0:     # never read: one row of NaN patterns
                k = torch.full((c.batch, 1, c.k_width), float("nan"), dtype=c.dtype)
            self.k.append(self._place(k, c.ld("ldk"), c.bs("k"), ac.K_MARGIN_ROWS))
            self.vt.append(self._place(ac.vt_image(v, c), c.ld("ldvt"), c.bs("vt"), ac.VT_MARGIN_ROWS))
        # 16 to 64 rows, as many as keep the float64 score matrix of all heads near 48 M elements: the first rows, the last ones, a sample between
        n = max(16, min(64, int(48e6 // (c.keys * c.n_heads * c.batch))))
        first, last = n // 8, n // 2
        g = torch.Generator().manual_seed(c.tq)
        mid = first + torch.randperm(c.tq - first - last, generator=g)[:n - first - last].sort().values
        self.rows = torch.cat([torch.arange(first), mid, torch.arange(c.tq - last, c.tq)])
        self.ref = ac.reference(c, d, self.rows)


def every_row_written(o):
    """no output row still holds nothing but sentinel words"""
    return not bool((o.view.view(torch.int16) == ac.SENTINEL).all(-1).any())


def run(c, expect, expect_resume=None):
    dt = ac._dt(c.dtype)
    assert ac.legal(c) is None and ac.asm_eligible(c), c.id
    L = SampledLauncher(c)
    tol = 2 * lp_tol(c.dtype)
    missed = []
    what = f"{c.id} on {expect.format(dt=dt)}"
    if c.state:
        cut = c.state[1]
        o, st = L.out(), L.state()
        L.launch(2, o, expect.format(dt=dt), range(cut), st, state_out=True)
        assert ac.untouched(o), f"{what}: the parking launch wrote o"
        assert ac.out_intact(st[0]) and ac.out_intact(st[1]), f"{what}: a store outside the state rows (parked)"
        L.launch(2, o, (expect_resume or expect).format(dt=dt), range(cut, len(c.segs)), st, state_in=True)
        assert ac.out_intact(o), f"{what}: the resumed launch stored outside the outputs"
        assert ac.out_intact(st[0]) and ac.out_intact(st[1]), f"{what}: a store outside the state rows (resumed)"
        assert every_row_written(o), f"{what}: a row nobody computed"
        check(f"grp-resumed-{dt}", L.got(o), L.ref, tol, what + " park + resume", missed)
        assert not missed, "; ".join(missed)
        return None
    outs = {}
    for sel in (2, 0):
        o = L.out()
        name = L.launch(sel, o, expect.format(dt=dt))
        assert ac.out_intact(o), f"{what} ({name}, kernel_sel {sel}): a store outside the {c.batch} x {c.tq} x {c.o_width} outputs (row stride {c.ld('ldo')})"
        assert every_row_written(o), f"{what}: a row nobody computed"
        outs[sel] = o
    check(f"grp-{dt}", L.got(outs[2]), L.ref, tol, what, missed)
    assert torch.equal(outs[0].view.view(torch.int16), outs[2].view.view(torch.int16)), f"{what}: kernel_sel 0 and kernel_sel 2 differ"
    assert not missed, "; ".join(missed)
    return outs[2]


def heads(tq, batch=1):
    return ac.heads_for_512(tq, n_cus(), batch)


def test_threshold_is_a_whole_number_of_tiles_at_or_above_4096_keys():
    assert TH >= 4096 and TH % 64 == 0 and TH >= ac.ASM_MIN_KEYS


def test_one_tile_below_the_threshold_stays_on_the_plain_kernel(built_lib):
    run(AttnCase(640, (TH - 64,), 64, H16, heads(640), 4, forms=("asm512",)), PLAIN)


@pytest.mark.parametrize("r", range(3))
def test_at_the_threshold_and_every_remainder_of_the_group(built_lib, r):
    """keys = threshold + r tiles for every remainder mod the group (and r = 2 whatever the group); tq = 513 (one row in the last workgroup), 640, and
    257: the fewest rows the launch rule leaves on 512-query items (three of the four waves re-aimed at the last 128 rows)"""
    assert group() <= 3
    tq = (513, 640, 257)[r]
    c = AttnCase(tq, (TH + 64 * r,), 64, (H16, BF16, H16)[r], heads(tq), (4, 2, 4)[r], forms=("asm512",))
    assert ac.asm_form(c, n_cus()) == "asm512"
    run(c, GRP)


def test_128_query_rows_stay_on_256_query_items(built_lib):
    """tq = 128 at the threshold: up to 256 rows a launch has as many 256-query items as 512-query ones, so the launch rule takes the 256-query form
    whatever the heads (tests/test_attn_geometry_gpu.py) -- and the grouped form changes 512-query launches only: the name and the kernel stay"""
    c = AttnCase(128, (TH,), 64, BF16, heads(128), 4, forms=("q256",))
    assert ac.asm_form(c, n_cus()) == "q256"
    run(c, ac.FORM_NAMES["q256"])


def test_eight_tiles_above_the_threshold(built_lib):
    run(AttnCase(513, (TH + 8 * 64,), 64, BF16, heads(513), 4, forms=("asm512",)), GRP)


def test_threshold_over_three_segments_with_an_empty_one(built_lib):
    """the segment hop falls inside a group of tiles (an odd tile count in the first segment)"""
    run(AttnCase(640, (TH // 2 + 64, 0, TH // 2 - 64), 64, BF16, heads(640), 2, forms=("asm512",)), GRP)


def test_batch_of_two_with_wide_strides(built_lib):
    t, Hb = 640, heads(640, batch=2)
    run(AttnCase(t, (TH + 64,), 64, H16, Hb, 2, 2, ldq=Hb * 64 + 8, ldk=Hb // 2 * 64 + 16, ldo=Hb * 64 + 4, ldvt=ops.vt_ld(TH + 64) + 64,
                 q_bs=(t + 3) * (Hb * 64 + 8), o_bs=(t + 1) * (Hb * 64 + 4), k_pad_rows=2, vt_pad_rows=3, forms=("asm512",)), GRP)


def test_park_and_resume(built_lib):
    """both launches on the grouped kernel: the tile count of the group starts again with the second launch"""
    run(AttnCase(513, (TH, TH + 64), 64, H16, heads(513), 4, state=("park", 1), forms=("asm512",)), GRP)


def test_parked_by_the_grouped_kernel_and_resumed_by_the_plain_one(built_lib):
    run(AttnCase(640, (TH + 64, 192), 64, BF16, heads(640), 4, state=("park", 1), forms=("asm512",)), GRP, PLAIN)


def test_two_rounds_take_the_work_stealing_form(built_lib):
    """two rounds of 512-query items at 16 heads: persistent workgroups re-enter the prologue per item; bit for bit the static launch"""
    n_cu = n_cus()
    c = AttnCase(512 * -(-2 * n_cu // 16), (TH + 64,), 64, H16, 16, 2, forms=("asm512",))
    assert ac.steals(c, n_cu) and ops.ATTN_WORK_STEALING and ac.asm_form(c, n_cu) == "asm512"
    stolen = run(c, GRP)
    ops.ATTN_WORK_STEALING = False
    try:
        static = run(c, GRP)
    finally:
        ops.ATTN_WORK_STEALING = True
    assert torch.equal(stolen.view.view(torch.int16), static.view.view(torch.int16)), f"{c.id}: work stealing and the static launch differ"
