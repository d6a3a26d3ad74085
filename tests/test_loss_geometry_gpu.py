"""f3r_mv_conf_loss at the edges of its indexing, on a real MI355X through the C ABI: the tile partition around nb = min(4 x CUs, 2048) tiles
and with workgroups that meet four and more segments, cross all-invalid and zero-pixel segments between two multi-tile ones; group, member,
segment and view counts beyond every stride; pixel counts around the 4 of a thread and the 1024 of a tile; one operand at a time off the
16-byte path; poses whose inverse swaps rows; mask bytes other than 0 / 1 and NaN / inf ground truth (cases and what each is there for:
tests/loss_edge_cases.py; that they reach it and discriminate: tests/test_loss_edge_cases.py).

The cases module owns every buffer: operands in arenas of 0xFF bytes, `out` and a workspace of exactly f3r_mv_conf_loss_workspace_bytes between
sentinel words, the workspace 0xFF-filled before every run (NaN to whoever reads a slot he did not write).  After each launch: synchronise,
guards intact, arenas unchanged, then all 1 + 4 V outputs against loss_ref.multiview_conf_loss in float64 through test_losses_gpu.check_outputs,
at its bound REL_F64 = 10 x 5.3e-15 (half an fp32 ulp more for `loss`), NaN exactly where the reference has it.  Measured on an MI355X over
every case here, as |got - ref64| / max(|ref64|, 1e-2): worst REL_F64_MEASURED_EDGE = 2.3e-15 (A-T=nb-v4; next to test_losses_gpu's 5.3e-15 of
the 20-Mpixel size case; docs/rows_f.md); every shifted run of family D and every second run bit-equal.
"""
import functools
import math

import pytest
import torch

import loss_cases as C
import loss_edge_cases as E
import test_losses_gpu as TL

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL_F64_MEASURED_EDGE = 2.3e-15  # worst figure of the measurement run over the cases of this module (nb = 1024); the bound asserted is TL.REL_F64
TWICE = ("A-four-", "A-crossing-")   # run twice on the 0xFF-filled workspace: the same bits


@pytest.fixture(scope="module")
def nb():
    return E.num_blocks(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def reference(name, nb):
    return E.reference(E.case(name, nb))


def bits(t):
    return t.contiguous().view(torch.int64)


def check_empty_views(c, got):
    for v in c.empty:
        for kind in ("global", "local"):
            term = got[f"ConfLossMultiviewV2_conf_loss_{kind}/{v:02d}"]
            assert term == 0.0 and math.copysign(1.0, term) == 1.0, (c.name, v, kind, term)   # the literal +0.0
            assert math.isnan(got[f"Regr3DMultiviewV3_pts3d_loss_{kind}/{v:02d}"]), (c.name, v, kind)


def test_partition_cases_reach_what_they_are_named_for_on_this_device(nb):
    print(f"LOSS-MEASURE grid: nb = {nb}")
    E.check_a_preconditions(nb)


@pytest.mark.parametrize("name", E.NAMES)
def test_case_against_the_float64_reference(built_lib, nb, name):
    c = E.case(name, nb)
    want = reference(name, nb)
    runs = E.run_loss(built_lib, DEV, c, runs=2 if name.startswith(TWICE) else 1)
    raw, got = runs[0]
    assert len(got) == len(want) == 1 + 4 * c.V
    TL.check_outputs(got, want, what=name)
    check_empty_views(c, got)
    if len(runs) > 1:
        assert torch.equal(bits(raw), bits(runs[1][0])), f"{name}: two runs on a workspace of 0xFF bytes differ"


def test_value_cases_relate_as_stated(built_lib):
    """NaN ground truth at an invalid pixel changes no bit; under a dist_clip the NaN pixel is dropped and everything is finite"""
    base, inv = (E.run_loss(built_lib, DEV, E.case(n))[0] for n in ("F-base", "F-nan-invalid"))
    same = torch.equal(bits(base[0]), bits(inv[0]))
    print(f"LOSS-MEASURE F-nan-invalid against F-base: bit-equal {same}")
    assert same
    for n in ("F-nan-v4-clip", "F-nan-v3-clip"):
        got = E.run_loss(built_lib, DEV, E.case(n))[0][1]
        print(f"LOSS-MEASURE {n}: {sum(not math.isfinite(x) for x in got.values())} outputs of {len(got)} not finite")
        assert all(math.isfinite(x) for x in got.values()), n


def test_one_operand_at_a_time_off_the_vector_path(built_lib):
    """1025 pixels, B = 1: every operand starts 16-byte aligned.  Each of gt, pred, conf, pred_local, conf_local moved by 4 bytes and the mask by
    1 byte, alone and then all together: per-pixel arithmetic and the order of the sums do not depend on the load path, so the bits are equal"""
    c = E.case(E.D_BASE)
    raw, got = E.run_loss(built_lib, DEV, c)[0]
    TL.check_outputs(got, E.reference(c), what=E.D_BASE)
    for shifts in [{k: E.D_SHIFT[k]} for k in E.D_OPERANDS] + [dict(E.D_SHIFT)]:
        moved, _ = E.run_loss(built_lib, DEV, c, shifts=shifts)[0]
        same = torch.equal(bits(raw), bits(moved))
        print(f"LOSS-MEASURE {E.D_BASE} shifted {sorted(shifts)}: bit-equal {same}")
        assert same, shifts


@pytest.mark.parametrize("name", ["B-V300-B1-v4", "A-crossing-v3clip"])
def test_public_wrapper_on_many_views_and_zero_pixel_views(built_lib, nb, name):
    """ConfLossMultiviewV2 itself: the 300-view table upload, and zero-pixel views through the wrapper's shape checks"""
    c = E.case(name, nb)
    views, preds = C.to_device(c.views, c.preds, DEV)
    kw = {"dist_clip": c.recipe["dist_clip"]} if "dist_clip" in c.recipe else {}
    loss, details = TL.criterion(c.recipe)(views, preds, **kw)
    assert loss.dtype == torch.float32 and loss.is_cuda
    got = {"loss": float(loss), **details}
    TL.check_outputs(got, reference(name, nb), what=f"{name} through the wrapper")
    check_empty_views(c, got)
