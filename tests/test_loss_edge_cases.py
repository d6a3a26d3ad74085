"""No GPU: the cases of tests/loss_edge_cases.py reach what they are named for, the partition restated there has the properties the kernel's
slot addressing rests on, the float64 reference is stable on every new case to half the bound the GPU module asserts, and every deliberately
wrong variant of the restatement misses that bound on the cases that are there to catch it."""
import functools
import math
import random

import pytest
import torch

import loss_edge_cases as E
import test_losses_gpu as TL

F64 = torch.float64
NBS = (1024, 2048)   # 4 x 256 CUs (MI355X), and the cap MAX_BLOCKS


@functools.lru_cache(maxsize=None)
def reference(name):
    return E.reference(E.case(name))


def figure(got, want):
    """worst |got - want| / max(|want|, 1e-2) over the finite outputs; NaN and infinities must agree exactly"""
    worst = 0.0
    assert list(got) == list(want)
    for k, w in want.items():
        if math.isnan(w) or math.isinf(w) or math.isnan(got[k]) or math.isinf(got[k]):
            assert (math.isnan(w) and math.isnan(got[k])) or got[k] == w, (k, got[k], w)
            continue
        worst = max(worst, abs(got[k] - w) / TL.scale(w))
    return worst


# ================================================================================================ constants, check_outputs
def test_constants_match_the_kernel_source():
    assert E.source_constants() == dict(THREADS=E.THREADS, PX=E.PX, TILE=E.TILE, MAX_BLOCKS=E.MAX_BLOCKS, BLOCKS_PER_CU=E.BLOCKS_PER_CU, WAVES=E.WAVES)
    assert E.num_blocks(256) == 1024 and E.num_blocks(512) == E.num_blocks(4096) == E.MAX_BLOCKS and E.WAVE * E.WAVES == E.THREADS


def test_check_outputs_takes_infinities_literally():
    inf = math.inf
    TL.check_outputs({"loss": 1.0, "a": inf, "b": -inf}, {"loss": 1.0, "a": inf, "b": -inf})
    for got in ({"loss": 1.0, "a": -inf}, {"loss": 1.0, "a": 1e300}, {"loss": 1.0, "a": math.nan}):
        with pytest.raises(AssertionError):
            TL.check_outputs(got, {"loss": 1.0, "a": inf})
    with pytest.raises(AssertionError):
        TL.check_outputs({"loss": 1.0, "a": inf}, {"loss": 1.0, "a": 2.0})


# ================================================================================================ preconditions
@pytest.mark.parametrize("nb", NBS)
def test_partition_cases_reach_what_they_are_named_for(nb):
    E.check_a_preconditions(nb)
    if nb == NBS[0]:
        (views, _), geo = E._a_data("crossing", nb)
        assert all(not bool(views[e]["valid_mask"].any()) for e in geo["empty"]) and all(views[z]["pts3d"].shape == (1, 0, E.ZERO_W, 3) for z in geo["zero"])


def test_count_cases_exceed_the_strides():
    shapes = set(E.B_SHAPES)
    assert any(B > E.WAVES for _, B in shapes)                                      # V4 global: more groups than waves
    assert any(B > E.WAVE for _, B in shapes) and any(V > E.WAVE for V, _ in shapes)   # V3 local / V4 global: more members than lanes
    assert any(V > 2 * E.WAVE for V, _ in shapes)                                   # the lane stride taken twice
    assert any(V * B > E.THREADS and V <= E.WAVE for V, B in shapes)                 # more than 256 segments (second setup workgroup, gather stride)
    assert any(V > E.THREADS for V, _ in shapes)                                    # more than 256 views (finish stride)
    c = E.case("B-V3-B100-v4")
    scales = E.sample_scales(100)
    assert len({round(s, 6) for s in scales}) == 100 and all(abs(scales[b] - scales[b % 4]) > 1e-3 for b in range(4, 100))
    assert c.V == 3 and c.B == 100 and c.npix == [15] * 3


def test_pixel_count_cases_start_samples_at_every_residue():
    assert {n % E.PX for n in E.C_NPIX} == {0, 1, 2, 3} and {2 * n % E.PX for n in E.C_NPIX if n % 2} == {2}
    assert all(n in E.C_NPIX for n in (E.TILE - 1, E.TILE, E.TILE + 1, 2 * E.TILE - 1, 2 * E.TILE, 2 * E.TILE + 1, 3 * E.TILE + 1))
    c = E.case("C-n1022")
    assert c.B == 3 and c.npix == [1022, 1022] and (1022 * 2) % E.PX == 0 and 1022 % E.PX == 2   # sample 2 is aligned and its last thread partial


def e_poses(name):
    return [P.float().to(F64) for v in E.case(name).views for P in v["camera_pose"]]   # as the kernel sees them


def test_pose_cases_force_the_row_swaps():
    """Columns 0 and 1 swap rows in some pose, with every pair of rows (0, 1), (0, 2), (1, 2).  Column 2 cannot: its only candidate is row 3,
    and with the bottom row 0 0 0 1 the entry a[3][2] stays exactly 0 through the elimination (asserted); a swap there needs a projective
    matrix, which is not a pose."""
    for name in E.E_NAMES:
        swaps = set()
        for P in e_poses(name):
            assert P[3].tolist() == [0.0, 0.0, 0.0, 1.0]
            assert float(torch.linalg.cond(P, p=2)) <= 10.0
            inv, rows = E.gauss_jordan(P.tolist())
            assert float((torch.tensor(inv, dtype=F64) - torch.linalg.inv(P)).abs().max()) < 1e-13
            assert rows[2] == 2 and rows[3] == 3
            swaps |= {(c, r) for c, r in enumerate(rows) if r != c}
            bad, _ = E.gauss_jordan(P.tolist(), pivoting=False)
            if rows != [0, 1, 2, 3] and name != "E-affine":   # without the swap the pivot is about SMALL: the inverse loses digits (the shear
                assert not float((torch.tensor(bad, dtype=F64) - torch.linalg.inv(P)).abs().max()) < 1e-12   # of E-affine fills the would-be pivots)
        assert swaps == {(0, 1), (0, 2), (1, 2)}, (name, swaps)
    A = e_poses("E-affine")[0][:3, :3]
    assert float((A.t() @ A - torch.eye(3, dtype=F64)).abs().max()) > 0.3          # not orthonormal
    assert E.case("E-fp64").views[0]["camera_pose"].dtype == F64 and E.case("E-turns").views[0]["camera_pose"].dtype == torch.float32
    P64 = E.case("E-fp64").views[1]["camera_pose"]
    assert not torch.equal(P64.float().to(F64), P64)                              # not representable in fp32: the rounding matters


def test_value_cases_hold_what_they_claim():
    v, b, i, j, c = E.GT_PIXEL
    m = E.case("F-maskbytes").views[0]["valid_mask"]
    assert m.dtype == torch.uint8 and all(int((m == x).sum()) > 0 for x in (0, 1, 2, 128, 255))
    for name, value, ok in (("F-nan-v4", math.nan, True), ("F-nan-v3", math.nan, True), ("F-nan-v4-clip", math.nan, True), ("F-inf-v4", math.inf, True),
                            ("F-nan-invalid", math.nan, False), ("F-base", None, False)):
        view = E.case(name).views[v]
        x = float(view["pts3d"][b, i, j, c])
        assert bool(view["valid_mask"][b, i, j]) == ok and (math.isfinite(x) if value is None else (math.isnan(x) if math.isnan(value) else x == value))
    base, inv = E.case("F-base"), E.case("F-nan-invalid")
    assert all(torch.equal(p[k], q[k]) for p, q in zip(base.preds, inv.preds) for k in p)
    assert all(torch.equal(p["valid_mask"], q["valid_mask"]) for p, q in zip(base.views, inv.views))
    # NaN exactly where the restatement has it: V4 the view of the pixel (both sets), V3 every global output and the view's local ones
    nan_keys = lambda name: {k for k, x in reference(name).items() if math.isnan(x)}  # noqa: E731
    tag = f"/{v:02d}"
    assert nan_keys("F-nan-v4") == {"loss"} | {k for k in reference("F-nan-v4") if k.endswith(tag)}
    assert nan_keys("F-nan-v3") == {"loss"} | {k for k in reference("F-nan-v3") if k.endswith(tag) or "_global/" in k}
    for name in ("F-nan-v4-clip", "F-nan-v3-clip"):
        assert all(math.isfinite(x) for x in reference(name).values())
    assert reference("F-nan-invalid") == reference("F-base")


# ================================================================================================ partition properties
def kernel_walk(p):
    """loss_pass_kernel's own loop over the tiles: last_le, then `do ++s; while (t >= tile0[s + 1])` -> the (k, s) at which it calls block_sum"""
    out = []
    for k in range(p.nb):
        ta, tb = p.first[k], p.first[k + 1]
        if ta >= tb:
            continue
        lo, hi = 0, p.nseg
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if p.tile0[mid] <= ta:
                lo = mid
            else:
                hi = mid
        s = lo
        for t in range(ta, tb):
            if t >= p.tile0[s + 1]:
                out.append((k, s))
                s += 1
                while t >= p.tile0[s + 1]:
                    s += 1
            assert p.tile0[s] <= t < p.tile0[s + 1] and p.seg_npix[s] > (t - p.tile0[s]) * E.TILE
        out.append((k, s))
    return out


def check_partition(p):
    slots = [x for _, _, x in p.slots]
    assert len(set(slots)) == len(slots)                                  # k + s is unique among the pairs met
    assert all(0 <= x < E.MAX_BLOCKS + p.nseg for x in slots) and p.nb <= E.MAX_BLOCKS
    assert kernel_walk(p) == [(k, s) for k, s, _ in p.slots]              # the kernel's loop meets exactly these, in this order
    meeting = p.meeting()
    for s in range(p.nseg):
        assert p.gathered(s) == meeting.get(s, []), s                      # what the gather sums is what was written
    owner = p.owner()
    assert len(owner) == p.T and all(E.block_of_tile(t, p.T, p.nb)[0] == owner[t] for t in range(0, p.T, max(1, p.T // 997)))
    assert sum(len(p.gathered(s)) for s in range(p.nseg)) == len(slots)


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("geom", E.A_GEOMS)
def test_partition_properties_of_the_cases(geom, nb):
    geo = E.a_geometry(geom, nb)
    check_partition(E.partition([h * w for h, w in geo["shapes"]], geo["B"], nb))


def test_partition_properties_of_random_lengths():
    rnd = random.Random(11)
    lengths = [0, 0, 1, 2, 5, 7, 1023, 1024, 1025, 2048, 3000, 4097, 9217]
    seen_multi_cross = 0
    for trial in range(600):
        nb = rnd.randint(1, 40)
        npix = [rnd.choice(lengths) for _ in range(rnd.randint(1, 30))]
        if not any(npix):
            npix[rnd.randrange(len(npix))] = 1
        p = E.partition(npix, rnd.randint(1, 3), nb)
        check_partition(p)
        seen_multi_cross += any(len(row) >= 4 for row in p.met)
    assert seen_multi_cross > 50


# ================================================================================================ the reference on the new cases
@pytest.mark.parametrize("name", E.NAMES + [E.D_BASE])
def test_reference_is_stable_and_the_flat_restatement_agrees(name):
    """pixels in reversed order and the inverse poses from a solve: within half of what the GPU module allows, so the kernel keeps at least the
    same share; no finite output of a view with pixels is small against its terms (see loss_edge_cases.BIAS_GLOBAL)"""
    c = E.case(name)
    want = reference(name)
    assert len(want) == 1 + 4 * c.V
    again = E.reference(E.reversed_pixels(c), inv=E.solved_inverses(c))
    fig = figure(again, want)
    flat = figure(E.restate(c), want)
    print(f"LOSS-MEASURE {name}: two float64 evaluations differ by {fig:.3e}, the flat restatement by {flat:.3e}")
    assert fig <= TL.REL_F64 / 2 and flat <= TL.REL_F64 / 2
    small = [k for k, x in want.items() if math.isfinite(x) and abs(x) < 0.1 and not ("conf_loss" in k and x == 0.0)]
    assert not small, small
    for v in c.empty:
        for kind in ("global", "local"):
            term = want[f"ConfLossMultiviewV2_conf_loss_{kind}/{v:02d}"]
            assert term == 0.0 and math.copysign(1.0, term) == 1.0 and math.isnan(want[f"Regr3DMultiviewV3_pts3d_loss_{kind}/{v:02d}"])


@pytest.mark.parametrize("name", [n for n in E.NAMES if "clip" in n])
def test_no_pixel_lies_at_the_clip_distance(name):
    c = E.case(name)
    clip = c.recipe["dist_clip"]
    for v, view in enumerate(c.views):
        inv = torch.linalg.inv(torch.stack([c.views[0]["camera_pose"], view["camera_pose"]]).float().to(F64))
        x = view["pts3d"].to(F64)
        for m in inv:
            d = ((m[:, None, None, :3, :3] * x[..., None, :]).sum(-1) + m[:, None, None, :3, 3]).norm(dim=-1)
            assert not bool(((d - clip).abs() < 1e-9).any()), (name, v)


# ================================================================================================ discrimination
CATCHES = {
    "first64": ("B-V65-B2-v4", "B-V129-B1-v4", "B-V300-B1-v4lsc"),
    "group_mod4": ("B-V2-B5-v4", "B-V2-B65-v4lsc", "B-V3-B100-v4", "B-V65-B2-v3", "B-V300-B1-v3"),
    "mask_eq1": ("F-maskbytes",),
    "no_pivot": ("E-turns", "E-fp64"),
    "v3_nanmean": ("F-nan-v3",),
    "clip_keeps_nan": ("F-nan-v4-clip", "F-nan-v3-clip"),
    "merged_partials": ("A-T=nb+1-v4", "A-T=2nb+1-v3clip", "A-four-v4", "A-crossing-v4", "A-crossing-v3clip"),
}


@pytest.mark.parametrize("wrong", E.WRONG)
def test_wrong_variants_miss_the_bound_the_gpu_module_asserts(wrong):
    assert set(CATCHES) == set(E.WRONG)
    for name in CATCHES[wrong]:
        c = E.case(name)
        TL.check_outputs(E.restate(c), reference(name), what=f"{name} restated")          # the control
        with pytest.raises(AssertionError):
            TL.check_outputs(E.restate(c, wrong=wrong), reference(name), what=f"{name} with {wrong}")
