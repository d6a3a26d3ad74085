"""The convolution geometry cases without a GPU: the references of tests/conv_cases.py against F.conv2d on the materialised batch, the case
lists against the structural properties tests/test_conv_geometry_gpu.py relies on (computed from shapes alone), and the K-tile table guard
of f3r_gemm256_eligible through a host-side call."""
import ctypes
import dataclasses

import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
from conv_cases import BF16, H16, ConvCase
from fast3r_amd import _lib, ops


# ------------------------------------------------------------------------------------------------ references
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("split,dt", [(None, BF16), ("x3", H16)])
def test_periodic_reference_equals_conv2d_on_the_full_batch(stride, split, dt):
    c = ConvCase(7, 5, 4, 64, 128, stride, split, dt, ("bias", "skips"), P=3)
    d = cc.build(c)
    assert d["x"].shape[0] == 3 and d["ref"]["out"].shape == (3, *c.out_hw, 128)
    x = cc.periodic(d["x"], c.B).double()
    if split == "x3":
        x = x + cc.periodic(d["x_lo"], c.B).double()
    w = d["w32"].double() if split == "x3" else d["w32"].to(dt).double()
    full = F.conv2d(x.permute(0, 3, 1, 2), w, d["bias"].double(), stride=stride, padding=1).permute(0, 2, 3, 1)
    for hi, lo in d["res"]:
        full = full + cc.periodic(hi, c.B).double() + (cc.periodic(lo, c.B).double() if lo is not None else 0.0)
    assert full.shape[0] == 7
    ref = cc.periodic(d["ref"]["out"], c.B)
    # float64 against float64 on the same operands: the summation order of conv2d may differ between batch sizes, nothing else
    assert float((full - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.equal(cc.periodic(d["ref"]["relu"], c.B), F.relu(ref))
    assert torch.equal(ref[5], ref[2]) and torch.equal(ref[6], ref[0]) and not torch.equal(ref[0], ref[1])


def test_periodic_is_the_identity_without_a_period():
    c = ConvCase(4, 3, 3, 64, 128)
    d = cc.build(c)
    assert d["x"].shape[0] == 4 and cc.periodic(d["x"], 4) is d["x"]


def test_a_relu_reference_applies_the_relu_to_the_operand():
    c = ConvCase(2, 3, 3, 24, 40, 1, None, H16, ("bias", "a_relu"))
    d = cc.build(c)
    ref = F.conv2d(F.relu(d["x"].double()).permute(0, 3, 1, 2), d["w32"].to(H16).double(), d["bias"].double(), padding=1).permute(0, 2, 3, 1)
    assert float((ref - d["ref"]["out"]).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float((cc.conv64(d["x"], d["w32"].to(H16)) + d["bias"].double() - ref).abs().max()) > 0.1  # (and differs from the plain conv)


@pytest.mark.parametrize("stride", [1, 2])
def test_decoded_planes_reference_equals_the_plain_one_to_the_fp8_bound(stride):
    """unit-scale data, nothing clamped: hi x hi + hi8 x lo8 + lo8 x hi8 recovers the product of the fp32 operands to 3e-5 of the output scale
    (the bound test_conv_x3f8_planes_and_accuracy holds the kernel to), where one fp16 plane is two orders of magnitude coarser"""
    c = ConvCase(2, 5, 4, 128, 128, stride, "x3f8", H16, ("bias",))
    d = cc.build(c)
    true = cc.conv64(d["x32"], d["w32"], stride) + d["bias"].double()
    scale = float(true.abs().max())
    err = float((d["ref"]["out"] - true).abs().max()) / scale
    single = float((cc.conv64(d["x32"].to(H16), d["w32"].to(H16), stride) + d["bias"].double() - true).abs().max()) / scale
    assert err < 3e-5 and single > 8 * err, (err, single)
    assert float(d["x32"].abs().max()) < 448.0  # out-of-range fp8 inputs stay with the test that owns clamping
    assert d["x_f8"].shape == (2, 5, 4, 256) and d["x"].dtype == H16


def test_fin_reference_is_the_postprocessed_1x1_conv():
    c = ConvCase(2, 4, 3, 128, 128, 1, None, H16, ("bias", "fin"))
    d = cc.build(c)
    w4, b4, conf_mode = d["fin"]
    y = F.relu(d["ref"]["out"])
    z = y @ w4.double().t() + b4.double()
    n = z[..., :3].norm(dim=-1)
    assert torch.allclose(d["ref"]["pts"].norm(dim=-1), torch.expm1(n), rtol=1e-12) and torch.allclose(d["ref"]["conf"], 1.0 + z[..., 3].exp(), rtol=1e-12)
    assert conf_mode[0] == "exp"


# ------------------------------------------------------------------------------------------------ the case lists
ALL_STATIC = cc.TINY + cc.STRIDE2 + cc.TAILS + [cc.GUARD_OVER_X3, cc.GUARD_OVER_F8, cc.GUARD_FITS_X3]


def test_case_ids_are_unique():
    for cases in (cc.TINY, cc.STRIDE2, cc.TAILS, cc.second_tile_cases(cc.CU_NOMINAL)):
        ids = [c.id for c in cases]
        assert len(set(ids)) == len(ids)


def test_every_case_is_a_legal_launch():
    for c in ALL_STATIC + cc.second_tile_cases(cc.CU_NOMINAL):
        assert c.Ci % 8 == 0 and c.Co % 4 == 0 and c.stride in (1, 2) and c.M > 0
        if c.split == "x3f8":
            assert c.Ci % 128 == 0 and c.dtype == H16 and c.Co % 128 == 0
        if "fin" in c.extras:
            assert c.Co == 128 and c.Ci % 64 == 0
        if "a_relu" in c.extras:
            assert c.split is None
        assert 1 in cc.kernel_sels(c) or cc.kernel_sels(c) == [0]


def test_tiny_cases_cover_the_small_images():
    t = cc.TINY
    hw = {(c.H, c.W) for c in t}
    assert {(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (3, 1)} <= hw
    assert all(c.H <= 5 and (c.W <= 5 or (c.H, c.W) == (1, 7)) for c in t)
    for h, w in hw:  # every image size at both strides, on one plane in both dtypes, with x3 in both, with x3f8
        for s in (1, 2):
            kinds = {(c.split, c.dtype) for c in t if (c.H, c.W, c.stride) == (h, w, s)}
            assert kinds == {(None, H16), (None, BF16), ("x3", H16), ("x3", BF16), ("x3f8", H16)}, (h, w, s)
    assert {c.Ci for c in t} == {64, 128, 192} and {c.Co for c in t} == {128, 256}
    assert all("bias" in c.extras and cc.eligible256(c) for c in t)   # every form of the 256-tile kernel takes every tiny case
    # narrower or shorter than the kernel: the tap offsets alias the centre pixel or another row, at both strides
    assert any(c.H == 1 and c.W == 1 for c in t) and any(c.H <= 2 and c.W > 2 for c in t) and any(c.W <= 2 and c.H > 2 for c in t)
    # M below one tile, and just above it: a second m-tile that is nearly empty (rows past M)
    for s in (1, 2):
        assert any(c.M < 256 for c in t if c.stride == s) and any(256 < c.M <= 300 for c in t if c.stride == s)
    assert any((c.B, c.H, c.W, c.M) == (7, 2, 3, 42) for c in t) and any((c.B, c.H, c.W, c.M) == (37, 1, 7, 259) for c in t)
    assert all(c.M % 256 != 0 for c in t)
    # tiles that hold several whole images and a ragged end
    assert any(cc.images_in_tile(c, 0) >= 3 and c.per_img < 256 and 256 % c.per_img != 0 and c.M > 256 for c in t)
    assert any(cc.images_in_tile(c, 0) == 256 for c in t)      # 1 x 1 images: every row its own image
    skips = [c for c in t if "skips" in c.extras]
    assert {(c.split, c.dtype) for c in skips} == {(None, H16), (None, BF16), ("x3", H16), ("x3", BF16)}
    assert all(c.M % 256 != 0 and cc.images_in_tile(c, 0) >= 3 for c in skips)


def test_stride2_cases_cover_both_parities():
    sizes = {(c.H, c.W) for c in cc.STRIDE2}
    assert sizes == {(4, 4), (5, 4), (4, 5), (5, 5), (8, 7)}
    assert {(h % 2, w % 2) for h, w in sizes} == {(0, 0), (1, 0), (0, 1), (1, 1)}
    for hw in sizes:
        kinds = {(c.split, c.dtype) for c in cc.STRIDE2 if (c.H, c.W) == hw}
        assert kinds == {(None, H16), (None, BF16), ("x3", H16), ("x3", BF16), ("x3f8", H16)}
    assert all(c.stride == 2 and c.B == 3 and cc.eligible256(c) for c in cc.STRIDE2)
    assert all(cc.kernel_sels(c) == ([0] if c.split == "x3f8" else [1, 2, 3, 4, 0]) for c in cc.STRIDE2)


def test_tail_cases_stay_on_the_128_tile_kernel():
    t = cc.TAILS
    assert {c.Ci for c in t} == {8, 24, 72, 136} and all(c.Ci % 64 != 0 for c in t)
    assert {(c.H, c.W) for c in t} == {(3, 3), (5, 6)} and {c.stride for c in t} == {1, 2}
    for ci in (8, 24, 72, 136):
        for relu in (False, True):
            assert {(c.H, c.stride, c.dtype) for c in t if c.Ci == ci and ("a_relu" in c.extras) == relu} == \
                {(h, s, dt) for h in (3, 5) for s in (1, 2) for dt in (H16, BF16)}
    assert all(cc.kernel_sels(c) == [1, 0] for c in t)
    assert any(c.Co % 64 != 0 for c in t)   # a ragged n-tile too


def test_second_tile_cases_need_more_tiles_than_cus():
    n_cu = cc.CU_NOMINAL
    cases = cc.second_tile_cases(n_cu)
    for c in cases:
        assert c.out_hw == (15, 17) and c.per_img == 255 and c.P == 5 and not cc.period_hides_a_stale_tile(c, n_cu)
        n = cc.tiles(c, 256 if c.Co == 256 else 128)
        assert n_cu + 4 <= n <= n_cu + 6, n                      # workgroups 0 .. 3 (at least) walk a second tile
        assert c.M % 256 != 0 and c.M > 65536                    # a ragged last tile; more output pixels than a dense reference would want
        assert all(cc.images_in_tile(c, t) == 2 for t in range(1, cc.m_tiles(c) - 1))   # every full tile but the first straddles two images
        assert cc.eligible256(c)
        # the second tile of a workgroup starts n_cu * 256 rows on: at another pixel of an image with other content
        assert (n_cu * 256) % 255 != 0 and (n_cu * 256 // 255) % c.P != 0
    kinds = {(c.split, c.dtype, "fin" in c.extras) for c in cases if c.stride == 1 and c.Ci == 128}
    assert kinds == {(s, d, f) for s, d in ((None, H16), (None, BF16), ("x3", H16), ("x3", BF16), ("x3f8", H16)) for f in (False, True)}
    assert {c.split for c in cases if c.stride == 2} == {"x3", "x3f8"} and all((c.H, c.W) == (30, 34) for c in cases if c.stride == 2)
    wide = [c for c in cases if c.Co == 256]
    assert len(wide) == 1 and wide[0].Ci == 64 and cc.k_tiles(wide[0]) % 2 == 1
    assert max(cc.k_tiles(c) for c in cases) == 486
    assert cc.period_hides_a_stale_tile(cases[0], 255) and cc.second_tile_B(256) == 262


def test_guard_cases_sit_on_the_table_limit():
    assert cc.k_tiles(cc.GUARD_OVER_X3) == 513 and cc.k_tiles(cc.GUARD_OVER_F8) == 540 and cc.k_tiles(cc.GUARD_FITS_X3) == 486
    assert cc.k_tiles(ConvCase(1, 8, 8, 1792, 128, 1, "x3f8")) == 504 and cc.k_tiles(ConvCase(1, 8, 8, 3648, 128)) == 513
    assert cc.k_tiles(ConvCase(1, 8, 8, 1856, 128, 1, "w2")) == 522 and cc.k_tiles(ConvCase(1, 8, 8, 1792, 128, 1, "w2")) == 504
    assert cc.kernel_sels(cc.GUARD_OVER_X3) == [1, 0] and cc.kernel_sels(cc.GUARD_FITS_X3) == [1, 2, 3, 4, 0]
    # the smallest x3 shape that does not fit: one 64-channel step above the largest that does
    assert cc.GUARD_OVER_X3.Ci - cc.GUARD_FITS_X3.Ci == 64


# ------------------------------------------------------------------------------------------------ guarded placement
@pytest.mark.parametrize("dt", [H16, BF16, torch.uint8])
def test_guarded_operand_is_a_16_byte_aligned_view_between_nan_patterns(dt):
    t = (torch.arange(2 * 3 * 5 * 8) % 200).to(dt).view(2, 3, 5, 8)
    view, buf = cc.guarded_operand(t, "cpu", margin_bytes=7 * 8 * t.element_size())
    assert torch.equal(view, t) and view.is_contiguous() and view.data_ptr() % 16 == 0 and view.data_ptr() % 32 == 16
    nb = t.numel() * t.element_size()
    off = view.data_ptr() - buf.data_ptr()
    assert off >= 7 * 8 * t.element_size() and buf.numel() - off - nb >= 7 * 8 * t.element_size()
    outside = torch.cat([buf[:off], buf[off + nb:]])
    assert bool((outside == 0xFF).all())
    if dt != torch.uint8:
        assert bool(outside.view(dt).isnan().all())
    else:
        assert bool(outside.view(torch.float8_e4m3fn).float().isnan().all())


def test_guarded_out_notices_a_stray_store():
    view, buf, lo, hi = cc.guarded_out((3, 2, 2, 40), BF16, "cpu")
    assert view.shape == (3, 2, 2, 40) and view.data_ptr() % 16 == 0 and hi - lo == view.numel() and lo >= 3 * 40 and buf.numel() - hi >= 3 * 40
    view.fill_(1.5)
    assert cc.guards_intact(buf, lo, hi)
    assert bool(torch.isfinite(buf.view(BF16).float()).all()) and bool(torch.isfinite(buf.view(H16).float()).all())
    for at in (lo - 1, hi, 0, buf.numel() - 1):   # one element before the outputs, one row past M, either end
        b2 = buf.clone()
        b2[at] = 0
        assert not cc.guards_intact(b2, lo, hi)


# ------------------------------------------------------------------------------------------------ the guard itself, on the host
def _gemm_args(c, fin=False):
    """the f3r_gemm_args ops.conv3x3 builds for the case, with stand-in operand addresses (eligibility reads no memory)"""
    g = _lib.GemmArgs()
    oh, ow = c.out_hw
    planes = 1 if c.split is None else 2
    g.A = g.W = g.out_lp = 0x1000
    g.M, g.N, g.Kpad = c.M, c.Co, planes * 9 * ((c.Ci + 63) // 64) * 64
    g.a_mode, g.conv_H, g.conv_W, g.conv_C, g.conv_stride, g.conv_OH, g.conv_OW = _lib.F3R_A_CONV3X3, c.H, c.W, c.Ci, c.stride, oh, ow
    g.epi, g.dtype, g.split, g.ldo_lp = _lib.F3R_EPI_GENERIC, _lib.dtype_id(c.dtype), ops.SPLIT[c.split], c.Co
    if c.split is not None:
        g.A_lo = 0x1000
    if fin:
        g.fin_w = g.fin_b = g.fin_pts = 0x1000
        g.out_lp = None
    return g


def _eligible(lib, g):
    f = lib._Z20f3r_gemm256_eligibleRK13f3r_gemm_args   # bool f3r_gemm256_eligible(const f3r_gemm_args&): csrc/f3r_common.h
    f.restype, f.argtypes = ctypes.c_bool, [ctypes.POINTER(_lib.GemmArgs)]
    return bool(f(ctypes.byref(g)))


@pytest.mark.parametrize("split,c_fits,c_over", [(None, 3584, 3648), ("w2", 1792, 1856), ("x3", 1152, 1216), ("x3f8", 1792, 1920)])
def test_eligibility_stops_at_the_k_tile_table(built_lib, split, c_fits, c_over):
    """a 3x3 convolution with more K-tiles than the table in LDS has records is not eligible for the 256-tile kernel: automatic selection then takes
    the 128-tile kernel, a forced kernel_sel >= 2 and x3f8 / fin_w report an error (f3r_gemm) instead of reading records nobody wrote"""
    entries = built_lib._Z28f3r_gemm256_max_conv_k_tilesv()
    assert entries == cc.TAB_ENTRIES
    fits, over = ConvCase(1, 8, 8, c_fits, 128, 1, split), ConvCase(1, 8, 8, c_over, 128, 1, split)
    assert cc.k_tiles(fits) <= entries < cc.k_tiles(over)
    assert _eligible(built_lib, _gemm_args(fits)) and not _eligible(built_lib, _gemm_args(over))
    assert _eligible(built_lib, _gemm_args(fits, fin=True)) and not _eligible(built_lib, _gemm_args(over, fin=True))
    # the rule is about K-tiles, not about the image: the same at 64 x 64 and at stride 2
    big = dataclasses.replace(over, H=64, W=64, stride=2)
    assert not _eligible(built_lib, _gemm_args(big)) and _eligible(built_lib, _gemm_args(dataclasses.replace(big, Ci=c_fits)))
