"""Sky detection, the parts that need no GPU: the golden of the reference's `detect_sky_mask` (tests/golden/sky_cases.pt,
tools/make_golden_sky.py) regenerates and the numpy restatement (tests/sky_ref.py) matches it; the integer HSV that both the restatement
and the OpenCV stand-in (tests/cv2_sky_stub.py) compute is pinned on its definition over all 2^24 colours; the library exports the entry
points and rejects bad arguments before any launch; and the product's union-find (fast3r_amd/csrc/f3r_ccl.h), compiled for the host,
labels the stress bitmaps as scipy does under seeded interleavings of concurrent unions."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cv2_sky_stub
import sky_cases as C
import sky_ref as R
from fast3r_amd import _lib, post_ops
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sky_cases.pt")
needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


@needs_reference
def test_golden_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_sky.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_golden_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 200 * 1000
    assert set(golden["cases"]) == {C.case_name(*c) for c in C.CASES} and len(C.CASES) == len(C.SHAPES) * len(C.SCENES)
    assert golden["restatement_matches"] and golden["non_top_component_dropped"]
    assert golden["branch_kinds"] == sorted(("empty", "no_top", "top_all", "top_none", "top_some"))
    assert {(7, 7), (1, 64), (64, 1), (224, 288)} <= set(C.SHAPES)


def test_restatement_matches_the_golden(golden):
    for scene, H, W in C.CASES:
        g = golden["cases"][C.case_name(scene, H, W)]
        img = C.build(scene, H, W)
        assert C.checksum(img) == g["input_sha256"], (scene, H, W)
        not_sky, stats = R.detect_sky_mask(img)
        want = np.unpackbits(g["not_sky_bits"].numpy())[:H * W].reshape(H, W).astype(np.int8)
        assert not_sky.dtype == np.int8 and np.array_equal(not_sky, want), (scene, H, W)
        assert [stats[k] for k in ("sky_pixels", "components", "components_top", "components_kept")] == g["stats"]
        assert stats["branch"] == g["branch"]
        assert np.array_equal(R.detect_sky_mask(img, saturate=True)[0], want)   # inside [-1, 1] saturation changes nothing


def test_single_top_pixel_exercises_the_size_filter():
    """one sky-coloured pixel on row 0 is a 4 x 7 component after the morphology: below 1 % from 48 x 64 up, so it is dropped"""
    not_sky, stats = R.detect_sky_mask(C.build("top_pixel", 48, 64))
    assert stats == {"sky_pixels": 28, "components": 1, "components_top": 1, "components_kept": 0, "branch": "top"} and not_sky.all()


def test_u8_conversion_is_the_references_arithmetic_not_the_inverse_of_imgnorm():
    u = np.arange(256, dtype=np.uint8)
    back = R.to_u8(C.normalise(u))
    assert np.all((back == u) | (back == u - 1)) and back[0] == 0 and back[255] == 255
    n_less = int((back == u - 1).sum())   # measured with this fp32 ImgNorm: 63 of the 256 byte values come back one lower
    print(f"trunc((ImgNorm(u) + 1) * 127.5) == u - 1 for {n_less} of 256 byte values")
    assert 0 < n_less < 256
    # half a unit of margin truncates back exactly (the construction of the all-colours GPU test)
    exact = (u.astype(np.float32) + np.float32(0.5)) / np.float32(127.5) - np.float32(1)
    assert np.array_equal(R.to_u8(exact), u) and np.array_equal(R.to_u8_saturating(exact), u)
    assert np.array_equal(R.to_u8_saturating(np.array([-3.0, np.nan, 7.0, -1.0, 1.0], np.float32)), [0, 0, 255, 0, 255])


def _real_hsv(r, g, b):
    r, g, b = (x.astype(np.float64) for x in (r, g, b))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(v > 0, 255.0 * d / v, 0.0)
        h = np.where(v == r, 30.0 * (g - b) / d, np.where(v == g, 60.0 + 30.0 * (b - r) / d, 120.0 + 30.0 * (r - g) / d))
    h = np.where(d == 0, 0.0, h)
    return np.where(h < 0, h + 180.0, h), s, v


def test_integer_hsv_is_pinned_on_its_definition_over_all_colours():
    """H (circular, 180 steps) and S strictly within 1 of the real-valued HSV for all 2^24 colours (half a rounding plus the error of the
    12-bit tables), V exact, H in 0..179; the OpenCV stand-in and the restatement, written apart, agree everywhere."""
    g, b = (x.ravel() for x in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    worst_h = worst_s = 0.0
    for r0 in range(0, 256, 16):
        r = np.repeat(np.arange(r0, r0 + 16), 256 * 256)
        gg, bb = np.tile(g, 16), np.tile(b, 16)
        h, s, v = R.hsv_u8(r, gg, bb)
        hr, sr, vr = _real_hsv(r, gg, bb)
        assert np.array_equal(v, vr.astype(np.int32)) and h.min() >= 0 and h.max() <= 179 and s.min() >= 0 and s.max() <= 255
        dh = np.abs(h - hr)
        worst_h = max(worst_h, float(np.minimum(dh, 180.0 - dh).max()))
        worst_s = max(worst_s, float(np.abs(s - sr).max()))
        stub = cv2_sky_stub.cvtColor(cv2_sky_stub.cvtColor(np.stack([r, gg, bb], axis=-1).astype(np.uint8)[None], cv2_sky_stub.COLOR_RGB2BGR),
                                     cv2_sky_stub.COLOR_BGR2HSV)[0]
        assert np.array_equal(stub[:, 0], h) and np.array_equal(stub[:, 1], s) and np.array_equal(stub[:, 2], v)
    print(f"integer HSV vs real-valued: worst |dH| = {worst_h:.4f}, worst |dS| = {worst_s:.4f}")
    assert worst_h < 1 and worst_s < 1


def test_hsv_anchors():
    def hsv(r, g, b):
        return tuple(int(x) for x in R.hsv_u8(np.array(r), np.array(g), np.array(b)))
    assert hsv(255, 0, 0) == (0, 255, 255) and hsv(0, 255, 0) == (60, 255, 255) and hsv(0, 0, 255) == (120, 255, 255)
    assert hsv(255, 255, 0) == (30, 255, 255) and hsv(0, 255, 255) == (90, 255, 255) and hsv(255, 0, 255) == (150, 255, 255)
    assert hsv(0, 0, 0) == (0, 0, 0) and hsv(128, 128, 128) == (0, 0, 128) and hsv(255, 255, 255) == (0, 0, 255)
    # v == r == g: the r test comes first, h0 = g - b = d -> 30; v == g == b: h0 = b - r + 2 d = 3 d -> 90; v == r == b: g - b = -d -> 150
    # s = (100 * sdiv[200] + 2048) >> 12 with sdiv[200] = rint(5222.4) = 5222: 524248 >> 12 = 127 (the real value is 127.5)
    assert hsv(200, 200, 100) == (30, 127, 200) and hsv(100, 200, 200) == (90, 127, 200) and hsv(200, 100, 200) == (150, 127, 200)
    assert hsv(100, 150, 230) == (108, 144, 230)   # tests/sky_cases.py's sky colour: 217 degrees / 2, inside the blue range


def test_morphology_restatement_equals_the_stand_in_on_mixed_values():
    """the stand-in's max / min filters run on 0 / 1 / 255, the restatement on booleans: same non-zero set, borders ignored"""
    rng = np.random.default_rng(5)
    k = np.ones((7, 7), np.uint8)
    for H, W, dens in ((7, 7, 0.3), (5, 9, 0.5), (40, 61, 0.02), (40, 61, 0.5), (1, 30, 0.4), (30, 1, 0.4)):
        m = (rng.random((H, W)) < dens).astype(np.uint8) * rng.choice(np.array([1, 255], np.uint8), size=(H, W))
        got = cv2_sky_stub.morphologyEx(cv2_sky_stub.dilate(m, k, iterations=1), cv2_sky_stub.MORPH_OPEN, k)
        assert np.array_equal(got != 0, R.morphology(m != 0))
    one = np.zeros((20, 20), bool)
    one[0, 0] = True   # a corner pixel survives: the erosion at the edge looks only at in-image neighbours
    assert np.array_equal(R.morphology(one), np.pad(np.ones((4, 4), bool), ((0, 16), (0, 16))))


def test_library_exports_the_sky_entry_points(built_lib):
    assert _lib.ABI_VERSION >= 400
    assert built_lib.f3r_version() >= 400
    for name, arity in (("f3r_sky_workspace_bytes", 4), ("f3r_sky_detect", 14)):
        assert hasattr(built_lib, name) and len(_lib.SYMBOLS[name][1]) == arity
    import fast3r_amd
    from fast3r_amd import sky
    assert fast3r_amd.detect_sky_mask is sky.detect_sky_mask and fast3r_amd.detect_sky_masks is sky.detect_sky_masks
    assert fast3r_amd.label_components is sky.label_components
    # 48 x 64: 48 words; label needs two bitmaps, the parents and the top-row counters
    assert built_lib.f3r_sky_workspace_bytes(48, 48 * 64, 64, 7) == 2 * 512 + 48 * 64 * 4 + 256
    assert built_lib.f3r_sky_workspace_bytes(48, 48 * 64, 64, 3) == 2 * 512
    assert built_lib.f3r_sky_workspace_bytes(0, 1, 1, 7) == 0


def test_argument_errors_come_before_any_launch(built_lib):
    """no GPU here: every call below must return F3R_ERR_ARG without touching the device"""
    hw = (ctypes.c_int64 * 2)(48, 64)
    ok = dict(table=0x1000, hw=hw, n=1, pt=3, wt=1, words=48, pix=48 * 64, width=64, stages=7, ws=0x2000, wsb=1 << 20, stats=0x3000, bits=None)

    def call(**kw):
        a = dict(ok, **kw)
        return built_lib.f3r_sky_detect(a["table"], a["hw"], a["n"], a["pt"], a["wt"], a["words"], a["pix"], a["width"], a["stages"], a["ws"],
                                        a["wsb"], a["stats"], a["bits"], None)
    for bad in (dict(table=None), dict(hw=None), dict(ws=None), dict(n=0), dict(stages=0), dict(stages=8), dict(stats=None),
                dict(stages=3, bits=None), dict(words=47), dict(pix=48 * 64 + 1), dict(width=63), dict(pt=4), dict(wt=2), dict(wsb=16),
                dict(hw=(ctypes.c_int64 * 2)(0, 64)), dict(hw=(ctypes.c_int64 * 2)(48, 0)), dict(hw=(ctypes.c_int64 * 2)(1 << 16, 1 << 16))):
        assert call(**bad) == -1, bad
        assert b"f3r_sky_detect" in built_lib.f3r_last_error_string()
    with pytest.raises(ValueError, match="one shape per view"):
        post_ops.sky_detect([torch.zeros(3, 4)], [], 7)
    with pytest.raises(ValueError, match="H, W >= 1"):
        post_ops.sky_detect([torch.zeros(3, 0)], [(0, 4)], 7)
    from fast3r_amd import sky
    with pytest.raises(ValueError, match=r"\(H, W, 3\)"):
        sky.detect_sky_mask(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="float32"):   # the reference would do the 8-bit conversion in double: not reproduced, so refused
        sky.detect_sky_mask(np.zeros((4, 4, 3), np.float64))
    with pytest.raises(ValueError, match="bitmap"):
        sky.label_components(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="no views"):
        sky.detect_sky_masks([])


def test_assemble_scene_names_the_accepted_not_sky_values():
    from fast3r_amd import assemble_scene
    z = torch.zeros(1, 4, 4)
    preds = [{"pts3d_local_aligned_to_global": z, "pts3d_in_other_view": z, "conf": z, "conf_local": z}]
    with pytest.raises(ValueError, match="'detect'"):
        assemble_scene(preds, [{"img": torch.zeros(1, 3, 4, 4)}], not_sky="auto")


@pytest.fixture(scope="module")
def ccl_host(tmp_path_factory):
    """the product's union-find (f3r_ccl.h) compiled for the host by tests/csrc/ccl_host.cpp"""
    so = str(tmp_path_factory.mktemp("ccl") / "libccl_host.so")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "csrc", "ccl_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    lib.ccl_host_label.restype = ctypes.c_longlong
    lib.ccl_host_label.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint64, ctypes.c_void_p]
    return lib


def test_host_compiled_union_find_matches_scipy_under_interleavings(ccl_host):
    """every stress bitmap, with 1, 7, 64 and 4096 unions in flight whose single-access steps are interleaved in a seeded order: the roots
    are scipy's partition with the smallest index as label, every time, and no run exceeds the step bound of the termination argument"""
    for name, m in C.stress_bitmaps().items():
        H, W = m.shape
        bits = np.ascontiguousarray(R.pack_bits(m))
        want, _ = R.label_roots(m)
        for in_flight, seed in ((1, 11), (7, 12), (64, 13), (4096, 14), (4096, 15)):
            roots = np.full((H, W), -7, dtype=np.int32)
            steps = ccl_host.ccl_host_label(bits.ctypes.data, H, W, in_flight, seed, roots.ctypes.data)
            assert steps >= 0, (name, in_flight, "step bound exceeded")
            assert np.array_equal(roots, want), (name, in_flight, seed)


def test_restated_labelling_helpers():
    m = C.diagonal_pair(20, 20)
    roots, n = R.label_roots(m)
    assert n == 2 and sorted(set(roots[m].tolist())) == [7 * 20 + 7, 10 * 20 + 10] and (roots[~m] == -1).all()
    assert R.label_roots(C.spiral(96, 128))[1] == 1 and R.label_roots(C.spiral(37, 131))[1] == 1 and C.spiral(96, 128).sum() > 6000
    assert R.label_roots(C.checkerboard(6, 8))[1] == 24 and R.label_roots(C.serpentine(9, 8))[1] == 1 and R.label_roots(C.comb(9, 9))[1] == 1
    assert np.array_equal(R.pack_bits(np.ones((1, 65), bool)), np.array([[2 ** 64 - 1, 1]], dtype=np.uint64))
