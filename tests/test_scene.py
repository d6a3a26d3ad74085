"""Scene assembly and PLY export, the parts that need no GPU: the golden of the reference's `start_visualization`
(tests/golden/scene_cases.pt, tools/make_golden_scene.py) regenerates, the numpy restatement (tests/scene_ref.py) matches it, the
host logic of fast3r_amd/scene.py matches the recorded states, the library exports the entry points, and argument errors are raised
before anything is launched."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_cases as C
import scene_ref as R
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_cases.pt")
needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def restated_frames(name, lut):
    scene = C.build(name)
    s, V = scene["sample"], len(scene["preds"])
    masks = scene["masks"] or [np.ones(sh, np.int8) for sh in scene["shapes"]]
    frames = []
    for i in range(V):
        pred = {k: v[s].numpy() for k, v in scene["preds"][i].items()}
        frames.append(R.frame_data(pred, {"img": scene["views"][i]["img"][s].numpy()}, masks[i], i, V, C.DEFAULT_THRESHOLD, lut))
    return scene, frames


@needs_reference
def test_golden_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_scene.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_golden_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 500 * 1000
    assert golden["tile"] == C.T and set(golden["scenes"]) == set(C.SCENES) and set(golden["ply"]) == set(C.PLY_CASES)
    assert golden["rgb_round_trip"] is True
    for name, g in golden["scenes"].items():
        assert g["restatement_matches"] is True and g["extent_matches_np_percentile"] is True
        assert g["reference"] == C.SCENES[name].get("reference", True)
        assert set(g["states"]) == {"initial"} | {f"s{j:02d}" for j in range(len(C.STATES))}
    lengths = sorted(n for name in ("lengths", "edge") for n in C.SCENES[name]["lengths"])
    T = C.T
    assert set(lengths) >= {1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 17}
    assert any(s["ply"] is None for s in golden["scenes"]["lengths"]["states"].values())


def test_turbo_table_is_shipped_as_data():
    from fast3r_amd import scene
    lut = scene.turbo_lut_u8()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    assert tuple(lut[0]) == (48, 18, 59) and tuple(lut[255]) == (122, 4, 2)   # matplotlib's turbo ends, trunc(x * 255)
    text = open(scene.__file__).read()
    assert "import matplotlib" not in text and "from matplotlib" not in text   # the product ships the table, not the dependency


@pytest.mark.parametrize("name", sorted(C.SCENES))
def test_restatement_matches_the_golden(golden, name):
    from fast3r_amd import scene as S
    g = golden["scenes"][name]
    scene, frames = restated_frames(name, S.turbo_lut_u8())
    assert C.checksum(scene) == g["checksum"], "the seeded inputs differ from the ones the golden was made from"
    V = len(frames)
    for i, fd in enumerate(frames):
        for h in ("global", "local"):
            assert np.array_equal(fd[f"order_{h}"], g["orders"][i][h].numpy().astype(np.int32))
        assert np.float64(fd["max_conf_global"]).tobytes() == np.float64(g["max_conf_global"][i]).tobytes()
        assert fd["is_high_confidence"] == g["is_high_confidence"][i]
    assert R.scene_extent([f["sorted_pts3d_global"] for f in frames]).tobytes() == g["scene_extent"].numpy().tobytes()
    assert bool(R.is_outdoor(frames)) == g["is_outdoor"]
    for key, rec in g["states"].items():
        st = rec["state"]
        mask_sky = g["is_outdoor"] if st["mask_sky"] is None else st["mask_sky"]
        p, c, counts = R.collect(frames, percentile=st["percentile"], mask_sky=mask_sky, color=st["color"], show_global=st["show_global"],
                                 show_local=st["show_local"], show_high_conf=st["show_high_conf"], show_low_conf=st["show_low_conf"],
                                 upto=V - 1 - st["back"], threshold=st["threshold"])
        assert counts == rec["counts"], key
        assert R.digest(None if p is None else R.ply_bytes(p, c)) == rec["ply"], key


def test_host_logic_matches_the_recorded_states(golden):
    """num, the visibility rule and the rainbow colours of fast3r_amd/scene.py against what the reference's nodes held"""
    from fast3r_amd import scene as S
    for name, g in golden["scenes"].items():
        V = len(g["shapes"])
        for key, rec in g["states"].items():
            st = rec["state"]
            mask_sky = g["is_outdoor"] if st["mask_sky"] is None else st["mask_sky"]
            for i, (h, w) in enumerate(g["shapes"]):
                high = g["max_conf_global"][i] >= st["threshold"]
                on = S.view_contributes(i, high, V - 1 - st["back"], st["show_high_conf"], st["show_low_conf"])
                if rec["visible"] is not None:
                    assert rec["visible"][2 * i] == (on and st["show_global"]), (name, key, i)
                    assert rec["visible"][2 * i + 1] == (on and st["show_local"]), (name, key, i)
                if not mask_sky:
                    assert rec["counts"][2 * i] == rec["counts"][2 * i + 1] == S.num_to_show(h * w, st["percentile"]), (name, key, i)
    assert S.num_to_show(1, 100) == 1 and S.num_to_show(4096, 10) == 3686 and S.num_to_show(65, 50) == 32 and S.num_to_show(7, 0) == 7
    for n in (1, 3, 7):
        for i in range(n):
            rb = S.rainbow_color(i, n)
            assert S.rainbow_u8(rb) == tuple(int(x) for x in R.safe_color_conversion(np.array(rb)))
    assert S.rainbow_u8(S.rainbow_color(0, 3)) == (255, 0, 0)
    assert S.is_outdoor_scene([0.3, 0.0, 0.0, 0.0]) and not S.is_outdoor_scene([0.3, 0.0, 0.0, 0.0, 0.0]) and not S.is_outdoor_scene([0.2])


def test_extent_index_arithmetic_is_numpys():
    from fast3r_amd import scene as S
    rs = np.random.RandomState(5)
    for n in (1, 2, 3, 5, 6, 11, 101, 4097, 20000):
        x = rs.randn(n, 3).astype(np.float32)
        for pct in (20, 80):
            assert R.percentile_linear(x, pct).tobytes() == np.percentile(x, pct, axis=0).tobytes(), (n, pct)
    # a length at which the float32 virtual index is no longer exact
    prev, nxt, gamma = S.percentile_indexes(320 * 512 * 512, 80)
    assert gamma.dtype == np.float32 and 0 <= prev <= nxt < 320 * 512 * 512
    x = np.array([[1.0, np.nan, 0.0], [2.0, 0.0, np.inf], [3.0, 1.0, 1.0]], np.float32)
    with np.errstate(invalid="ignore"):
        assert R.percentile_linear(x, 80).tobytes() == np.percentile(x, 80, axis=0).tobytes()


def test_rgb_round_trip_is_the_identity():
    """the reference keeps uint8 / 255.0 and converts back with clip(c * 255).astype(uint8) on the way to the PLY"""
    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal(R.safe_color_conversion(u / 255.0), u)


def test_library_exports_the_scene_entry_points(built_lib):
    from fast3r_amd import _lib
    assert _lib.ABI_VERSION >= 390
    assert built_lib.f3r_version() >= 390
    for n in ("f3r_scene_sort", "f3r_scene_sort_workspace_bytes", "f3r_scene_extent", "f3r_scene_extent_workspace_bytes",
              "f3r_scene_collect_count", "f3r_scene_collect_write", "f3r_ply_pack", "f3r_color_range", "f3r_color_to_u8"):
        assert hasattr(built_lib, n) and n in _lib.SYMBOLS, n
    assert built_lib.f3r_scene_sort_workspace_bytes(0, 0) == 0
    assert built_lib.f3r_scene_sort(None, 1, 1, 1, None, None, 0, None, None, None, None, None, None, None, None) == -1
    assert b"null" in built_lib.f3r_last_error_string()
    assert built_lib.f3r_color_to_u8(0x1000, 4, 0, 2, 2.0, 2.0, 0x2000, None) == -1 and b"zero" in built_lib.f3r_last_error_string()
    assert built_lib.f3r_ply_pack(0x1000, 0x2000, 3, 0x3001, None) == -1


def test_argument_errors_come_before_any_launch():
    import fast3r_amd
    from fast3r_amd import scene as S
    sc = C.build("batch2")
    preds = [dict(p) for p in sc["preds"]]
    del preds[1]["pts3d_local_aligned_to_global"]
    with pytest.raises(KeyError, match="align_local_pts3d_to_global"):
        fast3r_amd.assemble_scene({"preds": preds, "views": sc["views"]})
    bad = [np.ones(s, np.int8) for s in sc["shapes"]]
    bad[2] = np.ones((3, 3), np.int8)
    with pytest.raises(ValueError, match="not_sky"):
        fast3r_amd.assemble_scene(sc["preds"], sc["views"], not_sky=bad)
    with pytest.raises(ValueError, match="not_sky"):
        fast3r_amd.assemble_scene(sc["preds"], sc["views"], not_sky=bad[:2])
    with pytest.raises(ValueError, match="sample"):
        fast3r_amd.assemble_scene(sc["preds"], sc["views"], sample=2)
    empty = S.Scene([], np.zeros(3, np.float32), False, 1.5)
    for p in (-1, 100.5):
        with pytest.raises(ValueError, match="percentile"):
            empty.collect_points(min_conf_thr_percentile=p)
    with pytest.raises(ValueError, match="color"):
        empty.collect_points(color="turbo")
    assert empty.collect_points() == (None, None)
    assert S.color_rule(0.0, 1.0) == 0 and S.color_rule(-1.0, 1.0) == 1 and S.color_rule(-20.0, 280.0) == 2 and S.color_rule(0.0, 1.5) == 2
    assert S.ply_header(3) == R.ply_bytes(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.uint8))[:-45]
