"""Confidence cleaning, the parts that need no GPU: the torch restatement (tests/clean_ref.py) against the reference's own
BasePCOptimizer.clean_pointcloud (tests/golden/clean_cases.npz, written by tools/make_golden_clean.py) on every untainted pixel, the stored
margin conditions re-derived, the order case, and the host logic of fast3r_amd/clean.py: neighbour lists, the table, every refusal."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import clean_cases as C
import clean_ref as R
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clean_cases.npz")
NEW_SYMBOLS = {"f3r_clean_workspace_bytes": 1, "f3r_clean_confidence": 20}


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


def split(flat, shapes):
    out, off = [], 0
    for h, w in shapes:
        out.append(flat[off:off + h * w].reshape(h, w))
        off += h * w
    return out


def bits(packed, shapes):
    total = sum(h * w for h, w in shapes)
    return split(np.unpackbits(packed)[:total].astype(bool), shapes)


# ------------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")
def test_golden_generator_reproduces_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_clean.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_restatement_equals_the_reference_on_every_untainted_pixel(golden, name):
    s = C.golden_scene(name)
    shapes = s["shapes"]
    tainted = bits(golden[f"{name}_tainted"], shapes)
    assert int(golden[f"{name}_seed"]) == C.GOLDEN[name][1]
    ref32 = split(golden[f"{name}_conf32"], shapes)
    got32, lowered32 = R.clean_ref(s)
    for i in range(len(shapes)):
        ok = ~tainted[i]
        assert got32[i].dtype == torch.float32 and got32[i].numpy()[ok].tobytes() == ref32[i][ok].tobytes(), (name, i)
    changed64 = bits(golden[f"{name}_changed64"], shapes)
    got64, _ = R.clean_ref(s, dtype=torch.float64)
    for i in range(len(shapes)):
        ok = ~tainted[i]
        c = s["conf"][i].astype(np.float64)
        want = np.where(changed64[i], np.minimum(c, float(s["max_bad_conf"])), c)
        assert got64[i].dtype == torch.float64 and got64[i].numpy()[ok].tobytes() == want[ok].tobytes(), (name, i)
    # not vacuous: the untainted pixels hold nearly all of what is lowered, and the counts of the fixture are the restatement's up to the tainted ones
    n_tainted = sum(int(t.sum()) for t in tainted)
    assert abs(sum(lowered32) - int(golden[f"{name}_lowered"].sum())) <= n_tainted and sum(lowered32) > 10 * max(n_tainted, 1)
    if s["max_bad_conf"] > 0:  # some flagged pixels lie below max_bad_conf and keep their value
        kept_floaters = sum(int(((g.numpy() == c) & f & (c < s["max_bad_conf"])).sum()) for g, c, f in zip(got32, s["conf"], s["floater"]))
        assert kept_floaters > 0


@pytest.mark.parametrize("name", list(C.GOLDEN))
def test_stored_margin_conditions_are_rederived(golden, name):
    s = C.golden_scene(name)
    shapes = s["shapes"]
    total = sum(h * w for h, w in shapes)
    d = float(golden[f"{name}_d"])
    # the restatement's own fp32 - fp64 shift is of the size of the reference's: the 16 d band covers either
    p32, p64 = R.projections(s, torch.float32), R.projections(s, torch.float64)
    mine = R.pixel_shift(s, {k: v[:2] for k, v in p32.items()}, {k: v[:2] for k, v in p64.items()})
    assert 0 < d < 1e-4 and 0 < mine < 4 * d
    m = R.margins(s, d)
    tainted = bits(golden[f"{name}_tainted"], shapes)
    assert all(np.array_equal(t.numpy(), g) for t, g in zip(m["tainted"], tainted))
    share = sum(int(t.sum()) for t in tainted) / total
    assert share == float(golden[f"{name}_tainted_share"]) <= float(golden["tainted_cap"]) == 0.05 and bool(golden["conditions_ok"])
    for i in range(len(shapes)):  # the definitions
        f = m["fragile"][i]
        assert torch.equal(f, (m["px"][i] < 16 * d) | (m["rel"][i] < 1e-5) | (m["absz"][i] < 16 * d)) and bool((m["tainted"][i] | ~f).all())
    lowered = golden[f"{name}_lowered"]
    assert (lowered[1:] >= 8).all() and lowered.sum() >= 0.02 * total
    changed32 = [a != c for a, c in zip(split(golden[f"{name}_conf32"], shapes), s["conf"])]
    changed64 = bits(golden[f"{name}_changed64"], shapes)
    assert all(np.array_equal(a[~t], b[~t]) for a, b, t in zip(changed32, changed64, tainted))
    assert [int(c.sum()) for c in changed32] == lowered.tolist()


def test_golden_holds_data_only():
    assert os.path.getsize(GOLDEN) < 200 * 1000
    with np.load(GOLDEN) as f:
        assert all(f[k].dtype.kind in "bfiu" for k in f.files)


def test_order_case_on_the_restatement():
    s = C.order_case()
    seq, seq_lowered = R.clean_ref(s)
    jac, jac_lowered = R.clean_ref(s, jacobi=True)
    assert seq_lowered == [1, 0, 0] and float(seq[0][0, 0]) == 0.0 and float(seq[1][0, 0]) == 1.0
    assert jac_lowered == [1, 1, 0] and float(jac[1][0, 0]) == 0.0                     # a Jacobi evaluation gives another answer
    rev, rev_lowered = R.clean_ref(C.reversed_views(s))
    assert rev_lowered == [0, 1, 1] and float(rev[1][0, 0]) == 0.0 and float(rev[2][0, 0]) == 0.0
    for a in (seq, jac, rev):                                                        # nothing else moves
        assert sum(int((x != 5.0).sum()) for x in a) == 2
    # within one view the order of the neighbours does not matter (the j-loop is an OR)
    g = C.golden_scene("six_tol3")
    fwd, _ = R.clean_ref(g)
    bwd, _ = R.clean_ref(g, [list(reversed(n)) for n in C.complete(6)])
    assert all(torch.equal(a, b) for a, b in zip(fwd, bwd))


def test_pose_inverse_closed_form():
    rs = np.random.RandomState(0)
    P = np.tile(np.eye(4, dtype=np.float32), (5, 1, 1))
    P[:, :3, :] = rs.uniform(-2, 2, (5, 3, 4)).astype(np.float32)
    inv = R.pose_inverse(P)
    full = np.linalg.inv(P.astype(np.float64))
    assert np.allclose(inv, full[:, :3, :], rtol=1e-9, atol=1e-12)
    assert np.array_equal(R.pose_inverse(np.eye(4, dtype=np.float32)[None])[0], np.eye(4)[:3])


# ------------------------------------------------------------------------------------------------------------------- host logic
def test_neighbour_lists():
    from fast3r_amd import clean, scene_graph_pairs
    starts, nbr = clean.neighbour_lists("complete", 4)
    assert starts == [0, 3, 6, 9, 12] and nbr.dtype == np.int32 and nbr.tolist() == [1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2]
    assert clean.neighbour_lists("complete", 1)[0] == [0, 0] and clean.neighbour_lists("complete", 1)[1].size == 0
    starts, nbr = clean.neighbour_lists("swin-1", 5)
    assert starts == [0, 2, 4, 6, 8, 10] and nbr.tolist() == [1, 4, 0, 2, 1, 3, 2, 4, 0, 3]
    for graph in ("swin-2", "oneref-1", "swin"):
        for n in (2, 3, 6):
            if graph == "oneref-1" and n < 2:
                continue
            starts, nbr = clean.neighbour_lists(graph, n)
            want = C.lists_of(scene_graph_pairs(n, graph, symmetrize=False).tolist(), n)
            got = [nbr[starts[i]:starts[i + 1]].tolist() for i in range(n)]
            assert got == want and all(i not in row and row == sorted(set(row)) for i, row in enumerate(got))
            assert all((i in got[j]) for i, row in enumerate(got) for j in row)      # both directions
    starts, nbr = clean.neighbour_lists([(2, 0), (0, 2), (1, 1), (0, 1)], 3)        # repeats and a self pair
    assert starts == [0, 2, 3, 4] and nbr.tolist() == [1, 2, 0, 0]
    starts, nbr = clean.neighbour_lists(torch.tensor([[0, 1]]), 3)
    assert starts == [0, 1, 2, 2] and nbr.tolist() == [1, 0]
    assert clean.neighbour_lists([], 2) [0] == [0, 0, 0]
    for bad in ([(0, 3)], [(-1, 0)], [(0, 1, 2)], [(0.0, 1.0)]):
        with pytest.raises(ValueError, match="pairs"):
            clean.neighbour_lists(bad, 3)
    with pytest.raises(ValueError, match="scene graph"):
        clean.neighbour_lists("ring", 3)


def test_table_building():
    from fast3r_amd import post_ops
    table, total = post_ops.clean_table([(2, 3), (4, 1), (1, 1)], [0, 2, 3, 4])
    assert table.dtype == torch.int64 and total == 11 and table.tolist() == [2, 3, 0, 4, 1, 6, 1, 1, 10, 0, 2, 3, 4]
    assert post_ops.clean_frame_id("world") == 0 and post_ops.clean_frame_id("camera") == 1
    with pytest.raises(ValueError, match="frame"):
        post_ops.clean_frame_id("object")


def scene_args(n=2, H=3, W=4):
    return [[torch.zeros(H, W, 3) for _ in range(n)], [torch.ones(H, W) for _ in range(n)], [torch.ones(H, W) for _ in range(n)],
            torch.eye(4).repeat(n, 1, 1), torch.ones(n)]


def test_clean_confidences_refuses_bad_arguments_before_any_device_work():
    import fast3r_amd
    bad_calls = [
        (lambda a: a, {"tol": 1.0}, "tol"), (lambda a: a, {"tol": -0.1}, "tol"), (lambda a: a, {"tol": float("nan")}, "tol"),
        (lambda a: a, {"max_bad_conf": float("nan")}, "max_bad_conf"), (lambda a: a, {"frame": "object"}, "frame"),
        (lambda a: a, {"pairs": [(0, 2)]}, "pairs"), (lambda a: a, {"pairs": "ring"}, "scene graph"),
        (lambda a: [a[0][:1]] + a[1:], {}, "pts3d has 1 entries"), (lambda a: a[:2] + [a[2][:1]] + a[3:], {}, "depthmaps has 1"),
        (lambda a: a[:3] + [a[3][:1]] + a[4:], {}, "im_poses has 1"), (lambda a: a[:4] + [torch.ones(3)], {}, "focals"),
        (lambda a: a[:4] + [torch.ones(2, 3)], {}, "focals"), (lambda a: a, {"pp": torch.zeros(3, 2)}, "pp"),
        (lambda a: [[torch.zeros(3, 5, 3)] * 2] + a[1:], {}, "pts3d of view 0"), (lambda a: a[:2] + [[torch.ones(4, 3)] * 2] + a[3:], {}, "depthmap of view 0"),
        (lambda a: a[:1] + [[torch.ones(12)] * 2] + a[2:], {}, r"\(H, W\)"), (lambda a: a[:3] + [torch.eye(3).repeat(2, 1, 1)] + a[4:], {}, r"\(4, 4\)"),
        (lambda a: [[], [], [], torch.zeros(0, 4, 4), torch.zeros(0)], {}, "at least one view"),
    ]
    for change, kw, word in bad_calls:
        with pytest.raises(ValueError, match=word):
            fast3r_amd.clean_confidences(*change(scene_args()), **kw)


def test_clean_pointcloud_refuses_bad_arguments_before_any_device_work():
    import fast3r_amd
    p = [{"pts3d_local": torch.zeros(1, 4, 5, 3), "conf_local": torch.ones(1, 4, 5), "pts3d_in_other_view": torch.zeros(1, 4, 5, 3),
          "conf": torch.ones(1, 4, 5)} for _ in range(2)]
    for kw, exc, word in (({"head": "both"}, ValueError, "head"), ({"tol": 1}, ValueError, "tol"), ({"sample": 1}, ValueError, "sample"),
                          ({"sample": -1}, ValueError, "sample"), ({"pairs": [(0, 5)]}, ValueError, "pairs"), ({"pairs": "star"}, ValueError, "scene graph"),
                          ({"poses": torch.eye(4).repeat(2, 1, 1)}, ValueError, "together"), ({"max_bad_conf": float("nan")}, ValueError, "max_bad_conf")):
        with pytest.raises(exc, match=word):
            fast3r_amd.clean_pointcloud(p, **kw)
    with pytest.raises(ValueError, match="at least one view"):
        fast3r_amd.clean_pointcloud([])
    with pytest.raises(ValueError, match="preds"):
        fast3r_amd.clean_pointcloud({"views": []})
    with pytest.raises(KeyError, match="conf_local"):
        fast3r_amd.clean_pointcloud([{k: v for k, v in q.items() if k != "conf_local"} for q in p])
    with pytest.raises(ValueError, match="differ in size"):
        fast3r_amd.clean_pointcloud([dict(q, conf_local=torch.ones(1, 4, 6)) for q in p])
    assert isinstance(fast3r_amd.MultiViewDUSt3RLitModule.__dict__["clean_pointcloud"], staticmethod)
    assert fast3r_amd.CleanedCloud is fast3r_amd.clean.CleanedCloud


# ------------------------------------------------------------------------------------------------------------------- the library
def test_library_side(built_lib):
    from fast3r_amd import _lib, post_ops
    for name, arity in NEW_SYMBOLS.items():
        assert len(_lib.SYMBOLS[name][1]) == arity and _lib.symbol_since(name) == 0 and _lib.if_present(name)
        assert name in _lib.SYMBOL_IF_PRESENT_CLEAN and name not in _lib.SYMBOL_IF_PRESENT_MATCH and _lib.entry(name) is getattr(built_lib, name)
    assert set(_lib.SYMBOL_IF_PRESENT_CLEAN) == set(NEW_SYMBOLS) and not _lib.if_present("f3r_gemm") and _lib.if_present("f3r_match_index")
    assert built_lib.f3r_version() == 430                                     # unchanged
    build = open(os.path.join(ROOT, "fast3r_amd", "csrc", "build.sh")).read()
    assert '[ "$f" = f3r_clean ] && extra="-ffp-contract=off"' in build and "obj/f3r_clean.o" in build
    assert built_lib.f3r_clean_workspace_bytes(0) == 0 and built_lib.f3r_clean_workspace_bytes(-3) == 0
    assert built_lib.f3r_clean_workspace_bytes(1) == 256 and built_lib.f3r_clean_workspace_bytes(320) == 320 * 80 and built_lib.f3r_clean_workspace_bytes(1500) == 120064
    with pytest.raises(_lib.F3RError):                                        # CPU tensors: no fallback
        post_ops.clean_confidence(torch.zeros(4, 3), torch.zeros(4), torch.zeros(4), torch.eye(4)[None], torch.ones(1, 4), [(2, 2)], [0, 0], [])


def test_entry_point_refuses_before_any_launch(built_lib):
    """every refusal of f3r_clean_confidence with pointers that are never dereferenced: the host tables decide"""
    err = lambda: built_lib.f3r_last_error_string()  # noqa: E731

    def call(table, nbr, N, tol=0.001, max_bad=0.0, frame=0, ws=1 << 20, ptrs=0x1000, ws_ptr=0x1000):
        t, n = np.asarray(table, dtype=np.int64), np.asarray(nbr, dtype=np.int32)
        return built_lib.f3r_clean_confidence(ptrs, ptrs, ptrs, ptrs, ptrs, ptrs, t.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), N, 0x1000,
                                              n.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(nbr), tol, max_bad, frame, ptrs, ptrs, ptrs, ws_ptr, ws,
                                              None)
    good = [2, 3, 0, 2, 3, 6, 0, 1, 2]
    assert call(good, [1, 0], 0) == -1 and b"at least one view" in err()
    assert call(good, [1, 0], 2, ptrs=None) == -1 and b"null pointer" in err()
    assert call([0, 3, 0, 2, 3, 0, 0, 1, 2], [1, 0], 2) == -1 and b"view 0 is 0 x 3" in err()
    assert call([1 << 16, 1 << 15, 0, 2, 3, 1 << 31, 0, 1, 2], [1, 0], 2) == -1 and b"2^31 - 1" in err()       # 2^31 pixels
    assert call([(1 << 24) + 1, 1, 0, 2, 3, (1 << 24) + 1, 0, 1, 2], [1, 0], 2) == -1 and b"2^24" in err()     # a side that is not exact in fp32
    assert call([2, 3, 0, 2, 3, 5, 0, 1, 2], [1, 0], 2) == -1 and b"running sum" in err()
    assert call([2, 3, 1, 2, 3, 7, 0, 1, 2], [1, 0], 2) == -1 and b"running sum" in err()
    assert call(good, [0, 0], 2) == -1 and b"not its own neighbour" in err()
    assert call(good, [1, 2], 2) == -1 and b"neighbour 2 of view 1" in err()
    assert call(good, [-1, 0], 2) == -1 and b"neighbour -1" in err()
    assert call([2, 3, 0, 2, 3, 6, 2, 3, 12, 0, 2, 3, 4], [2, 1, 0, 0], 3) == -1 and b"must ascend" in err()
    assert call([2, 3, 0, 2, 3, 6, 2, 3, 12, 0, 2, 3, 4], [1, 1, 0, 0], 3) == -1 and b"must ascend" in err()    # a view twice
    assert call([2, 3, 0, 2, 3, 6, 1, 1, 2], [1, 0], 2) == -1 and b"start at 0" in err()
    assert call([2, 3, 0, 2, 3, 6, 0, 1, 3], [1, 0], 2) == -1 and b"end at n_nbr" in err()
    assert call([2, 3, 0, 2, 3, 6, 0, 2, 2], [1, 0], 2) == -1                                                    # view 0's list holds itself
    assert call([2, 3, 0, 2, 3, 6, 2, 3, 12, 0, 2, 1, 2], [1, 2], 3) == -1 and b"neighbour list of view 1" in err()  # starts that descend
    for tol in (1.0, -1e-9, float("nan"), float("inf")):
        assert call(good, [1, 0], 2, tol=tol) == -1 and b"tol" in err()
    assert call(good, [1, 0], 2, max_bad=float("nan")) == -1 and b"max_bad_conf is NaN" in err()
    assert call(good, [1, 0], 2, frame=2) == -1 and b"frame" in err()
    assert call(good, [1, 0], 2, ws=255) == -1 and b"workspace" in err()
    assert call(good, [1, 0], 2, ws_ptr=0x1010) == -1 and b"workspace" in err()
    assert call(good, [1, 0], 2, ptrs=0x1002) == -1 and b"misaligned" in err()
