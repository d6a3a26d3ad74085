"""Mesh export, the parts that need no GPU: the golden of the reference's `pts3d_to_trimesh` / `cat_meshes`
(tests/golden/mesh_cases.pt, tools/make_golden_mesh.py) regenerates, the numpy restatement (tests/mesh_ref.py) matches it, the PLY
layout, the library exports the entry points, and argument errors are return codes before anything is launched."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mesh_cases as C
import mesh_ref as R
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_cases.pt")
needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def matches(stored, a):
    """a golden entry (a whole tensor, or dtype / shape / SHA-256) against an array, bit for bit"""
    a = np.ascontiguousarray(a)
    if torch.is_tensor(stored):
        s = stored.numpy()
        return s.dtype == a.dtype and s.shape == a.shape and s.tobytes() == a.tobytes()
    return stored["dtype"] == str(a.dtype) and tuple(stored["shape"]) == a.shape and stored["sha256"] == R.digest(a)[1]


def parse_mesh_ply(raw):
    """the 20-line reader of the layout in fast3r_amd/mesh.py -> (vertices, faces int32, face_colors, bytes the header implies)"""
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    counts, props, cur = {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur], props[cur] = int(w[2]), []
        elif w[:1] == ["property"]:
            props[cur].append(" ".join(w[1:]))
    assert props["vertex"] == ["float x", "float y", "float z"]
    assert props["face"] == ["list uchar int vertex_indices", "uchar red", "uchar green", "uchar blue"]
    nv, nf = counts["vertex"], counts["face"]
    v = np.frombuffer(raw, "<f4", nv * 3, end).reshape(nv, 3)
    f = np.frombuffer(raw, np.dtype([("n", "u1"), ("idx", "<i4", 3), ("rgb", "u1", 3)]), nf, end + nv * 12)
    assert (f["n"] == 3).all()
    return v, f["idx"], f["rgb"], end + nv * 12 + nf * 16


@needs_reference
def test_golden_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_mesh.py"), "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_golden_is_small_and_complete(golden):
    assert os.path.getsize(GOLDEN) < 500 * 1000
    assert golden["tile"] == C.T and set(golden["cases"]) == set(C.CASES)
    for name, g in golden["cases"].items():
        assert g["restatement_matches"] is True and g["mesh"]["restatement_matches"] is True, name
    shapes = {tuple(s) for r in C.CASES.values() for s in r["shapes"]}
    assert shapes >= {(2, 2), (1, 5), (5, 1), (2, 9), (9, 2), (3, 65), (5, 67)}
    quads = {(h - 1) * (w - 1) for h, w in shapes}
    assert C.T in quads and C.T + 1 in quads
    assert {r["pct"] for r in C.CASES.values()} >= {0, 10, 80, 99.5, 100}
    # the single invalid pixel takes its 6 / 3 / 1 / 2 triangles, in both windings; none valid and the checkerboard leave nothing
    per_view = dict(zip(C.MASK_KINDS, golden["cases"]["masks"]["mask_only"]["faces_per_view"].tolist()))
    full = 4 * (C.MASK_SHAPE[0] - 1) * (C.MASK_SHAPE[1] - 1)
    assert per_view["none"] == per_view["checker"] == 0
    for kind, removed in C.MASK_REMOVES.items():
        assert per_view[kind] == full - 2 * removed, kind
    assert golden["cases"]["no_quads"]["mesh"]["faces_per_view"].tolist() == [0, 0]
    assert golden["cases"]["three_views"]["mesh"]["faces_per_view"][1] == 0 and golden["cases"]["three_views"]["mesh"]["faces_per_view"][2] > 0
    thr = golden["cases"]["confs"]["mesh"]["thresholds"].numpy()
    assert np.isnan(thr[2]) and thr[0] == 2.5 and np.isfinite(thr[[0, 1, 3, 4]]).all()
    assert golden["cases"]["confs"]["mesh"]["faces_per_view"][:3].tolist() == [0, 0, 0]


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_restatement_matches_the_golden(golden, name):
    g = golden["cases"][name]
    case = C.build(name)
    assert C.checksum(case) == g["checksum"], "the seeded inputs differ from the ones the golden was made from"
    views = C.numpy_views(case)
    runs = [("mesh", case["pct"])] + ([("mask_only", None)] if "mask_only" in g else [])
    for key, pct in runs:
        m = R.build(views, pct, case["masks"])
        for k in ("vertices", "faces", "face_colors"):
            assert matches(g[key][k], m[k]), (key, k)
        assert matches(g[key]["thresholds"], m["thresholds"]) and matches(g[key]["faces_per_view"], m["faces_per_view"]), key
        assert m["vertices"].dtype == np.float32 and m["faces"].dtype == np.int64 and m["face_colors"].dtype == np.uint8


def test_restated_threshold_is_np_percentile():
    from fast3r_amd import scene as S
    rs = np.random.RandomState(7)
    for n in (1, 2, 3, 5, 30, 101, 4097):
        x = (1.0 + np.exp(rs.randn(n))).astype(np.float32)
        for pct in (0, 10, 50, 80, 99.5, 100):
            want = np.percentile(x, pct)
            assert np.float32(R.threshold(x, pct)).tobytes() == np.float32(want).tobytes(), (n, pct)
            # what build_mesh hands the kernel: the two ranks and the weight of fast3r_amd.scene.percentile_indexes
            lo, hi, gamma = S.percentile_indexes(n, pct)
            xs = np.sort(x)
            assert S.percentile_finish(xs[lo], xs[hi], gamma).astype(np.float32).tobytes() == np.float32(want).tobytes(), (n, pct)


def test_restated_options():
    """what has no reference counterpart, on the restatement itself: drop_unreferenced, double_sided=False, flip_axes"""
    case = C.build("three_views")
    views = C.numpy_views(case)
    full = R.build(views, case["pct"], case["masks"])
    one = R.build(views, case["pct"], case["masks"], double_sided=False)
    assert len(one["faces"]) * 2 == len(full["faces"]) and (one["faces_per_view"] * 2 == full["faces_per_view"]).all()
    drop = R.build(views, case["pct"], case["masks"], drop_unreferenced=True)
    assert len(drop["vertices"]) < len(full["vertices"]) and len(drop["faces"]) == len(full["faces"])
    assert np.array_equal(np.unique(drop["faces"]), np.arange(len(drop["vertices"])))
    vbase = np.cumsum([0] + [h * w for h, w in case["shapes"]])
    assert np.array_equal(drop["vertices"][drop["faces"]], full["vertices"][full["faces"]])
    assert drop["vertices_per_view"].tolist() == [len(np.unique(full["faces"][(full["faces"][:, 0] >= vbase[i]) & (full["faces"][:, 0] < vbase[i + 1])]))
                                                  for i in range(3)]
    flip = R.build(views, case["pct"], case["masks"], flip_axes=True)
    v = full["vertices"].copy()           # the notebook's two assignments
    v[:, [1, 2]] = v[:, [2, 1]]
    v[:, 2] = -v[:, 2]
    assert flip["vertices"].tobytes() == v.tobytes()
    checker = R.build(C.numpy_views(C.build("masks"))[2:3], None, [C.build("masks")["masks"][2]], drop_unreferenced=True)
    assert checker["vertices"].shape == (0, 3) and checker["faces"].shape == (0, 3)


def test_ply_header_and_record_sizes():
    from fast3r_amd import mesh as M
    assert M.MESH_VERTEX_BYTES == 12 and M.MESH_FACE_BYTES == 16
    head = M.mesh_ply_header(5, 7)
    assert head == (b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\n"
                    b"element face 7\nproperty list uchar int vertex_indices\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                    b"end_header\n")
    v = np.zeros((5, 3), np.float32)
    f = np.zeros((7, 3), np.int64)
    c = np.zeros((7, 3), np.uint8)
    raw = R.ply_bytes(v, f, c)
    assert raw[:len(head)] == head and len(raw) == len(head) + 5 * 12 + 7 * 16
    assert M.mesh_ply_header(0, 0) == R.ply_bytes(v[:0], f[:0], c[:0])


def test_ply_round_trip_on_restated_data():
    case = C.build("three_views")
    m = R.build(C.numpy_views(case), case["pct"], case["masks"])
    raw = R.ply_bytes(m["vertices"], m["faces"], m["face_colors"])
    v, f, c, implied = parse_mesh_ply(raw)
    assert implied == len(raw)
    assert v.tobytes() == m["vertices"].tobytes() and np.array_equal(f, m["faces"]) and np.array_equal(c, m["face_colors"])
    assert f.dtype == np.dtype("<i4") and len(f) > 0


def test_library_exports_the_mesh_entry_points(built_lib):
    from fast3r_amd import _lib
    assert _lib.ABI_VERSION >= 410
    assert built_lib.f3r_version() >= 410
    for n in ("f3r_mesh_workspace_bytes", "f3r_mesh_threshold", "f3r_mesh_count", "f3r_mesh_write", "f3r_mesh_ply_pack"):
        assert hasattr(built_lib, n) and n in _lib.SYMBOLS, n
    import fast3r_amd
    for n in ("pts3d_to_trimesh", "cat_meshes", "build_mesh", "generate_mesh_ply_bytes", "save_mesh_ply", "Mesh"):
        assert hasattr(fast3r_amd, n), n


def test_argument_errors_are_codes_before_any_launch(built_lib):
    """fake pointers throughout: a launch would fault, a return code proves there was none"""
    L = built_lib
    err = L.f3r_last_error_string
    T = C.T

    def hw(*pairs):
        flat = [x for p in pairs for x in p]
        return (ctypes.c_int64 * len(flat))(*flat)

    one = hw((4, 5))          # 20 vertices: one vertex tile, one quad tile
    assert L.f3r_mesh_workspace_bytes(1, 1, 20, 0) > 0 and L.f3r_mesh_workspace_bytes(1, 1, 20, 1) > L.f3r_mesh_workspace_bytes(1, 1, 20, 0)
    assert L.f3r_mesh_workspace_bytes(0, 1, 20, 0) == 0 and L.f3r_mesh_workspace_bytes(1, 1, 2 ** 31, 0) == 0
    big = L.f3r_mesh_workspace_bytes(1, 1, 20, 1)
    # null table / outputs
    assert L.f3r_mesh_threshold(None, 1, 0x1000, 0x2000, None) == -1 and b"null" in err()
    assert L.f3r_mesh_threshold(0x1000, 0, 0x1000, 0x2000, None) == -1 and b"n_views" in err()
    assert L.f3r_mesh_count(None, one, 1, 1, 1, 20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"null" in err()
    assert L.f3r_mesh_count(0x1000, None, 1, 1, 1, 20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"null" in err()
    assert L.f3r_mesh_count(0x1000, one, 1, 1, 1, 20, None, 0, None, big, 0x2000, None) == -1 and b"null" in err()
    assert L.f3r_mesh_write(None, one, 1, 1, 1, 20, 1, 0, 0, 1, 0x1000, big, 0x2000, 0x3000, 0x4000, None) == -1 and b"null" in err()
    # negative counts
    assert L.f3r_mesh_count(0x1000, one, -1, 1, 1, 20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"n_views" in err()
    assert L.f3r_mesh_count(0x1000, one, 1, -1, 1, 20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"negative" in err()
    assert L.f3r_mesh_count(0x1000, one, 1, 1, 1, -20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"negative" in err()
    assert L.f3r_mesh_count(0x1000, hw((0, 5)), 1, 1, 1, 20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"H, W >= 1" in err()
    assert L.f3r_mesh_ply_pack(0x1000, -1, 0x2000, 0x3000, 1, 0, 0x4000, None) == -1 and b"negative" in err()
    # totals that disagree with the shapes
    assert L.f3r_mesh_count(0x1000, one, 1, 1, 1, 21, None, 0, 0x1000, big, 0x2000, None) == -1 and b"host_hw gives" in err()
    assert L.f3r_mesh_count(0x1000, one, 1, 2, 1, 20, None, 0, 0x1000, big, 0x2000, None) == -1 and b"host_hw gives" in err()
    # 2^31 vertices or more: one view, and the running sum over two
    n31 = 2 ** 31
    for shapes in (((65536, 32768),), ((32768, 32768), (32768, 32768))):
        nvt = sum((h * w + T - 1) // T for h, w in shapes)
        nqt = sum(((h - 1) * (w - 1) + T - 1) // T for h, w in shapes)
        assert L.f3r_mesh_count(0x1000, hw(*shapes), len(shapes), nvt, nqt, n31, None, 0, 0x1000, 1 << 40, 0x2000, None) == -1
        assert b"2^31" in err()
        assert L.f3r_mesh_write(0x1000, hw(*shapes), len(shapes), nvt, nqt, n31, 1, 0, 0, 1, 0x1000, 1 << 40, 0x2000, 0x3000, 0x4000, None) == -1
        assert b"2^31" in err()
    assert L.f3r_mesh_ply_pack(0x1000, n31, 0x2000, 0x3000, 1, 0, 0x4000, None) == -1 and b"2^31" in err()
    # workspace too small (drop_unreferenced needs more than the plain one)
    small = L.f3r_mesh_workspace_bytes(1, 1, 20, 0)
    assert L.f3r_mesh_count(0x1000, one, 1, 1, 1, 20, None, 0, 0x1000, small - 1, 0x2000, None) == -1 and b"workspace too small" in err()
    assert L.f3r_mesh_count(0x1000, one, 1, 1, 1, 20, None, 1, 0x1000, small, 0x2000, None) == -1 and b"workspace too small" in err()
    assert L.f3r_mesh_write(0x1000, one, 1, 1, 1, 20, 1, 1, 0, 1, 0x1000, small, 0x2000, 0x3000, 0x4000, None) == -1
    assert b"workspace too small" in err()
    # bad index dtype
    assert L.f3r_mesh_write(0x1000, one, 1, 1, 1, 20, 1, 0, 0, 2, 0x1000, big, 0x2000, 0x3000, 0x4000, None) == -1 and b"index_dtype" in err()
    assert L.f3r_mesh_ply_pack(0x1000, 3, 0x2000, 0x3000, 1, 7, 0x4000, None) == -1 and b"index_dtype" in err()
    assert L.f3r_mesh_ply_pack(0x1000, 3, 0x2000, 0x3000, 1, 0, 0x4001, None) == -1 and b"aligned" in err()
    assert L.f3r_mesh_write(0x1000, one, 1, 1, 1, 20, 1, 0, 0, 1, 0x1000, big, 0x2000, 0x3000, None, None) == -1 and b"face_colors" in err()


def test_python_argument_errors_come_before_any_launch():
    import fast3r_amd
    from fast3r_amd import _lib
    case = C.build("batch2")
    with pytest.raises(ValueError, match="index_dtype"):
        fast3r_amd.build_mesh(case["preds"], case["views"], index_dtype=torch.int16)
    with pytest.raises(ValueError, match="sample"):
        fast3r_amd.build_mesh(case["preds"], case["views"], sample=2)
    with pytest.raises(ValueError, match="head"):
        fast3r_amd.build_mesh(case["preds"], case["views"], head="both")
    with pytest.raises(ValueError, match="percentile"):
        fast3r_amd.build_mesh(case["preds"], case["views"], min_conf_thr_percentile=101)
    with pytest.raises(ValueError, match="valid"):
        fast3r_amd.build_mesh(case["preds"], case["views"], valid=[np.ones((4, 5), bool)])
    with pytest.raises(ValueError, match=r"valid\[1\]"):
        fast3r_amd.build_mesh(case["preds"], case["views"], valid=[np.ones((4, 5), bool), np.ones((3, 3), bool)])
    preds = [dict(p) for p in case["preds"]]
    del preds[1]["conf_local"]
    with pytest.raises(KeyError, match="conf_local"):
        fast3r_amd.build_mesh(preds, case["views"], head="local")
    with pytest.raises(ValueError, match="views"):
        fast3r_amd.build_mesh(case["preds"])
    # CPU tensors: no CPU path behind the reference's names
    img = torch.zeros(4, 5, 3, dtype=torch.uint8)
    with pytest.raises(_lib.F3RError):
        fast3r_amd.pts3d_to_trimesh(img, torch.zeros(4, 5, 3))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.F3RError):
            fast3r_amd.build_mesh(case["preds"], case["views"])
