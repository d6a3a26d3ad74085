"""Mesh export on a real MI355X: every golden case of the reference's `pts3d_to_trimesh` / `cat_meshes` bit for bit (thresholds,
per-view counts, vertices, faces and face colours by dtype, shape and bytes), the reference's two names against `build_mesh`, the
options without a reference counterpart against tests/mesh_ref.py, the PLY bytes, determinism, a size case against a torch-on-device
restatement, and the README flow end to end.  No tolerances: integer work, or fp32 arithmetic with numpy's roundings."""
import os

import numpy as np
import pytest
import torch

import mesh_cases as C
import mesh_ref as R
from test_mesh import matches, parse_mesh_ply

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mesh_cases.pt")
KEYS = ("vertices", "faces", "face_colors")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def on_device(case):
    preds = [{k: v.cuda() for k, v in p.items()} for p in case["preds"]]
    views = [{k: v.cuda() for k, v in vw.items()} for vw in case["views"]]
    masks = None if case["masks"] is None else [torch.from_numpy(m).cuda() for m in case["masks"]]
    return preds, views, masks


def run(case, **kw):
    import fast3r_amd
    preds, views, masks = on_device(case)
    return fast3r_amd.build_mesh(preds, views, sample=case["sample"], min_conf_thr_percentile=case["pct"], valid=masks, **kw)


def same_as_ref(mesh, ref, index_dtype=np.int64):
    for k in KEYS:
        got = getattr(mesh, k).cpu().numpy()
        want = ref[k].astype(index_dtype) if k == "faces" else ref[k]
        assert got.dtype == want.dtype and got.shape == want.shape and bits(got) == bits(want), k
    assert bits(mesh.thresholds) == bits(ref["thresholds"]) and mesh.thresholds.dtype == np.float32
    assert np.array_equal(mesh.faces_per_view, ref["faces_per_view"]) and np.array_equal(mesh.vertices_per_view, ref["vertices_per_view"])


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_golden_case_bit_for_bit(built_lib, golden, name):
    import fast3r_amd
    g = golden["cases"][name]
    case = C.build(name)
    assert C.checksum(case) == g["checksum"]
    preds, views, masks = on_device(case)
    keep = [{k: v.clone() for k, v in p.items()} for p in preds], [v["img"].clone() for v in views], [m.clone() for m in masks or []]
    mesh = fast3r_amd.build_mesh(preds, views, sample=case["sample"], min_conf_thr_percentile=case["pct"], valid=masks)
    for p, q in zip(preds, keep[0]):
        assert all(bits(p[k].cpu().numpy()) == bits(q[k].cpu().numpy()) for k in q), "inputs were written to"
    assert all(torch.equal(v["img"], q) for v, q in zip(views, keep[1])) and all(torch.equal(m, q) for m, q in zip(masks or [], keep[2]))
    for k in KEYS:
        t = getattr(mesh, k)
        assert t.is_cuda and matches(g["mesh"][k], t.cpu().numpy()), k
    assert mesh.faces.dtype == torch.int64 and mesh.vertices.dtype == torch.float32 and mesh.face_colors.dtype == torch.uint8
    assert mesh.thresholds.dtype == np.float32 and bits(mesh.thresholds) == bits(g["mesh"]["thresholds"].numpy())
    assert np.array_equal(mesh.faces_per_view, g["mesh"]["faces_per_view"].numpy())
    assert mesh.vertices_per_view.tolist() == [h * w for h, w in case["shapes"]]
    assert mesh.faces.shape[0] == int(mesh.faces_per_view.sum()) and mesh.vertices.shape[0] == int(mesh.vertices_per_view.sum())


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_pts3d_to_trimesh_and_cat_meshes_equal_build_mesh(built_lib, golden, name):
    """the reference's two names, fed the notebook's three preparation lines, against the one-pass path on the same views"""
    import fast3r_amd
    case = C.build(name)
    mesh = run(case)
    meshes = []
    for i, (img, pts, conf) in enumerate(C.numpy_views(case)):
        valid = torch.from_numpy(conf).cuda() > float(mesh.thresholds[i])   # fp32 > fp32: the threshold is exact as a double
        if case["masks"] is not None:
            valid = valid & torch.from_numpy(case["masks"][i]).cuda()
        meshes.append(fast3r_amd.pts3d_to_trimesh(torch.from_numpy(R.colors_u8(img)).cuda(), torch.from_numpy(pts).cuda(), valid))
        assert meshes[-1]["faces"].dtype == torch.int64 and meshes[-1]["vertices"].shape == (conf.size, 3)
    before = [m["faces"].clone() for m in meshes]
    cat = fast3r_amd.cat_meshes(meshes)
    assert all(torch.equal(m["faces"], b) for m, b in zip(meshes, before)), "cat_meshes wrote to its inputs"
    for k in KEYS:
        assert cat[k].dtype == getattr(mesh, k).dtype and torch.equal(cat[k], getattr(mesh, k)), k
    if name == "masks":   # valid alone (no confidences), and valid=None: every face
        g = golden["cases"][name]["mask_only"]
        only = []
        for i, (img, pts, conf) in enumerate(C.numpy_views(case)):
            m = torch.from_numpy(case["masks"][i]).cuda()
            only.append(fast3r_amd.pts3d_to_trimesh(torch.from_numpy(R.colors_u8(img)).cuda(), torch.from_numpy(pts).cuda(),
                                                    m if i % 2 else m.to(torch.uint8)))
        cat = fast3r_amd.cat_meshes(only)
        for k in KEYS:
            assert matches(g[k], cat[k].cpu().numpy()), k
        img, pts, _ = C.numpy_views(case)[0]
        every = fast3r_amd.pts3d_to_trimesh(torch.from_numpy(R.colors_u8(img)).cuda(), torch.from_numpy(pts).cuda())
        assert all(torch.equal(every[k], only[0][k]) for k in KEYS)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_options_against_the_restatement(built_lib, name):
    case = C.build(name)
    views = C.numpy_views(case)
    full = run(case)
    same_as_ref(full, R.build(views, case["pct"], case["masks"]))
    same_as_ref(run(case, index_dtype=torch.int32), R.build(views, case["pct"], case["masks"]), np.int32)
    i32 = run(case, index_dtype=torch.int32)
    assert i32.faces.dtype == torch.int32 and torch.equal(i32.faces, full.faces.to(torch.int32))
    same_as_ref(run(case, double_sided=False), R.build(views, case["pct"], case["masks"], double_sided=False))
    same_as_ref(run(case, flip_axes=True), R.build(views, case["pct"], case["masks"], flip_axes=True))
    drop = run(case, drop_unreferenced=True)
    same_as_ref(drop, R.build(views, case["pct"], case["masks"], drop_unreferenced=True))
    nv = drop.vertices.shape[0]
    if drop.faces.shape[0]:
        assert int(drop.faces.min()) == 0 and int(drop.faces.max()) == nv - 1
        assert torch.equal(torch.unique(drop.faces), torch.arange(nv, device="cuda")), "a vertex that no face uses was kept"
        assert torch.equal(drop.vertices[drop.faces], full.vertices[full.faces])   # the same triangles in space
    else:
        assert nv == 0
    both = run(case, drop_unreferenced=True, double_sided=False, flip_axes=True, index_dtype=torch.int32)
    same_as_ref(both, R.build(views, case["pct"], case["masks"], drop_unreferenced=True, double_sided=False, flip_axes=True), np.int32)


def test_checkerboard_with_drop_unreferenced_leaves_nothing(built_lib):
    import fast3r_amd
    case = C.build("masks")
    preds, views, masks = on_device(case)
    i = C.MASK_KINDS.index("checker")
    mesh = fast3r_amd.build_mesh(preds[i:i + 1], views[i:i + 1], min_conf_thr_percentile=0, valid=masks[i:i + 1], drop_unreferenced=True)
    assert mesh.vertices.shape == (0, 3) and mesh.faces.shape == (0, 3) and mesh.face_colors.shape == (0, 3)
    assert mesh.vertices_per_view.tolist() == [0] and mesh.faces_per_view.tolist() == [0]
    assert fast3r_amd.generate_mesh_ply_bytes(mesh.vertices, mesh.faces, mesh.face_colors) == fast3r_amd.mesh.mesh_ply_header(0, 0)


def test_local_head(built_lib):
    """head="local" reads pts3d_local / conf_local, and pts3d_local_aligned_to_global once it is there"""
    import fast3r_amd
    case = C.build("three_views")
    preds, views, _ = on_device(case)
    mesh = fast3r_amd.build_mesh(preds, views, head="local", min_conf_thr_percentile=case["pct"])
    same_as_ref(mesh, R.build(C.numpy_views(case, "local"), case["pct"]))
    aligned = [dict(p, pts3d_local_aligned_to_global=p["pts3d_in_other_view"] + 1.0) for p in preds]
    moved = fast3r_amd.build_mesh(aligned, views, head="local", min_conf_thr_percentile=case["pct"])
    assert torch.equal(moved.faces, mesh.faces) and torch.equal(moved.vertices, torch.cat([p["pts3d_local_aligned_to_global"][0].reshape(-1, 3)
                                                                                         for p in aligned]))


@pytest.mark.parametrize("name", ["three_views", "tile_plus_one", "no_quads"])
def test_mesh_ply_bytes_equal_the_restatement(built_lib, name, tmp_path):
    import fast3r_amd
    case = C.build(name)
    ref = R.build(C.numpy_views(case), case["pct"], case["masks"])
    want = R.ply_bytes(ref["vertices"], ref["faces"], ref["face_colors"])
    for dt in (torch.int64, torch.int32):
        mesh = run(case, index_dtype=dt)
        assert fast3r_amd.generate_mesh_ply_bytes(mesh.vertices, mesh.faces, mesh.face_colors) == want
    assert fast3r_amd.generate_mesh_ply_bytes(ref["vertices"], ref["faces"], ref["face_colors"]) == want   # numpy in, uploaded
    path = tmp_path / "mesh.ply"
    assert mesh.save_ply(str(path)) == (len(ref["vertices"]), len(ref["faces"]))
    raw = path.read_bytes()
    assert raw == want and parse_mesh_ply(raw)[3] == len(raw)
    fast3r_amd.save_mesh_ply(str(path), mesh.vertices, mesh.faces, mesh.face_colors)
    assert path.read_bytes() == want


def test_two_runs_give_the_same_bits(built_lib):
    case = C.build("wave_crossing")
    a, b = run(case, drop_unreferenced=True), run(case, drop_unreferenced=True)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in KEYS) and bits(a.thresholds) == bits(b.thresholds)
    a, b = run(case), run(case)
    assert all(torch.equal(getattr(a, k), getattr(b, k)) for k in KEYS)


def torch_restatement(img, pts, valid, base):
    """one view on the device with torch: (faces int64 (F, 3), face colours, kept A, kept B) in the reference's order"""
    H, W = valid.shape
    a = valid[:-1, :-1] & valid[:-1, 1:] & valid[1:, :-1]
    b = valid[:-1, 1:] & valid[1:, :-1] & valid[1:, 1:]
    tl = (torch.arange(H, device="cuda")[:, None] * W + torch.arange(W, device="cuda")[None, :])[:-1, :-1]
    ia, ib = tl[a], tl[b]
    fa = torch.stack([ia, ia + 1, ia + W], 1) + base
    fb = torch.stack([ib + 1, ib + W, ib + W + 1], 1) + base
    u8 = ((img + 1.0) * 127.5).to(torch.uint8).permute(1, 2, 0).reshape(-1, 3)   # values in [-1, 1]: two rounded fp32 operations
    ca, cb = u8[ia], u8[ib + W + 1]
    return torch.cat([fa, fa.flip(1), fb, fb.flip(1)]), torch.cat([ca, ca, cb, cb]), ia.numel(), ib.numel()


def test_size_case_against_torch_on_device(built_lib):
    """3 views of 512 x 512 at percentile 80; torch.quantile is not numpy's fp32 lerp, so the threshold comes from the host percentile"""
    import hashlib
    import fast3r_amd
    rs = np.random.RandomState(77)
    V, H, W = 3, 512, 512
    preds, views, want_thr = [], [], []
    for i in range(V):
        # a smooth confidence field with noise on top: the kept region has an interior as well as a ragged border
        conf = (1.0 + np.exp(np.kron(rs.randn(16, 16), np.ones((32, 32))) + 0.3 * rs.randn(H, W))).astype(np.float32)
        want_thr.append(np.percentile(conf, 80))
        preds.append({"conf": torch.from_numpy(conf)[None].cuda(), "pts3d_in_other_view": torch.from_numpy(rs.randn(1, H, W, 3).astype(np.float32)).cuda()})
        views.append({"img": torch.from_numpy((rs.rand(1, 3, H, W) * 2.0 - 1.0).astype(np.float32)).cuda()})
    mesh = fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=80)
    assert bits(mesh.thresholds) == bits(np.asarray(want_thr, np.float32))
    faces, cols, per_view = [], [], []
    for i in range(V):
        valid = preds[i]["conf"][0] > float(want_thr[i])
        f, c, na, nb = torch_restatement(views[i]["img"][0], preds[i]["pts3d_in_other_view"][0], valid, i * H * W)
        faces.append(f)
        cols.append(c)
        per_view.append(2 * (na + nb))
    assert mesh.faces_per_view.tolist() == per_view and min(per_view) > 100000
    faces, cols = torch.cat(faces), torch.cat(cols)
    assert mesh.faces.shape == faces.shape and torch.equal(mesh.faces, faces) and torch.equal(mesh.face_colors, cols)
    sha = lambda t: hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()   # noqa: E731
    assert sha(mesh.faces) == sha(faces) and sha(mesh.face_colors) == sha(cols)
    assert torch.equal(mesh.vertices, torch.cat([p["pts3d_in_other_view"][0].reshape(-1, 3) for p in preds]))
    drop = fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=80, drop_unreferenced=True, index_dtype=torch.int32)
    used, inv = torch.unique(faces, return_inverse=True)
    assert torch.equal(drop.vertices, mesh.vertices[used]) and torch.equal(drop.faces, inv.to(torch.int32))
    assert int(drop.vertices_per_view.sum()) == used.numel()


def test_readme_flow_end_to_end(built_lib, tmp_path):
    """tiny synthetic model -> inference -> build_mesh(out) -> save_ply; the file is as long as its header says"""
    import fast3r_amd
    from fast3r_amd import Fast3R, MultiViewDUSt3RLitModule, inference
    from fast3r_amd.synthetic import make_views, synth_state_dict, tiny_args
    enc, dec, head = tiny_args()
    m = Fast3R(enc, dec, head).eval()
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0), strict=True)
    lit = MultiViewDUSt3RLitModule.load_for_inference(m.cuda())
    torch.manual_seed(3)
    out = inference(make_views(3, 64, 64), lit, torch.device("cuda"), dtype=torch.float16, verbose=False)
    mesh = fast3r_amd.build_mesh(out)
    assert mesh.vertices.shape == (3 * 64 * 64, 3) and mesh.vertices.is_cuda and len(mesh.thresholds) == 3
    for i, p in enumerate(out["preds"]):
        assert np.float32(np.percentile(p["conf"][0].float().cpu().numpy(), 80)).tobytes() == mesh.thresholds[i].tobytes()
    path = tmp_path / "mesh.ply"
    nv, nf = mesh.save_ply(str(path))
    assert (nv, nf) == (3 * 64 * 64, int(mesh.faces_per_view.sum()))
    raw = path.read_bytes()
    v, f, c, implied = parse_mesh_ply(raw)
    assert implied == len(raw) and len(v) == nv and len(f) == nf
    assert np.array_equal(v, mesh.vertices.cpu().numpy()) and np.array_equal(f, mesh.faces.cpu().numpy()) and np.array_equal(c, mesh.face_colors.cpu().numpy())
    assert torch.equal(torch.from_numpy(v[:64 * 64].copy()), out["preds"][0]["pts3d_in_other_view"][0].reshape(-1, 3).float().cpu())
