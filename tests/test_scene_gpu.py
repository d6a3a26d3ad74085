"""Scene assembly and PLY export on a real MI355X: every golden case of the reference's `start_visualization` bit for bit (orders,
sorted arrays, the three colourings, max_conf_global, scene_extent, counts and PLY bytes by length and SHA-256), a size case against
torch.sort / torch.gather on the device, determinism, and the README flow end to end.  No tolerances: integer work, or fp32
arithmetic with numpy's roundings."""
import os

import numpy as np
import pytest
import torch

import scene_cases as C
import scene_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_cases.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def on_device(scene):
    preds = [{k: v.cuda() for k, v in p.items()} for p in scene["preds"]]
    views = [{k: v.cuda() for k, v in vw.items()} for vw in scene["views"]]
    return preds, views


@pytest.mark.parametrize("name", sorted(C.SCENES))
def test_golden_scene_bit_for_bit(built_lib, golden, name):
    import fast3r_amd
    from fast3r_amd import scene as S
    from test_scene import restated_frames
    g = golden["scenes"][name]
    scene, frames = restated_frames(name, S.turbo_lut_u8())
    assert C.checksum(scene) == g["checksum"]
    V = len(frames)
    preds, views = on_device(scene)
    keep = [{k: v.clone() for k, v in p.items()} for p in preds]
    sc = fast3r_amd.assemble_scene(preds, views, sample=scene["sample"], not_sky=scene["masks"], poses=False)
    for p, q in zip(preds, keep):
        assert all(bits(p[k].cpu().numpy()) == bits(q[k].cpu().numpy()) for k in q), "inputs were written to"
    for i, (fd, ref) in enumerate(zip(sc.frames, frames)):
        for h in ("global", "local"):
            order = fd[f"order_{h}"].cpu().numpy()
            assert order.dtype == np.int32 and np.array_equal(order, g["orders"][i][h].numpy().astype(np.int32)), (i, h)
            for key in (f"sorted_pts3d_{h}", f"sorted_conf_{h}", f"sorted_not_sky_{h}", f"colors_rgb_{h}", f"colors_confidence_{h}",
                        f"colors_rainbow_{h}"):
                got = fd[key].cpu().numpy()
                assert got.dtype == ref[key].dtype and got.shape == ref[key].shape and bits(got) == bits(ref[key]), (i, key)
        assert np.float64(fd["max_conf_global"]).tobytes() == np.float64(g["max_conf_global"][i]).tobytes(), i
        assert fd["is_high_confidence"] == g["is_high_confidence"][i]
        assert (fd["height"], fd["width"]) == tuple(g["shapes"][i]) and fd["rainbow_color"] == ref["rainbow_color"]
    assert sc.scene_extent.dtype == np.float32 and bits(sc.scene_extent) == bits(g["scene_extent"].numpy())
    assert sc.is_outdoor == g["is_outdoor"]
    ext = g["scene_extent"].numpy()
    assert sc.frustum_scale(2.0) == float(np.max(ext)) * (2.0 / 100.0)
    for key, rec in g["states"].items():
        st = rec["state"]
        sc.set_global_conf_threshold(st["threshold"])
        p, c = sc.collect_points(min_conf_thr_percentile=st["percentile"], mask_sky=st["mask_sky"], color=st["color"],
                                 show_global=st["show_global"], show_local=st["show_local"], show_high_conf=st["show_high_conf"],
                                 show_low_conf=st["show_low_conf"], upto_timestep=V - 1 - st["back"])
        visible = 0
        for i in range(V):
            if S.view_contributes(i, g["max_conf_global"][i] >= st["threshold"], V - 1 - st["back"], st["show_high_conf"], st["show_low_conf"]):
                visible += rec["counts"][2 * i] * st["show_global"] + rec["counts"][2 * i + 1] * st["show_local"]
        if rec["ply"] is None:
            assert p is None and c is None and visible == 0, key
            continue
        assert p.is_cuda and p.dtype == torch.float32 and c.dtype == torch.uint8 and p.shape == c.shape == (visible, 3), key
        assert R.digest(fast3r_amd.generate_ply_bytes(p, c)) == rec["ply"], key


@pytest.mark.parametrize("name", sorted(C.PLY_CASES))
def test_generate_ply_bytes_matches_the_reference(built_lib, golden, name, tmp_path):
    import fast3r_amd
    pts, col = C.ply_case(name)
    assert R.digest(fast3r_amd.generate_ply_bytes(pts, col)) == golden["ply"][name]                                    # numpy in
    assert R.digest(fast3r_amd.generate_ply_bytes(torch.from_numpy(pts).cuda(), torch.from_numpy(col).cuda())) == golden["ply"][name]
    path = tmp_path / "cloud.ply"
    fast3r_amd.save_ply(str(path), pts, col)
    assert R.digest(path.read_bytes()) == golden["ply"][name]


def test_generate_ply_bytes_argument_errors(built_lib):
    import fast3r_amd
    pts = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="divides by zero"):
        fast3r_amd.generate_ply_bytes(pts, np.full((4, 3), 2.0, np.float32))
    with pytest.raises(ValueError, match="NaN"):
        fast3r_amd.generate_ply_bytes(pts, np.full((4, 3), np.nan, np.float64))
    with pytest.raises(ValueError):
        fast3r_amd.generate_ply_bytes(pts, np.zeros((3, 3), np.uint8))
    empty = fast3r_amd.generate_ply_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))
    assert empty == R.ply_bytes(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint8))


def size_case():
    """8 views of 224 x 288, generated on the device, no NaN; confidences quantised so that ties cross tiles"""
    g = torch.Generator(device="cuda").manual_seed(77)
    H, W, V = 224, 288, 8
    preds, views, masks = [], [], []
    for i in range(V):
        r = lambda *s: torch.rand(*s, generator=g, device="cuda")  # noqa: E731
        conf = 1.0 + torch.floor(r(1, H, W) * 4096.0) / 256.0
        conf_l = 1.0 + 20.0 * r(1, H, W) ** 2
        preds.append({"pts3d_in_other_view": r(1, H, W, 3) * 4 - 2, "pts3d_local_aligned_to_global": r(1, H, W, 3) * 4 - 2, "conf": conf,
                      "conf_local": conf_l})
        views.append({"img": r(1, 3, H, W) * 2 - 1})
        masks.append((r(H, W) < 0.8).to(torch.int8))
    return preds, views, masks


def test_size_case_against_torch_sort_and_gather(built_lib):
    import fast3r_amd
    preds, views, masks = size_case()
    sc = fast3r_amd.assemble_scene(preds, views, not_sky=masks, poses=False)
    lut = fast3r_amd.scene.turbo_lut_u8()
    for i, fd in enumerate(sc.frames):
        img = views[i]["img"][0].reshape(3, -1)
        for h, pk, ck in (("global", "pts3d_in_other_view", "conf"), ("local", "pts3d_local_aligned_to_global", "conf_local")):
            conf, pts = preds[i][ck].reshape(-1), preds[i][pk].reshape(-1, 3)
            sconf, order = torch.sort(conf, stable=True, descending=True)
            assert torch.equal(fd[f"order_{h}"].long(), order), (i, h)
            assert torch.equal(fd[f"sorted_conf_{h}"], sconf)
            assert torch.equal(fd[f"sorted_pts3d_{h}"], torch.gather(pts, 0, order[:, None].expand(-1, 3)))
            assert torch.equal(fd[f"sorted_not_sky_{h}"], torch.gather(masks[i].reshape(-1), 0, order))
            rgb = ((torch.gather(img, 1, order[None].expand(3, -1)) + 1) * 127.5).to(torch.uint8).t()
            assert torch.equal(fd[f"colors_rgb_{h}"], rgb)
            sc_np = sconf.cpu().numpy()   # the normalisation in numpy: its fp32 division is the correctly rounded one
            idx = R.turbo_index((sc_np - sc_np.min()) / (sc_np.max() - sc_np.min() + 1e-8))
            assert idx.min() >= 0 and np.array_equal(fd[f"colors_confidence_{h}"].cpu().numpy(), lut[idx])
        assert fd["max_conf_global"] == float(preds[i]["conf"].max())
    allp = torch.cat([p["pts3d_in_other_view"].reshape(-1, 3) for p in preds]).cpu().numpy()
    want = np.percentile(allp, 80, axis=0) - np.percentile(allp, 20, axis=0)
    assert bits(sc.scene_extent) == bits(want)
    p, c = sc.collect_points(min_conf_thr_percentile=25, mask_sky=True, color="rgb", show_global=True, show_local=True)
    want_p, want_c = [], []
    for fd in sc.frames:
        for h in ("global", "local"):
            n = fast3r_amd.scene.num_to_show(fd[f"sorted_pts3d_{h}"].shape[0], 25)
            k = fd[f"sorted_not_sky_{h}"][:n] > 0
            want_p.append(fd[f"sorted_pts3d_{h}"][:n][k])
            want_c.append(fd[f"colors_rgb_{h}"][:n][k])
    assert torch.equal(p, torch.cat(want_p)) and torch.equal(c, torch.cat(want_c))


def boundary_segments(lengths, seed):
    """one (conf, pts, img, mask) per length, generated on the device; confidences quantised to 1/16 so that ties cross tiles, a mask on
    every other segment"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, device="cuda")  # noqa: E731
    conf = [1.0 + torch.floor(r(L) * 64.0) / 16.0 for L in lengths]
    pts = [r(L, 3) * 4 - 2 for L in lengths]
    img = [r(3, L) * 2 - 1 for L in lengths]
    mask = [(r(L) < 0.8).to(torch.int8) if s % 2 == 0 else None for s, L in enumerate(lengths)]
    return conf, pts, img, mask


def test_scene_sort_at_wave_and_tile_boundaries(built_lib):
    """segments of one key, of a wave's 64 keys and a tile's 4096 keys, and one short and one over each, in one call"""
    import fast3r_amd
    from fast3r_amd import post_ops
    lengths = [1, 63, 64, 65, 4095, 4096, 4097]
    conf, pts, img, mask = boundary_segments(lengths, 91)
    out = post_ops.scene_sort(conf, pts, img, mask, torch.from_numpy(fast3r_amd.scene.turbo_lut_u8()).cuda())
    assert out["offsets"] == [sum(lengths[:s]) for s in range(len(lengths))] and out["order"].shape[0] == sum(lengths)
    for s, L in enumerate(lengths):
        sl = slice(out["offsets"][s], out["offsets"][s] + L)
        sconf, order = torch.sort(conf[s], stable=True, descending=True)
        assert torch.equal(out["order"][sl].long(), order), L
        assert torch.equal(out["conf"][sl], sconf), L
        assert torch.equal(out["pts"][sl], torch.gather(pts[s], 0, order[:, None].expand(-1, 3))), L
        m = mask[s] if mask[s] is not None else torch.ones(L, dtype=torch.int8, device="cuda")  # no mask: every pixel counts as kept
        assert torch.equal(out["mask"][sl], torch.gather(m, 0, order)), L


def test_scene_collect_at_wave_and_tile_boundaries(built_lib):
    """prefixes of one entry, of a wave's 64 and a collect tile's 1024 entries, and one short and one over each, over sorted segments"""
    import fast3r_amd
    from fast3r_amd import post_ops
    nums = [1, 63, 64, 65, 1023, 1024, 1025]
    conf, pts, img, mask = boundary_segments([1100] * len(nums), 92)
    out = post_ops.scene_sort(conf, pts, img, mask, torch.from_numpy(fast3r_amd.scene.turbo_lut_u8()).cuda())
    seg = [slice(o, o + 1100) for o in out["offsets"]]
    spts = [out["pts"][sl].contiguous() for sl in seg]
    srgb = [out["rgb"][sl].contiguous() for sl in seg]
    smask = [out["mask"][sl].contiguous() if mask[s] is not None else None for s, sl in enumerate(seg)]
    p, c = post_ops.scene_collect(spts, srgb, smask, nums, [None] * len(nums))
    want_p, want_c = [], []
    for s, n in enumerate(nums):
        k = smask[s][:n] > 0 if smask[s] is not None else torch.ones(n, dtype=torch.bool, device="cuda")
        want_p.append(spts[s][:n][k])
        want_c.append(srgb[s][:n][k])
    assert torch.equal(p, torch.cat(want_p)) and torch.equal(c, torch.cat(want_c))


def test_two_runs_give_the_same_bits(built_lib):
    import fast3r_amd
    scene = C.build("lengths")
    preds, views = on_device(scene)
    keep = [{k: v.clone() for k, v in p.items()} for p in preds]
    runs = []
    for _ in range(2):
        sc = fast3r_amd.assemble_scene(preds, views, not_sky=scene["masks"], poses=False)
        p, c = sc.collect_points(min_conf_thr_percentile=10, mask_sky=True, color="confidence", show_global=True)
        runs.append([bits(fd[k].cpu().numpy()) for fd in sc.frames for k in sorted(fd) if torch.is_tensor(fd[k])]
                    + [bits(sc.scene_extent), fast3r_amd.generate_ply_bytes(p, c)])
    assert runs[0] == runs[1]
    for p, q in zip(preds, keep):
        assert all(bits(p[k].cpu().numpy()) == bits(q[k].cpu().numpy()) for k in q)


def test_readme_flow_end_to_end(built_lib, tmp_path):
    """tiny synthetic model -> inference -> align_local_pts3d_to_global -> assemble_scene -> save_ply; the file parses back"""
    import fast3r_amd
    from fast3r_amd import Fast3R, MultiViewDUSt3RLitModule, inference
    from fast3r_amd.synthetic import make_views, synth_state_dict, tiny_args
    enc, dec, head = tiny_args()
    m = Fast3R(enc, dec, head).eval()
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0), strict=True)
    lit = MultiViewDUSt3RLitModule.load_for_inference(m.cuda())
    torch.manual_seed(3)
    out = inference(make_views(3, 64, 64), lit, torch.device("cuda"), dtype=torch.float16, verbose=False)
    with pytest.raises(KeyError, match="align_local_pts3d_to_global"):
        fast3r_amd.assemble_scene(out)
    lit.align_local_pts3d_to_global(out["preds"], out["views"], min_conf_thr_percentile=85)
    sc = fast3r_amd.assemble_scene(out, global_conf_thr_value_to_drop_view=0.0)
    assert len(sc.frames) == 3 and all(fd["c2w"].shape == (4, 4) and fd["is_high_confidence"] for fd in sc.frames)
    assert sc.is_outdoor is False and np.isfinite(sc.scene_extent).all() and sc.max_extent > 0
    path = tmp_path / "scene.ply"
    n = sc.save_ply(str(path), min_conf_thr_percentile=10, show_global=True)
    want = 3 * 2 * fast3r_amd.scene.num_to_show(64 * 64, 10)
    raw = path.read_bytes()
    head_end = raw.index(b"end_header\n") + len(b"end_header\n")
    assert f"element vertex {want}".encode() in raw[:head_end] and n == want
    rec = np.frombuffer(raw[head_end:], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    assert len(rec) == want
    first = sc.frames[0]
    k = fast3r_amd.scene.num_to_show(64 * 64, 10)
    assert np.array_equal(rec["xyz"][:k], first["sorted_pts3d_global"][:k].cpu().numpy())
    assert np.array_equal(rec["rgb"][:k], first["colors_rgb_global"][:k].cpu().numpy())
    order = first["order_global"][:k].long().cpu()
    assert torch.equal(torch.from_numpy(rec["xyz"][:k].copy()), out["preds"][0]["pts3d_in_other_view"][0].reshape(-1, 3)[order])

