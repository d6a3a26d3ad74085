"""Ground-truth views on the GPU (fast3r_amd/gt_views.py, fast3r_amd/csrc/f3r_views.hip) against what the reference's dataset path
returned (tests/golden/gt_views_cases.pt) and, where the reference never ran, against its numpy / Pillow restatement
(tests/gt_views_ref.py, pinned on the golden by tests/test_gt_views.py).

Bit for bit: img, img_u8, depthmap, valid_mask, camera_intrinsics, true_shape (integer work, or fp32 operations in the reference's order)
and the camera-frame points (the fp64 expression rounded once).  pts3d: |delta_i| <= 8 * 2^-24 * (sum_k |R_ik X_k| + |t_i|) per component
wherever the golden is finite, and non-finite exactly where the golden is -- a derived bound: numpy's einsum fixes no summation order,
any fp32 evaluation of three products and three sums lies within 3 * 2^-24 * S of the exact value, two of them within 6, and 8 leaves
room for the final rounding."""
import os

import numpy as np
import pytest
import torch

import gt_views_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gt_views_cases.pt")
CASES = ("1_plain_lanczos", "2_half_even_square_target", "3_odd_sizes", "4_portrait", "5_upscale_bicubic", "6_square_landscape",
         "6_square_portrait", "7_depth_edge_values", "8_three_views_one_geometry", "8_four_views_two_geometries", "9_no_pose")
TENSOR_KEYS = ("img", "depthmap", "pts3d", "valid_mask", "camera_pose", "camera_intrinsics", "true_shape", "img_u8")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def case_inputs(golden, name):
    c = golden["cases"][name]
    frames = [golden["frames"][k] for k in c["frames"]]
    poses = [golden["poses"][k].numpy() for k in c["frames"]] if c["with_pose"] else None
    return ([f["image"].numpy() for f in frames], [f["depthmap"].numpy() for f in frames], [f["intrinsics"].numpy() for f in frames], poses,
            c["resolution"], c["square_portrait"], c["views"])


@pytest.fixture(scope="module")
def built(golden, built_lib):
    """every golden case through build_gt_views once, with the restatement beside it; shared, never changed"""
    import fast3r_amd
    out = {}
    for name in CASES:
        images, depths, Ks, poses, resolution, choices, want = case_inputs(golden, name)
        views = fast3r_amd.build_gt_views(images, depths, Ks, poses, resolution=resolution, square_portrait=choices, dataset="golden",
                                          labels=[f"scene/{i}" for i in range(len(images))])
        out[name] = (views, R.build(images, depths, Ks, poses, resolution, choices), want)
    torch.cuda.synchronize()
    return out


def same_bytes(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = want.cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


def check_view(view, ref, want=None):
    """a built view against the restatement's view `ref` and, where given, the golden's `want` (B = 1 against uncollated arrays)"""
    assert view["img"].is_cuda and view["img"].dtype == torch.float32 and view["valid_mask"].dtype == torch.bool
    assert view["true_shape"].dtype == torch.int32 and tuple(view["true_shape"].shape) == (1, 2)
    for key in R.KEYS_EXACT:
        assert same_bytes(view[key][0], ref[key]), key
        if want is not None:
            assert same_bytes(view[key][0], want[key]), key
    assert same_bytes(view["img_u8"], ref["img_u8"])
    assert tuple(view["img"].shape[2:]) == tuple(view["img_u8"].shape[:2]) == tuple(view["depthmap"].shape[1:])
    assert np.array_equal(view["camera_pose"][0].cpu().numpy(), ref["camera_pose"], equal_nan=True)
    target = dict(ref, pts3d=want["pts3d"].numpy()) if want is not None else ref
    ok, ratio = R.pts3d_close(view["pts3d"][0].cpu().numpy(), target)
    print(f"pts3d: {ratio:.3f} of the derived bound")
    assert ok, ratio


@pytest.mark.parametrize("name", CASES)
def test_build_gt_views_reproduces_the_golden(built, name):
    views, refs, wants = built[name]
    assert len(views) == len(wants)
    for i, (view, ref, want) in enumerate(zip(views, refs, wants)):
        check_view(view, ref, want)
        assert view["dataset"] == ["golden"] and view["label"] == [f"scene/{i}"] and view["instance"] == [str(i)]
        assert [int(t) for t in view["idx"]] == [0, 0, i]
    if name == "4_portrait":
        v = views[0]
        assert v["true_shape"].tolist() == [[32, 24]] and tuple(v["img"].shape) == (1, 3, 24, 32) and tuple(v["pts3d"].shape) == (1, 24, 32, 3)
        K = v["camera_intrinsics"][0].cpu()
        assert K[0, 0] == 0 and K[1, 1] == 0 and K[0, 1] > 0 and K[1, 0] > 0      # rows [1, 0, 2]
    if name == "7_depth_edge_values":
        v = views[0]
        assert not torch.isfinite(v["pts3d"][0, 12, 30]).all() and not v["valid_mask"][0, 12, 30] and v["depthmap"][0, 12, 30] == 3.0e38
    if name == "9_no_pose":
        v = views[0]
        assert torch.isnan(v["pts3d"]).all() and torch.isnan(v["camera_pose"]).all() and not v["valid_mask"].any()


def test_a_group_shares_one_allocation_and_results_keep_the_input_order(built):
    views, _, _ = built["8_four_views_two_geometries"]       # landscape, portrait, landscape, portrait
    for key in ("img", "depthmap", "pts3d", "valid_mask"):
        a, b = views[0][key], views[2][key]
        assert b.data_ptr() - a.data_ptr() == a.numel() * a.element_size(), key      # consecutive slices of the group's tensor
        assert views[1][key].untyped_storage().data_ptr() != a.untyped_storage().data_ptr()
        assert views[3][key].data_ptr() - views[1][key].data_ptr() == views[1][key].numel() * views[1][key].element_size()
    assert [v["true_shape"].tolist() for v in views] == [[[24, 32]], [[32, 24]], [[24, 32]], [[32, 24]]]
    three, _, _ = built["8_three_views_one_geometry"]
    assert three[2]["img"].data_ptr() - three[0]["img"].data_ptr() == 2 * three[0]["img"].numel() * 4


@pytest.mark.parametrize("name", CASES)
def test_the_three_named_functions(golden, built, name):
    import fast3r_amd
    images, depths, Ks, poses, resolution, choices, wants = case_inputs(golden, name)
    dev = torch.device("cuda")
    for i, want in enumerate(wants):
        image, depth = torch.from_numpy(images[i]).to(dev), torch.from_numpy(depths[i]).to(dev)
        pic, ref_depth, ref_K, _ = R.crop_resize(images[i], depths[i], Ks[i], (resolution, resolution) if isinstance(resolution, int) else resolution,
                                                 choices[i])
        img_u8, d2, K2 = fast3r_amd.crop_resize_if_necessary(image, depth, Ks[i], resolution, square_portrait=choices[i])
        assert same_bytes(img_u8, np.asarray(pic)) and same_bytes(d2, ref_depth) and same_bytes(K2, ref_K)
        turned = want["true_shape"][1] < want["true_shape"][0]
        assert same_bytes(d2, want["depthmap"].numpy().swapaxes(0, 1) if turned else want["depthmap"])       # not transposed, as the reference returns it
        assert same_bytes(K2, want["camera_intrinsics"].numpy()[[1, 0, 2]] if turned else want["camera_intrinsics"])
        X, positive = fast3r_amd.depthmap_to_camera_coordinates(d2, K2)
        ref_X, ref_positive = R.camera_points(ref_depth, ref_K)
        assert same_bytes(X, ref_X) and same_bytes(positive, ref_positive)
        if poses is None:
            continue
        world, positive = fast3r_amd.depthmap_to_absolute_camera_coordinates(d2, K2.cpu().numpy(), torch.from_numpy(poses[i]).to(dev))
        assert same_bytes(positive, ref_positive)
        gold = want["pts3d"].numpy().swapaxes(0, 1) if turned else want["pts3d"].numpy()
        ok, ratio = R.pts3d_close(world.cpu().numpy(), {"pts3d": gold, "X_cam": ref_X, "camera_pose": poses[i]})
        assert ok, ratio
        world34, _ = fast3r_amd.depthmap_to_absolute_camera_coordinates(d2, K2, poses[i][:3])
        assert same_bytes(world34, world)


@pytest.fixture(scope="module")
def large():
    """four views of 641 x 479 to (512, 384): every tile of the kernels and more than one workgroup; the second and fourth share a plan"""
    rs = np.random.RandomState(5)
    H, W, n = 479, 641, 4
    images = [rs.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(n)]
    yy, xx = np.mgrid[0:H, 0:W]
    depths = [(2.0 + np.sin(xx / 50.0 + i) * np.cos(yy / 40.0) + 0.01 * rs.standard_normal((H, W))).astype(np.float32) for i in range(n)]
    depths[1][100:120, 200:260] = 0.0
    Ks = [np.array([[520.0 + i, 0, cx], [0, 521.0, cy], [0, 0, 1]], dtype=np.float32) for i, (cx, cy) in
          enumerate(((318.7, 241.2), (320.5, 239.5), (300.2, 236.9), (320.5, 239.5)))]
    poses = []
    for i in range(n):
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = q, rs.uniform(-3, 3, 3)
        poses.append(T.astype(np.float32))
    return images, depths, Ks, poses, R.build(images, depths, Ks, poses, (512, 384))


def test_a_large_frame_against_the_restatement(large, built_lib):
    import fast3r_amd
    images, depths, Ks, poses, refs = large
    views = fast3r_amd.build_gt_views(images, depths, Ks, poses, resolution=(512, 384))
    assert views[3]["img"].untyped_storage().data_ptr() == views[1]["img"].untyped_storage().data_ptr()
    for view, ref in zip(views, refs):
        assert tuple(view["img"].shape) == (1, 3, 384, 512)
        check_view(view, ref)


@pytest.mark.parametrize("W", (16384, 16386))
def test_the_widest_staged_row_and_the_first_wider_one(W, built_lib):
    """the horizontal pass stages a window's row in LDS up to 16384 pixels and reads its taps from memory beyond: both sides of that
    threshold, on a strip that is upscaled (BICUBIC) and cropped to 64 columns in its middle"""
    import fast3r_amd
    rs = np.random.RandomState(W)
    image = rs.randint(0, 256, (24, W, 3)).astype(np.uint8)
    depth = (1.0 + rs.rand(24, W)).astype(np.float32)
    K = np.array([[900.0, 0, W / 2], [0, 900.0, 12.0], [0, 0, 1]], dtype=np.float32)
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = [0.5, -1.0, 2.0]
    (ref,) = R.build([image], [depth], [K], [pose], (64, 48))
    assert ref["trace"]["box1"] == (0, 0, W, 24) and ref["trace"]["resized"] == (2 * W, 48) and ref["trace"]["box2"][0] == W - 32
    (view,) = fast3r_amd.build_gt_views([image], [depth], [K], [pose], resolution=(64, 48))
    check_view(view, ref)


def test_host_device_and_non_contiguous_inputs_agree_and_a_second_call_repeats(large, built_lib):
    import fast3r_amd
    images, depths, Ks, poses, _ = large
    images, depths, Ks, poses = images[:2], depths[:2], Ks[:2], poses[:2]
    dev = torch.device("cuda")
    base = fast3r_amd.build_gt_views(images, depths, Ks, poses, resolution=(512, 384))
    again = fast3r_amd.build_gt_views(images, depths, Ks, poses, resolution=(512, 384))
    on_device = fast3r_amd.build_gt_views([torch.from_numpy(a).to(dev) for a in images], [torch.from_numpy(a).to(dev) for a in depths],
                                          [torch.from_numpy(a).to(dev) for a in Ks], [torch.from_numpy(a).to(dev) for a in poses], resolution=(512, 384))
    # rows with a pitch (a window of a wider frame, read in place), pixels with a stride (a copy is made), a depth stored column-major
    odd_images, odd_depths = [], []
    for a, d in zip(images, depths):
        wide = torch.zeros((a.shape[0], a.shape[1] + 5, 3), dtype=torch.uint8, device=dev)
        wide[:, 2:-3] = torch.from_numpy(a).to(dev)
        odd_images.append(wide[:, 2:-3])
        odd_depths.append(torch.from_numpy(np.ascontiguousarray(d.T)).to(dev).t())
    spaced = torch.zeros(images[1].shape[:2] + (6,), dtype=torch.uint8, device=dev)
    spaced[:, :, ::2] = torch.from_numpy(images[1]).to(dev)
    odd_images[1] = spaced[:, :, ::2]
    assert not odd_images[0].is_contiguous() and not odd_images[1].is_contiguous() and not odd_depths[0].is_contiguous()
    odd = fast3r_amd.build_gt_views(odd_images, odd_depths, Ks, poses, resolution=(512, 384))
    for other in (again, on_device, odd):
        for a, b in zip(base, other):
            for key in TENSOR_KEYS:
                assert same_bytes(a[key], b[key]), key


def test_a_depth_that_is_not_finite_raises_unless_unchecked(golden, built_lib):
    import fast3r_amd
    images, depths, Ks, poses, resolution, choices, _ = case_inputs(golden, "1_plain_lanczos")
    bad = depths[0].copy()
    bad[30, 40] = np.nan
    with pytest.raises(ValueError, match="depthmap"):
        fast3r_amd.build_gt_views(images, [bad], Ks, poses, resolution=resolution)
    views = fast3r_amd.build_gt_views(images, [bad], Ks, poses, resolution=resolution, check_finite=False)
    assert torch.isnan(views[0]["depthmap"]).sum() >= 1 and not views[0]["valid_mask"][torch.isnan(views[0]["depthmap"])].any()


def test_end_to_end_with_the_reconstruction_metrics(built):
    """preds = the returned pts3d moved by a known similarity: the registration inside reconstruction_metrics undoes it"""
    from fast3r_amd import recon_metric
    views, _, _ = built["8_three_views_one_geometry"]
    rs = np.random.RandomState(3)
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    Rm = torch.from_numpy(q.astype(np.float32)).to(views[0]["pts3d"].device)
    t = torch.tensor([0.3, -1.2, 2.0], device=Rm.device)
    preds = [{"pts3d_in_other_view": 1.7 * (v["pts3d"] @ Rm.T) + t, "conf": torch.ones_like(v["depthmap"])} for v in views]
    assert all(bool(v["valid_mask"].all()) for v in views)
    gt = torch.cat([v["pts3d"].reshape(-1, 3) for v in views])
    extent = float((gt.max(0).values - gt.min(0).values).norm())
    (result,) = recon_metric.reconstruction_metrics(views, preds, use_pts3d_from_local_head=False)
    (metrics,) = result.values()
    assert list(result) == ["scene"]
    print(f"accuracy {metrics['accuracy']:.3e}, completion {metrics['completion']:.3e}, extent {extent:.3f}")
    assert 0 <= metrics["accuracy"] < 1e-4 * extent and 0 <= metrics["completion"] < 1e-4 * extent
