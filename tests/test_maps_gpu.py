"""The map pictures on a real MI355X against matplotlib's own bytes (tests/golden/map_cases.npz, written by tools/make_golden_maps.py from
matplotlib.pylab.imsave): exact equality, no tolerance -- tests/test_maps.py shows on the CPU that the arithmetic is fully specified.  The
cases (tests/map_cases.py) are sized to break the kernel: ragged for any vector width, more than one workgroup per map, extremes in the
first and last element, every truncation boundary, division rounding, overflowing and subnormal ranges, NaN and infinities, a channel read
in place, windows of a larger picture."""
import os

import numpy as np
import pytest
import torch

import map_cases as C
import maps_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(C.GOLDEN)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def numpy_ranges(maps):
    with np.errstate(invalid="ignore"):
        return np.array([[m.min(), m.max()] for m in maps], np.float32)


# ------------------------------------------------------------------------------------------------------------------- colorize_maps
@pytest.mark.parametrize("name", list(C.scalar_cases()))
def test_colorize_maps_equals_matplotlib(built_lib, golden, name):
    """every map of the case in one call, both tables: the bytes, the ranges bit for bit (NaN included), twice the same, inputs unwritten"""
    import fast3r_amd
    maps = [golden[f"s/{name}/{i}/in"] for i in range(len(C.scalar_cases()[name]))]
    on_dev = [dev(m) for m in maps]
    for cmap in C.CMAPS:
        pictures, ranges = fast3r_amd.colorize_maps(on_dev, cmap, return_ranges=True)
        assert len(pictures) == len(maps) and ranges.is_cuda and ranges.dtype == torch.float32 and tuple(ranges.shape) == (len(maps), 2)
        for i, (p, m) in enumerate(zip(pictures, maps)):
            assert p.is_cuda and p.dtype == torch.uint8 and tuple(p.shape) == m.shape + (4,)
            want = golden[f"s/{name}/{i}/{cmap}"]
            got = p.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (name, i, cmap, int((got != want).any(-1).sum()))
        got_r, want_r = ranges.cpu().numpy(), numpy_ranges(maps)
        print(f"{name} {cmap}: ranges {got_r.tolist()} (numpy {want_r.tolist()})")
        assert bits(got_r).tobytes() == bits(want_r).tobytes()
        again, ranges2 = fast3r_amd.colorize_maps(on_dev, cmap, return_ranges=True)
        assert all(torch.equal(a, b) for a, b in zip(again, pictures)) and bits(ranges2.cpu().numpy()).tobytes() == bits(got_r).tobytes()
    assert all(d.cpu().numpy().tobytes() == m.tobytes() for d, m in zip(on_dev, maps))
    assert fast3r_amd.colorize_maps(on_dev, "Turbo")[0].cpu().numpy().tobytes() == golden[f"s/{name}/0/turbo"].tobytes()   # the notebook's other spelling


def test_all_cases_in_one_call(built_lib, golden):
    """maps of every size in one table: each map keeps its own range and its own tiles"""
    import fast3r_amd
    todo = [(label, a, want) for label, a, cmap, want in C.scalar_pictures(golden) if cmap == "turbo" and not label.startswith("z/")]
    pictures, ranges = fast3r_amd.colorize_maps([dev(a) for _, a, _ in todo], return_ranges=True)
    for (label, a, want), p in zip(todo, pictures):
        assert p.cpu().numpy().tobytes() == want.tobytes(), label
    assert bits(ranges.cpu().numpy()).tobytes() == bits(numpy_ranges([a for _, a, _ in todo])).tobytes()


def test_channel_read_in_place(built_lib, golden):
    """the z channel of an (H, W, 3) pointmap: element stride 3 from element 2, no copy; also as a strided view, and a map whose base is
    not 16-byte aligned (a batch row of an odd-sized stack)"""
    import fast3r_amd
    p = golden["z/in"]
    dp = dev(p)
    for cmap in C.CMAPS:
        (pic,), ranges = fast3r_amd.colorize_maps([dp], cmap, channel=2, return_ranges=True)
        assert pic.cpu().numpy().tobytes() == golden[f"z/{cmap}"].tobytes()
        assert bits(ranges.cpu().numpy()).tobytes() == bits(numpy_ranges([p[..., 2]])).tobytes()
        (view,) = fast3r_amd.colorize_maps([dp[..., 2]], cmap)
        assert torch.equal(view, pic)
    for ch in (0, 1, -1):
        (pic,) = fast3r_amd.colorize_maps([dp], "turbo", channel=ch)
        assert pic.cpu().numpy().tobytes() == R.colorize(p[..., ch], R.table("turbo")).tobytes()
    assert dp.cpu().numpy().tobytes() == p.tobytes()
    with pytest.raises(ValueError, match="channel"):
        fast3r_amd.colorize_maps([dp], channel=3)
    a = golden["s/ragged_37x53/0/in"]
    stack = dev(np.stack([a[::-1], a, a.T.reshape(37, 53)]))                              # 1961 floats per row: rows 1 and 2 start off 16 bytes
    assert stack[1].data_ptr() % 16 != 0
    pics = fast3r_amd.colorize_maps([stack[1], stack[0], stack[2][:, ::2]])               # and a view that needs a dense copy
    assert pics[0].cpu().numpy().tobytes() == golden["s/ragged_37x53/0/turbo"].tobytes()
    assert pics[1].cpu().numpy().tobytes() == R.colorize(a[::-1], R.table("turbo")).tobytes()
    assert pics[2].cpu().numpy().tobytes() == R.colorize(a.T.reshape(37, 53)[:, ::2], R.table("turbo")).tobytes()


def test_windows_of_a_larger_picture_do_not_bleed(built_lib, golden):
    """post_ops.maps_colorize into windows of one buffer pre-filled with 0xAB, at pitches larger than the rows and at window origins that
    are and are not 16-byte aligned: the windows hold matplotlib's bytes and every byte outside them is still 0xAB"""
    from fast3r_amd import _lib, maps, post_ops
    names = ["ragged_37x53", "row_1x1025", "portrait_and_landscape", "one_by_one", "nan_in_the_middle_map"]
    srcs = [golden[f"s/{n}/0/in"] for n in names] + [golden["s/nan_in_the_middle_map/1/in"]]
    want = [golden[f"s/{n}/0/Greys"] for n in names] + [golden["s/nan_in_the_middle_map/1/Greys"]]
    height, width = 140, 1100
    origins = [(1, 3), (40, 8), (45, 1), (139, 1099), (90, 64), (100, 501)]
    canvas = torch.full((height, width, 4), 0xAB, dtype=torch.uint8, device="cuda")
    dsts = [canvas[y:y + s.shape[0], x:x + s.shape[1]] for s, (y, x) in zip(srcs, origins)]
    ranges = post_ops.maps_colorize([dev(s) for s in srcs], dsts, maps._lut_on(canvas.device, "Greys"), mode=_lib.F3R_MAPS_LUT)
    host = canvas.cpu().numpy()
    outside = np.ones((height, width), bool)
    for s, w, (y, x) in zip(srcs, want, origins):
        assert host[y:y + s.shape[0], x:x + s.shape[1]].tobytes() == w.tobytes()
        outside[y:y + s.shape[0], x:x + s.shape[1]] = False
    assert (host[outside] == 0xAB).all()
    assert bits(ranges.cpu().numpy()).tobytes() == bits(numpy_ranges(srcs)).tobytes()
    # the RGB mode through the same windows
    _, views = C.views_case()
    canvas.fill_(0xAB)
    imgs = [v["img"][1] for v in views]
    origins = [(1, 3), (40, 8), (90, 64)]
    dsts = [canvas[y:y + i.shape[1], x:x + i.shape[2]] for i, (y, x) in zip(imgs, origins)]
    assert post_ops.maps_colorize([dev(i) for i in imgs], dsts, mode=_lib.F3R_MAPS_RGB) is None
    host = canvas.cpu().numpy()
    outside[:] = True
    for v, (i, (y, x)) in enumerate(zip(imgs, origins)):
        assert host[y:y + i.shape[1], x:x + i.shape[2]].tobytes() == golden[f"v/{v}/img/1"].tobytes()
        outside[y:y + i.shape[1], x:x + i.shape[2]] = False
    assert (host[outside] == 0xAB).all()
    with pytest.raises(ValueError, match="dense pixels"):
        post_ops.maps_colorize([dev(srcs[0])], [canvas[:37, :106:2]], maps._lut_on(canvas.device, "Greys"))


def test_cpu_tensors_raise(built_lib):
    import fast3r_amd
    from fast3r_amd import _lib
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.colorize_maps([torch.zeros(4, 5)])
    with pytest.raises(_lib.F3RError, match="ROCm device"):
        fast3r_amd.colorize_maps([torch.zeros(4, 5).cuda(), torch.zeros(4, 5)])
    with pytest.raises(ValueError, match="fp32"):
        fast3r_amd.colorize_maps([torch.zeros(4, 5, dtype=torch.float16).cuda()])
    with pytest.raises(ValueError, match="'turbo' and 'Greys'"):
        fast3r_amd.colorize_maps([torch.zeros(4, 5).cuda()], "viridis")


# ------------------------------------------------------------------------------------------------------------------- the plot functions
def want_cells(golden, kind, sample):
    """per view the list of golden pictures (None: the view lacks the key) of one plot function"""
    keys = {"rgb": ["img"], "conf": ["conf"], "local": ["conf_local", "depth_local"]}[kind]
    return [[golden[f"v/{v}/{k}/{sample}"] if f"v/{v}/{k}/{sample}" in golden.files else None for k in keys] for v in range(len(C.VIEW_SHAPES))]


def read_png(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "RGBA"
    return np.asarray(im)


@pytest.mark.parametrize("sample", [0, 1])
@pytest.mark.parametrize("where", ["device", "host"])
def test_plot_functions_equal_matplotlib(built_lib, golden, tmp_path, sample, where):
    """the three functions on a portrait, a landscape and a ragged view, B = 2; view 1 has no conf_local and view 2 no pts3d_local: the
    sheets equal the restatement's sheet of matplotlib's pictures (empty cells and margins 0), and the files decode to those pictures"""
    import fast3r_amd
    preds, views = C.views_case()
    to = dev if where == "device" else torch.from_numpy
    preds = [{k: to(v) for k, v in p.items()} for p in preds]
    views = [{k: to(v) for k, v in vw.items()} for vw in views]
    before = [{k: v.clone() for k, v in p.items()} for p in preds]
    calls = {"rgb": (fast3r_amd.plot_rgb_images, views, ["view_{i}.png"], "RGB_Images.png"),
             "conf": (fast3r_amd.plot_confidence_maps, preds, ["view_{i}_conf.png"], "Confidence_Maps.png"),
             "local": (fast3r_amd.maybe_plot_local_depth_and_conf, preds, ["view_{i}_conf_local.png", "view_{i}_depth_local.png"],
                       "Local_Depth_and_Confidence_Maps.png")}
    for kind, (fn, arg, files, title_file) in calls.items():
        cells = want_cells(golden, kind, sample)
        for max_columns in (8, 2):
            folder = tmp_path / f"{kind}_{max_columns}"
            sheet = fn(arg, save_image_to_folder=str(folder), max_columns=max_columns, sample=sample)
            want = R.sheet(cells, max_columns)
            assert sheet.is_cuda and sheet.dtype == torch.uint8 and tuple(sheet.shape) == want.shape
            assert sheet.cpu().numpy().tobytes() == want.tobytes(), (kind, max_columns)
            expected = {title_file: want}
            for i, row in enumerate(cells):
                for f, p in zip(files, row):
                    if p is not None:
                        expected[f.format(i=i)] = p
            assert sorted(os.listdir(folder)) == sorted(expected)
            for f, p in expected.items():
                assert read_png(folder / f).tobytes() == p.tobytes(), f
        assert torch.equal(fn(arg, sample=sample), torch.from_numpy(R.sheet(cells)).cuda())          # no folder: nothing is written
        nothing = tmp_path / f"{kind}_untitled"
        fn(arg, None, str(nothing), sample=sample)                                        # no title: the views' files only
        assert title_file not in os.listdir(nothing) and len(os.listdir(nothing)) == sum(p is not None for row in cells for p in row)
    for p, b in zip(preds, before):
        assert all(torch.equal(p[k], b[k]) for k in p)
    out = {"preds": preds, "views": views}                                                # what inference() returns goes in as it is
    assert torch.equal(fast3r_amd.plot_confidence_maps(out, sample=sample), torch.from_numpy(R.sheet(want_cells(golden, "conf", sample))).cuda())
    assert torch.equal(fast3r_amd.plot_rgb_images(out, sample=sample), torch.from_numpy(R.sheet(want_cells(golden, "rgb", sample))).cuda())
    with pytest.raises(ValueError, match="sample"):
        fast3r_amd.plot_confidence_maps(preds, sample=2)


# ------------------------------------------------------------------------------------------------------------------- whole functions
@pytest.fixture(scope="module")
def tiny_output():
    from fast3r_amd import Fast3R, MultiViewDUSt3RLitModule, inference
    from fast3r_amd.synthetic import make_views, synth_state_dict, tiny_args
    enc, dec, head = tiny_args()
    m = Fast3R(enc, dec, head).eval()
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0), strict=True)
    lit = MultiViewDUSt3RLitModule.load_for_inference(m.cuda())
    torch.manual_seed(3)
    return inference(make_views(3, 64, 64), lit, torch.device("cuda"), dtype=torch.float16, verbose=False)


def test_on_the_output_of_inference(built_lib, tiny_output, tmp_path):
    """3 views of 64 x 64 through the tiny model: the four notebook functions under their names; the pictures equal the restatement on
    the predictions, the npz loads back with the notebook's structure"""
    import fast3r_amd
    out = tiny_output
    preds, views = out["preds"], out["views"]
    turbo, greys = R.table("turbo"), R.table("Greys")
    folder = tmp_path / "maps"
    sheet = fast3r_amd.plot_confidence_maps(preds, save_image_to_folder=str(folder))
    want = R.sheet([[R.colorize(p["conf"][0].float().numpy(), turbo)] for p in preds])
    assert sheet.cpu().numpy().tobytes() == want.tobytes() and tuple(sheet.shape) == (64, 192, 4)
    sheet = fast3r_amd.maybe_plot_local_depth_and_conf(preds, save_image_to_folder=str(folder))
    want = R.sheet([[R.colorize(p["conf_local"][0].float().numpy(), turbo), R.colorize(p["pts3d_local"][0][..., 2].float().numpy(), greys)]
                    for p in preds])
    assert sheet.cpu().numpy().tobytes() == want.tobytes() and tuple(sheet.shape) == (128, 192, 4)
    sheet = fast3r_amd.plot_rgb_images(views, save_image_to_folder=str(folder))
    want = R.sheet([[R.rgb_picture(v["img"][0].float().numpy())] for v in views])
    assert sheet.cpu().numpy().tobytes() == want.tobytes()
    assert len(os.listdir(folder)) == 4 * 3 + 3
    assert read_png(folder / "view_2_depth_local.png").tobytes() == R.colorize(preds[2]["pts3d_local"][0][..., 2].float().numpy(), greys).tobytes()
    with pytest.raises(KeyError, match="call align_local_pts3d_to_global"):
        fast3r_amd.save_pointmaps_and_camera_parameters_to_folder(preds, str(tmp_path / "early"))
    fast3r_amd.align_local_pts3d_to_global(preds, views)
    path = fast3r_amd.save_pointmaps_and_camera_parameters_to_folder(preds, str(tmp_path / "dump"))
    data = R.check_npz(path, 3, 64, 64)
    assert data["global_pointmaps"].tobytes() == np.stack([p["pts3d_in_other_view"][0].numpy() for p in preds]).tobytes()
    assert data["local_aligned_to_global_pointmaps"].tobytes() == np.stack([p["pts3d_local_aligned_to_global"][0].numpy() for p in preds]).tobytes()
    poses, focals = fast3r_amd.estimate_camera_poses(preds, niter_PnP=100)
    assert np.array_equal(data["estimated_poses_c2w"], np.stack(poses[0]))
    assert np.array_equal(data["estimated_focals"], np.array([np.nan if f is None else f for f in focals[0]]), equal_nan=True)
