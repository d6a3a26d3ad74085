"""Point-cloud export on a real MI355X against the numpy restatement (tests/cloud_ref.py), bit for bit: the arithmetic order is
specified, so there are no tolerances.  Combine (tile edges, percentiles, constant / NaN / signed-zero / inf confidences, batch rows,
flipped axes, saturating colours), the voxel downsampler (sizes around the sort tile, 0 to 6 radix passes, one voxel, own voxels,
boundaries, the colour quirk, refusals), farthest-point sampling (both kernels, ties, repeats, a grid-stride wrap against torch fp64 on
the device), uniform sampling's contract, the whole function on a tiny model, determinism and untouched inputs."""
import numpy as np
import pytest
import torch

import cloud_cases as C
import cloud_ref as R

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8).tobytes()


def same(got, want):
    """a device tensor (or None) against a numpy array (or None): dtype, shape and bytes"""
    if want is None or got is None:
        return want is None and got is None
    g = got.cpu().numpy()
    return g.dtype == want.dtype and g.shape == want.shape and bits(g) == bits(want)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def on_device(preds, views):
    return [{k: dev(v) for k, v in p.items()} for p in preds], [{k: dev(v) for k, v in vw.items()} for vw in views]


@pytest.fixture(scope="module")
def combine_case():
    preds, views = C.combine_case()
    return preds, views, on_device(preds, views)


# ------------------------------------------------------------------------------------------------------------------- combine
@pytest.mark.parametrize("pct", [0, 50, 80, 100])
def test_combine_against_the_restatement(built_lib, combine_case, pct):
    import fast3r_amd
    preds, views, (dp, dv) = combine_case
    keep = [{k: v.clone() for k, v in p.items()} for p in dp], [v["img"].clone() for v in dv]
    for sample, flip in ((0, False), (1, False), (1, True)):
        got = fast3r_amd.combine_points(dp, dv, min_conf_thr_percentile=pct, sample=sample, flip_axes=flip)
        want = R.combine(preds, views, percentile=pct, sample=sample, flip_axes=flip)
        print(f"combine pct {pct} sample {sample} flip {flip}: kept {0 if want[0] is None else len(want[0])}")
        assert same(got[0], want[0]) and same(got[1], want[1]), (pct, sample, flip)
    if pct < 100:
        assert want[0] is not None and len(want[0]) > 1000
    for a, b in zip(keep[0], dp):
        assert all(bits(a[k].cpu().numpy()) == bits(b[k].cpu().numpy()) for k in a)
    assert all(bits(a.cpu().numpy()) == bits(b["img"].cpu().numpy()) for a, b in zip(keep[1], dv))


def test_combine_views_that_keep_nothing(built_lib, combine_case):
    import fast3r_amd
    preds, views, (dp, dv) = combine_case
    n = len(C.COMBINE_PIXELS)
    for i in (n, n + 1):                                             # constant confidence; a NaN confidence
        for pct in (0, 50, 100):
            assert fast3r_amd.combine_points(dp[i:i + 1], dv[i:i + 1], min_conf_thr_percentile=pct) == (None, None)
    i = n + 2                                                        # -0.0 / +0.0 / +inf: -0.0 > -0.0 is false and so is +0.0 > -0.0
    for pct in (0, 50, 80, 100):
        got = fast3r_amd.combine_points(dp[i:i + 1], dv[i:i + 1], min_conf_thr_percentile=pct)
        want = R.combine(preds[i:i + 1], views[i:i + 1], percentile=pct)
        assert same(got[0], want[0]) and same(got[1], want[1]), pct
    assert len(R.combine(preds[i:i + 1], views[i:i + 1], percentile=0)[0]) == 72 - 20
    p1, c1 = fast3r_amd.combine_points(dp[:1], dv[:1], min_conf_thr_percentile=0)     # one pixel is its own minimum
    assert p1 is None and c1 is None


def test_combine_saturates_colours(built_lib, combine_case):
    import fast3r_amd
    preds, views, (dp, dv) = combine_case
    lo = [{C.PTS_KEY: p[C.PTS_KEY], C.CONF_KEY: torch.arange(p[C.CONF_KEY].numel(), device="cuda", dtype=torch.float32).reshape(p[C.CONF_KEY].shape)}
          for p in dp[1:3]]
    _, c = fast3r_amd.combine_points(lo, dv[1:3])                    # every pixel but the first kept, in pixel order
    img = views[1]["img"][0].reshape(3, -1).T[1:]
    assert same(c[:len(img)], R.color_u8(img))
    assert c[4].tolist()[0] == 0 and c[5].tolist()[1] == 255 and c[6].tolist()[2] == 255 and c[9].tolist()[2] == 0   # -1.5, 1.25, 3.0, NaN


# ------------------------------------------------------------------------------------------------------------------- voxel
def run_voxel(p, c, vs):
    from fast3r_amd import post_ops
    out = post_ops.cloud_voxel_down_sample(dev(p), None if c is None else dev(c), vs)
    want = R.voxel_down_sample(p, c, vs)
    ok = same(out["points"], want[0]) and same(out["colors"], want[1]) and same(out["counts"], want[2])
    return ok, out, want


@pytest.mark.parametrize("n", C.VOXEL_SIZES)
def test_voxel_sizes_around_the_sort_tile(built_lib, n):
    p, c = C.random_cloud(n, 100 + n)
    ok, out, want = run_voxel(p, c, 0.5)
    print(f"voxel n {n}: {len(want[0])} voxels, bits {out['bits']}, passes {out['passes']}")
    assert ok and out["bits"] == R.key_bits(p, 0.5)
    if n > 1000:
        assert 100 < len(want[0]) < n and want[2].max() > 1
    ok, _, _ = run_voxel(p, None, 0.5)
    assert ok


@pytest.mark.parametrize("recipe", ["one_voxel", "own_voxels", "on_boundaries", "duplicates", "small_integers", "own_voxels_1023", "own_voxels_1024",
                                    "own_voxels_1025"])
def test_voxel_recipes(built_lib, recipe):
    import fast3r_amd
    p, c, vs = getattr(C, recipe)()
    ok, out, want = run_voxel(p, c, vs)
    assert ok, recipe
    if recipe == "one_voxel":
        assert want[2].tolist() == [5000] and out["passes"] == 0
    if recipe.startswith("own_voxels"):
        assert len(want[0]) == len(p) and same(out["colors"], want[1])
    gp, gc, gn = fast3r_amd.voxel_down_sample(dev(p), dev(c), vs)   # the public name returns the same three
    assert torch.equal(gp, out["points"]) and torch.equal(gc, out["colors"]) and torch.equal(gn, out["counts"])


def test_voxel_colour_quirk_and_extremes(built_lib):
    p, c, vs, listed = C.quirk_colors()
    ok, out, want = run_voxel(p, c, vs)
    assert ok
    got = out["colors"].cpu().numpy()[1:, 0].tolist()
    assert got[:3] == [0, 255, 255] and sum(g == cc - 1 for g, (cc, _) in zip(got[3:], listed[3:])) == 173


@pytest.mark.parametrize("total", sorted(C.BIT_CASES))
def test_voxel_key_widths_and_pass_counts(built_lib, total):
    want_bits = C.BIT_CASES[total]
    p, c, vs = C.bits_cloud(want_bits)
    ok, out, want = run_voxel(p, c, vs)
    print(f"voxel key {total} bits: {out['bits']}, {out['passes']} passes, {len(want[0])} voxels")
    assert out["bits"] == list(want_bits) and sum(out["bits"]) == total and out["passes"] == -(-total // 8)
    assert ok and want[2].max() > 1 and len(want[0]) > 150


def test_voxel_pass_counts_cover_one_to_six(built_lib):
    assert sorted({-(-t // 8) for t in C.BIT_CASES}) == [1, 2, 3, 4, 5, 6] and sorted(C.BIT_CASES) == [8, 9, 16, 17, 24, 25, 40, 41]


def test_voxel_heuristic_path(built_lib):
    import fast3r_amd
    p, c = C.random_cloud(5000, 31)
    gp, gc = fast3r_amd.downsample_cloud(dev(p), dev(c), 500, "voxel")
    wp, wc = R.downsample(p, c, 500, "voxel")
    print(f"voxel heuristic: 5000 -> {len(wp)} for max_num_points 500, voxel_size {R.heuristic_voxel_size(p, 500)}")
    assert same(gp, wp) and same(gc, wc) and 100 < len(wp) < 2000
    gp, gc = fast3r_amd.downsample_cloud(dev(p), dev(c), 500, "voxel", voxel_size=0.7)
    wp, wc = R.downsample(p, c, 500, "voxel", voxel_size=0.7)
    assert same(gp, wp) and same(gc, wc)
    same_p, same_c = fast3r_amd.downsample_cloud(dev(p), dev(c), 5000, "voxel")
    assert same(same_p, p) and same(same_c, c)                      # not more than max_num_points: unchanged
    assert fast3r_amd.downsample_cloud(dev(p), dev(c), None, "no such strategy")[0].shape == (5000, 3)   # as in the notebook
    with pytest.raises(ValueError, match="Unsupported sampling strategy: octree"):
        fast3r_amd.downsample_cloud(dev(p), dev(c), 500, "octree")


def test_voxel_refusals(built_lib):
    import fast3r_amd
    p, c = C.random_cloud(300, 41)
    planar = p.copy()
    planar[:, 2] = 1.5
    with pytest.raises(ValueError, match="voxel_size"):
        fast3r_amd.downsample_cloud(dev(planar), dev(c), 100, "voxel")            # the heuristic gives 0
    with pytest.raises(ValueError, match="voxel_size"):
        fast3r_amd.voxel_down_sample(dev(p), dev(c), 0.0)
    with pytest.raises(ValueError, match="voxel_size too small for this extent"):
        fast3r_amd.voxel_down_sample(dev(p), dev(c), 1e-7)                        # 26 + 25 + 25 bits
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[17, 1] = bad
        with pytest.raises(ValueError, match="NaN or inf"):
            fast3r_amd.voxel_down_sample(dev(q), dev(c), 0.5)
        with pytest.raises(ValueError, match="NaN or inf"):
            fast3r_amd.downsample_cloud(dev(q), dev(c), 100, "voxel")
        with pytest.raises(ValueError, match="NaN or inf"):
            fast3r_amd.farthest_point_down_sample(dev(q), 5)


# ------------------------------------------------------------------------------------------------------------------- farthest point
ONE, TILED = 1, 2


def fps(p, k, start=0, mode=0):
    import fast3r_amd
    return fast3r_amd.farthest_point_down_sample(dev(p), k, start, mode=mode)


@pytest.mark.parametrize("n,k", C.FPS_SIZES)
def test_fps_sizes_in_both_kernels(built_lib, n, k):
    p, _ = C.random_cloud(n, 200 + n)
    want = R.farthest_point_down_sample(p, k)
    for mode in (0, ONE, TILED):
        assert same(fps(p, k, 0, mode), want), (n, k, mode)
    start = n // 2
    want = R.farthest_point_down_sample(p, k, start)
    assert same(fps(p, k, start, ONE), want) and same(fps(p, k, start, TILED), want) and want[0] == start


def test_fps_tiled_over_several_tiles(built_lib):
    n, k = 3 * C.FT + 17, 257
    p, _ = C.random_cloud(n, 77)
    want = R.farthest_point_down_sample(p, k, 5)
    a, b = fps(p, k, 5, TILED), fps(p, k, 5, ONE)
    assert same(a, want) and torch.equal(a, b) and len(set(want.tolist())) == k


def test_fps_lattice_ties_take_the_smallest_index(built_lib):
    p = C.lattice()
    want = R.farthest_point_down_sample(p, 40)
    assert R.fps_ties(p, 40) >= 30
    assert same(fps(p, 40, 0, ONE), want) and same(fps(p, 40, 0, TILED), want)
    far = np.tile(p, (20, 1))                                        # 2500 points, every one 20 times: ties across tiles and workgroups
    want = R.farthest_point_down_sample(far, 60, 1300)
    assert same(fps(far, 60, 1300, ONE), want) and same(fps(far, 60, 1300, TILED), want)


def test_fps_cloud_that_runs_out_of_distinct_points(built_lib):
    import fast3r_amd
    p, c = C.few_distinct()
    want = R.farthest_point_down_sample(p, 40)
    assert len(set(want[10:].tolist())) == 1 and len(set(want.tolist())) == 10
    assert same(fps(p, 40, 0, ONE), want) and same(fps(p, 40, 0, TILED), want)
    gp, gc = fast3r_amd.downsample_cloud(dev(p), dev(c), 40, "farthest_point")
    wp, wc = R.downsample(p, c, 40, "farthest_point")
    assert len(wp) == 10 and same(gp, wp) and same(gc, wc)
    gp, gc = fast3r_amd.downsample_cloud(dev(p), dev(c), 40, "farthest_point", order="selection")
    wp, wc = R.downsample(p, c, 40, "farthest_point", order="selection")
    assert len(wp) == 40 and same(gp, wp) and same(gc, wc)


def test_fps_both_orders_on_a_plain_cloud(built_lib):
    import fast3r_amd
    p, c = C.random_cloud(9000, 55)                                  # above the one-workgroup bound: the tiled kernel by default
    for order in ("index", "selection"):
        gp, gc = fast3r_amd.downsample_cloud(dev(p), dev(c), 300, "farthest_point", order=order)
        wp, wc = R.downsample(p, c, 300, "farthest_point", order=order)
        assert len(wp) == 300 and same(gp, wp) and same(gc, wc), order
    with pytest.raises(ValueError, match="order"):
        fast3r_amd.downsample_cloud(dev(p), dev(c), 300, "farthest_point", order="random")


def test_fps_argument_checks(built_lib):
    import fast3r_amd
    p = dev(C.random_cloud(50, 3)[0])
    for k in (0, 51, -1):
        with pytest.raises(ValueError, match="num_samples"):
            fast3r_amd.farthest_point_down_sample(p, k)
    for s in (-1, 50):
        with pytest.raises(ValueError, match="start_index"):
            fast3r_amd.farthest_point_down_sample(p, 5, s)
    big = torch.zeros((C._lib.CLOUD_FPS_ONE_MAX + 1, 3), device="cuda")
    with pytest.raises(ValueError, match="mode"):
        fast3r_amd.farthest_point_down_sample(big, 2, mode=ONE)


def test_fps_grid_stride_wrap_against_torch_fp64(built_lib):
    """more tiles than workgroups: the tiled kernel's grid-stride assignment wraps; inputs made on the device"""
    n, k = 1024 * C.FT + 4097, 8
    g = torch.Generator(device="cuda").manual_seed(9)
    p = torch.rand((n, 3), device="cuda", generator=g) * 5.0
    p[n - 3] = torch.tensor([40.0, 40.0, 40.0], device="cuda")       # the farthest point lives in the wrapped tail
    got = fps_device(p, k, 11)
    p64 = p.double()
    d = torch.full((n,), float("inf"), dtype=torch.float64, device="cuda")
    far, want = 11, []
    for _ in range(k):
        want.append(far)
        diff = p64 - p64[far]
        d = torch.minimum(d, (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
        m = d.max()
        if float(m) > 0:
            far = int(torch.nonzero(d == m)[0])
    assert got.cpu().tolist() == want and want[1] == n - 3


def fps_device(p, k, start):
    import fast3r_amd
    return fast3r_amd.farthest_point_down_sample(p, k, start)


# ------------------------------------------------------------------------------------------------------------------- uniform
def test_uniform_contract(built_lib):
    import fast3r_amd
    n, m = 5000, 700
    p = np.arange(n, dtype=np.float32)[:, None] * np.ones(3, np.float32)          # row i is (i, i, i): a row names its index
    c = (np.arange(n)[:, None] % np.array([251, 241, 239])).astype(np.uint8)
    dp, dc = dev(p), dev(c)
    g = torch.Generator(device="cuda").manual_seed(4)
    a = fast3r_amd.downsample_cloud(dp, dc, m, "uniform", generator=g)
    idx = a[0][:, 0].long().cpu().numpy()
    assert a[0].shape == (m, 3) and a[1].shape == (m, 3) and a[0].dtype == torch.float32 and a[1].dtype == torch.uint8
    assert len(set(idx.tolist())) == m and idx.min() >= 0 and idx.max() < n
    assert same(a[0], p[idx]) and same(a[1], c[idx]) and not np.array_equal(idx, np.sort(idx))
    b = fast3r_amd.downsample_cloud(dp, dc, m, "uniform", generator=torch.Generator(device="cuda").manual_seed(4))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    other = fast3r_amd.downsample_cloud(dp, dc, m, "uniform", generator=torch.Generator(device="cuda").manual_seed(5))
    assert not torch.equal(a[0], other[0])
    assert same(dp, p) and same(dc, c)


# ------------------------------------------------------------------------------------------------------------------- the whole function
@pytest.fixture(scope="module")
def tiny_output(built_lib):
    import fast3r_amd
    from fast3r_amd import Fast3R, MultiViewDUSt3RLitModule, inference
    from fast3r_amd.synthetic import make_views, synth_state_dict, tiny_args
    enc, dec, head = tiny_args()
    m = Fast3R(enc, dec, head).eval()
    m.load_state_dict(synth_state_dict({k: v.shape for k, v in m.state_dict().items()}, seed=0), strict=True)
    lit = MultiViewDUSt3RLitModule.load_for_inference(m.cuda())
    torch.manual_seed(3)
    out = inference(make_views(3, 64, 64), lit, torch.device("cuda"), dtype=torch.float16, verbose=False)
    fast3r_amd.align_local_pts3d_to_global(out["preds"], out["views"])
    return out


def as_numpy(out):
    preds = [{k: p[k].float().cpu().numpy() for k in (C.PTS_KEY, C.CONF_KEY)} for p in out["preds"]]
    return preds, [{"img": v["img"].float().cpu().numpy()} for v in out["views"]]


@pytest.mark.parametrize("strategy", ["uniform", "voxel", "farthest_point"])
def test_export_combined_ply_end_to_end(built_lib, tiny_output, tmp_path, strategy):
    import fast3r_amd
    out = tiny_output
    preds, views = as_numpy(out)
    full_p, full_c = R.combine(preds, views, percentile=10)
    path = tmp_path / f"{strategy}.ply"
    g = torch.Generator(device="cuda").manual_seed(1) if strategy == "uniform" else None
    gp, gc = fast3r_amd.export_combined_ply(out["preds"], out["views"], str(path), min_conf_thr_percentile=10, max_num_points=400,
                                            sampling_strategy=strategy, generator=g)
    assert gp.is_cuda and gc.is_cuda and gp.dtype == torch.float32 and gc.dtype == torch.uint8 and len(full_p) > 10000
    if strategy == "uniform":
        assert gp.shape == (400, 3)
        rows = {bits(r) for r in np.concatenate([full_p.view(np.uint8), full_c], axis=1)}
        assert all(bits(r) in rows for r in np.concatenate([gp.cpu().numpy().view(np.uint8), gc.cpu().numpy()], axis=1))
    else:
        wp, wc = R.downsample(full_p, full_c, 400, strategy)
        assert same(gp, wp) and same(gc, wc)
    fp, fc = R.parse_ply(path.read_bytes())
    assert same(gp, fp) and same(gc, fc)


def test_export_combined_ply_input_forms_and_small_clouds(built_lib, tiny_output, tmp_path):
    import fast3r_amd
    out = tiny_output
    preds, views = as_numpy(out)
    want = R.combine(preds, views, percentile=0)
    a = fast3r_amd.export_combined_ply(out["preds"], out["views"])                          # what inference() returns: host tensors
    assert not out["preds"][0][C.CONF_KEY].is_cuda and a[0].is_cuda and same(a[0], want[0]) and same(a[1], want[1])
    b = fast3r_amd.export_combined_ply(out, None, max_num_points=len(want[0]), sampling_strategy="voxel")   # the dict; nothing to bound
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    dp = [{k: v.cuda() for k, v in p.items() if torch.is_tensor(v)} for p in out["preds"]]
    dv = [{"img": v["img"].cuda()} for v in out["views"]]
    c = fast3r_amd.export_combined_ply(dp, dv, max_num_points=10 ** 6, flip_axes=True)      # device tensors
    wf = R.combine(preds, views, percentile=0, flip_axes=True)
    assert same(c[0], wf[0]) and same(c[1], wf[1])
    const = [{C.PTS_KEY: p[C.PTS_KEY], C.CONF_KEY: torch.ones_like(p[C.CONF_KEY])} for p in dp]
    path = tmp_path / "none.ply"
    assert fast3r_amd.export_combined_ply(const, dv, str(path)) == (None, None) and not path.exists()
    scene = fast3r_amd.assemble_scene(out, poses=False)                                     # what collect_points returns goes in as it is
    sp, sc = scene.collect_points()
    vp, vc = fast3r_amd.downsample_cloud(sp, sc, 300, "voxel")
    wp, wc = R.downsample(sp.cpu().numpy(), sc.cpu().numpy(), 300, "voxel")
    assert same(vp, wp) and same(vc, wc)
    assert fast3r_amd.downsample_cloud(None, None, 300, "voxel") == (None, None)


def test_two_runs_give_the_same_bits_and_inputs_stay(built_lib):
    import fast3r_amd
    p, c = C.random_cloud(3 * C.ST + 211, 8)
    dp, dc = dev(p), dev(c)
    for strategy, kw in (("voxel", {}), ("farthest_point", {}), ("farthest_point", {"order": "selection"})):
        a = fast3r_amd.downsample_cloud(dp, dc, 200, strategy, **kw)
        b = fast3r_amd.downsample_cloud(dp, dc, 200, strategy, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), strategy
    assert same(dp, p) and same(dc, c)
