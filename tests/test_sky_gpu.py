"""Sky detection on the GPU (fast3r_amd/sky.py, fast3r_amd/csrc/f3r_sky.hip) against the reference's recorded results
(tests/golden/sky_cases.pt) and the numpy restatement (tests/sky_ref.py): every comparison is exact.  The kernels tile the WORDS of the
bit-packed bitmap (16 per workgroup where a wave owns a word, 256 where a thread does), never the image, and keep nothing per view in
LDS, so there is no view size at which another path is taken; the shapes below put word, row and tile borders everywhere else."""
import numpy as np
import pytest
import torch

import sky_cases as C
import sky_ref as R
from fast3r_amd import _lib, assemble_scene, detect_sky_mask, detect_sky_masks, generate_ply_bytes, label_components, post_ops, sky

pytestmark = pytest.mark.gpu
GOLDEN_KEYS = ("sky_pixels", "components", "components_top", "components_kept")


@pytest.fixture(scope="module")
def golden():
    import os
    return torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky_cases.pt"), weights_only=False)


def _view(img_hw3, dev="cuda"):
    return {"img": torch.from_numpy(img_hw3).permute(2, 0, 1)[None].contiguous().to(dev)}


def test_every_golden_case_in_one_batched_call(built_lib, golden):
    """72 views of eight different (H, W) in the same launches: not_sky, the stats and the branch equal the reference's, bit for bit"""
    views = [_view(C.build(*c)) for c in C.CASES]
    masks, stats = detect_sky_masks(views)
    assert len(masks) == len(stats) == len(C.CASES)
    for (scene, H, W), m, st in zip(C.CASES, masks, stats):
        g = golden["cases"][C.case_name(scene, H, W)]
        want = np.unpackbits(g["not_sky_bits"].numpy())[:H * W].reshape(H, W).astype(np.int8)
        assert m.dtype == torch.int8 and m.is_cuda and tuple(m.shape) == (H, W)
        assert np.array_equal(m.cpu().numpy(), want), (scene, H, W)
        assert [st[k] for k in GOLDEN_KEYS] == g["stats"] and st["branch"] == g["branch"], (scene, H, W, st, g)


def test_all_colours_above_and_below_the_upper_region(built_lib):
    """4096 x 4096 images whose pixel (y, x) has the colour number ((y + roll) % 4096) * 4096 + x = r << 16 | g << 8 | b, with values that
    truncate back to the byte with half a unit of margin.  Three rolls put every one of the 2^24 colours once above and once below
    int(H * 0.4); the pre-morphology bitmap equals the restatement exactly."""
    N = 4096
    u = np.arange(256, dtype=np.uint8)
    lut = (u.astype(np.float32) + np.float32(0.5)) / np.float32(127.5) - np.float32(1)
    assert np.array_equal(R.to_u8(lut), u)
    upper = int(N * 0.4)
    rolls = (0, upper, 2 * upper)
    assert 3 * upper >= N and N - upper >= upper   # three bands of `upper` rows cover all colour rows above; the rest covers them below
    col = np.arange(N * N, dtype=np.int64)
    h, s, v = R.hsv_u8(col >> 16, (col >> 8) & 255, col & 255)
    base = R.sky_coloured(h, s, v, np.zeros((), bool)).reshape(N, N)
    in_up = base | ((s < 50) & (v > 150)).reshape(N, N)   # sky_coloured(..., in_upper=True)
    assert np.array_equal(in_up[:64], R.sky_coloured(h[:64 * N], s[:64 * N], v[:64 * N], np.ones((), bool)).reshape(64, N))
    assert 0 < base.sum() < in_up.sum() < N * N
    dev = torch.device("cuda")
    lut_d = torch.from_numpy(lut).to(dev)
    col_d = torch.arange(N * N, device=dev, dtype=torch.int64).reshape(N, N)
    planes = []
    for roll in rolls:
        c = torch.roll(col_d, -roll, 0).reshape(-1)   # row y shows colour row (y + roll) % N
        planes.append(torch.stack([lut_d[(c >> 16) & 255], lut_d[(c >> 8) & 255], lut_d[c & 255]]))
    out = post_ops.sky_detect(planes, [(N, N)] * 3, _lib.F3R_SKY_CLASSIFY)
    n_words = N * N // 64
    seen_up, seen_down = np.zeros(N, bool), np.zeros(N, bool)
    for i, roll in enumerate(rolls):
        want = np.roll(base, -roll, 0)
        want[:upper] = np.roll(in_up, -roll, 0)[:upper]
        got = sky.unpack_bits(out["bits"][i * n_words:(i + 1) * n_words], N, N)
        assert torch.equal(got, torch.from_numpy(want).to(dev)), roll
        rows = (np.arange(N) + roll) % N
        seen_up[rows[:upper]] = True
        seen_down[rows[upper:]] = True
    assert seen_up.all() and seen_down.all()


def test_imgnorm_values_on_colour_slices(built_lib):
    """what real inputs look like: ((u / 255) - 0.5) / 0.5, which the reference's conversion mostly does NOT bring back to u"""
    u = np.arange(256, dtype=np.uint8)
    g, b = np.meshgrid(u, u, indexing="ij")
    slices = [np.stack([np.full_like(g, 100), g, b], -1), np.stack([g, np.full_like(g, 150), b], -1), np.stack([g, b, np.full_like(g, 230)], -1)]
    imgs = [C.normalise(s) for s in slices]
    out = post_ops.sky_detect([torch.from_numpy(i).permute(2, 0, 1).reshape(3, -1).contiguous().cuda() for i in imgs], [(256, 256)] * 3,
                              _lib.F3R_SKY_CLASSIFY)
    for i, img in enumerate(imgs):
        got = sky.unpack_bits(out["bits"][i * 1024:(i + 1) * 1024], 256, 256).cpu().numpy()
        want = R.classify(img)
        assert 0 < want.sum() < want.size and np.array_equal(got, want), i
    # outside [-1, 1] the stated deviation: saturation, NaN as 0
    wild = np.random.default_rng(3).uniform(-1.6, 1.6, size=(40, 70, 3)).astype(np.float32)
    wild[5, 5] = np.nan
    assert np.array_equal(sky.classify(np.ascontiguousarray(wild.transpose(2, 0, 1))), R.classify(wild, saturate=True))


def _morph_cases():
    rng = np.random.default_rng(17)
    cases = []
    for W in (63, 64, 65, 127, 129):
        for H, dens in ((3, 0.05), (6, 0.5), (7, 0.005), (8, 0.05), (37, 0.005), (37, 0.5), (90, 0.05)):   # 90 x 129: 270 words, two word tiles
            cases.append(rng.random((H, W)) < dens)
    H, W = 20, 130
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)):
        m = np.zeros((H, W), bool)
        m[y, x] = True
        cases.append(m)
    for x in range(54, 75):   # every position of a crossing of the word border at x = 64, alone and next to a second word border
        m = np.zeros((H, W), bool)
        m[9, x] = True
        m[2, min(W - 1, x + 60)] = True
        cases.append(m)
    for y in range(0, 14):    # every position of a crossing of the word-tile border (256 words = row 85.33 at 3 words per row)
        m = np.zeros((100, 129), bool)
        m[78 + y, 64] = True
        cases.append(m)
    cases.append(np.ones((9, 70), bool))
    cases.append(np.zeros((9, 70), bool))
    return cases


def test_morphology_alone_on_word_and_tile_borders(built_lib):
    cases = _morph_cases()
    out = post_ops.sky_detect([torch.from_numpy(m.astype(np.int8)).cuda() for m in cases], [m.shape for m in cases], _lib.F3R_SKY_MORPH)
    offs = out["word_offsets"] + [out["bits"].numel()]
    n_changed = 0
    for i, m in enumerate(cases):
        H, W = m.shape
        got = sky.unpack_bits(out["bits"][offs[i]:offs[i + 1]], H, W).cpu().numpy()
        want = R.morphology(m)
        assert np.array_equal(got, want), (i, m.shape, int(m.sum()))
        n_changed += int((want != m).any())
    assert n_changed > len(cases) // 2
    assert np.array_equal(sky.morphology(cases[3]), R.morphology(cases[3]))   # the single-view wrapper, numpy in and out


def _label_cases():
    cases = dict(C.stress_bitmaps())
    cases["noise59_big"] = C.noise(300, 517, 0.59, 9)   # near the percolation threshold: long chains over many tiles
    return cases


def test_components_alone_on_bitmaps_morphology_never_emits(built_lib):
    cases = _label_cases()
    names = list(cases)
    src = [torch.from_numpy(cases[n].astype(np.int8)).cuda() for n in names]
    out = post_ops.sky_detect(src, [cases[n].shape for n in names], _lib.F3R_SKY_LABEL, want_not_sky=True, want_roots=True)
    stats = sky.stats_dicts(out["stats"])
    for i, n in enumerate(names):
        m = cases[n]
        roots, count = R.label_roots(m)
        want_sky, want_stats = R.select(m)
        assert np.array_equal(out["roots"][i].cpu().numpy(), roots), n
        assert stats[i] == want_stats and stats[i]["components"] == count, (n, stats[i], want_stats)
        assert np.array_equal(out["not_sky"][i].cpu().numpy(), (~want_sky).astype(np.int8)), n
    assert R.label_roots(cases["diagonal_pair"])[1] == 2 and R.label_roots(cases["checkerboard"])[1] == 96 * 128 // 2
    assert {s["branch"] for s in stats} == {"empty", "no_top", "top"}
    # the public wrapper: numpy in -> numpy out; tensor in -> tensor on its device
    r_np, c_np = label_components(cases["spiral"])
    assert isinstance(r_np, np.ndarray) and r_np.dtype == np.int32 and np.array_equal(r_np, R.label_roots(cases["spiral"])[0]) and c_np == 1
    r_t, c_t = label_components(torch.from_numpy(cases["noise40"]).cuda())
    assert r_t.is_cuda and r_t.dtype == torch.int32 and np.array_equal(r_t.cpu().numpy(), R.label_roots(cases["noise40"])[0])
    assert c_t == R.label_roots(cases["noise40"])[1]


def _scene(scenes, shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    preds, views, masks = [], [], []
    for scene, (H, W) in zip(scenes, shapes):
        img = C.build(scene, H, W)
        views.append(_view(img))
        masks.append(R.detect_sky_mask(img)[0])
        preds.append({"pts3d_in_other_view": torch.randn(1, H, W, 3, generator=gen).cuda(), "conf": (1 + 3 * torch.rand(1, H, W, generator=gen)).cuda(),
                      "pts3d_local_aligned_to_global": torch.randn(1, H, W, 3, generator=gen).cuda(),
                      "conf_local": (1 + 3 * torch.rand(1, H, W, generator=gen)).cuda()})
    return preds, views, masks


@pytest.mark.parametrize("kind", ["outdoor", "indoor"])
def test_assemble_scene_detect_equals_the_restated_masks(built_lib, kind):
    if kind == "outdoor":
        preds, views, masks = _scene(("outdoor", "outdoor_lake", "partial_top", "indoor"), ((48, 64), (37, 53), (64, 48), (48, 64)), 1)
    else:
        preds, views, masks = _scene(("indoor", "top_pixel", "lake_only", "indoor"), ((48, 64), (48, 64), (37, 53), (64, 48)), 2)
    got = assemble_scene(preds, views, not_sky="detect", poses=False)
    want = assemble_scene(preds, views, not_sky=masks, poses=False)
    none = assemble_scene(preds, views, poses=False)
    assert got.is_outdoor == want.is_outdoor == (kind == "outdoor") and none.is_outdoor is False
    for a, b, c in zip(got.frames, want.frames, none.frames):
        assert a.keys() == b.keys()
        for k in a:
            if torch.is_tensor(a[k]):
                assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
        assert bool((c["sorted_not_sky_global"] == 1).all()) and bool((c["sorted_not_sky_local"] == 1).all())
    assert generate_ply_bytes(*got.collect_points()) == generate_ply_bytes(*want.collect_points())
    assert generate_ply_bytes(*got.collect_points(mask_sky=True, show_global=True)) == generate_ply_bytes(*want.collect_points(mask_sky=True, show_global=True))
    if kind == "outdoor":   # the sky really is cut from the export
        assert got.collect_points(mask_sky=True)[0].shape[0] < got.collect_points(mask_sky=False)[0].shape[0]


def test_two_runs_give_the_same_bits_and_inputs_stay(built_lib):
    cases = [("partial_top", 224, 288), ("noise", 96, 128), ("outdoor_lake", 37, 53), ("bluish_noise", 64, 1)]
    views = [_view(C.build(*c)) for c in cases]
    before = [v["img"].clone() for v in views]
    m1, s1 = detect_sky_masks(views)
    m2, s2 = detect_sky_masks(views)
    assert s1 == s2 and all(torch.equal(a, b) for a, b in zip(m1, m2))
    assert all(torch.equal(v["img"], b) for v, b in zip(views, before))
    noisy = torch.from_numpy(C.noise(300, 517, 0.59, 9).astype(np.int8)).cuda()
    r1, r2 = label_components(noisy)[0], label_components(noisy)[0]
    assert torch.equal(r1, r2)
    # the reference's signature: numpy in -> numpy int8 out, equal to the device path; a host tensor comes back on the host
    img = C.build("partial_top", 224, 288)
    out = detect_sky_mask(img)
    assert isinstance(out, np.ndarray) and out.dtype == np.int8 and np.array_equal(out, m1[0].cpu().numpy())
    out_t = detect_sky_mask(torch.from_numpy(img).cuda())
    assert out_t.is_cuda and out_t.dtype == torch.int8 and torch.equal(out_t, m1[0])
    assert not detect_sky_mask(torch.from_numpy(img)).is_cuda
    # host views, as inference() returns them
    mh, sh = detect_sky_masks([{"img": v["img"].cpu()} for v in views])
    assert sh == s1 and all(m.is_cuda and torch.equal(a, m) for a, m in zip(m1, mh))
