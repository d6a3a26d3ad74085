"""No GPU: the cases of tests/compact_cases.py reach the edges they are named for, the walk restated there -- last_le over the tile starts,
stop = min(base + T, end), 64-element steps, rank = kept lanes below, an exclusive scan over n_tiles + 1 words, two streams on one flags call
-- stores exactly what a plain boolean index keeps on every case, and every deliberately wrong variant of it differs on a named case.  The
argument that the GPU module would notice such a defect in a kernel is made here: no mutated kernel is built or run."""
import os
import re

import numpy as np
import pytest

import compact_cases as C
from fast3r_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def constant(text, name):
    return int(re.search(rf"constexpr int {name} = (\d+);", text).group(1))


def define(name):
    return int(re.search(rf"#define {name} (\d+)", source("include", "f3r.h")).group(1))


# ================================================================================================ constants, fills
def test_tile_constants_match_the_kernel_source_the_header_and_the_bindings():
    csrc = ("fast3r_amd", "csrc")
    assert C.T_COLLECT == _lib.COLLECT_TILE == constant(source(*csrc, "f3r_scene.hip"), "COL_TILE") == 1024
    assert C.T_CLOUD == _lib.CLOUD_TILE == constant(source(*csrc, "f3r_cloud.hip"), "CLOUD_TILE") == define("F3R_CLOUD_TILE")
    assert C.T_MESH == _lib.MESH_TILE == constant(source(*csrc, "f3r_mesh.hip"), "MESH_TILE") == define("F3R_MESH_TILE")
    assert C.T_DEPTH == _lib.DEPTH_TILE == constant(source(*csrc, "f3r_depth.hip"), "TILE") == define("F3R_DEPTH_TILE")
    assert C.T_RECON == constant(source(*csrc, "f3r_recon.hip"), "TILE") == 2048
    assert C.T_MATCH == _lib.MATCH_TILE == constant(source(*csrc, "f3r_match.hip"), "MATCH_TILE") == define("F3R_MATCH_TILE")
    assert C.SCAN_NT == constant(source(*csrc, "f3r_prims.h"), "SCAN_NT")
    assert all(T % C.WAVE == 0 for T in (C.T_COLLECT, C.T_CLOUD, C.T_MESH, C.T_DEPTH, C.T_RECON, C.T_MATCH))


def test_the_predicate_fill_reads_as_kept_and_the_data_fill_as_poison():
    pred, data = bytes([C.PRED_FILL]) * 4, bytes([C.DATA_FILL]) * 4
    f = np.frombuffer(pred, np.float32)[0]
    assert np.isfinite(f) and f > 3.3e38                                  # above every threshold, >= every quantile, g > 0 and finite
    assert np.frombuffer(pred, np.int8)[0] == 127 and np.frombuffer(pred, np.uint8)[0] != 0
    assert np.frombuffer(pred, np.int32)[0] > 2 * C.T_MATCH + 17          # as a neighbour index: out of range (dropped, see compact_cases)
    assert np.isnan(np.frombuffer(data, np.float32)[0]) and np.frombuffer(data, np.int8)[0] == -1   # what 0xFF would read as: never kept
    assert C.SENTINEL_BYTE not in (C.PRED_FILL, C.DATA_FILL, 0)


# ================================================================================================ lengths, patterns
@pytest.mark.parametrize("T", [1024, 2048])
def test_lengths_take_both_branches_of_tile_compact(T):
    L = C.lengths(T)
    assert L == (1, 63, 64, 65, T - 65, T - 64, T - 63, T - 1, T, T + 1, 2 * T, 2 * T + 17)
    def steps(n):                              # steps of the last tile, elements of its ragged step
        last = (n - 1) % T + 1
        return (last + 63) // 64, last % 64
    assert steps(T - 64) == (T // 64 - 1, 0) and steps(T - 63) == (T // 64, 1) and steps(T - 1) == (T // 64, 63)
    assert [n for n in L if n % T == 0] == [T, 2 * T]                      # the unrolled full-tile branch
    pairs = C.pairings(T)
    assert len(pairs) == len(set(pairs)) == 3 * len(C.PATTERNS) + 9 * 3
    for n in L:
        assert {"half", "last", "lane63"} <= {p for m, p in pairs if m == n}
    for n in (T - 1, T, 2 * T + 17):
        assert {p for m, p in pairs if m == n} == set(C.PATTERNS)


@pytest.mark.parametrize("T", [1024, 2048])
def test_patterns_reach_their_edges(T):
    for n in C.lengths(T):
        last = C.pattern("last", n, T)
        assert np.flatnonzero(last).tolist() == [n - 1] and (n - 1) % 64 == ((n - 1) % T) % 64   # the last tile's last occupied lane
        l63 = C.pattern("lane63", n, T)
        whole = n // 64
        assert l63.sum() == whole and not l63[whole * 64:].any()          # one keeper per whole step, none in a ragged step
        assert all(l63[s * 64:(s + 1) * 64].sum() == 1 and l63[s * 64 + 63] for s in range(whole))
    n = 2 * T + 17
    hole = C.pattern("hole", n, T)
    assert hole[:T].all() and not hole[T:2 * T].any() and hole[2 * T:].all()   # tile 1 of three counts zero
    assert C.tile_scan([hole.astype(np.int64)], T).tolist() == [0, T, T, T + 17]
    st = C.pattern("straddle", n, T)
    assert st[T - 65:T + 65].all() and st[2 * T - 65:2 * T + 17].all() and not st[65:T - 65].any()
    half = C.pattern("half", n, T)
    assert 0.4 < half.mean() < 0.6 and not np.array_equal(half, C.pattern("half", n, T, seed=1))


def test_scan_cases_give_a_scan_thread_two_and_three_words():
    for name, tiles, per in (("scan-1025", 1025, 2), ("scan-2049", 2049, 3)):
        c = C.by_name(C.SCENE, name)
        ts = C.tile_starts(c.lens, C.T_COLLECT)
        assert len(c.lens) == 5 and ts[-1] == tiles and C.scan_words_per_thread(tiles) == per and C.scan_words_per_thread(tiles + 1) == per
        assert {(-n) % C.T_COLLECT for n in c.lens} == {0, 1, 63, 64, 65}
    assert C.scan_words_per_thread(1024) == 1
    assert max(sum(c.lens) for c in C.SCENE) == sum(C.by_name(C.SCENE, "scan-2049").lens) < 2.2e6   # the largest case of the suite
    assert C.ragged_lens(1024) == (65, 1024, 1)


# ================================================================================================ the cases of each family
def family_flags():
    """every case of every family as (family, name, tile, streams, flags per segment, scan convention)"""
    out = []
    for c in C.SCENE:
        out.append(("scene", c.name, C.T_COLLECT, 1, C.scene_flags(C.scene_data(c.name)), False))
    for c in C.CLOUD:
        out.append(("cloud", c.name, C.T_CLOUD, 1, C.cloud_flags(C.cloud_data(c.name)), True))
    for c in C.VOXEL:
        out.append(("voxel", c.name, C.T_CLOUD, 1, [C.head_flags(C.voxel_sorted_keys(c.name)).astype(np.int64)], True))
    for c in C.MESH:
        out.append(("mesh", c.name, C.T_MESH, 2, [C.quad_flags(v["valid"]) for v in C.mesh_data(c.name)], True))
    for c in C.DEPTH:
        out.append(("depth", c.name, C.T_DEPTH, 1, [s["keep"].astype(np.int64) for s in C.depth_data(c.name)], True))
    for c in C.RECON:
        m = C.recon_masks(c.name)
        out.append(("recon", c.name, C.T_RECON, 2, [m[i * c.L:(i + 1) * c.L] for i in range(c.B)], False))
    for c in C.MATCH:
        out.append(("match", c.name, C.T_MATCH, 1, [ok.astype(np.int64) for ok, _ in C.match_flags(C.match_data(c.name))], True))
    return out


FAMILY = family_flags()
SMALL = [f for f in FAMILY if sum(len(x) for x in f[4]) < 20000]


def test_case_counts_and_names():
    counts = {fam: sum(1 for f in FAMILY if f[0] == fam) for fam in ("scene", "cloud", "voxel", "mesh", "depth", "recon", "match")}
    print("COMPACT-MEASURE cases per family:", counts, "total", len(FAMILY))
    assert counts == dict(scene=68, cloud=89, voxel=60, mesh=112, depth=62, recon=61, match=60)
    for cases in (C.SCENE, C.CLOUD, C.VOXEL, C.MESH, C.DEPTH, C.RECON, C.MATCH):
        names = [c.name for c in cases]
        assert len(names) == len(set(names)) and any(c.twice for c in cases)


def test_the_builders_keep_what_their_pattern_says():
    for c in C.SCENE:
        if not c.extra:
            assert all(np.array_equal(f.astype(bool), k) for f, k in zip(C.scene_flags(C.scene_data(c.name)), C.case_flags(c, C.T_COLLECT))), c.name
    short = C.scene_data(f"num-short@{C.T_COLLECT - 1}")[0]
    assert len(short["mask"]) == short["num"] + C.SCENE_SHORT_TAIL and (short["mask"][short["num"]:] > 0).all()   # past num: all "keep"
    for c in C.CLOUD:
        d = C.cloud_data(c.name)
        if not c.extra or c.extra == "mask-carrier":
            assert all(np.array_equal(f.astype(bool), k) for f, k in zip(C.cloud_flags(d), C.case_flags(c, C.T_CLOUD))), c.name
        for v in d["views"]:
            if v["conf"] is not None and d["thresholds"] and c.extra != "nan-conf":
                with np.errstate(invalid="ignore"):
                    dropped = ~(v["conf"] > np.float32(v["thr"]))
                assert np.array_equal(v["conf"] == np.float32(v["thr"]), dropped & (np.arange(v["n"]) % 2 == 0)), c.name   # every other dropped pixel EXACTLY on the threshold
    assert sum((C.cloud_data(c.name)["views"][0]["conf"] == np.float32(1.5)).any() for c in C.CLOUD if C.cloud_data(c.name)["views"][0]["conf"] is not None) > 40
    assert np.isnan(C.cloud_data(f"nan-conf@{C.T_CLOUD - 1}")["views"][0]["conf"]).any()
    for c in C.DEPTH:
        for s in C.depth_data(c.name):
            import depth_ref
            assert np.array_equal(depth_ref.valid_pixels(s["g"], s["p"], s["conf"], s["mask"]), s["keep"]), c.name
            kc = depth_ref.fkey(s["conf"][s["keep"]])
            assert len(set(kc.tolist())) == len(kc), c.name                                       # distinct confidences: the order is unique
    for c in C.MATCH:
        flags = C.match_flags(C.match_data(c.name))
        assert np.array_equal(flags[1][0], C.pattern(c.pat, c.n, C.T_MATCH)) and not flags[0][0].size and not flags[2][0].any(), c.name
        assert flags[3][0].sum() == flags[1][0].sum()                                             # the mirrored pair finds the same matches


def test_depth_orders_are_unique():
    import depth_ref
    for c in C.DEPTH:
        for s, ref in zip(C.depth_data(c.name), C.depth_ref_of(c.name)):
            if ref["n_valid"] < 2:
                continue
            g, p = s["g"][s["keep"]].astype(np.float64), s["p"][s["keep"]].astype(np.float64)
            e = (np.abs(ref["scale"] * p - g) / g).astype(np.float32)
            assert len(set(depth_ref.fkey(e).tolist())) == len(e), c.name


def test_depth_segment_counts_give_four_to_six_sort_passes():
    assert [C.depth_passes(n) for n in C.DEPTH_SEGS] == [4, 5, 5, 6]
    by_segs = {len(c.lens) for c in C.DEPTH}
    assert set(C.DEPTH_SEGS) <= by_segs
    few = C.by_name(C.DEPTH, "segs-257-twice")
    assert C.depth_passes(len(few.lens)) == 6 and set(few.lens) == {1, 2, 3}
    for name in ("segs-257-twice", "segs-256", "empty-between"):
        n = [r["n_valid"] for r in C.depth_ref_of(name)]
        assert any(n[i] == 0 and n[i - 1] > 0 and n[i + 1] > 0 for i in range(1, len(n) - 1)), name   # no valid pixel between two valid segments


def test_voxel_cases_place_their_heads():
    T = C.T_CLOUD
    at, across = C.voxel_sorted_keys("head-at-T"), C.voxel_sorted_keys("run-across-T")
    assert at[T] != at[T - 1] and across[T] == across[T - 1] and across[T - 1] != across[0]
    assert len(set(C.voxel_sorted_keys(f"none@{T}").tolist())) == 1                               # one voxel
    assert len(set(C.voxel_sorted_keys(f"all@{T}").tolist())) == T                                # every point its own voxel
    for c in C.VOXEL:
        assert np.array_equal(C.head_flags(C.voxel_sorted_keys(c.name)), C.voxel_heads(c)), c.name
        p, col, counts = C.voxel_ref(c.name)
        assert len(p) == C.voxel_heads(c).sum() == len(counts) and counts.sum() == c.lens[0]


def test_mesh_cases_keep_only_a_only_b_and_both():
    seen = set()
    for c in C.MESH:
        for (H, W, pat, kind), v in zip(c.views, C.mesh_data(c.name)):
            q = C.quad_flags(v["valid"])
            seen |= set(q.tolist())
            if kind == "quads":
                assert np.array_equal(q != 0, C.pattern(pat, H - 1, C.T_MESH)), c.name            # the construction keeps exactly the pattern's quads
    assert seen == {0, 1, 2, 3}
    lone = C.quad_flags(C.mesh_data(f"quads-lane63@{2 * C.T_MESH + 17}")[0]["valid"])
    assert {1, 2, 3} <= set(lone.tolist())                                                        # lone keepers take the three kinds in turn
    assert {(H - 1) * (W - 1) for c in C.MESH for H, W, _, _ in c.views} >= set(C.lengths(C.T_MESH))
    flat = [v for v in C.by_name(C.MESH, "row-and-column").views[:2]]
    assert [(H - 1) * (W - 1) for H, W, _, _ in flat] == [0, 0] and C.mesh_tiles(C.mesh_data("row-and-column"))[1].tolist() == [0, 1, 2, 3]
    assert {c.cfg for c in C.MESH} == set(C.MESH_CFG) and {c.carrier for c in C.MESH} == {"conf", "mask"}


def test_recon_cases_carry_the_passenger_and_split_the_streams():
    c = C.by_name(C.RECON, "views-3")
    assert all(b % 64 for b in c.bounds[1:-1])                                                    # view boundaries inside a step
    m = C.recon_masks("views-3")
    assert ((m & 3) == 0).any() and ((m & 7) == 4).any() and ((m & 3) == 2).any() and ((m & 3) == 3).any()   # passenger alone; valid but below thr; both
    none = C.recon_masks(f"none@{C.T_RECON - 1}")
    assert (none & 3).max() == 0 and (none & 4).any()                                             # ICP weight set on invalid pixels only
    two = C.by_name(C.RECON, "two-samples-twice")
    assert two.B == 2 and C.recon_data(two.name)["seg"].tolist() == [0, 333, two.L, two.L + 333, 2 * two.L]
    import recon_ref
    import torch
    d = C.recon_data("views-3")
    k0 = (m & 1) == 1
    x, y, w = torch.from_numpy(d["pred"][k0]), torch.from_numpy(d["gt"][k0]), torch.from_numpy(((m & 4) == 4)[k0])
    R, t, s = recon_ref.rigid_points_registration(x.double(), y.double(), w, compute_scaling=True)
    R2, t2, s2 = C.umeyama(x, y, w, torch.float64)
    assert torch.equal(R, R2) and torch.equal(t, t2) and torch.equal(s, s2)                       # umeyama IS the reference, in float64
    for c in C.RECON:                                                                             # the float32 run stays near it: d is a rounding figure
        _, _, r64, p64 = C.recon_ref_of(c.name)
        _, _, r32, p32 = C.recon_ref_of(c.name, torch.float32)
        assert C.rel_err(r32, r64) < 1e-3, c.name


# ================================================================================================ the restatement against a boolean index
@pytest.mark.parametrize("family", ["scene", "cloud", "voxel", "mesh", "depth", "recon", "match"])
def test_restated_walk_is_a_boolean_index(family):
    for fam, name, T, K, flags, zeroed in SMALL:
        if fam == family:
            assert C.walk_agrees(flags, T, K, zeroed_last=zeroed), (fam, name)


def test_restated_walk_on_the_scan_cases():
    for fam, name, T, K, flags, zeroed in FAMILY:
        if name == "scan-1025":
            assert C.walk_agrees(flags, T, K, zeroed_last=zeroed) and C.walk_agrees(flags, T, K, zeroed_last=True), name
        if name == "scan-2049":                # the count and the scan only: the walk of 2.1 M entries in Python is the GPU module's to check
            scan = C.tile_scan(flags, T)
            assert scan[-1] == sum(int(f.sum()) for f in flags) and len(scan) == 2050


def flags_of(family, name):
    return next(f for f in FAMILY if f[0] == family and f[1] == name)


# which named case catches which wrong restatement (each listed case must; the first is the one recorded in docs/kernels.md)
CATCHES = {
    "stop": [("scene", "half@1"), ("scene", "last@1023"), ("scene", "three-ragged-twice"), ("recon", "lane63@2047")],
    "rank_own": [("scene", "first@1023"), ("scene", "last@1024"), ("mesh", "quads-last@1")],
    "inclusive_scan": [("scene", "last@1"), ("cloud", "hole@2065"), ("scene", "scan-1025")],
    "stream1_advances_0": [("mesh", "pixels-half@2065-twice"), ("mesh", "quads-lane63@2065"), ("recon", "half@4113-twice")],
    "seg_lt": [("scene", "three-ragged-twice"), ("cloud", "three-ragged-twice"), ("depth", "three-ragged-twice"), ("mesh", "three-ragged-quads")],
    "passenger": [("recon", "none@2047"), ("recon", "views-3")],
}


@pytest.mark.parametrize("wrong", sorted(CATCHES))
def test_wrong_restatements_are_caught(wrong):
    for family, name in CATCHES[wrong]:
        _, _, T, K, flags, zeroed = flags_of(family, name)
        assert C.walk_agrees(flags, T, K, zeroed_last=zeroed), (family, name)
        caught = not C.walk_agrees(flags, T, K, wrong=wrong, zeroed_last=zeroed)
        print(f"COMPACT-MEASURE wrong restatement {wrong}: {family} {name} {'catches it' if caught else 'MISSES it'}")
        assert caught, (wrong, family, name)


def test_is_head_without_the_first_position_clause_is_caught():
    """Without `i == 0` position 0 compares with whatever lies in front of the keys.  Where that equals keys[0] the first voxel is lost: one
    voxel (none@T) then has no head at all.  On the GPU the word in front is workspace or sentinel, which the rule 'exactly sized, 0xFF-filled'
    makes differ from every key of at most 63 bits: there the defect would show only as the out-of-bounds read it is."""
    for name in (f"none@{C.T_CLOUD}", "head-at-T", f"first@{C.T_CLOUD - 1}"):
        keys = C.voxel_sorted_keys(name)
        right = C.head_flags(keys)
        wrong = C.head_flags(keys, i0_clause=False, before=keys[0])
        print(f"COMPACT-MEASURE wrong restatement is_head-without-i0: voxel {name}: {int(right.sum())} heads become {int(wrong.sum())}")
        assert right[0] and not wrong[0] and wrong.sum() == right.sum() - 1
        assert C.walk_agrees([right.astype(np.int64)], C.T_CLOUD) and not np.array_equal(C.walk_ref([wrong.astype(np.int64)])[0], C.walk_ref([right.astype(np.int64)])[0])


def test_an_unzeroed_last_word_cannot_be_caught_by_value():
    """The finding of this module about the 'n_tiles + 1 words, last one zeroed' convention: under an EXCLUSIVE scan the last output is the sum of
    the words before it, whatever the last input holds, so no case can tell a count kernel that forgets the zero from one that writes it -- the
    zero matters only together with an inclusive scan, which `inclusive_scan` above catches.  What guards the word on the GPU is placement: it is
    0xFF before every run, and every family's total (the scan's last word) is compared with the reference."""
    for family, name in (("cloud", "half@2065-twice"), ("cloud", "three-ragged-twice"), ("mesh", "pixels-half@2065-twice"), ("depth", "hole@2065")):
        _, _, T, K, flags, zeroed = flags_of(family, name)
        assert zeroed and C.walk_agrees(flags, T, K, wrong="last_not_zeroed")
        right, wrong = C.walk(flags, T, K)[0], C.walk(flags, T, K, wrong="last_not_zeroed")[0]
        assert np.array_equal(right, wrong)
    assert set(C.WRONG) == set(CATCHES) | {"last_not_zeroed"}
