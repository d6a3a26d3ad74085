"""The tile-compaction kernels at the edges of their walk, on a real MI355X through the C ABI (cases, references and what each case is there
for: tests/compact_cases.py; that they reach it and that a wrong walk misses: tests/test_compact_cases.py).

The cases module owns every buffer: predicate operands in arenas of 0x7F bytes (an element read past the end is kept and changes a count), data
operands in arenas of 0xFF bytes, every output -- scan arrays and count words included -- exactly as long as the count states between sentinels,
workspaces of exactly f3r_*_workspace_bytes, 0xFF-filled before every run.  After each launch: synchronise, sentinels, arenas, then values:
gathers and integer outputs bit for bit.  A case named *-twice runs again on re-poisoned buffers and must give the same bits.

Measured on an MI355X: all 512 cases pass (scene 68, cloud 89, voxel 60, mesh 112, depth 62, recon 61, match 60) in under 4 s; no defect found.
f3r_recon_prepare against the float64 reference, bound max(4 d, 2^-20): worst err 5.8e-8 for rts (alternate@2048, d 1.1e-7) and 2.2e-7 for
pred_out (half@63, d 9.5e-7), at most 0.14 of the bound; docs/rows_f.md has err and d of every case.
"""
import numpy as np
import pytest

import compact_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_runs(case, got, want, names):
    for r, run in enumerate(got):
        assert len(run) == len(want)
        for what, g, w in zip(names, run, want):
            if w is None:
                assert g is None, (case.name, what)
                continue
            assert same_bits(g, np.asarray(w)), f"{case.name} run {r}: {what} differs from the reference"
    if case.twice:
        assert len(got) == 2 and all(same_bits(a, b) for a, b in zip(got[0], got[1]) if a is not None), f"{case.name}: two runs differ"


@pytest.mark.parametrize("name", [c.name for c in C.SCENE])
def test_scene_collect(built_lib, name):
    c = C.by_name(C.SCENE, name)
    got = C.run_scene(built_lib, DEV, name, runs=2 if c.twice else 1)
    check_runs(c, got, C.scene_ref(name), ("scan", "points", "colours"))


@pytest.mark.parametrize("name", [c.name for c in C.CLOUD])
def test_cloud_combine(built_lib, name):
    c = C.by_name(C.CLOUD, name)
    got = C.run_cloud(built_lib, DEV, name, runs=2 if c.twice else 1)
    check_runs(c, got, C.cloud_ref_of(name), ("scan", "points", "colours"))


@pytest.mark.parametrize("name", [c.name for c in C.VOXEL])
def test_voxel_heads(built_lib, name):
    c = C.by_name(C.VOXEL, name)
    got = C.run_voxel(built_lib, DEV, name, runs=2 if c.twice else 1)
    p, col, counts = C.voxel_ref(name)
    check_runs(c, got, (np.int64(len(p)), p, col, counts), ("n_voxels", "points", "colours", "counts"))


@pytest.mark.parametrize("name", [c.name for c in C.MESH])
def test_mesh(built_lib, name):
    c = C.by_name(C.MESH, name)
    got = C.run_mesh(built_lib, DEV, name, runs=2 if c.twice else 1)
    counts, vertices, faces, colours = C.mesh_ref_of(name)
    check_runs(c, got, (counts, vertices, faces.astype(np.int64 if c.cfg[2] else np.int32), colours), ("counts", "vertices", "faces", "face colours"))


def bits64(x):
    return np.float64(x).tobytes()


@pytest.mark.parametrize("name", [c.name for c in C.DEPTH])
def test_depth_sparsify(built_lib, name):
    """n_valid, the medians, the scale, starts and both orders bit for bit; the curves and their area within depth_ref's tolerances"""
    import depth_ref as R
    c = C.by_name(C.DEPTH, name)
    got = C.run_depth(built_lib, DEV, name, runs=2 if c.twice else 1)
    K = C.DEPTH_BINS
    for r, (out, oc, oe, starts) in enumerate(got):
        for i, ref in enumerate(C.depth_ref_of(name)):
            row, n, w = out[i], ref["n_valid"], f"{name} run {r} segment {i}"
            assert row[0] == n and int(starts[i + 1]) - int(starts[i]) == n, w
            assert np.isnan(row[1]), w
            for col, key in ((2, "median_gt"), (3, "median_pred"), (4, "scale")):
                assert bits64(row[col]) == bits64(ref[key]) or (np.isnan(row[col]) and np.isnan(ref[key])), (w, key, row[col], ref[key])
            s_k, o_k = row[16:16 + K], row[16 + K:16 + 2 * K]
            if n == 0:
                assert np.isnan(row[15]) and np.isnan(s_k).all() and np.isnan(o_k).all(), w
                continue
            assert oc[starts[i]:starts[i + 1]].tolist() == ref["order_conf"].tolist(), w
            assert oe[starts[i]:starts[i + 1]].tolist() == ref["order_err"].tolist(), w
            for k in range(K):
                assert abs(s_k[k] - ref["s"][k]) <= R.tolerance(n, ref["s"][k]), (w, "s", k, s_k[k], ref["s"][k])
                assert abs(o_k[k] - ref["o"][k]) <= R.tolerance(n, ref["o"][k]), (w, "o", k, o_k[k], ref["o"][k])
            assert abs(row[15] - ref["ause"]) <= R.ause_tolerance(n, ref["s"]), (w, "ause", row[15], ref["ause"])
    if c.twice:                                # columns 5 .. 14 belong to f3r_depth_errors, which is not called: they hold the sentinel in both runs
        assert len(got) == 2 and all(same_bits(a, b) for a, b in zip(got[0], got[1])), f"{name}: two runs differ"


@pytest.mark.parametrize("name", [c.name for c in C.RECON])
def test_recon_prepare(built_lib, name):
    """counts and gt_out exact; rts and pred_out within max(4 d, 2^-20) of the float64 reference, d = the float32 run of that reference"""
    import torch
    c = C.by_name(C.RECON, name)
    got = C.run_recon(built_lib, DEV, name, runs=2 if c.twice else 1)
    counts, gts, rts64, pred64 = C.recon_ref_of(name)
    _, _, rts32, pred32 = C.recon_ref_of(name, torch.float32)
    for r, (cn, g, rts, pred) in enumerate(got):
        assert same_bits(cn, counts), (name, r, cn.tolist(), counts.tolist())
        assert all(same_bits(a, b) for a, b in zip(g, gts)), f"{name} run {r}: gt_out differs"
        assert [len(p) for p in pred] == [len(p) for p in pred64]
        rows = {"rts": (C.rel_err(rts, rts64), C.rel_err(rts32, rts64)),
                "pred_out": (C.rel_err(np.concatenate(pred), np.concatenate(pred64)), C.rel_err(np.concatenate(pred32), np.concatenate(pred64)))}
        print(f"COMPACT-MEASURE recon {name} run {r}: " + ", ".join(f"{k} err {e:.2e} d {d:.2e}" for k, (e, d) in rows.items()))
        for k, (e, d) in rows.items():
            assert e <= max(4 * d, C.RECON_FLOOR), (name, r, k, e, d)
    if c.twice:
        a, b = got
        assert same_bits(a[0], b[0]) and same_bits(a[2], b[2]) and all(same_bits(x, y) for x, y in zip(a[1] + a[3], b[1] + b[3])), f"{name}: two runs differ"


@pytest.mark.parametrize("name", [c.name for c in C.MATCH])
def test_match_write(built_lib, name):
    c = C.by_name(C.MATCH, name)
    got = C.run_match(built_lib, DEV, name, runs=2 if c.twice else 1)
    check_runs(c, got, C.match_ref_of(name), ("tile counts", "offsets", "xy_i", "xy_j", "dist"))
