"""Reconstruction metrics, CPU side: the restatement in tests/recon_ref.py against the live reference, the fixture generator, the normal
restatement on analytic surfaces, and the argument checks of the new C entry points (no kernel is launched here)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import recon_ref  # noqa: E402
from oracle import ref_loader  # noqa: E402

needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout")


def bits(x):
    return np.asarray(x).tobytes()


@needs_reference
def test_restated_metrics_equal_reference_bit_for_bit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_golden_recon as mg
    rm, _ = mg.load_reference()
    for name, case in mg.METRIC_CASES.items():
        gt, rec, ngt, nrec, th = mg.metric_inputs(case)
        for ours, theirs in ((recon_ref.accuracy(gt, rec, ngt, nrec), rm.accuracy(gt, rec, ngt, nrec)),
                             (recon_ref.completion(gt, rec, ngt, nrec), rm.completion(gt, rec, ngt, nrec)),
                             (recon_ref.accuracy(gt, rec), rm.accuracy(gt, rec))):
            assert [bits(v) for v in ours] == [bits(v) for v in theirs], name
            assert [type(v) for v in ours] == [type(v) for v in theirs], name
        a, b = recon_ref.completion_ratio(gt, rec, th), rm.completion_ratio(gt, rec, th)
        assert bits(a) == bits(b) and type(a) is type(b) is np.float32, name


@needs_reference
def test_golden_generator_reproduces_fixture():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_recon.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def _plane(n, seed):
    g = np.random.default_rng(seed)
    u, v = g.uniform(-1, 1, n), g.uniform(-1, 1, n)
    a = np.array([1.0, 0.5, -0.3])
    a /= np.linalg.norm(a)
    e1 = np.cross(a, [0.0, 0.0, 1.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    p = 0.3 * a + u[:, None] * e1 + v[:, None] * e2
    return p, np.tile(a, (n, 1))


def _sphere(n, seed, r=2.0):
    # a Fibonacci lattice with a small tangential jitter: neighbourhoods are nearly symmetric, so the fitted plane is radial
    i = np.arange(n) + 0.5
    phi = np.arccos(1 - 2 * i / n)
    th = np.pi * (1 + 5 ** 0.5) * i
    d = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1)
    g = np.random.default_rng(seed)
    d = d + 1e-3 * g.standard_normal(d.shape) / np.sqrt(n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return r * d, d


@pytest.mark.parametrize("surface", ["plane", "sphere"])
def test_normal_restatement_recovers_analytic_normals(surface):
    p, n_true = _plane(5000, 1) if surface == "plane" else _sphere(1000000, 2)
    n = recon_ref.estimate_normals(p, 30)
    dot = np.abs(np.sum(n * n_true, axis=1))
    assert dot.min() >= 1 - 1e-6, (surface, dot.min())


def test_knn_restatement_orders_ties_by_index():
    p = np.repeat(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]), 4, axis=0)  # four copies of each point
    idx, d = recon_ref.knn_sorted(p, 6)
    assert idx[0].tolist() == [0, 1, 2, 3, 4, 5] and idx[5].tolist() == [4, 5, 6, 7, 0, 1]
    assert d[0].tolist() == [0, 0, 0, 0, 1, 1]


def test_recon_entry_points_reject_bad_arguments(built_lib):
    from fast3r_amd import _lib
    l = built_lib
    assert l.f3r_version() >= 360 and _lib.ABI_VERSION >= 360
    assert l.f3r_nn_index_bytes(1000) > 16 * 1000 and l.f3r_nn_index_bytes(-1) == 0 and l.f3r_nn_workspace_bytes(-5) == 0
    F = 0x10000  # a fake, aligned device address: every call below must fail its argument checks before touching it
    nb, wb = l.f3r_nn_index_bytes(100), l.f3r_nn_workspace_bytes(100)
    assert l.f3r_nn_build(None, 100, F, nb, F, wb, None) == -1 and b"null" in l.f3r_last_error_string()
    assert l.f3r_nn_build(F, -1, F, nb, F, wb, None) == -1
    assert l.f3r_nn_build(F, 100, F, nb - 1, F, wb, None) == -1 and b"index too small" in l.f3r_last_error_string()
    assert l.f3r_nn_build(F, 100, F, nb, F, wb - 1, None) == -1 and b"workspace" in l.f3r_last_error_string()
    assert l.f3r_nn_build(F, 100, F + 8, nb, F, wb, None) == -1 and b"misaligned" in l.f3r_last_error_string()
    assert l.f3r_nn_query(F, F, -3, F, F, F, wb, None) == -1
    assert l.f3r_nn_query(F, None, 100, F, F, F, wb, None) == -1 and b"null" in l.f3r_last_error_string()
    assert l.f3r_nn_query(F, F, 100, F, F, F, wb - 1, None) == -1 and b"workspace" in l.f3r_last_error_string()
    for k in (0, 65, -1):
        assert l.f3r_estimate_normals(F, F, k, F, None, None, None) == -1 and b"outside 1..64" in l.f3r_last_error_string()
    assert l.f3r_estimate_normals(F, F, 30, None, None, None, None) == -1 and b"no output" in l.f3r_last_error_string()
    sb = l.f3r_recon_stats_workspace_bytes(100)
    assert l.f3r_recon_stats(F, F, F, None, 100, 100, 0.0, F, F, sb, None) == -1 and b"normals" in l.f3r_last_error_string()
    assert l.f3r_recon_stats(F, F, None, None, -1, 0, 0.0, F, F, sb, None) == -1
    assert l.f3r_recon_stats(F, F, None, None, 100, 0, 0.0, F, F, sb - 1, None) == -1 and b"workspace" in l.f3r_last_error_string()
    assert l.f3r_recon_stats(None, None, None, None, 100, 0, 0.0, F, F, sb, None) == -1
    pb = l.f3r_recon_prepare_workspace_bytes(2, 3, 1000)
    assert pb > 0 and l.f3r_recon_prepare_workspace_bytes(0, 3, 1000) == 0
    args = [F, F, F, F, F, 2, 3, 1000, 0.5, 0.5, F, F, F, F, F, pb, None]
    assert l.f3r_recon_prepare(*args[:3], None, *args[4:]) == -1 and b"null" in l.f3r_last_error_string()
    assert l.f3r_recon_prepare(*args[:8], ctypes.c_float(1.5), *args[9:]) == -1 and b"quantile" in l.f3r_last_error_string()
    assert l.f3r_recon_prepare(*args[:5], 0, *args[6:]) == -1 and b"bad sizes" in l.f3r_last_error_string()
    assert l.f3r_recon_prepare(*args[:15], pb - 1, None) == -1 and b"workspace" in l.f3r_last_error_string()
