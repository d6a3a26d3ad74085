"""No GPU: the cases of tests/post_cases.py do what tests/test_post_geometry_gpu.py relies on.  Per family a restatement of the kernel's arithmetic
meets the tolerance the GPU module asserts against the same reference, and a deliberately wrong variant misses a listed case; the cases reach the
branches they are named for; the product's similarity solve (csrc/f3r_linalg.h), built for the host, meets the orthonormality and Horn bounds
on every degenerate cloud; oracle/pnp_oracle.py agrees with the reference's route (oracle/cv2_stub.py) at 4 and 5 points."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import post_cases as pc
from oracle import align_oracle, pnp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ================================================================================================ quantile threshold
def quantile_restate(rows, q, nearest=False):
    """block_quantile in float32: rank = q (n - 1), the two order statistics (a sort stands in for the radix select), at::lerp with its
    multiply-add fused, as the compilers of both the kernel and ATen contract it (the product is exact in float64, which rounds once more).
    nearest: the order statistic nearest to the rank, without interpolation (what the kernel must NOT do)"""
    n = rows.shape[1]
    q = torch.tensor(pc.f32(q), dtype=torch.float32)
    rank = q * torch.tensor(float(n - 1), dtype=torch.float32)
    srt = rows.sort(dim=1).values
    if nearest:
        return srt[:, int(torch.round(rank))]
    lo, hi = srt[:, int(torch.floor(rank))], srt[:, int(torch.ceil(rank))]
    w, d = rank - torch.floor(rank), hi - lo
    fused = lo.double() + w.double() * d.double() if float(w) < 0.5 else hi.double() - d.double() * (1.0 - w).double()
    return fused.float()


def test_quantile_restatement_is_bit_equal_and_nearest_misses():
    missed = 0
    for n in pc.Q_NPIX:
        for q in pc.quantile_qs(n):
            rows = pc.quantile_rows(n, q)
            ref = pc.quantile_ref(rows, q)
            assert pc.same_f32(quantile_restate(rows, q), ref), (n, q)
            missed += not pc.same_f32(quantile_restate(rows, q, nearest=True), ref)
    assert missed > 0
    # the integer-rank q is one: the interpolation weight is exactly 0 there
    assert 0.25 in pc.quantile_qs(65) and (0.25 * 64) == 16


def test_quantile_rows_are_what_they_are_named_for():
    for n in (65, 1025):
        bits = {k: pc.quantile_row(k, n).view(torch.int32) for k in ("low10", "mid11", "top11")}
        assert len(set((bits["low10"] >> 10).tolist())) == 1 and len(set(bits["low10"].tolist())) > 10
        assert len(set((bits["mid11"] & 0x3FF).tolist())) == 1 and len(set((bits["mid11"] >> 21).tolist())) == 1 and len(set(bits["mid11"].tolist())) > 10
        assert len(set((bits["top11"] & 0x1FFFFF).tolist())) == 1 and len(set(bits["top11"].tolist())) > 10
        assert torch.isfinite(pc.quantile_row("top11", n)).all()
    z = pc.quantile_row("zeros", 65)
    assert bool(((z == 0) & torch.signbit(z)).any()) and bool(((z == 0) & ~torch.signbit(z)).any())
    sub = pc.quantile_row("subnormal", 65)
    assert bool((sub > 0).all()) and float(sub.max()) < 2.0 ** -126
    assert bool(torch.isinf(pc.quantile_row("inf", 65)).any()) and bool((pc.quantile_row("negative", 65) < 0).any())
    t = pc.quantile_row("ties100", 1025, 0.85)
    v, cnt = t.unique(return_counts=True)
    k = int(cnt.argmax())
    assert int(cnt[k]) == 100 and float(v[k]) == float(pc.quantile_ref(t[None], 0.85)[0])      # the run of ties holds the cut


# ================================================================================================ alignment
def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


@pytest.mark.parametrize("c", pc.ALIGN_SHAPES + pc.ALIGN_FALLBACKS, ids=lambda c: c.id)
def test_align_restatement_follows_the_oracle(c):
    d = pc.build_align(c)
    ref = pc.align_ref(d, c.q)
    assert _rel(pc.align_restate(d, c.q), ref) <= 1e-9, c.id
    paths = [pc.align_path(d["conf"][p], None if d["valid"] is None else d["valid"][p], c.q) for p in range(c.n_prob)]
    if c.path:
        assert paths == [c.path], (c.id, paths)
    if c.npix < 3:
        assert paths == ["I"] * c.n_prob and torch.equal(ref, d["loc"].double())


def test_align_cases_reach_every_route():
    seen = set()
    for c in pc.ALIGN_SHAPES:
        d = pc.build_align(c)
        seen |= {pc.align_path(d["conf"][p], None if d["valid"] is None else d["valid"][p], c.q) for p in range(c.n_prob)}
    assert seen == {"A", "B", "I"}


def test_align_wrong_variants_miss():
    by = {c.id: c for c in pc.ALIGN_FALLBACKS}
    c = by["tie-at-threshold"]
    d = pc.build_align(c)
    assert float(torch.quantile(d["conf"][0], 0.5)) == 2.0 and int((d["conf"][0] == 2.0).sum()) == 10
    assert _rel(pc.align_restate(d, c.q, strict=True), pc.align_ref(d, c.q)) > pc.ALIGN_PTS_TOL          # `>` at the threshold drops the ten ties
    c = by["two-confident"]
    d = pc.build_align(c)
    assert _rel(pc.align_restate(d, c.q, skip_valid_fallback=True), pc.align_ref(d, c.q)) > pc.ALIGN_PTS_TOL   # no valid-only fall-back: identity
    x, y, m = pc.cloud("mirrored")
    assert not pc.horn_misses(*pc.umeyama_raw_moments(x[m], y[m]), x, y, m, "mirrored")
    missed = dict((k, v) for k, v, _ in pc.horn_misses(*pc.umeyama_plain(x[m], y[m]), x, y, m, "mirrored"))
    assert "det" in missed and "R" in missed                                                              # Umeyama without the determinant correction


@pytest.mark.parametrize("kind", pc.ALIGN_CLOUDS)
def test_float64_raw_moment_restatement_meets_the_horn_bounds(kind):
    """the reference side of the cloud cases: Umeyama on RAW float64 moments with LAPACK's SVD, results rounded to fp32 like rts"""
    x, y, m = pc.cloud(kind)
    assert int(m.sum()) == pc.CLOUD_N and x.shape[0] == pc.CLOUD_N + pc.CLOUD_OFF
    assert pc.horn_misses(*pc.umeyama_raw_moments(x[m], y[m]), x, y, m, kind) == []
    if kind.startswith(("plane", "line", "axis")):      # the masked points are degenerate, the pixels outside the mask are not
        sv = torch.linalg.svdvals(x[m].double() - x[m].double().mean(0))
        assert float(sv[2] / sv[0]) < 1e-6 and float(torch.linalg.svdvals(x.double() - x.double().mean(0))[2]) > 1.0
        if kind.startswith("line"):
            assert float(sv[1] / sv[0]) < 1e-6


def test_far_offset_is_the_largest_that_meets_the_bounds():
    ok = []
    for off in pc.FAR_OFFSETS:
        x, y, m = pc.cloud("far", off)
        assert float(x.abs().max()) > 0.5 * off
        if not pc.horn_misses(*pc.umeyama_raw_moments(x[m], y[m]), x, y, m, "far"):
            ok.append(off)
    assert max(ok) == pc.FAR_OFFSET


@pytest.fixture(scope="module")
def host_similarity(tmp_path_factory):
    """the product's svd3 + similarity_from_moments (fast3r_amd/csrc/f3r_linalg.h) compiled for the host by tests/csrc/linalg_host.cpp"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    so = str(tmp_path_factory.mktemp("linalg") / "liblinalg_host.so")
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "csrc", "linalg_host.cpp")], check=True)
    lib = ctypes.CDLL(so)
    fp = ctypes.POINTER(ctypes.c_float)

    def solve(x, y):
        x, y = np.ascontiguousarray(x.numpy(), np.float32), np.ascontiguousarray(y.numpy(), np.float32)
        o = np.zeros(13, np.float32)
        lib.linalg_host_similarity(x.ctypes.data_as(fp), y.ctypes.data_as(fp), len(x), o.ctypes.data_as(fp))
        o = torch.from_numpy(o)
        return o[:9].view(3, 3), o[9:12], o[12]
    return solve


@pytest.mark.parametrize("kind", pc.ALIGN_CLOUDS)
def test_product_similarity_solve_on_the_host(host_similarity, kind):
    """every bound the GPU module asserts, on the product's own header: R orthonormal with det +1 on tilted planes and lines (the parent commit's
    svd3 returned |R^T R - I| up to 1.0 there: docs/parity.md), R / s / t and all pixels -- the off-plane ones included -- within the Horn bounds
    where the rotation is determined"""
    for seed in (None, 1, 2, 3):
        x, y, m = pc.cloud(kind, seed=seed)
        R, t, s = host_similarity(x[m], y[m])
        misses = pc.horn_misses(R, t, s, x, y, m, kind)
        print(f"[post-cases] host similarity {kind} seed={seed} ortho={pc.ortho_err(R):.2e} misses={misses}")
        assert misses == [], (kind, seed, misses)


def test_product_similarity_solve_on_identical_points(host_similarity):
    """sum |x - xm|^2 == 0: the oracle's scale is 0 / 0; the product must agree on what is NaN"""
    x, y = torch.full((16, 3), 0.75), torch.full((16, 3), -1.5)
    Ro, to, so = align_oracle.rigid_points_registration(x.double(), y.double())
    R, t, s = host_similarity(x, y)
    assert bool(torch.isnan(so)) == bool(torch.isnan(s)) and torch.equal(torch.isnan(to), torch.isnan(t))
    assert torch.equal(torch.isnan(Ro), torch.isnan(R)) and pc.ortho_err(R) <= pc.ORTHO_TOL


# ================================================================================================ focal
def focal_restate64(c, d):
    """the estimator in float64 on the fp32 inputs, per-point arithmetic as focal_kernel orders it"""
    H, W = c.H, c.W
    thr = torch.quantile(d["conf"].reshape(-1), pc.f32(c.q))
    m = (d["conf"] >= thr).reshape(-1)
    if not bool(m.any()):
        return c.base
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    px, py = (xs.reshape(-1) - np.float32(c.ppxy[0]))[m], (ys.reshape(-1) - np.float32(c.ppxy[1]))[m]
    p = d["pts"].reshape(-1, 3)[m]
    xz, yz = (p[:, 0] / p[:, 2]).double(), (p[:, 1] / p[:, 2]).double()      # the ratio itself is fp32 in kernel and reference alike
    xz, yz = torch.where(torch.isfinite(xz), xz, torch.zeros_like(xz)), torch.where(torch.isfinite(yz), yz, torch.zeros_like(yz))
    dpx, dxx = xz * px + yz * py, xz * xz + yz * yz
    f = dpx.mean() / dxx.mean()
    for _ in range(c.n_iter):
        w = 1.0 / ((px - f * xz) ** 2 + (py - f * yz) ** 2).sqrt().clamp_min(1e-8)
        f = (w * dpx).sum() / (w * dxx).sum()
    f = float(f)
    return f if f != f else min(max(f, c.rng[0] * c.base), c.rng[1] * c.base)


@pytest.mark.parametrize("c", pc.FOCAL, ids=lambda c: c.id)
def test_focal_restatement_follows_the_oracle(c):
    d = pc.build_focal(c)
    ref, thr = pc.focal_ref(c, d)
    got = focal_restate64(c, d)
    if c.kind == "z0-all":
        assert ref != ref and got != got                                     # 0 / 0, kept by clip
    elif c.kind == "nan-thr":
        assert bool(torch.isnan(thr)) and ref == pytest.approx(c.base, rel=1e-6) and got == c.base
    else:
        assert abs(got - ref) <= pc.FOCAL_TOL * abs(ref), (c.id, got, ref)
        if c.id.endswith("clamp-lo"):
            assert ref == pytest.approx(c.rng[0] * c.base, rel=1e-6)
        if c.id.endswith("clamp-hi"):
            assert ref == pytest.approx(c.rng[1] * c.base, rel=1e-6)
        if c.id.endswith(("bounded", "it10")) and min(c.H, c.W) > 1:
            assert c.rng[0] * c.base < ref < c.rng[1] * c.base and abs(ref - c.frac * c.base) < 0.05 * ref     # the estimator does its job
    if c.q == 1.0 and c.kind == "scene":
        assert int((d["conf"] >= thr).sum()) == 1


def test_focal_without_nan_to_num_misses():
    for cid in ("5x7-z0-some", "31x33-z0-some"):
        c = next(c for c in pc.FOCAL if c.id == cid)
        d = pc.build_focal(c)
        ref, thr = pc.focal_ref(c, d)
        kept = (d["conf"] >= thr) & (d["pts"][..., 2] == 0)
        assert int(kept.sum()) >= 3 and ref == ref
        bad, _ = pc.focal_ref(c, d, nan_to_num=False)
        assert not abs(bad - ref) <= pc.FOCAL_TOL * abs(ref)


# ================================================================================================ PnP
@pytest.mark.parametrize("c", pc.PNP, ids=lambda c: c.id)
def test_pnp_oracle_on_the_cases(c):
    d = pc.build_pnp(c)
    n = int(d["mask"].sum())
    assert n == (c.H * c.W if c.mask == "all" else 10 if c.mask == "first10" else c.W if c.mask == "last-row" else c.mask)
    assert any(abs(c.f - g) < 1e-12 for g in c.grid)                         # the scene focal is a member of the grid
    f, T, inl = pc.pnp_ref(c.id)
    if n < 4:
        assert T is None and inl == 0
        return
    assert T is not None and abs(f - c.f) <= 1e-9 * c.f, (c.id, f)
    assert inl == n - c.n_out or (c.n_out and n - c.n_out <= inl <= n - c.n_out + 25), (c.id, inl)   # a gross outlier can land within 5 px by chance
    tol = 2e-2 if c.n_out else 1e-5
    assert float((T - d["T"]).abs().max()) < tol, (c.id, float((T - d["T"]).abs().max()))
    R = T[:3, :3]
    assert pc.ortho_err(R) < pc.ORTHO_TOL and abs(float(torch.det(R)) - 1) < pc.ORTHO_TOL      # SQPnP ends at a squared step of 1e-10


@pytest.mark.parametrize("c", [c for c in pc.PNP if c.few and c.focal == "given"], ids=lambda c: c.id)
def test_pnp_oracle_agrees_with_the_reference_route_at_4_and_5_points(c):
    """with the parent commit's oracle (and kernel) these views failed or came back up to 2.9 from the camera (docs/parity.md)"""
    d = pc.build_pnp(c)
    f, T, inl = pc.pnp_ref(c.id)
    want = pc.cv2_route(c, d)
    assert want is not None and float((T - want).abs().max()) < pc.POSE_TOL
    assert float((T - pc.sqpnp_on_mask(c, d)).abs().max()) < pc.POSE_TOL and inl == c.mask


def test_a_dlt_on_4_or_5_points_is_underdetermined():
    """why the few-point views take the direct path: 8 or 10 equations leave the 12 unknowns of the calibrated DLT a null space of 4 or 2 dimensions
    -- that many eigenvalues of its reduced 4 x 4 matrix are zero up to rounding, and the 'smallest eigenvector', the pose, is an arbitrary member;
    from 6 noise-free points on exactly one is"""
    for n, null_dim in ((4, 4), (5, 2), (6, 1), (12, 1)):
        c = pc.pnp_case(f"31x33-m{n}-given")
        d = pc.build_pnp(c)
        m = d["mask"].reshape(-1)
        X = d["pts"].double().reshape(-1, 3)[m]
        ys, xs = torch.meshgrid(torch.arange(c.H, dtype=torch.float64), torch.arange(c.W, dtype=torch.float64), indexing="ij")
        P = torch.cat([(X - X.mean(0)) / (X - X.mean(0)).square().sum(1).mean().sqrt(), torch.ones(n, 1, dtype=torch.float64)], 1)
        S0, S1x, S1y, S2 = pnp_oracle._moments(P, xs.reshape(-1)[m] - c.ppxy[0], ys.reshape(-1)[m] - c.ppxy[1])
        S0i = torch.linalg.inv(S0)
        ev = torch.linalg.eigvalsh(S2 - S1x @ S0i @ S1x - S1y @ S0i @ S1y)
        scale = float(torch.linalg.eigvalsh(S2).max())
        assert int((ev.abs() < 1e-9 * scale).sum()) == null_dim, (n, ev, scale)


def test_pnp_mask_taken_with_ge_misses():
    """the pixels outside the mask hold conf == conf_thr on points that fit the camera: a mask with >= counts them"""
    for cid in ("31x33-m4-given", "31x33-thr2.5", "31x33-m3-fails"):
        assert pc.pnp_ref(cid, ge_mask=True)[2] == 31 * 33 != pc.pnp_ref(cid)[2]


def test_pnp_batches_are_made_of_listed_cases():
    ids = {c.id for c in pc.PNP}
    assert set(pc.PNP_BATCH) <= ids and set(pc.PNP_MIXED) <= ids and len(ids) == len(pc.PNP)
    assert [pc.pnp_case(i).focal for i in pc.PNP_MIXED] == ["given", "search", "given"]
    assert len({(pc.pnp_case(i).H, pc.pnp_case(i).W) for i in pc.PNP_BATCH + pc.PNP_MIXED}) == 1
