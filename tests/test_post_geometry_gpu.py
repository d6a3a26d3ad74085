"""f3r_align_local_to_global, f3r_estimate_focal and f3r_estimate_poses at the edges of their geometry, on a real MI355X through the C ABI: one to
2049 pixels around the 1024 threads of a workgroup, every quantile rank and value pattern the radix select can mishandle, every fall-back of the
alignment, planar / collinear / mirrored / far clouds, focal views with Z == 0 or no confident point, poses from 4 points up and from masks on
one image line (cases, float64 references and what each case is there for: tests/post_cases.py; that they discriminate: tests/test_post_cases.py).

The cases module owns every buffer: each operand lies inside 0xFF bytes (NaN as fp32, true as a mask byte), each output and workspace between
sentinel words.  After each launch: synchronise, guards intact, then the comparison, at the bound the project already holds that kind of output to
(thresholds bit-equal to torch.quantile, aligned points 2e-5, R / s / t 2e-6 / 2e-6 / 1e-5 against Horn, focal 5e-5, poses 1e-4; R^T R - I 1e-5);
the measured figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import post_cases as pc

pytestmark = pytest.mark.gpu
DEV = "cuda"
ID = dict(ids=lambda c: c.id)


def fig(kind, err, tol, what):
    print(f"[post-geometry] kind={kind} err={err:.3e} tol={tol:.1e} {what}")
    assert err == err and err <= tol, f"{what}: {kind} {err:.3e} > {tol:.1e}"


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ================================================================================================ quantile threshold
@pytest.mark.parametrize("n", pc.Q_NPIX)
def test_quantile_threshold(built_lib, n):
    """both thr_out outputs (align: one problem per row; focal: one 1 x n view per row) against torch.quantile, every kind of row in one launch"""
    g = pc._gen(9, n)
    pts = torch.randn(len(pc.Q_ROWS), n, 3, generator=g)
    for q in pc.quantile_qs(n):
        rows = pc.quantile_rows(n, q)
        ref = pc.quantile_ref(rows, q)
        _, _, thr_a = pc.run_align(built_lib, DEV, dict(conf=rows, loc=pts, glob=pts, valid=None), q, what=f"align n={n} q={q}")
        _, thr_f = pc.run_focal(built_lib, DEV, pts.view(-1, 1, n, 3), rows.view(-1, 1, n), q, (n / 2, 0.5), 1, (0.0, 3.0e38), what=f"focal n={n} q={q}")
        for name, thr in (("align", thr_a), ("focal", thr_f)):
            bad = [k for i, k in enumerate(pc.Q_ROWS) if not pc.same_f32(thr[i], ref[i])]
            print(f"[post-geometry] kind=quantile-{name} mismatches={len(bad)} of {len(pc.Q_ROWS)} n={n} q={q:.7g}")
            assert not bad, (name, n, q, bad, thr, ref)


# ================================================================================================ alignment
def _check_align(c, d, out, rts, thr):
    ref = pc.align_ref(d, c.q)
    for p in range(c.n_prob):
        valid = None if d["valid"] is None else d["valid"][p]
        assert pc.same_f32(thr[p], torch.quantile(d["conf"][p], pc.f32(c.q))), (c.id, p)
        path = pc.align_path(d["conf"][p], valid, c.q)
        R, t, s = rts[p, :9].view(3, 3), rts[p, 9:12], rts[p, 12]
        if path == "I":
            assert bits_equal(out[p], d["loc"][p]), f"{c.id}[{p}]: the identity route must hand the local points back bit for bit"
            assert torch.equal(R, torch.eye(3)) and torch.equal(t, torch.zeros(3)) and float(s) == 1.0
        else:
            fig("align-ortho", pc.ortho_err(R), pc.ORTHO_TOL, f"{c.id}[{p}] route {path}")
            fig("align-det", abs(float(torch.det(R.double())) - 1), pc.ORTHO_TOL, f"{c.id}[{p}]")
            fig("align-points", float((out[p].double() - ref[p]).abs().max()) / float(ref[p].abs().max()), pc.ALIGN_PTS_TOL, f"{c.id}[{p}] route {path}")


@pytest.mark.parametrize("c", pc.ALIGN_SHAPES + pc.ALIGN_FALLBACKS, **ID)
def test_align_shapes_and_fallbacks(built_lib, c):
    """1 .. 4 pixels (identity below 3, a three-point plane at 3), 1023 / 1025 pixels, one and three problems, with and without valid_mask; exactly two
    and three confident points, two and no valid points, ten ties at the threshold"""
    d = pc.build_align(c)
    out, rts, thr = pc.run_align(built_lib, DEV, d, c.q, what=c.id)
    _check_align(c, d, out, rts, thr)
    if c.kind != "shape":      # thr_out is optional: the same launch without it
        out2, rts2, _ = pc.run_align(built_lib, DEV, d, c.q, want_thr=False, what=c.id)
        assert bits_equal(out, out2) and bits_equal(rts, rts2)


@pytest.mark.parametrize("kind", pc.ALIGN_CLOUDS)
def test_align_degenerate_and_hard_clouds(built_lib, kind):
    """400 masked points on a tilted plane or line (at the origin and 50 away), a mirrored, an axis-planar and a far cloud, plus 40 pixels outside
    the mask that lie off the plane: R orthonormal with det +1; R, s, t and ALL pixels against Horn where the rotation is determined"""
    x, y, m = pc.cloud(kind)
    d = dict(conf=torch.ones(1, len(x)), loc=x[None].contiguous(), glob=y[None].contiguous(), valid=m[None])
    out, rts, _ = pc.run_align(built_lib, DEV, d, 0.0, what=kind)
    R, t, s = rts[0, :9].view(3, 3), rts[0, 9:12], rts[0, 12]
    Rh, th, sh = pc.horn_similarity(x[m], y[m])
    sel = torch.ones_like(m) if kind in pc.ROTATION_DETERMINED else m
    ref = (sh * x.double() @ Rh.t() + th)[sel]
    figs = {"ortho": pc.ortho_err(R), "det": abs(float(torch.det(R.double())) - 1), "scale": abs(float(s) - float(sh)) / float(sh),
            "points": float((out[0].double()[sel] - ref).abs().max()) / float(ref.abs().max())}
    if kind in pc.ROTATION_DETERMINED:
        figs.update(R=float((R.double() - Rh).abs().max()), t=float((t.double() - th).abs().max()))
    tol = dict(ortho=pc.ORTHO_TOL, det=pc.ORTHO_TOL, scale=pc.HORN_S_TOL, points=pc.ALIGN_PTS_TOL, R=pc.HORN_R_TOL, t=pc.HORN_T_TOL)
    for k, v in figs.items():
        print(f"[post-geometry] kind=cloud-{k} err={v:.3e} tol={tol[k]:.1e} {kind}")
    assert pc.horn_misses(R, t, s, x, y, m, kind) == []
    for k, v in figs.items():
        assert v <= tol[k], (kind, k, v)


def test_align_identical_points(built_lib):
    """sum |x - xm|^2 == 0: what is NaN in the oracle (the scale 0 / 0, hence t and every output) is NaN here, and R is still a rotation"""
    d = dict(conf=torch.ones(1, 16), loc=torch.full((1, 16, 3), 0.75), glob=torch.full((1, 16, 3), -1.5), valid=None)
    out, rts, _ = pc.run_align(built_lib, DEV, d, 0.0, what="identical")
    ref = pc.align_ref(d, 0.0)
    Ro, to, so = pc.align_oracle.rigid_points_registration(d["loc"][0].double(), d["glob"][0].double())
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and bool(torch.isnan(rts[0, 12])) == bool(torch.isnan(so))
    assert torch.equal(torch.isnan(rts[0, 9:12]), torch.isnan(to)) and torch.equal(torch.isnan(rts[0, :9].view(3, 3)), torch.isnan(Ro))
    fig("align-ortho", pc.ortho_err(rts[0, :9].view(3, 3)), pc.ORTHO_TOL, "identical points")


# ================================================================================================ focal
def _focal_close(got, ref, what):
    if ref != ref or got != got:
        assert ref != ref and got != got, f"{what}: NaN-ness differs from the oracle (kernel {got}, oracle {ref})"
        print(f"[post-geometry] kind=focal-nan both NaN {what}")
    else:
        fig("focal", abs(got - ref) / abs(ref), pc.FOCAL_TOL, what)


@pytest.mark.parametrize("c", pc.FOCAL, **ID)
def test_focal(built_lib, c):
    """1 x 1 .. 31 x 33 views, 0 / 1 / 10 iterations, q = 0 and q = 1 (one point), an off-centre principal point, both clamps, a NaN threshold (no
    point kept: focal_base), Z == 0 everywhere (NaN, as the reference's clip keeps it) and on a few kept pixels (nan_to_num); thr_out or not"""
    d = pc.build_focal(c)
    ref, thr_ref = pc.focal_ref(c, d)
    got, thr = pc.run_focal(built_lib, DEV, d["pts"][None], d["conf"][None], c.q, c.ppxy, c.n_iter, c.rng, what=c.id)
    assert pc.same_f32(thr[0], thr_ref), (c.id, thr, thr_ref)
    _focal_close(float(got[0]), ref, c.id)
    got2, none = pc.run_focal(built_lib, DEV, d["pts"][None], d["conf"][None], c.q, c.ppxy, c.n_iter, c.rng, want_thr=False, what=c.id)
    assert none is None and pc.same_f32(got, got2)
    if c.kind == "nan-thr":
        assert float(got[0]) == float(np.float32(c.base))


def test_focal_views_of_one_launch(built_lib):
    """three views in one launch: each bit-equal to its own single-view launch, and within the tolerance of the oracle"""
    cs = [next(c for c in pc.FOCAL if c.id == i) for i in pc.FOCAL_BATCH]
    pp = cs[2].ppxy
    ds = [pc.build_focal(c, pp=pp) for c in cs]
    pts, conf = torch.stack([d["pts"] for d in ds]), torch.stack([d["conf"] for d in ds])
    got, thr = pc.run_focal(built_lib, DEV, pts, conf, 0.1, pp, 10, (0.0, 3.0e38), what="batch")
    for v, (c, d) in enumerate(zip(cs, ds)):
        one, thr1 = pc.run_focal(built_lib, DEV, d["pts"][None], d["conf"][None], 0.1, pp, 10, (0.0, 3.0e38), what=c.id)
        assert bits_equal(one, got[v:v + 1]) and bits_equal(thr1, thr[v:v + 1]), c.id
        _focal_close(float(got[v]), pc.focal_ref(c, d, pp=pp)[0], f"batch view {v} ({c.id})")


# ================================================================================================ PnP
def _run_case(lib, c, d=None):
    d = d or pc.build_pnp(c)
    fin = torch.tensor([c.f], dtype=torch.float32) if c.focal == "given" else None
    pose, f, inl = pc.run_pnp(lib, DEV, d["pts"][None], d["conf"][None], fin, c.ppxy, c.conf_thr, c.n_focals, c.n_iter, what=c.id)
    return pose[0], float(f[0]), int(inl[0])


def _check_pose(c, d, pose, f, inl):
    n = int(d["mask"].sum())
    f_ref, T_ref, inl_ref = pc.pnp_ref(c.id)
    if T_ref is None:
        assert torch.equal(pose, torch.eye(4)) and f != f and inl == 0, f"{c.id}: a failed view is the identity, a NaN focal and 0 inliers"
        return
    assert f == f, f"{c.id}: the view failed, the oracle solves it"
    R = pose[:3, :3]
    fig("pose-ortho", pc.ortho_err(R), pc.ORTHO_TOL, c.id)
    fig("pose-det", abs(float(torch.det(R.double())) - 1), pc.ORTHO_TOL, c.id)
    cnt, worst, zmin = pc.recount(c, d["pts"], d["mask"], pose, f)
    print(f"[post-geometry] kind=pose-recount inliers={cnt} of {n} reported={inl} worst_px={worst:.3e} {c.id}")
    assert cnt >= 1, f"{c.id}: no masked point within 5 px of the returned pose"
    if c.few and c.focal == "search":       # no value-by-value comparison: the plateau rules differ (docs/rows_f.md)
        assert float(np.abs(c.grid - f).min()) <= 1e-6 * f, f"{c.id}: {f} is no grid candidate"
        assert worst <= pc.REPROJ_THR and zmin > 0 and cnt == n and inl == n, (c.id, worst, zmin, cnt, inl)
        return
    fig("pose-focal", abs(f - f_ref) / f_ref, 1e-4 if c.focal == "search" else 1e-6, c.id)
    fig("pose", float((pose.double() - T_ref).abs().max()), pc.POSE_TOL, c.id)
    assert inl == inl_ref, (c.id, inl, inl_ref)
    if c.few:
        fig("pose-sqpnp", float((pose.double() - pc.sqpnp_on_mask(c, d)).abs().max()), pc.POSE_TOL, c.id)
        assert inl == n


@pytest.mark.parametrize("c", pc.PNP, **ID)
def test_poses(built_lib, c):
    """5 x 7 .. 48 x 64 and a one-row image; masks of 4, 5 (SQPnP on all masked points), 6, 7, 8, 12 and all points, on the first ten pixels and on
    the last row (every sample degenerate); 1 .. 100 iterations, 1 .. 100 focal candidates, focal given or searched, an off-centre principal point,
    another confidence threshold, 10 % gross outliers, fewer than 4 points"""
    d = pc.build_pnp(c)
    _check_pose(c, d, *_run_case(built_lib, c, d))


def _batch(lib, ids, what):
    cs = [pc.pnp_case(i) for i in ids]
    ds = [pc.build_pnp(c) for c in cs]
    fin = torch.tensor([c.f if c.focal == "given" else -1.0 for c in cs], dtype=torch.float32)
    pose, f, inl = pc.run_pnp(lib, DEV, torch.stack([d["pts"] for d in ds]), torch.stack([d["conf"] for d in ds]), fin, cs[0].ppxy, 1.0, 100, 100, what=what)
    for v, (c, d) in enumerate(zip(cs, ds)):
        p1, f1, i1 = _run_case(lib, c, d)
        assert bits_equal(pose[v], p1) and pc.same_f32(f[v], torch.tensor(f1)) and int(inl[v]) == i1, f"{what}: view {v} ({c.id}) differs from its own launch"
        _check_pose(c, d, pose[v], float(f[v]), int(inl[v]))


def test_pose_views_of_one_launch(built_lib):
    """a failing view, an ordinary one, one with four points and one with outliers in one launch: each bit-equal to its single-view launch"""
    _batch(built_lib, pc.PNP_BATCH, "batch")


def test_pose_mixed_focal_in(built_lib):
    """focal_in positive for one view and <= 0 for the next: that view searches the grid, as if launched alone with focal_in == NULL"""
    _batch(built_lib, pc.PNP_MIXED, "mixed focal_in")
