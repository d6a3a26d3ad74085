"""Times the confidence cleaning (`fast3r_amd.post_ops.clean_confidence`: f3r_clean_confidence, one launch per target view) against an eager
torch formulation of the same contract on the same GPU: per target view one set of tensor operations vectorised over its neighbours (what a
user would write from the reference's loop).  Both are bracketed by events on one stream after a warm-up; the record holds the median of the
repetitions with their minimum and maximum, and how many pixels the two disagree on (the eager einsum sums in another order).

Synthetic capture: N cameras on an arc of one radian, all looking at the same patch of the plane z = 3, so nearly every projection lands inside
the other image -- the expensive case for the gathers.  8 % of the pixels are floaters (pulled to 40 % .. 80 % of their depth, confidence
below every surface pixel's).  Workloads: 320 views of 512 x 512 over swin-5 and over the complete graph, 20 views over the complete graph;
the complete graph of 320 views is also timed on the same capture without floaters, which shows what the early exit of flagged lanes is
worth.  Appends JSON lines to --out (profiles/clean_pointcloud_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast3r_amd import clean, post_ops  # noqa: E402

WORKLOADS = {"n320_swin5": dict(views=320, pairs="swin-5"), "n320_complete": dict(views=320, pairs="complete"),
             "n320_complete_no_floaters": dict(views=320, pairs="complete", floaters=0.0, eager=False),
             "n20_complete": dict(views=20, pairs="complete")}


def make_capture(n, H, W, dev, floaters=0.08, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    vv, uu = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    f = 0.9 * max(H, W)
    ray = torch.stack([(uu - W / 2) / f, (vv - H / 2) / f, torch.ones_like(uu)], -1).reshape(-1, 3)
    pts, conf, depth, poses = [], [], [], []
    for v in range(n):
        a = (v / max(n - 1, 1) - 0.5) * 1.0
        b = 0.2 * np.sin(7.0 * v)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        R = Ry @ Rx
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = np.array([0.0, 0.0, 3.0]) - 3.0 * R[:, 2]  # the camera looks at (0, 0, 3) from three units away
        Tt = torch.from_numpy(T).to(dev)
        d = ray @ Tt[:3, :3].T
        t = (3.0 - Tt[2, 3]) / d[:, 2]
        fl = torch.rand(H * W, device=dev, generator=g) < floaters
        t = torch.where(fl, t * (0.4 + 0.4 * torch.rand(H * W, device=dev, generator=g).double()), t)
        c = torch.where(fl, 1.0 + 0.4 * torch.rand(H * W, device=dev, generator=g), 1.5 + 4.5 * torch.rand(H * W, device=dev, generator=g))
        local = (ray * t[:, None]).float()
        pts.append((local.double() @ Tt[:3, :3].T + Tt[:3, 3]).float())
        conf.append(c.float())
        depth.append(local[:, 2].contiguous())
        poses.append(Tt.float())
    intr = torch.tensor([[f, f, W / 2, H / 2]] * n, dtype=torch.float32, device=dev)
    return torch.cat(pts).contiguous(), torch.cat(conf).contiguous(), torch.cat(depth).contiguous(), torch.stack(poses).contiguous(), intr


def eager_clean(pts, conf, depth, poses, intr, shapes, starts, nbr, tol, max_bad_conf):
    """the contract in eager torch: per target view, every neighbour at once"""
    dev, N = pts.device, len(shapes)
    cams = torch.linalg.inv(poses.double()).float()
    Hs = torch.tensor([s[0] for s in shapes], device=dev)
    Ws = torch.tensor([s[1] for s in shapes], device=dev)
    off = torch.cumsum(Hs * Ws, 0) - Hs * Ws
    off_host = off.tolist()
    nbr_t = torch.from_numpy(nbr.astype(np.int64)).to(dev)
    omt = float(np.float32(1.0 - tol))
    res = conf.clone()
    for i in range(N):
        J = nbr_t[starts[i]:starts[i + 1]]
        if J.numel() == 0:
            continue
        n = shapes[i][0] * shapes[i][1]
        p, c = pts[off_host[i]:off_host[i] + n], conf[off_host[i]:off_host[i] + n]
        m = cams[J]
        q = torch.einsum("jrc,nc->jnr", m[:, :3, :3], p) + m[:, None, :3, 3]
        Z = q[..., 2]
        k = intr[J]
        u = (k[:, None, 0] * q[..., 0] + k[:, None, 2] * Z) / Z
        v = (k[:, None, 1] * q[..., 1] + k[:, None, 3] * Z) / Z
        ur, vr = u.round(), v.round()
        cone = (Z > 0) & (ur >= 0) & (ur < Ws[J, None]) & (vr >= 0) & (vr < Hs[J, None])
        e = off[J, None] + torch.where(cone, vr, 0.0).long() * Ws[J, None] + torch.where(cone, ur, 0.0).long()
        bad = (cone & (Z < omt * depth[e]) & (c[None, :] < res[e])).any(0)
        res[off_host[i]:off_host[i] + n] = torch.where(bad, c.clamp(max=max_bad_conf), c)
    return res


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / 1e3)
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "runs": len(ts)}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--eager-reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=0, help="override the number of views (a rehearsal)")
    ap.add_argument("--tol", type=float, default=0.001)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_pointcloud_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_clean: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda")
    for name in (list(WORKLOADS) if args.workload == "all" else [args.workload]):
        w = WORKLOADS[name]
        n, H, W = args.views or w["views"], args.size, args.size
        floaters = w.get("floaters", 0.08)
        pts, conf, depth, poses, intr = make_capture(n, H, W, dev, floaters)
        shapes = [(H, W)] * n
        starts, nbr = clean.neighbour_lists(w["pairs"], n)
        kernel = lambda: post_ops.clean_confidence(pts, conf, depth, poses, intr, shapes, starts, nbr, tol=args.tol, max_bad_conf=0.0)  # noqa: E731
        kernel()  # warm-up
        s_kernel, (out, lowered) = timed(kernel, args.reps)
        rec = {"workload": name, "views": n, "H": H, "W": W, "pairs": w["pairs"], "projections": int(len(nbr)) * H * W, "floaters": floaters,
               "tol": args.tol, "device": torch.cuda.get_device_name(0), "lowered_pixels": int(lowered.sum()), "pixels": n * H * W,
               "kernel": s_kernel, "projections_per_s": int(len(nbr)) * H * W / s_kernel["median_s"]}
        if w.get("eager", True):
            eager = lambda: eager_clean(pts, conf, depth, poses, intr, shapes, starts, nbr, args.tol, 0.0)  # noqa: E731
            eager()
            s_eager, ref = timed(eager, args.eager_reps)
            rec.update({"eager_torch": s_eager, "speedup": s_eager["median_s"] / s_kernel["median_s"],
                        "pixels_that_differ_from_eager": int((ref != out).sum())})
            del ref
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del pts, conf, depth, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
