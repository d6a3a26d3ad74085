"""Timing of the multi-view depth metrics (fast3r_amd/depth_metric.py, f3r_depth.hip) as JSON lines, for N views of H x W, B = 1, the
local head, alignment "median", with and without the sparsification curves:
  * the three entry points on a prepared table: device events around f3r_depth_medians, f3r_depth_errors and f3r_depth_sparsify, one
    warm-up, the median, minimum and maximum of --reps runs, and the algorithmic bytes per second of the error pass (ground truth, the
    pointmap's cache lines, mask: 4 + 12 + 1 bytes per pixel read once);
  * `evaluate_multiview_depth` as a whole (table build and upload, launches, the one copy back): wall clock around a synchronise;
  * a torch-eager restatement of the same steps on the same GPU in the same run (per view: masks, sort-based medians, fp64 errors, two
    stable argsorts, suffix sums), timed the same way, and whether its results agree;
  * the numpy restatement (tests/depth_ref.py) on this box's CPU for the first --cpu-views views, scaled linearly to N and labelled so.
Inputs are generated on the device from a seed: a smooth positive depth with holes, a prediction at half scale with 5 % noise."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import depth_ref  # noqa: E402
import fast3r_amd  # noqa: E402
from fast3r_amd import _lib, post_ops  # noqa: E402


def make_views(n, H, W, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    views, preds = [], []
    for i in range(n):
        depth = 3.0 + torch.sin(xx / 50.0 + i) * torch.cos(yy / 40.0) + 0.01 * torch.randn(H, W, device=dev, generator=g)
        depth[torch.rand(H, W, device=dev, generator=g) < 0.02] = 0.0
        pts = torch.randn(1, H, W, 3, device=dev, generator=g)
        pts[0, ..., 2] = 0.5 * depth * (1.0 + 0.05 * torch.randn(H, W, device=dev, generator=g))
        views.append({"depthmap": depth[None].contiguous(), "valid_mask": (depth > 0)[None].contiguous(), "label": [f"bench/{i}"]})
        preds.append({"pts3d_local": pts, "conf_local": 1.0 + torch.rand(1, H, W, device=dev, generator=g)})
    return views, preds


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    return {"ms": statistics.median(ev), "ms_min": min(ev), "ms_max": max(ev), "wall_ms": statistics.median(wall), "wall_ms_min": min(wall),
            "wall_ms_max": max(wall)}


def eager(views, preds, uncertainty, K, thr=1.03):
    """the same steps with torch ops, view by view -> (scale, absrel, inliers, ause) lists"""
    out = []
    for v, p in zip(views, preds):
        g, z, c = v["depthmap"].reshape(-1), p["pts3d_local"][..., 2].reshape(-1), p["conf_local"].reshape(-1)
        ok = (g > 0) & torch.isfinite(g) & torch.isfinite(z) & v["valid_mask"].reshape(-1)
        gv, pv = g[ok].double(), z[ok].double()
        n = gv.numel()
        gs, ps = gv.sort().values, pv.sort().values
        s = ((gs[(n - 1) // 2] + gs[n // 2]) / 2) / ((ps[(n - 1) // 2] + ps[n // 2]) / 2)
        sp = s * pv
        e = (sp - gv).abs() / gv
        inl = 100.0 * (torch.maximum(gv / sp, sp / gv) < thr).sum().double() / n
        row = [s, 100.0 * e.sum() / n, inl]
        if uncertainty:
            r = (n * torch.arange(K, device=g.device)) // K
            curves = []
            for order in (torch.argsort(c[ok], stable=True), torch.argsort(-e.float(), stable=True)):
                suffix = torch.flip(torch.cumsum(torch.flip(e[order], (0,)), 0), (0,))
                curves.append(suffix[r] / (n - r))
            d = (curves[0] - curves[1]) / curves[0][0]
            row.append(((d[:-1] + d[1:]) / (2.0 * K)).sum())
        out.append(torch.stack([x.double() for x in row]))
    return torch.stack(out).cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, nargs="+", default=[100, 320])
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu-views", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = args.size
    K = args.bins
    for N in args.views:
        views, preds = make_views(N, H, W, dev)
        base = {"views": N, "H": H, "W": W, "B": 1, "head": "local", "alignment": "median", "n_bins": K, "device": torch.cuda.get_device_name(0),
                "reps": args.reps, "pixels": N * H * W}
        g = [v["depthmap"][0] for v in views]
        p = [q["pts3d_local"][0] for q in preds]
        c = [q["conf_local"][0] for q in preds]
        m = [v["valid_mask"][0].view(torch.uint8) for v in views]
        plan = post_ops.depth_plan(g, p, c, m, n_bins=K)
        med = timed(lambda: post_ops.depth_medians(plan, _lib.F3R_DEPTH_ALIGN_MEDIAN, None), args.reps)
        err = timed(lambda: post_ops.depth_errors(plan), args.reps)
        spa = timed(lambda: post_ops.depth_sparsify(plan), args.reps)
        read = N * H * W * (4 + 12 + 1)
        print(json.dumps(dict(base, what="entry points on a prepared table (device events)", medians_ms=med, errors_ms=err, sparsify_ms=spa,
                              errors_read_bytes=read, errors_algorithmic_GB_per_s=read / (err["ms"] * 1e-3) / 1e9,
                              sparsify_workspace_bytes=_lib.lib().f3r_depth_workspace_bytes(N, plan["n_tiles"], plan["total"], 1, K))), flush=True)
        for unc in (False, True):
            call = lambda: fast3r_amd.evaluate_multiview_depth(views, preds, eval_uncertainty=unc, n_bins=K)  # noqa: E731
            ours = timed(call, args.reps)
            res = call()[0]
            theirs = timed(lambda: eager(views, preds, unc, K), max(3, args.reps // 3))
            ref = eager(views, preds, unc, K)
            pv = res["per_view"]
            agree = {"scale": float(np.abs(pv["scale"] / ref[:, 0] - 1).max()), "absrel": float(np.abs(pv["absrel"] / ref[:, 1] - 1).max()),
                     "inliers": float(np.abs(pv["inliers_1.03"] - ref[:, 2]).max())}
            if unc:
                agree["ause"] = float(np.abs(pv["ause"] - ref[:, 3]).max())
            print(json.dumps(dict(base, what="evaluate_multiview_depth against the torch-eager restatement, same GPU, same run", eval_uncertainty=unc,
                                  call_wall_ms=ours["wall_ms"], call_wall_ms_min=ours["wall_ms_min"], call_wall_ms_max=ours["wall_ms_max"],
                                  eager_wall_ms=theirs["wall_ms"], eager_wall_ms_min=theirs["wall_ms_min"], eager_wall_ms_max=theirs["wall_ms_max"],
                                  largest_differences=agree, agree=bool(agree["scale"] < 1e-12 and agree["absrel"] < 1e-10 and agree["inliers"] < 1e-9
                                                                        and agree.get("ause", 0.0) < 1e-9),
                                  absrel=res["absrel"], inliers=res["inliers_1.03"], ause=res.get("ause"))), flush=True)
        n = min(args.cpu_views, N)
        if n > 0 and N == args.views[-1]:
            host = [(g[i].cpu().numpy(), p[i][..., 2].cpu().numpy(), c[i].cpu().numpy(), m[i].cpu().numpy()) for i in range(n)]
            for unc in (False, True):
                t0 = time.perf_counter()
                for a in host:
                    depth_ref.segment(*a, uncertainty=unc, n_bins=K)
                ms = (time.perf_counter() - t0) * 1e3
                print(json.dumps(dict(base, what="numpy restatement on the host CPU (tests/depth_ref.py)", eval_uncertainty=unc, cpu_views=n,
                                      cpu_ms_per_view=ms / n, cpu_ms_scaled_linearly_to_views=ms * N / n)), flush=True)
        del views, preds, plan, g, p, c, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
