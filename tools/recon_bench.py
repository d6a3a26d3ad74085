"""Timings of the reconstruction metrics (fast3r_amd/recon_metric.py) as JSON lines:
  * index build, 1-NN of as many queries, k-NN + normals (k = 30) for 1 M and 4 M points: pointmap-like surfaces, and two
    clusters with 0.1 % far outliers at 1e4 x the scene scale;
  * one full evaluate_reconstruction sample of 20 views of 512 x 384;
  * the CPU path of tests/recon_ref.py (scipy cKDTree + numpy, the reference's metric code) on that sample's clouds, 16 threads.
GPU times are medians of --reps runs after one warm-up, each synchronised."""
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

import recon_ref  # noqa: E402
from fast3r_amd import MultiViewDUSt3RLitModule  # noqa: E402
from fast3r_amd.recon_metric import NNIndex  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    for kind, n in (("surface", 1 << 20), ("surface", 1 << 22), ("outliers", 1 << 20), ("outliers", 1 << 22)):
        db = torch.from_numpy(recon_ref.make_cloud(kind, n, 1)).to(dev)
        q = torch.from_numpy(recon_ref.make_cloud(kind, n, 2)).to(dev)
        ix = NNIndex(db)
        rec = {"what": "nn", "cloud": kind, "points": n, "queries": n, "device": name,
               "build_ms": timed(lambda: NNIndex(db), args.reps),
               "query_1nn_ms": timed(lambda: ix.query(q), args.reps),
               "knn30_normals_ms": timed(lambda: ix.knn(30), args.reps)}
        print(json.dumps(rec), flush=True)

    views, preds = recon_ref.make_eval_case(1, [(384, 512)] * 20, 7)
    views = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in views]
    preds = [{k: v.to(dev) for k, v in d.items()} for d in preds]
    lit = MultiViewDUSt3RLitModule(net=torch.nn.Identity())
    res = {}

    def run():
        res.update(lit.evaluate_reconstruction(views, preds, "bench", 50, 10))
    ms = timed(run, args.reps)
    pts = sum(v["valid_mask"].sum().item() for v in views)
    print(json.dumps({"what": "evaluate_reconstruction", "views": 20, "H": 384, "W": 512, "gt_points": pts, "ms": ms, "device": name}), flush=True)

    if args.no_cpu:
        return
    # the CPU path on the same clouds: normals of both (the Open3D restatement) + accuracy / completion with normals
    torch.set_num_threads(args.cpu_threads)
    gt = torch.cat([v["pts3d"][0][v["valid_mask"][0]] for v in views]).cpu().numpy()
    pr = torch.cat([p["pts3d_local_aligned_to_global"][0].reshape(-1, 3) for p in preds]).cpu().numpy()
    t0 = time.perf_counter()
    ngt, npr = recon_ref.estimate_normals(gt), recon_ref.estimate_normals(pr)
    t1 = time.perf_counter()
    recon_ref.accuracy(gt, pr, ngt, npr)
    recon_ref.completion(gt, pr, ngt, npr)
    t2 = time.perf_counter()
    print(json.dumps({"what": "cpu_recon_ref", "threads": args.cpu_threads, "gt_points": len(gt), "pred_points": len(pr),
                      "normals_ms": (t1 - t0) * 1e3, "metrics_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
