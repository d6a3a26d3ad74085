"""Times `fast3r_amd.match_views` against the same work done with the entry points that existed before it, in the same process on one GPU:
one `NNIndex` per view (f3r_nn_build), one `query` per directed pair (f3r_nn_query), the reciprocity in torch.  Both take the same candidates
(`matching.view_candidates`, timed inside both) and must return identical matches: the tool asserts it.  Runs alternate after a warm-up; the
baseline is run twice per repetition (as A and as A'), so that the record shows the run-to-run spread next to the difference.

Synthetic pointmaps: every view samples one smooth surface with noise through a 512 x 512 window whose centre moves round a circle, so that
neighbouring views overlap and distant ones do not.  Three workloads: N = 320 with subsample 4 over swin-3; N = 20 at full resolution over
the complete graph; N = 20 with subsample 4 where 1 % of every view's points lie 1000 extents away (a stretched grid: run it with fewer
views and repetitions).  A host figure for scipy's cKDTree (the reference's find_reciprocal_matches, 8 workers) on a few pairs of the same data
is scaled to all pairs.  Appends JSON lines to --out (profiles/match_views_bench.jsonl)."""
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

import fast3r_amd  # noqa: E402
from fast3r_amd import matching  # noqa: E402
from fast3r_amd.recon_metric import NNIndex  # noqa: E402

WORKLOADS = {"n320_sub4_swin3": dict(views=320, subsample=4, pairs="swin-3"), "n20_full_complete": dict(views=20, subsample=1, pairs="complete"),
             # 1 % of every view's points 1000 extents away (sky, depth outliers): match_views keeps one grid per view, f3r_nn_build has two
             "n20_sub4_complete_outliers": dict(views=20, subsample=4, pairs="complete", outliers=0.01)}


def make_views(n, H, W, dev, seed=0, outliers=0.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    preds = []
    radius = 0.12 * n / (2 * np.pi)  # neighbouring windows of side 1 are 0.12 apart: about seven views overlap a view on either side
    for v in range(n):
        a = 2 * np.pi * v / n
        x = radius * np.cos(a) + xx / W + 0.3 / W * (torch.rand((H, W), device=dev, generator=g) - 0.5)
        y = radius * np.sin(a) + yy / H + 0.3 / H * (torch.rand((H, W), device=dev, generator=g) - 0.5)
        z = 2.0 + 0.3 * torch.sin(1.7 * x) * torch.cos(1.3 * y) + 0.002 * torch.randn((H, W), device=dev, generator=g)
        conf = 1.0 + 4.0 * torch.rand((H, W), device=dev, generator=g)
        if outliers > 0:
            far = torch.rand((H, W), device=dev, generator=g) < outliers
            z = torch.where(far, z + 1000.0 * (1.0 + torch.rand((H, W), device=dev, generator=g)), z)
        preds.append({"pts3d_in_other_view": torch.stack([x, y, z], -1)[None].contiguous(), "conf": conf[None].contiguous()})
    return preds


def baseline(preds, pairs, subsample):
    """the parent commit's entry points: an index per view, a query per directed pair, torch for the rest"""
    pts = [p["pts3d_in_other_view"][0] for p in preds]
    conf = [p["conf"][0] for p in preds]
    points, pix, counts, widths = matching.view_candidates(pts, conf, [None] * len(pts), 0.0, subsample)
    seg = np.concatenate([[0], np.cumsum(counts)])
    cand = [points[seg[v]:seg[v + 1]] for v in range(len(pts))]
    index, nn = {}, {}
    for i, j in pairs.tolist():
        for a, b in ((i, j), (j, i)):
            if (a, b) not in nn:
                if b not in index:
                    index[b] = NNIndex(cand[b])
                nn[(a, b)] = index[b].query(cand[a])
    xy_i, xy_j, dist, cnt = [], [], [], []
    for i, j in pairs.tolist():
        (_, nn_ij), (d_ji, nn_ji) = nn[(i, j)], nn[(j, i)]
        rec = nn_ij.long()[nn_ji.long()] == torch.arange(counts[j], device=points.device)
        q = rec.nonzero().squeeze(1)
        pj, pi = pix[seg[j]:seg[j + 1]][q].long(), pix[seg[i]:seg[i + 1]][nn_ji.long()[q]].long()
        wi, wj = int(pts[i].shape[1]), int(pts[j].shape[1])
        xy_j.append(torch.stack([pj % wj, pj // wj], 1).int())
        xy_i.append(torch.stack([pi % wi, pi // wi], 1).int())
        dist.append(d_ji[q])
        cnt.append(q.numel())
    return torch.cat(xy_i), torch.cat(xy_j), torch.cat(dist), cnt


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "runs": len(ts)}


def ckdtree_host(preds, pairs, subsample, n_pairs):
    from scipy.spatial import cKDTree
    ts = []
    for i, j in pairs[:n_pairs].tolist():
        P1, P2 = (preds[v]["pts3d_in_other_view"][0, ::subsample, ::subsample].reshape(-1, 3).cpu().numpy() for v in (i, j))
        t0 = time.perf_counter()
        t1, t2 = cKDTree(P1), cKDTree(P2)
        _, nn1 = t2.query(P1, workers=8)
        _, nn2 = t1.query(P2, workers=8)
        (nn1[nn2] == np.arange(len(nn2))).sum()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=sorted(WORKLOADS) + ["all"], default="all")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=0, help="override the number of views (a rehearsal)")
    ap.add_argument("--host-pairs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_views_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("match_views_bench: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda")
    for name in (sorted(WORKLOADS) if args.workload == "all" else [args.workload]):
        w = dict(WORKLOADS[name])
        n = args.views or w["views"]
        preds = make_views(n, args.size, args.size, dev, outliers=w.get("outliers", 0.0))
        pairs = fast3r_amd.scene_graph_pairs(n, w["pairs"], symmetrize=False)
        new = lambda: fast3r_amd.match_views(preds, pairs=w["pairs"], subsample=w["subsample"])  # noqa: E731
        old = lambda: baseline(preds, pairs, w["subsample"])  # noqa: E731
        vm, ref = new(), old()  # warm-up of both, and the comparison
        same = (torch.equal(vm.xy_i, ref[0]) and torch.equal(vm.xy_j, ref[1]) and torch.equal(vm.dist, ref[2]) and vm.counts.tolist() == ref[3])
        assert same, f"{name}: match_views and the per-view loop disagree"
        t_new, t_old, t_old2 = [], [], []
        for _ in range(args.reps):
            t_old.append(timed(old)[0])
            t_new.append(timed(new)[0])
            t_old2.append(timed(old)[0])
        cand = (-(-args.size // w["subsample"])) ** 2
        queries = int(sum(2 if i != j else 1 for i, j in pairs.tolist())) * cand
        host = ckdtree_host(preds, pairs, w["subsample"], args.host_pairs)
        s_new, s_old, s_old2 = summary(t_new), summary(t_old), summary(t_old2)
        rec = {"workload": name, "views": n, "H": args.size, "W": args.size, "subsample": w["subsample"], "pairs": w["pairs"], "outliers": w.get("outliers", 0.0), "n_pairs": int(len(pairs)),
               "candidates_per_view": cand, "directed_queries": queries, "matches": int(vm.counts.sum()), "device": torch.cuda.get_device_name(0),
               "identical_matches": bool(same), "chunks": vm.n_chunks, "workspace_bytes": int(vm.workspace_bytes),
               "match_views": s_new, "per_view_loop": s_old, "per_view_loop_again": s_old2,
               "queries_per_s": {"match_views": queries / s_new["median_s"], "per_view_loop": queries / s_old["median_s"]},
               "speedup": s_old["median_s"] / s_new["median_s"],
               "baseline_spread": abs(s_old["median_s"] - s_old2["median_s"]) / s_old["median_s"],
               "ckdtree_host": {"pairs_timed": len(host), "median_s_per_pair": statistics.median(host), "scaled_to_all_pairs_s": statistics.median(host) * len(pairs),
                                "workers": 8}}
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del preds, vm, ref


if __name__ == "__main__":
    main()
