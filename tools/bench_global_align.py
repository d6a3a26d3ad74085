"""Times the global alignment: one loss-and-gradient evaluation (`fast3r_amd.post_ops.galign_loss_grad`: f3r_galign_loss_grad) and a
300-iteration `PointCloudOptimizer.compute_global_alignment`, against an eager torch restatement of the reference's `forward` plus autograd
on the same GPU in the same run (stacked predictions, full-size temporaries for every transform, as optimizer.py:237-256 computes it; its
loop reads the loss back every iteration, as base_opt.py:453 does).  Events on one stream, one warm-up, the median of the repetitions with
their minimum and maximum.

Workloads, each as K-anchor passes (pass a holds the edges (a, v), and all of them share the anchor's pointmap): 20 views of 512 x 512 over
the complete graph (380 edges), and 100 views over swin-3 (every view anchors its 3 neighbours on either side: 600 edges).  Pointmaps are
seeded noise around a consistent scene: the timing does not depend on the values.  Also reported: the bytes the contract must move -- 16 per
observation-pixel read, 8 per view-pixel read and written -- over the measured time.  Appends JSON lines to --out
(profiles/global_align_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fast3r_amd import PointCloudOptimizer, post_ops  # noqa: E402

WORKLOADS = {"n20_complete": dict(views=20, window=None), "n100_swin3": dict(views=100, window=3)}


def make_passes(n, window, H, W, dev, seed=0):
    """(view1, view2, pred1, pred2) of n anchor passes: edges (a, v) for the views v within `window` of a (cyclic), or all others"""
    g = torch.Generator(device=dev).manual_seed(seed)
    idx1, idx2, p1, c1, p2, c2 = [], [], [], [], [], []
    for a in range(n):
        others = [v for v in range(n) if v != a] if window is None else sorted({(a + d) % n for d in range(-window, window + 1) if d} - {a})
        maps = {}
        for v in [a] + others:
            pts = torch.randn((H, W, 3), device=dev, generator=g) * 0.3
            pts[..., 2] += 3.0
            maps[v] = (pts, 1.0 + 4.0 * torch.rand((H, W), device=dev, generator=g))
        for v in others:
            idx1.append(a), idx2.append(v)
            p1.append(maps[a][0]), c1.append(maps[a][1]), p2.append(maps[v][0]), c2.append(maps[v][1])
    return {"idx": idx1}, {"idx": idx2}, {"pts3d": p1, "conf": c1}, {"pts3d_in_other_view": p2, "conf": c2}


def eager_problem(net):
    """the reference's buffers: stacked predictions and weights per side, the pixel grid, the edge indices"""
    dev, (H, W) = net.device, net.imshapes[0]
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    grid = torch.stack((xs, ys), dim=-1).reshape(1, H * W, 2).expand(net.n_imgs, -1, -1).contiguous()
    E = net.n_edges
    return {"grid": grid, "pred_i": torch.stack([net._pts[2 * e].reshape(-1, 3) for e in range(E)]),
            "pred_j": torch.stack([net._pts[2 * e + 1].reshape(-1, 3) for e in range(E)]),
            "w_i": torch.stack([net._weight[2 * e].reshape(-1) for e in range(E)]), "w_j": torch.stack([net._weight[2 * e + 1].reshape(-1) for e in range(E)]),
            "ei": torch.tensor([i for i, j in net.edges], device=dev), "ej": torch.tensor([j for i, j in net.edges], device=dev),
            "area_i": net.total_area_i, "area_j": net.total_area_j, "l2": net.dist == "l2"}


def eager_loss(leaves, B):
    """PointCloudOptimizer.forward in eager torch on the matrices"""
    poses, focals, pp, log_depth, pw, adapt = leaves
    depth = log_depth.view(poses.shape[0], -1).exp().unsqueeze(-1)
    rel = torch.cat((depth * (B["grid"] - pp.unsqueeze(1)) / focals.view(-1, 1, 1), depth), dim=-1)
    proj = rel @ poses[:, :3, :3].transpose(1, 2) + poses[:, None, :3, 3]
    dist = (lambda a, b, w: (a - b).square().sum(dim=-1) * w) if B["l2"] else (lambda a, b, w: (a - b).norm(dim=-1) * w)
    al_i = (adapt.unsqueeze(1) * B["pred_i"]) @ pw[:, :3, :3].transpose(1, 2) + pw[:, None, :3, 3]
    al_j = (adapt.unsqueeze(1) * B["pred_j"]) @ pw[:, :3, :3].transpose(1, 2) + pw[:, None, :3, 3]
    return dist(proj[B["ei"]], al_i, B["w_i"]).sum() / B["area_i"] + dist(proj[B["ej"]], al_j, B["w_j"]).sum() / B["area_j"]


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
    ap.add_argument("--loop-reps", type=int, default=3)
    ap.add_argument("--niter", type=int, default=300)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--views", type=int, default=0, help="override the number of views (a rehearsal)")
    ap.add_argument("--no-eager", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_align_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_global_align: needs a GPU (nothing is measured without one)")
    dev = torch.device("cuda")
    for name in (list(WORKLOADS) if args.workload == "all" else [args.workload]):
        w = WORKLOADS[name]
        n, H, W = args.views or w["views"], args.size, args.size
        torch.manual_seed(0)
        net = PointCloudOptimizer(*make_passes(n, w["window"], H, W, dev), rand_pose=lambda *s: 0.1 * torch.randn(*s)).to(dev)
        with torch.no_grad():  # a start near a plausible scene: identity-like poses, depth 3, pairwise scale about base_scale
            net.im_poses.data[:, 3] += 1.0
            net.pw_poses.data[:, 3] += 1.0
            net.im_depthmaps.data[:] = net.im_depthmaps.data * 0.1 + 0.4
        start = {k: p.detach().clone() for k, p in net.named_parameters()}
        obs = net._observations()
        E = net.n_edges
        with torch.no_grad():
            mats = [net.get_im_poses()[:, :3].contiguous(), net.get_focals().reshape(-1).contiguous(), net.get_principal_points().contiguous(),
                    net.im_depthmaps.detach().clone(), net.get_pw_poses()[:, :3].contiguous(), net.get_adaptors().contiguous()]
        kernel = lambda: post_ops.galign_loss_grad(*mats, obs.tables, "l1")  # noqa: E731
        kernel()  # warm-up
        s_kernel, out = timed(kernel, args.reps)
        moved = 16 * 2 * E * H * W + 8 * n * H * W
        rec = {"workload": name, "views": n, "H": H, "W": W, "edges": E, "observation_pixels": 2 * E * H * W, "dist": "l1",
               "device": torch.cuda.get_device_name(0), "loss": float(out[0]), "evaluation": s_kernel, "contract_bytes": moved,
               "contract_GB_per_s": moved / s_kernel["median_s"] / 1e9}

        def loop():
            with torch.no_grad():
                for k, p in net.named_parameters():
                    p.data[:] = start[k]
            return net.compute_global_alignment(niter=args.niter)
        loop()
        s_loop, final = timed(loop, args.loop_reps)
        rec.update({"niter": args.niter, "alignment": s_loop, "final_loss": final, "first_loss": float(net.loss_history[0])})
        if not args.no_eager:
            B = eager_problem(net)

            def eager():
                leaves = [m.clone().requires_grad_() for m in mats]
                loss = eager_loss(leaves, B)
                loss.backward()
                return loss.detach(), [x.grad for x in leaves]
            eager()
            s_eager, (eloss, egrads) = timed(eager, args.reps)
            worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip([out[2], out[3], out[4], out[1], out[5], out[6]], egrads))
            rec.update({"eager_evaluation": s_eager, "evaluation_speedup": s_eager["median_s"] / s_kernel["median_s"], "eager_loss": float(eloss),
                        "worst_gradient_difference_from_eager": worst})
            del egrads

            def eager_loop():
                leaves = [m.clone().requires_grad_() for m in mats]
                opt = torch.optim.Adam(leaves, lr=0.01, betas=(0.9, 0.9))
                last = None
                for _ in range(args.niter):
                    opt.zero_grad()
                    loss = eager_loss(leaves, B)
                    loss.backward()
                    opt.step()
                    last = float(loss)  # the reference's per-iteration read-back
                return last
            s_eloop, _ = timed(eager_loop, 1)
            rec.update({"eager_alignment": s_eloop, "alignment_speedup": s_eloop["median_s"] / s_loop["median_s"]})
            del B
        print(json.dumps(rec), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")
        del net, obs, mats, out, start
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
