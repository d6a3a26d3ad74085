#!/usr/bin/env python3
"""Times the stages of render_cumulative_pts3d_viz on the GPU, on seeded random pointmaps of the flagship shape (no model run): one JSON
line per stage, absolute times (the reference's pyrender path has no display or GL stack to run on here, so there is nothing to compare
with).  Device stages are host clocks around work that ends in a synchronise, after a warm-up pass; every stage is repeated and the
median and the spread are printed.

  combine    combine_points (percentile thresholds, compaction, colour line) + the centre + the bounding box
  splat      the N splats into one key buffer (a library built with F3R_EXTRA_FLAGS=-DF3R_RENDER_NO_EARLY_OUT times the atomics alone)
  resolve    N resolves of the final key buffer
  d2h        N device-to-host copies of a picture
  png        PNG encoding of --png-frames pictures through PIL on --workers threads, scaled to N in the line's "scaled_s"

    python tools/render_bench.py --views 320 --size 512 [--width 1920 --height 1080 --point-size 5 --reps 3 --zoom 4]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return out


def line(stage, times, **extra):
    print(json.dumps(dict(stage=stage, median_s=round(statistics.median(times), 6), min_s=round(min(times), 6), max_s=round(max(times), 6),
                          reps=len(times), **extra)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=320)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--point-size", type=float, default=5.0)
    ap.add_argument("--percentile", type=float, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--png-frames", type=int, default=32)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--zoom", type=float, default=1.0, help="camera distance divided by this (1: the notebook's camera, which leaves the "
                    "cloud small in the picture; 4 fills most of it)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: no ROCm device; a time taken elsewhere says nothing about this path")
    import fast3r_amd
    from fast3r_amd import post_ops, render
    dev = torch.device("cuda")
    N, S = args.views, args.size
    g = torch.Generator(device=dev).manual_seed(0)
    preds, views = [], []
    for i in range(N):  # a room-like scene: a slab of points per view, shifted along x
        pts = torch.rand((1, S, S, 3), generator=g, device=dev) * torch.tensor([4.0, 3.0, 1.5], device=dev) + torch.tensor([0.02 * i, -1.5, 0.0], device=dev)
        preds.append({"pts3d_in_other_view": pts, "conf": torch.rand((1, S, S), generator=g, device=dev) + 1.0})
        views.append({"img": torch.rand((1, 3, S, S), generator=g, device=dev) * 2.0 - 1.0})
    shape = dict(views=N, size=S, width=args.width, height=args.height, point_size=args.point_size, zoom=args.zoom)

    state = {}

    def combine():
        p, c, ends = fast3r_amd.combine_points(preds, views, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                               min_conf_thr_percentile=args.percentile, return_offsets=True)
        lo, hi, _ = post_ops.cloud_bounds(p)
        center = post_ops.render_center(p)
        box = [[m + (b - m) / args.zoom for m, b in zip(center, side)] for side in (lo, hi)]   # the box shrunk about the centre: a nearer camera
        state.update(points=p, colors=c, ends=ends, camera=fast3r_amd.birdseye_camera(center, *box))

    combine()
    line("combine+center+bounds", timed(combine, args.reps), points=int(state["points"].shape[0]), **shape)
    p, c, ends, cam = state["points"], state["colors"], state["ends"], state["camera"].words()

    def splats():
        keys = post_ops.render_keys(args.width, args.height, dev)
        start = 0
        for end in ends:
            post_ops.render_splat(p, start, end, cam, args.point_size, keys)
            start = end
        state["keys"] = keys

    splats()
    line("splat x N", timed(splats, args.reps), **shape)

    keys = state["keys"]
    post_ops.render_resolve(keys, c)
    line("resolve x N", timed(lambda: [post_ops.render_resolve(keys, c) for _ in range(N)], args.reps), **shape)
    picture = post_ops.render_resolve(keys, c)
    covered = float((picture != 255).any(-1).float().mean().item())
    line("d2h x N", timed(lambda: [picture.cpu() for _ in range(N)], args.reps), covered=round(covered, 4), **shape)

    host = picture.cpu().numpy()
    k = max(1, min(args.png_frames, N))
    with tempfile.TemporaryDirectory() as tmp:
        def pngs():
            with ThreadPoolExecutor(max_workers=args.workers) as pool:
                list(pool.map(lambda i: render._save_png(host, os.path.join(tmp, f"f{i:03d}.png")), range(k)))
        pngs()
        t = timed(pngs, args.reps)
        line(f"png x {k} on {args.workers} threads", t, scaled_s=round(statistics.median(t) * N / k, 3),
             png_bytes=os.path.getsize(os.path.join(tmp, "f000.png")), **shape)

    with tempfile.TemporaryDirectory() as tmp:   # the whole function, PNG files included
        t = timed(lambda: fast3r_amd.render_cumulative_pts3d_viz(preds, views, tmp, args.point_size, args.percentile, width=args.width,
                                                                 height=args.height, camera=state["camera"]), 1)
        line("render_cumulative_pts3d_viz, whole", t, files=len(os.listdir(tmp)), **shape)


if __name__ == "__main__":
    main()
