"""Timing of the ground-truth views (fast3r_amd/gt_views.py) as JSON lines:
  * the launch group: N frames of H x W to a resolution, frames on the device, plan and tables made once -- device events around the two
    kernel calls (`f3r_gtview_resample`, `f3r_gtview_unproject`) and the output allocations, one warm-up, the median and range of --reps
    runs, and the algorithmic bytes per second: per view the crop window's image bytes and the gathered depth read once, every output
    written once (the 8-bit intermediate between Pillow's passes is not counted);
  * `build_gt_views` on the same device frames: the whole call, with the host plan of every view, the table uploads and the read-back of
    the finite-depth flag (wall clock around a synchronise);
  * the PIL and numpy recipe on this box's host for the first --cpu-views frames: tests/gt_views_ref.py, the restatement that
    tools/make_golden_gt_views.py pins on the reference's dataset path (the reference itself is not needed to run this), per view, and
    whether `build_gt_views` equals it on those frames.
Images are random bytes, depths a smooth positive field with noise; the principal point sits off the centre, so both crops are real."""
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

import fast3r_amd  # noqa: E402
import gt_views_ref  # noqa: E402
from fast3r_amd import gt_views  # noqa: E402


def make_frames(n, H, W, seed=0):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    images, depths, poses = [], [], []
    for i in range(n):
        images.append(rs.randint(0, 256, (H, W, 3)).astype(np.uint8))
        depths.append((2.0 + np.sin(xx / 50.0 + i) * np.cos(yy / 40.0) + 0.01 * rs.standard_normal((H, W))).astype(np.float32))
        q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = q, rs.uniform(-3, 3, 3)
        poses.append(T.astype(np.float32))
    K = np.array([[0.8 * W, 0, W / 2 - 1.3], [0, 0.8 * W, H / 2 + 1.2], [0, 0, 1]], dtype=np.float32)
    return images, depths, [K] * n, poses


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
    return {"ms": statistics.median(ev), "ms_min": min(ev), "ms_max": max(ev), "wall_ms": statistics.median(wall)}


def algorithmic_bytes(plan):
    """per view: the window's image bytes and one depth per output pixel read; img_u8, img, depthmap, pts3d and valid_mask written"""
    l, t, r, b = plan["box1"]
    out = plan["target"][0] * plan["target"][1]
    return (r - l) * (b - t) * 3 + out * 4, out * (3 + 12 + 4 + 12 + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=320)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--resolution", type=int, nargs=2, default=(512, 384))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--cpu-views", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, H, W, res = args.views, args.height, args.width, tuple(args.resolution)
    images, depths, Ks, poses = make_frames(N, H, W)
    d_images = [torch.from_numpy(a).to(dev) for a in images]
    d_depths = [torch.from_numpy(a).to(dev) for a in depths]
    base = {"views": N, "H": H, "W": W, "resolution": list(res), "device": torch.cuda.get_device_name(0), "reps": args.reps}

    plan = gt_views.plan_view((W, H), Ks[0], res)
    tables = gt_views._Tables(plan, dev)
    cams = np.zeros((N, 25), dtype=np.float32)
    for i in range(N):
        cams[i, :9], cams[i, 9:] = plan["intrinsics"].reshape(-1), poses[i].reshape(-1)
    cams = torch.from_numpy(cams).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rd, wr = algorithmic_bytes(plan)
    rec = dict(base, what="one launch group: f3r_gtview_resample + f3r_gtview_unproject, frames on the device", window=list(plan["box1"]),
               resized=list(plan["resized"]), crop=list(plan["box2"]), filter=plan["filter"], read_bytes=rd * N, written_bytes=wr * N,
               **timed(lambda: gt_views._run_group(plan, tables, d_images, d_depths, cams, flag), args.reps))
    rec["algorithmic_GB_per_s"] = (rd + wr) * N / (rec["ms"] * 1e-3) / 1e9
    rec["us_per_view"] = rec["ms"] * 1e3 / N
    print(json.dumps(rec), flush=True)

    whole = timed(lambda: fast3r_amd.build_gt_views(d_images, d_depths, Ks, poses, resolution=res), max(3, args.reps // 3))
    print(json.dumps(dict(base, what="build_gt_views, frames on the device: host plans, table uploads, launches, the flag's read-back",
                          wall_ms=whole["wall_ms"], wall_us_per_view=whole["wall_ms"] * 1e3 / N)), flush=True)

    n = min(args.cpu_views, N)
    if n > 0:
        t0 = time.perf_counter()
        ref = gt_views_ref.build(images[:n], depths[:n], Ks[:n], poses[:n], res)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        sub = fast3r_amd.build_gt_views(d_images[:n], d_depths[:n], Ks[:n], poses[:n], resolution=res)
        same = all(np.ascontiguousarray(v[key][0].cpu().numpy()).tobytes() == np.ascontiguousarray(r[key]).tobytes()
                   for v, r in zip(sub, ref) for key in gt_views_ref.KEYS_EXACT)
        close = all(gt_views_ref.pts3d_close(v["pts3d"][0].cpu().numpy(), r)[0] for v, r in zip(sub, ref))
        print(json.dumps(dict(base, what="PIL and numpy recipe on the host (tests/gt_views_ref.py)", cpu_views=n, cpu_ms_per_view=cpu_ms / n,
                              cpu_ms_scaled_linearly_to_views=cpu_ms * N / n, exact_fields_equal_build_gt_views=bool(same),
                              pts3d_within_the_derived_bound=bool(close))), flush=True)


if __name__ == "__main__":
    main()
