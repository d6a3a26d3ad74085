"""Timing of mesh export (fast3r_amd/mesh.py) as JSON lines:
  * `build_mesh` on N views of H x W at a percentile, inputs on the device: device events around the call (it reads the per-view counts
    back once inside, so the span includes that synchronisation), one warm-up, the median and range of --reps runs;
  * the same with drop_unreferenced=True, and `generate_mesh_ply_bytes` of the result when --ply is given;
  * the numpy path on this box's host for the first --cpu-views views of the same data: tests/mesh_ref.py, the restatement that
    tools/make_golden_mesh.py pins on the reference's `pts3d_to_trimesh` / `cat_meshes` bit for bit (the reference itself is not needed
    to run this), and its time scaled linearly to N views, labelled as scaled.
The confidences are a smooth lognormal field with noise on top, so that the kept fifth of a view has an interior and a ragged border."""
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
import mesh_ref  # noqa: E402


def make_views(n, H, W, dev, seed=0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    preds, views = [], []
    for _ in range(n):
        coarse = torch.randn(H // 32 + 1, W // 32 + 1, device=dev, generator=g)
        field = coarse.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W]
        conf = 1.0 + torch.exp(field + 0.3 * torch.randn(H, W, device=dev, generator=g))
        preds.append({"conf": conf[None].contiguous(), "pts3d_in_other_view": torch.randn(1, H, W, 3, device=dev, generator=g)})
        views.append({"img": torch.rand(1, 3, H, W, device=dev, generator=g) * 2.0 - 1.0})
    return preds, views


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=320)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--percentile", type=float, default=80)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-views", type=int, default=4)
    ap.add_argument("--ply", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    name = torch.cuda.get_device_name(0)
    N, H, W, p = args.views, args.height, args.width, args.percentile
    preds, views = make_views(N, H, W, dev)
    torch.cuda.synchronize()
    base = {"views": N, "H": H, "W": W, "percentile": p, "device": name, "reps": args.reps}
    mesh = fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=p)
    rec = dict(base, what="build_mesh", vertices=int(mesh.vertices.shape[0]), faces=int(mesh.faces.shape[0]),
               **timed(lambda: fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=p), args.reps))
    print(json.dumps(rec), flush=True)
    drop = fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=p, drop_unreferenced=True, index_dtype=torch.int32)
    rec = dict(base, what="build_mesh drop_unreferenced int32", vertices=int(drop.vertices.shape[0]), faces=int(drop.faces.shape[0]),
               **timed(lambda: fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=p, drop_unreferenced=True, index_dtype=torch.int32),
                       args.reps))
    print(json.dumps(rec), flush=True)
    if args.ply:
        t0 = time.perf_counter()
        raw = fast3r_amd.generate_mesh_ply_bytes(drop.vertices, drop.faces, drop.face_colors)
        print(json.dumps(dict(base, what="generate_mesh_ply_bytes of the drop_unreferenced mesh", bytes=len(raw),
                              wall_ms=(time.perf_counter() - t0) * 1e3)), flush=True)
        del raw
    n = min(args.cpu_views, N)
    if n > 0:
        host = [(views[i]["img"][0].cpu().numpy(), preds[i]["pts3d_in_other_view"][0].cpu().numpy(), preds[i]["conf"][0].cpu().numpy())
                for i in range(n)]
        t0 = time.perf_counter()
        ref = mesh_ref.build(host, p)
        cpu_ms = (time.perf_counter() - t0) * 1e3
        sub = fast3r_amd.build_mesh(preds[:n], views[:n], min_conf_thr_percentile=p)
        same = bool(np.array_equal(sub.faces.cpu().numpy(), ref["faces"]) and np.array_equal(sub.face_colors.cpu().numpy(), ref["face_colors"])
                    and sub.thresholds.tobytes() == ref["thresholds"].tobytes())
        print(json.dumps(dict(base, what="numpy restatement on the host (tests/mesh_ref.py)", cpu_views=n, cpu_ms=cpu_ms,
                              cpu_ms_scaled_linearly_to_views=cpu_ms * N / n, equals_build_mesh_on_those_views=same)), flush=True)


if __name__ == "__main__":
    main()
