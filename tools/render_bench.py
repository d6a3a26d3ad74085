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

--what mesh times the triangle rasteriser instead, on surface-like pointmaps of the same shape: build_mesh double- and single-sided, then
per mesh the rasteriser (host clock; its two kernels' device times from torch.profiler, with the number of triangles stage 1 queued for
stage 2), the resolve and render_mesh as a whole; for context the point splat of the same vertices through the same camera, and the
scene-with-cameras picture (the cloud at percentile 80 plus one camera pyramid per view carrying its image).

    python tools/render_bench.py --what mesh --views 320 --size 512 --zoom 4 [--out profiles/raster_bench.jsonl]
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


def kernel_times(fn, names):
    """device time per kernel-name fragment over one run of fn, from torch.profiler's kernel records (seconds); None where the profiler
    gives no device records on this build"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {n: 0.0 for n in names}
    seen = False
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA"):
            for n in names:
                if n in ev.name:
                    out[n] += ev.device_time_total * 1e-6 if hasattr(ev, "device_time_total") else ev.cuda_time_total * 1e-6
                    seen = True
    return {n: round(v, 6) for n, v in out.items()} if seen else None


def mesh_main(args):
    """--what mesh: surface-like pointmaps (a wavy sheet per view with a depth step, so the mesh holds rubber-sheet triangles), build_mesh,
    and render_mesh's stages through the bird's-eye camera of the vertices, its distance divided by --zoom"""
    import fast3r_amd
    from fast3r_amd import post_ops
    dev = torch.device("cuda")
    N, S, W, H = args.views, args.size, args.width, args.height
    g = torch.Generator(device=dev).manual_seed(0)
    v, u = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float32), torch.arange(S, device=dev, dtype=torch.float32), indexing="ij")
    focal = 1.2 * S
    preds, views = [], []
    for i in range(N):
        z = 2.0 + 0.3 * torch.sin(u / 40.0 + i) + 0.2 * torch.cos(v / 30.0) + 0.8 * (u > S / 2 + (i % 50)).float()
        pts = torch.stack([(u - S / 2 + 0.5 + 0.1 * i) * z / focal, (v - S / 2 + 0.5) * z / focal, z], dim=-1)
        preds.append({"pts3d_in_other_view": pts[None].contiguous(), "conf": torch.rand((1, S, S), generator=g, device=dev) + 1.0})
        views.append({"img": torch.rand((1, 3, S, S), generator=g, device=dev) * 2.0 - 1.0})
    shape = dict(views=N, size=S, width=W, height=H, zoom=args.zoom)
    sink = open(args.out, "a") if args.out else None

    def row(stage, times=None, **extra):
        rec = dict(stage=stage, **extra, **shape)
        if times is not None:
            rec.update(median_s=round(statistics.median(times), 6), min_s=round(min(times), 6), max_s=round(max(times), 6), reps=len(times))
        text = json.dumps(rec)
        print(text, flush=True)
        if sink:
            sink.write(text + "\n")
            sink.flush()

    def zoomed_camera(points):
        lo, hi, _ = post_ops.cloud_bounds(points)
        center = post_ops.render_center(points)
        box = [[m + (b - m) / args.zoom for m, b in zip(center, side)] for side in (lo, hi)]
        return fast3r_amd.birdseye_camera(center, *box)

    camera = None
    for double_sided in (True, False):
        sides = "double" if double_sided else "single"
        torch.cuda.synchronize()
        t = time.perf_counter()
        mesh = fast3r_amd.build_mesh(preds, views, min_conf_thr_percentile=args.percentile, double_sided=double_sided)
        torch.cuda.synchronize()
        build_s = time.perf_counter() - t
        if camera is None:
            camera = zoomed_camera(mesh.vertices)
        cam, nf = camera.words(), int(mesh.faces.shape[0])
        state = {}

        def raster():
            keys = post_ops.render_keys(W, H, dev)
            post_ops.raster_triangles(mesh.vertices, mesh.faces, cam, keys)
            state["keys"] = keys

        raster()
        ws, _ = post_ops.raster_workspace(dev, post_ops.RASTER_FACES_PER_LAUNCH)
        queued = int(ws[1].item())
        row(f"raster ({sides})", timed(raster, args.reps), faces=nf, queued=queued, build_mesh_s=round(build_s, 3))
        split = kernel_times(raster, ("raster_stage1_kernel", "raster_stage2_kernel"))
        row(f"raster kernels ({sides})", faces=nf, queued=queued, device_s=split)
        keys = state["keys"]
        row(f"resolve ({sides})", timed(lambda: post_ops.render_resolve(keys, mesh.face_colors), args.reps), faces=nf)
        picture = post_ops.render_resolve(keys, mesh.face_colors)
        covered = float((picture != 255).any(-1).float().mean().item())
        row(f"render_mesh, whole ({sides})", timed(lambda: fast3r_amd.render_mesh(mesh, camera, width=W, height=H), args.reps), faces=nf,
            covered=round(covered, 4))
        if double_sided:   # for context: the point splat of the same vertices through the same camera
            nv = int(mesh.vertices.shape[0])

            def splat():
                k = post_ops.render_keys(W, H, dev)
                post_ops.render_splat(mesh.vertices, 0, nv, cam, args.point_size, k)

            splat()
            row("splat of the vertices", timed(splat, args.reps), points=nv, point_size=args.point_size)
        del mesh, keys, picture, state
        torch.cuda.empty_cache()

    # the scene-with-cameras picture: the cloud at the notebook's percentile 80 and one camera per view carrying its image
    p, c = fast3r_amd.combine_points(preds, views, pts3d_key_to_visualize="pts3d_in_other_view", conf_key_to_visualize="conf",
                                     min_conf_thr_percentile=80)
    poses = []
    for i in range(N):   # where the sheets were seen from: the origin, shifted as the sheets are
        pose = torch.eye(4, dtype=torch.float64)
        pose[0, 3] = -0.1 * i * 2.5 / focal
        poses.append(pose.numpy())
    images = [vw["img"][0] for vw in views]
    cams = {}

    def cameras():
        cams["mesh"] = fast3r_amd.camera_meshes(poses, [focal] * N, images=images, cam_size=0.05)

    cameras()
    row("camera_meshes", timed(cameras, args.reps), cameras=N, faces=int(cams["mesh"]["faces"].shape[0]))
    scene_camera = zoomed_camera(p)
    scene = lambda: fast3r_amd.render_mesh(cams["mesh"], scene_camera, points=p, colors=c, point_size=1.0, width=W, height=H)   # noqa: E731
    scene()
    queued = int(post_ops.raster_workspace(dev, post_ops.RASTER_FACES_PER_LAUNCH)[0][1].item())
    row("scene with cameras (splat + raster + resolve)", timed(scene, args.reps), points=int(p.shape[0]), faces=int(cams["mesh"]["faces"].shape[0]),
        queued=queued)
    if sink:
        sink.close()


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
    ap.add_argument("--what", choices=("points", "mesh"), default="points", help="points: the stages above; mesh: render_mesh of build_mesh "
                    "output, double- and single-sided, split into the rasteriser's two stages and the resolve, the point splat of the same "
                    "vertices, and the scene-with-cameras picture")
    ap.add_argument("--out", default=None, help="--what mesh: also append the JSON lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_bench: no ROCm device; a time taken elsewhere says nothing about this path")
    if args.what == "mesh":
        return mesh_main(args)
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
