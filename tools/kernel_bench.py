"""Kernel micro-benchmarks on the GPU box (interleaved rounds, random data, HIP events on the launch stream): the attention kernels
f3r_attn_fwd can take (--what attnproduct / attnsel / attnhd) and the model's GEMM / conv shapes per f3r_gemm_args.kernel_sel, with the vendor
library beside them (--what gemmref); --what loss: the validation criterion next to a torch-eager restatement; --what scene: scene assembly and PLY export likewise; --what cloud: point-cloud export (combine, voxel, farthest point) likewise; --what sky: sky detection alone, inside assemble_scene and next to the CPU (--what skydetect: its kernels alone, for a profiler run); --what maps: the map pictures next to PNG encoding and matplotlib's imsave.  Prints one JSON line per item.  (--what lab / labtime: ablations of the 8-wave GEMM, need
F3R_LAB_LIB=tools/lab/libf3r_hip_lab.so.)"""
import argparse
import math
import json
import sys

import torch

sys.path.insert(0, ".")
from fast3r_amd import _lib, ops, post_ops  # noqa: E402

DEV = "cuda"


def time_ms(fn, rounds=5, inner=3):
    best = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) / inner)
    best.sort()
    return best[len(best) // 2], best[0]


SEL_NAME = {0: "automatic", 1: "128-tile", 2: "256-tile persistent", 3: "256-tile lock-step", 4: "256x128-tile", 5: "256-tile one tile per workgroup",
            6: "hand-scheduled (asm)", 7: "compiler-scheduled kernels only"}


def bench_attn_product(dt, views, H=16):
    """The product attention kernel (no variant knob in the product library) on the fusion shape."""
    T = views * 1024
    D = H * 64
    q = torch.randn((T, D), device=DEV).to(dt)
    k = torch.randn((T, D), device=DEV).to(dt)
    vt = torch.randn((D, T), device=DEV).to(dt)
    o = torch.empty((T, D), dtype=dt, device=DEV)

    def f():
        ops.attention(q, o, H, 0.160192, [(k, vt, T, 0, 0)])
    f()
    med, mn = time_ms(f, rounds=3, inner=2)
    print(json.dumps({"kernel": "attn (product)", "dtype": str(dt).split(".")[-1], "views": views, "T": T, "ms": round(med, 3),
                      "tflops": round(4.0 * T * T * 64 * H / med / 1e9, 1)}), flush=True)


def bench_attn_sel(dt, views, sels=(1, 2), H=16, rounds=3, inner=2, tokens_per_view=1024):
    """The general HIP kernel (kernel_sel 1) next to the hand-scheduled one (kernel_sel 2) on the fusion shape, q pre-scaled."""
    T = views * tokens_per_view
    D = H * 64
    q = (torch.randn((T, D), device=DEV) * (0.160192 * 1.4426950408889634)).to(dt)
    k = torch.randn((T, D), device=DEV).to(dt)
    vt = torch.zeros((D, ops.vt_ld(T)), device=DEV, dtype=dt)
    vt[:, :T] = torch.randn((D, T), device=DEV).to(dt)
    outs = {}
    for sel in sels:
        o = torch.empty((T, D), dtype=dt, device=DEV)

        def f(sel=sel, o=o):
            ops.attention(q, o, H, 0.160192, [(k, vt, T, 0, 0)], q_prescaled=True, kernel_sel=sel)
        f()
        med, mn = time_ms(f, rounds=rounds, inner=inner)
        outs[sel] = o
        print(json.dumps({"kernel": "attn_sel", "kernel_sel": sel, "dtype": str(dt).split(".")[-1], "views": views, "T": T, "ms": round(med, 3),
                          "ms_min": round(mn, 3), "tflops": round(4.0 * T * T * 64 * H / med / 1e9, 1)}), flush=True)
    if 1 in outs and 2 in outs:
        a, b = outs[1].float(), outs[2].float()
        print(json.dumps({"kernel": "attn_sel", "views": views, "dtype": str(dt).split(".")[-1],
                          "rel_l2_asm_vs_hip": float((a - b).norm() / a.norm()), "nan": int(torch.isnan(b).sum())}), flush=True)


def bench_attn_head_dim(dt, views, hd, H=16, sels=(1, 0), T=None):
    """f3r_attn_fwd on a fusion-shaped problem with head_dim hd per f3r_attn_args.kernel_sel: 1 = the HIP kernel (the generic one unless hd = 64),
    0 = automatic (the generated kernel of csrc/asm/attn_gen.py at 64 / 80 / 128)"""
    T = views * 1024 if T is None else T
    D = H * hd
    q = (torch.randn((T, D), device=DEV) * (hd ** -0.5 * 1.4426950408889634)).to(dt)
    k = torch.randn((T, D), device=DEV).to(dt)
    vt = torch.zeros((D, ops.vt_ld(T)), device=DEV, dtype=dt)
    vt[:, :T] = torch.randn((D, T), device=DEV).to(dt)
    outs = {}
    for sel in sels:
        o = torch.empty((T, D), dtype=dt, device=DEV)

        def f():
            ops.attention(q, o, H, hd ** -0.5, [(k, vt, T, 0, 0)], q_prescaled=True, head_dim=hd, kernel_sel=sel)
        ops.ATTN_TIMER = []
        f()
        torch.cuda.synchronize()
        name = ops.ATTN_TIMER[0][5]
        ops.ATTN_TIMER = None
        med, mn = time_ms(f, rounds=3, inner=2)
        outs[sel] = o.float()
        print(json.dumps({"kernel": "attn_head_dim", "head_dim": hd, "kernel_sel": sel, "runs": name, "dtype": str(dt).split(".")[-1], "views": views, "T": T,
                          "ms": round(med, 3), "tflops": round(4.0 * T * T * hd * H / med / 1e9, 1), "tflops_best": round(4.0 * T * T * hd * H / mn / 1e9, 1)}), flush=True)
    if len(outs) == 2:
        a, b = list(outs.values())
        print(json.dumps({"kernel": "attn_head_dim", "head_dim": hd, "rel_l2_between_kernels": float((a - b).norm() / a.norm()), "nan": int(torch.isnan(b).sum())}), flush=True)


def bench_gemm(dt, M, N, K, name, act=None, res=False, out="f32", sels=(1, 2, 3), split=None):
    a = torch.randn((M, K), device=DEV).to(dt)
    a_lo = torch.randn((M, K), device=DEV).mul_(2.0 ** -11).to(dt) if split == "x3" else None
    w = ops.pack_linear_weight(torch.randn((N, K), device=DEV) * K ** -0.5, dt, split=split is not None)
    bias = torch.randn(N, device=DEV)
    x = torch.randn((M, N), device=DEV) if (res or out == "f32") else None
    olp = torch.empty((M, N), dtype=dt, device=DEV) if out == "lp" else None
    fns = {}
    for sel in sels:
        def f(sel=sel):
            if out == "f32":
                ops.gemm(a, w, bias=bias, act=act, res_f32=x if res else None, out_f32=x, kernel_sel=sel, split=split, a_lo=a_lo)
            else:
                ops.gemm(a, w, bias=bias, act=act, out_lp=olp, kernel_sel=sel, split=split, a_lo=a_lo)
        f()
        fns[sel] = f
    res_ms = {sel: [] for sel in sels}
    for _ in range(3):  # interleaved rounds
        for sel in sels:
            res_ms[sel].append(time_ms(fns[sel], rounds=3, inner=3)[0])
    mult = {None: 1, "w2": 2, "x3": 3}[split]
    for sel in sels:
        ms = sorted(res_ms[sel])[1]
        print(json.dumps({"kernel": "gemm", "name": name, "variant": SEL_NAME[sel], "split": split, "dtype": str(dt).split(".")[-1], "M": M, "N": N, "K": K,
                          "ms": round(ms, 3), "tflops_algorithmic": round(2.0 * M * N * K / ms / 1e9, 1),
                          "tflops_mfma": round(2.0 * M * N * K * mult / ms / 1e9, 1)}), flush=True)


def bench_library_matmul(dt, M, N, K, name):
    """A KNOWN-GOOD reference on the same box and the same random data (cdna_hip_programming.md rule 10 / 25): torch.matmul, i.e. the vendor
    library (hipBLASLt / rocBLAS), plain A W^T -> lowp, no epilogue.  Not a product path: a yardstick for what the chip gives this shape."""
    a = torch.randn((M, K), device=DEV).to(dt)
    w = (torch.randn((N, K), device=DEV) * K ** -0.5).to(dt)
    out = torch.empty((M, N), dtype=dt, device=DEV)
    f = lambda: torch.matmul(a, w.t(), out=out)  # noqa: E731
    f()
    ms = sorted(time_ms(f, rounds=3, inner=3)[0] for _ in range(3))[1]
    print(json.dumps({"kernel": "library matmul (torch.matmul -> hipBLASLt/rocBLAS)", "name": name, "dtype": str(dt).split(".")[-1], "M": M, "N": N, "K": K,
                      "ms": round(ms, 3), "tflops": round(2.0 * M * N * K / ms / 1e9, 1)}), flush=True)


LAB_BITS = {0: "lab baseline (staggered)", 1: "no LDS-DMA in loop", 2: "no fragment reads", 3: "no DMA, no reads (MFMA + barriers)", 4: "no MFMA",
            7: "barriers only", 8: "no vmcnt wait", 16: "no s_setprio", 32: "buffer_load lds", 33: "buffer_load, no DMA (sanity)",
            64: "no sched_barrier pin", 96: "buffer_load + no pin"}


def bench_lab(M, N, K):
    """Ablations of the 256-tile kernel (tools/lab/libf3r_hip_lab.so, F3R_LAB_LIB): which section of the phase costs what."""
    dt = torch.bfloat16
    a = torch.randn((M, K), device=DEV).to(dt)
    w = ops.pack_linear_weight(torch.randn((N, K), device=DEV) * K ** -0.5, dt)
    olp = torch.empty((M, N), dtype=dt, device=DEV)
    fns = {}
    for bits in LAB_BITS:
        def f(bits=bits):
            ops.gemm(a, w, out_lp=olp, kernel_sel=16 + bits)
        f()
        fns[bits] = f
    fns[-2] = lambda: ops.gemm(a, w, out_lp=olp, kernel_sel=2)
    fns[-1] = lambda: ops.gemm(a, w, out_lp=olp, kernel_sel=1)
    res_ms = {b: [] for b in fns}
    for _ in range(3):
        for b in fns:
            res_ms[b].append(time_ms(fns[b], rounds=3, inner=3)[0])
    for b in fns:
        ms = sorted(res_ms[b])[1]
        name = LAB_BITS.get(b, "product 256-tile" if b == -2 else "product 128-tile")
        print(json.dumps({"kernel": "gemm256_lab", "bits": b, "what": name, "M": M, "N": N, "K": K, "ms": round(ms, 3),
                          "tflops_nominal": round(2.0 * M * N * K / ms / 1e9, 1)}), flush=True)


def bench_labtime(M, N, K, act=None, bits=128):
    """Where a 256 x 256 output tile spends its time (lab bit 128: s_memtime stamps of wave 0 of every workgroup)."""
    from fast3r_amd import _lib
    dt = torch.bfloat16
    a = torch.randn((M, K), device=DEV).to(dt)
    w = ops.pack_linear_weight(torch.randn((N, K), device=DEV) * K ** -0.5, dt)
    bias = torch.randn(N, device=DEV)
    olp = torch.empty((M, N), dtype=dt, device=DEV)
    tiles = (M // 256) * (N // 256)
    dbg = torch.zeros((tiles, 5), dtype=torch.int64, device=DEV)
    L = _lib.lib()
    orig = L.f3r_gemm

    def patched(argp, stream):
        argp._obj.rope_cos = dbg.data_ptr()  # unused by the generic epilogue: carries the stamp buffer
        return orig(argp, stream)
    L.f3r_gemm = patched
    try:
        for _ in range(3):
            ops.gemm(a, w, bias=bias, act=act, out_lp=olp, kernel_sel=16 + bits)
        torch.cuda.synchronize()
        ms = time_ms(lambda: ops.gemm(a, w, bias=bias, act=act, out_lp=olp, kernel_sel=16 + bits), rounds=3, inner=3)[0]
    finally:
        L.f3r_gemm = orig
    d = dbg.cpu().double()
    t0 = d[:, 0].min()
    span = (d[:, 4].max() - t0).item()
    seg = [(d[:, i + 1] - d[:, i]).mean().item() for i in range(4)]
    tot = (d[:, 4] - d[:, 0]).mean().item()
    rounds = -(-tiles // 256)
    print(json.dumps({"kernel": "gemm256_lab stamps", "bits": bits, "M": M, "N": N, "K": K, "act": act, "ms": round(ms, 3), "tiles": tiles, "rounds_of_256": rounds,
                      "ticks_kernel_span": span, "ticks_per_tile_mean": tot, "prologue": seg[0], "main_loop": seg[1], "epilogue_issue": seg[2],
                      "store_retire": seg[3], "ticks_per_us": round(span / (ms * 1e3), 1),
                      "frac": {k: round(v / tot, 3) for k, v in zip(("prologue", "main_loop", "epilogue_issue", "store_retire"), seg)}}), flush=True)


def bench_qkv(dt, M, D, seq, sels=(1, 2, 3)):
    a = torch.randn((M, D), device=DEV).to(dt)
    w = ops.pack_linear_weight(torch.randn((3 * D, D), device=DEV) * D ** -0.5, dt)
    bias = torch.randn(3 * D, device=DEV)
    q = torch.empty((M, D), dtype=dt, device=DEV)
    k = torch.empty((M, D), dtype=dt, device=DEV)
    vt = torch.empty((M // seq, D, seq), dtype=dt, device=DEV)
    cos, sin = ops.rope_tables(32, 100.0, DEV)
    all_sels = sels
    for rope in (None, (cos, sin, 32)):
        fns = {}
        sels = [x for x in all_sels if not (x == 6 and rope is not None)]  # the hand-scheduled kernels take QKV without rotary embedding only
        for sel in sels:
            def f(sel=sel):
                ops.gemm_qkv(a, w, bias, q, k, vt, seq, rope, kernel_sel=sel)
            f()
            fns[sel] = f
        res_ms = {sel: [] for sel in sels}
        for _ in range(3):
            for sel in sels:
                res_ms[sel].append(time_ms(fns[sel], rounds=3, inner=3)[0])
        for sel in sels:
            ms = sorted(res_ms[sel])[1]
            print(json.dumps({"kernel": "gemm_qkv", "variant": SEL_NAME[sel], "rope": rope is not None, "dtype": str(dt).split(".")[-1], "M": M, "seq": seq,
                              "ms": round(ms, 3), "tflops": round(2.0 * M * 3 * D * D / ms / 1e9, 1)}), flush=True)


def bench_conv(dt, B, H, W, Ci, Co, name, stride=1, sels=(1, 2, 3), split=None):
    x = torch.randn((B, H, W, Ci), device=DEV).to(dt)
    x_lo = torch.randn((B, H, W, Ci), device=DEV).mul_(2.0 ** -11).to(dt) if split == "x3" else None
    w = ops.pack_conv3x3_weight(torch.randn((Co, Ci, 3, 3), device=DEV) * (9 * Ci) ** -0.5, dt, split=split is not None)
    bias = torch.randn(Co, device=DEV)
    oh, ow = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    r1 = torch.randn((B, oh, ow, Co), device=DEV).to(dt)
    cases = [("a_relu (round-1 form)", dict(a_relu=True, res_lp=r1), (1,))] if split is None else []
    cases.append(("skip + relu copy", dict(res_lp=r1, want_relu=True), tuple(s_ for s_ in sels if stride == 1 and Ci % 64 == 0 and Co % 128 == 0 or s_ == 1)))
    for cname, kw, csels in cases:
        fns = {}
        for sel in csels:
            def f(sel=sel, kw=kw):
                ops.conv3x3(x, w, stride=stride, bias=bias, kernel_sel=sel, split=split, x_lo=x_lo, **kw)
            f()
            fns[sel] = f
        res_ms = {sel: [] for sel in csels}
        for _ in range(3):
            for sel in csels:
                res_ms[sel].append(time_ms(fns[sel], rounds=3, inner=3)[0])
        mult = {None: 1, "w2": 2, "x3": 3}[split]
        for sel in csels:
            ms = sorted(res_ms[sel])[1]
            fl = 2.0 * B * oh * ow * 9 * Ci * Co
            print(json.dumps({"kernel": "conv3x3", "name": name, "case": cname, "variant": SEL_NAME[sel], "split": split, "dtype": str(dt).split(".")[-1], "B": B,
                              "HW": [H, W], "Ci": Ci, "Co": Co, "ms": round(ms, 3), "tflops_algorithmic": round(fl / ms / 1e9, 1),
                              "tflops_mfma": round(fl * mult / ms / 1e9, 1)}), flush=True)


def bench_dpt_final(n_views=25, H=512, W=512):
    """head[4] 1x1 conv + postprocess over one head chunk: algorithmic bytes = npix * (Cin * 2 [* 2 planes] + 16)."""
    for dt in (torch.bfloat16, torch.float16):
        for pair in (False, True):
            x = torch.randn((n_views, H, W, 128), device=DEV).to(dt)
            lo = (torch.randn((n_views, H, W, 128), device=DEV) * 2.0 ** -11).to(dt) if pair else None
            w, b = torch.randn(4, 128, device=DEV) * 0.1, torch.randn(4, device=DEV) * 0.1
            f = lambda: ops.dpt_final(x, w, b, ["exp", 1, float("inf")], x_lo=lo)
            f()
            ms = sorted(time_ms(f, rounds=3, inner=3)[0] for _ in range(3))[1]
            nbytes = n_views * H * W * (128 * 2 * (2 if pair else 1) + 16)
            print(json.dumps({"kernel": "dpt_final", "dtype": str(dt).split(".")[-1], "planes": 2 if pair else 1, "views": n_views, "ms": round(ms, 3),
                              "GBps_algorithmic": round(nbytes / ms / 1e6, 1)}), flush=True)


def bench_align(n_views=320, H=512, W=512, pct=85):
    """align_local_pts3d_to_global at the headline shape: HBM-bound.  Algorithmic bytes per view: conf 4 B x (6 radix passes + 1)
    + local/global points 2 x 12 B (moments) + local 12 B + out 12 B (apply) = 76 B per pixel."""
    import time
    from fast3r_amd import align_local_pts3d_to_global
    from oracle.align_oracle import align_local_pts3d_to_global as align_oracle
    g = torch.Generator().manual_seed(0)
    base = {"pts3d_local": torch.randn(1, H, W, 3, generator=g), "pts3d_in_other_view": torch.randn(1, H, W, 3, generator=g),
            "conf": 1 + torch.exp(torch.randn(1, H, W, generator=g))}
    base["conf_local"] = base["conf"]
    preds = [{k: v.cuda() + 0.001 * i for k, v in base.items()} for i in range(n_views)]
    views = [{} for _ in range(n_views)]

    def f():
        align_local_pts3d_to_global(preds, views, pct)
    f()
    med, mn = time_ms(f, rounds=3, inner=1)
    nbytes = n_views * H * W * 76.0
    t0 = time.perf_counter()
    align_oracle([{k: v.cpu() for k, v in preds[i].items()} for i in range(4)], views[:4], pct)
    cpu_s = (time.perf_counter() - t0) / 4
    print(json.dumps({"kernel": "align_local_to_global", "views": n_views, "HW": [H, W], "percentile": pct, "ms": round(med, 3),
                      "views_per_s": round(n_views / med * 1e3, 1), "GBps_algorithmic": round(nbytes / med / 1e6, 1),
                      "cpu_oracle_ms_per_view": round(cpu_s * 1e3, 1), "note": "ms includes torch.stack of the inputs (3 copies)"}), flush=True)


def bench_focal(n_views=320, H=512, W=512, pct=10):
    """estimate_focal at the headline shape.  Algorithmic bytes per pixel: conf 4 B x (6 radix passes + 1) + points 12 B + workspace
    16 B written once and read 100 times (L2-resident: 4 MB per view) = 1656 B; HBM-side only the first 56 B."""
    import time
    from fast3r_amd import estimate_focals
    from oracle import focal_oracle as FO
    g = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 1.5 + 3 * torch.rand(H, W, generator=g)
    pts1 = torch.stack([(xs - W / 2) * z / 400.0, (ys - H / 2) * z / 400.0, z], -1) + 0.01 * torch.randn(H, W, 3, generator=g)
    conf1 = 1 + 5 * torch.rand(H, W, generator=g)
    pts = pts1[None].repeat(n_views, 1, 1, 1).cuda() * (1 + 0.001 * torch.arange(n_views).view(-1, 1, 1, 1).cuda())
    conf = conf1[None].repeat(n_views, 1, 1).cuda()
    out = estimate_focals(pts, conf, min_conf_thr_percentile=pct)
    med, mn = time_ms(lambda: estimate_focals(pts, conf, min_conf_thr_percentile=pct), rounds=3, inner=1)
    t0 = time.perf_counter()
    ref = FO.estimate_focal(pts[:1].cpu(), conf[:1].cpu(), min_conf_thr_percentile=pct)
    cpu_s = time.perf_counter() - t0
    print(json.dumps({"kernel": "estimate_focal", "views": n_views, "HW": [H, W], "percentile": pct, "ms": round(med, 3),
                      "views_per_s": round(n_views / med * 1e3, 1), "L2_GBps": round(n_views * H * W * 1656.0 / med / 1e6, 1),
                      "focal_view0": float(out[0]), "cpu_oracle_focal_view0": ref, "cpu_oracle_ms_per_view": round(cpu_s * 1e3, 1)}), flush=True)


def bench_pnp(n_views=320, H=512, W=512):
    """estimate_poses at the headline shape: ~50 passes over 16 B per pixel (L2-resident, 4 MB per view) of fp64 per-point arithmetic."""
    import time
    from fast3r_amd import estimate_poses
    from oracle import pnp_oracle as PO
    g = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 2 + 3 * torch.rand(H, W, generator=g)
    Xc = torch.stack([(xs - W / 2) * z / 400.0, (ys - H / 2) * z / 400.0, z], -1)
    c, s_ = math.cos(0.3), math.sin(0.3)
    R = torch.tensor([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    t = torch.tensor([0.2, -0.1, 0.5])
    Xw = (Xc - t) @ R + 0.003 * torch.randn(H, W, 3, generator=g)
    conf1 = 1.001 + 4 * torch.rand(H, W, generator=g)
    pts = Xw[None].repeat(n_views, 1, 1, 1).cuda()
    conf = conf1[None].repeat(n_views, 1, 1).cuda()
    for mode, focal in (("focal given", 400.0), ("focal searched", None)):
        estimate_poses(pts, conf, focal)
        med, mn = time_ms(lambda: estimate_poses(pts, conf, focal), rounds=3, inner=1)
        P, F, I = estimate_poses(pts[:1], conf[:1], focal)
        t0 = time.perf_counter()
        fo, To = PO.fast_pnp(Xw, focal, conf1 > 1.0)
        cpu_s = time.perf_counter() - t0
        print(json.dumps({"kernel": "estimate_poses", "mode": mode, "views": n_views, "HW": [H, W], "ms": round(med, 3),
                          "views_per_s": round(n_views / med * 1e3, 1), "focal_view0": float(F[0]), "inliers_view0": int(I[0]),
                          "max_abs_diff_vs_cpu_restatement": float((P[0].double().cpu() - To).abs().max()),
                          "cpu_restatement_ms_per_view": round(cpu_s * 1e3, 1)}), flush=True)


def bench_loss(sizes=(100, 320), H=512, W=512, alpha=0.2, out_path="profiles/r08_loss_bench.jsonl"):
    """The validation criterion ConfLossMultiviewV2(Regr3DMultiviewV4(L21, "avg_dis"), alpha) at B = 1 with local heads, N views of H x W:
    the device-side criterion (f3r_loss.hip: two streaming passes) against a torch-eager fp32 restatement of the reference's steps
    (transform per view and frame, concatenate, NaN-fill, norm, nanmean, divide, boolean gathers, means) in the same run on the same GPU.
    Wall clock per call, synchronised, median of 5 after a warm-up; the launches alone by stream events; achieved bytes/s against the
    2 x 45 B per pixel the two passes must read.  One JSON line, also appended to profiles/."""
    import os
    import statistics
    import time
    from fast3r_amd import losses as L

    def wall_ms(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def eager(views, preds, inverses):
        """fp32, the reference's order of work for V4 / avg_dis / B = 1 (the 4 x 4 inverses are handed in: they are not what is measured)"""
        nan = float("nan")
        terms = []
        for local in (False, True):
            gts, prs, masks = [], [], []
            for v, (view, pred) in enumerate(zip(views, preds)):
                m = inverses[v] if local else inverses[0]
                gts.append(torch.einsum("bij,bhwj->bhwi", m[:, :3, :3], view["pts3d"]) + m[:, None, None, :3, 3])
                prs.append(pred["pts3d_local" if local else "pts3d_in_other_view"])
                masks.append(view["valid_mask"].clone())
            normed = []
            for pts_list in (prs, gts):
                if local:  # one factor per (sample, view)
                    out = []
                    for pts, valid in zip(pts_list, masks):
                        vp = pts.clone().view(pts.shape[0], -1, 3)
                        vp[valid.view(valid.shape[0], -1) == 0] = nan
                        f = vp.norm(dim=-1).nanmean(dim=-1).clip(min=1e-8)
                        out.append(pts / f[:, None, None, None])
                    normed.append(out)
                else:  # one factor per sample over all views
                    allp = torch.cat(pts_list, dim=1)
                    allp = allp.view(allp.shape[0], -1, 3)
                    allv = torch.cat(masks, dim=1).view(allp.shape[0], -1)
                    allp[allv == 0] = nan
                    f = allp.norm(dim=-1).nanmean(dim=-1).clip(min=1e-8)
                    normed.append([pts / f[:, None, None, None] for pts in pts_list])
            for v, (pr, gt, valid) in enumerate(zip(normed[0], normed[1], masks)):
                l = torch.norm(pr[valid] - gt[valid], dim=-1)
                c = preds[v]["conf_local" if local else "conf"][valid]
                terms.append((l * c - alpha * torch.log(c)).mean())
        return torch.stack(terms).sum() / len(terms)

    crit = L.ConfLossMultiviewV2(L.Regr3DMultiviewV4(L.L21, norm_mode="avg_dis"), alpha=alpha)
    rec = {"what": "loss", "device": torch.cuda.get_device_name(0), "B": 1, "HW": [H, W], "criterion": repr(crit), "alpha": alpha, "sizes": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)  # noqa: E731
    for n in sizes:
        views, preds = [], []
        for v in range(n):
            z = 1.0 + 3.0 * rnd(1, H, W)
            cam = torch.cat([(rnd(1, H, W, 2) - 0.5) * 1.2 * z[..., None], z[..., None]], dim=-1)
            a = 0.02 * v
            P = torch.tensor([[[math.cos(a), 0, math.sin(a), 0.01 * v], [0, 1, 0, 0], [-math.sin(a), 0, math.cos(a), 0], [0, 0, 0, 1]]], device=DEV)
            world = cam @ P[0, :3, :3].T + P[0, :3, 3]
            views.append({"pts3d": world, "valid_mask": rnd(1, H, W) >= 0.1, "camera_pose": P})
            preds.append({"pts3d_in_other_view": 1.4 * world + 0.02 * (rnd(1, H, W, 3) - 0.5), "conf": 1.0 + 4.0 * rnd(1, H, W) ** 2,
                          "pts3d_local": 0.7 * cam + 0.02 * (rnd(1, H, W, 3) - 0.5), "conf_local": 1.0 + 4.0 * rnd(1, H, W) ** 2})
        inverses = [torch.linalg.inv(view["camera_pose"].cpu()).to(DEV) for view in views]
        loss, _ = crit(views, preds)
        ref = eager(views, preds, inverses)
        crit_ms = wall_ms(lambda: crit(views, preds))
        eager_ms = wall_ms(lambda: float(eager(views, preds, inverses)), reps=3)
        lists = ([v["pts3d"] for v in views], [v["valid_mask"] for v in views], [v["camera_pose"] for v in views],
                 [p["pts3d_in_other_view"] for p in preds], [p["conf"] for p in preds], [p["pts3d_local"] for p in preds], [p["conf_local"] for p in preds])
        kernel_ms, kernel_best = time_ms(lambda: post_ops.mv_conf_loss(*lists, version=4, alpha=alpha), rounds=5, inner=3)
        must_read = 2 * 45 * n * H * W
        rec["sizes"][str(n)] = {"pixels_per_set": n * H * W, "criterion_call_ms": round(crit_ms, 3), "wrapper_and_launches_stream_ms": round(kernel_ms, 3),
                                "wrapper_and_launches_stream_best_ms": round(kernel_best, 3), "eager_fp32_restatement_ms": round(eager_ms, 3),
                                "eager_over_criterion": round(eager_ms / crit_ms, 2), "bytes_2x45_per_pixel": must_read,
                                "achieved_TB_per_s_of_stream_time": round(must_read / (kernel_ms * 1e-3) / 1e12, 3),
                                "loss": float(loss), "eager_loss": float(ref), "rel_diff_vs_eager_fp32": abs(float(loss) - float(ref)) / abs(float(ref))}
        del views, preds, lists, inverses
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def bench_scene(sizes=(100, 320), H=512, W=512, out_path="profiles/r09_scene_bench.jsonl", sort_only=False):
    """Scene assembly (fast3r_amd/scene.py, f3r_scene.hip) at N views of H x W, both heads, B = 1, poses=False (the pose solve is an
    existing stage and is timed elsewhere).  Wall clock, synchronised, every shape warmed up, medians with min / max:
    * `assemble_scene` on device-resident inputs, alternating call by call with a torch-eager restatement of the same steps on the same GPU
      (one batched torch.sort(stable, descending) over the (2 N, H W) confidences, batched gathers, the colour arithmetic, the extrema, and
      one torch.sort per axis for the extent's order statistics): the library composition at its best, since the views here share one size;
    * `assemble_scene` on host inputs as `inference()` returns them (uploads included);
    * `collect_points` (both heads, 10th percentile, sky mask on) and `generate_ply_bytes` (packing + one pinned copy) separately;
    * f3r_scene_sort alone by stream events, with the bytes per key it must move (29 B read + 27 B written) over that time;
    * tests/scene_ref.py (numpy, this machine's CPU) on 8 views, scaled to N: a CPU time, reported as such.
    sort_only: just a few f3r_scene_sort calls at the first size, for a profiler run of its own.  One JSON line, appended to profiles/."""
    import os
    import statistics
    import time
    import numpy as np
    import fast3r_amd
    from fast3r_amd import scene as S
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import scene_ref as R

    def once_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "n": len(ts)}

    lut = torch.from_numpy(S.turbo_lut_u8().copy()).to(DEV)

    def eager(preds, views, masks):
        n, L = len(preds), H * W
        conf = torch.stack([p["conf"].reshape(L) for p in preds] + [p["conf_local"].reshape(L) for p in preds])
        pts = torch.stack([p["pts3d_in_other_view"].reshape(L, 3) for p in preds] + [p["pts3d_local_aligned_to_global"].reshape(L, 3) for p in preds])
        img = torch.stack([v["img"].reshape(3, L) for v in views])
        mask = torch.stack([m.reshape(L) for m in masks])
        sconf, order = torch.sort(conf, dim=1, descending=True, stable=True)
        spts = torch.gather(pts, 1, order[:, :, None].expand(-1, -1, 3))
        order_v = order.view(2, n, L)
        rgb = torch.stack([((torch.gather(img, 2, order_v[h][:, None, :].expand(-1, 3, -1)) + 1) * 127.5).to(torch.uint8).transpose(1, 2) for h in range(2)])
        smask = torch.stack([torch.gather(mask, 1, order_v[h]) for h in range(2)])
        lo, hi = sconf[:, -1:], sconf[:, :1]
        x = (sconf - lo) / (hi - lo + 1e-8) * 256
        ccol = lut[torch.where(x >= 256, torch.full_like(x, 255), x).long().clamp_(0, 255)]
        max_conf = conf[:n].amax(dim=1).cpu()
        sky = smask[0].float().mean(dim=1).cpu()
        allp = pts[:n].reshape(-1, 3)
        m = allp.shape[0]
        ks = sorted({k for pct in (20, 80) for k in S.percentile_indexes(m, pct)[:2]})
        ext = torch.sort(allp, dim=0).values[ks].cpu()   # one sort per axis (torch.kthvalue takes 137 ms per call at 26 M values: 40 x this)
        return order.to(torch.int32), sconf, spts, rgb, smask, ccol, max_conf, sky, ext

    rec = {"what": "scene", "device": torch.cuda.get_device_name(0), "B": 1, "HW": [H, W], "tile": _lib.SCENE_TILE, "sizes": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)  # noqa: E731
    for n in sizes:
        preds, views, masks = [], [], []
        for v in range(n):
            preds.append({"pts3d_in_other_view": rnd(1, H, W, 3) * 4 - 2, "pts3d_local_aligned_to_global": rnd(1, H, W, 3) * 4 - 2,
                          "conf": 1.0 + 20.0 * rnd(1, H, W) ** 2, "conf_local": 1.0 + 20.0 * rnd(1, H, W) ** 2})
            views.append({"img": rnd(1, 3, H, W) * 2 - 1})
            masks.append((rnd(H, W) < 0.8).to(torch.int8))
        keys = 2 * n * H * W
        flat = lambda k, tail: [p[k].reshape(*tail) for p in preds]  # noqa: E731
        seg = (flat("conf", (H * W,)) + flat("conf_local", (H * W,)), flat("pts3d_in_other_view", (H * W, 3)) + flat("pts3d_local_aligned_to_global", (H * W, 3)),
               [v["img"].reshape(3, H * W) for v in views] * 2, [m.reshape(-1) for m in masks] * 2)
        if sort_only:
            for _ in range(3):
                post_ops.scene_sort(*seg, lut)
            torch.cuda.synchronize()
            return
        product = lambda: fast3r_amd.assemble_scene(preds, views, not_sky=masks, poses=False)  # noqa: E731
        once_ms(product)
        once_ms(lambda: eager(preds, views, masks))
        tp, te = [], []
        for _ in range(5):   # alternating
            tp.append(once_ms(product)[0])
            te.append(once_ms(lambda: eager(preds, views, masks))[0])
            torch.cuda.empty_cache()
        sort_ms, sort_best = time_ms(lambda: post_ops.scene_sort(*seg, lut), rounds=5, inner=1)
        conf_all = torch.stack(seg[0])
        torch_sort_ms, _ = time_ms(lambda: torch.sort(conf_all, dim=1, descending=True, stable=True), rounds=5, inner=1)
        del conf_all
        gpts = torch.cat(seg[1][:n])
        ranks = sorted({k for pct in (20, 80) for k in S.percentile_indexes(gpts.shape[0], pct)[:2]})
        extent_ms, _ = time_ms(lambda: post_ops.scene_extent_stats(gpts, (ranks * 4)[:4]), rounds=5, inner=1)
        del gpts
        sc = product()
        tc, tply = [], []
        collect = lambda: sc.collect_points(min_conf_thr_percentile=10, mask_sky=True, show_global=True, show_local=True)  # noqa: E731
        once_ms(collect)
        for _ in range(3):
            ms, (p, c) = once_ms(collect)
            tc.append(ms)
        once_ms(lambda: fast3r_amd.generate_ply_bytes(p, c))
        for _ in range(3):
            ms, ply = once_ms(lambda: fast3r_amd.generate_ply_bytes(p, c))
            tply.append(ms)
        n_points, ply_len = int(p.shape[0]), len(ply)
        del sc, p, c, ply
        torch.cuda.empty_cache()
        host = {"preds": [{k: v.cpu() for k, v in pr.items()} for pr in preds], "views": [{k: v.cpu() for k, v in vw.items()} for vw in views]}
        host_masks = [m.cpu() for m in masks]
        th = []
        once_ms(lambda: fast3r_amd.assemble_scene(host, not_sky=host_masks, poses=False))
        for _ in range(2):
            th.append(once_ms(lambda: fast3r_amd.assemble_scene(host, not_sky=host_masks, poses=False))[0])
        # the numpy restatement on this machine's CPU: 8 views, scaled to n
        lut_np = S.turbo_lut_u8()
        t0 = time.perf_counter()
        frames = []
        for i in range(8):
            pred = {k: v[0].numpy() for k, v in host["preds"][i].items()}
            frames.append(R.frame_data(pred, {"img": host["views"][i]["img"][0].numpy()}, host_masks[i].numpy(), i, 8, 1.5, lut_np))
        R.scene_extent([f["sorted_pts3d_global"] for f in frames])
        cpu8_ms = (time.perf_counter() - t0) * 1e3
        must = 56 * keys
        p_med, e_med = statistics.median(tp), statistics.median(te)
        rec["sizes"][str(n)] = {
            "keys": keys, "assemble_scene_device_inputs": stats(tp), "eager_torch_restatement": stats(te), "eager_over_product": round(e_med / p_med, 3),
            "f3r_scene_sort_stream_ms": round(sort_ms, 3), "f3r_scene_sort_stream_best_ms": round(sort_best, 3), "torch_sort_alone_stream_ms": round(torch_sort_ms, 3),
            "f3r_scene_extent_stream_ms": round(extent_ms, 3), "bytes_must_move_per_key": 56,
            "sort_TB_per_s_of_must_move_bytes": round(must / (sort_ms * 1e-3) / 1e12, 3), "assemble_scene_host_inputs": stats(th),
            "collect_points": stats(tc), "collected_points": n_points, "generate_ply_bytes": stats(tply), "ply_bytes": ply_len,
            "cpu_numpy_restatement_8_views_ms": round(cpu8_ms, 1), "cpu_numpy_restatement_scaled_to_n_ms": round(cpu8_ms * n / 8, 1),
            "cpu_scaled_over_product": round(cpu8_ms * n / 8 / p_med, 1)}
        del preds, views, masks, host, host_masks, seg, frames
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def bench_sky(sizes=(100, 320), H=512, W=512, out_path="profiles/r10_sky_bench.jsonl", detect_only=False):
    """Sky detection (fast3r_amd/sky.py, f3r_sky.hip) at N views of H x W generated on the device: a procedural outdoor set (blue sky with
    noise above a horizon that differs per view, ground colours below, a lake) and a uniform-noise set, the labelling's bad case.  Per set:
    * `detect_sky_planes` alone (what `assemble_scene(not_sky="detect")` calls: no read-back), wall clock and stream time, with the bytes
      the stage must move whatever the method (12 B read + 1 B written per pixel) over that time;
    * `assemble_scene(not_sky="detect")` against `assemble_scene(not_sky=None)`, alternating call by call, poses=False;
    * two CPU times on this machine, 8 views scaled to N: tests/sky_ref.py (numpy boolean box filters + scipy's labelling), and the
      reference's own steps through the stand-in tests/cv2_sky_stub.py (its uint8 cvtColor / inRange / dilate / morphologyEx, then
      sky_ref's labelling and rule);
    * at the first size the labelling alone (`F3R_SKY_LABEL` on a caller's bitmaps) on N one-pixel spirals, its longest parent chains,
      next to N bitmaps of 50 % noise.
    detect_only: a few detection calls at the first size, for a profiler run of its own.  One JSON line, appended to profiles/."""
    import os
    import statistics
    import time
    import fast3r_amd
    from fast3r_amd import sky as K
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import numpy as np
    import cv2_sky_stub as CV
    import sky_cases as C
    import sky_ref as R

    def once_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def cpu_through_stand_in(img):
        """the reference's steps with the stand-in's uint8 calls in place of cv2's, then sky_ref's labelling and rule"""
        hsv = CV.cvtColor(CV.cvtColor(R.to_u8(img), CV.COLOR_RGB2BGR), CV.COLOR_BGR2HSV)
        mask = (CV.inRange(hsv, [105, 50, 140], [135, 255, 255]) | CV.inRange(hsv, [95, 5, 150], [145, 100, 255])
                | CV.inRange(hsv, [0, 0, 235], [180, 10, 255]))
        upper = int(img.shape[0] * 0.4)
        mask[:upper] |= ((hsv[:upper, :, 1] < 50) & (hsv[:upper, :, 2] > 150)).astype(np.uint8)
        k = np.ones((7, 7), np.uint8)
        mask = CV.morphologyEx(CV.dilate(mask, k, iterations=1), CV.MORPH_OPEN, k)
        sky, _ = R.select(mask != 0)
        return (~sky).astype(np.int8)

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "n": len(ts)}

    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)  # noqa: E731

    def outdoor(v):
        u = torch.empty(3, H, W, device=DEV)
        horizon = int(H * (0.3 + 0.3 * ((v * 37) % 11) / 10))
        sky_c = torch.tensor([100.0, 150.0, 230.0], device=DEV)[:, None, None]
        ground = torch.tensor([[70.0, 110.0, 50.0], [110.0, 90.0, 60.0]], device=DEV)[v % 2][:, None, None]
        u[:, :horizon] = sky_c + (rnd(3, horizon, W) * 12 - 6)
        u[:, horizon:] = ground + (rnd(3, H - horizon, W) * 60 - 30)
        y0 = min(H - 40, horizon + 60)
        u[:, y0:y0 + 30, W // 5:W // 2] = sky_c + (rnd(3, 30, W // 2 - W // 5) * 12 - 6)
        return ((u.clamp_(0, 255).floor_() / 255 - 0.5) / 0.5)[None]

    rec = {"what": "sky", "device": torch.cuda.get_device_name(0), "B": 1, "HW": [H, W], "sizes": {}}
    for n in sizes:
        row = {}
        for kind in ("outdoor", "noise"):
            views = [{"img": outdoor(v) if kind == "outdoor" else rnd(1, 3, H, W) * 2 - 1} for v in range(n)]
            planes = [v["img"][0].reshape(3, H * W) for v in views]
            shapes = [(H, W)] * n
            detect = lambda: K.detect_sky_planes(planes, shapes)  # noqa: E731
            once_ms(detect)
            if detect_only:
                for _ in range(3):
                    detect()
                torch.cuda.synchronize()
                continue
            preds = [{"pts3d_in_other_view": rnd(1, H, W, 3) * 4 - 2, "pts3d_local_aligned_to_global": rnd(1, H, W, 3) * 4 - 2,
                      "conf": 1.0 + 20.0 * rnd(1, H, W) ** 2, "conf_local": 1.0 + 20.0 * rnd(1, H, W) ** 2} for _ in range(n)]
            with_detect = lambda: fast3r_amd.assemble_scene(preds, views, not_sky="detect", poses=False)  # noqa: E731
            without = lambda: fast3r_amd.assemble_scene(preds, views, not_sky=None, poses=False)  # noqa: E731
            once_ms(with_detect)
            once_ms(without)
            td, ta, tn = [], [], []
            for _ in range(5):   # alternating
                td.append(once_ms(detect)[0])
                ta.append(once_ms(with_detect)[0])
                tn.append(once_ms(without)[0])
            stream_ms, stream_best = time_ms(detect, rounds=5, inner=1)
            st = K.stats_dicts(detect()[1])
            sc = with_detect()
            # the numpy restatement on this machine's CPU: 8 views, scaled to n
            host = [views[i]["img"][0].permute(1, 2, 0).contiguous().cpu().numpy() for i in range(8)]
            t0 = time.perf_counter()
            want = [R.detect_sky_mask(img)[0] for img in host]
            cpu8_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            want_cv = [cpu_through_stand_in(img) for img in host]
            cpu8_cv_ms = (time.perf_counter() - t0) * 1e3
            masks = detect()[0]
            assert all(np.array_equal(masks[i].cpu().numpy(), want[i]) and np.array_equal(want[i], want_cv[i]) for i in range(8))
            must = 13 * n * H * W
            d_med, a_med, n_med = statistics.median(td), statistics.median(ta), statistics.median(tn)
            row[kind] = {
                "pixels": n * H * W, "detect_sky_planes": stats(td), "detect_stream_ms": round(stream_ms, 3), "detect_stream_best_ms": round(stream_best, 3),
                "bytes_must_move_per_pixel": 13, "detect_TB_per_s_of_must_move_bytes": round(must / (stream_ms * 1e-3) / 1e12, 3),
                "assemble_scene_detect": stats(ta), "assemble_scene_none": stats(tn), "detect_over_none": round(a_med / n_med, 3),
                "added_ms": round(a_med - n_med, 3), "is_outdoor": bool(sc.is_outdoor),
                "mean_components": round(sum(s["components"] for s in st) / n, 1), "mean_sky_fraction": round(sum(s["sky_pixels"] for s in st) / (n * H * W), 3),
                "branches": {b: sum(s["branch"] == b for s in st) for b in ("empty", "no_top", "top")},
                "cpu_numpy_restatement_8_views_ms": round(cpu8_ms, 1), "cpu_numpy_restatement_scaled_to_n_ms": round(cpu8_ms * n / 8, 1),
                "cpu_scaled_over_detect": round(cpu8_ms * n / 8 / d_med, 1),
                "cpu_stand_in_8_views_ms": round(cpu8_cv_ms, 1), "cpu_stand_in_scaled_to_n_ms": round(cpu8_cv_ms * n / 8, 1),
                "first_8_masks_equal_both_cpu_paths": True}
            del preds, views, planes, sc, masks
            torch.cuda.empty_cache()
        if detect_only:
            return
        if n == sizes[0]:   # the labelling alone: its longest chains (one-pixel spirals) next to 50 % noise
            lab = {}
            for kind, bm in (("spiral", torch.from_numpy(C.spiral(H, W).astype(np.int8)).to(DEV)), ("noise50", None)):
                src = [bm.clone() if bm is not None else (rnd(H, W) < 0.5).to(torch.int8) for _ in range(n)]
                label = lambda: post_ops.sky_detect(src, [(H, W)] * n, _lib.F3R_SKY_LABEL, want_not_sky=True, want_roots=False)  # noqa: E731
                once_ms(label)
                ms, best = time_ms(label, rounds=5, inner=1)
                lab[kind] = {"label_stream_ms": round(ms, 3), "label_stream_best_ms": round(best, 3),
                             "set_pixels_per_view": int(src[0].sum().item()), "components_view0": int(label()["stats"][0, 1].item())}
                del src
            row["labelling_alone"] = lab
        rec["sizes"][str(n)] = row
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def bench_cloud(sizes=(100, 320), H=512, W=512, max_num_points=1_000_000, out_path="profiles/r11_cloud_bench.jsonl"):
    """Point-cloud export (fast3r_amd/cloud.py, f3r_cloud.hip) at N views of H x W generated on the device, percentile 0, B = 1.  Every shape
    warmed up, medians of 5 calls with min / max:
    * combine: `post_ops.cloud_combine` with the thresholds handed in, wall clock (synchronised) and stream events, alternating call by
      call with a torch-eager restatement on the same GPU (one batched comparison, boolean gathers, the colour arithmetic);
    * voxel with max_num_points (the notebook's heuristic size): stream times of f3r_cloud_bounds, of f3r_cloud_voxel_sort whole and with
      a key of zero bits (keys, heads, scan and starts without any sort pass: the difference is the passes) and of f3r_cloud_voxel_sums;
      torch.unique(return_inverse) + index_add_ in fp64 beside it (unordered atomic sums: a speed yardstick only); tests/cloud_ref.py on
      this machine's CPU at the first size;
    * farthest point, tiled: stream time per iteration at n = 1 M and n = N H W points, the rate that n (12 + 16) bytes per iteration
      imply, and a torch-eager loop of the same step; the one-workgroup kernel per iteration at its largest n.
    One JSON line, appended to profiles/."""
    import ctypes
    import os
    import statistics
    import time
    import numpy as np
    from fast3r_amd import cloud
    from fast3r_amd.scene import percentile_indexes
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import cloud_ref as R

    def once_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "n": len(ts)}

    def events(fn, n=5):
        fn()
        ts = []
        for _ in range(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return stats(ts)

    def fps_eager(p, k):
        d = torch.full((p.shape[0],), float("inf"), dtype=torch.float64, device=DEV)
        far = torch.zeros((), dtype=torch.long, device=DEV)
        for _ in range(k):
            diff = p.double() - p[far].double()
            d = torch.minimum(d, (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2])
            far = torch.argmax(d)
        return far

    def fps_rates(p, k=17):
        n = p.shape[0]
        tiled = events(lambda: post_ops.cloud_fps(p, k, 0, _lib.F3R_FPS_TILED))
        eager = events(lambda: fps_eager(p, k - 1))
        per = tiled["median_ms"] / (k - 1)   # k selections are k - 1 distance updates
        return {"n": n, "iterations_timed": k - 1, "tiled_call": tiled, "tiled_ms_per_iteration": round(per, 4),
                "implied_GB_per_s_of_28_bytes_per_point": round(n * 28 / (per * 1e-3) / 1e9, 1), "eager_torch_loop": eager,
                "eager_ms_per_iteration": round(eager["median_ms"] / (k - 1), 4), "eager_over_tiled": round(eager["median_ms"] / tiled["median_ms"], 3)}

    rec = {"what": "cloud", "device": torch.cuda.get_device_name(0), "B": 1, "HW": [H, W], "percentile": 0, "max_num_points": max_num_points,
           "tiles": {"combine": _lib.CLOUD_TILE, "sort": _lib.CLOUD_SORT_TILE, "fps": _lib.CLOUD_FPS_TILE, "fps_one_max": _lib.CLOUD_FPS_ONE_MAX},
           "sizes": {}}
    g = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)  # noqa: E731
    L = H * W
    for pos, n in enumerate(sizes):
        conf = 1.0 + 20.0 * rnd(n, L) ** 2
        pts = torch.randn(n, L, 3, generator=g, device=DEV) * torch.tensor([4.0, 1.5, 3.0], device=DEV)   # an unbounded scene: most voxels of the box stay empty
        img = rnd(n, 3, L) * 2 - 1
        thr = conf.amin(dim=1)                                           # percentile 0: the minimum, handed to both sides
        ranks = [percentile_indexes(L, 0)] * n
        lists = ([conf[i] for i in range(n)], [pts[i] for i in range(n)], [img[i] for i in range(n)], [None] * n, [(H, W)] * n, ranks)
        product = lambda: post_ops.cloud_combine(*lists, thresholds=thr)  # noqa: E731

        def eager_combine():
            mask = conf > thr[:, None]
            col = ((img + 1.0) * 127.5).to(torch.uint8).transpose(1, 2)
            return pts[mask], col[mask]

        once_ms(product)
        once_ms(eager_combine)
        tp, te = [], []
        for _ in range(5):   # alternating
            tp.append(once_ms(product)[0])
            te.append(once_ms(eager_combine)[0])
        ev_p, ev_e = events(product), events(eager_combine)
        cp, cc = product()
        ep, ec = eager_combine()
        assert torch.equal(cp, ep) and torch.equal(cc, ec)
        del ep, ec, conf, img, lists
        torch.cuda.empty_cache()
        m = cp.shape[0]
        combine = {"points": m, "product_wall": stats(tp), "eager_wall": stats(te), "product_stream": ev_p, "eager_stream": ev_e,
                   "eager_over_product_wall": round(statistics.median(te) / statistics.median(tp), 3),
                   "eager_over_product_stream": round(ev_e["median_ms"] / ev_p["median_ms"], 3)}

        print(f"cloud: N = {n}: combine done ({m} points)", file=sys.stderr, flush=True)
        # ---- voxel
        lo, hi, bad = post_ops.cloud_bounds(cp)
        vs = cloud.heuristic_voxel_size(lo, hi, max_num_points)
        bits = cloud.voxel_key_bits(lo, hi, vs)
        l = _lib.lib()
        ws_bytes = l.f3r_cloud_voxel_workspace_bytes(m)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        nv = torch.empty(1, dtype=torch.int32, device=DEV)
        bout = torch.empty(8, dtype=torch.int32, device=DEV)
        mb = (ctypes.c_double * 3)(*lo)
        st = _lib.stream_ptr
        sort = lambda b: _lib.check(l.f3r_cloud_voxel_sort(_lib.ptr(cp), m, mb, vs, (ctypes.c_int * 3)(*b), _lib.ptr(ws), ws_bytes, _lib.ptr(nv), st()), "sort")  # noqa: E731
        t_bounds = events(lambda: _lib.check(l.f3r_cloud_bounds(_lib.ptr(cp), m, _lib.ptr(bout), st()), "bounds"))
        t_nosort = events(lambda: sort([0, 0, 0]))
        t_sort = events(lambda: sort(bits))
        n_vox = int(nv.item())
        op, oc = torch.empty((n_vox, 3), device=DEV), torch.empty((n_vox, 3), dtype=torch.uint8, device=DEV)
        ocnt = torch.empty(n_vox, dtype=torch.int32, device=DEV)
        t_sums = events(lambda: _lib.check(l.f3r_cloud_voxel_sums(_lib.ptr(cp), _lib.ptr(cc), m, n_vox, _lib.ptr(ws), ws_bytes, _lib.ptr(op), _lib.ptr(oc),
                                                                  _lib.ptr(ocnt), st()), "sums"))
        max_count = int(ocnt.max().item())
        del ws, op, oc, ocnt
        torch.cuda.empty_cache()
        whole = lambda: post_ops.cloud_voxel_down_sample(cp, cc, vs, (lo, hi, bad))  # noqa: E731

        def eager_voxel():
            p64 = cp.double()
            idx = torch.floor((p64 - (torch.tensor(lo, dtype=torch.float64, device=DEV) - 0.5 * vs)) / vs).long()
            key = (idx[:, 0] << (bits[1] + bits[2])) | (idx[:, 1] << bits[2]) | idx[:, 2]
            uniq, inv, cnt = torch.unique(key, return_inverse=True, return_counts=True)
            sp = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=DEV).index_add_(0, inv, p64)
            sc = torch.zeros((uniq.shape[0], 3), dtype=torch.float64, device=DEV).index_add_(0, inv, cc.double() / 255.0)
            c = cnt.double()[:, None]
            return (sp / c).float(), (sc / c * 255.0).to(torch.uint8), cnt

        once_ms(whole)
        once_ms(eager_voxel)
        tw, tev = [], []
        for _ in range(5):
            tw.append(once_ms(whole)[0])
            tev.append(once_ms(eager_voxel)[0])
        assert eager_voxel()[2].shape[0] == n_vox
        voxel = {"points": m, "voxel_size": vs, "key_bits": bits, "passes": cloud.voxel_sort_passes(bits), "voxels": n_vox, "largest_voxel": max_count,
                 "bounds_stream": t_bounds, "keys_heads_scan_starts_stream": t_nosort, "voxel_sort_whole_stream": t_sort,
                 "sort_passes_stream_ms": round(t_sort["median_ms"] - t_nosort["median_ms"], 3), "sums_stream": t_sums,
                 "voxel_down_sample_wall": stats(tw), "eager_unique_index_add_wall": stats(tev),
                 "eager_over_product_wall": round(statistics.median(tev) / statistics.median(tw), 3)}
        if pos == 0:   # the numpy restatement on this machine's CPU
            hp, hc = cp.cpu().numpy(), cc.cpu().numpy()
            t0 = time.perf_counter()
            ref = R.voxel_down_sample(hp, hc, vs)
            voxel["cpu_numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            voxel["cpu_over_product_wall"] = round(voxel["cpu_numpy_restatement_ms"] / statistics.median(tw), 1)
            got = whole()
            voxel["equals_cpu_restatement"] = bool(np.array_equal(got["points"].cpu().numpy(), ref[0]) and np.array_equal(got["colors"].cpu().numpy(), ref[1])
                                                   and np.array_equal(got["counts"].cpu().numpy(), ref[2]))
            del hp, hc, ref, got
        torch.cuda.empty_cache()

        print(f"cloud: N = {n}: voxel done ({n_vox} voxels)", file=sys.stderr, flush=True)
        # ---- farthest point
        fps = {"full_cloud": fps_rates(cp)}
        if pos == 0:
            fps["one_million"] = fps_rates(cp[:1_000_000].contiguous())
            small = cp[:_lib.CLOUD_FPS_ONE_MAX].contiguous()
            k1 = 257
            one = events(lambda: post_ops.cloud_fps(small, k1, 0, _lib.F3R_FPS_ONE))
            til = events(lambda: post_ops.cloud_fps(small, k1, 0, _lib.F3R_FPS_TILED))
            fps["one_workgroup"] = {"n": small.shape[0], "iterations_timed": k1 - 1, "call": one, "ms_per_iteration": round(one["median_ms"] / (k1 - 1), 5),
                                    "tiled_same_input_ms_per_iteration": round(til["median_ms"] / (k1 - 1), 5)}
        rec["sizes"][str(n)] = {"combine": combine, "voxel": voxel, "farthest_point": fps}
        del cp, cc, pts
        torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def bench_maps(n=320, H=512, W=512, host_views=8, out_path="profiles/maps_bench.jsonl"):
    """The map pictures (fast3r_amd/maps.py, f3r_maps.hip) at n views of H x W generated on the device, warmed up, medians of 7 with
    min / max.  Device time: stream events around 5 back-to-back `post_ops.maps_launch` calls on a table built before (the launches alone,
    the queue never empty), per call:
    * the n confidence maps (dense, 16-byte loads) into separate pictures, and into the cells of one contact sheet;
    * the z channel of n (H, W, 3) pointmaps read in place (element stride 3);
    * the n images (three planes each) in RGB mode;
    with the algorithmic bytes of each -- a map is read twice and written once: 12 bytes per pixel; the images are read once: 16 -- and
    the rate they imply.  Separately the host side: the whole `post_ops.maps_colorize` call on a wall clock (checks, table and upload for
    n maps, then the launches, synchronised); the sheet's device-to-host copy, and PNG encoding of `host_views` pictures on one
    thread (PIL, as `render._save_png`), and the path this replaces: `matplotlib.pylab.imsave(path, conf, cmap='turbo')` of the same
    `host_views` host maps on this machine's CPU, per view.  One JSON line, appended to profiles/."""
    import os
    import statistics
    import tempfile
    import time
    import numpy as np
    from fast3r_amd import maps, render

    def stats(ts):
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3), "n": len(ts)}

    def events(fn, rounds=7, inner=5):
        fn()
        ts = []
        for _ in range(rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) / inner)
        return stats(ts)

    def device_time(srcs, dsts, lut, mode, nbytes):
        plan = post_ops.maps_table(srcs, dsts, mode)
        return with_rate(events(lambda: post_ops.maps_launch(plan, lut)), nbytes)

    def with_rate(st, nbytes):
        return dict(st, algorithmic_bytes=nbytes, TB_per_s_at_median=round(nbytes / (st["median_ms"] * 1e-3) / 1e12, 3))

    g = torch.Generator(device=DEV).manual_seed(0)
    conf = 1.0 + 20.0 * torch.rand(n, H, W, generator=g, device=DEV) ** 2
    pts = torch.randn(n, H, W, 3, generator=g, device=DEV)
    img = torch.rand(n, 3, H, W, generator=g, device=DEV) * 2 - 1
    turbo, greys = maps._lut_on(conf.device, "turbo"), maps._lut_on(conf.device, "Greys")
    pictures = torch.empty((n, H, W, 4), dtype=torch.uint8, device=DEV)
    height, width, _, origins = maps.sheet_layout([(H, W)] * n)
    sheet = torch.zeros((height, width, 4), dtype=torch.uint8, device=DEV)
    cells = [sheet[y:y + H, x:x + W] for ((y, x),) in origins]
    px = n * H * W
    rec = {"what": "maps", "device": torch.cuda.get_device_name(0), "views": n, "HW": [H, W], "tile": _lib.MAPS_TILE,
           "conf_separate_pictures": device_time(list(conf), list(pictures), turbo, _lib.F3R_MAPS_LUT, 12 * px),
           "conf_into_sheet_cells": device_time(list(conf), cells, turbo, _lib.F3R_MAPS_LUT, 12 * px),
           "depth_channel_in_place": device_time(list(pts[..., 2]), list(pictures), greys, _lib.F3R_MAPS_LUT, 12 * px),
           "rgb_planes": device_time(list(img), list(pictures), None, _lib.F3R_MAPS_RGB, 16 * px)}
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        post_ops.maps_colorize(list(conf), cells, turbo)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    rec["conf_into_sheet_cells_wall_clock"] = stats(walls)
    t0 = time.perf_counter()
    host_sheet = sheet.cpu().numpy()
    rec["sheet_to_host_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    k = min(host_views, n)
    with tempfile.TemporaryDirectory() as tmp:
        enc = []
        for i in range(k):
            (y, x), = origins[i]
            a = np.ascontiguousarray(host_sheet[y:y + H, x:x + W])
            t0 = time.perf_counter()
            render._save_png(a, os.path.join(tmp, f"view_{i}_conf.png"))
            enc.append((time.perf_counter() - t0) * 1e3)
        rec["png_encode_per_view_one_thread"] = stats(enc)
        rec["png_workers"] = render.PNG_WORKERS
        try:
            from matplotlib import pylab
            host_conf = conf[:k].cpu().numpy()
            ims = []
            for i in range(k):
                t0 = time.perf_counter()
                pylab.imsave(os.path.join(tmp, f"imsave_{i}.png"), host_conf[i], cmap="turbo")
                ims.append((time.perf_counter() - t0) * 1e3)
            rec["matplotlib_imsave_per_view_cpu"] = stats(ims)
        except ImportError:
            rec["matplotlib_imsave_per_view_cpu"] = "not measured: matplotlib does not import here"
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def bench_posemetric(sizes=(320, 1500), H=512, W=512, out_path="profiles/r07_pose_metric_bench.jsonl"):
    """camera_pose_metrics (RRA / RTA / mAA from f3r_pose_pair_metrics) at B = 1 next to estimate_poses at the same view count in the same
    run: the metric stage is O(pairs) trigonometry on a few hundred kilobytes of poses and must stay below 5 % of the PnP stage.  Wall
    clock per call, synchronised (the metric call ends with the counts on the host), median of 7 after a warm-up; one JSON line, also
    appended to profiles/."""
    import os
    import statistics
    import time
    from fast3r_amd import camera_pose_metrics, estimate_poses
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import cam_pose_cases as C

    def wall_ms(fn, reps=7):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    g = torch.Generator().manual_seed(0)
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    z = 2 + 3 * torch.rand(H, W, generator=g)
    Xc = torch.stack([(xs - W / 2) * z / 400.0, (ys - H / 2) * z / 400.0, z], -1)
    c, s_ = math.cos(0.3), math.sin(0.3)
    R = torch.tensor([[c, 0, s_], [0, 1, 0], [-s_, 0, c]])
    Xw = (Xc - torch.tensor([0.2, -0.1, 0.5])) @ R + 0.003 * torch.randn(H, W, 3, generator=g)
    conf1 = 1.001 + 4 * torch.rand(H, W, generator=g)
    rec = {"what": "posemetric", "device": torch.cuda.get_device_name(0), "B": 1, "HW": [H, W], "sizes": {}}
    ok = True
    for n in sizes:
        pred, gt = (x.cuda()[None] for x in C.pose_set(n, 0))
        counts_ms = wall_ms(lambda: camera_pose_metrics(pred, gt))
        pairs_ms = wall_ms(lambda: post_ops.pose_pair_metrics(pred, gt, C.RRA_THRESHOLDS, C.RTA_THRESHOLDS, C.N_BINS, float(C.MAX_THRESHOLD), want_pairs=True)[0].cpu())
        kernel_ms, _ = time_ms(lambda: post_ops.pose_pair_metrics(pred, gt, C.RRA_THRESHOLDS, C.RTA_THRESHOLDS, C.N_BINS, float(C.MAX_THRESHOLD)), rounds=5, inner=10)
        pts = Xw[None].cuda().expand(n, H, W, 3).contiguous()
        conf = conf1[None].cuda().expand(n, H, W).contiguous()
        pnp_ms = wall_ms(lambda: estimate_poses(pts, conf, 400.0), reps=3)
        del pts, conf
        ratio = counts_ms / pnp_ms
        ok = ok and ratio < 0.05
        rec["sizes"][str(n)] = {"pairs": n * (n - 1) // 2, "metrics_counts_only_ms": round(counts_ms, 4), "metrics_with_pairs_ms": round(pairs_ms, 4),
                                "pair_kernel_launch_ms": round(kernel_ms, 4), "estimate_poses_focal_given_ms": round(pnp_ms, 3),
                                "counts_only_over_estimate_poses": round(ratio, 5)}
    rec["below_5_percent"] = ok
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "a") as f:
        f.write(line + "\n")


def bench_image(H=3000, W=4000, size=512, n=16):
    """load_images' per-pixel work at a 12 MP camera frame: PIL LANCZOS resize + crop + ImgNorm on the host vs upload + GPU."""
    import time
    import numpy as np
    from PIL import Image
    from fast3r_amd.image import img_norm_crop, resize_u8, _resized_size
    rng = np.random.default_rng(0)
    frame = (rng.random((H, W, 3)) * 255).astype(np.uint8)
    (nw, nh), interp = _resized_size((W, H), size)
    pil = Image.fromarray(frame)
    t0 = time.perf_counter()
    for _ in range(3):
        ref = np.asarray(pil.resize((nw, nh), Image.LANCZOS))
        x = (np.transpose(ref, (2, 0, 1)).astype(np.float32) / 255 - 0.5) / 0.5
    cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    cache = {}
    host = torch.from_numpy(frame).pin_memory()

    def f():
        u8 = host.to(DEV, non_blocking=True)
        r = resize_u8(u8, nw, nh, interp, cache)
        return img_norm_crop(r, (0, 0, nw - nw % 16, nh - nh % 16)), r
    out, r = f()
    assert np.array_equal(r.cpu().numpy(), ref)
    med, mn = time_ms(f, rounds=3, inner=n)
    u8 = host.to(DEV)
    med_k, _ = time_ms(lambda: resize_u8(u8, nw, nh, interp, cache), rounds=3, inner=n)
    print(json.dumps({"kernel": "load_images per-pixel work", "frame": [H, W], "to": [nh, nw], "gpu_ms_incl_upload": round(med, 3),
                      "gpu_ms_resize_only": round(med_k, 3), "resize_GBps": round((H * W * 3 + H * nw * 3 * 2 + nh * nw * 3) / med_k / 1e6, 1),
                      "pil_ms": round(cpu_ms, 1), "bit_exact_vs_pil": True}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="gemm,conv")
    ap.add_argument("--views", default="20,100")
    ap.add_argument("--attn-dtypes", default="bf16,fp16", help="attnproduct: which operand formats")
    ap.add_argument("--sels", default="1,2", help="attnsel: f3r_attn_args.kernel_sel values to time")
    ap.add_argument("--tokens-per-view", type=int, default=1024, help="attnsel: 768 = 384x512 images (an odd view count gives a partial last workgroup)")
    args = ap.parse_args()
    dt = torch.bfloat16
    if args.what == "gemmsmall":  # scenes of 3 - 40 views: which tile form fills 256 CUs best
        for M in (3072, 8192, 20480, 40960):
            bench_gemm(dt, M, 1024, 1024, f"proj+res M={M}", res=True, sels=(1, 2, 4))
            bench_gemm(dt, M, 1024, 4096, f"fc2+res M={M}", res=True, sels=(1, 2, 4))
            bench_gemm(dt, M, 4096, 1024, f"fc1+gelu M={M}", act="gelu", out="lp", sels=(1, 2, 4))
        sys.exit(0)
    if args.what == "gemmsmallw2":  # the same question for the product's W2 launches, with the hand-scheduled kernel (6) in the field: automatic (0) should be the fastest
        for M in [int(v) * 1024 for v in args.views.split(",")]:
            for sels in ((0, 6, 2, 4, 1),):
                bench_gemm(torch.float16, M, 1024, 1024, f"proj+res M={M}", res=True, sels=sels, split="w2")
                bench_gemm(torch.float16, M, 1024, 4096, f"fc2+res M={M}", res=True, sels=sels, split="w2")
                bench_gemm(torch.float16, M, 4096, 1024, f"fc1+gelu M={M}", act="gelu", out="lp", sels=sels, split="w2")
        sys.exit(0)
    if args.what == "attnproduct":
        for nv in [int(v) for v in args.views.split(",")]:
            for d in (args.attn_dtypes.split(",")):
                bench_attn_product({"bf16": torch.bfloat16, "fp16": torch.float16}[d], nv)
        sys.exit(0)
    if args.what == "gemmref":  # the transformer's GEMM roles at N = 320 beside the vendor library on the same data
        sels = tuple(int(x) for x in args.sels.split(","))
        for dt in (torch.float16, torch.bfloat16):
            for M in [int(v) * 1024 for v in args.views.split(",")]:
                for (n, k, nm, kw) in ((1024, 1024, "proj+res", dict(res=True)), (4096, 1024, "fc1+gelu", dict(act="gelu", out="lp")),
                                       (1024, 4096, "fc2+res", dict(res=True)), (4096, 1024, "fc1 plain lp", dict(out="lp"))):
                    bench_gemm(dt, M, n, k, f"{nm} M={M}", sels=sels, **kw)
                    bench_library_matmul(dt, M, n, k, f"{nm} M={M}")
                bench_qkv(dt, M, 1024, M, sels=sels)
                bench_library_matmul(dt, M, 3072, 1024, f"qkv M={M}")
        for M in [int(v) * 1024 for v in args.views.split(",")]:
            bench_gemm(torch.float16, M, 4096, 1024, f"fc1+gelu w2 M={M}", act="gelu", out="lp", split="w2", sels=sels)
            bench_gemm(torch.float16, M, 1024, 4096, f"fc2+res w2 M={M}", res=True, split="w2", sels=sels)
        sys.exit(0)
    if args.what == "attnsteal":  # the fusion attention (T = 1024 x views, 16 heads, fp16) with f3r_attn_args.sched_counter off / on, interleaved
        for nv in [int(x) for x in args.views.split(",")]:
            T, H = nv * 1024, 16
            q = (torch.randn((T, H * 64), device=DEV) * 0.2).half()
            k = torch.randn((T, H * 64), device=DEV).half()
            vt = torch.randn((H * 64, ops.vt_ld(T)), device=DEV).half()
            o = torch.empty_like(q)
            res = {False: [], True: []}
            ops.ATTN_COUNTERS = None
            for rnd_ in range(4):
                for steal in (False, True):
                    ops.ATTN_WORK_STEALING = steal
                    f = lambda: ops.attention(q, o, H, 1.0, [(k, vt, T, 0, 0)], q_prescaled=True, kernel_sel=2)  # noqa: E731
                    if rnd_ == 0:
                        f()
                    res[steal].append(time_ms(f, rounds=3, inner=1 if nv >= 100 else 8)[0])
            fl = 4.0 * T * T * 64 * H
            for steal in (False, True):
                ms = sorted(res[steal])[len(res[steal]) // 2]
                print(json.dumps({"kernel": "f3r_attn_asm_f16", "work_stealing": steal, "views": nv, "T": T, "ms": round(ms, 3), "tflops": round(fl / ms / 1e9, 1),
                                  "frac_of_peak": round(fl / ms / 1e9 / 2500.0, 4), "rounds_ms": [round(x, 3) for x in res[steal]]}), flush=True)
            ops.ATTN_WORK_STEALING = True
        sys.exit(0)
    if args.what == "gemmf8":  # the transformer's linear roles: two fp16 weight planes (W2, today) next to the low plane in fp8 (W2F8), hand-scheduled kernels
        f16 = torch.float16
        for M in [int(v) * 1024 for v in args.views.split(",")]:
            for (n, k, nm, kw) in ((4096, 1024, "fc1+gelu", dict(act="gelu", out="lp")), (1024, 4096, "fc2+res", dict(res=True)), (1024, 1024, "proj+res", dict(res=True)),
                                   (2048, 1024, "q|k lp", dict(out="lp"))):
                a16 = torch.randn((M, k), device=DEV).to(f16)
                rows = torch.empty((M, 3 * k // 2), dtype=f16, device=DEV)
                rows[:, :k] = a16
                rows.view(torch.uint8).view(M, 3 * k)[:, 2 * k:] = a16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
                w32 = torch.randn((n, k), device=DEV) * k ** -0.5
                w2 = ops.pack_linear_weight(w32, f16, split=True)
                w8, ws = ops.pack_linear_weight_f8(w32)
                bias = torch.randn(n, device=DEV)
                o32 = torch.randn((M, n), device=DEV) if kw.get("res") else None
                olp = torch.empty((M, n), dtype=f16, device=DEV) if kw.get("out") == "lp" else None
                common = dict(bias=bias, act=kw.get("act"), res_f32=o32, out_f32=o32, out_lp=olp)
                fns = {"w2 (two fp16 planes), skewed start": lambda: ops.gemm(rows[:, :k], w2, split="w2", kernel_sel=9, **common),
                       "w2 (two fp16 planes)": lambda: ops.gemm(rows[:, :k], w2, split="w2", kernel_sel=6, **common),
                       "w2f8 (low plane in fp8), skewed start": lambda: ops.gemm(rows, w8, split="w2f8", w_scale=ws, kernel_sel=9, **common),
                       "w2f8 (low plane in fp8)": lambda: ops.gemm(rows, w8, split="w2f8", w_scale=ws, **common)}
                res = {nm_: [] for nm_ in fns}
                for rnd_ in range(4):
                    for nm_, f in fns.items():
                        if rnd_ == 0:
                            f()
                        res[nm_].append(time_ms(f, rounds=3, inner=3)[0])
                base = None
                for nm_ in fns:
                    ms = sorted(res[nm_])[len(res[nm_]) // 2]
                    base = base or ms
                    print(json.dumps({"kernel": "gemm", "role": nm, "form": nm_, "M": M, "N": n, "K": k, "ms": round(ms, 3), "tflops_algorithmic": round(2.0 * M * n * k / ms / 1e9, 1),
                                      "speedup_vs_w2": round(base / ms, 3)}), flush=True)
        sys.exit(0)
    if args.what == "convheads":  # the DPT-head convolutions and the encoder's QKV + RoPE-2D as the N = 320 forward runs them (fp16, X3 / W2; 25-view head chunks)
        f16 = torch.float16
        bench_conv(f16, 25, 256, 256, 256, 128, "head0 x3", split="x3", sels=(0,))
        bench_conv(f16, 25, 512, 512, 128, 128, "head2 x3", split="x3", sels=(0,))
        bench_conv(f16, 25, 256, 256, 256, 256, "refinenet1 rcu x3", split="x3", sels=(0,))
        bench_conv(f16, 25, 128, 128, 256, 256, "refinenet2 rcu x3", split="x3", sels=(0,))
        bench_conv(f16, 25, 64, 64, 256, 256, "refinenet3 rcu x3", split="x3", sels=(0,))
        bench_qkv(f16, 128 * 1024, 1024, 1024, sels=(0,))
        sys.exit(0)
    if args.what == "gemmpersist":  # persistent grid (kernel_sel 2) next to one tile per workgroup (5) on the model's shapes
        for dt in (torch.bfloat16, torch.float16):
            for M in (40960, 102400, 327680):
                bench_gemm(dt, M, 1024, 1024, f"proj+res M={M}", res=True, sels=(2, 5))
                bench_gemm(dt, M, 4096, 1024, f"fc1+gelu M={M}", act="gelu", out="lp", sels=(2, 5))
                bench_gemm(dt, M, 1024, 4096, f"fc2+res M={M}", res=True, sels=(2, 5))
                bench_qkv(dt, M, 1024, M, sels=(2, 5))
            bench_conv(dt, 8, 128, 128, 256, 256, "refinenet1 rcu", sels=(2, 5))
            bench_conv(dt, 8, 256, 256, 256, 128, "head0", sels=(4,))
            bench_conv(dt, 8, 512, 512, 128, 128, "head2", sels=(4,))
        bench_gemm(torch.float16, 102400, 4096, 1024, "fc1+gelu w2", act="gelu", out="lp", split="w2", sels=(2, 5))
        bench_conv(torch.float16, 8, 128, 128, 256, 256, "refinenet1 rcu x3", split="x3", sels=(2, 5))
        sys.exit(0)
    if args.what == "exactattn":  # precision "exact": the FMA-pipe fp32 attention against its matrix-pipe form (three-plane products)
        for T in [int(x) * 1024 for x in args.views.split(",")]:
            H = 16
            qkv = (torch.randn((T, 3 * H * 64), device=DEV) * 1.2)
            res = {}
            for name, thr in (("fma", 1 << 62), ("mfma", 0)):
                if name == "fma" and T > 40960:
                    continue  # minutes
                ops.ATTN_F32_MFMA_MIN_KEYS = thr
                f = lambda: ops.attention_f32(qkv, H, 1, T, 0.125, torch.float16, want_f32=True)  # noqa: E731
                res[name] = f()[2]
                med, mn = time_ms(f, rounds=2, inner=1)
                print(json.dumps({"kernel": "attention_f32", "form": name, "T": T, "heads": H, "ms": round(med, 2), "tflops_algorithmic": round(4.0 * T * T * 64 * H / med / 1e9, 1)}), flush=True)
            if len(res) == 2:
                print(json.dumps({"kernel": "attention_f32", "T": T, "rel_l2_between_forms": float((res["mfma"] - res["fma"]).norm() / res["fma"].norm())}), flush=True)
        sys.exit(0)
    if args.what == "attnhdsmall":  # where the generated head_dim-80 / 128 kernels overtake the generic one: short sequences (sel 1 = generic, 2 = generated)
        for hd in (80, 128):
            for T in (128, 256, 512, 1024, 2048, 4096):
                bench_attn_head_dim(torch.float16, 0, hd, sels=(1, 2), T=T)
        sys.exit(0)
    if args.what == "attnhd":  # generic head_dim kernel next to the tuned head_dim-64 path
        for hd in (64, 80, 128):
            for nv in [int(x) for x in args.views.split(",")]:
                for d in args.attn_dtypes.split(","):
                    bench_attn_head_dim(torch.float16 if d == "fp16" else torch.bfloat16, nv, hd)
        sys.exit(0)
    if args.what == "attnsel":
        for nv in [int(x) for x in args.views.split(",")]:
            for d in (args.attn_dtypes.split(",")):
                bench_attn_sel({"bf16": torch.bfloat16, "fp16": torch.float16}[d], nv, sels=tuple(int(x) for x in args.sels.split(",")), tokens_per_view=args.tokens_per_view)
        sys.exit(0)
    if args.what == "labtime":
        M = 40 * 1024
        for bits in (128, 384, 640):
            bench_labtime(M, 4096, 1024, bits=bits)
            bench_labtime(M, 4096, 1024, act="gelu", bits=bits)
            bench_labtime(M, 1024, 4096, bits=bits)
            bench_labtime(8 * M, 4096, 1024, act="gelu", bits=bits)
        sys.exit(0)
    if args.what == "labphase":  # plain timing (no stamps): baseline / 2 phases / 4 phases
        M = 40 * 1024
        dt = torch.bfloat16
        for (m, n, k, act) in ((M, 4096, 1024, None), (M, 4096, 1024, "gelu"), (M, 1024, 1024, None), (M, 1024, 4096, None), (8 * M, 4096, 1024, "gelu"), (8 * M, 1024, 1024, None)):
            a = torch.randn((m, k), device=DEV).to(dt)
            w = ops.pack_linear_weight(torch.randn((n, k), device=DEV) * k ** -0.5, dt)
            bias = torch.randn(n, device=DEV)
            olp = torch.empty((m, n), dtype=dt, device=DEV)
            for bits in (0, 256, 512):
                f = lambda: ops.gemm(a, w, bias=bias, act=act, out_lp=olp, kernel_sel=16 + bits)
                f()
                ms = sorted(time_ms(f, rounds=3, inner=3)[0] for _ in range(3))[1]
                print(json.dumps({"kernel": "gemm256_lab dephase", "bits": bits, "M": m, "N": n, "K": k, "act": act, "ms": round(ms, 3),
                                  "tflops": round(2.0 * m * n * k / ms / 1e9, 1)}), flush=True)
        sys.exit(0)
    if "lab" in args.what:
        bench_lab(40 * 1024, 4096, 1024)
        bench_lab(40 * 1024, 1024, 4096)
        sys.exit(0)
    if "gemm" in args.what:
        M = 40 * 1024
        bench_gemm(dt, M, 1024, 1024, "proj+res", res=True)
        bench_gemm(dt, M, 4096, 1024, "fc1+gelu", act="gelu", out="lp")
        bench_gemm(dt, M, 1024, 4096, "fc2+res", res=True)
        bench_gemm(dt, M, 1024, 768, "patch_embed")
        bench_gemm(dt, 8 * M, 1024, 1024, "proj+res N=320", res=True)
        bench_gemm(dt, 8 * M, 4096, 1024, "fc1+gelu N=320", act="gelu", out="lp")
        bench_qkv(dt, M, 1024, 1024)
        bench_qkv(dt, M, 1024, M)
        bench_gemm(torch.float16, M, 1024, 1024, "proj+res w2", res=True, split="w2")
        bench_gemm(torch.float16, M, 4096, 1024, "fc1+gelu w2", act="gelu", out="lp", split="w2")
        bench_gemm(torch.float16, M, 1024, 1024, "proj+res x3", res=True, split="x3")
    if "dptfinal" in args.what:
        bench_dpt_final()
    if "focal" in args.what:
        bench_focal()
    if args.what == "loss":  # the validation criterion on the device next to a torch-eager restatement of the reference's steps
        bench_loss()
    if args.what == "scene":  # scene assembly and PLY export next to a torch-eager restatement and the numpy restatement on the CPU
        bench_scene()
        sys.exit(0)
    if args.what == "sky":  # sky detection alone and inside assemble_scene, next to the numpy restatement on the CPU
        bench_sky()
        sys.exit(0)
    if args.what == "cloud":  # point-cloud export: combine, voxel and farthest-point downsampling next to torch-eager and the CPU restatement
        bench_cloud(sizes=tuple(int(v) for v in args.views.split(",")) if args.views != "20,100" else (100, 320))
        sys.exit(0)
    if args.what == "skydetect":  # the detection kernels alone at N = 100 (both sets), for a profiler run of its own
        bench_sky(sizes=(100,), detect_only=True)
        sys.exit(0)
    if args.what == "scenesort":  # f3r_scene_sort alone at N = 100, for a profiler run of its own
        bench_scene(sizes=(100,), sort_only=True)
        sys.exit(0)
    if args.what == "maps":  # the map pictures: conf maps, the depth channel in place and the images, next to PNG encoding and matplotlib's imsave
        bench_maps(*(tuple(int(v) for v in args.views.split(","))[:1] if args.views != "20,100" else ()))
        sys.exit(0)
    if args.what == "posemetric":  # RRA / RTA / mAA over all view pairs next to the PnP stage that feeds it
        bench_posemetric()
        sys.exit(0)
    if "pnp" in args.what:
        bench_pnp()
    if "image" in args.what:
        bench_image()
    if "align" in args.what:
        bench_align()
    if "conv" in args.what:
        bench_conv(dt, 8, 128, 128, 256, 256, "refinenet1 rcu")
        bench_conv(dt, 8, 256, 256, 256, 128, "head0")
        bench_conv(dt, 8, 512, 512, 128, 128, "head2")
        bench_conv(dt, 8, 64, 64, 256, 256, "refinenet2 rcu")
        bench_conv(dt, 8, 32, 32, 768, 768, "act3 s2", stride=2)
        bench_conv(torch.float16, 8, 128, 128, 256, 256, "refinenet1 rcu x3", split="x3")
