"""Fast3R on MI355X: the reference's model API (fast3r/models/fast3r.py) executed by hand-written HIP kernels.

Drop-in surface kept from the reference (file:line = /root/reference/fast3r/models/fast3r.py):
  Fast3R(encoder_args, decoder_args, head_args, freeze="none")       :50-70
  Fast3R.forward(views, profiling=False) -> list[dict] | (list, dict) :302-497
  Fast3R.set_max_parallel_views_for_head(int)                         :298-300
  attributes encoder_args / decoder_args / head_args, .encoder / .decoder / .downstream_head[_local]
  state_dict(): identical keys and shapes, so `load_state_dict(ref.state_dict(), strict=True)`
  works, including the duplicated `scratch.layer_rn.{i}` aliases (croco/models/dpt_block.py:79-86).

What is different by design: torch.nn modules are used ONLY as parameter containers (names, shapes, device moves);
none of their forward() methods is ever called.  All arithmetic goes through fast3r_amd.ops -> libf3r_hip.so.  The
residual stream, LayerNorm statistics, softmax and post-processing are fp32; GEMM / conv / attention operands are
16-bit (`compute_dtype`, fp16 by default, bf16 selectable) with fp32 MFMA accumulation.  There is no CPU path.
"""
import math
import time
from collections import OrderedDict
from copy import deepcopy

from typing import NamedTuple, Optional

import numpy as np
import torch
import torch.nn as nn

from . import dpt_head, ops
from ._lib import F3RError
from .dist import ViewSharding, split_range
from .packing import _f32, _pack_block, _pack_dino_block, _pack_llama_block
from .params import (_ROPE_PERM, CroCoEncoder, DinoEncoder, Fast3RDecoder, LlamaDecoder, PixelwiseTaskWithDPT,  # noqa: F401  (re-exported)
                     sincos_1d_table)


# ======================================================================================= operand format
class OperandFormat(NamedTuple):
    """Which operand format every launch of a forward takes: derived from the model's knobs by Fast3R._format(), once per _pack / forward.
    The first five fields decide the packed bytes (pack_part: the weight-pack key); the whole record is part of the graph key."""
    lp: torch.dtype                  # compute_dtype: the 16-bit MFMA operand type
    planes: bool                     # split (hi + lo) weight planes and head activations: "high", "robust" and "exact"
    low_f8: bool                     # the MLP / QKV weights a second time with their low plane in fp8 (low_plane)
    fc1_planes: bool                 # fc1's weight as hi + lo planes (high_fc1_planes)
    head_f8: bool                    # the heads' 3x3 convolutions packed for, and run with, their corrections in fp8 (head_corrections)
    linear_split: Optional[str]      # split mode of the transformer's linear layers: weights only ("w2") in "high", both operands ("x3") in "robust" / "exact"
    x3: bool                         # both operands of every GEMM / conv as hi + lo planes (three MFMA products): "robust" and "exact"
    qk3: bool                        # "robust": the three-product attention kernels where a block can take them (Fast3R._qk3_ok) ...
    qk3_planes: int                  # ... with 3 (robust_corrections "fp8") or 2 planes per q / k row ...
    qk3_encoder: bool                # ... and also in the encoder's per-view attention (robust_encoder_attention "planes")
    head_f8_min_rows: int
    head_tail_fused_min_rows: int

    @property
    def pack_part(self):
        return self[:5]


def _fills_chip(rows, cols):
    """Do the 256 x 256 output tiles of a [rows][cols] GEMM fill the chip (256 CUs) at least once?"""
    return (rows // 256) * (cols // 256) >= 256


def _planes(fmt, x_f32):
    """fp32 -> (hi, lo) planes of the operand format; (lowp, None) in the formats without low planes."""
    if fmt.planes:
        return ops.cast_lp(x_f32, fmt.lp, want_lo=True)
    return ops.cast_lp(x_f32, fmt.lp), None


def _f8_gemms(pb, T, seq_len):
    """Which GEMMs of a block over T tokens take their low plane in fp8 (Fast3R.low_plane) -> (q | k, fc1, fc2)."""
    # the q | k launch with its low plane in fp8 (Fast3R.low_plane) where its 256 x 256 tiles fill the chip (from 8192 tokens on; the encoder's
    # RoPE-2D rides in that launch's epilogue since round 5), V^T on two fp16 planes; sequences must be multiples of 256 tokens for the V^T tiles
    qk = (pb.qk_w8 is not None and T % 256 == 0 and seq_len % 256 == 0 and pb.rope_mode == 0 and pb.q_dim == 0
          and _fills_chip(T, pb.qk_w8.shape[0]))
    # low plane in fp8 (Fast3R.low_plane): only the hand-scheduled 256 x 256-tile kernels read the [fp16 | fp8] rows, so a GEMM takes that form
    # when its tiles fill the chip at least once (256 CUs): fc1 (4 D wide) from 4096 tokens on, fc2 from 16 384; below that the scene is
    # launch- and occupancy-bound and the compiler-scheduled small-tile kernels win (N = 3: 118 us against 36 us per fc2, round-5 profile)
    fc1 = pb.fc1_w8 is not None and T % 256 == 0 and not pb.swiglu_hidden and _fills_chip(T, pb.fc1_w8.shape[0])
    return qk, fc1, fc1 and _fills_chip(T, pb.fc2_w8.shape[0])


# ======================================================================================= the model
class _GraphCache:
    """Captured forwards by scene shape (see Fast3R.enable_graphs); least-recently-used shapes are dropped beyond `max_entries`
    (every entry pins a private memory pool the size of a forward's activations)."""

    def __init__(self):
        self.max_views = 64
        self.max_entries = 8
        self.entries = OrderedDict()
        self.seen = set()

    def clear(self):
        self.entries.clear()
        self.seen.clear()

    def run(self, model, views, host_outputs=False):
        imgs = [v["img"] for v in views]
        dev = imgs[0].device
        shapes = {tuple(i.shape) for i in imgs}
        if len(views) > self.max_views or len(shapes) != 1 or any(i.dtype != torch.float32 for i in imgs):
            return None
        if model._orientation_plan(views)["any_portrait"]:  # also the eager path's argument checks (utils/misc.py:69), done on the host
            return None
        # (the whole operand format is part of the key: a graph captured with another low_plane / high_fc1_planes would keep replaying the old
        # packed weights after the model re-packed)
        key = (len(views), tuple(imgs[0].shape), str(dev), model.max_parallel_views_for_head, model.training, model._params_version(), model._format())
        dec = model.decoder
        B = imgs[0].shape[0]
        if key not in self.entries:
            if key not in self.seen:  # first sight of a shape: plain eager forward (also warms the packed weights / RoPE tables)
                self.seen.add(key)
                return None
            static_imgs = [torch.empty_like(i) for i in imgs]
            static_emb = torch.zeros((B, len(views), dec.embed_dim), dtype=torch.float32, device=dev)
            static_views = [{"img": t} for t in static_imgs]
            for t, i in zip(static_imgs, imgs):
                t.copy_(i)
            graph = torch.cuda.CUDAGraph()
            sched = torch.zeros(2, dtype=torch.int32, device=dev)   # this graph's own work-stealing pair (ops.sched_scope), allocated outside the capture
            torch.cuda.synchronize()
            with torch.cuda.graph(graph), ops.sched_scope(sched):
                outs = model._forward_eager(static_views, False, _emb_rows=static_emb)
            self.entries[key] = (graph, static_imgs, static_emb, outs, sched)
            while len(self.entries) > self.max_entries:
                self.entries.popitem(last=False)
        self.entries.move_to_end(key)
        graph, static_imgs, static_emb, outs, _sched = self.entries[key]
        for t, i in zip(static_imgs, imgs):
            t.copy_(i, non_blocking=True)
        ids = dec.draw_image_ids(B, len(views))
        static_emb.copy_(dec.image_idx_emb.to(dev)[ids.to(dev)])
        graph.replay()
        if host_outputs:  # inference(): the replayed (static) outputs go to the host through the same sink as the eager path's head chunks
            sink = _HostSink(dev, B)
            sink.push([(i, slice(None), k, v) for i, r in enumerate(outs) for k, v in r.items()], [])
            sink.finish()   # before the next replay may overwrite the static outputs
            return [{k: sink.result(i, k) for k in r} for i, r in enumerate(outs)]
        return [{k: v.clone() for k, v in r.items()} for r in outs]


try:  # the reference's loading API (fast3r.py:44-48): Fast3R.from_pretrained(repo id or local snapshot dir) / save_pretrained
    import huggingface_hub as _hf
    _HubMixin = _hf.PyTorchModelHubMixin
except Exception:  # pragma: no cover  (huggingface_hub is a requirement of the reference; without it only from_pretrained is missing)
    class _HubMixin:
        def __init_subclass__(cls, **kw):
            super().__init_subclass__()


class _HostSink:
    """Device -> host leg of `inference()` (fast3r/dust3r/inference_multiview.py:92-93 + utils/device.py:17-53 `to_cpu`): one pinned host
    tensor per (view, output) -- torch's caching host allocator recycles them between calls, and a tensor the caller still holds is
    never handed out again -- filled by non_blocking copies on a side stream that waits for the event recorded behind the head chunk that
    produced the data.  The copies of chunk c overlap the heads of chunk c + 1; finish() waits for the last one.

    The returned tensors are PAGE-LOCKED for as long as the caller holds them (~8.4 MB per view: 2.7 GB at N = 320).  PINNED_LIMIT_BYTES
    bounds what one call locks (default 8 GiB; 0 = never pin); past the limit, or when the host refuses a page-locked allocation, the
    remaining outputs land in ordinary pageable tensors (the copy is then synchronous, as the reference's `to_cpu` is) -- never an error."""
    PINNED_LIMIT_BYTES = 8 << 30

    def __init__(self, dev, batch):
        self.dev, self.B = dev, batch
        self.stream = torch.cuda.Stream(device=dev)
        self.bufs = {}
        self.pinned_bytes = 0
        self.pageable = 0   # outputs that fell back to pageable memory

    def _alloc(self, shape, dtype):
        nbytes = int(torch.empty((), dtype=dtype).element_size())
        for s_ in shape:
            nbytes *= int(s_)
        if self.pinned_bytes + nbytes <= self.PINNED_LIMIT_BYTES:
            try:
                t = torch.empty(shape, dtype=dtype, pin_memory=True)
                self.pinned_bytes += nbytes
                return t
            except RuntimeError:   # hipHostMalloc refused (locked-memory limit of the host / container): from here on, pageable
                self.PINNED_LIMIT_BYTES = 0
        self.pageable += 1
        return torch.empty(shape, dtype=dtype)

    def push(self, items, keep_alive):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        for t in keep_alive:
            if t is not None:
                t.record_stream(self.stream)  # the caching allocator must not recycle the chunk's tensors before the side stream has read them
        with torch.cuda.stream(self.stream):
            self.stream.wait_event(ev)
            for i, b, name, src in items:
                key = (i, name)
                if key not in self.bufs:
                    shape = tuple(src.shape) if isinstance(b, slice) else (self.B,) + tuple(src.shape)
                    self.bufs[key] = self._alloc(shape, src.dtype)
                self.bufs[key][b].copy_(src, non_blocking=True)   # (a pageable destination makes this copy synchronous: still correct)

    def result(self, i, name):
        return self.bufs[(i, name)]

    def finish(self):
        self.stream.synchronize()


# compute_dtype travels through config.json as text ("torch.float16"): the constructor accepts the string back
_DTYPE_CODER = {torch.dtype: (lambda d: str(d), lambda s_: getattr(torch, str(s_).replace("torch.", "")))}


class Fast3R(nn.Module, _HubMixin, repo_url="https://github.com/facebookresearch/fast3r", tags=["image-to-3d"], coders=_DTYPE_CODER):
    """`Fast3R.from_pretrained("jedyang97/Fast3R_ViT_Large_512")` (or a local directory holding config.json + model.safetensors) works as
    in the reference: the mixin reads the three *_args dicts from config.json, builds the model and loads the state dict (identical keys).

    Two arguments the reference does not have (both optional):
      compute_dtype   the 16-bit MFMA operand type (torch.float16 default, torch.bfloat16);
      precision       default "high" with fp16 operands: the one format that is within 1e-3 rel-L2 of the fp32 reference on EVERY
                      fixture, the stress fixture included (DESIGN.md section 3 (Precision modes)) -- what bench.py measures;
                      "fast": every GEMM / conv operand is ONE 16-bit number (within 1e-3 on default-init weights only).
                      "high": split-precision operands (f3r.h f3r_split) -- transformer weights as hi + lo planes (2 MFMA passes per
                      GEMM), both operands of the DPT heads as hi + lo planes (3 passes, activations kept as two planes in HBM);
                      attention unchanged.  With fp16 this brings the stress fixture inside 1e-3 of the fp32 reference (DESIGN.md
                      section 4, oracle/precision_study.py) at ~1.15x the time of "fast" at N=320.
                      "exact": what `inference(dtype="32")` means in the reference (no autocast): BOTH operands of every GEMM / conv as
                      hi + lo planes (~22 significand bits each, 3 MFMA passes), the attention core in plain fp32 (f3r_attn_f32).  A
                      validation mode for scenes of tens of views; CroCo / DINOv2 encoder + Fast3R decoder on one GPU only."""

    def __init__(self, encoder_args: dict, decoder_args: dict, head_args: dict, freeze="none",
                 compute_dtype: torch.dtype = torch.float16, precision: str = "high"):
        super().__init__()
        if isinstance(compute_dtype, str):  # config.json round trip stores the dtype as text
            compute_dtype = getattr(torch, compute_dtype.replace("torch.", ""))
        if precision not in ("fast", "high", "robust", "exact"):
            raise ValueError(f"precision must be 'fast', 'high', 'robust' or 'exact', got {precision!r}")
        self.encoder_args = dict(encoder_args)
        self.build_encoder(encoder_args)
        self.decoder_args = dict(decoder_args)
        self.build_decoder(decoder_args)
        self.head_args = dict(head_args)
        self.build_head(head_args)
        self.max_parallel_views_for_head = 25  # fast3r.py:68
        self.max_parallel_views_for_encoder = 128  # the reference chunks at 400 (fast3r.py:250); bounds the workspace
        self.compute_dtype = compute_dtype
        self.precision = precision
        self.sharding = None  # set by shard_views(): view-sharded multi-GPU execution (fast3r_amd/dist.py)
        self.debug_taps = None  # set to a dict to capture the lowp DPT inputs (hooks 0, L/2, 3L/4, L) per sample
        self.kv_tap = None  # callable(k, vt): sees every fusion layer's K [T][D] / V^T [D][ld] of an UNSHARDED forward (tests)
        self.use_graphs = False  # enable_graphs(): hipGraph replay of small scenes
        self._graphs = _GraphCache()
        self._packed = None
        self._rope_cache = {}
        self.weights_loaded = False   # load_state_dict / from_pretrained sets it: a checkpoint, not this constructor's default init
        self.calibration = None       # calibrate_precision()'s report: which precision tier THESE weights need for 1e-3
        self.set_freeze(freeze)

    # ---------------------------------------------------------------- construction (fast3r.py:72-157)
    def build_encoder(self, encoder_args):
        a = deepcopy(dict(encoder_args))
        kinds = {"croco": CroCoEncoder, "dino_v2": DinoEncoder}  # fast3r.py:80-83
        if a.pop("encoder_type") not in kinds:
            raise ValueError(f"Unsupported encoder type: {encoder_args['encoder_type']}")
        self.encoder = kinds[encoder_args["encoder_type"]](**a)

    def build_decoder(self, decoder_args):
        dt = decoder_args.get("decoder_type", "fast3r")
        self.decoder_args["decoder_type"] = dt
        kinds = {"fast3r": Fast3RDecoder, "llama": LlamaDecoder}
        if dt not in kinds:
            raise ValueError(f"Unsupported decoder type: {dt}")
        a = deepcopy(dict(decoder_args))
        a.pop("decoder_type", None)
        self.decoder = kinds[dt](**a)

    def build_head(self, head_args):
        self.output_mode, self.head_type = head_args["output_mode"], head_args["head_type"]
        self.depth_mode, self.conf_mode = head_args["depth_mode"], head_args["conf_mode"]
        mk = lambda: self.head_factory(head_args["head_type"], head_args["output_mode"], has_conf=bool(head_args["conf_mode"]),
                                       patch_size=head_args["patch_size"])
        self.downstream_head = mk()
        self.downstream_head_local = mk() if head_args.get("with_local_head", False) else None
        # transpose_to_landscape(head, activate=landscape_only) (fast3r.py:123-130, dust3r/utils/misc.py:61-106): see _orientation_plan
        self.landscape_only = bool(head_args.get("landscape_only", False))

    # `.head` / `.local_head` of the reference are closures over the two heads (utils/misc.py:61-106), not modules:
    # expose the names without registering the heads a second time (state_dict keys must not change).
    @property
    def head(self):
        return self.downstream_head

    @property
    def local_head(self):
        return self.downstream_head_local

    def head_factory(self, head_type, output_mode, has_conf=False, patch_size=16):
        if head_type == "dpt" and output_mode == "pts3d":
            assert self.decoder_args["depth"] > 9  # fast3r.py:137
            l2 = self.decoder_args["depth"]
            ed, dd = self.encoder_args["embed_dim"], self.decoder_args["embed_dim"]
            if tuple(self.head_args["depth_mode"])[0] not in ops.DEPTH_MODES:
                raise ValueError(f"bad mode={tuple(self.head_args['depth_mode'])[0]!r}")  # postprocess.py:51 (raised at the first forward there)
            if self.head_args["conf_mode"] and tuple(self.head_args["conf_mode"])[0] not in ops.CONF_MODES:
                raise ValueError(f"bad mode={tuple(self.head_args['conf_mode'])[0]!r}")   # :64
            return PixelwiseTaskWithDPT(num_channels=3 + has_conf, feature_dim=256, last_dim=128,
                                        hooks_idx=[0, l2 * 2 // 4, l2 * 3 // 4, l2], dim_tokens=[ed, dd, dd, dd],
                                        patch_size=patch_size, depth_mode=self.head_args["depth_mode"],
                                        conf_mode=self.head_args["conf_mode"])
        raise NotImplementedError(f"unexpected {head_type=} and {output_mode=}")  # fast3r.py:157

    def load_from_dust3r_checkpoint(self, dust3r_checkpoint_path):
        """fast3r.py:162-234: initialise from a DUSt3R checkpoint ({'model': state_dict}): `patch_embed.* | enc_blocks.* | enc_norm.*`
        go to `encoder.*`, `downstream_head1.*` to `downstream_head.*` (skipped with head_args['skip_load_pretrained_head'], and
        reverted if the shapes do not fit); everything else in the file is ignored.  Returns (loaded_keys, not_loaded_keys)."""
        checkpoint = torch.load(dust3r_checkpoint_path, weights_only=False)["model"]
        enc_sd, head_sd, loaded = {}, {}, set()
        for key, value in checkpoint.items():
            if key.startswith(("patch_embed", "enc_blocks", "enc_norm")):
                enc_sd["encoder." + key] = value
                loaded.add(key)
            elif key.startswith("downstream_head1"):
                head_sd[key.replace("downstream_head1", "downstream_head")] = value
                loaded.add(key)
        res = self.load_state_dict(enc_sd, strict=False)
        bad = set(res.unexpected_keys)
        loaded -= {k[len("encoder."):] for k in bad}
        if not self.head_args.get("skip_load_pretrained_head", False):
            backup = {k: v.clone() for k, v in self.downstream_head.state_dict().items()}
            try:
                res = self.load_state_dict(head_sd, strict=False)
                loaded -= {k.replace("downstream_head", "downstream_head1", 1) for k in res.unexpected_keys}
            except RuntimeError:  # size mismatch: keep the head as it was (:213-222)
                self.downstream_head.load_state_dict(backup)
                loaded -= {k for k in checkpoint if k.startswith("downstream_head1")}
        else:
            loaded -= {k for k in checkpoint if k.startswith("downstream_head1")}
        return loaded, set(checkpoint.keys()) - loaded

    def set_freeze(self, freeze):
        self.freeze = freeze
        todo = {"none": [], "encoder": [self.encoder], "sandwich": [self.encoder, self.downstream_head]}[freeze]
        for m in todo:
            for p in m.parameters():
                p.requires_grad = False

    def set_max_parallel_views_for_head(self, n):
        self.max_parallel_views_for_head = n

    def shard_views(self, process_group=None, exchange="allgather", p2p_channels=3, reserve_cus=32):
        """Enable the view-sharded multi-GPU path: this rank encodes / decodes / regresses only its contiguous range of
        views and exchanges K / V^T per fusion layer over RCCL (fast3r_amd/dist.py).  exchange: "allgather" (one collective per tensor
        and layer, one remote attention launch), "p2p" (pairwise rounds dealt onto p2p_channels communicators, one remote launch per
        arrived shard) or "auto" (three fusion layers with each on the first forward, then the one that exposed less)."""
        self.sharding = ViewSharding(process_group, exchange=exchange, p2p_channels=p2p_channels, reserve_cus=reserve_cus)
        return self

    def emulate_rank(self, rank, world, kv_source=None, exchange="allgather", reserve_cus=0):
        """ONE GPU runs exactly rank `rank`'s share of a `world`-rank view-sharded forward -- its views through the encoder, the fusion
        layers as local launch (parking the softmax state) + remote launch over world - 1 K / V^T segments, its heads -- with no
        collective (dist.EmulatedSharding).  kv_source fills the remote segments per layer (parity test); without it they hold random
        operands (bench.py --emulate-rank: a per-rank step time, clearly not a multi-GPU measurement).  `emulate_rank(None, 0)` undoes it."""
        from .dist import EmulatedSharding
        self.sharding = None if rank is None else EmulatedSharding(world, rank, kv_source, exchange=exchange)
        if self.sharding is not None:
            self.sharding.reserve_cus = int(reserve_cus)   # what ViewSharding.reserve_cus costs the local launch, measurable on one GPU
        return self

    # ---------------------------------------------------------------- packed weights
    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.invalidate_packed_weights()
        self.weights_loaded, self.calibration = True, None
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    # ---------------------------------------------------------------- which precision tier do these weights need?
    PRECISION_TIERS = ("fast", "high", "robust", "exact")   # cheapest first (N = 320: 8.3 / 8.9 / ~19 / 36 s on one MI355X)

    @torch.no_grad()
    def calibrate_precision(self, views, tol=1e-3, tiers=("fast", "high", "robust"), max_views=8, seed=1234):
        """Measure, on up to `max_views` of the caller's own views, how far every 16-bit operand tier is from the fp32-equivalent mode
        (precision="exact", 3e-7 of the reference on its golden outputs) WITH THE WEIGHTS THE MODEL HOLDS NOW, and say which tier to use.

        Why: the distance of a 16-bit tier to the fp32 reference depends on the checkpoint.  Default-init-like and N(0, 1 / fan_in) weights keep
        "high" (the default) within 3e-4; a noise-amplifying set (heavy-tailed weights, LayerNorm gains spread over a decade) measured 2.5e-3 with
        "high" and 3.6e-4 with "robust" (DESIGN.md section 3).  Nobody can test the released `Fast3R.from_pretrained("jedyang97/Fast3R_ViT_Large_512")`
        weights offline, so the model measures itself: ~2 s for 8 views of 512 x 512 at ViT-L size (the exact pass is most of it).

        Returns (and keeps in `self.calibration`) {"per_tier": {tier: {output: rel-L2 vs exact}}, "worst": {tier: max}, "recommended": the cheapest
        tier within `tol` (or "exact"), "tol", "n_views", ...}.  Does not change `self.precision`: set it from the answer, or pass
        `inference(..., dtype=...)` as before.  Reference context: fast3r/croco/models/blocks.py:158-190 (bf16 autocast there), README.md:84."""
        views = list(views)[:max(1, int(max_views))]
        if not views:
            raise ValueError("calibrate_precision needs at least one view")
        if self.sharding is not None:
            raise ValueError("calibrate_precision runs on one GPU: call it before shard_views()")
        dev = next(self.parameters()).device
        views = [dict(v, img=v["img"].to(dev)) for v in views]
        saved = (self.precision, self.use_graphs)
        rng = torch.get_rng_state()
        per_tier, ms = {}, {}
        try:
            self.use_graphs = False

            def run(p):
                self.precision = p
                torch.manual_seed(seed)   # the image ids consume the global CPU RNG (fast3r.py:702-743): the same ids for every tier
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                out = self._forward_eager(views)
                torch.cuda.synchronize(dev)
                ms[p] = (time.perf_counter() - t0) * 1e3
                return out
            ref = run("exact")
            for p in tiers:
                if p not in self.PRECISION_TIERS[:-1]:
                    raise ValueError(f"unknown precision tier {p!r}")
                out = run(p)
                worst = {}
                for o, r in zip(out, ref):
                    for k in r:
                        e = float((o[k].double() - r[k].double()).norm() / r[k].double().norm().clamp_min(1e-30))
                        worst[k] = max(worst.get(k, 0.0), e)
                per_tier[p] = worst
                del out
            del ref
        finally:
            self.precision, self.use_graphs = saved
            torch.set_rng_state(rng)
        worst = {p: max(v.values()) for p, v in per_tier.items()}
        order = [p for p in self.PRECISION_TIERS if p in worst]
        ok = [p for p in order if worst[p] <= tol and math.isfinite(worst[p])]
        self.calibration = dict(per_tier=per_tier, worst=worst, recommended=ok[0] if ok else "exact", tol=tol, n_views=len(views),
                                ms_incl_weight_packing=ms, compute_dtype=str(self.compute_dtype), params_version=self._params_version(),
                                checker="precision='exact' on the same views and weights")
        return self.calibration

    def precision_is_calibrated(self):
        """True when calibrate_precision() ran on the weights the model holds now and the tier in use is at least the recommended one."""
        c = self.calibration
        if c is None or c.get("params_version") != self._params_version():
            return False
        t = self.PRECISION_TIERS
        return t.index(self.precision) >= t.index(c["recommended"])

    def _apply(self, fn, *a, **k):
        self.invalidate_packed_weights()
        return super()._apply(fn, *a, **k)

    def invalidate_packed_weights(self):
        self._packed = self._packed_alt = None
        if getattr(self, "_graphs", None) is not None:
            self._graphs.clear()  # captured graphs hold pointers into the packed weights

    def _params_version(self):
        """Sum of the in-place version counters of all parameters: `p.copy_` under no_grad, a submodule's own load_state_dict or an
        optimizer step change it, so packed (device, 16-bit) weights and captured graphs built from older values are never reused.
        Edits made through `p.data` (`p.data.copy_`, `p.data.add_`) do NOT bump the counter (`.data` is a detached alias with its own
        version): call `invalidate_packed_weights()` after them."""
        return sum(p._version for p in self.parameters())

    # "fp8" (the default; precision "high" with fp16 operands): the correction products A W_lo of the transformer's MLPs (fc1, fc2) run on the
    # block-scaled fp8 MFMA (f3r.h F3R_SPLIT_W2F8: 1.4x the matrix-pipe rate of a second fp16 plane; LayerNorm and fc1's GELU epilogue write the
    # fp8 copies beside their fp16 outputs) for every pass whose token count is a multiple of 256; "fp16": two fp16 planes everywhere.  Measured
    # on ViT-L stress weights (profiles/r05_parity_low_plane_fp8_vs_fp16_vit_large_hot.txt): the same distance to the fp32 path (2.34e-4 vs
    # 2.39e-4 at N = 3, 2.76e-4 both at N = 100), +0.7 % views/s at N = 320, +1.7 % at N = 100, +3.9 % fusion-only at N = 20.  Changing it
    # needs invalidate_packed_weights().
    low_plane = "fp8"
    # precision "robust": where the two correction products of the fusion attention's scores (q_lo k_hi + q_hi k_lo) run -- "fp8": the block-scaled
    # fp8 MFMA (f3r_attn_asm_qk3f8_f16: 256 matrix-pipe cycles per score block; the fp8 copies move the softmax by ~2e-5), "fp16": two more fp16
    # products (f3r_attn_asm_qk3_f16: 384 cycles).  Read per forward: no re-packing needed.
    robust_corrections = "fp8"
    # precision "robust": the ENCODER's per-view attention (1024 keys; 0.6 % of the step's attention FLOPs at N = 320) -- "fp32": the fp32 attention of
    # precision "exact" (0.8 s of a 14.2 s step on the FMA pipe), "planes": the same three-product kernel as the fusion layers, one launch over the
    # batch of views (59 ms).  Measured on the heavy-tailed ViT-L set (N = 3 vs the CPU oracle): 7.8e-5 with "fp32", 5.2e-4 with "planes" -- both
    # inside 1e-3, the default keeps the larger margin (a tier people turn to because their checkpoint amplifies noise); N = 320: 14.2 s / 13.7 s.
    robust_encoder_attention = "fp32"
    # DPT heads in precision "high" with fp16 planes: "fp8" (the default, round 6) runs the two correction products of every 3x3 convolution with
    # Cin % 128 == 0 and at least head_f8_min_rows output pixels PER VIEW (from the 64 x 64 level on at 512 x 512: refinenet2 / 1, head[0],
    # head[2]: ~88 % of the heads' FLOPs) on the block-
    # scaled fp8 MFMA (f3r.h F3R_SPLIT_X3F8: two matrix-pipe units instead of X3's three; the producers write the fp8 planes beside the fp16 high
    # plane instead of an fp16 low plane nobody else reads); "fp16": three fp16 products everywhere.  oracle/precision_study.py --study heads_f8:
    # the stress fixture moves from 6.94e-4 to 6.93e-4.  Changing it needs invalidate_packed_weights().
    head_corrections = "fp8"
    head_f8_min_rows = 4096
    # head[2] + ReLU -> head[4] (1x1 conv to 3 / 4 channels) -> postprocess in ONE launch (f3r_gemm_args.fin_w) whenever head[2] has at least
    # this many output pixels per view and the head's last_dim is 128: the 128-channel activation at full resolution (512 B per pixel with planes) is never
    # written or read back.  A very large value restores conv -> f3r_dpt_final.
    head_tail_fused_min_rows = 4096
    high_fc1_planes = True   # False: fc1 weights single-plane in precision "high" (see _pack_block); changing it needs invalidate_packed_weights()

    def _format(self):
        """The knobs above + precision + compute_dtype -> the OperandFormat of the next _pack / forward (the ONE place that reads them)."""
        p, lp = self.precision, self.compute_dtype
        high_f16 = p == "high" and lp == torch.float16   # the fp8 correction products exist beside fp16 planes in "high" only
        return OperandFormat(
            lp=lp, planes=p != "fast", low_f8=high_f16 and self.low_plane == "fp8", fc1_planes=p != "fast" and (p != "high" or bool(self.high_fc1_planes)),
            head_f8=high_f16 and self.head_corrections == "fp8", linear_split={"fast": None, "high": "w2", "robust": "x3", "exact": "x3"}[p], x3=p in ("robust", "exact"),
            qk3=p == "robust", qk3_planes=3 if self.robust_corrections == "fp8" else 2, qk3_encoder=self.robust_encoder_attention == "planes",
            head_f8_min_rows=self.head_f8_min_rows, head_tail_fused_min_rows=self.head_tail_fused_min_rows)

    @property
    def _head_f8(self):
        return self._format().head_f8

    def _pack(self, device, fmt=None):
        fmt = fmt or self._format()
        lp, hp = fmt.lp, fmt.planes
        key = (str(device), self._params_version(), fmt.pack_part)
        if self._packed is not None and self._packed["key"] == key:
            return self._packed
        alt = getattr(self, "_packed_alt", None)
        if alt is not None and alt["key"] == key:  # two packs are kept, so alternating inference(dtype=...) calls do not re-pack
            self._packed, self._packed_alt = alt, self._packed
            return self._packed
        if self._packed is not None and self._packed["key"][1] != key[1]:  # parameters changed: both packs are stale
            self._packed = self._packed_alt = None
            self._graphs.clear()
        if alt is not None:  # a third format evicts the older pack: captured graphs may hold pointers into its weight tensors
            self._graphs.clear()
        self._packed_alt = self._packed
        enc, dec = self.encoder, self.decoder
        pk = dict(key=key)
        dino = isinstance(enc, DinoEncoder)
        vit = enc.model if dino else enc
        norm = vit.norm if dino else enc.enc_norm
        pk["pe_w"] = ops.pack_linear_weight(vit.patch_embed.proj.weight.detach().float(), lp, hp)  # (DINOv2: (D, 3*14*14 = 588) -> Kpad 640)
        pk["pe_b"] = _f32(vit.patch_embed.proj.bias)
        pk["enc"] = [_pack_dino_block(b, lp, hp) for b in vit.blocks] if dino else [_pack_block(b, fmt) for b in enc.enc_blocks]
        pk["enc_norm"] = (_f32(norm.weight), _f32(norm.bias), norm.eps)
        if dino:
            pk["dino_pos"] = {}  # (h, w) -> interpolated position rows, filled on demand (_dino_pos)
        pk["de_w"] = ops.pack_linear_weight(dec.decoder_embed.weight.detach().float(), lp, hp)
        pk["de_b"] = _f32(dec.decoder_embed.bias)
        if isinstance(dec, LlamaDecoder):
            pk["dec"] = [_pack_llama_block(b, dec.num_heads, lp, hp, dec.n_kv_heads, dec.is_causal) for b in dec.layers]
            pk["dec_norm"] = (_f32(dec.norm.weight), None, dec.norm.eps)
            pk["view0"] = _f32(dec.view0_embed)
        else:
            pk["dec"] = [_pack_block(b, fmt, dec.embed_dim // dec.num_heads) for b in dec.dec_blocks]
            pk["dec_norm"] = (_f32(dec.dec_norm.weight), _f32(dec.dec_norm.bias), dec.dec_norm.eps)
        pk["head"] = dpt_head._pack_head(self.downstream_head, fmt)
        pk["head_local"] = dpt_head._pack_head(self.downstream_head_local, fmt) if self.downstream_head_local is not None else None
        self._packed = pk
        return pk

    def _rope(self, n_pos, device):
        key = (n_pos, str(device))
        if key not in self._rope_cache:
            self._rope_cache[key] = ops.rope_tables(n_pos, self.encoder.rope_freq, device)
        return self._rope_cache[key]

    # ---------------------------------------------------------------- transformer block on the HIP kernels
    def _block_ws(self, fmt, pb, T, D, n_seq, seq_len, dev, external_kv=False):
        """Workspace of the blocks of one encoder pass / decoder sample: ONE allocation shared by all of its layers.  external_kv: K / V^T
        are written into the buffers of a KVExchange (view-sharded path), the workspace keeps no room for them."""
        hidden = pb.fc1_w.shape[0]  # rows of the (possibly stacked [w1; w3]) up-projection
        f8_rows = any(_f8_gemms(pb, T, seq_len))   # the pass takes fp8-low-plane GEMMs
        return ops.BlockWorkspace(T, D, hidden, n_seq, seq_len, fmt.lp, dev, kv_dim=0 if external_kv else pb.kv_dim, f8_rows=f8_rows)

    def _block(self, fmt, x, pb, n_heads, scale, seq_len, n_seq, rope, kv_exchange=None, ws=None, kv_tap=None):
        """x: fp32 residual stream [n_seq*seq_len][D], updated in place.  blocks.py:236-239.  precision "high": every projection runs
        with split weights (hi + lo planes, split="w2"); the activations (LN output, attention output, MLP hidden) stay single.
        ws: the pass's BlockWorkspace (made here when absent): no per-layer allocation."""
        lp, sp = fmt.lp, fmt.linear_split
        if fmt.x3:
            return self._block_exact(fmt, x, pb, n_heads, scale, seq_len, n_seq, rope, kv_exchange)
        D = x.shape[1]
        T = x.shape[0]
        if ws is None:
            ws = self._block_ws(fmt, pb, T, D, n_seq, seq_len, x.device)
        q = ws.q
        if kv_exchange is None:
            k, vt = ws.k, ws.vt
            ldvt = vt.shape[-1]
        else:  # view-sharded: write K / V^T straight into the (padded, persistent) send buffers of the exchange
            k, vt = kv_exchange.k_loc, kv_exchange.vt_loc
        f8_qkv, f8_fc1, f8_fc2 = _f8_gemms(pb, T, seq_len)
        if f8_qkv:
            rows1 = ops.layernorm_f8(x, pb.n1w, pb.n1b, pb.eps, out_rows=ws.rows8(D), rms=pb.rms)
            ops.gemm_qkv(rows1, pb.qk_w8, pb.qkv_b, q, k, vt, seq_len, rope, q_scale=scale * ops.LOG2E, split="w2f8", w_scale=pb.qk_ws, w_aux=pb.v_w2)
            h = ws.h
        else:
            h, _ = ops.layernorm(x, pb.n1w, pb.n1b, pb.eps, lp, out_lp=ws.h, rms=pb.rms)
            ops.gemm_qkv(h, pb.qkv_w, pb.qkv_b, q, k, vt, seq_len, rope, q_scale=scale * ops.LOG2E, rope_mode=pb.rope_mode, split=sp, q_dim=pb.q_dim)
        if kv_tap is not None and kv_exchange is None:
            kv_tap(k, vt)  # the K / V^T of this fusion layer (capture for the per-rank emulation test)
        o = h  # LN output is dead: reuse as the attention output buffer
        gqa = dict(kv_group=pb.kv_group, causal=pb.causal, head_dim=pb.head_dim)
        if kv_exchange is None:
            Dkv = k.shape[1]
            ops.attention(q, o, n_heads, scale, [(k, vt, seq_len, seq_len * Dkv, Dkv * ldvt)], tq=seq_len, batch=n_seq,
                          q_batch_stride=seq_len * D, o_batch_stride=seq_len * D, q_prescaled=True, **gqa)
        else:
            # view-sharded: the all-gather of the remote K / V^T runs while the kernel attends over the local shard; the
            # online-softmax state (m, l, O) is parked in fp32 and resumed over the remote segments once they have landed
            sharding = self.sharding
            sharding.begin_layer(kv_exchange)  # exchange="auto": which form this layer uses (probe, then the winner)
            kv_exchange.start()
            if seq_len == 0:
                kv_exchange.finish()  # a rank without tokens still takes part in the collective
            elif kv_exchange.has_remote:
                pos = kv_exchange.positions()  # global token index of the first row of every rank's shard (causal attention only)
                # (reserve_cus: the persistent launch leaves a few CUs to the kernels that move the other ranks' shards meanwhile -- ViewSharding.reserve_cus)
                ops.attention(q, o, n_heads, scale, [kv_exchange.local_segment()], tq=seq_len, q_prescaled=True,
                              state=kv_exchange.state, state_out=True, q_pos0=pos[kv_exchange.rank], seg_pos0=[pos[kv_exchange.rank]],
                              reserve_cus=getattr(sharding, "reserve_cus", 0), **gqa)
                kv_exchange.mark_local_done()
                # the remote shards, as ONE group once the all-gathers have landed or ("p2p" exchange) shard by shard in arrival order
                groups = [(w, sg) for w, sg in kv_exchange.remote_groups()]
                live = [i for i, (_, sg) in enumerate(groups) if sg]
                for i, (wait, segs) in enumerate(groups):
                    wait()
                    if live and i == live[0]:
                        kv_exchange.mark_remote_start()  # what the local launch did not hide = the gap on this stream up to here
                    if not segs:
                        continue
                    ops.attention(q, o, n_heads, scale, segs, tq=seq_len, q_prescaled=True, state=kv_exchange.state, state_in=True,
                                  state_out=(i != live[-1]), q_pos0=pos[kv_exchange.rank],
                                  seg_pos0=[kv_exchange.remote_position_of(sg) for sg in segs], **gqa)
            else:
                kv_exchange.finish()
                ops.attention(q, o, n_heads, scale, [kv_exchange.local_segment()], tq=seq_len, q_prescaled=True, **gqa)
            sharding.end_layer(kv_exchange)
        ops.gemm(o, pb.proj_w, bias=pb.proj_b, res_f32=x, out_f32=x, split=sp)
        if f8_fc1:
            rows = ops.layernorm_f8(x, pb.n2w, pb.n2b, pb.eps, out_rows=ws.rows8(D), rms=pb.rms)
            if f8_fc2:   # fc1's GELU epilogue writes rows [4 D fp16 | 4 D fp8], fc2 runs on them
                _, hid = ops.gemm(rows, pb.fc1_w8, bias=pb.fc1_b, act="gelu", out_lp=ws.hid8(), split="w2f8", w_scale=pb.fc1_ws, out_f8_rows=True)
                ops.gemm(hid, pb.fc2_w8, bias=pb.fc2_b, res_f32=x, out_f32=x, split="w2f8", w_scale=pb.fc2_ws)
            else:
                _, hid = ops.gemm(rows, pb.fc1_w8, bias=pb.fc1_b, act="gelu", out_lp=ws.hid, split="w2f8", w_scale=pb.fc1_ws)
                ops.gemm(hid, pb.fc2_w, bias=pb.fc2_b, res_f32=x, out_f32=x, split=sp)
            return x
        h2, _ = ops.layernorm(x, pb.n2w, pb.n2b, pb.eps, lp, out_lp=o, rms=pb.rms)
        if pb.swiglu_hidden:  # LlamaDecoder FeedForward: w2(silu(w1 x) * w3 x) (llama.py:284)
            _, ab = ops.gemm(h2, pb.fc1_w, out_lp=ws.hid, split=sp)
            hid = ops.silu_mul(ab, pb.swiglu_hidden)
        else:
            _, hid = ops.gemm(h2, pb.fc1_w, bias=pb.fc1_b, act="gelu", out_lp=ws.hid, split=sp if pb.fc1_split in (None, True) else None)
        ops.gemm(hid, pb.fc2_w, bias=pb.fc2_b, res_f32=x, out_f32=x, split=sp)
        return x

    def _block_exact(self, fmt, x, pb, n_heads, scale, seq_len, n_seq, rope, kv_exchange):
        """precision "exact": the same block with every operand as hi + lo planes and fp32 attention.  LayerNorm / RMSNorm -> fp32 -> planes;
        QKV through the generic epilogue into an fp32 [T][Dq + 2 Dkv] buffer (+ rotary embedding in place, 2-D or per-view); f3r_attn_f32_ex
        (grouped-query heads, causal by absolute position) -> planes; proj / fc1 (+GELU | SwiGLU gate, planes out) / fc2 as X3 GEMMs with the
        fp32 residual epilogue.  View-sharded: the fp32 K and V rows of all ranks are all-gathered (blocking: this is the validation mode)
        and the rank's queries attend over them in one launch."""
        lp = fmt.lp
        T = x.shape[0]
        _, hf = ops.layernorm(x, pb.n1w, pb.n1b, pb.eps, lp, want_lp=False, want_f32=True, rms=pb.rms)
        h, hl = _planes(fmt, hf)
        qkv, _ = ops.gemm(h, pb.qkv_w, bias=pb.qkv_b, want_f32=True, split="x3", a_lo=hl)
        n_kv = n_heads // pb.kv_group
        if rope is not None and T:
            ops.rope_f32(qkv, n_heads + n_kv, max(1, seq_len), rope, pb.rope_mode)
        gqa = dict(head_dim=pb.head_dim, kv_group=pb.kv_group, causal=pb.causal)
        if kv_exchange is None and fmt.qk3 and self._qk3_ok(fmt, pb, n_seq, seq_len) and (n_seq == 1 or fmt.qk3_encoder):
            # precision "robust": Q and K as hi + lo fp16 planes, three products per score block on the hand-scheduled kernel (f3r_attn_args.qk_planes),
            # P and V single fp16; the launch parks its softmax state and a small pass turns it into the planes of the attention output
            # (robust_corrections "fp8": the two correction products on the block-scaled fp8 MFMA -- rows [hi fp16 | e4m3(hi) | e4m3(lo 2^12)])
            planes = fmt.qk3_planes
            qp, kp, vt = ops.qkv_planes(qkv, n_heads, n_kv, n_seq, seq_len, scale * ops.LOG2E, lp, planes=planes)
            state = ops.attention_state(T, n_heads, x.device, pb.head_dim)
            ldvt_ = vt.shape[-1]
            ops.attention(qp, state[0], n_heads, scale, [(kp, vt.view(n_seq * n_kv * 64, ldvt_), seq_len, seq_len * n_kv * 128, n_kv * 64 * ldvt_)], tq=seq_len,
                          batch=n_seq, q_batch_stride=seq_len * n_heads * 128, o_batch_stride=seq_len * n_heads * 64, q_prescaled=True, state=state,
                          state_out=True, kv_group=pb.kv_group, head_dim=64, qk_planes=planes, kernel_sel=2)
            o, ol = ops.attention_state_finish(state, n_heads, 64, lp)
            del qp, kp, vt, state
        elif kv_exchange is None:
            o, ol = ops.attention_f32(qkv, n_heads, n_seq, seq_len, scale, lp, **gqa)
        else:
            Dq, Dkv = n_heads * pb.head_dim, n_kv * pb.head_dim
            k_all, v_all = kv_exchange.gather_rows_f32(qkv[:, Dq:Dq + Dkv], qkv[:, Dq + Dkv:])
            if T:
                o, ol = ops.attention_f32(qkv, n_heads, 1, seq_len, scale, lp, kv=(k_all, v_all), q_pos0=kv_exchange.positions()[kv_exchange.rank], **gqa)
            else:
                o = ol = torch.empty((0, Dq), dtype=lp, device=x.device)
        ops.gemm(o, pb.proj_w, bias=pb.proj_b, res_f32=x, out_f32=x, split="x3", a_lo=ol)
        _, hf = ops.layernorm(x, pb.n2w, pb.n2b, pb.eps, lp, want_lp=False, want_f32=True, out_f32=hf, rms=pb.rms)
        h, hl = _planes(fmt, hf)
        if pb.swiglu_hidden:  # LlamaDecoder FeedForward: w2(silu(w1 x) * w3 x) (llama.py:284)
            ab, _ = ops.gemm(h, pb.fc1_w, want_f32=True, split="x3", a_lo=hl)
            hid, hid_lo = ops.silu_mul_f32(ab, pb.swiglu_hidden, lp)
        else:
            _, hid, hid_lo = ops.gemm(h, pb.fc1_w, bias=pb.fc1_b, act="gelu", want_lp=True, want_lo=True, split="x3", a_lo=hl)
        ops.gemm(hid, pb.fc2_w, bias=pb.fc2_b, res_f32=x, out_f32=x, split="x3", a_lo=hid_lo)
        return x

    def _qk3_ok(self, fmt, pb, n_seq, seq_len):
        """can this block's attention take the three-product kernels (f3r_attn_asm_qk3{,f8}_f16)?  head_dim 64, fp16, no causal mask, whole 64-key
        tiles per sequence, at least one wave of queries, a power-of-two head group; any number of sequences (the fusion decoder's one, the
        encoder's one per view: the kernels park their softmax state per sequence).  Everything else in precision "robust" -- odd token counts
        (DINOv2's class token), causal Llama decoders, sharded models -- runs the fp32 attention of precision "exact" (more exact, slower)."""
        g = pb.kv_group
        return (fmt.lp == torch.float16 and pb.head_dim == 64 and not pb.causal and n_seq >= 1 and seq_len >= 64 and seq_len % 64 == 0
                and n_seq < 65536 and g >= 1 and (g & (g - 1)) == 0)

    @staticmethod
    def _norm_planes(fmt, x, norm, rms=False, out_lp=None, f32=False):
        """The final LayerNorm / RMSNorm of a pass (norm = its packed (weight, bias, eps)) -> the (hi, lo) planes the heads read; (lowp, None),
        written to out_lp when given, in the formats without low planes.  f32: (the fp32 rows, None) instead, i.e. before that rounding."""
        w_, b_, eps = norm
        if fmt.planes or f32:
            _, y = ops.layernorm(x, w_, b_, eps, fmt.lp, want_lp=False, want_f32=True, rms=rms)
            return (y.clone(), None) if f32 else _planes(fmt, y)
        return ops.layernorm(x, w_, b_, eps, fmt.lp, out_lp=out_lp, rms=rms)[0], None

    def _dino_pos(self, pk, h, w, dev):
        """DINOv2 `interpolate_pos_encoding` (models/vision_transformer.py) for an h x w token grid -> (cls row + pos[0] (D,), patch rows
        (h*w, D)) fp32, cached per grid.  Parameter preprocessing on the host side of the boundary (like the RoPE tables): the trained
        (pos_grid x pos_grid) table is resized bicubically with the hub models' settings (interpolate_offset 0.1, no antialias)."""
        key = (h, w)
        if key not in pk["dino_pos"]:
            vit = self.encoder.model
            pe = vit.pos_embed.detach().float().to(dev)
            M, D = vit.pos_grid, vit.embed_dim
            patch = pe[:, 1:]
            if not (h * w == M * M and h == w):
                patch = torch.nn.functional.interpolate(patch.reshape(1, M, M, D).permute(0, 3, 1, 2), mode="bicubic", antialias=False,
                                                        scale_factor=(float(h + 0.1) / M, float(w + 0.1) / M))
                assert tuple(patch.shape[-2:]) == (h, w)
                patch = patch.permute(0, 2, 3, 1).reshape(1, h * w, D)
            cls_row = (vit.cls_token.detach().float().to(dev)[0, 0] + pe[0, 0]).contiguous()
            pk["dino_pos"][key] = (cls_row, patch[0].contiguous())
        return pk["dino_pos"][key]

    def _patch_lo(self, fmt, imgs, ps, ld_out):
        """precision "exact": the low plane of the im2col rows = the im2col rows of the image's low plane (patchify only moves and rounds:
        its output is lowp(img), so lowp(img - lowp(img)) patchified is exactly the remainder plane); None otherwise."""
        if not fmt.x3:
            return None
        _, lo = ops.cast_lp(imgs.contiguous(), fmt.lp, want_lo=True)
        return ops.patchify(lo.float(), ps, fmt.lp, ld_out=ld_out)

    def _encode(self, fmt, imgs, pk):
        """CroCoEncoder.forward (fast3r.py:549-559) for a batch of same-size images -> enc_norm output [NV*P][D] as (lowp, low plane or
        None).  The high plane alone feeds decoder_embed; both planes are hook 0 of the heads in "high" precision.
        DinoEncoder: DINOv2 forward_features -> x_norm_patchtokens (DinoEncoder._process_images, fast3r.py:636-651) for a batch of same-size,
        upright images: patch embedding (k = s = 14) + [cls] + resized position table, the ViT blocks (no RoPE; LayerScale folded into
        the packed weights), final LayerNorm, patch tokens only."""
        lp, hp, sp = fmt.lp, fmt.planes, fmt.linear_split
        dino = isinstance(self.encoder, DinoEncoder)
        enc = self.encoder.model if dino else self.encoder
        NV, _, H, W = imgs.shape
        ps, D = enc.patch_size, enc.embed_dim
        if dino:
            assert H % ps == 0 and W % ps == 0, f"Input image size ({H}, {W}) is not a multiple of the patch size ({ps})"
        else:
            assert H % ps == 0, f"Input image height ({H}) is not a multiple of patch size ({ps})."  # patch_embed.py:27-32
            assert W % ps == 0, f"Input image width ({W}) is not a multiple of patch size ({ps})."
        h, w = H // ps, W // ps
        P = h * w
        seq = P + dino  # DINOv2: [cls | patches] per image
        if dino:
            cls_row, pos_rows = self._dino_pos(pk, h, w, imgs.device)
        rope = None if dino else self._rope(max(h, w), imgs.device) + (w,)
        kpad = pk["pe_w"].shape[1] // (2 if hp else 1) if dino else 0
        out = torch.empty((NV * P, D), dtype=lp, device=imgs.device)
        out_lo = torch.empty_like(out) if hp else None
        step = max(1, self.max_parallel_views_for_encoder)
        for v0 in range(0, NV, step):
            v1 = min(NV, v0 + step)
            n = v1 - v0
            a = ops.patchify(imgs[v0:v1].contiguous(), ps, lp, ld_out=kpad)
            if dino:
                tok, _ = ops.gemm(a, pk["pe_w"], bias=pk["pe_b"], res_f32=pos_rows.repeat(n, 1), want_f32=True, split=sp,
                                  a_lo=self._patch_lo(fmt, imgs[v0:v1], ps, kpad))
                x = torch.empty((n, seq, D), dtype=torch.float32, device=imgs.device)
                x[:, 0] = cls_row
                x[:, 1:] = tok.view(n, P, D)
                x = x.view(n * seq, D)
            else:
                x, _ = ops.gemm(a, pk["pe_w"], bias=pk["pe_b"], want_f32=True, split=sp, a_lo=self._patch_lo(fmt, imgs[v0:v1], ps, kpad))
            ws = self._block_ws(fmt, pk["enc"][0], x.shape[0], D, n, seq, imgs.device)
            for pb in pk["enc"]:
                self._block(fmt, x, pb, enc.num_heads, (D // enc.num_heads) ** -0.5, seq, n, rope, ws=ws)
            rows = slice(v0 * P, v1 * P)
            hi, lo = self._norm_planes(fmt, x, pk["enc_norm"], out_lp=None if hp or dino else out[rows])
            if hp or dino:  # (a single CroCo plane is already there); DINOv2: the patch tokens only
                out[rows].view(n, P, D).copy_(hi.view(n, seq, D)[:, -P:])
            if hp:
                out_lo[rows].view(n, P, D).copy_(lo.view(n, seq, D)[:, -P:])
        return out, out_lo, P, (h, w)

    # ---------------------------------------------------------------- fusion decoder on the HIP kernels
    def _decode_sample(self, fmt, pk, enc_hi, enc_lo, Ps, emb_rows, v_lo, kvx, f32_hooks=False):
        """Fast3RDecoder.forward / LlamaDecoder.forward (fast3r.py:768-808 / :924-966) for ONE sample: enc_hi [T_loc][Denc] lowp (the
        local views' encoder tokens, view after view; enc_lo = their low plane or None), Ps = tokens per local view, emb_rows
        (N_total, D) fp32 = the image-id rows of ALL views (this rank's are [v_lo, v_lo + len(Ps))).  Returns the 4 hooked
        outputs (fast3r.py:148) as (plane, low plane or None) pairs; f32_hooks: as (fp32 tensor, None) instead, i.e. before the rounding
        to the heads' operand format (decode_tokens: parity of the decoder alone)."""
        dec = self.decoder
        sp = fmt.linear_split
        a_lo = enc_lo if fmt.x3 else None  # "exact": decoder_embed reads both planes of the encoder tokens
        dev = enc_hi.device
        L = dec.depth
        llama = isinstance(dec, LlamaDecoder)
        hd_ = int(self.decoder_args["depth"]) if llama else L  # the heads read decoder_args["depth"] for both decoder types (fast3r.py:137-148)
        hooks = [0, hd_ * 2 // 4, hd_ * 3 // 4, hd_]
        scale = dec.attention_scale(self.training)
        D = dec.embed_dim
        T_loc, n_loc = sum(Ps), len(Ps)
        x = torch.empty((T_loc, D), dtype=torch.float32, device=dev)
        ws = self._block_ws(fmt, pk["dec"][0], T_loc, D, 1, T_loc, dev, external_kv=kvx is not None)  # one allocation for all L blocks
        planes = (lambda t: (t.clone(), None)) if f32_hooks else (lambda t: _planes(fmt, t))
        rope = None
        if llama:
            # embed; per layer add view0_embed to the tokens of view 0, then the block with the rotary angles of each token's view;
            # outputs[0] = embedded tokens, outputs[n_layers] = final RMSNorm
            ops.gemm(enc_hi, pk["de_w"], bias=pk["de_b"], out_f32=x, split=sp, a_lo=a_lo)
            rows = emb_rows[v_lo:v_lo + n_loc]                              # (n_loc, 64) = [cos (32) | sin (32)] of each view's id
            if len(set(Ps)) == 1:
                rope = (rows[:, :32].contiguous(), rows[:, 32:].contiguous(), Ps[0])
            else:  # mixed resolutions: one table row per token
                per_tok = rows.repeat_interleave(torch.tensor(Ps, device=dev), dim=0)
                rope = (per_tok[:, :32].contiguous(), per_tok[:, 32:].contiguous(), 1)
            view0_rows = Ps[0] if v_lo == 0 else 0                          # view 0 lives on the rank that owns the first views
            taps = {0: planes(x)}
        else:
            if len(set(Ps)) == 1:
                ops.gemm(enc_hi, pk["de_w"], bias=pk["de_b"], rowadd=emb_rows[v_lo:v_lo + n_loc].contiguous(), rowadd_div=Ps[0], out_f32=x, split=sp,
                         a_lo=a_lo)
            else:
                r0 = 0
                for i in range(n_loc):
                    ops.gemm(enc_hi[r0:r0 + Ps[i]], pk["de_w"], bias=pk["de_b"], rowadd=emb_rows[v_lo + i:v_lo + i + 1].contiguous(),
                             rowadd_div=Ps[i], out_f32=x[r0:r0 + Ps[i]], split=sp, a_lo=None if a_lo is None else a_lo[r0:r0 + Ps[i]])
                    r0 += Ps[i]
            taps = {0: (enc_hi.float(), None) if f32_hooks else (enc_hi, enc_lo)}
        for li, pb in enumerate(pk["dec"]):
            if llama:
                ops.rows_add(x, pk["view0"], view0_rows)
            self._block(fmt, x, pb, dec.num_heads, scale, T_loc, 1, rope, kvx, ws=ws, kv_tap=self.kv_tap)
            if (li + 1) in hooks and (li + 1) != L:
                taps[li + 1] = planes(x)
        if L in hooks:  # (always, but for a LlamaDecoder whose n_layers is not decoder_args["depth"])
            taps[L] = self._norm_planes(fmt, x, pk["dec_norm"], rms=llama, f32=f32_hooks)
        return [taps[hk] for hk in hooks]

    @torch.no_grad()
    def decode_tokens(self, enc_tokens, tokens_per_view, image_ids, return_f32=False, enc_tokens_lo=None):
        """The fusion decoder alone (BASELINE configs[1]: "fusion transformer only, frozen random encoder"): enc_tokens lowp
        [sum(tokens_per_view)][enc_embed_dim] on the GPU, image_ids (N,) or (1, N) long -> the 4 hooked outputs [T][D], lowp as the
        heads read them, or fp32 before that rounding with return_f32.  enc_tokens_lo: optional low plane of the tokens (split-precision
        modes: tokens = enc_tokens + enc_tokens_lo), default zero."""
        dev = enc_tokens.device
        if dev.type != "cuda":
            raise F3RError(f"fast3r_amd.Fast3R runs only on a ROCm GPU (tokens are on {dev}); there is no CPU fallback")
        with torch.cuda.device(dev):
            fmt = self._format()
            pk = self._pack(dev, fmt)
            ids = torch.as_tensor(image_ids).reshape(-1).to(dev)
            assert ids.numel() == len(tokens_per_view)
            emb_rows = self.decoder.image_idx_emb.to(dev)[ids]
            enc_lo = None
            if fmt.planes and not isinstance(self.decoder, LlamaDecoder):
                enc_lo = torch.zeros_like(enc_tokens) if enc_tokens_lo is None else enc_tokens_lo.contiguous()
            with ops.family("transformer_linears"):
                out = self._decode_sample(fmt, pk, enc_tokens.contiguous(), enc_lo, list(tokens_per_view), emb_rows, 0, None, f32_hooks=return_f32)
            return [t[0] for t in out]

    # ---------------------------------------------------------------- DPT head on the HIP kernels
    # ---------------------------------------------------------------- forward
    def forward(self, views, profiling=False, host_outputs=False):
        """fast3r.py:302-497.  views: list[N] of dicts with 'img' (B,3,H,W) on a ROCm device.
        host_outputs (fast3r_amd.inference sets it): return the per-view tensors on the HOST instead of the device -- every head chunk's
        pointmaps / confidences are copied into pinned host memory by a side stream as soon as the chunk is done, overlapped with the heads
        of the next chunk (what the reference does after the forward with a blocking `to_cpu`, dust3r/inference_multiview.py:92-93)."""
        if len(views) == 0:
            return ([], {}) if profiling else []
        if (self.use_graphs and not profiling and self.sharding is None and self.debug_taps is None and not isinstance(self.decoder, LlamaDecoder)
                and not self._format().x3):  # (the plane modes allocate per layer: they always run eagerly)
            dev = views[0]["img"].device
            if dev.type == "cuda":  # (anything else: the eager path raises its F3RError)
                with torch.cuda.device(dev):  # capture and replay on the tensors' device, whatever the caller's current device is
                    out = self._graphs.run(self, views, host_outputs=host_outputs)
                if out is not None:
                    return out
        return self._forward_eager(views, profiling, host_outputs=host_outputs)

    def enable_graphs(self, on=True, max_views=64):
        """Opt-in hipGraph replay for launch-bound scenes (a forward of N <= max_views same-size views is a chain of
        ~400 + 30 N short launches; below N of about 20 the host cannot issue them as fast as the GPU retires them).  The
        first forward of a new (N, B, H, W) shape runs eagerly once and is then captured; later forwards of that shape copy
        the images into the captured input buffers, draw the image ids on the host exactly like the eager path and replay.
        Same kernels, same order, same results."""
        self.use_graphs = bool(on)
        self._graphs.max_views = max_views
        return self

    def _orientation_plan(self, views):
        """Per (view, sample): is the image stored transposed (a portrait picture kept as a landscape tensor)?

        The reference handles aspect ratio in two places: `ManyAR_PatchEmbed` (dust3r/patch_embed.py:41-105) swaps the
        axes of the samples whose `true_shape` is portrait before the patch convolution, and `transpose_to_landscape(head,
        activate=landscape_only)` (dust3r/utils/misc.py:61-106) runs the head of those samples on the (W, H) grid and swaps the output
        back.  With PatchEmbedDust3R / landscape_only=False (what the inference loaders set, utils/checkpoint_utils.py:37-38) neither
        happens and `true_shape` must be identical for all samples of a view (misc.py:69).  Returns, per view, `enc_swap` (B bools),
        `head_hw` (B (H, W) pairs: the image size the head predicts at) and `head_swap` (B bools)."""
        many_ar = self.encoder.patch_embed_cls in ("ManyAR_PatchEmbed", "dino")  # DinoEncoder.forward also encodes portraits upright (:592-599)
        plan, any_p = [], False
        for v in views:
            img = v["img"]
            B, H, W = img.shape[0], img.shape[-2], img.shape[-1]
            ts = v.get("true_shape", None)
            ts = torch.tensor([[H, W]] * B) if ts is None else torch.as_tensor(ts).cpu().reshape(B, 2).long()
            portrait = (ts[:, 1] < ts[:, 0]).tolist()
            if self.encoder.patch_embed_cls == "ManyAR_PatchEmbed":
                assert W >= H, f"img should be in landscape mode, but got {W=} {H=}"  # patch_embed.py:62
            enc_swap = [bool(p) and many_ar for p in portrait]
            if self.landscape_only:  # wrapper_yes: by definition the batch is stored in landscape mode, W >= H (misc.py:77-80)
                Ht, Wt = int(ts.min()), int(ts.max())
                head_hw = [(Wt, Ht) if p else (Ht, Wt) for p in portrait]
                head_swap = [bool(p) for p in portrait]
            else:                    # wrapper_no
                if not bool((ts[0:1] == ts).all()):
                    raise AssertionError("true_shape must be all identical")  # utils/misc.py:69
                head_hw = [tuple(ts[0].tolist())] * B
                head_swap = [False] * B
            any_p = any_p or any(enc_swap) or any(head_swap) or any(tuple(hw) != (H, W) for hw in head_hw)
            plan.append(dict(enc_swap=enc_swap, head_hw=head_hw, head_swap=head_swap))
        return dict(views=plan, any_portrait=any_p)

    def _forward_eager(self, views, profiling=False, _emb_rows=None, host_outputs=False):
        dev = views[0]["img"].device
        if dev.type != "cuda":
            raise F3RError(f"fast3r_amd.Fast3R runs only on a ROCm GPU (views are on {dev}); there is no CPU fallback")
        if any(v["img"].device != dev for v in views) or next(self.parameters()).device != dev:
            raise F3RError("fast3r_amd.Fast3R: the model and every view must live on the same device")
        with torch.cuda.device(dev):  # kernels launch on the CURRENT device / stream: make that the tensors' device
            return self._forward_on_device(views, profiling, _emb_rows, dev, host_outputs)

    def _forward_on_device(self, views, profiling, _emb_rows, dev, host_outputs=False):
        prof = {} if profiling else None
        fmt = self._format()
        pk = self._pack(dev, fmt)
        enc, dec = self.encoder, self.decoder
        ps = enc.patch_size
        sh = self.sharding
        N_total = len(views)
        v_lo, v_hi = (0, N_total) if sh is None else sh.my_range(N_total)
        if sh is not None and N_total < sh.world:
            raise ValueError(f"view sharding needs at least one view per rank ({N_total} views, {sh.world} ranks)")
        my_views = views[v_lo:v_hi]
        n_loc = len(my_views)
        B = views[0]["img"].shape[0]

        # ---- encode (fast3r.py:250-296): every (view, sample) image, grouped by its (possibly un-transposed) size
        t0 = time.time()
        plan = self._orientation_plan(views) if _emb_rows is None else dict(views=[None] * N_total, any_portrait=False)
        Ps, feats = [], [[None] * B for _ in range(n_loc)]  # feats[i][b] = (hi [P][D], lo or None)
        if not plan["any_portrait"] and all(tuple(v["img"].shape[-2:]) == tuple(my_views[0]["img"].shape[-2:]) for v in my_views) and n_loc > 0:
            imgs = torch.cat([v["img"] for v in my_views], dim=0).float()
            with ops.family("transformer_linears"):   # (bench.py roofline.others: which family a GEMM-like launch is booked under)
                f, flo, P, grid = self._encode(fmt, imgs, pk)
            f = f.view(n_loc, B, P, -1)
            flo = None if flo is None else flo.view(n_loc, B, P, -1)
            for i in range(n_loc):
                for b in range(B):
                    feats[i][b] = (f[i, b], None if flo is None else flo[i, b])
            Ps = [P] * n_loc
            head_grid = [[grid] * B for _ in range(n_loc)]
            head_swap = [[False] * B for _ in range(n_loc)]
        else:
            groups = {}  # image size as encoded -> [(i, b, image (3, H', W'))]
            head_grid, head_swap = [], []
            for i, v in enumerate(my_views):
                pl = plan["views"][v_lo + i]
                img = v["img"].float()
                P_view = (img.shape[-2] // ps) * (img.shape[-1] // ps)
                Ps.append(P_view)
                grids_i = []
                for b in range(B):
                    im = img[b].transpose(-1, -2) if pl["enc_swap"][b] else img[b]
                    groups.setdefault(tuple(im.shape[-2:]), []).append((i, b, im))
                    hh, ww = pl["head_hw"][b]
                    assert hh % ps == 0 and ww % ps == 0 and (hh // ps) * (ww // ps) == P_view, \
                        f"true_shape {pl['head_hw'][b]} does not describe the {tuple(img.shape[-2:])} image of view {v_lo + i}"
                    grids_i.append((hh // ps, ww // ps))
                head_grid.append(grids_i)
                head_swap.append(list(pl["head_swap"]))
            untranspose = isinstance(enc, DinoEncoder)  # its portrait tokens go back to the stored (landscape) order (fast3r.py:601-622)
            for _, items in groups.items():
                with ops.family("transformer_linears"):
                    f, flo, P, (gh_, gw_) = self._encode(fmt, torch.stack([im for _, _, im in items]).contiguous(), pk)
                f = f.view(len(items), P, -1)
                flo = None if flo is None else flo.view(len(items), P, -1)
                for j, (i, b, _) in enumerate(items):
                    fj, fl = f[j], (None if flo is None else flo[j])
                    if untranspose and plan["views"][v_lo + i]["enc_swap"][b]:
                        fj = fj.view(gh_, gw_, -1).transpose(0, 1).reshape(P, -1)
                        fl = None if fl is None else fl.view(gh_, gw_, -1).transpose(0, 1).reshape(P, -1)
                    feats[i][b] = (fj, fl)
        if profiling:
            torch.cuda.synchronize()
            prof["encode_images_time"] = time.time() - t0

        # ---- image ids (fast3r.py:339-348 / 702-743): drawn once for all N views (rank 0 decides when sharded)
        t1 = time.time()
        if _emb_rows is not None:  # graph capture / replay: the rows sit in a captured buffer the caller fills before each replay
            emb_rows = _emb_rows
        else:
            ids = dec.draw_image_ids(B, N_total)
            if sh is not None:
                ids = sh.broadcast_ids(ids, dev)
            emb_rows = dec.image_idx_emb.to(dev)[ids.to(dev)]  # (B, N_total, D) fp32 rows of the table
        if profiling:
            prof["pos_emb_time"] = time.time() - t1

        # ---- fusion decoder (fast3r.py:768-808) per sample; local tokens are queries, K/V cover all views
        if profiling:
            torch.cuda.synchronize()
        t2 = time.time()
        D = dec.embed_dim
        T_loc = sum(Ps)
        hook_toks = []  # per sample: [4] (plane [T_loc][C], low plane or None)
        for b in range(B):
            enc_hi = torch.cat([feats[i][b][0] for i in range(n_loc)], dim=0) if n_loc > 1 else feats[0][b][0]
            enc_hi = enc_hi.contiguous()
            enc_lo = None
            if feats[0][b][1] is not None:
                enc_lo = (torch.cat([feats[i][b][1] for i in range(n_loc)], dim=0) if n_loc > 1 else feats[0][b][1]).contiguous()
            kv_dim = getattr(pk["dec"][0], "kv_dim", None) or D
            kvx = None
            if sh is not None:
                # every rank holds the same list of views, so it knows every rank's token count without asking (no per-forward collective)
                tok = [(v["img"].shape[-2] // ps) * (v["img"].shape[-1] // ps) for v in views]
                t_all = [sum(tok[slice(*split_range(N_total, sh.world, r))]) for r in range(sh.world)]
                assert t_all[sh.rank] == T_loc
                kvx = sh.make_kv_exchange(T_loc, kv_dim, fmt.lp, dev, n_heads=dec.num_heads, q_dim=D, t_all=t_all)
            with ops.family("transformer_linears"):
                hook_toks.append(self._decode_sample(fmt, pk, enc_hi, enc_lo, Ps, emb_rows[b], v_lo, kvx))
            if self.debug_taps is not None:
                self.debug_taps.setdefault("hooks", []).append([t[0].float().cpu() for t in hook_toks[-1]])
        del feats
        if profiling:
            torch.cuda.synchronize()
            prof["decoder_time"] = time.time() - t2
            prof["head_prepare_input_time"] = 0.0  # hooks are consumed in place: no rearrange step (fast3r.py:385-398)

        # ---- heads (fast3r.py:407-485), per sample in chunks of max_parallel_views_for_head consecutive views with one token grid
        t3 = time.time()
        results = [{} for _ in range(n_loc)]
        per_view = [[None] * B for _ in range(n_loc)]  # per (view, sample): {name: tensor (H, W[, 3])}
        offs = np.concatenate([[0], np.cumsum(Ps)]).tolist()
        step = max(1, self.max_parallel_views_for_head)
        heads = [("pts3d_in_other_view", "conf", pk["head"])]
        if pk["head_local"] is not None:
            heads.append(("pts3d_local", "conf_local", pk["head_local"]))
        sink = _HostSink(dev, B) if (host_outputs and sh is None) else None
        for b in range(B):
            i0 = 0
            while i0 < n_loc:
                i1 = i0 + 1
                gh, gw = head_grid[i0][b]
                chunk = dpt_head.chunk_views(step, gh, gw)
                while i1 < n_loc and i1 - i0 < chunk and head_grid[i1][b] == head_grid[i0][b]:
                    i1 += 1
                toks = [(t[0][offs[i0]:offs[i1]], None if t[1] is None else t[1][offs[i0]:offs[i1]]) for t in hook_toks[b]]
                for i in range(i0, i1):
                    per_view[i][b] = {}
                for pname, cname, hk in heads:
                    with ops.family("head_convs"):
                        pts, conf = dpt_head.dpt(fmt, hk, toks, i1 - i0, gh, gw)
                    for i in range(i0, i1):
                        sw = head_swap[i][b]
                        per_view[i][b][pname] = pts[i - i0].swapaxes(0, 1) if sw else pts[i - i0]  # transposed(): misc.py:105-106
                        if conf is not None:
                            per_view[i][b][cname] = conf[i - i0].swapaxes(0, 1) if sw else conf[i - i0]
                    if sink is not None:  # this chunk's outputs start their way to the host while the next chunk's heads run
                        sink.push([(i, b, nm, per_view[i][b][nm]) for i in range(i0, i1) for nm in (pname, cname) if nm in per_view[i][b]], (pts, conf))
                i0 = i1
        for i in range(n_loc):
            for name in per_view[i][0]:
                if sink is not None:
                    results[i][name] = sink.result(i, name)
                elif B == 1:   # one sample: the (1, H, W[, 3]) result IS the head chunk's row (no copy: 4 N device-to-device copies per forward otherwise)
                    results[i][name] = per_view[i][0][name].unsqueeze(0)
                else:
                    results[i][name] = torch.stack([per_view[i][b][name] for b in range(B)], dim=0)
        if sink is not None:
            sink.finish()
        if sh is not None:
            results = sh.gather_results(results, N_total, dev)
        if profiling:
            torch.cuda.synchronize()
            prof["head_forward_time"] = time.time() - t3
            prof["total_time"] = time.time() - t0
            return results, prof
        return results
