"""Packed (device, 16-bit) weights of the transformer blocks: what Fast3R._pack builds from the parameter containers, in the operand format
the model's knobs ask for (fast3r.py OperandFormat)."""
import torch

from . import ops
from .params import _ROPE_PERM, _Block, _DinoBlock, _LlamaBlock


class _PackedBlock:
    __slots__ = ("n1w", "n1b", "n2w", "n2b", "eps", "qkv_w", "qkv_b", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b",
                 "rms", "rope_mode", "swiglu_hidden", "q_dim", "kv_dim", "kv_group", "causal", "head_dim", "fc1_split",
                 "fc1_w8", "fc1_ws", "fc2_w8", "fc2_ws",   # the MLP weights with their low plane in fp8 (Fast3R.low_plane = "fp8"), or None
                 "qk_w8", "qk_ws", "v_w2")                 # ... and the q | k rows of the QKV weight; its v rows as two fp16 planes

    def __init__(self, norm1, norm2):
        """norm1 / norm2: the block's two LayerNorm (weight, bias) or RMSNorm (weight only) modules."""
        self.n1w, self.n1b, self.n2w, self.n2b = (_f32(getattr(n, a, None)) for n in (norm1, norm2) for a in ("weight", "bias"))
        self.eps = norm1.eps
        self.fc1_w8 = self.fc1_ws = self.fc2_w8 = self.fc2_ws = self.qk_w8 = self.qk_ws = self.v_w2 = None
        self.rms, self.rope_mode, self.swiglu_hidden = False, 0, 0
        self.fc1_split = None  # None: like every other projection of the block
        self.head_dim = 64  # the Fast3R fusion decoder may have another width (model_scaling_huge.yaml: 80)
        self.q_dim, self.kv_dim, self.kv_group, self.causal = 0, None, 1, False  # grouped-query / causal attention (LlamaDecoder only)


def _f32(t):
    return None if t is None else t.detach().float().contiguous()


def _pack_block(blk: _Block, fmt, head_dim=64):
    p = _PackedBlock(blk.norm1, blk.norm2)
    lp, split = fmt.lp, fmt.planes
    p.head_dim = head_dim
    p.qkv_w, p.qkv_b = ops.pack_linear_weight(blk.attn.qkv.weight.detach().float(), lp, split), _f32(blk.attn.qkv.bias)
    p.proj_w, p.proj_b = ops.pack_linear_weight(blk.attn.proj.weight.detach().float(), lp, split), _f32(blk.attn.proj.bias)
    # fc1_split False = fc1 single-plane inside "high" (Fast3R.high_fc1_planes = False): measured +3.5 % views/s at N = 100 for TWICE the
    # distance to the fp32 path on the real-size stress model (4.8e-4 / 6.1e-4 against 2.4e-4 / 2.8e-4), so it is an experiment knob, not
    # the default (oracle/precision_study.py per-role run, DESIGN.md section 3 (Precision modes))
    p.fc1_split = fmt.fc1_planes
    p.fc1_w, p.fc1_b = ops.pack_linear_weight(blk.mlp.fc1.weight.detach().float(), lp, p.fc1_split), _f32(blk.mlp.fc1.bias)
    p.fc2_w, p.fc2_b = ops.pack_linear_weight(blk.mlp.fc2.weight.detach().float(), lp, split), _f32(blk.mlp.fc2.bias)
    # Fast3R.low_plane = "fp8" (precision "high", fp16): fc1's weight a second time as rows [K fp16 hi | K fp8 low plane] + one scale per output
    # channel (f3r.h F3R_SPLIT_W2F8); the block uses it whenever its token count is a multiple of 256, the two-fp16-plane pack otherwise
    w1 = blk.mlp.fc1.weight.detach().float()
    w2_ = blk.mlp.fc2.weight.detach().float()
    if fmt.low_f8 and p.fc1_split and w1.shape[1] % 128 == 0 and w1.shape[0] % 256 == 0 and w2_.shape[0] % 256 == 0:
        p.fc1_w8, p.fc1_ws = ops.pack_linear_weight_f8(w1)
        p.fc2_w8, p.fc2_ws = ops.pack_linear_weight_f8(w2_)
    wq = blk.attn.qkv.weight.detach().float()
    Dm = wq.shape[0] // 3
    if fmt.low_f8 and wq.shape[1] % 128 == 0 and Dm % 256 == 0 and head_dim == 64:
        p.qk_w8, p.qk_ws = ops.pack_linear_weight_f8(wq[:2 * Dm])
        p.v_w2 = ops.pack_linear_weight(wq[2 * Dm:], lp, True)
    return p


def _pack_dino_block(blk: _DinoBlock, lp, split=False):
    """DINOv2 block -> the packed fields of a ViT block.  LayerScale is folded into the projection that precedes it:
    gamma * (W a + b) = (gamma[:, None] * W) a + gamma * b -- exact in real arithmetic, no epilogue change."""
    p = _PackedBlock(blk.norm1, blk.norm2)
    g1, g2 = blk.ls1.gamma.detach().float(), blk.ls2.gamma.detach().float()
    p.qkv_w, p.qkv_b = ops.pack_linear_weight(blk.attn.qkv.weight.detach().float(), lp, split), _f32(blk.attn.qkv.bias)
    p.proj_w = ops.pack_linear_weight(g1[:, None] * blk.attn.proj.weight.detach().float(), lp, split)
    p.proj_b = (g1 * blk.attn.proj.bias.detach().float()).contiguous()
    p.fc1_w, p.fc1_b = ops.pack_linear_weight(blk.mlp.fc1.weight.detach().float(), lp, split), _f32(blk.mlp.fc1.bias)
    p.fc2_w = ops.pack_linear_weight(g2[:, None] * blk.mlp.fc2.weight.detach().float(), lp, split)
    p.fc2_b = (g2 * blk.mlp.fc2.bias.detach().float()).contiguous()
    return p


def _pack_llama_block(blk: _LlamaBlock, n_heads, lp, split=False, n_kv_heads=None, causal=False):
    """LlamaDecoder layer -> the same packed fields as a ViT block: [wq; wk; wv] as one QKV matrix (q / k rows permuted per head, see
    _ROPE_PERM), [w1; w3] stacked for one up-projection GEMM, no biases, RMSNorm weights."""
    p = _PackedBlock(blk.attention_norm, blk.ffn_norm)
    p.rms, p.rope_mode = True, 1
    n_kv_heads = n_heads if n_kv_heads is None else n_kv_heads
    perm = torch.tensor([h * 64 + d for h in range(n_heads) for d in _ROPE_PERM])
    perm_kv = torch.tensor([h * 64 + d for h in range(n_kv_heads) for d in _ROPE_PERM])
    wq, wk, wv = (m.weight.detach().float() for m in (blk.attention.wq, blk.attention.wk, blk.attention.wv))
    p.qkv_w, p.qkv_b = ops.pack_linear_weight(torch.cat([wq[perm], wk[perm_kv], wv], dim=0), lp, split), None
    if n_kv_heads != n_heads:
        p.q_dim, p.kv_dim, p.kv_group = n_heads * 64, n_kv_heads * 64, n_heads // n_kv_heads
    p.causal = bool(causal)
    p.proj_w, p.proj_b = ops.pack_linear_weight(blk.attention.wo.weight.detach().float(), lp, split), None
    w1, w3 = blk.feed_forward.w1.weight.detach().float(), blk.feed_forward.w3.weight.detach().float()
    p.swiglu_hidden = w1.shape[0]
    p.fc1_w, p.fc1_b = ops.pack_linear_weight(torch.cat([w1, w3], dim=0), lp, split), None
    p.fc2_w, p.fc2_b = ops.pack_linear_weight(blk.feed_forward.w2.weight.detach().float(), lp, split), None
    return p
