"""Parameter containers of Fast3R: torch.nn modules used ONLY to own parameters.  Their class and attribute names are the state-dict keys of
the reference and the `from_pretrained` contract; none of their forward() methods is ever called (fast3r_amd/fast3r.py)."""
import math

import numpy as np
import torch
import torch.nn as nn

from ._lib import F3RError


class _Params(nn.Module):
    """A module that only owns parameters; calling it is a bug (the compute lives in the HIP engine)."""

    def forward(self, *a, **k):  # pragma: no cover
        raise F3RError("fast3r_amd parameter containers are not callable; use Fast3R.forward")


class _Attention(_Params):
    def __init__(self, dim, qkv_bias=True):
        super().__init__()
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)  # blocks.py:125
        self.proj = nn.Linear(dim, dim)                    # blocks.py:128


class _Mlp(_Params):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)  # blocks.py:94
        self.fc2 = nn.Linear(hidden, dim)  # blocks.py:97


class _Block(_Params):
    def __init__(self, dim, mlp_ratio, eps, qkv_bias=True):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)  # blocks.py:214
        self.attn = _Attention(dim, qkv_bias)
        self.norm2 = nn.LayerNorm(dim, eps=eps)  # blocks.py:227
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class _PatchEmbed(_Params):
    def __init__(self, patch_size, dim):
        super().__init__()
        self.patch_size = (patch_size, patch_size)
        self.proj = nn.Conv2d(3, dim, kernel_size=patch_size, stride=patch_size)  # blocks.py:412-414
        self.norm = nn.Identity()


class CroCoEncoder(_Params):
    """fast3r.py:499-559.  RoPE-2D (freq from 'RoPE<freq>'), LayerNorm eps 1e-6."""

    def __init__(self, img_size=512, patch_size=16, patch_embed_cls="ManyAR_PatchEmbed", embed_dim=768, num_heads=12,
                 depth=12, mlp_ratio=4, pos_embed="RoPE100", attn_implementation="pytorch_naive"):
        super().__init__()
        assert patch_embed_cls in ["PatchEmbedDust3R", "ManyAR_PatchEmbed"]  # patch_embed.py:19
        if not pos_embed.startswith("RoPE"):
            raise NotImplementedError("Unknown pos_embed " + pos_embed)  # fast3r.py:533
        if attn_implementation not in ("pytorch_naive", "flash_attention", "pytorch_auto"):
            raise ValueError(f"Unknown attn_implementation: {attn_implementation}")  # blocks.py:192
        if embed_dim % num_heads != 0 or embed_dim // num_heads != 64:
            raise ValueError("fast3r_amd kernels are built for head_dim 64 (ViT-B/L/H family)")
        self.patch_embed_cls = patch_embed_cls
        self.patch_size, self.embed_dim, self.num_heads, self.depth = patch_size, embed_dim, num_heads, depth
        self.pos_embed = pos_embed
        self.rope_freq = float(pos_embed[len("RoPE"):])
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        self.enc_blocks = nn.ModuleList([_Block(embed_dim, mlp_ratio, 1e-6) for _ in range(depth)])
        self.enc_norm = nn.LayerNorm(embed_dim, eps=1e-6)


class _LayerScale(_Params):
    def __init__(self, dim, init_values=1.0):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class _DinoBlock(_Params):
    """DINOv2 `Block` (dinov2/layers/block.py): x + ls1(attn(norm1(x))); x + ls2(mlp(norm2(x)))."""

    def __init__(self, dim, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim, qkv_bias=True)
        self.ls1 = _LayerScale(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))
        self.ls2 = _LayerScale(dim)


class _DinoViT(_Params):
    """Parameter layout of DINOv2's `DinoVisionTransformer` as torch.hub's `dinov2_vitl14` builds it (facebookresearch/dinov2
    models/vision_transformer.py: img_size 518, patch 14, no register tokens, LayerScale, MLP ffn, block_chunks = 0): the keys under
    `encoder.model.` are the hub checkpoint's own."""

    def __init__(self, embed_dim, depth, num_heads, mlp_ratio, patch_size, pos_grid):
        super().__init__()
        self.embed_dim, self.num_heads, self.patch_size, self.pos_grid = embed_dim, num_heads, patch_size, pos_grid
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + pos_grid * pos_grid, embed_dim))
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))  # in the checkpoint; unused at inference
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        self.blocks = nn.ModuleList([_DinoBlock(embed_dim, mlp_ratio) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)


class DinoEncoder(_Params):
    """fast3r.py:561-651: DINOv2 ViT-L/14 patch tokens (`forward_features(...)['x_norm_patchtokens']`), portrait samples encoded upright
    and their tokens put back in the stored (landscape) order.  The reference builds the backbone with torch.hub.load (network); here
    the same architecture is built locally (random init; a checkpoint's `encoder.model.*` keys load as they are).  The size arguments
    exist only so that tests can build a small one: the reference class is always ViT-L/14."""

    def __init__(self, patch_size=14, embed_dim=1024, depth=24, num_heads=16, mlp_ratio=4, pos_grid=37, **kwargs):
        super().__init__()
        assert patch_size == 14, "DINOv2 model must have patch size 14"  # fast3r.py:570
        if embed_dim // num_heads != 64:
            raise ValueError("fast3r_amd kernels are built for head_dim 64")
        self.patch_size, self.embed_dim, self.num_heads, self.depth = patch_size, embed_dim, num_heads, depth
        self.patch_embed_cls = "dino"
        self.model = _DinoViT(embed_dim, depth, num_heads, mlp_ratio, patch_size, pos_grid)


def sincos_1d_table(embed_dim, n_pos):
    """get_1d_sincos_pos_embed_from_grid (croco/models/pos_embed.py:58-76): [sin | cos], float64 -> float32."""
    omega = np.arange(embed_dim // 2, dtype=float)
    omega /= embed_dim / 2.0
    omega = 1.0 / 10000 ** omega
    out = np.einsum("m,d->md", np.arange(n_pos).reshape(-1).astype(float), omega)
    return torch.from_numpy(np.concatenate([np.sin(out), np.cos(out)], axis=1)).float()


class Fast3RDecoder(_Params):
    """fast3r.py:654-808.  No RoPE; additive image-index embedding; block LayerNorm eps 1e-5, dec_norm 1e-6."""

    def __init__(self, random_image_idx_embedding, enc_embed_dim, embed_dim=768, num_heads=12, depth=12, mlp_ratio=4.0,
                 qkv_bias=True, drop=0.0, attn_drop=0.0, attn_implementation="pytorch_naive",
                 attn_bias_for_inference_enabled=True, max_image_idx=1000):
        super().__init__()
        if attn_implementation not in ("pytorch_naive", "flash_attention", "pytorch_auto"):
            raise ValueError(f"Unknown attn_implementation: {attn_implementation}")
        hd = embed_dim // num_heads
        if embed_dim % num_heads != 0 or hd % 16 != 0 or not 16 <= hd <= 128:
            # the reference takes any dim // num_heads (blocks.py:113-143); 64 runs the tuned attention kernels, the other multiples of
            # 16 up to 128 (model_scaling_huge.yaml: 1280 / 16 = 80) the generic one (f3r_attn_generic.hip)
            raise ValueError(f"fast3r_amd attention kernels are built for head_dim = a multiple of 16 up to 128 (got {embed_dim} / {num_heads})")
        if embed_dim % 64 != 0:
            raise ValueError(f"fast3r_amd: the fused QKV epilogue splits q / k / v on 64-column groups: embed_dim must be a multiple of 64 (got {embed_dim})")
        self.embed_dim, self.num_heads, self.depth = embed_dim, num_heads, depth
        self.random_image_idx_embedding = random_image_idx_embedding
        self.attn_bias_for_inference_enabled = attn_bias_for_inference_enabled
        self.decoder_embed = nn.Linear(enc_embed_dim, embed_dim, bias=True)
        self.dec_blocks = nn.ModuleList([_Block(embed_dim, mlp_ratio, 1e-5, qkv_bias) for _ in range(depth)])
        # The reference table has 1000 rows (fast3r.py:691-697) and therefore fails for N > 1000 views
        # (SURVEY.md section 0.7).  Same formula, more rows when asked for: ids < 1000 are bit-identical.
        self.register_buffer("image_idx_emb", sincos_1d_table(embed_dim, max_image_idx), persistent=False)
        self.dec_norm = nn.LayerNorm(embed_dim, eps=1e-6)

    def attention_scale(self, training: bool) -> float:
        """blocks.py:116-124,151-154."""
        hd = self.embed_dim // self.num_heads
        if (not training) and self.attn_bias_for_inference_enabled:
            return hd ** -0.5 * (1.0 * math.log(137) / math.log(20)) ** 0.5
        return hd ** -0.5

    def draw_image_ids(self, batch_size, num_views, rank=0):
        """fast3r.py:702-743 (_generate_per_rank_generator + _get_random_image_pos), or 0..N-1 (fast3r.py:339-348,794-796).
        Consumes exactly one value of the global torch CPU RNG when random ids are on, like the reference."""
        if not self.random_image_idx_embedding:
            return torch.arange(num_views)[None].repeat(batch_size, 1)
        max_image_idx = self.image_idx_emb.shape[0] - 1
        if num_views - 1 > max_image_idx:
            raise ValueError(f"{num_views} views need an image-index table of at least {num_views} rows "
                             f"(have {max_image_idx + 1}); build the decoder with max_image_idx >= {num_views}")
        seed = torch.randint(0, 2 ** 32, (1,)).item()
        g = torch.Generator()
        g.manual_seed(seed + rank)
        ids = torch.zeros(batch_size, num_views, dtype=torch.long)
        for b in range(batch_size):
            ids[b, 1:] = torch.randperm(max_image_idx, generator=g)[: num_views - 1] + 1
        return ids


class _RMSNorm(_Params):
    def __init__(self, dim, eps=1e-6):
        super().__init__()
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(dim))  # llama.py:150-153


class _LlamaAttention(_Params):
    def __init__(self, dim, n_heads, n_kv_heads):
        super().__init__()
        hd = dim // n_heads
        self.wq = nn.Linear(dim, n_heads * hd, bias=False)     # llama.py:195-198
        self.wk = nn.Linear(dim, n_kv_heads * hd, bias=False)
        self.wv = nn.Linear(dim, n_kv_heads * hd, bias=False)
        self.wo = nn.Linear(n_heads * hd, dim, bias=False)


class _LlamaFeedForward(_Params):
    def __init__(self, dim, hidden_dim, multiple_of, ffn_dim_multiplier):
        super().__init__()
        hidden_dim = int(2 * hidden_dim / 3)                   # llama.py:273-277
        if ffn_dim_multiplier is not None:
            hidden_dim = int(ffn_dim_multiplier * hidden_dim)
        hidden_dim = multiple_of * ((hidden_dim + multiple_of - 1) // multiple_of)
        self.w1 = nn.Linear(dim, hidden_dim, bias=False)
        self.w2 = nn.Linear(hidden_dim, dim, bias=False)
        self.w3 = nn.Linear(dim, hidden_dim, bias=False)


class _LlamaBlock(_Params):
    def __init__(self, dim, n_heads, n_kv_heads, multiple_of, ffn_dim_multiplier, norm_eps):
        super().__init__()
        self.attention = _LlamaAttention(dim, n_heads, n_kv_heads)                       # llama.py:323-326
        self.feed_forward = _LlamaFeedForward(dim, 4 * dim, multiple_of, ffn_dim_multiplier)  # llama.py:327-332
        self.attention_norm = _RMSNorm(dim, norm_eps)
        self.ffn_norm = _RMSNorm(dim, norm_eps)


class LlamaDecoder(_Params):
    """fast3r.py:810-968 (the `llama_dec` experiment, configs/experiment/llama_dec/llama_dec.yaml): pre-norm RMSNorm blocks with SwiGLU,
    bias-free projections, rotary embedding of q / k by the IMAGE id of a token's view (all patches of a view share one angle set), a
    learnable embedding added to the tokens of view 0 before every layer, final RMSNorm.  Bidirectional (the released config) or
    causal attention; grouped-query attention with any n_kv_heads that divides n_heads (incl. 1: multi-query); head_dim must be 64."""

    def __init__(self, random_image_idx_embedding, enc_embed_dim, embed_dim=4096, n_layers=32, n_heads=32, n_kv_heads=None,
                 multiple_of=256, ffn_dim_multiplier=None, norm_eps=1e-5, rope_theta=10000, max_seq_len=1000, is_causal=False,
                 depth_init=True, **kwargs):
        super().__init__()
        if embed_dim % n_heads != 0 or embed_dim // n_heads != 64:
            raise ValueError("fast3r_amd kernels are built for head_dim 64")
        n_kv_heads = n_heads if n_kv_heads is None else int(n_kv_heads)
        if n_heads % n_kv_heads != 0:
            raise ValueError(f"n_heads ({n_heads}) must be a multiple of n_kv_heads ({n_kv_heads})")  # repeat_kv, llama.py:125-134,196
        self.embed_dim, self.num_heads, self.depth = embed_dim, n_heads, n_layers
        self.n_kv_heads, self.is_causal = n_kv_heads, bool(is_causal)
        self.random_image_idx_embedding = random_image_idx_embedding
        self.rope_theta, self.norm_eps = rope_theta, norm_eps
        self.view0_embed = nn.Parameter(torch.zeros(embed_dim))                          # fast3r.py:841-842
        nn.init.normal_(self.view0_embed, mean=0.0, std=0.02)
        self.decoder_embed = nn.Linear(enc_embed_dim, embed_dim, bias=True)              # :845
        self.layers = nn.ModuleList([_LlamaBlock(embed_dim, n_heads, n_kv_heads, multiple_of, ffn_dim_multiplier, norm_eps)
                                     for _ in range(n_layers)])                          # :848-852
        self.norm = _RMSNorm(embed_dim, norm_eps)                                        # :854
        # precompute_freqs_cis (llama.py:41-60) as [cos (32) | sin (32)] per position instead of complex64; a plain attribute, not a
        # buffer, like the reference's precomputed_freqs_cis (fast3r.py:837)
        hd = embed_dim // n_heads
        freqs = 1.0 / (rope_theta ** (torch.arange(0, hd, 2)[: hd // 2].float() / hd))
        ang = torch.outer(torch.arange(max_seq_len).float(), freqs).float()
        self.image_idx_emb = torch.cat([ang.cos(), ang.sin()], dim=1)

    def attention_scale(self, training: bool) -> float:
        return (self.embed_dim // self.num_heads) ** -0.5  # F.scaled_dot_product_attention default (llama.py:239)

    draw_image_ids = Fast3RDecoder.draw_image_ids  # same RNG recipe (fast3r.py:856-897 == :702-743)


# within a 64-wide head: destination position -> source dim, so that the reference's complex pairs (2j, 2j+1) land where the QKV
# epilogue rotates (rope_mode 1: dims [0,32) pair i with i+16 using table columns 0-15, dims [32,64) likewise with columns 16-31).
# The same permutation on q and k leaves every q . k unchanged.
_ROPE_PERM = [2 * j for j in range(16)] + [2 * j + 1 for j in range(16)] + [2 * j for j in range(16, 32)] + [2 * j + 1 for j in range(16, 32)]


class _RCU(_Params):
    def __init__(self, f):
        super().__init__()
        self.conv1 = nn.Conv2d(f, f, 3, padding=1)  # dpt_block.py:105-123
        self.conv2 = nn.Conv2d(f, f, 3, padding=1)


class _Fusion(_Params):
    def __init__(self, f):
        super().__init__()
        self.out_conv = nn.Conv2d(f, f, 1)  # dpt_block.py:180-188
        self.resConfUnit1 = _RCU(f)
        self.resConfUnit2 = _RCU(f)


class _DPT(_Params):
    """Parameter layout of DPTOutputAdapter_fix (heads/dpt_head.py:28-40; croco/models/dpt_block.py:315-490)."""

    def __init__(self, num_channels, feature_dim, last_dim, hooks, dim_tokens, patch_size, layer_dims=(96, 192, 384, 768)):
        super().__init__()
        self.hooks, self.patch_size, self.num_channels = hooks, patch_size, num_channels
        self.feature_dim, self.last_dim, self.layer_dims = feature_dim, last_dim, list(layer_dims)
        ld = layer_dims
        scratch = _Params()
        for i in range(4):
            setattr(scratch, f"layer{i + 1}_rn", nn.Conv2d(ld[i], feature_dim, 3, padding=1, bias=False))
        scratch.layer_rn = nn.ModuleList([getattr(scratch, f"layer{i + 1}_rn") for i in range(4)])  # aliases
        for i in range(1, 5):
            setattr(scratch, f"refinenet{i}", _Fusion(feature_dim))
        self.scratch = scratch
        self.head = nn.Sequential(nn.Conv2d(feature_dim, feature_dim // 2, 3, padding=1), nn.Identity(),
                                  nn.Conv2d(feature_dim // 2, last_dim, 3, padding=1), nn.Identity(),
                                  nn.Conv2d(last_dim, num_channels, 1))
        self.act_postprocess = nn.ModuleList([
            nn.Sequential(nn.Conv2d(dim_tokens[0], ld[0], 1), nn.ConvTranspose2d(ld[0], ld[0], 4, stride=4)),
            nn.Sequential(nn.Conv2d(dim_tokens[1], ld[1], 1), nn.ConvTranspose2d(ld[1], ld[1], 2, stride=2)),
            nn.Sequential(nn.Conv2d(dim_tokens[2], ld[2], 1)),
            nn.Sequential(nn.Conv2d(dim_tokens[3], ld[3], 1), nn.Conv2d(ld[3], ld[3], 3, stride=2, padding=1)),
        ])


class PixelwiseTaskWithDPT(_Params):
    """heads/dpt_head.py:93-129 (parameters under `.dpt`)."""

    def __init__(self, *, hooks_idx, dim_tokens, num_channels, feature_dim, last_dim, patch_size, depth_mode, conf_mode):
        super().__init__()
        self.depth_mode, self.conf_mode = depth_mode, conf_mode
        self.dpt = _DPT(num_channels, feature_dim, last_dim, hooks_idx, dim_tokens, patch_size)

