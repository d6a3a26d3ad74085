/*
 * f3r.h -- C ABI of libf3r_hip.so: the MI355X (gfx950 / CDNA4) kernels behind the Fast3R
 * single-forward-pass inference hot path
 *     fast3r/dust3r/inference_multiview.py:70-99  inference()
 *       -> fast3r/models/fast3r.py:302-497        Fast3R.forward
 *
 * The reference has exactly one native binding, the pybind `curope.rope_2d(tokens, positions,
 * base, fwd)` (fast3r/croco/models/curope/curope.cpp:49-69); everything else it computes through
 * torch ops (nn.Linear / Conv2d / LayerNorm / SDPA / F.interpolate).  This header is what a
 * from-scratch native backend for the same path binds instead: one entry point per fused op,
 * plain device pointers + sizes, no torch types.  Each entry cites the reference code it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (the PyTorch-ROCm allocator); the
 *     library allocates nothing and keeps no mutable state except the calling thread's last-error
 *     string (kernel choices that used to be process-wide knobs are per-call fields: f3r_gemm_args.kernel_sel);
 *   - every launch is asynchronous on the caller's `stream` (unlike the reference extension,
 *     which launches on the legacy default stream: curope/kernels.cu:102);
 *   - return value: F3R_OK (0) or a negative f3r_status; nothing throws across the boundary.
 *     The Python host (fast3r_amd/_lib.py) maps errors onto the exception types the reference
 *     raises (ValueError / AssertionError / RuntimeError);
 *   - "lowp" = the 16-bit MFMA operand type selected by `dtype` (F3R_F16 or F3R_BF16);
 *     accumulation, residual stream, LayerNorm statistics, softmax and post-processing are fp32.
 */
#ifndef F3R_H_
#define F3R_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* f3r_stream_t; /* hipStream_t */

typedef enum {
  F3R_OK = 0,
  F3R_ERR_ARG = -1,         /* bad argument (null pointer, bad size, misalignment) */
  F3R_ERR_UNSUPPORTED = -2, /* shape / mode not implemented by the kernels */
  F3R_ERR_LAUNCH = -3       /* hipGetLastError() after the launch was not hipSuccess */
} f3r_status;

typedef enum { F3R_F16 = 0, F3R_BF16 = 1 } f3r_dtype;
typedef enum { F3R_REAL_F32 = 0, F3R_REAL_F64 = 1 } f3r_real; /* element type of the pose-metric entry points and of the loss's camera poses */
typedef enum { F3R_LOSS_DIS = 0, F3R_LOSS_LOG1P = 1 } f3r_loss_dis_mode; /* avg_dis / avg_log1p of the multi-view loss */

#define F3R_MAX_SEG 8

/* library version (major*10000 + minor*100 + patch) and last error text of the calling thread */
int f3r_version(void);  /* 430 = 0.4.3 (+ f3r_render_clear, f3r_render_splat, f3r_render_resolve, f3r_render_center); 420 = 0.4.2 (+ f3r_cloud_combine_count, f3r_cloud_combine_write, f3r_cloud_bounds, f3r_cloud_voxel_workspace_bytes, f3r_cloud_voxel_sort, f3r_cloud_voxel_sums, f3r_cloud_fps_workspace_bytes, f3r_cloud_fps, f3r_cloud_mark, f3r_cloud_gather); 410 = 0.4.1 (+ f3r_mesh_threshold, f3r_mesh_count, f3r_mesh_write, f3r_mesh_ply_pack, f3r_mesh_workspace_bytes); 400 = 0.4.0 (+ f3r_sky_detect, f3r_sky_workspace_bytes); 390 = 0.3.9 (+ f3r_scene_*, f3r_ply_pack, f3r_color_range, f3r_color_to_u8); 380 = 0.3.8 (+ f3r_mv_conf_loss, f3r_mv_conf_loss_workspace_bytes); 370 = 0.3.7 (+ f3r_pose_pair_metrics, f3r_pose_error_stats); 360 = 0.3.6 (+ f3r_nn_*, f3r_estimate_normals, f3r_recon_stats, f3r_recon_prepare); 350 = 0.3.5, round 6 (F3R_SPLIT_X3F8, f3r_gemm_args.out_f8 / out_relu_f8 / fin_*, f3r_interp_bilinear_f8); 340 = 0.3.4, round 6 (+ f3r_block_workspace_bytes_ex; the library clears sched_counter per launch); 330 = 0.3.3, round 5 (f3r_attn_args.dbg_counters is uint32[8] incl. two clock sums; f3r_wall_clock_khz); 320 = 0.3.2, round 4 (+ f3r_attn_f32_mfma, head_dim 80 / 128 kernels); 310: f3r_attn_args.dbg_counters, f3r_gemm_args.kernel_sel 6; 300 = round 3; 200 = round 2 */
const char* f3r_last_error_string(void);
/* sizeof(f3r_gemm_args) (what == 0) / sizeof(f3r_attn_args) (what == 1) / sizeof(f3r_attn_f32_args) (what == 2): lets a foreign-language binding
   verify its struct layout before the first call; 0 for an unknown `what` */
size_t f3r_sizeof(int what);
/* rate of the constant clock s_memrealtime counts on the current device, in kHz (hipDeviceAttributeWallClockRate; 100 000 on MI355X); 0 on failure */
int f3r_wall_clock_khz(void);

/* ---------------------------------------------------------------------------------------------
 * f3r_patchify: fp32 NCHW image -> lowp im2col rows for the k=s=ps patch-embedding convolution.
 * Replaces the input side of PatchEmbedDust3R.forward's Conv2d (fast3r/dust3r/patch_embed.py:24-38,
 * fast3r/croco/models/blocks.py:412-415) and of DINOv2's PatchEmbed (DinoEncoder, fast3r/models/fast3r.py:561-651, ps = 14).
 * out[(b*h+py)*w+px][c*ps*ps+dy*ps+dx] = img[b][c][py*ps+dy][px*ps+dx] (the Conv2d weight's own (c,dy,dx) order, so
 * weight.view(D, 3*ps*ps) is the GEMM operand).  ld_out = row stride of `out` in elements (0 = 3*ps*ps; a multiple of 8;
 * columns >= 3*ps*ps are written as zeros: 3*14*14 = 588 is padded to 640 this way).
 */
int f3r_patchify(const float* img, void* out, int batch, int H, int W, int ps, int ld_out, int dtype, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_layernorm: rows of fp32 -> normalised lowp (GEMM operand) and/or fp32.
 * Replaces nn.LayerNorm in Block.forward (blocks.py:236-239), enc_norm (fast3r.py:558) and dec_norm
 * (fast3r.py:805).  Biased variance, y=(x-mu)/sqrt(var+eps)*gamma+beta; eps is 1e-6 or 1e-5 per
 * site (fast3r.py:509,683,700).  rms!=0: RMSNorm (no mean, no beta: components/llama.py:137-163).
 * D % 4 == 0.  out_lp / out_f32 may each be NULL.
 */
int f3r_layernorm(const float* x, const float* gamma, const float* beta, void* out_lp, float* out_f32,
                  int64_t rows, int D, float eps, int rms, int dtype, f3r_stream_t stream);
/* the same LayerNorm / RMSNorm writing the operand rows of F3R_SPLIT_W2F8 (f3r_split): out row r = [D fp16 | D fp8 e4m3 of the same values
   clamped to +-448], ld_out sixteen-bit elements apart (>= 3 D / 2, a multiple of 8).  fp16 only; D % 8 == 0. */
int f3r_layernorm_f8(const float* x, const float* gamma, const float* beta, void* out_rows, int64_t ld_out, int64_t rows, int D, float eps, int rms,
                     f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_gemm: out = epilogue( A(M,K) * W(N,K)^T ) on MFMA, fp32 accumulate.
 * Replaces every nn.Linear on the path (blocks.py:94-105 Mlp, :125-131,138,169 Attention qkv/proj,
 * fast3r.py:782 decoder_embed), the patch-embed Conv2d (as GEMM over f3r_patchify rows), and all
 * Conv2d / ConvTranspose2d of the DPT head (dpt_block.py:42-78,105-154,187-250,365-382,416-481).
 */
typedef enum { F3R_A_PLAIN = 0, F3R_A_CONV3X3 = 1 } f3r_a_mode;
typedef enum { F3R_EPI_GENERIC = 0, F3R_EPI_QKV = 1, F3R_EPI_CONVT = 2 } f3r_epi_mode;
typedef enum { F3R_ACT_NONE = 0, F3R_ACT_GELU = 1, F3R_ACT_RELU = 2 } f3r_act;

typedef struct f3r_gemm_args {
  /* operands */
  const void* A;     /* lowp. PLAIN: [M][lda].  CONV3X3: NHWC [B][conv_H][conv_W][conv_C] */
  const void* W;     /* lowp [N][Kpad] row-major, zero padded. PLAIN: k < K real.  CONV3X3: k = tap*Cpad + ci */
  const float* bias; /* [N] or NULL */
  int64_t M;         /* rows (tokens / output pixels) */
  int32_t N;
  int32_t K;         /* PLAIN: real K (multiple of 8).  CONV3X3: ignored */
  int32_t Kpad;      /* multiple of 64.  CONV3X3: 9*Cpad with Cpad = roundup(conv_C, 64) */
  int64_t lda;       /* PLAIN: row stride of A in elements */
  int32_t a_mode;    /* f3r_a_mode */
  int32_t a_relu;    /* ReLU applied to A as it is staged (the pre-activation of ResidualConvUnit_custom, dpt_block.py:143,148) */
  int32_t conv_H, conv_W, conv_C, conv_stride, conv_OH, conv_OW; /* CONV3X3 (pad 1): M = B*conv_OH*conv_OW */
  /* epilogue */
  int32_t epi;       /* f3r_epi_mode */
  int32_t act;       /* f3r_act, applied after bias */
  const float* rowadd; /* GENERIC: out += rowadd[m / rowadd_div][n] (image-index embedding, fast3r.py:799) or NULL */
  int64_t rowadd_div;
  const float* res_f32; /* GENERIC: fp32 residual [M][ldr_f32] or NULL (x + attn(..), x + mlp(..): blocks.py:237-238) */
  int64_t ldr_f32;
  const void* res_lp;   /* GENERIC: lowp residuals (skip_add of the RCU / fusion block, dpt_block.py:154,216) or NULL */
  int64_t ldr_lp;
  const void* res_lp2;
  int64_t ldr_lp2;
  float* out_f32;    /* GENERIC: fp32 output [M][ldo_f32] or NULL */
  int64_t ldo_f32;
  void* out_lp;      /* GENERIC: lowp output [M][ldo_lp] or NULL.  CONVT: NHWC [B][h*s][w*s][ct_cout] */
  int64_t ldo_lp;
  /* QKV epilogue (N = 3*D, D = heads*64): q -> [M][D], k -> [M][D], v -> transposed vt[m / seq_len][D][ldvt] at column m % seq_len */
  void* q;
  void* k;
  void* vt;
  int64_t seq_len;
  int64_t ldvt;
  const float* rope_cos; /* [n_pos][16] fp32 cos/sin of pos * 100^(-i/16) (pos_embed.py:139-150) or NULL = no RoPE (fusion decoder) */
  const float* rope_sin;
  int32_t rope_w;    /* tokens per image row: token p of a view sits at (y, x) = (p / rope_w, p % rope_w) (blocks.py:376-388) */
  float q_scale;     /* QKV: q (after bias and RoPE) is multiplied by this before rounding; 0 means 1.  The attention kernel
                        wants softmax_scale*log2(e) folded in here (f3r_attn_args.q_prescaled) */
  /* CONVT epilogue (ConvTranspose2d with kernel == stride == ct_s): rows m = (b, y, x) on a ct_h x ct_w grid,
     columns n = (dy*ct_s + dx)*ct_cout + co  ->  out_lp[b][y*ct_s+dy][x*ct_s+dx][co] */
  int32_t ct_s, ct_h, ct_w, ct_cout;
  int32_t dtype;     /* f3r_dtype */
  int32_t rope_mode; /* QKV with rope_cos != NULL.  0: RoPE-2D of the CroCo encoder as described above.  1: one rotation angle set per
                        ROW GROUP (LlamaDecoder, fast3r/models/components/llama.py:96-122 with freqs_cis gathered per view,
                        fast3r.py:872-922): rope_cos / rope_sin are [n_groups][32] (32 complex pairs of a 64-wide head), row m uses
                        group m / rope_w (rope_w = tokens per view, or 1 with one table row per token); the first 32 dims of a head
                        rotate with table columns 0-15 (dim i pairs with i+16), the last 32 with columns 16-31 -- the host permutes
                        the q / k weight rows so that the reference's interleaved pairs (2j, 2j+1) land on these positions */
  /* Split-precision operands (the "high" precision mode, DESIGN.md section 3 (Precision modes)): a value x is carried as two lowp numbers
     hi = lowp(x), lo = lowp(x - hi) (~22 significand bits with fp16 pieces) and the product is summed over K SEGMENTS on the same
     MFMA path (fp32 accumulate):  F3R_SPLIT_W2: A.W_hi + A.W_lo (weights exact to ~2^-22, activations single);
     F3R_SPLIT_X3: A_hi.W_hi + A_hi.W_lo + A_lo.W_hi.  With split != 0, W is [N][2][Kpad/2] (plane 0 = hi, plane 1 = lo; Kpad is still
     the row stride, K the real depth of ONE plane) and, for X3, A_lo is the low plane of A (same layout / strides as A). */
  int32_t split;     /* f3r_split */
  int32_t kernel_sel; /* 0 = pick the kernel by shape; 1 = 128x128-tile kernel; 2 / 3 = 256x256-tile kernel with / without staggered wave rows;
                         4 = its 256x128 tile form; 5 = 256x256 with one tile per workgroup instead of the persistent grid (2 - 5 are for
                         measurement: an ineligible shape is F3R_ERR_ARG, never a silent fallback);
                         6 = the hand-scheduled one-wave-per-SIMD kernel (csrc/asm/gemm_gen.py: 4 waves x 128 x 128 outputs of
                         v_mfma_f32_32x32x16, five-slot LDS-DMA ring; ABI 310).  It takes plain GEMMs with the GENERIC epilogue, M and N multiples
                         of 256, K == Kpad (split NONE or W2), ONE output: fp32 (+ bias, + fp32 residual, no activation) or lowp (+ bias,
                         + GELU / ReLU), or F3R_EPI_QKV without rotary embedding and equal q / k / v widths (two launches) -- F3R_ERR_UNSUPPORTED otherwise.
                         0 uses it for eligible launches whose 256 x 256 tiles fill its persistent grid (>= one tile per CU, last round >= 80 % full);
                         7 = pick by shape among the compiler-scheduled kernels only;
                         9 = like 6 but WITH a start-up skew of the persistent workgroups (measurement only, round 5: workgroup b of a launch with >= 2
                         tiles per workgroup starts ((b / 8) % 4) quarter tile periods late, so that the epilogues' HBM traffic of one quarter of the
                         chip overlaps the K loops of the rest; measured 6 % SLOWER on fc2, neutral elsewhere -- lock-step workgroups share their
                         operand panels through L2 -- hence not the default) */
  const void* A_lo;
  /* low planes of the lowp outputs / residuals (NULL = not carried): out_lp_lo = lowp(v - float(out_lp)); res_lp*_lo are added like
     their high planes.  Same leading dimensions as the high planes. */
  void* out_lp_lo;
  const void* res_lp_lo;
  const void* res_lp2_lo;
  /* GENERIC: second lowp output relu(v) [M][ldo_lp] (+ its low plane): the pre-activated copy the next ResidualConvUnit conv reads
     (dpt_block.py:143,148), so that conv needs no a_relu and can stage its operand by LDS-DMA */
  void* out_relu;
  void* out_relu_lo;
  /* QKV epilogue with grouped-query attention (LlamaDecoder n_kv_heads < n_heads, components/llama.py:195-198,220-232): the N columns are
     [ q: qkv_dq | k: (N - qkv_dq) / 2 | v: (N - qkv_dq) / 2 ], q -> [M][qkv_dq], k -> [M][Dkv], v -> vt[m / seq_len][Dkv][ldvt].
     0 = three equal thirds (N / 3 each).  Both widths must be multiples of 64 (whole heads). */
  int32_t qkv_dq;
  /* F3R_SPLIT_W2F8 with act = GELU and out_lp (ABI 330; was reserved): != 0 = the rows of out_lp are [N fp16 | N fp8] (ldo_lp >= 3 N / 2) and the
     epilogue also writes the fp8 (e4m3, clamped to 448) copy of its output N sixteen-bit elements into the row: the A operand of the NEXT
     W2F8 GEMM (fc1 -> fc2 of a transformer MLP, blocks.py:94-105) */
  int32_t out_lp_f8;
  const uint32_t* w_scale; /* F3R_SPLIT_W2F8: [N] scale words of the weight rows' fp8 plane (see f3r_split); NULL otherwise (ABI 330) */
  /* F3R_EPI_QKV with F3R_SPLIT_W2F8 (ABI 330): W / w_scale hold the q and k rows only ([N - Dkv] rows of [K fp16 | K fp8]); the v rows come as TWO
     fp16 planes here ([Dkv][2 K], as F3R_SPLIT_W2 packs them): the V^T launch runs with swapped operand roles on the fp16 kernel (its "weights"
     are the activations).  NULL otherwise. */
  const void* W_aux;
  /* ABI 350 (round 6).  fp8 COPIES of the lowp outputs for the next F3R_SPLIT_X3F8 convolution (GENERIC epilogue; NULL = not written): row m of
     out_f8 is 2 N bytes [ e4m3(clamp(v, +-448)) x N | e4m3(clamp((v - float(fp16(v))) 2^12, +-448)) x N ] for the values v that out_lp rounds;
     out_relu_f8 the same for relu(v) (what out_relu carries).  fp16 only, N % 8 == 0, 8-byte aligned. */
  void* out_f8;
  void* out_relu_f8;
  /* ABI 350: the tail of the DPT head fused into the epilogue of its last 3x3 convolution (head[2] + ReLU -> head[4] 1x1 conv -> postprocess,
     dpt_block.py:375-381, heads/postprocess.py:16-64): with fin_w != NULL the launch must be a CONV3X3 whose N <= 128 output channels lie in ONE
     256 x 128 tile of the 256-tile kernel (N % 128 == 0 today: the DPT head's last_dim = 128); the epilogue applies `act` to the fp32
     accumulators, multiplies them by fin_w (fp32 [4][N], rows >= fin_n_out zero) + fin_b (fp32 [4]) on the vector pipe and writes
     fin_pts (fp32 [M][3]) / fin_conf (fp32 [M] or NULL) exactly as f3r_dpt_final does (fin_depth_mode / fin_conf_mode / fin_vmin / fin_vmax: its
     arguments).  No lowp output is written then (out_lp may be NULL): the 128-channel activation never reaches HBM.  F3R_ERR_UNSUPPORTED when the
     launch cannot take the 256 x 128 tile form. */
  const float* fin_w;
  const float* fin_b;
  float* fin_pts;
  float* fin_conf;
  int32_t fin_n_out, fin_depth_mode, fin_conf_mode;
  float fin_vmin, fin_vmax;
  int32_t reserved0;
} f3r_gemm_args;

/* F3R_SPLIT_W2F8 (ABI 330): W2 with the LOW plane of the weights, and the copy of the activations it multiplies, in fp8 (OCP e4m3) on the
   block-scaled MFMA of gfx950 (v_mfma_scale_f32_32x32x64_f8f6f4: 1.40x the matrix-pipe rate of the two-fp16-plane form under the power cap,
   profiles/r05_ubench_mfma_mixed_fp16_fp8_fp6.jsonl): A(M, K) rows are [K fp16 | K fp8] (lda >= 3 K / 2 sixteen-bit elements; the fp8 copy holds
   the same numbers clamped to +-448: f3r_layernorm_f8 writes such rows), W rows are [K fp16 hi | K fp8 e4m3((W - hi) 2^s_n)] (row stride 3 K
   bytes: Kpad = K, a multiple of 128) with one power-of-two scale per output channel in w_scale (E8M0 byte 127 - s_n replicated into the four
   bytes of a word).  The correction term A W_lo is 2^-11 of the product and tolerates the 2^-4 relative error of both fp8 operands: the
   weight's rounding error drops ~24x instead of vanishing (tools/emu_gemm.py run_case_f8).  fp16 operands, plain A, GENERIC epilogue with ONE
   output (as kernel_sel 6), M and N multiples of 256 -- anything else is F3R_ERR_UNSUPPORTED (there is no second kernel for this layout). */
/* F3R_SPLIT_X3F8 (ABI 350; the 3x3 convolutions of the DPT head, dpt_block.py:133-154,365-382): X3 whose two CORRECTION products run on the
   block-scaled fp8 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4): A_hi W_hi on fp16 + A_hi8 W_lo8 + A_lo8 W_hi8 -- two matrix-pipe units instead of
   three (each correction is 2^-11 of the product and tolerates the 2^-4 relative error of both fp8 operands; oracle/precision_study.py --study
   heads_f8: the stress fixture moves from 6.94e-4 to 6.93e-4).  CONV3X3 only, stride 1, conv_C % 128 == 0, fp16, the 256-tile kernel
   (F3R_ERR_UNSUPPORTED otherwise).  A = the fp16 high plane (NHWC); A_lo = the fp8 planes of the same tensor, per pixel [C bytes e4m3(hi, clamped to
   +-448) | C bytes e4m3(lo 2^12, clamped)] (what out_f8 / f3r_interp_bilinear_f8 write); W rows are [9 C fp16 hi | 9 C bytes e4m3(w_lo 2^s_n) |
   9 C bytes e4m3(w_hi 2^t_n)] (4 * 9 C bytes: Kpad = 2 * 9 C as for X3, k = tap * C + ci in every plane) and w_scale[n] holds the E8M0 bytes
   127 - s_n (byte 0) and 127 - t_n (byte 1) (ops.pack_conv3x3_weight_f8). */
typedef enum { F3R_SPLIT_NONE = 0, F3R_SPLIT_W2 = 1, F3R_SPLIT_X3 = 2, F3R_SPLIT_W2F8 = 3, F3R_SPLIT_X3F8 = 4 } f3r_split;

int f3r_gemm(const f3r_gemm_args* args, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_block_workspace_bytes: size and layout of the intermediates of ONE transformer block (Block.forward, blocks.py:236-239) over
 * `tokens` rows = n_seq sequences of seq_len tokens, model width D, MLP hidden width `hidden` (2 x the SwiGLU width for the
 * LlamaDecoder's stacked [w1; w3] projection).  The library allocates nothing: the caller makes ONE allocation of the returned size
 * per encoder pass / decoder sample and every block of that pass reuses it (the intermediates of a block are dead when it ends).
 * offsets[0..4] (bytes, 256-byte aligned) = { LN output / attention output (lowp [tokens][D]),  q (lowp [tokens][D]),
 * k (lowp [tokens][kv_dim]),  V^T (lowp [n_seq][kv_dim][ldvt], ldvt = seq_len rounded up to 64: pad columns are never written, zero
 * them once; kv_dim = D, or n_kv_heads * 64 with grouped-query attention, or 0 when K / V^T live elsewhere -- the view-sharded path
 * writes them into the exchange buffers -- and the two regions are empty),
 * MLP hidden (lowp [tokens][hidden]) }.  Returns 0 on bad arguments.
 */
size_t f3r_block_workspace_bytes(int64_t tokens, int D, int kv_dim, int hidden, int64_t n_seq, int64_t seq_len, size_t offsets[5]);
/* ABI 340: the same layout for passes that run the F3R_SPLIT_W2F8 GEMMs (f8_rows != 0): regions 0 and 4 are sized for rows [w fp16 | w fp8]
   (3 w bytes per row, w = D / hidden; both multiples of 8) -- what f3r_layernorm_f8 and the GELU epilogue (out_lp_f8) write -- and the plain
   [tokens][w] 16-bit forms of the same intermediates (attention output; a hidden state kept on fp16 planes) alias the head of those regions: the
   wide and the plain form of a region are never live at the same time inside a block.  f8_rows = 0 is f3r_block_workspace_bytes. */
size_t f3r_block_workspace_bytes_ex(int64_t tokens, int D, int kv_dim, int hidden, int64_t n_seq, int64_t seq_len, int f8_rows, size_t offsets[5]);

/* ---------------------------------------------------------------------------------------------
 * f3r_attn_fwd: O = softmax(scale * Q K^T) V, head_dim 64 (other widths: f3r_attn_args.head_dim), flash-style (never forms
 * the T x T matrix), fp32 online softmax.  Replaces the q@k^T -> softmax -> @v core of
 * Attention.forward (blocks.py:158-190; all three `attn_implementation`s compute this).
 * K/V arrive as up to F3R_MAX_SEG segments so that the view-sharded multi-GPU path can attend
 * over the local shard plus the all-gathered remote shards without concatenating them.
 *   q  : [batch][tq][ldq]   (head h at columns h*64 .. h*64+63)
 *   k_seg[s]  : [batch][seg_len[s]][ldk]
 *   vt_seg[s] : [batch][heads*64][ldvt[s]]  (V transposed, as written by the F3R_EPI_QKV epilogue)
 *   o  : [batch][tq][ldo]
 *
 * What a launch may touch (every kernel form; tests/test_attn_geometry_gpu.py holds each of them to it with every buffer between NaN patterns
 * and sentinel words):
 *   q      read: rows [0, tq) of each sequence, columns [0, n_heads * head_dim * planes) (planes = 2 with qk_planes 2 / 3, else 1).  Never the gap
 *          columns up to ldq, the rows between two sequences when q_batch_stride > tq * ldq, or anything before / behind the buffer.
 *   k_seg  read: rows [0, seg_len[s]) of each sequence, the columns of the K / V heads.  Never a row behind seg_len[s] or a gap column.
 *   vt_seg read: rows [0, kv_heads * head_dim), columns [0, round_up(seg_len[s], 64)); the caller zeroes [seg_len[s], round_up(seg_len[s], 64)).
 *          Columns from round_up(seg_len[s], 64) to ldvt[s] are never read (a short segment next to a long one under one ldvt has such columns).
 *   o      written: rows [0, tq) x columns [0, n_heads * head_dim) of each sequence, nothing else; with state_out, nothing at all.
 *   st_o / st_ml  read (state_in) and written (state_out): rows [0, batch * tq), nothing else.
 */
typedef struct f3r_attn_args {
  const void* q;
  void* o;
  int64_t ldq, ldo;
  int64_t q_batch_stride, o_batch_stride; /* elements */
  int64_t tq;
  int32_t batch;
  int32_t n_heads;
  int32_t n_seg;
  int32_t dtype;
  const void* k_seg[F3R_MAX_SEG];
  const void* vt_seg[F3R_MAX_SEG];
  int64_t seg_len[F3R_MAX_SEG];
  int64_t ldvt[F3R_MAX_SEG];
  int64_t ldk;
  int64_t k_batch_stride[F3R_MAX_SEG];  /* elements */
  int64_t vt_batch_stride[F3R_MAX_SEG]; /* elements */
  float scale; /* 0.125, or 0.160192 for the fusion decoder in eval mode (blocks.py:119-124,151-154) */
  int32_t q_prescaled; /* != 0: q was already multiplied by scale*log2(e) (F3R_EPI_QKV with q_scale) before its one
                          rounding to lowp, so the kernel exponentiates with exp2 directly; `scale` is then unused */
  /* Online-softmax state carried between launches over different K/V segments of the SAME queries (view-sharded path:
     launch 1 attends over the local shard while the all-gather of the remote shards is in flight and writes the state,
     launch 2 resumes from it over the remote shards and writes the normalised output).
       st_o  : fp32 [batch][tq][n_heads*64]   un-normalised O accumulators
       st_ml : fp32 [batch][tq][n_heads][4]   {running max, partial row sum of lane half 0, of lane half 1, unused}
     state_in != 0: start from the state instead of (O=0, m=-inf, l=0).  state_out != 0: write the state and NOT o. */
  float* st_o;
  float* st_ml;
  int32_t state_in;
  int32_t state_out;
  /* Grouped-query attention (repeat_kv, components/llama.py:125-134,229-232): query head h reads K / V head h / kv_group; the K rows
     and V^T planes then hold n_heads / kv_group heads.  0 or 1 = one K / V head per query head. */
  int32_t kv_group;
  /* Causal attention (F.scaled_dot_product_attention(..., is_causal=True), components/llama.py:239): key at sequence position j is
     visible to the query at position i iff j <= i.  Positions are GLOBAL token indices: query row r of this launch sits at
     q_pos0 + r, key row r of segment s at seg_pos0[s] + r (the view-sharded path attends over shards that start anywhere).
     One precondition: a launch WITHOUT state_in must see its first key from every query row -- seg_pos0[first non-empty segment] <= q_pos0;
     anything else is F3R_ERR_ARG.  The kernel takes its first softmax reference from the first key tile, and a row with nothing visible there
     would take it from the mask value.  A sharded caller therefore starts from the shard that holds its queries (its first key sits AT q_pos0)
     and resumes (state_in) over the other shards in any order, hidden ones included. */
  int32_t causal;
  int64_t q_pos0;
  int64_t seg_pos0[F3R_MAX_SEG];
  /* Kernel choice (per call, like f3r_gemm_args.kernel_sel; no process-wide switch):
       0 = automatic: the hand-scheduled one-wave-per-SIMD kernel (csrc/asm/attn_gen.py: 512-query workgroups, 128 queries per
           wave; a partial last workgroup is fine) when the launch is eligible -- no causal mask, q_prescaled, tq >= 128, every non-empty K/V segment a
           multiple of 64 keys with one ldvt and one pair of batch strides, at least F3R_ATTN_ASM_MIN_KEYS keys in total, kv_group a
           power of two, batch 1 when the softmax state is carried (state_in / state_out; the state layout is the HIP kernel's, so
           the two kernels can resume each other's launches) -- and the general HIP kernel otherwise;
       1 = the general HIP kernel;  2 = the hand-scheduled kernel (F3R_ERR_UNSUPPORTED if the launch is not eligible).
     Under 0 and 2 alike, a launch on 512-query items over at least F3R_ATTN_GROUPED_MIN_KEYS keys runs f3r_attn_asm_*_grp: the same arithmetic per
     wave (results bit for bit those of f3r_attn_asm_*), one s_barrier per group of key tiles on an 8-slot LDS ring instead of one per tile. */
  int32_t kernel_sel;
  /* Width of a head: 0 or 64 = the tuned kernels; any other multiple of 16 up to 128 (the reference's Attention takes any dim //
     num_heads, blocks.py:113-143; its model_scaling_huge.yaml fusion decoder has 80): same layouts with head_dim columns per head
     (q / k / o rows, head_dim V^T planes per head, st_o rows of n_heads * head_dim), no causal mask.  80 and 128 have hand-scheduled
     kernels of their own (csrc/asm/attn_gen.py: 256-query workgroups, 64 queries per wave; eligibility as for kernel_sel 0 below
     with tq >= 64 and NO minimum number of keys: they beat the generic kernel from 128 keys on,
     profiles/r04_attn_head_dim_short_sequences.jsonl); everything else, and launches those kernels cannot take, run the generic kernel
     (f3r_attn_generic.hip). */
  int32_t head_dim;
  /* Optional counters of the hand-scheduled kernel (NULL = none; ABI 310, widened in ABI 330): device uint32[56], 8-byte aligned, zeroed by the
     caller; every wave of a launch that takes that kernel adds {entries into the block that moves the softmax reference (the forced first
     one included), 1} and, as three uint64 at bytes 8, 16 and 24, {64-key tiles it walked, shader-clock cycles (s_memtime) the wave lived,
     ticks of the constant-rate clock (s_memrealtime, f3r_wall_clock_khz) over the same span}, followed from byte 32 on by the
     same sums per XCD (8 records of three uint64: cycles, ticks, waves; the XCD is read from HW_REG_XCC_ID).  bench.py reports (entries - waves) / waves
     (how often the lazy reference really moved) and, from the clocks, the effective shader clock and the matrix-pipe utilisation of the
     timed launches themselves (roofline.live). */
  uint32_t* dbg_counters;
  /* Work stealing for the hand-scheduled kernels (NULL = off; ABI 330): device uint32[2] {next item, workgroups done}.  The library clears the two
     words on `stream` ahead of every launch that uses them (since round 6; the kernel also leaves them zero), so one buffer serves any number of
     launches that do not overlap in time -- one buffer per stream, and per captured graph if graphs may replay concurrently: two launches in
     flight on the same pair would steal each other's items.
     With it, launches of at least two rounds of workgroups run as ONE persistent workgroup per CU that takes (query block, head, batch)
     items from `next`: the hardware deals workgroup ids round-robin over the 8 XCDs whatever their clocks (up to 6 % apart under the power
     cap), which left the faster XCDs idle for ~2.4 % of every fusion-attention launch (profiles/r05_*per_xcd*).  Other launches ignore it. */
  uint32_t* sched_counter;
  /* Operand planes of Q and K (ABI 340, precision "robust"): 0 / 1 = one 16-bit number per element, as described above.  3 = like 2 with the two
     CORRECTION products on the block-scaled fp8 MFMA: a head of a q / K row is [hi fp16 (128 bytes) | e4m3(hi) (64 bytes) | e4m3(lo 2^12) (64 bytes)]
     (f3r_qkv_planes with planes = 3; the same 256 bytes per head) and a score block is q_hi k_hi on fp16 + q_lo8 k_hi8 + q_hi8 k_lo8 on
     v_mfma_scale_f32_32x32x64_f8f6f4 (kernel f3r_attn_asm_qk3f8_f16: 256 matrix-pipe cycles per block instead of 384; the fp8 copies move the
     softmax by ~2e-5, csrc/asm/attn_gen.py corr = "f8").  2 = every head of a q row
     and of a K row holds [hi (64) | lo (64)] fp16 (x = hi + lo to ~22 bits; f3r_qkv_planes writes such rows): ldq / ldk / the batch strides count
     elements of these 128-wide heads (ldq >= n_heads * 128), and the scores are q_hi k_hi + q_lo k_hi + q_hi k_lo with fp32 accumulation -- three
     MFMA products per score block, P V unchanged (V^T, o, the parked state: head_dim 64 layouts).  Only the hand-scheduled kernel
     f3r_attn_asm_qk3_f16 reads this layout (csrc/asm/attn_gen.py AttnGen(qk_planes = 2): 256-query workgroups): fp16, head_dim 64, q_prescaled, and
     the eligibility rules of kernel_sel 0 with tq >= 64 and no minimum number of keys -- anything else is F3R_ERR_UNSUPPORTED, never a fallback.
     These kernels carry the softmax state at ANY batch: sequence z owns rows [z tq, (z + 1) tq) of st_o / st_ml. */
  int32_t qk_planes;
  /* Compute units the persistent (work-stealing) form leaves FREE (ABI 340; 0 = none; needs sched_counter).  The hand-scheduled kernels hold a
     CU completely -- one 488-register wave per SIMD -- so while a launch of one persistent workgroup per CU runs, no other kernel of more than a
     few registers can become resident anywhere on the chip until it ends.  A view-sharded rank launches its local-shard attention next to the
     RCCL kernels (or copy kernels) that move the other ranks' K / V^T: with reserve_cus = r the launch runs cus - r persistent workgroups
     (whenever it has more work items than that), so a kernel that arrives late still finds r CUs -- at the price of r / cus of this launch's rate
     (tools/ubench/exchange_overlap.hip measures both sides: profiles/r06_exchange_under_persistent_attention.json). */
  int32_t reserve_cus;
} f3r_attn_args;
#define F3R_ATTN_ASM_MIN_KEYS 2048
#define F3R_ATTN_GROUPED_MIN_KEYS 8192

int f3r_attn_fwd(const f3r_attn_args* args, f3r_stream_t stream);
/* which kernel f3r_attn_fwd takes for `args` (a static string; reporting only) */
const char* f3r_attn_kernel_name(const f3r_attn_args* args);

/* ---------------------------------------------------------------------------------------------
 * f3r_upsample2x: bilinear x2, align_corners=True, NHWC lowp -> NHWC lowp.
 * Replaces F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) in
 * FeatureFusionBlock_custom.forward (dpt_block.py:238-243) and the head's Interpolate (:374).
 * The output may be cropped to (out_h, out_w) <= (2h, 2w) (refinenet4 crop, dpt_head.py:69-71).
 * in_lo / out_lo: optional low planes (split precision, see f3r_gemm_args.split): the input is in + in_lo, the output is
 * written as hi = lowp(y), lo = lowp(y - hi).  Either may be NULL.
 */
int f3r_upsample2x(const void* in, const void* in_lo, void* out, void* out_lo, int batch, int h, int w, int C, int out_h, int out_w,
                   int dtype, f3r_stream_t stream);
/* f3r_interp_bilinear: the same kernel for any nominal output size (full_h, full_w) >= (out_h, out_w): F.interpolate(size or
 * scale_factor, mode="bilinear", align_corners=True), src = dst * (in - 1) / (full - 1).  The head's Interpolate(scale_factor =
 * patch_size / 8) (dpt_block.py:374) is x2 for patch 16 and x1.75 for DINOv2's patch 14. */
int f3r_interp_bilinear(const void* in, const void* in_lo, void* out, void* out_lo, int batch, int h, int w, int C, int full_h, int full_w,
                        int out_h, int out_w, int dtype, f3r_stream_t stream);
/* ABI 350: the same with an optional fp8 copy of the output for the next F3R_SPLIT_X3F8 convolution: out_f8 (NULL = none) is
   [batch][out_h][out_w][2 C] bytes, per pixel [C bytes e4m3(y clamped to +-448) | C bytes e4m3((y - float(fp16(y))) 2^12, clamped)] (f3r_gemm_args.out_f8
   describes the same layout).  fp16 only when out_f8 is given. */
int f3r_interp_bilinear_f8(const void* in, const void* in_lo, void* out, void* out_lo, void* out_f8, int batch, int h, int w, int C, int full_h,
                           int full_w, int out_h, int out_w, int dtype, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_dpt_final: last 1x1 conv (Cin -> n_out) fused with postprocess.
 * Replaces head[4] Conv2d(last_dim, 3 + has_conf, 1) (dpt_block.py:379-381) + postprocess / reg_dense_depth /
 * reg_dense_conf (heads/postprocess.py:16-64):
 *   xyz,c = W(n_out,Cin) x + b;  d = |xyz|
 *   depth_mode  F3R_DEPTH_EXP    pts = xyz / max(d, 1e-8) * expm1(d)      ('exp', -inf, inf): the released configuration
 *               F3R_DEPTH_LINEAR pts = xyz                                 ('linear', -inf, inf)
 *               F3R_DEPTH_SQUARE pts = xyz / max(d, 1e-8) * d^2            ('square', -inf, inf)
 *               (the reference asserts the depth bounds are infinite, postprocess.py:33-34)
 *   conf_mode   F3R_CONF_EXP     conf = vmin + min(exp(c), vmax - vmin)    ('exp', vmin, vmax)
 *               F3R_CONF_SIGMOID conf = (vmax - vmin) sigmoid(c) + vmin    ('sigmoid', vmin, vmax)
 *   x (+ x_lo, optional low plane): NHWC lowp [npix][Cin];  w: fp32 [n_out][Cin];  b: fp32 [n_out];  n_out = 3 (no confidence:
 *   conf must be NULL) or 4;  pts3d: fp32 [npix][3];  conf: fp32 [npix] or NULL
 */
typedef enum { F3R_DEPTH_EXP = 0, F3R_DEPTH_LINEAR = 1, F3R_DEPTH_SQUARE = 2 } f3r_depth_mode;
typedef enum { F3R_CONF_EXP = 0, F3R_CONF_SIGMOID = 1 } f3r_conf_mode;
int f3r_dpt_final(const void* x, const void* x_lo, const float* w, const float* b, int n_out, float* pts3d, float* conf, int64_t npix,
                  int Cin, int depth_mode, int conf_mode, float conf_vmin, float conf_vmax, int dtype, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_cast_f32_to_lp: fp32 -> lowp copy (hooked residual streams 12/18 as DPT inputs, dpt_head.py:54;
 * weight packing).  out_lo (optional): the low plane lowp(x - float(out)) of the split-precision operand format.
 */
int f3r_cast_f32_to_lp(const float* in, void* out, void* out_lo, int64_t n, int dtype, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_align_local_to_global: similarity alignment of the local pointmap of every (view, sample) to its global pointmap.
 * Replaces MultiViewDUSt3RLitModule.align_local_pts3d_to_global (fast3r/models/multiview_dust3r_module.py:427-549), i.e. per
 * problem p of npix pixels: thr = torch.quantile(conf, quantile) (:476); mask = conf >= thr & valid (:479-482), falling back
 * to valid alone below 3 points and to the identity below 3 valid points (:495-510); (R, t, s) =
 * roma.rigid_points_registration(local[mask], global[mask], compute_scaling=True) (:509-511; Umeyama); out = s*(local R^T) + t (:514).
 *   conf [n_prob][npix] fp32, pts_local / pts_global / out [n_prob][npix][3] fp32, valid_mask [n_prob][npix] bytes or NULL,
 *   rts [n_prob][13] fp32 = {R row-major (9), t (3), s}, thr_out [n_prob] fp32 or NULL,
 *   workspace: f3r_align_workspace_bytes(n_prob) bytes, 8-byte aligned.
 */
size_t f3r_align_workspace_bytes(int n_prob);
int f3r_align_local_to_global(const float* conf, const float* pts_local, const float* pts_global, const uint8_t* valid_mask,
                              float* out, float* rts, float* thr_out, void* workspace, size_t ws_bytes, int n_prob,
                              int64_t npix, float quantile, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_estimate_focal: robust focal length of every view from its pointmap + confidence.
 * Replaces estimate_focal (fast3r/models/multiview_dust3r_module.py:1081-1109): thr = torch.quantile(conf, quantile) (:1089-1093),
 * mask = conf >= thr (:1096), then the "weiszfeld" branch of estimate_focal_knowing_depth_and_confidence_mask
 * (fast3r/dust3r/post_process.py:77-142): closed-form start mean(xy/z . px) / mean(|xy/z|^2) (:121-128), n_iter re-weighted
 * least-squares steps with weights 1 / max(|px - f xy/z|, 1e-8) (:131-136; the reference uses 100), clip to
 * [min_focal, max_focal] x max(H, W) / (2 tan 30deg) (:140-142).  (ppx, ppy) is the principal point; the reference default is (W/2, H/2).
 *   pts3d [n_views][H][W][3] fp32, conf [n_views][H][W] fp32, focal [n_views] fp32, thr_out [n_views] fp32 or NULL,
 *   workspace: f3r_focal_workspace_bytes(n_views, H, W) bytes, 16-byte aligned.
 */
size_t f3r_focal_workspace_bytes(int n_views, int H, int W);
int f3r_estimate_focal(const float* pts3d, const float* conf, float* focal, float* thr_out, void* workspace, size_t ws_bytes,
                       int n_views, int H, int W, float quantile, float ppx, float ppy, int n_iter, float min_focal, float max_focal,
                       f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Reconstruction metrics (ABI 360): MultiViewDUSt3RLitModule.evaluate_reconstruction (fast3r/models/multiview_dust3r_module.py:551-735)
 * and accuracy / completion / completion_ratio (fast3r/eval/recon_metric.py:14-49).  Synchronous with the host where noted (they
 * read small results back), so they are not for graph capture.
 * f3r_nn_build: exact nearest-neighbour index over m fp32 points [m][3] (a uniform grid, points sorted by cell); index:
 *   f3r_nn_index_bytes(m) device bytes, 16-byte aligned; workspace: f3r_nn_workspace_bytes(m) bytes, 256-byte aligned.  The index
 *   keeps no pointer to pts.  NaN / inf coordinates -> F3R_ERR_ARG (the buffer then holds an empty index).  Synchronises the stream.
 * f3r_nn_query: for each of n fp32 query points, the nearest database point: dist [n] fp64 = sqrt(dx^2 + dy^2 + dz^2) of the
 *   fp32 coordinates in fp64 (scipy cKDTree.query), idx [n] int32, ties to the smaller index; an empty database gives inf and 0.
 *   workspace: f3r_nn_workspace_bytes(n).  NaN / inf query coordinates -> F3R_ERR_ARG.  Reads the index header back (synchronises
 *   the stream).
 * f3r_estimate_normals: the min(k, m) nearest database points of every database point (itself included; 1 <= k <= 64), in
 *   (distance, index) order -> knn_idx / knn_dist [m][k] (either may be NULL), and the normal of Open3D's
 *   PointCloud.estimate_normals() (fast_normal_computation) -> normals [m][3] fp64 (NULL = none): eigenvector of the smallest
 *   eigenvalue of the fp64 cumulant covariance, (0, 0, 1) below 3 neighbours; the sign is arbitrary.  pts is the array the index
 *   was built from.
 * f3r_recon_stats: out[5] fp64 (device) = { mean dist, median dist, mean dot, median dot, completion ratio } with
 *   dot[i] = |normals_q[i] . normals_db[idx[i]]| (NaN without normals; normals_db has m_db rows), medians as np.median, the ratio as
 *   np.mean((dist < dist_th).astype(np.float32)); n = 0 gives NaN.  workspace: f3r_recon_stats_workspace_bytes(n).
 * f3r_recon_prepare: the per-sample part of evaluate_reconstruction before the metrics.  Inputs are the views of every sample
 *   concatenated sample-major: sample i, view j covers pixels seg[i*n_views + j] .. seg[i*n_views + j + 1] (seg: device int64,
 *   n_samples*n_views + 1 entries, seg[i*n_views] = i*L) of conf [.] fp32, pred / gt [.][3] fp32, valid [.] bytes.  Per view:
 *   thr_m = torch.quantile(conf, q_metric), thr_icp = torch.quantile(conf, q_icp); kept = valid & conf >= thr_m.  Per sample, in
 *   view order: pred_out [i*L + r] = s (pred R^T) + t of the kept points, with (R, t, s) -> rts [i][13] the similarity
 *   registration of kept pred onto kept gt weighted by conf >= thr_icp (identity below 3 weighted points); gt_out [i*L + r] = gt
 *   of the valid points; counts [2][n_samples] int32 = { kept, valid }.  workspace: f3r_recon_prepare_workspace_bytes.
 */
size_t f3r_nn_index_bytes(int64_t m);
size_t f3r_nn_workspace_bytes(int64_t n);
int f3r_nn_build(const float* pts, int64_t m, void* index, size_t index_bytes, void* workspace, size_t ws_bytes, f3r_stream_t stream);
int f3r_nn_query(const void* index, const float* query, int64_t n, double* dist, int32_t* idx, void* workspace, size_t ws_bytes,
                 f3r_stream_t stream);
int f3r_estimate_normals(const void* index, const float* pts, int k, double* normals, int32_t* knn_idx, double* knn_dist, f3r_stream_t stream);
size_t f3r_recon_stats_workspace_bytes(int64_t n);
int f3r_recon_stats(const double* dist, const int32_t* idx, const double* normals_q, const double* normals_db, int64_t n, int64_t m_db,
                    double dist_th, double* out, void* workspace, size_t ws_bytes, f3r_stream_t stream);
size_t f3r_recon_prepare_workspace_bytes(int n_samples, int n_views, int64_t L);
int f3r_recon_prepare(const float* conf, const float* pred, const float* gt, const uint8_t* valid, const int64_t* seg, int n_samples,
                      int n_views, int64_t L, float q_metric, float q_icp, float* pred_out, float* gt_out, int32_t* counts, float* rts,
                      void* workspace, size_t ws_bytes, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_estimate_poses: camera pose (cam-to-world) and, when unknown, focal length of every view from its global pointmap.
 * Replaces the per-view body of MultiViewDUSt3RLitModule.estimate_camera_poses (fast3r/models/multiview_dust3r_module.py:807-869,
 * estimate_cam_pose_one_sample :1038-1078) = fast_pnp (fast3r/dust3r/cloud_opt/init_im_poses.py:300-350): mask = conf > conf_thr
 * (:1045 uses 1.0); fewer than 4 masked points -> failure (:302-303); focal_in[v] > 0 is used as is, otherwise the focal is searched
 * on np.geomspace(max(H,W)/2, 3 max(H,W), n_focals) (:312-316; the reference uses 100) by inlier count at 5 px (:335,:342);
 * result = inverse of the world-to-camera [R|T] (:349-350).  The reference solves with cv2.solvePnPRansac(iterationsCount = niter_PnP,
 * SQPNP); this library uses min(n_iter, 32) sampled closed-form DLT hypotheses + inlier DLT + gated Gauss-Newton (f3r_pnp.hip) -- same
 * contract (n_iter = the RANSAC iteration count), different solver.
 *   pts3d [n_views][H][W][3] fp32 (world frame), conf [n_views][H][W] fp32, focal_in [n_views] fp32 or NULL,
 *   focal_out [n_views] fp32 (NaN on failure), cam_to_world [n_views][4][4] fp32 row-major (identity on failure, :1062-1064),
 *   inliers [n_views] int32 (0 on failure).
 */
int f3r_estimate_poses(const float* pts3d, const float* conf, const float* focal_in, float* focal_out, float* cam_to_world, int* inliers,
                       int n_views, int H, int W, float conf_thr, float ppx, float ppy, int n_focals, int n_iter, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Relative camera-pose metrics (ABI 370): RRA / RTA / mAA of MultiViewDUSt3RLitModule.evaluate_camera_poses
 * (fast3r/models/multiview_dust3r_module.py:737-804) = camera_to_rel_deg + calculate_auc (fast3r/eval/cam_pose_metric.py:17-40,73-100)
 * over all view pairs i < j, without the reference's (pairs, 4, 4) tensors.
 * The pair-metrics entry point: pred / gt = cam-to-world matrices [n_samples][n_views][4][4] row-major, fp32 or fp64 (dtype: f3r_real).  Per pair,
 *   in fp64 on the exactly widened inputs: relative poses inv(P_i) P_j with the closed-form inverse (R^T, -R^T t); rotation error from
 *   cos = (trace(R_gt_rel R_pred_rel^T) - 1) / 2 with acos inside (-(1 - 1e-4), 1 - 1e-4) and its first-order extrapolation about the bound
 *   outside (fast3r/utils/so3_utils.py: identical rotations score 0.4051 degrees, not 0); translation error acos(sqrt(1 - loss)) with both
 *   vectors divided by (norm + 1e-15), loss = max(1 - dot^2, 1e-15), a NaN / inf error replaced by 1e6 rad (blind to sign: opposite
 *   translations score 0); both in degrees.
 *   counts [n_samples][n_r + n_t + n_bins + 2] int64 (device; cleared by the call) = { #(r < r_thresholds[k]) | #(t < t_thresholds[k]) |
 *   torch.histc(max(r, t), bins = n_bins, min = 0, max = max_threshold): bin = (int64)(m / max_threshold * n_bins), m == max_threshold in the
 *   last bin, m < 0, m > max_threshold and NaN dropped (the reference asks for 31 bins over [0, 30]: bin width 30 / 31) | #pairs whose trace
 *   lies outside [-1 - 1e-4, 3 + 1e-4] (the reference raises ValueError) | #pairs that took the 1e6 default }.
 *   rel_r / rel_t: optional (both or neither) per-pair errors [n_samples][n_views (n_views - 1) / 2] in the input dtype, pair (i, j) at
 *   i (2 n_views - i - 1) / 2 + (j - i - 1) -- the order of torch.combinations; with NULL nothing of size O(pairs) is written.
 *   r_thresholds / t_thresholds are HOST arrays (at most 8 each).  Integer atomics only: every output is deterministic.
 *   F3R_ERR_ARG before any launch: n_views < 2, n_samples < 1, null pred / gt / counts, more than 8 thresholds per kind, n_bins outside 1..256.
 * The error-stats entry point: the same counts [n_r + n_t + n_bins + 2] (the last two zero) from given per-pair errors r [n], t [n] (device, dtype as above):
 *   the body of calculate_auc and of the (x < tau).float().mean() threshold means.
 */
int f3r_pose_pair_metrics(const void* pred, const void* gt, int dtype, int n_samples, int n_views, const double* r_thresholds, int n_r,
                          const double* t_thresholds, int n_t, int n_bins, double max_threshold, void* rel_r, void* rel_t, int64_t* counts,
                          f3r_stream_t stream);
int f3r_pose_error_stats(const void* r, const void* t, int64_t n, int dtype, const double* r_thresholds, int n_r, const double* t_thresholds,
                         int n_t, int n_bins, double max_threshold, int64_t* counts, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The multi-view confidence loss of validation (ABI 380): ConfLossMultiviewV2(Regr3DMultiviewV3 | V4(L21Loss, "avg_dis" | "avg_log1p"), alpha)
 * (fast3r/dust3r/losses.py:404-848), forward only, as MultiViewDUSt3RLitModule.model_step calls it on a batch.
 * Tables: DEVICE arrays of n_views device pointers, one per view; view v has n_pixels[v] (device int64 table) pixels per sample, and the
 *   views may differ in that.  gt_pts [n_samples][n_pixels][3] fp32, valid_mask [n_samples][n_pixels] bytes (0 / 1), camera_pose
 *   [n_samples][4][4] cam-to-world in pose_dtype (f3r_real; fp64 is rounded to fp32 first, as the reference's .float() does), pred_pts /
 *   pred_conf = pts3d_in_other_view / conf, pred_pts_local / pred_conf_local = pts3d_local / conf_local (both NULL: no local head).
 *   Nothing is stacked, concatenated, compacted or written to; 16-byte loads are used where a sample's base addresses allow them.
 * Per pixel, in fp64 on the exactly widened inputs: g_glob = inv(P_view 0, b) x and g_loc = inv(P_v, b) x (general 4 x 4 inverse, top
 *   three rows, as geotrf applies them); with use_dist_clip the global set drops |g_glob| > dist_clip and the local set |g_loc| > dist_clip.
 *   Factors (each clipped to >= 1e-8, NaN kept): version 4 = per sample over all views the NaN-excluding mean of f(|.|) (global) and per
 *   (sample, view) (local; with local_scale_consistent the global ones); version 3 = one NaN-propagating mean over the whole batch (global)
 *   and one per view (local); f = identity (F3R_LOSS_DIS) or log1p (F3R_LOSS_LOG1P); gt_scale sets the ground truth's factors to 1.
 *   L = |pred / n_pred - gt / n_gt|; per view and set pts3d_loss = mean of L over the valid pixels of all samples (NaN without any) and
 *   conf_loss = mean of L conf - alpha log conf (exactly 0 without any); total = sum of the conf_losses / (number of them).
 * out (device, fp64) [1 + 4 n_views] = { total | pts3d_loss_global [n_views] | pts3d_loss_local | conf_loss_global | conf_loss_local }; the
 *   local parts are meaningless without a local head.  workspace: f3r_mv_conf_loss_workspace_bytes(n_views, n_samples) bytes, 8-byte
 *   aligned: O(workgroups + n_views n_samples), never O(pixels) (0 for a bad shape).  No floating-point atomics: partial sums are added
 *   in a fixed order, and two runs on one device give the same bits.
 * F3R_ERR_ARG before any launch: a null table, workspace or out; n_views < 1; n_samples < 1; alpha <= 0; an unknown version / dis_mode /
 *   pose_dtype; local_scale_consistent with version 3; one of the two local tables without the other; a workspace too small.
 */
size_t f3r_mv_conf_loss_workspace_bytes(int n_views, int n_samples);
int f3r_mv_conf_loss(const void* const* gt_pts, const void* const* valid_mask, const void* const* camera_pose, int pose_dtype,
                     const void* const* pred_pts, const void* const* pred_conf, const void* const* pred_pts_local,
                     const void* const* pred_conf_local, const int64_t* n_pixels, int n_views, int n_samples, int version, int dis_mode,
                     int gt_scale, int local_scale_consistent, int use_dist_clip, double dist_clip, double alpha, void* workspace,
                     size_t workspace_bytes, double* out, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Scene assembly and PLY export (ABI 390): the per-view body of the reference's viser visualizer (fast3r/viz/viser_visualizer.py:343-427,
 * :115-165, :168-254) -- np.argsort(-conf) with four gathers, the colourings, the extrema, the percentile scene extent, the prefix cut with
 * the sky mask and generate_ply_bytes -- on the device.  Python: fast3r_amd/scene.py.
 *
 * f3r_scene_sort: a segmented stable sort with fused gathers.  Every (view, head) is a segment.  `table` is a DEVICE int64 array:
 *   n_segments rows of 6 { conf pointer (len fp32), points pointer (len x 3 fp32), image pointer (3 planes of len fp32, values in [-1, 1]),
 *   mask pointer (len int8; 0 = no mask: all ones), len (1 <= len < 2^31), off (the segment's first slot in the outputs: the running sum of
 *   the lengths) }, then n_segments + 1 tile starts (the running sum of ceil(len / F3R_SCENE_TILE)); n_tiles and total_keys are the two totals.
 *   order[off + j] = np.argsort(-conf, kind='stable')[j]: descending confidence, equal values in pixel order, -0.0 == +0.0, +inf first, NaN
 *   last in pixel order.  pts / conf / mask = the inputs gathered by that order; rgb = trunc((img + 1) * 127.5) per plane, fp32 with one
 *   rounding per operation, packed to 3 bytes, saturated outside [0, 255]; conf_rgb = lut[index] with lut the 256 x 3 byte colour table on
 *   the device and index as matplotlib's Colormap.__call__ gives it for t = (c - min) / (max - min + 1e-8) in fp32 (t * 256 truncated, 256 ->
 *   255, NaN -> (0, 0, 0); a NaN anywhere in the segment makes every colour (0, 0, 0)).
 *   stats (device uint32 [n_segments][4]) = { key of the largest conf, key of the smallest, NaN count, count of mask > 0 } where
 *   key(c) = ~k(c), k the usual order-preserving map (sign bit set: ~bits, else bits | 2^31) of c with -0.0 read as +0.0; no non-NaN value:
 *   { 0xffffffff, 0 }.  Integer atomics only: two runs give the same bits.  Inputs are not written to.
 * f3r_scene_extent: the order statistics ranks[0..3] (HOST array, 0-based, ascending order) of each axis of pts [m][3] by exact radix
 *   select; out (device uint32 [15]) = 12 fp32 bit patterns [axis][rank] and the NaN count of each axis (-0.0 orders below +0.0; NaN
 *   orders by its bits and is for the caller to act on, as np.percentile returns NaN then).
 * f3r_scene_collect_count / f3r_scene_collect_write: `table` = n_segments rows of 5 { sorted points pointer, sorted colour pointer (3 bytes
 *   each; 0 = use the constant colour), sorted mask pointer (0 = keep all), num (entries taken from the front, >= 1), constant colour
 *   r | g << 8 | b << 16 }, then n_segments + 1 tile starts (running sum of ceil(num / 1024)).  _count writes the exclusive scan of the
 *   kept counts per tile to scan[0 .. n_tiles) and the total to scan[n_tiles]; _write places the kept entries, in order, at those slots
 *   of out_pts [total][3] fp32 and out_rgb [total][3] bytes.
 * f3r_ply_pack: n records of 15 bytes (xyz little-endian fp32, rgb) into out (4-byte aligned, 15 n rounded up to 4 bytes).
 * f3r_color_range: out (device uint64 [3]) = { key of the minimum, key of the maximum, NaN count } of n fp32 / fp64 (f3r_real) values
 *   widened to fp64, key = the 64-bit order-preserving map.  f3r_color_to_u8: safe_color_conversion's three rules in the input's own type
 *   (0: c * 255; 1: (c + 1) * 127.5; 2: ((c - lo) / (hi - lo)) * 255; clipped to [0, 255], truncated; F3R_ERR_ARG for rule 2 with hi == lo).
 */
#define F3R_SCENE_TILE 4096
size_t f3r_scene_sort_workspace_bytes(int64_t total_keys, int64_t n_tiles);
int f3r_scene_sort(const int64_t* table, int n_segments, int64_t n_tiles, int64_t total_keys, const uint8_t* lut, void* workspace,
                   size_t workspace_bytes, int32_t* order, float* pts, float* conf, uint8_t* rgb, uint8_t* conf_rgb, int8_t* mask,
                   uint32_t* stats, f3r_stream_t stream);
size_t f3r_scene_extent_workspace_bytes(void);
int f3r_scene_extent(const float* pts, int64_t m, const int64_t* ranks, void* workspace, size_t workspace_bytes, uint32_t* out,
                     f3r_stream_t stream);
int f3r_scene_collect_count(const int64_t* table, int n_segments, int64_t n_tiles, uint32_t* scan, f3r_stream_t stream);
int f3r_scene_collect_write(const int64_t* table, int n_segments, int64_t n_tiles, const uint32_t* scan, float* out_pts, uint8_t* out_rgb,
                            f3r_stream_t stream);
int f3r_ply_pack(const float* pts, const uint8_t* rgb, int64_t n, void* out, f3r_stream_t stream);
int f3r_color_range(const void* colors, int64_t n, int dtype, uint64_t* out, f3r_stream_t stream);
int f3r_color_to_u8(const void* colors, int64_t n, int dtype, int rule, double lo, double hi, uint8_t* out, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Sky detection (ABI 400): the reference's detect_sky_mask (fast3r/viz/viser_visualizer.py:24-72) for every view of a scene in one call.
 * Python: fast3r_amd/sky.py.  Per view, in the reference's order:
 *   1. u = trunc((img + 1) * 127.5) per channel (an fp32 add and an fp32 multiply; saturated outside [0, 255], NaN -> 0);
 *   2. OpenCV's 8-bit BGR2HSV (H in [0, 180), 12-bit fixed-point tables, rounding to nearest even);
 *   3. sky-coloured = H, S, V inside one of [105, 50, 140]-[135, 255, 255], [95, 5, 150]-[145, 100, 255], [0, 0, 235]-[180, 10, 255]
 *      (inclusive), or in rows < int(H * 0.4): S < 50 and V > 150;
 *   4. dilate 7 x 7, then open 7 x 7 (erode, dilate), pixels outside the image ignored;
 *   5. 4-connected components; none: nothing changes (F3R_SKY_EMPTY); none touches row 0: the mask stays as it is (F3R_SKY_NO_TOP);
 *      otherwise (F3R_SKY_TOP) sky = the components that touch row 0 and have more than thr pixels;
 *   6. not_sky = 1 where not sky, else 0 (int8).
 * `stages` selects what runs: F3R_SKY_CLASSIFY (steps 1-3 from the image; without it `src` is an (H, W) int8 bitmap, nonzero = set),
 *   F3R_SKY_MORPH (step 4), F3R_SKY_LABEL (steps 5-6).  bits_out (optional with F3R_SKY_LABEL, else required) receives the bitmap after
 *   the last of the first two stages that ran: total_words uint64, view i from its word_off, row y of a view = ceil(W / 64) words, pixel
 *   x = bit x % 64 of word x / 64, bits beyond W zero.
 * `table` is a DEVICE int64 array: n_views rows of 10 { src pointer (fp32 planes (3, H * W) as stored, or the int8 bitmap), not_sky
 *   pointer ((H, W) int8 out; 0 = none), roots pointer ((H, W) int32 out: the smallest pixel index y * W + x of the pixel's component, -1
 *   for background; 0 = none), H, W, word_off, pix_off, width_off (the running sums of H * ceil(W / 64), H * W and W), thr (floor(H * W *
 *   0.01) with the product formed in double), upper (int(H * 0.4)) }, then n_views + 1 tile starts of F3R_SKY_PIX_TILE words and n_views +
 *   1 tile starts of F3R_SKY_WORD_TILE words (running sums of ceil(H * ceil(W / 64) / tile)).  host_hw: HOST int64 [n_views][2] = the same
 *   H, W; the totals are checked against it before anything is launched.
 * stats (device int32 [n_views][5], written with F3R_SKY_LABEL) = { set pixels entering step 5, components, components touching row 0,
 *   components kept as sky, branch }.  Integer atomics only, and a component's label is its smallest pixel index: two runs give the
 *   same bits.  Inputs are not written to.
 * F3R_ERR_ARG before any launch: a null table, host_hw or workspace; n_views < 1; H or W < 1 or H * W >= 2^31; totals that do not match
 *   host_hw; an unknown stage bit; stats null with F3R_SKY_LABEL; bits_out null without it; a workspace that is too small.
 */
#define F3R_SKY_CLASSIFY 1
#define F3R_SKY_MORPH 2
#define F3R_SKY_LABEL 4
#define F3R_SKY_EMPTY 0
#define F3R_SKY_NO_TOP 1
#define F3R_SKY_TOP 2
#define F3R_SKY_PIX_TILE 16
#define F3R_SKY_WORD_TILE 256
size_t f3r_sky_workspace_bytes(int64_t total_words, int64_t total_pixels, int64_t total_width, int stages);
int f3r_sky_detect(const int64_t* table, const int64_t* host_hw, int n_views, int64_t n_pix_tiles, int64_t n_word_tiles, int64_t total_words,
                   int64_t total_pixels, int64_t total_width, int stages, void* workspace, size_t workspace_bytes, int32_t* stats,
                   uint64_t* bits_out, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh export (ABI 410): the as_mesh=True branch of the reference's notebooks/demo_multiview.ipynb plot_3d_points_with_colors --
 * np.percentile(conf, p), conf > thr, fast3r/dust3r/viz.py pts3d_to_trimesh (:43-90) and cat_meshes (:93-104) -- for every view of a scene
 * in one pass.  Python: fast3r_amd/mesh.py.  Quads of a view are numbered q = y (W - 1) + x, y < H - 1, x < W - 1; with i = y W + x,
 * triangle A = (i, i + 1, i + W) and B = (i + 1, i + W, i + W + 1); a triangle is kept iff its three vertices are valid.
 * `table` is a DEVICE int64 array: n_views rows of 12 { conf pointer ((H W) fp32; 0 = validity is the mask alone), pts pointer ((H W, 3)
 *   fp32), img pointer (fp32 planes (3, H W) as stored, or with img_u8 != 0 the (H W, 3) colour bytes), mask pointer ((H W) bytes, nonzero =
 *   valid; 0 = none), H, W, vbase (the sum of H W over the views before), img_u8, k_lo, k_hi (the two 0-based ranks np.percentile reads),
 *   gamma (the bits of its fp32 weight), 0 }, then n_views + 1 vertex-tile starts (running sum of ceil(H W / F3R_MESH_TILE)) and n_views +
 *   1 quad-tile starts (running sum of max(1, ceil((H - 1)(W - 1) / F3R_MESH_TILE))).  host_hw: HOST int64 [n_views][2] = the same H, W;
 *   f3r_mesh_count and f3r_mesh_write check the three totals against it before anything is launched.
 * f3r_mesh_threshold: thresholds[v] = numpy's fp32 _lerp (a + (b - a) g, or b - (b - a)(1 - g) where g >= 0.5) of the order statistics
 *   k_lo, k_hi of view v's conf, found exactly by radix select, one workgroup per view; nan_counts[v] = its NaNs, and then thresholds[v]
 *   is the quiet NaN 0x7fc00000 (np.percentile returns a NaN; nothing passes conf > NaN).
 * f3r_mesh_count: valid = conf > thresholds[v] (skipped when thresholds or the view's conf is null) AND mask != 0, bit-packed into the
 *   workspace; kept A and B per quad tile and their exclusive scans; with drop_unreferenced the vertices that a kept triangle uses (from
 *   the validity of the up to six triangles at a vertex: no atomics) and their scan.  counts (device uint32 [n_views][3]) = { kept A, kept
 *   B, vertices (used ones with drop_unreferenced, else H W) }.  View v then has (double_sided ? 2 : 1)(A + B) faces.
 * f3r_mesh_write, with the same table, totals, drop_unreferenced and workspace as the count: vertices [sum of counts[.][2]][3] fp32 in view
 *   order then pixel order ((x, y, z) -> (x, z, -y) with flip_axes); faces [F][3] of index_dtype and face_colors [F][3] bytes, view v's
 *   from slot F_v = the faces of the views before: kept A in quad order as (i1, i2, i3); the same as (i3, i2, i1); kept B as (i2, i3,
 *   i4); the same as (i4, i3, i2) -- the two backward blocks only with double_sided.  Indices are vbase + pixel, or with
 *   drop_unreferenced the vertex's rank among the used ones.  A faces take the colour of the quad's top-left pixel, B faces of its
 *   bottom-right: the byte as given, or trunc((img + 1.0f) * 127.5f) as two rounded fp32 operations, saturated to [0, 255] (NaN -> 0).
 *   vertices may be null when there are none to write, faces when the count found none.
 * f3r_mesh_ply_pack: n_vertices records of 12 bytes (xyz little-endian fp32), then n_faces of 16 { 3, three little-endian int32, r, g,
 *   b }, into out (4-byte aligned, 12 n_vertices + 16 n_faces bytes).
 * Limits, F3R_ERR_ARG before any launch: fewer than 2^31 vertices in all (indices, and the file's, are 32-bit; vbase and every face slot
 *   are 64-bit).  The scan's counters are uint32: they hold kept A and kept B triangles separately, each at most the quad count, which
 *   is below the vertex count, so they cannot wrap; up to 4 (2^31 - 1) faces are addressed.  Also F3R_ERR_ARG: null table, host_hw,
 *   workspace or counts; n_views < 1; negative counts; H or W < 1; totals that do not match host_hw; an unknown index_dtype; a workspace
 *   that is too small.  Inputs are not written to; two runs give the same bits.
 */
#define F3R_MESH_TILE 1024
#define F3R_INDEX_I32 0
#define F3R_INDEX_I64 1
size_t f3r_mesh_workspace_bytes(int64_t n_vertex_tiles, int64_t n_quad_tiles, int64_t total_vertices, int drop_unreferenced);
int f3r_mesh_threshold(const int64_t* table, int n_views, float* thresholds, uint32_t* nan_counts, f3r_stream_t stream);
int f3r_mesh_count(const int64_t* table, const int64_t* host_hw, int n_views, int64_t n_vertex_tiles, int64_t n_quad_tiles,
                   int64_t total_vertices, const float* thresholds, int drop_unreferenced, void* workspace, size_t workspace_bytes,
                   uint32_t* counts, f3r_stream_t stream);
int f3r_mesh_write(const int64_t* table, const int64_t* host_hw, int n_views, int64_t n_vertex_tiles, int64_t n_quad_tiles,
                   int64_t total_vertices, int double_sided, int drop_unreferenced, int flip_axes, int index_dtype, const void* workspace,
                   size_t workspace_bytes, float* vertices, void* faces, uint8_t* face_colors, f3r_stream_t stream);
int f3r_mesh_ply_pack(const float* vertices, int64_t n_vertices, const void* faces, const uint8_t* face_colors, int64_t n_faces,
                      int index_dtype, void* out, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Point-cloud export (ABI 420): export_combined_ply of the reference's notebooks/demo_multiview.ipynb -- per view np.percentile(conf, p),
 * conf > thr, the colour line, concatenation -- and its two Open3D downsamplers, VoxelDownSample and FarthestPointDownSample, restated
 * in a fixed arithmetic order.  Python: fast3r_amd/cloud.py.  Kernels: fast3r_amd/csrc/f3r_cloud.hip.
 * `table` of the two combine entries is a DEVICE int64 array: n_views rows of 12 words laid out as the mesh rows above { conf pointer (0 =
 *   no threshold test), pts pointer ((H W, 3) fp32), img pointer (fp32 planes (3, H W), or with img_u8 != 0 the (H W, 3) colour bytes), mask
 *   pointer ((H W) bytes, nonzero = keep; 0 = none), H, W, vbase, img_u8, k_lo, k_hi, gamma, 0 } -- the thresholds come from
 *   f3r_mesh_threshold on the same rows -- then n_views + 1 tile starts (running sum of ceil(H W / F3R_CLOUD_TILE)).
 * f3r_cloud_combine_count: keep = conf > thresholds[v] (skipped when thresholds or the view's conf is null) AND mask != 0; scan (device
 *   uint32 [n_tiles + 1]) = the exclusive scan of the kept pixels per tile; scan[n_tiles] = the total.
 * f3r_cloud_combine_write, with the same table, thresholds and scan: points [total][3] fp32 and colors [total][3] bytes in view order then
 *   pixel order; (x, y, z) -> (x, z, -y) with flip_axes; the colour is the byte as given, or trunc((img + 1.0f) * 127.5f) as two rounded
 *   fp32 operations, saturated to [0, 255] (NaN -> 0).
 * f3r_cloud_bounds: out (device uint32 [8]) = { the order-preserving keys (sign bit set -> all bits flipped, else sign bit set) of the
 *   minimum of x, y, z over the finite coordinates, of the maximum of x, y, z, the count of non-finite coordinates, 0 }; integer atomics.
 * f3r_cloud_voxel_sort: index_a = floor((p_a - vmin_a) / voxel_size) in fp64, vmin_a = min_bound[a] - 0.5 voxel_size (min_bound: HOST
 *   double [3]); key = (index_x << (bits[1] + bits[2])) | (index_y << bits[2]) | index_z (bits: HOST int [3], at most 63 in all); a stable
 *   LSD radix sort of (key, point index) with 8-bit digits in ceil(total bits / 8) passes; the segment heads (key differs from its
 *   predecessor's) and their scan.  *n_voxels (device uint32) = the number of distinct keys.  The workspace then holds what
 * f3r_cloud_voxel_sums reads (same n and workspace; n_voxels read back by the caller): one thread per voxel walks its run -- in original
 *   index order: the sort is stable -- and adds, sequentially in fp64, the widened coordinates and colour / 255.0 per channel;
 *   out_points[v] = (float)(sum / count), out_colors[v] = trunc(sum_c / count * 255.0), counts[v] = count; voxels in ascending key order.
 *   colors may be null (then out_colors is not written).  No floating-point atomics: the outputs equal a sequential restatement bit for bit.
 * f3r_cloud_fps: FarthestPointDownSample.  d[j] = inf; far = start_index; num_samples times: selected[i] = far; d[j] = min(d[j], (dx dx +
 *   dy dy) + dz dz) in fp64 on the widened coordinates, (dx, dy, dz) = p[j] - p[far]; far = the smallest index attaining max d if that
 *   maximum is > 0, else unchanged.  mode 0: one workgroup for n <= F3R_CLOUD_FPS_ONE_MAX, else tiled; 1: one workgroup (the whole loop in
 *   one kernel; F3R_ERR_ARG beyond F3R_CLOUD_FPS_ONE_MAX); 2: tiled -- one launch per iteration of min(ceil(n / F3R_CLOUD_FPS_TILE), 1024)
 *   workgroups with a grid-stride tile assignment; each reduces the previous launch's per-workgroup (distance, index) partials, updates its
 *   tiles' d and writes its own partial into the other half of a ping-pong pair.  The launch boundary is the only cross-workgroup
 *   synchronisation: no cooperative launch, no grid barrier, no spin-wait, no atomics.  The input must be finite (f3r_cloud_bounds counts).
 * f3r_cloud_mark: mask[0 .. n) = 0, then mask[selected[i]] = 1 (plain stores).  f3r_cloud_gather: out[i] = in[index[i]] for points and
 *   (unless null) colours; index is int32, or int64 with index_i64 != 0; every index in [0, n) (the caller's contract).
 * Limits, F3R_ERR_ARG before any launch: 1 <= n < 2^31 everywhere; null pointers; a workspace that is too small; bits outside [0, 31] or
 *   more than 63 in all; voxel_size not > 0; num_samples outside [1, n]; start_index outside [0, n); an unknown mode.  The
 *   *_workspace_bytes functions return 0 for refused arguments.  Inputs are not written to; two runs give the same bits.
 */
#define F3R_CLOUD_TILE 1024
#define F3R_CLOUD_SORT_TILE 2048
#define F3R_CLOUD_FPS_TILE 1024
#define F3R_CLOUD_FPS_ONE_MAX 8192
int f3r_cloud_combine_count(const int64_t* table, int n_views, int64_t n_tiles, const float* thresholds, uint32_t* scan, f3r_stream_t stream);
int f3r_cloud_combine_write(const int64_t* table, int n_views, int64_t n_tiles, const float* thresholds, const uint32_t* scan, int flip_axes,
                            float* points, uint8_t* colors, f3r_stream_t stream);
int f3r_cloud_bounds(const float* points, int64_t n, uint32_t* out, f3r_stream_t stream);
size_t f3r_cloud_voxel_workspace_bytes(int64_t n);
int f3r_cloud_voxel_sort(const float* points, int64_t n, const double* min_bound, double voxel_size, const int* bits, void* workspace,
                         size_t workspace_bytes, uint32_t* n_voxels, f3r_stream_t stream);
int f3r_cloud_voxel_sums(const float* points, const uint8_t* colors, int64_t n, int64_t n_voxels, const void* workspace,
                         size_t workspace_bytes, float* out_points, uint8_t* out_colors, int32_t* counts, f3r_stream_t stream);
size_t f3r_cloud_fps_workspace_bytes(int64_t n);
int f3r_cloud_fps(const float* points, int64_t n, int64_t num_samples, int64_t start_index, int mode, void* workspace,
                  size_t workspace_bytes, int32_t* selected, f3r_stream_t stream);
int f3r_cloud_mark(const int32_t* selected, int64_t num_samples, int64_t n, uint8_t* mask, f3r_stream_t stream);
int f3r_cloud_gather(const float* points, const uint8_t* colors, const void* index, int index_i64, int64_t n, int64_t m, float* out_points,
                     uint8_t* out_colors, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Point-splat renderer (ABI 430): the pictures of render_cumulative_pts3d_viz of the reference's notebooks/demo_multiview.ipynb -- there a
 * pyrender scene of GL points under a perspective camera with zfar = None, one scene and one GL context per frame; here a z-buffered splat
 * of a device cloud.  Python: fast3r_amd/render.py.  Kernels: fast3r_amd/csrc/f3r_render.hip.
 * `camera` is a HOST double [17]: V[3][4] row-major, the world-to-eye matrix (eye frame as OpenGL's: x right, y up, looking along -z);
 *   sx = 1 / (aspect tan(yfov / 2)), sy = 1 / tan(yfov / 2); cx, cy, the principal point's offset in normalised device coordinates (0 for a
 *   centred camera); znear.  The projection is infinite (no far plane).
 * The arithmetic of one point (x, y, z) (fp32, widened), in fp64, every operation rounded on its own, in this order:
 *   e_r = ((V[r][0] x + V[r][1] y) + V[r][2] z) + V[r][3] for r = x, y, z;  d = -e_z;
 *   p_x = sx e_x + cx d;  p_y = sy e_y + cy d;                              (clip-space x and y; clip-space w is d)
 *   the point is drawn iff d >= znear and |p_x| <= d and |p_y| <= d and (float)d is finite -- comparisons a NaN fails; a point whose centre
 *     is outside the frustum is dropped even where its square would reach into the viewport (GL's rule for points);
 *   x_w = (p_x / d + 1) (W / 2);  y_w = (p_y / d + 1) (H / 2);  h = point_size / 2;
 *   it covers the columns i with x_w - h <= i + 0.5 and i + 0.5 < x_w + h, and the window rows j likewise with y_w, both within the
 *     viewport: half-open, so an integer point_size covers that many pixels per axis.  Window row j is image row H - 1 - j.
 * f3r_render_clear: keys (device uint64 [H][W], image order: row 0 is the top) = all ones, the empty key.
 * f3r_render_splat: points [n0, n1) of the cloud (device fp32 [n][3]) are min-reduced into keys with 64-bit integer atomics:
 *   key = ((uint64_t)bits of (float)d << 32) | point index.  The smallest key wins: the nearest point, at equal depth the lowest index
 *   (GL_LESS for points drawn in index order).  Calls accumulate: after the ranges of views 0 .. i the keys are frame i of the cumulative
 *   pictures.  A relaxed load of the current key skips the atomic where the point already loses (the minimum is monotone: the result is
 *   the same).  n0 == n1 launches nothing.
 * f3r_render_resolve: image (device bytes [H][W][3]) = the colour (device bytes [n][3], unchanged: the point path has no lighting) of the
 *   point in the key's low word, or background (r | g << 8 | b << 16) where the key is all ones or names no point below n; depth
 *   (device fp32 [H][W], or null) = the key's high word as a float, +inf where the pixel is empty.
 * f3r_render_center: out (device double [3]) = the sum of the widened coordinates in a fixed order: min(ceil(n / 2048),
 *   F3R_RENDER_CENTER_PARTS) workgroups of 256 threads, thread t of workgroup b adds points b 256 + t, (b + G) 256 + t, .. sequentially from
 *   +0.0, then the xor butterfly over the wave and the waves in order; one workgroup adds the partials (device double
 *   [F3R_RENDER_CENTER_PARTS][3], scratch) the same way.  The caller divides by n.  The bounding box is f3r_cloud_bounds.
 * Limits, F3R_ERR_ARG before any launch: null pointers; W or H < 1, W H >= 2^31; n < 1 or n >= 2^32; n0 > n1 or n1 > n; point_size not
 *   finite or <= 0; znear <= 0; a camera entry that is not finite.  No floating-point atomics: two runs give the same bits; inputs are
 *   not written to.
 */
#define F3R_RENDER_CENTER_PARTS 1024
int f3r_render_clear(uint64_t* keys, int W, int H, f3r_stream_t stream);
int f3r_render_splat(const float* points, int64_t n, int64_t n0, int64_t n1, const double* camera, double point_size, int W, int H,
                     uint64_t* keys, f3r_stream_t stream);
int f3r_render_resolve(const uint64_t* keys, const uint8_t* colors, int64_t n, int W, int H, uint32_t background, uint8_t* image,
                       float* depth, f3r_stream_t stream);
int f3r_render_center(const float* points, int64_t n, double* partials, double* out, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Triangle rasteriser: depth-tested, flat-coloured triangles into the key buffer of the point-splat renderer above -- what shows a mesh
 * (build_mesh) and the camera pyramids of the reference's SceneViz (fast3r/dust3r/viz.py:133-305) without a GL stack.  It writes the keys
 * the splat writes, so points and triangles share one picture and f3r_render_resolve is unchanged.  Python: fast3r_amd/viz.py.  Kernels:
 * fast3r_amd/csrc/f3r_raster.hip.  f3r_version() is unchanged: a caller learns whether a library has these entry points by looking for them.
 * `camera`, `keys`, W, H: as f3r_render_splat takes them.  vertices: device fp32 [nv][3]; faces: device int32 or int64 [nf][3]
 * (index_dtype: F3R_INDEX_I32 / F3R_INDEX_I64).  Every operation below is fp64 and rounded on its own; only + - * /, comparisons and the
 * ceil of first_center_ge appear.
 * Per triangle f in [f0, f1), vertex indices (a, b, c) = faces[f]:
 *   1. skipped if any index is outside [0, nv); the indices are checked before any vertex is read.
 *   2. per vertex k, from (x, y, z) (fp32, widened): e_r = ((V[r][0] x + V[r][1] y) + V[r][2] z) + V[r][3];  d_k = -e_z;
 *      p_x = sx e_x + cx d;  p_y = sy e_y + cy d;  x_k = (p_x / d + 1) (W / 2);  y_k = (p_y / d + 1) (H / 2)      (as the splat).
 *   3. skipped unless d_k >= znear for all three and all six window coordinates are finite (no comparison passes on a NaN).  There is no
 *      near-plane clipping: a triangle with a vertex nearer than znear is dropped whole.  The frustum's sides do not drop a triangle.
 *   4. A = (x1 - x0) (y2 - y0) - (y1 - y0) (x2 - x0); skipped if A == 0 or A is not finite.
 *   5. the pixel box: columns [i0, i1) with i0 = first(min x_k, W), i1 = min(first(max x_k, W) + 1, W), where first(t, hi) is the
 *      smallest integer i with i + 0.5 >= t clamped to [0, hi] (the splat's first_center_ge); window rows [j0, j1) likewise with y and H.
 *      The box ends one past the first centre >= the maximum because edges are inclusive.  Its pixel count is (i1 - i0) (j1 - j0).
 *   6. r_k = 1 / d_k;  dmin = min(d_k);  dmax = max(d_k).
 * Per pixel (column i, window row j) of the box, centre (cx, cy) = (i + 0.5, j + 0.5):
 *   w0 = (x2 - x1) (cy - y1) - (y2 - y1) (cx - x1);  w1 = (x0 - x2) (cy - y2) - (y0 - y2) (cx - x2);
 *   w2 = (x1 - x0) (cy - y0) - (y1 - y0) (cx - x0);
 *   covered iff w0, w1, w2 >= 0 when A > 0, or w0, w1, w2 <= 0 when A < 0: edges are inclusive and there is no fill rule (two triangles
 *     that share an edge may both write the pixel; the key decides); no culling (both windings cover the same pixels);
 *   inv = (w0 r0 + w1 r1) + w2 r2;  dd = ((w0 + w1) + w2) / inv  (perspective-correct);  dd = dmin unless dd >= dmin;  dd = dmax if
 *     dd > dmax (so a triangle at constant depth writes exactly that depth);
 *   key = ((uint64_t)bits of (float)dd << 32) | (index_base + f), min-reduced into keys[H - 1 - j][i] with a 64-bit integer atomicMin
 *     behind the splat's relaxed early-out load.  With points at indices [0, n) and index_base = n, a point wins over a face at equal
 *     depth and a lower face over a higher one.
 * Work distribution: stage 1 runs one thread per triangle; a triangle whose box holds at most F3R_RASTER_SMALL_PIXELS pixels is drawn by
 *   its thread, a larger one is appended to a queue in the workspace (ballot compaction, one integer atomic per wave).  Stage 2 runs one
 *   wave per queued triangle, the lanes striding over the box with the same per-pixel code.  The queue's order depends on arrival, the
 *   keys do not.  [f0, f1) is walked in launches of at most faces_per_launch faces; the queue holds one uint32 slot per face of a launch.
 * workspace: f3r_raster_workspace_bytes(faces_per_launch) bytes (0 for an invalid faces_per_launch), 8-byte aligned.  After the call its
 *   first words read { uint32 queue length of the last launch, uint32 0, uint64 queue length over all launches }.
 * Limits, F3R_ERR_ARG before any launch: null pointers; W or H < 1, W H >= 2^31; nv < 1; an unknown index_dtype; not 0 <= f0 <= f1 <= nf;
 *   index_base < 0 or index_base + nf >= 2^32; a camera entry that is not finite; znear <= 0; faces_per_launch < 1 or >= 2^31; a workspace
 *   that is too small or misaligned.  f0 == f1 launches nothing.  No floating-point atomics: two runs give the same bits; inputs are
 *   not written to.
 */
#define F3R_RASTER_SMALL_PIXELS 64
size_t f3r_raster_workspace_bytes(int64_t faces_per_launch);
int f3r_raster_triangles(const float* vertices, int64_t nv, const void* faces, int index_dtype, int64_t nf, int64_t f0, int64_t f1,
                         int64_t index_base, const double* camera, int W, int H, uint64_t* keys, void* workspace, size_t workspace_bytes,
                         int64_t faces_per_launch, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Map pictures: scalar fields and images as RGBA8 pictures -- what plot_confidence_maps, maybe_plot_local_depth_and_conf and
 * plot_rgb_images of the reference's notebooks/demo_multiview.ipynb save through matplotlib.pylab.imsave(path, map, cmap='turbo' | 'Greys')
 * and imsave(path, uint8 image), byte for byte (matplotlib 3.10: Normalize, then Colormap.__call__(bytes=True)).  Python:
 * fast3r_amd/maps.py.  Kernels: fast3r_amd/csrc/f3r_maps.hip.  f3r_version() is unchanged: a caller learns whether a library has this
 * entry point by looking for it.
 * One call covers n_maps maps, which may differ in size.  table: device int64, n_maps rows of 6 words
 *   { source pointer (fp32), element stride in floats, H, W, destination pointer (bytes), destination row pitch in bytes },
 *   then the n_maps + 1 running tile counts of the maps, ceil(H W / F3R_MAPS_TILE) tiles each; host_rows: the same rows in HOST memory
 *   (the argument checks read them; the kernels read the device copy).  Pixel (y, x) of a map is source[(y W + x) stride] -- stride 3 and
 *   a pointer to element 2 read the z channel of an [H][W][3] pointmap in place -- and lands in the four bytes at destination + y pitch +
 *   4 x as R, G, B, A, so a map can be written into its cell of a larger picture.  Bytes outside the H x W cells are not written.
 * mode F3R_MAPS_LUT, per map, every operation rounded on its own, as numpy 2 runs matplotlib's lines on an fp32 array (vmin and vmax are
 * Python floats there, so `resdat -= vmin` and `resdat /= (vmax - vmin)` compute in fp64 and round into the fp32 array):
 *   1. vmin, vmax = the fp32 minimum and maximum with numpy's semantics: a NaN anywhere makes both NaN; +-inf take part as values (of
 *      -0.0 and +0.0 the minimum is -0.0 and the maximum +0.0, where numpy's choice depends on their order; no byte depends on it).
 *      They are reduced as order-preserving integer keys with integer atomics: two runs give the same bits.  keys: device uint32
 *      [n_maps][2], scratch.  ranges: device fp32 [n_maps][2] = { vmin, vmax }, written for the caller.
 *   2. x = 0 if vmin == vmax, otherwise t = a - vmin in fp32 (equal to the fp64 difference rounded to fp32: 53 >= 2 * 24 + 2 bits), then
 *      x = (float)((double)t / ((double)vmax - (double)vmin)): a correctly rounded fp64 division by the fp64 range -- which is finite
 *      where the fp32 range overflows, and is not rounded to fp32 -- rounded once more to fp32.  An all-fp32 division gives another
 *      byte at about one pixel in 10^4 (tests/map_cases.py "fp64_divisor" holds one);
 *   3. xa = x * 256; xa == 256 becomes 255;
 *   4. a NaN xa gives the bytes (0, 0, 0, 0); otherwise i = trunc(xa) clamped to [0, 255] and the bytes are (lut[i][0], lut[i][1],
 *      lut[i][2], 255).  lut: device bytes [256][3].
 * mode F3R_MAPS_RGB: the source is three planes ([3][H][W]; plane c begins H W stride elements after plane c - 1), each channel
 *   trunc((x + 1) * 127.5) -- an add and a multiply, each rounded -- clipped to [0, 255] (NaN reads as 0), alpha 255.  lut, keys and ranges
 *   are not used and may be null.
 * Launches only (one for RGB, three for LUT): nothing is allocated, copied or waited for.  Inputs are not written to.
 * Limits, F3R_ERR_ARG before any launch: a null table or host_rows; n_maps < 1; an unknown mode; in mode F3R_MAPS_LUT a null lut, keys or
 *   ranges; per map a null source or destination, H or W < 1 or H W > 2^30, a stride outside [1, 2^31), a pitch smaller than 4 W, a
 *   source, destination or pitch that is not a multiple of 4 bytes; n_tiles that is not the maps' tile count.
 */
#define F3R_MAPS_TILE 1024
typedef enum { F3R_MAPS_LUT = 0, F3R_MAPS_RGB = 1 } f3r_maps_mode;
int f3r_maps_colorize(const int64_t* table, const int64_t* host_rows, int n_maps, int64_t n_tiles, int mode, const uint8_t* lut,
                      uint32_t* keys, float* ranges, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Ground-truth views: posed RGB-D frames as the views the reference's datasets hand to the metrics and the loss -- what
 * BaseStereoViewDataset.__getitem__ (fast3r/dust3r/datasets/base/base_stereo_view_dataset.py:78-142) makes of a frame through
 * _crop_resize_if_necessary (:165-221), ImgNorm, depthmap_to_absolute_camera_coordinates (dust3r/utils/geometry.py:186-243) and
 * transpose_to_landscape (:243-261).  Python: fast3r_amd/gt_views.py, whose plan_view does the reference's host arithmetic (crop boxes,
 * sizes, intrinsics).  Kernels: fast3r_amd/csrc/f3r_views.hip.  f3r_version() is unchanged: a caller learns whether a library has these
 * entry points by looking for them.
 * One call covers a launch group: n_views views that share every number below and differ in their source pointers and cameras.
 * Geometry: crop box 1 (win_x, win_y, win_w, win_h) in the frame, around the rounded principal point; the window resized to res_w x
 * res_h; crop box 2 (crop_x, crop_y, out_w, out_h) in the resized picture: the out_h x out_w picture (v, u) of the view.  With
 * transpose = 1 (a portrait view) every output is written transposed: output pixel (oy, ox) is picture pixel (v, u) = (ox, oy), and the
 * output is out_w rows of out_h pixels.
 * f3r_gtview_resample: PIL.Image.crop(box 1).resize((res_w, res_h), LANCZOS | BICUBIC).crop(box 2) and ImgNorm, bit for bit.
 *   src_table: device int64 [n_views][2] = { pointer to the frame's [H][W][3] bytes, row pitch in bytes }; the frame must contain box 1.
 *   bounds_h int32 [res_w][2] = { first source column inside the window, count } and kk_h int32 [res_w][ksize_h]: Pillow's 22-bit
 *   fixed-point filter tables (precompute_coeffs / normalize_coeffs_8bpc) for in_size = win_w, so taps are clipped at the window's edges
 *   as Pillow clips them at the cropped picture's; bounds_v, kk_v, ksize_v the same for rows (in_size = win_h).  The horizontal pass
 *   writes an 8-bit intermediate (accumulator 1 << 21, shift >> 22, saturation) of the window rows [row0, row0 + rows) -- the caller
 *   passes the rows the kept output rows read -- and the columns crop box 2 keeps, into workspace (f3r_gtview_workspace_bytes(n_views,
 *   rows, out_w) bytes, 16-byte aligned); the vertical pass writes img_u8 [n_views][out_h][out_w][3] and img fp32 [n_views][3][out_h][out_w] =
 *   ((u / 255) - 0.5) / 0.5, three rounded operations in torchvision's order (dimensions swapped when transposed).
 * f3r_gtview_unproject: depth and points of the same picture.  src_table: device int64 [n_views][2] = { pointer to the frame's fp32
 *   depth, row pitch in floats }.  nx int32 [res_w], ny int32 [res_h]: cv2.resize(..., INTER_NEAREST)'s source index per resized column
 *   and row, inside the window (both null: no resize, res = win).  cams: device fp32 [n_views][F3R_GTVIEW_CAM_WORDS] = the 3 x 3
 *   intrinsics of the picture as the view returns them (rows [1, 0, 2] of K when transposed), then the 4 x 4 cam-to-world pose.  Per pixel:
 *   z = depth[win_y + ny[crop_y + v]][win_x + nx[crop_x + u]]; x = (u - cu) z / fu, y = (v - cv) z / fv in fp64, every operation rounded,
 *   rounded once to fp32 (numpy promotes the reference's expression to float64); with F3R_GTVIEW_POSE the point is R (x, y, z) + t in
 *   fp32, ((r0 x + r1 y) + r2 z) + t, each operation rounded; valid = z > 0, and with F3R_GTVIEW_FINITE_MASK also every coordinate
 *   finite.  Outputs, each optional but one: depthmap fp32 [n_views][out_h][out_w], pts3d fp32 [...][3], valid_mask bytes 0 / 1
 *   (dimensions swapped when transposed).  flag (optional): one device int32 the caller zeroed; set to 1 with a plain store when a
 *   gathered depth is not finite.
 * Launches only (two, and one): nothing is allocated, copied or waited for.  Inputs are not written to.  Table entries that point
 * outside the window are clamped to it, so a wrong table gives wrong pixels, never a fault.
 * Limits, F3R_ERR_ARG before any launch: a null pointer where one is needed; n_views outside [1, 2^20]; a box with a negative origin, an
 * empty size or an end beyond 2^24; crop box 2 outside the resized picture; rows outside the window; transpose not 0 or 1; unknown flags;
 * one of nx, ny without the other, or neither with res != win; a workspace that is too small or not 16-byte aligned.
 */
#define F3R_GTVIEW_CAM_WORDS 25
typedef enum { F3R_GTVIEW_POSE = 1, F3R_GTVIEW_FINITE_MASK = 2 } f3r_gtview_flags;
size_t f3r_gtview_workspace_bytes(int n_views, int rows, int out_w);
int f3r_gtview_resample(const int64_t* src_table, int n_views, int win_x, int win_y, int win_w, int win_h, const int32_t* bounds_h,
                        const int32_t* kk_h, int ksize_h, int res_w, const int32_t* bounds_v, const int32_t* kk_v, int ksize_v, int res_h,
                        int row0, int rows, int crop_x, int crop_y, int out_w, int out_h, int transpose, uint8_t* img_u8, float* img,
                        void* workspace, size_t workspace_bytes, f3r_stream_t stream);
int f3r_gtview_unproject(const int64_t* src_table, const float* cams, int n_views, int win_x, int win_y, int win_w, int win_h,
                         const int32_t* nx, const int32_t* ny, int res_w, int res_h, int crop_x, int crop_y, int out_w, int out_h,
                         int transpose, int flags, float* depthmap, float* pts3d, uint8_t* valid_mask, int32_t* flag, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Multi-view depth metrics: what the reference's scripts/robustmvd_eval.py obtains, per sample on the host, from an external benchmark
 * library with alignment="median" -- absolute relative error, inlier ratios, sparsification curves and their area -- for every (view,
 * sample) segment of a forward pass in one call, on the device.  That library is installed nowhere this project runs, so the definitions
 * are this project's own (docs/rows_f.md states them in full; docs/parity.md says so).  Python: fast3r_amd/depth_metric.py.  Kernels:
 * fast3r_amd/csrc/f3r_depth.hip.  f3r_version() is unchanged: a caller learns whether a library has these entry points by looking for them.
 * table: device int64, n_seg rows of F3R_DEPTH_ROW_WORDS words = { ground-truth depth fp32 [n], prediction fp32, its stride in floats (1: a
 *   depth map; 3: a pointmap read in place), its channel (0 with stride 1; 0 .. 2 with stride 3), confidence fp32 [n] or 0, mask bytes [n]
 *   (nonzero = valid) or 0, n = H W, the sum of the n before }, then the n_seg + 1 running tile counts, ceil(n / F3R_DEPTH_TILE) each.
 *   host_table: the same words on the host; every entry point checks them before it launches.  n_tiles: the last running count.
 * A pixel is valid when g > 0, g and p are finite, its mask byte (if any) is nonzero and, with use_thr, conf >= thr (a NaN confidence
 * fails), thr = torch.quantile(conf of the whole segment, q) by the rule of f3r_align_local_to_global.  All arithmetic is fp64 on the
 * exactly widened fp32 values, every operation rounded.
 * out: device fp64 [n_seg][out_ld], out_ld >= F3R_DEPTH_OUT_WORDS: { 0 n_valid, 1 thr (NaN without use_thr or confidence), 2 median of g,
 *   3 median of p (numpy's: the mean of the two middle order statistics, which are found exactly), 4 scale, 5 absrel, 6 rmse, 7 .. 10 inlier
 *   percentages, 11 .. 14 inlier counts, 15 ause }, then with curves n_bins words s_k and n_bins words o_k.
 * f3r_depth_medians writes columns 0 .. 4: scale = 1 (F3R_DEPTH_ALIGN_NONE) or median g / median p, 1 where that is not finite; a
 *   negative scale is kept.  With n_valid = 0 the medians and the scale are NaN.  One workgroup per segment.
 * f3r_depth_errors reads columns 0 .. 4 and writes 5 .. 15: sp = scale p, clipped to [clip_lo, clip_hi] with clip; e = |sp - g| / g;
 *   absrel = 100 sum e / n; rmse = sqrt(sum (sp - g)^2 / n); inlier t = 100 count(max(g / sp, sp / g) < t) / n, strictly; NaN with n = 0
 *   and for thresholds not given; ause = NaN until f3r_depth_sparsify.  workspace: f3r_depth_workspace_bytes(.., 0, 0) bytes at least.
 * f3r_depth_sparsify reads columns 0 .. 4 and writes ause and the curves: the valid pixels by ascending confidence key (ties in pixel
 *   order; without a confidence: pixel order) and by descending e rounded to fp32 (ties in pixel order); for k < n_bins, with n k / n_bins
 *   pixels (integer division) removed from the front, s_k and o_k are the means of e over the rest, each from the sums of the bins kept,
 *   never from total - prefix; ause = sum_{k < K - 1} (d_k + d_{k+1}) / (2 K), d_k = (s_k - o_k) / s_0; 0 with s_0 = 0, NaN with n = 0.
 *   order_conf, order_err: device uint32 [total pixels], the two orders as pixel indices inside their segments, segment after segment,
 *   segment s at [starts[s], starts[s + 1]); starts: device uint32 [n_seg + 1].  workspace: f3r_depth_workspace_bytes(.., 1, n_bins).
 * Launches and device-to-device copies only.  Sums are fixed-order partials added in slot order, without floating-point atomics: two runs
 * give the same bits.  Inputs are not written to.
 * Limits, F3R_ERR_ARG before any launch: a null table, host_table, out, workspace or order; n_seg outside [1, 2^24]; a row with a null
 *   depth or prediction, a stride other than 1 or 3, a pointer that is not a multiple of 4 bytes, n < 1 or n >= 2^31, a base or tile
 *   starts that do not follow from the sizes; more than F3R_DEPTH_MAX_THRESHOLDS thresholds; clip bounds that are no interval; n_bins
 *   outside [1, 65536]; 2^31 pixels or more in all (sparsify); out_ld or workspace too small.  f3r_depth_workspace_bytes returns 0 for them.
 */
#define F3R_DEPTH_TILE 1024
#define F3R_DEPTH_ROW_WORDS 8
#define F3R_DEPTH_OUT_WORDS 16
#define F3R_DEPTH_MAX_THRESHOLDS 4
typedef enum { F3R_DEPTH_ALIGN_NONE = 0, F3R_DEPTH_ALIGN_MEDIAN = 1 } f3r_depth_alignment;
size_t f3r_depth_workspace_bytes(int n_seg, int64_t n_tiles, int64_t total_pixels, int eval_uncertainty, int n_bins);
int f3r_depth_medians(const int64_t* table, const int64_t* host_table, int n_seg, int64_t n_tiles, int alignment, int use_thr, float q,
                      double* out, int64_t out_ld, f3r_stream_t stream);
int f3r_depth_errors(const int64_t* table, const int64_t* host_table, int n_seg, int64_t n_tiles, int use_thr, int clip, double clip_lo,
                     double clip_hi, const double* thresholds, int n_thresholds, void* workspace, size_t workspace_bytes, double* out,
                     int64_t out_ld, f3r_stream_t stream);
int f3r_depth_sparsify(const int64_t* table, const int64_t* host_table, int n_seg, int64_t n_tiles, int use_thr, int clip, double clip_lo,
                       double clip_hi, int n_bins, void* workspace, size_t workspace_bytes, uint32_t* order_conf, uint32_t* order_err,
                       uint32_t* starts, double* out, int64_t out_ld, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * View matching: the reference's find_reciprocal_matches (fast3r/dust3r/utils/geometry.py:381-397: two cKDTrees, mutual nearest
 * neighbours) over the view pairs of make_pairs (fast3r/dust3r/image_pairs.py:17-47), for all views and pairs of a scene at once.
 * Python: fast3r_amd/matching.py.  Kernels: fast3r_amd/csrc/f3r_match.hip, on the search of f3r_nn_query (f3r_nn.h).  f3r_version() is
 * unchanged: a caller learns whether a library has these entry points by looking for them.
 * Candidates: pts fp32 [total][3], the candidates of view 0, 1, .. one after another; seg: device int64 [n_views + 1], view v at
 *   [seg[v], seg[v + 1]).  Every table has a host copy (*_host) with the same words: the entry points check the host copies before they
 *   launch, and the kernels guard every index they take from the device copies.
 * f3r_match_index builds, in one call without a host round trip, one exact nearest-neighbour index per view in `index`
 *   (f3r_match_index_bytes): a grid over the view's own bounding box, its cell from the view's extent and occupied-cell count (the rule of
 *   f3r_nn_build, at most 4 m + 63 cells for m candidates), all points sorted once per round by (view, cell).  A view with a NaN or inf
 *   coordinate is counted in the index's flag word; f3r_match_search then searches nothing and f3r_match_count reports the word.
 * f3r_match_search: one launch over all directed pairs.  directed: int32 [n_directed][2] = (a, b); qoff: int64 [n_directed + 1], the running
 *   sum of the candidates of a.  For candidate q of a (local index) nn_idx[qoff[d] + q] = its nearest candidate of b (local to b; exact by
 *   the fp64 distance ((dx^2 + dy^2) + dz^2) of the fp32 coordinates, ties to the smaller index; 0 for an empty b) and nn_dist = the fp64
 *   distance (inf for an empty b).
 * f3r_match_count / f3r_match_write: pairs: int32 [n_pairs][4] = (i, j, the directed row of i -> j, the directed row of j -> i); tile_off:
 *   int64 [n_pairs + 1], the running sum of ceil(candidates of j / F3R_MATCH_TILE).  Candidate q of j matches iff nn_ij[nn_ji[q]] == q.
 *   _count writes tile_counts (uint32 [tiles + 1], scanned) and offsets: int64 [n_pairs + 2] = matches before each pair, the total, then the
 *   flag word: the one read-back of a call.  _write fills xy_i, xy_j (int32 [n_matches][2] = (x, y) from pix, the candidate's row-major
 *   pixel index, and widths[view]) and dist (fp64 [n_matches]) in pair order, inside a pair in ascending candidate order of j.
 * Launches only; integer atomics for boxes and occupied cells only: two runs give the same bits.  Inputs are not written to.
 * Limits, F3R_ERR_ARG before any launch: null or misaligned buffers (index and workspace: 256 bytes); n_views outside [1, 65536]; a
 *   segment table that does not ascend from 0, 2^31 candidates in a view or 2^32 in all; pairs outside the views or the directed rows;
 *   offsets that do not follow from the segments; 2^31 directed queries or 2^21 tiles or more in one call; index or workspace too small.  The *_bytes functions return 0 for them.
 */
#define F3R_MATCH_TILE 2048
size_t f3r_match_index_bytes(const int64_t* seg_host, int n_views);
size_t f3r_match_workspace_bytes(int64_t total, int n_views);
int f3r_match_index(const float* pts, const int64_t* seg, const int64_t* seg_host, int n_views, void* index, size_t index_bytes,
                    void* workspace, size_t workspace_bytes, f3r_stream_t stream);
int f3r_match_search(const void* index, const int64_t* seg_host, int n_views, const int32_t* directed, const int32_t* directed_host,
                     const int64_t* qoff, const int64_t* qoff_host, int n_directed, int32_t* nn_idx, double* nn_dist, f3r_stream_t stream);
int f3r_match_count(const void* index, const int64_t* seg, const int64_t* seg_host, int n_views, const int32_t* pairs,
                    const int32_t* pairs_host, const int64_t* tile_off, const int64_t* tile_off_host, int n_pairs, const int64_t* qoff,
                    const int64_t* qoff_host, int n_directed, const int32_t* nn_idx, uint32_t* tile_counts, int64_t* offsets,
                    f3r_stream_t stream);
int f3r_match_write(const int64_t* seg, const int64_t* seg_host, int n_views, const int32_t* pairs, const int32_t* pairs_host,
                    const int64_t* tile_off, const int64_t* tile_off_host, int n_pairs, const int64_t* qoff, const int64_t* qoff_host,
                    int n_directed, const int32_t* nn_idx, const double* nn_dist, const uint32_t* tile_counts, const int32_t* pix,
                    const int32_t* widths, int32_t* xy_i, int32_t* xy_j, double* dist, int64_t n_matches, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Cross-view occlusion filter: the reference's BasePCOptimizer.clean_pointcloud (fast3r/dust3r/cloud_opt/base_opt.py:279-317).  Every point
 * of view i is projected into the camera of each neighbour j; one that lies in front of camera j's depth map and is less confident than
 * the pixel it lands on has its confidence clipped to max_bad_conf.  Python: fast3r_amd/clean.py.  Kernels: fast3r_amd/csrc/f3r_clean.hip.
 * The library version is unchanged: a caller learns whether a library has these entry points by looking for them.
 * Views lie one after another: pts fp32 [total][3], conf, depth, out_conf fp32 [total]; poses fp32 [n_views][4][4] camera-to-world (the
 *   affine part is used); intrinsics fp32 [n_views][4] = fx, fy, cx, cy.  table: int64 [n_views][3] = H, W, first element of the view, then
 *   int64 [n_views + 1] = the starts of the neighbour lists in nbr (int32 [n_nbr], ascending inside a list, never the view itself).  table
 *   and nbr have host copies with the same words: they are checked before anything is launched, and the kernel guards what it takes from
 *   the device copies.
 * One small launch copies conf to out_conf, zeroes n_lowered and writes the view table into the workspace: the fp64 cofactor inverse of the
 *   pose's 3 x 3 block and -A^-1 t, rounded to fp32; a determinant that is 0 or not finite sets bit 0 of *flag (then nothing is tested:
 *   the caller reads the word and raises).  Then one launch per view i with a neighbour, in ascending order: one thread per pixel,
 *     frame F3R_CLEAN_CAMERA only: p = ((r00 x + r01 y) + r02 z) + t0, .. with the pose of view i, in fp32
 *     X = ((m00 x + m01 y) + m02 z) + m03, Y, Z likewise;  u = (fx X + cx Z) / Z;  v = (fy Y + cy Z) / Z;  ur = rint(u), vr = rint(v)
 *     in cone: Z > 0, 0 <= ur < W_j, 0 <= vr < H_j, on the rounded floats (NaN fails)
 *     bad: in cone and Z < (float)(1 - tol) * depth_j[vr][ur] and conf_i[p] < out_conf_j[vr][ur]
 *   every operation rounded on its own.  A pixel with a bad neighbour gets out_conf = fminf(conf, max_bad_conf); n_lowered[i] counts those
 *   whose value changed.  View i reads the working copy: cleaned already for j < i, the input for j > i, as the reference's loop does.
 * Inputs are not written to.  F3R_ERR_ARG before any launch: null or misaligned buffers (workspace: 256 bytes); n_views < 1; a view
 *   with a side outside [1, 2^24] or more than 2^31 - 1 pixels; offsets that are not the running sum of the shapes; neighbour lists that do not
 *   start at 0, end at n_nbr and ascend, or name a view outside the views or the view itself; tol outside [0, 1) or NaN; NaN max_bad_conf; an
 *   unknown frame; a workspace that is too small.  The sizing function returns 0 for n_views < 1.
 */
typedef enum { F3R_CLEAN_WORLD = 0, F3R_CLEAN_CAMERA = 1 } f3r_clean_frame;
size_t f3r_clean_workspace_bytes(int n_views);
int f3r_clean_confidence(const float* pts, const float* conf, const float* depth, const float* poses, const float* intrinsics,
                         const int64_t* table, const int64_t* table_host, int n_views, const int32_t* nbr, const int32_t* nbr_host,
                         int64_t n_nbr, double tol, float max_bad_conf, int frame, float* out_conf, uint32_t* n_lowered, uint32_t* flag,
                         void* workspace, size_t workspace_bytes, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Global alignment: the loss of the reference's PointCloudOptimizer.forward (fast3r/dust3r/cloud_opt/optimizer.py:219-266, l1_dist /
 * l2_dist of commons.py) and every gradient it has, at the level of matrices, in one evaluation.  Python: fast3r_amd/global_align.py.
 * Kernels: fast3r_amd/csrc/f3r_galign.hip.  The library version is unchanged: a caller learns whether a library has these entry points by
 * looking for them.  All inputs fp32 on the device:
 *   poses [n_views][3][4] = [R | t] camera-to-world; focals [n_views]; pp [n_views][2] = cx, cy; log_depth [total], the views one after
 *   another; pw_poses [n_edges][3][4] = [S | m], the top of the scaled pairwise pose; adaptors [n_edges][3].
 *   view_table: int64 [n_views][3] = H, W, first element of the view in log_depth, then the n_views + 1 starts of the observation lists.
 *   edges: int32 [n_edges][2] = (i, j).  Observation o = 2 e + side belongs to view i_e (side 0) or j_e (side 1).
 *   obs_table: int64 [2 n_edges][4] = { pointmap fp32 [H][W][3], weight map fp32 [H][W], H, W }: pointers, so that edges may share a map.
 *   obs_list: int32 [2 n_edges], the observations by view, ascending inside a view (the CSR the starts index).
 *   *_host: the same words on the host, checked before the first launch.
 * With (x, y) = (column, row) of pixel p of view v, for every observation o of v:
 *   d = exp(l_v[p]);  q = (d (x - cx) / f, d (y - cy) / f, d);  X = R q + t;  A = S (a * P_o[p]) + m;  r = X - A
 *   cost = w_o[p] |r| (F3R_GALIGN_L1) or w_o[p] |r|^2 (F3R_GALIGN_L2);  loss = sum_o k_o sum_p cost,  k_o = 1 / sum_e H W of that side
 *   g = k_o w_o[p] r / |r| (exactly 0 where r = 0) or 2 k_o w_o[p] r; a weight of exactly 0 contributes exactly nothing
 * Outputs: loss (one double); d_log_depth fp32 [total]; d_poses fp32 [n_views][3][4]; d_focals [n_views]; d_pp [n_views][2]; d_pw_poses
 *   [n_edges][3][4]; d_adaptors [n_edges][3].  fp64 arithmetic on the widened inputs, fp64 sums in a fixed order, no atomics: two runs give
 *   the same bits.  Inputs are not written to.  Launches only.
 * F3R_ERR_ARG before any launch: null or misaligned buffers (workspace: 256 bytes); fewer than 2 views or more than 65535; no edge; a
 *   view with more than 2^31 - 1 pixels; offsets that are not the running sum of the shapes; an edge outside the views or with i == j; a null
 *   or misaligned map pointer; an observation whose shape is not its view's; lists that do not hold every observation once under its own
 *   view, ascending; an unknown dist; a workspace that is too small.  The workspace bound does not depend on the image sizes; the sizing
 *   function returns 0 for an unsupported shape.
 */
typedef enum { F3R_GALIGN_L1 = 0, F3R_GALIGN_L2 = 1 } f3r_galign_dist;
size_t f3r_galign_workspace_bytes(int n_views, int n_edges);
int f3r_galign_loss_grad(const float* poses, const float* focals, const float* pp, const float* log_depth, const float* pw_poses,
                         const float* adaptors, const int64_t* view_table, const int64_t* view_table_host, int n_views,
                         const int32_t* edges, const int32_t* edges_host, int n_edges, const int64_t* obs_table,
                         const int64_t* obs_table_host, const int32_t* obs_list, const int32_t* obs_list_host, int dist, double* loss,
                         float* d_log_depth, float* d_poses, float* d_focals, float* d_pp, float* d_pw_poses, float* d_adaptors,
                         void* workspace, size_t workspace_bytes, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * f3r_resample_u8 / f3r_imgnorm_u8: the device side of the input pipeline `load_images` (fast3r/dust3r/utils/image.py:76-159).
 * f3r_resample_u8 is ONE pass of PIL.Image.resize for 8-bit RGB (`_resize_pil_image`, :68-74; Pillow's Resample.c): axis 1 =
 * horizontal ([H][W][3] -> [H][out_size][3]), axis 0 = vertical ([H][W][3] -> [out_size][W][3]); bounds [out_size][2] = {first source
 * index, count}, kk [out_size][ksize] = 22-bit fixed-point weights, both computed by the host exactly as Pillow computes them
 * (fast3r_amd/image.py); accumulator 1 << 21, >> 22, saturate: bit-exact with PIL.  f3r_imgnorm_u8 crops (:131-139) and applies
 * `ImgNorm` (:32: ToTensor + Normalize(0.5, 0.5)): [H][W][3] uint8 -> [3][h][w] fp32 = ((u / 255) - 0.5) / 0.5.
 */
int f3r_resample_u8(const uint8_t* in, uint8_t* out, int H, int W, int axis, int out_size, const int32_t* bounds, const int32_t* kk,
                    int ksize, f3r_stream_t stream);
int f3r_imgnorm_u8(const uint8_t* in, float* out, int H, int W, int x0, int y0, int w, int h, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LlamaDecoder variant (fast3r/models/fast3r.py:810-968, fast3r/models/components/llama.py): RMSNorm is f3r_layernorm with rms = 1;
 * f3r_silu_mul: SwiGLU gate of FeedForward.forward (llama.py:284), out[r][j] = silu(ab[r][j]) * ab[r][hidden + j], lowp in / out
 * ([rows][2*hidden] -> [rows][hidden]; the two projections w1, w3 are one GEMM with stacked weights);
 * f3r_rows_add_f32: x[r][:] += vec for r < rows -- `x + view0_mask * view0_embed` before every layer (fast3r.py:957-958; the view-0
 * tokens are the first rows of the sequence).
 */
int f3r_silu_mul(const void* ab, void* out, int64_t rows, int hidden, int dtype, f3r_stream_t stream);
int f3r_rows_add_f32(float* x, const float* vec, int64_t rows, int D, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * precision "exact" -- what `inference(dtype="32")` means in the reference (fast3r/dust3r/inference_multiview.py:41-52: no autocast, fp32
 * everywhere).  Every GEMM / conv of that mode is f3r_gemm with split = F3R_SPLIT_X3 (both operands as hi + lo planes); the attention
 * core (blocks.py:158-169) runs in plain fp32 on q / k / v taken from an fp32 buffer -- a validation mode for scenes of tens of views.
 * f3r_rope2d_f32: RoPE-2D (pos_embed.py:162-183) in place on the q and k parts of qkv[rows][ld] (the first 2 * n_heads * 64 columns);
 *   tables as in f3r_gemm_args.rope_cos / rope_sin ([n_pos][16]), token t of a sequence sits at (t / rope_w, t % rope_w).
 * f3r_attn_f32: o[r][h*64 + d] = sum_j softmax_j(q[r] . k[j] * scale) v[j][d] over the keys of r's sequence (n_seq sequences of seq_len
 *   rows; q, k, v row stride ld floats, head_dim floats per head: 0 or 64, or another multiple of 16 up to 128).  Output as fp32 (o_f32) and / or as lowp hi [+ lo] planes ([rows][ldo]), the
 *   A operand of the X3 projection that follows.
 */
int f3r_rope2d_f32(float* qkv, int64_t rows, int64_t ld, int n_heads, int64_t seq_len, int rope_w, const float* rope_cos,
                   const float* rope_sin, f3r_stream_t stream);
int f3r_attn_f32(const float* q, const float* k, const float* v, int64_t ld, void* o_hi, void* o_lo, float* o_f32, int64_t ldo,
                 int64_t n_seq, int64_t seq_len, int n_heads, float scale, int dtype, int head_dim, f3r_stream_t stream);

/* The general forms (LlamaDecoder and view-sharded models in precision "exact"):
 * f3r_rope_f32: rotary embedding in place on the first n_rot_heads 64-wide column groups of qkv (q heads, then k heads); rope_mode as in
 *   f3r_gemm_args.rope_mode (0: RoPE-2D tables [n_pos][16]; 1: one [32]-angle row per group of rope_w rows, llama.py:96-122).
 * f3r_silu_mul_f32: SwiGLU gate (llama.py:284) on fp32 ab[rows][2*hidden] -> hi + lo planes [rows][hidden].
 * f3r_attn_f32_ex: fp32 attention with separate query / key counts (tq, tk per sequence), grouped-query heads (query head h reads K / V
 *   head h / kv_group: repeat_kv, llama.py:195-198) and an optional causal mask on absolute positions (key j visible to query i iff
 *   k_pos0 + j <= q_pos0 + i), so a rank of a view-sharded model can attend its queries over the gathered keys of all ranks. */
typedef struct f3r_attn_f32_args {
  const float* q;    /* [n_seq * tq][ldq], head h at columns [h * head_dim, (h + 1) * head_dim) */
  const float* k;    /* [n_seq * tk][ldkv], K / V head g at columns [g * head_dim, ...) */
  const float* v;
  int64_t ldq, ldkv;
  void* o_hi;        /* lowp planes [n_seq * tq][ldo] (o_lo optional), and / or */
  void* o_lo;
  float* o_f32;      /* fp32 [n_seq * tq][ldo] */
  int64_t ldo;
  int64_t n_seq, tq, tk;
  int64_t q_pos0, k_pos0; /* causal only */
  int32_t n_heads;   /* query heads */
  int32_t kv_group;  /* query heads per K / V head (0 / 1 = plain multi-head) */
  int32_t causal;
  int32_t dtype;     /* f3r_dtype of the lowp planes */
  int32_t head_dim;  /* 0 = 64, or a multiple of 16 up to 128 */
  float scale;
} f3r_attn_f32_args;
int f3r_rope_f32(float* qkv, int64_t rows, int64_t ld, int n_rot_heads, int64_t seq_len, int rope_w, int rope_mode, const float* rope_cos,
                 const float* rope_sin, f3r_stream_t stream);
int f3r_silu_mul_f32(const float* ab, void* out_hi, void* out_lo, int64_t rows, int hidden, int dtype, f3r_stream_t stream);
int f3r_attn_f32_ex(const f3r_attn_f32_args* args, f3r_stream_t stream);
/* The same attention on the matrix pipe (f3r_exact_mfma.hip; ABI 320): every operand as an exact sum of two 16-bit planes (~22 significand bits),
 * every product as three MFMAs with fp32 accumulation, softmax in fp32 -- the FMA-pipe kernel's numbers to ~1e-6 at 10x its speed, for the
 * scenes where that kernel takes minutes (it stays the reference implementation of the mode; tests compare the two).  head_dim 64, no causal
 * mask: f3r_attn_f32_mfma_workspace returns 0 for anything else, and the bytes of caller-owned scratch (the planes of q, k and V^T) otherwise. */
int64_t f3r_attn_f32_mfma_workspace(const f3r_attn_f32_args* args);
int f3r_attn_f32_mfma(const f3r_attn_f32_args* args, void* workspace, int64_t workspace_bytes, f3r_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * precision "robust" (ABI 340) -- between "high" (every operand one fp16 number, weights hi + lo) and "exact": every GEMM / conv as in "exact"
 * (F3R_SPLIT_X3), the attention core (blocks.py:158-190) with Q and K as hi + lo planes (f3r_attn_args.qk_planes = 2: three products per score
 * block) and P, V single fp16 -- the cheapest operand set that keeps a noise-amplifying checkpoint within 1e-3 of the fp32 path
 * (oracle/precision_study.py --study robust_vitl).  The two passes around that attention launch:
 * f3r_qkv_planes: qkv fp32 [n_seq * seq_len][ld] = q | k | v column blocks of n_heads * 64 | kv_heads * 64 | kv_heads * 64 (the output of the QKV
 *   projection; rotary embedding already applied) -> q_planes [rows][n_heads][hi 64 | lo 64] (values multiplied by q_scale = softmax scale x
 *   log2(e) BEFORE the split), k_planes [rows][kv_heads][hi 64 | lo 64], vt [n_seq][kv_heads * 64][ldvt] one plane (key columns >= seq_len zero).
 * f3r_attn_state_finish: the state an attention launch parked (f3r_attn_args.state_out: st_o fp32 [rows][n_heads * head_dim] un-normalised,
 *   st_ml fp32 [rows][n_heads][4] = {m, l of lane half 0, of lane half 1, -}) -> O / (l0 + l1) as hi + lo planes [rows][ldo] (the A operand of the
 *   X3 output projection; o_lo may be NULL) and / or fp32 (o_f32).
 */
int f3r_qkv_planes(const float* qkv, int64_t ld, int64_t n_seq, int64_t seq_len, int n_heads, int kv_heads, float q_scale, void* q_planes, void* k_planes,
                   void* vt, int64_t ldvt, int dtype, int planes /* 2 or 3: the row layout of f3r_attn_args.qk_planes */, f3r_stream_t stream);
int f3r_attn_state_finish(const float* st_o, const float* st_ml, int64_t rows, int n_heads, int head_dim, void* o_hi, void* o_lo, float* o_f32,
                          int64_t ldo, int dtype, f3r_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* F3R_H_ */
