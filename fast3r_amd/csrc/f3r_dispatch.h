// How f3r_gemm and f3r_attn_fwd pick their kernel (host only).  Both validate their arguments, decide the COMPLETE launch once -- a GemmPlan /
// AttnPlan -- and then launch exactly that: below the two plan functions nothing reads kernel_sel or an environment switch again, and the reporting
// functions (f3r_gemm_plan_name, f3r_attn_kernel_name) format the same plan.  docs/kernels.md, "How a call picks its kernel".
#pragma once
#include <atomic>
#include <map>
#include <mutex>

#include "f3r_common.h"

inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
inline bool al8(const void* p) { return (((uintptr_t)p) & 7) == 0; }

// CUs of the CURRENT device (256 when it cannot be asked), cached per device index: what the attention kernels' work counter serves ...
inline int f3r_device_cus() {
  static std::atomic<int> cache[64];  // zero-initialised; a racing first call computes the same value twice
  int dev = 0, cu = 0;
  if (hipGetDevice(&dev) != hipSuccess) dev = 0;
  std::atomic<int>* slot = (dev >= 0 && dev < 64) ? &cache[dev] : nullptr;
  if (slot && (cu = slot->load(std::memory_order_relaxed)) != 0) return cu;
  if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cu < 8) cu = 256;
  if (slot) slot->store(cu, std::memory_order_relaxed);
  return cu;
}
// ... and rounded down to a multiple of 8 (XCDs): the persistent grids of the GEMM kernels, whose tile maps give every XCD a contiguous run
inline int f3r_num_cus() { return f3r_device_cus() / 8 * 8; }

// A code object embedded in the library (obj/*_blob.cpp, written by build.sh) and its N kernels, loaded once per DEVICE (hipModule handles are per device
// context): with the per-thread error string the only process-wide state of the library.  One that does not load leaves every kernel null.
template <int N>
struct F3rCodeObject {
  const unsigned char* image;
  const char* names[N];
  struct Dev { bool tried = false; hipModule_t mod = nullptr; hipFunction_t fn[N] = {}; };
  std::map<int, Dev> devs;
  std::mutex mu;
  hipFunction_t get(int i) {   // kernel names[i] on the current device, or null
    int dev = 0;
    if (i < 0 || i >= N || hipGetDevice(&dev) != hipSuccess || dev < 0) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    Dev& d = devs[dev];
    if (!d.tried) {
      d.tried = true;
      if (hipModuleLoadData(&d.mod, image) == hipSuccess)
        for (int k = 0; k < N; ++k)
          if (hipModuleGetFunction(&d.fn[k], d.mod, names[k]) != hipSuccess) d.fn[k] = nullptr;
      (void)hipGetLastError();
    }
    return d.fn[i];
  }
};

// ------------------------------------------------------------------------------------------------ f3r_gemm
enum {                         // f3r_gemm_args.kernel_sel (2 - 5, 9 and the lab forms are for measurement; an ineligible launch is an error, never a fallback)
  GEMM_SEL_AUTO = 0,           // by shape: the hand-scheduled kernel where the launch fills its grid, else the 256-tile kernel where its score wins, else the 128-tile one
  GEMM_SEL_128 = 1,            // the 128 x 128-tile kernel
  GEMM_SEL_256_STAGGER = 2,    // the 256-tile kernel, 256 x 256 tiles where N fills them, staggered wave rows
  GEMM_SEL_256_LOCKSTEP = 3,   // ... without the stagger
  GEMM_SEL_256_NARROW = 4,     // ... its 256 x 128 tile form
  GEMM_SEL_256_ALL_TILES = 5,  // ... one tile per workgroup instead of the persistent grid; on the fused-tail X3F8 launch also the MERGED schedule
  GEMM_SEL_ASM = 6,            // the hand-scheduled kernels
  GEMM_SEL_AUTO_NO_ASM = 7,    // by shape among the compiler-scheduled kernels only
  GEMM_SEL_ASM_SKEW = 9,       // 6 with a start-up skew of the persistent workgroups (measured slower: f3r_gemm_asm.hip launch_tiles)
  GEMM_SEL_LAB = 16,           // 16 + LAB bits: the ablation variants of -DF3R_GEMM_LAB builds (tools/lab)
};
enum GemmFamily {
  GEMM_128,        // gemm_kernel, f3r_gemm.hip
  GEMM_256,        // gemm256_kernel, f3r_gemm256.hip / f3r_gemm256_bf16.hip
  GEMM_256_F8FIN,  // ... its F3R_SPLIT_X3F8 / fused-tail (fin_w) instances, f3r_gemm256_f8.hip: the only family for those launches
  GEMM_ASM,        // f3r_gemm_asm_{f32,lp}_* (csrc/asm/gemm_gen.py), one launch
  GEMM_ASM_F8,     // ... with the low plane in fp8 (F3R_SPLIT_W2F8): the only family for that layout
  GEMM_ASM_QKV,    // ... the QKV projection as a q | k launch and a V^T launch (W2F8: the first on the fp8 kernels)
  GEMM_LAB,        // gemm256_lab_kernel
};
// The launch f3r_gemm makes for an argument block: the family and every form parameter kernel_sel stands for.
struct GemmPlan {
  GemmFamily family = GEMM_128;
  bool stagger = true;     // 256-tile: wave row 1 runs one barrier behind row 0
  int halves = 2;          // 256-tile: W half tiles per K-tile, 2 = 256 x 256 outputs, 1 = 256 x 128 (as kernel_sel 2 - 5 ask, else by tile_score)
  bool all_tiles = false;  // 256-tile: a grid of all tiles instead of one persistent workgroup per CU
  bool merged = false;     // the fused-tail X3F8 launch: the MERGED schedule (32 MFMAs per barrier pair)
  bool skew = false;       // hand-scheduled: start the persistent workgroups up to 3/4 of a tile period apart
  int lab = 0;             // GEMM_LAB: the LAB bits
};
// F3R_OK and the plan, or why no kernel takes the (validated) launch; evaluates each eligibility predicate at most once
int f3r_gemm_plan(const f3r_gemm_args& a, GemmPlan* plan);
// the plan's family and form as text; "" where f3r_gemm refuses the block, by an argument rule or at selection
const char* f3r_gemm_plan_name(const f3r_gemm_args& a);

// f3r_gemm256.hip: the 256-tile kernel
bool f3r_gemm256_eligible(const f3r_gemm_args& a);            // can take the problem at all
int f3r_gemm256_max_conv_k_tiles();                           // records of its K-tile table in LDS (TileCfg::TAB_ENTRIES): the most K-tiles a 3x3 convolution may have
int f3r_gemm256_launch(const f3r_gemm_args& a, hipStream_t stream, const GemmPlan& plan);   // GEMM_256, GEMM_256_F8FIN, GEMM_LAB
// f3r_gemm_asm.hip: the hand-scheduled GEMM kernels
bool f3r_gemm_asm_eligible(const f3r_gemm_args& a, const char** why);       // *why: the first obstacle
bool f3r_gemm_asm_f8_eligible(const f3r_gemm_args& a, const char** why);    // F3R_SPLIT_W2F8
bool f3r_gemm_asm_qkv_eligible(const f3r_gemm_args& a, const char** why);   // the QKV projection as two launches
bool f3r_gemm_asm_preferred(int64_t tiles);   // does a launch of that many 256 x 256 tiles fill the persistent grid well enough?
int f3r_gemm_asm_launch(const f3r_gemm_args& a, hipStream_t stream, const GemmPlan& plan);   // GEMM_ASM, GEMM_ASM_F8, GEMM_ASM_QKV

// Which tile form fills the 256 CUs best (256-wide tiles only where N fills them; QKV needs the wide tile).  score = (fraction of the last round's slots that do work, over all rounds) x (relative
// main-loop efficiency of the form: 256x256 1.0, 256x128 0.82, 128x128 with two workgroups per CU 0.72 -- tools/kernel_bench.py
// --what gemmsmall / gemm, profiles/r02_kernel_microbench_gemm_small.jsonl).  E.g. 8 views (M = 8192, N = 1024): 128 tiles of 256^2 = half a
// round (0.50), 256 tiles of 256x128 = one full round (0.82), 512 tiles of 128^2 = one full round (0.72) -> 256x128.
inline float tile_score(int64_t tiles, int slots, float eff) {
  if (tiles <= 0) return 0.f;
  const int64_t rounds = (tiles + slots - 1) / slots;
  return eff * (float)tiles / (float)(rounds * slots);
}
inline float score_256(const f3r_gemm_args& a, int nh) {
  return tile_score(((a.M + 255) / 256) * ((a.N + 128 * nh - 1) / (128 * nh)), 256, nh == 2 ? 1.0f : 0.82f);
}
inline float score_128(const f3r_gemm_args& a) { return tile_score(((a.M + 127) / 128) * ((a.N + 127) / 128), 512, 0.72f); }

// GemmPlan::halves.  forced: the tile form kernel_sel asks for (1 / 2 half tiles), 0 = whichever scores better
inline int f3r_gemm256_halves(const f3r_gemm_args& a, int forced) {
  if (a.epi == F3R_EPI_QKV) return 2;
  if (a.N % 256 != 0 || forced == 1) return 1;
  if (forced == 2) return 2;
  return score_256(a, 1) > score_256(a, 2) ? 1 : 2;
}
// is the 256-tile kernel (one workgroup per CU; in the tile form its score picks) also FASTER than the 128-tile kernel (two per CU, 4x the tiles)?
inline bool f3r_gemm256_preferred(const f3r_gemm_args& a) { return score_256(a, f3r_gemm256_halves(a, 0)) >= score_128(a); }

// ------------------------------------------------------------------------------------------------ f3r_attn_fwd
enum {                // f3r_attn_args.kernel_sel
  ATTN_SEL_AUTO = 0,  // the hand-scheduled kernels where the launch is eligible (head_dim 64: from F3R_ATTN_ASM_MIN_KEYS keys on), else the HIP kernels
  ATTN_SEL_HIP = 1,   // attn_kernel (head_dim 64) / attn_generic_kernel
  ATTN_SEL_ASM = 2,   // the hand-scheduled kernels (csrc/asm/attn_gen.py); an ineligible launch is an error
};
enum AttnFamily {
  ATTN_HIP_CAUSAL,   // attn_kernel<causal>, f3r_attn.hip
  ATTN_HIP_BATCHED,  // attn_kernel<batched>
  ATTN_HIP,          // attn_kernel
  ATTN_GENERIC,      // attn_generic_kernel, f3r_attn_generic.hip: head_dim != 64
  ATTN_ASM,          // f3r_attn_asm_*, f3r_attn_asm.hip
};
enum AttnItem {     // queries of a work item (a workgroup of four waves) of a hand-scheduled launch
  ATTN_ITEM_512,    // four 32-query blocks per wave: the head_dim-64 kernel
  ATTN_ITEM_256,    // two: head_dim 80 / 128, the three-product kernels, and the q256 form of the head_dim-64 kernel
};
inline int attn_item_wave_rows(AttnItem item) { return item == ATTN_ITEM_512 ? 128 : 64; }
struct AttnAsmLaunch {   // that many query rows (0: no such launch) on that work item
  int64_t rows = 0;
  AttnItem item = ATTN_ITEM_512;
  bool grouped = false;   // ATTN_ITEM_512 at head_dim 64, one product: f3r_attn_asm_*_grp, one barrier per group of key tiles (F3R_ATTN_GROUPED_MIN_KEYS, f3r_attn_asm.hip)
};
// The launch(es) f3r_attn_fwd makes for an argument block.
struct AttnPlan {
  AttnFamily family = ATTN_HIP;
  int hd_index = 0;          // ATTN_ASM: which generated head_dim (f3r_attn_asm.hip kHd),
  int planes = 1;            // 1 or f3r_attn_args.qk_planes 2 / 3 (the three-product kernels),
  AttnAsmLaunch main, tail;  // query rows [0, main.rows) and [main.rows, tq): the last, partly filled round of a head_dim-64 launch on 256-query items
};
// F3R_OK and the plan, or F3R_ERR_UNSUPPORTED: no kernel takes the (validated) launch the way kernel_sel / qk_planes ask
int f3r_attn_plan(const f3r_attn_args& a, AttnPlan* plan);
// f3r_attn_asm.hip: can the hand-scheduled kernels take the launch (*why: the first obstacle)?  If so, the plan is filled.
bool f3r_attn_asm_plan(const f3r_attn_args& a, int64_t min_keys, AttnPlan* plan, const char** why);
int f3r_attn_asm_launch(const f3r_attn_args& a, const AttnPlan& plan, hipStream_t stream);
const char* f3r_attn_asm_name(const f3r_attn_args& a, const AttnPlan& plan);
int f3r_attn_generic_launch(const f3r_attn_args& a, hipStream_t stream);   // f3r_attn_generic.hip: head_dim != 64
