// Host side of the hand-scheduled attention kernel: the code object assembled from csrc/asm/attn_gen.py is embedded in the library
// (obj/f3r_attn_asm_blob.cpp, written by build.sh), loaded once per device with hipModuleLoadData and launched with
// hipModuleLaunchKernel on the caller's stream (capturable in a hipGraph like any other launch).  f3r_attn_fwd (f3r_attn.hip)
// decides per call whether a launch goes here (f3r_attn_args.kernel_sel, include/f3r.h).
#include <cstddef>
#include <cstdlib>
#include <cstring>

#include "f3r_common.h"
#include "f3r_dispatch.h"

extern "C" const unsigned char f3r_attn_asm_hsaco[];
extern "C" const unsigned int f3r_attn_asm_hsaco_len;

namespace {

// kernel argument block: the ARG_* offsets of csrc/asm/attn_gen.py
struct f3r_attn_asm_seg {
  const void* k;
  const void* vt;
  uint32_t tiles, pad;
};
struct f3r_attn_asm_args {
  const void* q;
  void* o;
  uint32_t ldq_b, ldk_b, ldvt_b, ldo_b;  // row strides in bytes
  uint32_t n_tiles, n_seg;               // 64-key tiles over all segments, number of (non-empty) segments
  uint64_t q_bs, o_bs;                   // batch strides in bytes
  uint32_t kv_shift, flags;              // bit 0: state_in, bit 1: state_out
  float* st_o;
  float* st_ml;
  uint64_t k_bs, vt_bs;
  uint32_t st_o_ld_b, st_ml_ld_b;
  uint32_t tq, pad;                      // query rows (the last workgroup may be partial: ARG_TQ)
  f3r_attn_asm_seg seg[8];
  uint32_t* dbg;                         // ARG_DBG: optional counters (f3r_attn_args.dbg_counters)
  uint32_t* sched;                       // ARG_SCHED: {next, done} of the work-stealing form, or NULL = one work item per workgroup id
  uint32_t n_work, nx, nxy, nx_magic, nxy_magic, grid;   // items, q blocks, q blocks x heads, ceil(2^32 / nx), ceil(2^32 / nxy), workgroups launched
};
static_assert(sizeof(f3r_attn_asm_args) == 344 && offsetof(f3r_attn_asm_args, seg) == 112 && offsetof(f3r_attn_asm_args, dbg) == 304 &&
              offsetof(f3r_attn_asm_args, sched) == 312 && offsetof(f3r_attn_asm_args, n_work) == 320,
              "must match ARG_SIZE / ARG_SEG / ARG_DBG / ARG_SCHED of attn_gen.py");

// The generated kernels: head_dim 64 (512 queries per workgroup), 80 and 128 (256 queries per workgroup); HEAD_DIMS of attn_gen.py
constexpr int kNumHd = 3, kHd[kNumHd] = {64, 80, 128};
int hd_index(int hd) {
  for (int i = 0; i < kNumHd; ++i)
    if (kHd[i] == hd) return i;
  return -1;
}
// The work item of a generated kernel (AttnGen.QPW of csrc/asm/attn_gen.py: 32-query blocks per wave): four at head_dim 64, two everywhere else --
// and in the q256 form of head_dim 64, AttnGen(head_dim=64, qpw=2), which a plan asks for with ATTN_ITEM_256.  A wave whose rows
// (attn_item_wave_rows) would run past the last query works on the LAST rows of that many instead (attn_gen.py: s_sub_u32 tq, QW / s_min_u32): with
// fewer query rows than a wave's the subtraction wraps and the wave reads and writes past tq.
AttnItem native_item(int hd, int planes) { return (hd == 64 && planes < 2) ? ATTN_ITEM_512 : ATTN_ITEM_256; }

// [head_dim index][F3R_F16, F3R_BF16]; head_dim 64, fp16 with Q and K as hi + lo planes (f3r_attn_args.qk_planes = 2) and with the correction products
// on the fp8 MFMA (3); head_dim 64 with 256-query work items (two query blocks per wave): small launches (q256_wins); head_dim 64 on 512-query items
// with one barrier per group of key tiles on an 8-slot LDS ring (AttnGen(tiles_per_barrier=...)): long key sequences (F3R_ATTN_GROUPED_MIN_KEYS)
F3rCodeObject<12> g_kernels = {f3r_attn_asm_hsaco,
                               {"f3r_attn_asm_f16", "f3r_attn_asm_bf16", "f3r_attn_asm_d80_f16", "f3r_attn_asm_d80_bf16", "f3r_attn_asm_d128_f16", "f3r_attn_asm_d128_bf16",
                                "f3r_attn_asm_qk3_f16", "f3r_attn_asm_qk3f8_f16", "f3r_attn_asm_q256_f16", "f3r_attn_asm_q256_bf16", "f3r_attn_asm_f16_grp",
                                "f3r_attn_asm_bf16_grp"}};

hipFunction_t get_fn(int dtype, int hi, int planes, AttnItem item, bool grouped = false) {
  if (dtype < 0 || dtype > 1 || hi < 0) return nullptr;
  const bool hd64 = kHd[hi] == 64;
  if (planes >= 2) return (hd64 && dtype == F3R_F16) ? g_kernels.get(4 + planes) : nullptr;
  if (item != native_item(kHd[hi], planes)) return hd64 ? g_kernels.get(8 + dtype) : nullptr;   // the 256-query form of the head_dim-64 kernel
  if (grouped) return hd64 ? g_kernels.get(10 + dtype) : nullptr;
  return g_kernels.get(2 * hi + dtype);
}

bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// Small launches at head_dim 64 on 256-query items (f3r_attn_asm_q256_*: twice the items, 0.64 of a 512-query item's time each inside the model):
// taken where the round count wins at that ratio, i.e. below HALF a round of 512-query items.  Measurements: docs/kernels.md, "How a call picks its kernel".
bool q256_wins(int64_t tq, int64_t hb, int64_t cus) {
  const int64_t n512 = (tq + 511) / 512 * hb, n256 = (tq + 255) / 256 * hb;
  const double t512 = (double)((n512 + cus - 1) / cus), t256 = 0.64 * (double)((n256 + cus - 1) / cus);
  return t256 < 0.97 * t512;
}

// The last, partly filled round of a head_dim-64 launch as a SECOND launch on 256-query items, when its r items are at most half a round: 2 r <= cus
// items of 0.64 round time instead of a whole round (docs/kernels.md).  The main launch keeps whole query blocks x all heads x all batches, so its item
// count is a multiple of cus exactly when its block count is a multiple of cus / gcd(cus, heads x batch).  -> the rows of the main launch, 0: one launch
int64_t tail_split_rows(int64_t tq, int64_t hb, int64_t cus) {
  const int64_t nqb = (tq + 511) / 512;
  if (nqb * hb <= cus) return 0;   // less than a round: q256_wins decides for the whole launch
  int64_t x = cus, y = hb;
  while (y) { const int64_t t = x % y; x = y; y = t; }
  const int64_t g = cus / x;       // query blocks per whole number of rounds
  const int64_t nqb_main = nqb / g * g;
  if (nqb_main == 0 || nqb_main == nqb) return 0;
  if (nqb_main * hb / cus > 8) return 0;     // long launches: work stealing inside ONE launch beats a chip-wide join between two
  const int64_t r = (nqb - nqb_main) * hb;   // items of the last round (< cus)
  if (2 * r > cus) return 0;                 // the tail would need two rounds of 256-query items: 1.28 > 1
  return nqb_main * 512;
}

// The launches of an eligible call: their rows and work items.  Every rule and measurement switch about the FORM of a hand-scheduled launch is
// here, evaluated once per call; f3r_attn_asm_launch executes what this leaves in the plan and f3r_attn_asm_name formats it.
void plan_items(const f3r_attn_args& a, AttnPlan& p) {
  const int hd = kHd[p.hd_index];
  p.main.rows = a.tq;
  p.main.item = native_item(hd, p.planes);
  if (p.main.item != ATTN_ITEM_512 || get_fn(a.dtype, p.hd_index, p.planes, ATTN_ITEM_256) == nullptr) return;
  // measurement only (tools/kernel_bench.py; the product never sets them): F3R_ATTN_Q256 = "0" never / "1" always the 256-query form, in one launch;
  // F3R_ATTN_TAIL_SPLIT = "0": no second launch
  static const char* force = getenv("F3R_ATTN_Q256");
  static const char* split = getenv("F3R_ATTN_TAIL_SPLIT");
  if (force && (force[0] == '0' || force[0] == '1')) {
    if (force[0] == '1') p.main.item = ATTN_ITEM_256;
    return;
  }
  const int64_t cus = f3r_device_cus(), hb = (int64_t)a.n_heads * a.batch;
  // two launches: not with a carried softmax state (the sharded path compares its two-launch form against one launch), not with CUs reserved
  const bool may_split = !(split && split[0] == '0') && !a.state_in && !a.state_out && a.reserve_cus <= 0;
  const int64_t rows = may_split ? tail_split_rows(a.tq, hb, cus) : 0;
  if (rows > 0) {
    // the tail is a launch of its own: it needs at least one wave's rows of the form that takes it.  A shorter one -- tq = 8192 + 40 at 16 heads --
    // stays in ONE launch of all the query blocks, whose partial last workgroup handles any number of rows
    const AttnItem item = q256_wins(a.tq - rows, hb, cus) ? ATTN_ITEM_256 : ATTN_ITEM_512;
    if (a.tq - rows >= attn_item_wave_rows(item)) {
      p.main.rows = rows;   // (whole rounds of 512-query items: q256_wins never holds for them)
      p.tail.rows = a.tq - rows;
      p.tail.item = item;
      return;
    }
  }
  if (q256_wins(a.tq, hb, cus)) p.main.item = ATTN_ITEM_256;
}

// From F3R_ATTN_GROUPED_MIN_KEYS keys on (include/f3r.h), a 512-query launch at head_dim 64 (one product) runs the grouped-barrier kernel: f3r_attn_asm_*_grp
// meets at one s_barrier per TWO 64-key tiles instead of one per tile, on an 8-slot LDS ring (128 KiB); per wave the same instructions on the same
// numbers, so the results are bit for bit those of f3r_attn_asm_*.  Measured on one box, arms interleaved (profiles/attn_grouped_barrier_ab.jsonl):
// -1.06 % per launch at 327 680 keys, -1.3 % at 102 400, -1.06 % at 40 960, -0.75 % at 20 480; at 8 192, the shortest launch measured, ahead in
// all twelve grouped samples (mean -1.2 %, where two product runs in a row differ by 0.8 - 1.7 %): that is the threshold, nothing shorter was measured.
// The 256-query launches (q256, the split tail) keep their kernel.  docs/kernels.md, "How a call picks its kernel".
void plan_launches(const f3r_attn_args& a, int64_t keys, AttnPlan& p) {
  plan_items(a, p);
  if (kHd[p.hd_index] != 64 || p.planes != 1 || keys < F3R_ATTN_GROUPED_MIN_KEYS) return;
  p.main.grouped = p.main.item == ATTN_ITEM_512;   // (a split tail is at most half a round of 512-query items: it always takes the 256-query form)
}

}  // namespace

// Can the hand-scheduled kernels take this launch?  *why names the first obstacle; an eligible launch leaves with its complete ATTN_ASM plan.
bool f3r_attn_asm_plan(const f3r_attn_args& a, int64_t min_keys, AttnPlan* plan, const char** why) {
  *why = "";
  const int hd = a.head_dim == 0 ? 64 : a.head_dim;
  const int hi = hd_index(hd);
  if (hi < 0) { *why = "no generated kernel for this head_dim (64, 80, 128)"; return false; }
  const int qkp = a.qk_planes >= 2 ? a.qk_planes : 1;
  if (qkp >= 2 && (hd != 64 || a.dtype != F3R_F16)) { *why = "qk_planes 2 / 3 need head_dim 64 and fp16"; return false; }
  const int64_t wrows = attn_item_wave_rows(native_item(hd, qkp));
  if (a.causal) { *why = "causal mask"; return false; }
  if (!a.q_prescaled) { *why = "q not pre-scaled"; return false; }
  if (a.tq < wrows) { *why = "fewer query rows than one wave takes (128 at head_dim 64, 64 otherwise)"; return false; }
  if (a.kv_group > 1 && !pow2(a.kv_group)) { *why = "kv_group not a power of two"; return false; }
  // (the three-product kernels index the parked state by sequence: rows [z tq, (z + 1) tq) -- they park it on every launch; the others at batch 1 only)
  if ((a.state_in || a.state_out) && a.batch != 1 && qkp < 2) { *why = "carried softmax state with batch > 1"; return false; }
  int first = -1;
  int64_t keys = 0;
  for (int s = 0; s < a.n_seg; ++s) {
    if (a.seg_len[s] == 0) continue;
    if (a.seg_len[s] % 64 != 0) { *why = "a K/V segment is not a multiple of 64 keys"; return false; }
    if (first < 0) first = s;
    if (a.ldvt[s] != a.ldvt[first] || a.k_batch_stride[s] != a.k_batch_stride[first] || a.vt_batch_stride[s] != a.vt_batch_stride[first]) {
      *why = "K/V segments with different ldvt / batch strides";
      return false;
    }
    keys += a.seg_len[s];
  }
  if (first < 0) { *why = "no keys"; return false; }
  if (keys < min_keys) { *why = "fewer keys than F3R_ATTN_ASM_MIN_KEYS"; return false; }
  if (keys / 64 >= (1ll << 31)) { *why = "too many keys"; return false; }
  // 32-bit lane offsets: a wave's query rows, 64 key rows, head_dim V^T rows must span < 4 GiB
  if (wrows * a.ldq * 2 >= (1ll << 32) || wrows * a.ldo * 2 >= (1ll << 32) || 64 * a.ldk * 2 >= (1ll << 32) || (int64_t)hd * a.ldvt[first] * 2 >= (1ll << 32) ||
      wrows * a.n_heads * hd * 4 >= (1ll << 32)) {
    *why = "row strides too large for 32-bit lane offsets";
    return false;
  }
  if (a.tq >= (1ll << 31) || a.n_heads >= 65536 || a.batch >= 65536) { *why = "grid too large"; return false; }
  // a code object that does not load on this device makes the launch INELIGIBLE (kernel_sel 0 then takes the general HIP kernel,
  // kernel_sel 2 reports why) instead of failing every fusion-attention call of the process
  if (get_fn(a.dtype, hi, qkp, native_item(hd, qkp)) == nullptr) { *why = "the embedded code object could not be loaded on this device"; return false; }
  plan->family = ATTN_ASM;
  plan->hd_index = hi;
  plan->planes = qkp;
  plan_launches(a, keys, *plan);
  return true;
}

const char* f3r_attn_asm_name(const f3r_attn_args& a, const AttnPlan& p) {
  const bool h = a.dtype == F3R_F16;
  if (p.planes == 2) return "f3r_attn_asm_qk3_f16 (hand-scheduled, three products per score block, csrc/asm/attn_gen.py)";
  if (p.planes == 3) return "f3r_attn_asm_qk3f8_f16 (hand-scheduled, three products per score block, the corrections on the fp8 MFMA, csrc/asm/attn_gen.py)";
  if (kHd[p.hd_index] == 80) return h ? "f3r_attn_asm_d80_f16 (hand-scheduled, csrc/asm/attn_gen.py)" : "f3r_attn_asm_d80_bf16 (hand-scheduled, csrc/asm/attn_gen.py)";
  if (kHd[p.hd_index] == 128) return h ? "f3r_attn_asm_d128_f16 (hand-scheduled, csrc/asm/attn_gen.py)" : "f3r_attn_asm_d128_bf16 (hand-scheduled, csrc/asm/attn_gen.py)";
  if (p.tail.rows > 0 && p.main.grouped)   // (a split tail is at most half a round: q256_wins holds for it, it is never a 512-query launch)
    return h ? "f3r_attn_asm_f16_grp + f3r_attn_asm_q256_f16 for the last round (hand-scheduled, one barrier per group of key tiles, csrc/asm/attn_gen.py)"
             : "f3r_attn_asm_bf16_grp + f3r_attn_asm_q256_bf16 for the last round (hand-scheduled, one barrier per group of key tiles, csrc/asm/attn_gen.py)";
  if (p.tail.rows > 0)
    return h ? "f3r_attn_asm_f16 + f3r_attn_asm_q256_f16 for the last round (hand-scheduled, csrc/asm/attn_gen.py)"
             : "f3r_attn_asm_bf16 + f3r_attn_asm_q256_bf16 for the last round (hand-scheduled, csrc/asm/attn_gen.py)";
  if (p.main.item == ATTN_ITEM_256)
    return h ? "f3r_attn_asm_q256_f16 (hand-scheduled, 256-query work items, csrc/asm/attn_gen.py)" : "f3r_attn_asm_q256_bf16 (hand-scheduled, 256-query work items, csrc/asm/attn_gen.py)";
  if (p.main.grouped)
    return h ? "f3r_attn_asm_f16_grp (hand-scheduled, one barrier per group of key tiles, csrc/asm/attn_gen.py)"
             : "f3r_attn_asm_bf16_grp (hand-scheduled, one barrier per group of key tiles, csrc/asm/attn_gen.py)";
  return h ? "f3r_attn_asm_f16 (hand-scheduled, csrc/asm/attn_gen.py)" : "f3r_attn_asm_bf16 (hand-scheduled, csrc/asm/attn_gen.py)";
}

// one launch of the plan: query rows [row0, row0 + l.rows) on the work item l.item
static int launch_one(const f3r_attn_args& a, const AttnPlan& p, int64_t row0, const AttnAsmLaunch& l, hipStream_t stream) {
  const int hd = kHd[p.hd_index];
  const int wave_rows = attn_item_wave_rows(l.item);
  // (f3r_attn_asm_plan checks the caller's tq against a wave's rows; this one guards every launch of the plan)
  F3R_REQUIRE(l.rows >= wave_rows, "f3r_attn_fwd: a hand-scheduled launch of %lld query rows, fewer than the %d of one wave", (long long)l.rows, wave_rows);
  hipFunction_t fn = get_fn(a.dtype, p.hd_index, p.planes, l.item, l.grouped);
  if (!fn) {
    f3r_set_error("f3r_attn_fwd: the embedded hand-scheduled kernel could not be loaded on this device");
    return F3R_ERR_LAUNCH;
  }
  f3r_attn_asm_args k;
  memset(&k, 0, sizeof(k));
  k.q = (const char*)a.q + row0 * a.ldq * 2;
  k.o = (char*)a.o + row0 * a.ldo * 2;
  k.ldq_b = (uint32_t)(a.ldq * 2);
  k.ldk_b = (uint32_t)(a.ldk * 2);
  k.ldo_b = (uint32_t)(a.ldo * 2);
  k.q_bs = (uint64_t)a.q_batch_stride * 2;
  k.o_bs = (uint64_t)a.o_batch_stride * 2;
  int sh = 0;
  for (int gsz = a.kv_group > 1 ? a.kv_group : 1; gsz > 1; gsz >>= 1) ++sh;
  k.kv_shift = (uint32_t)sh;
  k.flags = (a.state_in ? 1u : 0u) | (a.state_out ? 2u : 0u);
  k.st_o = a.st_o;
  k.st_ml = a.st_ml;
  k.st_o_ld_b = (uint32_t)a.n_heads * (uint32_t)hd * 4u;
  k.st_ml_ld_b = (uint32_t)a.n_heads * 16u;
  k.tq = (uint32_t)l.rows;
  k.dbg = a.dbg_counters;
  for (int s = 0; s < a.n_seg; ++s) {
    if (a.seg_len[s] == 0) continue;
    f3r_attn_asm_seg& g = k.seg[k.n_seg++];
    g.k = a.k_seg[s];
    g.vt = a.vt_seg[s];
    g.tiles = (uint32_t)(a.seg_len[s] / 64);
    k.n_tiles += g.tiles;
    k.ldvt_b = (uint32_t)(a.ldvt[s] * 2);
    k.k_bs = (uint64_t)a.k_batch_stride[s] * 2;
    k.vt_bs = (uint64_t)a.vt_batch_stride[s] * 2;
  }
  // Work stealing (f3r_attn_args.sched_counter): one persistent workgroup per CU takes (q block, head, batch) items from a shared counter, so
  // the XCDs -- which the hardware feeds round-robin by workgroup id whatever their clocks -- finish together.  Worth it from two rounds of
  // workgroups on; the kernel's magic-number division needs item x period < 2^32.
  const int64_t wg_rows = 4 * wave_rows;
  const unsigned nx = (unsigned)((l.rows + wg_rows - 1) / wg_rows);
  unsigned gx = nx, gy = (unsigned)a.n_heads, gz = (unsigned)a.batch;
  const uint64_t n_work = (uint64_t)nx * gy * gz, nxy = (uint64_t)nx * gy;
  unsigned cus = (unsigned)f3r_device_cus();
  // f3r_attn_args.reserve_cus: leave that many CUs to whatever else must become resident while this launch runs (a rank's local-shard launch
  // next to the exchange of the other ranks' K / V^T); the persistent form is then taken whenever there are more items than workgroups
  const unsigned reserve = a.reserve_cus > 0 ? (unsigned)a.reserve_cus : 0u;
  const bool reserving = a.sched_counter && reserve > 0 && reserve < cus && n_work > (uint64_t)(cus - reserve);
  if (reserving) cus -= reserve;
  if (a.sched_counter && (reserving || n_work >= 2ull * cus) && n_work * nxy < (1ull << 32)) {
    k.sched = a.sched_counter;
    k.n_work = (uint32_t)n_work;
    k.nx = nx;
    k.nxy = (uint32_t)nxy;
    k.nx_magic = nx > 1 ? (uint32_t)(((1ull << 32) + nx - 1) / nx) : 0;
    k.nxy_magic = nxy > 1 ? (uint32_t)(((1ull << 32) + nxy - 1) / nxy) : 0;
    k.grid = cus;
    gx = cus;
    gy = gz = 1;
    // the kernel trusts {next, done} to be zero on entry and leaves them zero; a launch that was aborted (or a buffer the caller did not clear)
    // would make the next one silently skip items [0, next): clear the two words on the launch stream (a memset node under graph capture)
    hipError_t me = hipMemsetAsync(a.sched_counter, 0, 2 * sizeof(uint32_t), stream);
    if (me != hipSuccess) {
      f3r_set_error("f3r_attn_fwd: clearing sched_counter failed: %s", hipGetErrorString(me));
      return F3R_ERR_LAUNCH;
    }
  }
  size_t size = sizeof(k);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &k, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
  hipError_t e = hipModuleLaunchKernel(fn, gx, gy, gz, 256, 1, 1, 0, stream, nullptr, config);
  if (e != hipSuccess) {
    f3r_set_error("f3r_attn_fwd: hipModuleLaunchKernel failed: %s", hipGetErrorString(e));
    return F3R_ERR_LAUNCH;
  }
  return f3r_check_launch("f3r_attn_fwd(asm)");
}

int f3r_attn_asm_launch(const f3r_attn_args& a, const AttnPlan& p, hipStream_t stream) {
  const int rc = launch_one(a, p, 0, p.main, stream);
  return (rc != F3R_OK || p.tail.rows == 0) ? rc : launch_one(a, p, p.main.rows, p.tail, stream);
}
