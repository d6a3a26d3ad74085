// 4-connected component labelling on a bit-packed bitmap: the union-find helpers of f3r_sky.hip.  Header-only; with F3R_HOST_BUILD
// defined the same source compiles as plain C++ (tests/csrc/ccl_host.cpp drives it on the CPU, with the steps of many concurrent unions
// interleaved in seeded orders, before anything runs on a GPU; the product never builds it that way).
//
// The bitmap.  Row y of a W-pixel image is WW = ceil(W / 64) words; pixel (y, x) is bit x % 64 of word y * WW + x / 64; bits at x >= W are 0.
// A pixel's index is p = y * W + x (int32: H * W < 2^31).  parent[p] is defined for set pixels only.
//
// The invariant every loop below rests on: parent[p] <= p, parent[p] is a set pixel of p's component, and a stored parent only ever
// DECREASES (it is written once by the initialisation, then only by an atomic minimum or by the flattening, which stores a root that
// is <= every index on p's chain).  So following parents strictly descends until it meets a root (parent[r] == r), a stale read is
// still an ancestor, and the root of a finished component is its smallest pixel index: the canonical label, whatever order the atomics ran in.
#pragma once
#include <stdint.h>

#ifdef F3R_HOST_BUILD
#define F3R_CCL_FN inline
namespace f3r_ccl {
inline int32_t load(const int32_t* p) { return *p; }
inline void store(int32_t* p, int32_t v) { *p = v; }
inline int32_t fetch_min(int32_t* p, int32_t v) {  // the host driver is single-threaded: it interleaves whole steps
  const int32_t old = *p;
  if (v < old) *p = v;
  return old;
}
inline int clz64(uint64_t x) { return __builtin_clzll(x); }
inline int ctz64(uint64_t x) { return __builtin_ctzll(x); }
}  // namespace f3r_ccl
#else
#include <hip/hip_runtime.h>
#define F3R_CCL_FN __device__ __forceinline__
namespace f3r_ccl {
F3R_CCL_FN int32_t load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
F3R_CCL_FN void store(int32_t* p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
F3R_CCL_FN int32_t fetch_min(int32_t* p, int32_t v) { return atomicMin(p, v); }
F3R_CCL_FN int clz64(uint64_t x) { return __builtin_clzll(x); }
F3R_CCL_FN int ctz64(uint64_t x) { return __builtin_ctzll(x); }
}  // namespace f3r_ccl
#endif

namespace f3r_ccl {

// ---- initialisation: a set pixel points at the first pixel of its horizontal run within its word, or -- when that run starts at bit 0
// and the previous word of the row ends set -- at that word's last pixel (which points at ITS run start: a chain of at most WW links).
// w: the pixel's word; b: its bit; prev_last: bit 63 of the previous word of the row (false at xw == 0); p: the pixel's index.
F3R_CCL_FN int32_t initial_parent(uint64_t w, int b, bool prev_last, int32_t p) {
  const uint64_t zeros_below = ~w & ((1ull << b) - 1ull);
  const int start = zeros_below ? 64 - clz64(zeros_below) : 0;
  if (start == 0 && prev_last) return p - b - 1;
  return p - (b - start);
}

// ---- the vertical links that need a union: w, up = a word and the one above it; every maximal run of w & up is connected along both
// rows, so one union at its first bit joins it; prev_link = bit 63 of (w & up) of the previous word pair (the run continues from there).
F3R_CCL_FN uint64_t link_starts(uint64_t w, uint64_t up, bool prev_link) {
  const uint64_t m = w & up;
  return m & ~((m << 1) | (prev_link ? 1ull : 0ull));
}

// length of the run of set bits of w that starts at bit b (bit b is set), within the word
F3R_CCL_FN int run_length(uint64_t w, int b) {
  const uint64_t rest = ~(w >> b);  // bits shifted in from above are 0 in w >> b, so 1 here: rest != 0 unless b == 0 and w is all ones
  return rest ? ctz64(rest) : 64;
}

// ---- find.  Terminates: parent[x] < x whenever x is not a root (the invariant), so x strictly decreases and is bounded below by 0.
F3R_CCL_FN int32_t find_root(const int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = load(parent + x);
    if (p == x) return x;
    x = p;  // p < x
  }
}

// ---- union of the components of a and b, as a machine that makes ONE memory access per step, so that a test can interleave the steps of
// many unions.  phase 0 walks a to a root, phase 1 walks b to a root, phase 2 links the larger root below the smaller with an atomic minimum.
struct UnionOp {
  int32_t a, b;
  int32_t phase;
};

// One step; true when the union is done.  Terminates: a step of phase 0 / 1 either lowers a / b strictly (parent[x] < x) or moves on to
// the next phase; a step of phase 2 either ends the union (the roots are equal, or the minimum was applied to what was still a root) or
// restarts from old < a, the value another union had already linked a under.  3 (a + b) + (2 - phase) falls with every step and is >= 0.
F3R_CCL_FN bool union_step(int32_t* parent, UnionOp& u) {
  if (u.phase == 0) {
    const int32_t p = load(parent + u.a);
    if (p == u.a) u.phase = 1; else u.a = p;
    return false;
  }
  if (u.phase == 1) {
    const int32_t p = load(parent + u.b);
    if (p == u.b) u.phase = 2; else u.b = p;
    return false;
  }
  if (u.a == u.b) return true;
  if (u.a < u.b) {
    const int32_t t = u.a;
    u.a = u.b;
    u.b = t;
  }
  const int32_t old = fetch_min(parent + u.a, u.b);  // b < a: the stored parent can only fall
  if (old == u.a) return true;                       // a was still a root: it now hangs under b
  u.a = old;                                         // old < a: a had been linked meanwhile; go on from there (b may no longer be a root: phase 0, then 1)
  u.phase = 0;
  return false;
}

F3R_CCL_FN void unite(int32_t* parent, int32_t a, int32_t b) {
  UnionOp u = {a, b, 0};
  while (!union_step(parent, u)) {  // bounded: see union_step
  }
}

}  // namespace f3r_ccl
