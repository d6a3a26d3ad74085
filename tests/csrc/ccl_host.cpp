// TEST INFRASTRUCTURE: the product's union-find helpers (fast3r_amd/csrc/f3r_ccl.h) compiled for the host, so that tests/test_sky.py can
// run the labelling of f3r_sky.hip on the CPU -- the same initialisation, the same list of unions, the same find -- with the steps of
// the unions interleaved the way concurrent threads would interleave them, in a seeded order.  Nothing in the product links this file.
#define F3R_HOST_BUILD 1
#include "../../fast3r_amd/csrc/f3r_ccl.h"

#include <cstddef>
#include <utility>
#include <vector>

namespace {
uint64_t next_rand(uint64_t& s) {  // splitmix64
  s += 0x9e3779b97f4a7c15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
}  // namespace

// bits: H * ceil(W / 64) words; roots: H * W out (-1 background).  `in_flight` unions are live at a time (the "threads"); every round one
// of them, picked by the seeded generator, makes one step (= one memory access).  Returns the total number of steps, or -1 if they exceed
// the bound that f3r_ccl.h's termination argument gives (the sum of 3 (a + b) + 3 over the unions): a hang would show up as that, not as
// a hung test.
extern "C" long long ccl_host_label(const uint64_t* bits, int H, int W, int in_flight, uint64_t seed, int32_t* roots) {
  using namespace f3r_ccl;
  const int WW = (W + 63) / 64;
  std::vector<int32_t> parent((size_t)H * W, -1);
  for (int y = 0; y < H; ++y)
    for (int xw = 0; xw < WW; ++xw) {
      const uint64_t w = bits[(size_t)y * WW + xw];
      const bool prev_last = xw > 0 && (bits[(size_t)y * WW + xw - 1] >> 63);
      for (int b = 0; b < 64 && xw * 64 + b < W; ++b)
        if ((w >> b) & 1ull) {
          const int32_t p = y * W + xw * 64 + b;
          parent[p] = initial_parent(w, b, prev_last, p);
        }
    }
  std::vector<UnionOp> todo;
  for (int y = 1; y < H; ++y)
    for (int xw = 0; xw < WW; ++xw) {
      const uint64_t w = bits[(size_t)y * WW + xw], up = bits[(size_t)(y - 1) * WW + xw];
      const bool prev_link = xw > 0 && ((bits[(size_t)y * WW + xw - 1] & bits[(size_t)(y - 1) * WW + xw - 1]) >> 63);
      uint64_t starts = link_starts(w, up, prev_link);
      while (starts) {
        const int b = ctz64(starts);
        starts &= starts - 1ull;
        const int32_t p = y * W + xw * 64 + b;
        todo.push_back({p, p - W, 0});
      }
    }
  // shuffle the order in which the unions are issued, too
  for (size_t i = todo.size(); i > 1; --i) std::swap(todo[i - 1], todo[next_rand(seed) % i]);
  std::vector<UnionOp> live;
  size_t next = 0;
  long long steps = 0;
  long long budget = 0;
  for (const UnionOp& u : todo) budget += 3ll * (u.a + u.b) + 3;
  while (next < todo.size() || !live.empty()) {
    while ((int)live.size() < in_flight && next < todo.size()) live.push_back(todo[next++]);
    const size_t k = next_rand(seed) % live.size();
    if (++steps > budget) return -1;
    if (union_step(parent.data(), live[k])) {
      live[k] = live.back();
      live.pop_back();
    }
  }
  for (int32_t p = 0; p < H * W; ++p) roots[p] = parent[p] < 0 ? -1 : find_root(parent.data(), p);
  return steps;
}
