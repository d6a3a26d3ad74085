// The workspace carver (fast3r_amd/csrc/f3r_carve.h) on the host, as a stand-alone program built with -fsanitize=address,undefined
// (tests/test_workspace_bytes.py).  For each list of regions: size it on a null base, malloc exactly that many bytes, carve, and write
// every byte of every region.  The asserts pin the totals and the alignment; AddressSanitizer then shows that the regions lie inside
// the block, and the byte patterns that no two of them overlap.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../fast3r_amd/csrc/f3r_carve.h"

namespace {

struct Odd {  // 20 bytes: a region whose size is no multiple of any alignment in use
  uint32_t w[5];
};

struct Region {
  int kind;  // 0: uint8_t, 1: uint32_t, 2: double, 3: Odd
  size_t count;
};
const size_t kSize[4] = {sizeof(uint8_t), sizeof(uint32_t), sizeof(double), sizeof(Odd)};

char* take(Carve& c, const Region& r) {
  switch (r.kind) {
    case 0: return (char*)c.take<uint8_t>(r.count);
    case 1: return (char*)c.take<uint32_t>(r.count);
    case 2: return (char*)c.take<double>(r.count);
    default: return (char*)c.take<Odd>(r.count);
  }
}

size_t up(size_t b, size_t a) { return (b + a - 1) / a * a; }

int run(const std::vector<Region>& regions, size_t align) {
  Carve sizing(nullptr, align);
  size_t expect = 0;
  for (const Region& r : regions) {
    assert(take(sizing, r) == nullptr);  // a null base hands out null pointers only
    expect += up(r.count * kSize[r.kind], align);
    assert(sizing.bytes() == expect);
  }
  const size_t total = sizing.bytes();
  assert(total % align == 0);
  // aligned_alloc: the device allocations the library carves are aligned to more than 256 bytes; `total` is a multiple of `align`
  char* block = total ? (char*)aligned_alloc(align < sizeof(void*) ? sizeof(void*) : align, total) : nullptr;
  assert(block || !total);
  Carve c(block, align);
  std::vector<char*> at;
  for (size_t i = 0; i < regions.size(); ++i) {
    const size_t before = c.bytes();
    char* p = take(c, regions[i]);
    if (total) {
      assert(p == block + before);
      assert(((uintptr_t)p) % align == 0 && (size_t)(p - block) % align == 0);
      memset(p, (int)(i + 1), regions[i].count * kSize[regions[i].kind]);  // every byte of the region
    } else {
      assert(p == nullptr);
    }
    at.push_back(p);
  }
  assert(c.bytes() == total);  // the carve pass ends where the sizing pass did
  for (size_t i = 0; i < regions.size() && total; ++i)  // nobody wrote into anybody else's region
    for (size_t b = 0; b < regions[i].count * kSize[regions[i].kind]; ++b) assert(at[i][b] == (char)(i + 1));
  free(block);
  return (int)regions.size();
}

}  // namespace

int main() {
  assert(align256(0) == 0 && align256(1) == 256 && align256(255) == 256 && align256(256) == 256 && align256(257) == 512);
  int n = 0;
  for (size_t align : {(size_t)8, (size_t)256}) {
    n += run({}, align);
    n += run({{1, 0}}, align);                                            // a lone zero-sized region: nothing to allocate
    n += run({{1, 1}, {1, 0}, {2, 3}}, align);                            // a zero-sized region between two others shares its address, not bytes
    n += run({{1, 63}, {1, 64}, {1, 65}, {0, 255}, {0, 256}, {0, 257}}, align);
    n += run({{3, 1}, {3, 13}, {0, 1}, {2, 4097}, {1, 4096}, {3, 0}, {0, 7}}, align);
    n += run({{1, 1000}, {1, 1000}, {1, 1000}, {1, 1000}, {1, 256 * 3 + 1}, {0, 512}}, align);  // the shape of a radix-sort workspace
  }
  printf("carve_host: %d regions ok\n", n);
  return 0;
}
