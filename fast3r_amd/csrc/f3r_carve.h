// Workspace carving for the host side of the post-processing kernels.  A workspace's regions are listed once, in one function that takes
// them from a Carve: on a null base that function gives the size (the *_workspace_bytes entry points), on the caller's block the pointers,
// so a size and its layout cannot drift apart.  Plain C++, no HIP: tests/csrc/carve_host.cpp builds it with g++ under the sanitizers.
#pragma once

#include <cstddef>
#include <cstdint>

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

class Carve {  // bump allocator: every region starts at a multiple of `align` bytes from the base
 public:
  Carve(void* base, size_t align) : base_((char*)base), align_(align) {}
  template <typename T>
  T* take(size_t count) {  // `count` elements of T (null under a null base); moves on by their size rounded up to the alignment
    T* p = base_ ? (T*)(base_ + off_) : nullptr;
    off_ += (count * sizeof(T) + align_ - 1) / align_ * align_;
    return p;
  }
  size_t bytes() const { return off_; }

 private:
  char* base_;
  size_t align_, off_ = 0;
};
