// The one way a workspace is laid out. Host code only; compiles as plain C++ (tests/native/ws_check.cpp).
// An op's workspace is a sequence of 256-byte aligned regions. Each op has one layout struct and one
// function that fills it by walking the regions once, over a base pointer that may be null: the
// *_workspace_bytes query is layout(nullptr, ...).bytes, the entry point checks the caller's size
// against the same value and launches with the pointers of the same struct, so a query and its carve
// cannot disagree. A layout function returns its struct as one braced list, the takes in region order
// and the walk's `off` last (a braced list is evaluated left to right). A region that several stages
// use one after the other in stream order is one take() of the largest stage layout's `bytes`; the
// compound op hands that region's pointer to the stage's launch, which lays it out with the stage's
// own function, so a stage's layout is written once too.
#pragma once
#include <stdint.h>
#include <algorithm>

namespace ast_ws {

inline int64_t al256(int64_t b) { return (b + 255) & ~(int64_t)255; }

struct Walk {
  unsigned char* base;  // null: only the sizes are wanted
  int64_t off = 0;      // the bytes taken so far, a multiple of 256: the layout's `bytes` at the end
  explicit Walk(void* b) : base((unsigned char*)b) {}
  // where the next region starts: the base that a compound op hands to a stage's layout function
  void* here() const { return base ? base + off : nullptr; }
  // the next region, of `bytes` bytes rounded up to 256
  template <class T>
  T* take(int64_t bytes) {
    T* p = (T*)here();
    off += al256(bytes);
    return p;
  }
};

}  // namespace ast_ws
