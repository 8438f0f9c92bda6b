// gsr_carve.h - how an entry point describes its caller-owned workspace, ONCE: typed spans laid one behind another, each on a
// 256-byte boundary.  One function per workspace does the carving; called on a null base it only sizes the blob (x_ws(nullptr,
// n).total is what gsr_x_workspace_bytes returns), called on the caller's pointer it hands out the typed views the launches
// use - the same lines, so the element type and count of a span cannot differ between the two.  Host only, no HIP.
#pragma once

#include <stddef.h>

#ifdef __HIPCC__
#define GSR_CARVE_HD __host__ __device__
#else
#define GSR_CARVE_HD
#endif
static inline GSR_CARVE_HD size_t gsr_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct GsrCarve {
  char* base;      // nullptr: sizing only - every span comes back as nullptr
  size_t o = 0;    // bytes carved so far (a multiple of 256): the offset of the next span, the blob's total at the end
  explicit GsrCarve(const void* blob) : base((char*)blob) {}
  // `n` bytes handed on whole: a sub-workspace that another description carves
  char* bytes(size_t n) {
    char* p = base ? base + o : nullptr;
    o += gsr_align(n);
    return p;
  }
  template <class T> T* take(size_t n) { return (T*)bytes(n * sizeof(T)); }
};
