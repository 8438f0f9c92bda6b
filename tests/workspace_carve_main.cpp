// Stand-alone check of csrc/gsr_carve.h for tests/test_workspace_layouts_cpu.py: host compiler, AddressSanitizer and UBSan, no GPU.
// For every size it carves a made-up workspace that uses each span width, and the neighbour-search blob of csrc/knn_common.h
// (host code above that header's __HIPCC__ guard), twice: on a null base, which only sizes it, and on a malloc of exactly
// `total` bytes.  Both must give the same offsets; every span starts on a 256-byte boundary, behind the one declared before it,
// and ends inside the blob; the first and last element of every span are written - the sanitizer judges whether that stayed
// inside the allocation.  Prints one line per size; any failed check aborts.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "knn_common.h"

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      abort();                                                          \
    }                                                                   \
  } while (0)

struct Span { const char* name; char* p; size_t bytes; };      // a span as carved: where it starts, the bytes its elements take
template <class T> static Span span(const char* name, T* p, size_t n) { return Span{name, (char*)p, n * sizeof(T)}; }

// a workspace with 1-, 4-, 8-, 12- and 16-byte elements, a fixed 256-byte span, n + 1 elements and a nested blob
struct MixedWs {
  uint32_t* meta; uint8_t* flags; uint32_t* key; double* sum; float* xyz; float4* rec; uint32_t* start; char* nested;
  size_t nested_bytes, total;
};
static MixedWs mixed_ws(void* base, size_t n) {
  GsrCarve c(base);
  MixedWs w;
  w.meta = c.take<uint32_t>(64);
  w.flags = c.take<uint8_t>(n);
  w.key = c.take<uint32_t>(n);
  w.sum = c.take<double>(n);
  w.xyz = c.take<float>(3 * n);
  w.rec = c.take<float4>(n);
  w.start = c.take<uint32_t>(n + 1);
  w.nested_bytes = nn_ws(nullptr, n).total;
  w.nested = c.bytes(w.nested_bytes);
  w.total = c.o;
  return w;
}
static std::vector<Span> spans_of(const MixedWs& w, size_t n) {
  return {span("meta", w.meta, 64),     span("flags", w.flags, n), span("key", w.key, n),         span("sum", w.sum, n),
          span("xyz", w.xyz, 3 * n),    span("rec", w.rec, n),     span("start", w.start, n + 1), span("nested", w.nested, w.nested_bytes)};
}
static std::vector<Span> spans_of(const GsrNnWs& w, size_t P) {
  if (P == 0) P = 1;      // (the blob's own clamp)
  return {span("bbox", w.bbox, 64),
          span("pts", w.pts, P),
          span("box_lo", w.box_lo, knn_nbox(P)),
          span("box_hi", w.box_hi, knn_nbox(P)),
          span("sup_lo", w.sup_lo, knn_nsuper(P)),
          span("sup_hi", w.sup_hi, knn_nsuper(P)),
          span("bbox_part", w.bbox_part, GSR_KNN_BBOX_PART),
          span("key0", w.key[0], P),
          span("key1", w.key[1], P),
          span("val0", w.val[0], P),
          span("val1", w.val[1], P),
          span("radix_tmp", w.radix_tmp, gsr_radix_tmp_elems(P))};
}

// `sized`: carved on a null base; `viewed`: on `blob`, an allocation of exactly `total` bytes
static void check(const char* what, size_t n, const std::vector<Span>& sized, const std::vector<Span>& viewed, char* blob,
                  size_t total) {
  CHECK(sized.size() == viewed.size());
  CHECK(total % 256 == 0);
  size_t end = 0;      // where the span before ended
  for (size_t i = 0; i < viewed.size(); i++) {
    const Span& v = viewed[i];
    CHECK(sized[i].p == nullptr);
    CHECK(v.p != nullptr && v.bytes == sized[i].bytes && v.bytes > 0);
    const size_t off = (size_t)(v.p - blob);
    CHECK(off % 256 == 0);                       // aligned relative to the base
    CHECK(off >= end);                           // disjoint from, and behind, the span declared before it
    CHECK(off == gsr_align(end));                // ... with nothing but the rounding in between: the sizing pass's offset
    CHECK(off + v.bytes <= total);
    v.p[0] = (char)i;                            // first and last byte of the first and last element
    v.p[v.bytes - 1] = (char)i;
    end = off + v.bytes;
  }
  CHECK(gsr_align(end) == total);
  for (size_t i = 0; i < viewed.size(); i++) CHECK(viewed[i].p[0] == (char)i && viewed[i].p[viewed[i].bytes - 1] == (char)i);
  printf("%s n=%zu spans=%zu total=%zu ok\n", what, n, viewed.size(), total);
}

int main() {
  const size_t sizes[] = {0, 1, 63, 64, 65, 255, 256, 257, 100000};
  for (size_t n : sizes) {
    {
      const MixedWs s = mixed_ws(nullptr, n);
      char* blob = (char*)malloc(s.total);
      CHECK(blob);
      const MixedWs v = mixed_ws(blob, n);
      CHECK(v.total == s.total && v.nested_bytes == s.nested_bytes);
      if (n > 0) check("mixed", n, spans_of(s, n), spans_of(v, n), blob, s.total);
      else CHECK(s.total == gsr_align(256) + gsr_align(4) + gsr_align(s.nested_bytes));      // empty spans take no room
      free(blob);
    }
    {
      const GsrNnBlob s = nn_ws(nullptr, n);
      char* blob = (char*)malloc(s.total);
      CHECK(blob);
      const GsrNnBlob v = nn_ws(blob, n);
      CHECK(v.total == s.total && v.nn.keep == s.nn.keep);
      CHECK(v.nn.keep == (size_t)((char*)v.nn.bbox_part - blob));      // what a search reads ends where the build's scratch starts
      check("nn", n, spans_of(s.nn, n), spans_of(v.nn, n), blob, s.total);
      free(blob);
    }
  }
  return 0;
}
