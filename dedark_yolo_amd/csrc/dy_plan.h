// The pure host arithmetic of the launchers: the access width and the overlap test of NHWC views and the split plan of a weight
// gradient's pixel loop.  Nothing here needs the HIP headers or DY_CHECK, so a host compiler takes this file alone
// (tests/test_launch_plan_cpu.py does).
#pragma once
#include <cstdint>

// widest access (in bytes: 16, 8 or 0 = one element) that pointer, pixel stride and channel count allow
inline int dy_view_bytes(const void* p, long ld, int C, int es) {
  const uintptr_t a = (uintptr_t)p;
  const long lb = ld * es, cb = (long)C * es;
  if (a % 16 == 0 && lb % 16 == 0 && cb % 16 == 0) return 16;
  if (a % 8 == 0 && lb % 8 == 0 && cb % 8 == 0) return 8;
  return 0;
}

// Do the sC lanes of a source view (sp pixels) and the dC lanes of a destination view (dp pixels) share a byte?  A thread reads a
// halo, or all channels of a pixel, that other threads write, so any overlap races.  Views whose extents are disjoint cannot; inside
// one buffer (equal pixel strides) the lane ranges [0, sC) and [0, dC) are compared modulo the pixel stride, which is exact;
// intersecting extents with different pixel strides are refused outright.
inline bool dy_views_overlap(const void* src, long s_ld, long sp, int sC, const void* dst, long d_ld, long dp, int dC, int es) {
  const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
  const uintptr_t scb = (uintptr_t)sC * es, dcb = (uintptr_t)dC * es;
  const uintptr_t s1 = s0 + (uintptr_t)(sp - 1) * s_ld * es + scb, d1 = d0 + (uintptr_t)(dp - 1) * d_ld * es + dcb;
  if (s1 <= d0 || d1 <= s0) return false;
  if (s_ld != d_ld) return true;
  const uintptr_t row = (uintptr_t)s_ld * es;
  const uintptr_t off = d0 >= s0 ? (d0 - s0) % row : (row - (s0 - d0) % row) % row;      // first destination byte within a source row
  return off < scb || row - off < dcb;
}

namespace dy_route {

// The M output pixels of a weight gradient in `splits` chunks of `chunk` pixels, one slab set (all tiles) per split: `want` splits
// (the caller's target block count over its tile count), no more than leave `min_pixels` per split, than `fit` slab sets in the
// scratch buffer (scratch_elems / slab_set_elems) or than `grid_cap`, at least one; the chunk is a whole number of `step`-pixel
// K-steps, and the splits are recounted for it.
struct WgradSplits {
  long splits, chunk;
};
constexpr long kGridDimYCap = 65535, kNoGridCap = 1L << 40;
inline WgradSplits plan_wgrad_splits(long M, long want, long min_pixels, long step, long fit, long grid_cap) {
  const long max_splits = (M + min_pixels - 1) / min_pixels;
  long splits = want < max_splits ? want : max_splits;
  if (splits > fit) splits = fit;
  if (splits < 1) splits = 1;
  if (splits > grid_cap) splits = grid_cap;
  long chunk = (M + splits - 1) / splits;
  chunk = (chunk + step - 1) / step * step;
  return {(M + chunk - 1) / chunk, chunk};
}

}  // namespace dy_route
