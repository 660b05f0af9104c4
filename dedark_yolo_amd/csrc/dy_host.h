// Host-side helpers shared by the C-ABI launchers: the dtype dispatches, the dynamic-LDS limit of the big-tile kernels, the NHWC
// view checks and the small grid / alignment helpers.  Nothing here is device code; the pure arithmetic (access width, overlap test,
// split plan) is dy_plan.h's.
#pragma once
#include <initializer_list>
#include <unordered_set>
#include "dy_common.h"
#include "dy_plan.h"

static inline int dy_elem_size(int dtype) { return dtype == DY_F32 ? 4 : 2; }   // bytes per element
static inline int dy_vec_elems(int dtype) { return dtype == DY_F32 ? 4 : 8; }   // elements per 16-byte vector (DT<T>::VE)

static inline int dy_check_dtype(const char* who, int dtype) {
  DY_CHECK(dtype == DY_F32 || dtype == DY_BF16 || dtype == DY_F16, "%s: bad dtype %d", who, dtype);
  return 0;
}

// The dtype is a launch parameter, the kernels want it as a type (the idea of bnact.hip's with_act): f is a generic lambda, called
// once with a tag whose ::type is float, f16_t or bf16_t.  Any other dtype value calls nothing, sets "<who>: bad dtype %d" and
// returns 1.
template <typename T> struct DyType { using type = T; };
template <typename F> inline int dy_dispatch_dtype(const char* who, int dtype, F&& f) {
  if (dtype == DY_F32) f(DyType<float>{});
  else if (dtype == DY_F16) f(DyType<f16_t>{});
  else if (dtype == DY_BF16) f(DyType<bf16_t>{});
  else return dy_check_dtype(who, dtype);
  return 0;
}
// The form the entries use: the statement sees the element type as T, a bad dtype returns from the entry.
//   DY_DISPATCH_DTYPE("dy_entry", dtype, kernel<T><<<grid, block, shm, st>>>((const T*)x, x_ld, (T*)y, y_ld, n));
//   DY_LAUNCH_CHECK();
#define DY_DISPATCH_DTYPE(who, dtype, ...)                                                      \
  do {                                                                                          \
    if (int e__ = dy_dispatch_dtype(who, dtype, [&](auto tag__) {                               \
          using T = typename decltype(tag__)::type;                                             \
          __VA_ARGS__;                                                                          \
        }))                                                                                     \
      return e__;                                                                               \
  } while (0)

// The kernels that exist for the two 16-bit types only: the same tag form, but f returns the launcher's status and that is what
// comes back; any other dtype calls nothing, sets "<who>: dtype %d is not a 16-bit type" and returns 1.
template <typename F> inline int dy_dispatch_16bit(const char* who, int dtype, F&& f) {
  if (dtype == DY_F16) return f(DyType<f16_t>{});
  if (dtype == DY_BF16) return f(DyType<bf16_t>{});
  DY_CHECK(false, "%s: dtype %d is not a 16-bit type", who, dtype);
  return 1;
}

// Raise the dynamic-LDS limit of kernels that use more than the default 64 KiB: each {kernel, bytes} pair is configured the first
// time it is passed and remembered, so a launcher calls this in front of every launch with the kernels it wants ready from then on
// (one kernel: configured at its own first launch; a whole family: all of them at the first launch of any).  Like the flags it
// replaces this expects the launchers to run on one host thread.  Returns 3 with "<family>: hipFuncSetAttribute failed: ..." set.
struct DyLdsLimit {
  const void* kernel;
  int bytes;
  template <typename K> DyLdsLimit(K* k, int b) : kernel(reinterpret_cast<const void*>(k)), bytes(b) {}
};
inline int dy_raise_lds_limit(const char* family, std::initializer_list<DyLdsLimit> kernels) {
  static std::unordered_set<const void*> raised;
  for (const DyLdsLimit& k : kernels) {
    if (raised.count(k.kernel)) continue;
    const hipError_t e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes);
    if (e != hipSuccess) {
      dy_set_error("%s: hipFuncSetAttribute failed: %s", family, hipGetErrorString(e));
      return 3;
    }
    raised.insert(k.kernel);
  }
  return 0;
}

// the NHWC view (pointer + pixel stride ld, C channels) every vectorised kernel takes: whole 16-byte vectors, 16-byte aligned rows
static inline int dy_check_view(const char* who, const void* p, long ld, int C, int dtype) {
  DY_CHECK(p != nullptr, "%s: null pointer", who);
  if (int e = dy_check_dtype(who, dtype)) return e;
  const int ve = dy_vec_elems(dtype);
  DY_CHECK(C > 0 && C % ve == 0, "%s: C=%d must be a multiple of %d", who, C, ve);
  DY_CHECK(ld >= C && (ld * dy_elem_size(dtype)) % 16 == 0 && ((uintptr_t)p) % 16 == 0, "%s: view not 16-byte aligned (ld=%ld)", who, ld);
  return 0;
}

// the same view for the kernels that touch exactly the lanes [0, C) of every pixel, element by element where they must: any
// element-aligned channel slice of a wider buffer, no vector demands
static inline int dy_check_lanes(const char* who, const void* p, long ld, int C, int dtype) {
  DY_CHECK(p != nullptr, "%s: null pointer", who);
  if (int e = dy_check_dtype(who, dtype)) return e;
  DY_CHECK(ld >= C && ((uintptr_t)p) % dy_elem_size(dtype) == 0, "%s: bad view (ld=%ld, C=%d)", who, ld, C);
  return 0;
}

// rows of ld elements can be read with 16-byte vectors
static inline bool dy_aligned16(const void* p, long ld, int elem_size) { return ((uintptr_t)p % 16) == 0 && (ld * elem_size) % 16 == 0; }

// blocks of 256 threads for a grid-stride loop over `total` items, at most `cap`
static inline int dy_ew_blocks(long total, int cap) {
  const long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// out[e] = sum_k part[k * E + e], k = 0 .. nparts-1 in index order (the second pass of a deterministic weight gradient); dwconv.hip
int dy_sum_partials(const float* part, int nparts, long E, float* out, hipStream_t stream);
