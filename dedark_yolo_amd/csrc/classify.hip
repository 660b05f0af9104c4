// Classify task: global average pool, soft-max cross-entropy, eval soft-max, top-k and the accuracy counters.
// Replaces Classify's AdaptiveAvgPool2d(1) and softmax(1) (reference ultralytics/nn/modules/head.py:244-260), v8ClassificationLoss
// (ultralytics/utils/loss.py:380-385: cross_entropy(reduction='sum') / 64) and the argsort / compare of ClassificationValidator and
// ClassifyMetrics (ultralytics/models/yolo/classify/val.py:39-60, ultralytics/utils/metrics.py:197-207, 1018-1061).
//
// Every operand is addressed through its leading dimension (channel counts are padded, logits are never compacted).  A row is read
// with 16-byte vector loads where its base and leading dimension allow it, a scalar loop takes the tail.  Rows are one wave each:
//   soft-max statistics in ONE read of the row: every lane keeps a running maximum m and the sum s of exp(z - m), rescaled when m
//   grows; lanes merge pairwise, (m, s) + (m', s') = (M, s exp(m - M) + s' exp(m' - M)), M = max(m, m'), in the fixed butterfly order.
// No float atomics anywhere: the loss is summed by one block in a strided-then-tree order, so two runs give identical bytes.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

#include <math.h>

namespace {

constexpr int NT = 256;                 // threads per block
constexpr int ROWS = NT / 64;           // rows (waves) per block
constexpr int TOPK_MAX = 8;
constexpr float XENT_DIV = 64.f;        // the reference divides by the constant 64, not by the batch size

// ---- global average pool -------------------------------------------------------------------------------------------------------
// thread = one 16-byte channel group (or one tail channel) of one image; the HW loop stays inside the thread
template <typename T>
__global__ __launch_bounds__(NT) void gap_fwd_kernel(const T* __restrict__ x, long x_ld, int HW, int C, int nv, T* __restrict__ y, long y_ld,
                                                     bool y_vec) {
  constexpr int VE = DT<T>::VE;
  const int t = blockIdx.x * NT + threadIdx.x, n = blockIdx.y;
  const int tail = C - nv * VE;
  if (t >= nv + tail) return;
  const T* xi = x + (long)n * HW * x_ld;
  T* yi = y + (long)n * y_ld;
  const float hw = (float)HW;
  if (t < nv) {
    float acc[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) acc[e] = 0.f;
    for (int p = 0; p < HW; ++p) {
      float v[VE];
      ldvec<T>(xi + (long)p * x_ld + t * VE, v);
#pragma unroll
      for (int e = 0; e < VE; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) acc[e] = acc[e] / hw;
    if (y_vec) {
      stvec<T>(yi + t * VE, acc);
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) DT<T>::st(yi + t * VE + e, acc[e]);
    }
  } else {
    const int c = nv * VE + (t - nv);
    float acc = 0.f;
    for (int p = 0; p < HW; ++p) acc += DT<T>::ld(xi + (long)p * x_ld + c);
    DT<T>::st(yi + c, acc / hw);
  }
}

template <typename T>
__global__ __launch_bounds__(NT) void gap_bwd_kernel(const T* __restrict__ dy, long dy_ld, bool dy_vec, int HW, int C, int nv,
                                                     T* __restrict__ dx, long dx_ld) {
  constexpr int VE = DT<T>::VE;
  const int t = blockIdx.x * NT + threadIdx.x, n = blockIdx.y;
  const int tail = C - nv * VE;
  if (t >= nv + tail) return;
  const T* gi = dy + (long)n * dy_ld;
  T* xi = dx + (long)n * HW * dx_ld;
  const float hw = (float)HW;
  if (t < nv) {
    float g[VE];
    if (dy_vec) {
      ldvec<T>(gi + t * VE, g);
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) g[e] = DT<T>::ld(gi + t * VE + e);
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) g[e] = g[e] / hw;
    for (int p = 0; p < HW; ++p) stvec<T>(xi + (long)p * dx_ld + t * VE, g);
  } else {
    const int c = nv * VE + (t - nv);
    const float g = DT<T>::ld(gi + c) / hw;
    for (int p = 0; p < HW; ++p) DT<T>::st(xi + (long)p * dx_ld + c, g);
  }
}

// ---- one row, one wave ---------------------------------------------------------------------------------------------------------
// f(j, z_j) for the lane's share of row[0, n): vectors of VE elements when `vec`, then the scalar tail
template <typename T, typename F>
__device__ inline void row_each(const T* __restrict__ row, int n, int lane, bool vec, F f) {
  constexpr int VE = DT<T>::VE;
  const int nv = vec ? n / VE : 0;
  for (int v = lane; v < nv; v += 64) {
    float x[VE];
    ldvec<T>(row + v * VE, x);
#pragma unroll
    for (int e = 0; e < VE; ++e) f(v * VE + e, x[e]);
  }
  for (int j = nv * VE + lane; j < n; j += 64) f(j, DT<T>::ld(row + j));
}

struct MaxSum { float m, s; };

__device__ inline void ms_add(MaxSum& a, float z) {
  if (z > a.m) {                                   // (a NaN compares false and poisons s below, so it reaches the result)
    a.s = a.s * expf(a.m - z) + 1.f;               // first element: s = 0 * exp(-inf) + 1
    a.m = z;
  } else {
    a.s += z == -INFINITY ? 0.f : expf(z - a.m);     // (a leading -inf would give exp(-inf + inf))
  }
}
__device__ inline MaxSum ms_merge(MaxSum a, MaxSum b) {
  MaxSum r;
  r.m = fmaxf(a.m, b.m);
  const float fa = a.m == -INFINITY ? 0.f : expf(a.m - r.m);      // a lane without elements holds (-inf, 0)
  const float fb = b.m == -INFINITY ? 0.f : expf(b.m - r.m);
  r.s = a.s * fa + b.s * fb;
  return r;
}
// log-sum-exp statistics of the row in one read; the result is in every lane
template <typename T>
__device__ inline MaxSum row_maxsum(const T* __restrict__ row, int n, int lane, bool vec) {
  MaxSum a = {-INFINITY, 0.f};
  row_each<T>(row, n, lane, vec, [&](int, float z) { ms_add(a, z); });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    MaxSum b = {__shfl_xor(a.m, o, 64), __shfl_xor(a.s, o, 64)};
    // both partners must add in the same operand order, or their results differ in the last bit
    a = (lane & o) ? ms_merge(b, a) : ms_merge(a, b);
  }
  return a;
}

template <typename T>
__global__ __launch_bounds__(NT) void xent_lse_kernel(const T* __restrict__ logits, long ld, bool vec, int B, int nc, float* __restrict__ row_lse) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= B) return;
  const MaxSum a = row_maxsum<T>(logits + (long)b * ld, nc, lane, vec);
  if (lane == 0) row_lse[b] = a.m + logf(a.s);
}

// loss[0] = sum_b (lse_b - z[b, t_b]) / 64 over the rows with a label in [0, nc): thread i adds rows i, i + NT, ... in order, then a tree
template <typename T>
__global__ __launch_bounds__(NT) void xent_sum_kernel(const T* __restrict__ logits, long ld, const int64_t* __restrict__ cls, int B, int nc,
                                                      const float* __restrict__ row_lse, float* __restrict__ loss) {
  __shared__ float red[NT];
  float acc = 0.f;
  for (int b = threadIdx.x; b < B; b += NT) {
    const int64_t t = cls[b];
    if (t >= 0 && t < nc) acc += row_lse[b] - DT<T>::ld(logits + (long)b * ld + t);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] / XENT_DIV;
}

// dlogits[b, j] = (exp(z - lse_b) - [j == t_b]) * grad_out / 64 for j < nc (0 for an ignored row), 0 for nc <= j < dld
template <typename T>
__global__ __launch_bounds__(NT) void xent_bwd_kernel(const T* __restrict__ logits, long ld, bool vec, const int64_t* __restrict__ cls,
                                                      const float* __restrict__ row_lse, const float* __restrict__ grad_out, int B, int nc,
                                                      T* __restrict__ dlogits, long dld, bool dvec) {
  constexpr int VE = DT<T>::VE;
  const int lane = threadIdx.x & 63, b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= B) return;
  const T* row = logits + (long)b * ld;
  T* drow = dlogits + (long)b * dld;
  const int64_t t64 = cls[b];
  const bool valid = t64 >= 0 && t64 < nc;
  const int t = valid ? (int)t64 : -1;
  const float lse = row_lse[b], g = grad_out[0] / XENT_DIV;
  auto grad = [&](int j, float z) { return valid ? (expf(z - lse) - (j == t ? 1.f : 0.f)) * g : 0.f; };
  const int nv = (vec && dvec) ? nc / VE : 0;
  for (int v = lane; v < nv; v += 64) {
    float x[VE];
    ldvec<T>(row + v * VE, x);
#pragma unroll
    for (int e = 0; e < VE; ++e) x[e] = grad(v * VE + e, x[e]);
    stvec<T>(drow + v * VE, x);
  }
  for (int j = nv * VE + lane; j < nc; j += 64) DT<T>::st(drow + j, grad(j, DT<T>::ld(row + j)));
  for (long j = nc + lane; j < dld; j += 64) DT<T>::st(drow + j, 0.f);
}

// probs[b, j] = exp(z - m) / s: the statistics take one read of the row, the write pass reads it again (from cache) and stores
// 16 bytes of f32 at a time where the compact probs rows are 16-byte aligned (`pvec`: base aligned and nc a multiple of 4)
template <typename T>
__global__ __launch_bounds__(NT) void softmax_kernel(const T* __restrict__ logits, long ld, bool vec, int B, int nc, float* __restrict__ probs,
                                                     bool pvec) {
  constexpr int VE = DT<T>::VE;
  const int lane = threadIdx.x & 63, b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= B) return;
  const T* row = logits + (long)b * ld;
  const MaxSum a = row_maxsum<T>(row, nc, lane, vec);
  float* out = probs + (long)b * nc;
  const int nv = vec ? nc / VE : 0;
  for (int v = lane; v < nv; v += 64) {
    float x[VE];
    ldvec<T>(row + v * VE, x);
#pragma unroll
    for (int e = 0; e < VE; ++e) x[e] = expf(x[e] - a.m) / a.s;
    if (pvec) {
#pragma unroll
      for (int q = 0; q < VE; q += 4) stvec<float>(out + v * VE + q, x + q);
    } else {
#pragma unroll
      for (int e = 0; e < VE; ++e) out[v * VE + e] = x[e];
    }
  }
  for (int j = nv * VE + lane; j < nc; j += 64) out[j] = expf(DT<T>::ld(row + j) - a.m) / a.s;
}

// ---- top-k ---------------------------------------------------------------------------------------------------------------------
// 64-bit key, larger = earlier: the value mapped to an order-preserving uint32 (NaN -> 0, below -inf; -0 -> +0) in the high word,
// 0xFFFFFFFF - index in the low word, so equal values rank by ascending index.  0 = no candidate.
__device__ inline unsigned long long topk_key(float v, int j) {
  unsigned u = 0;
  if (v == v) {
    if (v == 0.f) v = 0.f;
    const unsigned bits = __builtin_bit_cast(unsigned, v);
    u = (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
  }
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)j);
}

template <typename T>
__global__ __launch_bounds__(NT) void topk_kernel(const T* __restrict__ scores, long ld, bool vec, int B, int nc, int k, int32_t* __restrict__ idx) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * ROWS + (threadIdx.x >> 6);
  if (b >= B) return;
  unsigned long long best[TOPK_MAX];              // the lane's own candidates, descending
#pragma unroll
  for (int i = 0; i < TOPK_MAX; ++i) best[i] = 0ull;
  row_each<T>(scores + (long)b * ld, nc, lane, vec, [&](int j, float v) {
    unsigned long long x = topk_key(v, j);
#pragma unroll
    for (int i = 0; i < TOPK_MAX; ++i) {
      const unsigned long long hi = x > best[i] ? x : best[i], lo = x > best[i] ? best[i] : x;
      best[i] = hi;
      x = lo;
    }
  });
  for (int r = 0; r < k; ++r) {
    unsigned long long w = best[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_xor(w, o, 64);
      w = other > w ? other : w;
    }
    if (w == best[0]) {                           // keys are unique (they hold the index): exactly one lane pops
#pragma unroll
      for (int i = 0; i + 1 < TOPK_MAX; ++i) best[i] = best[i + 1];
      best[TOPK_MAX - 1] = 0ull;
    }
    if (lane == 0) idx[(long)b * k + r] = (int32_t)(0xFFFFFFFFu - (unsigned)(w & 0xFFFFFFFFull));
  }
}

// ---- accuracy counters ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void metrics_kernel(const int32_t* __restrict__ idx, int k, const int64_t* __restrict__ cls, int B, int nc,
                                                     unsigned long long* __restrict__ counts, int32_t* __restrict__ confusion) {
  __shared__ int red[3][NT];
  const int b = blockIdx.x * NT + threadIdx.x;
  int n = 0, h1 = 0, h5 = 0;
  if (b < B) {
    const int64_t t = cls[b];
    if (t >= 0 && t < nc) {
      n = 1;
      const int p0 = idx[(long)b * k];
      h1 = p0 == (int)t;
      for (int r = 0; r < k; ++r) h5 |= idx[(long)b * k + r] == (int)t;
      if (confusion && p0 >= 0 && p0 < nc) atomicAdd(confusion + (long)p0 * nc + t, 1);
    }
  }
  red[0][threadIdx.x] = n; red[1][threadIdx.x] = h1; red[2][threadIdx.x] = h5;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3 && red[threadIdx.x][0]) atomicAdd(counts + threadIdx.x, (unsigned long long)red[threadIdx.x][0]);
}

}  // namespace

extern "C" int dy_gap_fwd(const void* x, int64_t x_ld, int N, int HW, int C, int dtype, void* y, int64_t y_ld, void* stream) {
  if (int e = dy_check_dtype("dy_gap_fwd", dtype)) return e;
  DY_CHECK(x && y && N > 0 && HW > 0 && C > 0 && x_ld >= C && y_ld >= C, "dy_gap_fwd: bad arguments (N %d HW %d C %d x_ld %ld y_ld %ld)", N,
           HW, C, (long)x_ld, (long)y_ld);
  DY_CHECK(N <= 65535, "dy_gap_fwd: N %d above 65535", N);
  const int es = dy_elem_size(dtype), ve = dy_vec_elems(dtype);
  const int nv = dy_aligned16(x, x_ld, es) ? C / ve : 0;
  const bool y_vec = dy_aligned16(y, y_ld, es);
  dim3 grid(dy_cdiv(nv + (C - nv * ve), NT), N);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("gap_fwd_kernel");
  DY_DISPATCH_DTYPE("dy_gap_fwd", dtype, gap_fwd_kernel<T><<<grid, NT, 0, st>>>((const T*)x, x_ld, HW, C, nv, (T*)y, y_ld, y_vec));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_gap_bwd(const void* dy, int64_t dy_ld, int N, int HW, int C, int dtype, void* dx, int64_t dx_ld, void* stream) {
  if (int e = dy_check_dtype("dy_gap_bwd", dtype)) return e;
  DY_CHECK(dy && dx && N > 0 && HW > 0 && C > 0 && dy_ld >= C && dx_ld >= C, "dy_gap_bwd: bad arguments (N %d HW %d C %d dy_ld %ld dx_ld %ld)",
           N, HW, C, (long)dy_ld, (long)dx_ld);
  DY_CHECK(N <= 65535, "dy_gap_bwd: N %d above 65535", N);
  const int es = dy_elem_size(dtype), ve = dy_vec_elems(dtype);
  const int nv = dy_aligned16(dx, dx_ld, es) ? C / ve : 0;
  const bool dy_vec = dy_aligned16(dy, dy_ld, es);
  dim3 grid(dy_cdiv(nv + (C - nv * ve), NT), N);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("gap_bwd_kernel");
  DY_DISPATCH_DTYPE("dy_gap_bwd", dtype, gap_bwd_kernel<T><<<grid, NT, 0, st>>>((const T*)dy, dy_ld, dy_vec, HW, C, nv, (T*)dx, dx_ld));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_cls_xent_fwd(const void* logits, int64_t ld, int dtype, const int64_t* cls, int B, int nc, float* row_lse, float* loss,
                               void* stream) {
  if (int e = dy_check_dtype("dy_cls_xent_fwd", dtype)) return e;
  DY_CHECK(logits && cls && row_lse && loss && B > 0 && nc > 0 && ld >= nc, "dy_cls_xent_fwd: bad arguments (B %d nc %d ld %ld)", B, nc, (long)ld);
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(logits, ld, es);
  const int grid = dy_cdiv(B, ROWS);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("xent_lse_kernel");
  DY_DISPATCH_DTYPE("dy_cls_xent_fwd", dtype, xent_lse_kernel<T><<<grid, NT, 0, st>>>((const T*)logits, ld, vec, B, nc, row_lse));
  DY_LAUNCH_CHECK();
  dy_note_kernel("xent_sum_kernel");
  DY_DISPATCH_DTYPE("dy_cls_xent_fwd", dtype, xent_sum_kernel<T><<<1, NT, 0, st>>>((const T*)logits, ld, cls, B, nc, row_lse, loss));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_cls_xent_bwd(const void* logits, int64_t ld, int dtype, const int64_t* cls, const float* row_lse, const float* grad_out,
                               int B, int nc, void* dlogits, int64_t dld, void* stream) {
  if (int e = dy_check_dtype("dy_cls_xent_bwd", dtype)) return e;
  DY_CHECK(logits && cls && row_lse && grad_out && dlogits && B > 0 && nc > 0 && ld >= nc && dld >= nc,
           "dy_cls_xent_bwd: bad arguments (B %d nc %d ld %ld dld %ld)", B, nc, (long)ld, (long)dld);
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(logits, ld, es), dvec = dy_aligned16(dlogits, dld, es);
  const int grid = dy_cdiv(B, ROWS);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("xent_bwd_kernel");
  DY_DISPATCH_DTYPE("dy_cls_xent_bwd", dtype,
                    xent_bwd_kernel<T><<<grid, NT, 0, st>>>((const T*)logits, ld, vec, cls, row_lse, grad_out, B, nc, (T*)dlogits, dld,
                                                            dvec));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_cls_softmax(const void* logits, int64_t ld, int dtype, int B, int nc, float* probs, void* stream) {
  if (int e = dy_check_dtype("dy_cls_softmax", dtype)) return e;
  DY_CHECK(logits && probs && B > 0 && nc > 0 && ld >= nc, "dy_cls_softmax: bad arguments (B %d nc %d ld %ld)", B, nc, (long)ld);
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(logits, ld, es);
  const int grid = dy_cdiv(B, ROWS);
  hipStream_t st = (hipStream_t)stream;
  const bool pvec = dy_aligned16(probs, nc, 4);
  dy_note_kernel("softmax_kernel");
  DY_DISPATCH_DTYPE("dy_cls_softmax", dtype, softmax_kernel<T><<<grid, NT, 0, st>>>((const T*)logits, ld, vec, B, nc, probs, pvec));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_cls_topk(const void* scores, int64_t ld, int dtype, int B, int nc, int k, int32_t* idx, void* stream) {
  if (int e = dy_check_dtype("dy_cls_topk", dtype)) return e;
  DY_CHECK(scores && idx && B > 0 && nc > 0 && ld >= nc, "dy_cls_topk: bad arguments (B %d nc %d ld %ld)", B, nc, (long)ld);
  DY_CHECK(k >= 1 && k <= nc && k <= TOPK_MAX, "dy_cls_topk: k %d outside [1, min(nc, %d)]", k, TOPK_MAX);
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(scores, ld, es);
  const int grid = dy_cdiv(B, ROWS);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("topk_kernel");
  DY_DISPATCH_DTYPE("dy_cls_topk", dtype, topk_kernel<T><<<grid, NT, 0, st>>>((const T*)scores, ld, vec, B, nc, k, idx));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_cls_metrics_update(const int32_t* idx, int k, const int64_t* cls, int B, int nc, int64_t* counts, int32_t* confusion,
                                     void* stream) {
  DY_CHECK(idx && cls && counts && B > 0 && nc > 0 && k >= 1, "dy_cls_metrics_update: bad arguments (B %d nc %d k %d)", B, nc, k);
  dy_note_kernel("metrics_kernel");
  metrics_kernel<<<dy_cdiv(B, NT), NT, 0, (hipStream_t)stream>>>(idx, k, cls, B, nc, reinterpret_cast<unsigned long long*>(counts), confusion);
  DY_LAUNCH_CHECK();
  return 0;
}
