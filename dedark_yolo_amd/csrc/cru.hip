// The convolutions of SCConv's channel reconstruction unit (reference ultralytics/nn/modules/conv.py:379-417) at any width C % 16 == 0,
// for the SCConv C2f family (block.py:418-470, 610-700) whose SCConv width is the C2f hidden width: 16 / 48 / 80 / ... channels, i.e.
// channel slices of 2, 6, 10 (GWC group inputs), 4, 12, 20 (squeezed halves) and 12, 36, 60 (PWC2) lanes that are no 16-byte vectors.
//
// One "CRU conv" is, per group g < G and output channel n < N of the group,
//   y[m][g N + n] = bias[g N + n] + sum_{tap < 9, ci < C3} x[m + off(tap)][g C3 + ci] w3[g N + n][ci][tap] + sum_{c < C1} x[m][c] w1[g N + n][c]
// the up branch Y1 = GWC(up') + PWC1(up') is (G, N, C3, C1) = (2, C/2, C/8, C/4): per group ONE GEMM with K = 9 C/8 + C/4 into one
// accumulator (no separate PWC1 tensor, no add pass); squeeze1 / squeeze2 / PWC2 are the same kernel with C3 = 0, G = 1.
//
// Forward and data gradient are one implicit-GEMM kernel: rows = output channels of the group (MFMA operand A, from a packed
// [G][rows][K] weight image in the compute dtype that dy_cru_conv_pack writes: forward order, or transposed + tap-flipped for the
// gather-form data gradient), columns = 64 consecutive pixels per block (operand B, gathered from the NHWC view), K = 9 S3 + S1 in
// tap-major order, walked in steps of 32: both operands of a step are staged in LDS as [row][32 + pad] (rows 80 bytes apart for the
// 16-bit types: the 16-byte fragment reads of 16 consecutive rows spread over all banks; 33 floats for f32), a wave owns 16 pixels and
// up to four 16-row blocks: v_mfma_f32_16x16x32 (bf16 / f16) or v_mfma_f32_16x16x4_f32, f32 accumulate.  With weights as operand A a
// lane ends up with 4 consecutive channels of one pixel.  K is padded to the step with zeros in LDS only; the gather reads exactly
// the channels of its slice (element loads when a slice is no whole vector, 16-byte loads when S3, S1 and the view allow it) and the
// epilogue writes exactly the rows of the group, so the views may be channel slices of wider buffers with live neighbours -- of one
// buffer too, as long as the source and the destination lanes do not overlap (a block reads all channels and the halo of its pixels
// while others write theirs: refused, dy_views_overlap).
//
// Weight gradient: per group a GEMM over the pixels, rows = dy channels, columns = the 9 C3 + C1 weight columns (+ one column of
// ones: the bias gradient); both operands are needed pixel-contiguous per channel: f32 stages them transposed ([channel][32 pixels]),
// the 16-bit types stage them as they lie in memory ([pixel][channel], 16-byte stores) and transpose in the read (ds_read_b64_tr_b16).
// Deterministic: the pixels are split into ranges by the shape alone, each block writes its f32 partial tile into the scratch, a
// second launch adds the ranges in a fixed order and scatters into the OIHW gradients; no atomics.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NT = 256;
constexpr int TM = 64;     // pixels per block of the forward / data gradient (16 per wave)
constexpr int TR = 64;     // rows per block: four 16-row MFMA blocks
constexpr int KC = 32;     // K per staged step

template <typename T> struct Tile {
  static constexpr int LD = KC + (sizeof(T) == 4 ? 1 : 8);
};

// 8 consecutive elements from a 16-byte aligned address
template <typename T> __device__ inline void load8(const T* p, T* v) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4*>(v) = *reinterpret_cast<const f32x4*>(p);
    *reinterpret_cast<f32x4*>(v + 4) = *reinterpret_cast<const f32x4*>(p + 4);
  } else {
    *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(p);
  }
}
template <typename T> __device__ inline T one_of() {
  if constexpr (sizeof(T) == 4) return 1.0f;
  else if constexpr (__is_same(T, f16_t)) return (f16_t)1.0f;
  else return (bf16_t)0x3F80;
}
template <typename T> __device__ inline T zero_of() {
  if constexpr (sizeof(T) == 4) return 0.0f;
  else if constexpr (__is_same(T, f16_t)) return (f16_t)0.0f;
  else return (bf16_t)0;
}
// 8 elements of one LDS row (v 16-byte aligned; the f32 rows are 33 floats apart: element stores)
template <typename T> __device__ inline void put8(T* row, const T* v) {
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int i = 0; i < 8; ++i) row[i] = v[i];
  } else {
    *reinterpret_cast<u32x4*>(row) = *reinterpret_cast<const u32x4*>(v);
  }
}

struct Gather {            // the im2col view of one group: k < K3: tap k / S3 of channel coff + k % S3; k < K3 + S1: channel k - K3 of the pixel
  long ld;
  int H, W, S3, S1, K3, coff, vec, ones;   // vec: 16-byte loads allowed; ones: column K3 + S1 reads 1 (the bias gradient's column)
};

// v[0..8) = columns k0 .. k0+7 of pixel (n, oh, ow); zeros outside the image, beyond the last column and for a dead pixel
template <typename T>
__device__ inline void gather8(const T* __restrict__ x, const Gather& gt, bool live, int n, int oh, int ow, int k0, T* v) {
  const T z = zero_of<T>();
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = z;
  if (!live) return;
  const int K = gt.K3 + gt.S1;
  if (gt.vec && k0 + 8 <= K) {                  // S3 % 8 == 0 and S1 % 8 == 0: the eight columns are eight channels of one tap
    if (k0 < gt.K3) {
      const int tap = k0 / gt.S3, ci = k0 - tap * gt.S3;
      const int sh = oh + tap / 3 - 1, sw = ow + tap % 3 - 1;
      if ((unsigned)sh < (unsigned)gt.H && (unsigned)sw < (unsigned)gt.W) load8<T>(x + (((long)n * gt.H + sh) * gt.W + sw) * gt.ld + gt.coff + ci, v);
    } else {
      load8<T>(x + (((long)n * gt.H + oh) * gt.W + ow) * gt.ld + (k0 - gt.K3), v);
    }
    return;
  }
  int tap = 0, ci = 0;
  if (k0 < gt.K3) {
    tap = k0 / gt.S3;
    ci = k0 - tap * gt.S3;
  }
  const T* centre = x + (((long)n * gt.H + oh) * gt.W + ow) * gt.ld;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    if (k < gt.K3) {
      const int sh = oh + tap / 3 - 1, sw = ow + tap % 3 - 1;
      if ((unsigned)sh < (unsigned)gt.H && (unsigned)sw < (unsigned)gt.W) v[i] = x[(((long)n * gt.H + sh) * gt.W + sw) * gt.ld + gt.coff + ci];
      if (++ci == gt.S3) {
        ci = 0;
        ++tap;
      }
    } else if (k < K) {
      v[i] = centre[k - gt.K3];
    } else if (k == K && gt.ones) {
      v[i] = one_of<T>();
    }
  }
}

template <typename T> __device__ inline void store4(T* o, const float* v) {
  if constexpr (sizeof(T) == 4) {
    *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
  } else if constexpr (__is_same(T, f16_t)) {
    typedef __attribute__((ext_vector_type(4))) _Float16 h4;
    *reinterpret_cast<h4*>(o) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
  } else {
    *reinterpret_cast<uint2*>(o) = uint2{pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
  }
}

// one K step of a wave over the 32 staged k of two [row][k] images: acc[nb] += A[a_row0 + 16 nb + row][k] * B[b_row0 + col][k]
// (a_is_blocked: `blocks` 16-row blocks of A against one block of B, the forward) or A[a_row0 + row][k] * B[b_row0 + 16 nb + col][k]
template <typename T, int NB>
__device__ inline void mfma_step(const T* __restrict__ As, int a_row0, int blocks, const T* __restrict__ Bs, int b_row0, bool a_is_blocked,
                                 f32x4* acc) {
  constexpr int LD = Tile<T>::LD;
  const int lane = threadIdx.x & 63, col = lane & 15, kg = lane >> 4;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int s = 0; s < KC / 4; ++s) {
      const float fixed = a_is_blocked ? Bs[(b_row0 + col) * LD + 4 * s + kg] : As[(a_row0 + col) * LD + 4 * s + kg];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) {
        if (nb < blocks) {
          if (a_is_blocked)
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[(a_row0 + 16 * nb + col) * LD + 4 * s + kg], fixed, acc[nb], 0, 0, 0);
          else
            acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(fixed, Bs[(b_row0 + 16 * nb + col) * LD + 4 * s + kg], acc[nb], 0, 0, 0);
        }
      }
    }
  } else {
    const u32x4 fixed = a_is_blocked ? *reinterpret_cast<const u32x4*>(Bs + (b_row0 + col) * LD + 8 * kg)
                                     : *reinterpret_cast<const u32x4*>(As + (a_row0 + col) * LD + 8 * kg);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (nb < blocks) {
        if (a_is_blocked)
          acc[nb] = mfma_16x16x32<T>(*reinterpret_cast<const u32x4*>(As + (a_row0 + 16 * nb + col) * LD + 8 * kg), fixed, acc[nb]);
        else
          acc[nb] = mfma_16x16x32<T>(fixed, *reinterpret_cast<const u32x4*>(Bs + (b_row0 + 16 * nb + col) * LD + 8 * kg), acc[nb]);
      }
    }
  }
}

// The 16x16x32 operand of a pixel-major LDS image [32 pixels][rs 16-bit elements]: lane (channel c0 + (lane & 15), k group lane >> 4)
// gets pixels 8 (lane >> 4) .. + 7 of its channel through two ds_read_b64_tr_b16 (a 16-lane group fetches 4 pixels x 16 channels, lane
// 4 q + p supplying the address of pixel q, channels 4 p .. 4 p + 3).  The whole wave must be active.
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;
template <typename T> __device__ inline u32x4 tr_frag(const T* img, int rs, int c0) {
  const int lane = threadIdx.x & 63, kg = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const T* a = img + (8 * kg + q) * rs + c0 + 4 * p;
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(a + 4 * rs));
  u32x4 v;
  v[0] = (uint32_t)(uint16_t)lo[0] | ((uint32_t)(uint16_t)lo[1] << 16);
  v[1] = (uint32_t)(uint16_t)lo[2] | ((uint32_t)(uint16_t)lo[3] << 16);
  v[2] = (uint32_t)(uint16_t)hi[0] | ((uint32_t)(uint16_t)hi[1] << 16);
  v[3] = (uint32_t)(uint16_t)hi[2] | ((uint32_t)(uint16_t)hi[3] << 16);
  return v;
}

// ---- forward / data gradient ------------------------------------------------------------------------------------------------------------
// grid (pixel tiles, row tiles, groups).  wp: [G][R][K] of T.  y[m][g R + r] = [y +] bias[g R + r] + sum_k wp[g][r][k] * col_k(x, m)
template <typename T>
__global__ __launch_bounds__(NT) void cru_conv_kernel(const T* __restrict__ x, Gather gt, const T* __restrict__ wp, const float* __restrict__ bias,
                                                      T* __restrict__ y, long y_ld, long M, int R, int S3g, int accumulate, int kvec, int ovec) {
  constexpr int LD = Tile<T>::LD;
  __shared__ __attribute__((aligned(16))) T Ws[TR * LD];
  __shared__ __attribute__((aligned(16))) T Xs[TM * LD];
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int g = blockIdx.z, r0 = blockIdx.y * TR;
  const long m0 = (long)blockIdx.x * TM;
  gt.coff = g * S3g;
  const int K = gt.K3 + gt.S1;
  const int rows = R - r0 < TR ? R - r0 : TR, rblocks = (rows + 15) >> 4;
  // staging role: row (weights) / pixel (activations) t >> 2, k octet t & 3 of every step
  const int srow = t >> 2, soct = t & 3;
  const long sm = m0 + srow;
  const bool live = sm < M;
  int n = 0, oh = 0, ow = 0;
  if (live) {
    const long hw = (long)gt.H * gt.W;
    n = (int)(sm / hw);
    const int rem = (int)(sm - (long)n * hw);
    oh = rem / gt.W;
    ow = rem - oh * gt.W;
  }
  const T* wrow = wp + ((long)g * R + r0 + srow) * K;
  const bool wlive = srow < rows;
  f32x4 acc[4];
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kc = 0; kc < K; kc += KC) {
    const int k0 = kc + 8 * soct;
    __attribute__((aligned(16))) T v[8];
    gather8<T>(x, gt, live, n, oh, ow, k0, v);
    put8<T>(Xs + srow * LD + 8 * soct, v);
    if (wlive && kvec && k0 + 8 <= K) {
      load8<T>(wrow + k0, v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (wlive && k0 + i < K) ? wrow[k0 + i] : zero_of<T>();
    }
    put8<T>(Ws + srow * LD + 8 * soct, v);
    __syncthreads();
    mfma_step<T, 4>(Ws, 0, rblocks, Xs, 16 * wave, true, acc);
    __syncthreads();
  }
  // lane (pixel col, group kg) holds rows 16 rb + 4 kg + i of its pixel
  const int col = lane & 15, kg = lane >> 4;
  const long m = m0 + 16 * wave + col;
  if (m >= M) return;
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int r = r0 + 16 * rb + 4 * kg;
    if (rb >= rblocks || r >= R) continue;
    T* o = y + m * y_ld + (long)g * R + r;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = acc[rb][i];
      if (r + i < R) {
        if (bias) v[i] += bias[g * R + r + i];
        if (accumulate) v[i] += DT<T>::ld(o + i);
      }
    }
    if (ovec && r + 4 <= R) {
      store4<T>(o, v);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (r + i < R) DT<T>::st(o + i, v[i]);
    }
  }
}

// ---- weight pack --------------------------------------------------------------------------------------------------------------------------
// transposed == 0: wp[g][n][k] = w3[g N + n][ci][tap] (k = tap C3 + ci) | w1[g N + n][c] (k = 9 C3 + c)
// transposed == 1, C3 > 0 (G C3 == C1): wp[g][ci][k] = w3[g N + n][ci][8 - tap] (k = tap N + n) | w1[c][g C3 + ci] (k = 9 N + c, c < G N)
// transposed == 1, C3 == 0 (G == 1):    wp[0][c1][n] = w1[n][c1]
template <typename T>
__global__ __launch_bounds__(NT) void cru_pack_kernel(const float* __restrict__ w3, const float* __restrict__ w1, T* __restrict__ wp, int G, int N,
                                                      int C3, int C1, int transposed) {
  const long total = (long)G * N * (9 * C3 + C1);
  for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    float v;
    if (!transposed) {
      const int K = 9 * C3 + C1;
      const int k = (int)(i % K);
      const long gn = i / K;
      if (k < 9 * C3) {
        const int tap = k / C3, ci = k - tap * C3;
        v = w3[(gn * C3 + ci) * 9 + tap];
      } else {
        v = w1[gn * C1 + (k - 9 * C3)];
      }
    } else if (C3 > 0) {
      const int K = 9 * N + G * N;
      const int k = (int)(i % K);
      const long gci = i / K;
      const int g = (int)(gci / C3), ci = (int)(gci - (long)g * C3);
      if (k < 9 * N) {
        const int tap = k / N, nn = k - tap * N;
        v = w3[(((long)g * N + nn) * C3 + ci) * 9 + (8 - tap)];
      } else {
        v = w1[(long)(k - 9 * N) * C1 + gci];
      }
    } else {
      const int nn = (int)(i % N);
      const long c1 = i / N;
      v = w1[(long)nn * C1 + c1];
    }
    DT<T>::st(wp + i, v);
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
// grid (pixel ranges, row tiles * column tiles, groups); part[s][g][n][j] (j < NC) = sum over the pixels of range s of dy[m][g N + n] * col_j(x, m)
template <typename T>
__global__ __launch_bounds__(NT) void cru_wgrad_kernel(const T* __restrict__ x, Gather gt, const T* __restrict__ dy, long dy_ld, float* __restrict__ part,
                                                       long M, long range, int N, int NC, int col_tiles, int S3g, int dvec) {
  // f32: both operands transposed by the staging stores, [channel][32 pixels + pad].  16-bit: pixel-major [pixel][64 channels + pad]
  // (one 16-byte store per thread and operand), transposed by the reads (tr_frag)
  constexpr int LD = Tile<T>::LD;
  constexpr int RS = TR + 8;
  constexpr bool TRR = sizeof(T) == 2;
  constexpr int ELEMS = TRR ? KC * RS : TR * LD;
  __shared__ __attribute__((aligned(16))) T Ds[ELEMS];        // dy channels x pixels
  __shared__ __attribute__((aligned(16))) T Xs[ELEMS];        // weight columns x pixels
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int g = blockIdx.z;
  const int rt = blockIdx.y / col_tiles, ct = blockIdx.y - rt * col_tiles;
  const int r0 = rt * TR, j0 = ct * TR;
  gt.coff = g * S3g;
  const long p0 = (long)blockIdx.x * range, p1 = p0 + range < M ? p0 + range : M;
  const int rows = N - r0 < TR ? N - r0 : TR;
  const int cols = NC - j0 < TR ? NC - j0 : TR, cblocks = (cols + 15) >> 4;
  // staging role: pixel t >> 3 of the step, channels / columns 8 (t & 7) .. + 7
  const int spx = t >> 3, soct = t & 7;
  const long hw = (long)gt.H * gt.W;
  f32x4 acc[4];
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (long pc = p0; pc < p1; pc += KC) {
    const long m = pc + spx;
    const bool live = m < p1;
    int n = 0, oh = 0, ow = 0;
    if (live) {
      n = (int)(m / hw);
      const int rem = (int)(m - (long)n * hw);
      oh = rem / gt.W;
      ow = rem - oh * gt.W;
    }
    __attribute__((aligned(16))) T v[8];
    const int rr = 8 * soct;
    const T* dp = dy + m * dy_ld + (long)g * N + r0 + rr;
    if (live && dvec && rr + 8 <= rows) {
      load8<T>(dp, v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = (live && rr + i < rows) ? dp[i] : zero_of<T>();
    }
    if constexpr (TRR) {
      put8<T>(Ds + spx * RS + rr, v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) Ds[(rr + i) * LD + spx] = v[i];
    }
    gather8<T>(x, gt, live, n, oh, ow, j0 + rr, v);
    if constexpr (TRR) {
      put8<T>(Xs + spx * RS + rr, v);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) Xs[(rr + i) * LD + spx] = v[i];
    }
    __syncthreads();
    if (16 * wave < rows) {                                   // (wave-uniform: the transposing reads need the whole wave)
      if constexpr (TRR) {
        const u32x4 a = tr_frag<T>(Ds, RS, 16 * wave);
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
          if (cb < cblocks) acc[cb] = mfma_16x16x32<T>(a, tr_frag<T>(Xs, RS, 16 * cb), acc[cb]);
      } else {
        mfma_step<T, 4>(Ds, 16 * wave, cblocks, Xs, 0, false, acc);
      }
    }
    __syncthreads();
  }
  // lane (column col, group kg) holds dy channels r0 + 16 wave + 4 kg + i of weight column j0 + 16 cb + col
  const int col = lane & 15, kg = lane >> 4;
  float* dst = part + (((long)blockIdx.x * gridDim.z + g) * N) * NC;
#pragma unroll
  for (int cb = 0; cb < 4; ++cb) {
    const int j = j0 + 16 * cb + col;
    if (cb >= cblocks || j >= NC) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + 16 * wave + 4 * kg + i;
      if (r < N) dst[(long)r * NC + j] = acc[cb][i];
    }
  }
}

// dw3 / dw1 / db = the ranges' partials added in a fixed order (overwrite): 16 threads per output element take the ranges
// k = lane, lane + 16, ... one after the other, their 16 sums are added in lane order
constexpr int RL = 16;
__global__ __launch_bounds__(NT) void cru_wgrad_reduce_kernel(const float* __restrict__ part, int splits, float* __restrict__ dw3, float* __restrict__ db,
                                                              float* __restrict__ dw1, int GN, int C3, int C1, int NC) {
  __shared__ float red[RL][NT / RL];
  const long total = (long)GN * NC;
  const int el = threadIdx.x & (NT / RL - 1), sl = threadIdx.x / (NT / RL);
  for (long base = (long)blockIdx.x * (NT / RL); base < total; base += (long)gridDim.x * (NT / RL)) {
    const long i = base + el;
    float s = 0.f;
    if (i < total)
      for (int k = sl; k < splits; k += RL) s += part[(long)k * total + i];
    red[sl][el] = s;
    __syncthreads();
    if (sl == 0 && i < total) {
      float t = 0.f;
#pragma unroll
      for (int r = 0; r < RL; ++r) t += red[r][el];
      const int j = (int)(i % NC);
      const long gn = i / NC;
      if (j < 9 * C3) {
        const int tap = j / C3, ci = j - tap * C3;
        if (dw3) dw3[(gn * C3 + ci) * 9 + tap] = t;
      } else if (j < 9 * C3 + C1) {
        if (dw1) dw1[gn * C1 + (j - 9 * C3)] = t;
      } else if (db) {
        db[gn] = t;
      }
    }
    __syncthreads();
  }
}

int check_shape(const char* who, int B, int H, int W, int G, int N, int C3, int C1) {
  DY_CHECK(B > 0 && H > 0 && W > 0 && (long)B * H * W < (1L << 31) - TM, "%s: bad image size %d x %d x %d", who, B, H, W);
  DY_CHECK((G == 1 || G == 2) && N > 0 && C3 >= 0 && C1 > 0 && (C3 == 0 ? G == 1 : G * C3 == C1) && (long)G * N <= 4096 && 9L * C3 + C1 <= 8192,
           "%s: unsupported CRU conv G=%d N=%d C3=%d C1=%d (3x3 group inputs must tile the 1x1 input)", who, G, N, C3, C1);
  return 0;
}

// x view of `rows` output rows per group from the gather (S3 per group at g S3, S1 at 0), K = 9 S3 + S1
int launch_conv(const char* who, const void* x, long x_ld, const void* wp, const float* bias, void* y, long y_ld, int B, int H, int W, int G, int R,
                int S3, int S1, int accumulate, int dtype, hipStream_t st) {
  const long M = (long)B * H * W;
  const int es = dy_elem_size(dtype);
  Gather gt;
  gt.ld = x_ld; gt.H = H; gt.W = W; gt.S3 = S3; gt.S1 = S1; gt.K3 = 9 * S3; gt.coff = 0; gt.ones = 0;
  gt.vec = (S3 % 8 == 0 && S1 % 8 == 0 && dy_aligned16(x, x_ld, es)) ? 1 : 0;
  const int K = 9 * S3 + S1;
  const int kvec = (K % 8 == 0 && ((uintptr_t)wp) % 16 == 0) ? 1 : 0;
  const int ovec = (R % 4 == 0 && ((uintptr_t)y) % (4 * es) == 0 && y_ld % 4 == 0) ? 1 : 0;
  const dim3 grid((unsigned)((M + TM - 1) / TM), (unsigned)((R + TR - 1) / TR), (unsigned)G);
  dy_note_kernel("cru_conv_kernel");
  DY_DISPATCH_DTYPE(who, dtype,
                    cru_conv_kernel<T><<<grid, NT, 0, st>>>((const T*)x, gt, (const T*)wp, bias, (T*)y, y_ld, M, R, S3, accumulate, kvec, ovec));
  DY_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int dy_cru_conv_pack(const float* w3, const float* w1, void* wp, int G, int N, int C3, int C1, int transposed, int dtype, void* stream) {
  if (int e = check_shape("dy_cru_conv_pack", 1, 1, 1, G, N, C3, C1)) return e;
  DY_CHECK(w1 && wp && (C3 == 0 || w3), "dy_cru_conv_pack: null pointer");
  const long total = (long)G * N * (9 * C3 + C1);
  hipStream_t st = (hipStream_t)stream;
  DY_DISPATCH_DTYPE("dy_cru_conv_pack", dtype,
                    cru_pack_kernel<T><<<dy_ew_blocks(total, 1024), NT, 0, st>>>(w3, w1, (T*)wp, G, N, C3, C1, transposed ? 1 : 0));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_cru_conv_fwd(const void* x, int64_t x_ld, const void* wp, const float* bias, void* y, int64_t y_ld, int B, int H, int W, int G, int N,
                               int C3, int C1, int dtype, void* stream) {
  if (int e = check_shape("dy_cru_conv_fwd", B, H, W, G, N, C3, C1)) return e;
  if (int e = dy_check_lanes("dy_cru_conv_fwd(x)", x, x_ld, C1, dtype)) return e;
  if (int e = dy_check_lanes("dy_cru_conv_fwd(y)", y, y_ld, G * N, dtype)) return e;
  DY_CHECK(wp != nullptr, "dy_cru_conv_fwd: null weight pack");
  DY_CHECK(!dy_views_overlap(x, x_ld, (long)B * H * W, C1, y, y_ld, (long)B * H * W, G * N, dy_elem_size(dtype)),
           "dy_cru_conv_fwd: the lanes of x and y overlap (in-place or misplaced slices)");
  return launch_conv("dy_cru_conv_fwd", x, x_ld, wp, bias, y, y_ld, B, H, W, G, N, C3, C1, 0, dtype, (hipStream_t)stream);
}

extern "C" int dy_cru_conv_dgrad(const void* dy, int64_t dy_ld, const void* wp, void* dx, int64_t dx_ld, int B, int H, int W, int G, int N, int C3,
                                 int C1, int accumulate, int dtype, void* stream) {
  if (int e = check_shape("dy_cru_conv_dgrad", B, H, W, G, N, C3, C1)) return e;
  if (int e = dy_check_lanes("dy_cru_conv_dgrad(dy)", dy, dy_ld, G * N, dtype)) return e;
  if (int e = dy_check_lanes("dy_cru_conv_dgrad(dx)", dx, dx_ld, C1, dtype)) return e;
  DY_CHECK(wp != nullptr, "dy_cru_conv_dgrad: null weight pack");
  DY_CHECK(!dy_views_overlap(dy, dy_ld, (long)B * H * W, G * N, dx, dx_ld, (long)B * H * W, C1, dy_elem_size(dtype)),
           "dy_cru_conv_dgrad: the lanes of dy and dx overlap (in-place or misplaced slices)");
  // rows: the C3 input channels of the group (all C1 for a pure 1x1); K = the group's N dy channels at nine taps + all G N at the centre
  const int R = C3 > 0 ? C3 : C1, S3 = C3 > 0 ? N : 0;
  return launch_conv("dy_cru_conv_dgrad", dy, dy_ld, wp, nullptr, dx, dx_ld, B, H, W, G, R, S3, G * N, accumulate ? 1 : 0, dtype, (hipStream_t)stream);
}

extern "C" int dy_cru_conv_wgrad(const void* x, int64_t x_ld, const void* dy, int64_t dy_ld, float* dw3, float* db, float* dw1, int B, int H, int W,
                                 int G, int N, int C3, int C1, float* scratch, int64_t scratch_elems, int dtype, void* stream) {
  if (int e = check_shape("dy_cru_conv_wgrad", B, H, W, G, N, C3, C1)) return e;
  if (int e = dy_check_lanes("dy_cru_conv_wgrad(x)", x, x_ld, C1, dtype)) return e;
  if (int e = dy_check_lanes("dy_cru_conv_wgrad(dy)", dy, dy_ld, G * N, dtype)) return e;
  const int NC = 9 * C3 + C1 + (db ? 1 : 0);
  const long slab = (long)G * N * NC;
  DY_CHECK(scratch && scratch_elems >= slab, "dy_cru_conv_wgrad: scratch of %ld floats needed", slab);
  const long M = (long)B * H * W;
  const int es = dy_elem_size(dtype);
  const int row_tiles = (N + TR - 1) / TR, col_tiles = (NC + TR - 1) / TR;
  // pixel ranges: whole steps of 32 pixels, about 1024 blocks in all, as many as the scratch holds; a function of the shape alone
  const dy_route::WgradSplits plan =
      dy_route::plan_wgrad_splits(M, 1024 / ((long)row_tiles * col_tiles * G), KC, KC, scratch_elems / slab, dy_route::kNoGridCap);
  const long splits = plan.splits, range = plan.chunk;
  Gather gt;
  gt.ld = x_ld; gt.H = H; gt.W = W; gt.S3 = C3; gt.S1 = C1; gt.K3 = 9 * C3; gt.coff = 0; gt.ones = db ? 1 : 0;
  gt.vec = (C3 % 8 == 0 && C1 % 8 == 0 && dy_aligned16(x, x_ld, es)) ? 1 : 0;
  const int dvec = (N % 8 == 0 && dy_aligned16(dy, dy_ld, es)) ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)splits, (unsigned)(row_tiles * col_tiles), (unsigned)G);
  dy_note_kernel("cru_wgrad_kernel");
  DY_DISPATCH_DTYPE("dy_cru_conv_wgrad", dtype,
                    cru_wgrad_kernel<T><<<grid, NT, 0, st>>>((const T*)x, gt, (const T*)dy, dy_ld, scratch, M, range, N, NC, col_tiles, C3, dvec));
  DY_LAUNCH_CHECK();
  const long rblocks = (slab + NT / RL - 1) / (NT / RL);
  cru_wgrad_reduce_kernel<<<(unsigned)(rblocks < 4096 ? rblocks : 4096), NT, 0, st>>>(scratch, (int)splits, dw3, db, dw1, G * N, C3, C1, NC);
  DY_LAUNCH_CHECK();
  return 0;
}
