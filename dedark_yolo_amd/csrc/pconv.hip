// PConv, FasterNet's partial convolution (reference U/nn/modules/conv.py:157-190, n_div = 4, forward_split_cat): a bias-free
// 3x3 s1 p1 conv over the first c3 = C/4 channels, the other C - c3 channels passed through:
//   forward   y[.., :c3] = conv3x3(x[.., :c3], W)            y[.., c3:] = x[.., c3:]                      one launch
//   dgrad     dx[.., :c3] (+)= conv3x3^T(dy[.., :c3]) [+ s]   dx[.., c3:] (+)= dy[.., c3:] [+ s]          one launch
//   wgrad     dW[c3, c3, 3, 3] = sum_p dy[p, :c3] x x[p + tap, :c3], f32, deterministic             partials + fixed-order reduce
// 16-bit with c3 >= 16 runs the forward / dgrad on MFMA (pconv_mfma_kernel, weights packed per step by dy_pconv_pack); fp32 and
// c3 < 16 run the VALU kernel below.
//
// Channel bounds are exact: c3 and C need not be vector multiples, a view may be a channel slice of a wider buffer whose
// neighbouring lanes hold live data, so no kernel here reads a source lane outside [0, C) (the conv part reads only [0, c3)) or
// writes a destination lane outside [0, C).  That is why PConv is not "existing conv on the slice + copy": the tiled convs read
// and write whole 16-byte vectors (ops.padded_channels).  Source and destination may be slices of one buffer as long as their lanes do not
// overlap: a thread reads the halo that other threads write, so overlapping views are refused (dy_views_overlap).
//
// VALU route (fp32, c3 < 16): one thread per pixel keeps COB output-channel accumulators, each input value is loaded once and feeds COB FMAs against weights that
// sit in LDS as f32 (the whole [9][c3][COB] slab of the block's output-channel group; ds_read_b128, one address per wave = a
// broadcast).  Wider c3 splits the output channels over blockIdx.y so that the slab stays <= 64 KiB.
#include <hip/hip_runtime.h>

#include "dy_host.h"

namespace {

constexpr int PC_THREADS = 256;
constexpr int PC_LDS_MAX = 64 * 1024;       // bytes of weight slab per block (two blocks per CU on the 160 KiB LDS)

template <typename T>
__device__ inline float pld(const T* p) { return DT<T>::ld(p); }
template <typename T>
__device__ inline void pst(T* p, float v) { DT<T>::st(p, v); }

// One kernel for the forward and the data gradient: the data gradient of a 3x3 s1 p1 conv is the same conv over dy with the
// weights transposed (ci <-> co) and flipped (tap -> 8 - tap).  blockIdx.x: 256 consecutive pixels, blockIdx.y: output-channel
// group [co0, co0 + COB).  The y == 0 blocks also write the pass-through channels of their pixels.
template <typename T, int COB>
__global__ __launch_bounds__(PC_THREADS) void pconv_kernel(const T* __restrict__ src, long src_ld, T* __restrict__ dst, long dst_ld,
                                                           const float* __restrict__ w, int transposed, long pixels, int H, int W,
                                                           int C, int c3, int accumulate, const T* __restrict__ add, long add_ld) {
  extern __shared__ float wl[];             // [9 * c3][COB] f32
  const int co0 = blockIdx.y * COB;
  const int nw = 9 * c3 * COB;
  for (int i = threadIdx.x; i < nw; i += PC_THREADS) {
    const int j = i % COB, r = i / COB, ci = r % c3, tap = r / c3, co = co0 + j;
    float v = 0.f;
    if (co < c3) v = transposed ? w[((long)ci * c3 + co) * 9 + (8 - tap)] : w[((long)co * c3 + ci) * 9 + tap];
    wl[i] = v;
  }
  __syncthreads();
  const long pb = (long)blockIdx.x * PC_THREADS;
  const long p = pb + threadIdx.x;
  if (p < pixels) {
    const int wq = (int)(p % W), hq = (int)((p / W) % H);
    float acc[COB];
#pragma unroll
    for (int j = 0; j < COB; ++j) acc[j] = 0.f;
    for (int kh = 0; kh < 3; ++kh) {
      const int hh = hq + kh - 1;
      if (hh < 0 || hh >= H) continue;
      for (int kw = 0; kw < 3; ++kw) {
        const int ww = wq + kw - 1;
        if (ww < 0 || ww >= W) continue;
        const T* xp = src + (p + (long)(kh - 1) * W + (kw - 1)) * src_ld;
        const float4* wt = reinterpret_cast<const float4*>(wl + (kh * 3 + kw) * c3 * COB);
        for (int ci = 0; ci < c3; ++ci) {
          const float xv = pld(xp + ci);
#pragma unroll
          for (int j = 0; j < COB / 4; ++j) {
            const float4 q = wt[ci * (COB / 4) + j];
            acc[4 * j + 0] = fmaf(xv, q.x, acc[4 * j + 0]);
            acc[4 * j + 1] = fmaf(xv, q.y, acc[4 * j + 1]);
            acc[4 * j + 2] = fmaf(xv, q.z, acc[4 * j + 2]);
            acc[4 * j + 3] = fmaf(xv, q.w, acc[4 * j + 3]);
          }
        }
      }
    }
    T* yp = dst + p * dst_ld;
#pragma unroll
    for (int j = 0; j < COB; ++j) {
      const int co = co0 + j;
      if (co < c3) {
        float v = acc[j];
        if (accumulate) v += pld(yp + co);
        if (add) v += pld(add + p * add_ld + co);
        pst(yp + co, v);
      }
    }
  }
  if (blockIdx.y == 0) {                    // pass-through lanes [c3, C): channel-fastest walk, coalesced
    const int nc = C - c3;
    const long np = pixels - pb < PC_THREADS ? pixels - pb : PC_THREADS;
    for (long i = threadIdx.x; i < np * nc; i += PC_THREADS) {
      const long q = pb + i / nc;
      const int c = c3 + (int)(i % nc);
      float v = pld(src + q * src_ld + c);
      if (accumulate) v += pld(dst + q * dst_ld + c);
      if (add) v += pld(add + q * add_ld + c);
      pst(dst + q * dst_ld + c, v);
    }
  }
}

// Weight gradient, pass 1: blockIdx.x = (output-channel group, slice of 256 (tap, ci) pairs), blockIdx.y = pixel chunk.  Each
// thread owns one (tap, ci) pair and COB output channels; the block stages dy[64 pixels][COB] in LDS (read back as broadcasts),
// each thread loads x[p + tap][ci] itself (consecutive ci across a wave: coalesced).  Partial sums of chunk k go to
// part[k][co][ci][tap] (OIHW): no atomics.
constexpr int WG_TPX = 64;

template <typename T, int COB>
__global__ __launch_bounds__(PC_THREADS) void pconv_wgrad_kernel(const T* __restrict__ x, long x_ld, const T* __restrict__ dy,
                                                                 long dy_ld, float* __restrict__ part, long pixels, int H, int W,
                                                                 int c3, long chunk) {
  __shared__ float4 dyt4[WG_TPX * COB / 4];
  float* dyt = reinterpret_cast<float*>(dyt4);
  const int npairs = 9 * c3, nslices = (npairs + PC_THREADS - 1) / PC_THREADS;
  const int co0 = (blockIdx.x / nslices) * COB;
  const int task = (blockIdx.x % nslices) * PC_THREADS + threadIdx.x;
  const bool active = task < npairs;
  const int tap = active ? task / c3 : 0, ci = active ? task % c3 : 0;
  const int dh = tap / 3 - 1, dw = tap % 3 - 1;
  const long p0 = (long)blockIdx.y * chunk;
  const long p1 = p0 + chunk < pixels ? p0 + chunk : pixels;
  float acc[COB];
#pragma unroll
  for (int j = 0; j < COB; ++j) acc[j] = 0.f;
  for (long pb = p0; pb < p1; pb += WG_TPX) {
    const int n = p1 - pb < WG_TPX ? (int)(p1 - pb) : WG_TPX;
    __syncthreads();
    for (int i = threadIdx.x; i < WG_TPX * COB; i += PC_THREADS) {
      const int px = i / COB, co = co0 + i % COB;
      dyt[i] = (px < n && co < c3) ? pld(dy + (pb + px) * dy_ld + co) : 0.f;
    }
    __syncthreads();
    if (!active) continue;
    int wq = (int)(pb % W), hq = (int)((pb / W) % H);
    for (int px = 0; px < n; ++px) {
      const int hh = hq + dh, ww = wq + dw;
      if (hh >= 0 && hh < H && ww >= 0 && ww < W) {
        const float xv = pld(x + (pb + px + (long)dh * W + dw) * x_ld + ci);
        const float4* d4 = dyt4 + px * (COB / 4);
#pragma unroll
        for (int j = 0; j < COB / 4; ++j) {
          const float4 q = d4[j];
          acc[4 * j + 0] = fmaf(xv, q.x, acc[4 * j + 0]);
          acc[4 * j + 1] = fmaf(xv, q.y, acc[4 * j + 1]);
          acc[4 * j + 2] = fmaf(xv, q.z, acc[4 * j + 2]);
          acc[4 * j + 3] = fmaf(xv, q.w, acc[4 * j + 3]);
        }
      }
      if (++wq == W) {
        wq = 0;
        if (++hq == H) hq = 0;
      }
    }
  }
  if (!active) return;
  float* out = part + (long)blockIdx.y * c3 * c3 * 9;
#pragma unroll
  for (int j = 0; j < COB; ++j) {
    const int co = co0 + j;
    if (co < c3) out[((long)co * c3 + ci) * 9 + tap] = acc[j];
  }
}

// ---- 16-bit route, c3 >= 16: implicit GEMM on v_mfma_f32_16x16x32_{bf16,f16}.  A = packed weights (16 output channels x 32 input
// channels of one tap per fragment, from dy_pconv_pack), B = input pixels (32 channels x 16 pixels), f32 accumulate.  A block of 4 waves
// owns a 4-row x 16*MT-column pixel tile and ALL output channels: the c3 slice of the input halo tile is staged once in LDS (16-byte
// loads where the channel bounds and alignment allow, zero lanes past c3) and every input element is then read from LDS for its 9 taps.
// The same blocks copy the pass-through channels of their pixels (16-byte vectors where aligned).
constexpr int MF_TH = 4, MF_HR = MF_TH + 2;            // tile columns: 16 * MT (MT = 1 or 2 pixel fragments per wave)

template <typename T>
__global__ __launch_bounds__(PC_THREADS) void pconv_pack_kernel(const float* __restrict__ w, T* __restrict__ wp, int c3, int KC, int NT,
                                                                int transposed) {
  const long total = 9L * KC * NT * 512;
  for (long i = (long)blockIdx.x * PC_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * PC_THREADS) {
    const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
    long r = i >> 9;
    const int nt = (int)(r % NT);
    r /= NT;
    const int kc = (int)(r % KC), tap = (int)(r / KC);
    const int n = nt * 16 + (lane & 15), k = kc * 32 + (lane >> 4) * 8 + j;
    float v = 0.f;
    if (n < c3 && k < c3) v = transposed ? w[((long)k * c3 + n) * 9 + (8 - tap)] : w[((long)n * c3 + k) * 9 + tap];
    DT<T>::st(wp + i, v);
  }
}

template <typename T, int NT, int MT>
__global__ __launch_bounds__(PC_THREADS) void pconv_mfma_kernel(const T* __restrict__ src, long src_ld, T* __restrict__ dst, long dst_ld,
                                                                const T* __restrict__ wp, int H, int W, int C, int c3, int KC, int accumulate,
                                                                const T* __restrict__ add, long add_ld, int vec_in, int vec_pass) {
  constexpr int MF_TW = 16 * MT, MF_HC = MF_TW + 2;
  extern __shared__ __attribute__((aligned(16))) uint16_t tile[];      // [MF_HR][MF_HC][PS] 16-bit
  const int KP = KC * 32, PS = KP + 8;                                  // (+8: 16 B of row padding against LDS bank conflicts)
  const int w0 = blockIdx.x * MF_TW, h0 = blockIdx.y * MF_TH, n = blockIdx.z;
  const long img = (long)n * H * W;
  const int nchunk = KP / 8;
  for (int i = threadIdx.x; i < MF_HR * MF_HC * nchunk; i += PC_THREADS) {
    const int ch = (i % nchunk) * 8, pc = i / nchunk, c = pc % MF_HC, r = pc / MF_HC;
    const int hh = h0 - 1 + r, ww = w0 - 1 + c;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (hh >= 0 && hh < H && ww >= 0 && ww < W && ch < c3) {
      const T* p = src + (img + (long)hh * W + ww) * src_ld + ch;
      if (vec_in && ch + 8 <= c3) {
        v = *reinterpret_cast<const u32x4*>(p);
      } else {
        uint16_t e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = ch + j < c3 ? __builtin_bit_cast(uint16_t, p[j]) : (uint16_t)0;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (uint32_t)e[2 * j] | ((uint32_t)e[2 * j + 1] << 16);
      }
    }
    *reinterpret_cast<u32x4*>(tile + pc * PS + ch) = v;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const s16x8* wv = reinterpret_cast<const s16x8*>(wp);
  for (int kh = 0; kh < 3; ++kh)
    for (int kw = 0; kw < 3; ++kw) {
      const int tap = kh * 3 + kw;
      const uint16_t* trow = tile + ((wave + kh) * MF_HC + kw + (lane & 15)) * PS + (lane >> 4) * 8;
      for (int kc = 0; kc < KC; ++kc) {
        s16x8 b[MT];
#pragma unroll
        for (int m = 0; m < MT; ++m) b[m] = *reinterpret_cast<const s16x8*>(trow + m * 16 * PS + kc * 32);
        const s16x8* wa = wv + ((long)(tap * KC + kc) * NT) * 64 + lane;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const s16x8 a = wa[t * 64];
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m][t] = mfma_16x16x32<T>(a, b[m], acc[m][t]);
        }
      }
    }
  // D of 16x16x32: column (pixel) = lane & 15, rows (output channels) = 4 * (lane >> 4) + r
  const int h = h0 + wave;
  if (h < H) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int ww = w0 + m * 16 + (lane & 15);
      if (ww >= W) continue;
      const long q = img + (long)h * W + ww;
      T* yp = dst + q * dst_ld;
      const T* ap = add ? add + q * add_ld : nullptr;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = t * 16 + (lane >> 4) * 4 + r;
          if (co < c3) {
            float v = acc[m][t][r];
            if (accumulate) v += DT<T>::ld(yp + co);
            if (ap) v += DT<T>::ld(ap + co);
            DT<T>::st(yp + co, v);
          }
        }
    }
  }
  // pass-through lanes [c3, C) of the block's pixels
  const int nc = C - c3;
  const int npx = MF_TH * MF_TW;
  if (vec_pass) {
    const int nv = nc / 8;
    for (int i = threadIdx.x; i < npx * nv; i += PC_THREADS) {
      const int c = c3 + (i % nv) * 8, px = i / nv, hh = h0 + px / MF_TW, ww = w0 + px % MF_TW;
      if (hh >= H || ww >= W) continue;
      const long q = img + (long)hh * W + ww;
      if (!accumulate && !add) {
        *reinterpret_cast<u32x4*>(dst + q * dst_ld + c) = *reinterpret_cast<const u32x4*>(src + q * src_ld + c);
        continue;
      }
      float v[8], u[8];
      ldvec<T>(src + q * src_ld + c, v);
      if (accumulate) {
        ldvec<T>(dst + q * dst_ld + c, u);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += u[j];
      }
      if (add) {
        ldvec<T>(add + q * add_ld + c, u);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] += u[j];
      }
      stvec<T>(dst + q * dst_ld + c, v);
    }
  } else {
    for (int i = threadIdx.x; i < npx * nc; i += PC_THREADS) {
      const int c = c3 + i % nc, px = i / nc, hh = h0 + px / MF_TW, ww = w0 + px % MF_TW;
      if (hh >= H || ww >= W) continue;
      const long q = img + (long)hh * W + ww;
      float v = DT<T>::ld(src + q * src_ld + c);
      if (accumulate) v += DT<T>::ld(dst + q * dst_ld + c);
      if (add) v += DT<T>::ld(add + q * add_ld + c);
      DT<T>::st(dst + q * dst_ld + c, v);
    }
  }
}

template <typename T>
int launch_mfma(const void* src, long src_ld, void* dst, long dst_ld, const void* wp, int N, int H, int W, int C, int c3,
                int accumulate, const void* add, long add_ld, hipStream_t st) {
  const int KC = (c3 + 31) / 32, NT = (c3 + 15) / 16;
  const int vec_in = c3 % 8 == 0 && dy_aligned16(src, src_ld, sizeof(T));
  const int vec_pass = c3 % 8 == 0 && (C - c3) % 8 == 0 && vec_in && dy_aligned16(dst, dst_ld, sizeof(T)) &&
                       (add == nullptr || dy_aligned16(add, add_ld, sizeof(T)));
  // 32-column tiles unless 16-column ones waste fewer pixel slots at the right edge (W = 40: 48 vs 64 columns)
  const int MT = ((W + 15) / 16 * 16 - W) < ((W + 31) / 32 * 32 - W) ? 1 : 2, TW = 16 * MT;
  dim3 grid((unsigned)((W + TW - 1) / TW), (unsigned)((H + MF_TH - 1) / MF_TH), (unsigned)N);
  const size_t lds = (size_t)MF_HR * (TW + 2) * (KC * 32 + 8) * 2;
#define MF_GO(NT_)                                                                                                                     \
  case NT_:                                                                                                                            \
    if (MT == 1)                                                                                                                       \
      pconv_mfma_kernel<T, NT_, 1><<<grid, PC_THREADS, lds, st>>>((const T*)src, src_ld, (T*)dst, dst_ld, (const T*)wp, H, W, C, c3, \
                                                                  KC, accumulate, (const T*)add, add_ld, vec_in, vec_pass);        \
    else                                                                                                                               \
      pconv_mfma_kernel<T, NT_, 2><<<grid, PC_THREADS, lds, st>>>((const T*)src, src_ld, (T*)dst, dst_ld, (const T*)wp, H, W, C, c3, \
                                                                  KC, accumulate, (const T*)add, add_ld, vec_in, vec_pass);        \
    dy_note_kernel(MT == 1 ? "pconv_mfma_kernel<NT=" #NT_ ",MT=1>" : "pconv_mfma_kernel<NT=" #NT_ ",MT=2>");                        \
    break;
  switch (NT) {
    MF_GO(1) MF_GO(2) MF_GO(3) MF_GO(4) MF_GO(5) MF_GO(6) MF_GO(7) MF_GO(8)
    default: DY_CHECK(false, "pconv: c3=%d has no MFMA instantiation", c3);
  }
#undef MF_GO
  DY_LAUNCH_CHECK();
  return 0;
}

int pconv_cob(int c3) {                     // output channels per block: the smallest group that holds c3, within the LDS budget
  for (int cob : {8, 16, 32})
    if (cob >= c3 && 9 * c3 * cob * 4 <= PC_LDS_MAX) return cob;
  return 9 * c3 * 32 * 4 <= PC_LDS_MAX ? 32 : (9 * c3 * 16 * 4 <= PC_LDS_MAX ? 16 : 8);
}

template <typename T>
int launch_conv(const void* src, long src_ld, void* dst, long dst_ld, const float* w, int transposed, long pixels, int H, int W, int C,
                int c3, int accumulate, const void* add, long add_ld, hipStream_t st) {
  const int cob = pconv_cob(c3);
  dim3 grid((unsigned)((pixels + PC_THREADS - 1) / PC_THREADS), (unsigned)((c3 + cob - 1) / cob));
  const size_t lds = (size_t)9 * c3 * cob * sizeof(float);
#define PC_GO(COB_)                                                                                                                 \
  pconv_kernel<T, COB_><<<grid, PC_THREADS, lds, st>>>((const T*)src, src_ld, (T*)dst, dst_ld, w, transposed, pixels, H, W, C, c3, \
                                                       accumulate, (const T*)add, add_ld)
  if (cob == 8) PC_GO(8);
  else if (cob == 16) PC_GO(16);
  else PC_GO(32);
#undef PC_GO
  dy_note_kernel(cob == 8 ? "pconv_kernel<COB=8>" : (cob == 16 ? "pconv_kernel<COB=16>" : "pconv_kernel<COB=32>"));
  DY_LAUNCH_CHECK();
  return 0;
}

template <typename T>
int launch_wgrad(const void* x, long x_ld, const void* dy, long dy_ld, float* dw, long pixels, int H, int W, int c3, float* scratch,
                 long scratch_elems, hipStream_t st) {
  const long E = 9L * c3 * c3;
  const int cob = c3 <= 8 ? 8 : 16;
  const int nslices = (9 * c3 + PC_THREADS - 1) / PC_THREADS, ngroups = (c3 + cob - 1) / cob;
  DY_CHECK(scratch_elems >= E, "dy_pconv_wgrad: scratch of %ld floats < one partial of %ld", scratch_elems, E);
  // >= 2048 pixels of work per thread block, at most 512 chunks
  const dy_route::WgradSplits plan = dy_route::plan_wgrad_splits(pixels, 512, 2048, 1, scratch_elems / E, dy_route::kNoGridCap);
  const long nchunks = plan.splits, chunk = plan.chunk;
  dim3 grid((unsigned)(nslices * ngroups), (unsigned)nchunks);
  if (cob == 8)
    pconv_wgrad_kernel<T, 8><<<grid, PC_THREADS, 0, st>>>((const T*)x, x_ld, (const T*)dy, dy_ld, scratch, pixels, H, W, c3, chunk);
  else
    pconv_wgrad_kernel<T, 16><<<grid, PC_THREADS, 0, st>>>((const T*)x, x_ld, (const T*)dy, dy_ld, scratch, pixels, H, W, c3, chunk);
  DY_LAUNCH_CHECK();
  dy_note_kernel(cob == 8 ? "pconv_wgrad_kernel<COB=8>" : "pconv_wgrad_kernel<COB=16>");
  return dy_sum_partials(scratch, (int)nchunks, E, dw, st);
}

int check_common(const char* who, int N, int H, int W, int C, int c3, int dtype) {
  DY_CHECK(N > 0 && H > 0 && W > 0, "%s: bad shape %dx%dx%d", who, N, H, W);
  DY_CHECK(c3 >= 1 && c3 <= 128 && c3 <= C, "%s: c3=%d must be in [1, min(C=%d, 128)]", who, c3, C);
  return dy_check_dtype(who, dtype);
}

}  // namespace

static bool use_mfma(int c3, int dtype) { return dtype != DY_F32 && c3 >= 16; }

extern "C" int dy_pconv_pack(const float* w, void* wp, int c3, int transposed, int dtype, void* stream) {
  DY_CHECK(w && wp && c3 >= 16 && c3 <= 128 && (dtype == DY_BF16 || dtype == DY_F16),
           "dy_pconv_pack: bad args (16-bit weights for c3 in [16, 128])");
  const int KC = (c3 + 31) / 32, NT = (c3 + 15) / 16;
  const long total = 9L * KC * NT * 512;
  const unsigned blocks = (unsigned)((total + PC_THREADS - 1) / PC_THREADS);
  dy_note_kernel("pconv_pack_kernel");
  return dy_dispatch_16bit("dy_pconv_pack", dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    pconv_pack_kernel<T><<<blocks, PC_THREADS, 0, (hipStream_t)stream>>>(w, (T*)wp, c3, KC, NT, transposed ? 1 : 0);
    DY_LAUNCH_CHECK();
    return 0;
  });
}

extern "C" int dy_pconv_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, const float* w, const void* wp, int N, int H, int W,
                            int C, int c3, int dtype, void* stream) {
  if (int e = check_common("dy_pconv_fwd", N, H, W, C, c3, dtype)) return e;
  if (int e = dy_check_lanes("dy_pconv_fwd(x)", x, x_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_pconv_fwd(y)", y, y_ld, C, dtype)) return e;
  DY_CHECK(w != nullptr, "dy_pconv_fwd: null weight");
  DY_CHECK(!use_mfma(c3, dtype) || wp != nullptr, "dy_pconv_fwd: 16-bit c3=%d needs the packed weights of dy_pconv_pack", c3);
  DY_CHECK(!dy_views_overlap(x, x_ld, (long)N * H * W, C, y, y_ld, (long)N * H * W, C, dy_elem_size(dtype)),
           "dy_pconv_fwd: the lanes of x and y overlap (in-place or misplaced slices)");
  if (use_mfma(c3, dtype))
    return dy_dispatch_16bit("dy_pconv_fwd", dtype, [&](auto tag) {
      return launch_mfma<typename decltype(tag)::type>(x, x_ld, y, y_ld, wp, N, H, W, C, c3, 0, nullptr, 0, (hipStream_t)stream);
    });
  int r = 0;
  DY_DISPATCH_DTYPE("dy_pconv_fwd", dtype,
                    r = launch_conv<T>(x, x_ld, y, y_ld, w, 0, (long)N * H * W, H, W, C, c3, 0, nullptr, 0, (hipStream_t)stream));
  return r;
}

extern "C" int dy_pconv_dgrad(const void* dy, int64_t dy_ld, void* dx, int64_t dx_ld, const float* w, const void* wp, int N, int H,
                              int W, int C, int c3, int accumulate, const void* add_src, int64_t add_ld, int dtype, void* stream) {
  if (int e = check_common("dy_pconv_dgrad", N, H, W, C, c3, dtype)) return e;
  if (int e = dy_check_lanes("dy_pconv_dgrad(dy)", dy, dy_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_pconv_dgrad(dx)", dx, dx_ld, C, dtype)) return e;
  if (add_src)
    if (int e = dy_check_lanes("dy_pconv_dgrad(add_src)", add_src, add_ld, C, dtype)) return e;
  DY_CHECK(w != nullptr, "dy_pconv_dgrad: null weight");
  DY_CHECK(!use_mfma(c3, dtype) || wp != nullptr, "dy_pconv_dgrad: 16-bit c3=%d needs the transposed packed weights of dy_pconv_pack", c3);
  DY_CHECK(!dy_views_overlap(dy, dy_ld, (long)N * H * W, C, dx, dx_ld, (long)N * H * W, C, dy_elem_size(dtype)),
           "dy_pconv_dgrad: the lanes of dy and dx overlap (in-place or misplaced slices)");
  if (use_mfma(c3, dtype))
    return dy_dispatch_16bit("dy_pconv_dgrad", dtype, [&](auto tag) {
      return launch_mfma<typename decltype(tag)::type>(dy, dy_ld, dx, dx_ld, wp, N, H, W, C, c3, accumulate ? 1 : 0, add_src, add_ld,
                                                       (hipStream_t)stream);
    });
  int r = 0;
  DY_DISPATCH_DTYPE("dy_pconv_dgrad", dtype,
                    r = launch_conv<T>(dy, dy_ld, dx, dx_ld, w, 1, (long)N * H * W, H, W, C, c3, accumulate ? 1 : 0, add_src, add_ld,
                                       (hipStream_t)stream));
  return r;
}

extern "C" int dy_pconv_wgrad(const void* x, int64_t x_ld, const void* dy, int64_t dy_ld, float* dw, int N, int H, int W, int c3,
                              float* scratch, int64_t scratch_elems, int dtype, void* stream) {
  if (int e = check_common("dy_pconv_wgrad", N, H, W, c3, c3, dtype)) return e;
  if (int e = dy_check_lanes("dy_pconv_wgrad(x)", x, x_ld, c3, dtype)) return e;
  if (int e = dy_check_lanes("dy_pconv_wgrad(dy)", dy, dy_ld, c3, dtype)) return e;
  DY_CHECK(dw != nullptr && scratch != nullptr, "dy_pconv_wgrad: null dw / scratch");
  int r = 0;
  DY_DISPATCH_DTYPE("dy_pconv_wgrad", dtype,
                    r = launch_wgrad<T>(x, x_ld, dy, dy_ld, dw, (long)N * H * W, H, W, c3, scratch, scratch_elems, (hipStream_t)stream));
  return r;
}
