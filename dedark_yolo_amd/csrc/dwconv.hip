// Depthwise 2-D convolution (channel multiplier 1: c_in == c_out == groups), the nn.Conv2d(groups=C) inside DWConv / GhostConv /
// GhostBottleneck (reference U/nn/modules/conv.py:95-99,142-154, block.py:535-550): odd k <= 7, stride 1 or 2, pad = k / 2, dilation 1.
//   forward   y[n,oy,ox,c] = epilogue( sum_taps x[n, oy*s - pad + ky, ox*s - pad + kx, c] * w[c,ky,kx] )   or raw z + BN statistics
//   dgrad     dx[n,iy,ix,c] (+)= sum_taps dz[n,(iy+pad-ky)/s,(ix+pad-kx)/s,c] * w[c,ky,kx] [+ add]           gather form, no atomics
//   wgrad     dw[c,ky,kx]   = sum_{n,oy,ox} dz * x, f32                                                     partials + fixed-order reduce
// One weight row per channel and no reduction over channels: nothing for the MFMA unit to do, so these are VALU kernels that sit at
// the HBM roofline for 3x3 and near the ridge for 5x5 in 16-bit (25 FMA per 4 bytes).
//
// Work split: a thread owns V consecutive channels (one 16-byte, 8-byte or scalar access) and DW_TW = 4 consecutive output columns of
// one output row.  For each of the k input rows it streams the (DW_TW - 1) * s + k source columns once through registers and feeds
// every (output column, tap) pair they belong to, so a 5x5 s1 output costs 10 vector loads instead of 25.  The weights of the
// block's channel chunk sit in LDS as f32 [tap][channel] (flipped for the stride-1 data gradient, which is the same convolution);
// a thread reads the k taps of one kernel row as V-wide vectors once per input row.  Lanes run channel-fastest, so a wave's loads
// cover whole pixels.
//
// Channel bounds are exact: GhostConv is cat(y, dw5x5(y)), so source and destination are sibling channel slices of one buffer whose
// neighbouring lanes hold live data.  No kernel here reads a source lane outside [0, C) or writes a destination lane outside [0, C),
// for any C >= 1 and any slice offset: the launcher picks V = 16 bytes where every pointer, every pixel stride and C allow it, 8
// bytes where only those allow, and one element otherwise.
#include <hip/hip_runtime.h>

#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int DW_THREADS = 256;
constexpr int DW_TW = 4;                      // output columns per thread
constexpr int DW_CHUNK = 256;                 // channels per block at most (49 taps * 256 * 4 B = 49 KiB of LDS for k = 7)

// V elements of T <-> float registers in ONE access of V * sizeof(T) bytes (16, 8 or 4 bytes, or one element)
template <typename T, int V>
__device__ inline void ldv(const T* p, float* out) {
  if constexpr (V == DT<T>::VE) {
    ldvec<T>(p, out);
  } else if constexpr (V == 1) {
    out[0] = DT<T>::ld(p);
  } else if constexpr (sizeof(T) == 4) {      // 2 x f32
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    const f32x2 v = *reinterpret_cast<const f32x2*>(p);
    out[0] = v[0];
    out[1] = v[1];
  } else if constexpr (V == 2) {              // 2 x 16-bit (the k = 7 weight gradient)
    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
    out[0] = cvt32<T>((uint16_t)(v & 0xffffu));
    out[1] = cvt32<T>((uint16_t)(v >> 16));
  } else {                                    // 4 x 16-bit
    static_assert(V == 4, "16-bit accesses of 2, 4 or 8 elements");
    typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
    const u32x2 v = *reinterpret_cast<const u32x2*>(p);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      out[2 * i] = cvt32<T>((uint16_t)(v[i] & 0xffffu));
      out[2 * i + 1] = cvt32<T>((uint16_t)(v[i] >> 16));
    }
  }
}
template <typename T, int V>
__device__ inline void stv(T* p, const float* in) {
  if constexpr (V == DT<T>::VE) {
    stvec<T>(p, in);
  } else if constexpr (V == 1) {
    DT<T>::st(p, in[0]);
  } else if constexpr (sizeof(T) == 4) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    *reinterpret_cast<f32x2*>(p) = f32x2{in[0], in[1]};
  } else if constexpr (V == 2) {
    *reinterpret_cast<uint32_t*>(p) = (uint32_t)cvt16<T>(in[0]) | ((uint32_t)cvt16<T>(in[1]) << 16);
  } else {
    static_assert(V == 4, "16-bit accesses of 2, 4 or 8 elements");
    typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
    u32x2 v;
#pragma unroll
    for (int i = 0; i < 2; ++i) v[i] = (uint32_t)cvt16<T>(in[2 * i]) | ((uint32_t)cvt16<T>(in[2 * i + 1]) << 16);
    *reinterpret_cast<u32x2*>(p) = v;
  }
}

struct DwArgs {
  const void* src;      // forward: x      dgrad: dz
  long src_ld;
  void* dst;            // forward: y / z  dgrad: dx
  long dst_ld;
  const float* w;       // f32 [C][K][K]
  int N, Hs, Ws, Hd, Wd, C;
  int cbv;              // channel vectors per block (power of two), block chunk = cbv * V channels
  long groups;          // N * Hd * ceil(Wd / DW_TW)
  const float* scale;   // epilogue mode
  const float* shift;
  int act;
  double* stats;        // statistics mode: [DY_STATS_REPLICAS][2 * stats_c]
  int stats_c;
  int accumulate;       // dgrad
  int flip;             // stage the weights flipped (tap -> K*K - 1 - tap)
  const void* add;
  long add_ld;
};

// weights of channels [cb0, cb0 + CB) -> LDS [tap][CB]; flip: tap -> K*K - 1 - tap (the stride-1 data gradient)
template <int K>
__device__ inline void stage_weights(float* wl, const float* __restrict__ w, int cb0, int CB, int C, bool flip) {
  constexpr int KK = K * K;
  for (int i = threadIdx.x; i < KK * CB; i += DW_THREADS) {
    const int tap = i / CB, cl = i - tap * CB, c = cb0 + cl;
    wl[i] = c < C ? w[(long)c * KK + (flip ? KK - 1 - tap : tap)] : 0.f;
  }
}

// MODE 0: dst = conv_{K, S}(src) (the forward; with flipped weights and S = 1 the stride-1 data gradient).
// MODE 1: dst = the stride-2 data gradient of src = dz (S is 2): only taps with (i + pad - k) even and in range contribute.
// STATS: raw store + per-channel (sum, sum of squares) of the f32 accumulators; otherwise the affine / activation epilogue, or for a
// data gradient dst = [dst +] acc [+ add].
template <typename T, int V, int K, int S, int MODE, bool STATS>
__global__ __launch_bounds__(DW_THREADS) void dwconv_kernel(DwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float wl[];       // [K*K][CB]; the statistics mode appends 2 * CB doubles
  constexpr int PAD = K / 2;
  const int CB = a.cbv * V, cb0 = blockIdx.y * CB;
  stage_weights<K>(wl, a.w, cb0, CB, a.C, a.flip != 0);
  double* sred = reinterpret_cast<double*>(wl + ((K * K * CB + 1) & ~1));
  if (STATS)
    for (int i = threadIdx.x; i < 2 * CB; i += DW_THREADS) sred[i] = 0.0;
  __syncthreads();
  const int cvl = threadIdx.x & (a.cbv - 1), pgl = threadIdx.x / a.cbv, PG = DW_THREADS / a.cbv;
  const int c0 = cb0 + cvl * V;
  const bool cok = c0 < a.C;                                        // (C is a multiple of V: all V lanes are inside or all outside)
  const int GW = (a.Wd + DW_TW - 1) / DW_TW;
  const T* src = (const T*)a.src;
  T* dst = (T*)a.dst;
  const T* add = (const T*)a.add;
  const int accumulate = a.accumulate;
  double s1[STATS ? V : 1], s2[STATS ? V : 1];
#pragma unroll
  for (int v = 0; v < (STATS ? V : 1); ++v) s1[v] = s2[v] = 0.0;
  const float* wt = wl + cvl * V;
  for (long g = (long)blockIdx.x * PG + pgl; g < a.groups && cok; g += (long)gridDim.x * PG) {
    const int gx = (int)(g % GW);
    const long r = g / GW;
    const int dy_ = (int)(r % a.Hd), n = (int)(r / a.Hd);
    const int dx0 = gx * DW_TW;
    float acc[DW_TW][V];
#pragma unroll
    for (int t = 0; t < DW_TW; ++t)
#pragma unroll
      for (int v = 0; v < V; ++v) acc[t][v] = 0.f;
    if constexpr (MODE == 0) {
      constexpr int NC = (DW_TW - 1) * S + K;
      const int sx0 = dx0 * S - PAD;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int sy = dy_ * S - PAD + ky;
        if (sy < 0 || sy >= a.Hs) continue;
        float wr[K][V];
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int v = 0; v < V; ++v) wr[kx][v] = wt[(ky * K + kx) * CB + v];
        const T* rp = src + (((long)n * a.Hs + sy) * a.Ws) * a.src_ld + c0;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
          const int sx = sx0 + j;
          float xv[V];
          if (sx >= 0 && sx < a.Ws) {
            ldv<T, V>(rp + (long)sx * a.src_ld, xv);
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v) xv[v] = 0.f;
          }
#pragma unroll
          for (int t = 0; t < DW_TW; ++t) {
            const int kx = j - t * S;                               // compile-time after unrolling
            if (kx >= 0 && kx < K) {
#pragma unroll
              for (int v = 0; v < V; ++v) acc[t][v] = fmaf(xv[v], wr[kx][v], acc[t][v]);
            }
          }
        }
      }
    } else {
      // dx column dx0 + t takes dz column (dx0 + t + PAD - kx) / 2 when that is an integer; dx0 is a multiple of DW_TW (even), so
      // the parity of (t + PAD - kx) decides at compile time.  d = (t + PAD - kx) / 2 runs over [DMIN, DMAX].
      constexpr int DMIN = -(PAD / 2), DMAX = (DW_TW - 1 + PAD) / 2;
      const int zx0 = dx0 / 2;
#pragma unroll
      for (int ky = 0; ky < K; ++ky) {
        const int num = dy_ + PAD - ky;
        if (num < 0 || (num & 1)) continue;
        const int zy = num >> 1;
        if (zy >= a.Hs) continue;
        float wr[K][V];
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
          for (int v = 0; v < V; ++v) wr[kx][v] = wt[(ky * K + kx) * CB + v];
        const T* rp = src + (((long)n * a.Hs + zy) * a.Ws) * a.src_ld + c0;
#pragma unroll
        for (int d = DMIN; d <= DMAX; ++d) {
          const int zx = zx0 + d;
          float zv[V];
          if (zx >= 0 && zx < a.Ws) {
            ldv<T, V>(rp + (long)zx * a.src_ld, zv);
          } else {
#pragma unroll
            for (int v = 0; v < V; ++v) zv[v] = 0.f;
          }
#pragma unroll
          for (int t = 0; t < DW_TW; ++t) {
            const int kx = t + PAD - 2 * d;
            if (kx >= 0 && kx < K) {
#pragma unroll
              for (int v = 0; v < V; ++v) acc[t][v] = fmaf(zv[v], wr[kx][v], acc[t][v]);
            }
          }
        }
      }
    }
    T* yp = dst + (((long)n * a.Hd + dy_) * a.Wd + dx0) * a.dst_ld + c0;
    if constexpr (STATS) {
#pragma unroll
      for (int t = 0; t < DW_TW; ++t) {
        if (dx0 + t >= a.Wd) break;
#pragma unroll
        for (int v = 0; v < V; ++v) {
          s1[v] += (double)acc[t][v];
          s2[v] += (double)(acc[t][v] * acc[t][v]);                // f32 addends: the f64 sums do not depend on their order
        }
        stv<T, V>(yp + (long)t * a.dst_ld, acc[t]);
      }
    } else if (add != nullptr || accumulate) {
      const T* ap = add ? add + (((long)n * a.Hd + dy_) * a.Wd + dx0) * a.add_ld + c0 : nullptr;
#pragma unroll
      for (int t = 0; t < DW_TW; ++t) {
        if (dx0 + t >= a.Wd) break;
        float u[V];
        if (accumulate) {
          ldv<T, V>(yp + (long)t * a.dst_ld, u);
#pragma unroll
          for (int v = 0; v < V; ++v) acc[t][v] += u[v];
        }
        if (ap) {
          ldv<T, V>(ap + (long)t * a.add_ld, u);
#pragma unroll
          for (int v = 0; v < V; ++v) acc[t][v] += u[v];
        }
        stv<T, V>(yp + (long)t * a.dst_ld, acc[t]);
      }
    } else {
      float sc[V], sh[V];
#pragma unroll
      for (int v = 0; v < V; ++v) {
        sc[v] = a.scale ? a.scale[c0 + v] : 1.f;
        sh[v] = a.shift ? a.shift[c0 + v] : 0.f;
      }
#pragma unroll
      for (int t = 0; t < DW_TW; ++t) {
        if (dx0 + t >= a.Wd) break;
#pragma unroll
        for (int v = 0; v < V; ++v) acc[t][v] = dy_act(a.act, fmaf(acc[t][v], sc[v], sh[v]));
        stv<T, V>(yp + (long)t * a.dst_ld, acc[t]);
      }
    }
  }
  if constexpr (STATS) {
    // lanes of a wave that share cvl sit cbv apart: xor tree over them, then one LDS add per (wave, channel), then one global f64
    // atomic per (block, channel) into the block's replica
#pragma unroll
    for (int v = 0; v < V; ++v) {
      for (int o = 32; o >= a.cbv && o > 0; o >>= 1) {
        s1[v] += __shfl_xor(s1[v], o, 64);
        s2[v] += __shfl_xor(s2[v], o, 64);
      }
    }
    const int lane = threadIdx.x & 63;
    if (cok && (a.cbv >= 64 || lane < a.cbv)) {
#pragma unroll
      for (int v = 0; v < V; ++v) {
        atomicAdd(&sred[cvl * V + v], s1[v]);
        atomicAdd(&sred[CB + cvl * V + v], s2[v]);
      }
    }
    __syncthreads();
    double* rep = a.stats + (long)(blockIdx.x % DY_STATS_REPLICAS) * 2 * a.stats_c;
    for (int i = threadIdx.x; i < CB; i += DW_THREADS) {
      const int c = cb0 + i;
      if (c < a.C) {
        atomic_add_f64(rep + c, sred[i]);
        atomic_add_f64(rep + a.stats_c + c, sred[CB + i]);
      }
    }
  }
}

// Weight gradient, pass 1: the forward's work split; a thread keeps the K*K partial sums of its V channels over all its pixel groups
// (V is capped so that they fit the register file), the block adds its threads' partials tap by tap through LDS in a fixed order and
// writes part[blockIdx.x][c][tap].  No atomics.
template <typename T, int V, int K, int S>
__global__ __launch_bounds__(DW_THREADS) void dwconv_wgrad_kernel(const T* __restrict__ x, long x_ld, const T* __restrict__ dz, long dz_ld,
                                                                  float* __restrict__ part, int N, int H, int W, int Ho, int Wo, int C,
                                                                  int cbv, long groups) {
  __shared__ float red[DW_THREADS * V];
  constexpr int PAD = K / 2, KK = K * K, NC = (DW_TW - 1) * S + K;
  const int CB = cbv * V, cb0 = blockIdx.y * CB;
  const int cvl = threadIdx.x & (cbv - 1), pgl = threadIdx.x / cbv, PG = DW_THREADS / cbv;
  const int c0 = cb0 + cvl * V;
  const bool cok = c0 < C;
  const int GW = (Wo + DW_TW - 1) / DW_TW;
  float acc[KK][V];
#pragma unroll
  for (int i = 0; i < KK; ++i)
#pragma unroll
    for (int v = 0; v < V; ++v) acc[i][v] = 0.f;
  for (long g = (long)blockIdx.x * PG + pgl; g < groups && cok; g += (long)gridDim.x * PG) {
    const int gx = (int)(g % GW);
    const long r = g / GW;
    const int oy = (int)(r % Ho), n = (int)(r / Ho);
    const int ox0 = gx * DW_TW, sx0 = ox0 * S - PAD;
    float gz[DW_TW][V];
    const T* zp = dz + (((long)n * Ho + oy) * Wo + ox0) * dz_ld + c0;
#pragma unroll
    for (int t = 0; t < DW_TW; ++t) {
      if (ox0 + t < Wo) {
        ldv<T, V>(zp + (long)t * dz_ld, gz[t]);
      } else {
#pragma unroll
        for (int v = 0; v < V; ++v) gz[t][v] = 0.f;
      }
    }
#pragma unroll
    for (int ky = 0; ky < K; ++ky) {
      const int sy = oy * S - PAD + ky;
      if (sy < 0 || sy >= H) continue;
      const T* rp = x + (((long)n * H + sy) * W) * x_ld + c0;
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int sx = sx0 + j;
        if (sx < 0 || sx >= W) continue;
        float xv[V];
        ldv<T, V>(rp + (long)sx * x_ld, xv);
#pragma unroll
        for (int t = 0; t < DW_TW; ++t) {
          const int kx = j - t * S;
          if (kx >= 0 && kx < K) {
#pragma unroll
            for (int v = 0; v < V; ++v) acc[ky * K + kx][v] = fmaf(xv[v], gz[t][v], acc[ky * K + kx][v]);
          }
        }
      }
    }
  }
  float* out = part + (long)blockIdx.x * C * KK;
#pragma unroll
  for (int tap = 0; tap < KK; ++tap) {
    __syncthreads();
#pragma unroll
    for (int v = 0; v < V; ++v) red[threadIdx.x * V + v] = acc[tap][v];
    __syncthreads();
    if ((int)threadIdx.x < CB) {
      const int cl = threadIdx.x / V, v = threadIdx.x % V, c = cb0 + threadIdx.x;
      if (c < C) {
        float s = 0.f;
        for (int pg = 0; pg < PG; ++pg) s += red[(pg * cbv + cl) * V + v];
        out[(long)c * KK + tap] = s;
      }
    }
  }
}

// pass 2 of this and of PConv's weight gradient (dy_sum_partials): out[e] = sum_k part[k][e] in index order
__global__ __launch_bounds__(DW_THREADS) void sum_partials_kernel(const float* __restrict__ part, float* __restrict__ out, long E,
                                                                  int nparts) {
  const long e = (long)blockIdx.x * DW_THREADS + threadIdx.x;
  if (e >= E) return;
  float s = 0.f;
  for (int k = 0; k < nparts; ++k) s += part[(long)k * E + e];
  out[e] = s;
}

// exact-bounds strided copy / add of pixels x C lanes (the twin of dy_copy2d for views that are not vector-aligned)
template <typename T>
__global__ __launch_bounds__(DW_THREADS) void copy2d_exact_kernel(const T* __restrict__ src, long src_ld, T* __restrict__ dst, long dst_ld,
                                                                  long total, int C, int accumulate) {
  for (long i = (long)blockIdx.x * DW_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * DW_THREADS) {
    const long p = i / C;
    const int c = (int)(i - p * C);
    float v = DT<T>::ld(src + p * src_ld + c);
    if (accumulate) v += DT<T>::ld(dst + p * dst_ld + c);
    DT<T>::st(dst + p * dst_ld + c, v);
  }
}

// ---- host side
int pow2_ceil(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

struct DwGeom {
  int K, S, N, H, W, Ho, Wo, C;
};

int check_geom(const char* who, const DwGeom& g, int dtype) {
  if (int e = dy_check_dtype(who, dtype)) return e;
  DY_CHECK(g.N > 0 && g.H > 0 && g.W > 0 && g.C >= 1, "%s: bad shape %dx%dx%dx%d", who, g.N, g.H, g.W, g.C);
  DY_CHECK(g.K == 3 || g.K == 5 || g.K == 7, "%s: k=%d (odd k in 3..7)", who, g.K);
  DY_CHECK(g.S == 1 || g.S == 2, "%s: stride=%d (1 or 2)", who, g.S);
  DY_CHECK((long)g.N * g.H * g.W < (1L << 31), "%s: more than 2^31 pixels", who);
  return 0;
}

unsigned grid_x(long groups, int PG, int ny) {
  long need = (groups + PG - 1) / PG;
  const long cap = 8192 / (ny < 1 ? 1 : ny) + 1;              // grid-stride beyond this: the weights are staged once per block
  if (need > cap) need = cap;
  return (unsigned)(need < 1 ? 1 : need);
}

template <typename T, int V, int K, int S, int MODE, bool STATS>
int launch_one(const DwArgs& a0, hipStream_t st, const char* name) {
  DwArgs a = a0;
  const int CV = (a.C + V - 1) / V;
  int cbv = pow2_ceil(CV);
  const int cap = DW_CHUNK / V < 64 ? DW_CHUNK / V : 64;
  if (cbv > cap) cbv = cap;
  a.cbv = cbv;
  const int CB = cbv * V, ny = (a.C + CB - 1) / CB, PG = DW_THREADS / cbv;
  a.groups = (long)a.N * a.Hd * ((a.Wd + DW_TW - 1) / DW_TW);
  size_t lds = (size_t)((K * K * CB + 1) & ~1) * sizeof(float) + (STATS ? (size_t)2 * CB * sizeof(double) : 0);
  dim3 grid(grid_x(a.groups, PG, ny), (unsigned)ny);
  dwconv_kernel<T, V, K, S, MODE, STATS><<<grid, DW_THREADS, lds, st>>>(a);
  dy_note_kernel(name);
  DY_LAUNCH_CHECK();
  return 0;
}

// kind 0: forward epilogue, 1: forward statistics, 2: data gradient
template <typename T, int V, int K>
int launch_k(const DwArgs& a, int S, int kind, hipStream_t st) {
  if (kind == 1) return S == 1 ? launch_one<T, V, K, 1, 0, true>(a, st, "dwconv_kernel<fwd,stats>") : launch_one<T, V, K, 2, 0, true>(a, st, "dwconv_kernel<fwd,stats>");
  if (kind == 0) return S == 1 ? launch_one<T, V, K, 1, 0, false>(a, st, "dwconv_kernel<fwd>") : launch_one<T, V, K, 2, 0, false>(a, st, "dwconv_kernel<fwd>");
  return S == 1 ? launch_one<T, V, K, 1, 0, false>(a, st, "dwconv_kernel<dgrad>") : launch_one<T, V, K, 2, 1, false>(a, st, "dwconv_kernel<dgrad,s2>");
}

template <typename T, int V>
int launch_v(const DwArgs& a, int K, int S, int kind, hipStream_t st) {
  if (K == 3) return launch_k<T, V, 3>(a, S, kind, st);
  if (K == 5) return launch_k<T, V, 5>(a, S, kind, st);
  return launch_k<T, V, 7>(a, S, kind, st);
}

template <typename T>
int launch_conv(const DwArgs& a, int K, int S, int kind, int bytes, hipStream_t st) {
  constexpr int VE = DT<T>::VE;
  if (bytes == 16) return launch_v<T, VE>(a, K, S, kind, st);
  if (bytes == 8) return launch_v<T, VE / 2>(a, K, S, kind, st);
  return launch_v<T, 1>(a, K, S, kind, st);
}

template <typename T, int V, int K>
int launch_wg(const void* x, long x_ld, const void* dz, long dz_ld, float* dw, const DwGeom& g, float* scratch, long scratch_elems,
              hipStream_t st) {
  const int CV = (g.C + V - 1) / V;
  int cbv = pow2_ceil(CV);
  const int cap = DW_CHUNK / V < 64 ? DW_CHUNK / V : 64;
  if (cbv > cap) cbv = cap;
  const int CB = cbv * V, ny = (g.C + CB - 1) / CB, PG = DW_THREADS / cbv;
  const long groups = (long)g.N * g.Ho * ((g.Wo + DW_TW - 1) / DW_TW), E = (long)g.C * K * K;
  long nparts = (groups + (long)PG * 16 - 1) / ((long)PG * 16);      // >= 16 pixel groups per thread before the block reduction
  const long cap_parts = scratch_elems / E;
  if (nparts > 512) nparts = 512;
  if (nparts > cap_parts) nparts = cap_parts;
  DY_CHECK(nparts >= 1, "dy_dwconv_wgrad: scratch of %ld floats < one partial of %ld", scratch_elems, E);
  dim3 grid((unsigned)nparts, (unsigned)ny);
  if (g.S == 1)
    dwconv_wgrad_kernel<T, V, K, 1><<<grid, DW_THREADS, 0, st>>>((const T*)x, x_ld, (const T*)dz, dz_ld, scratch, g.N, g.H, g.W, g.Ho,
                                                                  g.Wo, g.C, cbv, groups);
  else
    dwconv_wgrad_kernel<T, V, K, 2><<<grid, DW_THREADS, 0, st>>>((const T*)x, x_ld, (const T*)dz, dz_ld, scratch, g.N, g.H, g.W, g.Ho,
                                                                  g.Wo, g.C, cbv, groups);
  DY_LAUNCH_CHECK();
  dy_note_kernel("dwconv_wgrad_kernel");
  return dy_sum_partials(scratch, (int)nparts, E, dw, st);
}

// the K*K*V partial sums of a thread stay in registers: V <= 8 for k = 3 (72), 4 for k = 5 (100), 2 for k = 7 (98)
template <typename T>
int launch_wgrad(const void* x, long x_ld, const void* dz, long dz_ld, float* dw, const DwGeom& g, int bytes, float* scratch,
                 long scratch_elems, hipStream_t st) {
  constexpr int VE = DT<T>::VE;
  const int vmax = bytes == 16 ? VE : (bytes == 8 ? VE / 2 : 1);
#define DW_WG(V_, K_) return launch_wg<T, V_, K_>(x, x_ld, dz, dz_ld, dw, g, scratch, scratch_elems, st)
  if (g.K == 3) {
    if (vmax == VE) DW_WG(VE, 3);
    if (vmax == VE / 2) DW_WG(VE / 2, 3);
    DW_WG(1, 3);
  }
  if (g.K == 5) {
    if (vmax >= 4) DW_WG(4, 5);
    if (vmax == 2) DW_WG(2, 5);
    DW_WG(1, 5);
  }
  if (vmax >= 2) DW_WG(2, 7);
  DW_WG(1, 7);
#undef DW_WG
}

}  // namespace

int dy_sum_partials(const float* part, int nparts, long E, float* out, hipStream_t stream) {
  sum_partials_kernel<<<(unsigned)((E + DW_THREADS - 1) / DW_THREADS), DW_THREADS, 0, stream>>>(part, out, E, nparts);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_dwconv_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, const float* w, int N, int H, int W, int C, int k,
                             int stride, const float* scale, const float* shift, int act, double* stats, int stats_c, int dtype,
                             void* stream) {
  DwGeom g{k, stride, N, H, W, 0, 0, C};
  if (int e = check_geom("dy_dwconv_fwd", g, dtype)) return e;
  if (int e = dy_check_lanes("dy_dwconv_fwd(x)", x, x_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_dwconv_fwd(y)", y, y_ld, C, dtype)) return e;
  DY_CHECK(w != nullptr, "dy_dwconv_fwd: null weight");
  DY_CHECK(!dy_views_overlap(x, x_ld, (long)N * H * W, C, y, y_ld,
                             (long)N * ((H + 2 * (k / 2) - k) / stride + 1) * ((W + 2 * (k / 2) - k) / stride + 1), C, dy_elem_size(dtype)),
           "dy_dwconv_fwd: the lanes of x and y overlap (in-place or misplaced slices)");
  DY_CHECK(act == DY_ACT_NONE || act == DY_ACT_SILU || act == DY_ACT_LEAKY, "dy_dwconv_fwd: bad act %d", act);
  DY_CHECK(stats == nullptr || (scale == nullptr && shift == nullptr && act == DY_ACT_NONE && stats_c >= C),
           "dy_dwconv_fwd: the statistics mode writes the raw output (no scale / shift / act) and needs stats_c >= C");
  const int es = dy_elem_size(dtype);
  int bytes = dy_view_bytes(x, x_ld, C, es);
  const int by = dy_view_bytes(y, y_ld, C, es);
  if (by < bytes) bytes = by;
  DwArgs a{};
  a.src = x, a.src_ld = x_ld, a.dst = y, a.dst_ld = y_ld, a.w = w;
  a.N = N, a.Hs = H, a.Ws = W, a.Hd = (H + 2 * (k / 2) - k) / stride + 1, a.Wd = (W + 2 * (k / 2) - k) / stride + 1, a.C = C;
  a.scale = scale, a.shift = shift, a.act = act, a.stats = stats, a.stats_c = stats_c;
  int r = 0;
  DY_DISPATCH_DTYPE("dy_dwconv_fwd", dtype, r = launch_conv<T>(a, k, stride, stats ? 1 : 0, bytes, (hipStream_t)stream));
  return r;
}

extern "C" int dy_dwconv_dgrad(const void* dz, int64_t dz_ld, void* dx, int64_t dx_ld, const float* w, int N, int H, int W, int C, int k,
                               int stride, int accumulate, const void* add_src, int64_t add_ld, int dtype, void* stream) {
  DwGeom g{k, stride, N, H, W, 0, 0, C};
  if (int e = check_geom("dy_dwconv_dgrad", g, dtype)) return e;
  if (int e = dy_check_lanes("dy_dwconv_dgrad(dz)", dz, dz_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_dwconv_dgrad(dx)", dx, dx_ld, C, dtype)) return e;
  if (add_src)
    if (int e = dy_check_lanes("dy_dwconv_dgrad(add_src)", add_src, add_ld, C, dtype)) return e;
  DY_CHECK(w != nullptr, "dy_dwconv_dgrad: null weight");
  DY_CHECK(!dy_views_overlap(dz, dz_ld, (long)N * ((H + 2 * (k / 2) - k) / stride + 1) * ((W + 2 * (k / 2) - k) / stride + 1), C, dx,
                             dx_ld, (long)N * H * W, C, dy_elem_size(dtype)),
           "dy_dwconv_dgrad: the lanes of dz and dx overlap (in-place or misplaced slices)");
  const int es = dy_elem_size(dtype);
  int bytes = dy_view_bytes(dz, dz_ld, C, es);
  const int b1 = dy_view_bytes(dx, dx_ld, C, es), b2 = add_src ? dy_view_bytes(add_src, add_ld, C, es) : 16;
  if (b1 < bytes) bytes = b1;
  if (b2 < bytes) bytes = b2;
  DwArgs a{};
  a.src = dz, a.src_ld = dz_ld, a.dst = dx, a.dst_ld = dx_ld, a.w = w;
  a.N = N, a.Hs = (H + 2 * (k / 2) - k) / stride + 1, a.Ws = (W + 2 * (k / 2) - k) / stride + 1, a.Hd = H, a.Wd = W, a.C = C;
  a.accumulate = accumulate ? 1 : 0;
  a.flip = stride == 1;                        // the stride-1 data gradient is the same convolution with the taps flipped
  a.add = add_src, a.add_ld = add_ld;
  int r = 0;
  DY_DISPATCH_DTYPE("dy_dwconv_dgrad", dtype, r = launch_conv<T>(a, k, stride, 2, bytes, (hipStream_t)stream));
  return r;
}

extern "C" int dy_dwconv_wgrad(const void* x, int64_t x_ld, const void* dz, int64_t dz_ld, float* dw, int N, int H, int W, int C, int k,
                               int stride, float* scratch, int64_t scratch_elems, int dtype, void* stream) {
  DwGeom g{k, stride, N, H, W, (H + 2 * (k / 2) - k) / stride + 1, (W + 2 * (k / 2) - k) / stride + 1, C};
  if (int e = check_geom("dy_dwconv_wgrad", g, dtype)) return e;
  if (int e = dy_check_lanes("dy_dwconv_wgrad(x)", x, x_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_dwconv_wgrad(dz)", dz, dz_ld, C, dtype)) return e;
  DY_CHECK(dw != nullptr && scratch != nullptr, "dy_dwconv_wgrad: null dw / scratch");
  const int es = dy_elem_size(dtype);
  int bytes = dy_view_bytes(x, x_ld, C, es);
  const int b1 = dy_view_bytes(dz, dz_ld, C, es);
  if (b1 < bytes) bytes = b1;
  int r = 0;
  DY_DISPATCH_DTYPE("dy_dwconv_wgrad", dtype, r = launch_wgrad<T>(x, x_ld, dz, dz_ld, dw, g, bytes, scratch, scratch_elems, (hipStream_t)stream));
  return r;
}

extern "C" int dy_copy2d_exact(const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int64_t pixels, int C, int accumulate,
                               int dtype, void* stream) {
  if (int e = dy_check_dtype("dy_copy2d_exact", dtype)) return e;
  DY_CHECK(pixels >= 0 && C >= 1, "dy_copy2d_exact: bad size");
  if (int e = dy_check_lanes("dy_copy2d_exact(src)", src, src_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_copy2d_exact(dst)", dst, dst_ld, C, dtype)) return e;
  if (pixels == 0) return 0;
  const long total = pixels * C;
  const int blocks = dy_ew_blocks(total, 4096);
  DY_DISPATCH_DTYPE("dy_copy2d_exact", dtype,
                    copy2d_exact_kernel<T><<<blocks, DW_THREADS, 0, (hipStream_t)stream>>>((const T*)src, src_ld, (T*)dst, dst_ld, total, C,
                                                                                         accumulate ? 1 : 0));
  dy_note_kernel("copy2d_exact_kernel");
  DY_LAUNCH_CHECK();
  return 0;
}
