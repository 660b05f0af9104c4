// Channel and spatial attention (CBAM), forward and backward, NHWC.  Replaces ChannelAttention.forward (reference
// ultralytics/nn/modules/conv.py:294-304 `x * self.act(self.fc(self.pool(x)))`), SpatialAttention.forward (conv.py:307-320
// `x * self.act(self.cv1(torch.cat([torch.mean(x, 1, keepdim=True), torch.max(x, 1, keepdim=True)[0]], 1)))`), CBAM.forward
// (conv.py:449-459) and their autograd.  The pool is dy_chan_pool_fwd below and the fc a 1x1 convolution; the other kernels take the fc's logits
// a [B, C] and do the rest:
//   g = sigmoid(a[b]), u = x g, m = (mean_c u, max_c u), s = sigmoid(conv_kxk(m)), y = u s            (u is never stored)
// All are bandwidth-bound: forward = pool (1 read) + stats (1 read) + gate (1 read, 1 write); backward = px (2 reads) + reduce (2 reads) + apply
// (1 read, 1 write); the per-pixel planes (mean, max, argmax, s, dpre, dmean, dmax; f32 / int32) are 1 / C of a pass each.
//
// Views: (pointer, pixel stride) with exactly the lanes [0, C) of every pixel touched.  16-byte accesses when every map view of
// the call is 16-byte aligned in pointer and pitch, element accesses otherwise (template flag VEC); C % 8 == 0 so a pixel is whole
// groups of VE elements either way.  One image per blockIdx.y / z: sigmoid(a[b]) is evaluated once per workgroup (LDS or
// registers), never per element.
//
// Lane mappings:
//   team  (stats, px): a pixel belongs to a team of TL lanes, TL = the smallest power of two >= C / VE, at most 64; lane l of the
//         team loads the groups l, l + TL, ... of the pixel and the team reduces with xor shuffles.  bf16 C = 64: 8 lanes a pixel,
//         8 pixels a wave load; C >= 512: one pixel a wave; every load instruction of a wave covers whole contiguous pixels.
//   owner (pool, chan gate, reduce, apply; bn2act.hip's): a thread owns one group of VE channels and walks pixels, so its gate values
//         and channel sums stay in registers.
//   tile  (gate forward, plane convolution backward): a workgroup owns a square tile of one image and keeps the tile plus a halo
//         of k / 2 pixels of the planes in LDS (zeros outside the image = the convolution's zero padding).
// Ties of the channel max go to the lowest channel index (torch.max on the CPU), the running max starts from -inf.
// Every sum over pixels is deterministic: per-workgroup partials over ranges fixed by the shape, a fixed-order second pass in f64,
// no atomics.
#include <limits.h>
#include <math.h>
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NT = 256;
constexpr int MAXC = DY_CBAM_MAX_C;
constexpr int MAX_PARTS = DY_CBAM_MAX_PARTS;
constexpr int RMAX = 3;                 // k <= 7
constexpr int GT = DY_CBAM_GATE_TILE;   // gate forward: GT x GT pixels per workgroup
constexpr int CT = DY_CBAM_CONV_TILE;   // plane convolution backward: CT x CT pixels per workgroup (one per thread)
static_assert(CT * CT == NT && GT * GT <= NT, "tile sizes");

template <typename T, bool VEC> __device__ inline void ldg(const T* p, float* out) {
  constexpr int VE = DT<T>::VE;
  if constexpr (VEC) {
    ldvec<T>(p, out);
  } else {
#pragma unroll
    for (int e = 0; e < VE; ++e) out[e] = DT<T>::ld(p + e);
  }
}
template <typename T, bool VEC> __device__ inline void stg(T* p, const float* in) {
  constexpr int VE = DT<T>::VE;
  if constexpr (VEC) {
    stvec<T>(p, in);
  } else {
#pragma unroll
    for (int e = 0; e < VE; ++e) DT<T>::st(p + e, in[e]);
  }
}

// gate[c] = sigmoid(a[b, c]) (1 without a gate) for the workgroup's image; the caller synchronises
template <typename T> __device__ inline void fill_gate(float* gate, const T* __restrict__ a, long a_ld, int b, int C) {
  for (int c = threadIdx.x; c < C; c += NT) gate[c] = a ? dy_sigmoid(DT<T>::ld(a + (long)b * a_ld + c)) : 1.f;
}

// ---- owner mapping ---------------------------------------------------------------------------------------------------------------
struct Geo { int cgb, rows; dim3 grid; };

// cgb channel groups x rows pixels per workgroup; gridDim.y covers the groups, gridDim.x <= MAX_PARTS walks the pixels of one image
// (at least 4 per thread where there are that many), gridDim.z = B.  A function of the shape alone: gridDim.x is the partial count.
Geo geometry(int B, int HW, int C, int ve) {
  Geo g;
  const int CG = C / ve;
  g.cgb = CG < NT ? CG : NT;
  g.rows = NT / g.cgb;
  const int gy = dy_cdiv(CG, g.cgb);
  long gx = ((long)HW + 4L * g.rows - 1) / (4L * g.rows);
  if (gx > MAX_PARTS) gx = MAX_PARTS;
  if (gx < 1) gx = 1;
  g.grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)B);
  return g;
}

struct Map { int c, first, step; bool active; };

template <int VE> __device__ inline Map make_map(int C, int cgb, int rows) {
  Map m;
  const int cg = blockIdx.y * cgb + threadIdx.x % cgb, prow = threadIdx.x / cgb;
  m.active = prow < rows && cg < C / VE;
  m.c = cg * VE;
  m.first = blockIdx.x * rows + prow;
  m.step = gridDim.x * rows;
  return m;
}

template <typename T, int VE> __device__ inline void owner_gate(const T* __restrict__ a, long a_ld, int b, int c, float* g) {
#pragma unroll
  for (int e = 0; e < VE; ++e) g[e] = a ? dy_sigmoid(DT<T>::ld(a + (long)b * a_ld + c + e)) : 1.f;
}

// y = x sigmoid(a[b])
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void chan_gate_fwd_kernel(const T* __restrict__ x, long x_ld, const T* __restrict__ a, long a_ld,
                                                           T* __restrict__ y, long y_ld, int HW, int C, int cgb, int rows) {
  constexpr int VE = DT<T>::VE;
  const Map m = make_map<VE>(C, cgb, rows);
  if (!m.active) return;
  const int b = blockIdx.z;
  float g[VE];
  owner_gate<T, VE>(a, a_ld, b, m.c, g);
  const long p0 = (long)b * HW;
  for (int p = m.first; p < HW; p += m.step) {
    float v[VE];
    ldg<T, VEC>(x + (p0 + p) * x_ld + m.c, v);
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] *= g[e];
    stg<T, VEC>(y + (p0 + p) * y_ld + m.c, v);
  }
}

// the planes of one pixel as the backward kernels read them (s == nullptr: no spatial stage, du = dy)
struct PxPlanes { float s, dmean_c, dmax; int arg; };
__device__ inline PxPlanes px_planes(const float* __restrict__ s, const float* __restrict__ dmean, const float* __restrict__ dmx,
                                     const int* __restrict__ arg, long q, float invC) {
  PxPlanes r;
  r.s = s[q];
  r.dmean_c = dmean[q] * invC;
  r.dmax = dmx[q];
  r.arg = arg[q];
  return r;
}
// du = dy s + dmean / C + (c == argmax ? dmax : 0)
__device__ inline float du_of(float dy, const PxPlanes& k, int c) { return dy * k.s + k.dmean_c + (c == k.arg ? k.dmax : 0.f); }

// The two sums over the pixels of an image, pass 1: part[b][blockIdx.x][C] = this workgroup's sum over its pixels of
//   POOL: x (the average pool in front of the fc; dy_gap_fwd walks an image's pixels in ONE thread per channel group, 6400 dependent
//         loads at 80 x 80, which suits Classify's 7 x 7 map: here the pixels are spread over gridDim.x workgroups of `rows` threads)
//   else: du x (the gate logits' gradient)
template <typename T, bool VEC, bool POOL>
__global__ __launch_bounds__(NT) void owner_reduce_kernel(const T* __restrict__ dy, long dy_ld, const T* __restrict__ x, long x_ld,
                                                          const float* __restrict__ s, const float* __restrict__ dmean,
                                                          const float* __restrict__ dmx, const int* __restrict__ arg,
                                                          float* __restrict__ part, int HW, int C, int cgb, int rows) {
  constexpr int VE = DT<T>::VE;
  __shared__ float join[NT * VE];                // [rows][cgb * VE]
  const int nch = cgb * VE, cl = (threadIdx.x % cgb) * VE, prow = threadIdx.x / cgb;
  const Map m = make_map<VE>(C, cgb, rows);
  const int b = blockIdx.z;
  if (m.active) {
    const long p0 = (long)b * HW;
    const float invC = 1.f / (float)C;
    float acc[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) acc[e] = 0.f;
    for (int p = m.first; p < HW; p += m.step) {
      float g[VE], v[VE];
      ldg<T, VEC>(x + (p0 + p) * x_ld + m.c, v);
      if constexpr (POOL) {
#pragma unroll
        for (int e = 0; e < VE; ++e) acc[e] += v[e];
      } else {
        ldg<T, VEC>(dy + (p0 + p) * dy_ld + m.c, g);
        if (s) {
          const PxPlanes k = px_planes(s, dmean, dmx, arg, p0 + p, invC);
#pragma unroll
          for (int e = 0; e < VE; ++e) g[e] = du_of(g[e], k, m.c + e);
        }
#pragma unroll
        for (int e = 0; e < VE; ++e) acc[e] += g[e] * v[e];
      }
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) join[prow * nch + cl + e] = acc[e];
  }
  __syncthreads();
  const int c0 = blockIdx.y * nch;
  float* dst = part + ((long)b * gridDim.x + blockIdx.x) * C;
  for (int ch = threadIdx.x; ch < nch; ch += NT) {
    if (c0 + ch < C) {
      float t = 0.f;
      for (int r = 0; r < rows; ++r) t += join[r * nch + ch];
      dst[c0 + ch] = t;
    }
  }
}

// pass 2: out[b, c] = k sum_j part[b][j][c], j in index order in f64, rounded once to T; k = g (1 - g) of the logit a[b, c] (the gate
// logits' gradient) or, without a, 1 / HW (the pool)
template <typename T>
__global__ __launch_bounds__(NT) void owner_final_kernel(const float* __restrict__ part, int parts, const T* __restrict__ a, long a_ld,
                                                         T* __restrict__ out, long out_ld, int B, int C, int HW) {
  const long i = (long)blockIdx.x * NT + threadIdx.x;
  if (i >= (long)B * C) return;
  const int b = (int)(i / C), c = (int)(i - (long)b * C);
  double t = 0.0;
  for (int j = 0; j < parts; ++j) t += (double)part[((long)b * parts + j) * C + c];
  if (a) {
    const float z = DT<T>::ld(a + (long)b * a_ld + c);
    t *= (double)(dy_sigmoid(z) * dy_sigmoid(-z));
  } else {
    t /= (double)HW;
  }
  DT<T>::st(out + (long)b * out_ld + c, (float)t);
}

// dx = du g + dpool[b] / HW (+ dx)
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void gate_bwd_apply_kernel(const T* __restrict__ dy, long dy_ld, const T* __restrict__ a, long a_ld,
                                                            const float* __restrict__ s, const float* __restrict__ dmean,
                                                            const float* __restrict__ dmx, const int* __restrict__ arg,
                                                            const T* __restrict__ dpool, long dpool_ld, T* __restrict__ dx, long dx_ld,
                                                            int accumulate, int HW, int C, int cgb, int rows) {
  constexpr int VE = DT<T>::VE;
  const Map m = make_map<VE>(C, cgb, rows);
  if (!m.active) return;
  const int b = blockIdx.z;
  float g[VE], pool[VE];
  owner_gate<T, VE>(a, a_ld, b, m.c, g);
#pragma unroll
  for (int e = 0; e < VE; ++e) pool[e] = dpool ? DT<T>::ld(dpool + (long)b * dpool_ld + m.c + e) / (float)HW : 0.f;
  const long p0 = (long)b * HW;
  const float invC = 1.f / (float)C;
  for (int p = m.first; p < HW; p += m.step) {
    float d[VE];
    ldg<T, VEC>(dy + (p0 + p) * dy_ld + m.c, d);
    if (s) {
      const PxPlanes k = px_planes(s, dmean, dmx, arg, p0 + p, invC);
#pragma unroll
      for (int e = 0; e < VE; ++e) d[e] = du_of(d[e], k, m.c + e);
    }
#pragma unroll
    for (int e = 0; e < VE; ++e) d[e] = d[e] * g[e] + pool[e];
    T* dst = dx + (p0 + p) * dx_ld + m.c;
    if (accumulate) {
      float o[VE];
      ldg<T, VEC>(dst, o);
#pragma unroll
      for (int e = 0; e < VE; ++e) d[e] += o[e];
    }
    stg<T, VEC>(dst, d);
  }
}

// ---- team mapping ----------------------------------------------------------------------------------------------------------------
static int team_lanes(int C, int ve) {
  int tl = 1;
  while (tl < C / ve && tl < 64) tl <<= 1;
  return tl;
}
static dim3 team_grid(int B, int HW, int tl) {
  const int nteam = NT / tl;
  long gx = ((long)HW + 4L * nteam - 1) / (4L * nteam);
  if (gx > 4096) gx = 4096;
  return dim3((unsigned)(gx < 1 ? 1 : gx), (unsigned)B);
}

// mean[q] = mean_c(x g), mx[q] = max_c(x g), arg[q] = the lowest channel that reaches the max (when arg != nullptr)
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void spatial_stats_kernel(const T* __restrict__ x, long x_ld, const T* __restrict__ a, long a_ld,
                                                           float* __restrict__ mean, float* __restrict__ mx, int* __restrict__ arg,
                                                           int HW, int C, int TL) {
  constexpr int VE = DT<T>::VE;
  __shared__ float gate[MAXC];
  const int b = blockIdx.y;
  fill_gate<T>(gate, a, a_ld, b, C);
  __syncthreads();
  const int G = C / VE, lt = threadIdx.x & (TL - 1), team = threadIdx.x / TL, nteam = NT / TL;
  const long p0 = (long)b * HW;
  for (int p = blockIdx.x * nteam + team; p < HW; p += gridDim.x * nteam) {      // the lanes of a team share p: they leave together
    float sum = 0.f, best = -INFINITY;
    int bi = INT_MAX;
    for (int gi = lt; gi < G; gi += TL) {
      float v[VE];
      ldg<T, VEC>(x + (p0 + p) * x_ld + gi * VE, v);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float u = v[e] * gate[gi * VE + e];
        sum += u;
        if (u > best) {                     // channels ascend inside a lane: strict > keeps the lowest index
          best = u;
          bi = gi * VE + e;
        }
      }
    }
    for (int o = TL >> 1; o > 0; o >>= 1) {
      sum += __shfl_xor(sum, o, 64);
      const float ob = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    if (lt == 0) {
      mean[p0 + p] = sum / (float)C;
      mx[p0 + p] = best;
      if (arg) arg[p0 + p] = bi;
    }
  }
}

// dpre[q] = s (1 - s) sum_c dy x g
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void spatial_gate_bwd_px_kernel(const T* __restrict__ dy, long dy_ld, const T* __restrict__ x, long x_ld,
                                                                 const T* __restrict__ a, long a_ld, const float* __restrict__ s,
                                                                 float* __restrict__ dpre, int HW, int C, int TL) {
  constexpr int VE = DT<T>::VE;
  __shared__ float gate[MAXC];
  const int b = blockIdx.y;
  fill_gate<T>(gate, a, a_ld, b, C);
  __syncthreads();
  const int G = C / VE, lt = threadIdx.x & (TL - 1), team = threadIdx.x / TL, nteam = NT / TL;
  const long p0 = (long)b * HW;
  for (int p = blockIdx.x * nteam + team; p < HW; p += gridDim.x * nteam) {
    float sum = 0.f;
    for (int gi = lt; gi < G; gi += TL) {
      float d[VE], v[VE];
      ldg<T, VEC>(dy + (p0 + p) * dy_ld + gi * VE, d);
      ldg<T, VEC>(x + (p0 + p) * x_ld + gi * VE, v);
#pragma unroll
      for (int e = 0; e < VE; ++e) sum += d[e] * (v[e] * gate[gi * VE + e]);
    }
    for (int o = TL >> 1; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lt == 0) {
      const float sv = s[p0 + p];
      dpre[p0 + p] = sum * (sv * (1.f - sv));
    }
  }
}

// ---- tile mapping ----------------------------------------------------------------------------------------------------------------
// halo[hy][hx] = plane[(ty0 + hy - r, tx0 + hx - r)] of one image, 0 outside it; hs = tile + 2 r entries a row
__device__ inline void fill_halo(float* halo, const float* __restrict__ plane, int ty0, int tx0, int r, int hs, int H, int W) {
  for (int i = threadIdx.x; i < hs * hs; i += NT) {
    const int hy = i / hs, hx = i - hy * hs, yy = ty0 + hy - r, xx = tx0 + hx - r;
    halo[i] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? plane[(long)yy * W + xx] : 0.f;
  }
}

// s = sigmoid(sum_{plane, i, j} w[plane][i][j] m[plane][(y + i - r, x + j - r)]), y = x g s
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void spatial_gate_fwd_kernel(const T* __restrict__ x, long x_ld, const T* __restrict__ a, long a_ld,
                                                              const float* __restrict__ mean, const float* __restrict__ mx,
                                                              const float* __restrict__ w, int k, T* __restrict__ y, long y_ld,
                                                              float* __restrict__ s_out, int H, int W, int C) {
  constexpr int VE = DT<T>::VE;
  constexpr int HS = GT + 2 * RMAX;
  __shared__ float gate[MAXC];
  __shared__ float halo[2][HS * HS];
  __shared__ float wt[2 * 49];
  __shared__ float sv[GT * GT];
  const int b = blockIdx.y, tiles_x = (W + GT - 1) / GT;
  const int ty0 = (blockIdx.x / tiles_x) * GT, tx0 = (blockIdx.x % tiles_x) * GT;
  const int r = k >> 1, hs = GT + 2 * r;
  const long p0 = (long)b * H * W;
  fill_gate<T>(gate, a, a_ld, b, C);
  fill_halo(halo[0], mean + p0, ty0, tx0, r, hs, H, W);
  fill_halo(halo[1], mx + p0, ty0, tx0, r, hs, H, W);
  for (int i = threadIdx.x; i < 2 * k * k; i += NT) wt[i] = w[i];
  __syncthreads();
  if (threadIdx.x < GT * GT) {
    const int ly = threadIdx.x / GT, lx = threadIdx.x % GT;
    float acc = 0.f;
    for (int pl = 0; pl < 2; ++pl)
      for (int i = 0; i < k; ++i)
        for (int j = 0; j < k; ++j) acc += wt[(pl * k + i) * k + j] * halo[pl][(ly + i) * hs + lx + j];
    const float sg = dy_sigmoid(acc);
    sv[threadIdx.x] = sg;
    if (s_out && ty0 + ly < H && tx0 + lx < W) s_out[p0 + (long)(ty0 + ly) * W + tx0 + lx] = sg;
  }
  __syncthreads();
  const int G = C / VE;
  for (int i = threadIdx.x; i < GT * GT * G; i += NT) {
    const int px = i / G, gi = i - px * G, yy = ty0 + px / GT, xx = tx0 + px % GT;
    if (yy >= H || xx >= W) continue;
    const long q = p0 + (long)yy * W + xx;
    float v[VE];
    ldg<T, VEC>(x + q * x_ld + gi * VE, v);
    const float sg = sv[px];
#pragma unroll
    for (int e = 0; e < VE; ++e) v[e] = v[e] * gate[gi * VE + e] * sg;
    stg<T, VEC>(y + q * y_ld + gi * VE, v);
  }
}

// planes only: (dmean, dmax)[q] = sum_{i, j} w[plane][i][j] dpre[q - (i - r, j - r)] (the transposed convolution: flipped taps, zero
// padding) and part[b][tile][plane][i][j] = sum over the tile's pixels q, in row-major order, of dpre[q] m[plane][q + (i - r, j - r)]
__global__ __launch_bounds__(NT) void spatial_conv_bwd_kernel(const float* __restrict__ dpre, const float* __restrict__ mean,
                                                              const float* __restrict__ mx, const float* __restrict__ w, int k,
                                                              float* __restrict__ dmean, float* __restrict__ dmx,
                                                              float* __restrict__ part, int H, int W) {
  constexpr int HS = CT + 2 * RMAX;
  __shared__ float dh[HS * HS];
  __shared__ float mh[2][HS * HS];
  __shared__ float wt[2 * 49];
  const int b = blockIdx.y, tiles_x = (W + CT - 1) / CT;
  const int ty0 = (blockIdx.x / tiles_x) * CT, tx0 = (blockIdx.x % tiles_x) * CT;
  const int r = k >> 1, hs = CT + 2 * r, kk = k * k;
  const long p0 = (long)b * H * W;
  fill_halo(dh, dpre + p0, ty0, tx0, r, hs, H, W);
  fill_halo(mh[0], mean + p0, ty0, tx0, r, hs, H, W);
  fill_halo(mh[1], mx + p0, ty0, tx0, r, hs, H, W);
  for (int i = threadIdx.x; i < 2 * kk; i += NT) wt[i] = w[i];
  __syncthreads();
  const int ly = threadIdx.x / CT, lx = threadIdx.x % CT;
  if (ty0 + ly < H && tx0 + lx < W) {
    float a0 = 0.f, a1 = 0.f;
    for (int i = 0; i < k; ++i)
      for (int j = 0; j < k; ++j) {
        const float d = dh[(ly + 2 * r - i) * hs + lx + 2 * r - j];
        a0 += wt[i * k + j] * d;
        a1 += wt[kk + i * k + j] * d;
      }
    const long q = p0 + (long)(ty0 + ly) * W + tx0 + lx;
    dmean[q] = a0;
    dmx[q] = a1;
  }
  if (threadIdx.x < 2 * kk) {
    const int pl = threadIdx.x / kk, t = threadIdx.x - pl * kk, i = t / k, j = t - i * k;
    float acc = 0.f;
    for (int py = 0; py < CT; ++py)                                   // pixels outside the image hold dpre = 0
      for (int px = 0; px < CT; ++px) acc += dh[(py + r) * hs + px + r] * mh[pl][(py + i) * hs + px + j];
    part[((long)b * gridDim.x + blockIdx.x) * 2 * kk + threadIdx.x] = acc;
  }
}

// dw[e] = sum_k part[k][e]: thread j adds the partials j, j + 256, ... in that order in f64, then a halving tree through LDS
__global__ __launch_bounds__(NT) void spatial_dw_final_kernel(const float* __restrict__ part, int parts, int E, float* __restrict__ dw) {
  __shared__ double sm[NT];
  const int e = blockIdx.x;
  double t = 0.0;
  for (int j = threadIdx.x; j < parts; j += NT) t += (double)part[(long)j * E + e];
  sm[threadIdx.x] = t;
  __syncthreads();
  for (int h = NT / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) sm[threadIdx.x] += sm[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) dw[e] = (float)sm[0];
}

// ---- launch helpers --------------------------------------------------------------------------------------------------------------
int check_shape(const char* who, int B, long HW, int C, int dtype) {
  if (int e = dy_check_dtype(who, dtype)) return e;
  DY_CHECK(C % 8 == 0 && C >= 8 && C <= MAXC, "%s: C=%d outside the rule C %% 8 == 0, 8 <= C <= %d", who, C, MAXC);
  DY_CHECK(B >= 1 && B <= 65535, "%s: B=%d outside 1 .. 65535", who, B);
  DY_CHECK(HW >= 1 && (double)B * (double)HW < 2147483647.0, "%s: B HW = %d x %ld outside 1 .. 2^31 - 1", who, B, HW);
  return 0;
}
int check_gate(const char* who, const void* a, long a_ld, int C, int dtype) {
  DY_CHECK(a == nullptr || (a_ld >= C && ((uintptr_t)a) % dy_elem_size(dtype) == 0), "%s: bad gate view (ld=%ld, C=%d)", who, a_ld, C);
  return 0;
}
int check_k(const char* who, int k) {
  DY_CHECK(k == 3 || k == 7, "%s: kernel size must be 3 or 7, got %d", who, k);
  return 0;
}

}  // namespace

// the statement sees the element type as T and the access width as the constant VEC
#define CBAM_LAUNCH(who, dtype, vec, ...)                              \
  DY_DISPATCH_DTYPE(who, dtype, if (vec) {                             \
    constexpr bool VEC = true;                                         \
    __VA_ARGS__;                                                       \
  } else {                                                             \
    constexpr bool VEC = false;                                        \
    __VA_ARGS__;                                                       \
  })

extern "C" int64_t dy_cbam_reduce_workspace(int B, int HW, int C, int dtype);

extern "C" int dy_chan_gate_fwd(const void* x, int64_t x_ld, const void* a, int64_t a_ld, void* y, int64_t y_ld, int B, int HW, int C,
                                int dtype, void* stream) {
  if (int e = check_shape("dy_chan_gate_fwd", B, HW, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_chan_gate_fwd(x)", x, x_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_chan_gate_fwd(y)", y, y_ld, C, dtype)) return e;
  DY_CHECK(a != nullptr, "dy_chan_gate_fwd: null gate");
  if (int e = check_gate("dy_chan_gate_fwd", a, a_ld, C, dtype)) return e;
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(x, x_ld, es) && dy_aligned16(y, y_ld, es);
  const Geo g = geometry(B, HW, C, dy_vec_elems(dtype));
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("chan_gate_fwd_kernel");
  CBAM_LAUNCH("dy_chan_gate_fwd", dtype, vec,
              chan_gate_fwd_kernel<T, VEC><<<g.grid, NT, 0, st>>>((const T*)x, x_ld, (const T*)a, a_ld, (T*)y, y_ld, HW, C, g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_chan_pool_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, float* workspace, int64_t workspace_elems, int B, int HW,
                               int C, int dtype, void* stream) {
  if (int e = check_shape("dy_chan_pool_fwd", B, HW, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_chan_pool_fwd(x)", x, x_ld, C, dtype)) return e;
  DY_CHECK(y != nullptr, "dy_chan_pool_fwd: null output");
  if (int e = check_gate("dy_chan_pool_fwd(y)", y, y_ld, C, dtype)) return e;
  const int64_t need = dy_cbam_reduce_workspace(B, HW, C, dtype);
  DY_CHECK(workspace && workspace_elems >= need, "dy_chan_pool_fwd: workspace of %ld floats needed, %ld given", (long)need,
           (long)workspace_elems);
  const bool vec = dy_aligned16(x, x_ld, dy_elem_size(dtype));
  const Geo g = geometry(B, HW, C, dy_vec_elems(dtype));
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("owner_reduce_kernel");
  CBAM_LAUNCH("dy_chan_pool_fwd", dtype, vec,
              owner_reduce_kernel<T, VEC, true><<<g.grid, NT, 0, st>>>(nullptr, 0, (const T*)x, x_ld, nullptr, nullptr, nullptr, nullptr, workspace,
                                                                       HW, C, g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  dy_note_kernel("owner_final_kernel");
  DY_DISPATCH_DTYPE("dy_chan_pool_fwd", dtype,
                    owner_final_kernel<T><<<dy_cdiv((long)B * C, NT), NT, 0, st>>>(workspace, (int)g.grid.x, nullptr, 0, (T*)y, y_ld, B, C, HW));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_spatial_stats_fwd(const void* x, int64_t x_ld, const void* a, int64_t a_ld, float* mean, float* mx, int32_t* arg, int B,
                                    int HW, int C, int dtype, void* stream) {
  if (int e = check_shape("dy_spatial_stats_fwd", B, HW, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_stats_fwd(x)", x, x_ld, C, dtype)) return e;
  if (int e = check_gate("dy_spatial_stats_fwd", a, a_ld, C, dtype)) return e;
  DY_CHECK(mean && mx, "dy_spatial_stats_fwd: null plane");
  const bool vec = dy_aligned16(x, x_ld, dy_elem_size(dtype));
  const int tl = team_lanes(C, dy_vec_elems(dtype));
  const dim3 grid = team_grid(B, HW, tl);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("spatial_stats_kernel");
  CBAM_LAUNCH("dy_spatial_stats_fwd", dtype, vec,
              spatial_stats_kernel<T, VEC><<<grid, NT, 0, st>>>((const T*)x, x_ld, (const T*)a, a_ld, mean, mx, arg, HW, C, tl));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_spatial_gate_fwd(const void* x, int64_t x_ld, const void* a, int64_t a_ld, const float* mean, const float* mx,
                                   const float* w, int k, void* y, int64_t y_ld, float* s, int B, int H, int W, int C, int dtype,
                                   void* stream) {
  DY_CHECK(H >= 1 && W >= 1, "dy_spatial_gate_fwd: H=%d W=%d", H, W);
  if (int e = check_shape("dy_spatial_gate_fwd", B, (long)H * W, C, dtype)) return e;
  if (int e = check_k("dy_spatial_gate_fwd", k)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_fwd(x)", x, x_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_fwd(y)", y, y_ld, C, dtype)) return e;
  if (int e = check_gate("dy_spatial_gate_fwd", a, a_ld, C, dtype)) return e;
  DY_CHECK(mean && mx && w, "dy_spatial_gate_fwd: null plane or weight");
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(x, x_ld, es) && dy_aligned16(y, y_ld, es);
  const dim3 grid((unsigned)(dy_cdiv(H, GT) * dy_cdiv(W, GT)), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("spatial_gate_fwd_kernel");
  CBAM_LAUNCH("dy_spatial_gate_fwd", dtype, vec,
              spatial_gate_fwd_kernel<T, VEC><<<grid, NT, 0, st>>>((const T*)x, x_ld, (const T*)a, a_ld, mean, mx, w, k, (T*)y, y_ld, s, H, W, C));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_spatial_gate_bwd_px(const void* dy, int64_t dy_ld, const void* x, int64_t x_ld, const void* a, int64_t a_ld, const float* s,
                                      float* dpre, int B, int HW, int C, int dtype, void* stream) {
  if (int e = check_shape("dy_spatial_gate_bwd_px", B, HW, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_bwd_px(dy)", dy, dy_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_bwd_px(x)", x, x_ld, C, dtype)) return e;
  if (int e = check_gate("dy_spatial_gate_bwd_px", a, a_ld, C, dtype)) return e;
  DY_CHECK(s && dpre, "dy_spatial_gate_bwd_px: null plane");
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(dy, dy_ld, es) && dy_aligned16(x, x_ld, es);
  const int tl = team_lanes(C, dy_vec_elems(dtype));
  const dim3 grid = team_grid(B, HW, tl);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("spatial_gate_bwd_px_kernel");
  CBAM_LAUNCH("dy_spatial_gate_bwd_px", dtype, vec,
              spatial_gate_bwd_px_kernel<T, VEC><<<grid, NT, 0, st>>>((const T*)dy, dy_ld, (const T*)x, x_ld, (const T*)a, a_ld, s, dpre, HW, C, tl));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t dy_spatial_conv_bwd_workspace(int B, int H, int W, int k) {
  if (B < 1 || H < 1 || W < 1 || (k != 3 && k != 7)) return 0;
  return (int64_t)B * dy_cdiv(H, CT) * dy_cdiv(W, CT) * 2 * k * k;
}

extern "C" int dy_spatial_conv_bwd(const float* dpre, const float* mean, const float* mx, const float* w, int k, float* dmean, float* dmx,
                                   float* dw, float* workspace, int64_t workspace_elems, int B, int H, int W, void* stream) {
  DY_CHECK(H >= 1 && W >= 1, "dy_spatial_conv_bwd: H=%d W=%d", H, W);
  if (int e = check_shape("dy_spatial_conv_bwd", B, (long)H * W, 8, DY_F32)) return e;
  if (int e = check_k("dy_spatial_conv_bwd", k)) return e;
  DY_CHECK(dpre && mean && mx && w && dmean && dmx && dw, "dy_spatial_conv_bwd: null plane, weight or gradient");
  const int64_t need = dy_spatial_conv_bwd_workspace(B, H, W, k);
  DY_CHECK(workspace && workspace_elems >= need, "dy_spatial_conv_bwd: workspace of %ld floats needed, %ld given", (long)need,
           (long)workspace_elems);
  const int tiles = dy_cdiv(H, CT) * dy_cdiv(W, CT);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("spatial_conv_bwd_kernel");
  spatial_conv_bwd_kernel<<<dim3((unsigned)tiles, (unsigned)B), NT, 0, st>>>(dpre, mean, mx, w, k, dmean, dmx, workspace, H, W);
  DY_LAUNCH_CHECK();
  dy_note_kernel("spatial_dw_final_kernel");
  spatial_dw_final_kernel<<<2 * k * k, NT, 0, st>>>(workspace, B * tiles, 2 * k * k, dw);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t dy_cbam_reduce_workspace(int B, int HW, int C, int dtype) {
  if (B < 1 || HW < 1 || C < 8 || C % 8 || C > MAXC || (dtype != DY_F32 && dtype != DY_BF16 && dtype != DY_F16)) return 0;
  return (int64_t)B * geometry(B, HW, C, dy_vec_elems(dtype)).grid.x * C;
}

extern "C" int dy_spatial_gate_bwd_reduce(const void* dy, int64_t dy_ld, const void* x, int64_t x_ld, const void* a, int64_t a_ld,
                                          const float* s, const float* dmean, const float* dmx, const int32_t* arg, void* da, int64_t da_ld,
                                          float* workspace, int64_t workspace_elems, int B, int HW, int C, int dtype, void* stream) {
  if (int e = check_shape("dy_spatial_gate_bwd_reduce", B, HW, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_bwd_reduce(dy)", dy, dy_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_bwd_reduce(x)", x, x_ld, C, dtype)) return e;
  DY_CHECK(a != nullptr && da != nullptr, "dy_spatial_gate_bwd_reduce: null gate or gate gradient");
  if (int e = check_gate("dy_spatial_gate_bwd_reduce(a)", a, a_ld, C, dtype)) return e;
  if (int e = check_gate("dy_spatial_gate_bwd_reduce(da)", da, da_ld, C, dtype)) return e;
  DY_CHECK(s == nullptr || (dmean && dmx && arg), "dy_spatial_gate_bwd_reduce: s without dmean / dmax / argmax");
  const int64_t need = dy_cbam_reduce_workspace(B, HW, C, dtype);
  DY_CHECK(workspace && workspace_elems >= need, "dy_spatial_gate_bwd_reduce: workspace of %ld floats needed, %ld given", (long)need,
           (long)workspace_elems);
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(dy, dy_ld, es) && dy_aligned16(x, x_ld, es);
  const Geo g = geometry(B, HW, C, dy_vec_elems(dtype));
  const int parts = (int)g.grid.x;
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("owner_reduce_kernel");
  CBAM_LAUNCH("dy_spatial_gate_bwd_reduce", dtype, vec,
              owner_reduce_kernel<T, VEC, false><<<g.grid, NT, 0, st>>>((const T*)dy, dy_ld, (const T*)x, x_ld, s, dmean, dmx, arg, workspace, HW, C,
                                                                    g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  dy_note_kernel("owner_final_kernel");
  DY_DISPATCH_DTYPE("dy_spatial_gate_bwd_reduce", dtype,
                    owner_final_kernel<T><<<dy_cdiv((long)B * C, NT), NT, 0, st>>>(workspace, parts, (const T*)a, a_ld, (T*)da, da_ld, B, C, HW));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_spatial_gate_bwd_apply(const void* dy, int64_t dy_ld, const void* a, int64_t a_ld, const float* s, const float* dmean,
                                         const float* dmx, const int32_t* arg, const void* dpool, int64_t dpool_ld, void* dx, int64_t dx_ld,
                                         int accumulate, int B, int HW, int C, int dtype, void* stream) {
  if (int e = check_shape("dy_spatial_gate_bwd_apply", B, HW, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_bwd_apply(dy)", dy, dy_ld, C, dtype)) return e;
  if (int e = dy_check_lanes("dy_spatial_gate_bwd_apply(dx)", dx, dx_ld, C, dtype)) return e;
  if (int e = check_gate("dy_spatial_gate_bwd_apply(a)", a, a_ld, C, dtype)) return e;
  if (int e = check_gate("dy_spatial_gate_bwd_apply(dpool)", dpool, dpool_ld, C, dtype)) return e;
  DY_CHECK(s == nullptr || (dmean && dmx && arg), "dy_spatial_gate_bwd_apply: s without dmean / dmax / argmax");
  const int es = dy_elem_size(dtype);
  const bool vec = dy_aligned16(dy, dy_ld, es) && dy_aligned16(dx, dx_ld, es);
  const Geo g = geometry(B, HW, C, dy_vec_elems(dtype));
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("gate_bwd_apply_kernel");
  CBAM_LAUNCH("dy_spatial_gate_bwd_apply", dtype, vec,
              gate_bwd_apply_kernel<T, VEC><<<g.grid, NT, 0, st>>>((const T*)dy, dy_ld, (const T*)a, a_ld, s, dmean, dmx, arg, (const T*)dpool,
                                                                   dpool_ld, (T*)dx, dx_ld, accumulate, HW, C, g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  return 0;
}
