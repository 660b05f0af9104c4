// BatchNorm + activation over the SUM of two raw convolution outputs, forward and backward, NHWC, 16 B per lane:
//   y = act(u scale_u + shift_u + v scale_v + shift_v)
// Replaces RepConv.forward of the reference (ultralytics/nn/modules/conv.py:215-218 `self.act(self.conv1(x) + self.conv2(x))`,
// conv1 / conv2 = Conv(act=False), conv.py:208-209): two BatchNorm2d with separate batch statistics, one add, one SiLU, and
// their autograd.  scale / shift / mean / invstd of each branch come from dy_bn_finalize_valid (training) or
// dy_bn_fold_eval_valid (eval); these kernels take no statistics themselves.  All are HBM-bound streaming kernels: forward
// 2 reads + 1 write, backward 3 reads for the sums and 3 reads + 2 writes for the apply.
//
// Thread mapping (bnact.hip's): a thread owns ONE 16-byte channel group for its whole life, so the per-channel constants sit
// in registers, and walks pixels with a grid stride; a workgroup is `rows` pixels by `cgb` channel groups.
// The backward sums are deterministic: the grid is fixed by (pixels, C, dtype), a thread adds its pixels in order, the
// `rows` threads of a channel are joined through LDS in row order, every workgroup stores its three sums per channel as a
// partial, and a second kernel adds the partials in an order fixed by their count (in f64).  No atomics; two runs give identical bytes.
#include <type_traits>
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_PARTS = DY_BN2_MAX_PARTS;

template <typename F> __device__ inline void with_act(int act, F&& f) {
  if (act == DY_ACT_SILU) f(std::integral_constant<int, DY_ACT_SILU>{});
  else if (act == DY_ACT_LEAKY) f(std::integral_constant<int, DY_ACT_LEAKY>{});
  else f(std::integral_constant<int, DY_ACT_NONE>{});
}

struct Geo { int cgb, rows; dim3 grid; };

// cgb channel groups x rows pixels per workgroup; gridDim.y covers the channel groups, gridDim.x <= MAX_PARTS walks the pixels
// (at least 4 per thread where there are that many).  Depends on the shape alone: the backward's partial count is gridDim.x.
Geo geometry(long pixels, int C, int ve) {
  Geo g;
  const int CG = C / ve;
  g.cgb = CG < NT ? CG : NT;
  g.rows = NT / g.cgb;
  const int gy = dy_cdiv(CG, g.cgb);
  long gx = (pixels + 4L * g.rows - 1) / (4L * g.rows);
  const long most = MAX_PARTS / gy > 1 ? MAX_PARTS / gy : 1;
  if (gx > most) gx = most;
  if (gx < 1) gx = 1;
  g.grid = dim3((unsigned)gx, (unsigned)gy);
  return g;
}

struct Map {           // thread -> (first channel of its group, first pixel, pixel stride)
  int c;
  long first, step;
  bool active;
};

template <int VE> __device__ inline Map make_map(int C, int cgb, int rows) {
  Map m;
  const int cg = blockIdx.y * cgb + threadIdx.x % cgb, prow = threadIdx.x / cgb;
  m.active = prow < rows && cg < C / VE;
  m.c = cg * VE;
  m.first = (long)blockIdx.x * rows + prow;
  m.step = (long)gridDim.x * rows;
  return m;
}

// VE per-channel constants of a thread (element loads: gamma may be a view at any 4-byte offset of a flat parameter buffer)
template <int VE> __device__ inline void ld_const(const float* __restrict__ p, int c, float* out) {
#pragma unroll
  for (int e = 0; e < VE; ++e) out[e] = p[c + e];
}

template <typename T>
__global__ __launch_bounds__(NT) void bn2_act_fwd_kernel(const T* __restrict__ u, long u_ld, const T* __restrict__ v, long v_ld,
                                                         const float* __restrict__ scale_u, const float* __restrict__ shift_u,
                                                         const float* __restrict__ scale_v, const float* __restrict__ shift_v, int act,
                                                         T* __restrict__ y, long y_ld, long pixels, int C, int cgb, int rows) {
  constexpr int VE = DT<T>::VE;
  const Map m = make_map<VE>(C, cgb, rows);
  if (!m.active) return;
  float su[VE], sv[VE], sh[VE], t[VE];
  ld_const<VE>(scale_u, m.c, su);
  ld_const<VE>(scale_v, m.c, sv);
  ld_const<VE>(shift_u, m.c, sh);
  ld_const<VE>(shift_v, m.c, t);
#pragma unroll
  for (int e = 0; e < VE; ++e) sh[e] += t[e];
  with_act(act, [&](auto actc) {
    constexpr int ACT = decltype(actc)::value;
    for (long p0 = m.first; p0 < pixels; p0 += 2 * m.step) {
      float a[2][VE], b[2][VE];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const long p = p0 + k * m.step;
        if (p < pixels) {
          ldvec<T>(u + p * u_ld + m.c, a[k]);
          ldvec<T>(v + p * v_ld + m.c, b[k]);
        }
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const long p = p0 + k * m.step;
        if (p < pixels) {
#pragma unroll
          for (int e = 0; e < VE; ++e) a[k][e] = dy_act(ACT, a[k][e] * su[e] + b[k][e] * sv[e] + sh[e]);
          stvec<T>(y + p * y_ld + m.c, a[k]);
        }
      }
    }
  });
}

// backward pass 1: part[blockIdx.x][3][C] = this workgroup's sums of g, g u^ and g v^ over its pixels, g = dy act'(z)
template <typename T>
__global__ __launch_bounds__(NT) void bn2_act_bwd_reduce_kernel(const T* __restrict__ dy, long dy_ld, const T* __restrict__ u, long u_ld,
                                                                const T* __restrict__ v, long v_ld, const float* __restrict__ scale_u,
                                                                const float* __restrict__ shift_u, const float* __restrict__ mean_u,
                                                                const float* __restrict__ invstd_u, const float* __restrict__ scale_v,
                                                                const float* __restrict__ shift_v, const float* __restrict__ mean_v,
                                                                const float* __restrict__ invstd_v, int act, float* __restrict__ part,
                                                                long pixels, int C, int cgb, int rows) {
  constexpr int VE = DT<T>::VE;
  __shared__ float join[3 * NT * VE];          // [3][rows][cgb * VE]
  const int nch = cgb * VE, cl = (threadIdx.x % cgb) * VE, prow = threadIdx.x / cgb;
  const Map m = make_map<VE>(C, cgb, rows);
  if (m.active) {
    float su[VE], sv[VE], sh[VE], mu[VE], iu[VE], mv[VE], iv[VE], s0[VE], s1[VE], s2[VE];
    ld_const<VE>(scale_u, m.c, su);
    ld_const<VE>(scale_v, m.c, sv);
    ld_const<VE>(shift_u, m.c, sh);
    ld_const<VE>(shift_v, m.c, s0);
    ld_const<VE>(mean_u, m.c, mu);
    ld_const<VE>(invstd_u, m.c, iu);
    ld_const<VE>(mean_v, m.c, mv);
    ld_const<VE>(invstd_v, m.c, iv);
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      sh[e] += s0[e];
      s0[e] = s1[e] = s2[e] = 0.f;
    }
    with_act(act, [&](auto actc) {
      constexpr int ACT = decltype(actc)::value;
      for (long p = m.first; p < pixels; p += m.step) {
        float g[VE], a[VE], b[VE];
        ldvec<T>(dy + p * dy_ld + m.c, g);
        ldvec<T>(u + p * u_ld + m.c, a);
        ldvec<T>(v + p * v_ld + m.c, b);
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          const float ge = g[e] * dy_dact(ACT, a[e] * su[e] + b[e] * sv[e] + sh[e]);
          s0[e] += ge;
          s1[e] += ge * ((a[e] - mu[e]) * iu[e]);
          s2[e] += ge * ((b[e] - mv[e]) * iv[e]);
        }
      }
    });
    float* mine = join + prow * nch + cl;
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      mine[e] = s0[e];
      mine[rows * nch + e] = s1[e];
      mine[2 * rows * nch + e] = s2[e];
    }
  }
  __syncthreads();
  const int c0 = blockIdx.y * nch;
  float* dst = part + (long)blockIdx.x * 3 * C;
  for (int i = threadIdx.x; i < 3 * nch; i += NT) {
    const int which = i / nch, ch = i - which * nch;
    if (c0 + ch < C) {
      const float* col = join + which * rows * nch + ch;
      float acc = 0.f;
      for (int r = 0; r < rows; ++r) acc += col[r * nch];
      dst[which * C + c0 + ch] = acc;
    }
  }
}

// backward pass 2: sums[3][C] = the partials added in a fixed order: a workgroup owns 4 of the 3 C columns (C % 4 == 0), thread
// (column, group g) adds the partials g, g + 64, g + 128, ... in that order in f64, and the 64 group sums are folded by a halving
// tree through LDS whose shape does not depend on the data; the parameter gradients are these sums.  (16 columns x 16 groups, the
// layout of layernorm.hip's second kernel, left 24 workgroups walking 64 partials each at C = 128: 16 us, as long as pass 1.)
__global__ __launch_bounds__(NT) void bn2_act_bwd_final_kernel(const float* __restrict__ part, int parts, int C, float* __restrict__ sums,
                                                               float* dgamma_u, float* dbeta_u, float* dgamma_v, float* dbeta_v) {
  __shared__ double sm[64][4];
  const int col = threadIdx.x & 3, grp = threadIdx.x >> 2;
  const int i = blockIdx.x * 4 + col;                               // < 3 C: the grid is 3 C / 4 workgroups
  double t = 0.0;
#pragma unroll 4
  for (int j = grp; j < parts; j += 64) t += (double)part[(long)j * 3 * C + i];
  sm[grp][col] = t;
  __syncthreads();
  for (int h = 32; h > 0; h >>= 1) {
    if (grp < h) sm[grp][col] += sm[grp + h][col];
    __syncthreads();
  }
  if (grp != 0) return;
  t = sm[0][col];
  const float s = (float)t;
  sums[i] = s;
  const int which = i / C, c = i - which * C;
  if (which == 0) {
    if (dbeta_u) dbeta_u[c] = s;
    if (dbeta_v) dbeta_v[c] = s;
  } else if (which == 1) {
    if (dgamma_u) dgamma_u[c] = s;
  } else if (dgamma_v) dgamma_v[c] = s;
}

// backward pass 3: du = k_u (g - S0 / M - u^ S1 / M), k_u = gamma_u invstd_u; dv likewise with S2
template <typename T>
__global__ __launch_bounds__(NT) void bn2_act_bwd_apply_kernel(const T* __restrict__ dy, long dy_ld, const T* __restrict__ u, long u_ld,
                                                               const T* __restrict__ v, long v_ld, const float* __restrict__ scale_u,
                                                               const float* __restrict__ shift_u, const float* __restrict__ mean_u,
                                                               const float* __restrict__ invstd_u, const float* __restrict__ gamma_u,
                                                               const float* __restrict__ scale_v, const float* __restrict__ shift_v,
                                                               const float* __restrict__ mean_v, const float* __restrict__ invstd_v,
                                                               const float* __restrict__ gamma_v, int act, const float* __restrict__ sums,
                                                               T* __restrict__ du, long du_ld, T* __restrict__ dv, long dv_ld, long pixels,
                                                               int C, int cgb, int rows) {
  constexpr int VE = DT<T>::VE;
  const Map m = make_map<VE>(C, cgb, rows);
  if (!m.active) return;
  const float invM = 1.f / (float)pixels;
  float su[VE], sv[VE], sh[VE], mu[VE], iu[VE], mv[VE], iv[VE], ku[VE], kv[VE], m0[VE], m1[VE], m2[VE];
  ld_const<VE>(scale_u, m.c, su);
  ld_const<VE>(scale_v, m.c, sv);
  ld_const<VE>(shift_u, m.c, sh);
  ld_const<VE>(shift_v, m.c, m0);
  ld_const<VE>(mean_u, m.c, mu);
  ld_const<VE>(invstd_u, m.c, iu);
  ld_const<VE>(mean_v, m.c, mv);
  ld_const<VE>(invstd_v, m.c, iv);
  ld_const<VE>(gamma_u, m.c, ku);
  ld_const<VE>(gamma_v, m.c, kv);
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    sh[e] += m0[e];
    ku[e] *= iu[e];
    kv[e] *= iv[e];
  }
  ld_const<VE>(sums, m.c, m0);
  ld_const<VE>(sums + C, m.c, m1);
  ld_const<VE>(sums + 2 * C, m.c, m2);
#pragma unroll
  for (int e = 0; e < VE; ++e) {
    m0[e] *= invM;
    m1[e] *= invM;
    m2[e] *= invM;
  }
  with_act(act, [&](auto actc) {
    constexpr int ACT = decltype(actc)::value;
    for (long p = m.first; p < pixels; p += m.step) {
      float g[VE], a[VE], b[VE];
      ldvec<T>(dy + p * dy_ld + m.c, g);
      ldvec<T>(u + p * u_ld + m.c, a);
      ldvec<T>(v + p * v_ld + m.c, b);
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const float ge = g[e] * dy_dact(ACT, a[e] * su[e] + b[e] * sv[e] + sh[e]) - m0[e];
        a[e] = ku[e] * (ge - (a[e] - mu[e]) * iu[e] * m1[e]);
        b[e] = kv[e] * (ge - (b[e] - mv[e]) * iv[e] * m2[e]);
      }
      stvec<T>(du + p * du_ld + m.c, a);
      stvec<T>(dv + p * dv_ld + m.c, b);
    }
  });
}

}  // namespace

extern "C" int dy_bn2_act_fwd(const void* u, int64_t u_ld, const void* v, int64_t v_ld, const float* scale_u, const float* shift_u,
                              const float* scale_v, const float* shift_v, int act, void* y, int64_t y_ld, int64_t pixels, int C,
                              int dtype, void* stream) {
  if (int e = dy_check_view("dy_bn2_act_fwd(u)", u, u_ld, C, dtype)) return e;
  if (int e = dy_check_view("dy_bn2_act_fwd(v)", v, v_ld, C, dtype)) return e;
  if (int e = dy_check_view("dy_bn2_act_fwd(y)", y, y_ld, C, dtype)) return e;
  DY_CHECK(scale_u && shift_u && scale_v && shift_v, "dy_bn2_act_fwd: null scale / shift");
  DY_CHECK(act == DY_ACT_NONE || act == DY_ACT_SILU || act == DY_ACT_LEAKY, "dy_bn2_act_fwd: bad activation %d", act);
  if (pixels <= 0) return 0;
  const Geo g = geometry(pixels, C, dy_vec_elems(dtype));
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("bn2_act_fwd_kernel");
  DY_DISPATCH_DTYPE("dy_bn2_act_fwd", dtype,
                    bn2_act_fwd_kernel<T><<<g.grid, NT, 0, st>>>((const T*)u, u_ld, (const T*)v, v_ld, scale_u, shift_u, scale_v, shift_v, act,
                                                                 (T*)y, y_ld, pixels, C, g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int64_t dy_bn2_act_bwd_workspace(int64_t pixels, int C, int dtype) {
  if (pixels <= 0 || C <= 0 || (dtype != DY_F32 && dtype != DY_BF16 && dtype != DY_F16) || C % dy_vec_elems(dtype)) return 0;
  const Geo g = geometry(pixels, C, dy_vec_elems(dtype));
  return 3L * C * ((long)g.grid.x + 1);
}

extern "C" int dy_bn2_act_bwd(const void* dy, int64_t dy_ld, const void* u, int64_t u_ld, const void* v, int64_t v_ld,
                              const float* scale_u, const float* shift_u, const float* mean_u, const float* invstd_u,
                              const float* gamma_u, const float* scale_v, const float* shift_v, const float* mean_v,
                              const float* invstd_v, const float* gamma_v, int act, void* du, int64_t du_ld, void* dv, int64_t dv_ld,
                              float* dgamma_u, float* dbeta_u, float* dgamma_v, float* dbeta_v, float* workspace,
                              int64_t workspace_elems, int64_t pixels, int C, int dtype, void* stream) {
  if (int e = dy_check_view("dy_bn2_act_bwd(dy)", dy, dy_ld, C, dtype)) return e;
  if (int e = dy_check_view("dy_bn2_act_bwd(u)", u, u_ld, C, dtype)) return e;
  if (int e = dy_check_view("dy_bn2_act_bwd(v)", v, v_ld, C, dtype)) return e;
  if (int e = dy_check_view("dy_bn2_act_bwd(du)", du, du_ld, C, dtype)) return e;
  if (int e = dy_check_view("dy_bn2_act_bwd(dv)", dv, dv_ld, C, dtype)) return e;
  DY_CHECK(scale_u && shift_u && mean_u && invstd_u && gamma_u && scale_v && shift_v && mean_v && invstd_v && gamma_v,
           "dy_bn2_act_bwd: null per-channel vector");
  DY_CHECK(act == DY_ACT_NONE || act == DY_ACT_SILU || act == DY_ACT_LEAKY, "dy_bn2_act_bwd: bad activation %d", act);
  DY_CHECK(pixels >= 1, "dy_bn2_act_bwd: pixels=%ld", (long)pixels);
  const int64_t need = dy_bn2_act_bwd_workspace(pixels, C, dtype);
  DY_CHECK(workspace && workspace_elems >= need && ((uintptr_t)workspace) % 16 == 0,
           "dy_bn2_act_bwd: workspace of %ld floats (16-byte aligned) needed, %ld given", (long)need, (long)workspace_elems);
  const Geo g = geometry(pixels, C, dy_vec_elems(dtype));
  const int parts = (int)g.grid.x;
  float* sums = workspace;                     // [3][C], then the partials [parts][3][C]
  float* part = workspace + 3L * C;
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("bn2_act_bwd_reduce_kernel");
  DY_DISPATCH_DTYPE("dy_bn2_act_bwd", dtype,
                    bn2_act_bwd_reduce_kernel<T><<<g.grid, NT, 0, st>>>((const T*)dy, dy_ld, (const T*)u, u_ld, (const T*)v, v_ld, scale_u, shift_u,
                                                                        mean_u, invstd_u, scale_v, shift_v, mean_v, invstd_v, act, part,
                                                                        pixels, C, g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  dy_note_kernel("bn2_act_bwd_final_kernel");
  bn2_act_bwd_final_kernel<<<3 * C / 4, NT, 0, st>>>(part, parts, C, sums, dgamma_u, dbeta_u, dgamma_v, dbeta_v);
  DY_LAUNCH_CHECK();
  dy_note_kernel("bn2_act_bwd_apply_kernel");
  DY_DISPATCH_DTYPE("dy_bn2_act_bwd", dtype,
                    bn2_act_bwd_apply_kernel<T><<<g.grid, NT, 0, st>>>((const T*)dy, dy_ld, (const T*)u, u_ld, (const T*)v, v_ld, scale_u, shift_u,
                                                                       mean_u, invstd_u, gamma_u, scale_v, shift_v, mean_v, invstd_v, gamma_v,
                                                                       act, sums, (T*)du, du_ld, (T*)dv, dv_ld, pixels, C, g.cgb, g.rows));
  DY_LAUNCH_CHECK();
  return 0;
}
