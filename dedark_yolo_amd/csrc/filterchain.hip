// Front-end filter chains: the pointwise part of an arbitrary chain of the reference's filters (the list `cfg.filters` of
// ultralytics/nn/modules/filter_cfg.py:17-75, applied in order by llie.py:51-52) and the ToneFilter the default chain lacks
// (filtersB.py:262-286).  frontend.hip keeps the fused pair of the default chain DeDark -> WB -> Gamma -> Contrast; this file
// runs any order of DeDark / WB / Gamma / Tone / Contrast (each at most once, UsmFilter stays with usm.hip) in ONE pass:
// 1 read + 1 write of the image whatever the chain length, as the fused pair.
//
// Same design as pointwise_fwd/bwd_kernel: one WAVE per (b, c, row), four rows per block, wave shuffles for the row sums, the
// block meets in LDS only to merge its rows' parameter gradients into one set of f64 atomics.  The stage loop is a wave-uniform
// switch over 4-bit codes passed by value; every filter occurs at most once, so the values the backward needs are fields named
// by filter, not an array indexed by stage at run time (which would live in scratch).
//
// Contrast quirk (filtersB.py:299-303, util_filters.py:270-273): the luminance is a per-(b, c, row) scalar from pixel columns
// 0, 1, 2 of the contrast filter's INPUT, i.e. of whatever stages precede it in this chain: lanes 0..2 run that prefix first.
// The row gain K multiplies the row and the stages after Contrast act on the multiplied values.  Backward recomputes the forward
// per pixel, walks the stages in reverse (suffix adjoint -> dK and d(sK), prefix adjoint of d(sK) * K) and afterwards gives the
// three luminance pixels their extra term d lum, as pointwise_bwd_kernel does.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int FC_ROWS = 4;
constexpr int FC_PX = 2;                // pixels per lane and stage dispatch, forward
constexpr int FC_PX_BWD = 2;            // backward
constexpr int FC_NACC = 12;             // omega, wb, gamma, alpha, tone[8]
constexpr float LN2 = 0.69314718055994530942f;
constexpr float PI_F = 3.14159265358979323846f;

__host__ __device__ inline int fc_code(unsigned chain, int k) { return (int)((chain >> (4 * k)) & 15u); }

// per-(image, channel) constants of a row
struct RowCtx {
  float omega, s, gamma, alpha, A;
  float t[DY_TONE_STEPS];
  float Tsum, T8;                       // sum t_i + 1e-30 and 8 / Tsum
  float K;                              // contrast row gain (1 until the luminance is known)
};

// What the adjoint of a pixel needs from its forward, by field.  Two homes: registers (RegState: the forward kernel and the per-row
// luminance lanes, where the compiler drops what nobody reads) and LDS (LdsState: the backward's pixel loop).  In registers the
// fields are loop-carried through both stage loops, and every trip of a dispatch loop copies the fields its case did not touch;
// a field in LDS is written by the one case that owns it and read by its adjoint, [field][thread] so that a wave's accesses are
// consecutive words.
enum { IN_DF, IN_W, IN_G, IN_T, IN_CT, TXR, RTX, BASE, LOG2B, OUT_G, OUT_T, PX_FIELDS };

template <int U>
struct RegState {
  float f[PX_FIELDS][U];
  __device__ inline float& at(int field, int u) { return f[field][u]; }
  __device__ inline float at(int field, int u) const { return f[field][u]; }
};

template <int U>
struct LdsState {
  float* p;                             // this thread's column of s_px[PX_FIELDS * U][256]
  __device__ inline float& at(int field, int u) { return p[(field * U + u) * 256]; }
  __device__ inline float at(int field, int u) const { return p[(field * U + u) * 256]; }
};

struct ChainAcc { float om, wb, gamma, t[DY_TONE_STEPS]; };

template <bool FAST>
__device__ inline RowCtx load_ctx(const float* __restrict__ params, const float* __restrict__ tone, const float* __restrict__ A, int b,
                                  int c) {
  RowCtx r;
  const float* q = params + b * 8;
  r.omega = q[0]; r.s = q[1 + c]; r.gamma = q[4]; r.alpha = q[5];
  r.A = A ? A[b * 3 + c] : 0.8f;
  float T = 0.f;
#pragma unroll
  for (int i = 0; i < DY_TONE_STEPS; ++i) {
    r.t[i] = tone ? tone[b * DY_TONE_STEPS + i] : 1.f;
    T += r.t[i];
  }
  r.Tsum = T + 1e-30f;
  r.T8 = FAST ? (float)DY_TONE_STEPS * __builtin_amdgcn_rcpf(r.Tsum) : (float)DY_TONE_STEPS / r.Tsum;
  r.K = 1.f;
  return r;
}

// Stages [lo, hi) of the chain on U pixels of one row at once: the wave-uniform dispatch (a scalar branch per stage) is paid once
// for U independent dependency chains.
template <bool FAST, int U, typename S>
__device__ inline void chain_fwd_px(float (&v)[U], const float (&I)[U], const RowCtx& r, unsigned chain, int lo, int hi, S& s) {
  for (int k = lo; k < hi; ++k) {
    switch (fc_code(chain, k)) {                               // wave-uniform
      case DY_FILTER_DEDARK:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float txr = 1.f - r.omega * I[u];
          const float tx = fmaxf(txr, 0.01f);
          const float rtx = FAST ? __builtin_amdgcn_rcpf(tx) : 1.f / tx;
          s.at(IN_DF, u) = v[u];
          s.at(TXR, u) = txr;
          s.at(RTX, u) = rtx;
          v[u] = FAST ? (v[u] - r.A) * rtx + r.A : (v[u] - r.A) / tx + r.A;
        }
        break;
      case DY_FILTER_WB:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s.at(IN_W, u) = v[u];
          v[u] = v[u] * r.s;
        }
        break;
      case DY_FILTER_GAMMA:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float base = fmaxf(v[u], 1e-4f);
          float L;
          s.at(IN_G, u) = v[u];
          if (FAST) {
            L = __builtin_amdgcn_logf(base);                   // v_log_f32 = log2
            v[u] = __builtin_amdgcn_exp2f(r.gamma * L);        // v_exp_f32 = 2^x
          } else {
            L = log2f(base);
            v[u] = powf(base, r.gamma);
          }
          s.at(BASE, u) = base;
          s.at(LOG2B, u) = L;
          s.at(OUT_G, u) = v[u];
        }
        break;
      case DY_FILTER_TONE:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s.at(IN_T, u) = v[u];
          float tot = 0.f;
#pragma unroll
          for (int i = 0; i < DY_TONE_STEPS; ++i)
            tot += fminf(fmaxf(v[u] - (float)i / DY_TONE_STEPS, 0.f), 1.f / DY_TONE_STEPS) * r.t[i];
          v[u] = FAST ? tot * r.T8 : tot * (float)DY_TONE_STEPS / r.Tsum;
          s.at(OUT_T, u) = v[u];
        }
        break;
      case DY_FILTER_CONTRAST:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          s.at(IN_CT, u) = v[u];
          v[u] = v[u] * r.K;
        }
        break;
      default:
        break;
    }
  }
}

// adjoint of stages [lo, hi) in reverse for U pixels: g = d loss / d (output of stage hi - 1) -> d loss / d (input of stage lo)
template <bool FAST, int U, typename S>
__device__ inline void chain_bwd_px(float (&g)[U], const float (&I)[U], const RowCtx& r, unsigned chain, int lo, int hi,
                                    const S& s, ChainAcc& a, float& dK) {
  for (int k = hi - 1; k >= lo; --k) {
    switch (fc_code(chain, k)) {
      case DY_FILTER_DEDARK:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float rtx = s.at(RTX, u);
          if (s.at(TXR, u) >= 0.01f) a.om += g[u] * (s.at(IN_DF, u) - r.A) * I[u] * rtx * rtx;
          g[u] = g[u] * rtx;
        }
        break;
      case DY_FILTER_WB:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          a.wb += g[u] * s.at(IN_W, u);
          g[u] = g[u] * r.s;
        }
        break;
      case DY_FILTER_GAMMA:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float out = s.at(OUT_G, u), base = s.at(BASE, u);
          a.gamma += g[u] * out * (s.at(LOG2B, u) * LN2);
          g[u] = (s.at(IN_G, u) >= 1e-4f) ? g[u] * r.gamma * (FAST ? out * __builtin_amdgcn_rcpf(base) : out / base) : 0.f;
        }
        break;
      case DY_FILTER_TONE:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          // torch.clamp passes the gradient on both bounds: at a knot v = i/8 the slope is t_{i-1} + t_i
          const float gT = FAST ? g[u] * __builtin_amdgcn_rcpf(r.Tsum) : g[u] / r.Tsum;
          const float vin = s.at(IN_T, u), y = s.at(OUT_T, u);
          float slope = 0.f;
#pragma unroll
          for (int i = 0; i < DY_TONE_STEPS; ++i) {
            const float d = vin - (float)i / DY_TONE_STEPS;
            const float cl = fminf(fmaxf(d, 0.f), 1.f / DY_TONE_STEPS);
            a.t[i] += gT * ((float)DY_TONE_STEPS * cl - y);
            slope += (d >= 0.f && d <= 1.f / DY_TONE_STEPS) ? r.t[i] : 0.f;
          }
          g[u] = gT * ((float)DY_TONE_STEPS * slope);
        }
        break;
      case DY_FILTER_CONTRAST:
#pragma unroll
        for (int u = 0; u < U; ++u) {
          dK += g[u] * s.at(IN_CT, u);
          g[u] = g[u] * r.K;
        }
        break;
      default:
        break;
    }
  }
}

struct ChainShape { int n, ct; };      // number of stages, position of Contrast (-1: none)

__device__ inline ChainShape chain_shape(unsigned chain) {
  ChainShape cs = {0, -1};
  for (int k = 0; k < DY_CHAIN_MAX && fc_code(chain, k) != 0; ++k) {
    if (fc_code(chain, k) == DY_FILTER_CONTRAST) cs.ct = k;
    cs.n = k + 1;
  }
  return cs;
}

struct RowLum { float lraw, lum, cl, q; };

// the contrast stage's per-row luminance from columns 0..2 of ITS input (the chain's prefix); sets r.K
template <bool FAST>
__device__ inline RowLum row_gain(const float* xr, const float* ir, RowCtx& r, unsigned chain, int ct, int lane) {
  float v[1] = {0.f};
  if (lane < 3) {
    RegState<1> s;
    const float I[1] = {ir ? ir[lane] : 0.5f};
    v[0] = xr[lane];
    chain_fwd_px<FAST, 1>(v, I, r, chain, 0, ct, s);
  }
  RowLum o;
  o.lraw = 0.27f * __shfl(v[0], 0, 64) + 0.67f * __shfl(v[0], 1, 64) + 0.06f * __shfl(v[0], 2, 64);
  o.lum = fminf(fmaxf(o.lraw, 0.f), 1.f);
  // lerp(img, img / (lum + 1e-6) * cl, alpha) (util_filters.py:316-317) = img * K with a per-row K
  o.cl = -cosf(PI_F * o.lum) * 0.5f + 0.5f;
  o.q = o.cl / (o.lum + 1e-6f);
  r.K = (1.f - r.alpha) + r.alpha * o.q;
  return o;
}

template <bool FAST>
__global__ __launch_bounds__(256) void chain_fwd_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                         const float* __restrict__ tone, const float* __restrict__ A,
                                                         const float* __restrict__ IcA, unsigned chain, float* __restrict__ y, int B,
                                                         int H, int W) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * FC_ROWS + wave;                // (b*3 + c)*H + h
  if (row >= (long)B * 3 * H) return;
  const int h = (int)(row % H), bc = (int)(row / H), c = bc % 3, b = bc / 3;
  RowCtx r = load_ctx<FAST>(params, tone, A, b, c);
  const ChainShape cs = chain_shape(chain);
  const float* xr = x + row * W;
  const float* ir = IcA ? IcA + ((long)b * H + h) * W : nullptr;
  if (cs.ct >= 0) row_gain<FAST>(xr, ir, r, chain, cs.ct, lane);
  float* o = y + row * W;
  for (int w0 = lane; w0 < W; w0 += 64 * FC_PX) {
    float v[FC_PX], I[FC_PX];
    RegState<FC_PX> s;
#pragma unroll
    for (int u = 0; u < FC_PX; ++u) {
      const int w = w0 + 64 * u;
      v[u] = w < W ? xr[w] : 0.f;
      I[u] = (ir && w < W) ? ir[w] : 0.5f;
    }
    chain_fwd_px<FAST, FC_PX>(v, I, r, chain, 0, cs.n, s);
#pragma unroll
    for (int u = 0; u < FC_PX; ++u)
      if (w0 + 64 * u < W) o[w0 + 64 * u] = v[u];
  }
}

// The upstream gradient: f32 planar (what dy_usm_bwd writes), or in the compute dtype T planar (ld == 0) / an NHWC view with
// pixel stride ld (the two layouts dy_usm_bwd itself accepts), for chains without UsmFilter.
template <typename T>
struct GradSrc {
  const float* g32;
  const T* g;
  int ld;
};

template <bool FAST, typename T>
__global__ __launch_bounds__(256) void chain_bwd_kernel(const float* __restrict__ x, const float* __restrict__ params,
                                                         const float* __restrict__ tone, const float* __restrict__ A,
                                                         const float* __restrict__ IcA, unsigned chain, GradSrc<T> gs,
                                                         float* __restrict__ dx, double* dparams, double* dtone, int B, int H, int W,
                                                         int accumulate) {
  __shared__ float s_part[FC_ROWS][FC_NACC];
  __shared__ float s_px[PX_FIELDS * FC_PX_BWD][256];
  LdsState<FC_PX_BWD> st = {&s_px[0][threadIdx.x]};
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * FC_ROWS + wave;
  const bool live = row < (long)B * 3 * H;
  const bool merged = (H % FC_ROWS) == 0;                            // then the block's rows share (b, c)
  const ChainShape cs = chain_shape(chain);
  float tot[FC_NACC];
#pragma unroll
  for (int i = 0; i < FC_NACC; ++i) tot[i] = 0.f;
  int b = 0, c = 0;
  if (live) {
    const int h = (int)(row % H), bc = (int)(row / H);
    c = bc % 3;
    b = bc / 3;
    RowCtx r = load_ctx<FAST>(params, tone, A, b, c);
    const float* xr = x + row * W;
    const float* ir = IcA ? IcA + ((long)b * H + h) * W : nullptr;
    float* dxr = dx ? dx + row * W : nullptr;
    const float* g32 = gs.g32 ? gs.g32 + row * W : nullptr;
    const T* gpl = gs.g ? gs.g + (gs.ld == 0 ? row * W : ((long)b * H + h) * W * gs.ld + c) : nullptr;
    const int gstep = gs.ld == 0 ? 1 : gs.ld;
    RowLum lm = {0.f, 0.f, 0.f, 0.f};
    if (cs.ct >= 0) lm = row_gain<FAST>(xr, ir, r, chain, cs.ct, lane);
    ChainAcc acc;
    acc.om = acc.wb = acc.gamma = 0.f;
#pragma unroll
    for (int i = 0; i < DY_TONE_STEPS; ++i) acc.t[i] = 0.f;
    float dK = 0.f;
    for (int w0 = lane; w0 < W; w0 += 64 * FC_PX_BWD) {
      // a slot past the row's end runs on x = 0 with a zero gradient: every sum it touches gets exactly 0
      float v[FC_PX_BWD], I[FC_PX_BWD], g[FC_PX_BWD];
#pragma unroll
      for (int u = 0; u < FC_PX_BWD; ++u) {
        const int w = w0 + 64 * u;
        const bool in = w < W;
        v[u] = in ? xr[w] : 0.f;
        I[u] = (ir && in) ? ir[w] : 0.5f;
        g[u] = !in ? 0.f : (g32 ? g32[w] : DT<T>::ld(gpl + (long)w * gstep));
      }
      chain_fwd_px<FAST, FC_PX_BWD>(v, I, r, chain, 0, cs.n, st);
      chain_bwd_px<FAST, FC_PX_BWD>(g, I, r, chain, 0, cs.n, st, acc, dK);
      if (dxr) {
#pragma unroll
        for (int u = 0; u < FC_PX_BWD; ++u) {
          const int w = w0 + 64 * u;
          if (w < W) dxr[w] = accumulate ? dxr[w] + g[u] : g[u];
        }
      }
    }
    if (cs.ct >= 0) {
      dK = wave_sum(dK);
      tot[3] = dK * (lm.q - 1.f);
      // d q / d lum, gated by clamp(lum, 0, 1) (inclusive bounds pass the gradient, as torch.clamp does)
      float dlum = 0.f;
      if (lm.lraw >= 0.f && lm.lraw <= 1.f) {
        const float dcl = 0.5f * PI_F * sinf(PI_F * lm.lum);
        dlum = dK * r.alpha * (dcl * (lm.lum + 1e-6f) - lm.cl) / ((lm.lum + 1e-6f) * (lm.lum + 1e-6f));
      }
      if (lane < 3) {                                                 // W >= 3 with Contrast in the chain
        const float coef = lane == 0 ? 0.27f : (lane == 1 ? 0.67f : 0.06f);
        const float I[1] = {ir ? ir[lane] : 0.5f};
        float v[1] = {xr[lane]}, g[1] = {coef * dlum};
        RegState<1> s;
        chain_fwd_px<FAST, 1>(v, I, r, chain, 0, cs.ct, s);
        float unused = 0.f;
        chain_bwd_px<FAST, 1>(g, I, r, chain, 0, cs.ct, s, acc, unused);
        if (dxr) dxr[lane] += g[0];                                   // same lane wrote dxr[lane] in the loop above
      }
    }
    tot[0] = wave_sum(acc.om);
    tot[1] = wave_sum(acc.wb);
    tot[2] = wave_sum(acc.gamma);
    if (tone) {
#pragma unroll
      for (int i = 0; i < DY_TONE_STEPS; ++i) tot[4 + i] = wave_sum(acc.t[i]);
    }
  }
  if (merged) {
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < FC_NACC; ++i) s_part[wave][i] = tot[i];
    }
    __syncthreads();
    const int k = threadIdx.x;
    if (k < FC_NACC && (long)blockIdx.x * FC_ROWS < (long)B * 3 * H && (k < 4 || dtone)) {
      const int bc0 = (int)(((long)blockIdx.x * FC_ROWS) / H);
      float v = 0.f;
#pragma unroll
      for (int rr = 0; rr < FC_ROWS; ++rr) v += s_part[rr][k];
      // f64 atomics: the sum of the f32 block partials does not depend on their arrival order beyond 2^-52 relative (frontend.hip)
      if (k < 4) atomic_add_f64(dparams + (bc0 / 3) * 8 + (k == 0 ? 0 : (k == 1 ? 1 + bc0 % 3 : (k == 2 ? 4 : 5))), (double)v);
      else atomic_add_f64(dtone + (bc0 / 3) * DY_TONE_STEPS + (k - 4), (double)v);
    }
  } else if (live && lane == 0) {
    double* dp = dparams + b * 8;
    atomic_add_f64(dp + 0, (double)tot[0]);
    atomic_add_f64(dp + 1 + c, (double)tot[1]);
    atomic_add_f64(dp + 4, (double)tot[2]);
    atomic_add_f64(dp + 5, (double)tot[3]);
    if (dtone) {
#pragma unroll
      for (int i = 0; i < DY_TONE_STEPS; ++i) atomic_add_f64(dtone + b * DY_TONE_STEPS + i, (double)tot[4 + i]);
    }
  }
}

// ---- feat[5..12] -> tone[8] (tanh_range(0.5, 2), filter_cfg.py:34) -----------------------------------------------------
__global__ void tone_params_fwd_kernel(const float* __restrict__ feat, int feat_ld, float* __restrict__ tone, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * DY_TONE_STEPS) return;
  const int b = i / DY_TONE_STEPS, k = i % DY_TONE_STEPS;
  tone[i] = tanhf(feat[(long)b * feat_ld + 5 + k]) * 0.75f + 1.25f;
}

__global__ void tone_params_bwd_kernel(const float* __restrict__ feat, int feat_ld, const double* __restrict__ dtone,
                                       float* __restrict__ dfeat, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * DY_TONE_STEPS) return;
  const int b = i / DY_TONE_STEPS, k = i % DY_TONE_STEPS;
  const float t = tanhf(feat[(long)b * feat_ld + 5 + k]);
  dfeat[(long)b * feat_ld + 5 + k] = (float)dtone[i] * 0.75f * (1.f - t * t);   // the f64 sum of the f32 block partials, rounded once
}

// host-side check of a chain word; returns 0 and fills has_* or sets the error
int check_chain(const char* who, unsigned chain, bool* has_tone, bool* has_contrast) {
  unsigned seen = 0;
  int n = 0;
  for (; n < 8 && fc_code(chain, n) != 0; ++n) {
    const int code = fc_code(chain, n);
    DY_CHECK(code >= DY_FILTER_DEDARK && code <= DY_FILTER_CONTRAST, "%s: unknown filter code %d at position %d", who, code, n);
    DY_CHECK(!(seen & (1u << code)), "%s: filter code %d is repeated", who, code);
    seen |= 1u << code;
  }
  DY_CHECK(n >= 1 && n <= DY_CHAIN_MAX && (n == 8 || (chain >> (4 * n)) == 0), "%s: a chain has 1..%d stages, codes end at the first 0", who,
           DY_CHAIN_MAX);
  *has_tone = (seen & (1u << DY_FILTER_TONE)) != 0;
  *has_contrast = (seen & (1u << DY_FILTER_CONTRAST)) != 0;
  return 0;
}

}  // namespace

extern "C" int dy_tone_params_fwd(const float* feat, int feat_ld, float* tone, int B, void* stream) {
  DY_CHECK(feat && tone && B > 0 && feat_ld >= 15, "dy_tone_params_fwd: bad args");
  tone_params_fwd_kernel<<<dy_cdiv(B * DY_TONE_STEPS, 256), 256, 0, (hipStream_t)stream>>>(feat, feat_ld, tone, B);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_tone_params_bwd(const float* feat, int feat_ld, const double* dtone, float* dfeat, int B, void* stream) {
  DY_CHECK(feat && dtone && dfeat && B > 0 && feat_ld >= 15, "dy_tone_params_bwd: bad args");
  tone_params_bwd_kernel<<<dy_cdiv(B * DY_TONE_STEPS, 256), 256, 0, (hipStream_t)stream>>>(feat, feat_ld, dtone, dfeat, B);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_filter_chain_fwd(const float* x, const float* params, const float* tone, const float* A, const float* IcA,
                                   unsigned chain, float* y, int B, int H, int W, int fast_math, void* stream) {
  bool has_tone, has_ct;
  if (int e = check_chain("dy_filter_chain_fwd", chain, &has_tone, &has_ct)) return e;
  DY_CHECK(x && params && y && B > 0 && H > 0 && W >= (has_ct ? 3 : 1), "dy_filter_chain_fwd: bad args (W must be >= 3 with Contrast)");
  DY_CHECK(tone || !has_tone, "dy_filter_chain_fwd: the chain has a tone stage but tone is NULL");
  if (!has_tone) tone = nullptr;
  const unsigned grid = dy_cdiv((long)B * 3 * H, FC_ROWS);
  if (fast_math) chain_fwd_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(x, params, tone, A, IcA, chain, y, B, H, W);
  else chain_fwd_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(x, params, tone, A, IcA, chain, y, B, H, W);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_filter_chain_bwd(const float* x, const float* params, const float* tone, const float* A, const float* IcA,
                                   unsigned chain, const float* dy_nchw, const void* dy_any, int dy_ld, int dtype, float* dx,
                                   double* dparams, double* dtone, int B, int H, int W, int accumulate, int fast_math, void* stream) {
  bool has_tone, has_ct;
  if (int e = check_chain("dy_filter_chain_bwd", chain, &has_tone, &has_ct)) return e;
  DY_CHECK(x && params && dparams && B > 0 && H > 0 && W >= (has_ct ? 3 : 1), "dy_filter_chain_bwd: bad args (W must be >= 3 with Contrast)");
  DY_CHECK((tone && dtone) || !has_tone, "dy_filter_chain_bwd: the chain has a tone stage but tone / dtone is NULL");
  DY_CHECK((dy_nchw != nullptr) != (dy_any != nullptr), "dy_filter_chain_bwd: exactly one of dy_nchw / dy_any");
  DY_CHECK(dy_any == nullptr || dy_ld >= 3 || dy_ld == 0, "dy_filter_chain_bwd: bad dy_ld");
  if (int e = dy_check_dtype("dy_filter_chain_bwd", dtype)) return e;
  if (!has_tone) tone = nullptr, dtone = nullptr;
  const unsigned grid = dy_cdiv((long)B * 3 * H, FC_ROWS);
  DY_DISPATCH_DTYPE("dy_filter_chain_bwd", dtype, {
    GradSrc<T> gs = {dy_nchw, (const T*)dy_any, dy_ld};
    if (fast_math)
      chain_bwd_kernel<true, T><<<grid, 256, 0, (hipStream_t)stream>>>(x, params, tone, A, IcA, chain, gs, dx, dparams, dtone, B, H, W, accumulate);
    else
      chain_bwd_kernel<false, T><<<grid, 256, 0, (hipStream_t)stream>>>(x, params, tone, A, IcA, chain, gs, dx, dparams, dtone, B, H, W, accumulate);
  });
  DY_LAUNCH_CHECK();
  return 0;
}
