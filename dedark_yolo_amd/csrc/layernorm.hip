// The element-wise side of the transformer encoder layer (reference ultralytics/nn/modules/transformer.py:14-83,
// TransformerEncoderLayer.forward_post / AIFI): the residual add fused into LayerNorm, exact GELU, and the add of the fixed
// sine-cosine position table.  All HBM-bound VALU kernels over NHWC token matrices [rows = B H W][ld], ld >= C; a view may be a
// channel slice of a wider buffer: exactly C channels of a row are read / written.
//
// dy_add_layernorm_fwd / _bwd: z = a + b lives in registers only.  A row is owned by one wave (C <= 1024, four rows per workgroup)
// or by the whole workgroup (C <= 2048); a lane keeps its 16 (8) values of z as f32, so a and b are read once and y written once.
// The statistics are two reductions over those registers: the mean, then the mean of the squared CENTRED values (never
// E[z^2] - mean^2: a row of mean 1e3 and unit spread would lose every digit of its variance in f32).
// The backward recomputes z^ = (z - mean) rstd from a, b and the forward's stats.  dgamma / dbeta are deterministic: a workgroup
// owns a row range fixed by the shape, a lane sums its own columns over the rows of its wave in order, the four waves are joined
// through LDS in wave order, and a second kernel adds the per-workgroup partials in an order fixed by their count.  No atomics.
//
// Access width: 16-byte vectors where C, every ld and every base allow it, chunks of four element accesses otherwise (C % 4 == 0
// is the rule of all five entries).
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NT = 256;
constexpr int LN_WAVE_C = 1024;            // widest row one wave owns
constexpr int LN_MAX_C = DY_LN_MAX_C;      // widest row at all (one workgroup)
constexpr int LN_PARTS = DY_LN_MAX_PARTS;  // most workgroups of the backward = most dgamma / dbeta partials
constexpr int EW_CAP = 8192;

// W consecutive elements at p into / out of f32 registers: one 16-byte access (VEC: W == DT<T>::VE) or W element accesses
template <typename T, bool VEC, int W> __device__ inline void ld_chunk(const T* p, float* v) {
  if constexpr (VEC) ldvec<T>(p, v);
  else {
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = DT<T>::ld(p + e);
  }
}
template <typename T, bool VEC, int W> __device__ inline void st_chunk(T* p, const float* v) {
  if constexpr (VEC) stvec<T>(p, v);
  else {
#pragma unroll
    for (int e = 0; e < W; ++e) DT<T>::st(p + e, v[e]);
  }
}

// How a row is spread over its owner (G = 64 lanes or 256 threads): chunk p of thread t covers columns (p G + t) W .. + W
template <typename T, bool VEC, bool BLOCK> struct Row {
  static constexpr int W = VEC ? DT<T>::VE : 4;
  static constexpr int G = BLOCK ? NT : 64;
  static constexpr int NP = (BLOCK ? LN_MAX_C / NT : LN_WAVE_C / 64) / W;   // chunks per thread
  static constexpr int NV = NP * W;                                          // values per thread
  __device__ static inline int tid() { return BLOCK ? threadIdx.x : (threadIdx.x & 63); }
  __device__ static inline float sum(float v, float* sm) { return BLOCK ? block_sum(v, sm) : wave_sum(v); }
};

// z = a (+ b) of one row into registers, zeros beyond C
template <typename R, typename T, bool VEC>
__device__ inline void load_z(const T* __restrict__ a, const T* __restrict__ b, int C, float* z) {
  const int t = R::tid();
#pragma unroll
  for (int p = 0; p < R::NP; ++p) {
    const int c = (p * R::G + t) * R::W;
    float* zp = z + p * R::W;
    if (c < C) {
      ld_chunk<T, VEC, R::W>(a + c, zp);
      if (b) {
        float t2[R::W];
        ld_chunk<T, VEC, R::W>(b + c, t2);
#pragma unroll
        for (int e = 0; e < R::W; ++e) zp[e] += t2[e];
      }
    } else {
#pragma unroll
      for (int e = 0; e < R::W; ++e) zp[e] = 0.f;
    }
  }
}

template <typename T, bool VEC, bool BLOCK>
__global__ __launch_bounds__(NT) void add_layernorm_fwd_kernel(const T* __restrict__ a, long a_ld, const T* __restrict__ b, long b_ld,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               T* __restrict__ y, long y_ld, float* __restrict__ stats, long rows, int C,
                                                               float eps) {
  using R = Row<T, VEC, BLOCK>;
  __shared__ float sm[17];
  const long row = BLOCK ? (long)blockIdx.x : (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;                                      // (wave-uniform; in BLOCK mode workgroup-uniform)
  const int t = R::tid();
  float z[R::NV];
  load_z<R, T, VEC>(a + row * a_ld, b ? b + row * b_ld : nullptr, C, z);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < R::NV; ++i) s += z[i];
  const float mean = R::sum(s, sm) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int p = 0; p < R::NP; ++p) {
    const bool in = (p * R::G + t) * R::W < C;
#pragma unroll
    for (int e = 0; e < R::W; ++e) {
      const float d = z[p * R::W + e] - mean;
      z[p * R::W + e] = d;
      q += in ? d * d : 0.f;
    }
  }
  const float rstd = rsqrtf(R::sum(q, sm) / (float)C + eps);
  if (stats && t == 0) {
    stats[2 * row] = mean;
    stats[2 * row + 1] = rstd;
  }
  T* yr = y + row * y_ld;
#pragma unroll
  for (int p = 0; p < R::NP; ++p) {
    const int c = (p * R::G + t) * R::W;
    if (c < C) {
      float o[R::W];
#pragma unroll
      for (int e = 0; e < R::W; ++e) o[e] = z[p * R::W + e] * rstd * gamma[c + e] + beta[c + e];
      st_chunk<T, VEC, R::W>(yr + c, o);
    }
  }
}

// Workgroup j owns rows [j per, (j + 1) per), per = ceil(rows / gridDim.x); in wave mode wave w takes every fourth of them.
// part (nullable): f32 [gridDim.x][2][C], this workgroup's sums of dy z^ and of dy over its rows.
template <typename T, bool VEC, bool BLOCK>
__global__ __launch_bounds__(NT) void add_layernorm_bwd_kernel(const T* __restrict__ a, long a_ld, const T* __restrict__ b, long b_ld,
                                                               const float* __restrict__ stats, const float* __restrict__ gamma,
                                                               const T* __restrict__ dy, long dy_ld, T* __restrict__ dz, long dz_ld,
                                                               int accumulate, float* __restrict__ part, long rows, int C) {
  using R = Row<T, VEC, BLOCK>;
  __shared__ float sm[17];
  __shared__ float join[BLOCK ? 1 : 3 * 2 * LN_WAVE_C];          // waves 1..3 hand their column sums to wave 0
  const int t = R::tid(), wave = threadIdx.x >> 6;
  const long per = (rows + gridDim.x - 1) / gridDim.x;
  const long r0 = (long)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
  const float inv_c = 1.0f / (float)C;
  float gm[R::NV], dg[R::NV], db[R::NV];
#pragma unroll
  for (int p = 0; p < R::NP; ++p) {
    const int c = (p * R::G + t) * R::W;
#pragma unroll
    for (int e = 0; e < R::W; ++e) {
      gm[p * R::W + e] = c < C ? gamma[c + e] : 0.f;
      dg[p * R::W + e] = 0.f;
      db[p * R::W + e] = 0.f;
    }
  }
  for (long row = BLOCK ? r0 : r0 + wave; row < r1; row += BLOCK ? 1 : 4) {
    float z[R::NV], g[R::NV];
    load_z<R, T, VEC>(a + row * a_ld, b ? b + row * b_ld : nullptr, C, z);
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    const T* gr = dy + row * dy_ld;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int p = 0; p < R::NP; ++p) {
      const int c = (p * R::G + t) * R::W;
      float* gp = g + p * R::W;
      if (c < C) {
        ld_chunk<T, VEC, R::W>(gr + c, gp);
#pragma unroll
        for (int e = 0; e < R::W; ++e) {
          const int i = p * R::W + e;
          z[i] = (z[i] - mean) * rstd;                           // z^
          db[i] += gp[e];
          dg[i] += gp[e] * z[i];
          gp[e] *= gm[i];                                        // g = dy gamma
          s1 += gp[e];
          s2 += gp[e] * z[i];
        }
      } else {
#pragma unroll
        for (int e = 0; e < R::W; ++e) gp[e] = 0.f, z[p * R::W + e] = 0.f;
      }
    }
    const float m1 = R::sum(s1, sm) * inv_c;
    const float m2 = R::sum(s2, sm) * inv_c;
    T* dr = dz + row * dz_ld;
#pragma unroll
    for (int p = 0; p < R::NP; ++p) {
      const int c = (p * R::G + t) * R::W;
      if (c < C) {
        float o[R::W];
#pragma unroll
        for (int e = 0; e < R::W; ++e) o[e] = rstd * (g[p * R::W + e] - m1 - z[p * R::W + e] * m2);
        if (accumulate) {
          float old[R::W];
          ld_chunk<T, VEC, R::W>(dr + c, old);
#pragma unroll
          for (int e = 0; e < R::W; ++e) o[e] += old[e];
        }
        st_chunk<T, VEC, R::W>(dr + c, o);
      }
    }
  }
  if (!part) return;
  if constexpr (!BLOCK) {
    if (wave > 0) {
#pragma unroll
      for (int p = 0; p < R::NP; ++p) {
        const int c = (p * R::G + t) * R::W;
        if (c < C) {
#pragma unroll
          for (int e = 0; e < R::W; ++e) {
            join[((wave - 1) * 2 + 0) * LN_WAVE_C + c + e] = dg[p * R::W + e];
            join[((wave - 1) * 2 + 1) * LN_WAVE_C + c + e] = db[p * R::W + e];
          }
        }
      }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int p = 0; p < R::NP; ++p) {
      const int c = (p * R::G + t) * R::W;
      if (c < C) {
        for (int w = 0; w < 3; ++w) {
#pragma unroll
          for (int e = 0; e < R::W; ++e) {
            dg[p * R::W + e] += join[(w * 2 + 0) * LN_WAVE_C + c + e];
            db[p * R::W + e] += join[(w * 2 + 1) * LN_WAVE_C + c + e];
          }
        }
      }
    }
  }
  float* pg = part + (long)blockIdx.x * 2 * C;
#pragma unroll
  for (int p = 0; p < R::NP; ++p) {
    const int c = (p * R::G + t) * R::W;
    if (c < C) {
#pragma unroll
      for (int e = 0; e < R::W; ++e) {
        pg[c + e] = dg[p * R::W + e];
        pg[C + c + e] = db[p * R::W + e];
      }
    }
  }
}

// dgamma | dbeta [c] = sum of the partials in a fixed order: a workgroup owns 16 of the 2 C columns, thread (column, group g) adds
// the partials g, g + 16, g + 32, ... in that order, and the 16 group sums are added in group order.  (One thread per column walking
// all 512 partials alone took 120 us at C = 256: two workgroups of dependent loads.)
__global__ __launch_bounds__(NT) void layernorm_param_final_kernel(const float* __restrict__ part, int parts, int C, float* __restrict__ dgamma,
                                                                   float* __restrict__ dbeta) {
  __shared__ float sm[16][17];
  const int col = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + col;
  float v = 0.f;
  if (i < 2 * C)
    for (int j = grp; j < parts; j += 16) v += part[(long)j * 2 * C + i];
  sm[grp][col] = v;
  __syncthreads();
  if (grp != 0 || i >= 2 * C) return;
  float t = 0.f;
#pragma unroll
  for (int g = 0; g < 16; ++g) t += sm[g][col];
  if (i < C) dgamma[i] = t;
  else dbeta[i - C] = t;
}

// ---- exact GELU ---------------------------------------------------------------------------------------------------------------
__device__ inline float gelu_f(float u) { return 0.5f * u * (1.0f + erff(u * 0.70710678118654752440f)); }
__device__ inline float dgelu_f(float u) {
  const float cdf = 0.5f * (1.0f + erff(u * 0.70710678118654752440f));
  const float pdf = 0.39894228040143267794f * expf(-0.5f * u * u);
  return cdf + u * pdf;
}

template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void gelu_fwd_kernel(const T* __restrict__ u, long u_ld, T* __restrict__ y, long y_ld, long pixels, int C) {
  constexpr int W = VEC ? DT<T>::VE : 4;
  const int CG = C / W;
  const long total = pixels * CG;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const long px = i / CG;
    const int c = (int)(i - px * CG) * W;
    float v[W];
    ld_chunk<T, VEC, W>(u + px * u_ld + c, v);
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = gelu_f(v[e]);
    st_chunk<T, VEC, W>(y + px * y_ld + c, v);
  }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void gelu_bwd_kernel(const T* __restrict__ u, long u_ld, const T* __restrict__ dy, long dy_ld,
                                                      T* __restrict__ du, long du_ld, long pixels, int C) {
  constexpr int W = VEC ? DT<T>::VE : 4;
  const int CG = C / W;
  const long total = pixels * CG;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const long px = i / CG;
    const int c = (int)(i - px * CG) * W;
    float v[W], g[W];
    ld_chunk<T, VEC, W>(u + px * u_ld + c, v);
    ld_chunk<T, VEC, W>(dy + px * dy_ld + c, g);
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] = g[e] * dgelu_f(v[e]);
    st_chunk<T, VEC, W>(du + px * du_ld + c, v);
  }
}

// ---- y[b][l][c] = x[b][l][c] + pos[l][c] ----------------------------------------------------------------------------------------
template <typename T, bool VEC>
__global__ __launch_bounds__(NT) void add_pos_kernel(const T* __restrict__ x, long x_ld, const T* __restrict__ pos, T* __restrict__ y,
                                                     long y_ld, long rows, int L, int C) {
  constexpr int W = VEC ? DT<T>::VE : 4;
  const int CG = C / W;
  const long total = rows * CG;
  for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
    const long px = i / CG;
    const int c = (int)(i - px * CG) * W;
    const int l = (int)(px % L);
    float v[W], p[W];
    ld_chunk<T, VEC, W>(x + px * x_ld + c, v);
    ld_chunk<T, VEC, W>(pos + (long)l * C + c, p);
#pragma unroll
    for (int e = 0; e < W; ++e) v[e] += p[e];
    st_chunk<T, VEC, W>(y + px * y_ld + c, v);
  }
}

// dy_check_lanes for one more view of the entry; `vec` is cleared when the view does not allow 16-byte accesses
int check_row_view(const char* who, const void* p, long ld, int C, int dtype, bool* vec) {
  if (int e = dy_check_lanes(who, p, ld, C, dtype)) return e;
  if (dy_view_bytes(p, ld, C, dy_elem_size(dtype)) != 16) *vec = false;
  return 0;
}

int check_c(const char* who, int C, int dtype, int max_c) {
  if (int e = dy_check_dtype(who, dtype)) return e;
  DY_CHECK(C >= 4 && C % 4 == 0 && (max_c == 0 || C <= max_c), "%s: C=%d must be a multiple of 4%s", who, C, max_c ? ", 4 <= C <= 2048" : "");
  return 0;
}

int ln_parts(long rows, int C) {
  const long per_pass = C > LN_WAVE_C ? 1 : 4;
  const long p = (rows + per_pass - 1) / per_pass;
  return (int)(p < 1 ? 1 : (p > LN_PARTS ? LN_PARTS : p));
}

}  // namespace

#define LN_DISPATCH(who, dtype, vec, block, KERNEL, GRID, ...)                                        \
  DY_DISPATCH_DTYPE(who, dtype, {                                                                     \
    if (vec && block) KERNEL<T, true, true><<<GRID, NT, 0, st>>>(__VA_ARGS__);                        \
    else if (vec) KERNEL<T, true, false><<<GRID, NT, 0, st>>>(__VA_ARGS__);                           \
    else if (block) KERNEL<T, false, true><<<GRID, NT, 0, st>>>(__VA_ARGS__);                         \
    else KERNEL<T, false, false><<<GRID, NT, 0, st>>>(__VA_ARGS__);                                   \
  })

#define EW_DISPATCH(who, dtype, vec, KERNEL, GRID, ...)                                               \
  DY_DISPATCH_DTYPE(who, dtype, {                                                                     \
    if (vec) KERNEL<T, true><<<GRID, NT, 0, st>>>(__VA_ARGS__);                                       \
    else KERNEL<T, false><<<GRID, NT, 0, st>>>(__VA_ARGS__);                                          \
  })

extern "C" int dy_add_layernorm_fwd(const void* a, int64_t a_ld, const void* b, int64_t b_ld, const float* gamma, const float* beta, void* y,
                                    int64_t y_ld, float* stats, int64_t rows, int C, float eps, int dtype, void* stream) {
  if (int e = check_c("dy_add_layernorm_fwd", C, dtype, LN_MAX_C)) return e;
  DY_CHECK(rows >= 0 && rows < (1L << 31) && gamma && beta, "dy_add_layernorm_fwd: bad rows or null gamma / beta");
  bool vec = true;
  if (int e = check_row_view("dy_add_layernorm_fwd(a)", a, a_ld, C, dtype, &vec)) return e;
  if (b)
    if (int e = check_row_view("dy_add_layernorm_fwd(b)", b, b_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_add_layernorm_fwd(y)", y, y_ld, C, dtype, &vec)) return e;
  if (rows == 0) return 0;
  const bool block = C > LN_WAVE_C;
  const int grid = block ? (int)rows : dy_cdiv(rows, 4);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("add_layernorm_fwd_kernel");
  LN_DISPATCH("dy_add_layernorm_fwd", dtype, vec, block, add_layernorm_fwd_kernel, grid, (const T*)a, a_ld, (const T*)b, b_ld, gamma, beta,
              (T*)y, y_ld, stats, rows, C, eps);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_add_layernorm_bwd(const void* a, int64_t a_ld, const void* b, int64_t b_ld, const float* stats, const float* gamma,
                                    const void* dy, int64_t dy_ld, void* dz, int64_t dz_ld, int accumulate, float* dgamma, float* dbeta,
                                    float* scratch, int64_t scratch_elems, int64_t rows, int C, int dtype, void* stream) {
  if (int e = check_c("dy_add_layernorm_bwd", C, dtype, LN_MAX_C)) return e;
  DY_CHECK(rows >= 0 && rows < (1L << 31) && gamma && stats, "dy_add_layernorm_bwd: bad rows or null gamma / stats");
  DY_CHECK((dgamma != nullptr) == (dbeta != nullptr), "dy_add_layernorm_bwd: dgamma and dbeta come together");
  bool vec = true;
  if (int e = check_row_view("dy_add_layernorm_bwd(a)", a, a_ld, C, dtype, &vec)) return e;
  if (b)
    if (int e = check_row_view("dy_add_layernorm_bwd(b)", b, b_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_add_layernorm_bwd(dy)", dy, dy_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_add_layernorm_bwd(dz)", dz, dz_ld, C, dtype, &vec)) return e;
  const int parts = ln_parts(rows, C);
  DY_CHECK(!dgamma || (scratch && scratch_elems >= (int64_t)parts * 2 * C), "dy_add_layernorm_bwd: scratch needs %ld floats",
           (long)parts * 2 * C);
  const bool block = C > LN_WAVE_C;
  hipStream_t st = (hipStream_t)stream;
  float* part = dgamma ? scratch : nullptr;
  dy_note_kernel("add_layernorm_bwd_kernel");
  LN_DISPATCH("dy_add_layernorm_bwd", dtype, vec, block, add_layernorm_bwd_kernel, parts, (const T*)a, a_ld, (const T*)b, b_ld, stats, gamma,
              (const T*)dy, dy_ld, (T*)dz, dz_ld, accumulate, part, rows, C);
  DY_LAUNCH_CHECK();
  if (dgamma) {
    layernorm_param_final_kernel<<<dy_cdiv(2 * C, 16), NT, 0, st>>>(scratch, parts, C, dgamma, dbeta);
    DY_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int dy_gelu_fwd(const void* u, int64_t u_ld, void* y, int64_t y_ld, int64_t pixels, int C, int dtype, void* stream) {
  if (int e = check_c("dy_gelu_fwd", C, dtype, 0)) return e;
  DY_CHECK(pixels >= 0, "dy_gelu_fwd: bad size");
  bool vec = true;
  if (int e = check_row_view("dy_gelu_fwd(u)", u, u_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_gelu_fwd(y)", y, y_ld, C, dtype, &vec)) return e;
  if (pixels == 0) return 0;
  const int grid = dy_ew_blocks(pixels * (C / (vec ? dy_vec_elems(dtype) : 4)), EW_CAP);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("gelu_fwd_kernel");
  EW_DISPATCH("dy_gelu_fwd", dtype, vec, gelu_fwd_kernel, grid, (const T*)u, u_ld, (T*)y, y_ld, pixels, C);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_gelu_bwd(const void* u, int64_t u_ld, const void* dy, int64_t dy_ld, void* du, int64_t du_ld, int64_t pixels, int C,
                           int dtype, void* stream) {
  if (int e = check_c("dy_gelu_bwd", C, dtype, 0)) return e;
  DY_CHECK(pixels >= 0, "dy_gelu_bwd: bad size");
  bool vec = true;
  if (int e = check_row_view("dy_gelu_bwd(u)", u, u_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_gelu_bwd(dy)", dy, dy_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_gelu_bwd(du)", du, du_ld, C, dtype, &vec)) return e;
  if (pixels == 0) return 0;
  const int grid = dy_ew_blocks(pixels * (C / (vec ? dy_vec_elems(dtype) : 4)), EW_CAP);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("gelu_bwd_kernel");
  EW_DISPATCH("dy_gelu_bwd", dtype, vec, gelu_bwd_kernel, grid, (const T*)u, u_ld, (const T*)dy, dy_ld, (T*)du, du_ld, pixels, C);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_add_pos(const void* x, int64_t x_ld, const void* pos, void* y, int64_t y_ld, int B, int L, int C, int dtype, void* stream) {
  if (int e = check_c("dy_add_pos", C, dtype, 0)) return e;
  DY_CHECK(B >= 0 && L >= 1, "dy_add_pos: bad size");
  bool vec = true;
  if (int e = check_row_view("dy_add_pos(x)", x, x_ld, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_add_pos(pos)", pos, C, C, dtype, &vec)) return e;
  if (int e = check_row_view("dy_add_pos(y)", y, y_ld, C, dtype, &vec)) return e;
  if (B == 0) return 0;
  const long rows = (long)B * L;
  const int grid = dy_ew_blocks(rows * (C / (vec ? dy_vec_elems(dtype) : 4)), EW_CAP);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("add_pos_kernel");
  EW_DISPATCH("dy_add_pos", dtype, vec, add_pos_kernel, grid, (const T*)x, x_ld, (const T*)pos, (T*)y, y_ld, rows, L, C);
  DY_LAUNCH_CHECK();
  return 0;
}
