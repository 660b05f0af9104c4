// Fused multi-head attention for the transformer blocks (reference ultralytics/nn/modules/transformer.py:109,115: the
// nn.MultiheadAttention call of TransformerLayer; torch's multi_head_attention_forward after its in-projection and before out_proj):
//   O[b, i, h D + c] = sum_j softmax_j(scale * Q[b, i, h, :] . K[b, j, h, :]) V[b, j, h D + c]
// and its backward in the flash form: P is recomputed from Q, K and the forward's log-sum-exp, no L x L tensor reaches global memory.
//
// Views: Q, K, V, O (and dO, dQ, dK, dV) are token-major [B L][pitch] views, normally channel slices of one [B, L, 3C] buffer; head
// h is the channel run [h D, (h + 1) D) of its view.  Exactly those channels are read / written; D % 8 == 0, 8 <= D <= 128.
//
// One workgroup = 4 waves owns 64 rows (queries in attn_fwd_kernel and attn_dq_kernel, keys in attn_dkv_kernel) of one (batch, head),
// a wave 16 of them, and sweeps the other side in tiles of TS rows (64 for the 16-bit types, 32 for f32).  All operands are staged in
// LDS as [row][DP + pad] images, DP = D rounded up to 32 with zeros (the MFMA K step; in LDS only).  Products are
// v_mfma_f32_16x16x32 (bf16 / f16) or v_mfma_f32_16x16x4_f32 with f32 accumulators; an operand whose K index runs over the image's
// rows (V in P V, dO in P^T dO, K in dS K, Q in dS^T Q) is read transposed (ds_read_b64_tr_b16, the 16-bit types) or element-wise
// (f32).  P and dS cross LDS once per tile to become the A operand of the second product; in the 16-bit modes they are rounded to
// the operand type there, in f32 nothing is rounded.  Softmax statistics (running maximum, sum, LSE, delta) are f32.
// Each kernel is instantiated per padded head dim (DP / 16 = 2, 4, 6 or 8 accumulator blocks), so registers and occupancy follow D.
//
// Backward is two kernels and deterministic: attn_dq_kernel owns a query tile and sweeps the keys (dQ), attn_dkv_kernel owns a key
// tile and sweeps the queries (dK, dV); every output element is summed by one wave in a fixed order.  No atomics, no hand-off
// between workgroups, every loop bound is a function of the shape.
#include <type_traits>
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NT = 256;
constexpr int TQ = 64;      // rows a workgroup owns (16 per wave)

template <typename T> struct Cfg {
  static constexpr int TS = sizeof(T) == 4 ? 32 : 64;     // rows of a swept tile
  static constexpr int PAD = sizeof(T) == 4 ? 4 : 8;      // 16 bytes: rows stay 16-byte aligned and spread over the banks
  static constexpr int LDP = TS + PAD;                    // row pitch of a wave's [16][TS] P / dS image
};

// The 16x16x32 operand of an LDS image [32 k-rows][rs 16-bit elements] whose K index runs over the ROWS: lane (column c0 + (lane & 15),
// k group lane >> 4) gets rows 8 (lane >> 4) .. + 7 of its column through two ds_read_b64_tr_b16 (cru.hip's tr_frag).  The whole wave
// must be active.
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

// acc[m][n] += sum_{k < 32} A[a0 + m][ak + k] * Bop[k][n] over two LDS images; A is row-major in k, Bop[k][n] is
// B[b0 + n][bk + k] (BT == false: both operands K-contiguous) or B[bk + k][b0 + n] (BT == true: K runs over B's rows)
template <typename T, bool BT>
__device__ inline f32x4 mma32(const T* __restrict__ A, int lda, int a0, int ak, const T* __restrict__ B, int ldb, int b0, int bk, f32x4 acc) {
  const int lane = threadIdx.x & 63, col = lane & 15, kg = lane >> 4;
  if constexpr (sizeof(T) == 4) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int k = 4 * s + kg;
      const float a = A[(a0 + col) * lda + ak + k];
      const float b = BT ? B[(bk + k) * ldb + b0 + col] : B[(b0 + col) * ldb + bk + k];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
  } else {
    const u32x4 a = *reinterpret_cast<const u32x4*>(A + (a0 + col) * lda + ak + 8 * kg);
    u32x4 b;
    if constexpr (BT) b = tr_frag<T>(B + bk * ldb, ldb, b0);
    else b = *reinterpret_cast<const u32x4*>(B + (b0 + col) * ldb + bk + 8 * kg);
    acc = mfma_16x16x32<T>(a, b, acc);
  }
  return acc;
}

// img[r][0 .. DP) = src row (row0 + r), channels [0, D), zeros for rows >= L and channels >= D; r < rows.  src points at channel 0 of
// the head in token 0 of the batch; vec: 16-byte loads allowed
template <typename T>
__device__ inline void stage(T* __restrict__ img, int ld, const T* __restrict__ src, long pitch, int row0, int rows, int L, int D, int DP, int vec) {
  const int octs = DP >> 3;
  for (int idx = threadIdx.x; idx < rows * octs; idx += NT) {
    const int r = idx / octs, o = idx - r * octs;
    __attribute__((aligned(16))) T v[8];
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = 0.f;
    } else {
      *reinterpret_cast<u32x4*>(v) = u32x4{0u, 0u, 0u, 0u};
    }
    if (row0 + r < L && 8 * o < D) {           // D % 8 == 0: an octet is whole or empty
      const T* p = src + (long)(row0 + r) * pitch + 8 * o;
      if (vec) {
        if constexpr (sizeof(T) == 4) {
          *reinterpret_cast<f32x4*>(v) = *reinterpret_cast<const f32x4*>(p);
          *reinterpret_cast<f32x4*>(v + 4) = *reinterpret_cast<const f32x4*>(p + 4);
        } else {
          *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(p);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[i];
      }
    }
    T* d = img + r * ld + 8 * o;
    if constexpr (sizeof(T) == 4) {
      *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(v);
      *reinterpret_cast<f32x4*>(d + 4) = *reinterpret_cast<const f32x4*>(v + 4);
    } else {
      *reinterpret_cast<u32x4*>(d) = *reinterpret_cast<const u32x4*>(v);
    }
  }
}

// the f32 row constants of a staged query tile: lse_s[r] = LSE of query row0 + r, del_s[r] = sum_c dO[r][c] O[r][c] (dO from its LDS
// image, O from global memory); 0 for rows >= L.  rows <= 64: four threads per row, whole waves active
template <typename T>
__device__ inline void stage_rowconst(float* __restrict__ lse_s, float* __restrict__ del_s, const T* __restrict__ dOs, int ld, const T* __restrict__ o,
                                      long o_pitch, const float* __restrict__ lse, int row0, int rows, int L, int D) {
  const int t = threadIdx.x, r = t >> 2, part = t & 3;
  if (r < rows) {
    float s = 0.f;
    const bool live = row0 + r < L;
    if (live) {
      const T* op = o + (long)(row0 + r) * o_pitch;
      for (int c = part; c < D; c += 4) s += DT<T>::ld(dOs + r * ld + c) * DT<T>::ld(op + c);
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    if (part == 0) {
      del_s[r] = s;
      lse_s[r] = live ? lse[row0 + r] : 0.f;
    }
  }
}

__device__ inline float group16_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ inline float group16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------
// grid (query tiles, H, B).  LDS: Qs[TQ][ld] Ks[TS][ld] Vs[TS][ld] Ps[4][16][LDP]
template <typename T, int NDB>
__global__ __launch_bounds__(NT) void attn_fwd_kernel(const T* __restrict__ q, long q_ld, const T* __restrict__ k, long k_ld, const T* __restrict__ v,
                                                      long v_ld, T* __restrict__ o, long o_ld, float* __restrict__ lse, int L, int H, int D, int DP,
                                                      float scale, int vq, int vk, int vv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  constexpr int TS = Cfg<T>::TS, NS = TS / 16, LDP = Cfg<T>::LDP;
  const int ld = DP + Cfg<T>::PAD;
  T* Qs = reinterpret_cast<T*>(attn_smem);
  T* Ks = Qs + TQ * ld;
  T* Vs = Ks + TS * ld;
  T* Ps = Vs + TS * ld;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, col = lane & 15, kg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * TQ;
  const long tok0 = (long)b * L;
  const int ndb = (D + 15) >> 4;
  T* Pw = Ps + wave * 16 * LDP;
  stage<T>(Qs, ld, q + tok0 * q_ld + h * D, q_ld, q0, TQ, L, D, DP, vq);
  float m[4], l[4];
  f32x4 acc[NDB];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    m[i] = -INFINITY;
    l[i] = 0.f;
  }
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < L; k0 += TS) {
    __syncthreads();                                        // the previous tile's reads are done
    stage<T>(Ks, ld, k + tok0 * k_ld + h * D, k_ld, k0, TS, L, D, DP, vk);
    stage<T>(Vs, ld, v + tok0 * v_ld + h * D, v_ld, k0, TS, L, D, DP, vv);
    __syncthreads();
    f32x4 s[NS];
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < DP; kk += 32) {
#pragma unroll
      for (int nb = 0; nb < NS; ++nb) s[nb] = mma32<T, false>(Qs, ld, 16 * wave, kk, Ks, ld, 16 * nb, kk, s[nb]);
    }
    // lane: key k0 + 16 nb + col, queries 4 kg + i.  Keys beyond L leave the softmax
    float mx[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) {
      const bool valid = k0 + 16 * nb + col < L;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float sv = valid ? s[nb][i] * scale : -INFINITY;
        s[nb][i] = sv;
        mx[i] = fmaxf(mx[i], sv);
      }
    }
    float al[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float mn = fmaxf(m[i], group16_max(mx[i]));     // finite: key k0 of every tile is < L
      al[i] = expf(m[i] - mn);                              // 0 on the first tile
      m[i] = mn;
      l[i] *= al[i];
    }
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = expf(s[nb][i] - m[i]);
        l[i] += p;                                          // this lane's keys; the 16 lanes of a row are added at the end
        DT<T>::st(Pw + (4 * kg + i) * LDP + 16 * nb + col, p);
      }
    }
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[db][i] *= al[i];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < TS; ks += 32) {
#pragma unroll
      for (int db = 0; db < NDB; ++db)
        if (db < ndb) acc[db] = mma32<T, true>(Pw, LDP, 0, ks, Vs, ld, 16 * db, ks, acc[db]);
    }
  }
  // lane: channel 16 db + col, queries q0 + 16 wave + 4 kg + i
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qi = q0 + 16 * wave + 4 * kg + i;
    const float lt = group16_sum(l[i]);
    if (qi >= L) continue;
    const float inv = 1.0f / lt;
    T* op = o + (tok0 + qi) * o_ld + h * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int c = 16 * db + col;
      if (db < ndb && c < D) DT<T>::st(op + c, acc[db][i] * inv);
    }
    if (lse != nullptr && col == 0) lse[((long)b * H + h) * L + qi] = m[i] + logf(lt);
  }
}

// ---- backward: dQ -------------------------------------------------------------------------------------------------------------------------
// grid (query tiles, H, B).  LDS: Qs[TQ][ld] dOs[TQ][ld] Ks[TS][ld] Vs[TS][ld] Ps[4][16][LDP] lse_s[TQ] del_s[TQ]
template <typename T, int NDB>
__global__ __launch_bounds__(NT) void attn_dq_kernel(const T* __restrict__ q, long q_ld, const T* __restrict__ k, long k_ld, const T* __restrict__ v,
                                                     long v_ld, const T* __restrict__ o, long o_ld, const T* __restrict__ dout, long do_ld,
                                                     const float* __restrict__ lse, T* __restrict__ dq, long dq_ld, int L, int H, int D, int DP,
                                                     float scale, int vq, int vk, int vv, int vdo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  constexpr int TS = Cfg<T>::TS, NS = TS / 16, LDP = Cfg<T>::LDP;
  const int ld = DP + Cfg<T>::PAD;
  T* Qs = reinterpret_cast<T*>(attn_smem);
  T* dOs = Qs + TQ * ld;
  T* Ks = dOs + TQ * ld;
  T* Vs = Ks + TS * ld;
  T* Ps = Vs + TS * ld;
  float* lse_s = reinterpret_cast<float*>(Ps + 4 * 16 * LDP);
  float* del_s = lse_s + TQ;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, col = lane & 15, kg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * TQ;
  const long tok0 = (long)b * L;
  const int ndb = (D + 15) >> 4;
  T* Pw = Ps + wave * 16 * LDP;
  stage<T>(Qs, ld, q + tok0 * q_ld + h * D, q_ld, q0, TQ, L, D, DP, vq);
  stage<T>(dOs, ld, dout + tok0 * do_ld + h * D, do_ld, q0, TQ, L, D, DP, vdo);
  __syncthreads();
  stage_rowconst<T>(lse_s, del_s, dOs, ld, o + tok0 * o_ld + h * D, o_ld, lse + ((long)b * H + h) * L, q0, TQ, L, D);
  f32x4 acc[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < L; k0 += TS) {
    __syncthreads();
    stage<T>(Ks, ld, k + tok0 * k_ld + h * D, k_ld, k0, TS, L, D, DP, vk);
    stage<T>(Vs, ld, v + tok0 * v_ld + h * D, v_ld, k0, TS, L, D, DP, vv);
    __syncthreads();
    f32x4 s[NS], dp[NS];
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) {
      s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int kk = 0; kk < DP; kk += 32) {
#pragma unroll
      for (int nb = 0; nb < NS; ++nb) {
        s[nb] = mma32<T, false>(Qs, ld, 16 * wave, kk, Ks, ld, 16 * nb, kk, s[nb]);
        dp[nb] = mma32<T, false>(dOs, ld, 16 * wave, kk, Vs, ld, 16 * nb, kk, dp[nb]);
      }
    }
    // lane: key k0 + 16 nb + col, queries 16 wave + 4 kg + i
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) {
      const bool valid = k0 + 16 * nb + col < L;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = 16 * wave + 4 * kg + i;
        const float p = valid ? expf(s[nb][i] * scale - lse_s[r]) : 0.f;
        DT<T>::st(Pw + (4 * kg + i) * LDP + 16 * nb + col, p * (dp[nb][i] - del_s[r]));
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < TS; ks += 32) {
#pragma unroll
      for (int db = 0; db < NDB; ++db)
        if (db < ndb) acc[db] = mma32<T, true>(Pw, LDP, 0, ks, Ks, ld, 16 * db, ks, acc[db]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int qi = q0 + 16 * wave + 4 * kg + i;
    if (qi >= L) continue;
    T* gp = dq + (tok0 + qi) * dq_ld + h * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int c = 16 * db + col;
      if (db < ndb && c < D) DT<T>::st(gp + c, acc[db][i] * scale);
    }
  }
}

// ---- backward: dK, dV ---------------------------------------------------------------------------------------------------------------------
// grid (key tiles, H, B).  LDS: Ks[TQ][ld] Vs[TQ][ld] Qs[TS][ld] dOs[TS][ld] Pt[4][16][LDP] St[4][16][LDP] lse_s[TS] del_s[TS]
template <typename T, int NDB>
__global__ __launch_bounds__(NT) void attn_dkv_kernel(const T* __restrict__ q, long q_ld, const T* __restrict__ k, long k_ld, const T* __restrict__ v,
                                                      long v_ld, const T* __restrict__ o, long o_ld, const T* __restrict__ dout, long do_ld,
                                                      const float* __restrict__ lse, T* __restrict__ dk, long dk_ld, T* __restrict__ dv, long dv_ld,
                                                      int L, int H, int D, int DP, float scale, int vq, int vk, int vv, int vdo) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
  constexpr int TS = Cfg<T>::TS, NS = TS / 16, LDP = Cfg<T>::LDP;
  const int ld = DP + Cfg<T>::PAD;
  T* Ks = reinterpret_cast<T*>(attn_smem);
  T* Vs = Ks + TQ * ld;
  T* Qs = Vs + TQ * ld;
  T* dOs = Qs + TS * ld;
  T* Pt = dOs + TS * ld;
  T* St = Pt + 4 * 16 * LDP;
  float* lse_s = reinterpret_cast<float*>(St + 4 * 16 * LDP);
  float* del_s = lse_s + TS;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63, col = lane & 15, kg = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * TQ;
  const long tok0 = (long)b * L;
  const int ndb = (D + 15) >> 4;
  T* Pw = Pt + wave * 16 * LDP;
  T* Sw = St + wave * 16 * LDP;
  stage<T>(Ks, ld, k + tok0 * k_ld + h * D, k_ld, k0, TQ, L, D, DP, vk);
  stage<T>(Vs, ld, v + tok0 * v_ld + h * D, v_ld, k0, TQ, L, D, DP, vv);
  f32x4 ak[NDB], av[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    ak[db] = f32x4{0.f, 0.f, 0.f, 0.f};
    av[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int q0 = 0; q0 < L; q0 += TS) {
    __syncthreads();
    stage<T>(Qs, ld, q + tok0 * q_ld + h * D, q_ld, q0, TS, L, D, DP, vq);
    stage<T>(dOs, ld, dout + tok0 * do_ld + h * D, do_ld, q0, TS, L, D, DP, vdo);
    __syncthreads();
    stage_rowconst<T>(lse_s, del_s, dOs, ld, o + tok0 * o_ld + h * D, o_ld, lse + ((long)b * H + h) * L, q0, TS, L, D);
    // S^T and dP^T: rows = this wave's keys, columns = the tile's queries
    f32x4 s[NS], dp[NS];
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) {
      s[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int kk = 0; kk < DP; kk += 32) {
#pragma unroll
      for (int nb = 0; nb < NS; ++nb) {
        s[nb] = mma32<T, false>(Ks, ld, 16 * wave, kk, Qs, ld, 16 * nb, kk, s[nb]);
        dp[nb] = mma32<T, false>(Vs, ld, 16 * wave, kk, dOs, ld, 16 * nb, kk, dp[nb]);
      }
    }
    __syncthreads();                                        // lse_s / del_s are written
    // lane: query q0 + 16 nb + col, keys k0 + 16 wave + 4 kg + i
#pragma unroll
    for (int nb = 0; nb < NS; ++nb) {
      const int r = 16 * nb + col;
      const bool qlive = q0 + r < L;
      const float ls = lse_s[r], de = del_s[r];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool valid = qlive && (k0 + 16 * wave + 4 * kg + i < L);
        const float p = valid ? expf(s[nb][i] * scale - ls) : 0.f;
        DT<T>::st(Pw + (4 * kg + i) * LDP + r, p);
        DT<T>::st(Sw + (4 * kg + i) * LDP + r, p * (dp[nb][i] - de));
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < TS; ks += 32) {
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        if (db < ndb) {
          av[db] = mma32<T, true>(Pw, LDP, 0, ks, dOs, ld, 16 * db, ks, av[db]);
          ak[db] = mma32<T, true>(Sw, LDP, 0, ks, Qs, ld, 16 * db, ks, ak[db]);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int ki = k0 + 16 * wave + 4 * kg + i;
    if (ki >= L) continue;
    T* gk = dk + (tok0 + ki) * dk_ld + h * D;
    T* gv = dv + (tok0 + ki) * dv_ld + h * D;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const int c = 16 * db + col;
      if (db < ndb && c < D) {
        DT<T>::st(gk + c, ak[db][i] * scale);
        DT<T>::st(gv + c, av[db][i]);
      }
    }
  }
}

int check_shape(const char* who, int B, int L, int H, int D) {
  DY_CHECK(B > 0 && L > 0 && H > 0 && B <= 65535 && H <= 65535 && (long)B * L < (1L << 31), "%s: bad shape B=%d L=%d H=%d", who, B, L, H);
  DY_CHECK(D >= 8 && D <= 128 && D % 8 == 0, "%s: head dim D=%d is outside the rule D %% 8 == 0, 8 <= D <= 128", who, D);
  return 0;
}

template <typename T> int lds_bytes(int DP, int own_imgs, int swept_imgs, int p_imgs, int row_consts) {
  const int ld = DP + Cfg<T>::PAD;
  return (int)sizeof(T) * ((own_imgs * TQ + swept_imgs * Cfg<T>::TS) * ld + p_imgs * 4 * 16 * Cfg<T>::LDP) + 8 * row_consts;
}

// the kernels are instantiated per padded head dim DP = 32 / 64 / 96 / 128 (NDB = DP / 16 accumulator blocks of 16 channels): the
// accumulators, and with them the occupancy, follow the head dim.  f is called with std::integral_constant<int, NDB>
template <typename F> void with_blocks(int DP, F&& f) {
  if (DP <= 32) f(std::integral_constant<int, 2>{});
  else if (DP <= 64) f(std::integral_constant<int, 4>{});
  else if (DP <= 96) f(std::integral_constant<int, 6>{});
  else f(std::integral_constant<int, 8>{});
}

}  // namespace

// reference transformer.py:115 (nn.MultiheadAttention inside TransformerLayer.forward): torch's multi_head_attention_forward between
// its in-projection and out_proj, dropout 0, no masks
extern "C" int dy_attn_fwd(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, void* o, int64_t o_ld, float* lse, int B,
                           int L, int H, int D, float scale, int dtype, void* stream) {
  if (int e = check_shape("dy_attn_fwd", B, L, H, D)) return e;
  if (int e = dy_check_lanes("dy_attn_fwd(q)", q, q_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_fwd(k)", k, k_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_fwd(v)", v, v_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_fwd(o)", o, o_ld, H * D, dtype)) return e;
  const int es = dy_elem_size(dtype), DP = (D + 31) / 32 * 32;
  const int vq = dy_aligned16(q, q_ld, es), vk = dy_aligned16(k, k_ld, es), vv = dy_aligned16(v, v_ld, es);
  const dim3 grid((unsigned)((L + TQ - 1) / TQ), (unsigned)H, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("attn_fwd_kernel");
  int rc = 0;
  DY_DISPATCH_DTYPE("dy_attn_fwd", dtype, with_blocks(DP, [&](auto nb) {
    constexpr int NDB = decltype(nb)::value;
    const int shm = lds_bytes<T>(DP, 1, 2, 1, 0);
    rc = dy_raise_lds_limit("dy_attn_fwd", {{&attn_fwd_kernel<T, NDB>, lds_bytes<T>(16 * NDB, 1, 2, 1, 0)}});
    if (rc == 0)
      attn_fwd_kernel<T, NDB><<<grid, NT, shm, st>>>((const T*)q, q_ld, (const T*)k, k_ld, (const T*)v, v_ld, (T*)o, o_ld, lse, L, H, D, DP, scale, vq, vk, vv);
  }));
  if (rc) return rc;
  DY_LAUNCH_CHECK();
  return 0;
}

// the backward of the call above (transformer.py:115 under autograd): dQ, dK, dV from dO, flash form, deterministic
extern "C" int dy_attn_bwd(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, const void* o, int64_t o_ld,
                           const void* dout, int64_t do_ld, const float* lse, void* dq, int64_t dq_ld, void* dk, int64_t dk_ld, void* dv, int64_t dv_ld,
                           int B, int L, int H, int D, float scale, int dtype, void* stream) {
  if (int e = check_shape("dy_attn_bwd", B, L, H, D)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(q)", q, q_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(k)", k, k_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(v)", v, v_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(o)", o, o_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(do)", dout, do_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(dq)", dq, dq_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(dk)", dk, dk_ld, H * D, dtype)) return e;
  if (int e = dy_check_lanes("dy_attn_bwd(dv)", dv, dv_ld, H * D, dtype)) return e;
  DY_CHECK(lse != nullptr, "dy_attn_bwd: the forward's LSE is needed");
  const int es = dy_elem_size(dtype), DP = (D + 31) / 32 * 32;
  const int vq = dy_aligned16(q, q_ld, es), vk = dy_aligned16(k, k_ld, es), vv = dy_aligned16(v, v_ld, es), vdo = dy_aligned16(dout, do_ld, es);
  const dim3 grid((unsigned)((L + TQ - 1) / TQ), (unsigned)H, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  dy_note_kernel("attn_dq_kernel");
  DY_DISPATCH_DTYPE("dy_attn_bwd", dtype, with_blocks(DP, [&](auto nb) {
    constexpr int NDB = decltype(nb)::value;
    const int shm = lds_bytes<T>(DP, 2, 2, 1, TQ);
    rc = dy_raise_lds_limit("dy_attn_bwd", {{&attn_dq_kernel<T, NDB>, lds_bytes<T>(16 * NDB, 2, 2, 1, TQ)},
                                            {&attn_dkv_kernel<T, NDB>, lds_bytes<T>(16 * NDB, 2, 2, 2, Cfg<T>::TS)}});
    if (rc == 0)
      attn_dq_kernel<T, NDB><<<grid, NT, shm, st>>>((const T*)q, q_ld, (const T*)k, k_ld, (const T*)v, v_ld, (const T*)o, o_ld, (const T*)dout, do_ld, lse,
                                                    (T*)dq, dq_ld, L, H, D, DP, scale, vq, vk, vv, vdo);
  }));
  if (rc) return rc;
  DY_LAUNCH_CHECK();
  dy_note_kernel("attn_dkv_kernel");
  DY_DISPATCH_DTYPE("dy_attn_bwd", dtype, with_blocks(DP, [&](auto nb) {
    constexpr int NDB = decltype(nb)::value;
    const int shm = lds_bytes<T>(DP, 2, 2, 2, Cfg<T>::TS);
    attn_dkv_kernel<T, NDB><<<grid, NT, shm, st>>>((const T*)q, q_ld, (const T*)k, k_ld, (const T*)v, v_ld, (const T*)o, o_ld, (const T*)dout, do_ld, lse,
                                                   (T*)dk, dk_ld, (T*)dv, dv_ld, L, H, D, DP, scale, vq, vk, vv, vdo);
  }));
  DY_LAUNCH_CHECK();
  return 0;
}
