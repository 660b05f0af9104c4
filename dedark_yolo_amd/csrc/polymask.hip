// Ground-truth instance masks of the segment task, rasterised on the device from the augmented polygons.
//
// Reference (host, per sample, in the dataloader workers): ultralytics/data/utils.py:137-155 polygon2mask (cv2.fillPoly at the input
// resolution, then cv2.resize by 1 / mask_ratio), :158-170 polygons2masks, :173-190 polygons2masks_overlap (areas, argsort, the overlap
// index map), called from Format._format_segments (ultralytics/data/augment.py:753-764).
//
// cv2 is not part of the reference, so the pixel rule is the project's stated one ("Polygon masks"):
//   * full-resolution pixel (x, y) is set iff the integer point (x, y) lies in the CLOSED polygon: inside by the even-odd rule or on
//     one of its edges (closing edge included) -- all in integer arithmetic;
//   * the mask at ratio r is cv2.resize(INTER_LINEAR) of that 0/1 plane, which for even r is "at least 2 of the 4 taps set" with tap
//     rows / columns r i + r / 2 - 1 and r i + r / 2 (r == 1: the plane itself).  Only the tap rows are rasterised.
//
// Schedule: one workgroup per (instance, band of mask rows); the P vertices are staged once in LDS; one wave per mask row walks the
// edges (64 per pass) and records, per tap row, in a row bitmap in LDS
//   * one parity toggle per edge that crosses the row, at the first pixel not left of the crossing (integer ceiling division), and
//   * the pixels that lie exactly on an edge;
// a prefix XOR over the toggle bitmap (in-word shifts + a ballot for the carry between the <= 64 words) gives the even-odd interior.
// Integer LDS atomics (xor / or) only, so the result does not depend on the order of the edges.  Areas are integer counts (atomicAdd on
// int32): no float atomics anywhere, identical bytes from run to run.
#include "dy_common.h"

namespace {

constexpr int PM_NT = 256;            // 4 waves
constexpr int PM_WAVES = PM_NT / 64;
constexpr int PM_MAX_P = 4096;        // vertices per polygon staged in LDS (16 KiB)
constexpr int PM_MAX_WORDS = 64;      // 32-pixel words per row: one per lane -> width <= 2048
constexpr int PM_ROWS = 16;           // mask rows per workgroup
constexpr int PM_MAX_INST = 255;      // instances per image of the uint8 overlap map

__device__ inline void pm_edge(uint32_t* tog, uint32_t* edg, int x0, int y0, int x1, int y1, int y, int w) {
  if (y0 == y1) {                                            // horizontal (or repeated vertex): the closed span on its own row
    if (y0 != y) return;
    int xa = min(x0, x1), xb = max(x0, x1);
    xa = max(xa, 0);
    xb = min(xb, w - 1);
    if (xa > xb) return;
    for (int wd = xa >> 5; wd <= (xb >> 5); ++wd) {
      const int lo = max(xa - wd * 32, 0), hi = min(xb - wd * 32, 31);
      const uint32_t m = (hi == 31 ? 0xffffffffu : ((1u << (hi + 1)) - 1u)) & ~((1u << lo) - 1u);
      atomicOr(&edg[wd], m);
    }
    return;
  }
  if (y < min(y0, y1) || y > max(y0, y1)) return;
  long long dy = (long long)y1 - y0, num = ((long long)y - y0) * ((long long)x1 - x0);
  if (dy < 0) { dy = -dy; num = -num; }
  const long long q = num / dy, rem = num % dy;              // truncating division: q == ceil for num < 0, floor for num > 0
  if (rem == 0) {                                            // the row meets the edge in an integer point
    const long long x = x0 + q;
    if (x >= 0 && x < w) atomicOr(&edg[(int)x >> 5], 1u << ((int)x & 31));
  }
  if ((y0 > y) != (y1 > y)) {                                // half-open crossing rule: every pixel x < crossing changes parity
    long long k = x0 + q + (rem > 0 ? 1 : 0);                 // ceil(crossing): pixels [0, k) toggle
    if (k < 0) k = 0;
    if (k < w) atomicXor(&tog[(int)k >> 5], 1u << ((int)k & 31));   // k >= w: toggles the whole row == no bit in the prefix form
  }
}

// planes [n_total][mh][mw] 0/1, area[n] += set pixels (area zeroed by the caller)
__global__ __launch_bounds__(PM_NT) void polymask_raster_kernel(const uint32_t* __restrict__ polys, int P, int h, int w, int r,
                                                                uint8_t* __restrict__ planes, int* __restrict__ area) {
  __shared__ uint32_t vtx[PM_MAX_P];
  __shared__ uint32_t tog[PM_WAVES][2][PM_MAX_WORDS];
  __shared__ uint32_t edg[PM_WAVES][2][PM_MAX_WORDS];
  const int n = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mh = h / r, mw = w / r, words = (w + 31) >> 5, ntap = r == 1 ? 1 : 2;
  const uint32_t* poly = polys + (long)n * P;
  for (int e = threadIdx.x; e < P; e += PM_NT) vtx[e] = poly[e];
  int count = 0;
  for (int it = 0; it < PM_ROWS / PM_WAVES; ++it) {           // uniform trip count: every wave reaches every barrier
    const int i = blockIdx.y * PM_ROWS + it * PM_WAVES + wave;
    const bool active = i < mh;
    const int ybase = r == 1 ? i : r * i + r / 2 - 1;
    tog[wave][0][lane] = 0; tog[wave][1][lane] = 0;
    edg[wave][0][lane] = 0; edg[wave][1][lane] = 0;
    __syncthreads();
    if (active) {
      for (int e = lane; e < P; e += 64) {
        const uint32_t a = vtx[e], b = vtx[e + 1 == P ? 0 : e + 1];
        const int x0 = (int16_t)(a & 0xffff), y0 = (int16_t)(a >> 16), x1 = (int16_t)(b & 0xffff), y1 = (int16_t)(b >> 16);
        for (int t = 0; t < ntap; ++t) pm_edge(tog[wave][t], edg[wave][t], x0, y0, x1, y1, ybase + t, w);
      }
    }
    __syncthreads();
    for (int t = 0; t < 2; ++t) {                             // prefix XOR of the toggles: bit x = parity of pixel x
      uint32_t v = lane < words ? tog[wave][t][lane] : 0u;
      v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16;
      const unsigned long long odd = __ballot(v >> 31);        // words whose own toggles are odd in number
      if (__popcll(odd & ((1ull << lane) - 1ull)) & 1) v = ~v;
      tog[wave][t][lane] = v | edg[wave][t][lane];
    }
    __syncthreads();
    if (active) {
      const uint32_t* f0 = tog[wave][0];
      const uint32_t* f1 = tog[wave][1];
      for (int j = lane; j < mw; j += 64) {
        int on;
        if (r == 1) {
          on = (f0[j >> 5] >> (j & 31)) & 1;
        } else {
          const int c0 = r * j + r / 2 - 1, c1 = c0 + 1;
          const int taps = ((f0[c0 >> 5] >> (c0 & 31)) & 1) + ((f0[c1 >> 5] >> (c1 & 31)) & 1) + ((f1[c0 >> 5] >> (c0 & 31)) & 1) +
                           ((f1[c1 >> 5] >> (c1 & 31)) & 1);
          on = taps >= 2;
        }
        planes[((long)n * mh + i) * mw + j] = (uint8_t)on;
        count += on;
      }
    }
    __syncthreads();
  }
  for (int o = 32; o > 0; o >>= 1) count += __shfl_down(count, o, 64);
  if (lane == 0 && count) atomicAdd(&area[n], count);
}

// per image: rank by (area descending, index ascending); block x == 0 also writes the permutation and the permuted label rows
__global__ __launch_bounds__(PM_NT) void polymask_compose_kernel(const uint8_t* __restrict__ planes, const int* __restrict__ area,
                                                                 const int* __restrict__ offsets, int n_total, long hw,
                                                                 const float* __restrict__ rows_in, float* __restrict__ rows_out,
                                                                 int* __restrict__ perm, uint8_t* __restrict__ masks) {
  __shared__ int ar[PM_NT];
  __shared__ int rank[PM_NT];
  const int b = blockIdx.y, t = threadIdx.x;
  int off = offsets[b], n = offsets[b + 1] - off;
  off = min(max(off, 0), n_total);                            // the table is host data: never index past the arrays whatever it holds
  n = min(max(n, 0), min(PM_MAX_INST, n_total - off));
  if (t < n) ar[t] = area[off + t];
  __syncthreads();
  if (t < n) {
    int rk = 0;
    for (int k = 0; k < n; ++k) rk += (ar[k] > ar[t]) || (ar[k] == ar[t] && k < t);
    rank[t] = rk;
    if (blockIdx.x == 0) {
      perm[off + rk] = t;
      for (int c = 0; c < 6; ++c) rows_out[(long)(off + rk) * 6 + c] = rows_in[(long)(off + t) * 6 + c];
    }
  }
  __syncthreads();
  const long pix = (long)blockIdx.x * PM_NT + t;
  if (pix >= hw) return;
  int v = 0;
  for (int j = 0; j < n; ++j)
    if (planes[(long)(off + j) * hw + pix]) v = max(v, rank[j] + 1);
  masks[(long)b * hw + pix] = (uint8_t)v;
}

}  // namespace

extern "C" int dy_polymask_raster(const int16_t* polys, int n_total, int P, int h, int w, int ratio, uint8_t* planes, int32_t* area,
                                  void* stream) {
  DY_CHECK(n_total >= 0 && P >= 1 && P <= PM_MAX_P, "dy_polymask_raster: P=%d outside [1, %d]", P, PM_MAX_P);
  DY_CHECK(h > 0 && w > 0 && w <= 32 * PM_MAX_WORDS && h <= 32767, "dy_polymask_raster: plane %dx%d (width <= %d)", h, w, 32 * PM_MAX_WORDS);
  DY_CHECK(ratio == 1 || (ratio > 0 && ratio % 2 == 0), "dy_polymask_raster: mask_ratio %d (1 or even)", ratio);
  DY_CHECK(h % ratio == 0 && w % ratio == 0, "dy_polymask_raster: %dx%d is not a multiple of mask_ratio %d", h, w, ratio);
  if (n_total == 0) return 0;
  DY_CHECK(polys && planes && area, "dy_polymask_raster: null pointer");
  DY_CHECK(((uintptr_t)polys) % 4 == 0, "dy_polymask_raster: polygons must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(area, 0, sizeof(int32_t) * (size_t)n_total, st) != hipSuccess) {
    dy_set_error("dy_polymask_raster: hipMemsetAsync failed");
    return 2;
  }
  dim3 grid(n_total, dy_cdiv(h / ratio, PM_ROWS));
  dy_note_kernel("polymask_raster_kernel");
  polymask_raster_kernel<<<grid, PM_NT, 0, st>>>((const uint32_t*)polys, P, h, w, ratio, planes, area);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_polymask_compose(const uint8_t* planes, const int32_t* area, const int32_t* offsets, int B, int n_total, int mh, int mw,
                                   const float* rows_in, float* rows_out, int32_t* perm, uint8_t* masks, void* stream) {
  DY_CHECK(B > 0 && n_total >= 0 && mh > 0 && mw > 0, "dy_polymask_compose: bad geometry");
  DY_CHECK(offsets && masks, "dy_polymask_compose: null pointer");
  DY_CHECK(n_total == 0 || (planes && area && rows_in && rows_out && perm), "dy_polymask_compose: null pointer");
  DY_CHECK(B <= 65535, "dy_polymask_compose: B=%d", B);
  dim3 grid(dy_cdiv((long)mh * mw, PM_NT), B);
  dy_note_kernel("polymask_compose_kernel");
  polymask_compose_kernel<<<grid, PM_NT, 0, (hipStream_t)stream>>>(planes, area, offsets, n_total, (long)mh * mw, rows_in, rows_out, perm, masks);
  DY_LAUNCH_CHECK();
  return 0;
}
