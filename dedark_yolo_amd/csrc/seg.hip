// Segment task: mask loss over the prototype map and the bias pieces of the Proto's ConvTranspose2d(k=2, s=2).
// Replaces v8SegmentationLoss's mask term (reference ultralytics/utils/loss.py:252-288, single_mask_loss, crop_mask of
// ultralytics/utils/ops.py:553-569, the nearest resize of F.interpolate) and ConvTranspose2d's bias and bias gradient.
//
// The mask loss runs per positive anchor p of image i (fg_mask from the HIP assigner, utils/loss.py:assign):
//   z(pix)  = c_p . P_i[pix]                                    c_p: the anchor's nm mask coefficients, P_i: image i's proto map
//   l_p     = sum over pix inside the crop box of BCEwithLogits(z, gt) / (mh*mw) / area_p
//   item    = hyp_box / B * sum_i mean_{p in i} l_p
// Every sum has a fixed order (in-block trees, per-image sequential sums): no float atomics, two runs agree bit for bit.  The
// positive counts stay on the device; nothing here synchronises with the host.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NM = 32;          // mask coefficients per anchor (Segment's nm; the only value the reference's yamls use)
constexpr int NT = 256;         // threads per block
constexpr int CHUNK = 64;       // positives staged in LDS at a time by the proto-gradient kernel

struct Seg {
  const char* mc; long mc_ld;           // [B][A][mc_ld] compute dtype
  const char* proto; long proto_ld;     // [B][mh][mw][proto_ld]
  int B, A, mh, mw;
  const int32_t* tgi; const uint8_t* fg; const float* tbox;
  const void* masks; int mask_i32, mask_h, mask_w, overlap;
  const int32_t* gt_rows; int n_max;
  float img_h, img_w;
  const int32_t* pos; const int32_t* npos;
};

Seg seg_of(const dy_seg_desc* d) {
  Seg s;
  s.mc = (const char*)d->mc; s.mc_ld = d->mc_ld; s.proto = (const char*)d->proto; s.proto_ld = d->proto_ld;
  s.B = d->B; s.A = d->A; s.mh = d->mh; s.mw = d->mw;
  s.tgi = d->target_gt_idx; s.fg = d->fg_mask; s.tbox = d->target_box;
  s.masks = d->masks; s.mask_i32 = d->mask_dtype; s.mask_h = d->mask_h; s.mask_w = d->mask_w; s.overlap = d->overlap;
  s.gt_rows = d->gt_rows; s.n_max = d->n_max; s.img_h = d->img_h; s.img_w = d->img_w;
  s.pos = d->pos; s.npos = d->npos;
  return s;
}

// crop box of one positive in proto pixels: columns [x0, x1), rows [y0, y1) (crop_mask keeps x1 <= r < x2 with the box
// xyxy / imgsz * (mw, mh) computed in f32 in this order), and the normalised box area of the reference's marea
struct Box { int x0, x1, y0, y1; float area; };

__device__ inline Box crop_box(const Seg& s, int b, int a) {
  const float* t = s.tbox + ((long)b * s.A + a) * 4;
  const float x1n = __fdiv_rn(t[0], s.img_w), y1n = __fdiv_rn(t[1], s.img_h);
  const float x2n = __fdiv_rn(t[2], s.img_w), y2n = __fdiv_rn(t[3], s.img_h);
  Box r;
  r.area = __fmul_rn(__fsub_rn(x2n, x1n), __fsub_rn(y2n, y1n));
  const float fw = (float)s.mw, fh = (float)s.mh;
  // integer r satisfies r >= x  <=>  r >= ceil(x), and r < x  <=>  r < ceil(x)
  r.x0 = (int)fminf(fmaxf(ceilf(__fmul_rn(x1n, fw)), 0.f), fw);
  r.x1 = (int)fminf(fmaxf(ceilf(__fmul_rn(x2n, fw)), 0.f), fw);
  r.y0 = (int)fminf(fmaxf(ceilf(__fmul_rn(y1n, fh)), 0.f), fh);
  r.y1 = (int)fminf(fmaxf(ceilf(__fmul_rn(y2n, fh)), 0.f), fh);
  if (r.x1 < r.x0) r.x1 = r.x0;
  if (r.y1 < r.y0) r.y1 = r.y0;
  return r;
}

// F.interpolate(mode='nearest') source index (ATen nearest_idx: scale = in / out in f32, floor(dst * scale), clamped)
__device__ inline int nearest_src(int o, int in, int out) {
  if (in == out) return o;
  const float sc = (float)in / (float)out;
  const int v = (int)floorf((float)o * sc);
  return v < in - 1 ? v : in - 1;
}

// gt mask plane of positive (b, gt g): a pointer to its [mask_h][mask_w] plane and the value that means "inside"
// (overlap maps: k + 1 for gt k; per-instance planes: read as the target value itself, key = -1)
struct GtRef { long plane; int key; };

__device__ inline GtRef gt_ref(const Seg& s, int b, int g) {
  GtRef r;
  if (s.overlap) { r.plane = b; r.key = g + 1; }
  else {
    const int row = (g >= 0 && g < s.n_max) ? s.gt_rows[(long)b * s.n_max + g] : -1;
    r.plane = row; r.key = -1;
  }
  return r;
}

__device__ inline float gt_at(const Seg& s, const GtRef& r, int y, int x) {
  if (r.plane < 0) return 0.f;
  const int sy = nearest_src(y, s.mask_h, s.mh), sx = nearest_src(x, s.mask_w, s.mw);
  const long o = (r.plane * s.mask_h + sy) * (long)s.mask_w + sx;
  const int v = s.mask_i32 ? ((const int32_t*)s.masks)[o] : (int)((const uint8_t*)s.masks)[o];
  if (r.key >= 0) return v == r.key ? 1.f : 0.f;
  return (float)v;
}

template <typename T>
__device__ inline void load_nm(const T* p, float* out) {
#pragma unroll
  for (int k = 0; k < NM; k += DT<T>::VE) ldvec<T>(p + k, out + k);
}

// BCEWithLogits(z, t) = (1 - t) z + softplus(-z), softplus(-z) = max(-z, 0) + log1p(exp(-|z|))
__device__ inline float bce_logits(float z, float t) {
  return (1.f - t) * z + fmaxf(-z, 0.f) + log1pf(expf(-fabsf(z)));
}

__device__ inline float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// fixed-order block sum of one float per thread (NT threads); every thread gets the result
__device__ inline float block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// ---- positives per image, in anchor order --------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void seg_positives_kernel(const uint8_t* __restrict__ fg, int A, int32_t* __restrict__ pos,
                                                           int32_t* __restrict__ npos) {
  constexpr int NW = NT / 64;
  __shared__ int wtot[NW];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint8_t* f = fg + (long)b * A;
  int32_t* out = pos + (long)b * A;
  int base = 0;
  for (int a0 = 0; a0 < A; a0 += NT) {
    const int a = a0 + threadIdx.x;
    const bool on = a < A && f[a];
    const unsigned long long m = __ballot(on);
    if (lane == 0) wtot[wave] = __popcll(m);
    __syncthreads();
    int off = base;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    if (on) out[off + __popcll(m & ((1ull << lane) - 1ull))] = a;
    for (int w = 0; w < NW; ++w) base += wtot[w];
    __syncthreads();
  }
  if (threadIdx.x == 0) npos[b] = base;
}

// row of gt j of image b in a per-instance mask stack [N][h][w]: the j-th row with batch_idx == b (v8SegmentationLoss:
// masks[batch_idx == i][mask_idx]); -1 where image b has fewer rows
__global__ void seg_gt_rows_kernel(const float* __restrict__ bidx, int n, int B, int n_max, int32_t* __restrict__ rows) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int32_t* r = rows + (long)b * n_max;
  int j = 0;
  for (int t = 0; t < n && j < n_max; ++t)
    if ((int)bidx[t] == b) r[j++] = t;
  for (; j < n_max; ++j) r[j] = -1;
}

// ---- forward: per-positive loss l_p (grid-stride over the image's positives) ----------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void seg_loss_fwd_kernel(Seg s, float* __restrict__ lossp) {
  __shared__ float red[NT];
  __shared__ float c[NM];
  const int b = blockIdx.y;
  const int np = s.npos[b];
  for (int slot = blockIdx.x; slot < np; slot += gridDim.x) {
    const int a = s.pos[(long)b * s.A + slot];
    if (threadIdx.x < NM) c[threadIdx.x] = DT<T>::ld(reinterpret_cast<const T*>(s.mc) + ((long)b * s.A + a) * s.mc_ld + threadIdx.x);
    __syncthreads();
    const Box bx = crop_box(s, b, a);
    const GtRef g = gt_ref(s, b, s.tgi[(long)b * s.A + a]);
    const int bw = bx.x1 - bx.x0, n = bw * (bx.y1 - bx.y0);
    float acc = 0.f;
    for (int q = threadIdx.x; q < n; q += NT) {
      const int y = bx.y0 + q / bw, x = bx.x0 + q % bw;
      float pv[NM];
      load_nm<T>(reinterpret_cast<const T*>(s.proto) + (((long)b * s.mh + y) * s.mw + x) * s.proto_ld, pv);
      float z = 0.f;
#pragma unroll
      for (int k = 0; k < NM; ++k) z = fmaf(c[k], pv[k], z);
      acc += bce_logits(z, gt_at(s, g, y, x));
    }
    const float tot = block_sum(acc, red);
    if (threadIdx.x == 0) lossp[(long)b * s.A + slot] = tot / (float)(s.mh * s.mw) / bx.area;
    __syncthreads();
  }
}

// per image: mean of l_p over its positives (0 without positives) -> means[b]
__global__ __launch_bounds__(NT) void seg_image_mean_kernel(const float* __restrict__ lossp, const int32_t* __restrict__ npos, int A,
                                                            float* __restrict__ means) {
  __shared__ float red[NT];
  const int b = blockIdx.x, n = npos[b];
  float v = 0.f;
  for (int j = threadIdx.x; j < n; j += NT) v += lossp[(long)b * A + j];
  const float tot = block_sum(v, red);
  if (threadIdx.x == 0) means[b] = n > 0 ? tot / (float)n : 0.f;
}

// images in order; total / items of the whole criterion: det = dy_loss_finish's (total, box, cls, dfl) ->
// out = (total + seg * B, box, seg, cls, dfl)
__global__ void seg_loss_finish_kernel(const float* __restrict__ means, int B, float hyp_box, const float* __restrict__ det,
                                       float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  float sum = 0.f;
  for (int b = 0; b < B; ++b) sum += means[b];
  const float item = sum * (hyp_box / (float)B);
  out[0] = det[0] + item * (float)B;
  out[1] = det[1]; out[2] = item; out[3] = det[2]; out[4] = det[3];
}

// weight of positive (b, slot): d total / d l_p = grad * hyp_box / npos_b (the 1/(mh*mw)/area factor is applied by the caller)
__device__ inline float pos_weight(const Seg& s, int b, const float* grad_out, float hyp_box, float area) {
  return grad_out[0] * hyp_box / (float)s.npos[b] / (float)(s.mh * s.mw) / area;
}

// ---- backward 1: d mc for every positive (in-block fixed-order reduction over the crop box) ----------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void seg_loss_dmc_kernel(Seg s, const float* __restrict__ grad_out, float hyp_box, char* __restrict__ dmc,
                                                          long dmc_ld) {
  __shared__ float red[NT][NM + 1];
  __shared__ float part[NT / NM][NM];
  __shared__ float c[NM];
  const int b = blockIdx.y;
  const int np = s.npos[b];
  for (int slot = blockIdx.x; slot < np; slot += gridDim.x) {
    const int a = s.pos[(long)b * s.A + slot];
    if (threadIdx.x < NM) c[threadIdx.x] = DT<T>::ld(reinterpret_cast<const T*>(s.mc) + ((long)b * s.A + a) * s.mc_ld + threadIdx.x);
    __syncthreads();
    const Box bx = crop_box(s, b, a);
    const GtRef g = gt_ref(s, b, s.tgi[(long)b * s.A + a]);
    const float w = pos_weight(s, b, grad_out, hyp_box, bx.area);
    const int bw = bx.x1 - bx.x0, n = bw * (bx.y1 - bx.y0);
    float acc[NM];
#pragma unroll
    for (int k = 0; k < NM; ++k) acc[k] = 0.f;
    for (int q = threadIdx.x; q < n; q += NT) {
      const int y = bx.y0 + q / bw, x = bx.x0 + q % bw;
      float pv[NM];
      load_nm<T>(reinterpret_cast<const T*>(s.proto) + (((long)b * s.mh + y) * s.mw + x) * s.proto_ld, pv);
      float z = 0.f;
#pragma unroll
      for (int k = 0; k < NM; ++k) z = fmaf(c[k], pv[k], z);
      const float dz = (sigmoidf_(z) - gt_at(s, g, y, x)) * w;
#pragma unroll
      for (int k = 0; k < NM; ++k) acc[k] = fmaf(dz, pv[k], acc[k]);
    }
#pragma unroll
    for (int k = 0; k < NM; ++k) red[threadIdx.x][k] = acc[k];
    __syncthreads();
    {   // thread (part j, channel k) sums rows 32j .. 32j+31 in order, then channel k sums the 8 parts in order
      const int k = threadIdx.x % NM, j = threadIdx.x / NM;
      float v = 0.f;
      for (int r = 0; r < NT / (NT / NM); ++r) v += red[j * (NT / (NT / NM)) + r][k];
      part[j][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NM) {
      float v = 0.f;
      for (int j = 0; j < NT / NM; ++j) v += part[j][threadIdx.x];
      DT<T>::st(reinterpret_cast<T*>(dmc) + ((long)b * s.A + a) * dmc_ld + threadIdx.x, v);
    }
    __syncthreads();
  }
}

// ---- backward 2: d proto, one thread per proto pixel, the image's positives in slot order --------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void seg_loss_dproto_kernel(Seg s, const float* __restrict__ grad_out, float hyp_box,
                                                             char* __restrict__ dproto, long dproto_ld) {
  __shared__ float c[CHUNK][NM];
  __shared__ int box[CHUNK][4];
  __shared__ int key[CHUNK];
  __shared__ long plane[CHUNK];
  __shared__ float wt[CHUNK];
  const int b = blockIdx.y;
  const long HW = (long)s.mh * s.mw;
  const long pix = (long)blockIdx.x * NT + threadIdx.x;
  const bool live = pix < HW;
  const int y = live ? (int)(pix / s.mw) : 0, x = live ? (int)(pix - (long)y * s.mw) : 0;
  float pv[NM], acc[NM];
#pragma unroll
  for (int k = 0; k < NM; ++k) { pv[k] = 0.f; acc[k] = 0.f; }
  if (live) load_nm<T>(reinterpret_cast<const T*>(s.proto) + ((long)b * HW + pix) * s.proto_ld, pv);
  const int np = s.npos[b];
  for (int p0 = 0; p0 < np; p0 += CHUNK) {
    const int nc = np - p0 < CHUNK ? np - p0 : CHUNK;
    for (int e = threadIdx.x; e < nc * NM; e += NT) {
      const int j = e / NM, k = e % NM;
      const int a = s.pos[(long)b * s.A + p0 + j];
      c[j][k] = DT<T>::ld(reinterpret_cast<const T*>(s.mc) + ((long)b * s.A + a) * s.mc_ld + k);
    }
    for (int j = threadIdx.x; j < nc; j += NT) {
      const int a = s.pos[(long)b * s.A + p0 + j];
      const Box bx = crop_box(s, b, a);
      const GtRef g = gt_ref(s, b, s.tgi[(long)b * s.A + a]);
      box[j][0] = bx.x0; box[j][1] = bx.x1; box[j][2] = bx.y0; box[j][3] = bx.y1;
      key[j] = g.key; plane[j] = g.plane;
      wt[j] = pos_weight(s, b, grad_out, hyp_box, bx.area);
    }
    __syncthreads();
    if (live)
      for (int j = 0; j < nc; ++j) {
        if (x < box[j][0] || x >= box[j][1] || y < box[j][2] || y >= box[j][3]) continue;
        float z = 0.f;
#pragma unroll
        for (int k = 0; k < NM; ++k) z = fmaf(c[j][k], pv[k], z);
        GtRef g;
        g.plane = plane[j]; g.key = key[j];
        const float dz = (sigmoidf_(z) - gt_at(s, g, y, x)) * wt[j];
#pragma unroll
        for (int k = 0; k < NM; ++k) acc[k] = fmaf(dz, c[j][k], acc[k]);
      }
    __syncthreads();
  }
  if (live) {
    T* o = reinterpret_cast<T*>(dproto) + ((long)b * HW + pix) * dproto_ld;
#pragma unroll
    for (int k = 0; k < NM; k += DT<T>::VE) stvec<T>(o + k, acc + k);
  }
}

// ---- ConvTranspose2d bias ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void seg_bias_add_kernel(T* __restrict__ x, long ld, const float* __restrict__ bias, long pixels, int C) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= pixels * C) return;
  const long p = i / C;
  const int c = (int)(i - p * C);
  T* e = x + p * ld + c;
  DT<T>::st(e, DT<T>::ld(e) + bias[c]);
}

// db[c] = sum over pixels of dy[p, c]: pass 1 = per pixel chunk partial sums (pixels in order), pass 2 = chunks in order
constexpr int BG_CHUNKS = DY_BIAS_GRAD_CHUNKS;
template <typename T>
__global__ __launch_bounds__(NT) void seg_bias_grad_partial_kernel(const T* __restrict__ dy, long ld, long pixels, int C,
                                                                   float* __restrict__ part) {
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= C) return;
  const long per = (pixels + BG_CHUNKS - 1) / BG_CHUNKS;
  const long p0 = blockIdx.x * per, p1 = p0 + per < pixels ? p0 + per : pixels;
  float v = 0.f;
  for (long p = p0; p < p1; ++p) v += DT<T>::ld(dy + p * ld + c);
  part[(long)blockIdx.x * C + c] = v;
}

__global__ void seg_bias_grad_final_kernel(const float* __restrict__ part, int C, float* __restrict__ db) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  float v = 0.f;
  for (int j = 0; j < BG_CHUNKS; ++j) v += part[(long)j * C + c];
  db[c] = v;
}

// ---- validation: mask decode (process_mask, ops.py:593-623, upsample=False) ------------------------------------------------
// det rows (x1, y1, x2, y2, conf, cls, c_0 .. c_nm-1) at pixel stride det_ld; one thread per (detection, proto pixel):
// s = sigmoid(c . P) in f32, kept where s > 0.5 inside the box scaled by (sx, sy) = (mw / iw, mh / ih) (crop_mask's x1 <= r < x2)
template <typename T>
__global__ __launch_bounds__(NT) void seg_mask_decode_kernel(const T* __restrict__ proto, long proto_ld, int mh, int mw,
                                                             const float* __restrict__ det, long det_ld, const int32_t* __restrict__ det_img,
                                                             int n, float sx, float sy, uint8_t* __restrict__ out) {
  const long HW = (long)mh * mw;
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= (long)n * HW) return;
  const int j = (int)(i / HW);
  const long pix = i - (long)j * HW;
  const int y = (int)(pix / mw), x = (int)(pix - (long)y * mw);
  const float* r = det + (long)j * det_ld;
  const int b = det_img[j];
  float pv[NM];
  load_nm<T>(proto + ((long)b * HW + pix) * proto_ld, pv);
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < NM; ++k) z = fmaf(r[6 + k], pv[k], z);
  const float s = sigmoidf_(z);
  const float fx = (float)x, fy = (float)y;
  const bool in = fx >= __fmul_rn(r[0], sx) && fx < __fmul_rn(r[2], sx) && fy >= __fmul_rn(r[1], sy) && fy < __fmul_rn(r[3], sy);
  out[i] = (in && s > 0.5f) ? 1 : 0;
}

// crop_mask (ops.py:553-569) in place on f32 masks [n][h][w]
__global__ __launch_bounds__(NT) void seg_crop_mask_kernel(float* __restrict__ m, const float* __restrict__ boxes, int n, int h, int w) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  const long HW = (long)h * w;
  if (i >= (long)n * HW) return;
  const int j = (int)(i / HW);
  const long pix = i - (long)j * HW;
  const float fy = (float)(pix / w), fx = (float)(pix % w);
  const float* bx = boxes + 4L * j;
  if (!(fx >= bx[0] && fx < bx[2] && fy >= bx[1] && fy < bx[3])) m[i] = m[i] * 0.f;      // (keeps NaN a NaN, like masks * 0)
}

// ---- validation: mask IoU (metrics.py:131-147) with integer counts ----------------------------------------------------------
// gt: overlap = one index map [HW] (label k is value k + 1), else m planes [m][HW] of 0 / 1.  Per detection j (one block):
// inter[k][j] = #(pred_j & gt_k) from an LDS histogram over the gt index (overlap) or per plane (in a fixed order), area_p[j].
__global__ __launch_bounds__(NT) void seg_mask_inter_kernel(const uint8_t* __restrict__ pred, long HW, int n, const void* __restrict__ gt,
                                                            int gt_i32, int overlap, int m, int32_t* __restrict__ inter,
                                                            int32_t* __restrict__ area_p) {
  extern __shared__ int hist[];                        // m + 1 counters
  __shared__ int red[NT];
  const int j = blockIdx.x;
  const uint8_t* p = pred + (long)j * HW;
  for (int k = threadIdx.x; k <= m; k += NT) hist[k] = 0;
  __syncthreads();
  int ap = 0;
  for (long q = threadIdx.x; q < HW; q += NT) {
    if (!p[q]) continue;
    ++ap;
    if (overlap) {
      const int v = gt_i32 ? ((const int32_t*)gt)[q] : (int)((const uint8_t*)gt)[q];
      if (v >= 1 && v <= m) atomicAdd(&hist[v], 1);     // integer counts: the order does not change the result
    }
  }
  red[threadIdx.x] = ap;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) area_p[j] = red[0];
  __syncthreads();
  if (overlap) {
    for (int k = threadIdx.x; k < m; k += NT) inter[(long)k * n + j] = hist[k + 1];
    return;
  }
  for (int k = 0; k < m; ++k) {
    const uint8_t* g = (const uint8_t*)gt + (long)k * HW;
    int c = 0;
    for (long q = threadIdx.x; q < HW; q += NT) c += (p[q] && g[q]) ? 1 : 0;
    red[threadIdx.x] = c;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) inter[(long)k * n + j] = red[0];
    __syncthreads();
  }
}

// area of every gt (one block per gt), then iou[k][j] = inter / ((area_g + area_p) - inter + 1e-7) in f32
__global__ __launch_bounds__(NT) void seg_mask_iou_kernel(const void* __restrict__ gt, int gt_i32, int overlap, long HW, int m, int n,
                                                          const int32_t* __restrict__ inter, const int32_t* __restrict__ area_p,
                                                          float* __restrict__ iou) {
  __shared__ int red[NT];
  const int k = blockIdx.x;
  int c = 0;
  for (long q = threadIdx.x; q < HW; q += NT) {
    if (overlap) {
      const int v = gt_i32 ? ((const int32_t*)gt)[q] : (int)((const uint8_t*)gt)[q];
      c += v == k + 1 ? 1 : 0;
    } else {
      c += ((const uint8_t*)gt)[(long)k * HW + q] ? 1 : 0;
    }
  }
  red[threadIdx.x] = c;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float ag = (float)red[0];
  for (int j = threadIdx.x; j < n; j += NT) {
    const float in = (float)inter[(long)k * n + j];
    iou[(long)k * n + j] = in / (((ag + (float)area_p[j]) - in) + 1e-7f);
  }
}

int check_seg(const dy_seg_desc* d, const char* who) {
  DY_CHECK(d && d->mc && d->proto && d->target_gt_idx && d->fg_mask && d->target_box && d->pos && d->npos, "%s: null pointer", who);
  if (int e = dy_check_dtype(who, d->dtype)) return e;
  DY_CHECK(d->nm == NM, "%s: nm=%d (the kernels are built for %d mask coefficients)", who, d->nm, NM);
  DY_CHECK(d->B > 0 && d->A > 0 && d->mh > 0 && d->mw > 0, "%s: empty geometry", who);
  DY_CHECK(d->mc_ld >= NM && d->proto_ld >= NM, "%s: mc_ld / proto_ld below nm", who);
  const int es = dy_elem_size(d->dtype);
  DY_CHECK(dy_aligned16(d->mc, d->mc_ld, es) && dy_aligned16(d->proto, d->proto_ld, es), "%s: mc / proto rows must be 16-byte aligned", who);
  DY_CHECK(d->img_h > 0.f && d->img_w > 0.f, "%s: bad image size", who);
  DY_CHECK(d->masks != nullptr && d->mask_h > 0 && d->mask_w > 0 && (d->mask_dtype == 0 || d->mask_dtype == 1), "%s: bad gt masks", who);
  DY_CHECK(d->overlap || (d->gt_rows && d->n_max > 0), "%s: per-instance masks need gt_rows", who);
  return 0;
}

int seg_grid_x(const dy_seg_desc* d) {
  long g = (long)d->n_max * 10;                 // a gt has at most topk = 10 positives; the kernels loop past it anyway
  if (g < 1) g = 1;
  if (g > d->A) g = d->A;
  return (int)g;
}

}  // namespace

extern "C" int dy_seg_positives(const uint8_t* fg_mask, int B, int A, int32_t* pos, int32_t* npos, void* stream) {
  DY_CHECK(fg_mask && pos && npos && B > 0 && A > 0, "dy_seg_positives: bad args");
  dy_note_kernel("seg_positives_kernel");
  seg_positives_kernel<<<B, NT, 0, (hipStream_t)stream>>>(fg_mask, A, pos, npos);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_seg_gt_rows(const float* batch_idx, int n_targets, int B, int n_max, int32_t* rows, void* stream) {
  DY_CHECK(rows && B > 0 && n_max > 0 && n_targets >= 0 && (n_targets == 0 || batch_idx), "dy_seg_gt_rows: bad args");
  dy_note_kernel("seg_gt_rows_kernel");
  seg_gt_rows_kernel<<<dy_cdiv(B, 64), 64, 0, (hipStream_t)stream>>>(batch_idx, n_targets, B, n_max, rows);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_seg_loss_fwd(const dy_seg_desc* d, float hyp_box, float* lossp, const float* det_out, float* out, void* stream) {
  if (int e = check_seg(d, "dy_seg_loss_fwd")) return e;
  DY_CHECK(lossp && det_out && out, "dy_seg_loss_fwd: null output");
  const Seg s = seg_of(d);
  hipStream_t st = (hipStream_t)stream;
  dim3 grid(seg_grid_x(d), d->B);
  dy_note_kernel("seg_loss_fwd_kernel");
  DY_DISPATCH_DTYPE("dy_seg_loss_fwd", d->dtype, seg_loss_fwd_kernel<T><<<grid, NT, 0, st>>>(s, lossp));
  DY_LAUNCH_CHECK();
  float* means = lossp + (long)d->B * d->A;
  seg_image_mean_kernel<<<d->B, NT, 0, st>>>(lossp, d->npos, d->A, means);
  DY_LAUNCH_CHECK();
  seg_loss_finish_kernel<<<1, 64, 0, st>>>(means, d->B, hyp_box, det_out, out);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_seg_loss_bwd(const dy_seg_desc* d, const float* grad_out, float hyp_box, void* dmc, int64_t dmc_ld, void* dproto,
                               int64_t dproto_ld, void* stream) {
  if (int e = check_seg(d, "dy_seg_loss_bwd")) return e;
  DY_CHECK(grad_out && dmc && dproto, "dy_seg_loss_bwd: null output");
  const int es = dy_elem_size(d->dtype);
  DY_CHECK(dmc_ld >= NM && dproto_ld >= NM && dy_aligned16(dproto, dproto_ld, es),
           "dy_seg_loss_bwd: dmc_ld / dproto_ld below nm or d proto rows not 16-byte aligned");
  const Seg s = seg_of(d);
  hipStream_t st = (hipStream_t)stream;
  dim3 g1(seg_grid_x(d), d->B), g2(dy_cdiv((long)d->mh * d->mw, NT), d->B);
  dy_note_kernel("seg_loss_dproto_kernel");
  DY_DISPATCH_DTYPE("dy_seg_loss_bwd", d->dtype, {
    seg_loss_dmc_kernel<T><<<g1, NT, 0, st>>>(s, grad_out, hyp_box, (char*)dmc, dmc_ld);
    seg_loss_dproto_kernel<T><<<g2, NT, 0, st>>>(s, grad_out, hyp_box, (char*)dproto, dproto_ld);
  });
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_bias_add(void* x, int64_t ld, const float* bias, int64_t pixels, int C, int dtype, void* stream) {
  DY_CHECK(x && bias && ld >= C && C > 0 && pixels >= 0, "dy_bias_add: bad args");
  if (int e = dy_check_dtype("dy_bias_add", dtype)) return e;
  if (pixels == 0) return 0;
  const int blocks = dy_cdiv(pixels * C, NT);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("seg_bias_add_kernel");
  DY_DISPATCH_DTYPE("dy_bias_add", dtype, seg_bias_add_kernel<T><<<blocks, NT, 0, st>>>((T*)x, ld, bias, pixels, C));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_bias_grad(const void* dy, int64_t ld, int64_t pixels, int C, int dtype, float* scratch, int64_t scratch_elems, float* db,
                            void* stream) {
  DY_CHECK(dy && db && scratch && ld >= C && C > 0 && pixels >= 0, "dy_bias_grad: bad args");
  if (int e = dy_check_dtype("dy_bias_grad", dtype)) return e;
  DY_CHECK(scratch_elems >= (int64_t)BG_CHUNKS * C, "dy_bias_grad: scratch needs %ld floats", (long)BG_CHUNKS * C);
  hipStream_t st = (hipStream_t)stream;
  dim3 g1(BG_CHUNKS, dy_cdiv(C, NT));
  dy_note_kernel("seg_bias_grad_final_kernel");
  DY_DISPATCH_DTYPE("dy_bias_grad", dtype, seg_bias_grad_partial_kernel<T><<<g1, NT, 0, st>>>((const T*)dy, ld, pixels, C, scratch));
  DY_LAUNCH_CHECK();
  seg_bias_grad_final_kernel<<<dy_cdiv(C, NT), NT, 0, st>>>(scratch, C, db);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_seg_mask_decode(const void* proto, int64_t proto_ld, int nm, int mh, int mw, const float* det, int64_t det_ld,
                                  const int32_t* det_img, int n, float sx, float sy, int dtype, uint8_t* out, void* stream) {
  DY_CHECK(nm == NM, "dy_seg_mask_decode: nm=%d (built for %d)", nm, NM);
  DY_CHECK(n >= 0 && mh > 0 && mw > 0 && det_ld >= 6 + NM && proto_ld >= NM, "dy_seg_mask_decode: bad geometry");
  if (n == 0) return 0;
  DY_CHECK(proto && det && det_img && out, "dy_seg_mask_decode: null pointer");
  if (int e = dy_check_dtype("dy_seg_mask_decode", dtype)) return e;
  DY_CHECK(dy_aligned16(proto, proto_ld, dy_elem_size(dtype)), "dy_seg_mask_decode: proto rows must be 16-byte aligned");
  const int blocks = dy_cdiv((long)n * mh * mw, NT);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("seg_mask_decode_kernel");
  DY_DISPATCH_DTYPE("dy_seg_mask_decode", dtype,
                    seg_mask_decode_kernel<T><<<blocks, NT, 0, st>>>((const T*)proto, proto_ld, mh, mw, det, det_ld, det_img, n, sx, sy,
                                                                     out));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_seg_crop_mask(float* masks, const float* boxes, int n, int h, int w, void* stream) {
  DY_CHECK(n >= 0 && h > 0 && w > 0, "dy_seg_crop_mask: bad geometry");
  if (n == 0) return 0;
  DY_CHECK(masks && boxes, "dy_seg_crop_mask: null pointer");
  dy_note_kernel("seg_crop_mask_kernel");
  seg_crop_mask_kernel<<<dy_cdiv((long)n * h * w, NT), NT, 0, (hipStream_t)stream>>>(masks, boxes, n, h, w);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_seg_mask_iou(const uint8_t* pred, int n, const void* gt, int gt_dtype, int overlap, int m, int64_t hw, int32_t* work,
                               float* iou, void* stream) {
  DY_CHECK(n >= 0 && m >= 0 && hw > 0 && (gt_dtype == 0 || gt_dtype == 1), "dy_seg_mask_iou: bad args");
  DY_CHECK(overlap || gt_dtype == 0, "dy_seg_mask_iou: per-instance gt planes must be uint8");
  DY_CHECK(m <= 16384, "dy_seg_mask_iou: %d gt masks (at most 16384)", m);
  if (n == 0 || m == 0) return 0;
  DY_CHECK(pred && gt && work && iou, "dy_seg_mask_iou: null pointer");
  hipStream_t st = (hipStream_t)stream;
  int32_t* inter = work;                      // [m][n]
  int32_t* area_p = work + (long)m * n;       // [n]
  dy_note_kernel("seg_mask_iou_kernel");
  seg_mask_inter_kernel<<<n, NT, (overlap ? (m + 1) : 1) * sizeof(int), st>>>(pred, hw, n, gt, gt_dtype, overlap, m, inter, area_p);
  DY_LAUNCH_CHECK();
  seg_mask_iou_kernel<<<m, NT, 0, st>>>(gt, gt_dtype, overlap, hw, m, n, inter, area_p, iou);
  DY_LAUNCH_CHECK();
  return 0;
}
