// Segment inference at image resolution: the fused mask decode + bilinear resize + threshold of process_mask(upsample=True),
// process_mask_upsample and process_mask_native (reference ultralytics/utils/ops.py:572-642, scale_masks :645-666, crop_mask :553-569)
// and the bilinear resize of gt mask planes (ultralytics/models/yolo/segment/val.py:140-148).
//
// The reference writes sigmoid(c . P) as f32 [n, mh, mw], crops, F.interpolate()s it to f32 [n, H, W], crops and thresholds: four to
// five passes over n * H * W floats for one bit per pixel.  Here a workgroup owns one output tile (up to 64 x 64 pixels) of one image:
//   * the proto pixels under the tile plus the bilinear halo (at most RCAP of them; the launcher shrinks the tile until they fit) are
//     read ONCE into registers, NM channels each, and stay there for every detection of the image the workgroup walks;
//   * per detection the NM-deep dot product and the sigmoid run once per proto pixel (not once per tap: at scale 4 that is 64 times
//     fewer than per output pixel and tap), the values go to LDS (double buffered: one barrier per detection);
//   * a lane interpolates 16 consecutive output pixels of one row from LDS with tap indices / weights it computed once for the tile, and
//     stores them as one 16-byte vector;
//   * a tile that a detection's crop box does not reach is written as zeros without any arithmetic.
// No atomics, no cross-workgroup sums: two runs give the same bytes.
//
// The interpolation follows ATen's upsample_bilinear2d (align_corners=False, size given): scale = in / out in f32,
// src = scale * (dst + 0.5) - 0.5 clamped at 0, i0 = (int)src, i1 = min(i0 + 1, in - 1), w1 = src - i0, and the value
// wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d).  The file is built with -ffp-contract=off so that the index arithmetic
// and the weights round as written, on the device and in the launcher's region bound alike; the dot product uses fmaf explicitly.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"
#include "dy_bilinear.h"          // Tap, tap_of, bilerp

namespace {

constexpr int NM = 32;            // mask coefficients (Segment's nm)
constexpr int NT = 256;           // threads per workgroup
constexpr int PPT = 2;            // proto pixels a thread keeps in registers
constexpr int RCAP = NT * PPT;    // proto pixels under one output tile, halo included
constexpr int SEG = 16;           // output pixels per lane = one 16-byte store
constexpr int TILE_MAX = 64;      // output tile edge: (64 / SEG) lanes per row x 64 rows = NT lanes

struct Up {
  long proto_ld; int mh, mw;
  long det_ld;
  const int32_t* img_off; const int32_t* img_ids;
  int det_chunk, nsplit;
  int crop_before; float sx, sy;
  int top, left, wh, ww;              // source window: origin and size
  int oh, ow; float sch, scw;         // output size, in / out per axis
  int crop_after;
  int th, tw, tiles_x;                // output tile
};

template <typename T>
__device__ inline void load_nm(const T* p, float* out) {
#pragma unroll
  for (int k = 0; k < NM; k += DT<T>::VE) ldvec<T>(p + k, out + k);
}

template <typename T>
__global__ __launch_bounds__(NT) void seg_mask_upsample_kernel(Up u, const T* __restrict__ proto, const float* __restrict__ det,
                                                               uint8_t* __restrict__ out) {
  // (proto / det / out are kernel arguments of their own so that `__restrict__` holds: the detection row is wave-uniform and is then
  // read with scalar loads, which the stores to `out` would otherwise forbid)
  __shared__ float S[2][RCAP];
  const int g = blockIdx.y / u.nsplit, part = blockIdx.y - g * u.nsplit;
  const int j0 = u.img_off[g] + part * u.det_chunk;
  const int jend = u.img_off[g + 1];
  const int j1 = j0 + u.det_chunk < jend ? j0 + u.det_chunk : jend;
  if (j0 >= j1) return;
  const int b = u.img_ids[g];
  const int ty = blockIdx.x / u.tiles_x, tx = blockIdx.x - ty * u.tiles_x;
  const int y0 = ty * u.th, x0 = tx * u.tw;
  const int y1 = y0 + u.th < u.oh ? y0 + u.th : u.oh, x1 = x0 + u.tw < u.ow ? x0 + u.tw : u.ow;
  // proto region under the tile, in window coordinates (tap indices are monotone in the output coordinate)
  const int r0 = tap_of(y0, u.sch, u.wh).i0, r1 = tap_of(y1 - 1, u.sch, u.wh).i1;
  const int c0 = tap_of(x0, u.scw, u.ww).i0, c1 = tap_of(x1 - 1, u.scw, u.ww).i1;
  const int rw = c1 - c0 + 1, np = (r1 - r0 + 1) * rw;
  if (np > RCAP) return;              // cannot happen: the launcher sizes the tile by the same arithmetic
  const int tid = threadIdx.x;

  // this thread's proto pixels, resident for the whole detection walk
  float pv[PPT][NM];
  float pxf[PPT], pyf[PPT];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int p = tid + k * NT;
    const int ry = p / rw, rx = p - ry * rw;
    const int py = u.top + r0 + ry, px = u.left + c0 + rx;
    pxf[k] = (float)px; pyf[k] = (float)py;
    if (p < np) {
      load_nm<T>(proto + (((long)b * u.mh + py) * u.mw + px) * u.proto_ld, pv[k]);
    } else {
#pragma unroll
      for (int c = 0; c < NM; ++c) pv[k][c] = 0.f;
    }
  }

  // this lane's 16 output pixels: row y, columns xs .. xs + 15
  const int nsx = u.tw / SEG;
  const int row = tid / nsx, sg = tid - row * nsx;
  const int y = y0 + row, xs = x0 + sg * SEG;
  const bool active = row < u.th && y < y1 && xs < x1;
  int ya = 0, yb = 0;
  float wy1 = 0.f;
  int xo[SEG];                         // region column of tap 0, bit 16: tap 1 is one to the right
  float wx1[SEG];
  if (active) {
    const Tap t = tap_of(y, u.sch, u.wh);
    ya = (t.i0 - r0) * rw; yb = (t.i1 - r0) * rw; wy1 = t.w1;
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
      const int x = xs + i < x1 ? xs + i : x1 - 1;
      const Tap tx_ = tap_of(x, u.scw, u.ww);
      xo[i] = (tx_.i0 - c0) | ((tx_.i1 - tx_.i0) << 16);
      wx1[i] = tx_.w1;
    }
  } else {
#pragma unroll
    for (int i = 0; i < SEG; ++i) { xo[i] = 0; wx1[i] = 0.f; }
  }
  const float fy = (float)y;

  int buf = 0;
  for (int j = j0; j < j1; ++j) {
    const float* r = det + (long)j * u.det_ld;
    const float bx0 = r[0], by0 = r[1], bx1 = r[2], by1 = r[3];
    const float cx0 = __fmul_rn(bx0, u.sx), cy0 = __fmul_rn(by0, u.sy), cx1 = __fmul_rn(bx1, u.sx), cy1 = __fmul_rn(by1, u.sy);
    // does the crop box reach this tile at all?  (conservative; the per-pixel tests below decide)
    bool reach = true;
    if (u.crop_after) reach = (float)(x1 - 1) >= bx0 && (float)x0 < bx1 && (float)(y1 - 1) >= by0 && (float)y0 < by1;
    if (u.crop_before)
      reach = reach && (float)(u.left + c1) >= cx0 && (float)(u.left + c0) < cx1 && (float)(u.top + r1) >= cy0 && (float)(u.top + r0) < cy1;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (reach) {
      float* s = S[buf];
      buf ^= 1;
#pragma unroll
      for (int k = 0; k < PPT; ++k) {
        const int p = tid + k * NT;
        if (p < np) {
          float z = 0.f;
#pragma unroll
          for (int c = 0; c < NM; ++c) z = fmaf(r[6 + c], pv[k][c], z);
          float v = 1.f / (1.f + expf(-z));
          if (u.crop_before && !(pxf[k] >= cx0 && pxf[k] < cx1 && pyf[k] >= cy0 && pyf[k] < cy1)) v = 0.f;
          s[p] = v;
        }
      }
      __syncthreads();
      if (active) {
        const bool rowin = !u.crop_after || (fy >= by0 && fy < by1);
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
          const int o = xo[i] & 0xffff, st = xo[i] >> 16;
          const float v = bilerp(s[ya + o], s[ya + o + st], s[yb + o], s[yb + o + st], wx1[i], wy1);
          const float fx = (float)(xs + i);
          const bool in = rowin && (!u.crop_after || (fx >= bx0 && fx < bx1));
          if (in && v > 0.5f) w[i >> 2] |= 1u << (8 * (i & 3));
        }
      }
    }
    if (active) {
      const long base = ((long)j * u.oh + y) * u.ow + xs;
      if (((base & 15) == 0) && xs + SEG <= x1) {
        const u32x4 v = {w[0], w[1], w[2], w[3]};
        *reinterpret_cast<u32x4*>(out + base) = v;
      } else {
#pragma unroll
        for (int i = 0; i < SEG; ++i)
          if (xs + i < x1) out[base + i] = (uint8_t)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
      }
    }
  }
}

// ---- plane resize ---------------------------------------------------------------------------------------------------------------
struct Rs {
  const void* src; int kind, m, h, w, top, left, wh, ww;
  void* out; int out_f32, oh, ow; float sch, scw;
};

__device__ inline float rs_src(const Rs& r, int k, int y, int x) {
  const long o = (long)y * r.w + x;
  if (r.kind == 0) return (float)((const uint8_t*)r.src)[(long)k * r.h * r.w + o];
  if (r.kind == 1) return (int)((const uint8_t*)r.src)[o] == k + 1 ? 1.f : 0.f;
  if (r.kind == 2) return ((const int32_t*)r.src)[o] == k + 1 ? 1.f : 0.f;
  return ((const float*)r.src)[(long)k * r.h * r.w + o];
}

// one thread per four consecutive output pixels of one row
__global__ __launch_bounds__(NT) void mask_resize_kernel(Rs r) {
  const int gw = (r.ow + 3) / 4;
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= (long)r.m * r.oh * gw) return;
  const int gx = (int)(i % gw);
  const long t = i / gw;
  const int y = (int)(t % r.oh), k = (int)(t / r.oh);
  const Tap ty = tap_of(y, r.sch, r.wh);
  const int ya = r.top + ty.i0, yb = r.top + ty.i1;
  const int xs = gx * 4, n = r.ow - xs < 4 ? r.ow - xs : 4;
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e = 0; e < n; ++e) {
    const Tap tx = tap_of(xs + e, r.scw, r.ww);
    const int xa = r.left + tx.i0, xb = r.left + tx.i1;
    v[e] = bilerp(rs_src(r, k, ya, xa), rs_src(r, k, ya, xb), rs_src(r, k, yb, xa), rs_src(r, k, yb, xb), tx.w1, ty.w1);
  }
  const long base = ((long)k * r.oh + y) * r.ow + xs;
  if (r.out_f32) {
    float* o = (float*)r.out + base;
    if (n == 4 && (base & 3) == 0) { const f32x4 q = {v[0], v[1], v[2], v[3]}; *reinterpret_cast<f32x4*>(o) = q; }
    else for (int e = 0; e < n; ++e) o[e] = v[e];
  } else {
    uint8_t* o = (uint8_t*)r.out + base;
    if (n == 4 && (base & 3) == 0) {
      uint32_t q = 0;
      for (int e = 0; e < 4; ++e) q |= (v[e] > 0.5f ? 1u : 0u) << (8 * e);
      *reinterpret_cast<uint32_t*>(o) = q;
    } else {
      for (int e = 0; e < n; ++e) o[e] = v[e] > 0.5f ? 1 : 0;
    }
  }
}

// largest count of source rows (columns) under one tile of `t` output rows (columns)
int max_span(int out, int t, float scale, int in) {
  int best = 0;
  for (int a = 0; a < out; a += t) {
    const int e = a + t < out ? a + t : out;
    const int span = tap_of(e - 1, scale, in).i1 - tap_of(a, scale, in).i0 + 1;
    if (span > best) best = span;
  }
  return best;
}

int check_window(const char* who, int h, int w, int top, int left, int bottom, int right, int oh, int ow) {
  DY_CHECK(h > 0 && w > 0 && oh > 0 && ow > 0, "%s: empty geometry", who);
  DY_CHECK(top >= 0 && left >= 0 && bottom <= h && right <= w && top < bottom && left < right,
           "%s: window rows [%d, %d) columns [%d, %d) outside the %d x %d plane", who, top, bottom, left, right, h, w);
  return 0;
}

}  // namespace

extern "C" int dy_seg_mask_upsample(const void* proto, int64_t proto_ld, int nm, int mh, int mw, int dtype, const float* det,
                                    int64_t det_ld, const int32_t* img_off, const int32_t* img_ids, int n_groups, int max_group,
                                    int det_chunk, int crop_before, float sx, float sy, int top, int left, int bottom, int right, int oh,
                                    int ow, int crop_after, uint8_t* out, void* stream) {
  DY_CHECK(nm == NM, "dy_seg_mask_upsample: nm=%d (built for %d)", nm, NM);
  DY_CHECK(n_groups >= 0 && max_group >= 0 && det_ld >= 6 + NM && proto_ld >= NM, "dy_seg_mask_upsample: bad geometry");
  if (int e = check_window("dy_seg_mask_upsample", mh, mw, top, left, bottom, right, oh, ow)) return e;
  if (n_groups == 0 || max_group == 0) return 0;
  DY_CHECK(proto && det && img_off && img_ids && out, "dy_seg_mask_upsample: null pointer");
  if (int e = dy_check_dtype("dy_seg_mask_upsample", dtype)) return e;
  DY_CHECK(det_chunk > 0, "dy_seg_mask_upsample: det_chunk must be positive");
  DY_CHECK(dy_aligned16(proto, proto_ld, dy_elem_size(dtype)), "dy_seg_mask_upsample: proto rows must be 16-byte aligned");
  DY_CHECK(((uintptr_t)out) % 16 == 0, "dy_seg_mask_upsample: out must be 16-byte aligned");
  Up u;
  u.proto_ld = proto_ld; u.mh = mh; u.mw = mw;
  u.det_ld = det_ld; u.img_off = img_off; u.img_ids = img_ids;
  u.det_chunk = det_chunk; u.nsplit = dy_cdiv(max_group, det_chunk);
  u.crop_before = crop_before; u.sx = sx; u.sy = sy;
  u.top = top; u.left = left; u.wh = bottom - top; u.ww = right - left;
  u.oh = oh; u.ow = ow; u.sch = (float)u.wh / (float)oh; u.scw = (float)u.ww / (float)ow;
  u.crop_after = crop_after;
  // the largest tile whose proto region fits the registers of one workgroup
  int th = TILE_MAX, tw = TILE_MAX;
  for (;;) {
    const int sh = max_span(oh, th, u.sch, u.wh), sw = max_span(ow, tw, u.scw, u.ww);
    if ((long)sh * sw <= RCAP) break;
    if ((sh >= sw || tw == SEG) && th > 1) th /= 2;
    else if (tw > SEG) tw /= 2;
    else DY_CHECK(false, "dy_seg_mask_upsample: %d x %d -> %d x %d shrinks too much for one tile", u.wh, u.ww, oh, ow);
  }
  u.th = th; u.tw = tw; u.tiles_x = dy_cdiv(ow, tw);
  const long gy = (long)n_groups * u.nsplit;
  DY_CHECK(gy <= 65535, "dy_seg_mask_upsample: %ld image chunks (at most 65535)", gy);
  dim3 grid(u.tiles_x * dy_cdiv(oh, th), (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("seg_mask_upsample_kernel");
  DY_DISPATCH_DTYPE("dy_seg_mask_upsample", dtype, seg_mask_upsample_kernel<T><<<grid, NT, 0, st>>>(u, (const T*)proto, det, out));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_mask_resize(const void* src, int src_kind, int m, int h, int w, int top, int left, int bottom, int right, void* out,
                              int out_f32, int oh, int ow, void* stream) {
  DY_CHECK(src_kind >= 0 && src_kind <= 3 && m >= 0, "dy_mask_resize: bad args");
  if (int e = check_window("dy_mask_resize", h, w, top, left, bottom, right, oh, ow)) return e;
  if (m == 0) return 0;
  DY_CHECK(src && out, "dy_mask_resize: null pointer");
  DY_CHECK(((uintptr_t)out) % 16 == 0, "dy_mask_resize: out must be 16-byte aligned");
  Rs r;
  r.src = src; r.kind = src_kind; r.m = m; r.h = h; r.w = w; r.top = top; r.left = left; r.wh = bottom - top; r.ww = right - left;
  r.out = out; r.out_f32 = out_f32; r.oh = oh; r.ow = ow;
  r.sch = (float)r.wh / (float)oh; r.scw = (float)r.ww / (float)ow;
  const long groups = (long)m * oh * ((ow + 3) / 4);
  dy_note_kernel("mask_resize_kernel");
  mask_resize_kernel<<<dy_cdiv(groups, NT), NT, 0, (hipStream_t)stream>>>(r);
  DY_LAUNCH_CHECK();
  return 0;
}
