// What the convolution routes share outside their kernels: two device helpers, the descriptor -> kernel-parameter fills, the
// eligibility checks more than one route repeats, and the prototype of every route's entry points; for the weight gradient also
// the slab layout its shared reduce kernel reads (the split plan of the pixel loop is dy_plan.h's).  The order in which the routes
// are tried is the pair of tables in conv.hip (kRoutes, kWgradRoutes); tile-count and K thresholds stay with the kernel they tune.
#pragma once
#include <type_traits>
#include <utility>
#include "dy_common.h"
#include "dy_plan.h"
#include "../../include/dedark_yolo.h"

namespace dy_route {

// ---- device helpers (each kernel namespace pulls them in with `using`) ---------------------------------------------------------------
// bijective: blocks b, b+8, ... share an XCD; give each XCD a contiguous chunk of tile ids
__device__ inline int xcd_remap(int bid, int nblk) {
  int q = nblk >> 3, r = nblk & 7, x = bid & 7;
  int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + (bid >> 3);
}

// element offset of output pixel m (dst_row == 0: dense, offset = m * dst_ld; otherwise row / image strides of a strided destination)
template <typename P>
__device__ inline long dst_offset(const P& p, long m) {
  if (p.dst_row == 0) return m * p.dst_ld;
  const long HWd = (long)p.Hd * p.Wd;
  const long img = m / HWd;
  const int rem = (int)(m - img * HWd);
  const int oh = rem / p.Wd, ow = rem - oh * p.Wd;
  return img * p.dst_img + (long)oh * p.dst_row + (long)ow * p.dst_ld;
}

// ---- host fills: templates over a kernel's own parameter struct P, fields written by name ---------------------------------------------
// window tap (th, tw) -> weight tap (kh0 + khs*th, kw0 + kws*tw) of a KWf-wide pack (the tap subsets of a parity-split data gradient)
template <typename P>
inline void fill_weight_taps(P& p, const dy_conv_desc* d) {
  if (d->KHf > 0) {
    p.kh0 = d->kh0; p.khs = d->kh_step; p.kw0 = d->kw0; p.kws = d->kw_step; p.KWf = d->KWf;
    p.w_row = (long)d->KHf * d->KWf * d->Cs;
  } else {
    p.kh0 = 0; p.khs = 1; p.kw0 = 0; p.kws = 1; p.KWf = d->KW;
    p.w_row = (long)d->KH * d->KW * d->Cs;
  }
}

template <typename P>
inline void fill_dst_strides(P& p, const dy_conv_desc* d) {
  p.dst_row = d->dst_row_stride;
  p.dst_img = d->dst_img_stride ? d->dst_img_stride : (long)d->Hd * d->dst_row_stride;
}

// the block ConvP (conv.hip) and v2::P share
template <typename P>
inline void fill_gather(P& p, const dy_conv_desc* d) {
  p.src = (const char*)d->src; p.src_ld = d->src_ld; p.N = d->N; p.Hs = d->Hs; p.Ws = d->Ws; p.Cs = d->Cs;
  p.w = (const char*)d->w; p.dst = (char*)d->dst; p.dst_ld = d->dst_ld; p.Hd = d->Hd; p.Wd = d->Wd; p.Cd = d->Cd;
  p.KH = d->KH; p.KW = d->KW; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
  p.scale = d->scale; p.shift = d->shift; p.act = d->act; p.stats = d->stats; p.accumulate = d->accumulate;
  p.M = (long)d->N * d->Hd * d->Wd;
  p.Ktot = d->KH * d->KW * d->Cs;
  static const int ablate = dy_env("DY_ABLATE") ? atoi(dy_env("DY_ABLATE")) : 0;
  p.ablate = ablate;
  fill_dst_strides(p, d);
  fill_weight_taps(p, d);
}

// the tap geometry and DMA extents v4::P and v5::P share (mode 0: forward, 1: stride-1 data gradient)
template <typename P>
inline void fill_taps_extents(P& p, const dy_conv_desc* d, int mode) {
  p.src = (const char*)d->src; p.w = (const char*)d->w; p.dst = (char*)d->dst;
  p.src_ld = d->src_ld; p.dst_ld = d->dst_ld;
  p.src_bytes = (unsigned)((((long)d->N * d->Hs * d->Ws - 1) * d->src_ld + d->Cs) * 2);
  p.Hs = d->Hs; p.Ws = d->Ws; p.Cs = d->Cs; p.Hd = d->Hd; p.Wd = d->Wd; p.Cd = d->Cd;
  p.KH = d->KH; p.KW = d->KW;
  if (mode == 0) {
    p.stride = d->stride; p.dh0 = -d->pad; p.dhs = d->dil; p.dw0 = -d->pad; p.dws = d->dil;
  } else {               // stride-1 data gradient: dx[h] += dz[h + pad - kh*dil] * w[kh]
    p.stride = 1; p.dh0 = d->pad; p.dhs = -d->dil; p.dw0 = d->pad; p.dws = -d->dil;
  }
  fill_weight_taps(p, d);
  p.w_bytes = (unsigned)((long)d->Cd * p.w_row * 2);
  {
    const int dh_lo = p.dhs < 0 ? p.dh0 + p.dhs * (p.KH - 1) : p.dh0, dw_lo = p.dws < 0 ? p.dw0 + p.dws * (p.KW - 1) : p.dw0;
    const long lo = ((long)dh_lo * p.Ws + dw_lo) * p.src_ld * 2;
    p.a_min = lo < 0 ? (int)lo : 0;
  }
  p.scale = d->scale; p.shift = d->shift; p.act = d->act; p.stats = d->stats; p.accumulate = d->accumulate;
  // (bit 1: an output beyond 128 MB is streamed past the L2 with non-temporal stores -- its lines would evict the operand lines the
  //  taps re-read, and whoever reads it next streams it from memory anyway)
  if ((long)d->N * d->Hd * d->Wd * d->Cd * 2 > (128L << 20)) p.accumulate |= 2;
  p.M = (long)d->N * d->Hd * d->Wd;
  p.add_src = mode == 1 ? (const char*)d->add_src : nullptr; p.add_src_ld = d->add_src_ld;
  fill_dst_strides(p, d);
}

// `classes[0..ncls)`: forward-style problems that differ only in destination offset, grid extent, tap subset and pad (the parity
// classes of a stride-2 data gradient) as ONE launch: the per-class fields of p.cls ...
template <typename P>
inline void fill_parity_classes(P& p, const dy_conv_desc* classes, int ncls) {
  p.ncls = ncls > 1 ? ncls : 0;
  for (int c = 0; c < p.ncls; ++c) {
    const dy_conv_desc& q = classes[c];
    DyParityCls& k = p.cls[c];
    k.dst = (char*)q.dst; k.M = (long)q.N * q.Hd * q.Wd; k.Hd = q.Hd; k.Wd = q.Wd; k.KH = q.KH; k.KW = q.KW; k.pad = q.pad;
    k.kh0 = q.kh0; k.kw0 = q.kw0; k.Ktot = q.KH * q.KW * q.Cs; k.blk0 = 0; k._r = 0;
  }
}

// ... and their block ranges, once the tile (bm rows, p.tiles_n channel tiles) is known.  Returns the launch's block count.
// CLS_SEQUENTIAL: class after class, blk0 = first block.  CLS_XCD_SLOTS: every XCD works through its eighth of class 0, then of
// class 1, ...: blk0 = first slot of the class in every XCD's block sequence, _r = its slots per XCD.
enum ClsOrder { CLS_SEQUENTIAL, CLS_XCD_SLOTS };
template <typename P>
inline int number_parity_blocks(P& p, int bm, ClsOrder order) {
  int next = 0;
  for (int c = 0; c < p.ncls; ++c) {
    DyParityCls& k = p.cls[c];
    const int tiles = dy_cdiv(k.M, bm) * p.tiles_n;
    k.blk0 = next;
    k._r = order == CLS_XCD_SLOTS ? dy_cdiv(tiles, 8) : 0;
    next += order == CLS_XCD_SLOTS ? k._r : tiles;
  }
  return order == CLS_XCD_SLOTS ? 8 * next : next;
}

// ---- host predicates ---------------------------------------------------------------------------------------------------------------
// The buffer descriptors of the DMA kernels (conv_v4.hip, conv_v5.hip): the activation extent plus the halo of a KH x KW window -- the
// most negative tap offset is folded into the descriptor's base -- stays below 2^31 (bit 31 marks a padded lane), the weights below 2^30.
inline bool dma_extents_ok(const dy_conv_desc* d, int KH, int KW, int dil) {
  const long src_bytes = (((long)d->N * d->Hs * d->Ws - 1) * d->src_ld + d->Cs) * 2;
  const long w_row = d->KHf > 0 ? (long)d->KHf * d->KWf * d->Cs : (long)d->KH * d->KW * d->Cs;
  const long w_bytes = (long)d->Cd * w_row * 2;
  const long halo = ((long)KH * dil * d->Ws + (long)KW * dil) * d->src_ld * 2;
  return src_bytes + halo <= 0x7fffffffL && w_bytes <= 0x3fffffffL;
}

// parity classes that one launch can take: same dz, weight pack, channel counts and views, raw output, 16-byte aligned
inline bool parity_classes_uniform(const dy_conv_desc* c, int ncls) {
  const dy_conv_desc* d = &c[0];
  for (int i = 0; i < ncls; ++i) {
    const dy_conv_desc& q = c[i];
    if (q.src != d->src || q.w != d->w || q.Cs != d->Cs || q.Cd != d->Cd || q.dtype != d->dtype || q.stride != 1 || q.dil != 1 || q.KHf != d->KHf ||
        q.KWf != d->KWf || q.kh_step != d->kh_step || q.kw_step != d->kw_step || q.dst_ld != d->dst_ld || q.dst_row_stride != d->dst_row_stride ||
        q.dst_img_stride != d->dst_img_stride || q.src_ld != d->src_ld || q.accumulate != d->accumulate || q.scale || q.shift || q.stats ||
        q.act != DY_ACT_NONE)
      return false;
    if ((q.dst_ld * 2) % 16 != 0 || ((uintptr_t)q.dst) % 16 != 0 || (q.src_ld * 2) % 16 != 0) return false;
  }
  return true;
}

}  // namespace dy_route

// ---- the routes' entry points --------------------------------------------------------------------------------------------------------
// A forward / data-gradient route is `bool eligible(d, mode)` + `int launch(d, mode, stream)`; mode 0: forward (and the forward-style
// parity classes of a stride-2 data gradient), 1: data gradient.  Routes that serve one mode only ignore the argument.
bool dy_dense_fwd_eligible(const dy_conv_desc* d, int mode);                 // dense.hip: whole-input windows = fully connected layers
int dy_dense_fwd_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_dense_dgrad_eligible(const dy_conv_desc* d, int mode);
int dy_dense_dgrad_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_stem_fwd_eligible(const dy_conv_desc* d, int mode);             // conv_small.hip: direct stem / thin kernels
int dy_conv_stem_fwd_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_small_dgrad_eligible(const dy_conv_desc* d, int mode);
int dy_conv_small_dgrad_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_px_eligible(const dy_conv_desc* d, int mode);                   // conv_px.hip: pixel-streaming 1x1 kernel
int dy_conv_px_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_v4_eligible(const dy_conv_desc* d, int mode);                   // conv_v4.hip: 256 x 256 tiles, one block per CU
int dy_conv_v4_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_v4_classes_eligible(const dy_conv_desc* classes, int ncls);
int dy_conv_v4_launch_classes(const dy_conv_desc* classes, int ncls, void* stream);
bool dy_conv_v5_eligible(const dy_conv_desc* d, int mode);                   // conv_v5.hip: 256 x 128 / 256 x 64 tiles, 3x3 band kernel
int dy_conv_v5_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_v5_classes_eligible(const dy_conv_desc* classes, int ncls);
int dy_conv_v5_launch_classes(const dy_conv_desc* classes, int ncls, void* stream);
bool dy_conv_v3_eligible(const dy_conv_desc* d, int mode);                   // conv_v3.hip: 3x3 / stride-1 band kernel
int dy_conv_v3_launch(const dy_conv_desc* d, int mode, void* stream);
bool dy_conv_v2_eligible(const dy_conv_desc* d, int mode);                   // conv_v2.hip: pipelined kernel, any window / stride
int dy_conv_v2_launch(const dy_conv_desc* d, int mode, void* stream);
int dy_conv_v2_launch_classes(const dy_conv_desc* classes, int ncls, void* stream);
bool dy_conv_prefers_256(const dy_conv_desc* d);                             // conv_v2.hip: its 256 x 256 tile still fills the chip

// The weight-gradient routes take the checked arguments of dy_conv2d_wgrad as one struct (host only).
struct DyWgradArgs {
  const void* x;
  long x_ld;
  int N, Hi, Wi, Cin_pad;
  const void* dz;
  long dz_ld;
  int Ho, Wo, Cout_pad, KH, KW, stride, pad, dil, Cout, Cin;
  float* scratch;
  long scratch_elems;
  float* g_oihw;
  int dtype;
};

namespace dy_route {

// the problem description WgP (conv.hip), wg2::P and wg4::P share; `pointwise` (1x1 / stride 1 / no padding: x rows are the output
// pixels) only where the kernel reads it from its parameters
template <typename P, typename = void> struct HasPointwise : std::false_type {};
template <typename P> struct HasPointwise<P, std::void_t<decltype(std::declval<P&>().pointwise)>> : std::true_type {};

template <typename P>
inline void fill_wgrad_problem(P& p, const DyWgradArgs& a) {
  p.x = (const char*)a.x; p.x_ld = a.x_ld; p.N = a.N; p.Hi = a.Hi; p.Wi = a.Wi; p.Cin = a.Cin_pad;
  p.dz = (const char*)a.dz; p.dz_ld = a.dz_ld; p.Ho = a.Ho; p.Wo = a.Wo; p.Cout = a.Cout_pad;
  p.KH = a.KH; p.KW = a.KW; p.stride = a.stride; p.pad = a.pad; p.dil = a.dil; p.part = a.scratch;
  p.M = (long)a.N * a.Ho * a.Wo;
  p.Ktot = a.KH * a.KW * a.Cin_pad;
  if constexpr (HasPointwise<P>::value) p.pointwise = (a.KH == 1 && a.KW == 1 && a.stride == 1 && a.pad == 0) ? 1 : 0;
}

}  // namespace dy_route

// Slabs with the output channel contiguous (wgrad_v2.hip, wgrad_v3.hip): split s keeps the partial dW[k'][co], k' = tap * Cin_pad +
// ci, at part[s * split_stride + (co / co_tile) * co_stride + (k' / k_tile) * k_stride + (k' % k_tile) * co_tile + co % co_tile].
struct DyCoSlabs {
  int co_tile;           // output channels per tile = length of a tile row
  long co_stride;        // elements from one co tile to the next
  int k_tile;            // k' rows per tile
  long k_stride;         // elements from one k' tile to the next
  long split_stride;     // elements from one split's slab set to the next
  int Cin_pad, KH, KW;
};
// conv.hip: g[co][ci][kh][kw] (f32 OIHW, real channel counts) = sum over the splits, in a fixed order
int dy_wgrad_reduce_co_slabs(const float* part, int splits, const DyCoSlabs& L, int Cout, int Cin, float* g_oihw, void* stream);

bool dy_dense_wgrad_eligible(const DyWgradArgs& a);                          // dense.hip
int dy_dense_wgrad_launch(const DyWgradArgs& a, void* stream);
bool dy_wgrad_v3_eligible(const DyWgradArgs& a);                             // wgrad_v3.hip: band kernel of the 64 / 128-channel 3x3 layers
int dy_wgrad_v3_launch(const DyWgradArgs& a, void* stream);
bool dy_wgrad_v4_eligible(const DyWgradArgs& a);                             // wgrad_v4.hip: 256 x 256 tiles
int dy_wgrad_v4_launch(const DyWgradArgs& a, void* stream);
bool dy_wgrad_v2_eligible(const DyWgradArgs& a);                             // wgrad_v2.hip: pipelined 128 x 128 / 256 x 256 tiles
int dy_wgrad_v2_launch(const DyWgradArgs& a, void* stream);
