/* dedark_yolo.h -- C-ABI of the MI355X-native Dedark-YOLO hot path (libdedark_yolo.so).
 *
 * Drop-in boundary: the reference is 100 % Python on PyTorch; every entry point below replaces the
 * ATen op sequence issued by one reference function (cited as U/<file>:<lines>, U = ultralytics/ in the reference
 * tree).  Signatures are plain pointers and sizes -- no torch types.  All pointers are DEVICE pointers unless
 * named host_*.  Every function enqueues on `stream` (a hipStream_t passed as void*), never synchronises, never
 * allocates, and returns 0 on success; on failure it returns non-zero and dy_last_error() describes it.  (Where an entry
 * departs from this -- dy_aug_resize_area_u8 allocates stream-ordered, dy_cls_render waits for its descriptor check -- its
 * own comment says so.)
 *
 * Layouts: activations are NHWC ("pixel-major"); a tensor view is (pointer to element [n=0,h=0,w=0,c=c0], ld) where
 * `ld` is the pixel stride in ELEMENTS, so a channel slice of a wider concat buffer is a view with ld = total width.
 * dtype: DY_F32 (parity path, exact-f32 MFMA 32x32x2), DY_BF16 (throughput path, MFMA 32x32x16 / 16x16x32, f32 accumulate) or
 * DY_F16 (IEEE half: the same kernels on the f16 MFMA; the reference's AMP dtype, BASELINE configs[4]).
 * Any other dtype value is an error: the entry launches nothing and returns 1 with "<entry>: bad dtype <value>".
 * Weights: f32 OIHW master (the reference state_dict layout) is packed per step into [Cout][KH][KW][Cin] ("KRSC").
 */
#ifndef DEDARK_YOLO_H
#define DEDARK_YOLO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DY_F32 0
#define DY_BF16 1
#define DY_F16 2
#define DY_ACT_NONE 0
#define DY_ACT_SILU 1
#define DY_ACT_LEAKY 2 /* LeakyReLU(0.1) */
#define DY_STATS_REPLICAS 64 /* copies of the BN batch-statistics accumulators filled by dy_conv2d_fwd */
#define DY_BN_BWD_REPLICAS 8 /* copies of the (sum g, sum g*zhat) accumulators of dy_bn_act_bwd_reduce */

const char* dy_last_error(void);
int dy_version(void);
/* Profiling aid: symbol of the GPU kernel launched by the last call on this thread ("" if the entry reports none); bench.py
 * attaches its per-kernel roofline to it.  dy_clear_last_kernel resets it. */
const char* dy_last_kernel(void);
void dy_clear_last_kernel(void);

/* ------------------------------------------------------------------------------------------------ convolution
 * Replaces nn.Conv2d inside Conv (U/nn/modules/conv.py:38-55), add_conv (U/nn/modules/block.py:24-45),
 * ConvBlock (U/nn/modules/common.py:9-23), Detect's 1x1 heads (U/nn/modules/head.py:40-46), RFBblock
 * (block.py:703-734) and nn.Linear of the extractor (common.py:65-66).  Implicit GEMM on MFMA. */
typedef struct {
  const void* src;   /* source activations view */
  int64_t src_ld;
  int N, Hs, Ws, Cs; /* source geometry; Cs = channels consumed per tap (multiple of 4 for f32, 8 for bf16) */
  const void* w;     /* packed weights [Cd][KH][KW][Cs], compute dtype */
  void* dst;         /* destination view */
  int64_t dst_ld;
  int Hd, Wd, Cd;    /* destination geometry; Cd = channels produced */
  int KH, KW, stride, pad, dil;
  const float* scale; /* optional per-Cd affine applied to the accumulator: v = acc*scale + shift (NULL = 1) */
  const float* shift; /* optional (bias / folded BN shift) (NULL = 0) */
  int act;            /* DY_ACT_* applied after the affine */
  double* stats;      /* optional [DY_STATS_REPLICAS][2*Cd] zeroed accumulators: (sum, sum of squares) of the RAW conv
                         output over all pixels, spread over replicas to avoid atomic contention (BN batch stats) */
  int accumulate;     /* 1: dst += result */
  int dtype;          /* DY_F32 | DY_BF16 | DY_F16 (src, w, dst) */
  /* optional extensions, all zero = dense destination / full window (a zero-initialised descriptor keeps the old meaning) */
  int64_t dst_row_stride; /* elements between destination rows    (0: Wd * dst_ld) */
  int64_t dst_img_stride; /* elements between destination images  (0: Hd * row stride) */
  int KHf, KWf;           /* tap subset: `w` is a [Cd][KHf][KWf][Cs] pack and window tap (th, tw) of the KH x KW window uses */
  int kh0, kh_step;       /* weight tap (kh0 + kh_step*th, kw0 + kw_step*tw).  KHf == 0: no subset.  dy_conv2d_dgrad uses   */
  int kw0, kw_step;       /* this internally to run a stride-2 data gradient as 4 dense stride-1 problems (one per parity)   */
  int dst_valid_channels; /* hint: only the first k destination channels can be non-zero (the rest is channel padding whose
                             weights are zero); 0 = unknown.  Lets the stem kernels skip the padding. */
  void* dst_planar;       /* dy_conv2d_dgrad only, optional: write dx as PLANAR [N, dst_valid_channels, Hd, Wd] (compute dtype)
                             instead of the NHWC view `dst` (which may then be NULL).  Only the direct stem kernel (3x3,
                             stride 2, pad 1, <= 8 padded input channels, bf16) supports it; otherwise the call fails. */
  const void* add_src;    /* dy_conv2d_dgrad only, optional: a [N,Hd,Wd,Cd] view (pixel stride add_src_ld, compute dtype) added to */
  int64_t add_src_ld;     /* the result: dst = [dst +] dx + add_src.  Bottleneck's shortcut gradient (U/nn/modules/block.py:565:
                             x + cv2(cv1(x))) joins the data gradient of cv1 this way instead of through a separate pass; the
                             large-tile kernels add it in their epilogue, other routes run dy_copy2d(accumulate) afterwards. */
} dy_conv_desc;

/* forward: dst[n,ho,wo,:] = epilogue( sum_{kh,kw,c} src[n, ho*stride-pad+kh*dil, wo*stride-pad+kw*dil, c] * w[:,kh,kw,c] ) */
int dy_conv2d_fwd(const dy_conv_desc* d, void* stream);
/* data gradient: src = dz [N,Hs,Ws,Cs=Cout], w = transposed pack [Cd=Cin][KH][KW][Cs=Cout], dst = dx [N,Hd,Wd,Cd];
 * dx[n,h,w,:] = sum over taps with (h+pad-kh*dil) % stride == 0 of dz[n,(h+pad-kh*dil)/stride, ...,:] * w */
int dy_conv2d_dgrad(const dy_conv_desc* d, void* stream);
/* weight gradient: g_oihw[Cout][Cin][KH][KW] (f32, overwritten) = sum_pixels dz^T * gather(x).
 * x view [N,Hi,Wi,Cin_pad], dz view [N,Ho,Wo,Cout_pad] (zero-padded channels).  The pixel reduction is split over
 * thread blocks that store partial tiles into `scratch` (any f32 workspace of scratch_elems floats, >= one tile set;
 * more allows more splits); a second kernel sums the slabs in a fixed order (deterministic, no atomics) and writes OIHW. */
int dy_conv2d_wgrad(const void* x, int64_t x_ld, int N, int Hi, int Wi, int Cin_pad, const void* dz, int64_t dz_ld, int Ho,
                    int Wo, int Cout_pad, int KH, int KW, int stride, int pad, int dil, int Cout, int Cin, float* scratch,
                    int64_t scratch_elems, float* g_oihw, int dtype, void* stream);
/* f32 OIHW [Cout][Cin][KH][KW] -> packed [Cout_pad][KH][KW][Cin_pad] (transposed=0) or [Cin_pad][KH][KW][Cout_pad]
 * (transposed=1) in `dtype`; padded input/output channels are written as zero. */
int dy_pack_weight(const float* w_oihw, void* packed, int Cout, int Cout_pad, int Cin, int Cin_pad, int KH, int KW,
                   int transposed, int dtype, void* stream);
/* The same for every weight of a model in ONE launch (after each optimizer step): `items_dev` is a DEVICE array sorted by
 * first_block; item i owns thread blocks [first_block, first_block + dy_pack_item_blocks(...)); n_blocks = their sum. */
typedef struct {
  const float* w;   /* f32 OIHW master weight */
  void* packed;     /* destination, `dtype` elements */
  int Cout, Cout_pad, Cin, Cin_pad, KH, KW, transposed, dtype;
  int64_t first_block;
} dy_pack_item;
int64_t dy_pack_item_blocks(int Cout_pad, int Cin_pad, int KH, int KW);
int dy_pack_weights_multi(const dy_pack_item* items_dev, int n_items, int64_t n_blocks, void* stream);

/* ------------------------------------------------------------------------------------ BatchNorm + activation
 * Replaces nn.BatchNorm2d (train: batch statistics, eps 1e-3, momentum 0.03, U/utils/torch_utils.py:263-265) followed by
 * SiLU / LeakyReLU(0.1) (conv.py:40,51; block.py:42) and the Bottleneck residual add (block.py:565). */
/* stats[DY_STATS_REPLICAS][2C] (from dy_conv2d_fwd) -> scale/shift (y = z*scale + shift), saved mean/invstd, running buffers
 * update. */
int dy_bn_finalize(const double* stats, int64_t count, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, float momentum, float eps, float* scale, float* shift, float* mean, float* invstd,
                   int C, void* stream);
/* eval-mode fold: scale = gamma/sqrt(var+eps), shift = beta - mean*scale */
int dy_bn_fold_eval(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                    float* scale, float* shift, int C, void* stream);
/* Channel padding.  The entries above and below treat all C channels as real: every per-channel buffer is C floats.  Their
 * *_valid variants take the layer's real channel count C_valid <= C as well, for views padded to C channels (C = Cout rounded
 * up to 4 in f32, to 8 in bf16 / f16):
 *   - gamma, beta, running_mean, running_var, dgamma and dbeta are C_valid floats; nothing at or past index C_valid is read or
 *     written (a flat parameter store puts the next tensor right there);
 *   - stats, sums, scale, shift, mean, invstd and aff stay C wide; the pad channels get scale = shift = mean = invstd = 0, so
 *     the pad lanes of y are act(0) = 0 and those of dz are 0.
 * dy_X(..., C, ...) is dy_X_valid(..., C, C, ...). */
int dy_bn_finalize_valid(const double* stats, int64_t count, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, float* scale, float* shift, float* mean, float* invstd,
                         int C, int C_valid, void* stream);
int dy_bn_fold_eval_valid(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                          float* scale, float* shift, int C, int C_valid, void* stream);
/* y = act(z*scale + shift) (+ residual); views over `pixels` pixels x C channels */
int dy_bn_act_fwd(const void* z, int64_t z_ld, const float* scale, const float* shift, int act, const void* residual,
                  int64_t res_ld, void* y, int64_t y_ld, int64_t pixels, int C, int dtype, void* stream);
/* backward pass 1: sums[0:C] = sum g, sums[C:2C] = sum g*zhat with g = dy*act'(u), u = z*scale+shift,
 * zhat = (z-mean)*invstd (has_bn) ; without BN only sum g (bias gradient).
 * z must be the PRE-activation (with scale = shift = NULL: u = z = conv + bias): act' is evaluated at u.  Only for an activation
 * that keeps the sign and whose slope depends on nothing else (none, LeakyReLU) may the caller pass the stored output y = act(u)
 * as z without BatchNorm; for SiLU act'(y) != act'(u).
 * `sums` is [DY_BN_BWD_REPLICAS][2C] doubles, zeroed by the caller; thread blocks spread their atomics over the replicas
 * and dy_bn_act_bwd_apply adds them up. */
int dy_bn_act_bwd_reduce(const void* dy, int64_t dy_ld, const void* z, int64_t z_ld, const float* scale,
                         const float* shift, const float* mean, const float* invstd, int act, int has_bn, double* sums,
                         int64_t pixels, int C, int dtype, void* stream);
/* backward pass 2: dz = gamma*invstd*(g - sum_g/M - zhat*sum_gz/M)  (has_bn) or dz = g; also dgamma = sum_gz,
 * dbeta = sum_g (written when the pointers are non-NULL, by block 0). */
int dy_bn_act_bwd_apply(const void* dy, int64_t dy_ld, const void* z, int64_t z_ld, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* gamma, int act, int has_bn,
                        const double* sums, void* dz, int64_t dz_ld, float* dgamma, float* dbeta, int64_t pixels, int C,
                        int dtype, void* stream);
int dy_bn_act_bwd_apply_valid(const void* dy, int64_t dy_ld, const void* z, int64_t z_ld, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const float* gamma, int act, int has_bn,
                              const double* sums, void* dz, int64_t dz_ld, float* dgamma, float* dbeta, int64_t pixels, int C,
                              int C_valid, int dtype, void* stream);

/* Two-branch BatchNorm + activation: y = act(u scale_u + shift_u + v scale_v + shift_v) over the raw outputs u, v of two
 * convolutions (RepConv.forward, U/nn/modules/conv.py:215-218 `self.act(self.conv1(x) + self.conv2(x))` with conv1 / conv2 =
 * Conv(act=False), conv.py:208-209: two nn.BatchNorm2d, the add and the SiLU).  scale / shift (/ mean / invstd) of each branch
 * come from dy_bn_finalize_valid (training) or dy_bn_fold_eval_valid (eval).  Views are `pixels` x C slices (ld >= C) of the
 * dtype; C is a whole number of 16-byte vectors and nothing outside the C columns is touched; the per-channel vectors are C floats. */
int dy_bn2_act_fwd(const void* u, int64_t u_ld, const void* v, int64_t v_ld, const float* scale_u, const float* shift_u,
                   const float* scale_v, const float* shift_v, int act, void* y, int64_t y_ld, int64_t pixels, int C, int dtype,
                   void* stream);
/* its backward (the autograd of conv.py:215-218 through both BatchNorms): z recomputed from u and v, g = dy act'(z),
 * S0 = sum g, S1 = sum g u^, S2 = sum g v^ (u^ = (u - mean_u) invstd_u), du = gamma_u invstd_u (g - S0 / M - u^ S1 / M), dv
 * likewise with S2, dgamma_u = S1, dgamma_v = S2, dbeta_u = dbeta_v = S0 (all four nullable), M = pixels >= 1.  The sums are
 * per-workgroup f32 partials over pixel ranges fixed by (pixels, C, dtype), added by a second kernel in f64 in an order fixed by
 * their count: no atomics, identical bytes on every run.  workspace: dy_bn2_act_bwd_workspace(pixels, C, dtype) floats, at most
 * 3 C (DY_BN2_MAX_PARTS + 1), 16-byte aligned, not initialised by the caller. */
#define DY_BN2_MAX_PARTS 1024
int64_t dy_bn2_act_bwd_workspace(int64_t pixels, int C, int dtype);
int dy_bn2_act_bwd(const void* dy, int64_t dy_ld, const void* u, int64_t u_ld, const void* v, int64_t v_ld, const float* scale_u,
                   const float* shift_u, const float* mean_u, const float* invstd_u, const float* gamma_u, const float* scale_v,
                   const float* shift_v, const float* mean_v, const float* invstd_v, const float* gamma_v, int act, void* du,
                   int64_t du_ld, void* dv, int64_t dv_ld, float* dgamma_u, float* dbeta_u, float* dgamma_v, float* dbeta_v,
                   float* workspace, int64_t workspace_elems, int64_t pixels, int C, int dtype, void* stream);

/* ----------------------------------------------------------------------------- pooling / resampling / concat
 * SPPF's 3 chained MaxPool2d(5,1,2) (block.py:331-338), ASFF's MaxPool2d(2,2) and max_pool2d(3,2,1) (block.py:58,85-86),
 * nn.Upsample / F.interpolate nearest (yolov8.yaml head; block.py:91,97,99), torch.cat (conv.py:473), x + y. */
/* argmax (optional) stores the window offset kh*k+kw of the FIRST maximum in scan order, one byte per output element */
int dy_maxpool_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, uint8_t* argmax, int N, int H, int W, int C, int k,
                   int stride, int pad, int Ho, int Wo, int dtype, void* stream);
/* dx (+)= adjoint of the pooling through argmax (gather form, no atomics) */
int dy_maxpool_bwd(const void* dy, int64_t dy_ld, const uint8_t* argmax, void* dx, int64_t dx_ld, int N, int H, int W, int C,
                   int k, int stride, int pad, int Ho, int Wo, int accumulate, int dtype, void* stream);
int dy_upsample_nearest_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, int N, int H, int W, int C, int scale,
                            int dtype, void* stream);
/* dx (+)= sum over the scale x scale children of dy */
int dy_upsample_nearest_bwd(const void* dy, int64_t dy_ld, void* dx, int64_t dx_ld, int N, int H, int W, int C, int scale,
                            int accumulate, int dtype, void* stream);
/* strided copy / add of `pixels` x C channel slabs (concat writes, chunk reads, gradient accumulation) */
int dy_copy2d(const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int64_t pixels, int C, int accumulate, int dtype,
              void* stream);
int dy_cast(const void* src, int src_dtype, void* dst, int dst_dtype, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------ PConv (FasterNet partial convolution)
 * Replaces PConv.forward_split_cat (U/nn/modules/conv.py:157-190, n_div=4): torch.split -> bias-free 3x3 s1 p1 nn.Conv2d on the
 * first c3 = C/4 channels -> torch.cat with the untouched C - c3 channels, and its autograd backward.  Views are NHWC over
 * N*H*W pixels with their own pixel strides; C and c3 (1..128) need no vector padding: only lanes [0, C) of a row are read or
 * written (the conv part reads [0, c3)), so the views may be channel slices of C2f / Concat buffers with live neighbours.
 * w / dw: f32 OIHW [c3][c3][3][3] (the state_dict layout; no packing). */
/* MFMA operand layout of w for the 16-bit route (dtype bf16 / f16, 16 <= c3 <= 128): wp holds
 * 9 * ceil(c3/32) * ceil(c3/16) * 512 elements of dtype; transposed = 1 packs the data gradient's (ci <-> co, flipped) weights */
int dy_pconv_pack(const float* w, void* wp, int c3, int transposed, int dtype, void* stream);
/* y[.., :c3] = conv3x3(x[.., :c3], w), y[.., c3:] = x[.., c3:]  (U/nn/modules/conv.py:185-190).  wp: dy_pconv_pack(transposed=0)
 * of w, required for 16-bit c3 >= 16 (ignored otherwise) */
int dy_pconv_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, const float* w, const void* wp, int N, int H, int W, int C, int c3,
                 int dtype, void* stream);
/* dx[.., :c3] = [dx +] conv3x3^T(dy[.., :c3], w) [+ add_src], dx[.., c3:] = [dx +] dy[.., c3:] [+ add_src]: the split/cat
 * adjoint; accumulate adds into C2f's gradient buffer, add_src (optional view of dx's shape) is PconvBottleneck's shortcut
 * gradient (U/nn/modules/block.py:587,606).  wp: dy_pconv_pack(transposed=1) of w, required for 16-bit c3 >= 16 */
int dy_pconv_dgrad(const void* dy, int64_t dy_ld, void* dx, int64_t dx_ld, const float* w, const void* wp, int N, int H, int W, int C,
                   int c3, int accumulate, const void* add_src, int64_t add_ld, int dtype, void* stream);
/* dw = sum over pixels of dy[.., :c3] x x[.., :c3] at each tap (overwrite), f32.  Deterministic: per-chunk partials in `scratch`
 * (>= 9*c3*c3 floats; more allows more chunks), summed in chunk order by a second launch; no atomics */
int dy_pconv_wgrad(const void* x, int64_t x_ld, const void* dy, int64_t dy_ld, float* dw, int N, int H, int W, int c3, float* scratch,
                   int64_t scratch_elems, int dtype, void* stream);
/* ------------------------------------------------------------------------------------ depthwise convolution (Ghost family)
 * Replaces nn.Conv2d(c, c, k, s, k // 2, groups = c, bias = False) inside DWConv (U/nn/modules/conv.py:95-99), GhostConv's cv2
 * (conv.py:142-154: cat(y, cv2(y)) with a 5x5 depthwise cv2) and GhostBottleneck's stride-2 stages (U/nn/modules/block.py:535-550), and
 * its autograd backward.  Channel multiplier 1, k in {3, 5, 7}, stride 1 or 2, pad = k / 2, dilation 1.  Views are NHWC with their own
 * pixel strides; x / dx are [N,H,W,C], y / dz are [N,Ho,Wo,C] with Ho = (H + 2 * (k / 2) - k) / stride + 1.  C >= 1 needs no vector
 * padding and no alignment beyond the element size: only lanes [0, C) of a pixel are read or written, so the views may be sibling
 * channel slices of one buffer (GhostConv's two halves) with live neighbours.  16-byte accesses are taken where every pointer, pixel
 * stride and C allow, 8-byte ones where only those allow, single elements otherwise.  w / dw: f32 [C][1][k][k] (the state_dict layout).
 * csrc/conv_route.h and dy_conv_desc are not involved. */
/* forward, two exclusive modes on the f32 accumulator:
 *   stats == NULL: y = act(acc * scale[c] + shift[c]) (scale NULL = 1, shift NULL = 0): eval with folded BatchNorm, or bias only;
 *   stats != NULL: y = raw acc (scale, shift NULL, act NONE) and (sum, sum of squares) of the accumulators are added per channel c to
 *                  stats[replica][c] / stats[replica][stats_c + c] of the zeroed double stats[DY_STATS_REPLICAS][2 * stats_c] that
 *                  dy_conv2d_fwd fills (stats_c >= C: the row width of the caller's padded buffer); dy_bn_finalize_valid,
 *                  dy_bn_act_fwd and dy_bn_act_bwd* then run unchanged. */
int dy_dwconv_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, const float* w, int N, int H, int W, int C, int k, int stride,
                  const float* scale, const float* shift, int act, double* stats, int stats_c, int dtype, void* stream);
/* data gradient, gather form (no atomics): dx[n,iy,ix,c] = [dx +] sum over taps with (iy + pad - ky) % stride == 0 and
 * (ix + pad - kx) % stride == 0 and both quotients in range of dz[n, (iy+pad-ky)/stride, (ix+pad-kx)/stride, c] * w[c,ky,kx] [+ add_src];
 * accumulate / add_src (optional view of dx's shape) as in dy_pconv_dgrad. */
int dy_dwconv_dgrad(const void* dz, int64_t dz_ld, void* dx, int64_t dx_ld, const float* w, int N, int H, int W, int C, int k, int stride,
                    int accumulate, const void* add_src, int64_t add_ld, int dtype, void* stream);
/* dw[c,ky,kx] = sum_{n,oy,ox} dz[n,oy,ox,c] * x[n, oy*stride - pad + ky, ox*stride - pad + kx, c] (overwrite), f32.  Deterministic:
 * per-block partials in `scratch` (>= C*k*k floats; more allows more blocks), summed in block order by a second launch; no atomics */
int dy_dwconv_wgrad(const void* x, int64_t x_ld, const void* dz, int64_t dz_ld, float* dw, int N, int H, int W, int C, int k, int stride,
                    float* scratch, int64_t scratch_elems, int dtype, void* stream);
/* dy_copy2d for views that are not whole aligned vectors: exactly lanes [0, C) of `pixels` pixels, any C >= 1, element alignment
 * (how a half of GhostConv's buffer is filled from / read into a vector-padded temporary when its width is not a vector multiple) */
int dy_copy2d_exact(const void* src, int64_t src_ld, void* dst, int64_t dst_ld, int64_t pixels, int C, int accumulate, int dtype,
                    void* stream);
/* ASFF blend (block.py:103-111): w = softmax(logits[.,3]); out = sum_i w_i * x_i */
int dy_asff_fuse_fwd(const void* x0, int64_t ld0, const void* x1, int64_t ld1, const void* x2, int64_t ld2,
                     const void* logits, int64_t ldl, void* out, int64_t ldo, int64_t pixels, int C, int dtype, void* stream);
int dy_asff_fuse_bwd(const void* dout, int64_t lddo, const void* x0, int64_t ld0, const void* x1, int64_t ld1,
                     const void* x2, int64_t ld2, const void* logits, int64_t ldl, void* dx0, int64_t ldd0, void* dx1,
                     int64_t ldd1, void* dx2, int64_t ldd2, void* dlogits, int64_t lddl, int64_t pixels, int C,
                     int acc0, int acc1, int acc2, int dtype, void* stream);

/* ------------------------------------------------------------------------------------- low-light front-end
 * lowlight_recovery.forward (U/nn/modules/llie.py:17-54) and the five filters of U/nn/modules/filtersB.py. */
/* NCHW f32 [B,3,H,W] -> NHWC with 8 channels (3 used, 5 zero) in `dtype`; optional bilinear resize to (Ho,Wo)
 * with align_corners=False (llie.py:43). Ho==H && Wo==W is a plain relayout. */
int dy_image_to_nhwc8(const float* x, int B, int H, int W, void* y, int Ho, int Wo, int dtype, void* stream);
/* adjoint of the bilinear resize: dx[B,3,H,W] f32 += resize^T(dy NHWC8 f32) */
int dy_resize_bwd(const float* dy_nhwc, int dy_ld, int B, int H, int W, int Ho, int Wo, float* dx, void* stream);
/* feat[B, feat_ld >= 15] -> params[B,8] = (omega, s_r, s_g, s_b, gamma, alpha, lambda, 0)  (filtersB.py regressors);
 * the backward writes all feat_ld columns of dfeat (zeros beyond the used slots) */
int dy_filter_params_fwd(const float* feat, int feat_ld, float* params, int B, void* stream);
/* dparams: f64 [B,8], zeroed by the caller and accumulated by dy_usm_bwd / dy_filters_pointwise_bwd with f64 atomics (a sum of f32
 * block partials that does not depend on their arrival order: the regressor's gradients repeat from run to run) */
int dy_filter_params_bwd(const float* feat, int feat_ld, const double* dparams, float* dfeat, int B, void* stream);
/* DeDark -> WB -> Gamma -> Contrast pointwise chain (filtersB.py:190-303) x -> s4 ; A [B,3] or NULL (0.8);
 * IcA [B,H,W] or NULL (0.5).  fast_math = 0: libm powf / division (f32 parity mode, comparable with torch.pow to ~1 ulp);
 * fast_math = 1: v_log_f32 / v_exp_f32 / v_rcp_f32 (~2e-6 relative; the throughput mode, 10x faster backward) */
int dy_filters_pointwise_fwd(const float* x, const float* params, const float* A, const float* IcA, float* s4, int B,
                             int H, int W, int fast_math, void* stream);
/* USM (filtersB.py:153-175) as a separable 25-tap gaussian with reflect halo: out = (s4 - blur)*lambda + s4.
 * Writes out NCHW f32 (optional), the NHWC8 copy in `dtype` for the stem conv (optional), and hp = s4 - blur (optional). */
int dy_usm_fwd(const float* s4, const float* params, float* out_nchw, void* out_nhwc8, float* hp, int B, int H, int W,
               int dtype, void* stream);
/* USM backward: ds4 = dout*(1+lambda) - lambda*blur^T(dout); dparams[b,6] += sum dout*hp.  dout is either NCHW f32
 * (dout_nchw) or, in `dtype`, a padded NHWC view with pixel stride dout_ld >= 3 / a planar [B,3,H,W] tensor when
 * dout_ld == 0 (dout_nhwc); exactly one of the two pointers is non-NULL. */
int dy_usm_bwd(const float* dout_nchw, const void* dout_nhwc, int dout_ld, const float* hp, const float* params, float* ds4,
               double* dparams, int B, int H, int W, int dtype, void* stream);
/* pointwise backward: recomputes the chain from x, consumes ds4, writes dx (overwrite or +=; NULL = not needed) and
 * accumulates dparams[b, 0..5] */
int dy_filters_pointwise_bwd(const float* x, const float* params, const float* A, const float* IcA, const float* ds4,
                             float* dx, double* dparams, int B, int H, int W, int accumulate, int fast_math, void* stream);

/* ------------------------------------------------------------------------------------- front-end filter chains
 * Any order of the reference's pointwise filters (U/nn/modules/filter_cfg.py:17-75 builds the list, llie.py:51-52 applies it in
 * order), ToneFilter (filtersB.py:262-286) among them.  The default chain keeps dy_filters_pointwise_fwd/bwd. */
#define DY_TONE_STEPS 8          /* cfg.curve_steps (filter_cfg.py:28): features 5..12 (tone_begin_param, :23) */
#define DY_CHAIN_MAX 5           /* pointwise stages of a chain: each filter at most once; UsmFilter stays with dy_usm_* */
#define DY_FILTER_DEDARK 1       /* DF  filtersB.py:178-216 */
#define DY_FILTER_WB 2           /* W   filtersB.py:237-259 */
#define DY_FILTER_GAMMA 3        /* G   filtersB.py:219-233 */
#define DY_FILTER_TONE 4         /* T   filtersB.py:262-286 */
#define DY_FILTER_CONTRAST 5     /* Ct  filtersB.py:289-303 */
/* ToneFilter.filter_param_regressor (filtersB.py:271-274, tanh_range(0.5, 2) of filter_cfg.py:34):
 * tone[b, i] = tanh(feat[b, 5 + i]) * 0.75 + 1.25, i < 8.  Columns outside 5..12 are not read. */
int dy_tone_params_fwd(const float* feat, int feat_ld, float* tone, int B, void* stream);
/* its adjoint: writes columns 5..12 of dfeat ONLY (run it after dy_filter_params_bwd, which zeroes the row); dtone f64 [B,8] is
 * zeroed by the caller and accumulated by dy_filter_chain_bwd */
int dy_tone_params_bwd(const float* feat, int feat_ld, const double* dtone, float* dfeat, int B, void* stream);
/* The pointwise part of a filter chain in one pass, x [B,3,H,W] f32 -> y (replaces the loop of llie.py:51-52 over the filters of
 * filter_cfg.py:17-75 up to UsmFilter).  `chain`: one DY_FILTER_* code per 4 bits, first stage in the lowest bits, 0 ends it;
 * 1..DY_CHAIN_MAX stages, none repeated.  Each stage sees the output of the one before it; the contrast filter's per-row luminance
 * comes from columns 0..2 of ITS input and the stages after it act on the multiplied row.  params [B,8] as dy_filter_params_fwd
 * writes them; tone [B,8] (NULL without a tone stage); A [B,3] or NULL (0.8); IcA [B,H,W] or NULL (0.5).  W >= 3 with a contrast
 * stage, else W >= 1.  fast_math as dy_filters_pointwise_fwd. */
int dy_filter_chain_fwd(const float* x, const float* params, const float* tone, const float* A, const float* IcA,
                        unsigned chain, float* y, int B, int H, int W, int fast_math, void* stream);
/* Backward: recomputes the chain from x, writes dx (overwrite or +=; NULL = not needed) and accumulates dparams[b, 0..5] and
 * dtone[b, 0..7] (f64 atomics, as dy_filters_pointwise_bwd; dtone may be NULL without a tone stage).  The upstream gradient is
 * either NCHW f32 (dy_nchw: what dy_usm_bwd writes) or, for a chain that ends without UsmFilter, in `dtype` a padded NHWC view
 * with pixel stride dy_ld >= 3 / a planar [B,3,H,W] tensor when dy_ld == 0 (dy_any: the two layouts dy_usm_bwd accepts);
 * exactly one of the two pointers is non-NULL. */
int dy_filter_chain_bwd(const float* x, const float* params, const float* tone, const float* A, const float* IcA,
                        unsigned chain, const float* dy_nchw, const void* dy_any, int dy_ld, int dtype, float* dx,
                        double* dparams, double* dtone, int B, int H, int W, int accumulate, int fast_math, void* stream);

/* ------------------------------------------------------------------------------------------ detection loss
 * v8DetectionLoss / RcoveryDetectionLoss (U/utils/loss.py:103-193,388-416), TaskAlignedAssigner (U/utils/tal.py),
 * bbox_iou CIoU (U/utils/metrics.py:75-128), make_anchors / dist2bbox (tal.py:246-271). */
typedef struct {
  const void* map[3]; /* Detect train outputs, NHWC views [B, h_l*w_l, no], no = 64+nc */
  int64_t map_ld[3];
  int h[3], w[3];
  float stride[3];
  int B, nc, n_levels, dtype;
} dy_det_maps;

/* Four-level heads: Detect on P2..P5 (strides 4/8/16/32) or P3..P6 (8..64), i.e. nl = 4 in Detect (U/nn/modules/head.py:19-45)
 * with make_anchors walking all four maps (U/utils/tal.py:246-258).  dy_det_maps4 starts with a dy_det_maps (n_levels = 4)
 * and appends the fourth map; pass &x.base wherever a dy_det_maps* is taken.  The entry points read the tail only when
 * base.n_levels == 4, so 1-3 level callers keep passing a plain dy_det_maps.  Anchors are numbered level by level in the
 * order of the maps, whatever their strides. */
#define DY_DET_MAX_LEVELS 4
typedef struct {
  dy_det_maps base;
  const void* map3; /* fourth level: NHWC view [B, h3*w3, no] */
  int64_t map_ld3;
  int h3, w3;
  float stride3;
} dy_det_maps4;

/* group targets per image: rows (batch_idx, cls, cx, cy, w, h normalised) -> gt[B][n_max][5] = (cls, x1,y1,x2,y2 px),
 * counts[B]; order within an image is preserved (loss.py:124-139). */
int dy_loss_prepare_targets(const float* batch_idx, const float* cls, const float* bboxes, int n_targets, int B,
                            int n_max, float img_w, float img_h, float* gt, int32_t* counts, void* stream);
/* decode (loss.py:141-146): pred_boxes[B,A,4] xyxy in grid units, via softmax over 16 bins . arange */
int dy_loss_decode(const dy_det_maps* m, float* pred_boxes, void* stream);
/* task-aligned assignment (tal.py:83-127; topk 10, alpha .5, beta 6).  Scratch: work_f [2*R + 2*B*n_max] floats,
 * work_i [R] int32, work_b [R] bytes with R = B*n_max*A.  Outputs: target_gt_idx[B,A] i32, fg_mask[B,A] u8,
 * norm[B,A] f32 (= target_scores at the assigned label, 0 elsewhere), target_label[B,A] i32, target_box[B,A,4] f32 (px).
 * top-10 ties follow std::partial_sort as torch.topk does on CPU for A >= 640. */
int dy_tal_assign(const dy_det_maps* m, const float* pred_boxes, const float* gt, const int32_t* counts, int n_max,
                  float* work_f, int32_t* work_i, uint8_t* work_b, int32_t* target_gt_idx, uint8_t* fg_mask, float* norm,
                  int32_t* target_label, float* target_box, void* stream);
/* The same assigner on TaskAlignedAssigner.forward's own arguments (U/utils/tal.py:84-132): class probabilities pd_scores
 * [B,A,nc] f32, decoded boxes pd_bboxes [B,A,4] f32 in pixels, anchor points [A,2] in pixels; gt rows = (label, x1,y1,x2,y2) with
 * masked-out rows zeroed, counts[b] = rows of image b to consider.  Outputs as dy_tal_assign. */
int dy_tal_assign_decoded(const float* pd_scores, const float* pd_bboxes, const float* anc_points, const float* gt,
                          const int32_t* counts, int B, int A, int nc, int n_max, float* work_f, int32_t* work_i, uint8_t* work_b,
                          int32_t* target_gt_idx, uint8_t* fg_mask, float* norm, int32_t* target_label, float* target_box,
                          void* stream);
/* ---- SCConv pieces of MFRU (reference ultralytics/nn/modules/conv.py:323-440, block.py:164-217); NHWC views, HW = pixels per image ----
 * dy_chan_moments: out[n][c][2] += (sum x, sum x^2) over the pixels of image n (out zeroed by the caller): the group statistics
 * of GroupBatchnorm2d (conv.py:337-343) and the AdaptiveAvgPool2d(1) of CRU (conv.py:403,415). */
int dy_chan_moments(const void* x, int64_t ld, int N, int64_t HW, int C, double* out, int dtype, void* stream);
/* SRU.forward (conv.py:360-378): group norm over `groups` channel groups per image (torch.std: unbiased; eps added to std),
 * gate sigmoid(gn * gamma / sum(gamma)) >= 0.5, cross reconstruction y[c] = m[c] gn[c] + (1 - m[c']) gn[c'], c' = c +- C/2.
 * moments = dy_chan_moments(x). */
int dy_sru_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, int N, int64_t HW, int C, int groups, const double* moments,
               const float* gamma, const float* beta, float eps, int dtype, void* stream);
/* its backward: dx (written), red[n][c][2] += (sum dgn, sum dgn * xhat) (zeroed by the caller) from which the caller takes
 * d gamma[c] = sum_n red[n][c][1], d beta[c] = sum_n red[n][c][0] (the gate has no gradient). */
int dy_sru_bwd(const void* x, int64_t x_ld, const void* dy, int64_t dy_ld, void* dx, int64_t dx_ld, int N, int64_t HW, int C, int groups,
               const double* moments, const float* gamma, const float* beta, float eps, double* red, int dtype, void* stream);
/* CRU tail (conv.py:413-417): o [.., 2C] = cat(Y1, Y2); s = softmax over the 2C channels of mean_pixels(o) per image;
 * res[c] = o[c] s[c] + o[c + C] s[c + C].  moments = dy_chan_moments(o) with 2C channels. */
int dy_cru_fuse_fwd(const void* o, int64_t o_ld, void* res, int64_t r_ld, int N, int64_t HW, int C, const double* moments, int dtype,
                    void* stream);
/* its backward: dout [.., 2C] (written); ds[n][k][2] scratch (zeroed by the caller; slot 0 = sum_pixels dres[c(k)] o[k]). */
int dy_cru_fuse_bwd(const void* o, int64_t o_ld, const void* dres, int64_t d_ld, void* dout, int64_t do_ld, int N, int64_t HW, int C,
                    const double* moments, double* ds, int dtype, void* stream);
/* ------------------------------------------------------------------------------------ CRU convolutions (SCConv C2f family)
 * The convolutions of CRU.forward (U/nn/modules/conv.py:406-417) at any width C % 16 == 0.  One "CRU conv" over NHWC views of
 * M = B*H*W pixels, G groups (1 or 2) of N output channels:
 *   y[m][g N + n] = bias[g N + n] + sum_{tap < 9, ci < C3} x[m + off(tap)][g C3 + ci] w3[g N + n][ci][tap] + sum_{c < C1} x[m][c] w1[g N + n][c]
 * (3x3 pad 1 stride 1; C3 == 0: a plain 1x1 with G == 1; C3 > 0: G C3 == C1).  Y1 = GWC(up') + PWC1(up') is (G, N, C3, C1) =
 * (2, C/2, C/8, C/4) in one accumulator; squeeze1 / squeeze2 / PWC2 are C3 == 0.  x has C1 channels, y has G N; exactly those lanes
 * of a pixel are read / written (element alignment is enough), so both may be channel slices of wider buffers with live neighbours.
 * w3: f32 [G N][C3][3][3], w1: f32 [G N][C1], bias: f32 [G N] or NULL (the state_dict layouts).
 * wp: G N (9 C3 + C1) elements of dtype, 16-byte aligned: the MFMA operand image of (w3, w1); transposed = 1 packs the data
 * gradient's (input <-> output, taps flipped) image. */
int dy_cru_conv_pack(const float* w3, const float* w1, void* wp, int G, int N, int C3, int C1, int transposed, int dtype, void* stream);
/* wp = dy_cru_conv_pack(transposed = 0) */
int dy_cru_conv_fwd(const void* x, int64_t x_ld, const void* wp, const float* bias, void* y, int64_t y_ld, int B, int H, int W, int G, int N,
                    int C3, int C1, int dtype, void* stream);
/* dx [.., C1] = [dx +] GWC^T(dy) + PWC1^T(dy), gather form; wp = dy_cru_conv_pack(transposed = 1) */
int dy_cru_conv_dgrad(const void* dy, int64_t dy_ld, const void* wp, void* dx, int64_t dx_ld, int B, int H, int W, int G, int N, int C3,
                      int C1, int accumulate, int dtype, void* stream);
/* dw3 / db / dw1 (each nullable; overwrite, f32, the layouts above).  Deterministic: the pixels are split into ranges by the
 * shape and scratch_elems alone, partial tiles go to `scratch` (>= G N (9 C3 + C1 + 1) floats; more allows more ranges) and a second
 * launch adds them in range order; no atomics */
int dy_cru_conv_wgrad(const void* x, int64_t x_ld, const void* dy, int64_t dy_ld, float* dw3, float* db, float* dw1, int B, int H, int W,
                      int G, int N, int C3, int C1, float* scratch, int64_t scratch_elems, int dtype, void* stream);
/* ------------------------------------------------------------------------------------ fused multi-head attention (C3TR family)
 * The nn.MultiheadAttention call of TransformerLayer.forward (U/nn/modules/transformer.py:109,115; torch's
 * multi_head_attention_forward between its in-projection and out_proj, no masks, dropout 0):
 *   O[b, i, h D + c] = sum_j softmax_j(scale * Q[b, i, h, :] . K[b, j, h, :]) * V[b, j, h D + c]
 * q / k / v / o: token-major views [B L][ld] of the dtype, head h = channels [h D, (h + 1) D); exactly the H D channels of a token
 * are read / written (element alignment is enough), so the views may be channel slices of one [B, L, 3 C] buffer with live
 * neighbours.  L >= 1, H >= 1, D % 8 == 0, 8 <= D <= 128; anything else is an argument error.
 * lse (nullable; training): f32 [B][H][L], log sum_j exp(scale * Q.K_j).  Softmax statistics are f32; in the 16-bit dtypes P is
 * rounded to the dtype before P V. */
int dy_attn_fwd(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, void* o, int64_t o_ld, float* lse, int B,
                int L, int H, int D, float scale, int dtype, void* stream);
/* backward of dy_attn_fwd in the flash form (P = exp(scale S - lse) recomputed per tile, no L x L tensor in global memory):
 * delta_i = sum_c dO_ic O_ic per head, dV = P^T dO, dS = P o (dO V^T - delta), dQ = scale dS K, dK = scale dS^T Q.  dq / dk / dv
 * (overwritten) follow the view rules above.  Deterministic: dQ is summed by the workgroup that owns the query tile, dK / dV by the
 * one that owns the key tile; no atomics, no hand-off between workgroups. */
int dy_attn_bwd(const void* q, int64_t q_ld, const void* k, int64_t k_ld, const void* v, int64_t v_ld, const void* o, int64_t o_ld,
                const void* dout, int64_t do_ld, const float* lse, void* dq, int64_t dq_ld, void* dk, int64_t dk_ld, void* dv, int64_t dv_ld,
                int B, int L, int H, int D, float scale, int dtype, void* stream);
/* ------------------------------------------------------------------------------------ transformer encoder layer (AIFI family)
 * The element-wise side of TransformerEncoderLayer.forward_post / AIFI.forward (U/nn/modules/transformer.py:53-62, 88-109).
 * All views are token matrices [rows][ld] of the dtype, ld >= C, C % 4 == 0; exactly C channels of a row are touched, so a view may
 * be a channel slice with live neighbours.  16-byte accesses where C, every ld and every base allow, element accesses otherwise.
 *
 * y = LayerNorm(a + b) (transformer.py:59-60 `src = src + self.dropout1(src2); src = self.norm1(src)`, :61-62 for norm2):
 *   z = a + b (b nullable: z = a), y = (z - mean(z)) rsqrt(var(z) + eps) gamma + beta, biased variance of the centred values, f32
 * statistics; z is never written.  stats (nullable; training): f32 [rows][2] = mean, rstd.  4 <= C <= DY_LN_MAX_C. */
#define DY_LN_MAX_C 2048
#define DY_LN_MAX_PARTS 512
int dy_add_layernorm_fwd(const void* a, int64_t a_ld, const void* b, int64_t b_ld, const float* gamma, const float* beta, void* y,
                         int64_t y_ld, float* stats, int64_t rows, int C, float eps, int dtype, void* stream);
/* backward: z^ recomputed from a, b and stats; g = dy gamma, dz = rstd (g - mean(g) - z^ mean(g z^)) is the gradient of a AND of b
 * (accumulate != 0: added into dz).  dgamma = sum_rows dy z^, dbeta = sum_rows dy (both nullable, together): per-workgroup f32
 * partials over row ranges fixed by the shape, added by a second kernel in an order fixed by their count; no atomics, identical
 * bytes on every run.  scratch: 2 C min(DY_LN_MAX_PARTS, ceil(rows / (C > 1024 ? 1 : 4))) floats. */
int dy_add_layernorm_bwd(const void* a, int64_t a_ld, const void* b, int64_t b_ld, const float* stats, const float* gamma, const void* dy,
                         int64_t dy_ld, void* dz, int64_t dz_ld, int accumulate, float* dgamma, float* dbeta, float* scratch,
                         int64_t scratch_elems, int64_t rows, int C, int dtype, void* stream);
/* exact GELU, nn.GELU()'s default (transformer.py:61 `self.act(self.fc1(src))`): y = 0.5 u (1 + erf(u / sqrt 2));
 * du = dy (Phi(u) + u phi(u)); f32 arithmetic */
int dy_gelu_fwd(const void* u, int64_t u_ld, void* y, int64_t y_ld, int64_t pixels, int C, int dtype, void* stream);
int dy_gelu_bwd(const void* u, int64_t u_ld, const void* dy, int64_t dy_ld, void* du, int64_t du_ld, int64_t pixels, int C, int dtype,
                void* stream);
/* y[b][l][c] = x[b][l][c] + pos[l][c] (transformer.py:49-51 with_pos_embed; AIFI.forward :103-105): pos is the dense [L][C] table
 * in the dtype, built on the host; the sum is taken in f32 and rounded once */
int dy_add_pos(const void* x, int64_t x_ld, const void* pos, void* y, int64_t y_ld, int B, int L, int C, int dtype, void* stream);
/* CIoU of n box pairs, xyxy f32 (reference ultralytics/utils/metrics.py:75-128 bbox_iou(b1, b2, xywh=False, CIoU=True): eps added to
 * h only, alpha constant in the backward); grad_b1 (nullable) [n,4] = d out[i] / d b1[i]. */
int dy_bbox_ciou(const float* b1, const float* b2, int64_t n, float* out, float* grad_b1, void* stream);
/* Every mode of the same function (metrics.py:75-128): kind 0 IoU, 1 GIoU, 2 DIoU, 3 CIoU; xywh != 0: (cx, cy, w, h) boxes, w / h used
 * as given (:95-99), else xyxy with eps added to h only (:100-104).  grad_b1 (nullable) [n,4] = d out[i] / d b1[i] in b1's own
 * coordinates (b2 is a target; CIoU's alpha constant as under the reference's no_grad). */
int dy_bbox_iou(const float* b1, const float* b2, int64_t n, int xywh, int kind, float eps, float* out, float* grad_b1, void* stream);
/* Distribution focal loss (reference ultralytics/utils/loss.py:75-84 BboxLoss._df_loss): pred_dist [n_boxes*4, 16] logits,
 * target [n_boxes, 4] in [0, 15); out [n_boxes] = mean over the 4 sides; grad (nullable) = d sum(out) / d pred_dist. */
int dy_dfl_loss(const float* pred_dist, const float* target, int64_t n_boxes, float* out, float* grad, void* stream);
/* loss sums: acc[0]=sum target_scores, acc[1]=BCE sum, acc[2]=sum (1-ciou)*w, acc[3]=sum dfl*w (acc zeroed first) */
int dy_loss_fwd(const dy_det_maps* m, const float* pred_boxes, const uint8_t* fg_mask, const float* norm,
                const int32_t* target_label, const float* target_box, double* acc, void* stream);
/* finish: loss_out[0] = (box*hb + cls*hc + dfl*hd)*B + lrl*rec ; items[3] = (box*hb, cls*hc + lrl*rec, dfl*hd) */
int dy_loss_finish(const double* acc, const float* recovery, float hyp_box, float hyp_cls, float hyp_dfl, float lrl,
                   int B, float* loss_out, float* items, void* stream);
/* gradient wrt the maps (written in `dtype`, every element), scaled by *grad_out (device scalar); dmap / dmap_ld hold
 * m->n_levels entries (up to DY_DET_MAX_LEVELS) */
int dy_loss_bwd(const dy_det_maps* m, void* const* dmap, const int64_t* dmap_ld, const float* pred_boxes,
                const uint8_t* fg_mask, const float* norm, const int32_t* target_label, const float* target_box,
                const double* acc, const float* grad_out, float hyp_box, float hyp_cls, float hyp_dfl, void* stream);
/* Detect eval decode (head.py:66-93): y[B, 4+nc, A] f32 = cat(xywh*stride, sigmoid(cls)) */
int dy_detect_decode(const dy_det_maps* m, float* y, void* stream);
/* the same into y[B, rows, A] f32, rows >= 4+nc (rows past 4+nc are not written: the Pose head's keypoint rows, dy_pose_kpt_decode) */
int dy_detect_decode_rows(const dy_det_maps* m, float* y, int rows, void* stream);
/* ---- test-time augmentation for detect (U/nn/tasks.py:303-340 DetectionModel._predict_augment; csrc/tta.hip, csrc/loss.hip) ----------
 * dy_tta_scale_img: the input of one augmented pass, scale_img(x.flip(flip), ratio, gs) (tasks.py:310, U/utils/torch_utils.py:270-279), in
 * one pass over the output: x f32 NCHW [B][C][H][W] -> out f32 NCHW [B][C][Hp][Wp].  flip 0 none, 2 up-down, 3 left-right (folded into
 * the source index).  Pixels inside (hs, ws) are the bilinear resize of the flipped image with the arithmetic documented at
 * dy_seg_mask_upsample (scale = in / out in f32, src = scale * (dst + 0.5) - 0.5 clamped at 0, upper tap clamped to the last row /
 * column, wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d)); the others (right, bottom) are 0.447.  The caller computes
 * hs = int(H * ratio), ws = int(W * ratio), Hp = ceil(H * ratio / gs) * gs, Wp likewise (in doubles, as the reference does) and passes
 * them in.  (hs, ws) == (H, W): the mirrored pixels themselves, bit for bit.  out 16-byte aligned, not x.  No atomics. */
int dy_tta_scale_img(const float* x, int B, int C, int H, int W, int hs, int ws, int Hp, int Wp, int flip, float* out, void* stream);
/* dy_detect_decode of one augmented pass written into its column window of the merged y [B][4+nc][a_total] f32, with _descale_pred
 * (tasks.py:320-329) and _clip_augmented (:331-340) applied: anchor a in [a_lo, a_hi) of the pass goes to column col0 + a - a_lo; box
 * rows = (decoded * stride) / scale in f32 (a division, as the reference's `p[:, :4] /= scale`), then row 0 = img_w - x for flip 3 or
 * row 1 = img_h - y for flip 2, img_h / img_w being those of the ORIGINAL image (not of the padded pass); class rows = sigmoid,
 * unchanged.  Anchors outside [a_lo, a_hi) are not computed; columns outside the window are not written. */
int dy_detect_decode_tta(const dy_det_maps* m, float* y, int64_t a_total, int col0, int a_lo, int a_hi, float scale, int flip,
                         float img_h, float img_w, void* stream);
/* ------------------------------------------------------------------------------------------------ NMS
 * non_max_suppression (U/utils/ops.py:144-278; called from U/models/yolo/detect/val.py:62-70) for the whole batch.
 * pred [B, 4+nc, A] f32 = Detect's eval output (xywh px + class scores).  Three stages:
 *  dy_nms_candidates: keys[b, slot] = (~bits(score) << 32) | (anchor*nc + cls) for every candidate (score > conf_thres; every
 *                     (anchor, cls) pair when multi_label && nc > 1 (ops.py:244-246), else the anchor's best class (:248-249));
 *                     counts[b] = number of candidates (may exceed cap = slots per image; the excess is dropped).
 *  dy_nms_sort:       per-image ascending key sort == stable descending-score order of the reference's candidate list.
 *                     workspace == NULL: only *workspace_bytes is written (size query).
 *  dy_nms_greedy:     first min(count, max_nms) candidates (ops.py:255-256), boxes + cls*max_wh unless agnostic (:258-259),
 *                     greedy suppression IoU > iou_thres (torchvision.ops.nms semantics, :261), first max_det kept (:262).
 *                     out [B, max_det, 6] = (x1,y1,x2,y2,conf,cls); keep_idx [B, max_det] = anchor*nc + cls of each kept row;
 *                     out_counts[B].  boxes_ws: B*max_nms*4 floats (16-byte aligned), dead_ws: B*max_nms bytes.
 * The wall-clock break of ops.py:274-276 is deliberately not reproduced. */
int dy_nms_candidates(const float* pred, int B, int nc, int A, float conf_thres, int multi_label, uint64_t* keys, int* counts,
                      int64_t cap, void* stream);
int dy_nms_sort(const uint64_t* keys, uint64_t* keys_sorted, const int* counts, int B, int64_t cap, void* workspace,
                size_t* workspace_bytes, void* stream);
int dy_nms_greedy(const float* pred, const uint64_t* keys_sorted, const int* counts, int B, int nc, int A, int64_t cap,
                  double iou_thres, int max_nms, int max_det, float max_wh, int agnostic, float* boxes_ws, uint8_t* dead_ws,
                  float* out, int64_t* keep_idx, int* out_counts, void* stream);

/* preprocess_batch tensor part (U/models/yolo/detect/train.py:70-111): u8 NCHW -> f32 /255 (^gamma), mse accumulators */
int dy_preprocess_batch(const uint8_t* img, float* img_out, float* clean_out, float dark_param, int lowlight, int dedark,
                        double* mse_acc, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------ optimizer
 * BaseTrainer.optimizer_step (U/engine/trainer.py:459-467): clip_grad_norm_(10.0) + SGD(nesterov) / AdamW step +
 * ModelEMA.update (U/utils/torch_utils.py:360-371) on flat f32 parameter ranges. */
int dy_sumsq(const float* g, int64_t n, double* acc, void* stream);
/* One flat buffer holds every trainable parameter; group_id[i] in {0,1,2} selects (lr, weight_decay) of the reference's three
 * parameter groups (decayed weights / BN weights / biases; NULL = group 0).  g is multiplied by grad_scale and by the clip
 * coefficient min(1, max_norm / (sqrt(*sumsq) + 1e-6)) when sumsq != NULL; ema may be NULL. */
int dy_sgd_step(float* p, const float* g, float* mom_buf, float* ema, const uint8_t* group_id, float lr0, float lr1, float lr2,
                float wd0, float wd1, float wd2, float momentum, int nesterov, float ema_decay, const double* sumsq,
                float max_norm, float grad_scale, int64_t n, void* stream);
int dy_adamw_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, const uint8_t* group_id, float lr0,
                  float lr1, float lr2, float wd0, float wd1, float wd2, float beta1, float beta2, float eps, int step,
                  float ema_decay, const double* sumsq, float max_norm, float grad_scale, int64_t n, void* stream);
/* fp16 training (reference AMP: torch.cuda.amp.GradScaler, U/engine/trainer.py:221,330,340,459-467).  The loss gradient is
 * multiplied by loss_scale[0] before the backward pass; the *_scaled steps divide it out again (clip on the TRUE norm), and leave
 * parameters and optimizer state untouched when *sumsq is inf / NaN (the EMA is still updated, as trainer.optimizer_step does).
 * dy_loss_scale_update then applies GradScaler.update to state = {scale, consecutive finite steps, overflowed steps in total} (three
 * floats): scale *= backoff after an overflow, scale *= growth after `interval` finite steps.  dy_adamw_step_scaled takes its bias
 * correction at step - state[2]: torch's Adam does not advance on the steps GradScaler skips.  loss_scale == NULL: exactly
 * dy_sgd_step / dy_adamw_step. */
int dy_sgd_step_scaled(float* p, const float* g, float* mom_buf, float* ema, const uint8_t* group_id, float lr0, float lr1, float lr2,
                       float wd0, float wd1, float wd2, float momentum, int nesterov, float ema_decay, const double* sumsq,
                       float max_norm, float grad_scale, const float* loss_scale, int64_t n, void* stream);
int dy_adamw_step_scaled(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, const uint8_t* group_id, float lr0,
                         float lr1, float lr2, float wd0, float wd1, float wd2, float beta1, float beta2, float eps, int step,
                         float ema_decay, const double* sumsq, float max_norm, float grad_scale, const float* loss_scale, int64_t n,
                         void* stream);
int dy_loss_scale_update(float* state, const double* sumsq, float growth, float backoff, int interval, void* stream);
/* The other optimizers of build_optimizer (U/engine/trainer.py:648-651): torch.optim.Adam / Adamax / NAdam / RAdam with
 * betas = (momentum, 0.999), and RMSprop(momentum = momentum); the update rules are torch's _single_tensor_adam / _adamax / _nadam /
 * _radam / _rmsprop (torch.optim), weight decay as L2 (added to the gradient), no amsgrad, not centered.  One call replaces
 * clip_grad_norm_ + optimizer.step() + ema.update() like the entries above, with the same group_id / sumsq / grad_scale / loss_scale /
 * ema contract.  buf1 / buf2 are the two per-element state buffers:
 *   DY_OPT_ADAM, DY_OPT_NADAM, DY_OPT_RADAM: exp_avg / exp_avg_sq     DY_OPT_ADAMAX: exp_avg / exp_inf
 *   DY_OPT_RMSPROP: square_avg / momentum_buffer (beta1 = momentum, beta2 = alpha; momentum == 0 leaves buf2 alone)
 * momentum_decay is NAdam's (0.004), ignored by the other rules.
 * The scalar state of the optimizer lives on the device in *state (64 bytes, 8-byte aligned; the caller sets step = 0 and
 * mu_product = 1 before the first step and may read or write both between steps, e.g. for a checkpoint).  A one-thread launch ahead of
 * the element kernel decides the overflow skip from *sumsq and loss_scale, advances `step` (steps really TAKEN: a skipped step leaves
 * step, mu_product, the parameters and both buffers untouched, only the EMA moves) and NAdam's running mu_product, and computes the
 * step's uniform scalars in double precision; the element kernel reads them as floats.  No host synchronisation. */
enum { DY_OPT_ADAM = 0, DY_OPT_ADAMAX = 1, DY_OPT_NADAM = 2, DY_OPT_RADAM = 3, DY_OPT_RMSPROP = 4 };
typedef struct dy_optim_state {
  double step;        /* optimizer steps taken so far (torch's state['step']) */
  double mu_product;  /* NAdam: product of mu_1 .. mu_step, rounded to f32 after every step as torch's f32 state['mu_product'] is; 1 before the first step */
  float grad_coef;    /* written every call: clip coefficient * grad_scale / loss scale of this step */
  int32_t skipped;    /* written every call: 1 = this step found an inf / NaN gradient and was skipped */
  float c[4];         /* written on a taken step.  Adam: {1 - beta1^t, sqrt(1 - beta2^t)}; Adamax: {1 - beta1^t};
                         NAdam: {1 - beta2^t, (1 - mu_t) / (1 - mu_product_t), mu_{t+1} / (1 - mu_product_t * mu_{t+1})};
                         RAdam: {1 - beta1^t, sqrt(1 - beta2^t), rectification r_t, rho_t > 5 ? 1 : 0}; RMSProp: none */
  float reserved[6];
} dy_optim_state;
int dy_optim_step(int rule, float* p, const float* g, float* buf1, float* buf2, float* ema, const uint8_t* group_id, float lr0,
                  float lr1, float lr2, float wd0, float wd1, float wd2, double beta1, double beta2, double eps,
                  double momentum_decay, float ema_decay, const double* sumsq, float max_norm, float grad_scale,
                  const float* loss_scale, dy_optim_state* state, int64_t n, void* stream);
/* ema = decay*ema + (1-decay)*src (EMA of the BatchNorm running buffers) */
int dy_ema_lerp(float* ema, const float* src, float decay, int64_t n, void* stream);
/* acc += g: gradient accumulation over `accumulate` batches (nbs / batch, U/engine/trainer.py:248,340-342) */
int dy_grad_accumulate(float* acc, const float* g, int64_t n, void* stream);
/* Merged entries: exactly the launches of the separate calls, behind ONE foreign-function call (the training step of BASELINE
 * configs[1] is ~700 launches issued from Python and had become host-bound).
 *   dy_conv2d_bn_act_fwd  = dy_conv2d_fwd(d: dst = raw z, stats) + dy_bn_finalize + dy_bn_act_fwd(z -> y); aff = 4*Cd floats
 *                           [scale | shift | mean | invstd] (kept for the backward pass)
 *   dy_bn_act_bwd         = dy_bn_act_bwd_reduce + dy_bn_act_bwd_apply with the same aff buffer
 *   dy_conv2d_wgrad_forked = dy_stream_fork(wait_for, stream) + dy_conv2d_wgrad on `stream` */
int dy_conv2d_bn_act_fwd(const dy_conv_desc* d, int64_t count, const float* gamma, const float* beta, float* running_mean,
                         float* running_var, float momentum, float eps, float* aff, int act, const void* residual, int64_t res_ld,
                         void* y, int64_t y_ld, void* stream);
int dy_bn_act_bwd(const void* dy, int64_t dy_ld, const void* z, int64_t z_ld, const float* aff, const float* gamma, int act,
                  double* sums, void* dz, int64_t dz_ld, float* dgamma, float* dbeta, int64_t pixels, int C, int dtype, void* stream);
/* ... with channel padding (see dy_bn_finalize_valid): C = Cd of the descriptor / of the views, C_valid real channels */
int dy_conv2d_bn_act_fwd_valid(const dy_conv_desc* d, int64_t count, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, float* aff, int act, const void* residual,
                               int64_t res_ld, void* y, int64_t y_ld, int C_valid, void* stream);
int dy_bn_act_bwd_valid(const void* dy, int64_t dy_ld, const void* z, int64_t z_ld, const float* aff, const float* gamma, int act,
                        double* sums, void* dz, int64_t dz_ld, float* dgamma, float* dbeta, int64_t pixels, int C, int C_valid,
                        int dtype, void* stream);
int dy_conv2d_wgrad_forked(void* wait_for, const void* x, int64_t x_ld, int N, int Hi, int Wi, int Cin_pad, const void* dz,
                           int64_t dz_ld, int Ho, int Wo, int Cout_pad, int KH, int KW, int stride, int pad, int dil, int Cout,
                           int Cin, float* scratch, int64_t scratch_elems, float* g_oihw, int dtype, void* stream);

/* Stream plumbing of the backward pass (no counterpart in the single-stream reference): `to` waits for everything issued so far
 * on `from` (hipEventRecord on an internal ring of timing-free events + hipStreamWaitEvent; no host synchronisation).  Used to
 * run the weight gradients of a conv on a second HIP stream next to its dgrad -> BatchNorm-backward chain. */
int dy_stream_fork(void* from, void* to);
int dy_frontend_init(void); /* uploads the gaussian taps (call once per process, outside graph capture) */

/* ---- device-side input pipeline ----------------------------------------------------------------------------------
 * The pixel work of the reference's dataloader workers (ultralytics/data/augment.py:118-603,745-751, data/base.py:142-169) and of the
 * trainer's dark-channel loop (models/yolo/detect/train.py:42-68).  Images are uint8 HWC BGR (cv2.imread layout) in device memory. */
typedef struct dy_aug_sample {
  const uint8_t* src[4];   /* the (up to) four images of a mosaic, at their load_image size; one image for the letterbox case */
  int32_t sh[4], sw[4];
  int64_t pitch[4];        /* bytes per row */
  int32_t rect[4][6];      /* x1a, y1a, x2a, y2a on the canvas, x1b, y1b in the image (Mosaic._mosaic4, augment.py:166-188) */
  int32_t n_src, canvas_h, canvas_w;
  int32_t hsv, flipud, fliplr;
  double minv[6];          /* inverse of RandomPerspective's 2x3 matrix as cv::warpAffine inverts it (output -> canvas) */
  uint8_t lut[3][256];     /* RandomHSV's hue / saturation / value tables (augment.py:493-497) */
} dy_aug_sample;
/* cv2.resize(INTER_LINEAR) of load_image (base.py:152-157). */
int dy_aug_resize_u8(const uint8_t* src, int sh, int sw, int64_t src_pitch, uint8_t* dst, int dh, int dw, int64_t dst_pitch, void* stream);
/* cv2.resize(INTER_AREA) of load_image for a validation image that shrinks (base.py:152-157: `interp = cv2.INTER_LINEAR if (self.augment or
   r > 1) else cv2.INTER_AREA`), uint8 HWC, 3 channels, dh <= sh and dw <= sw (anything else: argument error).  OpenCV's scalar rule
   (computeResizeAreaTab + ResizeArea_Invoker) as tests/resize_area_ref.py states it: per-axis (index, f32 weight) tables built on the host in
   double and uploaded with the call on `stream`, f32 accumulation in table order without FMA, cvRound + saturate. */
int dy_aug_resize_area_u8(const uint8_t* src, int sh, int sw, int64_t src_pitch, uint8_t* dst, int dh, int dw, int64_t dst_pitch, void* stream);
/* LetterBox + Format (augment.py:559-591,745-751): resize to new_h x new_w, border 114 (top / left given), out = uint8 [3, out_h, out_w] RGB. */
int dy_aug_letterbox(const uint8_t* src, int sh, int sw, int64_t src_pitch, int new_h, int new_w, int top, int left, int out_h, int out_w,
                     uint8_t* out, void* stream);
/* Mosaic canvas -> cv2.warpAffine(borderValue 114) -> RandomHSV -> RandomFlip x2 -> Format for B samples in one launch (augment.py:158-195,
 * 323-345,486-499,527-532,745-751); samples: DEVICE array of B descriptors; out = uint8 [B, 3, out_h, out_w] RGB = batch['img']. */
int dy_aug_mosaic_warp(const dy_aug_sample* samples, int B, int out_h, int out_w, uint8_t* out, void* stream);
/* The same with MixUp (augment.py:272-288) for the samples whose `mix` is set: `b` (the partner after ITS Mosaic / RandomPerspective; only
 * the geometry fields src, sh, sw, pitch, rect, n_src, canvas_*, minv are read) is warped at the same pixel and blended per channel as
 * numpy's `(img1 * r + img2 * (1 - r)).astype(np.uint8)` -- float64 products and sum, each rounded once, truncation; r1 = 1.0 - r is
 * computed by the caller in float64.  HSV gains and flips are `a`'s and act on the blend.  A sample with mix == 0 gives the bits of
 * dy_aug_mosaic_warp on `a`. */
typedef struct dy_aug_mix_sample {
  dy_aug_sample a, b;
  double r, r1;
  int32_t mix;
} dy_aug_mix_sample;
int dy_aug_mosaic_warp_mix(const dy_aug_mix_sample* samples, int B, int out_h, int out_w, uint8_t* out, void* stream);
/* The classify task's transform for B samples in one launch: out[b] = Format(RandomHSV(flips(cv2.resize(src[y0:y0+ch, x0:x0+cw], (S, S),
 * INTER_LINEAR)))), uint8 [B, 3, S, S] planar RGB.  With the centre crop (m = min(h, w), top = (h - m) // 2, left = (w - m) // 2), no flips
 * and hsv = 0 this is the reference's classify_transforms = CenterCrop(size) + ToTensor() before its / 255 (data/augment.py:799-806,
 * 879-907), the transform of the classify predictor and of the train / val sets when albumentations is absent; a random crop, flips and
 * the RandomHSV tables (augment.py:493-497) make the training augmentation.  Clamped resize taps clamp to the crop (cv2 sees a view),
 * never to the image around it.  samples: DEVICE array of B descriptors.  The descriptors are read back and checked before the launch
 * (one copy and a wait on `stream`: this entry does wait): a null source, pitch < 3 * sw, or a crop that is empty or not inside its image
 * is an argument error (1), as are B < 0, S <= 0 and a null pointer with B > 0.  B == 0 succeeds and writes nothing. */
typedef struct dy_cls_sample {
  const uint8_t* src;      /* decoded image, uint8 HWC BGR, at its decoded size */
  int64_t pitch;           /* bytes per row */
  int32_t sh, sw;
  int32_t x0, y0, cw, ch;  /* the crop, in pixels of src */
  int32_t fliplr, flipud, hsv, reserved;
  uint8_t lut[3][256];     /* RandomHSV's hue / saturation / value tables, read when hsv != 0 */
} dy_cls_sample;
int dy_cls_render(const dy_cls_sample* samples, int B, int S, uint8_t* out, void* stream);
/* DarkChannel / AtmLight / DarkIcA of preprocess_batch (train.py:42-68,81-96) without the device->host copy and the Python loop:
 * img f32 [B,3,H,W] in [0,1] (the darkened batch) -> A [B,3] (0..255 scale, as train.py:95), ica [B,1,H,W].  Deterministic: ties of the
 * reference's unstable argsort go by pixel index, the rows DarkIcA leaves uninitialised use the per-channel formula. */
int dy_dark_channel_prior(const float* img, int B, int H, int W, float* A, float* ica, void* stream);


/* ---- ground-truth masks of the segment task from polygons (csrc/polymask.hip) -------------------------------------------------------
 * Replaces polygon2mask (ultralytics/data/utils.py:137-155: cv2.fillPoly at the input resolution + cv2.resize by 1 / mask_ratio) for
 * every instance of a batch in one launch.  polys: int16 [n_total][P][2] (x, y) vertices as polygon2mask truncates them
 * (astype(np.int32)), 1 <= P <= 4096; coordinates outside the plane (x == w, y == h included) are legal and never touch memory outside
 * it.  Pixel rule: full-resolution pixel (x, y) is set iff the integer point lies in the CLOSED polygon (even-odd interior or on an
 * edge, closing edge included; integer arithmetic); the mask is cv2.resize(INTER_LINEAR) of that 0/1 plane: ratio 1 = the plane, even
 * ratio = at least 2 of the 4 taps (rows / columns ratio i + ratio / 2 - 1 and + 1).  planes: uint8 [n_total][h / ratio][w / ratio]
 * 0/1 (= polygons2masks, utils.py:158-170, in label order); area: int32 [n_total] set-pixel counts (utils.py:182).  w <= 2048. */
int dy_polymask_raster(const int16_t* polys, int n_total, int P, int h, int w, int ratio, uint8_t* planes, int32_t* area, void* stream);
/* polygons2masks_overlap (utils.py:173-190) + the re-ordering of Format._format_segments (augment.py:757-760) for B images: instances
 * of image b are rows offsets[b] .. offsets[b + 1] (at most 255); they are ranked by area descending, equal areas by original index
 * (the reference's unstable argsort leaves ties open); masks uint8 [B][mh][mw] = 1 + largest rank covering the pixel, else 0;
 * rows_out [n_total][6] = the f32 label rows in rank order, perm int32 [n_total] = index within the image of the instance at each
 * rank (`sorted_idx`). */
int dy_polymask_compose(const uint8_t* planes, const int32_t* area, const int32_t* offsets, int B, int n_total, int mh, int mw,
                        const float* rows_in, float* rows_out, int32_t* perm, uint8_t* masks, void* stream);


/* ---- segment task (csrc/seg.hip) ---------------------------------------------------------------------------------------------------
 * Mask loss of v8SegmentationLoss (U/utils/loss.py:252-288, single_mask_loss; crop_mask U/utils/ops.py:553-569) on the assignment of
 * dy_tal_assign, and the bias of the Proto's ConvTranspose2d(k=2, s=2) (U/nn/modules/block.py:242-254; its weight runs on
 * dy_conv2d_dgrad / dy_conv2d_fwd / dy_conv2d_wgrad as a 2x2 stride-2 conv mapping c2 -> c1).  Fixed-order sums, no float atomics,
 * no host synchronisation. */
typedef struct dy_seg_desc {
  const void* mc; int64_t mc_ld;          /* mask coefficients [B][A][mc_ld] (compute dtype, nm used) */
  const void* proto; int64_t proto_ld;    /* proto map NHWC [B][mh][mw][proto_ld] (compute dtype) */
  int32_t B, A, nm, mh, mw;               /* nm must be 32 */
  const int32_t* target_gt_idx;           /* [B][A] from dy_tal_assign */
  const uint8_t* fg_mask;                 /* [B][A] */
  const float* target_box;                /* [B][A][4] xyxy pixels */
  const void* masks;                      /* overlap: [B][mask_h][mask_w] index map, gt k of image b == k + 1 (batch-label order);
                                           * else [N][mask_h][mask_w] per-instance planes, gt j of image b = j-th row with batch_idx == b */
  int32_t mask_dtype;                     /* 0: uint8, 1: int32 */
  int32_t mask_h, mask_w;                 /* != (mh, mw): sampled as F.interpolate(mode='nearest') (loss.py:254-255) */
  int32_t overlap;
  const int32_t* gt_rows; int32_t n_max;  /* overlap == 0: dy_seg_gt_rows table [B][n_max] */
  float img_h, img_w;                     /* network input size (pixels of target_box) */
  const int32_t* pos; const int32_t* npos;/* dy_seg_positives: pos [B][A] anchor indices in anchor order, npos [B] */
  int32_t dtype;                          /* DY_F32 / DY_BF16 / DY_F16 of mc and proto */
} dy_seg_desc;
/* positives of every image in anchor order: pos[b][0..npos[b]) = anchors a with fg_mask[b][a] != 0 */
int dy_seg_positives(const uint8_t* fg_mask, int B, int A, int32_t* pos, int32_t* npos, void* stream);
/* rows[b][j] = index of the j-th target row with batch_idx == b (-1 past the image's count); batch_idx f32 [n_targets] */
int dy_seg_gt_rows(const float* batch_idx, int n_targets, int B, int n_max, int32_t* rows, void* stream);
/* Mask loss.  lossp: f32 workspace [B*A + B].  det_out = dy_loss_finish's (total, box, cls, dfl) -> out[5] = (total + seg * B, box,
 * seg, cls, dfl) with seg = hyp_box / B * sum_b mean over b's positives of the cropped BCE / (mh*mw) / normalised box area. */
int dy_seg_loss_fwd(const dy_seg_desc* d, float hyp_box, float* lossp, const float* det_out, float* out, void* stream);
/* d total / d mc for every positive anchor (rows [B][A][dmc_ld]; rows of other anchors are not written) and d total / d proto
 * (NHWC [B][mh][mw][dproto_ld], every pixel written), both in the compute dtype; grad_out = d loss / d total (f32, device). */
int dy_seg_loss_bwd(const dy_seg_desc* d, const float* grad_out, float hyp_box, void* dmc, int64_t dmc_ld, void* dproto,
                    int64_t dproto_ld, void* stream);
/* x[p][c] += bias[c] for p < pixels, c < C (NHWC view, pixel stride ld): ConvTranspose2d's bias after the dgrad-route forward */
int dy_bias_add(void* x, int64_t ld, const float* bias, int64_t pixels, int C, int dtype, void* stream);
/* db[c] = sum over pixels of dy[p][c], c < C, in a fixed order.  scratch: DY_BIAS_GRAD_CHUNKS * C floats. */
#define DY_BIAS_GRAD_CHUNKS 2048
int dy_bias_grad(const void* dy, int64_t ld, int64_t pixels, int C, int dtype, float* scratch, int64_t scratch_elems, float* db,
                 void* stream);

/* Validation (process_mask with upsample=False, U/utils/ops.py:593-623): out[j][mh][mw] = sigmoid(c_j . P_b) > 0.5 inside box_j * (sx, sy)
 * (crop_mask's x1 <= col < x2), in f32.  det rows (x1, y1, x2, y2, conf, cls, c_0 .. c_31) at stride det_ld, det_img[j] = image b;
 * proto NHWC [B][mh][mw][proto_ld] in `dtype`. */
int dy_seg_mask_decode(const void* proto, int64_t proto_ld, int nm, int mh, int mw, const float* det, int64_t det_ld,
                       const int32_t* det_img, int n, float sx, float sy, int dtype, uint8_t* out, void* stream);
/* crop_mask (U/utils/ops.py:553-569) in place: masks f32 [n][h][w] zeroed outside box_j = (x1, y1, x2, y2). */
int dy_seg_crop_mask(float* masks, const float* boxes, int n, int h, int w, void* stream);
/* mask_iou (U/utils/metrics.py:131-147) with integer counts: pred uint8 [n][hw]; gt = overlap ? one index map [hw] (uint8 / int32
 * by gt_dtype 0 / 1, label k == k + 1) : uint8 planes [m][hw].  iou f32 [m][n] = inter / ((area_g + area_p) - inter + 1e-7);
 * work: int32 [m*n + n]. */
int dy_seg_mask_iou(const uint8_t* pred, int n, const void* gt, int gt_dtype, int overlap, int m, int64_t hw, int32_t* work,
                    float* iou, void* stream);

/* ---- segment inference at image resolution (csrc/segmask.hip) -------------------------------------------------------------------------
 * Fused process_mask(upsample=True) / process_mask_upsample / process_mask_native (U/utils/ops.py:593-623, 572-590, 625-642 with
 * scale_masks :645-666 and crop_mask :553-569): per detection j of image b
 *   s = sigmoid(c_j . P_b) at the proto resolution in f32; crop_before: s = 0 outside box_j * (sx, sy) (x1 <= col < x2);
 *   window rows [top, bottom), columns [left, right) of the proto plane (scale_masks' padding crop; the whole plane = 0, 0, mh, mw);
 *   bilinear resize of the window to (oh, ow) as F.interpolate(mode='bilinear', align_corners=False) does it: scale = in / out in f32,
 *   src = scale * (dst + 0.5) - 0.5 clamped at 0, upper tap clamped to the window, wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d);
 *   crop_after: 0 outside box_j as given (output pixels); out[j][oh][ow] = value > 0.5.
 * No f32 plane reaches memory.  det rows (x1, y1, x2, y2, conf, cls, c_0 .. c_31) at stride det_ld, grouped by image: the rows of group g
 * are img_off[g] .. img_off[g + 1] - 1 and belong to proto image img_ids[g] (n_groups groups, img_off [n_groups + 1]).  det_chunk > 0:
 * detections one workgroup walks with its proto tile resident (the groups are split into ceil(max_group / det_chunk) chunks, max_group =
 * the largest group).  proto NHWC [B][mh][mw][proto_ld] in `dtype`.  The resize may scale down by at most about 10 in either axis. */
int dy_seg_mask_upsample(const void* proto, int64_t proto_ld, int nm, int mh, int mw, int dtype, const float* det, int64_t det_ld,
                         const int32_t* img_off, const int32_t* img_ids, int n_groups, int max_group, int det_chunk, int crop_before,
                         float sx, float sy, int top, int left, int bottom, int right, int oh, int ow, int crop_after, uint8_t* out,
                         void* stream);
/* Bilinear resize (align_corners=False, the arithmetic above) of m mask planes: the gt side of SegmentationValidator._process_batch
 * (U/models/yolo/segment/val.py:140-148: torch.where(gt == k + 1, 1.0, 0.0), F.interpolate(..., mode='bilinear'), gt_(0.5)) and the body
 * of scale_masks (U/utils/ops.py:645-666).  src_kind 0: uint8 planes [m][h][w]; 1 / 2: one uint8 / int32 index map [h][w], plane k = (map
 * == k + 1); 3: f32 planes [m][h][w].  Source window rows [top, bottom), columns [left, right).  out_f32 == 0: uint8 [m][oh][ow] of value
 * > 0.5 (strict), else the f32 value. */
int dy_mask_resize(const void* src, int src_kind, int m, int h, int w, int top, int left, int bottom, int right, void* out, int out_f32,
                   int oh, int ow, void* stream);

/* ---- pose task (csrc/pose.hip) ------------------------------------------------------------------------------------------------------
 * Keypoint terms of v8PoseLoss / KeypointLoss (U/utils/loss.py:87-99, 292-377) on the assignment of dy_tal_assign, Pose.kpts_decode
 * (U/nn/modules/head.py:221-241) and kpt_iou (U/utils/metrics.py:150-169).  Fixed-order sums, no float atomics, no host
 * synchronisation.  The keypoint maps are the per-level outputs of Pose.cv4[l][2], read in place: NHWC [B][h_l][w_l][kpt_ld_l] in the
 * compute dtype, channel k * ndim + j = coordinate j (x, y, visibility logit) of keypoint k; anchors are numbered level by level as in
 * dy_det_maps / dy_det_maps4. */
#define DY_POSE_MAX_LEVELS 4
typedef struct dy_pose_desc {
  const void* kpt[DY_POSE_MAX_LEVELS];    /* level maps (n_levels used) */
  int64_t kpt_ld[DY_POSE_MAX_LEVELS];     /* pixel stride of each map, >= K * ndim */
  int32_t h[DY_POSE_MAX_LEVELS], w[DY_POSE_MAX_LEVELS];
  float stride[DY_POSE_MAX_LEVELS];
  int32_t n_levels, B, A, K, ndim, dtype; /* A = sum of h_l * w_l; ndim 2 or 3; DY_F32 / DY_BF16 / DY_F16 */
  /* loss only (dy_pose_kpt_decode reads none of these): */
  const int32_t* target_gt_idx;           /* [B][A] from dy_tal_assign */
  const uint8_t* fg_mask;                 /* [B][A] */
  const float* target_box;                /* [B][A][4] xyxy pixels */
  const float* keypoints;                 /* [n_targets][K][3] f32: normalised x, y and visibility (3 columns for ndim 2 as well) */
  int32_t n_targets;
  const int32_t* gt_rows; int32_t n_max;  /* dy_seg_gt_rows table [B][n_max]: gt g of image b = keypoints row gt_rows[b][g] */
  float img_h, img_w;                     /* network input size */
  const float* sigma;                     /* [K] f32: OKS_SIGMA for kpt_shape [17, 3], else 1 / K */
  const int32_t* pos; const int32_t* npos;/* dy_seg_positives of fg_mask */
} dy_pose_desc;
/* Keypoint loss.  work: f32 [3*B*A + 3*B] (per-positive sums, then per image pose_b, kobj_b, visible count; dy_pose_loss_bwd reads it).
 * det_out = dy_loss_finish's (total, box, cls, dfl) -> out[6] = (total + (pose + kobj) * B, box, pose, kobj, cls, dfl) with
 * pose = hyp_pose / B * sum_b (n_b K) / (nnz_b + 1e-9) * mean((1 - exp(-e)) * vis), kobj = hyp_kobj / B * sum_b mean BCE(logit, vis)
 * (0 for ndim 2), n_b = positives of image b; images without positives add 0. */
int dy_pose_loss_fwd(const dy_pose_desc* d, float hyp_pose, float hyp_kobj, float* work, const float* det_out, float* out, void* stream);
/* d total / d keypoint maps, scaled by *grad_out (f32, device): dkpt[l] = NHWC [B][h_l][w_l][dk_ld] in the compute dtype, every element
 * written (non-positive anchors, channels >= K * ndim and pad lanes get 0); dk_ld >= K * ndim rounded up to the vector width. */
int dy_pose_loss_bwd(const dy_pose_desc* d, const float* work, const float* grad_out, float hyp_pose, float hyp_kobj,
                     void* const* dkpt, int64_t dk_ld, void* stream);
/* Eval decode into rows [4+nc, 4+nc+K*ndim) of y [B][4+nc+K*ndim][A] f32 (dy_detect_decode fills rows [0, 4+nc)):
 * x = (raw * 2 + (anchor_x - 0.5)) * stride, likewise y, sigmoid(raw) for the visibility of ndim 3. */
int dy_pose_kpt_decode(const dy_pose_desc* d, int nc, float* y, void* stream);
/* OKS (kpt_iou): gt f32 [N][K][3], pred f32 [M][K][pred_dim], area f32 [N], sigma f32 [K] -> out f32 [N][M] =
 * sum_k exp(-e) [vis != 0] / (sum_k [vis != 0] + eps), e = d / (2 sigma)^2 / (area + eps) / 2. */
int dy_kpt_oks(const float* gt, int N, const float* pred, int M, int pred_dim, const float* area, const float* sigma, int K, float eps,
               float* out, void* stream);

/* ---- classify task (csrc/classify.hip) ----------------------------------------------------------------------------------------------
 * The device side of Classify (U/nn/modules/head.py:244-260), v8ClassificationLoss (U/utils/loss.py:380-385) and the top-k accuracy of
 * ClassificationValidator / ClassifyMetrics (U/models/yolo/classify/val.py:39-60, U/utils/metrics.py:197-207, 1018-1061).  dtype =
 * DY_F32 / DY_BF16 / DY_F16; every operand is addressed through its leading dimension (elements); rows are read with 16-byte loads where
 * base and leading dimension are 16-byte aligned.  No float atomics: every sum runs in a fixed order. */
/* AdaptiveAvgPool2d(1) (head.py:250): x NHWC [N][HW][x_ld] -> y [N][y_ld], channels [0, C); f32 accumulation, one rounding.  N <= 65535. */
int dy_gap_fwd(const void* x, int64_t x_ld, int N, int HW, int C, int dtype, void* y, int64_t y_ld, void* stream);
/* its adjoint: dx[n][p][c] = dy[n][c] / HW for c < C, overwritten (channels >= C of a pixel are not touched). */
int dy_gap_bwd(const void* dy, int64_t dy_ld, int N, int HW, int C, int dtype, void* dx, int64_t dx_ld, void* stream);
/* cross_entropy(logits, cls, reduction='sum') / 64 (loss.py:383-385): row_lse f32 [B] = log sum_j exp(z[b][j]) (one read of each logit),
 * loss f32 [1] = sum_b (row_lse[b] - z[b][cls[b]]) / 64.  A label outside [0, nc) (torch's ignore_index -100 among them) adds 0 and
 * indexes nothing. */
int dy_cls_xent_fwd(const void* logits, int64_t ld, int dtype, const int64_t* cls, int B, int nc, float* row_lse, float* loss, void* stream);
/* dlogits[b][j] = (exp(z - row_lse[b]) - [j == cls[b]]) * *grad_out / 64 in the logits' dtype, rows [B][dld]; rows with a label outside
 * [0, nc) and columns nc <= j < dld are written as 0.  grad_out: f32 device scalar. */
int dy_cls_xent_bwd(const void* logits, int64_t ld, int dtype, const int64_t* cls, const float* row_lse, const float* grad_out, int B,
                    int nc, void* dlogits, int64_t dld, void* stream);
/* softmax(1) of the eval head (head.py:259): probs f32 [B][nc], compact. */
int dy_cls_softmax(const void* logits, int64_t ld, int dtype, int B, int nc, float* probs, void* stream);
/* argsort(1, descending=True)[:, :k] (val.py:57): idx int32 [B][k], 1 <= k <= min(nc, 8).  Equal values rank by ascending index (the
 * order of a stable descending sort; -0 equals +0); NaN ranks below every number. */
int dy_cls_topk(const void* scores, int64_t ld, int dtype, int B, int nc, int k, int32_t* idx, void* stream);
/* ClassifyMetrics.process / ConfusionMatrix.process_cls_preds (metrics.py:1043-1048, 197-207) for one batch: counts int64 [3] += (rows,
 * rows with idx[b][0] == cls[b], rows with any idx[b][:] == cls[b]); confusion int32 [nc][nc] (or null): [idx[b][0]][cls[b]] += 1.
 * Integer atomics.  A row whose label is outside [0, nc) is not counted. */
int dy_cls_metrics_update(const int32_t* idx, int k, const int64_t* cls, int B, int nc, int64_t* counts, int32_t* confusion, void* stream);

/* ------------------------------------------------------------------------------------------------ validation matching
 * The per-image bookkeeping of DetectionValidator.update_metrics (U/models/yolo/detect/val.py:72-116) for a whole batch: one
 * workgroup per image, nothing read back.
 *  dy_val_box_match: replaces scale_boxes on predictions and labels (U/utils/ops.py:95-125), box_iou (U/utils/metrics.py:52-72),
 *                    `_process_batch` (val.py:151-174) and ConfusionMatrix.process_batch (metrics.py:209-253).
 *    det [B, max_det, ld] f32 rows (x1,y1,x2,y2,conf,cls,...) and ocnt [B] as dy_nms_greedy leaves them (ld >= 6);
 *    lcls [L] f32, lxywh [L, 4] f32 normalised, loff [B + 1] int32: the batch's labels sorted by image; (H, W) the network input;
 *    rec [B, 5] f32 = (gain, pad_x, pad_y, h0, w0) per image, filled as scale_boxes computes them; iouv [T] f32, T <= 16.
 *    -> correct u8 [B, max_det, T] (rows >= ocnt[b] zero), predn f32 [B, max_det, 4] and tboxn f32 [L, 4] native-space boxes,
 *       confusion int32 [nc + 1, nc + 1] [predicted][true] accumulated with integer atomics (NULL: not filled; detections with
 *       conf > conf_thres, pairs with IoU > iou_thres, both strict; background = nc).  All arithmetic f32 in the host order.
 *    `correct` is the rule of engine/validator.match_from_iou: at threshold k the candidates are the equal-class pairs with
 *    IoU >= iouv[k]; a detection keeps the label it overlaps most (tie: higher label index), a label the lowest-index detection.
 *    single_cls: every detection class reads as 0.
 *  dy_val_iou_match: the same rule on precomputed IoU matrices (mask IoU, U/models/yolo/segment/val.py:131-166; OKS,
 *                    U/models/yolo/pose/val.py:110-141): iou = the [M_b, N_b] f32 matrices of the batch one after another
 *                    (row-major, M_b = loff[b+1] - loff[b], N_b = ocnt[b]), moff [B] int64 their element offsets.
 *  workspace: B * max_det * 5 int32 when max_det * 20 bytes exceed 40 KiB (the per-detection state then does not fit in LDS),
 *             else it may be NULL.  Labels per image are not limited.  Label offsets outside [0, L] and a matrix that does not lie
 *             inside the iou_numel elements of `iou` read as an image without labels. */
int dy_val_box_match(const float* det, int ld, const int* ocnt, int B, int max_det, const float* lcls, const float* lxywh,
                     const int* loff, int L, int H, int W, const float* rec, const float* iouv, int T, int single_cls, float conf_thres,
                     float iou_thres, int nc, uint8_t* correct, float* predn, float* tboxn, int32_t* confusion, void* workspace,
                     void* stream);
int dy_val_iou_match(const float* iou, int64_t iou_numel, const int64_t* moff, const float* det, int ld, const int* ocnt, int B,
                     int max_det, const float* lcls, const int* loff, int L, const float* iouv, int T, int single_cls, uint8_t* correct,
                     void* workspace, void* stream);

/* ---- channel and spatial attention (csrc/cbam.hip) --------------------------------------------------------------------------------
 * The device side of ChannelAttention (U/nn/modules/conv.py:294-304), SpatialAttention (conv.py:307-320) and CBAM (conv.py:449-459):
 *   g = sigmoid(a[b]), u = x g, m = (mean_c u, max_c u), s = sigmoid(cv1(m)), y = u s
 * a [B][a_ld]: the fc's logits in the compute dtype (the pool is dy_chan_pool_fwd, the fc a 1x1 convolution); a == NULL: no channel gate
 * (SpatialAttention alone).  x / y / dy / dx: NHWC views [B][HW][ld] of which exactly the channels [0, C) are touched, 16-byte
 * accesses when every map view of a call is 16-byte aligned in pointer and pitch, element accesses otherwise.  C % 8 == 0,
 * 8 <= C <= DY_CBAM_MAX_C, B <= 65535, B HW < 2^31, k = 3 or 7; all arithmetic f32.  The planes (mean, mx, s, dpre, dmean, dmx: f32
 * [B][HW]; arg: int32 [B][HW]) are dense.  w: cv1.weight f32 [1][2][k][k] (plane 0 = mean, 1 = max), zero padding k / 2.
 * Every backward entry gives identical bytes on every run (fixed partial ranges, fixed-order second pass, no atomics). */
#define DY_CBAM_MAX_C 2048
#define DY_CBAM_MAX_PARTS 64   /* most workgroups (= partial sums per channel) along the pixels of one image in the reduce */
#define DY_CBAM_GATE_TILE 8    /* dy_spatial_gate_fwd: pixels per workgroup and direction */
#define DY_CBAM_CONV_TILE 16   /* dy_spatial_conv_bwd: likewise */
/* AdaptiveAvgPool2d(1) of ChannelAttention (conv.py:299, 304) for maps of many pixels: y[b][c] = mean_p x[b][p][c] in the compute
 * dtype, f32 partial sums of at most DY_CBAM_MAX_PARTS workgroups per image added in index order in f64 (deterministic); dy_gap_fwd
 * walks an image in one thread per channel group and is left as it is.  workspace: dy_cbam_reduce_workspace floats. */
int dy_chan_pool_fwd(const void* x, int64_t x_ld, void* y, int64_t y_ld, float* workspace, int64_t workspace_elems, int B, int HW, int C,
                     int dtype, void* stream);
/* ChannelAttention.forward (conv.py:302-304): y = x sigmoid(a[b]) */
int dy_chan_gate_fwd(const void* x, int64_t x_ld, const void* a, int64_t a_ld, void* y, int64_t y_ld, int B, int HW, int C, int dtype,
                     void* stream);
/* torch.mean(x, 1) / torch.max(x, 1) (conv.py:320) of u = x g in one read, u not stored: mean, mx; arg (NULL: not wanted) = the
 * lowest channel index that reaches the maximum (torch.max's gradient rule on the CPU).  The running maximum starts from -inf. */
int dy_spatial_stats_fwd(const void* x, int64_t x_ld, const void* a, int64_t a_ld, float* mean, float* mx, int32_t* arg, int B, int HW,
                         int C, int dtype, void* stream);
/* cat + cv1 + sigmoid + the two scales (conv.py:320, 458): s = sigmoid(conv_kxk(mean, mx)) from a halo tile of the planes in LDS,
 * y = x g s; s (NULL: not kept) is stored for the backward. */
int dy_spatial_gate_fwd(const void* x, int64_t x_ld, const void* a, int64_t a_ld, const float* mean, const float* mx, const float* w,
                        int k, void* y, int64_t y_ld, float* s, int B, int H, int W, int C, int dtype, void* stream);
/* autograd of `u * s` towards s and of the sigmoid: dpre = s (1 - s) sum_c dy x g */
int dy_spatial_gate_bwd_px(const void* dy, int64_t dy_ld, const void* x, int64_t x_ld, const void* a, int64_t a_ld, const float* s,
                           float* dpre, int B, int HW, int C, int dtype, void* stream);
/* autograd of cv1 on the planes: (dmean, dmx) = the transposed convolution of dpre (flipped taps, zero padding) and
 * dw f32 [2][k][k] = sum_{b, p} dpre[p] m[p + tap].  workspace: dy_spatial_conv_bwd_workspace floats. */
int64_t dy_spatial_conv_bwd_workspace(int B, int H, int W, int k);
int dy_spatial_conv_bwd(const float* dpre, const float* mean, const float* mx, const float* w, int k, float* dmean, float* dmx, float* dw,
                        float* workspace, int64_t workspace_elems, int B, int H, int W, void* stream);
/* autograd of mean / max / `x * g`, split around the fc's backward so that dx is written once:
 *   du = dy s + dmean / C + (c == arg ? dmx : 0)                       (s == NULL: no spatial stage, du = dy: ChannelAttention alone)
 *   reduce: da[b][c] = g (1 - g) sum_p du x, rounded once to the compute dtype; workspace: dy_cbam_reduce_workspace floats
 *   apply:  dx = du g + dpool[b][c] / HW (+ dx when accumulate); dpool [B][dpool_ld] = the fc's data gradient (NULL: none) */
int64_t dy_cbam_reduce_workspace(int B, int HW, int C, int dtype);
int dy_spatial_gate_bwd_reduce(const void* dy, int64_t dy_ld, const void* x, int64_t x_ld, const void* a, int64_t a_ld, const float* s,
                               const float* dmean, const float* dmx, const int32_t* arg, void* da, int64_t da_ld, float* workspace,
                               int64_t workspace_elems, int B, int HW, int C, int dtype, void* stream);
int dy_spatial_gate_bwd_apply(const void* dy, int64_t dy_ld, const void* a, int64_t a_ld, const float* s, const float* dmean,
                              const float* dmx, const int32_t* arg, const void* dpool, int64_t dpool_ld, void* dx, int64_t dx_ld,
                              int accumulate, int B, int HW, int C, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif
