// Pose task: keypoint loss, keypoint decode and OKS.
// Replaces v8PoseLoss's keypoint terms and KeypointLoss (reference ultralytics/utils/loss.py:87-99, 292-377), Pose.kpts_decode
// (ultralytics/nn/modules/head.py:221-241) and kpt_iou (ultralytics/utils/metrics.py:150-169).
//
// The keypoint maps are the per-level outputs of Pose.cv4[i][2], read in place: NHWC [B][h_l][w_l][kpt_ld_l], channel
// k * ndim + j = coordinate j of keypoint k, anchors numbered level by level.  For positive (b, a) with gt row r (the
// target_gt_idx[b][a]-th label of image b) and stride s of the anchor's level:
//   px = raw_x * 2 + (ax - 0.5),  gx = kx * img_w / s      (likewise y)         grid units
//   e  = ((px - gx)^2 + (py - gy)^2) / (2 sigma_k)^2 / (area + 1e-9) / 2       area: w * h of target_box / s
//   pose_b = (n_b K) / (nnz_b + 1e-9) * mean over b's n_b K keypoints of (1 - exp(-e)) * [vis != 0]
//   kobj_b = mean over the same n_b K keypoints of BCEWithLogits(raw_v, [vis != 0])            (ndim 3 only)
//   pose = hyp_pose / B * sum_b pose_b,  kobj = hyp_kobj / B * sum_b kobj_b
// Sums run in a fixed order: one thread sums the K keypoints of a positive, one block per image sums its positives in a
// strided-then-tree order, one thread sums the images.  No float atomics (two runs agree bit for bit) and no host
// synchronisation: the positive counts stay on the device.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

constexpr int NT = 256;

struct Pose {
  const char* kpt[DY_POSE_MAX_LEVELS];
  long ld[DY_POSE_MAX_LEVELS];
  int h[DY_POSE_MAX_LEVELS], w[DY_POSE_MAX_LEVELS], off[DY_POSE_MAX_LEVELS + 1];
  float stride[DY_POSE_MAX_LEVELS];
  int nl, B, A, K, ndim;
  const int32_t* tgi; const uint8_t* fg; const float* tbox;
  const float* kp; const int32_t* gt_rows; int n_max;
  float img_h, img_w;
  const float* sigma;
  const int32_t* pos; const int32_t* npos;
};

struct DyPoseGrad { void* p[DY_POSE_MAX_LEVELS]; };

__device__ inline int level_of(const Pose& p, int a) {
  int l = 0;
#pragma unroll
  for (int i = 1; i < DY_POSE_MAX_LEVELS; ++i) l += (a >= p.off[i]);
  return l;
}

template <typename T>
__device__ inline const T* kpt_row(const Pose& p, int b, int lvl, int cell) {
  return reinterpret_cast<const T*>(p.kpt[lvl]) + ((long)b * p.h[lvl] * p.w[lvl] + cell) * p.ld[lvl];
}

__device__ inline float sigmoidf_(float z) { return 1.f / (1.f + expf(-z)); }

// BCEWithLogits(z, t) = (1 - t) z + softplus(-z), softplus(-z) = max(-z, 0) + log1p(exp(-|z|))
__device__ inline float bce_logits(float z, float t) { return (1.f - t) * z + fmaxf(-z, 0.f) + log1pf(expf(-fabsf(z))); }

// one keypoint of positive (b, a): the predicted xy decode and the gt in grid units, the OKS exponent and its visibility
struct Kp { float dx, dy, e, c, area, vis; };

template <typename T>
__device__ inline Kp keypoint(const Pose& p, const T* r, int lvl, int cell, const float* g, float area, int k) {
  const float s = p.stride[lvl];
  const int yy = cell / p.w[lvl], xx = cell - yy * p.w[lvl];
  const float ax = (float)xx + 0.5f, ay = (float)yy + 0.5f;
  const float px = DT<T>::ld(r + k * p.ndim) * 2.f + (ax - 0.5f);
  const float py = DT<T>::ld(r + k * p.ndim + 1) * 2.f + (ay - 0.5f);
  Kp q;
  q.vis = g ? (g[3 * k + 2] != 0.f ? 1.f : 0.f) : 0.f;
  const float gx = g ? g[3 * k] * p.img_w / s : 0.f, gy = g ? g[3 * k + 1] * p.img_h / s : 0.f;
  q.dx = px - gx;
  q.dy = py - gy;
  const float d = q.dx * q.dx + q.dy * q.dy;
  const float two_s = 2.f * p.sigma[k];
  q.c = two_s * two_s;                                   // (2 sigma)^2
  q.area = area;
  q.e = d / q.c / (area + 1e-9f) / 2.f;
  return q;
}

// gt keypoints [K][3] of positive (b, a), or null when the image has no such row
__device__ inline const float* gt_kpts(const Pose& p, int b, int a) {
  const int g = p.tgi[(long)b * p.A + a];
  const int row = (g >= 0 && g < p.n_max) ? p.gt_rows[(long)b * p.n_max + g] : -1;
  return row >= 0 ? p.kp + (long)row * p.K * 3 : nullptr;
}

// area of the target box after its division by the stride (xyxy2xywh(target_bboxes / s)[:, 2:].prod)
__device__ inline float box_area(const Pose& p, int b, int a, float s) {
  const float* t = p.tbox + ((long)b * p.A + a) * 4;
  return (t[2] / s - t[0] / s) * (t[3] / s - t[1] / s);
}

// ---- forward 1: per positive, the sums over its K keypoints in keypoint order --------------------------------------------------
// work[0][b][slot] = sum (1 - exp(-e)) * vis, work[1][b][slot] = sum vis, work[2][b][slot] = sum BCE (ndim 3)
template <typename T>
__global__ __launch_bounds__(NT) void pose_pos_kernel(Pose p, float* __restrict__ work) {
  const int b = blockIdx.y;
  const int slot = blockIdx.x * NT + threadIdx.x;
  if (slot >= p.npos[b]) return;
  const int a = p.pos[(long)b * p.A + slot];
  const int lvl = level_of(p, a), cell = a - p.off[lvl];
  const T* r = kpt_row<T>(p, b, lvl, cell);
  const float* g = gt_kpts(p, b, a);
  const float area = box_area(p, b, a, p.stride[lvl]);
  float l = 0.f, nnz = 0.f, bce = 0.f;
  for (int k = 0; k < p.K; ++k) {
    const Kp q = keypoint<T>(p, r, lvl, cell, g, area, k);
    l += (1.f - expf(-q.e)) * q.vis;
    nnz += q.vis;
    if (p.ndim == 3) bce += bce_logits(DT<T>::ld(r + k * 3 + 2), q.vis);
  }
  const long n = (long)p.B * p.A, o = (long)b * p.A + slot;
  work[o] = l;
  work[n + o] = nnz;
  work[2 * n + o] = bce;
}

// fixed-order block sum of three floats per thread (NT threads); thread 0 gets the results
__device__ inline void block_sum3(float& a, float& b, float& c, float (*red)[NT]) {
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[0][threadIdx.x] += red[0][threadIdx.x + s];
      red[1][threadIdx.x] += red[1][threadIdx.x + s];
      red[2][threadIdx.x] += red[2][threadIdx.x + s];
    }
    __syncthreads();
  }
  a = red[0][0]; b = red[1][0]; c = red[2][0];
}

// ---- forward 2: per image.  img[0][b] = pose_b, img[1][b] = kobj_b, img[2][b] = nnz_b ---------------------------------------------
__global__ __launch_bounds__(NT) void pose_image_kernel(Pose p, const float* __restrict__ work, float* __restrict__ img) {
  __shared__ float red[3][NT];
  const int b = blockIdx.x, n = p.npos[b];
  const long N = (long)p.B * p.A;
  float l = 0.f, nnz = 0.f, bce = 0.f;
  for (int j = threadIdx.x; j < n; j += NT) {
    const long o = (long)b * p.A + j;
    l += work[o]; nnz += work[N + o]; bce += work[2 * N + o];
  }
  block_sum3(l, nnz, bce, red);
  if (threadIdx.x == 0) {
    const float nk = (float)n * (float)p.K;
    img[b] = n > 0 ? nk / (nnz + 1e-9f) * (l / nk) : 0.f;                 // kpt_loss_factor * mean
    img[p.B + b] = (n > 0 && p.ndim == 3) ? bce / nk : 0.f;
    img[2 * p.B + b] = nnz;
  }
}

// ---- forward 3: images in order; det = dy_loss_finish's (total, box, cls, dfl) -> out = (total, box, pose, kobj, cls, dfl) -------
__global__ void pose_finish_kernel(const float* __restrict__ img, int B, float hyp_pose, float hyp_kobj, const float* __restrict__ det,
                                   float* __restrict__ out) {
  if (threadIdx.x || blockIdx.x) return;
  float sp = 0.f, sk = 0.f;
  for (int b = 0; b < B; ++b) { sp += img[b]; sk += img[B + b]; }
  const float pose = sp * (hyp_pose / (float)B), kobj = sk * (hyp_kobj / (float)B);
  out[0] = det[0] + (pose + kobj) * (float)B;
  out[1] = det[1]; out[2] = pose; out[3] = kobj; out[4] = det[2]; out[5] = det[3];
}

// ---- backward: every element of every level's gradient map [B][h][w][dk_ld], one thread each --------------------------------------
// total = (sum of the items) * B, so the 1 / B of the pose / kobj gains cancels:
// d total / d raw_x = g * hyp_pose * vis * exp(-e) / (nnz_b + 1e-9) * 2 dx * 2 / (2 sigma)^2 / (area + 1e-9) / 2
// d total / d raw_v = g * hyp_kobj * (sigmoid(raw_v) - vis) / (n_b K)
// non-positive anchors, channels past K * ndim and pad lanes get 0
template <typename T>
__global__ __launch_bounds__(NT) void pose_bwd_kernel(Pose p, const float* __restrict__ img, const float* __restrict__ grad_out,
                                                      float hyp_pose, float hyp_kobj, DyPoseGrad dk, long dk_ld) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  const long per_b = (long)p.A * dk_ld;
  if (i >= (long)p.B * per_b) return;
  const int b = (int)(i / per_b);
  const long rem = i - (long)b * per_b;
  const int a = (int)(rem / dk_ld), c = (int)(rem - (long)a * dk_ld);
  const int lvl = level_of(p, a), cell = a - p.off[lvl];
  float v = 0.f;
  const int nk = p.K * p.ndim;
  if (c < nk && p.fg[(long)b * p.A + a]) {
    const int k = c / p.ndim, j = c - k * p.ndim;
    const T* r = kpt_row<T>(p, b, lvl, cell);
    const float* g = gt_kpts(p, b, a);
    const float gr = grad_out[0];
    if (j == 2) {
      const float vis = g ? (g[3 * k + 2] != 0.f ? 1.f : 0.f) : 0.f;
      const float nkb = (float)p.npos[b] * (float)p.K;
      v = gr * hyp_kobj * (sigmoidf_(DT<T>::ld(r + c)) - vis) / nkb;
    } else {
      const Kp q = keypoint<T>(p, r, lvl, cell, g, box_area(p, b, a, p.stride[lvl]), k);
      const float w = gr * hyp_pose * q.vis * expf(-q.e) / (img[2 * p.B + b] + 1e-9f);
      v = w * (2.f * (j == 0 ? q.dx : q.dy)) * 2.f / q.c / (q.area + 1e-9f) / 2.f;
    }
  }
  T* o = reinterpret_cast<T*>(dk.p[lvl]) + ((long)b * p.h[lvl] * p.w[lvl] + cell) * dk_ld + c;
  DT<T>::st(o, v);
}


// ---- eval decode: rows [4+nc, 4+nc+nk) of y [B][4+nc+nk][A] f32 (the rows before are dy_detect_decode's) ---------------------------
template <typename T>
__global__ __launch_bounds__(NT) void pose_decode_kernel(Pose p, int nc, float* __restrict__ y) {
  const int a = blockIdx.x * NT + threadIdx.x;
  if (a >= p.A) return;
  const int c = blockIdx.y, b = blockIdx.z;
  const int lvl = level_of(p, a), cell = a - p.off[lvl];
  const float raw = DT<T>::ld(kpt_row<T>(p, b, lvl, cell) + c);
  const int j = c % p.ndim;
  float v;
  if (j == 2) v = sigmoidf_(raw);
  else {
    const int yy = cell / p.w[lvl], xx = cell - yy * p.w[lvl];
    const float anc = j == 0 ? (float)xx + 0.5f : (float)yy + 0.5f;
    v = (raw * 2.f + (anc - 0.5f)) * p.stride[lvl];
  }
  y[((long)b * (4 + nc + p.K * p.ndim) + 4 + nc + c) * p.A + a] = v;
}

// ---- OKS [N][M] (kpt_iou): gt [N][K][3], pred [M][K][pred_dim], area [N], sigma [K]; the reference's arithmetic order ----------------
__global__ __launch_bounds__(NT) void kpt_oks_kernel(const float* __restrict__ gt, int N, const float* __restrict__ pred, int M,
                                                     int pred_dim, const float* __restrict__ area, const float* __restrict__ sigma,
                                                     int K, float eps, float* __restrict__ out) {
  const long i = blockIdx.x * (long)NT + threadIdx.x;
  if (i >= (long)N * M) return;
  const int n = (int)(i / M), m = (int)(i - (long)n * M);
  const float* g = gt + (long)n * K * 3;
  const float* q = pred + (long)m * K * pred_dim;
  const float ar = area[n] + eps;
  float num = 0.f, cnt = 0.f;
  for (int k = 0; k < K; ++k) {
    const float dx = g[3 * k] - q[pred_dim * k], dy = g[3 * k + 1] - q[pred_dim * k + 1];
    const float d = dx * dx + dy * dy;
    const float two_s = 2.f * sigma[k];
    const float e = d / (two_s * two_s) / ar / 2.f;
    const float vis = g[3 * k + 2] != 0.f ? 1.f : 0.f;
    num += expf(-e) * vis;
    cnt += vis;
  }
  out[i] = num / (cnt + eps);
}

// d points at the caller's descriptor; which fields are needed depends on the entry (decode: maps only)
int make_pose(const dy_pose_desc* d, Pose& p, bool loss, const char* who) {
  DY_CHECK(d && d->n_levels >= 1 && d->n_levels <= DY_POSE_MAX_LEVELS, "%s: bad descriptor / level count", who);
  if (int e = dy_check_dtype(who, d->dtype)) return e;
  DY_CHECK(d->B > 0 && d->K > 0 && (d->ndim == 2 || d->ndim == 3), "%s: bad B / K / ndim (%d, %d, %d)", who, d->B, d->K, d->ndim);
  p.nl = d->n_levels; p.B = d->B; p.K = d->K; p.ndim = d->ndim;
  int off = 0;
  for (int l = 0; l < DY_POSE_MAX_LEVELS; ++l) {
    p.off[l] = off;
    if (l < d->n_levels) {
      DY_CHECK(d->kpt[l] && d->h[l] > 0 && d->w[l] > 0 && d->kpt_ld[l] >= (long)d->K * d->ndim && d->stride[l] > 0.f,
               "%s: bad level %d", who, l);
      p.kpt[l] = (const char*)d->kpt[l]; p.ld[l] = d->kpt_ld[l]; p.h[l] = d->h[l]; p.w[l] = d->w[l]; p.stride[l] = d->stride[l];
      off += d->h[l] * d->w[l];
    } else {
      p.kpt[l] = nullptr; p.ld[l] = 0; p.h[l] = 1; p.w[l] = 1; p.stride[l] = 1.f;
    }
  }
  p.off[DY_POSE_MAX_LEVELS] = off;
  for (int l = d->n_levels; l <= DY_POSE_MAX_LEVELS; ++l) p.off[l] = off;
  DY_CHECK(d->A == off, "%s: A=%d but the levels hold %d anchors", who, d->A, off);
  p.A = off;
  p.tgi = d->target_gt_idx; p.fg = d->fg_mask; p.tbox = d->target_box;
  p.kp = d->keypoints; p.gt_rows = d->gt_rows; p.n_max = d->n_max;
  p.img_h = d->img_h; p.img_w = d->img_w; p.sigma = d->sigma;
  p.pos = d->pos; p.npos = d->npos;
  if (loss) {
    DY_CHECK(d->target_gt_idx && d->fg_mask && d->target_box && d->gt_rows && d->n_max > 0 && d->sigma && d->pos && d->npos,
             "%s: null pointer", who);
    DY_CHECK(d->keypoints || d->n_targets == 0, "%s: null keypoints", who);
    DY_CHECK(d->img_h > 0.f && d->img_w > 0.f, "%s: bad image size", who);
  }
  return 0;
}

template <typename T>
void launch_pos(const Pose& p, float* work, hipStream_t st) {
  dim3 grid(dy_cdiv(p.A, NT), p.B);
  pose_pos_kernel<T><<<grid, NT, 0, st>>>(p, work);
}

}  // namespace

extern "C" int dy_pose_loss_fwd(const dy_pose_desc* d, float hyp_pose, float hyp_kobj, float* work, const float* det_out, float* out,
                                void* stream) {
  Pose p;
  if (int e = make_pose(d, p, true, "dy_pose_loss_fwd")) return e;
  DY_CHECK(work && det_out && out, "dy_pose_loss_fwd: null output");
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("pose_pos_kernel");
  DY_DISPATCH_DTYPE("dy_pose_loss_fwd", d->dtype, launch_pos<T>(p, work, st));
  DY_LAUNCH_CHECK();
  float* img = work + 3L * p.B * p.A;
  dy_note_kernel("pose_image_kernel");
  pose_image_kernel<<<p.B, NT, 0, st>>>(p, work, img);
  DY_LAUNCH_CHECK();
  dy_note_kernel("pose_finish_kernel");
  pose_finish_kernel<<<1, 64, 0, st>>>(img, p.B, hyp_pose, hyp_kobj, det_out, out);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_pose_loss_bwd(const dy_pose_desc* d, const float* work, const float* grad_out, float hyp_pose, float hyp_kobj,
                                void* const* dkpt, int64_t dk_ld, void* stream) {
  Pose p;
  if (int e = make_pose(d, p, true, "dy_pose_loss_bwd")) return e;
  DY_CHECK(work && grad_out && dkpt, "dy_pose_loss_bwd: null argument");
  const int ve = dy_vec_elems(d->dtype);
  DY_CHECK(dk_ld >= ((long)d->K * d->ndim + ve - 1) / ve * ve, "dy_pose_loss_bwd: dk_ld %ld below the padded keypoint width",
           (long)dk_ld);
  DyPoseGrad g;
  for (int l = 0; l < DY_POSE_MAX_LEVELS; ++l) {
    g.p[l] = l < p.nl ? dkpt[l] : nullptr;
    DY_CHECK(l >= p.nl || g.p[l], "dy_pose_loss_bwd: null gradient map %d", l);
  }
  const float* img = work + 3L * p.B * p.A;
  const int blocks = dy_cdiv((long)p.B * p.A * dk_ld, NT);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("pose_bwd_kernel");
  DY_DISPATCH_DTYPE("dy_pose_loss_bwd", d->dtype,
                    pose_bwd_kernel<T><<<blocks, NT, 0, st>>>(p, img, grad_out, hyp_pose, hyp_kobj, g, dk_ld));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_pose_kpt_decode(const dy_pose_desc* d, int nc, float* y, void* stream) {
  Pose p;
  if (int e = make_pose(d, p, false, "dy_pose_kpt_decode")) return e;
  DY_CHECK(y && nc > 0, "dy_pose_kpt_decode: bad args");
  dim3 grid(dy_cdiv(p.A, NT), p.K * p.ndim, p.B);
  hipStream_t st = (hipStream_t)stream;
  dy_note_kernel("pose_decode_kernel");
  DY_DISPATCH_DTYPE("dy_pose_kpt_decode", d->dtype, pose_decode_kernel<T><<<grid, NT, 0, st>>>(p, nc, y));
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_kpt_oks(const float* gt, int N, const float* pred, int M, int pred_dim, const float* area, const float* sigma, int K,
                          float eps, float* out, void* stream) {
  DY_CHECK(N >= 0 && M >= 0 && K > 0 && (pred_dim == 2 || pred_dim == 3), "dy_kpt_oks: bad sizes");
  if ((long)N * M == 0) return 0;
  DY_CHECK(gt && pred && area && sigma && out, "dy_kpt_oks: null pointer");
  dy_note_kernel("kpt_oks_kernel");
  kpt_oks_kernel<<<dy_cdiv((long)N * M, NT), NT, 0, (hipStream_t)stream>>>(gt, N, pred, M, pred_dim, area, sigma, K, eps, out);
  DY_LAUNCH_CHECK();
  return 0;
}
