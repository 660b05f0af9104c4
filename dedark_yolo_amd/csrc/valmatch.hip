// Validation bookkeeping of a whole batch in one launch (reference ultralytics/models/yolo/detect/val.py:72-116, 151-174 and
// ultralytics/utils/metrics.py:209-253).  The reference walks the images in Python: scale_boxes on the detections and on the labels,
// box_iou, `_process_batch` (a sort / unique pass per IoU threshold) and ConfusionMatrix.process_batch.  Here one workgroup owns one
// image:
//
//   1. labels  xywh (normalised) -> xyxy -> x (W, H, W, H) -> - pad -> / gain -> clamp   (ops.py:95-125 scale_boxes, f32, that order)
//      detections xyxy                                     -> - pad -> / gain -> clamp
//   2. every detection walks the image's labels once: IoU = inter / (a1 + a2 - inter + 1e-7) (metrics.box_iou).  It keeps
//        * for `correct`: the best label of its own class (an exact tie -> the higher label index) and the bit mask of the thresholds
//          that IoU reaches.  The chosen label does not depend on the threshold, only whether the detection takes part does;
//        * for the confusion matrix, if conf > conf_thres: the best label of any class with IoU > iou_thres (tie -> lower label index).
//   3. `correct`: a detection is correct at threshold k when it takes part at k and no detection of lower index that chose the same
//      label does.  Its mask loses the bits of those detections: one pass over the detections in front of it, no table per label.
//   4. confusion: every label looks for the best-overlapping detection that chose it (tie -> lower detection index): matched ->
//      [det cls][gt cls] += 1, else [nc][gt cls] += 1; then, if the image has a match, every counted unmatched detection adds
//      [det cls][nc].  Integer atomics: the accumulated matrix does not depend on the order of the workgroups.
//
// dy_val_iou_match runs steps 2 (`correct` half) and 3 on IoU matrices that already exist (mask IoU, OKS).
// Every comparison against a threshold must see the bits the host statement sees: csrc/Makefile builds this file with
// -ffp-contract=off, the quotient is one IEEE division.
#include "dy_common.h"

namespace {

constexpr int VM_THREADS = 256;
constexpr int VM_MAX_T = 16;
constexpr int VM_SLOTS = 5;                       // ints of per-detection state: label, mask, confusion label, confusion IoU, matched
constexpr int VM_LDS_BYTES = 40 * 1024;           // per-detection state up to this size lives in LDS, else in the caller's workspace

// the matching rule of engine/validator.match_from_iou.  `iou(i, j)` = overlap of label i and detection j; lcls [M]; dcls(j) = class
// of detection j.  st_label / st_mask: N ints each (LDS or global, private to the workgroup).  correct: [max_det][T] of this image.
template <class IouFn, class ClsFn>
__device__ inline void vm_match(int M, int N, int max_det, const float* __restrict__ lcls, ClsFn dcls, IouFn iou,
                                const float* s_iouv, int T, int* st_label, int* st_mask, unsigned char* __restrict__ correct) {
  const int tid = threadIdx.x;
  for (int j = tid; j < N; j += VM_THREADS) {
    const float dc = dcls(j);
    float best = -1.f;
    int bl = -1;
    for (int i = 0; i < M; ++i) {
      if (lcls[i] != dc) continue;
      const float v = iou(i, j);
      if (v >= best) { best = v; bl = i; }         // >= : the last maximum, the higher label index on an exact tie
    }
    int mask = 0;
    if (bl >= 0)
      for (int k = 0; k < T; ++k) mask |= (best >= s_iouv[k]) ? (1 << k) : 0;
    st_label[j] = bl;
    st_mask[j] = mask;
  }
  __syncthreads();
  for (int j = tid; j < max_det; j += VM_THREADS) {
    int mask = 0;
    if (j < N) {
      mask = st_mask[j];
      const int l = st_label[j];
      for (int j2 = 0; j2 < j && mask; ++j2)
        if (st_label[j2] == l) mask &= ~st_mask[j2];
    }
    for (int k = 0; k < T; ++k) correct[(long)j * T + k] = (unsigned char)((mask >> k) & 1);
  }
}

__device__ inline float vm_scale(float v, float pad, float gain, float hi) {
  v = __fdiv_rn(__fsub_rn(v, pad), gain);
  v = v < 0.f ? 0.f : v;
  return v > hi ? hi : v;
}

__device__ inline float vm_box_iou(const float4 a, const float area_a, const float4 b, const float area_b) {
  const float w = fmaxf(__fsub_rn(fminf(a.z, b.z), fmaxf(a.x, b.x)), 0.f);
  const float h = fmaxf(__fsub_rn(fminf(a.w, b.w), fmaxf(a.y, b.y)), 0.f);
  const float inter = __fmul_rn(w, h);
  return __fdiv_rn(inter, __fadd_rn(__fsub_rn(__fadd_rn(area_a, area_b), inter), 1e-7f));
}

__device__ inline float vm_area(const float4 b) { return __fmul_rn(__fsub_rn(b.z, b.x), __fsub_rn(b.w, b.y)); }

__global__ __launch_bounds__(VM_THREADS) void val_box_match_kernel(
    const float* __restrict__ det, int ld, const int* __restrict__ ocnt, int max_det, const float* __restrict__ lcls_all,
    const float* __restrict__ lxywh, const int* __restrict__ loff, int L, float W, float H, const float* __restrict__ rec,
    const float* __restrict__ iouv, int T, int single_cls, float conf_thres, float iou_thres, int nc, unsigned char* __restrict__ correct,
    float* predn, float* tboxn, int* __restrict__ confusion, int* ws) {
  extern __shared__ int vm_lds[];
  __shared__ float s_iouv[VM_MAX_T];
  __shared__ int s_any;
  const int b = blockIdx.x, tid = threadIdx.x;
  int N = ocnt[b];
  N = N < 0 ? 0 : (N > max_det ? max_det : N);
  int l0 = loff[b];                                // offsets outside [0, L] read as an image without labels
  int M = loff[b + 1] - l0;
  if (l0 < 0 || M < 0 || (long)l0 + M > L) { l0 = 0; M = 0; }
  const float gain = rec[b * 5], padx = rec[b * 5 + 1], pady = rec[b * 5 + 2], h0 = rec[b * 5 + 3], w0 = rec[b * 5 + 4];
  int* st = ws ? ws + (long)b * max_det * VM_SLOTS : vm_lds;
  int* st_label = st;
  int* st_mask = st + max_det;
  int* st_clabel = st + 2 * max_det;
  float* st_ciou = (float*)(st + 3 * max_det);
  int* st_matched = st + 4 * max_det;
  if (tid < T) s_iouv[tid] = iouv[tid];
  if (tid == 0) s_any = 0;
  const float* dimg = det + (long)b * max_det * ld;
  float* pn = predn + (long)b * max_det * 4;
  float4* tb = (float4*)tboxn + l0;
  const float* lcls = lcls_all + l0;

  // 1. native-space labels and detections
  for (int i = tid; i < M; i += VM_THREADS) {
    const float4 q = ((const float4*)lxywh)[l0 + i];
    const float dw = q.z / 2, dh = q.w / 2;
    float4 o;
    o.x = vm_scale(__fmul_rn(__fsub_rn(q.x, dw), W), padx, gain, w0);
    o.y = vm_scale(__fmul_rn(__fsub_rn(q.y, dh), H), pady, gain, h0);
    o.z = vm_scale(__fmul_rn(__fadd_rn(q.x, dw), W), padx, gain, w0);
    o.w = vm_scale(__fmul_rn(__fadd_rn(q.y, dh), H), pady, gain, h0);
    tb[i] = o;
  }
  for (int j = tid; j < max_det; j += VM_THREADS) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < N) {
      const float* p = dimg + (long)j * ld;
      o.x = vm_scale(p[0], padx, gain, w0);
      o.y = vm_scale(p[1], pady, gain, h0);
      o.z = vm_scale(p[2], padx, gain, w0);
      o.w = vm_scale(p[3], pady, gain, h0);
    }
    ((float4*)pn)[j] = o;
  }
  __syncthreads();

  // 2. (confusion half) the label a counted detection overlaps most, of any class
  if (confusion)
    for (int j = tid; j < N; j += VM_THREADS) {
      float cbest = iou_thres;
      int cl = -1;
      if (dimg[(long)j * ld + 4] > conf_thres) {
        const float4 db = ((const float4*)pn)[j];
        const float da = vm_area(db);
        for (int i = 0; i < M; ++i) {
          const float4 lb = tb[i];
          const float v = vm_box_iou(lb, vm_area(lb), db, da);
          if (v > cbest) { cbest = v; cl = i; }    // > : above the threshold, and the lower label index on an exact tie
        }
      }
      st_clabel[j] = cl;
      st_ciou[j] = cbest;
      st_matched[j] = 0;
    }

  // 2. + 3. `correct`
  auto dcls = [&](int j) { return single_cls ? 0.f : dimg[(long)j * ld + 5]; };
  auto iou = [&](int i, int j) {
    const float4 lb = tb[i], db = ((const float4*)pn)[j];
    return vm_box_iou(lb, vm_area(lb), db, vm_area(db));
  };
  vm_match(M, N, max_det, lcls, dcls, iou, s_iouv, T, st_label, st_mask, correct + (long)b * max_det * T);
  if (!confusion) return;
  __syncthreads();

  // 4. confusion matrix [predicted][true], background = nc
  const int ncp = nc + 1;
  for (int i = tid; i < M; i += VM_THREADS) {
    const int gc = (int)lcls[i];
    if (gc < 0 || gc >= nc) continue;
    float bv = 0.f;
    int w = -1;
    for (int j = 0; j < N; ++j)
      if (st_clabel[j] == i && (w < 0 || st_ciou[j] > bv)) { bv = st_ciou[j]; w = j; }     // the lower detection index on a tie
    int row = nc;
    if (w >= 0) {
      st_matched[w] = 1;
      s_any = 1;
      const int dc = (int)dcls(w);
      row = (dc >= 0 && dc < nc) ? dc : -1;
    }
    if (row >= 0) atomicAdd(&confusion[row * ncp + gc], 1);
  }
  __syncthreads();
  if (s_any)
    for (int j = tid; j < N; j += VM_THREADS)
      if (!st_matched[j] && dimg[(long)j * ld + 4] > conf_thres) {
        const int dc = (int)dcls(j);
        if (dc >= 0 && dc < nc) atomicAdd(&confusion[dc * ncp + nc], 1);
      }
}

__global__ __launch_bounds__(VM_THREADS) void val_iou_match_kernel(
    const float* __restrict__ iou_all, const long long* __restrict__ moff, const float* __restrict__ det, int ld,
    const int* __restrict__ ocnt, int max_det, const float* __restrict__ lcls_all, const int* __restrict__ loff, int L,
    long long iou_numel, const float* __restrict__ iouv, int T, int single_cls, unsigned char* __restrict__ correct, int* ws) {
  extern __shared__ int vm_lds[];
  __shared__ float s_iouv[VM_MAX_T];
  const int b = blockIdx.x, tid = threadIdx.x;
  int N = ocnt[b];
  N = N < 0 ? 0 : (N > max_det ? max_det : N);
  int l0 = loff[b];                                // offsets outside [0, L] read as an image without labels
  int M = loff[b + 1] - l0;
  if (l0 < 0 || M < 0 || (long)l0 + M > L) { l0 = 0; M = 0; }
  int* st = ws ? ws + (long)b * max_det * VM_SLOTS : vm_lds;
  if (tid < T) s_iouv[tid] = iouv[tid];
  __syncthreads();
  const float* dimg = det + (long)b * max_det * ld;
  const long long m0 = moff[b];
  if (m0 < 0 || m0 + (long long)M * N > iou_numel) M = 0;       // a matrix outside the buffer reads as no labels
  const float* mat = iou_all + (M ? m0 : 0);
  auto dcls = [&](int j) { return single_cls ? 0.f : dimg[(long)j * ld + 5]; };
  auto iou = [&](int i, int j) { return mat[(long)i * N + j]; };
  vm_match(M, N, max_det, lcls_all + l0, dcls, iou, s_iouv, T, st, st + max_det, correct + (long)b * max_det * T);
}

int vm_check(const char* who, int B, int max_det, int ld, int T) {
  DY_CHECK(B >= 0 && max_det > 0 && ld >= 6, "%s: bad sizes B=%d max_det=%d ld=%d", who, B, max_det, ld);
  DY_CHECK(T >= 1 && T <= VM_MAX_T, "%s: %d IoU thresholds (1..%d)", who, T, VM_MAX_T);
  DY_CHECK((int64_t)B * max_det * (ld > T ? ld : T) < (1LL << 31), "%s: index range", who);
  return 0;
}

// bytes of global workspace the per-detection state needs (0: it fits in LDS)
size_t vm_workspace(int B, int max_det) {
  const size_t per = (size_t)max_det * VM_SLOTS * sizeof(int);
  return per <= (size_t)VM_LDS_BYTES ? 0 : per * (size_t)(B > 0 ? B : 0);
}

}  // namespace

extern "C" int dy_val_box_match(const float* det, int ld, const int* ocnt, int B, int max_det, const float* lcls, const float* lxywh,
                                const int* loff, int L, int H, int W, const float* rec, const float* iouv, int T, int single_cls,
                                float conf_thres, float iou_thres, int nc, uint8_t* correct, float* predn, float* tboxn,
                                int32_t* confusion, void* workspace, void* stream) {
  if (vm_check("dy_val_box_match", B, max_det, ld, T)) return 1;
  DY_CHECK(L >= 0 && H > 0 && W > 0 && nc > 0 && nc < 32768, "dy_val_box_match: bad H=%d W=%d nc=%d", H, W, nc);
  DY_CHECK((((uintptr_t)lxywh | (uintptr_t)predn | (uintptr_t)tboxn) & 15) == 0, "dy_val_box_match: boxes must be 16-byte aligned");
  const size_t need = vm_workspace(B, max_det);
  DY_CHECK(need == 0 || workspace != nullptr, "dy_val_box_match: max_det=%d needs a workspace of %zu bytes", max_det, need);
  if (B == 0) return 0;
  const size_t lds = need ? 0 : (size_t)max_det * VM_SLOTS * sizeof(int);
  val_box_match_kernel<<<B, VM_THREADS, lds, (hipStream_t)stream>>>(det, ld, ocnt, max_det, lcls, lxywh, loff, L, (float)W, (float)H, rec,
                                                                     iouv, T, single_cls, conf_thres, iou_thres, nc, correct, predn,
                                                                     tboxn, confusion, need ? (int*)workspace : nullptr);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_val_iou_match(const float* iou, int64_t iou_numel, const int64_t* moff, const float* det, int ld, const int* ocnt, int B, int max_det,
                                const float* lcls, const int* loff, int L, const float* iouv, int T, int single_cls,
                                uint8_t* correct, void* workspace, void* stream) {
  if (vm_check("dy_val_iou_match", B, max_det, ld, T)) return 1;
  const size_t need = vm_workspace(B, max_det);
  DY_CHECK(need == 0 || workspace != nullptr, "dy_val_iou_match: max_det=%d needs a workspace of %zu bytes", max_det, need);
  if (B == 0) return 0;
  const size_t lds = need ? 0 : (size_t)max_det * VM_SLOTS * sizeof(int);
  val_iou_match_kernel<<<B, VM_THREADS, lds, (hipStream_t)stream>>>(iou, (const long long*)moff, det, ld, ocnt, max_det, lcls, loff, L,
                                                                     (long long)iou_numel, iouv, T, single_cls, correct, need ? (int*)workspace : nullptr);
  DY_LAUNCH_CHECK();
  return 0;
}
