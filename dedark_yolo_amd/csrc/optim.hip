// Fused optimizer step on ONE flat f32 parameter buffer: gradient clipping coefficient, SGD(nesterov)/AdamW/Adam/Adamax/NAdam/RAdam/RMSProp update with
// per-element parameter-group hyper-parameters and the EMA lerp in one pass (reference: BaseTrainer.optimizer_step
// ultralytics/engine/trainer.py:459-467, build_optimizer :611-665, ModelEMA.update ultralytics/utils/torch_utils.py:360-371).
// Pure HBM streaming: 4-5 reads + 3 writes per element instead of ~230 x (5-8) small launches.
#include "dy_host.h"
#include "../../include/dedark_yolo.h"

namespace {

struct Hyp { float lr[4]; float wd[4]; };

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, double* acc) {
  __shared__ float sm[20];
  float s = 0.f;
  const long n4 = n >> 2;
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 v = g4[i];
    s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { float v = g[(n4 << 2) + threadIdx.x]; s += v * v; }
  s = block_sum(s, sm);
  if (threadIdx.x == 0) atomic_add_f64(acc, (double)s);
}

// Coefficient applied to every gradient element: clip factor min(1, max_norm / (|g| + 1e-6)) on the TRUE norm, times 1 / loss_scale
// when the gradients were produced from a scaled loss (fp16, reference GradScaler: unscale_ -> clip -> step).  *skip = the scaled
// gradients hold an inf / NaN: the reference's scaler.step() then leaves parameters and optimizer state untouched.
__device__ inline float step_coef(const double* sumsq, float max_norm, const float* loss_scale, bool* skip) {
  const float inv = loss_scale ? 1.f / loss_scale[0] : 1.f;
  *skip = false;
  if (!sumsq) return inv;
  const double ss = *sumsq;
  if (loss_scale && !(ss < (double)INFINITY)) {
    *skip = true;
    return 0.f;
  }
  const float nrm = (float)sqrt(ss) * inv;
  const float c = max_norm / (nrm + 1e-6f);
  return (c < 1.f ? c : 1.f) * inv;
}

// ModelEMA.update (torch_utils.py:360-371) of one element: the line every step kernel below ends with
__device__ inline float ema_mix(float e, float w, float ed) { return ed * e + (1.f - ed) * w; }

__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, float* __restrict__ ema,
                           const uint8_t* __restrict__ gid, Hyp h, float mom, int nesterov, float ed, const double* sumsq,
                           float max_norm, float gscale, const float* loss_scale, long n) {
  bool skip;
  const float cc = step_coef(sumsq, max_norm, loss_scale, &skip) * gscale;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (skip) {
      if (ema) ema[i] = ema_mix(ema[i], p[i], ed);
      continue;
    }
    const int k = gid ? (gid[i] & 3) : 0;
    float w = p[i];
    float d = g[i] * cc + h.wd[k] * w;
    float b = mom * buf[i] + d;
    buf[i] = b;
    d = nesterov ? d + mom * b : b;
    w -= h.lr[k] * d;
    p[i] = w;
    if (ema) ema[i] = ema_mix(ema[i], w, ed);
  }
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m1, float* __restrict__ m2,
                             float* __restrict__ ema, const uint8_t* __restrict__ gid, Hyp h, float b1, float b2, float eps,
                             int step, float ed, const double* sumsq, float max_norm, float gscale,
                             const float* loss_scale, long n) {
  bool skip;
  const float cc = step_coef(sumsq, max_norm, loss_scale, &skip) * gscale;
  // bias correction counts the steps the optimizer really TOOK: GradScaler.step does not call optimizer.step() after an overflow, so
  // torch's Adam `step` does not advance there; loss_scale[2] = overflowed steps so far (dy_loss_scale_update)
  const float eff = (float)(step - (loss_scale ? (int)loss_scale[2] : 0));
  const float bc1 = 1.f - powf(b1, eff), bc2 = 1.f - powf(b2, eff);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (skip) {
      if (ema) ema[i] = ema_mix(ema[i], p[i], ed);
      continue;
    }
    const int k = gid ? (gid[i] & 3) : 0;
    float w = p[i] * (1.f - h.lr[k] * h.wd[k]);
    float gi = g[i] * cc;
    float a = b1 * m1[i] + (1.f - b1) * gi;
    float v = b2 * m2[i] + (1.f - b2) * gi * gi;
    m1[i] = a;
    m2[i] = v;
    float denom = sqrtf(v) / sqrtf(bc2) + eps;
    w -= (h.lr[k] / bc1) * a / denom;
    p[i] = w;
    if (ema) ema[i] = ema_mix(ema[i], w, ed);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Adam / Adamax / NAdam / RAdam / RMSProp (torch/optim/{adam,adamax,nadam,radam,rmsprop}.py, the _single_tensor_* functions, L2 weight
// decay).  The optimizer's scalar state (steps really taken, NAdam's running mu_product) lives in a dy_optim_state on the device: one
// thread advances it ahead of the element kernel -- unless the step is skipped -- and leaves the step's uniform scalars there.
__global__ void optim_scalars_kernel(dy_optim_state* __restrict__ s, int rule, double b1, double b2, double mdecay, const double* sumsq,
                                     float max_norm, float gscale, const float* loss_scale) {
  if (threadIdx.x || blockIdx.x) return;
  bool skip;
  s->grad_coef = step_coef(sumsq, max_norm, loss_scale, &skip) * gscale;
  s->skipped = skip;
  if (skip) return;                                            // GradScaler.step: optimizer.step() is not called, nothing advances
  const double t = s->step + 1.0;
  s->step = t;
  const double b1t = pow(b1, t), b2t = pow(b2, t), bc1 = 1.0 - b1t, bc2 = 1.0 - b2t;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  if (rule == DY_OPT_ADAM) {
    c0 = bc1, c1 = sqrt(bc2);
  } else if (rule == DY_OPT_ADAMAX) {
    c0 = bc1;
  } else if (rule == DY_OPT_NADAM) {
    const double mu = b1 * (1.0 - 0.5 * pow(0.96, t * mdecay)), mu_next = b1 * (1.0 - 0.5 * pow(0.96, (t + 1.0) * mdecay));
    // torch keeps mu_product as an f32 tensor (mu_product *= mu in f32) and its state_dict stores that: rounding the running product
    // the same way makes a checkpoint in torch's format restore it exactly
    const double mp = (double)((float)s->mu_product * (float)mu);
    s->mu_product = mp;
    c0 = bc2, c1 = (1.0 - mu) / (1.0 - mp), c2 = mu_next / (1.0 - mp * mu_next);
  } else if (rule == DY_OPT_RADAM) {
    const double rho_inf = 2.0 / (1.0 - b2) - 1.0, rho_t = rho_inf - 2.0 * t * b2t / bc2;
    c0 = bc1, c1 = sqrt(bc2);
    if (rho_t > 5.0) c2 = sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t)), c3 = 1.0;
  }
  s->c[0] = (float)c0, s->c[1] = (float)c1, s->c[2] = (float)c2, s->c[3] = (float)c3;
}

struct RuleK { float b1, w1, b2, w2, eps, c0, c1, c2, c3; };   // uniform values of one step; w1 = 1 - beta1, w2 = 1 - beta2

// Tensor.lerp_(end, weight) as ATen evaluates it
__device__ inline float lerp_to(float a, float end, float weight) {
  const float d = end - a;
  return weight < 0.5f ? a + weight * d : end - d * (1.f - weight);
}

// One element of rule R: w = parameter, a / b = the two state buffers, lr = the group's step size (lr / bias_correction1 for Adam and
// Adamax, whose rules have it as one factor), g = clipped and unscaled gradient.
template <int R> __device__ inline void rule_update(float& w, float g, float& a, float& b, float lr, float wd, const RuleK& k) {
  g += wd * w;                                                  // grad.add(param, alpha=weight_decay)
  if constexpr (R == DY_OPT_RMSPROP) {
    a = k.b2 * a + k.w2 * g * g;                                // square_avg, alpha = b2
    const float q = g / (sqrtf(a) + k.eps);
    if (k.b1 > 0.f) {
      b = k.b1 * b + q;                                         // momentum_buffer
      w -= lr * b;
    } else {
      w -= lr * q;
    }
  } else {
    a = lerp_to(a, g, k.w1);                                    // exp_avg
    if constexpr (R == DY_OPT_ADAMAX) {
      b = fmaxf(k.b2 * b, fabsf(g) + k.eps);                    // exp_inf
      w -= lr * a / b;
    } else {
      b = k.b2 * b + k.w2 * g * g;                              // exp_avg_sq
      if constexpr (R == DY_OPT_ADAM) {
        w -= lr * a / (sqrtf(b) / k.c1 + k.eps);
      } else if constexpr (R == DY_OPT_NADAM) {
        const float den = sqrtf(b / k.c0) + k.eps;
        w -= lr * k.c1 * g / den;
        w -= lr * k.c2 * a / den;
      } else {                                                  // RAdam: rectified only once rho_t > 5
        const float ba = a / k.c0;
        w -= k.c3 != 0.f ? ba * lr * (k.c1 / (sqrtf(b) + k.eps)) * k.c2 : ba * lr;
      }
    }
  }
}

__device__ inline float sel3(int k, float x0, float x1, float x2) { return k == 0 ? x0 : (k == 1 ? x1 : x2); }

// nvec 16-byte vectors (0 when a pointer is not 16-byte aligned), then the elements [4 * nvec, n) one by one
template <int R>
__global__ __launch_bounds__(256) void optim_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                    float* __restrict__ s2, float* __restrict__ ema, const uint8_t* __restrict__ gid,
                                                    Hyp h, float b1, float b2, float eps, float ed,
                                                    const dy_optim_state* __restrict__ st, long nvec, long n) {
  const bool skip = st->skipped != 0;
  const float cc = st->grad_coef;
  const RuleK k = {b1, 1.f - b1, b2, 1.f - b2, eps, st->c[0], st->c[1], st->c[2], st->c[3]};
  const bool over_bc1 = R == DY_OPT_ADAM || R == DY_OPT_ADAMAX;
  const float lr0 = over_bc1 ? h.lr[0] / k.c0 : h.lr[0], lr1 = over_bc1 ? h.lr[1] / k.c0 : h.lr[1],
              lr2 = over_bc1 ? h.lr[2] / k.c0 : h.lr[2];
  const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
  f32x4* p4 = reinterpret_cast<f32x4*>(p);
  f32x4* e4 = reinterpret_cast<f32x4*>(ema);
  for (long i = tid; i < nvec; i += stride) {
    f32x4 w = p4[i];
    if (!skip) {
      const f32x4 gv = reinterpret_cast<const f32x4*>(g)[i];
      f32x4 a = reinterpret_cast<f32x4*>(s1)[i], b = reinterpret_cast<f32x4*>(s2)[i];
      const uint32_t ids = gid ? reinterpret_cast<const uint32_t*>(gid)[i] : 0u;       // four group ids, one per element
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int q = (ids >> (8 * j)) & 3;
        float wj = w[j], aj = a[j], bj = b[j];
        rule_update<R>(wj, gv[j] * cc, aj, bj, sel3(q, lr0, lr1, lr2), sel3(q, h.wd[0], h.wd[1], h.wd[2]), k);
        w[j] = wj, a[j] = aj, b[j] = bj;
      }
      reinterpret_cast<f32x4*>(s1)[i] = a;
      if (R != DY_OPT_RMSPROP || k.b1 > 0.f) reinterpret_cast<f32x4*>(s2)[i] = b;
      p4[i] = w;
    }
    if (ema) {
      f32x4 e = e4[i];
#pragma unroll
      for (int j = 0; j < 4; ++j) e[j] = ema_mix(e[j], w[j], ed);
      e4[i] = e;
    }
  }
  for (long i = (nvec << 2) + tid; i < n; i += stride) {
    float w = p[i];
    if (!skip) {
      const int q = gid ? (gid[i] & 3) : 0;
      float a = s1[i], b = s2[i];
      rule_update<R>(w, g[i] * cc, a, b, sel3(q, lr0, lr1, lr2), sel3(q, h.wd[0], h.wd[1], h.wd[2]), k);
      s1[i] = a;
      if (R != DY_OPT_RMSPROP || k.b1 > 0.f) s2[i] = b;
      p[i] = w;
    }
    if (ema) ema[i] = ema_mix(ema[i], w, ed);
  }
}

// dynamic loss scale (torch.cuda.amp.GradScaler.update: growth 2, backoff 0.5, growth_interval 2000):
// st = {scale, consecutive finite steps, overflowed (skipped) steps in total}
__global__ void loss_scale_update_kernel(float* st, const double* sumsq, float growth, float backoff, int interval) {
  if (threadIdx.x || blockIdx.x) return;
  if (!(*sumsq < (double)INFINITY)) {
    st[0] *= backoff;
    st[1] = 0.f;
    st[2] += 1.f;
  } else {
    const float good = st[1] + 1.f;
    if (good >= (float)interval) {
      st[0] *= growth;
      st[1] = 0.f;
    } else {
      st[1] = good;
    }
  }
}

__global__ void ema_lerp_kernel(float* __restrict__ ema, const float* __restrict__ src, float d, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    ema[i] = d * ema[i] + (1.f - d) * src[i];
}

constexpr int EW_CAP = 2048;   // blocks of an element-wise launch

}  // namespace

extern "C" int dy_sumsq(const float* g, int64_t n, double* acc, void* stream) {
  DY_CHECK(g && acc && n >= 0 && ((uintptr_t)g) % 16 == 0, "dy_sumsq: bad args");
  // every block ends with ONE f64 atomic on the same address (~8 ns each, serialised): 256 blocks, not 2048 (30 -> ~8 us at 3 M)
  int blocks = dy_ew_blocks(n / 4 + 1, EW_CAP);
  if (blocks > 256) blocks = 256;
  sumsq_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(g, n, acc);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_sgd_step_scaled(float* p, const float* g, float* mom_buf, float* ema, const uint8_t* group_id, float lr0, float lr1,
                                  float lr2, float wd0, float wd1, float wd2, float momentum, int nesterov, float ema_decay,
                                  const double* sumsq, float max_norm, float grad_scale, const float* loss_scale, int64_t n,
                                  void* stream) {
  DY_CHECK(p && g && mom_buf && n >= 0 && (!loss_scale || sumsq), "dy_sgd_step: bad args");
  if (n == 0) return 0;
  Hyp h = {{lr0, lr1, lr2, lr2}, {wd0, wd1, wd2, wd2}};
  sgd_kernel<<<dy_ew_blocks(n, EW_CAP), 256, 0, (hipStream_t)stream>>>(p, g, mom_buf, ema, group_id, h, momentum, nesterov, ema_decay, sumsq,
                                                            max_norm, grad_scale, loss_scale, n);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_sgd_step(float* p, const float* g, float* mom_buf, float* ema, const uint8_t* group_id, float lr0, float lr1,
                           float lr2, float wd0, float wd1, float wd2, float momentum, int nesterov, float ema_decay,
                           const double* sumsq, float max_norm, float grad_scale, int64_t n, void* stream) {
  return dy_sgd_step_scaled(p, g, mom_buf, ema, group_id, lr0, lr1, lr2, wd0, wd1, wd2, momentum, nesterov, ema_decay, sumsq, max_norm,
                            grad_scale, nullptr, n, stream);
}

extern "C" int dy_adamw_step_scaled(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, const uint8_t* group_id,
                                    float lr0, float lr1, float lr2, float wd0, float wd1, float wd2, float beta1, float beta2,
                                    float eps, int step, float ema_decay, const double* sumsq, float max_norm, float grad_scale,
                                    const float* loss_scale, int64_t n, void* stream) {
  DY_CHECK(p && g && exp_avg && exp_avg_sq && n >= 0 && step >= 1 && (!loss_scale || sumsq), "dy_adamw_step: bad args");
  if (n == 0) return 0;
  Hyp h = {{lr0, lr1, lr2, lr2}, {wd0, wd1, wd2, wd2}};
  adamw_kernel<<<dy_ew_blocks(n, EW_CAP), 256, 0, (hipStream_t)stream>>>(p, g, exp_avg, exp_avg_sq, ema, group_id, h, beta1, beta2, eps, step,
                                                              ema_decay, sumsq, max_norm, grad_scale, loss_scale, n);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_adamw_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, const uint8_t* group_id,
                             float lr0, float lr1, float lr2, float wd0, float wd1, float wd2, float beta1, float beta2, float eps,
                             int step, float ema_decay, const double* sumsq, float max_norm, float grad_scale, int64_t n,
                             void* stream) {
  return dy_adamw_step_scaled(p, g, exp_avg, exp_avg_sq, ema, group_id, lr0, lr1, lr2, wd0, wd1, wd2, beta1, beta2, eps, step,
                              ema_decay, sumsq, max_norm, grad_scale, nullptr, n, stream);
}

extern "C" int dy_optim_step(int rule, float* p, const float* g, float* buf1, float* buf2, float* ema, const uint8_t* group_id, float lr0,
                             float lr1, float lr2, float wd0, float wd1, float wd2, double beta1, double beta2, double eps,
                             double momentum_decay, float ema_decay, const double* sumsq, float max_norm, float grad_scale,
                             const float* loss_scale, dy_optim_state* state, int64_t n, void* stream) {
  DY_CHECK(rule >= DY_OPT_ADAM && rule <= DY_OPT_RMSPROP, "dy_optim_step: bad rule %d", rule);
  DY_CHECK(p && g && buf1 && buf2 && state && ((uintptr_t)state) % 8 == 0 && n >= 0 && (!loss_scale || sumsq), "dy_optim_step: bad args");
  if (n == 0) return 0;
  optim_scalars_kernel<<<1, 1, 0, (hipStream_t)stream>>>(state, rule, beta1, beta2, momentum_decay, sumsq, max_norm, grad_scale, loss_scale);
  DY_LAUNCH_CHECK();
  // 16-byte accesses need every buffer 16-byte aligned (and whole dwords of group ids); otherwise every element takes the scalar loop
  const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)buf1 | (uintptr_t)buf2 | (uintptr_t)ema) % 16 == 0) && ((uintptr_t)group_id % 4 == 0);
  const long nvec = vec ? n >> 2 : 0;
  const Hyp h = {{lr0, lr1, lr2, lr2}, {wd0, wd1, wd2, wd2}};
  const int blocks = dy_ew_blocks(nvec ? nvec : n, EW_CAP);
#define DY_OPTIM_LAUNCH(R)                                                                                                          \
  optim_kernel<R><<<blocks, 256, 0, (hipStream_t)stream>>>(p, g, buf1, buf2, ema, group_id, h, (float)beta1, (float)beta2, (float)eps, \
                                                           ema_decay, state, nvec, n)
  switch (rule) {
    case DY_OPT_ADAM: DY_OPTIM_LAUNCH(DY_OPT_ADAM); break;
    case DY_OPT_ADAMAX: DY_OPTIM_LAUNCH(DY_OPT_ADAMAX); break;
    case DY_OPT_NADAM: DY_OPTIM_LAUNCH(DY_OPT_NADAM); break;
    case DY_OPT_RADAM: DY_OPTIM_LAUNCH(DY_OPT_RADAM); break;
    default: DY_OPTIM_LAUNCH(DY_OPT_RMSPROP); break;
  }
#undef DY_OPTIM_LAUNCH
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_loss_scale_update(float* state, const double* sumsq, float growth, float backoff, int interval, void* stream) {
  DY_CHECK(state && sumsq && growth >= 1.f && backoff > 0.f && backoff <= 1.f && interval >= 1, "dy_loss_scale_update: bad args");
  loss_scale_update_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state, sumsq, growth, backoff, interval);
  DY_LAUNCH_CHECK();
  return 0;
}

namespace {
__global__ void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, long n) {
  const long n4 = n >> 2;
  f32x4* a4 = reinterpret_cast<f32x4*>(acc);
  const f32x4* g4 = reinterpret_cast<const f32x4*>(g);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) a4[i] = a4[i] + g4[i];
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc[(n4 << 2) + threadIdx.x] += g[(n4 << 2) + threadIdx.x];
}
}  // namespace

extern "C" int dy_grad_accumulate(float* acc, const float* g, int64_t n, void* stream) {
  DY_CHECK(acc && g && n >= 0 && ((uintptr_t)acc % 16 == 0) && ((uintptr_t)g % 16 == 0), "dy_grad_accumulate: bad args");
  if (n == 0) return 0;
  grad_accumulate_kernel<<<dy_ew_blocks(n, EW_CAP), 256, 0, (hipStream_t)stream>>>(acc, g, n);
  DY_LAUNCH_CHECK();
  return 0;
}

extern "C" int dy_ema_lerp(float* ema, const float* src, float decay, int64_t n, void* stream) {
  DY_CHECK(ema && src && n >= 0, "dy_ema_lerp: bad args");
  if (n == 0) return 0;
  ema_lerp_kernel<<<dy_ew_blocks(n, EW_CAP), 256, 0, (hipStream_t)stream>>>(ema, src, decay, n);
  DY_LAUNCH_CHECK();
  return 0;
}
