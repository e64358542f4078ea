// Fused optimizer math shared by the flat multi-tensor optimizer kernel
// (csrc/kernels/optim.hip) and the LeNet engine's finalize kernel
// (csrc/kernels/lenet.hip).
//
// Semantics follow torch.optim exactly (the reference selects these by name at
// src/trainer.py:123-138): SGD(momentum, dampening, nesterov, weight_decay as L2),
// Adam (L2 weight decay), AdamW (decoupled decay), Adagrad (lr_decay,
// initial_accumulator_value=0), Adamax (infinity norm).
//
// LAMB (You et al., layer-wise trust ratio; apex FusedLAMB with use_nvlamb=False) is not a
// torch.optim rule and not an element-wise one: tensor i moves along
//   u = (m / bc1) / (sqrtf(v) / sqrtf(bc2) + eps) + wd_i * w
// by lr * r_i with r_i = |w_i| / |u_i| (1 for an excluded tensor or a zero norm), so it needs two
// per-tensor norms between the moment update and the weight update. lamb_moments / lamb_direction /
// lamb_trust / lamb_apply are the pieces; the three launches of optim.hip put them together. The
// moments are Adam's, bit for bit (the same expressions as opt_update_k<OPT_ADAM> with no decay).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mlt {

enum OptKind : int { OPT_SGD = 0, OPT_ADAM = 1, OPT_ADAMW = 2, OPT_ADAGRAD = 3, OPT_ADAMAX = 4, OPT_LAMB = 5 };

struct OptHyper {
  float lr;            // used when lr_ptr == nullptr
  float momentum;
  float dampening;
  float weight_decay;
  // The betas are kept as their complements, rounded to fp32 once from the host's doubles
  // (make_opt_hyper). Kept as (float)beta, 1.f - (float)0.999 is off by 1.3e-5 relative (beta's rounding
  // error against a difference a thousand times smaller), which went straight into exp_avg_sq and,
  // through 1 - powf(beta, t), into the bias corrections. From the complement all come out right:
  // beta = 1.f - omb rounds to (float)beta for beta >= 0.5 (within 3e-8 of it below), and
  // 1 - beta^t = -expm1f(t * log1pf(-omb)) has no cancellation.
  float omb1, omb2;    // 1 - beta1, 1 - beta2
  float eps;
  float lr_decay;      // adagrad
  float grad_scale;    // multiply incoming grads (e.g. 1/world or 1/loss_scale)
  int nesterov;
  int maximize;
  int kind;
};

// The one place that fills an OptHyper from a user's (double) hyper-parameters.
inline OptHyper make_opt_hyper(int kind, double lr, double momentum, double dampening, double weight_decay,
                               double beta1, double beta2, double eps, double lr_decay, double grad_scale,
                               bool nesterov, bool maximize) {
  OptHyper h;
  h.kind = kind;
  h.lr = (float)lr;
  h.momentum = (float)momentum;
  h.dampening = (float)dampening;
  h.weight_decay = (float)weight_decay;
  h.omb1 = (float)(1.0 - beta1);
  h.omb2 = (float)(1.0 - beta2);
  h.eps = (float)eps;
  h.lr_decay = (float)lr_decay;
  h.grad_scale = (float)grad_scale;
  h.nesterov = nesterov ? 1 : 0;
  h.maximize = maximize ? 1 : 0;
  return h;
}

// 1 - beta^t from omb = 1 - beta (beta = 0: log1pf(-1) = -inf, expm1f(-inf) = -1, correction 1)
__device__ __forceinline__ float opt_bias_correction(float omb, float t) { return -expm1f(t * log1pf(-omb)); }

// One element update. s1/s2 are the optimizer state slots for this element:
//   SGD: s1 = momentum buffer; Adam/AdamW/Adamax: s1 = exp_avg, s2 = exp_avg_sq / exp_inf;
//   Adagrad: s1 = state_sum.
// `t` is the 1-based step count (after increment), as torch tracks it.
// opt_update_k<K>: the update of one optimizer kind (compile-time): kernels that dispatch the kind
// once at their top keep only that kind's code on their hot path (a compact instruction footprint);
// opt_update: the same arithmetic behind a runtime switch (bitwise identical).
template <int K>
__device__ __forceinline__ void opt_update_k(const OptHyper& h, float lr, float t, float& p, float g, float& s1,
                                             float& s2) {
  g *= h.grad_scale;
  if (h.maximize) g = -g;
  if constexpr (K == OPT_SGD) {
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    if (h.momentum != 0.f) {
      // torch initialises the buffer to a clone of d_p on the first step.
      float b = (t <= 1.f) ? g : fmaf(h.momentum, s1, (1.f - h.dampening) * g);
      s1 = b;
      g = h.nesterov ? fmaf(h.momentum, b, g) : b;
    }
    p = fmaf(-lr, g, p);
  } else if constexpr (K == OPT_ADAM || K == OPT_ADAMW) {
    if constexpr (K == OPT_ADAMW) {
      p *= (1.f - lr * h.weight_decay);
    } else {
      if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    }
    s1 = fmaf(h.omb1, g - s1, s1);  // torch's lerp_(g, 1 - beta1)
    s2 = fmaf(1.f - h.omb2, s2, h.omb2 * g * g);
    const float bc1 = opt_bias_correction(h.omb1, t);
    const float bc2 = opt_bias_correction(h.omb2, t);
    const float step_size = lr / bc1;
    const float denom = sqrtf(s2) / sqrtf(bc2) + h.eps;
    p = fmaf(-step_size, s1 / denom, p);
  } else if constexpr (K == OPT_ADAGRAD) {
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    const float clr = lr / (1.f + (t - 1.f) * h.lr_decay);
    s1 = fmaf(g, g, s1);
    p = fmaf(-clr, g / (sqrtf(s1) + h.eps), p);
  } else if constexpr (K == OPT_ADAMAX) {
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    s1 = fmaf(h.omb1, g - s1, s1);  // torch's lerp_(g, 1 - beta1)
    s2 = fmaxf((1.f - h.omb2) * s2, fabsf(g) + h.eps);
    const float clr = lr / opt_bias_correction(h.omb1, t);
    p = fmaf(-clr, s1 / s2, p);
  }
}

// ---- LAMB --------------------------------------------------------------------------------
// Moments of one element: g scaled / negated as in opt_update_k, then Adam's exp_avg / exp_avg_sq.
__device__ __forceinline__ void lamb_moments(const OptHyper& h, float g, float& m, float& v) {
  g *= h.grad_scale;
  if (h.maximize) g = -g;
  m = fmaf(h.omb1, g - m, m);
  v = fmaf(1.f - h.omb2, v, h.omb2 * g * g);
}

// Update direction of one element from the UPDATED moments. Stage 1 (norms) and stage 2 (apply) both
// call this with the same m, v, w, so both see the same bits; every fused multiply-add is written
// out, none is left to the compiler's contraction.
__device__ __forceinline__ float lamb_direction(float wd, float eps, float bc1, float bc2, float w, float m,
                                                float v) {
  return fmaf(wd, w, (m / bc1) / (sqrtf(v) / sqrtf(bc2) + eps));
}

// Trust ratio of a tensor from its sums of squares: |w| / |u|, 1 when not adapted or a norm is 0.
__device__ __forceinline__ float lamb_trust(int adapt, float w_sq, float u_sq) {
  return (adapt != 0 && w_sq > 0.f && u_sq > 0.f) ? sqrtf(w_sq) / sqrtf(u_sq) : 1.f;
}

__device__ __forceinline__ float lamb_apply(float lr, float r, float u, float w) { return fmaf(-lr * r, u, w); }

__device__ __forceinline__ void opt_update(const OptHyper& h, float lr, float t, float& p, float g, float& s1,
                                           float& s2) {
  switch (h.kind) {
    case OPT_SGD: opt_update_k<OPT_SGD>(h, lr, t, p, g, s1, s2); break;
    case OPT_ADAM: opt_update_k<OPT_ADAM>(h, lr, t, p, g, s1, s2); break;
    case OPT_ADAMW: opt_update_k<OPT_ADAMW>(h, lr, t, p, g, s1, s2); break;
    case OPT_ADAGRAD: opt_update_k<OPT_ADAGRAD>(h, lr, t, p, g, s1, s2); break;
    case OPT_ADAMAX: opt_update_k<OPT_ADAMAX>(h, lr, t, p, g, s1, s2); break;
    default: break;
  }
}

}  // namespace mlt
