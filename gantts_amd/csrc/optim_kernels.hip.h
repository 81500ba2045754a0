// gantts_amd -- the fused clip_grad_norm_ + optimizer step over a network's flat parameter buffer: ONE kernel frame,
// optim_step_kernel<KIND, F>, and one per-element rule, optim_update<KIND, F>, for every kind of torch.optim's first-order
// family (reference train.py:275-276, 317-318).  Included by eng_ops.hip alone, which holds the table of the legal (KIND, F)
// pairs and the only launch; the squared-norm partials the frame sums come from sqnorm_partial_kernel or
// slab_reduce_norm_kernel (frame_kernels.hip.h).
// One instantiation per (kind, flags): nothing is decided per element.  Each rule restates torch's single-tensor code path
// (torch/optim/<name>.py, _single_tensor_<name>, foreach=False), operation by operation in float32.
// HBM traffic: 16 B per parameter (p and g, read and written) + 8 B per live state buffer, up to three of them (40 B); + 8 B with the
// weight-average rider (gt_set_param_ema: the average read and written).
#pragma once
#include "frame_kernels.hip.h"

namespace gt {

enum OptimKind { OPTK_ADAGRAD = 0, OPTK_ADAM = 1, OPTK_SGD = 2, OPTK_RMSPROP = 3, OPTK_ADADELTA = 4, OPTK_ADAMW = 5, OPTK_ADAMAX = 6,
                 OPTK_NADAM = 7, OPTK_RADAM = 8, OPTK_RPROP = 9, OPTK_ASGD = 10 };
constexpr unsigned OPTI_NESTEROV = 1u, OPTI_CENTERED = 2u, OPTI_AMSGRAD = 4u;   // GT_OPTF_* of the C ABI
constexpr unsigned OPTI_MOMENTUM = 16u;                                         // momentum != 0 (SGD, RMSprop)
constexpr unsigned OPTI_DECOUPLED = 32u;                                        // GT_OPTF_DECOUPLED_WD (NAdam, RAdam)
constexpr unsigned OPTI_RECTIFIED = 64u;                                        // RAdam: rho_t > 5 at this step; decided by the host
constexpr unsigned OPTI_AVERAGE = 128u;                                         // ASGD: mu != 1 at this step; decided by the host
// Adagrad, and Adam without amsgrad: the project's two original kinds keep the arithmetic they were first written with.  Their
// three step scalars (clr, step_size, bc2_sqrt) are formed IN the kernel, in double, from the float-rounded hyper-parameters (the
// device pow, which need not round as the host's does); Adam is beta1 * m + (1 - beta1) * g (not torch's lerp) and the step is
// step_size * (m / denom).  Every other pair -- Adam WITH amsgrad among them -- takes its scalars from the host, formed in double
// from the double hyper-parameters and rounded once (optim_spec, eng_ops.hip), and torch's operations one by one.  Plain Adam
// and Adam with amsgrad therefore differ in the last bits beyond the maximum itself.
constexpr unsigned OPTI_ORIGINAL = 256u;

struct OptimSpec {
  float max_norm;      // clip threshold (1.0 in the reference); <= 0 disables clipping
  float wd;            // weight_decay
  float eps;
  float neg_step;      // -lr (SGD, RMSprop, Adadelta), -lr / (1 - beta1^t) (Adam, AdamW, Adamax), -eta (ASGD)
  float decay;         // AdamW, decoupled NAdam / RAdam: 1 - lr * weight_decay; ASGD: 1 - lambd * eta
  float mu;            // momentum; ASGD: the averaging weight mu
  float omd;           // SGD: 1 - dampening
  float a, oma;        // RMSprop alpha, Adadelta rho, Adam / Adamax beta2, and one minus it
  float w1;            // Adam / Adamax: 1 - beta1 (the lerp weight)
  float bc2_sqrt;      // Adam: sqrt(1 - beta2^t)
  int live;            // SGD: momentum_buffer holds a value (not the first update)
  float lr;            // RAdam, OPTI_ORIGINAL: lr
  float bc1;           // RAdam: 1 - beta1^t
  float bc2;           // NAdam: 1 - beta2^t
  float rect;          // RAdam: the variance rectification term (OPTI_RECTIFIED)
  float c_g, c_m;      // NAdam: -lr (1 - mu_t) / (1 - mu_product_t), -lr mu_{t+1} / (1 - mu_product_t mu_{t+1})
  float eta_minus, eta_plus, step_min, step_max;      // Rprop
  float lr_decay;      // OPTI_ORIGINAL Adagrad
  float beta1, beta2;  // OPTI_ORIGINAL Adam
  long step;           // OPTI_ORIGINAL: 1-based step count of THIS update
  float wclip;         // gt_set_weight_clip: > 0 clamps every updated parameter to [-wclip, wclip] behind the rule (param.clamp_ after optimizer.step()); 0: off
  float* ema;          // gt_set_param_ema: the running average of the parameters, updated from every STORED parameter (behind rule and clamp); null: off
  float ema_w;         // its lerp weight, float32(1.0 - decay)
  int ema_first;       // the first applied update: the average becomes a copy of the stored parameters (AveragedModel, n_averaged == 0)
};
// which of the three state streams a (kind, flags) pair reads and writes
template <int KIND, unsigned F> struct OptimStreams {
  static constexpr bool s0 = KIND != OPTK_SGD || (F & OPTI_MOMENTUM) != 0;
  static constexpr bool s1 = (KIND == OPTK_ADAGRAD || KIND == OPTK_SGD || KIND == OPTK_ASGD) ? false
                             : KIND == OPTK_RMSPROP ? (F & OPTI_MOMENTUM) != 0 : true;
  static constexpr bool s2 = KIND == OPTK_RMSPROP ? (F & OPTI_CENTERED) != 0 : (KIND == OPTK_ADAM || KIND == OPTK_ADAMW) && (F & OPTI_AMSGRAD) != 0;
};
// OPTI_ORIGINAL: the step scalars formed in the kernel, into the fields the host fills for every other pair
// (neg_step = -clr for Adagrad, -step_size for Adam; bc2_sqrt)
template <int KIND>
__device__ __forceinline__ void optim_original_scalars(OptimSpec& o) {
  if (KIND == OPTK_ADAGRAD) {
    o.neg_step = -(o.lr / (1.f + (float)(o.step - 1) * o.lr_decay));
  } else {
    const double bc1 = 1.0 - pow((double)o.beta1, (double)o.step);
    const double bc2 = 1.0 - pow((double)o.beta2, (double)o.step);
    o.neg_step = -(float)((double)o.lr / bc1);
    o.bc2_sqrt = (float)sqrt(bc2);
  }
}
// Tensor.lerp_(end, weight) as ATen evaluates it (aten/src/ATen/native/Lerp.h): the form that is exact at the nearer end
__device__ __forceinline__ float torch_lerp(float a, float b, float w) { return w < 0.5f ? a + w * (b - a) : b - (b - a) * (1.f - w); }

// one element of clip_grad_norm_ + the update (`coef` = the clip coefficient).  The clipped gradient is written back
// (clip_grad_norm_ scales .grad in place).
template <int KIND, unsigned F>
__device__ __forceinline__ void optim_update(float& p, float& g, float& s0, float& s1, float& s2, float coef, const OptimSpec& o) {
  float gi = g * coef;
  g = gi;
  float pi = p;
  if constexpr ((F & OPTI_ORIGINAL) != 0) {
    // Every fused multiply-add these two rules have always been compiled to is spelled out, and the compiler forms no other:
    // their bits (tests/golden/optim_step_digests.json) do not hang on what the vectoriser makes of an a * b + c.
#pragma clang fp contract(off)
    if (o.wd != 0.f) gi = fmaf(o.wd, pi, gi);
    if (KIND == OPTK_ADAGRAD) {
      const float s = fmaf(gi, gi, s0);
      s0 = s;
      p = fmaf(o.neg_step, gi / (sqrtf(s) + o.eps), pi);                  // pi - clr * (gi / (sqrt(s) + eps))
    } else {
      const float m = fmaf(o.beta1, s0, (1.f - o.beta1) * gi);            // beta1 * m + (1 - beta1) * g: not torch's lerp
      const float v = o.beta2 * s1 + (1.f - o.beta2) * gi * gi;           // three products and a sum, each rounded
      s0 = m; s1 = v;
      const float denom = sqrtf(v) / o.bc2_sqrt + o.eps;
      p = fmaf(o.neg_step, m / denom, pi);                                // pi - step_size * (m / denom)
    }
    return;
  }
  if (KIND == OPTK_ADAMW || (F & OPTI_DECOUPLED)) {      // decoupled_weight_decay: param.mul_(1 - lr * weight_decay)
    if (o.wd != 0.f) pi *= o.decay;
  } else if (o.wd != 0.f) {
    gi = gi + o.wd * pi;                      // grad.add(param, alpha=weight_decay)
  }
  if (KIND == OPTK_SGD) {                     // _single_tensor_sgd
    if (F & OPTI_MOMENTUM) {
      const float buf = o.live ? s0 * o.mu + o.omd * gi : gi;     // buf = clone(grad) on the first update, else buf.mul_(mu).add_(grad, alpha=1 - dampening)
      s0 = buf;
      gi = (F & OPTI_NESTEROV) ? gi + o.mu * buf : buf;
    }
    p = pi + o.neg_step * gi;
  } else if (KIND == OPTK_RMSPROP) {          // _single_tensor_rmsprop
    const float sq = s0 * o.a + (o.oma * gi) * gi;                // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    s0 = sq;
    float avg;
    if (F & OPTI_CENTERED) {
      const float ga = torch_lerp(s2, gi, o.oma);                 // grad_avg.lerp_(grad, 1 - alpha)
      s2 = ga;
      avg = sqrtf(sq + (-ga) * ga);                               // square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
    } else {
      avg = sqrtf(sq);
    }
    avg += o.eps;
    if (F & OPTI_MOMENTUM) {
      const float buf = s1 * o.mu + gi / avg;                     // buf.mul_(momentum).addcdiv_(grad, avg)
      s1 = buf;
      p = pi + o.neg_step * buf;
    } else {
      p = pi + (o.neg_step * gi) / avg;                           // param.addcdiv_(grad, avg, value=-lr)
    }
  } else if (KIND == OPTK_ADADELTA) {         // _single_tensor_adadelta
    const float sq = s0 * o.a + (o.oma * gi) * gi;
    s0 = sq;
    const float delta = sqrtf(s1 + o.eps) / sqrtf(sq + o.eps) * gi;
    s1 = s1 * o.a + (o.oma * delta) * delta;
    p = pi + o.neg_step * delta;
  } else if (KIND == OPTK_ADAM || KIND == OPTK_ADAMW) {           // _single_tensor_adam
    const float m = torch_lerp(s0, gi, o.w1);                     // exp_avg.lerp_(grad, 1 - beta1)
    const float v = s1 * o.a + (o.oma * gi) * gi;                 // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    s0 = m; s1 = v;
    float vd = v;
    if (F & OPTI_AMSGRAD) { vd = fmaxf(s2, v); s2 = vd; }         // torch.maximum(max_exp_avg_sq, exp_avg_sq, out=max_exp_avg_sq)
    const float denom = sqrtf(vd) / o.bc2_sqrt + o.eps;
    p = pi + (o.neg_step * m) / denom;                            // param.addcdiv_(exp_avg, denom, value=-step_size)
  } else if (KIND == OPTK_ADAMAX) {           // _single_tensor_adamax
    const float m = torch_lerp(s0, gi, o.w1);
    const float u = fmaxf(s1 * o.a, fabsf(gi) + o.eps);           // torch.maximum(exp_inf.mul_(beta2), grad.abs().add_(eps), out=exp_inf)
    s0 = m; s1 = u;
    p = pi + (o.neg_step * m) / u;                                // param.addcdiv_(exp_avg, exp_inf, value=-clr)
  } else if (KIND == OPTK_NADAM) {            // _single_tensor_nadam
    const float m = torch_lerp(s0, gi, o.w1);
    const float v = s1 * o.a + (o.oma * gi) * gi;
    s0 = m; s1 = v;
    const float denom = sqrtf(v / o.bc2) + o.eps;                 // exp_avg_sq.div(bias_correction2).sqrt().add_(eps)
    pi = pi + (o.c_g * gi) / denom;                               // param.addcdiv_(grad, denom, value=-lr (1 - mu) / (1 - mu_product))
    p = pi + (o.c_m * m) / denom;                                 // param.addcdiv_(exp_avg, denom, value=-lr mu_next / (1 - mu_product_next))
  } else if (KIND == OPTK_RADAM) {            // _single_tensor_radam
    const float m = torch_lerp(s0, gi, o.w1);
    const float v = s1 * o.a + (o.oma * gi) * gi;
    s0 = m; s1 = v;
    const float upd = (m / o.bc1) * o.lr;                         // bias_corrected_exp_avg * lr
    if (F & OPTI_RECTIFIED) {
      const float adaptive = (1.f / (sqrtf(v) + o.eps)) * o.bc2_sqrt;      // bias_correction2 ** 0.5 / exp_avg_sq.sqrt().add_(eps): reciprocal, then the scalar
      p = pi - (upd * adaptive) * o.rect;
    } else {
      p = pi - upd;
    }
  } else if (KIND == OPTK_RPROP) {            // _single_tensor_rprop: s0 = prev, s1 = step_size
    const float dir = gi * s0;                                    // grad.mul(prev).sign(), as the float32 product
    const float factor = dir > 0.f ? o.eta_plus : dir < 0.f ? o.eta_minus : 1.f;
    const float st = fminf(fmaxf(s1 * factor, o.step_min), o.step_max);      // step_size.mul_(sign).clamp_(min, max)
    const float gz = dir < 0.f ? 0.f : gi;                        // grad[sign.eq(etaminus)] = 0
    const float sg = gz > 0.f ? 1.f : gz < 0.f ? -1.f : 0.f;
    p = pi - sg * st;                                             // param.addcmul_(grad.sign(), step_size, value=-1)
    s0 = gz; s1 = st;                                             // prev.copy_(grad)
  } else {                                    // _single_tensor_asgd: s0 = ax
    pi = pi * o.decay;                                            // param.mul_(1 - lambd * eta)
    pi = pi + o.neg_step * gi;                                    // param.add_(grad, alpha=-eta)
    p = pi;
    s0 = (F & OPTI_AVERAGE) ? s0 + (pi - s0) * o.mu : pi;         // ax.add_(param.sub(ax).mul_(mu)), or ax.copy_(param) while mu == 1
  }
}

// AveragedModel.update_parameters with get_ema_multi_avg_fn(decay): ema.lerp_(p, w) as this torch build's CPU path evaluates it, ONE fused
// multiply-add per element in the form that is exact at the nearer end.  Spelled out, not left to contraction (torch_lerp above, with its two
// roundings where the compiler does not contract, stays what the rules were pinned with).
__device__ __forceinline__ float ema_lerp(float ema, float p, float w) {
  const float d = p - ema;
  return w < 0.5f ? fmaf(w, d, ema) : fmaf(-(1.f - w), d, p);
}

// the elements of one thread: clip coefficient and step scalars are known.  CLIP: each updated parameter is clamped to [-wclip, wclip]
// behind the rule and before the store -- two comparisons, so that a NaN parameter stays a NaN, as Tensor.clamp_ leaves it.
// EMA: the average's four loads join the group of p / g / s0..s2; its update reads the value that is stored, behind rule and clamp.
template <int KIND, unsigned F, bool CLIP, bool EMA>
__device__ __forceinline__ void optim_step_elements(float* __restrict__ p, float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1,
                                                    float* __restrict__ s2, long n, float coef, const OptimSpec& o) {
  typedef OptimStreams<KIND, F> S;
  float* __restrict__ const ema = EMA ? o.ema : (float*)nullptr;      // (no other stream of this launch: gt_set_param_ema's buffer is the caller's own)
  // four grid strides per trip: the loads of four elements are in flight together (a thread of the cfg2 generator's launch walks 3-4)
  const long gstride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i < n; i += 4 * gstride) {      // (the last trip is predicated: no one-element tail)
    float pv[4], gv[4], av[4], bv[4], cv[4], ev[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long k = i + u * gstride;
      const bool ok = k < n;
      pv[u] = ok ? p[k] : 0.f; gv[u] = ok ? g[k] : 0.f;
      av[u] = (S::s0 && ok) ? s0[k] : 0.f; bv[u] = (S::s1 && ok) ? s1[k] : 0.f; cv[u] = (S::s2 && ok) ? s2[k] : 0.f;
      ev[u] = (EMA && ok) ? ema[k] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long k = i + u * gstride;
      if (k >= n) continue;
      optim_update<KIND, F>(pv[u], gv[u], av[u], bv[u], cv[u], coef, o);
      if (CLIP) pv[u] = pv[u] < -o.wclip ? -o.wclip : pv[u] > o.wclip ? o.wclip : pv[u];
      p[k] = pv[u]; g[k] = gv[u];
      if (S::s0) s0[k] = av[u];
      if (S::s1) s1[k] = bv[u];
      if (S::s2) s2[k] = cv[u];
      if (EMA) ema[k] = o.ema_first ? pv[u] : ema_lerp(ev[u], pv[u], o.ema_w);
    }
  }
}

// EMA: the weight-average rider (gt_set_param_ema; o.ema is then not null).  A template parameter of the KERNEL, chosen by the launch, and not
// a third uniform test beside wclip's: as a test it cost every instantiation some 20 VGPRs -- a kernel is allocated for its widest path -- and
// 16 of the 23 an occupancy step with the average off (Adagrad 6 -> 4 waves per SIMD, the amsgrad rows 4 -> 3: fewer than the 1024 workgroups
// of a large launch resident at once).  With EMA = false this is the kernel that was always here.
template <int KIND, unsigned F, bool EMA = false>
static __global__ __launch_bounds__(RED_THREADS) void optim_step_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ s0, float* __restrict__ s1, float* __restrict__ s2, long n,
    const double* __restrict__ norm_partial, int n_partial, double* __restrict__ norm2_out, OptimSpec o,
    const unsigned int* __restrict__ fault_dev, unsigned int* fault_host /* pinned, or null */,
    unsigned int* skipped_host /* pinned, or null */,
    const float* __restrict__ gscale /* or null: the gradient in g is that of a loss still to be multiplied by *gscale (1 / Tv) */) {
  __shared__ float coef_sh;
  __shared__ double shn[16];
  // A persistent launch of this step that gave up raised the device fault word: its gradients are garbage.  Mirror the
  // word to the host (no copy launch) and leave parameters, gradients and optimizer state untouched; the skipped step
  // is counted so that gt_clear_faults can take it back out of the host's step counter.
  if (fault_dev && *fault_dev) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (fault_host) *fault_host = *fault_dev;
      if (skipped_host) *skipped_host += 1u;
      if (norm2_out) *norm2_out = __longlong_as_double(0x7ff8000000000000LL);   // no update, no norm: NaN, not the previous step's value
    }
    return;
  }
  double part = 0.0;
  {
    const int bd = blockDim.x;
    int i = threadIdx.x;
    for (; i + 3 * bd < n_partial; i += 4 * bd) {      // four partials in flight per thread, added in index order as before
      const double a0 = norm_partial[i], a1 = norm_partial[i + bd], a2 = norm_partial[i + 2 * bd], a3 = norm_partial[i + 3 * bd];
      part += a0; part += a1; part += a2; part += a3;
    }
    for (; i < n_partial; i += bd) part += norm_partial[i];
  }
  double tot = block_sum_d(part, shn);      // same fixed order in every workgroup
  if (threadIdx.x == 0) {
    const float gsc = gscale ? *gscale : 1.f;
    tot *= (double)gsc * (double)gsc;
    if (blockIdx.x == 0 && norm2_out) *norm2_out = tot;
    float coef = 1.f;
    if (o.max_norm > 0.f) {
      const float total_norm = (float)sqrt(tot);
      coef = fminf(o.max_norm / (total_norm + 1e-6f), 1.f);
    }
    coef_sh = coef * gsc;       // (the scaled, clipped gradient is what optim_update writes back)
  }
  __syncthreads();
  const float coef = coef_sh;
  if constexpr ((F & OPTI_ORIGINAL) != 0) optim_original_scalars<KIND>(o);
  // weight clipping (gt_set_weight_clip): ONE uniform test of a spec field per thread, not a row of the (kind, flags) table and not a
  // test per element.  With the field 0 the elements go through the loop that was always here, compiled from the same statements.
  if (o.wclip > 0.f) optim_step_elements<KIND, F, true, EMA>(p, g, s0, s1, s2, n, coef, o);
  else optim_step_elements<KIND, F, false, EMA>(p, g, s0, s1, s2, n, coef, o);
}

}  // namespace gt
