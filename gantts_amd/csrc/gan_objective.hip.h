// The adversarial objective of the discriminator's head, one frame at a time: the row's pre-activation z goes in, what the row adds
// to the step's loss sums and the seed dz of its backward pass come out.  Called by d_head_kernel (frame_kernels.hip.h) and by
// dstack_kernel (dstack_f32.hip.h) in place of lines of their own, so the two cannot drift apart.  The objective is a template
// parameter of both kernels: nothing is decided per row.
//
//   id  name    D(x)        real row                  generated row, D step     generated row, G step    "correct" threshold
//   0   bce     sigmoid(z)  -log(D + eps)             -log(1 - D + eps)         -log(D + eps)            0.5     (train.py:261-271, 307-308)
//   1   ls      z           0.5 (z - 1)^2             0.5 z^2                   0.5 (z - 1)^2            0.5
//   2   hinge   z           max(0, 1 - z)             max(0, 1 + z)             -z                       0
//   3   wgan    z           -z                        z                         -z                       0
//   4   kl      z           -z                        exp(z - 1)                -z                       1       (on z)
//   5   rkl     z           exp(-z)                   z - 1                     exp(-z)                  0
//   6   js      z           sp(-z) - ln 2             sp(z) - ln 2              sp(-z) - ln 2            0
//
// Ids 4 .. 6 are the f-GAN divergences (Nowozin et al. 2016): the D loss is the negative of the variational bound
// E_real g_f(v) - E_fake f*(g_f(v)) with the paper's output activations g_f and conjugates f*, a real row adding -g_f(z) and a generated
// row f*(g_f(z)); the G step is the non-saturating form (generated rows scored as real ones, as id 0's -log D); the threshold is
// g_f(z) > f'(1).  sp(x) = max(x, 0) + log(1 + exp(-|x|)), the overflow-safe softplus; js is the logistic loss minus 2 ln 2 without
// the eps.  eps is not read by ids 1 .. 6.
//
// Whatever the objective, the row's addend is -phi * m in float32 (m: the frame's mask value), summed in double by the caller, and the
// loss is -sum / Tv: the partials, both finalising launches, the riders and the results channel do not know which objective ran.
// Seeds of ids 1 .. 6 with u = m * inv_tv formed once; the hinge's derivative at a kink is 0, as torch's relu.
//
// The float32 sequences of ids 4 .. 6, operation by operation (expf and logf are the only math functions, as in id 0):
//   kl   real / G   phi = -z;  dz = -u                                                      exact given z and u
//        generated  t = z - 1;  e = expf(t);  phi = e;  dz = e * u                            phi: 1 rounding + expf;  dz: one more
//   rkl  real / G   e = expf(-z);  phi = e;  dz = -(e * u)                                    phi: expf;  dz: one more
//        generated  phi = z - 1;  dz = u                                                     phi: 1 rounding
//   js   x = -z (real / G) or z (generated);  a = |z|;  l = logf(1 + expf(-a));  r = max(x, 0);
//        phi = (r + l) - ln2f;  dz = -+u / (1 + expf(-x))                                    phi: expf, logf, 3 roundings;  dz: expf, 2 roundings
// js is 0 at z = 0 by cancellation (sp(0) = ln 2): its error is absolute, on the magnitudes of r, l and ln 2, not relative to phi.
// expf(-x) = inf gives 1 + inf = inf and u / inf = 0: the seed of a saturated js row is 0, never a NaN.
// exp(z - 1) and exp(-z) are unbounded and NOT clamped (a clamp would change the divergence): a row with z - 1 > 88.7 (kl) or z < -88.7
// (rkl) has an infinite loss term and seed (with m = 0 the addend is inf * 0, a NaN), and that non-finite gradient goes where any other
// does: the step's gradient norm is not finite and the clipped update stores NaN, as torch's clip_grad_norm_ and step would.  The engine's
// fault word is raised by device time-outs, not by values.
#pragma once
#include <hip/hip_runtime.h>

namespace gt {

enum GanObjective { GAN_OBJ_BCE = 0, GAN_OBJ_LS = 1, GAN_OBJ_HINGE = 2, GAN_OBJ_WGAN = 3, GAN_OBJ_KL = 4, GAN_OBJ_RKL = 5, GAN_OBJ_JS = 6, GAN_OBJ_COUNT = 7 };

struct GanRow {
  float D;                       // what the discriminator returns for the frame
  float addend;                  // -phi * m: goes to s_real (real and G-step rows) or s_fake (generated rows of the D step)
  float dz;                      // dloss / dz (0 without want_grad)
  double n_real_ok, n_fake_ok;   // the frame's terms of real_correct_count / fake_correct_count
};

// is_real: the row is scored against the "natural" label (a natural row of the D step, or any row of the G step's adversarial term)
template <int OBJ>
__device__ __forceinline__ GanRow gan_objective_row(float z, float m, bool is_real, bool g_mode, float eps, float inv_tv, bool want_grad) {
  static_assert(OBJ >= 0 && OBJ < GAN_OBJ_COUNT, "gan objective id");
  GanRow o;
  o.n_real_ok = 0.0; o.n_fake_ok = 0.0;
  if constexpr (OBJ == GAN_OBJ_BCE) {
    const float D = 1.f / (1.f + expf(-z));
    float dD;
    if (is_real) {
      o.addend = logf(D + eps) * m;
      if (!g_mode) o.n_real_ok = (D > 0.5f ? 1.0 : 0.0) * (double)m;
      dD = -m * inv_tv / (D + eps);
    } else {
      const float om = (1.f - D) + eps;
      o.addend = logf(om) * m;
      o.n_fake_ok = (D < 0.5f ? 1.0 : 0.0) * (double)m;
      dD = m * inv_tv / om;
    }
    o.D = D;
    o.dz = want_grad ? dD * ((1.f - D) * D) : 0.f;
  } else if constexpr (OBJ >= GAN_OBJ_KL) {
    constexpr float thr = OBJ == GAN_OBJ_KL ? 1.f : 0.f;
    const float u = m * inv_tv;
    float phi, dz;
    if (is_real) {
      if (!g_mode) o.n_real_ok = (z > thr ? 1.0 : 0.0) * (double)m;
    } else {
      o.n_fake_ok = (z < thr ? 1.0 : 0.0) * (double)m;
    }
    if (OBJ == GAN_OBJ_JS) {
      const float x = is_real ? -z : z;
      const float l = logf(1.f + expf(-fabsf(z)));
      const float r = x < 0.f ? 0.f : x;        // (a NaN stays a NaN)
      phi = (r + l) - 0.69314718f;              // ln2f, the float32 nearest to ln 2
      const float s = u / (1.f + expf(-x));
      dz = is_real ? -s : s;
    } else if (is_real == (OBJ == GAN_OBJ_KL)) {  // kl's real and G rows, rkl's generated rows: linear in z
      phi = OBJ == GAN_OBJ_KL ? -z : z - 1.f;
      dz = OBJ == GAN_OBJ_KL ? -u : u;
    } else {                                    // kl's generated rows: exp(z - 1); rkl's real and G rows: exp(-z)
      const float e = expf(OBJ == GAN_OBJ_KL ? z - 1.f : -z);
      phi = e;
      dz = OBJ == GAN_OBJ_KL ? e * u : -(e * u);
    }
    o.D = z;
    o.addend = -phi * m;
    o.dz = want_grad ? dz : 0.f;
  } else {
    constexpr float thr = OBJ == GAN_OBJ_LS ? 0.5f : 0.f;
    const float u = m * inv_tv;
    float phi, dz;
    if (is_real) {
      if (!g_mode) o.n_real_ok = (z > thr ? 1.0 : 0.0) * (double)m;
      if (OBJ == GAN_OBJ_LS) {
        const float d = z - 1.f;
        phi = 0.5f * (d * d);
        dz = d * u;
      } else if (OBJ == GAN_OBJ_HINGE && !g_mode) {
        const float t = 1.f - z;
        phi = t < 0.f ? 0.f : t;              // (a NaN stays a NaN)
        dz = z < 1.f ? -u : 0.f;
      } else {                                // hinge's G step, wgan
        phi = -z;
        dz = -u;
      }
    } else {
      o.n_fake_ok = (z < thr ? 1.0 : 0.0) * (double)m;
      if (OBJ == GAN_OBJ_LS) {
        phi = 0.5f * (z * z);
        dz = z * u;
      } else if (OBJ == GAN_OBJ_HINGE) {
        const float t = 1.f + z;
        phi = t < 0.f ? 0.f : t;
        dz = z > -1.f ? u : 0.f;
      } else {
        phi = z;
        dz = u;
      }
    }
    o.D = z;
    o.addend = -phi * m;
    o.dz = want_grad ? dz : 0.f;
  }
  return o;
}

}  // namespace gt
