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
//
// Whatever the objective, the row's addend is -phi * m in float32 (m: the frame's mask value), summed in double by the caller, and the
// loss is -sum / Tv: the partials, both finalising launches, the riders and the results channel do not know which objective ran.
// Seeds of ids 1 .. 3 with u = m * inv_tv formed once; the hinge's derivative at a kink is 0, as torch's relu.
#pragma once
#include <hip/hip_runtime.h>

namespace gt {

enum GanObjective { GAN_OBJ_BCE = 0, GAN_OBJ_LS = 1, GAN_OBJ_HINGE = 2, GAN_OBJ_WGAN = 3, GAN_OBJ_COUNT = 4 };

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
