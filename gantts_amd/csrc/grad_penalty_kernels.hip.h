// Gradient penalties of the MLP discriminator (R1, WGAN-GP) for gfx950: the small kernels between the products of the second-order pass.
// Included by eng_grad_penalty.hip alone (behind engine_internal.hip.h, which names the kinds: GpKind).  The products themselves are launches of the float32 family (backward-data, forward with
// ACT_NONE, weight gradient); what is left is per-element or per-row work:
//
//   gp_interp    x_hat[r][j] = eps_r real[r][idx[j]] + (1 - eps_r) fake[r][idx[j]]      (WGAN-GP; eps_r injected or one Philox draw per row)
//   gp_slope     Y[r][c] = X[r][c] s(r, c),  s = f'(h) x dropout factor of the layer that stored H, recovered as the backward-data epilogue
//                recovers it (leaky_drop_grad on the stored activation and the site's keep bit); X may be one row for all r (the seed w)
//   gp_row       per row: ss = sum g^2, n = sqrt(ss + 1e-12), phi and r (in place of g); per workgroup a double partial of mask phi and mask n
//   gp_finalize  the partials in a fixed order, times 1 / T, added into the running record {sum P, sum mean-norm, steps}
//   gp_add_cols  dW[:, col0 : col0 + n] += S      (a dense [out][n] product into a column slab of a pitched matrix, element stores)
//
// Every sum has a fixed order (lanes by the xor butterfly, waves in order, workgroups in order): no atomics, the same bits from run to run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frame_kernels.hip.h"

namespace gt {

constexpr int GP_THREADS = 256;
constexpr int GP_ROWS_PER_WG = 16;      // gp_row: four waves, four rows each
constexpr float GP_EPS = 1e-12f;        // under the square root of the norm

// eps of row r: the top 24 bits of word 0 of Philox4x32-10 at counter (r, 'GPEP'), in [0, 1) exactly
constexpr uint32_t GP_EPS_STREAM = 0x47504550u;
__device__ __forceinline__ float gp_eps_draw(uint32_t key0, uint32_t key1, uint32_t row) {
  uint32_t w[4];
  philox4x32_10(row, GP_EPS_STREAM, key0, key1, w);
  return (float)(w[0] >> 8) * 5.9604644775390625e-08f;      // 2^-24
}

// one thread per element of the [rows][na] image; eps_out (may be null): the draws, one per row
static __global__ __launch_bounds__(GP_THREADS) void gp_interp_kernel(const float* __restrict__ real, const float* __restrict__ fake, int ldf,
                                                                      const int* __restrict__ idx, int na, const float* __restrict__ eps_in,
                                                                      uint32_t key0, uint32_t key1, float* __restrict__ out, int ldo, int col0,
                                                                      long rows, float* __restrict__ eps_out) {
  const long e = (long)blockIdx.x * GP_THREADS + threadIdx.x;
  if (e >= rows * na) return;
  const long r = e / na;
  const int j = (int)(e - r * na);
  const float eps = eps_in ? eps_in[r] : gp_eps_draw(key0, key1, (uint32_t)r);
  const int c = idx ? idx[j] : j;
  const float a = real[r * ldf + c], b = fake[r * ldf + c];
  out[r * ldo + col0 + j] = __fadd_rn(__fmul_rn(eps, a), __fmul_rn(1.f - eps, b));
  if (eps_out && j == 0) eps_out[r] = eps;
}

// Y = X (.) s.  ldx == 0: X is one row [cols] (the head's weight: the seed of the gradient chain)
static __global__ __launch_bounds__(GP_THREADS) void gp_slope_kernel(const float* X, int ldx, const float* __restrict__ H, int ldh,
                                                                     const DropoutSpec d, float* Y, int ldy, long rows, int cols) {
  const long e = (long)blockIdx.x * GP_THREADS + threadIdx.x;
  if (e >= rows * cols) return;
  const long r = e / cols;
  const int c = (int)(e - r * cols);
  const float scale = d.mode == DROP_NONE ? 1.f : d.scale;
  const float s = leaky_drop_grad(H[r * ldh + c], dropout_keep(d, (int)r, c), scale);
  Y[r * ldy + c] = X[r * (long)ldx + c] * s;
}

struct GpRowArgs {
  float* g; int ld;            // [rows][ld]: the gradient w.r.t. the adversarial columns in, r out; pad columns [na, ld) are zeroed
  int na, kind;
  long rows;
  const float* mask;           // [rows]
  const float* inv_tv_dev;     // 1 / T on the device, or null: inv_tv
  float inv_tv, weight;
  float* phi; float* nrm;      // [rows] per-row phi and n (either may be null)
  double* part;                // [2][nblk]: mask phi, then mask n
  int nblk;
};
static __global__ __launch_bounds__(GP_THREADS) void gp_row_kernel(const GpRowArgs a) {
  __shared__ double sh[2][4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float inv_tv = a.inv_tv_dev ? *a.inv_tv_dev : a.inv_tv;
  double s_phi = 0.0, s_n = 0.0;
  for (int i = 0; i < GP_ROWS_PER_WG / 4; ++i) {
    const long r = (long)blockIdx.x * GP_ROWS_PER_WG + w * (GP_ROWS_PER_WG / 4) + i;      // wave-uniform
    if (r >= a.rows) break;
    float* row = a.g + r * a.ld;
    float ss = 0.f;
    for (int c = lane; c < a.na; c += 64) { const float v = row[c]; ss = fmaf(v, v, ss); }
    ss = wave_sum(ss);
    const float n = sqrtf(ss + GP_EPS);
    const float m = a.mask[r];
    float phi, k;
    if (a.kind == GP_R1) { phi = 0.5f * a.weight * ss; k = a.weight * (m * inv_tv); }
    else { const float d = n - 1.f; phi = a.weight * d * d; k = 2.f * a.weight * (m * inv_tv) * (1.f - 1.f / n); }
    for (int c = lane; c < a.ld; c += 64) row[c] = c < a.na ? k * row[c] : 0.f;
    if (lane == 0) {
      if (a.phi) a.phi[r] = phi;
      if (a.nrm) a.nrm[r] = n;
    }
    s_phi += (double)m * (double)phi;
    s_n += (double)m * (double)n;
  }
  if (lane == 0) { sh[0][w] = s_phi; sh[1][w] = s_n; }
  __syncthreads();
  if (threadIdx.x == 0) {
    a.part[blockIdx.x] = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    a.part[a.nblk + blockIdx.x] = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
  }
}

// one workgroup: thread t sums partials t, t + 256, ... in order, then block_sum_d's fixed combine.  sums (may be null): this call's
// {sum mask phi, sum mask n} before the 1 / T; rec (may be null): {sum P, sum mean-norm, steps} += {sum phi / T, sum n / T, 1}
static __global__ __launch_bounds__(GP_THREADS) void gp_finalize_kernel(const double* __restrict__ part, int nblk, const float* __restrict__ inv_tv_dev,
                                                                        float inv_tv, double* __restrict__ sums, double* __restrict__ rec) {
  __shared__ double sh[4];
  double p = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < nblk; i += GP_THREADS) { p += part[i]; q += part[nblk + i]; }
  const double P = block_sum_d(p, sh);
  const double Q = block_sum_d(q, sh);
  if (threadIdx.x == 0) {
    const double it = (double)(inv_tv_dev ? *inv_tv_dev : inv_tv);
    if (sums) { sums[0] = P; sums[1] = Q; }
    if (rec) { rec[0] += P * it; rec[1] += Q * it; rec[2] += 1.0; }
  }
}

static __global__ __launch_bounds__(GP_THREADS) void gp_add_cols_kernel(const float* __restrict__ S, int n, float* __restrict__ dW, int ldw, int col0,
                                                                        int out) {
  const long e = (long)blockIdx.x * GP_THREADS + threadIdx.x;
  if (e >= (long)out * n) return;
  const int h = (int)(e / n), j = (int)(e - (long)h * n);
  float* p = dW + (long)h * ldw + col0 + j;
  *p = *p + S[e];
}

}  // namespace gt
