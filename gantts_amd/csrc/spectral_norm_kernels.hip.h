// Spectral normalisation of the MLP discriminator's weights (gfx950): one power iteration per discriminator pass (sn_prepare: three
// launches for the whole network) and the gradient's projection onto the caller's weights (sn_project: two launches), each driven by
// ONE job table over the flat parameter buffer.  Included by eng_spectral_norm.hip alone.
//
// Per nn.Linear weight W (out, in), with the persistent unit vectors u (out), v (in) and eps = 1e-12:
//   iterate   t = W^T u;  v' = t / max(|t|, eps);  r = W v';  u' = r / max(|r|, eps);  sigma = u'^T r;  W_eff = W / sigma;  u <- u', v <- v'
//   eval      r = W v;  sigma = u^T r;  W_eff = W / sigma                      (nothing stored but W_eff and sigma)
//   project   s = sum G (.) W_eff;  G <- (G - s u' v'^T) / sigma                (G = d loss / d W_eff, in place)
//
// Arithmetic (restated by tests/spectral_norm_ref.py).  A product of two float32 values is formed in double, where it is exact.  Every sum is
// a two-stage double sum in an order fixed by the job table: lanes or waves first, then a fixed combine; no atomics.  t, r and the
// norms stay double; u', v' and sigma are rounded to float32 once.  W / sigma is the correctly rounded float32 quotient, and the
// projected element is ((G - (float(s) * u'_i) * v'_j) / sigma) in float32 with contraction off.
//
// No workgroup waits for another: every workgroup that needs a normalised vector (at most SN_MAX_DIM entries) or sigma re-derives it from
// the double sums of the previous launch, with the same code on the same values, hence the same bits.
//
// Alignment.  Weight ranges start wherever the biases before them end, so only 4-byte alignment holds.  The products walk a row (or a
// column block) with one float per lane: coalesced at any alignment.  The element passes walk the flat buffer in windows of SN_CHUNK
// floats that start on a multiple of 4 floats; a quad that lies wholly inside the weight range moves as 16 bytes (when both buffers
// are 16-byte aligned: SnJobs::vec), the head and tail quads of a range go element by element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "frame_kernels.hip.h"

namespace gt {

constexpr int SN_MAX_JOBS = 17;        // an MLP's hidden layers (gt_bind_model: at most 16) + last_linear
constexpr int SN_MAX_DIM = 512;        // out and in of a normalised layer: the vectors every workgroup re-normalises for itself
constexpr int SN_CHUNK = 4096;         // floats of the flat buffer per workgroup of an element pass (256 threads x 4 quads)
constexpr int SN_THREADS = 256;
constexpr double SN_EPS = 1e-12;       // torch.nn.utils.spectral_norm's eps

struct SnJob {
  long w_off;                  // first weight element in the flat buffer
  int out, in, u_off, v_off;   // u_off also indexes r, v_off also indexes t
  int cb0, rb0, eb0, nb;       // first workgroup of the job in the W^T u launch / the W v launch / an element pass; its element-pass workgroups
};
struct SnJobs { int n, vec; SnJob j[SN_MAX_JOBS]; };
struct SnRest { long off[SN_MAX_JOBS + 1]; long n[SN_MAX_JOBS + 1]; int n_rest, pad_; };      // what no job covers (biases): squared for the norm only

// the sum over the workgroup (SN_THREADS threads), the same bits in every thread
__device__ __forceinline__ double sn_block_total(double v, double* sh) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// |x| of a double vector of n <= SN_MAX_DIM entries, clamped from below as torch's normalize does
__device__ __forceinline__ double sn_norm(const double* __restrict__ x, int n, double* sh) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += SN_THREADS) acc += x[i] * x[i];
  const double nrm = sqrt(sn_block_total(acc, sh));
  return nrm > SN_EPS ? nrm : SN_EPS;
}
__device__ __forceinline__ int sn_job_of(const SnJobs& jobs, int blk, int which) {
  int q = 0;
  while (q + 1 < jobs.n && blk >= (which == 0 ? jobs.j[q + 1].cb0 : which == 1 ? jobs.j[q + 1].rb0 : jobs.j[q + 1].eb0)) ++q;
  return q;
}

// launch 1 (iterate only): t = W^T u.  One workgroup per 64 columns: lane <-> column, wave w sums rows w, w + 4, ..., then the four waves in order.
static __global__ __launch_bounds__(SN_THREADS) void sn_wtu_kernel(const SnJobs jobs, const float* __restrict__ W, const float* __restrict__ u,
                                                                   double* __restrict__ t) {
  __shared__ double sh[4][64];
  const SnJob J = jobs.j[sn_job_of(jobs, (int)blockIdx.x, 0)];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int c = ((int)blockIdx.x - J.cb0) * 64 + lane;
  double acc = 0.0;
  if (c < J.in) {
    const float* col = W + J.w_off + c;
    for (int i = w; i < J.out; i += 4) acc += (double)col[(long)i * J.in] * (double)u[J.u_off + i];
  }
  sh[w][lane] = acc;
  __syncthreads();
  if (w == 0 && c < J.in) t[J.v_off + c] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

// launch 2: r = W v' (iterate: v' from t, re-normalised here) or W v (eval: the stored v).  One wave per row, lanes stride the row.
static __global__ __launch_bounds__(SN_THREADS) void sn_wv_kernel(const SnJobs jobs, const float* __restrict__ W, const double* __restrict__ t,
                                                                  const float* __restrict__ v, double* __restrict__ r, const int iterate) {
  __shared__ double sh[4];
  __shared__ float vs[SN_MAX_DIM];
  const SnJob J = jobs.j[sn_job_of(jobs, (int)blockIdx.x, 1)];
  if (iterate) {
    const double nrm = sn_norm(t + J.v_off, J.in, sh);
    for (int j = threadIdx.x; j < J.in; j += SN_THREADS) vs[j] = (float)(t[J.v_off + j] / nrm);
  } else {
    for (int j = threadIdx.x; j < J.in; j += SN_THREADS) vs[j] = v[J.v_off + j];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int i = ((int)blockIdx.x - J.rb0) * 4 + (int)(threadIdx.x >> 6);
  if (i >= J.out) return;      // (whole waves; no barrier follows)
  const float* row = W + J.w_off + (long)i * J.in;
  double acc = 0.0;
  for (int j = lane; j < J.in; j += 64) acc += (double)row[j] * (double)vs[j];
  acc = wave_sum_d(acc);
  if (lane == 0) r[J.u_off + i] = acc;
}

__device__ __forceinline__ float sn_div(float a, float b) { return __fdiv_rn(a, b); }
__device__ __forceinline__ float sn_project_elem(float g, float su, float vj, float sigma) {
#pragma clang fp contract(off)
  const float p = su * vj;
  const float d = g - p;
  return sn_div(d, sigma);
}

// the quads of this workgroup's window of job J: f(flat index of the quad, first and one-past-last valid lane of it, whole)
template <typename F>
__device__ __forceinline__ void sn_window(const SnJob& J, int chunk, bool vec, F f) {
  const long beg = J.w_off, end = J.w_off + (long)J.out * J.in;
  const long base = (beg & ~3L) + (long)chunk * SN_CHUNK;
#pragma unroll
  for (int m = 0; m < SN_CHUNK / (4 * SN_THREADS); ++m) {
    const long q = base + 4L * ((long)threadIdx.x + (long)m * SN_THREADS);
    if (q >= end || q + 4 <= beg) continue;
    const int c0 = q < beg ? (int)(beg - q) : 0, c1 = q + 4 > end ? (int)(end - q) : 4;
    f(q, c0, c1, vec && c0 == 0 && c1 == 4);
  }
}

// launch 3: u', sigma (iterate) or sigma = u^T r (eval) re-derived by every workgroup from r; W_eff = W / sigma over this workgroup's window;
// the first workgroup of a job stores u', v' (iterate) and sigma.
static __global__ __launch_bounds__(SN_THREADS) void sn_finish_kernel(const SnJobs jobs, const float* __restrict__ W, const double* __restrict__ t,
                                                                      const double* __restrict__ r, float* __restrict__ u, float* __restrict__ v,
                                                                      float* __restrict__ sigma, float* __restrict__ weff, const int iterate) {
  __shared__ double sh[4];
  const int q = sn_job_of(jobs, (int)blockIdx.x, 2);
  const SnJob J = jobs.j[q];
  const bool first = (int)blockIdx.x == J.eb0;
  const double nr = iterate ? sn_norm(r + J.u_off, J.out, sh) : 1.0;
  double acc = 0.0;
  for (int i = threadIdx.x; i < J.out; i += SN_THREADS) {
    const double ri = r[J.u_off + i];
    const float ui = iterate ? (float)(ri / nr) : u[J.u_off + i];
    acc += (double)ui * ri;
    if (iterate && first) u[J.u_off + i] = ui;      // (no workgroup reads u in this launch when it iterates)
  }
  const float sg = (float)sn_block_total(acc, sh);
  if (first) {
    if (threadIdx.x == 0) sigma[q] = sg;
    if (iterate) {
      const double nt = sn_norm(t + J.v_off, J.in, sh);
      for (int j = threadIdx.x; j < J.in; j += SN_THREADS) v[J.v_off + j] = (float)(t[J.v_off + j] / nt);
    }
  }
  sn_window(J, (int)blockIdx.x - J.eb0, jobs.vec != 0, [&](long e, int c0, int c1, bool whole) {
    if (whole) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(W + e);
      f32x4 y;
#pragma unroll
      for (int c = 0; c < 4; ++c) y[c] = sn_div(x[c], sg);
      *reinterpret_cast<f32x4*>(weff + e) = y;
    } else {
      for (int c = c0; c < c1; ++c) weff[e + c] = sn_div(W[e + c], sg);
    }
  });
}

// projection, launch 1: one double per workgroup, the sum of G (.) W_eff over its window
static __global__ __launch_bounds__(SN_THREADS) void sn_gw_partial_kernel(const SnJobs jobs, const float* __restrict__ G, const float* __restrict__ weff,
                                                                          double* __restrict__ sp) {
  __shared__ double sh[4];
  const SnJob J = jobs.j[sn_job_of(jobs, (int)blockIdx.x, 2)];
  double acc = 0.0;
  sn_window(J, (int)blockIdx.x - J.eb0, jobs.vec != 0, [&](long e, int c0, int c1, bool whole) {
    if (whole) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(G + e), w = *reinterpret_cast<const f32x4*>(weff + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) acc += (double)g[c] * (double)w[c];
    } else {
      for (int c = c0; c < c1; ++c) acc += (double)G[e + c] * (double)weff[e + c];
    }
  });
  const double tot = sn_block_total(acc, sh);
  if (threadIdx.x == 0) sp[blockIdx.x] = tot;
}

// projection, launch 2: s of the job (its partials in order), the element pass in place, and one squared-norm partial per workgroup of what it
// has just written -- or, for the trailing workgroups, of the ranges no job covers (the biases): the whole flat gradient, once.
static __global__ __launch_bounds__(SN_THREADS) void sn_project_kernel(const SnJobs jobs, const int n_job_blocks, const SnRest rest, float* __restrict__ G,
                                                                       const float* __restrict__ u, const float* __restrict__ v,
                                                                       const float* __restrict__ sigma, const double* __restrict__ sp,
                                                                       double* __restrict__ s_out, double* __restrict__ norm_part) {
  __shared__ double sh[4];
  double acc = 0.0;
  if ((int)blockIdx.x < n_job_blocks) {
    const int q = sn_job_of(jobs, (int)blockIdx.x, 2);
    const SnJob J = jobs.j[q];
    double s = 0.0;
    for (int k = 0; k < J.nb; ++k) s += sp[J.eb0 + k];
    if ((int)blockIdx.x == J.eb0 && threadIdx.x == 0) s_out[q] = s;
    const float sf = (float)s, sg = sigma[q];
    sn_window(J, (int)blockIdx.x - J.eb0, jobs.vec != 0, [&](long e, int c0, int c1, bool whole) {
      const long rel = e + c0 - J.w_off;
      int i = (int)(rel / J.in), j = (int)(rel - (long)i * J.in);
      float su = sf * u[J.u_off + i];
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (whole) g = *reinterpret_cast<const f32x4*>(G + e);
#pragma unroll
      for (int c = 0; c < 4; ++c) {      // (constant indices into g: registers, not scratch)
        if (c < c0 || c >= c1) continue;
        if (!whole) g[c] = G[e + c];
        g[c] = sn_project_elem(g[c], su, v[J.v_off + j], sg);
        acc += (double)g[c] * (double)g[c];
        if (!whole) G[e + c] = g[c];
        if (++j == J.in && c + 1 < c1) { j = 0; ++i; su = sf * u[J.u_off + i]; }
      }
      if (whole) *reinterpret_cast<f32x4*>(G + e) = g;
    });
  } else {
    const long nrb = (long)gridDim.x - n_job_blocks, rb = (long)blockIdx.x - n_job_blocks;
    for (int k = 0; k < rest.n_rest; ++k)
      for (long i = rb * SN_THREADS + threadIdx.x; i < rest.n[k]; i += nrb * SN_THREADS) {
        const double x = (double)G[rest.off[k] + i];
        acc += x * x;
      }
  }
  const double tot = sn_block_total(acc, sh);
  if (threadIdx.x == 0) norm_part[blockIdx.x] = tot;
}

}  // namespace gt
