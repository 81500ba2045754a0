// The MLPG band built on the device from the window set, without a dense R (gfx950).
//
// R = (W^T W)^-1 W^T with W the stacked window operators, (W_w x)[t] = sum_{k=-l_w..u_w} coef_w[k + l_w] x[t + k] (terms outside
// [0, T) dropped: gantts_amd/paramgen.py).  The step kernels read band[t][w][j] = R[t][w*T + t + j - kb]; this file produces those taps
// in O(T (K + hb)) memory and work:
//   (a) P = W^T W, banded with half-bandwidth hb = max_w (l_w + u_w), float64, column-major lower band  Lb[j][k] = P[j + k][j]
//   (b) banded Cholesky P = L L^T in place (Lb[j][k] = L[j + k][j]), left-looking, one column per step
//   (c) selected inversion (Takahashi): from L^T S = L^-1 (lower triangular, diagonal 1 / L[i][i]), for j > i
//           S[i][j] = - sum_{k=1..hb} (L[i+k][i] / L[i][i]) S[i+k][j]         S[i][i] = 1 / L[i][i]^2 - sum_k (L[i+k][i] / L[i][i]) S[i][i+k]
//       exact for every j, so the entries |i - j| <= KS of S = P^-1 come from rows below with offsets <= max(KS - 1, hb - 1):
//       rows from the last upwards, the off-diagonals of a row in parallel, then its diagonal.  Sb[i][d] = S[i][i + d].
//   (d) R[t][w*T + t'] = sum_k coef_w[k + l_w] S[t][t' + k] for |t - t'| <= K, rounded to float32: wide[t][w][t' - t + K], zero
//       where t' is outside [0, T); then the per-offset maxima ensure_band's half-width rule reads.
// K = min(MLPG_BUILD_K, T - 1) with MLPG_BUILD_K = 64, ONE more than the widest half-width ensure_band accepts: a tap above the
// threshold right outside that width is seen and refused as the dense path refuses it.  KS = min(max(K + max_w max(l_w, u_w), hb), T - 1).
//
// (a)-(c) run in ONE workgroup: the sequential loops are bounded by T, the threads meet at workgroup barriers only, and no workgroup
// waits for another one anywhere.  Plain sqrt and / on doubles (no fast-math in the Makefile).  A pivot that is not a finite positive
// number raises *flag and every thread leaves at once (the pivot is read from LDS: the same value in all of them).
#pragma once
#include "engine_internal.hip.h"      // MlpgWindows, MLPG_WIN_SPAN

constexpr int MLPG_BUILD_K = 64;          // candidate half-width
constexpr int MLPG_BUILD_THREADS = 128;   // >= KS = MLPG_BUILD_K + MLPG_WIN_SPAN at most, > MLPG_WIN_SPAN
static_assert(MLPG_BUILD_K + MLPG_WIN_SPAN <= MLPG_BUILD_THREADS && MLPG_WIN_SPAN < MLPG_BUILD_THREADS, "one thread per off-diagonal of a row");

// Lb [T][hb + 1], Sb [T][KS + 1]; grid 1, MLPG_BUILD_THREADS threads
static __global__ __launch_bounds__(MLPG_BUILD_THREADS) void mlpg_build_inverse_kernel(MlpgWindows win, int T, int hb, int KS,
                                                                                      double* Lb, double* Sb, int* flag) {
  __shared__ double sh_v[MLPG_WIN_SPAN + 1];
  const int tid = threadIdx.x, ldl = hb + 1, lds = KS + 1;
  if (tid == 0) *flag = 0;
  // (a) P[i][j] = sum_w sum_t coef_w[i - t + l_w] coef_w[j - t + l_w], t in [0, T) with both indices inside the window
  for (int idx = tid; idx < T * ldl; idx += MLPG_BUILD_THREADS) {
    const int j = idx / ldl, k = idx - j * ldl, i = j + k;
    double p = 0.0;
    if (i < T)
      for (int w = 0; w < win.n; ++w) {
        const int l = win.l[w], u = win.u[w];
        for (int t = max(0, i - u); t <= min(T - 1, j + l); ++t) p += win.coef[w][i - t + l] * win.coef[w][j - t + l];
      }
    Lb[idx] = p;
  }
  __syncthreads();
  // (b) column j: v_k = P[j+k][j] - sum_m L[j+k][m] L[j][m], m from max(0, j + k - hb) to j - 1; L[j][j] = sqrt(v_0), L[j+k][j] = v_k / L[j][j]
  const bool col = tid <= hb;
  for (int j = 0; j < T; ++j) {
    const bool mine = col && j + tid < T;
    if (mine) {
      double v = Lb[j * ldl + tid];
      for (int m = max(0, j + tid - hb); m < j; ++m) v -= Lb[m * ldl + (j + tid - m)] * Lb[m * ldl + (j - m)];
      sh_v[tid] = v;
    }
    __syncthreads();
    const double piv = sh_v[0];
    if (!(piv > 0.0) || !isfinite(piv)) {      // the same in every thread
      if (tid == 0) *flag = 1;
      return;
    }
    const double d = sqrt(piv);
    if (mine) Lb[j * ldl + tid] = tid == 0 ? d : sh_v[tid] / d;
    __syncthreads();
  }
  // (c) row i, thread tid owns the off-diagonal d = tid + 1; S[r][c] is Sb[min][|r - c|]
  for (int i = T - 1; i >= 0; --i) {
    const double lii = Lb[i * ldl];
    const int d = tid + 1, c = i + d;
    if (d <= KS && c < T) {
      double s = 0.0;
      for (int k = 1; k <= hb && i + k < T; ++k) {
        const int r = i + k;
        const double srv = c >= r ? Sb[r * lds + (c - r)] : Sb[c * lds + (r - c)];
        s -= (Lb[i * ldl + k] / lii) * srv;
      }
      Sb[i * lds + d] = s;
    }
    __syncthreads();
    if (tid == 0) {
      double s = 1.0 / (lii * lii);
      for (int k = 1; k <= hb && i + k < T; ++k) s -= (Lb[i * ldl + k] / lii) * Sb[i * lds + k];
      Sb[i * lds] = s;
    }
    __syncthreads();
  }
}

// (d) wide[t][w][o + K] = float32(R[t][w*T + t + o]), |o| <= K
static __global__ void mlpg_build_taps_kernel(MlpgWindows win, int T, int K, int KS, const double* __restrict__ Sb,
                                              const int* __restrict__ flag, float* __restrict__ wide) {
  const int nk = 2 * K + 1, lds = KS + 1;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long)T * win.n * nk || *flag) return;
  const int o = (int)(idx % nk) - K, w = (int)((idx / nk) % win.n), t = (int)(idx / ((long)nk * win.n));
  const int tp = t + o;
  double r = 0.0;
  if (tp >= 0 && tp < T) {
    const int l = win.l[w], u = win.u[w];
    for (int k = max(-l, -tp); k <= min(u, T - 1 - tp); ++k) {
      const int c = tp + k;
      const double s = c >= t ? Sb[(long)t * lds + (c - t)] : Sb[(long)c * lds + (t - c)];
      r += win.coef[w][k + l] * s;
    }
  }
  wide[idx] = (float)r;
}

// per-offset max |wide[t][w][o + K]| -> offmax[o + K]; NaN if any of them is (grid 2 K + 1)
static __global__ void mlpg_build_offset_max_kernel(const float* __restrict__ wide, int T, int nW, int K, float* __restrict__ offmax) {
  const int nk = 2 * K + 1;
  __shared__ float sh[16];
  float mx = 0.f;
  for (long i = threadIdx.x; i < (long)T * nW; i += blockDim.x) mx = max_or_nan(mx, fabsf(wide[i * nk + blockIdx.x]));
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mx = max_or_nan(mx, __shfl_xor(mx, s, 64));
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sh[wv] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) mx = max_or_nan(mx, sh[i]);
    offmax[blockIdx.x] = mx;
  }
}

// band[t][w][j] = wide[t][w][K + j - kb]: the image mlpg_extract_band_kernel makes from a dense R
static __global__ void mlpg_build_band_kernel(const float* __restrict__ wide, int T, int nW, int K, int kb, float* __restrict__ band) {
  const int nb = 2 * kb + 1, nk = 2 * K + 1;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)T * nW * nb) return;
  const int j = (int)(i % nb);
  band[i] = wide[(i / nb) * nk + K + j - kb];
}
