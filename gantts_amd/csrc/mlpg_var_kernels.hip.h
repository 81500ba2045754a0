// Variance-weighted MLPG (nnmnkwii.paramgen.mlpg) as a batch of independent banded solves (gfx950).
//
// For every (sequence b, static column c) with windows (W_w x)[t] = sum_k coef_w[k + l_w] x[t + k] (terms outside [0, len_b) dropped, as
// in gantts_amd/paramgen.py), precisions p_w[t] = 1 / var[t][scol[c] + w sstride[c]] and means mu_w[t] = y[t][scol[c] + w sstride[c]]:
//       P x = b,     P[i][j] = sum_w sum_t p_w[t] coef_w[i - t + l_w] coef_w[j - t + l_w],     b[i] = sum_w sum_t coef_w[i - t + l_w] p_w[t] mu_w[t]
// P is symmetric positive definite with half-bandwidth hb = max_w (l_w + u_w).  With variances it differs per column, so there is nothing to
// cache: ONE THREAD solves one column, sequentially over the sequence's OWN length n = len_b (its edge rows are those of an utterance
// evaluated alone), in float64 throughout:
//   forward   column j of the Cholesky factor  v_k = P[j+k][j] - sum_m L[j+k][m] L[j][m],  L[j][j] = sqrt(v_0),  L[j+k][j] = v_k / L[j][j],
//             with the forward substitution riding along:  z[j] = (b[j] - sum_m L[j][m] z[m]) / L[j][j]
//   backward  x[j] = (z[j] - sum_k L[j+k][j] x[j+k]) / L[j][j] from the last row upwards, rounded to float32 once
// L and z go to a float64 scratch  ws[(t (hb + 2) + k) ncols + column], k <= hb the factor's column t, k = hb + 1 z[t]: column fastest, so the
// 64 threads of a workgroup (c fastest) read and write whole lines, as they do in y, var and ys.
//
// No barrier, no LDS, no thread waits for another thread or workgroup; every loop is bounded by the thread's own n <= T.  Rows t >= n of
// the output are written as 0; a pass-through column (sstride == 0) is copied for t < n.  A variance or a pivot that is not a finite
// positive number ORs a bit into *flag (an ordinary vector atomic) and the thread abandons its own column: the launcher reads the flag.
// Plain sqrt and / on doubles (no fast-math in the Makefile).
//
// Two forms:
//   mlpg_var_solve_kernel<HB>  HB = 1, 2 (the reference's windows: 2).  Frame-major assembly: at column j window w takes in ITS frame
//       t = j + l_w, which touches the columns j .. j + l_w + u_w of P and b -- slots 0 .. HB of a sliding register window, whatever l_w is,
//       and column j is complete when it is consumed.  The windows' taps are zero-padded to HB + 1 on the host (MlpgVarTaps) and come from
//       the kernel arguments; with the last HB columns of L in registers every index is a compile-time constant.
//   mlpg_var_generic_kernel    0 <= hb <= MLPG_WIN_SPAN: column-major assembly straight from the formulas above, earlier columns of L
//       re-read from the scratch.
#pragma once
#include "engine_internal.hip.h"      // MlpgWindows, MLPG_WIN_SPAN, MLPG_MAXW

constexpr int MLPG_VAR_THREADS = 64;
constexpr int MLPG_VAR_BAD_VARIANCE = 1, MLPG_VAR_BAD_PIVOT = 2;      // bits of *flag

struct MlpgVarArgs {
  const float* y; const float* var; float* ys;      // y [nseq*T][ldy]; var [nseq*T][ldv], or one row when ldv == 0; ys [nseq*T][ldys]
  const int* scol; const int* sstride; const int* len;      // device: [Ds], [Ds], [nseq]
  double* ws; int* flag;
  int nseq, T, Ds, ldy, ldv, ldys;
};
// window w zero-padded to HB + 1 taps: c[w][s] = coef_w[s] for s <= l_w + u_w, else 0
template <int HB> struct MlpgVarTaps { int n; int l[MLPG_MAXW]; int pad_[3]; double c[MLPG_MAXW][HB + 1]; };

static __device__ __forceinline__ bool mlpg_var_positive(double v) { return v > 0.0 && isfinite(v); }

// the rows the solve does not reach, and the pass-through columns
static __device__ __forceinline__ void mlpg_var_zero_tail(const MlpgVarArgs& a, long row0, int n, int c) {
  for (int t = n; t < a.T; ++t) a.ys[(row0 + t) * a.ldys + c] = 0.f;
}
static __device__ __forceinline__ void mlpg_var_copy(const MlpgVarArgs& a, long row0, int n, int c, int col) {
  for (int t = 0; t < n; ++t) a.ys[(row0 + t) * a.ldys + c] = a.y[(row0 + t) * a.ldy + col];
  mlpg_var_zero_tail(a, row0, n, c);
}
// x from L and z in the scratch, last row upwards; L[j+k][j] is 0 for j + k >= n
template <int HB> static __device__ __forceinline__ void mlpg_var_back_regs(const MlpgVarArgs& a, long row0, int n, int c, const double* ws, long ncols) {
  double xs[HB > 0 ? HB : 1] = {};      // x[j+1 .. j+HB]
  for (int j = n - 1; j >= 0; --j) {
    const double* q = ws + (long)j * (HB + 2) * ncols;
    double s = q[(HB + 1) * ncols];
#pragma unroll
    for (int k = 1; k <= HB; ++k) s -= q[k * ncols] * xs[k - 1];
    const double x = s / q[0];
#pragma unroll
    for (int k = HB - 1; k >= 1; --k) xs[k] = xs[k - 1];
    if (HB > 0) xs[0] = x;
    a.ys[(row0 + j) * a.ldys + c] = (float)x;
  }
}

// grid cdiv(nseq * Ds, 64), 64 threads
template <int HB>
static __global__ __launch_bounds__(MLPG_VAR_THREADS) void mlpg_var_solve_kernel(MlpgVarArgs a, MlpgVarTaps<HB> taps) {
  constexpr int S = HB + 1;
  const long g = (long)blockIdx.x * MLPG_VAR_THREADS + threadIdx.x, ncols = (long)a.nseq * a.Ds;
  if (g >= ncols) return;
  const int b = (int)(g / a.Ds), c = (int)(g - (long)b * a.Ds);
  const int n = a.len[b], col = a.scol[c], st = a.sstride[c];
  const long row0 = (long)b * a.T;
  if (st == 0) { mlpg_var_copy(a, row0, n, c, col); return; }
  double* ws = a.ws + g;
  double accP[S][HB + 1] = {}, accB[S] = {};      // slot d: column j + d of P (rows j + d + k) and of b
  double Lp[HB][HB + 1] = {}, zp[HB] = {};         // Lp[m-1][k] = L[j-m+k][j-m], zp[m-1] = z[j-m]; zero before the first column
  // the taps live in vector registers across the loop (an empty asm pins them there): 8 (HB + 1) scalar registers beside the arguments
  // exceed the scalar file, and the loop's fma take one scalar operand each anyway
  double tc[MLPG_MAXW][S];
#pragma unroll
  for (int w = 0; w < MLPG_MAXW; ++w)
#pragma unroll
    for (int s = 0; s < S; ++s) { tc[w][s] = taps.c[w][s]; asm volatile("" : "+v"(tc[w][s])); }
  for (int j = -HB; j < n; ++j) {                  // l_w <= HB: frame 0 of window w enters at j = -l_w, into columns that are shifted out before j = 0
#pragma unroll
    for (int w = 0; w < MLPG_MAXW; ++w) {
      const int t = j + taps.l[w];      // this window's frame: columns t - l_w .. t + u_w are slots 0 .. l_w + u_w
      if (w < taps.n && t >= 0 && t < n) {
        const double v = (double)a.var[(a.ldv ? (row0 + t) * a.ldv : 0L) + col + (long)w * st];
        if (!mlpg_var_positive(v)) { atomicOr(a.flag, MLPG_VAR_BAD_VARIANCE); return; }
        const double p = 1.0 / v, pm = p * (double)a.y[(row0 + t) * a.ldy + col + (long)w * st];
#pragma unroll
        for (int s = 0; s < S; ++s) {
          const double pc = p * tc[w][s];
#pragma unroll
          for (int k = 0; k <= HB; ++k)
            if (s + k < S) accP[s][k] += pc * tc[w][s + k];
          accB[s] += tc[w][s] * pm;
        }
      }
    }
    if (j >= 0) {
      double v[HB + 1];
#pragma unroll
      for (int k = 0; k <= HB; ++k) {
        double s = accP[0][k];
#pragma unroll
        for (int m = 1; m + k <= HB; ++m) s -= Lp[m - 1][m + k] * Lp[m - 1][m];
        v[k] = (k == 0 || j + k < n) ? s : 0.0;
      }
      if (!mlpg_var_positive(v[0])) { atomicOr(a.flag, MLPG_VAR_BAD_PIVOT); return; }
      const double d = sqrt(v[0]);
      double zz = accB[0];
#pragma unroll
      for (int m = 1; m <= HB; ++m) zz -= Lp[m - 1][m] * zp[m - 1];
      zz = zz / d;
      v[0] = d;
#pragma unroll
      for (int k = 1; k <= HB; ++k) v[k] = v[k] / d;
      double* q = ws + (long)j * (HB + 2) * ncols;
#pragma unroll
      for (int k = 0; k <= HB; ++k) q[k * ncols] = v[k];
      q[(HB + 1) * ncols] = zz;
#pragma unroll
      for (int m = HB - 1; m >= 1; --m) {
#pragma unroll
        for (int k = 0; k <= HB; ++k) Lp[m][k] = Lp[m - 1][k];
        zp[m] = zp[m - 1];
      }
#pragma unroll
      for (int k = 0; k <= HB; ++k) Lp[0][k] = v[k];
      zp[0] = zz;
    }
#pragma unroll
    for (int s = 0; s + 1 < S; ++s) {
#pragma unroll
      for (int k = 0; k <= HB; ++k) accP[s][k] = accP[s + 1][k];
      accB[s] = accB[s + 1];
    }
#pragma unroll
    for (int k = 0; k <= HB; ++k) accP[S - 1][k] = 0.0;
    accB[S - 1] = 0.0;
  }
  mlpg_var_back_regs<HB>(a, row0, n, c, ws, ncols);
  mlpg_var_zero_tail(a, row0, n, c);
}

// grid cdiv(nseq * Ds, 64), 64 threads; hb = max_w (l_w + u_w) of win
static __global__ __launch_bounds__(MLPG_VAR_THREADS) void mlpg_var_generic_kernel(MlpgVarArgs a, MlpgWindows win, int hb) {
  const long g = (long)blockIdx.x * MLPG_VAR_THREADS + threadIdx.x, ncols = (long)a.nseq * a.Ds;
  if (g >= ncols) return;
  const int b = (int)(g / a.Ds), c = (int)(g - (long)b * a.Ds);
  const int n = a.len[b], col = a.scol[c], st = a.sstride[c];
  const long row0 = (long)b * a.T;
  if (st == 0) { mlpg_var_copy(a, row0, n, c, col); return; }
  double* ws = a.ws + g;
  const long ldw = (long)(hb + 2) * ncols;      // scratch of one frame
  const long vstep = a.ldv ? a.ldv : 0L;         // one row: every frame reads the same variances
  const float* vcol = a.var + (a.ldv ? row0 * a.ldv : 0L) + col;
  const float* ycol = a.y + row0 * a.ldy + col;
  for (int w = 0; w < win.n; ++w)
    for (int t = 0; t < (a.ldv ? n : 1); ++t)
      if (!mlpg_var_positive((double)vcol[t * vstep + (long)w * st])) { atomicOr(a.flag, MLPG_VAR_BAD_VARIANCE); return; }
  for (int j = 0; j < n; ++j) {
    double d = 0.0;
    for (int k = 0; k <= hb && j + k < n; ++k) {
      const int i = j + k;
      double v = 0.0;
      for (int w = 0; w < win.n; ++w) {
        const int l = win.l[w], u = win.u[w];
        for (int t = max(0, i - u); t <= min(n - 1, j + l); ++t)
          v += (1.0 / (double)vcol[t * vstep + (long)w * st]) * win.coef[w][i - t + l] * win.coef[w][j - t + l];
      }
      for (int m = max(0, i - hb); m < j; ++m) v -= ws[m * ldw + (i - m) * ncols] * ws[m * ldw + (j - m) * ncols];
      if (k == 0) {
        if (!mlpg_var_positive(v)) { atomicOr(a.flag, MLPG_VAR_BAD_PIVOT); return; }
        d = sqrt(v);
        ws[j * ldw] = d;
      } else {
        ws[j * ldw + k * ncols] = v / d;
      }
    }
    for (int k = max(1, n - j); k <= hb; ++k) ws[j * ldw + k * ncols] = 0.0;      // rows beyond the sequence
    double z = 0.0;
    for (int w = 0; w < win.n; ++w) {
      const int l = win.l[w], u = win.u[w];
      for (int t = max(0, j - u); t <= min(n - 1, j + l); ++t)
        z += win.coef[w][j - t + l] * ((1.0 / (double)vcol[t * vstep + (long)w * st]) * (double)ycol[(long)t * a.ldy + (long)w * st]);
    }
    for (int m = max(0, j - hb); m < j; ++m) z -= ws[m * ldw + (j - m) * ncols] * ws[m * ldw + (hb + 1) * ncols];
    ws[j * ldw + (hb + 1) * ncols] = z / d;
  }
  for (int j = n - 1; j >= 0; --j) {      // x[j] takes z[j]'s place in the scratch: the rows above read it in float64
    double s = ws[j * ldw + (hb + 1) * ncols];
    for (int k = 1; k <= hb && j + k < n; ++k) s -= ws[j * ldw + k * ncols] * ws[(j + k) * ldw + (hb + 1) * ncols];
    const double x = s / ws[j * ldw];
    ws[j * ldw + (hb + 1) * ncols] = x;
    a.ys[(row0 + j) * a.ldys + c] = (float)x;
  }
  mlpg_var_zero_tail(a, row0, n, c);
}
