// Banded MLPG of the G+D step (gfx950): the band's extraction from a dense R, the forward kernel and its transpose.  eng_mlpg.hip alone includes it.
#pragma once
#include "engine_internal.hip.h"      // StepScalars; the MLPG_* constants (frame_kernels.hip.h)

namespace gt {
// ---------------------------------------------------------------------------------------
// MLPG.  The reference multiplies by a dense (T x nW*T) matrix R (nnmnkwii
// unit_variance_mlpg, call sites gantts/multistream.py:120, models.py:66).  R is numerically
// banded; the engine extracts band[t][w][j] = R[t][w*T + t + j - kb] from the caller's dense R
// and verifies that everything outside the band is negligible before using the O(T*kb) form.
// ---------------------------------------------------------------------------------------
// max that keeps a NaN once it has seen one (fmaxf returns the other operand): a NaN in R must reach ensure_band's finiteness check
__device__ __forceinline__ float max_or_nan(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
// per-offset max |R[t][w*T + t + o]| , o in [-(T-1), T-1]  ->  offmax[o + T - 1]; NaN if any of them is
static __global__ void mlpg_offset_max_kernel(const float* __restrict__ R, int T, int nW, float* __restrict__ offmax) {
  const int o = blockIdx.x - (T - 1);
  __shared__ float sh[16];
  float mx = 0.f;
  for (int i = threadIdx.x; i < T * nW; i += blockDim.x) {
    const int w = i / T, t = i - w * T;
    const int tt = t + o;
    if (tt >= 0 && tt < T) mx = max_or_nan(mx, fabsf(R[(long)t * nW * T + (long)w * T + tt]));
  }
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

static __global__ void mlpg_extract_band_kernel(const float* __restrict__ R, int T, int nW, int kb, float* __restrict__ band) {
  const int nb = 2 * kb + 1;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * nW * nb) return;
  const int j = i % nb, w = (i / nb) % nW, t = i / (nb * nW);
  const int tt = t + j - kb;
  band[i] = (tt >= 0 && tt < T) ? R[(long)t * nW * T + (long)w * T + tt] : 0.f;
}

// static-column map: for static column c, scol[c] = column of its static component in the full
// (static+delta) layout, sstride[c] = stream's static width (distance between window blocks),
// 0 for a stream without dynamic features (pass-through copy, bit-exact).

// y_static[b][t][c] = sum_w sum_j band[t][w][j] * y[b][t+j-kb][scol[c] + w*sstride[c]]
//
// Workgroup = (sequence b, MLPG_TT = 32 output frames, MLPG_CC = 64 static columns).  LDS holds the
// (T,D) tile with its +-kb halo, [(TT+2kb)][nW][CC], and the TT band rows, zero-padded by
// MLPG_PAD taps on both sides, [TT][nW][nb+2*PAD].  Each lane owns a 2-column x 4-frame register
// block: one ds_read_b64 of data feeds 8 FMAs, the 4 coefficients are wave-broadcast reads
// (0.6 LDS instructions per FMA instead of 2 for the one-output-per-lane form).

template <int FPL, int TT = MLPG_TT>   // FPL: frames per lane of the compute phase: TT / FPL frame groups x 32 column pairs = TT * 32 / FPL compute threads;
                                       // TT: output frames per workgroup (32, or 64: half the halo re-reads, one workgroup per CU)
__global__ __launch_bounds__(MLPG_THREADS) void mlpg_forward_kernel(
    const float* __restrict__ y, int ldy, const float* __restrict__ band, int kb, int nW,
    const int* __restrict__ scol, const int* __restrict__ sstride, int Ds,
    float* __restrict__ ys, int ldys, int B, int T) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nb = 2 * kb + 1, nbp = nb + 2 * MLPG_PAD;
  const int tiles_t = (T + TT - 1) / TT;
  const int b = blockIdx.x / tiles_t, t0 = (blockIdx.x % tiles_t) * TT;
  const int c0 = blockIdx.y * MLPG_CC;
  const int nc = min(MLPG_CC, Ds - c0);
  const int rows = TT + 2 * kb;
  float* sb = sm + rows * nW * MLPG_CC;            // [TT][nW][nbp]
  const float* yb = y + (long)b * T * ldy;
  // Staging is one wave per LDS row (64 lanes = the 64 columns of a data row / the taps of a band row), rows strided over
  // the 16 waves, (row, window) advanced incrementally: no integer division per element, 8 independent loads in flight.
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = MLPG_THREADS / 64;
  // The first batch of band rows (taps jp = lane of rows wv, wv + 16, ...) is requested FIRST and parked in registers: it depends on
  // nothing, so it travels with the column-map loads and the first batch of tile rows instead of being a fourth dependent round trip
  // behind them (round 5).
  float vb0[8];
  {
    const long src_rows = (long)T * nW;
    const int jc = min(max(lane - MLPG_PAD, 0), nb - 1);
#pragma unroll
    for (int q = 0; q < 8; ++q) vb0[q] = band[min((long)t0 * nW + wv + q * nwv, src_rows - 1) * nb + jc];
  }
  {  // data tile: LDS row rw = r * nW + w holds frame t0 - kb + r, window w
    const bool c_ok = lane < nc;
    const int my_col = c_ok ? scol[c0 + lane] : 0, my_st = c_ok ? sstride[c0 + lane] : 0;
    const int nrw = rows * nW;
    const int dr = nwv / nW, dw = nwv % nW;
    int r = wv / nW, w = wv % nW;
    for (int rw0 = wv; rw0 < nrw; rw0 += 8 * nwv) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t = t0 - kb + r;
        const int tc = min(max(t, 0), T - 1);
        const float x = yb[(long)tc * ldy + my_col + (my_st > 0 ? w * my_st : 0)];
        v[q] = (c_ok && t >= 0 && t < T && (my_st > 0 || w == 0)) ? x : 0.f;
        r += dr; w += dw;
        if (w >= nW) { w -= nW; ++r; }
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int rw = rw0 + q * nwv;
        if (rw < nrw) sm[rw * MLPG_CC + lane] = v[q];
      }
    }
  }
  {  // band rows: LDS row tw = tl * nW + w  <-  band row t0 * nW + tw (the band is [t][w][nb], so rows are consecutive)
    const int nrow = TT * nW;
    const long src_rows = (long)T * nW;
    if (lane < nbp) {       // the batch requested up front
      const int j = lane - MLPG_PAD;
      const bool j_ok = j >= 0 && j < nb;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int tw = wv + q * nwv;
        if (tw < nrow) sb[tw * nbp + lane] = (j_ok && (long)t0 * nW + tw < src_rows) ? vb0[q] : 0.f;
      }
    }
    for (int jp = lane; jp < nbp; jp += 64) {      // one pass for half-widths up to 28 (nbp <= 64 taps)
      const int j = jp - MLPG_PAD;
      const bool j_ok = j >= 0 && j < nb;
      const int jc = min(max(j, 0), nb - 1);
      for (int tw0 = jp == lane ? wv + 8 * nwv : wv; tw0 < nrow; tw0 += 8 * nwv) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const long row = (long)t0 * nW + tw0 + q * nwv;
          const float x = band[min(row, src_rows - 1) * nb + jc];
          v[q] = (j_ok && row < src_rows) ? x : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int tw = tw0 + q * nwv;
          if (tw < nrow) sb[tw * nbp + jp] = v[q];
        }
      }
    }
  }
  __syncthreads();
  static_assert(FPL >= 1 && FPL <= MLPG_PAD + 1, "the band rows are padded for at most MLPG_PAD + 1 frames per lane");
  if (threadIdx.x >= TT * 32 / FPL) return;  // every wave stages (memory-level parallelism); 16 / FPL of them compute
  const int cp = threadIdx.x & 31, fg = threadIdx.x >> 5;     // column pair, frame group (FPL frames)
  const int tl0 = fg * FPL;
  float acc[FPL][2];
#pragma unroll
  for (int i = 0; i < FPL; ++i) acc[i][0] = acc[i][1] = 0.f;
  // The tap loop runs on a counter that is the same in every lane (the staged row is tl0 + j0) and is unrolled by eight: the LDS reads of
  // eight taps are in flight before the first FMA waits (round 5: written over r = tl0 .. the compiler kept a lane-dependent loop with one
  // s_waitcnt lgkmcnt(0) per tap; 20.3 -> 18.9 us at cfg2).  Same products in the same order.
  const int ntap = (FPL - 1) + nb;
  for (int w = 0; w < nW; ++w) {
    const float* dcol = sm + (tl0 * nW + w) * MLPG_CC + 2 * cp;      // + j0*nW*CC
    const float* cf = sb + (tl0 * nW + w) * nbp + MLPG_PAD;           // + i*nW*nbp + (j0 - i)
#pragma unroll 8
    for (int j0 = 0; j0 < ntap; ++j0) {
      const float2 d = *reinterpret_cast<const float2*>(dcol + j0 * nW * MLPG_CC);
#pragma unroll
      for (int i = 0; i < FPL; ++i) {
        const float cfi = cf[i * nW * nbp + j0 - i];
        acc[i][0] = fmaf(cfi, d.x, acc[i][0]);
        acc[i][1] = fmaf(cfi, d.y, acc[i][1]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = 2 * cp + q;
    if (c >= nc) continue;
    const bool pass = sstride[c0 + c] == 0;
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int t = t0 + tl0 + i;
      if (t >= T) continue;
      const float out = pass ? sm[((tl0 + i + kb) * nW + 0) * MLPG_CC + c] : acc[i][q];   // pass-through: bit-exact copy
      ys[((long)b * T + t) * ldys + c0 + c] = out;
    }
  }
}

// transpose of the above:  gy[b][t'][scol[c]+w*st] = sum_t band[t][w][t'-t+kb] * gs[b][t][c]
// plus the masked-MSE gradient in the static+delta domain when mse_w != 0:
//   gy += mse_w * 2 * (yhat*m - y*m) * m / Tv        (reference gantts/seqloss.py:41-43)
// LDS: gs tile [(TT+2kb)][CC] + the band rows of the same frames, padded, [(TT+2kb)][nW][nb+2*PAD].
// Lane = 2 columns x 4 frames x all windows: one ds_read_b64 of gs feeds 8*nW FMAs.
template <int FPL, int TT = MLPG_TT>
__global__ __launch_bounds__(MLPG_THREADS) __attribute__((amdgpu_waves_per_eu(FPL <= 2 ? 8 : 4)))      // two 16-wave workgroups per CU: <= 64 VGPRs AND <= 96 SGPRs
void mlpg_backward_kernel(
    const float* __restrict__ gs, int ldgs, const float* __restrict__ band, int kb, int nW,
    const int* __restrict__ scol, const int* __restrict__ sstride, int Ds,
    float* __restrict__ gy, int ldgy, int B, int T,
    float mse_w, const float* __restrict__ yhat, const float* __restrict__ ytgt, int ldt,
    const float* __restrict__ mask, const StepScalars* __restrict__ sc) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  const int nb = 2 * kb + 1, nbp = nb + 2 * MLPG_PAD;
  const int tiles_t = (T + TT - 1) / TT;
  const int b = blockIdx.x / tiles_t, t0 = (blockIdx.x % tiles_t) * TT;
  const int c0 = blockIdx.y * MLPG_CC;
  const int nc = min(MLPG_CC, Ds - c0);
  const int rows = TT + 2 * kb;
  float* sb = sm + rows * MLPG_CC;                 // [rows][nW][nbp]; frames outside [0,T) are zero
  const float* gb = gs + (long)b * T * ldgs;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nwv = MLPG_THREADS / 64;
  float vb0[16];            // the first TWO batches of band rows (all of them at TT = 32: (TT + 2 kb) nW / 16 <= 16 rows per wave), requested first
  {
    const long src_rows = (long)T * nW, base = (long)(t0 - kb) * nW;
    const int jc = min(max(lane - MLPG_PAD, 0), nb - 1);
#pragma unroll
    for (int q = 0; q < 16; ++q) vb0[q] = band[min(max(base + wv + q * nwv, 0L), src_rows - 1) * nb + jc];
  }
  {  // gradient tile: one wave per frame row (see the forward kernel's staging)
    const bool c_ok = lane < nc;
    const int ccl = c_ok ? c0 + lane : c0;
    for (int r0 = wv; r0 < rows; r0 += 8 * nwv) {
      float v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int t = t0 - kb + r0 + q * nwv;
        const int tc = min(max(t, 0), T - 1);
        const float x = gb[(long)tc * ldgs + ccl];
        v[q] = (c_ok && t >= 0 && t < T) ? x : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int r = r0 + q * nwv;
        if (r < rows) sm[r * MLPG_CC + lane] = v[q];
      }
    }
  }
  {  // band rows of the staged frames: LDS row rw = r * nW + w  <-  band row (t0 - kb) * nW + rw; frames outside [0,T) are zero
    const int nrow = rows * nW;
    const long src_rows = (long)T * nW, base = (long)(t0 - kb) * nW;
    if (lane < nbp) {       // the batch requested up front
      const int j = lane - MLPG_PAD;
      const bool j_ok = j >= 0 && j < nb;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int rw = wv + q * nwv;
        const long row = base + rw;
        if (rw < nrow) sb[rw * nbp + lane] = (j_ok && row >= 0 && row < src_rows) ? vb0[q] : 0.f;
      }
    }
    for (int jp = lane; jp < nbp; jp += 64) {
      const int j = jp - MLPG_PAD;
      const bool j_ok = j >= 0 && j < nb;
      const int jc = min(max(j, 0), nb - 1);
      for (int rw0 = jp == lane ? wv + 16 * nwv : wv; rw0 < nrow; rw0 += 8 * nwv) {
        float v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const long row = base + rw0 + q * nwv;
          const float x = band[min(max(row, 0L), src_rows - 1) * nb + jc];
          v[q] = (j_ok && row >= 0 && row < src_rows) ? x : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const int rw = rw0 + q * nwv;
          if (rw < nrow) sb[rw * nbp + jp] = v[q];
        }
      }
    }
  }
  __syncthreads();
  static_assert(FPL >= 1 && FPL <= MLPG_PAD + 1, "the band rows are padded for at most MLPG_PAD + 1 frames per lane");
  if (threadIdx.x >= TT * 32 / FPL) return;
  const int cp = threadIdx.x & 31, fg = threadIdx.x >> 5;
  const int tl0 = fg * FPL;
  float acc[MLPG_MAXW][FPL][2];
#pragma unroll
  for (int w = 0; w < MLPG_MAXW; ++w)
#pragma unroll
    for (int i = 0; i < FPL; ++i) acc[w][i][0] = acc[w][i][1] = 0.f;
  // staged row r holds frame t = t0 - kb + r; it reaches output frame tl (t' = t0 + tl) with
  // q = r - tl in [0, nb) through the coefficient band[t][w][nb - 1 - q]
  const int ntap = (FPL - 1) + nb;       // (uniform counter + unroll: see the forward kernel; 21.9 -> 21.1 us)
  const float* drow = sm + tl0 * MLPG_CC + 2 * cp;
  const float* cfrow = sb + (long)tl0 * nW * nbp + MLPG_PAD + (nb - 1);
#pragma unroll 4
  for (int j0 = 0; j0 < ntap; ++j0) {
    const float2 d = *reinterpret_cast<const float2*>(drow + j0 * MLPG_CC);
    const float* cf = cfrow + (long)j0 * nW * nbp - j0;   // + w*nbp + i
#pragma unroll
    for (int w = 0; w < MLPG_MAXW; ++w) {
      if (w >= nW) break;
#pragma unroll
      for (int i = 0; i < FPL; ++i) {
        const float cfi = cf[w * nbp + i];
        acc[w][i][0] = fmaf(cfi, d.x, acc[w][i][0]);
        acc[w][i][1] = fmaf(cfi, d.y, acc[w][i][1]);
      }
    }
  }
  const float msk_scale = mse_w != 0.f ? 2.f * mse_w * sc->inv_tv : 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int c = 2 * cp + q;
    if (c >= nc) continue;
    const int col0 = scol[c0 + c], st = sstride[c0 + c];
#pragma unroll
    for (int i = 0; i < FPL; ++i) {
      const int tp = t0 + tl0 + i;
      if (tp >= T) continue;
      const long row = (long)b * T + tp;
      const float m = msk_scale != 0.f ? mask[row] : 0.f;
#pragma unroll
      for (int w = 0; w < MLPG_MAXW; ++w) {
        if (w >= nW || (st == 0 && w > 0)) break;
        float out = st == 0 ? sm[(tl0 + i + kb) * MLPG_CC + c] : acc[w][i][q];
        const int col = col0 + w * st;
        if (msk_scale != 0.f) out += msk_scale * (yhat[row * ldt + col] * m - ytgt[row * ldt + col] * m) * m;
        gy[row * ldgy + col] = out;
      }
    }
  }
}

}  // namespace gt
