// Normalisation statistics of one side of a device-resident corpus in one pass (gt_op_corpus_stats; gantts_amd/data.py:
// ResidentCorpus.minmax / .meanvar): per column min and max in float32 and (count, mean, M2 = sum (x - mean)^2) in float64 over the
// valid rows of A [F][ld], what data.minmax / data.meanvar compute on the host one utterance at a time (train.py:718-751).
//
// Valid rows: a device table seg [n_seg][2] int64 = (first frame, valid frame count), in ascending order, none beginning before the
// previous one ends (the corpus' offsets with each utterance cut to lengths[idx]).  A segment that does not lie inside [0, F) counts
// as empty, the rule of gt_op_assemble_batch's table rows.  Rows outside every segment and the pad columns [D, ld) reach no result;
// a table out of order gives statistics of the wrong rows but never a read outside [0, F): rows are addressed from the slab, not
// from the table.
//
// Two launches, no atomics, every combination in a fixed order: the result does not depend on which workgroup finishes first.
//   corpus_stats_slab_kernel    workgroup p owns the CS_SLAB rows [p * CS_SLAB, ...).  It finds the slab's segments by bisection, marks
//       the valid rows in LDS and sweeps the slab once per chunk of 256 columns: a lane holds a float4 (4 columns) of a row, LPR = the
//       power of two >= ld / 4 (at most 64) lanes a row, 64 / LPR rows a wave-instruction (1 KiB contiguous when ld / 4 = LPR), 4 rows
//       in flight per lane before the first is used.  Each lane runs Welford's recurrence in double over its own rows (the reciprocal
//       1 / n from a table in LDS, shared by its 4 columns) and the NaN-propagating min / max of numpy; the lanes and waves that hold the same column
//       meet in LDS and are folded in ascending order by Chan's pairwise update
//           d = m_b - m_a,  w = k / (n + k),  m = m_a + d w,  M2 = M2_a + M2_b + d^2 n w
//       (data.meanvar's, with the weight k / (n + k) formed once); the workgroup's partial (n, mean, M2, min, max) per column goes to the caller's workspace.
//   corpus_stats_merge_kernel   4 columns a workgroup (many small workgroups: one CU reads slowly, and the partials are 3 % of the corpus),
//       CS_FANIN = 64 threads a column: thread q folds partials q, q + 64, ... in ascending order, 8 loaded before the first is folded,
//       an LDS tree folds the 64 in a fixed pairing, and the prior (mean_, var_, last_sample_count; M2 = var_ n) is continued
//       by the total: meanvar(..., mean_=, var_=, last_sample_count=).
// Nowhere is a sum of squares formed: a constant column leaves every d at exactly 0, so its mean is the constant and its M2 is 0.0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gt {

constexpr int CS_WAVES = 4, CS_THREADS = CS_WAVES * 64, CS_SLAB = 256, CS_IN_FLIGHT = 4;      // GT_CORPUS_STATS_SLAB
constexpr int CS_FANIN = 64, CS_MERGE_COLS = 4, CS_MERGE_THREADS = CS_FANIN * CS_MERGE_COLS; // GT_CORPUS_STATS_FANIN
constexpr int CS_MERGE_BATCH = 8;
static_assert(CS_THREADS == CS_SLAB, "one thread clears one row's flag and fills one entry of the reciprocal table");

struct CorpusStatsArgs {
  int D, ld, lpr_log2;
  long F, n_seg, n_part;
  double prior_count;
  const float* A;
  const long* seg;
  const double *prior_mean, *prior_var;
  // workspace: [n_part][3][ld] double (n, mean, M2), then [n_part][2][ld] float (min, max)
  double* part_d;
  float* part_f;
  float *out_min, *out_max;
  double *out_count, *out_mean, *out_m2;
};

__host__ __device__ inline long corpus_stats_parts(long F) { return (F + CS_SLAB - 1) / CS_SLAB; }
__host__ __device__ inline size_t corpus_stats_ws_bytes(long F, int ld) {
  return (size_t)corpus_stats_parts(F) * (size_t)ld * (3 * sizeof(double) + 2 * sizeof(float));
}

// (n, m, M2) <- (n, m, M2) joined with (k, mb, M2b): Chan et al.; an empty side changes nothing.
__device__ __forceinline__ void cs_chan(double& n, double& m, double& M2, double k, double mb, double M2b) {
  if (k == 0.0) return;
  if (n == 0.0) { n = k; m = mb; M2 = M2b; return; }
  const double tot = n + k, d = mb - m, w = k / tot;
  m = m + d * w;
  M2 = M2 + M2b + d * d * (n * w);
  n = tot;
}
// numpy's minimum / maximum: a NaN on either side is the result (IEEE 754-2019 minimum / maximum: one v_minimum3_f32 / v_maximum3_f32)
__device__ __forceinline__ float cs_min(float a, float b) { return __builtin_elementwise_minimum(a, b); }
__device__ __forceinline__ float cs_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }

// first frame and valid count of segment s; a segment that does not lie inside [0, F) is empty
__device__ __forceinline__ void cs_segment(const long* seg, long s, long F, long& start, long& len) {
  start = seg[2 * s];
  len = seg[2 * s + 1];
  if (start < 0 || len < 0 || start > F || len > F - start) len = 0;
}

__global__ __launch_bounds__(CS_THREADS) void corpus_stats_slab_kernel(const CorpusStatsArgs g) {
  __shared__ unsigned char s_valid[CS_SLAB];
  __shared__ __align__(16) double s_mean[CS_THREADS * 4];      // [fold index][column of the chunk]: 4 * RPW rows of 4 * LPR columns
  __shared__ __align__(16) double s_m2[CS_THREADS * 4];
  __shared__ __align__(16) float s_lo[CS_THREADS * 4];
  __shared__ __align__(16) float s_hi[CS_THREADS * 4];
  __shared__ double s_n[CS_THREADS];                           // [fold index][float4 of the chunk]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long r0 = (long)blockIdx.x * CS_SLAB;
  const int rows = (int)(g.F - r0 < CS_SLAB ? g.F - r0 : CS_SLAB);

  // ---- the slab's valid rows ----------------------------------------------------------------------------------------------------
  s_valid[tid] = 0;      // CS_THREADS == CS_SLAB
  __syncthreads();
  long lo = 0, hi = g.n_seg;      // first segment that ends after r0 (the ends ascend)
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    long start, len;
    cs_segment(g.seg, mid, g.F, start, len);
    if (start + len > r0) hi = mid; else lo = mid + 1;
  }
  for (long s = lo + tid; s < g.n_seg; s += CS_THREADS) {
    long start, len;
    cs_segment(g.seg, s, g.F, start, len);
    if (start >= r0 + rows) break;
    const long a = start > r0 ? start : r0, b = start + len < r0 + rows ? start + len : r0 + rows;
    for (long r = a; r < b; ++r) s_valid[r - r0] = 1;
  }
  __syncthreads();

  const int lpr = 1 << g.lpr_log2, rpw = 64 >> g.lpr_log2;      // lanes per row, rows per wave-instruction
  const int v = lane & (lpr - 1), sub = lane >> g.lpr_log2;
  const int fold = wave * rpw + sub, n_fold = CS_WAVES * rpw;   // this lane's place among those that share its columns
  const int step = CS_WAVES * rpw;                              // rows per workgroup-instruction
  const int nv = g.ld >> 2;

  double* s_inv = s_mean;      // 1 / k, k = 1 .. CS_SLAB, while the rows are swept: the fold's arrays are idle then
  for (int v0 = 0; v0 < nv; v0 += 64) {      // chunks of 256 columns; one chunk unless ld > 256
    s_inv[tid + 1] = 1.0 / (double)(tid + 1);
    __syncthreads();
    const bool has_cols = v0 + v < nv;
    const float* col = g.A + r0 * g.ld + 4 * (v0 + v);
    int cnt = 0;
    double mean[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};
    float mn[4], mx[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { mn[e] = __builtin_inff(); mx[e] = -__builtin_inff(); }
    for (int rb = 0; rb < rows; rb += CS_IN_FLIGHT * step) {
      float4 q[CS_IN_FLIGHT];
      bool ok[CS_IN_FLIGHT];
#pragma unroll
      for (int j = 0; j < CS_IN_FLIGHT; ++j) {
        const int r = rb + j * step + fold;
        ok[j] = has_cols && r < rows && s_valid[r < CS_SLAB ? r : 0];
        q[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[j]) q[j] = *(const float4*)(col + (long)r * g.ld);
      }
#pragma unroll
      for (int j = 0; j < CS_IN_FLIGHT; ++j) {
        if (!ok[j]) continue;
        const float x4[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
        const double inv = s_inv[++cnt];      // the correctly rounded 1 / n, shared by the lane's 4 columns
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const double x = (double)x4[e], d = x - mean[e];
          mean[e] += d * inv;
          m2[e] += d * (x - mean[e]);
          mn[e] = cs_min(mn[e], x4[e]);
          mx[e] = cs_max(mx[e], x4[e]);
        }
      }
    }
    // ---- lanes and waves that hold the same columns meet in LDS; thread c folds column c of the chunk in ascending order ---------
    const int cw = 4 * lpr;      // columns of the chunk that have a holder
    __syncthreads();             // every wave is done with s_inv
    s_n[fold * lpr + v] = (double)cnt;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int at = fold * cw + 4 * v + e;
      s_mean[at] = mean[e]; s_m2[at] = m2[e]; s_lo[at] = mn[e]; s_hi[at] = mx[e];
    }
    __syncthreads();
    const int c = 4 * v0 + tid;
    if (tid < cw && c < g.D) {
      double tn = 0.0, tm = 0.0, t2 = 0.0;
      float tlo = __builtin_inff(), thi = -__builtin_inff();
      for (int k = 0; k < n_fold; ++k) {
        cs_chan(tn, tm, t2, s_n[k * lpr + (tid >> 2)], s_mean[k * cw + tid], s_m2[k * cw + tid]);
        tlo = cs_min(tlo, s_lo[k * cw + tid]);
        thi = cs_max(thi, s_hi[k * cw + tid]);
      }
      double* pd = g.part_d + (long)blockIdx.x * 3 * g.ld;
      float* pf = g.part_f + (long)blockIdx.x * 2 * g.ld;
      pd[c] = tn; pd[g.ld + c] = tm; pd[2 * g.ld + c] = t2;
      pf[c] = tlo; pf[g.ld + c] = thi;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(CS_MERGE_THREADS) void corpus_stats_merge_kernel(const CorpusStatsArgs g) {
  __shared__ double s_n[CS_MERGE_THREADS], s_mean[CS_MERGE_THREADS], s_m2[CS_MERGE_THREADS];
  __shared__ float s_lo[CS_MERGE_THREADS], s_hi[CS_MERGE_THREADS];
  const int tid = threadIdx.x, cl = tid & (CS_MERGE_COLS - 1), q = tid / CS_MERGE_COLS;
  const int c = blockIdx.x * CS_MERGE_COLS + cl;
  const bool live = c < g.D;
  double n = 0.0, m = 0.0, M2 = 0.0;
  float lo = __builtin_inff(), hi = -__builtin_inff();
  if (live)
    for (long p0 = q; p0 < g.n_part; p0 += (long)CS_MERGE_BATCH * CS_FANIN) {      // a batch's loads are issued before its first fold
      double bn[CS_MERGE_BATCH], bm[CS_MERGE_BATCH], b2[CS_MERGE_BATCH];
      float blo[CS_MERGE_BATCH], bhi[CS_MERGE_BATCH];
#pragma unroll
      for (int j = 0; j < CS_MERGE_BATCH; ++j) {
        const long p = p0 + (long)j * CS_FANIN;
        const bool in = p < g.n_part;
        const double* pd = g.part_d + (in ? p : 0) * 3 * g.ld;
        const float* pf = g.part_f + (in ? p : 0) * 2 * g.ld;
        bn[j] = in ? pd[c] : 0.0; bm[j] = pd[g.ld + c]; b2[j] = pd[2 * g.ld + c];
        blo[j] = in ? pf[c] : __builtin_inff(); bhi[j] = in ? pf[g.ld + c] : -__builtin_inff();
      }
#pragma unroll
      for (int j = 0; j < CS_MERGE_BATCH; ++j) {
        cs_chan(n, m, M2, bn[j], bm[j], b2[j]);
        lo = cs_min(lo, blo[j]);
        hi = cs_max(hi, bhi[j]);
      }
    }
  s_n[tid] = n; s_mean[tid] = m; s_m2[tid] = M2; s_lo[tid] = lo; s_hi[tid] = hi;
  __syncthreads();
  for (int h = CS_FANIN / 2; h >= 1; h >>= 1) {      // thread (q, column) takes (q + h, column)
    if (q < h) {
      const int o = tid + h * CS_MERGE_COLS;
      cs_chan(n, m, M2, s_n[o], s_mean[o], s_m2[o]);
      lo = cs_min(lo, s_lo[o]);
      hi = cs_max(hi, s_hi[o]);
      s_n[tid] = n; s_mean[tid] = m; s_m2[tid] = M2; s_lo[tid] = lo; s_hi[tid] = hi;
    }
    __syncthreads();
  }
  if (q == 0 && live) {
    // the prior comes first, as the host continues from it; an empty selection leaves the prior as it is
    double pn = g.prior_count, pm = g.prior_mean ? g.prior_mean[c] : 0.0;
    double p2 = (g.prior_var ? g.prior_var[c] : 0.0) * pn;
    cs_chan(pn, pm, p2, n, m, M2);
    g.out_min[c] = lo; g.out_max[c] = hi;
    g.out_count[c] = pn; g.out_mean[c] = pm; g.out_m2[c] = p2;
  }
}

}  // namespace gt
