// Batch assembly from a device-resident corpus (gt_op_assemble_batch; gantts_amd/data.py: ResidentCorpus / ResidentLoader).
//
// One launch builds everything the training loop derives from a batch (train.py:494-519 with train.py:111-159 underneath):
//   gi (B, T, Dx + nz) on pitch ld_gi   [ scaled x | z ~ U[0,1) | zero pad columns ]
//   y (B, T, Dy)   y_static (B, T, Ds)   mask (B, T)   lengths (B)
// from the un-normalised corpus X_all [F][ldX], Y_all [F][ldY] and one row of the epoch table per sequence:
//   table[slot] = { first frame, length, corpus utterance index }     (int64, slot = first_slot + b * slot_stride)
// gt_op_assemble_batch passes slot_stride 1.  gt_op_assemble_shard (one data-parallel rank's share of a batch) passes first_slot + rank
// and stride world -- local sequence b is sequence rank + world * b of the whole batch, padded to the WHOLE batch's T -- and may ask
// for tv_global, the valid frames of the whole batch: sum of min(length, T) over its slots, every rank's launch writing the same value.
//
// Arithmetic: what numpy does on the host, bit for bit.  The statistics' dtype of a side (SX, SY) is that side's compute dtype (numpy promotes the float32
// utterance to float64 when the statistics are float64, and np.array(..., dtype=np.float32) rounds ONCE at the end); every operation is
// rounded on its own -- MINMAX is a multiply, then an add (never an FMA), MEANVAR a subtraction, then a correctly rounded division.
// Frames t >= length are 0 (the host scales first and pads afterwards), not scale(0).
//
// Noise keying (restated in tests/resident_ref.py): column j of z at frame t of corpus utterance u is word j & 3 of
//   philox4x32_10(c0 = u, c1 = t * G + (j >> 2), key0, key1),   G = ceil(nz / 4),   z = (word >> 8) * 2^-24
// (c2, c3 are the constants inside philox4x32_10).  The key is the caller's: ResidentLoader passes key0 = the low word of
// hp.generator_noise_seed and key1 = its draw counter (one per epoch).  z is drawn on EVERY frame of the padded batch, t >= length
// included (train.py:504-506 draws (B, max_len, noise_dim)); it depends on which utterance the row holds, not on the row's place in
// the batch.
//
// Delta recomputation (gantts/multistream.py:15-30; DELTA): column c of y with dwin[c] = w >= 0 is
//   sum_k coef[w][k] * scaled(Y)[t + k - (len_w - 1) / 2, dsrc[c]]      frames outside [0, length) of the UTTERANCE count as 0
// accumulated in double in ascending k and rounded once; dwin[c] < 0: the plain scaled column c.
//
// Shape: one wave per destination row, ROWS_PER_WAVE rows in flight per wave (their 16-byte loads are issued before the first
// store), 4 waves per workgroup.  The statistics and the column lists are read once per workgroup into LDS.  The scaled y row
// is staged in LDS: y_static is a gather of it, and the dense (B, T, Dy) rows are not 16-byte aligned when Dy % 4 != 0, so y and
// y_static leave as consecutive dwords of consecutive lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_f32.hip.h"

namespace gt {

constexpr int ASM_WAVES = 4, ASM_ROWS_PER_WAVE = 4, ASM_ROWS_PER_WG = ASM_WAVES * ASM_ROWS_PER_WAVE;
constexpr int ASM_MAX_WINDOWS = 4, ASM_MAX_TAPS = 9;       // GT_ASSEMBLE_MAX_WINDOWS / _TAPS

struct AssembleArgs {
  int B, T, Dx, Dy, nz, Ds;
  int ldX, ldY, ld_gi, ld_y, ld_ys;
  int x_kind, y_kind, n_windows;
  uint32_t key0, key1;
  long F, first_slot, slot_stride;         // sequence b is table slot first_slot + b * slot_stride
  long tv_first;                           // tv_global: the slots [tv_first, tv_first + tv_count) of the WHOLE batch
  int tv_count;
  double* tv_global;                       // null: not wanted
  const float *X_all, *Y_all;
  const void *x_a, *x_b, *y_a, *y_b;       // MINMAX: a = scale_, b = min_;  MEANVAR: a = mean, b = std
  const long* table;
  const int32_t *scol, *dsrc, *dwin;
  float *gi, *y, *y_static, *mask;
  long* lengths;
  int win_len[ASM_MAX_WINDOWS];
  double coef[ASM_MAX_WINDOWS][ASM_MAX_TAPS];
};

// byte offset of the staged y rows inside the workgroup's LDS (16-byte aligned), and the whole allocation
__host__ __device__ inline size_t assemble_ystat_offset(size_t sx, int Dx) { return (sx * 2 * (size_t)Dx + 7) & ~(size_t)7; }
__host__ __device__ inline size_t assemble_stage_offset(size_t sx, size_t sy, int Dx, int Dy, int Ds, bool delta) {
  const size_t n = assemble_ystat_offset(sx, Dx) + sy * 2 * (size_t)Dy + sizeof(int32_t) * ((size_t)Ds + (delta ? 2 * (size_t)Dy : 0));
  return (n + 15) & ~(size_t)15;
}
__host__ __device__ inline size_t assemble_lds_bytes(size_t sx, size_t sy, int Dx, int Dy, int Ds, int ldY, bool delta) {
  return assemble_stage_offset(sx, sy, Dx, Dy, Ds, delta) + sizeof(float) * ASM_WAVES * (size_t)ldY;
}

// One element through the host's normalisation, in the statistics' dtype, every operation rounded on its own.
template <typename ST>
__device__ __forceinline__ ST assemble_scale(float v, int kind, ST a, ST b) {
#pragma clang fp contract(off)
  const ST x = (ST)v;
  if (kind == 1) { const ST m = x * a; return m + b; }
  if (kind == 2) { const ST d = x - a; return d / b; }
  return x;
}

// Valid frames of one table row in a batch padded to T: a row that does not lie inside the corpus reads nothing (the sequence comes
// out empty), a length above T is cut.
__device__ __forceinline__ long assemble_row_length(long start, long len, long F, int T) {
  if (start < 0 || len < 0 || start > F || len > F - start) len = 0;
  return len > T ? (long)T : len;
}

template <typename SX, typename SY, bool DELTA>
__global__ __launch_bounds__(ASM_WAVES * 64) void assemble_batch_kernel(const AssembleArgs g) {
  extern __shared__ __align__(16) unsigned char asm_smem[];
  // LDS: [x_a | x_b] Dx each (SX), [y_a | y_b] Dy each (SY), scol [Ds], dsrc / dwin [Dy] (DELTA), then one staged y row per wave
  SX* sxa = (SX*)asm_smem;
  SX* sxb = sxa + g.Dx;
  SY* sya = (SY*)(asm_smem + assemble_ystat_offset(sizeof(SX), g.Dx));
  SY* syb = sya + g.Dy;
  int32_t* s_scol = (int32_t*)(syb + g.Dy);
  int32_t* s_dsrc = s_scol + g.Ds;
  int32_t* s_dwin = s_dsrc + (DELTA ? g.Dy : 0);
  float* stage = (float*)(asm_smem + assemble_stage_offset(sizeof(SX), sizeof(SY), g.Dx, g.Dy, g.Ds, DELTA));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < g.Dx; c += ASM_WAVES * 64) {
    sxa[c] = g.x_kind ? ((const SX*)g.x_a)[c] : (SX)0;
    sxb[c] = g.x_kind ? ((const SX*)g.x_b)[c] : (SX)0;
  }
  for (int c = tid; c < g.Dy; c += ASM_WAVES * 64) {
    sya[c] = g.y_kind ? ((const SY*)g.y_a)[c] : (SY)0;
    syb[c] = g.y_kind ? ((const SY*)g.y_b)[c] : (SY)0;
    if (DELTA) {      // a list entry that names no column / no window reads column 0 / is a plain column
      const int sc = g.dsrc[c], w = g.dwin[c];
      s_dsrc[c] = (sc >= 0 && sc < g.Dy) ? sc : 0;
      s_dwin[c] = (w >= 0 && w < g.n_windows) ? w : -1;
    }
  }
  for (int c = tid; c < g.Ds; c += ASM_WAVES * 64) {
    const int sc = g.scol[c];
    s_scol[c] = (sc >= 0 && sc < g.Dy) ? sc : 0;
  }
  __syncthreads();
  float* my_stage = stage + (long)wave * g.ldY;

  // ---- tv_global (a sharded launch): the valid frames of the WHOLE batch, summed by wave 0 of workgroup 0 over the batch's table rows.
  // An integer sum -- exact, and the same on every rank --, converted once and stored by one lane.
  if (g.tv_global && blockIdx.x == 0 && wave == 0) {
    long long sum = 0;
    for (int i = lane; i < g.tv_count; i += 64) {
      const long* e = g.table + 3 * (g.tv_first + i);
      sum += assemble_row_length(e[0], e[1], g.F, g.T);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) *g.tv_global = (double)sum;
  }

  const long n_rows = (long)g.B * g.T;
  const long row0 = ((long)blockIdx.x * ASM_WAVES + wave) * ASM_ROWS_PER_WAVE;
  // per row of this wave (all wave-uniform): does it exist, is it a valid frame, where does it come from
  bool exists[ASM_ROWS_PER_WAVE], valid[ASM_ROWS_PER_WAVE];
  long src[ASM_ROWS_PER_WAVE], ustart[ASM_ROWS_PER_WAVE], ulen[ASM_ROWS_PER_WAVE];
  uint32_t utt[ASM_ROWS_PER_WAVE];
  int tt[ASM_ROWS_PER_WAVE];
#pragma unroll
  for (int j = 0; j < ASM_ROWS_PER_WAVE; ++j) {
    const long r = row0 + j;
    exists[j] = r < n_rows;
    const long b = exists[j] ? r / g.T : 0;
    tt[j] = exists[j] ? (int)(r - b * g.T) : 0;
    const long* e = g.table + 3 * (g.first_slot + b * g.slot_stride);
    const long start = e[0], len = assemble_row_length(start, e[1], g.F, g.T);
    utt[j] = (uint32_t)e[2];
    ustart[j] = start; ulen[j] = len;
    valid[j] = exists[j] && tt[j] < len;
    src[j] = valid[j] ? start + tt[j] : 0;
    if (exists[j] && lane == 0) {
      if (g.mask) g.mask[r] = valid[j] ? 1.f : 0.f;
      if (g.lengths && tt[j] == 0) g.lengths[b] = len;
    }
  }

  // ---- gi = [ scaled x | z | 0 ] : float4 v of the corpus row is float4 v of the output row ------------------------------------
  if (g.gi) {
    const int nv_in = (g.Dx + 3) >> 2, nv_out = g.ld_gi >> 2, G = (g.nz + 3) >> 2;
    for (int v0 = 0; v0 < nv_out; v0 += 64) {
      const int v = v0 + lane;
      float4 in[ASM_ROWS_PER_WAVE];
#pragma unroll
      for (int j = 0; j < ASM_ROWS_PER_WAVE; ++j) {
        in[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid[j] && v < nv_in) in[j] = *(const float4*)(g.X_all + src[j] * g.ldX + 4 * v);
      }
      if (v >= nv_out) continue;
#pragma unroll
      for (int j = 0; j < ASM_ROWS_PER_WAVE; ++j) {
        if (!exists[j]) continue;
        const float iv[4] = {in[j].x, in[j].y, in[j].z, in[j].w};
        float ov[4];
        int gc = -1;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = 4 * v + e;
          float o = 0.f;
          if (c < g.Dx) {
            if (valid[j]) o = (float)assemble_scale<SX>(iv[e], g.x_kind, sxa[c], sxb[c]);
          } else if (c < g.Dx + g.nz) {
            const int z = c - g.Dx;
            if ((z >> 2) != gc) {
              gc = z >> 2;
              philox4x32_10(utt[j], (uint32_t)tt[j] * (uint32_t)G + (uint32_t)gc, g.key0, g.key1, w);
            }
            o = (float)(w[z & 3] >> 8) * 5.9604644775390625e-8f;      // 2^-24: exact
          }
          ov[e] = o;
        }
        *(float4*)(g.gi + (row0 + j) * g.ld_gi + 4 * v) = make_float4(ov[0], ov[1], ov[2], ov[3]);
      }
    }
  }

  // ---- y, y_static: the scaled row through LDS ------------------------------------------------------------------------------------
  if (!g.y && !g.y_static) return;
  const int nv_y = (g.Dy + 3) >> 2;
  float4 yin[ASM_ROWS_PER_WAVE];
  if (!DELTA && nv_y <= 64) {      // the common width: every row's load in flight before the first use
#pragma unroll
    for (int j = 0; j < ASM_ROWS_PER_WAVE; ++j) {
      yin[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (valid[j] && lane < nv_y) yin[j] = *(const float4*)(g.Y_all + src[j] * g.ldY + 4 * lane);
    }
  }
#pragma unroll
  for (int j = 0; j < ASM_ROWS_PER_WAVE; ++j) {
    if (!exists[j]) continue;                      // wave-uniform
    const long r = row0 + j;
    if (valid[j]) {
      if (DELTA) {
        for (int c = lane; c < g.Dy; c += 64) {
          const int w = s_dwin[c], sc = w >= 0 ? s_dsrc[c] : c;
          const SY a = sya[sc], b = syb[sc];
          float o;
          if (w < 0) {
            o = (float)assemble_scale<SY>(g.Y_all[src[j] * g.ldY + c], g.y_kind, a, b);
          } else {
#pragma clang fp contract(off)
            const int n = g.win_len[w], half = (n - 1) >> 1;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) {
              const long t2 = (long)tt[j] + k - half;
              if (t2 < 0 || t2 >= ulen[j]) continue;
              const double s = (double)assemble_scale<SY>(g.Y_all[(ustart[j] + t2) * g.ldY + sc], g.y_kind, a, b);
              const double p = g.coef[w][k] * s;
              acc = acc + p;
            }
            o = (float)acc;
          }
          my_stage[c] = o;
        }
      } else {
        for (int v = lane; v < nv_y; v += 64) {
          const float4 q = nv_y <= 64 ? yin[j] : *(const float4*)(g.Y_all + src[j] * g.ldY + 4 * v);
          const float iv[4] = {q.x, q.y, q.z, q.w};
          float ov[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int c = 4 * v + e;
            ov[e] = c < g.Dy ? (float)assemble_scale<SY>(iv[e], g.y_kind, sya[c], syb[c]) : 0.f;
          }
          *(float4*)(my_stage + 4 * v) = make_float4(ov[0], ov[1], ov[2], ov[3]);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (g.y)
      for (int c = lane; c < g.ld_y; c += 64) g.y[r * g.ld_y + c] = (valid[j] && c < g.Dy) ? my_stage[c] : 0.f;
    if (g.y_static)
      for (int c = lane; c < g.ld_ys; c += 64) g.y_static[r * g.ld_ys + c] = (valid[j] && c < g.Ds) ? my_stage[s_scol[c]] : 0.f;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

}  // namespace gt
