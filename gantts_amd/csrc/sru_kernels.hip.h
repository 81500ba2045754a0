// SRU recurrence of SRURNN (reference gantts/models.py:144-167 -> third-party `cuda_functional.SRU`,
// github.com/taolei87/sru 2017 layout, NOT vendored in the reference: restated from the published
// recurrence, Lei et al. 2017 arXiv:1709.02755; parity unpinned, see oracle/gantts_oracle.py).
//
//   U = x W  (one f32 MFMA GEMM per layer, gemm_f32.hip.h; column j owns U[.., j*k .. j*k+k-1])
//   f = sigmoid(u1 + b_f[j]),  r = sigmoid(u2 + b_r[j])
//   c_t = (c_{t-1} - u0) f + u0
//   h_t = (g(c_t) mask_h - x') r + x'          x' = x_t[j] (k == 3) or u3 (k == 4)
//
// The scan is sequential in time per (sequence, column) and embarrassingly parallel across them:
// one lane per column, lanes <-> consecutive columns (coalesced rows of U), time unrolled by 4 so
// that the U / x loads of the next frames (which do not depend on the carried state) are in flight
// while the current frame is computed -> HBM-streaming bound.  Columns j >= H of a bidirectional
// layer walk time backwards.  Sequence lengths are ignored, exactly like the reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "gemm_f32.hip.h"
#include "fast_math.hip.h"
#include "sru_args.hip.h"

namespace gt {

__device__ __forceinline__ float sru_act(float c, int act) { return act == SRU_RELU ? fmaxf(c, 0.f) : (act == SRU_TANH ? tanhf(c) : c); }
__device__ __forceinline__ float sru_dact(float c, float val, int act) {
  return act == SRU_RELU ? (c > 0.f ? 1.f : 0.f) : (act == SRU_TANH ? 1.f - val * val : 1.f);
}
__device__ __forceinline__ float sru_mask(const SruArgs& a, int b, int col) {
  if (!a.use_mask) return 1.f;
  if (a.mask_buf) return a.mask_buf[(long)b * (a.H * a.dirs) + col] != 0.f ? a.keep_scale : 0.f;
  uint32_t r[4];
  philox4x32_10((uint32_t)(a.seq_add + a.seq_mul * b), (uint32_t)col, a.key0, a.key1, r);
  return r[0] >= a.thresh ? a.keep_scale : 0.f;
}

// One frame of the recurrence / of its adjoint, written with explicit fmaf / __fmul_rn: the contractions are fixed here, not
// chosen by the compiler per call site.
struct SruFwdOut { float c, h; };
// The two sigmoids are fast_sigmoid (fast_math.hip.h: v_exp_f32 + v_rcp_f32, a few ulp): with one or two waves per SIMD the
// scan is bound by the instruction count of a frame, and the library expf was most of it.
// The gates (f, r) of a block of frames do not depend on the carried state: the kernels evaluate them for the whole block first
// (independent transcendental chains the scheduler can interleave), then walk the short dependent chain.
__device__ __forceinline__ SruFwdOut sru_fwd_frame(float u0, float f, float r, float xp, float c_in, float mk, int act) {
  SruFwdOut o;
  o.c = fmaf(c_in - u0, f, u0);
  const float val = __fmul_rn(sru_act(o.c, act), mk);
  o.h = fmaf(val - xp, r, xp);
  return o;
}
struct SruBwdOut { float du0, du1, du2, dxp, dc; };
__device__ __forceinline__ SruBwdOut sru_bwd_frame(float u0, float f, float r, float xp, float c_here, float c_prev, float dh, float dc_in,
                                                   float mk, int act) {
  const float val = sru_act(c_here, act);
  const float dr = __fmul_rn(dh, fmaf(val, mk, -xp));
  SruBwdOut o;
  o.dxp = __fmul_rn(dh, 1.f - r);
  const float dct = fmaf(__fmul_rn(__fmul_rn(dh, r), mk), sru_dact(c_here, val, act), dc_in);
  o.du0 = __fmul_rn(dct, 1.f - f);
  const float df = __fmul_rn(dct, c_prev - u0);
  o.dc = __fmul_rn(dct, f);
  o.du1 = __fmul_rn(__fmul_rn(df, f), 1.f - f);
  o.du2 = __fmul_rn(__fmul_rn(dr, r), 1.f - r);
  return o;
}

// The scan has only B * ncols independent lanes (32 768 at B = 32, 6x512 bidirectional): its HBM rate is set by the bytes
// each lane keeps in flight: SRU_UNROLL_F / _B frames of loads per lane (under the 63 the vmcnt counter can track) and
// 64-lane workgroups, so that the 512 waves spread over all 256 CUs instead of 128.
constexpr int SRU_UNROLL_F = 12;      // forward: 4 loads per frame -> 48 in flight
constexpr int SRU_UNROLL_B = 8;       // backward: 6 loads per frame (7 with the next layer's highway gradient) -> 48 / 56 in flight
// (measured per layer at B = 32, T = 1024, 6x512 bidirectional: 4 frames x 256-lane workgroups 430 / 648 us forward /
//  backward; 8 frames x 64 lanes 320 / 428 us; 12 frames forward 284 us; dwordx3 / dwordx4 loads of a frame's k values are
//  SLOWER: 352 / 737 us)
constexpr int SRU_THREADS = 64;

// grid = ceil(B*ncols / SRU_THREADS)
__global__ __launch_bounds__(SRU_THREADS) void sru_fwd_kernel(const SruArgs a) {
  const int ncols = a.H * a.dirs;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)a.B * ncols) return;
  const int col = (int)(gid % ncols), b = (int)(gid / ncols);
  const bool flip = col >= a.H;                 // reverse direction
  const int T = a.T, k = a.k;
  const float bf = a.bias[col], br = a.bias[ncols + col];
  const float mk = sru_mask(a, b, col);
  const float* Ub = a.U + (long)b * T * a.ldu + (long)col * k;
  const float* xb = a.x + (long)b * T * a.ldx + col;
  float* hb = a.h + (long)b * T * ncols + col;
  float* cb = a.c + (long)b * T * ncols + col;
  float c = 0.f;
  for (int t0 = 0; t0 < T; t0 += SRU_UNROLL_F) {
    float u0[SRU_UNROLL_F], u1[SRU_UNROLL_F], u2[SRU_UNROLL_F], xp[SRU_UNROLL_F];
#pragma unroll
    for (int q = 0; q < SRU_UNROLL_F; ++q) {      // loads of the next frames: independent of c
      const int tt = min(t0 + q, T - 1);
      const int t = flip ? T - 1 - tt : tt;
      const float* u = Ub + (long)t * a.ldu;
      u0[q] = u[0]; u1[q] = u[1]; u2[q] = u[2];
      xp[q] = k == 3 ? xb[(long)t * a.ldx] : u[3];
    }
#pragma unroll
    for (int q = 0; q < SRU_UNROLL_F; ++q) { u1[q] = fast_sigmoid(u1[q] + bf); u2[q] = fast_sigmoid(u2[q] + br); }     // f, r
#pragma unroll
    for (int q = 0; q < SRU_UNROLL_F; ++q) {
      const int tt = t0 + q;
      if (tt < T) {                               // predicated, not a break: the frame loop stays fully unrolled (registers)
        const int t = flip ? T - 1 - tt : tt;
        const SruFwdOut o = sru_fwd_frame(u0[q], u1[q], u2[q], xp[q], c, mk, a.act);
        c = o.c;
        hb[(long)t * ncols] = o.h;
        cb[(long)t * ncols] = c;
      }
    }
  }
}

// same thread mapping, time walked in the reverse of the forward order
__global__ __launch_bounds__(SRU_THREADS) void sru_bwd_kernel(const SruArgs a) {
  const int ncols = a.H * a.dirs;
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (long)a.B * ncols) return;
  const int col = (int)(gid % ncols), b = (int)(gid / ncols);
  const bool flip = col >= a.H;
  const int T = a.T, k = a.k;
  const float bf = a.bias[col], br = a.bias[ncols + col];
  const float mk = sru_mask(a, b, col);
  const float* Ub = a.U + (long)b * T * a.ldu + (long)col * k;
  const float* xb = a.x + (long)b * T * a.ldx + col;
  const float* cb = a.c + (long)b * T * ncols + col;
  const float* dhb = a.dh + (long)b * T * ncols + col;
  const float up_mul = a.up_mul ? a.up_mul[(long)b * ncols + col] : 1.f;
  const float* upb = a.up_add ? a.up_add + (long)b * T * a.ld_up_add + col : nullptr;
  float* dUb = a.dU + (long)b * T * a.ldu + (long)col * k;
  float* dxb = a.dx ? a.dx + (long)b * T * a.lddx + col : nullptr;
  float dc = 0.f, dbf = 0.f, dbr = 0.f;
  // c_{tt-1} of a frame is c_tt of the frame the walk visits next: the cell states are read once -- cc[q + 1] is frame
  // q's predecessor, and the first state of the NEXT block of frames is requested with this block (cc[SRU_UNROLL_B])
  float c_first = cb[(long)(flip ? 0 : T - 1) * ncols];
  for (int s0 = 0; s0 < T; s0 += SRU_UNROLL_B) {
    float u0[SRU_UNROLL_B], u1[SRU_UNROLL_B], u2[SRU_UNROLL_B], xp[SRU_UNROLL_B], cc[SRU_UNROLL_B + 1], dh[SRU_UNROLL_B];
    cc[0] = c_first;
#pragma unroll
    for (int q = 0; q < SRU_UNROLL_B; ++q) {
      const int tt = max(T - 1 - (s0 + q), 0);          // forward-order index, descending
      const int t = flip ? T - 1 - tt : tt;
      const int tp = flip ? t + 1 : t - 1;              // frame of c_{tt-1}
      const float* u = Ub + (long)t * a.ldu;
      u0[q] = u[0]; u1[q] = u[1]; u2[q] = u[2];
      xp[q] = k == 3 ? xb[(long)t * a.ldx] : u[3];
      cc[q + 1] = tt > 0 ? cb[(long)min(max(tp, 0), T - 1) * ncols] : 0.f;
      dh[q] = fmaf(dhb[(long)t * ncols], up_mul, upb ? upb[(long)t * a.ld_up_add] : 0.f);
    }
    c_first = cc[SRU_UNROLL_B];
#pragma unroll
    for (int q = 0; q < SRU_UNROLL_B; ++q) { u1[q] = fast_sigmoid(u1[q] + bf); u2[q] = fast_sigmoid(u2[q] + br); }     // f, r
#pragma unroll
    for (int q = 0; q < SRU_UNROLL_B; ++q) {
      const int tt = T - 1 - (s0 + q);
      if (tt < 0) continue;                       // (the tail of the last block of frames)
      const int t = flip ? T - 1 - tt : tt;
      const SruBwdOut o = sru_bwd_frame(u0[q], u1[q], u2[q], xp[q], cc[q], cc[q + 1], dh[q], dc, mk, a.act);
      dc = o.dc;
      float* du = dUb + (long)t * a.ldu;
      du[0] = o.du0; du[1] = o.du1; du[2] = o.du2;
      if (k == 3) dxb[(long)t * a.lddx] = o.dxp; else du[3] = o.dxp;
      dbf += o.du1; dbr += o.du2;
    }
  }
  a.dbias_part[(long)b * 2 * ncols + col] = dbf;
  a.dbias_part[(long)b * 2 * ncols + ncols + col] = dbr;
}

// Helpers of the cooperative block scans (sru_cs_kernels.hip.h).  sru_ring_barrier: the workgroup barrier between the phases of a block,
// a bare s_barrier behind lgkmcnt(0) -- what is exchanged is in LDS; __syncthreads() would also drain the global loads of the next
// block that are in flight, i.e. undo the run-ahead.  sru_pack_bf16x2: two floats rounded to bf16, as one 32-bit word of an image store.
__device__ __forceinline__ void sru_ring_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ unsigned sru_pack_bf16x2(float lo, float hi) {
  return (unsigned)__builtin_bit_cast(unsigned short, (__bf16)lo) | ((unsigned)__builtin_bit_cast(unsigned short, (__bf16)hi) << 16);
}

// The variational input-dropout mask of a layer as multipliers {0, 1/(1-p)}, [B][n]: drawn once per step (Philox, or the
// injected 0/1 mask of the parity hook) and read by the forward pass (dropout kernel below, or the fused dropout + bf16
// cast of GT_OPT_MATMUL_BF16) and by the backward scan of the layer underneath (SruArgs::up_mul).
__global__ void sru_input_mask_kernel(float* __restrict__ mul, int B, int n, float keep_scale, uint32_t thresh, uint32_t key0, uint32_t key1,
                                      const float* __restrict__ inj, int seq_mul, int seq_add) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * n) return;
  bool keep;
  if (inj) keep = inj[e] != 0.f;
  else {
    uint32_t r[4];
    philox4x32_10((uint32_t)(seq_add + seq_mul * (e / n)), (uint32_t)(e % n), key0, key1, r);
    keep = r[0] >= thresh;
  }
  mul[e] = keep ? keep_scale : 0.f;
}

// variational input dropout for the float32 products: y[row][i] = x[row][i] * mul[b][i]    (mask shared over time)
__global__ void sru_input_dropout_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int B, int T, int n,
                                         const float* __restrict__ mul) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)B * T * n) return;
  const int i = (int)(e % n);
  const long row = e / n;
  y[row * ldy + i] = x[row * ldx + i] * mul[(row / T) * n + i];
}

// The last step of a discriminator's gradient w.r.t. its input (eng_sru.hip: sru_stack_backward): g = dU0 . W0^T of the generated rows'
// adversarial columns, dense [rows][Da], becomes  g * mul[b][j] + hw[row][j]  in place -- layer 0's variational input-dropout multiplier
// (one per (sequence, column), shared over time; null: 1) and the k = 3 highway gradient of the layer-0 scan (null: 0).  mul / hw point at
// the first generated sequence / row and the first adversarial column.  One lane owns four consecutive elements of the dense buffer:
// one 16-byte load and store of g where the buffer allows, the gathered operands element by element.
__global__ __launch_bounds__(256) void sru_dx_adv_finish_kernel(const SruDxAdvArgs a) {
  const long total = a.rows * a.Da;
  const long e0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (e0 >= total) return;
  const bool vec = e0 + 4 <= total && (((uintptr_t)a.dx_adv & 15) == 0);
  float g[4];
  if (vec) { const float4 v = *(const float4*)(a.dx_adv + e0); g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w; }
  else {
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] = e0 + q < total ? a.dx_adv[e0 + q] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long e = min(e0 + q, total - 1);
    const long row = e / a.Da;
    const int j = (int)(e - row * a.Da);
    const float m = a.mul ? a.mul[(row / a.T) * a.ld_mul + j] : 1.f;
    const float h = a.hw ? a.hw[row * a.ld_hw + j] : 0.f;
    g[q] = fmaf(g[q], m, h);
  }
  if (vec) *(float4*)(a.dx_adv + e0) = make_float4(g[0], g[1], g[2], g[3]);
  else {
#pragma unroll
    for (int q = 0; q < 4; ++q) if (e0 + q < total) a.dx_adv[e0 + q] = g[q];
  }
}

}  // namespace gt
