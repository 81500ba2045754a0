// Launch functions of the per-frame kernels that sit between the products of a G+D step (frame_kernels.hip.h): the masked sums of
// squares and their gradient, the gradient assembly at y_hat_static with its finalisation rider, the valid-frame count, the scalar
// finalisation, the highway combine, the sigmoid / dropout element kernels and the builders of the discriminator's input images.
// One function per launch, with its grid arithmetic: shared by the step (eng_step.hip, eng_comm.hip, eng_lstm.hip, eng_sru.hip) and the
// parity hook gt_op_frame (eng_ops.hip).  Nothing here knows the engine: every buffer is a pointer, every matrix comes with its pitch.
// The functions only enqueue; the caller checks the launch (LAUNCH_CHECK).
#pragma once
#include "frame_kernels.hip.h"

namespace gt {

constexpr int FRAME_RED_MAX_BLOCKS = 1024;      // workgroups (= partials) of a masked reduction: the engine's cap
constexpr int MASK_SUM_THREADS = 1024;          // the one workgroup of mask_sum_kernel / mask_total_kernel

// workgroups of a masked reduction over n elements: four elements per thread, at most max_blocks
inline int frame_red_blocks(long n, int max_blocks = FRAME_RED_MAX_BLOCKS) {
  const long b = (n + RED_THREADS * 4 - 1) / (RED_THREADS * 4);
  return (int)(b < max_blocks ? b : max_blocks);
}
inline int frame_grid(long n, int threads = 256) { return (int)((n + threads - 1) / threads); }

// ---- the valid-frame count -----------------------------------------------------------------
inline void launch_mask_sum(const float* mask, long n, float tv_override, const double* tv_dev, StepScalars* sc, hipStream_t s) {
  hipLaunchKernelGGL(mask_sum_kernel, dim3(1), dim3(MASK_SUM_THREADS), 0, s, mask, (int)n, tv_override, tv_dev, sc);
}
inline void launch_mask_total(const float* mask, long n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(mask_total_kernel, dim3(1), dim3(MASK_SUM_THREADS), 0, s, mask, (int)n, out);
}

// ---- masked sums of squares ----------------------------------------------------------------
// partial[blk] = sum over the workgroup's elements of (a m - b m)^2; g (or null) [rows][ldg] = 2 gscale (a m - b m) m / Tv
struct SqerrArgs {
  const float* a; int lda;
  const float* b; int ldb;
  const float* mask;
  long rows; int D;
  double* partial;             // one per workgroup
  float* g; int ldg;
  float gscale;
  const StepScalars* sc;       // inv_tv is read when g is given
};
// returns the number of workgroups (= partials written)
inline int launch_masked_sqerr(const SqerrArgs& q, hipStream_t s, int max_blocks = FRAME_RED_MAX_BLOCKS) {
  const int nblk = frame_red_blocks(q.rows * q.D, max_blocks);
  hipLaunchKernelGGL(masked_sqerr_kernel, dim3(nblk), dim3(RED_THREADS), 0, s, q.a, q.lda, q.b, q.ldb, q.mask, q.rows, q.D, q.partial, q.g, q.ldg,
                     q.gscale, q.sc);
  return nblk;
}
inline void launch_sum_partials(const double* partial, int n, double* out, hipStream_t s) {
  hipLaunchKernelGGL(sum_partials_kernel, dim3(1), dim3(256), 0, s, partial, n, out);
}
// both reported sums of squares of a generator step in one launch: (a1, b1) over D1 columns -> partial1, (a2, b2) over D2 -> partial2
struct GLossesArgs {
  const float* a1; int lda1; const float* b1; int ldb1; int D1; double* partial1;
  const float* a2; int lda2; const float* b2; int ldb2; int D2; double* partial2;
  const float* mask; long rows;
};
inline void launch_g_losses(const GLossesArgs& q, int* n1, int* n2, hipStream_t s, int max_blocks = FRAME_RED_MAX_BLOCKS) {
  *n1 = frame_red_blocks(q.rows * q.D1, max_blocks);
  *n2 = frame_red_blocks(q.rows * q.D2, max_blocks);
  hipLaunchKernelGGL(g_losses_kernel, dim3(*n1 + *n2), dim3(RED_THREADS), 0, s, q.a1, q.lda1, q.b1, q.ldb1, q.D1, *n1, q.partial1,
                     q.a2, q.lda2, q.b2, q.ldb2, q.D2, q.partial2, q.mask, q.rows);
}

// ---- gradient assembly at y_hat_static -----------------------------------------------------
struct StaticGradArgs {
  const float* yhs; int ld1;
  const float* ys; int ld2;
  const float* mask;
  long rows; int Ds;
  float mge_w;
  const int* adv_inv;          // [Ds] -> adversarial column or -1; null: no adversarial columns
  const float* leak; int ldl;  // kept dloss_d / dy_hat_static, or null
  const float* gadv; int lda;  // dloss_adv / dy_hat_static, or null
  float adv_w;
  float* gs; int ldg;          // the assembled gradient, or null (nothing is written)
  double* partial;             // the sum of squares per workgroup, or null
  StepScalars* sc;
  GFinalize fin;               // fin.on: one extra workgroup finalises the step's scalars
  int leak_unnorm;
};
// returns the number of workgroups that walk the elements (the rider's workgroup not counted)
inline int launch_static_grad(const StaticGradArgs& q, hipStream_t s, int max_blocks = FRAME_RED_MAX_BLOCKS) {
  const int nblk = frame_red_blocks(q.rows * q.Ds, max_blocks);
  hipLaunchKernelGGL(static_grad_kernel, dim3(nblk + (q.fin.on ? 1 : 0)), dim3(RED_THREADS), 0, s, q.yhs, q.ld1, q.ys, q.ld2, q.mask, q.rows, q.Ds,
                     q.mge_w, q.adv_inv, q.leak, q.ldl, q.gadv, q.lda, q.adv_w, q.gs, q.ldg, q.partial, q.sc, q.fin, q.leak_unnorm);
  return nblk;
}

// ---- scalar finalisation -------------------------------------------------------------------
inline void launch_finalize_g_rider(const GFinalize& fin, hipStream_t s) {
  hipLaunchKernelGGL(finalize_g_rider_kernel, dim3(1), dim3(RED_THREADS), 0, s, fin);
}
// with partials (either one): 256 threads reduce them first; without: one thread
inline void launch_finalize_g(StepScalars* sc, StepResults* out, float adv_w, float mse_w, float mge_w, int has_adv, int zero_gnorm,
                              const double* part_mge, int n_mge, const double* part_mse, int n_mse, hipStream_t s) {
  hipLaunchKernelGGL(finalize_g_kernel, dim3(1), dim3((part_mge || part_mse) ? 256 : 1), 0, s, sc, out, adv_w, mse_w, mge_w, has_adv, zero_gnorm,
                     part_mge, n_mge, part_mse, n_mse);
}
inline void launch_finalize_d(StepScalars* sc, StepResults* out, int zero_gnorm, int tv_from_sum, hipStream_t s) {
  hipLaunchKernelGGL(finalize_d_kernel, dim3(1), dim3(1), 0, s, sc, out, zero_gnorm, tv_from_sum);
}
inline void launch_scale_by_inv_tv(float* g, long n, const StepScalars* sc, hipStream_t s) {
  hipLaunchKernelGGL(scale_by_inv_tv_kernel, dim3(frame_grid(n)), dim3(256), 0, s, g, n, sc);
}

// ---- element kernels -----------------------------------------------------------------------
inline void launch_highway_forward(const float* x, int ldx, const float* Tx, int ldt, const float* Gx, int ldg, float* out, int ldo, long rows, int sd,
                                   hipStream_t s) {
  hipLaunchKernelGGL(highway_forward_kernel, dim3(frame_grid(rows * sd)), dim3(256), 0, s, x, ldx, Tx, ldt, Gx, ldg, out, ldo, rows, sd);
}
inline void launch_highway_backward(const float* g, int ldgr, const float* Tx, int ldt, const float* Gx, int ldg, float* dGx, int ld1, float* dTz, int ld2,
                                    long rows, int sd, hipStream_t s) {
  hipLaunchKernelGGL(highway_backward_kernel, dim3(frame_grid(rows * sd)), dim3(256), 0, s, g, ldgr, Tx, ldt, Gx, ldg, dGx, ld1, dTz, ld2, rows, sd);
}
inline void launch_sigmoid_grad(float* g, int ldg, const float* y, int ldy, long rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(sigmoid_grad_kernel, dim3(frame_grid(rows * cols)), dim3(256), 0, s, g, ldg, y, ldy, rows, cols);
}
// dense [rows][cols]; in == out allowed
inline void launch_dropout_apply(const float* in, float* out, long rows, int cols, const DropoutSpec& d, hipStream_t s) {
  hipLaunchKernelGGL(dropout_apply_kernel, dim3(frame_grid(rows * cols)), dim3(256), 0, s, in, out, rows, cols, d);
}

// ---- builders of the discriminator's input images and other copies ---------------------------
// out[r][0..ldo) = (r < split ? fa[r] : fb[r - split])[idx[0..na)], pad columns 0 (ldo % 4 == 0, out 16-byte aligned).
// tv_mask != null: one extra workgroup sums it, into *tv_total when given, else into sc->tv / inv_tv (tv_override > 0 wins)
struct BuildAdvArgs {
  const float* fa; const float* fb; int ldf;
  const int* idx; int na;
  float* out; int ldo;
  long split, rows;
  const float* tv_mask; long tv_n; float tv_override;
  StepScalars* sc;
  double* tv_total;
};
inline void launch_build_adv(const BuildAdvArgs& q, hipStream_t s) {
  hipLaunchKernelGGL(build_adv_kernel, dim3(frame_grid(q.rows * (q.ldo / 4)) + (q.tv_mask ? 1 : 0)), dim3(256), 0, s, q.fa, q.fb, q.ldf, q.idx, q.na,
                     q.out, q.ldo, q.split, q.rows, q.tv_mask, (int)q.tv_n, q.tv_override, q.sc, q.tv_total);
}
// rows [0, N) = [x | fa[:, idx]], rows [N, 2N) = [x | fb[:, idx]]; x dense [N][cd]
inline void launch_build_cat2(const float* x, int cd, const float* fa, const float* fb, int ldf, const int* idx, int na, float* out, int ldo, long N,
                              hipStream_t s) {
  hipLaunchKernelGGL(build_cat2_kernel, dim3(frame_grid(N * (cd + na))), dim3(256), 0, s, x, cd, fa, fb, ldf, idx, na, out, ldo, N);
}
// out[r][ooff + j] = in[r][ioff + j], j < nj: a copy between two pitches (gather_cols_kernel without an index map)
inline void launch_copy_cols(const float* in, int ldi, int ioff, float* out, int ldo, int ooff, long rows, int nj, hipStream_t s) {
  hipLaunchKernelGGL(gather_cols_kernel, dim3(frame_grid(rows * nj)), dim3(256), 0, s, in, ldi, ioff, (const int*)nullptr, out, ldo, ooff, (int)rows, nj);
}
// [rows][cols] at pitch ld_in -> pitch ldo (multiple of 4 floats, out 16-byte aligned), pad columns 0
inline void launch_repitch(const float* in, int ld_in, int cols, long rows, float* out, int ldo, hipStream_t s) {
  hipLaunchKernelGGL(repitch_kernel, dim3(frame_grid(rows * (ldo / 4))), dim3(256), 0, s, in, ld_in, cols, rows, out, ldo);
}
// dense [rows][cols] -> pitch ldo, pad columns 0
inline void launch_pad_rows(const float* in, int cols, int rows, float* out, int ldo, hipStream_t s) {
  hipLaunchKernelGGL(pad_rows_kernel, dim3(frame_grid((long)rows * ldo)), dim3(256), 0, s, in, cols, rows, out, ldo);
}
// out[c][r] = in[r][c]
inline void launch_transpose_f32(const float* in, int rows, int cols, int ldi, float* out, int ldo, hipStream_t s) {
  hipLaunchKernelGGL(transpose_f32_kernel, dim3(frame_grid(cols, 32), frame_grid(rows, 32)), dim3(256), 0, s, in, rows, cols, ldi, out, ldo);
}

}  // namespace gt
