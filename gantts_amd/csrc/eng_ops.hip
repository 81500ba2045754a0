// libgantts_hip.so -- stand-alone operators of the C ABI (gt_op_* but the MLPG hooks of eng_mlpg.hip, gt_compute_distortions)
#include "engine_internal.hip.h"
#include "optim_kernels.hip.h"
#include "d_tail_args.hip.h"
#include <stddef.h>

using namespace gt;
// ------------------------------------------------------------------------------------------
// stand-alone operators
// ------------------------------------------------------------------------------------------
extern "C" int gt_op_sequence_mask(const int64_t* lengths, int B, int T, float* mask, void* stream) {
  if (!lengths || !mask || B < 1 || T < 1) return fail(GT_ERR_INVALID, "bad argument");
  hipLaunchKernelGGL(sequence_mask_kernel, dim3(cdiv((long)B * T, 256)), dim3(256), 0, (hipStream_t)stream, (const long*)lengths, B, T, mask);
  LAUNCH_CHECK();
  return GT_OK;
}

extern "C" int gt_op_masked_mse(const float* input, const float* target, const float* mask, int B, int T, int D, float* loss_out,
                                float* grad_input, void* stream) {
  if (!input || !target) return fail(GT_ERR_INVALID, "null tensor");
  if (!mask) return fail(GT_ERR_INVALID, "Should provide either lengths or mask");  // seqloss.py:33-34
  hipStream_t s = (hipStream_t)stream;
  const long N = (long)B * T;
  static thread_local HookScratch tls_ws;     // grow-only, no per-call hipMalloc/hipFree (both synchronise the device)
  CHK(tls_ws.ensure(1024 + 1024 * sizeof(double)));
  void* ws = tls_ws.p;
  StepScalars* sc = (StepScalars*)ws;
  double* part = (double*)((char*)ws + 1024);
  launch_mask_sum(mask, N, -1.f, nullptr, sc, s);
  SqerrArgs q;
  memset(&q, 0, sizeof(q));
  q.a = input; q.lda = D; q.b = target; q.ldb = D; q.mask = mask; q.rows = N; q.D = D; q.partial = part; q.g = grad_input; q.ldg = D; q.gscale = 1.f; q.sc = sc;
  const int nblk = launch_masked_sqerr(q, s, 1000);
  launch_sum_partials(part, nblk, &sc->s_mse, s);
  StepScalars h;
  hipError_t err = hipMemcpyAsync(&h, sc, sizeof(h), hipMemcpyDeviceToHost, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);
  if (err != hipSuccess) return fail(GT_ERR_HIP, "masked_mse: %s", hipGetErrorString(err));
  if (loss_out) *loss_out = (float)h.s_mse / h.tv;
  return GT_OK;
}

extern "C" int gt_compute_distortions(const float* y_static, const float* y_hat_static, int Ds, const void* stat_mean,
                                      const void* stat_std, int stats_f64, const int32_t* col_stat_host,
                                      const int32_t* col_role_host, int vuv_col, const int64_t* lengths_host, int B, int T,
                                      gt_distortion_sums* out, void* stream) {
  if (!y_static || !y_hat_static || !stat_mean || !stat_std || !col_stat_host || !col_role_host || !out)
    return fail(GT_ERR_INVALID, "null argument");
  if (Ds < 1 || B < 1 || T < 1 || vuv_col >= Ds) return fail(GT_ERR_DIM, "bad sizes: Ds=%d B=%d T=%d vuv_col=%d", Ds, B, T, vuv_col);
  hipStream_t s = (hipStream_t)stream;
  const long N = (long)B * T;
  const int nblk = (int)std::min<long>(1024, cdiv(N, 4));
  std::vector<int> host(2 * Ds + B);
  for (int c = 0; c < Ds; ++c) {
    if (col_stat_host[c] < 0) return fail(GT_ERR_INVALID, "negative statistics index");
    host[c] = col_stat_host[c];
    host[Ds + c] = col_role_host[c];
  }
  for (int b = 0; b < B; ++b) {
    const int64_t n = lengths_host ? lengths_host[b] : T;
    if (n < 0 || n > T) return fail(GT_ERR_INVALID, "length %lld outside [0, T=%d]", (long long)n, T);
    host[2 * Ds + b] = (int)n;
  }
  // grow-only workspace shared by all calls of this thread: the function runs once per training step
  // (train.py:588-595) -- a hipMalloc/hipFree pair per call would synchronise the device every step
  static thread_local HookScratch tls_ws;
  const size_t off_part = ((host.size() * sizeof(int) + 255) / 256) * 256;
  const size_t off_out = off_part + (size_t)nblk * DIST_NSUM * sizeof(double);
  CHK(tls_ws.ensure(off_out + DIST_NSUM * sizeof(double)));
  void* ws = tls_ws.p;
  int* d_int = (int*)ws;
  double* part = (double*)((char*)ws + off_part);
  double* d_out = (double*)((char*)ws + off_out);
  hipError_t err = hipMemcpyAsync(d_int, host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice, s);
  if (err == hipSuccess) {
    if (stats_f64)
      hipLaunchKernelGGL(distortion_kernel<double>, dim3(nblk), dim3(256), 0, s, y_static, y_hat_static, Ds, (const double*)stat_mean,
                         (const double*)stat_std, d_int, d_int + Ds, vuv_col, d_int + 2 * Ds, B, T, part);
    else
      hipLaunchKernelGGL(distortion_kernel<float>, dim3(nblk), dim3(256), 0, s, y_static, y_hat_static, Ds, (const float*)stat_mean,
                         (const float*)stat_std, d_int, d_int + Ds, vuv_col, d_int + 2 * Ds, B, T, part);
    hipLaunchKernelGGL(distortion_finalize_kernel, dim3(1), dim3(64 * DIST_NSUM), 0, s, part, nblk, d_out);
    err = hipGetLastError();
  }
  double h[DIST_NSUM];
  if (err == hipSuccess) err = hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, s);
  if (err == hipSuccess) err = hipStreamSynchronize(s);   // also keeps `host` alive until the H2D is done
  if (err != hipSuccess) return fail(GT_ERR_HIP, "compute_distortions: %s", hipGetErrorString(err));
  out->s_mcd = h[0]; out->s_bap = h[1]; out->s_f0 = h[2]; out->n_voiced = h[3];
  out->n_vuv_err = h[4]; out->s_mse = h[5]; out->n_frames = h[6];
  return GT_OK;
}

extern "C" int gt_op_pad_sequences(const float* ragged, int D, const int64_t* start, const int64_t* len, int B, int T, float* out, int ld_out,
                                   void* stream) {
  if (!ragged || !start || !len || !out || D < 1 || B < 1 || T < 1 || ld_out < D) return fail(GT_ERR_INVALID, "bad argument");
  hipLaunchKernelGGL(pad_sequences_kernel, dim3(cdiv((long)B * T * ld_out, 256)), dim3(256), 0, (hipStream_t)stream, ragged, D,
                     (const long*)start, (const long*)len, B, T, out, ld_out);
  LAUNCH_CHECK();
  return GT_OK;
}
extern "C" int gt_op_gather_cols(const float* in, int ld_in, const int32_t* idx, int n_idx, float* out, int ld_out,
                                 int out_col_offset, int64_t rows, void* stream) {
  if (!in || !out || n_idx < 0 || rows < 0) return fail(GT_ERR_INVALID, "bad argument");
  if (rows == 0 || n_idx == 0) return GT_OK;
  hipLaunchKernelGGL(gather_cols_kernel, dim3(cdiv(rows * n_idx, 256)), dim3(256), 0, (hipStream_t)stream, in, ld_in, 0, idx, out,
                     ld_out, out_col_offset, (int)rows, n_idx);
  LAUNCH_CHECK();
  return GT_OK;
}

static DropoutSpec buffer_spec(const float* keep_mask, float p, int ld) {
  DropoutSpec d = no_drop();
  if (keep_mask && p > 0.f) { d.mode = DROP_BUFFER; d.mask = keep_mask; d.ld_mask = ld; d.p = p; d.scale = 1.f / (1.f - p); }
  return d;
}

extern "C" int gt_op_linear_forward(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy, int64_t rows,
                                    int in_dim, int out_dim, int act, const float* keep_mask, float p, void* stream) {
  if (!X || !W || !Y || rows < 1 || in_dim < 1 || out_dim < 1) return fail(GT_ERR_INVALID, "bad argument");
  if (act < 0 || act > 2) return fail(GT_ERR_INVALID, "unknown activation");
  return linear_forward(X, ldx, W, in_dim, bias, Y, ldy, rows, in_dim, out_dim, act, buffer_spec(keep_mask, p, out_dim), PREC_F32, (hipStream_t)stream);
}

extern "C" int gt_op_linear_backward(const float* dY, int lddy, const float* X, int ldx, const float* W, int64_t rows, int in_dim,
                                     int out_dim, float* dX, int lddx, const float* H_prev, int act_prev,
                                     const float* keep_mask_prev, float p_prev, float* dW, float* db, void* stream) {
  if (!dY || rows < 1 || in_dim < 1 || out_dim < 1) return fail(GT_ERR_INVALID, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (dX) {
    if (!W) return fail(GT_ERR_INVALID, "dX requested without W");
    if (act_prev != ACT_NONE && !H_prev) return fail(GT_ERR_INVALID, "activation derivative requested without H_prev");
    CHK(linear_backward_data(dY, lddy, W, in_dim, 0, dX, lddx, rows, out_dim, in_dim, act_prev, H_prev, in_dim,
                             buffer_spec(keep_mask_prev, p_prev, in_dim), PREC_F32, s));
  }
  if (dW || db) {
    if (dW && !X) return fail(GT_ERR_INVALID, "dW requested without X");
    Scratch slabs, colp;
    int r = linear_backward_weight(dY, lddy, X, ldx, rows, out_dim, in_dim, dW, db, false, slabs, colp, PREC_F32, s);
    hipError_t err = hipStreamSynchronize(s);      // on every path: slabs and colp are freed behind it
    if (r) return r;
    if (err != hipSuccess) return fail(GT_ERR_HIP, "linear_backward: %s", hipGetErrorString(err));
  }
  return GT_OK;
}

// nn.Linear forward / backward through the bf16-STORAGE products (gemm_bf16s.hip.h): operands are cast to bfloat16 images
// (both orientations) exactly as the engine keeps them with GT_OPT_MATMUL_BF16, results come back as float32.  Parity
// hook: against float64 arithmetic on the bf16-rounded operands the results agree to float32 accumulation error.
extern "C" int gt_op_linear_bf16(const float* X, const float* W, const float* bias, int64_t rows, int in_dim, int out_dim, int act,
                                 const float* keep_mask, float p, float* Y, const float* dY, const float* H_prev, int act_prev,
                                 const float* keep_mask_prev, float p_prev, float* dX, float* dW, float* db,
                                 float* Y_image, float* YT_image, void* stream) {
  if (!X || !W || rows < 1 || in_dim < 1 || out_dim < 1) return fail(GT_ERR_INVALID, "bad argument");
  if (act < 0 || act > 2 || act_prev < 0 || act_prev > 2) return fail(GT_ERR_INVALID, "unknown activation");
  hipStream_t s = (hipStream_t)stream;
  const int in8 = pad8(in_dim), out8 = pad8(out_dim);
  const long rows8 = pad8(rows);
  Scratch xb, xbt, wb, wbt, yb, ybt, dyb, dybt, hb, slabs, colp;
  int r = GT_OK;
  auto body = [&]() -> int {
    CHK(xb.ensure((size_t)rows * in8 * 2)); CHK(xbt.ensure((size_t)in_dim * rows8 * 2));
    CHK(wb.ensure((size_t)out_dim * in8 * 2)); CHK(wbt.ensure((size_t)in_dim * out8 * 2));
    CHK(cast_transpose(X, in_dim, rows, in_dim, xb.as<__bf16>(), in8, xbt.as<__bf16>(), rows8, nullptr, false, &colp, s));
    CHK(cast_transpose(W, in_dim, out_dim, in_dim, wb.as<__bf16>(), in8, wbt.as<__bf16>(), out8, nullptr, false, &colp, s));
    if (Y) {
      CHK(yb.ensure((size_t)rows * out8 * 2)); CHK(ybt.ensure((size_t)out_dim * rows8 * 2));
      GemmB16Args g = b16_args();
      g.A = xb.as<__bf16>(); g.lda = in8; g.B = wb.as<__bf16>(); g.ldb = in8; g.M = (int)rows; g.N = out_dim; g.K = in_dim;
      g.C = Y; g.ldc = out_dim; g.Cb = yb.as<__bf16>(); g.ldcb = out8; g.CbT = ybt.as<__bf16>(); g.ldcbt = (int)rows8;
      g.bias = bias; g.epi = B16_FWD; g.act = act; g.drop = buffer_spec(keep_mask, p, out_dim);
      CHK(launch_gemm_b16(g, 1, s));
      // the two bf16 images the same epilogue wrote ([frame][out] and [out][frame]), widened to float32 for inspection
      if (Y_image) {
        hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(cdiv(rows * out_dim, 256)), dim3(256), 0, s, (const __bf16*)yb.as<__bf16>(), (long)out8, rows, out_dim, Y_image);
        LAUNCH_CHECK();
      }
      if (YT_image) {
        hipLaunchKernelGGL(bf16_to_f32_kernel, dim3(cdiv(rows * out_dim, 256)), dim3(256), 0, s, (const __bf16*)ybt.as<__bf16>(), rows8, (long)out_dim, (int)rows, YT_image);
        LAUNCH_CHECK();
      }
    }
    if (dY) {
      CHK(dyb.ensure((size_t)rows * out8 * 2)); CHK(dybt.ensure((size_t)out_dim * rows8 * 2));
      CHK(cast_transpose(dY, out_dim, rows, out_dim, dyb.as<__bf16>(), out8, dybt.as<__bf16>(), rows8, nullptr, false, &colp, s));
      if (dX) {
        GemmB16Args g = b16_args();
        g.A = dyb.as<__bf16>(); g.lda = out8; g.B = wbt.as<__bf16>(); g.ldb = out8; g.M = (int)rows; g.N = in_dim; g.K = out_dim;
        g.C = dX; g.ldc = in_dim; g.epi = B16_BWD_DATA; g.act = ACT_NONE;
        if (H_prev && act_prev != ACT_NONE) {
          CHK(hb.ensure((size_t)rows * in8 * 2));
          CHK(cast_transpose(H_prev, in_dim, rows, in_dim, hb.as<__bf16>(), in8, nullptr, 0, nullptr, false, &colp, s));
          g.act = act_prev; g.H = hb.as<__bf16>(); g.ldh = in8; g.drop = buffer_spec(keep_mask_prev, p_prev, in_dim);
        }
        CHK(launch_gemm_b16(g, 1, s));
      }
      if (dW) CHK(weight_grad_b16(dybt.as<__bf16>(), rows8, xbt.as<__bf16>(), rows8, rows, out_dim, in_dim, dW, db, false, slabs, s));
    }
    return GT_OK;
  };
  r = body();
  const hipError_t err = hipStreamSynchronize(s);      // on every path: the buffers are freed behind it
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "linear_bf16: %s", hipGetErrorString(err));
  return GT_OK;
}

// the dropout of a parity-hook case: none, the caller's Philox keys (as philox_site_spec) or the caller's mask
static DropoutSpec case_drop_spec(int mode, const float* mask, int ld_mask, float p, uint32_t key0, uint32_t key1) {
  DropoutSpec drop = no_drop();
  if (mode == DROP_BUFFER) {
    drop = buffer_spec(mask, p, ld_mask);
  } else if (mode == DROP_PHILOX) {
    drop.mode = DROP_PHILOX; drop.p = p; drop.scale = 1.f / (1.f - p);
    const double th = (double)p * 65536.0 + 0.5;
    drop.thresh = th >= 65535.0 ? 65535u : (uint32_t)th;
    drop.key0 = key0; drop.key1 = key1;
  }
  return drop;
}

// One product of the float32 MFMA family through the engine's own dispatch (linear_forward / launch_gemm / linear_backward_data /
// linear_backward_weight / linear_backward_weight_split): parity hook of tests/test_gpu_gemm_f32.py.  The added-matrix and two-segment
// forward of the split first layer go through the builders the engine's stack_forward calls (linear_forward, linear_forward_seg).
extern "C" int gt_op_gemm_f32(const gt_gemm_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (c->route < GT_GEMM_ROUTE_FORWARD || c->route > GT_GEMM_ROUTE_WEIGHT_GRAD_SPLIT) return fail(GT_ERR_INVALID, "unknown route %d", c->route);
  if (c->prec != 0 && c->prec != 1) return fail(GT_ERR_INVALID, "prec must be 0 (float32) or 1 (bf16)");
  if (c->rows < 1 || c->in_dim < 1 || c->out_dim < 1) return fail(GT_ERR_INVALID, "bad sizes");
  if (c->act < ACT_NONE || c->act > ACT_SIGMOID || c->drop < DROP_NONE || c->drop > DROP_BUFFER) return fail(GT_ERR_INVALID, "unknown activation / dropout");
  if (c->drop != DROP_NONE && (c->act != ACT_LEAKY_DROPOUT || !(c->p > 0.f && c->p < 1.f) || (c->drop == DROP_BUFFER && !c->mask)))
    return fail(GT_ERR_INVALID, "dropout needs act 1, 0 < p < 1 and (buffer) a mask");
  const int route = c->route;
  const bool seg = route == GT_GEMM_ROUTE_FORWARD_SEG, split = route == GT_GEMM_ROUTE_WEIGHT_GRAD_SPLIT;
  const bool wgrad = route == GT_GEMM_ROUTE_WEIGHT_GRAD || split;
  const bool data = route == GT_GEMM_ROUTE_BACKWARD_DATA || (wgrad && c->rider);
  if ((seg || split) && (c->rows != c->wrap && c->rows != 2L * c->wrap)) return fail(GT_ERR_INVALID, "rows must be wrap or 2 wrap");
  if ((seg || split) && (c->cd < 1 || c->cd >= c->in_dim || !c->x || !c->adv)) return fail(GT_ERR_INVALID, "split layer needs x, adv and 0 < cd < in_dim");
  if ((route == GT_GEMM_ROUTE_FORWARD || seg) && (!c->x || !c->w || !c->y)) return fail(GT_ERR_INVALID, "forward needs x, w and y");
  if (route == GT_GEMM_ROUTE_FORWARD && c->addm && (c->wrap < 1 || c->rows > 2L * c->wrap)) return fail(GT_ERR_INVALID, "added matrix needs rows <= 2 wrap");
  if (data && (!c->dy || !c->w || !c->dx || c->col0 < 0 || c->ncols < 1 || (long)c->col0 + c->ncols > c->in_dim))
    return fail(GT_ERR_INVALID, "backward-data needs dy, w, dx and col0 + ncols <= in_dim");
  if (data && c->act != ACT_NONE && !c->h) return fail(GT_ERR_INVALID, "activation derivative without h");
  if (wgrad && (!c->dy || (!c->dw && !c->db) || (c->dw && !c->x) || (split && !c->dw))) return fail(GT_ERR_INVALID, "weight gradient needs dy, x and dw / db");
  hipStream_t s = (hipStream_t)stream;
  const DropoutSpec drop = case_drop_spec(c->drop, c->mask, c->ld_mask, c->p, c->key0, c->key1);
  Scratch slabs, colp;
  SlabDefer sd;
  sd.active = c->defer != 0;
  const int prec = c->prec ? PREC_BF16 : PREC_F32;
  auto body = [&]() -> int {
    if (route == GT_GEMM_ROUTE_FORWARD)
      return linear_forward(c->x, c->ldx, c->w, c->ldw, c->bias, c->y, c->ldy, c->rows, c->in_dim, c->out_dim, c->act, drop, prec, s, c->addm,
                            c->ld_addm, c->wrap, c->accumulate != 0);
    if (seg)
      return linear_forward_seg(c->x, c->ldx, c->wrap, c->cd, c->adv, c->ld_adv, c->rows, c->w, c->ldw, c->in_dim, c->bias, c->y, c->ldy, c->out_dim,
                                c->act, drop, prec, s);
    if (route == GT_GEMM_ROUTE_BACKWARD_DATA) {
      GemmArgs g = backward_data_args(c->dy, c->ld_dy, c->w, c->ldw, c->col0, c->dx, c->ld_dx, c->rows, c->out_dim, c->ncols, c->act, c->h,
                                      c->ldh, drop);
      g.accumulate = c->accumulate ? 1 : 0;
      return launch_gemm(GEMM_NN, g, prec, s);
    }
    bool rode = false;
    const long row0 = split ? c->rows - c->wrap : 0;      // split: the rider reads the last half's rows (the generated rows of the D step)
    GemmArgs nn{};
    if (c->rider)
      nn = backward_data_args(c->dy + row0 * c->ld_dy, c->ld_dy, c->w, c->ldw, c->col0, c->dx, c->ld_dx, c->rows - row0, c->out_dim, c->ncols, c->act,
                              c->h, c->ldh, drop);
    if (!split) {
      CHK(linear_backward_weight(c->dy, c->ld_dy, c->x, c->ldx, c->rows, c->out_dim, c->in_dim, c->dw, c->db, c->accumulate != 0, slabs, colp, prec, s,
                                 &sd, c->rider ? &nn : nullptr, &rode));
    } else {
      CHK(linear_backward_weight_split(c->dy, c->ld_dy, c->rows, c->wrap, c->x, c->ldx, c->cd, c->adv, c->ld_adv, c->in_dim - c->cd, c->out_dim,
                                       c->dw, c->db, c->accumulate != 0, slabs, prec, s, &sd, c->rider ? &nn : nullptr, &rode));
    }
    if (c->rider && !rode) CHK(launch_gemm(GEMM_NN, nn, prec, s));
    return slab_defer_flush(sd, s);
  };
  const int r = body();
  const hipError_t err = hipStreamSynchronize(s);      // on every path: the buffers are freed behind it
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "gemm_f32: %s", hipGetErrorString(err));
  return GT_OK;
}

// One product of the bf16-storage family through the production dispatch (launch_gemm_b16 / weight_grad_b16): parity hook of
// tests/test_gpu_gemm_b16.py.  The operand images are built by cast_transpose into buffers filled with 0xFF bytes (bf16 NaN), so a
// loader that uses a pad element shows in the result.
extern "C" int gt_op_gemm_b16(const gt_gemm_b16_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  const int route = c->route;
  if (route != GT_GEMM_ROUTE_FORWARD && route != GT_GEMM_ROUTE_BACKWARD_DATA && route != GT_GEMM_ROUTE_WEIGHT_GRAD)
    return fail(GT_ERR_INVALID, "bf16 product hook: unknown route %d", route);
  if (c->rows < 1 || c->in_dim < 1 || c->out_dim < 1) return fail(GT_ERR_INVALID, "bf16 product hook: bad sizes");
  if (c->act < ACT_NONE || c->act > ACT_SIGMOID || c->drop < DROP_NONE || c->drop > DROP_BUFFER)
    return fail(GT_ERR_INVALID, "bf16 product hook: unknown activation / dropout");
  if (c->drop != DROP_NONE && (c->act != ACT_LEAKY_DROPOUT || !(c->p > 0.f && c->p < 1.f) || (c->drop == DROP_BUFFER && !c->mask)))
    return fail(GT_ERR_INVALID, "bf16 product hook: dropout needs act 1, 0 < p < 1 and (buffer) a mask");
  const bool wg = route == GT_GEMM_ROUTE_WEIGHT_GRAD, fwd = route == GT_GEMM_ROUTE_FORWARD;
  const int M = c->rows, N = fwd ? c->out_dim : c->in_dim;
  for (const void* q : {(const void*)c->x, (const void*)c->w, (const void*)c->bias, (const void*)c->dy, (const void*)c->h, (const void*)c->mask,
                        (const void*)c->c, (const void*)c->dw, (const void*)c->db})
    if (((uintptr_t)q) & 3) return fail(GT_ERR_INVALID, "bf16 product hook: misaligned float32 operand");
  if (fwd && (!c->x || !c->w || c->ldx < c->in_dim || c->ldw < c->in_dim)) return fail(GT_ERR_INVALID, "bf16 product hook: forward needs x and w");
  if (route == GT_GEMM_ROUTE_BACKWARD_DATA && (!c->dy || !c->w || c->ld_dy < c->out_dim || c->ldw < c->in_dim))
    return fail(GT_ERR_INVALID, "bf16 product hook: backward-data needs dy and w");
  if (route == GT_GEMM_ROUTE_BACKWARD_DATA && c->act != ACT_NONE && (!c->h || c->ldh < c->in_dim))
    return fail(GT_ERR_INVALID, "bf16 product hook: activation derivative without h");
  if (wg && (!c->dy || !c->x || !c->dw || c->ld_dy < c->out_dim || c->ldx < c->in_dim || c->act != ACT_NONE))
    return fail(GT_ERR_INVALID, "bf16 product hook: weight gradient needs dy, x and dw, and no activation");
  if (c->drop == DROP_BUFFER && c->ld_mask < N) return fail(GT_ERR_INVALID, "bf16 product hook: mask pitch");
  if (!wg) {
    if (!c->c && !c->cb && !c->cbt) return fail(GT_ERR_INVALID, "bf16 product hook: no result requested");
    if ((c->c && c->ldc < N) || (c->cb && c->ldcb < N) || (c->cbt && c->ldcbt < M)) return fail(GT_ERR_INVALID, "bf16 product hook: result pitch");
    if (((uintptr_t)c->cb) & 1) return fail(GT_ERR_INVALID, "bf16 product hook: misaligned bf16 result");
    if (c->cbt && ((c->ldcbt & 3) || (((uintptr_t)c->cbt) & 7)))
      return fail(GT_ERR_INVALID, "bf16 product hook: transposed result must be 8-byte aligned with a pitch that is a multiple of 4");
    if (c->accumulate && !c->c) return fail(GT_ERR_INVALID, "bf16 product hook: accumulate needs the float32 result");
  }
  hipStream_t s = (hipStream_t)stream;
  const int in8 = pad8(c->in_dim), out8 = pad8(c->out_dim);
  const long rows8 = pad8((long)c->rows);
  Scratch ab, bb, hb, slabs, colp;
  auto poisoned = [&](Scratch& q, size_t bytes) -> int {
    CHK(q.ensure(bytes));
    HIPCHK(hipMemsetAsync(q.p, 0xFF, bytes, s));
    return GT_OK;
  };
  auto body = [&]() -> int {
    __bf16* const none = nullptr;
    if (wg) {      // dZT [out][rows8], XT [in][rows8]
      CHK(poisoned(ab, (size_t)c->out_dim * rows8 * 2)); CHK(poisoned(bb, (size_t)c->in_dim * rows8 * 2));
      CHK(cast_transpose(c->dy, c->ld_dy, c->rows, c->out_dim, none, 0, ab.as<__bf16>(), rows8, nullptr, false, &colp, s));
      CHK(cast_transpose(c->x, c->ldx, c->rows, c->in_dim, none, 0, bb.as<__bf16>(), rows8, nullptr, false, &colp, s));
      return weight_grad_b16(ab.as<__bf16>(), rows8, bb.as<__bf16>(), rows8, c->rows, c->out_dim, c->in_dim, c->dw, c->db, c->accumulate != 0, slabs, s);
    }
    GemmB16Args g = b16_args();
    if (fwd) {     // X [rows][in8], W [out][in8]
      CHK(poisoned(ab, (size_t)c->rows * in8 * 2)); CHK(poisoned(bb, (size_t)c->out_dim * in8 * 2));
      CHK(cast_transpose(c->x, c->ldx, c->rows, c->in_dim, ab.as<__bf16>(), in8, none, 0, nullptr, false, &colp, s));
      CHK(cast_transpose(c->w, c->ldw, c->out_dim, c->in_dim, bb.as<__bf16>(), in8, none, 0, nullptr, false, &colp, s));
      g.lda = g.ldb = in8; g.K = c->in_dim; g.bias = c->bias; g.epi = B16_FWD;
    } else {       // dZ [rows][out8], WT [in][out8], H [rows][in8]
      CHK(poisoned(ab, (size_t)c->rows * out8 * 2)); CHK(poisoned(bb, (size_t)c->in_dim * out8 * 2));
      CHK(cast_transpose(c->dy, c->ld_dy, c->rows, c->out_dim, ab.as<__bf16>(), out8, none, 0, nullptr, false, &colp, s));
      CHK(cast_transpose(c->w, c->ldw, c->out_dim, c->in_dim, none, 0, bb.as<__bf16>(), out8, nullptr, false, &colp, s));
      g.lda = g.ldb = out8; g.K = c->out_dim; g.epi = B16_BWD_DATA;
      if (c->act != ACT_NONE) {
        CHK(poisoned(hb, (size_t)c->rows * in8 * 2));
        CHK(cast_transpose(c->h, c->ldh, c->rows, c->in_dim, hb.as<__bf16>(), in8, none, 0, nullptr, false, &colp, s));
        g.H = hb.as<__bf16>(); g.ldh = in8;
      }
    }
    g.A = ab.as<__bf16>(); g.B = bb.as<__bf16>(); g.M = M; g.N = N;
    g.C = c->c; g.ldc = c->ldc; g.Cb = (__bf16*)c->cb; g.ldcb = c->ldcb; g.CbT = (__bf16*)c->cbt; g.ldcbt = c->ldcbt;
    g.act = c->act; g.accumulate = c->accumulate ? 1 : 0;
    g.drop = case_drop_spec(c->drop, c->mask, c->ld_mask, c->p, c->key0, c->key1);
    return launch_gemm_b16(g, 1, s);
  };
  const int r = body();
  const hipError_t err = hipStreamSynchronize(s);      // on every path: the buffers are freed behind it
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "gemm_b16: %s", hipGetErrorString(err));
  return GT_OK;
}

// One image builder of the bf16-storage family through the engine's launch code: parity hook of tests/test_gpu_gemm_b16.py.
extern "C" int gt_op_cast_image(const gt_cast_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (c->kind < GT_CAST_PLAIN_F32 || c->kind > GT_CAST_MULTI) return fail(GT_ERR_INVALID, "cast hook: unknown kind %d", c->kind);
  hipStream_t s = (hipStream_t)stream;
  if (c->kind == GT_CAST_MULTI) {
    if (c->n_jobs < 1 || c->n_jobs > CAST_MAX_JOBS) return fail(GT_ERR_INVALID, "cast hook: 1 .. %d jobs", CAST_MAX_JOBS);
    CastJobs jobs;
    jobs.n = 0; jobs.pad_ = 0;
    int blocks = 0;
    for (int i = 0; i < c->n_jobs; ++i) {
      const gt_cast_job& j = c->jobs[i];
      if (!j.in || (!j.out && !j.outT) || j.rows < 1 || j.cols < 1 || j.ldi < j.cols || (j.out && j.ldo < j.cols) || (j.outT && j.ldt < j.rows))
        return fail(GT_ERR_INVALID, "cast hook: bad job %d", i);
      if ((((uintptr_t)j.in) & 3) || (((uintptr_t)j.out) & 1) || (((uintptr_t)j.outT) & 1)) return fail(GT_ERR_INVALID, "cast hook: misaligned job %d", i);
      CHK(cast_jobs_add(jobs, blocks, j.in, j.ldi, j.rows, j.cols, (__bf16*)j.out, j.ldo, (__bf16*)j.outT, j.ldt));
    }
    CHK(cast_transpose_multi(jobs, blocks, s));
    HIPCHK(hipStreamSynchronize(s));
    return GT_OK;
  }
  if (c->rows < 1 || c->cols < 1 || (!c->out && !c->outT) || (c->out && c->ldo < c->cols) || (c->outT && c->ldt < c->rows))
    return fail(GT_ERR_INVALID, "cast hook: bad sizes");
  if ((((uintptr_t)c->out) & 1) || (((uintptr_t)c->outT) & 1)) return fail(GT_ERR_INVALID, "cast hook: misaligned image");
  const bool cat = c->kind == GT_CAST_CAT || c->kind == GT_CAST_CATDROP, drop = c->kind == GT_CAST_SEQDROP || c->kind == GT_CAST_CATDROP;
  if (!cat && (!c->in || c->ldi < c->cols || (((uintptr_t)c->in) & (c->kind == GT_CAST_PLAIN_BF16 ? 1 : 3))))
    return fail(GT_ERR_INVALID, "cast hook: bad source");
  if (c->colsum && c->kind != GT_CAST_PLAIN_F32) return fail(GT_ERR_INVALID, "cast hook: column sums ride with the float32 source only");
  if (drop && (!c->mul || c->T < 1)) return fail(GT_ERR_INVALID, "cast hook: dropout needs mul and T");
  if (cat && (c->cd < 0 || c->cd > c->cols || (c->cd > 0 && !c->x) || (c->cd < c->cols && (!c->idx || !c->fa || !c->fb || c->ldf < 1)) || c->N < 1 ||
              c->row_off < 0 || c->row_off + c->rows > 2 * c->N))
    return fail(GT_ERR_INVALID, "cast hook: bad [x | feats[:, idx]] source");
  __bf16* out = (__bf16*)c->out;
  __bf16* outT = (__bf16*)c->outT;
  Scratch colp;
  int r = GT_OK;
  const CatSrc cs{c->x, c->cd, c->fa, c->fb, c->ldf, c->idx, (long)c->N, (long)c->row_off};
  switch (c->kind) {
    case GT_CAST_PLAIN_F32:
      r = cast_transpose((const float*)c->in, c->ldi, c->rows, c->cols, out, c->ldo, outT, c->ldt, c->colsum, c->colsum_accumulate != 0, &colp, s);
      break;
    case GT_CAST_PLAIN_BF16:
      r = cast_transpose((const __bf16*)c->in, c->ldi, c->rows, c->cols, out, c->ldo, outT, c->ldt, nullptr, false, &colp, s);
      break;
    case GT_CAST_SEQDROP: {
      const SeqDropSrc src{(const float*)c->in, c->ldi, c->mul, c->T, c->cols};
      r = seqdrop_cast_transpose(src, c->rows, c->cols, out, c->ldo, outT, c->ldt, s);
      break;
    }
    case GT_CAST_CAT: r = cat_cast_transpose(cs, c->rows, c->cols, out, c->ldo, outT, c->ldt, s); break;
    default: {
      const CatDropSrc src{cs, c->mul, c->T, c->cols};
      r = catdrop_cast_transpose(src, c->rows, c->cols, out, c->ldo, outT, c->ldt, s);
    }
  }
  const hipError_t err = hipStreamSynchronize(s);
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "cast_image: %s", hipGetErrorString(err));
  return GT_OK;
}

// One SRU scan launch through the stacks' launch functions (sru_launch_fwd / _bwd, eng_sru.hip): parity hook of
// tests/test_gpu_sru_scan.py.  Everything a kernel would index with is checked first: no case reaches a launch it could fault in.
extern "C" int gt_op_sru_scan(const gt_sru_scan_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (c->B < 1 || c->T < 1 || c->H < 1 || (c->dirs != 1 && c->dirs != 2)) return fail(GT_ERR_INVALID, "SRU scan hook: bad sizes");
  if (c->k != 3 && c->k != 4) return fail(GT_ERR_INVALID, "SRU scan hook: k = %d (3 or 4)", c->k);
  if (c->act < SRU_ID || c->act > SRU_RELU || c->mask_mode < 0 || c->mask_mode > 2) return fail(GT_ERR_INVALID, "SRU scan hook: unknown activation / mask mode");
  const long ncols = (long)c->H * c->dirs, N = (long)c->B * c->T;
  if (ncols * c->k > 0x7FFFFFFFL || N > 0x7FFFFFFFL) return fail(GT_ERR_INVALID, "SRU scan hook: sizes beyond the kernels' int indices");
  const bool bwd = c->backward != 0;
  for (const void* q : {(const void*)c->U, (const void*)c->x, (const void*)c->bias, (const void*)c->h, (const void*)c->c, (const void*)c->dh,
                        (const void*)c->dU, (const void*)c->dx, (const void*)c->dbias_part, (const void*)c->mask, (const void*)c->up_mul,
                        (const void*)c->up_add, (const void*)c->nx_mul})
    if (((uintptr_t)q) & 3) return fail(GT_ERR_INVALID, "SRU scan hook: misaligned float32 operand");
  if (!c->U || !c->bias || !c->c || c->ldu < ncols * c->k) return fail(GT_ERR_INVALID, "SRU scan hook: needs U (ldu >= ncols * k), bias and c");
  if (c->k == 3 && (!c->x || c->ldx < ncols)) return fail(GT_ERR_INVALID, "SRU scan hook: k = 3 needs x with ldx >= ncols");
  if (c->mask_mode == 1 && !c->mask) return fail(GT_ERR_INVALID, "SRU scan hook: mask mode 1 without a mask");
  if (c->mask_mode == 2 && !(c->p > 0.f && c->p < 1.f)) return fail(GT_ERR_INVALID, "SRU scan hook: Philox mask needs 0 < p < 1");
  const int waves = sru_scan_waves(c->B, (int)ncols);
  auto image_ok = [&](const uint16_t* r, long ldr, long wr, const uint16_t* t, long ldt) {
    return waves != 0 && c->T % 8 == 0 && c->H % 64 == 0 && r && !(((uintptr_t)r) & 15) && !(((uintptr_t)t) & 15) && ldr >= wr && ldr % 8 == 0 &&
           ldr <= 0x7FFFFFFFL && (!t || (ldt >= N && ldt % 8 == 0));
  };
  if (!bwd) {
    if (!c->h) return fail(GT_ERR_INVALID, "SRU scan hook: forward needs h");
    if (c->dU_b || c->dU_bt) return fail(GT_ERR_INVALID, "SRU scan hook: dU images belong to the backward scan");
    if ((c->nx_b || c->nx_bt) && !image_ok(c->nx_b, c->ld_nxb, ncols, c->nx_bt, c->ld_nxbt))
      return fail(GT_ERR_INVALID, "SRU scan hook: forward images need a cooperative form, T %% 8 == 0, H %% 64 == 0, 16-byte aligned buffers and pitches");
  } else {
    if (!c->dh || !c->dbias_part) return fail(GT_ERR_INVALID, "SRU scan hook: backward needs dh and dbias_part");
    if (c->nx_b || c->nx_bt) return fail(GT_ERR_INVALID, "SRU scan hook: nx images belong to the forward scan");
    if (c->k == 3 && (!c->dx || c->lddx < ncols)) return fail(GT_ERR_INVALID, "SRU scan hook: k = 3 needs dx with lddx >= ncols");
    if (c->up_add && c->ld_up_add < ncols) return fail(GT_ERR_INVALID, "SRU scan hook: up_add pitch");
    if ((c->dU_b || c->dU_bt) && !image_ok(c->dU_b, c->ld_dub, ncols * c->k, c->dU_bt, c->ld_dubt))
      return fail(GT_ERR_INVALID, "SRU scan hook: dU images need a cooperative form, T %% 8 == 0, H %% 64 == 0, 16-byte aligned buffers and pitches");
    if (!c->dU_b && !c->dU) return fail(GT_ERR_INVALID, "SRU scan hook: backward needs dU or its images");
  }
  hipStream_t s = (hipStream_t)stream;
  SruArgs a;
  memset(&a, 0, sizeof(a));
  a.B = c->B; a.T = c->T; a.H = c->H; a.dirs = c->dirs; a.k = c->k; a.act = c->act;
  a.U = c->U; a.ldu = c->ldu; a.x = c->x; a.ldx = c->ldx; a.bias = c->bias; a.h = c->h; a.c = c->c;
  a.seq_mul = c->seq_mul; a.seq_add = c->seq_add;
  if (c->mask_mode == 1) { a.use_mask = 1; a.keep_scale = c->keep_scale; a.mask_buf = c->mask; }
  if (c->mask_mode == 2) { a.use_mask = 1; a.keep_scale = 1.f / (1.f - c->p); a.thresh = sru_drop_thresh(c->p); a.key0 = c->key0; a.key1 = c->key1; }
  int r;
  if (!bwd) {
    if (c->nx_b) { a.nx_b = (__bf16*)c->nx_b; a.ld_nxb = c->ld_nxb; a.nx_bt = (__bf16*)c->nx_bt; a.ld_nxbt = (long)c->ld_nxbt; a.nx_mul = c->nx_mul; }
    r = sru_launch_fwd(a, s);
  } else {
    a.dh = c->dh; a.dU = c->dU_b ? nullptr : c->dU; a.dx = c->k == 3 ? c->dx : nullptr; a.lddx = c->lddx; a.dbias_part = c->dbias_part;
    a.up_mul = c->up_mul; a.up_add = c->up_add; a.ld_up_add = c->ld_up_add;
    if (c->dU_b) { a.dU_b = (__bf16*)c->dU_b; a.ld_dub = c->ld_dub; a.dU_bt = (__bf16*)c->dU_bt; a.ld_dubt = (long)c->ld_dubt; }
    r = sru_launch_bwd(a, s);
  }
  const hipError_t err = hipStreamSynchronize(s);
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "sru_scan: %s", hipGetErrorString(err));
  return GT_OK;
}

// The three helper kernels of the SRU stack, each through the engine's launch function: parity hooks of tests/test_gpu_sru_scan.py.
extern "C" int gt_op_sru_dx_adv_finish(float* dx_adv, int64_t rows, int Da, int T, const float* mul, int ld_mul, const float* hw, int ld_hw,
                                       void* stream) {
  if (!dx_adv || rows < 1 || Da < 1 || T < 1 || rows % T) return fail(GT_ERR_INVALID, "dx finish hook: needs dx_adv and rows = sequences x T");
  if ((((uintptr_t)dx_adv) | ((uintptr_t)mul) | ((uintptr_t)hw)) & 3) return fail(GT_ERR_INVALID, "dx finish hook: misaligned float32 operand");
  if ((mul && ld_mul < Da) || (hw && ld_hw < Da)) return fail(GT_ERR_INVALID, "dx finish hook: operand pitch below Da");
  if (rows * Da > 0x7FFFFFFFL * 256) return fail(GT_ERR_INVALID, "dx finish hook: too many elements for one launch");
  hipStream_t s = (hipStream_t)stream;
  SruDxAdvArgs f;
  f.dx_adv = dx_adv; f.rows = (long)rows; f.Da = Da; f.T = T; f.mul = mul; f.ld_mul = ld_mul; f.hw = hw; f.ld_hw = ld_hw;
  CHK(sru_launch_dx_adv_finish(f, s));
  HIPCHK(hipStreamSynchronize(s));
  return GT_OK;
}
extern "C" int gt_op_sru_input_mask(float* mul, int B, int n, float p, uint32_t key0, uint32_t key1, const float* inj, int seq_mul, int seq_add,
                                    void* stream) {
  if (!mul || B < 1 || n < 1 || (long)B * n > 0x7FFFFFFFL - 256) return fail(GT_ERR_INVALID, "input mask hook: bad sizes");
  if (!(p > 0.f && p < 1.f)) return fail(GT_ERR_INVALID, "input mask hook: needs 0 < p < 1");
  if ((((uintptr_t)mul) | ((uintptr_t)inj)) & 3) return fail(GT_ERR_INVALID, "input mask hook: misaligned float32 operand");
  hipStream_t s = (hipStream_t)stream;
  CHK(sru_launch_input_mask(mul, B, n, 1.f / (1.f - p), sru_drop_thresh(p), key0, key1, inj, seq_mul, seq_add, s));
  HIPCHK(hipStreamSynchronize(s));
  return GT_OK;
}
extern "C" int gt_op_sru_input_dropout(const float* x, int ldx, float* y, int ldy, int B, int T, int n, const float* mul, void* stream) {
  if (!x || !y || !mul || B < 1 || T < 1 || n < 1 || ldx < n || ldy < n) return fail(GT_ERR_INVALID, "input dropout hook: bad argument");
  if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)mul)) & 3) return fail(GT_ERR_INVALID, "input dropout hook: misaligned float32 operand");
  if ((long)B * T * n > 0x7FFFFFFFL * 256) return fail(GT_ERR_INVALID, "input dropout hook: too many elements for one launch");
  hipStream_t s = (hipStream_t)stream;
  CHK(sru_launch_input_dropout(x, ldx, y, ldy, B, T, n, mul, s));
  HIPCHK(hipStreamSynchronize(s));
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// parity hooks of the discriminator's tail (tests/test_gpu_d_tail.py): one head pass / one fused pass plus its finalising launch
// through launch_d_head / launch_dstack_pass (eng_step.hip).  Everything a kernel would index with is checked first.
// ------------------------------------------------------------------------------------------
static bool tail_site_ok(const gt_drop_site& d, int width, long rows, bool exact_pitch, const char** why) {
  *why = nullptr;
  if (d.mode < DROP_NONE || d.mode > DROP_BUFFER) *why = "unknown dropout mode";
  else if (d.mode != DROP_NONE && !(d.p > 0.f && d.p < 1.f)) *why = "dropout needs 0 < p < 1";
  else if (d.mode == DROP_BUFFER && (!d.mask || (((uintptr_t)d.mask) & 3))) *why = "injected dropout mask missing or misaligned";
  else if (d.mode == DROP_BUFFER && (exact_pitch ? d.ld_mask != width : d.ld_mask < width)) *why = "injected dropout mask pitch";
  else if (d.mode == DROP_PHILOX && d.dp_t16 != 0u && (rows / 16 >= (1L << 21) || !(d.dp_inv_t16 > 0.f))) *why = "data-parallel Philox map out of range";
  return *why == nullptr;
}
static DropoutSpec tail_site_spec(const gt_drop_site& d) {
  DropoutSpec s = case_drop_spec(d.mode, d.mask, d.ld_mask, d.p, d.key0, d.key1);
  if (d.mode == DROP_PHILOX) {
    s.dp_t16 = d.dp_t16; s.dp_nl16 = d.dp_nl16; s.dp_half = d.dp_half; s.dp_add = d.dp_add; s.dp_mul = d.dp_mul; s.dp_inv_t16 = d.dp_inv_t16;
  }
  return s;
}
// the scratch of one tail hook call: the step's scalars and the partial buffers, all NaN (0xFF bytes) until something writes them
struct TailScratch {
  Scratch mem;
  StepScalars* sc = nullptr;
  HeadSums o;
  float tv_host[2];
  int init(int nblk, int K, int has_tv, float tv, float* dW, float* db, int accumulate, hipStream_t s) {
    const size_t off_hp = 256, off_dw = off_hp + (((size_t)nblk * sizeof(HeadPartials) + 255) & ~(size_t)255);
    const size_t total = off_dw + (size_t)nblk * K * sizeof(float);
    static_assert(sizeof(StepScalars) <= 256, "scratch layout");
    CHK(mem.ensure(total));
    HIPCHK(hipMemsetAsync(mem.p, 0xFF, total, s));
    sc = (StepScalars*)mem.p;
    if (has_tv) {
      tv_host[0] = tv; tv_host[1] = 1.0f / tv;
      HIPCHK(hipMemcpyAsync(mem.p, tv_host, sizeof(tv_host), hipMemcpyHostToDevice, s));      // StepScalars: tv, inv_tv lead
    }
    memset(&o, 0, sizeof(o));
    o.sc = sc;
    o.hp = (HeadPartials*)((char*)mem.p + off_hp); o.hp_cap = nblk;
    o.dw_partial = (float*)((char*)mem.p + off_dw); o.dw_cap = (long)nblk * K;
    o.dW = dW; o.db = db; o.accumulate = accumulate;
    return GT_OK;
  }
  // synchronises and reports the scalars (the memory goes with the object, behind that); r: the launch function's status
  int finish(int r, int nblk, double* scalars, const char* what, hipStream_t s) {
    hipError_t err = hipStreamSynchronize(s);
    StepScalars h;
    if (err == hipSuccess && r == GT_OK && scalars) {
      err = hipMemcpy(&h, sc, sizeof(h), hipMemcpyDeviceToHost);
      if (err == hipSuccess) {
        scalars[0] = h.s_real; scalars[1] = h.s_fake; scalars[2] = h.n_real_ok; scalars[3] = h.n_fake_ok; scalars[4] = h.s_adv;
        scalars[5] = (double)h.tv; scalars[6] = (double)h.inv_tv; scalars[7] = (double)nblk;
      }
    }
    if (r) return r;
    if (err != hipSuccess) return fail(GT_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
    return GT_OK;
  }
};
static_assert(offsetof(StepScalars, tv) == 0 && offsetof(StepScalars, inv_tv) == 4, "TailScratch::init writes tv, inv_tv at the front");

// mask, n_real, normaliser: what both tail hooks share
static const char* tail_common_bad(int mode, int64_t rows, int64_t n_real, int64_t n_mask, const float* mask, int has_tv, float tv,
                                   const double* tv_dev, int unit_tv) {
  if (mode != HEAD_D_STEP && mode != HEAD_G_ADV) return "mode 0 (D step) or 1 (adversarial term)";
  if (rows < 1 || rows > 0x7FFFFFFFL - 64) return "rows out of range";
  if (!mask || (((uintptr_t)mask) & 3) || n_mask < 1 || n_mask > 0x7FFFFFFFL) return "needs a mask and 1 <= n_mask";
  if (mode == HEAD_D_STEP && (n_real < 0 || n_real > rows)) return "0 <= n_real <= rows";
  const int given = (has_tv ? 1 : 0) + (tv_dev ? 1 : 0) + (unit_tv ? 1 : 0);
  if (given != 1) return "exactly one normaliser: has_tv, tv_dev or unit_tv";
  if (has_tv && !(tv > 0.f)) return "tv must be positive";
  if (((uintptr_t)tv_dev) & 7) return "misaligned tv_dev";
  return nullptr;
}

extern "C" int gt_op_d_head(const gt_d_head_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (const char* why = tail_common_bad(c->mode, c->rows, c->n_real, c->n_mask, c->mask, c->has_tv, c->tv, c->tv_dev, c->unit_tv))
    return fail(GT_ERR_INVALID, "head hook: %s", why);
  if (c->objective < 0 || c->objective >= GAN_OBJ_COUNT) return fail(GT_ERR_INVALID, "head hook: objective = %d (0 bce, 1 ls, 2 hinge, 3 wgan, 4 kl, 5 rkl, 6 js)", c->objective);
  if (c->K < 1 || c->K > 1024) return fail(GT_ERR_INVALID, "head hook: K = %d (1 .. 1024)", c->K);
  if (!c->H || !c->w || !c->bias) return fail(GT_ERR_INVALID, "head hook: needs H, w and bias");
  const bool img = c->h_ld > 0;
  if (c->h_ld < 0 || (img ? c->h_ld < c->K : c->ldh < c->K)) return fail(GT_ERR_INVALID, "head hook: pitch of H below K");
  if ((((uintptr_t)c->H) & (img ? 1 : 3)) || ((((uintptr_t)c->w) | ((uintptr_t)c->bias) | ((uintptr_t)c->Dout) | ((uintptr_t)c->dH) | ((uintptr_t)c->dW) |
                                                 ((uintptr_t)c->db)) & 3))
    return fail(GT_ERR_INVALID, "head hook: misaligned operand");
  const char* why;
  if (!tail_site_ok(c->drop, c->K, c->rows, false, &why)) return fail(GT_ERR_INVALID, "head hook: %s", why);
  if (c->drop.mode != DROP_NONE && !c->has_act) return fail(GT_ERR_INVALID, "head hook: a dropout site needs has_act");
  if (c->dH && c->lddh < c->K) return fail(GT_ERR_INVALID, "head hook: pitch of dH below K");
  if ((c->dHb || c->dHbT) && !img) return fail(GT_ERR_INVALID, "head hook: bf16 results belong to the image form (h_ld > 0)");
  if (c->dHb && ((((uintptr_t)c->dHb) & 1) || c->lddhb < c->K)) return fail(GT_ERR_INVALID, "head hook: dHb misaligned or its pitch below K");
  if (c->dHbT && ((((uintptr_t)c->dHbT) & 7) || c->lddhbt % 4 != 0 || c->lddhbt < c->rows))
    return fail(GT_ERR_INVALID, "head hook: dHbT needs 8-byte alignment and a pitch >= rows that is a multiple of 4");
  const bool w = c->want_grad && c->want_w;
  if (w && (!c->dW || !c->db)) return fail(GT_ERR_INVALID, "head hook: weight gradients need dW and db");
  hipStream_t s = (hipStream_t)stream;
  const int nblk = d_head_blocks((long)c->rows);
  TailScratch t;
  int r = t.init(nblk, c->K, c->has_tv, c->tv, c->dW, c->db, c->accumulate ? 1 : 0, s);
  int deferred = -1;
  if (r == GT_OK) {
    HeadArgs h;
    memset(&h, 0, sizeof(h));
    h.c.mode = c->mode; h.c.rows = (long)c->rows; h.c.n_real = (long)c->n_real; h.c.mask = c->mask; h.c.n_mask = (long)c->n_mask; h.c.eps = c->eps;
    h.c.want_grad = c->want_grad != 0; h.c.want_w = c->want_w != 0; h.c.defer_scalars = c->defer_scalars ? &deferred : nullptr;
    h.c.tv_dev = c->tv_dev; h.c.unit_tv = c->unit_tv != 0; h.c.objective = c->objective;
    h.o = t.o;
    h.H = c->H; h.K = c->K; h.ldh = c->ldh; h.h_ld = c->h_ld; h.has_act = c->has_act != 0; h.spec = tail_site_spec(c->drop);
    h.w = c->w; h.bias = c->bias; h.Dout = c->Dout; h.dH = c->dH; h.lddh = c->lddh;
    h.dHb = (__bf16*)c->dHb; h.lddhb = c->lddhb; h.dHbT = (__bf16*)c->dHbT; h.lddhbt = (long)c->lddhbt;
    r = launch_d_head(h, s);
  }
  return t.finish(r, deferred >= 0 ? deferred : nblk, c->scalars, "d_head", s);
}

extern "C" int gt_op_dstack(const gt_dstack_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (const char* why = tail_common_bad(c->mode, c->rows, c->n_real, c->n_mask, c->mask, c->has_tv, c->tv, c->tv_dev, c->unit_tv))
    return fail(GT_ERR_INVALID, "fused stack hook: %s", why);
  if (c->objective < 0 || c->objective >= GAN_OBJ_COUNT) return fail(GT_ERR_INVALID, "fused stack hook: objective = %d (0 bce, 1 ls, 2 hinge, 3 wgan, 4 kl, 5 rkl, 6 js)", c->objective);
  if (c->L < 1 || c->L > DS_MAXL) return fail(GT_ERR_INVALID, "fused stack hook: L = %d (1 .. %d)", c->L, DS_MAXL);
  if (!dstack_hidden_ok(c->hidden_dim)) return fail(GT_ERR_INVALID, "fused stack hook: hidden_dim 128 or 256");
  const int H = c->hidden_dim;
  const bool g_mode = c->mode == HEAD_G_ADV, grad = c->want_grad != 0;
  uintptr_t bits = ((uintptr_t)c->H0) | ((uintptr_t)c->w_last) | ((uintptr_t)c->b_last) | ((uintptr_t)c->dZtop) | ((uintptr_t)c->Dout) |
                   ((uintptr_t)c->dW_last) | ((uintptr_t)c->db_last) | ((uintptr_t)c->W0) | ((uintptr_t)c->gadv);
  if (!c->H0 || !c->w_last || !c->b_last) return fail(GT_ERR_INVALID, "fused stack hook: needs H0, w_last and b_last");
  for (int l = 0; l < c->L; ++l) {
    if (l > 0 && (!c->W[l] || !c->b[l])) return fail(GT_ERR_INVALID, "fused stack hook: layer %d needs W and b", l);
    bits |= ((uintptr_t)c->W[l]) | ((uintptr_t)c->b[l]) | ((uintptr_t)c->Hout[l]);
    const char* why;
    if (!tail_site_ok(c->drop[l], H, c->rows, true, &why)) return fail(GT_ERR_INVALID, "fused stack hook: layer %d: %s", l, why);
  }
  if (bits & 3) return fail(GT_ERR_INVALID, "fused stack hook: misaligned float32 operand");
  if (!g_mode && grad && (!c->dZtop || !c->dW_last || !c->db_last)) return fail(GT_ERR_INVALID, "fused stack hook: the D step's gradients need dZtop, dW_last and db_last");
  if (g_mode && grad) {
    if (c->Da < 1 || c->Da > 64) return fail(GT_ERR_INVALID, "fused stack hook: Da = %d (1 .. 64)", c->Da);
    if (!c->W0 || !c->gadv || c->col0 < 0 || (long)c->col0 + c->Da > c->ldw0 || c->ld_gadv < c->Da)
      return fail(GT_ERR_INVALID, "fused stack hook: the G step's gradient needs W0 (col0 + Da <= ldw0) and gadv (ld_gadv >= Da)");
  }
  hipStream_t s = (hipStream_t)stream;
  const int nblk = dstack_panels((long)c->rows);
  TailScratch t;
  int r = t.init(nblk, H, c->has_tv, c->tv, c->dW_last, c->db_last, c->accumulate ? 1 : 0, s);
  if (r == GT_OK) {
    DStackCall k;
    memset(&k, 0, sizeof(k));
    k.c.mode = c->mode; k.c.rows = (long)c->rows; k.c.n_real = (long)c->n_real; k.c.mask = c->mask; k.c.n_mask = (long)c->n_mask; k.c.eps = c->eps;
    k.c.want_grad = grad; k.c.want_w = grad && !g_mode; k.c.tv_dev = c->tv_dev; k.c.unit_tv = c->unit_tv != 0; k.c.objective = c->objective;
    k.o = t.o; k.hidden_dim = H;
    DStackArgs& a = k.a;
    a.L = c->L; a.H0 = c->H0;
    for (int l = 0; l < c->L; ++l) { a.W[l] = c->W[l]; a.b[l] = c->b[l]; a.drop[l] = tail_site_spec(c->drop[l]); }
    a.w_last = c->w_last; a.b_last = c->b_last; a.Dout = c->Dout;
    if (!g_mode) {
      for (int l = 1; l < c->L; ++l) a.Hout[l] = c->Hout[l];
      a.dZtop = c->dZtop;
    } else {
      a.W0 = c->W0; a.ldw0 = c->ldw0; a.col0 = c->col0; a.Da = c->Da; a.gadv = c->gadv; a.ld_gadv = c->ld_gadv;
    }
    r = launch_dstack_pass(k, s);
  }
  return t.finish(r, nblk, c->scalars, "dstack", s);
}

// ------------------------------------------------------------------------------------------
// parity hook of the per-frame kernels between the products of a step (tests/test_gpu_frame_kernels.py): ONE launch function of
// frame_args.hip.h -- the functions the step itself calls -- on the caller's buffers.  Everything a kernel would index with is checked first.
// ------------------------------------------------------------------------------------------
static_assert(offsetof(StepScalars, tv_sum) == 8 && offsetof(StepScalars, gnorm2_g) == 80 && sizeof(StepScalars) == 88, "gt_op_frame: layout of `sums` / `scalars`");
static_assert(sizeof(StepResults) == 12 * sizeof(float), "gt_op_frame: layout of `scalars`");
static_assert(sizeof(HeadPartials) == 5 * sizeof(double), "gt_op_frame: hp is [n_hp][5] doubles");
static_assert(sizeof(gt_frame_case) == 320 && offsetof(gt_frame_case, tv) == 88 && offsetof(gt_frame_case, rows) == 112 && offsetof(gt_frame_case, drop) == 144 &&
              offsetof(gt_frame_case, a) == 200 && offsetof(gt_frame_case, scalars) == 312, "gt_frame_case: the layout tests/test_abi.py and gantts_amd/_lib.py state");

static bool frame_mat_ok(const void* p, long ld, long cols) { return p && !(((uintptr_t)p) & 3) && ld >= cols; }
// device int32 map -> host, every entry in [lo, hi)
static int frame_map_check(const int32_t* idx, int n, long lo, long hi, const char* what) {
  if (!idx || (((uintptr_t)idx) & 3) || n < 1) return fail(GT_ERR_INVALID, "frame hook: %s missing or misaligned", what);
  std::vector<int32_t> h((size_t)n);
  HIPCHK(hipMemcpy(h.data(), idx, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i)
    if (h[i] < lo || h[i] >= hi) return fail(GT_ERR_INVALID, "frame hook: %s[%d] = %d outside [%ld, %ld)", what, i, h[i], lo, hi);
  return GT_OK;
}

extern "C" int gt_op_frame(const gt_frame_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  const int op = c->op;
  if (op < GT_FRAME_MASK_SUM || op > GT_FRAME_TRANSPOSE) return fail(GT_ERR_INVALID, "frame hook: unknown op %d", op);
  hipStream_t s = (hipStream_t)stream;
  const int max_blocks = c->max_blocks ? c->max_blocks : FRAME_RED_MAX_BLOCKS;
  if (max_blocks < 1 || max_blocks > FRAME_RED_MAX_BLOCKS) return fail(GT_ERR_INVALID, "frame hook: max_blocks = %d (0, or 1 .. %d)", c->max_blocks, FRAME_RED_MAX_BLOCKS);
  const long rows = (long)c->rows, n_mask = (long)c->n_mask;
  const int cols = c->cols, cols2 = c->cols2;
  const bool reduction = op == GT_FRAME_SQERR || op == GT_FRAME_G_LOSSES || op == GT_FRAME_STATIC_GRAD;
  const bool finalizer = op == GT_FRAME_FINALIZE_G || op == GT_FRAME_FINALIZE_G_RIDER || op == GT_FRAME_FINALIZE_D;
  const bool mask_op = op == GT_FRAME_MASK_SUM || op == GT_FRAME_MASK_TOTAL;
  if (!finalizer && !mask_op) {
    if (rows < 1 || rows > 0x7FFFFFFFL - 64) return fail(GT_ERR_INVALID, "frame hook: rows out of range");
    if (cols < 1 || rows * cols > (1L << 36)) return fail(GT_ERR_INVALID, "frame hook: cols out of range");
  }
  // ---- the normaliser --------------------------------------------------------------------------
  const bool fin_rider = op == GT_FRAME_STATIC_GRAD && c->rider != 0;
  const bool needs_tv = (op == GT_FRAME_SQERR && c->out) || op == GT_FRAME_STATIC_GRAD || op == GT_FRAME_SCALE_INV_TV || op == GT_FRAME_FINALIZE_G ||
                        op == GT_FRAME_FINALIZE_G_RIDER || (op == GT_FRAME_FINALIZE_D && !c->tv_from_sum);
  const bool has_mask = c->mask != nullptr;
  if (has_mask && ((((uintptr_t)c->mask) & 3) || n_mask < 1 || n_mask > 0x7FFFFFFFL)) return fail(GT_ERR_INVALID, "frame hook: mask misaligned or n_mask out of range");
  if (((uintptr_t)c->tv_dev) & 7) return fail(GT_ERR_INVALID, "frame hook: misaligned tv_dev");
  if (c->has_tv && !(c->tv > 0.f)) return fail(GT_ERR_INVALID, "frame hook: tv must be positive");
  if (c->has_tv && c->tv_dev) return fail(GT_ERR_INVALID, "frame hook: has_tv and tv_dev exclude each other");
  if (reduction && (!has_mask || n_mask != rows)) return fail(GT_ERR_INVALID, "frame hook: a reduction needs a mask of n_mask == rows entries");
  if (mask_op && !has_mask) return fail(GT_ERR_INVALID, "frame hook: needs a mask");
  bool tv_from_mask = false;
  if (needs_tv) {
    if (!c->has_tv && !has_mask) return fail(GT_ERR_INVALID, "frame hook: needs a normaliser: has_tv, or a mask (with tv_override / tv_dev)");
    tv_from_mask = !c->has_tv;
  } else if (c->tv_dev && op != GT_FRAME_MASK_SUM) return fail(GT_ERR_INVALID, "frame hook: tv_dev is read by the mask sum only");
  // ---- per-op checks -----------------------------------------------------------------------------
  int n_part = 0, n1 = 0;
  if (op == GT_FRAME_SQERR) {
    if (!frame_mat_ok(c->a, c->lda, cols) || !frame_mat_ok(c->b, c->ldb, cols)) return fail(GT_ERR_INVALID, "frame hook: sqerr needs a and b with pitches >= cols");
    if (c->out && !frame_mat_ok(c->out, c->ldo, cols)) return fail(GT_ERR_INVALID, "frame hook: gradient misaligned or its pitch below cols");
    n_part = frame_red_blocks(rows * cols, max_blocks);
  } else if (op == GT_FRAME_G_LOSSES) {
    if (cols2 < 1 || rows * cols2 > (1L << 36)) return fail(GT_ERR_INVALID, "frame hook: cols2 out of range");
    if (!frame_mat_ok(c->a, c->lda, cols) || !frame_mat_ok(c->b, c->ldb, cols) || !frame_mat_ok(c->c, c->ldc, cols2) || !frame_mat_ok(c->d, c->ldd, cols2))
      return fail(GT_ERR_INVALID, "frame hook: g_losses needs a, b (cols) and c, d (cols2) with pitches >= their widths");
    n1 = frame_red_blocks(rows * cols, max_blocks);
    n_part = n1 + frame_red_blocks(rows * cols2, max_blocks);
  } else if (op == GT_FRAME_STATIC_GRAD) {
    if (!frame_mat_ok(c->a, c->lda, cols) || !frame_mat_ok(c->b, c->ldb, cols)) return fail(GT_ERR_INVALID, "frame hook: static_grad needs a and b with pitches >= cols");
    if (c->out && !frame_mat_ok(c->out, c->ldo, cols)) return fail(GT_ERR_INVALID, "frame hook: gs misaligned or its pitch below cols");
    if (c->idx) {
      if (cols2 < 1) return fail(GT_ERR_INVALID, "frame hook: a column map needs cols2 = the number of adversarial columns");
      CHK(frame_map_check(c->idx, cols, -1, cols2, "adv_inv"));
    }
    if (c->c && !frame_mat_ok(c->c, c->ldc, c->idx ? cols2 : 0)) return fail(GT_ERR_INVALID, "frame hook: leak misaligned or its pitch below cols2");
    if (c->d && !frame_mat_ok(c->d, c->ldd, c->idx ? cols2 : 0)) return fail(GT_ERR_INVALID, "frame hook: gadv misaligned or its pitch below cols2");
    n_part = c->want_partial ? frame_red_blocks(rows * cols, max_blocks) : 0;
  }
  if (fin_rider || op == GT_FRAME_FINALIZE_G || op == GT_FRAME_FINALIZE_G_RIDER) {
    const bool with_hp = op != GT_FRAME_FINALIZE_G;
    if ((c->part_mge ? (c->n_mge < 1 || c->n_mge > (1 << 20)) : c->n_mge != 0) || (c->part_mse ? (c->n_mse < 1 || c->n_mse > (1 << 20)) : c->n_mse != 0) ||
        (c->hp ? (!with_hp || c->n_hp < 1 || c->n_hp > (1 << 20)) : c->n_hp != 0))
      return fail(GT_ERR_INVALID, "frame hook: partials come with a count of 1 .. 2^20, none with 0 (hp: the rider forms only)");
    if ((((uintptr_t)c->part_mge) | ((uintptr_t)c->part_mse) | ((uintptr_t)c->hp)) & 7) return fail(GT_ERR_INVALID, "frame hook: misaligned partials");
  }
  if (op == GT_FRAME_SCALE_INV_TV && !frame_mat_ok(c->out, cols, cols)) return fail(GT_ERR_INVALID, "frame hook: scale_inv_tv needs out [rows * cols]");
  if (op == GT_FRAME_HIGHWAY_FWD && !(frame_mat_ok(c->a, c->lda, cols) && frame_mat_ok(c->b, c->ldb, cols) && frame_mat_ok(c->c, c->ldc, cols) && frame_mat_ok(c->out, c->ldo, cols)))
    return fail(GT_ERR_INVALID, "frame hook: highway_fwd needs a (x), b (Tx), c (Gx) and out with pitches >= cols");
  if (op == GT_FRAME_HIGHWAY_BWD && !(frame_mat_ok(c->a, c->lda, cols) && frame_mat_ok(c->b, c->ldb, cols) && frame_mat_ok(c->c, c->ldc, cols) && frame_mat_ok(c->out, c->ldo, cols) &&
                                      frame_mat_ok(c->out2, c->ldo2, cols)))
    return fail(GT_ERR_INVALID, "frame hook: highway_bwd needs a (g), b (Tx), c (Gx), out (dGx) and out2 (dTz) with pitches >= cols");
  if (op == GT_FRAME_SIGMOID_GRAD && !(frame_mat_ok(c->a, c->lda, cols) && frame_mat_ok(c->out, c->ldo, cols)))
    return fail(GT_ERR_INVALID, "frame hook: sigmoid_grad needs a (y) and out (g, in place) with pitches >= cols");
  if (op == GT_FRAME_DROPOUT_APPLY) {
    if (!frame_mat_ok(c->a, cols, cols) || !frame_mat_ok(c->out, cols, cols)) return fail(GT_ERR_INVALID, "frame hook: dropout_apply needs dense a and out");
    const char* why;
    if (!tail_site_ok(c->drop, cols, rows, false, &why)) return fail(GT_ERR_INVALID, "frame hook: %s", why);
  }
  if (op == GT_FRAME_BUILD_ADV) {
    if (c->split < 0 || c->split > rows) return fail(GT_ERR_INVALID, "frame hook: 0 <= split <= rows");
    if (c->lda < 1 || (c->split > 0 && !frame_mat_ok(c->a, c->lda, 1)) || (c->split < rows && !frame_mat_ok(c->b, c->lda, 1)))
      return fail(GT_ERR_INVALID, "frame hook: build_adv needs a (rows below split) and b (the rest), both with pitch lda");
    CHK(frame_map_check(c->idx, cols, 0, c->lda, "idx"));
    if (!c->out || (((uintptr_t)c->out) & 15) || c->ldo < cols || (c->ldo & 3)) return fail(GT_ERR_INVALID, "frame hook: build_adv needs a 16-byte aligned out with a pitch >= cols that is a multiple of 4");
    if (c->rider < 0 || c->rider > 2 || (c->rider && !has_mask)) return fail(GT_ERR_INVALID, "frame hook: rider 0, 1 (scalars) or 2 (the count alone), with a mask");
  }
  if (op == GT_FRAME_BUILD_CAT2) {
    if (cols2 < 1 || !frame_mat_ok(c->a, cols, cols) || c->ldb < 1 || !frame_mat_ok(c->b, c->ldb, 1) || !frame_mat_ok(c->c, c->ldb, 1))
      return fail(GT_ERR_INVALID, "frame hook: build_cat2 needs a (x, dense [rows][cols]), b and c (pitch ldb) and cols2 mapped columns");
    CHK(frame_map_check(c->idx, cols2, 0, c->ldb, "idx"));
    if (!frame_mat_ok(c->out, c->ldo, (long)cols + cols2)) return fail(GT_ERR_INVALID, "frame hook: out misaligned or its pitch below cols + cols2");
  }
  if (op == GT_FRAME_REPITCH && (!frame_mat_ok(c->a, c->lda, cols) || !c->out || (((uintptr_t)c->out) & 15) || c->ldo < cols || (c->ldo & 3)))
    return fail(GT_ERR_INVALID, "frame hook: repitch needs a and a 16-byte aligned out with a pitch >= cols that is a multiple of 4");
  if (op == GT_FRAME_DENSE_COPY && !(frame_mat_ok(c->a, c->lda, cols) && frame_mat_ok(c->out, c->ldo, cols))) return fail(GT_ERR_INVALID, "frame hook: dense_copy needs a and out with pitches >= cols");
  if (op == GT_FRAME_PAD_ROWS && !(frame_mat_ok(c->a, cols, cols) && frame_mat_ok(c->out, c->ldo, cols))) return fail(GT_ERR_INVALID, "frame hook: pad_rows needs dense a and out with a pitch >= cols");
  if (op == GT_FRAME_TRANSPOSE && !(frame_mat_ok(c->a, c->lda, cols) && frame_mat_ok(c->out, c->ldo, rows))) return fail(GT_ERR_INVALID, "frame hook: transpose needs a (pitch >= cols) and out (pitch >= rows)");
  if (c->partials && c->partials_cap < n_part) return fail(GT_ERR_INVALID, "frame hook: %d partials for a buffer of %lld", n_part, (long long)c->partials_cap);
  // ---- scratch: the step's scalars, its results, the two partial regions of the engine -- all NaN (0xFF bytes) until something writes them ----
  const size_t off_res = 256, off_part = 512, total = off_part + 2 * FRAME_RED_MAX_BLOCKS * sizeof(double);
  static thread_local HookScratch mem;     // grow-only, no per-call hipMalloc / hipFree (both synchronise the device)
  CHK(mem.ensure(total));
  StepScalars* sc = (StepScalars*)mem.p;
  StepResults* res = (StepResults*)((char*)mem.p + off_res);
  double* part_mge = (double*)((char*)mem.p + off_part);
  double* part_mse = part_mge + FRAME_RED_MAX_BLOCKS;
  float tv_host[2] = {c->tv, 1.0f / c->tv};
  auto body = [&]() -> int {
    HIPCHK(hipMemsetAsync(mem.p, 0xFF, total, s));
    if (c->has_tv) HIPCHK(hipMemcpyAsync(mem.p, tv_host, sizeof(tv_host), hipMemcpyHostToDevice, s));
    if (c->sums) HIPCHK(hipMemcpyAsync((char*)mem.p + offsetof(StepScalars, tv_sum), c->sums, 10 * sizeof(double), hipMemcpyHostToDevice, s));
    if (tv_from_mask) { launch_mask_sum(c->mask, n_mask, c->tv_override, c->tv_dev, sc, s); LAUNCH_CHECK(); }
    GFinalize fin;
    memset(&fin, 0, sizeof(fin));
    if (fin_rider || op == GT_FRAME_FINALIZE_G_RIDER) {
      fin.on = 1; fin.sc = sc; fin.out = c->fin_out ? res : (StepResults*)nullptr; fin.adv_w = c->adv_w; fin.mse_w = c->mse_w; fin.mge_w = c->mge_w;
      fin.has_adv = c->has_adv ? 1 : 0; fin.part_mge = c->part_mge; fin.n_mge = c->n_mge; fin.part_mse = c->part_mse; fin.n_mse = c->n_mse;
      fin.hp = (const HeadPartials*)c->hp; fin.n_hp = c->n_hp;
    }
    switch (op) {
      case GT_FRAME_MASK_SUM: launch_mask_sum(c->mask, n_mask, c->tv_override, c->tv_dev, sc, s); break;
      case GT_FRAME_MASK_TOTAL: launch_mask_total(c->mask, n_mask, &sc->tv_sum, s); break;
      case GT_FRAME_SQERR: {
        SqerrArgs q;
        memset(&q, 0, sizeof(q));
        q.a = c->a; q.lda = c->lda; q.b = c->b; q.ldb = c->ldb; q.mask = c->mask; q.rows = rows; q.D = cols; q.partial = part_mse; q.g = c->out; q.ldg = c->ldo;
        q.gscale = c->w0; q.sc = sc;
        const int nblk = launch_masked_sqerr(q, s, max_blocks);
        LAUNCH_CHECK();
        launch_sum_partials(part_mse, nblk, &sc->s_mse, s);
        break;
      }
      case GT_FRAME_G_LOSSES: {
        GLossesArgs q;
        memset(&q, 0, sizeof(q));
        q.a1 = c->a; q.lda1 = c->lda; q.b1 = c->b; q.ldb1 = c->ldb; q.D1 = cols; q.partial1 = part_mse;
        q.a2 = c->c; q.lda2 = c->ldc; q.b2 = c->d; q.ldb2 = c->ldd; q.D2 = cols2; q.partial2 = part_mge;
        q.mask = c->mask; q.rows = rows;
        int m1 = 0, m2 = 0;
        launch_g_losses(q, &m1, &m2, s, max_blocks);
        LAUNCH_CHECK();
        launch_sum_partials(part_mse, m1, &sc->s_mse, s);
        LAUNCH_CHECK();
        launch_sum_partials(part_mge, m2, &sc->s_mge, s);
        break;
      }
      case GT_FRAME_STATIC_GRAD: {
        StaticGradArgs q;
        memset(&q, 0, sizeof(q));
        q.yhs = c->a; q.ld1 = c->lda; q.ys = c->b; q.ld2 = c->ldb; q.mask = c->mask; q.rows = rows; q.Ds = cols; q.mge_w = c->w0;
        q.adv_inv = c->idx; q.leak = c->c; q.ldl = c->ldc; q.gadv = c->d; q.lda = c->ldd; q.adv_w = c->adv_w; q.gs = c->out; q.ldg = c->ldo;
        q.partial = c->want_partial ? part_mge : (double*)nullptr; q.sc = sc; q.fin = fin; q.leak_unnorm = c->leak_unnorm ? 1 : 0;
        const int nblk = launch_static_grad(q, s, max_blocks);
        if (c->want_partial && !fin_rider) { LAUNCH_CHECK(); launch_sum_partials(part_mge, nblk, &sc->s_mge, s); }
        break;
      }
      case GT_FRAME_FINALIZE_G:
        launch_finalize_g(sc, res, c->adv_w, c->mse_w, c->mge_w, c->has_adv ? 1 : 0, c->zero_gnorm ? 1 : 0, c->part_mge, c->n_mge, c->part_mse, c->n_mse, s);
        break;
      case GT_FRAME_FINALIZE_G_RIDER: launch_finalize_g_rider(fin, s); break;
      case GT_FRAME_FINALIZE_D: launch_finalize_d(sc, res, c->zero_gnorm ? 1 : 0, c->tv_from_sum ? 1 : 0, s); break;
      case GT_FRAME_SCALE_INV_TV: launch_scale_by_inv_tv(c->out, rows * cols, sc, s); break;
      case GT_FRAME_HIGHWAY_FWD: launch_highway_forward(c->a, c->lda, c->b, c->ldb, c->c, c->ldc, c->out, c->ldo, rows, cols, s); break;
      case GT_FRAME_HIGHWAY_BWD: launch_highway_backward(c->a, c->lda, c->b, c->ldb, c->c, c->ldc, c->out, c->ldo, c->out2, c->ldo2, rows, cols, s); break;
      case GT_FRAME_SIGMOID_GRAD: launch_sigmoid_grad(c->out, c->ldo, c->a, c->lda, rows, cols, s); break;
      case GT_FRAME_DROPOUT_APPLY: launch_dropout_apply(c->a, c->out, rows, cols, tail_site_spec(c->drop), s); break;
      case GT_FRAME_BUILD_ADV: {
        BuildAdvArgs q;
        memset(&q, 0, sizeof(q));
        q.fa = c->a; q.fb = c->b; q.ldf = c->lda; q.idx = c->idx; q.na = cols; q.out = c->out; q.ldo = c->ldo; q.split = (long)c->split; q.rows = rows;
        q.tv_mask = c->rider ? c->mask : (const float*)nullptr; q.tv_n = n_mask; q.tv_override = c->tv_override; q.sc = sc;
        q.tv_total = c->rider == 2 ? &sc->tv_sum : (double*)nullptr;
        launch_build_adv(q, s);
        break;
      }
      case GT_FRAME_BUILD_CAT2: launch_build_cat2(c->a, cols, c->b, c->c, c->ldb, c->idx, cols2, c->out, c->ldo, rows, s); break;
      case GT_FRAME_REPITCH: launch_repitch(c->a, c->lda, cols, rows, c->out, c->ldo, s); break;
      case GT_FRAME_DENSE_COPY: launch_copy_cols(c->a, c->lda, 0, c->out, c->ldo, 0, rows, cols, s); break;
      case GT_FRAME_PAD_ROWS: launch_pad_rows(c->a, cols, (int)rows, c->out, c->ldo, s); break;
      case GT_FRAME_TRANSPOSE: launch_transpose_f32(c->a, (int)rows, cols, c->lda, c->out, c->ldo, s); break;
    }
    LAUNCH_CHECK();
    return GT_OK;
  };
  const int r = body();
  hipError_t err = hipStreamSynchronize(s);
  if (err == hipSuccess && r == GT_OK && c->scalars) {
    StepScalars h;
    StepResults hr;
    err = hipMemcpy(&h, sc, sizeof(h), hipMemcpyDeviceToHost);
    if (err == hipSuccess) err = hipMemcpy(&hr, res, sizeof(hr), hipMemcpyDeviceToHost);
    if (err == hipSuccess) {
      double* o = c->scalars;
      o[0] = (double)h.tv; o[1] = (double)h.inv_tv; o[2] = h.tv_sum; o[3] = h.s_real; o[4] = h.s_fake; o[5] = h.n_real_ok; o[6] = h.n_fake_ok;
      o[7] = h.s_adv; o[8] = h.s_mge; o[9] = h.s_mse; o[10] = h.gnorm2_d; o[11] = h.gnorm2_g;
      const float* f = (const float*)&hr;
      for (int i = 0; i < 12; ++i) o[12 + i] = (double)f[i];
      o[24] = (double)n_part; o[25] = (double)n1;
    }
  }
  if (err == hipSuccess && r == GT_OK && c->partials && n_part > 0) {
    if (op == GT_FRAME_G_LOSSES) {
      err = hipMemcpy(c->partials, part_mse, (size_t)n1 * sizeof(double), hipMemcpyDeviceToHost);
      if (err == hipSuccess) err = hipMemcpy(c->partials + n1, part_mge, (size_t)(n_part - n1) * sizeof(double), hipMemcpyDeviceToHost);
    } else err = hipMemcpy(c->partials, op == GT_FRAME_SQERR ? part_mse : part_mge, (size_t)n_part * sizeof(double), hipMemcpyDeviceToHost);
  }
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "frame hook: %s", hipGetErrorString(err));
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// the optimizer family: validation, the step's scalars, the launch (engine and stand-alone operator alike)
// ------------------------------------------------------------------------------------------
// what the descriptor's head (up to state2) decides, the state buffers aside
static int optim_check_head(const gt_optim_desc_ex* od) {
  const int k = od->kind;
  if (k < GT_OPT_ADAGRAD || k > GT_OPT_ASGD) return fail(GT_ERR_INVALID, "unknown optimizer kind %d", k);
  const unsigned allowed = GT_OPTF_BUFFER_LIVE | (k == GT_OPT_SGD ? GT_OPTF_NESTEROV : 0u) | (k == GT_OPT_RMSPROP ? GT_OPTF_CENTERED : 0u) |
                           ((k == GT_OPT_ADAM || k == GT_OPT_ADAMW) ? GT_OPTF_AMSGRAD : 0u) |
                           ((k == GT_OPT_NADAM || k == GT_OPT_RADAM) ? GT_OPTF_DECOUPLED_WD : 0u);
  if (od->flags & ~allowed) return fail(GT_ERR_INVALID, "optimizer flags 0x%x do not belong to kind %d", od->flags, k);
  // the checks of torch.optim's constructors (written so that a NaN fails them)
  if (!(od->lr >= 0.0)) return fail(GT_ERR_INVALID, "Invalid learning rate: %g", od->lr);
  if (!(od->weight_decay >= 0.0)) return fail(GT_ERR_INVALID, "Invalid weight_decay value: %g", od->weight_decay);
  if (k != GT_OPT_SGD && k != GT_OPT_RPROP && k != GT_OPT_ASGD && !(od->eps >= 0.0)) return fail(GT_ERR_INVALID, "Invalid epsilon value: %g", od->eps);
  if (k == GT_OPT_ADAGRAD && !(od->lr_decay >= 0.0)) return fail(GT_ERR_INVALID, "Invalid lr_decay value: %g", od->lr_decay);
  if (k == GT_OPT_ADAM || k == GT_OPT_ADAMW || k == GT_OPT_ADAMAX || k == GT_OPT_NADAM || k == GT_OPT_RADAM) {
    if (!(od->beta1 >= 0.0 && od->beta1 < 1.0)) return fail(GT_ERR_INVALID, "Invalid beta parameter at index 0: %g", od->beta1);
    if (!(od->beta2 >= 0.0 && od->beta2 < 1.0)) return fail(GT_ERR_INVALID, "Invalid beta parameter at index 1: %g", od->beta2);
  }
  if ((k == GT_OPT_SGD || k == GT_OPT_RMSPROP) && !(od->momentum >= 0.0)) return fail(GT_ERR_INVALID, "Invalid momentum value: %g", od->momentum);
  if (k == GT_OPT_SGD && (od->flags & GT_OPTF_NESTEROV) && (od->momentum <= 0.0 || od->dampening != 0.0))
    return fail(GT_ERR_INVALID, "Nesterov momentum requires a momentum and zero dampening");
  if (k == GT_OPT_RMSPROP && !(od->alpha >= 0.0)) return fail(GT_ERR_INVALID, "Invalid alpha value: %g", od->alpha);
  if (k == GT_OPT_ADADELTA && !(od->alpha >= 0.0 && od->alpha <= 1.0)) return fail(GT_ERR_INVALID, "Invalid rho value: %g", od->alpha);
  if (od->step < 0) return fail(GT_ERR_INVALID, "negative step count");
  return GT_OK;
}
// the descriptor's tail, which exists for GT_OPT_NADAM .. GT_OPT_ASGD only
static int optim_check_tail(const gt_optim_desc_ex* od) {
  const int k = od->kind;
  if (k == GT_OPT_NADAM) {
    if (!(od->momentum_decay >= 0.0)) return fail(GT_ERR_INVALID, "Invalid momentum_decay value: %g", od->momentum_decay);
    // (0 is a legitimate value: the float32 product of factors near 0.45 underflows to it after some 135 updates, and torch goes on with 1 - 0)
    if (!(od->host_state0 >= 0.0 && od->host_state0 <= 1.0) || (od->step == 0 && od->host_state0 != 1.0))
      return fail(GT_ERR_INVALID, "NAdam: host_state0 (mu_product) is %g: 1 before the first update, in [0, 1] after", od->host_state0);
  }
  if (k == GT_OPT_RPROP) {
    if (!(0.0 < od->etaminus && od->etaminus < 1.0 && 1.0 < od->etaplus))
      return fail(GT_ERR_INVALID, "Invalid eta values: %g, %g", od->etaminus, od->etaplus);
    if (od->weight_decay != 0.0) return fail(GT_ERR_INVALID, "Rprop has no weight_decay");
  }
  if (k == GT_OPT_ASGD && !(od->host_state1 > 0.0 && od->host_state1 <= 1.0 && od->host_state0 >= 0.0))
    return fail(GT_ERR_INVALID, "ASGD: host_state0 (eta) is %g and host_state1 (mu) is %g: (float)lr and 1 before the first update", od->host_state0,
                od->host_state1);
  return GT_OK;
}

// The variants of optim_step_kernel: one row per legal (kind, internal flags) pair, with the state streams it
// reads and writes.
typedef void (*OptimKernel)(float*, float*, float*, float*, float*, long, const double*, int, double*, OptimSpec, const unsigned int*,
                            unsigned int*, unsigned int*, const float*);
// kernel_ema: the same pair with the weight-average rider (gt_set_param_ema) compiled in -- a second column, not a second set of rows
struct OptimVariant { int kind; unsigned flags; bool s0, s1, s2; OptimKernel kernel, kernel_ema; };
#define OPTIM_ROW(KIND, F) \
  {KIND, (F), OptimStreams<KIND, (F)>::s0, OptimStreams<KIND, (F)>::s1, OptimStreams<KIND, (F)>::s2, optim_step_kernel<KIND, (F)>, \
   optim_step_kernel<KIND, (F), true>}
static const OptimVariant OPTIM_VARIANTS[] = {
  OPTIM_ROW(OPTK_ADAGRAD, OPTI_ORIGINAL),
  OPTIM_ROW(OPTK_ADAM, OPTI_ORIGINAL), OPTIM_ROW(OPTK_ADAM, OPTI_AMSGRAD),
  OPTIM_ROW(OPTK_SGD, 0u), OPTIM_ROW(OPTK_SGD, OPTI_MOMENTUM), OPTIM_ROW(OPTK_SGD, OPTI_NESTEROV | OPTI_MOMENTUM),
  OPTIM_ROW(OPTK_RMSPROP, 0u), OPTIM_ROW(OPTK_RMSPROP, OPTI_CENTERED),
  OPTIM_ROW(OPTK_RMSPROP, OPTI_MOMENTUM), OPTIM_ROW(OPTK_RMSPROP, OPTI_CENTERED | OPTI_MOMENTUM),
  OPTIM_ROW(OPTK_ADADELTA, 0u),
  OPTIM_ROW(OPTK_ADAMW, 0u), OPTIM_ROW(OPTK_ADAMW, OPTI_AMSGRAD),
  OPTIM_ROW(OPTK_ADAMAX, 0u),
  OPTIM_ROW(OPTK_NADAM, 0u), OPTIM_ROW(OPTK_NADAM, OPTI_DECOUPLED),
  OPTIM_ROW(OPTK_RADAM, 0u), OPTIM_ROW(OPTK_RADAM, OPTI_RECTIFIED),
  OPTIM_ROW(OPTK_RADAM, OPTI_DECOUPLED), OPTIM_ROW(OPTK_RADAM, OPTI_DECOUPLED | OPTI_RECTIFIED),
  OPTIM_ROW(OPTK_RPROP, 0u),
  OPTIM_ROW(OPTK_ASGD, 0u), OPTIM_ROW(OPTK_ASGD, OPTI_AVERAGE),
};
#undef OPTIM_ROW
// The internal flags of a descriptor's update: its GT_OPTF_* (the OPTI_* of the same values), what its hyper-parameters decide
// (OPTI_MOMENTUM, OPTI_ORIGINAL) and what the host decides for the step at hand (`step_flags`: OPTI_RECTIFIED, OPTI_AVERAGE, which
// change no stream: a descriptor's row with step_flags = 0 tells its state buffers).
static unsigned optim_flags(const gt_optim_desc_ex& od, unsigned step_flags) {
  const int k = od.kind;
  unsigned f = (od.flags & (OPTI_NESTEROV | OPTI_CENTERED | OPTI_AMSGRAD | OPTI_DECOUPLED)) | step_flags;
  if ((k == GT_OPT_SGD || k == GT_OPT_RMSPROP) && od.momentum != 0.0) f |= OPTI_MOMENTUM;
  if (k == GT_OPT_ADAGRAD || (k == GT_OPT_ADAM && !(f & OPTI_AMSGRAD))) f |= OPTI_ORIGINAL;
  return f;
}
static const OptimVariant* optim_variant(int kind, unsigned flags) {
  for (const OptimVariant& v : OPTIM_VARIANTS)
    if (v.kind == kind && v.flags == flags) return &v;
  return nullptr;
}

int optim_check_desc(const gt_optim_desc_ex* od) {
  CHK(optim_check_head(od));
  const int k = od->kind;
  const OptimVariant* v = optim_variant(k, optim_flags(*od, 0u));
  if (!v) return fail(GT_ERR_INVALID, "unknown optimizer kind %d", k);
  if ((v->s0 && !od->state0) || (v->s1 && !od->state1) || (v->s2 && !od->state2))
    return fail(GT_ERR_INVALID, "optimizer state buffer is null (kind %d, flags 0x%x needs state%s%s%s)", k, od->flags, v->s0 ? " 0" : "",
                v->s1 ? " 1" : "", v->s2 ? " 2" : "");
  return optim_check_tail(od);      // after everything that the head alone decides: a null buffer is reported without reading the tail
}

// The descriptor as the library keeps it: the first family's kinds are copied up to state2 (a caller built against that
// 120-byte struct passes no more) with a zero tail, the kinds that have a tail whole.
void optim_desc_copy(const gt_optim_desc_ex* in, gt_optim_desc_ex* out) {
  memset(out, 0, sizeof(*out));
  memcpy(out, in, (in->kind >= GT_OPT_NADAM && in->kind <= GT_OPT_ASGD) ? sizeof(*out) : offsetof(gt_optim_desc_ex, momentum_decay));
}

// NAdam's momentum cache mu_t (python floats in torch: double)
static double nadam_mu(const gt_optim_desc_ex& od, long t) { return od.beta1 * (1.0 - 0.5 * pow(0.96, (double)t * od.momentum_decay)); }

// The host scalar state after `t` updates (t >= od.step): torch's 0-dim float32 state tensors mu_product (NAdam) and eta, mu (ASGD).
// A pure function of the descriptor (its step and host_state* are those of the bind) and t, so that a step counter that
// gt_clear_faults moved back needs no undo here; `cache` only shortens NAdam's running product and may be null.
void optim_host_scalars(const gt_optim_desc_ex& od, long t, OptimScalarCache* cache, double out[2]) {
  out[0] = out[1] = 0.0;
  if (od.kind == GT_OPT_NADAM) {
    long s = (long)od.step;
    float mp = (float)od.host_state0;
    if (cache && cache->valid && cache->step >= s && cache->step <= t) { s = cache->step; mp = cache->mu_product; }
    for (; s < t; ++s) mp = mp * (float)nadam_mu(od, s + 1);      // mu_product *= mu: a float32 tensor times a python float, in float32
    if (cache) { cache->valid = true; cache->step = t; cache->mu_product = mp; }
    out[0] = (double)mp;
  } else if (od.kind == GT_OPT_ASGD) {
    if (t == (long)od.step) { out[0] = od.host_state0; out[1] = od.host_state1; return; }
    // eta.copy_(lr / (1 + lambd lr step) ** alpha), mu.copy_(1 / max(1, step - t0)): python floats stored into float32 tensors
    out[0] = (double)(float)(od.lr / pow(1.0 + od.lambd * od.lr * (double)t, od.alpha));
    out[1] = (double)(float)(1.0 / std::max(1.0, (double)t - od.t0));
  }
}

// The scalars of update number `step` (1-based), formed in double from the double hyper-parameters and rounded to float
// once -- python arithmetic followed by a Scalar -> float conversion in torch's single-tensor code paths.  `flags` receives
// what the host decides for this update beyond the descriptor's flags (OPTI_RECTIFIED, OPTI_AVERAGE).  The OPTI_ORIGINAL kinds
// alone get their hyper-parameters rounded to float and the step count: they form their scalars in the kernel.
static OptimSpec optim_spec(const gt_optim_desc_ex& od, long step, bool buf_live, OptimScalarCache* cache, unsigned* flags) {
  OptimSpec o;
  memset(&o, 0, sizeof(o));
  const double lr = od.lr;
  o.max_norm = od.max_grad_norm; o.wd = (float)od.weight_decay; o.eps = (float)od.eps;
  o.neg_step = (float)-lr;
  o.live = buf_live ? 1 : 0;
  if (optim_flags(od, 0u) & OPTI_ORIGINAL) {
    o.lr = (float)lr; o.lr_decay = (float)od.lr_decay; o.beta1 = (float)od.beta1; o.beta2 = (float)od.beta2; o.step = step;
    return o;
  }
  switch (od.kind) {
    case GT_OPT_SGD:
      o.mu = (float)od.momentum; o.omd = (float)(1.0 - od.dampening);
      break;
    case GT_OPT_RMSPROP:
      o.mu = (float)od.momentum; o.a = (float)od.alpha; o.oma = (float)(1.0 - od.alpha);
      break;
    case GT_OPT_ADADELTA:
      o.a = (float)od.alpha; o.oma = (float)(1.0 - od.alpha);
      break;
    case GT_OPT_ADAM: case GT_OPT_ADAMW:
      o.w1 = (float)(1.0 - od.beta1); o.a = (float)od.beta2; o.oma = (float)(1.0 - od.beta2);
      o.neg_step = (float)-(lr / (1.0 - pow(od.beta1, (double)step)));
      o.bc2_sqrt = (float)sqrt(1.0 - pow(od.beta2, (double)step));
      o.decay = (float)(1.0 - lr * od.weight_decay);
      break;
    case GT_OPT_ADAMAX:
      o.w1 = (float)(1.0 - od.beta1); o.a = (float)od.beta2;
      o.neg_step = (float)-(lr / (1.0 - pow(od.beta1, (double)step)));
      break;
    case GT_OPT_NADAM: {
      double hs[2];
      optim_host_scalars(od, step, cache, hs);                  // mu_product after this update's `mu_product *= mu`
      const double mu = nadam_mu(od, step), mu_next = nadam_mu(od, step + 1), mu_product = hs[0];
      o.w1 = (float)(1.0 - od.beta1); o.a = (float)od.beta2; o.oma = (float)(1.0 - od.beta2);
      o.bc2 = (float)(1.0 - pow(od.beta2, (double)step));
      o.c_g = (float)(-lr * (1.0 - mu) / (1.0 - mu_product));
      o.c_m = (float)((-lr * mu_next) / (1.0 - mu_product * mu_next));
      o.decay = (float)(1.0 - lr * od.weight_decay);
      break;
    }
    case GT_OPT_RADAM: {
      const double t = (double)step, b2t = pow(od.beta2, t);
      const double bc1 = 1.0 - pow(od.beta1, t), bc2 = 1.0 - b2t;
      const double rho_inf = 2.0 / (1.0 - od.beta2) - 1.0;
      const double rho_t = rho_inf - 2.0 * t * b2t / bc2;
      o.w1 = (float)(1.0 - od.beta1); o.a = (float)od.beta2; o.oma = (float)(1.0 - od.beta2);
      o.bc1 = (float)bc1; o.lr = (float)lr; o.bc2_sqrt = (float)sqrt(bc2);
      o.decay = (float)(1.0 - lr * od.weight_decay);
      if (rho_t > 5.0) {
        *flags |= OPTI_RECTIFIED;
        o.rect = (float)sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t));
      }
      break;
    }
    case GT_OPT_RPROP:
      o.wd = 0.f;
      o.eta_minus = (float)od.etaminus; o.eta_plus = (float)od.etaplus;
      o.step_min = (float)od.step_size_min; o.step_max = (float)od.step_size_max;
      break;
    case GT_OPT_ASGD: {
      double hs[2];
      optim_host_scalars(od, step - 1, cache, hs);              // eta and mu as the previous update left them
      o.decay = (float)(1.0 - od.lambd * hs[0]);
      o.neg_step = (float)-hs[0];
      o.mu = (float)hs[1];
      if (hs[1] != 1.0) *flags |= OPTI_AVERAGE;
      break;
    }
  }
  return o;
}

int launch_optim_step(const gt_optim_desc_ex& od, long step, bool buf_live, OptimScalarCache* cache, float* params, float* grads, long n,
                      const double* part, int n_partial, double* norm2_out, const unsigned int* fault_dev, unsigned int* fault_host,
                      unsigned int* skipped_host, const float* gscale, hipStream_t s, float weight_clip, float* ema, float ema_w,
                      bool ema_first) {
  const dim3 grid((unsigned)std::min<long>(1024, cdiv(n, RED_THREADS))), block(RED_THREADS);
  unsigned step_flags = 0u;
  OptimSpec o = optim_spec(od, step, buf_live, cache, &step_flags);
  o.wclip = weight_clip;      // gt_set_weight_clip: the updated parameters are clamped to [-c, c] in the same launch (0: stored as computed)
  o.ema = ema; o.ema_w = ema_w; o.ema_first = ema_first ? 1 : 0;      // gt_set_param_ema: the average of the stored parameters, same launch (null: none)
  const OptimVariant* v = optim_variant(od.kind, optim_flags(od, step_flags));
  if (!v) return fail(GT_ERR_INVALID, "unknown optimizer kind %d", od.kind);
  // gt_profile_enable(2 + 8): this launch between two events (slot 15).  Only when selected by its kind, never under "every product launch"
  GemmProfiler::Rec rec;
  const bool prof = g_prof.on && g_prof.only_kind == 8;
  if (prof) {
    rec.kind = 8; rec.bn = 0; rec.am = -1; rec.flops = 0.0;
    rec.bytes = (double)n * (16.0 + 8.0 * ((v->s0 ? 1 : 0) + (v->s1 ? 1 : 0) + (v->s2 ? 1 : 0)) + (ema ? 8.0 : 0.0));
    rec.e0 = g_prof.get(); rec.e1 = g_prof.get();
    HIPCHK(hipEventRecord(rec.e0, s));
  }
  hipLaunchKernelGGL(ema ? v->kernel_ema : v->kernel, grid, block, 0, s, params, grads, od.state0, od.state1, od.state2, n, part, n_partial, norm2_out, o,
                     fault_dev, fault_host, skipped_host, gscale);
  LAUNCH_CHECK();
  if (prof) { HIPCHK(hipEventRecord(rec.e1, s)); g_prof.recs.push_back(rec); }
  return GT_OK;
}

extern "C" int gt_op_optim_scalars(const gt_optim_desc_ex* desc, int64_t t, double out[2]) {
  if (!desc || !out) return fail(GT_ERR_INVALID, "bad argument");
  CHK(optim_check_head(desc));      // everything gt_bind_optimizer_ex checks but the state buffers
  CHK(optim_check_tail(desc));
  if (desc->step < 0 || t < desc->step) return fail(GT_ERR_INVALID, "the scalars are defined from the descriptor's step (%lld) on, not at %lld",
                                                     (long long)desc->step, (long long)t);
  gt_optim_desc_ex od;
  optim_desc_copy(desc, &od);
  if (od.kind != GT_OPT_ASGD) od.lr = (double)(float)desc->lr;
  optim_host_scalars(od, (long)t, (OptimScalarCache*)nullptr, out);
  return GT_OK;
}

// gt_set_param_ema / gt_op_optim_step_ema: the decay is a number in [0, 1] (written so that a NaN fails)
int param_ema_check_decay(const char* who, double decay) {
  if (!(decay >= 0.0 && decay <= 1.0)) return fail(GT_ERR_INVALID, "%s: decay = %g -- a number in [0, 1]", who, decay);
  return GT_OK;
}

static int op_optim_step(const gt_optim_desc_ex* desc, float* params, float* grads, int64_t n, const float* gscale, float* grad_norm_out,
                         float* ema, bool ema_first, double decay, void* stream) {
  if (!desc || !params || !grads || n < 1) return fail(GT_ERR_INVALID, "bad argument");
  CHK(optim_check_desc(desc));
  hipStream_t s = (hipStream_t)stream;
  static thread_local HookScratch tls_ws;     // [0, 512) squared-norm partials, [512] the squared norm
  CHK(tls_ws.ensure(513 * sizeof(double)));
  double* part = (double*)tls_ws.p;
  gt_optim_desc_ex od;
  optim_desc_copy(desc, &od);
  if (od.kind != GT_OPT_ASGD) od.lr = (double)(float)desc->lr;        // as gt_bind_optimizer_ex keeps it
  // the engine's fallback branch (optimizer_step, eng_step.hip): partials, then clip + update
  const int nblk = (int)std::min<long>(512, cdiv(n, RED_THREADS * 4));
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(nblk), dim3(RED_THREADS), 0, s, (const float*)grads, (long)n, part);
  LAUNCH_CHECK();
  CHK(launch_optim_step(od, (long)desc->step + 1, (desc->flags & GT_OPTF_BUFFER_LIVE) != 0, (OptimScalarCache*)nullptr, params, grads, (long)n, part, nblk,
                        grad_norm_out ? part + 512 : (double*)nullptr, (const unsigned int*)nullptr, (unsigned int*)nullptr,
                        (unsigned int*)nullptr, gscale, s, 0.f, ema, param_ema_weight(decay), ema_first));
  if (grad_norm_out) {
    double norm2 = 0.0;
    HIPCHK(hipMemcpyAsync(&norm2, part + 512, sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *grad_norm_out = (float)sqrt(norm2);
  }
  return GT_OK;
}
extern "C" int gt_op_optim_step(const gt_optim_desc_ex* desc, float* params, float* grads, int64_t n, const float* gscale,
                                float* grad_norm_out, void* stream) {
  return op_optim_step(desc, params, grads, n, gscale, grad_norm_out, (float*)nullptr, false, 0.0, stream);
}
extern "C" int gt_op_optim_step_ema(const gt_optim_desc_ex* desc, float* params, float* grads, int64_t n, const float* gscale,
                                    float* grad_norm_out, float* ema, int64_t n_averaged, double decay, void* stream) {
  if (!ema) return fail(GT_ERR_INVALID, "gt_op_optim_step_ema: ema is null");
  if (n_averaged < 0) return fail(GT_ERR_INVALID, "gt_op_optim_step_ema: n_averaged = %lld -- the updates already averaged, >= 0", (long long)n_averaged);
  CHK(param_ema_check_decay("gt_op_optim_step_ema", decay));
  return op_optim_step(desc, params, grads, n, gscale, grad_norm_out, ema, n_averaged == 0, decay, stream);
}

// ------------------------------------------------------------------------------------------
// spectral normalisation (eng_spectral_norm.hip): the hooks build the job table the engine builds at a bind and call its launch functions
// ------------------------------------------------------------------------------------------
static int sn_case_plan(const gt_sn_case* c, SnPlan** plan, SnBufs* b) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (c->n_layers < 1 || c->n_layers > GT_SN_MAX_LAYERS) return fail(GT_ERR_INVALID, "spectral norm: n_layers %d (1 .. %d)", c->n_layers, GT_SN_MAX_LAYERS);
  if (c->n_flat < 1 || !c->u || !c->v || !c->weff || !c->sigma) return fail(GT_ERR_INVALID, "spectral norm: null buffer or empty flat buffer");
  SnLayerDesc layers[GT_SN_MAX_LAYERS];
  for (int q = 0; q < c->n_layers; ++q) { layers[q].w_off = (long)c->w_off[q]; layers[q].out = c->out[q]; layers[q].in = c->in[q]; }
  CHK(sn_plan_build(layers, c->n_layers, (long)c->n_flat, plan));
  static thread_local HookScratch tls_ws;     // the double sums between the launches (grow-only)
  const int r = tls_ws.ensure(sn_plan_bytes(*plan));
  if (r != GT_OK) { sn_plan_free(*plan); return r; }
  *b = sn_plan_bufs(*plan, tls_ws.p);
  b->sigma = c->sigma;
  return GT_OK;
}
extern "C" int gt_op_spectral_norm(const gt_sn_case* c, void* stream) {
  SnPlan* plan = nullptr;
  SnBufs b;
  CHK(sn_case_plan(c, &plan, &b));
  int r = c->W ? GT_OK : fail(GT_ERR_INVALID, "spectral norm: W is null");
  if (r == GT_OK) r = launch_sn_prepare(plan, c->W, c->u, c->v, c->weff, b, c->iterate != 0, (hipStream_t)stream);
  sn_plan_free(plan);
  return r;
}
extern "C" int gt_op_sn_project(const gt_sn_case* c, void* stream) {
  SnPlan* plan = nullptr;
  SnBufs b;
  CHK(sn_case_plan(c, &plan, &b));
  int r = GT_OK;
  if (!c->G || !c->s || !c->norm_partials || !c->n_norm_partials) r = fail(GT_ERR_INVALID, "spectral norm projection: null buffer");
  else if (c->norm_cap < sn_plan_partials(plan)) r = fail(GT_ERR_INVALID, "spectral norm projection: %d squared-norm partials, room for %ld", sn_plan_partials(plan), (long)c->norm_cap);
  if (r == GT_OK) {
    b.s = c->s;
    *c->n_norm_partials = sn_plan_partials(plan);
    r = launch_sn_project(plan, c->G, c->weff, c->u, c->v, b, c->norm_partials, (hipStream_t)stream);
  }
  sn_plan_free(plan);
  return r;
}

// ------------------------------------------------------------------------------------------
// gradient penalties (eng_grad_penalty.hip): the hook fills the block the step fills from the engine and calls the same launch function
// ------------------------------------------------------------------------------------------
extern "C" int gt_op_grad_penalty(const gt_gp_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  if (c->L < 1 || c->L > GT_GP_MAX_LAYERS || c->H < 1 || c->cd < 0 || c->Da < 1 || c->rows < 1 || c->ld_g < c->Da || (c->kind != GP_R1 && c->kind != GP_WGAN))
    return fail(GT_ERR_INVALID, "gradient penalty: malformed case (L %d, H %d, cd %d, Da %d, rows %ld, ld_g %d, kind %d)", c->L, c->H, c->cd, c->Da,
                (long)c->rows, c->ld_g, c->kind);
  if (!c->w_last || !c->dw_last || !c->mask || !c->g || !c->sums) return fail(GT_ERR_INVALID, "gradient penalty: null buffer");
  GpCall k;
  memset(&k, 0, sizeof(k));
  k.L = c->L; k.cd = c->cd; k.Da = c->Da; k.kind = c->kind; k.prec = PREC_F32; k.weight = c->weight; k.rows = (long)c->rows;
  for (int l = 0; l < c->L; ++l) {
    const char* why = nullptr;
    if (!c->W[l] || !c->dW[l] || !c->Hact[l] || !c->a[l] || !c->c[l]) return fail(GT_ERR_INVALID, "gradient penalty: null buffer of layer %d", l);
    if (!tail_site_ok(c->drop[l], c->H, (long)c->rows, false, &why)) return fail(GT_ERR_INVALID, "gradient penalty: layer %d: %s", l, why);
    GpLayer& q = k.l[l];
    q.W = c->W[l]; q.dW = c->dW[l]; q.in = l == 0 ? c->cd + c->Da : c->H; q.out = c->H;
    q.H = c->Hact[l]; q.spec = tail_site_spec(c->drop[l]); q.a = c->a[l]; q.c = c->c[l];
  }
  static thread_local HookScratch tls_part, tls_dw0, tls_slabs, tls_colp;      // scratch of the call (grow-only)
  const int nblk = gp_row_blocks((long)c->rows);
  CHK(tls_part.ensure((size_t)2 * nblk * sizeof(double)));
  CHK(tls_dw0.ensure((size_t)c->H * c->Da * sizeof(float)));
  k.w_last = c->w_last; k.dw_last = c->dw_last; k.g = c->g; k.ld_g = c->ld_g; k.g_copy = c->g_copy;
  k.mask = c->mask; k.inv_tv = c->inv_tv; k.phi = c->phi; k.nrm = c->nrm;
  k.part = tls_part.as<double>(); k.part_cap = 2L * nblk; k.sums = c->sums; k.rec = c->rec;
  k.dw0s = tls_dw0.as<float>(); k.slabs = &tls_slabs; k.colp = &tls_colp;
  return launch_grad_penalty(k, (hipStream_t)stream);
}
