// libgantts_hip.so -- the G+D step: MLP stacks, apply_generator / update_discriminator / update_generator (reference train.py:245-355), plain forward
#include "engine_internal.hip.h"
#include "d_tail_args.hip.h"
#include "d_tail_launch.hip.h"
#include <atomic>

using namespace gt;
// ------------------------------------------------------------------------------------------
// network passes
// ------------------------------------------------------------------------------------------
// stacked injected-mask buffer for one layer of a D pass group (real rows then fake rows)
static int stage_injected(gt_engine* e, int role, int layer, const int* passes, int npass, long rows_each, int width,
                          const float** out, hipStream_t s) {
  Net& n = e->net[role];
  *out = nullptr;
  if (!n.training || n.d.dropout <= 0.f) return GT_OK;
  bool any = false, all = true;
  for (int i = 0; i < npass; ++i) { any |= n.inj[passes[i]][layer] != nullptr; all &= n.inj[passes[i]][layer] != nullptr; }
  if (!any) return GT_OK;
  if (!all) return fail(GT_ERR_INVALID, "injected dropout masks must be given for every pass of a step or for none");
  if (npass == 1) { *out = n.inj[passes[0]][layer]; return GT_OK; }
  const size_t per_layer = (size_t)npass * rows_each * width * sizeof(float);
  CHK(e->dmask.ensure(per_layer * n.d.num_hidden));
  float* base = (float*)((char*)e->dmask.p + per_layer * layer);
  for (int i = 0; i < npass; ++i)
    HIPCHK(hipMemcpyAsync(base + (size_t)i * rows_each * width, n.inj[passes[i]][layer], (size_t)rows_each * width * sizeof(float),
                          hipMemcpyDeviceToDevice, s));
  *out = base;
  return GT_OK;
}

// SPLIT first layer of the conditioned discriminator (float32 path).  D sees [x | adv] (train.py:254-256) for the real AND the
// generated rows of a D step with the SAME x, so layer 0 is evaluated as
//     P = x . W[:, :cd]^T + b                      once, over the `wrap` rows of x             (no activation)
//     H = act(adv . W[:, cd:]^T + P[r mod wrap])   over all rows of the pass                   (K = Da = 58 columns)
// instead of one product over a concatenated [2N][cd + Da] image: no image of x is built (109 MB / step at cfg2), the
// x product of a D step is done once instead of twice (- 44 % of the layer's flops), and the weight gradient contracts
// (dZ_real + dZ_generated) with x over N frames (linear_backward_weight_split).  Same sums up to float32 association.
struct FirstSplit {
  const float* x; int ldx; int cd;     // conditioning input: `wrap` rows, any pitch (k-contiguous operand)
  const float* xp; int ldxp;           // the same rows with a 16-byte pitch (weight gradient), or null (forward only)
  const float* adv; int ld_adv;        // [rows][ld_adv]: the pass's adversarial columns, 16-byte pitch
  long wrap;
};
// M's copy of p [rows][cols] (row pitch ld) with row pitch ldo, dense or with a 16-byte pitch: made unless M holds it already, i.e. once per step.
// (the key: source pointer, pitch, columns, rows, step -- ADVICE r5: the pointer and the step alone served a too small copy to a caller that
//  changed B*T between two update_* calls of one step.  The CONTENTS of p are not part of it: a tensor refilled in place within a step is not seen.
//  A copy never outlives its batch: gt_apply_generator and gt_set_seed forget all three -- the step count goes back under gt_set_seed, and the next
//  batch from a staging buffer refilled in place then had the key of the one before.)
static int step_copy(gt_engine* e, StepCopy& M, const float* p, int ld, int cols, long rows, int ldo, bool dense, const float** out, hipStream_t s) {
  if (!M.holds(p, ld, cols, rows, e->step_counter)) {
    CHK(M.buf.ensure((size_t)rows * ldo * sizeof(float)));
    if (dense) launch_copy_cols(p, ld, 0, M.buf.as<float>(), ldo, 0, rows, cols, s);
    else launch_repitch(p, ld, cols, rows, M.buf.as<float>(), ldo, s);
    LAUNCH_CHECK();
    M.built(p, ld, cols, rows, e->step_counter);
  }
  *out = M.buf.as<float>();
  return GT_OK;
}
// a caller tensor's rows with a 16-byte pitch: the tensor itself when it already has one, else M's copy
static int pitched_rows(gt_engine* e, StepCopy& M, const float* p, int ld, int cols, long rows, const float** out, int* ldo, hipStream_t s) {
  if (gemm_vec_ok(p, ld)) { *out = p; *ldo = ld; return GT_OK; }
  *ldo = (cols + 3) & ~3;
  return step_copy(e, M, p, ld, cols, rows, *ldo, false, out, s);
}

// hidden stack forward: in -> acts[0..L-1]; returns specs used (for backward)
static int stack_forward(gt_engine* e, int role, const float* in, int ld_in, long rows, const int* passes, int npass, long rows_each, std::vector<DropoutSpec>& specs, hipStream_t s,
                         const FirstSplit* fs = nullptr, int max_layers = 1 << 30 /* launch only the first max_layers layers (the dropout
                         sites and the stash buffers of ALL layers are still set up: the fused stack launch takes over from there) */) {
  Net& n = e->net[role];
  std::vector<Scratch>& acts = e->ws[role].act;
  const int prec = product_prec(e, role);
  specs.resize(n.hidden.size());
  const float* cur = in;
  int ld = ld_in;
  for (size_t l = 0; l < n.hidden.size(); ++l) {
    const Lin& L = n.hidden[l];
    CHK(acts[l].ensure((size_t)rows * L.out * sizeof(float)));
    const float* inj = nullptr;
    CHK(stage_injected(e, role, (int)l, passes, npass, rows_each, L.out, &inj, s));
    specs[l] = drop_spec(e, role, passes[0], (int)l, inj, L.out, npass == 2 ? rows_each : 0);
    if ((int)l >= max_layers) continue;
    if (l == 0 && fs && specs[l].mode == DROP_PHILOX && gt_tuning().split_fused && gemm_vec_ok(fs->x, fs->ldx, true) &&
        gemm_vec_ok(L.W, L.in, true) && gemm_vec_ok(fs->adv, fs->ld_adv, true) && fs->wrap > 64 && gemm_small_tiles_ok() &&
        prec == PREC_F32 && (rows == fs->wrap || rows == 2 * fs->wrap)) {
      // ONE launch (linear_forward_seg): no P buffer
      CHK(linear_forward_seg(fs->x, fs->ldx, fs->wrap, fs->cd, fs->adv, fs->ld_adv, rows, L.W, L.in, L.in, L.b, acts[l].as<float>(), L.out, L.out,
                             ACT_LEAKY_DROPOUT, specs[l], prec, s));
      cur = acts[l].as<float>();
      ld = L.out;
      continue;
    }
    if (l == 0 && fs) {
      const int Da = L.in - fs->cd;
      CHK(e->d_pre.ensure((size_t)fs->wrap * L.out * sizeof(float)));
      CHK(linear_forward(fs->x, fs->ldx, L.W, L.in, L.b, e->d_pre.as<float>(), L.out, fs->wrap, fs->cd, L.out, ACT_NONE, no_drop(), prec, s));
      CHK(linear_forward(fs->adv, fs->ld_adv, L.W + fs->cd, L.in, nullptr, acts[l].as<float>(), L.out, rows, Da, L.out, ACT_LEAKY_DROPOUT, specs[l],
                         prec, s, e->d_pre.as<float>(), L.out, fs->wrap));
      cur = acts[l].as<float>();
      ld = L.out;
      continue;
    }
    const float* W = L.W;
    int ldw = L.in;
    if (l == 0 && (L.in & 3) && gemm_vec_ok(cur, ld) && !gemm_vec_ok(L.W, L.in, true) && prec == PREC_F32) {
      // The input image takes 16-byte loads (the discriminator's [x | adv] image, pitch 484) but the weight rows (483
      // floats) do not: multiply by a copy of W with its row pitch rounded up to 4 floats, re-made from the caller's
      // parameter buffer before every pass (it may have been stepped, loaded or broadcast since).
      ldw = (L.in + 3) & ~3;
      CHK(e->ws[role].w0pad.ensure((size_t)L.out * ldw * sizeof(float)));
      launch_pad_rows(L.W, L.in, L.out, e->ws[role].w0pad.as<float>(), ldw, s);
      LAUNCH_CHECK();
      W = e->ws[role].w0pad.as<float>();
    }
    CHK(linear_forward(cur, ld, W, ldw, L.b, acts[l].as<float>(), L.out, rows, L.in, L.out, ACT_LEAKY_DROPOUT, specs[l], prec, s));
    cur = acts[l].as<float>();
    ld = L.out;
  }
  return GT_OK;
}

// Measured with one rank and forced collectives (bench.py --force-dp, plain step 1.465 ms): round-2 schedule 1.577 ms; the
// discriminator's gradient as ONE message 1.561 (kept); additionally ncclGroupStart/End around a step's closing messages
// 1.571 (removed); generator loss sums sent with the closing messages instead of early 1.604 (off: the host then waits for the
// whole step before it can enqueue the next one).

// hidden stack backward.  dz_top: gradient w.r.t. the pre-activation of the TOP hidden layer
// (already multiplied by f'), in buffer `cur` (rows x hidden).  Produces dW/db (if want_w) and,
// optionally, dX[:, col0:col0+ncols] of the stack input for rows [row0, row0+nrows).
static int stack_backward(gt_engine* e, int role, const float* in, int ld_in, long rows, const std::vector<DropoutSpec>& specs, float* cur, float* other, bool want_w,
                          float* dX, int lddx, int col0, int ncols, long row0, long nrows, hipStream_t s, const FirstSplit* fs = nullptr) {
  Net& n = e->net[role];
  std::vector<Scratch>& acts = e->ws[role].act;
  const int L = (int)n.hidden.size(), prec = product_prec(e, role);
  // per-layer launches: each layer's weight gradient right behind the product that made its dZ (still warm in L2 / MALL)
  for (int l = L - 1; l >= 0; --l) {
    const Lin& Lr = n.hidden[l];
    const float* Xin = l > 0 ? acts[l - 1].as<float>() : in;
    const int ldx = l > 0 ? n.hidden[l - 1].out : ld_in;
    bool rode = false;
    GemmArgs nn;
    if (l > 0) nn = backward_data_args(cur, Lr.out, Lr.W, Lr.in, 0, other, Lr.in, rows, Lr.out, Lr.in, ACT_LEAKY_DROPOUT,
                                       acts[l - 1].as<float>(), Lr.in, specs[l - 1]);
    if (want_w && l == 0 && fs) {
      // the kept gradient w.r.t. the generated rows' adversarial columns (no activation derivative) rides in the same launch
      GemmArgs leak;
      if (dX) leak = backward_data_args(cur + row0 * Lr.out, Lr.out, Lr.W, Lr.in, col0, dX, lddx, nrows, Lr.out, ncols, ACT_NONE, nullptr, 0, no_drop());
      CHK(linear_backward_weight_split(cur, Lr.out, rows, fs->wrap, fs->xp, fs->ldxp, fs->cd, fs->adv, fs->ld_adv, Lr.in - fs->cd, Lr.out,
                                       Lr.dW, Lr.db, n.grads_dirty, e->slabs, prec, s, &e->ws[role].sdefer, dX && gt_tuning().leak_rider ? &leak : nullptr, &rode));
      CHK(comm_grads_ready(e, role, Lr.dW, (long)Lr.out * Lr.in + Lr.out, s));
    } else if (want_w) {
      CHK(linear_backward_weight(cur, Lr.out, Xin, ldx, rows, Lr.out, Lr.in, Lr.dW, Lr.db, n.grads_dirty, e->slabs, e->colp, prec, s, &e->ws[role].sdefer,
                                 l > 0 ? &nn : nullptr, &rode));
      CHK(comm_grads_ready(e, role, Lr.dW, (long)Lr.out * Lr.in + Lr.out, s));
      // generator: all layers above the first leave as one message under the first layer's backward; the discriminator's
      // whole gradient (1 MB) is ONE message at the end of its backward pass (a second launch costs more than it hides)
      if (l == 1 && (role == GT_ROLE_G || !e->opt_comm_d_one_msg)) CHK(comm_flush(e, role, s));
    }
    if (l > 0) {
      if (!rode) CHK(launch_gemm(GEMM_NN, nn, prec, s));
      std::swap(cur, other);
    } else if (dX && !rode) {
      CHK(linear_backward_data(cur + row0 * Lr.out, Lr.out, Lr.W, Lr.in, col0, dX, lddx, nrows, Lr.out, ncols, ACT_NONE, nullptr, 0,
                               no_drop(), prec, s));
    }
  }
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// bf16-storage MLP stacks (GT_OPT_MATMUL_BF16; gemm_bf16s.hip.h): activations, dZ, the input images and weight shadows
// live in HBM as bf16, in both orientations; every product is the k-contiguous form.
// ------------------------------------------------------------------------------------------
static bool use_b16(const gt_engine* e, int role) {
  const Net& n = e->net[role];
  if (!e->matmul_bf16 || !n.bound || n.d.arch != GT_ARCH_MLP || (n.d.hidden_dim & 7)) return false;
  return true;
}
// re-made from the caller's float32 parameters before every pass (they may have been stepped, loaded or broadcast since)
static int refresh_shadows(gt_engine* e, int role, bool with_last, hipStream_t s) {
  Net& n = e->net[role];
  auto& sh = e->ws[role].wsh;
  CHK(resize_owned(sh, n.hidden.size() + 1));
  CastJobs jobs;
  jobs.n = 0; jobs.pad_ = 0;
  int blocks = 0;
  auto flush = [&]() -> int {
    CHK(cast_transpose_multi(jobs, blocks, s));
    jobs.n = 0; blocks = 0;
    return GT_OK;
  };
  for (size_t l = 0; l <= n.hidden.size(); ++l) {     // all layers of the network in ONE launch
    if (l == n.hidden.size() && !with_last) break;
    const Lin& L = l < n.hidden.size() ? n.hidden[l] : n.last;
    LinShadow& w = sh[l];
    CHK(w.ensure(L.out, L.in));
    if (jobs.n == CAST_MAX_JOBS) CHK(flush());
    CHK(cast_jobs_add(jobs, blocks, L.W, L.in, L.out, L.in, w.r(), w.ldw, w.t(), w.ldwt));
  }
  return flush();
}
// in_b [rows][ld_in] bf16 -> acts[l] (bf16, + transposed twin when want_t: the weight gradients read it)
static int stack_forward_b16(gt_engine* e, int role, const __bf16* in_b, int ld_in, long rows, const int* passes, int npass, long rows_each,
                             std::vector<DropoutSpec>& specs, bool want_t, hipStream_t s) {
  Net& n = e->net[role];
  std::vector<B16Img>& acts = e->ws[role].actb;
  const std::vector<LinShadow>& wsh = e->ws[role].wsh;
  specs.resize(n.hidden.size());
  CHK(resize_owned(acts, n.hidden.size()));
  const __bf16* cur = in_b;
  int ld = ld_in;
  for (size_t l = 0; l < n.hidden.size(); ++l) {
    const Lin& L = n.hidden[l];
    CHK(acts[l].ensure(rows, L.out, want_t));
    const float* inj = nullptr;
    CHK(stage_injected(e, role, (int)l, passes, npass, rows_each, L.out, &inj, s));
    specs[l] = drop_spec(e, role, passes[0], (int)l, inj, L.out, npass == 2 ? rows_each : 0);
    CHK(b16_forward(cur, ld, rows, wsh[l].r(), wsh[l].ldw, L.out, L.in, L.b, ACT_LEAKY_DROPOUT, specs[l], B16Dst(acts[l], want_t), s));
    cur = acts[l].r();
    ld = acts[l].ld;
  }
  return GT_OK;
}
// dz[cur]: gradient w.r.t. the pre-activation of the TOP hidden layer (both orientations when want_w).  in_t: transposed
// image of the stack input [in][rows8] (weight gradient of layer 0).  dX (float32, optional): d loss / d input columns
// [col0, col0 + ncols) for rows [row0, row0 + nrows).
static int stack_backward_b16(gt_engine* e, int role, const __bf16* in_t, long ld_int, long rows, const std::vector<DropoutSpec>& specs, int cur, bool want_w,
                              float* dX, int lddx, int col0, int ncols, long row0, long nrows, hipStream_t s) {
  Net& n = e->net[role];
  std::vector<B16Img>& acts = e->ws[role].actb;
  const std::vector<LinShadow>& wsh = e->ws[role].wsh;
  for (int l = (int)n.hidden.size() - 1; l >= 0; --l) {
    const Lin& Lr = n.hidden[l];
    B16Img& dz = e->dz_b[cur];
    if (want_w) {
      const __bf16* XT = l > 0 ? acts[l - 1].t() : in_t;
      const long ldxt = l > 0 ? acts[l - 1].ldt : ld_int;
      CHK(weight_grad_b16(dz.t(), dz.ldt, XT, ldxt, rows, Lr.out, Lr.in, Lr.dW, Lr.db, n.grads_dirty, e->slabs, s, &e->ws[role].sdefer));
      CHK(comm_grads_ready(e, role, Lr.dW, (long)Lr.out * Lr.in + Lr.out, s));
      if (l == 1 && (role == GT_ROLE_G || !e->opt_comm_d_one_msg)) CHK(comm_flush(e, role, s));
    }
    if (l > 0) {
      B16Img& nx = e->dz_b[cur ^ 1];
      CHK(nx.ensure(rows, Lr.in, want_w));
      CHK(b16_backward_data(dz.r(), dz.ld, rows, wsh[l].t(), wsh[l].ldwt, Lr.in, Lr.out, ACT_LEAKY_DROPOUT, &acts[l - 1], specs[l - 1],
                            B16Dst(nx, want_w), s));
      cur ^= 1;
    } else if (dX) {
      CHK(b16_backward_data(dz.r() + row0 * dz.ld, dz.ld, nrows, wsh[0].t() + (long)col0 * wsh[0].ldwt, wsh[0].ldwt, ncols, Lr.out, ACT_NONE,
                            nullptr, no_drop(), B16Dst(dX, lddx), s));
    }
  }
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// The output layer of every stack (`last`: an MLP's last_linear, a recurrent network's hidden2out), either storage form
// ------------------------------------------------------------------------------------------
// out [rows][out_dim] (float32) = act(top . W_last^T + b), act = sigmoid iff last_sigmoid
int out_layer_forward(gt_engine* e, int role, const OutTop& top, long rows, float* out, hipStream_t s) {
  const Net& n = e->net[role];
  const Lin& L = n.last;
  const int act = n.d.last_sigmoid ? ACT_SIGMOID : ACT_NONE;
  if (!top.img) return linear_forward(top.x, top.ld, L.W, L.in, L.b, out, n.d.out_dim, rows, L.in, L.out, act, no_drop(), product_prec(e, role), s);
  B16Img& I = *top.img;
  if (!top.img_ready) {
    CHK(I.ensure(rows, L.in, top.want_t));
    CHK(cast_transpose(top.x, top.ld, rows, L.in, I.r(), I.ld, top.want_t ? I.t() : (__bf16*)nullptr, I.ldt, nullptr, false, &e->colp, s));
  }
  return b16_forward(I.r(), I.ld, rows, top.sh->r(), top.sh->ldw, L.out, L.in, L.b, act, no_drop(), B16Dst(out, n.d.out_dim), s);
}
// gy [rows][ldgy] = d loss / d (W_last's product): dW = gy^T top, db, then d loss / d top through dst.  bf16 storage: gy goes to the image
// e->gy_b in both orientations first; the weight gradient reads its and top's transposed twins, backward-data the shadow's wt.
int out_layer_backward(gt_engine* e, int role, const float* gy, int ldgy, long rows, const OutTop& top, const OutGrad& dst, SlabDefer* defer,
                       hipStream_t s) {
  const Net& n = e->net[role];
  const Lin& L = n.last;
  const int Do = n.d.out_dim;
  const bool through_act = dst.act_prev != ACT_NONE;
  if (top.img) {
    B16Img& GY = e->gy_b;
    CHK(GY.ensure(rows, Do, true));
    CHK(cast_transpose(gy, ldgy, rows, Do, GY.r(), GY.ld, GY.t(), GY.ldt, nullptr, false, &e->colp, s));
    CHK(weight_grad_b16(GY.t(), GY.ldt, top.img->t(), top.img->ldt, rows, Do, L.in, L.dW, L.db, n.grads_dirty, e->slabs, s, defer));
    CHK(comm_grads_ready(e, role, L.dW, (long)Do * L.in + Do, s));
    return b16_backward_data(GY.r(), GY.ld, rows, top.sh->t(), top.sh->ldwt, L.in, Do, dst.act_prev, through_act ? top.img : nullptr, dst.drop,
                             dst.to, s);
  }
  const GemmArgs nn = backward_data_args(gy, ldgy, L.W, L.in, 0, dst.to.C, dst.to.ldc, rows, Do, L.in, dst.act_prev, through_act ? top.x : nullptr,
                                         through_act ? top.ld : 0, dst.drop);
  const int prec = product_prec(e, role);
  bool rode = false;
  CHK(linear_backward_weight(gy, ldgy, top.x, top.ld, rows, Do, L.in, L.dW, L.db, n.grads_dirty, e->slabs, e->colp, prec, s, defer,
                             dst.ride ? &nn : nullptr, &rode));
  CHK(comm_grads_ready(e, role, L.dW, (long)Do * L.in + Do, s));
  if (!rode) CHK(launch_gemm(GEMM_NN, nn, prec, s));
  return GT_OK;
}
// what an MLP stack's pass left for its output layer: the top activation, as float32 rows or (bf16 storage, after refresh_shadows(with_last)) as image
static OutTop mlp_top(gt_engine* e, int role, bool b16) {
  const Net& n = e->net[role];
  NetWs& W = e->ws[role];
  OutTop top;
  if (b16) { top.img = &W.actb.back(); top.sh = &W.wsh[n.hidden.size()]; top.img_ready = true; }
  else { top.x = W.act.back().as<float>(); top.ld = n.hidden.back().out; }
  return top;
}

// row pitch of the generator's input / of the conditioning x (gt_set_x_pitch; dense by default)
static int gx_pitch(const gt_engine* e) { return (e->ld_gx > 0 && !e->pass.input_dense()) ? e->ld_gx : e->net[GT_ROLE_G].d.in_dim; }
static int cx_pitch(gt_engine* e) { return e->ld_cx > 0 ? e->ld_cx : cond_dim(e); }
// the generator input as the network can read it: pitched rows (gt_set_x_pitch) stay where they are for the float32 MLP generator;
// every other generator reads a dense copy made here (the copy is also what its backward pass reads: GenPass::input)
static int dense_gx(gt_engine* e, const float** x, long N, hipStream_t s) {
  Net& G = e->net[GT_ROLE_G];
  e->pass.input_dense(false);
  if (e->ld_gx <= 0 || e->ld_gx == G.d.in_dim) return GT_OK;
  if (e->ld_gx < G.d.in_dim) return fail(GT_ERR_INVALID, "gt_set_x_pitch: pitch %d for %d generator input columns", e->ld_gx, G.d.in_dim);
  if (G.d.arch == GT_ARCH_MLP && !use_b16(e, GT_ROLE_G)) return GT_OK;
  CHK(e->gx_dense.ensure((size_t)N * G.d.in_dim * sizeof(float)));
  launch_copy_cols(*x, e->ld_gx, 0, e->gx_dense.as<float>(), G.d.in_dim, 0, N, G.d.in_dim, s);
  LAUNCH_CHECK();
  *x = e->gx_dense.as<float>();
  e->pass.input_dense(true);
  return GT_OK;
}
// the conditioning x of the discriminator passes that cannot read pitched rows (no split first layer): a dense copy, once per step
static int dense_cx(gt_engine* e, const float** x, long N, hipStream_t s) {
  if (!*x || !e->cfg.discriminator_linguistic_condition || e->ld_cx <= 0 || e->ld_cx == cond_dim(e)) return GT_OK;
  const int cd = cond_dim(e);
  if (e->ld_cx < cd) return fail(GT_ERR_INVALID, "gt_set_x_pitch: pitch %d for %d conditioning columns", e->ld_cx, cd);
  return step_copy(e, e->din.cx_dense, *x, e->ld_cx, cd, N, cd, true, x, s);
}

static int generator_forward(gt_engine* e, const float* x, const float* R, int B, int T, float* y_hat, float* y_hat_static,
                             bool stash, hipStream_t s, std::vector<DropoutSpec>& specs) {
  Net& G = e->net[GT_ROLE_G];
  const long N = (long)B * T;
  CHK(dense_gx(e, &x, N, s));
  const int pass0[1] = {0};
  const float* gsrc = y_hat;            // what MLPG is applied to
  if (G.d.arch == GT_ARCH_LSTM) {
    CHK(lstm_forward(e, x, B, T, y_hat, s));
  } else if (G.d.arch == GT_ARCH_IN2OUT_RNN) {
    // G(x) = hidden2out(LSTM(x)) stays internal; the model returns its INPUT as y_hat (models.py:118)
    CHK(e->i2o_gout.ensure((size_t)N * G.d.out_dim * sizeof(float)));
    CHK(lstm_forward(e, x, B, T, e->i2o_gout.as<float>(), s));
    launch_copy_cols(x, G.d.in_dim, 0, y_hat, G.d.in_dim, 0, N, G.d.in_dim, s);
    LAUNCH_CHECK();
    gsrc = e->i2o_gout.as<float>();
  } else if (G.d.arch == GT_ARCH_SRU) {
    CHK(sru_forward(e, x, B, T, y_hat, s));
  } else {
    const bool b16 = use_b16(e, GT_ROLE_G);
    if (b16) {
      const bool want_t = stash && G.d.grads != nullptr;
      CHK(e->xin_b.ensure(N, G.d.in_dim, want_t));
      CHK(cast_transpose(x, G.d.in_dim, N, G.d.in_dim, e->xin_b.r(), e->xin_b.ld, want_t ? e->xin_b.t() : (__bf16*)nullptr, e->xin_b.ldt,
                                nullptr, false, &e->colp, s));
      CHK(refresh_shadows(e, GT_ROLE_G, true, s));
      CHK(stack_forward_b16(e, GT_ROLE_G, e->xin_b.r(), e->xin_b.ld, N, pass0, 1, N, specs, want_t, s));
    } else {
      CHK(stack_forward(e, GT_ROLE_G, x, gx_pitch(e), N, pass0, 1, N, specs, s));
    }
    CHK(out_layer_forward(e, GT_ROLE_G, mlp_top(e, GT_ROLE_G, b16), N, y_hat, s));
  }
  if (is_i2o(G.d.arch)) {
    if (!R) return fail(GT_ERR_INVALID, "In2OutHighwayNet needs the MLPG matrix R (models.py:54)");
    const int sd = G.d.static_dim;
    const MlpgBand* band;
    CHK(ensure_band(e, R, T, s, &band));
    if (stash) e->pass.went_through(band);
    CHK(e->tx.ensure((size_t)N * sd * sizeof(float)));
    CHK(e->gx.ensure((size_t)N * sd * sizeof(float)));
    // T(x) = sigmoid(T x_static), x_static = x[:, :, :static_dim]   (models.py:57-60)
    CHK(linear_forward(x, G.d.in_dim, G.gate.W, sd, G.gate.b, e->tx.as<float>(), sd, N, sd, sd, ACT_SIGMOID, no_drop(), product_prec(e, GT_ROLE_G), s));
    CHK(mlpg_forward(e, gsrc, G.d.out_dim, e->d_scol_i2o.as<int>(), e->d_sstride_i2o.as<int>(), sd, e->gx.as<float>(), sd, B, T, *band, s));
    launch_highway_forward(x, G.d.in_dim, e->tx.as<float>(), sd, e->gx.as<float>(), sd, y_hat_static, sd, N, sd, s);
    LAUNCH_CHECK();
  } else {
    if (G.d.out_dim != e->Dout_cfg)
      return fail(GT_ERR_DIM, "You probably have specified wrong dimention params.");  // multistream.py:93-94
    if (R) {
      const MlpgBand* band;
      CHK(ensure_band(e, R, T, s, &band));
      if (stash) e->pass.went_through(band);
      CHK(mlpg_forward(e, y_hat, G.d.out_dim, e->d_scol.as<int>(), e->d_sstride.as<int>(), e->Ds, y_hat_static, e->Ds, B, T, *band, s));
    } else {
      if (e->Ds != G.d.out_dim) return fail(GT_ERR_INVALID, "R is None but the stream config has dynamic features");
      if (stash) e->pass.went_through(nullptr);
      // R is None: num_windows = 1, every stream passes through (multistream.py:88-89,119-120)
      launch_copy_cols(y_hat, G.d.out_dim, 0, y_hat_static, G.d.out_dim, 0, N, G.d.out_dim, s);
      LAUNCH_CHECK();
    }
  }
  return GT_OK;
}

extern "C" int gt_apply_generator(gt_engine* e, const float* x, const float* R, int B, int T, float* y_hat,
                                  float* y_hat_static, void* stream) {
  CHK(check_common(e, B, T));
  Net& G = e->net[GT_ROLE_G];
  if (!G.bound) return fail(GT_ERR_STATE, "generator not bound");
  if (!x || !y_hat || !y_hat_static) return fail(GT_ERR_INVALID, "null tensor");
  hipStream_t s = (hipStream_t)stream;
  CHK(fault_seen(e));
  e->step_counter++;
  on_new_batch(e);
  CHK(generator_forward(e, x, R, B, T, y_hat, y_hat_static, true, s, e->ws[GT_ROLE_G].specs));
  e->pass.stash(B, T, e->pass.input_dense() ? e->gx_dense.as<float>() : x, y_hat, y_hat_static);
  return GT_OK;
}

// width of the conditioning input x fed to D (train.py:254-256); derived from the bound D when not configured
int cond_dim(gt_engine* e) {
  if (!e->cfg.discriminator_linguistic_condition) return 0;
  if (e->cfg.cond_dim > 0) return e->cfg.cond_dim;
  return e->net[GT_ROLE_D].bound ? e->net[GT_ROLE_D].d.in_dim - e->Da : 0;
}
static int d_in_dim(gt_engine* e) { return e->Da + cond_dim(e); }

// rows [row0, row0+N) of dcat <- [x | feats[:, adv_cols]]   (x: checked by d_pass_plan)
static int build_cat(gt_engine* e, const float* x, const float* feats, int ld_feats, long row0, long N, int ldc, hipStream_t s) {
  float* dst = e->dcat.as<float>() + row0 * ldc;
  const int cd = cond_dim(e);
  if (cd > 0) {
    launch_copy_cols(x, cd, 0, dst, ldc, 0, N, cd, s);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(gather_cols_kernel, dim3(cdiv(N * e->Da, 256)), dim3(256), 0, s, feats, ld_feats, 0, e->d_adv_cols.as<int>(), dst, ldc,
                     cd, (int)N, e->Da);
  LAUNCH_CHECK();
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// the discriminator's tail: launch functions over plain argument blocks (d_tail_args.hip.h), shared by the engine's wrappers below and the
// parity hooks gt_op_d_head / gt_op_dstack (eng_ops.hip).  The whole dispatch lives here; the wrappers only fill the blocks from the engine.
// ------------------------------------------------------------------------------------------
// gt_head_path_counts: process-wide, one relaxed increment per launch on the host (no device work, no synchronisation)
static std::atomic<int64_t> g_head_paths[GT_HEAD_PATH_SLOTS];
void head_path_count(int slot) { g_head_paths[slot].fetch_add(1, std::memory_order_relaxed); }
extern "C" int gt_head_path_counts(int64_t* counts, int reset) {
  for (int i = 0; i < GT_HEAD_PATH_SLOTS; ++i) {
    const int64_t v = reset ? g_head_paths[i].exchange(0, std::memory_order_relaxed) : g_head_paths[i].load(std::memory_order_relaxed);
    if (counts) counts[i] = v;
  }
  return GT_OK;
}

// the pass's per-workgroup partials (o.hp, o.dw_partial: nblk of them) -> the step's scalars and d last_linear
int launch_head_finalize(const HeadCall& c, const HeadSums& o, int nblk, int K, hipStream_t s) {
  const bool w = c.want_grad && c.want_w;
  if (c.defer_scalars && !w) { *c.defer_scalars = nblk; return GT_OK; }
  if (nblk > o.hp_cap || (w && (long)nblk * K > o.dw_cap)) return fail(GT_ERR_INVALID, "discriminator head: partial buffers too small for %d workgroups", nblk);
  const int cgw = (w && nblk >= 512) ? 16 : 64;       // many rows of partials: narrower column groups, more workgroups (frame_kernels.hip.h)
  const int n_dw = cdiv(K, cgw), extra = cgw == 16 ? 1 : 0;       // (with many partials the scalars get a workgroup of their own, beside the dw ones)
  hipLaunchKernelGGL(d_head_finalize_kernel, dim3(n_dw + extra), dim3(1024), 0, s, o.hp, o.dw_partial, nblk, K, c.mode, o.sc,
                     w ? o.dW : (float*)nullptr, w ? o.db : (float*)nullptr, o.accumulate, c.early_res,
                     c.ticket ? o.ticket_dev : (unsigned*)nullptr, c.ticket, cgw, extra ? n_dw : 0);
  LAUNCH_CHECK();
  head_path_count(cgw == 16 ? HEAD_PATH_FINALIZE16 : HEAD_PATH_FINALIZE64);
  return GT_OK;
}

// c.mode HEAD_D_STEP (DSTACK_D_STEP): rows = 2N (natural then generated), writes the stashes a.Hout[1 ..], the seed gradient a.dZtop and the
// head's partials, then finalises them (as launch_d_head does).  HEAD_G_ADV (DSTACK_G_ADV): rows = N, writes a.gadv (want_grad) and the partials.
int launch_dstack_pass(const DStackCall& k, hipStream_t s) {
  const HeadCall& c = k.c;
  const int H = k.hidden_dim;
  const bool d_step = c.mode == HEAD_D_STEP;
  const int nblk = dstack_panels(c.rows);
  if (nblk > k.o.hp_cap || (d_step && c.want_grad && (long)nblk * H > k.o.dw_cap))
    return fail(GT_ERR_INVALID, "fused discriminator stack: partial buffers too small for %d panels", nblk);
  DStackArgs a = k.a;
  a.mode = d_step ? DSTACK_D_STEP : DSTACK_G_ADV; a.rows = (int)c.rows; a.n_real = (int)c.n_real;
  for (int l = 0; l < a.L && l < DS_MAXL; ++l)
    if (a.drop[l].mode == DROP_BUFFER && a.drop[l].ld_mask != H) return fail(GT_ERR_INVALID, "injected dropout mask pitch");
  a.mask = c.mask; a.n_mask = (int)c.n_mask; a.eps = c.eps; a.unit_tv = c.unit_tv ? 1 : 0; a.tv_dev = c.tv_dev;
  a.sc = k.o.sc; a.want_grad = c.want_grad ? 1 : 0; a.hp = k.o.hp;
  a.dw_partial = (d_step && c.want_grad) ? k.o.dw_partial : (float*)nullptr;
  if (!d_step && c.want_grad && !a.gadv) return fail(GT_ERR_INVALID, "fused discriminator stack: no gradient buffer");
  CHK(launch_dstack(a, H, s, c.objective));
  return launch_head_finalize(c, k.o, nblk, H, s);
}

// (the launch templates of the head pass: d_tail_launch.hip.h; objective 0 is instantiated here, 1 .. 3 in eng_gan_objective.hip, 4 .. 6 in eng_gan_fdiv.hip)
int launch_d_head(const HeadArgs& a, hipStream_t s) {
  const int nblk = d_head_blocks(a.c.rows);
  if (nblk > a.o.hp_cap || (long)nblk * a.K > a.o.dw_cap) return fail(GT_ERR_INVALID, "discriminator head: partial buffers too small for %d workgroups", nblk);
  if (a.c.objective == GAN_OBJ_BCE) CHK(head_launch_by_k<GAN_OBJ_BCE>(a, nblk, s));
  else CHK(launch_d_head_objective(a, nblk, s));
  return launch_head_finalize(a.c, a.o, nblk, a.K, s);
}

// the engine's partial buffers (grown to `nblk` workgroups of K columns) and where their sums go
static int head_sums(gt_engine* e, int nblk, int K, bool dw, HeadSums* o) {
  Net& D = e->net[GT_ROLE_D];
  CHK(e->headp.ensure((size_t)nblk * sizeof(HeadPartials)));
  if (dw) CHK(e->headw.ensure((size_t)nblk * K * sizeof(float)));
  o->sc = e->sc();
  o->hp = e->headp.as<HeadPartials>(); o->hp_cap = (long)(e->headp.bytes / sizeof(HeadPartials));
  o->dw_partial = e->headw.as<float>(); o->dw_cap = (long)(e->headw.bytes / sizeof(float));
  o->dW = D.last.dW; o->db = D.last.db; o->accumulate = D.grads_dirty ? 1 : 0;
  o->ticket_dev = e->results.ticket_dev();
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// fused discriminator stack (dstack_f32.hip.h): layers 1 .. L-1 + head (+ the generator step's backward-data chain) in one launch
// ------------------------------------------------------------------------------------------
// rows: frames of the pass.  A panel is walked through all layers by ONE workgroup (about 60 us of latency at 3 x 256): the fused
// launch pays when the pass has at least one panel per CU; below that (per-rank batches of a few sequences) the per-layer launches,
// which spread every layer over all CUs, are faster (b = 4: 0.413 vs 0.417 ms per step).  GT_OPT_FUSED_DSTACK = 2 forces the fused
// path at any size (tests).
static bool d_fused_ok(gt_engine* e, long rows) {
  Net& D = e->net[GT_ROLE_D];
  if (e->opt_fused_dstack < 2 && dstack_panels(rows) < gemm_cu_count()) return false;
  if (!e->opt_fused_dstack || D.d.arch != GT_ARCH_MLP || product_prec(e, GT_ROLE_D) != PREC_F32 || !dstack_hidden_ok(D.d.hidden_dim)) return false;
  if (D.hidden.empty() || (int)D.hidden.size() > DS_MAXL || D.last.out != 1 || e->Da < 1 || e->Da > 64) return false;
  for (size_t l = 0; l < D.hidden.size(); ++l)
    if (D.hidden[l].out != D.d.hidden_dim || (l > 0 && D.hidden[l].in != D.d.hidden_dim)) return false;
  return true;
}
// the fused pass over the engine's discriminator (launch_dstack_pass): the stashes go to the discriminator's act[1 ..], the seed gradient to e->dzA
static int run_dstack(gt_engine* e, const HeadCall& c, float* gadv, hipStream_t s) {
  Net& D = e->net[GT_ROLE_D];
  NetWs& W = e->ws[GT_ROLE_D];
  const int H = D.d.hidden_dim, L = (int)D.hidden.size();
  const bool d_step = c.mode == HEAD_D_STEP;
  DStackCall k;
  memset(&k, 0, sizeof(k));
  k.c = c; k.hidden_dim = H;
  CHK(head_sums(e, dstack_panels(c.rows), H, d_step && c.want_grad, &k.o));
  CHK(e->dout.ensure((size_t)c.rows * sizeof(float)));
  DStackArgs& a = k.a;
  a.L = L;
  a.H0 = W.act[0].as<float>();
  for (int l = 0; l < L; ++l) { a.W[l] = D.hidden[l].W; a.b[l] = D.hidden[l].b; a.drop[l] = W.specs[l]; }
  a.w_last = D.last.W; a.b_last = D.last.b; a.Dout = e->dout.as<float>();
  if (d_step) {
    for (int l = 1; l + 1 < L; ++l) a.Hout[l] = W.act[l].as<float>();      // (the top layer's activation only feeds the head, which is fused: no stash)
    a.dZtop = e->dzA.as<float>();
    if (e->gp.kind == GP_R1 && c.want_grad && L > 1) a.Hout[L - 1] = W.act[L - 1].as<float>();      // R1 recovers the top layer's slopes from it (d_pass_penalty)
  } else {
    a.W0 = D.hidden[0].W; a.ldw0 = D.hidden[0].in; a.col0 = cond_dim(e); a.Da = e->Da; a.gadv = gadv; a.ld_gadv = e->Da;
  }
  return launch_dstack_pass(k, s);
}

// what the per-layer head reads and where its seed gradient goes
struct HeadAct {
  const void* H; int K;        // the top hidden activation, float32 [rows][K] ...
  int h_ld;                    // ... or (h_ld > 0) its bf16 image with row pitch h_ld
  bool has_act;                // H is LeakyReLU + dropout of a pre-activation (MLP); false: a recurrent stack's output
  DropoutSpec spec;            // the top layer's dropout site
  float* dH;                   // float32 seed gradient, or
  B16Img* dz_img; bool dz_t;   // (bf16 storage) the top dZ image, transposed twin too when dz_t
};
// the per-layer head over the engine's discriminator (launch_d_head)
static int run_head(gt_engine* e, const HeadCall& c, const HeadAct& a, hipStream_t s) {
  Net& D = e->net[GT_ROLE_D];
  HeadArgs h;
  memset(&h, 0, sizeof(h));
  h.c = c;
  CHK(head_sums(e, d_head_blocks(c.rows), a.K, true, &h.o));
  CHK(e->dout.ensure((size_t)c.rows * sizeof(float)));
  B16Img* z = a.h_ld > 0 ? a.dz_img : nullptr;
  h.H = a.H; h.K = a.K; h.ldh = a.K; h.h_ld = a.h_ld; h.has_act = a.has_act; h.spec = a.spec;
  h.w = D.last.W; h.bias = D.last.b; h.Dout = e->dout.as<float>();
  h.dH = z ? (float*)nullptr : a.dH; h.lddh = a.K;
  if (z) { h.dHb = z->r(); h.lddhb = z->ld; if (a.dz_t) { h.dHbT = z->t(); h.lddhbt = z->ldt; } }
  return launch_d_head(h, s);
}

static int optimizer_step(gt_engine* e, int role, double* norm2_out, hipStream_t s) {
  Net& n = e->net[role];
  if (!n.has_opt) return fail(GT_ERR_STATE, "phase == \"train\" but no optimizer is bound for role %d", role);
  const long np = n.d.n_params;
  CHK(e->partial.ensure(4096 * sizeof(double)));
  double* part = e->partial.as<double>() + 2048;
  unsigned int* skipped = e->h_fault_dev ? e->h_fault_dev + 1 + role : (unsigned int*)nullptr;
  // the discriminator's gradient of a GT_OPT_COMM_TV_IN_SUMS step is that of the unnormalised loss: x 1 / Tv in the update kernel
  const float* gscale = role == GT_ROLE_D ? e->norm.take_d_scale(e->sc()) : (const float*)nullptr;
  SlabDefer& sd = e->ws[role].sdefer;
  int n_partial = 0;      // squared-norm partials in `part`: none until one of the routes below has launched them
  if (role == GT_ROLE_D && e->sn.on) {
    // gt_set_spectral_norm: the flat gradient holds d loss / d W_eff.  Combines first, then the projection onto the caller's W, whose element
    // pass leaves the squared-norm partials of the whole projected gradient: clip-norm and the update see d loss / d W
    CHK(slab_defer_flush(sd, s));
    sd.active = false;
    CHK(sn_project_grads(e, part, &n_partial, s));
  } else if (sd.active && sd.jobs.n > 0) {
    // The fused step recorded this network's weight-gradient combines.  They write disjoint ranges of the flat gradient; whatever
    // they do not cover (the discriminator's last layer, written by the head's reduction) still counts for the norm and is
    // stepped: `rest`.  Combines + squared norm in ONE launch (slab_reduce_norm_kernel), then clip + step.
    std::vector<std::pair<long, long>> cov;
    bool ok = true;
    for (int q = 0; q < sd.jobs.n && ok; ++q) {
      const SlabJob& J = sd.jobs.j[q];
      const long o0 = J.out - n.d.grads;
      if (o0 < 0 || o0 + J.n4 * 4 > np) ok = false;
      cov.push_back(std::make_pair(o0, J.n4 * 4));
      if (J.bout && J.main_blocks < (q + 1 < sd.jobs.n ? sd.jobs.j[q + 1].block0 : sd.blocks) - J.block0) {
        const long b0 = J.bout - n.d.grads;
        if (b0 < 0 || b0 + J.nb > np) ok = false;
        cov.push_back(std::make_pair(b0, (long)J.nb));
      }
    }
    std::sort(cov.begin(), cov.end());
    OptimRest rest;
    memset(&rest, 0, sizeof(rest));
    long pos = 0, rest_total = 0;
    for (size_t i = 0; i <= cov.size() && ok; ++i) {
      const long next = i < cov.size() ? cov[i].first : np;
      if (next < pos) { ok = false; break; }                       // overlapping jobs: not this path
      if (next > pos) {
        if (rest.n_rest == OPTIM_REST_MAX) { ok = false; break; }
        rest.off[rest.n_rest] = pos; rest.n[rest.n_rest] = next - pos; ++rest.n_rest;
        rest_total += next - pos;
      }
      if (i < cov.size()) pos = cov[i].first + cov[i].second;
    }
    const int rest_blocks = rest_total > 0 ? (int)std::min<long>(64, cdiv(rest_total, 256)) : 0;
    if (ok && sd.blocks + rest_blocks <= 2048) {
      hipLaunchKernelGGL(slab_reduce_norm_kernel, dim3(sd.blocks + rest_blocks), dim3(256), 0, s, sd.jobs, sd.blocks, rest, n.d.grads, part);
      LAUNCH_CHECK();
      n_partial = sd.blocks + rest_blocks;
      sd.reset(false);
    }
  }
  if (!n_partial) {
    n_partial = (int)std::min<long>(512, cdiv(np, RED_THREADS * 4));
    CHK(slab_defer_flush(sd, s));            // the fused step's recorded weight-gradient combines, one launch
    sd.active = false;
    hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(n_partial), dim3(RED_THREADS), 0, s, n.d.grads, np, part);
    LAUNCH_CHECK();
  }
  n.step += 1;
  // gt_set_param_ema: the generator's weight average rides this launch; its first applied update copies, every later one is a lerp
  float* ema = role == GT_ROLE_G ? e->ema.buf : (float*)nullptr;
  CHK(launch_optim_step(n.od, n.step, n.buf_live, &n.hs_cache, n.d.params, n.d.grads, np, part, n_partial, norm2_out,
                        e->fault_dev(), e->h_fault_dev, skipped, gscale, s, e->weight_clip[role], ema,
                        param_ema_weight(e->ema.decay), e->ema.count == 0));
  if (ema) e->ema.count += 1;
  n.buf_live = true;
  return GT_OK;
}

// ResultsChannel (engine_internal.hip.h): how a step's scalars reach the host
int ResultsChannel::create(StepResults* device_results, const bool* poll_option) {
  static_assert(sizeof(StepResults) <= 64, "the result ticket sits 64 bytes behind the results");
  d_res = device_results; poll = poll_option;
  CHK(h_res.alloc(128));
  memset(h_res, 0, 128);
  if (hipHostGetDevicePointer((void**)&h_res_dev, h_res, 0) != hipSuccess) { (void)hipGetLastError(); h_res_dev = nullptr; }
  if (!env_flag("GT_RES_HOSTMAP", true)) h_res_dev = nullptr;      // (measurement: results through a device -> host copy instead)
  return GT_OK;
}
int ResultsChannel::post_deferred(int role, hipStream_t s) {
  if (!h_def[role]) CHK(h_def[role].alloc(sizeof(StepResults)));
  CHK(ev_def[role].ensure(hipEventDisableTiming));
  HIPCHK(hipMemcpyAsync(h_def[role], d_res, sizeof(StepResults), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(ev_def[role], s));
  def_pending[role] = true;
  return GT_OK;
}
int ResultsChannel::wait_early() {
  ++waits;
  if (ticket_wait) {
    volatile unsigned* t = ticket_host();
    const unsigned want = ticket_wait;
    ticket_wait = 0;
    unsigned long spins = 0;
    std::chrono::steady_clock::time_point t0;
    while (__atomic_load_n((const unsigned*)t, __ATOMIC_ACQUIRE) != want) {
      __builtin_ia32_pause();
      if ((++spins & 0xfffff) == 0) {      // a kernel that died never writes the ticket: give up after a minute
        if (spins == 0x100000) t0 = std::chrono::steady_clock::now();
        else if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 60.0) {
          HIPCHK(hipDeviceSynchronize());
          return fail(GT_ERR_HIP, "the step's results never arrived in host memory");
        }
      }
    }
  } else HIPCHK(hipEventSynchronize(ev_res));
  early_done = false;
  return GT_OK;
}
int ResultsChannel::post_early(hipStream_t s, unsigned ticket) {
  ticket_wait = ticket;
  if (!ticket) {
    CHK(ev_res.ensure(hipEventDisableTiming));
    if (!h_res_dev) HIPCHK(hipMemcpyAsync(h_res, d_res, sizeof(StepResults), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(ev_res, s));
  }
  early_done = true;
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// one pass through the discriminator: the D step (natural then generated rows, weight gradients) and the adversarial term of the
// generator step (generated rows, backward-data only) are the same four stages over a DPass that d_pass_plan() fills once
// ------------------------------------------------------------------------------------------
// the split first layer (FirstSplit) applies to the conditioned float32 MLP discriminator
static bool d_split_ok(gt_engine* e, const float* x) {
  return e->opt_split_first && product_prec(e, GT_ROLE_D) == PREC_F32 && e->cfg.discriminator_linguistic_condition && x && cond_dim(e) > 0 &&
         e->Da > 0 && gemm_small_tiles_ok() && (e->net[GT_ROLE_D].d.hidden_dim & 3) == 0;     // (dZ as a 16-byte loadable operand)
}
// A recurrent discriminator (LSTMRNN / SRURNN in the discriminator slot, train.py:773-774) runs the natural and the generated sequences of
// a D step as ONE batch of 2B sequences through its stack; the fused head reads the top layer's output (hidden2out is its weight).
enum DKind { D_MLP_F32, D_MLP_B16, D_LSTM, D_SRU };
struct DPass {
  DKind kind;
  bool split;                  // D_MLP_F32: split first layer, no image of x (fs)
  bool fused;                  // D_MLP_F32: layers 1 .. L-1 + the head (+ the G step's backward-data chain) as ONE launch (dstack_f32.hip.h)
  bool sru_d16;                // D_SRU under GT_OPT_SRU_D_BF16: the stack writes layer 0's bf16 images straight from cat0
  bool needs_f32_image;        // the float32 [x | adv] image is read (every float32 route but the split one; an SRU-bf16 layer 0 with k == 3)
  bool want_w;                 // weight gradients follow: transposed images, pitched x
  int passes[2], npass;        // dropout passes: {0, 1} for the D step, {2} for the adversarial term
  long N, rows;                // frames of the batch; rows of the pass = npass * N
  int B, nseq, T, K0, ldc, H;  // nseq = npass * B; K0 = D's in_dim, ldc its image's pitch; H: width of what the head reads
  const float* x;              // conditioning input (d_pass_input: its dense copy unless split)
  const float* real; const float* fake; int ldf;      // y_static (D step only), y_hat_static, their pitch
  FirstSplit fs;               // split
  CatSrc cat0;                 // D_MLP_B16, sru_d16: the rows of the pass as [x | feats[:, adv_cols]]
  const float* img;            // needs_f32_image: the pass's rows of e->dcat (d_pass_input)
  const float* top; int ld_top;      // recurrent: the stack's output (d_pass_forward)
};
static int d_pass_plan(gt_engine* e, const float* x, const float* real, const float* fake, int ldf, int npass, int B, int T, bool want_w, DPass* out) {
  Net& D = e->net[GT_ROLE_D];
  if (D.d.in_dim != d_in_dim(e))
    return fail(GT_ERR_DIM, "discriminator in_dim %d != adversarial input width %d (train.py:760-768)", D.d.in_dim, d_in_dim(e));
  const int cd = cond_dim(e);
  if (e->cfg.discriminator_linguistic_condition) {
    if (!x) return fail(GT_ERR_INVALID, "discriminator_linguistic_condition is set but x is null");
    if (cd <= 0) return fail(GT_ERR_DIM, "discriminator in_dim too small for linguistic conditioning");
  }
  DPass& p = *out;
  memset(&p, 0, sizeof(p));
  p.kind = D.d.arch == GT_ARCH_SRU ? D_SRU : has_lstm_body(D.d.arch) ? D_LSTM : use_b16(e, GT_ROLE_D) ? D_MLP_B16 : D_MLP_F32;
  p.npass = npass; p.passes[0] = npass == 2 ? 0 : 2; p.passes[1] = 1;
  p.B = B; p.T = T; p.N = (long)B * T; p.rows = npass * p.N; p.nseq = npass * B;
  p.K0 = D.d.in_dim; p.ldc = (p.K0 + 3) & ~3; p.H = D.d.hidden_dim;
  p.want_w = want_w; p.x = x; p.real = real; p.fake = fake; p.ldf = ldf;
  p.split = p.kind == D_MLP_F32 && d_split_ok(e, x);
  p.fused = p.kind == D_MLP_F32 && d_fused_ok(e, p.rows);
  p.sru_d16 = p.kind == D_SRU && sru_b16(e, GT_ROLE_D);
  p.needs_f32_image = p.kind == D_LSTM || (p.kind == D_SRU && sru_d_needs_f32_input(e)) || (p.kind == D_MLP_F32 && !p.split);
  if (p.split) { p.fs.x = x; p.fs.ldx = cx_pitch(e); p.fs.cd = cd; p.fs.ld_adv = (e->Da + 3) & ~3; p.fs.wrap = p.N; }
  CatSrc& c = p.cat0;
  c.x = x; c.cd = cd; c.fa = npass == 2 ? real : fake; c.fb = fake; c.ldf = ldf; c.idx = e->d_adv_cols.as<int>(); c.N = p.N; c.row_off = npass == 2 ? 0 : p.N;
  return GT_OK;
}

// How Tv = sum(mask) and 1 / Tv reach the discriminator step's head and its gradient consumers: decided once, at the top of
// gt_update_discriminator_begin, from what LossNormaliser knows.  F: a fused call with GT_OPT_LAUNCH_RIDERS; S: GT_OPT_COMM_TV_IN_SUMS in a
// step that trains through a bound optimizer (`steps`).
//   the scalars hold it | communicator | the caller's | F   | S   | route     | the (local) sum                                   | the head's normaliser
//   yes                 |              |              |     |     | KNOWN     | --                                                | the scalars
//   no                  | no           |              | no  |     | LOCAL     | mask_sum launch in front of the head              | the scalars
//   no                  | no           |              | yes |     | LOCAL     | split: rider (*), else as the row above           | the scalars
//   no                  | yes          | yes          |     |     | LOCAL     | mask_sum launch in front of the head              | the scalars
//   no                  | yes          | no           | no  |     | ALLREDUCE | mask_total launch in front of the input           | riders on: the message; else the scalars (mask_sum launch)
//   no                  | yes          | no           | yes | no  | ALLREDUCE | split: rider, else mask_total launch              | the message
//   no                  | yes          | no           | yes | yes | IN_SUMS   | split: rider, else mask_total launch; into tv_sum | none: unit seeds, 1 / Tv where the gradient is consumed
// rider: one extra workgroup of the adversarial-column gather (split first layer), `ride`.  (*) takes the override, not a device total.
// ALLREDUCE: the message is sent by before_input or rode and joined by before_head -- in flight only between the two, inside this one call.
// The generator step takes none of these routes: one LossNormaliser::ensure.
struct TvPlan {
  enum Route { KNOWN, LOCAL, ALLREDUCE, IN_SUMS } route;
  bool ride, head_reads;      // head_reads (ALLREDUCE): the head takes the count where the collective left it and files it in the scalars
  const float* mask; long N;
  TvPlan(gt_engine* e, const DPass& p, const float* mask_, bool steps) : mask(mask_), N(p.N) {
    const bool comm = comm_on(e), fused = e->results.early && e->opt_launch_riders;
    route = e->norm.known(mask, N) ? KNOWN : !comm || e->norm.given() ? LOCAL : fused && e->opt_comm_tv_in_sums && steps ? IN_SUMS : ALLREDUCE;
    ride = p.split && (route == IN_SUMS || (route == ALLREDUCE && fused) || (route == LOCAL && fused && !comm));
    head_reads = e->opt_launch_riders;
  }
  int before_input(gt_engine* e, hipStream_t s) const {      // the local sum as a launch of its own, where a message or the loss sums carry it
    if (ride || route == KNOWN || route == LOCAL) return GT_OK;
    if (route == ALLREDUCE) return e->norm.start(e, mask, N, s);      // (the all-reduce then runs under the forward pass)
    launch_mask_total(mask, N, &e->sc()->tv_sum, s);
    LAUNCH_CHECK();
    return GT_OK;
  }
  void ride_on(gt_engine* e, BuildAdvArgs& ba) const {      // ... or as a rider of the gather launch
    ba.tv_mask = ride ? mask : (const float*)nullptr; ba.tv_n = N; ba.tv_override = e->norm.override(); ba.sc = e->sc();
    ba.tv_total = !ride || route == LOCAL ? (double*)nullptr : route == IN_SUMS ? &e->sc()->tv_sum : e->norm.reduced();
  }
  int rode(gt_engine* e, hipStream_t s) const {
    if (ride && route == LOCAL) e->norm.note(mask, N);
    return ride && route == ALLREDUCE ? e->norm.send(e, s) : GT_OK;      // on the communicator's stream, joined in front of the head
  }
  int before_head(gt_engine* e, HeadCall& hc, hipStream_t s) const {
    LossNormaliser& n = e->norm;
    hc.unit_tv = route == IN_SUMS;
    switch (route) {
      case KNOWN: return GT_OK;
      case LOCAL: return n.ensure(e, mask, N, s);      // (a no-op behind the rider)
      case ALLREDUCE:
        CHK(n.join(e, s));
        if (!head_reads) return n.file(e, mask, N, n.reduced(), s);
        hc.tv_dev = n.reduced();      // no conversion launch between the join and the head
        break;
      case IN_SUMS: break;      // the normaliser arrives with the sums (finalize_d_kernel on the communicator's stream files it); valid from the join on
    }
    n.note(mask, N);
    return GT_OK;
  }
  // what the early results' collective carries: the four loss / count sums, with the count in front of them under IN_SUMS
  double* early_sums(StepScalars* sc) const { return route == IN_SUMS ? &sc->tv_sum : &sc->s_real; }      int n_early_sums() const { return route == IN_SUMS ? 5 : 4; }
};
// What the backend reads: the float32 [x | adv] image, its bf16 image (transposed twin too when want_w), the adversarial columns alone
// (split), or nothing (an SRU-bf16 discriminator that does not read float32 rows).  The D step writes both halves; the adversarial term
// writes the generated half (rows N .. 2N of the same buffers) unless the D step of the same batch left it there.
static int d_pass_input(gt_engine* e, DPass& p, const TvPlan* tv /* the D step's, else null */, hipStream_t s) {
  const long N = p.N;
  const bool both = p.npass == 2;
  const long row0 = both ? 0 : N;
  if (!p.split) {        // pitched rows are read in place by the split first layer only
    CHK(dense_cx(e, &p.x, N, s));
    p.cat0.x = p.x;
  }
  if (both) e->din.invalidate_d_images();
  if (p.kind == D_MLP_B16) {
    CHK(e->dcat_b.ensure(2 * N, p.K0, p.want_w));
    if (both || !e->din.img_cat_b.holds(p.x, p.fake)) {
      CHK(cat_cast_transpose(p.cat0, p.rows, p.K0, e->dcat_b.r() + row0 * e->dcat_b.ld, e->dcat_b.ld, p.want_w ? e->dcat_b.t() : (__bf16*)nullptr,
                             p.want_w ? e->dcat_b.ldt : 0L, s));
      e->din.img_cat_b.built(p.x, p.fake);
    }
  } else if (p.split) {
    // only the adversarial columns are gathered (58 of 483 columns at cfg2)
    const int ld = e->ld_adv2 = p.fs.ld_adv;
    CHK(e->adv2.ensure((size_t)2 * N * ld * sizeof(float)));
    float* dst = e->adv2.as<float>() + row0 * ld;
    if (both || !e->din.img_adv2.holds(nullptr, p.fake)) {
      BuildAdvArgs ba;
      memset(&ba, 0, sizeof(ba));
      ba.fa = p.cat0.fa; ba.fb = p.cat0.fb; ba.ldf = p.ldf; ba.idx = e->d_adv_cols.as<int>(); ba.na = e->Da; ba.out = dst; ba.ldo = ld; ba.split = N; ba.rows = p.rows;
      if (tv) tv->ride_on(e, ba);
      launch_build_adv(ba, s);
      LAUNCH_CHECK();
      if (tv) CHK(tv->rode(e, s));
      e->din.img_adv2.built(nullptr, p.fake);
    }
    p.fs.adv = dst;
    if (p.want_w) CHK(pitched_rows(e, e->din.dx_pitched, p.x, p.fs.ldx, p.fs.cd, N, &p.fs.xp, &p.fs.ldxp, s));
  } else if (p.needs_f32_image) {
    CHK(e->dcat.ensure((size_t)2 * N * p.ldc * sizeof(float)));
    if (both && p.cat0.cd > 0) {
      launch_build_cat2(p.x, p.cat0.cd, p.real, p.fake, p.ldf, e->d_adv_cols.as<int>(), e->Da, e->dcat.as<float>(), p.ldc, N, s);
      LAUNCH_CHECK();
    } else {
      if (both) CHK(build_cat(e, p.x, p.real, p.ldf, 0, N, p.ldc, s));
      if (both || !e->din.img_cat.holds(p.x, p.fake)) CHK(build_cat(e, p.x, p.fake, p.ldf, N, N, p.ldc, s));
    }
    e->din.img_cat.built(p.x, p.fake);
    p.img = e->dcat.as<float>() + row0 * p.ldc;
  }
  return GT_OK;
}

// the stack forward; a recurrent stack leaves its output in p.top / p.ld_top (= p.H)
static int d_pass_forward(gt_engine* e, DPass& p, hipStream_t s) {
  CHK(sn_prepare_pass(e, s));      // gt_set_spectral_norm: W_eff of this pass, ahead of every reader of Lin::W (refresh_shadows and w0pad included)
  switch (p.kind) {
    case D_SRU:        // (sequence lengths ignored as in the reference)
      CHK(sru_stack_forward(e, GT_ROLE_D, p.img, p.ldc, p.nseq, p.T, p.passes, p.npass, s, &p.top, &p.ld_top, p.sru_d16 ? &p.cat0 : nullptr, p.want_w));
      p.H = p.ld_top;
      break;
    case D_LSTM:
      CHK(lstm_check_lengths(e, p.B, p.T));
      CHK(lstm_stack_forward(e, GT_ROLE_D, p.img, p.ldc, p.nseq, p.T, p.passes, p.npass, s, &p.top, &p.ld_top));
      p.H = p.ld_top;
      break;
    case D_MLP_B16:
      CHK(refresh_shadows(e, GT_ROLE_D, false, s));        // (G step: D has just been stepped, train.py:276 before :307)
      CHK(stack_forward_b16(e, GT_ROLE_D, e->dcat_b.r() + (p.npass == 2 ? 0 : p.N) * e->dcat_b.ld, e->dcat_b.ld, p.rows, p.passes, p.npass, p.N,
                            e->ws[GT_ROLE_D].specs, p.want_w, s));
      break;
    case D_MLP_F32:      // fused: layer 0 alone, the fused stack launch (d_pass_head) takes over from there
      CHK(stack_forward(e, GT_ROLE_D, p.img, p.ldc, p.rows, p.passes, p.npass, p.N, e->ws[GT_ROLE_D].specs, s, p.split ? &p.fs : nullptr, p.fused ? 1 : 1 << 30));
      break;
  }
  return GT_OK;
}

// the head on what the stack left, seeding the backward pass where that backend's stack backward reads it (c.want_grad).
// dst: where the fused launch of the adversarial term writes the generated rows' adversarial-column gradient (it IS that pass's backward).
static int d_pass_head(gt_engine* e, DPass& p, const HeadCall& c_in, float* dst, hipStream_t s) {
  const int H = p.H;
  NetWs& W = e->ws[GT_ROLE_D];
  CHK(e->dzA.ensure((size_t)2 * p.N * std::max(H, 1) * sizeof(float)));
  CHK(e->dzB.ensure((size_t)2 * p.N * std::max(H, 1) * sizeof(float)));
  HeadCall c = c_in;
  c.objective = e->gan_objective;      // the one place a pass learns the engine's objective: every discriminator kind reaches its head from here
  if (p.fused) return run_dstack(e, c, p.npass == 1 ? dst : nullptr, s);
  HeadAct a;
  memset(&a, 0, sizeof(a));
  a.K = H; a.has_act = true; a.dH = e->dzA.as<float>();
  switch (p.kind) {
    case D_SRU: case D_LSTM:
      CHK(W.dout.ensure((size_t)2 * p.rows * H * sizeof(float)));
      a.H = p.top; a.has_act = false; a.spec = no_drop(); a.dH = W.dout.as<float>();
      break;
    case D_MLP_B16:      // the head writes its seed gradient as the top dZ image (both orientations for the weight gradients)
      a.H = W.actb.back().r(); a.h_ld = W.actb.back().ld; a.spec = W.specs.back();
      if (c.want_grad) { CHK(e->dz_b[0].ensure(p.rows, H, p.want_w)); a.dz_img = &e->dz_b[0]; a.dz_t = p.want_w; }
      break;
    case D_MLP_F32:
      a.H = W.act.back().as<float>(); a.spec = W.specs.back();
      break;
  }
  return run_head(e, c, a, s);
}

// the stack backward (phase == "train"): weight gradients when p.want_w, and the gradient w.r.t. the generated rows' adversarial columns
// -> dst [N][Da] (the kept leak of the D step, may be null; gadv of the adversarial term)
static int d_pass_backward(gt_engine* e, DPass& p, float* dst, hipStream_t s) {
  if (p.fused && p.npass == 1) return GT_OK;      // done inside the fused launch
  const long N = p.N, row0 = p.npass == 2 ? N : 0;      // the generated rows of the pass
  const int col0 = cond_dim(e), Da = e->Da;
  switch (p.kind) {
    case D_SRU:
      return sru_stack_backward(e, GT_ROLE_D, p.img, p.ldc, p.nseq, p.T, p.passes, p.npass, p.want_w, dst, s);
    case D_LSTM: {     // the gradient w.r.t. the [x | adv] rows, then its generated rows' adversarial columns (train.py:265, 274, 307-308)
      float* dx0 = nullptr;
      if (dst) { CHK(e->d_dx0.ensure((size_t)2 * N * p.K0 * sizeof(float))); dx0 = e->d_dx0.as<float>(); }
      CHK(lstm_stack_backward(e, GT_ROLE_D, p.img, p.ldc, p.nseq, p.T, p.passes, p.npass, p.want_w, dx0, s));
      if (dst) {
        launch_copy_cols(dx0 + row0 * p.K0, p.K0, col0, dst, Da, 0, N, Da, s);
        LAUNCH_CHECK();
      }
      return GT_OK;
    }
    case D_MLP_B16:
      return stack_backward_b16(e, GT_ROLE_D, p.want_w ? e->dcat_b.t() : (__bf16*)nullptr, p.want_w ? e->dcat_b.ldt : 0, p.rows, e->ws[GT_ROLE_D].specs, 0,
                                p.want_w, dst, Da, col0, Da, row0, N, s);
    case D_MLP_F32:
      return stack_backward(e, GT_ROLE_D, p.img, p.ldc, p.rows, e->ws[GT_ROLE_D].specs, e->dzA.as<float>(), e->dzB.as<float>(), p.want_w, dst, Da, col0, Da,
                            row0, N, s, p.split ? &p.fs : nullptr);
  }
  return GT_OK;
}

// gt_set_grad_penalty: the second-order pass behind the D step's backward pass (eng_grad_penalty.hip), its weight gradients added to what
// that pass left.  R1 penalises the natural rows, whose activations and dropout sites (pass 0) the forward pass stored; WGAN-GP runs one
// more forward (dropout pass 3, per-layer launches) over x_hat = eps real + (1 - eps) fake, written over the natural half of the pass's
// input image.  Scratch: the generated rows' half of every stored activation (a_l), dzA / dzB (c_l, alternating) -- all dead by now.
static int d_pass_penalty(gt_engine* e, DPass& p, const float* mask, hipStream_t s) {
  GpState& G = e->gp;
  if (G.kind == GP_OFF) return GT_OK;
  Net& D = e->net[GT_ROLE_D];
  NetWs& W = e->ws[GT_ROLE_D];
  const long N = p.N;
  const int L = (int)D.hidden.size(), H = D.d.hidden_dim, cd = cond_dim(e), Da = e->Da, ld_g = (Da + 3) & ~3;
  if (p.kind != D_MLP_F32 || L < 1 || Da < 1) return fail(GT_ERR_INVALID, "gradient penalty: float32 MLP discriminator only");
  CHK(slab_defer_flush(W.sdefer, s));      // the backward pass's recorded combines land before anything is added to their results
  G.stream = s;
  if (G.kind == GP_WGAN) {
    float* img = p.split ? e->adv2.as<float>() : e->dcat.as<float>();
    const int ldo = p.split ? p.fs.ld_adv : p.ldc, col0 = p.split ? 0 : cd;
    uint32_t k0, k1;
    gp_eps_keys(e, &k0, &k1);
    CHK(G.eps.ensure((size_t)N * sizeof(float)));
    CHK(launch_gp_interp(p.real, p.fake, p.ldf, e->d_adv_cols.as<int>(), Da, G.eps_inj, k0, k1, img, ldo, col0, N, G.eps.as<float>(), s));
    G.img = img; G.img_ld = ldo; G.img_col0 = col0; G.img_rows = N;
    const int pass3[1] = {3};
    CHK(stack_forward(e, GT_ROLE_D, p.img, p.ldc, N, pass3, 1, N, W.specs, s, p.split ? &p.fs : nullptr));
  }
  CHK(G.g.ensure((size_t)N * ld_g * sizeof(float)));
  CHK(G.dw0.ensure((size_t)H * Da * sizeof(float)));
  const int nblk = gp_row_blocks(N);
  CHK(G.part.ensure((size_t)2 * nblk * sizeof(double)));
  GpCall c;
  memset(&c, 0, sizeof(c));
  c.L = L; c.cd = cd; c.Da = Da; c.kind = G.kind; c.prec = product_prec(e, GT_ROLE_D); c.weight = G.weight; c.rows = N;
  for (int l = 0; l < L; ++l) {
    const Lin& Lr = D.hidden[l];
    if (Lr.out != H) return fail(GT_ERR_INVALID, "gradient penalty: hidden layers of one width only");
    GpLayer& q = c.l[l];
    q.W = Lr.W; q.dW = Lr.dW; q.in = Lr.in; q.out = Lr.out;
    q.H = W.act[l].as<float>(); q.spec = W.specs[l];
    q.a = W.act[l].as<float>() + N * (long)Lr.out;
    q.c = (l & 1) ? e->dzB.as<float>() : e->dzA.as<float>();
  }
  c.w_last = D.last.W; c.dw_last = D.last.dW;
  c.g = G.g.as<float>(); c.ld_g = ld_g;
  c.mask = mask; c.inv_tv_dev = LossNormaliser::inv_tv(e->sc());
  c.part = G.part.as<double>(); c.part_cap = (long)(G.part.bytes / sizeof(double));
  c.rec = G.rec.as<double>();
  c.dw0s = G.dw0.as<float>();
  c.slabs = &e->slabs; c.colp = &e->colp;
  return launch_grad_penalty(c, s);
}

// ------------------------------------------------------------------------------------------
// update_discriminator
// ------------------------------------------------------------------------------------------
// keep dloss_d/dy_hat_static only when y_hat_static is the tensor apply_generator produced (the autograd graph in the reference,
// train.py:265) and a generator with grads exists
int KeptLeak::claim(gt_engine* e, const float* y_hat_static, long N, float** out) {
  const Net& G = e->net[GT_ROLE_G];
  *out = nullptr;
  if (!(G.bound && G.d.grads && e->pass.made(y_hat_static, N))) return GT_OK;
  if (pending) return fail(GT_ERR_STATE, "update_discriminator called twice without optimizer_g.zero_grad() (train.py:538)");
  CHK(buf.ensure((size_t)N * e->Da * sizeof(float)));
  *out = buf.as<float>();
  return GT_OK;
}

extern "C" int gt_update_discriminator_begin(gt_engine* e, const float* x, const float* y_static, const float* y_hat_static,
                                             const float* mask, int B, int T, int train, float eps, void* stream) {
  CHK(check_common(e, B, T));
  Net& D = e->net[GT_ROLE_D];
  if (!D.bound) return fail(GT_ERR_STATE, "discriminator not bound");
  if (!y_static || !y_hat_static || !mask) return fail(GT_ERR_INVALID, "null tensor");
  CHK(check_gan_objective(e));
  CHK(gp_refusals(e));
  hipStream_t s = (hipStream_t)stream;
  const long N = (long)B * T;
  const bool tr = train != 0;
  ResultsChannel& rc = e->results;
  // fused call: losses and counts are final after the head (the gradient norm is not: reported as 0), so the head's
  // reduction kernel also writes the result struct and the scalars start their way to the host right behind it
  const bool plain_early = rc.early && !comm_on(e), comm_early = rc.early && comm_on(e);
  DPass p;
  CHK(d_pass_plan(e, x, y_static, y_hat_static, e->Ds, 2, B, T, tr, &p));
  if (comm_on(e) && tr && D.grads_dirty)
    return fail(GT_ERR_STATE, "data-parallel step: optimizer_d.zero_grad() must precede update_discriminator (the gradient buckets are summed over the ranks in place)");
  if (e->sn.on && tr && D.grads_dirty)
    return fail(GT_ERR_STATE, "spectral norm: optimizer_d.zero_grad() must precede update_discriminator (the last step's gradient was projected in place)");
  e->ws[GT_ROLE_D].sdefer.reset(rc.early && tr && D.has_opt);
  const TvPlan tv(e, p, mask, tr && D.has_opt && D.d.grads);
  e->norm.d_step_begins(tv.route == TvPlan::IN_SUMS);
  CHK(tv.before_input(e, s));
  CHK(d_pass_input(e, p, &tv, s));
  CHK(d_pass_forward(e, p, s));
  if (tr && !D.d.grads) return fail(GT_ERR_STATE, "phase == \"train\" but the discriminator was bound without grads");
  HeadCall hc;
  memset(&hc, 0, sizeof(hc));
  hc.mode = HEAD_D_STEP; hc.rows = p.rows; hc.n_real = N; hc.mask = mask; hc.n_mask = N; hc.eps = eps; hc.want_grad = tr; hc.want_w = tr;
  if (plain_early) { hc.early_res = rc.target(); hc.ticket = rc.take_ticket(); }
  CHK(tv.before_head(e, hc, s));
  CHK(d_pass_head(e, p, hc, nullptr, s));
  rc.clear_early();
  if (plain_early) CHK(rc.post_early(s, hc.ticket));
  if (comm_early) CHK(comm_early_results(e, GT_ROLE_D, tv.early_sums(e->sc()), tv.n_early_sums(), 0.f, 0.f, 0.f, s));
  if (tr) {
    CHK(comm_grads_ready(e, GT_ROLE_D, D.last.dW, (long)D.last.in * D.last.out + D.last.out, s));
    float* leak;
    CHK(e->leak.claim(e, y_hat_static, N, &leak));
    CHK(d_pass_backward(e, p, leak, s));
    CHK(d_pass_penalty(e, p, mask, s));      // gt_set_grad_penalty: added before anything closes the step's gradients (sdefer, clip-norm)
    D.grads_dirty = true;
    if (leak) e->leak.kept(tv.route == TvPlan::IN_SUMS);
  }
  // data parallel: the rest of D's gradient + the four loss / count sums, then the step stream waits for the communicator
  CHK(comm_finish_step(e, GT_ROLE_D, tr, &e->sc()->s_real, comm_early ? 0 : 4, s));
  rc.begin_done[GT_ROLE_D] = true;
  return GT_OK;
}

static void fill_d_result(const StepResults* h, gt_d_result* out) {
  out->loss_d = h->loss_d; out->loss_fake_d = h->loss_fake_d; out->loss_real_d = h->loss_real_d;
  out->real_correct_count = h->real_correct; out->fake_correct_count = h->fake_correct;
  out->grad_norm = h->gnorm_d;
}
static void fill_g_result(const StepResults* h, gt_g_result* out) {
  out->loss_mse = h->loss_mse; out->loss_mge = h->loss_mge; out->loss_adv = h->loss_adv;
  out->loss_g = h->loss_g; out->grad_norm = h->gnorm_g;
}

// The second half of either step: the optimizer step, enqueued BEFORE the host waits for anything; then early results posted by _begin are waited for, else
// `finalize` launches the role's finalisation and the results are posted as deferred (out == null: nothing synchronises) or fetched into rc.h_res.
template <typename Finalize>
static int step_end(gt_engine* e, int role, bool train, bool out_is_null, hipStream_t s, Finalize finalize) {
  if (!e) return fail(GT_ERR_INVALID, "null argument");
  ResultsChannel& rc = e->results;
  if (!rc.begin_done[role]) return fail(GT_ERR_STATE, "gt_update_%s_end without _begin", role == GT_ROLE_D ? "discriminator" : "generator");
  rc.begin_done[role] = false;
  if (out_is_null && rc.early_posted()) return fail(GT_ERR_STATE, "deferred results are a split-phase feature");
  if (train) CHK(optimizer_step(e, role, role == GT_ROLE_D ? &e->sc()->gnorm2_d : &e->sc()->gnorm2_g, s));
  if (rc.early_posted()) return rc.wait_early();
  finalize();
  LAUNCH_CHECK();
  return out_is_null ? rc.post_deferred(role, s) : rc.fetch(s);
}
static int step_result(gt_engine* e, int role) { return e->results.collect(role); }      // ... then in e->results.h_def[role]

extern "C" int gt_update_discriminator_end(gt_engine* e, int train, gt_d_result* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CHK(step_end(e, GT_ROLE_D, train != 0, !out, s, [&] { launch_finalize_d(e->sc(), e->res(), train ? 0 : 1, 0, s); }));
  if (out) fill_d_result(e->results.h_res, out);
  return GT_OK;
}
extern "C" int gt_update_discriminator_result(gt_engine* e, gt_d_result* out) {
  if (!e || !out) return fail(GT_ERR_INVALID, "null argument");
  CHK(step_result(e, GT_ROLE_D));
  fill_d_result(e->results.h_def[GT_ROLE_D], out);
  return GT_OK;
}

extern "C" int gt_update_discriminator(gt_engine* e, const float* x, const float* y_static, const float* y_hat_static,
                                       const float* mask, int B, int T, int train, float eps, gt_d_result* out, void* stream) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  e->results.early = true;
  int r = gt_update_discriminator_begin(e, x, y_static, y_hat_static, mask, B, T, train, eps, stream);
  e->results.early = false;
  if (r != GT_OK) { e->results.abandon(); e->norm.d_step_begins(false); return r; }
  return gt_update_discriminator_end(e, train, out, stream);
}

// ------------------------------------------------------------------------------------------
// update_generator
// ------------------------------------------------------------------------------------------
// e->partial: [0, 1024) MGE partials, [1024, 2048) MSE partials, [2048, ...) the optimizer's squared-norm partials.
// deferred_blocks != null: the per-block partial sums stay in the MSE region and *deferred_blocks says how many -- the
// caller folds their reduction into a later launch (finalize_g_kernel) instead of paying a launch for it here.
static int sum_sqerr(gt_engine* e, const float* a, int lda, const float* b, int ldb, const float* mask, long rows, int D,
                     double* out, float* g, int ldg, float gscale, hipStream_t s, int* deferred_blocks = nullptr) {
  CHK(e->partial.ensure(4096 * sizeof(double)));
  double* part = e->partial.as<double>() + 1024;
  SqerrArgs q;
  memset(&q, 0, sizeof(q));
  q.a = a; q.lda = lda; q.b = b; q.ldb = ldb; q.mask = mask; q.rows = rows; q.D = D; q.partial = part; q.g = g; q.ldg = ldg; q.gscale = gscale; q.sc = e->sc();
  const int nblk = launch_masked_sqerr(q, s);
  LAUNCH_CHECK();
  if (deferred_blocks) { *deferred_blocks = nblk; return GT_OK; }
  launch_sum_partials(part, nblk, out, s);
  LAUNCH_CHECK();
  return GT_OK;
}

// backward of G from the gradient at y_hat_static (gs) [+ masked-MSE term at y_hat]
static int generator_backward(gt_engine* e, const float* x, const float* y, const float* y_hat, const float* mask,
                              float mse_w, hipStream_t s) {
  Net& G = e->net[GT_ROLE_G];
  NetWs& W = e->ws[GT_ROLE_G];
  const long N = e->pass.N();
  const int B = e->pass.B(), T = e->pass.T(), Do = G.d.out_dim;
  // dloss/dy_hat is an engine buffer: for the MLP stacks its row pitch is rounded up to 4 floats, so that the last layer's
  // two backward products (K = out_dim = 187 for the acoustic model) take the 16-byte loader and the 64x64 tiles; the
  // pad column is never read as data (K tail / row clamp of the GEMM loader)
  const bool mlp_body = !(has_lstm_body(G.d.arch) || G.d.arch == GT_ARCH_SRU);
  const int ldgy = mlp_body && e->pass.band() ? (Do + 3) & ~3 : Do;      // (In2Out always has one)
  CHK(e->gy.ensure((size_t)N * ldgy * sizeof(float)));
  float* gy = e->gy.as<float>();
  const float* gs = e->gs.as<float>();
  if (is_i2o(G.d.arch)) {
    const int sd = G.d.static_dim;
    if (G.d.arch == GT_ARCH_IN2OUT_RNN) mse_w = 0.f;   // y_hat is the input x there: the MSE term has no path into G
    CHK(e->dgx.ensure((size_t)N * sd * sizeof(float)));
    CHK(e->dtz.ensure((size_t)N * sd * sizeof(float)));
    launch_highway_backward(gs, sd, e->tx.as<float>(), sd, e->gx.as<float>(), sd, e->dgx.as<float>(), sd, e->dtz.as<float>(), sd, N, sd, s);
    LAUNCH_CHECK();
    CHK(linear_backward_weight(e->dtz.as<float>(), sd, x, G.d.in_dim, N, sd, sd, G.gate.dW, G.gate.db, G.grads_dirty, e->slabs, e->colp, product_prec(e, GT_ROLE_G), s,
                               &W.sdefer));
    CHK(comm_grads_ready(e, GT_ROLE_G, G.gate.dW, (long)sd * sd + sd, s));
    CHK(mlpg_backward(e, e->dgx.as<float>(), sd, e->d_scol_i2o.as<int>(), e->d_sstride_i2o.as<int>(), sd, gy, ldgy, B, T, mse_w, y_hat, y, Do, mask, *e->pass.band(), s));
  } else if (e->pass.band()) {
    CHK(mlpg_backward(e, gs, e->Ds, e->d_scol.as<int>(), e->d_sstride.as<int>(), e->Ds, gy, ldgy, B, T, mse_w, y_hat, y, Do, mask, *e->pass.band(), s));
  } else {
    // no parameter generation: y_hat_static == y_hat, the gradient passes straight through,
    // plus the masked-MSE gradient (which also yields loss_mse's sum)
    if (mse_w != 0.f) CHK(sum_sqerr(e, y_hat, Do, y, Do, mask, N, Do, &e->sc()->s_mse, gy, Do, mse_w, s));
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(cdiv(N * Do, 256)), dim3(256), 0, s, gs, 0L, 1, N * Do, gy, mse_w != 0.f ? 1 : 0);
    LAUNCH_CHECK();
  }
  if (G.d.last_sigmoid && !is_i2o(G.d.arch)) {      // y_hat = sigmoid(last layer) (models.py:141, 167, 190, 213): through s (1 - s)
    launch_sigmoid_grad(gy, ldgy, y_hat, Do, N, Do, s);
    LAUNCH_CHECK();
  }
  if (has_lstm_body(G.d.arch) || G.d.arch == GT_ARCH_SRU) {
    CHK(has_lstm_body(G.d.arch) ? lstm_backward(e, x, gy, B, T, s) : sru_backward(e, x, gy, B, T, s));
    G.grads_dirty = true;
    return GT_OK;
  }
  // last_linear: dW = gy^T H_top, db ; dZ_top = (gy W_last) (.) f'(H_top), into the buffer the hidden stack's backward starts from
  const int H = G.d.hidden_dim;
  if (use_b16(e, GT_ROLE_G)) {
    CHK(e->dz_b[0].ensure(N, H, true));
    CHK(out_layer_backward(e, GT_ROLE_G, gy, ldgy, N, mlp_top(e, GT_ROLE_G, true), OutGrad{B16Dst(e->dz_b[0], true), ACT_LEAKY_DROPOUT, W.specs.back(), false},
                           &W.sdefer, s));
    CHK(stack_backward_b16(e, GT_ROLE_G, e->xin_b.t(), e->xin_b.ldt, N, W.specs, 0, true, nullptr, 0, 0, 0, 0, 0, s));
    G.grads_dirty = true;
    return GT_OK;
  }
  CHK(e->dzA.ensure((size_t)2 * N * H * sizeof(float)));
  CHK(e->dzB.ensure((size_t)2 * N * H * sizeof(float)));
  CHK(out_layer_backward(e, GT_ROLE_G, gy, ldgy, N, mlp_top(e, GT_ROLE_G, false), OutGrad{B16Dst(e->dzA.as<float>(), H), ACT_LEAKY_DROPOUT, W.specs.back(), true},
                         &W.sdefer, s));
  // The first layer's weight gradient reads G's input as its n-contiguous frame operand: with a 16-byte pitch it takes the
  // 16-byte loader and the 64 x 64 tiles.  The caller's tensor when it has one, else the discriminator's input image of this step
  // when that holds the very same x (bit-exact copy), else a pitched copy made once per step (shared with the split first layer
  // of D when it conditions on the same tensor).
  const float* xin = x;
  int ldxin = gx_pitch(e);
  if (!gemm_vec_ok(x, ldxin) && product_prec(e, GT_ROLE_G) == PREC_F32) {
    if (e->din.img_cat.valid && e->din.img_cat.x == x && e->cfg.discriminator_linguistic_condition && cond_dim(e) == G.d.in_dim && e->dcat.p) {
      ldxin = (d_in_dim(e) + 3) & ~3;
      xin = e->dcat.as<float>() + N * ldxin;      // the generated half: the one that is valid whenever img_cat is
    } else {
      StepCopy& M = e->din.dx_pitched.holds(x, gx_pitch(e), G.d.in_dim, N, e->step_counter) ? e->din.dx_pitched : e->din.gx_pitched;
      CHK(pitched_rows(e, M, x, gx_pitch(e), G.d.in_dim, N, &xin, &ldxin, s));
    }
  }
  CHK(stack_backward(e, GT_ROLE_G, xin, ldxin, N, W.specs, e->dzA.as<float>(), e->dzB.as<float>(), true,
                     nullptr, 0, 0, 0, 0, 0, s));
  G.grads_dirty = true;
  return GT_OK;
}

// Which launches of the generator step carry which sums, and how its scalars are reported (the discriminator side: DPass, and TvPlan for the
// loss normaliser).  With X = mse_in_backward:
//   call                               | sums                                                        | report
//   split-phase, or X                  | own launches (with X the MSE sum comes from the backward)   | at _end
//   fused, single GPU, riders off      | folded                                                      | early, this stream
//   fused, single GPU, riders on       | riders (the rider writes results and ticket)                | early, this stream
//   fused, communicator, riders off    | own launches                                                | early via the communicator iff opt_comm_early_g, else at _end
//   fused, communicator, riders on     | riders (the rider files the sums only: no results, no ticket) | as the row above
struct GPlan {
  bool mse_in_backward;      // phase "train", no parameter generation in the stashed pass (In2Out always has it), mse_w != 0: generator_backward's MSE launch yields the sum
  // where the reported sums of squares and the head's partials are reduced: launches of their own; the finalisation launch; riders -- both sums of squares in ONE launch,
  enum { SUMS_OWN, SUMS_FOLDED, SUMS_RIDERS } sums;      // the head's scalars and the finalisation as one extra workgroup of the gradient assembly: four launches become two
  enum { REPORT_AT_END, REPORT_EARLY, REPORT_EARLY_COMM } report;      // by _end; early from this stream; early from the communicator's stream
  GPlan(gt_engine* e, bool train, float mse_w) : mse_in_backward(train && !e->pass.band() && mse_w != 0.f) {
    const bool fused = e->results.early && !mse_in_backward, comm = comm_on(e);
    sums = !fused ? SUMS_OWN : e->opt_launch_riders ? SUMS_RIDERS : comm ? SUMS_OWN : SUMS_FOLDED;
    report = !fused ? REPORT_AT_END : !comm ? REPORT_EARLY : e->opt_comm_early_g ? REPORT_EARLY_COMM : REPORT_AT_END;
  }
};

extern "C" int gt_update_generator_begin(gt_engine* e, const float* x, const float* y, const float* y_hat, const float* y_static,
                                         const float* y_hat_static, float adv_w, const float* mask, int B, int T, int train,
                                         float mse_w, float mge_w, float eps, void* stream) {
  CHK(check_common(e, B, T));
  Net& G = e->net[GT_ROLE_G];
  Net& D = e->net[GT_ROLE_D];
  if (!G.bound) return fail(GT_ERR_STATE, "generator not bound");
  if (!y || !y_hat || !y_static || !y_hat_static || !mask) return fail(GT_ERR_INVALID, "null tensor");
  if (adv_w > 0.f) CHK(check_gan_objective(e));
  if (train) CHK(check_param_ema(e));
  hipStream_t s = (hipStream_t)stream;
  const long N = (long)B * T;
  const bool tr = train != 0;
  if (tr) {
    if (!e->pass.is(y_hat, y_hat_static, N))
      return fail(GT_ERR_STATE, "update_generator(phase=\"train\") needs the y_hat / y_hat_static returned by the last apply_generator");
    if (!G.d.grads) return fail(GT_ERR_STATE, "phase == \"train\" but the generator was bound without grads");
  }
  const int Do = G.d.out_dim;
  const int Ds = is_i2o(G.d.arch) ? G.d.static_dim : e->Ds;
  if (comm_on(e) && tr && G.grads_dirty)
    return fail(GT_ERR_STATE, "data-parallel step: optimizer_g.zero_grad() must precede update_generator");
  ResultsChannel& rc = e->results;
  e->ws[GT_ROLE_G].sdefer.reset(rc.early && tr && G.has_opt);
  CHK(e->norm.ensure(e, mask, N, s));
  const GPlan plan(e, tr, mse_w);
  const bool riders = plan.sums == GPlan::SUMS_RIDERS;
  CHK(e->partial.ensure(4096 * sizeof(double)));
  // loss_mse (always reported, train.py:294); its gradient is fused into the MLPG^T kernel
  int mse_blocks = 0, mge_pre_blocks = 0;
  if (riders) {
    GLossesArgs q;
    memset(&q, 0, sizeof(q));
    q.a1 = y_hat; q.lda1 = Do; q.b1 = y; q.ldb1 = Do; q.D1 = Do; q.partial1 = e->partial.as<double>() + 1024;
    q.a2 = y_hat_static; q.lda2 = Ds; q.b2 = y_static; q.ldb2 = Ds; q.D2 = Ds; q.partial2 = e->partial.as<double>(); q.mask = mask; q.rows = N;
    launch_g_losses(q, &mse_blocks, &mge_pre_blocks, s);
    LAUNCH_CHECK();
  } else if (!plan.mse_in_backward) {
    CHK(sum_sqerr(e, y_hat, Do, y, Do, mask, N, Do, &e->sc()->s_mse, nullptr, 0, 0.f, s, plan.sums == GPlan::SUMS_FOLDED ? &mse_blocks : nullptr));
  }
  // adversarial term with the CURRENT (already updated) D weights and a fresh dropout mask (train.py:297-308)
  e->g_has_adv = adv_w > 0.f;
  float* gadv = nullptr;
  int head_blocks = 0;
  if (adv_w > 0.f) {
    if (!D.bound) return fail(GT_ERR_STATE, "adv_w > 0 but no discriminator bound");
    DPass p;
    CHK(d_pass_plan(e, x, nullptr, y_hat_static, Ds, 1, B, T, false, &p));
    CHK(d_pass_input(e, p, nullptr, s));      // the generated half: kept from the D step of the same batch, or built here
    CHK(d_pass_forward(e, p, s));
    if (tr) { CHK(e->gadv.ensure((size_t)N * e->Da * sizeof(float))); gadv = e->gadv.as<float>(); }
    HeadCall hc;
    memset(&hc, 0, sizeof(hc));
    hc.mode = HEAD_G_ADV; hc.rows = p.rows; hc.n_real = N; hc.mask = mask; hc.n_mask = N; hc.eps = eps; hc.want_grad = tr; hc.want_w = false;
    hc.defer_scalars = riders ? &head_blocks : nullptr;
    CHK(d_pass_head(e, p, hc, gadv, s));
    if (tr) CHK(d_pass_backward(e, p, gadv, s));      // no weight gradients (train.py:307-308)
  }
  // MGE loss + gradient assembly at y_hat_static
  rc.clear_early();
  int mge_blocks = frame_red_blocks(N * Ds);
  float* gs = nullptr;
  if (tr) { CHK(e->gs.ensure((size_t)N * Ds * sizeof(float))); gs = e->gs.as<float>(); }
  const float* leak = tr ? e->leak.get() : nullptr;
  GFinalize fin;
  memset(&fin, 0, sizeof(fin));
  const bool reports = riders && plan.report == GPlan::REPORT_EARLY;      // the rider writes results and ticket; else it only files the sums
  if (riders) {
    fin.on = 1; fin.sc = e->sc(); fin.out = reports ? rc.target() : (StepResults*)nullptr; fin.adv_w = adv_w; fin.mse_w = mse_w; fin.mge_w = mge_w;
    fin.has_adv = e->g_has_adv ? 1 : 0; fin.part_mge = e->partial.as<double>(); fin.n_mge = mge_pre_blocks;
    fin.part_mse = e->partial.as<double>() + 1024; fin.n_mse = mse_blocks;
    fin.hp = head_blocks ? e->headp.as<HeadPartials>() : (const HeadPartials*)nullptr; fin.n_hp = head_blocks;
    if (reports) { fin.ticket_value = rc.take_ticket(); fin.ticket = fin.ticket_value ? rc.ticket_dev() : (unsigned*)nullptr; }
  }
  if (tr || !riders) {
    StaticGradArgs q;
    memset(&q, 0, sizeof(q));
    q.yhs = y_hat_static; q.ld1 = Ds; q.ys = y_static; q.ld2 = Ds; q.mask = mask; q.rows = N; q.Ds = Ds; q.mge_w = mge_w;
    q.adv_inv = e->d_adv_inv.as<int>(); q.leak = leak; q.ldl = e->Da; q.gadv = gadv; q.lda = e->Da; q.adv_w = adv_w; q.gs = gs; q.ldg = Ds;
    q.partial = riders ? (double*)nullptr : e->partial.as<double>(); q.sc = e->sc(); q.fin = fin; q.leak_unnorm = leak && e->leak.unnormalised() ? 1 : 0;
    mge_blocks = launch_static_grad(q, s);
  } else      // phase != "train": no gradient to assemble, the finalisation alone
    launch_finalize_g_rider(fin, s);
  LAUNCH_CHECK();
  if (reports) CHK(rc.post_early(s, fin.ticket_value));
  else if (plan.sums == GPlan::SUMS_OWN) {   // the split-phase (data-parallel) caller all-reduces the sum itself: it must exist now
    launch_sum_partials(e->partial.as<double>(), mge_blocks, &e->sc()->s_mge, s);
    LAUNCH_CHECK();
  }
  if (plan.sums == GPlan::SUMS_FOLDED) {   // all four losses are final here; the MSE and MGE partials are reduced inside the finalisation launch
    launch_finalize_g(e->sc(), rc.target(), adv_w, mse_w, mge_w, e->g_has_adv ? 1 : 0, 1, e->partial.as<double>(), mge_blocks,
                      mse_blocks ? (const double*)(e->partial.as<double>() + 1024) : (const double*)nullptr, mse_blocks, s);
    LAUNCH_CHECK();
    CHK(rc.post_early(s));
  }
  const bool comm_early = plan.report == GPlan::REPORT_EARLY_COMM;
  if (comm_early) CHK(comm_early_results(e, GT_ROLE_G, &e->sc()->s_adv, 3, adv_w, mse_w, mge_w, s));
  if (tr) {
    CHK(generator_backward(e, e->pass.input(), y, y_hat, mask, mse_w, s));  // G's own input (cat(x, z), train.py:542)
    e->leak.drop();
  }
  CHK(comm_finish_step(e, GT_ROLE_G, tr, &e->sc()->s_adv, comm_early ? 0 : 3, s));
  rc.begin_done[GT_ROLE_G] = true;
  return GT_OK;
}

extern "C" int gt_update_generator_end(gt_engine* e, int train, float adv_w, float mse_w, float mge_w, gt_g_result* out,
                                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  CHK(step_end(e, GT_ROLE_G, train != 0, !out, s, [&] {
    launch_finalize_g(e->sc(), e->res(), adv_w, mse_w, mge_w, e->g_has_adv ? 1 : 0, train ? 0 : 1, nullptr, 0, nullptr, 0, s);
  }));
  if (!out) return GT_OK;
  fill_g_result(e->results.h_res, out);
  return fault_seen(e);
}
extern "C" int gt_update_generator_result(gt_engine* e, gt_g_result* out) {
  if (!e || !out) return fail(GT_ERR_INVALID, "null argument");
  CHK(step_result(e, GT_ROLE_G));
  fill_g_result(e->results.h_def[GT_ROLE_G], out);
  return GT_OK;
}

extern "C" int gt_update_generator(gt_engine* e, const float* x, const float* y, const float* y_hat, const float* y_static,
                                   const float* y_hat_static, float adv_w, const float* mask, int B, int T, int train,
                                   float mse_w, float mge_w, float eps, gt_g_result* out, void* stream) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  e->results.early = true;
  int r = gt_update_generator_begin(e, x, y, y_hat, y_static, y_hat_static, adv_w, mask, B, T, train, mse_w, mge_w, eps, stream);
  e->results.early = false;
  if (r != GT_OK) { e->results.abandon(); return r; }
  return gt_update_generator_end(e, train, adv_w, mse_w, mge_w, out, stream);
}

extern "C" int gt_flush_generator_grads(gt_engine* e, void* stream) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  Net& G = e->net[GT_ROLE_G];
  if (!G.bound || !G.d.grads || !e->pass.live()) return fail(GT_ERR_STATE, "no generator pass to back-propagate");
  hipStream_t s = (hipStream_t)stream;
  CHK(fault_seen(e));
  e->ws[GT_ROLE_G].sdefer.reset(false);      // combines run in place here
  const long N = e->pass.N();
  const int Ds = is_i2o(G.d.arch) ? G.d.static_dim : e->Ds;
  CHK(e->gs.ensure((size_t)N * Ds * sizeof(float)));
  HIPCHK(hipMemsetAsync(e->gs.p, 0, (size_t)N * Ds * sizeof(float), s));
  if (const float* leak = e->leak.get()) {
    // scatter leak[:, j] -> gs[:, adv_cols[j]]  (gather with swapped roles: one column at a time is fine here)
    std::vector<int>& cols = e->h_adv_cols;
    for (int j = 0; j < e->Da; ++j) {
      launch_copy_cols(leak, e->Da, j, e->gs.as<float>(), Ds, cols[j], N, 1, s);
    }
    if (e->leak.unnormalised()) launch_scale_by_inv_tv(e->gs.as<float>(), N * Ds, e->sc(), s);
    LAUNCH_CHECK();
  }
  CHK(generator_backward(e, e->pass.input(), e->pass.y_hat(), e->pass.y_hat(), (const float*)nullptr, 0.f, s));
  e->leak.drop();
  HIPCHK(hipStreamSynchronize(s));
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// plain forward
// ------------------------------------------------------------------------------------------
extern "C" int gt_model_forward(gt_engine* e, int role, const float* x, const float* R, int B, int T, float* out, float* out2,
                                void* stream) {
  CHK(check_common(e, B, T));
  if (role < 0 || role > 1 || !e->net[role].bound) return fail(GT_ERR_STATE, "model not bound");
  if (!x || !out) return fail(GT_ERR_INVALID, "null tensor");
  hipStream_t s = (hipStream_t)stream;
  Net& n = e->net[role];
  const long N = (long)B * T;
  e->step_counter++;
  std::vector<DropoutSpec> specs;
  if (role == GT_ROLE_G && is_i2o(n.d.arch)) {
    if (!out2) return fail(GT_ERR_INVALID, "In2OutHighwayNet forward returns two tensors");
    on_generator_plain_forward(e);
    return generator_forward(e, x, R, B, T, out, out2, false, s, specs);
  }
  if (n.d.arch == GT_ARCH_LSTM || n.d.arch == GT_ARCH_SRU) {
    if (role != GT_ROLE_G) {
      // the recurrent discriminator's plain forward: its stack over the caller's rows as they are (no image, no layer-0 CatSrc:
      // GT_OPT_SRU_D_BF16 then casts them itself), then hidden2out (+ sigmoid)
      DPass p;
      memset(&p, 0, sizeof(p));
      p.kind = n.d.arch == GT_ARCH_SRU ? D_SRU : D_LSTM;
      p.npass = 1; p.passes[0] = 0; p.B = p.nseq = B; p.T = T; p.img = x; p.ldc = n.d.in_dim;
      CHK(d_pass_forward(e, p, s));
      return out_layer_forward(e, role, OutTop{p.top, p.ld_top}, N, out, s);
    }
    on_generator_plain_forward(e);
    return n.d.arch == GT_ARCH_LSTM ? lstm_forward(e, x, B, T, out, s) : sru_forward(e, x, B, T, out, s);
  }
  const int pass0[1] = {0};
  if (role == GT_ROLE_G) on_generator_plain_forward(e);
  const bool b16 = use_b16(e, role);
  if (role == GT_ROLE_D) CHK(sn_prepare_pass(e, s));
  if (b16) {
    CHK(e->fwd_b.ensure(N, n.d.in_dim, false));
    CHK(cast_transpose(x, n.d.in_dim, N, n.d.in_dim, e->fwd_b.r(), e->fwd_b.ld, (__bf16*)nullptr, 0, nullptr, false, &e->colp, s));
    CHK(refresh_shadows(e, role, true, s));
    CHK(stack_forward_b16(e, role, e->fwd_b.r(), e->fwd_b.ld, N, pass0, 1, N, specs, false, s));
  } else {
    CHK(stack_forward(e, role, x, n.d.in_dim, N, pass0, 1, N, specs, s));      // (plain forward: dense rows)
  }
  return out_layer_forward(e, role, mlp_top(e, role, b16), N, out, s);
}

