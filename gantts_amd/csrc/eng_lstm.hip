// libgantts_hip.so -- recurrent generator (GT_ARCH_LSTM / GT_ARCH_IN2OUT_RNN): persistent and per-step LSTM kernels
#include "engine_internal.hip.h"
#include "lstm_kernels.hip.h"
#include "lstm_seq_kernels.hip.h"
using namespace gt;
// ------------------------------------------------------------------------------------------
// recurrent generator (GT_ARCH_LSTM): forward / backward of the LSTM stack
// ------------------------------------------------------------------------------------------
// (the stashes are the role's own, e->ws[role]: NetWs in engine_internal.hip.h)
int lstm_check_lengths(gt_engine* e, int B, int T) {
  if ((int)e->h_lengths.size() != B)
    return fail(GT_ERR_STATE, "recurrent network: call with lengths (gt_set_lengths) for this batch of %d sequences "
                "(reference models.py:204-210 packs the batch by `lengths`)", B);
  for (int b = 0; b < B; ++b)
    if (e->h_lengths[b] > T) return fail(GT_ERR_INVALID, "length %d exceeds the padded length %d", e->h_lengths[b], T);
  return GT_OK;
}

enum { GT_LSTM_PATH_STEPS = 32, GT_LSTM_PATH_DECLINED = 33 };    // gt_lstm_path_counts: per-step kernels / no persistent grid fitted

static int lstm_launch_steps(gt_engine* e, const Net& G, NetWs& W, int layer, int B, int T, bool backward, const float* dout, hipStream_t s) {
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1;
  const int Bpad = cdiv(B, 32) * 32;
  e->lstm_paths[GT_LSTM_PATH_STEPS]++;
  const size_t st = (size_t)dirs * Bpad * H;              // floats per state array
  CHK(e->l_state.ensure(5 * st * sizeof(float)));          // h0,h1,c0,c1 (ping-pong) + dc
  float* base = e->l_state.as<float>();
  HIPCHK(hipMemsetAsync(base, 0, 5 * st * sizeof(float), s));
  CHK(ensure_dyn_lds((const void*)lstm_fwd_step_kernel, lstm_lds_bytes()));
  CHK(ensure_dyn_lds((const void*)lstm_bwd_step_kernel, lstm_lds_bytes()));
  LstmStepArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = T; a.H = H; a.dirs = dirs; a.Bpad = Bpad;
  a.lengths = e->d_lengths();
  for (int d = 0; d < dirs; ++d) { a.Whh[d] = G.lstm[layer].d[d].Whh; a.bih[d] = G.lstm[layer].d[d].bih; a.bhh[d] = G.lstm[layer].d[d].bhh; }
  a.xproj = W.xproj[layer].as<float>();
  a.gates = W.gates[layer].as<float>();
  a.cst = W.cst[layer].as<float>();
  a.out = W.out[layer].as<float>();
  a.dout = dout;
  a.dc_state = base + 4 * st;
  for (int step = 0; step < T; ++step) {
    a.step = step;
    if (!backward) {
      const int cur = step & 1;
      a.h_prev = base + (size_t)cur * st;       a.c_prev = base + (2 + (size_t)cur) * st;
      a.h_next = base + (size_t)(cur ^ 1) * st; a.c_next = base + (2 + (size_t)(cur ^ 1)) * st;
      hipLaunchKernelGGL(lstm_fwd_step_kernel, dim3(cdiv(H, 8), dirs, cdiv(B, 32)), dim3(256), lstm_lds_bytes(), s, a);
    } else {
      hipLaunchKernelGGL(lstm_bwd_step_kernel, dim3(cdiv(H, 32), dirs, cdiv(B, 32)), dim3(256), lstm_lds_bytes(), s, a);
    }
  }
  LAUNCH_CHECK();
  return GT_OK;
}

// ---- persistent recurrence (lstm_seq_kernels.hip.h): one launch per layer and pass ----
// Co-resident workgroups per XCD: all workgroups of a launch spin on each other, so the whole grid must be resident
// at once.  The occupancy API may over-report by one block per CU (MI355X_MICROARCH.md, residency): keep that margin
// above one per CU.  The grid is laid out per XCD (seq_group_of), so the bound is per XCD as well.
static int seq_xcds(int* nxcd, int* cus_per_xcd) {
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  static std::map<int, int> cus;
  if (!cus.count(dev)) { hipDeviceProp_t prop; HIPCHK(hipGetDeviceProperties(&prop, dev)); cus[dev] = prop.multiProcessorCount; }
  *nxcd = cus[dev] % 8 == 0 && cus[dev] >= 64 ? 8 : 1;      // MI355X: 8 XCDs x 32 CUs
  *cus_per_xcd = cus[dev] / *nxcd;
  return GT_OK;
}
template <typename K>
static int launch_seq(K kern, size_t lds, LstmSeqArgs& a, hipStream_t s, bool* launched, int block = 256) {
  CHK(ensure_dyn_lds((const void*)kern, lds));
  int per_cu = 0, nxcd = 1, cpx = 1;
  CHK(seq_xcds(&nxcd, &cpx));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, block, lds));
  if (per_cu > 1) per_cu -= 1;
  per_cu = std::min(per_cu, 4);
  const int ngroups = a.dirs * a.nbt;
  const int rounds = cdiv(ngroups, nxcd);                   // groups that share one XCD
  if ((long)a.ncu * rounds > (long)cpx * per_cu) { *launched = false; return GT_OK; }
  a.nxcd = nxcd;
  hipLaunchKernelGGL(kern, dim3(nxcd * a.ncu * rounds), dim3(block), lds, s, a);
  LAUNCH_CHECK();
  *launched = true;
  return GT_OK;
}
// forward: loader waves + the fast gate functions (lstm_seq_kernels.hip.h: 2.15 -> 1.59 us per step in bf16, 2.54 -> 1.92
// in f32 on a cfg3 layer; tools/lstm_sched_bench keeps the round-2 variant as the A/B reference)
template <int HP, int UPC>
static int launch_fwd_seq(LstmSeqArgs& a, int bt, bool bf16, hipStream_t s, bool* launched) {
  if (bf16)
    return bt == 8 ? launch_seq(lstm_fwd_seq_kernel<HP, UPC, 8, PREC_BF16, false, true, true>, lstm_fwd_seq_lds<HP, UPC>(), a, s, launched, lstm_fwd_block(UPC, 8, true))
                   : launch_seq(lstm_fwd_seq_kernel<HP, UPC, 16, PREC_BF16, false, true, true>, lstm_fwd_seq_lds<HP, UPC>(), a, s, launched, lstm_fwd_block(UPC, 16, true));
  return bt == 8 ? launch_seq(lstm_fwd_seq_kernel<HP, UPC, 8, PREC_F32, false, true, true>, lstm_fwd_seq_lds<HP, UPC>(), a, s, launched, lstm_fwd_block(UPC, 8, true))
                 : launch_seq(lstm_fwd_seq_kernel<HP, UPC, 16, PREC_F32, false, true, true>, lstm_fwd_seq_lds<HP, UPC>(), a, s, launched, lstm_fwd_block(UPC, 16, true));
}
// backward: loader waves in both precisions; the tagged exchange where dG travels as bf16 (in f32 it doubles the exchange
// volume and loses).  cfg3 layer, us per step: bf16 2.38 -> 1.85, f32 3.13 -> 2.76 (tools/lstm_sched_bench).
template <int HP>
static int launch_bwd_seq(LstmSeqArgs& a, int bt, bool bf16, hipStream_t s, bool* launched) {
  if (bf16)
    return bt == 8 ? launch_seq(lstm_bwd_seq_kernel<HP, 8, PREC_BF16, true, true>, lstm_bwd_seq_lds<HP>(), a, s, launched, lstm_bwd_block(8, true))
                   : launch_seq(lstm_bwd_seq_kernel<HP, 16, PREC_BF16, true, true>, lstm_bwd_seq_lds<HP>(), a, s, launched, lstm_bwd_block(16, true));
  return bt == 8 ? launch_seq(lstm_bwd_seq_kernel<HP, 8, PREC_F32, true, false>, lstm_bwd_seq_lds<HP>(), a, s, launched, lstm_bwd_block(8, true))
                 : launch_seq(lstm_bwd_seq_kernel<HP, 16, PREC_F32, true, false>, lstm_bwd_seq_lds<HP>(), a, s, launched, lstm_bwd_block(16, true));
}

// Runs one layer's recurrence (forward, or backward when `backward`) as ONE persistent launch when the shape fits
// (H <= 512, grid co-resident); *launched = false leaves the work to the per-step kernels.
static int lstm_launch_seq(gt_engine* e, const Net& G, NetWs& W, bool bf16, int layer, int B, int T, bool backward, const float* dout,
                           hipStream_t s, bool* launched) {
  *launched = false;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1;
  if (!e->lstm_persistent || H > 512 || T < 2) return GT_OK;
  const int HP = H <= 256 ? 256 : 512;
  int nxcd = 1, cpx = 1;
  CHK(seq_xcds(&nxcd, &cpx));
  // batch tile: 16 sequences per group (full MFMA rows) once that already gives every XCD a group; else 8, which
  // halves the exchange volume of a group and spreads the recurrences over more XCDs (their L2s bound the exchange).
  // gt_set_tuning("lstm_bt") forces one.
  const int bt = gt_tuning().lstm_bt ? gt_tuning().lstm_bt : dirs * cdiv(B, 16) >= nxcd ? 16 : 8;
  // gt_lstm_path_counts: slot of the instantiation that runs (the forward's UPC bit is added below)
  const int slot = 16 * (backward ? 1 : 0) + 8 * (HP == 512 ? 1 : 0) + 2 * (bt == 16 ? 1 : 0) + (bf16 ? 1 : 0);
  LstmSeqArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = T; a.H = H; a.dirs = dirs; a.nbt = cdiv(B, bt);
  a.lengths = e->d_lengths();
  for (int d = 0; d < dirs; ++d) { a.Whh[d] = G.lstm[layer].d[d].Whh; a.bih[d] = G.lstm[layer].d[d].bih; a.bhh[d] = G.lstm[layer].d[d].bhh; }
  a.xproj = W.xproj[layer].as<float>();
  a.gates = W.gates[layer].as<float>();
  a.cst = W.cst[layer].as<float>();
  a.out = W.out[layer].as<float>();
  a.dout = dout;
  a.fault = e->fault_dev();
  a.timeout_ticks = 200000000ULL;          // 2 s at 100 MHz: far beyond any real wait, far below the watchdog
  const int ngroups = dirs * a.nbt;
  const size_t xch_n = (size_t)ngroups * (backward ? lstm_bwd_xch_u64(HP) : lstm_fwd_xch_u64(HP)), chk_n = (size_t)ngroups * 256;
  CHK(e->l_xch.ensure((xch_n + chk_n) * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(e->l_xch.p, 0, (xch_n + chk_n) * sizeof(unsigned long long), s));   // no tag / flag of an earlier launch survives
  a.xch = e->l_xch.as<unsigned long long>();
  a.xcc_chk = a.xch + xch_n;              // [group][256]
  a.allow_xcd_local = e->lstm_xcd_local ? 1 : 0;
  if (backward) {
    a.ncu = cdiv(H, 16);
    CHK(HP == 256 ? launch_bwd_seq<256>(a, bt, bf16, s, launched) : launch_bwd_seq<512>(a, bt, bf16, s, launched));
    e->lstm_paths[*launched ? slot : GT_LSTM_PATH_DECLINED]++;
    if (*launched) HIPCHK(hipMemcpyAsync(e->h_fault, e->d_fault.p, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
    return GT_OK;
  }
  // forward: 8 hidden units per workgroup (32 workgroups per group at H = 256: one XCD's worth), else 16
  int upc = e->lstm_fwd_upc;
  if (upc != 8 && upc != 16) upc = 8;
  for (; upc <= 16 && !*launched; upc *= 2) {
    a.ncu = cdiv(H, upc);
    if (upc == 8) CHK(HP == 256 ? (launch_fwd_seq<256, 8>(a, bt, bf16, s, launched)) : (launch_fwd_seq<512, 8>(a, bt, bf16, s, launched)));
    else          CHK(HP == 256 ? (launch_fwd_seq<256, 16>(a, bt, bf16, s, launched)) : (launch_fwd_seq<512, 16>(a, bt, bf16, s, launched)));
    if (*launched) e->lstm_paths[slot + (upc == 16 ? 4 : 0)]++;
  }
  if (!*launched) e->lstm_paths[GT_LSTM_PATH_DECLINED]++;
  if (*launched) HIPCHK(hipMemcpyAsync(e->h_fault, e->d_fault.p, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  return GT_OK;
}

static bool lstm_b16(const gt_engine* e) { return e->matmul_bf16 && (e->net[GT_ROLE_G].d.hidden_dim & 7) == 0; }
// nn.LSTM(dropout=p) between the layers: layer `layer`'s dropout applied to src's N rows into dst (in place when they are equal), every pass's
// rows (a row group of N / npass) at its own site -- the forward's sites again in the backward
static int lstm_interlayer_dropout(gt_engine* e, int role, int layer, const int* passes, int npass, const float* src, float* dst, long N, int width,
                                   hipStream_t s) {
  const Net& G = e->net[role];
  const long Ng = N / npass;
  for (int q = 0; q < npass; ++q) {
    const DropoutSpec ds = drop_spec(e, role, passes[q], layer, G.inj[passes[q]][layer], width);
    launch_dropout_apply(src + q * Ng * width, dst + q * Ng * width, Ng, width, ds, s);
  }
  LAUNCH_CHECK();
  return GT_OK;
}
// The LSTM stack of network `role` over nseq sequences (rows = nseq * T of x, row pitch ld_x): X-projections, recurrences, inter-layer
// dropout; stashes X-projections / gates / cell states / layer outputs in the role's buffers.  passes / npass: the dropout sites of the
// row groups (the D step runs the natural and the generated sequences as ONE batch of 2B: two groups of nseq / 2 sequences).
// *top / *ld_top: the top layer's (dropped, if applicable) output.
int lstm_stack_forward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, hipStream_t s,
                       const float** top, int* ld_top) {
  Net& G = e->net[role];
  NetWs& W = e->ws[role];
  const int B = nseq;
  const long N = (long)B * T;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1;
  const float* in = x;
  int ld_in = ld_x;
  // GT_OPT_MATMUL_BF16: the layer inputs go through bf16 images (both orientations: the weight gradients read the
  // transposed one) and W_ih of all directions is one stacked bf16 shadow -- the X-projection of a layer is ONE product
  const bool b16 = role == GT_ROLE_G && lstm_b16(e);
  const bool want_t = G.d.grads != nullptr;
  const int Lc_ = G.d.num_hidden;
  if (b16) {
    CHK(resize_owned(W.l_in_b, Lc_ + 1)); CHK(resize_owned(W.lsh, Lc_ + 1));
    for (int l = 0; l < Lc_; ++l) {
      const LstmLayerP& L = G.lstm[l];
      CHK(W.lsh[l].ensure(dirs * 4 * H, L.in));
      for (int d = 0; d < dirs; ++d) CHK(shadow_cast(W.lsh[l], L.d[d].Wih, d * 4 * H, 4 * H, L.in, s));
    }
    CHK(W.lsh[Lc_].ensure(G.last.out, G.last.in));
    CHK(shadow_cast(W.lsh[Lc_], G.last.W, 0, G.last.out, G.last.in, s));
  }
  for (int l = 0; l < G.d.num_hidden; ++l) {
    const LstmLayerP& L = G.lstm[l];
    CHK(W.xproj[l].ensure((size_t)N * dirs * 4 * H * sizeof(float)));
    CHK(W.gates[l].ensure((size_t)N * dirs * 4 * H * sizeof(float)));
    CHK(W.cst[l].ensure((size_t)N * dirs * H * sizeof(float)));
    CHK(W.out[l].ensure((size_t)N * dirs * H * sizeof(float)));
    if (b16) {
      B16Img& I = W.l_in_b[l];
      CHK(I.ensure(N, L.in, want_t));
      CHK(cast_transpose(in, ld_in, N, L.in, I.r(), I.ld, want_t ? I.t() : (__bf16*)nullptr, I.ldt, nullptr, false, &e->colp, s));
      CHK(b16_forward(I.r(), I.ld, N, W.lsh[l].r(), W.lsh[l].ldw, dirs * 4 * H, L.in, nullptr, ACT_NONE, no_drop(),
                      B16Dst(W.xproj[l].as<float>(), dirs * 4 * H), s));
    } else {
      for (int d = 0; d < dirs; ++d)   // Xp[:, d*4H:(d+1)*4H] = X W_ih^T (biases are added in the step kernel)
        CHK(linear_forward(in, ld_in, L.d[d].Wih, L.in, nullptr, W.xproj[l].as<float>() + (size_t)d * 4 * H, dirs * 4 * H, N, L.in,
                           4 * H, ACT_NONE, no_drop(), product_prec(e, role), s));
    }
    bool seq = false;
    CHK(lstm_launch_seq(e, G, W, role == GT_ROLE_G && e->matmul_bf16, l, B, T, false, nullptr, s, &seq));
    if (!seq) CHK(lstm_launch_steps(e, G, W, l, B, T, false, nullptr, s));
    in = W.out[l].as<float>();
    ld_in = dirs * H;
    if (G.training && G.d.dropout > 0.f && l + 1 < G.d.num_hidden) {
      // nn.LSTM(dropout=p): dropout on the outputs of every layer but the last (training only)
      CHK(W.outd[l].ensure((size_t)N * dirs * H * sizeof(float)));
      CHK(lstm_interlayer_dropout(e, role, l, passes, npass, in, W.outd[l].as<float>(), N, dirs * H, s));
      in = W.outd[l].as<float>();
    }
  }
  *top = in; *ld_top = ld_in;
  return GT_OK;
}

// x (N, in_dim) -> y_hat (N, out_dim): the generator's stack + hidden2out
int lstm_forward(gt_engine* e, const float* x, int B, int T, float* y_hat, hipStream_t s) {
  Net& G = e->net[GT_ROLE_G];
  CHK(lstm_check_lengths(e, B, T));
  NetWs& W = e->ws[GT_ROLE_G];
  const int Lc = G.d.num_hidden;
  const int passes[1] = {0};
  OutTop top;
  CHK(lstm_stack_forward(e, GT_ROLE_G, x, G.d.in_dim, B, T, passes, 1, s, &top.x, &top.ld));
  if (lstm_b16(e)) { top.img = &W.l_in_b[Lc]; top.sh = &W.lsh[Lc]; top.want_t = G.d.grads != nullptr; }
  return out_layer_forward(e, GT_ROLE_G, top, (long)B * T, y_hat, s);
}

// gy (N, out_dim) = dL/dy_hat -> parameter gradients of hidden2out and of every LSTM layer
int lstm_backward(gt_engine* e, const float* x, const float* gy, int B, int T, hipStream_t s) {
  Net& G = e->net[GT_ROLE_G];
  NetWs& W = e->ws[GT_ROLE_G];
  const long N = (long)B * T;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1, Lc = G.d.num_hidden;
  CHK(W.dout.ensure((size_t)2 * N * dirs * H * sizeof(float)));      // first half: gradient w.r.t. the top layer's output
  OutTop top{W.out[Lc - 1].as<float>(), dirs * H};
  if (lstm_b16(e) && (int)W.l_in_b.size() == Lc + 1 && (int)W.lsh.size() == Lc + 1) { top.img = &W.l_in_b[Lc]; top.sh = &W.lsh[Lc]; }
  CHK(out_layer_backward(e, GT_ROLE_G, gy, G.d.out_dim, N, top, OutGrad{B16Dst(W.dout.as<float>(), dirs * H), ACT_NONE, no_drop(), false}, nullptr, s));
  const int passes[1] = {0};
  return lstm_stack_backward(e, GT_ROLE_G, x, G.d.in_dim, B, T, passes, 1, true, nullptr, s);
}

// From the gradient w.r.t. the top layer's output (first half of the role's `dout` buffer, row pitch dirs * H) down through the
// stack: weight gradients of every layer (want_w), and the gradient w.r.t. the stack's input when dx0 != null ([rows][in_dim], dense)
// -- what a recurrent discriminator hands back to the generator.
int lstm_stack_backward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, bool want_w,
                        float* dx0, hipStream_t s) {
  Net& G = e->net[role];
  NetWs& W = e->ws[role];
  const int B = nseq;
  const long N = (long)B * T;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1, Lc = G.d.num_hidden;
  const bool acc = G.grads_dirty;
  const int prec = product_prec(e, role);
  CHK(W.dout.ensure((size_t)2 * N * dirs * H * sizeof(float)));
  CHK(W.hshift.ensure((size_t)N * H * sizeof(float)));
  float* dout = W.dout.as<float>();                          // gradient w.r.t. the current layer's output
  float* dout_other = dout + (size_t)N * dirs * H;
  const bool b16 = role == GT_ROLE_G && lstm_b16(e) && (int)W.l_in_b.size() == Lc + 1 && (int)W.lsh.size() == Lc + 1;
  if (b16) CHK(resize_owned(W.l_dg_b, Lc));
  for (int l = Lc - 1; l >= 0; --l) {
    const LstmLayerP& L = G.lstm[l];
    bool seq = false;
    CHK(lstm_launch_seq(e, G, W, role == GT_ROLE_G && e->matmul_bf16, l, B, T, true, dout, s, &seq));  // dG overwrites xproj[l]
    if (!seq) CHK(lstm_launch_steps(e, G, W, l, B, T, true, dout, s));
    const float* dG = W.xproj[l].as<float>();
    const bool dropped_in = l > 0 && G.training && G.d.dropout > 0.f;
    if (b16) {
      // dG -> bf16 image in both orientations (one pass), then every product of this layer reads bf16:
      // dW_ih_d = dGT_d . inT^T (+ db from the loader), dW_hh_d = dGT_d . hshiftT^T, d in = dG . W_ihT^T (all directions in ONE product)
      B16Img& DG = W.l_dg_b[l];
      B16Img& I = W.l_in_b[l];
      CHK(DG.ensure(N, dirs * 4 * H, true));
      CHK(cast_transpose(dG, dirs * 4 * H, N, dirs * 4 * H, DG.r(), DG.ld, DG.t(), DG.ldt, nullptr, false, &e->colp, s));
      if (l > 0) {      // d(layer input) first, all directions in ONE product
        CHK(b16_backward_data(DG.r(), DG.ld, N, W.lsh[l].t(), W.lsh[l].ldwt, L.in, dirs * 4 * H, ACT_NONE, nullptr, no_drop(), B16Dst(dout_other, L.in), s));
        if (dropped_in) CHK(lstm_interlayer_dropout(e, role, l - 1, passes, npass, dout_other, dout_other, N, dirs * H, s));
        std::swap(dout, dout_other);
      }
      for (int d = 0; d < dirs; ++d) {
        const __bf16* dgt = DG.t() + (size_t)d * 4 * H * DG.ldt;
        CHK(weight_grad_b16(dgt, DG.ldt, I.t(), I.ldt, N, 4 * H, L.in, L.d[d].dWih, L.d[d].dbih, acc, e->slabs, s));
        hipLaunchKernelGGL(slab_reduce_small_kernel, dim3(cdiv(4 * H, 64)), dim3(1024), 0, s, L.d[d].dbih, (long)4 * H, 1, 4 * H,
                           L.d[d].dbhh, 0);
        LAUNCH_CHECK();
        hipLaunchKernelGGL(lstm_shift_kernel, dim3(cdiv(N * H, 256)), dim3(256), 0, s, W.out[l].as<float>(), dirs * H, d, H, B, T,
                           e->d_lengths(), W.hshift.as<float>());
        LAUNCH_CHECK();
        CHK(W.l_hs_b.ensure(N, H, true));
        CHK(cast_transpose(W.hshift.as<float>(), H, N, H, (__bf16*)nullptr, 0, W.l_hs_b.t(), W.l_hs_b.ldt, nullptr, false, &e->colp, s));
        CHK(weight_grad_b16(dgt, DG.ldt, W.l_hs_b.t(), W.l_hs_b.ldt, N, 4 * H, H, L.d[d].dWhh, nullptr, acc, e->slabs, s));
      }
      CHK(comm_grads_ready(e, role, L.d[0].dWih, (long)dirs * (4L * H * L.in + 4L * H * H + 8L * H), s));
      CHK(comm_flush(e, role, s));
      continue;
    }
    const float* Xl = l == 0 ? x : (dropped_in ? W.outd[l - 1].as<float>() : W.out[l - 1].as<float>());
    const int ldx = l == 0 ? ld_x : dirs * H;
    for (int d = 0; d < dirs && want_w; ++d) {
      const float* dGd = dG + (size_t)d * 4 * H;
      // dW_ih = dG_d^T X, db_ih = colsum(dG_d) (= db_hh)
      CHK(linear_backward_weight(dGd, dirs * 4 * H, Xl, ldx, N, 4 * H, L.in, L.d[d].dWih, L.d[d].dbih, acc, e->slabs, e->colp, prec, s));
      // bias_ih and bias_hh always receive the same gradient: keep them equal by copy
      hipLaunchKernelGGL(slab_reduce_small_kernel, dim3(cdiv(4 * H, 64)), dim3(1024), 0, s, L.d[d].dbih, (long)4 * H, 1, 4 * H,
                         L.d[d].dbhh, 0);
      LAUNCH_CHECK();
      // dW_hh = dG_d^T H_shift (h that entered each frame)
      hipLaunchKernelGGL(lstm_shift_kernel, dim3(cdiv(N * H, 256)), dim3(256), 0, s, W.out[l].as<float>(), dirs * H, d, H, B, T,
                         e->d_lengths(), W.hshift.as<float>());
      LAUNCH_CHECK();
      CHK(linear_backward_weight(dGd, dirs * 4 * H, W.hshift.as<float>(), H, N, 4 * H, H, L.d[d].dWhh, nullptr, acc, e->slabs,
                                 e->colp, prec, s));
    }
    // this layer's parameters (both directions: W_ih, W_hh, b_ih, b_hh each) are one contiguous bucket
    if (want_w) {
      CHK(comm_grads_ready(e, role, L.d[0].dWih, (long)dirs * (4L * H * L.in + 4L * H * H + 8L * H), s));
      if (role == GT_ROLE_G || !e->opt_comm_d_one_msg) CHK(comm_flush(e, role, s));              // with hidden2out above it: under the recurrence of the layer below
    }
    if (l > 0 || dx0) {   // gradient w.r.t. the layer below's output (or the stack's input): sum over directions of dG_d W_ih_d
      float* const dst = l > 0 ? dout_other : dx0;
      for (int d = 0; d < dirs; ++d)
        CHK(plain_product(GEMM_NN, dG + (size_t)d * 4 * H, dirs * 4 * H, L.d[d].Wih, L.in, dst, L.in, N, L.in, 4 * H, d > 0, prec, s));
      // through the inter-layer dropout of layer l-1 (same Philox sites as the forward)
      if (dropped_in) CHK(lstm_interlayer_dropout(e, role, l - 1, passes, npass, dout_other, dout_other, N, dirs * H, s));
      if (l > 0) std::swap(dout, dout_other);
    }
  }
  return GT_OK;
}

