// libgantts_hip.so -- the SRU stack (GT_ARCH_SRU) of either role: the recurrent generator, an SRURNN in the discriminator slot
#include <atomic>
#include "engine_internal.hip.h"
#include "sru_cs_kernels.hip.h"
#include "sru_kernels.hip.h"
using namespace gt;
// gt_sru_path_counts: process-wide, one relaxed increment per launch on the host (no device work, no synchronisation)
static std::atomic<int64_t> g_sru_paths[GT_SRU_PATH_SLOTS];
static void sru_path_count(int slot) { g_sru_paths[slot].fetch_add(1, std::memory_order_relaxed); }
extern "C" int gt_sru_path_counts(int64_t* counts, int reset) {
  for (int i = 0; i < GT_SRU_PATH_SLOTS; ++i) {
    const int64_t v = reset ? g_sru_paths[i].exchange(0, std::memory_order_relaxed) : g_sru_paths[i].load(std::memory_order_relaxed);
    if (counts) counts[i] = v;
  }
  return GT_OK;
}
// ------------------------------------------------------------------------------------------
// SRU stack (GT_ARCH_SRU), role-generic
// ------------------------------------------------------------------------------------------
static void sru_keys(gt_engine* e, int role, int pass, int layer, int which, uint32_t* k0, uint32_t* k1) {
  // data parallel: the masks are per (sequence, column); the kernels count sequences globally (SruArgs::seq_mul / seq_add), so a
  // world-k run draws the whole minibatch's masks of a world-1 run -- no rank in the key
  const uint64_t site = e->step_counter * 64ULL + 40 + (uint64_t)(layer * 2 + which);
  *k0 = (uint32_t)(e->seed ^ (site * 0x9E3779B97F4A7C15ULL));
  *k1 = (uint32_t)((e->seed >> 32) ^ (site >> 7) ^ 0x5A5A5A5Au) + (uint32_t)site;
  if (role != GT_ROLE_G || pass != 0) {      // a discriminator's three passes: never the generator's bits, never another pass's (G's keys are the ones above)
    const uint32_t salt = 0x85EBCA6Bu * (uint32_t)(1 + role * 3 + pass);
    *k0 ^= salt;
    *k1 += (salt >> 5) | 1u;
  }
}
uint32_t sru_drop_thresh(float p) {
  const double th = (double)p * 4294967296.0;
  return th >= 4294967295.0 ? 4294967295u : (uint32_t)th;
}

// (the stashes, images and shadows are the role's own, e->ws[role]: NetWs in engine_internal.hip.h)
// entries of s_in_b / ssh: one per layer; the generator has one more for hidden2out's product (a discriminator's top h goes to the fused
// head as float32, which holds hidden2out and its gradient)
static int sru_b16_entries(const gt_engine* e, int role) { return e->net[role].d.num_hidden + (role == GT_ROLE_G ? 1 : 0); }

// One variational dropout table [nseq][width] of layer `l` (which: 0 input, 1 output): every row group of the launch (the D step runs
// D(real) and D(fake) as ONE batch of 2B sequences) draws from its own pass -- its own Philox key, or its own injected 0/1 mask.
// Sequence ids stay global: group q starts at local sequence q * nseq / npass.
static int sru_draw_table(gt_engine* e, const Net& G, int role, int l, int which, float* tab, int nseq, int width, float p, float keep_scale,
                          const int* passes, int npass, hipStream_t s) {
  const int Bg = nseq / npass;
  for (int q = 0; q < npass; ++q) {
    uint32_t k0, k1;
    sru_keys(e, role, passes[q], l, which, &k0, &k1);
    CHK(sru_launch_input_mask(tab + (size_t)q * Bg * width, Bg, width, keep_scale, sru_drop_thresh(p), k0, k1,
                              (const float*)G.inj[passes[q]][2 * l + which], e->dp_world, e->dp_rank + e->dp_world * q * Bg, s));
  }
  return GT_OK;
}

static SruArgs sru_args(gt_engine* e, int role, NetWs& W, int l, int B, int T, const float* in, int ld_in) {
  const Net& G = e->net[role];
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1, ncols = H * dirs;
  const SruLayerP& L = G.sru[l];
  SruArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.T = T; a.H = H; a.dirs = dirs; a.k = L.k; a.act = G.d.use_relu ? SRU_RELU : SRU_TANH;
  a.U = W.u[l].as<float>(); a.ldu = ncols * L.k;
  a.x = in; a.ldx = ld_in;
  a.bias = L.b;
  a.h = W.h[l].as<float>(); a.c = W.c[l].as<float>();
  a.seq_mul = e->dp_world; a.seq_add = e->dp_rank;
  if (G.training && G.d.dropout > 0.f && l + 1 < G.d.num_hidden) {   // the last layer has dropout 0 (SRU.__init__)
    a.use_mask = 1; a.keep_scale = 1.f / (1.f - G.d.dropout); a.thresh = sru_drop_thresh(G.d.dropout);
    if (role == GT_ROLE_G) {
      sru_keys(e, GT_ROLE_G, 0, l, 1, &a.key0, &a.key1);
      a.mask_buf = G.inj[0][2 * l + 1];                              // gt_set_dropout_mask(G, 0, 2*l + 1): [B][ncols]
    } else {
      a.mask_buf = W.omask[l].as<float>();                           // drawn per pass by the forward (sru_draw_table): [nseq][ncols] of 0 / 1
    }
  }
  return a;
}

// GT_SRU_COOP=1 (default): the cooperative block scans (sru_cs_kernels.hip.h): every wave of a workgroup loads AND walks eight frames
// of a block, the waves' composites are combined through LDS.  Eight waves per 64 columns up to two workgroups per CU (cfg4's B = 16, the
// hparams-default generator's B = 32), four beyond.  0 selects the one-wave kernels (sru_kernels.hip.h), the sequential reference of the
// tests (read at every launch: a test flips it between two steps of one process).
static bool sru_coop() { return gt_tuning().sru_coop != 0; }
static int sru_coop_waves(long B, int ncols) {
  const int forced = gt_tuning().sru_cs_waves;      // (tests: both instantiations on every shape)
  if (forced == 4 || forced == 8) return forced;
  return cdiv(B * ncols, 64) <= 2 * gemm_cu_count() ? 8 : 4;      // (measured: cfg4 B = 16 7.39 vs 7.85 ms; hparams-default generator B = 32, T = 1024 8.07 vs 8.32 ms)
}
int sru_scan_waves(long B, int ncols) { return sru_coop() ? sru_coop_waves(B, ncols) : 0; }
// The one launch site of every scan kernel, for the stacks below and the parity hook (gt_op_sru_scan) alike: the form (sequential, four
// or eight waves) from the tuning knobs and the shape, the image forms from a.nx_b / a.dU_b being set (the caller has checked their
// conditions: sru_fold / du_b16).  Each launch is counted in its slot of gt_sru_path_counts.
int sru_launch_fwd(const SruArgs& a, hipStream_t s) {
  const int ncols = a.H * a.dirs;
  if (sru_coop()) {
    const int grid = cdiv((long)a.B * ncols, 64);
    const bool w8 = sru_coop_waves(a.B, ncols) == 8, img = a.nx_b != nullptr;
    if (img) {
      if (w8) { CHK(ensure_dyn_lds((const void*)sru_fwd_cs_kernel<8, true>, sru_fwd_cs_lds<8>(true)));
                hipLaunchKernelGGL((sru_fwd_cs_kernel<8, true>), dim3(grid), dim3(512), sru_fwd_cs_lds<8>(true), s, a); }
      else hipLaunchKernelGGL((sru_fwd_cs_kernel<4, true>), dim3(grid), dim3(256), sru_fwd_cs_lds<4>(true), s, a);
    } else if (w8) hipLaunchKernelGGL((sru_fwd_cs_kernel<8, false>), dim3(grid), dim3(512), sru_fwd_cs_lds<8>(), s, a);
    else hipLaunchKernelGGL((sru_fwd_cs_kernel<4, false>), dim3(grid), dim3(256), sru_fwd_cs_lds<4>(), s, a);
    sru_path_count(SRU_PATH_FWD_CS + 2 * (w8 ? 1 : 0) + (img ? 1 : 0));
  } else {
    hipLaunchKernelGGL(sru_fwd_kernel, dim3(cdiv((long)a.B * ncols, SRU_THREADS)), dim3(SRU_THREADS), 0, s, a);
    sru_path_count(SRU_PATH_FWD);
  }
  LAUNCH_CHECK();
  return GT_OK;
}
int sru_launch_bwd(const SruArgs& a, hipStream_t s) {
  const int ncols = a.H * a.dirs;
  if (sru_coop()) {
    const int grid = cdiv((long)a.B * ncols, 64);
    const bool w8 = sru_coop_waves(a.B, ncols) == 8, img = a.dU_b != nullptr;
#define GT_SRU_CS_LAUNCH(NW_, B16_)                                                                                           \
    do {                                                                                                                     \
      CHK(ensure_dyn_lds((const void*)sru_bwd_cs_kernel<NW_, B16_>, sru_bwd_cs_lds<NW_>(B16_)));                             \
      hipLaunchKernelGGL((sru_bwd_cs_kernel<NW_, B16_>), dim3(grid), dim3(64 * NW_), sru_bwd_cs_lds<NW_>(B16_), s, a);        \
    } while (0)
    if (img) { if (w8) GT_SRU_CS_LAUNCH(8, true); else GT_SRU_CS_LAUNCH(4, true); }
    else { if (w8) GT_SRU_CS_LAUNCH(8, false); else GT_SRU_CS_LAUNCH(4, false); }
#undef GT_SRU_CS_LAUNCH
    sru_path_count(SRU_PATH_BWD_CS + 2 * (w8 ? 1 : 0) + (img ? 1 : 0));
  } else {
    hipLaunchKernelGGL(sru_bwd_kernel, dim3(cdiv((long)a.B * ncols, SRU_THREADS)), dim3(SRU_THREADS), 0, s, a);
    sru_path_count(SRU_PATH_BWD);
  }
  LAUNCH_CHECK();
  return GT_OK;
}
// ... and of the three helper kernels
int sru_launch_input_mask(float* mul, int B, int n, float keep_scale, uint32_t thresh, uint32_t key0, uint32_t key1, const float* inj,
                          int seq_mul, int seq_add, hipStream_t s) {
  hipLaunchKernelGGL(sru_input_mask_kernel, dim3(cdiv((long)B * n, 256)), dim3(256), 0, s, mul, B, n, keep_scale, thresh, key0, key1, inj, seq_mul,
                     seq_add);
  sru_path_count(SRU_PATH_INPUT_MASK);
  LAUNCH_CHECK();
  return GT_OK;
}
int sru_launch_input_dropout(const float* x, int ldx, float* y, int ldy, int B, int T, int n, const float* mul, hipStream_t s) {
  hipLaunchKernelGGL(sru_input_dropout_kernel, dim3(cdiv((long)B * T * n, 256)), dim3(256), 0, s, x, ldx, y, ldy, B, T, n, mul);
  sru_path_count(SRU_PATH_INPUT_DROPOUT);
  LAUNCH_CHECK();
  return GT_OK;
}
int sru_launch_dx_adv_finish(const SruDxAdvArgs& f, hipStream_t s) {
  hipLaunchKernelGGL(sru_dx_adv_finish_kernel, dim3(cdiv(cdiv(f.rows * f.Da, 4), 256)), dim3(256), 0, s, f);
  sru_path_count(SRU_PATH_DX_ADV_FINISH);
  LAUNCH_CHECK();
  return GT_OK;
}
// Measured and dropped (round 4, gpurun_out/r4k): 32 columns per workgroup (twice the recurrence waves per CU, half of every wave
// idle) for the shapes that give fewer than three 64-column workgroups per CU -- cfg4 (B = 16, T = 2048) 11.36 vs 10.84 ms, the
// hparams-default generator at B = 32 9.49 vs 9.32 ms: the scan is not bound by one wave's per-frame latency.
// bf16 storage per role: GT_OPT_MATMUL_BF16 puts the generator's stack on the bf16 images; a discriminator's stays float32 under it and
// has its own switch, GT_OPT_SRU_D_BF16.  Either needs hidden_dim % 8 == 0 (16-byte rows of the images), else float32.
bool sru_b16(const gt_engine* e, int role) {
  return (role == GT_ROLE_G ? e->matmul_bf16 : e->sru_d_bf16) && (e->net[role].d.hidden_dim & 7) == 0;
}
// a discriminator on the bf16 path reads its [x | adv] rows as float32 only where layer 0's scan takes them as the highway input x'
bool sru_d_needs_f32_input(const gt_engine* e) {
  const Net& D = e->net[GT_ROLE_D];
  return !sru_b16(e, GT_ROLE_D) || D.sru.empty() || D.sru[0].k == 3;
}
// (the float32-storage products of a stack run at product_prec(e, role): a discriminator's stay float32 products)
// ... with the cooperative scans on whole 8-frame blocks and whole workgroups: the scans write the bf16 images of the next product's input
static bool sru_fold(const gt_engine* e, int role, int nseq, int T) {
  const Net& G = e->net[role];
  const int H = G.d.hidden_dim, ncols = H * (G.d.bidirectional ? 2 : 1);
  return sru_b16(e, role) && sru_coop() && T % 8 == 0 && H % 64 == 0 && ((long)nseq * ncols) % 64 == 0;
}
// The SRU stack of network `role` over nseq sequences (rows = nseq * T of x, row pitch ld_x): per layer the U product and the scan, the
// variational dropout of both sites; stashes U / h / c (and the dropped inputs and mask tables) in the role's buffers.  passes / npass:
// the dropout passes of the row groups (the D step runs the natural and the generated sequences as ONE batch of 2B: two groups of
// nseq / 2 sequences).  Sequence lengths are ignored, as in the reference.  *top / *ld_top: the top layer's h.
int sru_stack_forward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, hipStream_t s,
                      const float** top, int* ld_top, const CatSrc* cat0, bool want_w) {
  Net& G = e->net[role];
  NetWs& W = e->ws[role];
  const int prec = product_prec(e, role);
  const int B = nseq;
  const long N = (long)B * T;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1, ncols = H * dirs;
  if (npass < 1 || nseq % npass) return fail(GT_ERR_INVALID, "SRU stack: %d sequences do not split into %d passes", nseq, npass);
  const float* in = x;
  int ld_in = ld_x;
  // GT_OPT_MATMUL_BF16: the (dropped) layer inputs go through bf16 images in both orientations, W through bf16 shadows in
  // both orientations: U = xin . WT^T, dW = xinT . dUT^T, d in = dU . W^T are all the k-contiguous bf16 product
  const bool b16 = sru_b16(e, role);
  const bool want_t = G.d.grads != nullptr && want_w;      // the transposed images feed the weight gradients only
  const int Lc_ = G.d.num_hidden, nent = sru_b16_entries(e, role);
  if (!(b16 && cat0) && !x) return fail(GT_ERR_INVALID, "SRU stack: null input");
  if (b16) {      // the shadows are re-made at every call: a discriminator's weights change between the two passes of one step
    CHK(resize_owned(W.s_in_b, nent)); CHK(resize_owned(W.ssh, nent));
    for (int l = 0; l < nent; ++l) {
      const float* Wl = l < Lc_ ? G.sru[l].W : G.last.W;
      const int rows = l < Lc_ ? G.sru[l].in : G.last.out, cols = l < Lc_ ? ncols * G.sru[l].k : G.last.in;
      CHK(W.ssh[l].ensure(rows, cols));
      CHK(shadow_cast(W.ssh[l], Wl, 0, rows, cols, s));
    }
  }
  // bf16 storage + cooperative scans: layer l's scan writes the bf16 input images of the product behind it (layer l + 1's U product, or
  // hidden2out) itself -- with that layer's variational input dropout applied -- so the multiplier tables of ALL layers are drawn first
  const bool rdrop_all = G.training && G.d.rnn_dropout > 0.f;
  const bool fold = sru_fold(e, role, nseq, T);
  if (rdrop_all) {
    for (int l = 0; l < G.d.num_hidden; ++l) {
      const SruLayerP& L = G.sru[l];
      CHK(W.xmask[l].ensure((size_t)B * L.in * sizeof(float)));
      // gt_set_dropout_mask(role, pass, 2*l): [B][n_in]
      CHK(sru_draw_table(e, G, role, l, 0, W.xmask[l].as<float>(), B, L.in, G.d.rnn_dropout, 1.f / (1.f - G.d.rnn_dropout), passes, npass, s));
    }
  }
  if (role != GT_ROLE_G && G.training && G.d.dropout > 0.f) {      // a discriminator's output-dropout keep tables (the generator's scans draw theirs inline)
    for (int l = 0; l + 1 < G.d.num_hidden; ++l) {
      CHK(W.omask[l].ensure((size_t)B * ncols * sizeof(float)));
      CHK(sru_draw_table(e, G, role, l, 1, W.omask[l].as<float>(), B, ncols, G.d.dropout, 1.f, passes, npass, s));
    }
  }
  bool img_ready = false;       // the current layer's input images were written by the scan underneath
  for (int l = 0; l < G.d.num_hidden; ++l) {
    const SruLayerP& L = G.sru[l];
    CHK(W.u[l].ensure((size_t)N * ncols * L.k * sizeof(float)));
    CHK(W.h[l].ensure((size_t)N * ncols * sizeof(float)));
    CHK(W.c[l].ensure((size_t)N * ncols * sizeof(float)));
    const float* xin = in;
    int ld_xin = ld_in;
    const bool rdrop = rdrop_all;      // (variational input dropout, mask shared over time: the multipliers [B][n_in] were drawn above)
    if (rdrop && !b16) {      // float32 products read a dropped float32 copy
      CHK(W.xdrop[l].ensure((size_t)N * L.in * sizeof(float)));
      CHK(sru_launch_input_dropout(in, ld_in, W.xdrop[l].as<float>(), L.in, B, T, L.in, (const float*)W.xmask[l].as<float>(), s));
      xin = W.xdrop[l].as<float>();
      ld_xin = L.in;
    }
    if (b16) {
      B16Img& I = W.s_in_b[l];
      CHK(I.ensure(N, L.in, want_t));
      if (img_ready) {
        // written by the scan of the layer underneath (SruArgs::nx_*): no cast pass
      } else if (l == 0 && cat0) {   // a discriminator's [x | adv] rows: one pass from the caller's tensors to both images, dropout riding along
        if (rdrop) {
          const CatDropSrc src{*cat0, W.xmask[0].as<float>(), T, L.in};
          CHK(catdrop_cast_transpose(src, N, L.in, I.r(), I.ld, want_t ? I.t() : (__bf16*)nullptr, I.ldt, s));
        } else {
          CHK(cat_cast_transpose(*cat0, N, L.in, I.r(), I.ld, want_t ? I.t() : (__bf16*)nullptr, I.ldt, s));
        }
      } else if (rdrop) {            // bf16 products: dropout rides in the cast, the dropped input exists as bf16 images only
        const SeqDropSrc src{in, ld_in, W.xmask[l].as<float>(), T, L.in};
        CHK(seqdrop_cast_transpose(src, N, L.in, I.r(), I.ld, want_t ? I.t() : (__bf16*)nullptr, I.ldt, s));
      } else {
        CHK(cast_transpose(xin, ld_xin, N, L.in, I.r(), I.ld, want_t ? I.t() : (__bf16*)nullptr, I.ldt, nullptr, false, &e->colp, s));
      }
      CHK(b16_forward(I.r(), I.ld, N, W.ssh[l].t(), W.ssh[l].ldwt, ncols * L.k, L.in, nullptr, ACT_NONE, no_drop(),      // WT [ncols*k][n_in]: k = n_in contiguous
                      B16Dst(W.u[l].as<float>(), ncols * L.k), s));
    } else if ((L.in & 3) == 0 && N >= 4096) {
      // U = xin W with W (n_in, ncols*k): the k-contiguous (NT) product runs at 146 TFLOP/s on these shapes, the n-contiguous (NN)
      // one at 114 (profiles/r03_sru_fp32_summary.md: 1.41 vs 1.80 ms per layer) -- multiply by a transposed copy of W, re-made
      // from the caller's parameter buffer before every pass (12 MB, ~10 us)
      CHK(W.wt[l].ensure((size_t)ncols * L.k * L.in * sizeof(float)));
      launch_transpose_f32(L.W, L.in, ncols * L.k, ncols * L.k, W.wt[l].as<float>(), L.in, s);
      LAUNCH_CHECK();
      CHK(plain_product(GEMM_NT, xin, ld_xin, W.wt[l].as<float>(), L.in, W.u[l].as<float>(), ncols * L.k, N, ncols * L.k, L.in, false, prec, s));
    } else {  // U = xin W   (W is (n_in, ncols*k): n-contiguous rows -> NN orientation)
      CHK(plain_product(GEMM_NN, xin, ld_xin, L.W, ncols * L.k, W.u[l].as<float>(), ncols * L.k, N, ncols * L.k, L.in, false, prec, s));
    }
    SruArgs a = sru_args(e, role, W, l, B, T, in, ld_in);
    img_ready = false;
    if (fold) {       // the images of the product behind this layer: layer l + 1's input (its dropout applied), or hidden2out's
      const int nl = l + 1;
      const int n_in_next = nl < Lc_ ? G.sru[nl].in : G.last.in;
      if (nl < nent && n_in_next == ncols) {      // (a discriminator's top layer writes none: the fused head reads the float32 h)
        B16Img& NI = W.s_in_b[nl];
        CHK(NI.ensure(N, ncols, want_t));
        a.nx_b = NI.r(); a.ld_nxb = NI.ld; a.nx_bt = want_t ? NI.t() : (__bf16*)nullptr; a.ld_nxbt = NI.ldt;
        a.nx_mul = (nl < Lc_ && rdrop_all) ? W.xmask[nl].as<float>() : (const float*)nullptr;
        img_ready = true;
      }
    }
    CHK(sru_launch_fwd(a, s));      // (the image form: a.nx_b is set)
    in = W.h[l].as<float>();
    ld_in = ncols;
  }
  *top = in; *ld_top = ld_in;
  return GT_OK;
}

// x (N, in_dim) -> y_hat (N, out_dim): the generator's stack + hidden2out
int sru_forward(gt_engine* e, const float* x, int B, int T, float* y_hat, hipStream_t s) {
  Net& G = e->net[GT_ROLE_G];
  NetWs& W = e->ws[GT_ROLE_G];
  const int Lc = G.d.num_hidden;
  const int passes[1] = {0};
  OutTop top;
  CHK(sru_stack_forward(e, GT_ROLE_G, x, G.d.in_dim, B, T, passes, 1, s, &top.x, &top.ld));
  if (sru_b16(e, GT_ROLE_G)) {
    top.img = &W.s_in_b[Lc]; top.sh = &W.ssh[Lc]; top.want_t = G.d.grads != nullptr;
    top.img_ready = sru_fold(e, GT_ROLE_G, B, T);      // hidden2out's input images were written by the last layer's scan
  }
  return out_layer_forward(e, GT_ROLE_G, top, (long)B * T, y_hat, s);
}

// gy (N, out_dim) = dL/dy_hat -> parameter gradients of hidden2out and of every SRU layer of the generator
int sru_backward(gt_engine* e, const float* x, const float* gy, int B, int T, hipStream_t s) {
  Net& G = e->net[GT_ROLE_G];
  NetWs& W = e->ws[GT_ROLE_G];
  const long N = (long)B * T;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1, ncols = H * dirs, Lc = G.d.num_hidden;
  int inmax = ncols;
  for (auto& L : G.sru) inmax = std::max(inmax, L.in);
  CHK(W.dout.ensure((size_t)2 * N * std::max(ncols, inmax) * sizeof(float)));      // first half: gradient w.r.t. the top layer's h
  OutTop top{W.h[Lc - 1].as<float>(), ncols};
  if (sru_b16(e, GT_ROLE_G) && (int)W.s_in_b.size() == Lc + 1 && (int)W.ssh.size() == Lc + 1) { top.img = &W.s_in_b[Lc]; top.sh = &W.ssh[Lc]; }
  CHK(out_layer_backward(e, GT_ROLE_G, gy, G.d.out_dim, N, top, OutGrad{B16Dst(W.dout.as<float>(), ncols), ACT_NONE, no_drop(), false}, nullptr, s));
  const int passes[1] = {0};
  return sru_stack_backward(e, GT_ROLE_G, x, G.d.in_dim, B, T, passes, 1, true, nullptr, s);
}

// From the gradient w.r.t. the top layer's h (first half of the role's `dout` buffer, row pitch ncols) down through the stack: weight and
// bias gradients of every layer (want_w), and -- dx_adv != null, what a discriminator hands back to the generator -- the gradient w.r.t.
// the adversarial columns [col0, col0 + Da) of the LAST row group's input rows (the generated sequences), written at pitch Da.  Only that
// slice of d input is ever read (train.py:265,274,307-308), so only that slice is formed.
int sru_stack_backward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, bool want_w,
                       float* dx_adv, hipStream_t s) {
  (void)passes;      // (the passes' dropout tables are the forward's stash)
  Net& G = e->net[role];
  NetWs& W = e->ws[role];
  const int prec = product_prec(e, role);
  const int B = nseq;
  const long N = (long)B * T;
  const int H = G.d.hidden_dim, dirs = G.d.bidirectional ? 2 : 1, ncols = H * dirs, Lc = G.d.num_hidden;
  const bool acc = G.grads_dirty;
  if (npass < 1 || nseq % npass) return fail(GT_ERR_INVALID, "SRU stack: %d sequences do not split into %d passes", nseq, npass);
  int kmax = 3, inmax = ncols;
  for (auto& L : G.sru) { kmax = std::max(kmax, L.k); inmax = std::max(inmax, L.in); }
  // the generator's buffer is sized by sru_backward; a discriminator's holds two [N][ncols] halves (the head wrote the first one)
  const size_t dh_pitch = role == GT_ROLE_G ? (size_t)std::max(ncols, inmax) : (size_t)ncols;
  CHK(W.dout.ensure((size_t)2 * N * dh_pitch * sizeof(float)));
  CHK(e->s_du.ensure((size_t)N * ncols * kmax * sizeof(float)));
  CHK(e->s_dx.ensure((size_t)2 * N * ncols * sizeof(float)));     // highway gradients of two consecutive layers (read by the layer underneath)
  CHK(e->s_dbias.ensure((size_t)B * 2 * ncols * sizeof(float)));
  float* dh = W.dout.as<float>();
  float* dh_other = dh + (size_t)N * dh_pitch;
  const int nent = sru_b16_entries(e, role);
  const bool b16 = sru_b16(e, role) && (int)W.s_in_b.size() == nent && (int)W.ssh.size() == nent;
  for (int l = Lc - 1; l >= 0; --l) {
    const SruLayerP& L = G.sru[l];
    const float* in = l == 0 ? x : W.h[l - 1].as<float>();
    const int ld_in = l == 0 ? ld_x : ncols;
    const bool rdrop = G.training && G.d.rnn_dropout > 0.f;
    SruArgs a = sru_args(e, role, W, l, B, T, in, ld_in);
    a.dh = dh; a.dU = e->s_du.as<float>();
    // k == 3: the highway gradient goes straight to the layer input.  Without input dropout it is
    // written into the next dh buffer and the GEMM below accumulates onto it.
    auto dx_of = [&](int layer) { return e->s_dx.as<float>() + (size_t)(layer & 1) * N * ncols; };
    float* dx_res = L.k == 3 ? (rdrop ? dx_of(l) : dh_other) : nullptr;
    a.dx = dx_res; a.lddx = ncols;
    if (rdrop && l + 1 < Lc) {      // dh is the raw dU.W^T of the layer above: its input dropout and highway gradient are applied by the scan
      if (G.sru[l + 1].in != ncols || !W.xmask[l + 1].p)
        return fail(GT_ERR_STATE, "SRU backward: layer %d's input-dropout table is missing or not %d wide", l + 1, ncols);
      a.up_mul = W.xmask[l + 1].as<float>();
      a.up_add = G.sru[l + 1].k == 3 ? dx_of(l + 1) : nullptr;
      a.ld_up_add = ncols;
    }
    a.dbias_part = e->s_dbias.as<float>();
    // bf16 storage with the cooperative scans, whole blocks of 8 frames, whole workgroups inside one sequence and one direction: dU
    // leaves the scan as the bf16 images the two products read (no float32 dU, no cast pass)
    const bool du_b16 = b16 && sru_coop() && T % 8 == 0 && H % 64 == 0;
    // (want_w == false, the generator step's pass through a discriminator: the transposed image feeds dW alone and is not written)
    if (du_b16) {
      B16Img& DU = W.du_b;
      CHK(DU.ensure(N, ncols * L.k, want_w));
      a.dU = nullptr; a.dU_b = DU.r(); a.ld_dub = DU.ld; a.dU_bt = want_w ? DU.t() : (__bf16*)nullptr; a.ld_dubt = DU.ldt;
    }
    CHK(sru_launch_bwd(a, s));      // (the image form: a.dU_b is set)
    if (b16 && !du_b16) {      // dU -> bf16 image in both orientations (one pass)
      B16Img& DU = W.du_b;
      CHK(DU.ensure(N, ncols * L.k, want_w));
      CHK(cast_transpose(e->s_du.as<float>(), ncols * L.k, N, ncols * L.k, DU.r(), DU.ld, want_w ? DU.t() : (__bf16*)nullptr, DU.ldt, nullptr, false,
                         &e->colp, s));
    }
    if (want_w) {      // (the generator step's pass through a discriminator launches no weight-gradient kernel: train.py:307-308)
      hipLaunchKernelGGL(slab_reduce_small_kernel, dim3(cdiv(2 * ncols, 64)), dim3(1024), 0, s, e->s_dbias.as<float>(), (long)2 * ncols, B,
                         2 * ncols, L.db, acc ? 1 : 0);
      LAUNCH_CHECK();
      const float* xin = rdrop ? W.xdrop[l].as<float>() : in;
      const int ld_xin = rdrop ? L.in : ld_in;
      if (b16) {
        // dW = xinT . dUT^T over the frames, d in = dU . W^T
        B16Img& DU = W.du_b;
        B16Img& I = W.s_in_b[l];
        CHK(weight_grad_b16(I.t(), I.ldt, DU.t(), DU.ldt, N, L.in, ncols * L.k, L.dW, nullptr, acc, e->slabs, s));
      } else {
        // dW = xin^T dU   (TN: A = xin is m-contiguous over n_in, B = dU)
        CHK(linear_backward_weight(xin, ld_xin, e->s_du.as<float>(), ncols * L.k, N, L.in, ncols * L.k, L.dW, nullptr, acc, e->slabs,
                                   e->colp, prec, s));
      }
      CHK(comm_grads_ready(e, role, L.dW, (long)L.in * ncols * L.k + 2L * ncols, s));
      if (l > 0 && (role == GT_ROLE_G || !e->opt_comm_d_one_msg)) CHK(comm_flush(e, role, s));
    }
    if (l > 0) {
      if (b16) {      // W [n_in][ncols*k]: k contiguous
        CHK(b16_backward_data(W.du_b.r(), W.du_b.ld, N, W.ssh[l].r(), W.ssh[l].ldw, L.in, ncols * L.k, ACT_NONE, nullptr, no_drop(),
                              B16Dst(dh_other, L.in, L.k == 3 && !rdrop), s));
      } else {
        // d in = (dU W^T) (.) mask_in + highway term     (NT: B[n = i][k = c] = W[i*ldw + c])
        CHK(plain_product(GEMM_NT, e->s_du.as<float>(), ncols * L.k, L.W, ncols * L.k, dh_other, L.in, N, L.in, ncols * L.k, L.k == 3 && !rdrop, prec, s));
      }
      std::swap(dh, dh_other);         // (with input dropout: finished by the scan of layer l - 1, SruArgs::up_mul / up_add)
    }
    // l == 0, the generator: no gradient with respect to the network input is produced (nothing upstream of the generator
    // takes one: x is data, train.py:542).  NOTE for anything that wants to read `dh` between layers: with rnn_dropout it
    // is the RAW dU.W^T -- the input-dropout mask and the k = 3 highway term are applied by the next scan's loads.
    if (l == 0 && dx_adv) {
      // l == 0, a discriminator: d input of the generated rows' adversarial columns = dU0[generated rows] . W0[col0 .. col0 + Da, :]^T
      // (NT, M = rows of the last group, N = Da, K = ncols * k) straight into the caller's [rows][Da] buffer, finished per element with
      // layer 0's input-dropout multiplier and, k == 3, the highway gradient of the layer-0 scan (which by-passes the input dropout)
      const int Da = e->Da, col0 = cond_dim(e);
      if (col0 < 0 || col0 + Da > L.in) return fail(GT_ERR_DIM, "SRU discriminator: adversarial columns [%d, %d) outside in_dim %d", col0, col0 + Da, L.in);
      const int Bf = nseq / npass;
      const long Nf = (long)Bf * T, row0 = N - Nf;
      if (b16) {      // the bf16 product from the dU image's row offset and the row slice of the layer-0 shadow (both 16-byte aligned: pitches % 8 == 0)
        CHK(b16_backward_data(W.du_b.r() + (size_t)row0 * W.du_b.ld, W.du_b.ld, Nf, W.ssh[0].r() + (size_t)col0 * W.ssh[0].ldw, W.ssh[0].ldw, Da,
                              ncols * L.k, ACT_NONE, nullptr, no_drop(), B16Dst(dx_adv, Da), s));
      } else {
        CHK(plain_product(GEMM_NT, e->s_du.as<float>() + (size_t)row0 * ncols * L.k, ncols * L.k, L.W + (size_t)col0 * ncols * L.k, ncols * L.k, dx_adv, Da,
                          Nf, Da, ncols * L.k, false, prec, s));
      }
      if (rdrop || L.k == 3) {
        SruDxAdvArgs f;
        f.dx_adv = dx_adv; f.rows = Nf; f.Da = Da; f.T = T;
        f.mul = rdrop ? W.xmask[0].as<float>() + (size_t)(nseq - Bf) * L.in + col0 : nullptr; f.ld_mul = L.in;
        f.hw = L.k == 3 ? dx_res + (size_t)row0 * ncols + col0 : nullptr; f.ld_hw = ncols;
        CHK(sru_launch_dx_adv_finish(f, s));
      }
    }
  }
  return GT_OK;
}

