// libgantts_hip.so -- gradient penalties of the MLP discriminator (R1, WGAN-GP): the second-order pass as a chain of existing products and
// the kernels of grad_penalty_kernels.hip.h, the engine's switch and running record (C ABI: include/gantts_hip.h)
#include <atomic>
#include "engine_internal.hip.h"
#include "grad_penalty_kernels.hip.h"

using namespace gt;

// gt_gp_path_counts: process-wide, one relaxed increment per launch (slots 0 .. 4) or per product call (5 .. 7) on the host
enum { GP_PATH_INTERP = 0, GP_PATH_SLOPE = 1, GP_PATH_ROW = 2, GP_PATH_FINALIZE = 3, GP_PATH_ADD_COLS = 4, GP_PATH_BACKWARD_DATA = 5,
       GP_PATH_FORWARD = 6, GP_PATH_WEIGHT_GRAD = 7 };
static_assert(GP_PATH_WEIGHT_GRAD + 1 == GT_GP_PATH_SLOTS, "gt_gp_path_counts slots");
static std::atomic<int64_t> g_gp_paths[GT_GP_PATH_SLOTS];
static void gp_path_count(int slot) { g_gp_paths[slot].fetch_add(1, std::memory_order_relaxed); }
extern "C" int gt_gp_path_counts(int64_t* counts, int reset) {
  for (int i = 0; i < GT_GP_PATH_SLOTS; ++i) {
    const int64_t v = reset ? g_gp_paths[i].exchange(0, std::memory_order_relaxed) : g_gp_paths[i].load(std::memory_order_relaxed);
    if (counts) counts[i] = v;
  }
  return GT_OK;
}

int gp_row_blocks(long rows) { return cdiv(rows, GP_ROWS_PER_WG); }

// the keys of a step's eps draws: the engine's seed and step counter under a salt of their own (no dropout site's (key0, key1): those
// mix a site number below 64 per step into the same seed, philox_site_spec)
void gp_eps_keys(const gt_engine* e, uint32_t* key0, uint32_t* key1) {
  const uint64_t m = (e->step_counter + 1ULL) * 0xD6E8FEB86659FD93ULL;
  *key0 = (uint32_t)(e->seed ^ m) ^ 0x6A09E667u;
  *key1 = (uint32_t)((e->seed >> 32) ^ (m >> 32)) + 0xBB67AE85u;
}

int launch_gp_interp(const float* real, const float* fake, int ldf, const int* idx, int na, const float* eps_in, uint32_t key0, uint32_t key1,
                     float* out, int ldo, int col0, long rows, float* eps_out, hipStream_t s) {
  if (rows < 1 || na < 1 || rows * na > 0x7fffffffL * GP_THREADS) return fail(GT_ERR_INVALID, "gradient penalty: empty or oversized interpolation");
  hipLaunchKernelGGL(gp_interp_kernel, dim3(cdiv(rows * na, GP_THREADS)), dim3(GP_THREADS), 0, s, real, fake, ldf, idx, na, eps_in, key0, key1, out,
                     ldo, col0, rows, eps_out);
  LAUNCH_CHECK();
  gp_path_count(GP_PATH_INTERP);
  return GT_OK;
}
static int launch_gp_slope(const float* X, int ldx, const float* H, int ldh, const DropoutSpec& d, float* Y, int ldy, long rows, int cols,
                           hipStream_t s) {
  hipLaunchKernelGGL(gp_slope_kernel, dim3(cdiv(rows * cols, GP_THREADS)), dim3(GP_THREADS), 0, s, X, ldx, H, ldh, d, Y, ldy, rows, cols);
  LAUNCH_CHECK();
  gp_path_count(GP_PATH_SLOPE);
  return GT_OK;
}

// The four parts over `rows` rows whose activations and dropout sites are in c.l[]: the one place that issues them, for the
// step (d_pass_penalty, eng_step.hip) and the parity hook alike.
int launch_grad_penalty(const GpCall& c, hipStream_t s) {
  const int L = c.L, Da = c.Da, cd = c.cd;
  const long rows = c.rows;
  if (L < 1 || L > GT_GP_MAX_LAYERS || Da < 1 || cd < 0 || rows < 1 || rows > 0x7fffffffL || c.ld_g < Da || (c.kind != GP_R1 && c.kind != GP_WGAN))
    return fail(GT_ERR_INVALID, "gradient penalty: malformed call");
  const int nblk = gp_row_blocks(rows);
  if (2L * nblk > c.part_cap) return fail(GT_ERR_INVALID, "gradient penalty: partial buffer too small for %d workgroups", nblk);
  const GpLayer& top = c.l[L - 1];
  // 1. the gradient chain, seed 1: a_{L-1} = s_{L-1} (.) w, a_{l-1} = s_{l-1} (.) (a_l W_l), g = a_0 W_0[:, adv]
  CHK(launch_gp_slope(c.w_last, 0, top.H, top.out, top.spec, top.a, top.out, rows, top.out, s));
  for (int l = L - 1; l >= 1; --l) {
    const GpLayer& u = c.l[l]; const GpLayer& d = c.l[l - 1];
    CHK(linear_backward_data(u.a, u.out, u.W, u.in, 0, d.a, d.out, rows, u.out, u.in, ACT_LEAKY_DROPOUT, d.H, d.out, d.spec, c.prec, s));
    gp_path_count(GP_PATH_BACKWARD_DATA);
  }
  const GpLayer& l0 = c.l[0];
  CHK(linear_backward_data(l0.a, l0.out, l0.W, l0.in, cd, c.g, c.ld_g, rows, l0.out, Da, ACT_NONE, nullptr, 0, no_drop(), c.prec, s));
  gp_path_count(GP_PATH_BACKWARD_DATA);
  if (c.g_copy) HIPCHK(hipMemcpyAsync(c.g_copy, c.g, (size_t)rows * c.ld_g * sizeof(float), hipMemcpyDeviceToDevice, s));
  // 2. per row: phi and r (in place of g), the partials of the two sums; then their fixed-order total
  GpRowArgs ra;
  memset(&ra, 0, sizeof(ra));
  ra.g = c.g; ra.ld = c.ld_g; ra.na = Da; ra.kind = c.kind; ra.rows = rows; ra.mask = c.mask; ra.inv_tv_dev = c.inv_tv_dev; ra.inv_tv = c.inv_tv;
  ra.weight = c.weight; ra.phi = c.phi; ra.nrm = c.nrm; ra.part = c.part; ra.nblk = nblk;
  hipLaunchKernelGGL(gp_row_kernel, dim3(nblk), dim3(GP_THREADS), 0, s, ra);
  LAUNCH_CHECK();
  gp_path_count(GP_PATH_ROW);
  hipLaunchKernelGGL(gp_finalize_kernel, dim3(1), dim3(GP_THREADS), 0, s, (const double*)c.part, nblk, c.inv_tv_dev, c.inv_tv, c.sums, c.rec);
  LAUNCH_CHECK();
  gp_path_count(GP_PATH_FINALIZE);
  // 3. the tangent chain c_0 = s_0 (.) (r W_0[:, adv]^T), c_l = s_l (.) (c_{l-1} W_l^T), and 4. the weight gradients, added: each layer's right
  // behind the product that made its operand.  No bias gradient is produced anywhere (db = null)
  CHK(linear_backward_weight(l0.a, l0.out, c.g, c.ld_g, rows, l0.out, Da, c.dw0s, nullptr, false, *c.slabs, *c.colp, c.prec, s));
  gp_path_count(GP_PATH_WEIGHT_GRAD);
  hipLaunchKernelGGL(gp_add_cols_kernel, dim3(cdiv((long)l0.out * Da, GP_THREADS)), dim3(GP_THREADS), 0, s, (const float*)c.dw0s, Da, l0.dW, l0.in, cd,
                     l0.out);
  LAUNCH_CHECK();
  gp_path_count(GP_PATH_ADD_COLS);
  CHK(linear_forward(c.g, c.ld_g, l0.W + cd, l0.in, nullptr, l0.c, l0.out, rows, Da, l0.out, ACT_NONE, no_drop(), c.prec, s));
  gp_path_count(GP_PATH_FORWARD);
  CHK(launch_gp_slope(l0.c, l0.out, l0.H, l0.out, l0.spec, l0.c, l0.out, rows, l0.out, s));
  for (int l = 1; l < L; ++l) {
    const GpLayer& u = c.l[l]; const GpLayer& d = c.l[l - 1];
    CHK(linear_backward_weight(u.a, u.out, d.c, d.out, rows, u.out, u.in, u.dW, nullptr, true, *c.slabs, *c.colp, c.prec, s));
    gp_path_count(GP_PATH_WEIGHT_GRAD);
    CHK(linear_forward(d.c, d.out, u.W, u.in, nullptr, u.c, u.out, rows, u.in, u.out, ACT_NONE, no_drop(), c.prec, s));
    gp_path_count(GP_PATH_FORWARD);
    CHK(launch_gp_slope(u.c, u.out, u.H, u.out, u.spec, u.c, u.out, rows, u.out, s));
  }
  // d last_linear.weight += column sums of c_{L-1} (the weight-gradient path's bias route, with the head's weight gradient as its destination)
  CHK(linear_backward_weight(top.c, top.out, nullptr, 0, rows, top.out, 0, nullptr, c.dw_last, true, *c.slabs, *c.colp, c.prec, s));
  gp_path_count(GP_PATH_WEIGHT_GRAD);
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// the engine's side
// ------------------------------------------------------------------------------------------
int gp_refusals(const gt_engine* e) {
  if (e->gp.kind == GP_OFF) return GT_OK;
  const Net& D = e->net[GT_ROLE_D];
  if (D.bound && D.d.arch != GT_ARCH_MLP)
    return fail(GT_ERR_INVALID, "gt_set_grad_penalty: an LSTMRNN or SRURNN discriminator is not supported (the closed form is the MLP's)");
  if (e->matmul_bf16)
    return fail(GT_ERR_INVALID, "gt_set_grad_penalty: bf16 products (GT_OPT_MATMUL_BF16) are not supported for the penalised discriminator");
  if (e->comm || e->dp_world > 1)
    return fail(GT_ERR_INVALID, "gt_set_grad_penalty: a sharded or communicating engine (gt_set_shard, gt_comm_*) is not supported yet");
  if (e->sn.on)
    return fail(GT_ERR_INVALID, "gt_set_grad_penalty: spectral normalisation (gt_set_spectral_norm) is on; the two together are not supported yet");
  return GT_OK;
}
extern "C" int gt_set_grad_penalty(gt_engine* e, int role, int kind, float weight) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  if (role != GT_ROLE_D) return fail(GT_ERR_INVALID, "gt_set_grad_penalty: role %d -- the gradient penalty is the discriminator's (role 1) alone", role);
  if (kind != GP_OFF && kind != GP_R1 && kind != GP_WGAN)
    return fail(GT_ERR_INVALID, "gt_set_grad_penalty: kind %d -- 0 (off), 1 (r1) or 2 (wgan-gp)", kind);
  if (!(weight >= 0.f) || !(weight <= 3.402823466e+38f))
    return fail(GT_ERR_INVALID, "gt_set_grad_penalty: weight = %g -- a finite value >= 0", (double)weight);
  GpState& G = e->gp;
  const int was = G.kind;
  G.kind = kind;
  if (int r = gp_refusals(e)) { G.kind = was; return r; }
  G.weight = weight;
  if (kind != GP_OFF && !G.rec.p) {
    CHK(G.rec.ensure(3 * sizeof(double)));
    HIPCHK(hipMemset(G.rec.p, 0, 3 * sizeof(double)));
  }
  if (was != kind) on_penalty_kind_changed(e);
  return GT_OK;
}
extern "C" int gt_set_gp_epsilon(gt_engine* e, const float* eps) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  e->gp.eps_inj = eps;
  return GT_OK;
}
extern "C" int gt_grad_penalty_result(gt_engine* e, double* penalty_mean, double* grad_norm_mean, int64_t* steps, int reset) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  GpState& G = e->gp;
  double h[3] = {0.0, 0.0, 0.0};
  if (G.rec.p) {
    HIPCHK(hipStreamSynchronize(G.stream));
    HIPCHK(hipMemcpy(h, G.rec.p, sizeof(h), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(G.rec.p, 0, sizeof(h)));
  }
  const double n = h[2] > 0.0 ? h[2] : 1.0;
  if (penalty_mean) *penalty_mean = h[0] / n;
  if (grad_norm_mean) *grad_norm_mean = h[1] / n;
  if (steps) *steps = (int64_t)h[2];
  return GT_OK;
}
// parity: the last WGAN-GP step's eps draws [N] and x_hat image [N][Da] (dense), device buffers of the caller, either may be null
extern "C" int gt_grad_penalty_peek(gt_engine* e, float* eps, float* x_hat, void* stream) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  GpState& G = e->gp;
  if (!G.img || G.img_rows < 1) return fail(GT_ERR_STATE, "gt_grad_penalty_peek: no wgan-gp step has run");
  hipStream_t s = (hipStream_t)stream;
  if (eps) HIPCHK(hipMemcpyAsync(eps, G.eps.p, (size_t)G.img_rows * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (x_hat) HIPCHK(hipMemcpy2DAsync(x_hat, (size_t)e->Da * sizeof(float), G.img + G.img_col0, (size_t)G.img_ld * sizeof(float), (size_t)e->Da * sizeof(float),
                                     (size_t)G.img_rows, hipMemcpyDeviceToDevice, s));
  return GT_OK;
}
