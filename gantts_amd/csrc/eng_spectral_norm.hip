// libgantts_hip.so -- spectral normalisation of the MLP discriminator: the job table, the five launches, the engine's use of them and
// gt_set_spectral_norm (C ABI: include/gantts_hip.h; kernels: spectral_norm_kernels.hip.h)
#include <atomic>
#include "engine_internal.hip.h"
#include "spectral_norm_kernels.hip.h"

using namespace gt;

// gt_sn_path_counts: process-wide, one relaxed increment per launch on the host
enum { SN_PATH_WTU = 0, SN_PATH_WV = 1, SN_PATH_FINISH = 2, SN_PATH_GW_PARTIAL = 3, SN_PATH_PROJECT = 4 };
static_assert(SN_PATH_PROJECT + 1 == GT_SN_PATH_SLOTS, "gt_sn_path_counts slots");
static std::atomic<int64_t> g_sn_paths[GT_SN_PATH_SLOTS];
static void sn_path_count(int slot) { g_sn_paths[slot].fetch_add(1, std::memory_order_relaxed); }
extern "C" int gt_sn_path_counts(int64_t* counts, int reset) {
  for (int i = 0; i < GT_SN_PATH_SLOTS; ++i) {
    const int64_t v = reset ? g_sn_paths[i].exchange(0, std::memory_order_relaxed) : g_sn_paths[i].load(std::memory_order_relaxed);
    if (counts) counts[i] = v;
  }
  return GT_OK;
}

struct SnPlan {
  SnJobs jobs;
  SnRest rest;
  int col_blocks, row_blocks, elem_blocks, rest_blocks;
  long sum_out, sum_in, n_flat;
};

int sn_plan_build(const SnLayerDesc* layers, int n, long n_flat, SnPlan** out) {
  if (!layers || !out || n < 1 || n > SN_MAX_JOBS) return fail(GT_ERR_INVALID, "spectral norm: %d layers (1 .. %d)", n, SN_MAX_JOBS);
  SnPlan* p = new SnPlan();
  memset(p, 0, sizeof(*p));
  p->jobs.n = n; p->n_flat = n_flat;
  long pos = 0, rest_total = 0;
  for (int q = 0; q < n; ++q) {
    const SnLayerDesc& L = layers[q];
    if (L.out < 1 || L.in < 1 || L.out > SN_MAX_DIM || L.in > SN_MAX_DIM) {
      delete p;
      return fail(GT_ERR_INVALID, "spectral norm: layer %d is (%d, %d); out and in must lie in [1, %d]", q, L.out, L.in, SN_MAX_DIM);
    }
    const long cnt = (long)L.out * L.in;
    if (L.w_off < pos || L.w_off + cnt > n_flat) {
      delete p;
      return fail(GT_ERR_INVALID, "spectral norm: layer %d (offset %ld, %ld elements) overlaps its predecessor or leaves the flat buffer (%ld)", q, L.w_off, cnt, n_flat);
    }
    if (L.w_off > pos) { p->rest.off[p->rest.n_rest] = pos; p->rest.n[p->rest.n_rest] = L.w_off - pos; ++p->rest.n_rest; rest_total += L.w_off - pos; }
    SnJob& J = p->jobs.j[q];
    J.w_off = L.w_off; J.out = L.out; J.in = L.in; J.u_off = (int)p->sum_out; J.v_off = (int)p->sum_in;
    J.cb0 = p->col_blocks; J.rb0 = p->row_blocks; J.eb0 = p->elem_blocks;
    J.nb = cdiv(L.w_off + cnt - (L.w_off & ~3L), SN_CHUNK);
    p->col_blocks += cdiv(L.in, 64); p->row_blocks += cdiv(L.out, 4); p->elem_blocks += J.nb;
    p->sum_out += L.out; p->sum_in += L.in;
    pos = L.w_off + cnt;
  }
  if (pos < n_flat) { p->rest.off[p->rest.n_rest] = pos; p->rest.n[p->rest.n_rest] = n_flat - pos; ++p->rest.n_rest; rest_total += n_flat - pos; }
  p->rest_blocks = rest_total > 0 ? (int)std::min<long>(64, cdiv(rest_total, SN_THREADS)) : 0;
  *out = p;
  return GT_OK;
}
void sn_plan_free(SnPlan* p) { delete p; }
long sn_plan_sum_out(const SnPlan* p) { return p->sum_out; }
long sn_plan_sum_in(const SnPlan* p) { return p->sum_in; }
int sn_plan_partials(const SnPlan* p) { return p->elem_blocks + p->rest_blocks; }
size_t sn_plan_bytes(const SnPlan* p) {
  return (size_t)(p->sum_in + p->sum_out + p->elem_blocks + p->jobs.n) * sizeof(double) + (size_t)p->jobs.n * sizeof(float);
}
SnBufs sn_plan_bufs(const SnPlan* p, void* ws) {
  SnBufs b;
  b.t = (double*)ws; b.r = b.t + p->sum_in; b.sp = b.r + p->sum_out; b.s = b.sp + p->elem_blocks; b.sigma = (float*)(b.s + p->jobs.n);
  return b;
}
static bool sn_aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

int launch_sn_prepare(const SnPlan* p, const float* W, float* u, float* v, float* weff, const SnBufs& b, bool iterate, hipStream_t s) {
  SnJobs jobs = p->jobs;
  jobs.vec = sn_aligned16(W, weff) ? 1 : 0;
  if (iterate) {
    hipLaunchKernelGGL(sn_wtu_kernel, dim3(p->col_blocks), dim3(SN_THREADS), 0, s, jobs, W, (const float*)u, b.t);
    LAUNCH_CHECK();
    sn_path_count(SN_PATH_WTU);
  }
  hipLaunchKernelGGL(sn_wv_kernel, dim3(p->row_blocks), dim3(SN_THREADS), 0, s, jobs, W, (const double*)b.t, (const float*)v, b.r, iterate ? 1 : 0);
  LAUNCH_CHECK();
  sn_path_count(SN_PATH_WV);
  hipLaunchKernelGGL(sn_finish_kernel, dim3(p->elem_blocks), dim3(SN_THREADS), 0, s, jobs, W, (const double*)b.t, (const double*)b.r, u, v, b.sigma, weff,
                     iterate ? 1 : 0);
  LAUNCH_CHECK();
  sn_path_count(SN_PATH_FINISH);
  return GT_OK;
}

int launch_sn_project(const SnPlan* p, float* G, const float* weff, const float* u, const float* v, const SnBufs& b, double* norm_part, hipStream_t s) {
  SnJobs jobs = p->jobs;
  jobs.vec = sn_aligned16(G, weff) ? 1 : 0;
  hipLaunchKernelGGL(sn_gw_partial_kernel, dim3(p->elem_blocks), dim3(SN_THREADS), 0, s, jobs, (const float*)G, weff, b.sp);
  LAUNCH_CHECK();
  sn_path_count(SN_PATH_GW_PARTIAL);
  hipLaunchKernelGGL(sn_project_kernel, dim3(p->elem_blocks + p->rest_blocks), dim3(SN_THREADS), 0, s, jobs, p->elem_blocks, p->rest, G, u, v,
                     (const float*)b.sigma, (const double*)b.sp, b.s, norm_part);
  LAUNCH_CHECK();
  sn_path_count(SN_PATH_PROJECT);
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// the engine's side
// ------------------------------------------------------------------------------------------
// every Lin::W of the discriminator: into W_eff when the feature is on, into the caller's buffer otherwise (biases and gradients never move)
void sn_point_weights(gt_engine* e) {
  Net& D = e->net[GT_ROLE_D];
  if (!D.bound) return;
  float* base = e->sn.on ? e->sn.weff.as<float>() : D.d.params;
  auto point = [&](Lin& l) { l.W = base + ((l.b - D.d.params) - (long)l.out * l.in); };
  for (Lin& l : D.hidden) point(l);
  point(D.last);
}
static int sn_plan_of(const Net& D, SnPlan** plan) {
  std::vector<SnLayerDesc> layers;
  auto add = [&](const Lin& l) { SnLayerDesc d; d.out = l.out; d.in = l.in; d.w_off = (l.b - D.d.params) - (long)l.out * l.in; layers.push_back(d); };
  for (const Lin& l : D.hidden) add(l);
  add(D.last);
  return sn_plan_build(layers.data(), (int)layers.size(), (long)D.d.n_params, plan);
}
static int sn_refusals(const gt_engine* e, const Net& D) {
  if (D.d.arch != GT_ARCH_MLP)
    return fail(GT_ERR_INVALID, "gt_set_spectral_norm: an LSTMRNN or SRURNN discriminator is not supported (the MLP discriminator's nn.Linear weights are what is normalised)");
  if (e->comm || e->dp_world > 1)
    return fail(GT_ERR_INVALID, "gt_set_spectral_norm: a sharded or communicating engine (gt_set_shard, gt_comm_*) is not supported yet");
  return GT_OK;
}
static int sn_install(gt_engine* e, float* u, float* v, long n_u, long n_v) {
  Net& D = e->net[GT_ROLE_D];
  CHK(sn_refusals(e, D));
  SnPlan* raw = nullptr;
  CHK(sn_plan_of(D, &raw));
  SnPlanPtr plan(raw);
  if (n_u != sn_plan_sum_out(raw) || n_v != sn_plan_sum_in(raw))
    return fail(GT_ERR_INVALID, "gt_set_spectral_norm: u has %ld and v %ld entries, the bound discriminator needs %ld (sum of out) and %ld (sum of in)", n_u, n_v,
                sn_plan_sum_out(raw), sn_plan_sum_in(raw));
  SnState& S = e->sn;
  CHK(S.weff.ensure((size_t)D.d.n_params * sizeof(float)));
  CHK(S.ws.ensure(sn_plan_bytes(raw)));
  HIPCHK(hipMemset(S.weff.p, 0, (size_t)D.d.n_params * sizeof(float)));
  S.plan = std::move(plan); S.bufs = sn_plan_bufs(raw, S.ws.p);
  S.u = u; S.v = v; S.on = true;
  sn_point_weights(e);
  return GT_OK;
}
extern "C" int gt_set_spectral_norm(gt_engine* e, int role, float* u, float* v, int64_t n_u, int64_t n_v) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  if (role != GT_ROLE_D) return fail(GT_ERR_INVALID, "gt_set_spectral_norm: role %d -- spectral normalisation is the discriminator's (role 1) alone", role);
  SnState& S = e->sn;
  if (!u || !v) {
    if (u || v) return fail(GT_ERR_INVALID, "gt_set_spectral_norm: u and v are both given or both null");
    const bool was = S.on;
    S.on = false; S.u = S.v = nullptr;
    S.plan.reset();
    if (was) { sn_point_weights(e); on_spectral_norm_off(e); }
    return GT_OK;
  }
  if (!e->net[GT_ROLE_D].bound) return fail(GT_ERR_STATE, "gt_set_spectral_norm: bind the discriminator first (the lengths are checked against it)");
  const bool was = S.on;
  CHK(sn_install(e, u, v, (long)n_u, (long)n_v));
  if (!was) on_spectral_norm_on(e);
  return GT_OK;
}
// gt_bind_model(role D) while the feature is on: the registered buffers must fit the new network too
int sn_rebind(gt_engine* e) {
  if (!e->sn.on) return GT_OK;
  const long n_u = sn_plan_sum_out(e->sn.plan.get()), n_v = sn_plan_sum_in(e->sn.plan.get());
  return sn_install(e, e->sn.u, e->sn.v, n_u, n_v);
}

// the head of every discriminator pass: W_eff from the caller's current weights; one power iteration in training mode
int sn_prepare_pass(gt_engine* e, hipStream_t s) {
  SnState& S = e->sn;
  if (!S.on) return GT_OK;
  Net& D = e->net[GT_ROLE_D];
  return launch_sn_prepare(S.plan.get(), D.d.params, S.u, S.v, S.weff.as<float>(), S.bufs, D.training, s);
}
int sn_project_grads(gt_engine* e, double* norm_part, int* n_partial, hipStream_t s) {
  SnState& S = e->sn;
  Net& D = e->net[GT_ROLE_D];
  *n_partial = sn_plan_partials(S.plan.get());
  if (*n_partial > 2048) return fail(GT_ERR_INVALID, "spectral norm: %d squared-norm partials (at most 2048)", *n_partial);
  CHK(launch_sn_project(S.plan.get(), D.d.grads, S.weff.as<float>(), S.u, S.v, S.bufs, norm_part, s));
  return GT_OK;
}
