// libgantts_hip.so -- the epoch ledger (gt_ledger_*, gt_op_epoch_ledger, gt_host_wait_count): train_loop's running sums of a
// phase, added on the device behind each step so that the host waits once per phase instead of three times per batch.
// The only unit that includes ledger_kernels.hip.h (epoch_ledger_kernel has external linkage: a stable name).
#include "engine_internal.hip.h"
#include "ledger_kernels.hip.h"

using namespace gt;

static_assert(LEDGER_SLOTS == GT_LEDGER_SLOTS && LEDGER_HAS_D == GT_LEDGER_HAS_D && LEDGER_HAS_G == GT_LEDGER_HAS_G &&
              LEDGER_HAS_DIST == GT_LEDGER_HAS_DIST && LEDGER_ACOUSTIC == GT_LEDGER_ACOUSTIC && LEDGER_DURATION == GT_LEDGER_DURATION &&
              LEDGER_VC == GT_LEDGER_VC, "include/gantts_hip.h and ledger_kernels.hip.h disagree");
static_assert(sizeof(StepResults) == 12 * sizeof(float), "epoch_ledger_kernel reads the step's results as 12 floats");
static_assert(DIST_NSUM <= 8, "the record keeps 8 doubles for the distortion sums");

constexpr int LEDGER_MAX_PARTIALS = 1024;      // gt_compute_distortions' cap: the same partial count, the same reduction order

static int ledger_flags_ok(int flags, int kind) {
  if (flags <= 0 || (flags & ~(LEDGER_HAS_D | LEDGER_HAS_G | LEDGER_HAS_DIST))) return fail(GT_ERR_INVALID, "ledger flags 0x%x", flags);
  if (kind < LEDGER_ACOUSTIC || kind > LEDGER_VC) return fail(GT_ERR_INVALID, "ledger kind %d", kind);
  return GT_OK;
}

static void launch_epoch_ledger(double* ledger, const float* res, const double* dist, int flags, int kind, int Ds, double logdb_const,
                                hipStream_t s) {
  hipLaunchKernelGGL(epoch_ledger_kernel, dim3(1), dim3(64), 0, s, ledger, res, dist, flags, kind, Ds, logdb_const);
}

extern "C" int gt_ledger_configure(gt_engine* e, int kind, int Ds, const int32_t* col_stat_host, const int32_t* col_role_host, int vuv_col,
                                   const void* stat_mean, const void* stat_std, int stats_f64, double logdb_const) {
  if (!e || !col_stat_host || !col_role_host || !stat_mean || !stat_std) return fail(GT_ERR_INVALID, "null argument");
  if (kind < LEDGER_ACOUSTIC || kind > LEDGER_VC) return fail(GT_ERR_INVALID, "ledger kind %d", kind);
  if (Ds < 1 || vuv_col >= Ds) return fail(GT_ERR_DIM, "bad sizes: Ds=%d vuv_col=%d", Ds, vuv_col);
  std::vector<int> host(2 * (size_t)Ds);
  for (int c = 0; c < Ds; ++c) {
    if (col_stat_host[c] < 0) return fail(GT_ERR_INVALID, "negative statistics index");
    host[c] = col_stat_host[c];
    host[Ds + c] = col_role_host[c];
  }
  EpochLedger& L = e->ledger;
  HIPCHK(hipDeviceSynchronize());      // a record still being added to, tables still being read: all done before they change
  L.configured = false;
  L.off_tab = (GT_LEDGER_SLOTS + 8) * sizeof(double);
  L.off_part = ((L.off_tab + host.size() * sizeof(int) + 255) / 256) * 256;
  CHK(L.rec.ensure(L.off_part + (size_t)LEDGER_MAX_PARTIALS * DIST_NSUM * sizeof(double)));
  CHK(L.len.ensure(1024 * sizeof(int)));
  if (!L.h_out) CHK(L.h_out.alloc(GT_LEDGER_SLOTS * sizeof(double)));
  L.kind = kind; L.Ds = Ds; L.vuv_col = vuv_col; L.stats_f64 = stats_f64 ? 1 : 0; L.logdb_const = logdb_const;
  L.mean = stat_mean; L.stdv = stat_std;
  HIPCHK(hipMemset(L.rec.p, 0, L.off_tab));
  HIPCHK(hipMemcpy(L.col_stat(), host.data(), host.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  L.configured = true;
  return GT_OK;
}

extern "C" int gt_ledger_reset(gt_engine* e, void* stream) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  if (!e->ledger.configured) return fail(GT_ERR_STATE, "gt_ledger_reset before gt_ledger_configure");
  HIPCHK(hipMemsetAsync(e->ledger.record(), 0, GT_LEDGER_SLOTS * sizeof(double), (hipStream_t)stream));
  return GT_OK;
}

// the batch's seven distortion sums into L.dist(): gt_compute_distortions' two launches with everything they read on the device
static int ledger_distortions(EpochLedger& L, const float* y_static, const float* y_hat_static, const int64_t* lengths_dev, int B, int T,
                              hipStream_t s) {
  const long N = (long)B * T;
  const int nblk = (int)std::min<long>(LEDGER_MAX_PARTIALS, cdiv(N, 4));
  CHK(L.len.ensure((size_t)B * sizeof(int)));      // grows (and synchronises) only for a batch of more sequences than any before
  int* len32 = L.len.as<int>();
  hipLaunchKernelGGL(ledger_lengths_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, (const long long*)lengths_dev, B, T, len32);
  if (L.stats_f64)
    hipLaunchKernelGGL(distortion_kernel<double>, dim3(nblk), dim3(256), 0, s, y_static, y_hat_static, L.Ds, (const double*)L.mean,
                       (const double*)L.stdv, L.col_stat(), L.col_role(), L.vuv_col, len32, B, T, L.partials());
  else
    hipLaunchKernelGGL(distortion_kernel<float>, dim3(nblk), dim3(256), 0, s, y_static, y_hat_static, L.Ds, (const float*)L.mean,
                       (const float*)L.stdv, L.col_stat(), L.col_role(), L.vuv_col, len32, B, T, L.partials());
  hipLaunchKernelGGL(distortion_finalize_kernel, dim3(1), dim3(64 * DIST_NSUM), 0, s, L.partials(), nblk, L.dist());
  LAUNCH_CHECK();
  return GT_OK;
}

extern "C" int gt_ledger_add(gt_engine* e, int flags, const float* y_static, const float* y_hat_static, const int64_t* lengths_dev_i64,
                             int B, int T, void* stream) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  EpochLedger& L = e->ledger;
  if (!L.configured) return fail(GT_ERR_STATE, "gt_ledger_add before gt_ledger_configure");
  CHK(ledger_flags_ok(flags, L.kind));
  hipStream_t s = (hipStream_t)stream;
  if (flags & LEDGER_HAS_DIST) {
    if (!y_static || !y_hat_static) return fail(GT_ERR_INVALID, "null tensor");
    if (B < 1 || T < 1 || (long)B * T > 0x3fffffffL) return fail(GT_ERR_DIM, "bad sizes: B=%d T=%d", B, T);
    CHK(ledger_distortions(L, y_static, y_hat_static, lengths_dev_i64, B, T, s));
  }
  launch_epoch_ledger(L.record(), (const float*)e->res(), L.dist(), flags, L.kind, L.Ds, L.logdb_const, s);
  LAUNCH_CHECK();
  return GT_OK;
}

extern "C" int gt_ledger_read(gt_engine* e, double out[GT_LEDGER_SLOTS], void* stream) {
  if (!e || !out) return fail(GT_ERR_INVALID, "null argument");
  EpochLedger& L = e->ledger;
  if (!L.configured) return fail(GT_ERR_STATE, "gt_ledger_read before gt_ledger_configure");
  hipStream_t s = (hipStream_t)stream;
  ++e->results.waits;
  HIPCHK(hipMemcpyAsync(L.h_out, L.record(), GT_LEDGER_SLOTS * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  memcpy(out, L.h_out, GT_LEDGER_SLOTS * sizeof(double));
  return GT_OK;
}

extern "C" int gt_ledger_buffers(gt_engine* e, double** ledger_dev, double** dist_dev) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  if (!e->ledger.configured) return fail(GT_ERR_STATE, "gt_ledger_buffers before gt_ledger_configure");
  if (ledger_dev) *ledger_dev = e->ledger.record();
  if (dist_dev) *dist_dev = e->ledger.dist();
  return GT_OK;
}

extern "C" int gt_op_epoch_ledger(double* ledger_dev, const float* results_dev, const double* dist_dev, int flags, int kind, int Ds,
                                  double logdb_const, void* stream) {
  if (!ledger_dev || !results_dev) return fail(GT_ERR_INVALID, "null argument");
  CHK(ledger_flags_ok(flags, kind));
  if ((flags & LEDGER_HAS_DIST) && !dist_dev) return fail(GT_ERR_INVALID, "GT_LEDGER_HAS_DIST without distortion sums");
  if (Ds < 1) return fail(GT_ERR_DIM, "bad sizes: Ds=%d", Ds);
  launch_epoch_ledger(ledger_dev, results_dev, dist_dev, flags, kind, Ds, logdb_const, (hipStream_t)stream);
  LAUNCH_CHECK();
  return GT_OK;
}

extern "C" int gt_host_wait_count(gt_engine* e, long long* n) {
  if (!e || !n) return fail(GT_ERR_INVALID, "null argument");
  *n = e->results.waits;
  return GT_OK;
}
