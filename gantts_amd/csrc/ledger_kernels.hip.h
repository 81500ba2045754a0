// Epoch ledger (include/gantts_hip.h: gt_ledger_*): the running sums train_loop keeps per phase, kept on the device.
//
// epoch_ledger_kernel is ONE workgroup, launched once per batch behind the step's finalising launches.  Lane i owns slot i of
// the record: it forms the addend the host loop would form (gantts_amd/train.py: train_loop, compute_distortions) -- the same
// operations in the same order, each rounded alone -- and adds it with one load, one add and one vector store.  Nothing else
// touches the record between gt_ledger_reset and gt_ledger_read, so a phase's sums have the bits of the host sums.
//   * float32 results are widened to double and added (python: running_loss[k] += float32 value as a float);
//   * the metric ratios use IEEE double division and square root; contraction is switched off for the kernel, so (C * s) / n
//     stays a rounded product followed by a rounded quotient;
//   * C = 10 / ln 10 * sqrt 2 arrives as a kernel argument from the host (train._LOGDB_CONST): a device log / sqrt need not
//     round as the host's libm does.
// n_frames == 0 (a batch without a valid frame) is NOT defined here: the host raises ZeroDivisionError there and train_loop
// never forms such a batch.  Slots LEDGER_USED .. LEDGER_SLOTS - 1 are reserved and never written.
#pragma once
#include <hip/hip_runtime.h>

namespace gt {
constexpr int LEDGER_SLOTS = 32, LEDGER_USED = 16;
enum LedgerFlag { LEDGER_HAS_D = 1, LEDGER_HAS_G = 2, LEDGER_HAS_DIST = 4 };
enum LedgerKind { LEDGER_ACOUSTIC = 0, LEDGER_DURATION = 1, LEDGER_VC = 2 };
enum LedgerSlot {
  LS_GENERATOR = 0, LS_MSE, LS_MGE, LS_LOSS_REAL_D, LS_LOSS_FAKE_D, LS_LOSS_ADV, LS_DISCRIMINATOR,      // the keys of running_loss
  LS_REAL_CORRECT, LS_FAKE_CORRECT,
  LS_MCD, LS_BAP_MCD, LS_F0_RMSE, LS_VUV_ERR, LS_DUR_RMSE,
  LS_N_D, LS_N_G
};
static_assert(LS_N_G + 1 == LEDGER_USED, "ledger slot table");

// int64 lengths of a device batch -> the int32 lengths distortion_kernel reads, cut to [0, T] (gt_compute_distortions refuses
// anything outside on the host; here there is no host in the path).  in == null: every sequence has T frames.
static __global__ void ledger_lengths_kernel(const long long* __restrict__ in, int B, int T, int* __restrict__ out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  long long n = in ? in[b] : (long long)T;
  n = n < 0 ? 0 : n > T ? (long long)T : n;
  out[b] = (int)n;
}
}  // namespace gt

// res: the step's StepResults as 12 floats -- loss_d, loss_fake_d, loss_real_d, real_correct, fake_correct, loss_mse, loss_mge,
// loss_adv, loss_g, gnorm_d, gnorm_g, tv.  dist: s_mcd, s_bap, s_f0, n_voiced, n_vuv_err, s_mse, n_frames (read only with
// LEDGER_HAS_DIST).  extern "C": the kernel keeps this name in profiles and traces.
extern "C" __global__ __launch_bounds__(64) void epoch_ledger_kernel(double* __restrict__ ledger, const float* __restrict__ res,
                                                                     const double* __restrict__ dist, int flags, int kind, int Ds,
                                                                     double logdb_const) {
#pragma clang fp contract(off)
  using namespace gt;
  const int slot = threadIdx.x;
  if (blockIdx.x || slot >= LEDGER_USED) return;
  const bool has_d = (flags & LEDGER_HAS_D) != 0, has_g = (flags & LEDGER_HAS_G) != 0, has_dist = (flags & LEDGER_HAS_DIST) != 0;
  bool on = false;
  double v = 0.0;
  switch (slot) {
    case LS_DISCRIMINATOR: on = has_d; if (on) v = (double)res[0]; break;
    case LS_LOSS_FAKE_D:   on = has_d; if (on) v = (double)res[1]; break;
    case LS_LOSS_REAL_D:   on = has_d; if (on) v = (double)res[2]; break;
    case LS_REAL_CORRECT:  on = has_d; if (on) v = (double)res[3]; break;
    case LS_FAKE_CORRECT:  on = has_d; if (on) v = (double)res[4]; break;
    case LS_MSE:           on = has_g; if (on) v = (double)res[5]; break;
    case LS_MGE:           on = has_g; if (on) v = (double)res[6]; break;
    case LS_LOSS_ADV:      on = has_g; if (on) v = (double)res[7]; break;
    case LS_GENERATOR:     on = has_g; if (on) v = (double)res[8]; break;
    case LS_N_D:           on = has_d; v = 1.0; break;
    case LS_N_G:           on = has_g; v = 1.0; break;
    case LS_MCD:           // _LOGDB_CONST * r.s_mcd / r.n_frames
      on = has_dist && (kind == LEDGER_ACOUSTIC || kind == LEDGER_VC);
      if (on) { const double p = logdb_const * dist[0]; v = p / dist[6]; }
      break;
    case LS_BAP_MCD:       // _LOGDB_CONST * r.s_bap / r.n_frames / 10.0
      on = has_dist && kind == LEDGER_ACOUSTIC;
      if (on) { const double p = logdb_const * dist[1]; const double q = p / dist[6]; v = q / 10.0; }
      break;
    case LS_F0_RMSE:       // sqrt(r.s_f0 / r.n_voiced), NaN without a frame voiced in both
      on = has_dist && kind == LEDGER_ACOUSTIC;
      if (on) { const double nv = dist[3]; v = nv > 0.0 ? sqrt(dist[2] / nv) : __builtin_nan(""); }
      break;
    case LS_VUV_ERR:       // r.n_vuv_err / r.n_frames
      on = has_dist && kind == LEDGER_ACOUSTIC;
      if (on) v = dist[4] / dist[6];
      break;
    case LS_DUR_RMSE:      // sqrt(r.s_mse / (r.n_frames * Ds))
      on = has_dist && kind == LEDGER_DURATION;
      if (on) { const double d = dist[6] * (double)Ds; v = sqrt(dist[5] / d); }
      break;
    default: break;
  }
  if (on) ledger[slot] = ledger[slot] + v;
}
