// libgantts_hip.so -- MLPG: the band cache and window registration, the banded forward / transpose launches, variance-weighted solves, gt_op_mlpg*
#include "engine_internal.hip.h"
#include "mlpg_kernels.hip.h"
#include "mlpg_band_kernels.hip.h"
#include "mlpg_var_kernels.hip.h"
#include <atomic>
#include <stddef.h>

using namespace gt;
// ------------------------------------------------------------------------------------------
// MLPG band cache
// ------------------------------------------------------------------------------------------
// first sight of (GT_MLPG_R_FROM_WINDOWS, T): Cholesky factor and selected inverse of W^T W in one workgroup, then the taps at the candidate
// half-width K and their per-offset maxima -> m.tmp [2 K + 1] floats and the pivot flag behind them.  No O(T^2) memory, no host work.
static int build_taps_from_windows(gt_engine* e, int T, int K, hipStream_t s) {
  MlpgCache& m = e->mlpg;
  const MlpgWindows& win = m.win;
  if (T > (1 << 20)) return fail(GT_ERR_INVALID, "MLPG band from windows: T = %d is beyond 2^20 frames", T);
  int hb = 0, reach = 0;
  for (int w = 0; w < win.n; ++w) { hb = std::max(hb, win.l[w] + win.u[w]); reach = std::max(reach, std::max(win.l[w], win.u[w])); }
  const int KS = std::min(std::max(K + reach, hb), T - 1);
  const int nk = 2 * K + 1;
  const size_t n_fac = (size_t)T * (hb + 1), n_inv = (size_t)T * (KS + 1);
  CHK(m.tmp.ensure((size_t)(nk + 1) * sizeof(float)));
  CHK(m.fac.ensure((n_fac + n_inv) * sizeof(double)));
  CHK(m.wide.ensure((size_t)T * win.n * nk * sizeof(float)));
  double* Lb = m.fac.as<double>();
  double* Sb = Lb + n_fac;
  int* flag = (int*)(m.tmp.as<float>() + nk);
  hipLaunchKernelGGL(mlpg_build_inverse_kernel, dim3(1), dim3(MLPG_BUILD_THREADS), 0, s, win, T, hb, KS, Lb, Sb, flag);
  LAUNCH_CHECK();
  hipLaunchKernelGGL(mlpg_build_taps_kernel, dim3(cdiv((long)T * win.n * nk, 256)), dim3(256), 0, s, win, T, K, KS, Sb, flag, m.wide.as<float>());
  LAUNCH_CHECK();
  hipLaunchKernelGGL(mlpg_build_offset_max_kernel, dim3(nk), dim3(256), 0, s, m.wide.as<float>(), T, win.n, K, m.tmp.as<float>());
  LAUNCH_CHECK();
  return GT_OK;
}
int ensure_band(gt_engine* e, const float* R, int T, hipStream_t s, const MlpgBand** out) {
  MlpgCache& m = e->mlpg;
  *out = nullptr;
  ++m.tick;
  for (auto& b : m.entries)
    if (b->R == R && b->T == T) { b->last_use = m.tick; *out = b.get(); return GT_OK; }
  const int nW = e->cfg.num_windows;
  const bool built = R == GT_MLPG_R_FROM_WINDOWS;      // never dereferenced
  if (built && !m.has_win) return fail(GT_ERR_INVALID, "GT_MLPG_R_FROM_WINDOWS without a window set: call gt_set_mlpg_windows first");
  // first sight of this (R, T): per-offset maxima -> host, pick the smallest half-width whose outside is negligible.  A dense R shows
  // every offset; a built one the offsets up to MLPG_BUILD_K, one beyond the widest half-width accepted below
  const int K = built ? std::min(MLPG_BUILD_K, T - 1) : T - 1;
  if (built) {
    CHK(build_taps_from_windows(e, T, K, s));
  } else {
    CHK(m.tmp.ensure((size_t)(2 * K + 2) * sizeof(float)));
    hipLaunchKernelGGL(mlpg_offset_max_kernel, dim3(2 * T - 1), dim3(256), 0, s, R, T, nW, m.tmp.as<float>());
    LAUNCH_CHECK();
  }
  std::vector<float> off(2 * K + 2);      // the last word: the pivot flag of a build
  HIPCHK(hipMemcpyAsync(off.data(), m.tmp.p, (size_t)(2 * K + 1 + (built ? 1 : 0)) * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (built) {
    int flag;
    memcpy(&flag, &off[2 * K + 1], sizeof(flag));
    if (flag) return fail(GT_ERR_INVALID, "window set does not determine the static features (W^T W is not positive definite at T=%d)", T);
  }
  off.resize(2 * K + 1);
  float peak = 0.f;
  bool has_nan = false;
  for (float v : off) { has_nan |= v != v; peak = fmaxf(peak, v); }      // fmaxf drops a NaN: counted apart
  if (has_nan || !(peak > 0.f) || !isfinite(peak)) return fail(GT_ERR_INVALID, "MLPG matrix R is empty or not finite");
  int kb = 0;
  for (int o = -K; o <= K; ++o)
    if (off[o + K] > 1e-9f * peak) kb = std::max(kb, abs(o));
  if (kb > 63 || (kb > 48 && kb > T / 4))
    return fail(GT_ERR_INVALID, "MLPG matrix R is not banded (half-width %d of T=%d): only window sets whose "
                "R = (W^T W)^-1 W^T decays (hparams.py:22-26) are supported", kb, T);
  MlpgBand* b = nullptr;
  if (m.entries.size() >= MlpgCache::MAX_ENTRIES) {      // recycle the least recently used entry, the stashed generator pass's band apart
    const MlpgBand* held = e->pass.live() ? e->pass.band() : nullptr;
    for (auto& c : m.entries) if (c.get() != held && (!b || c->last_use < b->last_use)) b = c.get();
    HIPCHK(hipStreamSynchronize(s));                      // its band may still be read by queued kernels
  } else {
    m.entries.emplace_back(new MlpgBand());
    b = m.entries.back().get();
  }
  const int nb = 2 * kb + 1;
  b->R = nullptr;
  CHK(b->band.ensure((size_t)T * nW * nb * sizeof(float)));
  if (built) hipLaunchKernelGGL(mlpg_build_band_kernel, dim3(cdiv((long)T * nW * nb, 256)), dim3(256), 0, s, m.wide.as<float>(), T, nW, K, kb, b->band.as<float>());
  else hipLaunchKernelGGL(mlpg_extract_band_kernel, dim3(cdiv((long)T * nW * nb, 256)), dim3(256), 0, s, R, T, nW, kb, b->band.as<float>());
  LAUNCH_CHECK();
  b->R = R; b->T = T; b->kb = kb; b->last_use = m.tick;
  *out = b;
  return GT_OK;
}
extern "C" int gt_invalidate_mlpg_cache(gt_engine* e) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  HIPCHK(hipDeviceSynchronize());
  for (auto& b : e->mlpg.entries) on_band_freed(e, b.get());
  e->mlpg.clear();
  return GT_OK;
}
extern "C" int gt_set_mlpg_windows(gt_engine* e, int n, const int32_t* l, const int32_t* u, const double* coef_concat) {
  if (!e) return fail(GT_ERR_INVALID, "null engine");
  if (n != e->cfg.num_windows) return fail(GT_ERR_INVALID, "gt_set_mlpg_windows: %d windows, the engine was created with num_windows = %d", n, e->cfg.num_windows);
  if (!l || !u || !coef_concat) return fail(GT_ERR_INVALID, "gt_set_mlpg_windows: null argument");
  MlpgWindows win;
  memset(&win, 0, sizeof(win));
  win.n = n;
  const double* c = coef_concat;
  for (int w = 0; w < n; ++w) {
    if (l[w] < 0 || u[w] < 0 || (long)l[w] + u[w] > MLPG_WIN_SPAN)
      return fail(GT_ERR_INVALID, "gt_set_mlpg_windows: window %d reaches (%d, %d): l, u >= 0 and l + u <= %d", w, l[w], u[w], MLPG_WIN_SPAN);
    win.l[w] = l[w]; win.u[w] = u[w];
    for (int k = 0; k <= l[w] + u[w]; ++k, ++c) {
      if (!isfinite(*c)) return fail(GT_ERR_INVALID, "gt_set_mlpg_windows: coefficient %d of window %d is not finite", k, w);
      win.coef[w][k] = *c == 0.0 ? 0.0 : *c;      // -0.0 and 0.0 are the same set
    }
  }
  MlpgCache& m = e->mlpg;
  if (m.has_win && memcmp(&m.win, &win, sizeof(win)) == 0) return GT_OK;
  // another set: the built entries go (a dense R's stay), with gt_invalidate_mlpg_cache's synchronisation -- queued kernels may read them
  HIPCHK(hipDeviceSynchronize());
  for (size_t i = 0; i < m.entries.size();) {
    if (m.entries[i]->R != GT_MLPG_R_FROM_WINDOWS) { ++i; continue; }
    on_band_freed(e, m.entries[i].get());
    m.entries.erase(m.entries.begin() + i);
  }
  memcpy(&m.win, &win, sizeof(win));      // padding included: the comparison above is a memcmp
  m.has_win = true;
  return GT_OK;
}

// ------------------------------------------------------------------------------------------
// variance-weighted MLPG (mlpg_var_kernels.hip.h): a batch of independent banded solves, one thread per (sequence, static column)
// ------------------------------------------------------------------------------------------
// gt_mlpg_var_path_counts: process-wide, one relaxed increment per launch on the host (no device work, no synchronisation)
static std::atomic<int64_t> g_mlpg_var_paths[GT_MLPG_VAR_PATH_SLOTS];
extern "C" int gt_mlpg_var_path_counts(int64_t* counts, int n) {
  for (int i = 0; i < GT_MLPG_VAR_PATH_SLOTS; ++i) {
    if (!counts) g_mlpg_var_paths[i].store(0, std::memory_order_relaxed);
    else if (i < n) counts[i] = g_mlpg_var_paths[i].load(std::memory_order_relaxed);
  }
  return GT_OK;
}
template <int HB> static MlpgVarTaps<HB> mlpg_var_taps(const MlpgWindows& win) {
  MlpgVarTaps<HB> t;
  memset(&t, 0, sizeof(t));
  t.n = win.n;
  for (int w = 0; w < win.n; ++w) {
    t.l[w] = win.l[w];
    for (int q = 0; q <= win.l[w] + win.u[w]; ++q) t.c[w][q] = win.coef[w][q];
  }
  return t;
}
// y [B*T][ldy], var [B*T][ldv] (ldv == 0: one row), ys [B*T][ldys]; scol, sstride device [Ds]; lengths: host, B entries in [1, T] (checked by
// the caller, like every pointer and pitch).  The batch goes in groups of whole sequences whose scratch 8 (hb + 2) T nseq Ds stays within
// max_ws_bytes (0: 64 MB); the stream is synchronised, because the refusal flag is read.
static int launch_mlpg_var(gt_engine* e, const float* y, int ldy, const float* var, int ldv, const int* scol, const int* sstride, int Ds, float* ys, int ldys,
                           const int64_t* lengths, int B, int T, int64_t max_ws_bytes, hipStream_t s) {
  const MlpgCache& m = e->mlpg;
  if (!m.has_win) return fail(GT_ERR_INVALID, "variance-weighted MLPG without a window set: call gt_set_mlpg_windows first");
  const MlpgWindows& win = m.win;
  int hb = 0;
  for (int w = 0; w < win.n; ++w) hb = std::max(hb, win.l[w] + win.u[w]);
  const size_t cap = max_ws_bytes > 0 ? (size_t)max_ws_bytes : (size_t)64 << 20;
  const size_t per_seq = sizeof(double) * (size_t)(hb + 2) * (size_t)T * (size_t)Ds;
  const int per_group = (int)std::min<size_t>((size_t)B, cap / per_seq);
  if (per_group < 1)
    return fail(GT_ERR_INVALID, "variance-weighted MLPG: one sequence of T=%d frames and %d static columns needs %zu bytes of scratch, the cap is %zu", T, Ds, per_seq, cap);
  const size_t off_len = 256, off_ws = off_len + (((size_t)B * sizeof(int) + 255) & ~(size_t)255);
  Scratch& q = e->mlpg_var_ws;
  CHK(q.ensure(off_ws + per_seq * (size_t)per_group));
  int* flag = (int*)q.p;
  int* d_len = (int*)((char*)q.p + off_len);
  std::vector<int> h_len(B);
  for (int b = 0; b < B; ++b) h_len[b] = lengths ? (int)lengths[b] : T;
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));
  HIPCHK(hipMemcpyAsync(d_len, h_len.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
  hipError_t err = hipSuccess;
  for (int b0 = 0; b0 < B && err == hipSuccess; b0 += per_group) {
    MlpgVarArgs a;
    a.nseq = std::min(per_group, B - b0); a.T = T; a.Ds = Ds; a.ldy = ldy; a.ldv = ldv; a.ldys = ldys;
    a.y = y + (size_t)b0 * T * ldy; a.var = var + (size_t)b0 * T * ldv; a.ys = ys + (size_t)b0 * T * ldys;
    a.scol = scol; a.sstride = sstride; a.len = d_len + b0;
    a.ws = (double*)((char*)q.p + off_ws); a.flag = flag;
    const dim3 grid(cdiv((long)a.nseq * Ds, MLPG_VAR_THREADS)), block(MLPG_VAR_THREADS);
    int slot;
    if (hb == 1) { slot = 0; hipLaunchKernelGGL(mlpg_var_solve_kernel<1>, grid, block, 0, s, a, mlpg_var_taps<1>(win)); }
    else if (hb == 2) { slot = 1; hipLaunchKernelGGL(mlpg_var_solve_kernel<2>, grid, block, 0, s, a, mlpg_var_taps<2>(win)); }
    else { slot = 2; hipLaunchKernelGGL(mlpg_var_generic_kernel, grid, block, 0, s, a, win, hb); }
    err = hipGetLastError();
    if (err == hipSuccess) g_mlpg_var_paths[slot].fetch_add(1, std::memory_order_relaxed);
  }
  int h_flag = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&h_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s);
  const hipError_t err_sync = hipStreamSynchronize(s);      // also keeps h_len alive until its copy is done
  if (err == hipSuccess) err = err_sync;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "variance-weighted MLPG: %s", hipGetErrorString(err));
  if (h_flag & MLPG_VAR_BAD_VARIANCE) return fail(GT_ERR_INVALID, "variance-weighted MLPG: variances must be finite and positive");
  if (h_flag) return fail(GT_ERR_INVALID, "variance-weighted MLPG: variances must be finite and positive (a pivot of W^T diag(1/var) W is not: the windows do not determine the static features)");
  return GT_OK;
}

// output frames per workgroup of the MLPG kernels: 32; 16-frame tiles (gt_set_tuning("mlpg_tt", 16)): twice the workgroups for
// batches whose 32-frame tiles leave CUs empty (a rank's share of a strong-scaling run: B * ceil(T / 32) = 64 workgroups at 4 sequences of
// 512 frames), at (16 + 2 kb) / 16 staged rows per output frame.  (64-frame tiles -- half the halo re-reads, one workgroup per CU instead of two --
// measured no gain in round 4, 1.404 / 1.398 vs 1.393 / 1.398 ms, and left the library in round 6.)
static int mlpg_tile_frames() { return gt_tuning().mlpg_tt == 16 ? 16 : 32; }
// ensure_band accepts half-widths up to 63, and both kernels stage (tile + 2 kb) rows: a slowly decaying R asks for more dynamic LDS than a
// workgroup can have (nW = 4, kb = 39: 156 160 bytes forward, 177 760 transposed, of 160 KiB).  Checked here, per launcher and before anything
// is launched or any function attribute is raised, so that a window set whose forward fits still serves inference.  The limit is the
// device's own figure, read once per device.
static int mlpg_lds_fits(const char* which, int kb, int nW, int tt, size_t lds) {
  static std::mutex mu;
  static std::map<int, size_t> limits;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  size_t limit;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto it = limits.find(dev);
    if (it == limits.end()) {
      int v = 0;
      HIPCHK(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
      it = limits.emplace(dev, (size_t)v).first;
    }
    limit = it->second;
  }
  if (lds > limit)
    return fail(GT_ERR_INVALID, "MLPG %s: half-width %d with %d windows needs %zu bytes of LDS per %d-frame tile, the device allows %zu: "
                "this window set's R = (W^T W)^-1 W^T decays too slowly for the banded kernels", which, kb, nW, lds, tt, limit);
  return GT_OK;
}
int mlpg_forward(gt_engine* e, const float* y, int ldy, const int* scol, const int* sstride, int Ds,
                 float* ys, int ldys, int B, int T, const MlpgBand& band, hipStream_t s) {
  const int nW = e->cfg.num_windows, kb = band.kb;
  auto lds_of = [&](int tt) { return ((size_t)(tt + 2 * kb) * nW * MLPG_CC + (size_t)tt * nW * (2 * kb + 1 + 2 * MLPG_PAD)) * sizeof(float); };
  const int tt = mlpg_tile_frames();
  const size_t lds = lds_of(tt);
  CHK(mlpg_lds_fits("forward", kb, nW, tt, lds));
  dim3 grid(B * cdiv(T, tt), cdiv(Ds, MLPG_CC));
  const int fpl = gt_tuning().mlpg_fpl;   // frames per lane of the compute phase: 2 measured best (round 4: 4: 24.7 us, 2: 21.8, 1: 26.6; round 5, unrolled tap loops: forward 18.5 / 17.2 / 18.3, backward 24.9 / 19.5 / 20.6)
#define GT_MLPG_FWD(F, TTV) { CHK(ensure_dyn_lds((const void*)mlpg_forward_kernel<F, TTV>, lds)); \
    hipLaunchKernelGGL((mlpg_forward_kernel<F, TTV>), grid, dim3(MLPG_THREADS), lds, s, y, ldy, band.band.as<float>(), kb, nW, scol, sstride, Ds, ys, ldys, B, T); }
  if (tt == 16) GT_MLPG_FWD(2, 16)
  else { if (fpl == 1) GT_MLPG_FWD(1, 32) else if (fpl == 2) GT_MLPG_FWD(2, 32) else GT_MLPG_FWD(4, 32) }
#undef GT_MLPG_FWD
  LAUNCH_CHECK();
  return GT_OK;
}
int mlpg_backward(gt_engine* e, const float* gs, int ldgs, const int* scol, const int* sstride, int Ds,
                  float* gy, int ldgy, int B, int T, float mse_w, const float* yhat, const float* ytgt, int ldt,
                  const float* mask, const MlpgBand& band, hipStream_t s) {
  const int nW = e->cfg.num_windows, kb = band.kb;
  auto lds_of = [&](int tt) { return ((size_t)(tt + 2 * kb) * MLPG_CC + (size_t)(tt + 2 * kb) * nW * (2 * kb + 1 + 2 * MLPG_PAD)) * sizeof(float); };
  const int tt = mlpg_tile_frames();
  const size_t lds = lds_of(tt);
  CHK(mlpg_lds_fits("transpose", kb, nW, tt, lds));
  dim3 grid(B * cdiv(T, tt), cdiv(Ds, MLPG_CC));
  const int fpl = gt_tuning().mlpg_fpl;
#define GT_MLPG_BWD(F, TTV) { CHK(ensure_dyn_lds((const void*)mlpg_backward_kernel<F, TTV>, lds)); \
    hipLaunchKernelGGL((mlpg_backward_kernel<F, TTV>), grid, dim3(MLPG_THREADS), lds, s, gs, ldgs, band.band.as<float>(), kb, nW, scol, sstride, Ds, \
                       gy, ldgy, B, T, mse_w, yhat, ytgt, ldt, mask, e->sc()); }
  if (tt == 16) GT_MLPG_BWD(2, 16)
  else { if (fpl == 1) GT_MLPG_BWD(1, 32) else if (fpl == 2) GT_MLPG_BWD(2, 32) else GT_MLPG_BWD(4, 32) }
#undef GT_MLPG_BWD
  LAUNCH_CHECK();
  return GT_OK;
}

extern "C" int gt_op_mlpg_forward(gt_engine* e, const float* y, const float* R, int B, int T, float* y_static, void* stream) {
  CHK(check_common(e, B, T));
  if (!y || !R || !y_static) return fail(GT_ERR_INVALID, "null tensor");
  hipStream_t s = (hipStream_t)stream;
  const MlpgBand* band;
  CHK(ensure_band(e, R, T, s, &band));
  return mlpg_forward(e, y, e->Dout_cfg, e->d_scol.as<int>(), e->d_sstride.as<int>(), e->Ds, y_static, e->Ds, B, T, *band, s);
}
extern "C" int gt_op_mlpg_backward(gt_engine* e, const float* g_static, const float* R, int B, int T, float* g_y, void* stream) {
  CHK(check_common(e, B, T));
  if (!g_static || !R || !g_y) return fail(GT_ERR_INVALID, "null tensor");
  hipStream_t s = (hipStream_t)stream;
  const MlpgBand* band;
  CHK(ensure_band(e, R, T, s, &band));
  return mlpg_backward(e, g_static, e->Ds, e->d_scol.as<int>(), e->d_sstride.as<int>(), e->Ds, g_y, e->Dout_cfg, B, T, 0.f, nullptr, nullptr, 0, nullptr, *band, s);
}

// The column maps a hook's launch indexes with -- the engine's own, or the case's, read back from the device -- hold no negative entry, and
// the last window's column of every static column, col + (nW - 1) stride (pass-through, stride 0: its own column only), lies within each
// pitch given; dyn_only: asked of the columns with a stride alone
struct MlpgPitch { const char* name; long ld; bool dyn_only; };
static int check_column_maps(gt_engine* e, const char* who, const void* scol, const void* sstride, int Ds, const MlpgPitch* pitch, int n_pitch, hipStream_t s) {
  std::vector<int> h_scol = e->h_scol, h_sstride = e->h_sstride;
  if (scol) {
    h_scol.resize(Ds); h_sstride.resize(Ds);
    HIPCHK(hipMemcpyAsync(h_scol.data(), scol, (size_t)Ds * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(h_sstride.data(), sstride, (size_t)Ds * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  const int nW = e->cfg.num_windows;
  for (int i = 0; i < Ds; ++i) {
    const long col = h_scol[i], st = h_sstride[i];
    if (col < 0 || st < 0) return fail(GT_ERR_INVALID, "%s: negative entry in the column maps at %d", who, i);
    const long last = col + (long)(nW - 1) * st;
    for (int k = 0; k < n_pitch; ++k)
      if ((st || !pitch[k].dyn_only) && last >= pitch[k].ld)
        return fail(GT_ERR_INVALID, "%s: static column %d reaches column %ld, %s is %ld", who, i, last, pitch[k].name, pitch[k].ld);
  }
  return GT_OK;
}

// One MLPG launch with the step's freedom in the arguments (column maps, pitches, the fused masked-MSE gradient) through ensure_band and
// mlpg_forward / mlpg_backward: parity hook of tests/test_gpu_mlpg.py.  Everything a kernel would index with is checked first.
static_assert(offsetof(gt_mlpg_case, e) == 40 && offsetof(gt_mlpg_case, kb) == 128 && sizeof(gt_mlpg_case) == 136, "layout bound by gantts_amd/_lib.py");
extern "C" int gt_op_mlpg(const gt_mlpg_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  gt_engine* e = c->e;
  CHK(check_common(e, c->B, c->T));
  const bool bwd = c->backward != 0, own = !c->scol && !c->sstride, mse = bwd && c->mse_w != 0.f;
  if (c->backward != 0 && c->backward != 1) return fail(GT_ERR_INVALID, "MLPG hook: backward is 0 or 1");
  if (!c->R) return fail(GT_ERR_INVALID, "MLPG hook: null R");
  if (!own && (!c->scol || !c->sstride)) return fail(GT_ERR_INVALID, "MLPG hook: scol and sstride come together");
  if (own && c->Ds != 0 && c->Ds != e->Ds) return fail(GT_ERR_INVALID, "MLPG hook: Ds = %d with the engine's maps (%d)", c->Ds, e->Ds);
  const int Ds = own ? e->Ds : c->Ds;
  if (Ds < 1 || Ds > (1 << 20)) return fail(GT_ERR_INVALID, "MLPG hook: Ds = %d", Ds);
  if (bwd ? (!c->gs || !c->gy) : (!c->y || !c->ys)) return fail(GT_ERR_INVALID, "MLPG hook: null tensor");
  if (mse && (!c->yhat || !c->ytgt || !c->mask)) return fail(GT_ERR_INVALID, "MLPG hook: the masked-MSE gradient needs yhat, ytgt and mask");
  const bool built = c->R == GT_MLPG_R_FROM_WINDOWS;      // the sentinel is no address: ensure_band never dereferences it
  for (const void* q : {built ? nullptr : (const void*)c->R, (const void*)c->scol, (const void*)c->sstride, (const void*)c->y, (const void*)c->ys, (const void*)c->gs,
                        (const void*)c->gy, (const void*)c->yhat, (const void*)c->ytgt, (const void*)c->mask})
    if (((uintptr_t)q) & 3) return fail(GT_ERR_INVALID, "MLPG hook: misaligned operand");
  if (bwd ? c->ldgs < Ds : c->ldys < Ds) return fail(GT_ERR_INVALID, "MLPG hook: pitch of the static side below Ds = %d", Ds);
  hipStream_t s = (hipStream_t)stream;
  const MlpgPitch pitch[2] = {{"the pitch", bwd ? c->ldgy : c->ldy, false}, {"ldt", c->ldt, false}};
  CHK(check_column_maps(e, "MLPG hook", c->scol, c->sstride, Ds, pitch, mse ? 2 : 1, s));
  const MlpgBand* band;
  CHK(ensure_band(e, c->R, c->T, s, &band));
  if (c->kb) *c->kb = band->kb;
  const int* scol = own ? e->d_scol.as<int>() : (const int*)c->scol;
  const int* sstride = own ? e->d_sstride.as<int>() : (const int*)c->sstride;
  int r;
  if (!bwd) {
    r = mlpg_forward(e, c->y, c->ldy, scol, sstride, Ds, c->ys, c->ldys, c->B, c->T, *band, s);
  } else {
    if (mse) {      // sum(mask) and its reciprocal, as LossNormaliser::file puts them there, behind the step's memo of them
      launch_mask_sum(c->mask, (long)c->B * c->T, -1.f, nullptr, e->sc(), s);
      LAUNCH_CHECK();
      e->norm.overwritten();
    }
    r = mlpg_backward(e, c->gs, c->ldgs, scol, sstride, Ds, c->gy, c->ldgy, c->B, c->T, mse ? c->mse_w : 0.f, mse ? c->yhat : nullptr,
                      mse ? c->ytgt : nullptr, mse ? c->ldt : 0, mse ? c->mask : nullptr, *band, s);
  }
  const hipError_t err = hipStreamSynchronize(s);
  if (r) return r;
  if (err != hipSuccess) return fail(GT_ERR_HIP, "mlpg: %s", hipGetErrorString(err));
  return GT_OK;
}

extern "C" int gt_op_mlpg_band(gt_engine* e, const float* R, int T, float* band_host, int64_t capacity, int32_t* kb, void* stream) {
  CHK(check_common(e, 1, T));
  if (!R) return fail(GT_ERR_INVALID, "MLPG band hook: null R");
  if (R != GT_MLPG_R_FROM_WINDOWS && (((uintptr_t)R) & 3)) return fail(GT_ERR_INVALID, "MLPG band hook: misaligned R");
  hipStream_t s = (hipStream_t)stream;
  const MlpgBand* b;
  CHK(ensure_band(e, R, T, s, &b));
  if (kb) *kb = b->kb;
  const int64_t need = (int64_t)T * e->cfg.num_windows * (2 * b->kb + 1);
  if (!band_host || capacity < need) return fail(GT_ERR_INVALID, "MLPG band hook: the band has %ld floats, band_host holds %ld", (long)need, (long)capacity);
  HIPCHK(hipMemcpyAsync(band_host, b->band.p, (size_t)need * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return GT_OK;
}

// nnmnkwii.paramgen.mlpg for a batch (launch_mlpg_var above).  Everything a kernel would index with is checked first.
static_assert(offsetof(gt_mlpg_var_case, B) == 8 && offsetof(gt_mlpg_var_case, scol) == 32 && offsetof(gt_mlpg_var_case, max_ws_bytes) == 80 &&
              sizeof(gt_mlpg_var_case) == 88, "layout bound by gantts_amd/_lib.py");
extern "C" int gt_op_mlpg_var(const gt_mlpg_var_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "null case");
  gt_engine* e = c->e;
  CHK(check_common(e, c->B, c->T));
  if (!e->mlpg.has_win) return fail(GT_ERR_INVALID, "variance-weighted MLPG without a window set: call gt_set_mlpg_windows first");
  const bool own = !c->scol && !c->sstride;
  if (!own && (!c->scol || !c->sstride)) return fail(GT_ERR_INVALID, "variance-weighted MLPG: scol and sstride come together");
  if (own && c->Ds != 0 && c->Ds != e->Ds) return fail(GT_ERR_INVALID, "variance-weighted MLPG: Ds = %d with the engine's maps (%d)", c->Ds, e->Ds);
  const int Ds = own ? e->Ds : c->Ds;
  if (Ds < 1 || Ds > (1 << 20)) return fail(GT_ERR_INVALID, "variance-weighted MLPG: Ds = %d", Ds);
  if (!c->y || !c->var || !c->ys) return fail(GT_ERR_INVALID, "variance-weighted MLPG: null tensor");
  for (const void* q : {(const void*)c->scol, (const void*)c->sstride, (const void*)c->y, (const void*)c->var, (const void*)c->ys})
    if (((uintptr_t)q) & 3) return fail(GT_ERR_INVALID, "variance-weighted MLPG: misaligned operand");
  if (c->max_ws_bytes < 0) return fail(GT_ERR_INVALID, "variance-weighted MLPG: negative max_ws_bytes");
  if (c->ldys < Ds) return fail(GT_ERR_INVALID, "variance-weighted MLPG: pitch of the static side below Ds = %d", Ds);
  if (c->ldy < 1 || c->ldv < 0) return fail(GT_ERR_INVALID, "variance-weighted MLPG: ldy = %d, ldv = %d", c->ldy, c->ldv);
  if (c->lengths)
    for (int b = 0; b < c->B; ++b)
      if (c->lengths[b] < 1 || c->lengths[b] > c->T) return fail(GT_ERR_INVALID, "variance-weighted MLPG: length %lld outside [1, T=%d]", (long long)c->lengths[b], c->T);
  hipStream_t s = (hipStream_t)stream;
  const MlpgPitch pitch[2] = {{"ldy", c->ldy, false}, {"ldv", c->ldv, true}};
  CHK(check_column_maps(e, "variance-weighted MLPG", c->scol, c->sstride, Ds, pitch, c->ldv ? 2 : 1, s));
  return launch_mlpg_var(e, c->y, c->ldy, c->var, c->ldv, own ? e->d_scol.as<int>() : (const int*)c->scol, own ? e->d_sstride.as<int>() : (const int*)c->sstride, Ds,
                         c->ys, c->ldys, c->lengths, c->B, c->T, c->max_ws_bytes, s);
}
