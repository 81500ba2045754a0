// libgantts_hip.so -- internal header shared by the engine's translation units (eng_*.hip).
//
// The engine keeps the reference's step semantics (train.py:245-320) while restructuring the
// work for the hardware:
//   * D(real) and D(fake) of the D step run as ONE 2N-row pass (same weights), so the frame x
//     weight GEMMs see 32768 rows at the headline config;
//   * G is back-propagated ONCE per step: dloss_d/dy_hat_static (old D weights, the reference's
//     un-detached "leak", train.py:265,274) is stashed and summed with dloss_g/dy_hat_static at
//     y_hat_static before MLPG^T and the G backward (backward is linear in the upstream gradient);
//   * the G-step D pass computes no weight gradients (the reference's are discarded by the next
//     zero_grad, train.py:538-539);
//   * every reduction is two-stage with a fixed order => run-to-run bit-reproducible.
//
// Translation units: eng_core (life cycle, binding, options, dropout sites, faults), eng_gemm_f32 / eng_gemm_b16 (dispatch
// of the two product families; eng_gemm_b16 also holds the stacks' bf16 vocabulary: LinShadow::ensure / shadow_cast, b16_forward / b16_backward_data),
// eng_step (the G+D step, its ResultsChannel, its plans GPlan / TvPlan -- the latter: how LossNormaliser's count reaches the D head --, the MLP stacks and the output layer of every stack: out_layer_forward / out_layer_backward), eng_mlpg
// (band cache, MLPG launches), eng_dstack (fused discriminator stack), eng_spectral_norm (spectral normalisation of the MLP discriminator), eng_grad_penalty (its R1 / WGAN-GP gradient penalties), eng_lstm / eng_sru (recurrent stacks of either role), eng_comm / eng_ipc
// (data-parallel communicator), eng_ops (stand-alone operators).  Kernels live in the *.hip.h headers; the non-template ones have internal linkage
// (GT_KERNEL) so that several units may include them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/gantts_hip.h"
#pragma GCC visibility pop
#include "frame_kernels.hip.h"
#include "frame_args.hip.h"
#include "gemm_f32.hip.h"
#include "gemm_bf16s.hip.h"
#include "sru_args.hip.h"

using namespace gt;

// ------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------
int fail(int code, const char* fmt, ...);
#define HIPCHK(expr)                                                                         \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess)                                                                    \
      return fail(GT_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)
#define CHK(expr)            \
  do {                       \
    int _r = (expr);         \
    if (_r != GT_OK) return _r; \
  } while (0)
#define LAUNCH_CHECK() HIPCHK(hipGetLastError())

static inline bool env_flag(const char* name, bool dflt) { const char* v = getenv(name); return v && v[0] ? v[0] != '0' : dflt; }
static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline int pad8(long n) { return (int)((n + 7) & ~7L); }

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE function attribute: remembered per (kernel, device)
int ensure_dyn_lds(const void* kernel, size_t bytes);
int gemm_cu_count();

// ------------------------------------------------------------------------------------------
// Dispatch knobs of the product families and frame kernels: ONE process-wide table, read once from the environment when the
// library is first used and settable afterwards by name (gt_set_tuning; tools/ harnesses and A/B runs).  Every default is the
// measured best; none selects different arithmetic.  What changes a STEP's schedule or a network's path is
// per-engine state instead (gt_engine::opt_*, gt_set_option): two engines of one process may differ.
// ------------------------------------------------------------------------------------------
struct GtTuning {
  int gemm_pair = 1;          // GT_GEMM_PAIR      backward-data + weight gradient of a layer in one launch
  int pair_order = 1;         // GT_PAIR_ORDER     pair launch: weight-gradient workgroups first
  int gemm_tiles_big = 0;     // GT_GEMM_TILES=big residency model (128-wide tiles) for every float32 launch
  int gemm_unaligned = 1;     // GT_GEMM_UNALIGNED 16-byte loads of k-contiguous operands at 4-byte aligned addresses
  int tn_wgs = 512;           // GT_TN_WGS         workgroups of a weight-gradient launch
  int split_fused = 1;        // GT_SPLIT_FUSED    split first layer's forward as one two-segment launch (0: x product + K = 58 pass)
  int tn_split_wgs = 1024;    // GT_TN_SPLIT_WGS   ... of the split first layer's two-block launch
  int b16_tiles = 0;          // GT_B16_TILES      bf16-storage products: force 64 / 128 / 256 tiles (0 = by shape)
  int b16_wg_tile = 0;        // GT_B16_WG_TILE    ... their weight gradients
  int b16_dma = 1;            // GT_B16_DMA        LDS-DMA operand stages
  int mlpg_fpl = 2;           // GT_MLPG_FPL       frames per lane of the MLPG compute phase
  int head_vec = 0;           // GT_HEAD_VEC       discriminator head: 16-byte accesses (lane <-> four consecutive hidden units); measured -3 us
                              //                   per step, NOT the default: it sums the row's dot product in another order, and one oracle-only
                              //                   at-size case (a cold-Adagrad update, lr * g / |g|) then lands 1.2x outside its 1e-4
  int mlpg_tt = 0;            // GT_MLPG_TT        output frames per MLPG workgroup (0 = by shape, 16, 32)
  int leak_rider = 1;         // GT_LEAK_RIDER     D step: the kept dloss_d / dy_hat_static product rides in the split first layer's weight-gradient launch
  int sru_cs_waves = 0;       // GT_SRU_CS_WAVES   waves per 64 columns of the cooperative SRU scans: 0 = by shape (8 up to two 64-column workgroups per CU, i.e. B x ncols / 64 <= 2 CUs, else 4), 4, 8
  int sru_coop = 1;           // GT_SRU_COOP       1: cooperative block scans (sru_cs_kernels.hip.h); 0: one-wave kernels (sru_kernels.hip.h: the sequential reference)
  int lstm_bt = 0;            // GT_LSTM_BT        sequences per batch tile of the persistent LSTM kernels: 0 = by shape, 8, 16 (still subject to co-residency)
};
GtTuning& gt_tuning();

// optional per-launch timing of the product families (HIP events on the launch stream); bench.py's live roofline figure
struct GemmProfiler {
  bool on = false;
  int only_kind = -1;       // >= 0: only launches of this kind are instrumented (5 = the pair launches): gt_profile_enable(2 + kind)
  bool wants(int kind) const { return on && (only_kind < 0 || only_kind == kind); }
  struct Rec { int kind, bn, am; double flops, bytes; hipEvent_t e0, e1; };   // am: GemmAmode of a float32 kernel (-1: run-time flavour)
  double last_bytes[GT_PROFILE_SLOTS] = {};   // algorithmic bytes per slot of the last gt_profile_read
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
  }
};
extern GemmProfiler g_prof;

// Owning types: every device block, pinned host block and event of the engine belongs to one of these and goes back in its destructor.
// They alone call hipFree / hipHostMalloc / hipHostFree / hipEventCreate* / hipEventDestroy (besides the interprocess arena of eng_ipc.hip
// and g_prof's pool above) and they keep gt_live_resources' counters.  A destructor does not synchronise: whoever drops one of them
// under work that may still be queued synchronises first (gt_engine_destroy, resize_owned, the MLPG cache).  All are move-only or fixed.
enum { LIVE_DEV_BLOCKS = 0, LIVE_DEV_BYTES = 1, LIVE_PINNED = 2, LIVE_EVENTS = 3 };
void live_count(int slot, int64_t delta);      // eng_core.hip: relaxed, process-wide

struct Scratch {  // growable device buffer
  void* p = nullptr;
  size_t bytes = 0;
  Scratch() = default;      Scratch(Scratch&& o) noexcept : p(o.p), bytes(o.bytes), counted(o.counted) { o.p = nullptr; o.bytes = 0; }
  Scratch(const Scratch&) = delete;      Scratch& operator=(const Scratch&) = delete;      // a copy would be freed twice
  ~Scratch() { release(); }
  int ensure(size_t need) {
    if (need <= bytes) return GT_OK;
    if (p) { HIPCHK(hipDeviceSynchronize()); release(); }
    const size_t cap = need + need / 8;
    HIPCHK(hipMalloc(&p, cap));
    bytes = cap;
    if (counted) { live_count(LIVE_DEV_BLOCKS, 1); live_count(LIVE_DEV_BYTES, (int64_t)cap); }
    return GT_OK;
  }
  void release() {      // the block goes now (the caller has synchronised); today only ensure() and the destructor call it
    if (p) { (void)hipFree(p); if (counted) { live_count(LIVE_DEV_BLOCKS, -1); live_count(LIVE_DEV_BYTES, -(int64_t)bytes); } }
    p = nullptr; bytes = 0;
  }
  template <typename T> T* as() const { return (T*)p; }
 protected:
  bool counted = true;
};
// A hook's `static thread_local` buffer: its destructor frees NOTHING, because it runs at thread or process teardown, where a hipFree
// may come after the HIP runtime has gone.  How: the derived destructor runs first and empties the object, so ~Scratch finds no block.
// Not counted by gt_live_resources (`counted` is cleared before the first ensure()).
struct HookScratch : Scratch { HookScratch() { counted = false; }      ~HookScratch() { p = nullptr; bytes = 0; } };
template <typename T> struct Pinned {  // pinned host block
  T* p = nullptr;
  Pinned() = default;      Pinned(const Pinned&) = delete;      Pinned& operator=(const Pinned&) = delete;
  ~Pinned() { release(); }
  int alloc(size_t n_bytes) { release(); HIPCHK(hipHostMalloc((void**)&p, n_bytes)); live_count(LIVE_PINNED, 1); return GT_OK; }      // in place of what it held
  void release() { if (p) { (void)hipHostFree(p); live_count(LIVE_PINNED, -1); p = nullptr; } }
  operator T*() const { return p; }
};
struct Event {  // HIP event, created by the first ensure() with the flags given there
  hipEvent_t ev = nullptr;
  Event() = default;      Event(Event&& o) noexcept : ev(o.ev) { o.ev = nullptr; }
  Event(const Event&) = delete;      Event& operator=(const Event&) = delete;
  ~Event() { if (ev) { (void)hipEventDestroy(ev); live_count(LIVE_EVENTS, -1); } }
  int ensure(unsigned flags) { if (!ev) { HIPCHK(hipEventCreateWithFlags(&ev, flags)); live_count(LIVE_EVENTS, 1); } return GT_OK; }
  operator hipEvent_t() const { return ev; }
};
// a per-layer vector of owning buffers takes another length: dropping elements frees their blocks, so the device is idle first
template <typename V> static inline int resize_owned(V& v, size_t n) { if (n < v.size()) HIPCHK(hipDeviceSynchronize());      v.resize(n); return GT_OK; }

// Deferred weight-gradient combines (eng_gemm_f32.hip: linear_backward_weight): the partial slabs of every layer go to their
// own piece of a pool and the combine is only RECORDED; slab_defer_flush() runs all recorded combines in one launch.
struct SlabDefer {
  Scratch pool;
  size_t used = 0;
  SlabJobs jobs;
  int blocks = 0;
  bool active = false;
  SlabDefer() { jobs.n = 0; jobs.pad_ = 0; }
  void reset(bool on) { jobs.n = 0; blocks = 0; used = 0; active = on; }      // nothing recorded; record (on) or combine in place
};

// ------------------------------------------------------------------------------------------
// engine state
// ------------------------------------------------------------------------------------------
struct Lin { float *W, *b, *dW, *db; int in, out; };
// a tensor kept as bf16 in both orientations: rm [rows][ld], tr [cols][ldt]   (gemm_bf16s.hip.h)
struct B16Img {
  Scratch rm, tr;
  int ld = 0; long ldt = 0;
  __bf16* r() { return rm.as<__bf16>(); }
  __bf16* t() { return tr.as<__bf16>(); }
  int ensure(long rows, int cols, bool want_t) {
    ld = pad8(cols); ldt = pad8(rows);
    CHK(rm.ensure((size_t)rows * ld * 2 + 64));
    if (want_t) CHK(tr.ensure((size_t)cols * ldt * 2 + 64));
    return GT_OK;
  }
};
// bf16 shadows of one nn.Linear weight (out, in): w [out][ldw] feeds the forward product, wt [in][ldwt] backward-data
struct LinShadow {
  Scratch w, wt; int ldw = 0, ldwt = 0;
  __bf16* r() const { return w.as<__bf16>(); }
  __bf16* t() const { return wt.as<__bf16>(); }
  int ensure(int out, int in) {
    ldw = pad8(in); ldwt = pad8(out);
    CHK(w.ensure((size_t)out * ldw * 2 + 64));
    CHK(wt.ensure((size_t)in * ldwt * 2 + 64));
    return GT_OK;
  }
};
static inline bool is_i2o(int arch) { return arch == GT_ARCH_IN2OUT || arch == GT_ARCH_IN2OUT_RNN; }
static inline bool has_lstm_body(int arch) { return arch == GT_ARCH_LSTM || arch == GT_ARCH_IN2OUT_RNN; }
struct LstmDirP { float *Wih, *Whh, *bih, *bhh, *dWih, *dWhh, *dbih, *dbhh; };
struct LstmLayerP { int in; LstmDirP d[2]; };
struct SruLayerP { int in, k; float *W, *b, *dW, *db; };

// NAdam's mu_product after `step` updates, kept so that the running float32 product is not redone from the bind every step
struct OptimScalarCache { bool valid = false; long step = 0; float mu_product = 1.f; };

struct Net {
  bool bound = false;
  gt_model_desc d;
  std::vector<Lin> hidden;
  Lin last, gate;
  std::vector<LstmLayerP> lstm;   // GT_ARCH_LSTM; `last` is hidden2out
  std::vector<SruLayerP> sru;     // GT_ARCH_SRU;  `last` is hidden2out
  bool training = true;
  bool grads_dirty = false;      // false after zero_grad: next backward overwrites instead of accumulating
  bool has_opt = false;
  gt_optim_desc_ex od;            // gt_bind_optimizer widens its descriptor to this one
  long step = 0;
  long bound_step = 0;            // `step` at the bind
  bool buf_live = false;          // SGD: momentum_buffer holds a value (GT_OPTF_BUFFER_LIVE at the bind, or an update since)
  OptimScalarCache hs_cache;      // reset by every bind
  // injected dropout masks [pass][layer] (pass 3: the discriminator's forward over the WGAN-GP interpolates)
  const float* inj[4][16];
  Net() { memset(inj, 0, sizeof(inj)); }
};

// One network's device workspace, gt_engine::ws[role].  Per role is whatever must survive the OTHER role's passes inside a step: the generator's forward
// stash has to outlive both discriminator passes (update_generator back-propagates it last), so a discriminator has its own (its D-step stash is dead after
// the D step; the G-step pass reuses it).  Transient within one call and shared by both roles, hence on the engine: l_state, l_xch, s_du, s_dx, s_dbias, dzA,
// dzB, dz_b, slabs, colp, d_dx0, i2o_gout, the step workspace.  Unused members stay empty.  LSTM and SRU images / shadows stay apart: size() == layers + 1 catches a stale rebind.
struct NetWs {
  std::vector<Scratch> act; std::vector<B16Img> actb;     // MLP: hidden activations; under GT_OPT_MATMUL_BF16 their bf16 images (both orientations)
  std::vector<DropoutSpec> specs; std::vector<LinShadow> wsh;      // dropout sites of the stashed pass; bf16 shadows of the hidden layers' weights, then of the last layer's
  Scratch w0pad; SlabDefer sdefer;                 // first hidden layer's weight with a 16-byte row pitch (stack_forward); deferred weight-gradient combines of the fused step
  std::vector<Scratch> xproj, gates, cst, out, outd;      // LSTM, per layer (outd: inter-layer-dropped outputs)
  Scratch hshift, dout;                            // dout, either recurrent stack: gradient w.r.t. the current layer's output (a discriminator's head seeds it)
  // ... its bf16 path, the generator's alone: images of every layer's input (+ the top output, last entry), dG, h that entered each frame (transposed); W_ih of all directions stacked [dirs*4H][in] (last entry: hidden2out)
  std::vector<B16Img> l_in_b, l_dg_b; B16Img l_hs_b; std::vector<LinShadow> lsh;
  // SRU, per layer: stashes; xmask: input-dropout multipliers [B][n_in]; wt: float32 mode's transposed W; omask: a discriminator's output-dropout keep
  // tables [nseq][ncols], each row group of a launch drawn from its own pass (the generator's scans draw theirs inline: empty).  The bf16 path is role-owned
  // too: the generator's s_in_b[l].t() and ssh[l] are read by sru_backward AFTER both discriminator passes.  A discriminator (GT_OPT_SRU_D_BF16) has no top
  // s_in_b entry (the fused head reads the float32 h) and no hidden2out ssh (that product lives in the head kernel)
  std::vector<Scratch> u, h, c, xdrop, xmask, wt, omask;
  std::vector<B16Img> s_in_b; B16Img du_b;         // image of every layer's (dropped) input (+ the top output); dU of the current layer, both orientations
  std::vector<LinShadow> ssh;                      // per layer W (n_in, ncols*k) as w [n_in][..] and wt [ncols*k][n_in]; last entry: hidden2out
};
struct StepCopy {      // a copy of a caller tensor made once per step (with a 16-byte pitch, or dense), keyed by what it was made from
  Scratch buf; const float* src = nullptr; int ld = 0, cols = 0; long rows = 0; uint64_t step = ~0ULL;
  bool holds(const float* s, int l, int c, long r, uint64_t st) const { return src == s && ld == l && cols == c && rows == r && step == st; }
  void built(const float* s, int l, int c, long r, uint64_t st) { src = s; ld = l; cols = c; rows = r; step = st; }      void forget() { src = nullptr; }
};
// Banded images of the MLPG matrices the caller has passed so far, one per (R pointer, T): batches of a corpus come in
// many padded lengths and the caller (gantts_amd.paramgen / the reference's per-batch R) keeps one R per T, so after the
// first sight of a T there is no extraction kernel, no D2H copy and no host synchronisation on the step path.
// Contract (include/gantts_hip.h): R is immutable while cached; gt_invalidate_mlpg_cache() after rewriting / freeing it.
struct MlpgBand {
  const float* R = nullptr;
  int T = 0, kb = 0;
  uint64_t last_use = 0;
  Scratch band;
};
// The window set of gt_set_mlpg_windows, as the build kernels take it (by value): entries whose R is GT_MLPG_R_FROM_WINDOWS are built from
// it on the device (mlpg_band_kernels.hip.h) instead of being extracted from a dense R, and can be rebuilt after an eviction.
constexpr int MLPG_WIN_SPAN = GT_MLPG_MAX_WINDOW_SPAN;      // l + u of a registered window
struct MlpgWindows {
  int n;
  int l[MLPG_MAXW], u[MLPG_MAXW];
  double coef[MLPG_MAXW][MLPG_WIN_SPAN + 1];
};
struct MlpgCache {
  static constexpr size_t MAX_ENTRIES = 256;
  std::vector<std::unique_ptr<MlpgBand>> entries;
  uint64_t tick = 0;
  Scratch tmp;                      // per-offset maxima of a new R (persistent: no hipFree on the step path)
  bool has_win = false;
  MlpgWindows win;                  // zero-filled beyond the registered windows and coefficients: compared with memcmp
  Scratch fac, wide;                // device build: Cholesky factor and selected inverse (float64), the taps at the candidate width
  void clear() { entries.clear(); }      // (the caller has synchronised and told on_band_freed)
};

// How a step's scalars reach the host, three routes and the one owner of their state.  early: the finalising launch of a fused call writes them into
// the pinned page and the call returns once they have landed -- seen by polling a ticket behind them (GT_OPT_POLL_RESULTS) or, ticket 0, by an event -- with the rest
// of the step still queued; deferred (split-phase, out == NULL): own pinned copy + event per role, collected by gt_update_*_result; blocking: copy + synchronise.
struct ResultsChannel {
  Pinned<StepResults> h_res; StepResults* h_res_dev = nullptr;      // pinned page: the results, the ticket 64 bytes behind them; the same page as the kernels see it (null: GT_RES_HOSTMAP=0, or no device view)
  StepResults* d_res = nullptr; const bool* poll = nullptr;      // of the engine: res(), where the finalising launches of the other routes leave the results; opt_poll_results
  bool early = false, early_done = false;  // a fused call is running; its early results are posted and not waited for yet
  unsigned ticket_next = 0, ticket_wait = 0; Event ev_res;      // last number handed out / the one the posted early results carry (0: ev_res is used)
  Pinned<StepResults> h_def[2]; Event ev_def[2]; bool def_pending[2] = {false, false};
  bool begin_done[2] = {false, false};     // per role: gt_update_*_begin has run, _end has not
  long long waits = 0;                     // gt_host_wait_count: times a call blocked its thread on the device (wait_early, collect, fetch; gt_ledger_read adds its own)
  int create(StepResults* device_results, const bool* poll_option);
  StepResults* target() const { return h_res_dev ? h_res_dev : d_res; }      // where a launch that reports early writes the results
  unsigned* ticket_dev() const { return h_res_dev ? (unsigned*)((char*)h_res_dev + 64) : nullptr; }
  volatile unsigned* ticket_host() const { return (volatile unsigned*)((char*)h_res.p + 64); }
  unsigned take_ticket() { if (!*poll || !h_res_dev) return 0;      if (++ticket_next == 0) ++ticket_next;      return ticket_next; }      // for results that the NEXT finalising launch writes into the host page (0: not available)
  int post_early(hipStream_t s, unsigned ticket = 0);
  int wait_early();                        // only the scalars; backward + step stay queued
  bool early_posted() const { return early_done; }      void clear_early() { early_done = false; }
  int post_deferred(int role, hipStream_t s);
  int collect(int role) {                  // ... then in h_def[role]
    if (!def_pending[role]) return fail(GT_ERR_STATE, "no deferred %s result pending", role == GT_ROLE_D ? "discriminator" : "generator");
    ++waits;
    HIPCHK(hipEventSynchronize(ev_def[role]));
    def_pending[role] = false;
    return GT_OK;
  }
  int fetch(hipStream_t s) { ++waits; HIPCHK(hipMemcpyAsync(h_res, d_res, sizeof(StepResults), hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return GT_OK; }
  void abandon() { early_done = false; ticket_wait = 0; }      // a fused call whose _begin failed
  void forget_begin() { begin_done[0] = begin_done[1] = false; }      // an option changed what an open _begin had stashed
  void reset() { forget_begin(); early_done = false; }         // gt_clear_faults
};

// Epoch ledger (eng_ledger.hip, ledger_kernels.hip.h): train_loop's running sums of a phase in device memory.  `rec` is sized once by
// gt_ledger_configure and never grows afterwards: [GT_LEDGER_SLOTS doubles: the record | 8 doubles: the last batch's distortion sums |
// col_stat[Ds], col_role[Ds] | 1024 x DIST_NSUM doubles: partials of the distortion reduction].
struct EpochLedger {
  bool configured = false;
  int kind = 0, Ds = 0, vuv_col = -1, stats_f64 = 0;
  double logdb_const = 0.0;
  const void *mean = nullptr, *stdv = nullptr;     // the caller's statistics (device), read by every gt_ledger_add
  Scratch rec, len;                                // len: the batch's lengths as int32 (grows with B only)
  size_t off_tab = 0, off_part = 0;
  Pinned<double> h_out;                            // gt_ledger_read's copy
  double* record() const { return rec.as<double>(); }
  double* dist() const { return rec.as<double>() + GT_LEDGER_SLOTS; }
  int* col_stat() const { return (int*)((char*)rec.p + off_tab); }
  int* col_role() const { return col_stat() + Ds; }
  double* partials() const { return (double*)((char*)rec.p + off_part); }
};

// Spectral normalisation of the MLP discriminator (eng_spectral_norm.hip, spectral_norm_kernels.hip.h).  SnPlan: the job table of a
// network (one job per nn.Linear weight), its launch grids and the ranges no job covers, built once per bind.  SnBufs: the double sums
// between the launches, sized by sn_plan_bytes.  SnState: the engine's -- u, v are the caller's (like optimizer state), W_eff the engine's.
struct SnLayerDesc { long w_off; int out, in; };
struct SnPlan;
void sn_plan_free(SnPlan* p);
struct SnPlanFree { void operator()(SnPlan* p) const { sn_plan_free(p); } };
using SnPlanPtr = std::unique_ptr<SnPlan, SnPlanFree>;
struct SnBufs { double *t, *r, *sp, *s; float* sigma; };
struct SnState {
  bool on = false;
  float *u = nullptr, *v = nullptr;                // caller-owned, sum(out) and sum(in) floats
  SnPlanPtr plan;
  Scratch weff, ws;                                // W / sigma in the flat buffer's layout (biases unused); SnBufs
  SnBufs bufs = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

// Gradient penalties of the MLP discriminator (eng_grad_penalty.hip, grad_penalty_kernels.hip.h).  GpCall: one second-order pass over plain
// buffers, what the step (d_pass_penalty) and the hook gt_op_grad_penalty hand to launch_grad_penalty.  GpState: the engine's switch, its
// scratch and the running record {sum P, sum mean-norm, steps} in device memory.
namespace gt { enum GpKind { GP_OFF = 0, GP_R1 = 1, GP_WGAN = 2 }; }
struct GpLayer {
  const float* W; float* dW; int in, out;          // dense (out, in) weight and its gradient (layer 0: in = cd + Da)
  const float* H; gt::DropoutSpec spec;            // the stored activation [rows][out] and its dropout site
  float* a; float* c;                              // [rows][out]: gradient chain and tangent chain (c may alias another layer's c two layers away)
};
struct GpCall {
  int L, cd, Da, kind, prec; float weight; long rows;
  GpLayer l[16];
  const float* w_last; float* dw_last;             // the head's weight [H] and its gradient
  float* g; int ld_g; float* g_copy;               // [rows][ld_g]: g, then r in its place; g_copy (may be null) keeps g
  const float* mask; const float* inv_tv_dev; float inv_tv;
  float* phi; float* nrm;                          // per-row values [rows], may be null
  double* part; long part_cap;                     // [2][workgroups of gp_row]
  double* sums; double* rec;                       // this call's two sums; the running record (either may be null)
  float* dw0s;                                     // dense [out_0][Da]: a_0^T r before it is added into dW_0[:, cd:]
  Scratch* slabs; Scratch* colp;
};
struct GpState {
  int kind = 0; float weight = 0.f;                // gt_set_grad_penalty: 0 off, 1 r1, 2 wgan-gp
  const float* eps_inj = nullptr;                  // gt_set_gp_epsilon: [N] or null (Philox)
  Scratch g, dw0, part, rec, eps;
  hipStream_t stream = nullptr;                    // of the last penalised step (gt_grad_penalty_result synchronises it)
  const float* img = nullptr; int img_ld = 0, img_col0 = 0; long img_rows = 0;      // where the last step's x_hat image lies (gt_grad_penalty_peek)
};

// The loss normaliser Tv = sum(mask) (or what the caller gave instead) and 1 / Tv in the step's scalars: the one owner of everything the host
// knows about them, one method per event.  Which launches put them there in a discriminator step is TvPlan's (eng_step.hip); every other
// reader calls ensure().  With a communicator the count is the GLOBAL one: losses are normalised by the valid frames of the whole minibatch
// (train.py:258, seqloss.py:43); start / send hand the local term to the communicator's stream, join makes the step stream wait for it.
// No "all-reduce in flight" flag is kept: a call that sends also joins before it returns (ensure; TvPlan's ALLREDUCE route), so the flag was
// false between calls unless one failed midway -- and then the resets on a new batch / zero_grad made the next call count afresh, as every call
// does now.  The un-joined message of such a failed call stays ordered on the communicator's stream in front of the next one.
struct LossNormaliser {
  float override() const { return ovr; }                      // gt_set_loss_normalizer: > 0 wins over the mask's sum
  const double* total_dev() const { return dev; }             // gt_set_loss_normalizer_device: the caller's global count, read in stream order
  bool given() const { return dev || ovr > 0.f; }             // the caller's: no collective of the engine's own
  double* reduced() const { return total.as<double>(); }      // the all-reduced count (local term before send, global after join)
  bool known(const float* m, long N) const { return mask == m && n == N && memo_ovr == ovr; }      // the scalars hold the normaliser of this mask already
  void note(const float* m, long N) { mask = m; n = N; memo_ovr = ovr; }
  // forget: a new batch (gt_apply_generator), gt_zero_grad, another device total -- the mask's contents may have changed.  overwritten: the MLPG
  // hook's masked-MSE gradient put another mask's normaliser into the scalars (with no in-flight flag, all there is to clear is the memo).
  void forget() { mask = nullptr; }      void overwritten() { forget(); }
  void set_override(float tv) { ovr = tv; dev = nullptr; }      // (the memo is keyed on the override: nothing to forget)
  void set_total_dev(const double* p) { dev = p; forget(); }    // re-read on the next step function
  int attach() { return total.ensure(64); }      // gt_comm_init
  int start(gt_engine* e, const float* m, long N, hipStream_t s);      // the local count by a launch of its own, then send
  int send(gt_engine* e, hipStream_t s);                               // all-reduce of reduced() on the communicator's stream, behind what `s` holds
  int join(gt_engine* e, hipStream_t s);
  int file(gt_engine* e, const float* m, long N, const double* from, hipStream_t s);      // override / *from / sum(mask) -> the scalars, by a launch; noted
  int ensure(gt_engine* e, const float* m, long N, hipStream_t s);     // once per (step, mask): no-op when known
  // GT_OPT_COMM_TV_IN_SUMS: D's gradient of the running step is that of the UNNORMALISED loss.  Set by every D step's _begin, read by the early
  // finalisation, taken (and cleared) by the optimizer step as the update kernel's gradient scale.
  void d_step_begins(bool unnormalised) { d_unnorm = unnormalised; }
  bool d_unnormalised() const { return d_unnorm; }
  const float* take_d_scale(StepScalars* sc) { const bool u = d_unnorm; d_unnorm = false; return u ? &sc->inv_tv : (const float*)nullptr; }
  static const float* inv_tv(StepScalars* sc) { return &sc->inv_tv; }      // 1 / Tv on the device, for launches that read it there
 private:
  float ovr = -1.f; const double* dev = nullptr;
  const float* mask = nullptr; long n = 0; float memo_ovr = 0.f;      // the memo: of which mask, over how many frames, under which override
  Scratch total; bool d_unnorm = false;                                // total: device double, the communicator's message
};

// dloss_d/dy_hat_static of the D step, kept for the generator step's gradient assembly (the reference's un-detached "leak", train.py:265,274).
// unnorm: it is that of the unnormalised loss (GT_OPT_COMM_TV_IN_SUMS): x 1 / Tv where it is consumed.
struct KeptLeak {
  // D step: *out = where the backward pass leaves it, or null when this step keeps none (eng_step.hip); refuses a second one before zero_grad
  int claim(gt_engine* e, const float* y_hat_static, long N, float** out);
  void kept(bool unnormalised) { pending = true; unnorm = unnormalised; }
  const float* get() const { return pending ? buf.as<float>() : (const float*)nullptr; }      // null: none pending
  bool unnormalised() const { return pending && unnorm; }
  // gt_zero_grad(G); consumed by the G step / gt_flush_generator_grads; no longer the gradient of what the next G step runs (storage form,
  // objective, spectral norm, a recycled band, gt_clear_faults)
  void drop() { pending = unnorm = false; }
 private:
  Scratch buf; bool pending = false, unnorm = false;
};

// The stashed generator pass: what gt_apply_generator's forward left behind for the step's one backward pass (the training G step, or
// gt_flush_generator_grads).  The activations themselves are ws[GT_ROLE_G]'s; this is which pass they are of, and whether they still are.
struct GenPass {
  // gt_apply_generator, after its forward has succeeded (dropped before it); x: what the backward pass reads, the dense copy when one was made
  void stash(int B_, int T_, const float* x_, const float* y_hat, const float* y_hat_static) {
    b = B_; t = T_; n = (long)B_ * T_; x = x_; yhat = y_hat; yhs = y_hat_static; valid = true;
  }
  void drop() { valid = false; }
  bool live() const { return valid; }
  bool is(const float* y_hat, const float* y_hat_static, long N_) const { return valid && yhat == y_hat && yhs == y_hat_static && n == N_; }      // the training G step's
  bool made(const float* y_hat_static, long N_) const { return valid && yhs == y_hat_static && n == N_; }      // KeptLeak::claim's
  // the band the pass went through (null: R is None), set by generator_forward under `stash` alone; the cache never recycles it while live().
  // band_freed: the cache frees b; true when it was this pass's, which can then no longer be back-propagated
  const MlpgBand* band() const { return bnd; }      void went_through(const MlpgBand* band_) { bnd = band_; }
  bool band_freed(const MlpgBand* band_) { if (bnd != band_) return false;      bnd = nullptr; valid = false; return true; }
  // the generator forward in hand reads the dense copy of its input (dense_gx, every generator forward): gx_pitch() == in_dim
  bool input_dense() const { return dense; }      void input_dense(bool on) { dense = on; }
  int B() const { return b; }      int T() const { return t; }      long N() const { return n; }
  const float* input() const { return x; }      const float* y_hat() const { return yhat; }
 private:
  int b = 0, t = 0; long n = 0;
  const float *x = nullptr, *yhat = nullptr, *yhs = nullptr;
  const MlpgBand* bnd = nullptr;
  bool dense = false, valid = false;
};

// The memos of D's input.  DImage: "the generated half of this image of D's input is built", and from which x / y_hat_static: the generator
// step's adversarial term reuses what the D step of the same batch left behind.  One record per image kind, one StepCopy per engine-made copy
// of x; the buffers they describe (dcat, dcat_b, adv2) stay the engine's.
struct DImage {
  bool valid = false; const float* x = nullptr; const float* yhs = nullptr;
  bool holds(const float* x_, const float* yhs_) const { return valid && x == x_ && yhs == yhs_; }
  void built(const float* x_, const float* yhs_) { valid = true; x = x_; yhs = yhs_; }
};
struct DInputMemos {
  DImage img_cat, img_cat_b, img_adv2;             // of dcat (float32 [x | adv]), dcat_b (its bf16 image), adv2 (adversarial columns only: x is ignored, kept null)
  StepCopy dx_pitched, gx_pitched, cx_dense;       // 16-byte-pitch copies of D's conditioning x / G's input (pitched_rows), the dense conditioning x (dense_cx)
  void invalidate_d_images() { img_cat.valid = img_cat_b.valid = img_adv2.valid = false; }      // whatever image of D's input is kept gets rebuilt
  void forget_copies() { dx_pitched.forget(); gx_pitched.forget(); cx_dense.forget(); }
};

struct gt_engine {
  gt_stream_config cfg;
  Net net[2];
  uint64_t seed = 0x5DEECE66DULL;
  uint64_t step_counter = 0;
  LossNormaliser norm;
  KeptLeak leak;
  // derived stream maps (device)
  int Dout_cfg = 0, Ds = 0, Da = 0;
  std::vector<int> h_scol, h_sstride, h_adv_cols, h_adv_inv;
  Scratch d_scol, d_sstride, d_adv_cols, d_adv_inv;      // int [Ds] / [Da] / [Ds]
  // In2Out uses a single dynamic stream of width out_dim
  Scratch d_scol_i2o, d_sstride_i2o; int i2o_ds = 0;
  MlpgCache mlpg;
  Scratch mlpg_var_ws;                     // variance-weighted MLPG: refusal flag, lengths, then L and z of one group of sequences (float64)
  NetWs ws[2];                             // workspace: per role, then (below) what one call uses and both roles share
  Scratch dcat, dzA, dzB, gadv, gs, gy, slabs, colp, partial, headp, headw, dmask, tx, gx, dgx, dtz, dout;
  Scratch scal;                            // StepScalars + StepResults
  ResultsChannel results;                  // how the step's scalars reach the host
  EpochLedger ledger;                      // gt_ledger_*: the loop's running sums, added on the device behind each step
  // per-step state: what outlives a call is forgotten by the events below the struct
  GenPass pass;
  DInputMemos din;
  bool g_has_adv = false;
  Scratch i2o_gout, d_dx0;                         // In2OutRNNHighwayNet: hidden2out output G(x); a recurrent DISCRIMINATOR (train.py:773-774 allows any model class): gradient w.r.t. its [x | adv] input
  Scratch l_state, l_xch, s_du, s_dx, s_dbias;     // recurrent layer in hand (either role): LSTM per-step kernels' state, persistent kernels' exchange granules; SRU backward temporaries
  struct GtComm* comm = nullptr;                   // gt_comm_init: RCCL communicator + comm stream (data parallel)
  struct GtIpc* ipc = nullptr;                     // gt_comm_ipc_*: interprocess arenas of the two-shot all-reduce (eng_ipc.hip)
  bool opt_comm_ipc = env_flag("GT_COMM_IPC", true);      // GT_OPT_COMM_IPC: messages that fit the arena's slots take that path once the arenas are attached
  int dp_rank = 0, dp_world = 1;                   // this engine's shard of the minibatch (gt_comm_init / gt_set_shard): sequence b here
                                                   // is sequence dp_rank + dp_world * b of the whole minibatch (round-robin dealing)
  int chk_B = 0, chk_T = 0;                        // (B, T) of the entry point that is running (check_common)
  std::vector<std::pair<long, long>> comm_done[2]; // per role: gradient ranges (offset, count) already handed to RCCL this step
  std::vector<std::pair<long, long>> comm_pending[2];   // final on the step stream, not handed over yet (merged into few messages)
  // GT_OPT_MATMUL_BF16 on MLP stacks: bf16 images (both orientations) of everything that only feeds products
  B16Img xin_b, dcat_b, gy_b, dz_b[2], fwd_b;      // G's input, D's [x | adv] image (2N rows), dloss/dy_hat, dZ ping-pong, gt_model_forward's input
  Scratch d_pre;                                   // split first layer of the conditioned D: P = x . W[:, :cd]^T + b  (eng_step.hip: FirstSplit)
  Scratch adv2; int ld_adv2 = 0;                   // ... and the adversarial columns of a pass's rows, [real | generated], 16-byte pitch
  // GT_OPT_SPLIT_FIRST_LAYER (per engine; the environment only provides the default at creation)
  // GT_OPT_FUSED_DSTACK: the float32 MLP discriminator's layers above the first one + the head (+, in the generator step, the
  // backward-data chain down to the adversarial columns) as ONE launch per pass (dstack_f32.hip.h)
  int opt_fused_dstack = getenv("GT_FUSED_DSTACK") ? atoi(getenv("GT_FUSED_DSTACK")) : 1;      // 0 off, 1 when the pass has >= one panel per CU, 2 always
  bool opt_split_first = env_flag("GT_D_SPLIT", true);
  // data-parallel schedule (GT_OPT_COMM_*): D's gradient as one message, G's loss sums early,
  // collectives issued even with one rank (bench.py --force-dp, tests)
  bool opt_comm_d_one_msg = env_flag("GT_COMM_D_ONE_MSG", true), opt_comm_early_g = env_flag("GT_COMM_EARLY_G", true),
       opt_comm_force = getenv("GT_COMM_FORCE_COLLECTIVES") != nullptr;
  bool opt_comm_close_inline = env_flag("GT_COMM_CLOSE_INLINE", true);   // GT_OPT_COMM_CLOSE_INLINE: a step's closing messages on the step stream itself
  // GT_OPT_COMM_TV_IN_SUMS: the data-parallel D step does not all-reduce the valid-frame count ahead of the head; the head seeds the
  // backward pass of the UNNORMALISED loss, the local count leaves with the four loss / count sums (one message instead of two), and
  // 1 / Tv is applied where the gradient is consumed: by the optimizer kernel (which writes the normalised, clipped gradient back) and
  // by the generator step's gradient assembly for the kept dloss_d/dy_hat_static.  In that state right now: LossNormaliser::d_unnormalised,
  // KeptLeak::unnormalised.
  bool opt_comm_tv_in_sums = env_flag("GT_COMM_TV_IN_SUMS", true);
  bool opt_poll_results = env_flag("GT_POLL_RESULTS", true);      // GT_OPT_POLL_RESULTS (ResultsChannel::take_ticket): round 4: no gain (1.380 / 1.384 vs 1.381 / 1.375 ms); round 5, the step 60 us shorter: 1.3125 / 1.312 vs
                                                                  // 1.319 / 1.315 / 1.3175 / 1.3206 ms, b = 4 0.400 vs 0.406 -- the two 5.8 us holes behind the finalising launches now show
  bool opt_launch_riders = env_flag("GT_LAUNCH_RIDERS", true);     // GT_OPT_LAUNCH_RIDERS: small reductions as extra workgroups of neighbouring launches
  int ld_gx = 0, ld_cx = 0;                        // gt_set_x_pitch: row pitch of the generator input / the conditioning x (0 = dense)
  // gt_set_x_pitch: pitched rows are read in place by the float32 MLP generator and by the split first layer of the conditioned float32 MLP
  // discriminator.  Every other network gets a DENSE copy made by the engine, once per step (dense_gx / dense_cx in eng_step.hip):
  // gt_set_x_pitch never makes a step fail (DevicePrefetcher(pitch_x=True) with a recurrent discriminator did).
  Scratch gx_dense;                                // dense_gx's copy (GenPass::input_dense)
  unsigned int* h_fault_dev = nullptr;             // device view of h_fault[1]: the optimizer kernel mirrors a raised fault word
  Scratch d_fault;                                 // device fault word of the persistent kernels (0 = ok)
  Pinned<unsigned int> h_fault;                    // pinned mirror, refreshed behind every persistent launch
  bool lstm_persistent = getenv("GT_LSTM_STEPS") == nullptr;   // GT_OPT_LSTM_PERSISTENT (the environment only provides the default at creation)
  int lstm_fwd_upc = 0;                            // 0 = automatic
  bool lstm_xcd_local = getenv("GT_LSTM_NO_XCD_LOCAL") == nullptr;   // GT_OPT_LSTM_XCD_LOCAL
  int64_t lstm_paths[GT_LSTM_PATH_SLOTS] = {};      // recurrence layer-passes by kernel instantiation (gt_lstm_path_counts), counted on the host
  bool matmul_bf16 = false;                                          // GT_OPT_MATMUL_BF16
  // sequence lengths travel on the step stream through a small ring (pinned host slot -> device slot): the kernels of
  // the previous step, still queued when the next batch's lengths arrive, keep reading THEIR slot
  static constexpr int LEN_RING = 4;
  Pinned<int> len_host[LEN_RING];
  Scratch len_dev[LEN_RING];
  Event len_ev[LEN_RING];
  int len_cap = 0, len_slot = -1;
  unsigned int* fault_dev() const { return d_fault.as<unsigned int>(); }
  int* d_lengths() { return len_slot < 0 ? nullptr : len_dev[len_slot].as<int>(); }
  bool sru_d_bf16 = env_flag("GT_SRU_D_BF16", false);      // GT_OPT_SRU_D_BF16: an SRU discriminator's products through the bf16-storage family
  int gan_objective = 0;                           // GT_OPT_GAN_OBJECTIVE: the head's adversarial objective (gan_objective.hip.h), 0 = the reference's sigmoid + log loss
  float weight_clip[2] = {0.f, 0.f};               // gt_set_weight_clip (role D only): every optimizer step clamps the updated parameters to [-c, c]; 0 = off
  // gt_set_param_ema (role G only): the caller's running average of the generator's parameters, its length, the decay, and the updates
  // applied to it (torch's n_averaged: counted where Net::step is, skipped steps taken back out by gt_clear_faults); buf null = off
  struct ParamEma { float* buf = nullptr; long n = 0; double decay = 0.0; long count = 0; } ema;
  SnState sn;                                      // gt_set_spectral_norm (role D, MLP only): Lin::W of the discriminator then points into sn.weff
  GpState gp;                                      // gt_set_grad_penalty (role D, MLP only): one more stage of the D step (d_pass_penalty)
  std::vector<int> h_lengths;
  StepScalars* sc() { return scal.as<StepScalars>(); }
  StepResults* res() { return (StepResults*)((char*)scal.p + 256); }
};
// What each event forgets of the state the engine keeps between calls: one function per event, each entry point calls its
// own and writes none of this itself.  Assignments only -- several are on the step path.  (A D step rebuilding both halves of its input
// calls DInputMemos::invalidate_d_images itself: that is use, not an event; KeptLeak::drop where the gradient is consumed likewise.)
// gt_apply_generator.  No StepCopy outlives a batch: the step count alone does not tell two batches apart (gt_set_seed restarts it, and a staging
// buffer refilled in place has the same pointer, pitch and shape).  Both update calls of a batch come behind this one: they still share a copy.
// The mask's contents may have changed as well.
static inline void on_new_batch(gt_engine* e) { e->pass.drop(); e->din.invalidate_d_images(); e->din.forget_copies(); e->norm.forget(); }
static inline void on_reseed(gt_engine* e) { e->din.forget_copies(); }      // gt_set_seed: the step count, part of the copies' key, has just gone back
static inline void on_first_layer_route_changed(gt_engine* e) { e->din.invalidate_d_images(); }      // GT_OPT_SPLIT_FIRST_LAYER
// GT_OPT_MATMUL_BF16: the storage precision belongs to a PASS -- buffers of a stashed forward pass (bf16 images vs float32 stashes) are not
// interchangeable, so the next update_* asks for a fresh apply_generator instead of back-propagating through buffers the forward never filled
static inline void on_storage_form_changed(gt_engine* e) {
  e->din.invalidate_d_images(); e->pass.drop(); e->leak.drop(); e->din.cx_dense.forget(); e->results.forget_begin();
}
// GT_OPT_SRU_D_BF16 (as above: a discriminator pass stashed in one storage form is not back-propagated in the other)
static inline void on_sru_d_storage_form_changed(gt_engine* e) { e->din.invalidate_d_images(); e->leak.drop(); e->results.forget_begin(); }
// GT_OPT_GAN_OBJECTIVE: a discriminator pass begun under one objective is not finished, and its kept gradient not used, under another
static inline void on_objective_changed(gt_engine* e) { e->leak.drop(); e->results.forget_begin(); }
// gt_set_spectral_norm, off / on: a pass begun with the feature is not finished without it, nor the other way round
static inline void on_spectral_norm_off(gt_engine* e) { e->din.invalidate_d_images(); e->leak.drop(); e->results.forget_begin(); }
static inline void on_spectral_norm_on(gt_engine* e) { e->leak.drop(); e->results.forget_begin(); }
static inline void on_penalty_kind_changed(gt_engine* e) { e->results.forget_begin(); }      // gt_set_grad_penalty: a D step begun under one setting is not finished under another
// the MLPG cache frees b: the stashed pass would transpose through it
static inline void on_band_freed(gt_engine* e, const MlpgBand* b) { if (e->pass.band_freed(b)) e->leak.drop(); }
static inline void on_generator_rebound(gt_engine* e) { e->pass.drop(); }      // gt_bind_model(role G)
static inline void on_generator_plain_forward(gt_engine* e) { e->pass.drop(); }      // gt_model_forward(role G): it ran over the stashed pass's activations
static inline void on_zero_grad(gt_engine* e, int role) { e->norm.forget();      if (role == GT_ROLE_G) e->leak.drop(); }
static inline void on_faults_cleared(gt_engine* e) {      // gt_clear_faults
  e->din.invalidate_d_images(); e->pass.drop(); e->leak.drop(); e->din.cx_dense.forget(); e->results.reset();
}

// ------------------------------------------------------------------------------------------
// eng_core.hip
// ------------------------------------------------------------------------------------------
int check_common(gt_engine* e, int B, int T);
int fault_seen(gt_engine* e);
// the optimizer family (eng_ops.hip): validation shared by gt_bind_optimizer_ex / gt_op_optim_step, and the one place that
// launches the fused clip + update kernel.  `step`: 1-based count of THIS update; `part`: n_partial squared-norm partials.
int optim_check_desc(const gt_optim_desc_ex* od);
void optim_desc_copy(const gt_optim_desc_ex* in, gt_optim_desc_ex* out);      // head only for the first family's kinds
int launch_optim_step(const gt_optim_desc_ex& od, long step, bool buf_live, OptimScalarCache* cache, float* params, float* grads, long n,
                      const double* part, int n_partial, double* norm2_out, const unsigned int* fault_dev, unsigned int* fault_host,
                      unsigned int* skipped_host, const float* gscale, hipStream_t s, float weight_clip = 0.f, float* ema = nullptr,
                      float ema_w = 0.f, bool ema_first = false);
// the weight average of gt_set_param_ema: its decay's check (`who` names the entry point in the message), the lerp weight float32(1.0 - decay)
// -- the subtraction in double, rounded once, as python forms it for Tensor.lerp_ --, and the setting against the bound generator
int param_ema_check_decay(const char* who, double decay);
static inline float param_ema_weight(double decay) { return (float)(1.0 - decay); }
int check_param_ema(const gt_engine* e);
// GT_OPT_GAN_OBJECTIVE against the bound discriminator's last_sigmoid (true under objective 0, false under 1 .. 6): checked at whichever of
// gt_bind_model / gt_set_option comes second and at the entry of every step that runs the discriminator, before any launch
int check_gan_objective(const gt_engine* e);
// NAdam's mu_product / ASGD's eta and mu after `t` updates (t >= od.step); `cache` may be null
void optim_host_scalars(const gt_optim_desc_ex& od, long t, OptimScalarCache* cache, double out[2]);
gt::DropoutSpec philox_site_spec(gt_engine* e, int role, int pass, int layer, uint64_t step, float p, long half_rows = 0);
gt::DropoutSpec drop_spec(gt_engine* e, int role, int pass, int layer, const float* stacked_mask, int ld, long half_rows = 0);

// ------------------------------------------------------------------------------------------
// eng_gemm_f32.hip -- products of the float32 family (PREC_F32) or bf16 products on float32 storage (PREC_BF16): `prec`, an argument of
// every launch function.  product_prec (eng_core.hip) is the policy: PREC_F32 for an SRU network in the discriminator slot (its stack and
// hidden2out stay float32 products under either bf16 option), else PREC_BF16 iff GT_OPT_MATMUL_BF16.
// ------------------------------------------------------------------------------------------
int product_prec(const gt_engine* e, int role);
// gt_gemm_path_counts: launches of the family by kernel, counted on the host where they are issued (slot encoding in gantts_hip.h)
enum { GEMM_PATH_PAIR = 576, GEMM_PATH_TN_PAIR = 580, GEMM_PATH_REDUCE4 = 582, GEMM_PATH_REDUCE = 583, GEMM_PATH_REDUCE_SMALL = 584,
       GEMM_PATH_COLSUM_PARTIAL = 585, GEMM_PATH_COLSUM_FINALIZE = 586, GEMM_PATH_REDUCE_MULTI = 587 };
static_assert(GEMM_PATH_REDUCE_MULTI + 1 == GT_GEMM_PATH_SLOTS, "gt_gemm_path_counts slots");
constexpr int gemm_path_slot(int kind, int bm, int bn, bool va, bool vb, int prec, int amode) {
  return (((((kind * 2 + (bm == 128)) * 2 + (bn == 128)) * 2 + va) * 2 + vb) * 2 + (prec == gt::PREC_BF16)) * 6 + (amode + 1);
}
void gemm_path_count(int slot);
// may this operand be loaded 16 bytes per lane?  k-contiguous operands (rows of X / W in the forward product, rows of dZ in
// backward-data): any float pointer and pitch (unaligned 16-byte loads, gemm_f32.hip.h: ld4u); operands whose contiguous
// direction is m / n: 16-byte aligned base and a pitch that is a multiple of 4 floats (GT_GEMM_UNALIGNED=0: that rule for all)
bool gemm_vec_ok(const float* p, int ld, bool k_contiguous = false);
bool gemm_wide_store_ok(int kind, const gt::GemmArgs& g);
bool gemm_small_tiles_ok();
// fused discriminator stack (eng_dstack.hip, dstack_f32.hip.h)
namespace gt { struct DStackArgs; }
bool dstack_hidden_ok(int hidden_dim);
int dstack_panels(long rows);
int launch_dstack(const gt::DStackArgs& a, int hidden_dim, hipStream_t s, int objective = 0);
// eng_gan_objective.hip: the instantiations of both tail kernels for the objectives 1 .. 3 (gan_objective.hip.h), in a unit of their own
int launch_dstack_objective(const gt::DStackArgs& a, int hidden_dim, int objective, hipStream_t s);
// eng_gan_fdiv.hip: the same for the f-GAN divergences 4 .. 6, reached through launch_dstack_objective
int launch_dstack_fdiv(const gt::DStackArgs& a, int hidden_dim, int objective, hipStream_t s);
// gt_head_path_counts: launches of the discriminator's tail by kernel, counted on the host where they are issued (slot layout in
// gantts_hip.h).  launch_d_head / launch_dstack_pass / launch_head_finalize (eng_step.hip, d_tail_args.hip.h): the one launch site of each
// kernel, shared by the engine's run_head / run_dstack and the parity hooks (eng_ops.hip).
enum { HEAD_PATH_F32 = 0, HEAD_PATH_VEC = 4, HEAD_PATH_IMG = 7, HEAD_PATH_DSTACK128 = 11, HEAD_PATH_DSTACK256 = 12, HEAD_PATH_FINALIZE64 = 13,
       HEAD_PATH_FINALIZE16 = 14 };
static_assert(HEAD_PATH_FINALIZE16 + 1 == GT_HEAD_PATH_SLOTS, "gt_head_path_counts slots");
void head_path_count(int slot);
namespace gt { struct HeadCall; struct HeadSums; struct HeadArgs; struct DStackCall; }
int launch_head_finalize(const gt::HeadCall& c, const gt::HeadSums& o, int nblk, int K, hipStream_t s);
int launch_d_head(const gt::HeadArgs& a, hipStream_t s);
int launch_d_head_objective(const gt::HeadArgs& a, int nblk, hipStream_t s);      // (eng_gan_objective.hip) the head pass alone, objectives 1 .. 6
int launch_d_head_fdiv(const gt::HeadArgs& a, int nblk, hipStream_t s);           // (eng_gan_fdiv.hip) objectives 4 .. 6, reached through launch_d_head_objective
int launch_dstack_pass(const gt::DStackCall& k, hipStream_t s);
gt::DropoutSpec no_drop();
int launch_gemm(int kind, const gt::GemmArgs& g, int prec, hipStream_t s);      // GEMM_NT / GEMM_NN, tiles chosen from the shape
// C [M][N] (+)= A [M][K] . B^T (GEMM_NT: B [N][K]) or A . B (GEMM_NN: B [K][N]): no bias, activation or dropout
int plain_product(int kind, const float* A, int lda, const float* B, int ldb, float* C, int ldc, long M, int N, int K, bool accumulate, int prec,
                  hipStream_t s);
// Y (+)= act(X W^T + b [+ addm[r mod addm_wrap]]): addm, the split first layer's added matrix (forward of [x | adv] as two products)
int linear_forward(const float* X, int ldx, const float* W, int ldw, const float* b, float* Y, int ldy, long rows, int in, int out, int act,
                   const gt::DropoutSpec& drop, int prec, hipStream_t s, const float* addm = nullptr, int ld_addm = 0, long addm_wrap = 0,
                   bool accumulate = false);
int linear_forward_seg(const float* x, int ldx, long wrap, int cd, const float* adv, int ld_adv, long rows, const float* W, int ldw, int in,
                       const float* b, float* Y, int ldy, int out, int act, const gt::DropoutSpec& drop, int prec, hipStream_t s);
gt::GemmArgs backward_data_args(const float* dZ, int lddz, const float* W, int ldw, int col0, float* dX, int lddx,
                                long rows, int out, int ncols, int act_prev, const float* H, int ldh, const gt::DropoutSpec& drop);
int linear_backward_data(const float* dZ, int lddz, const float* W, int ldw, int col0, float* dX, int lddx,
                         long rows, int out, int ncols, int act_prev, const float* H, int ldh, const gt::DropoutSpec& drop, int prec, hipStream_t s);
// the weight-gradient slab protocol of both product families: slab_place decides where the partial slabs of one dW go (the pool of an
// active `defer`, flushed first when it is full or dW accumulates; else `slabs`), slab_combine records or launches their fixed-order sum
struct SlabSet {
  float* base; float* bias;      // [nslab][stride] product slabs, [nslab][out] bias slabs behind them
  long stride; size_t bytes;     // out * in; bytes of both slab sets
  int nslab, out;
  bool can4;                     // 16-byte combine (a recorded SlabJob or slab_reduce4_kernel)
  SlabDefer* defer;              // where the combine is recorded, or null: launched by slab_combine
};
int slab_defer_flush(SlabDefer& d, hipStream_t s);
int slab_place(SlabDefer* defer, Scratch& slabs, int nslab, int out, int in, const float* dW, bool accumulate, hipStream_t s, SlabSet* set);
int slab_combine(const SlabSet& set, float* dW, float* db, bool accumulate, hipStream_t s);
int linear_backward_weight(const float* dZ, int lddz, const float* X, int ldx, long rows, int out, int in,
                           float* dW, float* db, bool accumulate, Scratch& slabs, Scratch& colp, int prec, hipStream_t s,
                           SlabDefer* defer = nullptr, const gt::GemmArgs* ride_along = nullptr, bool* rode = nullptr);
int linear_backward_weight_split(const float* dZ, int lddz, long rows, long wrap, const float* xp, int ldxp, int cd,
                                 const float* adv, int ld_adv, int Da, int out, float* dW, float* db, bool accumulate,
                                 Scratch& slabs, int prec, hipStream_t s, SlabDefer* defer, const GemmArgs* rider = nullptr, bool* rode = nullptr);

// ------------------------------------------------------------------------------------------
// eng_gemm_b16.hip
// ------------------------------------------------------------------------------------------
gt::GemmB16Args b16_args();
// gt_gemm_b16_path_counts: launches of the family by kernel, counted on the host where they are issued (slot layout in gantts_hip.h)
enum { B16_PATH_CAST_F32 = 60, B16_PATH_CAST_BF16 = 61, B16_PATH_CAST_SEQDROP = 62, B16_PATH_CAST_MULTI = 63, B16_PATH_CAST_CAT = 64,
       B16_PATH_CAST_CATDROP = 65 };
static_assert(B16_PATH_CAST_CATDROP + 1 == GT_GEMM_B16_PATH_SLOTS, "gt_gemm_b16_path_counts slots");
constexpr int b16_path_slot(int epi, int amode, int form) { return (epi * 5 + amode) * 4 + form; }
void b16_path_count(int slot);
int launch_gemm_b16(const gt::GemmB16Args& g, int nslab, hipStream_t s, int tile = 0);
// [rows][ld_in] float32 / bf16 -> bf16 [rows][ldo] and / or its transpose [cols][ldt] (+ per-column sums -> colsum)
int cast_transpose(const float* in, int ld_in, long rows, int cols, __bf16* out, int ldo, __bf16* outT, long ldt,
                   float* colsum, bool colsum_accumulate, Scratch* colp, hipStream_t s);
int cast_transpose(const __bf16* in, int ld_in, long rows, int cols, __bf16* out, int ldo, __bf16* outT, long ldt,
                   float* colsum, bool colsum_accumulate, Scratch* colp, hipStream_t s);
int cast_jobs_add(gt::CastJobs& jobs, int& blocks, const float* in, int ldi, long rows, int cols, __bf16* out, int ldo, __bf16* outT, long ldt);
int cast_transpose_multi(const gt::CastJobs& jobs, int blocks, hipStream_t s);
int seqdrop_cast_transpose(const gt::SeqDropSrc& src, long rows, int cols, __bf16* out, int ldo, __bf16* outT, long ldt, hipStream_t s);
int cat_cast_transpose(const gt::CatSrc& src, long rows, int cols, __bf16* out, int ldo, __bf16* outT, long ldt, hipStream_t s);
int catdrop_cast_transpose(const gt::CatDropSrc& src, long rows, int cols, __bf16* out, int ldo, __bf16* outT, long ldt, hipStream_t s);
int weight_grad_b16(const __bf16* dZT, long lddzt, const __bf16* XT, long ldxt, long rows, int out, int in, float* dW, float* db,
                    bool accumulate, Scratch& slabs, hipStream_t s, SlabDefer* defer = nullptr);
// the float32 matrix W (out, in) into rows [r0, r0 + out) of sh.w and columns [r0, r0 + out) of sh.wt (sh sized by LinShadow::ensure)
int shadow_cast(LinShadow& sh, const float* W, int r0, int out, int in, hipStream_t s);
// where a product of the family leaves its result: a float32 matrix (+= when accumulate), or an image, with its transposed twin when asked
struct B16Dst {
  float* C = nullptr; int ldc = 0; B16Img* img = nullptr; bool twin = false, accumulate = false;
  B16Dst(float* C_, int ldc_, bool accumulate_ = false) : C(C_), ldc(ldc_), accumulate(accumulate_) {}
  B16Dst(B16Img& img_, bool twin_) : img(&img_), twin(twin_) {}
};
// The two product shapes of the stacks, one launch each (launch_gemm_b16(g, 1, s)); W [n][ldw]: a shadow's w or wt, from whichever row.
//   forward:        dst [rows][n] = act(X [rows][k] . W^T + bias), dropout site `drop` under ACT_LEAKY_DROPOUT
//   backward-data:  dst [rows][n] = (dZ [rows][k] . W^T) (.) f'(H), f' and `drop` of the layer that produced H (act_prev == ACT_NONE: H is null)
int b16_forward(const __bf16* X, int ldx, long rows, const __bf16* W, int ldw, int n, int k, const float* bias, int act,
                const gt::DropoutSpec& drop, const B16Dst& dst, hipStream_t s);
int b16_backward_data(const __bf16* dZ, int lddz, long rows, const __bf16* W, int ldw, int n, int k, int act_prev, const B16Img* H,
                      const gt::DropoutSpec& drop, const B16Dst& dst, hipStream_t s);

// eng_mlpg.hip: a launch takes the band it goes through, as ensure_band handed it back
int ensure_band(gt_engine* e, const float* R, int T, hipStream_t s, const MlpgBand** out);
int mlpg_forward(gt_engine* e, const float* y, int ldy, const int* scol, const int* sstride, int Ds,
                 float* ys, int ldys, int B, int T, const MlpgBand& band, hipStream_t s);
int mlpg_backward(gt_engine* e, const float* gs, int ldgs, const int* scol, const int* sstride, int Ds,
                  float* gy, int ldgy, int B, int T, float mse_w, const float* yhat, const float* ytgt, int ldt,
                  const float* mask, const MlpgBand& band, hipStream_t s);

// ------------------------------------------------------------------------------------------
// eng_step.hip
// ------------------------------------------------------------------------------------------
int cond_dim(gt_engine* e);
// The output layer (`last`: last_linear / hidden2out, + sigmoid iff last_sigmoid) of every stack and role, in either storage form.
// OutTop, the rows it reads.  float32: x / ld.  bf16 storage: img and sh, the shadow of `last`; img_ready: the image is written already (an MLP
// stack's top activation, a folded SRU scan's output), else the forward casts x / ld into it, with the transposed twin iff want_t.
struct OutTop { const float* x = nullptr; int ld = 0; B16Img* img = nullptr; const LinShadow* sh = nullptr; bool img_ready = false, want_t = false; };
// OutGrad, where d loss / d top goes (the buffer the stack below reads) and what it passes on the way.  act_prev = ACT_LEAKY_DROPOUT: times f'(top)
// at dropout site `drop` (an MLP's top hidden layer); ACT_NONE: as it is (recurrent stacks).  ride: the float32 product is offered to the weight
// gradient's launch as its rider and launched on its own only when it did not ride.
struct OutGrad { B16Dst to; int act_prev; gt::DropoutSpec drop; bool ride; };
int out_layer_forward(gt_engine* e, int role, const OutTop& top, long rows, float* out, hipStream_t s);
int out_layer_backward(gt_engine* e, int role, const float* gy, int ldgy, long rows, const OutTop& top, const OutGrad& dst, SlabDefer* defer,
                       hipStream_t s);

// ------------------------------------------------------------------------------------------
// eng_spectral_norm.hip -- the launch functions below are the one launch site of each kernel, shared by the step and the hooks
// gt_op_spectral_norm / gt_op_sn_project (eng_ops.hip); gt_sn_path_counts counts them on the host (slot layout in gantts_hip.h)
// ------------------------------------------------------------------------------------------
int sn_plan_build(const SnLayerDesc* layers, int n, long n_flat, SnPlan** out);      // checks the table: dims in [1, 512], ranges ascending inside [0, n_flat)
long sn_plan_sum_out(const SnPlan* p);
long sn_plan_sum_in(const SnPlan* p);
int sn_plan_partials(const SnPlan* p);                   // squared-norm partials launch_sn_project writes
size_t sn_plan_bytes(const SnPlan* p);                   // of the SnBufs
SnBufs sn_plan_bufs(const SnPlan* p, void* ws);
// W_eff (and sigma) from W; iterate: one power iteration, u and v advanced (3 launches); else the eval form from the stored u, v (2 launches)
int launch_sn_prepare(const SnPlan* p, const float* W, float* u, float* v, float* weff, const SnBufs& b, bool iterate, hipStream_t s);
// G (d loss / d W_eff, the flat gradient) -> d loss / d W in place (2 launches); norm_part: sn_plan_partials() squared-norm partials of all of G
int launch_sn_project(const SnPlan* p, float* G, const float* weff, const float* u, const float* v, const SnBufs& b, double* norm_part, hipStream_t s);
// the engine's: (re)points the discriminator's Lin::W, prepares W_eff at the head of a pass, projects in front of the optimizer step
void sn_point_weights(gt_engine* e);
int sn_rebind(gt_engine* e);                              // gt_bind_model(role D) with the feature on: the new network against the registered buffers
int sn_prepare_pass(gt_engine* e, hipStream_t s);         // no-op when the feature is off
int sn_project_grads(gt_engine* e, double* norm_part, int* n_partial, hipStream_t s);

// ------------------------------------------------------------------------------------------
// eng_grad_penalty.hip -- launch_grad_penalty / launch_gp_interp are the one launch site of each kernel, shared by the step and the hook
// gt_op_grad_penalty (eng_ops.hip); gt_gp_path_counts counts them on the host (slot layout in gantts_hip.h)
// ------------------------------------------------------------------------------------------
int gp_row_blocks(long rows);                             // workgroups of gp_row: GpCall::part holds two doubles for each
void gp_eps_keys(const gt_engine* e, uint32_t* key0, uint32_t* key1);      // Philox keys of the current step's eps draws
int launch_gp_interp(const float* real, const float* fake, int ldf, const int* idx, int na, const float* eps_in, uint32_t key0, uint32_t key1,
                     float* out, int ldo, int col0, long rows, float* eps_out, hipStream_t s);
int launch_grad_penalty(const GpCall& c, hipStream_t s);
int gp_refusals(const gt_engine* e);                      // no-op when the feature is off

// ------------------------------------------------------------------------------------------
// eng_comm.hip
// ------------------------------------------------------------------------------------------
struct GtComm {
  void* comm = nullptr;
  int rank = 0, world = 1;
  hipStream_t stream = nullptr;
  Event ev[8];
  int next_ev = 0;
  Event ev_done;
  // schedule trace (gt_comm_trace, a measurement): every message and every join of the step stream bracketed by timed events
  struct TraceRec { int kind, inl; double bytes; Event e0, e1; bool closed; };     // kind 0 message, 1 join; closed: e1 was recorded
  bool trace = false;
  long trace_dropped = 0;                          // messages / joins that found the trace full
  std::vector<TraceRec> trec;
};
bool comm_on(const gt_engine* e);
int comm_grads_ready(gt_engine* e, int role, const float* lo, long count, hipStream_t compute);
int comm_flush(gt_engine* e, int role, hipStream_t compute, bool closing = false);
// eng_ipc.hip
void ipc_destroy(gt_engine* e);
bool ipc_usable(const gt_engine* e, size_t bytes);
int ipc_allreduce(gt_engine* e, void* buf, size_t count, bool dtype_double, hipStream_t s);
int comm_finish_step(gt_engine* e, int role, bool grads, double* sums, int n_sums, hipStream_t compute);
int comm_early_results(gt_engine* e, int role, double* sums, int n_sums, float adv_w, float mse_w, float mge_w, hipStream_t compute);
// (LossNormaliser::start / send / join / file / ensure are defined there too, next to the collectives they use)
// (the data-parallel schedule switches are per-engine state: gt_engine::opt_comm_*)

// ------------------------------------------------------------------------------------------
// eng_lstm.hip / eng_sru.hip
// ------------------------------------------------------------------------------------------
int lstm_forward(gt_engine* e, const float* x, int B, int T, float* y_hat, hipStream_t s);
int lstm_check_lengths(gt_engine* e, int B, int T);
int lstm_stack_forward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, hipStream_t s,
                       const float** top, int* ld_top);
int lstm_stack_backward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, bool want_w,
                        float* dx0, hipStream_t s);
int lstm_backward(gt_engine* e, const float* x, const float* gy, int B, int T, hipStream_t s);
int sru_forward(gt_engine* e, const float* x, int B, int T, float* y_hat, hipStream_t s);
int sru_backward(gt_engine* e, const float* x, const float* gy, int B, int T, hipStream_t s);
// cat0 (a discriminator on the bf16 path): layer 0's input images are written straight from [x | feats[:, idx]] (x may then be null
// unless layer 0 has k == 3: its scan reads the float32 rows as x').  want_w = false: no transposed images (no weight gradients follow).
int sru_stack_forward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, hipStream_t s,
                      const float** top, int* ld_top, const gt::CatSrc* cat0 = nullptr, bool want_w = true);
bool sru_b16(const gt_engine* e, int role);
// gt_sru_path_counts: launches of the SRU scans and their helper kernels by kernel, counted on the host where they are issued (slot
// layout in gantts_hip.h).  sru_launch_*: the one launch site of each kernel, shared by the stacks and the parity hooks (eng_ops.hip);
// sru_scan_waves: the form sru_launch_fwd / _bwd pick for a shape under the current knobs (0 sequential, 4 / 8 waves per 64 columns).
enum { SRU_PATH_FWD = 0, SRU_PATH_FWD_CS = 1, SRU_PATH_BWD = 5, SRU_PATH_BWD_CS = 6, SRU_PATH_INPUT_MASK = 10, SRU_PATH_INPUT_DROPOUT = 11,
       SRU_PATH_DX_ADV_FINISH = 12 };
static_assert(SRU_PATH_DX_ADV_FINISH + 1 == GT_SRU_PATH_SLOTS, "gt_sru_path_counts slots");
int sru_scan_waves(long B, int ncols);
uint32_t sru_drop_thresh(float p);
int sru_launch_fwd(const gt::SruArgs& a, hipStream_t s);
int sru_launch_bwd(const gt::SruArgs& a, hipStream_t s);
int sru_launch_input_mask(float* mul, int B, int n, float keep_scale, uint32_t thresh, uint32_t key0, uint32_t key1, const float* inj,
                          int seq_mul, int seq_add, hipStream_t s);
int sru_launch_input_dropout(const float* x, int ldx, float* y, int ldy, int B, int T, int n, const float* mul, hipStream_t s);
int sru_launch_dx_adv_finish(const gt::SruDxAdvArgs& f, hipStream_t s);
bool sru_d_needs_f32_input(const gt_engine* e);
int sru_stack_backward(gt_engine* e, int role, const float* x, int ld_x, int nseq, int T, const int* passes, int npass, bool want_w,
                       float* dx_adv, hipStream_t s);
