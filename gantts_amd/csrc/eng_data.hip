// libgantts_hip.so -- the data path's stand-alone operators: gt_op_assemble_batch (one training batch out of a device-resident corpus),
// gt_op_assemble_shard (one data-parallel rank's share of it)
// and gt_op_corpus_stats (the normalisation statistics of one side of that corpus)
#include "engine_internal.hip.h"
#include "data_kernels.hip.h"
#include "corpus_stats_kernels.hip.h"

using namespace gt;

static_assert(ASM_MAX_WINDOWS == GT_ASSEMBLE_MAX_WINDOWS && ASM_MAX_TAPS == GT_ASSEMBLE_MAX_TAPS, "window table of the kernel and of the ABI");
static_assert(CS_SLAB == GT_CORPUS_STATS_SLAB && CS_FANIN == GT_CORPUS_STATS_FANIN, "slab and fan-in of the kernels and of the ABI");

template <typename SX, typename SY, bool DELTA>
static int launch_assemble(const AssembleArgs& a, hipStream_t s) {
  const size_t lds = assemble_lds_bytes(sizeof(SX), sizeof(SY), a.Dx, a.Dy, a.Ds, a.ldY, DELTA);
  if (lds > 64 * 1024)
    return fail(GT_ERR_INVALID, "assemble_batch: statistics of %d + %d columns need %zu bytes of LDS (limit 65536)", a.Dx, a.Dy, lds);
  const long rows = (long)a.B * a.T;
  hipLaunchKernelGGL((assemble_batch_kernel<SX, SY, DELTA>), dim3(cdiv(rows, ASM_ROWS_PER_WG)), dim3(ASM_WAVES * 64), lds, s, a);
  LAUNCH_CHECK();
  return GT_OK;
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static bool aligned8(const void* p) { return ((uintptr_t)p & 7) == 0; }

// Both entry points: sh == null is gt_op_assemble_batch (slot stride 1, no tv_global), otherwise one rank's share of the batch.
static int assemble(const gt_assemble_case* c, const gt_assemble_shard* sh, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "assemble_batch: null case");
  if (!c->X_all || !c->Y_all || !c->table) return fail(GT_ERR_INVALID, "assemble_batch: null corpus or table");
  if (c->B < 1 || c->T < 1 || c->Dx < 1 || c->Dy < 1 || c->nz < 0 || c->Ds < 0 || c->F < 0)
    return fail(GT_ERR_INVALID, "assemble_batch: bad sizes B=%d T=%d Dx=%d Dy=%d nz=%d Ds=%d", c->B, c->T, c->Dx, c->Dy, c->nz, c->Ds);
  if ((long)c->B * c->T > (1L << 31) - 64) return fail(GT_ERR_INVALID, "assemble_batch: B * T = %ld rows", (long)c->B * c->T);
  if (c->ldX < c->Dx || c->ldY < c->Dy || c->ldX % 4 || c->ldY % 4 || !aligned16(c->X_all) || !aligned16(c->Y_all))
    return fail(GT_ERR_INVALID, "assemble_batch: the corpus rows must sit on a 16-byte pitch (ldX=%d for %d, ldY=%d for %d columns)", c->ldX,
                c->Dx, c->ldY, c->Dy);
  if (sh) {
    if (sh->world < 1 || sh->rank < 0 || sh->rank >= sh->world)
      return fail(GT_ERR_INVALID, "assemble_shard: rank %d of a world of %d", sh->rank, sh->world);
    if (sh->B_global < 1) return fail(GT_ERR_INVALID, "assemble_shard: B_global = %d", sh->B_global);
    const long share = sh->rank < sh->B_global ? ((long)sh->B_global - sh->rank + sh->world - 1) / sh->world : 0;
    if (share < 1 || c->B != share)
      return fail(GT_ERR_INVALID, "assemble_shard: rank %d of %d holds %ld of %d sequences, the case has B = %d", sh->rank, sh->world, share,
                  sh->B_global, c->B);
    if (!aligned8(sh->tv_global)) return fail(GT_ERR_INVALID, "assemble_shard: tv_global must be 8-byte aligned");
  }
  const long n_seq = sh ? sh->B_global : c->B;      // the slots of the whole batch
  if (c->first_slot < 0 || c->n_slots < 0 || c->first_slot > c->n_slots - n_seq)      // (n_seq >= 1: no overflow)
    return fail(GT_ERR_INVALID, "assemble_batch: slots [%lld, %lld) of a table of %lld", (long long)c->first_slot,
                (long long)((unsigned long long)c->first_slot + (unsigned long long)n_seq), (long long)c->n_slots);
  for (int k = 0; k < 2; ++k) {
    const int kind = k ? c->y_kind : c->x_kind;
    if (kind < GT_SCALE_NONE || kind > GT_SCALE_MEANVAR) return fail(GT_ERR_INVALID, "assemble_batch: unknown scaling kind %d", kind);
    if (kind != GT_SCALE_NONE && (!(k ? c->y_a : c->x_a) || !(k ? c->y_b : c->x_b))) return fail(GT_ERR_INVALID, "assemble_batch: null statistics");
  }
  if (c->stats_f64 < 0 || c->stats_f64 > 3) return fail(GT_ERR_INVALID, "assemble_batch: stats_f64 is a mask of bits 1 (x) and 2 (y)");
  if (c->gi && (c->ld_gi < c->Dx + c->nz || c->ld_gi % 4 || !aligned16(c->gi)))
    return fail(GT_ERR_INVALID, "assemble_batch: gi needs a 16-byte aligned pitch of at least %d floats, got %d", c->Dx + c->nz, c->ld_gi);
  // the Philox counter of a frame is t * ceil(nz / 4) + group: one 32-bit word
  if (c->nz > 0 && (long)c->T * ((c->nz + 3) / 4) > 0xFFFFFFFFL) return fail(GT_ERR_INVALID, "assemble_batch: T * ceil(nz / 4) exceeds 32 bits");
  if (c->y && c->ld_y < c->Dy) return fail(GT_ERR_INVALID, "assemble_batch: ld_y %d for %d columns", c->ld_y, c->Dy);
  if (c->y_static && (c->ld_ys < c->Ds || (c->Ds > 0 && !c->scol))) return fail(GT_ERR_INVALID, "assemble_batch: y_static needs scol and ld_ys >= Ds");
  const bool delta = c->dsrc || c->dwin;
  if (delta) {
    if (!c->dsrc || !c->dwin || c->n_windows < 1 || c->n_windows > GT_ASSEMBLE_MAX_WINDOWS)
      return fail(GT_ERR_INVALID, "assemble_batch: delta recomputation needs dsrc, dwin and 1..%d windows", GT_ASSEMBLE_MAX_WINDOWS);
    for (int w = 0; w < c->n_windows; ++w)
      if (c->win_len[w] < 1 || c->win_len[w] > GT_ASSEMBLE_MAX_TAPS || c->win_len[w] % 2 == 0)
        return fail(GT_ERR_INVALID, "assemble_batch: window %d has %d taps (odd, at most %d)", w, c->win_len[w], GT_ASSEMBLE_MAX_TAPS);
  }
  AssembleArgs a;
  memset(&a, 0, sizeof(a));
  a.B = c->B; a.T = c->T; a.Dx = c->Dx; a.Dy = c->Dy; a.nz = c->nz; a.Ds = c->y_static ? c->Ds : 0;
  a.ldX = c->ldX; a.ldY = c->ldY; a.ld_gi = c->ld_gi; a.ld_y = c->ld_y; a.ld_ys = c->ld_ys;
  a.x_kind = c->x_kind; a.y_kind = c->y_kind; a.n_windows = delta ? c->n_windows : 0;
  a.key0 = c->key0; a.key1 = c->key1;
  a.F = c->F; a.first_slot = c->first_slot + (sh ? sh->rank : 0); a.slot_stride = sh ? sh->world : 1;
  a.tv_first = c->first_slot; a.tv_count = (int)n_seq; a.tv_global = sh ? sh->tv_global : nullptr;
  a.X_all = c->X_all; a.Y_all = c->Y_all;
  a.x_a = c->x_a; a.x_b = c->x_b; a.y_a = c->y_a; a.y_b = c->y_b;
  a.table = (const long*)c->table;
  a.scol = c->scol; a.dsrc = c->dsrc; a.dwin = c->dwin;
  a.gi = c->gi; a.y = c->y; a.y_static = c->y_static; a.mask = c->mask; a.lengths = (long*)c->lengths;
  for (int w = 0; w < a.n_windows; ++w) {
    a.win_len[w] = c->win_len[w];
    for (int k = 0; k < c->win_len[w]; ++k) a.coef[w][k] = c->coef[w][k];
  }
  hipStream_t s = (hipStream_t)stream;
  switch ((c->stats_f64 & 3) * 2 + (delta ? 1 : 0)) {
    case 0: return launch_assemble<float, float, false>(a, s);
    case 1: return launch_assemble<float, float, true>(a, s);
    case 2: return launch_assemble<double, float, false>(a, s);
    case 3: return launch_assemble<double, float, true>(a, s);
    case 4: return launch_assemble<float, double, false>(a, s);
    case 5: return launch_assemble<float, double, true>(a, s);
    case 6: return launch_assemble<double, double, false>(a, s);
    default: return launch_assemble<double, double, true>(a, s);
  }
}

extern "C" int gt_op_assemble_batch(const gt_assemble_case* c, void* stream) { return assemble(c, nullptr, stream); }

extern "C" int gt_op_assemble_shard(const gt_assemble_case* c, const gt_assemble_shard* s, void* stream) {
  if (!s) return fail(GT_ERR_INVALID, "assemble_shard: null shard");
  return assemble(c, s, stream);
}

extern "C" int64_t gt_corpus_stats_workspace_bytes(int64_t F, int32_t D) {
  if (F < 0 || D < 1) return 0;
  const size_t n = corpus_stats_ws_bytes(F, (D + 3) / 4 * 4);
  return (int64_t)(n ? n : 16);
}

extern "C" int gt_op_corpus_stats(const gt_corpus_stats_case* c, void* stream) {
  if (!c) return fail(GT_ERR_INVALID, "corpus_stats: null case");
  if (c->D < 1 || c->F < 0 || c->n_seg < 0 || c->prior_count < 0)
    return fail(GT_ERR_INVALID, "corpus_stats: bad sizes D=%d F=%lld n_seg=%lld prior_count=%lld", c->D, (long long)c->F, (long long)c->n_seg,
                (long long)c->prior_count);
  if (c->ld != (c->D + 3) / 4 * 4 || (c->F > 0 && (!c->A || !aligned16(c->A))))
    return fail(GT_ERR_INVALID, "corpus_stats: the corpus rows must sit on the 16-byte pitch roundup(D, 4) (ld=%d for %d columns)", c->ld, c->D);
  if (c->n_seg > 0 && !c->seg) return fail(GT_ERR_INVALID, "corpus_stats: null segment table");
  if (!c->out_min || !c->out_max || !c->out_count || !c->out_mean || !c->out_m2) return fail(GT_ERR_INVALID, "corpus_stats: null result");
  const long n_part = corpus_stats_parts(c->F);
  if (n_part > (1L << 31) - 1) return fail(GT_ERR_INVALID, "corpus_stats: F = %lld rows", (long long)c->F);
  const size_t need = corpus_stats_ws_bytes(c->F, c->ld);
  if (need && (!c->workspace || !aligned16(c->workspace) || c->workspace_bytes < (int64_t)need))
    return fail(GT_ERR_INVALID, "corpus_stats: a 16-byte aligned workspace of %zu bytes is needed (gt_corpus_stats_workspace_bytes), got %lld", need,
                (long long)c->workspace_bytes);
  CorpusStatsArgs a;
  memset(&a, 0, sizeof(a));
  a.D = c->D; a.ld = c->ld;
  while ((1 << a.lpr_log2) < (a.ld >> 2) && a.lpr_log2 < 6) ++a.lpr_log2;
  a.F = c->F; a.n_seg = c->n_seg; a.n_part = n_part;
  a.prior_count = (double)c->prior_count;
  a.A = c->A; a.seg = (const long*)c->seg;
  a.prior_mean = c->prior_mean; a.prior_var = c->prior_var;
  a.part_d = (double*)c->workspace;
  a.part_f = (float*)((char*)c->workspace + (size_t)n_part * 3 * a.ld * sizeof(double));
  a.out_min = c->out_min; a.out_max = c->out_max; a.out_count = c->out_count; a.out_mean = c->out_mean; a.out_m2 = c->out_m2;
  hipStream_t s = (hipStream_t)stream;
  if (n_part > 0) {
    hipLaunchKernelGGL(corpus_stats_slab_kernel, dim3((unsigned)n_part), dim3(CS_THREADS), 0, s, a);
    LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(corpus_stats_merge_kernel, dim3(cdiv(a.D, CS_MERGE_COLS)), dim3(CS_MERGE_THREADS), 0, s, a);
  LAUNCH_CHECK();
  return GT_OK;
}
