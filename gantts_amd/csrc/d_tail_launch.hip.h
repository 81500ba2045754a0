// The launches of d_head_kernel and dstack_kernel, templated on the adversarial objective (gan_objective.hip.h): included by eng_step.hip
// and eng_dstack.hip for objective 0 and by eng_gan_objective.hip for the objectives 1 .. 3 and eng_gan_fdiv.hip for 4 .. 6, so that the groups of instantiations
// build in parallel and share one dispatch.  gt_head_path_counts counts a launch in the slot of its FORM, whatever its objective.
#pragma once
#include "engine_internal.hip.h"
#include "d_tail_args.hip.h"

namespace gt {

template <int OBJ, int KP, typename TH, bool IMG, bool VEC = false>
static void head_launch(const HeadArgs& a, int nblk, hipStream_t s) {
  const HeadCall& c = a.c;
  hipLaunchKernelGGL((d_head_kernel<KP, TH, IMG, VEC, OBJ>), dim3(nblk), dim3(256), (size_t)4 * a.K * sizeof(float), s, (const TH*)a.H, IMG ? a.h_ld : a.ldh, a.K,
                     a.w, a.bias, c.mask, (int)c.n_mask, (int)c.n_real, (int)c.rows, c.mode, c.eps, a.Dout, a.dH, a.lddh,
                     c.want_grad ? 1 : 0, a.spec, a.has_act ? 1 : 0, a.o.sc, a.o.hp, a.o.dw_partial,
                     IMG ? a.dHb : (__bf16*)nullptr, IMG ? a.lddhb : 0, IMG ? a.dHbT : (__bf16*)nullptr, IMG ? a.lddhbt : 0L, c.tv_dev, c.unit_tv ? 1 : 0);
  constexpr int kp = KP == 2 ? 0 : KP == 4 ? 1 : KP == 8 ? 2 : 3;
  head_path_count(IMG ? HEAD_PATH_IMG + kp : VEC ? HEAD_PATH_VEC + kp - 1 : HEAD_PATH_F32 + kp);
}
template <int OBJ, int KP>
static void head_launch_k(const HeadArgs& a, int nblk, hipStream_t s) {
  if (a.h_ld > 0) head_launch<OBJ, KP, __bf16, true>(a, nblk, s);
  else if (KP % 4 == 0 && gt_tuning().head_vec) head_launch<OBJ, (KP % 4 == 0 ? KP : 4), float, false, true>(a, nblk, s);
  else head_launch<OBJ, KP, float, false>(a, nblk, s);
}
// the head pass alone (no finalising launch): the form follows from K, h_ld and the tuning knob head_vec
template <int OBJ>
static int head_launch_by_k(const HeadArgs& a, int nblk, hipStream_t s) {
  if (a.K <= 128) head_launch_k<OBJ, 2>(a, nblk, s);
  else if (a.K <= 256) head_launch_k<OBJ, 4>(a, nblk, s);
  else if (a.K <= 512) head_launch_k<OBJ, 8>(a, nblk, s);
  else if (a.K <= 1024) head_launch_k<OBJ, 16>(a, nblk, s);
  else return fail(GT_ERR_INVALID, "discriminator hidden_dim > 1024 is not supported by the fused head kernel");
  LAUNCH_CHECK();
  return GT_OK;
}

template <int HD, int OBJ>
static int launch_dstack_t(const DStackArgs& a, hipStream_t s) {
  const size_t lds = dstack_lds_bytes<HD>();
  CHK(ensure_dyn_lds((const void*)dstack_kernel<HD, OBJ>, lds));
  const int grid = cdiv(a.rows, DS_R);
  if (grid <= 0) return GT_OK;
  GemmProfiler::Rec rec;
  const bool prof = g_prof.wants(7);
  if (prof) {       // bench.py's per-kernel table: kind 7 = the fused discriminator stack (slot 14)
    const double both = a.mode == DSTACK_G_ADV && a.want_grad ? 2.0 : 1.0;
    rec.kind = 7; rec.bn = 64; rec.am = -1;
    rec.flops = 2.0 * a.rows * HD * HD * (a.L - 1) * both + (both > 1.0 ? 2.0 * a.rows * HD * a.Da : 0.0) + 2.0 * a.rows * HD;
    // algorithmic bytes: H0 once, the weights once, the D step's stashes (L - 1 activations + the seed gradient) once
    rec.bytes = 4.0 * ((double)a.rows * HD + (double)(a.L - 1) * HD * HD + (a.mode == DSTACK_D_STEP ? (double)a.L * a.rows * HD : (double)a.rows * a.Da));
    rec.e0 = g_prof.get(); rec.e1 = g_prof.get();
    HIPCHK(hipEventRecord(rec.e0, s));
  }
  hipLaunchKernelGGL((dstack_kernel<HD, OBJ>), dim3(grid), dim3(DS_THREADS), lds, s, a);
  LAUNCH_CHECK();
  head_path_count(HD == 128 ? HEAD_PATH_DSTACK128 : HEAD_PATH_DSTACK256);
  if (prof) { HIPCHK(hipEventRecord(rec.e1, s)); g_prof.recs.push_back(rec); }
  return GT_OK;
}
template <int OBJ>
static int launch_dstack_by_width(const DStackArgs& a, int hidden_dim, hipStream_t s) {
  if (hidden_dim == 256) return launch_dstack_t<256, OBJ>(a, s);
  if (hidden_dim == 128) return launch_dstack_t<128, OBJ>(a, s);
  return fail(GT_ERR_INVALID, "fused discriminator stack: hidden_dim 128 or 256");
}

}  // namespace gt
