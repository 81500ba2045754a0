// libgantts_hip.so -- the discriminator's tail under the f-GAN divergences, the adversarial objectives 4 .. 6 (gan_objective.hip.h: KL,
// reverse KL, Jensen-Shannon): every form of d_head_kernel and both widths of dstack_kernel, instantiated here so that they build beside
// the instantiations of eng_step.hip / eng_dstack.hip (objective 0) and eng_gan_objective.hip (1 .. 3) instead of behind them.  Same
// launch templates (d_tail_launch.hip.h); eng_gan_objective.hip's two entry points forward the ids 4 .. 6 here.
#include "d_tail_launch.hip.h"

using namespace gt;

int launch_d_head_fdiv(const HeadArgs& a, int nblk, hipStream_t s) {
  switch (a.c.objective) {
    case GAN_OBJ_KL: return head_launch_by_k<GAN_OBJ_KL>(a, nblk, s);
    case GAN_OBJ_RKL: return head_launch_by_k<GAN_OBJ_RKL>(a, nblk, s);
    case GAN_OBJ_JS: return head_launch_by_k<GAN_OBJ_JS>(a, nblk, s);
  }
  return fail(GT_ERR_INVALID, "discriminator head: adversarial objective %d is no f-GAN divergence (4 kl, 5 rkl, 6 js)", a.c.objective);
}

int launch_dstack_fdiv(const DStackArgs& a, int hidden_dim, int objective, hipStream_t s) {
  switch (objective) {
    case GAN_OBJ_KL: return launch_dstack_by_width<GAN_OBJ_KL>(a, hidden_dim, s);
    case GAN_OBJ_RKL: return launch_dstack_by_width<GAN_OBJ_RKL>(a, hidden_dim, s);
    case GAN_OBJ_JS: return launch_dstack_by_width<GAN_OBJ_JS>(a, hidden_dim, s);
  }
  return fail(GT_ERR_INVALID, "fused discriminator stack: adversarial objective %d is no f-GAN divergence (4 kl, 5 rkl, 6 js)", objective);
}
