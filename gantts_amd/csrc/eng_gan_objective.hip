// libgantts_hip.so -- the discriminator's tail under the adversarial objectives 1 .. 3 (gan_objective.hip.h: least squares, hinge,
// Wasserstein): every form of d_head_kernel and both widths of dstack_kernel, instantiated here so that they build beside the
// objective-0 instantiations of eng_step.hip / eng_dstack.hip instead of behind them.  Same launch templates (d_tail_launch.hip.h).
// The f-GAN divergences 4 .. 6 are instantiated in eng_gan_fdiv.hip, a unit of their own again; the two entry points here forward them.
#include "d_tail_launch.hip.h"

using namespace gt;

int launch_d_head_objective(const HeadArgs& a, int nblk, hipStream_t s) {
  switch (a.c.objective) {
    case GAN_OBJ_LS: return head_launch_by_k<GAN_OBJ_LS>(a, nblk, s);
    case GAN_OBJ_HINGE: return head_launch_by_k<GAN_OBJ_HINGE>(a, nblk, s);
    case GAN_OBJ_WGAN: return head_launch_by_k<GAN_OBJ_WGAN>(a, nblk, s);
    case GAN_OBJ_KL: case GAN_OBJ_RKL: case GAN_OBJ_JS: return launch_d_head_fdiv(a, nblk, s);      // eng_gan_fdiv.hip
  }
  return fail(GT_ERR_INVALID, "discriminator head: unknown adversarial objective %d (0 bce, 1 ls, 2 hinge, 3 wgan, 4 kl, 5 rkl, 6 js)", a.c.objective);
}

int launch_dstack_objective(const DStackArgs& a, int hidden_dim, int objective, hipStream_t s) {
  switch (objective) {
    case GAN_OBJ_LS: return launch_dstack_by_width<GAN_OBJ_LS>(a, hidden_dim, s);
    case GAN_OBJ_HINGE: return launch_dstack_by_width<GAN_OBJ_HINGE>(a, hidden_dim, s);
    case GAN_OBJ_WGAN: return launch_dstack_by_width<GAN_OBJ_WGAN>(a, hidden_dim, s);
    case GAN_OBJ_KL: case GAN_OBJ_RKL: case GAN_OBJ_JS: return launch_dstack_fdiv(a, hidden_dim, objective, s);      // eng_gan_fdiv.hip
  }
  return fail(GT_ERR_INVALID, "fused discriminator stack: unknown adversarial objective %d (0 bce, 1 ls, 2 hinge, 3 wgan, 4 kl, 5 rkl, 6 js)", objective);
}
