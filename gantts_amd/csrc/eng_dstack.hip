// libgantts_hip.so -- launcher of the fused discriminator stack (dstack_f32.hip.h): one launch per discriminator pass for the
// hidden layers above the first one + the head (+ the backward-data chain of the generator step's adversarial term).
#include "d_tail_launch.hip.h"

using namespace gt;

bool dstack_hidden_ok(int hidden_dim) { return hidden_dim == 128 || hidden_dim == 256; }

// panels of the pass = workgroups = entries of a.hp (and rows of a.dw_partial)
int dstack_panels(long rows) { return cdiv(rows, DS_R); }

// objective: GanObjective of the head; 0 is instantiated here, 1 .. 3 in eng_gan_objective.hip, 4 .. 6 in eng_gan_fdiv.hip (d_tail_launch.hip.h holds the launch)
int launch_dstack(const DStackArgs& a, int hidden_dim, hipStream_t s, int objective) {
  if (a.L < 1 || a.L > DS_MAXL) return fail(GT_ERR_INVALID, "fused discriminator stack: 1 .. %d hidden layers", DS_MAXL);
  if (a.mode == DSTACK_G_ADV && a.want_grad && (a.Da < 1 || a.Da > 64)) return fail(GT_ERR_INVALID, "fused discriminator stack: 1 .. 64 adversarial columns");
  if (objective != GAN_OBJ_BCE) return launch_dstack_objective(a, hidden_dim, objective, s);
  return launch_dstack_by_width<GAN_OBJ_BCE>(a, hidden_dim, s);
}
