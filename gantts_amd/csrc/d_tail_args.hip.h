// Argument blocks of the discriminator's tail -- the per-layer head (d_head_kernel), the fused stack (dstack_kernel) and the launch that
// finalises either one's partials (d_head_finalize_kernel): shared by the launch functions of eng_step.hip, the engine's wrappers around
// them and the parity hooks of eng_ops.hip.  Nothing here knows the engine: every buffer is a pointer with its capacity.
#pragma once
#include "dstack_f32.hip.h"

namespace gt {

// What the discriminator's head is asked for: shared by the per-layer head (launch_d_head) and the fused stack (launch_dstack_pass).
// Zero-initialise, then set by name.
struct HeadCall {
  int mode;                    // HEAD_D_STEP: rows = natural then generated; HEAD_G_ADV: generated rows only
  long rows, n_real;
  const float* mask; long n_mask;
  float eps;
  bool want_grad;              // seed the backward pass (phase == "train")
  bool want_w;                 // ... with weight gradients: d last_linear is reduced from the partials
  StepResults* early_res;      // the finalising launch also writes the step's results here
  int* defer_scalars;          // HEAD_G_ADV without weight gradients: the caller reduces the partials; <- their count
  const double* tv_dev;        // the valid-frame count when it is not in the step's scalars yet
  unsigned ticket;             // early_res in host memory: the ticket that announces it
  bool unit_tv;                // seed the backward pass of the UNNORMALISED loss (GT_OPT_COMM_TV_IN_SUMS)
  int objective;               // GanObjective (gan_objective.hip.h): 0 the reference's sigmoid + log loss, 1 ls, 2 hinge, 3 wgan, 4 kl, 5 rkl, 6 js
};

// Where a pass leaves its per-workgroup partials and where the finalising launch puts their sums.
struct HeadSums {
  StepScalars* sc;             // the step's scalars: inv_tv is read here (unless tv_dev / unit_tv), the sums land here
  HeadPartials* hp; long hp_cap;           // one per workgroup of the pass; capacity in entries
  float* dw_partial; long dw_cap;          // [workgroups][K] partial d last_linear.weight; capacity in floats
  float* dW; float* db;        // d last_linear (written when want_grad && want_w)
  int accumulate;              // ... added to what is there
  unsigned* ticket_dev;        // where HeadCall::ticket is published (early_res in host memory)
};

// launch_d_head: one per-layer head pass + its finalising launch
struct HeadArgs {
  HeadCall c;
  HeadSums o;
  const void* H; int K;        // the top hidden activation, float32 [rows][ldh] ...
  int ldh;
  int h_ld;                    // ... or (h_ld > 0) its bf16 image with row pitch h_ld
  bool has_act;                // H is LeakyReLU + dropout of a pre-activation (MLP); false: a recurrent stack's output
  DropoutSpec spec;            // the top layer's dropout site
  const float* w; const float* bias;       // last_linear: [K], [1]
  float* Dout;                 // D(x) per row, or null
  float* dH; int lddh;         // float32 seed gradient [rows][lddh], or null
  __bf16* dHb; int lddhb;      // (bf16 image form) the top dZ image [rows][lddhb], or null
  __bf16* dHbT; long lddhbt;   // ... and its transposed twin [K][lddhbt], or null
};

// launch_dstack_pass: one fused pass + its finalising launch.  Of `a` the caller fills the operands (H0, W, b, drop, w_last, b_last, W0,
// ldw0, col0, Da) and the results (Hout, dZtop, Dout, gadv, ld_gadv); everything HeadCall / HeadSums say is copied in by the launch function.
struct DStackCall {
  HeadCall c;
  HeadSums o;
  int hidden_dim;
  DStackArgs a;
};

// workgroups (= partials) of a pass over `rows` frames
inline int d_head_blocks(long rows) { const long n = (rows + 31) / 32; return (int)(n < 1024 ? n : 1024); }

}  // namespace gt
