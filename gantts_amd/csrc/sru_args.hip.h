// Argument blocks of the SRU scan kernels (sru_kernels.hip.h, sru_cs_kernels.hip.h) and of the discriminator's dx finish: shared by the
// kernels, the launch functions of eng_sru.hip and the parity hooks of eng_ops.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gt {

enum SruAct { SRU_ID = 0, SRU_TANH = 1, SRU_RELU = 2 };

struct SruArgs {
  int B, T, H, dirs, k, act;
  const float* U; int ldu;        // [N][ncols*k], row = b*T + t
  const float* x; int ldx;        // layer input (highway term when k == 3)
  const float* bias;              // [2*ncols] = b_f | b_r
  float* h;                       // [N][ncols]
  float* c;                       // [N][ncols] cell-state stash
  // backward
  const float* dh;                // [N][ncols]
  float* dU;                      // [N][ncols*k]
  float* dx; int lddx;            // k == 3: highway gradient d/dx' -> [N][ncols]
  float* dbias_part;              // [B][2*ncols]
  // variational output dropout (one mask per (sequence, column), shared over time)
  int use_mask; float keep_scale; uint32_t thresh, key0, key1;
  int seq_mul, seq_add;           // data parallel: local sequence b is sequence seq_add + seq_mul * b of the whole minibatch (1, 0 on one rank)
  const float* mask_buf;          // parity hook: injected 0/1 keep mask [B][ncols] instead of the Philox stream
  // backward only: this layer's output is the NEXT layer's input, and that layer's variational input dropout (+ its k == 3
  // highway gradient) is applied here, where the gradient is read: dh = g * up_mul[b][col] + up_add.  The multiplier is
  // constant per lane (one (sequence, column) pair per lane).
  // backward, GT_OPT_MATMUL_BF16 with the cooperative scans (T % 8 == 0, H % 64 == 0, B * ncols % 64 == 0): dU leaves the scan as the two
  // bf16 images the products read (row-major [N][ld_dub], transposed [ncols*k][ld_dubt]) instead of float32 + a cast pass
  __bf16* dU_b; int ld_dub;
  __bf16* dU_bt; long ld_dubt;    // (null: not written -- the generator step's pass through a discriminator forms no weight gradient)
  // forward, GT_OPT_MATMUL_BF16 with the cooperative scans (T % 8 == 0, H % 64 == 0, B * ncols % 64 == 0): the scan writes the bf16
  // images of the NEXT product's input (the next SRU layer's dropped input, or hidden2out's input) itself -- row-major [N][ld_nxb] and,
  // when the backward pass will want it, transposed [ncols][ld_nxbt] -- value h * nx_mul[b][col] rounded as the cast pass rounds it
  __bf16* nx_b; int ld_nxb;
  __bf16* nx_bt; long ld_nxbt;
  const float* nx_mul;            // [B][ncols] multipliers of the next layer's variational input dropout, or null (1)
  const float* up_mul;            // [B][ncols] multipliers {0, 1/(1-p)} of the next layer's input dropout, or null
  const float* up_add; int ld_up_add;   // [N][ncols] highway gradient of the next layer (k == 3), or null
};

// sru_dx_adv_finish_kernel (sru_kernels.hip.h)
struct SruDxAdvArgs {
  float* dx_adv; long rows; int Da, T;
  const float* mul; int ld_mul;
  const float* hw; int ld_hw;
};

}  // namespace gt
