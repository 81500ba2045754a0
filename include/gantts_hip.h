/* gantts_hip.h -- C ABI of the MI355X-native GAN training engine (libgantts_hip.so).
 *
 * Drop-in boundary for the G+D adversarial training step of r9y9/gantts.  Every entry point
 * cites the reference interface (file:line in the upstream tree) it stands in for; the Python
 * host package `gantts_amd` binds these with ctypes and re-exposes the reference's own Python
 * signatures.
 *
 * Conventions
 *  - plain C: opaque handle, raw device pointers (HIP, float32 unless noted), sizes; no C++/torch types.
 *  - every function returns 0 on success, non-zero on error; gt_last_error() gives the message
 *    (thread-local).  HIP errors are mapped to GT_ERR_HIP; the library never aborts.
 *  - all frame tensors are contiguous (B,T,D) row-major, feature dimension fastest
 *    (reference train.py:145-159).  A "row" is one frame; rows = B*T.
 *  - the caller owns inputs, outputs, parameters, gradients and optimizer state (so checkpoints
 *    stay torch.save-compatible, reference train.py:162-171); the engine borrows the pointers for
 *    the duration of a call and owns only its workspace (activation stash, slabs, scalars).
 *  - calls on one handle are not re-entrant; kernels are enqueued on the `stream` argument
 *    (a hipStream_t, may be NULL for the default stream); functions returning host scalars wait only
 *    for those scalars (an event after the loss kernels): the backward pass and the optimizer step of
 *    the same call may still be executing on the stream when the call returns -- stream order keeps
 *    every later call (and any reader on the same stream) correct.
 */
#ifndef GANTTS_HIP_H_
#define GANTTS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GT_OK 0
#define GT_ERR_INVALID 1      /* bad argument / unsupported configuration */
#define GT_ERR_HIP 2          /* HIP runtime error */
#define GT_ERR_STATE 3        /* call order violated (e.g. update_* before apply_generator) */
#define GT_ERR_DIM 4          /* "You probably have specified wrong dimention params." (multistream.py:93-94) */

#define GT_ROLE_G 0
#define GT_ROLE_D 1

#define GT_ARCH_MLP 0         /* gantts/models.py:121-141 */
#define GT_ARCH_IN2OUT 1      /* gantts/models.py:21-69  (In2OutHighwayNet) */
#define GT_ARCH_LSTM 2        /* gantts/models.py:170-213 (LSTMRNN, GRURNN: nn.LSTM + hidden2out) */
#define GT_ARCH_SRU 3         /* gantts/models.py:144-167 (SRURNN: third-party SRU cells + hidden2out) */
#define GT_ARCH_IN2OUT_RNN 4  /* gantts/models.py:72-118 (In2OutRNNHighwayNet: T gate | lstm.* | hidden2out.*) */

#define GT_OPT_ADAGRAD 0      /* torch.optim.Adagrad, train.py:796-799 with hparams.py:48-52,223-227 */
#define GT_OPT_ADAM 1         /* torch.optim.Adam,    hparams.py:125-130 */
/* the rest of the torch.optim names a reference script may put into hp.optimizer_g / hp.optimizer_d (gt_optim_desc_ex only) */
#define GT_OPT_SGD 2          /* torch.optim.SGD      (momentum, dampening, nesterov) */
#define GT_OPT_RMSPROP 3      /* torch.optim.RMSprop  (alpha, momentum, centered) */
#define GT_OPT_ADADELTA 4     /* torch.optim.Adadelta (rho) */
#define GT_OPT_ADAMW 5        /* torch.optim.AdamW == Adam(decoupled_weight_decay=True) */
#define GT_OPT_ADAMAX 6       /* torch.optim.Adamax */
/* (optimizer kinds are a namespace of their own: these numbers are unrelated to the gt_set_option ids further down) */
#define GT_OPT_NADAM  7       /* torch.optim.NAdam    (momentum_decay, decoupled_weight_decay) */
#define GT_OPT_RADAM  8       /* torch.optim.RAdam    (decoupled_weight_decay) */
#define GT_OPT_RPROP  9       /* torch.optim.Rprop    (etas, step_sizes) */
#define GT_OPT_ASGD   10      /* torch.optim.ASGD     (lambd, alpha, t0) */
/* gt_optim_desc_ex.flags */
#define GT_OPTF_NESTEROV 1u     /* SGD */
#define GT_OPTF_CENTERED 2u     /* RMSprop */
#define GT_OPTF_AMSGRAD 4u      /* Adam, AdamW */
#define GT_OPTF_BUFFER_LIVE 8u  /* SGD: momentum_buffer holds a value (a step was taken, or a checkpoint that has it was loaded) */
#define GT_OPTF_DECOUPLED_WD 32u /* NAdam, RAdam: decoupled_weight_decay=True (16u is taken inside the library) */

#define GT_MAX_STREAMS 8

typedef struct gt_engine gt_engine;

/* hp.* fields read on the step path (train.py:61, 233-241, 248, 254, 299, 304, 352-353). */
typedef struct {
  int32_t n_streams;
  int32_t stream_sizes[GT_MAX_STREAMS];          /* hp.stream_sizes (static+delta widths)        */
  int32_t has_dynamic_features[GT_MAX_STREAMS];  /* hp.has_dynamic_features                       */
  int32_t num_windows;                           /* len(hp.windows)                               */
  int32_t adversarial_streams[GT_MAX_STREAMS];   /* hp.adversarial_streams; [0] = -1 means None   */
  int32_t mask_nth_mgc_for_adv_loss;             /* hp.mask_nth_mgc_for_adv_loss                  */
  int32_t discriminator_linguistic_condition;    /* hp.discriminator_linguistic_condition         */
  int32_t cond_dim;                              /* width of x fed to D when conditioned (x, not cat(x,z): train.py:254-256) */
} gt_stream_config;

/* One network.  `params`/`grads` are flat float32 device buffers laid out in state_dict order:
 *   MLP:    layers.0.weight (hidden x in) | layers.0.bias | ... | last_linear.weight | last_linear.bias
 *   IN2OUT: T.weight (sd x sd) | T.bias | H.0.weight | H.0.bias | ... | last_linear.weight | last_linear.bias
 *   LSTM:   for layer k, for direction d (forward, then reverse when bidirectional):
 *             weight_ih (4H x in_k) | weight_hh (4H x H) | bias_ih (4H) | bias_hh (4H)     (gate order i,f,g,o)
 *           then hidden2out.weight (out x H*dirs) | hidden2out.bias        (torch.nn.LSTM parameter order)
 *   SRU:    for layer i: rnn_lst.i.weight (n_in x ncols*k, ncols = H*dirs, k = 3 if n_in == ncols else 4,
 *           column j owns entries j*k..j*k+k-1) | rnn_lst.i.bias (2*ncols = b_f | b_r);
 *           then hidden2out.weight (out x ncols) | hidden2out.bias
 * Linear / LSTM weights are (out, in) row-major exactly as torch stores them; SRU weights are (in, out). */
typedef struct {
  int32_t arch;
  int32_t in_dim, out_dim, num_hidden, hidden_dim;
  int32_t static_dim;        /* IN2OUT only */
  float dropout;
  int32_t last_sigmoid;
  int32_t bidirectional;     /* LSTM, SRU */
  int32_t use_relu;          /* SRU: g = relu (1) or tanh (0), models.py:152-154 */
  float rnn_dropout;         /* SRU: variational input dropout (training) */
  int32_t reserved_;
  float* params;
  float* grads;
  int64_t n_params;
} gt_model_desc;

typedef struct {
  int32_t kind;              /* GT_OPT_* */
  float lr, weight_decay, eps;
  float lr_decay;            /* Adagrad */
  float beta1, beta2;        /* Adam */
  float max_grad_norm;       /* clip_grad_norm_ threshold, 1.0 in train.py:275,317 */
  int64_t step;              /* number of steps already taken (restored from a checkpoint) */
  float* state0;             /* Adagrad "sum" / Adam "exp_avg"     (flat, same layout as params) */
  float* state1;             /* Adam "exp_avg_sq" (NULL for Adagrad) */
} gt_optim_desc;

/* Every kind of the family.  The hyper-parameters are doubles, as torch.optim keeps them (python floats): the per-step
 * scalars (1 - beta, 1 - alpha, lr / (1 - beta1^t), ...) are formed in double and rounded to float once, as torch's
 * single-tensor code path does.  lr alone is rounded to float first, so that gt_bind_optimizer_ex and gt_set_lr agree.
 * State buffers (flat float32, same layout as params; a buffer the kind / flags do not use may be NULL):
 *   kind       state0          state1                              state2
 *   ADAGRAD    sum             -                                   -
 *   ADAM(W)    exp_avg         exp_avg_sq                          max_exp_avg_sq (AMSGRAD)
 *   SGD        momentum_buffer (momentum != 0)  -                  -
 *   RMSPROP    square_avg      momentum_buffer (momentum > 0)      grad_avg (CENTERED)
 *   ADADELTA   square_avg      acc_delta                           -
 *   ADAMAX     exp_avg         exp_inf                             -
 *   NADAM      exp_avg         exp_avg_sq                          -
 *   RADAM      exp_avg         exp_avg_sq                          -
 *   RPROP      prev            step_size (the CALLER fills it with lr when it creates it)   -
 *   ASGD       ax              -                                   -
 * Host scalar state: torch keeps NAdam's mu_product and ASGD's eta and mu as 0-dim float32 tensors next to `step`.  They are
 * host values here: host_state0 / host_state1 give them as they stand after `step` updates (NADAM: mu_product, 1 at step 0, and
 * nothing -- the float32 product underflows to 0 after some 135 updates, as in torch, and 0 is accepted --; ASGD: eta, (float)lr at step 0, and mu, 1 at step 0), gt_get_optimizer_scalars returns them after the updates taken
 * since.  They are float32 values carried in doubles.  The value used by update t is a function of these bind-time values, the
 * bound step and t alone.  ASGD derives eta from lr in double and rounds it to float32 once, as torch does: for this kind lr is
 * kept as given, not rounded to float first (gt_set_lr still stores a float). */
typedef struct {
  int32_t kind;              /* GT_OPT_ADAGRAD .. GT_OPT_ASGD */
  uint32_t flags;            /* GT_OPTF_* */
  double lr, weight_decay, eps;
  double lr_decay;           /* Adagrad */
  double beta1, beta2;       /* Adam, AdamW, Adamax */
  double momentum;           /* SGD, RMSprop */
  double dampening;          /* SGD */
  double alpha;              /* RMSprop alpha, Adadelta rho, ASGD alpha */
  float max_grad_norm;       /* as in gt_optim_desc */
  int32_t reserved_;
  int64_t step;              /* number of steps already taken */
  float* state0;
  float* state1;
  float* state2;
  /* The fields below exist since GT_OPT_NADAM .. GT_OPT_ASGD and are read for those kinds ONLY: for GT_OPT_ADAGRAD .. GT_OPT_ADAMAX the
   * library never looks past state2, so a caller built against the 120-byte struct of the first family keeps working unchanged. */
  double momentum_decay;     /* NAdam */
  double etaminus, etaplus;  /* Rprop etas */
  double step_size_min, step_size_max;   /* Rprop step_sizes */
  double lambd, t0;          /* ASGD */
  double host_state0;        /* NAdam mu_product / ASGD eta, as they stand after `step` updates */
  double host_state1;        /* ASGD mu */
} gt_optim_desc_ex;

typedef struct {             /* return values of update_discriminator, train.py:278-279 (same order) */
  float loss_d, loss_fake_d, loss_real_d, real_correct_count, fake_correct_count;
  float grad_norm;           /* pre-clip ||grad D||_2 from the split-phase gt_update_discriminator_end; 0 from the fused call,
                              * which returns before the backward pass has finished */
} gt_d_result;

typedef struct {             /* return values of update_generator, train.py:320 (same order) */
  float loss_mse, loss_mge, loss_adv, loss_g;
  float grad_norm;           /* pre-clip ||grad G||_2 of the accumulated gradient (split-phase form only, see above) */
} gt_g_result;

/* ---- lifecycle ------------------------------------------------------------------------ */
const char* gt_last_error(void);
const char* gt_version(void);
int gt_engine_create(const gt_stream_config* cfg, gt_engine** out);
void gt_engine_destroy(gt_engine* e);
/* What the engines of this process own right now (introspection, tests): out[0] live device blocks, out[1] their bytes, out[2] live
 * pinned host blocks, out[3] live events -- all of engine lifetime, process-wide relaxed counters kept on the host by the types that own
 * them.  The grow-only scratch of the stand-alone gt_op_* hooks lives as long as its thread and is not counted. */
int gt_live_resources(int64_t out[4]);

/* getattr(gantts.models, name)(**params) + .cuda()            (train.py:773-793).  GT_ROLE_G: every architecture; GT_ROLE_D: GT_ARCH_MLP,
 * GT_ARCH_LSTM (an LSTMRNN scoring frames) or GT_ARCH_SRU (an SRURNN scoring frames: sequence lengths ignored as in the reference, at
 * most 8 layers; parity unpinned like every SRU path), out_dim 1, last_sigmoid set, for the recurrent ones hidden_dim x directions
 * <= 1024; other combinations (the tuple-returning In2Out* among them) are rejected (GT_ERR_INVALID). */
int gt_bind_model(gt_engine* e, int role, const gt_model_desc* desc);
/* getattr(optim, hp.optimizer_*)(model.parameters(), **params) (train.py:796-799).  GT_OPT_ADAGRAD and GT_OPT_ADAM through the first
 * descriptor: it is widened to gt_optim_desc_ex and bound by gt_bind_optimizer_ex, whose checks apply -- a negative lr / eps /
 * weight_decay / lr_decay or a beta outside [0, 1), which this entry once took unlooked at, is GT_ERR_INVALID. */
int gt_bind_optimizer(gt_engine* e, int role, const gt_optim_desc* desc);
/* The same for every GT_OPT_* kind.  Checks per kind which state buffers must be given and rejects what torch's constructors
 * reject (GT_ERR_INVALID): negative lr / eps / weight_decay / momentum / alpha / momentum_decay, betas or rho outside their
 * interval, etas that are not 0 < etaminus < 1 < etaplus, nesterov with zero momentum or non-zero dampening, a flag that does
 * not belong to the kind. */
int gt_bind_optimizer_ex(gt_engine* e, int role, const gt_optim_desc_ex* desc);
/* model.train() / model.eval()                                 (train.py:481-486) */
int gt_set_training(gt_engine* e, int role, int training);
/* exp_lr_scheduler writes param_group["lr"]                     (train.py:323-333) */
int gt_set_lr(gt_engine* e, int role, float lr);
int gt_get_optimizer_step(gt_engine* e, int role, int64_t* step);
/* The host scalar state of the bound optimizer after the updates taken so far (what optimizer.state_dict() holds beside
 * "step"): NADAM out[0] = mu_product; ASGD out[0] = eta, out[1] = mu; 0 for every other kind. */
int gt_get_optimizer_scalars(gt_engine* e, int role, double out[2]);
/* The seed of the Philox dropout streams.  RESTARTS THE STEP COUNT (the streams are keyed by seed, step count and site: the step
 * behind gt_set_seed is step 1 again) and forgets the engine-made per-step copies of x, whose key holds the step count.  From here
 * on the engine computes what a new engine with this seed computes, bit for bit. */
int gt_set_seed(gt_engine* e, uint64_t seed);
/* Parity hook: use the caller's 0/1 float mask ((rows, hidden) contiguous, device) instead of the
 * Philox stream for dropout site `layer` of forward pass `pass` of `role`; NULL restores Philox.
 * passes: G: 0 = apply_generator.  D: 0 = real rows of the D step, 1 = generated rows of the
 * D step, 2 = generated rows of the G step (the order nn.Dropout is consumed in train.py:261-307), 3 = the WGAN-GP
 * interpolates of the D step (gt_set_grad_penalty; role D only).
 * SRURNN (models.py:152-154: rnn_dropout / dropout of the SRU cell are VARIATIONAL masks, one per sequence and shared
 * over time): `layer` = 2*l selects the input mask of SRU layer l, shape (B, n_in_l); 2*l + 1 its output mask, (B, H*dirs); an
 * SRURNN in the discriminator slot takes them per pass like every discriminator. */
int gt_set_dropout_mask(gt_engine* e, int role, int pass, int layer, const float* mask);
/* Parity hook for the production (Philox) dropout path, nn.Dropout inside gantts/models.py:132-139: writes the 0/1 keep
 * mask ((rows, cols) contiguous, device) that the engine's counter-based stream assigns to dropout site (role, pass,
 * layer) of the step that starts `steps_ahead` gt_apply_generator calls from now (1 = the next step).  The D step runs
 * its real and generated rows as ONE 2N-row pass: its site is pass 0 with rows [0,N) = real, [N,2N) = generated; pass 2
 * is the N-row D pass of the G step.  Feeding these masks to the reference (patched nn.Dropout) reproduces the step. */
int gt_op_philox_mask(gt_engine* e, int role, int pass, int layer, int64_t steps_ahead, float p, int64_t rows, int cols,
                      float* mask, void* stream);

/* Sequence lengths of the NEXT batch (host int64 array, as the `lengths` list the reference passes to
 * model(x, lengths=lengths), train.py:344; models.py:204-210 pack_padded_sequence).  Needed by the
 * recurrent networks only -- a recurrent generator, or an LSTMRNN in the discriminator slot (train.py:262, 268, 307) --; MLP ignores
 * lengths like the reference.  Unlike pack_padded_sequence the
 * batch need not be sorted.  The array is copied before the call returns; it reaches the device IN STREAM ORDER on
 * `stream` (the stream of the following step functions) through a ring of pinned slots, so the still-queued kernels of
 * the previous step keep reading their own lengths and the host never waits for the GPU here. */
int gt_set_lengths(gt_engine* e, const int64_t* lengths_host, int B, void* stream);
/* The engine keeps a banded image of every MLPG matrix R it has been given, keyed by (R pointer, T) (the reference
 * rebuilds and uploads R every batch, train.py:511-513; callers of this library keep one device R per padded length).
 * R must not be rewritten in place or freed-and-reused while cached: call this first (drops all cached bands).  A stashed generator
 * pass that used a dropped band can no longer be back-propagated: the next step starts with gt_apply_generator. */
int gt_invalidate_mlpg_cache(gt_engine* e);
/* The MLPG band built on the device from the window set, without a dense R.  Register the windows once: window w is
 * (l[w], u[w], its l[w] + u[w] + 1 coefficients), (W_w x)[t] = sum_k coef_w[k + l[w]] x[t + k], the coefficients of all windows one
 * after the other in coef_concat (copied).  n must be the engine's num_windows; l, u >= 0, l + u <= GT_MLPG_MAX_WINDOW_SPAN, finite
 * coefficients.  Registering a DIFFERENT set drops the entries built from the former one (synchronises the device like
 * the invalidation above; entries of dense matrices stay); the same set again is free.
 * GT_MLPG_R_FROM_WINDOWS is then accepted wherever a dense R is: the apply_generator, model_forward and MLPG entry points below.  It is never
 * dereferenced.  The band cache keeps such entries under (GT_MLPG_R_FROM_WINDOWS, T) beside those of dense matrices; a miss builds the
 * taps in O(T) memory (banded Cholesky of W^T W and a selected inversion in float64, rounded to float32 once) and applies the same
 * half-width rule and refusals as for a dense R.  A window set whose W^T W is not positive definite returns GT_ERR_INVALID
 * ("window set does not determine the static features") and caches nothing; so does the sentinel without registered windows. */
#define GT_MLPG_MAX_WINDOW_SPAN 32
#define GT_MLPG_R_FROM_WINDOWS ((const float*)(uintptr_t)1)
int gt_set_mlpg_windows(gt_engine* e, int n, const int32_t* l, const int32_t* u, const double* coef_concat);

/* ---- hot path -------------------------------------------------------------------------- */
/* optimizer.zero_grad()                                         (train.py:538-539) */
int gt_zero_grad(gt_engine* e, int role);

/* apply_generator(model_g, x, R, lengths) -> (y_hat, y_hat_static)   (train.py:336-355)
 * x (B,T,in_dim of G); R dense (T, num_windows*T) from unit_variance_mlpg_matrix or NULL
 * (train.py:510-515); outputs y_hat (B,T,out_dim), y_hat_static (B,T,static width). */
int gt_apply_generator(gt_engine* e, const float* x, const float* R, int B, int T,
                       float* y_hat, float* y_hat_static, void* stream);

/* update_discriminator(model_d, optimizer_d, x, y_static, y_hat_static, lengths, mask, phase, eps)
 * (train.py:245-279).  x is the conditioning input (cond_dim wide, may be NULL when not
 * conditioned); mask (B,T) float; train != 0 <=> phase == "train".  When y_hat_static is the
 * buffer the last gt_apply_generator wrote (the autograd graph of the reference), the D-loss
 * gradient w.r.t. it is kept and added to G's gradient by gt_update_generator (train.py:265,274,316). */
int gt_update_discriminator(gt_engine* e, const float* x, const float* y_static, const float* y_hat_static,
                            const float* mask, int B, int T, int train, float eps,
                            gt_d_result* out, void* stream);

/* update_generator(model_g, model_d, optimizer_g, x, y, y_hat, y_static, y_hat_static, adv_w,
 *                  lengths, mask, phase, mse_w, mge_w, eps)      (train.py:282-320) */
int gt_update_generator(gt_engine* e, const float* x, const float* y, const float* y_hat,
                        const float* y_static, const float* y_hat_static, float adv_w,
                        const float* mask, int B, int T, int train, float mse_w, float mge_w, float eps,
                        gt_g_result* out, void* stream);

/* Split-phase forms for data parallelism (one process per GPU): *_begin runs forward+backward and
 * leaves the LOCAL gradient sums in the bound grads buffer and the local loss sums in
 * gt_scalar_buffer(); the host all-reduces both (RCCL), then *_end clips, steps and finalises.
 * tv_global > 0 overrides sum(mask) as the loss normaliser (global valid-frame count). */
int gt_set_loss_normalizer(gt_engine* e, float tv_global);
/* same, from a device double the caller keeps alive (e.g. the all-reduced sum(mask)): no host round trip; the
 * value is read by the next step functions in stream order.  NULL returns to the local / host normaliser. */
int gt_set_loss_normalizer_device(gt_engine* e, const double* tv_global_dev);
/* engine switches that do not change results beyond fp32 summation order. */
/* GT_OPT_LSTM_PERSISTENT (default 1): recurrent generators (models.py:170-213) run each layer's time loop as ONE
 * persistent launch (W_hh slices resident in registers, h exchanged between workgroups through tagged granules);
 * 0 = one launch per time step.  GT_OPT_LSTM_FWD_UNITS: hidden units per workgroup of the forward persistent kernel
 * (8 or 16; 0 = automatic). */
#define GT_OPT_LSTM_PERSISTENT 2
#define GT_OPT_LSTM_FWD_UNITS 3
/* GT_OPT_LSTM_XCD_LOCAL (default 1): a group of workgroups that verifies at kernel start that it runs on ONE XCD
 * exchanges through that XCD's L2 (workgroup-scope stores) instead of write-through stores; 0 = always write-through. */
#define GT_OPT_LSTM_XCD_LOCAL 4
/* GT_OPT_MATMUL_BF16 (default 0): mixed precision for the frame x weight products of BOTH networks (BASELINE.json
 * configs[2]): operands are rounded to bfloat16 inside the GEMM and multiplied on the bf16 matrix cores with float32
 * accumulation; parameters ("master weights"), optimizer state, activations in memory, the recurrent state and every
 * reduction stay float32.  Results differ from the float32 path at the 1e-2 relative level (tests/test_gpu_parity.py).
 * An SRURNN in the discriminator slot keeps float32 products and float32 stashes under this option (an SRURNN generator takes the
 * bf16 path).  GT_OPT_SRU_D_BF16 is the separate switch for that discriminator's products. */
#define GT_OPT_MATMUL_BF16 5
/* GT_OPT_SPLIT_FIRST_LAYER (default 1): the conditioned float32 discriminator evaluates its first layer as x . W_x^T (once per
 * D step, shared by the real and the generated rows) + adv . W_adv^T instead of one product over a concatenated [x | adv] image
 * (train.py:254-256); 0 = the concatenated image.  Same sums up to float32 association. */
#define GT_OPT_SPLIT_FIRST_LAYER 6
/* Schedule switches (defaults are the measured best; the GT_* environment variables of the same names only provide the default at
 * engine creation; the ids 7, 8, 9 and 12 are retired and not reused): GT_OPT_COMM_D_ONE_MSG (1) / _EARLY_G (1) data-parallel
 * message schedule; GT_OPT_COMM_FORCE (0) issue the collectives with one rank as well (bench.py --force-dp, tests);
 * GT_OPT_LAUNCH_RIDERS (1) the fused single-GPU step's small reductions (valid-frame count, the head's scalars in the generator
 * step, the generator step's finalisation) ride as an extra workgroup of a neighbouring launch instead of launches of their own;
 * GT_OPT_COMM_CLOSE_INLINE (1) a data-parallel step's closing messages are issued on the step's own stream (no event hand-off on
 * the critical path); GT_OPT_POLL_RESULTS (1; round 5: -6 us per cfg2 step, the event's two 5.8 us holes in the kernel trace) the fused single-GPU calls learn that their scalars have landed in host memory from
 * a ticket the finalising kernel writes behind them, not from an event recorded in the middle of the step;
 * GT_OPT_COMM_TV_IN_SUMS (1) the data-parallel discriminator step sends its valid-frame count WITH its loss sums (five collectives
 * per G+D step instead of six): the backward pass runs on the unnormalised loss, 1 / Tv is applied by the optimizer kernel (the
 * gradient it writes back is the normalised, clipped one) and by the generator step where it adds the kept gradient;
 * GT_OPT_COMM_IPC (1) see gt_comm_ipc_* below. */
#define GT_OPT_COMM_D_ONE_MSG 10
#define GT_OPT_COMM_EARLY_G 11
#define GT_OPT_COMM_FORCE 13
#define GT_OPT_LAUNCH_RIDERS 14
#define GT_OPT_COMM_CLOSE_INLINE 15
#define GT_OPT_POLL_RESULTS 16
#define GT_OPT_COMM_TV_IN_SUMS 17
#define GT_OPT_COMM_IPC 18
/* GT_OPT_FUSED_DSTACK (default 1): the float32 MLP discriminator (gantts/models.py:121-141; hidden_dim 128 or 256, <= 4 hidden
 * layers) runs its hidden layers above the first one, last_linear + sigmoid + the BCE terms (train.py:261-271) and -- in the
 * generator step (train.py:307-308) -- the whole backward-data chain down to the adversarial input columns as ONE launch per pass,
 * panel of 32 frames by panel, activations resident in LDS.  1 (default): when the pass has at least one panel per CU (a panel is
 * walked by ONE workgroup: small per-rank batches are faster as per-layer launches); 2: always; 0: one launch per layer + the head
 * kernel.  Same sums up to float32 association. */
#define GT_OPT_FUSED_DSTACK 19
/* GT_OPT_SRU_D_BF16 (default 0; 0 or 1; GT_SRU_D_BF16 in the environment provides the default at engine creation): an SRURNN in the
 * discriminator slot runs the three products of every layer (U = xin . W, dW, d input -- the gradient towards the generator
 * included) through the bf16-storage family of GT_OPT_MATMUL_BF16: operands live as bfloat16 images, float32 accumulation.  U, the
 * cell state, h, c, every reduction, the master weights and the optimizer state stay float32; hidden2out stays in the float32 head
 * kernel.  Independent of GT_OPT_MATMUL_BF16 (a float32 generator with a bf16 SRU discriminator is a supported pair).  Needs
 * hidden_dim % 8 == 0, the generator's rule: any other width silently keeps the float32 path.  LSTMRNN discriminators are not
 * affected.  Results differ from the float32 path at the 1e-2 relative level (tests/test_gpu_sru_d_bf16.py). */
#define GT_OPT_SRU_D_BF16 20
/* GT_OPT_GAN_OBJECTIVE (default 0; beyond the reference): the adversarial objective of both update steps.  With z the discriminator's
 * output pre-activation of a frame, m its mask value and Tv the valid-frame count:
 *   0 bce    D = sigmoid(z)  real -log(D + eps)   generated, D step -log(1 - D + eps)   generated, G step -log(D + eps)   threshold 0.5
 *   1 ls     D = z           real 0.5 (z - 1)^2   generated, D step 0.5 z^2             generated, G step 0.5 (z - 1)^2   threshold 0.5
 *   2 hinge  D = z           real max(0, 1 - z)   generated, D step max(0, 1 + z)       generated, G step -z              threshold 0
 *   3 wgan   D = z           real -z              generated, D step z                   generated, G step -z              threshold 0
 *   4 kl     D = z           real -z              generated, D step exp(z - 1)          generated, G step -z              threshold 1
 *   5 rkl    D = z           real exp(-z)         generated, D step z - 1               generated, G step exp(-z)         threshold 0
 *   6 js     D = z           real sp(-z) - ln 2   generated, D step sp(z) - ln 2        generated, G step sp(-z) - ln 2   threshold 0
 * 4 .. 6 are the f-GAN divergences (Nowozin et al. 2016: KL, reverse KL, Jensen-Shannon): the D loss is the negative of the variational
 * bound E_real g_f(z) - E_fake f*(g_f(z)) with the paper's output activations g_f and conjugates f*, the G step its non-saturating form
 * (generated rows scored as real ones), the threshold g_f(z) > f'(1); sp(x) = max(x, 0) + log(1 + exp(-|x|)).  js is the logistic loss
 * minus 2 ln 2, without eps.  exp(z - 1) and exp(-z) are NOT clamped (a clamp would change the divergence): a frame whose exponent
 * overflows float32 (z - 1 > 88.7 under kl, z < -88.7 under rkl) gives an infinite loss term and seed gradient, which behaves like any other
 * non-finite gradient: grad_norm is not finite and the clipped update stores NaN, as torch would (the fault word is for device time-outs).
 * The results keep their meaning: loss_real_d / loss_fake_d / loss_adv = sum(phi m) / Tv of the column, real_correct_count =
 * sum([D > threshold] m), fake_correct_count = sum([D < threshold] m).  Same launches as objective 0 (the objective is a template
 * parameter of the two head kernels); `eps` is read by objective 0 alone.  The bound discriminator must have last_sigmoid = 1 under
 * objective 0 and last_sigmoid = 0 under 1 .. 6: checked at whichever of gt_bind_model and this option comes second, and at the entry of
 * every step that runs the discriminator, before any launch.  Any other value returns GT_ERR_INVALID.  A change drops pending
 * split-phase results and the kept dloss_d / dy_hat_static.  hinge, wgan, kl, rkl (its generated column) and js losses can be <= 0. */
#define GT_OPT_GAN_OBJECTIVE 21
int gt_set_option(gt_engine* e, int option, int value);
/* Weight clipping (WGAN): every later optimizer step of `role` clamps each updated parameter to [-c, c] inside the fused clip + update
 * launch, behind the update rule (what `for p in D.parameters(): p.data.clamp_(-c, c)` does after optimizer_d.step()); a NaN parameter
 * stays a NaN.  c = 0 switches it off (the default: the stored values are the rule's own); c must be finite and >= 0, and role
 * GT_ROLE_D -- anything else returns GT_ERR_INVALID.  Independent of GT_OPT_GAN_OBJECTIVE. */
int gt_set_weight_clip(gt_engine* e, int role, float c);
/* Weight averaging of the generator (beyond the reference): an exponential moving average of its parameters, kept inside the fused clip +
 * update launch.  The definition is torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(decay)) with
 * update_parameters() called once after every applied generator update, bit for bit: the first applied update makes the average a copy of
 * the updated parameters; every later one is ema.lerp_(p, w), w = float32(1.0 - decay) (the subtraction in double, rounded once), ONE fused
 * multiply-add per element -- fmaf(w, p - ema, ema) for w < 0.5, fmaf(-(1 - w), p - ema, p) otherwise.  p is the value the launch stores,
 * behind the update rule and behind gt_set_weight_clip's clamp.  `ema`: a caller-owned float32 device buffer of n floats, like optimizer
 * state, n the bound generator's parameter count; it costs 8 B of memory traffic per parameter and no launch.  ema = NULL (with decay 0)
 * switches the average off (the default): nothing is read or written, and the launch computes what it always did, bit for bit.  The setting
 * and the count survive gt_bind_optimizer* and gt_set_lr; giving another buffer keeps the count (the same average, moved).
 * gt_get_param_ema_count: the updates applied to the average so far -- torch's n_averaged --, counted where the optimizer's step count is
 * counted; an update skipped on the device fault word leaves the average untouched and is taken back out by gt_clear_faults.  The host
 * picks "copy" or the lerp weight from this count at every launch.  gt_set_param_ema_count sets it (a restored checkpoint's n_averaged; 0
 * makes the next applied update a copy again).
 * GT_ERR_INVALID: role D; a decay outside [0, 1] or NaN; n < 1; a NULL buffer with a decay; an n that is not the bound generator's parameter
 * count -- checked at the call when a generator is bound, and at the entry of every training generator step before any launch.
 * DATA PARALLEL: nothing to do and nothing refused -- every rank applies the same all-reduced update to the same parameters, so the ranks'
 * averages are identical without a collective. */
int gt_set_param_ema(gt_engine* e, int role, float* ema, int64_t n, double decay);
int gt_set_param_ema_count(gt_engine* e, int role, int64_t n_averaged);
int gt_get_param_ema_count(gt_engine* e, int role, int64_t* n_averaged);
/* Spectral normalisation of the MLP discriminator (SN-GAN; beyond the reference; torch.nn.utils.spectral_norm with n_power_iterations = 1
 * on every nn.Linear weight, biases untouched).  u [n_u] and v [n_v] are caller-owned float32 device buffers, like optimizer state:
 * per layer in state_dict order a unit vector of `out` entries in u and one of `in` entries in v (torch's weight_u / weight_v), so
 * n_u = sum(out) and n_v = sum(in) of the bound discriminator -- checked.  u = v = NULL switches the feature off (the default).
 * With W (out, in) a layer's weight and eps = 1e-12, every discriminator pass in training mode (gt_set_training) runs ONE power iteration
 *   v' = W^T u / max(|W^T u|, eps);  r = W v';  u' = r / max(|r|, eps);  sigma = u'^T r;  u <- u', v <- v'
 * and multiplies by W_eff = W / sigma everywhere; in eval mode nothing is iterated or stored and sigma = u^T W v.  A pass is: the D step
 * (ONE pass over the natural and the generated rows, where the reference calls D twice: one iteration, not torch's two), the generator
 * step's adversarial pass, gt_model_forward(role D).  The D step's optimizer sees the gradient w.r.t. W,
 *   (G - (sum G (.) W_eff) u' v'^T) / sigma,   G = d loss / d W_eff,
 * (u', v' constants, as in torch) for clip-norm and update; the optimizer updates the caller's W and gt_set_weight_clip keeps clamping it.
 * An all-zero W gives sigma = 0 and NaN weights, as in torch.  At most 3 launches per pass and 2 per D step are added; with the feature
 * off nothing changes.  optimizer_d.zero_grad() must precede every update_discriminator(phase = "train") (GT_ERR_STATE otherwise: a
 * projected gradient is not accumulated into).  GT_ERR_INVALID: role G; an LSTMRNN or SRURNN discriminator; out or in of a layer above
 * 512; lengths that do not fit; a sharded or communicating engine (gt_set_shard with world > 1, gt_comm_init -- which in turn refuse an
 * engine with the feature on).  The discriminator must be bound first; binding another one keeps the feature on if the lengths still fit. */
int gt_set_spectral_norm(gt_engine* e, int role, float* u, float* v, int64_t n_u, int64_t n_v);
/* Gradient penalties of the MLP discriminator (beyond the reference): kind 0 off (the default), 1 R1 (Mescheder et al. 2018) on the natural
 * rows of the D step, 2 WGAN-GP (Gulrajani et al. 2017) on x_hat = eps real + (1 - eps) fake with eps ~ U[0, 1) per frame.  The penalty is
 * taken on the output layer's pre-activation z under every objective, w.r.t. the Da adversarial columns only (the conditioning x is data).
 * Per frame, with g = dz / d adv, n = sqrt(sum g^2 + 1e-12), T the step's valid-frame count:
 *   r1: phi = (weight / 2) sum g^2;   wgan-gp: phi = weight (n - 1)^2;   P = sum mask phi / T
 * Every gt_update_discriminator(train) then adds dP / dW to the discriminator's weight gradients behind its backward pass and ahead of
 * clip-norm and the update, so gt_d_result.grad_norm sees the sum; loss_d stays the adversarial loss alone.  Biases, the conditioning
 * columns of the first layer and the generator (the kept dloss_d / dy_hat_static included) get exactly nothing: LeakyReLU and dropout are
 * piecewise linear.  WGAN-GP runs one more forward pass, dropout pass 3 of gt_set_dropout_mask; eps is one Philox4x32-10 draw per frame
 * keyed by the seed and the step, or the caller's (gt_set_gp_epsilon: [B T] device floats, NULL restores Philox).  With kind 0 nothing
 * changes, bit for bit.  GT_ERR_INVALID, at the switch or at the next D step before any launch: role G; an LSTMRNN or SRURNN
 * discriminator; GT_OPT_MATMUL_BF16; a sharded or communicating engine; spectral normalisation on; weight < 0 or not finite; unknown kind.
 * gt_grad_penalty_result synchronises the stream of the last penalised step and reads the running device record: the means of P and of
 * sum mask n / T over the D steps since the last reset (0 when there were none), their number, and zeroes the record when reset != 0.
 * gt_grad_penalty_peek (parity): the last wgan-gp step's eps [B T] and x_hat [B T][Da] into the caller's device buffers (either may be null). */
int gt_set_grad_penalty(gt_engine* e, int role, int kind, float weight);
int gt_set_gp_epsilon(gt_engine* e, const float* eps);
int gt_grad_penalty_result(gt_engine* e, double* penalty_mean, double* grad_norm_mean, int64_t* steps, int reset);
int gt_grad_penalty_peek(gt_engine* e, float* eps, float* x_hat, void* stream);
/* Process-wide dispatch knobs of the kernels (tile shapes, pair launches, loader variants ...: measurement switches of the tools/
 * harnesses and A/B runs; none selects different arithmetic).  Names: gemm_pair, pair_order, gemm_tiles_big, gemm_unaligned, tn_wgs, tn_split_wgs, split_fused,
 * b16_tiles, b16_wg_tile, b16_dma, mlpg_fpl, mlpg_tt, sru_coop (its former name sru_lw, 0 / 1 / 2, is still accepted: 2 = 1), head_vec, lstm_bt; the environment variables GT_<NAME>
 * provide the initial values.  lstm_bt: sequences per batch tile of the persistent LSTM kernels, 0 (by shape), 8 or 16; any other
 * value is refused.  A forced tile still has to pass the co-residency check of the launch (else the per-step kernels run). */
int gt_set_tuning(const char* name, int value);
/* Row pitch (in floats) of the input tensors `x` of the step functions, like the `lda` of a BLAS call: ld_generator_input for the
 * x of gt_apply_generator (train.py:542: cat(x, z) or x), ld_condition for the conditioning x of gt_update_discriminator /
 * gt_update_generator (train.py:254-256).  0 (default) = dense rows (pitch = width).  A pitch that is a multiple of 4 floats on a
 * 16-byte aligned tensor lets every product read the caller's rows with 16-byte loads -- a batch pipeline that stages batches
 * anyway (gantts_amd.data.DevicePrefetcher(pitch_x=True)) provides it for free; with dense 425-wide rows the engine makes the
 * 16-byte-pitch copy its weight-gradient products need itself, once per step.  Supported where it pays: float32 MLP generators
 * and the conditioned float32 discriminator; other paths reject a non-dense pitch.
 * The engine-made copies are remembered by (pointer, pitch, columns, rows, step count), not by contents, and last one batch:
 * gt_apply_generator and gt_set_seed forget them, so a staging buffer refilled in place between steps is read anew.  The single
 * exception to "a step's result depends on the values of its inputs, not on what the engine did before"  is an x
 * refilled in place BETWEEN THE TWO UPDATE CALLS OF ONE STEP (behind one gt_apply_generator): the second call may read the copy
 * the first one made. */
int gt_set_x_pitch(gt_engine* e, int ld_generator_input, int ld_condition);
/* The persistent recurrence kernels bound every inter-workgroup wait by a wall-clock timeout and raise a device fault
 * word instead of hanging.  The step functions report a fault they have seen (GT_ERR_HIP) at their next entry;
 * this call synchronises `stream` and reports the current state. */
int gt_check_faults(gt_engine* e, void* stream);
/* Recurrence layer-passes of this engine (both roles) by the kernels that ran them, counted on the host when the launches are
 * issued (no device work, no synchronisation).  One layer's forward, or its backward, is one pass (all directions and batch
 * tiles in one launch).  Slot 16 * backward + 8 * (HP == 512) + 4 * (UPC == 16) + 2 * (BT == 16) + bf16 counts the persistent
 * kernel of that instantiation (HP: hidden units padded to 256 or 512; UPC: hidden units per workgroup of the forward, 8 or 16 --
 * always 0 in the bit for a backward; BT: sequences per batch tile; bf16: recurrent products in bf16).  Slot 32 counts passes run
 * on the per-step kernels; slot 33 those of them where the persistent path applied (GT_OPT_LSTM_PERSISTENT, H <= 512, T >= 2)
 * but no persistent grid was co-resident.  Copies the GT_LSTM_PATH_SLOTS counts to `counts` (may be null); reset != 0 then
 * zeroes them. */
#define GT_LSTM_PATH_SLOTS 34
int gt_lstm_path_counts(gt_engine* e, int64_t* counts, int reset);
/* A raised fault word makes every optimizer launch behind it a no-op (parameters, gradients and optimizer state of the
 * faulted step stay as they were; optimizer.step() of train.py:276,318 is simply not taken).  This call synchronises,
 * takes the skipped steps back out of the step counters, clears the word and resets the per-step call state, so the
 * engine can be used again -- e.g. after gt_set_option(e, GT_OPT_LSTM_PERSISTENT, 0).  The next call must be
 * gt_apply_generator.  The gradient norm of a skipped update is reported as NaN.
 * DATA PARALLEL: the fault word is local to a rank -- a timeout on one rank makes only that rank skip its update while its peers
 * apply the all-reduced gradient, and the faulted rank stops posting collectives at its next step entry.  Under a communicator a
 * fault is therefore FATAL for the job: tear the ranks down and restart from the last checkpoint (gt_clear_faults re-arms one
 * engine, it does not re-synchronise replicas). */
int gt_clear_faults(gt_engine* e, void* stream);
/* ---- data-parallel communicator (one process per GPU; RCCL == NCCL on ROCm, bound at run time) ----
 * The reference has no multi-device code; the step being sharded is train.py:538-585.  Every rank holds the
 * full G / D and whole sequences of the minibatch.  With a communicator attached the FUSED step functions above are
 * data-parallel by themselves: the valid-frame count, each network's gradient (one bucket per layer, handed to RCCL as
 * soon as that layer's weight gradient is final, i.e. overlapped with the rest of the backward pass) and the additive
 * loss / count sums are summed over the ranks; clip-norm + optimizer then run on the reduced gradient, so all replicas
 * take bit-identical steps and every rank returns the GLOBAL scalars.  zero_grad must precede each update_* call.
 * gt_comm_unique_id: rank 0 fills `id_out` (GT_COMM_ID_BYTES) and ships it to the other ranks by any means;
 * gt_comm_init: collective over all ranks (ncclCommInitRank); gt_comm_destroy detaches (also done by gt_engine_destroy). */
#define GT_COMM_ID_BYTES 128
int gt_comm_unique_id(void* id_out);
int gt_comm_init(gt_engine* e, int rank, int world, const void* id);
int gt_comm_destroy(gt_engine* e);
int gt_comm_info(gt_engine* e, int* rank, int* world);
/* Schedule trace of the data-parallel step (a measurement, bench.py --comm-trace): while it is on, every message of the step and every
 * wait of the step stream for the communicator's stream is bracketed by timed events.  gt_comm_trace(e, 1) clears and starts,
 * gt_comm_trace(e, 0) stops; gt_comm_trace_read synchronises the device and fills `out` with up to max_records records of five doubles
 * {kind (0 message, 1 wait of the step stream), bytes, issued on the step stream itself (closing message) 0/1, start, end} -- times in
 * microseconds after the first record's start -- and sets *n_records (max_records == 0: the number of records held).  The reference
 * has no counterpart: train.py:538-585 is one process. */
int gt_comm_trace(gt_engine* e, int enable);
int gt_comm_trace_read(gt_engine* e, double* out, int max_records, int* n_records);
/* The small-message collective of SURVEY 8(e): a full-mesh TWO-SHOT all-reduce over hipIpc peer buffers (gantts_amd/csrc/eng_ipc.hip),
 * for every message of the step that fits an 8 MB slot -- at cfg2 all of them.  Every rank exports an arena in its own HBM
 * (gt_comm_ipc_export fills `handle_out`, GT_IPC_HANDLE_BYTES), the handles travel to all ranks by any means (like the unique id),
 * gt_comm_ipc_attach maps the peers' arenas (`handles`: world x GT_IPC_HANDLE_BYTES, in rank order; the own entry is ignored).  From
 * then on (GT_OPT_COMM_IPC, default 1) such messages are reduced by three launches of the engine's own -- publish, reduce my 1/W
 * chunk in rank order and push it to every rank, collect -- instead of an RCCL call: two link latencies per message instead of a
 * ring's 2 (W - 1), bit-identical results on all replicas; larger messages and everything before the attach use RCCL.  A
 * communicator (gt_comm_init) must be attached as well: it provides the stream, the fallback and the rank / world the arenas must
 * agree with.  Cross-device waits are bounded by a wall-clock timeout that raises the fault word (gt_check_faults).
 * gt_comm_ipc_messages: how many messages have taken this path (tests). */
#define GT_IPC_HANDLE_BYTES 64
#define GT_IPC_MAX_WORLD 8
int gt_comm_ipc_export(gt_engine* e, void* handle_out);
int gt_comm_ipc_attach(gt_engine* e, int rank, int world, const void* handles);
int gt_comm_ipc_messages(gt_engine* e, long long* n);
/* The shard this engine holds, for hosts that all-reduce themselves between the split-phase calls (no communicator):
 * sequence b of this engine is sequence rank + world * b of the whole minibatch (round-robin dealing).
 * gt_comm_init implies it.  It keys the dropout streams by GLOBAL frame / sequence: with T % 16 == 0 a world-k run draws, for
 * its rows, exactly the bits a one-process run draws for the whole minibatch (the reference draws one mask over the whole
 * minibatch: gantts/models.py:139 inside train.py:538-585), so data-parallel runs reproduce the single-GPU run; for other T
 * the MLP sites fall back to independent per-rank streams (the SRU's per-sequence masks are global for every T). */
int gt_set_shard(gt_engine* e, int rank, int world);

int gt_update_discriminator_begin(gt_engine* e, const float* x, const float* y_static, const float* y_hat_static,
                                  const float* mask, int B, int T, int train, float eps, void* stream);
int gt_update_discriminator_end(gt_engine* e, int train, gt_d_result* out, void* stream);
int gt_update_generator_begin(gt_engine* e, const float* x, const float* y, const float* y_hat,
                              const float* y_static, const float* y_hat_static, float adv_w,
                              const float* mask, int B, int T, int train, float mse_w, float mge_w, float eps,
                              void* stream);
int gt_update_generator_end(gt_engine* e, int train, float adv_w, float mse_w, float mge_w,
                            gt_g_result* out, void* stream);
/* Deferred results: the *_end calls accept out == NULL -- optimizer step, the scalars' finalisation and their
 * D2H copy are enqueued, nothing is synchronised; these two block on just that copy.  A data-parallel host
 * uses the gap to enqueue the next phase, so the GPU never waits for the host. */
int gt_update_discriminator_result(gt_engine* e, gt_d_result* out);
int gt_update_generator_result(gt_engine* e, gt_g_result* out);
/* device pointer + length (in doubles) of the additive loss/count sums of the current step */
int gt_scalar_buffer(gt_engine* e, double** dev_ptr, int* n_doubles);

/* model(x, lengths=lengths) -- plain forward of a bound network (inference / reference-D spoofing
 * rate, train.py:549-558; evaluation_tts.py:167,221).  For IN2OUT `out2` receives y_hat_static and
 * R must be given; for MLP out2/R are ignored. */
int gt_model_forward(gt_engine* e, int role, const float* x, const float* R, int B, int T,
                     float* out, float* out2, void* stream);

/* Materialise G's pending gradient (the D-loss leak) into G's grads buffer without stepping --
 * parity/introspection helper mirroring `p.grad` after update_discriminator in the reference. */
int gt_flush_generator_grads(gt_engine* e, void* stream);

/* ---- stand-alone operators (same kernels as the engine; used by the host-side mirrors of
 *      gantts.seqloss / gantts.multistream and by the parity tests) ------------------------ */
/* sequence_mask(lengths, max_len)                                (gantts/seqloss.py:9-20); lengths int64 device */
int gt_op_sequence_mask(const int64_t* lengths, int B, int T, float* mask, void* stream);
/* MaskedMSELoss()(input, target, mask=mask)                      (gantts/seqloss.py:27-43); returns host scalar;
 * grad_input (optional) receives d loss / d input */
int gt_op_masked_mse(const float* input, const float* target, const float* mask, int B, int T, int D,
                     float* loss_out, float* grad_input, void* stream);
/* clip_grad_norm_(params, desc->max_grad_norm) + one optimizer step over the caller's flat buffers of n floats: the engine's own
 * two launches (squared-norm partials, then the fused clip + update kernel of desc->kind / flags), without an engine.  desc->step
 * is the number of steps already taken.  gscale (device, may be NULL): the gradient is that of a loss still to be multiplied by
 * *gscale.  grads receives the clipped gradient.  grad_norm_out (host, may be NULL): the pre-clip norm; synchronises if given. */
int gt_op_optim_step(const gt_optim_desc_ex* desc, float* params, float* grads, int64_t n, const float* gscale,
                     float* grad_norm_out, void* stream);
/* The same two launches with the weight-average rider of gt_set_param_ema: `ema` (device, n floats, not NULL) holds the average after
 * n_averaged >= 0 applied updates and receives the next one -- a copy of the updated parameters when n_averaged == 0, the lerp with
 * float32(1.0 - decay) otherwise.  The caller counts. */
int gt_op_optim_step_ema(const gt_optim_desc_ex* desc, float* params, float* grads, int64_t n, const float* gscale,
                         float* grad_norm_out, float* ema, int64_t n_averaged, double decay, void* stream);
/* Host only, no device: the host scalar state of desc's kind after `t` >= desc->step updates, from desc's hyper-parameters, step and
 * host_state* (the routine behind gt_get_optimizer_scalars and the update's own scalars; the descriptor is checked as by gt_bind_optimizer_ex, its state buffers aside, which are not looked at).  A caller
 * that steps through gt_op_optim_step passes out[] back in as host_state* of the next step's descriptor. */
int gt_op_optim_scalars(const gt_optim_desc_ex* desc, int64_t t, double out[2]);
/* Device-side collate: padding (train.py:139-159 `_pad_2d` / collate_fn) and the descending length sort of the batch
 * (train.py:494-501) without a padded host copy.  `ragged`: the batch's utterances un-padded, back to back, [total][D] (device);
 * start[b] / len[b] (device int64, B entries): first frame and frame count of the utterance that becomes OUTPUT sequence b (the
 * host passes them in sorted order); out: (B, T, D) on a row pitch of ld_out floats (>= D; pad columns and frames t >= len[b]
 * are zero, as `_pad_2d` leaves them).  Bit-exact copies. */
int gt_op_pad_sequences(const float* ragged, int D, const int64_t* start, const int64_t* len, int B, int T, float* out, int ld_out,
                        void* stream);
/* out[:, j] = in[:, idx[j]]  (select_streams / get_static_features / get_selected_static_stream:
 * gantts/multistream.py:33-79, train.py:232-242); idx int32 device array */
int gt_op_gather_cols(const float* in, int ld_in, const int32_t* idx, int n_idx, float* out, int ld_out,
                      int out_col_offset, int64_t rows, void* stream);
/* compute_distortions(y_static, y_hat_static, Y_data_mean, Y_data_std, lengths)  (train.py:399-432, with
 * split_streams / inv_scale :358-396 and nnmnkwii.metrics underneath) as one masked reduction over the valid
 * frames.  col_role[c] (host, Ds entries): 0 mel-cepstrum column of "mcd", 1 column of "bap_mcd", 2 lf0,
 * 3 vuv, 4 plain squared error ("dur_rmse"), -1 ignored; col_stat[c] (host): index of column c's
 * statistics inside stat_mean / stat_std (device; float, or double when stats_f64).  vuv_col = -1 if none.
 * lengths_host may be NULL (every sequence has T frames).  The caller forms the reference's ratios. */
typedef struct gt_distortion_sums {
  double s_mcd;      /* sum over valid frames of ||mgc - mgc_hat||_2 (inverse-scaled)            */
  double s_bap;      /* same for the bap columns                                                 */
  double s_f0;       /* sum of (exp(lf0) - exp(lf0_hat))^2 over frames voiced in both            */
  double n_voiced;   /* frames voiced in both (vuv binarised with > 0.5, train.py:375-377)        */
  double n_vuv_err;  /* frames whose binary vuv decisions differ                                 */
  double s_mse;      /* sum of squared errors of the role-4 columns                              */
  double n_frames;   /* valid frames                                                              */
} gt_distortion_sums;
int gt_compute_distortions(const float* y_static, const float* y_hat_static, int Ds, const void* stat_mean,
                           const void* stat_std, int stats_f64, const int32_t* col_stat_host,
                           const int32_t* col_role_host, int vuv_col, const int64_t* lengths_host, int B, int T,
                           gt_distortion_sums* out, void* stream);
/* ---- epoch ledger: the running sums of the training loop, kept on the device ------------------------------
 * train_loop (train.py:435-643) adds each step's scalars and each batch's distortion metrics into host sums and uses
 * none of them before the phase ends.  The ledger is a record of GT_LEDGER_SLOTS doubles in device memory; ONE
 * single-workgroup launch per batch (epoch_ledger_kernel) adds into it exactly what the loop adds on the host, each
 * operation in the host's order and rounded alone (no contraction), so a phase's sums have the host sums' bits:
 *   slots 0..6   generator, mse, mge, loss_real_d, loss_fake_d, loss_adv, discriminator   (float32 results, widened)
 *   slots 7..8   real_correct, fake_correct
 *   slots 9..13  mcd, bap_mcd, f0_rmse, vuv_err, dur_rmse     acoustic: mcd += (C * s_mcd) / n, bap_mcd += ((C * s_bap) / n) / 10,
 *                vuv_err += n_vuv_err / n, f0_rmse += n_voiced > 0 ? sqrt(s_f0 / n_voiced) : NaN (the NaN then stays, as in the
 *                host sum); duration: dur_rmse += sqrt(s_mse / (n * Ds)); vc: mcd += (C * s_mcd) / n.  C = logdb_const
 *                (10 / ln 10 * sqrt 2), computed by the HOST and passed as a double.
 *   slots 14..15 D updates and G updates counted
 *   slots 16..31 reserved, never written
 * A batch without valid frames (n == 0) is not defined: train_loop has none.
 * gt_ledger_configure: once per engine and layout (synchronises; zeroes the record).  The column tables are uploaded here;
 *   stat_mean / stat_std (device; float, or double when stats_f64) are READ BY EVERY gt_ledger_add and stay the caller's.
 * gt_ledger_reset: zeroes the record in stream order.
 * gt_ledger_add: to be enqueued behind the step's gt_update_*_end(out = NULL) calls on the SAME stream (the finalising launches
 *   leave the step's results in device memory, which this reads).  With GT_LEDGER_HAS_DIST it first forms the batch's seven
 *   distortion sums -- the kernels and the reduction order of gt_compute_distortions, bit for bit -- from device-resident
 *   lengths (int64, B entries; NULL: every sequence has T frames); no host table, no copy, no synchronisation.  Never waits.
 * gt_ledger_read: one copy and one wait.
 * gt_ledger_buffers: device addresses of the record and of the last batch's seven distortion sums (introspection, tests).
 * gt_op_epoch_ledger: the same kernel on caller-supplied device values -- results_dev: 12 floats in the order loss_d,
 *   loss_fake_d, loss_real_d, real_correct, fake_correct, loss_mse, loss_mge, loss_adv, loss_g, gnorm_d, gnorm_g, tv;
 *   dist_dev: 7 doubles in gt_distortion_sums order (may be NULL without GT_LEDGER_HAS_DIST).
 * gt_host_wait_count: how often an engine call has blocked the calling thread on the device since creation (the waits for a
 *   step's scalars -- early, deferred or fetched -- and gt_ledger_read).  A host-side census: no device work. */
#define GT_LEDGER_SLOTS 32
#define GT_LEDGER_HAS_D 1
#define GT_LEDGER_HAS_G 2
#define GT_LEDGER_HAS_DIST 4
#define GT_LEDGER_ACOUSTIC 0
#define GT_LEDGER_DURATION 1
#define GT_LEDGER_VC 2
int gt_ledger_configure(gt_engine* e, int kind, int Ds, const int32_t* col_stat_host, const int32_t* col_role_host, int vuv_col,
                        const void* stat_mean, const void* stat_std, int stats_f64, double logdb_const);
int gt_ledger_reset(gt_engine* e, void* stream);
int gt_ledger_add(gt_engine* e, int flags, const float* y_static, const float* y_hat_static, const int64_t* lengths_dev_i64,
                  int B, int T, void* stream);
int gt_ledger_read(gt_engine* e, double out[GT_LEDGER_SLOTS], void* stream);
int gt_ledger_buffers(gt_engine* e, double** ledger_dev, double** dist_dev);
int gt_op_epoch_ledger(double* ledger_dev, const float* results_dev, const double* dist_dev, int flags, int kind, int Ds,
                       double logdb_const, void* stream);
int gt_host_wait_count(gt_engine* e, long long* n);
/* multi_stream_mlpg(inputs, R, stream_sizes, has_dynamic_features) (gantts/multistream.py:82-123) and its
 * transpose (autograd backward).  Uses the engine's stream config. */
int gt_op_mlpg_forward(gt_engine* e, const float* y, const float* R, int B, int T, float* y_static, void* stream);
int gt_op_mlpg_backward(gt_engine* e, const float* g_static, const float* R, int B, int T, float* g_y, void* stream);
/* nn.Linear forward / backward with the fused activation used by the models
 * (act: 0 none, 1 LeakyReLU(0.01) [+dropout mask], 2 sigmoid).  Y (rows,out), X (rows,in), W (out,in). */
int gt_op_linear_forward(const float* X, int ldx, const float* W, const float* bias, float* Y, int ldy,
                         int64_t rows, int in_dim, int out_dim, int act, const float* keep_mask, float p,
                         void* stream);
/* dX = (dY . W) [* f'(H_prev)],  dW = dY^T . X,  db = colsum(dY); any output may be NULL.
 * workspace is managed internally (hipMallocAsync on `stream`). */
int gt_op_linear_backward(const float* dY, int lddy, const float* X, int ldx, const float* W,
                          int64_t rows, int in_dim, int out_dim,
                          float* dX, int lddx, const float* H_prev, int act_prev, const float* keep_mask_prev, float p_prev,
                          float* dW, float* db, void* stream);

/* nn.Linear forward / backward through the bf16-STORAGE products of GT_OPT_MATMUL_BF16 (gemm_bf16s.hip.h): X, W, dY (and
 * H_prev) are cast to bfloat16 images exactly as the engine keeps them, multiplied on the bf16 matrix cores with float32
 * accumulation, and the results returned as float32.  Same argument meaning as gt_op_linear_forward / _backward; any of
 * Y / dY / dX / dW / db may be NULL.  Y_image / YT_image (optional, (rows,out) / (out,rows) float32): the bf16 result
 * image and its transposed twin as the forward epilogue wrote them.  Parity hook (tests/test_gpu_parity.py). */
int gt_op_linear_bf16(const float* X, const float* W, const float* bias, int64_t rows, int in_dim, int out_dim, int act,
                      const float* keep_mask, float p, float* Y, const float* dY, const float* H_prev, int act_prev,
                      const float* keep_mask_prev, float p_prev, float* dX, float* dW, float* db,
                      float* Y_image, float* YT_image, void* stream);

/* Parity hook of the float32 MFMA product family (gemm_f32.hip.h): one product through the engine's own dispatch (tile,
 * loader, slab split, pair and combine choice are the production ones).  Precision: prec 0 float32 products, 1 bf16 products
 * (operands rounded to bf16 in the loader, float32 accumulation).  Dropout: drop 0 none, 1 Philox keep bits of (key0, key1)
 * (philox_keep of gemm_f32.hip.h; thresh = round(p * 2^16)), 2 the 0/1 float mask `mask` [rows][ld_mask].  All pointers are
 * device pointers, all pitches in floats.  Routes:
 *   FORWARD          y[rows][ldy] (+= if accumulate) act(x[rows][ldx] . w[out][ldw]^T + bias [+ addm[m mod wrap][ld_addm]]), act on y's
 *                    columns with the dropout of `drop`;  the addm form is the split first layer's adversarial product (rows <= 2 wrap)
 *   FORWARD_SEG      the split first layer in one launch: y = LeakyReLU + Philox of x[m mod wrap][ldx] . w[:, :cd]^T +
 *                    adv[rows][ld_adv] . w[:, cd:in]^T + bias, rows = wrap or 2 wrap (float32, 64 x 64 tiles, 16-byte loadable)
 *   BACKWARD_DATA    dx[rows][ld_dx] (+=) (dy[rows][ld_dy] . w[:, col0:col0+ncols]) (.) f'(h[rows][ldh]) for act (the
 *                    producer's activation) with the producer's dropout
 *   WEIGHT_GRAD      dw[out][in] (+=) dy^T . x over rows frames, db[out] (+=) column sums of dy (either may be null);
 *                    rider != 0: the BACKWARD_DATA product of the same case may share the launch; defer != 0: deferred combine
 *   WEIGHT_GRAD_SPLIT  the split first layer's weight gradient: dw[:, :cd] = (dy[:wrap] (+ dy[wrap:])) ^T . x over wrap frames,
 *                    dw[:, cd:] = dy^T . adv over rows frames, db = column sums of dy; rows = wrap or 2 wrap; rider != 0: the
 *                    backward-data product dx = dy[rows - wrap:] . w[:, col0:col0+ncols] (no f') may share the launch
 * Scratch is allocated, synchronised and released inside the call.  A malformed case returns GT_ERR_INVALID. */
#define GT_GEMM_ROUTE_FORWARD 0
#define GT_GEMM_ROUTE_FORWARD_SEG 1
#define GT_GEMM_ROUTE_BACKWARD_DATA 2
#define GT_GEMM_ROUTE_WEIGHT_GRAD 3
#define GT_GEMM_ROUTE_WEIGHT_GRAD_SPLIT 4
typedef struct gt_gemm_case {
  int32_t route, prec;
  int32_t rows, in_dim, out_dim;
  int32_t act, drop;
  float p;
  uint32_t key0, key1;
  int32_t accumulate;
  int32_t col0, ncols;       /* BACKWARD_DATA and riders: column slice of w */
  int32_t wrap, cd;          /* FORWARD addm wrap; FORWARD_SEG / WEIGHT_GRAD_SPLIT: rows of one half, width of x */
  int32_t rider, defer;
  int32_t ldx, ldw, ldy, ld_dy, ldh, ld_mask, ld_addm, ld_adv, ld_dx;
  const float* x;
  const float* w;
  const float* bias;
  float* y;
  const float* dy;
  const float* h;
  const float* mask;
  const float* addm;
  const float* adv;
  float* dx;
  float* dw;
  float* db;
} gt_gemm_case;
int gt_op_gemm_f32(const gt_gemm_case* c, void* stream);
/* Product and combine launches of the float32 family by kernel, process-wide (the stand-alone operators have no engine), counted on
 * the host where each launch is issued (no device work, no synchronisation).  Slots:
 *   single product  (((((kind * 2 + (BM == 128)) * 2 + (BN == 128)) * 2 + VA) * 2 + VB) * 2 + bf16) * 6 + (AMODE + 1)   (0..575)
 *                   kind 0 forward (GEMM_NT), 1 backward-data (GEMM_NN), 2 weight gradient (GEMM_TN); VA / VB: 16-byte loader of
 *                   A / B; AMODE: GemmAmode, -1 epilogue decided at run time, 0 none, 1 LeakyReLU + Philox, 2 ... + added matrix,
 *                   3 summed A operand, 4 two-segment forward
 *   576..579        gemm_pair_kernel: float32 none / float32 LeakyReLU + Philox / float32 run time / bf16
 *   580, 581        gemm_tn_pair_kernel without / with the riding backward-data product
 *   582..587        combines: slab_reduce4, slab_reduce, slab_reduce_small, colsum_partial, colsum_finalize, slab_reduce_multi
 * Copies the GT_GEMM_PATH_SLOTS counts to `counts` (may be null); reset != 0 then zeroes them. */
#define GT_GEMM_PATH_SLOTS 588
int gt_gemm_path_counts(int64_t* counts, int reset);

/* Launches of the bf16-storage product family (gemm_bf16s.hip.h; GT_OPT_MATMUL_BF16 / GT_OPT_SRU_D_BF16) by kernel, process-wide,
 * counted on the host where each launch is issued (no device work, no synchronisation).  Slots:
 *   product   (epi * 5 + amode) * 4 + form                                                                            (0..59)
 *             epi 0 forward, 1 backward-data, 2 weight-gradient slab (amode 0 only); amode (GemmB16Amode) 0 none, 1 LeakyReLU +
 *             Philox, 2 LeakyReLU + buffer mask, 3 LeakyReLU, 4 sigmoid; form 0 64 x 64, 1 128 x 128 register loader,
 *             2 128 x 128 LDS-DMA, 3 256 x 256 LDS-DMA (8 waves)
 *   60..65    image builders: cast_transpose<float>, cast_transpose<bf16>, seqdrop, multi, cat, catdrop
 * The combines of the weight gradient (slab_reduce4, slab_reduce, slab_reduce_small, the deferred multi combine) and the column-sum
 * finalize of cast_transpose are counted in slots 582..587 of gt_gemm_path_counts.
 * Copies the GT_GEMM_B16_PATH_SLOTS counts to `counts` (may be null); reset != 0 then zeroes them. */
#define GT_GEMM_B16_PATH_SLOTS 66
int gt_gemm_b16_path_counts(int64_t* counts, int reset);

/* Parity hook of the bf16-storage products: one product through the production dispatch (launch_gemm_b16 for FORWARD and
 * BACKWARD_DATA, weight_grad_b16 for WEIGHT_GRAD).  Operands are float32 device matrices (pitches in floats); the hook builds their
 * bf16 images with cast_transpose into buffers it has filled with 0xFF bytes (bf16 NaN) first, so every pad of an image is poisoned.
 *   FORWARD        M = rows, N = out_dim, K = in_dim:  act(x[rows][ldx] . w[out][ldw]^T + bias) with the dropout of `drop`
 *   BACKWARD_DATA  M = rows, N = in_dim, K = out_dim:  (dy[rows][ld_dy] . w[out][ldw]) (.) f'(h[rows][ldh]); act is the PRODUCER's
 *                  activation, the dropout its dropout (mask [rows][ld_mask], in_dim wide)
 *   WEIGHT_GRAD    dw[out][in] (+= if accumulate) dy^T . x over rows frames, db[out] (+=) the column sums of the bf16 dy, or null
 * FORWARD / BACKWARD_DATA results, any of them null: c float32 [M][ldc] (+= if accumulate), cb the bf16 image [M][ldcb], cbt its
 * transposed twin [N][ldcbt] (raw 16-bit elements, pitches in elements; ldcbt % 4 == 0 and cbt 8-byte aligned).  act 0 none,
 * 1 LeakyReLU (+ dropout), 2 sigmoid; drop 0 none, 1 Philox keep bits of (key0, key1), 2 the 0/1 float mask.
 * Scratch is allocated, synchronised and released inside the call.  A malformed case returns GT_ERR_INVALID. */
typedef struct gt_gemm_b16_case {
  int32_t route;             /* GT_GEMM_ROUTE_FORWARD / _BACKWARD_DATA / _WEIGHT_GRAD */
  int32_t rows, in_dim, out_dim;
  int32_t act, drop;
  float p;
  uint32_t key0, key1;
  int32_t accumulate;
  int32_t ldx, ldw, ld_dy, ldh, ld_mask, ldc, ldcb, ldcbt;
  const float* x;
  const float* w;
  const float* bias;
  const float* dy;
  const float* h;
  const float* mask;
  float* c;
  uint16_t* cb;
  uint16_t* cbt;
  float* dw;
  float* db;
} gt_gemm_b16_case;
int gt_op_gemm_b16(const gt_gemm_b16_case* c, void* stream);

/* Parity hook of the bf16 image builders: one launch of the named kind through the engine's own launch code.  out [rows][ldo] and
 * outT [cols][ldt] are the caller's 16-bit buffers (either may be null); pads are not written.
 *   PLAIN_F32   in float32 [rows][ldi]; colsum (optional) [cols] (+= if colsum_accumulate) the column sums of the float32 values
 *   PLAIN_BF16  in a bf16 image [rows][ldi]
 *   SEQDROP     in float32 [rows][ldi] times mul[r / T][c], mul [rows / T][cols]
 *   CAT         image row r (g = r + row_off) = [x[g mod N][cd] | (g < N ? fa : fb)[g mod N][ldf] gathered by idx[cols - cd]]
 *   CATDROP     ... times mul[r / T][c]
 *   MULTI       jobs[0 .. n_jobs) float32 matrices in one launch (n_jobs <= 8) */
#define GT_CAST_PLAIN_F32 0
#define GT_CAST_PLAIN_BF16 1
#define GT_CAST_SEQDROP 2
#define GT_CAST_CAT 3
#define GT_CAST_CATDROP 4
#define GT_CAST_MULTI 5
#define GT_CAST_MAX_JOBS 8
typedef struct gt_cast_job {
  const float* in;
  uint16_t* out;
  uint16_t* outT;
  int64_t rows, ldt;
  int32_t ldi, cols, ldo, pad_;
} gt_cast_job;
typedef struct gt_cast_case {
  int32_t kind, cols, ldi, ldo;
  int32_t colsum_accumulate, T, cd, ldf;
  int32_t n_jobs, pad_;
  int64_t rows, ldt, N, row_off;
  const void* in;
  uint16_t* out;
  uint16_t* outT;
  float* colsum;
  const float* mul;
  const float* x;
  const float* fa;
  const float* fb;
  const int32_t* idx;
  gt_cast_job jobs[GT_CAST_MAX_JOBS];
} gt_cast_case;
int gt_op_cast_image(const gt_cast_case* c, void* stream);

/* Launches of the SRU recurrence (sru_kernels.hip.h, sru_cs_kernels.hip.h) by kernel, process-wide, counted on the host where each
 * launch is issued (no device work, no synchronisation).  Slots:
 *   0        sru_fwd_kernel (the sequential scan)
 *   1..4     sru_fwd_cs_kernel<NW, NXOUT>: 1 + 2 * (NW == 8) + NXOUT     (NXOUT: the scan writes the next product's bf16 images)
 *   5        sru_bwd_kernel
 *   6..9     sru_bwd_cs_kernel<NW, B16OUT>: 6 + 2 * (NW == 8) + B16OUT   (B16OUT: dU leaves as bf16 images)
 *   10..12   sru_input_mask_kernel, sru_input_dropout_kernel, sru_dx_adv_finish_kernel
 * Copies the GT_SRU_PATH_SLOTS counts to `counts` (may be null); reset != 0 then zeroes them. */
#define GT_SRU_PATH_SLOTS 13
int gt_sru_path_counts(int64_t* counts, int reset);

/* Parity hook of the SRU scans: ONE scan launch through the launch functions the engine's stacks use.  The form -- sequential, four or
 * eight waves per 64 columns -- follows from the tuning knobs sru_coop / sru_cs_waves and the shape exactly as in a step; the image
 * forms follow from nx_b / dU_b being set.  All pointers are the caller's device buffers; ncols = H * dirs, N = B * T, row = b * T + t,
 * columns >= H of a two-direction layer walk time backwards.
 *   forward  (backward == 0): reads U [N][ldu] (column j owns U[.., j*k .. j*k+k-1]), x [N][ldx] (k == 3: the highway input), bias
 *            [2 * ncols] = b_f | b_r; writes h and c, dense [N][ncols]; with nx_b also the bf16 images of h * nx_mul[b][col]
 *            (nx_mul [B][ncols] or null = 1): nx_b [N][ld_nxb] and, unless null, nx_bt [ncols][ld_nxbt]
 *   backward (backward != 0): reads U, x, bias, the stash c [N][ncols], dh [N][ncols] -- taken as dh * up_mul[b][col] + up_add[row][col]
 *            (up_mul [B][ncols] / up_add [N][ld_up_add], either null) --; writes dU [N][ldu] (the pitch of U), k == 3: dx [N][lddx],
 *            dbias_part [B][2 * ncols]; with dU_b the bf16 images dU_b [N][ld_dub] and, unless null, dU_bt [ncols * k][ld_dubt]
 *            INSTEAD of dU (dx is still written)
 * act: 0 identity, 1 tanh, 2 relu.  mask_mode: 0 none; 1 `mask` [B][ncols] of 0 / 1 scaled by keep_scale; 2 the Philox stream of
 * (key0, key1): column col of sequence seq_add + seq_mul * b is kept iff the first word of philox4x32_10(sequence, col, key0, key1)
 * >= p * 2^32, and scaled by 1 / (1 - p).
 * Images are raw 16-bit elements, pitches in elements; they need a cooperative form, T % 8 == 0, H % 64 == 0, 16-byte aligned
 * pointers and pitches that are multiples of 8.  Synchronises the stream.  A malformed case returns GT_ERR_INVALID before any launch. */
typedef struct gt_sru_scan_case {
  int32_t backward;
  int32_t B, T, H, dirs, k, act;
  int32_t mask_mode;
  float keep_scale, p;
  uint32_t key0, key1;
  int32_t seq_mul, seq_add;
  int32_t ldu, ldx, lddx, ld_up_add, ld_nxb, ld_dub;
  int64_t ld_nxbt, ld_dubt;
  const float* U;
  const float* x;
  const float* bias;
  float* h;
  float* c;
  const float* dh;
  float* dU;
  float* dx;
  float* dbias_part;
  const float* mask;
  const float* up_mul;
  const float* up_add;
  const float* nx_mul;
  uint16_t* nx_b;
  uint16_t* nx_bt;
  uint16_t* dU_b;
  uint16_t* dU_bt;
} gt_sru_scan_case;
int gt_op_sru_scan(const gt_sru_scan_case* c, void* stream);
/* Parity hooks of the helper kernels of the SRU stack, each one launch through the engine's launch function; they synchronise the stream.
 *   dx_adv_finish  dx_adv [rows][Da] dense, in place: dx_adv * mul[row / T][j] + hw[row][j]; mul [rows / T][ld_mul] or null (1),
 *                  hw [rows][ld_hw] or null (0)
 *   input_mask     mul [B][n] = inj[b][j] != 0 (inj [B][n] of 0 / 1), or without inj the Philox stream of the scans' mask_mode 2, times
 *                  1 / (1 - p), else 0
 *   input_dropout  y [B * T][ldy] = x [B * T][ldx] * mul[row / T][j], n columns */
int gt_op_sru_dx_adv_finish(float* dx_adv, int64_t rows, int Da, int T, const float* mul, int ld_mul, const float* hw, int ld_hw,
                            void* stream);
int gt_op_sru_input_mask(float* mul, int B, int n, float p, uint32_t key0, uint32_t key1, const float* inj, int seq_mul, int seq_add,
                         void* stream);
int gt_op_sru_input_dropout(const float* x, int ldx, float* y, int ldy, int B, int T, int n, const float* mul, void* stream);

/* Launches of the discriminator's tail (frame_kernels.hip.h: d_head_kernel, d_head_finalize_kernel; dstack_f32.hip.h: dstack_kernel) by
 * kernel, process-wide, counted on the host where each launch is issued (no device work, no synchronisation).  Slots:
 *   0..3     d_head_kernel<KP, float>, 4-byte accesses:        log2(KP) - 1, KP = 2, 4, 8, 16   (K <= 64 KP)
 *   4..6     d_head_kernel<KP, float, false, VEC>, head_vec:   4 + log2(KP) - 2, KP = 4, 8, 16
 *   7..10    d_head_kernel<KP, bf16, B16OUT>, the image form:  7 + log2(KP) - 1, KP = 2, 4, 8, 16
 *   11, 12   dstack_kernel<128>, dstack_kernel<256>
 *   13, 14   d_head_finalize_kernel with 64 / with 16 columns per workgroup (the latter with the extra scalar workgroup)
 * A launch is counted in the slot of its FORM whatever its adversarial objective (GT_OPT_GAN_OBJECTIVE): the objective is a further
 * template parameter of d_head_kernel and dstack_kernel and changes neither the dispatch nor the number of launches.
 * Copies the GT_HEAD_PATH_SLOTS counts to `counts` (may be null); reset != 0 then zeroes them. */
#define GT_HEAD_PATH_SLOTS 15
int gt_head_path_counts(int64_t* counts, int reset);

/* Parity hooks of the spectral normalisation (gt_set_spectral_norm), through the launch functions the step calls.  The job table: n_layers
 * weights inside a flat float32 buffer of n_flat elements, layer q = (w_off[q], out[q], in[q]) in ascending, non-overlapping order; its
 * u slice starts at sum(out[0 .. q)), its v slice at sum(in[0 .. q)).  Whatever lies between the weights (biases) is never read by
 * gt_op_spectral_norm and only squared by gt_op_sn_project.  All pointers are device memory; no synchronisation.
 * Arithmetic: products of two float32 values in double (exact), two-stage double sums in an order fixed by the table, no atomics
 * (bit-identical from run to run); u', v', sigma rounded to float32 once; W / sigma the correctly rounded float32 quotient.
 *   gt_op_spectral_norm   iterate != 0: one power iteration, u and v advanced in place (3 launches); iterate == 0: the eval form, u and v
 *                         only read (2 launches).  Writes sigma [n_layers] and the weight ranges of weff [n_flat] (nothing else of it).
 *   gt_op_sn_project      G [n_flat] (d loss / d W_eff in the weight ranges) -> d loss / d W in place, element (i, j) of a layer as
 *                         ((G - (float(s) * u_i) * v_j) / sigma) in float32 without contraction, s = sum G (.) weff of the layer in double
 *                         -> s [n_layers].  norm_partials [norm_cap]: *n_norm_partials doubles whose sum is the squared norm of ALL of G
 *                         afterwards, biases included (what the fused clip + update launch takes).  2 launches.
 * gt_sn_path_counts: launches by kernel, process-wide, counted on the host: 0 W^T u, 1 W v, 2 normalise + W_eff, 3 partial sums of
 * G (.) W_eff, 4 the element pass. */
#define GT_SN_MAX_LAYERS 17
#define GT_SN_PATH_SLOTS 5
typedef struct gt_sn_case {
  int32_t n_layers, iterate;
  int64_t n_flat, norm_cap;
  int64_t w_off[GT_SN_MAX_LAYERS];
  int32_t out[GT_SN_MAX_LAYERS], in[GT_SN_MAX_LAYERS];
  const float* W;              /* gt_op_spectral_norm: the flat buffer */
  float* u;
  float* v;
  float* weff;
  float* sigma;                /* [n_layers]: written by gt_op_spectral_norm, read by gt_op_sn_project */
  float* G;                    /* gt_op_sn_project */
  double* s;
  double* norm_partials;
  int32_t* n_norm_partials;    /* host */
} gt_sn_case;
int gt_op_spectral_norm(const gt_sn_case* c, void* stream);
int gt_op_sn_project(const gt_sn_case* c, void* stream);
int gt_sn_path_counts(int64_t* counts, int reset);

/* One dropout site of the tail hooks: mode 0 none, 1 the Philox keep bits of (key0, key1) at drop probability p, 2 the 0 / 1 float
 * `mask` [rows][ld_mask] (p still gives the scale 1 / (1 - p)).  dp_*: the data-parallel row-group map of the Philox counter
 * (dp_t16 == 0: identity), the fields of the same name of the engine's dropout sites: dp_t16 = T / 16, dp_nl16 = 16-row groups per half
 * (0xffffffff: one block of rows), dp_half = B_global T / 16 - dp_nl16, dp_add = rank T / 16, dp_mul = (world - 1) T / 16,
 * dp_inv_t16 = 1 / dp_t16. */
typedef struct gt_drop_site {
  int32_t mode;
  float p;
  uint32_t key0, key1;
  uint32_t dp_t16, dp_nl16, dp_half, dp_add, dp_mul;
  float dp_inv_t16;
  int32_t ld_mask, pad_;
  const float* mask;
} gt_drop_site;

/* Parity hook of the gradient penalties (gt_set_grad_penalty): the four parts of the second-order pass through the launch functions the
 * step calls, over `rows` rows of an MLP with L hidden layers of width H whose first layer reads [cd conditioning | Da adversarial]
 * columns.  All pointers but the case itself are device memory; no synchronisation.
 *   reads    W[l] dense (H, in_l) with in_0 = cd + Da and in_l = H above; w_last [H]; Hact[l] [rows][H], the stored activations, and drop[l],
 *            the dropout site each was stored under; mask [rows]; inv_tv = 1 / T
 *   writes   a[l], c[l] [rows][H] (the gradient and tangent chains); g_copy [rows][ld_g] (may be null): g; g [rows][ld_g]: r (pad columns
 *            [Da, ld_g) zero); phi, nrm [rows]: per-row phi and n; sums [2] doubles: sum mask phi, sum mask n (before the 1 / T);
 *            rec [3] doubles or null: {sum P, sum mean-norm, steps} += {sums[0] / T, sums[1] / T, 1}
 *   adds     dW[0][:, cd : cd + Da] += a_0^T r;  dW[l] += a_l^T c_{l-1};  dw_last [H] += column sums of c_{L-1}.  Nothing else of a gradient
 *            buffer is written: no bias gradient, no dW[0][:, :cd].
 * gt_gp_path_counts: process-wide, counted on the host: 0 gp_interp, 1 gp_slope, 2 gp_row, 3 gp_finalize, 4 gp_add_cols (launches); 5
 * backward-data, 6 forward, 7 weight-gradient calls of the product family (their launches are in gt_gemm_path_counts).  A pass over L
 * layers issues L + 1 slope, 1 row, 1 finalize, 1 add_cols launches and L backward-data, L forward, L + 1 weight-gradient calls. */
#define GT_GP_MAX_LAYERS 16
#define GT_GP_PATH_SLOTS 8
typedef struct gt_gp_case {
  int32_t kind, L, H, cd, Da, ld_g;      /* kind: 1 r1, 2 wgan-gp */
  int64_t rows;
  float weight, inv_tv;
  const float* W[GT_GP_MAX_LAYERS];
  float* dW[GT_GP_MAX_LAYERS];
  const float* Hact[GT_GP_MAX_LAYERS];
  float* a[GT_GP_MAX_LAYERS];
  float* c[GT_GP_MAX_LAYERS];
  gt_drop_site drop[GT_GP_MAX_LAYERS];
  const float* w_last;
  float* dw_last;
  const float* mask;
  float* g;
  float* g_copy;
  float* phi;
  float* nrm;
  double* sums;
  double* rec;
} gt_gp_case;
int gt_op_grad_penalty(const gt_gp_case* c, void* stream);
int gt_gp_path_counts(int64_t* counts, int reset);

/* Parity hook of the discriminator's per-layer head: ONE head pass plus its finalising launch through the launch function the engine
 * uses (launch_d_head), so the kernel form follows from K (KP), h_ld (> 0: the bf16 image form) and the tuning knob head_vec exactly as
 * in a step.  All pointers but `scalars` are the caller's device buffers.
 *   reads    H: float32 [rows][ldh], or (h_ld > 0) raw 16-bit bf16 [rows][h_ld]; w [K], bias [1]; mask [n_mask], row r -> mask[r % n_mask];
 *            mode 0 (D step): rows [0, n_real) natural, the rest generated; mode 1 (adversarial term): every row scored as natural.
 *            has_act: H is LeakyReLU + dropout (site `drop`) of a pre-activation, and dH carries its derivative.
 *   normaliser, exactly one of: has_tv (the hook puts tv and 1 / tv into its scratch scalars), tv_dev (a device double the kernel reads
 *            and copies into the scalars), unit_tv (1)
 *   writes   Dout [rows] or null; with want_grad dH [rows][lddh] (float32), and in the image form dHb [rows][lddhb] / dHbT [K][lddhbt]
 *            (raw 16-bit, either null; dHbT 8-byte aligned, lddhbt % 4 == 0); with want_grad && want_w dW [K] and db [1] (+= if
 *            accumulate).  defer_scalars: the finalising launch is left to the caller (as the generator step's riders do) unless
 *            weight gradients are wanted.
 *   scalars  host, 8 doubles or null, filled after the stream is synchronised: s_real, s_fake, n_real_ok, n_fake_ok, s_adv, tv, inv_tv
 *            as the scratch scalars hold them (what no launch wrote stays NaN), and the number of partials (workgroups of the pass).
 *   objective  GT_OPT_GAN_OBJECTIVE id (0 .. 6): Dout, the sums and the seed gradient are that objective's; same kernel form, same slot of
 *            gt_head_path_counts
 * The partial buffers are scratch of the call, filled with NaN first.  A malformed case returns GT_ERR_INVALID before any launch. */
typedef struct gt_d_head_case {
  int32_t mode, K, ldh, h_ld;
  int32_t has_act, want_grad, want_w, defer_scalars;
  int32_t accumulate, unit_tv, has_tv, lddh;
  int32_t lddhb, objective;    /* GT_OPT_GAN_OBJECTIVE id of the pass, 0 .. 6 (formerly padding: a zero-initialised case is objective 0) */
  float eps, tv;
  int64_t rows, n_real, n_mask, lddhbt;
  gt_drop_site drop;
  const void* H;
  const float* w;
  const float* bias;
  const float* mask;
  const double* tv_dev;
  float* Dout;
  float* dH;
  uint16_t* dHb;
  uint16_t* dHbT;
  float* dW;
  float* db;
  double* scalars;
} gt_d_head_case;
int gt_op_d_head(const gt_d_head_case* c, void* stream);

/* Parity hook of the fused discriminator stack: ONE fused pass plus its finalising launch through launch_dstack_pass.  hidden_dim 128 or
 * 256, L = 1 .. 4 hidden layers of which layer 0's OUTPUT H0 [rows][hidden_dim] (dropout applied) is the input; W[l] [hidden][hidden],
 * b[l] for l = 1 .. L-1; drop[l] the dropout site of layer l = 0 .. L-1 (an injected mask has pitch hidden_dim); w_last [hidden],
 * b_last [1]; mask, n_real, eps, the normaliser and `scalars` as in gt_d_head_case.
 *   mode 0 (D step)  writes Hout[l] [rows][hidden] for every l = 1 .. L-1 that is given, Dout [rows] or null, and with want_grad dZtop
 *                    [rows][hidden], dW_last [hidden], db_last [1] (+= if accumulate)
 *   mode 1 (G step)  writes Dout and with want_grad gadv [rows][ld_gadv] = dZ_0 . W0[:, col0 .. col0 + Da), W0 [hidden][ldw0], Da 1 .. 64
 * A malformed case returns GT_ERR_INVALID before any launch. */
typedef struct gt_dstack_case {
  int32_t mode, L, hidden_dim, want_grad;
  int32_t accumulate, unit_tv, has_tv, ldw0;
  int32_t col0, Da, ld_gadv, objective;      /* as in gt_d_head_case */
  float eps, tv;
  int64_t rows, n_real, n_mask;
  gt_drop_site drop[4];
  const float* H0;
  const float* W[4];
  const float* b[4];
  const float* w_last;
  const float* b_last;
  const float* mask;
  const double* tv_dev;
  float* Hout[4];
  float* dZtop;
  float* Dout;
  float* dW_last;
  float* db_last;
  const float* W0;
  float* gadv;
  double* scalars;
} gt_dstack_case;
int gt_op_dstack(const gt_dstack_case* c, void* stream);

/* Parity hook of the per-frame kernels between the products of a G+D step (frame_kernels.hip.h): ONE launch function of frame_args.hip.h,
 * the function the step itself calls, with the step's freedom in the arguments.  `op` selects it; a, b, c, d, mask, idx, tv_dev, part_mge,
 * part_mse, hp, out, out2 are the caller's device buffers, every matrix with its row pitch in floats; sums, partials, scalars are host arrays.
 *   MASK_SUM       mask [n_mask], tv_override (> 0 wins over the sum), tv_dev (a device double, wins over both) -> scalars tv, inv_tv
 *   MASK_TOTAL     mask [n_mask] -> scalars tv_sum
 *   SQERR          a, b [rows][lda / ldb] over cols columns, mask [rows] -> partials, scalars s_mse (sum_partials_kernel); out != null: the
 *                  gradient [rows][ldo] = 2 w0 (a m - b m) m / tv
 *   G_LOSSES       (a, b) over cols columns -> the first n1 partials and s_mse, (c, d) over cols2 columns -> the rest and s_mge
 *   STATIC_GRAD    a = y_hat_static, b = y_static over cols columns, w0 = mge_w, idx = adv_inv [cols] with entries in [-1, cols2), c = leak,
 *                  d = gadv [rows][ldc / ldd] (each may be null), adv_w, leak_unnorm; out = gs [rows][ldo] or null; want_partial: partials
 *                  (and, without the rider, s_mge).  rider != 0: the finalisation workgroup, as FINALIZE_G_RIDER
 *   FINALIZE_G     finalize_g_kernel: 256 threads with part_mge / part_mse (device, n_mge / n_mse entries), one thread without; zero_gnorm
 *   FINALIZE_G_RIDER   finalize_g_rider_kernel; hp: device [n_hp][5] doubles (HeadPartials) or null; fin_out == 0: the sums only
 *   FINALIZE_D     finalize_d_kernel; zero_gnorm, tv_from_sum
 *   SCALE_INV_TV   out [rows * cols] *= 1 / tv
 *   HIGHWAY_FWD    out = a + b c (x, Tx, Gx); HIGHWAY_BWD: a = g, b = Tx, c = Gx -> out = dGx, out2 = dTz
 *   SIGMOID_GRAD   out (g, in place) *= a (1 - a)
 *   DROPOUT_APPLY  dense a -> out [rows][cols] (a == out allowed), site `drop`
 *   BUILD_ADV      a = fa (rows below split), b = fb (the rest), pitch lda, idx [cols] with entries in [0, lda) -> out [rows][ldo], ldo % 4 == 0,
 *                  16-byte aligned; rider 1: mask [n_mask] -> scalars tv, inv_tv (tv_override); rider 2: -> scalars tv_sum
 *   BUILD_CAT2     a = x dense [rows][cols], b = fa, c = fb (pitch ldb), idx [cols2] -> out [2 rows][ldo], columns [0, cols + cols2)
 *   REPITCH, DENSE_COPY   a [rows][lda] -> out [rows][ldo] (repitch: ldo % 4 == 0, 16-byte aligned, pad columns 0)
 *   PAD_ROWS       dense a [rows][cols] -> out [rows][ldo], pad columns 0;  TRANSPOSE: a [rows][lda] -> out [cols][ldo]
 * max_blocks: the cap on a reduction's workgroups, 0 for the engine's 1024.
 * The normaliser of an op that reads one: has_tv (the hook puts tv and 1 / tv into its scratch scalars), else mask [n_mask] with tv_override
 * / tv_dev, summed by the launch the step uses.  A reduction's mask has n_mask == rows entries.
 *   sums      host, 10 doubles or null: tv_sum, s_real, s_fake, n_real_ok, n_fake_ok, s_adv, s_mge, s_mse, gnorm2_d, gnorm2_g put into the
 *             scratch scalars before the launch (what a finalisation without partials reads)
 *   partials  host, partials_cap doubles, or null: the reduction's per-workgroup sums
 *   scalars   host, 26 doubles or null, filled after the stream is synchronised: tv, inv_tv and the ten sums as the scratch scalars hold
 *             them, the twelve results (loss_d, loss_fake_d, loss_real_d, real_correct, fake_correct, loss_mse, loss_mge, loss_adv, loss_g,
 *             gnorm_d, gnorm_g, tv), the number of partials, and G_LOSSES' n1.  What nothing wrote stays NaN.
 * The scratch scalars, results and partial buffers are filled with NaN first.  A malformed case returns GT_ERR_INVALID before any launch. */
enum {
  GT_FRAME_MASK_SUM = 0, GT_FRAME_MASK_TOTAL = 1, GT_FRAME_SQERR = 2, GT_FRAME_G_LOSSES = 3, GT_FRAME_STATIC_GRAD = 4, GT_FRAME_FINALIZE_G = 5,
  GT_FRAME_FINALIZE_G_RIDER = 6, GT_FRAME_FINALIZE_D = 7, GT_FRAME_SCALE_INV_TV = 8, GT_FRAME_HIGHWAY_FWD = 9, GT_FRAME_HIGHWAY_BWD = 10,
  GT_FRAME_SIGMOID_GRAD = 11, GT_FRAME_DROPOUT_APPLY = 12, GT_FRAME_BUILD_ADV = 13, GT_FRAME_BUILD_CAT2 = 14, GT_FRAME_REPITCH = 15,
  GT_FRAME_DENSE_COPY = 16, GT_FRAME_PAD_ROWS = 17, GT_FRAME_TRANSPOSE = 18
};
typedef struct gt_frame_case {
  int32_t op, max_blocks, cols, cols2;
  int32_t lda, ldb, ldc, ldd;
  int32_t ldo, ldo2, has_tv, want_partial;
  int32_t leak_unnorm, rider, fin_out, has_adv;
  int32_t zero_gnorm, tv_from_sum, n_mge, n_mse;
  int32_t n_hp, pad_;
  float tv, tv_override;
  float w0, adv_w, mse_w, mge_w;
  int64_t rows, split, n_mask, partials_cap;
  gt_drop_site drop;
  const float* a;
  const float* b;
  const float* c;
  const float* d;
  const float* mask;
  const int32_t* idx;
  const double* tv_dev;
  const double* part_mge;
  const double* part_mse;
  const double* hp;
  float* out;
  float* out2;
  const double* sums;
  double* partials;
  double* scalars;
} gt_frame_case;
int gt_op_frame(const gt_frame_case* c, void* stream);

/* Parity hook of banded MLPG: ONE forward or transpose launch through ensure_band and mlpg_forward / mlpg_backward, the functions the
 * step calls, with the step's own freedom in the arguments: column maps, pitches, and the masked-MSE gradient fused into the transpose.
 *   e        the engine: num_windows, the band cache and (mse_w != 0) the scalars; R [T][num_windows * T] as in gt_op_mlpg_forward
 *   scol, sstride   device int32 [Ds]: static column c reads / writes full-layout columns scol[c] + w * sstride[c], w < num_windows;
 *            sstride[c] == 0: a pass-through column (copied).  Both null: the engine's own maps (Ds is then the engine's, 0 accepted).
 *   forward  (backward == 0) reads y [B*T][ldy], writes ys [B*T][ldys] columns [0, Ds)
 *   backward reads gs [B*T][ldgs] columns [0, Ds), writes gy [B*T][ldgy] at the mapped columns only.  mse_w != 0 adds
 *            2 mse_w (yhat m - ytgt m) m / sum(m) with yhat, ytgt [B*T][ldt] and mask m [B*T]: the hook first puts sum(m) and its
 *            reciprocal into the engine's scalars with the launch the step uses.  mse_w == 0: yhat, ytgt, mask may be null.
 *   kb       host, or null: receives the half-width the band cache holds for (R, T), before the launchers' checks
 * Every pointer is checked, every pitch against the widest column the maps reach (the maps are copied to the host for this).  A
 * malformed case, and a band whose tiles exceed the device's LDS (see gt_op_mlpg_forward's launchers), returns GT_ERR_INVALID before
 * any MLPG launch. */
typedef struct gt_mlpg_case {
  int32_t backward, B, T, Ds;
  int32_t ldy, ldys, ldgs, ldgy;
  int32_t ldt;
  float mse_w;
  gt_engine* e;
  const float* R;
  const int32_t* scol;
  const int32_t* sstride;
  const float* y;
  float* ys;
  const float* gs;
  float* gy;
  const float* yhat;
  const float* ytgt;
  const float* mask;
  int32_t* kb;
} gt_mlpg_case;
int gt_op_mlpg(const gt_mlpg_case* c, void* stream);
/* Parity hook of the band cache: ensures the entry of (R or GT_MLPG_R_FROM_WINDOWS, T) as the MLPG entry points do, writes its half-width
 * to *kb (host, may be null) and copies the band image [T][num_windows][2 kb + 1] (band[t][w][j] = R[t][w*T + t + j - kb], zero where
 * t + j - kb is outside [0, T)) to band_host.  capacity: floats band_host holds; too few return GT_ERR_INVALID after *kb is written.
 * Synchronises the stream. */
int gt_op_mlpg_band(gt_engine* e, const float* R, int T, float* band_host, int64_t capacity, int32_t* kb, void* stream);

/* Variance-weighted MLPG: nnmnkwii.paramgen.mlpg(mean_frames, variance_frames, windows) for a batch, on the device.  For every sequence b
 * and static column c it solves, in float64 and over the sequence's OWN length len_b,
 *     (sum_w W_w^T diag(1 / var_w) W_w) x = sum_w W_w^T (y_w / var_w)
 * with the windows registered through gt_set_mlpg_windows, (W_w x)[t] = sum_k coef_w[k + l_w] x[t + k] (terms outside [0, len_b) dropped),
 * y_w[t] = y[b*T + t][scol[c] + w * sstride[c]] and var_w likewise: one thread per (b, c), a banded Cholesky with the forward substitution
 * riding along, the back substitution, the result rounded to float32 once (gantts_amd/csrc/mlpg_var_kernels.hip.h).
 *   e        the engine: num_windows, the registered windows, the scratch (8 (hb + 2) T Ds bytes per sequence, hb = max_w (l_w + u_w))
 *   y        device [B*T][ldy]: the means, static and dynamic features in the full layout
 *   var      device: [B*T][ldv] per frame, or ONE row of the full layout when ldv == 0 (time-invariant: the data variance of gen_parameters)
 *   ys       device [B*T][ldys], columns [0, Ds) written: the solution for t < len_b, 0 for t >= len_b; a pass-through column
 *            (sstride[c] == 0) is y's column scol[c] copied for t < len_b
 *   scol, sstride   device int32 [Ds] as in gt_mlpg_case; both null: the engine's own maps (Ds is then the engine's, 0 accepted)
 *   lengths  host, B entries in [1, T]; null: all T
 *   max_ws_bytes    cap of the scratch of one group of whole sequences the batch is walked in; 0: 64 MB.  A cap below one sequence's
 *            scratch is refused.  The result does not depend on the grouping.
 * Malformed cases -- no registered windows, a null pointer, T < 1, a length outside [1, T], a pitch below the columns the maps address --
 * return GT_ERR_INVALID before any launch.  A variance that is not a finite positive number (or a pivot that is not) returns GT_ERR_INVALID
 * ("variances must be finite and positive") AFTER the launch: nothing in ys is to be trusted then; the engine serves the next call.
 * Synchronises the stream: the refusal flag is read. */
typedef struct gt_mlpg_var_case {
  gt_engine* e;
  int32_t B, T, Ds;
  int32_t ldy, ldv, ldys;
  const int32_t* scol;
  const int32_t* sstride;
  const int64_t* lengths;
  const float* y;
  const float* var;
  float* ys;
  int64_t max_ws_bytes;
} gt_mlpg_var_case;
int gt_op_mlpg_var(const gt_mlpg_var_case* c, void* stream);
/* Launches of the variance-weighted solve by kernel, process-wide, counted on the host where each launch is issued (one per group of
 * sequences): 0 mlpg_var_solve_kernel<1>, 1 mlpg_var_solve_kernel<2>, 2 mlpg_var_generic_kernel.  Copies the first min(n,
 * GT_MLPG_VAR_PATH_SLOTS) counts to `counts`; counts == NULL zeroes them instead. */
#define GT_MLPG_VAR_PATH_SLOTS 3
int gt_mlpg_var_path_counts(int64_t* counts, int n);

/* Batch assembly from a device-resident corpus (gantts_amd/csrc/data_kernels.hip.h; gantts_amd/data.py: ResidentLoader): ONE launch
 * writes what the training loop derives from a batch -- TTSDataset / VCDataset.__getitem__, collate_fn, the length sort, torch.rand
 * + torch.cat, get_static_features and sequence_mask (train.py:111-159, 494-519) -- bit for bit as the host pipeline computes it.
 * Stateless; every pointer is caller-owned device memory; no synchronisation.
 *   X_all [F][ldX], Y_all [F][ldY]   the un-normalised utterances back to back; 16-byte aligned, ldX and ldY multiples of 4
 *   x_kind / y_kind   GT_SCALE_NONE, GT_SCALE_MINMAX (v * a[c] + b[c]: a = scale_, b = min_) or GT_SCALE_MEANVAR ((v - a[c]) / b[c]:
 *            a = mean, b = std); x_a, x_b [Dx] are float64 when stats_f64 & 1, y_a, y_b [Dy] when stats_f64 & 2, float32 otherwise.
 *            The arithmetic of a side runs in its statistics' dtype, each operation rounded on its own (no FMA, correctly rounded division), one rounding to float32.
 *   table    [n_slots][3] int64: first frame, length, corpus utterance index of every batch slot of the epoch; sequence b of this
 *            call is slot first_slot + b.  A slot that does not lie inside [0, F) yields an empty sequence; a length above T is cut.
 *   gi       (B, T, Dx + nz) on pitch ld_gi (a multiple of 4, 16-byte aligned): columns [0, Dx) the scaled x, 0 at frames
 *            t >= length; [Dx, Dx + nz) noise z in [0, 1) on every frame; pad columns 0.  z[t][j] of utterance u is word j & 3 of
 *            Philox4x32-10(counter = (u, t * ceil(nz / 4) + (j >> 2)), key = (key0, key1)), (word >> 8) * 2^-24.
 *   y        (B, T, Dy) on pitch ld_y;  y_static (B, T, Ds) on pitch ld_ys: columns scol[j] (device int32 [Ds]) of that y;
 *            mask (B, T) float 0 / 1;  lengths (B) int64.  Any output may be null.  Padded frames and pad columns are 0.
 *   dsrc, dwin, n_windows, win_len, coef   delta recomputation (gantts/multistream.py:15-30), both lists null for none: column c of y
 *            with dwin[c] = w >= 0 is sum_k coef[w][k] * scaled(Y)[t + k - (win_len[w] - 1) / 2][dsrc[c]] over the frames of the
 *            UTTERANCE (zeros beyond its edges), accumulated in double and rounded once; dwin[c] < 0 is the plain scaled column.
 * A malformed case (null corpus, sizes < 1, a pitch below its width or not a multiple of 4 where 16-byte access needs it, widths
 * whose statistics do not fit the workgroup's LDS) returns GT_ERR_INVALID before the launch. */
#define GT_SCALE_NONE 0
#define GT_SCALE_MINMAX 1
#define GT_SCALE_MEANVAR 2
#define GT_ASSEMBLE_MAX_WINDOWS 4
#define GT_ASSEMBLE_MAX_TAPS 9
typedef struct gt_assemble_case {
  int32_t B, T, Dx, Dy, nz, Ds;
  int32_t ldX, ldY, ld_gi, ld_y, ld_ys;
  int32_t x_kind, y_kind, stats_f64, n_windows;
  uint32_t key0, key1;
  int32_t win_len[GT_ASSEMBLE_MAX_WINDOWS];
  int32_t pad_;
  int64_t F, n_slots, first_slot;
  double coef[GT_ASSEMBLE_MAX_WINDOWS][GT_ASSEMBLE_MAX_TAPS];
  const float* X_all;
  const float* Y_all;
  const void* x_a;
  const void* x_b;
  const void* y_a;
  const void* y_b;
  const int64_t* table;
  const int32_t* scol;
  const int32_t* dsrc;
  const int32_t* dwin;
  float* gi;
  float* y;
  float* y_static;
  float* mask;
  int64_t* lengths;
} gt_assemble_case;
int gt_op_assemble_batch(const gt_assemble_case* c, void* stream);

/* One data-parallel rank's share of a batch, by the same kernel.  Whole sequences are dealt round-robin: local sequence b of rank r is
 * sequence r + world * b of the length-sorted batch, table slot first_slot + rank + b * world.  c->B is the LOCAL sequence count,
 * ceil((B_global - rank) / world) and at least 1; c->T is the T of the WHOLE batch (every rank pads to it: MLPG is built for the padded
 * length); every output of gt_op_assemble_batch keeps its meaning for the local rows, lengths is the local (B).  The noise of a row is
 * keyed by its corpus utterance, so the ranks' rows are the rows of the whole batch.
 *   tv_global   device double, 8-byte aligned, may be null: receives sum of min(length, T) over the B_global slots of the whole
 *               batch (a slot that does not lie inside [0, F) counts 0) -- the loss normaliser of the data-parallel step
 *               (gt_set_loss_normalizer_device).  Written by the launch itself (workgroup 0; an int64 sum, one conversion, one store):
 *               exact, identical on every rank, no atomics, no second launch, no host read.
 * Everything gt_op_assemble_batch checks is checked the same way (the table must hold the slots [first_slot, first_slot + B_global));
 * a null shard, world < 1, a rank outside [0, world), B_global < 1, a c->B that is not the rank's share (a share of 0 included) and a
 * misaligned tv_global return GT_ERR_INVALID before the launch.  rank 0 of world 1 writes what gt_op_assemble_batch writes. */
typedef struct gt_assemble_shard {
  int32_t rank, world;
  int32_t B_global, pad_;
  double* tv_global;
} gt_assemble_shard;
int gt_op_assemble_shard(const gt_assemble_case* c, const gt_assemble_shard* s, void* stream);

/* Normalisation statistics of one side of a device-resident corpus in one pass (gantts_amd/csrc/corpus_stats_kernels.hip.h; gantts_amd/data.py:
 * ResidentCorpus.minmax / .meanvar): what data.minmax and data.meanvar compute on the host (train.py:718-751).  Stateless; every pointer is
 * caller-owned device memory; no synchronisation; two launches on `stream`, no atomics, bit-identical from run to run.
 *   A        [F][ld] float32, ld = roundup(D, 4), 16-byte aligned; the pad columns [D, ld) reach no result
 *   seg      [n_seg][2] int64 = (first frame, valid frame count) in ascending order, none beginning before the previous one ends: the
 *            valid rows.  A segment that does not lie inside [0, F) counts as empty; rows outside every segment are not counted.
 *   prior_mean, prior_var [D] float64 (null: zeros), prior_count: the statistics continue from these (M2 = prior_var * prior_count), as
 *            meanvar(..., mean_=, var_=, last_sample_count=) does; an empty selection returns the prior.
 *   workspace   gt_corpus_stats_workspace_bytes(F, D) bytes, 16-byte aligned: one partial per slab of GT_CORPUS_STATS_SLAB rows.
 *   out_min, out_max [D] float32: numpy's min / max (a NaN makes its column NaN; +inf / -inf of an empty selection);
 *   out_count, out_mean, out_m2 [D] float64: the number of valid rows (+ prior_count), the mean and M2 = sum (x - mean)^2 (Welford per lane,
 *            Chan's pairwise update between lanes, waves, slabs -- GT_CORPUS_STATS_FANIN partial chains per column -- and with the prior; no
 *            sum of squares anywhere: a constant column has M2 exactly 0).
 * A malformed case returns GT_ERR_INVALID before any launch. */
#define GT_CORPUS_STATS_SLAB 256
#define GT_CORPUS_STATS_FANIN 64
typedef struct gt_corpus_stats_case {
  int32_t D, ld;
  int64_t F, n_seg, prior_count;
  const float* A;
  const int64_t* seg;
  const double* prior_mean;
  const double* prior_var;
  void* workspace;
  int64_t workspace_bytes;
  float* out_min;
  float* out_max;
  double* out_count;
  double* out_mean;
  double* out_m2;
} gt_corpus_stats_case;
int64_t gt_corpus_stats_workspace_bytes(int64_t F, int32_t D);
int gt_op_corpus_stats(const gt_corpus_stats_case* c, void* stream);

/* ---- measurement (bench.py): HIP-event timing of every GEMM launch on its own stream --------
 * One slot per KERNEL (template instantiation family), so that the figures line up with a rocprofv3 kernel trace:
 *   0..5  = kind*2 + (tile N == 128), kind: 0 forward (X W^T), 1 backward-data (dZ W), 2 backward-weight (dZ^T X) -- the
 *           instantiations whose epilogue flavour is decided at run time, and every bf16-storage product;
 *   6, 7  = 64x64 forward kernels with a compiled-in epilogue: none / LeakyReLU + Philox dropout;
 *   8     = pair launches (one layer's backward-data product and weight gradient in one launch);
 *   9     = 64x64 forward, LeakyReLU + Philox dropout on (product + added matrix): the split first layer of the conditioned D;
 *   10,11 = 64x64 backward-data kernels with a compiled-in epilogue: none / LeakyReLU + Philox;
 *   12    = the two weight-gradient products of a split first layer in one launch;
 *   13    = the split first layer's forward in one launch (two K segments, two result halves);
 *   14    = the fused discriminator stack (GT_OPT_FUSED_DSTACK: layers 1..L-1 + head [+ backward-data chain] of one pass);
 *   15    = the fused clip + update launch of either network (kind 8; no flops, bytes = 16 + 8 per live state buffer + 8 with the weight
 *           average, per parameter).  Instrumented ONLY when selected by its kind, gt_profile_enable(2 + 8): (1) leaves it alone.
 * flops are algorithmic 2*M*N*K of the unpadded problems.  The three arrays hold GT_PROFILE_SLOTS entries.
 * gt_profile_enable(0) off, (1) every product launch, (2 + k) only launches of kind k (5 = the pair launches: what bench.py samples
 * inside its timed region -- two events per launch are not free). */
#define GT_PROFILE_SLOTS 16
int gt_profile_enable(int on);
int gt_profile_read(double* ms_per_slot, double* flops_per_slot, int64_t* launches_per_slot);
/* algorithmic HBM bytes (each operand once + the result once, fp32) of the launches the last gt_profile_read summed */
int gt_profile_bytes(double* bytes_per_slot);

#ifdef __cplusplus
}
#endif
#endif /* GANTTS_HIP_H_ */
