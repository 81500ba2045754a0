"""ctypes binding of libgantts_hip.so (C ABI declared in include/gantts_hip.h).

The HIP library is the product: if it is missing or fails to load this module raises --
there is no CPU or PyTorch fallback.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C gantts_amd/csrc``.
"""
import ctypes as C
import os

# PyTorch-ROCm first: it carries its own HIP runtime (libamdhip64 of its wheel).  Loaded first, the dynamic loader resolves this library's
# libamdhip64 dependency to that SAME copy; loaded second it maps a second runtime beside the system one and every HIP call of the process
# that lands in the late copy fails with "no ROCm-capable device is detected" (seen in round 6 when build() imported the package before
# smoke() imported torch, in one process).  The tensors the step functions take are torch tensors: torch is a dependency either way.
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GT_HIP_LIB") or os.path.join(_HERE, "libgantts_hip.so")      # GT_HIP_LIB: A/B of two builds (tools/)

GT_OK, GT_ERR_INVALID, GT_ERR_HIP, GT_ERR_STATE, GT_ERR_DIM = 0, 1, 2, 3, 4
ROLE_G, ROLE_D = 0, 1
OPT_LSTM_PERSISTENT, OPT_LSTM_FWD_UNITS, OPT_LSTM_XCD_LOCAL, OPT_MATMUL_BF16, OPT_SPLIT_FIRST_LAYER = 2, 3, 4, 5, 6
OPT_COMM_D_ONE_MSG, OPT_COMM_EARLY_G, OPT_COMM_FORCE = 10, 11, 13      # (7, 8, 9, 12: retired, not reused)
OPT_LAUNCH_RIDERS, OPT_COMM_CLOSE_INLINE, OPT_POLL_RESULTS = 14, 15, 16
OPT_COMM_TV_IN_SUMS, OPT_COMM_IPC, OPT_FUSED_DSTACK = 17, 18, 19
OPT_SRU_D_BF16 = 20
OPT_GAN_OBJECTIVE = 21
# GT_OPT_GAN_OBJECTIVE ids by hp.gan_objective name, and the "correct" threshold of D(x) under each (sigmoid output: 0.5; ls scores z
# against the labels 0 / 1: 0.5; hinge and wgan: the sign of z)
GAN_OBJECTIVES = {"bce": 0, "ls": 1, "hinge": 2, "wgan": 3}
GAN_OBJECTIVE_THRESHOLD = {"bce": 0.5, "ls": 0.5, "hinge": 0.0, "wgan": 0.0}
# the f-GAN divergences (Nowozin et al. 2016) of the same option, in tables of their own: ids and the "correct" threshold on z,
# g_f(z) > f'(1) (kl: z > 1; reverse kl and Jensen-Shannon: z > 0)
GAN_F_DIVERGENCES = {"kl": 4, "rkl": 5, "js": 6}
GAN_F_DIVERGENCE_THRESHOLD = {"kl": 1.0, "rkl": 0.0, "js": 0.0}
IPC_HANDLE_BYTES, IPC_MAX_WORLD = 64, 8
PROFILE_SLOTS = 16
LSTM_PATH_SLOTS, LSTM_PATH_STEPS, LSTM_PATH_DECLINED = 34, 32, 33      # gt_lstm_path_counts
GEMM_PATH_SLOTS = 588                                                   # gt_gemm_path_counts
GEMM_B16_PATH_SLOTS = 66                                                # gt_gemm_b16_path_counts
SRU_PATH_SLOTS = 13                                                     # gt_sru_path_counts
HEAD_PATH_SLOTS = 15                                                    # gt_head_path_counts
SN_MAX_LAYERS, SN_PATH_SLOTS = 17, 5                                    # GT_SN_MAX_LAYERS; gt_sn_path_counts: W^T u, W v, normalise + W_eff, G (.) W_eff partials, element pass
GP_MAX_LAYERS, GP_PATH_SLOTS = 16, 8                                    # GT_GP_MAX_LAYERS; gt_gp_path_counts: gp_interp, gp_slope, gp_row, gp_finalize, gp_add_cols launches, then backward-data, forward, weight-gradient calls
GRAD_PENALTIES = {None: 0, "r1": 1, "wgan-gp": 2}                       # gt_set_grad_penalty kinds by hp.discriminator_grad_penalty name
(FRAME_MASK_SUM, FRAME_MASK_TOTAL, FRAME_SQERR, FRAME_G_LOSSES, FRAME_STATIC_GRAD, FRAME_FINALIZE_G, FRAME_FINALIZE_G_RIDER, FRAME_FINALIZE_D,
 FRAME_SCALE_INV_TV, FRAME_HIGHWAY_FWD, FRAME_HIGHWAY_BWD, FRAME_SIGMOID_GRAD, FRAME_DROPOUT_APPLY, FRAME_BUILD_ADV, FRAME_BUILD_CAT2, FRAME_REPITCH,
 FRAME_DENSE_COPY, FRAME_PAD_ROWS, FRAME_TRANSPOSE) = range(19)         # FrameCase.op
FRAME_SCALARS = 26                                                      # doubles gt_op_frame reports
CAST_PLAIN_F32, CAST_PLAIN_BF16, CAST_SEQDROP, CAST_CAT, CAST_CATDROP, CAST_MULTI = 0, 1, 2, 3, 4, 5      # CastCase.kind
CAST_MAX_JOBS = 8
GEMM_ROUTE_FORWARD, GEMM_ROUTE_FORWARD_SEG, GEMM_ROUTE_BACKWARD_DATA, GEMM_ROUTE_WEIGHT_GRAD, GEMM_ROUTE_WEIGHT_GRAD_SPLIT = 0, 1, 2, 3, 4
ARCH_MLP, ARCH_IN2OUT, ARCH_LSTM, ARCH_SRU, ARCH_IN2OUT_RNN = 0, 1, 2, 3, 4
OPT_ADAGRAD, OPT_ADAM = 0, 1
OPT_SGD, OPT_RMSPROP, OPT_ADADELTA, OPT_ADAMW, OPT_ADAMAX = 2, 3, 4, 5, 6
OPT_NADAM, OPT_RADAM, OPT_RPROP, OPT_ASGD = 7, 8, 9, 10
OPTF_NESTEROV, OPTF_CENTERED, OPTF_AMSGRAD, OPTF_BUFFER_LIVE = 1, 2, 4, 8      # OptimDescEx.flags
OPTF_DECOUPLED_WD = 32                                                         # NAdam, RAdam
MLPG_VAR_PATH_SLOTS = 3                                                 # gt_mlpg_var_path_counts: solve<1>, solve<2>, generic
MAX_STREAMS = 8
MLPG_R_FROM_WINDOWS = 1                 # GT_MLPG_R_FROM_WINDOWS: "build the band from the registered windows", passed in place of R
MLPG_MAX_WINDOW_SPAN = 32               # GT_MLPG_MAX_WINDOW_SPAN
COMM_ID_BYTES = 128
SCALE_NONE, SCALE_MINMAX, SCALE_MEANVAR = 0, 1, 2      # AssembleCase.x_kind / y_kind
ASSEMBLE_MAX_WINDOWS, ASSEMBLE_MAX_TAPS = 4, 9
CORPUS_STATS_SLAB, CORPUS_STATS_FANIN = 256, 64        # GT_CORPUS_STATS_SLAB / _FANIN: rows per workgroup, partial chains per column of the merge
LEDGER_SLOTS = 32                                      # GT_LEDGER_SLOTS: doubles of the epoch ledger's record
LEDGER_HAS_D, LEDGER_HAS_G, LEDGER_HAS_DIST = 1, 2, 4  # gt_ledger_add / gt_op_epoch_ledger flags
LEDGER_ACOUSTIC, LEDGER_DURATION, LEDGER_VC = 0, 1, 2  # ... kind
# slot i of the record holds the running sum named LEDGER_KEYS[i]; the slots behind them are reserved
LEDGER_KEYS = ("generator", "mse", "mge", "loss_real_d", "loss_fake_d", "loss_adv", "discriminator", "real_correct", "fake_correct",
               "mcd", "bap_mcd", "f0_rmse", "vuv_err", "dur_rmse", "d_updates", "g_updates")


class StreamConfig(C.Structure):
    _fields_ = [("n_streams", C.c_int32),
                ("stream_sizes", C.c_int32 * MAX_STREAMS),
                ("has_dynamic_features", C.c_int32 * MAX_STREAMS),
                ("num_windows", C.c_int32),
                ("adversarial_streams", C.c_int32 * MAX_STREAMS),
                ("mask_nth_mgc_for_adv_loss", C.c_int32),
                ("discriminator_linguistic_condition", C.c_int32),
                ("cond_dim", C.c_int32)]


class ModelDesc(C.Structure):
    _fields_ = [("arch", C.c_int32), ("in_dim", C.c_int32), ("out_dim", C.c_int32),
                ("num_hidden", C.c_int32), ("hidden_dim", C.c_int32), ("static_dim", C.c_int32),
                ("dropout", C.c_float), ("last_sigmoid", C.c_int32),
                ("bidirectional", C.c_int32), ("use_relu", C.c_int32),
                ("rnn_dropout", C.c_float), ("reserved_", C.c_int32),
                ("params", C.c_void_p), ("grads", C.c_void_p), ("n_params", C.c_int64)]


class OptimDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lr", C.c_float), ("weight_decay", C.c_float), ("eps", C.c_float),
                ("lr_decay", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float),
                ("max_grad_norm", C.c_float), ("step", C.c_int64),
                ("state0", C.c_void_p), ("state1", C.c_void_p)]


class OptimDescEx(C.Structure):
    _fields_ = ([("kind", C.c_int32), ("flags", C.c_uint32)]
                + [(n, C.c_double) for n in ("lr", "weight_decay", "eps", "lr_decay", "beta1", "beta2", "momentum", "dampening", "alpha")]
                + [("max_grad_norm", C.c_float), ("reserved_", C.c_int32), ("step", C.c_int64),
                   ("state0", C.c_void_p), ("state1", C.c_void_p), ("state2", C.c_void_p)])


class OptimDescEx2(OptimDescEx):
    """The whole gt_optim_desc_ex.  OptimDescEx is its head up to state2: all the library reads for OPT_ADAGRAD .. OPT_ADAMAX, and
    what a caller of the first family passes; OPT_NADAM .. OPT_ASGD need the tail."""
    _fields_ = [(n, C.c_double) for n in ("momentum_decay", "etaminus", "etaplus", "step_size_min", "step_size_max", "lambd", "t0",
                                          "host_state0", "host_state1")]


class DResult(C.Structure):
    _fields_ = [("loss_d", C.c_float), ("loss_fake_d", C.c_float), ("loss_real_d", C.c_float),
                ("real_correct_count", C.c_float), ("fake_correct_count", C.c_float), ("grad_norm", C.c_float)]


class GResult(C.Structure):
    _fields_ = [("loss_mse", C.c_float), ("loss_mge", C.c_float), ("loss_adv", C.c_float),
                ("loss_g", C.c_float), ("grad_norm", C.c_float)]


class GemmCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("route", "prec", "rows", "in_dim", "out_dim", "act", "drop")] + [("p", C.c_float)]
                + [("key0", C.c_uint32), ("key1", C.c_uint32)]
                + [(n, C.c_int32) for n in ("accumulate", "col0", "ncols", "wrap", "cd", "rider", "defer", "ldx", "ldw", "ldy", "ld_dy",
                                            "ldh", "ld_mask", "ld_addm", "ld_adv", "ld_dx")]
                + [(n, C.c_void_p) for n in ("x", "w", "bias", "y", "dy", "h", "mask", "addm", "adv", "dx", "dw", "db")])


class GemmB16Case(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("route", "rows", "in_dim", "out_dim", "act", "drop")] + [("p", C.c_float)]
                + [("key0", C.c_uint32), ("key1", C.c_uint32)]
                + [(n, C.c_int32) for n in ("accumulate", "ldx", "ldw", "ld_dy", "ldh", "ld_mask", "ldc", "ldcb", "ldcbt")]
                + [(n, C.c_void_p) for n in ("x", "w", "bias", "dy", "h", "mask", "c", "cb", "cbt", "dw", "db")])


class SruScanCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("backward", "B", "T", "H", "dirs", "k", "act", "mask_mode")]
                + [("keep_scale", C.c_float), ("p", C.c_float), ("key0", C.c_uint32), ("key1", C.c_uint32)]
                + [(n, C.c_int32) for n in ("seq_mul", "seq_add", "ldu", "ldx", "lddx", "ld_up_add", "ld_nxb", "ld_dub")]
                + [("ld_nxbt", C.c_int64), ("ld_dubt", C.c_int64)]
                + [(n, C.c_void_p) for n in ("U", "x", "bias", "h", "c", "dh", "dU", "dx", "dbias_part", "mask", "up_mul", "up_add", "nx_mul",
                                             "nx_b", "nx_bt", "dU_b", "dU_bt")])


class DropSite(C.Structure):
    _fields_ = ([("mode", C.c_int32), ("p", C.c_float), ("key0", C.c_uint32), ("key1", C.c_uint32)]
                + [(n, C.c_uint32) for n in ("dp_t16", "dp_nl16", "dp_half", "dp_add", "dp_mul")]
                + [("dp_inv_t16", C.c_float), ("ld_mask", C.c_int32), ("pad_", C.c_int32), ("mask", C.c_void_p)])


class DHeadCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("mode", "K", "ldh", "h_ld", "has_act", "want_grad", "want_w", "defer_scalars", "accumulate", "unit_tv",
                                          "has_tv", "lddh", "lddhb", "objective")]
                + [("eps", C.c_float), ("tv", C.c_float)]
                + [(n, C.c_int64) for n in ("rows", "n_real", "n_mask", "lddhbt")]
                + [("drop", DropSite)]
                + [(n, C.c_void_p) for n in ("H", "w", "bias", "mask", "tv_dev", "Dout", "dH", "dHb", "dHbT", "dW", "db")]
                + [("scalars", C.POINTER(C.c_double))])


class DStackCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("mode", "L", "hidden_dim", "want_grad", "accumulate", "unit_tv", "has_tv", "ldw0", "col0", "Da",
                                          "ld_gadv", "objective")]
                + [("eps", C.c_float), ("tv", C.c_float)]
                + [(n, C.c_int64) for n in ("rows", "n_real", "n_mask")]
                + [("drop", DropSite * 4), ("H0", C.c_void_p), ("W", C.c_void_p * 4), ("b", C.c_void_p * 4)]
                + [(n, C.c_void_p) for n in ("w_last", "b_last", "mask", "tv_dev")]
                + [("Hout", C.c_void_p * 4)]
                + [(n, C.c_void_p) for n in ("dZtop", "Dout", "dW_last", "db_last", "W0", "gadv")]
                + [("scalars", C.POINTER(C.c_double))])


class FrameCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("op", "max_blocks", "cols", "cols2", "lda", "ldb", "ldc", "ldd", "ldo", "ldo2", "has_tv", "want_partial",
                                          "leak_unnorm", "rider", "fin_out", "has_adv", "zero_gnorm", "tv_from_sum", "n_mge", "n_mse", "n_hp", "pad_")]
                + [(n, C.c_float) for n in ("tv", "tv_override", "w0", "adv_w", "mse_w", "mge_w")]
                + [(n, C.c_int64) for n in ("rows", "split", "n_mask", "partials_cap")]
                + [("drop", DropSite)]
                + [(n, C.c_void_p) for n in ("a", "b", "c", "d", "mask", "idx", "tv_dev", "part_mge", "part_mse", "hp", "out", "out2")]
                + [("sums", C.POINTER(C.c_double)), ("partials", C.POINTER(C.c_double)), ("scalars", C.POINTER(C.c_double))])


class MlpgCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("backward", "B", "T", "Ds", "ldy", "ldys", "ldgs", "ldgy", "ldt")] + [("mse_w", C.c_float)]
                + [(n, C.c_void_p) for n in ("e", "R", "scol", "sstride", "y", "ys", "gs", "gy", "yhat", "ytgt", "mask")]
                + [("kb", C.POINTER(C.c_int32))])


class MlpgVarCase(C.Structure):
    _fields_ = ([("e", C.c_void_p)] + [(n, C.c_int32) for n in ("B", "T", "Ds", "ldy", "ldv", "ldys")]
                + [(n, C.c_void_p) for n in ("scol", "sstride")] + [("lengths", C.POINTER(C.c_int64))]
                + [(n, C.c_void_p) for n in ("y", "var", "ys")] + [("max_ws_bytes", C.c_int64)])


class AssembleCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("B", "T", "Dx", "Dy", "nz", "Ds", "ldX", "ldY", "ld_gi", "ld_y", "ld_ys", "x_kind", "y_kind",
                                          "stats_f64", "n_windows")]
                + [("key0", C.c_uint32), ("key1", C.c_uint32), ("win_len", C.c_int32 * ASSEMBLE_MAX_WINDOWS), ("pad_", C.c_int32)]
                + [(n, C.c_int64) for n in ("F", "n_slots", "first_slot")]
                + [("coef", (C.c_double * ASSEMBLE_MAX_TAPS) * ASSEMBLE_MAX_WINDOWS)]
                + [(n, C.c_void_p) for n in ("X_all", "Y_all", "x_a", "x_b", "y_a", "y_b", "table", "scol", "dsrc", "dwin", "gi", "y",
                                             "y_static", "mask", "lengths")])


class AssembleShard(C.Structure):
    _fields_ = [("rank", C.c_int32), ("world", C.c_int32), ("B_global", C.c_int32), ("pad_", C.c_int32), ("tv_global", C.c_void_p)]


class CorpusStatsCase(C.Structure):
    _fields_ = ([("D", C.c_int32), ("ld", C.c_int32)] + [(n, C.c_int64) for n in ("F", "n_seg", "prior_count")]
                + [(n, C.c_void_p) for n in ("A", "seg", "prior_mean", "prior_var", "workspace")] + [("workspace_bytes", C.c_int64)]
                + [(n, C.c_void_p) for n in ("out_min", "out_max", "out_count", "out_mean", "out_m2")])


class SnCase(C.Structure):
    _fields_ = ([("n_layers", C.c_int32), ("iterate", C.c_int32), ("n_flat", C.c_int64), ("norm_cap", C.c_int64),
                 ("w_off", C.c_int64 * SN_MAX_LAYERS), ("out", C.c_int32 * SN_MAX_LAYERS), ("in_", C.c_int32 * SN_MAX_LAYERS)]
                + [(n, C.c_void_p) for n in ("W", "u", "v", "weff", "sigma", "G", "s", "norm_partials")]
                + [("n_norm_partials", C.POINTER(C.c_int32))])


class GpCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("kind", "L", "H", "cd", "Da", "ld_g")] + [("rows", C.c_int64), ("weight", C.c_float), ("inv_tv", C.c_float)]
                + [(n, C.c_void_p * GP_MAX_LAYERS) for n in ("W", "dW", "Hact", "a", "c")] + [("drop", DropSite * GP_MAX_LAYERS)]
                + [(n, C.c_void_p) for n in ("w_last", "dw_last", "mask", "g", "g_copy", "phi", "nrm", "sums", "rec")])


class CastJob(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("in_", "out", "outT")] + [("rows", C.c_int64), ("ldt", C.c_int64)]
                + [(n, C.c_int32) for n in ("ldi", "cols", "ldo", "pad_")])


class CastCase(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("kind", "cols", "ldi", "ldo", "colsum_accumulate", "T", "cd", "ldf", "n_jobs", "pad_")]
                + [(n, C.c_int64) for n in ("rows", "ldt", "N", "row_off")]
                + [(n, C.c_void_p) for n in ("in_", "out", "outT", "colsum", "mul", "x", "fa", "fb", "idx")]
                + [("jobs", CastJob * CAST_MAX_JOBS)])


_P, _I, _F, _L = C.c_void_p, C.c_int, C.c_float, C.c_int64

# name -> (restype, argtypes); every symbol declared in include/gantts_hip.h
class DistortionSums(C.Structure):
    _fields_ = [(n, C.c_double) for n in
                ("s_mcd", "s_bap", "s_f0", "n_voiced", "n_vuv_err", "s_mse", "n_frames")]


SIGNATURES = {
    "gt_last_error": (C.c_char_p, []),
    "gt_version": (C.c_char_p, []),
    "gt_engine_create": (_I, [C.POINTER(StreamConfig), C.POINTER(_P)]),
    "gt_engine_destroy": (None, [_P]),
    "gt_live_resources": (_I, [C.POINTER(_L)]),
    "gt_bind_model": (_I, [_P, _I, C.POINTER(ModelDesc)]),
    "gt_bind_optimizer": (_I, [_P, _I, C.POINTER(OptimDesc)]),
    "gt_bind_optimizer_ex": (_I, [_P, _I, C.POINTER(OptimDescEx)]),
    "gt_op_optim_step": (_I, [C.POINTER(OptimDescEx), _P, _P, _L, _P, C.POINTER(_F), _P]),
    "gt_set_training": (_I, [_P, _I, _I]),
    "gt_set_lr": (_I, [_P, _I, _F]),
    "gt_get_optimizer_step": (_I, [_P, _I, C.POINTER(_L)]),
    "gt_get_optimizer_scalars": (_I, [_P, _I, C.POINTER(C.c_double)]),
    "gt_op_optim_scalars": (_I, [C.POINTER(OptimDescEx), _L, C.POINTER(C.c_double)]),
    "gt_set_seed": (_I, [_P, C.c_uint64]),
    "gt_set_dropout_mask": (_I, [_P, _I, _I, _I, _P]),
    "gt_op_philox_mask": (_I, [_P, _I, _I, _I, _L, _F, _L, _I, _P, _P]),
    "gt_set_lengths": (_I, [_P, C.POINTER(_L), _I, _P]),
    "gt_invalidate_mlpg_cache": (_I, [_P]),
    "gt_set_mlpg_windows": (_I, [_P, _I, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "gt_zero_grad": (_I, [_P, _I]),
    "gt_apply_generator": (_I, [_P, _P, _P, _I, _I, _P, _P, _P]),
    "gt_update_discriminator": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, C.POINTER(DResult), _P]),
    "gt_update_generator": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _F, _F, _F, C.POINTER(GResult), _P]),
    "gt_set_loss_normalizer": (_I, [_P, _F]),
    "gt_set_loss_normalizer_device": (_I, [_P, _P]),
    "gt_set_option": (_I, [_P, _I, _I]),
    "gt_set_weight_clip": (_I, [_P, _I, _F]),
    "gt_set_param_ema": (_I, [_P, _I, _P, _L, C.c_double]),
    "gt_set_param_ema_count": (_I, [_P, _I, _L]),
    "gt_get_param_ema_count": (_I, [_P, _I, C.POINTER(_L)]),
    "gt_op_optim_step_ema": (_I, [C.POINTER(OptimDescEx), _P, _P, _L, _P, C.POINTER(_F), _P, _L, C.c_double, _P]),
    "gt_set_spectral_norm": (_I, [_P, _I, _P, _P, _L, _L]),
    "gt_op_spectral_norm": (_I, [C.POINTER(SnCase), _P]),
    "gt_op_sn_project": (_I, [C.POINTER(SnCase), _P]),
    "gt_sn_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_set_grad_penalty": (_I, [_P, _I, _I, _F]),
    "gt_set_gp_epsilon": (_I, [_P, _P]),
    "gt_grad_penalty_result": (_I, [_P, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_L), _I]),
    "gt_grad_penalty_peek": (_I, [_P, _P, _P, _P]),
    "gt_op_grad_penalty": (_I, [C.POINTER(GpCase), _P]),
    "gt_gp_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_set_x_pitch": (_I, [_P, _I, _I]),
    "gt_set_tuning": (_I, [C.c_char_p, _I]),
    "gt_check_faults": (_I, [_P, _P]),
    "gt_lstm_path_counts": (_I, [_P, C.POINTER(_L), _I]),
    "gt_gemm_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_op_gemm_f32": (_I, [C.POINTER(GemmCase), _P]),
    "gt_gemm_b16_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_op_gemm_b16": (_I, [C.POINTER(GemmB16Case), _P]),
    "gt_op_cast_image": (_I, [C.POINTER(CastCase), _P]),
    "gt_sru_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_op_sru_scan": (_I, [C.POINTER(SruScanCase), _P]),
    "gt_op_sru_dx_adv_finish": (_I, [_P, _L, _I, _I, _P, _I, _P, _I, _P]),
    "gt_op_sru_input_mask": (_I, [_P, _I, _I, _F, C.c_uint32, C.c_uint32, _P, _I, _I, _P]),
    "gt_op_sru_input_dropout": (_I, [_P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "gt_head_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_op_d_head": (_I, [C.POINTER(DHeadCase), _P]),
    "gt_op_dstack": (_I, [C.POINTER(DStackCase), _P]),
    "gt_op_frame": (_I, [C.POINTER(FrameCase), _P]),
    "gt_op_mlpg": (_I, [C.POINTER(MlpgCase), _P]),
    "gt_op_mlpg_band": (_I, [_P, _P, _I, C.POINTER(_F), _L, C.POINTER(C.c_int32), _P]),
    "gt_op_mlpg_var": (_I, [C.POINTER(MlpgVarCase), _P]),
    "gt_mlpg_var_path_counts": (_I, [C.POINTER(_L), _I]),
    "gt_op_assemble_batch": (_I, [C.POINTER(AssembleCase), _P]),
    "gt_op_assemble_shard": (_I, [C.POINTER(AssembleCase), C.POINTER(AssembleShard), _P]),
    "gt_corpus_stats_workspace_bytes": (_L, [_L, C.c_int32]),
    "gt_op_corpus_stats": (_I, [C.POINTER(CorpusStatsCase), _P]),
    "gt_clear_faults": (_I, [_P, _P]),
    "gt_comm_unique_id": (_I, [_P]),
    "gt_comm_init": (_I, [_P, _I, _I, _P]),
    "gt_comm_destroy": (_I, [_P]),
    "gt_comm_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "gt_comm_trace": (_I, [_P, _I]),
    "gt_comm_trace_read": (_I, [_P, C.POINTER(C.c_double), _I, C.POINTER(_I)]),
    "gt_set_shard": (_I, [_P, _I, _I]),
    "gt_comm_ipc_export": (_I, [_P, _P]),
    "gt_comm_ipc_attach": (_I, [_P, _I, _I, _P]),
    "gt_comm_ipc_messages": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gt_update_discriminator_begin": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _P]),
    "gt_update_discriminator_end": (_I, [_P, _I, C.POINTER(DResult), _P]),
    "gt_update_generator_begin": (_I, [_P, _P, _P, _P, _P, _P, _F, _P, _I, _I, _I, _F, _F, _F, _P]),
    "gt_update_generator_end": (_I, [_P, _I, _F, _F, _F, C.POINTER(GResult), _P]),
    "gt_update_discriminator_result": (_I, [_P, C.POINTER(DResult)]),
    "gt_update_generator_result": (_I, [_P, C.POINTER(GResult)]),
    "gt_scalar_buffer": (_I, [_P, C.POINTER(_P), C.POINTER(_I)]),
    "gt_model_forward": (_I, [_P, _I, _P, _P, _I, _I, _P, _P, _P]),
    "gt_flush_generator_grads": (_I, [_P, _P]),
    "gt_op_sequence_mask": (_I, [_P, _I, _I, _P, _P]),
    "gt_op_masked_mse": (_I, [_P, _P, _P, _I, _I, _I, C.POINTER(_F), _P, _P]),
    "gt_compute_distortions": (_I, [_P, _P, _I, _P, _P, _I, C.POINTER(_I), C.POINTER(_I), _I, C.POINTER(_L), _I, _I,
                                    C.POINTER(DistortionSums), _P]),
    "gt_ledger_configure": (_I, [_P, _I, _I, C.POINTER(_I), C.POINTER(_I), _I, _P, _P, _I, C.c_double]),
    "gt_ledger_reset": (_I, [_P, _P]),
    "gt_ledger_add": (_I, [_P, _I, _P, _P, _P, _I, _I, _P]),
    "gt_ledger_read": (_I, [_P, C.POINTER(C.c_double), _P]),
    "gt_ledger_buffers": (_I, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "gt_op_epoch_ledger": (_I, [_P, _P, _P, _I, _I, _I, C.c_double, _P]),
    "gt_host_wait_count": (_I, [_P, C.POINTER(C.c_longlong)]),
    "gt_op_gather_cols": (_I, [_P, _I, _P, _I, _P, _I, _I, _L, _P]),
    "gt_op_pad_sequences": (_I, [_P, _I, _P, _P, _I, _I, _P, _I, _P]),
    "gt_op_mlpg_forward": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "gt_op_mlpg_backward": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "gt_op_linear_forward": (_I, [_P, _I, _P, _P, _P, _I, _L, _I, _I, _I, _P, _F, _P]),
    "gt_op_linear_bf16": (_I, [_P, _P, _P, _L, _I, _I, _I, _P, _F, _P, _P, _P, _I, _P, _F, _P, _P, _P, _P, _P, _P]),
    "gt_profile_enable": (_I, [_I]),
    "gt_profile_read": (_I, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_L)]),
    "gt_profile_bytes": (_I, [C.POINTER(C.c_double)]),
    "gt_op_linear_backward": (_I, [_P, _I, _P, _I, _P, _L, _I, _I, _P, _I, _P, _I, _P, _F, _P, _P, _P]),
}


def _build_if_missing():
    """The in-tree library is normally built by ``__graft_entry__.build()``.  If it is MISSING and a HIP compiler is
    at hand, build it now (one process at a time: ranks of a multi-GPU job import concurrently) -- this is still the
    HIP product, not a fallback.  An existing library is never rebuilt here."""
    import fcntl
    import shutil
    import subprocess
    if os.path.isfile(LIB_PATH):
        return
    if shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"):
        return
    with open(os.path.join(_HERE, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not os.path.isfile(LIB_PATH):       # another rank may have built it while we waited
                subprocess.call(["make", "-j8", "-C", os.path.join(_HERE, "csrc")], stdout=subprocess.DEVNULL)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _load():
    _build_if_missing()
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            "gantts_amd: %s not found -- the HIP engine is the product and has no fallback. "
            "Build it: make -C %s" % (LIB_PATH, os.path.join(_HERE, "csrc")))
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype, fn.argtypes = res, args
    return lib


lib = _load()


class GanttsHipError(RuntimeError):
    pass


def check(rc):
    """Maps a C status to the exception the reference raises at the same place."""
    if rc == GT_OK:
        return
    msg = lib.gt_last_error().decode("utf-8", "replace")
    if rc == GT_ERR_DIM:
        raise RuntimeError(msg)            # multistream.py:93-94 raises RuntimeError
    if rc == GT_ERR_INVALID:
        raise ValueError(msg)
    if rc == GT_ERR_STATE:
        raise RuntimeError(msg)
    raise GanttsHipError("HIP error: " + msg)


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
