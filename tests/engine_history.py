"""A used engine against a fresh one, bit for bit (tests/test_gpu_engine_history.py, tests/test_engine_history_host.py).

A `Session` holds one (hp, G, D, optimizers, engine) set of a golden case and steps it through the reference-shaped API as
hip_runner.run_hip_case does.  The WORN session stages every batch of every shape into buffers allocated once at the largest shape of its
history (`inplace`: every batch starts at the same device address and is filled with copy_), runs a history, then the probe; its TWIN is a
new set of objects loaded from the worn session's snapshot -- engine_for keys engines on the generator object, so it has a new engine --
that stages into exact-size new allocations (`fresh`) and runs the probe alone.  DESIGN.md ("Engine state across steps"): a step's result
depends on the parameters, the optimizer state, the seed, the step count and the inputs' values, not on what the engine did before -- so
everything the probe returns and leaves behind is compared on its bits, with no tolerance anywhere in this module.

FEATURE_BACKENDS / FEATURE_PAIRS / FEATURE_HISTORIES / feature_probe: the same for the opt-in GAN features (objectives, weight clip, spectral
normalisation, gradient penalties, the generator's weight average), whose state the old probe does not record; a table, a pair list and a probe
of their own, PAIRS and COMM_PAIRS stay what they are."""
import contextlib

import numpy as np

import cases as C

PROBE_SEED = 0x5EED0BAD
FUSED_PANEL = 32           # frames per panel of the fused discriminator stack (dstack_f32.hip.h)

# ---------------------------------------------------------------------------------------------
# shapes: every padding boundary of a wear shape differs from the probe's (checked by tests/test_engine_history_host.py)
# ---------------------------------------------------------------------------------------------
SHAPES = {
    "probe": (3, 19),      # N = 57, N % 16 = 9, pad8(N) = 64; fused stack forced: two 32-frame panels, the last with 25 rows
    "BIG": (7, 40),        # N = 280, N % 16 = 8; nine panels, the last with 24 rows; pad8(T) changes
    "WIDE": (33, 5),       # batch tiles 32 + 1; 2B = 66 > 64: the lengths ring re-allocates its pinned slots
    "TINY_A": (1, 2),      # the shortest sequence the persistent LSTM kernels take
    "TINY_B": (2, 1),      # T = 1: the same engine goes to the per-step kernels
}
ABANDONED_T = (7, 19, 12, 40, 25)      # apply_generator alone, B = 3; then model_forward at FORWARD_SHAPE
FORWARD_SHAPE = (5, 23)


def pad8(n):
    return (n + 7) & ~7


def shape_facts(name):
    B, T = SHAPES[name]
    N = B * T
    return dict(B=B, T=T, N=N, n_mod16=N % 16, pad8_n=pad8(N), pad8_t=pad8(T), panels=-(-N // FUSED_PANEL),
                last_panel_rows=N - (-(-N // FUSED_PANEL) - 1) * FUSED_PANEL, batch_tiles32=-(-B // 32), len_ring_grows=2 * B > 64)


# ---------------------------------------------------------------------------------------------
# backends: one row per path a step can take.  case: (table, name); options: what StepEngine.set_option gets;
# flip: (option, value the backend runs with, its other value) of the option_flip history -- the backend's own option, else launch_riders
# ---------------------------------------------------------------------------------------------
def _case_tables():
    from gan_objective_ref import STEP_CASES
    from test_gpu_sru_discriminator import SRUD_CASES
    return {"CASES": C.CASES, "ORACLE_ONLY_CASES": C.ORACLE_ONLY_CASES, "SRUD_CASES": SRUD_CASES, "STEP_CASES": STEP_CASES}


OPTION_VALUES = {"split_first_layer": (0, 1), "fused_dstack": (0, 1, 2), "matmul_bf16": (0, 1), "lstm_persistent": (0, 1), "sru_d_bf16": (0, 1),
                 "launch_riders": (0, 1), "comm_tv_in_sums": (0, 1)}
_RIDERS = ("launch_riders", 1, 0)
BACKENDS = {
    "mlp_philox": dict(case=("CASES", "acoustic_mlp_dropout"), options={}, flip=_RIDERS),
    "mlp_cond_split": dict(case=("CASES", "acoustic_chain_d"), options={}, flip=("split_first_layer", 1, 0)),
    "mlp_cond_cat": dict(case=("CASES", "acoustic_chain_d"), options={"split_first_layer": 0}, flip=("split_first_layer", 0, 1)),
    "mlp_cond_fused": dict(case=("CASES", "acoustic_chain_d"), options={"fused_dstack": 2}, flip=("fused_dstack", 2, 0)),
    "mlp_bf16": dict(case=("CASES", "acoustic_mlp_dropout"), options={"matmul_bf16": 1}, flip=("matmul_bf16", 1, 0)),
    "mlp_adam_noR": dict(case=("CASES", "duration_mlp"), options={}, flip=_RIDERS),
    "lstm_g": dict(case=("CASES", "acoustic_lstm"), options={}, flip=("lstm_persistent", 1, 0)),
    "lstm_steps": dict(case=("CASES", "acoustic_lstm"), options={"lstm_persistent": 0}, flip=("lstm_persistent", 0, 1)),
    "lstm_bf16": dict(case=("CASES", "acoustic_lstm"), options={"matmul_bf16": 1}, flip=("matmul_bf16", 1, 0)),
    "lstm_d": dict(case=("CASES", "acoustic_lstm_d"), options={}, flip=_RIDERS),
    "gru_g": dict(case=("CASES", "acoustic_grurnn_uni"), options={}, flip=_RIDERS),
    "sru_g": dict(case=("ORACLE_ONLY_CASES", "acoustic_sru_dropout"), options={}, flip=_RIDERS),
    "sru_bf16": dict(case=("ORACLE_ONLY_CASES", "acoustic_sru_dropout"), options={"matmul_bf16": 1}, flip=("matmul_bf16", 1, 0)),
    "sru_d": dict(case=("SRUD_CASES", "srud_uni_k4_cond"), options={}, flip=_RIDERS),
    "sru_d_bf16": dict(case=("SRUD_CASES", "srud_uni_k4_cond"), options={"sru_d_bf16": 1}, flip=("sru_d_bf16", 1, 0)),
    "in2out": dict(case=("CASES", "vc_in2out"), options={}, flip=_RIDERS),
    "in2out_rnn": dict(case=("CASES", "vc_in2out_rnn"), options={}, flip=_RIDERS),
}
HISTORIES_ALL = ("none_inplace", "same_shape_refill", "shrink", "grow", "poison_eval", "poison_train_restore", "option_flip")
HISTORIES_FEW = ("phase_and_roles", "abandoned_passes", "other_d", "shard_and_normaliser", "split_phase")
BACKENDS_FEW = ("mlp_cond_split", "lstm_d", "sru_g")
# every (backend, history) pair applies: no NaN poison had to become +-3e38, no pair is left out
PAIRS = [(b, h) for b in BACKENDS for h in HISTORIES_ALL] + [(b, h) for b in BACKENDS_FEW for h in HISTORIES_FEW]
# Communicating engines: Session.__init__ attaches a one-rank communicator (comm: True), so every step takes the data-parallel routes of the
# valid-frame count -- with the loss sums (comm_tv_in_sums, the default; the flip's other value all-reduces it ahead of the head), its local
# term a rider of the adversarial-column gather (split first layer) or a launch of its own (no split).  A table and a pair list of their own:
# the full cross product stays what it is.
COMM_BACKENDS = {
    "comm_cond_split": dict(case=("CASES", "acoustic_chain_d"), options={}, flip=("comm_tv_in_sums", 1, 0), comm=True),
    # (this case's discriminator is conditioned too and would split by default: the option is what makes the count a launch of its own)
    "comm_philox": dict(case=("CASES", "acoustic_mlp_dropout"), options={"split_first_layer": 0}, flip=("comm_tv_in_sums", 1, 0), comm=True),
}
HISTORIES_COMM = ("same_shape_refill", "shrink", "poison_train_restore", "option_flip", "split_phase")
COMM_PAIRS = [(b, h) for b in COMM_BACKENDS for h in HISTORIES_COMM]
# The opt-in GAN features, which keep state of their own between steps.  A row carries, beside case / options / flip, any of
# objective (hp.gan_objective), weight_clip (hp.discriminator_weight_clip), spectral_norm (hp.discriminator_spectral_norm and
# MLP(spectral_norm=True)), grad_penalty=(kind, weight) (hp.discriminator_grad_penalty[_weight]) and ema_decay (mg.enable_weight_average).
# Cases of gan_objective_ref.STEP_CASES have last_sigmoid=False; a row without an objective ("bce") runs their bce_twin (backend_case).
# Dropout is Philox as everywhere in this module.  One row per path: the per-layer head, the fused stack, a recurrent D; the bf16 shadows
# cast from W_eff; R1 per layer and fused; x_hat written into adv2 (split first layer) and into dcat (no split); the average riding Adagrad
# and Adam; and everything that may be on together in one engine.
FEATURE_BACKENDS = {
    "wgan_clip": dict(case=("STEP_CASES", "mlp32"), options={}, flip=_RIDERS, objective="wgan", weight_clip=0.01),
    "hinge_fused": dict(case=("STEP_CASES", "mlp128_fused"), options={"fused_dstack": 2}, flip=("fused_dstack", 2, 0), objective="hinge"),
    "ls_lstm_d": dict(case=("STEP_CASES", "lstm"), options={}, flip=_RIDERS, objective="ls"),
    "sn_hinge": dict(case=("STEP_CASES", "mlp32_cond"), options={}, flip=_RIDERS, objective="hinge", spectral_norm=True),
    "sn_bce_bf16": dict(case=("STEP_CASES", "mlp32"), options={"matmul_bf16": 1}, flip=("matmul_bf16", 1, 0), spectral_norm=True),
    "gp_r1": dict(case=("STEP_CASES", "mlp32_cond"), options={}, flip=_RIDERS, grad_penalty=("r1", 10.0)),
    "gp_r1_fused": dict(case=("STEP_CASES", "mlp128_fused"), options={"fused_dstack": 2}, flip=("fused_dstack", 2, 0), grad_penalty=("r1", 10.0)),
    "gp_wgan_split": dict(case=("STEP_CASES", "mlp32_cond"), options={}, flip=_RIDERS, objective="wgan", grad_penalty=("wgan-gp", 10.0)),
    "gp_wgan_cat": dict(case=("STEP_CASES", "mlp32_cond"), options={"split_first_layer": 0}, flip=("split_first_layer", 0, 1), objective="wgan",
                        grad_penalty=("wgan-gp", 10.0)),
    "ema_adagrad": dict(case=("CASES", "acoustic_mlp_dropout"), options={}, flip=_RIDERS, ema_decay=0.9),
    "ema_adam": dict(case=("CASES", "duration_mlp"), options={}, flip=_RIDERS, ema_decay=0.999),
    "all_wgan": dict(case=("STEP_CASES", "mlp32_cond"), options={}, flip=_RIDERS, objective="wgan", weight_clip=0.01, grad_penalty=("wgan-gp", 10.0),
                     ema_decay=0.9),
}
FEATURE_KEYS = ("objective", "weight_clip", "spectral_norm", "grad_penalty", "ema_decay")
LAST_SIGMOID = {"bce": True, "ls": False, "hinge": False, "wgan": False}       # what the bound discriminator must have under the objective
AWAY_OBJECTIVE = {"ls": "hinge", "hinge": "ls", "wgan": "ls"}                    # feature_off_and_on: another objective with the same last_sigmoid
HISTORIES_FEATURE_FEW = ("phase_and_roles", "abandoned_passes", "split_phase")
FEATURE_BACKENDS_FEW = ("sn_hinge", "gp_wgan_split", "ema_adam")


def _rows_with(*keys):
    return [b for b, row in FEATURE_BACKENDS.items() if any(row.get(k) and row.get(k) != "bce" for k in keys)]


FEATURE_PAIRS = ([(b, h) for b in FEATURE_BACKENDS for h in HISTORIES_ALL]
                 + [(b, "feature_off_and_on") for b in _rows_with("grad_penalty", "weight_clip", "objective")]
                 + [(b, "gp_hooks") for b in _rows_with("grad_penalty")]
                 + [(b, "sn_other_d") for b in _rows_with("spectral_norm")]
                 + [(b, "ema_swap_and_roles") for b in _rows_with("ema_decay")]
                 + [(b, h) for b in FEATURE_BACKENDS_FEW for h in HISTORIES_FEATURE_FEW]
                 + [("gp_wgan_split", "normaliser"), ("sn_hinge", "shard_and_normaliser"), ("ema_adam", "shard_and_normaliser")])
ALL_BACKENDS = dict(BACKENDS, **COMM_BACKENDS)
ALL_BACKENDS.update(FEATURE_BACKENDS)
# the second discriminator of `other_d`: another kind and width, the same in_dim
OTHER_D = {"MLP": dict(kind="LSTMRNN", out_dim=1, num_hidden=1, hidden_dim=20, bidirectional=True, dropout=0.0, last_sigmoid=True),
           "LSTMRNN": dict(kind="MLP", out_dim=1, num_hidden=2, hidden_dim=24, dropout=0.0, last_sigmoid=True)}


def backend_case(backend):
    table, name = ALL_BACKENDS[backend]["case"]
    case = _case_tables()[table][name]
    if table == "STEP_CASES" and ALL_BACKENDS[backend].get("objective", "bce") == "bce":
        from gan_objective_ref import bce_twin
        case = bce_twin(case)
    return case


def backend_features(backend, override=None):
    row = ALL_BACKENDS[backend]
    return dict({k: row[k] for k in FEATURE_KEYS if k in row}, **(override or {}))


# ---------------------------------------------------------------------------------------------
# the comparator
# ---------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def difference(name, worn, twin):
    """None when `worn` and `twin` are finite and the same bits (uint32 views of float32: -0.0 is not +0.0, one ulp is a difference);
    else one line that says what differs, or which side is not finite."""
    a, b = np.atleast_1d(np.asarray(worn)), np.atleast_1d(np.asarray(twin))
    if a.shape != b.shape or a.dtype != b.dtype:
        return "%s: worn %s %s, twin %s %s" % (name, a.dtype, a.shape, b.dtype, b.shape)
    for side, v in (("worn", a), ("twin", b)):
        if v.dtype.kind == "f" and not np.isfinite(v).all():
            return "%s: %s has %d non-finite of %d elements" % (name, side, int((~np.isfinite(v)).sum()), v.size)
    ne = _bits(a) != _bits(b)
    if ne.any():
        i = np.unravel_index(int(np.argmax(ne)), ne.shape)
        return "%s: %d of %d elements differ, first at %s: worn %r twin %r" % (name, int(ne.sum()), ne.size, tuple(int(v) for v in i), a[i], b[i])
    return None


def differences(worn, twin):
    """Every difference between two records (dicts name -> array), in the worn record's order; a missing name is one."""
    out = []
    for k in worn:
        d = difference(k, worn[k], twin[k]) if k in twin else "%s: missing in the twin" % k
        if d:
            out.append(d)
    out += ["%s: missing in the worn session" % k for k in twin if k not in worn]
    return out


# ---------------------------------------------------------------------------------------------
# batches: host arrays, made once per (case, shape, seed, poison) and never modified
# ---------------------------------------------------------------------------------------------
_BATCHES = {}


def make_batch(backend, B, T, seed, poison=False):
    """dict(B, T, x, y, lengths) of cases.make_batch for the backend's case at (B, T); poison: x and y are NaN at every valid frame."""
    key = (ALL_BACKENDS[backend]["case"], B, T, seed, poison)
    if key not in _BATCHES:
        x, y, lengths = C.make_batch(dict(backend_case(backend), B=B, T=T), seed=seed)
        if poison:
            for b, n in enumerate(lengths):
                x[b, :n] = np.nan
                y[b, :n] = np.nan
        for a in (x, y, lengths):
            a.setflags(write=False)
        _BATCHES[key] = dict(B=B, T=T, x=x, y=y, lengths=lengths)
    return _BATCHES[key]


def shape_batch(backend, shape, seed, poison=False):
    B, T = SHAPES[shape]
    return make_batch(backend, B, T, seed, poison)


def probe_batches(backend):
    return [shape_batch(backend, "probe", s) for s in (4101, 4102, 4103)]


@contextlib.contextmanager
def _recorded_results():
    """The step functions return the reference's tuples (five and four scalars); the engine's result structs carry the gradient norm as a
    sixth and fifth.  Keeps the struct each call fills."""
    from gantts_amd import _lib as L
    seen = {}
    saved = (L.DResult, L.GResult)

    def factory(tag, cls):
        def make():
            seen[tag] = cls()
            return seen[tag]
        return make
    L.DResult, L.GResult = factory("d", saved[0]), factory("g", saved[1])
    try:
        yield seen
    finally:
        L.DResult, L.GResult = saved


def _struct_array(s):
    return np.array([getattr(s, n) for n, _ in s._fields_], dtype=np.float32)


def build_sn_mlp(spec, seed):
    """The case's MLP discriminator as MLP(spectral_norm=True): the weights build_model gives it, sn_u / sn_v the deterministic unit vectors
    of spectral_norm_ref.initial_uv (the constructor's are drawn from torch's global generator)."""
    import torch
    import spectral_norm_ref as S
    from gantts_amd import models
    assert spec["kind"] == "MLP"
    m = models.MLP(spectral_norm=True, **{k: v for k, v in spec.items() if k != "kind"})
    sd = {k: torch.from_numpy(v) for k, v in C.make_weights(spec, seed).items()}
    u0, v0 = S.initial_uv(spec)
    sd["sn_u"], sd["sn_v"] = torch.from_numpy(np.concatenate(u0)), torch.from_numpy(np.concatenate(v0))
    m.load_state_dict(sd)
    return m.cuda()


class Session(object):
    def __init__(self, backend, policy, shapes=(), options=None, snapshot=None, features=None):
        """policy "inplace": x, y, y_static, mask and the lengths tensor are views of the first elements of buffers sized for the largest of
        `shapes` ((B, T) pairs); "fresh": exact-size new allocations, all kept alive so that no address comes back.  features: values that
        replace the row's own (FEATURE_KEYS), for the negative controls."""
        import torch
        from gantts_amd import optim
        from gantts_amd.engine import engine_for
        from hip_runner import build_model, make_hp
        assert policy in ("inplace", "fresh")
        self.backend, self.policy = backend, policy
        self.case = case = backend_case(backend)
        self.features = ft = backend_features(backend, features)
        # the opt-in features as a train_loop user switches them on: on the hp before engine_for, MLP(spectral_norm=True), enable_weight_average
        self.hp = make_hp(case)
        if "objective" in ft:
            self.hp.gan_objective = ft["objective"]
        if ft.get("weight_clip"):
            self.hp.discriminator_weight_clip = ft["weight_clip"]
        if ft.get("spectral_norm"):
            self.hp.discriminator_spectral_norm = True
        if ft.get("grad_penalty"):
            self.hp.discriminator_grad_penalty, self.hp.discriminator_grad_penalty_weight = ft["grad_penalty"]
        self.mg = build_model(case["g"], 11, case.get("saturate_gates", False))
        self.md = build_sn_mlp(case["d"], 22) if ft.get("spectral_norm") else build_model(case["d"], 22)
        if ft.get("ema_decay") is not None:
            self.mg.enable_weight_average(ft["ema_decay"])
        self.og = getattr(optim, case["opt_g"][0])(self.mg.parameters(), **case["opt_g"][1])
        self.od = getattr(optim, case["opt_d"][0])(self.md.parameters(), **case["opt_d"][1])
        if snapshot is not None:
            self.restore(snapshot)
        self.train_mode()
        self.engine = engine_for(self.hp, self.mg)
        self.options = dict(ALL_BACKENDS[backend]["options"], **(options or {}))
        for k, v in self.options.items():
            self.engine.set_option(k, v)
        if ALL_BACKENDS[backend].get("comm"):      # as hip_runner.run_hip_case(comm_world_1=True); one rank's collectives are issued, not skipped
            self.engine.set_option("comm_force", 1)
            self.engine.comm_init(0, 1, self.engine.comm_unique_id())
        self._keep = []
        if policy == "inplace":
            n, b = max(B * T for B, T in shapes), max(B for B, _ in shapes)
            ds = self.engine.static_dim
            self._buf = dict(x=torch.zeros(n * case["din"], device="cuda"), y=torch.zeros(n * case["dout"], device="cuda"),
                             y_static=torch.zeros(n * ds, device="cuda"), mask=torch.zeros(n, device="cuda"),
                             lengths=torch.zeros(b, dtype=torch.int64, device="cuda"))

    # ---- modes, state -----------------------------------------------------------------------
    def train_mode(self):
        """the modules as run_hip_case leaves them for the case: .train() iff its dropout is on (Philox: nothing is injected)"""
        if self.case["dropout_on"]:
            self.mg.train(), self.md.train()
        else:
            self.mg.eval(), self.md.eval()

    def snapshot(self):
        import copy
        snap = dict(g={k: v.detach().clone() for k, v in self.mg.state_dict().items()},
                    d={k: v.detach().clone() for k, v in self.md.state_dict().items()},      # (sn_u / sn_v of a spectrally normalised D are in here)
                    og=copy.deepcopy(self.og.state_dict()), od=copy.deepcopy(self.od.state_dict()))
        if self.mg.ema_decay is not None:      # what a generator checkpoint carries beside the parameters (train.save_checkpoint)
            snap["ema"], snap["n_averaged"] = self.mg.ema_state_dict(), self.mg.n_averaged
        return snap

    def restore(self, snap):
        self.mg.load_state_dict(snap["g"])
        self.md.load_state_dict(snap["d"])
        self.og.load_state_dict(snap["og"])
        self.od.load_state_dict(snap["od"])
        if "ema" in snap:
            self.mg.load_ema_state_dict(snap["ema"], snap["n_averaged"])

    def set_option(self, name, value):
        self.options[name] = value
        self.engine.set_option(name, value)

    # ---- staging ----------------------------------------------------------------------------
    def _place(self, name, value):
        if self.policy == "fresh":
            t = value.contiguous().clone()
            self._keep.append(t)
            return t
        v = self._buf[name][:value.numel()].view(value.shape)
        v.copy_(value)
        return v

    def stage(self, batch):
        import torch
        from gantts_amd import paramgen
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        hp, Tn = self.hp, batch["T"]
        x = self._place("x", torch.tensor(batch["x"], device="cuda"))
        y = self._place("y", torch.tensor(batch["y"], device="cuda"))
        sl = self._place("lengths", torch.tensor(batch["lengths"], device="cuda"))
        ys = self._place("y_static", get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features))
        mask = self._place("mask", sequence_mask(sl, max_len=Tn).unsqueeze(-1).to(torch.float32))
        R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn) if bool(np.any(self.case["has_dynamic_features"])) else None
        return x, y, ys, mask, R, [int(v) for v in batch["lengths"]]

    # ---- steps ------------------------------------------------------------------------------
    def step(self, batch, phase, update_d=True, update_g=True, split_phase=False, model_d=None, optimizer_d=None, after_d=None):
        """One batch through zero_grad twice, T.apply_generator, T.update_discriminator, T.update_generator (split_phase: the engine's
        update_*_begin / _end(defer=True) / _result instead of the two fused calls).  Returns dict(y_hat, y_hat_static, d_scalars (six),
        g_scalars (five)) as numpy; a skipped update leaves its scalars out.  after_d(out): called between the two updates."""
        import torch
        import gantts_amd.train as T
        case, eng = self.case, self.engine
        md, od = (self.md, self.od) if model_d is None else (model_d, optimizer_d)
        if phase == "train":
            self.train_mode()
        else:
            self.mg.eval(), md.eval()
        x, y, ys, mask, R, lengths = self.stage(batch)
        T.hp = self.hp
        out = {}
        with _recorded_results() as seen:
            self.og.zero_grad()
            od.zero_grad()
            y_hat, yhs = T.apply_generator(self.mg, x, R, lengths)
            if self.policy == "fresh":
                self._keep += [y_hat, yhs]
            if update_d:
                if split_phase:
                    eng.update_discriminator_begin(md, od, x, ys, yhs, mask, phase, lengths=lengths)
                    eng.update_discriminator_end(od, phase, defer=True)
                    eng.update_discriminator_result()
                else:
                    T.update_discriminator(md, od, x, ys, yhs, lengths, mask, phase)
                out["d_scalars"] = _struct_array(seen["d"])
                if after_d is not None:
                    after_d(out)
            if update_g:
                if split_phase:
                    eng.update_generator_begin(self.mg, md, self.og, x, y, y_hat, ys, yhs, case["adv_w"], mask, phase, case["mse_w"],
                                               case["mge_w"], lengths=lengths)
                    eng.update_generator_end(self.og, case["adv_w"], case["mse_w"], case["mge_w"], phase, defer=True)
                    eng.update_generator_result()
                else:
                    T.update_generator(self.mg, md, self.og, x, y, y_hat, ys, yhs, case["adv_w"], lengths, mask, phase,
                                       mse_w=case["mse_w"], mge_w=case["mge_w"])
                out["g_scalars"] = _struct_array(seen["g"])
        torch.cuda.synchronize()
        out["y_hat"], out["y_hat_static"] = y_hat.cpu().numpy(), yhs.cpu().numpy()
        self.train_mode()
        return out

    def apply_generator_only(self, batch):
        import gantts_amd.train as T
        x, _, _, _, R, lengths = self.stage(batch)
        T.hp = self.hp
        self.og.zero_grad()
        self.od.zero_grad()
        T.apply_generator(self.mg, x, R, lengths)

    def state(self):
        """parameters, every optimizer state tensor and the step counts (the optimizer objects' and the engine's)"""
        import torch
        from gantts_amd import _lib as L
        torch.cuda.synchronize()
        out = {}
        for tag, model, opt, role in (("G", self.mg, self.og, L.ROLE_G), ("D", self.md, self.od, L.ROLE_D)):
            names = list(model.state_dict().keys())
            for k, v in model.state_dict().items():
                out["%s.%s" % (tag, k)] = v.detach().cpu().numpy()
            for i, st in opt.state_dict()["state"].items():
                for key, v in st.items():
                    out["%s.opt.%s.%s" % (tag, key, names[i])] = torch.as_tensor(v).detach().cpu().numpy()
            out["%s.opt.steps" % tag] = np.array([opt._step, self.engine.optimizer_step_count(role)], dtype=np.int64)
        return out

    def next_masks(self, rows):
        """the keep masks of the next step's first G site and first D-step site (hip_runner.run_hip_case's `extra`)"""
        return {"philox_g": self.engine.philox_mask(0, 0, 0, 0.5, rows, 48).cpu().numpy(),
                "philox_d": self.engine.philox_mask(1, 0, 0, 0.5, 2 * rows, 40).cpu().numpy()}


# ---------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------
def probe(session, seed=PROBE_SEED):
    """set_seed, two train steps and one eval-phase step at the probe shape: one flat record of everything compared"""
    session.engine.set_seed(seed)
    b = probe_batches(session.backend)
    rec = {}
    for i, (batch, phase) in enumerate(zip(b, ("train", "train", "test"))):
        for k, v in session.step(batch, phase).items():
            rec["step%d.%s" % (i, k)] = v
    rec.update(session.state())
    B, Tn = SHAPES["probe"]
    rec.update(session.next_masks(B * Tn))
    session.engine.check_faults()
    return rec


def gp_record(engine, reset):
    """gt_grad_penalty_result as two records: the two means (float64) and the count of penalised steps"""
    r = engine.grad_penalty_result(reset=reset)
    return np.array([r["grad_penalty"], r["grad_norm_at_penalty"]], dtype=np.float64), np.array([r["steps"]], dtype=np.int64)


def feature_probe(session, seed=PROBE_SEED):
    """The probe of the FEATURE_PAIRS: the same three steps, and beside what `probe` records what the features leave behind --
    gradient penalty: the running record, read and reset before the first step as train_loop does once per phase (what a history left in it
      is discarded) and read again behind the third; wgan-gp: eps and the x_hat image of the last train step, peeked between its two updates;
    weight average: its bits, both counts (the model's and the engine's), y_hat of one eval-mode forward inside averaged_weights() and the
      parameters behind it (the swap gives them back);
    spectral norm: sn_u / sn_v are part of D's state_dict, so of state();
    gp_paths / sn_paths: the launches of either feature's kernels over the probe (process-wide counters, read before and after)."""
    import torch
    eng, ft = session.engine, session.features
    gp_kind = ft["grad_penalty"][0] if ft.get("grad_penalty") else None
    eng.set_seed(seed)
    before = (eng.gp_path_counts(), eng.sn_path_counts())
    if gp_kind:
        gp_record(eng, reset=True)
    b = probe_batches(session.backend)
    B, Tn = SHAPES["probe"]
    rec = {}

    def peek(out):
        e_, xh = eng.grad_penalty_peek(B * Tn, eng._adv_width())
        torch.cuda.synchronize()
        rec["gp_peek.eps"], rec["gp_peek.x_hat"] = e_.cpu().numpy(), xh.cpu().numpy()

    for i, (batch, phase) in enumerate(zip(b, ("train", "train", "test"))):
        for k, v in session.step(batch, phase, after_d=peek if (gp_kind == "wgan-gp" and i == 1) else None).items():
            rec["step%d.%s" % (i, k)] = v
    if gp_kind:
        rec["gp_record"], rec["gp_steps"] = gp_record(eng, reset=True)
    if ft.get("ema_decay") is not None:
        mg = session.mg
        for k, v in mg.ema_state_dict().items():
            rec["ema.%s" % k] = v.cpu().numpy()
        rec["ema_counts"] = np.array([mg.n_averaged, eng.param_ema_count()], dtype=np.int64)
        mg.eval()
        with mg.averaged_weights():
            rec["ema_forward.y_hat"] = eng.model_forward(mg, torch.tensor(b[2]["x"], device="cuda"),
                                                         lengths=[int(v) for v in b[2]["lengths"]]).cpu().numpy()
        session.train_mode()
        rec["ema_after_swap.params"] = mg.flat_params().detach().cpu().numpy()
    rec.update(session.state())
    rec.update(session.next_masks(B * Tn))
    after = (eng.gp_path_counts(), eng.sn_path_counts())
    rec["gp_paths"] = np.array(after[0], dtype=np.int64) - np.array(before[0], dtype=np.int64)
    rec["sn_paths"] = np.array(after[1], dtype=np.int64) - np.array(before[1], dtype=np.int64)
    eng.check_faults()
    return rec


# ---------------------------------------------------------------------------------------------
# histories: name -> (the shapes its inplace buffers must hold, what the worn session does before the probe).
# A history returns the snapshot the twin is loaded from when that is not the state at its end.
# ---------------------------------------------------------------------------------------------
def _h_none(s):
    pass


def _h_same_shape_refill(s):
    s.step(shape_batch(s.backend, "probe", 5201), "train")


def _h_shrink(s):
    for seed in (5301, 5302):
        s.step(shape_batch(s.backend, "BIG", seed), "train")


def _h_grow(s):
    for shape, seed in (("TINY_A", 5401), ("TINY_B", 5402), ("WIDE", 5403)):
        s.step(shape_batch(s.backend, shape, seed), "train")


def _h_poison_eval(s):
    out = s.step(shape_batch(s.backend, "BIG", 5501, poison=True), "test")
    s.engine.check_faults()
    # the premise: the poison went through both networks (else this history wears nothing)
    assert np.isnan(out["y_hat_static"]).any() and np.isnan(out["d_scalars"][:3]).all() and np.isnan(out["g_scalars"][3]), out


def _h_poison_train_restore(s):
    import torch
    snap = s.snapshot()
    s.step(shape_batch(s.backend, "BIG", 5601, poison=True), "train")
    s.engine.check_faults()
    # the premise: parameters and optimizer state of both networks are poisoned, so the restore below has something to undo
    for model, opt in ((s.mg, s.og), (s.md, s.od)):
        assert torch.isnan(model.flat_params()).any() and any(torch.isnan(st).any() for st in opt._state if st is not None), s.backend
    # ... and so is what the features keep: the average and sn_u / sn_v (undone through the snapshot).  The penalty's record has taken the step
    # (cleared by the probe's opening reset) but is NOT NaN: the penalty sees D's input only through the signs of the activations -- a NaN
    # activation takes the leaky slope, in the kernels (leaky_drop_grad) as in torch's leaky_relu_backward -- and the weights are still finite
    # when it is formed, so |grad_x D| and the penalty are finite numbers in the double-backward reference too.
    if s.features.get("ema_decay") is not None:
        assert torch.isnan(s.mg._ema).any() and s.mg.n_averaged == 1, s.backend
    if s.features.get("spectral_norm"):
        assert torch.isnan(s.md.sn_u).any() and torch.isnan(s.md.sn_v).any(), s.backend
    if s.features.get("grad_penalty"):
        means, steps = gp_record(s.engine, reset=False)
        assert steps[0] == 1 and np.isfinite(means).all() and means.all(), (s.backend, means, steps)
    s.restore(snap)
    return snap


def _h_option_flip(s):
    name, home, away = ALL_BACKENDS[s.backend]["flip"]
    s.set_option(name, away)
    s.step(shape_batch(s.backend, "BIG", 5701), "train")
    s.set_option(name, home)


def _h_phase_and_roles(s):
    s.step(shape_batch(s.backend, "BIG", 5801), "test")
    s.step(shape_batch(s.backend, "probe", 5802), "train", update_d=False)
    s.step(shape_batch(s.backend, "probe", 5803), "train", update_g=False)


def _h_abandoned_passes(s):
    import torch
    for i, Tn in enumerate(ABANDONED_T):
        s.apply_generator_only(make_batch(s.backend, 3, Tn, 5901 + i))
    B, Tn = FORWARD_SHAPE
    b = make_batch(s.backend, B, Tn, 5950)
    lengths = [int(v) for v in b["lengths"]]
    s.engine.model_forward(s.mg, torch.tensor(b["x"], device="cuda"), lengths=lengths)
    xd = torch.from_numpy(np.random.RandomState(5951).rand(B, Tn, s.md.in_dim).astype(np.float32)).cuda()
    s.engine.model_forward(s.md, xd, lengths=lengths)
    torch.cuda.synchronize()


def _h_other_d(s):
    from gantts_amd import optim
    from hip_runner import build_model
    spec = dict(OTHER_D[s.case["d"]["kind"]], in_dim=s.md.in_dim)
    md2 = build_model(spec, 33)
    od2 = optim.Adagrad(md2.parameters(), lr=0.01)
    s.step(shape_batch(s.backend, "probe", 6001), "train", update_g=False, model_d=md2, optimizer_d=od2)


def _h_shard_and_normaliser(s):
    s.engine.set_shard(1, 2)
    s.engine.set_loss_normalizer(123.0)
    s.step(shape_batch(s.backend, "BIG", 6101), "train")
    s.engine.set_shard(0, 1)
    s.engine.set_loss_normalizer(-1.0)       # not positive: the mask's own sum again


def _h_split_phase(s):
    s.step(shape_batch(s.backend, "BIG", 6201), "train", split_phase=True)
    s.step(shape_batch(s.backend, "probe", 6202), "train", split_phase=True)


_P, _ABANDONED_SHAPES = SHAPES["probe"], tuple((3, t) for t in ABANDONED_T)
HISTORIES = {
    "none_inplace": ((_P, SHAPES["BIG"]), _h_none),      # (buffers of BIG's size: what the control isolates is the aliasing, not a history)
    "same_shape_refill": ((_P,), _h_same_shape_refill),
    "shrink": ((_P, SHAPES["BIG"]), _h_shrink),
    "grow": ((_P, SHAPES["TINY_A"], SHAPES["TINY_B"], SHAPES["WIDE"]), _h_grow),
    "poison_eval": ((_P, SHAPES["BIG"]), _h_poison_eval),
    "poison_train_restore": ((_P, SHAPES["BIG"]), _h_poison_train_restore),
    "option_flip": ((_P, SHAPES["BIG"]), _h_option_flip),
    "phase_and_roles": ((_P, SHAPES["BIG"]), _h_phase_and_roles),
    "abandoned_passes": ((_P,) + _ABANDONED_SHAPES, _h_abandoned_passes),
    "other_d": ((_P,), _h_other_d),
    "shard_and_normaliser": ((_P, SHAPES["BIG"]), _h_shard_and_normaliser),
    "split_phase": ((_P, SHAPES["BIG"]), _h_split_phase),
}


def run_pair(backend, history):
    """(the worn session's probe record, its twin's)"""
    shapes, wear = HISTORIES[history]
    worn = Session(backend, "inplace", shapes=shapes)
    snap = wear(worn) or worn.snapshot()
    twin = Session(backend, "fresh", options=worn.options, snapshot=snap)
    return probe(worn), probe(twin)


# ---------------------------------------------------------------------------------------------
# the features' own histories (FEATURE_PAIRS).  Each asserts its premise: that it wore the state it names.
# ---------------------------------------------------------------------------------------------
def _gp_steps(s):
    return int(gp_record(s.engine, reset=False)[1][0])


def _h_feature_off_and_on(s):
    """Every switch of the row goes off (the penalty, the clip, the objective to another one that fits the same discriminator) for one
    train step at BIG and comes back; a penalised row then takes one step under the other kind and another weight."""
    import torch
    from gantts_amd import _lib as L
    eng, ft = s.engine, s.features
    gp, clip, obj = ft.get("grad_penalty"), ft.get("weight_clip"), ft.get("objective", "bce")
    assert gp or clip or obj != "bce", s.backend
    steps0 = _gp_steps(s) if gp else 0
    if gp:
        eng.set_grad_penalty(None)
    if clip:
        eng.set_weight_clip(L.ROLE_D, 0.0)
    if obj != "bce":
        assert LAST_SIGMOID[AWAY_OBJECTIVE[obj]] == LAST_SIGMOID[obj]
        eng.set_option("gan_objective", L.GAN_OBJECTIVES[AWAY_OBJECTIVE[obj]])
    s.step(shape_batch(s.backend, "BIG", 6301), "train")
    # the premises: no penalty was recorded; no parameter was clamped (the unclipped network has weights beyond the bound)
    if gp:
        assert eng.grad_penalty is None and _gp_steps(s) == steps0, (s.backend, steps0, _gp_steps(s))
    if clip:
        assert float(s.md.flat_params().abs().max()) > clip, s.backend
    if obj != "bce":
        assert eng.gan_objective == AWAY_OBJECTIVE[obj]
        eng.set_option("gan_objective", L.GAN_OBJECTIVES[obj])
    if clip:
        eng.set_weight_clip(L.ROLE_D, clip)
    if gp:
        other = "wgan-gp" if gp[0] == "r1" else "r1"      # (either kind is allowed under every objective)
        eng.set_grad_penalty(other, 0.5 * gp[1] + 1.0)
        s.step(shape_batch(s.backend, "BIG", 6302), "train")
        assert _gp_steps(s) == steps0 + 1, (s.backend, _gp_steps(s))
        eng.set_grad_penalty(*gp)
    torch.cuda.synchronize()


def _h_gp_hooks(s):
    """The parity hooks around a step at BIG: injected interpolation weights, and the two readers in between.  Reading changes nothing."""
    import torch
    eng, (kind, _) = s.engine, s.features["grad_penalty"]
    B, Tn = SHAPES["BIG"]
    eps = torch.from_numpy(np.random.RandomState(6401).rand(B * Tn).astype(np.float32)).cuda()
    steps0 = _gp_steps(s)
    eng.set_gp_epsilon(eps)
    seen = {}

    def between(out):
        seen["record"] = gp_record(eng, reset=False)
        if kind == "wgan-gp":
            e_, xh = eng.grad_penalty_peek(B * Tn, eng._adv_width())
            seen["eps"], seen["x_hat"] = e_.cpu().numpy(), xh.cpu().numpy()

    s.step(shape_batch(s.backend, "BIG", 6402), "train", after_d=between)
    eng.set_gp_epsilon(None)
    assert seen["record"][1][0] == steps0 + 1 and np.isfinite(seen["record"][0]).all(), (s.backend, seen["record"])
    if kind == "wgan-gp":      # the premise: the step interpolated with the injected weights
        assert np.array_equal(seen["eps"].view(np.uint32), eps.cpu().numpy().view(np.uint32)) and np.isfinite(seen["x_hat"]).all(), s.backend
    assert _gp_steps(s) == steps0 + 1


def _h_sn_other_d(s):
    """other_d with a second spectrally normalised MLP of other widths (a new job table, W_eff of another size, its own sn_u / sn_v), one
    D-only train step; then an eval-phase step at BIG with the first discriminator, which must leave its sn_u / sn_v alone."""
    import torch
    from gantts_amd import optim
    spec = dict(s.case["d"], num_hidden=2, hidden_dim=24, dropout=0.0, in_dim=s.md.in_dim)
    assert (spec["num_hidden"], spec["hidden_dim"]) != (s.case["d"]["num_hidden"], s.case["d"]["hidden_dim"])
    md2 = build_sn_mlp(spec, 33)
    od2 = optim.Adagrad(md2.parameters(), lr=0.01)
    u2 = md2.sn_u.clone()
    s.step(shape_batch(s.backend, "probe", 6501), "train", update_g=False, model_d=md2, optimizer_d=od2)
    assert not torch.equal(md2.sn_u, u2), "the second discriminator's pass did not iterate"
    u, v = s.md.sn_u.clone(), s.md.sn_v.clone()
    s.step(shape_batch(s.backend, "BIG", 6502), "test")
    torch.cuda.synchronize()
    assert torch.equal(s.md.sn_u.view(torch.int32), u.view(torch.int32)) and torch.equal(s.md.sn_v.view(torch.int32), v.view(torch.int32)), \
        "%s: an eval-phase step advanced sn_u / sn_v" % s.backend


def _h_ema_swap_and_roles(s):
    """An eval-phase step at BIG on the averaged weights, a discriminator-only train step (the average stays), a generator-only one (it moves)."""
    import torch
    mg, eng = s.mg, s.engine
    params, count = mg.flat_params().detach().clone(), mg.n_averaged
    mg.eval()
    with mg.averaged_weights():
        s.step(shape_batch(s.backend, "BIG", 6601), "test")
    s.train_mode()
    assert torch.equal(mg.flat_params().view(torch.int32), params.view(torch.int32)) and mg.n_averaged == count == eng.param_ema_count()
    s.step(shape_batch(s.backend, "probe", 6602), "train", update_g=False)
    assert mg.n_averaged == count == eng.param_ema_count(), (s.backend, mg.n_averaged, eng.param_ema_count())
    s.step(shape_batch(s.backend, "probe", 6603), "train", update_d=False)
    assert mg.n_averaged == count + 1 == eng.param_ema_count(), (s.backend, mg.n_averaged, eng.param_ema_count())


def _h_normaliser(s):
    """The penalty reads 1 / Tv where the head does (LossNormaliser::inv_tv); sharding is refused under a penalty, so the override alone."""
    s.engine.set_loss_normalizer(123.0)
    s.step(shape_batch(s.backend, "BIG", 6701), "train")
    s.engine.set_loss_normalizer(-1.0)


def _h_feature_shard_and_normaliser(s):
    """shard_and_normaliser; where the engine refuses the shard (spectral norm), the refusal by its message, then the override alone on
    the engine that refused."""
    if not s.features.get("spectral_norm"):
        return _h_shard_and_normaliser(s)
    s.step(shape_batch(s.backend, "probe", 6801), "train")      # (binds the discriminator: the normalisation is the bound network's)
    try:
        s.engine.set_shard(1, 2)
    except ValueError as e:
        assert "gt_set_shard: spectral normalisation" in str(e), str(e)
    else:
        raise AssertionError("%s: set_shard(1, 2) was not refused" % s.backend)
    s.engine.set_shard(0, 1)
    return _h_normaliser(s)


_BIG2 = (_P, SHAPES["BIG"])
FEATURE_HISTORIES = {
    "feature_off_and_on": (_BIG2, _h_feature_off_and_on),
    "gp_hooks": (_BIG2, _h_gp_hooks),
    "sn_other_d": (_BIG2, _h_sn_other_d),
    "ema_swap_and_roles": (_BIG2, _h_ema_swap_and_roles),
    "normaliser": (_BIG2, _h_normaliser),
    "shard_and_normaliser": (_BIG2, _h_feature_shard_and_normaliser),
}


def feature_history(name):
    return FEATURE_HISTORIES[name] if name in FEATURE_HISTORIES else HISTORIES[name]


def run_feature_pair(backend, history):
    """run_pair for the FEATURE_PAIRS: the features' histories first, feature_probe on both sides"""
    shapes, wear = feature_history(history)
    worn = Session(backend, "inplace", shapes=shapes)
    snap = wear(worn) or worn.snapshot()
    twin = Session(backend, "fresh", options=worn.options, snapshot=snap)
    return feature_probe(worn), feature_probe(twin)
