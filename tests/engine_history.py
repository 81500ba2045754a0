"""A used engine against a fresh one, bit for bit (tests/test_gpu_engine_history.py, tests/test_engine_history_host.py).

A `Session` holds one (hp, G, D, optimizers, engine) set of a golden case and steps it through the reference-shaped API as
hip_runner.run_hip_case does.  The WORN session stages every batch of every shape into buffers allocated once at the largest shape of its
history (`inplace`: every batch starts at the same device address and is filled with copy_), runs a history, then the probe; its TWIN is a
new set of objects loaded from the worn session's snapshot -- engine_for keys engines on the generator object, so it has a new engine --
that stages into exact-size new allocations (`fresh`) and runs the probe alone.  DESIGN.md ("Engine state across steps"): a step's result
depends on the parameters, the optimizer state, the seed, the step count and the inputs' values, not on what the engine did before -- so
everything the probe returns and leaves behind is compared on its bits, with no tolerance anywhere in this module."""
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
    from test_gpu_sru_discriminator import SRUD_CASES
    return {"CASES": C.CASES, "ORACLE_ONLY_CASES": C.ORACLE_ONLY_CASES, "SRUD_CASES": SRUD_CASES}


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
ALL_BACKENDS = dict(BACKENDS, **COMM_BACKENDS)
# the second discriminator of `other_d`: another kind and width, the same in_dim
OTHER_D = {"MLP": dict(kind="LSTMRNN", out_dim=1, num_hidden=1, hidden_dim=20, bidirectional=True, dropout=0.0, last_sigmoid=True),
           "LSTMRNN": dict(kind="MLP", out_dim=1, num_hidden=2, hidden_dim=24, dropout=0.0, last_sigmoid=True)}


def backend_case(backend):
    table, name = ALL_BACKENDS[backend]["case"]
    return _case_tables()[table][name]


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


class Session(object):
    def __init__(self, backend, policy, shapes=(), options=None, snapshot=None):
        """policy "inplace": x, y, y_static, mask and the lengths tensor are views of the first elements of buffers sized for the largest of
        `shapes` ((B, T) pairs); "fresh": exact-size new allocations, all kept alive so that no address comes back."""
        import torch
        from gantts_amd import optim
        from gantts_amd.engine import engine_for
        from hip_runner import build_model, make_hp
        assert policy in ("inplace", "fresh")
        self.backend, self.policy = backend, policy
        self.case = case = backend_case(backend)
        self.hp = make_hp(case)
        self.mg, self.md = build_model(case["g"], 11, case.get("saturate_gates", False)), build_model(case["d"], 22)
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
        return dict(g={k: v.detach().clone() for k, v in self.mg.state_dict().items()},
                    d={k: v.detach().clone() for k, v in self.md.state_dict().items()},
                    og=copy.deepcopy(self.og.state_dict()), od=copy.deepcopy(self.od.state_dict()))

    def restore(self, snap):
        self.mg.load_state_dict(snap["g"])
        self.md.load_state_dict(snap["d"])
        self.og.load_state_dict(snap["og"])
        self.od.load_state_dict(snap["od"])

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
    def step(self, batch, phase, update_d=True, update_g=True, split_phase=False, model_d=None, optimizer_d=None):
        """One batch through zero_grad twice, T.apply_generator, T.update_discriminator, T.update_generator (split_phase: the engine's
        update_*_begin / _end(defer=True) / _result instead of the two fused calls).  Returns dict(y_hat, y_hat_static, d_scalars (six),
        g_scalars (five)) as numpy; a skipped update leaves its scalars out."""
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
