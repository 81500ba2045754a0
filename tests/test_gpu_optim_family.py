"""-m gpu: the fused clip + update kernel of every optimizer kind (optim_step_kernel<KIND, F>,
gantts_amd/csrc/optim_kernels.hip.h) against torch.optim on the CPU.

The oracle is the torch class itself (``foreach=False``) behind ``clip_grad_norm_``, once in float64 (the truth) and once in
float32 (the reference's own error).  Rule, per case and compared tensor (parameters and every state buffer):

    rms(engine - ref64) <= 3 x rms(torch32 - ref64)

the project's arbiter margin over the reference's own float32 level, with no absolute floor.  An rms is a
statistic of a population: the sizes 1 and 4099 (the predicated tail: one element, and 3 past 16 x 256) are judged as ONE
population of 4100 elements per tensor -- a single element's rounding error against another single rounding error is a
coin toss, not a level, while an element the tail mishandled would sit orders of magnitude above the population's level
and fail it -- and the cfg2 generator's size 839 355 is judged on its own.

Power: for every case the float64 oracle re-run with each non-default hyper-parameter reset to its default must lie OUTSIDE
the bound, so that a kernel that ignored the argument could not pass."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

K_STEPS = 12
MAX_NORM = 1.0
MARGIN = 3.0
SIZES = (1, 4099, 839355)
GROUPS = ((1, 4099), (839355,))       # populations the rule is applied to (see the module docstring)

# name -> (torch class name, keyword arguments).  Defaults everywhere the issue does not name a value.
CASES = {
    "sgd": ("SGD", dict()),
    "sgd_momentum_dampening_wd": ("SGD", dict(momentum=0.9, dampening=0.1, weight_decay=1e-4)),
    "sgd_nesterov": ("SGD", dict(momentum=0.9, nesterov=True)),
    "rmsprop": ("RMSprop", dict()),
    "rmsprop_momentum_centered_wd": ("RMSprop", dict(momentum=0.9, centered=True, weight_decay=1e-5)),
    "adadelta_rho_wd": ("Adadelta", dict(rho=0.9, weight_decay=1e-5)),
    "adamw_betas": ("AdamW", dict(betas=(0.5, 0.9))),
    "adamw_amsgrad": ("AdamW", dict(amsgrad=True)),
    "adam_amsgrad": ("Adam", dict(amsgrad=True)),
    "adamax_wd": ("Adamax", dict(weight_decay=1e-5)),
    "adagrad_lr_decay": ("Adagrad", dict(lr_decay=1e-3)),
}
# state keys in the order state0, state1, state2 of gt_optim_desc_ex (None: the slot is not used)
STATE_SLOTS = {
    "SGD": lambda kw: ("momentum_buffer" if kw.get("momentum", 0) != 0 else None, None, None),
    "RMSprop": lambda kw: ("square_avg", "momentum_buffer" if kw.get("momentum", 0) > 0 else None, "grad_avg" if kw.get("centered") else None),
    "Adadelta": lambda kw: ("square_avg", "acc_delta", None),
    "Adam": lambda kw: ("exp_avg", "exp_avg_sq", "max_exp_avg_sq" if kw.get("amsgrad") else None),
    "AdamW": lambda kw: ("exp_avg", "exp_avg_sq", "max_exp_avg_sq" if kw.get("amsgrad") else None),
    "Adamax": lambda kw: ("exp_avg", "exp_inf", None),
    "Adagrad": lambda kw: ("sum", None, None),
}


def _defaults(tname):
    import inspect
    sig = inspect.signature(getattr(torch.optim, tname).__init__).parameters
    return {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty}


def make_inputs(n, seed):
    """p0 ~ N(0, 1); per step g = N(0, 1) * 10^U(-3, 0) per element, drawn afresh (float32)."""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    gs = [torch.randn(n, generator=gen) * torch.pow(10.0, -3.0 * torch.rand(n, generator=gen)) for _ in range(K_STEPS)]
    return p0, gs


class TorchRef(object):
    """One tensor under torch.optim.<tname>(foreach=False) on the CPU in `dtype`."""

    def __init__(self, tname, kw, p0, dtype, state=None, step=0):
        self.p = p0.detach().to(dtype).clone().requires_grad_(True)
        self.opt = getattr(torch.optim, tname)([self.p], foreach=False, **kw)
        self.dtype = dtype
        if state:      # continue from the given state (what a loaded checkpoint would hold)
            st = {k: v.detach().to(dtype).clone() for k, v in state.items()}
            if tname != "SGD":
                st["step"] = torch.tensor(float(step))
            self.opt.state[self.p] = st

    def step(self, g, max_norm=MAX_NORM):
        self.p.grad = g.detach().to(self.dtype).clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([self.p], max_norm, foreach=False)
        self.opt.step()

    def tensors(self, keys):
        out = {"param": self.p.detach().clone()}
        for k in keys:
            if k is not None:
                out[k] = self.opt.state[self.p][k].detach().clone()
        return out


def run_oracle(tname, kw, p0, gs, dtype):
    ref = TorchRef(tname, kw, p0, dtype)
    for g in gs:
        ref.step(g)
    out = ref.tensors(STATE_SLOTS[tname](kw))
    out["grad"] = ref.p.grad.detach().clone()
    return out


def make_desc(tname, kw, step, live, states):
    from gantts_amd import _lib as L
    d = _defaults(tname)
    d.update(kw)
    desc = L.OptimDescEx()
    desc.kind = dict(SGD=L.OPT_SGD, RMSprop=L.OPT_RMSPROP, Adadelta=L.OPT_ADADELTA, Adam=L.OPT_ADAM, AdamW=L.OPT_ADAMW,
                     Adamax=L.OPT_ADAMAX, Adagrad=L.OPT_ADAGRAD)[tname]
    desc.flags = ((L.OPTF_NESTEROV if d.get("nesterov") else 0) | (L.OPTF_CENTERED if d.get("centered") else 0)
                  | (L.OPTF_AMSGRAD if d.get("amsgrad") else 0) | (L.OPTF_BUFFER_LIVE if live and tname == "SGD" else 0))
    desc.lr, desc.weight_decay, desc.eps = d["lr"], d["weight_decay"], d.get("eps", 0.0)
    desc.lr_decay = d.get("lr_decay", 0.0)
    desc.beta1, desc.beta2 = d.get("betas", (0.0, 0.0))
    desc.momentum, desc.dampening = d.get("momentum", 0.0), d.get("dampening", 0.0)
    desc.alpha = d.get("alpha", d.get("rho", 0.0))
    desc.max_grad_norm = MAX_NORM
    desc.step = step
    for i, s in enumerate(states):
        setattr(desc, "state%d" % i, None if s is None else s.data_ptr())
    return desc


def run_engine(tname, kw, p0, gs, want_norm=False):
    """K consecutive steps of the production launches (sqnorm_partial_kernel + the update kernel) through gt_op_optim_step."""
    from gantts_amd import _lib as L
    keys = STATE_SLOTS[tname](kw)
    p = p0.cuda()
    states = [None if k is None else torch.zeros_like(p) for k in keys]
    g = torch.empty_like(p)
    norms = []
    for k, gk in enumerate(gs):
        g.copy_(gk)
        norm = C.c_float()
        L.check(L.lib.gt_op_optim_step(C.byref(make_desc(tname, kw, k, k > 0, states)), L.ptr(p), L.ptr(g), p.numel(), None,
                                       C.byref(norm) if want_norm else None, L.current_stream()))
        norms.append(norm.value)
    torch.cuda.synchronize()
    out = {"param": p.cpu(), "grad": g.cpu()}
    for key, s in zip(keys, states):
        if key is not None:
            out[key] = s.cpu()
    return (out, norms) if want_norm else out


def rms(a, b, key):
    """rms of a - b over the population made of the given runs' tensors `key` (two lists of runs)."""
    num = sum(float(((x[key].double() - y[key].double()) ** 2).sum()) for x, y in zip(a, b))
    return (num / sum(x[key].numel() for x in a)) ** 0.5


def reset_variants(tname, kw):
    """The case's keyword arguments with each non-default one reset to its default (nesterov needs momentum: both go)."""
    d = _defaults(tname)
    for k in kw:
        if kw[k] == d[k]:
            continue
        v = dict(kw)
        v[k] = d[k]
        if k == "momentum":
            v.pop("nesterov", None)
        yield k, v


def _report(line):
    print(line)
    path = os.environ.get("GT_OPTIM_REPORT")      # keeps the table of a run: DESIGN.md 6 quotes it
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("name", list(CASES))
def test_update_kernel_against_float64(name):
    tname, kw = CASES[name]
    runs = {}
    for i, n in enumerate(SIZES):
        p0, gs = make_inputs(n, 1000 + i)
        r64 = run_oracle(tname, kw, p0, gs, torch.float64)
        r32 = run_oracle(tname, kw, p0, gs, torch.float32)
        for r in (r64, r32):
            for k, v in r.items():
                assert bool(torch.isfinite(v).all()), "the oracle is not finite: %s n=%d %s" % (name, n, k)
        eng, norms = run_engine(tname, kw, p0, gs, want_norm=True)
        # the reported pre-clip norm is the float64 norm rounded to float32 once
        want = float(gs[-1].double().norm())
        assert abs(norms[-1] - want) <= 1e-6 * want, (name, n, norms[-1], want)
        variants = [(k, run_oracle(tname, v, p0, gs, torch.float64)) for k, v in reset_variants(tname, kw)]
        runs[n] = (r64, r32, eng, variants)
    failures = []
    for group in GROUPS:
        r64s, r32s, engs = ([runs[n][j] for n in group] for j in range(3))
        for key in r64s[0]:
            level = rms(r32s, r64s, key)
            dist = rms(engs, r64s, key)
            ratio = dist / level if level > 0 else (0.0 if dist == 0 else float("inf"))
            _report("optim-family %-30s n=%-10s %-16s level %.3e engine %.3e ratio %.2f" % (
                name, "+".join(str(n) for n in group), key, level, dist, ratio))
            if key == "grad":
                continue      # the written-back clipped gradient: reported, not a tensor of the rule
            if not dist <= MARGIN * level:
                failures.append("%s n=%s %s: engine %.3e > %.0f x level %.3e" % (name, group, key, dist, MARGIN, level))
            if key != "param":
                continue
            # power: the oracle with one argument ignored must be told apart by the bound on the parameters
            for vi, (vk, _) in enumerate(runs[group[0]][3]):
                vd = rms([runs[n][3][vi][1] for n in group], r64s, key)
                _report("optim-family %-30s n=%-10s reset %-14s moves the parameters by %.3e = %.0f x level" % (
                    name, "+".join(str(n) for n in group), vk, vd, vd / level if level > 0 else float("inf")))
                if not vd > MARGIN * level:
                    failures.append("%s n=%s: resetting %s moves the parameters by %.3e, inside %.0f x level %.3e -- no power" % (
                        name, group, vk, vd, MARGIN, level))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------
# in the engine: a small MLP generator / discriminator pair, dropout 0
# ------------------------------------------------------------------------------------------
def _mini_case(opt_g, opt_d):
    import cases as Cs
    return dict(Cs.CASES["acoustic_mlp"], steps=2,
                g=dict(kind="MLP", in_dim=425, out_dim=187, num_hidden=2, hidden_dim=64, dropout=0.0, last_sigmoid=False),
                d=dict(kind="MLP", in_dim=483, out_dim=1, num_hidden=2, hidden_dim=32, dropout=0.0, last_sigmoid=True),
                opt_g=opt_g, opt_d=opt_d)


class _Pair(object):
    """Models, optimizers, engine and batch of a case, stepped by hand (the loop of tests/hip_runner.py, opened up)."""

    def __init__(self, case, seeds=(11, 22)):
        import cases as Cs
        import gantts_amd.train as T
        from gantts_amd import optim, paramgen
        from gantts_amd.engine import engine_for
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        from hip_runner import build_model, make_hp
        self.case, self.T = case, T
        self.hp = make_hp(case)
        T.hp = self.hp
        self.mg, self.md = build_model(case["g"], seeds[0]).eval(), build_model(case["d"], seeds[1]).eval()
        self.og = getattr(optim, case["opt_g"][0])(self.mg.parameters(), **case["opt_g"][1])
        self.od = getattr(optim, case["opt_d"][0])(self.md.parameters(), **case["opt_d"][1])
        self.eng = engine_for(self.hp, self.mg)
        x_np, y_np, lengths = Cs.make_batch(case)
        self.x, self.y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        self.lengths = list(lengths)
        self.R = paramgen.unit_variance_mlpg_matrix_cuda(self.hp.windows, case["T"])
        self.y_static = get_static_features(self.y, len(self.hp.windows), self.hp.stream_sizes, self.hp.has_dynamic_features)
        self.mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)

    def step(self, split_phase=False, hook=None):
        """zero_grad, apply_generator, update_discriminator, update_generator.  split_phase: the *_begin / *_end forms, whose
        optimizer step takes the stand-alone squared-norm launch; otherwise the fused calls (combine + norm in one launch).
        hook(tag, model, optimizer, before) is called around each update."""
        c, e = self.case, self.eng
        self.T.hp = self.hp
        self.og.zero_grad()
        self.od.zero_grad()
        if split_phase:
            e.set_loss_normalizer(float(self.mask.sum().item()))
        y_hat, y_hat_static = e.apply_generator(self.mg, self.x, self.R, self.lengths)
        for tag, model, opt in (("D", self.md, self.od), ("G", self.mg, self.og)):
            if hook:
                hook(tag, model, opt, True)
            if tag == "D" and split_phase:
                e.update_discriminator_begin(self.md, self.od, self.x, self.y_static, y_hat_static, self.mask, "train")
                e.update_discriminator_end(self.od, "train")
            elif tag == "D":
                e.update_discriminator(self.md, self.od, self.x, self.y_static, y_hat_static, self.mask, "train", lengths=self.lengths)
            elif split_phase:
                e.update_generator_begin(self.mg, self.md, self.og, self.x, self.y, y_hat, self.y_static, y_hat_static, c["adv_w"],
                                         self.mask, "train", c["mse_w"], c["mge_w"])
                e.update_generator_end(self.og, c["adv_w"], c["mse_w"], c["mge_w"], "train")
            else:
                e.update_generator(self.mg, self.md, self.og, self.x, self.y, y_hat, self.y_static, y_hat_static, c["adv_w"],
                                   self.mask, "train", c["mse_w"], c["mge_w"], lengths=self.lengths)
            torch.cuda.synchronize()
            if hook:
                hook(tag, model, opt, False)

    def snapshot(self):
        out = {}
        for tag, model, opt in (("G", self.mg, self.og), ("D", self.md, self.od)):
            out[tag + ".params"] = model.flat_params().detach().cpu().clone()
            for key, slot in zip(opt.STATE_KEYS, opt._slots()):
                out["%s.%s" % (tag, key)] = opt._state[slot].detach().cpu().clone()
        return out


def _opt_state(opt):
    return {key: opt._state[slot].detach().cpu().clone() for key, slot in zip(opt.STATE_KEYS, opt._slots()) if opt._state[slot] is not None}


WIRING = {
    "rmsprop_momentum_centered": ("RMSprop", dict(lr=1e-3, momentum=0.9, centered=True)),
    "sgd_nesterov": ("SGD", dict(lr=0.01, momentum=0.9, nesterov=True)),
    "adamw_amsgrad": ("AdamW", dict(lr=1e-3, amsgrad=True)),
}
REDUCE_SLOTS = slice(582, 588)      # gt_gemm_path_counts: the stand-alone weight-gradient combines


@pytest.mark.timeout(900)
@pytest.mark.parametrize("split_phase", [False, True], ids=["fused_combine_norm", "standalone_norm"])
@pytest.mark.parametrize("name", list(WIRING))
def test_engine_update_equals_torch_on_the_written_back_gradient(name, split_phase):
    """Two G+D steps; around every update the pre-step parameters and state and the written-back clipped gradient are read
    back, torch's class is applied to them on the CPU (no further clipping), and the post-step parameters and state are
    compared by the rule of the stand-alone test.  Once through the fused calls, whose optimizer step sums the norm
    partials of the combine launch, once through the split-phase calls, which take the stand-alone squared-norm launch."""
    from gantts_amd import _lib as L
    tname, kw = WIRING[name]
    pair = _Pair(_mini_case((tname, kw), (tname, kw)))
    held, failures, seen = {}, [], []

    def hook(tag, model, opt, before):
        if before:
            held["p"], held["state"], held["step"] = model.flat_params().detach().cpu().clone(), _opt_state(opt), opt._step
            return
        grad = model.flat_grads().detach().cpu().clone()
        post = dict(_opt_state(opt), param=model.flat_params().detach().cpu().clone())
        assert opt._step == held["step"] + 1
        live = held["step"] > 0
        refs = {}
        for dtype in (torch.float64, torch.float32):
            ref = TorchRef(tname, kw, held["p"], dtype, state=held["state"] if live else None, step=held["step"])
            ref.step(grad, max_norm=None)
            refs[dtype] = ref.tensors(list(post.keys() - {"param"}))
        for key in post:
            assert bool(torch.isfinite(refs[torch.float64][key]).all())
            level = rms([refs[torch.float32]], [refs[torch.float64]], key)
            dist = rms([post], [refs[torch.float64]], key)
            _report("optim-wiring %-28s %-5s %s step %d %-16s level %.3e engine %.3e ratio %.2f" % (
                name, "split" if split_phase else "fused", tag, held["step"] + 1, key, level, dist, dist / level if level > 0 else 0.0))
            seen.append(key)
            if not dist <= MARGIN * level:
                failures.append("%s %s step %d %s: engine %.3e > %.0f x level %.3e" % (name, tag, held["step"] + 1, key, dist, MARGIN, level))
        assert float(grad.double().norm()) <= MAX_NORM * (1 + 1e-5)      # what was written back is clipped

    L.check(L.lib.gt_gemm_path_counts(None, 1))
    for _ in range(2):
        pair.step(split_phase=split_phase, hook=hook)
    counts = (C.c_int64 * L.GEMM_PATH_SLOTS)()
    L.check(L.lib.gt_gemm_path_counts(counts, 1))
    combines = sum(list(counts)[REDUCE_SLOTS])
    _report("optim-wiring %-28s %-5s stand-alone combine launches %d" % (name, "split" if split_phase else "fused", combines))
    # the split-phase calls run every weight-gradient combine as a launch of its own (nothing is recorded for a combine + norm launch:
    # SlabDefer::active is set by the fused calls only), so their optimizer step is the stand-alone squared-norm branch
    if split_phase:
        assert combines > 0
    assert len(seen) == 4 * (1 + len(STATE_SLOTS[tname](kw)) - STATE_SLOTS[tname](kw).count(None))
    assert not failures, "\n".join(failures)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,opt", [("sgd_momentum", ("SGD", dict(lr=0.01, momentum=0.9, dampening=0.1))),
                                      ("adamax", ("Adamax", dict(lr=2e-3)))])
def test_resume_from_checkpoint_is_bit_identical(name, opt, tmp_path):
    """Two steps, save_checkpoint, a fresh model and optimizer, load_checkpoint, two more steps == four uninterrupted steps,
    bit for bit (SGD: the loaded momentum_buffer must be continued, not overwritten as on a first update)."""
    import gantts_amd.train as T
    case = _mini_case(opt, opt)
    straight = _Pair(case)
    for _ in range(4):
        straight.step()
    first = _Pair(case)
    for _ in range(2):
        first.step()
    paths = {tag: T.save_checkpoint(m, o, 2, str(tmp_path), tag) for tag, m, o in (("G", first.mg, first.og), ("D", first.md, first.od))}
    resumed = _Pair(case, seeds=(33, 44))       # other initial weights: everything must come from the checkpoint
    assert T.load_checkpoint(resumed.mg, resumed.og, paths["G"]) == 2 and T.load_checkpoint(resumed.md, resumed.od, paths["D"]) == 2
    for _ in range(2):
        resumed.step()
    a, b = straight.snapshot(), resumed.snapshot()
    # parameters and every state buffer of both networks (SGD: momentum_buffer; Adamax: exp_avg, exp_inf)
    assert sorted(a) == sorted(b) and len(a) == 2 * (1 + len(straight.og.STATE_KEYS)) and len(straight.og.STATE_KEYS) >= 1
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs after the resume (max |d| %.3e)" % (name, k, float((a[k] - b[k]).abs().max()))
    if opt[0] != "SGD":
        assert resumed.og._step == 4 and resumed.od._step == 4


@pytest.mark.timeout(900)
def test_lr_path_and_step_counter_for_a_new_kind():
    """gt_set_lr / gt_get_optimizer_step for a kind bound through gt_bind_optimizer_ex: lr edited in param_groups takes effect
    without a re-bind, and the step counter follows."""
    tname, kw = "RMSprop", dict(lr=1e-3, momentum=0.9)
    pair = _Pair(_mini_case((tname, kw), (tname, kw)))
    pair.step()
    bound = pair.eng._bound_opt[0]
    for o in (pair.og, pair.od):
        o.param_groups[0]["lr"] = 0.0
    before = pair.mg.flat_params().detach().clone()
    pair.step()
    assert pair.eng._bound_opt[0][1] == bound[1]                       # no re-bind: the version of the bind is unchanged
    assert torch.equal(pair.mg.flat_params(), before)                     # lr = 0, momentum buffer x 0: nothing moves
    assert pair.og._step == 2 and pair.eng.optimizer_step_count(0) == 2
    pair.eng.check_faults()


@pytest.mark.timeout(900)
def test_data_parallel_world_2_equals_world_1_with_rmsprop_momentum():
    """RMSprop with momentum on both networks over the shared-memory RCCL double (tests/test_gpu_comm2.py's method and rule),
    GT_OPT_COMM_TV_IN_SUMS on: the discriminator's gradient reaches the update kernel unnormalised and 1 / Tv is applied there.
    eps = 1e-5: g / (sqrt(v) + eps) has slope <= 1 / eps in g, so the two world sizes' different summation orders (an element that is
    a cancelling sum is off by ~1e-10 absolutely) stay far inside the file's 1e-4 where eps = 1e-8 would amplify them to it."""
    import cases as Cs
    from hip_runner import run_hip_case
    from test_gpu_comm2 import _check, _run_world2
    opt = ("RMSprop", dict(lr=1e-3, alpha=0.9, eps=1e-5, momentum=0.9))
    case = dict(Cs.CASES["acoustic_mlp"], opt_g=opt, opt_d=opt)
    old = os.environ.get("GT_COMM_TV_IN_SUMS")
    os.environ["GT_COMM_TV_IN_SUMS"] = "1"
    try:
        r0, r1 = _run_world2(case)
        ref = run_hip_case(case)
    finally:
        if old is None:
            os.environ.pop("GT_COMM_TV_IN_SUMS", None)
        else:
            os.environ["GT_COMM_TV_IN_SUMS"] = old
    assert any(k.startswith("G.") for k in ref) and any(k.startswith("D.") for k in ref)
    _check("acoustic_mlp/rmsprop", r0, r1, ref)
