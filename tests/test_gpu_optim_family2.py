"""-m gpu: the fused clip + update kernel of NAdam, RAdam, Rprop and ASGD (optim_step_kernel<OPTK_NADAM .. OPTK_ASGD>,
gantts_amd/csrc/optim_kernels.hip.h) against torch.optim on the CPU, by the protocol and the rule of
tests/test_gpu_optim_family.py (whose helpers are imported, not restated):

    rms(engine - ref64) <= 3 x rms(torch32 - ref64)      per case and tensor (parameters and every full-size state buffer)

over twelve consecutive clipped steps, the sizes 1 and 4099 judged as one population and 4 * 1024 * 256 + 4099 = 1 052 675 on its
own: the smallest size at which the 1024-workgroup grid takes a SECOND trip of its four-stride loop and ends on a predicated tail.

The cases are chosen so that every branch runs inside twelve steps: RAdam unrectified (steps 1-5) and rectified (from 6), both
weight decays, Rprop's two clamps, ASGD's copy (mu == 1) and averaging branches -- each asserted on the float64 oracle.

Power: the float64 oracle with each non-default argument reset to its default must lie outside the bound.  It is judged on the
parameters, with one exception that torch's rule forces: ASGD's ``t0`` feeds ``mu`` and through it ``ax`` alone (the parameters
never read ``ax``), so ``t0`` is judged on ``ax``.

The host scalar state (NAdam ``mu_product``, ASGD ``eta`` / ``mu``) must equal torch's float32 state tensors exactly.

The four classes are in ``gantts_amd.optim_full``.  No world-2 run here: the data-parallel driver of the first family's file
(tests/hip_runner.py through tests/test_gpu_comm2.py) builds its optimizers from ``gantts_amd.optim`` alone."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_optim_family import (K_STEPS, MARGIN, MAX_NORM, _defaults, _mini_case, _opt_state, _Pair, _report, make_inputs,
                                   reset_variants, rms)

pytestmark = pytest.mark.gpu

SIZES = (1, 4099, 4 * 1024 * 256 + 4099)
GROUPS = ((1, 4099), (4 * 1024 * 256 + 4099,))

CASES = {
    "radam": ("RAdam", dict()),
    "radam_betas_decoupled_wd": ("RAdam", dict(betas=(0.5, 0.9), weight_decay=1e-4, decoupled_weight_decay=True)),
    "nadam_momentum_decay_wd": ("NAdam", dict(momentum_decay=1e-2, weight_decay=1e-5)),
    "nadam_decoupled_wd": ("NAdam", dict(decoupled_weight_decay=True, weight_decay=1e-2)),
    "rprop_etas_step_sizes": ("Rprop", dict(etas=(0.3, 1.5), step_sizes=(1e-4, 0.05))),
    "asgd_t0_lambd_wd": ("ASGD", dict(t0=4, lambd=1e-3, weight_decay=1e-5)),
}
STATE_KEYS = {"RAdam": ("exp_avg", "exp_avg_sq"), "NAdam": ("exp_avg", "exp_avg_sq"), "Rprop": ("prev", "step_size"), "ASGD": ("ax",)}
SCALAR_KEYS = {"RAdam": (), "NAdam": ("mu_product",), "Rprop": (), "ASGD": ("eta", "mu")}
POWER_TENSOR = {("ASGD", "t0"): "ax"}      # see the module docstring


def _kind(tname):
    from gantts_amd import _lib as L
    return dict(NAdam=L.OPT_NADAM, RAdam=L.OPT_RADAM, Rprop=L.OPT_RPROP, ASGD=L.OPT_ASGD)[tname]


def _hyper(tname, kw):
    """The descriptor's hyper-parameter fields of torch's class `tname` built with `kw`."""
    d = _defaults(tname)
    d.update(kw)
    h = dict(lr=d["lr"], weight_decay=d.get("weight_decay", 0.0), eps=d.get("eps", 0.0))
    h["beta1"], h["beta2"] = d.get("betas", (0.0, 0.0))
    if tname == "NAdam":
        h["momentum_decay"] = d["momentum_decay"]
    if tname == "Rprop":
        (h["etaminus"], h["etaplus"]), (h["step_size_min"], h["step_size_max"]) = d["etas"], d["step_sizes"]
    if tname == "ASGD":
        h["alpha"], h["lambd"], h["t0"] = d["alpha"], d["lambd"], d["t0"]
    return h, bool(d.get("decoupled_weight_decay", False))


def _initial_scalars(tname, kw):
    if tname == "NAdam":
        return (1.0, 0.0)
    if tname == "ASGD":
        return (float(torch.tensor(_hyper(tname, kw)[0]["lr"], dtype=torch.float32)), 1.0)
    return (0.0, 0.0)


class TorchRef2(object):
    """One tensor under torch.optim.<tname>(foreach=False) on the CPU in `dtype`; optionally continued from a given state (what a
    loaded checkpoint would hold: the full-size buffers in `dtype`, step and the 0-dim scalars as float32 tensors, as torch keeps them)."""

    def __init__(self, tname, kw, p0, dtype, state=None, step=0, scalars=()):
        self.p = p0.detach().to(dtype).clone().requires_grad_(True)
        self.opt = getattr(torch.optim, tname)([self.p], foreach=False, **kw)
        self.tname, self.dtype = tname, dtype
        if state:
            st = {"step": torch.tensor(float(step))}
            for k, v in zip(SCALAR_KEYS[tname], scalars):
                st[k] = torch.tensor(v, dtype=torch.float32)
            st.update({k: v.detach().to(dtype).clone() for k, v in state.items()})
            self.opt.state[self.p] = st

    def state(self, key, default=None):
        st = self.opt.state.get(self.p, {})
        return st[key] if key in st else default

    def step(self, g, max_norm=MAX_NORM):
        self.p.grad = g.detach().to(self.dtype).clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_([self.p], max_norm, foreach=False)
        self.opt.step()

    def tensors(self):
        out = {"param": self.p.detach().clone()}
        for k in STATE_KEYS[self.tname]:
            out[k] = self.opt.state[self.p][k].detach().clone()
        return out

    def scalars(self):
        return tuple(float(self.opt.state[self.p][k]) for k in SCALAR_KEYS[self.tname])


def run_oracle(tname, kw, p0, gs, dtype):
    """-> final tensors, final scalars, and what the branches did: per step the sign of grad * prev (Rprop) and the mu the step
    used (ASGD)."""
    ref = TorchRef2(tname, kw, p0, dtype)
    trace = []
    for g in gs:
        if tname == "Rprop":
            ref.p.grad = g.detach().to(dtype).clone()
            torch.nn.utils.clip_grad_norm_([ref.p], MAX_NORM, foreach=False)
            prev = ref.state("prev", torch.zeros_like(ref.p))
            trace.append(torch.sign(ref.p.grad * prev).to(torch.int8))
            ref.opt.step()
        else:
            if tname == "ASGD":
                trace.append(float(ref.state("mu", torch.tensor(1.0))))
            ref.step(g)
    out = ref.tensors()
    out["grad"] = ref.p.grad.detach().clone()
    return out, ref.scalars(), trace


def make_desc(tname, kw, step, scalars, states):
    from gantts_amd import _lib as L
    h, decoupled = _hyper(tname, kw)
    desc = L.OptimDescEx2()
    desc.kind, desc.flags = _kind(tname), (L.OPTF_DECOUPLED_WD if decoupled else 0)
    for k, v in h.items():
        setattr(desc, k, v)
    desc.max_grad_norm, desc.step = MAX_NORM, step
    desc.host_state0, desc.host_state1 = scalars
    for i, s in enumerate(states):
        setattr(desc, "state%d" % i, s.data_ptr())
    return desc


def run_engine(tname, kw, p0, gs):
    """K consecutive steps of the production launches through gt_op_optim_step.  The caller of the stand-alone operator keeps the host
    scalar state, as gt_op_optim_scalars gives it, and creates Rprop's step_size filled with lr."""
    from gantts_amd import _lib as L
    from gantts_amd.optim_full import host_scalars
    p = p0.cuda()
    states = [torch.zeros_like(p) for _ in STATE_KEYS[tname]]
    h, _ = _hyper(tname, kw)
    if tname == "Rprop":
        states[1].fill_(h["lr"])
    scalars = _initial_scalars(tname, kw)
    g = torch.empty_like(p)
    norm = C.c_float()
    for k, gk in enumerate(gs):
        g.copy_(gk)
        L.check(L.lib.gt_op_optim_step(C.byref(make_desc(tname, kw, k, scalars, states)), L.ptr(p), L.ptr(g), p.numel(), None,
                                       C.byref(norm), L.current_stream()))
        scalars = host_scalars(_kind(tname), k, k + 1, scalars, **h)
    torch.cuda.synchronize()
    out = {"param": p.cpu(), "grad": g.cpu()}
    for key, s in zip(STATE_KEYS[tname], states):
        out[key] = s.cpu()
    return out, scalars, norm.value


def _check_branches(name, tname, kw, group, runs):
    """Every branch the case is there for was taken, on the float64 oracle of the population `group`."""
    r64 = [runs[n][0] for n in group]
    if name == "radam":
        # rho_t of the defaults: below 5 for steps 1-5, above from step 6 (torch/optim/radam.py)
        rho_inf = 2 / (1 - 0.999) - 1
        rho = [rho_inf - 2 * t * 0.999 ** t / (1 - 0.999 ** t) for t in range(1, K_STEPS + 1)]
        assert [r > 5.0 for r in rho] == [False] * 5 + [True] * (K_STEPS - 5)
    if tname == "Rprop":
        lo, hi = kw["step_sizes"]
        ss = torch.cat([r[0]["step_size"] for r in r64])
        at_lo, at_hi = int((ss == lo).sum()), int((ss == hi).sum())
        _report("optim-family2 %-26s n=%-12s step_size: %d at the minimum, %d at the maximum, %d at neither" % (
            name, "+".join(str(n) for n in group), at_lo, at_hi, ss.numel() - at_lo - at_hi))
        assert at_lo > 0 and at_hi > 0 and ss.numel() - at_lo - at_hi > 0
        # the sign test is discrete: float32 and float64 agree on every factor, so that a failure below means the kernel, not the inputs
        for n in group:
            t64, t32 = runs[n][0][2], runs[n][1][2]
            assert len(t64) == len(t32) == K_STEPS
            for k in range(K_STEPS):
                assert torch.equal(t64[k], t32[k]), "step %d: float32 and float64 disagree on a sign of grad * prev" % (k + 1)
            seen = torch.stack(t64)
            assert bool((seen > 0).any()) and bool((seen < 0).any()) and bool((seen == 0).any())
    if tname == "ASGD":
        mus = runs[group[0]][0][2]
        assert mus[0] == 1.0 and sum(m == 1.0 for m in mus) >= 2 and sum(m != 1.0 for m in mus) >= 2, mus


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("name", list(CASES))
def test_update_kernel_against_float64(name):
    tname, kw = CASES[name]
    runs = {}
    for i, n in enumerate(SIZES):
        p0, gs = make_inputs(n, 2000 + i)
        r64 = run_oracle(tname, kw, p0, gs, torch.float64)
        r32 = run_oracle(tname, kw, p0, gs, torch.float32)
        for r in (r64, r32):
            for k, v in r[0].items():
                assert bool(torch.isfinite(v).all()), "the oracle is not finite: %s n=%d %s" % (name, n, k)
        eng, scalars, norm = run_engine(tname, kw, p0, gs)
        want = float(gs[-1].double().norm())
        assert abs(norm - want) <= 1e-6 * want, (name, n, norm, want)
        # the host scalar state after twelve steps: float32 values formed by the same arithmetic as torch's state tensors
        assert r64[1] == r32[1]
        assert scalars[:len(r32[1])] == r32[1], (name, n, scalars, r32[1])
        variants = [(k, run_oracle(tname, v, p0, gs, torch.float64)[0]) for k, v in reset_variants(tname, kw)]
        runs[n] = (r64, r32, eng, variants)
    failures = []
    for group in GROUPS:
        _check_branches(name, tname, kw, group, runs)
        r64s, r32s, engs = [runs[n][0][0] for n in group], [runs[n][1][0] for n in group], [runs[n][2] for n in group]
        levels = {}
        for key in r64s[0]:
            level = levels[key] = rms(r32s, r64s, key)
            dist = rms(engs, r64s, key)
            ratio = dist / level if level > 0 else (0.0 if dist == 0 else float("inf"))
            _report("optim-family2 %-26s n=%-12s %-12s level %.3e engine %.3e ratio %.2f" % (
                name, "+".join(str(n) for n in group), key, level, dist, ratio))
            if key == "grad":
                continue      # the written-back clipped gradient: reported, not a tensor of the rule
            if not dist <= MARGIN * level:
                failures.append("%s n=%s %s: engine %.3e > %.0f x level %.3e" % (name, group, key, dist, MARGIN, level))
        # power: the oracle with one argument ignored must be told apart by the bound
        for vi, (vk, _) in enumerate(runs[group[0]][3]):
            key = POWER_TENSOR.get((tname, vk), "param")
            vd = rms([runs[n][3][vi][1] for n in group], r64s, key)
            _report("optim-family2 %-26s n=%-12s reset %-22s moves %s by %.3e = %.0f x level" % (
                name, "+".join(str(n) for n in group), vk, key, vd, vd / levels[key] if levels[key] > 0 else float("inf")))
            if not vd > MARGIN * levels[key]:
                failures.append("%s n=%s: resetting %s moves %s by %.3e, inside %.0f x level %.3e -- no power" % (
                    name, group, vk, key, vd, MARGIN, levels[key]))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------
# in the engine: the small MLP generator / discriminator pair of tests/test_gpu_optim_family.py, dropout 0
# ------------------------------------------------------------------------------------------
class _Pair2(_Pair):
    """tests/test_gpu_optim_family.py's pair with its optimizers taken from gantts_amd.optim_full (everything else is inherited)."""

    def __init__(self, case, seeds=(11, 22)):
        import cases as Cs
        import gantts_amd.train as T
        from gantts_amd import optim_full, paramgen
        from gantts_amd.engine import engine_for
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        from hip_runner import build_model, make_hp
        self.case, self.T = case, T
        self.hp = make_hp(case)
        T.hp = self.hp
        self.mg, self.md = build_model(case["g"], seeds[0]).eval(), build_model(case["d"], seeds[1]).eval()
        self.og = getattr(optim_full, case["opt_g"][0])(self.mg.parameters(), **case["opt_g"][1])
        self.od = getattr(optim_full, case["opt_d"][0])(self.md.parameters(), **case["opt_d"][1])
        self.eng = engine_for(self.hp, self.mg)
        x_np, y_np, lengths = Cs.make_batch(case)
        self.x, self.y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        self.lengths = list(lengths)
        self.R = paramgen.unit_variance_mlpg_matrix_cuda(self.hp.windows, case["T"])
        self.y_static = get_static_features(self.y, len(self.hp.windows), self.hp.stream_sizes, self.hp.has_dynamic_features)
        self.mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)


WIRING = {
    # six updates per network: RAdam's sixth is its first rectified one; ASGD averages from the fourth (mu = 1 / max(1, step - t0))
    "g_radam_d_nadam": (("RAdam", dict(lr=1e-3, weight_decay=1e-4, decoupled_weight_decay=True)),
                        ("NAdam", dict(lr=2e-3, momentum_decay=1e-2, weight_decay=1e-5))),
    "g_rprop_d_asgd": (("Rprop", dict(lr=1e-3, etas=(0.3, 1.5), step_sizes=(1e-5, 3e-3))),
                       ("ASGD", dict(lr=1e-2, t0=2, lambd=1e-3, weight_decay=1e-5))),
    "g_asgd_d_rprop": (("ASGD", dict(lr=1e-2, t0=2, lambd=1e-3)),
                       ("Rprop", dict(lr=1e-3))),
}
WIRING_STEPS = 6


@pytest.mark.timeout(900)
@pytest.mark.parametrize("split_phase", [False, True], ids=["fused_combine_norm", "standalone_norm"])
@pytest.mark.parametrize("name", list(WIRING))
def test_engine_update_equals_torch_on_the_written_back_gradient(name, split_phase):
    """Six G+D steps; around every update the pre-step parameters, state and host scalars and the written-back clipped gradient are
    read back, torch's class is applied to them on the CPU (no further clipping), and the post-step parameters and state are compared
    by the rule of the stand-alone test; gt_get_optimizer_step advances once per update and gt_get_optimizer_scalars equals torch's
    float32 state tensors after it.  Once through the fused calls, once through the split-phase calls."""
    from gantts_amd import _lib as L
    opts = dict(zip("GD", WIRING[name]))
    pair = _Pair2(_mini_case(*WIRING[name]))
    held, failures, seen = {}, [], []
    role = dict(G=L.ROLE_G, D=L.ROLE_D)

    def hook(tag, model, opt, before):
        tname, kw = opts[tag]
        if before:
            held["p"], held["state"], held["step"] = model.flat_params().detach().cpu().clone(), _opt_state(opt), opt._step
            held["scalars"] = tuple(opt._scalars)
            return
        grad = model.flat_grads().detach().cpu().clone()
        post = dict(_opt_state(opt), param=model.flat_params().detach().cpu().clone())
        assert opt._step == held["step"] + 1 == pair.eng.optimizer_step_count(role[tag])
        live = held["step"] > 0
        refs = {}
        for dtype in (torch.float64, torch.float32):
            ref = TorchRef2(tname, kw, held["p"], dtype, state=held["state"] if live else None, step=held["step"], scalars=held["scalars"])
            ref.step(grad, max_norm=None)
            refs[dtype] = ref
        want = refs[torch.float32].scalars()
        assert refs[torch.float64].scalars() == want
        got = pair.eng.optimizer_scalars(role[tag])
        assert got[:len(want)] == want and tuple(opt._scalars)[:len(want)] == want, (name, tag, held["step"] + 1, got, want)
        t64, t32 = refs[torch.float64].tensors(), refs[torch.float32].tensors()
        assert sorted(post) == sorted(t64)
        for key in post:
            assert bool(torch.isfinite(t64[key]).all())
            level = rms([t32], [t64], key)
            dist = rms([post], [t64], key)
            _report("optim-wiring2 %-18s %-5s %s %-5s step %d %-12s level %.3e engine %.3e ratio %.2f" % (
                name, "split" if split_phase else "fused", tag, tname, held["step"] + 1, key, level, dist, dist / level if level > 0 else 0.0))
            seen.append((tag, key))
            if not dist <= MARGIN * level:
                failures.append("%s %s step %d %s: engine %.3e > %.0f x level %.3e" % (name, tag, held["step"] + 1, key, dist, MARGIN, level))
        assert float(grad.double().norm()) <= MAX_NORM * (1 + 1e-5)      # what was written back is clipped

    for _ in range(WIRING_STEPS):
        pair.step(split_phase=split_phase, hook=hook)
    pair.eng.check_faults()
    assert len(seen) == WIRING_STEPS * sum(1 + len(STATE_KEYS[opts[t][0]]) for t in "GD")
    assert pair.og._step == pair.od._step == WIRING_STEPS
    assert not failures, "\n".join(failures)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("name,opt", [("nadam", ("NAdam", dict(lr=2e-3, momentum_decay=1e-2))),
                                      ("asgd", ("ASGD", dict(lr=1e-2, t0=1, lambd=1e-3))),
                                      ("rprop", ("Rprop", dict(lr=1e-3, etas=(0.3, 1.5), step_sizes=(1e-5, 3e-3))))])
def test_resume_from_checkpoint_is_bit_identical(name, opt, tmp_path):
    """Three steps, save_checkpoint, a fresh model and optimizer, load_checkpoint, three more steps == six uninterrupted steps, bit
    for bit: NAdam's mu_product, ASGD's eta, mu and ax, Rprop's step_size must come from the checkpoint (Rprop: an lr written after the
    load changes nothing, as in torch, where lr is only the fill of a new step_size)."""
    import gantts_amd.train as T
    case = _mini_case(opt, opt)
    straight = _Pair2(case)
    for _ in range(6):
        straight.step()
    first = _Pair2(case)
    for _ in range(3):
        first.step()
    paths = {tag: T.save_checkpoint(m, o, 3, str(tmp_path), tag) for tag, m, o in (("G", first.mg, first.og), ("D", first.md, first.od))}
    saved = torch.load(paths["G"], map_location="cpu")["optimizer"]["state"][0]
    assert list(saved) == ["step"] + list(first.og.SCALAR_KEYS) + list(first.og.STATE_KEYS)
    for k in first.og.SCALAR_KEYS:
        assert saved[k].dtype == torch.float32 and saved[k].dim() == 0
    resumed = _Pair2(case, seeds=(33, 44))       # other initial weights: everything must come from the checkpoint
    assert T.load_checkpoint(resumed.mg, resumed.og, paths["G"]) == 3 and T.load_checkpoint(resumed.md, resumed.od, paths["D"]) == 3
    assert resumed.og._scalars == first.og._scalars and resumed.od._scalars == first.od._scalars
    if name == "rprop":
        for o in (resumed.og, resumed.od):
            o.param_groups[0]["lr"] = 0.5
    for _ in range(3):
        resumed.step()
    a, b = straight.snapshot(), resumed.snapshot()
    assert sorted(a) == sorted(b) and len(a) == 2 * (1 + len(straight.og.STATE_KEYS))
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs after the resume (max |d| %.3e)" % (name, k, float((a[k] - b[k]).abs().max()))
    assert resumed.og._step == 6 and resumed.od._step == 6
    assert resumed.og._scalars == straight.og._scalars and resumed.od._scalars == straight.od._scalars
    if name == "nadam":
        assert 0.0 < straight.og._scalars[0] < 0.05      # six factors of about 0.45
    if name == "asgd":
        assert straight.og._scalars[1] == float(torch.tensor(0.2))      # mu = 1 / max(1, 6 - t0), a float32


@pytest.mark.timeout(900)
def test_lr_reaches_radam_through_set_lr_and_asgd_through_a_rebind():
    """RAdam: lr edited in param_groups takes the gt_set_lr path (no re-bind) and takes effect.  ASGD keeps lr as a double: the edit
    re-binds, and the scalars and the step count survive the re-bind."""
    pair = _Pair2(_mini_case(("RAdam", dict(lr=1e-3)), ("ASGD", dict(lr=1e-2, t0=0))))
    pair.step()
    pair.step()
    bound_g, bound_d = pair.eng._bound_opt[0], pair.eng._bound_opt[1]
    scalars = tuple(pair.od._scalars)
    assert scalars[1] == 0.5
    pair.og.param_groups[0]["lr"] = 0.0
    pair.od.param_groups[0]["lr"] = 5e-3
    before = pair.mg.flat_params().detach().clone()
    pair.step()
    assert pair.eng._bound_opt[0][1] == bound_g[1] and pair.eng._bound_opt[0][2][0] == 0.0      # same bind, new lr
    assert torch.equal(pair.mg.flat_params(), before)                                            # lr = 0: nothing moves
    assert pair.eng._bound_opt[1][2] != bound_d[2]
    assert pair.og._step == pair.od._step == 3 and pair.eng.optimizer_step_count(1) == 3
    # update 3 used the eta and mu that update 2 left (the bind values of the re-bind); what it leaves comes from the new lr
    want_eta = float(torch.as_tensor(5e-3 / ((1 + 1e-4 * 5e-3 * 3.0) ** 0.75), dtype=torch.float32))
    assert tuple(pair.od._scalars) == (want_eta, float(torch.tensor(1.0 / 3.0, dtype=torch.float32)))
    pair.eng.check_faults()


@pytest.mark.timeout(900)
def test_nadam_binds_and_steps_with_an_underflowed_mu_product():
    """A long run's checkpoint: after some 135 updates the float32 mu_product is exactly 0 (torch goes on with 1 - 0).  Such a state
    loads, binds and steps; the update equals torch's on the same state and written-back gradient by the rule, and mu_product stays 0."""
    from gantts_amd import _lib as L
    opt = ("NAdam", dict(lr=2e-3, weight_decay=1e-5))
    pair = _Pair2(_mini_case(opt, opt))
    for _ in range(2):
        pair.step()
    for o in (pair.og, pair.od):
        sd = o.state_dict()
        for st in sd["state"].values():
            st["step"], st["mu_product"] = torch.tensor(200.0), torch.tensor(0.0)
        o.load_state_dict(sd)
        assert o._step == 200 and o._scalars[0] == 0.0
    held, failures = {}, []

    def hook(tag, model, o, before):
        if before:
            held["p"], held["state"] = model.flat_params().detach().cpu().clone(), _opt_state(o)
            return
        grad = model.flat_grads().detach().cpu().clone()
        post = dict(_opt_state(o), param=model.flat_params().detach().cpu().clone())
        refs = {}
        for dtype in (torch.float64, torch.float32):
            refs[dtype] = TorchRef2(opt[0], opt[1], held["p"], dtype, state=held["state"], step=200, scalars=(0.0,))
            refs[dtype].step(grad, max_norm=None)
        assert refs[torch.float32].scalars() == (0.0,) == pair.eng.optimizer_scalars(dict(G=L.ROLE_G, D=L.ROLE_D)[tag])[:1]
        t64, t32 = refs[torch.float64].tensors(), refs[torch.float32].tensors()
        for key in post:
            assert bool(torch.isfinite(post[key]).all())
            level, dist = rms([t32], [t64], key), rms([post], [t64], key)
            _report("optim-wiring2 nadam_mu_product_0 %s step 201 %-12s level %.3e engine %.3e" % (tag, key, level, dist))
            if not dist <= MARGIN * level:
                failures.append("%s %s: engine %.3e > %.0f x level %.3e" % (tag, key, dist, MARGIN, level))

    pair.step(hook=hook)
    assert pair.og._step == pair.od._step == 201 and pair.og._scalars[0] == 0.0
    pair.eng.check_faults()
    assert not failures, "\n".join(failures)
