"""Spectral normalisation of the MLP discriminator (gt_set_spectral_norm, hp.discriminator_spectral_norm, MLP(spectral_norm=True)) on the
device: the two hooks against float64 with derived bounds (tests/spectral_norm_ref.py), convergence on a matrix with known singular
values, bit-for-bit equivalence of a step with the feature on and a step of the plain engine on the hook's W_eff, two G+D steps against a
CPU step reference, eval mode / checkpoints / the switch left off, and the refusals."""
import ctypes as Ct
import functools

import numpy as np
import pytest
import torch

import gan_objective_ref as G
import spectral_norm_ref as S

pytestmark = pytest.mark.gpu

GUARD = 64            # floats of sentinel on either side of every buffer a hook writes (keeps the payload 16-byte aligned)
SENT = np.float32(-7.25e11)


def _lb():
    from gantts_amd import _lib as Lb
    return Lb


def sn_counts(reset=False):
    Lb = _lb()
    c = (Ct.c_int64 * Lb.SN_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_sn_path_counts(c, 1 if reset else 0))
    return list(c)


class Guarded(object):
    """A device buffer with sentinels on both sides; shift = 1 moves the payload one float off its 16-byte boundary."""

    def __init__(self, payload, dtype=torch.float32, shift=0):
        payload = np.asarray(payload)
        self.n, self.lo = payload.size, GUARD + shift
        sent = float(SENT)
        self.buf = torch.full((self.n + 2 * GUARD + 4,), sent, dtype=dtype, device="cuda")
        self.t = self.buf[self.lo:self.lo + self.n]
        self.t.copy_(torch.from_numpy(payload.astype(np.float64 if dtype == torch.float64 else np.float32)).cuda())

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        return self.t.cpu().numpy().copy()

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:self.lo] == b.dtype.type(SENT)) and np.all(b[self.lo + self.n:] == b.dtype.type(SENT)))


def sn_case(tab, n_flat, iterate, W=None, u=None, v=None, weff=None, sigma=None, Gr=None, s=None, parts=None, n_parts=None):
    Lb = _lb()
    c = Lb.SnCase()
    c.n_layers, c.iterate, c.n_flat = len(tab), int(iterate), n_flat
    for q, (off, out, in_, _, _) in enumerate(tab):
        c.w_off[q], c.out[q], c.in_[q] = off, out, in_
    for name, b in (("W", W), ("u", u), ("v", v), ("weff", weff), ("sigma", sigma), ("G", Gr), ("s", s), ("norm_partials", parts)):
        if b is not None:
            setattr(c, name, b if isinstance(b, int) else b.ptr())
    if parts is not None:
        c.norm_cap = parts.n
        c.n_norm_partials = Ct.pointer(n_parts)
    return c


def hook_prepare(tab, n_flat, W, u, v, weff, sigma, iterate):
    Lb = _lb()
    Lb.check(Lb.lib.gt_op_spectral_norm(Ct.byref(sn_case(tab, n_flat, iterate, W=W, u=u, v=v, weff=weff, sigma=sigma)), Lb.current_stream()))
    torch.cuda.synchronize()


def hook_project(tab, n_flat, Gr, weff, u, v, sigma, s, parts):
    Lb = _lb()
    n = Ct.c_int32(0)
    Lb.check(Lb.lib.gt_op_sn_project(Ct.byref(sn_case(tab, n_flat, 0, u=u, v=v, weff=weff, sigma=sigma, Gr=Gr, s=s, parts=parts, n_parts=n)),
                                     Lb.current_stream()))
    torch.cuda.synchronize()
    return n.value


def _flat_inputs(seed=7):
    """The hook tests' flat buffer: NaN wherever no weight lies, so that anything that reads a bias slot or the lead shows."""
    tab, n_flat = S.flat_layout()
    rs = np.random.RandomState(seed)
    W = np.full(n_flat, np.nan, np.float32)
    u, v = [], []
    for off, out, in_, _, _ in tab:
        W[off:off + out * in_] = ((rs.rand(out * in_) * 2 - 1) / np.sqrt(in_)).astype(np.float32)
        u.append(S.unit(rs.randn(out)).astype(np.float32))
        v.append(S.unit(rs.randn(in_)).astype(np.float32))
    return tab, n_flat, W, np.concatenate(u), np.concatenate(v)


def _weight_mask(tab, n_flat):
    m = np.zeros(n_flat, bool)
    for off, out, in_, _, _ in tab:
        m[off:off + out * in_] = True
    return m


def _run_prepare(shift, iterate, W_np, u_np, v_np, tab, n_flat):
    W, u, v = Guarded(W_np, shift=shift), Guarded(u_np), Guarded(v_np)
    weff, sigma = Guarded(np.full(n_flat, SENT, np.float32), shift=shift), Guarded(np.full(len(tab), SENT, np.float32))
    hook_prepare(tab, n_flat, W, u, v, weff, sigma, iterate)
    assert all(b.guards_intact() for b in (W, u, v, weff, sigma))
    return W.get(), u.get(), v.get(), weff.get(), sigma.get()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the hook against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off_by_one_float"])
def test_hook_against_float64(shift):
    tab, n_flat, W_np, u_np, v_np = _flat_inputs()
    wm = _weight_mask(tab, n_flat)
    sn_counts(reset=True)
    W1, u1, v1, weff, sigma = _run_prepare(shift, 1, W_np, u_np, v_np, tab, n_flat)
    assert sn_counts(reset=True) == [1, 1, 1, 0, 0]                                     # at most 3 launches
    assert np.array_equal(_bits(W1), _bits(W_np))                                        # the caller's W is untouched
    assert np.all(weff[~wm] == SENT)                                                     # bias slots and the lead are untouched
    for q, (off, out, in_, uo, vo) in enumerate(tab):
        Wl = W_np[off:off + out * in_].reshape(out, in_)
        S.check_iterate(Wl, u_np[uo:uo + out], u1[uo:uo + out], v1[vo:vo + in_], sigma[q])
        S.check_weff(Wl, sigma[q], weff[off:off + out * in_].reshape(out, in_))
    # two runs are bit-equal, and so are the 16-byte and the element-by-element form of the element pass
    again = _run_prepare(shift, 1, W_np, u_np, v_np, tab, n_flat)
    other = _run_prepare(1 - shift, 1, W_np, u_np, v_np, tab, n_flat)
    for a, b, c in zip((u1, v1, weff, sigma), again[1:], other[1:]):
        assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    # the eval form from the advanced vectors: u and v untouched bit for bit, two launches, sigma = u^T W v
    sn_counts(reset=True)
    _, ue, ve, weff_e, sigma_e = _run_prepare(shift, 0, W_np, u1, v1, tab, n_flat)
    assert sn_counts(reset=True) == [0, 1, 1, 0, 0]
    assert np.array_equal(_bits(ue), _bits(u1)) and np.array_equal(_bits(ve), _bits(v1))
    assert np.all(weff_e[~wm] == SENT)
    for q, (off, out, in_, uo, vo) in enumerate(tab):
        Wl = W_np[off:off + out * in_].reshape(out, in_)
        S.check_eval(Wl, u1[uo:uo + out], v1[vo:vo + in_], sigma_e[q])
        S.check_weff(Wl, sigma_e[q], weff_e[off:off + out * in_].reshape(out, in_))


# ---------------------------------------------------------------------------------------------------------------------
# 2. convergence on a matrix whose singular values are known exactly
# ---------------------------------------------------------------------------------------------------------------------
def _hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def test_power_iteration_converges_to_the_top_singular_value():
    """W = U diag(2, 1, 0.5, ...) V^T with U = H16 / 4 and V = the first 16 columns of H64 / 8 (Sylvester-Hadamard: orthonormal columns
    with entries +-2^-2, +-2^-3), so every entry of W is a short dyadic sum and float32 holds W exactly: sigma_1 = 2, sigma_2 = 1.
    Power method: the angle to the top pair shrinks by sigma_2 / sigma_1 = 0.5 per iteration and the Rayleigh-type estimate's error by
    0.25: after k iterations sigma_1 - sigma <= 2 tan^2(theta_0) 0.25^k; with cos(theta_0) >= 0.1, tan^2 <= 99 and k = 40 that is
    1.7e-22 -- negligible.  What remains is float32 rounding in the LAST iteration: v' and u' are unit vectors rounded per component, so
    |v'| and u'^T r / |r| are each within 2^-24 of 1, and sigma is rounded once: |sigma - 2| <= 2 ((1 + 2^-24)^3 - 1) plus second-order
    terms (the per-component roundings of earlier iterations enter orthogonally to the top pair, at 2^-48: the factor 1 + 2^-20 below)
    plus the double sums (five chained sums of at most 66 terms: 10 gamma(66) relative)."""
    out, in_ = 16, 64
    sv = np.array([2.0, 1.0, 0.5, 0.5] + [0.25] * 12)
    Um, Vm = _hadamard(16) / 4.0, (_hadamard(64) / 8.0)[:, :16]
    W64 = Um @ np.diag(sv) @ Vm.T
    W_np = W64.astype(np.float32)
    assert np.array_equal(W_np.astype(np.float64), W64) and np.allclose(np.linalg.svd(W64, compute_uv=False)[:2], [2.0, 1.0], atol=1e-12)
    rs = np.random.RandomState(3)
    # the start: mostly the second and third left singular vectors, a fifth of the first (cos(theta_0) = 0.2 / |(0.2, 0.9, 0.4)| = 0.199)
    u_np, v_np = S.unit(0.2 * Um[:, 0] + 0.9 * Um[:, 1] + 0.4 * Um[:, 2]).astype(np.float32), S.unit(rs.randn(in_)).astype(np.float32)
    cos0 = abs(float(Um[:, 0] @ u_np.astype(np.float64)))
    assert cos0 >= 0.1
    tab, n_flat = S.flat_layout(((out, in_),), lead=1)
    flat = np.full(n_flat, np.nan, np.float32)
    flat[1:1 + out * in_] = W_np.ravel()
    W, u, v = Guarded(flat), Guarded(u_np), Guarded(v_np)
    weff, sigma = Guarded(np.full(n_flat, SENT, np.float32)), Guarded(np.full(1, SENT, np.float32))
    for _ in range(40):
        hook_prepare(tab, n_flat, W, u, v, weff, sigma, 1)
    power = 2.0 * 99.0 * 0.25 ** 40
    bound = 2.0 * ((1.0 + S.F32) ** 3 - 1.0) * (1.0 + 2.0 ** -20) + 2.0 * 10.0 * S.gamma(66) + power
    got = float(sigma.get()[0])
    print("SNCONV sigma %r |sigma - 2| %.3e bound %.3e" % (got, abs(got - 2.0), bound))
    assert abs(got - 2.0) <= bound
    S.check_weff(W_np, sigma.get()[0], weff.get()[1:1 + out * in_].reshape(out, in_))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the projection hook
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "off_by_one_float"])
def test_projection_hook_against_float64(shift):
    tab, n_flat, W_np, u_np, v_np = _flat_inputs()
    wm = _weight_mask(tab, n_flat)
    _, u1, v1, weff_np, sigma_np = _run_prepare(shift, 1, W_np, u_np, v_np, tab, n_flat)
    rs = np.random.RandomState(21)
    G_np = rs.randn(n_flat).astype(np.float32)                     # bias slots and the lead hold gradients too: squared, never written
    Gr, weff, u, v, sigma = Guarded(G_np, shift=shift), Guarded(weff_np, shift=shift), Guarded(u1), Guarded(v1), Guarded(sigma_np)
    s = Guarded(np.full(len(tab), float(SENT)), dtype=torch.float64)
    parts = Guarded(np.full(2048, float(SENT)), dtype=torch.float64)
    sn_counts(reset=True)
    n_parts = hook_project(tab, n_flat, Gr, weff, u, v, sigma, s, parts)
    assert sn_counts(reset=True) == [0, 0, 0, 1, 1]                                      # at most 2 launches
    assert all(b.guards_intact() for b in (Gr, weff, u, v, sigma, s, parts))
    got, s_got, p_got = Gr.get(), s.get(), parts.get()
    assert 0 < n_parts <= 2048 and np.all(p_got[n_parts:] == float(SENT))
    assert np.array_equal(_bits(got[~wm]), _bits(G_np[~wm]))                            # bias gradients are untouched
    for q, (off, out, in_, uo, vo) in enumerate(tab):
        sl = slice(off, off + out * in_)
        S.check_project(G_np[sl].reshape(out, in_), weff_np[sl].reshape(out, in_), u1[uo:uo + out], v1[vo:vo + in_], sigma_np[q], s_got[q],
                        got[sl].reshape(out, in_))
    S.check_sqnorm(got, p_got[:n_parts])
    # bit-equal again, and across the two forms of the element pass
    for sh in (shift, 1 - shift):
        G2, we2, s2, p2 = Guarded(G_np, shift=sh), Guarded(weff_np, shift=sh), Guarded(np.zeros(len(tab)), dtype=torch.float64), \
            Guarded(np.zeros(2048), dtype=torch.float64)
        assert hook_project(tab, n_flat, G2, we2, u, v, sigma, s2, p2) == n_parts
        assert np.array_equal(_bits(G2.get()), _bits(got)) and np.array_equal(_bits(s2.get()), _bits(s_got))
        assert np.array_equal(_bits(p2.get()[:n_parts]), _bits(p_got[:n_parts]))


# ---------------------------------------------------------------------------------------------------------------------
# whole steps
# ---------------------------------------------------------------------------------------------------------------------
def _layers_of(spec):
    ins = [spec["in_dim"]] + [spec["hidden_dim"]] * (spec["num_hidden"] - 1) + [spec["hidden_dim"]]
    outs = [spec["hidden_dim"]] * spec["num_hidden"] + [spec["out_dim"]]
    return tuple(zip(outs, ins))


def build_d(spec, sn, seed=22):
    """The case's discriminator; sn: MLP(spectral_norm=True) with the deterministic sn_u / sn_v of the step reference."""
    import cases as C
    from gantts_amd import models
    kw = {k: v for k, v in spec.items() if k != "kind"}
    m = models.MLP(spectral_norm=sn, **kw)
    sd = {k: torch.from_numpy(v) for k, v in C.make_weights(spec, seed).items()}
    if sn:
        u0, v0 = S.initial_uv(spec)
        sd["sn_u"], sd["sn_v"] = torch.from_numpy(np.concatenate(u0)), torch.from_numpy(np.concatenate(v0))
    m.load_state_dict(sd)
    return m.cuda()


class Run(object):
    """One (G, D, optimizers, engine) set on a step case, driven step by step."""

    def __init__(self, case, obj, sn, hp_flag="same", bf16=False, d_lr=None, md=None, d_clip_norm=None):
        import cases as C
        import gantts_amd.train as Tr
        from gantts_amd import optim, paramgen
        from gantts_amd.engine import engine_for
        from hip_runner import build_model, make_hp
        self.case, self.Tr, self.C = case, Tr, C
        hp = make_hp(case)
        hp.gan_objective = obj
        flag = sn if hp_flag == "same" else hp_flag
        if flag is not None:
            hp.discriminator_spectral_norm = flag
        self.hp = hp
        Tr.hp = hp
        self.mg = build_model(case["g"], 11)
        self.md = md if md is not None else build_d(case["d"], sn)
        self.mg.train(), self.md.train()
        self.og = getattr(optim, case["opt_g"][0])(self.mg.parameters(), **case["opt_g"][1])
        d_kw = dict(case["opt_d"][1])
        if d_lr is not None:
            d_kw["lr"] = d_lr
        self.od = getattr(optim, case["opt_d"][0])(self.md.parameters(), **d_kw)
        if d_clip_norm is not None:
            self.od.max_grad_norm = d_clip_norm
        self.eng = engine_for(hp, self.mg)
        if case.get("fused"):
            self.eng.set_option("fused_dstack", 2)
        if bf16:
            self.eng.set_option("matmul_bf16", 1)
        x_np, y_np, lengths = C.make_batch(case)
        self.x, self.y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        self.R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"])
        self.sl = torch.from_numpy(np.ascontiguousarray(lengths)).cuda()
        self.cpu_lengths = list(lengths)

    def begin(self, step):
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        self.Tr.hp = self.hp
        gm, dm = self.C.make_dropout_masks(self.case, step)
        third = len(dm) // 3
        self.mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
        for p in range(3):
            self.md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * third:(p + 1) * third]])
        hp = self.hp
        self.y_static = get_static_features(self.y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
        self.mask = sequence_mask(self.sl, max_len=self.case["T"]).unsqueeze(-1)
        self.og.zero_grad()
        self.od.zero_grad()
        self.y_hat, self.y_hat_static = self.Tr.apply_generator(self.mg, self.x, self.R, self.cpu_lengths)

    def d_step(self, phase="train"):
        return np.array(self.Tr.update_discriminator(self.md, self.od, self.x, self.y_static, self.y_hat_static, self.cpu_lengths, self.mask, phase),
                        dtype=np.float64)

    def g_step(self, phase="train"):
        c = self.case
        return np.array(self.Tr.update_generator(self.mg, self.md, self.og, self.x, self.y, self.y_hat, self.y_static, self.y_hat_static,
                                                 c["adv_w"], self.cpu_lengths, self.mask, phase, mse_w=c["mse_w"], mge_w=c["mge_w"]), dtype=np.float64)

    def steps(self, n, first=0):
        out = {}
        for step in range(first, first + n):
            self.begin(step)
            if step == 0:
                out["y_hat"], out["y_hat_static"] = self.y_hat.cpu().numpy(), self.y_hat_static.cpu().numpy()
            out["d_scalars_%d" % step] = self.d_step()
            out["g_scalars_%d" % step] = self.g_step()
        torch.cuda.synchronize()
        return out

    def state(self):
        from hip_runner import state_arrays
        torch.cuda.synchronize()
        return state_arrays(self.mg, self.md, self.og, self.od)


def head_counts(reset=False):
    Lb = _lb()
    h = (Ct.c_int64 * Lb.HEAD_PATH_SLOTS)()
    g = (Ct.c_int64 * Lb.GEMM_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_head_path_counts(h, 1 if reset else 0))
    Lb.check(Lb.lib.gt_gemm_path_counts(g, 1 if reset else 0))
    return list(h), list(g)


class FlatView(object):
    """A torch tensor handed to the hooks as it is."""

    def __init__(self, t):
        self.t, self.n = t, t.numel()

    def ptr(self):
        return self.t.data_ptr()


def _hook_weff(tab, n_flat, flat, u, v):
    """gt_op_spectral_norm (iterate) on a model's flat parameters: (W_eff with the biases of `flat`, sigma); u, v advance in place."""
    weff = flat.clone()
    sigma = torch.zeros(len(tab), device="cuda")
    hook_prepare(tab, n_flat, FlatView(flat), FlatView(u), FlatView(v), FlatView(weff), FlatView(sigma), 1)
    return weff, sigma


# ---------------------------------------------------------------------------------------------------------------------
# 4. equivalence, no tolerance
# ---------------------------------------------------------------------------------------------------------------------
def _equivalence(name, obj="hinge", bf16=False):
    """clip_grad_norm_ scales the gradient in place by a coefficient formed from its own norm, and the two engines clip different gradients
    (the projected one, the plain one): both discriminator optimizers run with the clip off here (max_grad_norm = 0), so that the flat
    gradient buffers hold what the backward passes and the projection wrote.  The clip on the projected gradient is test 5's."""
    import test_gpu_d_tail as T
    case = G.STEP_CASES[name]
    tab, n_flat = S.flat_layout(_layers_of(case["d"]), lead=0)
    # the feature ON
    head_counts(reset=True)
    on = Run(case, obj, sn=True, bf16=bf16, d_clip_norm=0.0)
    W0, u, v = on.md.flat_params().clone(), on.md.sn_u.clone(), on.md.sn_v.clone()
    on.begin(0)
    d_on = on.d_step()
    torch.cuda.synchronize()
    W1, grad_on = on.md.flat_params().clone(), on.md.flat_grads().clone()
    weff1, sigma1 = _hook_weff(tab, n_flat, W0, u, v)
    u1, v1 = u.clone(), v.clone()
    assert np.array_equal(_bits(on.md.sn_u.cpu().numpy()), _bits(u1.cpu().numpy())) and np.array_equal(_bits(on.md.sn_v.cpu().numpy()), _bits(v1.cpu().numpy()))
    g_on = on.g_step()
    torch.cuda.synchronize()
    head_on = head_counts(reset=True)[0]
    weff2, _ = _hook_weff(tab, n_flat, W1, u, v)
    assert np.array_equal(_bits(on.md.sn_u.cpu().numpy()), _bits(u.cpu().numpy())) and np.array_equal(_bits(on.md.sn_v.cpu().numpy()), _bits(v.cpu().numpy()))
    gG_on, pG_on = on.mg.flat_grads().clone(), on.mg.flat_params().clone()
    # the feature OFF, on the hook's W_eff; its optimizer never moves the weights (lr = 0), so the G step sees exactly what is written there
    off = Run(case, obj, sn=False, bf16=bf16, d_lr=0.0, d_clip_norm=0.0)
    off.md.flat_params().copy_(weff1)
    off.begin(0)
    d_off = off.d_step()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(off.md.flat_params().cpu().numpy()), _bits(weff1.cpu().numpy()))
    grad_off = off.md.flat_grads().clone()
    off.md.flat_params().copy_(weff2)
    g_off = off.g_step()
    torch.cuda.synchronize()
    head_off = head_counts(reset=True)[0]
    print("SNEQ %s %s bf16=%s D on %s off %s | G on %s off %s" % (name, obj, bf16, d_on.tolist(), d_off.tolist(), g_on.tolist(), g_off.tolist()))
    assert np.array_equal(_bits(d_on), _bits(d_off)), "D step: losses and counts"
    assert np.array_equal(_bits(g_on), _bits(g_off)), "G step: losses"
    # the y-side gradients (the kept dloss_d / dy_hat_static and the adversarial term's) reach G's gradient and update: bit for bit
    assert np.array_equal(_bits(gG_on.cpu().numpy()), _bits(off.mg.flat_grads().cpu().numpy()))
    assert np.array_equal(_bits(pG_on.cpu().numpy()), _bits(off.mg.flat_params().cpu().numpy()))
    # D's gradient = the OFF engine's gradient through gt_op_sn_project
    s = torch.zeros(len(tab), dtype=torch.float64, device="cuda")
    parts = torch.zeros(2048, dtype=torch.float64, device="cuda")
    hook_project(tab, n_flat, FlatView(grad_off), FlatView(weff1), FlatView(u1), FlatView(v1), FlatView(sigma1), FlatView(s), FlatView(parts))
    assert np.array_equal(_bits(grad_on.cpu().numpy()), _bits(grad_off.cpu().numpy())), "D's gradient is not the projected one"
    assert head_on == head_off
    if case.get("fused"):
        assert head_on[T.DSTACK128] == 2, head_on       # both passes took the fused stack


@pytest.mark.parametrize("name", ["mlp32", "mlp128_fused", "mlp32_cond"])
def test_step_equals_plain_engine_on_hook_weff(name):
    _equivalence(name)


def test_bf16_shadows_are_cast_from_weff():
    _equivalence("mlp32", bf16=True)


# ---------------------------------------------------------------------------------------------------------------------
# 5. two G+D steps against the CPU step reference
# ---------------------------------------------------------------------------------------------------------------------
def _case_for(name, obj):
    case = G.STEP_CASES[name]
    return G.bce_twin(case) if obj == "bce" else case


@functools.lru_cache(maxsize=None)
def sn_reference(name, obj):
    return S.run_step_reference(_case_for(name, obj), obj)


@functools.lru_cache(maxsize=None)
def sn_run(name, obj):
    case = _case_for(name, obj)
    sn_counts(reset=True)
    head_counts(reset=True)
    r = Run(case, obj, sn=True)
    out = r.steps(case["steps"])
    out.update(r.state())
    return out, sn_counts(reset=True), head_counts(reset=True)


@pytest.mark.parametrize("obj", ["bce", "hinge"])
@pytest.mark.parametrize("name", ["mlp32", "mlp128_fused", "mlp32_cond"])
def test_two_steps_match_the_step_reference(name, obj):
    """The suite's 1e-4 (gan_objective_ref.step_close: per tensor scale, counts exactly); D.sn_u / D.sn_v are two more tensors of the run,
    unit vectors judged on their own scale: the float32 rounding bound of the hook test (6e-8 of an entry) widened by that tolerance."""
    import test_gpu_d_tail as T
    got, sn, (head, _) = sn_run(name, obj)
    ref = sn_reference(name, obj)
    for k in sorted(ref):
        if "scalars" in k:
            print("SNSTEP %s %s %s got %s ref %s" % (name, obj, k, got[k].tolist(), ref[k].tolist()))
    assert "D.sn_u" in ref and "D.sn_v" in ref
    bad = G.step_close(got, ref)
    assert not bad, "%s / %s: outside 1e-4 of the step reference: %s" % (name, obj, bad)
    steps = G.STEP_CASES[name]["steps"]
    assert sn == [2 * steps, 2 * steps, 2 * steps, steps, steps], sn      # 3 + 3 + 2 launches per G+D step
    if name == "mlp128_fused":
        assert head[T.DSTACK128] == 2 * steps, head


# ---------------------------------------------------------------------------------------------------------------------
# 6. eval, checkpoint and off
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_mode_leaves_u_and_v_alone():
    case = G.STEP_CASES["mlp32"]
    r = Run(case, "hinge", sn=True)
    r.steps(1)
    u, v = r.md.sn_u.clone(), r.md.sn_v.clone()
    r.mg.eval(), r.md.eval()
    r.begin(1)
    sn_counts(reset=True)
    d, g = r.d_step("test"), r.g_step("test")
    for p in range(3):
        r.md.set_dropout_masks(p, None)      # (the injected masks are the step batch's; the forward below has its own shape)
    out = r.md(torch.rand(2, 5, case["d"]["in_dim"], device="cuda"))      # the model's own forward (the spoofing rate's path): eval form too
    torch.cuda.synchronize()
    assert sn_counts(reset=True) == [0, 3, 3, 0, 0]
    assert np.all(np.isfinite(d)) and np.all(np.isfinite(g)) and bool(torch.isfinite(out).all())
    assert torch.equal(r.md.sn_u, u) and torch.equal(r.md.sn_v, v)


def test_checkpoint_round_trip_continues_bit_identically(tmp_path):
    from gantts_amd import optim
    case = G.STEP_CASES["mlp32"]
    whole = Run(case, "hinge", sn=True)
    whole.steps(2)
    want = whole.state()
    first = Run(case, "hinge", sn=True)
    first.steps(1)
    Tr = first.Tr
    paths = [Tr.save_checkpoint(m, o, 1, str(tmp_path), n) for m, o, n in ((first.mg, first.og, "Generator"), (first.md, first.od, "Discriminator"))]
    second = Run(case, "hinge", sn=True)
    assert not torch.equal(second.md.sn_u, first.md.sn_u)
    Tr.load_checkpoint(second.mg, second.og, paths[0])
    Tr.load_checkpoint(second.md, second.od, paths[1])
    assert torch.equal(second.md.sn_u, first.md.sn_u) and torch.equal(second.md.sn_v, first.md.sn_v)
    second.steps(1, first=1)
    got = second.state()
    assert sorted(got) == sorted(want) and "D.sn_u" in got
    for k in want:
        assert np.array_equal(_bits(want[k]), _bits(got[k])), k


def test_off_is_the_engine_that_never_saw_the_option():
    case = G.STEP_CASES["mlp32"]
    from gantts_amd import models
    assert sorted(build_d(case["d"], False).state_dict()) == sorted(models.MLP(**{k: v for k, v in case["d"].items() if k != "kind"}).state_dict())
    assert not any("sn_" in k for k in build_d(case["d"], False).state_dict())
    assert {"sn_u", "sn_v"} <= set(build_d(case["d"], True).state_dict())
    res = []
    for flag in (None, False):
        sn_counts(reset=True)
        head_counts(reset=True)
        r = Run(case, "hinge", sn=False, hp_flag=flag)
        out = r.steps(1)
        out.update(r.state())
        res.append((out, sn_counts(reset=True), head_counts(reset=True)))
    (a, sa, ha), (b, sb, hb) = res
    assert sa == sb == [0] * 5 and ha == hb
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(_bits(np.asarray(a[k])), _bits(np.asarray(b[k]))), k


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals, by message
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    Lb = _lb()
    from gantts_amd import models
    from gantts_amd.engine import StepEngine
    from hip_runner import build_model, make_hp
    case = G.STEP_CASES["mlp32"]
    hp = make_hp(case)
    hp.gan_objective = "hinge"
    hp.discriminator_spectral_norm = True
    md = build_d(case["d"], True)
    eng = StepEngine(hp)
    u, v = md.sn_u, md.sn_v
    # before a discriminator is bound; role G
    with pytest.raises(RuntimeError, match="bind the discriminator first"):
        eng.set_spectral_norm(Lb.ROLE_D, u, v)
    eng.bind_model(Lb.ROLE_D, md)
    with pytest.raises(ValueError, match="discriminator's \\(role 1\\) alone"):
        eng.set_spectral_norm(Lb.ROLE_G, u, v)
    with pytest.raises(ValueError, match="cannot be bound as the generator"):
        eng.bind_model(Lb.ROLE_G, md)
    # lengths against the bound model; one of the two missing
    with pytest.raises(ValueError, match="sum of out"):
        eng.set_spectral_norm(Lb.ROLE_D, u[:-1].contiguous(), v)
    with pytest.raises(ValueError, match="sum of out"):
        eng.set_spectral_norm(Lb.ROLE_D, u, torch.cat([v, v[:1]]))
    assert Lb.lib.gt_set_spectral_norm(eng._h, Lb.ROLE_D, Lb.ptr(u), None, u.numel(), 0) == Lb.GT_ERR_INVALID
    assert b"both given or both null" in Lb.lib.gt_last_error()
    # hp and model must agree
    hp_off = make_hp(case)
    hp_off.gan_objective = "hinge"
    with pytest.raises(ValueError, match="hp.discriminator_spectral_norm is False"):
        StepEngine(hp_off).bind_model(Lb.ROLE_D, md)
    with pytest.raises(ValueError, match="hp.discriminator_spectral_norm is True"):
        StepEngine(hp).bind_model(Lb.ROLE_D, build_d(case["d"], False))
    with pytest.raises(ValueError, match="out_dim = 1"):
        models.MLP(in_dim=8, out_dim=3, spectral_norm=True)
    # recurrent discriminators
    for kind in ("lstm", "sru"):
        e2 = StepEngine(hp_off)
        rec = build_model(G.STEP_CASES[kind]["d"], 22)
        e2.bind_model(Lb.ROLE_D, rec)
        with pytest.raises(ValueError, match="LSTMRNN or SRURNN discriminator is not supported"):
            e2.set_spectral_norm(Lb.ROLE_D, u, v)
    # sharded or communicating engines, in either order
    e3 = StepEngine(hp_off)
    e3.bind_model(Lb.ROLE_D, build_d(case["d"], False))
    e3.set_shard(0, 2)
    with pytest.raises(ValueError, match="sharded or communicating engine"):
        e3.set_spectral_norm(Lb.ROLE_D, u, v)
    with pytest.raises(ValueError, match="gt_set_shard: spectral normalisation"):
        eng.set_shard(1, 2)
    eng.set_shard(0, 1)          # (one shard is no shard)
    assert Lb.lib.gt_comm_init(eng._h, 0, 2, Ct.create_string_buffer(Lb.COMM_ID_BYTES)) == Lb.GT_ERR_INVALID
    assert b"gt_comm_init: spectral normalisation" in Lb.lib.gt_last_error()
    # the hooks: a layer wider than 512, overlapping ranges -- refused before any launch
    sn_counts(reset=True)
    fake = 256
    for tab, n_flat, msg in (([(0, 513, 4, 0, 0)], 4096, b"[1, 512]"), ([(0, 4, 4, 0, 0), (8, 4, 4, 4, 4)], 64, b"overlaps"),
                             ([(0, 4, 4, 0, 0)], 15, b"leaves the flat buffer")):
        c = sn_case(tab, n_flat, 1, W=fake, u=fake, v=fake, weff=fake, sigma=fake)
        assert Lb.lib.gt_op_spectral_norm(Ct.byref(c), None) == Lb.GT_ERR_INVALID and msg in Lb.lib.gt_last_error(), Lb.lib.gt_last_error()
    assert sn_counts(reset=True) == [0] * 5
    # a projected gradient is not accumulated into: zero_grad must precede the next D step
    r = Run(case, "hinge", sn=True)
    r.begin(0)
    r.d_step()
    with pytest.raises(RuntimeError, match="zero_grad\\(\\) must precede update_discriminator"):
        r.d_step()
