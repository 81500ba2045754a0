"""Spectral normalisation of the MLP discriminator (gt_set_spectral_norm), restated in float64 numpy: the power iteration, the eval form and
the gradient's projection -- what tests/test_spectral_norm_host.py holds against torch.nn.utils.spectral_norm -- the comparators of the GPU
test with their derived bounds, a float32 emulation of the kernels' arithmetic that the host test feeds them (with seeded mistakes), and
the CPU step reference of the two-step runs.

Per nn.Linear weight W (out, in), unit vectors u (out), v (in), eps = 1e-12:
    iterate   t = W^T u;  v' = t / max(|t|, eps);  r = W v';  u' = r / max(|r|, eps);  sigma = u'^T r;  W_eff = W / sigma
    eval      sigma = u^T W v;  W_eff = W / sigma                                 (u, v unchanged)
    project   s = sum G (.) W_eff;  dL/dW = (G - s u' v'^T) / sigma               (G = dL/dW_eff; u', v' constants)
The engine runs ONE iteration per discriminator pass in training mode: one in the D step (a single 2N-row pass), one in the generator
step's adversarial pass.

Bounds.  U = 2^-53.  A sum of K exact products accumulated in double in any order is off by at most gamma(K - 1) sum|terms|, gamma(n) =
n U / (1 - n U) (Higham, Accuracy and Stability, 3.1); numpy's float64 reference carries the same bound, so device and reference differ
by at most 2 gamma(K) sum|terms|.  Norms, quotients and the single float32 rounding are propagated below, term by term."""
import numpy as np

EPS = 1e-12
U = 2.0 ** -53
F32 = 2.0 ** -24          # relative half-ulp of float32 (round to nearest)
F32_TINY = 2.0 ** -149    # absolute floor: the smallest subnormal


def gamma(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ---------------------------------------------------------------------------------------------------------------------
def iterate(W, u, v=None):
    """One power iteration: (u', v', sigma, W_eff).  v is not read (torch's first statement overwrites it)."""
    W, u = np.asarray(W, np.float64), np.asarray(u, np.float64)
    t = W.T @ u
    v1 = t / max(np.linalg.norm(t), EPS)
    r = W @ v1
    u1 = r / max(np.linalg.norm(r), EPS)
    sigma = float(u1 @ r)
    return u1, v1, sigma, W / sigma


def eval_form(W, u, v):
    W, u, v = (np.asarray(a, np.float64) for a in (W, u, v))
    sigma = float(u @ (W @ v))
    return sigma, W / sigma


def project(G, W_eff, u1, v1, sigma):
    """(dL/dW, s) from G = dL/dW_eff."""
    G, W_eff = np.asarray(G, np.float64), np.asarray(W_eff, np.float64)
    s = float((G * W_eff).sum())
    return (G - s * np.outer(u1, v1)) / sigma, s


# the float32 statements of the kernels, evaluated by numpy (IEEE single, one rounding per operation, no contraction)
def weff_bits(W32, sigma32):
    return np.asarray(W32, np.float32) / np.float32(sigma32)


def project_bits(G32, s, u32, v32, sigma32):
    """((G - (float(s) * u_i) * v_j) / sigma) in float32."""
    su = np.float32(s) * np.asarray(u32, np.float32)
    p = su[:, None] * np.asarray(v32, np.float32)[None, :]
    return (np.asarray(G32, np.float32) - p) / np.float32(sigma32)


# ---------------------------------------------------------------------------------------------------------------------
# comparators (raise AssertionError); every bound is carried in float64
# ---------------------------------------------------------------------------------------------------------------------
def _unit_bound(W, x, transpose):
    """y = (W^T x or W x) / |.| in float64 and the bound on a device value that forms the products exactly, sums them in double in any
    order, takes the norm and the quotient in double and rounds to float32 once."""
    A = W.T if transpose else W
    K = A.shape[1]
    t = A @ x
    dt = 2.0 * gamma(K) * (np.abs(A) @ np.abs(x))                 # device + reference double summation
    n = float(np.linalg.norm(t))
    assert n > 1e-6, "degenerate test input: |W x| = %g" % n
    # |n_dev - n| <= |dt|_2 (the vector's error) + n (gamma(K' + 2) + 4 U): squares, their sum, a square root within 2 ulp, both sides
    dn = float(np.linalg.norm(dt)) + 2.0 * n * (gamma(t.size + 2) + 4.0 * U)
    y = t / n
    pre = dt / (n - dn) + np.abs(t) * dn / (n * (n - dn)) + 4.0 * U * np.abs(y)      # numerator, denominator, the quotient's rounding
    return y, t, dt, pre + F32 * (np.abs(y) + pre) + F32_TINY


def check_iterate(W32, u_in, got_u, got_v, got_sigma):
    """Stage by stage, so that each bound holds one float32 rounding: v' from (W, u); u' from (W, the DEVICE's v'); sigma from (W, the
    device's u' and v')."""
    W = np.asarray(W32, np.float64)
    v_ref, _, _, bv = _unit_bound(W, np.asarray(u_in, np.float64), True)
    gv = np.asarray(got_v, np.float64)
    assert np.all(np.abs(gv - v_ref) <= bv), "v': worst excess %g" % float(np.max(np.abs(gv - v_ref) - bv))
    u_ref, r, dr, bu = _unit_bound(W, gv, False)
    gu = np.asarray(got_u, np.float64)
    assert np.all(np.abs(gu - u_ref) <= bu), "u': worst excess %g" % float(np.max(np.abs(gu - u_ref) - bu))
    check_sigma(gu, r, dr, got_sigma)


def check_sigma(u, r, dr, got_sigma):
    """sigma = u^T r: r off by dr, the products u_i r_i rounded once each (u float32, r double), their double sum, one float32 rounding."""
    s_ref = float(u @ r)
    pre = float(np.abs(u) @ dr) + 2.0 * gamma(u.size + 1) * float(np.abs(u) @ np.abs(r))
    b = pre + F32 * (abs(s_ref) + pre) + F32_TINY
    assert abs(float(got_sigma) - s_ref) <= b, "sigma %r vs %r: off by %g, bound %g" % (float(got_sigma), s_ref, abs(float(got_sigma) - s_ref), b)


def check_eval(W32, u32, v32, got_sigma):
    W, v = np.asarray(W32, np.float64), np.asarray(v32, np.float64)
    r = W @ v
    dr = 2.0 * gamma(W.shape[1]) * (np.abs(W) @ np.abs(v))
    check_sigma(np.asarray(u32, np.float64), r, dr, got_sigma)


def check_weff(W32, sigma32, got_weff):
    want = weff_bits(W32, sigma32)
    got = np.asarray(got_weff, np.float32)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), "W_eff is not the correctly rounded float32 W / sigma (%d elements differ)" % int(
        (want.view(np.uint32) != got.view(np.uint32)).sum())


def check_project(G32, weff32, u32, v32, sigma32, got_s, got_dW):
    """s within the double-sum bound of its float64 value; every element bit for bit the float32 expression evaluated from the device's s."""
    G, We = np.asarray(G32, np.float64), np.asarray(weff32, np.float64)
    s_ref = float((G * We).sum())
    b = 2.0 * gamma(G.size) * float((np.abs(G) * np.abs(We)).sum())
    assert abs(float(got_s) - s_ref) <= b, "s %r vs %r: off by %g, bound %g" % (float(got_s), s_ref, abs(float(got_s) - s_ref), b)
    want = project_bits(G32, got_s, u32, v32, sigma32)
    got = np.asarray(got_dW, np.float32)
    assert np.array_equal(want.view(np.uint32), got.view(np.uint32)), "projected gradient: %d elements differ from the float32 expression" % int(
        (want.view(np.uint32) != got.view(np.uint32)).sum())


def check_sqnorm(flat_grad32, partials):
    """The partials sum to the float64 squared norm of the whole flat gradient: squares rounded once each, two-stage double sums."""
    g = np.asarray(flat_grad32, np.float64)
    ref = float((g * g).sum())
    got = float(np.sum(np.asarray(partials, np.float64)))
    b = 2.0 * gamma(g.size + len(partials) + 1) * ref
    assert abs(got - ref) <= b, "squared norm %r vs %r: off by %g, bound %g" % (got, ref, abs(got - ref), b)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in numpy (float64 sums of exact products, float32 where the kernels round), with seeded mistakes: what the host
# test feeds the comparators above
# ---------------------------------------------------------------------------------------------------------------------
MISTAKES = ("project_sigma_missing", "s_from_W", "sigma_from_old_u", "v_not_renormalised", "iterates_in_eval")


def emulate_iterate(W32, u32, v32, mistake=None):
    W = np.asarray(W32, np.float64)
    t = W.T @ np.asarray(u32, np.float64)
    nt = 1.0 if mistake == "v_not_renormalised" else max(np.linalg.norm(t), EPS)
    v1 = (t / nt).astype(np.float32)
    r = W @ v1.astype(np.float64)
    u1 = (r / max(np.linalg.norm(r), EPS)).astype(np.float32)
    us = np.asarray(u32, np.float64) if mistake == "sigma_from_old_u" else u1.astype(np.float64)
    sigma = np.float32(us @ r)
    return u1, v1, sigma, weff_bits(W32, sigma)


def emulate_eval(W32, u32, v32, mistake=None):
    if mistake == "iterates_in_eval":
        return emulate_iterate(W32, u32, v32)
    sigma = np.float32(np.asarray(u32, np.float64) @ (np.asarray(W32, np.float64) @ np.asarray(v32, np.float64)))
    return np.asarray(u32, np.float32).copy(), np.asarray(v32, np.float32).copy(), sigma, weff_bits(W32, sigma)


def emulate_project(G32, W32, weff32, u32, v32, sigma32, mistake=None):
    other = np.asarray(W32 if mistake == "s_from_W" else weff32, np.float64)
    s = float((np.asarray(G32, np.float64) * other).sum())
    return s, project_bits(G32, s, u32, v32, np.float32(1.0) if mistake == "project_sigma_missing" else sigma32)


# ---------------------------------------------------------------------------------------------------------------------
# the flat buffer of the hook tests: weights with biases between them, so that no weight range but the first is 16-byte aligned
# ---------------------------------------------------------------------------------------------------------------------
HOOK_LAYERS = ((32, 58), (32, 91), (128, 128), (1, 128), (3, 1), (256, 483))


def flat_layout(layers=HOOK_LAYERS, lead=3):
    """[(w_off, out, in, u_off, v_off)], n_flat: `lead` floats that belong to no layer, then weight (out, in) and bias (out), layer after
    layer.  With lead = 3 the weights start at 3, 3, 3, 3, 0, 2 floats past a 16-byte boundary."""
    tab, off, uo, vo = [], lead, 0, 0
    for out, in_ in layers:
        tab.append((off, out, in_, uo, vo))
        off += out * in_ + out
        uo += out
        vo += in_
    return tab, off


def unit(x):
    return x / np.linalg.norm(x)


# ---------------------------------------------------------------------------------------------------------------------
# the CPU step reference: the oracle's MLP with every weight replaced by W / sigma under autograd
# ---------------------------------------------------------------------------------------------------------------------
class SpectralOracleMLP(object):
    """Wraps an OracleMLP: begin_pass() runs the pass's power iteration (training mode; u, v detached) or the eval form and builds
    W_eff = W / sigma as autograd functions of the wrapped parameters; forward() then multiplies by W_eff until the next begin_pass().
    params / names / state_dict are the wrapped model's: the optimizer updates W itself."""

    def __init__(self, mlp, u_list, v_list):
        import torch
        self.m = mlp
        self.params, self.names = mlp.params, mlp.names
        self.u = [torch.as_tensor(np.asarray(a, np.float32)).clone() for a in u_list]
        self.v = [torch.as_tensor(np.asarray(a, np.float32)).clone() for a in v_list]
        self.weff = None

    @property
    def training(self):
        return self.m.training

    @training.setter
    def training(self, value):
        self.m.training = value

    def state_dict(self):
        return self.m.state_dict()

    def begin_pass(self):
        import torch
        import torch.nn.functional as F
        self.weff = []
        for q in range(len(self.params) // 2):
            W = self.params[2 * q]
            if self.m.training:
                with torch.no_grad():
                    v = F.normalize(torch.mv(W.t(), self.u[q]), dim=0, eps=EPS)
                    u = F.normalize(torch.mv(W, v), dim=0, eps=EPS)
                    self.u[q], self.v[q] = u, v
            sigma = torch.dot(self.u[q], torch.mv(W, self.v[q]))
            self.weff.append(W / sigma)

    def forward(self, x, lengths=None, drop=None):
        import gantts_oracle as O
        import torch
        import torch.nn.functional as F
        m = self.m
        drop = drop or O._DropoutSource()
        for i in range(m.num_hidden):
            x = F.leaky_relu(F.linear(x, self.weff[i], m.params[2 * i + 1]), O.LEAKY_SLOPE)
            if m.training and m.p > 0:
                x = x * drop.next(x, m.p) / (1.0 - m.p)
        x = F.linear(x, self.weff[-1], m.params[-1])
        return torch.sigmoid(x) if m.last_sigmoid else x

    __call__ = forward


def initial_uv(spec, seed=5):
    """Deterministic unit vectors for an MLP spec, layer by layer in state_dict order: (u_list, v_list) float32."""
    rng = np.random.RandomState(seed)
    ins = [spec["in_dim"]] + [spec["hidden_dim"]] * (spec["num_hidden"] - 1) + [spec["hidden_dim"]]
    outs = [spec["hidden_dim"]] * spec["num_hidden"] + [spec["out_dim"]]
    u = [unit(rng.randn(o)).astype(np.float32) for o in outs]
    v = [unit(rng.randn(i)).astype(np.float32) for i in ins]
    return u, v


def run_step_reference(case, obj="bce"):
    """tests/gan_objective_ref.py's run_step_reference with the discriminator wrapped: one begin_pass() in front of the D step (its two
    forward calls are ONE pass of the engine) and one in front of the generator step's adversarial pass.  Same keys, plus D.sn_u / D.sn_v."""
    import torch
    import cases as C
    import gan_objective_ref as G
    import gantts_oracle as O
    from oracle_runner import build_oracle_model, stream_config
    cfg = stream_config(case)
    mg = build_oracle_model(case["g"], 11)
    u0, v0 = initial_uv(case["d"])
    md = SpectralOracleMLP(build_oracle_model(case["d"], 22), u0, v0)
    mg.training = md.training = bool(case["dropout_on"])
    og = O.make_optimizer(case["opt_g"][0], mg.params, **case["opt_g"][1])
    od = O.make_optimizer(case["opt_d"][0], md.params, **case["opt_d"][1])
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np), torch.from_numpy(y_np)
    R = torch.from_numpy(O.unit_variance_mlpg_matrix(C.WINDOWS[:case["windows"]], case["T"]))
    mask = O.sequence_mask(lengths).unsqueeze(-1)
    out = {}
    for step in range(case["steps"]):
        gm, dm = C.make_dropout_masks(case, step)
        dg = O._DropoutSource([torch.from_numpy(m) for m in gm])
        dd = O._DropoutSource([torch.from_numpy(m) for m in dm])
        y_static = O.get_static_features(y, cfg.num_windows, cfg.stream_sizes, cfg.has_dynamic_features)
        og.zero_grad(), od.zero_grad()
        y_hat, y_hat_static = O.apply_generator(cfg, mg, x, R, list(lengths), drop=dg)
        if step == 0:
            out["y_hat"] = y_hat.detach().numpy().copy()
            out["y_hat_static"] = y_hat_static.detach().numpy().copy()
        md.begin_pass()
        res = G.update_discriminator(obj, cfg, md, od, x, y_static, y_hat_static, list(lengths), mask, "train", drop=dd)
        out["d_scalars_%d" % step] = np.array(res, dtype=np.float64)
        md.begin_pass()
        res = G.update_generator(obj, cfg, mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], list(lengths), mask, "train",
                                 mse_w=case["mse_w"], mge_w=case["mge_w"], drop=dd)
        out["g_scalars_%d" % step] = np.array(res, dtype=np.float64)
    for k, v in mg.state_dict().items():
        out["G." + k] = v.numpy()
    for k, v in md.state_dict().items():
        out["D." + k] = v.numpy()
    for tag, opt, model in (("G", og, mg), ("D", od, md)):
        for i, name in enumerate(model.names):
            out["%s.opt.sum.%s" % (tag, name)] = opt.sum[i].numpy()
    out["D.sn_u"] = np.concatenate([a.numpy() for a in md.u])
    out["D.sn_v"] = np.concatenate([a.numpy() for a in md.v])
    return out
