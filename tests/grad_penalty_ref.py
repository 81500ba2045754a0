"""References of the discriminator's gradient penalties (gt_set_grad_penalty: "r1", "wgan-gp") for tests/test_grad_penalty_host.py and
tests/test_gpu_grad_penalty.py.  Nothing here needs a GPU.

Two levels:
  * the closed form of DESIGN.md 7.1 in float64 numpy (`closed_form`), carrying a per-element error bound through every product as
    tests/test_gpu_d_tail.py's chain does: unit roundoff U = 2^-24 per term of a float32 product (K + 3 for a K-term sum in ANY order,
    the split-K weight gradients included), one more per stored or rescaled intermediate, operand errors propagated through |B|.
    `mistake=` plants one of MISTAKES; dtype=np.float32 evaluates the same statements in float32 (the stand-in for a device on the
    host, what the comparators must accept);
  * per step, in torch on the CPU: `run_step_reference` runs gan_objective_ref.run_step_reference with its update_discriminator wrapped:
    the penalty's double backward (torch.autograd.grad(..., create_graph=True)) adds to the .grad of the discriminator's parameters
    before the wrapped function back-propagates the adversarial loss, clips and steps.
Notation per layer: slope s_l = (1 or 0.01) x (0 or 1 / (1 - p)), LeakyReLU's derivative times the dropout factor."""
import numpy as np
import torch

import gan_objective_ref as G
import gantts_oracle as O

U = 2.0 ** -24
KINDS = {"r1": 1, "wgan-gp": 2}
SLOPE = float(np.float32(0.01))
EPS_N = 1e-12
MISTAKES = ("inv_tv_dropped", "mask_dropped", "bias_gradient_written", "cond_columns_in_norm", "slopes_from_wrong_pass", "n_minus_1",
            "factor_2_dropped")


def slopes_of(h, keep, p):
    """s_l from a stored activation h = dropout(leaky(pre)) and its keep mask, as the backward-data epilogue recovers it (float64)."""
    scale = float(np.float32(1.0) / np.float32(1.0 - p)) if p > 0 else 1.0
    lo = float(np.float32(SLOPE) * np.float32(scale))
    keep = np.ones(h.shape, dtype=bool) if keep is None else (np.asarray(keep) != 0)
    return np.where(keep, np.where(h > 0, scale, lo), 0.0)


def _prod(A, EA, B, EB=None):
    """A @ B with its bound: (K + 3) U |A| |B| + EA |B| (+ |A| EB + EA EB)."""
    K = A.shape[1]
    C = A @ B
    S = np.abs(A) @ np.abs(B)
    E = (K + 3) * U * S + EA @ np.abs(B)
    if EB is not None:
        E = E + np.abs(A) @ EB + EA @ EB
    return C, E


def _sloped(v, Ev, s):
    """s (.) v: two roundings in the epilogue and one in the slope constant."""
    out = v * s
    return out, Ev * np.abs(s) + 3 * U * np.abs(out)


def closed_form(kind, weight, Ws, w_last, slopes, mask, inv_tv, cd, Da, mistake=None, slopes_alt=None, dtype=np.float64):
    """Ws[l] (H, in_l), in_0 = cd + Da; w_last (H,); slopes[l] (rows, H); mask (rows,).  Returns a dict: g, r, a[l], c[l], phi, n, the
    increments dW0 (H, cd + Da: zero outside the adversarial columns), dW[l] (l >= 1), dw_last, db[l] / db_last (zeros), the sums
    s_phi = sum mask phi, s_n = sum mask n, P and mean_n (x inv_tv); every array X has its bound under "E_" + name."""
    f = dtype
    L = len(Ws)
    Ws = [np.asarray(W, dtype=f) for W in Ws]
    w_last = np.asarray(w_last, dtype=f)
    if mistake == "slopes_from_wrong_pass":
        slopes = slopes_alt
    s = [np.asarray(x, dtype=f) for x in slopes]
    m = np.asarray(mask, dtype=f)
    rows = m.shape[0]
    it = f(1.0) if mistake == "inv_tv_dropped" else f(inv_tv)
    mu = (np.ones_like(m) if mistake == "mask_dropped" else m) * it
    lam = f(weight)
    out = {}
    a, Ea = [None] * L, [None] * L
    a[L - 1] = s[L - 1] * w_last[None, :]
    Ea[L - 1] = 2 * U * np.abs(a[L - 1])
    for l in range(L - 1, 0, -1):
        v, Ev = _prod(a[l], Ea[l], Ws[l])
        a[l - 1], Ea[l - 1] = _sloped(v, Ev, s[l - 1])
    W0a = Ws[0][:, cd:cd + Da]
    g, Eg = _prod(a[0], Ea[0], W0a)
    gn, Egn = (g, Eg) if mistake != "cond_columns_in_norm" else _prod(a[0], Ea[0], Ws[0])
    ss = (gn * gn).sum(1)
    Ess = (2 * np.abs(gn) * Egn + Egn * Egn).sum(1) + (gn.shape[1] + 3) * U * ss
    n = np.sqrt(ss + f(EPS_N))
    En = Ess / n + 3 * U * n          # |sqrt(x) - sqrt(y)| <= |x - y| / sqrt(x)
    if kind == "r1":
        phi = f(0.5) * lam * ss
        Ephi = 0.5 * abs(float(lam)) * Ess + 3 * U * np.abs(phi)
        k = lam * mu
        Ek = 2 * U * np.abs(k)
    else:
        d = n - f(1.0)
        Ed = En + U * np.abs(d)
        phi = lam * d * d
        Ephi = abs(float(lam)) * (2 * np.abs(d) * Ed + Ed * Ed) + 3 * U * np.abs(phi)
        fac = (n - f(1.0)) if mistake == "n_minus_1" else (f(1.0) - f(1.0) / n)
        Efac = En / (n * n) + 2 * U / n + U * np.abs(fac)
        two = f(1.0) if mistake == "factor_2_dropped" else f(2.0)
        k = two * lam * mu * fac
        Ek = np.abs(two * lam * mu) * Efac + 4 * U * np.abs(k)
    r = k[:, None] * g
    Er = np.abs(k)[:, None] * Eg + Ek[:, None] * np.abs(g) + Ek[:, None] * Eg + U * np.abs(r)
    c, Ec = [None] * L, [None] * L
    v, Ev = _prod(r, Er, W0a.T)
    c[0], Ec[0] = _sloped(v, Ev, s[0])
    for l in range(1, L):
        v, Ev = _prod(c[l - 1], Ec[l - 1], Ws[l].T)
        c[l], Ec[l] = _sloped(v, Ev, s[l])
    dW0 = np.zeros_like(Ws[0])
    EdW0 = np.zeros(Ws[0].shape)
    inc, Einc = _prod(a[0].T, Ea[0].T, r, Er)
    dW0[:, cd:cd + Da], EdW0[:, cd:cd + Da] = inc, Einc
    out["dW0"], out["E_dW0"] = dW0, EdW0
    for l in range(1, L):
        out["dW%d" % l], out["E_dW%d" % l] = _prod(a[l].T, Ea[l].T, c[l - 1], Ec[l - 1])
    out["dw_last"] = c[L - 1].sum(0)
    out["E_dw_last"] = (rows + 3) * U * np.abs(c[L - 1]).sum(0) + Ec[L - 1].sum(0)
    for l in range(L):
        out["db%d" % l] = c[l].sum(0) if mistake == "bias_gradient_written" else np.zeros(Ws[l].shape[0], dtype=f)
        out["a%d" % l], out["E_a%d" % l], out["c%d" % l], out["E_c%d" % l] = a[l], Ea[l], c[l], Ec[l]
    out["db_last"] = np.zeros(1, dtype=f)
    out.update(g=g, E_g=Eg, r=r, E_r=Er, phi=phi, E_phi=Ephi, n=n, E_n=En)
    mm = np.asarray(mask, dtype=np.float64)
    out["s_phi"], out["s_n"] = float((mm * phi).sum()), float((mm * n).sum())
    out["E_s_phi"], out["E_s_n"] = float((mm * Ephi).sum()), float((mm * En).sum())
    out["P"], out["mean_n"] = out["s_phi"] * float(inv_tv), out["s_n"] * float(inv_tv)
    return out


ARRAYS = ("g", "r", "phi", "n")


def compare(got, ref, L, slack=1.0, base=None):
    """Every element of got[name] within slack x ref["E_" + name] of ref[name] (plus the float32 rounding of the stored value); bias
    increments exactly zero; the two sums within their bounds.  base[name]: what a gradient held before its increment was added (the
    stored sum is rounded once more, on its own scale).  Returns the names that miss."""
    names = list(ARRAYS) + ["a%d" % l for l in range(L)] + ["c%d" % l for l in range(L)] + ["dW0", "dw_last"] + ["dW%d" % l for l in range(1, L)]
    bad = []
    for k in names:
        gk, rk = np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64)
        tol = slack * ref["E_" + k] + U * np.abs(rk) + 1e-300
        if base is not None and k in base:
            tol = tol + 2 * U * (np.abs(np.asarray(base[k], dtype=np.float64)) + np.abs(rk))
        if gk.shape != rk.shape or not np.all(np.abs(gk - rk) <= tol):
            bad.append(k)
    for k in ["db%d" % l for l in range(L)] + ["db_last"]:
        if np.any(np.asarray(got[k]) != 0):
            bad.append(k)
    for k in ("s_phi", "s_n"):
        if not abs(got[k] - ref[k]) <= slack * ref["E_" + k] + 1e-12 * abs(ref[k]):
            bad.append(k)
    return bad


# ---------------------------------------------------------------------------------------------------------------------
# torch: the penalty by double backward
# ---------------------------------------------------------------------------------------------------------------------
def mlp_logit(params, inp, masks, p, training=True):
    """The MLP discriminator up to the output layer's pre-activation z (oracle.OracleMLP.forward without the sigmoid)."""
    L = len(params) // 2 - 1
    x = inp
    for i in range(L):
        x = torch.nn.functional.leaky_relu(torch.nn.functional.linear(x, params[2 * i], params[2 * i + 1]), SLOPE)
        if training and p > 0:
            x = x * masks[i] / (1.0 - p)
    return torch.nn.functional.linear(x, params[-2], params[-1])


def penalty_torch(kind, weight, params, cond, adv, masks, p, mask, Tv, training=True):
    """P and the masked mean norm, on the graph: `adv` must require grad (or be a function of something that does)."""
    inp = torch.cat((cond, adv), -1) if cond is not None else adv
    z = mlp_logit(params, inp, masks, p, training)
    g, = torch.autograd.grad(z.sum(), adv, create_graph=True)
    ss = (g * g).sum(-1, keepdim=True)
    n = torch.sqrt(ss + EPS_N)
    phi = 0.5 * weight * ss if kind == "r1" else weight * (n - 1.0) ** 2
    return (phi * mask).sum() / Tv, (n * mask).sum() / Tv, g


def run_step_reference(case, obj, kind, weight, eps_of_step=None, masks3_of_step=None, clip=0.0):
    """gan_objective_ref.run_step_reference with the penalty inside every D step.  eps_of_step(step) -> (B, T, 1) float32 array,
    masks3_of_step(step) -> the pass-3 dropout masks (wgan-gp).  Adds "gp_record": [mean P, mean norm] over the steps."""
    orig = G.update_discriminator
    state = dict(step=0, P=[], n=[])

    def wrapped(obj_, cfg, model_d, optimizer_d, x, y_static, y_hat_static, lengths, mask, phase, eps=1e-20, drop=None, clip=0.0, mistake=None):
        if phase == "train" and kind is not None:
            L = model_d.num_hidden
            p = model_d.p
            sel = (lambda t: t[:, :, cfg.adv_cols()]) if cfg.adversarial_streams is not None else (lambda t: t)
            cond = x if cfg.discriminator_linguistic_condition else None
            Tv = mask.sum().item()
            if kind == "r1":
                adv = sel(y_static).detach().clone().requires_grad_(True)
                masks = list(drop.masks[:L]) if (drop is not None and drop.masks is not None and model_d.training and p > 0) else None
            else:
                e = torch.from_numpy(np.asarray(eps_of_step(state["step"]), dtype=np.float32))
                adv = e * sel(y_static) + (1.0 - e) * sel(y_hat_static)
                masks = [torch.from_numpy(m) for m in masks3_of_step(state["step"])] if (model_d.training and p > 0) else None
            P, nm, _ = penalty_torch(kind, weight, model_d.params, cond, adv, masks, p, mask, Tv, model_d.training)
            P.backward(retain_graph=True)
            state["P"].append(P.item())
            state["n"].append(nm.item())
        state["step"] += 1
        return orig(obj_, cfg, model_d, optimizer_d, x, y_static, y_hat_static, lengths, mask, phase, eps=eps, drop=drop, clip=clip, mistake=mistake)

    G.update_discriminator = wrapped
    try:
        out = G.run_step_reference(case, obj, clip=clip)
    finally:
        G.update_discriminator = orig
    if kind is not None:
        out["gp_record"] = np.array([np.mean(state["P"]), np.mean(state["n"])], dtype=np.float64)
    return out
