"""The gradient penalties' float64 closed form (tests/grad_penalty_ref.py) against torch's double backward, and its comparators against
seeded mistakes.  Runs on the CPU."""
import numpy as np
import pytest
import torch

import grad_penalty_ref as R

L_, H_, CD, DA, ROWS, P_DROP = 3, 16, 5, 7, 40, 0.5
SEED = {"r1": 3, "wgan-gp": 4}
WEIGHT = 10.0
KINK_MARGIN = 64.0          # test_gpu_gan_objective.py::condition_margin: more than 64 error bounds away from every kink


def instance(kind, seed=None):
    """3 hidden layers, conditioning columns, fixed dropout masks (two passes: the second is the "wrong pass"), a ragged mask."""
    rs = np.random.RandomState(1000 + (SEED[kind] if seed is None else seed))
    ins = [CD + DA] + [H_] * (L_ - 1)
    Ws = [rs.randn(H_, i) / np.sqrt(i) for i in ins]
    bs = [0.1 * rs.randn(H_) for _ in ins]
    w_last, b_last = rs.randn(H_) / np.sqrt(H_), 0.1 * rs.randn(1)
    cond, adv = rs.randn(ROWS, CD), rs.randn(ROWS, DA)
    keeps = [[(rs.rand(ROWS, H_) >= P_DROP).astype(np.float64) for _ in range(L_)] for _ in range(2)]
    lengths = [ROWS // 2, ROWS // 2 - 7]
    mask = np.concatenate([(np.arange(ROWS // 2) < n).astype(np.float64) for n in lengths])
    inst = dict(kind=kind, Ws=Ws, bs=bs, w_last=w_last, b_last=b_last, cond=cond, adv=adv, keeps=keeps, mask=mask, inv_tv=1.0 / mask.sum())
    # the gradient's norm is linear in w_last: scale it so that the median row has n = 1
    fw = forward(inst, 0)
    ref = R.closed_form(kind, WEIGHT, Ws, w_last, fw["slopes"], mask, inst["inv_tv"], CD, DA)
    inst["w_last"] = w_last / np.median(ref["n"])
    # The discriminator is framewise: a row that misses the input condition (a pre-activation within KINK_MARGIN bounds of the kink in
    # either pass; for wgan-gp a norm outside [0.25, 4]) is drawn again from the same stream, as tests/test_gpu_d_tail.py redraws frames
    for _ in range(500):
        todo = np.flatnonzero(~rows_ok(inst))
        if not todo.size:
            break
        inst["cond"][todo], inst["adv"][todo] = rs.randn(len(todo), CD), rs.randn(len(todo), DA)
        for which in range(2):
            for l in range(L_):
                inst["keeps"][which][l][todo] = (rs.rand(len(todo), H_) >= P_DROP).astype(np.float64)
    assert rows_ok(inst).all()
    return inst


def rows_ok(inst):
    ok = np.ones(ROWS, dtype=bool)
    for which in (0, 1):
        fw = forward(inst, which)
        for p, E in zip(fw["pres"], fw["Epres"]):
            ok &= (np.abs(p) / E).min(1) > 2 * KINK_MARGIN
    if inst["kind"] == "wgan-gp":
        n = R.closed_form(inst["kind"], WEIGHT, inst["Ws"], inst["w_last"], forward(inst, 0)["slopes"], inst["mask"], inst["inv_tv"], CD, DA)["n"]
        ok &= (n >= 0.3) & (n <= 3.5)
    return ok


def forward(inst, which):
    """Pre-activations, their float32 error bound (K + 3) U |x| |W| + ..., and the slopes of pass `which`, in float64."""
    x = np.concatenate([inst["cond"], inst["adv"]], 1)
    Ex = np.zeros(x.shape)
    pres, Epres, slopes = [], [], []
    scale = 1.0 / (1.0 - P_DROP)
    for l in range(L_):
        pre = x @ inst["Ws"][l].T + inst["bs"][l]
        Epre = (x.shape[1] + 3) * R.U * (np.abs(x) @ np.abs(inst["Ws"][l]).T + np.abs(inst["bs"][l])) + Ex @ np.abs(inst["Ws"][l]).T
        s = np.where(pre > 0, 1.0, R.SLOPE) * inst["keeps"][which][l] * scale
        pres.append(pre), Epres.append(Epre), slopes.append(s)
        x, Ex = pre * s, Epre * np.abs(s) + 3 * R.U * np.abs(pre * s)
    return dict(pres=pres, Epres=Epres, slopes=slopes)


def torch_double_backward(inst, which=0):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    params = []
    for W, b in zip(inst["Ws"], inst["bs"]):
        params += [t(W).requires_grad_(True), t(b).requires_grad_(True)]
    params += [t(inst["w_last"][None, :]).requires_grad_(True), t(inst["b_last"]).requires_grad_(True)]
    adv = t(inst["adv"]).requires_grad_(True)
    masks = [t(k) for k in inst["keeps"][which]]
    mask = t(inst["mask"])[:, None]
    P, nm, g = R.penalty_torch(inst["kind"], WEIGHT, params, t(inst["cond"]), adv, masks, P_DROP, mask, 1.0 / inst["inv_tv"])
    grads = torch.autograd.grad(P, params + [adv], allow_unused=True)
    return P.item(), nm.item(), g.detach().numpy(), [None if x is None else x.numpy() for x in grads]


@pytest.mark.parametrize("kind", ["r1", "wgan-gp"])
def test_inputs_are_well_conditioned(kind):
    inst = instance(kind)
    for which in (0, 1):
        fw = forward(inst, which)
        margin = min(float((np.abs(p) / E).min()) for p, E in zip(fw["pres"], fw["Epres"]))
        assert margin > KINK_MARGIN, (kind, which, margin)
    ref = R.closed_form(kind, WEIGHT, inst["Ws"], inst["w_last"], forward(inst, 0)["slopes"], inst["mask"], inst["inv_tv"], CD, DA)
    if kind == "wgan-gp":
        assert ref["n"].min() >= 0.25 and ref["n"].max() <= 4.0, (ref["n"].min(), ref["n"].max())
    assert (inst["mask"] == 0).any() and (inst["mask"] == 1).any()


@pytest.mark.parametrize("kind", ["r1", "wgan-gp"])
def test_closed_form_equals_torch_double_backward(kind):
    inst = instance(kind)
    ref = R.closed_form(kind, WEIGHT, inst["Ws"], inst["w_last"], forward(inst, 0)["slopes"], inst["mask"], inst["inv_tv"], CD, DA)
    P, nm, g, grads = torch_double_backward(inst)
    close = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-10 * max(1.0, np.abs(np.asarray(b)).max())
    assert close(ref["P"], P) and close(ref["mean_n"], nm) and close(ref["g"], g)
    for l in range(L_):
        assert close(ref["dW%d" % l], grads[2 * l]), l
        assert grads[2 * l + 1] is None or not np.any(grads[2 * l + 1]), l          # biases: exactly nothing
    assert not np.any(grads[0][:, :CD])                                           # W_0[:, :cd]: exactly nothing
    assert close(ref["dw_last"], grads[2 * L_][0])
    assert grads[2 * L_ + 1] is None or not np.any(grads[2 * L_ + 1])
    assert grads[-1] is None or not np.any(grads[-1])                              # the sample itself: slopes have zero derivative


def _f32_stand_in(inst, **kw):
    return R.closed_form(inst["kind"], WEIGHT, inst["Ws"], inst["w_last"], forward(inst, 0)["slopes"], inst["mask"], np.float32(inst["inv_tv"]), CD, DA,
                         slopes_alt=forward(inst, 1)["slopes"], dtype=np.float32, **kw)


@pytest.mark.parametrize("kind", ["r1", "wgan-gp"])
def test_comparators_accept_float32_and_reject_seeded_mistakes(kind):
    inst = instance(kind)
    Ws32 = [W.astype(np.float32).astype(np.float64) for W in inst["Ws"]]
    inst = dict(inst, Ws=Ws32, w_last=inst["w_last"].astype(np.float32).astype(np.float64))
    ref = R.closed_form(kind, WEIGHT, inst["Ws"], inst["w_last"], forward(inst, 0)["slopes"], inst["mask"], float(np.float32(inst["inv_tv"])), CD, DA)
    assert R.compare(_f32_stand_in(inst), ref, L_) == []
    for mistake in R.MISTAKES:
        if kind == "r1" and mistake in ("n_minus_1", "factor_2_dropped"):
            continue                                                               # (wgan-gp's factor)
        bad = R.compare(_f32_stand_in(inst, mistake=mistake), ref, L_)
        assert bad, mistake


def test_the_penalty_wrapper_changes_the_step_reference_and_only_the_discriminator():
    """run_step_reference with kind=None is gan_objective_ref's own; with "r1" the discriminator's weights move, its first-step losses
    (computed before any update) do not."""
    import gan_objective_ref as G
    case = dict(G.bce_twin(G.STEP_CASES["mlp32"]), steps=1)
    base = G.run_step_reference(case, "bce")
    same = R.run_step_reference(case, "bce", None, 0.0)
    on = R.run_step_reference(case, "bce", "r1", 10.0)
    for k in base:
        assert np.array_equal(np.asarray(base[k]), np.asarray(same[k])), k
    assert np.array_equal(base["d_scalars_0"], on["d_scalars_0"])
    assert not np.array_equal(base["D.layers.0.weight"], on["D.layers.0.weight"])
    assert on["gp_record"][0] > 0 and on["gp_record"][1] > 0
