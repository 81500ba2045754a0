"""GT_OPT_SRU_D_BF16 without a device: the option's id, and the CPU model of its arithmetic (tests/bf16_sru_model.py) that the GPU tests
(tests/test_gpu_sru_d_bf16.py) judge the engine against."""
import os
import re

import numpy as np
import torch

import gantts_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_id_matches_the_header_and_is_unique():
    from gantts_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "gantts_hip.h")).read()
    # the gt_set_option ids: every GT_OPT_* define except the optimizer kinds (GT_OPT_ADAGRAD .. GT_OPT_ADAMAX, another namespace)
    kinds = {"ADAGRAD", "ADAM", "SGD", "RMSPROP", "ADADELTA", "ADAMW", "ADAMAX"}
    ids = {n: int(v) for n, v in re.findall(r"^#define GT_OPT_(\w+) (\d+)\b", text, flags=re.M) if n not in kinds}
    assert ids["SRU_D_BF16"] == 20 == L.OPT_SRU_D_BF16
    assert [n for n, v in ids.items() if v == ids["SRU_D_BF16"]] == ["SRU_D_BF16"]
    assert len(set(ids.values())) == len(ids)
    # ... and in the Python table
    py = {n: getattr(L, n) for n in dir(L) if n.startswith("OPT_") and n[4:] not in kinds}
    assert [n for n, v in py.items() if v == L.OPT_SRU_D_BF16] == ["OPT_SRU_D_BF16"]


def test_bf16_operand_model_is_the_oracle_on_bf16_representable_operands():
    """One layer, k = 4, weights and input already bf16-representable, no dropout: rounding the operands of U = x . W changes nothing,
    so the model's forward equals OracleSRURNN's bit for bit, and with it every gradient that does not pass through the product's
    backward (the SRU bias, hidden2out).  The gradients of W and x do pass through it, and there the model rounds the incoming
    gradient g = dL/dU, which no choice of inputs makes representable: they are held to the bound that rounding implies,
    |dW_model - dW_oracle| <= 2^-8 |x|^T |g| (round to nearest: 2^-9 relative per element of g, doubled for the float32 sums),
    with g identical in both runs because everything upstream of it is."""
    from bf16_sru_model import Bf16OperandSRURNN, Bf16Product, r
    kw = dict(in_dim=10, out_dim=1, num_hidden=1, hidden_dim=8, bidirectional=True, last_sigmoid=True, use_relu=1)
    mo, mb = O.OracleSRURNN(seed=3, **kw), Bf16OperandSRURNN(seed=3, **kw)
    assert mo.ks == [4]
    gen = torch.Generator().manual_seed(7)
    sd = {n: p.detach().clone() for n, p in zip(mo.names, mo.params)}
    sd["gru.rnn_lst.0.weight"] = r(sd["gru.rnn_lst.0.weight"])
    sd["gru.rnn_lst.0.bias"] = torch.rand(32, generator=gen) - 0.5
    mo.load_state_dict(sd), mb.load_state_dict(sd)
    mo.training = mb.training = False
    x0 = r(torch.rand(3, 7, 10, generator=gen) * 2 - 1)
    xo, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    yo, yb = mo(xo), mb(xb)
    assert torch.equal(yo, yb)
    w = torch.rand(3, 7, 1, generator=gen)
    Bf16Product.seen = []
    try:
        (yo * w).sum().backward()
        (yb * w).sum().backward()
        (g,) = Bf16Product.seen
    finally:
        Bf16Product.seen = None
    by_name = lambda m: dict(zip(m.names, m.params))      # noqa: E731
    po, pb = by_name(mo), by_name(mb)
    for n in ("gru.rnn_lst.0.bias", "hidden2out.weight", "hidden2out.bias"):
        assert torch.equal(po[n].grad, pb[n].grad), n
    W = po["gru.rnn_lst.0.weight"].detach()
    lim_w = 2.0 ** -8 * (x0.abs().reshape(-1, 10).t() @ g.abs().reshape(-1, g.shape[-1]))
    lim_x = 2.0 ** -8 * (g.abs() @ W.abs().t())
    dw, dx = (po["gru.rnn_lst.0.weight"].grad - pb["gru.rnn_lst.0.weight"].grad).abs(), (xo.grad - xb.grad).abs()
    assert float(dw.max()) > 0 and float(dx.max()) > 0      # (the rounding of g is there)
    assert bool((dw <= lim_w).all()) and bool((dx <= lim_x).all()), (float((dw / lim_w).max()), float((dx / lim_x).max()))
    # and the model's backward is the stated formula on that g
    assert torch.equal(pb["gru.rnn_lst.0.weight"].grad, x0.reshape(-1, 10).t() @ r(g).reshape(-1, g.shape[-1]))
    assert torch.equal(xb.grad, r(g) @ W.t())


def test_bf16_operand_model_is_measurably_away_from_the_float32_oracle():
    """The condition of the GPU test's rule (b), checked where no GPU is needed: on fold_bi_k4_cond at least one discriminator tensor of
    the bf16-operand model is 10 RTOL (relative rms) away from the float32 oracle's, and the classification counts agree."""
    from bf16_sru_model import run_bf16_model_case
    from oracle_runner import run_oracle_case
    from test_gpu_parity import RTOL
    from test_gpu_sru_d_bf16 import BF16_CASES, _d
    case = BF16_CASES["fold_bi_k4_cond"]
    F, M = run_oracle_case(case), run_bf16_model_case(case)
    far = [k for k in F if k.startswith("D.") and _d(M[k], F[k], F[k]) >= 10 * RTOL]
    print("%d discriminator tensors at >= 10 RTOL: %s" % (len(far), far))
    assert len(far) >= 1
    for st in range(case["steps"]):
        assert np.array_equal(F["d_scalars_%d" % st][3:], M["d_scalars_%d" % st][3:])
    for k in ("y_hat", "y_hat_static"):      # the generator is the float32 oracle's in both
        assert np.array_equal(F[k], M[k]), k
