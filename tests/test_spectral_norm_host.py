"""Host checks of the spectral-normalisation references (tests/spectral_norm_ref.py): the float64 restatement against
torch.nn.utils.spectral_norm itself, and the comparators of tests/test_gpu_spectral_norm.py against seeded mistakes.  Nothing here needs a
GPU, and nothing here runs the engine."""
import numpy as np
import pytest
import torch
from torch import nn

import spectral_norm_ref as S

SHAPES = [(5, 7), (1, 6), (4, 1)]


def _torch_layer(out, in_, seed):
    torch.manual_seed(seed)
    lin = nn.utils.spectral_norm(nn.Linear(in_, out).double(), n_power_iterations=1)
    return lin


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_is_torch_spectral_norm(shape):
    """weight_u, weight_v, the output and weight_orig.grad after one train-mode call; then the eval form."""
    out, in_ = shape
    lin = _torch_layer(out, in_, 3)
    W = lin.weight_orig.detach().numpy().copy()
    u0, v0 = lin.weight_u.numpy().copy(), lin.weight_v.numpy().copy()
    x = torch.randn(9, in_, dtype=torch.float64)
    c = torch.randn(9, out, dtype=torch.float64)          # dL/dy of L = sum(c * y)
    lin.train()
    y = lin(x)
    (c * y).sum().backward()
    u1, v1, sigma, weff = S.iterate(W, u0, v0)
    assert np.allclose(lin.weight_u.numpy(), u1, rtol=0, atol=1e-14) and np.allclose(lin.weight_v.numpy(), v1, rtol=0, atol=1e-14)
    b = lin.bias.detach().numpy()
    assert np.allclose(y.detach().numpy(), x.numpy() @ weff.T + b, rtol=0, atol=1e-13)
    G = c.numpy().T @ x.numpy()                           # dL/dW_eff
    dW, _ = S.project(G, weff, u1, v1, sigma)
    scale = np.abs(lin.weight_orig.grad.numpy()).max()
    assert np.abs(lin.weight_orig.grad.numpy() - dW).max() <= 1e-13 * max(scale, 1.0)
    # eval mode: nothing iterated, sigma from the stored vectors -- and equal to the train-mode output of the same call
    lin.eval()
    ye = lin(x).detach().numpy()
    assert np.allclose(lin.weight_u.numpy(), u1, rtol=0, atol=1e-14) and np.allclose(lin.weight_v.numpy(), v1, rtol=0, atol=1e-14)
    s_eval, weff_eval = S.eval_form(W, lin.weight_u.numpy(), lin.weight_v.numpy())
    assert np.allclose(ye, x.numpy() @ weff_eval.T + b, rtol=0, atol=1e-13)
    assert np.allclose(ye, y.detach().numpy(), rtol=0, atol=1e-13) and abs(s_eval - sigma) <= 1e-14 * abs(sigma)


def _case(shape, seed=11):
    rs = np.random.RandomState(seed)
    out, in_ = shape
    W = (rs.randn(out, in_) * 0.3).astype(np.float32)
    u = S.unit(rs.randn(out)).astype(np.float32)
    v = S.unit(rs.randn(in_)).astype(np.float32)
    G = rs.randn(out, in_).astype(np.float32)
    return W, u, v, G


def _judge(W, u, v, G, mistake):
    """Every comparator of the GPU test over one emulated layer: iterate, eval after it, project."""
    u1, v1, sigma, weff = S.emulate_iterate(W, u, v, mistake)
    S.check_iterate(W, u, u1, v1, sigma)
    S.check_weff(W, sigma, weff)
    ue, ve, se, _ = S.emulate_eval(W, u1, v1, mistake)
    assert np.array_equal(ue, u1) and np.array_equal(ve, v1), "the eval form moved u or v"
    S.check_eval(W, u1, v1, se)
    s, dW = S.emulate_project(G, W, weff, u1, v1, sigma, mistake)
    S.check_project(G, weff, u1, v1, sigma, s, dW)
    # ... and the float32 result is the float64 projection to float32 accuracy
    ref, _ = S.project(G, weff.astype(np.float64), u1.astype(np.float64), v1.astype(np.float64), float(sigma))
    assert np.abs(dW - ref).max() <= 8 * S.F32 * (np.abs(G).max() + abs(s)) / abs(float(sigma))


@pytest.mark.parametrize("shape", SHAPES + [(32, 91)], ids=lambda s: "%dx%d" % s)
def test_comparators_accept_the_emulated_kernels(shape):
    _judge(*_case(shape), mistake=None)


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_comparators_reject_seeded_mistakes(mistake):
    with pytest.raises(AssertionError):
        _judge(*_case((32, 91)), mistake=mistake)


def test_sqnorm_comparator():
    rs = np.random.RandomState(2)
    g = rs.randn(5000).astype(np.float32)
    parts = [float((g[i:i + 700].astype(np.float64) ** 2).sum()) for i in range(0, 5000, 700)]
    S.check_sqnorm(g, parts)
    with pytest.raises(AssertionError):
        S.check_sqnorm(g, parts[:-1])


def test_flat_layout_is_misaligned_on_purpose():
    tab, n = S.flat_layout()
    assert n == 3 + sum(o * i + o for o, i in S.HOOK_LAYERS)
    assert [off % 4 for (off, _, _, _, _) in tab] == [3, 3, 3, 3, 0, 2]      # weight ranges that do not start on 16 bytes


def test_step_reference_without_drift_is_plain_autograd():
    """SpectralOracleMLP in eval mode twice in a row builds the same W_eff and leaves u, v alone; in training mode it advances them."""
    import gantts_oracle as O
    m = O.OracleMLP(in_dim=6, out_dim=1, num_hidden=2, hidden_dim=5, dropout=0.0, last_sigmoid=False, seed=1)
    spec = dict(in_dim=6, out_dim=1, num_hidden=2, hidden_dim=5)
    u0, v0 = S.initial_uv(spec)
    w = S.SpectralOracleMLP(m, u0, v0)
    w.training = False
    w.begin_pass()
    a = [t.detach().numpy().copy() for t in w.weff]
    w.begin_pass()
    assert all(np.array_equal(x, y.detach().numpy()) for x, y in zip(a, w.weff))
    assert all(np.array_equal(x.numpy(), y) for x, y in zip(w.u, u0))
    w.training = True
    w.begin_pass()
    assert not np.array_equal(w.u[0].numpy(), u0[0])
    for q, We in enumerate(w.weff):      # one iteration of the restatement, float32 against float64
        u1, v1, sigma, ref = S.iterate(m.params[2 * q].detach().numpy(), u0[q], v0[q])
        assert np.allclose(We.detach().numpy(), ref, rtol=1e-5, atol=1e-6)
