"""The CPU statement of GT_OPT_SRU_D_BF16's arithmetic: a float32 SRURNN whose product U = xin . W -- and the two products of its
backward pass -- take both operands rounded to bfloat16 and accumulate in float32.  Everything else (the recurrence, hidden2out, every
reduction, the optimizer) is the float32 oracle's, untouched: the class below subclasses gantts_oracle.OracleSRURNN and restates its
forward with one line changed.  The engine's bf16 path is judged against THIS model (tests/test_gpu_sru_d_bf16.py), not against a flat
tolerance around the float32 oracle."""
import numpy as np
import torch
import torch.nn.functional as F

import cases as C
import gantts_oracle as O
import oracle_runner


def r(t):
    """round to nearest bfloat16, kept as float32"""
    return t.bfloat16().float()


class Bf16Product(torch.autograd.Function):
    """a @ b with bf16 operands and float32 accumulation, forward and backward.  `seen`: while it is a list, every backward call
    appends the gradient it received (tests look at it; None = off)."""
    seen = None

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return r(a) @ r(b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        if Bf16Product.seen is not None:
            Bf16Product.seen.append(g.detach().clone())
        gr = r(g)
        dA = gr @ r(b).t()
        dB = r(a).reshape(-1, a.shape[-1]).t() @ gr.reshape(-1, g.shape[-1])
        return dA, dB


class Bf16OperandSRURNN(O.OracleSRURNN):
    """OracleSRURNN.forward with U from Bf16Product: xin is rounded AFTER the input-dropout multiply, hidden2out stays float32."""

    def forward(self, x, lengths=None, drop=None):
        B, T, _ = x.shape
        H, ncols = self.H, self.H * self.dirs
        inp = x
        for l in range(self.L):
            W, bias = self.params[2 * l], self.params[2 * l + 1]
            k = self.ks[l]
            xin = inp
            if self.training and self.rnn_p > 0:
                drop = drop or O._DropoutSource()
                xin = inp * (drop.next(inp[:, 0], self.rnn_p) / (1.0 - self.rnn_p)).unsqueeze(1)
            U = Bf16Product.apply(xin, W).view(B, T, ncols, k)
            Ut = U.unbind(1)
            inp_t = inp.unbind(1) if k == 3 else None
            mask_h = None
            if self.training and self.p > 0 and l + 1 < self.L:
                drop = drop or O._DropoutSource()
                mask_h = drop.next(inp.new_zeros(B, ncols), self.p) / (1.0 - self.p)
            bf, br = bias[:ncols], bias[ncols:]
            outs = []
            for d in range(self.dirs):
                sl = slice(d * H, (d + 1) * H)
                c = x.new_zeros(B, H)
                seq = [None] * T
                for t in (range(T - 1, -1, -1) if d else range(T)):
                    u = Ut[t][:, sl]
                    f = torch.sigmoid(u[..., 1] + bf[sl])
                    rr = torch.sigmoid(u[..., 2] + br[sl])
                    c = (c - u[..., 0]) * f + u[..., 0]
                    val = self._g(c)
                    if mask_h is not None:
                        val = val * mask_h[:, sl]
                    xp = inp_t[t][:, sl] if k == 3 else u[..., 3]
                    seq[t] = (val - xp) * rr + xp
                outs.append(torch.stack(seq, 1))
            inp = torch.cat(outs, -1)
        out = F.linear(inp, self.params[-2], self.params[-1])
        return torch.sigmoid(out) if self.last_sigmoid else out

    __call__ = forward


def build_bf16_model(spec, seed):
    """oracle_runner.build_oracle_model for an SRURNN spec, as the bf16-operand model"""
    assert spec["kind"] == "SRURNN"
    m = Bf16OperandSRURNN(**{k: v for k, v in spec.items() if k != "kind"})
    m.load_state_dict(C.make_weights(spec, seed))
    return m


def run_bf16_model_case(case, roles="d"):
    """oracle_runner.run_oracle_case with the SRURNN of every role in `roles` ("d", "g" or "gd") built as the bf16-operand model: the
    runner's O.OracleSRURNN is pointed at a constructor that hands out the classes in the order the runner builds its models
    (generator, then discriminator), and restored afterwards."""
    sru_roles = [role for role in "gd" if case[role]["kind"] == "SRURNN"]
    assert set(roles) <= set(sru_roles), (roles, sru_roles)
    real = oracle_runner.O.OracleSRURNN
    built = []

    def construct(**kw):
        role = sru_roles[len(built)]
        built.append(role)
        return (Bf16OperandSRURNN if role in roles else real)(**kw)

    oracle_runner.O.OracleSRURNN = construct
    try:
        out = oracle_runner.run_oracle_case(case)
    finally:
        oracle_runner.O.OracleSRURNN = real
    assert built == sru_roles
    return {k: np.asarray(v) for k, v in out.items()}
