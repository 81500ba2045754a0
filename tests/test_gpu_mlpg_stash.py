"""The stashed generator pass owns its MLPG band (gt_engine::g_band, gantts_amd/csrc/eng_mlpg.hip): update_generator transposes through the
band apply_generator went through, whatever the band cache served, recycled or dropped in between.

  interleaved   mlpg_forward and mlpg_backward at another T between apply_generator and update_discriminator: the step's bits do not move
  eviction      more first sights than the cache holds entries in between: the pass's band is never the one recycled
  invalidation  invalidate_mlpg_cache, or another window set under an MLPGBand, in between: the pass can no longer be back-propagated
                (the refusals update_generator and flush_generator_grads already had), and the next full step gives the undisturbed bits

Every run is the STEP networks of test_gpu_mlpg_band.py (no dropout) from the same seeded state, and the G step in its split-phase form, so
that G's gradients are read before the update; "the same bits" is the losses, those gradients and every parameter."""
import os
import re

import numpy as np
import pytest
import torch

import cases as C
import test_gpu_mlpg_band as S
from gantts_amd import paramgen

DENSE, BAND = paramgen.unit_variance_mlpg_matrix_cuda, paramgen.unit_variance_mlpg_band
KINDS = [pytest.param(DENSE, id="dense"), pytest.param(BAND, id="band")]


class Step:
    """models, optimizers and one seeded batch of B sequences of T frames; run() is one G + D step on them"""

    def __init__(self, make_R, B, Tn, lengths):
        from gantts_amd import optim
        from gantts_amd.engine import engine_for
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        from hip_runner import build_model
        self.hp = S._step_hp()
        self.mg, self.md = build_model(S.STEP["g"], 11), build_model(S.STEP["d"], 22)
        self.mg.train(), self.md.train()
        self.og = optim.Adagrad(self.mg.parameters(), lr=0.01, weight_decay=1e-7)
        self.od = optim.Adagrad(self.md.parameters(), lr=0.01, weight_decay=1e-7)
        rs = np.random.RandomState(5)
        x = (0.01 + 0.98 * rs.rand(B, Tn, S.STEP["din"])).astype(np.float32)
        y = rs.randn(B, Tn, 16).astype(np.float32)
        for b, n in enumerate(lengths):
            x[b, n:] = 0
            y[b, n:] = 0
        self.x, self.y, self.lengths = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), list(lengths)
        self.R = make_R(self.hp.windows, Tn)
        self.y_static = get_static_features(self.y, 3, self.hp.stream_sizes, self.hp.has_dynamic_features)
        self.mask = sequence_mask(torch.tensor(self.lengths).cuda(), max_len=Tn).unsqueeze(-1)
        self.eng = engine_for(self.hp, self.mg)

    def apply(self):
        self.og.zero_grad()
        self.od.zero_grad()
        self.out = self.eng.apply_generator(self.mg, self.x, self.R, self.lengths)

    def g_args(self):
        return (self.mg, self.md, self.og, self.x, self.y, self.out[0], self.y_static, self.out[1], 1.0, self.mask, "train", 0.5, 1.0)

    def run(self, between=None):
        """apply_generator, `between(self)`, update_discriminator, update_generator -> everything the step produced"""
        e = self.eng
        self.apply()
        res = {"y_hat_static": self.out[1].cpu().numpy()}
        if between:
            between(self)
        res["d"] = np.array(e.update_discriminator(self.md, self.od, self.x, self.y_static, self.out[1], self.mask, "train", lengths=self.lengths), np.float64)
        e.update_generator_begin(*self.g_args())
        res["g_grads"] = self.mg.flat_grads().cpu().numpy().copy()
        res["g"] = np.array(e.update_generator_end(self.og, 1.0, 0.5, 1.0, "train"), np.float64)
        torch.cuda.synchronize()
        for t, m in (("G.", self.mg), ("D.", self.md)):
            res.update({t + k: v.cpu().numpy() for k, v in m.state_dict().items()})
        return res


def same_bits(got, want):
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
    assert np.isfinite(want["g"]).all() and np.isfinite(want["d"]).all() and np.abs(want["g_grads"]).max() > 0


def test_a_longer_matrix_differs_in_the_rows_it_shares_with_a_shorter_one():
    """What gives the interleaved test its power: for hp.windows, rows t < 24 of the T = 40 matrix are not the T = 24 matrix -- the last
    rows of the shorter one are edge rows -- so a transpose through the interloper's band cannot give the undisturbed gradients."""
    w = S._step_hp().windows
    R24 = np.asarray(paramgen.unit_variance_mlpg_matrix(w, 24), np.float64).reshape(24, 3, 24)
    R40 = np.asarray(paramgen.unit_variance_mlpg_matrix(w, 40), np.float64).reshape(40, 3, 40)
    assert np.abs(R40[:24, :, :24] - R24).max() > 1e-3 * np.abs(R24).max()


@pytest.mark.gpu
@pytest.mark.parametrize("make_R", KINDS)
def test_an_mlpg_call_at_another_length_between_the_passes_does_not_move_the_step(make_R):
    B, Tn, T2 = 2, 24, 40
    want = Step(make_R, B, Tn, [24, 17]).run()
    rs = np.random.RandomState(6)
    y2 = torch.from_numpy(rs.randn(B, T2, 16).astype(np.float32)).cuda()
    g2 = torch.from_numpy(rs.randn(B, T2, 6).astype(np.float32)).cuda()

    def interloper(st):
        R2 = make_R(st.hp.windows, T2)
        assert st.eng.static_dim == 6
        a, b = st.eng.mlpg_forward(y2, R2), st.eng.mlpg_backward(g2, R2, 16)
        torch.cuda.synchronize()
        assert a.shape == (B, T2, 6) and b.shape == (B, T2, 16) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())

    same_bits(Step(make_R, B, Tn, [24, 17]).run(interloper), want)


@pytest.mark.gpu
def test_the_band_of_the_stashed_pass_is_never_the_one_recycled():
    B, Tn = 2, 4      # T and nW of test_gpu_mlpg.py::test_band_cache_recycles_the_least_recently_used_entry
    src_text = open(os.path.join(S.M.ROOT, "gantts_amd", "csrc", "engine_internal.hip.h")).read()
    n = int(re.search(r"MAX_ENTRIES = (\d+)", src_text).group(1)) + 1
    want = Step(DENSE, B, Tn, [4, 3]).run()
    base = np.array(paramgen.unit_variance_mlpg_matrix(C.WINDOWS, Tn))
    many = torch.from_numpy((base[None] * (1.0 + np.arange(1, n + 1) / 1024.0).astype(np.float32)[:, None, None]).astype(np.float32)).cuda()
    y2 = torch.from_numpy(np.random.RandomState(6).randn(1, Tn, 16).astype(np.float32)).cuda()

    def crowd(st):
        for i in range(n):      # every one a first sight; the pass's entry is the least recently used throughout
            st.eng.mlpg_forward(y2, many[i])
        torch.cuda.synchronize()

    st = Step(DENSE, B, Tn, [4, 3])
    try:
        same_bits(st.run(crowd), want)
    finally:
        st.eng.invalidate_mlpg_cache()


def _drop_everything(st):
    st.eng.invalidate_mlpg_cache()


def _register_other_windows(st):
    st.eng.mlpg_band(paramgen.MLPGBand(S.M.WINDOW_SETS["asym"], st.x.size(1)))


@pytest.mark.gpu
@pytest.mark.parametrize("make_R,drop", [pytest.param(DENSE, _drop_everything, id="dense-invalidate"), pytest.param(BAND, _drop_everything, id="band-invalidate"),
                                         pytest.param(BAND, _register_other_windows, id="band-other_windows")])
def test_a_pass_whose_band_was_dropped_is_refused_and_the_next_step_is_undisturbed(make_R, drop):
    B, Tn = 2, 24
    want = Step(make_R, B, Tn, [24, 17]).run()
    st = Step(make_R, B, Tn, [24, 17])
    st.apply()
    drop(st)
    with pytest.raises(RuntimeError, match="needs the y_hat / y_hat_static returned by the last apply_generator"):
        st.eng.update_generator(*st.g_args())
    with pytest.raises(RuntimeError, match="no generator pass to back-propagate"):
        st.eng.flush_generator_grads()
    same_bits(st.run(), want)
