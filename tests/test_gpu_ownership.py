"""-m gpu: the engine gives back what it took.  Every device block, pinned host block and event of an engine belongs to an owning type
(gantts_amd/csrc/engine_internal.hip.h: Scratch, Pinned, Event), and gt_live_resources counts what those types hold, process-wide:
[live device blocks, their bytes, live pinned blocks, live events].  The tests read it around whole engine lives at the smallest shapes:

  * destroy returns all four slots to where they were before create, over cases that between them reach every member group of the engine and
    of its per-role workspace: the float32 and bf16 MLP stacks, both In2Out generators, an LSTM and an SRU network in either slot (the SRU
    discriminator with and without its bf16 products), the bf16 images of an LSTM and of an SRU generator (vc_in2out_rnn and
    acoustic_sru_dropout under matmul_bf16: added for l_in_b / l_dg_b / lsh and the generator's s_in_b / ssh, which none of the listed cases
    reaches), a dense copy of a pitched conditioning x (acoustic_lstm_d with pitch_x: cx_dense), the communicator, the event route of the
    early results (poll_results=0: ev_res), the deferred route with the epoch ledger, spectral normalisation and the WGAN-GP penalty, and
    three lives with one more call behind the steps, each of which must add a block: gt_model_forward under matmul_bf16 (fwd_b), one
    variance-weighted MLPG (mlpg_var_ws), gt_comm_ipc_export (the interprocess arena, the one block whose count is kept by hand);
  * binding a shallower discriminator frees the layers that go (the commit before this module leaked them: it had no counter to show it);
  * a step at a shape the engine has seen allocates nothing;
  * an engine whose creation is refused leaves nothing behind.

The engines are destroyed through StepEngine._finalizer, not by the collector, and every reading is taken behind a collection, so that an
engine another module left in a reference cycle cannot go away between two readings."""
import ctypes as C_
import gc

import numpy as np
import pytest
import torch

import cases as C
import hip_runner

pytestmark = pytest.mark.gpu


def live():
    from gantts_amd import _lib as L
    gc.collect()
    torch.cuda.synchronize()
    out = (C_.c_int64 * 4)()
    L.check(L.lib.gt_live_resources(out))
    return tuple(out)


def destroy(mg):
    """The engine anchored on the generator, now (weakref.finalize runs gt_engine_destroy once)."""
    torch.cuda.synchronize()
    fin = mg._step_engine._finalizer
    assert fin.alive
    fin()


@pytest.fixture(scope="module", autouse=True)
def warm():
    """One create / step / destroy cycle before the first reading: whatever the process creates lazily is in place."""
    _, objs = hip_runner.run_hip_case(dict(C.CASES["acoustic_mlp"], steps=1), return_objects=True)
    destroy(objs[0])


def _case(name):
    return C.CASES[name] if name in C.CASES else C.ORACLE_ONLY_CASES[name]


def _sru_d_case():
    """No golden case has an SRU discriminator: acoustic_lstm_d's generator and batch, its discriminator as a two-layer bidirectional
    SRURNN of the same input width (hidden_dim % 8 == 0: the bf16 products apply)."""
    g = _case("acoustic_sru_dropout")["g"]
    d = dict(kind="SRURNN", in_dim=C.CASES["acoustic_lstm_d"]["d"]["in_dim"], out_dim=1, num_hidden=2, hidden_dim=16, bidirectional=True,
             dropout=0.0, rnn_dropout=0.0, last_sigmoid=True, use_relu=g["use_relu"])
    return dict(C.CASES["acoustic_lstm_d"], d=d)


def _hp_with(monkeypatch, **attrs):
    real = hip_runner.make_hp

    def make_hp(case):
        hp = real(case)
        for k, v in attrs.items():
            setattr(hp, k, v)
        return hp
    monkeypatch.setattr(hip_runner, "make_hp", make_hp)


def _spectral_norm(monkeypatch, case):
    from test_gpu_spectral_norm import build_d
    real = hip_runner.build_model
    monkeypatch.setattr(hip_runner, "build_model", lambda spec, seed, *a: build_d(spec, True, seed) if spec is case["d"] else real(spec, seed, *a))
    _hp_with(monkeypatch, discriminator_spectral_norm=True)


def _split_phase_with_ledger(case):
    """The case's steps through the split-phase calls with defer=True and a configured epoch ledger, as train_loop drives them."""
    import gantts_amd.train as T
    from gantts_amd import _lib as L, optim, paramgen
    from gantts_amd.engine import HipStepBackend
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    hp = hip_runner.make_hp(case)
    T.hp = hp
    mg, md = hip_runner.build_model(case["g"], 11).eval(), hip_runner.build_model(case["d"], 22).eval()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    be = HipStepBackend(hp, mg, md, og, od)
    roles, stats, vuv_col, _ = T._acoustic_columns()
    mean, std = torch.zeros(max(stats) + 1).cuda(), torch.ones(max(stats) + 1).cuda()
    be.engine.ledger_configure(L.LEDGER_ACOUSTIC, roles, stats, vuv_col, mean, std, T._LOGDB_CONST)
    be.engine.ledger_reset()
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    sl = torch.from_numpy(np.ascontiguousarray(lengths)).cuda()
    batch = dict(x=x, y=y, y_static=get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features),
                 mask=sequence_mask(sl, max_len=case["T"]).unsqueeze(-1), R=paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"]),
                 lengths=list(lengths))
    w = case["adv_w"], case["mse_w"], case["mge_w"]
    for _ in range(case["steps"]):
        be.zero_grad()
        _, y_hat_static = be.apply_generator(batch)
        be.update_discriminator_begin(batch, "train")
        assert be.update_discriminator_end(batch, "train", defer=True) is None
        be.update_generator_begin(batch, *w, "train")
        assert be.update_generator_end(batch, *w, "train", defer=True) is None
        be.engine.ledger_add(L.LEDGER_HAS_D | L.LEDGER_HAS_G | L.LEDGER_HAS_DIST, batch["y_static"], y_hat_static, sl)
        assert all(np.isfinite(be.update_discriminator_result())) and all(np.isfinite(be.update_generator_result()))
    assert be.engine.ledger_read()["g_updates"] == case["steps"]
    return mg


# ... and one more call behind the case's steps, for the three groups no step reaches.  Each returns whether its group's block must exist now.
def _then_bf16_forward(eng, mg, case, monkeypatch):      # gt_model_forward's bf16 input image (fwd_b)
    x = torch.from_numpy(C.make_batch(case)[0]).cuda()
    assert torch.isfinite(eng.model_forward(mg, x)).all()
    return True


def _then_mlpg_var(eng, mg, case, monkeypatch):      # the variance-weighted MLPG's scratch (mlpg_var_ws)
    y = torch.from_numpy(C.make_batch(case)[1]).cuda()
    assert torch.isfinite(eng.mlpg_var(y, torch.ones(y.size(-1)).cuda())).all()
    return True


def _then_ipc_export(eng, mg, case, monkeypatch):      # the interprocess arena: the one block counted by hand (eng_ipc.hip)
    from gantts_amd._lib import GanttsHipError
    monkeypatch.setenv("GT_IPC_ALLOW_COARSE", "1")      # where the runtime has no fine-grained memory the arena is a plain allocation
    try:
        eng.comm_ipc_export()
    except GanttsHipError as err:      # no interprocess handles on this platform: the arena was allocated and freed again on that path
        assert "hipIpcGetMemHandle" in str(err), err
        return False
    return True


LIVES = {
    "acoustic_mlp": ("acoustic_mlp", {}),
    "acoustic_mlp_dropout": ("acoustic_mlp_dropout", {}),
    "vc_in2out": ("vc_in2out", {}),
    "vc_in2out_rnn": ("vc_in2out_rnn", {}),
    "acoustic_lstm_d": ("acoustic_lstm_d", {}),
    "acoustic_sru_dropout": ("acoustic_sru_dropout", {}),
    "acoustic_mlp-bf16": ("acoustic_mlp", dict(engine_options={"matmul_bf16": 1})),
    "acoustic_mlp-comm": ("acoustic_mlp", dict(comm_world_1=True)),
    "acoustic_mlp-event_route": ("acoustic_mlp", dict(engine_options={"poll_results": 0})),
    "acoustic_mlp-deferred_ledger": ("acoustic_mlp", "split"),
    "sru_d": ("sru_d", {}),
    "sru_d-bf16": ("sru_d", dict(engine_options={"sru_d_bf16": 1})),
    "acoustic_mlp-spectral_norm": ("acoustic_mlp", "sn"),
    "acoustic_mlp-wgan_gp": ("acoustic_mlp", "gp"),
    "vc_in2out_rnn-bf16": ("vc_in2out_rnn", dict(engine_options={"matmul_bf16": 1})),
    "acoustic_sru_dropout-bf16": ("acoustic_sru_dropout", dict(engine_options={"matmul_bf16": 1})),
    "acoustic_lstm_d-pitch_x": ("acoustic_lstm_d", dict(pitch_x=True)),
    "acoustic_mlp-bf16-forward": ("acoustic_mlp", dict(engine_options={"matmul_bf16": 1}, then=_then_bf16_forward)),
    "acoustic_mlp-mlpg_var": ("acoustic_mlp", dict(then=_then_mlpg_var)),
    "acoustic_mlp-ipc_arena": ("acoustic_mlp", dict(then=_then_ipc_export)),
}


@pytest.mark.parametrize("name", list(LIVES))
def test_destroy_gives_back_what_create_took(name, monkeypatch):
    case_name, how = LIVES[name]
    case = _sru_d_case() if case_name == "sru_d" else _case(case_name)
    before = live()
    if how == "split":
        mg = _split_phase_with_ledger(case)
    else:
        if how == "sn":
            _spectral_norm(monkeypatch, case)
        elif how == "gp":
            _hp_with(monkeypatch, discriminator_grad_penalty="wgan-gp")
        kw = dict(how) if isinstance(how, dict) else {}
        then = kw.pop("then", None)
        out, (mg, md, og, od) = hip_runner.run_hip_case(case, return_objects=True, **kw)
        assert all(np.isfinite(v).all() for v in out.values())
        if then is not None:
            stepped = live()
            grows = then(mg._step_engine, mg, case, monkeypatch)
            assert (live()[0] > stepped[0] and live()[1] > stepped[1]) if grows else (live() == stepped), (name, stepped, live())
        if how == "sn":
            assert mg._step_engine._sn_on
        if how == "gp":
            assert mg._step_engine.grad_penalty == "wgan-gp"
    during = live()
    print("%s: before %s, alive %s" % (name, before, during))
    assert during[0] > before[0] and during[1] > before[1] and during[2] > before[2]      # (the counters see this engine at all)
    destroy(mg)
    assert live() == before


class _Rebind(object):
    """One engine on acoustic_lstm_d's generator at B = 2, T = 8; D steps with whichever discriminator is handed in."""

    def __init__(self):
        import gantts_amd.train as T
        from gantts_amd import optim, paramgen
        from gantts_amd.multistream import get_static_features
        from gantts_amd.seqloss import sequence_mask
        self.case = case = dict(C.CASES["acoustic_lstm_d"], B=2, T=8)
        self.T, self.optim = T, optim
        self.hp = T.hp = hip_runner.make_hp(case)
        self.mg = hip_runner.build_model(case["g"], 11).eval()
        self.og = optim.Adagrad(self.mg.parameters(), **case["opt_g"][1])
        x_np, y_np, lengths = C.make_batch(case)
        self.x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        self.y_static = get_static_features(y, len(self.hp.windows), self.hp.stream_sizes, self.hp.has_dynamic_features)
        self.lengths = list(lengths)
        self.mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)
        self.R = paramgen.unit_variance_mlpg_matrix_cuda(self.hp.windows, case["T"])

    def d_step(self, kind, num_hidden):
        spec = dict(kind=kind, in_dim=self.case["d"]["in_dim"], out_dim=1, num_hidden=num_hidden, hidden_dim=16, dropout=0.0, last_sigmoid=True)
        if kind == "LSTMRNN":
            spec["bidirectional"] = True
        md = hip_runner.build_model(spec, 22).eval()
        od = self.optim.Adagrad(md.parameters(), **self.case["opt_d"][1])
        self.T.hp = self.hp
        self.og.zero_grad()
        od.zero_grad()
        _, y_hat_static = self.T.apply_generator(self.mg, self.x, self.R, self.lengths)
        res = self.T.update_discriminator(md, od, self.x, self.y_static, y_hat_static, self.lengths, self.mask, "train")
        assert all(np.isfinite(res))
        return live()


@pytest.mark.parametrize("kind", ["MLP", "LSTMRNN"])
def test_a_shallower_rebind_frees(kind):
    before = live()
    run = _Rebind()
    deep = run.d_step(kind, 3)
    shallow = run.d_step(kind, 1)
    print("%s: before %s, 3 layers %s, 1 layer %s" % (kind, before, deep, shallow))
    assert shallow[0] < deep[0] and shallow[1] < deep[1]
    destroy(run.mg)
    assert live() == before


def test_the_steady_state_allocates_nothing(monkeypatch):
    import gantts_amd.train as T
    readings, apply_generator = [], T.apply_generator

    def reading_first(*a, **kw):      # every step opens with apply_generator: a reading in front of it is one behind the step before
        readings.append(live())
        return apply_generator(*a, **kw)
    monkeypatch.setattr(T, "apply_generator", reading_first)
    case = C.CASES["acoustic_mlp"]
    assert case["steps"] == 3
    _, objs = hip_runner.run_hip_case(case, return_objects=True)
    readings.append(live())      # [before step 1, after step 1, after step 2, after step 3]
    print("after each step: %s" % (readings[1:],))
    assert len(readings) == 4 and readings[2] == readings[3]
    destroy(objs[0])


def test_a_failing_create_leaks_nothing():
    """The refusal of mask_nth_mgc_for_adv_loss comes before gt_engine_create's first device allocation: at that point only the host object
    exists, so this shows that the refused call leaves the counters alone, not that the error paths behind the allocations free (those are
    hipMalloc / hipHostMalloc failures, which no test provokes; they return under the same unique_ptr)."""
    from gantts_amd import _lib as L
    from gantts_amd.engine import stream_config_from_hp
    hp = hip_runner.make_hp(C.CASES["acoustic_mlp"])
    hp.mask_nth_mgc_for_adv_loss = 60      # the adversarial stream has 60 static columns: nothing would be left
    before = live()
    h = C_.c_void_p()
    rc = L.lib.gt_engine_create(C_.byref(stream_config_from_hp(hp)), C_.byref(h))
    assert rc == L.GT_ERR_INVALID and b"mask_nth_mgc_for_adv_loss" in L.lib.gt_last_error() and not h.value
    assert live() == before
