"""-m gpu: GT_OPT_SRU_D_BF16 -- an SRURNN in the discriminator slot with its three products per layer on bf16 images.

The reference is not a flat tolerance around the float32 oracle but the CPU model of exactly that arithmetic (tests/bf16_sru_model.py:
float32 SRU, both operands of U = xin . W and of the two backward products rounded to bf16, float32 accumulation).  With F the float32
oracle, M that model and E the engine, d(a, b) = rms(a - b) / rms(F) per tensor:

  (a) every parameter / optimizer-state tensor of both networks:  d(E, F) <= 2 d(M, F) + RTOL  (RTOL: the suite's float32 tolerance;
      the factor 2 covers the engine's different but equally valid rounding points);
  (b) every discriminator tensor with d(M, F) >= 10 RTOL:  d(E, M) < d(E, F) -- bf16 arithmetic, as modelled, is what ran;
  (c) losses: |E - F| <= 2 |M - F| + RTOL |F|;   (d) counts against M's within 0.02 max(1, B T);   (e) y_hat at the float32 rule.

The cases are the smallest shapes that reach each path of the bf16 stack (folded scans / cast passes, dU as images / cast, k = 4 and
k = 3, the column slice of the layer-0 shadow, dropout per row group).  `k3_input` is this file's own addition: `fold_uni_k3` has
k = 4 in layer 0 (in_dim 58 != 64 columns; its k = 3 layer is layer 1), so a 56-column adversarial input (mask_nth_mgc = 4) into a
56-unit layer covers k = 3 in layer 0: the float32 [x | adv] rows kept beside the images, the highway gradient into the leak."""
import copy

import numpy as np
import pytest
import torch

import cases as C
from test_gpu_sru_discriminator import ADAM, ADG, GMLP, SRUD_CASES, _case, oracle_of, run_srud_case

pytestmark = pytest.mark.gpu

ON = {"sru_d_bf16": 1}
_DROP = dict(dropout=0.3, rnn_dropout=0.25)
BF16_CASES = {
    "fold_bi_k4_cond": _case(2, 16, 20, True, 2, False, ADAM, GMLP,
                             dict(in_dim=78, num_hidden=2, hidden_dim=64, bidirectional=True, use_relu=1)),
    "fold_uni_k3": _case(3, 24, 20, False, 2, False, ADG, GMLP,
                         dict(in_dim=58, num_hidden=2, hidden_dim=64, bidirectional=False, use_relu=0)),
    "nofold_h8_ragged": _case(3, 19, 20, True, 2, True, ADAM, GMLP,
                              dict(in_dim=78, num_hidden=3, hidden_dim=24, bidirectional=True, use_relu=1, **_DROP)),
    "fold_dropout": _case(4, 16, 20, True, 2, True, ADG, GMLP,
                          dict(in_dim=78, num_hidden=3, hidden_dim=64, bidirectional=True, use_relu=1, **_DROP)),
    "k3_input": dict(_case(3, 16, 20, False, 2, True, ADAM, GMLP,
                           dict(in_dim=56, num_hidden=2, hidden_dim=56, bidirectional=False, use_relu=0, **_DROP)), mask_nth_mgc=4),
}
# test 3 / 6: an SRU generator beside the discriminator of fold_dropout (its in_dim follows the 30 conditioning columns: 30 + 58)
GSRU = dict(kind="SRURNN", in_dim=30, out_dim=187, num_hidden=2, hidden_dim=64, bidirectional=True, dropout=0.2, last_sigmoid=False,
            use_relu=1, rnn_dropout=0.2)
PAIR = _case(2, 16, 30, True, 2, True, ADG, GSRU, dict(BF16_CASES["fold_dropout"]["d"], in_dim=88))

_MODEL = {}


def model_of(name, case):
    """the bf16-operand model's run of the case, computed once and shared, never modified"""
    if name not in _MODEL:
        from bf16_sru_model import run_bf16_model_case
        ref = run_bf16_model_case(case, roles="d")
        for v in ref.values():
            v.setflags(write=False)
        _MODEL[name] = ref
    return _MODEL[name]


def _rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt((a * a).mean())) if a.size else 0.0


def _d(a, b, f):
    return _rms(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) / max(_rms(f), 1e-30)


def _track(tag, E, M, F, discriminator):
    """rules (a) and (b) on one tensor; returns whether (b) applied"""
    from test_gpu_parity import RTOL
    ef, mf, em = _d(E, F, F), _d(M, F, F), _d(E, M, F)
    applies = discriminator and mf >= 10 * RTOL
    print("%-62s d(E,F) %.3e  d(M,F) %.3e  d(E,M) %.3e  (a) %.3f%s" % (tag, ef, mf, em, ef / (2 * mf + RTOL), "  (b) %.3f" % (em / ef) if applies else ""))
    assert ef <= 2 * mf + RTOL, (tag, ef, mf)
    if applies:
        assert em < ef, (tag, em, ef)
    return applies


# ---------------------------------------------------------------------------------------------
# 1. whole steps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BF16_CASES))
def test_sru_d_bf16_steps_track_the_bf16_operand_model(name):
    from test_gpu_parity import RTOL, _close
    case = BF16_CASES[name]
    F, M = oracle_of("bf16/" + name, case), model_of(name, case)
    E = run_srud_case(case, engine_options=ON)
    n_b = 0
    for k in sorted(F):
        if k.split(".")[0] in ("D", "G"):
            assert k in E and k in M, k
            n_b += _track("%s %s" % (name, k), E[k], M[k], F[k], k.startswith("D."))
    assert n_b >= 1, "%s: no discriminator tensor on which the bf16 model is 10 RTOL away from the float32 oracle" % name
    for st in range(case["steps"]):
        for k, nl in (("d_scalars_%d" % st, 3), ("g_scalars_%d" % st, 4)):
            e, m, f = (np.asarray(v[k], dtype=np.float64) for v in (E, M, F))
            print("%s %s engine %s model %s float32 %s" % (name, k, e, m, f))
            assert (np.abs(e[:nl] - f[:nl]) <= 2 * np.abs(m[:nl] - f[:nl]) + RTOL * np.abs(f[:nl])).all(), (k, e, m, f)      # (c)
            if k.startswith("d_"):
                assert (np.abs(e[3:] - m[3:]) <= 0.02 * max(1.0, float(case["B"] * case["T"]))).all(), (k, e, m)            # (d)
    for k in ("y_hat", "y_hat_static"):      # (e): the generator is float32
        _close(E[k], F[k], msg="%s %s" % (name, k))


# ---------------------------------------------------------------------------------------------
# 2. launch census
# ---------------------------------------------------------------------------------------------
def _d_only_float32_launches(case, options):
    """One D step that keeps no leak (y_hat_static handed over as a plain tensor): launches of the float32 product kernels and the
    float32 pair launches (gt_gemm_path_counts slots 0 .. 578) issued by update_discriminator."""
    import ctypes as Ct
    import gantts_amd.train as T
    from gantts_amd import _lib as L
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    hp = make_hp(case)
    T.hp = hp
    mg, md = build_model(case["g"], 11).eval(), build_model(case["d"], 22).eval()
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = engine_for(hp, mg)
    for k, v in options.items():
        eng.set_option(k, v)
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"])
    y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)
    _, y_hat_static = T.apply_generator(mg, x, R, list(lengths))
    plain = y_hat_static.detach().clone()
    torch.cuda.synchronize()
    counts = (Ct.c_int64 * L.GEMM_PATH_SLOTS)()
    L.check(L.lib.gt_gemm_path_counts(None, 1))
    od.zero_grad()
    res = eng.update_discriminator(md, od, x, y_static, plain, mask, "train", lengths=list(lengths))
    torch.cuda.synchronize()
    L.check(L.lib.gt_gemm_path_counts(counts, 0))
    assert np.isfinite(np.asarray(res, dtype=np.float64)).all()
    return int(sum(counts[:579]))


def test_sru_d_bf16_issues_no_float32_product():
    """Option off: the D step's products are float32 launches.  On: none is left (hidden2out and its gradient live in the head kernel)."""
    case = BF16_CASES["fold_bi_k4_cond"]
    off = _d_only_float32_launches(case, {"sru_d_bf16": 0})
    on = _d_only_float32_launches(case, ON)
    print("float32 product launches of one D step: option off %d, on %d" % (off, on))
    assert off > 0
    assert on == 0


# ---------------------------------------------------------------------------------------------
# 3. the generator's stash
# ---------------------------------------------------------------------------------------------
def _run_pair(case, options, detached):
    """run_srud_case's loop; detached: update_discriminator gets y_hat_static.clone() (no leak is kept) -- with adv_w = 0 the
    discriminator then has no legitimate influence on the generator."""
    import gantts_amd.train as T
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp
    hp = make_hp(case)
    T.hp = hp
    mg, md = build_model(case["g"], 11).train(), build_model(case["d"], 22).train()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = engine_for(hp, mg)
    for k, v in options.items():
        eng.set_option(k, v)
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, case["T"])
    mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=case["T"]).unsqueeze(-1)
    y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
    cl = list(lengths)
    out = {}
    for step in range(case["steps"]):
        gm, dm = C.make_dropout_masks(case, step)
        third = len(dm) // 3
        mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
        for p in range(3):
            md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * third:(p + 1) * third]])
        og.zero_grad()
        od.zero_grad()
        y_hat, y_hat_static = T.apply_generator(mg, x, R, cl)
        if step == 0:
            out["y_hat"], out["y_hat_static"] = y_hat.cpu().numpy(), y_hat_static.cpu().numpy()
        yhs_d = y_hat_static.clone() if detached else y_hat_static
        # (on the generator's engine by name: train.update_discriminator finds the engine through the tensor apply_generator returned,
        #  and a clone does not carry it)
        out["d_scalars_%d" % step] = np.array(eng.update_discriminator(md, od, x, y_static, yhs_d, mask, "train", lengths=cl), dtype=np.float64)
        out["g_scalars_%d" % step] = np.array(T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cl, mask, "train",
                                                                 mse_w=case["mse_w"], mge_w=case["mge_w"]), dtype=np.float64)
    torch.cuda.synchronize()
    for tag, opt, model in (("G", og, mg), ("D", od, md)):
        names = list(model.state_dict().keys())
        for k, v in model.state_dict().items():
            out["%s.%s" % (tag, k)] = v.cpu().numpy()
        for i, st in opt.state_dict()["state"].items():
            for key in ("sum", "exp_avg", "exp_avg_sq"):
                if key in st:
                    out["%s.opt.%s.%s" % (tag, key, names[i])] = st[key].cpu().numpy()
    return out


def test_sru_d_bf16_leaves_the_generators_stash_alone():
    """An SRU generator on its own bf16 path (matmul_bf16 = 1) stashes images and weight shadows that its backward pass reads AFTER
    both discriminator passes.  With the leak cut (a clone goes to the D step) and adv_w = 0 the discriminator cannot legitimately move
    the generator: its scalars, parameters and optimizer state are bit-identical with the discriminator's bf16 path off and on --
    unless the discriminator wrote into an image or a shadow of the generator's."""
    case = dict(copy.deepcopy(PAIR), steps=1, adv_w=0.0)
    off = _run_pair(case, {"matmul_bf16": 1, "sru_d_bf16": 0}, detached=True)
    on = _run_pair(case, {"matmul_bf16": 1, "sru_d_bf16": 1}, detached=True)
    assert set(off) == set(on)
    for k in sorted(off):
        if k.startswith("G.") or k.startswith("g_scalars"):
            assert np.array_equal(off[k], on[k]), k
    # (and the option did change the discriminator: the comparison above is not one run against itself)
    assert any(not np.array_equal(off[k], on[k]) for k in off if k.startswith("D."))


# ---------------------------------------------------------------------------------------------
# 4. width fallback
# ---------------------------------------------------------------------------------------------
def test_sru_d_bf16_keeps_float32_for_a_width_that_is_no_multiple_of_8():
    """hidden_dim 12: the discriminator silently keeps the float32 path -- every output bit-identical to the option off."""
    case = SRUD_CASES["srud_bi_dropout"]
    off = run_srud_case(case)
    on = run_srud_case(case, engine_options=ON)
    assert set(off) == set(on)
    for k in sorted(off):
        assert np.array_equal(off[k], on[k]), k


# ---------------------------------------------------------------------------------------------
# 5. forward alone
# ---------------------------------------------------------------------------------------------
def test_sru_d_bf16_model_forward_tracks_the_bf16_operand_model():
    """gt_model_forward(GT_ROLE_D), eval mode, against the bf16 model's forward: rules (a) and (b) on the output."""
    from bf16_sru_model import build_bf16_model
    from gantts_amd import _lib as L
    from gantts_amd.engine import StepEngine
    from hip_runner import build_model
    from oracle_runner import build_oracle_model
    spec = BF16_CASES["fold_bi_k4_cond"]["d"]
    md = build_model(spec, 22).eval()
    mo, mb = build_oracle_model(spec, 22), build_bf16_model(spec, 22)
    mo.training = mb.training = False
    x = torch.from_numpy((np.random.RandomState(5).rand(2, 16, 78) * 2 - 1).astype(np.float32))
    with torch.no_grad():
        F, M = mo(x).numpy(), mb(x).numpy()
    eng = StepEngine.for_forward_only(md)
    eng.set_option("sru_d_bf16", 1)
    eng.bind_model(L.ROLE_D, md, with_grads=False)
    xd = x.cuda().contiguous()
    out = torch.empty(2, 16, 1, device="cuda", dtype=torch.float32)
    L.check(L.lib.gt_model_forward(eng._h, L.ROLE_D, L.ptr(xd), None, 2, 16, L.ptr(out), None, L.current_stream()))
    torch.cuda.synchronize()
    E = out.cpu().numpy()
    _track("SRURNN D forward, role D", E, M, F, True)
    assert not np.array_equal(E, F), "suspiciously exact: the option was not on"


# ---------------------------------------------------------------------------------------------
# 6. both options
# ---------------------------------------------------------------------------------------------
def test_sru_d_bf16_with_matmul_bf16_tracks_the_float32_oracle():
    """Both networks on bf16 images, an ordinary two-step run: the bounds of
    test_sru_discriminator_under_the_bf16_option_tracks_the_float32_oracle (outputs 2e-2 relative rms, scalars 3e-2, counts within 2 %)."""
    case = PAIR
    got = _run_pair(case, {"matmul_bf16": 1, "sru_d_bf16": 1}, detached=False)
    ref = oracle_of("bf16/pair", case)
    for k in ("y_hat", "y_hat_static"):
        err = _rms(got[k] - ref[k]) / _rms(ref[k])
        print("bf16 G + bf16 D %s rel-rms %.3e" % (k, err))
        assert err < 2e-2, (k, err)
    assert _rms(got["y_hat"] - ref["y_hat"]) > 0, "suspiciously exact: the bf16 option was not on"
    for st in range(case["steps"]):
        for k, nl in (("d_scalars_%d" % st, 3), ("g_scalars_%d" % st, 4)):
            a, b = np.asarray(got[k]), np.asarray(ref[k])
            print("bf16 G + bf16 D %s got %s ref %s" % (k, a, b))
            rel = np.abs(a - b) / np.maximum(np.abs(b), 1e-2)
            assert (rel[:nl] < 3e-2).all(), (k, a, b)
            if k.startswith("d_"):
                assert (np.abs(a[3:] - b[3:]) <= 0.02 * max(1.0, float(case["B"] * case["T"]))).all(), (k, a, b)
