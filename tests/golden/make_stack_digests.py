"""Digests of two G + D steps and one plain forward per role through every stack (MLP, LSTM, SRU) in both storage forms, case by case:
what tests/test_gpu_stack_digests.py demands bit for bit.

    python tests/golden/make_stack_digests.py [out.json [case ...]]      (needs the GPU; default: stack_step_digests.json beside this file)

Without case names every case is recorded; with names only those are, into the entries out.json already holds (the others stay as they are).

Every case runs hip_runner.run_hip_case's loop (apply_generator -> update_discriminator -> update_generator, `steps` = 2: the second
step goes through re-made shadows, accumulated-gradient flags and warm optimizer state) from seeded state and records the SHA-256 of
y_hat, y_hat_static, every step's D and G scalar tuples (as float64) and every parameter (sorted by name); then of one plain
gt_model_forward of each role on the step's engine (the generator on the case's x, the discriminator on the columns of [x | y] repeated
to its input width); and the five host-side launch-count vectors (gt_gemm_path_counts, gt_gemm_b16_path_counts, gt_sru_path_counts,
gt_head_path_counts, gt_lstm_path_counts), reset in front of the case, as {slot: count} of the non-zero slots.  The counts are how
"the same launches" is shown: the test demands them equal, not merely the values.

The loop is run_hip_case's with one difference: a discriminator's injected masks are dealt in thirds of what make_dropout_masks drew
(an SRURNN discriminator has more sites per pass than cases.hidden_sites counts), as tests/test_gpu_sru_d_bf16.py does.

The recorded file is the behaviour of the commit named in it -- the one before the output layer and the bf16 product helpers became one
function each; it is re-recorded only by a change that means to change a bit or a launch of the step.  A case added later carries its own
"recorded_on" (CASE_RECORDED_ON): the three precision routes of the float32 family were recorded on the commit before its product precision
became an argument."""
import copy
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DEFAULT_OUT = os.path.join(HERE, "stack_step_digests.json")
RECORDED_ON = "f6c54f8"
CASE_RECORDED_ON = {"mlp_mixed_bf16": "3a0194b", "lstm_d_p16": "3a0194b", "chain_d_fused_f32": "3a0194b"}      # cases added after RECORDED_ON
BF16, D16 = {"matmul_bf16": 1}, {"sru_d_bf16": 1}
STEPS = 2
COUNTERS = ("gemm", "gemm_b16", "sru", "head", "lstm")
DIGESTS = ("y_hat", "y_hat_static", "d", "g", "params", "forward_g", "forward_d", "all")


def _with_hidden(case, hidden_dim):
    case = copy.deepcopy(case)
    case["g"]["hidden_dim"] = hidden_dim
    return case


def case_table():
    """name -> (case, engine options)"""
    import cases as C
    from test_gpu_sru_d_bf16 import PAIR
    K, O = C.CASES, C.ORACLE_ONLY_CASES
    return {
        "mlp_f32": (K["acoustic_mlp_dropout"], {}),
        "mlp_bf16": (K["acoustic_mlp_dropout"], BF16),
        "mlp_sigmoid_f32": (K["acoustic_mlp_sigmoid_g"], {}),      # in_dim 425: pitched gy, sigmoid gradient, mse_w
        "mlp_sigmoid_bf16": (K["acoustic_mlp_sigmoid_g"], BF16),
        "duration_bf16": (K["duration_mlp"], BF16),                # R is None
        "lstm_f32": (O["acoustic_lstm_dropout"], {}),              # H = 12, three layers, bidirectional, inter-layer dropout
        "lstm_bf16": (_with_hidden(O["acoustic_lstm_dropout"], 16), BF16),      # (12 is no multiple of 8: it would silently stay float32)
        "lstm_sigmoid_bf16": (K["acoustic_lstm_sigmoid_g"], BF16),
        "lstm_d_f32": (O["acoustic_lstm_d_dropout"], {}),          # recurrent G and D, two row groups
        "i2o_rnn_f32": (O["vc_in2out_rnn_dropout"], {}),
        "i2o_rnn_bf16": (_with_hidden(O["vc_in2out_rnn_dropout"], 24), BF16),
        "sru_f32": (O["acoustic_sru_dropout"], {}),
        "sru_k3_f32": (O["acoustic_sru_uni_k3"], {}),
        "sru_bf16_nofold": (_with_hidden(O["acoustic_sru_dropout"], 24), BF16),
        "sru_pair_f32": (PAIR, {}),                                # SRU G and SRU D, H = 64, T = 16: the folded scans write the output layer's images
        "sru_pair_d16": (PAIR, D16),
        "sru_pair_both": (PAIR, dict(BF16, **D16)),
        # the float32 family's precision routes: G on float32 storage with bf16 products (12 is no multiple of 8; pair launches) beside D on
        # bf16 storage; both recurrent stacks (12, 20) on float32 storage at bf16 precision; the conditioned split first layer, its weight
        # gradient with the rider and the fused stack
        "mlp_mixed_bf16": (_with_hidden(K["acoustic_mlp_dropout"], 12), BF16),
        "lstm_d_p16": (O["acoustic_lstm_d_dropout"], BF16),
        "chain_d_fused_f32": (K["acoustic_chain_d"], {"fused_dstack": 2}),
    }


CASES = ("mlp_f32", "mlp_bf16", "mlp_sigmoid_f32", "mlp_sigmoid_bf16", "duration_bf16", "lstm_f32", "lstm_bf16", "lstm_sigmoid_bf16",
         "lstm_d_f32", "i2o_rnn_f32", "i2o_rnn_bf16", "sru_f32", "sru_k3_f32", "sru_bf16_nofold", "sru_pair_f32", "sru_pair_d16",
         "sru_pair_both", "mlp_mixed_bf16", "lstm_d_p16", "chain_d_fused_f32")


def _read_counts(eng, reset):
    from gantts_amd import _lib as L
    out = {}
    for key, fn, n in (("gemm", L.lib.gt_gemm_path_counts, L.GEMM_PATH_SLOTS), ("gemm_b16", L.lib.gt_gemm_b16_path_counts, L.GEMM_B16_PATH_SLOTS),
                       ("sru", L.lib.gt_sru_path_counts, L.SRU_PATH_SLOTS), ("head", L.lib.gt_head_path_counts, L.HEAD_PATH_SLOTS)):
        buf = (ctypes.c_int64 * n)()
        L.check(fn(buf, 1 if reset else 0))
        out[key] = list(buf)
    out["lstm"] = eng.lstm_path_counts(reset=reset) if eng is not None else []
    return out


def _run(case, options):
    """-> (run_hip_case's outputs + forward_g / forward_d, the five count vectors)"""
    import torch
    import cases as C
    import gantts_amd.train as T
    from gantts_amd import _lib as L
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp, state_arrays
    hp = make_hp(case)
    T.hp = hp
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    (mg.train(), md.train()) if case["dropout_on"] else (mg.eval(), md.eval())
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = engine_for(hp, mg)
    for k, v in options.items():
        eng.set_option(k, v)
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    Tn = case["T"]
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn) if bool(np.any(case["has_dynamic_features"])) else None
    mask = sequence_mask(torch.from_numpy(np.ascontiguousarray(lengths)).cuda(), max_len=Tn).unsqueeze(-1)
    y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
    cl = list(lengths)
    torch.cuda.synchronize()
    _read_counts(eng, reset=True)
    out = {}
    for step in range(STEPS):
        if case["dropout_on"]:
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
        out["d_scalars_%d" % step] = np.array(T.update_discriminator(md, od, x, y_static, y_hat_static, cl, mask, "train"), dtype=np.float64)
        out["g_scalars_%d" % step] = np.array(T.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cl, mask, "train",
                                                                 mse_w=case["mse_w"], mge_w=case["mge_w"]), dtype=np.float64)
    torch.cuda.synchronize()
    out.update(state_arrays(mg, md, og, od))
    # one plain forward of each role on the engine the steps ran on (its options, its bound networks)
    fg = eng.model_forward(mg, x, R, lengths=cl)
    out["forward_g"] = np.concatenate([t.cpu().numpy().reshape(-1) for t in (fg if isinstance(fg, tuple) else (fg,))])
    src = torch.cat([x, y], dim=-1)
    xd = src[..., torch.arange(md.in_dim, device=src.device) % src.size(-1)].contiguous()
    eng.bind_model(L.ROLE_D, md, with_grads=False)
    eng.set_lengths(cl, case["B"], Tn)
    fd = torch.empty(case["B"], Tn, md.out_dim, device="cuda", dtype=torch.float32)
    L.check(L.lib.gt_model_forward(eng._h, L.ROLE_D, L.ptr(xd), None, case["B"], Tn, L.ptr(fd), None, L.current_stream()))
    torch.cuda.synchronize()
    out["forward_d"] = fd.cpu().numpy()
    return out, _read_counts(eng, reset=False)


def run_case(name):
    """-> {"y_hat": sha256, ..., "all": sha256, "counts": {counter: {slot: launches}}}"""
    case, options = case_table()[name]
    out, counts = _run(case, options)
    params = sorted(k for k in out if k[:2] in ("G.", "D.") and ".opt." not in k)
    assert out["y_hat"].dtype == np.float32 and params
    parts = {"y_hat": [out["y_hat"]], "y_hat_static": [out["y_hat_static"]],
             "d": [out["d_scalars_%d" % s] for s in range(STEPS)], "g": [out["g_scalars_%d" % s] for s in range(STEPS)],
             "params": [out[k] for k in params], "forward_g": [out["forward_g"]], "forward_d": [out["forward_d"]]}
    rec, whole = {}, hashlib.sha256()
    for part in DIGESTS[:-1]:
        h = hashlib.sha256()
        for a in parts[part]:
            b = np.ascontiguousarray(a).tobytes()
            h.update(b)
            whole.update(b)
        rec[part] = h.hexdigest()
    rec["all"] = whole.hexdigest()
    rec["counts"] = {k: {str(i): int(v) for i, v in enumerate(counts[k]) if v} for k in COUNTERS}
    if name in CASE_RECORDED_ON:
        rec["recorded_on"] = CASE_RECORDED_ON[name]
    return rec


def check_family(name, rec):
    """Record time only: the case ran the product family it is named for (a width that silently falls back is caught before it is recorded)."""
    case, _ = case_table()[name]
    b16 ={int(k): v for k, v in rec["counts"]["gemm_b16"].items()}
    sru = {int(k): v for k, v in rec["counts"]["sru"].items()}
    products = sum(v for k, v in b16.items() if k < 60)      # (slots below the cast kernels': b16_path_slot)
    if name.endswith("_f32") or name == "lstm_d_p16":
        assert not b16, "%s: launches of the bf16 family %s" % (name, b16)
    else:
        assert products > 0, "%s: no bf16 product launch" % name
    if name in ("lstm_d_p16", "mlp_mixed_bf16"):      # bf16 products on float32 storage: gemm_path_slot's precision bit, the bf16 pair launch
        p16 = [k for k in map(int, rec["counts"]["gemm"]) if (k < 576 and (k // 6) % 2) or k == 579]
        assert p16, "%s: no float32-family launch at bf16 precision %s" % (name, rec["counts"]["gemm"])
    if name == "chain_d_fused_f32":      # split weight gradient with its rider (GEMM_PATH_TN_PAIR + 1), fused stack (HEAD_PATH_DSTACK128 / 256)
        assert ("580" in rec["counts"]["gemm"] or "581" in rec["counts"]["gemm"]) and ("11" in rec["counts"]["head"] or "12" in rec["counts"]["head"]), rec["counts"]
    if name in ("sru_pair_d16", "sru_pair_both"):
        # folded: every scan with a product behind it writes that product's images itself -- each generator layer (the top one writes the
        # output layer's, so no cast of its input is launched), each discriminator layer but the top one (the head reads float32)
        n_g, n_d = STEPS + 1, 2 * STEPS + 1      # stack forwards: one per apply_generator / two D passes per step, + the plain forward
        want = n_d * (case["d"]["num_hidden"] - 1) + (n_g * case["g"]["num_hidden"] if name == "sru_pair_both" else 0)
        img = sru.get(2, 0) + sru.get(4, 0)      # SRU_PATH_FWD_CS + 2 * (eight waves) + 1: the image forms
        assert img == want, "%s: %d image-form forward scans, %d expected of folded stacks %s" % (name, img, want, sru)


def main(argv):
    for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    names = argv[2:] or CASES
    record = {"recorded_on": RECORDED_ON, "steps": STEPS, "cases": {}}
    if argv[2:]:
        with open(out) as f:
            record = json.load(f)
    for name in names:
        record["cases"][name] = run_case(name)
        print("%-18s %s" % (name, json.dumps(record["cases"][name]["counts"], sort_keys=True)), flush=True)
    for name in names:
        check_family(name, record["cases"][name])
    with open(out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d cases recorded, %d held" % (out, len(names), len(record["cases"])))


if __name__ == "__main__":
    main(sys.argv)
