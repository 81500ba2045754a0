"""The adversarial objectives beyond the reference (GT_OPT_GAN_OBJECTIVE: 1 ls, 2 hinge, 3 wgan; gt_set_weight_clip) on the GPU.

(a) hook level: gt_op_d_head / gt_op_dstack with `objective` set, through the guards of tests/test_gpu_d_tail.py (NaN pitch padding,
    NaN-prefilled results, sentinels, two runs bit-equal, launch census) and its float64 chain, with the head's float64 functions of
    tests/gan_objective_ref.py.  Every element lies inside a bound carried in float64; counts are compared exactly (the inputs keep
    every row 64 bounds away from a kink or a threshold: conditioned_operands, asserted by tests/test_gan_objective_host.py); per tensor, rms(|err| / S) stays under 4x the
    worst value measured on the MI355X (profiles/gan_objective_parity.md).
(b) step level: two G+D steps against the CPU step reference at the suite's 1e-4, counts exactly, for an MLP discriminator on the
    per-layer head, one on the fused stack, an LSTMRNN and an SRURNN discriminator (PARITY UNPINNED like every SRU path: the SRU cell is
    un-vendored third-party code, the oracle restates it), and a conditioned discriminator.  "wgan" runs with the weight clip 0.01.
(c) the clamp: behind every D step each parameter equals clamp(reference update) and none exceeds c; c = 0 is bit-identical to never
    having called gt_set_weight_clip.
(d) same launches as "bce" on the same case.  (e) refusals, by message.

The hook cases reuse test_gpu_d_tail's operand and reference caches, which are keyed by case id: this module registers its cases in
that module's table under ids of its own, and hands `objective` to the hooks by letting run_case build its case structs from subclasses
that preset the field (run_case has no argument for a field that did not exist when it was written)."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

import gan_objective_ref as G
import test_gpu_d_tail as T

MODE_D, MODE_G = T.MODE_D, T.MODE_G
OBJS = ("ls", "hinge", "wgan")

# Per-tensor limits on rms(|got - ref| / S): 4x the worst value measured on the MI355X over this module's matrix against the float64
# reference (profiles/gan_objective_parity.md has the table).  S as in tests/test_gpu_d_tail.py.
RMS_LIM = {
    "head": {
        "Dout": 1.9e-05,      # measured worst 4.649e-06 (hd-vec-K256-r33-G10-wgan)
        "dH": 2.2e-06,        # measured worst 5.257e-07 (hd-f32-K65-r33-D11-ls)
        "dHb": 6.9e-03,       # measured worst 1.703e-03 (hd-img-K130-r17-G10-ls)
        "dHbT": 6.9e-03,      # measured worst 1.703e-03 (hd-img-K130-r17-G10-ls)
        "dW": 2.3e-07,        # measured worst 5.650e-08 (hd-f32-K130-r17-D11-ls)
        "db": 1.7e-07,        # measured worst 4.234e-08 (hd-f32-K65-r17-D11-ls-fill)
        "s_real": 4.3e-07,    # measured worst 1.057e-07 (hd-f32-K1024-r33-D00-ls)
        "s_fake": 8.5e-07,    # measured worst 2.106e-07 (hd-f32-K130-r1-D11-wgan)
        "s_adv": 2.1e-06,     # measured worst 5.059e-07 (hd-vec-K256-r1-G10-hinge)
    },
    "dstack": {
        "Hout1": 1.6e-07,     # measured worst 3.945e-08 (ds256-L2-D0-r33-hinge)
        "Hout2": 2.7e-07,     # measured worst 6.586e-08 (ds256-L3-D0-r74-wgan)
        "dZtop": 1.2e-05,     # measured worst 2.781e-06 (ds256-L3-D1-r33-ls)
        "Dout": 6.3e-05,      # measured worst 1.562e-05 (ds256-L2-D1-r74-ls)
        "dW": 3.4e-06,        # measured worst 8.259e-07 (ds256-L3-D1-r33-ls)
        "db": 2.6e-07,        # measured worst 6.375e-08 (ds128-L3-D1-r74-ls)
        "gadv": 1.8e-06,      # measured worst 4.476e-07 (ds128-L3-G1-r74-ls)
        "s_real": 7.9e-07,    # measured worst 1.952e-07 (ds256-L2-D0-r33-wgan)
        "s_fake": 1.3e-06,    # measured worst 3.075e-07 (ds256-L2-D0-r33-ls)
        "s_adv": 8.7e-07,     # measured worst 2.152e-07 (ds256-L2-G0-r33-hinge)
    },
}


# ---------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------
def _variants():
    """(mode, want_grad, norm) in an order whose every window of 8 covers all of mode x want_grad x {unit_tv, not}."""
    out = []
    for mode in (MODE_D, MODE_G):
        for wg in (1, 0):
            for norm in ("tv", "unit"):
                out.append((mode, wg, norm))
    return out


def _matrix():
    cases = []
    var = _variants()
    shapes = [("f32", K, r) for K in (1, 65, 130) for r in (1, 17, 33)] + [("vec", 256, r) for r in (1, 17, 33)] + [("f32", 1024, 33), ("img", 130, 17)]
    i = 0
    for obj in OBJS:
        for form, K, rows in shapes:
            for mode in (MODE_D, MODE_G):
                _, wg, norm = var[i % 8]
                wg = wg if (i // 8) % 2 == 0 else 1 - wg
                c = T.head_case(K, rows, form, mode=mode, want_grad=wg, drop=T.site("buf", 0.5) if (i % 3 == 0 and K > 1) else None,
                                norm=norm if i % 5 else "tv_dev", b16=(form == "img", form == "img"), acc=1 if (i % 4 == 0 and mode == MODE_D and wg) else 0,
                                tag=obj)
                cases.append((c, obj))
                i += 1
    dshapes = [(hd, rows, L) for hd in (128, 256) for rows in (33, 74) for L in (2, 3)]
    for obj in OBJS:
        for hd, rows, L in dshapes:
            for mode in (MODE_D, MODE_G):
                _, wg, norm = var[i % 8]
                wg = wg if (i // 8) % 2 == 0 else 1 - wg
                c = T.dstack_case(hd, L, mode, wg, rows, mask="ragged", sites=T._sites(L, i), norm=norm, Da=58, col0=425, tag=obj)
                cases.append((c, obj))
                i += 1
    # every (objective, mode, want_grad, unit_tv or not) of either entry at least once: the rotation above leaves gaps, filled here
    have = {(c["entry"], o, c["mode"], c["want_grad"], c["norm"] == "unit") for c, o in cases}
    for entry in ("head", "dstack"):
        for obj in OBJS:
            for mode, wg, norm in var:
                if (entry, obj, mode, wg, norm == "unit") in have:
                    continue
                if entry == "head":
                    c = T.head_case(65, 17, "f32", mode=mode, want_grad=wg, norm=norm, tag=obj + "-fill")
                else:
                    c = T.dstack_case(128, 2, mode, wg, 33, mask="ragged", sites=T._sites(2, i), norm=norm, tag=obj + "-fill")
                cases.append((c, obj))
                i += 1
    out, seen = [], {}
    for c, obj in cases:
        base = c["id"]
        seen[base] = seen.get(base, 0) + 1
        if seen[base] > 1:
            base += "-%d" % seen[base]
        c["objective"] = obj
        c["id"] = base
        out.append(c)
    return out


MATRIX = _matrix()
for _c in MATRIX:
    assert _c["id"] not in T._BY_ID
    T._BY_ID[_c["id"]] = _c          # test_gpu_d_tail's operand cache is keyed by id (see the module docstring)
HEAD = [c for c in MATRIX if c["entry"] == "head"]
DSTACK = [c for c in MATRIX if c["entry"] == "dstack"]


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference: test_gpu_d_tail.reference with the objective's head
# ---------------------------------------------------------------------------------------------------------------------
def _sums(c, q, obj, mistake):
    real = q["real"]
    out = {}
    if c["mode"] == MODE_D:
        out["s_real"] = T._entry([q["lt"][real].sum()], [q["El"][real].sum()], [np.abs(q["lt"][real]).sum()])
        out["s_fake"] = T._entry([q["lt"][~real].sum()], [q["El"][~real].sum()], [np.abs(q["lt"][~real]).sum()])
        out["n_real_ok"], out["n_fake_ok"] = G.counts(obj, q, False, mistake)
    else:
        out["s_adv"] = T._entry([q["lt"].sum()], [q["El"].sum()], [np.abs(q["lt"]).sum()])
    return out


@functools.lru_cache(maxsize=None)
def reference(key, mistake=None):
    """name -> dict(ref, E, S, keep) of every result of the case, the counts, and `_cond` for the input condition."""
    c = T._BY_ID[key]
    obj = c["objective"]
    ops = conditioned_operands(key)
    f8 = np.float64
    none = frozenset()
    res = {}
    mask, inv_tv = ops["mask"].astype(f8), T._inv_tv(c, ops)
    w, bias = ops["w"].astype(f8), float(ops["bias"][0])
    mode_g = c["mode"] == MODE_G
    if c["entry"] == "head":
        h = ops["H"].astype(f8)
        Eh = np.zeros_like(h)
        top_h, top_keep, top_site = h, ops["keep"], c["site"]
    else:
        hs, Ehs, zs, Ezs, Ss = T._chain(c, ops, ops["H0"], ops["keeps"])
        h, Eh = hs[-1], Ehs[-1]
        top_h, top_keep, top_site = hs[-1], ops["keeps"][-1], c["sites"][-1]
        for l in range(1, c["L"]):
            if c["mode"] == MODE_D and (l < c["L"] - 1 or c["hout_top"]):
                res["Hout%d" % l] = T._entry(hs[l], Ehs[l], Ss[l - 1], ops["keeps"][l])
    q = G.head_math(obj, mode_g, c["n_real"], c["n_mask"], h, Eh, w, bias, mask, inv_tv, mistake)
    if c["dout"]:
        res["Dout"] = T._entry(q["D"], q["ED"], np.maximum(np.abs(q["D"]), T.TINY))
    res.update(_sums(c, q, obj, mistake))
    if c["want_grad"]:
        has_act = c["entry"] == "dstack" or c["has_act"]
        fp = T._fprime(top_h, top_keep, top_site, none) if has_act else np.ones_like(top_h)
        dH = q["dz"][:, None] * w[None, :] * fp
        EdH = q["Edz"][:, None] * np.abs(w)[None, :] * fp + T.EPI_ULPS * T.U * np.abs(dH)
        kp = fp != 0
        if c["entry"] == "head":
            if c["form"] != "img":
                res["dH"] = T._entry(dH, EdH, np.abs(dH), kp)
            else:
                Eb = EdH + T.BF16_HALF_ULP * (np.abs(dH) + EdH)
                if c["dHb"]:
                    res["dHb"] = T._entry(dH, Eb, np.abs(dH), kp)
                if c["dHbT"]:
                    res["dHbT"] = T._entry(dH.T, Eb.T, np.abs(dH).T, kp.T)
            if c["want_w"]:
                res["dW"], res["db"] = T._weight_grads(c, q, h, Eh, ops, none, 32)
        elif c["mode"] == MODE_D:
            res["dZtop"] = T._entry(dH, EdH, np.abs(dH), kp)
            res["dW"], res["db"] = T._weight_grads(c, q, h, Eh, ops, none, 32)
        else:
            hd, dZ, EdZ = c["hd"], dH, EdH
            for l in range(c["L"] - 1, 0, -1):
                W = ops["W%d" % l].astype(f8)
                fpl = T._fprime(hs[l - 1], ops["keeps"][l - 1], c["sites"][l - 1], none)
                Sg = np.abs(dZ) @ np.abs(W)
                Eg = (hd + 2) * T.U * Sg + EdZ @ np.abs(W)
                dZ = (dZ @ W) * fpl
                EdZ = Eg * fpl + T.EPI_ULPS * T.U * np.abs(dZ)
            W0c = ops["W0"].astype(f8)[:, c["col0"]:c["col0"] + c["Da"]]
            Sg = np.abs(dZ) @ np.abs(W0c)
            res["gadv"] = T._entry(dZ @ W0c, (hd + 3) * T.U * Sg + EdZ @ np.abs(W0c), Sg)
    res["_cond"] = dict(z=q["z"], Ez=q["Ez"], kinks=G.kinks(obj, q["real"], mode_g))
    return res


def condition_margin(key):
    """min over the rows and their kinks / thresholds of |z - point| / E_z: the input condition asks for more than 64."""
    cond = reference(key)["_cond"]
    d = np.abs(cond["z"][:, None] - cond["kinks"]) / cond["Ez"][:, None]
    return float(np.nanmin(d)) if np.any(~np.isnan(d)) else math.inf


def _near_a_kink(c, ops, x, keeps, row_index):
    """Rows of x (the frames `row_index` of the case) whose head z lies within 64 of its own error bounds of a kink or a count threshold."""
    w, bias = ops["w"].astype(np.float64), float(ops["bias"][0])
    if c["entry"] == "head":
        z, Ez = T._head_z(x.astype(np.float64), np.zeros(x.shape), w, bias)
    else:
        hs, Ehs, _, _, _ = T._chain(c, ops, x, keeps)
        z, Ez = T._head_z(hs[-1], Ehs[-1], w, bias)
    mode_g = c["mode"] == MODE_G
    real = np.ones(len(row_index), dtype=bool) if mode_g else (row_index < c["n_real"])
    d = np.abs(z[:, None] - G.kinks(c["objective"], real, mode_g)) / Ez[:, None]
    return np.any(d <= 64.0, axis=1)            # (NaN: no such point for the row)


def conditioned_operands(key):
    """test_gpu_d_tail.operands(key) with the input condition of this module established: the kernels are per-frame, so a frame whose z
    lies within 64 bounds of a hinge kink (+-1) or of its count threshold is drawn again, from a stream seeded by the case id, as that
    module's own draw does for frames near a LeakyReLU kink (whose condition every redrawn frame keeps).  The cache entry itself is
    amended, once: run_case and the reference read the same operands.  Counts are then exact and the hinge needs no either-side rule."""
    import zlib
    c = T._BY_ID[key]
    ops = T.operands(key)
    if "gan_redrawn" in ops:
        return ops
    head = c["entry"] == "head"
    x = ops["H"] if head else ops["H0"]
    keeps = [ops["keep"]] if head else ops["keeps"]
    d = c["site"] if head else c["sites"][0]
    act = bool(c["has_act"]) if head else True
    img = head and c["form"] == "img"
    rs = np.random.RandomState(zlib.crc32((key + "/kinks").encode()))
    todo = np.flatnonzero(_near_a_kink(c, ops, x, keeps, np.arange(c["rows"])))
    redrawn = int(todo.size)
    for _ in range(2000):
        if not todo.size:
            break
        pre = rs.randn(len(todo), x.shape[1]).astype(np.float32)
        pre[pre == 0] = np.float32(0.5)
        v = T._act_of(pre, keeps[0][todo], d) if act else np.tanh(pre).astype(np.float32)
        x[todo] = T._bf16(v) if img else v
        sub = [k[todo] for k in keeps]
        bad = T._ambiguous_rows(c, ops, x[todo], sub) | _near_a_kink(c, ops, x[todo], sub, todo)
        todo = todo[bad]
    assert not todo.size, key
    ops["gan_redrawn"] = redrawn
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# (a) the hooks against float64
# ---------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def hook_objective(obj_id):
    """test_gpu_d_tail.run_case builds its structs as Lb.DHeadCase() / Lb.DStackCase(): for the duration, subclasses that preset `objective`."""
    from gantts_amd import _lib as Lb
    heads, stacks = Lb.DHeadCase, Lb.DStackCase

    class Head(heads):
        def __init__(self):
            super().__init__()
            self.objective = obj_id

    class Stack(stacks):
        def __init__(self):
            super().__init__()
            self.objective = obj_id
    Lb.DHeadCase, Lb.DStackCase = Head, Stack
    try:
        yield
    finally:
        Lb.DHeadCase, Lb.DStackCase = heads, stacks


def _check_case(c):
    from gantts_amd import _lib as Lb
    tag = c["id"]
    ops = conditioned_operands(tag)
    with hook_objective(G.IDS[c["objective"]]):
        rc, counts, scal, out = T.run_case(c)
    assert rc == Lb.GT_OK, "%s: %s" % (tag, Lb.lib.gt_last_error())
    exp = T.expected_counts(c)           # the slot of the FORM, whatever the objective
    assert counts == exp, "%s: launches %s, expected %s" % (tag, {i: n for i, n in enumerate(counts) if n}, {i: n for i, n in enumerate(exp) if n})
    res = reference(tag)
    written = set(T.tensors(res)) - {"s_real", "s_fake", "s_adv"}
    got = {}
    for name, (flat, logical, buf) in out.items():
        buf.check_outside(flat, name, tag)
        if name in written:
            v = T._from_bf16_bits(logical) if buf.dtype == np.uint16 else logical
            assert not np.isnan(v).any(), "%s: %s has %d elements that are NaN or were never written" % (tag, name, int(np.isnan(v).sum()))
            got[name] = v.astype(np.float64)
        else:
            same = np.array_equal(logical.view(np.uint32), buf.view(buf.host).view(np.uint32)) if buf.dtype == np.float32 else \
                np.array_equal(logical, buf.view(buf.host))
            assert same, "%s: %s was written although the case does not ask for it" % (tag, name)
    assert written <= set(got), (tag, sorted(written - set(got)))
    names = ["s_real", "s_fake", "n_real_ok", "n_fake_ok", "s_adv"]
    mine = names[:4] if c["mode"] == MODE_D else names[4:]
    for i, name in enumerate(names):
        if name in mine:
            assert math.isfinite(scal[i]), "%s: %s = %r" % (tag, name, scal[i])
            got[name] = np.array([scal[i]]) if name.startswith("s_") else scal[i]
        else:
            assert math.isnan(scal[i]), "%s: %s = %r was written by a pass that does not own it" % (tag, name, scal[i])
    if c["norm"] == "unit":
        assert math.isnan(scal[5]) and math.isnan(scal[6]), "%s: unit_tv touched the normaliser" % tag
    else:
        assert scal[5] == float(ops["tv"]) and scal[6] == float(np.float32(1.0) / ops["tv"]), (tag, scal[5], scal[6])
    assert scal[7] == T.n_partials(c), (tag, scal[7])
    for name in T.tensors(res):
        bad, rms, worst = T.criterion(got[name], res[name])
        lim = RMS_LIM[c["entry"]][name]
        print("GANOBJSTAT %s %s %s rms=%.3e worst_bound_ratio=%.3e" % (c["entry"], tag, name, rms, worst))
        assert bad == 0, "%s: %s has %d elements outside the float64 bound (worst ratio %.3g)" % (tag, name, bad, worst)
        assert rms <= lim, "%s: %s rms(|err| / S) %.3e over the limit %r" % (tag, name, rms, lim)
    for name in ("n_real_ok", "n_fake_ok"):
        if name in res:
            assert got[name] == res[name], "%s: %s = %r, the reference counts %r" % (tag, name, got[name], res[name])
    with hook_objective(G.IDS[c["objective"]]):
        rc2, _, scal2, out2 = T.run_case(c)
    assert rc2 == Lb.GT_OK
    for name in out:
        assert np.array_equal(out[name][0].view(np.uint8), out2[name][0].view(np.uint8)), "%s: %s differs between two runs" % (tag, name)
    assert np.array_equal(np.array(scal).view(np.uint64), np.array(scal2).view(np.uint64)), "%s: the scalars differ between two runs" % tag


@pytest.mark.gpu
@pytest.mark.parametrize("c", HEAD, ids=[c["id"] for c in HEAD])
def test_d_head_objective_vs_float64(c):
    _check_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", DSTACK, ids=[c["id"] for c in DSTACK])
def test_dstack_objective_vs_float64(c):
    _check_case(c)


# ---------------------------------------------------------------------------------------------------------------------
# (b) - (d) whole steps
# ---------------------------------------------------------------------------------------------------------------------
def head_and_gemm_counts(reset=False):
    import ctypes as Ct
    from gantts_amd import _lib as Lb
    h = (Ct.c_int64 * Lb.HEAD_PATH_SLOTS)()
    g = (Ct.c_int64 * Lb.GEMM_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_head_path_counts(h, 1 if reset else 0))
    Lb.check(Lb.lib.gt_gemm_path_counts(g, 1 if reset else 0))
    return list(h), list(g)


def run_hip_objective(case, obj="bce", clip=None, snapshots=None):
    """tests/hip_runner.py's run_hip_case with hp.gan_objective / hp.discriminator_weight_clip set (a discriminator's injected masks cut
    in thirds, as tests/test_gpu_sru_discriminator.py's driver does).  clip=None never calls gt_set_weight_clip.  snapshots: receives
    the discriminator's state behind every D step.  Returns (results, (head counts, gemm counts) of the run)."""
    import cases as C
    import gantts_amd.train as Tr
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp, state_arrays
    hp = make_hp(case)
    hp.gan_objective = obj
    if clip is not None:
        hp.discriminator_weight_clip = clip
    Tr.hp = hp
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    mg.train(), md.train()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = engine_for(hp, mg)
    assert eng.gan_objective == obj
    if case.get("fused"):
        eng.set_option("fused_dstack", 2)
    x_np, y_np, lengths = C.make_batch(case)
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    Tn = case["T"]
    R = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
    sl = torch.from_numpy(np.ascontiguousarray(lengths)).cuda()
    cpu_lengths = list(lengths)
    out = {}
    head_and_gemm_counts(reset=True)
    for step in range(case["steps"]):
        gm, dm = C.make_dropout_masks(case, step)
        third = len(dm) // 3
        mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
        if third:
            for p in range(3):
                md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * third:(p + 1) * third]])
        y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
        mask = sequence_mask(sl, max_len=Tn).unsqueeze(-1)
        og.zero_grad()
        od.zero_grad()
        y_hat, y_hat_static = Tr.apply_generator(mg, x, R, cpu_lengths)
        if step == 0:
            out["y_hat"] = y_hat.cpu().numpy()
            out["y_hat_static"] = y_hat_static.cpu().numpy()
        res = Tr.update_discriminator(md, od, x, y_static, y_hat_static, cpu_lengths, mask, "train")
        out["d_scalars_%d" % step] = np.array(res, dtype=np.float64)
        if snapshots is not None:
            snapshots.append({"D." + k: v.cpu().numpy().copy() for k, v in md.state_dict().items()})
        res = Tr.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cpu_lengths, mask, "train",
                                  mse_w=case["mse_w"], mge_w=case["mge_w"])
        out["g_scalars_%d" % step] = np.array(res, dtype=np.float64)
    torch.cuda.synchronize()
    counts = head_and_gemm_counts(reset=True)
    out.update(state_arrays(mg, md, og, od))
    return out, counts


CLIP = 0.01


def _clip_of(obj):
    return CLIP if obj == "wgan" else 0.0


@functools.lru_cache(maxsize=None)
def step_reference(name, obj):
    snaps = []
    return G.run_step_reference(G.STEP_CASES[name], obj, clip=_clip_of(obj), snapshots=snaps), snaps


@functools.lru_cache(maxsize=None)
def step_run(name, obj):
    snaps = []
    out, counts = run_hip_objective(G.STEP_CASES[name], obj, clip=_clip_of(obj) or None, snapshots=snaps)
    return out, counts, snaps


@pytest.mark.gpu
@pytest.mark.parametrize("obj", OBJS)
@pytest.mark.parametrize("name", sorted(G.STEP_CASES))
def test_two_steps_match_the_step_reference(name, obj):
    """(b).  The "sru" case is PARITY UNPINNED, like every SRU path."""
    got, _, _ = step_run(name, obj)
    ref, _ = step_reference(name, obj)
    for k in sorted(ref):
        if "scalars" in k:
            print("GANOBJSTEP %s %s %s got %s ref %s" % (name, obj, k, got[k].tolist(), ref[k].tolist()))
    bad = G.step_close(got, ref)
    assert not bad, "%s / %s: outside 1e-4 of the step reference: %s" % (name, obj, bad)
    if name == "mlp128_fused":
        head, _ = step_run(name, obj)[1]
        assert head[T.DSTACK128] == 2 * G.STEP_CASES[name]["steps"], head       # both passes of every step took the fused stack


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mlp32", "mlp128_fused", "lstm", "sru"])
def test_weight_clip_follows_every_update(name):
    """(c): behind every D step each parameter is clamp(reference update, -c, c) at 1e-4 of the tensor's scale, and none exceeds c."""
    _, _, snaps = step_run(name, "wgan")
    _, ref_snaps = step_reference(name, "wgan")
    assert len(snaps) == len(ref_snaps) == G.STEP_CASES[name]["steps"]
    for step, (g, r) in enumerate(zip(snaps, ref_snaps)):
        bad = G.step_close(g, r)
        assert not bad, "%s step %d: %s" % (name, step, bad)
        for k, v in g.items():
            assert float(np.abs(v).max()) <= np.float32(CLIP), (name, step, k, float(np.abs(v).max()))
            assert float(np.abs(r[k]).max()) <= np.float32(CLIP)
    assert any(np.any(np.abs(v) == np.float32(CLIP)) for v in snaps[0].values())          # the clamp was at work


@pytest.mark.gpu
def test_weight_clip_zero_is_bit_identical_to_no_clip():
    case = G.STEP_CASES["mlp32"]
    never, _ = run_hip_objective(case, "wgan", clip=None)
    zero, _ = run_hip_objective(case, "wgan", clip=0.0)

    def explicit_zero():         # the call itself, with c = 0, on the engine of a fresh run
        import gantts_amd.engine as E
        from gantts_amd import _lib as Lb
        orig = E.StepEngine.__init__

        def init(self, hp):
            orig(self, hp)
            self.set_weight_clip(Lb.ROLE_D, 0.0)
        E.StepEngine.__init__ = init
        try:
            return run_hip_objective(case, "wgan", clip=None)[0]
        finally:
            E.StepEngine.__init__ = orig
    called = explicit_zero()
    for k in never:
        a, b, c3 = np.asarray(never[k]), np.asarray(zero[k]), np.asarray(called[k])
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c3.view(np.uint8)), k
    clipped, _ = run_hip_objective(case, "wgan", clip=CLIP)
    assert not np.array_equal(clipped["D.last_linear.weight"], never["D.last_linear.weight"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mlp32", "mlp128_fused", "lstm", "sru", "mlp32_cond"])
def test_every_objective_issues_the_launches_of_bce(name):
    """(d): gt_head_path_counts and gt_gemm_path_counts of the two steps, objective by objective, against "bce" on the same case."""
    _, base = run_hip_objective(G.bce_twin(G.STEP_CASES[name]), "bce")
    assert sum(base[0]) > 0 and sum(base[1]) > 0
    for obj in OBJS:
        counts = step_run(name, obj)[1]
        assert counts[0] == base[0], (name, obj, "head", {i: (a, b) for i, (a, b) in enumerate(zip(counts[0], base[0])) if a != b})
        assert counts[1] == base[1], (name, obj, "gemm", {i: (a, b) for i, (a, b) in enumerate(zip(counts[1], base[1])) if a != b})


# ---------------------------------------------------------------------------------------------------------------------
# (e) refusals, by message
# ---------------------------------------------------------------------------------------------------------------------
def _engine_and_models(obj, last_sigmoid):
    import gantts_amd.train as Tr
    from gantts_amd.engine import StepEngine
    from hip_runner import build_model, make_hp
    case = G.STEP_CASES["mlp32"]
    hp = make_hp(case)
    hp.gan_objective = obj
    Tr.hp = hp
    md = build_model(dict(case["d"], last_sigmoid=last_sigmoid), 22)
    return StepEngine(hp), md


@pytest.mark.gpu
def test_refusals():
    import ctypes as Ct
    from gantts_amd import _lib as Lb
    eng, md_sig = _engine_and_models("bce", True)
    _, md_lin = _engine_and_models("bce", False)
    # an unknown objective id, by name and by number
    with pytest.raises(ValueError, match="GT_OPT_GAN_OBJECTIVE takes 0"):
        eng.set_option("gan_objective", 7)
    with pytest.raises(ValueError, match="GT_OPT_GAN_OBJECTIVE takes 0"):
        eng.set_option("gan_objective", -1)
    hp_bad = type("HP", (), dict(gan_objective="lsgan"))()
    with pytest.raises(ValueError, match="hp.gan_objective"):
        from gantts_amd.engine import gan_objective_of
        gan_objective_of(hp_bad)
    # objective 0 with last_sigmoid=False: the unchanged message, at bind
    with pytest.raises(ValueError, match="last_sigmoid=True"):
        eng.bind_model(Lb.ROLE_D, md_lin)
    # option second: a bound sigmoid discriminator refuses 1 .. 3, and the option stays what it was
    eng.bind_model(Lb.ROLE_D, md_sig)
    for obj_id in (1, 2, 3):
        with pytest.raises(ValueError, match="last_sigmoid=False"):
            eng.set_option("gan_objective", obj_id)
    assert eng.gan_objective == "bce"
    # bind second: objective 2, then a sigmoid discriminator
    eng2, md_sig2 = _engine_and_models("hinge", True)
    with pytest.raises(ValueError, match="last_sigmoid=False"):
        eng2.bind_model(Lb.ROLE_D, md_sig2)
    _, md_lin2 = _engine_and_models("hinge", False)
    eng2.bind_model(Lb.ROLE_D, md_lin2)
    with pytest.raises(ValueError, match="last_sigmoid=True"):
        eng2.set_option("gan_objective", 0)
    # the clip: negative, NaN, infinite, role G
    for c in (-0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gt_set_weight_clip: c ="):
            eng.set_weight_clip(Lb.ROLE_D, c)
    with pytest.raises(ValueError, match="discriminator's"):
        eng.set_weight_clip(Lb.ROLE_G, 0.01)
    eng.set_weight_clip(Lb.ROLE_D, 0.0)
    # a hook case with objective = 7: refused before any launch
    Lb.check(Lb.lib.gt_head_path_counts(None, 1))
    fake = Ct.c_void_p(64)
    g = Lb.DHeadCase()
    g.mode, g.K, g.ldh, g.rows, g.n_real, g.n_mask, g.has_tv, g.tv, g.eps = 0, 64, 64, 40, 20, 20, 1, 30.0, 1e-20
    g.want_grad, g.want_w, g.lddh, g.has_act = 1, 1, 64, 1
    g.H = g.w = g.bias = g.mask = g.Dout = g.dH = g.dW = g.db = fake
    g.objective = 7
    assert Lb.lib.gt_op_d_head(Ct.byref(g), None) == Lb.GT_ERR_INVALID and b"objective = 7" in Lb.lib.gt_last_error()
    k = Lb.DStackCase()
    k.mode, k.L, k.hidden_dim, k.want_grad, k.rows, k.n_real, k.n_mask, k.has_tv, k.tv, k.eps = 1, 2, 256, 1, 40, 40, 40, 1, 30.0, 1e-20
    k.Da, k.col0, k.ldw0, k.ld_gadv = 58, 425, 483, 58
    k.H0 = k.w_last = k.b_last = k.mask = k.W0 = k.gadv = fake
    for l in range(4):
        k.W[l] = k.b[l] = 64
    k.objective = 7
    assert Lb.lib.gt_op_dstack(Ct.byref(k), None) == Lb.GT_ERR_INVALID and b"objective = 7" in Lb.lib.gt_last_error()
    k.objective = -1
    assert Lb.lib.gt_op_dstack(Ct.byref(k), None) == Lb.GT_ERR_INVALID
    counts = (Ct.c_int64 * Lb.HEAD_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_head_path_counts(counts, 1))
    assert sum(counts) == 0
