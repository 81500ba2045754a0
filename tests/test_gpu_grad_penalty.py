"""The discriminator's gradient penalties on the device (gt_set_grad_penalty: "r1", "wgan-gp"):
  1. the parity hook gt_op_grad_penalty against the float64 closed form of tests/grad_penalty_ref.py, element by element inside derived bounds;
  2. two G+D steps against the CPU step reference (torch double backward), injected dropout masks and injected eps;
  3. the generator does not see the penalty;
  4. off is the engine that never saw the option;
  5. the Philox eps draws and the x_hat image;
  6. refusals by message, and the running record."""
import ctypes as Ct
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import gan_objective_ref as G
import grad_penalty_ref as R

KEYS = (0x1234ABCD, 0x0F1E2D3C)
WEIGHT = 10.0
P_DROP = 0.5
GUARD = 64
SENTINEL = 12345.0


# ---------------------------------------------------------------------------------------------------------------------
# 1. the hook
# ---------------------------------------------------------------------------------------------------------------------
def _hook_cases():
    """Every (rows, Da, L, kind); H, cd and the dropout mode rotate underneath so that each of their values meets every rows, Da and L."""
    ROWS, DA, LS = (1, 70, 257), (1, 7, 58), (1, 3)
    out = []
    for ri, di, li, kind in itertools.product(range(3), range(3), range(2), ("r1", "wgan-gp")):
        rows, Da, L = ROWS[ri], DA[di], LS[li]
        H, cd, mode = (12, 256)[(di + li) % 2], (0, 5)[(ri + li) % 2], ("none", "buffer", "philox")[(ri + di) % 3]
        out.append(dict(id="%s-L%d-H%d-cd%d-Da%d-r%d-%s" % (kind, L, H, cd, Da, rows, mode), kind=kind, L=L, H=H, cd=cd, Da=Da, rows=rows, mode=mode))
    return out


HOOK = _hook_cases()


def test_hook_cases_cover_every_value():
    for kind in ("r1", "wgan-gp"):
        for key, vals in (("H", (12, 256)), ("cd", (0, 5)), ("mode", ("none", "buffer", "philox"))):
            for v in vals:
                for k2, v2s in (("L", (1, 3)), ("rows", (1, 70, 257)), ("Da", (1, 7, 58))):
                    for v2 in v2s:
                        assert any(c[key] == v and c[k2] == v2 and c["kind"] == kind for c in HOOK), (kind, key, v, k2, v2)


@functools.lru_cache(maxsize=None)
def operands(cid):
    import zlib
    from test_gpu_gemm_f32 import philox_keep
    c = {x["id"]: x for x in HOOK}[cid]
    rs = np.random.RandomState(zlib.crc32(cid.encode()))
    L, H, cd, Da, rows = c["L"], c["H"], c["cd"], c["Da"], c["rows"]
    ins = [cd + Da] + [H] * (L - 1)
    Ws = [(rs.randn(H, i) / np.sqrt(i)).astype(np.float32) for i in ins]
    w_last = (rs.randn(H) / np.sqrt(H)).astype(np.float32)
    keeps, Hs = [], []
    for l in range(L):
        if c["mode"] == "none":
            keep = np.ones((rows, H), dtype=bool)
        elif c["mode"] == "buffer":
            keep = rs.rand(rows, H) >= P_DROP
        else:
            keep = philox_keep(KEYS[0] + l, KEYS[1], P_DROP, rows, H)
        v = rs.randn(rows, H).astype(np.float32)
        v[v == 0] = np.float32(0.5)
        keeps.append(keep)
        Hs.append(np.where(keep, v, np.float32(0)).astype(np.float32))
    mask = (rs.rand(rows) < 0.7).astype(np.float32)          # ragged, all-zero rows included
    if rows > 1:
        mask[0], mask[-1] = 1.0, 0.0
    else:
        mask[0] = 1.0
    inv_tv = np.float32(1.0 / max(float(mask.sum()), 1.0))
    p = 0.0 if c["mode"] == "none" else P_DROP
    slopes = [R.slopes_of(h, k, p) for h, k in zip(Hs, keeps)]
    # |g| is linear in w_last: the median row gets n = 1
    n = R.closed_form(c["kind"], WEIGHT, Ws, w_last, slopes, mask, inv_tv, cd, Da)["n"]
    med = float(np.median(n[n > 1e-5])) if np.any(n > 1e-5) else 1.0
    w_last = (w_last / np.float32(med)).astype(np.float32)
    ref = R.closed_form(c["kind"], WEIGHT, Ws, w_last, slopes, mask, float(inv_tv), cd, Da)
    # the flat buffers as the engine lays them out: W_l, b_l, ..., w_last, b_last.  Weights: NaN where no weight lies (the biases);
    # gradients: a prior value everywhere (what the D step's backward pass left), so that an untouched slot is recognisable by its bits
    sizes = [(H * i, H) for i in ins] + [(H, 1)]
    n_flat = sum(a + b for a, b in sizes)
    wflat = np.full(n_flat, np.nan, dtype=np.float32)
    gflat = (0.01 * rs.randn(n_flat)).astype(np.float32)
    offs, pos = [], 0
    for (nw, nb), W in zip(sizes, Ws + [w_last]):
        wflat[pos:pos + nw] = W.ravel()
        offs.append((pos, pos + nw))
        pos += nw + nb
    return dict(c=c, Ws=Ws, w_last=w_last, Hs=Hs, keeps=keeps, mask=mask, inv_tv=inv_tv, slopes=slopes, ref=ref, wflat=wflat, gflat=gflat,
                offs=offs, ins=ins, p=p)


def _guarded(n, dtype=torch.float32, fill=SENTINEL):
    full = torch.full((n + 2 * GUARD,), fill, device="cuda", dtype=dtype)
    return full, full[GUARD:GUARD + n]


def run_hook(cid):
    from gantts_amd import _lib as Lb
    o = operands(cid)
    c = o["c"]
    L, H, cd, Da, rows = c["L"], c["H"], c["cd"], c["Da"], c["rows"]
    ld_g = (Da + 3) & ~3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    wflat, gflat = dev(o["wflat"]), dev(o["gflat"])
    Hs = [dev(h) for h in o["Hs"]]
    masks = [dev(k.astype(np.float32)) for k in o["keeps"]]
    mask = dev(o["mask"])
    bufs = {}
    for name, n in [("a%d" % l, rows * H) for l in range(L)] + [("c%d" % l, rows * H) for l in range(L)] + [("g", rows * ld_g), ("g_copy", rows * ld_g),
                                                                                                            ("phi", rows), ("nrm", rows)]:
        bufs[name] = _guarded(n)
    bufs["sums"] = _guarded(2, torch.float64)
    bufs["rec"] = _guarded(3, torch.float64)
    bufs["rec"][1].zero_()
    k = Lb.GpCase()
    k.kind, k.L, k.H, k.cd, k.Da, k.ld_g, k.rows = R.KINDS[c["kind"]], L, H, cd, Da, ld_g, rows
    k.weight, k.inv_tv = WEIGHT, float(o["inv_tv"])
    esz = 4
    for l in range(L):
        k.W[l] = wflat.data_ptr() + esz * o["offs"][l][0]
        k.dW[l] = gflat.data_ptr() + esz * o["offs"][l][0]
        k.Hact[l] = Hs[l].data_ptr()
        k.a[l], k.c[l] = bufs["a%d" % l][1].data_ptr(), bufs["c%d" % l][1].data_ptr()
        d = k.drop[l]
        d.mode = {"none": 0, "philox": 1, "buffer": 2}[c["mode"]]
        d.p = o["p"]
        d.key0, d.key1 = KEYS[0] + l, KEYS[1]
        if c["mode"] == "buffer":
            d.mask, d.ld_mask = masks[l].data_ptr(), H
    k.w_last = wflat.data_ptr() + esz * o["offs"][L][0]
    k.dw_last = gflat.data_ptr() + esz * o["offs"][L][0]
    k.mask = mask.data_ptr()
    for name in ("g", "g_copy", "phi", "nrm", "sums", "rec"):
        setattr(k, name, bufs[name][1].data_ptr())
    Lb.check(Lb.lib.gt_gp_path_counts(None, 1))
    Lb.check(Lb.lib.gt_op_grad_penalty(Ct.byref(k), Lb.current_stream()))
    torch.cuda.synchronize()
    counts = (Ct.c_int64 * Lb.GP_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_gp_path_counts(counts, 1))
    for name, (full, _) in bufs.items():
        fv = full.cpu().numpy()
        assert np.all(fv[:GUARD] == SENTINEL) and np.all(fv[-GUARD:] == SENTINEL), (cid, name, "sentinel")
    out = {name: view.cpu().numpy().copy() for name, (_, view) in bufs.items()}
    out["gflat"] = gflat.cpu().numpy()
    out["counts"] = list(counts)
    return out


def _got_of(o, out):
    c = o["c"]
    L, H, cd, Da, rows = c["L"], c["H"], c["cd"], c["Da"], c["rows"]
    ld_g = (Da + 3) & ~3
    f8 = np.float64
    got = {"g": out["g_copy"].reshape(rows, ld_g)[:, :Da], "r": out["g"].reshape(rows, ld_g)[:, :Da], "phi": out["phi"], "n": out["nrm"]}
    base = {}
    for l in range(L):
        got["a%d" % l], got["c%d" % l] = out["a%d" % l].reshape(rows, H), out["c%d" % l].reshape(rows, H)
        lo, hi = o["offs"][l]
        before, after = o["gflat"][lo:hi].reshape(H, o["ins"][l]), out["gflat"][lo:hi].reshape(H, o["ins"][l])
        got["dW%d" % l], base["dW%d" % l] = after.astype(f8) - before.astype(f8), before
        got["db%d" % l] = (out["gflat"][hi:hi + H].view(np.uint32) != o["gflat"][hi:hi + H].view(np.uint32)).astype(f8)
    lo, hi = o["offs"][L]
    got["dw_last"], base["dw_last"] = out["gflat"][lo:hi].astype(f8) - o["gflat"][lo:hi].astype(f8), o["gflat"][lo:hi]
    got["db_last"] = (out["gflat"][hi:hi + 1].view(np.uint32) != o["gflat"][hi:hi + 1].view(np.uint32)).astype(f8)
    got["s_phi"], got["s_n"] = float(out["sums"][0]), float(out["sums"][1])
    return got, base


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in HOOK])
def test_hook_vs_float64(cid):
    o = operands(cid)
    c = o["c"]
    L, H, cd, Da, rows = c["L"], c["H"], c["cd"], c["Da"], c["rows"]
    out = run_hook(cid)
    got, base = _got_of(o, out)
    bad = R.compare(got, o["ref"], L, base=base)
    assert not bad, (cid, bad)
    ld_g = (Da + 3) & ~3
    assert not np.any(out["g"].reshape(rows, ld_g)[:, Da:]), "pad columns of r"
    # dW_0[:, :cd]: bit-identical to its state before the call
    lo, hi = o["offs"][0]
    b0, a0 = o["gflat"][lo:hi].reshape(H, cd + Da), out["gflat"][lo:hi].reshape(H, cd + Da)
    assert np.array_equal(b0[:, :cd].view(np.uint32), a0[:, :cd].view(np.uint32))
    # the two sums: within rows 2^-53 relative of the double sum of the device's own per-row values
    m = o["mask"].astype(np.float64)
    for dev_sum, per_row in ((out["sums"][0], out["phi"]), (out["sums"][1], out["nrm"])):
        host = math.fsum((m * per_row.astype(np.float64)).tolist())
        assert abs(float(dev_sum) - host) <= rows * 2.0 ** -53 * abs(host), (cid, float(dev_sum), host)
    # the running record: {sum P, sum mean-norm, steps}
    it = float(o["inv_tv"])
    assert out["rec"][2] == 1.0 and out["rec"][0] == out["sums"][0] * it and out["rec"][1] == out["sums"][1] * it
    # the census names every launch
    assert out["counts"] == [0, L + 1, 1, 1, 1, L, L, L + 1], out["counts"]
    # two calls agree to the bit
    again = run_hook(cid)
    for name in out:
        if name != "counts":
            assert np.array_equal(np.asarray(out[name]).view(np.uint8), np.asarray(again[name]).view(np.uint8)), (cid, name)


# ---------------------------------------------------------------------------------------------------------------------
# 2. - 4. whole steps
# ---------------------------------------------------------------------------------------------------------------------
def eps_of_step(case, step):
    return np.random.RandomState(777 + step).rand(case["B"], case["T"], 1).astype(np.float32)


def masks3_of_step(case, step):
    d = case["d"]
    rs = np.random.RandomState(4242 + step)
    return [(rs.rand(case["B"], case["T"], d["hidden_dim"]) >= d["dropout"]).astype(np.float32) for _ in range(d["num_hidden"])]


def all_counts(reset=False):
    from gantts_amd import _lib as Lb
    from test_gpu_gan_objective import head_and_gemm_counts
    gp = (Ct.c_int64 * Lb.GP_PATH_SLOTS)()
    Lb.check(Lb.lib.gt_gp_path_counts(gp, 1 if reset else 0))
    h, g = head_and_gemm_counts(reset)
    return list(gp), h, g


def run_hip_gp(case, obj, kind, weight=WEIGHT, how="hp", inject=True, seed=None, peek=False):
    """tests/test_gpu_gan_objective.py's run_hip_objective with hp.discriminator_grad_penalty set.  how: "hp" (the attributes), "absent"
    (an hp without them), "call" (kind through StepEngine.set_grad_penalty on an engine created without).  Returns (results, counts)."""
    import cases as C
    import gantts_amd.train as Tr
    from gantts_amd import optim, paramgen
    from gantts_amd.engine import StepEngine
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model, make_hp, state_arrays
    hp = make_hp(case)
    hp.gan_objective = obj
    if how == "hp":
        hp.discriminator_grad_penalty, hp.discriminator_grad_penalty_weight = kind, weight
    Tr.hp = hp
    mg, md = build_model(case["g"], 11), build_model(case["d"], 22)
    mg.train(), md.train()
    og = getattr(optim, case["opt_g"][0])(mg.parameters(), **case["opt_g"][1])
    od = getattr(optim, case["opt_d"][0])(md.parameters(), **case["opt_d"][1])
    eng = StepEngine(hp)                      # a fresh engine per run: its record, step counter and seed are this run's alone
    import gantts_amd.train as train_mod
    saved = train_mod.engine_for
    train_mod.engine_for = lambda hp_, model=None: eng
    try:
        if how == "call":
            eng.set_grad_penalty(kind, weight)
        assert eng.grad_penalty == (kind if how != "absent" else None)
        if seed is not None:
            eng.set_seed(seed)
        if case.get("fused"):
            eng.set_option("fused_dstack", 2)
        x_np, y_np, lengths = C.make_batch(case)
        x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
        Tn, N = case["T"], case["B"] * case["T"]
        R_ = paramgen.unit_variance_mlpg_matrix_cuda(hp.windows, Tn)
        sl = torch.from_numpy(np.ascontiguousarray(lengths)).cuda()
        cpu_lengths = list(lengths)
        out = {}
        all_counts(reset=True)
        for step in range(case["steps"]):
            if inject:
                gm, dm = C.make_dropout_masks(case, step)
                third = len(dm) // 3
                mg.set_dropout_masks(0, [torch.from_numpy(m) for m in gm])
                for p in range(3):
                    md.set_dropout_masks(p, [torch.from_numpy(m) for m in dm[p * third:(p + 1) * third]])
                if kind == "wgan-gp":
                    md.set_dropout_masks(3, [torch.from_numpy(m) for m in masks3_of_step(case, step)])
                    eng.set_gp_epsilon(torch.from_numpy(eps_of_step(case, step).reshape(-1)).cuda())
            y_static = get_static_features(y, len(hp.windows), hp.stream_sizes, hp.has_dynamic_features)
            mask = sequence_mask(sl, max_len=Tn).unsqueeze(-1)
            og.zero_grad()
            od.zero_grad()
            y_hat, y_hat_static = eng.apply_generator(mg, x, R_, cpu_lengths)
            if step == 0:
                out["y_hat"], out["y_hat_static"] = y_hat.cpu().numpy(), y_hat_static.cpu().numpy()
            res = Tr.update_discriminator(md, od, x, y_static, y_hat_static, cpu_lengths, mask, "train")
            out["d_scalars_%d" % step] = np.array(res, dtype=np.float64)
            if peek:
                cols = torch.tensor(eng_adv_cols(hp), device="cuda")
                e_, xh = eng.grad_penalty_peek(N, int(cols.numel()))
                out["peek_%d" % step] = (e_.cpu().numpy(), xh.cpu().numpy(), y_static.reshape(N, -1)[:, cols].cpu().numpy(),
                                         y_hat_static.detach().reshape(N, -1)[:, cols].cpu().numpy())
            res = Tr.update_generator(mg, md, og, x, y, y_hat, y_static, y_hat_static, case["adv_w"], cpu_lengths, mask, "train",
                                      mse_w=case["mse_w"], mge_w=case["mge_w"])
            out["g_scalars_%d" % step] = np.array(res, dtype=np.float64)
        torch.cuda.synchronize()
        counts = all_counts(reset=True)
        out.update(state_arrays(mg, md, og, od))
        if eng.grad_penalty is not None:
            rec = eng.grad_penalty_result(reset=True)
            out["gp_record"] = np.array([rec["grad_penalty"], rec["grad_norm_at_penalty"]], dtype=np.float64)
            out["gp_steps"] = rec["steps"]
            again = eng.grad_penalty_result(reset=True)
            assert again == {"grad_penalty": 0.0, "grad_norm_at_penalty": 0.0, "steps": 0}
        return out, counts
    finally:
        train_mod.engine_for = saved


def eng_adv_cols(hp):
    import gantts_oracle as O
    nW = len(hp.windows)
    return list(O.adversarial_columns(hp.stream_sizes, hp.has_dynamic_features, nW, hp.adversarial_streams, hp.mask_nth_mgc_for_adv_loss))


PAIRS = (("bce", "r1"), ("wgan", "wgan-gp"))


def _case(name, obj):
    case = G.STEP_CASES[name]
    return G.bce_twin(case) if obj == "bce" else case


@pytest.mark.gpu
@pytest.mark.parametrize("obj,kind", PAIRS)
@pytest.mark.parametrize("name", ["mlp32", "mlp128_fused", "mlp32_cond"])
def test_two_steps_match_the_step_reference(name, obj, kind):
    case = _case(name, obj)
    got, counts = run_hip_gp(case, obj, kind)
    ref = R.run_step_reference(case, obj, kind, WEIGHT, lambda s: eps_of_step(case, s), lambda s: masks3_of_step(case, s))
    for k in sorted(ref):
        if "scalars" in k or k == "gp_record":
            print("GPSTEP %s %s %s got %s ref %s" % (name, kind, k, np.asarray(got[k]).tolist(), np.asarray(ref[k]).tolist()))
    bad = G.step_close(got, ref)
    assert not bad, "%s / %s: outside 1e-4 of the step reference: %s" % (name, kind, bad)
    assert got["gp_steps"] == case["steps"]
    L = case["d"]["num_hidden"]
    steps = case["steps"]
    assert counts[0] == [steps if kind == "wgan-gp" else 0, steps * (L + 1), steps, steps, steps, steps * L, steps * L, steps * (L + 1)], counts[0]
    # the reference without the penalty is not met: the test sees the feature
    plain = G.run_step_reference(case, obj)
    assert G.step_close(got, plain)


@pytest.mark.gpu
@pytest.mark.parametrize("obj,kind", PAIRS)
def test_generator_does_not_see_the_penalty(obj, kind):
    """adv_w = 0: G's update is the MGE gradient plus what the D step left in the leak buffer, so G's parameters and optimizer state
    after a G+D step carry that buffer; they are bit-identical with the penalty on and off."""
    case = dict(_case("mlp32", obj), adv_w=0.0, steps=1)
    on, _ = run_hip_gp(case, obj, kind)
    off, _ = run_hip_gp(case, obj, None)
    n = 0
    for k in off:
        if k.startswith("G.") or k.startswith("g_scalars"):
            assert np.array_equal(np.asarray(on[k]).view(np.uint8), np.asarray(off[k]).view(np.uint8)), k
            n += 1
    assert n > 4
    assert not np.array_equal(on["D.layers.0.weight"], off["D.layers.0.weight"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mlp32", "mlp128_fused", "mlp32_cond"])
def test_off_is_the_engine_that_never_saw_the_option(name):
    case = _case(name, "bce")
    absent, c_absent = run_hip_gp(case, "bce", None, how="absent")
    none_hp, c_hp = run_hip_gp(case, "bce", None, how="hp")
    called, c_call = run_hip_gp(case, "bce", None, how="call")
    assert c_absent[0] == [0] * 8 and c_hp == c_absent and c_call == c_absent
    assert sum(c_absent[1]) > 0 and sum(c_absent[2]) > 0
    for k in absent:
        for other in (none_hp, called):
            assert np.array_equal(np.asarray(absent[k]).view(np.uint8), np.asarray(other[k]).view(np.uint8)), k
    # weight = 0 with the kind on: no parameter bit changes
    for kind in ("r1", "wgan-gp"):
        zero, c_zero = run_hip_gp(case, "bce", kind, weight=0.0)
        assert c_zero[0][2] == case["steps"]
        for k in absent:
            if k.startswith("D.") or k.startswith("G."):
                assert np.array_equal(np.asarray(absent[k]).view(np.uint8), np.asarray(zero[k]).view(np.uint8)), (kind, k)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Philox eps
# ---------------------------------------------------------------------------------------------------------------------
def host_eps(seed, step, rows):
    from test_gpu_gemm_f32 import philox4x32_10
    M64 = (1 << 64) - 1
    m = ((step + 1) * 0xD6E8FEB86659FD93) & M64
    key0 = ((seed ^ m) & 0xFFFFFFFF) ^ 0x6A09E667
    key1 = ((((seed >> 32) ^ (m >> 32)) & 0xFFFFFFFF) + 0xBB67AE85) & 0xFFFFFFFF
    r = np.arange(rows, dtype=np.uint64)
    w = philox4x32_10(r, np.full(rows, 0x47504550, dtype=np.uint64), 0x243F6A88, 0x85A308D3, key0, key1)
    return ((w[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


@pytest.mark.gpu
def test_philox_eps_and_the_interpolated_image():
    case = G.STEP_CASES["mlp32_cond"]
    N = case["B"] * case["T"]
    seed = 0x1234567
    a, _ = run_hip_gp(case, "wgan", "wgan-gp", inject=False, seed=seed, peek=True)
    b, _ = run_hip_gp(case, "wgan", "wgan-gp", inject=False, seed=seed, peek=True)
    for step in range(case["steps"]):
        eps, xh, real, fake = a["peek_%d" % step]
        assert np.all(eps >= 0) and np.all(eps < 1)
        assert np.array_equal(eps.view(np.uint32), host_eps(seed, step + 1, N).view(np.uint32)), step
        e = eps[:, None]
        want = (e * real).astype(np.float32) + ((np.float32(1) - e) * fake).astype(np.float32)
        assert np.array_equal(xh.view(np.uint32), want.astype(np.float32).view(np.uint32)), step
        assert np.array_equal(eps.view(np.uint32), b["peek_%d" % step][0].view(np.uint32))          # two engines, one seed
    assert not np.array_equal(a["peek_0"][0], a["peek_1"][0])                                     # two steps draw different eps
    for k in a:
        if k.startswith("D.") or k.startswith("G."):
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals():
    import gantts_amd.train as Tr
    from gantts_amd import _lib as Lb
    from gantts_amd.engine import StepEngine, grad_penalty_of
    from hip_runner import build_model, make_hp
    case = G.bce_twin(G.STEP_CASES["mlp32"])
    hp = make_hp(case)
    Tr.hp = hp
    eng = StepEngine(hp)
    h = eng._h
    err = lambda: Lb.lib.gt_last_error().decode()
    assert Lb.lib.gt_set_grad_penalty(h, Lb.ROLE_G, 1, 10.0) == Lb.GT_ERR_INVALID and "discriminator's" in err()
    assert Lb.lib.gt_set_grad_penalty(h, Lb.ROLE_D, 3, 10.0) == Lb.GT_ERR_INVALID and "kind 3" in err()
    for w in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gt_set_grad_penalty: weight ="):
            eng.set_grad_penalty("r1", w)
    with pytest.raises(ValueError, match="grad penalty"):
        eng.set_grad_penalty("r2", 1.0)
    with pytest.raises(ValueError, match="hp.discriminator_grad_penalty"):
        grad_penalty_of(type("HP", (), dict(discriminator_grad_penalty="gp"))())
    assert eng.grad_penalty is None
    # bf16 products
    eng.set_option("matmul_bf16", 1)
    with pytest.raises(ValueError, match="bf16 products"):
        eng.set_grad_penalty("r1", 10.0)
    eng.set_option("matmul_bf16", 0)
    # a recurrent discriminator: at the switch when it is bound first
    lstm = build_model(G.bce_twin(G.STEP_CASES["lstm"])["d"], 22)
    eng.bind_model(Lb.ROLE_D, lstm)
    with pytest.raises(ValueError, match="LSTMRNN or SRURNN"):
        eng.set_grad_penalty("wgan-gp", 10.0)
    # a sharded engine
    eng2 = StepEngine(hp)
    eng2.set_shard(0, 2)
    with pytest.raises(ValueError, match="sharded or communicating"):
        eng2.set_grad_penalty("r1", 10.0)
    # spectral norm at the same time: refused at the switch
    hp_sn = make_hp(case)
    hp_sn.discriminator_spectral_norm = True
    eng3 = StepEngine(hp_sn)
    from gantts_amd import models
    md_sn = models.MLP(spectral_norm=True, **{k: v for k, v in case["d"].items() if k != "kind"}).cuda()
    eng3.bind_model(Lb.ROLE_D, md_sn)
    with pytest.raises(ValueError, match="spectral normalisation"):
        eng3.set_grad_penalty("r1", 10.0)
    # allowed: wgan-gp under "bce", r1 under anything, and the record of an engine that has not stepped
    eng4 = StepEngine(hp)
    eng4.set_grad_penalty("wgan-gp", 1.0)
    eng4.set_grad_penalty("r1", 0.0)
    assert eng4.grad_penalty_result() == {"grad_penalty": 0.0, "grad_norm_at_penalty": 0.0, "steps": 0}
    eng4.set_grad_penalty(None)
    assert eng4.grad_penalty is None
