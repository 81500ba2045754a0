"""CPU checks of tests/frame_kernels_ref.py, the references and comparators tests/test_gpu_frame_kernels.py holds the per-frame kernels
against: the references agree with oracle/ in float64, the restated grid-stride assignment is a partition of every shape in the matrix,
and every comparator fails on the mistake it exists to catch, seeded on the reference side while the `result` is the correct one."""
import math

import numpy as np
import pytest
import torch

import frame_kernels_ref as R
import gantts_oracle as O
from frame_kernels_ref import F32, U, U64


def rs_of(*key):
    return np.random.RandomState(sum((i + 1) * 104729 * int(v) for i, v in enumerate(key)) % (1 << 31))


def _case(rows, D, rs, four_valued=False):
    a, b = rs.randn(rows, D).astype(np.float32), rs.randn(rows, D).astype(np.float32)
    m, lengths, T = R.make_mask(rows, rs, four_valued)
    return a, b, m, lengths, T


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ---------------------------------------------------------------------------------------------------------------------
# the references against oracle/
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", sorted({s[0] for s in R.RED_SHAPES}))
def test_masks_are_the_oracles_sequence_mask(rows):
    m, lengths, T = R.make_mask(rows, rs_of(rows))
    B = len(lengths)
    assert B * T == rows and set(np.unique(m)) <= {0.0, 1.0}
    assert np.array_equal(m.reshape(B, T), O.sequence_mask(lengths, T).numpy())
    if B >= 3:
        assert {0, 1, T} <= set(int(v) for v in lengths)
    m4, _, _ = R.make_mask(rows, rs_of(rows), four_valued=True)
    assert set(np.unique(m4)) <= {0.0, 0.25, 0.5, 1.0} and np.array_equal(m4 > 0, m > 0)


@pytest.mark.parametrize("shape", R.RED_SHAPES[:7], ids=["%dx%d" % s[:2] for s in R.RED_SHAPES[:7]])
def test_sqerr_reference_is_the_oracles_masked_mse(shape):
    """S / tv against masked_mse in float64: each difference carries one float32 rounding (the products with a 0 / 1 mask are exact), so
    its square is within 2 u + u^2; the gradient 2 w (a m - b m) m / tv carries four (difference, 1 / tv, gs, gs diff): 4 u + 7 u^2."""
    rows, D = shape[:2]
    a, b, m, lengths, T = _case(rows, D, rs_of(rows, D))
    B = len(lengths)
    tv = float(m.sum())
    w = 0.75
    x = _t(a).view(B, T, D).requires_grad_(True)
    loss = O.masked_mse(x, _t(b).view(B, T, D), _t(m).view(B, T, 1))
    (w * loss).backward()
    diff = R.masked_diff(a, b, m)
    S = R.sq_sum(diff)
    ref = float(loss.detach())
    assert abs(S / tv - ref) <= (2 * U + U * U) * ref + rows * D * U64 * ref
    g = R.sqerr_grad(diff, m, w, F32(1.0) / F32(tv)).astype(np.float64)
    gref = x.grad.numpy().reshape(rows, D)
    assert (np.abs(g - gref) <= (4 * U + 7 * U * U) * np.abs(gref)).all()
    assert (g[m == 0] == 0).all()
    # the per-workgroup sums add up to the total
    for mb in (shape[2], 1, 7):
        nblk = R.red_blocks(rows * D, mb)
        Sb, cnt = R.block_sq_sums(diff, nblk)
        assert cnt.sum() == rows * D and abs(math.fsum(Sb) - S) <= nblk * U64 * S


def test_generator_losses_reference_is_the_oracles():
    """finalize_g_ref on the references' sums against update_generator (adv_w == 0 needs no discriminator) in float64; then the
    adversarial term's arithmetic against the oracle's expression."""
    rs = rs_of(7)
    rows, Do, Ds = 41 * 4, 11, 5
    B, T = R.mask_layout(rows)
    y_hat, y, m, lengths, _ = _case(rows, Do, rs)
    ys_hat, ys = rs.randn(rows, Ds).astype(np.float32), rs.randn(rows, Ds).astype(np.float32)
    tv = float(m.sum())
    mse_w, mge_w = 0.5, 0.75
    v3 = lambda a, d: _t(a).view(B, T, d)      # noqa: E731
    ref = O.update_generator(None, None, None, None, None, v3(y, Do), v3(y_hat, Do), v3(ys, Ds), v3(ys_hat, Ds), 0.0, lengths, _t(m).view(B, T, 1),
                             "eval", mse_w=mse_w, mge_w=mge_w)
    s_mse, s_mge = R.sq_sum(R.masked_diff(y_hat, y, m)), R.sq_sum(R.masked_diff(ys_hat, ys, m))
    sc = R.finalize_g_ref(s_mse, s_mge, float("nan"), tv, 0.0, mse_w, mge_w, 0)
    R.check_finalize_g(sc, s_mse, s_mge, 0.0, tv, 0.0, mse_w, mge_w, 0, None, True, "reference")
    for got, want in ((sc[17], ref[0]), (sc[18], ref[1]), (sc[19], float(ref[2])), (sc[20], ref[3])):
        assert abs(got - want) <= 6 * U * abs(want)       # 2 u of the squares, 2 of the loss, 2 of loss_g's product and sum
    # with the adversarial term: loss_adv = -s_adv / tv, loss_g = (mse_w mse + mge_w mge) + adv_w adv
    s_adv, adv_w = -431.25, 0.25
    sc = R.finalize_g_ref(s_mse, s_mge, s_adv, tv, adv_w, mse_w, mge_w, 1, gnorm2=50.0)
    R.check_finalize_g(sc, s_mse, s_mge, s_adv, tv, adv_w, mse_w, mge_w, 1, 50.0, False, "reference")
    want = (mse_w * ref[0] + mge_w * ref[1]) + adv_w * (-s_adv / tv)
    assert abs(sc[20] - want) <= 6 * U * (abs(mse_w * ref[0]) + abs(mge_w * ref[1]) + abs(adv_w * s_adv / tv))


def test_discriminator_losses_reference():
    """finalize_d_ref against update_discriminator's expressions: -sum / Tv each, their sum, the counts."""
    s_real, s_fake, tv = -812.25, -1033.5, 1531.0
    sc = R.finalize_d_ref(s_real, s_fake, 1201.0, 987.0, tv, gnorm2=330.0)
    R.check_finalize_d(sc, s_real, s_fake, 1201.0, 987.0, tv, 330.0, False, "reference")
    lr, lf = -s_real / tv, -s_fake / tv
    assert abs(sc[14] - lr) <= 2 * U * lr and abs(sc[13] - lf) <= 2 * U * lf and abs(sc[12] - (lr + lf)) <= 3 * U * (lr + lf)


def test_highway_reference_is_the_oracles():
    """x_static + T(x) G(x) of OracleIn2OutHighwayNet.forward in float64 against the reference on its float32 operands; the backward
    formulas against autograd of the same expression."""
    rs = rs_of(3)
    B, T, sd, nW = 2, 9, 3, 3
    model = O.cast_model(O.OracleIn2OutHighwayNet(in_dim=7, out_dim=sd * nW, static_dim=sd, num_hidden=1, hidden_dim=8, dropout=0.0, seed=1), torch.float64)
    model.training = False
    windows = [(0, 0, np.array([1.0])), (1, 1, np.array([-0.5, 0.0, 0.5])), (1, 1, np.array([1.0, -2.0, 1.0]))]
    Rm = torch.from_numpy(O.unit_variance_mlpg_matrix(windows, T)).double()
    x = _t(rs.randn(B, T, 7).astype(np.float32))
    h, out = model(x, Rm)
    xs = x[:, :, :sd]
    Tx = torch.sigmoid(torch.nn.functional.linear(xs, model.params[0], model.params[1]))
    Gx = O.unit_variance_mlpg(Rm, h)
    f = lambda t: t.detach().numpy().reshape(B * T, sd).astype(np.float32)      # noqa: E731
    x32, t32, g32 = f(xs), f(Tx), f(Gx)
    ref = out.detach().numpy().reshape(B * T, sd)
    plain = (x32 + (t32 * g32).astype(np.float32)).astype(np.float32)
    R.check_highway_fwd(plain, x32, t32, g32, "reference")
    # the float32 operands are roundings of the oracle's: u on x, 2 u on the product
    assert (np.abs(plain - ref) <= 2 * U * (np.abs(x32) + np.abs(t32 * g32)) + U * np.abs(x32) + 2 * U * np.abs(t32.astype(np.float64) * g32)).all()
    # backward: out = x + sigmoid(Tz) Gx
    Tz = _t(rs.randn(B * T, sd).astype(np.float32)).requires_grad_(True)
    G = _t(g32).requires_grad_(True)
    g = rs.randn(B * T, sd).astype(np.float32)
    (((_t(x32) + torch.sigmoid(Tz) * G) * _t(g)).sum()).backward()
    tx32 = torch.sigmoid(Tz).detach().numpy().astype(np.float32)
    dGx, dTz = R.highway_bwd(g, tx32, g32)
    # tx32 is a rounding of sigmoid (u; 1 - Tx adds u / (1 - Tx) relative), dGx one product, dTz three products and a difference
    assert (np.abs(dGx - G.grad.numpy()) <= 3 * U * np.abs(G.grad.numpy())).all()
    lim = (6 * U + 2 * U / (1.0 - tx32.astype(np.float64))) * np.abs(Tz.grad.numpy())
    assert (np.abs(dTz - Tz.grad.numpy()) <= lim).all()
    # sigmoid_grad is the same factor
    assert np.array_equal(R.sigmoid_grad(g, tx32), (g * (tx32 * (F32(1.0) - tx32)).astype(np.float32)).astype(np.float32))


def test_dropout_and_images_references():
    rs = rs_of(5)
    x = rs.randn(6, 5).astype(np.float32)
    keep = rs.rand(6, 5) > 0.3
    y = R.dropout_apply(x, keep, 0.3)
    assert np.array_equal(R.bits(y[~keep]), np.zeros((~keep).sum(), dtype=np.uint32))       # +0
    t = torch.from_numpy(x) * torch.from_numpy(keep.astype(np.float32)) / (1.0 - 0.3)       # the oracle's h * mask / (1 - p)
    assert (np.abs(y - t.numpy()) <= 2 * U * np.abs(t.numpy())).all()
    fa, fb = rs.randn(4, 9).astype(np.float32), rs.randn(4, 9).astype(np.float32)
    idx = np.asarray([8, 0, 3], dtype=np.int32)
    cat = R.build_cat2(x[:4], fa, fb, idx)
    want = torch.cat((torch.cat((torch.from_numpy(x[:4]), torch.from_numpy(fa)[:, idx.tolist()]), -1),
                      torch.cat((torch.from_numpy(x[:4]), torch.from_numpy(fb)[:, idx.tolist()]), -1)), 0).numpy()      # _adv_input, real over generated
    assert np.array_equal(cat, want)
    adv = R.build_adv(fa, fb, idx, 4, 8, 4)
    assert np.array_equal(adv[:, :3], want[:, 5:]) and (R.bits(adv[:, 3]) == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the restated grid-stride assignment
# ---------------------------------------------------------------------------------------------------------------------
def _all_red_cases():
    out = [(r, d, mb) for r, d, mb, _ in R.RED_SHAPES]
    for r, d1, d2, mb in R.G_LOSSES_SHAPES:
        out += [(r, d1, mb), (r, d2, mb)]
    return sorted(set(out))


@pytest.mark.parametrize("case", _all_red_cases(), ids=lambda c: "%dx%d-mb%d" % c)
def test_grid_stride_assignment_is_a_partition(case):
    """Walking every workgroup the way the kernels do visits every element exactly once, and in the workgroup block_of names."""
    rows, D, mb = case
    n = rows * D
    nblk = R.red_blocks(n, mb)
    owner = np.full(n, -1, dtype=np.int64)
    for blk in range(nblk):
        r, d = R.walk_block(rows, D, nblk, blk)
        assert (r >= 0).all() and (r < rows).all() and (d >= 0).all() and (d < D).all()
        e = r * D + d
        assert (owner[e] == -1).all() and len(np.unique(e)) == len(e), "workgroup %d revisits an element" % blk
        owner[e] = blk
    assert (owner >= 0).all(), "%d elements are never visited" % int((owner < 0).sum())
    assert np.array_equal(owner, R.block_of(n, nblk))


@pytest.mark.parametrize("four_valued", [False, True], ids=["mask01", "mask4"])
@pytest.mark.parametrize("case", _all_red_cases(), ids=lambda c: "%dx%d-mb%d" % c)
def test_last_trip_and_tail_loop_see_unmasked_elements(case, four_valued):
    """A dropped or misread element of the predicated last trip (masked_sqerr_body) or of the one-element tail loop (static_grad_kernel)
    shows only where the mask is not 0: every shape has unmasked elements there, whatever the seed, and its very last element is one."""
    rows, D, mb = case
    n = rows * D
    nblk = R.red_blocks(n, mb)
    for seed in range(4):
        m, _, _ = R.make_mask(rows, rs_of(rows, D, seed), four_valued)
        live = np.repeat(m > 0, D)
        assert live[-1]
        last, tail = R.last_trip(n, nblk), R.tail_loop(n, nblk)
        assert (live & last).any(), "the last trip is masked out"
        assert not tail.any() or (live & tail).any(), "the tail loop is masked out"
    if case == (1030, 1, 1):
        assert R.tail_loop(n, nblk).sum() == 6 and R.last_trip(n, nblk).sum() == 6
    if case == (41, 187, 3):
        assert R.last_trip(n, nblk).sum() == 7667 - 2 * 4 * 768 and R.tail_loop(n, nblk).sum() == 7667 - 2 * 4 * 768
    if case == (5700, 187, 0):
        assert R.last_trip(n, nblk).sum() == 5700 * 187 - 4 * 1024 * 256


def test_matrix_holds_what_the_issue_asks():
    splits = [(R.red_blocks(r * d1, mb), R.red_blocks(r * d2, mb)) for r, d1, d2, mb in R.G_LOSSES_SHAPES]
    assert (3, 1) in splits and (1, 3) in splits and (1024, 351) in splits
    assert {(d1, d2) for _, d1, d2, _ in R.G_LOSSES_SHAPES} == {(187, 63), (1, 300)}
    assert R.red_blocks(41 * 187, 3) == 3 and 41 * 187 == 7667 and R.red_blocks(5700 * 187) == 1024 and R.red_blocks(4100 * 63) == 253
    assert sorted(r * c for r, c in R.ELEMENT_SHAPES) == [1, 255, 257, 33 * 63]
    cover = R.sg_covering_set(12)
    assert len(cover) >= 12
    seen = set()
    for c in cover:
        seen |= R.sg_pairs(c)
    assert seen == R.sg_all_pairs()
    assert {c["rider"] for c in cover} == {"none", "hp", "nohp", "outnull"}
    inv = R.adv_map(187, 58, rs_of(1))
    j = inv[inv >= 0]
    assert (inv == -1).sum() == 187 - 58 and sorted(j) == list(range(58)) and not (np.diff(j) > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# the comparators catch seeded mistakes
# ---------------------------------------------------------------------------------------------------------------------
def _simulated(diff, nblk):
    """What a correct kernel reports: per-workgroup float64 sums in some order (numpy's pairwise sum), and their sum."""
    d = np.asarray(diff, dtype=np.float64).reshape(-1)
    blk = R.block_of(d.size, nblk)
    parts = np.asarray([(d[blk == k] ** 2).sum() for k in range(nblk)])
    return parts, float(parts.sum())


def test_comparator_catches_an_element_dropped_from_the_last_trip():
    rows, D, mb = 41, 187, 3
    a, b, m, _, _ = _case(rows, D, rs_of(rows, D))
    m[:] = 1.0
    diff = R.masked_diff(a, b, m)
    nblk = R.red_blocks(rows * D, mb)
    parts, total = _simulated(diff, nblk)
    R.check_partials(parts, diff, nblk, "correct")
    R.check_sum(total, R.sq_sum(diff), rows * D, "correct")
    # the reference loses the last valid element of workgroup 1's last trip
    r, d = R.walk_block(rows, D, nblk, 1, drop_last=True)
    lost = np.ones((rows, D), dtype=bool)
    for blk in range(nblk):
        rr, dd = (r, d) if blk == 1 else R.walk_block(rows, D, nblk, blk)
        lost[rr, dd] = False
    assert lost.sum() == 1
    wrong = np.where(lost, F32(0.0), diff)
    with pytest.raises(AssertionError):
        R.check_partials(parts, wrong, nblk, "dropped element")
    with pytest.raises(AssertionError):
        R.check_sum(total, R.sq_sum(wrong), rows * D, "dropped element")


def test_comparator_catches_two_elements_swapped_across_a_row_wrap():
    rows, D, mb = 64, 64, 4
    rs = rs_of(rows, D, 1)
    a, b = rs.randn(rows, D).astype(np.float32), rs.randn(rows, D).astype(np.float32)
    m = np.where(np.arange(rows) % 2 == 0, 1.0, 0.5).astype(np.float32)       # neighbouring rows differ in their mask
    diff = R.masked_diff(a, b, m)
    nblk = R.red_blocks(rows * D, mb)
    parts, _ = _simulated(diff, nblk)
    inv_tv = F32(1.0) / F32(m.sum())
    g = R.sqerr_grad(diff, m, 0.7, inv_tv)
    R.check_bits(g, R.sqerr_grad(diff, m, 0.7, inv_tv), "correct")
    r = 3        # elements (3, 63) and (4, 0): flat 255 and 256, the last of workgroup 0's first stride and the first of workgroup 1's
    assert list(R.block_of(rows * D, nblk)[[255, 256]]) == [0, 1]
    with pytest.raises(AssertionError):
        R.check_bits(g, R.swap_across_wrap(R.sqerr_grad(diff, m, 0.7, inv_tv), r), "swapped")
    with pytest.raises(AssertionError):
        R.check_partials(parts, R.swap_across_wrap(diff, r), nblk, "swapped")
    # the same through the operands: the two elements read each other's row (and mask)
    with pytest.raises(AssertionError):
        R.check_bits(g, R.sqerr_grad(R.masked_diff(R.swap_across_wrap(a, r), R.swap_across_wrap(b, r), m), m, 0.7, inv_tv), "swapped operands")


def test_comparator_catches_the_mask_applied_once():
    rows, D = 12, 7
    a, b, m, _, _ = _case(rows, D, rs_of(rows, D), four_valued=True)
    assert ((m > 0) & (m < 1)).any()
    diff = R.masked_diff(a, b, m)
    inv_tv = F32(1.0) / F32(5.0)
    g = R.sqerr_grad(diff, m, 0.7, inv_tv)
    with pytest.raises(AssertionError):
        R.check_bits(g, R.sqerr_grad(diff, m, 0.7, inv_tv, mask_once=True), "mask once")
    t0, p1, p2 = R.static_grad_terms(diff, m, 0.9, inv_tv, None, None, None, 0.3, 0)
    R.check_static_grad(t0.astype(np.float32), t0, p1, p2, "correct")
    once = R.sqerr_grad(diff, m, 0.9, inv_tv, mask_once=True)
    with pytest.raises(AssertionError):
        R.check_static_grad(t0.astype(np.float32), once.astype(np.float64), p1, p2, "mask once")
    # with {0, 1} masks the two are the same: why one case per kernel takes four values
    m01 = (m > 0).astype(np.float32)
    d01 = R.masked_diff(a, b, m01)
    R.check_bits(R.sqerr_grad(d01, m01, 0.7, inv_tv), R.sqerr_grad(d01, m01, 0.7, inv_tv, mask_once=True), "0 / 1 masks cannot tell")


def test_comparator_bounds_the_added_terms_of_static_grad():
    rows, Ds, Da = 9, 12, 5
    rs = rs_of(rows, Ds)
    a, b, m, _, _ = _case(rows, Ds, rs)
    diff = R.masked_diff(a, b, m)
    inv = R.adv_map(Ds, Da, rs)
    leak, gadv = rs.randn(rows, Da).astype(np.float32), rs.randn(rows, Da).astype(np.float32)
    inv_tv = F32(1.0) / F32(m.sum())
    t0, p1, p2 = R.static_grad_terms(diff, m, 0.9, inv_tv, inv, leak, gadv, 0.35, 1)
    assert (p1[:, inv < 0] == 0).all() and (p2[:, inv < 0] == 0).all() and (p1[:, inv >= 0] != 0).all()
    plain = ((t0.astype(np.float32) + p1.astype(np.float32)).astype(np.float32) + p2.astype(np.float32)).astype(np.float32)      # no contraction
    fused = (t0 + p1 + p2).astype(np.float32)                                                                                      # at most one rounding
    terms = np.broadcast_to(inv >= 0, t0.shape)            # the kernel adds nothing elsewhere (a -0 stays -0)
    plain, fused = np.where(terms, plain, t0.astype(np.float32)), np.where(terms, fused, t0.astype(np.float32))
    R.check_static_grad(plain, t0, p1, p2, "separate roundings")
    R.check_static_grad(fused, t0, p1, p2, "contracted")
    for wrong in (t0 + p1, t0 + p2, t0 + p1 + 1.001 * p2):       # a lost term, a weight off by 1e-3
        with pytest.raises(AssertionError):
            R.check_static_grad(wrong.astype(np.float32), t0, p1, p2, "wrong")
    leaked = plain.copy()
    c0 = int(np.nonzero(inv < 0)[0][0])
    leaked[0, c0] = np.nextafter(leaked[0, c0], F32(np.inf)) if leaked[0, c0] != 0 else F32(1e-30)
    with pytest.raises(AssertionError):
        R.check_static_grad(leaked, t0, p1, p2, "a column without added terms is not bit for bit")


def test_comparator_catches_a_lost_last_partial():
    rows, D = 64, 64
    a, b, m, _, _ = _case(rows, D, rs_of(rows, D))
    m[-1] = 1.0
    diff = R.masked_diff(a, b, m)
    nblk = 4
    parts, total = _simulated(diff, nblk)
    R.check_sum(total, R.sq_sum(diff), rows * D, "correct")
    assert parts[-1] > 0
    with pytest.raises(AssertionError):
        R.check_sum(float(parts[:-1].sum()), R.sq_sum(diff), rows * D, "lost partial")
    with pytest.raises(AssertionError):
        R.check_partials(parts[:-1], diff, nblk, "lost partial")
    with pytest.raises(AssertionError):
        R.check_fsum(float(parts[:-1].sum()), parts, "lost partial")
    R.check_fsum(total, parts, "correct")


def test_comparator_catches_a_pad_column_written():
    host = np.full(40, R.SENT, dtype=np.float32)
    inside = np.zeros(40, dtype=bool)
    view = lambda f: f[8:8 + 4 * 6].reshape(4, 6)[:, :5]      # noqa: E731: [4][5] at pitch 6
    view(inside)[...] = True
    flat = host.copy()
    view(flat)[...] = 1.0
    R.check_guard(flat, host, inside, "correct")
    for at in (8 + 5, 7, 8 + 4 * 6):        # a pad column, the element in front, the row behind
        bad = flat.copy()
        bad[at] = 0.0
        with pytest.raises(AssertionError):
            R.check_guard(bad, host, inside, "written outside")
    same_value = flat.copy()
    same_value[8 + 5] = np.float32(-7.25e33) * np.float32(1.0000001)       # one ulp off the sentinel
    with pytest.raises(AssertionError):
        R.check_guard(same_value, host, inside, "one ulp off the sentinel")
    # a pad column the kernel owns must be +0: -0 and a tiny value fail the bit comparison
    ref = R.pad_cols(np.ones((2, 3), dtype=np.float32), 4)
    for v in (-0.0, 1e-45):
        got = ref.copy()
        got[1, 3] = v
        with pytest.raises(AssertionError):
            R.check_bits(got, ref, "pad column")


@pytest.mark.parametrize("aligned", [True, False], ids=["16byte", "4byte"])
@pytest.mark.parametrize("threads", [1024, 256])
def test_mask_sum_walk_reads_every_element_once(threads, aligned):
    """The restated walk of mask_total_body -- both alignment paths, the 8-deep loops and both tails -- is a partition of every n of the
    matrix, and its sum is the mask's."""
    for n in (R.MASK_N if threads == 1024 else R.MASK_N_RIDER):
        assert (R.mask_total_visits(n, threads, aligned) == 1).all(), n
        m = (rs_of(n).rand(n) < 0.6).astype(np.float32)
        assert R.mask_total_ref(m, threads, aligned) == float(m.astype(np.float64).sum())


def test_comparator_catches_a_count_off_by_one_in_the_tail():
    for n, threads in [(v, 1024) for v in R.MASK_N] + [(v, 256) for v in R.MASK_N_RIDER]:
        m = np.ones(n, dtype=np.float32)
        inv = float(F32(1.0) / F32(n))
        for aligned in (True, False):
            R.check_tv(R.mask_total_ref(m, threads, aligned), inv, m, what="correct")
            short = R.mask_total_ref(m, threads, aligned, tail_short=1)
            if short != n:       # the last element is read by a 4-byte loop: always, but for a whole number of 16-byte groups
                with pytest.raises(AssertionError):
                    R.check_tv(short, inv, m, what="tail one short")
            assert short != n or (aligned and n % 4 == 0)
    with pytest.raises(AssertionError):
        R.check_tv(5.0, float(np.nextafter(F32(0.2), F32(1.0))), np.ones(5), what="inv_tv one ulp off")


def test_comparators_of_the_finalisation_catch_a_wrong_rounding():
    tv = 1237.0
    sc = R.finalize_g_ref(5000.0, 3000.0, -411.5, tv, 0.35, 0.6, 0.9, 1, gnorm2=77.0)
    R.check_finalize_g(sc, 5000.0, 3000.0, -411.5, tv, 0.35, 0.6, 0.9, 1, 77.0, False, "correct")
    for i in (17, 18, 19, 20, 22):
        bad = sc.copy()
        bad[i] *= 1 + 8 * U
        with pytest.raises(AssertionError):
            R.check_finalize_g(bad, 5000.0, 3000.0, -411.5, tv, 0.35, 0.6, 0.9, 1, 77.0, False, "off")
    bad = sc.copy()
    bad[19] = -bad[19]         # the sign of the adversarial term
    with pytest.raises(AssertionError):
        R.check_finalize_g(bad, 5000.0, 3000.0, -411.5, tv, 0.35, 0.6, 0.9, 1, 77.0, False, "sign")
    with pytest.raises(AssertionError):
        R.check_finalize_g(sc, 5000.0, 3000.0, -411.5, tv, 0.35, 0.6, 0.9, 0, 77.0, False, "has_adv == 0 must report 0")
    with pytest.raises(AssertionError):
        R.check_finalize_g(sc, 5000.0, 3000.0, -411.5, tv, 0.35, 0.6, 0.9, 1, 77.0, True, "zero_gnorm must report 0")
    d = R.finalize_d_ref(-812.25, -1033.5, 1201.0, 987.0, 1531.0, gnorm2=330.0)
    for i in (12, 13, 14, 21):
        bad = d.copy()
        bad[i] *= 1 + 8 * U
        with pytest.raises(AssertionError):
            R.check_finalize_d(bad, -812.25, -1033.5, 1201.0, 987.0, 1531.0, 330.0, False, "off")
    bad = d.copy()
    bad[15] += 1
    with pytest.raises(AssertionError):
        R.check_finalize_d(bad, -812.25, -1033.5, 1201.0, 987.0, 1531.0, 330.0, False, "count")
    bad = d.copy()
    bad[13], bad[14] = bad[14], bad[13]      # real and fake exchanged
    with pytest.raises(AssertionError):
        R.check_finalize_d(bad, -812.25, -1033.5, 1201.0, 987.0, 1531.0, 330.0, False, "exchanged")


def test_comparator_of_the_highway_combine_and_dropout():
    rs = rs_of(9)
    x, t, g = (rs.randn(5, 7).astype(np.float32) for _ in range(3))
    plain = (x + (t * g).astype(np.float32)).astype(np.float32)
    fused = (x.astype(np.float64) + t.astype(np.float64) * g).astype(np.float32)
    R.check_highway_fwd(plain, x, t, g, "separate roundings")
    R.check_highway_fwd(fused, x, t, g, "contracted")
    with pytest.raises(AssertionError):
        R.check_highway_fwd((x + t).astype(np.float32), x, t, g, "wrong")
    with pytest.raises(AssertionError):
        R.check_highway_fwd(plain * F32(1 + 1e-5), x, t, g, "off")
    keep = rs.rand(5, 7) > 0.3
    y = R.dropout_apply(x, keep, 0.3)
    neg = y.copy()
    neg[~keep] = -0.0
    with pytest.raises(AssertionError):
        R.check_bits(neg, y, "-0 where dropped")
