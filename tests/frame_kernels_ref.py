"""numpy references, shapes and comparators of the per-frame kernels (frame_kernels.hip.h) that tests/test_gpu_frame_kernels.py runs
through gt_op_frame.  Nothing here needs a GPU: tests/test_frame_kernels_host.py holds these references against oracle/ and shows that
the comparators catch seeded mistakes.

All references work on the float32 operands the kernel reads.  u = 2^-24 is the unit roundoff of float32, 2^-53 that of float64.
"""
import itertools
import math

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
F32 = np.float32
RED_THREADS = 256
MAX_BLOCKS = 1024
SENT = np.float32(-7.25e33)       # what surrounds every result


def cdiv(a, b):
    return (a + b - 1) // b


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------
# shapes (the issue's matrix)
# ---------------------------------------------------------------------------------------------------------------------
# (rows, D, max_blocks, what it exercises); max_blocks 0: the engine's 1024
RED_SHAPES = [
    (1, 1, 0, "total of 1"),
    (3, 7, 0, "one partly filled workgroup"),
    (41, 187, 3, "stride 768 coprime with D: two full trips, a last trip with two valid strides of four"),
    (64, 64, 4, "stride a whole number of rows, column step 0"),
    (16, 256, 1, "D equal to the stride"),
    (5, 300, 1, "D larger than the stride, row step 0"),
    (1030, 1, 1, "one full trip, then a 6-element tail"),
    (4100, 63, 0, "the engine's grid, every thread at most four elements"),
    (5700, 187, 0, "just past the 1024-workgroup cap, a second trip for few threads"),
]
# g_losses: (rows, D1, D2, max_blocks) -> the block split (n1, n2)
G_LOSSES_SHAPES = [
    (12, 187, 63, 3),        # (3, 1)
    (8, 1, 300, 3),          # (1, 3)
    (41, 187, 63, 0),        # the engine's own: (8, 3)
    (5700, 187, 63, 0),      # the engine's own at the cap: (1024, 351)
    (1030, 1, 300, 2),       # (2, 2): D larger than the first stride, a tail in the second
]
MASK_N = [1, 3, 4, 5, 1023, 7169, 28677, 32771, 36869]
MASK_N_RIDER = [5, 7173, 9221]
BUILD_ADV_NA = [1, 58, 61, 256, 260]
BUILD_ADV_N = [1, 37, 300]
BUILD_CAT2 = [(5, 3, 7), (425, 58, 33)]
TRANSPOSE_DIMS = [1, 31, 32, 33, 70]
COPY_COLS = [1, 425, 428]
ELEMENT_SHAPES = [(1, 1), (5, 51), (1, 257), (33, 63)]      # rows * cols in {1, 255, 257, 33 * 63}


def red_blocks(n, max_blocks=0):
    """Workgroups (= partials) of a masked reduction over n elements (frame_args.hip.h: frame_red_blocks)."""
    return min(max_blocks or MAX_BLOCKS, cdiv(n, RED_THREADS * 4))


# ---------------------------------------------------------------------------------------------------------------------
# the grid-stride assignment restated
# ---------------------------------------------------------------------------------------------------------------------
def block_of(n, nblk):
    """Workgroup of every flat element e = row * D + col: element e is visited by thread (e mod stride), stride = nblk * 256."""
    e = np.arange(n, dtype=np.int64)
    return (e % (nblk * RED_THREADS)) // RED_THREADS


def walk_block(rows, D, nblk, blk, drop_last=False):
    """The (row, col) pairs workgroup `blk` visits, by the walk the kernels make: every thread starts at e = blk * 256 + tid, holds
    (row, col) = divmod(e, D) and advances both by divmod(stride, D) with one wrap of the column, four strides per trip, the strides past
    the end switched off (masked_sqerr_body; static_grad_kernel visits the same elements with a one-element tail loop).
    drop_last (a seeded mistake for the host tests): the last valid element of the last trip is lost."""
    total = rows * D
    stride = nblk * RED_THREADS
    sr, sd = divmod(stride, D)
    e = blk * RED_THREADS + np.arange(RED_THREADS, dtype=np.int64)
    r, d = np.divmod(e, D)
    out_r, out_d = [], []
    while (e < total).any():
        for u in range(4):
            ok = e + u * stride < total
            out_r.append(r[ok])
            out_d.append(d[ok])
            r = r + sr
            d = d + sd
            wrap = d >= D
            d = np.where(wrap, d - D, d)
            r = np.where(wrap, r + 1, r)
        e = e + 4 * stride
    rr = np.concatenate(out_r) if out_r else np.zeros(0, np.int64)
    dd = np.concatenate(out_d) if out_d else np.zeros(0, np.int64)
    if drop_last and len(rr):
        rr, dd = rr[:-1], dd[:-1]
    return rr, dd


def last_trip(n, nblk):
    """[n] bool: the elements of the LAST trip of the four-stride loop (trip of element e: (e div stride) div 4)."""
    trip = (np.arange(n, dtype=np.int64) // (nblk * RED_THREADS)) // 4
    return trip == trip[-1]


def tail_loop(n, nblk):
    """[n] bool: the elements static_grad_kernel's one-element tail loop visits: thread t = e mod stride walks n_t elements, the first
    4 (n_t div 4) of them in the four-stride loop."""
    stride = nblk * RED_THREADS
    e = np.arange(n, dtype=np.int64)
    k, t = e // stride, e % stride
    n_t = (n - t + stride - 1) // stride
    return k >= 4 * (n_t // 4)


def swap_across_wrap(a, r):
    """A seeded mistake for the host tests: the last element of row r and the first of row r + 1 trade places."""
    a = np.array(a, copy=True)
    a[r, -1], a[r + 1, 0] = a[r + 1, 0], a[r, -1]
    return a


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------
def mask_layout(rows):
    """(B, T) with B * T == rows: the smallest B >= 3 that divides rows, else rows sequences of one frame."""
    for B in range(3, rows + 1):
        if rows % B == 0:
            return B, rows // B
    return rows, 1


def make_lengths(rows, rs):
    """Lengths of the B sequences: 0 and 1 lead, random ones in [0, T] follow, and the LAST sequence has all T frames -- the last rows are
    where a reduction's last trip and tail loop run, so they must not be masked out."""
    B, T = mask_layout(rows)
    lengths = ([0, 1] + [int(v) for v in rs.randint(0, T + 1, size=max(0, B - 3))])[:B - 1] + [T]
    return np.asarray(lengths, dtype=np.int64), T


def sequence_mask(lengths, T):
    return (np.arange(T)[None, :] < np.asarray(lengths)[:, None]).astype(np.float32)


def make_mask(rows, rs, four_valued=False):
    """[rows] float32 in {0, 1} from lengths that include 0, 1 and T; four_valued: the valid frames take values in {0.25, 0.5, 1}."""
    lengths, T = make_lengths(rows, rs)
    m = sequence_mask(lengths, T).reshape(-1)
    if four_valued:
        m = m * rs.choice(np.asarray([0.25, 0.5, 1.0], dtype=np.float32), size=rows)
    return m.astype(np.float32), lengths, T


# ---------------------------------------------------------------------------------------------------------------------
# sums of squares and their gradients
# ---------------------------------------------------------------------------------------------------------------------
def masked_diff(a, b, m):
    """float32(a m - b m), [rows][D].  With m a power of two (or 0) both products are exact, so the value is the same whether the
    kernel's a*m - b*m is contracted to an fma or not; its square is exact in float64."""
    m = np.asarray(m, dtype=np.float32)[:, None]
    return (np.asarray(a, dtype=np.float32) * m - np.asarray(b, dtype=np.float32) * m).astype(np.float32)


def sq_sum(diff):
    """S = sum(float64(diff)^2), exactly rounded (math.fsum)."""
    d = np.asarray(diff, dtype=np.float64).reshape(-1)
    return math.fsum((d * d).tolist())


def block_sq_sums(diff, nblk):
    """Per-workgroup S and element counts, by the restated assignment."""
    d = np.asarray(diff, dtype=np.float64).reshape(-1)
    blk = block_of(d.size, nblk)
    order = np.argsort(blk, kind="stable")
    cnt = np.bincount(blk, minlength=nblk)
    sq = (d * d)[order]
    ends = np.cumsum(cnt)
    S = np.asarray([math.fsum(sq[e - c:e].tolist()) for c, e in zip(cnt, ends)])
    return S, cnt


def check_sum(got, S, n, what):
    """A float64 sum of n exact squares in ANY order: |got - S| <= n 2^-53 S."""
    assert np.isfinite(got), "%s: %r" % (what, got)
    assert abs(got - S) <= n * U64 * S, "%s: got %.17g, sum %.17g, off by %.3g of the bound" % (
        what, got, S, abs(got - S) / max(n * U64 * S, 1e-300))


def check_partials(got, diff, nblk, what):
    """Every partial against the squares of ITS workgroup's elements; one partial per workgroup."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (nblk,), "%s: %d partials for %d workgroups" % (what, got.size, nblk)
    S, cnt = block_sq_sums(diff, nblk)
    for k in range(nblk):
        check_sum(got[k], S[k], int(cnt[k]), "%s partial %d" % (what, k))


def grad_scale(w, inv_tv):
    """gs = float32(float32(2 w) inv_tv): the scalar in front of the masked-MSE gradient."""
    return F32(F32(F32(2.0) * F32(w)) * F32(inv_tv))


def sqerr_grad(diff, m, w, inv_tv, mask_once=False):
    """float32(float32(gs diff) m).  mask_once (seeded mistake): the mask already in diff is the only one."""
    g = (grad_scale(w, inv_tv) * np.asarray(diff, dtype=np.float32)).astype(np.float32)
    if mask_once:
        return g
    return (g * np.asarray(m, dtype=np.float32)[:, None]).astype(np.float32)


def check_bits(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    assert got.shape == ref.shape, "%s: shape %s != %s" % (what, got.shape, ref.shape)
    bad = bits(got) != bits(ref)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, reference %r" % (what, int(bad.sum()), bad.size, i, got[i], ref[i]))


def static_grad_terms(diff, m, mge_w, inv_tv, adv_inv, leak, gadv, adv_w, leak_unnorm):
    """The three terms of the assembled gradient in float64: t0 = float32(float32(sc2 diff) m) (no contractible expression), p1 = leak_s
    leak[:, j], p2 = adv_w gadv[:, j] for j = adv_inv[c] >= 0, zero elsewhere and for a missing operand."""
    t0 = sqerr_grad(diff, m, mge_w, inv_tv).astype(np.float64)
    p1, p2 = np.zeros_like(t0), np.zeros_like(t0)
    if adv_inv is not None:
        cols = np.nonzero(np.asarray(adv_inv) >= 0)[0]
        j = np.asarray(adv_inv)[cols]
        if leak is not None:
            leak_s = float(F32(inv_tv)) if leak_unnorm else 1.0
            p1[:, cols] = leak_s * np.asarray(leak, dtype=np.float64)[:, j]
        if gadv is not None:
            p2[:, cols] = float(F32(adv_w)) * np.asarray(gadv, dtype=np.float64)[:, j]
    return t0, p1, p2


def check_static_grad(got, t0, p1, p2, what):
    """Without added terms bit for bit t0; with them each may or may not be contracted: |got - (t0 + p1 + p2)| <= 4 u (|t0| + |p1| + |p2|)
    (three roundings plus second-order terms)."""
    got = np.asarray(got, dtype=np.float32)
    plain = (p1 == 0) & (p2 == 0)
    check_bits(np.where(plain, got, 0), np.where(plain, t0.astype(np.float32), 0), what + " (columns without added terms)")
    err = np.abs(got.astype(np.float64) - (t0 + p1 + p2))
    bound = 4 * U * (np.abs(t0) + np.abs(p1) + np.abs(p2))
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d elements beyond 4u, worst %.3g of the bound" % (what, int(bad.sum()), float((err / np.maximum(bound, 1e-300)).max()))


# ---------------------------------------------------------------------------------------------------------------------
# the valid-frame count and the finalisation
# ---------------------------------------------------------------------------------------------------------------------
def check_tv(tv, inv_tv, mask=None, expect=None, what="tv"):
    """tv exactly the sum of the mask (or `expect`), inv_tv within one rounding of 1 / tv."""
    want = float(np.asarray(mask, dtype=np.float64).sum()) if expect is None else float(expect)
    assert tv == want, "%s: tv %r, the mask sums to %r" % (what, tv, want)
    if want > 0:
        assert abs(inv_tv - 1.0 / want) <= U / want, "%s: inv_tv %r is not 1 / %r to one rounding" % (what, inv_tv, want)
        assert float(F32(inv_tv)) == inv_tv


def check_loss(got, s, tv, what, negate=False):
    """float32(s) / tv: two roundings."""
    exact = (-s if negate else s) / tv
    assert abs(got - exact) <= (2 * U + U * U) * abs(exact), "%s: got %r for %r" % (what, got, exact)


def check_fsum(got, parts, what):
    """A float64 sum of the doubles `parts` in any order: |got - sum| <= n 2^-53 sum|p|."""
    p = [float(v) for v in parts]
    assert abs(got - math.fsum(p)) <= len(p) * U64 * math.fsum(abs(v) for v in p), "%s: got %r, sum %r" % (what, got, math.fsum(p))


def check_finalize_g(sc, s_mse, s_mge, s_adv, tv, adv_w, mse_w, mge_w, has_adv, gnorm2, zero_gnorm, what):
    """`sc`: the 26 doubles gt_op_frame reports.  Losses float32(sum) / tv; loss_g within 4 u of the three weighted terms; gnorm_g within
    2 u of sqrt (exactly 0 with zero_gnorm); has_adv == 0 gives loss_adv == 0."""
    mse, mge, adv, lg, gn, rtv = sc[17], sc[18], sc[19], sc[20], sc[22], sc[23]
    check_loss(mse, s_mse, tv, what + " loss_mse")
    check_loss(mge, s_mge, tv, what + " loss_mge")
    if has_adv:
        check_loss(adv, s_adv, tv, what + " loss_adv", negate=True)
    else:
        assert adv == 0.0, "%s: loss_adv %r without an adversarial term" % (what, adv)
    t = [float(F32(mse_w)) * mse, float(F32(mge_w)) * mge, float(F32(adv_w)) * adv]
    assert abs(lg - sum(t)) <= 4 * U * sum(abs(v) for v in t), "%s: loss_g %r for %r" % (what, lg, sum(t))
    if zero_gnorm:
        assert gn == 0.0, "%s: gnorm_g %r with zero_gnorm" % (what, gn)
    else:
        assert abs(gn - math.sqrt(gnorm2)) <= 2 * U * math.sqrt(gnorm2), "%s: gnorm_g %r for sqrt(%r)" % (what, gn, gnorm2)
    assert rtv == tv, "%s: reported tv %r != %r" % (what, rtv, tv)
    assert all(np.isnan(sc[i]) for i in (12, 13, 14, 15, 16, 21)), "%s: the generator finalisation wrote a discriminator result" % what


def check_finalize_d(sc, s_real, s_fake, n_real_ok, n_fake_ok, tv, gnorm2, zero_gnorm, what):
    ld, lf, lr, rc, fc, gn, rtv = sc[12], sc[13], sc[14], sc[15], sc[16], sc[21], sc[23]
    check_loss(lr, s_real, tv, what + " loss_real_d", negate=True)
    check_loss(lf, s_fake, tv, what + " loss_fake_d", negate=True)
    assert abs(ld - (lr + lf)) <= U * abs(lr + lf), "%s: loss_d %r for %r + %r" % (what, ld, lr, lf)
    assert rc == n_real_ok and fc == n_fake_ok, "%s: correct counts %r, %r for %r, %r" % (what, rc, fc, n_real_ok, n_fake_ok)
    if zero_gnorm:
        assert gn == 0.0, "%s: gnorm_d %r with zero_gnorm" % (what, gn)
    else:
        assert abs(gn - math.sqrt(gnorm2)) <= 2 * U * math.sqrt(gnorm2), "%s: gnorm_d %r for sqrt(%r)" % (what, gn, gnorm2)
    assert rtv == tv, "%s: reported tv %r != %r" % (what, rtv, tv)
    assert all(np.isnan(sc[i]) for i in (17, 18, 19, 20, 22)), "%s: the discriminator finalisation wrote a generator result" % what


# ---------------------------------------------------------------------------------------------------------------------
# element kernels (float32, the kernel's own association)
# ---------------------------------------------------------------------------------------------------------------------
def highway_bwd(g, Tx, Gx):
    """dGx = g Tx; dTz = (g Gx) ((1 - Tx) Tx)."""
    g, Tx, Gx = (np.asarray(v, dtype=np.float32) for v in (g, Tx, Gx))
    return (g * Tx).astype(np.float32), ((g * Gx).astype(np.float32) * ((F32(1.0) - Tx).astype(np.float32) * Tx).astype(np.float32)).astype(np.float32)


def sigmoid_grad(g, y):
    """g (y (1 - y))."""
    g, y = np.asarray(g, dtype=np.float32), np.asarray(y, dtype=np.float32)
    return (g * (y * (F32(1.0) - y).astype(np.float32)).astype(np.float32)).astype(np.float32)


def scale_inv_tv(g, inv_tv):
    return (np.asarray(g, dtype=np.float32) * F32(inv_tv)).astype(np.float32)


def check_highway_fwd(got, x, Tx, Gx, what):
    """x + Tx Gx, contracted or not: within 2 u (|x| + |Tx Gx|)."""
    x, Tx, Gx = (np.asarray(v, dtype=np.float64) for v in (x, Tx, Gx))
    err = np.abs(np.asarray(got, dtype=np.float64) - (x + Tx * Gx))
    bound = 2 * U * (np.abs(x) + np.abs(Tx * Gx))
    assert (err <= bound).all(), "%s: worst %.3g of the bound" % (what, float((err / np.maximum(bound, 1e-300)).max()))


def dropout_scale(p):
    return F32(1.0) / (F32(1.0) - F32(p))


def dropout_apply(x, keep, p):
    """x scale where kept, +0 where dropped."""
    x = np.asarray(x, dtype=np.float32)
    return np.where(keep, (x * dropout_scale(p)).astype(np.float32), F32(0.0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# image builders
# ---------------------------------------------------------------------------------------------------------------------
def build_adv(fa, fb, idx, split, rows, ldo):
    """[rows][ldo]: rows below split from fa, the rest from fb (row r - split), columns idx; pad columns +0."""
    out = np.zeros((rows, ldo), dtype=np.float32)
    idx = np.asarray(idx)
    if split > 0:
        out[:split, :len(idx)] = fa[:split][:, idx]
    if split < rows:
        out[split:, :len(idx)] = fb[:rows - split][:, idx]
    return out


def build_cat2(x, fa, fb, idx):
    """[2 N][cd + na]: [x | fa[:, idx]] over [x | fb[:, idx]]."""
    idx = np.asarray(idx)
    return np.concatenate([np.concatenate([x, fa[:, idx]], axis=1), np.concatenate([x, fb[:, idx]], axis=1)], axis=0).astype(np.float32)


def pad_cols(a, ldo):
    out = np.zeros((a.shape[0], ldo), dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


def check_guard(flat, host, inside, what):
    """Everything outside the result (the boolean `inside` marks it) still holds what the host put there, bit for bit."""
    a, b = np.asarray(flat)[~inside], np.asarray(host)[~inside]
    assert np.array_equal(bits(a), bits(b)), "%s: written outside the result" % what


# ---------------------------------------------------------------------------------------------------------------------
# the covering set of static_grad's optional operands
# ---------------------------------------------------------------------------------------------------------------------
SG_FACTORS = [("gs", (0, 1)), ("partial", (0, 1)), ("adv_inv", (0, 1)), ("leak", (0, 1)), ("gadv", (0, 1)), ("leak_unnorm", (0, 1)),
              ("rider", ("none", "hp", "nohp", "outnull"))]


def sg_pairs(case):
    items = [(k, case[k]) for k, _ in SG_FACTORS]
    return set(itertools.combinations(items, 2))


def sg_all_pairs():
    out = set()
    for (ka, va), (kb, vb) in itertools.combinations(SG_FACTORS, 2):
        out |= {((ka, a), (kb, b)) for a in va for b in vb}
    return out


def sg_covering_set(minimum=12):
    """Greedy pairwise cover of SG_FACTORS (deterministic): every pair of settings occurs together at least once; at least `minimum`
    cases (further ones are the combinations that differ most from those chosen)."""
    combos = [dict(zip([k for k, _ in SG_FACTORS], v)) for v in itertools.product(*[vals for _, vals in SG_FACTORS])]
    need, chosen = sg_all_pairs(), []
    while need or len(chosen) < minimum:
        def gain(c):
            return (len(sg_pairs(c) & need), sum(sum(c[k] != d[k] for k in c) for d in chosen))
        best = max((c for c in combos if c not in chosen), key=gain)
        chosen.append(best)
        need -= sg_pairs(best)
    return chosen


def adv_map(Ds, Da, rs):
    """adv_inv [Ds] -> j or -1: a non-monotone map onto all of [0, Da), -1 elsewhere."""
    assert Da <= Ds
    inv = np.full(Ds, -1, dtype=np.int32)
    cols = np.sort(rs.choice(Ds, size=Da, replace=False))
    inv[cols] = rs.permutation(Da).astype(np.int32)
    if Da > 1 and (np.diff(inv[cols]) > 0).all():
        inv[cols[0]], inv[cols[1]] = inv[cols[1]], inv[cols[0]]
    return inv


# ---------------------------------------------------------------------------------------------------------------------
# the finalisation restated in float32 (what the host tests hold against oracle/ and feed to the comparators)
# ---------------------------------------------------------------------------------------------------------------------
def finalize_g_ref(s_mse, s_mge, s_adv, tv, adv_w, mse_w, mge_w, has_adv, gnorm2=None):
    """The 26 doubles gt_op_frame would report after a generator finalisation on these sums (NaN where nothing is written)."""
    sc = np.full(26, np.nan)
    T = F32(tv)
    mse, mge = F32(s_mse) / T, F32(s_mge) / T
    adv = -F32(s_adv) / T if has_adv else F32(0.0)
    lg = (F32(mse_w) * mse + F32(mge_w) * mge) + F32(adv_w) * adv
    sc[0], sc[1] = float(T), float(F32(1.0) / T)
    sc[7], sc[8], sc[9] = s_adv, s_mge, s_mse
    sc[17], sc[18], sc[19], sc[20] = float(mse), float(mge), float(adv), float(lg)
    sc[22] = 0.0 if gnorm2 is None else float(F32(math.sqrt(gnorm2)))
    sc[23] = float(T)
    return sc


def finalize_d_ref(s_real, s_fake, n_real_ok, n_fake_ok, tv, gnorm2=None):
    sc = np.full(26, np.nan)
    T = F32(tv)
    lr, lf = -F32(s_real) / T, -F32(s_fake) / T
    sc[0], sc[1] = float(T), float(F32(1.0) / T)
    sc[12], sc[13], sc[14] = float(lr + lf), float(lf), float(lr)
    sc[15], sc[16] = float(F32(n_real_ok)), float(F32(n_fake_ok))
    sc[21] = 0.0 if gnorm2 is None else float(F32(math.sqrt(gnorm2)))
    sc[23] = float(T)
    return sc


def mask_total_visits(n, threads=1024, aligned=True, tail_short=0):
    """How often mask_total_body reads each of the n elements (all ones for a correct walk).  aligned: 16-byte groups j = tid, tid + bd, ...
    below n4 = n div 4, eight per round trip while j + 7 bd < n4 and singly after that, then the tail elements 4 n4 + tid, ...; else (and
    for that tail) 4-byte elements i, eight per round trip while i + 7 bd < n and singly after that.
    tail_short (a seeded mistake for the host tests): the 4-byte loops stop that many elements before n."""
    seen = np.zeros(n, dtype=np.int64)
    bd = threads
    for tid in range(bd):
        i = tid
        if aligned:
            n4 = n >> 2
            j = tid
            while j + 7 * bd < n4:
                for u in range(8):
                    seen[4 * (j + u * bd):4 * (j + u * bd) + 4] += 1
                j += 8 * bd
            while j < n4:
                seen[4 * j:4 * j + 4] += 1
                j += bd
            i = 4 * n4 + tid
        end = n - tail_short
        while i + 7 * bd < end:
            for u in range(8):
                seen[i + u * bd] += 1
            i += 8 * bd
        while i < end:
            seen[i] += 1
            i += bd
    return seen


def mask_total_ref(mask, threads=1024, aligned=True, tail_short=0):
    """sum(mask) by the walk of mask_total_body: every element times the number of times the walk reads it."""
    m = np.asarray(mask, dtype=np.float64)
    return float((m * mask_total_visits(m.size, threads, aligned, tail_short)).sum())
