"""The per-frame kernels between the products of a G+D step (frame_kernels.hip.h) against float64, one launch at a time.

gt_op_frame runs ONE launch function of frame_args.hip.h -- the functions eng_step.hip, eng_comm.hip, eng_lstm.hip and eng_sru.hip call --
on the test's own buffers.  Every case fills the pitch padding of every input with NaN, pre-fills every result with NaN (random values
where the op works in place), surrounds every result (and fills every pad column the kernel does not own) with a sentinel that is
compared bit for bit afterwards, and runs twice: the kernels claim a fixed order, so the two runs must agree bit for bit.  The references
and comparators are numpy on the same float32 operands (tests/frame_kernels_ref.py; tests/test_frame_kernels_host.py holds them against
oracle/ and shows that they catch seeded mistakes).  No tolerance here is measured: u = 2^-24, and every bound is counted in roundings.

Which case reaches which kernel:

| test                                   | kernels                                                                                     |
|----------------------------------------|---------------------------------------------------------------------------------------------|
| test_mask_sum_and_total                | mask_sum_kernel, mask_total_kernel (1024 threads; 16-byte and 4-byte paths, both tails)      |
| test_mask_sum_normaliser_sources       | mask_sum_kernel with tv_override > 0 and with tv_dev                                        |
| test_build_adv (rider 1, 2)            | build_adv_kernel + mask_sum_body / mask_total_body at 256 threads (the `sc` / `tv_total` rider) |
| test_build_adv (rider 0)               | build_adv_kernel: LDS map (na <= 256) and memory map (na = 260), both halves / generated alone |
| test_sqerr, test_sqerr_four_valued_mask| masked_sqerr_kernel with and without the gradient, sum_partials_kernel                      |
| test_g_losses                          | g_losses_kernel, sum_partials_kernel                                                        |
| test_static_grad_shapes                | static_grad_kernel: four-stride loop and one-element tail over the shape matrix             |
| test_static_grad_operands              | static_grad_kernel: every optional operand pairwise, the GFinalize rider (hp, no hp, out == null) |
| test_finalize_g_forms                  | finalize_g_kernel at 256 threads (partials) and 1 thread, finalize_g_rider_kernel, static_grad's rider |
| test_finalize_g_rider_hp_and_gnorm     | finalize_g_rider_kernel with hp; finalize_g_kernel with the gradient norm                   |
| test_finalize_d                        | finalize_d_kernel with and without tv_from_sum, with and without zero_gnorm                 |
| test_element_kernels                   | scale_by_inv_tv_kernel, highway_forward_kernel, highway_backward_kernel, sigmoid_grad_kernel |
| test_dropout_apply                     | dropout_apply_kernel: buffer and Philox site, in == out                                     |
| test_build_cat2                        | build_cat2_kernel                                                                           |
| test_copies                            | repitch_kernel, gather_cols_kernel (idx == null, as step_copy launches it), pad_rows_kernel |
| test_transpose                         | transpose_f32_kernel                                                                        |
| test_malformed_cases_are_refused       | none: GT_ERR_INVALID before any launch                                                      |
"""
import ctypes as Ct

import numpy as np
import pytest
import torch

import frame_kernels_ref as R
from frame_kernels_ref import SENT
from test_gpu_gemm_f32 import philox_keep

pytestmark = pytest.mark.gpu

KEYS = (0x1234ABCD, 0x9E3779B9)
NS = 26      # doubles gt_op_frame reports
I_TV, I_INV_TV, I_TV_SUM, I_S_ADV, I_S_MGE, I_S_MSE, I_NPART, I_N1 = 0, 1, 2, 7, 8, 9, 24, 25


def _lib():
    from gantts_amd import _lib as Lb
    return Lb


# ---------------------------------------------------------------------------------------------------------------------
# buffers
# ---------------------------------------------------------------------------------------------------------------------
class Buf:
    """A device buffer holding [rows][cols] at pitch ld: `pad` in the pitch padding, in `lead` elements in front and in `extra` rows
    behind.  lead = 8 keeps the data 16-byte aligned, lead = 9 puts it one float past that."""

    def __init__(self, data, ld=None, pad=np.nan, lead=8, extra=2, dtype=np.float32):
        data = np.atleast_2d(np.asarray(data, dtype=dtype))
        self.rows, self.cols = data.shape
        self.ld = ld or self.cols
        assert self.ld >= self.cols
        self.off = lead
        self.host = np.full(lead + (self.rows + extra) * self.ld, pad, dtype=dtype)
        self.inside = np.zeros(self.host.shape, dtype=bool)
        self.view(self.inside)[...] = True
        self.view(self.host)[...] = data
        self.dev = torch.from_numpy(self.host).cuda()

    def view(self, flat):
        return flat[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.host.itemsize * self.off

    def result(self, what):
        """The result region after the call; everything around it must be untouched."""
        flat = self.dev.cpu().numpy()
        R.check_guard(flat, self.host, self.inside, what)
        return self.view(flat).copy()


def inp(data, ld=None, lead=8, dtype=np.float32):
    """An input: NaN in the pitch padding and around (int32 maps: a value that would index far out of bounds)."""
    return Buf(data, ld, np.nan if dtype == np.float32 else -(1 << 30), lead, dtype=dtype)


def outp(rows, cols, ld=None, init=None):
    """A result: NaN (or `init`, for ops that work in place) inside, the sentinel in the pitch padding and around."""
    return Buf(np.full((rows, cols), np.nan, dtype=np.float32) if init is None else init, ld, SENT)


def ddev(a):
    """A device array of doubles (partials, tv_dev)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def call(op, expect=0, **kw):
    """One gt_op_frame call -> (scalars [26], partials); buffers are passed as Buf (pointer and, with the matching ld* key absent, pitch)."""
    Lb = _lib()
    c = Lb.FrameCase()
    c.op = op
    pitch_of = dict(a="lda", b="ldb", c="ldc", d="ldd", out="ldo", out2="ldo2")
    hold = []
    for k, v in kw.items():
        if k == "drop":
            _fill_site(c.drop, v, hold)
        elif isinstance(v, Buf):
            setattr(c, k, v.ptr)
            if k in pitch_of and pitch_of[k] not in kw:
                setattr(c, pitch_of[k], v.ld)
        elif isinstance(v, torch.Tensor):
            setattr(c, k, v.data_ptr())
        elif k == "sums":
            arr = (Ct.c_double * 10)(*[float(x) for x in v])
            hold.append(arr)
            c.sums = Ct.cast(arr, Ct.POINTER(Ct.c_double))
        else:
            setattr(c, k, v)
    sc = (Ct.c_double * NS)(*([float("nan")] * NS))
    cap = 2 * R.MAX_BLOCKS
    parts = (Ct.c_double * cap)(*([float("nan")] * cap))
    c.scalars = Ct.cast(sc, Ct.POINTER(Ct.c_double))
    c.partials = Ct.cast(parts, Ct.POINTER(Ct.c_double))
    c.partials_cap = cap
    rc = Lb.lib.gt_op_frame(Ct.byref(c), Lb.current_stream())
    assert rc == expect, "gt_op_frame(op %d) returned %d: %s" % (op, rc, Lb.lib.gt_last_error().decode())
    sc = np.asarray(list(sc), dtype=np.float64)
    n = 0 if rc or np.isnan(sc[I_NPART]) else int(sc[I_NPART])
    return sc, np.asarray(list(parts[:n]), dtype=np.float64)


def _fill_site(cs, d, hold):
    cs.mode, cs.p, cs.key0, cs.key1 = d["mode"], d["p"], KEYS[0], KEYS[1]
    if d.get("mask") is not None:
        hold.append(d["mask"])
        cs.mask, cs.ld_mask = d["mask"].ptr, d["mask"].ld


def twice(run):
    """Runs the case twice on fresh buffers; the two runs agree bit for bit.  Returns the first run's results."""
    first, second = run(), run()
    assert len(first) == len(second)
    for i, (x, y) in enumerate(zip(first, second)):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "result %d differs between two runs" % i
    return first


def rs_of(*key):
    """A generator seeded by the case's numbers (the same in every process)."""
    return np.random.RandomState(sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (1 << 31))


# ---------------------------------------------------------------------------------------------------------------------
# the valid-frame count
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [8, 9], ids=["aligned", "plus1float"])
@pytest.mark.parametrize("n", R.MASK_N)
def test_mask_sum_and_total(n, lead):
    Lb = _lib()
    m = (rs_of(n, lead).rand(n) < 0.7).astype(np.float32)
    m[-1] = 1.0            # the last element counts: a tail that stops one short loses it

    def run():
        mb = inp(m[None, :], lead=lead)
        assert (mb.ptr % 16 == 0) == (lead == 8)
        s1, _ = call(Lb.FRAME_MASK_SUM, mask=mb, n_mask=n, tv_override=-1.0)
        s2, _ = call(Lb.FRAME_MASK_TOTAL, mask=mb, n_mask=n)
        return s1, s2
    s1, s2 = twice(run)
    R.check_tv(s1[I_TV], s1[I_INV_TV], m, what="mask_sum n=%d" % n)
    assert s1[I_TV] == R.mask_total_ref(m, 1024, lead == 8)       # the restated walk of the path this pointer takes
    assert np.isnan(s1[2:24]).all(), "mask_sum wrote more than tv, inv_tv"
    assert s2[I_TV_SUM] == float(m.astype(np.float64).sum()), "mask_total n=%d: %r" % (n, s2[I_TV_SUM])
    assert np.isnan(s2[:2]).all() and np.isnan(s2[3:24]).all(), "mask_total wrote more than tv_sum"


def test_mask_sum_normaliser_sources():
    """tv_override > 0 wins over the sum, tv_dev over both."""
    Lb = _lib()
    n = 1023
    m = (rs_of(n).rand(n) < 0.5).astype(np.float32)

    def run():
        mb = inp(m[None, :])
        s1, _ = call(Lb.FRAME_MASK_SUM, mask=mb, n_mask=n, tv_override=777.0)
        tvd = ddev([4242.0])
        s2, _ = call(Lb.FRAME_MASK_SUM, mask=mb, n_mask=n, tv_override=777.0, tv_dev=tvd)
        s3, _ = call(Lb.FRAME_MASK_SUM, mask=mb, n_mask=n, tv_override=-1.0, tv_dev=tvd)
        return s1, s2, s3
    s1, s2, s3 = twice(run)
    R.check_tv(s1[I_TV], s1[I_INV_TV], expect=777.0, what="tv_override")
    R.check_tv(s2[I_TV], s2[I_INV_TV], expect=4242.0, what="tv_dev over tv_override")
    R.check_tv(s3[I_TV], s3[I_INV_TV], expect=4242.0, what="tv_dev")


# ---------------------------------------------------------------------------------------------------------------------
# sums of squares
# ---------------------------------------------------------------------------------------------------------------------
def _operands(rows, D, rs):
    return rs.randn(rows, D).astype(np.float32), rs.randn(rows, D).astype(np.float32)


def _sqerr_case(rows, D, mb, pad, four_valued, seed):
    Lb = _lib()
    rs = rs_of(rows, D, mb, pad, seed)
    a, b = _operands(rows, D, rs)
    m, _, _ = R.make_mask(rows, rs, four_valued)
    diff = R.masked_diff(a, b, m)
    nblk = R.red_blocks(rows * D, mb)
    w = 0.7
    tag = "sqerr %dx%d mb%d pad%d" % (rows, D, mb, pad)

    def run():
        ab, bb, mk = inp(a, D + pad), inp(b, D + (pad and pad + 1)), inp(m[None, :])
        s0, p0 = call(Lb.FRAME_SQERR, a=ab, b=bb, mask=mk, n_mask=rows, rows=rows, cols=D, max_blocks=mb)
        g = outp(rows, D, D + (pad and pad + 2))
        s1, p1 = call(Lb.FRAME_SQERR, a=ab, b=bb, mask=mk, n_mask=rows, rows=rows, cols=D, max_blocks=mb, out=g, w0=w, tv_override=-1.0)
        return s0, p0, s1, p1, g.result(tag + " gradient")
    s0, p0, s1, p1, g = twice(run)
    S = R.sq_sum(diff)
    for s, p, what in ((s0, p0, tag), (s1, p1, tag + " with gradient")):
        assert int(s[I_NPART]) == nblk
        R.check_partials(p, diff, nblk, what)
        R.check_sum(s[I_S_MSE], S, rows * D, what + " total")
    assert np.isnan(s0[:2]).all(), "the sum without a gradient needs no normaliser"
    R.check_tv(s1[I_TV], s1[I_INV_TV], m, what=tag)
    R.check_bits(g, R.sqerr_grad(diff, m, w, s1[I_INV_TV]), tag + " gradient")
    assert p0.tobytes() == p1.tobytes(), "the gradient store changed a partial"


@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "ld+5"])
@pytest.mark.parametrize("shape", R.RED_SHAPES, ids=["%dx%d-mb%d" % s[:3] for s in R.RED_SHAPES])
def test_sqerr(shape, pad):
    _sqerr_case(shape[0], shape[1], shape[2], pad, False, 1)


def test_sqerr_four_valued_mask():
    """Mask values in {0, 0.25, 0.5, 1}: the only way to see whether the mask enters once, twice or three times."""
    _sqerr_case(41, 187, 3, 5, True, 2)


@pytest.mark.parametrize("four_valued", [False, True], ids=["mask01", "mask4"])
@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "ld+5"])
@pytest.mark.parametrize("shape", R.G_LOSSES_SHAPES, ids=["%dx(%d,%d)-mb%d" % s for s in R.G_LOSSES_SHAPES])
def test_g_losses(shape, pad, four_valued):
    Lb = _lib()
    rows, D1, D2, mb = shape
    rs = rs_of(rows, D1, D2, mb, pad, four_valued)
    a1, b1 = _operands(rows, D1, rs)
    a2, b2 = _operands(rows, D2, rs)
    m, _, _ = R.make_mask(rows, rs, four_valued)
    d1, d2 = R.masked_diff(a1, b1, m), R.masked_diff(a2, b2, m)
    n1, n2 = R.red_blocks(rows * D1, mb), R.red_blocks(rows * D2, mb)
    tag = "g_losses %dx(%d,%d) mb%d" % shape
    pads = (pad, pad and pad + 1, pad and pad + 2, pad and pad + 3)

    def run():
        s, p = call(Lb.FRAME_G_LOSSES, a=inp(a1, D1 + pads[0]), b=inp(b1, D1 + pads[1]), c=inp(a2, D2 + pads[2]), d=inp(b2, D2 + pads[3]),
                    mask=inp(m[None, :]), n_mask=rows, rows=rows, cols=D1, cols2=D2, max_blocks=mb)
        return s, p
    s, p = twice(run)
    assert (int(s[I_N1]), int(s[I_NPART])) == (n1, n1 + n2), "%s: block split (%d, %d)" % (tag, int(s[I_N1]), int(s[I_NPART]) - int(s[I_N1]))
    R.check_partials(p[:n1], d1, n1, tag + " first")
    R.check_partials(p[n1:], d2, n2, tag + " second")
    R.check_sum(s[I_S_MSE], R.sq_sum(d1), rows * D1, tag + " first total")
    R.check_sum(s[I_S_MGE], R.sq_sum(d2), rows * D2, tag + " second total")


# ---------------------------------------------------------------------------------------------------------------------
# gradient assembly
# ---------------------------------------------------------------------------------------------------------------------
def _fin_inputs(rs, n_mge=37, n_mse=1030, n_hp=33):
    return (rs.rand(n_mge) * 3.0, rs.rand(n_mse) * 5.0, -rs.rand(n_hp, 5) * 2.0)


def _static_grad_case(rows, Ds, mb, pad, cfg, four_valued, seed):
    """cfg: gs, partial, adv_inv, leak, gadv, leak_unnorm (0 / 1) and rider ('none', 'hp', 'nohp', 'outnull')."""
    Lb = _lib()
    rs = rs_of(rows, Ds, mb, pad, seed)
    a, b = _operands(rows, Ds, rs)
    m, _, _ = R.make_mask(rows, rs, four_valued)
    diff = R.masked_diff(a, b, m)
    nblk = R.red_blocks(rows * Ds, mb)
    Da = min(58, Ds)
    inv = R.adv_map(Ds, Da, rs) if cfg["adv_inv"] else None
    leak = rs.randn(rows, Da).astype(np.float32) if cfg["leak"] else None
    gadv = rs.randn(rows, Da).astype(np.float32) if cfg["gadv"] else None
    mge_w, adv_w, mse_w = 0.9, 0.35, 0.6
    rider = cfg["rider"]
    pm, ps, hp = _fin_inputs(rs)
    s_adv_in = -3.25
    tag = "static_grad %dx%d mb%d pad%d %s" % (rows, Ds, mb, pad, " ".join("%s=%s" % kv for kv in sorted(cfg.items())))

    def run():
        kw = dict(a=inp(a, Ds + pad), b=inp(b, Ds + (pad and pad + 1)), mask=inp(m[None, :]), n_mask=rows, rows=rows, cols=Ds, max_blocks=mb,
                  w0=mge_w, adv_w=adv_w, want_partial=cfg["partial"], leak_unnorm=cfg["leak_unnorm"], tv_override=-1.0, cols2=Da)
        if inv is not None:
            kw["idx"] = inp(inv[None, :], dtype=np.int32)
        if leak is not None:
            kw["c"] = inp(leak, Da + 3)
        if gadv is not None:
            kw["d"] = inp(gadv, Da + 2)
        g = outp(rows, Ds, Ds + (pad and pad + 2)) if cfg["gs"] else None
        if g is not None:
            kw["out"] = g
        if rider != "none":
            kw.update(rider=1, fin_out=0 if rider == "outnull" else 1, has_adv=1, mse_w=mse_w, mge_w=mge_w, part_mge=ddev(pm), n_mge=len(pm),
                      part_mse=ddev(ps), n_mse=len(ps), sums=[np.nan] * 5 + [s_adv_in] + [np.nan] * 4)
            if rider == "hp":
                kw.update(hp=ddev(hp), n_hp=len(hp))
        s, p = call(Lb.FRAME_STATIC_GRAD, **kw)
        return (s, p) + ((g.result(tag),) if g is not None else ())
    res = twice(run)
    s, p = res[0], res[1]
    R.check_tv(s[I_TV], s[I_INV_TV], m, what=tag)
    if cfg["partial"]:
        assert int(s[I_NPART]) == nblk
        R.check_partials(p, diff, nblk, tag)
        if rider == "none":
            R.check_sum(s[I_S_MGE], R.sq_sum(diff), rows * Ds, tag + " total")
    else:
        assert int(s[I_NPART]) == 0
    if cfg["gs"]:
        t0, p1, p2 = R.static_grad_terms(diff, m, mge_w, s[I_INV_TV], inv, leak, gadv, adv_w, cfg["leak_unnorm"])
        if inv is None or (leak is None and gadv is None):
            R.check_bits(res[2], t0.astype(np.float32), tag)
        R.check_static_grad(res[2], t0, p1, p2, tag)
    if rider == "none":
        assert np.isnan(s[12:24]).all() and np.isnan(s[I_S_MSE]) and np.isnan(s[I_S_ADV]), tag + ": results without a rider"
        if not cfg["partial"]:
            assert np.isnan(s[I_S_MGE])
    else:
        R.check_fsum(s[I_S_MGE], pm, tag + " rider s_mge")
        R.check_fsum(s[I_S_MSE], ps, tag + " rider s_mse")
        if rider == "hp":
            R.check_fsum(s[I_S_ADV], hp[:, 0], tag + " rider s_adv")
        else:
            assert s[I_S_ADV] == s_adv_in
        if rider == "outnull":
            assert np.isnan(s[12:24]).all(), tag + ": out == null wrote results"
        else:
            R.check_finalize_g(s, s[I_S_MSE], s[I_S_MGE], s[I_S_ADV], s[I_TV], adv_w, mse_w, mge_w, 1, None, True, tag + " rider")


_SG_FULL = dict(gs=1, partial=1, adv_inv=1, leak=1, gadv=1, leak_unnorm=0, rider="none")


@pytest.mark.parametrize("pad", [0, 5], ids=["dense", "ld+5"])
@pytest.mark.parametrize("shape", R.RED_SHAPES, ids=["%dx%d-mb%d" % s[:3] for s in R.RED_SHAPES])
def test_static_grad_shapes(shape, pad):
    _static_grad_case(shape[0], shape[1], shape[2], pad, _SG_FULL, False, 3)


_SG_COVER = R.sg_covering_set(12)


@pytest.mark.parametrize("i", range(len(_SG_COVER)), ids=["-".join("%s%s" % (k[:2], v) for k, v in sorted(c.items())) for c in _SG_COVER])
def test_static_grad_operands(i):
    """A pairwise covering set over gs, partial, adv_inv, leak, gadv, leak_unnorm and the rider; the four-valued mask on every other case."""
    _static_grad_case(41, 187, 3, 5, _SG_COVER[i], i % 2 == 1, 4 + i)


# ---------------------------------------------------------------------------------------------------------------------
# finalisation
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("has_adv", [1, 0])
def test_finalize_g_forms(has_adv):
    """finalize_g_kernel with partials (256 threads), finalize_g_rider_kernel, static_grad's rider workgroup and finalize_g_kernel on
    the reduced sums (1 thread): same partials, the same bits."""
    Lb = _lib()
    rs = rs_of(11, has_adv)
    pm, ps, _ = _fin_inputs(rs)
    tv, s_adv = 1237.0, -411.5
    adv_w, mse_w, mge_w = 0.35, 0.6, 0.9
    sums = [np.nan] * 5 + [s_adv] + [np.nan] * 4
    w = dict(adv_w=adv_w, mse_w=mse_w, mge_w=mge_w, has_adv=has_adv, has_tv=1, tv=tv)
    a, b = _operands(3, 7, rs)
    m = np.ones(3, dtype=np.float32)

    def run():
        parts = dict(part_mge=ddev(pm), n_mge=len(pm), part_mse=ddev(ps), n_mse=len(ps))
        s_a, _ = call(Lb.FRAME_FINALIZE_G, zero_gnorm=1, sums=sums, **w, **parts)
        s_c, _ = call(Lb.FRAME_FINALIZE_G_RIDER, fin_out=1, sums=sums, **w, **parts)
        s_d, _ = call(Lb.FRAME_STATIC_GRAD, a=inp(a), b=inp(b), mask=inp(m[None, :]), n_mask=3, rows=3, cols=7, w0=mge_w, rider=1, fin_out=1,
                      sums=sums, **w, **parts)
        s_b, _ = call(Lb.FRAME_FINALIZE_G, zero_gnorm=1, sums=[np.nan] * 5 + [s_a[I_S_ADV], s_a[I_S_MGE], s_a[I_S_MSE]] + [np.nan] * 2, **w)
        return s_a, s_b, s_c, s_d
    s_a, s_b, s_c, s_d = twice(run)
    R.check_fsum(s_a[I_S_MGE], pm, "s_mge")
    R.check_fsum(s_a[I_S_MSE], ps, "s_mse")
    assert s_a[I_S_ADV] == s_adv
    R.check_finalize_g(s_a, s_a[I_S_MSE], s_a[I_S_MGE], s_adv, tv, adv_w, mse_w, mge_w, has_adv, None, True, "finalize_g with partials")
    for other, name in ((s_b, "one thread on the sums"), (s_c, "rider kernel"), (s_d, "static_grad rider")):
        assert other[:24].tobytes() == s_a[:24].tobytes(), "finalize_g forms disagree: %s\n%r\n%r" % (name, other[:24], s_a[:24])


def test_finalize_g_rider_hp_and_gnorm():
    Lb = _lib()
    rs = rs_of(12)
    pm, ps, hp = _fin_inputs(rs)
    tv = 977.0
    adv_w, mse_w, mge_w = 1.0, 0.0, 1.0
    w = dict(adv_w=adv_w, mse_w=mse_w, mge_w=mge_w, has_tv=1, tv=tv)
    gn2 = 7.5e3

    def run():
        s1, _ = call(Lb.FRAME_FINALIZE_G_RIDER, fin_out=1, has_adv=1, part_mge=ddev(pm), n_mge=len(pm), part_mse=ddev(ps), n_mse=len(ps),
                     hp=ddev(hp), n_hp=len(hp), **w)
        s2, _ = call(Lb.FRAME_FINALIZE_G_RIDER, fin_out=0, has_adv=1, hp=ddev(hp), n_hp=len(hp), **w)
        s3, _ = call(Lb.FRAME_FINALIZE_G, zero_gnorm=0, has_adv=1, sums=[np.nan] * 5 + [-5.0, 11.0, 13.0, np.nan, gn2], **w)
        s4, _ = call(Lb.FRAME_FINALIZE_G, zero_gnorm=0, has_adv=0, part_mge=ddev(pm), n_mge=len(pm), sums=[np.nan] * 5 + [-5.0, np.nan, 13.0, np.nan, gn2], **w)
        return s1, s2, s3, s4
    s1, s2, s3, s4 = twice(run)
    R.check_fsum(s1[I_S_ADV], hp[:, 0], "rider s_adv")
    R.check_fsum(s1[I_S_MGE], pm, "rider s_mge")
    R.check_fsum(s1[I_S_MSE], ps, "rider s_mse")
    R.check_finalize_g(s1, s1[I_S_MSE], s1[I_S_MGE], s1[I_S_ADV], tv, adv_w, mse_w, mge_w, 1, None, True, "rider with hp")
    assert s2[I_S_ADV] == s1[I_S_ADV] and np.isnan(s2[I_S_MGE]) and np.isnan(s2[I_S_MSE]) and np.isnan(s2[12:24]).all(), "rider with out == null"
    R.check_finalize_g(s3, 13.0, 11.0, -5.0, tv, adv_w, mse_w, mge_w, 1, gn2, False, "finalize_g with the norm")
    R.check_fsum(s4[I_S_MGE], pm, "finalize_g, one partial array")
    R.check_finalize_g(s4, 13.0, s4[I_S_MGE], -5.0, tv, adv_w, mse_w, mge_w, 0, gn2, False, "finalize_g, one partial array")


@pytest.mark.parametrize("tv_from_sum", [0, 1])
@pytest.mark.parametrize("zero_gnorm", [0, 1])
def test_finalize_d(zero_gnorm, tv_from_sum):
    Lb = _lib()
    tv = 1531.0
    s_real, s_fake, n_rok, n_fok, gn2 = -812.25, -1033.5, 1201.0, 987.0, 3.3e2
    sums = [tv if tv_from_sum else np.nan, s_real, s_fake, n_rok, n_fok, np.nan, np.nan, np.nan, gn2, np.nan]

    def run():
        kw = dict(has_tv=0) if tv_from_sum else dict(has_tv=1, tv=tv)
        s, _ = call(Lb.FRAME_FINALIZE_D, zero_gnorm=zero_gnorm, tv_from_sum=tv_from_sum, sums=sums, **kw)
        return (s,)
    s, = twice(run)
    R.check_tv(s[I_TV], s[I_INV_TV], expect=tv, what="finalize_d")
    R.check_finalize_d(s, s_real, s_fake, n_rok, n_fok, tv, gn2, bool(zero_gnorm), "finalize_d zero_gnorm=%d tv_from_sum=%d" % (zero_gnorm, tv_from_sum))


# ---------------------------------------------------------------------------------------------------------------------
# element kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.ELEMENT_SHAPES, ids=["%dx%d" % s for s in R.ELEMENT_SHAPES])
def test_element_kernels(shape):
    Lb = _lib()
    rows, cols = shape
    rs = rs_of(rows, cols)
    x, Gx, g, g0 = (rs.randn(rows, cols).astype(np.float32) for _ in range(4))
    Tx = (1.0 / (1.0 + np.exp(-rs.randn(rows, cols)))).astype(np.float32)
    tv = 613.0
    tag = "%dx%d" % shape

    def run():
        xb, tb, gb, gr = inp(x, cols + 1), inp(Tx, cols + 2), inp(Gx, cols + 3), inp(g, cols + 4)
        o1 = outp(rows, cols, cols + 5)
        call(Lb.FRAME_HIGHWAY_FWD, a=xb, b=tb, c=gb, out=o1, rows=rows, cols=cols)
        o2, o3 = outp(rows, cols, cols + 6), outp(rows, cols, cols + 7)
        call(Lb.FRAME_HIGHWAY_BWD, a=gr, b=tb, c=gb, out=o2, out2=o3, rows=rows, cols=cols)
        o4 = outp(rows, cols, cols + 1, init=g0)
        call(Lb.FRAME_SIGMOID_GRAD, a=tb, out=o4, rows=rows, cols=cols)
        o5 = outp(1, rows * cols, init=g0.reshape(1, -1))
        s, _ = call(Lb.FRAME_SCALE_INV_TV, out=o5, rows=rows, cols=cols, has_tv=1, tv=tv)
        return (o1.result(tag + " highway_fwd"), o2.result(tag + " dGx"), o3.result(tag + " dTz"), o4.result(tag + " sigmoid_grad"),
                o5.result(tag + " scale_inv_tv"), s)
    o1, o2, o3, o4, o5, s = twice(run)
    R.check_highway_fwd(o1, x, Tx, Gx, tag + " highway_fwd")
    dGx, dTz = R.highway_bwd(g, Tx, Gx)
    R.check_bits(o2, dGx, tag + " dGx")
    R.check_bits(o3, dTz, tag + " dTz")
    R.check_bits(o4, R.sigmoid_grad(g0, Tx), tag + " sigmoid_grad")
    R.check_tv(s[I_TV], s[I_INV_TV], expect=tv, what=tag)
    R.check_bits(o5.reshape(rows, cols), R.scale_inv_tv(g0, s[I_INV_TV]), tag + " scale_inv_tv")


@pytest.mark.parametrize("site", ["buffer", "philox"])
@pytest.mark.parametrize("inplace", [0, 1], ids=["out", "inplace"])
@pytest.mark.parametrize("shape", R.ELEMENT_SHAPES, ids=["%dx%d" % s for s in R.ELEMENT_SHAPES])
def test_dropout_apply(shape, inplace, site):
    Lb = _lib()
    rows, cols = shape
    rs = rs_of(rows, cols, inplace)
    x = rs.randn(rows, cols).astype(np.float32)
    p = 0.3
    keep = philox_keep(KEYS[0], KEYS[1], p, rows, cols) if site == "philox" else rs.rand(rows, cols) >= p
    tag = "dropout %dx%d %s" % (rows, cols, site)

    def run():
        d = dict(mode=1, p=p) if site == "philox" else dict(mode=2, p=p, mask=inp(keep.astype(np.float32), cols + 3))
        if inplace:
            o = outp(rows, cols, init=x)
            call(Lb.FRAME_DROPOUT_APPLY, a=o, out=o, rows=rows, cols=cols, drop=d)
        else:
            o = outp(rows, cols)
            call(Lb.FRAME_DROPOUT_APPLY, a=inp(x), out=o, rows=rows, cols=cols, drop=d)
        return (o.result(tag),)
    o, = twice(run)
    R.check_bits(o, R.dropout_apply(x, keep, p), tag)        # bit for bit: dropped elements are +0, not -0


# ---------------------------------------------------------------------------------------------------------------------
# image builders
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("halves", ["both", "generated"])
@pytest.mark.parametrize("N", R.BUILD_ADV_N)
@pytest.mark.parametrize("na", R.BUILD_ADV_NA)
def test_build_adv(na, N, halves):
    """No rider, the `sc` rider and the `tv_total` rider (the 256-thread form of the mask sums) by turns over the matrix."""
    Lb = _lib()
    rs = rs_of(na, N, halves == "both")
    ncol = na + 7
    ldf = ncol + 9                      # larger than the largest index
    fa, fb = rs.randn(N, ncol).astype(np.float32), rs.randn(N, ncol).astype(np.float32)
    idx = rs.permutation(ncol)[:na].astype(np.int32)
    idx[0] = ncol - 1
    ldo = (na + 3) & ~3
    if na == 58:
        ldo += 4                        # a whole group of pad columns
    rows, split = (2 * N, N) if halves == "both" else (N, N)      # the generated half alone, as the adversarial term builds it
    k = (R.BUILD_ADV_NA.index(na) + R.BUILD_ADV_N.index(N)) % 3
    rider, n_mask = k, R.MASK_N_RIDER[(R.BUILD_ADV_NA.index(na) + (halves == "both")) % 3]
    m = (rs.rand(n_mask) < 0.6).astype(np.float32)
    m[-1] = 1.0
    tag = "build_adv na%d N%d %s rider%d" % (na, N, halves, rider)

    def run():
        o = outp(rows, ldo)
        kw = dict(a=inp(fa, ldf), idx=inp(idx[None, :], dtype=np.int32), out=o, rows=rows, cols=na, split=split, lda=ldf)
        kw["b"] = inp(fb, ldf) if halves == "both" else kw["a"]
        if rider:
            kw.update(rider=rider, mask=inp(m[None, :], lead=8 + (na % 2)), n_mask=n_mask, tv_override=-1.0)
        s, _ = call(Lb.FRAME_BUILD_ADV, **kw)
        return o.result(tag), s
    o, s = twice(run)
    ref = R.build_adv(fa, fb, idx, split, rows, ldo)
    R.check_bits(o, ref, tag)           # the pad columns [na, ldo) are the kernel's: exactly +0
    if rider == 1:
        R.check_tv(s[I_TV], s[I_INV_TV], m, what=tag)
        assert np.isnan(s[2:24]).all()
    elif rider == 2:
        assert s[I_TV_SUM] == float(m.astype(np.float64).sum()), tag
        assert np.isnan(s[:2]).all() and np.isnan(s[3:24]).all()
    else:
        assert np.isnan(s[:24]).all(), tag + ": scalars written without a rider"


@pytest.mark.parametrize("n", R.MASK_N_RIDER)
@pytest.mark.parametrize("rider", [1, 2])
def test_build_adv_rider_sizes(n, rider):
    """The 256-thread form of mask_sum_body / mask_total_body at every size of the issue, aligned and one float past alignment."""
    Lb = _lib()
    rs = rs_of(n, rider)
    fa = rs.randn(3, 5).astype(np.float32)
    idx = np.asarray([4, 0, 2], dtype=np.int32)
    for lead in (8, 9):
        m = (rs.rand(n) < 0.6).astype(np.float32)
        m[-1] = 1.0

        def run():
            o = outp(3, 4)
            s, _ = call(Lb.FRAME_BUILD_ADV, a=inp(fa, 6), b=0, idx=inp(idx[None, :], dtype=np.int32), out=o, rows=3, cols=3, split=3, lda=6, rider=rider,
                        mask=inp(m[None, :], lead=lead), n_mask=n, tv_override=-1.0)
            return o.result("rider n=%d" % n), s
        o, s = twice(run)
        R.check_bits(o, R.build_adv(fa, fa, idx, 3, 3, 4), "build_adv with a rider")
        if rider == 1:
            R.check_tv(s[I_TV], s[I_INV_TV], m, what="rider n=%d lead=%d" % (n, lead))
        else:
            assert s[I_TV_SUM] == float(m.astype(np.float64).sum())


@pytest.mark.parametrize("shape", R.BUILD_CAT2, ids=["cd%d-na%d-N%d" % s for s in R.BUILD_CAT2])
def test_build_cat2(shape):
    Lb = _lib()
    cd, na, N = shape
    rs = rs_of(*shape)
    ncol = na + 6
    ldf = ncol + 2
    x, fa, fb = rs.randn(N, cd).astype(np.float32), rs.randn(N, ncol).astype(np.float32), rs.randn(N, ncol).astype(np.float32)
    idx = rs.permutation(ncol)[:na].astype(np.int32)
    idx[-1] = ncol - 1
    tag = "build_cat2 cd%d na%d N%d" % shape

    def run():
        o = outp(2 * N, cd + na, cd + na + 4)       # the columns beyond cd + na are not the kernel's
        call(Lb.FRAME_BUILD_CAT2, a=inp(x), b=inp(fa, ldf), c=inp(fb, ldf), idx=inp(idx[None, :], dtype=np.int32), out=o, rows=N, cols=cd, cols2=na)
        return (o.result(tag),)
    o, = twice(run)
    R.check_bits(o, R.build_cat2(x, fa, fb, idx), tag)


@pytest.mark.parametrize("cols", R.COPY_COLS)
def test_copies(cols):
    Lb = _lib()
    rs = rs_of(cols)
    rows = 19
    a = rs.randn(rows, cols).astype(np.float32)
    ldo = (cols + 3) & ~3
    tag = "cols%d" % cols

    def run():
        ab = inp(a, cols + 3)
        o1 = outp(rows, ldo)                         # repitch owns the whole pitch
        call(Lb.FRAME_REPITCH, a=ab, out=o1, rows=rows, cols=cols)
        o2 = outp(rows, cols, cols + 2)              # the dense copy owns the columns only
        call(Lb.FRAME_DENSE_COPY, a=ab, out=o2, rows=rows, cols=cols)
        o3 = outp(rows, cols)
        call(Lb.FRAME_DENSE_COPY, a=ab, out=o3, rows=rows, cols=cols)
        o4 = outp(rows, ldo + 4)                     # pad_rows: dense in, any pitch out, pad columns owned
        call(Lb.FRAME_PAD_ROWS, a=inp(a), out=o4, rows=rows, cols=cols)
        return o1.result(tag + " repitch"), o2.result(tag + " dense_copy"), o3.result(tag + " dense_copy dense"), o4.result(tag + " pad_rows")
    o1, o2, o3, o4 = twice(run)
    R.check_bits(o1, R.pad_cols(a, ldo), tag + " repitch")
    R.check_bits(o2, a, tag + " dense_copy")
    R.check_bits(o3, a, tag + " dense_copy dense")
    R.check_bits(o4, R.pad_cols(a, ldo + 4), tag + " pad_rows")


@pytest.mark.parametrize("cols", R.TRANSPOSE_DIMS)
@pytest.mark.parametrize("rows", R.TRANSPOSE_DIMS)
def test_transpose(rows, cols):
    Lb = _lib()
    a = rs_of(rows, cols).randn(rows, cols).astype(np.float32)
    tag = "transpose %dx%d" % (rows, cols)

    def run():
        o = outp(cols, rows, rows + 3)
        call(Lb.FRAME_TRANSPOSE, a=inp(a, cols + 2), out=o, rows=rows, cols=cols)
        return (o.result(tag),)
    o, = twice(run)
    R.check_bits(o, a.T, tag)


# ---------------------------------------------------------------------------------------------------------------------
# malformed cases
# ---------------------------------------------------------------------------------------------------------------------
def test_malformed_cases_are_refused():
    """GT_ERR_INVALID before any launch: no result is touched."""
    Lb = _lib()
    bad = Lb.GT_ERR_INVALID
    assert Lb.lib.gt_op_frame(None, None) == bad
    rs = rs_of(99)
    a, b = _operands(4, 6, rs)
    m = np.ones(4, dtype=np.float32)
    ab, bb, mk = inp(a, 8), inp(b, 8), inp(m[None, :])
    o = outp(4, 6, 8)
    ok = dict(a=ab, b=bb, mask=mk, n_mask=4, rows=4, cols=6, out=o, w0=1.0, tv_override=-1.0)
    call(99, expect=bad)
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, max_blocks=2000))
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, lda=5))
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, ldo=5))
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, n_mask=3))
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, rows=0))
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, mask=0))
    call(Lb.FRAME_SQERR, expect=bad, **dict(ok, has_tv=1, tv=0.0))
    inv = np.asarray([0, -1, 1, 2, -1, 3], dtype=np.int32)
    sg = dict(ok, idx=inp(inv[None, :], dtype=np.int32), cols2=4, c=inp(rs.randn(4, 4).astype(np.float32), 5))
    call(Lb.FRAME_STATIC_GRAD, expect=bad, **dict(sg, cols2=3))            # adv_inv reaches column 3 of 3
    call(Lb.FRAME_STATIC_GRAD, expect=bad, **dict(sg, ldc=3))              # leak pitch below cols2
    call(Lb.FRAME_STATIC_GRAD, expect=bad, **dict(sg, rider=1, n_mge=5))   # a count without partials
    call(Lb.FRAME_FINALIZE_G, expect=bad, adv_w=1.0)                        # no normaliser
    call(Lb.FRAME_FINALIZE_G, expect=bad, has_tv=1, tv=5.0, hp=ddev(np.zeros((2, 5))), n_hp=2)      # hp belongs to the rider forms
    idx = np.asarray([0, 7, 2], dtype=np.int32)
    adv = dict(a=ab, b=bb, idx=inp(idx[None, :], dtype=np.int32), out=outp(8, 4), rows=8, cols=3, split=4, lda=8)
    call(Lb.FRAME_BUILD_ADV, expect=bad, **dict(adv, lda=7))               # idx reaches column 7 of 7
    call(Lb.FRAME_BUILD_ADV, expect=bad, **dict(adv, split=9))
    call(Lb.FRAME_BUILD_ADV, expect=bad, **dict(adv, ldo=3))
    call(Lb.FRAME_BUILD_ADV, expect=bad, **dict(adv, out=o.ptr + 4, ldo=4))      # out one float past 16-byte alignment
    call(Lb.FRAME_BUILD_ADV, expect=bad, **dict(adv, rider=1))              # a rider without a mask
    call(Lb.FRAME_BUILD_ADV, expect=bad, **dict(adv, b=0))                  # rows beyond split without fb
    call(Lb.FRAME_TRANSPOSE, expect=bad, a=ab, out=o, rows=4, cols=6, ldo=3)
    call(Lb.FRAME_DROPOUT_APPLY, expect=bad, a=ab, out=o, rows=4, cols=6, drop=dict(mode=2, p=0.5))      # a buffer site without a mask
    call(Lb.FRAME_DROPOUT_APPLY, expect=bad, a=ab, out=o, rows=4, cols=6, drop=dict(mode=1, p=1.5))
    assert np.isnan(o.result("refused cases")).all()
    call(Lb.FRAME_SQERR, **ok)                                               # and the well-formed case runs
    assert not np.isnan(o.result("well-formed case")).any()
