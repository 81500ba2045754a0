"""The discriminator's tail against float64: every d_head_kernel instantiation, both dstack_kernel widths and both finalize forms.

gt_op_d_head and gt_op_dstack run ONE pass plus its finalising launch through the launch functions the engine's step uses
(launch_d_head / launch_dstack_pass, eng_step.hip); gt_head_path_counts counts the launches per kernel, so every case asserts WHICH
kernels ran (against `expected_counts`, a restatement of the dispatch rules) as well as what they computed.

Each GPU case fills the pitch padding of every input with NaN, pre-fills every result with NaN (random values where it accumulates) and
everything around it with a sentinel that is compared bit for bit afterwards, asserts the census exactly, and runs twice: the kernels
claim a fixed summation order, so the two runs must agree bit for bit.  Every element is then held against float64 arithmetic on the
same float32 operands (the bf16-rounded activation in the image form) with a bound carried through the chain in float64: per product
the bound of a float32 sum of K + 2 terms in any order, a layer's input bound E entering the next as E |W|^T times the dropout scale
(and the same on the way back), |dD| <= 0.25 |dz| + SIG_ULPS ulps through the sigmoid, the log terms and dz by their derivatives at the
reference point.  Dropped elements are exactly zero and the correct-counts are exactly the reference's.  On top of the bound there is a
per-tensor limit on rms(|err| / S), 4x the worst value measured on the MI355X against this float64 reference (profiles/d_tail_parity.md).
"""
import collections
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from test_gpu_gemm_f32 import EPI_ULPS, LEAKY, SIG_ULPS, TINY, U, cdiv, philox4x32_10, philox_keep, philox_thresh

DROP_NONE, DROP_PHILOX, DROP_BUFFER = 0, 1, 2
MODE_D, MODE_G = 0, 1
# gt_head_path_counts (include/gantts_hip.h)
HEAD_F32, HEAD_VEC, HEAD_IMG, DSTACK128, DSTACK256, FINALIZE64, FINALIZE16, NSLOTS = 0, 4, 7, 11, 12, 13, 14, 15
UNREACHED = {}          # slot -> why no route reaches it: every kernel of the tail is reached by a case below
KEYS = (0x1234ABCD, 0x9E3779B9)
BF16_HALF_ULP = 2.0 ** -8        # half an ulp of a bf16 (8 significant bits) relative to the value
LOG_ULPS = 4            # logf (2 ulps of the result) and the rounding of its argument, the product with the mask

# Per-tensor limits on rms(|got - ref| / S): 4x the worst value measured on the MI355X over the matrix, against the float64 reference
# (profiles/d_tail_parity.md has the table and the run).  S is the |.|-sum of the product that forms the element, |ref| itself where the
# element is a product of scalars (D, dH, dZtop).  The rigorous bound was never approached closer than 0.20 of it in float32 (Dout,
# hd-f32-K1-r33-D11-k); the bf16 images sit at their rounding (0.99 of the bound, rms = half an ulp / sqrt 3).
RMS_LIM = {
    "head": {
        "Dout": 7.1e-7,        # measured worst 1.752e-7 (hd-img-K130-r1-D11-rows)
        "dH": 2.7e-6,          # measured worst 6.504e-7 (hd-f32-K1024-r33-G10-k)
        "dHb": 6.8e-3,         # measured worst 1.699e-3 (hd-img-K130-r16-D11-rows)
        "dHbT": 6.9e-3,        # measured worst 1.709e-3 (hd-img-K130-r17-D11-rows)
        "dW": 9.3e-7,          # measured worst 2.315e-7 (hd-img-K130-r1-D11-rows)
        "db": 9.6e-7,          # measured worst 2.380e-7 (hd-img-K130-r1-D11-rows)
        "s_real": 3.0e-7,      # measured worst 7.465e-8 (hd-img-K130-r16-D11-rows)
        "s_fake": 6.0e-7,      # measured worst 1.487e-7 (hd-f32-K65-r1-D11-rows)
        "s_adv": 3.2e-7,       # measured worst 7.956e-8 (hd-f32-K1024-r33-G10-k)
    },
    "dstack": {
        "Hout1": 1.6e-7,       # measured worst 3.877e-8 (ds256-L3-D1-r96-wrap)
        "Hout2": 2.6e-7,       # measured worst 6.478e-8 (ds256-L3-D1-r74-wrap)
        "Hout3": 2.7e-7,       # measured worst 6.652e-8 (ds256-L4-D0-r74-depth)
        "dZtop": 7.4e-7,       # measured worst 1.837e-7 (ds256-L3-D1-r96-wrap)
        "Dout": 9.3e-7,        # measured worst 2.319e-7 (ds256-L4-G0-r69-depth)
        "dW": 1.5e-6,          # measured worst 3.607e-7 (ds128-L4-D1-r74-depth)
        "db": 9.8e-8,          # measured worst 2.446e-8 (ds128-L3-D1-r74-wrap)
        "gadv": 3.5e-7,        # measured worst 8.648e-8 (ds128-L3-G1-r33-adv64c0)
        "s_real": 3.9e-7,      # measured worst 9.754e-8 (ds256-L2-D1-r74-depth)
        "s_fake": 3.2e-7,      # measured worst 7.878e-8 (ds256-L2-D1-r74-depth)
        "s_adv": 8.6e-7,       # measured worst 2.138e-7 (ds256-L2-G1-r1-rows)
    },
}


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch rules (eng_step.hip: launch_d_head, launch_dstack_pass, launch_head_finalize) restated
# ---------------------------------------------------------------------------------------------------------------------
def head_blocks(rows):
    return min(1024, cdiv(rows, 32))


def finalize_slot(nblk, want_grad, want_w, defer):
    """The finalising launch of `nblk` partials, or None when it is left to the caller."""
    w = bool(want_grad and want_w)
    if defer and not w:
        return None
    return FINALIZE16 if (w and nblk >= 512) else FINALIZE64


def head_slot(K, img, vec):
    kp = 2 if K <= 128 else 4 if K <= 256 else 8 if K <= 512 else 16
    i = {2: 0, 4: 1, 8: 2, 16: 3}[kp]
    if img:
        return HEAD_IMG + i
    if vec and kp % 4 == 0:
        return HEAD_VEC + i - 1
    return HEAD_F32 + i


def expected_counts(c):
    """Launches per slot of one hook call."""
    out = [0] * NSLOTS
    if c["entry"] == "head":
        out[head_slot(c["K"], c["form"] == "img", c["form"] == "vec")] += 1
        nblk = head_blocks(c["rows"])
        f = finalize_slot(nblk, c["want_grad"], c["want_w"], c["defer"])
    else:
        out[DSTACK128 if c["hd"] == 128 else DSTACK256] += 1
        nblk = cdiv(c["rows"], 32)
        f = finalize_slot(nblk, c["want_grad"], c["want_grad"] and c["mode"] == MODE_D, False)
    if f is not None:
        out[f] += 1
    return out


def n_partials(c):
    return head_blocks(c["rows"]) if c["entry"] == "head" else cdiv(c["rows"], 32)


# ---------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------
NONE = dict(mode=DROP_NONE, p=0.0)


def site(kind, p=0.5, dp=None):
    """A dropout site: 'none', 'buf' (injected mask) or 'philox'; dp = (T, B_local, world, rank, halves) adds the data-parallel map."""
    d = dict(mode=dict(none=DROP_NONE, buf=DROP_BUFFER, philox=DROP_PHILOX)[kind], p=p if kind != "none" else 0.0)
    if dp:
        T, B, world, rank, halves = dp
        t16 = T // 16
        nl16 = B * t16
        d.update(dp_t16=t16, dp_nl16=nl16 if halves == 2 else 0xFFFFFFFF, dp_half=(B * world * t16 - nl16) if halves == 2 else 0,
                 dp_add=rank * t16, dp_mul=(world - 1) * t16, dp_inv_t16=float(np.float32(1.0) / np.float32(t16)))
    return d


_FLAVOURS = [("none",), ("buf", 0.5), ("philox", 0.3), ("philox", 0.5), ("buf", 0.3)]


def _sites(L, i):
    return [site(*_FLAVOURS[(i + l) % len(_FLAVOURS)]) for l in range(L)]


def dstack_case(hd, L, mode, want_grad, rows, n_real=None, n_mask=None, mask="ones", sites=None, norm="tv", dout=True, acc=0, Da=58, col0=425,
                ldw0_pad=0, eps=1e-20, hout_top=True, sat=False, tag=""):
    if mode == MODE_D:
        n_real = rows // 2 if n_real is None else n_real
        n_mask = rows // 2 if n_mask is None else n_mask
    else:
        n_real, n_mask = rows, (rows if n_mask is None else n_mask)
    c = dict(entry="dstack", hd=hd, L=L, mode=mode, want_grad=want_grad, rows=rows, n_real=n_real, n_mask=n_mask, mask=mask,
             sites=sites if sites is not None else [dict(NONE) for _ in range(L)], norm=norm, dout=dout, acc=acc, Da=Da, col0=col0,
             ldw0=col0 + Da + ldw0_pad, ld_gadv=Da + 3, eps=eps, hout_top=hout_top, sat=sat)
    c["id"] = "ds%d-L%d-%s%d-r%d%s" % (hd, L, "DG"[mode], want_grad, rows, "-" + tag if tag else "")
    return c


def head_case(K, rows, form="f32", mode=MODE_D, want_grad=1, want_w=None, defer=0, has_act=1, drop=None, n_real=None, n_mask=None, mask="ragged",
              norm="tv", dout=True, acc=0, eps=1e-20, b16=(False, False), sat=False, tag=""):
    want_w = (1 if (mode == MODE_D and want_grad) else 0) if want_w is None else want_w
    if mode == MODE_D:
        n_real = rows // 2 if n_real is None else n_real
        n_mask = max(1, cdiv(rows, 2)) if n_mask is None else n_mask
    else:
        n_real, n_mask = rows, (rows if n_mask is None else n_mask)
    pad = {"f32": 3, "vec": 5, "img": 8}[form]
    c = dict(entry="head", K=K, rows=rows, form=form, mode=mode, want_grad=want_grad, want_w=want_w, defer=defer, has_act=has_act,
             site=drop if drop is not None else dict(NONE), n_real=n_real, n_mask=n_mask, mask=mask, norm=norm, dout=dout, acc=acc, eps=eps,
             ldh=K + pad, lddh=K + 1, lddhb=K + 2, lddhbt=cdiv(rows, 4) * 4 + 4, dHb=b16[0], dHbT=b16[1], sat=sat)
    c["id"] = "hd-%s-K%d-r%d-%s%d%d%s" % (form, K, rows, "DG"[mode], want_grad, want_w, "-" + tag if tag else "")
    return c


def _dstack_matrix():
    out = []
    i = 0
    norms = ["tv", "tv_dev", "unit"]
    masks = ["ones", "ragged", "zero_last"]
    for hd in (128, 256):
        # depth x mode x gradients, with the dropout flavours, the normalisers, the masks, Dout and accumulate rotating
        for L in (1, 2, 3, 4):
            for mode in (MODE_D, MODE_G):
                for wg in (0, 1):
                    rows = 2 * 37 if mode == MODE_D else 69
                    out.append(dstack_case(hd, L, mode, wg, rows, mask=masks[i % 3], sites=_sites(L, i), norm=norms[i % 3], dout=i % 4 != 3,
                                           acc=(i // 2) % 2 if (mode == MODE_D and wg) else 0, eps=1e-6 if i % 5 == 0 else 1e-20,
                                           hout_top=i % 2 == 0, tag="depth"))
                    i += 1
        # G-step rows: one row, one short of / exactly / one past a panel, two panels and a ragged third
        for rows in (1, 31, 32, 33, 69):
            out.append(dstack_case(hd, 2, MODE_G, 1, rows, mask=masks[i % 3], sites=_sites(2, i), norm=norms[i % 3], tag="rows"))
            i += 1
        # D-step rows: the real / generated boundary and the mask wrap in the middle of a panel; whole 16-row groups
        out.append(dstack_case(hd, 3, MODE_D, 1, 2 * 37, n_real=37, n_mask=37, mask="ragged", sites=_sites(3, i), tag="wrap"))
        out.append(dstack_case(hd, 3, MODE_D, 1, 2 * 48, mask="ragged", sites=_sites(3, i + 1), acc=1, tag="wrap"))
        i += 2
        # the adversarial columns
        for Da in (1, 31, 32, 33, 58, 64):
            for col0 in (0, 1, 425):
                out.append(dstack_case(hd, 1 + i % 3, MODE_G, 1, 33, sites=_sites(1 + i % 3, i), Da=Da, col0=col0, norm=norms[i % 3],
                                       mask=masks[i % 3], tag="adv%dc%d" % (Da, col0)))
                i += 1
        out.append(dstack_case(hd, 2, MODE_G, 1, 40, sites=_sites(2, i), Da=33, col0=7, ldw0_pad=5, tag="ldw0pad"))
        # the data-parallel Philox map inside the fused stack: T = 16, three local sequences per half of two ranks' six, rank 1; the half
        # boundary (row 48) is an odd 16-row group, the middle of panel 1
        dp = (16, 3, 2, 1, 2)
        out.append(dstack_case(hd, 3, MODE_D, 1, 96, mask="ragged", sites=[site("philox", 0.3, dp), site("philox", 0.5, dp), site("philox", 0.3, dp)],
                               tag="dp"))
        dp1 = (16, 3, 2, 1, 1)
        out.append(dstack_case(hd, 2, MODE_G, 1, 48, sites=[site("philox", 0.5, dp1), site("philox", 0.3, dp1)], tag="dp"))
        i += 3
    # many partials: 513 panels -> the 16-column finalize with the scalar workgroup; activation is an input (L = 1): no flips
    out.append(dstack_case(128, 1, MODE_D, 1, 16416, mask="ragged", sites=[site("philox", 0.5)], tag="large"))
    out.append(dstack_case(128, 1, MODE_D, 1, 16399, n_real=8207, n_mask=8209, mask="ragged", sites=[site("buf", 0.5)], acc=1, tag="large-ragged"))
    out.append(dstack_case(256, 3, MODE_D, 1, 2 * 37, mask="ragged", sites=_sites(3, 2), sat=True, tag="saturated"))
    return out


def _head_matrix():
    out = []
    i = 0
    flav = [site("none"), site("buf", 0.5), site("philox", 0.3), site("philox", 0.5)]
    norms = ["tv", "tv_dev", "unit"]
    # K edges of every KP, each form; the image form with both bf16 outputs
    for K in (1, 63, 64, 65, 128, 130, 200, 256, 257, 512, 1000, 1024):
        for form in ("f32", "vec", "img"):
            out.append(head_case(K, 33 + (i % 3), form, mode=MODE_D if i % 2 == 0 else MODE_G, drop=flav[i % 4], norm=norms[i % 3],
                                 b16=(form == "img", form == "img"), acc=1 if i % 4 == 0 else 0, eps=1e-6 if i % 5 == 0 else 1e-20, tag="k"))
            i += 1
    # row edges: a partial 8-row item, a whole 16-row group, one row more, two workgroups, four; rows % 4 in {0, 1, 3} for the transposed tail
    for rows in (1, 15, 16, 17, 33, 100):
        for form in ("f32", "vec", "img"):
            out.append(head_case(130 if form != "f32" else 65, rows, form, drop=flav[i % 4], b16=(i % 2 == 0, True) if form == "img" else (False, False),
                                 norm=norms[i % 3], tag="rows"))
            i += 1
    # the second grid-stride trip (1024 workgroups x 32 rows < rows) and 1024 partials through the 16-column finalize
    out.append(head_case(64, 32800, "f32", drop=site("philox", 0.5), tag="large"))
    out.append(head_case(64, 32800, "img", drop=site("buf", 0.5), b16=(True, True), acc=1, tag="large"))
    # has_act x dropout mode x mode x form
    for form in ("f32", "vec", "img"):
        for has_act, d in ((0, site("none")), (1, site("none")), (1, site("buf", 0.3)), (1, site("philox", 0.3))):
            for mode in (MODE_D, MODE_G):
                out.append(head_case(200, 50, form, mode=mode, has_act=has_act, drop=d, b16=(True, i % 2 == 1) if form == "img" else (False, False),
                                     tag="act%d-d%d" % (has_act, d["mode"])))
                i += 1
    # the combinations run_head is called with: evaluation (no gradients) of either mode, the D step's training pass, the adversarial
    # term's training pass with the finalising launch and with the scalars left to the caller
    out.append(head_case(256, 70, "f32", mode=MODE_D, want_grad=0, want_w=0, tag="call"))
    out.append(head_case(256, 70, "f32", mode=MODE_G, want_grad=0, want_w=0, tag="call"))
    out.append(head_case(256, 70, "vec", mode=MODE_D, want_grad=1, want_w=1, drop=site("philox", 0.5), tag="call"))
    out.append(head_case(256, 70, "vec", mode=MODE_G, want_grad=1, want_w=0, drop=site("philox", 0.5), tag="call"))
    out.append(head_case(256, 70, "f32", mode=MODE_G, want_grad=1, want_w=0, defer=1, drop=site("buf", 0.5), acc=1, tag="defer"))
    out.append(head_case(256, 70, "img", mode=MODE_G, want_grad=1, want_w=0, defer=1, b16=(True, False), tag="defer"))
    # the data-parallel Philox map in the head, masks: all ones, zero on the last rows
    out.append(head_case(130, 96, "vec", drop=site("philox", 0.5, (16, 3, 2, 1, 2)), mask="ones", tag="dp"))
    out.append(head_case(130, 100, "img", drop=site("philox", 0.3), mask="zero_last", b16=(True, True), tag="mask0"))
    out.append(head_case(200, 60, "f32", has_act=0, sat=True, tag="saturated"))
    return out


MATRIX = _dstack_matrix() + _head_matrix()
_seen = collections.Counter()
for _c in MATRIX:
    _seen[_c["id"]] += 1
    if _seen[_c["id"]] > 1:
        _c["id"] += "-%d" % _seen[_c["id"]]
_BY_ID = {c["id"]: c for c in MATRIX}
DSTACK = [c for c in MATRIX if c["entry"] == "dstack"]
HEAD = [c for c in MATRIX if c["entry"] == "head"]


# ---------------------------------------------------------------------------------------------------------------------
# Philox keep bits of a dropout site, with the data-parallel row-group map (gemm_f32.hip.h: philox_group, philox_keep_spec)
# ---------------------------------------------------------------------------------------------------------------------
def philox_group(d, g, grouped=True):
    g = np.asarray(g, dtype=np.uint64)
    if not grouped or not d.get("dp_t16"):
        return g
    nl16 = np.uint64(d["dp_nl16"])
    h = (g >= nl16).astype(np.uint64)
    gg = g - h * nl16
    b = np.floor((gg.astype(np.float32) + np.float32(0.5)) * np.float32(d["dp_inv_t16"])).astype(np.uint64)
    return (g + h * np.uint64(d["dp_half"]) + np.uint64(d["dp_add"]) + b * np.uint64(d["dp_mul"])) & np.uint64(0xFFFFFFFF)


def site_keep(d, rows, cols, grouped=True):
    """[rows][cols] bool of a Philox site: counter (2 group(row >> 4) + ((row >> 2) & 1), col), piece 4 ((row >> 3) & 1) + (row & 3)."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    col = np.arange(cols, dtype=np.uint64)[None, :]
    ctr = (np.uint64(2) * philox_group(d, r >> np.uint64(4), grouped) + ((r >> np.uint64(2)) & np.uint64(1))) & np.uint64(0xFFFFFFFF)
    words = philox4x32_10(np.broadcast_to(ctr, (rows, cols)), np.broadcast_to(col, (rows, cols)), 0x243F6A88, 0x85A308D3, KEYS[0], KEYS[1])
    piece = 4 * ((r >> np.uint64(3)) & np.uint64(1)) + (r & np.uint64(3))
    w = np.choose((piece >> np.uint64(1)).astype(np.int64), words)
    bits = (w >> (np.uint64(16) * (piece & np.uint64(1)))) & np.uint64(0xFFFF)
    return bits >= np.uint64(philox_thresh(d["p"]))


def site_scale(d):
    if d["mode"] == DROP_NONE:
        return 1.0
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(d["p"])))


# ---------------------------------------------------------------------------------------------------------------------
# operands (cached, seeded from the case id)
# ---------------------------------------------------------------------------------------------------------------------
def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).bfloat16().float().numpy()


def _bf16_bits(a):
    return (np.ascontiguousarray(_bf16(a)).view(np.uint32) >> 16).astype(np.uint16)


def _from_bf16_bits(b):
    return (b.astype(np.uint32) << 16).view(np.float32)


def _mask_of(c, rs):
    n = c["n_mask"]
    if c["mask"] == "ones":
        return np.ones(n, dtype=np.float32)
    m = (rs.rand(n) < 0.8).astype(np.float32)
    if c["mask"] == "zero_last":                      # every row of the last panel masked out (of either half when the mask wraps)
        last = np.arange(32 * ((c["rows"] - 1) // 32), c["rows"])
        m[np.unique(last % n)] = 0.0
    if not m.any():
        m[0] = 1.0
    return m


def _keep_of(d, rows, cols, rs):
    if d["mode"] == DROP_PHILOX:
        return site_keep(d, rows, cols)
    if d["mode"] == DROP_BUFFER:
        return rs.rand(rows, cols) >= d["p"]
    return np.ones((rows, cols), dtype=bool)


def _act_of(pre, keep, d):
    """An activation as the layer below would have left it: LeakyReLU of `pre`, the dropout of site d applied."""
    h = np.where(pre > 0, pre, np.float32(LEAKY) * pre).astype(np.float32) * np.float32(site_scale(d))
    return np.where(keep, h, np.float32(0)).astype(np.float32)


def _chain(c, ops, x, keeps):
    """The hidden layers above the input x (rows of H0) in float64 with the bounds carried along: lists over the layers 0 .. L-1 of the
    activation h and its bound Eh, and over 1 .. L-1 of the pre-activation z, its bound Ez and the |.|-sums S."""
    f8 = np.float64
    hd = c["hd"]
    h = x.astype(f8)
    Eh = np.zeros_like(h)
    hs, Ehs, zs, Ezs, Ss = [h], [Eh], [], [], []
    for l in range(1, c["L"]):
        W, b = ops["W%d" % l].astype(f8), ops["b%d" % l].astype(f8)
        z = h @ W.T + b
        S = np.abs(h) @ np.abs(W).T + np.abs(b)
        Ez = (hd + 2) * U * S + Eh @ np.abs(W).T
        sc = site_scale(c["sites"][l])
        slope = np.where(z > 0, 1.0, LEAKY)
        h = np.where(keeps[l], z * slope * sc, 0.0)
        Eh = np.where(keeps[l], Ez * slope * sc + EPI_ULPS * U * np.abs(h), 0.0)
        hs.append(h); Ehs.append(Eh); zs.append(z); Ezs.append(Ez); Ss.append(S * slope * sc)
    return hs, Ehs, zs, Ezs, Ss


def _head_z(h, Eh, w, bias):
    K = h.shape[1]
    z = h @ w + bias
    return z, (K + 2) * U * (np.abs(h) @ np.abs(w) + abs(bias)) + Eh @ np.abs(w)


def _ambiguous_rows(c, ops, x, keeps):
    """Rows of the input with a pre-activation (hidden or the head's) within 1.5 of its own error bound of zero."""
    w, bias = ops["w"].astype(np.float64), float(ops["bias"][0])
    if c["entry"] == "head":
        z, Ez = _head_z(x.astype(np.float64), np.zeros(x.shape), w, bias)
        return np.abs(z) <= 1.5 * Ez
    hs, Ehs, zs, Ezs, _ = _chain(c, ops, x, keeps)
    z, Ez = _head_z(hs[-1], Ehs[-1], w, bias)
    bad = np.abs(z) <= 1.5 * Ez
    for zl, El in zip(zs, Ezs):
        bad |= (np.abs(zl) <= 1.5 * El).any(axis=1)
    return bad


def _draw_input(c, ops, d, keeps, cols, rs, act=True, img=False):
    """The input rows, seeded from the case id.  The kernels are per-frame, so a row whose draw puts some pre-activation within its error
    bound of zero (about one row in ten of a deep stack: the bound of a 256-term float32 sum is 1e-4 of the sum's scale) is drawn again
    from the same stream until none is left: the derivative codes and the counts of every case are then unambiguous, and no element has
    to be excluded from any comparison.  test_input_conditions asserts that the set is empty."""
    rows = c["rows"]
    x = np.zeros((rows, cols), dtype=np.float32)
    todo = np.arange(rows)
    for _ in range(200):
        pre = rs.randn(len(todo), cols).astype(np.float32)
        pre[pre == 0] = np.float32(0.5)
        v = _act_of(pre, keeps[0][todo], d) if act else np.tanh(pre).astype(np.float32)
        x[todo] = _bf16(v) if img else v
        if c["sat"]:
            break
        bad = _ambiguous_rows(c, ops, x[todo], [k[todo] for k in keeps])
        todo = todo[bad]
        if todo.size == 0:
            break
    assert c["sat"] or todo.size == 0, c["id"]
    return x


@functools.lru_cache(maxsize=None)
def operands(key):
    c = _BY_ID[key]
    rs = np.random.RandomState(zlib.crc32(key.encode()))
    ops = {}
    rows = c["rows"]
    ops["mask"] = _mask_of(c, rs)
    ops["tv"] = np.float32(max(float(ops["mask"].sum()), 1.0))
    if c["entry"] == "head":
        K = c["K"]
        ops["w"] = (rs.randn(K) / np.sqrt(K) * (40.0 if c["sat"] else 1.0)).astype(np.float32)
        ops["bias"] = (rs.randn(1) * 0.3).astype(np.float32)
        ops["keep"] = _keep_of(c["site"], rows, K, rs) if c["has_act"] else np.ones((rows, K), dtype=bool)
        ops["H"] = _draw_input(c, ops, c["site"], [ops["keep"]], K, rs, act=bool(c["has_act"]), img=c["form"] == "img")
        if c["acc"]:
            ops["c0_dW"], ops["c0_db"] = rs.randn(K).astype(np.float32), rs.randn(1).astype(np.float32)
    else:
        hd, L = c["hd"], c["L"]
        ops["keeps"] = [_keep_of(c["sites"][l], rows, hd, rs) for l in range(L)]
        for l in range(1, L):
            ops["W%d" % l] = (rs.randn(hd, hd) / np.sqrt(hd)).astype(np.float32)
            ops["b%d" % l] = (rs.randn(hd) * 0.3).astype(np.float32)
        ops["w"] = (rs.randn(hd) / np.sqrt(hd) * (60.0 if c["sat"] else 1.0)).astype(np.float32)
        ops["bias"] = (rs.randn(1) * 0.3).astype(np.float32)
        ops["W0"] = (rs.randn(hd, c["col0"] + c["Da"]) / np.sqrt(hd)).astype(np.float32)
        ops["H0"] = _draw_input(c, ops, c["sites"][0], ops["keeps"], hd, rs)
        if c["acc"]:
            ops["c0_dW"], ops["c0_db"] = rs.randn(hd).astype(np.float32), rs.randn(1).astype(np.float32)
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference with its error bounds
# ---------------------------------------------------------------------------------------------------------------------
def _fprime(h, keep, d, mut):
    scale = 1.0 if "fprime_noscale" in mut else site_scale(d)
    slope = 1.0 if "slope1" in mut else LEAKY
    return np.where(keep, np.where(h > 0, scale, slope * scale), 0.0)


def _entry(ref, E, S, keep=None):
    return dict(ref=np.asarray(ref, dtype=np.float64), E=np.asarray(E, dtype=np.float64), S=np.asarray(S, dtype=np.float64), keep=keep)


def head_math(c, h, Eh, w, bias, mask, inv_tv, mut):
    """The head on h [rows][K] (float64, carrying the bound Eh): formulas of the comment above d_head_kernel.  Returns the per-row
    quantities with their bounds, and the sums."""
    f8 = np.float64
    rows, K = h.shape
    n_real = c["n_real"] + (1 if "n_real+1" in mut else 0)
    eps = float(np.float32(c["eps"]))
    if "mask_unwrapped" in mut:
        m = np.concatenate([mask, np.zeros(rows)])[:rows].astype(f8)
    else:
        m = mask[np.arange(rows) % c["n_mask"]].astype(f8)
    itv = 1.0 if "no_inv_tv" in mut else inv_tv
    z = h @ w + bias
    Sz = np.abs(h) @ np.abs(w) + abs(bias)
    Ez = (K + 2) * U * Sz + Eh @ np.abs(w)
    D = 1.0 / (1.0 + np.exp(-z))
    ED = 0.25 * Ez + SIG_ULPS * U * D
    real = np.ones(rows, dtype=bool) if c["mode"] == MODE_G else (np.arange(rows) < n_real)
    den = np.where(real, D + eps, (1.0 - D) + eps)
    Eden = ED + 2 * U * np.maximum(den, 1.0 - D)
    lt = np.log(den) * m
    t = Eden / den
    El = m * (t * (1.0 + t) + LOG_ULPS * U * (1.0 + np.abs(np.log(den))))

    def g(Dv):      # dz as a function of D
        dn = np.where(real, Dv + eps, (1.0 - Dv) + eps)
        return np.where(real, -1.0, 1.0) * m * itv * Dv * (1.0 - Dv) / dn

    def gp(Dv):     # |dg / dD|
        dn = np.where(real, Dv + eps, (1.0 - Dv) + eps)
        num = (1.0 - 2.0 * Dv) * dn - np.where(real, 1.0, -1.0) * Dv * (1.0 - Dv)
        return np.abs(m * itv * num / (dn * dn))

    dz = g(D)
    lo, hi = np.clip(D - ED, 0.0, 1.0), np.clip(D + ED, 0.0, 1.0)
    Edz = np.maximum(np.maximum(gp(D), gp(lo)), gp(hi)) * ED + 8 * U * np.abs(dz)
    return dict(z=z, Ez=Ez, D=D, ED=ED, m=m, real=real, lt=lt, El=El, dz=dz, Edz=Edz)


def _sums(c, q, mut, rows_sel=None):
    """The scalars of the pass: name -> entry."""
    real, m, D = q["real"], q["m"], q["D"]
    out = {}
    if c["mode"] == MODE_D:
        out["s_real"] = _entry([q["lt"][real].sum()], [q["El"][real].sum()], [np.abs(q["lt"][real]).sum()])
        out["s_fake"] = _entry([q["lt"][~real].sum()], [q["El"][~real].sum()], [np.abs(q["lt"][~real]).sum()])
        out["n_real_ok"] = float(((D > 0.5) * m)[real].sum())
        out["n_fake_ok"] = float(((D < 0.5) * m)[~real].sum())
    else:
        out["s_adv"] = _entry([q["lt"].sum()], [q["El"].sum()], [np.abs(q["lt"]).sum()])
    return out


def _weight_grads(c, q, h, Eh, ops, mut, panel):
    """d last_linear: db = sum dz, dW = dz^T h (float32 sums over the rows in a fixed but unspecified order)."""
    dz, Edz = q["dz"].copy(), q["Edz"]
    rows = dz.shape[0]
    dzb = dz.copy()
    if "db_missing_row" in mut:
        dzb[np.flatnonzero(dzb)[-1]] = 0.0
    sel = np.ones(rows, dtype=bool)
    if "dW_missing_panel" in mut:
        sel[panel * ((rows - 1) // panel):] = False
    db, Sdb = dzb.sum(), np.abs(dz).sum()
    dW = (dz * sel) @ h
    SdW = np.abs(dz) @ np.abs(h)
    EdW = (rows + 2) * U * SdW + Edz @ np.abs(h) + np.abs(dz) @ Eh
    Edb = Edz.sum() + 2 * U * Sdb
    if c["acc"]:
        c0w, c0b = ops["c0_dW"].astype(np.float64), float(ops["c0_db"][0])
        dW, SdW, EdW = dW + c0w, SdW + np.abs(c0w), EdW + U * (np.abs(c0w) + SdW)
        db, Sdb, Edb = db + c0b, Sdb + abs(c0b), Edb + U * (abs(c0b) + Sdb)
    return _entry(dW, EdW, SdW), _entry([db], [Edb], [Sdb])


def _inv_tv(c, ops):
    return 1.0 if c["norm"] == "unit" else float(np.float32(1.0) / ops["tv"])


@functools.lru_cache(maxsize=None)
def reference(key, mut=frozenset()):
    """name -> dict(ref, E (absolute bound), S (scale of the rms), keep) of every result of the case, the counts, and `cond`: what the
    input conditions are asserted on."""
    c = _BY_ID[key]
    ops = operands(key)
    f8 = np.float64
    res, cond = {}, {}
    mask, inv_tv = ops["mask"].astype(f8), _inv_tv(c, ops)
    w, bias = ops["w"].astype(f8), float(ops["bias"][0])
    if c["entry"] == "head":
        h = ops["H"].astype(f8)
        rows, K = h.shape
        d = c["site"]
        keep = ops["keep"]
        if "philox_nogroup" in mut and d["mode"] == DROP_PHILOX:
            keep = site_keep(d, rows, K, grouped=False)
        q = head_math(c, h, np.zeros_like(h), w, bias, mask, inv_tv, mut)
        cond.update(z_head=q["z"], Ez_head=q["Ez"], inputs=[(ops["H"], ops["keep"])])
        if c["dout"]:
            res["Dout"] = _entry(q["D"], q["ED"], np.maximum(q["D"], TINY))
        res.update(_sums(c, q, mut))
        if c["want_grad"]:
            fp = _fprime(h, keep, d, mut) if c["has_act"] else np.ones_like(h)
            dH = q["dz"][:, None] * w[None, :] * fp
            EdH = q["Edz"][:, None] * np.abs(w)[None, :] * fp + EPI_ULPS * U * np.abs(dH)
            kp = fp != 0
            if c["form"] != "img":
                res["dH"] = _entry(dH, EdH, np.abs(dH), kp)
            else:
                Eb = EdH + BF16_HALF_ULP * (np.abs(dH) + EdH)
                if c["dHb"]:
                    res["dHb"] = _entry(dH, Eb, np.abs(dH), kp)
                if c["dHbT"]:
                    t = dH.T
                    if "dHbT_shift" in mut:
                        t = np.roll(t, 1, axis=1)
                    res["dHbT"] = _entry(t, Eb.T, np.abs(dH).T, kp.T)
            if c["want_w"]:
                res["dW"], res["db"] = _weight_grads(c, q, h, np.zeros_like(h), ops, mut, 32)
        res["_cond"] = cond
        return res
    # ---- fused stack
    hd, L, rows = c["hd"], c["L"], c["rows"]
    sites = c["sites"]
    keeps = list(ops["keeps"])
    if "philox_nogroup" in mut:
        keeps = [site_keep(d, rows, hd, grouped=False) if d["mode"] == DROP_PHILOX else k for d, k in zip(sites, keeps)]
    hs, Ehs, zs, Ezs, Ss = _chain(c, ops, ops["H0"], ops["keeps"])       # (the forward pass always has the right bits: a mutation is in f' only)
    h, Eh = hs[-1], Ehs[-1]
    for l in range(1, L):
        if c["mode"] == MODE_D and (l < L - 1 or c["hout_top"]):
            res["Hout%d" % l] = _entry(hs[l], Ehs[l], Ss[l - 1], ops["keeps"][l])
    q = head_math(c, h, Eh, w, bias, mask, inv_tv, mut)
    cond.update(z_head=q["z"], Ez_head=q["Ez"], z_hidden=zs, Ez_hidden=Ezs, inputs=[(ops["H0"], ops["keeps"][0])] if L == 1 else [])
    if c["dout"]:
        res["Dout"] = _entry(q["D"], q["ED"], np.maximum(q["D"], TINY))
    res.update(_sums(c, q, mut))
    if c["want_grad"]:
        fp = _fprime(hs[L - 1], keeps[L - 1], sites[L - 1], mut)
        dZ = q["dz"][:, None] * w[None, :] * fp
        EdZ = q["Edz"][:, None] * np.abs(w)[None, :] * fp + EPI_ULPS * U * np.abs(dZ)
        if c["mode"] == MODE_D:
            res["dZtop"] = _entry(dZ, EdZ, np.abs(dZ), fp != 0)
            res["dW"], res["db"] = _weight_grads(c, q, h, Eh, ops, mut, 32)
        else:
            for l in range(L - 1, 0, -1):
                W = ops["W%d" % l].astype(f8)
                fp = _fprime(hs[l - 1], keeps[l - 1], sites[l - 1], mut)
                Sg = np.abs(dZ) @ np.abs(W)
                Eg = (hd + 2) * U * Sg + EdZ @ np.abs(W)
                dZ = (dZ @ W) * fp
                EdZ = Eg * fp + EPI_ULPS * U * np.abs(dZ)
            W0c = ops["W0"].astype(f8)[:, c["col0"]:c["col0"] + c["Da"]]
            Sg = np.abs(dZ) @ np.abs(W0c)
            Eg = (hd + 3) * U * Sg + EdZ @ np.abs(W0c)
            ga = dZ[:, :hd // 2] @ W0c[:hd // 2] if "gadv_half" in mut else dZ @ W0c
            res["gadv"] = _entry(ga, Eg, Sg)
    res["_cond"] = cond
    return res


def criterion(got, r):
    """(violations of the bound, rms(|got - ref| / S) over the kept elements, worst ratio to the bound)."""
    got = np.asarray(got, dtype=np.float64).reshape(r["ref"].shape)
    err = np.abs(got - r["ref"])
    bound = r["E"] + TINY
    k = np.ones(r["ref"].shape, dtype=bool) if r["keep"] is None else r["keep"]
    bad = int(np.count_nonzero(~(err <= bound) & k))
    if r["keep"] is not None:
        bad += int(np.count_nonzero(got[~k] != 0.0))            # dropped: exactly zero
    sel = k & (r["S"] > 0)
    rel = err[sel] / r["S"][sel]
    rms = float(np.sqrt(np.mean(rel * rel))) if rel.size else 0.0
    worst = float(np.max(err[k] / bound[k])) if np.any(k) else 0.0
    return bad, rms, worst


def tensors(res):
    return [k for k, v in res.items() if isinstance(v, dict) and "ref" in v]


def assert_case(c, got, res):
    """Every result of the case against its reference entry; got: name -> array (counts as floats)."""
    tag = c["id"]
    for name in tensors(res):
        bad, rms, worst = criterion(got[name], res[name])
        lim = RMS_LIM[c["entry"]][name]
        print("DTAILSTAT %s %s %s rms=%.3e worst_bound_ratio=%.3e" % (c["entry"], tag, name, rms, worst))
        assert bad == 0, "%s: %s has %d elements outside the float64 bound (worst ratio %.3g)" % (tag, name, bad, worst)
        assert rms <= lim, "%s: %s rms(|err| / S) %.3e over the limit %.1e" % (tag, name, rms, lim)
    for name in ("n_real_ok", "n_fake_ok"):
        if name in res:
            assert got[name] == res[name], "%s: %s = %r, the reference counts %r" % (tag, name, got[name], res[name])


def rounded(res):
    """The reference itself rounded to the storage type: the stand-in for a correct kernel."""
    out = {}
    for name in tensors(res):
        v = res[name]["ref"]
        out[name] = _bf16(v).astype(np.float64) if name in ("dHb", "dHbT") else v.astype(np.float32).astype(np.float64)
    for name in ("n_real_ok", "n_fake_ok"):
        if name in res:
            out[name] = res[name]
    return out


def rejects(c, res, got):
    """Does the criterion (bounds, exact zeros, exact counts) reject `got`?"""
    for name in tensors(res):
        if name in got and criterion(got[name], res[name])[0]:
            return True
    return any(name in res and got.get(name, res[name]) != res[name] for name in ("n_real_ok", "n_fake_ok"))


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the matrix, the census model, the inputs and the criterion
# ---------------------------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_kernel():
    reached = set()
    for c in MATRIX:
        reached |= {s for s, n in enumerate(expected_counts(c)) if n}
    assert sorted(set(range(NSLOTS)) - reached) == sorted(UNREACHED)
    assert len({c["id"] for c in MATRIX}) == len(MATRIX)
    # the edges the matrix is there for
    assert {c["K"] for c in HEAD} >= {1, 63, 64, 65, 128, 130, 200, 256, 257, 512, 1000, 1024}
    assert {c["rows"] for c in HEAD} >= {1, 15, 16, 17, 33, 100, 32800}
    assert {c["rows"] % 4 for c in HEAD if c["dHbT"]} >= {0, 1, 3}
    assert any(c["defer"] and c["acc"] for c in HEAD)
    for hd in (128, 256):
        mine = [c for c in DSTACK if c["hd"] == hd]
        assert {(c["L"], c["mode"], c["want_grad"]) for c in mine} == {(L, m, g) for L in (1, 2, 3, 4) for m in (0, 1) for g in (0, 1)}
        assert {c["rows"] for c in mine if c["mode"] == MODE_G} >= {1, 31, 32, 33, 69}
        assert {(c["Da"], c["col0"]) for c in mine if c["mode"] == MODE_G and c["want_grad"]} >= {(a, b) for a in (1, 31, 32, 33, 58, 64) for b in (0, 1, 425)}
        assert any(c["mode"] == MODE_D and c["rows"] == 74 and c["n_real"] == 37 and c["n_mask"] == 37 for c in mine)
        assert any(c["sites"][0].get("dp_t16") and c["sites"][0]["dp_nl16"] % 2 == 1 for c in mine)
        assert {c["norm"] for c in mine} == {"tv", "tv_dev", "unit"} and {c["mask"] for c in mine} == {"ones", "ragged", "zero_last"}
        assert {c["dout"] for c in mine} == {True, False} and {c["acc"] for c in mine if c["mode"] == MODE_D and c["want_grad"]} == {0, 1}
    assert any(c["ldw0"] > c["col0"] + c["Da"] for c in DSTACK) and all(c["ld_gadv"] > c["Da"] for c in DSTACK)
    assert max(c["rows"] for c in MATRIX) <= 35000


def test_expected_counts_model_the_launchers():
    """Spot checks of the census model against hand-derived cases."""
    def one(**kw):
        e = expected_counts(kw)
        return {s: n for s, n in enumerate(e) if n}
    hd = dict(entry="head", form="f32", want_grad=1, want_w=1, defer=0, rows=100)
    assert one(**dict(hd, K=128)) == {0: 1, 13: 1} and one(**dict(hd, K=129)) == {1: 1, 13: 1}
    assert one(**dict(hd, K=512)) == {2: 1, 13: 1} and one(**dict(hd, K=513)) == {3: 1, 13: 1}
    assert one(**dict(hd, K=128, form="vec")) == {0: 1, 13: 1}                   # KP = 2 has no 16-byte form
    assert one(**dict(hd, K=256, form="vec")) == {4: 1, 13: 1} and one(**dict(hd, K=1024, form="vec")) == {6: 1, 13: 1}
    assert one(**dict(hd, K=64, form="img")) == {7: 1, 13: 1} and one(**dict(hd, K=1000, form="img")) == {10: 1, 13: 1}
    # 511 x 32 rows: 511 partials stay on the 64-column finalize; one row more: 512 -> 16 columns; past 32768 rows: 1024 partials
    assert one(**dict(hd, K=64, rows=511 * 32)) == {0: 1, 13: 1} and one(**dict(hd, K=64, rows=511 * 32 + 1)) == {0: 1, 14: 1}
    assert head_blocks(32800) == 1024 and head_blocks(32768) == 1024 and head_blocks(33) == 2
    assert one(**dict(hd, K=64, rows=32800, want_w=0)) == {0: 1, 13: 1}           # no weight gradients: never the 16-column form
    assert one(**dict(hd, K=64, want_w=0, defer=1)) == {0: 1} and one(**dict(hd, K=64, want_w=1, defer=1)) == {0: 1, 13: 1}
    ds = dict(entry="dstack", hd=256, mode=MODE_D, want_grad=1, rows=74)
    assert one(**ds) == {12: 1, 13: 1} and one(**dict(ds, hd=128)) == {11: 1, 13: 1}
    assert one(**dict(ds, hd=128, rows=16416)) == {11: 1, 14: 1} and one(**dict(ds, hd=128, rows=16384)) == {11: 1, 14: 1}
    assert one(**dict(ds, hd=128, rows=16383)) == {11: 1, 14: 1} and one(**dict(ds, hd=128, rows=16352)) == {11: 1, 13: 1}
    assert one(**dict(ds, rows=16416, mode=MODE_G)) == {12: 1, 13: 1} and one(**dict(ds, rows=16416, want_grad=0)) == {12: 1, 13: 1}
    assert n_partials(dict(entry="dstack", rows=16416)) == 513 and n_partials(dict(entry="dstack", rows=16399)) == 513


def test_philox_group_map():
    """The data-parallel map: local group g of rank r holds the frames of global sequence r + world b."""
    d = site("philox", 0.5, (32, 3, 2, 1, 2))        # T = 32: two groups per sequence; 3 local sequences per half, 6 global
    g = philox_group(d, np.arange(12))
    # first half: local sequences 0, 1, 2 are global 1, 3, 5 -> groups 2 3, 6 7, 10 11; second half: + 12 global groups
    assert list(g) == [2, 3, 6, 7, 10, 11, 14, 15, 18, 19, 22, 23]
    assert list(philox_group(site("philox", 0.5), np.arange(4))) == [0, 1, 2, 3]
    one = site("philox", 0.5, (16, 3, 2, 1, 1))
    assert list(philox_group(one, np.arange(3))) == [1, 3, 5]
    k = site_keep(site("philox", 0.5), 64, 300)
    assert np.array_equal(k, philox_keep(KEYS[0], KEYS[1], 0.5, 64, 300))          # without the map: the product tests' stream
    assert 0.45 < k.mean() < 0.55 and not np.array_equal(site_keep(d, 64, 8), site_keep(d, 64, 8, grouped=False))


@pytest.mark.parametrize("c", MATRIX, ids=[c["id"] for c in MATRIX])
def test_input_conditions(c):
    """No pre-activation within its own error bound of zero (no derivative code and no count can legitimately flip), |z| <= 10 where
    float64 is the reference, no exact zero among the kept inputs of a single-layer case; and the criterion accepts the reference rounded
    to the storage type."""
    res = reference(c["id"])
    cond = res["_cond"]
    if c["sat"]:
        assert np.abs(cond["z_head"]).max() >= 40.0
        return
    assert not np.any(np.abs(cond["z_head"]) <= cond["Ez_head"]), "%s: a head z within its bound of 0" % c["id"]
    assert np.abs(cond["z_head"]).max() <= 10.0
    for z, Ez in zip(cond.get("z_hidden", []), cond.get("Ez_hidden", [])):
        flips = np.argwhere(np.abs(z) <= Ez)
        assert flips.size == 0, "%s: %d hidden pre-activations within their bound of 0 " % (c["id"], len(flips))
    for x, keep in cond["inputs"]:
        assert not np.any(x[keep] == 0) and not np.any(x[~keep] != 0)
    if c["entry"] == "dstack" and c["L"] > 1:
        assert c["rows"] * c["hd"] * (c["L"] - 1) <= 1e5
    got = rounded(res)
    for name in tensors(res):
        bad, rms, worst = criterion(got[name], res[name])
        assert bad == 0 and worst <= 1.0, (c["id"], name, bad, worst)


MUTATIONS = ["n_real+1", "mask_unwrapped", "fprime_noscale", "slope1", "no_inv_tv", "db_missing_row", "dW_missing_panel", "gadv_half",
             "philox_nogroup", "dHbT_shift"]


@pytest.mark.parametrize("mut", MUTATIONS)
def test_criterion_rejects_mutations(mut):
    """Each planted fault, applied to the float64 reference's own outputs, is rejected for at least one case of either entry it can
    occur in; the unmutated reference is accepted everywhere (test_input_conditions)."""
    only = {"gadv_half": ("dstack",), "dHbT_shift": ("head",)}.get(mut, ("dstack", "head"))
    for entry in only:
        hit = []
        for c in MATRIX:
            if c["entry"] != entry or c["sat"] or c["rows"] > 200:
                continue
            res = reference(c["id"])
            if rejects(c, res, rounded(reference(c["id"], frozenset([mut])))):
                hit.append(c["id"])
        assert hit, "no %s case rejects the mutation %r" % (entry, mut)


def _fake_ptr():
    import ctypes as Ct
    return Ct.c_void_p(64)        # never dereferenced: every case below is refused before any launch


def test_hooks_reject_malformed_cases():
    import ctypes as Ct
    from gantts_amd import _lib as Lb
    lib = Lb.lib
    fake = _fake_ptr()
    assert lib.gt_op_d_head(None, None) == Lb.GT_ERR_INVALID and lib.gt_op_dstack(None, None) == Lb.GT_ERR_INVALID
    assert lib.gt_head_path_counts(None, 1) == Lb.GT_OK

    def head(**kw):
        g = Lb.DHeadCase()
        g.mode, g.K, g.ldh, g.rows, g.n_real, g.n_mask, g.has_tv, g.tv, g.eps = 0, 64, 64, 40, 20, 20, 1, 30.0, 1e-20
        g.want_grad, g.want_w, g.lddh, g.has_act = 1, 1, 64, 1
        g.H = g.w = g.bias = g.mask = g.Dout = g.dH = g.dW = g.db = fake
        for k, v in kw.items():
            if k.startswith("drop_"):
                setattr(g.drop, k[5:], v)
            else:
                setattr(g, k, v)
        return g

    bad = [head(H=None), head(w=None), head(bias=None), head(mask=None), head(K=0), head(K=1025), head(rows=0), head(mode=2), head(n_real=41),
           head(n_mask=0), head(ldh=63), head(lddh=63), head(dW=None), head(has_tv=0), head(has_tv=1, unit_tv=1), head(has_tv=1, tv_dev=fake),
           head(has_tv=0, unit_tv=1, tv_dev=fake), head(tv=0.0), head(drop_mode=3), head(drop_mode=1, drop_p=1.0), head(drop_mode=2, drop_p=0.5),
           head(drop_mode=2, drop_p=0.5, drop_mask=fake, drop_ld_mask=63), head(drop_mode=1, drop_p=0.5, has_act=0),
           head(dHb=fake, lddhb=64), head(h_ld=64, dHbT=Ct.c_void_p(68), lddhbt=40), head(h_ld=64, dHbT=fake, lddhbt=42),
           head(h_ld=64, dHbT=fake, lddhbt=36), head(h_ld=63), head(h_ld=64, dHb=fake, lddhb=63)]
    for i, g in enumerate(bad):
        assert lib.gt_op_d_head(Ct.byref(g), None) == Lb.GT_ERR_INVALID, i
        assert lib.gt_last_error()

    def stack(**kw):
        g = Lb.DStackCase()
        g.mode, g.L, g.hidden_dim, g.want_grad, g.rows, g.n_real, g.n_mask, g.has_tv, g.tv, g.eps = 1, 2, 256, 1, 40, 40, 40, 1, 30.0, 1e-20
        g.Da, g.col0, g.ldw0, g.ld_gadv = 58, 425, 483, 58
        g.H0 = g.w_last = g.b_last = g.mask = g.W0 = g.gadv = g.dZtop = g.dW_last = g.db_last = fake
        for l in range(4):
            g.W[l] = g.b[l] = 64
        for k, v in kw.items():
            if k.startswith("drop1_"):
                setattr(g.drop[1], k[6:], v)
            elif k in ("W1", "b1"):
                getattr(g, k[0])[1] = v
            else:
                setattr(g, k, v)
        return g

    bad = [stack(H0=None), stack(w_last=None), stack(b_last=None), stack(mask=None), stack(W1=None), stack(b1=None), stack(L=0), stack(L=5),
           stack(hidden_dim=64), stack(hidden_dim=512), stack(Da=0), stack(Da=65), stack(rows=0), stack(W0=None), stack(gadv=None),
           stack(ldw0=482), stack(ld_gadv=57), stack(col0=-1), stack(mode=0, dZtop=None), stack(mode=0, dW_last=None), stack(mode=0, n_real=41),
           stack(has_tv=0), stack(unit_tv=1), stack(tv_dev=fake), stack(drop1_mode=2, drop1_p=0.5, drop1_mask=fake, drop1_ld_mask=260),
           stack(drop1_mode=2, drop1_p=0.5), stack(drop1_mode=1, drop1_p=0.0)]
    for i, g in enumerate(bad):
        assert lib.gt_op_dstack(Ct.byref(g), None) == Lb.GT_ERR_INVALID, i
    counts = (Ct.c_int64 * Lb.HEAD_PATH_SLOTS)()
    assert lib.gt_head_path_counts(counts, 1) == Lb.GT_OK and sum(counts) == 0      # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
SENT = np.float32(-7.25e33)
SENT16 = np.uint16(0xF1E2)
NAN16 = np.uint16(0x7FC0)


class _Buf:
    """A device buffer holding [rows][cols] at pitch ld: `pad` in the pitch padding, in `lead` elements in front and in `extra` rows behind."""

    def __init__(self, rows, cols, ld, pad, data=None, extra=2, lead=8, dtype=np.float32):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, lead
        self.host = np.full(lead + (rows + extra) * ld, pad, dtype=dtype)
        if data is not None:
            self.view(self.host)[...] = data
        self.dev = torch.from_numpy(self.host.view(np.int16) if dtype == np.uint16 else self.host).cuda()
        self.dtype = dtype

    def view(self, flat):
        return flat[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.dev.data_ptr() + self.host.itemsize * self.off

    def got(self):
        flat = self.dev.cpu().numpy()
        flat = flat.view(np.uint16) if self.dtype == np.uint16 else flat
        return flat, self.view(flat).copy()

    def check_outside(self, flat, name, tag):
        m = np.zeros(self.host.shape, dtype=bool)
        self.view(m)[...] = True
        a, b = flat[~m], self.host[~m]
        same = np.array_equal(a.view(np.uint32), b.view(np.uint32)) if self.dtype == np.float32 else np.array_equal(a, b)
        assert same, "%s: %s written outside its result" % (tag, name)


def _in(data, ld=None, dtype=np.float32):
    data = np.atleast_2d(data)
    return _Buf(data.shape[0], data.shape[1], ld or data.shape[1], np.nan if dtype == np.float32 else NAN16, data, dtype=dtype)


def _out(rows, cols, ld, init=None, dtype=np.float32):
    fill = (np.nan if dtype == np.float32 else NAN16) if init is None else init
    return _Buf(rows, cols, ld, SENT if dtype == np.float32 else SENT16, np.broadcast_to(fill, (rows, cols)), dtype=dtype)


def _fill_site(cs, d, keep, hold):
    cs.mode, cs.p, cs.key0, cs.key1 = d["mode"], d["p"], KEYS[0], KEYS[1]
    for k in ("dp_t16", "dp_nl16", "dp_half", "dp_add", "dp_mul", "dp_inv_t16"):
        setattr(cs, k, d.get(k, 0))
    if d["mode"] == DROP_BUFFER:
        b = _in(keep.astype(np.float32))
        hold.append(b)
        cs.mask, cs.ld_mask = b.ptr, b.ld


def _fill_norm(g, c, ops, hold):
    if c["norm"] == "tv":
        g.has_tv, g.tv = 1, float(ops["tv"])
    elif c["norm"] == "tv_dev":
        t = torch.tensor([float(ops["tv"])], dtype=torch.float64).cuda()
        hold.append(t)
        g.tv_dev = t.data_ptr()
    else:
        g.unit_tv = 1


def run_case(c):
    """Builds the buffers, runs the hook with the census reset; returns (rc, counts, scalars, {name: (flat, logical, buf)})."""
    import ctypes as Ct
    from gantts_amd import _lib as Lb
    ops = operands(c["id"])
    hold, outs = [], {}
    rows = c["rows"]
    scal = (Ct.c_double * 8)(*([-1.0] * 8))
    mask = _in(ops["mask"][None])
    w, bias = _in(ops["w"][None]), _in(ops["bias"][None])
    acc = c["acc"]
    if c["entry"] == "head":
        K = c["K"]
        g = Lb.DHeadCase()
        img = c["form"] == "img"
        H = _in(_bf16_bits(ops["H"]), c["ldh"], np.uint16) if img else _in(ops["H"], c["ldh"])
        g.mode, g.K, g.rows, g.n_real, g.n_mask, g.eps = c["mode"], K, rows, c["n_real"], c["n_mask"], c["eps"]
        g.ldh, g.h_ld = (0, c["ldh"]) if img else (c["ldh"], 0)
        g.has_act, g.want_grad, g.want_w, g.defer_scalars, g.accumulate = c["has_act"], c["want_grad"], c["want_w"], c["defer"], acc
        g.H, g.w, g.bias, g.mask = H.ptr, w.ptr, bias.ptr, mask.ptr
        _fill_site(g.drop, c["site"], ops["keep"], hold)
        if c["dout"]:
            outs["Dout"] = _out(1, rows, rows)
            g.Dout = outs["Dout"].ptr
        # the seed gradient buffers are handed over whether or not gradients are wanted: without want_grad they must stay untouched
        if not img:
            outs["dH"] = _out(rows, K, c["lddh"])
            g.dH, g.lddh = outs["dH"].ptr, c["lddh"]
        if c["dHb"]:
            outs["dHb"] = _out(rows, K, c["lddhb"], dtype=np.uint16)
            g.dHb, g.lddhb = outs["dHb"].ptr, c["lddhb"]
        if c["dHbT"]:
            outs["dHbT"] = _out(K, rows, c["lddhbt"], dtype=np.uint16)
            g.dHbT, g.lddhbt = outs["dHbT"].ptr, c["lddhbt"]
            assert g.dHbT % 8 == 0
        outs["dW"] = _out(1, K, K, ops["c0_dW"] if acc else None)
        outs["db"] = _out(1, 1, 1, ops["c0_db"] if acc else None)
        g.dW, g.db = outs["dW"].ptr, outs["db"].ptr
        call = Lb.lib.gt_op_d_head
        vec = c["form"] == "vec"
    else:
        hd, L = c["hd"], c["L"]
        g = Lb.DStackCase()
        g.mode, g.L, g.hidden_dim, g.want_grad, g.accumulate = c["mode"], L, hd, c["want_grad"], acc
        g.rows, g.n_real, g.n_mask, g.eps = rows, c["n_real"], c["n_mask"], c["eps"]
        H0 = _in(ops["H0"])
        hold.append(H0)
        g.H0, g.w_last, g.b_last, g.mask = H0.ptr, w.ptr, bias.ptr, mask.ptr
        for l in range(L):
            _fill_site(g.drop[l], c["sites"][l], ops["keeps"][l], hold)
            if l:
                Wl, bl = _in(ops["W%d" % l]), _in(ops["b%d" % l][None])
                hold += [Wl, bl]
                g.W[l], g.b[l] = Wl.ptr, bl.ptr
                if l < L - 1 or c["hout_top"]:
                    outs["Hout%d" % l] = _out(rows, hd, hd)
                    g.Hout[l] = outs["Hout%d" % l].ptr
        if c["dout"]:
            outs["Dout"] = _out(1, rows, rows)
            g.Dout = outs["Dout"].ptr
        outs["dZtop"] = _out(rows, hd, hd)
        outs["dW"] = _out(1, hd, hd, ops["c0_dW"] if acc else None)
        outs["db"] = _out(1, 1, 1, ops["c0_db"] if acc else None)
        g.dZtop, g.dW_last, g.db_last = outs["dZtop"].ptr, outs["dW"].ptr, outs["db"].ptr
        W0 = _in(ops["W0"], c["ldw0"])
        outs["gadv"] = _out(rows, c["Da"], c["ld_gadv"])
        g.W0, g.ldw0, g.col0, g.Da, g.gadv, g.ld_gadv = W0.ptr, c["ldw0"], c["col0"], c["Da"], outs["gadv"].ptr, c["ld_gadv"]
        hold.append(W0)
        call = Lb.lib.gt_op_dstack
        vec = False
    _fill_norm(g, c, ops, hold)
    g.scalars = scal
    counts = (Ct.c_int64 * Lb.HEAD_PATH_SLOTS)()
    torch.cuda.synchronize()
    try:
        if vec:
            Lb.check(Lb.lib.gt_set_tuning(b"head_vec", 1))
        Lb.check(Lb.lib.gt_head_path_counts(None, 1))
        rc = call(Ct.byref(g), Ct.c_void_p(torch.cuda.current_stream().cuda_stream))
        Lb.check(Lb.lib.gt_head_path_counts(counts, 1))
    finally:
        if vec:
            Lb.check(Lb.lib.gt_set_tuning(b"head_vec", 0))
    torch.cuda.synchronize()
    out = {}
    for name, b in outs.items():
        flat, logical = b.got()
        out[name] = (flat, logical, b)
    return rc, list(counts), list(scal), out


def _written(c, res):
    """The results the case must write; every other buffer handed over must come back untouched."""
    return set(tensors(res)) - {"s_real", "s_fake", "s_adv"}


def _check_case(c):
    from gantts_amd import _lib as Lb
    tag = c["id"]
    ops = operands(tag)
    rc, counts, scal, out = run_case(c)
    assert rc == Lb.GT_OK, "%s: %s" % (tag, Lb.lib.gt_last_error())
    exp = expected_counts(c)
    assert counts == exp, "%s: launches %s, expected %s" % (tag, {i: n for i, n in enumerate(counts) if n}, {i: n for i, n in enumerate(exp) if n})
    res = reference(tag)
    written = _written(c, res)
    got = {}
    for name, (flat, logical, buf) in out.items():
        buf.check_outside(flat, name, tag)
        if name in written:
            v = _from_bf16_bits(logical) if buf.dtype == np.uint16 else logical
            assert not np.isnan(v).any(), "%s: %s has %d elements that are NaN or were never written" % (tag, name, int(np.isnan(v).sum()))
            got[name] = v.astype(np.float64)
        else:           # not asked for: bit for bit what it was
            same = np.array_equal(logical.view(np.uint32), buf.view(buf.host).view(np.uint32)) if buf.dtype == np.float32 else \
                np.array_equal(logical, buf.view(buf.host))
            assert same, "%s: %s was written although the case does not ask for it" % (tag, name)
    assert written <= set(got), (tag, sorted(written - set(got)))
    # the scalars: what the finalising launch wrote, NaN where nothing did; the normaliser; the number of partials
    names = ["s_real", "s_fake", "n_real_ok", "n_fake_ok", "s_adv"]
    finalised = expected_counts(c)[FINALIZE64] + expected_counts(c)[FINALIZE16] > 0
    mine = (names[:4] if c["mode"] == MODE_D else names[4:]) if finalised else []
    for i, name in enumerate(names):
        if name in mine:
            assert math.isfinite(scal[i]), "%s: %s = %r" % (tag, name, scal[i])
            got[name] = np.array([scal[i]]) if name.startswith("s_") else scal[i]
        else:
            assert math.isnan(scal[i]), "%s: %s = %r was written by a pass that does not own it" % (tag, name, scal[i])
    if c["norm"] == "unit":
        assert math.isnan(scal[5]) and math.isnan(scal[6]), "%s: unit_tv touched the normaliser" % tag
    else:           # (tv_dev: the kernel fills the scratch scalars from the device double)
        assert scal[5] == float(ops["tv"]) and scal[6] == float(np.float32(1.0) / ops["tv"]), (tag, scal[5], scal[6])
    assert scal[7] == n_partials(c), (tag, scal[7])
    if c["sat"]:
        _check_saturated(c, ops, got)
    else:
        if not finalised:
            res = {k: v for k, v in res.items() if k not in names}
        assert_case(c, got, res)
    # determinism: a second run is bit-identical
    rc2, _, scal2, out2 = run_case(c)
    assert rc2 == Lb.GT_OK
    for name in out:
        a, b = out[name][0], out2[name][0]
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s: %s differs between two runs" % (tag, name)
    assert np.array_equal(np.array(scal).view(np.uint64), np.array(scal2).view(np.uint64)), "%s: the scalars differ between two runs" % tag


def _check_saturated(c, ops, got):
    """|z| up to 40 and beyond: float64 means something else there (1 - D saturates in float32).  Everything stays finite, D in [0, 1],
    every log term >= log(eps) - 1, and dz has the sign of its formula (natural rows <= 0, generated rows >= 0) or is zero."""
    tag = c["id"]
    eps = float(np.float32(c["eps"]))
    rows = c["rows"]
    for name, v in got.items():
        assert np.all(np.isfinite(v)), "%s: %s is not finite" % (tag, name)
    D = got["Dout"].reshape(-1)
    assert np.all((D >= 0) & (D <= 1)) and D.min() < 1e-6 and D.max() > 1 - 1e-6
    m = ops["mask"][np.arange(rows) % c["n_mask"]]
    real = np.arange(rows) < c["n_real"]
    floor = math.log(eps) - 1.0
    for name, sel in (("s_real", real), ("s_fake", ~real)):
        s = float(got[name][0])
        assert floor * float(m[sel].sum()) <= s <= 1e-6, "%s: %s = %r" % (tag, name, s)
    g = got["dH"] if "dH" in got else got["dZtop"]
    sign = np.where(real, -1.0, 1.0)[:, None] * np.sign(ops["w"].astype(np.float64))[None, :]
    assert np.all(g * sign >= 0), "%s: a seed gradient with the wrong sign" % tag
    assert np.all(g[m == 0] == 0)
    assert float(got["n_real_ok"]) <= float(m[real].sum()) and float(got["n_fake_ok"]) <= float(m[~real].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("c", HEAD, ids=[c["id"] for c in HEAD])
def test_d_head_case_vs_float64(c):
    _check_case(c)


@pytest.mark.gpu
@pytest.mark.parametrize("c", DSTACK, ids=[c["id"] for c in DSTACK])
def test_dstack_case_vs_float64(c):
    _check_case(c)
