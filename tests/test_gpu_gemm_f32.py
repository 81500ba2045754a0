"""Every float32 MFMA product instantiation and route against float64.

The float32 family (gantts_amd/csrc/gemm_f32.hip.h) is reached through launch_gemm, linear_backward_weight and
linear_backward_weight_split (eng_gemm_f32.hip), which choose one of 95 single-product kernels -- kind x tile x loader form x
precision x compiled-in epilogue -- two pair kernels and the slab combines from the shape, the pitches, the pointer alignment,
the epilogue, the precision and the tuning knobs.  gt_op_gemm_f32 runs one product through that same dispatch, and
gt_gemm_path_counts counts the launches per kernel, so each case here asserts WHICH kernels ran (against `expected_counts`, a
restatement of the dispatch rules) as well as what they computed.

Each GPU case fills the pitch padding of every input with NaN, pre-fills the result with NaN (random values when it
accumulates) and everything around the result with a sentinel, then checks: the census; the sentinels bit for bit and no NaN;
dropped elements exactly zero where a numpy restatement of the Philox stream (or the buffer mask) says so; and every kept
element against float64 arithmetic on the same float32 operands (bf16 products: on the operands rounded to bf16) with the
deterministic bound of a float32 sum in any order, plus a per-tensor rms limit that catches systematic loss of precision.
"""
import collections
import functools
import zlib

import numpy as np
import pytest
import torch

NT, NN, TN = 0, 1, 2
A_RT, A_NONE, A_LP, A_ADDM, A_SUM2, A_SEG = -1, 0, 1, 2, 3, 4
ACT_NONE, ACT_LEAKY, ACT_SIGMOID = 0, 1, 2
DROP_NONE, DROP_PHILOX, DROP_BUFFER = 0, 1, 2
PAIR, TN_PAIR, REDUCE4, REDUCE, REDUCE_SMALL, COLSUM_PARTIAL, COLSUM_FINALIZE, REDUCE_MULTI = 576, 580, 582, 583, 584, 585, 586, 587
NSLOTS = 588
KNOBS = dict(gemm_pair=1, pair_order=1, gemm_tiles_big=0, gemm_unaligned=1, tn_wgs=512, tn_split_wgs=1024)     # GtTuning defaults
U = 2.0 ** -24
LEAKY = float(np.float32(0.01))            # the kernels' slope (0.01f)
EPI_ULPS = 4                               # epilogue roundings: slope, dropout scale (and its own rounding), accumulate, f'
SIG_ULPS = 8                               # + expf and the division of 1 / (1 + expf(-z))
TINY = 1e-35

# Per-tensor limits on rms(|got - ref| / S): 4x the worst value measured on the MI355X over the whole matrix.
# The rigorous bound itself was never approached closer than 0.28 of it (f32, bf16: 0.24); the sigmoid results never used any of the
# SIG_ULPS beyond the product part of the bound (worst excess -15 ulps).
F32_RMS_LIM = 1.8e-7                       # measured worst 4.47e-8 (bwd-1x63x31-a1-d1-m dx)
BF16_RMS_LIM = 1.2e-7                      # measured worst 2.98e-8 (fwd-63x1x58-a1-d1-bf16-t128x64-v10 y)


def cdiv(a, b):
    return -(-a // b)


def slot(kind, bm, bn, va, vb, bf16, amode):
    return (((((kind * 2 + (bm == 128)) * 2 + (bn == 128)) * 2 + int(va)) * 2 + int(vb)) * 2 + int(bool(bf16))) * 6 + (amode + 1)


def compiled_slots():
    """The instantiations of the launch templates (eng_gemm_f32_{nt,nn,tn,pair}.hip, gemm_f32_launch.hip.h): launch_gemm_v
    instantiates launch_gemm_t for 4 loader forms x 2 precisions per tile shape; launch_gemm_t adds the compiled-in epilogues of
    the 64 x 64 float32 form with 16-byte loads; then the pair kernels and the combines."""
    tiles = {NT: [(64, 64), (64, 128), (128, 64), (128, 128)], NN: [(64, 64), (64, 128), (128, 64), (128, 128)],
             TN: [(64, 64), (128, 64), (128, 128)]}
    extra = {NT: [A_NONE, A_LP, A_ADDM, A_SEG], NN: [A_NONE, A_LP], TN: [A_SUM2]}
    out = set()
    for kind in (NT, NN, TN):
        for bm, bn in tiles[kind]:
            for va in (0, 1):
                for vb in (0, 1):
                    for bf16 in (0, 1):
                        out.add(slot(kind, bm, bn, va, vb, bf16, A_RT))
        out |= {slot(kind, 64, 64, 1, 1, 0, a) for a in extra[kind]}
    out |= set(range(PAIR, PAIR + 4)) | {TN_PAIR, TN_PAIR + 1}
    out |= {REDUCE4, REDUCE, REDUCE_SMALL, COLSUM_PARTIAL, COLSUM_FINALIZE, REDUCE_MULTI}
    return sorted(out)


_TN64_4B = "linear_backward_weight takes 64 x 64 tiles only when both operands take 16-byte loads, the split layer requires them"
UNREACHED = {slot(TN, 64, 64, va, vb, p, A_RT): _TN64_4B for va, vb in ((0, 0), (0, 1), (1, 0)) for p in (0, 1)}
UNREACHED[slot(TN, 64, 64, 1, 1, 0, A_SUM2)] = ("no route hands a summed operand to launch_gemm: the split layer's summed product "
                                               "runs inside gemm_tn_pair_kernel, its one-half form has no second operand")


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch rules (eng_gemm_f32.hip, gemm_f32_launch.hip.h, eng_gemm_f32_pair.hip) restated
# ---------------------------------------------------------------------------------------------------------------------
class Invalid(Exception):
    pass


def pick_bn(n):
    return 64 if cdiv(n, 64) * 64 < cdiv(n, 128) * 128 else 128


def vec_ok(op, kc, kn):
    """gemm_vec_ok: op = (offset in floats from a 16-byte aligned base, pitch)."""
    off, ld = op
    return (kc and kn["gemm_unaligned"] != 0) or (ld % 4 == 0 and off % 4 == 0)


def small_tiles_ok(kn):
    return kn["gemm_tiles_big"] == 0


def tile_of(kind, M, N, a, b, kn, tn64=False):
    bn = pick_bn(N)
    vec = vec_ok(a, kind != TN, kn) and vec_ok(b, kind == NT, kn)
    if kind != TN and vec and M > 64 and small_tiles_ok(kn):
        return 64, 64
    small = False
    if kind != TN and M > 64:
        t128, t64 = cdiv(M, 128) * cdiv(N, bn), cdiv(M, 64) * cdiv(N, bn)
        small = 0.55 * cdiv(t64, 1024 if bn == 64 else 768) < cdiv(t128, 512)
    if kind == TN:
        return (64, 64) if tn64 else (128, bn)
    return (64 if small else 128), bn


def launch_gemm(kind, M, N, a, b, kn, bf16, act=ACT_NONE, drop=DROP_NONE, addm=False, kseg=False, sum2=False, tn64=False):
    """The slot launch_gemm -> launch_gemm_t issues; Invalid where it returns GT_ERR_INVALID."""
    bm, bn = tile_of(kind, M, N, a, b, kn, tn64)
    va, vb = vec_ok(a, kind != TN, kn), vec_ok(b, kind == NT, kn)
    hot = bm == 64 and bn == 64 and va and vb and not bf16
    if kseg:
        if kind == NT and hot and act == ACT_LEAKY and drop == DROP_PHILOX and not addm:
            return slot(kind, bm, bn, va, vb, bf16, A_SEG)
        raise Invalid("segmented forward")
    if kind != TN and hot:
        if not addm:
            if act == ACT_NONE:
                return slot(kind, bm, bn, va, vb, bf16, A_NONE)
            if act == ACT_LEAKY and drop == DROP_PHILOX:
                return slot(kind, bm, bn, va, vb, bf16, A_LP)
        elif kind == NT and act == ACT_LEAKY and drop == DROP_PHILOX:
            return slot(kind, bm, bn, va, vb, bf16, A_ADDM)
    if sum2:
        if kind == TN and hot:
            return slot(kind, bm, bn, va, vb, bf16, A_SUM2)
        raise Invalid("summed operand")
    return slot(kind, bm, bn, va, vb, bf16, A_RT)


def wgrad_slabs(rows, out, in_, t64, kn):
    """linear_backward_weight: slab count and depth."""
    bn = 64 if t64 else pick_bn(in_)
    tiles = cdiv(out, 64 if t64 else 128) * cdiv(in_, bn)
    nslab = max(1, kn["tn_wgs"] // tiles)
    nslab = max(1, min(nslab, (rows + 255) // 256))
    k_chunk = cdiv(cdiv(rows, nslab), 32) * 32
    return cdiv(rows, k_chunk), k_chunk


def split_slabs(rows, wrap, out, cd, da, kn):
    """linear_backward_weight_split: (ns1, kc1, ns2, kc2)."""
    tiles = cdiv(out, 64) * (cdiv(cd, 64) + cdiv(da, 64))
    nslab = max(1, kn["tn_split_wgs"] // tiles)
    nslab = min(nslab, max(1, wrap // 256))
    kc1 = cdiv(cdiv(wrap, nslab), 32) * 32
    ns1 = cdiv(wrap, kc1)
    kc2 = cdiv(cdiv(rows, ns1), 32) * 32
    return ns1, kc1, cdiv(rows, kc2), kc2


def pair_ok(nn_a, nn_b, M, kn):
    return kn["gemm_pair"] != 0 and small_tiles_ok(kn) and M > 64 and vec_ok(nn_a, True, kn) and vec_ok(nn_b, False, kn)


def _op(c, name, extra=0):
    return c["off"].get(name, 0) + extra, c["ld"][name]


def _combine(counts, c, can4, defer_on, want_db):
    if can4:
        counts[REDUCE_MULTI if defer_on else REDUCE4] += 1
    else:
        counts[REDUCE] += 1
        if want_db:
            counts[REDUCE_SMALL] += 1


def expected_counts(c):
    """Launches per slot of one gt_op_gemm_f32 call, or Invalid."""
    kn = dict(KNOBS, **c["knobs"])
    bf16 = c["prec"]
    counts = collections.Counter()
    r, rows, in_, out = c["route"], c["rows"], c["in_dim"], c["out_dim"]
    if r == "fwd":
        counts[launch_gemm(NT, rows, out, _op(c, "x"), _op(c, "w"), kn, bf16, c["act"], c["drop"], addm=c["addm"])] += 1
    elif r == "seg":
        counts[launch_gemm(NT, c["wrap"], out, _op(c, "x"), _op(c, "w"), kn, bf16, c["act"], c["drop"], kseg=True)] += 1
    elif r == "bwd":
        counts[launch_gemm(NN, rows, c["ncols"], _op(c, "dy"), _op(c, "w", c["col0"]), kn, bf16, c["act"], c["drop"])] += 1
    elif r == "wg":
        rode = False
        if c["dw"]:
            t64 = vec_ok(_op(c, "dy"), False, kn) and vec_ok(_op(c, "x"), False, kn) and small_tiles_ok(kn)
            nslab, _ = wgrad_slabs(rows, out, in_, t64, kn)
            can4 = (out * in_) % 4 == 0 and c["off"].get("dw", 0) % 4 == 0
            if t64 and c["rider"] and pair_ok(_op(c, "dy"), _op(c, "w", c["col0"]), rows, kn):
                am = 3 if bf16 else (0 if c["act"] == ACT_NONE else 1 if (c["act"] == ACT_LEAKY and c["drop"] == DROP_PHILOX) else 2)
                counts[PAIR + am] += 1
                rode = True
            else:
                counts[launch_gemm(TN, out, in_, _op(c, "dy"), _op(c, "x"), kn, bf16, tn64=t64)] += 1
            _combine(counts, c, can4, c["defer"] and not c["acc"] and can4, c["db"])
        elif c["db"]:
            counts[COLSUM_PARTIAL] += 1
            counts[COLSUM_FINALIZE] += 1
        if c["rider"] and not rode:
            counts[launch_gemm(NN, rows, c["ncols"], _op(c, "dy"), _op(c, "w", c["col0"]), kn, bf16, c["act"], c["drop"])] += 1
    elif r == "split":
        wrap, cd = c["wrap"], c["cd"]
        da = in_ - cd
        if not (vec_ok(_op(c, "dy"), False, kn) and vec_ok(_op(c, "x"), False, kn) and vec_ok(_op(c, "adv"), False, kn)) or bf16:
            raise Invalid("split weight gradient")
        ns1, _, ns2, _ = split_slabs(rows, wrap, out, cd, da, kn)
        can4 = (out * in_) % 4 == 0 and c["off"].get("dw", 0) % 4 == 0
        rode = False
        if rows == 2 * wrap:
            rode = bool(c["rider"] and c["act"] == ACT_NONE and vec_ok(_op(c, "dy"), True, kn) and small_tiles_ok(kn))
            counts[TN_PAIR + int(rode)] += 1
        else:
            counts[launch_gemm(TN, out, cd, _op(c, "dy"), _op(c, "x"), kn, 0, tn64=True)] += 1
            counts[launch_gemm(TN, out, da, _op(c, "dy"), _op(c, "adv"), kn, 0, tn64=True)] += 1
        _combine(counts, c, can4, c["defer"] and not c["acc"] and can4, c["db"])
        if c["rider"] and not rode:
            counts[launch_gemm(NN, wrap, c["ncols"], _op(c, "dy", (rows - wrap) * c["ld"]["dy"]), _op(c, "w", c["col0"]), kn, 0,
                               c["act"], c["drop"])] += 1
    out_counts = [0] * NSLOTS
    for k, v in counts.items():
        out_counts[k] += v
    return out_counts


# ---------------------------------------------------------------------------------------------------------------------
# the matrix
# ---------------------------------------------------------------------------------------------------------------------
def _pad4(n):
    return cdiv(n, 4) * 4


def case(route, rows, in_dim, out_dim, act=ACT_NONE, drop=DROP_NONE, p=0.5, prec=0, acc=0, bias=True, addm=False, wrap=0, cd=0,
         col0=0, ncols=None, rider=0, defer=0, dw=True, db=True, ld=None, off=None, knobs=None, tag="", invalid=False):
    ncols = in_dim - col0 if ncols is None else ncols
    dflt = dict(x=cd if route in ("seg", "split") else in_dim, w=in_dim, y=out_dim, dy=out_dim, h=ncols, mask=out_dim if route == "fwd" else ncols,
                addm=out_dim, adv=in_dim - cd, dx=ncols)
    dflt.update(ld or {})
    c = dict(route=route, rows=rows, in_dim=in_dim, out_dim=out_dim, act=act, drop=drop, p=p, prec=prec, acc=acc, bias=bias, addm=addm,
             wrap=wrap, cd=cd, col0=col0, ncols=ncols, rider=rider, defer=defer, dw=dw, db=db, ld=dflt, off=dict(off or {}),
             knobs=dict(knobs or {}), invalid=invalid)
    c["id"] = "%s-%dx%dx%d%s%s%s%s%s" % (route, rows, in_dim, out_dim, "-a%d" % act if act else "", "-d%d" % drop if drop else "",
                                       "-bf16" if prec else "", "-acc" if acc else "", "-" + tag if tag else "")
    return c


def _loader_ld(n, vec):
    """A pitch (and offset) for an operand n floats wide whose loader should (not) be the 16-byte one."""
    if vec:
        return _pad4(n), 0
    return (n, 0) if n % 4 else (n, 1)


def _targeted():
    """One case per (kind, tile, loader form, precision) with a run-time epilogue."""
    out = []
    flavours = [(ACT_LEAKY, DROP_BUFFER, 0.5), (ACT_SIGMOID, DROP_NONE, 0.5), (ACT_LEAKY, DROP_PHILOX, 0.3), (ACT_NONE, DROP_NONE, 0.5)]
    ks = [425, 483, 33, 7, 58, 31, 1, 512]
    i = 0
    for prec in (0, 1):
        for va in (1, 0):
            for vb in (1, 0):
                for bm, bn in ((64, 64), (64, 128), (128, 64), (128, 128)):
                    K = ks[i % len(ks)]
                    act, drop, p = flavours[i % len(flavours)]
                    if bm == 64 and bn == 64 and va and vb and not prec and (act, drop) in ((ACT_NONE, DROP_NONE), (ACT_LEAKY, DROP_PHILOX)):
                        act, drop, p = ACT_SIGMOID, DROP_NONE, 0.5     # the run-time flavour of the hot form
                    M = 129 if bm == 64 else 63
                    N = 58 if bn == 64 else 256
                    kn = dict(gemm_unaligned=0 if not (va and vb) else 1, gemm_tiles_big=1 if (va and vb and (bm, bn) != (64, 64)) else 0)
                    # forward: x (K wide, k-contiguous) and w (K wide, k-contiguous)
                    ldx, ox = _loader_ld(K, va)
                    ldw, ow = _loader_ld(K, vb)
                    out.append(case("fwd", M, K, N, act, drop, p, prec, ld=dict(x=ldx, w=ldw), off=dict(x=ox, w=ow), knobs=kn,
                                    tag="t%dx%d-v%d%d" % (bm, bn, va, vb)))
                    # backward-data: dy (k-contiguous, K = out wide), w + col0 (n-contiguous, row pitch ldw)
                    ldd, od = _loader_ld(K, va)
                    if vb:
                        ldw2, col0 = _pad4(N + 3), 0
                    else:
                        ldw2, col0 = (N + 5, 0) if i % 2 else (_pad4(N + 3), 1)
                    out.append(case("bwd", M, ldw2 if col0 == 0 else N + 1, K, act, drop, p, prec, col0=col0, ncols=N,
                                    ld=dict(dy=ldd, w=ldw2), off=dict(dy=od), knobs=kn, tag="t%dx%d-v%d%d" % (bm, bn, va, vb)))
                    i += 1
    # weight gradients: A = dy (m-contiguous, out wide), B = x (n-contiguous, in wide)
    for prec in (0, 1):
        for va in (1, 0):
            for vb in (1, 0):
                for bn in (64, 128):
                    out_d = 63 if va else 65
                    in_ = 58 if bn == 64 else 256
                    ldd, od = (64, 0) if va else (65, 0)
                    ldx, ox = (_pad4(in_), 0) if vb else (in_, 1)
                    kn = dict(gemm_tiles_big=1) if (va and vb) else {}
                    out.append(case("wg", 300 + 37 * i % 400, in_, out_d, prec=prec, ld=dict(dy=ldd, x=ldx), off=dict(dy=od, x=ox),
                                    knobs=kn, tag="t128x%d-v%d%d" % (bn, va, vb)))
                    i += 1
        out.append(case("wg", 1000, 187, 64, prec=prec, ld=dict(x=188), tag="t64"))
    return out


P4 = dict(x=428, w=428)         # 425-wide operands on a 16-byte pitch


def _edges():
    c = []
    # the six shapes of test_linear_forward_backward_vs_torch, each route
    for rows, din, dout, act in [(77, 425, 512, 1), (1000, 512, 187, 0), (300, 483, 256, 1), (129, 25, 25, 2), (4096, 256, 58, 0), (33, 7, 3, 1)]:
        drop = DROP_BUFFER if act == 1 else DROP_NONE
        c.append(case("fwd", rows, din, dout, act, drop, tag="linear"))
        c.append(case("bwd", rows, din, dout, act, drop, tag="linear"))
        c.append(case("wg", rows, din, dout, tag="linear"))
    # M edges, N edges, K edges (forward and backward-data, f32 and bf16)
    for M in (1, 7, 63, 64, 65, 129):
        c.append(case("fwd", M, 33, 65, ACT_LEAKY, DROP_PHILOX, tag="m"))
        c.append(case("bwd", M, 63, 31, ACT_LEAKY, DROP_PHILOX, p=0.3, tag="m"))
    for N in (1, 3, 58, 63, 64, 65, 187, 256, 512):
        c.append(case("fwd", 200, 58, N, ACT_SIGMOID, tag="n"))
        c.append(case("bwd", 200, N, 58, ACT_SIGMOID, tag="n"))
    for K in (1, 7, 31, 32, 33, 58, 425, 483, 512):
        c.append(case("fwd", 97, K, 64, tag="k"))
        c.append(case("fwd", 97, K, 64, prec=1, tag="k"))
        c.append(case("bwd", 97, 64, K, ACT_LEAKY, DROP_BUFFER, tag="k"))
        c.append(case("wg", K * 3 + 1, 64, K, tag="k"))
    # grids: tile counts 1..7 (gemm_xcd_order q == 0), counts that are not multiples of 8, several resident rounds
    for t in range(1, 8):
        c.append(case("fwd", 64 * t + 1, 64, 64, ACT_LEAKY, DROP_PHILOX, tag="grid%d" % t))
    c.append(case("fwd", 64 * 37 + 5, 96, 64 * 3, ACT_NONE, tag="grid333"))
    c.append(case("fwd", 16384, 512, 512, ACT_LEAKY, DROP_PHILOX, tag="cfg2"))
    c.append(case("bwd", 32768, 256, 256, ACT_LEAKY, DROP_PHILOX, tag="cfg2"))
    c.append(case("bwd", 16384, 425, 512, ld=dict(dx=428), tag="cfg2-in"))
    # pitches: dense 425 / 483 / 187, padded, base offset one float; 16-byte loads of unaligned rows on and off
    for un in (1, 0):
        kn = dict(gemm_unaligned=un)
        c.append(case("fwd", 300, 425, 187, ACT_LEAKY, DROP_PHILOX, knobs=kn, tag="dense%d" % un))
        c.append(case("fwd", 300, 483, 256, ACT_SIGMOID, knobs=kn, off=dict(x=1, y=1), ld=dict(x=484, y=257), tag="off%d" % un))
        c.append(case("bwd", 300, 187, 483, ACT_LEAKY, DROP_BUFFER, knobs=kn, ld=dict(dy=483, dx=188, h=189), off=dict(dy=1, dx=1), tag="off%d" % un))
        c.append(case("bwd", 300, 188, 256, ACT_LEAKY, DROP_PHILOX, knobs=kn, ld=dict(dx=188, h=188), tag="wide%d" % un))
    # Philox: rows crossing 16-row groups, columns > 256, p 0.5 / 0.3, forward and backward-data
    c.append(case("fwd", 16 * 9 + 7, 40, 300, ACT_LEAKY, DROP_PHILOX, p=0.3, tag="philox"))
    c.append(case("bwd", 16 * 9 + 7, 300, 40, ACT_LEAKY, DROP_PHILOX, p=0.3, tag="philox"))
    c.append(case("fwd", 16 * 5 + 3, 40, 260, ACT_LEAKY, DROP_PHILOX, p=0.5, prec=1, tag="philox"))
    c.append(case("fwd", 100, 37, 70, ACT_LEAKY, DROP_NONE, tag="leaky"))
    # accumulate
    c.append(case("fwd", 129, 58, 187, ACT_LEAKY, DROP_PHILOX, acc=1))
    c.append(case("fwd", 33, 58, 65, ACT_SIGMOID, acc=1))
    c.append(case("bwd", 129, 187, 58, ACT_LEAKY, DROP_PHILOX, acc=1))
    c.append(case("bwd", 129, 187, 58, ACT_NONE, acc=1, prec=1))
    # backward-data column slices
    c.append(case("bwd", 200, 483, 256, col0=425, ncols=58, ld=dict(dx=60), tag="col425"))
    c.append(case("bwd", 200, 483, 256, ACT_LEAKY, DROP_PHILOX, col0=3, ncols=100, ld=dict(dx=104), tag="col3"))
    c.append(case("bwd", 16384, 484, 256, col0=425, ncols=58, ld=dict(w=484, dx=58), tag="col-cfg2"))
    # weight gradients: one slab; a ragged last slab; nslab cut by the k_chunk rounding; can4 false; db only; accumulate
    c.append(case("wg", 255, 64, 64, tag="oneslab"))
    c.append(case("wg", 1000, 64, 64, tag="ragged"))
    c.append(case("wg", 16384 + 33, 512, 512, knobs=dict(tn_wgs=4096), tag="kchunk"))
    c.append(case("wg", 513, 63, 65, tag="odd"))
    c.append(case("wg", 513, 64, 64, off=dict(dw=1), tag="dwoff"))
    c.append(case("wg", 700, 64, 187, dw=False, tag="dbonly"))
    c.append(case("wg", 700, 187, 64, db=False, tag="nodb"))
    c.append(case("wg", 700, 128, 64, acc=1, tag="acc"))
    c.append(case("wg", 700, 63, 65, acc=1, tag="acc-odd"))
    c.append(case("wg", 32768, 256, 256, tag="cfg2"))
    c.append(case("wg", 700, 58, 63, prec=1, ld=dict(dy=64, x=60), tag="bf16"))
    # pair launches (backward-data riding in the weight gradient's launch) and deferred combines
    for act, drop, prec in ((ACT_NONE, DROP_NONE, 0), (ACT_LEAKY, DROP_PHILOX, 0), (ACT_LEAKY, DROP_BUFFER, 0), (ACT_SIGMOID, DROP_NONE, 0),
                            (ACT_LEAKY, DROP_PHILOX, 1)):
        c.append(case("wg", 3000, 256, 128, act, drop, prec=prec, rider=1, tag="pair"))
    c.append(case("wg", 32768, 256, 256, ACT_LEAKY, DROP_PHILOX, rider=1, tag="pair-cfg2"))
    c.append(case("wg", 60, 64, 64, ACT_LEAKY, DROP_PHILOX, rider=1, tag="pair-m60"))
    c.append(case("wg", 3000, 256, 128, ACT_LEAKY, DROP_PHILOX, rider=1, knobs=dict(pair_order=0), tag="pair-order0"))
    c.append(case("wg", 3000, 256, 128, defer=1, tag="defer"))
    c.append(case("wg", 3000, 63, 65, defer=1, tag="defer-odd"))
    c.append(case("wg", 3000, 256, 128, defer=1, acc=1, tag="defer-acc"))
    # added matrix (split first layer's adversarial product), two-segment forward
    c.append(case("fwd", 2 * 100, 58, 256, ACT_LEAKY, DROP_PHILOX, addm=True, wrap=100, bias=False, tag="addm"))
    c.append(case("fwd", 130, 58, 187, ACT_LEAKY, DROP_BUFFER, addm=True, wrap=65, tag="addm-rt"))
    c.append(case("fwd", 2 * 16384, 58, 256, ACT_LEAKY, DROP_PHILOX, addm=True, wrap=16384, bias=False, ld=dict(x=60), tag="addm-cfg2"))
    # two halves with wrap % 64 != 0: the second half's tiles start at wrap + 64 t.  wrap = 100 and 69 (not multiples of 16) drew the
    # second half's keep bits from the wrong Philox pieces (about half of its elements wrong) until the epilogue took each element's
    # own bits there (gemm_f32.hip.h: gemm_store_tile, px_own); wrap = 80 starts the second half on a 16-row group
    c.append(case("seg", 2 * 100, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=100, cd=425, ld=dict(x=428, w=483, adv=60), tag="2half"))
    c.append(case("seg", 2 * 69, 88, 128, ACT_LEAKY, DROP_PHILOX, wrap=69, cd=30, ld=dict(x=32, adv=60), tag="2half-wrap69"))
    c.append(case("seg", 2 * 80, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=80, cd=425, ld=dict(x=428, w=483, adv=60), tag="2half-wrap80"))
    c.append(case("fwd", 2 * 100, 58, 256, ACT_LEAKY, DROP_PHILOX, addm=True, wrap=100, ld=dict(x=60), tag="addm-wrap100"))
    c.append(case("seg", 150, 483, 187, ACT_LEAKY, DROP_PHILOX, p=0.3, wrap=150, cd=425, ld=dict(x=425, adv=58), tag="1half"))
    c.append(case("seg", 2 * 16384, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=16384, cd=425, ld=dict(x=428, adv=60), tag="cfg2"))
    c.append(case("seg", 2 * 64, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=64, cd=425, tag="wrap64", invalid=True))
    c.append(case("seg", 2 * 100, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=100, cd=425, prec=1, tag="bf16", invalid=True))
    c.append(case("seg", 2 * 100, 483, 256, ACT_SIGMOID, wrap=100, cd=425, tag="sigmoid", invalid=True))
    # split weight gradient: two halves (gemm_tn_pair_kernel, with / without the rider), one half (two launches), cfg2
    sp = dict(x=428, adv=60)
    c.append(case("split", 2 * 300, 483, 256, wrap=300, cd=425, ld=sp, tag="2half"))
    c.append(case("split", 2 * 300, 483, 256, wrap=300, cd=425, ld=dict(sp, w=483, dx=58), rider=1, col0=425, ncols=58, tag="rider"))
    c.append(case("split", 2 * 300, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=300, cd=425, ld=dict(sp, dx=58, h=58), rider=1, col0=425,
                  ncols=58, tag="rider-act"))
    c.append(case("split", 300, 483, 256, wrap=300, cd=425, ld=sp, rider=1, col0=425, ncols=58, tag="1half"))
    c.append(case("split", 2 * 16384, 483, 256, wrap=16384, cd=425, ld=dict(sp, dx=58), rider=1, col0=425, ncols=58, defer=1, tag="cfg2"))
    c.append(case("split", 2 * 77, 483, 63, wrap=77, cd=425, ld=dict(sp, dy=64), acc=1, tag="odd-acc"))
    c.append(case("split", 2 * 100, 483, 256, wrap=100, cd=425, ld=dict(sp, dy=257), off=dict(dy=1), tag="misaligned", invalid=True))
    return c


MATRIX = _targeted() + _edges()
_seen = collections.Counter()
for _c in MATRIX:
    _seen[_c["id"]] += 1
    if _seen[_c["id"]] > 1:
        _c["id"] += "-%d" % _seen[_c["id"]]


# ---------------------------------------------------------------------------------------------------------------------
# Philox4x32-10 and the keep bits (gemm_f32.hip.h: philox4x32_10, philox_keep) in numpy
# ---------------------------------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    c = [np.asarray(v, dtype=np.uint64) & _M32 for v in (c0, c1, c2, c3)]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M32, (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def philox_thresh(p):
    th = float(np.float32(p)) * 65536.0 + 0.5
    return 65535 if th >= 65535.0 else int(th)


def philox_keep(key0, key1, p, rows, cols):
    """[rows][cols] bool: keep iff the 16-bit piece of (row, col) >= thresh."""
    r = np.arange(rows, dtype=np.uint64)[:, None]
    col = np.arange(cols, dtype=np.uint64)[None, :]
    ctr = np.uint64(2) * (r >> np.uint64(4)) + ((r >> np.uint64(2)) & np.uint64(1))
    words = philox4x32_10(np.broadcast_to(ctr, (rows, cols)), np.broadcast_to(col, (rows, cols)), 0x243F6A88, 0x85A308D3, key0, key1)
    piece = 4 * ((r >> np.uint64(3)) & np.uint64(1)) + (r & np.uint64(3))
    w = np.choose((piece >> np.uint64(1)).astype(np.int64), words)
    bits = (w >> (np.uint64(16) * (piece & np.uint64(1)))) & np.uint64(0xFFFF)
    return bits >= np.uint64(philox_thresh(p))


# ---------------------------------------------------------------------------------------------------------------------
# operands, float64 references, the acceptance criterion
# ---------------------------------------------------------------------------------------------------------------------
KEYS = (0x1234ABCD, 0x9E3779B9)


def _shapes(c):
    """name -> (rows, cols) of every operand of the case."""
    r, rows, in_, out, nc = c["route"], c["rows"], c["in_dim"], c["out_dim"], c["ncols"]
    s = {}
    if r == "fwd":
        s.update(x=(rows, in_), w=(out, in_), y=(rows, out))
        if c["addm"]:
            s["addm"] = (c["wrap"], out)
        if c["drop"] == DROP_BUFFER:
            s["mask"] = (rows, out)
    elif r == "seg":
        s.update(x=(c["wrap"], c["cd"]), adv=(rows, in_ - c["cd"]), w=(out, in_), y=(rows, out))
    else:
        s["dy"] = (rows, out)
        if r == "wg" and c["dw"]:
            s["x"] = (rows, in_)
        if r == "split":
            s.update(x=(c["wrap"], c["cd"]), adv=(rows, in_ - c["cd"]))
        if r == "bwd" or c["rider"]:
            drow = c["wrap"] if r == "split" else rows
            s.update(w=(out, in_), dx=(drow, nc))
            if c["act"] != ACT_NONE:
                s["h"] = (drow, nc)
            if c["drop"] == DROP_BUFFER:
                s["mask"] = (drow, nc)
    return s


@functools.lru_cache(maxsize=None)
def operands(key):
    """float32 operands of a case (cached per shape and flavour)."""
    c = _BY_ID[key]
    rs = np.random.RandomState(zlib.crc32(key.encode()))
    ops = {}
    for name, (r, n) in _shapes(c).items():
        if name in ("y", "dx"):
            continue
        if name == "mask":
            ops[name] = (rs.rand(r, n) >= c["p"]).astype(np.float32)
        elif name == "h":
            ops[name] = (rs.rand(r, n) if c["act"] == ACT_SIGMOID else rs.randn(r, n)).astype(np.float32)
        elif name == "w":
            ops[name] = (rs.randn(r, n) / np.sqrt(max(n, 1))).astype(np.float32)
        else:
            ops[name] = rs.randn(r, n).astype(np.float32)
    if c["bias"] and c["route"] in ("fwd", "seg"):
        ops["bias"] = rs.randn(c["out_dim"]).astype(np.float32)
    if c["acc"]:
        for name in ("y", "dx", "dw", "db"):
            if name in ("y", "dx") and name in _shapes(c):
                ops["c0_" + name] = rs.randn(*_shapes(c)[name]).astype(np.float32)
        if c["route"] in ("wg", "split"):
            ops["c0_dw"] = rs.randn(c["out_dim"], c["in_dim"]).astype(np.float32)
            ops["c0_db"] = rs.randn(c["out_dim"]).astype(np.float32)
    return ops


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a)).bfloat16().float().numpy()


def _keep(c, rows, cols, ops):
    if c["drop"] == DROP_PHILOX:
        return philox_keep(KEYS[0], KEYS[1], c["p"], rows, cols)
    if c["drop"] == DROP_BUFFER:
        return ops["mask"] != 0
    return np.ones((rows, cols), dtype=bool)


def _scale(c):
    return 1.0 / (1.0 - float(np.float32(c["p"]))) if c["drop"] != DROP_NONE else 1.0


@functools.lru_cache(maxsize=None)
def reference(key):
    """float64 results of the case: name -> dict(ref, S (the |.|-sums of the bound), L (Lipschitz factor), K, keep (None: all
    kept), ulps)."""
    c = _BY_ID[key]
    ops = operands(key)
    f8 = np.float64
    q = _bf16 if c["prec"] else (lambda a: a)
    res = {}
    r = c["route"]
    if r in ("fwd", "seg"):
        if r == "fwd":
            x, w = q(ops["x"]).astype(f8), q(ops["w"]).astype(f8)
            z, S, K = x @ w.T, np.abs(x) @ np.abs(w).T, c["in_dim"]
        else:
            wrap, cd = c["wrap"], c["cd"]
            x, adv, w = ops["x"].astype(f8), ops["adv"].astype(f8), ops["w"].astype(f8)
            idx = np.arange(c["rows"]) % wrap
            z = (x @ w[:, :cd].T)[idx] + adv @ w[:, cd:].T
            S = (np.abs(x) @ np.abs(w[:, :cd]).T)[idx] + np.abs(adv) @ np.abs(w[:, cd:]).T
            K = c["in_dim"]
        if "bias" in ops:
            z, S = z + ops["bias"].astype(f8), S + np.abs(ops["bias"].astype(f8))
        if c["addm"]:
            am = ops["addm"].astype(f8)[np.arange(c["rows"]) % c["wrap"]]
            z, S = z + am, S + np.abs(am)
        keep = _keep(c, c["rows"], c["out_dim"], ops)
        L = np.ones_like(z)
        ulps = EPI_ULPS
        if c["act"] == ACT_LEAKY:
            y = np.where(z > 0, z, LEAKY * z) * np.where(keep, _scale(c), 0.0)
            L = L * _scale(c)
        elif c["act"] == ACT_SIGMOID:
            y = 1.0 / (1.0 + np.exp(-z))
            L, ulps = L * 0.25, SIG_ULPS
        else:
            y = z
        if c["acc"]:
            y, S = y + ops["c0_y"].astype(f8), S + np.abs(ops["c0_y"].astype(f8))
        res["y"] = dict(ref=y, S=S, L=L, K=K, keep=keep if c["act"] == ACT_LEAKY and c["drop"] else None, ulps=ulps)
    if r == "bwd" or c["rider"]:
        if r == "split":
            dy = ops["dy"][c["rows"] - c["wrap"]:]
        else:
            dy = ops["dy"]
        dyq, w = q(dy).astype(f8), q(ops["w"]).astype(f8)[:, c["col0"]:c["col0"] + c["ncols"]]
        d, S = dyq @ w, np.abs(dyq) @ np.abs(w)
        nrows = d.shape[0]
        keep = _keep(c, nrows, c["ncols"], ops)
        if c["act"] == ACT_LEAKY:
            h = ops["h"].astype(f8)
            fp = np.where(keep, _scale(c), 0.0) * np.where(h > 0, 1.0, LEAKY)
        elif c["act"] == ACT_SIGMOID:
            h = ops["h"].astype(f8)
            fp = h * (1.0 - h)
        else:
            fp = np.ones_like(d)
        dx = d * fp
        L = np.abs(fp)
        if c["act"] == ACT_LEAKY:
            L = np.where(keep, _scale(c), 0.0)
        if c["acc"]:
            dx, S = dx + ops["c0_dx"].astype(f8), S + np.abs(ops["c0_dx"].astype(f8))
        res["dx"] = dict(ref=dx, S=S, L=L, K=c["out_dim"], keep=keep if c["act"] == ACT_LEAKY and c["drop"] else None, ulps=EPI_ULPS)
    if r in ("wg", "split"):
        dy = ops["dy"].astype(f8)
        dyq = q(ops["dy"]).astype(f8)
        if c["dw"]:
            if r == "wg":
                x = q(ops["x"]).astype(f8)
                dw, S, K = dyq.T @ x, np.abs(dyq).T @ np.abs(x), c["rows"]
            else:
                wrap, cd = c["wrap"], c["cd"]
                x, adv = ops["x"].astype(f8), ops["adv"].astype(f8)
                a1 = dy[:wrap] + (dy[wrap:] if c["rows"] == 2 * wrap else 0.0)
                s1 = np.abs(dy[:wrap]) + (np.abs(dy[wrap:]) if c["rows"] == 2 * wrap else 0.0)
                dw = np.concatenate([a1.T @ x, dy.T @ adv], axis=1)
                S = np.concatenate([s1.T @ np.abs(x), np.abs(dy).T @ np.abs(adv)], axis=1)
                K = c["rows"] + 1
            if c["acc"]:
                dw, S = dw + ops["c0_dw"].astype(f8), S + np.abs(ops["c0_dw"].astype(f8))
            res["dw"] = dict(ref=dw, S=S, L=np.ones_like(dw), K=K, keep=None, ulps=0)
        if c["db"]:
            db, S = dy.sum(axis=0), np.abs(dy).sum(axis=0)       # the bias gradient sums the float32 dy (the loader's values)
            if c["acc"]:
                db, S = db + ops["c0_db"].astype(f8), S + np.abs(ops["c0_db"].astype(f8))
            res["db"] = dict(ref=db, S=S, L=np.ones_like(db), K=c["rows"], keep=None, ulps=0)
    return res


def criterion(got, ref, S, L, K, keep=None, ulps=EPI_ULPS):
    """(rigorous-bound violations, rms of |got - ref| / S over the kept elements, worst ratio to the bound).  Rigorous per
    element: |got - ref| <= L (K + 2) 2^-24 S + ulps 2^-24 |ref| + tiny -- the bound of a float32 sum of K + 2 terms in any
    summation order (products exact: fma chains, or bf16 x bf16), the epilogue's roundings in ulps of the result."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    bound = L * (K + 2) * U * S + ulps * U * np.abs(ref) + TINY
    k = np.ones(ref.shape, dtype=bool) if keep is None else keep
    bad = int(np.count_nonzero((err > bound) & k))
    if keep is not None:
        bad += int(np.count_nonzero(got[~k] != ref[~k]))          # dropped: exactly 0 (or exactly the accumulated value)
    sel = k & (S > 0)
    rel = err[sel] / S[sel]
    rms = float(np.sqrt(np.mean(rel * rel))) if rel.size else 0.0
    worst = float(np.max(err[k] / bound[k])) if np.any(k) else 0.0
    ulps_used = float(np.max((err[k] - (L * (K + 2) * U * S)[k]) / np.maximum(U * np.abs(ref[k]), 1e-300))) if np.any(k) else 0.0
    return bad, rms, worst, ulps_used


def assert_criterion(got, r, prec, msg):
    bad, rms, worst, ulps_used = criterion(got, r["ref"], r["S"], r["L"], r["K"], r["keep"], r["ulps"])
    lim = BF16_RMS_LIM if prec else F32_RMS_LIM
    print("GEMMSTAT %s prec=%d rms=%.3e worst_bound_ratio=%.3e ulps=%.2f" % (msg, prec, rms, worst, ulps_used))
    assert bad == 0, "%s: %d elements outside the float64 bound (worst ratio %.3g)" % (msg, bad, worst)
    assert rms <= lim, "%s: rms(|err| / S) %.3e over the limit %.1e" % (msg, rms, lim)


_BY_ID = {c["id"]: c for c in MATRIX}


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the matrix and the criterion
# ---------------------------------------------------------------------------------------------------------------------
def _expected_or_invalid(c):
    try:
        return expected_counts(c)
    except Invalid:
        return None


def test_matrix_reaches_every_instantiation():
    """The union of the slots the cases expect is every compiled instantiation, minus the named unreachable ones."""
    alls = compiled_slots()
    assert len(alls) == 95 + 4 + 2 + 6
    reached = set()
    for c in MATRIX:
        e = _expected_or_invalid(c)
        assert (e is None) == c["invalid"], c["id"]
        if e is not None:
            reached |= {s for s, n in enumerate(e) if n}
    assert reached <= set(alls), sorted(reached - set(alls))
    assert sorted(set(alls) - reached) == sorted(UNREACHED), (sorted(set(alls) - reached), sorted(UNREACHED))


def test_split_slab_counts_never_differ():
    """linear_backward_weight_split zeroes its slabs when ns2 < ns1 (eng_gemm_f32.hip).  That cannot happen: with
    kc1 = ceil32(ceil(wrap / n)) and ns1 = ceil(wrap / kc1), wrap <= ns1 kc1, so kc2 = ceil32(ceil(2 wrap / ns1)) <= 2 kc1 and
    kc2 (ns1 - 1) <= 2 kc1 (ns1 - 1) < 2 wrap: ns2 >= ns1 (and ns2 <= ns1 since kc2 >= 2 wrap / ns1).  One half: ns2 == ns1
    trivially.  Exhaustively over every wrap up to 5e4 and every slab request the knob can make."""
    for wrap in range(1, 50001, 7):
        for wgs in (1024, 4096, 1 << 20):
            for out, cd, da in ((256, 425, 58), (1, 1, 1)):
                for rows in (wrap, 2 * wrap):
                    ns1, _, ns2, _ = split_slabs(rows, wrap, out, cd, da, dict(KNOBS, tn_split_wgs=wgs))
                    assert ns2 == ns1, (wrap, wgs, rows)


def test_expected_counts_model_the_launcher():
    """Spot checks of the dispatch model against hand-derived cases."""
    # 16-byte loadable forward at M > 64: 64 x 64 with the compiled-in epilogues
    c = case("fwd", 16384, 512, 512, ACT_LEAKY, DROP_PHILOX)
    assert expected_counts(c)[slot(NT, 64, 64, 1, 1, 0, A_LP)] == 1
    # M <= 64: 128-row tiles; N = 58 -> 64 columns, N = 256 -> 128
    assert expected_counts(case("fwd", 64, 33, 58))[slot(NT, 128, 64, 1, 1, 0, A_RT)] == 1
    assert expected_counts(case("fwd", 64, 33, 256))[slot(NT, 128, 128, 1, 1, 0, A_RT)] == 1
    # 4-byte W rows (pitch 483) without unaligned loads: the residency model, 187 columns -> bn 64, 384 tiles -> 64-row tiles
    c = case("fwd", 16384, 483, 187, knobs=dict(gemm_unaligned=0))
    assert pick_bn(187) == 64 and expected_counts(c)[slot(NT, 64, 64, 0, 0, 0, A_RT)] == 1
    # bn 128 and more than 768 64-row tiles but at most 512 128-row tiles: 128-row tiles (0.55 x 2 > 1)
    c = case("fwd", 64 * 385, 512, 256, knobs=dict(gemm_tiles_big=1))
    assert expected_counts(c)[slot(NT, 128, 128, 1, 1, 0, A_RT)] == 1
    # backward-data with W columns from col0 = 425 of a 483 pitch: 4-byte B loader
    c = case("bwd", 16384, 483, 256, col0=425, ncols=58)
    assert expected_counts(c)[slot(NN, 64, 64, 1, 0, 0, A_RT)] == 1
    # weight gradient 512 x 512 over 16384 frames: 64 tiles, 8 slabs of 2048 frames, one reduce4
    assert wgrad_slabs(16384, 512, 512, True, KNOBS) == (8, 2048)
    e = expected_counts(case("wg", 16384, 512, 512))
    assert e[slot(TN, 64, 64, 1, 1, 0, A_RT)] == 1 and e[REDUCE4] == 1 and sum(e) == 2
    # nslab cut by the rounding: 16417 frames over 64 slabs -> chunks of 288 -> 58 slabs
    assert wgrad_slabs(16384 + 33, 512, 512, True, dict(KNOBS, tn_wgs=4096)) == (58, 288)
    # odd out x in: slab_reduce + slab_reduce_small; db only: column sums
    e = expected_counts(case("wg", 513, 63, 65))
    assert e[REDUCE] == 1 and e[REDUCE_SMALL] == 1 and e[slot(TN, 128, 64, 0, 0, 0, A_RT)] == 1
    e = expected_counts(case("wg", 700, 64, 187, dw=False))
    assert e[COLSUM_PARTIAL] == 1 and e[COLSUM_FINALIZE] == 1 and sum(e) == 2
    # pair: rides when M > 64 on 64 x 64 tiles; the Philox flavour; at 60 rows it does not
    e = expected_counts(case("wg", 3000, 256, 128, ACT_LEAKY, DROP_PHILOX, rider=1))
    assert e[PAIR + 1] == 1 and e[REDUCE4] == 1 and sum(e) == 2
    e = expected_counts(case("wg", 60, 64, 64, ACT_LEAKY, DROP_PHILOX, rider=1))
    assert e[PAIR + 1] == 0 and e[slot(NN, 128, 64, 1, 1, 0, A_RT)] == 1
    # split layer cfg2: 4 x (7 + 1) tiles -> 32 slabs requested, 16384 / 256 = 64 allowed, chunks of 512 / 1024
    assert split_slabs(32768, 16384, 256, 425, 58, KNOBS) == (32, 512, 32, 1024)
    e = expected_counts(case("split", 32768, 483, 256, wrap=16384, cd=425, ld=dict(x=428, adv=60, dx=58), rider=1, col0=425, ncols=58,
                             defer=1))
    assert e[TN_PAIR + 1] == 1 and e[REDUCE_MULTI] == 1 and sum(e) == 2
    # two-segment forward: wrap <= 64 routes to 128-row tiles -> invalid; bf16 -> invalid
    with pytest.raises(Invalid):
        expected_counts(case("seg", 128, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=64, cd=425))
    assert expected_counts(case("seg", 65, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=65, cd=425))[slot(NT, 64, 64, 1, 1, 0, A_SEG)] == 1
    assert expected_counts(case("seg", 130, 483, 256, ACT_LEAKY, DROP_PHILOX, wrap=65, cd=425))[slot(NT, 64, 64, 1, 1, 0, A_SEG)] == 1


def test_philox_matches_the_random123_known_answer():
    """Counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8 (Random123 kat_vectors, philox4x32_10)."""
    w = [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert w == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], ["%08x" % v for v in w]
    # and the keep bits are a function of the element only: rows 16 g + 4 h + s share a counter, p = 0.5 keeps about half
    k = philox_keep(*KEYS, 0.5, 64, 300)
    assert 0.45 < k.mean() < 0.55
    assert philox_thresh(0.3) == int(float(np.float32(0.3)) * 65536 + 0.5)


def test_criterion_rejects_mutations():
    """The acceptance criterion fails a result with one element off by twice its bound, one missing 32-deep K slice, one
    missing slab, or bf16 operands truncated instead of rounded."""
    rs = np.random.RandomState(3)
    M, K, N = 70, 200, 50
    a, b = rs.randn(M, K).astype(np.float32), rs.randn(K, N).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    S = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    L = np.ones_like(ref)
    good = (a @ b).astype(np.float32)
    assert criterion(good, ref, S, L, K)[0] == 0
    bad = good.astype(np.float64).copy()
    bound = (K + 2) * U * S[5, 7] + EPI_ULPS * U * abs(ref[5, 7]) + TINY
    bad[5, 7] = ref[5, 7] + 2 * bound
    assert criterion(bad, ref, S, L, K)[0] == 1
    # a missing K slice (k 64..95) and a missing slab of frames
    sl = good - (a[:, 64:96] @ b[64:96, :])
    assert criterion(sl, ref, S, L, K)[0] > 0
    dy, x = rs.randn(1000, 30).astype(np.float32), rs.randn(1000, 20).astype(np.float32)
    dwr = dy.astype(np.float64).T @ x.astype(np.float64)
    Sw = np.abs(dy).astype(np.float64).T @ np.abs(x).astype(np.float64)
    lost = dy[:768].T @ x[:768]                   # slabs of 256 frames, the last one lost
    assert criterion(lost, dwr, Sw, np.ones_like(dwr), 1000)[0] > 0
    # bf16: truncation instead of round-to-nearest-even fails the criterion on the rounded operands
    def trunc(v):
        return (np.ascontiguousarray(v).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    aq, bq = _bf16(a).astype(np.float64), _bf16(b).astype(np.float64)
    refq, Sq = aq @ bq, np.abs(aq) @ np.abs(bq)
    assert criterion((aq @ bq).astype(np.float32), refq, Sq, L, K)[0] == 0
    assert criterion(trunc(a).astype(np.float64) @ trunc(b).astype(np.float64), refq, Sq, L, K)[0] > 0
    # dropped elements must be exactly zero
    keep = np.ones(ref.shape, dtype=bool)
    keep[3, 4] = False
    z = good.astype(np.float64).copy()
    z[3, 4] = 1e-30
    r0 = ref.copy()
    r0[3, 4] = 0.0
    assert criterion(z, r0, S, L, K, keep)[0] == 1


def test_gemm_hook_rejects_malformed_cases():
    import ctypes as Ct
    from gantts_amd import _lib as Lb
    lib = Lb.lib
    assert lib.gt_op_gemm_f32(None, None) == Lb.GT_ERR_INVALID
    assert lib.gt_gemm_path_counts(None, 0) == Lb.GT_OK
    fake = Ct.c_void_p(16)        # never dereferenced: every case below is refused before any launch

    def mk(**kw):
        g = Lb.GemmCase()
        g.route, g.rows, g.in_dim, g.out_dim = Lb.GEMM_ROUTE_FORWARD, 100, 64, 64
        g.ldx = g.ldw = g.ldy = g.ld_dy = g.ld_dx = g.ldh = g.ld_mask = g.ld_addm = g.ld_adv = 64
        g.x = g.w = g.y = g.dy = g.dx = g.dw = g.db = g.adv = fake
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    bad = [mk(route=7), mk(route=-1), mk(prec=2), mk(rows=0), mk(act=3), mk(drop=1, act=0, p=0.5), mk(drop=1, act=1, p=1.0),
           mk(drop=2, act=1, p=0.5), mk(x=None), mk(addm=fake, wrap=0), mk(addm=fake, wrap=10),
           mk(route=Lb.GEMM_ROUTE_FORWARD_SEG, wrap=30, cd=10), mk(route=Lb.GEMM_ROUTE_FORWARD_SEG, wrap=100, cd=64),
           mk(route=Lb.GEMM_ROUTE_FORWARD_SEG, wrap=50, cd=10, adv=None),
           mk(route=Lb.GEMM_ROUTE_BACKWARD_DATA, col0=10, ncols=60), mk(route=Lb.GEMM_ROUTE_BACKWARD_DATA, ncols=0),
           mk(route=Lb.GEMM_ROUTE_BACKWARD_DATA, ncols=64, dy=None), mk(route=Lb.GEMM_ROUTE_BACKWARD_DATA, ncols=64, act=2),
           mk(route=Lb.GEMM_ROUTE_WEIGHT_GRAD, dw=None, db=None), mk(route=Lb.GEMM_ROUTE_WEIGHT_GRAD, x=None),
           mk(route=Lb.GEMM_ROUTE_WEIGHT_GRAD, rider=1, ncols=64, col0=1),
           mk(route=Lb.GEMM_ROUTE_WEIGHT_GRAD_SPLIT, wrap=60, cd=10), mk(route=Lb.GEMM_ROUTE_WEIGHT_GRAD_SPLIT, wrap=100, cd=0),
           mk(route=Lb.GEMM_ROUTE_WEIGHT_GRAD_SPLIT, wrap=50, cd=10, dw=None)]
    for i, g in enumerate(bad):
        assert lib.gt_op_gemm_f32(Ct.byref(g), None) == Lb.GT_ERR_INVALID, i
    counts = (Ct.c_int64 * Lb.GEMM_PATH_SLOTS)()
    assert lib.gt_gemm_path_counts(counts, 1) == Lb.GT_OK


# ---------------------------------------------------------------------------------------------------------------------
# the kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
SENT = np.float32(-7.25e33)


class _Buf:
    """A device buffer holding one operand at (offset, pitch): `pad` everywhere else, `extra` rows behind it."""

    def __init__(self, rows, cols, ld, off, pad, data=None, extra=2):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.host = np.full(off + (rows + extra) * ld, pad, dtype=np.float32)
        if data is not None:
            self.view(self.host)[...] = data
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 256 == 0

    def view(self, flat):
        return flat[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * self.off

    def mask(self):
        m = np.zeros(self.host.shape, dtype=bool)
        self.view(m)[...] = True
        return m

    def got(self):
        flat = self.dev.cpu().numpy()
        return flat, self.view(flat).copy()


def _set_knobs(kn):
    from gantts_amd import _lib as Lb
    for k, v in kn.items():
        Lb.check(Lb.lib.gt_set_tuning(k.encode(), int(v)))


def run_case(c, knobs=None, defer=None):
    """Builds the buffers, runs the hook with the census reset; returns (rc, counts, {name: (flat, logical, buf)})."""
    import ctypes as Ct
    from gantts_amd import _lib as Lb
    ops = operands(c["id"])
    shapes = _shapes(c)
    nan = np.float32(np.nan)
    bufs = {}
    for name, (r, n) in shapes.items():
        ld, off = c["ld"][name], c["off"].get(name, 0)
        if name in ("y", "dx"):
            bufs[name] = _Buf(r, n, ld, off, SENT, ops.get("c0_" + name, np.full((r, n), nan, np.float32)))
        else:
            bufs[name] = _Buf(r, n, ld, off, nan, ops[name])
    if c["route"] in ("wg", "split"):
        if c["dw"]:
            bufs["dw"] = _Buf(c["out_dim"], c["in_dim"], c["in_dim"], c["off"].get("dw", 0), SENT,
                              ops.get("c0_dw", np.full((c["out_dim"], c["in_dim"]), nan, np.float32)), extra=1)
        if c["db"]:
            bufs["db"] = _Buf(1, c["out_dim"], c["out_dim"], 0, SENT, ops.get("c0_db", np.full(c["out_dim"], nan, np.float32))[None], extra=1)
    bias = torch.from_numpy(ops["bias"]).cuda() if "bias" in ops else None
    g = Lb.GemmCase()
    g.route = dict(fwd=0, seg=1, bwd=2, wg=3, split=4)[c["route"]]
    g.prec, g.rows, g.in_dim, g.out_dim, g.act, g.drop, g.p = c["prec"], c["rows"], c["in_dim"], c["out_dim"], c["act"], c["drop"], c["p"]
    g.key0, g.key1 = KEYS
    g.accumulate, g.col0, g.ncols, g.wrap, g.cd, g.rider = c["acc"], c["col0"], c["ncols"], c["wrap"], c["cd"], c["rider"]
    g.defer = c["defer"] if defer is None else defer
    for name in ("x", "w", "y", "dy", "h", "mask", "addm", "adv", "dx"):
        setattr(g, "ld" + name if name in ("x", "w", "y", "h") else "ld_" + name, c["ld"][name])
        if name in bufs:
            setattr(g, name, bufs[name].ptr)
    for name in ("dw", "db"):
        if name in bufs:
            setattr(g, name, bufs[name].ptr)
    if bias is not None:
        g.bias = bias.data_ptr()
    kn = dict(KNOBS)
    kn.update(c["knobs"])
    kn.update(knobs or {})
    counts = (Ct.c_int64 * Lb.GEMM_PATH_SLOTS)()
    torch.cuda.synchronize()
    _set_knobs(kn)
    try:
        Lb.check(Lb.lib.gt_gemm_path_counts(None, 1))
        rc = Lb.lib.gt_op_gemm_f32(Ct.byref(g), Ct.c_void_p(torch.cuda.current_stream().cuda_stream))
        Lb.check(Lb.lib.gt_gemm_path_counts(counts, 1))
    finally:
        _set_knobs(KNOBS)
    torch.cuda.synchronize()
    out = {}
    for name in ("y", "dx", "dw", "db"):
        if name in bufs:
            flat, logical = bufs[name].got()
            out[name] = (flat, logical, bufs[name])
    return rc, list(counts), out


def _check_sentinels(name, flat, buf, tag):
    m = buf.mask()
    outside = flat[~m]
    assert np.array_equal(outside.view(np.uint32), np.full(outside.shape, SENT).view(np.uint32)), "%s: %s written outside its result" % (tag, name)
    inside = flat[m]
    assert not np.isnan(inside).any(), "%s: %s has %d NaN" % (tag, name, int(np.isnan(inside).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("c", MATRIX, ids=[c["id"] for c in MATRIX])
def test_gemm_case_vs_float64(c):
    from gantts_amd import _lib as Lb
    tag = c["id"]
    rc, counts, out = run_case(c)
    if c["invalid"]:
        assert rc == Lb.GT_ERR_INVALID and sum(counts) == 0, (tag, rc, {i: n for i, n in enumerate(counts) if n})
        return
    assert rc == Lb.GT_OK, "%s: %s" % (tag, Lb.lib.gt_last_error())
    exp = expected_counts(c)
    assert counts == exp, "%s: launches %s, expected %s" % (tag, {i: n for i, n in enumerate(counts) if n}, {i: n for i, n in enumerate(exp) if n})
    ref = reference(tag)
    assert sorted(ref) == sorted(out), (tag, sorted(ref), sorted(out))
    for name, (flat, logical, buf) in out.items():
        _check_sentinels(name, flat, buf, tag)
        got = logical.reshape(-1) if name == "db" else logical
        assert_criterion(got, ref[name], c["prec"], "%s %s" % (tag, name))
    # determinism: a second run is bit-identical
    rc2, _, out2 = run_case(c)
    assert rc2 == Lb.GT_OK
    for name in out:
        assert np.array_equal(out[name][0].view(np.uint32), out2[name][0].view(np.uint32)), "%s: %s differs between two runs" % (tag, name)


_PAIRS = [c for c in MATRIX if c["route"] == "wg" and c["rider"] and "pair" in c["id"]]
_DEFERS = [c for c in MATRIX if c["defer"]]


@pytest.mark.gpu
@pytest.mark.parametrize("c", _PAIRS, ids=[c["id"] for c in _PAIRS])
def test_pair_launch_matches_separate_launches(c):
    """The pair kernel (both orders) runs the same tile code with the same k_chunk as two separate launches: bit-identical."""
    from gantts_amd import _lib as Lb
    results = []
    for kn in (dict(gemm_pair=0), dict(gemm_pair=1, pair_order=1), dict(gemm_pair=1, pair_order=0)):
        rc, counts, out = run_case(c, knobs=kn)
        assert rc == Lb.GT_OK
        results.append((kn, counts, out))
    assert sum(results[0][1][PAIR:PAIR + 4]) == 0
    for kn, counts, out in results[1:]:
        for name in results[0][2]:
            assert np.array_equal(out[name][0].view(np.uint32), results[0][2][name][0].view(np.uint32)), "%s %s: %s" % (c["id"], kn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("c", _DEFERS, ids=[c["id"] for c in _DEFERS])
def test_deferred_combine_matches_immediate(c):
    """slab_reduce_multi_kernel runs slab_reduce4_body: the deferred combine equals the immediate one bit for bit."""
    from gantts_amd import _lib as Lb
    rc0, c0, out0 = run_case(c, defer=0)
    rc1, c1, out1 = run_case(c, defer=1)
    assert rc0 == rc1 == Lb.GT_OK and c0[REDUCE_MULTI] == 0
    for name in out0:
        assert np.array_equal(out0[name][0].view(np.uint32), out1[name][0].view(np.uint32)), "%s: %s" % (c["id"], name)
