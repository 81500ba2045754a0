"""Every bf16-storage product instantiation and image builder against float64.

The bf16-storage family (gantts_amd/csrc/gemm_bf16s.hip.h) is reached through launch_gemm_b16 and weight_grad_b16
(eng_gemm_b16.hip), which choose one of 44 product kernels -- {forward, backward-data} x 5 epilogue flavours x 4 tile forms, plus
the slab form x 4 tile forms -- from the shape, the tuning knobs, K % 64 and the bias-gradient rider.  gt_op_gemm_b16 runs one
product through that dispatch on images it builds in NaN-filled buffers, gt_op_cast_image runs one image builder, and
gt_gemm_b16_path_counts counts the launches per kernel, so each case asserts WHICH kernel ran (against `expected_counts`, a
restatement of the dispatch rules) as well as what it computed.

Products: census; sentinels around C and in the pads of Cb / CbT bit for bit; no NaN (a read of a poisoned pad shows here); dropped
elements exactly zero where the numpy Philox stream (or the buffer mask) says so; kept elements against float64 arithmetic on the
bf16-rounded operands with the deterministic float32-sum bound of tests/test_gpu_gemm_f32.py; Cb == RNE bf16 of the float32 result
bit for bit and CbT == Cb^T.  Image builders are exact: float32 arithmetic in numpy, RNE to bf16, compared as 16-bit integers.

Measured on the MI355X over the whole matrix (profiles/gemm_b16_parity.md): worst ratio to the deterministic bound 0.143, worst
rms(|err| / S) 1.93e-8 (both fwd-77x70x1-f0-k) against BF16_RMS_LIM = 1.2e-7 of the float32 suite, which is used here unchanged.
"""
import collections
import ctypes as Ct
import functools
import zlib

import numpy as np
import pytest
import torch

from test_gpu_gemm_f32 import (ACT_LEAKY, ACT_NONE, ACT_SIGMOID, BF16_RMS_LIM, COLSUM_FINALIZE, DROP_BUFFER, DROP_NONE, DROP_PHILOX,
                               EPI_ULPS, KEYS, LEAKY, REDUCE, REDUCE4, REDUCE_SMALL, SENT, SIG_ULPS, TINY, U, cdiv,
                               criterion, philox_keep)

FWD, BWD, SLAB = 0, 1, 2
A_NONE, A_PHILOX, A_BUFFER, A_LEAKY, A_SIGMOID = 0, 1, 2, 3, 4
NSLOTS = 66
CAST_F32, CAST_BF16, CAST_SEQDROP, CAST_MULTI, CAST_CAT, CAST_CATDROP = 60, 61, 62, 63, 64, 65
KNOBS = dict(b16_tiles=0, b16_wg_tile=0, b16_dma=1)          # GtTuning defaults
FORM_KNOBS = {0: dict(b16_tiles=64), 1: dict(b16_tiles=128, b16_dma=0), 2: dict(b16_tiles=128), 3: dict(b16_tiles=256)}
CUS = 256
PAD16 = 0xABCD                                                # sentinel of the 16-bit images' pads
NAN16 = 0xFFFF                                                # bf16 NaN: what the images hold before the launch


def slot(epi, amode, form):
    return (epi * 5 + amode) * 4 + form


def pad8(n):
    return cdiv(n, 8) * 8


def compiled_slots():
    """The instantiations of launch_gemm_b16 (GT_B16_CASE: two routes x five flavours, and the slab form), each in four tile forms,
    and the six image builders."""
    out = {slot(e, a, f) for e in (FWD, BWD) for a in range(5) for f in range(4)} | {slot(SLAB, A_NONE, f) for f in range(4)}
    return sorted(out | {CAST_F32, CAST_BF16, CAST_SEQDROP, CAST_MULTI, CAST_CAT, CAST_CATDROP})


UNREACHED = {}


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch rules (eng_gemm_b16.hip) restated
# ---------------------------------------------------------------------------------------------------------------------
def amode_of(act, drop):
    if act == ACT_SIGMOID:
        return A_SIGMOID
    if act == ACT_LEAKY:
        return {DROP_PHILOX: A_PHILOX, DROP_BUFFER: A_BUFFER, DROP_NONE: A_LEAKY}[drop]
    return A_NONE


def launch_form(epi, M, N, K, nslab, kn, tile=0, k_chunk=0, rowsum=False):
    """launch_gemm_b16: 0 64 x 64, 1 128 x 128 register loader, 2 128 x 128 LDS-DMA, 3 256 x 256 LDS-DMA."""
    t128 = cdiv(M, 128) * cdiv(N, 128) * nslab
    ft = kn["b16_tiles"]
    if tile:
        big = tile >= 128
    else:
        big = False if ft == 64 else (epi != SLAB and M >= 128 and N >= 128 and (ft >= 128 or t128 >= 2 * CUS))
    dma = kn["b16_dma"] != 0 and big and K % 64 == 0 and (epi != SLAB or (k_chunk % 64 == 0 and not rowsum))
    t256 = cdiv(M, 256) * cdiv(N, 256) * nslab
    if tile:
        huge = tile == 256
    else:
        rounds = cdiv(t256, CUS) * CUS
        huge = ft == 256 or (ft == 0 and epi != SLAB and M >= 256 and N >= 256 and t256 >= CUS and (rounds - t256) <= 0.15 * rounds)
    huge = dma and huge
    return 3 if huge else 2 if dma else 1 if big else 0


def wgrad_plan(rows, out, in_, db, kn):
    """weight_grad_b16: (tile handed to launch_gemm_b16, nslab, k_chunk)."""
    f = kn["b16_wg_tile"]
    t128, t256 = cdiv(out, 128) * cdiv(in_, 128), cdiv(out, 256) * cdiv(in_, 256)
    big = (f >= 128) if f else (out >= 128 and in_ >= 128 and t128 >= 16)
    huge = big and not db and rows % 64 == 0 and ((f == 256) if f else (out >= 512 and in_ >= 512 and t256 >= 32))
    if big:
        slots, tl = (CUS, t256) if huge else (2 * CUS, t128)
        best, nslab = 2.0, 1
        for r in (1, 2, 3):
            ns = max(1, slots * r // tl)
            waste = 1.0 - tl * ns / (slots * cdiv(tl * ns, slots)) + 0.05 * (r - 1)
            if waste < best - 1e-9:
                best, nslab = waste, ns
    else:
        nslab = max(1, 1024 // (cdiv(out, 64) * cdiv(in_, 64)))
    nslab = min(nslab, max(1, rows // 512))
    k_chunk = cdiv(cdiv(rows, nslab), 64) * 64
    return (256 if huge else 128 if big else 64), cdiv(rows, k_chunk), k_chunk


def expected_counts(c):
    """(launches per slot of gt_gemm_b16_path_counts, {slot of gt_gemm_path_counts: combine launches}) of one gt_op_gemm_b16 call."""
    kn = dict(KNOBS, **c["knobs"])
    counts, comb = [0] * NSLOTS, collections.Counter()
    M, N, K = c["M"], c["N"], c["K"]
    if c["route"] == "wg":              # M = out, N = in, K = rows; both operands become transposed images
        counts[CAST_F32] += 2
        tile, nslab, k_chunk = wgrad_plan(K, M, N, c["db"], kn)
        counts[slot(SLAB, A_NONE, launch_form(SLAB, M, N, K, nslab, kn, tile, k_chunk, c["db"]))] += 1
        if (M * N) % 4 == 0:            # can4: dw is 16-byte aligned in every case here
            comb[REDUCE4] += 1
        else:
            comb[REDUCE] += 1
            if c["db"]:
                comb[REDUCE_SMALL] += 1
    else:
        epi = FWD if c["route"] == "fwd" else BWD
        counts[CAST_F32] += 2 + (1 if epi == BWD and c["act"] != ACT_NONE else 0)
        counts[slot(epi, amode_of(c["act"], c["drop"]), launch_form(epi, M, N, K, 1, kn))] += 1
    return counts, dict(comb)


# ---------------------------------------------------------------------------------------------------------------------
# the product matrix
# ---------------------------------------------------------------------------------------------------------------------
ALL3 = ("c", "cb", "cbt")


def case(route, M, N, K, act=ACT_NONE, drop=DROP_NONE, p=0.5, acc=0, outs=ALL3, form=None, ldc=None, c_off=0, ldcb=None, ldcbt=None, db=True,
         knobs=None, tag=""):
    """fwd: M rows, N = out, K = in;  bwd: M rows, N = in, K = out;  wg: M = out, N = in, K = rows."""
    kn = dict(FORM_KNOBS[form]) if form is not None else {}
    kn.update(knobs or {})
    c = dict(route=route, M=M, N=N, K=K, act=act, drop=drop, p=p, acc=acc, outs=tuple(outs) if route != "wg" else (), form=form,
             ldc=N if ldc is None else ldc, c_off=c_off, ldcb=pad8(N) if ldcb is None else ldcb, ldcbt=pad8(M) if ldcbt is None else ldcbt,
             db=bool(db) and route == "wg", knobs=kn)
    c["id"] = "%s-%dx%dx%d%s%s%s%s%s%s" % (route, M, N, K, "-a%d" % act if act else "", "-d%d" % drop if drop else "", "-acc" if acc else "",
                                         "-f%d" % form if form is not None else "", "-" + "+".join(outs) if route != "wg" and tuple(outs) != ALL3 else "",
                                         "-" + tag if tag else "")
    return c


EPILOGUES = [(ACT_NONE, DROP_NONE), (ACT_LEAKY, DROP_NONE), (ACT_LEAKY, DROP_BUFFER), (ACT_LEAKY, DROP_PHILOX), (ACT_SIGMOID, DROP_NONE)]
# the unaligned result of a full tile: the issue's "ldc = 187" cannot hold a 256-wide row; 256 + 187 keeps ldc % 4 == 3
EL = dict(ldc=256 + 187, c_off=1, ldcb=256 + 3, ldcbt=256 + 4)


def _matrix():
    c = []
    # K handling, register loader (forms 0 and 1): K = 1, a tail inside a 16-byte chunk, one stage, a second stage of 8, several stages
    for K in (1, 25, 64, 72, 200):
        for route in ("fwd", "bwd"):
            c.append(case(route, 77, 70, K, form=0, tag="k"))
            c.append(case(route, 130, 200, K, form=1, tag="k"))
    # K handling, LDS-DMA forms: one stage, two, three (the 2-stage ring wraps)
    for K in (64, 128, 192):
        for route in ("fwd", "bwd"):
            c.append(case(route, 130, 200, K, form=2, tag="k"))
            c.append(case(route, 295, 260, K, form=3, tag="k"))
    # M / N edges
    c.append(case("fwd", 1, 1, 40, tag="edge"))
    c.append(case("bwd", 1, 1, 40, ACT_SIGMOID, tag="edge"))
    for form in (1, 2, 3):
        c.append(case("fwd", 130, 200, 64, ACT_LEAKY, form=form, tag="edge"))
        c.append(case("bwd", 295, 260, 64, form=form, tag="edge"))
    # one full tile: staged epilogue (16-byte aligned results, ldc % 4 == 0), and the element-wise epilogue on the same tile
    for form in (0, 1, 2, 3):
        c.append(case("fwd", 256, 256, 64, ACT_LEAKY, DROP_PHILOX, form=form, tag="staged"))
        c.append(case("bwd", 256, 256, 64, ACT_LEAKY, DROP_PHILOX, p=0.3, form=form, tag="unaligned", **EL))
    c.append(case("fwd", 256, 256, 64, form=3, ldc=256 + 187, tag="ldc"))
    c.append(case("fwd", 256, 256, 64, form=2, c_off=1, tag="coff"))
    # outputs
    for outs in (("c",), ("cb", "cbt"), ("cbt",)):
        c.append(case("fwd", 77, 70, 25, ACT_LEAKY, DROP_BUFFER, outs=outs, form=0))
        c.append(case("bwd", 130, 200, 72, ACT_SIGMOID, outs=outs, form=1))
        c.append(case("fwd", 256, 256, 128, ACT_SIGMOID, outs=outs, form=3))
        c.append(case("bwd", 295, 260, 64, ACT_LEAKY, DROP_PHILOX, outs=outs, form=2))
    # accumulate: staged tile and edge tiles, C pre-filled with random values
    c.append(case("fwd", 256, 256, 64, ACT_LEAKY, DROP_PHILOX, acc=1, outs=("c",), form=2, tag="staged"))
    c.append(case("bwd", 256, 256, 128, acc=1, outs=("c",), form=3, tag="staged"))
    c.append(case("fwd", 77, 70, 25, ACT_SIGMOID, acc=1, outs=("c",), form=0, tag="edge"))
    c.append(case("bwd", 130, 200, 72, ACT_LEAKY, DROP_BUFFER, acc=1, outs=("c",), form=1, tag="edge"))
    # every flavour in forward and backward-data in each form; the Philox rows cross 16-row groups and both lane halves, N > 256
    for i, (act, drop) in enumerate(EPILOGUES):
        for j, route in enumerate(("fwd", "bwd")):
            p = 0.5 if (i + j) % 2 == 0 else 0.3
            c.append(case(route, 16 * 9 + 7, 260, 40, act, drop, p, form=0, tag="epi"))
            c.append(case(route, 295, 260, 72, act, drop, p, form=1, tag="epi"))
            c.append(case(route, 295, 260, 64, act, drop, 0.8 - p, form=2, tag="epi"))
            c.append(case(route, 295, 260, 128, act, drop, p, form=3, tag="epi"))
    # the shape rules without a forced form
    c.append(case("fwd", 300, 264, 72, ACT_LEAKY, DROP_PHILOX, tag="default"))
    # weight gradients (M = out, N = in, K = rows)
    for rows in (1, 63, 300, 1100):
        c.append(case("wg", 33, 7, rows, knobs=dict(b16_wg_tile=64), tag="odd"))               # odd slab_stride: slab_reduce + slab_reduce_small
        c.append(case("wg", 130, 136, rows, knobs=dict(b16_wg_tile=64), tag="t64"))
        c.append(case("wg", 130, 136, rows, knobs=dict(b16_wg_tile=128), tag="t128"))          # register loader with the row-sum rider
    c.append(case("wg", 300, 264, 1100, knobs=dict(b16_wg_tile=128), tag="t128"))
    c.append(case("wg", 300, 264, 1100, knobs=dict(b16_wg_tile=256), tag="t256-db"))           # db given: no 256 form, 128 x 128 register loader
    c.append(case("wg", 130, 136, 1152, db=False, knobs=dict(b16_wg_tile=128), tag="dma128"))
    c.append(case("wg", 300, 264, 1152, db=False, knobs=dict(b16_wg_tile=128), tag="dma128"))
    c.append(case("wg", 130, 136, 1152, db=False, knobs=dict(b16_wg_tile=256), tag="dma256"))
    c.append(case("wg", 300, 264, 1152, db=False, knobs=dict(b16_wg_tile=256), tag="dma256"))
    c.append(case("wg", 300, 264, 1152, db=False, knobs=dict(b16_wg_tile=256, b16_dma=0), tag="nodma"))
    c.append(case("wg", 130, 136, 1100, db=False, knobs=dict(b16_wg_tile=128), tag="tail-nodb"))   # rows % 64 != 0: register loader
    c.append(case("wg", 130, 136, 300, acc=1, knobs=dict(b16_wg_tile=64), tag="t64"))
    c.append(case("wg", 33, 7, 1100, acc=1, knobs=dict(b16_wg_tile=64), tag="odd"))
    c.append(case("wg", 300, 264, 1152, acc=1, db=False, knobs=dict(b16_wg_tile=256), tag="dma256"))
    c.append(case("wg", 130, 136, 1100, tag="default"))
    return c


MATRIX = _matrix()
_seen = collections.Counter()
for _c in MATRIX:
    _seen[_c["id"]] += 1
    assert _seen[_c["id"]] == 1, _c["id"]
_BY_ID = {c["id"]: c for c in MATRIX}


# ---------------------------------------------------------------------------------------------------------------------
# bf16 in numpy, operands, float64 references, the checker
# ---------------------------------------------------------------------------------------------------------------------
def bf16_bits(a):
    """RNE rounding of float32 to bf16, as 16-bit integers (finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bits_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def q16(a):
    return bits_f32(bf16_bits(a))


def _ordinal(b):
    """bf16 bit patterns on a line: neighbours differ by one (+0 and -0 coincide)."""
    b = np.asarray(b, dtype=np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def _shapes(c):
    M, N, K = c["M"], c["N"], c["K"]
    if c["route"] == "fwd":
        s = dict(x=(M, K), w=(N, K))
    elif c["route"] == "bwd":
        s = dict(dy=(M, K), w=(K, N))
        if c["act"] != ACT_NONE:
            s["h"] = (M, N)
    else:
        return dict(dy=(K, M), x=(K, N))
    if c["drop"] == DROP_BUFFER:
        s["mask"] = (M, N)
    return s


@functools.lru_cache(maxsize=None)
def operands(key):
    c = _BY_ID[key]
    rs = np.random.RandomState(zlib.crc32(key.encode()))
    ops = {}
    for name, (r, n) in _shapes(c).items():
        if name == "mask":
            ops[name] = (rs.rand(r, n) >= c["p"]).astype(np.float32)
        elif name == "h":
            ops[name] = (rs.rand(r, n) if c["act"] == ACT_SIGMOID else rs.randn(r, n)).astype(np.float32)
        elif name == "w":
            ops[name] = (rs.randn(r, n) / np.sqrt(c["K"])).astype(np.float32)
        else:
            ops[name] = rs.randn(r, n).astype(np.float32)
    if c["route"] == "fwd":
        ops["bias"] = rs.randn(c["N"]).astype(np.float32)
    if c["acc"]:
        ops["c0"] = rs.randn(c["M"], c["N"]).astype(np.float32)
        ops["c0_db"] = rs.randn(c["M"]).astype(np.float32)
    return ops


def reference_of(c, ops):
    """name -> dict(ref, S, L, K, keep, ulps) in float64 on the bf16-rounded operands (criterion of test_gpu_gemm_f32.py)."""
    f8 = np.float64
    M, N, K = c["M"], c["N"], c["K"]
    res = {}
    if c["route"] == "wg":
        dy, x = q16(ops["dy"]).astype(f8), q16(ops["x"]).astype(f8)
        dw, S = dy.T @ x, np.abs(dy).T @ np.abs(x)
        db, Sb = dy.sum(axis=0), np.abs(dy).sum(axis=0)       # the loader sums the bf16 values it multiplies
        if c["acc"]:
            dw, S = dw + ops["c0"].astype(f8), S + np.abs(ops["c0"].astype(f8))
            db, Sb = db + ops["c0_db"].astype(f8), Sb + np.abs(ops["c0_db"].astype(f8))
        res["dw"] = dict(ref=dw, S=S, L=np.ones_like(dw), K=K, keep=None, ulps=0)
        if c["db"]:
            res["db"] = dict(ref=db, S=Sb, L=np.ones_like(db), K=K - 2, keep=None, ulps=0)      # rows U sum|dy|
        return res
    scale = 1.0 / (1.0 - float(np.float32(c["p"]))) if c["drop"] != DROP_NONE else 1.0
    if c["drop"] == DROP_PHILOX:
        keep = philox_keep(KEYS[0], KEYS[1], c["p"], M, N)
    elif c["drop"] == DROP_BUFFER:
        keep = ops["mask"] != 0
    else:
        keep = np.ones((M, N), dtype=bool)
    ulps = EPI_ULPS
    if c["route"] == "fwd":
        x, w, b = q16(ops["x"]).astype(f8), q16(ops["w"]).astype(f8), ops["bias"].astype(f8)
        z, S = x @ w.T + b, np.abs(x) @ np.abs(w).T + np.abs(b)
        L = np.ones_like(z)
        if c["act"] == ACT_LEAKY:
            y, L = np.where(z > 0, z, LEAKY * z) * np.where(keep, scale, 0.0), L * scale
        elif c["act"] == ACT_SIGMOID:
            y, L, ulps = 1.0 / (1.0 + np.exp(-z)), L * 0.25, SIG_ULPS
        else:
            y = z
    else:
        dy, w = q16(ops["dy"]).astype(f8), q16(ops["w"]).astype(f8)
        d, S = dy @ w, np.abs(dy) @ np.abs(w)
        if c["act"] == ACT_LEAKY:
            h = q16(ops["h"]).astype(f8)
            fp = np.where(keep, scale, 0.0) * np.where(h > 0, 1.0, LEAKY)
            L = np.where(keep, scale, 0.0)
        elif c["act"] == ACT_SIGMOID:
            h = q16(ops["h"]).astype(f8)
            fp = h * (1.0 - h)
            L = np.abs(fp)
        else:
            fp = np.ones_like(d)
            L = fp
        y = d * fp
    y0 = y
    if c["acc"]:
        y, S = y + ops["c0"].astype(f8), S + np.abs(ops["c0"].astype(f8))
    res["c"] = dict(ref=y, S=S, L=L, K=K, keep=keep if c["act"] == ACT_LEAKY and c["drop"] else None, ulps=ulps, ref_image=y0)
    return res


@functools.lru_cache(maxsize=None)
def reference(key):
    return reference_of(_BY_ID[key], operands(key))


STATS = []


def check_tensor(tag, name, got, r):
    """Failure strings of one float32 result against its float64 reference (the deterministic bound; rms reported and limited)."""
    fails = []
    got = np.asarray(got)
    if np.isnan(got).any():
        return ["%s: %s has %d NaN" % (tag, name, int(np.isnan(got).sum()))]
    bad, rms, worst, ulps_used = criterion(got, r["ref"], r["S"], r["L"], r["K"], r["keep"], r["ulps"])
    STATS.append((tag, name, rms, worst))
    print("GEMMB16STAT %s %s rms=%.3e worst_bound_ratio=%.3e ulps=%.2f" % (tag, name, rms, worst, ulps_used))
    if bad:
        fails.append("%s: %s has %d elements outside the float64 bound (worst ratio %.3g)" % (tag, name, bad, worst))
    if rms > BF16_RMS_LIM:
        fails.append("%s: %s rms(|err| / S) %.3e over the limit %.1e" % (tag, name, rms, BF16_RMS_LIM))
    return fails


def check_images(tag, r, c32, cb, cbt):
    """Cb is the RNE bf16 of the float32 result bit for bit (float32 result known) or within one bf16 ulp of the bf16 roundings of the
    ends of the float64 interval ref +- bound (C null); CbT == Cb^T; dropped elements are zero."""
    fails = []
    img = cb if cb is not None else (cbt.T if cbt is not None else None)
    if img is None:
        return fails
    if cb is not None and cbt is not None and not np.array_equal(cb, cbt.T):
        fails.append("%s: CbT != Cb^T in %d elements" % (tag, int(np.count_nonzero(cb != cbt.T))))
    nan = (img & 0x7F80) == 0x7F80
    if nan.any():
        return fails + ["%s: the bf16 image has %d NaN / Inf" % (tag, int(nan.sum()))]
    if c32 is not None:
        want = bf16_bits(c32)
        if not np.array_equal(img, want):
            fails.append("%s: the bf16 image is not the RNE rounding of the float32 result in %d elements" % (tag, int(np.count_nonzero(img != want))))
        return fails
    ref = r["ref_image"]
    bound = r["L"] * (r["K"] + 2) * U * r["S"] + r["ulps"] * U * np.abs(ref) + TINY
    lo, hi = _ordinal(bf16_bits((ref - bound).astype(np.float32))) - 1, _ordinal(bf16_bits((ref + bound).astype(np.float32))) + 1
    k = _ordinal(img)
    out = (k < lo) | (k > hi)
    if r["keep"] is not None:
        out = np.where(r["keep"], out, k != 0)
    if out.any():
        fails.append("%s: the bf16 image is further than one bf16 ulp from the float64 reference in %d elements" % (tag, int(out.sum())))
    return fails


def pads_intact(flat, inside, sentinel):
    """flat: the whole buffer; inside: bool mask of the result's elements; everything else still holds the sentinel's bits."""
    outside = np.asarray(flat)[~inside]
    if outside.dtype == np.float32:
        return np.array_equal(outside.view(np.uint32), np.full(outside.shape, sentinel, np.float32).view(np.uint32))
    return bool(np.all(outside == sentinel))


# ---------------------------------------------------------------------------------------------------------------------
# host checks of the matrix, the model and the checker
# ---------------------------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_instantiation():
    alls = compiled_slots()
    assert len(alls) == 44 + 6
    reached = {CAST_BF16, CAST_SEQDROP, CAST_MULTI, CAST_CAT, CAST_CATDROP} & {s for cc in CAST_CASES for s in [CAST_SLOT[cc["kind"]]]}
    combines = set()
    for c in MATRIX:
        counts, comb = expected_counts(c)
        reached |= {s for s, n in enumerate(counts) if n}
        combines |= set(comb)
        if c["form"] is not None:       # a forced form is taken: the case runs the kernel its id names
            epi = FWD if c["route"] == "fwd" else BWD
            assert counts[slot(epi, amode_of(c["act"], c["drop"]), c["form"])] == 1, c["id"]
    assert reached <= set(alls), sorted(reached - set(alls))
    assert sorted(set(alls) - reached) == sorted(UNREACHED), (sorted(set(alls) - reached), sorted(UNREACHED))
    assert combines == {REDUCE4, REDUCE, REDUCE_SMALL}
    assert any(cc.get("colsum") is not None for cc in CAST_CASES)


def test_expected_counts_model_the_launcher():
    """Spot checks of the dispatch model against hand-derived cases."""
    # the production shapes: 32768 x 512 x 1024 forward fills 2 x 256 CUs with 128-tiles (1024) and whole rounds of 256-tiles (256)
    assert launch_form(FWD, 32768, 512, 1024, 1, KNOBS) == 3
    assert launch_form(FWD, 8192, 1024, 2048, 1, KNOBS) == 2        # 128 256-tiles < 256 CUs: 128 x 128 LDS-DMA
    assert launch_form(FWD, 8192, 1024, 2040, 1, KNOBS) == 1        # K % 64 != 0: register loader
    assert launch_form(FWD, 4096, 512, 1024, 1, KNOBS) == 0         # 128 128-tiles < 512
    # a forced form is taken when legal (M, N >= 128, not the slab route; 256 needs the DMA conditions), else the next smaller one
    kn = dict(KNOBS, b16_tiles=256)
    assert launch_form(FWD, 130, 200, 64, 1, kn) == 3 and launch_form(FWD, 130, 200, 72, 1, kn) == 1 and launch_form(FWD, 127, 200, 64, 1, kn) == 0
    assert launch_form(BWD, 130, 200, 64, 1, dict(KNOBS, b16_tiles=128)) == 2
    assert launch_form(BWD, 130, 200, 64, 1, dict(KNOBS, b16_tiles=128, b16_dma=0)) == 1
    # weight gradients: slabs of at least 512 frames, k_chunk a multiple of 64
    assert wgrad_plan(1100, 130, 136, True, dict(KNOBS, b16_wg_tile=128)) == (128, 2, 576)
    assert wgrad_plan(300, 33, 7, True, dict(KNOBS, b16_wg_tile=64)) == (64, 1, 320)
    assert wgrad_plan(1152, 300, 264, False, dict(KNOBS, b16_wg_tile=256)) == (256, 2, 576)
    assert wgrad_plan(1100, 300, 264, True, dict(KNOBS, b16_wg_tile=256))[0] == 128       # db rides in the register loader only
    assert wgrad_plan(32768, 1024, 3072, False, KNOBS)[0] == 256 and wgrad_plan(32768, 512, 2048, True, KNOBS)[0] == 128
    e, comb = expected_counts(case("wg", 33, 7, 1100, knobs=dict(b16_wg_tile=64)))
    assert e[slot(SLAB, A_NONE, 0)] == 1 and e[CAST_F32] == 2 and comb == {REDUCE: 1, REDUCE_SMALL: 1}
    e, comb = expected_counts(case("wg", 300, 264, 1152, db=False, knobs=dict(b16_wg_tile=256)))
    assert e[slot(SLAB, A_NONE, 3)] == 1 and comb == {REDUCE4: 1}
    e, _ = expected_counts(case("bwd", 295, 260, 64, ACT_LEAKY, DROP_PHILOX, form=2))
    assert e[slot(BWD, A_PHILOX, 2)] == 1 and e[CAST_F32] == 3 and sum(e) == 4


def test_bf16_rounding_is_round_to_nearest_even():
    a = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39, 0.0, 65504.0], dtype=np.float32)      # ties: to even
    want = torch.from_numpy(a).bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(bf16_bits(a), want)
    rs = np.random.RandomState(1)
    b = (rs.randn(10000) * np.exp(rs.randn(10000) * 5)).astype(np.float32)
    assert np.array_equal(bf16_bits(b), torch.from_numpy(b).bfloat16().view(torch.int16).numpy().view(np.uint16))
    assert np.array_equal(_ordinal(np.array([0x0000, 0x8000, 0x0001, 0x8001], np.uint16)), [0, 0, 1, -1])


def _emulate(c, ops, keep=None, k_extra=None):
    """The kernel's arithmetic in numpy float32 (any summation order is inside the bound): (float32 result, image bits)."""
    r = reference_of(c, ops)["c"]
    x, w = q16(ops["x"]), q16(ops["w"])
    z = (x @ w.T).astype(np.float32)
    if k_extra is not None:
        z = z + k_extra
    z = z + ops["bias"]
    keep = r["keep"] if keep is None else keep
    y = np.where(z > 0, z, np.float32(0.01) * z) * np.where(keep, np.float32(1.0 / (1.0 - c["p"])), np.float32(0)) if c["act"] == ACT_LEAKY else z
    y = y.astype(np.float32)
    return (y + ops["c0"] if c["acc"] else y).astype(np.float32), bf16_bits(y)


def test_criterion_rejects_mutations():
    """The checker passes a numpy emulation of the kernel and rejects: a transposed 8 x 8 block of CbT, one Philox half (lane >> 5)
    swapped, the masked K tail included, an image that is bf16(ref) instead of bf16(float32 result), a pad element overwritten,
    accumulate ignored."""
    rs = np.random.RandomState(5)
    M, N, K = 296, 300, 25
    c = case("fwd", M, N, K, ACT_LEAKY, DROP_PHILOX, tag="mutation")
    ops = dict(x=rs.randn(M, K).astype(np.float32), w=(rs.randn(N, K) / 5).astype(np.float32), bias=rs.randn(N).astype(np.float32))
    r = reference_of(c, ops)["c"]

    def verdict(c32, cb, cbt, ref=r):
        return check_tensor("m", "c", c32, ref) + check_images("m", ref, c32, cb, cbt) if c32 is not None else check_images("m", ref, None, cb, cbt)

    good, bits = _emulate(c, ops)
    assert verdict(good, bits, bits.T.copy()) == []
    assert verdict(None, bits, bits.T.copy()) == []
    # a transposed 8 x 8 block of the transposed image
    t = bits.T.copy()
    t[8:16, 24:32] = t[8:16, 24:32].T.copy()
    assert any("CbT != Cb^T" in f for f in verdict(good, bits, t))
    # one Philox half swapped: rows 4 h .. 4 h + 3 of every 8 take the other half's words
    swapped = r["keep"][np.arange(M) ^ 4]
    y2, b2 = _emulate(c, ops, keep=swapped)
    assert verdict(y2, b2, b2.T.copy()) and verdict(None, b2, None)
    # the masked K tail included: the poisoned pad (NaN), or any finite pad content
    y3, b3 = _emulate(c, ops, k_extra=np.float32(np.nan))
    assert any("NaN" in f for f in verdict(y3, b3, b3.T.copy())) and any("NaN" in f for f in verdict(None, b3, None))
    tail = (rs.randn(M, 7).astype(np.float32) @ rs.randn(7, N).astype(np.float32)) / 5
    y3, b3 = _emulate(c, ops, k_extra=tail)
    assert verdict(y3, b3, b3.T.copy())
    # an image rounded from the float64 reference instead of from the float32 result
    bref = bf16_bits(r["ref"].astype(np.float32))
    assert np.count_nonzero(bref != bits) > 0
    assert any("not the RNE rounding" in f for f in verdict(good, bref, bref.T.copy()))
    assert verdict(None, bref, bref.T.copy()) == []          # ... which is within one ulp when no float32 result exists to compare with
    # truncation instead of RNE is not
    btr = (good.view(np.uint32) >> 16).astype(np.uint16)
    assert verdict(good, btr, btr.T.copy())
    # a pad element overwritten
    flat = np.full(M * pad8(N) + 16, PAD16, np.uint16)
    inside = np.zeros(flat.shape, bool)
    inside[:M * pad8(N)].reshape(M, pad8(N))[:, :N] = True
    assert pads_intact(flat, inside, PAD16)
    flat[pad8(N) * 3 + N] = bits[3, 0]
    assert not pads_intact(flat, inside, PAD16)
    fl = np.full(40, SENT, np.float32)
    ins = np.zeros(40, bool)
    ins[4:30] = True
    assert pads_intact(fl, ins, SENT)
    fl[31] = 0.0
    assert not pads_intact(fl, ins, SENT)
    # accumulate ignored
    ca = case("fwd", M, N, K, ACT_LEAKY, DROP_PHILOX, acc=1, outs=("c",), tag="mutation")
    opa = dict(ops, c0=rs.randn(M, N).astype(np.float32))
    ra = reference_of(ca, opa)["c"]
    ya, _ = _emulate(ca, opa)
    assert check_tensor("m", "c", ya, ra) == []
    assert check_tensor("m", "c", good, ra)


def _mk_b16(Lb, **kw):
    fake = Ct.c_void_p(4096)          # never dereferenced: every case below is refused before any launch
    g = Lb.GemmB16Case()
    g.route, g.rows, g.in_dim, g.out_dim = Lb.GEMM_ROUTE_FORWARD, 100, 64, 64
    g.ldx = g.ldw = g.ld_dy = g.ldh = g.ld_mask = g.ldc = g.ldcb = 64
    g.ldcbt = 104
    g.x = g.w = g.dy = g.c = g.cb = g.cbt = g.dw = fake
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def test_hooks_reject_malformed_cases():
    from gantts_amd import _lib as Lb
    lib = Lb.lib
    assert lib.gt_op_gemm_b16(None, None) == Lb.GT_ERR_INVALID
    assert lib.gt_op_cast_image(None, None) == Lb.GT_ERR_INVALID
    assert lib.gt_gemm_b16_path_counts(None, 1) == Lb.GT_OK
    P = Ct.c_void_p
    bad = [_mk_b16(Lb, route=7), _mk_b16(Lb, route=Lb.GEMM_ROUTE_FORWARD_SEG), _mk_b16(Lb, route=-1),        # unknown route
           _mk_b16(Lb, x=P(4098)), _mk_b16(Lb, c=P(4097)), _mk_b16(Lb, cb=P(4097)), _mk_b16(Lb, cbt=P(4100)),   # misaligned operands / results
           _mk_b16(Lb, ldcbt=102), _mk_b16(Lb, ldcbt=96),                                                      # ldcbt % 4 != 0, ldcbt < rows
           _mk_b16(Lb, rows=0), _mk_b16(Lb, act=3), _mk_b16(Lb, drop=1, act=0), _mk_b16(Lb, drop=2, act=1, p=0.5), _mk_b16(Lb, drop=1, act=1, p=1.0),
           _mk_b16(Lb, x=None), _mk_b16(Lb, c=None, cb=None, cbt=None), _mk_b16(Lb, accumulate=1, c=None), _mk_b16(Lb, ldc=63),
           _mk_b16(Lb, route=Lb.GEMM_ROUTE_BACKWARD_DATA, dy=None), _mk_b16(Lb, route=Lb.GEMM_ROUTE_BACKWARD_DATA, act=2),
           _mk_b16(Lb, route=Lb.GEMM_ROUTE_WEIGHT_GRAD, dw=None), _mk_b16(Lb, route=Lb.GEMM_ROUTE_WEIGHT_GRAD, act=1)]
    for i, g in enumerate(bad):
        assert lib.gt_op_gemm_b16(Ct.byref(g), None) == Lb.GT_ERR_INVALID, i
        assert lib.gt_last_error(), i
    assert lib.gt_op_gemm_b16(Ct.byref(bad[0]), None) == Lb.GT_ERR_INVALID and b"unknown route" in lib.gt_last_error()
    assert lib.gt_op_gemm_b16(Ct.byref(bad[3]), None) == Lb.GT_ERR_INVALID and b"misaligned" in lib.gt_last_error()
    assert lib.gt_op_gemm_b16(Ct.byref(bad[7]), None) == Lb.GT_ERR_INVALID and b"multiple of 4" in lib.gt_last_error()

    def mkc(**kw):
        g = Lb.CastCase()
        g.kind, g.rows, g.cols, g.ldi, g.ldo, g.ldt = Lb.CAST_PLAIN_F32, 10, 12, 12, 16, 16
        g.in_ = g.out = g.outT = P(4096)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    badc = [mkc(kind=6), mkc(kind=-1), mkc(rows=0), mkc(out=None, outT=None), mkc(ldo=11), mkc(ldt=9), mkc(in_=None), mkc(in_=P(4098)),
            mkc(out=P(4097)), mkc(kind=Lb.CAST_SEQDROP), mkc(kind=Lb.CAST_SEQDROP, mul=P(4096), T=0), mkc(kind=Lb.CAST_PLAIN_BF16, colsum=P(4096)),
            mkc(kind=Lb.CAST_CAT, cd=4, N=10), mkc(kind=Lb.CAST_CAT, cd=13, x=P(4096), N=10),
            mkc(kind=Lb.CAST_CAT, cd=12, x=P(4096), N=5, row_off=1), mkc(kind=Lb.CAST_MULTI, n_jobs=0), mkc(kind=Lb.CAST_MULTI, n_jobs=9),
            mkc(kind=Lb.CAST_MULTI, n_jobs=1)]
    for i, g in enumerate(badc):
        assert lib.gt_op_cast_image(Ct.byref(g), None) == Lb.GT_ERR_INVALID, i
        assert lib.gt_last_error(), i
    counts = (Ct.c_int64 * Lb.GEMM_B16_PATH_SLOTS)()
    assert lib.gt_gemm_b16_path_counts(counts, 1) == Lb.GT_OK and sum(counts) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the product kernels against float64
# ---------------------------------------------------------------------------------------------------------------------
class _F32:
    """A float32 device matrix at (offset, pitch): `pad` everywhere else, two rows behind it."""

    def __init__(self, data, ld, off, pad, shape=None):
        rows, cols = data.shape if shape is None else shape
        self.rows, self.cols, self.ld, self.off = rows, cols, ld, off
        self.host = np.full(off + (rows + 2) * ld, pad, dtype=np.float32)
        self.view(self.host)[...] = data
        self.dev = torch.from_numpy(self.host).cuda()

    def view(self, flat):
        return flat[self.off:self.off + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.dev.data_ptr() + 4 * self.off

    def inside(self):
        m = np.zeros(self.host.shape, dtype=bool)
        self.view(m)[...] = True
        return m

    def got(self):
        flat = self.dev.cpu().numpy()
        return flat, self.view(flat).copy()


class _I16:
    """A 16-bit device image [rows][ld]: bf16 NaN inside (so an element the kernel does not write shows), PAD16 in the pads and in two
    rows behind it."""

    def __init__(self, rows, cols, ld, data=None, fill=NAN16):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.host = np.full((rows + 2) * ld, PAD16, dtype=np.uint16)
        self.view(self.host)[...] = fill if data is None else data
        self.dev = torch.from_numpy(self.host.view(np.int16)).cuda()

    def view(self, flat):
        return flat[:self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.cols]

    @property
    def ptr(self):
        return self.dev.data_ptr()

    def inside(self):
        m = np.zeros(self.host.shape, dtype=bool)
        self.view(m)[...] = True
        return m

    def got(self):
        flat = self.dev.cpu().numpy().view(np.uint16)
        return flat, self.view(flat).copy()


def _set_knobs(kn):
    from gantts_amd import _lib as Lb
    for k, v in kn.items():
        Lb.check(Lb.lib.gt_set_tuning(k.encode(), int(v)))


def _stream():
    return Ct.c_void_p(torch.cuda.current_stream().cuda_stream)


def _census(fn, knobs):
    """Runs fn() with the knobs set and both censuses reset; (rc, b16 counts, combine counts of gt_gemm_path_counts)."""
    from gantts_amd import _lib as Lb
    b16 = (Ct.c_int64 * Lb.GEMM_B16_PATH_SLOTS)()
    f32 = (Ct.c_int64 * Lb.GEMM_PATH_SLOTS)()
    torch.cuda.synchronize()
    _set_knobs(dict(KNOBS, **knobs))
    try:
        Lb.check(Lb.lib.gt_gemm_b16_path_counts(None, 1))
        Lb.check(Lb.lib.gt_gemm_path_counts(None, 1))
        rc = fn()
        Lb.check(Lb.lib.gt_gemm_b16_path_counts(b16, 1))
        Lb.check(Lb.lib.gt_gemm_path_counts(f32, 1))
    finally:
        _set_knobs(KNOBS)
    torch.cuda.synchronize()
    return rc, list(b16), {i: n for i, n in enumerate(f32) if n}


def run_product(c):
    from gantts_amd import _lib as Lb
    ops = operands(c["id"])
    nan = np.float32(np.nan)
    M, N, K = c["M"], c["N"], c["K"]
    ins = {name: _F32(ops[name], ops[name].shape[1] + 3, 1 if name in ("x", "dy") else 0, nan) for name in _shapes(c)}
    g = Lb.GemmB16Case()
    g.route = dict(fwd=Lb.GEMM_ROUTE_FORWARD, bwd=Lb.GEMM_ROUTE_BACKWARD_DATA, wg=Lb.GEMM_ROUTE_WEIGHT_GRAD)[c["route"]]
    g.rows, g.in_dim, g.out_dim = (K, N, M) if c["route"] == "wg" else (M, K, N) if c["route"] == "fwd" else (M, N, K)
    g.act, g.drop, g.p, g.accumulate = c["act"], c["drop"], c["p"], c["acc"]
    g.key0, g.key1 = KEYS
    for name, fld in (("x", "ldx"), ("w", "ldw"), ("dy", "ld_dy"), ("h", "ldh"), ("mask", "ld_mask")):
        if name in ins:
            setattr(g, name, ins[name].ptr)
            setattr(g, fld, ins[name].ld)
    keepalive = [ins]
    if "bias" in ops:
        bias = torch.from_numpy(ops["bias"]).cuda()
        keepalive.append(bias)
        g.bias = bias.data_ptr()
    outs = {}
    if c["route"] == "wg":
        outs["dw"] = _F32(ops["c0"] if c["acc"] else np.full((M, N), nan, np.float32), N, 0, SENT)
        g.dw = outs["dw"].ptr
        if c["db"]:
            outs["db"] = _F32((ops["c0_db"] if c["acc"] else np.full(M, nan, np.float32))[None], M, 0, SENT)
            g.db = outs["db"].ptr
    else:
        if "c" in c["outs"]:
            outs["c"] = _F32(ops["c0"] if c["acc"] else np.full((M, N), nan, np.float32), c["ldc"], c["c_off"], SENT)
            g.c, g.ldc = outs["c"].ptr, c["ldc"]
        if "cb" in c["outs"]:
            outs["cb"] = _I16(M, N, c["ldcb"])
            g.cb, g.ldcb = outs["cb"].ptr, c["ldcb"]
        if "cbt" in c["outs"]:
            outs["cbt"] = _I16(N, M, c["ldcbt"])
            g.cbt, g.ldcbt = outs["cbt"].ptr, c["ldcbt"]
    rc, b16, comb = _census(lambda: Lb.lib.gt_op_gemm_b16(Ct.byref(g), _stream()), c["knobs"])
    return rc, b16, comb, {name: b.got() + (b,) for name, b in outs.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("c", MATRIX, ids=[c["id"] for c in MATRIX])
def test_product_case_vs_float64(c):
    from gantts_amd import _lib as Lb
    tag = c["id"]
    rc, b16, comb, out = run_product(c)
    assert rc == Lb.GT_OK, "%s: %s" % (tag, Lb.lib.gt_last_error())
    exp, exp_comb = expected_counts(c)
    assert b16 == exp, "%s: launches %s, expected %s" % (tag, {i: n for i, n in enumerate(b16) if n}, {i: n for i, n in enumerate(exp) if n})
    assert comb == exp_comb, "%s: combines %s, expected %s" % (tag, comb, exp_comb)
    ref = reference(tag)
    fails = []
    for name, (flat, logical, buf) in out.items():
        if not pads_intact(flat, buf.inside(), SENT if flat.dtype == np.float32 else PAD16):
            fails.append("%s: %s written outside its result" % (tag, name))
    if c["route"] == "wg":
        fails += check_tensor(tag, "dw", out["dw"][1], ref["dw"])
        if c["db"]:
            fails += check_tensor(tag, "db", out["db"][1].reshape(-1), ref["db"])
    else:
        c32 = out["c"][1] if "c" in out else None
        if c32 is not None:
            fails += check_tensor(tag, "c", c32, ref["c"])
        if not c["acc"]:
            fails += check_images(tag, ref["c"], c32, out["cb"][1] if "cb" in out else None, out["cbt"][1] if "cbt" in out else None)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# the image builders: exact
# ---------------------------------------------------------------------------------------------------------------------
CAST_SLOT = dict(f32=CAST_F32, bf16=CAST_BF16, seqdrop=CAST_SEQDROP, multi=CAST_MULTI, cat=CAST_CAT, catdrop=CAST_CATDROP)
IDX = [0, 1, 2, 5, 6, 7, 8, 9, 20, 21, 22, 29]          # gathered feature columns, with gaps; feats are 30 wide


def ccase(kind, rows, cols, ldi=None, in_off=0, ldo=None, ldt=None, out=True, outT=True, colsum=None, tag="", **kw):
    c = dict(kind=kind, rows=rows, cols=cols, ldi=cols if ldi is None else ldi, in_off=in_off, ldo=pad8(cols) if ldo is None else ldo,
             ldt=pad8(rows) if ldt is None else ldt, out=out, outT=outT, colsum=colsum, **kw)
    c["id"] = "%s-%dx%d%s" % (kind, rows, cols, "-" + tag if tag else "")
    return c


def _cast_cases():
    c = []
    for rows, cols in ((64, 64), (128, 192)):
        c.append(ccase("f32", rows, cols, tag="aligned"))                                  # vector read, 16-byte stores
        c.append(ccase("f32", rows, cols, ldi=cols + 1, in_off=1, tag="scalar-read"))      # base offset by one float, odd pitch
    c.append(ccase("f32", 65, 70, tag="ragged"))
    c.append(ccase("f32", 1, 1, tag="ragged"))
    c.append(ccase("f32", 64, 70, ldo=70, ldt=68, tag="unaligned-stores"))
    c.append(ccase("f32", 128, 64, ldo=70, ldt=132, tag="unaligned-stores-full-tiles"))
    c.append(ccase("f32", 128, 192, outT=False, tag="out-only"))
    c.append(ccase("f32", 65, 70, out=False, tag="outT-only"))
    c.append(ccase("f32", 3 * 64 - 11, 70, colsum=0, tag="colsum"))
    c.append(ccase("f32", 3 * 64, 128, colsum=1, tag="colsum-acc"))
    c.append(ccase("bf16", 130, 72, ldi=80))
    c.append(ccase("seqdrop", 5 * 19, 70, T=19))                                           # sequences straddle the 64-row tile boundary
    for cd in (20, 0):
        c.append(ccase("cat", 2 * 69, cd + len(IDX), N=69, row_off=0, cd=cd, tag="cd%d-both" % cd))
        c.append(ccase("cat", 69, cd + len(IDX), N=69, row_off=69, cd=cd, tag="cd%d-generated" % cd))
        c.append(ccase("catdrop", 2 * 69, cd + len(IDX), N=69, row_off=0, cd=cd, T=23, tag="cd%d-both" % cd))   # two row groups, own table rows
    c.append(ccase("catdrop", 69, 20 + len(IDX), N=69, row_off=69, cd=20, T=23, tag="cd20-generated"))
    c.append(ccase("multi", 0, 0, jobs=[(64, 64, 64, 0), (33, 7, 7, 0), (130, 72, 73, 1)], tag="3jobs"))      # (rows, cols, ldi, in_off)
    c.append(ccase("multi", 0, 0, jobs=[(65, 70, 70, 0)], tag="1job"))
    return c


CAST_CASES = _cast_cases()


def _cast_source(c, rs):
    """(device inputs by name, expected float32 matrix or bits)."""
    kind, rows, cols = c["kind"], c["rows"], c["cols"]
    dev, want_bits = {}, None
    if kind in ("f32", "seqdrop"):
        src = (rs.randn(rows, cols) * np.exp(rs.randn(rows, cols))).astype(np.float32)
        dev["in_"] = _F32(src, c["ldi"], c["in_off"], np.float32(np.nan))
        val = src
    elif kind == "bf16":
        want_bits = bf16_bits(rs.randn(rows, cols).astype(np.float32))
        dev["in_"] = _I16(rows, cols, c["ldi"], data=want_bits)
        val = None
    else:
        N, cd = c["N"], c["cd"]
        x = rs.randn(N, max(cd, 1)).astype(np.float32)[:, :cd]
        fa, fb = rs.randn(N, 30).astype(np.float32), rs.randn(N, 30).astype(np.float32)
        if cd:
            dev["x"] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        dev["fa"], dev["fb"] = _F32(fa, 31, 0, np.float32(np.nan)), _F32(fb, 31, 0, np.float32(np.nan))
        dev["idx"] = torch.tensor(IDX, dtype=torch.int32).cuda()
        full = np.concatenate([np.concatenate([x, fa[:, IDX]], axis=1), np.concatenate([x, fb[:, IDX]], axis=1)], axis=0)
        val = full[c["row_off"]:c["row_off"] + rows]
    if kind in ("seqdrop", "catdrop"):
        nseq = cdiv(rows, c["T"])
        mul = np.where(rs.rand(nseq, cols) < 0.3, 0.0, rs.randn(nseq, cols) + 2.0).astype(np.float32)
        dev["mul"] = torch.from_numpy(mul).cuda()
        val = (val.astype(np.float32) * mul[np.arange(rows) // c["T"]]).astype(np.float32)      # one float32 product
    return dev, (bf16_bits(val) if want_bits is None else want_bits), val


def _ptr(v):
    return v.ptr if hasattr(v, "ptr") else v.data_ptr()


@pytest.mark.gpu
@pytest.mark.parametrize("c", CAST_CASES, ids=[c["id"] for c in CAST_CASES])
def test_image_builder_is_exact(c):
    from gantts_amd import _lib as Lb
    rs = np.random.RandomState(zlib.crc32(c["id"].encode()))
    g = Lb.CastCase()
    g.kind = dict(f32=Lb.CAST_PLAIN_F32, bf16=Lb.CAST_PLAIN_BF16, seqdrop=Lb.CAST_SEQDROP, cat=Lb.CAST_CAT, catdrop=Lb.CAST_CATDROP,
                  multi=Lb.CAST_MULTI)[c["kind"]]
    checks, keep = [], []
    if c["kind"] == "multi":
        g.n_jobs = len(c["jobs"])
        for i, (rows, cols, ldi, off) in enumerate(c["jobs"]):
            src = rs.randn(rows, cols).astype(np.float32)
            sin, o, t = _F32(src, ldi, off, np.float32(np.nan)), _I16(rows, cols, pad8(cols)), _I16(cols, rows, pad8(rows))
            j = g.jobs[i]
            j.in_, j.out, j.outT, j.rows, j.cols, j.ldi, j.ldo, j.ldt = sin.ptr, o.ptr, t.ptr, rows, cols, ldi, o.ld, t.ld
            keep.append(sin)
            checks += [("job %d out" % i, o, bf16_bits(src)), ("job %d outT" % i, t, bf16_bits(src).T)]
        val = None
    else:
        dev, bits, val = _cast_source(c, rs)
        keep.append(dev)
        g.rows, g.cols, g.ldi, g.ldo, g.ldt = c["rows"], c["cols"], c["ldi"], c["ldo"], c["ldt"]
        for name, v in dev.items():
            setattr(g, name, _ptr(v))
        if c["kind"] in ("cat", "catdrop"):
            g.N, g.row_off, g.cd, g.ldf = c["N"], c["row_off"], c["cd"], 31
        if "T" in c:
            g.T = c["T"]
        if c["out"]:
            o = _I16(c["rows"], c["cols"], c["ldo"])
            g.out = o.ptr
            checks.append(("out", o, bits))
        if c["outT"]:
            t = _I16(c["cols"], c["rows"], c["ldt"])
            g.outT = t.ptr
            checks.append(("outT", t, bits.T))
    cs = None
    if c["colsum"] is not None:
        c0 = rs.randn(c["cols"]).astype(np.float32) if c["colsum"] else np.full(c["cols"], np.nan, np.float32)
        cs = _F32(c0[None], c["cols"], 0, SENT)
        g.colsum, g.colsum_accumulate = cs.ptr, c["colsum"]
    rc, b16, comb = _census(lambda: Lb.lib.gt_op_cast_image(Ct.byref(g), _stream()), {})
    assert rc == Lb.GT_OK, "%s: %s" % (c["id"], Lb.lib.gt_last_error())
    exp = [0] * NSLOTS
    exp[CAST_SLOT[c["kind"]]] = 1
    assert b16 == exp, (c["id"], {i: n for i, n in enumerate(b16) if n})
    assert comb == ({COLSUM_FINALIZE: 1} if cs is not None else {}), (c["id"], comb)
    for name, buf, want in checks:
        flat, got = buf.got()
        assert pads_intact(flat, buf.inside(), PAD16), "%s: %s pad written" % (c["id"], name)
        assert np.array_equal(got, want), "%s: %s differs from the RNE rounding in %d of %d elements" % (c["id"], name, int(np.count_nonzero(got != want)), want.size)
    if cs is not None:
        flat, got = cs.got()
        assert pads_intact(flat, cs.inside(), SENT), "%s: column sums written outside" % c["id"]
        ref, S = val.astype(np.float64).sum(axis=0), np.abs(val.astype(np.float64)).sum(axis=0)
        if c["colsum"]:
            ref, S = ref + c0.astype(np.float64), S + np.abs(c0.astype(np.float64))
        err = np.abs(got.reshape(-1).astype(np.float64) - ref)
        assert not np.isnan(err).any() and np.all(err <= c["rows"] * U * S + TINY), "%s: column sums, worst ratio %.3g" % (
            c["id"], float(np.max(err / (c["rows"] * U * S + TINY))))


# ---------------------------------------------------------------------------------------------------------------------
# the production configuration: bf16 products with the engine's own Philox stream
# ---------------------------------------------------------------------------------------------------------------------
RTOL = 1e-4


def _rel_rms(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    den = float(np.sqrt((b * b).mean())) if b.size else 0.0
    return float(np.sqrt(((a - b) ** 2).mean())) / max(den, 1e-300) if b.size else 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("tag,B,Tn,gh,dh,b16", [("second-half-inside-a-philox-group", 3, 23, 64, 64, True), ("ragged-tiles", 2, 80, 130, 250, False),
                                                ("ragged-tiles-bf16", 2, 80, 136, 248, True)])
def test_bf16_philox_step_equals_the_same_step_with_its_masks_injected(tag, B, Tn, gh, dh, b16):
    """MLP generator and conditioned MLP discriminator, dropout 0.5 in both, matmul_bf16 on.  Run A draws its keep bits in the
    epilogues (B16_A_LEAKY_PHILOX); before each of its two steps the masks of every site are dumped (gt_op_philox_mask).  Run B is a
    fresh engine with the same weights and options and those masks injected (B16_A_LEAKY_BUFFER).  The two runs are the same bf16
    arithmetic and differ in the epilogue flavour only: every output, gradient, parameter and optimizer-state tensor agrees to
    rms(A - B) / rms(B) <= 1e-4 (a last-bit difference flips a bf16 rounding with probability about 2^-16 per element, about 7e-6
    rms; a wrong keep bit in 1 % of a layer costs more than 1e-2), scalars to 1e-4, counts exactly.
    Hidden widths 130 / 250 are not multiples of 8: the engine keeps such a network on float32 products under matmul_bf16 (eng_step.hip:
    use_b16), so that shape compares the float32 flavours; 136 / 248 is the same ragged tiling on the bf16 kernels."""
    import types
    import cases as C
    import gantts_amd.train as T
    from gantts_amd import _lib as L
    from gantts_amd import hparams, optim, paramgen
    from gantts_amd.engine import engine_for
    from gantts_amd.multistream import get_static_features
    from gantts_amd.seqloss import sequence_mask
    from hip_runner import build_model
    N, steps, p = B * Tn, 2, 0.5
    gs = dict(kind="MLP", in_dim=425, out_dim=187, num_hidden=3, hidden_dim=gh, dropout=p, last_sigmoid=False)
    ds = dict(kind="MLP", in_dim=483, out_dim=1, num_hidden=3, hidden_dim=dh, dropout=p, last_sigmoid=True)
    x_np, y_np, lengths = C.make_batch(dict(B=B, T=Tn, din=425, dout=187, stream_sizes=[180, 3, 1, 3]), seed=11)
    hp = types.SimpleNamespace(**hparams.tts_acoustic.values())
    T.hp = hp
    R = torch.from_numpy(np.array(paramgen.unit_variance_mlpg_matrix(hp.windows, Tn))).cuda()
    x, y = torch.from_numpy(x_np).cuda(), torch.from_numpy(y_np).cuda()
    ys = get_static_features(y, 3, hp.stream_sizes, hp.has_dynamic_features)
    mask = sequence_mask(torch.from_numpy(lengths).cuda()).unsqueeze(-1)
    okw = dict(lr=0.01, weight_decay=1e-7, initial_accumulator_value=1e-4)

    def run(inject):
        mg, md = build_model(gs, 1).train(), build_model(ds, 2).train()
        og, od = optim.Adagrad(mg.parameters(), **okw), optim.Adagrad(md.parameters(), **okw)
        eng = engine_for(hp, mg)
        eng.set_option("matmul_bf16", 1)
        eng.set_seed(1234)
        rec, dumped = [], []
        b16 = (Ct.c_int64 * L.GEMM_B16_PATH_SLOTS)()
        L.check(L.lib.gt_gemm_b16_path_counts(None, 1))
        for st in range(steps):
            if inject is None:
                gm = [eng.philox_mask(L.ROLE_G, 0, l, p, N, gh).cpu().view(B, Tn, gh) for l in range(3)]
                d0 = [eng.philox_mask(L.ROLE_D, 0, l, p, 2 * N, dh).cpu() for l in range(3)]
                d2 = [eng.philox_mask(L.ROLE_D, 2, l, p, N, dh).cpu().view(B, Tn, dh) for l in range(3)]
                dumped.append((gm, [m[:N].view(B, Tn, dh) for m in d0], [m[N:].view(B, Tn, dh) for m in d0], d2))
            else:
                gm, dreal, dfake, d2 = inject[st]
                mg.set_dropout_masks(0, gm)
                md.set_dropout_masks(0, dreal), md.set_dropout_masks(1, dfake), md.set_dropout_masks(2, d2)
            og.zero_grad(), od.zero_grad()
            yh, yhs = T.apply_generator(mg, x, R, list(lengths))
            d = T.update_discriminator(md, od, x, ys, yhs, list(lengths), mask, "train")
            dgrad = md.flat_grads().cpu().numpy().copy()
            g = T.update_generator(mg, md, og, x, y, yh, ys, yhs, 1.0, list(lengths), mask, "train", mse_w=0.0, mge_w=1.0)
            t = dict(yh=yh.cpu().numpy(), yhs=yhs.cpu().numpy(), dgrad=dgrad, ggrad=mg.flat_grads().cpu().numpy().copy(),
                     gparam=mg.flat_params().detach().cpu().numpy().copy(), dparam=md.flat_params().detach().cpu().numpy().copy())
            for nm, opt in (("g", og), ("d", od)):
                for i, stt in enumerate(opt._state):
                    if stt is not None:
                        t["%sstate%d" % (nm, i)] = stt.detach().cpu().numpy().copy()
            rec.append(dict(d=np.asarray(d, dtype=np.float64), g=np.asarray(g, dtype=np.float64), t=t))
        L.check(L.lib.gt_gemm_b16_path_counts(b16, 1))
        return rec, dumped, list(b16)

    a, masks, ca = run(None)
    for gm, dreal, dfake, d2 in masks:          # the dumped masks are Bernoulli(0.5) and differ between sites and steps
        assert all(abs(float(m.mean()) - 0.5) < 0.05 for m in gm + dreal + dfake + d2)
    assert not torch.equal(masks[0][0][0], masks[1][0][0]) and not torch.equal(masks[0][1][0], masks[0][2][0])
    b, _, cb = run(masks)
    fwd_philox = sum(ca[slot(FWD, A_PHILOX, f)] for f in range(4))
    print("B16PHILOX %s census A %s B %s" % (tag, {i: n for i, n in enumerate(ca) if n}, {i: n for i, n in enumerate(cb) if n}))
    assert (fwd_philox > 0) == b16 and (sum(ca[slot(BWD, A_PHILOX, f)] for f in range(4)) > 0) == b16, ca
    assert sum(ca[slot(e, A_BUFFER, f)] for e in (FWD, BWD) for f in range(4)) == 0, ca
    assert sum(cb[slot(FWD, A_BUFFER, f)] for f in range(4)) == fwd_philox and sum(cb[slot(e, A_PHILOX, f)] for e in (FWD, BWD) for f in range(4)) == 0, cb
    identical, fails = True, []
    for st in range(steps):
        for key in ("d", "g"):
            sa, sb = a[st][key], b[st][key]
            identical &= bool(np.array_equal(sa, sb))
            if not np.all(np.abs(sa - sb) <= RTOL * np.maximum(np.abs(sb), 1e-30)):
                fails.append("step %d %s scalars %s vs %s" % (st, key, sa, sb))
        assert a[st]["d"][3] == b[st]["d"][3] and a[st]["d"][4] == b[st]["d"][4], "correct counts differ"
        assert sorted(a[st]["t"]) == sorted(b[st]["t"])
        for name in a[st]["t"]:
            ta, tb = a[st]["t"][name], b[st]["t"][name]
            assert np.isfinite(tb).all() and float(np.abs(tb).max()) > 0, name
            identical &= bool(np.array_equal(ta, tb))
            dist = _rel_rms(ta, tb)
            print("B16PHILOX %s step %d %-8s rel rms %.3e" % (tag, st, name, dist))
            if not dist <= RTOL:
                fails.append("step %d %s: rms(A - B) / rms(B) = %.3e > %.0e" % (st, name, dist, RTOL))
    print("B16PHILOX %s: Philox run and injected-mask run bit-identical: %s" % (tag, identical))
    assert not fails, "\n".join(fails)
