"""Reference of the sharded resident batch path (gantts_amd.data.ResidentLoader with world > 1, gt_op_assemble_shard).

Expected values come from the HOST pipeline (resident_ref.reference_batches) on the whole batch: rank r of a world of w holds the rows
r::w of the length-sorted whole batch, padded to the whole batch's T, and ``tv_global`` is the whole batch's valid-frame count -- the sum of
the host mask.  ``slot_model`` restates the kernel's slot rule and its ``tv_global`` in numpy, with the mistakes the comparator
(``shard_mismatches``) has to reject.
"""
import numpy as np

import resident_ref as R

# the smallest shapes that can still go wrong: Dx = 6 on pitch 8, Dy = 10 on pitch 12, Ds = 3 + 1, gi = 6 + 5 noise columns on pitch 12
WIDTHS = dict(Dx=6, Dy=10, stream_sizes=[9, 1], has_dynamic_features=[True, False])
WIDTHS_VC = dict(Dx=10, Dy=10, stream_sizes=[9, 1], has_dynamic_features=[True, False])      # a VCDataset scales both sides with ONE set of statistics
NZ = 5
LENGTHS = [37, 3, 12, 37, 5, 20, 9, 31, 3, 16, 25]      # 11 utterances of 3 .. 37 frames; ties; every one holds the longest window
BATCHES = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10]]        # batch size 5: 5, 5, 1 sequences; B * T = 185, 155, 25 rows -- no multiple of 16
KEYS = ("x", "y", "y_static", "mask", "lengths", "z")


def expected_shard(ref, rank, world, T=None):
    """One batch of ``reference_batches`` -> what rank ``rank`` of ``world`` holds: the rows rank::world of every array (padded to the
    WHOLE batch's T, or cut to the caller's ``T`` below it), ``order``, ``T`` and ``tv``, the whole batch's valid frames (the sum of
    the host mask over the frames t < T)."""
    T = ref["T"] if T is None else T
    out = {}
    for k in ("x", "y", "y_static", "mask", "z", "gi"):
        out[k] = None if ref[k] is None else np.ascontiguousarray(ref[k][rank::world, :T])
    out["lengths"] = np.minimum(ref["lengths"][rank::world], T).astype(np.int64)
    out["order"] = ref["order"][rank::world]
    out["T"] = T
    out["tv"] = int(ref["mask"][:, :T].sum())
    return out


MISTAKES = ("contiguous_blocks", "rank_and_world_exchanged", "local_T", "tv_from_local_lengths", "tv_without_cut_at_T",
            "tv_counts_out_of_corpus_slot")


def slot_model(table, first, B_global, T, F, rank, world, mistake=None):
    """What one gt_op_assemble_shard launch derives from the table, restated from include/gantts_hip.h: ``order`` (corpus utterance of every
    local sequence), ``lengths`` (local), ``T`` and ``tv`` -- for the caller's T and the epoch table's slots [first, first + B_global)."""
    rows = np.asarray(table)[first:first + B_global]
    inside = (rows[:, 0] >= 0) & (rows[:, 1] >= 0) & (rows[:, 0] <= F) & (rows[:, 1] <= F - rows[:, 0])
    raw = rows[:, 1]
    share = -(-(B_global - rank) // world)
    slots = rank + world * np.arange(share)
    if mistake == "contiguous_blocks":
        per = -(-B_global // world)
        slots = np.arange(rank * per, min(B_global, (rank + 1) * per))
    elif mistake == "rank_and_world_exchanged":
        slots = (world + rank * np.arange(share)) % B_global
    if mistake == "local_T":
        T = int(raw[slots].max())
    valid = np.where(inside, np.minimum(raw, T), 0)
    tv = int(valid.sum())
    if mistake == "tv_from_local_lengths":
        tv = int(valid[slots].sum())
    elif mistake == "tv_without_cut_at_T":
        tv = int(np.where(inside, raw, 0).sum())
    elif mistake == "tv_counts_out_of_corpus_slot":
        tv = int(np.minimum(raw, T).sum())
    return dict(order=[int(u) for u in rows[slots, 2]], lengths=valid[slots].astype(np.int64), T=int(T), tv=tv)


def shard_mismatches(got, exp):
    """Names among order, lengths, T, tv on which one rank's share of one batch differs from the expectation."""
    bad = []
    if list(got["order"]) != list(exp["order"]):
        bad.append("order")
    if got["lengths"].dtype != np.int64 or got["lengths"].tolist() != exp["lengths"].tolist():
        bad.append("lengths")
    if got["T"] != exp["T"]:
        bad.append("T")
    if got["tv"] != exp["tv"]:
        bad.append("tv")
    return bad


def tts_case(recompute=False):
    """float32 min-max statistics on x (what minmax() of float32 utterances gives), float64 mean / variance on y."""
    hp = R.make_hp(WIDTHS, nz=NZ, recompute=recompute)
    ds = R.make_dataset("tts", WIDTHS, np.float64, lengths=LENGTHS, hp=hp)
    ds.X_data_min, ds.X_data_scale = ds.X_data_min.astype(np.float32), ds.X_data_scale.astype(np.float32)
    return ds, hp


def vc_case():
    hp = R.make_hp(WIDTHS_VC, nz=0, name="vc")
    return R.make_dataset("vc", WIDTHS_VC, np.float64, lengths=LENGTHS, hp=hp), hp
