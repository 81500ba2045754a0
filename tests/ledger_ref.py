"""The epoch ledger in pure Python: what ``epoch_ledger_kernel`` must hold after each add, following the slot table of
include/gantts_hip.h.  Python floats are IEEE doubles and ``math.sqrt`` is correctly rounded, so every operation here rounds as the
kernel's does; the expressions are written in the order gantts_amd/train.py evaluates them."""
import math
import struct

SLOTS = 32
KEYS = ("generator", "mse", "mge", "loss_real_d", "loss_fake_d", "loss_adv", "discriminator", "real_correct", "fake_correct",
        "mcd", "bap_mcd", "f0_rmse", "vuv_err", "dur_rmse", "d_updates", "g_updates")
HAS_D, HAS_G, HAS_DIST = 1, 2, 4
ACOUSTIC, DURATION, VC = 0, 1, 2
KIND_OF = {"acoustic": ACOUSTIC, "duration": DURATION, "vc": VC}
# StepResults order: where each float32 result of a step goes
D_FIELDS = ((0, "discriminator"), (1, "loss_fake_d"), (2, "loss_real_d"), (3, "real_correct"), (4, "fake_correct"))
G_FIELDS = ((5, "mse"), (6, "mge"), (7, "loss_adv"), (8, "generator"))


def batch_metrics(dist, kind, Ds, C):
    """{metric: value} of one batch from its seven distortion sums (s_mcd, s_bap, s_f0, n_voiced, n_vuv_err, s_mse, n_frames)."""
    s_mcd, s_bap, s_f0, n_voiced, n_vuv_err, s_mse, n = [float(v) for v in dist]
    if kind == ACOUSTIC:
        return {"mcd": (C * s_mcd) / n, "bap_mcd": ((C * s_bap) / n) / 10.0,
                "f0_rmse": math.sqrt(s_f0 / n_voiced) if n_voiced > 0 else float("nan"), "vuv_err": n_vuv_err / n}
    if kind == DURATION:
        return {"dur_rmse": math.sqrt(s_mse / (n * Ds))}
    return {"mcd": (C * s_mcd) / n}


class Ledger(object):
    def __init__(self):
        self.slots = [0.0] * SLOTS

    def add(self, results, dist, flags, kind, Ds, C):
        """``results``: the step's 12 float32 values (numpy float32 or exactly representable floats)."""
        s = self.slots
        for on, fields, count in ((flags & HAS_D, D_FIELDS, "d_updates"), (flags & HAS_G, G_FIELDS, "g_updates")):
            if on:
                for i, k in fields:
                    s[KEYS.index(k)] += float(results[i])
                s[KEYS.index(count)] += 1.0
        if flags & HAS_DIST:
            for k, v in batch_metrics(dist, kind, Ds, C).items():
                s[KEYS.index(k)] += v
        return self

    def as_dict(self):
        return dict(zip(KEYS, self.slots))


def same_bits(a, b):
    """Equality of two sequences of doubles in which NaN equals NaN and nothing else is forgiven."""
    bits = lambda v: struct.pack("<d", float(v))      # noqa: E731
    return len(a) == len(b) and all(bits(x) == bits(y) or (x != x and y != y) for x, y in zip(a, b))
