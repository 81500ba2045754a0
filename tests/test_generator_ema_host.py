"""Host (no GPU): the reference the weight-average tests judge by (tests/generator_ema_ref.py) against its definition, torch's
AveragedModel + get_ema_multi_avg_fn, and the power of the bit-for-bit comparator against the mistakes a kernel could make.

1. The numpy restatement -- first update copies, then one fused multiply-add per element in the branch ``w = float32(1.0 - decay)``
   selects -- equals AveragedModel over K random parameter snapshots bit for bit, for decays on both branches and w = 1.
2. Each seeded mistake changes at least one bit of the chain at every size the GPU tests use, for the committed seeds.  Decays: 0.99 and
   0.9 (w < 0.5) and 0.3 (w >= 0.5).  0.5 and 0.25 cannot serve for the second branch: their ``1 - w`` is a power of two, so the product of
   the two-rounding form is exact and the form equals the fused one.  ``w = 1 - float32(decay)`` is not seeded at 0.3, where it happens to
   be float32(0.7) itself."""
import numpy as np
import pytest

import generator_ema_ref as R

DECAYS = (0.999, 0.99, 0.9, 0.5, 0.25, 0.0, 0.3)
MISTAKE_DECAYS = (0.99, 0.9, 0.3)
MISTAKES = ("no_copy", "two_roundings", "w_from_float_decay", "before_update", "before_clamp")
SEEDS = {1: 23, 4099: 1, 839355: 2}      # searched: at these every mistake below shows at its size (one element needs the search)
CLAMP = 1.0


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("decay", DECAYS)
def test_numpy_restatement_equals_averaged_model(decay, n):
    _, stored = R.snapshots(n, 100 + n)
    ours, torchs = R.numpy_chain(stored[1:], decay), R.torch_chain(stored[1:], decay)
    assert len(ours) == len(torchs) == R.K_UPDATES
    assert R.same_bits(ours[0], stored[1])                                # the first update copies
    for k, (a, b) in enumerate(zip(ours, torchs)):
        assert R.same_bits(a, b), "decay %g n %d update %d: %d elements differ" % (decay, n, k + 1, R.differing(a, b))
    if decay == 0.0:
        assert R.same_bits(ours[-1], stored[-1])                          # w = 1: the average is the last snapshot


def test_both_branches_and_w_one_are_covered():
    ws = [float(R.lerp_weight(d)) for d in DECAYS]
    assert any(w < 0.5 for w in ws) and any(0.5 <= w < 1.0 for w in ws) and 1.0 in ws
    assert R.lerp_weight(0.999) != np.float32(1.0) - np.float32(0.999)      # the double subtraction is not the float one


def test_fma32_is_single_rounded():
    """A sum that float64 rounds ONTO a float32 tie follows the exact value, not the tie rule: with c = 1 + 2^-23 (odd last bit) and
    a b = 2^-24 (1 - 2^-46), the exact sum lies just below the tie c + 2^-24 and rounds to c; rounding through float64 first lands on the
    tie and then on the even neighbour above."""
    a, b, c = np.float32(2.0 ** -12 * (1 + 2.0 ** -23)), np.float32(2.0 ** -12 * (1 - 2.0 ** -23)), np.float32(1 + 2.0 ** -23)
    naive = np.float32(np.float64(a) * np.float64(b) + np.float64(c))
    assert float(naive) == 1 + 2.0 ** -22
    assert R.fma32(a, b, c).item() == float(c)
    assert R.fma32(-a, b, -c).item() == -float(c)
    assert R.fma32(np.float32(3.0), np.float32(5.0), np.float32(-1.0)).item() == 14.0


def test_float_decay_weight_is_no_mistake_at_0_3():
    assert np.float32(1.0) - np.float32(0.3) == R.lerp_weight(0.3)


@pytest.mark.parametrize("n", R.SIZES)
@pytest.mark.parametrize("mistake,decay", [(m, d) for m in MISTAKES for d in MISTAKE_DECAYS if (m, d) != ("w_from_float_decay", 0.3)])
def test_comparator_rejects_seeded_mistake(mistake, decay, n):
    raw, stored = R.snapshots(n, SEEDS[n], clamp=CLAMP)
    if mistake == "before_clamp":
        assert any(not R.same_bits(a, b) for a, b in zip(raw[1:], stored[1:]))      # the clamp bites
    good = R.numpy_chain(stored[1:], decay, initial=stored[0])
    bad = R.numpy_chain(stored[1:], decay, initial=stored[0], mistake=mistake, before=stored[:-1], raw=raw[1:])
    worst = max(R.differing(a, b) for a, b in zip(good, bad))
    assert worst >= 1, "%s at decay %g, n = %d: not told apart from the reference" % (mistake, decay, n)
