"""-m gpu: a used engine computes what a fresh one does, bit for bit (tests/engine_history.py holds the sessions, the tables and the
comparator; DESIGN.md "Engine state across steps" the contract).

Every other GPU test runs on an engine created for its case.  A training run keeps one engine for hours: batches of many (B, T) from
staging buffers refilled in place, train and eval phases, re-seeds, re-binds.  What decides correctness there is the engine's host-side
state -- pointer-keyed memos (StepCopy, DImage, LossNormaliser's, the MLPG band cache), per-step flags, the lengths ring, grow-only workspaces whose
pads and tails keep another batch's data.  One test per (backend, history): the worn session runs the history, then both it and its twin
(new objects and a new engine, loaded from the worn session's snapshot, exact-size new buffers) run the probe -- set_seed, two train steps
and one eval-phase step at (3, 19) -- and everything the probe returns or leaves behind must be the same bits and finite.  The
COMM_PAIRS run the same on engines that carry a one-rank communicator: the forgetting rules of the data-parallel valid-frame count.

On the commit before this module 13 pairs failed: same_shape_refill on the seven backends that make a 16-byte-pitch copy of a dense x
(gt_set_seed restarts the step count while the per-step copies of x stayed keyed on it), poison_train_restore on the six Adam backends
(a checkpoint without optimizer state did not empty a populated optimizer).  Causes and fixes: the last entry of HISTORY.md."""
import numpy as np
import pytest

import engine_history as H

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("backend,history", H.PAIRS + H.COMM_PAIRS, ids=["%s-%s" % p for p in H.PAIRS + H.COMM_PAIRS])
def test_used_engine_equals_fresh_engine(backend, history):
    worn, twin = H.run_pair(backend, history)
    assert len(worn) > 20 and any(k.startswith("step2.") for k in worn) and "philox_d" in worn
    diffs = H.differences(worn, twin)
    for d in diffs:
        print(d)
    assert not diffs, "%s after %s: %d of %d records differ or are not finite; first: %s" % (backend, history, len(diffs), len(worn), diffs[0])


# ---------------------------------------------------------------------------------------------
# negative controls: the comparison sees a seed and a single ulp
# ---------------------------------------------------------------------------------------------
def _twins(mutate=None):
    a = H.Session("mlp_philox", "fresh")
    snap = a.snapshot()
    if mutate is not None:
        snap = mutate(snap)
    return a, H.Session("mlp_philox", "fresh", snapshot=snap)


def test_a_twin_under_another_seed_differs_in_masks_and_parameters():
    a, b = _twins()
    ra, rb = H.probe(a), H.probe(b, seed=H.PROBE_SEED + 1)
    differing = [d.split(":")[0] for d in H.differences(ra, rb)]
    assert "philox_g" in differing and "philox_d" in differing, differing
    assert any(k.startswith("G.layers") for k in differing) and any(k.startswith("D.layers") for k in differing), differing


def test_a_twin_with_one_weight_moved_by_one_ulp_differs():
    import torch

    def one_ulp(snap):
        w = snap["g"]["last_linear.weight"]
        h = w.cpu().numpy().copy()
        h.view(np.uint32).reshape(-1)[7] += 1          # the next float32 away from zero
        snap["g"]["last_linear.weight"] = torch.from_numpy(h).to(w.device)
        return snap
    a, b = _twins(one_ulp)
    assert int((a.mg.flat_params() != b.mg.flat_params()).sum()) == 1 and torch.equal(a.md.flat_params(), b.md.flat_params())
    ra, rb = H.probe(a), H.probe(b)
    differing = [d.split(":")[0] for d in H.differences(ra, rb)]
    assert "G.last_linear.weight" in differing, differing
