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
(a checkpoint without optimizer state did not empty a populated optimizer).  Causes and fixes: the last entry of HISTORY.md.

The FEATURE_PAIRS hold the opt-in GAN features to the same contract: objectives and the weight clip, spectral normalisation, the gradient
penalties, the generator's weight average -- each keeps state of its own between steps (the table's last rows), and their
own test modules create an engine per run.  Twelve rows (engine_history.FEATURE_BACKENDS), the seven histories of the old rows on each,
and histories of their own: feature_off_and_on, gp_hooks, sn_other_d, ema_swap_and_roles, normaliser.  The probe is feature_probe: beside
the old record, the penalty's running record and the peeked eps / x_hat, the average with both its counts and a forward on it, and the
launch counts of either feature's kernels, which must be non-zero exactly where the feature is on.  Five negative controls: an ulp in the
snapshot's average or in sn_u, the average's count, another penalty weight, another clip bound.

No row was dropped: the engine refuses none of the twelve combinations (it refuses a penalty together with spectral norm, with bf16 products
or on a recurrent discriminator -- "gt_set_grad_penalty: ..." -- and no row asks for those; test_engine_history_host.py checks that).  The one
refusal met is sn_hinge's shard: "gt_set_shard: spectral normalisation (gt_set_spectral_norm) is on; a sharded engine is not supported with
it yet", asserted inside its shard_and_normaliser history, which then runs the override alone.

On the commit before these pairs none of the 115 failed, and every premise held but one that was wrong about the arithmetic, not about the
engine: after a NaN train step the penalty's record is NOT NaN.  The penalty sees D's input only through the signs of the activations (a
NaN activation takes the leaky slope, in leaky_drop_grad as in torch's leaky_relu_backward) and the weights are still finite when it is
formed, so |grad_x D|, the penalty and its weight gradients are finite in the double-backward reference as on the device; the history
asserts that the record took the step and is finite, and the probe's opening reset clears it.  The hinge keeps a NaN as torch's relu does
(poison_eval's and poison_train_restore's premises hold on hinge_fused and sn_hinge as they stand).  That the pairs can fail was checked
against two deliberately wrong builds of the library, not kept: eps keys that depend on the last penalised batch's size fail the 22 wgan-gp
pairs whose history takes a penalised step and no other; a record that reset=True does not clear, an average whose count a re-bind
forgets and a power iteration in eval passes fail 73 pairs -- the record's step count, the `ema.*` records, the launch counts and
sn_other_d's own assertion."""
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


@pytest.mark.parametrize("backend,history", H.FEATURE_PAIRS, ids=["%s-%s" % p for p in H.FEATURE_PAIRS])
def test_used_engine_equals_fresh_engine_with_the_features_on(backend, history):
    worn, twin = H.run_feature_pair(backend, history)
    ft = H.backend_features(backend)
    assert len(worn) > 20 and any(k.startswith("step2.") for k in worn) and "philox_d" in worn
    # a row that silently ran the plain path cannot pass: the features' own kernels were launched in the probe, and only those
    gp, sn = worn["gp_paths"], worn["sn_paths"]
    if ft.get("grad_penalty"):
        assert gp[2] == 2 and gp[3] == 2 and gp[0] == (2 if ft["grad_penalty"][0] == "wgan-gp" else 0), gp      # one gp_row / gp_finalize per train step
        assert worn["gp_steps"][0] == 2 and ("gp_peek.x_hat" in worn) == (ft["grad_penalty"][0] == "wgan-gp")
    else:
        assert not gp.any() and "gp_record" not in worn, gp
    if ft.get("spectral_norm"):
        assert sn[0] > 0 and sn[2] > sn[0] and sn[3] == 2 and "D.sn_u" in worn, sn      # iterating passes, eval-form passes, one projection per train step
    else:
        assert not sn.any() and "D.sn_u" not in worn, sn
    if ft.get("ema_decay") is not None:
        assert "ema_forward.y_hat" in worn and worn["ema_counts"][0] == worn["ema_counts"][1] >= 2
        assert H.difference("the parameters behind averaged_weights()", worn["ema_after_swap.params"],
                            np.concatenate([worn[k].ravel() for k in worn if k.startswith("G.") and ".opt." not in k])) is None
        assert any(H.difference(k, worn[k], worn["G." + k[4:]]) for k in worn if k.startswith("ema."))      # (the average is not the parameters)
    else:
        assert not any(k.startswith("ema") for k in worn)
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


# ... and what the features keep: two fresh twins each, the snapshot or one setting apart
def _feature_twins(backend, mutate_a=None, mutate_b=None, features_b=None):
    """The names of the records in which the feature probes of two fresh sessions of one snapshot differ."""
    import copy
    a = H.Session(backend, "fresh")
    snap = a.snapshot()
    if mutate_a is not None:
        a = H.Session(backend, "fresh", snapshot=mutate_a(copy.deepcopy(snap)))
    b = H.Session(backend, "fresh", snapshot=(mutate_b or (lambda s: s))(copy.deepcopy(snap)), features=features_b)
    return [d.split(":")[0] for d in H.differences(H.feature_probe(a), H.feature_probe(b))]


def _one_ulp(t, index):
    import torch
    h = t.cpu().numpy().copy()
    h.view(np.uint32).reshape(-1)[index] += 1
    return torch.from_numpy(h).to(t.device)


def _averaged(n):
    def mutate(snap):
        snap["n_averaged"] = n
        return snap
    return mutate


def test_one_ulp_in_the_snapshots_average_shows_in_the_average():
    def moved(snap):
        snap["ema"]["last_linear.weight"] = _one_ulp(snap["ema"]["last_linear.weight"], 7)
        return _averaged(2)(snap)
    # (with a count of 0 the first update would copy over either average.  decay 0.999: a lerp of weight 0.001 moves the exact result by
    # 0.999 of the planted ulp, so rounding keeps the difference; at decay 0.9 it is lost in one lerp out of ten)
    differing = _feature_twins("ema_adam", _averaged(2), moved)
    assert "ema.last_linear.weight" in differing, differing
    assert not any(k.startswith("G.") or k.startswith("D.") or k.startswith("step") for k in differing), differing


def test_the_snapshots_count_decides_whether_the_first_update_copies():
    differing = _feature_twins("ema_adagrad", _averaged(0), _averaged(2))
    assert "ema_counts" in differing and any(k.startswith("ema.") for k in differing), differing
    assert not any(k.startswith("G.") or k.startswith("D.") for k in differing), differing


def test_one_ulp_in_sn_u_shows_in_the_discriminator():
    def moved(snap):
        snap["d"]["sn_u"] = _one_ulp(snap["d"]["sn_u"], 3)
        return snap
    differing = _feature_twins("sn_hinge", None, moved)
    assert any(k.startswith("D.layers") for k in differing), differing


def test_another_penalty_weight_shows_in_the_discriminator_and_the_record():
    differing = _feature_twins("gp_r1", features_b=dict(grad_penalty=("r1", 5.0)))
    assert "gp_record" in differing and any(k.startswith("D.layers") for k in differing), differing
    assert "gp_steps" not in differing and "gp_paths" not in differing


def test_another_clip_bound_shows_in_the_discriminator():
    differing = _feature_twins("wgan_clip", features_b=dict(weight_clip=0.02))
    assert any(k.startswith("D.layers") for k in differing), differing
