"""Two G + D steps and one plain forward per role through every stack and storage form are bit for bit -- and launch for launch -- what
tests/golden/stack_step_digests.json recorded (-m gpu): SHA-256 of y_hat, y_hat_static, every step's D and G scalar tuples, every
parameter and both forwards, and the five host-side launch-count vectors, for the cases of tests/golden/make_stack_digests.py (MLP, LSTM,
In2OutRNN and SRU generators in float32 and bf16 storage, recurrent discriminators, the folded SRU pair).  The file was recorded on the
commit before the stacks' output layer and their bf16 products each became one function; a change that means to change a bit or a
launch of the step re-records it and says so.  Cases added later carry their own "recorded_on": the three precision routes of the float32
family (bf16 products on float32 storage beside bf16 storage, both recurrent stacks at bf16 precision, the split first layer with the fused
stack) were recorded on the commit before that family's product precision became an argument."""
import json

import pytest

import make_stack_digests as M

with open(M.DEFAULT_OUT) as _f:
    RECORD = json.load(_f)


def test_the_record_holds_every_case_and_key():
    assert RECORD["recorded_on"] == M.RECORDED_ON and RECORD["steps"] == M.STEPS
    assert sorted(RECORD["cases"]) == sorted(M.CASES)
    for name, rec in RECORD["cases"].items():
        later = name in M.CASE_RECORDED_ON      # a case added after the file's commit names its own
        assert sorted(rec) == sorted(M.DIGESTS + ("counts",) + (("recorded_on",) if later else ())), name
        assert not later or rec["recorded_on"] == M.CASE_RECORDED_ON[name], name
        assert all(len(rec[k]) == 64 for k in M.DIGESTS), name
        assert sorted(rec["counts"]) == sorted(M.COUNTERS), name
        assert all(int(slot) >= 0 and n > 0 for c in rec["counts"].values() for slot, n in c.items()), name
        assert sum(rec["counts"]["gemm"].values()) + sum(rec["counts"]["gemm_b16"].values()) > 0, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.CASES))
def test_steps_and_launches_are_identical_to_the_record(name):
    got, want = M.run_case(name), RECORD["cases"][name]
    for k in M.COUNTERS:
        print("%s %s launches: %s" % (name, k, json.dumps(got["counts"][k], sort_keys=True)))
    wrong = ["%s %s: %s, recorded %s" % (name, k, got[k], want[k]) for k in M.DIGESTS if got.get(k) != want[k]]
    wrong += ["%s launches of %s: %s, recorded %s" % (name, k, got["counts"][k], want["counts"][k]) for k in M.COUNTERS
              if got["counts"][k] != want["counts"][k]]
    assert sorted(got) == sorted(want) and not wrong, "\n".join(wrong)
