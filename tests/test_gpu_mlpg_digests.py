"""One G + D step through the MLPG path is bit for bit what tests/golden/mlpg_step_digests.json recorded (-m gpu): SHA-256 of y_hat_static,
the D and G loss tuples and every parameter after apply_generator -> update_discriminator -> update_generator, for the cases of
tests/golden/make_mlpg_digests.py (the STEP case of test_gpu_mlpg_band.py with a dense R and with an MLPGBand, one vc_in2out step).  The
file was recorded on the commit before MLPG moved into eng_mlpg.hip and its launches began to take the band as an argument; a change that
means to change a bit of the step re-records it and says so."""
import json

import pytest

import make_mlpg_digests as M

with open(M.DEFAULT_OUT) as _f:
    RECORD = json.load(_f)


def test_the_record_holds_every_case():
    assert sorted(RECORD["cases"]) == sorted(M.CASES)
    for name, rec in RECORD["cases"].items():
        assert sorted(rec) == ["all", "d", "g", "params", "y_hat_static"] and all(len(v) == 64 for v in rec.values()), name


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.CASES))
def test_step_is_bit_identical_to_the_record(name):
    got, want = M.run_case(name), RECORD["cases"][name]
    wrong = ["%s %s: %s, recorded %s" % (name, k, got[k], want[k]) for k in sorted(want) if got.get(k) != want[k]]
    assert sorted(got) == sorted(want) and not wrong, "\n".join(wrong)
