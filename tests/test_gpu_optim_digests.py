"""The fused clip + update step is bit for bit what tests/golden/optim_step_digests.json recorded (-m gpu), for every row of the
variant table of gantts_amd/csrc/eng_ops.hip: SHA-256 of params, grads and every live state buffer after the last update of each
case of tests/golden/make_optim_digests.py (which holds the cases, the inputs' integer formula and the reasons for the sizes), and
the bits of every update's reported norm.  The file was recorded on the commit before optim_step_kernel<KIND, F> became the one
kernel of the family; a change that means to change a bit of the update re-records it and says so.

The row check is a review aid tied to the table's spelling: it reads the OPTIM_ROW(OPTK_..., OPTI_... | ...) entries out of eng_ops.hip
with a regular expression (a table written otherwise fails it, by the count or by the comparison), and the rows a case reaches are
make_optim_digests.reached_rows' restatement of the host's rule, not a report of what the library launched.  A wrongly chosen row
is caught by the digests themselves."""
import json
import os
import re

import pytest

import make_optim_digests as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(M.DEFAULT_OUT) as _f:
    RECORD = json.load(_f)


def _table_rows():
    """The rows of the variant table, as "KIND|FLAG|..." in the table's own spelling without the prefixes."""
    with open(os.path.join(ROOT, "gantts_amd", "csrc", "eng_ops.hip")) as f:
        src = f.read()
    rows = []
    for kind, flags in re.findall(r"OPTIM_ROW\(OPTK_(\w+),\s*([^)]*)\)", src):
        rows.append("|".join([kind] + re.findall(r"OPTI_(\w+)", flags)))
    return rows


def test_the_recorded_cases_reach_every_row_of_the_variant_table():
    assert sorted(RECORD["cases"]) == sorted(M.CASES) and RECORD["sizes"] == list(M.SIZES)
    table = _table_rows()
    assert len(table) == len(set(table)) >= 23
    reached = set()
    for name, rec in RECORD["cases"].items():
        assert rec["rows"] == M.CASES[name]["rows"], name
        reached.update(rec["rows"])
    assert reached == set(table), "rows without a case: %s; cases without a row: %s" % (sorted(set(table) - reached), sorted(reached - set(table)))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(M.CASES))
def test_update_is_bit_identical_to_the_record(name):
    from gantts_amd import _lib as L
    rec = RECORD["cases"][name]
    assert M.reached_rows(M.CASES[name], L) == rec["rows"]
    wrong = []
    for n in M.SIZES:
        got, want = M.run_case(name, n), rec["digests"][str(n)]
        assert sorted(got) == sorted(want), (name, n, sorted(got), sorted(want))
        wrong += ["%s n=%d %s: %s, recorded %s" % (name, n, k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "\n".join(wrong)
