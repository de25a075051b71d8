"""The refusals of the DG entry points, replayed against the table recorded from the parent of the front-end refactor
(tools/record_refusals.py -> tests/golden/refusals.json): a call with one fault keeps its return code at every entry point;
a call with two faults keeps it too, or is one of the pairs that the one precedence of the argument check re-orders
("the front end").  No device is needed: every call here is refused before any device work."""
import importlib.util
import json
from pathlib import Path

import pytest

from feinsum_amd import _hip

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("record_refusals", ROOT / "tools" / "record_refusals.py")
rr = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rr)

GOLDEN = [{"entry": entry, "case": case, "rc": rc}
          for entry, cases in json.loads((ROOT / "tests" / "golden" / "refusals.json").read_text())["cases"].items()
          for case, rc in cases.items()]
EINVAL, EUNSUPPORTED, OK = _hip.FE_EINVAL, _hip.FE_EUNSUPPORTED, _hip.FE_OK

# The plain and the accumulating face-mass entry points looked at the alignment of their pointers last, behind the variant or
# the scope and behind the early return of an empty call.  Alignment is structure: with the one precedence a misaligned pointer
# is FE_EINVAL whatever else the call asks for, as it has been at the other entry points.  fe_launch inherits the two.
_ALIGNMENT = ("J misaligned", "field misaligned", "output misaligned")
_FACEMASS = ("fe_facemass_prepared_f64", "fe_facemass_acc_f64", "fe_launch(0x4)", "fe_launch(0x204)")
REORDERED = {}
for _entry in _FACEMASS:
    for _a in _ALIGNMENT:
        # behind an unknown variant, a shape or a field count without a kernel: FE_EUNSUPPORTED -> FE_EINVAL
        for _b in ("variant", "Np=56", "Nfp", "b=1"):
            REORDERED[(_entry, f"{_a} + {_b}")] = (EUNSUPPORTED, EINVAL)
        # in an empty call: FE_OK -> FE_EINVAL
        REORDERED[(_entry, f"{_a} + E=0")] = (OK, EINVAL)
# The plain face-mass entry point looked at the variant before the pointer tables: a null table is structure.
for _entry in ("fe_facemass_prepared_f64", "fe_launch(0x4)"):
    REORDERED[(_entry, "null table + variant")] = (EUNSUPPORTED, EINVAL)


@pytest.fixture(scope="module")
def lib():
    return _hip.load_library()


def _replay(lib, single):
    knobs = {entry: dict(rr.cases(entry)) for entry in rr.ENTRIES}
    for row in GOLDEN:
        if (" + " in row["case"]) != single:
            yield row, knobs[row["entry"]][row["case"]]


def test_the_table_holds_refusals_only_and_every_entry_point():
    assert {row["rc"] for row in GOLDEN} <= {EINVAL, EUNSUPPORTED, OK}
    assert {row["entry"] for row in GOLDEN} == set(rr.ENTRIES)
    assert all(row["rc"] != OK or "E=0" in row["case"] for row in GOLDEN)


def test_a_call_with_one_fault_keeps_its_return_code(lib):
    for row, k in _replay(lib, single=True):
        rc, msg = rr.run(lib, row["entry"], k)
        assert rc == row["rc"], (row, rc, msg)
        if rc != OK:
            assert msg.startswith(tuple(p.encode() for p in rr.ENTRIES[row["entry"]][1])), (row, msg)


def test_a_call_with_two_faults_keeps_its_return_code_or_follows_the_precedence(lib):
    seen = set()
    for row, k in _replay(lib, single=False):
        rc, msg = rr.run(lib, row["entry"], k)
        key = (row["entry"], row["case"])
        if rc != row["rc"]:
            assert REORDERED.get(key) == (row["rc"], rc), (row, rc, msg)
            seen.add(key)
        if rc != OK:
            assert msg.startswith(tuple(p.encode() for p in rr.ENTRIES[row["entry"]][1])), (row, msg)
    # every listed pair that the table holds did change: the list names no pair that kept its code
    assert {key for key in REORDERED if any((r["entry"], r["case"]) == key for r in GOLDEN)} == seen
