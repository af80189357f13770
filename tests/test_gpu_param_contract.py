"""kmm_set_param / kmm_get_param against the recorded contract: tests/golden/param_contract.json holds, for every name either
entry point knew at the commit noted in it and every value of a fixed probe list, the return code and message of the set and the
return code and value (or message) of a get of the same name, on a fresh handle per name over the index of smoke() — and one get
of every name on an untouched handle.  tools/record_param_contract.py made it and is the walk replayed here; every triple must be
equal.  Two exceptions, the fixture's own: "debug_skew_p2_counter" is probed with 0 alone (it exists to make the next
synchronising call fail) and "host_cpu_budget" is compared by its return code (its value is the machine's)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def contract():
    with open(os.path.join(ROOT, "tests", "golden", "param_contract.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replayed():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    from tools import record_param_contract as rec
    return rec, json.loads(json.dumps(rec.walk(rec.smoke_handles())))                   # (as the fixture went through JSON)


def test_the_fixture_is_the_tools_walk(contract, replayed):
    rec, _ = replayed
    assert contract["names"] == list(rec.NAMES) and len(set(rec.NAMES)) == len(rec.NAMES) > 120
    assert contract["probes"] == list(rec.PROBES)
    assert contract["zero_only"] == ["debug_skew_p2_counter"] and contract["code_only"] == ["host_cpu_budget"]
    assert list(rec.ZERO_ONLY) == contract["zero_only"] and list(rec.CODE_ONLY) == contract["code_only"]
    assert len(contract["recorded_from"]) >= 7


def test_defaults(contract, replayed):
    _, got = replayed
    assert sorted(got["defaults"]) == sorted(contract["names"])
    wrong = {n: (got["defaults"][n], contract["defaults"][n]) for n in contract["names"] if got["defaults"][n] != contract["defaults"][n]}
    assert not wrong


def test_every_triple(contract, replayed):
    rec, got = replayed
    compared, wrong = 0, []
    for name in contract["names"]:
        want_rows, got_rows = contract["walk"][name], got["walk"][name]
        assert [r[0] for r in want_rows] == [r[0] for r in got_rows] == list(rec.probes_of(name)), name
        for want, have in zip(want_rows, got_rows):
            compared += 1
            if want != have:
                wrong.append((name, want, have))
    assert not wrong, wrong[:20]
    assert compared == (len(contract["names"]) - 1) * len(contract["probes"]) + 1 == rec.n_triples()   # names x probes, but for the one name probed with 0
