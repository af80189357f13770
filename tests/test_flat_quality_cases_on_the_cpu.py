"""CPU tier of kmm_map_reads_qual: the new cases of tests/flat_quality_cases.py are held to the conditions they
exist for, so that tests/test_gpu_flat_quality.py cannot pass vacuously; and what can be said about the entry point without
a device — the library exports it, a NULL handle is refused, the Python wrappers take the new parameters."""
import inspect

import numpy as np
import pytest

from tests import flat_quality_cases as fq
from tests import quality_cases as qc

# the cases whose one read holds one window, which dies: nothing can survive there (tiny-all_low by design; tiny-middle
# because "one read of k bases with its middle base low" leaves no window either)
NO_SURVIVOR = ("tiny-all_low", "tiny-middle")


@pytest.fixture(scope="module", params=fq.NEW)
def case(request):
    c = dict(fq.build(request.param))
    c["low"] = fq.low_mask(c)
    c["dead"] = fq.dead_mask(c)
    return c


def test_surviving_windows_are_the_windows_of_the_split_reads(case):
    k = case["k"]
    win = qc.surviving_windows(case["offsets"], k, case["dead"])
    sb, so = qc.split_at_mask(case["bases"], case["offsets"], case["dead"])
    assert win.shape[0] == int(np.maximum(np.diff(so) - k + 1, 0).sum())
    assert np.array_equal(sb, case["bases"][~case["dead"]]) and so[0] == 0 and so[-1] == sb.shape[0]
    n_all = int(np.maximum(np.diff(case["offsets"]) - k + 1, 0).sum())
    assert win.shape[0] < n_all                                     # at least one window dies
    assert (win.shape[0] == 0) == (case["name"] in NO_SURVIVOR)     # ... and at least one survives
    assert case["quals"].shape == case["bases"].shape and case["low"].any()
    assert qc.is_uniform(case["offsets"]) == (case["name"] in fq.UNIFORM or case["name"].startswith(("tiny", "raw_phred")))


def test_the_old_cases_come_through_unchanged():
    for name in ("tile_edges", "with_skip_table", "q93"):
        old, new = qc.build(name), fq.build(name)
        assert new["qual_base"] == 33 and all(np.array_equal(old[f], new[f]) for f in ("bases", "quals", "offsets"))
        assert np.array_equal(fq.dead_mask(new), qc.dead_mask(old)) and np.array_equal(fq.low_mask(new, 21), qc.low_mask(old["quals"], 21))
    assert fq.CASES[:len(qc.CASES)] == qc.CASES and set(fq.UNIFORM) >= set(qc.UNIFORM)


def test_the_low_bytes_stand_where_the_cases_say():
    c = fq.build("span_edges")
    total, k, low = c["bases"].shape[0], c["k"], fq.low_mask(c)
    assert total >= 40_000 and fq.SPAN == 16384
    for p in (0, 15, 16, 31, 32, 16383, 16384, 32767, 32768, total - 1, total - k):
        assert low[p], p
    a, b = fq.SPAN_PAIR                  # k + 1 apart across a workgroup's seam: exactly one window survives between them
    assert low[a] and low[b] and b - a == k + 1 and a < 3 * fq.SPAN <= b and not low[a + 1:b].any()
    win = qc.surviving_windows(c["offsets"], k, low)
    assert a + 1 in win and a not in win and a + 2 not in win and a // qc.L == b // qc.L
    # at the floor below, the bytes exactly one under the floor are alive: the next floor down tells
    assert fq.low_mask(c, c["q"] - 1).sum() < low.sum() < fq.low_mask(c, c["q"] + 1).sum()

    for name, rest in (("odd_total-1", 1), ("odd_total-17", 17), ("odd_total-31", 31), ("odd_total-32", 0)):
        c = fq.build(name)
        total, low = c["bases"].shape[0], fq.low_mask(c)
        assert total % 32 == rest and total == c["offsets"][-1] and low[total - 1] and not low[total - 2]
        assert not qc.is_uniform(c["offsets"])

    c = fq.build("tiny-middle")
    low = fq.low_mask(c)
    assert c["bases"].shape[0] == c["k"] and len(c["offsets"]) == 2 and low[c["k"] // 2] and low.sum() == 1
    c = fq.build("tiny-short")
    low = fq.low_mask(c)
    assert c["bases"].shape[0] < 16 and len(c["offsets"]) == 2 and low[0] and c["bases"].shape[0] > c["k"]
    c = fq.build("tiny-all_low")
    assert c["bases"].shape[0] == c["k"] and len(c["offsets"]) == 2 and fq.low_mask(c).all()

    ref, c = fq.build("all_41_values"), fq.build("raw_phred")
    assert c["qual_base"] == 0 and set(c["quals"].tolist()) == set(range(41)) and np.array_equal(c["bases"], ref["bases"])
    for q in (1, 20, 21, 41):
        assert np.array_equal(fq.low_mask(c, q), fq.low_mask(ref, q))
    c = fq.build("raw_phred-absent")
    absent = c["quals"] == 0xFF
    assert c["qual_base"] == 0 and c["q"] == 93 and 0.04 < absent.mean() < 0.07
    assert np.array_equal(fq.low_mask(c), ~absent) and np.array_equal(fq.low_mask(c, 1), c["quals"] == 0)


def test_with_n_puts_breaks_under_and_beside_low_bases():
    c = fq.build("span_edges")
    low = fq.low_mask(c)
    n = fq.with_n(c, [16383, 32769, 100])
    assert n["use_lut"] and low[16383] and low[32768] and not low[32769] and not low[100]
    dead = fq.dead_mask(n)
    assert dead[32769] and dead[100] and dead.sum() == low.sum() + 2 and np.array_equal(fq.low_mask(n), low)


def test_the_library_exports_the_entry_point_and_refuses_a_null_handle():
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    assert hasattr(L, "kmm_map_reads_qual") and "kmm_map_reads_qual" in _lib.SIGNATURES
    bases = np.frombuffer(b"ACGT" * 10, np.uint8)
    offs = np.array([0, 40], dtype=np.int64)
    p = lambda a: a.ctypes.data                                     # noqa: E731
    rc = L.kmm_map_reads_qual(None, p(bases), p(bases), 33, p(offs), 1, 0, 31, 1000, 0, None)
    assert rc == _lib.KMM_ERR_INVALID_ARG and b"idx is NULL" in L.kmm_last_error()


def test_the_wrappers_take_qualities_and_qual_base():
    from kmer_mapper_amd import engine
    for fn in (engine.DeviceIndex.map_reads, engine.DeviceIndex.map_reads_uniform):
        params = inspect.signature(fn).parameters
        assert params["qualities"].default is None and params["qual_base"].default == 33
