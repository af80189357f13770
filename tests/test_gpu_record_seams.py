"""GPU tests of the FASTQ / two-line FASTA record compaction (csrc/kmm_records.hpp k_rec_count2 .. k_rec_uniform, launched by
rec_compact_piece in csrc/kmm.hip) at the seams of its vectors, lanes, tiles, wavefront ranges, table reloads, super-tiles,
pieces and of the limit.  The files and the line model are tests/record_seam_cases.py, held to their conditions by
tests/test_record_seam_cases_on_the_cpu.py.  "debug_records_grid" gives a file of a few KB the tile ranges per wavefront that only
a piece beyond 32 MiB has otherwise.

Every run is on a clean handle in "count_kmers" mode and is compared EXACTLY — no tolerance is involved — with the model's
(consumed, n_records), the oracle's node counts, per-k-mer counts and windows on the model's sub-reads, the model's
"quality_masked_bases" and its answer for "flat_uniform_batches"; a damaged file must fail with the model's error kind and raw
byte offset, and after reset() its well-formed twin maps correctly on the same handle.  Routes: (a) the device compaction
("path" 2, no host threads) with the hook at the case's value, at 1, and — files of 64 KiB and less — at the default grid, in
the variants plain / break table / quality floor / both; (b) the direct path ("path" 1); (c) the host packer.  The direct path
keeps no per-k-mer counts (use_radix, csrc/kmm_radix_host.hpp): they are compared on (a) and (c).

Measured on one MI355X: the whole file, 90 tests, takes 131 s; its slowest tests (the four super-tile files of 4.1 MiB of one
feature in FASTQ: 96 calls) 4.0 s each."""
import re

import numpy as np
import pytest

from tests import record_seam_cases as rc
from tests.skew_cases import numpy_entry_counts, revcomp_kmers

pytestmark = pytest.mark.gpu

KS = (5, 31)
DAMAGED = [g for g in rc.GROUPS if rc.is_damaged(g)]
WELL_FORMED = [g for g in rc.GROUPS if g not in DAMAGED]


@pytest.fixture(scope="module")
def devs():
    """One handle per k, in per-k-mer counting mode, shared by the tests of this module."""
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    assert (_lib.FORMAT_FASTQ, _lib.FORMAT_FASTA2) == (rc.FASTQ, rc.FASTA2)
    from kmer_mapper_amd.engine import DeviceIndex
    open_ = {}
    for k in KS:
        index = rc.index_for(k)
        d = DeviceIndex.from_index(index, index.max_node_id())
        assert d.get_param("radix_available")
        d.count_kmers_mode(True)
        assert d.get_param("debug_records_grid") == 0
        open_[k] = (d, d.get_param("host_pack_threads"))
    yield open_
    for d, _ in open_.values():
        d.close()


def test_the_hook_takes_0_to_65536_and_nothing_else(devs):
    dev, _ = devs[31]
    for bad in (-1, 65537, 1 << 40):
        with pytest.raises(ValueError):
            dev.set_param("debug_records_grid", bad)
        assert dev.get_param("debug_records_grid") == 0
    for ok in (65536, 1, 0):
        dev.set_param("debug_records_grid", ok)
        assert dev.get_param("debug_records_grid") == ok


# ---------------------------------------------------------------------------------------------- what is expected
_EXPECT = {}


@pytest.fixture(scope="module")
def expect(oracle):
    """(case name, variant, k) -> the model's answers and the oracle's on the model's sub-reads (computed once, never changed)."""
    def get(name, variant, k):
        key = (name, variant, k)
        if key not in _EXPECT:
            m = rc.model_of(rc.build(name), variant)
            e = dict(ret=(m["consumed"], m["n_records"]), masked=m["n_masked"], uniform=int(m["uniform"]), error=m["error"])
            if m["error"] is None:
                index = rc.index_for(k)
                bases, offsets = rc.reads_arrays(m["reads"])
                kmers = oracle.extract(bases, offsets, k)
                both = np.concatenate([kmers, revcomp_kmers(kmers, k)])
                entries = np.asarray(index._kmers, dtype=np.uint64)
                for rev, km in ((False, kmers), (True, both)):
                    counts, n = oracle.map_reads(index, index.max_node_id(), bases, offsets, k, also_revcomp=rev)
                    per_kmer = numpy_entry_counts(entries, km) if km.size else np.zeros(entries.shape[0], dtype=np.uint32)
                    assert n == kmers.shape[0] and (counts.sum() > 0 or n == 0)        # (reads of 15 bases hold no 31-mer)
                    counts.setflags(write=False)
                    per_kmer.setflags(write=False)
                    e[rev] = dict(counts=counts, lookups=(2 if rev else 1) * int(n), per_kmer=per_kmer)
            _EXPECT[key] = e
        return _EXPECT[key]
    return get


# ---------------------------------------------------------------------------------------------- one run
def _run(devs, case, variant, k, rev, route, grid):
    """One kmm_map_records call on a clean handle: what it returned and everything that is compared, or the error's text."""
    dev, default_threads = devs[k]
    brk, q = rc.VARIANTS[variant]
    params = dict(path=1 if route == "b" else 2, host_pack_threads=3 if route == "c" else 0, host_pack_slice_kb=4 if route == "c" else 0,
                  debug_records_grid=grid, debug_records_piece_kb=case["piece_kb"], min_base_quality=q)
    dev.reset()
    dev.get_stats(reset=True)
    for name, v in params.items():
        dev.set_param(name, v)
    uniform0, packed0 = dev.get_param("flat_uniform_batches"), dev.get_param("host_packed_record_calls")
    try:
        ret = dev.map_records(case["raw"], fmt=case["fmt"], k=k, also_revcomp=rev, lut=rc.table(True) if brk else None)
        got = dict(ret=ret, counts=dev.get_node_counts().copy(), per_kmer=dev.get_kmer_counts().copy(), lookups=dev.get_stats()[0],
                   masked=dev.get_param("quality_masked_bases"), uniform=dev.get_param("flat_uniform_batches") - uniform0,
                   packed=dev.get_param("host_packed_record_calls") - packed0)
    except ValueError as e:                                       # (a device-found error surfaces at the next synchronising call)
        dev.reset()
        got = dict(error=str(e))
    except Exception as e:                                        # a HIP error: the handle is not touched again, the session ends
        pytest.exit("%s: %r" % (case["name"], e), returncode=3)
    for name in params:
        dev.set_param(name, default_threads if name == "host_pack_threads" else 0)
    return got


def _compare(got, e, rev, route, what, wrong, any_route=False):
    """Appends to `wrong` what differs between a run and the expectation of a well-formed file.  any_route: the host packer may
    hand the call to the device route ("badtail" in tests/record_seam_cases.py)."""
    if "error" in got:
        wrong.append(what + ("refused: " + got["error"][:160],))
        return
    w = e[rev]
    if got["ret"] != e["ret"]:
        wrong.append(what + ("consumed, n_records", got["ret"], e["ret"]))
    if not np.array_equal(got["counts"], w["counts"]):
        wrong.append(what + ("node counts", int(np.abs(got["counts"].astype(np.int64) - w["counts"]).sum())))
    if got["lookups"] != w["lookups"]:
        wrong.append(what + ("lookups", got["lookups"], w["lookups"]))
    if route != "b" and not np.array_equal(got["per_kmer"], w["per_kmer"]):
        wrong.append(what + ("per-k-mer counts",))
    if got["masked"] != e["masked"]:
        wrong.append(what + ("quality_masked_bases", got["masked"], e["masked"]))
    if route != "b" and got["uniform"] != e["uniform"]:
        wrong.append(what + ("flat_uniform_batches", got["uniform"], e["uniform"]))
    if route == "b" and got["uniform"]:
        wrong.append(what + ("flat_uniform_batches moved on the direct path",))
    if (route == "c") != bool(got["packed"]) and not (any_route and route == "c"):
        wrong.append(what + ("host_packed_record_calls", got["packed"]))


def _routes(case):
    """(route, variant, hook value) of every run of a case."""
    grids = sorted({case["grid"], 1}) + ([0] if len(case["raw"]) <= (64 << 10) else [])
    runs = [("a", v, g) for v in rc.variants_of(case) for g in grids]
    return runs + [("b", "plain", 0), ("c", "plain", 0)]


def _report(wrong):
    names = sorted({w[0] for w in wrong})
    assert not wrong, "%d runs wrong in the cases %s; the first: %s" % (len(wrong), names, wrong[:4])


# ---------------------------------------------------------------------------------------------- the well-formed cases
@pytest.mark.parametrize("group", WELL_FORMED)
def test_well_formed_files_map_like_the_model(devs, expect, group):
    """Every placement of the group's files (the failure message names the cases; a case's placements are in its build())."""
    wrong = []
    for name in [n for n in rc.CASES if rc.group_of(n) == group]:
        case = rc.build(name)
        for k in KS:
            for route, variant, grid in _routes(case):
                e = expect(name, variant, k)
                assert e["error"] is None, name
                for rev in (False, True):
                    got = _run(devs, case, variant, k, rev, route, grid)
                    _compare(got, e, rev, route, (name, "k %d revcomp %d route %s %s hook %d" % (k, rev, route, variant, grid)), wrong,
                             case["any_route"])
    _report(wrong)


# ---------------------------------------------------------------------------------------------- the damaged cases
KIND = {"malformed": "record structure violated at byte offset", "invalid_base": "is not a nucleotide"}


@pytest.mark.parametrize("group", DAMAGED)
def test_damaged_files_fail_with_the_models_error_and_the_handle_recovers(devs, expect, group):
    """One byte of a well-formed file changed (a quality line made one byte short or long) at each placement of the composite,
    the reload and the super-tile files: the error kind and the raw byte offset in the message are the model's, and after
    reset() the well-formed twin maps correctly on the same handle.  Without a floor a quality line's length is not looked at:
    the file maps like its twin.  (The model's offset counts from the start of the error's piece and the message's from the
    start of the mapped chunk: the same here, no damaged file has more than one piece — asserted below.)"""
    wrong = []
    for name in [n for n in rc.CASES if rc.group_of(n) == group]:
        case = rc.build(name)
        twin = rc.build(case["twin"])
        assert case["piece_kb"] == 0, name
        for k in KS:
            for route, variant, grid in _routes(case):
                e = expect(name, variant, k)
                for rev in (False, True):
                    what = (name, "k %d revcomp %d route %s %s hook %d" % (k, rev, route, variant, grid))
                    got = _run(devs, case, variant, k, rev, route, grid)
                    if e["error"] is None:
                        _compare(got, e, rev, route, what, wrong)
                        continue
                    kind, offset, _ = e["error"]
                    text = got.get("error", "")
                    found = re.search(r"offset (\d+) of a mapped chunk", text)
                    if KIND[kind] not in text or not found or int(found.group(1)) != offset:
                        wrong.append(what + ("expected %s at %d" % (kind, offset), text[:120] or "mapped"))
                    # (route c: the packer gives the damaged file up, and packs the twin)
                    _compare(_run(devs, twin, variant, k, rev, route, grid), expect(case["twin"], variant, k), rev, route,
                             what + ("the twin after reset",), wrong)
    _report(wrong)
