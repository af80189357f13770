"""GPU tests of mates kept together in BAM output (include/kmm.h "record_bam_mates"): every case of
tests/bam_mates_cases.py through kmm_map_bam with the raw form, the keep mode and the mates on — as one window and in its windows —
against the catalogue's independent model (held to its conditions by tests/test_bam_mates_on_the_cpu.py): the queue's bytes, its
record counter, the entries in pair order, *n_records, the BAM counters, the BGZF take.  Every error case fails in the call that
completes the offending pair and leaves the handle as it was; an unpaired end whose last call brings no member; the carry dropped
by a reset and by a new stream; the refusals; the switch off; the façade and `select-reads --bam-out --keep-mates`."""
import os

import numpy as np
import pytest

from tests import bam_mates_cases as bm
from tests import bam_records_cases as br
from tests import read_hits_cases as rc
from tests.test_gpu_bam_records import _same_bytes, _select

pytestmark = pytest.mark.gpu

GOOD, BAD = bm.good_cases(), bm.error_cases()
K = bm.K
COUNTERS = ("bam_records", "bam_records_excluded", "records_reversed")


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _open(kmm, k=K):
    index = rc.genome_index(k)
    return kmm.DeviceIndex.from_index(index, index.max_node_id())


def _mates_on(dev, case):
    _select(dev, case.base)
    dev.record_hits(True, windows=True)
    dev.record_keep(True, min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)
    dev.record_pairs(False, rule=case.pair_rule)
    dev.record_bam(True, mates=True)


def _windows(case):
    comp, windows = bm.windowed_file(case, block=301 if len(case.base.payload) < 60_000 else 0xFF00)
    return np.frombuffer(comp, dtype=np.uint8), windows


def _stream(dev, case, upto=None, hinted=False):
    """The case's windows, one call each; every call takes its whole window.  upto: stop in front of that window.  Returns the
    records the calls reported."""
    buf, windows = _windows(case)
    total = 0
    for i, (lo, hi) in enumerate(windows):
        if i == upto:
            break
        nxt = windows[i + 1] if hinted and i + 1 < len(windows) else None
        used, n = dev.map_bam(buf[lo:hi], first=i == 0, last=i == len(windows) - 1, k=case.base.k, max_index_lookup_frequency=rc.NO_FILTER,
                              next_chunk=None if nxt is None else buf[nxt[0]:nxt[1]])
        assert used == hi - lo
        assert n % 2 == 0                                                          # (whole pairs per call)
        total += n
    return total


def _call(dev, case, i):
    buf, windows = _windows(case)
    lo, hi = windows[i]
    return dev.map_bam(buf[lo:hi], first=i == 0, last=i == len(windows) - 1, k=case.base.k, max_index_lookup_frequency=rc.NO_FILTER)


def _check_take(dev, case, times=1, bgzf=False, n_pairs=None):
    e = bm.expected(case, n_pairs)
    assert dev.get_param("record_keep_pending_bytes") == times * len(e.raw)
    assert dev.get_param("record_keep_pending_records") == times * e.n_records
    if bgzf:
        members, n_text, n = dev.take_kept_bgzf()
        assert n_text == times * len(e.raw)
        _same_bytes(br.inflate(members.tobytes()), e.raw * times)
    else:
        got, n = dev.take_kept_records()
        _same_bytes(got, e.raw * times)
    assert n == times * e.n_records
    hits, windows = dev.take_record_hits()
    assert np.array_equal(hits, np.tile(e.hits, times)) and np.array_equal(windows, np.tile(e.windows, times))


def _state(dev):
    return ([dev.get_param(name) for name in ("record_hits_pending", "record_keep_pending_bytes", "record_keep_pending_records") + COUNTERS],
            dev.get_node_counts().copy(), dev.get_stats())


def _same_state(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], (a[0], b[0])


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", GOOD, ids=lambda c: c.name)
def test_cases_as_one_window_and_in_their_windows(kmm, case):
    d = br.decoded(case.base)
    whole = case._replace(cuts=None)
    with _open(kmm, case.base.k) as dev:
        _mates_on(dev, case)
        assert dev.get_param("record_bam_mates") == 1 and dev.get_param("record_bam") == 1
        assert _stream(dev, whole) == len(d.records)
        assert dev.get_param("bam_records") == len(d.records) and dev.get_param("bam_records_excluded") == d.excluded
        assert dev.bam_header() == case.base.payload[:d.hdr]
        _check_take(dev, case)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        for hinted in (False, True):                                                # in its windows (a case without cuts: whole once more)
            assert _stream(dev, case, hinted=hinted) == len(d.records)
            _check_take(dev, case, bgzf=hinted)
        assert dev.get_param("bam_records") == 3 * len(d.records) and dev.get_param("bam_records_excluded") == 3 * d.excluded


def test_three_streams_without_a_take_and_pieces_of_one_kib(kmm):
    case = bm.by_name("windows_every_301__any")
    assert len(bm.expected(case).raw) % 16 != 0                                     # (the next stream's records start off a line)
    with _open(kmm) as dev:
        _mates_on(dev, case)
        for _ in range(3):
            _stream(dev, case)
        _check_take(dev, case, times=3)
        dev.set_param("debug_records_piece_kb", 1)
        _stream(dev, case._replace(cuts=None))
        _check_take(dev, case)


# ---------------------------------------------------------------------------------------------- what has to fail
def _message(case):
    if case.error[0] == "strangers":
        p = case.error[1]
        return "\"record_bam_mates\" is 1 and pair %d of the stream is none: records %d and %d are not mates .*collate the file by name " \
               "\\(`samtools collate`\\) and exclude secondary and supplementary records \\(0x900\\)" % (p, 2 * p, 2 * p + 1)
    return "\"record_bam_mates\" is 1 and the stream ends with an unpaired record: it holds %d selected records" % case.error[1]


def _the_waiting_mate_is_as_the_failing_call_found_it(dev, case, n_done):
    """Behind a failed call, with both queues taken: n_done selected records were complete in front of it, an odd number, so the
    last of them waits.  One more call of the same stream brings a record with its name — the waiting record itself once more, so
    with the same entry — and, under min_hits 0, must append the pair: the waiting record's bytes from the handle's carry, then
    the new one's, and two entries whose first is the waiting record's."""
    from kmer_mapper_amd import reads_io
    assert n_done % 2 == 1
    r = bm.selected_records(case.base)[n_done - 1]
    raw = case.base.payload[r.start:r.start + r.size]
    hits, windows = bm.entries(case.base)
    comp = np.frombuffer(reads_io.bgzf_members(raw, 0xFF00) + reads_io.BGZF_EOF, dtype=np.uint8)
    dev.record_keep(True, min_hits=0)
    used, n = dev.map_bam(comp, first=False, last=True, k=case.base.k, max_index_lookup_frequency=rc.NO_FILTER)
    assert (used, n) == (comp.shape[0], 2)
    got, n_kept = dev.take_kept_records()
    _same_bytes(got, raw + raw)
    assert n_kept == 2
    got_h, got_w = dev.take_record_hits()
    assert got_h.tolist() == [int(hits[n_done - 1])] * 2 and got_w.tolist() == [int(windows[n_done - 1])] * 2


@pytest.mark.parametrize("case", BAD, ids=lambda c: c.name)
def test_error_cases_fail_in_the_call_that_completes_the_pair_and_leave_the_handle_as_it_was(kmm, case):
    at = bm.window_of(case)
    good = bm.by_name("patterns__any")
    with _open(kmm) as dev:
        _mates_on(dev, case)
        _stream(dev, case, upto=at)                                                 # the windows in front of it map
        before = _state(dev)
        n_pairs = bm.selected_done(case)[at - 1] // 2 if at else 0
        assert before[0][0] == 2 * n_pairs                                          # (whole pairs only are pending)
        with pytest.raises(ValueError, match=_message(case)):
            _call(dev, case, at)
        _same_state(before, _state(dev))
        _check_take(dev, case, n_pairs=n_pairs)                                     # what the windows before it appended, no more
        n_done = bm.selected_done(case)[at - 1] if at else 0
        if n_done % 2:                                                              # a mate 1 waited when the call failed: it still does
            _the_waiting_mate_is_as_the_failing_call_found_it(dev, case, n_done)
        # a new stream on the handle maps correctly, and so does the same stream once more up to the failing call
        _mates_on(dev, good)
        _stream(dev, good)
        _check_take(dev, good)
        _mates_on(dev, case)
        _stream(dev, case, upto=at)
        _check_take(dev, case, n_pairs=n_pairs)


def test_an_unpaired_end_whose_last_call_brings_no_member(kmm):
    from kmer_mapper_amd import reads_io
    case = bm.by_name("odd_count")
    p = case.base.payload
    comp = np.frombuffer(reads_io.bgzf_members(p, 1999), dtype=np.uint8)           # (no end-of-file block: the stream goes on)
    with _open(kmm) as dev:
        _mates_on(dev, case)
        used, n = dev.map_bam(comp, first=True, last=False, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n) == (comp.shape[0], 12)
        before = _state(dev)
        with pytest.raises(ValueError, match="ends with an unpaired record: it holds 13 selected records"):
            dev.map_bam(np.zeros(0, np.uint8), first=False, last=True, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        _same_state(before, _state(dev))
        _check_take(dev, case, n_pairs=6)
        _the_waiting_mate_is_as_the_failing_call_found_it(dev, case, 13)            # the failed call touched nothing: the stream goes on


def test_a_reset_and_a_new_stream_drop_the_waiting_mate(kmm):
    case = bm.by_name("carry_over_empty_windows__any")
    with _open(kmm) as dev:
        _mates_on(dev, case)
        _stream(dev, case, upto=2)
        assert dev.get_param("record_hits_pending") == 2                            # (pair 0; mate 1 of pair 1 waits)
        dev.reset()
        assert dev.get_param("record_hits_pending") == 0 and dev.get_param("record_keep_pending_bytes") == 0
        _stream(dev, case)
        _check_take(dev, case)
        _stream(dev, case, upto=1)                                                  # without a reset: a new stream drops it
        dev.take_record_hits()
        dev.take_kept_records()
        _stream(dev, case)
        _check_take(dev, case)


def test_a_change_of_either_switch_drops_the_waiting_mate(kmm):
    """"record_bam" off and on again in the middle of a stream: the mate 1 that waited is gone (its text is two-line FASTA, which
    the named pair form of DESIGN 4.23 must never take for its own carry), so its mate arrives alone."""
    from kmer_mapper_amd import reads_io
    case = bm.by_name("carry_over_empty_windows__any")
    r = bm.selected_records(case.base)[2]                                          # mate 1 of pair 1: it waits behind window 1
    comp = np.frombuffer(reads_io.bgzf_members(case.base.payload[r.start:r.start + r.size]) + reads_io.BGZF_EOF, dtype=np.uint8)
    with _open(kmm) as dev:
        for switch in ("record_bam", "record_bam_mates"):
            _mates_on(dev, case)
            _stream(dev, case, upto=2)
            dev.take_record_hits()
            dev.take_kept_records()
            dev.set_param(switch, 0)                                                # (this switch alone moves)
            dev.set_param(switch, 1)
            with pytest.raises(ValueError, match="ends with an unpaired record"):
                dev.map_bam(comp, first=False, last=True, k=K, max_index_lookup_frequency=rc.NO_FILTER)
            assert dev.get_param("record_hits_pending") == 0 and dev.get_param("record_keep_pending_bytes") == 0


# ---------------------------------------------------------------------------------------------- refusals, the switch off
def test_refusals_map_nothing_and_append_nothing(kmm):
    case = bm.by_name("patterns__any")
    pending = lambda dev: (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"))
    with _open(kmm) as dev:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="record_bam_mates takes 0 or 1"):
                dev.set_param("record_bam_mates", bad)
        assert dev.get_param("record_bam_mates") == 0
        dev.set_param("record_bam_mates", 1)
        for hits, keep in ((0, 0), (2, 0), (2, 1)):
            dev.set_param("record_hits", hits)
            dev.set_param("record_keep", keep)
            with pytest.raises(ValueError, match="\"record_bam_mates\" is 1 and \"record_bam\" is 0: mates are kept together in the raw form"):
                _stream(dev, case)
        assert pending(dev) == (0, 0) and not dev.get_node_counts().any()
        # a change while entries or kept bytes are pending
        _mates_on(dev, case)
        _stream(dev, case)
        with pytest.raises(ValueError, match="record_bam_mates 0 with 10 entries pending"):
            dev.set_param("record_bam_mates", 0)
        dev.take_record_hits()
        with pytest.raises(ValueError, match="record_bam_mates 0 with %d kept bytes pending" % len(bm.expected(case).raw)):
            dev.set_param("record_bam_mates", 0)
        assert dev.get_param("record_bam_mates") == 1
        dev.take_kept_records()
        dev.set_param("record_bam_mates", 0)
        dev.set_param("record_bam_mates", 1)
        _stream(dev, case)                                                          # the handle serves the next call
        _check_take(dev, case)


def test_what_record_bam_refuses_stays_refused_in_its_words_and_comes_first(kmm):
    case = bm.by_name("patterns__any")
    with _open(kmm) as dev:
        dev.set_param("record_bam_mates", 1)
        dev.set_param("record_bam", 1)
        with pytest.raises(ValueError, match="\"record_bam\" is 1 and \"record_hits\" is 0"):
            _stream(dev, case)
        dev.record_hits(True, windows=True)
        with pytest.raises(ValueError, match="\"record_bam\" is 1 and \"record_keep\" is 0"):
            _stream(dev, case)
        dev.record_keep(True)
        dev.set_param("record_names", 1)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_names\" are 1"):
            _stream(dev, case)
        dev.set_param("record_names", 0)
        dev.set_param("record_names_pairs", 1)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_names_pairs\" are 1: mates are not kept together in BAM output"):
            _stream(dev, case)
        dev.set_param("record_names_pairs", 0)
        dev.set_param("record_pairs", 1)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_pairs\" are 1: mates are not kept together in BAM output"):
            _stream(dev, case)
        dev.set_param("record_pairs", 0)
        dev.set_param("bam_n_ref", 0)
        buf, _ = _windows(case)
        with pytest.raises(ValueError, match="\"record_bam\" is 1 and the stream begins behind the header"):
            dev.map_bam(buf, first=True, last=True, k=K, mid_stream=True, head_skip=0)
        assert dev.get_param("record_hits_pending") == 0 and dev.get_param("record_keep_pending_bytes") == 0


def test_with_the_switch_off_bam_out_gives_the_bytes_of_before_and_no_new_kernel_runs(kmm):
    from kmer_mapper_amd import _lib
    from tests.test_gpu_bam_records import _check_take as check_records, _file, _map, _raw_on
    case = next(c for c in br.all_cases() if c.name == "aux__default")
    mates = bm.by_name("patterns__any")
    with _open(kmm) as dev:
        dev.set_timing(True)
        _raw_on(dev, case)
        dev.set_param("record_bam_mates", 0)
        _map(dev, _file(case.base))
        assert dev.get_timing(_lib.KERNEL_BAM_RAW)[1] == 1
        assert dev.get_timing(_lib.KERNEL_BAM_RAW_MATES) == (0.0, 0)
        check_records(dev, case)
        _mates_on(dev, mates)
        _stream(dev, mates)
        assert dev.get_timing(_lib.KERNEL_BAM_RAW)[1] == 0 and dev.get_timing(_lib.KERNEL_BAM_RAW_MATES)[1] == 1
        _check_take(dev, mates)
        timings = dev.get_timing()
        assert "k_bam_raw_mates" in timings and _lib.KERNEL_NAMES[_lib.KERNEL_BAM_RAW_MATES] == "k_bam_raw_mates"


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    from kmer_mapper_amd.gz_io import BGZF_EOF
    index = rc.genome_index(K)
    try:
        for name in ("windows_every_301__any", "lengths_in_windows__both", "patterns__both_invert"):
            case = bm.by_name(name)
            base = case.base
            e = bm.expected(case)
            comp, _ = bm.windowed_file(case, block=1999)
            got, hits, windows = mapper.select_records(index, comp, fmt="bam", output="bam", k=K, max_index_lookup_frequency=rc.NO_FILTER,
                                                       exclude_flags=base.sel.excl, original_strand=base.orig, keep_mates=True,
                                                       pair_rule=case.pair_rule, min_hits=case.min_hits, min_permille=case.min_permille,
                                                       invert=case.invert)
            assert got.endswith(BGZF_EOF) and br.inflate(got) == bm.expected_file(case)
            assert np.array_equal(hits, e.hits) and np.array_equal(windows, e.windows)
        strangers = bm.by_name("coordinate_sorted")
        with pytest.raises(ValueError, match="pair 0 of the stream is none.*samtools collate"):
            mapper.select_records(index, br.bam_file(strangers.base), fmt="bam", output="bam", k=K, exclude_flags=0x900, keep_mates=True)
        dev = next(iter(mapper._CACHE.values()))[0]                                 # the cached handle is left as it was found
        assert [dev.get_param(name) for name in ("record_bam", "record_bam_mates", "record_hits", "record_keep", "bam_exclude_flags",
                                                 "record_hits_pending", "record_keep_pending_bytes")] == [0] * 7
        with pytest.raises(ValueError, match="keep_mates goes with output=\"bam\""):
            mapper.select_records(index, br.bam_file(strangers.base), fmt="bam", k=K, keep_mates=True)
    finally:
        mapper.clear_cache()


def test_command_line_end_to_end_on_a_windowed_case_and_an_error_removes_the_output(kmm, tmp_path):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.gz_io import BGZF_EOF
    index = rc.genome_index(K)
    npz = str(tmp_path / "index.npz")
    index.to_file(npz)
    case = bm.by_name("windows_every_301__any")._replace(name="cli_windows", min_hits=2, pair_rule="both")
    e = bm.expected(case)
    assert 0 < e.n_records < len(e.hits)
    path, out, hits_out = str(tmp_path / "reads.bam"), str(tmp_path / "kept.bam"), str(tmp_path / "hits")
    open(path, "wb").write(bm.windowed_file(case, block=499)[0])
    common = ["select-reads", "-i", npz, "--bam-out", "--keep-mates", "-k", str(K), "-c", "2000", "-I", str(rc.NO_FILTER), "--min-hits", "2"]
    seen, kept = run_argument_parser(common + ["-f", path, "-o", out, "--pair-rule", "both", "--hits-output", hits_out])
    assert (seen, kept) == (len(e.hits), e.n_records)
    written = open(out, "rb").read()
    assert written.endswith(BGZF_EOF) and br.inflate(written) == bm.expected_file(case)
    assert np.array_equal(np.load(hits_out + ".npy"), e.hits) and np.array_equal(np.load(hits_out + ".windows.npy"), e.windows)
    # strangers and an unpaired end reach the user with the library's hint, and -o is removed
    for name, message in (("strangers_in_windows", "pair 11 of the stream is none.*samtools collate.*0x900.*was removed"),
                          ("odd_count_in_windows", "ends with an unpaired record: it holds 13 selected records.*was removed")):
        bad = bm.by_name(name)
        bad_path, bad_out = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".out.bam"))
        open(bad_path, "wb").write(bm.windowed_file(bad, block=499)[0])
        with pytest.raises(ValueError, match=message):
            run_argument_parser(common + ["-f", bad_path, "-o", bad_out, "--hits-output", bad_out + ".hits"])
        assert not os.path.exists(bad_out)
        assert not os.path.exists(bad_out + ".hits.npy") and not os.path.exists(bad_out + ".hits.windows.npy")   # (written on success alone)
