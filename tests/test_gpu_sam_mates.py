"""GPU tests of mates kept together in SAM output (include/kmm.h "record_sam_mates"): every case of
tests/sam_mates_cases.py through kmm_map_records from host and device memory, byte for byte against the catalogue's independent
model (held to its conditions by tests/test_sam_mates_on_the_cpu.py), the entries too; pieces of one KiB; chunked calls cut
between the mates, inside mate 2's name and SEQ, inside a header line between the mates and around unselected lines behind a
waiting mate; the BGZF and gzip routes in two and three windows; the BGZF take; calls behind a strangers failure and behind an
unpaired end that still complete the waiting pair; queues and counters unchanged by a failing call; the refusals; the timing
slots both ways; the switch off; an index without the radix path; the façade and the command line end to end."""
import gzip
import os
import types
import zlib

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import sam_mates_cases as sm
from tests import sam_records_cases as sr
from tests import strand_cases

pytestmark = pytest.mark.gpu

CASES = sm.all_cases()
IDS = [c.name for c in CASES]
STRANGERS = "pair %d of the stream is none: selected records %d and %d are not mates.*group the file by name.*0x900"
UNPAIRED = "ends with an unpaired record: it holds %d selected records"


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _open(kmm, k=sm.K):
    index = rc.genome_index(k)
    return kmm.DeviceIndex.from_index(index, index.max_node_id())


def _select(dev, case):
    incl, min_mapq, regions, keep_unplaced = case.sel
    dev.set_param("bam_exclude_flags", case.excl)
    dev.set_param("bam_include_flags", incl)
    dev.set_param("bam_min_mapq", min_mapq)
    dev.set_record_regions([(name, -1, beg, end) for name, beg, end in (regions or [])], keep_unplaced)
    dev.set_param("original_strand", int(case.orig))


def _mates_on(dev, case):
    _select(dev, case)
    dev.record_hits(True, windows=True)
    dev.record_keep(True, min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)
    dev.record_pairs(False, rule=case.pair_rule)
    dev.record_sam(True, header=case.mode == 1, mates=True)


def _arr(data):
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _fmt(last):
    from kmer_mapper_amd import _lib
    return _lib.FORMAT_SAM | (_lib.FORMAT_LAST_CHUNK if last else 0)


def _map(dev, case, text=None, last=None, device_memory=False):
    raw = _arr(case.text if text is None else text)
    if device_memory:
        import torch
        raw = torch.from_numpy(raw.copy()).cuda()
    return dev.map_records(raw, fmt=_fmt(case.last if last is None else last), k=case.k, max_index_lookup_frequency=rc.NO_FILTER,
                           also_revcomp=case.revcomp)


def _same_bytes(got, want):
    got = bytes(memoryview(got)) if not isinstance(got, bytes) else got
    assert len(got) == len(want), (len(got), len(want))
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError("first difference at byte %d of %d: %r, wanted %r" % (at, len(want), got[max(at - 20, 0):at + 20],
                                                                                    want[max(at - 20, 0):at + 20]))


def _pending(dev):
    return (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"), dev.get_param("record_keep_pending_records"))


def _counters(dev):
    return dev.get_param("sam_records"), dev.get_param("sam_records_excluded"), dev.get_param("sam_header_lines")


def _check_take(dev, e):
    """Both queues against the model: the bytes, the record count (header lines are not counted), the entries of whole pairs."""
    assert _pending(dev) == (2 * e.n_pairs, len(e.out), e.n_kept)
    got, n = dev.take_kept_records()
    _same_bytes(got, e.out)
    assert n == e.n_kept
    if e.n_pairs:
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, e.hits) and np.array_equal(windows, e.windows)
    else:
        assert dev.get_param("record_hits_pending") == 0


def _inflate(members):
    out, rest = [], bytes(members)
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return b"".join(out)


def _expect_failure(e, case):
    if e.stranger is not None:
        return STRANGERS % (e.stranger, 2 * e.stranger, 2 * e.stranger + 1)
    if case.last and e.odd:
        return UNPAIRED % e.n_records
    return None


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model_from_host_and_device_memory(kmm, case):
    e = sm.expected(case)
    failure = _expect_failure(e, case)
    with _open(kmm, case.k) as dev:
        _mates_on(dev, case)
        assert dev.get_param("record_sam") == case.mode and dev.get_param("record_sam_mates") == 1
        for times, device_memory in enumerate((False, True), 1):
            if failure:
                with pytest.raises(ValueError, match=failure):
                    _map(dev, case, device_memory=device_memory)
                assert _pending(dev) == (0, 0, 0) and _counters(dev) == (0, 0, 0) and dev.get_param("record_sam_mate_waiting") == 0
                continue
            assert _map(dev, case, device_memory=device_memory) == (e.consumed, 2 * e.n_pairs)
            assert _counters(dev) == (times * e.n_records, times * e.n_excluded, times * e.n_headers)      # (they count on)
            assert dev.get_param("record_sam_mate_waiting") == int(e.odd)
            _check_take(dev, e)
            assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
            dev.reset()                                                             # (the stream starts over: no mate waits)
            assert dev.get_param("record_sam_mate_waiting") == 0


BLOCKS = sm.block_cases()


@pytest.mark.parametrize("case", BLOCKS, ids=[c.name for c in BLOCKS])
def test_more_than_one_block_of_spans_and_of_tiles(kmm, case):
    """Pairs on both sides of span 1023 / 1024 and of tile block 1023 / 1024; strangers in a later block of spans; the tail of the
    queue moved off a 16-byte line first by another call's kept lines"""
    e = sm.expected(case)
    small = sm.by_name("header_between")._replace(k=case.k, excl=case.excl, sel=case.sel, invert=case.invert, pair_rule=case.pair_rule,
                                                  min_hits=case.min_hits, min_permille=case.min_permille, mode=case.mode, last=False)
    first = sm.model(small)
    with _open(kmm, case.k) as dev:
        _mates_on(dev, case)
        assert _map(dev, small) == (first.consumed, 2 * first.n_pairs)
        state, counters = _pending(dev), _counters(dev)
        if e.stranger is not None:
            with pytest.raises(ValueError, match=STRANGERS % (first.n_pairs + e.stranger, 2 * (first.n_pairs + e.stranger), 2 * (first.n_pairs + e.stranger) + 1)):
                _map(dev, case)
            assert _pending(dev) == state and _counters(dev) == counters
            _check_take(dev, first)
            return
        assert _map(dev, case) == (e.consumed, 2 * e.n_pairs)
        got, n = dev.take_kept_records()
        _same_bytes(got, first.out + e.out)
        assert n == first.n_kept + e.n_kept
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, np.concatenate([first.hits, e.hits])) and np.array_equal(windows, np.concatenate([first.windows, e.windows]))


# ---------------------------------------------------------------------------------------------- pieces, chunks, windows
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pieces_of_one_kib_give_the_one_shot_result(kmm, case):
    """"debug_records_piece_kb" 1: the waiting mate is handed from piece to piece; a line longer than a piece ends the call in
    front of it, and what the call took is the model of that prefix"""
    longest = max([n for _, n in sr.lines_of(case.text)] or [0])
    with _open(kmm, case.k) as dev:
        _mates_on(dev, case)
        dev.set_param("debug_records_piece_kb", 1)
        if longest <= 1024:
            e = sm.expected(case)
            failure = _expect_failure(e, case)
            if failure:
                with pytest.raises(ValueError, match=failure):
                    _map(dev, case)
                assert _pending(dev) == (0, 0, 0) and _counters(dev) == (0, 0, 0) and dev.get_param("record_sam_mate_waiting") == 0
            else:
                assert _map(dev, case) == (e.consumed, 2 * e.n_pairs)
                assert dev.get_param("record_sam_mate_waiting") == int(e.odd)
                _check_take(dev, e)
        else:
            used, n = _map(dev, case)
            assert 0 < used < len(case.text) and case.text[used - 1:used] == b"\n"
            e = sm.model(case, case.text[:used])
            assert n == 2 * e.n_pairs and dev.get_param("record_sam_mate_waiting") == int(e.odd)
            _check_take(dev, e)
        dev.set_param("debug_records_piece_kb", 0)


def _chunked(dev, case, cuts):
    """The text handed over in chunks that end at `cuts`, the unconsumed bytes carried by the caller; the last chunk says so."""
    text = case.text
    ends = sorted(set([c for c in cuts if 0 < c < len(text)] + [len(text)]))
    carry, pos, total = b"", 0, 0
    for end in ends:
        chunk = carry + text[pos:end]
        pos = end
        used, n = _map(dev, case, chunk, last=case.last and end == len(text))
        assert n % 2 == 0
        total += n
        carry = chunk[used:]
    return total


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_chunked_calls_give_the_uncut_bytes_hits_and_windows(kmm, case):
    e = sm.expected(case)
    failure = _expect_failure(e, case)
    with _open(kmm, case.k) as dev:
        _mates_on(dev, case)
        for times, (kind, cuts) in enumerate(sm.cut_sets(case).items(), 1):
            if failure:
                with pytest.raises(ValueError, match=failure):
                    _chunked(dev, case, cuts)
            else:
                assert _chunked(dev, case, cuts) == 2 * e.n_pairs, kind
                assert _counters(dev) == (times * e.n_records, times * e.n_excluded, times * e.n_headers), kind
                _check_take(dev, e)
            dev.reset()
            assert dev.get_param("record_sam_mate_waiting") == 0 and _pending(dev) == (0, 0, 0)


def _windows(call, comp, n_windows):
    size = comp.shape[0]
    step = size // n_windows + 1
    pos, total, end = 0, 0, min(step, size)
    while pos < size:
        used, n = call(comp[pos:end], pos == 0, end == size)
        assert n % 2 == 0
        pos += used
        total += n
        if pos < end and end == size:
            assert used > 0
            continue
        end = min(end + step, size)
    return total


@pytest.mark.parametrize("name", ["patterns_both", "tile_seams", "tiles_on", "between_supplementary_mapq_region", "header_between", "names",
                                  "unterminated_last_line", "crlf", "strangers_prefix", "odd_count_last", "none_selected"])
def test_the_bgzf_and_gzip_routes_in_one_two_and_three_windows(kmm, name):
    """kmm_map_bgzf and kmm_map_gzip on their inflated bytes: the waiting mate crosses the windows; KMM_FORMAT_LAST_CHUNK supplies
    a final line's newline and ends the stream"""
    from kmer_mapper_amd import _lib, reads_io
    case = sm.by_name(name)
    e = sm.model(case, sr.with_final_newline(case.text))
    failure = _expect_failure(e, case)
    bgzf = _arr(reads_io.bgzf_members(case.text, 397) + reads_io.BGZF_EOF)
    gz = _arr(gzip.compress(case.text, 6))
    kw = dict(fmt=_lib.FORMAT_SAM, k=case.k, max_index_lookup_frequency=rc.NO_FILTER)
    with _open(kmm, case.k) as dev:
        _mates_on(dev, case)
        routes = ((lambda c, first, last: dev.map_bgzf(c, first=first, last=last, **kw), bgzf),
                  (lambda c, first, last: dev.map_gzip(c, first=first, last=last, **kw), gz))
        for call, comp in routes:
            for n_windows in (1, 2, 3):
                if failure:
                    with pytest.raises(ValueError, match=failure):
                        _windows(call, comp, n_windows)
                    dev.reset()
                    continue
                assert _windows(call, comp, n_windows) == 2 * e.n_pairs
                assert dev.get_param("record_sam_mate_waiting") == 0
                _check_take(dev, e)


def test_the_bgzf_take_inflates_to_the_plain_take(kmm):
    case = sm.by_name("tiles_on")
    e = sm.expected(case)
    with _open(kmm) as dev:
        _mates_on(dev, case)
        _map(dev, case)
        _map(dev, case)                                                              # two calls, one take: the second goes behind the first
        members, n_text, n = dev.take_kept_bgzf()
        assert (n_text, n) == (2 * len(e.out), 2 * e.n_kept)
        _same_bytes(_inflate(members.tobytes()), e.out * 2)
        assert dev.get_param("record_keep_pending_bytes") == 0
        dev.take_record_hits()
        _map(dev, case)
        _check_take(dev, e)


# ---------------------------------------------------------------------------------------------- failing calls
def test_a_call_behind_a_strangers_failure_and_behind_an_unpaired_end_still_completes_the_waiting_pair(kmm):
    case = sm.by_name("patterns_any")._replace(last=False)
    text = case.text
    sel = [(s, n) for s, n, kind in sm.classify(case, text) if kind]
    cut = sel[5][0]                                                                  # between the mates of pair 2: mate 1 waits
    e = sm.expected(sm.by_name("patterns_any"))
    first = sm.model(case, text[:cut])
    stranger = sm.mline(b"somebody_else", 0x83, sm.hit_read(100, 77)) + sm.pair(b"after", sm.hit_read(90, 5), sm.miss_read(90))
    with _open(kmm) as dev:
        _mates_on(dev, case)
        assert _map(dev, case, text[:cut]) == (cut, 4)
        assert dev.get_param("record_sam_mate_waiting") == 1
        state, counters = _pending(dev), _counters(dev)
        assert state == (4, len(first.out), first.n_kept)
        for piece_kb in (0, 1):
            dev.set_param("debug_records_piece_kb", piece_kb)
            with pytest.raises(ValueError, match=STRANGERS % (2, 4, 5)):
                _map(dev, case, stranger)                                            # the pair a waiting mate completes
            assert _pending(dev) == state and _counters(dev) == counters and dev.get_param("record_sam_mate_waiting") == 1
            with pytest.raises(ValueError, match=UNPAIRED % 5):
                _map(dev, case, b"", last=True)                                      # a last call that brings no byte
            with pytest.raises(ValueError, match=UNPAIRED % 5):
                _map(dev, case, sm.HEAD, last=True)                                  # ... or no selected record
            assert _pending(dev) == state and _counters(dev) == counters and dev.get_param("record_sam_mate_waiting") == 1
            # a call of several pieces that replaces the waiting mate in its first piece and fails in a later one
            later = text[cut:sel[10][0]] + sm.pair(b"x", sm.H(1), sm.H(2)) * 3 + sm.mline(b"one", 0x43, sm.H(3)) + sm.mline(b"two", 0x83, sm.H(4))
            with pytest.raises(ValueError, match=STRANGERS % (8, 16, 17)):
                _map(dev, case, later)
            assert _pending(dev) == state and _counters(dev) == counters and dev.get_param("record_sam_mate_waiting") == 1
        dev.set_param("debug_records_piece_kb", 0)
        assert _map(dev, case, text[cut:], last=True) == (len(text) - cut, 2 * e.n_pairs - 4)
        assert dev.get_param("record_sam_mate_waiting") == 0
        _check_take(dev, e)


def test_strangers_in_a_later_piece_report_the_streams_ordinal_and_append_nothing(kmm):
    good = sm.by_name("patterns_any")
    e = sm.expected(good)
    text = good.text + sm.pair(b"left", sm.H(1), sm.H(2), name2=b"right") + sm.pair(b"l", sm.H(1), sm.H(2), name2=b"r")
    with _open(kmm) as dev:
        _mates_on(dev, good)
        dev.set_param("debug_records_piece_kb", 1)
        with pytest.raises(ValueError, match=STRANGERS % (e.n_pairs, 2 * e.n_pairs, 2 * e.n_pairs + 1)):      # (the lowest one)
            _map(dev, good, text)
        assert _pending(dev) == (0, 0, 0) and _counters(dev) == (0, 0, 0)
        dev.set_param("debug_records_piece_kb", 0)
        _map(dev, good)
        _check_take(dev, e)


def test_refusals_and_the_state_the_parameter_keeps(kmm):
    case = sm.by_name("odd_count")
    e = sm.expected(case)
    with _open(kmm) as dev:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="record_sam_mates takes 0 or 1"):
                dev.set_param("record_sam_mates", bad)
        with pytest.raises(ValueError, match="record_sam_mates 1 with \"record_sam\" 0"):
            dev.set_param("record_sam_mates", 1)
        with pytest.raises(ValueError):
            dev.set_param("record_sam_mate_waiting", 1)                             # (read-only)
        dev.set_param("record_sam", 2)
        dev.set_param("record_sam_mates", 1)
        for call in (lambda: _map(dev, case),):
            with pytest.raises(ValueError, match="\"record_sam\" is 2 and \"record_hits\" is 0"):
                call()
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        dev.record_pairs(True)
        with pytest.raises(ValueError, match="\"record_sam\" is 2 and \"record_pairs\" is 1"):
            _map(dev, case)
        dev.record_pairs(False)
        dev.set_param("record_hits_min_base_quality", 20)
        with pytest.raises(ValueError, match="record_hits_min_base_quality is 20"):
            _map(dev, case)
        dev.set_param("record_hits_min_base_quality", 0)
        assert _pending(dev) == (0, 0, 0) and _counters(dev) == (0, 0, 0)
        _mates_on(dev, case)
        assert _map(dev, case) == (e.consumed, 2 * e.n_pairs) and dev.get_param("record_sam_mate_waiting") == 1
        # the switch does not move while entries or kept bytes are pending
        with pytest.raises(ValueError, match="record_sam_mates 0 with %d entries pending" % (2 * e.n_pairs)):
            dev.set_param("record_sam_mates", 0)
        dev.take_record_hits()
        with pytest.raises(ValueError, match="record_sam_mates 0 with %d kept bytes pending" % len(e.out)):
            dev.set_param("record_sam_mates", 0)
        assert dev.get_param("record_sam_mates") == 1 and dev.get_param("record_sam_mate_waiting") == 1
        dev.take_kept_records()
        # a change of either switch drops the waiting mate; so does kmm_reset_counts, and a new stream
        dev.set_param("record_sam_mates", 0)
        assert dev.get_param("record_sam_mate_waiting") == 0
        dev.set_param("record_sam_mates", 1)
        _map(dev, case)
        assert dev.get_param("record_sam_mate_waiting") == 1
        dev.take_record_hits(), dev.take_kept_records()
        dev.set_param("record_sam", 2)
        assert dev.get_param("record_sam_mate_waiting") == 0
        dev.set_param("record_sam", 1)
        _map(dev, case)
        assert dev.get_param("record_sam_mate_waiting") == 1
        dev.reset()
        assert dev.get_param("record_sam_mate_waiting") == 0
        _map(dev, case)
        from kmer_mapper_amd import _lib, reads_io
        dev.take_record_hits(), dev.take_kept_records()
        bgzf = _arr(reads_io.bgzf_members(sm.by_name("patterns_any").text) + reads_io.BGZF_EOF)
        want = sm.expected(sm.by_name("patterns_any"))
        assert dev.map_bgzf(bgzf, fmt=_lib.FORMAT_SAM, k=case.k, max_index_lookup_frequency=rc.NO_FILTER, first=True, last=True)[1] == 2 * want.n_pairs
        _check_take(dev, want)                                                      # (KMM_FORMAT_NEW_STREAM: the mate of the stream before is gone)


def test_the_timing_slots_both_ways_and_the_switch_off_gives_the_unpaired_bytes(kmm):
    from kmer_mapper_amd import _lib
    case = sm.by_name("between_supplementary_mapq_region")
    e = sm.expected(case)
    with _open(kmm) as dev:
        dev.set_timing(True)
        _mates_on(dev, case)
        _map(dev, case)
        ms, launches = dev.get_timing(_lib.KERNEL_SAM_RAW_MATES)
        assert launches == 3 and ms > 0                                             # the tiles' scan; spans by entry and names; flags to advance
        assert dev.get_timing(_lib.KERNEL_SAM_RAW) == (0.0, 0)
        assert "k_sam_raw_mates" in dev.get_timing() and _lib.KERNEL_NAMES[_lib.KERNEL_SAM_RAW_MATES] == "k_sam_raw_mates"
        _check_take(dev, e)
        dev.record_sam(True, header=case.mode == 1, mates=False)
        _map(dev, case)
        assert dev.get_timing(_lib.KERNEL_SAM_RAW)[1] == 2 and dev.get_timing(_lib.KERNEL_SAM_RAW_MATES) == (0.0, 0)   # (a read empties a slot)
        got, n = dev.take_kept_records()
        _same_bytes(got, e.unpaired_out)
        dev.take_record_hits()
    # the cases of "record_sam" itself on a handle that has had the switch on and off again
    for name in ("mixed", "tile_edges", "mixed_selection_no_header"):
        plain = sr.by_name(name)
        want = sr.expected(plain)
        with _open(kmm, plain.k) as dev:
            _select(dev, plain)
            dev.record_hits(True, windows=True)
            dev.record_keep(True, min_hits=plain.min_hits, min_permille=plain.min_permille, invert=plain.invert)
            dev.record_sam(True, header=plain.mode == 1, mates=True)
            dev.record_sam(True, header=plain.mode == 1)
            assert dev.get_param("record_sam_mates") == 0
            raw = _arr(plain.text)
            assert dev.map_records(raw, fmt=_lib.FORMAT_SAM | _lib.FORMAT_LAST_CHUNK, k=plain.k, max_index_lookup_frequency=rc.NO_FILTER,
                                   also_revcomp=plain.revcomp) == (want.consumed, want.n_records)
            got, n = dev.take_kept_records()
            _same_bytes(got, want.out)
            assert n == want.n_kept


def test_an_index_without_the_radix_path(kmm):
    case = sm.by_name("tile_seams")
    e = sm.expected(case)
    index = rc.genome_index(case.k)
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo)
    with kmm.DeviceIndex.from_index(dup, index.max_node_id()) as dev:
        assert dev.get_param("radix_available") == 0
        _mates_on(dev, case)
        assert _map(dev, case) == (e.consumed, 2 * e.n_pairs)
        _check_take(dev, e)


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    from kmer_mapper_amd.gz_io import BGZF_EOF
    try:
        for name in ("patterns_both_inverted", "tiles_on_no_header", "header_between", "read_orientation", "names"):
            case = sm.by_name(name)
            e = sm.expected(case)
            index = rc.genome_index(case.k)
            kw = dict(fmt="sam", output="sam", sam_mates=True, pair_rule=case.pair_rule, header=case.mode == 1, k=case.k,
                      max_index_lookup_frequency=rc.NO_FILTER, exclude_flags=case.excl, original_strand=case.orig, min_hits=case.min_hits,
                      min_permille=case.min_permille, invert=case.invert)
            got, hits, windows = mapper.select_records(index, case.text, **kw)
            _same_bytes(got, e.out)
            assert np.array_equal(hits, e.hits) and np.array_equal(windows, e.windows)
            packed, _, _ = mapper.select_records(index, case.text, compress=True, **kw)
            assert packed.endswith(BGZF_EOF) and _inflate(packed) == e.out
        index = rc.genome_index(sm.K)
        for name, message in (("strangers_prefix", STRANGERS % (2, 4, 5)), ("odd_count_last", UNPAIRED % 21)):
            with pytest.raises(ValueError, match=message):
                mapper.select_records(index, sm.by_name(name).text, fmt="sam", output="sam", sam_mates=True, k=sm.K,
                                      max_index_lookup_frequency=rc.NO_FILTER)
        assert len(mapper._CACHE) == 1
        dev = next(iter(mapper._CACHE.values()))[0]                                 # the cached handle is left as it was found
        assert [dev.get_param(name) for name in ("record_sam", "record_sam_mates", "record_sam_mate_waiting", "record_hits", "record_keep",
                                                 "bam_exclude_flags", "original_strand", "record_pairs_rule", "record_keep_pending_bytes",
                                                 "record_hits_pending")] == [0] * 10
        line = b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"
        for kw in (dict(fmt="sam"), dict(fmt="bam", output="bam"), dict(fmt="fastq")):
            with pytest.raises(ValueError, match="sam_mates goes with output=\"sam\""):
                mapper.select_records(index, line, k=sm.K, sam_mates=True, **kw)
        with pytest.raises(ValueError, match="pair_rule must be"):
            mapper.select_records(index, line, k=sm.K, fmt="sam", output="sam", sam_mates=True, pair_rule="one")
    finally:
        mapper.clear_cache()


CLI = {"plain": ("r.sam", [], "any"), "plain_bgzf_out_no_header": ("r.sam", ["--bgzf", "--no-header"], "both"),
       "sam_gz": ("r.sam.gz", ["--invert"], "any"), "plain_gz": ("r.sam.gz", ["--bgzf"], "both")}


def _cli_text(n_pairs=60):
    """An aligner's output: header lines, pairs with supplementary lines between some mates"""
    out = [b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n@CO\tmade for the test\n"]
    for i in range(n_pairs):
        s1 = (sm.hit_read(150, 101 * i), sm.miss_read(150), sm.hit_read(60 + i, 37 * i))[i % 3]
        s2 = (sm.miss_read(140), strand_cases.revcomp(sm.hit_read(140, 53 * i + 9)))[i % 2]   # (FLAG 0x10: it hits in read orientation)
        name = b"read%d" % i
        out.append(sm.mline(name, 0x63, s1, pos=1 + 31 * i))
        if i % 4 == 1:
            out.append(sm.mline(name, 0x863, sm.hit_read(50, i), pos=7))
        out.append(sm.mline(name, 0x93, s2, pos=200 + 31 * i))
    return b"".join(out)


@pytest.mark.parametrize("kind", list(CLI))
def test_command_line_end_to_end(kmm, tmp_path, kind):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.gz_io import BGZF_EOF
    name, options, pair_rule = CLI[kind]
    text = _cli_text()
    path, npz = str(tmp_path / name), str(tmp_path / "index.npz")
    if kind == "plain_gz":
        data = gzip.compress(text, 6)                                                # plain gzip: the kmm_map_gzip route
    elif name.endswith(".gz"):
        data = reads_io.bgzf_members(text, 1999) + reads_io.BGZF_EOF
    else:
        data = text
    open(path, "wb").write(data)
    case = sm.case("cli_" + kind, text, excl=0x900, orig=True, min_hits=2, invert="--invert" in options, pair_rule=pair_rule,
                   mode=2 if "--no-header" in options else 1, last=True)
    e = sm.model(case)
    assert 0 < e.n_kept < 2 * e.n_pairs and e.out != e.unpaired_out
    rc.genome_index(sm.K).to_file(npz)
    out, hits_out = str(tmp_path / "kept.sam"), str(tmp_path / "hits")
    seen, kept = run_argument_parser(["select-reads", "-i", npz, "-f", path, "--sam-out", "--sam-mates", "--pair-rule", pair_rule, "-k", str(sm.K),
                                      "-c", "3000", "-I", str(rc.NO_FILTER), "--min-hits", "2", "-o", out, "--hits-output", hits_out] + options)
    assert (seen, kept) == (2 * e.n_pairs, e.n_kept)
    written = open(out, "rb").read()
    if "--bgzf" in options:
        assert written.endswith(BGZF_EOF)
        written = _inflate(written)
    _same_bytes(written, e.out)
    assert np.array_equal(np.load(hits_out + ".npy"), e.hits) and np.array_equal(np.load(hits_out + ".windows.npy"), e.windows)
    assert open(path, "rb").read() == data


@pytest.mark.parametrize("name", ["r.sam", "r.sam.gz"])
def test_command_line_errors_remove_the_output(kmm, tmp_path, name):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    npz = str(tmp_path / "index.npz")
    rc.genome_index(sm.K).to_file(npz)
    good = _cli_text(20)
    texts = {"strangers": (good + sm.pair(b"one", sm.H(1), sm.H(2), name2=b"other") + _cli_text(3),
                           "pair 20 of the stream is none.*group the file by name.*0x900.*was removed"),
             "unpaired": (good + sm.mline(b"lonely", 0x43, sm.H(5)), "ends with an unpaired record: it holds 41 selected records.*was removed")}
    for kind, (text, message) in texts.items():
        path, out = str(tmp_path / (kind + "." + name)), str(tmp_path / (kind + ".kept.sam"))
        open(path, "wb").write(reads_io.bgzf_members(text, 1999) + reads_io.BGZF_EOF if name.endswith(".gz") else text)
        with pytest.raises(ValueError, match=message):
            run_argument_parser(["select-reads", "-i", npz, "-f", path, "--sam-out", "--sam-mates", "-k", str(sm.K), "-c", "1500", "-I",
                                 str(rc.NO_FILTER), "-o", out, "--hits-output", out + ".hits"])
        assert not os.path.exists(out) and not os.path.exists(out + ".hits.npy") and not os.path.exists(out + ".hits.windows.npy")
