"""GPU tests of keeping the mates of a name-collated BAM file together (include/kmm.h "record_names_pairs"): every
case of tests/bam_pairs_cases.py through kmm_map_bam with the names, the keep mode and the pairs on — whole and in windows, hinted
and not, in pieces of 1 KiB — against the catalogue's independent model (held to its conditions by
tests/test_bam_pairs_on_the_cpu.py) and against the route the library had: the model's interleaved text through map_records with
"record_pairs" 1.  Calls without a take, pairs behind an odd number of pending entries, the BGZF take; every error case fails in
the call that completes the offending pair and leaves the handle as it was; the refusals; the switch off; the façade and
`select-reads --bam-to-fastq --bam-pairs`.

Pieces of 1 KiB take the cases whose pairs fit one (a piece that holds no whole pair ends the records call, as it does for
interleaved text); the cases with records of 39 770 bases run whole and in windows, where their pairs cross the 1024-byte tiles
and the 4096-byte groups of the keep kernels some eighty times."""
import zlib

import numpy as np
import pytest

from tests import bam_fastq_cases as bc
from tests import bam_pairs_cases as bp
from tests import read_hits_cases as rc
from tests.test_gpu_bam_fastq import _same_text, _select

pytestmark = pytest.mark.gpu

GOOD, BAD = bp.good_cases(), bp.error_cases()
K = bp.K
COUNTERS = ("record_name_bytes_replaced", "records_reversed", "records_without_qual", "bam_records_excluded")


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def index():
    return rc.genome_index(K)


def _open(kmm, index):
    return kmm.DeviceIndex.from_index(index, index.max_node_id())


def _pairs_on(dev, case, pairs=True):
    _select(dev, case.base)
    dev.record_hits(True, windows=True)
    dev.record_keep(True, min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)
    dev.record_pairs(False, rule=case.pair_rule)
    dev.record_names(True, mate_suffix=case.base.suffix, pairs=pairs)


def _block(case):
    return 301 if case.piece_kb else 0xFF00                            # (the long records: not in eight hundred members)


def _stream(dev, case, hinted=False, upto=None):
    """The case's windows, one call each; every call takes its whole window.  upto: stop in front of that window.  Returns the
    records the calls reported."""
    comp, windows = bp.windowed_file(case, block=_block(case))
    buf = np.frombuffer(comp, dtype=np.uint8)
    total = 0
    for i, (lo, hi) in enumerate(windows):
        if i == upto:
            break
        nxt = windows[i + 1] if hinted and i + 1 < len(windows) else None
        used, n = dev.map_bam(buf[lo:hi], first=i == 0, last=i == len(windows) - 1, k=K, max_index_lookup_frequency=rc.NO_FILTER,
                              next_chunk=None if nxt is None else buf[nxt[0]:nxt[1]])
        assert used == hi - lo
        total += n
    return total


def _call(dev, case, i):
    comp, windows = bp.windowed_file(case, block=_block(case))
    buf = np.frombuffer(comp, dtype=np.uint8)
    lo, hi = windows[i]
    return dev.map_bam(buf[lo:hi], first=i == 0, last=i == len(windows) - 1, k=K, max_index_lookup_frequency=rc.NO_FILTER)


def _check_take(dev, case, times=1):
    e = bp.expected(case)
    assert dev.get_param("record_keep_pending_bytes") == times * len(e.text1)
    assert dev.get_param("record_keep_pending_records") == times * 2 * e.n_kept
    got, n = dev.take_kept_records()
    _same_text(got, e.text1 * times)
    assert n == times * 2 * e.n_kept
    hits, windows = dev.take_record_hits()
    assert np.array_equal(hits, np.tile(e.hits, times)) and np.array_equal(windows, np.tile(e.windows, times))


def _state(dev):
    return ([dev.get_param(name) for name in ("record_hits_pending", "record_keep_pending_bytes", "record_keep_pending_records") + COUNTERS],
            dev.get_node_counts().copy(), dev.get_stats())


def _same_state(a, b):
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2] == b[2], (a[0], b[0])


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", GOOD, ids=lambda c: c.name)
def test_cases_whole_against_the_model_and_against_the_interleaved_route(kmm, index, case):
    d = bc.decoded(case.base)
    e = bp.expected(case)
    whole = case._replace(cuts=None)
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        assert dev.get_param("record_names_pairs") == 1 and dev.get_param("record_pairs") == 0
        assert _stream(dev, whole) == len(d.records)
        _check_take(dev, case)
        assert [dev.get_param(n) for n in COUNTERS] == [d.replaced, d.reversed, d.no_qual, d.excluded]
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # the route the library had: the model's text as interleaved FASTQ under "record_pairs" 1
        from kmer_mapper_amd import _lib
        dev.record_names(False)
        assert dev.get_param("record_names_pairs") == 0
        dev.record_pairs(True, rule=case.pair_rule)
        text = np.frombuffer(d.text, dtype=np.uint8)
        assert dev.map_records(text, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER) == (len(d.text), len(d.records))
        got, n = dev.take_kept_records()
        _same_text(got, e.text1)
        hits, windows = dev.take_record_hits()
        assert n == 2 * e.n_kept and np.array_equal(hits, e.hits) and np.array_equal(windows, e.windows)


def _windowed(case):
    return case if case.cuts else case._replace(cuts=bp._every(case.base, 700 if case.piece_kb else 30_000))


@pytest.mark.parametrize("case", GOOD, ids=lambda c: c.name)
def test_cases_in_windows_hinted_and_not(kmm, index, case):
    """Windows end inside heads, names, sequences and qualities of either mate: the bytes of an incomplete record are the stream's
    carry, the text of a mate 1 whose mate has not come is the text carry."""
    case = _windowed(case)
    d = bc.decoded(case.base)
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        for hinted in (False, True):
            assert _stream(dev, case, hinted=hinted) == len(d.records)
            _check_take(dev, case)
        assert [dev.get_param(n) for n in COUNTERS[:3]] == [2 * d.replaced, 2 * d.reversed, 2 * d.no_qual]


@pytest.mark.parametrize("case", [c for c in GOOD if c.piece_kb], ids=lambda c: c.name)
def test_pieces_of_one_kib(kmm, index, case):
    d = bc.decoded(case.base)
    assert max(len(d.texts[i]) + len(d.texts[i + 1]) for i in range(0, len(d.texts), 2)) < 1024
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        dev.set_param("debug_records_piece_kb", case.piece_kb)
        assert _stream(dev, case) == len(d.records)                                 # (in the case's own windows, where it has some)
        _check_take(dev, case)


def test_three_calls_without_a_take_and_pairs_behind_an_odd_number_of_pending_entries(kmm, index):
    case = bp.by_name("names__any")
    e = bp.expected(case)
    assert len(e.text1) % 16 != 0
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        for _ in range(3):
            _stream(dev, case)
        _check_take(dev, case, times=3)
        # a take of an odd number of entries leaves the queue's head at an odd index: the next call's first entry lies at an even one
        _stream(dev, case)
        hits_1, windows_1 = dev.take_record_hits(capacity=3)
        assert dev.get_param("record_hits_pending") == len(e.hits) - 3
        _stream(dev, case)
        hits_2, windows_2 = dev.take_record_hits()
        assert np.array_equal(np.concatenate([hits_1, hits_2]), np.tile(e.hits, 2))
        assert np.array_equal(np.concatenate([windows_1, windows_2]), np.tile(e.windows, 2))
        got, n = dev.take_kept_records()
        _same_text(got, e.text1 * 2)
        assert n == 4 * e.n_kept


def test_the_bgzf_take_round_trips_to_the_same_text(kmm, index):
    case = bp.by_name("lengths__any")
    e = bp.expected(case)
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        _stream(dev, case._replace(cuts=None))
        members, n_text, n = dev.take_kept_bgzf()
        assert (n_text, n) == (len(e.text1), 2 * e.n_kept)
        assert bc.inflate(members.tobytes()) == e.text1
        first = zlib.decompressobj(-15).decompress(members.tobytes()[18:])          # (zlib on the first member's raw deflate stream)
        assert len(first) > 0 and e.text1.startswith(first)
        dev.take_record_hits()


# ---------------------------------------------------------------------------------------------- what has to fail
@pytest.mark.parametrize("case", BAD, ids=lambda c: c.name)
def test_error_cases_fail_in_the_call_that_completes_the_pair_and_leave_the_handle_as_it_was(kmm, index, case):
    at = bp.window_of(case)
    good = bp.by_name("patterns__any")
    if case.error[0] == "strangers":
        p = case.error[1]
        message = "pair %d of the stream is none: records %d and %d are not mates: collate the file by name \\(`samtools collate`\\) and " \
                  "exclude secondary and supplementary records \\(0x900\\)" % (p, 2 * p, 2 * p + 1)
    else:
        message = "the stream ends with an unpaired record: it holds %d selected records" % case.error[1]
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        _stream(dev, case, upto=at)                                                 # the windows in front of it map
        before = _state(dev)
        if at:
            assert before[0][0] == bp.selected_done(case)[at - 1] // 2 * 2          # (whole pairs only are pending)
        with pytest.raises(ValueError, match=message):
            _call(dev, case, at)
        _same_state(before, _state(dev))
        # the handle serves the next stream, behind what is pending of this one
        _pairs_on(dev, good)
        dev.take_record_hits()
        dev.take_kept_records()
        _stream(dev, good)
        _check_take(dev, good)


def test_reset_drops_the_text_carry_with_the_queues(kmm, index):
    """A stream left after a window that ends behind a mate 1; kmm_reset_counts; a new stream: nothing of the old one comes back."""
    case = bp.by_name("carry_over_empty_windows__any")
    with _open(kmm, index) as dev:
        _pairs_on(dev, case)
        _stream(dev, case, upto=2)
        assert dev.get_param("record_hits_pending") == 2                            # (pair 0; mate 1 of pair 1 waits)
        dev.reset()
        assert dev.get_param("record_hits_pending") == 0 and dev.get_param("record_keep_pending_bytes") == 0
        _stream(dev, case)
        _check_take(dev, case)
        # without a reset: a new stream drops the mate 1 of the one before
        _stream(dev, case, upto=1)
        dev.take_record_hits()
        dev.take_kept_records()
        _stream(dev, case)
        _check_take(dev, case)


def test_refusals_map_nothing_and_append_nothing(kmm, index):
    case = bp.by_name("patterns__any")
    pending = lambda dev: (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"))
    with _open(kmm, index) as dev:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="record_names_pairs takes 0 or 1"):
                dev.set_param("record_names_pairs", bad)
        assert dev.get_param("record_names_pairs") == 0
        dev.record_hits(True, windows=True)
        dev.set_param("record_names_pairs", 1)
        for names, keep, message in ((0, 0, "\"record_names_pairs\" is 1 and \"record_names\" is 0"),
                                     (0, 1, "QNAME is not carried"),                 # (the message of before, word for word)
                                     (1, 0, "\"record_names_pairs\" is 1 and \"record_keep\" is 0")):
            dev.set_param("record_names", names)
            dev.set_param("record_keep", keep)
            with pytest.raises(ValueError, match=message):
                _stream(dev, case)
        dev.set_param("record_names", 1)
        dev.set_param("record_keep", 1)
        dev.set_param("record_pairs", 1)
        with pytest.raises(ValueError, match="not pair-aligned ones"):              # ("record_pairs" on BAM: as before)
            _stream(dev, case)
        dev.set_param("record_keep", 0)
        dev.set_param("record_pairs", 0)
        assert pending(dev) == (0, 0) and not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # the switch does not change under pending entries
        _pairs_on(dev, case)
        _stream(dev, case)
        n = dev.get_param("record_hits_pending")
        with pytest.raises(ValueError, match="record_names_pairs 0 with %d entries pending that were appended under record_names_pairs 1" % n):
            dev.set_param("record_names_pairs", 0)
        dev.set_param("record_names_pairs", 1)                                      # (the same value: nothing to refuse)
        _check_take(dev, case)
        dev.set_param("record_names_pairs", 0)


def test_the_switch_off_is_the_named_route_as_it_was(kmm, index):
    """With "record_names_pairs" 0 — never set, or set and taken back — the named route gives what tests/bam_fastq_cases.py expects
    of it: one record at a time, an odd count and strangers included."""
    odd = bp.by_name("odd_count")
    strangers = bp.by_name("coordinate_sorted")
    with _open(kmm, index) as dev, _open(kmm, index) as fresh:
        _pairs_on(dev, bp.by_name("patterns__any"))
        _stream(dev, bp.by_name("patterns__any"))
        _check_take(dev, bp.by_name("patterns__any"))
        for case in (odd, strangers):
            single = bc.BCase("pairs_off_" + case.name, case.base, 1, 0, False)
            text, n_kept, _, want_h, want_w = bc.expected(single)
            for h in (dev, fresh):
                _pairs_on(h, case, pairs=False)
                assert h.get_param("record_names_pairs") == 0
                assert _stream(h, case._replace(cuts=None)) == len(want_h)
                got, n = h.take_kept_records()
                _same_text(got, text)
                hits, windows = h.take_record_hits()
                assert n == n_kept and np.array_equal(hits, want_h) and np.array_equal(windows, want_w)


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm, index):
    from kmer_mapper_amd import mapper
    try:
        for name in ("patterns__both_invert", "suffix_on__any", "strand__any", "permille_150__both"):
            case = bp.by_name(name)
            base, e = case.base, bp.expected(case)
            got, hits, windows = mapper.select_records(index, bc.bam_file(base), fmt="bam", k=K, max_index_lookup_frequency=rc.NO_FILTER,
                                                       exclude_flags=base.sel.excl, original_strand=base.orig, mate_suffix=base.suffix,
                                                       min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert,
                                                       pairs=True, pair_rule=case.pair_rule)
            assert got == e.text1 and np.array_equal(hits, e.hits) and np.array_equal(windows, e.windows)
        dev = next(iter(mapper._CACHE.values()))[0]                                 # the cached handle is left as it was found
        assert [dev.get_param(n) for n in ("record_names", "record_names_pairs", "record_hits", "record_keep", "bam_exclude_flags",
                                           "record_pairs_rule")] == [0] * 6
        case = bp.by_name("coordinate_sorted")
        with pytest.raises(ValueError, match="samtools collate"):
            mapper.select_records(index, bc.bam_file(case.base), fmt="bam", k=K, exclude_flags=0x900, pairs=True)
        assert dev.get_param("record_names_pairs") == 0 and dev.get_param("record_hits_pending") == 0
        with pytest.raises(ValueError, match="pairs goes with fmt=\"bam\""):
            mapper.select_records(index, b"@a\nACGT\n+\nIIII\n", fmt="fastq", k=2, pairs=True)
    finally:
        mapper.clear_cache()


CLI = {"plain": ("patterns__any", []),
       "both_invert": ("patterns__both_invert", ["--pair-rule", "both", "--invert"]),
       "mate_suffix_bgzf": ("suffix_on__any", ["--mate-suffix", "--bgzf"]),
       "excluded_as_stored": ("excluded_between__any", ["--as-stored"])}


@pytest.mark.parametrize("kind", list(CLI))
def test_command_line_end_to_end(kmm, index, tmp_path, kind):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    name, options = CLI[kind]
    case = bp.by_name(name)
    assert case.base.sel == bp.X900                                                 # (--bam-pairs brings the mask: none is given)
    base = case.base if "--as-stored" in options else case.base._replace(name=case.base.name + "_cli", orig=True)
    case = case._replace(name="cli_" + kind, base=base)
    e = bp.expected(case)
    path, npz = str(tmp_path / "collated.bam"), str(tmp_path / "index.npz")
    data = bc.bam_file(base, block=1999)
    open(path, "wb").write(data)
    index.to_file(npz)
    out, hits_out = str(tmp_path / "kept.fq"), str(tmp_path / "hits")
    seen, kept = run_argument_parser(["select-reads", "-i", npz, "-f", path, "--bam-to-fastq", "--bam-pairs", "-k", str(K), "-c", "3000", "-I",
                                      str(rc.NO_FILTER), "-o", out, "--hits-output", hits_out] + options)
    assert (seen, kept) == (2 * e.n_pairs, 2 * e.n_kept)
    written = open(out, "rb").read()
    assert (bc.inflate(written) if "--bgzf" in options else written) == e.text1
    assert np.array_equal(np.load(hits_out + ".npy"), e.hits) and np.array_equal(np.load(hits_out + ".windows.npy"), e.windows)
    assert open(path, "rb").read() == data


def test_command_line_errors_carry_the_hint(kmm, index, tmp_path):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    npz = str(tmp_path / "index.npz")
    index.to_file(npz)
    for name, message in (("coordinate_sorted", "are not mates: collate the file by name \\(`samtools collate`\\)"),
                          ("odd_count", "the stream ends with an unpaired record")):
        path = str(tmp_path / (name + ".bam"))
        open(path, "wb").write(bc.bam_file(bp.by_name(name).base))
        with pytest.raises(ValueError, match=message):
            run_argument_parser(["select-reads", "-i", npz, "-f", path, "--bam-to-fastq", "--bam-pairs", "-k", str(K), "-o",
                                 str(tmp_path / "kept.fq")])
