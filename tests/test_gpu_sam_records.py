"""GPU tests of SAM lines kept as SAM lines (include/kmm.h "record_sam"): every case of tests/sam_records_cases.py
through kmm_map_records with the switch and the record-keep mode on, byte for byte against the catalogue's independent model
(held to its conditions by tests/test_sam_records_on_the_cpu.py), the entries too; the BGZF and gzip routes; the BGZF take;
pieces of one KiB and streams in windows cut inside lines; a malformed line in a later piece; the refusals; the switch off — no
launch of the keep step, the entries of the record-hits mode, SAM still refused in the keep mode; the façade and the command
line end to end."""
import gzip
import zlib

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import sam_records_cases as sr

pytestmark = pytest.mark.gpu

CASES = sr.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _open(kmm, k=sr.K):
    index = rc.genome_index(k)
    return kmm.DeviceIndex.from_index(index, index.max_node_id())


def _select(dev, case):
    incl, min_mapq, regions, keep_unplaced = case.sel
    dev.set_param("bam_exclude_flags", case.excl)
    dev.set_param("bam_include_flags", incl)
    dev.set_param("bam_min_mapq", min_mapq)
    dev.set_record_regions([(name, -1, beg, end) for name, beg, end in (regions or [])], keep_unplaced)
    dev.set_param("original_strand", int(case.orig))


def _rule(case):
    return dict(min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)


def _raw_on(dev, case):
    _select(dev, case)
    dev.record_hits(True, windows=True)
    dev.record_keep(True, **_rule(case))
    dev.record_sam(True, header=case.mode == 1)


def _arr(data):
    return np.frombuffer(bytes(data), dtype=np.uint8)


def _map(dev, case, text=None, **kw):
    from kmer_mapper_amd import _lib
    return dev.map_records(_arr(case.text if text is None else text), fmt=_lib.FORMAT_SAM, k=case.k, max_index_lookup_frequency=rc.NO_FILTER,
                           also_revcomp=case.revcomp, **kw)


def _same_bytes(got, want):
    got = bytes(memoryview(got)) if not isinstance(got, bytes) else got
    assert len(got) == len(want), (len(got), len(want))
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError("first difference at byte %d of %d: %r, wanted %r" % (at, len(want), got[max(at - 20, 0):at + 20],
                                                                                    want[max(at - 20, 0):at + 20]))


def _check_take(dev, want, times=1):
    """Both queues against the model: the bytes, the record count (header lines are not counted), the entries."""
    assert dev.get_param("record_keep_pending_bytes") == times * len(want.out)
    assert dev.get_param("record_keep_pending_records") == times * want.n_kept
    got, n = dev.take_kept_records()
    _same_bytes(got, want.out * times)
    assert n == times * want.n_kept
    if want.n_records:
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, np.tile(want.hits, times)) and np.array_equal(windows, np.tile(want.windows, times))
    else:
        assert dev.get_param("record_hits_pending") == 0


def _inflate(members):
    """Concatenated gzip members through Python's zlib"""
    out, rest = [], bytes(members)
    while rest:
        d = zlib.decompressobj(31)
        out.append(d.decompress(rest))
        assert d.eof
        rest = d.unused_data
    return b"".join(out)


def _counters(dev):
    return dev.get_param("sam_records"), dev.get_param("sam_records_excluded"), dev.get_param("sam_header_lines")


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model_and_against_the_entries_with_the_switch_off(kmm, case):
    want = sr.expected(case)
    with _open(kmm, case.k) as dev:
        _raw_on(dev, case)
        assert dev.get_param("record_sam") == case.mode
        assert _map(dev, case) == (want.consumed, want.n_records)
        assert _counters(dev) == (want.n_records, want.n_excluded, want.n_headers)
        _check_take(dev, want)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # the same text in plain record-hits mode — the path the library had before: the same entries and counters, nothing kept
        dev.record_keep(False)
        dev.record_sam(False)
        assert _map(dev, case) == (want.consumed, want.n_records)
        assert _counters(dev) == (2 * want.n_records, 2 * want.n_excluded, 2 * want.n_headers)      # (they count on, as they did)
        if want.n_records:
            hits, windows = dev.take_record_hits()
            assert np.array_equal(hits, want.hits) and np.array_equal(windows, want.windows)
        assert dev.get_param("record_keep_pending_bytes") == 0


BLOCKS = sr.block_cases()


@pytest.mark.parametrize("case", BLOCKS, ids=[c.name for c in BLOCKS])
def test_more_than_one_block_of_spans_and_of_tiles(kmm, case):
    """The second level of both prefixes on the device: more than two blocks of 1024 spans (k_sam_raw_flags in several workgroups,
    k_sam_raw_scan over several blocks, a non-zero block base in k_sam_raw_copy), and more than 1024 tiles with records and header
    lines on both sides of tile 1024 (k_sam_raw_tiles in two workgroups; both columns of the second block's base non-zero in the
    write with spans), with the header lines kept and dropped.  The queue's tail is moved off a 16-byte line first."""
    from kmer_mapper_amd import _lib, reads_io
    want = sr.expected(case)
    small = sr.by_name("mixed")._replace(k=case.k, excl=case.excl, sel=case.sel, orig=case.orig, revcomp=case.revcomp, min_hits=case.min_hits,
                                         min_permille=case.min_permille, invert=case.invert, mode=case.mode)
    first = sr.model(small)
    bgzf = _arr(reads_io.bgzf_members(case.text) + reads_io.BGZF_EOF)
    with _open(kmm, case.k) as dev:
        _raw_on(dev, case)
        assert _map(dev, case) == (want.consumed, want.n_records)
        assert _counters(dev) == (want.n_records, want.n_excluded, want.n_headers)
        _check_take(dev, want)
        # behind another call's kept lines (the tail at some residue), and through the BGZF route
        assert _map(dev, small) == (first.consumed, first.n_records)
        assert dev.map_bgzf(bgzf, fmt=_lib.FORMAT_SAM, k=case.k, max_index_lookup_frequency=rc.NO_FILTER, first=True,
                            last=True) == (bgzf.shape[0], want.n_records)
        got, n = dev.take_kept_records()
        _same_bytes(got, first.out + want.out)
        assert n == first.n_kept + want.n_kept
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, np.concatenate([first.hits, want.hits])) and np.array_equal(windows, np.concatenate([first.windows, want.windows]))


@pytest.mark.parametrize("name", ["mixed", "unterminated_last_line", "mixed_selection_no_header"])
def test_the_bgzf_and_gzip_routes(kmm, name):
    """kmm_map_bgzf and kmm_map_gzip on their inflated bytes; KMM_FORMAT_LAST_CHUNK supplies a final line's newline, which is kept
    as the stage holds it."""
    from kmer_mapper_amd import _lib, reads_io
    case = sr.by_name(name)
    want = sr.model(case, sr.with_final_newline(case.text))
    bgzf = _arr(reads_io.bgzf_members(case.text, 1500) + reads_io.BGZF_EOF)
    gz = _arr(gzip.compress(case.text, 6))
    kw = dict(fmt=_lib.FORMAT_SAM, k=case.k, max_index_lookup_frequency=rc.NO_FILTER, first=True, last=True)
    with _open(kmm, case.k) as dev:
        _raw_on(dev, case)
        assert dev.map_bgzf(bgzf, **kw) == (bgzf.shape[0], want.n_records)
        _check_take(dev, want)
        assert dev.map_gzip(gz, **kw) == (gz.shape[0], want.n_records)
        _check_take(dev, want)


def test_the_bgzf_take_inflates_to_the_plain_take(kmm):
    case = sr.by_name("long_lines")
    want = sr.expected(case)
    with _open(kmm) as dev:
        _raw_on(dev, case)
        _map(dev, case)
        _map(dev, case)                                                              # two calls, one take: the second goes behind the first
        members, n_text, n = dev.take_kept_bgzf()
        assert (n_text, n) == (2 * len(want.out), 2 * want.n_kept)
        _same_bytes(_inflate(members.tobytes()), want.out * 2)
        assert dev.get_param("record_keep_pending_bytes") == 0
        dev.take_record_hits()
        _map(dev, case)
        _check_take(dev, want)


# ---------------------------------------------------------------------------------------------- pieces and windows
@pytest.mark.parametrize("name", ["mixed", "long_lines", "tile_edges", "dense_k1", "crlf", "mixed_selection"])
def test_pieces_of_one_kib_give_the_one_shot_result(kmm, name):
    """"debug_records_piece_kb" 1: every piece ends behind its last whole line, lines lie across the cuts, and a line longer than a
    piece ends the call in front of it (the caller brings it again)."""
    case = sr.by_name(name)
    want = sr.expected(case)
    longest = max(n for _, n in sr.lines_of(case.text))
    with _open(kmm, case.k) as dev:
        _raw_on(dev, case)
        dev.set_param("debug_records_piece_kb", 1)
        used, n = _map(dev, case)
        if longest <= 1024:
            assert (used, n) == (want.consumed, want.n_records)
            _check_take(dev, want)
        else:
            # the call stops in front of the line no piece can hold: what it took is the model of that prefix
            assert 0 < used < want.consumed and case.text[used - 1:used] == b"\n"
            _check_take(dev, sr.model(case, case.text[:used]))
        dev.set_param("debug_records_piece_kb", 0)


@pytest.mark.parametrize("name,block,step", [("mixed", 97, 700), ("long_lines", 1500, 1000), ("unterminated_last_line", 301, 450),
                                             ("dense_k1_inverted_no_header", 64, 333)])
def test_a_stream_in_windows_cut_inside_lines(kmm, name, block, step):
    """The carry: BGZF windows that end wherever the caller's buffer ends; members of `block` inflated bytes end inside lines;
    the kept lines of every window go behind those of the one before."""
    from kmer_mapper_amd import _lib, reads_io
    case = sr.by_name(name)
    want = sr.model(case, sr.with_final_newline(case.text))
    comp = _arr(reads_io.bgzf_members(case.text, block) + reads_io.BGZF_EOF)
    with _open(kmm, case.k) as dev:
        _raw_on(dev, case)
        pos, total, end, size = 0, 0, min(step, comp.shape[0]), comp.shape[0]
        while pos < size:
            used, n = dev.map_bgzf(comp[pos:end], fmt=_lib.FORMAT_SAM, k=case.k, max_index_lookup_frequency=rc.NO_FILTER, first=pos == 0,
                                   last=end == size)
            pos += used
            total += n
            if pos < end and end == size:
                assert used > 0
                continue
            end = min(end + step, size)
        assert total == want.n_records
        _check_take(dev, want)


# ---------------------------------------------------------------------------------------------- failing calls, refusals
def test_a_malformed_line_in_the_second_piece_leaves_both_queues_as_they_were(kmm):
    case = sr.by_name("mixed")
    want = sr.expected(case)
    bad, at = sr.malformed_behind(case.text)
    assert at > 2048
    with _open(kmm) as dev:
        _raw_on(dev, case)
        _map(dev, case)
        state = (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"), dev.get_param("record_keep_pending_records"))
        assert state == (want.n_records, len(want.out), want.n_kept)
        counters = _counters(dev)
        dev.set_param("debug_records_piece_kb", 1)
        with pytest.raises(ValueError, match="SAM line at byte %d of the chunk: fewer than 11" % at):
            _map(dev, case, bad)
        assert (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                dev.get_param("record_keep_pending_records")) == state
        assert _counters(dev) == counters
        dev.set_param("debug_records_piece_kb", 0)
        with pytest.raises(ValueError, match="SAM line at byte %d of the chunk: fewer than 11" % at):
            _map(dev, case, bad)                                                     # one piece: the same
        _check_take(dev, want)
        _map(dev, case)                                                              # and the handle goes on
        _check_take(dev, want)


def test_refusals_map_nothing_and_append_nothing(kmm):
    from kmer_mapper_amd import _lib, reads_io
    case = sr.by_name("mixed")
    want = sr.expected(case)
    bgzf = _arr(reads_io.bgzf_members(case.text) + reads_io.BGZF_EOF)
    gz = _arr(gzip.compress(case.text))
    kw = dict(fmt=_lib.FORMAT_SAM, k=case.k, first=True, last=True)
    pending = lambda dev: (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                           dev.get_param("record_keep_pending_records"))
    with _open(kmm) as dev:
        routes = (lambda: _map(dev, case), lambda: dev.map_bgzf(bgzf, **kw), lambda: dev.map_gzip(gz, **kw))
        for bad in (3, -1):
            with pytest.raises(ValueError, match="record_sam takes 0, 1 .* or 2"):
                dev.set_param("record_sam", bad)
        for mode in (1, 2):
            dev.set_param("record_sam", mode)                                       # "record_hits" and "record_keep" are 0
            for call in routes:
                with pytest.raises(ValueError, match="\"record_sam\" is %d and \"record_hits\" is 0" % mode):
                    call()
        dev.record_hits(True, windows=True)
        for call in routes:
            with pytest.raises(ValueError, match="\"record_sam\" is 2 and \"record_keep\" is 0"):
                call()
        dev.record_keep(True)
        dev.record_pairs(True)
        for call in routes:
            with pytest.raises(ValueError, match="\"record_sam\" is 2 and \"record_pairs\" is 1"):
                call()
        dev.record_pairs(False)
        assert pending(dev) == (0, 0, 0) and _counters(dev) == (0, 0, 0)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # the other formats never read the parameter
        fq = _arr(b"@a\n" + sr.hit_read(80, 3) + b"\n+\n" + b"I" * 80 + b"\n")
        assert dev.map_records(fq, fmt=_lib.FORMAT_FASTQ, k=case.k) == (fq.shape[0], 1)
        assert dev.take_kept_records()[0].tobytes() == fq.tobytes() and dev.take_record_hits()[0].shape == (1,)
        # raw lines and text never share a queue: the switch does not move while kept bytes are pending
        _raw_on(dev, case)
        _map(dev, case)
        for other in (0, 2):
            with pytest.raises(ValueError, match="record_sam %d with %d kept bytes pending" % (other, len(want.out))):
                dev.set_param("record_sam", other)
        assert dev.get_param("record_sam") == 1
        _check_take(dev, want)
        dev.record_sam(False)
        dev.map_records(fq, fmt=_lib.FORMAT_FASTQ, k=case.k)                        # FASTQ text pending: the switch stays off
        with pytest.raises(ValueError, match="record_sam 1 with %d kept bytes pending" % fq.shape[0]):
            dev.record_sam(True)
        dev.take_kept_records()
        dev.take_record_hits()
        _raw_on(dev, case)                                                          # the handle serves the next call
        _map(dev, case)
        _check_take(dev, want)


def test_with_the_switch_off_nothing_of_it_runs_and_sam_stays_refused_in_the_keep_mode(kmm):
    from kmer_mapper_amd import _lib, reads_io
    case = sr.by_name("mixed_selection")
    want = sr.expected(case)
    bgzf = _arr(reads_io.bgzf_members(case.text) + reads_io.BGZF_EOF)
    gz = _arr(gzip.compress(case.text))
    kw = dict(fmt=_lib.FORMAT_SAM, k=case.k, first=True, last=True)
    with _open(kmm) as dev:
        dev.set_timing(True)
        _select(dev, case)
        dev.record_hits(True, windows=True)
        _map(dev, case)                                                             # record-hits mode alone
        assert dev.get_timing(_lib.KERNEL_SAM_RAW) == (0.0, 0)
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, want.hits) and np.array_equal(windows, want.windows)
        dev.record_keep(True, **_rule(case))
        for call in (lambda: _map(dev, case), lambda: dev.map_bgzf(bgzf, **kw), lambda: dev.map_gzip(gz, **kw)):
            with pytest.raises(ValueError, match="QNAME is not carried"):
                call()
        assert dev.get_timing(_lib.KERNEL_SAM_RAW)[1] == 0
        dev.record_sam(True)
        _map(dev, case)
        ms, launches = dev.get_timing(_lib.KERNEL_SAM_RAW)
        assert launches == 2 and ms > 0                                             # the tiles' scan; flags, block scan, copy, advance
        timings = dev.get_timing()
        assert "k_sam_raw" in timings and _lib.KERNEL_NAMES[_lib.KERNEL_SAM_RAW] == "k_sam_raw"
        _check_take(dev, want)


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    from kmer_mapper_amd.gz_io import BGZF_EOF
    try:
        for name in ("mixed", "mixed_no_header", "mixed_excluded_between", "read_orientation", "mixed_inverted", "header_only"):
            case = sr.by_name(name)
            want = sr.expected(case)
            index = rc.genome_index(case.k)
            kw = dict(fmt="sam", output="sam", header=case.mode == 1, k=case.k, max_index_lookup_frequency=rc.NO_FILTER,
                      exclude_flags=case.excl, original_strand=case.orig, **_rule(case))
            got, hits, windows = mapper.select_records(index, case.text, **kw)
            _same_bytes(got, want.out)
            assert np.array_equal(hits, want.hits) and np.array_equal(windows, want.windows)
            packed, _, _ = mapper.select_records(index, case.text, compress=True, **kw)
            assert packed.endswith(BGZF_EOF) and _inflate(packed) == want.out
        assert len(mapper._CACHE) == 1
        dev = next(iter(mapper._CACHE.values()))[0]                                 # the cached handle is left as it was found
        assert [dev.get_param(name) for name in ("record_sam", "record_hits", "record_keep", "bam_exclude_flags", "original_strand",
                                                 "record_keep_pending_bytes", "record_hits_pending")] == [0] * 7
        index = rc.genome_index(sr.K)
        line = b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n"
        with pytest.raises(ValueError, match="QNAME is not carried"):
            mapper.select_records(index, line, fmt="sam", k=sr.K)
        for kw in (dict(fmt="fastq"), dict(fmt="bam"), dict(fmt="sam", pairs=True), dict(fmt="sam", mate_suffix=True),
                   dict(fmt="sam", keep_mates=True)):
            with pytest.raises(ValueError, match="output=\"sam\""):
                mapper.select_records(index, line, k=sr.K, output="sam", **kw)
    finally:
        mapper.clear_cache()


# kind -> (file, output options, selection options, the same selection for the model: exclude mask, include mask)
CLI = {"plain": ("r.sam", [], [], 0, 0), "plain_bgzf_out": ("r.sam", ["--bgzf", "--no-header"], [], 0, 0),
       "sam_gz": ("r.sam.gz", ["--invert"], ["--exclude-flags", "0x100"], 0x100, 0),
       "sam_gz_selected": ("r.sam.gz", ["--bgzf"], ["--exclude-flags", "0x80", "--include-flags", "0x10"], 0x80, 0x10)}


@pytest.mark.parametrize("kind", list(CLI))
def test_command_line_end_to_end(kmm, tmp_path, kind):
    """`select-reads --sam-out` on a .sam and a .sam.gz written by reads_io.write_sam (BGZF: bgzf_members), with and without --bgzf,
    --no-header and --hits-output; the hits are counted in read orientation."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.gz_io import BGZF_EOF
    from kmer_mapper_amd.util import ReadBatch
    from tests import record_hits_cases as rh
    from tests import strand_cases
    name, options, selection, excl, incl = CLI[kind]
    flags = [(0, 16, 0x100, 4, 0x93)[i % 5] for i in range(120)]
    reads = [(sr.hit_read(150, 101 * i), sr.miss_read(150), sr.hit_read(60 + i, 37 * i))[i % 3] for i in range(120)]
    reads = [strand_cases.revcomp(r) if f & 16 and i % 2 else r for i, (r, f) in enumerate(zip(reads, flags))]
    bases, offsets = rh.reads_arrays(reads)
    path, npz = str(tmp_path / name), str(tmp_path / "index.npz")
    header = b"@HD\tVN:1.6\tSO:unsorted\n@CO\tmade for the test\n"
    reads_io.write_sam(path, ReadBatch(bases, offsets), flags=flags, header=header, bgzf=name.endswith(".gz"), block=1999)
    data = open(path, "rb").read()
    text = _inflate(data) if name.endswith(".gz") else data
    case = sr.case("cli_" + kind, text, excl=excl, sel=(incl, 0, None, False), orig=True, min_hits=2, invert="--invert" in options,
                   mode=2 if "--no-header" in options else 1)
    want = sr.model(case)
    assert 0 < want.n_kept < want.n_records and want.n_headers == 2
    rc.genome_index(sr.K).to_file(npz)
    out, hits_out = str(tmp_path / "kept.sam"), str(tmp_path / "hits")
    more = ["--hits-output", hits_out] if kind != "plain" else []
    seen, kept = run_argument_parser(["select-reads", "-i", npz, "-f", path, "--sam-out", "-k", str(sr.K), "-c", "3000", "-I", str(rc.NO_FILTER),
                                      "--min-hits", "2", "-o", out] + options + selection + more)
    assert (seen, kept) == (want.n_records, want.n_kept)
    written = open(out, "rb").read()
    if "--bgzf" in options:
        assert written.endswith(BGZF_EOF)
        written = _inflate(written)
    _same_bytes(written, want.out)
    if more:
        assert np.array_equal(np.load(hits_out + ".npy"), want.hits) and np.array_equal(np.load(hits_out + ".windows.npy"), want.windows)
    assert open(path, "rb").read() == data
