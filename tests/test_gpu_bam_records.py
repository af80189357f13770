"""GPU tests of the raw form of the BAM keep (include/kmm.h "record_bam"): every case of tests/bam_records_cases.py
through kmm_map_bam with the switch and the record-keep mode on, against the catalogue's independent model (held to its
conditions by tests/test_bam_records_on_the_cpu.py) and against the entries the same file gives with the switch off; windows that
end inside the header, a block_size word and a record; pieces of one KiB; calls without a take, a device-side take, a short
capacity, the BGZF take; the identity; the mode's purity; the refusals; a malformed record; kmm_bam_stream_header; the façade,
`select-reads --bam-out`, and its output read back through this repository's own BAM route."""
import numpy as np
import pytest

from tests import bam_records_cases as br
from tests import read_hits_cases as rc
from tests import record_keep_cases as rk
from tests.test_gpu_bam import _feed

pytestmark = pytest.mark.gpu

CASES = br.all_cases()
IDS = [c.name for c in CASES]
K = br.K


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _open(kmm, k=K):
    index = rc.genome_index(k)
    return kmm.DeviceIndex.from_index(index, index.max_node_id())


def _file(base, **kw):
    return np.frombuffer(br.bam_file(base, **kw), dtype=np.uint8)


def _select(dev, base):
    sel = base.sel
    dev.set_param("bam_exclude_flags", sel.excl)
    dev.set_param("bam_include_flags", sel.incl)
    dev.set_param("bam_min_mapq", sel.min_mapq)
    dev.set_record_regions([(None, ref, beg, end) for ref, beg, end in (sel.regions or [])], sel.keep_unplaced)
    dev.set_param("original_strand", int(base.orig))


def _rule(case):
    return dict(min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)


def _raw_on(dev, case):
    _select(dev, case.base)
    dev.record_hits(True, windows=True)
    dev.record_keep(True, **_rule(case))
    dev.record_bam(True)


def _map(dev, comp, k=K, **kw):
    return dev.map_bam(comp, first=True, last=True, k=k, max_index_lookup_frequency=rc.NO_FILTER, **kw)


def _same_bytes(got, want):
    got = bytes(memoryview(got)) if not isinstance(got, bytes) else got
    assert len(got) == len(want), (len(got), len(want))
    if got != want:
        at = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        raise AssertionError("first difference at byte %d of %d: %r, wanted %r" % (at, len(want), got[max(at - 20, 0):at + 20],
                                                                                    want[max(at - 20, 0):at + 20]))


def _check_take(dev, case, times=1):
    """Both queues against the model: the bytes, the record count, the entries, and the rule over the entries."""
    raw, n_kept, keep, want_h, want_w = br.expected(case)
    assert dev.get_param("record_keep_pending_bytes") == times * len(raw)
    assert dev.get_param("record_keep_pending_records") == times * n_kept
    got, n = dev.take_kept_records()
    _same_bytes(got, raw * times)
    assert n == times * n_kept
    hits, windows = dev.take_record_hits()
    assert np.array_equal(hits, np.tile(want_h, times)) and np.array_equal(windows, np.tile(want_w, times))
    assert np.array_equal(rk.keep_rule(hits, windows, **_rule(case)), np.tile(keep, times))


def _case(name):
    return next(c for c in CASES if c.name == name)


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model_and_against_the_entries_with_the_switch_off(kmm, case):
    base = case.base
    d = br.decoded(base)
    comp = _file(base)
    with _open(kmm, base.k) as dev:
        _raw_on(dev, case)
        assert dev.get_param("record_bam") == 1
        assert _map(dev, comp, base.k) == (comp.shape[0], len(d.records))
        assert dev.get_param("bam_records_excluded") == d.excluded and dev.get_param("bam_records") == len(d.records)
        assert dev.bam_header() == base.payload[:d.hdr]
        _check_take(dev, case)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # the same file in plain record-hits mode — the path the library had before: the same entries, nothing kept
        dev.record_keep(False)
        dev.record_bam(False)
        assert _map(dev, comp, base.k) == (comp.shape[0], len(d.records))
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, br.expected(case)[3]) and np.array_equal(windows, br.expected(case)[4])
        assert dev.get_param("record_keep_pending_bytes") == 0


# ---------------------------------------------------------------------------------------------- windows, pieces, the queue
def _small_members(base, block):
    """The header in members of 16 inflated bytes — a first window can end inside it — the records in members of `block`."""
    from kmer_mapper_amd import reads_io
    hdr = br.decoded(base).hdr
    return reads_io.bgzf_members(base.payload[:hdr], 16) + reads_io.bgzf_members(base.payload[hdr:], block) + reads_io.BGZF_EOF


@pytest.mark.parametrize("name,block,step", [("sizes__default", 3, 4_000), ("aux__default", 97, 100), ("straddle__default", 4001, 9_000),
                                             ("long__default", 0xFF00, 30_000), ("selection__default", 301, 700),
                                             ("tiles__default", 1999, 5_000)])
def test_windows_that_end_inside_the_header_a_block_size_word_and_a_record(kmm, name, block, step):
    """The stream cut where the caller's windows happen to end (tests/test_gpu_bam.py's loop, hinted and not): members of three
    bytes end inside every block_size word, larger ones inside heads and aux; the bytes behind a window's last whole record are
    carried, and the kept records of every window go behind those of the one before."""
    case = _case(name)
    base = case.base
    d = br.decoded(base)
    comp = _small_members(base, block)
    with _open(kmm, base.k) as dev:
        _raw_on(dev, case)
        for hinted in (False, True):
            assert _feed(dev, comp, step=step, hinted=hinted, k=base.k) == len(d.records)
            assert dev.bam_header() == base.payload[:d.hdr]
            _check_take(dev, case)


@pytest.mark.parametrize("name", ["sizes__default", "aux__invert", "selection__invert"])
def test_pieces_of_one_kib(kmm, name):
    case = _case(name)
    comp = _file(case.base)
    with _open(kmm, case.base.k) as dev:
        _raw_on(dev, case)
        dev.set_param("debug_records_piece_kb", 1)
        assert _map(dev, comp, case.base.k)[1] == len(br.decoded(case.base).records)
        _check_take(dev, case)


def test_calls_without_a_take_a_device_side_take_a_short_capacity_and_the_bgzf_take(kmm):
    import torch
    case = _case("aux__default")
    raw, n_kept = br.expected(case)[:2]
    comp = _file(case.base)
    assert len(raw) % 16 != 0                                                     # (the second call's records start off a line)
    with _open(kmm) as dev:
        _raw_on(dev, case)
        _map(dev, comp)
        _map(dev, comp)
        _check_take(dev, case, times=2)
        _map(dev, comp)
        _map(dev, comp)
        short = torch.zeros(2 * len(raw) - 1, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="%d bytes of %d records are pending" % (2 * len(raw), 2 * n_kept)):
            dev.take_kept_records(out=short)
        assert not short.any() and dev.get_param("record_keep_pending_bytes") == 2 * len(raw)
        out = torch.full((2 * len(raw) + 7,), 0xEE, dtype=torch.uint8, device="cuda")
        assert dev.take_kept_records(out=out) == (2 * len(raw), 2 * n_kept)
        got = out.cpu().numpy()
        assert got[:2 * len(raw)].tobytes() == raw * 2 and (got[2 * len(raw):] == 0xEE).all()
        assert dev.take_record_hits()[0].shape == (2 * len(br.decoded(case.base).records),)
        # the BGZF take, inflated by the tests' own reader
        big = _case("big__default")
        _raw_on(dev, big)
        _map(dev, _file(big.base))
        members, n_text, n = dev.take_kept_bgzf()
        want = br.expected(big)[0]
        assert (n_text, n) == (len(want), br.expected(big)[1]) and n_text > 1 << 20
        _same_bytes(br.inflate(members.tobytes()), want)
        dev.take_record_hits()


def test_the_identity_the_inflated_output_is_the_inflated_input(kmm):
    """No selection, min_hits 0: every record is kept, and header + records + the end-of-file block inflate to the input."""
    from kmer_mapper_amd import util
    from kmer_mapper_amd.gz_io import BGZF_EOF
    for name in ("aux", "long", "sizes"):
        case = br.identity_case(name)
        base = case.base
        comp = _file(base)
        with _open(kmm, base.k) as dev:
            _raw_on(dev, case)
            _map(dev, comp, base.k)
            out = util.bgzf_compress(dev.bam_header()).tobytes() + dev.take_kept_bgzf()[0].tobytes() + BGZF_EOF
        _same_bytes(br.inflate(out), br.inflate(comp.tobytes()))
        assert br.inflate(out) == base.payload


# ---------------------------------------------------------------------------------------------- purity
def test_purity_the_counts_do_not_move_and_everything_off_is_a_fresh_handle(kmm, oracle):
    case = _case("aux__default")
    base = case.base
    comp = _file(base)
    index = rc.genome_index(K)
    recs = br.decoded(base).all_records
    stored = rc.batch([np.frombuffer(r.seq, dtype=np.uint8) for r in recs])        # everything off: SEQ as stored
    want = oracle.map_reads(index, index.max_node_id(), stored[0], stored[1], K, n_threads=4)[0]
    with _open(kmm) as dev, _open(kmm) as fresh:
        for h in (dev, fresh):
            assert h.get_param("record_bam") == 0
            assert _map(h, comp) == (comp.shape[0], len(recs))
        counts, stats = dev.get_node_counts().copy(), dev.get_stats()
        assert np.array_equal(counts, want) and counts.any()
        _raw_on(dev, case)
        _map(dev, comp)
        assert np.array_equal(dev.get_node_counts(), counts) and dev.get_stats() == stats
        _check_take(dev, case)
        dev.record_bam(False)
        dev.record_keep(False)
        dev.record_hits(False)
        dev.set_param("original_strand", 0)
        _map(dev, comp)
        _map(fresh, comp)
        assert np.array_equal(dev.get_node_counts(), fresh.get_node_counts()) and np.array_equal(dev.get_node_counts(), 2 * want)
        assert dev.get_stats() == fresh.get_stats()
        # "record_bam" 1 does nothing on the text routes
        from kmer_mapper_amd import _lib
        text = np.frombuffer(br.decoded(base).text, dtype=np.uint8)
        before = fresh.map_records(text, fmt=_lib.FORMAT_FASTA2, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        dev.set_param("record_bam", 1)
        assert dev.map_records(text, fmt=_lib.FORMAT_FASTA2, k=K, max_index_lookup_frequency=rc.NO_FILTER) == before
        assert np.array_equal(dev.get_node_counts(), fresh.get_node_counts())


def test_the_kernels_are_timed_under_one_id_and_not_launched_with_the_switch_off(kmm):
    from kmer_mapper_amd import _lib
    case = _case("aux__default")
    comp = _file(case.base)
    with _open(kmm) as dev:
        dev.set_timing(True)
        _select(dev, case.base)
        dev.record_hits(True, windows=True)
        _map(dev, comp)                                                             # record-hits mode alone
        assert dev.get_timing(_lib.KERNEL_BAM_RAW)[1] == 0
        dev.take_record_hits()
        dev.record_keep(True, **_rule(case))
        dev.record_bam(True)
        _map(dev, comp)
        assert dev.get_timing(_lib.KERNEL_BAM_RAW)[1] == 1
        _check_take(dev, case)


# ---------------------------------------------------------------------------------------------- refusals, failing calls
def test_refusals_map_nothing_and_append_nothing(kmm):
    case = _case("aux__default")
    comp = _file(case.base)
    pending = lambda dev: (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                           dev.get_param("record_keep_pending_records"))
    with _open(kmm) as dev:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="record_bam takes 0 or 1"):
                dev.set_param("record_bam", bad)
        dev.record_bam(True)                                                        # "record_hits" and "record_keep" are 0
        with pytest.raises(ValueError, match="\"record_bam\" is 1 and \"record_hits\" is 0"):
            _map(dev, comp)
        dev.record_hits(True, windows=True)
        with pytest.raises(ValueError, match="\"record_bam\" is 1 and \"record_keep\" is 0"):
            _map(dev, comp)
        dev.record_keep(True)
        dev.record_names(True)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_names\" are 1"):
            _map(dev, comp)
        dev.record_names(True, pairs=True)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_names\" are 1"):
            _map(dev, comp)
        dev.set_param("record_names", 0)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_names_pairs\" are 1"):
            _map(dev, comp)
        dev.record_names(False)
        dev.record_pairs(True)
        with pytest.raises(ValueError, match="\"record_bam\" and \"record_pairs\" are 1"):
            _map(dev, comp)
        dev.record_pairs(False)
        dev.set_param("bam_n_ref", 3)                                               # a mid-stream share
        with pytest.raises(ValueError, match="\"record_bam\" is 1 and the stream begins behind the header"):
            dev.map_bam(comp, first=True, last=True, k=K, mid_stream=True, head_skip=0)
        assert pending(dev) == (0, 0, 0)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        with pytest.raises(ValueError, match="no BAM stream with a header"):        # (nothing was mapped: no stream was started)
            dev.bam_header()
        # text and raw records never share a queue: the switch does not move while kept bytes are pending
        _raw_on(dev, case)
        _map(dev, comp)
        with pytest.raises(ValueError, match="record_bam 0 with %d kept bytes pending" % len(br.expected(case)[0])):
            dev.record_bam(False)
        assert dev.get_param("record_bam") == 1
        _check_take(dev, case)
        dev.record_bam(False)
        dev.record_names(True)                                                      # the named text pending: the switch stays off
        _map(dev, comp)
        with pytest.raises(ValueError, match="record_bam 1 with .* kept bytes pending"):
            dev.record_bam(True)
        dev.take_kept_records()
        dev.take_record_hits()
        dev.record_names(False)
        _raw_on(dev, case)                                                          # the handle serves the next call
        _map(dev, comp)
        _check_take(dev, case)


def test_a_malformed_record_behind_a_good_window_leaves_both_queues_as_they_were(kmm):
    from kmer_mapper_amd import reads_io
    case = _case("aux__default")
    base = case.base
    d = br.decoded(base)
    recs, hdr = d.all_records, d.hdr
    bad = bytearray(base.payload)
    victim = recs[len(recs) - 2]
    bad[victim.start + 36 + len(victim.name)] = 1
    cut = recs[len(recs) // 2].start                                               # members end at a record start: the first window is whole
    comp_1 = reads_io.bgzf_members(bytes(bad[:hdr])) + reads_io.bgzf_members(bytes(bad[hdr:cut]))
    comp_2 = reads_io.bgzf_members(bytes(bad[cut:])) + reads_io.BGZF_EOF
    comp = np.frombuffer(comp_1 + comp_2, dtype=np.uint8)
    with _open(kmm) as dev:
        _raw_on(dev, case)
        used, n_1 = dev.map_bam(comp[:len(comp_1)], first=True, last=False, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n_1) == (len(comp_1), len(recs) // 2)
        state = (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"), dev.get_param("record_keep_pending_records"))
        assert state[0] == n_1 and state[1] > 0
        with pytest.raises(ValueError, match="does not fit its block_size"):
            dev.map_bam(comp[len(comp_1):], first=False, last=True, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                dev.get_param("record_keep_pending_records")) == state
        got, n = dev.take_kept_records()
        keep = br.expected(case)[2][:n_1]
        _same_bytes(got, b"".join(base.payload[r.start:r.start + r.size] for r, kp in zip(d.records[:n_1], keep) if kp))
        assert n == int(keep.sum())
        dev.reset()
        assert dev.get_param("record_keep_pending_bytes") == 0 and dev.get_param("record_hits_pending") == 0
        _map(dev, _file(base))                                                      # and the handle goes on
        _check_take(dev, case)


def test_the_stream_header(kmm):
    """kmm_bam_stream_header: the bytes of the header, a short capacity that names the size, and no stream started."""
    import ctypes
    from kmer_mapper_amd import _lib, reads_io
    base = br.bases()["selection"]                                                  # (three references)
    d = br.decoded(base)
    header = base.payload[:d.hdr]
    long_header = reads_io.bam_header([(b"chr%d" % i, 1000 + i) for i in range(5000)], b"@HD\tVN:1.6\n" + b"@CO\tpadding\n" * 200)
    with _open(kmm) as dev:
        n = ctypes.c_int64(-1)
        assert _lib.lib().kmm_bam_stream_header(dev._h, None, 0, ctypes.byref(n)) == _lib.KMM_ERR_INVALID_ARG and n.value == 0
        with pytest.raises(ValueError, match="no BAM stream with a header"):
            dev.bam_header()
        _map(dev, _file(base))                                                      # the switch is not needed for it
        assert dev.bam_header() == header
        buf = np.zeros(len(header), np.uint8)
        assert _lib.lib().kmm_bam_stream_header(dev._h, buf.ctypes.data, len(header) - 1, ctypes.byref(n)) == _lib.KMM_ERR_INVALID_ARG
        assert n.value == len(header) and not buf.any()
        assert ("the header has %d bytes, capacity is %d" % (len(header), len(header) - 1)) in _lib.lib().kmm_last_error().decode()
        assert _lib.lib().kmm_bam_stream_header(dev._h, buf.ctypes.data, len(header), ctypes.byref(n)) == _lib.KMM_OK
        assert buf.tobytes() == header
        # a header of 100 KB over many small members, then the next stream's
        comp = np.frombuffer(reads_io.bgzf_members(long_header, 0x1F00) + reads_io.bgzf_members(base.payload[d.hdr:]) + reads_io.BGZF_EOF,
                             np.uint8)
        _map(dev, comp)
        assert dev.bam_header() == long_header and len(long_header) > 1 << 16
        # a first window that ends inside the header: no header yet; a mid-stream share: none
        used, _ = dev.map_bam(comp[:2000], first=True, last=False, k=K)
        assert used == 0
        with pytest.raises(ValueError, match="no BAM stream with a header"):
            dev.bam_header()


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    index = rc.genome_index(K)
    try:
        for name in ("aux__default", "long__invert", "selection_flags_only__default", "straddle__permille_200"):
            case = _case(name)
            base = case.base
            _, _, _, want_h, want_w = br.expected(case)
            got, hits, windows = mapper.select_records(index, br.bam_file(base), fmt="bam", output="bam", k=K,
                                                       max_index_lookup_frequency=rc.NO_FILTER, exclude_flags=base.sel.excl,
                                                       original_strand=base.orig, **_rule(case))
            assert got[-28:] == mapper_eof() and br.inflate(got) == br.expected_file(case)
            assert np.array_equal(hits, want_h) and np.array_equal(windows, want_w)
            br.read_bam(br.inflate(got))                                            # the tests' independent reader accepts it
        assert len(mapper._CACHE) == 1
        dev = next(iter(mapper._CACHE.values()))[0]                                 # the cached handle is left as it was found
        assert [dev.get_param(name) for name in ("record_bam", "record_names", "record_hits", "record_keep", "bam_exclude_flags",
                                                 "original_strand", "record_keep_pending_bytes")] == [0] * 7
        for kw in (dict(fmt="fastq"), dict(fmt="bam", mate_suffix=True), dict(fmt="bam", pairs=True), dict(fmt="bam", compress=True)):
            with pytest.raises(ValueError, match="output=\"bam\""):
                mapper.select_records(index, b"@a\nACGT\n+\nIIII\n", k=2, output="bam", **kw)
    finally:
        mapper.clear_cache()


def mapper_eof():
    from kmer_mapper_amd.gz_io import BGZF_EOF
    return BGZF_EOF


CLI = {"regions": (["--regions", "chr1:1001-2000", "--exclude-flags", "0x400", "--include-flags", "1", "--min-mapq", "20"],
                   lambda b: b["selection"]._replace(name="cli_regions", orig=True)),
       "invert": (["--invert"], lambda b: b["aux"]),
       "long": ([], lambda b: b["long"]._replace(name="cli_long", orig=True))}


@pytest.mark.parametrize("kind", list(CLI))
def test_command_line_end_to_end_and_the_output_as_input(kmm, tmp_path, kind):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    index = rc.genome_index(K)
    options, pick = CLI[kind]
    base = pick(br.bases())
    case = br.RCase("cli_" + kind, base, 2, 0, "--invert" in options)
    raw, n_kept, keep, hits, windows = br.expected(case)
    assert 0 < n_kept < len(keep)
    path, npz = str(tmp_path / "reads.bam"), str(tmp_path / "index.npz")
    data = br.bam_file(base, block=1999)
    open(path, "wb").write(data)
    index.to_file(npz)
    out, hits_out = str(tmp_path / "kept.bam"), str(tmp_path / "hits")
    seen, kept = run_argument_parser(["select-reads", "-i", npz, "-f", path, "--bam-out", "-k", str(K), "-c", "3000", "-I", str(rc.NO_FILTER),
                                      "--min-hits", "2", "-o", out, "--hits-output", hits_out] + options)
    assert (seen, kept) == (len(keep), n_kept)
    written = open(out, "rb").read()
    assert written.endswith(mapper_eof()) and br.inflate(written) == br.expected_file(case)
    assert np.array_equal(np.load(hits_out + ".npy"), hits) and np.array_equal(np.load(hits_out + ".windows.npy"), windows)
    assert open(path, "rb").read() == data
    # the output as input: this repository's own BAM route reads the file back and gives the kept records' entries
    again = str(tmp_path / "again")
    run_argument_parser(["read-hits", "-i", npz, "-f", out, "-k", str(K), "-I", str(rc.NO_FILTER), "-o", again, "--windows", "--device-parser",
                         "--original-strand"])
    assert np.array_equal(np.load(again + ".npy"), hits[keep]) and np.array_equal(np.load(again + ".windows.npy"), windows[keep])
