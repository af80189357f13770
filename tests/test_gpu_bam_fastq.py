"""GPU tests of the named FASTQ form of the BAM decode (include/kmm.h "record_names"): every case of
tests/bam_fastq_cases.py through kmm_map_bam with the names and the record-keep mode on, against the catalogue's independent model
(held to its conditions by tests/test_bam_fastq_on_the_cpu.py) and against the entries the same file gives without the names;
windows that end inside the header, a name and a record; calls without a take, a device-side take, a short capacity; the mode's
purity; the refusals; a malformed record; the counters; the façade and `select-reads --bam-to-fastq`."""
import numpy as np
import pytest

from tests import bam_fastq_cases as bc
from tests import read_hits_cases as rc
from tests import record_keep_cases as rk
from tests import select_cases as sc
from tests.test_gpu_bam import _feed

pytestmark = pytest.mark.gpu

CASES = bc.gpu_cases()
IDS = [c.name for c in CASES]
K = bc.K


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


def _file(base, **kw):
    return np.frombuffer(bc.bam_file(base, **kw), dtype=np.uint8)


def _select(dev, base):
    """The base's selection and switches on the handle (the names stay as they are)."""
    sel = base.sel
    dev.set_param("bam_exclude_flags", sel.excl)
    dev.set_param("bam_include_flags", sel.incl)
    dev.set_param("bam_min_mapq", sel.min_mapq)
    dev.set_record_regions([(None, ref, beg, end) for ref, beg, end in (sel.regions or [])], sel.keep_unplaced)
    dev.set_param("original_strand", int(base.orig))


def _rule(case):
    return dict(min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)


def _names_on(dev, case):
    _select(dev, case.base)
    dev.record_hits(True, windows=True)
    dev.record_keep(True, **_rule(case))
    dev.record_names(True, mate_suffix=case.base.suffix)


def _map(dev, comp, **kw):
    return dev.map_bam(comp, first=True, last=True, k=K, max_index_lookup_frequency=rc.NO_FILTER, **kw)


def _same_text(got, want):
    assert got.dtype == np.uint8 and got.shape == (len(want),), (got.shape, len(want))
    if got.tobytes() != want:
        at = next(i for i, (a, b) in enumerate(zip(got.tobytes(), want)) if a != b)
        raise AssertionError("first difference at byte %d of %d: %r, wanted %r" % (at, len(want), got.tobytes()[max(at - 20, 0):at + 20],
                                                                                    want[max(at - 20, 0):at + 20]))


def _check_take(dev, case, times=1):
    """Both queues against the model: the bytes, the record count, the entries, and the rule over the entries."""
    text, n_kept, keep, want_h, want_w = bc.expected(case)
    assert dev.get_param("record_keep_pending_bytes") == times * len(text)
    assert dev.get_param("record_keep_pending_records") == times * n_kept
    got, n = dev.take_kept_records()
    _same_text(got, text * times)
    assert n == times * n_kept
    hits, windows = dev.take_record_hits()
    assert np.array_equal(hits, np.tile(want_h, times)) and np.array_equal(windows, np.tile(want_w, times))
    assert np.array_equal(rk.keep_rule(hits, windows, **_rule(case)), np.tile(keep, times))


def _check_counters(dev, base, times=1):
    d = bc.decoded(base)
    assert dev.get_param("record_name_bytes_replaced") == times * d.replaced
    assert dev.get_param("records_reversed") == times * d.reversed
    assert dev.get_param("records_without_qual") == times * d.no_qual


def _case(name):
    return next(c for c in CASES if c.name == name)


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model_and_against_the_entries_without_names(kmm, index, case):
    base = case.base
    d = bc.decoded(base)
    comp = _file(base)
    with _open(kmm, index) as dev:
        _names_on(dev, case)
        assert dev.get_param("record_names") == 1 and dev.get_param("record_names_mate_suffix") == int(base.suffix)
        assert _map(dev, comp) == (comp.shape[0], len(d.records))
        assert dev.get_param("bam_records_excluded") == d.excluded
        _check_take(dev, case)
        _check_counters(dev, base)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # the same file in the record-hits mode without the names — the path the library had before: the same entries
        dev.record_keep(False)
        dev.record_names(False)
        assert _map(dev, comp) == (comp.shape[0], len(d.records))
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, bc.expected(case)[3]) and np.array_equal(windows, bc.expected(case)[4])
        assert dev.get_param("record_keep_pending_bytes") == 0
        assert dev.get_param("record_name_bytes_replaced") == d.replaced           # (the unnamed decode replaces nothing)


# ---------------------------------------------------------------------------------------------- windows, pieces, the queue
def _small_members(base, block):
    """The header in members of 16 inflated bytes — a first window can end inside it — the records in members of `block`."""
    from kmer_mapper_amd import reads_io
    _, _, hdr = bc.read_bam(base.payload)
    return reads_io.bgzf_members(base.payload[:hdr], 16) + reads_io.bgzf_members(base.payload[hdr:], block) + reads_io.BGZF_EOF


@pytest.mark.parametrize("name,block,step", [("names__default", 301, 100), ("mates_suffix__default", 301, 100),
                                             ("strand_read_orientation__default", 97, 400), ("lengths__default", 0xFF00, 30_000),
                                             ("straddle__default", 4001, 9_000), ("selection__default", 301, 700)])
def test_windows_that_end_inside_the_header_a_name_and_a_record(kmm, index, name, block, step):
    """The stream cut where the caller's windows happen to end (tests/test_gpu_bam.py's loop, hinted and not): members of a few
    hundred bytes end inside names, record heads and qualities, and the bytes behind a window's last whole record are carried."""
    case = _case(name)
    d = bc.decoded(case.base)
    comp = _small_members(case.base, block)
    assert step < 140 or name not in ("names__default", "mates_suffix__default")   # (the first window ends inside the header's members)
    with _open(kmm, index) as dev:
        _names_on(dev, case)
        for hinted in (False, True):
            assert _feed(dev, comp, step=step, hinted=hinted) == len(d.records)
            _check_take(dev, case)
        _check_counters(dev, case.base, times=2)


@pytest.mark.parametrize("name", ["names__default", "mates_suffix__default", "selection__invert"])
def test_pieces_of_one_kib(kmm, index, name):
    case = _case(name)
    comp = _file(case.base)
    assert max(len(t) for t in bc.decoded(case.base).texts) < 1024
    with _open(kmm, index) as dev:
        _names_on(dev, case)
        dev.set_param("debug_records_piece_kb", 1)
        assert _map(dev, comp)[1] == len(bc.decoded(case.base).records)
        _check_take(dev, case)


def test_calls_without_a_take_a_device_side_take_and_a_short_capacity(kmm, index):
    import torch
    case = _case("names__default")
    text, n_kept = bc.expected(case)[:2]
    comp = _file(case.base)
    assert len(text) % 16 != 0
    with _open(kmm, index) as dev:
        _names_on(dev, case)
        _map(dev, comp)
        _map(dev, comp)
        _check_take(dev, case, times=2)
        _map(dev, comp)
        _map(dev, comp)
        short = torch.zeros(2 * len(text) - 1, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="%d bytes of %d records are pending" % (2 * len(text), 2 * n_kept)):
            dev.take_kept_records(out=short)
        assert not short.any() and dev.get_param("record_keep_pending_bytes") == 2 * len(text)
        out = torch.full((2 * len(text) + 7,), 0xEE, dtype=torch.uint8, device="cuda")
        assert dev.take_kept_records(out=out) == (2 * len(text), 2 * n_kept)
        got = out.cpu().numpy()
        assert got[:2 * len(text)].tobytes() == text * 2 and (got[2 * len(text):] == 0xEE).all()
        assert dev.take_record_hits()[0].shape == (2 * len(bc.decoded(case.base).records),)


# ---------------------------------------------------------------------------------------------- purity
def test_purity_the_counts_do_not_move_and_the_switch_off_is_the_library_as_it_was(kmm, index, oracle):
    case = _case("strand_read_orientation__default")
    base = case.base
    comp = _file(base)
    _, recs, _ = bc.read_bam(base.payload)
    stored = rc.batch([np.frombuffer(r.seq, dtype=np.uint8) for r in recs])    # names off, original_strand off: SEQ as stored
    want = oracle.map_reads(index, index.max_node_id(), stored[0], stored[1], K, n_threads=4)[0]
    with _open(kmm, index) as dev, _open(kmm, index) as fresh:
        for h in (dev, fresh):
            assert h.get_param("record_names") == 0 and h.get_param("record_names_mate_suffix") == 0
            assert _map(h, comp) == (comp.shape[0], len(recs))
        counts, stats = dev.get_node_counts().copy(), dev.get_stats()
        assert np.array_equal(counts, want) and counts.any()
        _names_on(dev, case)
        _map(dev, comp)
        assert np.array_equal(dev.get_node_counts(), counts) and dev.get_stats() == stats
        _check_take(dev, case)
        # everything off again: a call counts what it counted on a handle that never had the switch
        dev.record_names(False)
        dev.record_keep(False)
        dev.record_hits(False)
        dev.set_param("original_strand", 0)
        _map(dev, comp)
        _map(fresh, comp)
        assert np.array_equal(dev.get_node_counts(), fresh.get_node_counts()) and np.array_equal(dev.get_node_counts(), 2 * want)
        assert dev.get_stats() == fresh.get_stats()
        # "record_names" 1 does nothing on the text routes
        from kmer_mapper_amd import _lib
        text = np.frombuffer(bc.decoded(base).text, dtype=np.uint8)
        before = fresh.map_records(text, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        dev.set_param("record_names", 1)
        dev.set_param("record_hits", 0)
        assert dev.map_records(text, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER) == before
        assert np.array_equal(dev.get_node_counts(), fresh.get_node_counts())


# ---------------------------------------------------------------------------------------------- refusals, failing calls, counters
def test_refusals_map_nothing_and_append_nothing(kmm, index):
    from kmer_mapper_amd import _lib, reads_io
    case = _case("names__default")
    comp = _file(case.base)
    pending = lambda dev: (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                           dev.get_param("record_keep_pending_records"))
    sam = np.frombuffer(b"r\t4\t*\t0\t0\t*\t*\t0\t0\t" + bc.hit(60, 0) + b"\t*\n", dtype=np.uint8)
    sam_bgzf = np.frombuffer(reads_io.bgzf_members(sam.tobytes()) + reads_io.BGZF_EOF, dtype=np.uint8)
    with _open(kmm, index) as dev:
        for name in ("record_names", "record_names_mate_suffix"):
            for bad in (2, -1):
                with pytest.raises(ValueError, match="%s takes 0 or 1" % name):
                    dev.set_param(name, bad)
        with pytest.raises(ValueError):
            dev.set_param("record_name_bytes_replaced", 0)                          # a counter, not a setting
        dev.record_names(True)                                                      # "record_hits" is 0
        with pytest.raises(ValueError, match="\"record_names\" is 1 and \"record_hits\" is 0"):
            _map(dev, comp)
        dev.record_names(False)
        dev.record_hits(True, windows=True)
        dev.record_keep(True)                                                       # the message of before the names, word for word
        with pytest.raises(ValueError, match="QNAME is not carried"):
            _map(dev, comp)
        for names in (False, True):                                                 # SAM text: refused on every route, names or not
            dev.record_names(names)
            for call in (lambda: dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=K),
                         lambda: dev.map_bgzf(sam_bgzf, fmt=_lib.FORMAT_SAM, k=K, first=True, last=True)):
                with pytest.raises(ValueError, match="QNAME is not carried"):
                    call()
        dev.set_param("min_base_quality", 20)                                       # a quality floor in the hits mode stays refused
        with pytest.raises(ValueError, match="applies no quality floor"):
            _map(dev, comp)
        dev.set_param("min_base_quality", 0)
        assert pending(dev) == (0, 0, 0)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        _names_on(dev, case)                                                        # the handle serves the next call
        _map(dev, comp)
        _check_take(dev, case)


def test_a_malformed_record_leaves_the_queue_as_it_was_and_reset_zeroes_the_counter(kmm, index):
    """A stream in two windows: the first maps (its kept records are pending), the second holds a record whose name has lost its
    NUL — KMM_ERR_MALFORMED, nothing of that call appended; then kmm_reset_counts: queues empty, the counter zero."""
    from kmer_mapper_amd import reads_io
    case = _case("names__default")
    base = case.base
    _, recs, hdr = bc.read_bam(base.payload)
    bad = bytearray(base.payload)
    victim = recs[len(recs) - 3]
    bad[victim.start + 36 + len(victim.name)] = 1
    cut = recs[len(recs) // 2].start                                               # members end at a record start: the first window is whole
    comp_1 = reads_io.bgzf_members(bytes(bad[:hdr])) + reads_io.bgzf_members(bytes(bad[hdr:cut]))
    comp_2 = reads_io.bgzf_members(bytes(bad[cut:])) + reads_io.BGZF_EOF
    comp = np.frombuffer(comp_1 + comp_2, dtype=np.uint8)
    with _open(kmm, index) as dev:
        _names_on(dev, case)
        used, n_1 = dev.map_bam(comp[:len(comp_1)], first=True, last=False, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n_1) == (len(comp_1), len(recs) // 2)
        state = (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"), dev.get_param("record_keep_pending_records"))
        assert state[0] == n_1 and state[1] > 0
        with pytest.raises(ValueError, match="does not fit its block_size"):
            dev.map_bam(comp[len(comp_1):], first=False, last=True, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                dev.get_param("record_keep_pending_records")) == state
        got, n = dev.take_kept_records()
        keep = bc.expected(case)[2][:n_1]
        _same_text(got, b"".join(t for t, kp in zip(bc.decoded(base).texts[:n_1], keep) if kp))
        assert n == int(keep.sum())
        assert dev.get_param("record_name_bytes_replaced") > 0
        _map(dev, _file(base))
        dev.reset()
        assert dev.get_param("record_name_bytes_replaced") == 0 and dev.get_param("record_keep_pending_bytes") == 0
        assert dev.get_param("record_hits_pending") == 0
        _map(dev, _file(base))                                                      # and the handle goes on
        _check_take(dev, case)
        _check_counters(dev, base)
        dev.get_stats(reset=True)                                                   # ... and it is zeroed with the other statistics
        assert dev.get_param("record_name_bytes_replaced") == 0 and dev.get_param("records_reversed") == 0


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm, index):
    from kmer_mapper_amd import mapper
    try:
        for name in ("strand_read_orientation__default", "mates_suffix__default", "lengths__permille_200", "selection_flags_only__default"):
            case = _case(name)
            base = case.base
            text, _, _, want_h, want_w = bc.expected(case)
            got, hits, windows = mapper.select_records(index, bc.bam_file(base), fmt="bam", k=K, max_index_lookup_frequency=rc.NO_FILTER,
                                                       exclude_flags=base.sel.excl, original_strand=base.orig, mate_suffix=base.suffix,
                                                       **_rule(case))
            assert got == text and np.array_equal(hits, want_h) and np.array_equal(windows, want_w)
        assert len(mapper._CACHE) == 1
        dev = next(iter(mapper._CACHE.values()))[0]                                 # the cached handle is left as it was found
        assert [dev.get_param(name) for name in ("record_names", "record_names_mate_suffix", "record_hits", "record_keep",
                                                 "bam_exclude_flags", "original_strand")] == [0] * 6
        with pytest.raises(ValueError, match="QNAME is not carried"):
            mapper.select_records(index, b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n", fmt="sam", k=2)
        with pytest.raises(ValueError, match="go with fmt=\"bam\""):
            mapper.select_records(index, b"@a\nACGT\n+\nIIII\n", fmt="fastq", k=2, mate_suffix=True)
    finally:
        mapper.clear_cache()


CLI = {"regions": (["--regions", "chr1:1001-2000", "--exclude-flags", "0x400", "--include-flags", "1", "--min-mapq", "20"],
                   lambda b: b["selection"]._replace(name="cli_regions", orig=True)),
       "regions_alone": (["--regions", "chr1:1001-2000"],
                         lambda b: b["selection"]._replace(name="cli_regions_alone", orig=True, sel=sc.NO_SEL._replace(regions=[(0, 1000, 2000)]))),
       "read_orientation": ([], lambda b: b["strand_read_orientation"]),
       "as_stored": (["--as-stored"], lambda b: b["strand_as_stored"]),
       "mate_suffix": (["--mate-suffix"], lambda b: b["mates_suffix"]._replace(name="cli_mates", orig=True)),
       "names_invert": (["--invert"], lambda b: b["names"]._replace(name="cli_names", orig=True))}


@pytest.mark.parametrize("kind", list(CLI))
def test_command_line_end_to_end(kmm, index, tmp_path, kind):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    options, pick = CLI[kind]
    base = pick(bc.bases())
    case = bc.BCase("cli_" + kind, base, 2, 0, "--invert" in options)
    text, n_kept, keep, hits, windows = bc.expected(case)
    assert 0 < n_kept < len(keep)
    path, npz = str(tmp_path / "reads.bam"), str(tmp_path / "index.npz")
    data = bc.bam_file(base, block=1999)
    open(path, "wb").write(data)
    index.to_file(npz)
    out, hits_out = str(tmp_path / "kept.fq"), str(tmp_path / "hits")
    seen, kept = run_argument_parser(["select-reads", "-i", npz, "-f", path, "--bam-to-fastq", "-k", str(K), "-c", "3000", "-I", str(rc.NO_FILTER),
                                      "--min-hits", "2", "-o", out, "--hits-output", hits_out] + options)
    assert (seen, kept) == (len(keep), n_kept)
    assert open(out, "rb").read() == text
    assert np.array_equal(np.load(hits_out + ".npy"), hits) and np.array_equal(np.load(hits_out + ".windows.npy"), windows)
    assert open(path, "rb").read() == data
