"""GPU tests of the record-keep mode (include/kmm.h): every case of tests/record_keep_cases.py against the
catalogue's model (held to a second route by tests/test_record_keep_on_the_cpu.py) under the six index layouts of the
record-hits tests, from host and from device bytes; calls without a take between them, queue growth, pieces; the stream routes
and multi-line FASTA; the mode's purity; the refusals; failing calls; the façade and the command line."""
import ctypes
import gzip

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests import record_keep_cases as rk
from tests.test_gpu_read_hits import LAYOUTS

pytestmark = pytest.mark.gpu

CASES = rk.all_cases()
IDS = [c.name for c in CASES]
K = 31


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _open(kmm, index, monkeypatch, layout="default"):
    env, wide, occ = LAYOUTS[layout]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    dev = kmm.DeviceIndex.from_index(index, index.max_node_id())
    assert (dev.get_param("wide_buckets"), dev.get_param("occupancy_filter")) == (wide, occ)
    return dev


def _kfmt(base):
    from kmer_mapper_amd import _lib
    return _lib.FORMAT_FASTQ if base.fmt == rh.FASTQ else _lib.FORMAT_FASTA2


def _map(dev, base, raw=None, lut="base", **kw):
    return dev.map_records(base.text if raw is None else raw, fmt=_kfmt(base), k=base.k, max_index_lookup_frequency=base.max_freq,
                           also_revcomp=base.revcomp, lut=base.lut if isinstance(lut, str) else lut, **kw)


def _rule(case):
    return dict(min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)


def _keep_on(dev, case):
    dev.record_hits(True, windows=True)
    dev.record_keep(True, **_rule(case))


def _same_text(got, want):
    assert got.dtype == np.uint8 and got.shape == (len(want),), (got.shape, len(want))
    if got.tobytes() != want:
        at = next(i for i, (a, b) in enumerate(zip(got.tobytes(), want)) if a != b)
        raise AssertionError("first difference at byte %d of %d" % (at, len(want)))


def _check_take(dev, case, times=1):
    """Both queues against the model: the bytes, the record count, the entries, and the rule over the entries."""
    text, n_kept, keep, want_h, want_w, _, n_records = rk.expected(case)
    assert dev.get_param("record_keep_pending_bytes") == times * len(text)
    assert dev.get_param("record_keep_pending_records") == times * n_kept
    got, n = dev.take_kept_records()
    _same_text(got, text * times)
    assert n == times * n_kept
    hits, windows = dev.take_record_hits()
    assert np.array_equal(hits, np.tile(want_h, times)) and np.array_equal(windows, np.tile(want_w, times))
    marks = rk.keep_rule(hits, windows, **_rule(case))
    assert np.array_equal(marks, np.tile(keep, times)) and int(marks.sum()) == n
    assert dev.get_param("record_keep_pending_bytes") == 0 and dev.get_param("record_keep_pending_records") == 0


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model(kmm, monkeypatch, case, layout):
    import torch
    base = case.base
    consumed, n_records = rk.expected(case)[5:7]
    with _open(kmm, base.index, monkeypatch, layout) as dev:
        _keep_on(dev, case)
        assert dev.get_param("record_keep") == 1 and dev.get_param("record_keep_min_hits") == case.min_hits
        assert _map(dev, base) == (consumed, n_records)                            # host bytes
        _check_take(dev, case)
        d_text = torch.from_numpy(base.text).cuda()                                # device bytes
        d_lut = None if base.lut is None else torch.from_numpy(base.lut).cuda()
        assert _map(dev, base, d_text, lut=d_lut) == (consumed, n_records)
        _check_take(dev, case)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)


def _case(name):
    return next(c for c in CASES if c.name == name)


QUEUE_CASES = ["rk_output_residues_fasta_k31__default", "rk_tile_ends_fastq_k31__default", "crlf_fastq_k31__default",
               "rk_single_short_record_k1__invert", "short_and_empty_fastq_k16__invert"]


@pytest.mark.parametrize("name", QUEUE_CASES)
def test_calls_without_a_take_between_them_and_a_device_buffer(kmm, monkeypatch, name):
    """Three calls on one handle: the second and third pieces start at a queue tail that is no multiple of 16; the output is
    the concatenation.  Then the take into a device buffer, and into one that is too short."""
    import torch
    from kmer_mapper_amd import _lib
    case = _case(name)
    text, n_kept = rk.expected(case)[:2]
    assert len(text) % 16 != 0
    with _open(kmm, case.base.index, monkeypatch) as dev:
        _keep_on(dev, case)
        for _ in range(3):
            _map(dev, case.base)
        _check_take(dev, case, times=3)
        _map(dev, case.base)
        _map(dev, case.base)
        short = torch.zeros(2 * len(text) - 1, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="%d bytes of %d records are pending" % (2 * len(text), 2 * n_kept)):
            dev.take_kept_records(out=short)
        assert not short.any()                                                     # nothing taken, the queue as it was
        assert dev.get_param("record_keep_pending_bytes") == 2 * len(text) and dev.get_param("record_keep_pending_records") == 2 * n_kept
        out = torch.full((2 * len(text) + 7,), 0xEE, dtype=torch.uint8, device="cuda")
        assert dev.take_kept_records(out=out) == (2 * len(text), 2 * n_kept)
        got = out.cpu().numpy()
        assert got[:2 * len(text)].tobytes() == text * 2 and (got[2 * len(text):] == 0xEE).all()
        assert dev.take_record_hits()[0].shape == (2 * rk.expected(case)[6],)
        # an empty queue: NULL and capacity 0 is KMM_OK with zeros
        nb, nr = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert _lib.lib().kmm_take_kept_records(dev._h, None, 0, ctypes.byref(nb), ctypes.byref(nr)) == _lib.KMM_OK
        assert (nb.value, nr.value) == (0, 0)


def test_the_queue_grows_with_bytes_pending(kmm, monkeypatch):
    """The first calls fit the queue's first allocation (1 MiB), the 1 MiB text does not: the pending bytes move to the new one."""
    small, big = _case("rk_tile_ends_fastq_k31__invert"), _case("super_tile_fastq_k31__invert")
    all_big = _case("super_tile_fastq_k31__default")
    with _open(kmm, small.base.index, monkeypatch) as dev:
        _keep_on(dev, small)
        _map(dev, small.base)
        _map(dev, small.base)
        dev.record_keep(True, **_rule(all_big))                                     # (the rule changes with bytes pending: they stay)
        _map(dev, big.base)
        _map(dev, big.base)
        want = rk.expected(small)[0] * 2 + rk.expected(all_big)[0] * 2
        assert len(want) > 2 << 20
        got, n = dev.take_kept_records()
        _same_text(got, want)
        assert n == 2 * rk.expected(small)[1] + 2 * rk.expected(all_big)[1]
        dev.record_keep(False)                                                      # off with nothing pending; entries still go to the hits queue
        _map(dev, small.base)
        assert dev.get_param("record_keep_pending_bytes") == 0


def _longest_record(base):
    ends = np.nonzero(base.text == 10)[0][rh.PERIOD[base.fmt] - 1::rh.PERIOD[base.fmt]] + 1
    return int(np.diff(np.concatenate([[0], ends])).max())


PIECE_CASES = [c for c in CASES if c.name.endswith(("__invert", "__default")) and 2048 < c.base.text.shape[0] < 100_000]


@pytest.mark.parametrize("case", PIECE_CASES, ids=[c.name for c in PIECE_CASES])
def test_pieces_and_two_calls_keep_file_order(kmm, monkeypatch, case):
    base = case.base
    consumed, n_records = rk.expected(case)[5:7]
    piece_kb = 1 if _longest_record(base) < 1024 else 4
    with _open(kmm, base.index, monkeypatch) as dev:
        _keep_on(dev, case)
        dev.set_param("debug_records_piece_kb", piece_kb)
        assert _map(dev, base) == (consumed, n_records)
        _check_take(dev, case)
        dev.set_param("debug_records_piece_kb", 0)
        first_end = int(np.nonzero(base.text == 10)[0][rh.PERIOD[base.fmt] - 1]) + 1
        cut = max(base.text.shape[0] * 2 // 5, first_end + 3)                       # inside a record behind the first
        used_1, n_1 = _map(dev, base, base.text[:cut].copy())
        used_2, n_2 = _map(dev, base, base.text[used_1:].copy())
        assert 0 < used_1 <= cut and (used_1 + used_2, n_1 + n_2) == (consumed, n_records)
        _check_take(dev, case)


# ---------------------------------------------------------------------------------------------- the routes
def _route_reads():
    reads = [rc.gslice(150 * i, 150).tobytes() for i in range(40)] + [r.tobytes() for r in rc.trio(K)] + [rc.gslice(77, 1300).tobytes()]
    reads[5] = reads[5][:20]
    for i in range(1, len(reads), 3):
        reads[i] = b"T" * (80 + i)
    return reads


def _want(index, reads, fmt, rule, text=None):
    bases, offsets = rh.reads_arrays(reads)
    hits, windows = rc.model(rc.index_arrays(index), bases, offsets, K, rc.NO_FILTER, False, None)
    keep = rk.keep_rule(hits, windows, **rule)
    text = rh.text_of(fmt, reads) if text is None else text
    spans = rk.record_spans(text, fmt)
    assert len(spans) == len(reads) and 0 < keep.sum() < len(reads)
    return b"".join(text[a:b] for (a, b), kp in zip(spans, keep) if kp), int(keep.sum()), hits, windows


def test_bgzf_fastq_with_a_record_carried_across_calls(kmm, monkeypatch):
    from kmer_mapper_amd import _lib, reads_io
    index = rc.genome_index(K)
    reads = _route_reads()
    text = rh.text_of(rh.FASTQ, reads)[:-1]                                         # (the final newline comes with LAST_CHUNK)
    comp = np.frombuffer(reads_io.bgzf_members(text, block=997) + reads_io.BGZF_EOF, dtype=np.uint8)
    for rule in (dict(min_hits=1), dict(min_hits=1, invert=True)):
        want, n_kept, want_h, want_w = _want(index, reads, rh.FASTQ, rule)
        with _open(kmm, index, monkeypatch) as dev:
            dev.record_hits(True, windows=True)
            dev.record_keep(True, **rule)
            cut = comp.shape[0] * 2 // 5
            used_1, n_1 = dev.map_bgzf(comp[:cut], fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, first=True)
            assert 0 < used_1 <= cut and 0 < n_1 < len(reads)
            used_2, n_2 = dev.map_bgzf(comp[used_1:], fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, last=True)
            assert used_1 + used_2 == comp.shape[0] and n_1 + n_2 == len(reads)
            got, n = dev.take_kept_records()
            _same_text(got, want)
            assert n == n_kept
            hits, windows = dev.take_record_hits()
            assert np.array_equal(hits, want_h) and np.array_equal(windows, want_w)
            assert not dev.get_node_counts().any()
            # record-hits mode alone cuts the same stream at the same places
            dev.record_keep(False)
            assert dev.map_bgzf(comp[:cut], fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, first=True) == (used_1, n_1)
            assert dev.map_bgzf(comp[used_1:], fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, last=True) == (used_2, n_2)
            assert np.array_equal(dev.take_record_hits()[0], want_h) and dev.get_param("record_keep_pending_bytes") == 0


def test_plain_gzip(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    index = rc.genome_index(K)
    reads = _route_reads()
    comp = np.frombuffer(gzip.compress(rh.text_of(rh.FASTQ, reads), 6), dtype=np.uint8)
    want, n_kept, want_h, want_w = _want(index, reads, rh.FASTQ, dict(min_hits=1))
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        used, n = dev.map_gzip(comp, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, first=True, last=True)
        assert (used, n) == (comp.shape[0], len(reads))
        got, n = dev.take_kept_records()
        _same_text(got, want)
        assert n == n_kept
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, want_h) and np.array_equal(windows, want_w)


def test_multi_line_fasta_comes_out_unwrapped(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    index = rc.genome_index(K)
    reads = [r for r in _route_reads() if r]
    wrapped = b"".join(b">r%d\n" % i + b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads))
    unwrapped = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(reads))
    want, n_kept, want_h, want_w = _want(index, reads, rh.FASTA, dict(min_hits=1), text=unwrapped)
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        raw = np.frombuffer(wrapped, dtype=np.uint8)
        used, n = dev.map_records(raw, fmt=_lib.FORMAT_FASTA | _lib.FORMAT_LAST_CHUNK, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n) == (len(wrapped), len(reads))
        got, n = dev.take_kept_records()
        _same_text(got, want)
        assert n == n_kept
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, want_h) and np.array_equal(windows, want_w)


# ---------------------------------------------------------------------------------------------- purity
def test_purity_against_record_hits_mode_and_a_fresh_handle(kmm, monkeypatch, oracle):
    case = _case("seams_fastq_k31__default")
    base = case.base
    want_h, want_w = rk.expected(case)[3:5]
    reads = rh.parse(base.text, base.fmt)[0]
    bases, offsets = rh.reads_arrays(reads)
    want_counts = oracle.map_reads(base.index, base.index.max_node_id(), bases, offsets, base.k, n_threads=4)[0]
    with _open(kmm, base.index, monkeypatch) as dev, _open(kmm, base.index, monkeypatch) as fresh:
        dev.count_kmers_mode()
        fresh.count_kmers_mode()
        _map(dev, base)
        _map(fresh, base)
        counts, kmer_counts, stats = dev.get_node_counts().copy(), dev.get_kmer_counts().copy(), dev.get_stats()
        assert np.array_equal(counts, want_counts) and counts.any()
        _keep_on(dev, case)
        _map(dev, base)
        assert np.array_equal(dev.get_node_counts(), counts) and np.array_equal(dev.get_kmer_counts(), kmer_counts)
        assert dev.get_stats() == stats
        _check_take(dev, case)
        # record_keep 0: the record-hits results, and nothing in the byte queue
        dev.record_keep(False)
        _map(dev, base)
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, want_h) and np.array_equal(windows, want_w)
        assert dev.get_param("record_keep_pending_bytes") == 0
        # every mode off: the counts of a handle that never had one
        dev.record_hits(False)
        _map(dev, base)
        _map(fresh, base)
        assert np.array_equal(dev.get_node_counts(), fresh.get_node_counts()) and np.array_equal(dev.get_node_counts(), 2 * want_counts)
        assert np.array_equal(dev.get_kmer_counts(), fresh.get_kmer_counts()) and dev.get_stats() == fresh.get_stats()


# ---------------------------------------------------------------------------------------------- refusals, failing calls
def _batch(reads):
    from kmer_mapper_amd.util import ReadBatch
    bases, offsets = rh.reads_arrays(reads)
    return ReadBatch(bases, offsets)


def test_refusals_map_nothing_and_append_nothing(kmm, monkeypatch):
    from kmer_mapper_amd import _lib, reads_io
    case = _case("seams_fastq_k31__default")
    base = case.base
    reads = rh.parse(base.text, base.fmt)[0]
    pending = lambda dev: (dev.get_param("record_hits_pending"), dev.get_param("record_keep_pending_bytes"),
                           dev.get_param("record_keep_pending_records"))
    with _open(kmm, base.index, monkeypatch) as dev:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="record_keep takes 0 or 1"):
                dev.set_param("record_keep", bad)
        with pytest.raises(ValueError, match="record_keep_min_permille outside"):
            dev.set_param("record_keep_min_permille", 1001)
        with pytest.raises(ValueError, match="record_keep_min_hits outside"):
            dev.set_param("record_keep_min_hits", 1 << 32)
        with pytest.raises(ValueError, match="read-only"):
            dev.set_param("record_keep_pending_bytes", 0)
        dev.set_param("record_keep_min_hits", (1 << 32) - 1)
        assert dev.get_param("record_keep_min_hits") == (1 << 32) - 1
        dev.record_keep(True)                                                       # record_hits is 0
        comp = np.frombuffer(reads_io.bgzf_members(base.text.tobytes()) + reads_io.BGZF_EOF, dtype=np.uint8)
        gz = np.frombuffer(gzip.compress(base.text.tobytes(), 1), dtype=np.uint8)
        calls = (lambda: _map(dev, base),
                 lambda: dev.map_bgzf(comp, fmt=_lib.FORMAT_FASTQ, k=base.k, first=True, last=True),
                 lambda: dev.map_gzip(gz, fmt=_lib.FORMAT_FASTQ, k=base.k, first=True, last=True))
        for call in calls:
            with pytest.raises(ValueError, match="\"record_hits\" is 0"):
                call()
        dev.record_hits(True)                                                       # mode 1 and a permille threshold
        dev.record_keep(True, min_permille=10)
        for call in calls:
            with pytest.raises(ValueError, match="needs the windows"):
                call()
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        sam = np.frombuffer(reads_io.sam_text(_batch(reads[:5])), dtype=np.uint8)
        sam_bgzf = np.frombuffer(reads_io.bgzf_members(sam.tobytes()) + reads_io.BGZF_EOF, dtype=np.uint8)
        sam_gz = np.frombuffer(gzip.compress(sam.tobytes(), 1), dtype=np.uint8)
        bam = np.frombuffer(reads_io.bgzf_members(reads_io.bam_header((), b"@HD\tVN:1.6\tSO:unsorted\n")) +
                            reads_io.bgzf_members(reads_io.bam_records(_batch(reads[:5]))) + reads_io.BGZF_EOF, dtype=np.uint8)
        for call in (lambda: dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=base.k),
                     lambda: dev.map_bgzf(sam_bgzf, fmt=_lib.FORMAT_SAM, k=base.k, first=True, last=True),
                     lambda: dev.map_gzip(sam_gz, fmt=_lib.FORMAT_SAM, k=base.k, first=True, last=True),
                     lambda: dev.map_bam(bam, first=True, last=True, k=base.k)):
            with pytest.raises(ValueError, match="QNAME is not carried"):
                call()
        dev.set_param("min_base_quality", 20)                                       # what record-hits mode refuses stays refused
        with pytest.raises(ValueError, match="applies no quality floor"):
            _map(dev, base)
        dev.set_param("min_base_quality", 0)
        bases, offsets = rh.reads_arrays(reads)
        with pytest.raises(ValueError, match="record_hits"):
            dev.map_reads(bases, offsets, base.k)
        assert pending(dev) == (0, 0, 0)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        _map(dev, base)                                                             # the handle serves the next call
        _check_take(dev, case)
        dev.record_keep(False)                                                      # with the switch off SAM is served again
        assert dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=base.k)[1] == 5


def test_a_malformed_call_appends_nothing_and_reset_empties_the_queue(kmm, monkeypatch):
    """Multi-line FASTA in pieces of 1 KiB whose third piece holds a '\\r' without '\\n' (the input the multi-line tests use):
    KMM_ERR_MALFORMED, and the bytes the first pieces appended are put back — the queue holds what it held before the call."""
    from kmer_mapper_amd import _lib
    case = _case("rk_tile_ends_fastq_k31__default")
    index = case.base.index
    text, n_kept = rk.expected(case)[:2]
    reads = [rc.gslice(200 * i, 150).tobytes() for i in range(30)]
    wrapped = bytearray(b"".join(b">r%d\n" % i + b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads)))
    good = np.frombuffer(bytes(wrapped), dtype=np.uint8)
    at = wrapped.index(b"\n", 2500) - 20                                            # inside a sequence line of the third piece
    assert wrapped[at:at + 1] != b"\n" and wrapped[wrapped.rfind(b"\n", 0, at) + 1:][:1] != b">" and 2048 < at < 3072
    wrapped[at:at + 1] = b"\r"
    bad = np.frombuffer(bytes(wrapped), dtype=np.uint8)
    fmt = _lib.FORMAT_FASTA | _lib.FORMAT_LAST_CHUNK
    with _open(kmm, index, monkeypatch) as dev:
        _keep_on(dev, case)
        _map(dev, case.base)
        dev.set_param("debug_records_piece_kb", 1)
        with pytest.raises(ValueError, match="is not followed by"):
            dev.map_records(bad, fmt=fmt, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        dev.set_param("debug_records_piece_kb", 0)
        assert dev.get_param("record_hits_pending") == rk.expected(case)[6]
        _check_take(dev, case)                                                      # exactly what the first call appended
        used, n = dev.map_records(good, fmt=fmt, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n) == (good.shape[0], len(reads))
        assert dev.get_param("record_keep_pending_records") == n and dev.get_param("record_keep_pending_bytes") > 0
        dev.reset()                                                                 # kmm_reset_counts empties both queues
        assert dev.get_param("record_keep_pending_bytes") == 0 and dev.get_param("record_keep_pending_records") == 0
        got, n = dev.take_kept_records()
        assert got.shape == (0,) and n == 0 and dev.get_param("record_hits_pending") == 0
        _map(dev, case.base)
        _check_take(dev, case)


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    case = _case("rk_permille_fastq_k31__permille_200")
    text, _, _, want_h, want_w = rk.expected(case)[:5]
    try:
        got, hits, windows = mapper.select_records(case.base.index, case.base.text, fmt="fastq", k=case.base.k,
                                                   max_index_lookup_frequency=case.base.max_freq, min_permille=200)
        assert got == text and np.array_equal(hits, want_h) and np.array_equal(windows, want_w)
        got, hits, windows = mapper.select_records(case.base.index, b">a\nACGT\n>b\n", fmt="fasta", k=2, min_hits=0)
        assert got == b">a\nACGT\n" and hits.shape == (1,) and len(mapper._CACHE) == 1
        with pytest.raises(ValueError, match="QNAME is not carried"):
            mapper.select_records(case.base.index, b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*\n", fmt="sam", k=2)
    finally:
        mapper.clear_cache()


@pytest.mark.parametrize("kind", ["fq", "fq_bgzf", "fq_gz"])
def test_command_line_end_to_end(kmm, tmp_path, kind):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    index = rc.genome_index(K)
    reads = _route_reads() * 3
    text = rh.text_of(rh.FASTQ, reads)
    path = str(tmp_path / ("reads.fq" if kind == "fq" else "reads.fq.gz"))
    data = {"fq": text, "fq_bgzf": reads_io.bgzf_members(text, block=4001) + reads_io.BGZF_EOF, "fq_gz": gzip.compress(text, 6)}[kind]
    open(path, "wb").write(data)
    npz = str(tmp_path / "index.npz")
    index.to_file(npz)
    bases, offsets = rh.reads_arrays(reads)
    hits, windows = rc.model(rc.index_arrays(index), bases, offsets, K, rc.NO_FILTER, False, None)
    spans = rk.record_spans(text, rh.FASTQ)
    common = ["select-reads", "-i", npz, "-f", path, "-k", "31", "-c", "1500", "-I", str(rc.NO_FILTER), "--min-hits", "3"]
    for flags, invert in (([], False), (["--invert"], True)):
        keep = rk.keep_rule(hits, windows, 3, 0, invert)
        assert 0 < keep.sum() < len(reads)
        out, hits_out = str(tmp_path / ("kept%d.fq" % invert)), str(tmp_path / ("hits%d" % invert))
        seen, kept = run_argument_parser(common + ["-o", out, "--hits-output", hits_out] + flags)
        assert (seen, kept) == (len(reads), int(keep.sum()))
        assert open(out, "rb").read() == b"".join(text[a:b] for (a, b), kp in zip(spans, keep) if kp)
        assert np.array_equal(np.load(hits_out + ".npy"), hits) and np.array_equal(np.load(hits_out + ".windows.npy"), windows)
    assert open(path, "rb").read() == data
