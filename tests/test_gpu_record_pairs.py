"""GPU tests of keeping mates together (include/kmm.h KEEPING MATES TOGETHER): every case of
tests/record_pairs_cases.py against the catalogue's model (held to the oracle by tests/test_record_pairs_on_the_cpu.py) under
the six index layouts of the record-keep tests, from host and from device bytes — interleaved text through "record_pairs",
two texts through kmm_map_record_pairs; the equivalence of the two forms; calls without a take between them; pieces; odd
record counts on the stream routes; the mode's purity; the refusals; the façade and the command line."""
import ctypes
import gzip

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests import record_pairs_cases as rp
from tests.test_gpu_read_hits import LAYOUTS

pytestmark = pytest.mark.gpu

CASES = rp.all_cases()
IDS = [c.name for c in CASES]
TWO = [c for c in CASES if c.text2 is not None]
K = rp.K


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


def _kfmt(fmt):
    from kmer_mapper_amd import _lib
    return _lib.FORMAT_FASTQ if fmt == rh.FASTQ else _lib.FORMAT_FASTA2


def _keep_on(dev, case, interleaved=None):
    dev.record_hits(True, windows=True)
    dev.record_keep(True, min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert)
    dev.record_pairs(case.text2 is None if interleaved is None else interleaved, rule=case.pair_rule)


def _on(where, a):
    import torch
    return a if where == "host" or a is None else torch.from_numpy(a).cuda()


def _map(dev, case, where=("host", "host")):
    """The case's call: (consumed1, consumed2, n_pairs)."""
    common = dict(fmt=_kfmt(case.fmt), k=case.k, max_index_lookup_frequency=rc.NO_FILTER, lut=_on(where[0], case.lut))
    if case.text2 is None:
        consumed, n_records = dev.map_records(_on(where[0], case.text1), **common)
        assert n_records % 2 == 0
        return consumed, 0, n_records // 2
    return dev.map_record_pairs(_on(where[0], case.text1), _on(where[1], case.text2), **common)


def _same_text(got, want):
    assert got.dtype == np.uint8 and got.shape == (len(want),), (got.shape, len(want))
    if got.tobytes() != want:
        at = next(i for i, (a, b) in enumerate(zip(got.tobytes(), want)) if a != b)
        raise AssertionError("first difference at byte %d of %d" % (at, len(want)))


def _pending(dev):
    return tuple(dev.get_param(name) for name in ("record_hits_pending", "record_keep_pending_bytes", "record_keep_pending_records",
                                                  "record_keep_pending_bytes_mate2", "record_keep_pending_records_mate2"))


def _check_take(dev, case, times=1):
    """The three queues against the model: the bytes, the record counts, the entries, and the pair rule over the entries."""
    e = rp.expected(case)
    per_queue = e.n_kept * (2 if case.text2 is None else 1)
    want2 = b"" if e.text2 is None else e.text2
    assert _pending(dev) == (2 * e.n_pairs * times, len(e.text1) * times, per_queue * times, len(want2) * times,
                             (0 if e.text2 is None else per_queue) * times)
    got, n = dev.take_kept_mates(0) if case.text2 is not None else dev.take_kept_records()
    _same_text(got, e.text1 * times)
    assert n == per_queue * times
    got2, n2 = dev.take_kept_mates(1)
    _same_text(got2, want2 * times)
    assert n2 == (0 if e.text2 is None else n)
    hits, windows = dev.take_record_hits() if e.n_pairs else (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    assert np.array_equal(hits, np.tile(e.hits, times)) and np.array_equal(windows, np.tile(e.windows, times))
    marks = rp.pair_keep_entries(hits, windows, **rp.rule_of(case))
    assert np.array_equal(marks, np.tile(e.keep, times)) and int(marks.sum()) * (2 if case.text2 is None else 1) == n
    assert _pending(dev) == (0, 0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model(kmm, monkeypatch, case, layout):
    e = rp.expected(case)
    want = (e.consumed1, e.consumed2, e.n_pairs)
    with _open(kmm, case.index, monkeypatch, layout) as dev:
        _keep_on(dev, case)
        assert dev.get_param("record_pairs") == int(case.text2 is None) and dev.get_param("record_pairs_rule") == int(case.pair_rule == rp.BOTH)
        for where in (("host", "host"), ("device", "device")) + ((("host", "device"), ("device", "host")) if case.text2 is not None else ()):
            assert _map(dev, case, where) == want, where
            _check_take(dev, case)
        if case.piece_kb:                                                          # the same in pieces: each ends behind a mate 2
            dev.set_param("debug_records_piece_kb", case.piece_kb)
            assert _map(dev, case) == want
            _check_take(dev, case)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)


@pytest.mark.parametrize("case", TWO, ids=[c.name for c in TWO])
def test_two_files_are_the_interleaved_file(kmm, monkeypatch, case):
    """Interleaving the two texts on the host and mapping with "record_pairs" 1 gives the same hits queue, and its kept text,
    de-interleaved by record, is the two queues of kmm_map_record_pairs."""
    both = np.frombuffer(rp.interleave(case.text1, case.text2, case.fmt), dtype=np.uint8)
    with _open(kmm, case.index, monkeypatch) as dev:
        _keep_on(dev, case)
        _, _, m = _map(dev, case)
        two = (dev.take_kept_mates(0), dev.take_kept_mates(1), dev.take_record_hits() if m else None)
        assert two[0][1] == two[1][1]
        _keep_on(dev, case, interleaved=True)
        consumed, n_records = dev.map_records(both, fmt=_kfmt(case.fmt), k=case.k, max_index_lookup_frequency=rc.NO_FILTER, lut=case.lut) \
            if both.shape[0] else (0, 0)
        assert (consumed, n_records) == (both.shape[0], 2 * m)
        text, n = dev.take_kept_records()
        one, other = rp.deinterleave(text.tobytes(), case.fmt)
        assert (one, other) == (two[0][0].tobytes(), two[1][0].tobytes()) and n == 2 * two[0][1]
        if m:
            hits, windows = dev.take_record_hits()
            assert np.array_equal(hits, two[2][0]) and np.array_equal(windows, two[2][1])


QUEUE_CASES = ["residues_fasta_interleaved__any", "residues_fasta_two_files__any", "patterns_fastq_two_files__both_invert",
               "seams_fastq_interleaved__both", "cut_at_tile_+1_two_files__any"]


@pytest.mark.parametrize("name", QUEUE_CASES)
def test_three_calls_without_a_take(kmm, monkeypatch, name):
    """The second and third calls start at queue tails — of both queues — that are no multiple of 16; then a take of the second
    queue into a device buffer, and into one that is too short."""
    import torch
    from kmer_mapper_amd import _lib
    case = rp.by_name(name)
    e = rp.expected(case)
    assert len(e.text1) % 16 != 0 and (e.text2 is None or len(e.text2) % 16 != 0)
    with _open(kmm, case.index, monkeypatch) as dev:
        _keep_on(dev, case)
        for _ in range(3):
            _map(dev, case)
        _check_take(dev, case, times=3)
        if e.text2 is None:
            return
        _map(dev, case)
        _map(dev, case)
        short = torch.zeros(2 * len(e.text2) - 1, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="%d bytes of %d records are pending" % (2 * len(e.text2), 2 * e.n_kept)):
            dev.take_kept_mates(1, out=short)
        assert not short.any() and dev.get_param("record_keep_pending_records_mate2") == 2 * e.n_kept
        out = torch.full((2 * len(e.text2) + 7,), 0xEE, dtype=torch.uint8, device="cuda")
        assert dev.take_kept_mates(1, out=out) == (2 * len(e.text2), 2 * e.n_kept)
        got = out.cpu().numpy()
        assert got[:2 * len(e.text2)].tobytes() == e.text2 * 2 and (got[2 * len(e.text2):] == 0xEE).all()
        assert dev.take_kept_mates(0)[1] == 2 * e.n_kept                          # (the other queue held as many records)
        nb, nr = ctypes.c_int64(-1), ctypes.c_int64(-1)
        for mate, rc_want in ((1, _lib.KMM_OK), (0, _lib.KMM_OK), (2, _lib.KMM_ERR_INVALID_ARG), (-1, _lib.KMM_ERR_INVALID_ARG)):
            assert _lib.lib().kmm_take_kept_mates(dev._h, mate, None, 0, ctypes.byref(nb), ctypes.byref(nr)) == rc_want
        dev.reset()                                                                # kmm_reset_counts empties all three
        assert _pending(dev) == (0, 0, 0, 0, 0)


def test_pairs_behind_an_odd_number_of_pending_entries(kmm, monkeypatch):
    """An unpaired call has left an odd number of entries pending (after a take of some of them, at an odd index of the queue's
    arrays too): the pairs of the two-file call behind them are still loaded as aligned 8-byte pairs — the pending ones move."""
    odd, two = rp.by_name("odd_fastq_interleaved__any"), rp.by_name("patterns_fastq_two_files__any")
    e = rp.expected(two)
    recs = rp.records(odd.text1, odd.fmt)
    bases, offsets = rh.reads_arrays([s for _, s in recs])
    one_h, one_w = rc.model(rc.index_arrays(odd.index), bases, offsets, K, rc.NO_FILTER, False, None)
    one_text = b"".join(r[0] for r, h in zip(recs, one_h.tolist()) if h >= 1)
    assert len(recs) % 2 == 1 and 0 < len(one_text) < odd.text1.shape[0]
    with _open(kmm, odd.index, monkeypatch) as dev:
        _keep_on(dev, two)                                                         # ("record_pairs" 0: every record by itself)
        for taken in (0, 2):
            assert dev.map_records(odd.text1, fmt=_kfmt(odd.fmt), k=K, max_index_lookup_frequency=rc.NO_FILTER) == (odd.text1.shape[0], len(recs))
            if taken:
                assert np.array_equal(dev.take_record_hits(capacity=taken)[0], one_h[:taken])
            _map(dev, two)
            hits, windows = dev.take_record_hits()
            assert np.array_equal(hits, np.concatenate([one_h[taken:], e.hits])) and np.array_equal(windows, np.concatenate([one_w[taken:], e.windows]))
            assert dev.take_kept_mates(0)[0].tobytes() == one_text + e.text1 and dev.take_kept_mates(1)[0].tobytes() == e.text2


# ---------------------------------------------------------------------------------------------- pieces, odd counts
@pytest.mark.parametrize("fmt", [rh.FASTQ, rh.FASTA])
def test_a_piece_limit_between_the_mates_cuts_in_front_of_mate_1(kmm, monkeypatch, fmt):
    """The first KiB of the text ends inside record 3, the mate 2 of pair 1: unpaired, three records are taken; with
    "record_pairs" 1 the call ends behind pair 0, n_records is even, and so for every later piece."""
    case = rp.by_name("pieces_%s_interleaved__any" % fmt)
    spans = np.cumsum([0] + [len(r[0]) for r in rp.records(case.text1, fmt)]).tolist()
    with _open(kmm, case.index, monkeypatch) as dev:
        _keep_on(dev, case)
        dev.record_pairs(False)
        assert dev.map_records(case.text1[:1024].copy(), fmt=_kfmt(fmt), k=K, max_index_lookup_frequency=rc.NO_FILTER) == (spans[3], 3)
        dev.reset()
        dev.record_pairs(True)
        start = 0
        while start < case.text1.shape[0]:
            piece = case.text1[start:start + 1024].copy()
            used, n = dev.map_records(piece, fmt=_kfmt(fmt), k=K, max_index_lookup_frequency=rc.NO_FILTER)
            whole = max(i for i in range(0, len(spans), 2) if spans[i] <= start + piece.shape[0])
            assert n % 2 == 0 and n > 0 and start + used == spans[whole]
            start += used
        assert start == case.text1.shape[0]
        _check_take(dev, case)                                                     # the single-piece output


def _stream(kind, text):
    from kmer_mapper_amd import reads_io
    if kind == "bgzf":
        return np.frombuffer(reads_io.bgzf_members(text, block=997) + reads_io.BGZF_EOF, dtype=np.uint8)
    return np.frombuffer(gzip.compress(text, 6), dtype=np.uint8)


@pytest.mark.parametrize("kind", ["bgzf", "gzip"])
def test_stream_routes_whole_pairs_and_an_unpaired_last_record(kmm, monkeypatch, kind):
    from kmer_mapper_amd import _lib
    whole, odd = rp.by_name("seams_fastq_interleaved__any"), rp.by_name("odd_fastq_interleaved__any")
    e, e_odd = rp.expected(whole), rp.expected(odd)
    call = lambda dev, comp, **kw: getattr(dev, "map_" + kind)(comp, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, **kw)
    with _open(kmm, whole.index, monkeypatch) as dev:
        _keep_on(dev, whole)
        comp = _stream(kind, whole.text1.tobytes())
        if kind == "bgzf":                                                         # two calls: a pair carried across them
            cut = comp.shape[0] * 2 // 5
            used_1, n_1 = call(dev, comp[:cut], first=True)
            used_2, n_2 = call(dev, comp[used_1:], last=True)
            assert n_1 % 2 == 0 and n_2 % 2 == 0 and 0 < n_1 and n_1 + n_2 == 2 * e.n_pairs and used_1 + used_2 == comp.shape[0]
        else:
            assert call(dev, comp, first=True, last=True) == (comp.shape[0], 2 * e.n_pairs)
        _check_take(dev, whole)
        # a stream that ends with an unpaired record: the last call fails and nothing of it stays in a queue
        _map(dev, whole)
        before = _pending(dev)
        with pytest.raises(ValueError, match="ends with an unpaired record"):
            call(dev, _stream(kind, odd.text1.tobytes()), first=True, last=True)
        assert _pending(dev) == before
        _check_take(dev, whole)
        # without the last-chunk flag the record is carried, and its mate may still come
        used, n = call(dev, _stream(kind, odd.text1.tobytes()), first=True)
        assert n == 2 * e_odd.n_pairs
        dev.reset()
        # plain text: the unpaired record stays unconsumed
        assert _map(dev, odd) == (e_odd.consumed1, 0, e_odd.n_pairs) and e_odd.consumed1 < odd.text1.shape[0]
        _check_take(dev, odd)


def test_two_files_in_pieces(kmm, monkeypatch):
    """Chunks beyond the piece limit are walked piece pair by piece pair: mates of 150 and 100 bases, pieces of 1 KiB."""
    case = rp.by_name("lengths_150_100_two_files__any")
    e = rp.expected(case)
    with _open(kmm, case.index, monkeypatch) as dev:
        _keep_on(dev, case)
        dev.set_param("debug_records_piece_kb", 1)
        assert _map(dev, case, ("host", "device")) == (e.consumed1, e.consumed2, e.n_pairs)
        _check_take(dev, case)
        # a record longer than the piece in one buffer: no pair in reach, nothing consumed, nothing appended
        long_one = np.frombuffer(rh.record(rh.FASTQ, rp.hit_read(1500, 0), b"long/1"), dtype=np.uint8)
        assert dev.map_record_pairs(long_one, case.text2, fmt=_kfmt(case.fmt), k=K) == (0, 0, 0)
        assert _pending(dev) == (0, 0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------- purity
def test_purity(kmm, monkeypatch, oracle):
    """"record_pairs" 1 with "record_keep" 0 changes nothing: the entries of the unpaired call (an odd count of them) and the
    node counts of a handle that never had the parameter; in pair mode the node counts and kmm_get_stats do not move."""
    case = rp.by_name("odd_fastq_interleaved__any")
    seqs = [s for _, s in rp.records(case.text1, case.fmt)]
    assert len(seqs) % 2 == 1
    bases, offsets = rh.reads_arrays(seqs)
    want_h, want_w = rc.model(rc.index_arrays(case.index), bases, offsets, K, rc.NO_FILTER, False, None)
    want_counts = oracle.map_reads(case.index, case.index.max_node_id(), bases, offsets, K, n_threads=4)[0]
    args = dict(fmt=_kfmt(case.fmt), k=K, max_index_lookup_frequency=rc.NO_FILTER)
    with _open(kmm, case.index, monkeypatch) as dev, _open(kmm, case.index, monkeypatch) as fresh:
        dev.record_pairs(True, rule="both")
        assert dev.map_records(case.text1, **args) == fresh.map_records(case.text1, **args) == (case.text1.shape[0], len(seqs))
        counts, stats = dev.get_node_counts().copy(), dev.get_stats()
        assert np.array_equal(counts, want_counts) and counts.any() and np.array_equal(counts, fresh.get_node_counts())
        assert stats == fresh.get_stats()
        dev.record_hits(True, windows=True)                                        # record-hits mode alone: every record, odd count
        assert dev.map_records(case.text1, **args) == (case.text1.shape[0], len(seqs))
        hits, windows = dev.take_record_hits()
        assert np.array_equal(hits, want_h) and np.array_equal(windows, want_w)
        assert _pending(dev) == (0, 0, 0, 0, 0)
        _keep_on(dev, case)                                                        # pair mode: counts and statistics stay
        _map(dev, case)
        _check_take(dev, case)
        two = rp.by_name("patterns_fastq_two_files__any")
        _keep_on(dev, two)
        _map(dev, two)
        assert np.array_equal(dev.get_node_counts(), counts) and dev.get_stats() == stats
        dev.reset()


# ---------------------------------------------------------------------------------------------- refusals
def _batch(reads):
    from kmer_mapper_amd.util import ReadBatch
    bases, offsets = rh.reads_arrays(reads)
    return ReadBatch(bases, offsets)


def test_refusals_map_nothing_and_append_nothing(kmm, monkeypatch):
    from kmer_mapper_amd import _lib, reads_io
    case = rp.by_name("patterns_fasta_interleaved__any")
    two = rp.by_name("patterns_fastq_two_files__any")
    reads = [s for _, s in rp.records(case.text1, case.fmt)]
    with _open(kmm, case.index, monkeypatch) as dev:
        for name in ("record_pairs", "record_pairs_rule"):
            for bad in (2, -1):
                with pytest.raises(ValueError, match=name + " takes 0"):
                    dev.set_param(name, bad)
        for name in ("record_keep_pending_bytes_mate2", "record_keep_pending_records_mate2"):
            with pytest.raises(ValueError, match="read-only"):
                dev.set_param(name, 0)
        with pytest.raises(ValueError, match="'any' or 'both'"):
            dev.record_pairs(True, rule="either")
        pairs_call = lambda fmt=_lib.FORMAT_FASTQ, **kw: dev.map_record_pairs(two.text1, two.text2, fmt=fmt, k=K, **kw)
        with pytest.raises(ValueError, match="\"record_hits\" is 0 and \"record_keep\" is 0"):      # the two-file call needs both modes
            pairs_call()
        dev.record_hits(True, windows=True)
        with pytest.raises(ValueError, match="\"record_hits\" is 2 and \"record_keep\" is 0"):
            pairs_call()
        dev.record_hits(True)
        dev.record_keep(True, min_permille=10)
        with pytest.raises(ValueError, match="needs the windows"):
            pairs_call()
        _keep_on(dev, case)
        for fmt in (_lib.FORMAT_FASTA, _lib.FORMAT_SAM, 0, _lib.FORMAT_FASTQ | _lib.FORMAT_LAST_CHUNK):
            with pytest.raises(ValueError, match="format must be KMM_FORMAT_FASTQ \\(4\\) or KMM_FORMAT_FASTA2"):
                pairs_call(fmt)
        with pytest.raises(ValueError, match="n1 or n2 negative"):
            dev.map_record_pairs(two.text1, two.text2, k=K, n_bytes2=-1)
        # "record_keep" and "record_pairs" both 1: multi-line FASTA, SAM and BAM — named or not — are refused
        wrapped = np.frombuffer(b"".join(b">r%d\n" % i + r[:30] + b"\n" + r[30:] + b"\n" for i, r in enumerate(reads)), dtype=np.uint8)
        with pytest.raises(ValueError, match="multi-line FASTA cuts at header lines"):
            dev.map_records(wrapped, fmt=_lib.FORMAT_FASTA | _lib.FORMAT_LAST_CHUNK, k=K)
        sam = np.frombuffer(reads_io.sam_text(_batch(reads[:4])), dtype=np.uint8)
        sam_bgzf = np.frombuffer(reads_io.bgzf_members(sam.tobytes()) + reads_io.BGZF_EOF, dtype=np.uint8)
        sam_gz = np.frombuffer(gzip.compress(sam.tobytes(), 1), dtype=np.uint8)
        bam = np.frombuffer(reads_io.bgzf_members(reads_io.bam_header((), b"@HD\tVN:1.6\tSO:unsorted\n")) +
                            reads_io.bgzf_members(reads_io.bam_records(_batch(reads[:4]))) + reads_io.BGZF_EOF, dtype=np.uint8)
        dev.record_names(True)
        for call in (lambda: dev.map_bam(bam, first=True, last=True, k=K),):
            with pytest.raises(ValueError, match="not pair-aligned ones"):
                call()
        dev.record_names(False)
        for call in (lambda: dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=K),
                     lambda: dev.map_bgzf(sam_bgzf, fmt=_lib.FORMAT_SAM, k=K, first=True, last=True),
                     lambda: dev.map_gzip(sam_gz, fmt=_lib.FORMAT_SAM, k=K, first=True, last=True),
                     lambda: dev.map_bam(bam, first=True, last=True, k=K)):
            with pytest.raises(ValueError, match="QNAME is not carried|not pair-aligned ones"):
                call()
        assert _pending(dev) == (0, 0, 0, 0, 0)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)
        # changing "record_pairs" with entries pending is refused, whichever way; the same value is no change
        _map(dev, case)
        with pytest.raises(ValueError, match="entries pending that were appended under record_pairs 1"):
            dev.set_param("record_pairs", 0)
        dev.set_param("record_pairs", 1)
        _check_take(dev, case)
        dev.set_param("record_pairs", 0)
        dev.map_records(case.text1, fmt=_kfmt(case.fmt), k=K, max_index_lookup_frequency=rc.NO_FILTER)
        with pytest.raises(ValueError, match="entries pending that were appended under record_pairs 0"):
            dev.record_pairs(True)
        dev.reset()
        _keep_on(dev, two)                                                         # the handle serves the next calls
        _map(dev, two)
        _check_take(dev, two)


def test_a_malformed_record_is_deferred_and_reset_empties_the_three_queues(kmm, monkeypatch):
    """A line of buffer 2 that does not start with '+' is found on the device, so the error is deferred and sticky as on every
    record call: the takes report it and take nothing; kmm_reset_counts clears the error and all three queues."""
    case = rp.by_name("patterns_fastq_two_files__any")
    bad = case.text2.copy()
    plus = int(np.nonzero(bad == ord("+"))[0][0])
    assert bad[plus - 1] == 10 and bad[plus + 1] == 10
    bad[plus] = ord("-")
    with _open(kmm, case.index, monkeypatch) as dev:
        _keep_on(dev, case)
        _map(dev, case)
        dev.map_record_pairs(case.text1, bad, fmt=_kfmt(case.fmt), k=K, max_index_lookup_frequency=rc.NO_FILTER)
        for take in (lambda: dev.take_kept_mates(1), lambda: dev.take_kept_mates(0), dev.take_record_hits):
            with pytest.raises(ValueError, match="record structure violated"):
                take()
        dev.reset()
        assert _pending(dev) == (0, 0, 0, 0, 0)
        _map(dev, case)
        _check_take(dev, case)


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    one, two = rp.by_name("permille_fastq_interleaved__150_both"), rp.by_name("permille_fastq_two_files__150_any_invert")
    try:
        e = rp.expected(one)
        got = mapper.select_record_pairs(one.index, one.text1, fmt="fastq", k=K, max_index_lookup_frequency=rc.NO_FILTER, min_permille=150,
                                         pair_rule="both")
        assert got[0] == e.text1 and got[1] is None and np.array_equal(got[2], e.hits) and np.array_equal(got[3], e.windows)
        e = rp.expected(two)
        got = mapper.select_record_pairs(two.index, two.text1.tobytes(), two.text2, fmt="fastq", k=K, max_index_lookup_frequency=rc.NO_FILTER,
                                         min_permille=150, invert=True)
        assert got[:2] == (e.text1, e.text2) and np.array_equal(got[2], e.hits) and np.array_equal(got[3], e.windows)
        dev = next(iter(mapper._CACHE.values()))[0]
        assert len(mapper._CACHE) == 1 and [dev.get_param(n) for n in ("record_pairs", "record_pairs_rule", "record_keep", "record_hits")] == [0] * 4
        # an unpaired record is not looked at; the handle as it was found
        got = mapper.select_record_pairs(one.index, b">a/1\nACGT\n>a/2\nCCGT\n>b/1\nACGT\n", fmt="fasta", k=2, min_hits=0)
        assert got[0] == b">a/1\nACGT\n>a/2\nCCGT\n" and got[2].shape == (2,)
        with pytest.raises(ValueError, match="'any' or 'both'"):
            mapper.select_record_pairs(one.index, one.text1, k=K, pair_rule="either")
        assert [dev.get_param(n) for n in ("record_pairs", "record_keep", "record_hits")] == [0] * 3
    finally:
        mapper.clear_cache()


def _cli_pairs():
    pairs = []
    for i in range(60):
        a = rc.gslice(150 * i, 150).tobytes() if i % 3 else b"T" * (100 + i)
        b = rc.gslice(150 * i + 40, 100).tobytes() if i % 4 < 2 else b"T" * (80 + i)
        pairs.append((a, b))
    pairs[7] = (pairs[7][0][:20], pairs[7][1])
    return pairs


def _names(text, fmt):
    return [r[0].split(b"\n")[0][1:].rsplit(b"/", 1)[0] for r in rp.records(text, fmt)]


@pytest.mark.parametrize("kind", ["plain", "bgzf", "gzip"])
def test_command_line_end_to_end(kmm, tmp_path, kind):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    index = rc.genome_index(K)
    pairs = _cli_pairs()
    both, (t1, t2) = rp.interleaved_text(rh.FASTQ, pairs), rp.two_texts(rh.FASTQ, pairs)
    pack = {"plain": lambda t: t, "bgzf": lambda t: reads_io.bgzf_members(t, block=4001) + reads_io.BGZF_EOF, "gzip": lambda t: gzip.compress(t, 6, mtime=0)}[kind]  # (mtime: the files are compared with a second pack() below)
    ext = ".fq" if kind == "plain" else ".fq.gz"
    paths = {name: str(tmp_path / (name + ext)) for name in ("both", "r1", "r2")}
    for name, text in (("both", both), ("r1", t1), ("r2", t2)):
        open(paths[name], "wb").write(pack(text))
    npz = str(tmp_path / "index.npz")
    index.to_file(npz)
    bases, offsets = rh.reads_arrays([s for pair in pairs for s in pair])
    hits, windows = rc.model(rc.index_arrays(index), bases, offsets, K, rc.NO_FILTER, False, None)
    r1, r2 = rp.records(t1, rh.FASTQ), rp.records(t2, rh.FASTQ)
    common = ["select-reads", "-i", npz, "-k", "31", "-c", "1500", "-I", str(rc.NO_FILTER), "--min-hits", "3"]
    for flags, rule in (([], dict(pair_rule=rp.ANY)), (["--pair-rule", "both"], dict(pair_rule=rp.BOTH)),
                        (["--pair-rule", "any", "--invert"], dict(pair_rule=rp.ANY, invert=True))):
        keep = rp.pair_keep_entries(hits, windows, min_hits=3, **rule)
        assert 0 < keep.sum() < len(pairs)
        want1 = b"".join(a[0] for a, kp in zip(r1, keep) if kp)
        want2 = b"".join(b[0] for b, kp in zip(r2, keep) if kp)
        out, hits_out = str(tmp_path / "kept.fq"), str(tmp_path / "hits")
        seen, kept = run_argument_parser(common + ["-f", paths["both"], "--interleaved", "-o", out, "--hits-output", hits_out] + flags)
        assert (seen, kept) == (2 * len(pairs), 2 * int(keep.sum()))
        assert rp.deinterleave(open(out, "rb").read(), rh.FASTQ) == (want1, want2)
        assert np.array_equal(np.load(hits_out + ".npy"), hits) and np.array_equal(np.load(hits_out + ".windows.npy"), windows)
        out1, out2 = str(tmp_path / "kept1.fq"), str(tmp_path / "kept2.fq")
        seen, kept = run_argument_parser(common + ["-f", paths["r1"], "-f2", paths["r2"], "-o", out1, "-o2", out2, "--hits-output", hits_out] + flags)
        assert (seen, kept) == (2 * len(pairs), 2 * int(keep.sum()))
        got1, got2 = open(out1, "rb").read(), open(out2, "rb").read()
        assert (got1, got2) == (want1, want2)
        assert len(rp.records(got1, rh.FASTQ)) == len(rp.records(got2, rh.FASTQ)) and _names(got1, rh.FASTQ) == _names(got2, rh.FASTQ)
        assert np.array_equal(np.load(hits_out + ".npy"), hits) and np.array_equal(np.load(hits_out + ".windows.npy"), windows)
    # an unpaired trailing record, and files of different record counts: errors that name the counts
    lone = rp.rec(rh.FASTQ, rc.gslice(0, 90).tobytes(), b"lone", 1)
    open(paths["both"], "wb").write(pack(both + lone))
    with pytest.raises(ValueError, match="does not end with a whole pair: it holds %d whole records, %d mate-1 and %d mate-2 "
                                         % (2 * len(pairs) + 1, len(pairs) + 1, len(pairs))):
        run_argument_parser(common + ["-f", paths["both"], "--interleaved", "-o", str(tmp_path / "odd.fq")])
    open(paths["r1"], "wb").write(pack(t1 + lone))
    with pytest.raises(ValueError, match="holds %d records and .* holds %d" % (len(pairs) + 1, len(pairs))):
        run_argument_parser(common + ["-f", paths["r1"], "-f2", paths["r2"], "-o", str(tmp_path / "o1.fq"), "-o2", str(tmp_path / "o2.fq")])
    for name, text in (("r1", t1 + lone), ("r2", t2)):
        assert open(paths[name], "rb").read() == pack(text)
