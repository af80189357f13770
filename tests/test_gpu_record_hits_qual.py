"""GPU tests of the base-quality floor of the record-hits mode ("record_hits_min_base_quality", include/kmm.h):
every case of tests/record_hits_qual_cases.py through kmm_map_records against the catalogue's parser + model — hits, windows,
consumed, n_records, quality_masked_bases, and under a keep rule the kept bytes, which are the records' own bytes whatever the
floor —; the stream cases through BGZF and gzip with a record split between two calls; pieces; mates in one and in two buffers;
the BAM forms and SAM text; the refusals, the deferred KMM_ERR_MALFORMED, an index without a radix view, the timing slot, the
route that already has a floor, and the command line."""
import gzip

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_qual_cases as qh

pytestmark = pytest.mark.gpu

CASES = qh.all_cases()
IDS = [c.name for c in CASES]
K = qh.K


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _open(kmm, index):
    return kmm.DeviceIndex.from_index(index, index.max_node_id())


def _fastq():
    from kmer_mapper_amd import _lib
    return _lib.FORMAT_FASTQ


def _same(got, want):
    assert got.dtype == np.uint32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), (int(np.nonzero(got != want)[0][0]), got[got != want][:4], want[got != want][:4])


def _mode(dev, case, q=None):
    dev.record_hits(True, windows=True, min_base_quality=case.q if q is None else q)
    if case.rule:
        dev.record_keep(True, min_hits=case.rule[0], min_permille=case.rule[1])
    if case.pairs:
        dev.record_pairs(True, rule=case.pairs)


def _map(dev, case, raw=None):
    return dev.map_records(case.text if raw is None else raw, fmt=_fastq(), k=case.k, max_index_lookup_frequency=rc.NO_FILTER, lut=case.lut)


def _check_entries(dev, case, q=None):
    e = qh.expected(case, q)
    hits, windows = dev.take_record_hits()
    _same(windows, e.windows)
    _same(hits, e.hits)
    if case.rule:
        text, n = dev.take_kept_records()
        keep, want = qh.kept(case, q)
        assert n == int(keep.sum()) and text.tobytes() == want
    return e


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model(kmm, case):
    e = qh.expected(case)
    with _open(kmm, case.index) as dev:
        dev.set_timing(True)
        _mode(dev, case, 0)                                                        # the floor off: the mode as it was
        assert _map(dev, case) == (e.consumed, e.n_records)
        _check_entries(dev, case, 0)
        assert dev.get_param("quality_masked_bases") == 0
        assert tuple(dev.get_timing(_lib().KERNEL_RH_QUAL_MARK)) == (0.0, 0)
        _mode(dev, case)
        assert dev.get_param("record_hits_min_base_quality") == case.q
        assert _map(dev, case) == (e.consumed, e.n_records)
        _check_entries(dev, case)
        assert dev.get_param("quality_masked_bases") == e.masked
        assert dev.get_timing(_lib().KERNEL_RH_QUAL_MARK)[1] >= 1
        assert not dev.get_node_counts().any()


def _lib():
    from kmer_mapper_amd import _lib
    return _lib


def test_device_bytes_and_mode_1(kmm):
    import torch
    case = qh.by_name("positions")
    e = qh.expected(case)
    with _open(kmm, case.index) as dev:
        dev.record_hits(True, windows=False, min_base_quality=case.q)
        assert dev.map_records(torch.from_numpy(case.text).cuda(), fmt=_fastq(), k=case.k, max_index_lookup_frequency=rc.NO_FILTER) == \
            (e.consumed, e.n_records)
        _same(dev.take_record_hits(), e.hits)
        dev.set_param("record_hits_min_base_quality", 0)                            # changed while nothing is pending, and while
        _map(dev, case)                                                             # entries are: an entry keeps its call's floor
        dev.set_param("record_hits_min_base_quality", case.q)
        _map(dev, case)
        _same(dev.take_record_hits(), np.concatenate([qh.expected(case, 0).hits, e.hits]))
        dev.record_hits(False)
        assert dev.get_param("record_hits_min_base_quality") == 0


def test_pieces_and_two_calls(kmm):
    """Pieces of PIECE_KB whose first record starts low; then two calls, the second with the unconsumed bytes in front."""
    case = qh.by_name("pieces")
    e = qh.expected(case)
    with _open(kmm, case.index) as dev:
        _mode(dev, case)
        dev.set_param("debug_records_piece_kb", qh.PIECE_KB)
        assert _map(dev, case) == (e.consumed, e.n_records)
        _check_entries(dev, case)
        dev.set_param("debug_records_piece_kb", 0)
        cut = e.recs[40].qual_at + 7                                                # inside a quality line
        used_1, n_1 = _map(dev, case, case.text[:cut].copy())
        assert (used_1, n_1) == (e.recs[39].end, 40)
        used_2, n_2 = _map(dev, case, case.text[used_1:].copy())
        assert (used_1 + used_2, n_1 + n_2) == (e.consumed, e.n_records)
        _check_entries(dev, case)
        assert dev.get_param("quality_masked_bases") == 2 * e.masked


STREAM_CASES = ("positions", "seam_1024_base_last", "seam_256_qual_first", "crlf_lookalikes", "keep_min_permille")


@pytest.mark.parametrize("name", STREAM_CASES)
def test_bgzf_and_gzip_streams_in_two_calls(kmm, name):
    from kmer_mapper_amd import reads_io
    case = qh.by_name(name)
    e = qh.expected(case)
    text = case.text.tobytes()
    bgzf = np.frombuffer(reads_io.bgzf_members(text, block=997) + reads_io.BGZF_EOF, dtype=np.uint8)   # no record ends with a member
    gz = np.frombuffer(gzip.compress(text, 6), dtype=np.uint8)
    with _open(kmm, case.index) as dev:
        _mode(dev, case)
        for comp, entry in ((bgzf, dev.map_bgzf), (gz, dev.map_gzip)):
            pos, end, total = 0, comp.shape[0] * 2 // 5, 0
            while pos < comp.shape[0]:
                used, n = entry(comp[pos:end], fmt=_fastq(), k=case.k, max_index_lookup_frequency=rc.NO_FILTER, lut=case.lut,
                                first=pos == 0, last=end == comp.shape[0])
                total += n
                pos += used
                if used == 0 or end < comp.shape[0]:
                    assert end < comp.shape[0]
                    end = comp.shape[0]
            assert total == e.n_records
            _check_entries(dev, case)
        assert dev.get_param("quality_masked_bases") == 2 * e.masked


@pytest.mark.parametrize("name", ["pairs_any", "pairs_both"])
def test_mates_in_two_buffers(kmm, name):
    case = qh.by_name(name)
    e = qh.expected(case)
    raw1, raw2 = qh.mate_texts(case)
    keep, _ = qh.kept(case)
    text = case.text.tobytes()
    with _open(kmm, case.index) as dev:
        dev.record_hits(True, windows=True, min_base_quality=case.q)
        dev.record_keep(True, min_hits=case.rule[0], min_permille=case.rule[1])
        dev.record_pairs(False, rule=case.pairs)
        used1, used2, m = dev.map_record_pairs(raw1, raw2, fmt=_fastq(), k=case.k, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used1, used2, m) == (raw1.shape[0], raw2.shape[0], e.n_records // 2)
        hits, windows = dev.take_record_hits()
        _same(windows, e.windows)
        _same(hits, e.hits)
        for mate in (0, 1):
            got, n = dev.take_kept_mates(mate)
            want = b"".join(text[r.start:r.end] for r, on in list(zip(e.recs, keep))[mate::2] if on)
            assert n == int(keep.sum()) // 2 and got.tobytes() == want
        assert dev.get_param("quality_masked_bases") == e.masked


# ---------------------------------------------------------------------------------------------- BAM and SAM
Q = 20


def _bam_in_two_calls(dev, bam, **kw):
    pos, end, total = 0, bam.shape[0] // 2, 0
    while pos < bam.shape[0]:
        used, n = dev.map_bam(bam[pos:end], first=pos == 0, last=end == bam.shape[0], k=K, max_index_lookup_frequency=rc.NO_FILTER, **kw)
        total += n
        pos += used
        if used == 0 or end < bam.shape[0]:
            assert end < bam.shape[0]
            end = bam.shape[0]
    return total


def _bam_handle(dev):
    dev.record_hits(True, windows=True, min_base_quality=Q)
    dev.set_param("use_record_qual", 1)
    dev.set_param("bam_exclude_flags", 0x400)
    dev.set_param("original_strand", 1)


def test_bam_plain_and_named(kmm):
    recs = qh.bam_records()
    h, w, masked, no_qual, texts = qh.bam_expected(recs, Q)
    h0, w0, _, _, _ = qh.bam_expected(recs, 0)
    bam = qh.bam_file(recs, block=700)
    with _open(kmm, rc.genome_index(K)) as dev:
        _bam_handle(dev)
        assert _bam_in_two_calls(dev, bam) == h.shape[0]                            # the decode's quality variant: '~' for 0xFF
        hits, windows = dev.take_record_hits()
        _same(windows, w)
        _same(hits, h)
        assert dev.get_param("quality_masked_bases") == masked and dev.get_param("records_without_qual") == no_qual
        dev.reset()
        dev.get_stats(reset=True)                                                   # (the counters of the decode and the mark pass)
        dev.record_keep(True, min_hits=8)                                           # the named form: '"' for 0xFF, exempt
        dev.record_names(True)
        assert _bam_in_two_calls(dev, bam) == h.shape[0]
        hits, windows = dev.take_record_hits()
        _same(windows, w)
        _same(hits, h)
        text, n = dev.take_kept_records()
        keep = qh.passes(h, w, (8, 0))
        assert n == int(keep.sum()) and text.tobytes() == b"".join(t for t, on in zip(texts, keep) if on)
        assert 0 < keep.sum() < qh.passes(h0, w0, (8, 0)).sum()
        assert dev.get_param("quality_masked_bases") == masked and dev.get_param("records_without_qual") == no_qual
        dev.record_names(False)
        dev.record_keep(False)


def _mate_records():
    """A name-collated file: mates 2p and 2p + 1 share a name; records without qualities on either side of a pair."""
    out = []
    for p in range(9):
        for mate in (0, 1):
            i = 2 * p + mate
            qual = None if i in (3, 8, 9, 17) else qh._phred(qh.L, range(10, 125) if p % 3 == 0 and mate == 0 else [6], seed=i)
            out.append(qh.BRec(b"pair%d" % p, (0x41, 0x81)[mate] | (0x10 if i % 4 == 1 else 0), qh.hit(qh.L, 370 * i + 11), qual))
    return out


def test_bam_mates_named_and_raw(kmm):
    from tests import bam_fastq_cases as bf
    from kmer_mapper_amd import reads_io
    recs = _mate_records()
    h, w, masked, no_qual, texts = qh.bam_expected(recs, Q)
    a, b = qh.passes(h, w, (3, 0))[0::2], qh.passes(h, w, (3, 0))[1::2]
    keep = np.repeat(a & b, 2)
    assert 0 < keep.sum() < keep.shape[0]
    raw = [reads_io.bam_record(r.seq, r.name, r.flag, qual=r.qual) for r in recs]
    for block in (700, 1900):                                                       # (windows that end behind a mate 1, or not)
        bam = qh.bam_file(recs, block=block)
        with _open(kmm, rc.genome_index(K)) as dev:
            _bam_handle(dev)
            dev.record_keep(True, min_hits=3)
            dev.record_names(True, pairs=True)                                      # interleaved FASTQ out
            dev.record_pairs(False, rule="both")
            assert _bam_in_two_calls(dev, bam) == h.shape[0]
            hits, windows = dev.take_record_hits()
            _same(windows, w)
            _same(hits, h)
            text, n = dev.take_kept_records()
            assert n == int(keep.sum()) and text.tobytes() == b"".join(t for t, on in zip(texts, keep) if on)
            assert dev.get_param("records_without_qual") == no_qual and dev.get_param("quality_masked_bases") == masked
            dev.record_names(False)
            dev.reset()
            for mates in (False, True):                                             # the records' own bytes out
                dev.record_bam(True, mates=mates)
                assert _bam_in_two_calls(dev, bam) == h.shape[0]
                hits, windows = dev.take_record_hits()
                _same(windows, w)
                _same(hits, h)
                on = keep if mates else qh.passes(h, w, (3, 0))
                data, _, n = dev.take_kept_bgzf()
                assert n == int(on.sum()) and bf.inflate(data.tobytes()) == b"".join(r for r, k_ in zip(raw, on) if k_)
            dev.record_bam(False)


def test_sam_text_hits(kmm):
    text, seqs, quals, exempt = qh.sam_case()
    h, w, masked = qh.model(rc.genome_index(K), K, seqs, quals, Q, exempt=exempt)
    with _open(kmm, rc.genome_index(K)) as dev:
        dev.record_hits(True, windows=True, min_base_quality=Q)
        dev.set_param("use_record_qual", 1)
        assert dev.map_records(text, fmt=_lib().FORMAT_SAM, k=K, max_index_lookup_frequency=rc.NO_FILTER) == (text.shape[0], len(seqs))
        hits, windows = dev.take_record_hits()
        _same(windows, w)
        _same(hits, h)
        assert dev.get_param("quality_masked_bases") == masked and dev.get_param("records_without_qual") == len(exempt)
        assert (w[exempt] == qh.L - K + 1).all()


# ---------------------------------------------------------------------------------------------- refusals, errors, routes
def test_refusals_map_nothing(kmm):
    from kmer_mapper_amd import reads_io
    case = qh.by_name("positions")
    e = qh.expected(case)
    sam = qh.sam_case()[0]
    bam = qh.bam_file(qh.bam_records())
    with _open(kmm, case.index) as dev:
        for bad in (-1, 94):
            with pytest.raises(ValueError, match="record_hits_min_base_quality outside"):
                dev.set_param("record_hits_min_base_quality", bad)
        dev.record_hits(True, windows=True, min_base_quality=20)
        with pytest.raises(ValueError, match="k = 1 with record_hits_min_base_quality 20"):
            dev.map_records(case.text, fmt=_fastq(), k=1)
        with pytest.raises(ValueError, match="record_hits_min_base_quality 20 is set, and SAM / BAM records are mapped without"):
            dev.map_records(sam, fmt=_lib().FORMAT_SAM, k=K)
        with pytest.raises(ValueError, match="record_hits_min_base_quality 20 is set, and SAM / BAM records are mapped without"):
            dev.map_bam(bam, first=True, last=True, k=K)
        dev.set_param("use_record_qual", 1)
        dev.record_keep(True)
        dev.record_sam(True)
        with pytest.raises(ValueError, match="\"record_sam\" is 1 and record_hits_min_base_quality is 20"):
            dev.map_records(sam, fmt=_lib().FORMAT_SAM, k=K)
        dev.record_sam(False)
        dev.record_keep(False)
        dev.set_param("min_base_quality", 20)                                       # the other floor stays refused, word for word
        with pytest.raises(ValueError, match="applies no quality floor"):
            _map(dev, case)
        dev.set_param("min_base_quality", 0)
        assert dev.get_param("record_hits_pending") == 0
        fasta = np.frombuffer(b"".join(b">r\n" + r.seq + b"\n" for r in e.recs), dtype=np.uint8)   # no qualities: served, no effect
        assert dev.map_records(fasta, fmt=_lib().FORMAT_FASTA2, k=K, max_index_lookup_frequency=rc.NO_FILTER)[1] == e.n_records
        _same(dev.take_record_hits()[0], qh.expected(case, 0).hits)
        assert _map(dev, case)[1] == e.n_records                                    # the handle serves the next call
        _same(dev.take_record_hits()[0], e.hits)


@pytest.mark.parametrize("which", [0, 1], ids=["qual_one_short", "qual_one_long"])
def test_a_quality_line_of_another_length_is_deferred_and_sticky(kmm, which):
    case, at = qh.malformed_cases()[which]
    with _open(kmm, case.index) as dev:
        dev.record_hits(True, windows=True, min_base_quality=case.q)
        n = _map(dev, case)[1]
        assert n == len(qh.parse_q(case.text)[0])
        for call in (dev.take_record_hits, dev.synchronize):
            with pytest.raises(ValueError, match="record structure violated at byte offset %d .*record_hits_min_base_quality" % at):
                call()
        assert dev.get_param("record_hits_pending") == n
        dev.reset()
        dev.record_hits(True, windows=True)                                         # without a floor the lengths are not compared
        _map(dev, case)
        assert dev.take_record_hits()[0].shape == (n,)


def test_an_index_without_a_radix_view_is_served(kmm):
    import types
    case = qh.by_name("positions")
    index = case.index
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo, max_node_id=index.max_node_id)
    recs = qh.expected(case).recs
    want_h, want_w, masked = qh.model(dup, case.k, [r.seq for r in recs], [r.qual for r in recs], case.q)
    with _open(kmm, dup) as dev:
        assert dev.get_param("radix_available") == 0
        _mode(dev, case)
        _map(dev, case)
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)
        assert hits.any() and dev.get_param("quality_masked_bases") == masked


@pytest.mark.parametrize("name", ["positions", "pieces", "seam_1024_qual_first", "values_q93"])
def test_the_route_that_already_has_a_floor_agrees(kmm, name):
    """FASTQ without the other orientation: the sum of the windows is n_lookups of kmm_map_records under "min_base_quality", and
    both routes count the same masked bases."""
    case = qh.by_name(name)
    e = qh.expected(case)
    with _open(kmm, case.index) as dev:
        assert dev.get_param("radix_available") == 1
        dev.set_param("min_base_quality", case.q)
        assert _map(dev, case) == (e.consumed, e.n_records)
        assert dev.get_stats()[0] == int(e.windows.sum())
        assert dev.get_param("quality_masked_bases") == e.masked


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    case, pairs = qh.by_name("keep_min_permille"), qh.by_name("pairs_both")
    e = qh.expected(case)
    try:
        hits, windows, used = mapper.record_hits(case.index, case.text, k=case.k, max_index_lookup_frequency=rc.NO_FILTER, windows=True,
                                                 min_base_quality=case.q)
        _same(windows, e.windows)
        _same(hits, e.hits)
        text, hits, windows = mapper.select_records(case.index, case.text, k=case.k, max_index_lookup_frequency=rc.NO_FILTER,
                                                    min_hits=case.rule[0], min_permille=case.rule[1], min_base_quality=case.q)
        assert text == qh.kept(case)[1]
        t1, t2, hits, windows = mapper.select_record_pairs(pairs.index, pairs.text, k=K, max_index_lookup_frequency=rc.NO_FILTER,
                                                           min_hits=3, pair_rule="both", min_base_quality=pairs.q)
        assert t2 is None and t1 == qh.kept(pairs)[1]
        _same(hits, qh.expected(pairs).hits)
        hits, used = mapper.record_hits(case.index, case.text, k=case.k, max_index_lookup_frequency=rc.NO_FILTER)   # the floor is off again
        _same(hits, qh.expected(case, 0).hits)
    finally:
        mapper.clear_cache()


def test_command_line_end_to_end(kmm, tmp_path):
    from kmer_mapper_amd import reads_io
    from tests import bam_fastq_cases as bf
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    case = qh.by_name("keep_min_permille")
    e = qh.expected(case)
    path, npz = str(tmp_path / "reads.fq.gz"), str(tmp_path / "index.npz")
    open(path, "wb").write(reads_io.bgzf_members(case.text.tobytes(), block=1500) + reads_io.BGZF_EOF)
    case.index.to_file(npz)
    out = str(tmp_path / "out")
    common = ["-i", npz, "-f", path, "-k", str(case.k), "-c", "1500", "-I", str(rc.NO_FILTER), "--min-base-quality", str(case.q)]
    got = run_argument_parser(["read-hits", "--windows", "-o", out] + common)      # (the floor implies the device parser)
    _same(got[0], e.hits)
    _same(got[1], e.windows)
    kept_path = str(tmp_path / "kept.fq.gz")
    seen, kept = run_argument_parser(["select-reads", "-o", kept_path, "--bgzf", "--min-hits", str(case.rule[0]), "--min-hit-permille",
                                      str(case.rule[1])] + common)
    keep, want = qh.kept(case)
    assert (seen, kept) == (e.n_records, int(keep.sum()))
    assert bf.inflate(open(kept_path, "rb").read()) == want
