"""GPU tests of the record-hits mode (include/kmm.h): every case of tests/record_hits_cases.py against the
catalogue's parser + model (held to a second route by tests/test_record_hits_on_the_cpu.py) under the index layouts that
select the four probe flavours, from host and from device bytes; the same texts cut into pieces and fed as two calls; the six
input routes; the mode's purity; the queue; the refusals; the command line."""
import ctypes
import gzip
import os

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests.test_gpu_read_hits import LAYOUTS

pytestmark = pytest.mark.gpu

CASES = rh.all_cases()
IDS = [c.name for c in CASES]
_P = ctypes.c_void_p


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


def _kfmt(case):
    from kmer_mapper_amd import _lib
    return _lib.FORMAT_FASTQ if case.fmt == rh.FASTQ else _lib.FORMAT_FASTA2


def _map(dev, case, raw=None, **kw):
    return dev.map_records(case.text if raw is None else raw, fmt=_kfmt(case), k=case.k, max_index_lookup_frequency=case.max_freq,
                           also_revcomp=case.revcomp, lut=case.lut, **kw)


def _same(got, want):
    assert got.dtype == np.uint32 and got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), int(np.nonzero(got != want)[0][0])


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_against_the_model(kmm, monkeypatch, case, layout):
    import torch
    want_h, want_w, want_consumed, want_records = rh.expected(case)
    with _open(kmm, case.index, monkeypatch, layout) as dev:
        dev.record_hits(True, windows=True)
        assert dev.get_param("record_hits") == 2
        assert _map(dev, case) == (want_consumed, want_records)                    # host bytes
        assert dev.get_param("record_hits_pending") == want_records
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)
        assert dev.get_param("record_hits_pending") == 0
        d_text = torch.from_numpy(case.text).cuda()                                # device bytes
        d_lut = None if case.lut is None else torch.from_numpy(case.lut).cuda()
        got = dev.map_records(d_text, fmt=_kfmt(case), k=case.k, max_index_lookup_frequency=case.max_freq, also_revcomp=case.revcomp,
                              lut=d_lut)
        assert got == (want_consumed, want_records)
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)
        dev.record_hits(True)                                                      # hits alone
        assert dev.get_param("record_hits") == 1
        assert _map(dev, case) == (want_consumed, want_records)
        _same(dev.take_record_hits(), want_h)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)


def _longest_record(case):
    ends = np.nonzero(case.text == 10)[0][rh.PERIOD[case.fmt] - 1::rh.PERIOD[case.fmt]] + 1
    return int(np.diff(np.concatenate([[0], ends])).max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_pieces_and_two_calls_keep_file_order(kmm, monkeypatch, case):
    """The text cut into pieces of 1 or 4 KiB ("debug_records_piece_kb": every piece holds a whole record), and fed as two calls,
    the second with the bytes the first did not consume in front: every record once, in file order."""
    want_h, want_w, want_consumed, want_records = rh.expected(case)
    piece_kb = 1 if _longest_record(case) < 1024 else 4
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        dev.set_param("debug_records_piece_kb", piece_kb)
        assert _map(dev, case) == (want_consumed, want_records)
        if case.text.shape[0] > piece_kb << 10:
            assert dev.get_param("record_hits_pending") == want_records
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)
        dev.set_param("debug_records_piece_kb", 0)
        first_end = int(np.nonzero(case.text == 10)[0][rh.PERIOD[case.fmt] - 1]) + 1
        for cut in (max(case.text.shape[0] * 2 // 5, first_end + 3), case.text.shape[0] - 3):   # (inside a record behind the first)
            used_1, n_1 = _map(dev, case, case.text[:cut].copy())
            assert 0 < used_1 <= cut and n_1 > 0
            used_2, n_2 = _map(dev, case, case.text[used_1:].copy())
            assert (used_1 + used_2, n_1 + n_2) == (want_consumed, want_records)
            assert dev.get_param("record_hits_pending") == want_records
            hits, windows = dev.take_record_hits()
            _same(windows, want_w)
            _same(hits, want_h)


# ---------------------------------------------------------------------------------------------- the routes
K = 31


def _route_reads():
    """Genome slices with hits, a read without a hit, reads shorter than k, and (where the format has one) an empty read."""
    reads = [rc.gslice(150 * i, 150).tobytes() for i in range(40)] + [r.tobytes() for r in rc.trio(K)] + [rc.gslice(77, 1300).tobytes()]
    reads[5] = reads[5][:20]
    reads[9] = b"T" * 90
    return reads


def _want(index, reads, revcomp=False, k=K):
    bases, offsets = rh.reads_arrays(reads)
    return rc.model(rc.index_arrays(index), bases, offsets, k, rc.NO_FILTER, revcomp, None)


def _batch(reads):
    from kmer_mapper_amd.util import ReadBatch
    bases, offsets = rh.reads_arrays(reads)
    return ReadBatch(bases, offsets)


def test_bgzf_fastq_with_records_across_members_and_calls(kmm, monkeypatch):
    from kmer_mapper_amd import _lib, reads_io
    index = rc.genome_index(K)
    reads = _route_reads()
    text = rh.text_of(rh.FASTQ, reads)
    comp = np.frombuffer(reads_io.bgzf_members(text, block=997) + reads_io.BGZF_EOF, dtype=np.uint8)     # no record ends with a member
    want_h, want_w = _want(index, reads)
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        cut = comp.shape[0] * 2 // 5
        used_1, n_1 = dev.map_bgzf(comp[:cut], fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, first=True)
        assert 0 < used_1 <= cut and 0 < n_1 < len(reads)
        assert dev.get_param("record_hits_pending") == n_1
        used_2, n_2 = dev.map_bgzf(comp[used_1:], fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, last=True)
        assert used_1 + used_2 == comp.shape[0] and n_1 + n_2 == len(reads)
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)
        assert not dev.get_node_counts().any()


def test_plain_gzip(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    index = rc.genome_index(K)
    reads = _route_reads()
    comp = np.frombuffer(gzip.compress(rh.text_of(rh.FASTQ, reads), 6), dtype=np.uint8)
    want_h, want_w = _want(index, reads)
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        used, n = dev.map_gzip(comp, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER, first=True, last=True)
        assert (used, n) == (comp.shape[0], len(reads))
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)


def test_multi_line_fasta(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    index = rc.genome_index(K)
    reads = [r for r in _route_reads() if r]
    text = b"".join(b">r%d\n" % i + b"".join(r[j:j + 60] + b"\n" for j in range(0, len(r), 60)) for i, r in enumerate(reads))
    want_h, want_w = _want(index, reads)
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        raw = np.frombuffer(text, dtype=np.uint8)
        used, n = dev.map_records(raw, fmt=_lib.FORMAT_FASTA | _lib.FORMAT_LAST_CHUNK, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n) == (len(text), len(reads))
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)


def test_sam_text(kmm, monkeypatch):
    from kmer_mapper_amd import _lib, reads_io
    index = rc.genome_index(K)
    reads = _route_reads() + [b""]                                                  # SEQ "*": an entry of 0 / 0
    text = reads_io.sam_text(_batch(reads))
    want_h, want_w = _want(index, reads)
    assert want_w[-1] == 0
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        used, n = dev.map_records(np.frombuffer(text, dtype=np.uint8), fmt=_lib.FORMAT_SAM, k=K, max_index_lookup_frequency=rc.NO_FILTER)
        assert (used, n) == (len(text), len(reads))
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)


def _bam_bytes(reads, flags=None):
    from kmer_mapper_amd import reads_io
    return np.frombuffer(reads_io.bgzf_members(reads_io.bam_header((), b"@HD\tVN:1.6\tSO:unsorted\n")) +
                         reads_io.bgzf_members(reads_io.bam_records(_batch(reads), flags=flags), block=3001) + reads_io.BGZF_EOF,
                         dtype=np.uint8)


def _map_bam(dev, comp, revcomp=False):
    return dev.map_bam(comp, first=True, last=True, k=K, max_index_lookup_frequency=rc.NO_FILTER, also_revcomp=revcomp)


def test_bam_and_its_include_flags(kmm, monkeypatch):
    index = rc.genome_index(K)
    reads = _route_reads() + [b""]                                                  # l_seq = 0: an entry of 0 / 0
    flags = [4 if i % 3 else 0 for i in range(len(reads))]
    comp = _bam_bytes(reads, flags)
    want_h, want_w = _want(index, reads)
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        assert _map_bam(dev, comp) == (comp.shape[0], len(reads))
        hits, windows = dev.take_record_hits()
        _same(windows, want_w)
        _same(hits, want_h)
        dev.set_param("bam_include_flags", 4)                                       # --include-flags 4: fewer entries, the right reads
        kept = [i for i, f in enumerate(flags) if f & 4]
        assert 0 < len(kept) < len(reads)
        assert _map_bam(dev, comp) == (comp.shape[0], len(kept))
        hits, windows = dev.take_record_hits()
        _same(windows, want_w[kept])
        _same(hits, want_h[kept])
        assert not dev.get_node_counts().any()


def test_bam_original_strand_gives_the_hits_of_the_fastq(kmm, monkeypatch):
    """Every third record stored on the reverse strand (FLAG 0x10, SEQ reverse-complemented): with "original_strand" the entries
    are those of the FASTQ the records were made from — with the other orientation off, so that orientation matters."""
    from kmer_mapper_amd import _lib, reads_io
    index = rc.genome_index(K)
    reads = _route_reads()
    flags = [16 if i % 3 == 0 else 0 for i in range(len(reads))]
    stored = [reads_io.stored_form(r, reverse=bool(f & 16))[0] for r, f in zip(reads, flags)]
    comp = _bam_bytes(stored, flags)
    with _open(kmm, index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        fastq = np.frombuffer(rh.text_of(rh.FASTQ, reads), dtype=np.uint8)
        assert dev.map_records(fastq, fmt=_lib.FORMAT_FASTQ, k=K, max_index_lookup_frequency=rc.NO_FILTER)[1] == len(reads)
        fq_hits, fq_windows = dev.take_record_hits()
        _same(fq_hits, _want(index, reads)[0])
        assert _map_bam(dev, comp)[1] == len(reads)
        as_stored, _ = dev.take_record_hits()
        _same(as_stored, _want(index, stored)[0])
        assert not np.array_equal(as_stored, fq_hits)
        dev.set_param("original_strand", 1)
        assert _map_bam(dev, comp)[1] == len(reads)
        hits, windows = dev.take_record_hits()
        _same(hits, fq_hits)
        _same(windows, fq_windows)


# ---------------------------------------------------------------------------------------------- purity, the queue
def _case(name):
    return next(c for c in CASES if c.name == name)


def test_mode_on_calls_leave_counts_and_statistics_alone(kmm, monkeypatch, oracle):
    case, other = _case("seams_fastq_k31"), _case("long_header_fastq_k31")
    want_h, want_w, _, want_records = rh.expected(case)
    reads = rh.parse(case.text, case.fmt)[0]
    bases, offsets = rh.reads_arrays(reads)
    mx = case.index.max_node_id()
    want_counts = oracle.map_reads(case.index, mx, bases, offsets, case.k, n_threads=4)[0]
    with _open(kmm, case.index, monkeypatch) as dev:
        assert dev.get_param("radix_available") == 1
        dev.count_kmers_mode()
        _map(dev, case)
        counts, kmer_counts, stats = dev.get_node_counts().copy(), dev.get_kmer_counts().copy(), dev.get_stats()
        assert np.array_equal(counts, want_counts) and counts.any() and kmer_counts.any()
        dev.record_hits(True, windows=True)
        _map(dev, case)
        _map(dev, other)
        assert np.array_equal(dev.get_node_counts(), counts) and np.array_equal(dev.get_kmer_counts(), kmer_counts)
        assert dev.get_stats() == stats
        pending = dev.get_param("record_hits_pending")
        assert pending == want_records + rh.expected(other)[3]
        # the mode off: the same chunk counts nodes again, as if the mode had never been on; what is pending stays takeable
        dev.record_hits(False)
        _map(dev, case)
        assert np.array_equal(dev.get_node_counts(), 2 * want_counts)
        assert dev.get_param("record_hits_pending") == pending
        hits, windows = dev.take_record_hits()
        _same(hits, np.concatenate([want_h, rh.expected(other)[0]]))
        _same(windows, np.concatenate([want_w, rh.expected(other)[1]]))
        # kmm_reset_counts empties the queue
        dev.record_hits(True)
        _map(dev, case)
        assert dev.get_param("record_hits_pending") == want_records
        dev.reset()
        assert dev.get_param("record_hits_pending") == 0 and dev.take_record_hits().shape == (0,)


def test_take_in_parts_into_device_memory_and_windows_in_mode_1(kmm, monkeypatch):
    import torch
    from kmer_mapper_amd import _lib
    case = _case("short_and_empty_fastq_k16")
    want_h, want_w, _, n = rh.expected(case)
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.record_hits(True, windows=True)
        _map(dev, case)
        _map(dev, case)
        first = dev.take_record_hits(capacity=n // 3)                               # a capacity below what is pending, then the rest
        assert first[0].shape == (n // 3,) and dev.get_param("record_hits_pending") == 2 * n - n // 3
        _map(dev, case)                                                             # (appended behind what is left)
        rest = dev.take_record_hits()
        _same(np.concatenate([first[0], rest[0]]), np.tile(want_h, 3))
        _same(np.concatenate([first[1], rest[1]]), np.tile(want_w, 3))
        _map(dev, case)                                                             # into device memory, hits and windows apart
        dt = getattr(torch, "uint32", torch.int32)
        d_hits = torch.zeros(n + 5, dtype=dt, device="cuda")
        h_windows = np.zeros(n + 5, dtype=np.uint32)
        assert dev.take_record_hits(out=(d_hits, h_windows)) == n
        _same(d_hits.cpu().numpy().view(np.uint32)[:n], want_h)
        _same(h_windows[:n], want_w)
        dev.record_hits(True)                                                       # mode 1: windows given is refused
        _map(dev, case)
        taken = ctypes.c_int64(-1)
        buf = np.zeros(n, dtype=np.uint32)
        code = _lib.lib().kmm_take_record_hits(dev._h, buf.ctypes.data_as(_P), h_windows.ctypes.data_as(_P), n, ctypes.byref(taken))
        assert code == _lib.KMM_ERR_INVALID_ARG and taken.value == 0 and dev.get_param("record_hits_pending") == n
        with pytest.raises(ValueError, match="record_hits 2 with"):                 # (1 -> 2 with entries pending)
            dev.set_param("record_hits", 2)
        _same(dev.take_record_hits(), want_h)
        with pytest.raises(ValueError, match="record_hits takes 0"):
            dev.set_param("record_hits", 3)


def test_an_index_without_a_radix_view_is_served(kmm, monkeypatch):
    import types
    case = _case("several_nodes_k31_fasta")
    index = case.index
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo, max_node_id=index.max_node_id)
    with _open(kmm, dup, monkeypatch) as dev:
        assert dev.get_param("radix_available") == 0
        dev.record_hits(True, windows=True)
        _map(dev, case)
        hits, windows = dev.take_record_hits()
        want = rh.run_model(case._replace(index=dup))
        _same(hits, want[0])
        _same(windows, want[1])
        assert hits.any()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_map_nothing(kmm, monkeypatch):
    from kmer_mapper_amd import _lib, reads_io
    case = _case("seams_fastq_k31")
    want_h, _, _, n = rh.expected(case)
    reads = rh.parse(case.text, case.fmt)[0]
    bases, offsets = rh.reads_arrays(reads)
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.record_hits(True)
        dev.set_param("min_base_quality", 20)                                       # no quality floor in this mode
        with pytest.raises(ValueError, match="applies no quality floor"):
            _map(dev, case)
        comp = np.frombuffer(reads_io.bgzf_members(case.text.tobytes()) + reads_io.BGZF_EOF, dtype=np.uint8)
        with pytest.raises(ValueError, match="applies no quality floor"):
            dev.map_bgzf(comp, fmt=_lib.FORMAT_FASTQ, k=case.k, first=True, last=True)
        dev.set_param("min_base_quality", 0)
        for call in (lambda: dev.map_reads(bases, offsets, case.k),                 # flat reads have kmm_read_hits
                     lambda: dev.map_reads_uniform(bases, 4, 31, case.k),
                     lambda: dev.map_packed(np.zeros(4, np.uint32), 62, 2, read_len=31, k=case.k),
                     lambda: dev.map_kmers(np.zeros(4, np.uint64), k=case.k)):
            with pytest.raises(ValueError, match="record_hits"):
                call()
        assert dev.get_param("record_hits_pending") == 0
        # text the SAM parser rejects: the call fails, nothing is appended, the handle serves the next call
        sam = reads_io.sam_text(_batch(reads[:5])) + b"r9\t4\t*\t0\n"
        with pytest.raises(ValueError, match="fewer than 11"):
            dev.map_records(np.frombuffer(sam, dtype=np.uint8), fmt=_lib.FORMAT_SAM, k=case.k)
        assert dev.get_param("record_hits_pending") == 0
        # a record line that does not start with '+': found on the device, so deferred and sticky — take reports it and takes
        # nothing; kmm_reset_counts clears the error and the queue
        bad = case.text.copy()
        plus = int(np.nonzero(bad == ord("+"))[0][0])
        assert bad[plus - 1] == 10 and bad[plus + 1] == 10
        bad[plus] = ord("-")
        assert _map(dev, case, bad)[1] == n
        with pytest.raises(ValueError, match="record structure violated"):
            dev.take_record_hits()
        assert dev.get_param("record_hits_pending") == n
        with pytest.raises(ValueError, match="record structure violated"):
            dev.synchronize()
        dev.reset()
        assert dev.get_param("record_hits_pending") == 0
        _map(dev, case)
        _same(dev.take_record_hits(), want_h)
        assert not dev.get_node_counts().any() and dev.get_stats() == (0, 0)


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade(kmm):
    from kmer_mapper_amd import mapper
    case = _case("crlf_fastq_k31")
    want_h, want_w, consumed, n = rh.expected(case)
    try:
        hits, windows, used = mapper.record_hits(case.index, case.text, fmt="fastq", k=case.k, max_index_lookup_frequency=case.max_freq,
                                                 windows=True)
        _same(hits, want_h)
        _same(windows, want_w)
        assert used == consumed and len(mapper._CACHE) == 1
        hits, used = mapper.record_hits(case.index, b">a\nACGT\n>b\n", fmt="fasta", k=2)
        assert hits.shape == (1,) and used == 8 and len(mapper._CACHE) == 1
    finally:
        mapper.clear_cache()


@pytest.mark.parametrize("kind", ["fq", "fq_gz", "bam"])
def test_command_line_end_to_end(kmm, tmp_path, kind):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    case = next(c for c in rc.all_cases() if c.name == "breaks_k31")
    lens = np.diff(case.offsets)
    reads = [case.bases[case.offsets[r]:case.offsets[r + 1]].tobytes() for r in np.nonzero(lens > 0)[0]]
    bases, offsets = rh.reads_arrays(reads)
    text = rh.text_of(rh.FASTQ, reads)
    flags = None
    if kind == "fq":
        path = str(tmp_path / "reads.fq")
        open(path, "wb").write(text)
    elif kind == "fq_gz":
        path = str(tmp_path / "reads.fq.gz")
        open(path, "wb").write(reads_io.bgzf_members(text, block=4001) + reads_io.BGZF_EOF)
    else:
        path = str(tmp_path / "reads.bam")
        flags = [4 if i % 2 else 0 for i in range(len(reads))]
        reads_io.write_bam(path, _batch(reads), flags=flags)
    npz = str(tmp_path / "index.npz")
    case.index.to_file(npz)
    out, host_out = str(tmp_path / "out"), str(tmp_path / "host")
    common = ["read-hits", "-i", npz, "-f", path, "-k", "31", "-c", "1500", "--windows", "-I", "2", "-r", "True", "--min-hits", "2",
              "--ambiguous-bases", "skip"]
    want_h, want_w = rc.model(rc.index_arrays(case.index), bases, offsets, 31, 2, True, case.lut)
    got = run_argument_parser(common + ["-o", out, "--device-parser"])
    _same(np.load(out + ".npy"), want_h)
    _same(np.load(out + ".windows.npy"), want_w)
    _same(got[0], want_h)
    if kind != "bam":                                                               # the host-parsed route on the same file
        run_argument_parser(common + ["-o", host_out])
        assert np.array_equal(np.load(host_out + ".npy"), np.load(out + ".npy"))
        assert np.array_equal(np.load(host_out + ".windows.npy"), np.load(out + ".windows.npy"))
    else:
        kept = [i for i, f in enumerate(flags) if f & 4]
        got = run_argument_parser(common + ["-o", out, "--device-parser", "--include-flags", "4"])
        _same(got[0], want_h[kept])
        _same(np.load(out + ".windows.npy"), want_w[kept])
