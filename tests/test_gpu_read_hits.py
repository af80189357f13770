"""GPU tests of kmm_read_hits (include/kmm.h): every case of tests/read_hits_cases.py against the catalogue's
model (held to a second route and to its conditions by tests/test_read_hits_on_the_cpu.py) — hits and windows, from host
arrays, from device arrays and through the uniform entry where the lengths allow, under the index layouts that select the
four probe flavours; cross-checks against the map path; the call as a pure query; its errors; the command line."""
import ctypes
import gzip
import os

import numpy as np
import pytest

from tests import read_hits_cases as rc

pytestmark = pytest.mark.gpu

CASES = rc.all_cases()
# (environment at index creation, wide_buckets, occupancy_filter): the probe flavour launch_map_reads would choose
LAYOUTS = {
    "default": ({}, 0, 1),                                                          # 16-byte buckets behind the Bloom filter
    "wide": ({"KMM_OCC_MAX_BYTES": "0"}, 1, 0),                                     # 32-byte buckets, no filter
    "narrow": ({"KMM_OCC_MAX_BYTES": "0", "KMM_WIDE_BUCKETS": "0"}, 0, 0),          # 16-byte buckets, no filter
    "bloom_256": ({"KMM_BLOOM_BYTES": "256"}, 0, 1),                                # a heavily loaded Bloom filter
    "bitmap": ({"KMM_BLOOM_BYTES": "0", "KMM_OCC_SHIFT": "1"}, 0, 1),               # the per-bucket bitmap
    "wide_filter": ({"KMM_WIDE_BUCKETS": "1", "KMM_BLOOM_BYTES": "4096"}, 1, 1),    # wide buckets behind a filter
}
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


def _call(dev, case, **kw):
    return dev.read_hits(case.bases, case.offsets, k=case.k, max_index_lookup_frequency=case.max_freq, also_revcomp=case.revcomp,
                         lut=case.lut, windows=True, **kw)


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_against_the_model(kmm, monkeypatch, case, layout):
    import torch
    want_h, want_w = rc.expected(case)
    with _open(kmm, case.index, monkeypatch, layout) as dev:
        # host arrays
        hits, windows = _call(dev, case)
        assert hits.dtype == np.uint32 and windows.dtype == np.uint32
        assert np.array_equal(windows, want_w), int(np.nonzero(windows != want_w)[0][0])
        assert np.array_equal(hits, want_h), int(np.nonzero(hits != want_h)[0][0])
        only = dev.read_hits(case.bases, case.offsets, k=case.k, max_index_lookup_frequency=case.max_freq,
                             also_revcomp=case.revcomp, lut=case.lut)
        assert np.array_equal(only, want_h)                                        # windows == NULL
        # device arrays
        d_bases, d_offs = torch.from_numpy(case.bases).cuda(), torch.from_numpy(case.offsets).cuda()
        d_lut = None if case.lut is None else torch.from_numpy(case.lut).cuda()
        d_hits, d_windows = dev.read_hits(d_bases, d_offs, k=case.k, max_index_lookup_frequency=case.max_freq,
                                          also_revcomp=case.revcomp, lut=d_lut, windows=True)
        assert d_hits.is_cuda and d_windows.is_cuda
        assert np.array_equal(d_hits.cpu().numpy().view(np.uint32), want_h)
        assert np.array_equal(d_windows.cpu().numpy().view(np.uint32), want_w)
        # the uniform entry
        L = rc.uniform_length(case)
        if L is not None:
            n = case.offsets.shape[0] - 1
            for b, t in ((case.bases, case.lut), (d_bases, d_lut)):
                u_hits, u_windows = dev.read_hits(b, n_reads=n, read_len=L, k=case.k, max_index_lookup_frequency=case.max_freq,
                                                  also_revcomp=case.revcomp, lut=t, windows=True)
                if not isinstance(u_hits, np.ndarray):
                    u_hits, u_windows = u_hits.cpu().numpy().view(np.uint32), u_windows.cpu().numpy().view(np.uint32)
                assert np.array_equal(u_hits, want_h) and np.array_equal(u_windows, want_w)
        assert dev.get_param("read_hits_calls") == (5 if L is not None else 3)


def test_bases_not_aligned_to_16_bytes(kmm, monkeypatch):
    """A device array that starts in the middle of a vector: the byte-wise loads of the tile front end."""
    import torch
    case = next(c for c in CASES if c.name == "seams_k31")
    want_h, want_w = rc.expected(case)
    with _open(kmm, case.index, monkeypatch) as dev:
        buf = torch.zeros(case.bases.shape[0] + 16, dtype=torch.uint8, device="cuda")
        for shift in (1, 7):
            view = buf[shift:shift + case.bases.shape[0]]
            view.copy_(torch.from_numpy(case.bases))
            hits, windows = dev.read_hits(view, torch.from_numpy(case.offsets).cuda(), k=case.k, windows=True,
                                          max_index_lookup_frequency=case.max_freq)
            assert np.array_equal(hits.cpu().numpy().view(np.uint32), want_h)
            assert np.array_equal(windows.cpu().numpy().view(np.uint32), want_w)


# ---------------------------------------------------------------------------------------------- against the map path
@pytest.mark.parametrize("k", [16, 31])
def test_sums_equal_the_map_path(kmm, monkeypatch, k):
    """No k-mer twice in the index and the filter off: every hit window adds one to one node count."""
    index = rc.genome_index(k, several_nodes=False)
    assert np.unique(index._kmers).shape[0] == index._kmers.shape[0]
    cases = [c for c in CASES if c.k == k and c.rule is None and c.name.split("_k")[0] in ("seams", "empty_reads", "short_reads")]
    assert len(cases) == (3 if k == 31 else 2)
    with _open(kmm, index, monkeypatch) as dev:
        dev.set_param("path", 1)
        for case in cases:
            dev.reset()
            dev.get_stats(reset=True)
            dev.map_reads(case.bases, case.offsets, k, rc.NO_FILTER)
            counts = dev.get_node_counts()
            n_lookups, n_hits = dev.get_stats()
            hits, windows = dev.read_hits(case.bases, case.offsets, k=k, max_index_lookup_frequency=rc.NO_FILTER, windows=True)
            assert int(hits.sum()) == int(counts.sum()) == n_hits > 0
            assert int(windows.sum()) == n_lookups


def test_sums_equal_the_map_path_with_breaks(kmm, monkeypatch):
    case = next(c for c in CASES if c.name == "breaks_k31")
    index = rc.genome_index(31, several_nodes=False)
    with _open(kmm, index, monkeypatch) as dev:
        dev.set_param("path", 1)
        dev.map_reads(case.bases, case.offsets, 31, rc.NO_FILTER, lut=case.lut)
        counts = dev.get_node_counts()
        n_lookups, _ = dev.get_stats()
        hits, windows = dev.read_hits(case.bases, case.offsets, k=31, max_index_lookup_frequency=rc.NO_FILTER, lut=case.lut, windows=True)
        assert int(hits.sum()) == int(counts.sum()) > 0 and int(windows.sum()) == n_lookups


# ---------------------------------------------------------------------------------------------- a pure query
def test_the_call_is_a_pure_query(kmm, monkeypatch):
    case = next(c for c in CASES if c.name == "several_nodes_k31")
    other = next(c for c in CASES if c.name == "seams_k31")
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.map_reads(case.bases, case.offsets, 31)
        counts_1, stats_1 = dev.get_node_counts().copy(), dev.get_stats()
        _call(dev, other)
        _call(dev, case)
        assert np.array_equal(dev.get_node_counts(), counts_1) and dev.get_stats() == stats_1
        dev.map_reads(other.bases, other.offsets, 31)
        both = dev.get_node_counts().copy()
        stats_both = dev.get_stats()
    with _open(kmm, case.index, monkeypatch) as dev:                              # the two map calls alone
        dev.map_reads(case.bases, case.offsets, 31)
        dev.map_reads(other.bases, other.offsets, 31)
        assert np.array_equal(dev.get_node_counts(), both) and dev.get_stats() == stats_both
        assert dev.get_param("read_hits_calls") == 0


def test_works_on_indexes_without_a_radix_view(kmm, monkeypatch):
    """The call needs the direct view only: an index the radix path refuses (200 empty buckets alias occupied ones, whose
    entries never match there: wrong hash) and one with a single bucket are served all the same."""
    import types
    from kmer_mapper_amd.kmer_index import KmerIndex
    big = next(c for c in CASES if c.name == "several_nodes_k31")
    index = big.index
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo, max_node_id=index.max_node_id)
    kmers = np.asarray(index._kmers)
    one_bucket = KmerIndex.from_flat_kmers(kmers, np.arange(kmers.shape[0]) % 50, 1)
    for ix, no_radix in ((dup, True), (one_bucket, False)):
        with _open(kmm, ix, monkeypatch) as dev:
            if no_radix:
                assert dev.get_param("radix_available") == 0
            hits, windows = dev.read_hits(big.bases, big.offsets, k=31, max_index_lookup_frequency=rc.NO_FILTER, windows=True)
            want = rc.model(rc.index_arrays(ix), big.bases, big.offsets, 31)
            assert np.array_equal(hits, want[0]) and np.array_equal(windows, want[1]) and hits.any()


# ---------------------------------------------------------------------------------------------- errors
def _raw(dev, bases, offsets, k=31, lut=None, n_reads=None, hits=None):
    from kmer_mapper_amd import _lib
    n = offsets.shape[0] - 1 if n_reads is None else n_reads
    out = np.zeros(max(n, 1), dtype=np.uint32) if hits is None else hits
    code = _lib.lib().kmm_read_hits(dev._h, bases.ctypes.data_as(_P), offsets.ctypes.data_as(_P), n, 0, k, 1000, 0,
                                    None if lut is None else lut.ctypes.data_as(_P), out.ctypes.data_as(_P), None)
    return code, _lib.lib().kmm_last_error().decode()


def test_errors_come_from_the_call_and_leave_the_handle_alone(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    case = next(c for c in CASES if c.name == "seams_k31")
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.map_reads(case.bases, case.offsets, 31)
        counts = dev.get_node_counts().copy()
        bad = case.bases.copy()
        bad[2051] = ord("X")
        bad[3000] = ord("-")
        code, msg = _raw(dev, bad, case.offsets)
        assert code == _lib.KMM_ERR_INVALID_BASE and "offset 2051 " in msg
        assert np.array_equal(dev.get_node_counts(), counts)                        # no sticky error, nothing counted
        down = case.offsets.copy()
        down[5], down[6] = down[6], down[5]
        assert down[6] < down[5]
        code, msg = _raw(dev, case.bases, down)
        assert code == _lib.KMM_ERR_INVALID_ARG and "not non-decreasing at read 5" in msg
        first = case.offsets.copy()
        first[0] = 1
        assert _raw(dev, case.bases, first)[0] == _lib.KMM_ERR_INVALID_ARG
        for k in (0, 32):
            assert _raw(dev, case.bases, case.offsets, k=k)[0] == _lib.KMM_ERR_INVALID_ARG
        code = _lib.lib().kmm_read_hits(dev._h, case.bases.ctypes.data_as(_P), case.offsets.ctypes.data_as(_P), 3, 0, 31, 1000, 0, None,
                                        None, None)
        assert code == _lib.KMM_ERR_INVALID_ARG                                     # hits == NULL
        from kmer_mapper_amd.util import ambiguous_skip_lut
        assert _raw(dev, case.bases, case.offsets, k=1, lut=ambiguous_skip_lut())[0] == _lib.KMM_ERR_INVALID_ARG
        with pytest.raises(ValueError, match="offset 2051 "):
            dev.read_hits(bad, case.offsets)
        assert np.array_equal(dev.get_node_counts(), counts)
        dev.synchronize()
        # the call after the errors is served as any other
        hits = dev.read_hits(case.bases, case.offsets, k=31, max_index_lookup_frequency=case.max_freq)
        assert np.array_equal(hits, rc.expected(case)[0])


def test_nothing_to_look_up_is_accepted(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    case = next(c for c in CASES if c.name == "seams_k31")
    with _open(kmm, case.index, monkeypatch) as dev:
        assert _raw(dev, case.bases, case.offsets, n_reads=0)[0] == _lib.KMM_OK    # n_reads == 0
        assert dev.read_hits(np.zeros(0, np.uint8), np.zeros(1, np.int64)).shape == (0,)
        empty = np.zeros(6, np.int64)                                               # five reads, no bases at all
        hits = np.full(5, 7, np.uint32)
        assert _raw(dev, np.zeros(0, np.uint8), empty, hits=hits)[0] == _lib.KMM_OK and not hits.any()
        h, w = dev.read_hits(np.zeros(0, np.uint8), n_reads=4, read_len=0, windows=True)
        assert h.shape == (4,) and not h.any() and not w.any()
        import torch
        h, w = dev.read_hits(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda"), windows=True)
        assert h.is_cuda and h.numel() == 5 and not h.cpu().numpy().any() and not w.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade_goes_through_the_handle_cache(kmm):
    from kmer_mapper_amd import mapper
    case = next(c for c in CASES if c.name == "short_reads_k16")
    try:
        hits, windows = mapper.read_hits(case.index, (case.bases, case.offsets), k=16, max_index_lookup_frequency=case.max_freq, windows=True)
        assert np.array_equal(hits, rc.expected(case)[0]) and np.array_equal(windows, rc.expected(case)[1])
        assert len(mapper._CACHE) == 1
        again = mapper.read_hits(case.index, ["ACGT" * 10, "", "TTTT"], k=16)
        assert again.shape == (3,) and len(mapper._CACHE) == 1
    finally:
        mapper.clear_cache()


@pytest.mark.parametrize("gz", [False, True], ids=["fastq", "fastq_gz"])
def test_command_line_end_to_end(kmm, tmp_path, gz):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    case = next(c for c in CASES if c.name == "breaks_k31")
    lens = np.diff(case.offsets)
    keep = np.nonzero(lens > 0)[0]                                                  # (a FASTQ record needs a base)
    bases, offsets = rc.batch([case.bases[case.offsets[r]:case.offsets[r + 1]] for r in keep])
    fq = str(tmp_path / ("reads.fq.gz" if gz else "reads.fq"))
    reads_io.write_fastq(fq, ReadBatch(bases, offsets), gz=gz)
    if gz:
        with gzip.open(fq, "rb") as f:
            assert f.read(1) == b"@"
    npz = str(tmp_path / "index.npz")
    case.index.to_file(npz)
    out = str(tmp_path / "out")
    for extra, lut in ((["--ambiguous-bases", "skip"], case.lut), ([], None)):
        got = run_argument_parser(["read-hits", "-i", npz, "-f", fq, "-k", "31", "-o", out, "-c", "1500", "--windows", "-I", "2",
                                   "-r", "True", "--min-hits", "2"] + extra)
        want_h, want_w = rc.model(rc.index_arrays(case.index), bases, offsets, 31, 2, True, lut)
        assert np.array_equal(np.load(out + ".npy"), want_h) and np.array_equal(np.load(out + ".windows.npy"), want_w)
        assert np.array_equal(got[0], want_h) and np.load(out + ".npy").dtype == np.uint32
        os.remove(out + ".npy")
        os.remove(out + ".windows.npy")
    run_argument_parser(["read-hits", "-i", npz, "-f", fq, "-k", "31", "-o", out])
    assert os.path.exists(out + ".npy") and not os.path.exists(out + ".windows.npy")
