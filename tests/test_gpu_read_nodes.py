"""GPU tests of kmm_read_nodes (include/kmm.h): every case of tests/read_nodes_cases.py against the catalogue's
model (held to the oracle's map_reads and to its conditions by tests/test_read_nodes_on_the_cpu.py) — all five outputs, from
host arrays, from device arrays and through the uniform entry where the lengths allow, under the index layouts that select the
four probe flavours; every subset of NULL outputs; cross-checks against the map path; determinism and rounds; the call as a
pure query; its errors; the command line from `index` to `assign-reads`."""
import ctypes
import gzip
import itertools
import os

import numpy as np
import pytest

from tests import read_nodes_cases as nc
from tests.test_gpu_read_hits import LAYOUTS, _open

pytestmark = pytest.mark.gpu

CASES = nc.all_cases()
_P = ctypes.c_void_p


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _call(dev, case, **kw):
    return dev.read_nodes(case.bases, case.offsets, k=case.k, max_index_lookup_frequency=case.max_freq, also_revcomp=case.revcomp,
                          lut=case.lut, **kw)


def _assert_equal(got, want, what=""):
    for name, g, w in zip(nc.OUTPUTS, got[:5], want):
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        g = g.view(w.dtype)
        assert g.shape == w.shape, (what, name)
        bad = np.nonzero(g != w)[0]
        assert bad.shape[0] == 0, (what, name, int(bad[0]), int(g[bad[0]]), int(w[bad[0]]))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cases_against_the_model(kmm, monkeypatch, case, layout):
    import torch
    want = nc.expected(case)
    with _open(kmm, case.index, monkeypatch, layout) as dev:
        got = _call(dev, case)                                                      # host arrays
        assert got.best_node.dtype == np.int32 and all(a.dtype == np.uint32 for a in got[1:5])
        assert got.n_rounds == 1
        _assert_equal(got, want, "host")
        d_bases, d_offs = torch.from_numpy(case.bases).cuda(), torch.from_numpy(case.offsets).cuda()
        d_lut = None if case.lut is None else torch.from_numpy(case.lut).cuda()
        d_got = dev.read_nodes(d_bases, d_offs, k=case.k, max_index_lookup_frequency=case.max_freq, also_revcomp=case.revcomp,
                               lut=d_lut)                                           # device arrays
        assert all(a.is_cuda for a in d_got[:5])
        _assert_equal(d_got, want, "device")
        L = rc_uniform_length(case)
        if L is not None:                                                           # the uniform entry
            n = case.offsets.shape[0] - 1
            for b, t in ((case.bases, case.lut), (d_bases, d_lut)):
                u = dev.read_nodes(b, n_reads=n, read_len=L, k=case.k, max_index_lookup_frequency=case.max_freq,
                                   also_revcomp=case.revcomp, lut=t)
                _assert_equal(u, want, "uniform")


def rc_uniform_length(case):
    from tests import read_hits_cases as rc
    return rc.uniform_length(case)


def _raw(dev, case, outs, table_bytes=0, k=None, lut=None, bases=None, offsets=None, n_reads=None, rounds=None):
    """kmm_read_nodes through ctypes; outs: five arrays or None each"""
    from kmer_mapper_amd import _lib
    bases = case.bases if bases is None else bases
    offsets = case.offsets if offsets is None else offsets
    n = offsets.shape[0] - 1 if n_reads is None else n_reads
    ptr = lambda a: None if a is None else a.ctypes.data_as(_P)
    code = _lib.lib().kmm_read_nodes(dev._h, ptr(bases), ptr(offsets), n, 0, case.k if k is None else k, case.max_freq,
                                     int(case.revcomp), ptr(case.lut if lut is None else lut), table_bytes, *[ptr(a) for a in outs],
                                     None if rounds is None else ctypes.byref(rounds))
    return code, _lib.lib().kmm_last_error().decode()


def test_every_subset_of_null_outputs(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    case = nc.case("seams_k31")
    want = nc.expected(case)
    n = want.best_node.shape[0]
    with _open(kmm, case.index, monkeypatch) as dev:
        for keep in itertools.product((False, True), repeat=4):
            outs = [np.full(n, 7, np.int32)] + [np.full(n, 7, np.uint32) if on else None for on in keep]
            assert _raw(dev, case, outs)[0] == _lib.KMM_OK
            for a, w in zip(outs, want):
                assert a is None or np.array_equal(a, w), keep


def test_bases_not_aligned_to_16_bytes(kmm, monkeypatch):
    import torch
    case = nc.case("seams_k31")
    with _open(kmm, case.index, monkeypatch) as dev:
        buf = torch.zeros(case.bases.shape[0] + 16, dtype=torch.uint8, device="cuda")
        for shift in (1, 7):
            view = buf[shift:shift + case.bases.shape[0]]
            view.copy_(torch.from_numpy(case.bases))
            got = dev.read_nodes(view, torch.from_numpy(case.offsets).cuda(), k=case.k, max_index_lookup_frequency=case.max_freq)
            _assert_equal(got, nc.expected(case), "shift %d" % shift)


# ---------------------------------------------------------------------------------------------- against the map path
@pytest.mark.parametrize("name", ["seams_k31", "breaks_k31", "revcomp_k16", "filter_k31", "one_node_3000x150_k31", "mixed_3000x150_k31",
                                  "long_read_one_node_k31"])
def test_votes_equal_the_map_path(kmm, monkeypatch, name):
    case = nc.case(name)
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.set_param("path", 1)
        dev.map_reads(case.bases, case.offsets, case.k, case.max_freq, also_revcomp=case.revcomp, lut=case.lut)
        counts = dev.get_node_counts()
        _, n_hits = dev.get_stats()
        got = _call(dev, case)
        assert int(got.total_votes.sum()) == int(counts.sum()) == n_hits > 0
        if (got.n_nodes <= 1).all():                                               # every read on one node at most
            have = got.best_node >= 0
            by_node = np.bincount(got.best_node[have], weights=got.best_votes[have], minlength=counts.shape[0])
            assert np.array_equal(by_node.astype(np.uint32), counts)


# ---------------------------------------------------------------------------------------------- determinism and rounds
def test_three_calls_give_identical_bytes(kmm, monkeypatch):
    case = nc.case("mixed_3000x150_k31")
    with _open(kmm, case.index, monkeypatch) as dev:
        first = _call(dev, case)
        for _ in range(2):
            again = _call(dev, case)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first[:5], again[:5]))


def _greedy_rounds(total_votes, cap):
    """Whole reads, at least one per round, as many as fit `cap` votes"""
    rounds, r, n = 0, 0, total_votes.shape[0]
    while r < n:
        votes, r = int(total_votes[r]), r + 1
        while r < n and votes + int(total_votes[r]) <= cap:
            votes, r = votes + int(total_votes[r]), r + 1
        rounds += 1
    return rounds


@pytest.mark.parametrize("name", ["mixed_3000x150_k31", "one_node_3000x150_k31", "oversize_read_k31", "empty_reads_k31"])
def test_rounds_give_the_single_round_answer(kmm, monkeypatch, name):
    import torch
    case = nc.case(name)
    want = nc.expected(case)
    with _open(kmm, case.index, monkeypatch) as dev:
        one = _call(dev, case)
        assert one.n_rounds == 1
        many = _call(dev, case, table_bytes=nc.MIN_TABLE_BYTES)
        assert many.n_rounds == _greedy_rounds(want.total_votes, nc.MIN_TABLE_BYTES // 32) >= (2 if name == "empty_reads_k31" else 3)
        _assert_equal(many, want, "rounds")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one[:5], many[:5]))
        tiny = _call(dev, case, table_bytes=1)                                      # below the minimum: counts as the minimum
        assert tiny.n_rounds == many.n_rounds
        d = dev.read_nodes(torch.from_numpy(case.bases).cuda(), torch.from_numpy(case.offsets).cuda(), k=case.k,
                           max_index_lookup_frequency=case.max_freq, table_bytes=nc.MIN_TABLE_BYTES)
        assert d.n_rounds == many.n_rounds
        _assert_equal(d, want, "rounds, device arrays")
        L = rc_uniform_length(case)
        if L is not None:
            u = dev.read_nodes(case.bases, n_reads=case.offsets.shape[0] - 1, read_len=L, k=case.k,
                               max_index_lookup_frequency=case.max_freq, table_bytes=nc.MIN_TABLE_BYTES)
            assert u.n_rounds == many.n_rounds
            _assert_equal(u, want, "rounds, uniform")
    if name == "oversize_read_k31":
        assert int(want.total_votes[1]) > nc.MIN_TABLE_BYTES // 32                  # one read alone exceeds the round's votes


# ---------------------------------------------------------------------------------------------- a pure query
def test_the_call_is_a_pure_query(kmm, monkeypatch):
    """Node counts, per-k-mer counts, statistics, "read_hits_calls", pending record-hits entries and a sticky error are as they
    were."""
    from kmer_mapper_amd import _lib
    case, other = nc.case("seams_k31"), nc.case("breaks_k31")
    fastq = b"".join(b"@r%d\n%s\n+\n%s\n" % (r, bytes(case.bases[case.offsets[r]:case.offsets[r + 1]]),
                                             b"I" * int(case.offsets[r + 1] - case.offsets[r])) for r in range(20, 26))
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.count_kmers_mode()
        dev.map_reads(case.bases, case.offsets, 31)
        dev.read_hits(case.bases, case.offsets, k=31)
        dev.record_hits(True)
        dev.map_records(np.frombuffer(fastq, np.uint8), fmt=_lib.FORMAT_FASTQ, k=31)
        dev.record_hits(False)
        counts, kmer_counts, stats = dev.get_node_counts().copy(), dev.get_kmer_counts().copy(), dev.get_stats()
        assert counts.any() and kmer_counts.any() and dev.get_param("record_hits_pending") == 6
        _call(dev, other)
        _assert_equal(_call(dev, case, table_bytes=nc.MIN_TABLE_BYTES), nc.expected(case))
        assert np.array_equal(dev.get_node_counts(), counts) and np.array_equal(dev.get_kmer_counts(), kmer_counts)
        assert dev.get_stats() == stats
        assert dev.get_param("read_hits_calls") == 1 and dev.get_param("record_hits_pending") == 6
        assert dev.take_record_hits().shape == (6,)
        # a sticky error stays where it is: the query is served behind it, and the handle reports it afterwards as before
        bad = case.bases.copy()
        bad[100] = ord("X")
        dev.map_reads(bad, case.offsets, 31)
        with pytest.raises(ValueError, match="offset 100 "):
            dev.get_node_counts()
        _assert_equal(_call(dev, case), nc.expected(case), "behind a sticky error")
        with pytest.raises(ValueError, match="offset 100 "):
            dev.get_node_counts()
        dev.reset()


def test_works_on_indexes_without_a_radix_view(kmm, monkeypatch):
    import types
    big = nc.case("modulo_257_k31")
    index = nc.block_index(31)
    h2i, nk = np.asarray(index._hashes_to_index).copy(), np.asarray(index._n_kmers).copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo, max_node_id=index.max_node_id)
    with _open(kmm, dup, monkeypatch) as dev:
        assert dev.get_param("radix_available") == 0
        got = dev.read_nodes(big.bases, big.offsets, k=31, max_index_lookup_frequency=nc.NO_FILTER)
        want = [nc.answer(nc.tally_read(dup, big.bases[big.offsets[r]:big.offsets[r + 1]], 31)[0]) for r in range(big.offsets.shape[0] - 1)]
        assert [tuple(int(a[r]) for a in got[:5]) for r in range(len(want))] == want and (got.best_node >= 0).any()


# ---------------------------------------------------------------------------------------------- errors
def test_errors_come_from_the_call_and_leave_the_handle_alone(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    from kmer_mapper_amd.util import ambiguous_skip_lut
    case = nc.case("seams_k31")
    n = case.offsets.shape[0] - 1
    outs = lambda: [np.zeros(n, np.int32)] + [np.zeros(n, np.uint32) for _ in range(4)]
    with _open(kmm, case.index, monkeypatch) as dev:
        dev.map_reads(case.bases, case.offsets, 31)
        counts = dev.get_node_counts().copy()

        def good():
            got = outs()
            assert _raw(dev, case, got)[0] == _lib.KMM_OK
            assert all(np.array_equal(a, w) for a, w in zip(got, nc.expected(case)))

        bad = case.bases.copy()
        bad[2051] = ord("X")
        bad[3000] = ord("-")
        code, msg = _raw(dev, case, outs(), bases=bad)
        assert code == _lib.KMM_ERR_INVALID_BASE and "offset 2051 " in msg
        assert np.array_equal(dev.get_node_counts(), counts)                        # no sticky error, nothing counted
        good()
        down = case.offsets.copy()
        down[5], down[6] = down[6], down[5]
        code, msg = _raw(dev, case, outs(), offsets=down)
        assert code == _lib.KMM_ERR_INVALID_ARG and "not non-decreasing at read 5" in msg
        good()
        first = case.offsets.copy()
        first[0] = 1
        assert _raw(dev, case, outs(), offsets=first)[0] == _lib.KMM_ERR_INVALID_ARG
        good()
        assert _raw(dev, case, [None] + outs()[1:])[0] == _lib.KMM_ERR_INVALID_ARG  # best_node == NULL
        good()
        for k in (0, 32):
            assert _raw(dev, case, outs(), k=k)[0] == _lib.KMM_ERR_INVALID_ARG
        good()
        assert _raw(dev, case, outs(), k=1, lut=ambiguous_skip_lut())[0] == _lib.KMM_ERR_INVALID_ARG
        good()
        code, msg = _raw(dev, case, outs(), table_bytes=-1)
        assert code == _lib.KMM_ERR_INVALID_ARG and "table_bytes" in msg
        good()
        with pytest.raises(ValueError, match="offset 2051 "):
            dev.read_nodes(bad, case.offsets)
        assert np.array_equal(dev.get_node_counts(), counts)


def test_nothing_to_look_up_is_accepted(kmm, monkeypatch):
    import torch
    from kmer_mapper_amd import _lib
    case = nc.case("seams_k31")
    with _open(kmm, case.index, monkeypatch) as dev:
        rounds = ctypes.c_int64(5)
        assert _raw(dev, case, [None] * 5, n_reads=0, rounds=rounds)[0] == _lib.KMM_OK and rounds.value == 0
        assert dev.read_nodes(np.zeros(0, np.uint8), np.zeros(1, np.int64)).best_node.shape == (0,)
        outs = [np.full(5, 7, np.int32)] + [np.full(5, 7, np.uint32) for _ in range(4)]
        assert _raw(dev, case, outs, bases=np.zeros(0, np.uint8), offsets=np.zeros(6, np.int64))[0] == _lib.KMM_OK
        assert (outs[0] == -1).all() and not any(a.any() for a in outs[1:])
        got = dev.read_nodes(np.zeros(0, np.uint8), n_reads=4, read_len=0)
        assert (got.best_node == -1).all() and got.best_node.shape == (4,) and not got.total_votes.any() and got.n_rounds == 0
        got = dev.read_nodes(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(6, dtype=torch.int64, device="cuda"))
        assert got.best_node.is_cuda and (got.best_node.cpu().numpy() == -1).all() and not got.best_votes.cpu().numpy().any()


# ---------------------------------------------------------------------------------------------- façade and command line
def test_mapper_facade_opens_and_closes_a_handle(kmm):
    from kmer_mapper_amd import mapper
    case = nc.case("ties_k31")
    before = len(mapper._CACHE)
    got = mapper.read_nodes(case.index, (case.bases, case.offsets), k=31, max_index_lookup_frequency=case.max_freq)
    _assert_equal(got, nc.expected(case))
    assert len(mapper._CACHE) == before


@pytest.mark.parametrize("gz", [False, True], ids=["fastq", "fastq_gz"])
def test_command_line_from_index_to_assign_reads(kmm, tmp_path, gz):
    """`index` on three short sequences that share one 60-base stretch, `assign-reads` on reads cut from them."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    from tests import read_hits_cases as rc
    k = 21
    shared = rc.gslice(8000, 60)
    seqs = [np.concatenate([rc.gslice(1000 * (i + 1), 300), shared, rc.gslice(1000 * (i + 1) + 400, 300)]) for i in range(3)]
    fa = tmp_path / "refs.fa"
    fa.write_bytes(b"".join(b">seq%d some text\n%s\n" % (i, bytes(s)) for i, s in enumerate(seqs)))
    npz, names = str(tmp_path / "index.npz"), str(tmp_path / "names.txt")
    run_argument_parser(["index", "-f", str(fa), "-k", str(k), "-o", npz, "--names-output", names])
    reads, source = [], []
    for i, s in enumerate((1, 2, 0, 2, 1, 0)):                                      # reads of their source alone
        reads.append(seqs[s][20 + 30 * i:20 + 30 * i + 100])
        source.append(s)
    reads += [shared[5:55], shared]                                                 # reads from the shared stretch: a three-way tie
    source += [0, 0]
    reads.append(rc.random_read(80, 1))                                             # a read of none of them
    source.append(-1)
    bases, offsets = rc.batch(reads)
    fq = str(tmp_path / ("reads.fq.gz" if gz else "reads.fq"))
    reads_io.write_fastq(fq, ReadBatch(bases, offsets), gz=gz)
    if gz:
        with gzip.open(fq, "rb") as f:
            assert f.read(1) == b"@"
    out, summary = str(tmp_path / "out"), str(tmp_path / "summary.tsv")
    got = run_argument_parser(["assign-reads", "-i", npz, "-f", fq, "-k", str(k), "-o", out, "-c", "300", "--names", names,
                               "--summary", summary])
    assert np.array_equal(got, source) and np.array_equal(np.load(out + ".npy"), source) and np.load(out + ".npy").dtype == np.int32
    best, second, total = (np.load(out + ".%s_votes.npy" % w) for w in ("best", "second", "total"))
    assert best.dtype == np.uint32 and (best[:6] == 100 - k + 1).all() and (second[:6] == 0).all()
    assert best[6] == second[6] == 50 - k + 1 and total[6] == 3 * best[6] and best[8] == 0
    lines = [ln.split("\t") for ln in open(summary).read().splitlines()]
    assert lines[0] == ["node", "name", "reads", "share"]
    assert [ln[0] for ln in lines[1:]] == ["0", "1", "2", "-1"] and [int(ln[2]) for ln in lines[1:]] == [4, 2, 2, 1]
    assert [ln[1] for ln in lines[1:4]] == open(names).read().splitlines()[:3] and lines[4][1] == "unassigned"
    assert all("seq%d" % i in lines[1 + i][1] for i in range(3))
    margin = run_argument_parser(["assign-reads", "-i", npz, "-f", fq, "-k", str(k), "-o", out, "--min-margin", "1"])
    assert np.array_equal(margin, source[:6] + [-1, -1, -1])
    votes = run_argument_parser(["assign-reads", "-i", npz, "-f", fq, "-k", str(k), "-o", out, "--min-votes", "31"])
    assert np.array_equal(votes, source[:6] + [-1, 0, -1])
