"""GPU tier of the skew suite: the radix path (csrc/kmm_radix.hpp) on the batches of tests/skew_cases.py — one k-mer
twelve million times, 99 % poly-A beside cold partitions, tandem repeats, duplicates, sorted hashes, one bucket, one slice,
the ends of the hash range, a Zipf draw — with a forced geometry of 391 coarse partitions, so that one partition holds
(nearly) everything and the others (nearly) nothing.  Counts are bit-exact against the oracle (mapper.pyx:53-69), the three
conservation counters and the item total of skew_cases.geometry must hold, no case may pass by taking the direct path,
and the direct kernels then map the same batch on the same handle.  tests/test_skew_cases_on_the_cpu.py proves on the CPU
that every case reaches the partition shapes it exists for.

Small scale first (`-k small`); no case is skipped or left out at run time."""
import numpy as np
import pytest

from tests import skew_cases as sk

pytestmark = pytest.mark.gpu

CASE_PARAMS = [pytest.param(name, scale, id="%s-%s" % (name, scale)) for scale in sk.SCALES for name in sk.CASES]
KNOB_PARAMS = [pytest.param(name, scale, id="%s-%s" % (name, scale))
               for scale in sk.SCALES for name in ("one_kmer-three_nodes", "hot_and_cold")]
PER_KMER_PARAMS = [pytest.param(name, scale, id="%s-%s" % (name, scale))
                   for scale in sk.SCALES for name in ("one_kmer-three_nodes", "duplicates-one_read", "zipf")]


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _force(dev, c, g, radix_filter=1):
    """The case's geometry, in the order the knobs depend on each other (radix_filter re-derives the fan-out, fine_bits
    overrides it); a refused or altered geometry fails the test."""
    dev.set_param("part_shift", c.w)
    dev.set_param("radix_filter", radix_filter)
    dev.set_param("fine_bits", c.f2)
    dev.set_param("path", 2)
    got = tuple(dev.get_param(n) for n in ("part_shift", "n_partitions", "n_coarse_partitions", "n_fine_per_coarse", "radix_filter"))
    assert got == (c.w, g.PF, g.F1, g.F2, radix_filter)
    assert g.F1 >= 64


def _radix(dev, run, expect, n_lookups, n_items=None, what=None):
    """One call on the radix path from a clean handle: the oracle's counts, conservation through the passes, the path
    taken, and (one sub-batch) the items pass 1's directory defines."""
    dev.reset()
    dev.get_stats(reset=True)
    rb, db = dev.get_param("radix_batches"), dev.get_param("direct_batches")
    run()
    got = dev.get_node_counts()
    assert got.dtype == np.uint32 and np.array_equal(got, expect), what
    p2, p3, dropped = (dev.get_param(n) for n in ("radix_p2_kmers", "radix_p3_kmers", "radix_p2_dropped"))
    assert (p2, p3 + dropped) == (n_lookups, n_lookups), (what, p2, p3, dropped, dev.get_param("debug_rx_t1_sum"),
                                                          dev.get_param("debug_rx_start1_sum"))
    assert dev.get_stats(reset=True) == (n_lookups, int(expect.sum(dtype=np.uint64))), what
    assert dev.get_param("radix_batches") > rb and dev.get_param("direct_batches") == db, what
    if n_items is not None:
        assert dev.get_param("debug_rx_items") == n_items, what
    return dropped


def _direct(dev, run, expect, what=None):
    dev.set_param("path", 1)
    dev.reset()
    rb, db = dev.get_param("radix_batches"), dev.get_param("direct_batches")
    run()
    assert np.array_equal(dev.get_node_counts(), expect), what
    assert dev.get_param("radix_batches") == rb and dev.get_param("direct_batches") > db, what
    dev.set_param("path", 2)


def _device(a):
    import torch
    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()      # (torch's copy runs on torch's stream, the map call on the handle's)
    return t


def _read_front_ends(dev, oracle, c, bases, mf, expect, n, n_items, tag):
    """Every way reads reach pass 1: whole-read and position tiles, from host memory packed by the host threads, staged as
    they are, from a device tensor; ragged reads with offsets; raw FASTQ compacted on the device and by the host threads."""
    from kmer_mapper_amd import _lib
    R, L, k, rc = c.n_reads, c.read_len, c.k, c.revcomp
    uniform = lambda src: (lambda: dev.map_reads_uniform(src, R, L, k, mf, also_revcomp=rc))
    on_device = _device(bases)
    for packed in (1, 0):
        dev.set_param("radix_packed_tiles", packed)
        dev.set_param("host_pack_threads", 3)
        before = dev.get_param("host_packed_calls")
        _radix(dev, uniform(bases), expect, n, n_items, (tag, "uniform, host-packed", packed))
        assert dev.get_param("host_packed_calls") == before + 1, (tag, packed)
        dev.set_param("host_pack_threads", 0)
        _radix(dev, uniform(bases), expect, n, n_items, (tag, "uniform, staged", packed))
        _radix(dev, uniform(on_device), expect, n, n_items, (tag, "uniform, device tensor", packed))
    dev.set_param("radix_packed_tiles", 1)
    # the same content cut into reads of 0..400 bases
    offs = sk.ragged_offsets(bases.shape[0], 7)
    e_ragged, n_ragged = oracle.map_reads(c.index, c.max_node_id, bases, offs, k, mf, also_revcomp=rc, n_threads=16)
    n_ragged *= 2 if rc else 1
    for threads in (3, 0):
        dev.set_param("host_pack_threads", threads)
        _radix(dev, lambda: dev.map_reads(bases, offs, k, mf, also_revcomp=rc), e_ragged, n_ragged, None, (tag, "ragged", threads))
    raw = sk.fastq(bases, R, L)
    for threads in (0, 3):
        dev.set_param("host_pack_threads", threads)
        seen = []
        _radix(dev, lambda: seen.append(dev.map_records(raw, fmt=_lib.FORMAT_FASTQ, k=k, max_index_lookup_frequency=mf, also_revcomp=rc)),
               expect, n, None, (tag, "FASTQ", threads))      # (a chunk of records may be mapped in pieces)
        assert seen == [(raw.shape[0], R)], (tag, threads)
    dev.set_param("host_pack_threads", 0)


@pytest.mark.parametrize("name, scale", CASE_PARAMS)
def test_radix_equals_oracle_on_skewed_batches(kmm, oracle, name, scale):
    c = sk.build(name, scale)
    q = sk.lookups(c, oracle.extract)
    g = sk.geometry(q, c.index._modulo, c.w, c.f2)
    n = q.shape[0]
    own = q[:n // 2] if c.revcomp else q                     # (the library derives the reverse complements itself)
    with kmm.DeviceIndex.from_index(c.index, c.max_node_id) as dev:
        _force(dev, c, g)
        for mf in c.max_freqs:
            expect = oracle.map_kmers(c.index, c.max_node_id, q, mf)
            kmers = lambda: dev.map_kmers(own, mf, also_revcomp=c.revcomp, k=c.k)
            dropped = _radix(dev, kmers, expect, n, g.n_items, (c.id, mf, "map_kmers"))
            if name == "one_kmer-absent":
                assert dropped == n and not expect.any()      # its bucket is empty: pass 2 drops the whole batch
            if name.startswith("one_kmer") or name == "edges-kmer_last_hash":
                assert dropped in (0, n)
            if c.bases is not None:
                _read_front_ends(dev, oracle, c, c.bases, mf, expect, n, g.n_items, (c.id, mf, "reads"))
                if c.bases_n is not None:
                    _read_front_ends(dev, oracle, c, c.bases_n, mf, expect, n, g.n_items, (c.id, mf, "reads with N"))
            _direct(dev, kmers, expect, (c.id, mf, "direct"))
            if c.bases is not None:
                _direct(dev, lambda: dev.map_reads_uniform(c.bases, c.n_reads, c.read_len, c.k, mf, also_revcomp=c.revcomp),
                        expect, (c.id, mf, "direct, reads"))


@pytest.mark.parametrize("name, scale", KNOB_PARAMS)
def test_knobs_change_no_result_on_skewed_batches(kmm, oracle, name, scale):
    """The plain and the filtering pass 2, both flush orders, one and two workgroups per CU, sub-batches that cut the hot
    partition every 4 blocks and every 5 blocks + 17 k-mers, and slices of 8192 buckets: the oracle's counts."""
    c = sk.build(name, scale)
    q = sk.lookups(c, oracle.extract)
    g = sk.geometry(q, c.index._modulo, c.w, c.f2)
    n = q.shape[0]
    expect = oracle.map_kmers(c.index, c.max_node_id, q)
    with kmm.DeviceIndex.from_index(c.index, c.max_node_id) as dev:
        on_device = _device(c.bases)
        reads = lambda: dev.map_reads_uniform(on_device, c.n_reads, c.read_len, c.k)
        kmers = lambda: dev.map_kmers(q, k=c.k)
        for radix_filter in (0, 1):
            _force(dev, c, g, radix_filter)
            for flush in (0, 1):
                dev.set_param("radix_sorted_flush", flush)
                for grid in (1, 2):
                    dev.set_param("radix_grid_per_cu", grid)
                    what = (c.id, "filter", radix_filter, "sorted flush", flush, "grid", grid)
                    _radix(dev, reads, expect, n, g.n_items, what)
                    _radix(dev, kmers, expect, n, g.n_items, what)
            dev.set_param("radix_grid_per_cu", 1)
            default_cap = dev.get_param("radix_sub_batch_kmers")
            for cap in (4 * 8192, 5 * 8192 + 17):
                dev.set_param("radix_sub_batch_kmers", cap)
                assert dev.get_param("radix_sub_batch_kmers") == cap
                for packed in (1, 0):
                    dev.set_param("radix_packed_tiles", packed)
                    _radix(dev, reads, expect, n, None, (c.id, "filter", radix_filter, "cap", cap, "packed", packed))
                dev.set_param("radix_packed_tiles", 1)
                _radix(dev, kmers, expect, n, None, (c.id, "filter", radix_filter, "cap", cap, "k-mers"))
            dev.set_param("radix_sub_batch_kmers", default_cap)
    # slices of 8192 buckets, on an index built for them (modulo 40 009: five slices, as test_slices_of_8192_buckets)
    base = name.partition("-")[0]
    c13 = getattr(sk, base)(scale, slices13=True)
    q = sk.lookups(c13, oracle.extract)                      # (its ordinary reads come from its own genome)
    n = q.shape[0]
    e13 = oracle.map_kmers(c13.index, c13.max_node_id, q)
    with kmm.DeviceIndex.from_index(c13.index, c13.max_node_id) as dev:
        for radix_filter in (0, 1):
            dev.set_param("part_shift", 13)
            dev.set_param("radix_filter", radix_filter)
            dev.set_param("path", 2)
            assert (dev.get_param("part_shift"), dev.get_param("n_partitions")) == (13, 5)
            _radix(dev, lambda: dev.map_reads_uniform(c13.bases, c13.n_reads, c13.read_len, c13.k), e13, n, None, (c.id, "8192-bucket slices", radix_filter))
            _radix(dev, lambda: dev.map_kmers(q, k=c13.k), e13, n, None, (c.id, "8192-bucket slices, k-mers", radix_filter))


@pytest.mark.parametrize("name, scale", PER_KMER_PARAMS)
def test_per_kmer_counts_on_skewed_batches(kmm, oracle, name, scale):
    """Per-k-mer mode (GpuCounter semantics, gpu_counter.py:23-37): a count per index entry, in the order the entries were
    given — at full scale one entry of one_kmer holds 12 M — and node counts that are their sum per node."""
    c = sk.build(name, scale)
    q = sk.lookups(c, oracle.extract)
    g = sk.geometry(q, c.index._modulo, c.w, c.f2)
    per_entry = sk.numpy_entry_counts(c.index._kmers, q)
    if name.startswith("one_kmer"):
        assert per_entry.max() == q.shape[0] and (per_entry > 0).sum() == 3
    with kmm.DeviceIndex.from_index(c.index, c.max_node_id) as dev:
        _force(dev, c, g)
        dev.count_kmers_mode(True)
        assert dev.get_param("count_kmers") == 1
        dev.map_kmers(q, 65535, k=c.k)
        got = dev.get_kmer_counts()
        assert got.dtype == np.uint32 and np.array_equal(got, per_entry)
        half = np.ascontiguousarray(q[:q.shape[0] // 2])               # a second call adds to the same entries
        dev.map_kmers(half, 65535, k=c.k)
        per_entry = per_entry + sk.numpy_entry_counts(c.index._kmers, half)
        per_node = np.bincount(c.index._nodes, per_entry.astype(np.float64), minlength=c.max_node_id + 1)
        assert np.array_equal(dev.get_kmer_counts(), per_entry)
        assert np.array_equal(dev.get_node_counts().astype(np.float64), per_node % 2.0 ** 32)
        assert np.array_equal(dev.get_kmer_counts(), per_entry)          # reading the node counts does not clear them


@pytest.mark.parametrize("scale", sk.SCALES)
def test_counts_wrap_around_on_the_radix_path(kmm, oracle, scale):
    """A caller's count tensor that starts at 0xFFFFFF00: the radix path's flush adds modulo 2^32 like the reference's
    uint32 vector (mapper.pyx:37,68)."""
    import torch
    c = sk.build("one_kmer-three_nodes", scale)
    q = sk.lookups(c, oracle.extract)
    g = sk.geometry(q, c.index._modulo, c.w, c.f2)
    expect = oracle.map_kmers(c.index, c.max_node_id, q)
    init = 0xFFFFFF00
    want = ((np.uint64(init) + expect.astype(np.uint64)) % np.uint64(1 << 32)).astype(np.uint32)
    assert want[11] == (init + q.shape[0]) % (1 << 32) < init and want[0] == init
    counts = torch.full((c.max_node_id + 1,), init - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with kmm.DeviceIndex.from_index(c.index, c.max_node_id) as dev:
        _force(dev, c, g)
        dev.bind_counts(counts)
        rb, db = dev.get_param("radix_batches"), dev.get_param("direct_batches")
        dev.map_reads_uniform(c.bases, c.n_reads, c.read_len, c.k)
        dev.synchronize()
        assert dev.get_param("radix_batches") > rb and dev.get_param("direct_batches") == db
        assert np.array_equal(counts.cpu().numpy().view(np.uint32), want)
        dev.bind_counts(None)


@pytest.mark.parametrize("scale", sk.SCALES)
def test_counts_accumulate_across_skewed_calls_without_a_flush(kmm, oracle, scale):
    """one_kmer three times, then hot_and_cold, and only then a synchronising call: the hot entry's count stays pending in
    the per-entry vector across the calls and the node counts are the sum."""
    a, b = sk.build("one_kmer-three_nodes", scale), sk.build("hot_and_cold", scale)
    qa, qb = sk.lookups(a, oracle.extract), sk.lookups(b, oracle.extract)
    g = sk.geometry(qb, b.index._modulo, b.w, b.f2)
    want = 3 * oracle.map_kmers(b.index, b.max_node_id, qa).astype(np.uint64) + oracle.map_kmers(b.index, b.max_node_id, qb)
    assert want[11] >= 3 * qa.shape[0] + int((qb == 0).sum())
    with kmm.DeviceIndex.from_index(b.index, b.max_node_id) as dev:
        _force(dev, b, g)
        dev.get_stats(reset=True)
        a_dev = _device(a.bases)
        dev.map_kmers(qa, k=a.k)
        dev.map_reads_uniform(a.bases, a.n_reads, a.read_len, a.k)
        dev.map_reads_uniform(a_dev, a.n_reads, a.read_len, a.k)
        dev.map_reads_uniform(b.bases, b.n_reads, b.read_len, b.k)
        got = dev.get_node_counts()
        assert np.array_equal(got, (want % np.uint64(1 << 32)).astype(np.uint32))
        assert dev.get_param("radix_batches") >= 4 and dev.get_param("direct_batches") == 0
        assert dev.get_stats() == (3 * qa.shape[0] + qb.shape[0], int(want.sum()))
