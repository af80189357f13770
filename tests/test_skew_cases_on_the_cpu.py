"""CPU tier of the skew suite (tests/skew_cases.py): every batch is deterministic, reaches — by skew_cases.geometry, which
restates kmm_radix.hpp:14-29 in numpy and knows nothing of the kernels — the partition shapes it exists for, and has one
answer on which the C oracle (map_reads with 1 and 16 threads, map_kmers on the extracted k-mers) and the numpy mapper
agree.  A case that does not reach its condition fails here, before anyone spends GPU time on it.

All comparisons run at FULL scale: np.unique on the 60 M k-mers of hot_and_cold takes about a second because nearly all of
them are equal, the oracle 0.2-0.5 s.  Run with -s to get the geometry figures (profiles/skew/README.md has them)."""
import functools
import time

import numpy as np
import pytest

from tests import skew_cases as sk

F1 = 391           # coarse partitions of the forced geometry: modulo 100 003, 16 buckets per slice, 16 slices per partition


@functools.lru_cache(maxsize=None)
def case(name, scale):
    return sk.build(name, scale)


def _geometry(c, oracle, by_position=False):
    q = sk.lookups(c, oracle.extract)
    pos = sk.read_positions(c.n_reads, c.read_len, c.k) if by_position else None
    g = sk.geometry(q, c.index._modulo, c.w, c.f2, pos)
    hot = int(np.argmax(g.T1))
    print("\n%-28s %s k-mers %d blocks %d | non-empty partitions %d of %d | hottest: share %.4f items %d rows %d | items %d | "
          "longest run %d (%d sub-runs), %d whole-block runs | blocks per item: max %d, hot partition max %d"
          % (c.id, "positions" if by_position else "k-mer order", g.n_kmers, g.n_blocks, int((g.T1 > 0).sum()), g.F1, g.hot_share,
             g.items[hot], g.rows[hot], g.n_items, g.max_run, -(-g.max_run // sk.SUB_RUN), g.whole_block_runs,
             int(g.item_blocks.max()), int(g.item_blocks[g.item_part == hot].max())))
    assert (g.PF, g.F1, g.F2) == (6251, F1, 16) and g.F1 >= 64 and max(g.F1, g.F2) <= 512
    assert int(g.T1.sum()) == q.shape[0] and g.n_items == int(g.items.sum())
    return g, q, hot


@pytest.mark.parametrize("scale", sk.SCALES)
@pytest.mark.parametrize("name", sk.CASES)
def test_cases_are_deterministic_and_sized(name, scale):
    a, b = sk.build(name, scale), sk.build(name, scale)
    for field in ("kmers", "bases", "bases_n"):
        x, y = getattr(a, field), getattr(b, field)
        assert (x is None) == (y is None) and (x is None or (x.dtype == y.dtype and np.array_equal(x, y))), field
    for field in ("_hashes_to_index", "_n_kmers", "_nodes", "_kmers", "_frequencies"):
        assert np.array_equal(getattr(a.index, field), getattr(b.index, field)), field
    assert (a.max_node_id, a.k, a.w, a.f2, a.revcomp, a.max_freqs) == (b.max_node_id, b.k, b.w, b.f2, b.revcomp, b.max_freqs)
    assert (a.kmers is None) != (a.bases is None)
    assert (a.name in sk.READ_SHAPED) == (a.bases is not None)
    n = a.kmers.shape[0] if a.kmers is not None else a.n_reads * (a.read_len - a.k + 1)
    if a.bases is not None:
        assert a.bases.shape[0] == a.n_reads * a.read_len
    if scale == "small":
        assert n <= 1_000_000
    assert a.max_node_id == a.index.max_node_id()


def test_tools(oracle):
    """revcomp_kmers against the oracle's, ragged_offsets and fastq against their definitions."""
    q = np.random.default_rng(1).integers(0, 1 << 62, size=200, dtype=np.uint64)
    assert np.array_equal(sk.revcomp_kmers(q, 31), oracle.revcomp(q, 31))
    assert int(sk.revcomp_kmers(np.zeros(1, np.uint64), 31)[0]) == 4 ** 31 - 1
    offs = sk.ragged_offsets(150 * 8000, 5)
    lens = np.diff(offs)
    assert offs[0] == 0 and offs[-1] == 150 * 8000 and lens.min() >= 0 and lens.max() <= 400 and (lens == 0).any() and (lens > 300).any()
    raw = sk.fastq(np.frombuffer(b"ACGTTGCA", dtype=np.uint8), 2, 4).tobytes()
    assert raw == b"@r\nACGT\n+\nIIII\n@r\nTGCA\n+\nIIII\n"


# ------------------------------------------------------------------- the right-hand column of the issue's table, at full scale
@pytest.mark.parametrize("name", ["one_kmer-three_nodes", "one_kmer-absent", "one_kmer-freq5"])
def test_one_kmer_is_one_partition_of_1465_items_in_two_rows(oracle, name):
    c = case(name, "full")
    g, q, hot = _geometry(c, oracle)
    assert q.shape[0] == 12_000_000 and not q.any()
    assert hot == 0 and g.T1[0] == 12_000_000 and (g.T1 > 0).sum() == 1          # all other partitions empty
    assert g.items[0] == 1465 and g.rows[0] == 2 and g.n_items == 1465
    assert g.n_blocks == 1465 and g.whole_block_runs == 1464 and g.max_run == 8192   # every run a whole block (but the last)
    assert g.max_run // sk.SUB_RUN == 512                                        # sub-runs of one run: a window holds 2 (6) runs
    gp, _, _ = _geometry(c, oracle, by_position=True)                            # position tiles: 15 M positions
    assert gp.n_blocks == 1832 and gp.items[0] == 1465 and gp.max_run >= 6500


def test_one_kmer_revcomp_is_two_hot_partitions(oracle):
    c = case("one_kmer_revcomp", "full")
    g, q, hot = _geometry(c, oracle)
    t = int(sk.POLY_T % np.uint64(c.index._modulo)) >> 8
    assert t != 0 and sorted(np.flatnonzero(g.T1)) == [0, t]
    assert g.T1[0] == g.T1[t] == 12_000_000 and g.items[0] == g.items[t] == 1465 and g.rows[0] == g.rows[t] == 2


def test_hot_and_cold_has_a_partition_of_8_rows_and_cold_items_across_all_blocks(oracle):
    c = case("hot_and_cold", "full")
    g, q, hot = _geometry(c, oracle, by_position=True)
    assert q.shape[0] == 60_000_000 and g.n_blocks == 9156
    assert hot == 0 and g.hot_share >= 0.99                    # 495 000 of 500 000 reads are poly-A
    assert 7251 <= g.items[0] <= 7253 and g.rows[0] == 8       # 59.4 M k-mers + partition 0's share of the ordinary ones
    cold = np.delete(g.T1, 0)
    assert (cold > 0).all() and 200 <= cold.min() and cold.max() <= 5000         # 600 000 ordinary k-mers over 390 partitions
    assert (np.delete(g.items, 0) == 1).all()
    spans = g.item_blocks[g.item_part != 0]
    assert spans.min() > 512 and spans.max() >= 9000           # one item per cold partition, its runs in (nearly) every block
    assert g.item_blocks[g.item_part == 0].max() <= 3          # the hot items: one block and a half each


def test_tandem_is_a_handful_of_hot_partitions(oracle):
    c = case("tandem", "full")
    g, q, hot = _geometry(c, oracle)
    assert q.shape[0] == 24_000_000 and c.distinct.shape[0] == 32
    assert np.array_equal(np.unique(q), c.distinct)
    n_hot = int((g.T1 > 0).sum())
    assert 8 <= n_hot <= 32 and g.items[g.T1 > 0].min() >= 40  # period 6: 24 M / 10 units / 6 phases = 400 000 k-mers = 49 items
    # equal keys in lane-periodic order: inside a read, k-mer i equals k-mer i + period
    rd = q[:120 * 1000].reshape(1000, 120)
    assert all((rd[:, :-p] == rd[:, p:]).all(axis=1).any() for p in (1, 2, 3, 4, 6))
    assert np.isin(c.distinct[::2], c.index._kmers).all() and not np.isin(c.distinct[1::2], c.index._kmers).any()


@pytest.mark.parametrize("name, distinct_lo, distinct_hi", [("duplicates-one_read", 120, 120), ("duplicates-300_reads", 30_000, 36_000)])
def test_duplicates_are_few_distinct_kmers_that_all_hit(oracle, name, distinct_lo, distinct_hi):
    c = case(name, "full")
    g, q, hot = _geometry(c, oracle)
    assert q.shape[0] == 9_600_000
    assert distinct_lo <= np.unique(q).shape[0] <= distinct_hi       # (300 reads of a 200 000-base genome overlap here and there)
    assert np.isin(q[:120 * 300], c.index._kmers).all()               # hit rate 1
    assert g.n_items >= 9_600_000 // 8192


@pytest.mark.parametrize("name", ["sorted_hashes-ascending", "sorted_hashes-descending"])
def test_sorted_hashes_keep_every_block_inside_two_partitions(oracle, name):
    c = case(name, "full")
    g, q, hot = _geometry(c, oracle)
    h = (q % np.uint64(c.index._modulo)).astype(np.int64)
    d = np.diff(h)
    assert (d >= 0).all() if name.endswith("ascending") else (d <= 0).all()
    assert g.parts_per_block_max == 2 and (g.T1 > 8192).all()         # 8 M / 391 = 20 000 k-mers per partition: 2.5 blocks
    assert (g.T1 % 8192 != 0).all() and g.item_blocks.max() <= 3      # items cut inside runs; an item = parts of at most 3 blocks
    assert (g.items >= 2).all()


def test_one_bucket_is_one_directory_slot(oracle):
    c = case("one_bucket", "full")
    g, q, hot = _geometry(c, oracle)
    M = np.uint64(c.index._modulo)
    assert np.unique(q % M).tolist() == [sk.ONE_BUCKET_HASH] and np.unique(q).shape[0] == 2 * sk.ONE_BUCKET_ENTRIES
    in_bucket = int(c.index._n_kmers[sk.ONE_BUCKET_HASH])
    assert sk.ONE_BUCKET_ENTRIES <= in_bucket <= 256
    assert (g.T1 > 0).sum() == 1 and g.items[hot] == -(-3_000_000 // 8192) == 367
    assert 0.45 < np.isin(q, c.index._kmers).mean() < 0.55


@pytest.mark.parametrize("name, fine, n_buckets", [("one_slice", 3000, 16), ("edges-slice_first", 0, 16), ("edges-slice_last", 6250, 3)])
def test_one_slice_is_one_fine_partition(oracle, name, fine, n_buckets):
    c = case(name, "full")
    g, q, hot = _geometry(c, oracle)
    h = q % np.uint64(c.index._modulo)
    assert np.unique(h >> np.uint64(4)).tolist() == [fine] and np.unique(h).shape[0] == n_buckets
    assert hot == fine >> 4 and (g.T1 > 0).sum() == 1 and g.items[hot] == -(-4_000_000 // 8192) == 489
    assert g.whole_block_runs == 488                                   # pass-2 items: one full run, F2 - 1 empty ones
    if name == "edges-slice_last":
        assert hot == F1 - 1 and g.PF - (F1 - 1) * 16 == 11 and int(h.max()) == c.index._modulo - 1   # short last partition, clipped slice
    assert 0.3 < np.isin(q, c.index._kmers).mean() < 0.37


def test_edges_last_hash_is_the_short_last_partition(oracle):
    c = case("edges-kmer_last_hash", "full")
    g, q, hot = _geometry(c, oracle)
    assert np.unique(q % np.uint64(c.index._modulo)).tolist() == [c.index._modulo - 1]
    assert hot == F1 - 1 and (g.T1 > 0).sum() == 1 and g.items[hot] == 1465 and g.rows[hot] == 2


def test_zipf_is_mild_skew_over_every_partition(oracle):
    c = case("zipf", "full")
    g, q, hot = _geometry(c, oracle)
    assert (g.T1 > 0).all()
    # the first rank alone draws 0.8 / H(50 000) = 7 % of the batch; the uniform share of a partition is 0.26 %
    assert 0.05 <= g.hot_share <= 0.5 and g.rows.max() == 1 and g.items.max() >= 50
    assert np.median(g.T1) < 0.005 * q.shape[0]
    counts = np.bincount(c.index._nodes)
    assert counts.shape[0] == 1000 and counts.min() >= 40              # the `skewed` node model: hot nodes


# ------------------------------------------------------------------- one answer from three mappers
@pytest.mark.parametrize("name", sk.CASES)
def test_oracle_and_numpy_mapper_agree_at_full_scale(oracle, name):
    c = case(name, "full")
    q = sk.lookups(c, oracle.extract)
    for mf in c.max_freqs:
        t0 = time.perf_counter()
        by_kmers = oracle.map_kmers(c.index, c.max_node_id, q, mf)
        t_oracle = time.perf_counter() - t0
        t0 = time.perf_counter()
        by_numpy = sk.numpy_map_kmers(c.index, c.max_node_id, q, mf)
        t_numpy = time.perf_counter() - t0
        print("\n%-28s max_freq %d: %d lookups, %d increments, oracle %.2f s, numpy %.2f s" % (c.id, mf, q.shape[0], int(by_kmers.sum(dtype=np.uint64)), t_oracle, t_numpy))
        assert by_kmers.dtype == by_numpy.dtype == np.uint32 and np.array_equal(by_kmers, by_numpy)
        if c.bases is not None:
            offs = np.arange(c.n_reads + 1, dtype=np.int64) * c.read_len
            for bases in (c.bases, c.bases_n):
                if bases is None:
                    continue
                for threads in (1, 16):                     # 16: a hot node under the oracle's own threaded reduce
                    got, n = oracle.map_reads(c.index, c.max_node_id, bases, offs, c.k, mf, also_revcomp=c.revcomp, n_threads=threads)
                    assert n * (2 if c.revcomp else 1) == q.shape[0] and np.array_equal(got, by_kmers), threads


def test_closed_forms(oracle):
    n = 12_000_000
    for name, mf, nodes in (("one_kmer-three_nodes", 1000, (11, 12, 13)), ("one_kmer-absent", 1000, ()), ("one_kmer-freq5", 4, ()),
                            ("one_kmer-freq5", 5, (21, 22, 23, 24, 25)), ("edges-kmer_last_hash", 1000, (31, 32, 33))):
        c = case(name, "full")
        want = np.zeros(c.max_node_id + 1, dtype=np.uint32)
        want[list(nodes)] = n
        assert mf in c.max_freqs
        assert np.array_equal(oracle.map_kmers(c.index, c.max_node_id, sk.lookups(c, oracle.extract), mf), want), (name, mf)
    c = case("one_kmer_revcomp", "full")
    want = np.zeros(c.max_node_id + 1, dtype=np.uint32)
    want[[11, 12, 13, 14, 15]] = n
    assert np.array_equal(oracle.map_kmers(c.index, c.max_node_id, sk.lookups(c, oracle.extract)), want)
    c = case("duplicates-one_read", "full")
    one, _ = oracle.map_reads(c.index, c.max_node_id, c.bases[:150], np.array([0, 150], dtype=np.int64), 31)
    assert one.sum() >= 120
    assert np.array_equal(oracle.map_kmers(c.index, c.max_node_id, sk.lookups(c, oracle.extract)), 80_000 * one)


def test_one_bucket_costs_the_oracle_less_than_the_other_cases_together(oracle):
    """one_bucket is the only case whose oracle cost grows with bucket length (queries x entries in the bucket).  Measured
    on an 8-core CPU-only machine at full scale: one_bucket (3 M queries x 200 entries) 0.68 s, the other fifteen cases
    together 2.17 s.  (No time is asserted on the absolute scale: only that the case stays the smaller part.)"""
    def cost(name):
        c = case(name, "full")
        q = sk.lookups(c, oracle.extract)
        t0 = time.perf_counter()
        oracle.map_kmers(c.index, c.max_node_id, q, c.max_freqs[-1])
        return time.perf_counter() - t0
    rest = sum(cost(n) for n in sk.CASES if n != "one_bucket")
    own = cost("one_bucket")
    print("\noracle seconds: one_bucket %.2f, the other cases together %.2f" % (own, rest))
    assert own < rest
