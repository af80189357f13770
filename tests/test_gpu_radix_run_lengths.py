"""GPU tests of the run-length form of the pass-1 directory (csrc/kmm_radix.hpp: k_rx_colscan<false>, k_rx_p2f): the scan
writes each run's start inside its block (S1T) and, per item, the virtual start of the run of the item's first block
(item_desc.y); pass 2 takes a run's length from two neighbouring columns and rebuilds the absolute starts with a prefix over
its 1024 table threads.  The shapes are the smallest at which that can go wrong: tables that are nearly all beyond the last
block, empty runs inside items, items of more than 1024 runs (the next table starts where the last one ended), items that
start in the middle of a run, runs of a whole block (the largest 16-bit difference), the last coarse partition (whose run
ends come from the block totals of the directory rows, strided), reverse complements, per-k-mer counts, sub-batches.

Every shape runs three ways on one handle — the filtering pass 2 with "radix_filter_slots" 1 and 0, and the plain pass 2
("radix_filter" 0), which still reads the absolute starts P1T from the scan's other form — with the geometry of
tests/skew_cases.py forced (391 coarse partitions of 16 fine ones: runs of a few k-mers), bit for bit against the oracle,
with the conservation counters of the passes."""
import numpy as np
import pytest

from tests import skew_cases as sk

pytestmark = pytest.mark.gpu

B = sk.B
WAYS = [pytest.param(1, 1, id="filter-slots"), pytest.param(1, 0, id="filter-bitmap"), pytest.param(0, None, id="plain")]


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def base():
    """The 50 000-entry index of the skew suite with the k-mer 0 under three nodes, and its genome (read-only)."""
    kmers, nodes, modulo, genome = sk._base()
    index, mx = sk._index(kmers, nodes, modulo, [(0, 11), (0, 12), (0, 13)], drop_hashes=(0,))
    return index, mx, genome


def _force(dev, radix_filter, slots, modulo):
    """tests/test_gpu_radix_skew.py::_force: the knobs in the order they depend on each other."""
    PF = -(-modulo // (1 << sk.W))
    F1 = -(-PF // (1 << sk.F2))
    dev.set_param("part_shift", sk.W)
    dev.set_param("radix_filter", radix_filter)
    dev.set_param("fine_bits", sk.F2)
    if slots is not None:
        dev.set_param("radix_filter_slots", slots)
        assert dev.get_param("radix_filter_slots") in (0, slots)      # (1 only where the geometry has a slot filter)
    dev.set_param("path", 2)
    got = tuple(dev.get_param(n) for n in ("part_shift", "n_partitions", "n_coarse_partitions", "n_fine_per_coarse", "radix_filter"))
    assert got == (sk.W, PF, F1, 1 << sk.F2, radix_filter)
    assert F1 == 391


def _radix(dev, run, expect, n_lookups, n_items=None, what=None):
    """One call on the radix path from a clean handle: the oracle's counts, conservation through the passes (the
    synchronising fetch runs the library's own check too), the path taken, the item total."""
    dev.reset()
    dev.get_stats(reset=True)
    rb, db = dev.get_param("radix_batches"), dev.get_param("direct_batches")
    run()
    got = dev.get_node_counts()
    assert got.dtype == np.uint32 and np.array_equal(got, expect), what
    p2, p3, dropped = (dev.get_param(n) for n in ("radix_p2_kmers", "radix_p3_kmers", "radix_p2_dropped"))
    assert (p2, p3 + dropped) == (n_lookups, n_lookups), (what, p2, p3, dropped)
    assert dev.get_stats(reset=True) == (n_lookups, int(expect.sum(dtype=np.uint64))), what
    assert dev.get_param("radix_batches") > rb and dev.get_param("direct_batches") == db, what
    if n_items is not None:
        assert dev.get_param("debug_rx_items") == n_items, what


def _item_shapes(q, modulo, positions=None):
    """From pass 1's directory restated in numpy: how many items have an EMPTY run starting inside them (pass 2 then walks /
    searches its table), how many have none (it uses the run-start bit mask), how many start in the middle of a run, the
    most blocks an item spans, the longest run."""
    q = np.asarray(q, dtype=np.uint64)
    PF = -(-modulo // (1 << sk.W))
    F1 = -(-PF // (1 << sk.F2))
    c = ((q % np.uint64(modulo)) >> np.uint64(sk.W + sk.F2)).astype(np.int64)
    block = (np.arange(q.shape[0], dtype=np.int64) if positions is None else np.asarray(positions, dtype=np.int64)) // B
    NB = int(block.max()) + 1
    runs = np.bincount(block * F1 + c, minlength=NB * F1).reshape(NB, F1)
    with_empty = without_empty = mid_run = span = 0
    for p in np.flatnonzero(runs.sum(axis=0)):
        P = np.concatenate([[0], np.cumsum(runs[:, p])])          # virtual start of every run, and the total
        for lo in range(0, int(P[-1]), B):
            hi = min(lo + B, int(P[-1]))
            b0 = int(np.searchsorted(P, lo, side="right")) - 1       # (the last run that starts at or below lo ...
            while runs[b0, p] == 0:
                b0 += 1                                               # ... and holds a k-mer: the item's first block)
            b1 = int(np.searchsorted(P, hi - 1, side="right")) - 1
            inside = (P[:-1] > lo) & (P[:-1] < hi)
            inside[:b0] = False
            if (inside & (runs[:, p] == 0)).any():
                with_empty += 1
            else:
                without_empty += 1
            mid_run += int(P[b0] < lo)
            span = max(span, b1 - b0 + 1)
    return dict(with_empty=with_empty, without_empty=without_empty, mid_run=mid_run, span=span, max_run=int(runs.max()), NB=NB)


def _reads_case(oracle, index, mx, bases, n_reads, revcomp=False):
    offs = np.arange(n_reads + 1, dtype=np.int64) * 150
    q = oracle.extract(bases, offs, sk.K)
    if revcomp:
        q = np.concatenate([q, sk.revcomp_kmers(q)])
    expect = oracle.map_kmers(index, mx, q)
    expect.setflags(write=False)
    return q, expect


def _open(kmm, index, mx, radix_filter, slots):
    dev = kmm.DeviceIndex.from_index(index, mx)
    _force(dev, radix_filter, slots, index._modulo)
    return dev


# ------------------------------------------------------------------------------------------------ 1, 2 and 3 blocks
@pytest.fixture(scope="module")
def tiny(base, oracle):
    """54, 109 and 163 reads of 150 bases: 8100, 16 350 and 24 450 positions = 1, 2 and 3 blocks of 8192 positions."""
    from kmer_mapper_amd import synthetic
    index, mx, genome = base
    out = []
    for nb, n_reads in ((1, 54), (2, 109), (3, 163)):
        assert -(-n_reads * 150 // B) == nb and n_reads <= 192
        bases, _ = synthetic.make_reads(genome, n_reads, 150, seed=400 + nb, n_rate=0.0)
        q, expect = _reads_case(oracle, index, mx, bases, n_reads)
        out.append((n_reads, bases, q, expect))
    return out


@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_one_two_and_three_blocks(kmm, base, tiny, radix_filter, slots):
    """Almost every thread of a run table lies beyond the last block: its empty run sits at the partition's total."""
    index, mx, _ = base
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        dev.set_param("radix_packed_tiles", 0)
        for n_reads, bases, q, expect in tiny:
            g = sk.geometry(q, index._modulo, sk.W, sk.F2, sk.read_positions(n_reads, 150))
            _radix(dev, lambda: dev.map_reads_uniform(bases, n_reads, 150, sk.K), expect, q.shape[0], g.n_items, ("blocks", g.n_blocks))
            # the same k-mers as an array
            _radix(dev, lambda: dev.map_kmers(q, k=sk.K), expect, q.shape[0], g.n_items, ("blocks, k-mers", g.n_blocks))


# ------------------------------------------------------------------------------------------------ empty runs inside items
@pytest.fixture(scope="module")
def gaps(base, oracle):
    """65 536 reads = 1200 blocks of ordinary reads (runs of ~17 k-mers per coarse partition and block: ~480 runs per item)
    with two stretches of 164 poly-A reads (three blocks) at blocks 300 and 900: the items of the other partitions that span
    a stretch hold empty runs, the rest hold none — and the first coarse partition gets runs of whole blocks."""
    from kmer_mapper_amd import synthetic
    index, mx, genome = base
    n_reads = 65536
    bases, _ = synthetic.make_reads(genome, n_reads, 150, seed=410, n_rate=0.0)
    rd = bases.reshape(n_reads, 150).copy()
    for blk in (300, 900):
        r0 = blk * B // 150
        rd[r0:r0 + 164] = ord("A")
    bases = rd.reshape(-1)
    q, expect = _reads_case(oracle, index, mx, bases, n_reads)
    shapes = _item_shapes(q, index._modulo, sk.read_positions(n_reads, 150))
    assert 1100 <= shapes["NB"] <= 1300
    assert shapes["with_empty"] >= 100 and shapes["without_empty"] >= 100, shapes     # the walk / search and the bit mask
    return n_reads, bases, q, expect


@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_empty_runs_inside_items(kmm, base, gaps, radix_filter, slots):
    index, mx, _ = base
    n_reads, bases, q, expect = gaps
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        dev.set_param("radix_packed_tiles", 0)
        n_items = sk.geometry(q, index._modulo, sk.W, sk.F2, sk.read_positions(n_reads, 150)).n_items
        _radix(dev, lambda: dev.map_reads_uniform(bases, n_reads, 150, sk.K), expect, q.shape[0], n_items, "gaps")


# ------------------------------------------------------------------------------------------------ hot and cold
@pytest.fixture(scope="module")
def hot_cold(base, oracle):
    """71 000 reads = 1300 blocks, 99 % of them poly-A (the k-mer 0: coarse partition 0), 1 % ordinary: a cold partition's
    one item spans all the blocks — more than one table of 1024 runs — and the hot partition's items start mid-run."""
    from kmer_mapper_amd import synthetic
    index, mx, genome = base
    n_reads, n_cold = 71000, 710
    cold, _ = synthetic.make_reads(genome, n_cold, 150, seed=420, n_rate=0.0)
    rd = sk._poly(n_reads, 150).reshape(n_reads, 150)
    rd[np.random.default_rng(421).choice(n_reads, size=n_cold, replace=False)] = cold.reshape(n_cold, 150)
    bases = rd.reshape(-1)
    q, expect = _reads_case(oracle, index, mx, bases, n_reads)
    shapes = _item_shapes(q, index._modulo, sk.read_positions(n_reads, 150))
    assert shapes["NB"] > 1024 and shapes["span"] > 1024 and shapes["mid_run"] >= 100, shapes
    assert int((q == 0).sum()) > 0.98 * q.shape[0]
    return n_reads, bases, q, expect


@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_items_of_more_than_1024_runs_and_items_that_start_mid_run(kmm, base, hot_cold, radix_filter, slots):
    index, mx, _ = base
    n_reads, bases, q, expect = hot_cold
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        dev.set_param("radix_packed_tiles", 0)
        n_items = sk.geometry(q, index._modulo, sk.W, sk.F2, sk.read_positions(n_reads, 150)).n_items
        _radix(dev, lambda: dev.map_reads_uniform(bases, n_reads, 150, sk.K), expect, q.shape[0], n_items, "hot and cold")
        _radix(dev, lambda: dev.map_kmers(q, k=sk.K), expect, q.shape[0], n_items, "hot and cold, k-mers")


# ------------------------------------------------------------------------------------------------ runs of a whole block
@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_runs_of_8192(kmm, base, oracle, radix_filter, slots):
    """One k-mer 3 x 8192 + 5 times: three runs of 8192 (the largest difference of two 16-bit starts) and one of 5; the
    partition's total is a multiple of 8192 plus a partly filled last item."""
    index, mx, _ = base
    q = np.zeros(3 * B + 5, dtype=np.uint64)
    expect = oracle.map_kmers(index, mx, q)
    assert expect[11] == expect[12] == expect[13] == q.shape[0]
    shapes = _item_shapes(q, index._modulo)
    assert shapes["max_run"] == B and shapes["NB"] == 4
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        _radix(dev, lambda: dev.map_kmers(q, k=sk.K), expect, q.shape[0], 4, "runs of 8192")


# ------------------------------------------------------------------------------------------------ the last coarse partition
@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_everything_in_the_last_coarse_partition(kmm, oracle, radix_filter, slots):
    """skew_cases.edges "slice_last": every k-mer hashes into the last fine partition, hence the last of the 391 coarse
    partitions (391 is no multiple of 8): its runs end at the block totals of the directory rows."""
    c = sk.build("edges-slice_last", "small")
    q = c.kmers
    F1 = 391
    assert (((q % np.uint64(c.index._modulo)) >> np.uint64(sk.W + sk.F2)) == F1 - 1).all()
    g = sk.geometry(q, c.index._modulo, c.w, c.f2)
    assert g.F1 == F1
    expect = oracle.map_kmers(c.index, c.max_node_id, q)
    with _open(kmm, c.index, c.max_node_id, radix_filter, slots) as dev:
        _radix(dev, lambda: dev.map_kmers(q, k=c.k), expect, q.shape[0], g.n_items, "last coarse partition")


# ------------------------------------------------------------------------------------------------ revcomp, per-k-mer, sub-batches
@pytest.fixture(scope="module")
def medium(base, oracle):
    """3000 reads = 55 blocks (110 with the reverse complements)."""
    from kmer_mapper_amd import synthetic
    index, mx, genome = base
    n_reads = 3000
    bases, _ = synthetic.make_reads(genome, n_reads, 150, seed=430, n_rate=0.0)
    q, expect = _reads_case(oracle, index, mx, bases, n_reads, revcomp=True)
    e_fwd = oracle.map_kmers(index, mx, q[:q.shape[0] // 2])
    e_fwd.setflags(write=False)
    return n_reads, bases, q, expect, e_fwd


@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_reverse_complements(kmm, base, medium, radix_filter, slots):
    index, mx, _ = base
    n_reads, bases, q, expect, _ = medium
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        _radix(dev, lambda: dev.map_reads_uniform(bases, n_reads, 150, sk.K, also_revcomp=True), expect, q.shape[0], None, "revcomp")
        own = np.ascontiguousarray(q[:q.shape[0] // 2])
        _radix(dev, lambda: dev.map_kmers(own, also_revcomp=True, k=sk.K), expect, q.shape[0], None, "revcomp, k-mers")


@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_per_kmer_counts(kmm, base, medium, radix_filter, slots):
    """Per-k-mer counting mode: a count per index entry, node counts that are their sum per node."""
    index, mx, _ = base
    _, _, q, _, _ = medium
    per_entry = sk.numpy_entry_counts(index._kmers, q)
    per_node = np.bincount(index._nodes, per_entry.astype(np.float64), minlength=mx + 1)
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        dev.count_kmers_mode(True)
        assert dev.get_param("count_kmers") == 1
        dev.map_kmers(q, 65535, k=sk.K)
        assert np.array_equal(dev.get_kmer_counts(), per_entry)
        assert np.array_equal(dev.get_node_counts().astype(np.float64), per_node)
        assert dev.get_param("radix_p2_kmers") == q.shape[0]
        assert dev.get_param("radix_p3_kmers") + dev.get_param("radix_p2_dropped") == q.shape[0]


@pytest.mark.parametrize("radix_filter, slots", WAYS)
def test_sub_batches_rebuild_the_tables(kmm, base, medium, radix_filter, slots):
    """Sub-batches of 4 blocks: 55 blocks take 14 of them, each with a directory, item table and run tables of its own."""
    index, mx, _ = base
    n_reads, bases, q, expect, e_half = medium
    half = q.shape[0] // 2
    with _open(kmm, index, mx, radix_filter, slots) as dev:
        dev.set_param("radix_sub_batch_kmers", 4 * B)
        assert dev.get_param("radix_sub_batch_kmers") == 4 * B
        assert -(-n_reads * 150 // (4 * B)) >= 3
        for packed in (1, 0):
            dev.set_param("radix_packed_tiles", packed)
            _radix(dev, lambda: dev.map_reads_uniform(bases, n_reads, 150, sk.K), e_half, half, None, ("sub-batches", packed))
        _radix(dev, lambda: dev.map_kmers(q, k=sk.K), expect, q.shape[0], None, "sub-batches, k-mers")
