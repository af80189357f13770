"""Skewed and low-complexity batches for the radix path (csrc/kmm_radix.hpp:48-51: "nothing depends on partition sizes
being balanced"), with the plain-numpy tools both tiers need: `geometry` restates how the passes cut a batch into
partitions, items and rows (kmm_radix.hpp:14-29, k_rx_tables) and `numpy_map_kmers` restates mapper.pyx:53-69 as a
second opinion beside the C oracle.  Pure numpy, seeded, no GPU; nothing here reads the library's kernels.

Every case is `build(name, scale)` with scale "small" (at most 1 M k-mers) or "full", and returns a record:

    index, max_node_id, k, w (part_shift), f2 (fine_bits)      the index and the radix geometry the GPU test forces
    kmers                                                        k-mer-shaped cases: the uint64 queries
    bases, n_reads, read_len [, bases_n]                         read-shaped cases: reads of one length, flat (bases_n: the
                                                                 same reads with N for A in every second poly-A read)
    revcomp, max_freqs                                           how the case is mapped

CASES lists the names; tests/test_skew_cases_on_the_cpu.py holds every case to the condition it exists for.
"""
import types

import numpy as np

from kmer_mapper_amd import synthetic
from kmer_mapper_amd.kmer_index import KmerIndex

B = 8192          # positions per pass-1 block = k-mers per pass-2 item (RX_B)
ITEMS_PER_ROW = 1024   # pass-2 items per pass-3 work item (RX_IC)
SUB_RUN = 16      # k-mers per sub-run of the pass-2 / pass-3 windows (RX_LPR)
K = 31
W, F2 = 4, 4      # modulo 100 003: PF = 6251 fine partitions of 16 buckets, F2 = 16, F1 = 391 coarse partitions
POLY_T = np.uint64(4 ** K - 1)

CASES = ["one_kmer-three_nodes", "one_kmer-absent", "one_kmer-freq5", "one_kmer_revcomp", "hot_and_cold", "tandem",
         "duplicates-one_read", "duplicates-300_reads", "sorted_hashes-ascending", "sorted_hashes-descending", "one_bucket",
         "one_slice", "edges-kmer_last_hash", "edges-slice_last", "edges-slice_first", "zipf"]
READ_SHAPED = ("one_kmer", "hot_and_cold", "tandem", "duplicates")
SCALES = ("small", "full")


# ---------------------------------------------------------------------------------------------- tools of both tiers
def geometry(kmers, modulo, w, f2, positions=None):
    """How the radix path cuts `kmers` (uint64, in the order pass 1 meets them) for slices of 2^w buckets and 2^f2 fine
    partitions per coarse one.  positions: the position of every k-mer in the flat input (reads: its first base; default:
    its index in the array, as kmm_map_kmers numbers them); block b of pass 1 = positions [8192 b, 8192 (b + 1)).

    T1[c]       k-mers of coarse partition c = (q % modulo) >> (w + f2)
    items[c]    ceil(T1[c] / 8192): c's runs, block after block, form one array that is cut every 8192 k-mers
    rows[c]     ceil(items[c] / 1024): pass-3 work items per fine partition of c
    item_part, item_blocks   for every item: its coarse partition and how many blocks it spans (first to last block
                that holds one of its k-mers)
    parts_per_block_max         the most coarse partitions any one block holds k-mers of
    max_run, whole_block_runs   longest pass-1 run (k-mers of one partition in one block) and how many runs fill a block
    """
    kmers = np.asarray(kmers, dtype=np.uint64)
    modulo, w, f2 = int(modulo), int(w), int(f2)
    PF = -(-modulo // (1 << w))
    F1 = -(-PF // (1 << f2))
    h = kmers % np.uint64(modulo)
    c = (h >> np.uint64(w + f2)).astype(np.int64)
    del h
    if positions is None:
        block = np.arange(kmers.shape[0], dtype=np.int64) // B
        n_blocks = -(-kmers.shape[0] // B)
    else:
        positions = np.asarray(positions)
        block = (positions // B).astype(np.int64)
        n_blocks = int(block.max()) + 1 if block.size else 0
    runs = np.bincount(block * F1 + c, minlength=n_blocks * F1).reshape(n_blocks, F1)   # the directory rows of pass 1
    del block, c
    T1 = runs.sum(axis=0)
    parts_per_block = (runs > 0).sum(axis=1)
    items = -(-T1 // B)
    rows = -(-items // ITEMS_PER_ROW)
    item_part, item_blocks = [], []
    for p in np.flatnonzero(T1):
        before = np.cumsum(runs[:, p])                     # k-mers of p up to and including each block
        first = np.arange(items[p], dtype=np.int64) * B    # rank of every item's first k-mer inside p
        last = np.minimum(first + B, T1[p]) - 1
        b0 = np.searchsorted(before, first, side="right")
        b1 = np.searchsorted(before, last, side="right")
        item_part.append(np.full(items[p], p, dtype=np.int64))
        item_blocks.append(b1 - b0 + 1)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    return types.SimpleNamespace(
        PF=PF, F1=F1, F2=1 << f2, n_blocks=n_blocks, n_kmers=int(kmers.shape[0]), T1=T1, items=items, rows=rows,
        n_items=int(items.sum()), item_part=cat(item_part), item_blocks=cat(item_blocks),
        parts_per_block_max=int(parts_per_block.max()) if runs.size else 0,
        max_run=int(runs.max()) if runs.size else 0, whole_block_runs=int((runs == B).sum()),
        hot_share=float(T1.max()) / max(1, int(kmers.shape[0])))


def numpy_map_kmers(index, max_node_id, kmers, max_freq=1000):
    """mapper.pyx:53-69 without its loop: every query equal to an entry's k-mer adds one to the entry's node unless the
    entry's frequency exceeds max_freq; the uint32 vector wraps."""
    uq, uc = np.unique(np.asarray(kmers, dtype=np.uint64), return_counts=True)
    ek = np.asarray(index._kmers, dtype=np.uint64)
    counts = np.zeros(int(max_node_id) + 1, dtype=np.uint64)
    if uq.size and ek.size:
        pos = np.minimum(np.searchsorted(uq, ek), uq.size - 1)
        hit = (uq[pos] == ek) & (np.asarray(index._frequencies).astype(np.int64) <= int(max_freq))
        np.add.at(counts, np.asarray(index._nodes, dtype=np.int64)[hit], uc[pos][hit].astype(np.uint64))
    return (counts % np.uint64(1 << 32)).astype(np.uint32)


def numpy_entry_counts(entry_kmers, kmers):
    """Per index entry: how many of `kmers` equal it (GpuCounter semantics, gpu_counter.py:23-37; no frequency test)."""
    uq, uc = np.unique(np.asarray(kmers, dtype=np.uint64), return_counts=True)
    pos = np.minimum(np.searchsorted(uq, entry_kmers), max(uq.size - 1, 0))
    return np.where(uq[pos] == entry_kmers, uc[pos], 0).astype(np.uint32)


def revcomp_kmers(q, k=K):
    """Reverse complements of packed k-mers (first base in the lowest two bits, A C G T = 0 1 2 3)."""
    x = ~np.asarray(q, dtype=np.uint64)
    m2, m4 = np.uint64(0x3333333333333333), np.uint64(0x0F0F0F0F0F0F0F0F)
    x = ((x >> np.uint64(2)) & m2) | ((x & m2) << np.uint64(2))
    x = ((x >> np.uint64(4)) & m4) | ((x & m4) << np.uint64(4))
    return x.byteswap() >> np.uint64(64 - 2 * k)


def read_positions(n_reads, read_len, k=K):
    """Position of every k-mer's first base in the flat input, in (read, offset) order."""
    return (np.arange(n_reads, dtype=np.int64)[:, None] * read_len + np.arange(read_len - k + 1, dtype=np.int64)[None, :]).reshape(-1)


def lookups(case, extract):
    """The k-mers a case looks up, in (read, offset) order, reverse complements behind them.  extract: the oracle's
    (util.py:71-75; the reads are the input, their k-mers are derived)."""
    if case.kmers is not None:
        q = case.kmers
    else:
        q = extract(case.bases, np.arange(case.n_reads + 1, dtype=np.int64) * case.read_len, case.k)
    return np.concatenate([q, revcomp_kmers(q, case.k)]) if case.revcomp else q


def ragged_offsets(n_bytes, seed):
    """Read lengths 0..400 that add up to n_bytes: the same content cut differently."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 401, size=n_bytes // 150 + 64, dtype=np.int64)
    ends = np.cumsum(lens)
    n = int(np.searchsorted(ends, n_bytes, side="left"))
    offs = np.concatenate([[0], ends[:n], [n_bytes]]).astype(np.int64)
    return offs


def fastq(bases, n_reads, read_len):
    """The reads as FASTQ bytes: '@r\\n' + read + '\\n+\\n' + quality + '\\n'."""
    rec = np.empty((n_reads, 2 * read_len + 7), dtype=np.uint8)
    rec[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + read_len] = np.asarray(bases).reshape(n_reads, read_len)
    rec[:, 3 + read_len:6 + read_len] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + read_len:6 + 2 * read_len] = ord("I")
    rec[:, -1] = ord("\n")
    return rec.reshape(-1)


# ---------------------------------------------------------------------------------------------- indexes
def _base(seed=1, skewed=False, n=50_000, modulo=None):
    index, genome = synthetic.make_index(n, seed=seed, skewed=skewed, modulo=modulo)
    return index._kmers.copy(), index._nodes.astype(np.int64), index._modulo, genome


def _index(kmers, nodes, modulo, extra=(), drop_hashes=()):
    """The base entries without those of `drop_hashes`' buckets, plus `extra` = (k-mer, node) pairs."""
    M = np.uint64(modulo)
    keep = ~np.isin(kmers % M, np.array(list(drop_hashes), dtype=np.uint64)) if len(drop_hashes) else np.ones(kmers.shape[0], bool)
    ek = np.array([e[0] for e in extra], dtype=np.uint64)
    en = np.array([e[1] for e in extra], dtype=np.int64)
    kmers, nodes = np.concatenate([kmers[keep], ek]), np.concatenate([nodes[keep], en])
    return KmerIndex.from_flat_kmers(kmers, nodes, modulo), int(nodes.max())


def _case(name, scale, index, mx, w=W, f2=F2, **kw):
    c = types.SimpleNamespace(name=name, scale=scale, index=index, max_node_id=mx, k=K, w=w, f2=f2, kmers=None, bases=None,
                              bases_n=None, n_reads=0, read_len=0, revcomp=False, max_freqs=(1000,), entry_order=None)
    c.__dict__.update(kw)
    return c


def _poly(n_reads, read_len, letter=b"A"):
    return np.full(n_reads * read_len, ord(letter), dtype=np.uint8)


def _n_for_a(bases, n_reads, read_len):
    """N instead of A in every second read that is all A (command_line_interface.py:41 maps N to A)."""
    rd = bases.reshape(n_reads, read_len).copy()
    poly = np.flatnonzero((rd == ord("A")).all(axis=1))
    rd[poly[::2]] = ord("N")
    return rd.reshape(-1)


# ---------------------------------------------------------------------------------------------- the cases
def one_kmer(scale, variant="three_nodes", slices13=False):
    """Reads of 150 A: the k-mer 0, 120 times per read.  Index variants: 0 under nodes 11, 12, 13; absent and its bucket
    empty; under 5 nodes (frequency 5), mapped with max_index_lookup_frequency 4 (filtered) and 5 (kept).  slices13: an
    index whose slices hold 8192 buckets (part_shift 13), for the knob test."""
    n_reads = 100_000 if scale == "full" else 8_000
    kmers, nodes, modulo, _ = _base(341, n=21_500, modulo=40_009) if slices13 else _base()
    extra = {"three_nodes": [(0, 11), (0, 12), (0, 13)], "absent": [], "freq5": [(0, n) for n in (21, 22, 23, 24, 25)],
             "revcomp": [(0, 11), (0, 12), (0, 13), (int(POLY_T), 14), (int(POLY_T), 15)]}[variant]
    index, mx = _index(kmers, nodes, modulo, extra, drop_hashes=(0, int(POLY_T) % modulo))
    bases = _poly(n_reads, 150)
    return _case("one_kmer", scale, index, mx, bases=bases, bases_n=_n_for_a(bases, n_reads, 150), n_reads=n_reads, read_len=150,
                 revcomp=variant == "revcomp", max_freqs=(4, 5) if variant == "freq5" else (1000,),
                 **(dict(w=13, f2=None) if slices13 else {}))


def hot_and_cold(scale, slices13=False):
    """99 % reads of 150 A, 1 % ordinary reads from the genome, shuffled: one coarse partition takes 99 % of the k-mers
    and the others a few hundred to a few thousand each, spread over every block of the batch."""
    n_reads = 500_000 if scale == "full" else 8_000
    kmers, nodes, modulo, genome = _base(341, n=21_500, modulo=40_009) if slices13 else _base()
    index, mx = _index(kmers, nodes, modulo, [(0, 11), (0, 12), (0, 13)], drop_hashes=(0,))
    n_cold = n_reads // 100
    cold, _ = synthetic.make_reads(genome, n_cold, 150, seed=21)
    rd = _poly(n_reads, 150).reshape(n_reads, 150)
    where = np.random.default_rng(22).choice(n_reads, size=n_cold, replace=False)
    rd[where] = cold.reshape(n_cold, 150)
    bases = rd.reshape(-1)
    return _case("hot_and_cold", scale, index, mx, bases=bases, bases_n=_n_for_a(bases, n_reads, 150), n_reads=n_reads,
                 read_len=150, **(dict(w=13, f2=None) if slices13 else {}))


TANDEM_UNITS = (b"A", b"C", b"AT", b"CG", b"ACG", b"AAT", b"ACGT", b"AACT", b"AACCGT", b"ACGTTG")


def tandem(scale):
    """Reads that repeat a unit of 1, 2, 3, 4 or 6 bases, starting at any phase: 32 distinct k-mers in all, every read
    one of them over and over at the unit's period, so equal keys sit in lanes a fixed distance apart.  Every second
    distinct k-mer is in the index."""
    n_reads = 200_000 if scale == "full" else 8_000
    rng = np.random.default_rng(31)
    unit = rng.integers(0, len(TANDEM_UNITS), size=n_reads)
    phase = rng.integers(0, 6, size=n_reads)
    rd = np.empty((n_reads, 150), dtype=np.uint8)
    for u, s in enumerate(TANDEM_UNITS):
        rows = np.flatnonzero(unit == u)
        long = np.frombuffer(s * (160 // len(s) + 1), dtype=np.uint8)
        rd[rows] = long[phase[rows][:, None] + np.arange(150)[None, :]]
    distinct = []
    for s in TANDEM_UNITS:
        code = np.frombuffer((s * 40)[:K + len(s)], dtype=np.uint8)
        code = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), code).astype(np.uint8)
        distinct.append(synthetic.pack_kmers_at(code, np.arange(len(s)), K))
    distinct = np.unique(np.concatenate(distinct))
    kmers, nodes, modulo, _ = _base()
    index, mx = _index(kmers, nodes, modulo, [(int(q), 100 + i) for i, q in enumerate(distinct[::2])])
    return _case("tandem", scale, index, mx, bases=rd.reshape(-1), n_reads=n_reads, read_len=150,
                 distinct=distinct)


def duplicates(scale, variant="one_read"):
    """One error-free 150-base read of the genome 80 000 times, or 300 distinct ones in turn: 120 (36 000) distinct
    k-mers, each of them in the index (node = 1000 + its number modulo 500), hit rate 1."""
    n_reads = 80_000 if scale == "full" else 8_000
    n_distinct = 1 if variant == "one_read" else 300
    kmers, nodes, modulo, genome = _base()
    reads, _ = synthetic.make_reads(genome, n_distinct, 150, seed=41, sub_rate=0.0, n_rate=0.0)
    codes = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), reads & 0xDF).astype(np.uint8)
    own = np.unique(synthetic.pack_kmers_at(codes, read_positions(n_distinct, 150), K))
    own = own[~np.isin(own, kmers)]
    index, mx = _index(kmers, nodes, modulo, [(int(q), 1000 + i % 500) for i, q in enumerate(own)])
    rd = reads.reshape(n_distinct, 150)[np.arange(n_reads) % n_distinct]
    return _case("duplicates", scale, index, mx, bases=np.ascontiguousarray(rd.reshape(-1)), n_reads=n_reads, read_len=150,
                 n_distinct_reads=n_distinct)


def _mixed_queries(index_kmers, n, rng, hit_share=0.5):
    hits = index_kmers[rng.integers(0, index_kmers.shape[0], size=int(n * hit_share))]
    miss = rng.integers(0, 1 << 62, size=n - hits.shape[0], dtype=np.uint64)
    q = np.concatenate([hits, miss])
    return q[rng.permutation(n)]


def sorted_hashes(scale, variant="ascending"):
    """8 M k-mers (half of them index entries) sorted by q % modulo: the hot partition moves through the batch, every
    block lies inside one or two coarse partitions and the items are cut in the middle of runs."""
    n = 8_000_000 if scale == "full" else 500_000
    kmers, nodes, modulo, _ = _base()
    index, mx = _index(kmers, nodes, modulo)
    q = _mixed_queries(kmers, n, np.random.default_rng(51))
    q = q[np.argsort(q % np.uint64(modulo), kind="stable")]
    return _case("sorted_hashes", scale, index, mx, kmers=np.ascontiguousarray(q if variant == "ascending" else q[::-1]))


ONE_BUCKET_HASH, ONE_BUCKET_ENTRIES = 54_321, 200


def one_bucket(scale):
    """q = h + modulo * j: distinct quotients in the one bucket h, which holds 200 such entries (j even) besides what the
    base index put there; the queries draw j from 0..399, so half of them match."""
    n = 3_000_000 if scale == "full" else 200_000
    kmers, nodes, modulo, _ = _base()
    own = [(ONE_BUCKET_HASH + modulo * 2 * j, 2000 + j % 37) for j in range(ONE_BUCKET_ENTRIES)]
    index, mx = _index(kmers, nodes, modulo, own)
    j = np.random.default_rng(61).integers(0, 2 * ONE_BUCKET_ENTRIES, size=n, dtype=np.uint64)
    return _case("one_bucket", scale, index, mx, kmers=np.uint64(ONE_BUCKET_HASH) + np.uint64(modulo) * j)


def one_slice(scale, fine=3000, name="one_slice"):
    """Hashes uniform inside ONE fine partition (16 buckets, fewer in the last one), any quotient; a third of the queries
    are the partition's own index entries."""
    n = 4_000_000 if scale == "full" else 300_000
    kmers, nodes, modulo, _ = _base()
    lo, hi = fine << W, min((fine + 1) << W, modulo)
    own = [(h + modulo * (7 + 3 * i), 3000 + i) for i, h in enumerate(range(lo, hi))]        # every bucket holds an entry
    index, mx = _index(kmers, nodes, modulo, own)
    rng = np.random.default_rng(71 + fine)
    eh = index._kmers % np.uint64(modulo)
    ek = index._kmers[(eh >= np.uint64(lo)) & (eh < np.uint64(hi))]
    h = rng.integers(lo, hi, size=n, dtype=np.uint64)
    q = h + np.uint64(modulo) * rng.integers(0, 1 << 40, size=n, dtype=np.uint64)
    own_q = rng.random(n) < 1 / 3
    q[own_q] = ek[rng.integers(0, ek.shape[0], size=int(own_q.sum()))]
    return _case(name, scale, index, mx, kmers=q)


def edges(scale, variant):
    """The ends of the hash range: the single k-mer whose hash is modulo - 1 (the last bucket of the clipped last slice of
    the short last coarse partition), one_slice in the last fine partition and in the first."""
    kmers, nodes, modulo, _ = _base()
    PF = -(-modulo // (1 << W))
    if variant == "slice_last":
        return one_slice(scale, fine=PF - 1, name="edges")
    if variant == "slice_first":
        return one_slice(scale, fine=0, name="edges")
    n = 12_000_000 if scale == "full" else 900_000
    q = modulo - 1 + modulo * 5
    index, mx = _index(kmers, nodes, modulo, [(q, 31), (q, 32), (q, 33)], drop_hashes=(modulo - 1,))
    return _case("edges", scale, index, mx, kmers=np.full(n, q, dtype=np.uint64))


def zipf(scale):
    """K-mers drawn from the index's own distinct entries with probability ~ 1 / rank (rank by a seeded shuffle), a fifth
    of the batch misses; the index has the `skewed` node model (1000 nodes, ~50 entries each)."""
    n = 8_000_000 if scale == "full" else 500_000
    kmers, nodes, modulo, _ = _base(seed=7, skewed=True)
    index, mx = _index(kmers, nodes, modulo)
    rng = np.random.default_rng(81)
    ranked = rng.permutation(np.unique(kmers))
    p = 1.0 / np.arange(1, ranked.shape[0] + 1)
    drawn = ranked[np.searchsorted(np.cumsum(p / p.sum()), rng.random(n - n // 5)).clip(0, ranked.shape[0] - 1)]
    q = np.concatenate([drawn, rng.integers(0, 1 << 62, size=n // 5, dtype=np.uint64)])
    return _case("zipf", scale, index, mx, kmers=q[rng.permutation(n)])


def build(name, scale):
    assert scale in SCALES, scale
    fn, _, variant = name.partition("-")
    if fn == "one_kmer_revcomp":
        c = one_kmer(scale, "revcomp")
    elif variant:
        c = globals()[fn](scale, variant)
    else:
        c = globals()[fn](scale)
    c.id = "%s-%s" % (name, scale)
    return c
