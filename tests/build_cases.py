"""Inputs for the GPU index builder (kmm_build_index: csrc/kmm_build.hpp, driver in csrc/kmm.hip) at the seams of its
kernels, with a model of the result that shares nothing with the builder or with the C oracle.  Pure numpy, seeded, no GPU,
no ctypes; nothing here reads the library's kernels.

`model(kmers, nodes, modulo)` spells the five arrays out with library calls only — a stable argsort by hash, a bincount, a
cumulative sum, np.unique for the frequencies.  It has no bucket-length threshold, no per-bucket loop, no sorted copy and no
binary search, which is what oracle_build_index and the kernels have in common.

Every case is `build(name)` and returns a record:

    kmers, nodes, modulo      the input: uint64 k-mers, int64 node ids in 0 .. 2^31 - 1, in a seeded shuffle (so that "input
                              order inside a bucket" differs from every order the generator or a sort would give)
    check(case, m)            the case's own claims about m = model(...): the bucket lengths it exists for, the number of
                              large buckets, the clipped frequencies ...; raises AssertionError when the case is not what
                              its name says

A bucket of a chosen length c at hash h holds the k-mers h + modulo * t for quotients t drawn from the whole range that keeps
the sum below 2^64, so bits 62 and 63 are set in about half the k-mers of every case.  CASES lists the names;
tests/test_build_cases_on_the_cpu.py holds every case to its claims, tests/test_gpu_index_builder.py runs them on the GPU.
"""
import collections
import functools
import types

import numpy as np

TOP = (1 << 64) - 1
BIG = 64                     # buckets with more entries go to the one-workgroup-per-bucket kernel (BI_BIG)
ENTRY_GRID = 65_536 * 256    # threads of the largest grid of the per-entry kernels: a longer input takes a second trip
CLIP = 65_535                # the format's frequencies are uint16

# The second high_bits modulo.  The arrays of `modulo` int32 for a modulo in the top 64 of the int32 range are 8.6 GB each
# on the host (17 GB as the int64 intermediates of the numpy builder): minutes of page faults and copies, not seconds.
# 2^26 - 5 is the largest of the moduli tried (2^26 - 5, 2^28 - 57) whose case models and compares in a few seconds on a
# CPU-only machine (2 s for the model; 2^28 - 57 took 8 s, with 2 GB per int64 intermediate); the modulo arithmetic on
# 64-bit k-mers, which is the point of the case, does not depend on the modulo's size.
HIGH_BITS_MODULI = (100_003, (1 << 26) - 5)

Index = collections.namedtuple("Index", "hashes_to_index n_kmers kmers nodes frequencies")   # the order of engine.build_index


def model(kmers, nodes, modulo):
    """What FlatKmers -> from_flat_kmers(modulo) -> convert_to_int32 leaves: entries in a stable sort by kmer % modulo,
    the bucket directory (0 for an empty bucket), the number of entries that hold each entry's k-mer, clipped to uint16."""
    kmers = np.asarray(kmers, dtype=np.uint64)
    nodes = np.asarray(nodes)
    M = int(modulo)
    hashes = (kmers % np.uint64(M)).astype(np.int64)
    order = np.argsort(hashes, kind="stable")
    n_kmers = np.bincount(hashes, minlength=M)
    hashes_to_index = np.cumsum(n_kmers) - n_kmers
    hashes_to_index[n_kmers == 0] = 0
    _, inverse, counts = np.unique(kmers, return_inverse=True, return_counts=True)
    frequencies = np.minimum(counts[inverse.reshape(-1)], CLIP)
    return Index(hashes_to_index.astype(np.int32), n_kmers.astype(np.int32), np.ascontiguousarray(kmers[order]),
                 nodes[order].astype(np.int32), frequencies[order].astype(np.uint16))


def as_index(arrays, node_mask=None):
    """The five arrays as the object the lookups read (mapper.pyx:22-29).  node_mask: node ids ANDed with it (a count
    vector over all 2^31 node ids is 8.6 GB; the lookup tests fold the ids into a vector they can compare)."""
    a = Index(*arrays)
    nodes = a.nodes if node_mask is None else (a.nodes & np.int32(node_mask))
    return types.SimpleNamespace(_hashes_to_index=a.hashes_to_index, _n_kmers=a.n_kmers, _nodes=nodes, _kmers=a.kmers,
                                 _frequencies=a.frequencies, _modulo=int(a.n_kmers.shape[0]))


# ---------------------------------------------------------------------------------------------- generators
def _quotients(rng, M, h, count):
    """`count` distinct t with h + M * t < 2^64, uniform over that whole range, in random order."""
    t_max = (TOP - h) // M
    assert t_max + 1 >= count, (M, h, count)
    t = np.zeros(0, dtype=np.uint64)
    while t.shape[0] < count:
        t = np.unique(np.concatenate([t, rng.integers(0, t_max, size=2 * count + 16, dtype=np.uint64, endpoint=True)]))
    return rng.permutation(t)[:count]


def _keys(rng, M, h, count):
    """`count` distinct k-mers of hash h."""
    return np.uint64(h) + np.uint64(M) * _quotients(rng, M, h, count)


def _bucket(rng, M, h, c):
    """c entries of hash h: two thirds of them distinct k-mers, the rest repeats of a quarter of those (which the nodes,
    drawn later, tell apart)."""
    n_rep = c // 3
    pool = _keys(rng, M, h, c - n_rep)
    return np.concatenate([pool, pool[rng.integers(0, max(1, pool.shape[0] // 4), size=n_rep)]])


def _any_keys(rng, M, hashes):
    """One k-mer per given hash, any quotient that fits below 2^64 for every hash."""
    hashes = np.asarray(hashes, dtype=np.uint64)
    t = rng.integers(0, (TOP - (M - 1)) // M, size=hashes.shape[0], dtype=np.uint64, endpoint=True)
    return hashes + np.uint64(M) * t


def _with_duplicates(rng, a, share=0.2):
    """`share` of the entries overwritten with copies of other entries."""
    n = a.shape[0]
    if n > 10:
        a[rng.integers(0, n, size=int(n * share))] = a[rng.integers(0, n, size=int(n * share))]
    return a


def _finish(name, rng, parts, M, check, **claims):
    kmers = np.concatenate([np.asarray(p, dtype=np.uint64) for p in parts]) if parts else np.zeros(0, dtype=np.uint64)
    n = kmers.shape[0]
    nodes = rng.integers(0, 1 << 31, size=n, dtype=np.int64)
    if n >= 2:
        nodes[0], nodes[1] = 0, (1 << 31) - 1
    elif n == 1:
        nodes[0] = (1 << 31) - 1
    perm = rng.permutation(n)
    kmers, nodes = np.ascontiguousarray(kmers[perm]), np.ascontiguousarray(nodes[perm])
    kmers.flags.writeable = nodes.flags.writeable = False
    return types.SimpleNamespace(name=name, kmers=kmers, nodes=nodes, modulo=int(M), check=check, **claims)


def _check_lengths(c, m):
    for h, length in c.lengths.items():
        assert int(m.n_kmers[h]) == length, (c.name, h, length, int(m.n_kmers[h]))


def _frequency_of(m, key):
    """The frequencies the model gives the entries that hold `key` (they must all be equal) and how many there are."""
    f = m.frequencies[m.kmers == np.uint64(key)]
    assert f.size and (f == f[0]).all(), key
    return int(f[0]), int(f.size)


# ---------------------------------------------------------------------------------------------- the cases
THRESHOLD_LENGTHS = (1, 2, 3, 4, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3000,
                     4097)
THRESHOLD_FIRST_HASH = 100


def threshold():
    """Modulo 4099; buckets of every length around the small / large hand-over (64), around powers of two up to 2048 (the
    bitonic network's mirrored step and its skipped comparators) and around one and two strides of the 1024-thread
    workgroup, at ADJACENT hashes in this order, so that a write past a bucket's end lands in the next bucket.  Bucket 0
    holds 65 entries and bucket modulo - 1 holds 64; every other bucket is empty."""
    M, rng = 4099, np.random.default_rng(1001)
    lengths = {THRESHOLD_FIRST_HASH + i: c for i, c in enumerate(THRESHOLD_LENGTHS)}
    lengths[0], lengths[M - 1] = 65, 64
    parts = [_bucket(rng, M, h, c) for h, c in lengths.items()]

    def check(c, m):
        _check_lengths(c, m)
        assert int(m.n_kmers.sum()) == sum(c.lengths.values()) and int((m.n_kmers > 0).sum()) == len(c.lengths)
        assert sorted(set(m.n_kmers[THRESHOLD_FIRST_HASH:THRESHOLD_FIRST_HASH + len(THRESHOLD_LENGTHS)].tolist())) == sorted(THRESHOLD_LENGTHS)
        for h, length in c.lengths.items():          # part distinct, part repeated, in every bucket that has room for both
            f = m.frequencies[m.hashes_to_index[h]:m.hashes_to_index[h] + length]
            assert length < 3 or ((f == 1).any() and (f > 1).any()), (h, length)
    return _finish("threshold", rng, parts, M, check, lengths=lengths)


CLIP_RUNS = (65_534, 65_535, 65_536, 65_537)


def clip():
    """Modulo 1009; four buckets (hashes 5, 105, 205, 305 — apart, so that a lookup of key +- 1 does not walk a heavy
    bucket) whose dominant k-mer occurs 65 534, 65 535, 65 536 and 65 537 times, each with 100 singletons and a second
    run of 70: frequencies 65 534, 65 535, 65 535, 65 535, and 1 / 70 for the others — the two binary searches of a large
    bucket that mixes long runs with singletons."""
    M, rng = 1009, np.random.default_rng(1002)
    parts, lengths, expected = [], {}, {}
    for i, run in enumerate(CLIP_RUNS):
        h = 5 + 100 * i
        keys = _keys(rng, M, h, 102)
        parts += [np.full(run, keys[0]), np.full(70, keys[1]), keys[2:]]
        lengths[h] = run + 70 + 100
        expected[int(keys[0])] = (min(run, CLIP), run)
        expected[int(keys[1])] = (70, 70)
        expected.update({int(k): (1, 1) for k in keys[2:]})

    def check(c, m):
        _check_lengths(c, m)
        for key, want in c.expected.items():
            assert _frequency_of(m, key) == want, (key, want)
        assert sorted(set(m.frequencies.tolist())) == [1, 70, 65_534, 65_535]
    return _finish("clip", rng, parts, M, check, lengths=lengths, expected=expected)


def many_big():
    """Modulo 1500 and 200 000 entries: every bucket near 137 entries, 40 buckets forced to exactly 65 — more large
    buckets than the 1024 workgroups that order them, so that workgroups take a second bucket."""
    M, rng = 1500, np.random.default_rng(1003)
    forced = list(range(7, M, 37))[:40]
    free = np.setdiff1d(np.arange(M), forced)
    rest = _with_duplicates(rng, _any_keys(rng, M, free[rng.integers(0, free.shape[0], size=200_000)]))
    parts = [rest] + [_bucket(rng, M, h, 65) for h in forced]

    def check(c, m):
        _check_lengths(c, m)
        assert int((m.n_kmers > BIG).sum()) >= 1100, int((m.n_kmers > BIG).sum())
        assert int((m.n_kmers == BIG + 1).sum()) >= 40
    return _finish("many_big", rng, parts, M, check, lengths={h: 65 for h in forced})


def one_bucket(n):
    """Modulo 1: one bucket for everything, just above the threshold (65) and at size (70 001, with a run of 3000)."""
    n, rng = int(n), np.random.default_rng(1004 + int(n))
    keys = _with_duplicates(rng, rng.integers(0, TOP, size=n, dtype=np.uint64, endpoint=True), 0.3)
    if n > 3000:
        keys[:3000] = keys[0]

    def check(c, m):
        _check_lengths(c, m)
        assert m.n_kmers.shape == (1,) and int(m.frequencies.max()) >= (3000 if n > 3000 else 2)
    return _finish("one_bucket-%d" % n, rng, [keys], 1, check, lengths={0: n})


def _placed(name, M, placed, seed, doc_n=5000):
    """About 5000 entries: three in every bucket of `placed` that exists, the rest anywhere."""
    M, rng = int(M), np.random.default_rng(seed)
    placed = sorted({h for h in placed if 0 <= h < M})
    parts = [_bucket(rng, M, h, 3) for h in placed]
    parts.append(_with_duplicates(rng, rng.integers(0, TOP, size=doc_n, dtype=np.uint64, endpoint=True)))

    def check(c, m):
        assert all(int(m.n_kmers[h]) >= 3 for h in c.placed), c.name
        assert int(m.n_kmers.sum()) == c.kmers.shape[0]
        if c.modulo > 2 * doc_n:
            assert int((m.n_kmers == 0).sum()) > c.modulo // 2          # empty buckets between used ones
            assert int(m.hashes_to_index[c.modulo - 1]) > 0
    return _finish("%s-%d" % (name, M), rng, parts, M, check, placed=placed)


SCAN_SEAM_MODULI = (1, 2, 1023, 1024, 1025, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 20) + 1025)


def scan_seams(M):
    """Entries on both sides of the scan's block boundaries (1024 buckets per block, 2^20 per block of blocks) and in the
    last bucket; 2^20 + 1025 puts two blocks on the scan's second level."""
    M = int(M)
    return _placed("scan_seams", M, (0, 1022, 1023, 1024, 1025, M - 1, (1 << 20) - 1, 1 << 20, (1 << 20) + 1), 1100 + M % 997)


WIDE_MODULI = ((1 << 24) + 1, (1 << 24) + 1025)
MODULO_GRID = 65_536 * 256   # threads of the largest grid of the per-bucket kernels


def wide_modulo(M):
    """More buckets than the per-bucket kernels have threads: entries in bucket 0, on both sides of 2^24 and in the last."""
    M = int(M)
    assert M > MODULO_GRID
    return _placed("wide_modulo", M, (0, (1 << 24) - 1, 1 << 24, M - 1), 1200 + M % 997)


def long_input():
    """65 536 x 256 + 300 entries, modulo 1 000 003: more entries than the per-entry kernels have threads; random 64-bit
    k-mers, a fifth of them copies of others."""
    M, n, rng = 1_000_003, ENTRY_GRID + 300, np.random.default_rng(1005)
    keys = _with_duplicates(rng, rng.integers(0, TOP, size=n, dtype=np.uint64, endpoint=True))

    def check(c, m):
        assert c.kmers.shape[0] == ENTRY_GRID + 300 and int(m.n_kmers.max()) <= BIG and int(m.frequencies.max()) >= 2
    return _finish("long_input", rng, [keys], M, check)


def high_bits(M):
    """50 000 k-mers from the whole uint64 range, with 0, 2^62 - 1, 2^62, 2^63 - 1, 2^63, 2^64 - 1 and the multiples of the
    modulo nearest 2^64, +- 1 (each twice, under two nodes)."""
    M, rng = int(M), np.random.default_rng(1300 + int(M) % 997)
    k = TOP // M
    special = [0, (1 << 62) - 1, 1 << 62, (1 << 63) - 1, 1 << 63, TOP]
    special += [v for q in (k - 1, k) for v in (q * M - 1, q * M, q * M + 1) if v <= TOP]
    special = np.array(sorted(set(special)), dtype=np.uint64)
    keys = _with_duplicates(rng, rng.integers(0, TOP, size=50_000, dtype=np.uint64, endpoint=True))

    def check(c, m):
        assert np.isin(c.special, m.kmers).all()
        assert all(_frequency_of(m, int(s))[0] >= 2 for s in c.special)
        assert int(m.n_kmers[0]) >= 4 and int(m.n_kmers[c.modulo - 1]) >= 2      # 0, k M, (k - 1) M; k M - 1
        assert int((m.kmers >> np.uint64(62) == np.uint64(1)).sum()) > 10_000    # bit 62 without bit 63
    return _finish("high_bits-%d" % M, rng, [keys, special, special], M, check, special=special)


def empty(M):
    """No entries: the directory alone."""
    def check(c, m):
        assert m.kmers.shape == (0,) and not m.n_kmers.any() and not m.hashes_to_index.any()
    return _finish("empty-%d" % int(M), np.random.default_rng(1), [], int(M), check)


def single(M):
    """One entry: the k-mer 2^64 - 1 under node 2^31 - 1."""
    def check(c, m):
        h = TOP % c.modulo
        assert m.kmers.tolist() == [TOP] and m.nodes.tolist() == [(1 << 31) - 1] and m.frequencies.tolist() == [1]
        assert int(m.n_kmers[h]) == 1 and int(m.n_kmers.sum()) == 1 and not m.hashes_to_index.any()
    return _finish("single-%d" % int(M), np.random.default_rng(2), [np.array([TOP], dtype=np.uint64)], int(M), check)


CASES = (["threshold", "clip", "many_big", "one_bucket-65", "one_bucket-70001"]
         + ["scan_seams-%d" % M for M in SCAN_SEAM_MODULI] + ["wide_modulo-%d" % M for M in WIDE_MODULI]
         + ["long_input"] + ["high_bits-%d" % M for M in HIGH_BITS_MODULI]
         + ["empty-%d" % M for M in (1, 5, 1024, 1025, (1 << 20) + 1)]
         + ["single-%d" % M for M in (1, 2, 1025, (1 << 20) + 1)])
LARGE_BUCKET_CASES = ("threshold", "clip", "many_big", "one_bucket-65", "one_bucket-70001", "scan_seams-1", "scan_seams-2")
OVER_A_MILLION = ("long_input",) + tuple("wide_modulo-%d" % M for M in WIDE_MODULI) + ("high_bits-%d" % HIGH_BITS_MODULI[1],)


@functools.lru_cache(maxsize=None)
def build(name):
    """The case of that name; built once per process, its arrays read-only."""
    assert name in CASES, name
    fn, _, arg = name.partition("-")
    return globals()[fn](int(arg)) if arg else globals()[fn]()


def first_difference(case, got, want):
    """Where two results for `case` part, for a failure message: the first array that differs, the first differing
    position in it, and for the per-entry arrays the bucket that position lies in (by `want`'s directory), its length and
    on which side of the small / large hand-over it is."""
    got, want = Index(*got), Index(*want)
    for field in Index._fields:
        x, y = np.asarray(getattr(got, field)), np.asarray(getattr(want, field))
        if x.dtype != y.dtype or x.shape != y.shape:
            return "%s: %s: dtype / shape %s %s, expected %s %s" % (case.name, field, x.dtype, x.shape, y.dtype, y.shape)
        bad = np.flatnonzero(x != y)
        if not bad.size:
            continue
        p = int(bad[0])
        msg = "%s: %s differs at %d of %d positions, first at %d: got %d, expected %d" % (case.name, field, bad.size, x.size, p, int(x[p]), int(y[p]))
        if field in ("hashes_to_index", "n_kmers"):
            return msg + " (bucket %d of %d, expected length %d)" % (p, case.modulo, int(want.n_kmers[p]))
        ends = np.cumsum(want.n_kmers.astype(np.int64))
        h = int(np.searchsorted(ends, p, side="right"))
        c = int(want.n_kmers[h])
        return msg + " (bucket %d: entries %d..%d, length %d, %s the hand-over at %d)" % (
            h, int(ends[h]) - c, int(ends[h]) - 1, c, "above" if c > BIG else "at or below", BIG)
    return None
