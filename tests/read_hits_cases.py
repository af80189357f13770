"""Catalogue of kmm_read_hits cases (include/kmm.h) and an independent model of the call.

model(index_arrays, bases, offsets, k, max_freq, revcomp, lut) -> (hits, windows) is numpy over the five index arrays: a
sorted table from k-mer to the smallest frequency among its entries.  It uses neither the product nor the oracle; the
reverse complement is taken from the base codes (complement, read backwards), not from the packed integer.

The kernel's seams: a lane takes 4 consecutive flat positions, a wavefront 256, a tile (one round of a workgroup) 1024.
A case is a batch of reads with one index, one k and one rule at most (frequency filter, reverse complement, break table);
without_rule(case) is the same batch with the rule off.  Every case carries the reads that keep it from being vacuous
(conditions()): one with 0 < hits < windows, one with hits == 0 < windows, one with windows == 0 — the last cannot exist in a
batch of equal-length reads of k bases or more without a break table, which is the one exemption (Case.needs_no_windows).
"""
from collections import namedtuple

import numpy as np

from kmer_mapper_amd import synthetic
from kmer_mapper_amd.kmer_index import KmerIndex
from kmer_mapper_amd.util import LUT_BREAK, ambiguous_skip_lut, default_lut

LANE, WAVE, TILE = 4, 256, 1024
NO_FILTER = 65535
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

Case = namedtuple("Case", "name index k bases offsets max_freq revcomp lut rule")


def index_arrays(index):
    return (np.asarray(index._hashes_to_index), np.asarray(index._n_kmers), int(index._modulo), np.asarray(index._kmers),
            np.asarray(index._frequencies))


# ------------------------------------------------------------------------------------------------ the model
def _min_freq_table(index_arrays_):
    """(sorted distinct k-mers reachable through their bucket, smallest frequency of each)"""
    h2i, nk, modulo, kmers, freqs = index_arrays_
    reach = np.zeros(kmers.shape[0], dtype=bool)
    for h in np.nonzero(nk > 0)[0]:
        lo = int(h2i[h])
        sl = slice(lo, lo + int(nk[h]))
        reach[sl] |= (kmers[sl] % np.uint64(modulo)) == np.uint64(h)
    km, fr = kmers[reach], freqs[reach].astype(np.int64)
    order = np.lexsort((fr, km))
    km, fr = km[order], fr[order]
    first = np.ones(km.shape[0], dtype=bool)
    first[1:] = km[1:] != km[:-1]
    return km[first], fr[first]


def _present(table, q, max_freq):
    km, fr = table
    if km.shape[0] == 0:
        return np.zeros(q.shape[0], dtype=bool)
    i = np.minimum(np.searchsorted(km, q), km.shape[0] - 1)
    return (km[i] == q) & (fr[i] <= max_freq)


def model(index_arrays_, bases, offsets, k, max_freq=NO_FILTER, revcomp=False, lut=None):
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_reads, total = offsets.shape[0] - 1, bases.shape[0]
    lut = default_lut() if lut is None else np.asarray(lut, dtype=np.uint8)
    ent = lut[bases]
    if (ent == 0xFF).any():
        raise ValueError("invalid base at %d" % int(np.nonzero(ent == 0xFF)[0][0]))
    hits = np.zeros(n_reads, dtype=np.uint32)
    windows = np.zeros(n_reads, dtype=np.uint32)
    n_pos = total - k + 1
    if n_pos <= 0:
        return hits, windows
    lens = np.diff(offsets)
    end_of = np.repeat(offsets[1:], lens)                           # end of the read that holds position p
    brk = np.concatenate([[0], np.cumsum(ent == LUT_BREAK)])
    p = np.arange(n_pos, dtype=np.int64)
    valid = (p + k <= end_of[:n_pos]) & (brk[p + k] == brk[p])
    codes = (ent & 3).astype(np.uint64)
    q = np.zeros(n_pos, dtype=np.uint64)
    rc = np.zeros(n_pos, dtype=np.uint64)
    for j in range(k):
        q |= codes[j:j + n_pos] << np.uint64(2 * j)
        rc |= (np.uint64(3) - codes[k - 1 - j:k - 1 - j + n_pos]) << np.uint64(2 * j)
    table = _min_freq_table(index_arrays_)
    hit = _present(table, q, max_freq)
    if revcomp:
        hit |= _present(table, rc, max_freq)
    hit &= valid
    ch = np.concatenate([[0], np.cumsum(hit), ]).astype(np.int64)
    cw = np.concatenate([[0], np.cumsum(valid)]).astype(np.int64)
    lo, hi = np.minimum(offsets[:-1], n_pos), np.minimum(offsets[1:], n_pos)
    hits[:] = (ch[hi] - ch[lo]).astype(np.uint32)
    windows[:] = (cw[hi] - cw[lo]).astype(np.uint32)
    return hits, windows


def run_model(case):
    return model(index_arrays(case.index), case.bases, case.offsets, case.k, case.max_freq, case.revcomp, case.lut)


def without_rule(case):
    return case._replace(max_freq=NO_FILTER if case.rule == "filter" else case.max_freq,
                         revcomp=False if case.rule == "revcomp" else case.revcomp,
                         lut=None if case.rule == "break" else case.lut, rule=None)


def uniform_length(case):
    lens = np.diff(case.offsets)
    return int(lens[0]) if lens.shape[0] and (lens == lens[0]).all() and lens[0] > 0 else None


def needs_no_windows(case):
    """False only where a read without windows cannot exist: equal lengths of k bases or more, no break table."""
    L = uniform_length(case)
    return not (L is not None and L >= case.k and case.lut is None)


def conditions(case, hits, windows):
    """The three kinds of read every case holds (see the module's docstring); returns the list of what is missing."""
    missing = []
    if not ((hits > 0) & (hits < windows)).any():
        missing.append("0 < hits < windows")
    if not ((hits == 0) & (windows > 0)).any():
        missing.append("hits == 0 < windows")
    if needs_no_windows(case) and not (windows == 0).any():
        missing.append("windows == 0")
    return missing


# ------------------------------------------------------------------------------------------------ indexes
_GENOMES, _INDEXES = {}, {}


def genome(seed=11, n=20_000):
    if (seed, n) not in _GENOMES:
        _GENOMES[(seed, n)] = synthetic.make_genome(n + 64, seed)
    return _GENOMES[(seed, n)]


def _first_base_c(k):
    """All k-mers whose first base is C: what the small-k indexes hold (4^k / 4 of them; no run of A or T among them)."""
    rest = np.arange(4 ** (k - 1), dtype=np.uint64)
    return (rest << np.uint64(2)) | np.uint64(1)


def genome_index(k, modulo=None, several_nodes=True, seed=11):
    """k >= 16: the k-mers at every fourth position of the 20 kb genome; several_nodes: every 50th of them under two or three
    further nodes.  k <= 5: the k-mers that start with C.  Frequencies are the entry counts (KmerIndex.from_flat_kmers)."""
    key = (k, modulo, several_nodes, seed)
    if key not in _INDEXES:
        if k <= 5:
            kmers = _first_base_c(k)
        else:
            kmers = synthetic.pack_kmers_strided(genome(seed), 5000, 4, k)
        nodes = np.arange(kmers.shape[0], dtype=np.int64)
        if several_nodes:
            extra = np.concatenate([kmers[::50], kmers[::100]])
            kmers = np.concatenate([kmers, extra])
            nodes = np.concatenate([nodes, np.arange(extra.shape[0], dtype=np.int64) % 97])
        _INDEXES[key] = KmerIndex.from_flat_kmers(kmers, nodes, modulo or synthetic.next_prime(2 * kmers.shape[0]))
    return _INDEXES[key]


def index_of(kmers, modulo=None):
    kmers = np.asarray(kmers, dtype=np.uint64)
    return KmerIndex.from_flat_kmers(kmers, np.arange(kmers.shape[0], dtype=np.int64), modulo or synthetic.next_prime(2 * kmers.shape[0] + 3))


# ------------------------------------------------------------------------------------------------ reads
def gslice(start, n, seed=11):
    return ACGT[genome(seed)[start:start + n]]


def random_read(n, seed):
    return ACGT[np.random.Generator(np.random.PCG64(seed)).integers(0, 4, size=n, dtype=np.uint8)]


def batch(reads):
    reads = [np.asarray(r, dtype=np.uint8) for r in reads]
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([r.shape[0] for r in reads], out=offsets[1:])
    return (np.concatenate(reads) if reads else np.zeros(0, np.uint8)), offsets


def trio(k):
    """A read with some hits, one with windows and no hit (a run of T: neither it nor its complement starts with C or lies in
    the genome's sample), one without windows."""
    mixed = gslice(1000, k + 60) if k > 5 else random_read(k + 60, 77)
    return [mixed, np.full(k + 10, ord("T"), np.uint8), gslice(40, k - 1)]


def reads_ending_at(ends, k, seed=11):
    """Consecutive genome slices whose flat ends are `ends` (increasing)."""
    out, at, g = [], 0, 0
    for e in ends:
        out.append(gslice(g, e - at, seed))
        g = (g + e - at + 3) % 15_000
        at = e
    return out


def make(name, index, k, reads, max_freq=NO_FILTER, revcomp=False, lut=None, rule=None):
    bases, offsets = batch(reads)
    return Case(name, index, k, bases, offsets, max_freq, revcomp, lut, rule)


# ------------------------------------------------------------------------------------------------ the cases
def seam_cases():
    ends = sorted({s + d for s in (LANE, 2 * LANE, WAVE, 2 * WAVE, TILE, 2 * TILE, 3 * TILE) for d in (-1, 0, 1)})
    out = []
    for k in (1, 2, 16, 31):
        reads = reads_ending_at(ends, k) + [gslice(300, 3000), gslice(5000, 2 * TILE + 452)] + trio(k)
        if k <= 5:          # (the genome's slices under a small-k index: a quarter of the windows start with C)
            reads.append(random_read(500, 5))
        out.append(make("seams_k%d" % k, genome_index(k), k, reads))
    return out


def empty_cases():
    out = []
    for k in (2, 31):
        e = np.zeros(0, np.uint8)
        reads = [e, e, e, gslice(10, 200), e, gslice(700, 90), e, e] + trio(k) + [gslice(900, 1500)] + [e] * 2000 + \
                [gslice(2500, 333), e, gslice(3000, 50), e, e, e]
        out.append(make("empty_reads_k%d" % k, genome_index(k), k, reads))
    return out


def short_cases():
    out = []
    for k in (2, 16, 31):
        reads = []
        for i in range(120):
            reads.append(gslice(17 * i, (k - 1, k, k + 1, k, 0, k + 2)[i % 6]))
        out.append(make("short_reads_k%d" % k, genome_index(k), k, reads + trio(k)))
    for k in (2, 3, 4, 5):  # one lane's four windows belong to four reads
        rng = np.random.Generator(np.random.PCG64(100 + k))
        reads = [random_read(int(n), 1000 + i) for i, n in enumerate(rng.integers(k, k + 3, size=700))]
        out.append(make("tiny_reads_k%d" % k, genome_index(k), k, reads + trio(k)))
    return out


def uniform_cases():
    out = []
    for L, ks in ((15, (2,)), (16, (2, 5)), (150, (16, 31)), (151, (31,)), (1024, (31,)), (1025, (2, 31))):
        for k in ks:
            n = max(12, 9000 // L)
            if k <= 5:
                reads = [random_read(L, 300 + i) for i in range(n)]
            else:
                reads = [gslice((137 * i) % 15_000, L) for i in range(n)]
            reads[1] = np.full(L, ord("T"), np.uint8)
            out.append(make("uniform_L%d_k%d" % (L, k), genome_index(k), k, reads))
    return out


def filter_cases():
    """X: entries with frequencies 5, 50, 500 (a hit under the filter 100); Y: 200, 300 (no hit); Z: one entry, 100 (a hit:
    the filter is <=); the planted frequencies are written into the index arrays by hand."""
    out = []
    for k in (16, 31):
        g = genome()
        base = synthetic.pack_kmers_strided(g, 5000, 4, k)
        x, y, z = (synthetic.pack_kmers_at(g, [pos], k)[0] for pos in (402, 801, 1203))
        kmers = np.concatenate([base, [x, x, x, y, y, z]]).astype(np.uint64)
        index = index_of(kmers)
        fr = index._frequencies
        for km, values in ((x, (5, 50, 500)), (y, (200, 300)), (z, (100,))):
            where = np.nonzero(index._kmers == km)[0]
            assert where.shape[0] == len(values)
            fr[where] = values
        reads = [gslice(380, 80), gslice(790, 60), gslice(1190, 60), gslice(801, k), gslice(402, k)] + trio(k)
        out.append(make("filter_k%d" % k, index, k, reads, max_freq=100, rule="filter"))
    return out


def index_cases():
    out = []
    for k in (16, 31):
        reads = [gslice(0, 400), gslice(100, 2000), gslice(196, 231)] + trio(k)
        out.append(make("several_nodes_k%d" % k, genome_index(k), k, reads))
        out.append(make("modulo_257_k%d" % k, genome_index(k, modulo=257), k, reads + [random_read(3000, 9)]))
    out.append(make("modulo_3_k2", genome_index(2, modulo=3), 2, [random_read(900, 3)] + trio(2)))
    return out


def _rc_codes(codes):
    return (3 - codes[::-1]).astype(np.uint8)


def revcomp_cases():
    """Windows at genome positions 4 i hold q (i < 400); at 4 i + 1 only the reverse complement is in the index (i < 200);
    at 4 i + 2 both are (i < 200).  k = 16: the palindrome (ACGT)^4, once in the index."""
    out = []
    for k in (16, 31):
        g = genome()
        fwd = synthetic.pack_kmers_strided(g, 400, 4, k)
        both = synthetic.pack_kmers_at(g, 4 * np.arange(200) + 2, k)
        rcg = _rc_codes(g[:1000])                                   # rc of genome[p : p + k] = rcg[1000 - p - k : 1000 - p]
        rc_of = lambda pos: synthetic.pack_kmers_at(rcg, 1000 - np.asarray(pos) - k, k)
        kmers = [fwd, rc_of(4 * np.arange(200) + 1), both, rc_of(4 * np.arange(200) + 2)]
        reads = [gslice(0, 700), gslice(5, 120), gslice(401, 200)] + trio(k)
        if k == 16:
            pal = np.tile(np.frombuffer(b"ACGT", np.uint8), 12)
            kmers.append(synthetic.pack_kmers_at(np.tile(np.arange(4, dtype=np.uint8), 4), [0], k))
            reads.append(pal)
        out.append(make("revcomp_k%d" % k, index_of(np.unique(np.concatenate(kmers))), k, reads, revcomp=True, rule="revcomp"))
    return out


def break_cases():
    out = []
    lut = ambiguous_skip_lut()
    for k in (2, 16, 31):
        a = (gslice(0, 400) if k > 5 else random_read(400, 41)).copy()
        a[0] = ord("N")                                             # at a read's start
        b = (gslice(500, 700) if k > 5 else random_read(700, 42)).copy()
        b[[300, 301, 450]] = ord("n"), ord("N"), ord("N")           # in the middle; flat 400 + 623, 624 below: next to the tile seam
        b[[TILE - 400 - 1, TILE - 400]] = ord("N")
        c = (gslice(1300, 300) if k > 5 else random_read(300, 43)).copy()
        c[-1] = ord("N")                                            # at a read's end
        d = np.full(k + 5, ord("N"), np.uint8)                      # nothing but breaks: no windows
        e = (gslice(2000, 2 * TILE + 100) if k > 5 else random_read(2 * TILE + 100, 44)).copy()
        at = 400 + 700 + 300 + k + 5
        e[[2 * TILE - at + 1, 3 * TILE - at - 2]] = ord("N")        # one position behind / two before a seam
        out.append(make("breaks_k%d" % k, genome_index(k), k, [a, b, c, d, e] + trio(k), lut=lut, rule="break"))
    # equal lengths with a break table: the ragged front end with arithmetic read ids
    reads = [gslice(151 * i, 150).copy() for i in range(40)]
    reads[3][:] = ord("N")
    reads[5][70] = ord("N")
    reads[6][:] = ord("T")
    out.append(make("breaks_uniform_L150_k31", genome_index(31), 31, reads, lut=lut, rule="break"))
    return out


def large_case():
    """40 000 reads of 150 bases: workgroups loop over several tiles."""
    g = genome()
    starts = np.random.Generator(np.random.PCG64(8)).integers(0, 15_000, size=40_000)
    codes = g[starts[:, None] + np.arange(150)[None, :]]
    codes[::7] = np.random.Generator(np.random.PCG64(9)).integers(0, 4, size=codes[::7].shape, dtype=np.uint8)  # reads without hits
    bases = np.ascontiguousarray(ACGT[codes].reshape(-1))
    return Case("large_uniform_40000x150_k31", genome_index(31), 31, bases, np.arange(40_001, dtype=np.int64) * 150, 1000, False, None, None)


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = (seam_cases() + empty_cases() + short_cases() + uniform_cases() + filter_cases() + index_cases() + revcomp_cases() +
                break_cases() + [large_case()])
    return _ALL


_EXPECT = {}


def expected(case):
    """The model's answer, computed once per case and shared by the tests (read-only)."""
    if case.name not in _EXPECT:
        h, w = run_model(case)
        h.setflags(write=False)
        w.setflags(write=False)
        _EXPECT[case.name] = (h, w)
    return _EXPECT[case.name]
