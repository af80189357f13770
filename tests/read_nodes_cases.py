"""Catalogue of kmm_read_nodes cases (include/kmm.h) and an independent model of the call.

The model shares no structure with the kernels: per read it splits the bytes at break bytes into break-free segments, walks
the five index arrays window by window (bucket q % modulo, every entry compared), tallies one vote per matching entry in a
dict, and takes the argmax with the tie rule (most votes, then the smallest node id).  The reverse complement is taken from
the base codes.  It uses neither the product nor the oracle; tests/test_read_nodes_on_the_cpu.py holds it to the oracle's
map_reads called read by read.

Geometry as tests/read_hits_cases.py (a lane takes 4 flat positions, a wavefront 256, a tile 1024), whose Case tuple, batch
helpers and genome this catalogue reuses.  The planted cases put single k-mers of the genome under chosen nodes so that a
read's votes are known by construction; PLANTED says where.
"""
from collections import namedtuple

import numpy as np

from kmer_mapper_amd import synthetic
from kmer_mapper_amd.kmer_index import KmerIndex
from kmer_mapper_amd.util import LUT_BREAK, ambiguous_skip_lut, default_lut
from tests import read_hits_cases as rc

LANE, WAVE, TILE = rc.LANE, rc.WAVE, rc.TILE
NO_FILTER = rc.NO_FILTER
MIN_TABLE_BYTES = 64 << 10                 # RN_MIN_TABLE_BYTES: 4096 slots, 2048 votes per round
Expected = namedtuple("Expected", "best_node best_votes second_votes total_votes n_nodes")
OUTPUTS = Expected._fields

BIG, SMALL, MID = 70_001, 9, 500           # node ids of the planted cases: one above 16 bits, met before the smaller ones


# ------------------------------------------------------------------------------------------------ the model
def _index_lists(index):
    key = id(index)
    if key not in _LISTS:
        _LISTS[key] = (index, np.asarray(index._hashes_to_index).tolist(), np.asarray(index._n_kmers).tolist(),
                       int(index._modulo), np.asarray(index._kmers).tolist(), np.asarray(index._nodes).tolist(),
                       np.asarray(index._frequencies).tolist())
    return _LISTS[key][1:]


_LISTS = {}


def _segments(ent):
    """(start, end) of the maximal runs of a read's table entries that hold no break"""
    brk = np.nonzero(ent == LUT_BREAK)[0].tolist()
    cuts = [-1] + brk + [ent.shape[0]]
    return [(a + 1, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a + 1]


def _pack(codes, k, reverse_complement=False):
    """The k-mers of every window of `codes` (first base in the lowest bits) as Python ints"""
    n = codes.shape[0] - k + 1
    q = np.zeros(n, dtype=np.uint64)
    c = codes.astype(np.uint64)
    for j in range(k):
        src = (np.uint64(3) - c[k - 1 - j:k - 1 - j + n]) if reverse_complement else c[j:j + n]
        q |= src << np.uint64(2 * j)
    return q.tolist()


def tally_read(index, bases, k, max_freq=NO_FILTER, revcomp=False, lut=None):
    """{node: votes} of one read, and the number of windows looked up"""
    h2i, nk, modulo, kmers, nodes, freqs = _index_lists(index)
    lut = default_lut() if lut is None else np.asarray(lut, dtype=np.uint8)
    ent = lut[np.asarray(bases, dtype=np.uint8)]
    if (ent == 0xFF).any():
        raise ValueError("invalid base at %d" % int(np.nonzero(ent == 0xFF)[0][0]))
    votes, windows = {}, 0
    for a, b in _segments(ent):
        if b - a < k:
            continue
        codes = ent[a:b] & 3
        for qs in ([_pack(codes, k)] + ([_pack(codes, k, True)] if revcomp else [])):
            for q in qs:
                h = q % modulo
                for l in range(h2i[h], h2i[h] + nk[h]):
                    if kmers[l] == q and freqs[l] <= max_freq:
                        votes[nodes[l]] = votes.get(nodes[l], 0) + 1
        windows += b - a - k + 1
    return votes, windows


def answer(votes):
    """(best_node, best_votes, second_votes, total_votes, n_nodes) of one read's tally"""
    if not votes:
        return -1, 0, 0, 0, 0
    ranked = sorted(votes.items(), key=lambda nv: (-nv[1], nv[0]))
    return ranked[0][0], ranked[0][1], (ranked[1][1] if len(ranked) > 1 else 0), sum(votes.values()), len(votes)


def tallies(case):
    """per read: ({node: votes}, windows); computed once per case"""
    if case.name not in _TALLIES:
        _TALLIES[case.name] = [tally_read(case.index, case.bases[case.offsets[r]:case.offsets[r + 1]], case.k, case.max_freq,
                                          case.revcomp, case.lut) for r in range(case.offsets.shape[0] - 1)]
    return _TALLIES[case.name]


_TALLIES, _EXPECT = {}, {}


def expected(case):
    """The model's five outputs, computed once per case and shared by the tests (read-only)."""
    if case.name not in _EXPECT:
        rows = [answer(v) for v, _ in tallies(case)]
        cols = list(zip(*rows)) if rows else [[]] * 5
        out = Expected(*(np.array(col, dtype=np.int32 if i == 0 else np.uint32) for i, col in enumerate(cols)))
        for a in out:
            a.setflags(write=False)
        _EXPECT[case.name] = out
    return _EXPECT[case.name]


# ------------------------------------------------------------------------------------------------ indexes
_INDEXES = {}
_BLOCK_IDS = ((np.arange(75, dtype=np.int64) * 7919 + SMALL) % (BIG + 1))      # block 0 is node 9; ids up to 70 001


def _cached(key, make_index):
    if key not in _INDEXES:
        _INDEXES[key] = make_index()
    return _INDEXES[key]


def pos_index(k, entries, modulo=None, extra=()):
    """entries: (genome positions, node id or ids) pairs -> an index holding the genome's k-mer at every position under the
    node(s); extra: (kmers, nodes) pairs taken as they are"""
    g = rc.genome()
    kmers, nodes = [], []
    for pos, node in entries:
        pos = np.atleast_1d(np.asarray(pos, dtype=np.int64))
        kmers.append(synthetic.pack_kmers_at(g, pos, k))
        nodes.append(np.broadcast_to(np.asarray(node, dtype=np.int64), pos.shape))
    for km, nd in extra:
        kmers.append(np.asarray(km, dtype=np.uint64))
        nodes.append(np.broadcast_to(np.asarray(nd, dtype=np.int64), kmers[-1].shape))
    kmers, nodes = np.concatenate(kmers), np.concatenate(nodes)
    return KmerIndex.from_flat_kmers(kmers, nodes, modulo or synthetic.next_prime(2 * kmers.shape[0] + 3))


def block_index(k, modulo=None):
    """Every position of the genome's first 15 000 under the node of its block of 200 (_BLOCK_IDS); every 50th k-mer also
    under the next block's node, every 100th under a third."""
    def make_index():
        p = np.arange(15_000)
        return pos_index(k, [(p, _BLOCK_IDS[p // 200]), (p[::50], _BLOCK_IDS[(p[::50] // 200 + 1) % 75]),
                             (p[::100], _BLOCK_IDS[(p[::100] // 200 + 2) % 75])], modulo)
    return _cached(("block", k, modulo), make_index)


def one_node_index(k=31):
    return _cached(("one", k), lambda: pos_index(k, [(np.arange(20_000), 12_345)]))


def fifty_node_index(k=31):
    ids = (np.arange(50, dtype=np.int64) * 1409 + 3) % 66_000
    return _cached(("fifty", k), lambda: pos_index(k, [(np.arange(15_000), ids[np.arange(15_000) // 300])]))


# Where the planted index puts which node (genome positions), and the reads cut over them.
PLANTED = {
    # a read that starts at flat 200 and crosses the wavefront seam (flat 256) at its offset 56
    "wave": dict(start=2000, a_front=[2005, 2015, 2025], b=[2030, 2035, 2040, 2045, 2050], a_behind=[2060, 2070, 2080], seam=56),
    # a read that starts at flat 900 and crosses the tile seam (flat 1024) at its offset 124
    "tile": dict(start=3000, a_front=[3010, 3020, 3030], b=[3040, 3050, 3060, 3070, 3080], a_behind=[3130, 3140, 3150], seam=124),
}


def planted_index(k=31):
    def make_index():
        entries = []
        for spec in PLANTED.values():
            entries += [(spec["a_front"] + spec["a_behind"], BIG), (spec["b"], SMALL)]
        entries += [([100, 110, 120], BIG), ([130, 140, 150], SMALL)]                   # a tie: the smaller id is met second
        entries += [([410, 415], MID), ([420, 425], BIG), ([430, 435], SMALL)]          # a three-way tie
        entries += [([600], 5), ([600], 6), ([600], 7)]                                  # one k-mer under three nodes
        entries += [(np.arange(5000, 5120), 1000 + 3 * np.arange(120))]                  # 120 windows, 120 nodes
        return pos_index(k, entries)
    return _cached(("planted", k), make_index)


def filter_index(k=31):
    """The k-mer at 700 under nodes 20 (frequency 500) and 30 (5); 710 and 712 under 20 (200); 720 under 30 (5).  Without the
    filter node 20 wins 3 : 2, under max_freq 100 it has no vote left."""
    def make_index():
        index = pos_index(k, [([700, 710, 712], 20), ([700, 720], 30)])
        fr, nodes = index._frequencies, np.asarray(index._nodes)
        fr[nodes == 20] = 200
        fr[nodes == 30] = 5
        x = synthetic.pack_kmers_at(rc.genome(), [700], k)[0]
        fr[(np.asarray(index._kmers) == x) & (nodes == 20)] = 500
        return index
    return _cached(("filter", k), make_index)


def revcomp_index(k):
    """Node 1: the genome's k-mers at 4 i (i < 100); node 2: the reverse complements of those at 1000 + 4 i; k = 16: node 3,
    the palindrome (ACGT)^4."""
    def make_index():
        g = rc.genome()
        rcg = rc._rc_codes(g[:2000])                                # rc of genome[p : p + k] = rcg[2000 - p - k : 2000 - p]
        extra = [(synthetic.pack_kmers_at(rcg, 2000 - (1000 + 4 * np.arange(100)) - k, k), 2)]
        if k == 16:
            extra.append((synthetic.pack_kmers_at(np.tile(np.arange(4, dtype=np.uint8), 4), [0], k), 3))
        return pos_index(k, [(4 * np.arange(100), 1)], extra=extra)
    return _cached(("revcomp", k), make_index)


# ------------------------------------------------------------------------------------------------ the cases
gslice, make = rc.gslice, rc.make


def seam_cases():
    ends = sorted({s + d for s in (LANE, 2 * LANE, WAVE, 2 * WAVE, TILE, 2 * TILE, 3 * TILE) for d in (-1, 0, 1)})
    out = []
    for k in (2, 31):
        index = block_index(k) if k > 5 else rc.genome_index(k)
        reads = rc.reads_ending_at(ends, k) + [gslice(300, 3000), gslice(5000, 2 * TILE + 452)] + rc.trio(k)
        if k <= 5:
            reads.append(rc.random_read(500, 5))
        out.append(make("seams_k%d" % k, index, k, reads))
    return out


def seam_winner_case():
    """The case the design exists for: node B wins the part of the read in front of the seam, node A the read."""
    w, t = PLANTED["wave"], PLANTED["tile"]
    reads = [gslice(9000, 200), gslice(w["start"], 300), gslice(9300, 400), gslice(t["start"], 300)]
    case = make("seam_winner_k31", planted_index(), 31, reads)
    assert case.offsets[1] + w["seam"] == WAVE and case.offsets[3] + t["seam"] == TILE
    return case


SEAM_READS = {1: PLANTED["wave"]["seam"], 3: PLANTED["tile"]["seam"]}   # read of seam_winner_k31 -> its offset at the seam


def planted_cases():
    hitless = gslice(9000, 90)                                      # a read without hits between reads with hits
    return [seam_winner_case(),
            make("ties_k31", planted_index(), 31, [gslice(90, 100), hitless, gslice(400, 80)]),
            make("three_nodes_k31", planted_index(), 31, [gslice(590, 60), hitless, gslice(95, 40)]),
            make("many_nodes_k31", planted_index(), 31, [gslice(5000, 150), gslice(8000, 150), gslice(5100, 150)])]


def filter_case():
    return make("filter_k31", filter_index(), 31, [gslice(690, 80), gslice(9000, 60), gslice(715, 40)], max_freq=100, rule="filter")


def revcomp_cases():
    out = []
    for k in (16, 31):
        reads = [gslice(0, 200), gslice(1000, 200), gslice(9000, 100), gslice(390, 700)]
        if k == 16:
            reads.append(np.tile(np.frombuffer(b"ACGT", np.uint8), 12))
        out.append(make("revcomp_k%d" % k, revcomp_index(k), k, reads, revcomp=True, rule="revcomp"))
    return out


def break_cases():
    out = []
    lut = ambiguous_skip_lut()
    for k in (2, 31):
        index = block_index(k) if k > 5 else rc.genome_index(k)
        a = (gslice(0, 400) if k > 5 else rc.random_read(400, 41)).copy()
        a[0] = ord("N")                                             # at a read's start
        b = (gslice(500, 700) if k > 5 else rc.random_read(700, 42)).copy()
        b[[300, 301, 450]] = ord("n"), ord("N"), ord("N")           # in the middle
        b[[TILE - 400 - 1, TILE - 400]] = ord("N")                  # flat 1023, 1024: next to the tile seam
        c = (gslice(1300, 300) if k > 5 else rc.random_read(300, 43)).copy()
        c[-1] = ord("N")                                            # at a read's end
        d = np.full(k + 5, ord("N"), np.uint8)                      # nothing but breaks
        e = (gslice(2000, 2 * TILE + 100) if k > 5 else rc.random_read(2 * TILE + 100, 44)).copy()
        at = 400 + 700 + 300 + k + 5
        e[[2 * TILE - at + 1, 3 * TILE - at - 2]] = ord("N")        # one position behind / two before a seam
        out.append(make("breaks_k%d" % k, index, k, [a, b, c, d, e] + rc.trio(k), lut=lut, rule="break"))
    reads = [gslice(151 * i, 150).copy() for i in range(40)]        # equal lengths with a break table
    reads[3][:] = ord("N")
    reads[5][70] = ord("N")
    reads[6][:] = ord("T")
    out.append(make("breaks_uniform_L150_k31", block_index(31), 31, reads, lut=lut, rule="break"))
    return out


def empty_and_short_cases():
    e = np.zeros(0, np.uint8)
    reads = [e, e, e, gslice(10, 200), e, gslice(700, 90), e, e] + rc.trio(31) + [gslice(900, 1500)] + [e] * 2000 + \
            [gslice(2500, 333), e, gslice(3000, 50), e, e, e]
    out = [make("empty_reads_k31", block_index(31), 31, reads)]
    for k in (2, 31):
        index = block_index(k) if k > 5 else rc.genome_index(k)
        reads = [gslice(17 * i, (k - 1, k, k + 1, k, 0, k + 2)[i % 6]) for i in range(120)]
        out.append(make("short_reads_k%d" % k, index, k, reads + rc.trio(k)))
    return out


def modulo_cases():
    reads = [gslice(0, 400), gslice(100, 2000), gslice(196, 231)] + rc.trio(31) + [rc.random_read(3000, 9)]
    return [make("modulo_257_k31", block_index(31, modulo=257), 31, reads),
            make("modulo_3_k2", rc.genome_index(2, modulo=3), 2, [rc.random_read(900, 3)] + rc.trio(2))]


def _uniform(name, index, starts, spoil_every=0):
    g = rc.genome()
    codes = g[starts[:, None] + np.arange(150)[None, :]]
    if spoil_every:                                                 # reads without hits
        codes[::spoil_every] = np.random.Generator(np.random.PCG64(9)).integers(0, 4, size=codes[::spoil_every].shape, dtype=np.uint8)
    bases = np.ascontiguousarray(rc.ACGT[codes].reshape(-1))
    return rc.Case(name, index, 31, bases, np.arange(starts.shape[0] + 1, dtype=np.int64) * 150, 1000, False, None, None)


def skew_cases():
    rng = np.random.Generator(np.random.PCG64(8))
    long_read = gslice(0, 20_000)
    return [make("long_read_one_node_k31", one_node_index(), 31, [long_read]),                     # one cell, many adders
            make("oversize_read_k31", one_node_index(), 31, [gslice(50, 100), long_read, gslice(700, 90)]),
            _uniform("one_node_3000x150_k31", one_node_index(), rng.integers(0, 19_800, size=3000)),  # many cells, one node
            _uniform("mixed_3000x150_k31", fifty_node_index(), rng.integers(0, 14_800, size=3000), spoil_every=7)]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = (seam_cases() + planted_cases() + [filter_case()] + revcomp_cases() + break_cases() + empty_and_short_cases() +
                modulo_cases() + skew_cases())
    return _ALL


def case(name):
    return next(c for c in all_cases() if c.name == name)


def first_node_met(case_, r):
    """The node of the first vote of read r in reading order (forward orientation first), or None"""
    read = case_.bases[case_.offsets[r]:case_.offsets[r + 1]]
    for p in range(read.shape[0] - case_.k + 1):
        votes, _ = tally_read(case_.index, read[p:p + case_.k], case_.k, case_.max_freq, case_.revcomp, case_.lut)
        if votes:
            return min(votes)
    return None
