"""Catalogue of cases for keeping mates together (include/kmm.h KEEPING MATES TOGETHER): paired-end reads as
interleaved FASTQ / two-line FASTA text, or as two texts whose i-th records are mates, whose kept pairs come back whole.

Expected values never come from the library, and the model shares nothing with the kernels: records() groups the lines of a
plain split at '\\n', their sequence lines go through the numpy hit model of tests/read_hits_cases.py, pair_keep applies the
pair rule in Python integers, and the kept text is a join of the kept records' bytes.  tests/test_record_pairs_on_the_cpu.py
holds the model to the oracle (extract -> in_index) and to the conditions that keep the catalogue from being vacuous.

The kernels' geometry the texts are placed against: a lane takes 16 bytes, a tile 1024, a scatter group four tiles (4096), a
super-tile 1024 tiles (1 MiB); the output leaves as aligned 16-byte lines with a ragged head and tail per group.
"""
from collections import namedtuple

import numpy as np

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests.record_keep_cases import hit_read, miss_read, _padded
from kmer_mapper_amd.util import ambiguous_skip_lut

LINE, TILE, GROUP, SUPER = 16, 1024, 4096, 1024 * 1024
ANY, BOTH = "any", "both"
K = 31

# text2 None: text1 holds the mates interleaved.  piece_kb: the "debug_records_piece_kb" the case is ALSO run under (0: none).
PCase = namedtuple("PCase", "name index k fmt text1 text2 min_hits min_permille invert pair_rule lut piece_kb")
Expect = namedtuple("Expect", "text1 text2 n_kept keep hits windows consumed1 consumed2 n_pairs")


# ------------------------------------------------------------------------------------------------ the model
def records(text, fmt):
    """[(the record's bytes, its sequence line without a '\\r')] of the whole records of `text`, by a plain split at '\\n'."""
    lines = bytes(text).split(b"\n")[:-1]                              # (what follows the last '\n' is no line)
    period = rh.PERIOD[fmt]
    out = []
    for r in range(len(lines) // period):
        rec = lines[r * period:(r + 1) * period]
        seq = rec[1][:-1] if rec[1].endswith(b"\r") else rec[1]
        out.append((b"".join(x + b"\n" for x in rec), seq))
    return out


def pair_keep(h1, w1, h2, w2, min_hits=1, min_permille=0, invert=False, pair_rule=ANY):
    """The pair rule of include/kmm.h in Python integers (no width to overflow)."""
    m1 = h1 >= min_hits and 1000 * h1 >= min_permille * w1
    m2 = h2 >= min_hits and 1000 * h2 >= min_permille * w2
    match = (m1 or m2) if pair_rule == ANY else (m1 and m2)
    return match != bool(invert)


def pair_keep_entries(hits, windows, **rule):
    """pair_keep over entries in pair order (2i: mate 1, 2i + 1: mate 2) -> one flag per pair."""
    h, w = hits.tolist(), windows.tolist()
    return np.array([pair_keep(h[i], w[i], h[i + 1], w[i + 1], **rule) for i in range(0, len(h), 2)], dtype=bool)


def rule_of(case):
    return dict(min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert, pair_rule=case.pair_rule)


def mates_of(case):
    """(records of mate 1, records of mate 2), as many of each: the whole pairs of the case."""
    if case.text2 is None:
        recs = records(case.text1, case.fmt)
        m = len(recs) // 2
        return recs[0:2 * m:2], recs[1:2 * m:2]
    r1, r2 = records(case.text1, case.fmt), records(case.text2, case.fmt)
    m = min(len(r1), len(r2))
    return r1[:m], r2[:m]


_EXPECT = {}


def expected(case):
    """Expect of the case, computed once and shared (read-only)."""
    if case.name not in _EXPECT:
        m1, m2 = mates_of(case)
        m = len(m1)
        seqs = [s for pair in zip(m1, m2) for (_, s) in pair]
        if seqs:
            bases, offsets = rh.reads_arrays(seqs)
            hits, windows = rc.model(rc.index_arrays(case.index), bases, offsets, case.k, rc.NO_FILTER, False, case.lut)
        else:
            hits = windows = np.zeros(0, dtype=np.uint32)
        keep = pair_keep_entries(hits, windows, **rule_of(case))
        len1, len2 = sum(len(b) for b, _ in m1), sum(len(b) for b, _ in m2)
        if case.text2 is None:
            text1 = b"".join(a[0] + b[0] for a, b, kp in zip(m1, m2, keep) if kp)
            text2, consumed1, consumed2 = None, len1 + len2, 0
        else:
            text1 = b"".join(a[0] for a, kp in zip(m1, keep) if kp)
            text2 = b"".join(b[0] for b, kp in zip(m2, keep) if kp)
            consumed1, consumed2 = len1, len2
        for a in (keep, hits, windows):
            a.setflags(write=False)
        _EXPECT[case.name] = Expect(text1, text2, int(keep.sum()), keep, hits, windows, consumed1, consumed2, m)
    return _EXPECT[case.name]


def interleave(text1, text2, fmt):
    """The whole pairs of two texts as one interleaved text (the equivalence the two-file call is held to)."""
    r1, r2 = records(text1, fmt), records(text2, fmt)
    return b"".join(a[0] + b[0] for a, b in zip(r1, r2))


def deinterleave(text, fmt):
    recs = records(text, fmt)
    return b"".join(r[0] for r in recs[0::2]), b"".join(r[0] for r in recs[1::2])


# ------------------------------------------------------------------------------------------------ writing pairs
def rec(fmt, seq, name, mate, seed=0):
    return rh.record(fmt, seq, name + b"/%d" % mate, seed=seed)


def two_texts(fmt, pairs, names=None):
    t1 = b"".join(rec(fmt, a, names[i] if names else b"p%d" % i, 1, seed=2 * i) for i, (a, _) in enumerate(pairs))
    t2 = b"".join(rec(fmt, b, names[i] if names else b"p%d" % i, 2, seed=2 * i + 1) for i, (_, b) in enumerate(pairs))
    return t1, t2


def interleaved_text(fmt, pairs):
    return b"".join(rec(fmt, a, b"p%d" % i, 1, seed=2 * i) + rec(fmt, b, b"p%d" % i, 2, seed=2 * i + 1) for i, (a, b) in enumerate(pairs))


def pattern_pairs():
    """The four hit patterns — mate 1 only, mate 2 only, both, neither — and the first once more; mates of different lengths."""
    return [(hit_read(100, 0), miss_read(90)), (miss_read(80), hit_read(120, 500)), (hit_read(70, 900), hit_read(75, 1300)),
            (miss_read(60), miss_read(65)), (hit_read(150, 2000), miss_read(100))]


def permille_pairs():
    """a: 8 hits in 30 windows (the index holds every fourth k-mer of the genome); b = a + 60 bases without a hit: the same hits
    over three times the windows.  A threshold of 150 per mille lies between them: one mate passes and the other fails, in
    either order."""
    a = hit_read(60, 2000)
    b = a + miss_read(60)
    return [(a, b), (b, a), (a, a), (b, b), (miss_read(80), miss_read(70))]


def break_pairs(k):
    """Under the break table a read of N alone has no window: it matches at min_hits 0 whatever the per-mille threshold says
    (200 here: the hit reads pass it with a quarter of their windows, the others fail it)."""
    n = b"N" * (k + 3)
    return [(n, hit_read(90, 100)), (hit_read(80, 700), n), (n, n), (miss_read(70), n), (miss_read(75), miss_read(66))]


def _end_at(fmt, seq, at, end, seed):
    """A record that starts at byte `at` of its text and ends (the byte behind its last '\\n') at `end`."""
    return _padded(fmt, seq, end - at, seed)


def _next_multiple(at, unit, least):
    """The first multiple of `unit` at or behind at + least."""
    return -(-(at + least) // unit) * unit


def seam_text(fmt=rh.FASTQ):
    """Interleaved pairs whose mate 1 ends exactly at a lane boundary that is no tile boundary, a tile boundary that is no
    group boundary, and a group boundary — so the mates lie on either side of it — then pairs whose mate 2 ends one byte
    before, at and one byte behind a tile boundary; (hit, miss) pairs at the seams, (miss, miss) and (hit, hit) between them.
    Returns (text, [(what, position)])."""
    parts, marks, at, i = [], [], 0, 0

    def add(r):
        nonlocal at
        parts.append(r)
        at += len(r)

    def filler():
        nonlocal i
        add(rec(fmt, miss_read(40 + i), b"m%d" % i, 1, seed=i))
        add(rec(fmt, miss_read(45 + i), b"m%d" % i, 2, seed=i))
        add(rec(fmt, hit_read(50 + i, 300 * i), b"h%d" % i, 1, seed=i))
        add(rec(fmt, hit_read(55 + i, 300 * i + 100), b"h%d" % i, 2, seed=i))
        i += 1

    bare = lambda n: len(rh.record(fmt, b"A" * n, b""))
    for what, unit, avoid in (("lane", LINE, TILE), ("tile", TILE, GROUP), ("group", GROUP, None)):
        filler()
        n = 60 + i
        end = _next_multiple(at, unit, bare(n) + 1)
        while avoid and end % avoid == 0:
            end += unit
        add(_end_at(fmt, hit_read(n, 400 * i), at, end, i))
        assert at == end
        marks.append((what, end))
        add(rec(fmt, miss_read(70 + i), b"s%d" % i, 2, seed=i))
    for d in (-1, 0, 1):
        filler()
        add(rec(fmt, miss_read(50 + i), b"e%d" % i, 1, seed=i))
        n = 80 + i
        end = _next_multiple(at, TILE, bare(n) + 2) + d
        add(_end_at(fmt, hit_read(n, 500 * i + 7), at, end, i))
        marks.append(("mate2 %+d" % d, end))
    filler()
    return b"".join(parts), marks


def super_seam_text():
    """Interleaved FASTQ just over 1 MiB: (hit, miss) and (miss, miss) pairs in turn up to the super-tile seam, a pair whose
    mate 1 ends exactly at the seam, and a few more pairs."""
    parts, at, i = [], 0, 0
    while at < SUPER - 4000:
        a = hit_read(150, 11 * i) if i % 2 == 0 else miss_read(150)
        for mate, seq in ((1, a), (2, miss_read(140))):
            r = rec(rh.FASTQ, seq, b"f%d" % i, mate, seed=i)
            parts.append(r)
            at += len(r)
        i += 1
    parts.append(_end_at(rh.FASTQ, hit_read(200, 4000), at, SUPER, 1))
    parts.append(rec(rh.FASTQ, miss_read(120), b"seam", 2, seed=2))
    tail = interleaved_text(rh.FASTQ, pattern_pairs())
    return b"".join(parts) + tail


def residue_texts(fmt=rh.FASTA):
    """Pairs alternately kept (hit, hit) and dropped (miss, miss).  Returns (interleaved, text1, text2): in the interleaved text
    the kept PAIRS end at 15, 16 and 17 modulo 16 of the output, three times over; in the two texts the kept RECORDS of each do,
    with different lengths in the two, so both queues pass those residues out of step with each other."""
    def build(sizes, mates):
        parts, out_len = [], 0
        for i, residue in enumerate((15, 16, 17) * 3):
            kept = [hit_read(sizes[0] + i, 100 * i), hit_read(sizes[1] + 2 * i, 100 * i + 50)]
            head = b"".join(rec(fmt, kept[j], b"k%d" % i, mates[j], seed=i) for j in range(len(mates) - 1))
            last = kept[len(mates) - 1]
            bare = len(rh.record(fmt, last, b""))
            total = bare + (residue - (out_len + len(head) + bare)) % LINE
            parts.append(head + _padded(fmt, last, total, i))
            out_len += len(head) + total
            assert out_len % LINE == residue % LINE
            for j, mate in enumerate(mates):
                parts.append(rec(fmt, miss_read(35 + 3 * i + j), b"d%d" % i, mate, seed=i))
        return b"".join(parts)

    return build((40, 47), (1, 2)), build((40, 0), (1,)), build((52, 0), (2,))


def piece_text(fmt=rh.FASTQ):
    """Records of exactly 300 bytes, pairs alternately kept and dropped: with pieces of 1 KiB every piece's byte limit falls inside
    a mate 2 whose mate 1 lies whole in front of it (records 3, 5, 7, ... of the text, counted from the pieces' starts)."""
    parts = []
    for i in range(8):
        a = hit_read(100, 200 * i) if i % 2 == 0 else miss_read(100)
        b = miss_read(90) if i % 4 < 2 else hit_read(90, 200 * i + 50)
        parts.append(_padded(fmt, a, 300, 2 * i))
        parts.append(_padded(fmt, b, 300, 2 * i + 1))
    return b"".join(parts)


def cut_texts(d, at_super=False):
    """Two FASTQ texts: the second holds m records, the first m + 3, and the m-th record of the first — where it is cut — ends
    d bytes from a tile boundary (at_super: from the super-tile seam; its records are long there, to keep the pairs few)."""
    n = 1300 if at_super else 120
    goal = SUPER if at_super else 3 * TILE
    parts, at, i = [], 0, 0
    bare = len(rh.record(rh.FASTQ, b"A" * n, b""))
    while at + 2 * (bare + 8) < goal + d:
        seq = hit_read(n, 37 * i) if i % 3 else miss_read(n)
        r = rec(rh.FASTQ, seq, b"c%d" % i, 1, seed=i)
        parts.append(r)
        at += len(r)
        i += 1
    parts.append(_end_at(rh.FASTQ, hit_read(n, 5000), at, goal + d, 3))
    m = len(parts)
    surplus = b"".join(rec(rh.FASTQ, hit_read(n, 900 * j), b"x%d" % j, 1, seed=j) for j in range(3))
    text2 = b"".join(rec(rh.FASTQ, miss_read(40) if j % 2 else hit_read(40, 61 * j), b"c%d" % j, 2, seed=j)
                     for j in range(m))
    return b"".join(parts) + surplus, text2


# ------------------------------------------------------------------------------------------------ the cases
def _mk(name, fmt, text1, text2=None, min_hits=1, min_permille=0, invert=False, pair_rule=ANY, lut=None, piece_kb=0, k=K):
    as_array = lambda t: None if t is None else np.frombuffer(bytes(t), dtype=np.uint8).copy()
    return PCase(name, rc.genome_index(k), k, fmt, as_array(text1), as_array(text2), min_hits, min_permille, invert, pair_rule, lut,
                 piece_kb)


RULES = [(ANY, False), (ANY, True), (BOTH, False), (BOTH, True)]


def _rule_name(pair_rule, invert):
    return pair_rule + ("_invert" if invert else "")


def _forms(name, fmt, pairs, **kw):
    """The same pairs interleaved and as two texts."""
    t1, t2 = two_texts(fmt, pairs)
    return [_mk(name.replace("{}", "interleaved"), fmt, interleaved_text(fmt, pairs), **kw), _mk(name.replace("{}", "two_files"), fmt, t1, t2, **kw)]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is not None:
        return _ALL
    out = []
    for fmt in (rh.FASTQ, rh.FASTA):                                  # 1. the four hit patterns
        for pair_rule, invert in RULES:
            out += _forms("patterns_%s_{}__%s" % (fmt, _rule_name(pair_rule, invert)), fmt, pattern_pairs(), pair_rule=pair_rule, invert=invert)
    for pair_rule, invert in RULES:
        out += _forms("permille_fastq_{}__150_%s" % _rule_name(pair_rule, invert), rh.FASTQ, permille_pairs(), min_permille=150,
                      pair_rule=pair_rule, invert=invert)
        out += _forms("breaks_fastq_{}__min_hits_0_permille_200_%s" % _rule_name(pair_rule, invert), rh.FASTQ, break_pairs(K), min_hits=0,
                      min_permille=200, pair_rule=pair_rule, invert=invert, lut=ambiguous_skip_lut())
    for fmt in (rh.FASTQ, rh.FASTA):                                  # 2. seams
        text = seam_text(fmt)[0]
        for pair_rule, invert in ((ANY, False), (BOTH, False), (ANY, True)):
            out.append(_mk("seams_%s_interleaved__%s" % (fmt, _rule_name(pair_rule, invert)), fmt, text, pair_rule=pair_rule, invert=invert))
    out.append(_mk("super_seam_fastq_interleaved__any", rh.FASTQ, super_seam_text()))
    both, one, two = residue_texts()
    out.append(_mk("residues_fasta_interleaved__any", rh.FASTA, both))
    out.append(_mk("residues_fasta_two_files__any", rh.FASTA, one, two))
    out.append(_mk("residues_fasta_two_files__both_invert", rh.FASTA, one, two, pair_rule=BOTH, invert=True))
    for fmt in (rh.FASTQ, rh.FASTA):                                  # 3. piece cuts
        out.append(_mk("pieces_%s_interleaved__any" % fmt, fmt, piece_text(fmt), piece_kb=1))
        t1, t2 = deinterleave(piece_text(fmt), fmt)
        out.append(_mk("pieces_%s_two_files__both" % fmt, fmt, t1, t2, pair_rule=BOTH, piece_kb=1))
    odd = interleaved_text(rh.FASTQ, pattern_pairs()) + rec(rh.FASTQ, hit_read(90, 40), b"lone", 1)      # 4. odd record counts
    out.append(_mk("odd_fastq_interleaved__any", rh.FASTQ, odd))
    out.append(_mk("odd_fasta_interleaved__both_invert", rh.FASTA, interleaved_text(rh.FASTA, pattern_pairs()[:3]) +
                   rec(rh.FASTA, miss_read(50), b"lone", 1) + b">cut/2\nACG", pair_rule=BOTH, invert=True))
    # 5. two files: mates of 150 and 100 bases; a surplus of one and of many records on either side
    long_short = [((hit_read(150, 160 * i) if i % 3 else miss_read(150)), (hit_read(100, 160 * i + 30) if i % 2 else miss_read(100)))
                  for i in range(12)]
    t1, t2 = two_texts(rh.FASTQ, long_short)
    r1, r2 = records(t1, rh.FASTQ), records(t2, rh.FASTQ)
    out.append(_mk("lengths_150_100_two_files__any", rh.FASTQ, t1, t2))
    for name, n1, n2 in (("first_one_more", 6, 5), ("first_many_more", 12, 5), ("second_one_more", 5, 6), ("second_many_more", 4, 12)):
        out.append(_mk("surplus_%s_two_files__both" % name, rh.FASTQ, b"".join(r[0] for r in r1[:n1]), b"".join(r[0] for r in r2[:n2]),
                       pair_rule=BOTH))
    out.append(_mk("surplus_incomplete_two_files__any", rh.FASTQ, t1[:-30], t2))   # (the last record of the first text is cut short)
    for d in (-1, 0, 1):
        t1, t2 = cut_texts(d)
        out.append(_mk("cut_at_tile_%+d_two_files__any" % d, rh.FASTQ, t1, t2))
        out.append(_mk("cut_at_tile_%+d_swapped_two_files__any" % d, rh.FASTQ, t2, t1))
        t1, t2 = cut_texts(d, at_super=True)
        out.append(_mk("cut_at_super_tile_%+d_two_files__any" % d, rh.FASTQ, t1, t2))
    out.append(_mk("empty_second_two_files__any", rh.FASTQ, two_texts(rh.FASTQ, pattern_pairs())[0], b""))
    out.append(_mk("empty_first_two_files__any", rh.FASTA, b"", two_texts(rh.FASTA, pattern_pairs())[1]))
    _ALL = out
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
