"""Catalogue of cases for the base-quality floor of the record-hits mode ("record_hits_min_base_quality", include/kmm.h;
DESIGN 4.27): raw FASTQ text (and BAM / SAM records) whose low-quality bases are breaks for the per-record hits and windows.

Expected values never come from the library: parse_q(text) is a plain-Python FASTQ parser (tests/record_hits_cases.py's line
rule: split at '\\n', whole records, a '\\r' before it is not part of the line), the bases a floor kills are
tests/quality_cases.py's low_mask over the quality line — byte i of it belongs to byte i of the sequence line — and the hits and
windows are tests/read_hits_cases.py's model over the reads with those bases turned into breaks.
tests/test_record_hits_qual_on_the_cpu.py holds the catalogue to the conditions its cases exist for (and the model's windows to
quality_cases.surviving_windows).

The seams of the direct front end: a lane takes 4 consecutive bytes of the text, a staged vector 16, a wavefront 256, a tile
1024, the newline census a super-tile of 1 MiB; the mark pass takes 16 bytes per lane and 1024 per wavefront.
"""
from collections import namedtuple

import numpy as np

from tests import quality_cases as qc
from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from kmer_mapper_amd.util import ambiguous_skip_lut

LANE, VECTOR, WAVE, TILE, SUPER = rh.LANE, rh.VECTOR, rh.WAVE, rh.TILE, rh.SUPER
K, L = 31, 150
HIGH = ord("I")
DEAD_BYTE = 1                # a byte no sequence line holds: the model's stand-in for a base the floor killed
PIECE_KB = 4                 # "debug_records_piece_kb" of the several-pieces case

# text: uint8; q: the floor; lut: None or the skip table; marks: [(raw offset of a low base, of its quality byte, unit)];
# rule: None or (min_hits, min_permille); pairs: None, "any" or "both" (the text is interleaved mates)
QCase = namedtuple("QCase", "name index k text q lut marks rule pairs")
QRec = namedtuple("QRec", "start end seq_at seq qual_at qual qual_nl")


# ------------------------------------------------------------------------------------------------ the parser and the model
def parse_q(text):
    """([QRec], consumed): the whole four-line records of `text`."""
    text = bytes(text)
    lines, at = [], 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            break
        lines.append((at, nl))
        at = nl + 1
    recs = []
    for r in range(len(lines) // 4):
        (s_lo, s_hi), (q_lo, q_hi) = lines[4 * r + 1], lines[4 * r + 3]
        strip = lambda lo, hi: hi - 1 if hi > lo and text[hi - 1:hi] == b"\r" else hi
        recs.append(QRec(lines[4 * r][0], q_hi + 1, s_lo, text[s_lo:strip(s_lo, s_hi)], q_lo, text[q_lo:strip(q_lo, q_hi)], q_hi))
    return recs, (recs[-1].end if recs else 0)


def first_malformed(recs):
    """The raw offset of the '\\n' of the first quality line that is not as long as its sequence line, or None."""
    for r in recs:
        if len(r.seq) != len(r.qual):
            return r.qual_nl
    return None


def floor_lut(lut):
    """The lookup table with DEAD_BYTE as one more break."""
    out = (rc.default_lut() if lut is None else np.asarray(lut, dtype=np.uint8)).copy()
    out[DEAD_BYTE] = rc.LUT_BREAK
    return out


def reads_under_floor(seqs, quals, q, exempt=()):
    """(bases, offsets, mask) of the reads with the bases a floor of q kills replaced by DEAD_BYTE; exempt: reads that pass
    unmasked (BAM / SAM records that store no qualities)."""
    bases, offsets = rc.batch([np.frombuffer(s, dtype=np.uint8) for s in seqs])
    allq = np.concatenate([np.frombuffer(x, dtype=np.uint8) for x in quals] + [np.zeros(0, np.uint8)])
    mask = qc.low_mask(allq, q)
    for r in exempt:
        mask[offsets[r]:offsets[r + 1]] = False
    bases = bases.copy()
    bases[mask] = DEAD_BYTE
    return bases, offsets, mask


def model(index, k, seqs, quals, q, lut=None, revcomp=False, exempt=()):
    """(hits, windows, masked bases) per the definition: a low base is a break."""
    bases, offsets, mask = reads_under_floor(seqs, quals, q, exempt)
    h, w = rc.model(rc.index_arrays(index), bases, offsets, k, rc.NO_FILTER, revcomp, floor_lut(lut))
    return h, w, int(mask.sum())


Expected = namedtuple("Expected", "hits windows masked consumed n_records recs")
_EXPECT = {}


def expected(case, q=None):
    """The case under its floor (or another one: 0 is the floor-off model), computed once and shared (read-only)."""
    q = case.q if q is None else q
    if (case.name, q) not in _EXPECT:
        recs, consumed = parse_q(case.text)
        assert first_malformed(recs) is None
        h, w, masked = model(case.index, case.k, [r.seq for r in recs], [r.qual for r in recs], q, case.lut)
        h.setflags(write=False)
        w.setflags(write=False)
        _EXPECT[(case.name, q)] = Expected(h, w, masked, consumed, len(recs), recs)
    return _EXPECT[(case.name, q)]


def passes(hits, windows, rule):
    min_hits, min_permille = rule
    return (hits.astype(np.int64) >= min_hits) & (1000 * hits.astype(np.int64) >= min_permille * windows.astype(np.int64))


def kept(case, q=None):
    """(keep mask per record, the kept text): the rule over the expected entries, mates together under case.pairs."""
    e = expected(case, q)
    keep = passes(e.hits, e.windows, case.rule)
    if case.pairs:
        a, b = keep[0::2], keep[1::2]
        pair = (a | b) if case.pairs == "any" else (a & b)
        keep = np.repeat(pair, 2)
    text = bytes(case.text)
    return keep, b"".join(text[r.start:r.end] for r, on in zip(e.recs, keep) if on)


# ------------------------------------------------------------------------------------------------ writing records
def hit(n, at):
    return rc.gslice(at % 15_000, n).tobytes()


def miss(n, seed):
    return rc.random_read(n, 9000 + seed).tobytes()          # (no 31-mer of 20 kb of genome in random bases)


def quals_of(n, low=(), q=20, seed=0, high=HIGH):
    """n quality bytes: `high`, the floor's own byte (alive) on a few, and bytes below the floor at `low`."""
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    out = np.full(n, max(high, 33 + q), dtype=np.uint8)
    out[rng.random(n) < 0.03] = 33 + q
    for i, o in enumerate(low):
        out[o] = max(33, 33 + q - 1 - (i % 3) * 5)
    return out.tobytes()


def rec(seq, qual, head=b"r", plus=b"", eol=b"\n"):
    return b"@" + head + eol + seq + eol + b"+" + plus + eol + qual + eol


def _filler(n, seed, q=20, high=HIGH):
    """n ordinary records, one low base in each of them at a place that moves."""
    return b"".join(rec(hit(L, 211 * (seed + i)), quals_of(L, [(17 * (seed + i)) % L], q, seed + i, high), b"f%d" % (seed + i),
                        eol=b"\r\n" if i % 5 == 2 else b"\n") for i in range(n))


def make(name, text, q=20, k=K, lut=None, marks=(), rule=None, pairs=None):
    return QCase(name, rc.genome_index(k), k, np.frombuffer(bytes(text), dtype=np.uint8).copy(), q, lut, list(marks), rule, pairs)


# ------------------------------------------------------------------------------------------------ the seams
SEAM_UNITS = (LANE, VECTOR, WAVE, TILE)
SHIFTS = ("plain", "long_plus_line", "long_header")


def _aligned_record(at, unit, side, shift, i, o=40):
    """A record written at raw offset `at` whose base at offset o of the sequence line is low, with its header padded so that
    (side "base_last") that base is the last byte of a unit — its quality byte lies in a later one — or (side "qual_first") its
    quality byte is the first byte of a unit — the base lies in an earlier one.  shift: what lies between the two."""
    seq, qual = hit(L, 977 * i + 13), quals_of(L, [o, o + 1, L - 1], seed=i)
    plus = b"n" * (300 + 7 * i) if shift == "long_plus_line" else b""
    head = b"h" * (2500 if shift == "long_header" else 1)
    for pad in range(unit + 1):
        r = rec(seq, qual, head + b"x" * pad, plus)
        seq_at = at + 1 + len(head) + pad + 1
        qual_at = seq_at + L + 1 + 1 + len(plus) + 1
        if (side == "base_last" and (seq_at + o) % unit == unit - 1) or (side == "qual_first" and (qual_at + o) % unit == 0):
            return r, (seq_at + o, qual_at + o, unit)
    raise AssertionError("no padding aligns the record")


def seam_cases():
    out = []
    for unit in SEAM_UNITS:
        for side in ("base_last", "qual_first"):
            parts, marks, at = [_filler(3, 10 * unit)], [], 0
            at = len(parts[0])
            for i, shift in enumerate(SHIFTS):
                r, mark = _aligned_record(at, unit, side, shift, unit + i)
                parts += [r, _filler(2, 7 * unit + 3 * i)]
                marks.append(mark)
                at += len(r) + len(parts[-1])
            out.append(make("seam_%d_%s" % (unit, side), b"".join(parts), marks=marks))
    return out


def super_tile_case():
    """Just over 1 MiB: ordinary records up to the super-tile seam, then a record whose sequence line's last base is the last
    byte of the first super-tile — its '\\n', the '+' line and the whole quality line lie in the second one, whose census
    numbers their lines — with its first and last base low; then more records."""
    parts, at, i = [], 0, 0
    while at < SUPER - 3 * 320:
        parts.append(_filler(1, 1000 + i))
        at += len(parts[-1])
        i += 1
    head = b"s" * (SUPER - at - L - 2)
    seq_at = at + 1 + len(head) + 1
    assert seq_at + L == SUPER
    qual_at = SUPER + 3
    parts.append(rec(hit(L, 4000), quals_of(L, [0, 70, L - 1], seed=5), head))
    parts.append(_filler(6, 5000))
    return make("super_tile", b"".join(parts), marks=[(seq_at + L - 1, qual_at + L - 1, SUPER), (seq_at, qual_at, SUPER)])


# ------------------------------------------------------------------------------------------------ where the low bases lie
def position_cases():
    k = K
    recs = [rec(hit(L, 100), quals_of(L, [0])), rec(hit(L, 300), quals_of(L, [L - 1])),
            rec(hit(L, 500), quals_of(L, [k - 1])), rec(hit(L, 700), quals_of(L, [L - k])),
            rec(hit(L, 900), quals_of(L, range(50, 90))),                              # a run of 40
            rec(hit(L, 1100), quals_of(L, [40, 40 + k])),                              # k apart: no window between them
            rec(hit(L, 1300), quals_of(L, [40, 40 + k + 1])),                          # k + 1 apart: one
            rec(hit(k - 1, 1500), quals_of(k - 1, [3])),                               # shorter than k
            rec(b"", b""),                                                             # an empty sequence line
            rec(hit(k, 1700), quals_of(k, [k // 2])),
            rec(hit(L, 1900), quals_of(L, range(L))),                                  # all low
            rec(hit(L, 2100), quals_of(L, []))]
    return [make("positions", _filler(2, 40) + b"".join(recs) + _filler(2, 50))]


def value_cases():
    """33 + Q - 1 (dead) and 33 + Q (alive) side by side, for the smallest floor, the usual one and the largest; a byte below
    '!' (dead) and bytes of 0x80 and more (alive: compared as unsigned)."""
    out = []
    for q in (1, 20, 93):
        high = 126 if q == 93 else HIGH
        a = bytearray(quals_of(L, [], q, 1, high))
        a[60:62] = bytes([33 + q - 1, 33 + q])
        a[100:102] = bytes([33 + q, 33 + q - 1])
        b = bytearray(quals_of(L, [], q, 2, high))
        b[40], b[75], b[76], b[110] = 0x20, 0x80, 0xFF, 0x09
        text = _filler(2, 60, q, high)                                # (q 93: 'I' is below the floor, '~' throughout)
        out.append(make("values_q%d" % q, text + rec(hit(L, 2500), bytes(a), b"edge") + rec(hit(L, 2900), bytes(b), b"odd") + text, q=q))
    return out


def lookalike_crlf_case():
    """CRLF records whose quality lines start with '@' (Q31: alive) and with '+' (Q10: dead)."""
    recs = []
    for i in range(8):
        a = bytearray(quals_of(L, [60 + i], seed=i))
        a[0] = ord("@+"[i % 2:i % 2 + 1])
        recs.append(rec(hit(L, 333 * i + 7), bytes(a), b"c%d" % i, eol=b"\r\n"))
    return make("crlf_lookalikes", b"".join(recs))


def skip_table_case():
    """The floor together with the break table of --ambiguous-bases skip: an N with a high quality, one with a low quality, a low
    base beside an N, and lower-case bases."""
    a = bytearray(hit(L, 3100))
    a[50:51], a[100:101] = b"N", b"n"
    b = bytearray(hit(L, 3500).lower())
    b[20:21] = b"N"
    recs = [rec(bytes(a), quals_of(L, [100, 101, 10])), rec(bytes(b), quals_of(L, [19, 70])), rec(hit(L, 3900), quals_of(L, [75]))]
    return make("with_skip_table", _filler(1, 70) + b"".join(recs) + _filler(1, 80), lut=ambiguous_skip_lut())


def malformed_cases():
    """A quality line one byte short, and one byte long: (case, raw offset of that line's '\\n')."""
    out = []
    for name, d in (("qual_one_short", -1), ("qual_one_long", 1)):
        head = _filler(3, 90)
        bad = rec(hit(L, 4100), quals_of(L + d, [5]), b"bad")
        text = head + bad + _filler(2, 95)
        out.append((make(name, text), len(head) + len(bad) - 1))
    return out


def pieces_case():
    """40 KB cut into pieces of PIECE_KB: the record every later piece starts on has its first base low."""
    n = 130
    seqs = [hit(L, 157 * i) for i in range(n)]
    lows = [[(11 * i) % L] for i in range(n)]
    for _ in range(2):                                                # (the layout does not depend on the quality bytes)
        text = b"".join(rec(s, quals_of(L, lo, seed=i), b"p%d" % i) for i, (s, lo) in enumerate(zip(seqs, lows)))
        for r in piece_starts(text):
            lows[r] = [0, 1] + lows[r]
    return make("pieces", text)


def piece_starts(text, piece=PIECE_KB << 10):
    """The records that kmm_map_records' later pieces start on: every piece begins where the last whole record of the one
    before ended."""
    recs, _ = parse_q(text)
    out, at = [], 0
    while True:
        inside = [i for i, r in enumerate(recs) if r.start >= at and r.end <= at + piece]
        if not inside or inside[-1] + 1 >= len(recs):
            return out
        out.append(inside[-1] + 1)
        at = recs[inside[-1]].end


# ------------------------------------------------------------------------------------------------ the keep rule, mates
def _half(i, low):
    """100 bases without a hit in front of 50 genome bases; low: the bases without a hit have low qualities."""
    return rec(miss(100, i) + hit(50, 450 * i), quals_of(L, range(100) if low else [], seed=i), b"half%d" % i)


def _stub(i, low):
    """A genome read; low: all of it but its last 35 bases has low qualities (5 windows are left)."""
    return rec(hit(L, 390 * i + 50), quals_of(L, range(L - 35) if low else [3], seed=i), b"stub%d" % i)


def keep_cases():
    """min_hits 3: genome reads pass, those the floor leaves 5 windows do not.  min_permille 150: a read whose first 100 bases
    hit nothing passes only when the floor takes their windows out of the denominator."""
    by_hits = [_stub(i, i % 3 == 0) for i in range(12)] + [rec(miss(L, 50 + i), quals_of(L, [9]), b"m%d" % i) for i in range(4)]
    by_share = [_half(i, i % 2 == 0) for i in range(10)] + [_stub(20 + i, False) for i in range(4)] + \
               [rec(miss(L, 70 + i), quals_of(L, [9]), b"m%d" % i) for i in range(3)]
    return [make("keep_min_hits", b"".join(by_hits), rule=(3, 0)), make("keep_min_permille", b"".join(by_share), rule=(1, 150))]


def pair_cases():
    """Interleaved mates under min_hits 3: pairs of two genome reads, of one genome read and one without a hit, and of two
    without; the floor takes one mate's hits (every third pair) or both (every fourth)."""
    parts = []
    for p in range(16):
        kind = p % 4
        m1 = _stub(2 * p, p % 3 == 0 or kind == 3)
        m2 = rec(miss(L, 200 + p), quals_of(L, [5]), b"n%d" % p) if kind == 1 else _stub(2 * p + 1, kind == 3)
        parts += [m1, m2] if kind != 2 else [rec(miss(L, 300 + p), quals_of(L, [5]), b"a%d" % p), rec(miss(L, 400 + p), quals_of(L, [7]), b"b%d" % p)]
    text = b"".join(parts)
    return [make("pairs_any", text, rule=(3, 0), pairs="any"), make("pairs_both", text, rule=(3, 0), pairs="both")]


def mate_texts(case):
    """The interleaved case as two buffers: (mate-1 text, mate-2 text)."""
    recs = expected(case).recs
    text = bytes(case.text)
    return (np.frombuffer(b"".join(text[r.start:r.end] for r in recs[0::2]), dtype=np.uint8),
            np.frombuffer(b"".join(text[r.start:r.end] for r in recs[1::2]), dtype=np.uint8))


# ------------------------------------------------------------------------------------------------ BAM and SAM
# seq / qual as stored (qual: raw Phred bytes, None: the record stores none)
BRec = namedtuple("BRec", "name flag seq qual")
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def _phred(n, low, q=20, seed=0):
    return bytes(c - 33 for c in quals_of(n, low, q, seed))


def bam_records():
    """Forward and reverse-strand records with real qualities, records that store none (0xFF) among them, a record without
    bases, and records that a flag filter (0x400) leaves out."""
    recs = []
    for i in range(14):
        seq = hit(L, 420 * i + 30)
        flag = (0x10 if i % 3 == 1 else 0) | (0x400 if i in (5, 9) else 0)
        qual = None if i in (2, 7, 10) else _phred(L, range(20, 100) if i % 2 == 0 else [4, L - 2], seed=i)
        recs.append(BRec(b"b%d" % i, flag, seq, qual))
    recs.insert(4, BRec(b"empty", 0, b"", b""))
    recs.append(BRec(b"short", 0x10, hit(45, 6000), _phred(45, [0, 44], seed=40)))
    return recs


def bam_payload(recs):
    from kmer_mapper_amd import reads_io
    return reads_io.bam_header((), b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(
        reads_io.bam_record(r.seq, r.name, r.flag, qual=r.qual) for r in recs)


def bam_file(recs, block=0xFF00):
    from kmer_mapper_amd import reads_io
    payload = bam_payload(recs)
    hdr = len(reads_io.bam_header((), b"@HD\tVN:1.6\tSO:unsorted\n"))
    return np.frombuffer(reads_io.bgzf_members(payload[:hdr], block) + reads_io.bgzf_members(payload[hdr:], block) + reads_io.BGZF_EOF,
                         dtype=np.uint8)


def bam_reads(recs, exclude=0x400, original_strand=True, absent=b"~"):
    """(names, seqs, quals as Phred+33 text, exempt indices) of the selected records as the decode hands them on: read
    orientation under original_strand, qualities clipped at '~', `absent` for every base of a record that stores none."""
    names, seqs, quals, exempt = [], [], [], []
    for r in recs:
        if r.flag & exclude:
            continue
        none = len(r.seq) > 0 and r.qual is None
        seq, qual = r.seq, (absent * len(r.seq) if none else bytes(min(c + 33, 126) for c in (r.qual or b"")))
        if original_strand and r.flag & 0x10 and seq:
            seq, qual = seq.translate(_COMP)[::-1], qual[::-1]
        if none:
            exempt.append(len(seqs))
        names.append(r.name)
        seqs.append(seq)
        quals.append(qual)
    return names, seqs, quals, exempt


def bam_expected(recs, q, k=K, original_strand=True):
    """(hits, windows, masked, records without qualities, the named FASTQ text per record)"""
    names, seqs, quals, exempt = bam_reads(recs, original_strand=original_strand)
    h, w, masked = model(rc.genome_index(k), k, seqs, quals, q, exempt=exempt)
    named = bam_reads(recs, original_strand=original_strand, absent=b'"')[2]
    texts = [b"@" + n + b"\n" + s + b"\n+\n" + t + b"\n" for n, s, t in zip(names, seqs, named)]
    return h, w, masked, len(exempt), texts


def sam_case():
    """(text, seqs, quals, exempt): SAM records with QUAL, and with QUAL '*' — whose '~' stand-in passes every floor."""
    from kmer_mapper_amd import reads_io
    seqs = [hit(L, 510 * i + 5) for i in range(9)]
    quals = [None if i in (1, 6) else quals_of(L, range(30, 90) if i % 2 == 0 else [7], seed=i) for i in range(9)]
    text = reads_io.sam_text(_Batch(seqs), quals=quals)
    return (np.frombuffer(text, dtype=np.uint8), seqs, [b"~" * L if x is None else x for x in quals],
            [i for i, x in enumerate(quals) if x is None])


class _Batch:
    def __init__(self, seqs):
        self.bases, self.offsets = rc.batch([np.frombuffer(s, dtype=np.uint8) for s in seqs])

    def __len__(self):
        return self.offsets.shape[0] - 1


# ------------------------------------------------------------------------------------------------ the catalogue
_ALL = None


def all_cases():
    """Every well-formed FASTQ case (the malformed ones, BAM and SAM have their own builders)."""
    global _ALL
    if _ALL is None:
        _ALL = (seam_cases() + [super_tile_case()] + position_cases() + value_cases() + [lookalike_crlf_case(), skip_table_case(),
                pieces_case()] + keep_cases() + pair_cases())
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)
