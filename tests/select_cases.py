"""Records for the SAM / BAM record selection (include/kmm.h RECORD SELECTION), shared by the CPU tier
(tests/test_record_select_on_the_cpu.py) and the GPU tier (tests/test_gpu_record_select.py).  Pure Python / numpy, no GPU; nothing
here reads the library's kernels or headers: keep() restates the rule from the specification.

    a record        Rec(flag, ref, pos, mapq, cigar, seq, qual): ref an index into the case's references or -1, pos 0-based or -1,
                    cigar a list of (length, letter) or None, seq as stored, qual Phred+33 text or None
    a selection     Sel(excl, incl, min_mapq, regions, keep_unplaced): regions a list of (ref, beg, end), 0-based half-open, or
                    None: no region list
    keep(r, sel)                    is the record mapped?
    bam_payload / sam_bytes         the same records as inflated BAM bytes / as SAM text
    text(records, sel, ...)         the two-line FASTA / four-line FASTQ the decoders have to write for the kept records
    tables(sel, refs)               the selection as the front ends take it: intervals by refID; names + intervals by name index
    CASES                           name -> builder of a Case(records, refs, sel)
"""
from collections import namedtuple

import numpy as np

Rec = namedtuple("Rec", "flag ref pos mapq cigar seq qual")
Sel = namedtuple("Sel", "excl incl min_mapq regions keep_unplaced")
Case = namedtuple("Case", "records refs sel")
NO_SEL = Sel(0, 0, 0, None, False)
OPS = "MIDNSHP=X"
REF_OPS = "MDN=X"                                  # the operations that consume reference
REFS3 = ((b"chr1", 100_000), (b"chr2", 50_000), (b"HLA:A*01", 20_000))


# ---------------------------------------------------------------------------------------------- the rule, restated
def ref_span(cigar):
    return sum(n for n, op in (cigar or ()) if op in REF_OPS)


def keep(r, sel):
    if r.flag & sel.excl:
        return False
    if r.flag & sel.incl != sel.incl:
        return False
    if r.mapq < sel.min_mapq:
        return False
    if sel.regions is None:
        return True
    if r.ref < 0:
        return bool(sel.keep_unplaced)
    if r.pos < 0:
        return False
    span = ref_span(r.cigar)
    end = r.pos + 1 if (r.flag & 4 or not r.cigar or span == 0) else r.pos + span
    return any(ref == r.ref and beg < end and r.pos < e for ref, beg, e in sel.regions)


def alone(sel):
    """The selection's rules one at a time: [(name, selection with that rule only)]"""
    out = []
    if sel.incl:
        out.append(("include", NO_SEL._replace(incl=sel.incl)))
    if sel.min_mapq:
        out.append(("mapq", NO_SEL._replace(min_mapq=sel.min_mapq)))
    if sel.regions is not None:
        out.append(("regions", NO_SEL._replace(regions=sel.regions, keep_unplaced=sel.keep_unplaced)))
    return out


def tables(sel, refs):
    """(intervals by refID, names, intervals by index into names) — unmerged, as a caller hands them over; the names are the
    distinct names of the regions' references, sorted."""
    regions = sel.regions or []
    names = sorted({bytes(refs[ref][0]) for ref, _, _ in regions})
    return list(regions), names, [(names.index(bytes(refs[ref][0])), beg, end) for ref, beg, end in regions]


# ---------------------------------------------------------------------------------------------- the two writers
def _cigar_words(cigar):
    return tuple(n << 4 | OPS.index(op) for n, op in (cigar or ()))


def bam_payload(records, refs, text=b"@HD\tVN:1.6\n"):
    from kmer_mapper_amd import reads_io
    out = [reads_io.bam_header(refs, text)]
    for i, r in enumerate(records):
        out.append(reads_io.bam_record(r.seq, b"q%d" % i + b"x" * (i % 5), r.flag, ref_id=r.ref, pos=r.pos, cigar=_cigar_words(r.cigar),
                                       qual=None if r.qual is None else bytes(c - 33 for c in r.qual), mapq=r.mapq,
                                       aux=b"NMC\x00" * (i % 3), next_ref_id=r.ref if r.flag & 1 else -1, next_pos=r.pos if r.flag & 1 else -1))
    return b"".join(out)


def sam_line(r, refs, name, crlf=False, tags=b""):
    cigar = b"*" if not r.cigar else b"".join(b"%d%s" % (n, op.encode()) for n, op in r.cigar)
    rname = b"*" if r.ref < 0 else bytes(refs[r.ref][0])
    return (b"%s\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s%s" % (name, r.flag, rname, r.pos + 1, r.mapq, cigar, r.seq or b"*",
                                                             (r.qual if r.seq else None) or b"*", tags)) + (b"\r\n" if crlf else b"\n")


def sam_bytes(records, refs, crlf=False, names=None):
    nl = b"\r\n" if crlf else b"\n"
    out = [b"@HD\tVN:1.6\tSO:unsorted" + nl] + [b"@SQ\tSN:%s\tLN:%d" % (n, ln) + nl for n, ln in refs]
    for i, r in enumerate(records):
        out.append(sam_line(r, refs, names[i] if names else b"q%d" % i + b"x" * (i % 5), crlf, b"\tNM:i:0" if i % 2 else b""))
    return b"".join(out)


def sam_line_starts(data):
    """Byte offset of every line of `data`"""
    starts, p = [], 0
    while p < len(data):
        starts.append(p)
        p = data.index(b"\n", p) + 1
    return starts


def shown(r, orig=False, upper=False):
    """(SEQ, QUAL) as the mapper gets them: as stored, or (orig) a record with FLAG 0x10 flipped back"""
    from tests import strand_cases
    seq = r.seq.upper() if upper else r.seq
    if orig and r.flag & 0x10 and seq:
        return strand_cases.revcomp(seq), None if r.qual is None else r.qual[::-1]
    return seq, r.qual


def text(records, sel, qual=False, orig=False, upper=False):
    out = []
    for r in records:
        if keep(r, sel):
            s, q = shown(r, orig, upper)
            out.append(b"@\n" + s + b"\n+\n" + (b"~" * len(s) if q is None else q) + b"\n" if qual else b">\n" + s + b"\n")
    return b"".join(out)


def counts(records, sel, orig=False):
    """(kept, excluded, kept records flipped by original_strand, kept records with bases and no qualities)"""
    kept = [r for r in records if keep(r, sel)]
    return (len(kept), len(records) - len(kept), sum(1 for r in kept if orig and r.flag & 0x10 and r.seq),
            sum(1 for r in kept if r.qual is None and r.seq))


# ---------------------------------------------------------------------------------------------- the cases
def _seq(rng, n, genome=None):
    if genome is not None and n:
        if n >= len(genome):
            return (bytes(genome) * (n // len(genome) + 1))[:n]
        at = int(rng.integers(0, len(genome) - n))
        return bytes(genome[at:at + n])
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n)))


def _qual(rng, n):
    q = rng.integers(35, 74, size=int(n)).astype(np.uint8)
    q[q == ord("*")] = ord("I")
    return q.tobytes()


def _random_cigar(rng, n):
    """A CIGAR whose query-consuming operations sum to n: clips at the ends, every operation in between"""
    if n == 0:
        return [(int(rng.integers(1, 30)), "D")] if rng.integers(2) else None
    cigar, left = [], n
    if rng.integers(3) == 0:
        cigar.append((int(rng.integers(1, 20)), "H"))
    if left > 2 and rng.integers(3) == 0:
        k = int(rng.integers(1, left // 2 + 1))
        cigar.append((k, "S"))
        left -= k
    tail = []
    if left > 2 and rng.integers(3) == 0:
        k = int(rng.integers(1, left // 2 + 1))
        tail.append((k, "S"))
        left -= k
    if rng.integers(4) == 0:
        tail.append((int(rng.integers(1, 20)), "H"))
    while left > 0:
        op = "M=XI"[int(rng.integers(4))] if cigar and cigar[-1][1] in "M=X" else "M=X"[int(rng.integers(3))]
        k = int(rng.integers(1, left + 1))
        cigar.append((k, op))
        left -= k
        if left > 0 and rng.integers(3) == 0:
            cigar.append((int(rng.integers(1, 400)), "DNP"[int(rng.integers(3))]))
    return cigar + tail


def mixed(seed=11, n=3000, genome=None):
    """~3000 records of 0 to 300 bases on three references plus unplaced ones, every flag / MAPQ / CIGAR shape of the issue."""
    rng = np.random.default_rng(seed)
    flags, mapqs = (0, 4, 16, 0x63, 0x93, 0x100, 0x800, 0x400), (0, 1, 29, 30, 60, 255)
    records = []
    for i in range(n):
        flag = flags[int(rng.integers(len(flags)))]
        ln = int(rng.integers(0, 301)) if i % 50 else 0
        seq = _seq(rng, ln, genome)
        qual = None if i % 11 == 0 else _qual(rng, ln)
        ref = int(rng.integers(-1, 3)) if flag != 4 or i % 3 == 0 else -1
        lim = REFS3[ref][1] if ref >= 0 else 0
        pos = int(rng.integers(0, lim)) if ref >= 0 else -1
        if flag & 4:                                                 # unplaced, or placed-unmapped at its mate's position: no CIGAR
            cigar = None
        else:
            cigar = None if i % 17 == 0 else _random_cigar(rng, ln)
        records.append(Rec(flag, ref, pos, mapqs[int(rng.integers(len(mapqs)))], cigar, seq, qual))
    sel = Sel(0x400, 0x1, 29, [(0, 20_000, 60_000), (0, 55_000, 70_000), (2, 0, 9_000), (2, 9_000, 12_000), (1, 49_000, 50_000)], True)
    return Case(records, REFS3, sel)


def boundaries():
    """One record per side of every region boundary rule."""
    S = lambda n: b"ACGTACGTAC" * (n // 10) + b"ACGTACGTAC"[:n % 10]
    q = lambda n: b"I" * n
    R = lambda ref, pos, cigar, n, flag=0, mapq=60: Rec(flag, ref, pos, mapq, cigar, S(n), q(n))
    records = [
        R(0, 990, [(10, "M")], 10),                       # ends exactly at beg 1000: out
        R(0, 991, [(10, "M")], 10),                       # its last base is 1000: in
        R(0, 1999, [(10, "M")], 10),                      # starts at end - 1: in
        R(0, 2000, [(10, "M")], 10),                      # starts at end: out
        R(0, 900, [(10, "M"), (95, "D"), (10, "M")], 20),  # reaches in through a D: in
        R(0, 900, [(10, "M"), (95, "N"), (10, "M")], 20),  # ... through an N: in
        R(0, 900, [(10, "M"), (95, "I"), (10, "M")], 115),  # I does not extend: out
        R(0, 985, [(10, "M"), (20, "S")], 30),            # reaches in only through S: out
        R(0, 985, [(10, "M"), (20, "H")], 10),            # ... through H: out
        R(0, 985, [(10, "M"), (20, "P"), (5, "M")], 15),  # P does not extend: ends at 1000: out
        R(0, 985, [(10, "="), (5, "X"), (1, "M")], 16),   # = and X extend: [985, 1001): in
        R(0, 1500, None, 10),                             # no CIGAR: one base at pos: in
        R(0, 999, None, 10),                              # ... at 999: out
        R(0, 999, [(10, "M")], 10, flag=4),               # unmapped but placed: one base at 999, the CIGAR is not looked at: out
        R(0, 1000, [(10, "M")], 10, flag=4),              # ... at 1000: in
        R(0, -1, [(2000, "M")], 10),                      # a reference and no position (POS 0): overlaps nothing
        R(0, -1, None, 10),
        R(-1, -1, None, 10, flag=4),                      # unplaced: keep_unplaced
        R(0, 999, [(5, "S"), (10, "I")], 15),             # the sum is 0: one base at 999: out
        R(0, 1000, [(5, "S"), (10, "I")], 15),            # ... at 1000: in
        R(0, 2990, [(10, "M")], 10),                      # [2990, 3000) against [3000, 3100): out
        R(0, 2991, [(10, "M")], 10),                      # in
        R(0, 3150, [(10, "M")], 10),                      # the abutting pair [3000, 3100) + [3100, 3200): in
        R(0, 3200, [(10, "M")], 10),                      # out
        R(1, 1500, [(10, "M")], 10),                      # the same coordinates on another reference: out
        R(1, 95, [(10, "M")], 10),                        # chr2 [100, 200) overlapping [150, 300): in
        R(1, 299, [(10, "M")], 10),                       # in
        R(1, 300, [(10, "M")], 10),                       # out
        R(2, 1500, [(10, "M")], 10),                      # a reference without regions: out
        R(0, 1500, [(10, "M")], 10, mapq=29),             # in the region, below the floor: out
        R(0, 1500, [(10, "M")], 10, mapq=255),            # 255 is a number: in
        R(0, 1500, [(10, "M")], 10, flag=0x10),           # without the include bit: out
        R(0, 1500, [(10, "M")], 10, flag=0x411),          # an excluded bit: out
    ]
    records = [r if r.flag in (0x10, 0x411) or r.flag & 4 else r._replace(flag=r.flag | 1) for r in records]
    # 30 soft-clipped bases in front of every read: S moves neither pos nor the span, and every read is longer than a 31-mer
    clip = lambda c: c if not c else [(c[0][0] + 30, "S")] + c[1:] if c[0][1] == "S" else [(30, "S")] + c
    records = [r._replace(seq=S(len(r.seq) + 30), qual=q(len(r.qual) + 30), cigar=clip(r.cigar)) for r in records]
    sel = Sel(0x400, 0x1, 30, [(0, 3100, 3200), (0, 1000, 2000), (1, 150, 300), (0, 3000, 3100), (1, 100, 200)], True)
    records[17] = records[17]._replace(flag=5)
    records[13] = records[13]._replace(flag=5)
    records[14] = records[14]._replace(flag=5)
    return Case(records, REFS3, sel)


def long_cigars():
    """CIGARs of 63, 64, 65, 128 and 5000 operations whose LAST reference-consuming operation carries the record into the region
    (a step of 64 that drops its tail misses it), each beside a twin that stops one base short; and the long-CIGAR placeholder."""
    records = []
    for n_ops in (1, 2, 63, 64, 65, 127, 128, 129, 5000):
        n_pairs = n_ops // 2
        cigar = [(1, "M"), (1, "I")] * n_pairs + ([(1, "M")] if n_ops % 2 else [])
        n_m = n_pairs + n_ops % 2                                      # reference span; the query is n_ops bases long
        seq = (b"ACGTTGCA" * (n_ops // 8 + 1))[:n_ops]
        for short in (0, 1):                                           # [pos, pos + n_m) reaches 10_000 exactly / stops one short
            records.append(Rec(1, 0, 10_000 - n_m + 1 - short, 60, cigar, seq, b"I" * n_ops))
    seq = b"ACGT" * 50
    records.append(Rec(1, 0, 9_000, 60, [(200, "S"), (1001, "N")], seq, None))     # the placeholder <l_seq>S<n>N: [9000, 10001): in
    records.append(Rec(1, 0, 9_000, 60, [(200, "S"), (1000, "N")], seq, None))     # out
    records.append(Rec(0, 0, 10_000, 60, [(1, "M")], b"A", b"I"))                    # (no include bit: out)
    records.append(Rec(1, 0, 10_000, 0, [(1, "M")], b"A", b"I"))                     # (below the floor: out)
    return Case(records, REFS3, Sel(0, 1, 1, [(0, 10_000, 10_001)], False))


def long_records(seed=12):
    """Records longer than a 16 KiB BAM tile between ordinary ones, the CIGAR array of one straddling a tile edge: the record
    before it is sized so that its CIGAR words lie across inflated byte 3 * 16384."""
    rng = np.random.default_rng(seed)
    records = []
    for i in range(12):
        n = int(rng.integers(20, 200))
        records.append(Rec(1 if i % 3 else 0, i % 3, 4_000 + 10 * i, 60 if i % 4 else 3, [(n, "M")], _seq(rng, n), _qual(rng, n)))
    big = 40_000
    records.insert(4, Rec(1, 0, 4_000, 60, [(big, "M")], _seq(rng, big), _qual(rng, big)))
    records.insert(8, Rec(1, 1, 4_000, 60, [(1, "M"), (1, "D")] * 600 + [(big - 600, "M")], _seq(rng, big), None))
    records.insert(9, Rec(1, 0, 100, 30, [(10, "M"), (3899, "N"), (10, "M"), (big - 20, "S")], _seq(rng, big), _qual(rng, big)))
    return Case(records, REFS3, Sel(0, 1, 30, [(0, 4_000, 4_060), (1, 4_000 + big + 599, 4_000 + big + 600)], False))


def straddling_cigar(edge=5 * 16384):
    """long_records with a filler record in front sized so that the 1200-operation CIGAR array lies across inflated byte `edge`."""
    case = long_records()
    at = 8
    before = len(bam_payload(case.records[:at], case.refs))
    head = 36 + len(b"q%d" % (at + 1) + b"x" * ((at + 1) % 5)) + 1           # the fixed part + read_name of the record with the CIGAR
    want = edge - 2400 - head - before                                       # bytes the filler record has to take
    name = len(b"q%d" % at + b"x" * (at % 5)) + 1
    n = (want - 36 - name - 4 * (at % 3)) * 2 // 3                           # l_seq + (l_seq + 1) / 2 bytes of SEQ and QUAL
    filler = Rec(1, 2, 5, 60, None, b"A" * n, None)
    records = case.records[:at] + [filler] + case.records[at:]
    payload = bam_payload(records[:at + 1], case.refs)
    assert abs(len(payload) + head + 2400 - edge) < 2400, "the CIGAR array does not straddle the tile edge"
    return Case(records, case.refs, case.sel)


NAME_REFS = ((b"chr1", 1000), (b"chr10", 1000), (b"chr", 1000), (b"chr1_alt", 1000), (b"1", 1000), (b"chr11", 1000))


def sam_names():
    """chr1 against chr10, chr, chr1_alt, 1, chr11: compared exactly and whole."""
    records = [Rec(1, i % len(NAME_REFS), 100 + i, 60 if i % 7 else 0, [(40, "M")], b"ACGTACGTAC" * 4, b"I" * 40) for i in range(48)]
    records += [Rec(0, 0, 100, 60, [(40, "M")], b"ACGTACGTAC" * 4, b"I" * 40)]
    return Case(records, NAME_REFS, Sel(0, 1, 1, [(0, 0, 1000)], False))


def sam_extremes():
    """POS 1 and 2^31 - 1, MAPQ 0 and 255."""
    M = (1 << 31) - 2
    seq, qual, cigar = b"ACGTA" * 7, b"I" * 35, [(35, "M")]
    records = [Rec(1, 0, 0, 255, cigar, seq, qual), Rec(1, 0, M, 255, cigar, seq, qual), Rec(1, 0, M, 0, cigar, seq, qual),
               Rec(1, 0, 0, 0, None, seq, None), Rec(1, 0, 7, 255, cigar, seq, qual), Rec(0, 0, 0, 255, cigar, seq, qual),
               Rec(1, 1, M, 255, cigar, seq, qual)]
    return Case(records, ((b"chr1", 1 << 31), (b"chr2", 1 << 31)), Sel(0, 1, 255, [(0, 0, 5), (0, M, M + 1)], False))


def sam_seams(seed=13):
    """SAM lines whose QNAMEs are sized so that TABs 3 to 6 — and with them the digits of POS and MAPQ on either side — fall on
    every place of a 16-byte block and on the six places around the 1 KiB window edge (the window of a line starts at the line's
    start rounded down to 16 bytes; the CPU tier asserts the places on the text itself); one record in six has a CIGAR text
    longer than 1 KiB.  Returns (case, names) for sam_bytes(..., names=names) with LF line ends."""
    rng = np.random.default_rng(seed)
    records, names = [], []
    at = len(sam_bytes([], REFS3))
    targets = [(k, w, 16) for k in range(3, 7) for w in range(16)] + [(k, w, 1024) for k in range(3, 7) for w in (1021, 1022, 1023, 0, 1, 2)]
    for i, (k, w, mod) in enumerate(targets):
        n = int(rng.integers(5, 40))
        if i % 6 == 0:
            cigar = [(1, "M"), (2, "D"), (1, "I")] * 200                        # 600 operations: 1200 bytes of text
            n = 400
        else:
            cigar = [(n, "M")]
        r = Rec((1, 0x63, 0x93, 0)[i % 4], i % 3, 1_000 + 37 * i, (0, 29, 30, 255)[i % 4], cigar, _seq(rng, n), _qual(rng, n))
        line = sam_line(r, REFS3, b"", tags=b"\tNM:i:0" if i % 2 else b"")
        c_k = [j for j, c in enumerate(line) if c == 9][k - 1]                  # TAB k's offset behind the name
        ln = (w - (at % 16 if mod == 1024 else at) - c_k) % mod
        ln += mod if ln < 1 else 0
        records.append(r)
        names.append(b"n" * ln)
        at += len(line) + ln
    return Case(records, REFS3, Sel(0, 1, 30, [(0, 1_500, 3_000), (1, 0, 2_500), (2, 4_000, 7_000)], False)), names


# one malformed line per new error code: (field, its text, error code, the rule that reads it)
MALFORMED = [("mapq", b"", 4, "mapq"), ("mapq", b"6x", 4, "mapq"), ("mapq", b"256", 4, "mapq"), ("mapq", b"-1", 4, "mapq"),
             ("pos", b"", 5, "regions"), ("pos", b"1e3", 5, "regions"), ("pos", b"2147483648", 5, "regions"),
             ("cigar", b"", 6, "regions"), ("cigar", b"10", 6, "regions"), ("cigar", b"M", 6, "regions"), ("cigar", b"5M3Q", 6, "regions"),
             ("cigar", b"5M*", 6, "regions"), ("cigar", b"268435456M", 6, "regions"), ("cigar", b"5MM", 6, "regions")]


def malformed_sam(field, value, n_before=40, genome=None):
    """SAM text with one line whose `field` reads `value` behind n_before good lines: (data, byte offset of the bad line)"""
    rng = np.random.default_rng(14)
    good = [Rec(1, 0, 100 + i, 60, [(60, "M")], _seq(rng, 60, genome), _qual(rng, 60)) for i in range(n_before + 5)]
    lines = [sam_line(r, REFS3, b"g%d" % i) for i, r in enumerate(good)]
    f = lines[n_before].split(b"\t")
    f[{"pos": 3, "mapq": 4, "cigar": 5}[field]] = value
    lines[n_before] = b"\t".join(f)
    head = b"@HD\tVN:1.6\n"
    return head + b"".join(lines), len(head) + sum(len(t) for t in lines[:n_before])


MALFORMED_SEL = {"mapq": NO_SEL._replace(min_mapq=1), "regions": NO_SEL._replace(regions=[(0, 0, 1000)])}

CASES = {"mixed": mixed, "boundaries": boundaries, "long_cigars": long_cigars, "long_records": long_records,
         "straddling_cigar": straddling_cigar, "sam_names": sam_names, "sam_extremes": sam_extremes}


def with_genome(case, genome, seed=15):
    """The case with every SEQ drawn from `genome` (ASCII bytes), lengths, qualities and alignments as they are: reads that hit
    an index built on that genome, so that a record kept or dropped wrongly shows in the node counts."""
    rng = np.random.default_rng(seed)
    return case._replace(records=[r._replace(seq=_seq(rng, len(r.seq), genome)) for r in case.records])


def check_not_vacuous(case):
    """The issue's condition on the catalogue: every rule taken alone removes at least one record and keeps at least one; the
    combined selection keeps between 5 % and 95 %."""
    for name, one in alone(case.sel):
        kept = sum(keep(r, one) for r in case.records)
        assert 0 < kept < len(case.records), (name, kept, len(case.records))
    kept = sum(keep(r, case.sel) for r in case.records)
    assert 0.05 * len(case.records) <= kept <= 0.95 * len(case.records), (kept, len(case.records))
