"""Catalogue of cases for the record-hits mode (include/kmm.h): raw FASTQ / two-line FASTA text whose records'
index hits come back per record.

A case is a small text (a few KB, one just over 1 MiB) with one index, one k and at most one rule.  Expected values never
come from the library: parse(text, fmt) is a plain-Python record parser (split at '\\n', whole records only, the sequence line
without its '\\r'), and its reads go through the numpy model of tests/read_hits_cases.py (model, index_arrays).
tests/test_record_hits_on_the_cpu.py holds that pair to the oracle and to the conditions that keep the catalogue from being
vacuous.

The kernel's seams: a lane takes 4 consecutive bytes of the text, a staged vector 16, a wavefront 256, a tile 1024, and the
newline census counts per super-tile of 1024 tiles (1 MiB).
"""
from collections import namedtuple

import numpy as np

from tests import read_hits_cases as rc
from kmer_mapper_amd.util import ambiguous_skip_lut

LANE, VECTOR, WAVE, TILE, SUPER = 4, 16, 256, 1024, 1024 * 1024
FASTQ, FASTA = "fastq", "fasta"
PERIOD = {FASTQ: 4, FASTA: 2}

RCase = namedtuple("RCase", "name index k fmt text max_freq revcomp lut rule")


# ------------------------------------------------------------------------------------------------ the parser
def parse(text, fmt):
    """(reads, consumed, n_records): the sequence lines of the whole records of `text` (bytes), in order, as bytes; the byte
    behind the last whole record; their number.  A record is PERIOD[fmt] lines, each ended by '\\n'; a '\\r' before it is not
    part of the line."""
    text = bytes(text)
    period = PERIOD[fmt]
    lines, at = [], 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            break
        lines.append((at, nl))
        at = nl + 1
    n_records = len(lines) // period
    reads = []
    for r in range(n_records):
        lo, hi = lines[r * period + 1]
        if hi > lo and text[hi - 1:hi] == b"\r":
            hi -= 1
        reads.append(text[lo:hi])
    consumed = lines[n_records * period - 1][1] + 1 if n_records else 0
    return reads, consumed, n_records


def reads_arrays(reads):
    return rc.batch([np.frombuffer(r, dtype=np.uint8) for r in reads])


def run_model(case, reads=None):
    if reads is None:
        reads = parse(case.text, case.fmt)[0]
    bases, offsets = reads_arrays(reads)
    return rc.model(rc.index_arrays(case.index), bases, offsets, case.k, case.max_freq, case.revcomp, case.lut)


_EXPECT = {}


def expected(case):
    """(hits, windows, consumed, n_records) of the case: parser + model, computed once and shared (read-only)."""
    if case.name not in _EXPECT:
        reads, consumed, n_records = parse(case.text, case.fmt)
        h, w = run_model(case, reads)
        h.setflags(write=False)
        w.setflags(write=False)
        _EXPECT[case.name] = (h, w, consumed, n_records)
    return _EXPECT[case.name]


# ------------------------------------------------------------------------------------------------ writing records
def _qual(n, seed, first=None):
    q = np.random.Generator(np.random.PCG64(seed)).integers(ord("#"), ord("J"), size=n, dtype=np.uint8)
    q[q == ord("@")] = ord("A")                # (only the lookalike case starts a quality line with '@' or '+')
    q[q == ord("+")] = ord("B")
    if first is not None and n:
        q[0] = ord(first)
    return q.tobytes()


def record(fmt, seq, header=b"r", eol=b"\n", qual_first=None, seed=0):
    """One record; header: the bytes behind '@' / '>'."""
    seq = bytes(np.asarray(seq, dtype=np.uint8).tobytes()) if not isinstance(seq, bytes) else seq
    if fmt == FASTA:
        return b">" + header + eol + seq + eol
    return b"@" + header + eol + seq + eol + b"+" + eol + _qual(len(seq), seed, qual_first) + eol


def text_of(fmt, reads, eol=b"\n", headers=None):
    return b"".join(record(fmt, r, (headers[i] if headers else b"r%d" % i), eol, seed=i) for i, r in enumerate(reads))


def make(name, index, k, fmt, text, max_freq=rc.NO_FILTER, revcomp=False, lut=None, rule=None):
    return RCase(name, index, k, fmt, np.frombuffer(bytes(text), dtype=np.uint8).copy(), max_freq, revcomp, lut, rule)


def _read(n, k, at):
    """n bases with hits under genome_index(k): a genome slice, or for the small-k indexes random bases."""
    return (rc.gslice(at % 15_000, n) if k > 5 else rc.random_read(n, 500 + at)).tobytes()


# ------------------------------------------------------------------------------------------------ the cases
SEAM_UNITS = (LANE, VECTOR, WAVE, TILE)


def seam_text(fmt, k, units=SEAM_UNITS):
    """Records whose sequence lines end — the position of the line's '\\n' — one before, at and one behind a multiple of every
    unit (three instances of the seam each); returns (text, [(unit, d, position of that newline)])."""
    out, ends, at, i = [], [], 0, 0
    for unit in units:
        for d in (-1, 0, 1):
            n = k + 2 + 3 * i                                        # bases of this record
            least = at + 2 + n                                       # '@' / '>' and the header's '\n' in front
            e = -(-(least + 1) // unit) * unit + d
            header = b"h" * (e - at - n - 2)
            rec = record(fmt, _read(n, k, 37 * i + 5), header, seed=i)
            assert rec[e - at:e - at + 1] == b"\n" and len(header) >= 0
            out.append(rec)
            ends.append((unit, d, e))
            at += len(rec)
            i += 1
    return b"".join(out), ends


def trio_text(fmt, k, eol=b"\n"):
    return text_of(fmt, [bytes(r.tobytes()) for r in rc.trio(k)], eol)


def seam_cases():
    out = []
    for fmt, k in ((FASTQ, 31), (FASTA, 31), (FASTQ, 16), (FASTA, 2), (FASTQ, 1)):
        text, _ = seam_text(fmt, k)
        out.append(make("seams_%s_k%d" % (fmt, k), rc.genome_index(k), k, fmt, text + trio_text(fmt, k)))
    return out


def super_tile_case():
    """Just over 1 MiB: ordinary FASTQ records up to the super-tile seam, then a sequence line of 200 bases that starts before
    the seam and whose '\\n' lies one behind it (its line number comes from the second super-tile's census), then more records."""
    k, parts, at, i = 31, [], 0, 0
    while at < SUPER - 2000:
        rec = record(FASTQ, _read(150, k, 11 * i), b"f%d" % i, seed=i)
        parts.append(rec)
        at += len(rec)
        i += 1
    n = 200
    header = b"s" * (SUPER + 1 - at - n - 2)
    parts.append(record(FASTQ, _read(n, k, 4000), header, seed=1))
    assert len(b"".join(parts[-1:])) and (at + 1 + len(header) + 1 + n) == SUPER + 1
    tail = text_of(FASTQ, [_read(150, k, 7000 + 13 * j) for j in range(20)] + [bytes(r.tobytes()) for r in rc.trio(k)])
    return make("super_tile_fastq_k31", rc.genome_index(k), k, FASTQ, b"".join(parts) + tail)


def tiny_cases():
    """Records of 3 to 6 bytes ('>\\nA\\n' and its like): many inside one vector, lanes that hold two records, empty sequence
    lines, reads shorter than k."""
    out = []
    for k in (1, 2):
        rng = np.random.Generator(np.random.PCG64(40 + k))
        reads = []
        for i in range(900):
            n = int(rng.integers(0, 4))
            reads.append(rc.ACGT[rng.integers(0, 4, size=n)].tobytes())
        reads[:4] = [b"A", b"C", b"", b"CC"]
        text = b"".join(record(FASTA, r, b"") for r in reads)
        out.append(make("tiny_fasta_k%d" % k, rc.genome_index(k), k, FASTA, text + text_of(FASTA, [_read(k + 60, k, 3)])))
    for fmt, k in ((FASTQ, 16), (FASTA, 31)):
        reads = [_read((0, k - 1, k, 5, 0, 0, k + 1, 1)[i % 8], k, 17 * i) for i in range(160)]
        out.append(make("short_and_empty_%s_k%d" % (fmt, k), rc.genome_index(k), k, fmt, text_of(fmt, reads) + trio_text(fmt, k)))
    return out


def long_header_cases():
    out = []
    for fmt in (FASTQ, FASTA):
        k = 31
        reads = [_read(90, k, 100), _read(200, k, 300), _read(60, k, 900)]
        headers = [b"a", b"x" * 3000, b"b"]                         # tiles 1 and 2 hold no base at all
        out.append(make("long_header_%s_k31" % fmt, rc.genome_index(k), k, fmt, text_of(fmt, reads, headers=headers) + trio_text(fmt, k)))
    return out


def lookalike_case():
    k = 16
    recs = [record(FASTQ, _read(40 + i, k, 50 * i), b"q%d" % i, qual_first=("@", "+")[i % 2], seed=i) for i in range(12)]
    return make("quality_lines_start_with_at_and_plus_k16", rc.genome_index(k), k, FASTQ, b"".join(recs) + trio_text(FASTQ, k))


def crlf_cases():
    out = []
    for fmt, k in ((FASTQ, 31), (FASTA, 16)):
        reads = [_read(n, k, 7 * n) for n in (150, 33, 0, 70, k - 1, 1500)]
        out.append(make("crlf_%s_k%d" % (fmt, k), rc.genome_index(k), k, fmt, text_of(fmt, reads, eol=b"\r\n") + trio_text(fmt, k, b"\r\n")))
    return out


def break_case():
    """The break table of --ambiguous-bases skip: N at a read's start, middle and end, and next to a tile seam."""
    k = 16
    a = bytearray(_read(300, k, 0))
    a[0:1] = b"N"
    b = bytearray(_read(500, k, 400))
    b[250:252] = b"nN"
    c = bytearray(_read(200, k, 1000))
    c[-1:] = b"N"
    head = text_of(FASTQ, [bytes(a), bytes(b), bytes(c), b"N" * (k + 3)])
    # a read across a tile seam: breaks one before and one behind it
    d = bytearray(_read(1500, k, 2000))
    start = len(head) + len(b"@seam\n")
    seam = -(-(start + 100) // TILE) * TILE
    assert seam + 2 + k < start + len(d)
    d[seam - 1 - start:seam - start] = b"N"
    d[seam + 1 - start:seam + 2 - start] = b"N"
    text = head + record(FASTQ, bytes(d), b"seam", seed=9) + trio_text(FASTQ, k)
    return make("breaks_fastq_k16", rc.genome_index(k), k, FASTQ, text, lut=ambiguous_skip_lut(), rule="break")


def _reads_of(case):
    return [case.bases[case.offsets[r]:case.offsets[r + 1]].tobytes() for r in range(case.offsets.shape[0] - 1)]


def rule_cases():
    """The other orientation (a read that hits only there, a palindrome), the frequency filter between two entries of one
    k-mer, a k-mer under several nodes: the reads and indexes of tests/read_hits_cases.py, written as records."""
    out = []
    by_name = {c.name: c for c in rc.revcomp_cases() + rc.filter_cases() + rc.index_cases()}
    for name, fmt in (("revcomp_k16", FASTQ), ("revcomp_k31", FASTA), ("filter_k31", FASTQ), ("several_nodes_k31", FASTA)):
        c = by_name[name]
        reads = _reads_of(c)
        if c.rule == "revcomp":
            # the reverse complement of genome[800 : 808 + k]: its own k-mers are not in the index (that holds reverse complements
            # of the windows below 800 only), those of its other orientation at 800, 804 and 808 are
            codes = rc.genome()[800:808 + c.k]
            reads.append(rc.ACGT[(3 - codes[::-1]).astype(np.uint8)].tobytes())
        out.append(make("%s_%s" % (name, fmt), c.index, c.k, fmt, text_of(fmt, reads), c.max_freq, c.revcomp, c.lut, c.rule))
    return out


def incomplete_cases():
    """A chunk whose last record is incomplete: it is not consumed and gets no entry."""
    k = 31
    reads = [_read(100, k, 10), _read(150, k, 500), _read(80, k, 900)] + [bytes(r.tobytes()) for r in rc.trio(k)]
    whole = text_of(FASTQ, reads)
    cut_quality = whole + record(FASTQ, _read(120, k, 1500), b"cut")[:-30]          # ends inside the quality line
    cut_seq = text_of(FASTA, reads) + b">last\n" + _read(50, k, 1600)              # a sequence line without its newline
    return [make("incomplete_fastq_k31", rc.genome_index(k), k, FASTQ, cut_quality),
            make("incomplete_fasta_k31", rc.genome_index(k), k, FASTA, cut_seq)]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = (seam_cases() + [super_tile_case()] + tiny_cases() + long_header_cases() + [lookalike_case()] + crlf_cases() +
                [break_case()] + rule_cases() + incomplete_cases())
    return _ALL


# ------------------------------------------------------------------------------------------------ what keeps it from being vacuous
def lanes_that_hold_two_records(case):
    """Lanes (4 aligned bytes of the consumed text) whose first byte lies in one record and that hold a base of a LATER record
    with a window starting there: the fold must change records inside the lane."""
    _, consumed, _ = parse(case.text, case.fmt)
    text = case.text[:consumed]
    period = PERIOD[case.fmt]
    line = np.concatenate([[0], np.cumsum(text == 10)[:-1]])
    rec = line // period
    lut = rc.default_lut() if case.lut is None else case.lut
    term = (text == 10) | (text == 13)
    base = ((line % period) == 1) & ~term & (lut[text] != rc.LUT_BREAK)
    run = np.concatenate([np.cumsum(~base), ]).astype(np.int64)      # a window at p: k bases in a row
    ok = np.zeros(text.shape[0], dtype=bool)
    n = text.shape[0] - case.k + 1
    if n > 0:
        ok[:n] = base[:n] & (run[case.k - 1:] == run[:n])
    n_lanes = text.shape[0] // LANE
    first = rec[:n_lanes * LANE:LANE]
    count = 0
    for j in range(1, LANE):
        count += int((ok[j:n_lanes * LANE:LANE] & (rec[j:n_lanes * LANE:LANE] != first)).sum())
    return count
