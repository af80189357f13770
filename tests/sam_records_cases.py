"""Catalogue of cases for SAM lines kept as SAM lines (include/kmm.h "record_sam"), and an independent model.

A case is a SAM text of a few KiB with a selection, a keep rule and the mode (1: header lines kept, 2: dropped).  Expected values
never come from the library.  The model is pure Python: the text is split at '\\n' (only lines that have their newline count),
a line whose first byte is '@' is a header line, every other line is a record of 11 or more TAB-separated fields; the flag masks
and the selection (MAPQ floor, regions by reference name) are restated here from the SAM specification.  The selected records'
SEQs — those with FLAG 0x10 reverse-complemented when the case counts hits in read orientation — form the model's own two-line
FASTA, whose per-record (hits, windows) come from the numpy model of tests/read_hits_cases.py, and the keep rule from
tests/record_keep_cases.py.  The expected bytes are cut out of the input by line start and length.

The kernels' seams: the walk's tiles are 1024 bytes, its windows 1024, the copy's stores 16 bytes; both prefixes are two-level, over
blocks of 1024 spans and of 1024 tiles (block_cases).
"""
from collections import namedtuple

import numpy as np

from tests import read_hits_cases as rc
from tests import record_keep_cases as rk
from tests import strand_cases

K = 31
TILE = 1024
# sel: (include mask, MAPQ floor, [(reference name, beg, end)] 0-based half-open or None, keep_unplaced)
NO_SEL = (0, 0, None, False)
SCase = namedtuple("SCase", "name text k excl sel orig revcomp min_hits min_permille invert mode")
Expected = namedtuple("Expected", "out n_kept keep hits windows consumed n_records n_excluded n_headers fasta")
REF_OPS = b"MDN=X"


def case(name, text, k=K, excl=0, sel=NO_SEL, orig=False, revcomp=False, min_hits=1, min_permille=0, invert=False, mode=1):
    return SCase(name, bytes(text), k, excl, sel, orig, revcomp, min_hits, min_permille, invert, mode)


# ------------------------------------------------------------------------------------------------ the model
def lines_of(text):
    """[(start, length with the newline)] of the lines of `text` that have their newline"""
    out, at = [], 0
    while True:
        nl = text.find(b"\n", at)
        if nl < 0:
            return out
        out.append((at, nl + 1 - at))
        at = nl + 1


def _cigar(field):
    """[(length, operation byte)] of a CIGAR text; [] for "*" """
    if field == b"*":
        return []
    out, n = [], 0
    for c in field:
        if 48 <= c <= 57:
            n = 10 * n + c - 48
        else:
            out.append((n, c))
            n = 0
    return out


def selected(fields, excl, sel):
    """Is the record mapped?  The flag masks, the MAPQ floor, the region list (SAM specification 1.4; `samtools view` semantics:
    a record covers [POS - 1, POS - 1 + the reference bases of its CIGAR), one base when it is unmapped or has none)."""
    incl, min_mapq, regions, keep_unplaced = sel
    flag = int(fields[1])
    if flag & excl or flag & incl != incl or int(fields[4]) < min_mapq:
        return False
    if regions is None:
        return True
    if fields[2] == b"*":
        return bool(keep_unplaced)
    pos = int(fields[3]) - 1
    if pos < 0:
        return False
    span = sum(n for n, op in _cigar(fields[5]) if op in REF_OPS)
    end = pos + 1 if (flag & 4 or span == 0) else pos + span
    return any(name == fields[2] and beg < end and pos < e for name, beg, e in regions)


_EXPECT = {}


def model(c, text=None):
    """Expected of the case (text: another text under the case's rules)."""
    text = c.text if text is None else bytes(text)
    lines = lines_of(text)
    reads, is_record, n_headers, n_excluded = [], [], 0, 0
    for start, length in lines:
        body = text[start:start + length - 1]
        if body.endswith(b"\r"):
            body = body[:-1]
        if body[:1] == b"@":
            n_headers += 1
            is_record.append(None)
            continue
        f = body.split(b"\t")
        assert len(f) >= 11 and f[1].isdigit(), body[:60]
        if not selected(f, c.excl, c.sel):
            n_excluded += 1
            is_record.append(False)
            continue
        seq = b"" if f[9] == b"*" else f[9]
        if c.orig and int(f[1]) & 0x10 and seq:
            seq = strand_cases.revcomp(seq)
        reads.append(seq)
        is_record.append(True)
    bases, offsets = rc.batch([np.frombuffer(r, dtype=np.uint8) for r in reads])
    hits, windows = rc.model(rc.index_arrays(rc.genome_index(c.k)), bases, offsets, c.k, rc.NO_FILTER, c.revcomp, None)
    keep = rk.keep_rule(hits, windows, c.min_hits, c.min_permille, c.invert)
    out, e = [], 0
    for (start, length), kind in zip(lines, is_record):
        if kind is None:
            if c.mode == 1:
                out.append(text[start:start + length])
        elif kind:
            if keep[e]:
                out.append(text[start:start + length])
            e += 1
    consumed = lines[-1][0] + lines[-1][1] if lines else 0
    for a in (hits, windows, keep):
        a.setflags(write=False)
    return Expected(b"".join(out), int(keep.sum()), keep, hits, windows, consumed, len(reads), n_excluded, n_headers,
                    b"".join(b">\n" + r + b"\n" for r in reads))


def expected(c):
    """The case's own text under the model, computed once and shared (read-only)."""
    if c.name not in _EXPECT:
        _EXPECT[c.name] = model(c)
    return _EXPECT[c.name]


# ------------------------------------------------------------------------------------------------ writing lines
HEAD = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100000\n@SQ\tSN:chr2\tLN:50000\n@PG\tID:aln\tPN:aln\tCL:aln -t 4 ref.fa\treads.fq\n"


def hit_read(n, at):
    return rc.gslice(at % 15_000, n).tobytes()


def miss_read(n):
    return b"T" * n                                                   # (no window of it is in genome_index(31))


def line(name, flag, seq, rname=b"chr1", pos=101, mapq=60, cigar=None, tags=b"", eol=b"\n", qual=b"*"):
    cigar = cigar if cigar is not None else (b"%dM" % len(seq) if seq and rname != b"*" else b"*")
    return b"\t".join([name, b"%d" % flag, rname, b"%d" % pos, b"%d" % mapq, cigar, b"*", b"0", b"0", seq or b"*", qual]) + tags + eol


def padded(total, flag, seq, **kw):
    """A record line of exactly `total` bytes: the QNAME takes what the other fields leave."""
    bare = len(line(b"", flag, seq, **kw))
    assert total > bare, (total, bare)
    out = line(b"p" * (total - bare), flag, seq, **kw)
    assert len(out) == total
    return out


def mixed_text(n=60, eol=b"\n", seed=5, lower=False):
    """Header lines in front and between the records; reads that hit, reads that miss, short ones and SEQ '*'; forward and reverse
    strand, secondary and supplementary; odd tags; two references and unplaced records."""
    rng = np.random.default_rng(seed)
    flags = (0, 16, 4, 0x100, 0x800, 0x63, 0x93, 0)
    out = [HEAD.replace(b"\n", eol)]
    for i in range(n):
        flag = flags[i % len(flags)]
        ln = int(rng.integers(35, 220))
        seq = (hit_read(ln, 211 * i), miss_read(ln), hit_read(ln, 97 * i + 13), b"", hit_read(20, i))[i % 5]
        if lower and i % 7 == 0 and not flag & 16:
            seq = seq.lower()
        rname = b"*" if flag == 4 else (b"chr1", b"chr2")[i % 2]
        tags = (b"", b"\tNM:i:0\tMD:Z:%d" % ln, b"\tRG:Z:g\t\tXX:Z:\tco:Z:a b  c", b"\tXB:B:c,1,-2,3")[i % 4]
        out.append(line(b"q%d:%d/1" % (i, i * 7), flag, seq, rname, 1 + 397 * i if rname != b"*" else 0, (0, 10, 30, 60)[i % 4],
                        tags=tags, eol=eol, qual=b"I" * len(seq) if seq and i % 3 else b"*"))
        if i % 11 == 5:
            out.append(b"@CO\ta comment\twith\ttabs between the records" + eol)
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ the cases
def tile_edge_text():
    """A line whose newline is a tile's last byte, then a line that ends one byte short of the next tile's end, so that the line
    behind it STARTS at the last byte of a tile; kept, dropped, kept."""
    parts = [HEAD, line(b"a0", 0, hit_read(120, 50)), line(b"a1", 0, miss_read(90))]
    at = sum(len(p) for p in parts)
    first = 2 * TILE - at                                             # ends at 2048: its newline is byte 2047
    parts.append(padded(first, 0, hit_read(150, 700), tags=b"\tNM:i:1"))
    parts.append(padded(TILE - 1, 0, miss_read(200)))                 # [2048, 3071)
    parts.append(line(b"edge", 16, hit_read(140, 2100), tags=b"\tXS:i:7"))      # starts at byte 3071
    parts.append(line(b"z", 0, miss_read(40)))
    parts.append(line(b"zz", 0, hit_read(60, 3000)))
    text = b"".join(parts)
    starts = [s for s, _ in lines_of(text)]
    assert 2 * TILE in starts and 3 * TILE - 1 in starts and text[2 * TILE - 1:2 * TILE] == b"\n"
    return text


def long_line_text():
    """A kept line longer than three windows and a dropped one longer than two tiles: tiles in which no line starts."""
    text = (HEAD + line(b"s", 0, hit_read(70, 10)) + line(b"long_kept", 0, hit_read(3400, 3000), tags=b"\tMD:Z:3400") +
            line(b"m", 0, miss_read(50)) + line(b"long_dropped", 0, miss_read(2500)) + line(b"e", 16, hit_read(90, 900)) +
            b"@CO\t" + b"c" * 2300 + b"\n" + line(b"last", 0, hit_read(45, 77)))
    lens = sorted(n for _, n in lines_of(text))
    assert lens[-1] > 3 * 1024 + 16 and lens[-2] > 2 * TILE and lens[-3] > 2 * TILE
    return text


def dense_text(n=260):
    """As many lines as fit into a tile: minimal 22-byte records (46 per tile), SEQ 'C' (a hit at k = 1), 'A' (a window, no hit)
    and '*' (no window).  (More than a block of 1024 spans needs 22 KiB: block_cases below.)"""
    recs = [b"q\t4\t*\t0\t0\t*\t*\t0\t0\t" + (b"C", b"A", b"*", b"C")[i % 4] + b"\t*\n" for i in range(n)]
    assert all(len(r) == 22 for r in recs)
    return b"".join(recs[:100]) + b"@CO\tx\n" + b"".join(recs[100:])


def strand_text():
    """Reverse-strand records that hit only in read orientation (the file stores the reverse complement of a genome slice), next
    to forward ones that hit and a reverse one that hits as stored."""
    g = lambda n, at: hit_read(n, at)
    return (HEAD + line(b"f0", 0, g(100, 400)) + line(b"r0", 16, strand_cases.revcomp(g(100, 1200))) + line(b"f1", 0, miss_read(80)) +
            line(b"r1", 0x93, strand_cases.revcomp(g(151, 5000)), tags=b"\tNM:i:2") + line(b"r2", 16, g(90, 7000)) +
            line(b"r3", 16, b""))


def _build():
    mixed = mixed_text()
    regions = (0, 30, [(b"chr1", 2_000, 15_000), (b"chr2", 0, 12_000)], True)
    out = [
        case("tile_edges", tile_edge_text()),
        case("long_lines", long_line_text()),
        case("dense_k1", dense_text(), k=1),
        case("dense_k1_all", dense_text(), k=1, min_hits=0),
        case("dense_k1_inverted_no_header", dense_text(), k=1, invert=True, mode=2),
        case("mixed", mixed),
        case("mixed_no_header", mixed, mode=2),
        case("mixed_all_kept", mixed, min_hits=0),                  # (SEQ '*' has no window: kept at min_hits 0 alone)
        case("mixed_none_kept", mixed, min_hits=100_000),
        case("mixed_inverted", mixed, invert=True),
        case("mixed_permille", mixed, min_hits=2, min_permille=250),
        case("mixed_excluded_between", mixed, excl=0x904),          # (entry ordinals skip the excluded records)
        case("mixed_selection", mixed, excl=0x800, sel=regions),
        case("mixed_selection_no_header", mixed, excl=0x800, sel=regions, orig=True, mode=2),
        case("read_orientation", strand_text(), orig=True),
        case("as_stored", strand_text(), orig=False),
        case("as_stored_both_orientations", strand_text(), revcomp=True),
        case("crlf", mixed_text(40, b"\r\n", seed=6, lower=True)),
        case("header_only", HEAD + b"@CO\tnothing else\n"),
        case("header_only_no_header", HEAD, mode=2),
        case("no_complete_line", b"q\t0\tchr1\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\t*"),
        case("unterminated_last_line", mixed_text(12, seed=7) + line(b"tail", 0, hit_read(80, 123))[:-1]),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


# ---- the second level of both prefixes: more than 1024 spans (the flags' blocks) and more than 1024 tiles (the tiles' blocks)
BLOCK = 1024


def dense_blocks_text(n=2700):
    """Minimal records, kept and dropped in turn, a header line every 500: more than two blocks of spans, header lines in three."""
    recs = [b"q\t4\t*\t0\t0\t*\t*\t0\t0\t" + (b"C", b"A", b"*", b"C", b"A")[i % 5] + b"\t*\n" for i in range(n)]
    parts = []
    for i in range(0, n, 500):
        parts += [b"@CO\tbefore record %d\n" % i] + recs[i:i + 500]
    return b"".join(parts)


def big_text(size=1_400_000, seed=9):
    """More than 1024 tiles: records that hit and miss, secondary and reverse-strand ones, a header line every 150 records, on
    both sides of tile 1024 — both columns of the second block's base are non-zero, and its tiles' spans lie in the fourth block
    of spans and behind."""
    rng = np.random.default_rng(seed)
    parts, at, i = [HEAD], len(HEAD), 0
    while at < size:
        ln = int(rng.integers(120, 260))
        seq = (hit_read(ln, 53 * i), miss_read(ln), hit_read(ln, 29 * i + 7))[i % 3]
        rec = line(b"b%d" % i, (0, 16, 0x100, 0, 0x800, 4)[i % 6], seq, (b"chr1", b"chr2")[i % 2], 1 + 17 * i, 60,
                   tags=b"\tNM:i:%d" % (i % 7) if i % 2 else b"")
        if i % 150 == 75:
            rec += b"@CO\tbehind record %d\n" % i
        parts.append(rec)
        at += len(rec)
        i += 1
    return b"".join(parts)


_BLOCKS = None


def block_cases():
    """The cases whose spans and tiles fill more than one block of 1024; what makes them so is asserted here."""
    global _BLOCKS
    if _BLOCKS is None:
        dense, big = dense_blocks_text(), big_text()
        _BLOCKS = [case("blocks_dense_k1", dense, k=1), case("blocks_dense_k1_inverted_no_header", dense, k=1, invert=True, mode=2),
                   case("blocks_big", big), case("blocks_big_excluded_no_header", big, excl=0x900, mode=2)]
        starts = [s for s, _ in lines_of(dense)]
        assert len(starts) > 2 * BLOCK and sum(1 for s in starts[2 * BLOCK:] if dense[s:s + 1] == b"@") >= 1
        edge = BLOCK * TILE                                           # the first byte of tile 1024
        assert len(big) > edge + 100 * TILE
        for c in _BLOCKS[2:]:
            e = expected(c)
            kinds = [(s, big[s:s + 1] == b"@") for s, _ in lines_of(big)]
            for side in (lambda s: s < edge, lambda s: s >= edge):
                assert sum(1 for s, h in kinds if side(s) and h) >= 3 and sum(1 for s, h in kinds if side(s) and not h) > BLOCK
            assert e.n_records > 3 * BLOCK and 0.2 * e.n_records < e.n_kept < 0.8 * e.n_records
        assert expected(_BLOCKS[3]).n_excluded > BLOCK
    return _BLOCKS


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = _build()
    return _ALL


def by_name(name):
    return next(c for c in all_cases() + (_BLOCKS or []) if c.name == name)


def with_final_newline(text):
    """What the stream routes map under KMM_FORMAT_LAST_CHUNK: a final line without its newline gets one."""
    return text if not text or text.endswith(b"\n") else text + b"\n"


def malformed_behind(text, n_good=30):
    """`text`, then n_good good records, a line of five fields, and two more good ones: (bytes, offset of the malformed line)"""
    good = b"".join(line(b"g%d" % i, 0, hit_read(150, 31 * i)) for i in range(n_good))
    bad = b"bad\t0\tchr1\t5\t60\n"
    return text + good + bad + line(b"h", 0, hit_read(50, 5)) + line(b"i", 0, miss_read(50)), len(text) + len(good)
