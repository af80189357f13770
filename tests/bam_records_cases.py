"""Catalogue of cases for the raw form of the BAM keep (include/kmm.h "record_bam"): BAM files whose selected records
come back AS BAM RECORDS — the block_size word and the block_size bytes behind it, untouched — when their entry passes a keep rule.

Nothing here reads the library.  The model is
    bam_fastq_cases.inflate + read_bam   that module's own BAM reader (zlib over the BGZF members, struct over the records);
                                         BRec.start and BRec.size locate a record's raw bytes
    bam_fastq_cases.selected             which records are selected (select_cases.keep: the selection's rule from the specification)
    fasta_of                             the two-line FASTA of a selected record, SEQ flipped where `orig` is set and FLAG has 0x10
    record_keep_cases                    hits and windows per read of that text (its parser and numpy hit model), the keep rule
so a case's expected queue bytes are b"".join(payload[r.start:r.start + r.size]) over the selected records that pass the rule, its
entries one (hits, windows) per selected record, and its expected file, once inflated, payload[:hdr] followed by those bytes.
tests/test_bam_records_on_the_cpu.py holds the catalogue to the conditions that keep it from being vacuous.

The copy's seams: one wavefront per 16 KiB tile of the inflated stream walks the records that start in it; 64 lanes over a kept
record's bytes, the destination-aligned middle as 16-byte lines, its ragged head and tail byte by byte — so the residues of the
source and of the destination offset modulo 16, records across a tile boundary, and tiles without a record start.
"""
from collections import namedtuple

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests import record_keep_cases as rk
from tests import select_cases as sc
from tests.bam_fastq_cases import inflate, read_bam, selected, hit, miss, _rec, _payload      # noqa: F401 (inflate: the tests' reader)
from tests import bam_fastq_cases as bc

K = 31
TILE = 16384
_COMP = bytes.maketrans(b"=ACMGRSVTWYHKDBN", b"=TGKCYSBAWRDMHVN")

# payload: the inflated stream (header + records); sel: select_cases.Sel; orig: "original_strand" for the hits; k: the index is
# read_hits_cases.genome_index(k)
RBase = namedtuple("RBase", "name payload sel orig k")
RCase = namedtuple("RCase", "name base min_hits min_permille invert")


# ------------------------------------------------------------------------------------------------ the model
def fasta_of(r, orig):
    seq = r.seq
    if orig and r.flag & 0x10 and seq:
        seq = seq.translate(_COMP)[::-1]
    return b">\n" + seq + b"\n"


Decoded = namedtuple("Decoded", "records all_records text excluded hdr")
_DECODED = {}


def decoded(base):
    """The selected records of `base`, all its records, the two-line FASTA the hits are counted on, the header's length."""
    if base.name not in _DECODED:
        _, recs, hdr = read_bam(base.payload)
        keep = [r for r in recs if selected(r, base.sel)]
        _DECODED[base.name] = Decoded(keep, recs, b"".join(fasta_of(r, base.orig) for r in keep), len(recs) - len(keep), hdr)
    return _DECODED[base.name]


def keep_case(case):
    base = case.base
    text = decoded(base).text
    return rk.KCase("bam_records_" + case.name, rh.make("bam_records_" + base.name, rc.genome_index(base.k), base.k, rh.FASTA, text),
                    case.min_hits, case.min_permille, case.invert)


_EXPECT = {}


def expected(case):
    """(queue bytes, n_kept, keep mask, hits, windows): the kept records' raw bytes and the entries, one per selected record."""
    if case.name not in _EXPECT:
        _, n_kept, keep, hits, windows, consumed, n_records = rk.expected(keep_case(case))
        d = decoded(case.base)
        assert consumed == len(d.text) and n_records == len(d.records)
        p = case.base.payload
        raw = b"".join(p[r.start:r.start + r.size] for r, kp in zip(d.records, keep) if kp)
        _EXPECT[case.name] = (raw, n_kept, keep, hits, windows)
    return _EXPECT[case.name]


def expected_file(case):
    """What the output file inflates to: the input's header, verbatim, and the kept records."""
    return case.base.payload[:decoded(case.base).hdr] + expected(case)[0]


def bam_file(base, block=0xFF00, level=6):
    return bc.bam_file(base, block, level)


# ------------------------------------------------------------------------------------------------ the bases
MIN_SIZE = 37                                                         # 4 + 32 + l_read_name 1 (the NUL alone), no bases
SIZES = tuple(range(MIN_SIZE, 101))


def _sized(size, keep, salt):
    """A record of exactly `size` bytes with an empty name; under genome_index(1) (the 1-mer C) it has a hit iff `keep` — which
    takes a base: sizes 37 and 38 hold none and never have one.  What is left after one base is aux, with 0x00 and 0xFF in it."""
    if size < 39:
        rec = _rec(b"", b"", qual=b"", aux=bytes([0xFF, 0x00][:size - MIN_SIZE]))
    else:
        aux = bytes((0x00, 0xFF, 0x41 + (salt + j) % 26)[j % 3] for j in range(size - 39))
        rec = _rec(b"C" if keep else b"AGT"[salt % 3:salt % 3 + 1], b"", qual=bytes([salt % 60]), aux=aux)
    assert len(rec) == size, (len(rec), size)
    return rec


def sizes_base():
    """Sizes 37 to 100 consecutively, a kept and a dropped record of each — ascending, then descending with the two swapped: every
    size has kept and dropped neighbours.  Behind them the residue walk: sixteen rounds of one dropped record of 49 bytes (1
    modulo 16: the source moves on by one against the destination) and sixteen kept ones of 49, 65, 81 and 97 bytes (1 modulo 16
    each: source and destination move on by one together) — the kept records' source and destination offsets take all 16 x 16
    residues modulo 16."""
    recs, salt = [], 0
    for order, swap in ((SIZES, False), (SIZES[::-1], True)):
        for s in order:
            pair = [_sized(s, True, salt), _sized(s, False, salt + 1)]
            salt += 2
            recs += pair[::-1] if swap else pair
    for _ in range(16):
        recs.append(_sized(49, False, salt))
        for j in range(16):
            recs.append(_sized((49, 65, 81, 97)[j % 4], True, salt + j))
        salt += 17
    return RBase("sizes", _payload(recs), sc.NO_SEL, False, 1)


AUX_SIZES = (1, 15, 16, 17, 300)


def aux_base():
    """CIGARs and aux blocks of 1, 15, 16, 17 and 300 bytes with 0x00 and 0xFF inside, each on a record with hits and on one
    without; some stored reverse-complemented (the hits are counted in read orientation, the bytes are never altered)."""
    recs = []
    for i, n in enumerate(AUX_SIZES):
        aux = bytes((0x00, 0xFF, 0x30 + j % 64)[(i + j) % 3] for j in range(n))
        for j, seq in enumerate(bc._both(64 + i, 70 + i)):
            flag = 0x10 if (i + j) % 2 else 0
            cigar = tuple(((10 + c) << 4) | (0, 1, 2, 4)[c % 4] for c in range(i + 1))
            recs.append(_rec(bc.revcomp(seq) if flag else seq, b"aux%d_%d" % (n, j), flag, aux=aux, cigar=cigar, ref_id=0, pos=100 * i,
                             mapq=30 + i, next_ref_id=0, next_pos=7, tlen=-3))
    return RBase("aux", _payload(recs, sc.REFS3), sc.NO_SEL, True, K)


def straddle_base():
    """Records whose block_size word lies across a 16 KiB boundary of the inflated stream (they start 1, 2 and 3 bytes in front of
    it), whose fixed head does (10 bytes in front), and whose aux does; each once with hits and once without.  A filler record in
    front of each puts it there.  Returns the base and [(kind, start, size)]."""
    from kmer_mapper_amd import reads_io
    parts = [reads_io.bam_header((), b"@HD\tVN:1.6\n")]
    at, m = len(parts[0]), 1
    bare = len(_rec(miss(40, 900), b"fill"))
    across = []
    for kind in ("word1", "word2", "word3", "head", "aux"):
        for j in range(2):
            seq = bc._both(90, 20 + m)[j]
            name = b"%s_%d" % (kind.encode(), j)
            rec = _rec(seq, name, aux=bytes((0xFF, 0x00, 0x55)[c % 3] for c in range(200)))
            inside = {"word1": 1, "word2": 2, "word3": 3, "head": 10, "aux": len(rec) - 100}[kind]
            start = m * TILE - inside
            assert start - at >= bare
            parts.append(_rec(miss(40, 900 + m), b"fill", aux=b"Z" * (start - at - bare)))
            parts.append(rec)
            across.append((kind, start, len(rec)))
            at = start + len(rec)
            m += 1
    return RBase("straddle", b"".join(parts), sc.NO_SEL, False, K), across


LONG = (39_769, 39_770)                                               # bases: 4 + block_size is over three and a half tiles


def long_base():
    """Reads that pass through whole tiles in which no record starts, odd and even, each once kept and once dropped, with a kept
    record right behind: its destination comes from the long record's bytes (or from their absence)."""
    recs = [_rec(hit(50, 1), b"first")]
    for i, n in enumerate(LONG):
        for j, seq in enumerate(bc._both(n, 9 + i)):
            recs.append(_rec(seq, b"long%d_%d" % (n, j), flag=0))
            recs.append(_rec(hit(45 + i + j, 800 + 100 * i + 10 * j), b"behind%d_%d" % (n, j)))
    return RBase("long", _payload(recs), sc.NO_SEL, False, K)


def selection_base():
    """bam_fastq_cases' selection: one rule after the other drops a record that lies between two selected ones (exclude, include,
    MAPQ, a region reached through the CIGAR only), so the entry ordinals skip the unselected records."""
    b = bc.selection_base()
    return RBase("selection", b.payload, b.sel, False, K)


def tiles_base():
    """A tile with exactly one record, a tile with none selected (its records carry 0x400, which is excluded), a tile with all
    kept, and a last tile with a kept and a dropped one.  Returns the base and the four tile numbers."""
    from kmer_mapper_amd import reads_io
    parts = [reads_io.bam_header((), b"@HD\tVN:1.6\n")]
    at = len(parts[0])

    def fill_to(end, make):
        """Records made by make(i) from `at` on, the last one padded with aux so that it ends exactly at `end`."""
        nonlocal at
        i = 0
        while True:
            rec = make(i, b"")
            if end - at - len(rec) < 2 * len(rec):                                # (the last one takes the rest)
                rec = make(i, b"P" * (end - at - len(rec)))
                parts.append(rec)
                at += len(rec)
                assert at == end
                return
            parts.append(rec)
            at += len(rec)
            i += 1

    fill_to(TILE, lambda i, aux: _rec(bc._both(70, i)[i % 2], b"t0_%d" % i, aux=aux))
    fill_to(2 * TILE, lambda i, aux: _rec(hit(200, 33), b"alone", aux=b"Q" * (TILE - len(_rec(hit(200, 33), b"alone")))))
    fill_to(3 * TILE, lambda i, aux: _rec(hit(80, 5 * i), b"t2_%d" % i, 0x404, aux=aux))
    fill_to(4 * TILE, lambda i, aux: _rec(hit(90, 7 * i), b"t3_%d" % i, aux=aux))
    parts += [_rec(miss(60, 3), b"t4_miss"), _rec(hit(60, 3), b"t4_hit")]
    return RBase("tiles", b"".join(parts), sc.NO_SEL._replace(excl=0x400), False, K), (1, 2, 3, 4)


def big_base():
    """4 500 reads of 150 bases with 64 bytes of aux each, three in four with hits: the kept bytes exceed 1 MiB."""
    recs = []
    for i in range(4500):
        seq = miss(150, 100 + i) if i % 4 == 1 else hit(150, 37 * i)
        flag = 0x10 if i % 5 == 0 else 0
        aux = b"RGZgrp%04d\0" % (i % 7) + bytes((i + j) % 256 for j in range(53))
        recs.append(_rec(bc.revcomp(seq) if flag else seq, b"read%d" % i, flag, qual=bc.ramp(150, first=i % 40), aux=aux))
    return RBase("big", _payload(recs), sc.NO_SEL, True, K)


_BASES = None


def bases():
    global _BASES
    if _BASES is None:
        sel = selection_base()
        out = [sizes_base(), aux_base(), straddle_base()[0], long_base(), sel,
               sel._replace(name="selection_flags_only", sel=sc.NO_SEL._replace(excl=0x400)), tiles_base()[0], big_base()]
        _BASES = {b.name: b for b in out}
    return _BASES


_ALL = None


def all_cases():
    """Every base under min_hits 1; min_hits 0, one above the largest count and invert on four of them; 200 per mille."""
    global _ALL
    if _ALL is None:
        out = [RCase(name + "__default", b, 1, 0, False) for name, b in bases().items()]
        for name in ("sizes", "aux", "long", "selection"):
            b = bases()[name]
            top = int(expected(RCase(name + "__default", b, 1, 0, False))[3].max())
            out.append(RCase(name + "__min_hits_0", b, 0, 0, False))
            out.append(RCase(name + "__above_the_largest", b, top + 1, 0, False))
            out.append(RCase(name + "__invert", b, 1, 0, True))
        out.append(RCase("straddle__permille_200", bases()["straddle"], 1, 200, False))
        out.append(RCase("tiles__invert", bases()["tiles"], 1, 0, True))
        out.append(RCase("big__invert", bases()["big"], 1, 0, True))
        _ALL = out
    return _ALL


def identity_case(name="aux"):
    """No selection and min_hits 0: every record is kept."""
    b = bases()[name]
    return RCase(name + "__identity", b._replace(name=name + "_identity", sel=sc.NO_SEL), 0, 0, False)


# ------------------------------------------------------------------------------------------------ what keeps it from being vacuous
FEATURES = ("aux of 1", "aux of 15", "aux of 16", "aux of 17", "aux of 300", "0x00 and 0xFF in aux", "cigar",
            "block_size word across a tile boundary", "head across a tile boundary", "aux across a tile boundary",
            "through whole tiles", "behind an unselected record", "stored reversed")
# features a record has by being kept: the record right behind a long one is a kept one by construction, so is the one alone in
# its tile.  (And a record of 37 or 38 bytes has no base and so no hit: under min_hits 1 it is always dropped; min_hits 0 and
# invert keep it — tests/test_bam_records_on_the_cpu.py asserts both.)
FEATURES_KEPT = ("behind a long record", "alone in its tile")


def features(base):
    """Per selected record of `base`, the set of the features it has."""
    d = decoded(base)
    out = []
    prev_by_start = {}
    prev = None
    for r in d.all_records:
        prev_by_start[r.start] = prev
        prev = r
    chosen = {r.start for r in d.records}
    starts = sorted(r.start for r in d.all_records)
    for r in d.records:
        f = set()
        fixed = 36 + len(r.name) + 1 + 4 * len(r.cigar) + (len(r.seq) + 1) // 2 + len(r.seq)
        n_aux = r.size - fixed
        aux = base.payload[r.start + fixed:r.start + r.size]
        if n_aux in AUX_SIZES:
            f.add("aux of %d" % n_aux)
        if 0x00 in aux and 0xFF in aux:
            f.add("0x00 and 0xFF in aux")
        if r.cigar:
            f.add("cigar")
        first, last = r.start // TILE, (r.start + r.size - 1) // TILE
        if (r.start + 3) // TILE != first:
            f.add("block_size word across a tile boundary")
        elif (r.start + 35) // TILE != first:
            f.add("head across a tile boundary")
        if n_aux and (r.start + fixed) // TILE != last:
            f.add("aux across a tile boundary")
        if last - first >= 3:
            f.add("through whole tiles")
        before = prev_by_start[r.start]
        if before is not None and before.size > 3 * TILE:
            f.add("behind a long record")
        if before is not None and before.start not in chosen:
            f.add("behind an unselected record")
        if sum(1 for s in starts if s // TILE == first) == 1:
            f.add("alone in its tile")
        if base.orig and r.flag & 0x10 and r.seq:
            f.add("stored reversed")
        out.append(f)
    return out


def residues(case):
    """{(source offset % 16, destination offset % 16)} of the case's kept records (the queue's tail at 0)."""
    out, dst = set(), 0
    for r, kp in zip(decoded(case.base).records, expected(case)[2]):
        if kp:
            out.add((r.start % 16, dst % 16))
            dst += r.size
    return out
