"""Catalogue of cases for the named FASTQ form of the BAM decode (include/kmm.h "record_names"): BAM files whose
selected records come back as four-line FASTQ with their names and qualities, and of those the ones a keep rule keeps.

Nothing here reads the library's decode.  The model is
    inflate + read_bam      this module's own BAM reader: zlib over the BGZF members, struct over the records
    select_cases.keep       which records are selected (the selection's rule, restated there from the specification)
    fastq_of                the text rules of the named form, restated from the issue: '@' NAME [/1 | /2] '\\n' SEQ '\\n' "+\\n" QUAL '\\n'
    record_keep_cases       hits and windows per read of that text (its parser and numpy hit model), the keep rule, the kept bytes
so a case's expected queue bytes are b"".join of the kept records' model text, and its entries one (hits, windows) per selected
record.  tests/test_bam_fastq_on_the_cpu.py holds the catalogue to the conditions that keep it from being vacuous.

The decode's seams: 64 lanes over a record's name bytes and then over its SEQ bytes (two bases each), one wavefront per 16 KiB
tile of the inflated stream, records that start in one tile and end in a later one; behind it the compaction's (1024-byte tiles,
1 MiB super-tiles of the decoded text).
"""
import struct
import zlib
from collections import namedtuple

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests import record_keep_cases as rk
from tests import select_cases as sc

K = 31
TILE = 16384
_NIB = b"=ACMGRSVTWYHKDBN"
_COMP = bytes.maketrans(_NIB, b"=TGKCYSBAWRDMHVN")

# name: the l_read_name - 1 bytes in front of the NUL, as stored; cigar: [(length, letter)]; seq: letters; qual: the raw bytes;
# start / size: where the record lies in the inflated stream (block_size included)
BRec = namedtuple("BRec", "name flag ref pos mapq cigar seq qual start size")
# payload: the inflated stream (header + records); sel: select_cases.Sel; cpu_only: letters the default lookup table refuses
Base = namedtuple("Base", "name payload sel orig suffix cpu_only")
BCase = namedtuple("BCase", "name base min_hits min_permille invert")


# ------------------------------------------------------------------------------------------------ the reader
def inflate(comp):
    """The inflated bytes of a BGZF file: member by member, CRC32 and ISIZE checked."""
    comp, out, p = bytes(comp), [], 0
    while p < len(comp):
        if comp[p:p + 4] != b"\x1f\x8b\x08\x04" or comp[p + 12:p + 14] != b"BC":
            raise ValueError("no BGZF member at byte %d" % p)
        size = struct.unpack_from("<H", comp, p + 16)[0] + 1
        raw = zlib.decompress(comp[p + 18:p + size - 8], -15)
        crc, isize = struct.unpack_from("<II", comp, p + size - 8)
        if zlib.crc32(raw) & 0xFFFFFFFF != crc or len(raw) != isize:
            raise ValueError("corrupt BGZF member at byte %d" % p)
        out.append(raw)
        p += size
    return b"".join(out)


def read_bam(raw):
    """(references [(name, length)], records [BRec], header length) of inflated BAM bytes (SAM/BAM specification 4.2)."""
    raw = bytes(raw)
    if raw[:4] != b"BAM\1":
        raise ValueError("magic")
    p = 8 + struct.unpack_from("<i", raw, 4)[0]
    (n_ref,) = struct.unpack_from("<i", raw, p)
    p += 4
    refs = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from("<i", raw, p)
        refs.append((raw[p + 4:p + 4 + ln - 1], struct.unpack_from("<i", raw, p + 4 + ln)[0]))
        p += 8 + ln
    hdr, recs = p, []
    while p < len(raw):
        (bs,) = struct.unpack_from("<i", raw, p)
        if bs < 32 or p + 4 + bs > len(raw):
            raise ValueError("truncated record at %d" % p)
        ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq, _nref, _npos, _tlen = struct.unpack_from("<iiBBHHHiiii", raw, p + 4)
        q = p + 36
        name = raw[q:q + l_name]
        if not name or name[-1] != 0:
            raise ValueError("read_name at %d" % p)
        q += l_name
        cigar = [(w >> 4, sc.OPS[w & 15]) for w in struct.unpack_from("<%dI" % n_cig, raw, q)]
        q += 4 * n_cig
        packed = raw[q:q + (l_seq + 1) // 2]
        q += (l_seq + 1) // 2
        if q + l_seq > p + 4 + bs:
            raise ValueError("block_size at %d" % p)
        seq = bytes(_NIB[(packed[j // 2] >> (4 if j % 2 == 0 else 0)) & 15] for j in range(l_seq))
        recs.append(BRec(name[:-1], flag, ref, pos, mapq, cigar, seq, raw[q:q + l_seq], p, 4 + bs))
        p += 4 + bs
    return refs, recs, hdr


# ------------------------------------------------------------------------------------------------ the text rules
def selected(r, sel):
    return sc.keep(sc.Rec(r.flag, r.ref, r.pos, r.mapq, r.cigar, r.seq, r.qual), sel)


def mate_suffix(flag, on):
    if on and flag & 0x40 and not flag & 0x80:
        return b"/1"
    if on and flag & 0x80 and not flag & 0x40:
        return b"/2"
    return b""


def fastq_of(r, orig=False, suffix=False):
    """(text, replaced name bytes, reversed, qualities absent) of one selected record."""
    name = bytes(c if 0x21 <= c <= 0x7E else 0x3F for c in r.name)
    replaced = sum(1 for c in r.name if not 0x21 <= c <= 0x7E)
    absent = len(r.seq) > 0 and r.qual[0] == 0xFF
    qual = b'"' * len(r.seq) if absent else bytes(min(q + 33, 126) for q in r.qual)
    seq = r.seq
    rev = bool(orig and r.flag & 0x10 and len(seq) > 0)
    if rev:
        seq, qual = seq.translate(_COMP)[::-1], qual[::-1]
    return b"@" + name + mate_suffix(r.flag, suffix) + b"\n" + seq + b"\n+\n" + qual + b"\n", replaced, rev, absent


Decoded = namedtuple("Decoded", "text records texts replaced reversed no_qual excluded")
_DECODED = {}


def decoded(base):
    """What the decode has to write for `base`: the text of all its selected records, those records, and the counters."""
    if base.name not in _DECODED:
        _, recs, _ = read_bam(base.payload)
        keep = [r for r in recs if selected(r, base.sel)]
        parts = [fastq_of(r, base.orig, base.suffix) for r in keep]
        for r, (t, _, _, _) in zip(keep, parts):                                  # the length the issue states, from the head alone
            assert len(t) == len(r.name) + len(mate_suffix(r.flag, base.suffix)) + 2 * len(r.seq) + 6
        _DECODED[base.name] = Decoded(b"".join(p[0] for p in parts), keep, [p[0] for p in parts], sum(p[1] for p in parts),
                                      sum(p[2] for p in parts), sum(p[3] for p in parts), len(recs) - len(keep))
    return _DECODED[base.name]


def keep_case(case):
    """The case as tests/record_keep_cases.py takes it: the decoded text as a FASTQ chunk under genome_index(K)."""
    base = case.base
    text = decoded(base).text
    return rk.KCase("bam_fastq_" + case.name, rh.make("bam_fastq_" + base.name, rc.genome_index(K), K, rh.FASTQ, text), case.min_hits,
                    case.min_permille, case.invert)


def expected(case):
    """(kept text, n_kept, keep mask, hits, windows) — the queue bytes and the entries, one per selected record."""
    text, n_kept, keep, hits, windows, consumed, n_records = rk.expected(keep_case(case))
    d = decoded(case.base)
    assert consumed == len(d.text) and n_records == len(d.records)
    return text, n_kept, keep, hits, windows


def bam_file(base, block=0xFF00, level=6):
    """The case as a BAM file: the header in members of its own, as htslib writes it, the records behind, the EOF member."""
    from kmer_mapper_amd import reads_io
    _, _, hdr = read_bam(base.payload)
    return (reads_io.bgzf_members(base.payload[:hdr], block, level) + reads_io.bgzf_members(base.payload[hdr:], block, level) +
            reads_io.BGZF_EOF)


# ------------------------------------------------------------------------------------------------ reads
def hit(n, at):
    """n bases with hits under genome_index(K): genome slices (one is at most 15 000 bases)."""
    out, i = [], 0
    while n > 0:
        m = min(n, 4000)
        out.append(rc.gslice((at + 4100 * i) % 15_000, m).tobytes())
        n -= m
        i += 1
    return b"".join(out)


def miss(n, seed):
    return rc.random_read(n, 7000 + seed).tobytes()                   # (no 31-mer of 20 kb of genome in random bases)


def revcomp(seq):
    return seq.translate(_COMP)[::-1]


def ramp(n, first=3, step=7, top=60):
    """Raw qualities that differ from base to base (a reversed or shifted line is seen), never 0xFF."""
    return bytes((first + step * j) % top for j in range(n))


def name_of(n, tag=0):
    """A name of n printable bytes that differ from one position to the next."""
    return bytes(0x30 + (j * 5 + tag) % 75 for j in range(n))


def _rec(seq, name=b"r", flag=4, qual="ramp", **kw):
    from kmer_mapper_amd import reads_io
    return reads_io.bam_record(seq, name, flag, qual=ramp(len(seq)) if isinstance(qual, str) else qual, **kw)


def _payload(records, refs=(), text=b"@HD\tVN:1.6\tSO:unsorted\n"):
    from kmer_mapper_amd import reads_io
    return reads_io.bam_header(refs, text) + b"".join(records)


def _both(n, i):
    """The same record shape once with hits and once without: every feature has a kept and a dropped instance."""
    return (hit(n, 300 * i), miss(n, i))


# ------------------------------------------------------------------------------------------------ the bases
NAME_LENGTHS = (1, 63, 64, 65, 128, 254)                              # the lane seams of a 64-lane copy; 254 = the longest
BAD_NAMES = (b"tab\there", b"new\nline", b"sp ace", b"del\x7f", b"high\x80\xff", b"in\0ner", b"\t\n \x7f", b"\x1f!~\x7f")


def names_base():
    recs = []
    names = [name_of(n, n) for n in NAME_LENGTHS] + [b"*"] + list(BAD_NAMES)
    for i, nm in enumerate(names):
        for seq in _both(70 + i, i):
            recs.append(_rec(seq, nm))
    return Base("names", _payload(recs), sc.NO_SEL, False, False, False)


SEQ_LENGTHS = (0, 1, 2, 3, 127, 128, 129)
LONG = 2 * TILE + 7001                                                # bases: the record is longer than three tiles


def lengths_base():
    recs = []
    for i, n in enumerate(SEQ_LENGTHS):
        for j, seq in enumerate(_both(n, i)):
            recs.append(_rec(seq, b"len%d_%d" % (n, j)))
    recs.append(_rec(hit(60, 500) + miss(60, 50), b"half"))          # (its hits over its windows: below a pure slice's)
    for j, seq in enumerate(_both(LONG, 9)):
        recs.append(_rec(seq, b"long%d" % j, flag=0))
        recs.append(_rec(miss(40, 60 + j), b"behind%d" % j))
    for j, seq in enumerate(_both(LONG + 1, 10)):                    # (odd and even: the last byte's padding nibble)
        recs.append(_rec(revcomp(seq), b"rlong%d" % j, flag=0x10))
    return Base("lengths", _payload(recs), sc.NO_SEL, True, False, False)


def straddle_base():
    """Records whose head, whose name and whose qualities lie across a 16 KiB boundary of the inflated stream, each once with hits
    and once without; a filler record in front of each puts it there."""
    from kmer_mapper_amd import reads_io
    parts = [reads_io.bam_header((), b"@HD\tVN:1.6\n")]
    at, m = len(parts[0]), 1
    bare = len(_rec(miss(40, 900), b"fill"))
    across = []
    for kind in ("head", "name", "qual"):
        for j in range(2):
            seq = _both(150, 20 + m)[j]
            name = name_of(100, m) if kind == "name" else b"%s%d" % (kind.encode(), j)
            rec = _rec(seq, name)
            inside = {"head": 10, "name": 36 + 50, "qual": 36 + len(name) + 1 + 75 + 70}[kind]
            start = m * TILE - inside
            assert start - at >= bare
            parts.append(_rec(miss(40, 900 + m), b"fill", aux=b"Z" * (start - at - bare)))
            parts.append(rec)
            across.append((kind, start, len(rec)))
            at = start + len(rec)
            m += 1
    return Base("straddle", b"".join(parts), sc.NO_SEL, False, False, False), across


def strand_payload():
    recs = []
    for i, n in enumerate((1, 2, 61, 62, 127, 128)):
        h, x = _both(n, 30 + i)
        for j, (seq, flag) in enumerate(((h, 0), (h, 0x10), (revcomp(h), 0x10), (x, 0x10), (x, 0))):
            recs.append(_rec(seq, b"s%d_%d" % (n, j), flag))
    recs.append(_rec(revcomp(hit(90, 77)), b"noqual_rev", 0x10, qual=None))
    recs.append(_rec(b"", b"empty_rev", 0x10))
    return _payload(recs)


def mates_payload():
    recs = []
    for i, flag in enumerate((0x41, 0x81, 0xC1, 0x1, 0x40, 0x80)):
        for j, seq in enumerate(_both(80 + i, 40 + i)):
            recs.append(_rec(seq, name_of((3, 62, 63, 64, 20, 253)[i], j), flag))
    return _payload(recs)


def quals_base():
    recs = []
    for i, q in enumerate((None, 0, 92, 93, 254)):
        for j, seq in enumerate(_both(64 + i, 50 + i)):
            recs.append(_rec(seq, b"q%s_%d" % (str(q).encode(), j), qual=None if q is None else bytes([q]) * len(seq)))
    seq = hit(70, 900)
    recs.append(_rec(seq, b"ff_inside", qual=bytes([10, 255] + [j * 4 % 256 for j in range(68)])))   # (the first byte decides)
    return Base("quals", _payload(recs), sc.NO_SEL, False, False, False)


SELECTION = sc.Sel(0x400, 0x1, 20, [(0, 1000, 2000)], False)


def selection_base():
    """One rule after the other drops a record that lies between two selected ones: the output offsets skip."""
    M = lambda n: (n << 4,)
    shapes = [dict(flag=0x1, mapq=30, ref_id=0, pos=1200, cigar=M(60)),       # selected
              dict(flag=0x401, mapq=30, ref_id=0, pos=1200, cigar=M(60)),     # the exclude mask
              dict(flag=0x1, mapq=30, ref_id=0, pos=950, cigar=M(100)),       # selected: starts outside, its CIGAR reaches in
              dict(flag=0x0, mapq=30, ref_id=0, pos=1200, cigar=M(60)),       # the include mask
              dict(flag=0x11, mapq=20, ref_id=0, pos=1999, cigar=M(60)),      # selected
              dict(flag=0x1, mapq=19, ref_id=0, pos=1200, cigar=M(60)),       # the MAPQ floor
              dict(flag=0x1, mapq=30, ref_id=0, pos=950, cigar=M(50)),        # ends where the region starts
              dict(flag=0x1, mapq=30, ref_id=1, pos=1200, cigar=M(60)),       # another reference
              dict(flag=0x5, mapq=255, ref_id=-1, pos=-1, cigar=())]          # unplaced
    recs = []
    for rep in range(4):
        for i, shape in enumerate(shapes):
            seq = _both(60, 60 + i)[(rep + i) % 2]
            recs.append(_rec(seq, b"sel%d_%d" % (rep, i), next_ref_id=-1, **shape))
    return Base("selection", _payload(recs, sc.REFS3), SELECTION, False, False, False)


def big_base():
    """4 500 reads of 150 bases: the decoded text is over 1 MiB, so the selected records lie on both sides of a super-tile seam of
    the compaction, and so do the kept ones."""
    recs = []
    for i in range(4500):
        seq = miss(150, 100 + i) if i % 4 == 1 else hit(150, 37 * i)
        flag = 0x10 if i % 5 == 0 else 0
        recs.append(_rec(revcomp(seq) if flag else seq, b"read%d" % i, flag, qual=ramp(150, first=i % 40)))
    return Base("big", _payload(recs), sc.NO_SEL, True, False, False)


def all_codes_base():
    recs = [_rec(_NIB * 4 + b"A", b"codes_fwd", 0), _rec(_NIB * 4 + b"A", b"codes_rev", 0x10), _rec(_NIB * 4, b"codes_rev_even", 0x10)]
    return Base("all_codes", _payload(recs), sc.NO_SEL, True, False, True)


_BASES = None


def bases():
    global _BASES
    if _BASES is None:
        strand, mates = strand_payload(), mates_payload()
        out = [names_base(), lengths_base(), straddle_base()[0],
               Base("strand_read_orientation", strand, sc.NO_SEL, True, False, False),
               Base("strand_as_stored", strand, sc.NO_SEL, False, False, False),
               Base("mates_suffix", mates, sc.NO_SEL, False, True, False),
               Base("mates_no_suffix", mates, sc.NO_SEL, False, False, False),
               quals_base(), selection_base(),
               selection_base()._replace(name="selection_flags_only", sel=sc.NO_SEL._replace(excl=0x400)),
               big_base(), all_codes_base()]
        _BASES = {b.name: b for b in out}
    return _BASES


_ALL = None


def all_cases():
    """Every base under min_hits 1; min_hits 0, one above the largest count and invert on three of them; a permille threshold."""
    global _ALL
    if _ALL is None:
        out = [BCase(name + "__default", b, 1, 0, False) for name, b in bases().items()]
        for name in ("names", "lengths", "selection"):
            b = bases()[name]
            top = int(expected(BCase(name + "__default", b, 1, 0, False))[3].max())
            out.append(BCase(name + "__min_hits_0", b, 0, 0, False))
            out.append(BCase(name + "__above_the_largest", b, top + 1, 0, False))
            out.append(BCase(name + "__invert", b, 1, 0, True))
        out.append(BCase("lengths__permille_200", bases()["lengths"], 1, 200, False))
        out.append(BCase("big__invert", bases()["big"], 1, 0, True))
        _ALL = out
    return _ALL


def gpu_cases():
    return [c for c in all_cases() if not c.base.cpu_only]


# ------------------------------------------------------------------------------------------------ what keeps it from being vacuous
def features(base):
    """Per selected record of `base`, the set of the features it has."""
    out = []
    for r in decoded(base).records:
        f = set()
        if base.orig and r.flag & 0x10 and r.seq:
            f.add("reversed")
        if r.seq and r.qual[0] == 0xFF:
            f.add("absent qualities")
        if len(r.seq) % 2:
            f.add("odd l_seq")
        if len(r.name) >= 65:
            f.add("name of 65 bytes or more")
        if any(not 0x21 <= c <= 0x7E for c in r.name):
            f.add("replaced name byte")
        if mate_suffix(r.flag, base.suffix):
            f.add("mate suffix")
        if r.start // TILE != (r.start + r.size - 1) // TILE:
            f.add("across a tile boundary")
        out.append(f)
    return out


FEATURES = ("reversed", "absent qualities", "odd l_seq", "name of 65 bytes or more", "replaced name byte", "mate suffix",
            "across a tile boundary")
