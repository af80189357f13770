"""Records for "original_strand" (include/kmm.h): reads in READ ORIENTATION with a FLAG each, written the way an
aligner stores them — a read whose FLAG has 0x10 reverse-complemented, its qualities reversed — as BAM and as SAM.  With the
switch on the library has to hand the mapper the reads as they stand here; with it off, the stored text.  Pure Python / numpy, no
GPU; nothing here reads the library's kernels.

    a record                                (flag, SEQ in read orientation, QUAL as Phred+33 text in read orientation or None)
    revcomp(seq)                            the complement table of the issue, written out here (not reads_io.stored_form)
    stored(records)                         the same records as the file holds them
    bam_payload(records) / sam_bytes(..)    the inflated BAM bytes / the SAM text of the stored records
    text(records, ...)                      the two-line FASTA / four-line FASTQ the decoders have to write, switch on or off
    length_sweep(seed)                      every length of LENGTHS forward and reversed, interleaved
"""
import numpy as np

REVERSE = 0x10
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 150, 151, 255, 256, 257)
BAM_LETTERS = b"=ACMGRSVTWYHKDBN"
BAM_COMPLEMENT = b"=TGKCYSBAWRDMHVN"          # htslib's table: the letter of the bit-reversed code

_PAIRS = ("AT", "CG", "MK", "RY", "VB", "HD")
_COMP = {}
for _a, _b in _PAIRS:
    for _x, _y in ((_a, _b), (_b, _a), (_a.lower(), _b.lower()), (_b.lower(), _a.lower())):
        _COMP[ord(_x)] = ord(_y)


def revcomp(seq):
    """Reversed, every letter complemented; W, S, N, '=', '.', U and every other byte as they are; case kept."""
    return bytes(_COMP.get(c, c) for c in reversed(bytes(seq)))


def stored(records):
    """[(flag, SEQ, QUAL)] as the file holds them: FLAG 0x10 -> SEQ reverse-complemented, QUAL reversed."""
    return [(f, revcomp(s), None if q is None else q[::-1]) if f & REVERSE else (f, bytes(s), q) for f, s, q in records]


def bam_payload(records, refs=(), text=b"@HD\tVN:1.6\n"):
    """Header + the stored records, with names, CIGARs and tags of varying length (BAM qualities: raw Phred, None = 0xFF)."""
    from kmer_mapper_amd import reads_io
    out = [reads_io.bam_header(refs, text)]
    for i, (f, s, q) in enumerate(stored(records)):
        out.append(reads_io.bam_record(s, b"read%d" % i + b"x" * (i % 7), f, qual=None if q is None else bytes(c - 33 for c in q),
                                       cigar=(len(s) << 4,) * (i % 3), aux=b"NMC\x00" * (i % 4)))
    return b"".join(out)


def sam_bytes(records, crlf=False, upper=False):
    """Header lines + the stored records as SAM lines (SEQ "" -> "*", QUAL None or of an empty SEQ -> "*"), tags behind every
    second QUAL."""
    nl = b"\r\n" if crlf else b"\n"
    out = [b"@HD\tVN:1.6\tSO:unsorted" + nl, b"@CO\ta\tcomment\twith\ttabs\t\t\t\t\t\t\t\t" + nl]
    for i, (f, s, q) in enumerate(stored(records)):
        if upper:
            s = s.upper()
        assert q != b"*", "a one-base QUAL that reads '*' is absent"
        tag = b"\tNM:i:0\tRG:Z:g" if i % 2 else b""
        out.append(b"q%d\t%d\tchr1\t%d\t60\t%dM\t=\t0\t0\t%s\t%s%s" % (i, f, i + 1, max(len(s), 1), s or b"*", (q if s else None) or b"*", tag)
                   + nl)
    return b"".join(out)


def text(records, orig, qual, excl=0, upper=False):
    """What the decoders write for the kept records: orig — in read orientation, else as stored; qual — "@\\n" SEQ "\\n+\\n" QUAL
    "\\n" (absent: '~' per base), else ">\\n" SEQ "\\n".  upper: BAM has no lower case."""
    out = []
    for f, s, q in (records if orig else stored(records)):
        if f & excl:
            continue
        s = bytes(s).upper() if upper else bytes(s)
        out.append(b"@\n" + s + b"\n+\n" + (b"~" * len(s) if q is None else q) + b"\n" if qual else b">\n" + s + b"\n")
    return b"".join(out)


def n_flipped(records, excl=0):
    return sum(1 for f, s, _ in records if f & REVERSE and not f & excl and len(s))


def random_read(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(np.frombuffer(alphabet, np.uint8), size=int(n)))


def random_qual(rng, n):
    """Phred+33 text '!' .. '~' without '*' (a one-base QUAL "*" is absent), distinct enough that a reversal shows."""
    q = rng.integers(33, 127, size=int(n)).astype(np.uint8)
    q[q == ord("*")] = ord("I")
    return q.tobytes()


def length_sweep(seed, alphabet=b"ACGTN", absent=()):
    """Every length of LENGTHS as a forward and as a reversed record, interleaved (forward, reversed, reversed, forward, ...) so
    that a byte written one place too far lands in a neighbour of the other kind; `absent`: records without qualities."""
    rng = np.random.default_rng(seed)
    recs = []
    for i, n in enumerate(LENGTHS):
        for f in ((0, REVERSE) if i % 2 == 0 else (REVERSE | 1 | 64, 4)):
            recs.append((f, random_read(rng, n, alphabet), None if len(recs) in absent else random_qual(rng, n)))
    return recs
