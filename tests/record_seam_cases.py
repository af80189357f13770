"""FASTQ / two-line FASTA files for the seams of the record compaction (csrc/kmm_records.hpp: k_rec_count2 .. k_rec_uniform,
launched by rec_compact_piece in csrc/kmm.hip), and a line model of what kmm_map_records must make of them (include/kmm.h).
Pure Python / numpy, seeded, no GPU.

The compaction kernels work in units that a file of a few KB never crosses unless it is built for it; the builder here writes a
well-formed file and pads HEADER lines — never sequence content — until one chosen byte (the feature) lies at seam + delta:

    model(raw, fmt, brk, q, piece_bytes)    consumed, n_records, the sub-reads that may carry windows, the quality-masked bases,
                                            the expected error (kind, raw offset) or None, and whether the reads have one length
    naive_piece(...)                        the same rules once more, byte by byte, for tests/test_record_seam_cases_on_the_cpu.py
    CASES / build(name)                     a dict: name, feature, fmt, raw, grid, piece_kb, placements, error, twin
    seam_ok(case, placement)                is the placement's seam what its name says, given consumed and the hook's value?

tests/test_record_seam_cases_on_the_cpu.py holds every case to the condition it exists for.
"""
import numpy as np

from kmer_mapper_amd.util import LUT_BREAK, default_lut
from tests.ambiguous_cases import ACGT, GENOME, index_for  # noqa: F401 (index_for: for the GPU tier)

# ---------------------------------------------------------------------------------------------- geometry, stated once
# (all in csrc/kmm_records.hpp)
VEC = 16              # bytes of one vector load: rec_load16
LANE = 64             # bytes per lane: rec_load64, four vector loads
TILE = 4096           # REC_TB, bytes per tile = one wavefront's step
RELOAD = 64           # tiles per load of the per-tile table: k_rec_scatter, slot == 0
SUPER = 1024          # tiles per super-tile: k_rec_scatter, t >> 10
WAVES = 4             # wavefronts per workgroup: k_rec_scatter and k_rec_count2, per_wave = ceil(n_live / (4 * grid))

FASTQ, FASTA2 = 4, 2
FMT_NAME = {FASTQ: "fastq", FASTA2: "fasta2"}
DELTAS = (-2, -1, 0, 1)
Q = 20                                            # the quality floor of the QUAL variants
HIGH, FLOOR, JUST_LOW, LOW = ord("I"), 33 + Q, 33 + Q - 1, ord("#")
VARIANTS = {"plain": (False, 0), "brk": (True, 0), "qual": (False, Q), "brk_qual": (True, Q)}     # name -> (break table, floor)
CR, NL = 13, 10


def table(brk):
    """The default lookup table, or the one with KMM_LUT_BREAK on N / n."""
    t = default_lut()
    if brk:
        t[ord("N")] = t[ord("n")] = LUT_BREAK
    return t


def variants_of(case):
    """FASTA has no qualities: the floor has no effect there (include/kmm.h "min_base_quality")."""
    return ("plain", "brk", "qual", "brk_qual") if case["fmt"] == FASTQ else ("plain", "brk")


# ---------------------------------------------------------------------------------------------- the model
def _result(consumed=0, n_records=0, reads=(), total=0, n_masked=0, error=None, uniform_len=0):
    return dict(consumed=consumed, n_records=n_records, reads=list(reads), total=total, n_masked=n_masked, error=error,
                uniform_len=uniform_len)


def model_piece(raw, fmt, lut, q):
    """One piece (what one census sees).  The complete lines in groups of fmt; of every sequence line the bytes that are no
    '\\r' are the record's bases; a '\\r' that no '\\n' follows, a break byte and a base whose quality byte is below 33 + q
    split the read there (the latter two are dropped with it).  total: flat bases the piece appends (dead ones included)."""
    a = np.frombuffer(raw, np.uint8)
    nl = np.flatnonzero(a == NL)
    n_rec = nl.size // fmt
    if not n_rec:
        return _result()
    n_lines = n_rec * fmt
    consumed = int(nl[n_lines - 1]) + 1
    a = a[:consumed]
    is_nl, is_cr = a == NL, a == CR
    phase = (np.cumsum(is_nl) - is_nl) % fmt                      # (newlines before the byte) mod lines per record
    starts = np.concatenate([[0], nl[:n_lines - 1] + 1]).astype(np.int64)
    bad = []
    heads = starts[0::fmt]
    bad += list(heads[a[heads] != ord("@" if fmt == FASTQ else ">")])
    if fmt == FASTQ:
        plus = starts[2::4]
        bad += list(plus[a[plus] != ord("+")])
    term_cr = is_cr & np.concatenate([is_nl[1:], [False]])
    on_seq = phase == 1
    stream = on_seq & ~is_nl & ~is_cr
    before = np.concatenate([[0], np.cumsum(stream)]).astype(np.int64)            # before[i]: bases before raw byte i
    total = int(before[-1])
    bases = a[stream]
    entry = lut[bases]
    bad_base = np.flatnonzero(stream)[entry == 0xFF]
    dead = entry == LUT_BREAK
    marks = [before[starts[1::fmt]], before[np.flatnonzero(on_seq & is_cr & ~term_cr)]]
    n_masked = 0
    if q and fmt == FASTQ:
        qstream = (phase == 3) & ~is_nl & ~is_cr
        qbefore = np.concatenate([[0], np.cumsum(qstream)]).astype(np.int64)
        ends = nl[3:n_lines:4]
        bad += list(ends[before[ends] != qbefore[ends]])          # as many bases as quality bytes so far, at every quality line's end
        low = np.flatnonzero(a[qstream] < 33 + q)
        n_masked = int(low.size)
        dead[low[low < total]] = True
    f = np.flatnonzero(dead)
    marks = np.unique(np.concatenate(marks + [f, f + 1]))
    new_pos = np.concatenate([[0], np.cumsum(~dead)]).astype(np.int64)
    bounds = np.unique(np.concatenate([new_pos[marks[marks <= total]], [0, new_pos[-1]]]))
    kept = bases[~dead].tobytes()
    reads = [kept[s:e] for s, e in zip(bounds[:-1], bounds[1:])]
    error = ("malformed", int(min(bad))) if bad else ("invalid_base", int(bad_base.min())) if bad_base.size else None
    # one length: as many distinct read starts as records, every one a multiple of L = bases / records (k_rec_uniform)
    inner = marks[marks < total]
    L = total // n_rec if total and total % n_rec == 0 else 0
    uniform_len = L if L and inner.size == n_rec and not (inner % L).any() else 0
    return _result(consumed, n_rec, reads, total, n_masked, error, uniform_len)


def naive_piece(raw, fmt, lut, q):
    """model_piece once more, deliberately naive: one pass over the bytes with a line counter, no vector operation."""
    n_nl = 0
    for c in raw:
        if c == NL:
            n_nl += 1
    n_rec = n_nl // fmt
    if not n_rec:
        return _result()
    head = ord("@") if fmt == FASTQ else ord(">")
    reads, bad, bad_base, lengths = [], [], [], []
    n_masked = total = 0
    interior = False
    line = seen = consumed = 0
    at_start = True
    seq, cut_before, dead, quals = [], set(), set(), []
    for pos, c in enumerate(raw):
        if at_start:
            if line == 0 and c != head:
                bad.append(pos)
            if line == 2 and fmt == FASTQ and c != ord("+"):
                bad.append(pos)
            at_start = False
        if c == NL:
            seen += 1
            if line == fmt - 1:                                   # the record is complete
                if q and fmt == FASTQ:
                    if len(quals) != len(seq):
                        bad.append(pos)
                    for j, v in enumerate(quals):
                        if v < 33 + q:
                            n_masked += 1
                            if j < len(seq):
                                dead.add(j)
                n = len(seq)
                cur = bytearray()
                for j in range(n):
                    if j in cut_before or j in dead or (j - 1) in dead:
                        if cur:
                            reads.append(bytes(cur))
                        cur = bytearray()
                        if 0 < j:
                            interior = True
                    if j not in dead:
                        cur.append(seq[j])
                if cur:
                    reads.append(bytes(cur))
                lengths.append(n)
                total += n
                seq, cut_before, dead, quals = [], set(), set(), []
            line = (line + 1) % fmt
            at_start = True
            if seen == n_rec * fmt:
                consumed = pos + 1
                break
            continue
        if line == 1:
            if c == CR:
                if raw[pos + 1] != NL:
                    cut_before.add(len(seq))
            else:
                e = lut[c]
                if e == 0xFF:
                    bad_base.append(pos)
                if e == LUT_BREAK:
                    dead.add(len(seq))
                seq.append(c)
        elif line == 3 and q and c != CR:
            quals.append(c)
    error = ("malformed", min(bad)) if bad else ("invalid_base", min(bad_base)) if bad_base else None
    L = lengths[0]
    uniform_len = L if L and all(n == L for n in lengths) and not interior else 0
    return _result(consumed, n_rec, reads, total, n_masked, error, uniform_len)


def model(raw, fmt, brk=False, q=0, piece_bytes=None, piece=model_piece):
    """A whole kmm_map_records call: pieces of piece_bytes (None: one), every one starting where the last complete record of the
    one before ended; the reads of all pieces are one batch, mapped through the uniform route iff every piece has the same
    one length >= 16.  error: (kind, offset inside its piece, the piece's start) of the first piece that has one.
    pieces: (raw start, flat_base) of every piece."""
    raw = bytes(raw)
    lut = table(brk)
    pm = piece_bytes or (1 << 30)
    off = recs = flat = masked = 0
    L, reads, error, pieces = -1, [], None, []
    while off < len(raw):
        ln = min(len(raw) - off, pm)
        p = piece(raw[off:off + ln], fmt, lut, q)
        pieces.append((off, flat))
        if p["consumed"] > 0:
            L = p["uniform_len"] if L in (-1, p["uniform_len"]) else 0
            flat += p["total"]
        reads += p["reads"]
        masked += p["n_masked"]
        if error is None and p["error"]:
            error = p["error"] + (off,)
        off += p["consumed"]
        recs += p["n_records"]
        if p["consumed"] == 0 or ln < pm:
            break
    uniform = bool(flat > 0 and L >= 16 and L * recs == flat)
    return dict(consumed=off, n_records=recs, reads=reads, n_masked=masked, error=error, uniform=uniform, pieces=pieces, total=flat)


def reads_arrays(reads):
    """(bases, offsets) of a list of reads, as the oracle takes them."""
    offsets = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    return np.frombuffer(b"".join(reads), dtype=np.uint8), offsets


# ---------------------------------------------------------------------------------------------- the writer
class _Writer:
    """Appends records; advance_to(p) brings the file to length p exactly with filler records, the last one's header padded.
    Fillers are ragged reads from the genome with, here and there, an N, a few low quality bytes, lower case and "\\r\\n"
    lines, so that every file gives the four variants something to differ on."""

    def __init__(self, fmt, seed, quiet=False):
        self.fmt, self.rng, self.quiet = fmt, np.random.Generator(np.random.PCG64(seed)), quiet
        self.out, self.n, self.placed = bytearray(), 0, []

    def read(self, n):
        s = int(self.rng.integers(0, GENOME.shape[0] - n))
        return ACGT[GENOME[s:s + n]].tobytes()

    def rec(self, name, seq, qual, eol=b"\n", pad=0):
        head = (b"@" if self.fmt == FASTQ else b">") + name + (b" " + b"x" * (pad - 1) if pad else b"")
        if self.fmt == FASTQ:
            return head + eol + bytes(seq) + eol + b"+" + eol + bytes(qual) + eol
        return head + eol + bytes(seq) + eol

    def _filler(self):
        rng = self.rng
        n = int(rng.integers(40, 71))
        seq, qual = bytearray(self.read(n)), bytearray([HIGH]) * n
        qual[int(rng.integers(n))] = FLOOR                          # at the floor: alive
        eol = b"\n"
        if not self.quiet:
            if rng.random() < 0.15:
                seq[int(rng.integers(n))] = ord("N")
            if rng.random() < 0.2:
                j, ln = int(rng.integers(n)), int(rng.integers(1, 4))
                qual[j:j + ln] = bytes([JUST_LOW if rng.random() < 0.5 else LOW]) * len(qual[j:j + ln])
            if rng.random() < 0.08:
                seq = bytearray(bytes(seq).lower())
            if rng.random() < 0.1:
                eol = b"\r\n"
        self.n += 1
        return b"f%d" % self.n, seq, qual, eol

    def filler(self):
        self.out += self.rec(*self._filler())

    def advance_to(self, start):
        gap = start - len(self.out)
        assert gap == 0 or gap >= 200, ("no room for a padded filler", start, len(self.out))
        while start - len(self.out) > 600:
            self.filler()
        gap = start - len(self.out)
        if gap:
            f = self._filler()
            base = len(self.rec(*f))
            assert 0 <= gap - base, (gap, base)
            self.out += self.rec(*f, pad=gap - base)
        assert len(self.out) == start

    def place(self, seam, delta, seam_pos, made):
        rec, off, meta = made
        self.advance_to(seam_pos + delta - off)
        start = len(self.out)
        self.out += rec
        self.placed.append(dict(seam=seam, delta=delta, seam_pos=seam_pos, pos=seam_pos + delta, byte=rec[off], rec_start=start,
                                rec_len=len(rec), **{k: start + v for k, v in meta.items()}))


# ---------------------------------------------------------------------------------------------- the features
# name -> what the placed byte is; FASTQ_ONLY: features of the '+' and quality lines
FEATURES = {
    "nl_header": "the '\\n' that ends a header line",
    "nl_seq": "the '\\n' that ends a sequence line",
    "nl_plus": "the '\\n' that ends a '+' line",
    "nl_qual": "the '\\n' that ends a quality line",
    "crlf": "the '\\n' of a sequence line that ends in \"\\r\\n\" (delta 0: the pair straddles the seam)",
    "lone_cr": "a '\\r' in the middle of a sequence line",
    "first_header": "the '@' / '>' that starts a record",
    "first_plus": "the '+' that starts a record's third line",
    "break": "an N in the middle of a read: a break under the break table, an A under the default one",
    "low_qual": "one quality byte below the floor",
    "low_run": "byte 36 of a run of 70 quality bytes below the floor (longer than a lane and two bitset words)",
    "empty_seq": "the '\\n' of an empty sequence line",
    "long_seq": "the '\\n' of a sequence line of 9000 bases (tiles without any newline before it)",
    "long_header": "a '\\r' inside a header line of 5 KB that also holds '@', '+' and '>'",
    "qual_at": "the '@' that starts a quality line",
    "qual_plus": "the '+' that starts a quality line (Q10: below the floor)",
}
FASTQ_ONLY = ("nl_plus", "nl_qual", "first_plus", "low_qual", "low_run", "qual_at", "qual_plus")
LONG = ("long_seq", "long_header")
# damaged files: one byte of a well-formed composite file changed (or, for the quality line, one byte moved between the
# quality line and the header line of the same record, so that nothing else moves) -> (the composite's feature, the error);
# the same is done to that feature's reload file and to its four super-tile files, so every damage lies at every seam and delta
DAMAGED = {
    "bad_header": ("first_header", "malformed"),
    "bad_plus": ("first_plus", "malformed"),
    "bad_base": ("break", "invalid_base"),
    "qual_short": ("nl_qual", "malformed"),          # (with the floor set; well-formed without it: nothing new is checked)
    "qual_long": ("nl_qual", "malformed"),
}


def _feature_record(w, feature):
    """(record bytes, offset of the feature byte in it, offsets of the header's '\\n' and of the quality line's first byte)."""
    n = 9000 if feature == "long_seq" else 80 if feature == "low_run" else 0 if feature == "empty_seq" else 60
    w.n += 1
    name = b"r%d the feature" % w.n
    seq, qual = bytearray(w.read(n)) if n else bytearray(), bytearray([HIGH]) * n
    eol = b"\r\n" if feature == "crlf" else b"\n"
    if feature == "lone_cr":
        seq[25:25] = b"\r"
    elif feature == "break":
        seq[30] = ord("N")
    elif feature == "low_qual":
        qual[30] = JUST_LOW
    elif feature == "low_run":
        qual[5:75] = bytes([LOW, JUST_LOW]) * 35
    elif feature == "qual_at":
        qual[0] = ord("@")
    elif feature == "qual_plus":
        qual[0] = ord("+")
    elif feature == "long_header":
        name = b"r%d " % w.n + b"h" * 2500 + b"x\r@+>x" + b"h" * 2500
    rec = w.rec(name, seq, qual, eol)
    e = len(eol)
    h_nl = 1 + len(name) + e - 1
    s0 = h_nl + 1
    s_nl = s0 + len(seq) + e - 1
    p0 = s_nl + 1
    q0 = p0 + 1 + e
    off = {"nl_header": h_nl, "nl_seq": s_nl, "nl_plus": p0 + e, "nl_qual": len(rec) - 1, "crlf": s_nl, "lone_cr": s0 + 25,
           "first_header": 0, "first_plus": p0, "break": s0 + 30, "low_qual": q0 + 30, "low_run": q0 + 5 + 35, "empty_seq": s_nl,
           "long_seq": s_nl, "long_header": 1 + name.find(b"\r"), "qual_at": q0, "qual_plus": q0}[feature]
    return rec, off, dict(header_nl=h_nl, qual_start=q0)


def _plan(long_records):
    """[(seam, delta, seam position)] of a composite file and (its tiles, the hook's value): four blocks, one per delta, each with
    a vector, a lane, a wave-range start and an in-range tile seam."""
    block, at = (32, (3, 9, 16, 24)) if long_records else (4, (0, 0, 2, 3))       # (the long records span three tiles, twice in FASTQ)
    plan = []
    for i, delta in enumerate(DELTAS):
        b = block * i
        plan += [("vector", delta, (b + at[0]) * TILE + 592), ("lane", delta, (b + at[1]) * TILE + 2496),
                 ("wave", delta, (b + at[2]) * TILE), ("tile", delta, (b + at[3]) * TILE)]
    return plan, 4 * block, 2                                     # (grid 2: eight wavefronts of per_wave tiles)


COMPOSITE_SEAMS = ("vector", "lane", "wave", "tile")


def _composite(feature, fmt, seed):
    w = _Writer(fmt, seed)
    plan, n_tiles, grid = _plan(feature in LONG)
    for seam, delta, pos in plan:
        w.place(seam, delta, pos, _feature_record(w, feature))
    w.advance_to(n_tiles * TILE - 9)
    return dict(feature=feature, fmt=fmt, raw=bytes(w.out), grid=grid, placements=w.placed)


def _damage(case, kind, idx):
    """The composite with its idx-th placement damaged: (bytes, the error's offset)."""
    b, p = bytearray(case["raw"]), case["placements"][idx]
    if kind in ("bad_header", "bad_plus"):
        b[p["pos"]] = ord("x") if kind == "bad_header" else ord("-")
    elif kind == "bad_base":
        b[p["pos"]] = ord("X")
    elif kind == "qual_short":                                    # the header one byte longer, the quality line one byte shorter
        del b[p["qual_start"]]
        b[p["header_nl"]:p["header_nl"]] = b"x"
    else:
        b[p["qual_start"]:p["qual_start"]] = b"I"
        del b[p["header_nl"] - 1]
    assert len(b) == len(case["raw"])
    return bytes(b), p["pos"]


# reload: with the hook at 1, 280 tiles are 70 per wavefront: tile 64 of every range reloads the table
RELOAD_TILES = 280
# super-tile: 1040 tiles are 260 per wavefront; tile 1024 is tile 244 of the last range.  A super-tile seam costs the 4 MiB
# before it, in the same piece, so every (feature, delta) is a file of its own; the first 1012 tiles are the same in all of them
SUPER_FILE_TILES = 1040
SUPER_PREFIX_TILES = 1012
_PREFIX = {}


def _reload(feature, fmt, seed):
    w = _Writer(fmt, seed)
    per_wave = RELOAD_TILES // WAVES
    for i, delta in enumerate(DELTAS):
        w.place("reload", delta, (i * per_wave + RELOAD) * TILE, _feature_record(w, feature))
    w.advance_to(RELOAD_TILES * TILE - 9)
    return dict(feature=feature, fmt=fmt, raw=bytes(w.out), grid=1, placements=w.placed)


def super_prefix(fmt):
    """The records every super-tile file of a format starts with (built once)."""
    if fmt not in _PREFIX:
        w = _Writer(fmt, 4200 + fmt)
        w.advance_to(SUPER_PREFIX_TILES * TILE)
        _PREFIX[fmt] = bytes(w.out)
    return _PREFIX[fmt]


def _super(feature, delta, fmt, seed):
    w = _Writer(fmt, seed)
    w.out += super_prefix(fmt)
    w.n = 1 << 20
    w.place("super", delta, SUPER * TILE, _feature_record(w, feature))
    w.advance_to(SUPER_FILE_TILES * TILE - 9)
    return dict(feature=feature, fmt=fmt, raw=bytes(w.out), grid=1, placements=w.placed)


# limit / end of the chunk: the '\n' that ends the last complete record at seam + delta (delta -1: the record ends with the tile
# or the lane); "limit": an incomplete record follows — in FASTQ three complete lines, with 40 bases of the genome that would
# show in every count if they were mapped, and half a quality line.  (Its bytes are well-formed as far as they go: with a byte
# without a code and a line without '+' there, the host packer handed some of these calls to the device route.)
TAIL = {FASTQ: b"@tail\n" + ACGT[GENOME[777:817]].tobytes() + b"\n+\nIIII", FASTA2: b">tail ACGT"}
# "badtail": the same with a byte without a code among the bases and, in FASTQ, a third line without '+': neither may be
# reported, both lie behind the limit.  (The host packer may hand such a call to the device route: a slice that holds a byte
# without a code reports its own first byte — "somewhere in this slice" in csrc/kmm_hostpack.hpp — and where that lies before
# the limit the packer gives up, so "host_packed_record_calls" is not looked at for these files.)
_T = ACGT[GENOME[777:817]].tobytes()
TAIL_BAD = {FASTQ: b"@tail\n" + _T[:20] + b"X" + _T[20:] + b"\n-bad\nIIII", FASTA2: b">tail\n" + _T[:20] + b"X" + _T[20:]}
END_SEAMS = {"tile": 11 * TILE, "lane": 10 * TILE + 37 * LANE}          # (twelve tiles: three per wavefront with the hook at 1)


def _end(what, seam, delta, fmt, seed):
    w = _Writer(fmt, seed)
    rec, _, meta = _feature_record(w, "nl_seq")
    w.place(what + "_" + seam, delta, END_SEAMS[seam], (rec, len(rec) - 1, meta))
    if what != "end":
        w.out += (TAIL if what == "limit" else TAIL_BAD)[fmt]
    return dict(feature="record_end", fmt=fmt, raw=bytes(w.out), grid=1, placements=w.placed, any_route=what == "badtail")


# piece boundary: pieces of 32 KiB (two tiles per wavefront with the hook at 1); the '\n' that ends a record at (end of the first piece) + delta — delta -1: the record is the
# piece's last, delta 0: it is the next piece's first, and that piece starts at its header, wherever that lies
PIECE_KB = 32


def _piece(delta, fmt, seed):
    w = _Writer(fmt, seed)
    rec, _, meta = _feature_record(w, "nl_seq")
    w.place("piece", delta, PIECE_KB << 10, (rec, len(rec) - 1, meta))
    w.advance_to(20 * TILE - 9)
    return dict(feature="record_end", fmt=fmt, raw=bytes(w.out), grid=1, piece_kb=PIECE_KB, placements=w.placed)


# flat side: dst0 & 15 of tile t + 1 is v for v = 0 .. 15 (the sequence bytes before a tile start: the word two tiles share); an
# N and a low quality byte at flat positions 31 mod 32 (f + 1 opens the next bitset word); the last bases of the file low, and
# their number a multiple of 32 (the mark behind the last base is the first bit of a word that holds no base)
def _flat_side(fmt, seed):
    w = _Writer(fmt, seed)
    n_bases = 0

    def count():
        return model(bytes(w.out), fmt)["total"]
    for v in range(16):
        tile = (v + 1) * TILE
        while tile - len(w.out) > 900:
            w.filler()
        n_bases = count()
        n = 40 + (v - n_bases - 40) % 16                          # the read that brings the bases before the tile to v mod 16
        seq, qual = bytearray(w.read(n)), bytearray([HIGH]) * n
        j = (31 - n_bases) % 32                                   # flat position 31 mod 32
        if j < n - 1 and v % 2:
            seq[j] = ord("N")
        elif j < n - 1:
            qual[j] = JUST_LOW
        w.n += 1
        w.out += w.rec(b"a%d" % w.n, seq, qual)
        w.placed.append(dict(seam="flat_dst0", delta=v, seam_pos=tile, pos=tile, byte=ord("x"), rec_start=len(w.out), rec_len=0,
                             flat31=n_bases + j if j < n - 1 else -1, flat31_is_n=bool(v % 2)))
        # the next record's header spans the tile start
        name, seq, qual, eol = w._filler()
        w.out += w.rec(name, seq, qual, eol, pad=tile + 40 - len(w.out) - (1 + len(name)))
        assert w.out[tile] == ord("x"), "the tile starts inside a header's padding"
    n = 40 + (-(count() + 40)) % 32                               # the bases end with a bitset word: f + 1 of the last one opens the next
    w.n += 1
    w.out += w.rec(b"last%d" % w.n, w.read(n), bytes([HIGH]) * (n - 3) + bytes([LOW]) * 3)
    return dict(feature="flat_side", fmt=fmt, raw=bytes(w.out), grid=1, placements=w.placed)


# uniform detection: reads of one length L (the uniform route), and four near misses
UNIFORM_L = 40
UNIFORM = ("one_length", "one_length_lone_cr", "alternating", "length_15", "two_pieces")


def _uniform(kind, fmt, seed):
    w = _Writer(fmt, seed, quiet=True)
    L = 15 if kind == "length_15" else UNIFORM_L
    case = dict(feature="uniform", fmt=fmt, grid=1, placements=[])
    for i in range(120):
        n = L + (1 if i % 2 else -1) if kind == "alternating" else L
        seq = bytearray(w.read(n))
        if kind == "one_length_lone_cr" and i == 70:
            seq[10:10] = b"\r"
        if kind == "two_pieces" and len(w.out) >= 1024:
            n = L + 4
            seq = bytearray(w.read(n))
        rec = w.rec(b"u%d" % i, seq, bytes([HIGH]) * n)
        if kind == "two_pieces" and len(w.out) + len(rec) <= 1024 < len(w.out) + 2 * len(rec):
            rec = w.rec(b"u%d" % i, seq, bytes([HIGH]) * n, pad=1024 - len(w.out) - len(rec))     # the piece ends with this record
        w.out += rec
        if kind == "two_pieces" and len(w.out) >= 1850:
            break
    if kind == "two_pieces":
        case["piece_kb"] = 1
    case["raw"] = bytes(w.out)
    return case


# ---------------------------------------------------------------------------------------------- the registry
def _names():
    names = {}
    for fmt in (FASTQ, FASTA2):
        f = FMT_NAME[fmt]
        for feature in FEATURES:
            if fmt == FASTQ or feature not in FASTQ_ONLY:
                names["%s/%s" % (feature, f)] = ("composite", feature, fmt)
        for kind, (base, _) in DAMAGED.items():
            if fmt == FASTQ or base not in FASTQ_ONLY:
                for idx in range(16):
                    names["%s/%s/%d" % (kind, f, idx)] = ("damaged", kind, fmt, "%s/%s" % (base, f), idx)
                for idx in range(4):
                    names["reload_%s/%s/%d" % (kind, f, idx)] = ("damaged", kind, fmt, "reload/%s/%s" % (base, f), idx)
                for delta in DELTAS:
                    names["super_%s/%s/%d" % (kind, f, delta)] = ("damaged", kind, fmt, "super/%s/%s/%d" % (base, f, delta), 0)
        for what in ("limit", "badtail", "end"):
            for seam in END_SEAMS:
                for delta in DELTAS:
                    names["%s_%s/%s/%d" % (what, seam, f, delta)] = ("end", what, seam, delta, fmt)
        for delta in DELTAS:
            names["piece/%s/%d" % (f, delta)] = ("piece", delta, fmt)
        names["flat_side/%s" % f] = ("flat_side", fmt)
        for kind in UNIFORM:
            names["uniform_%s/%s" % (kind, f)] = ("uniform", kind, fmt)
        for feature in FEATURES:
            if fmt == FASTQ or feature not in FASTQ_ONLY:
                names["reload/%s/%s" % (feature, f)] = ("reload", feature, fmt)
                for delta in DELTAS:
                    names["super/%s/%s/%d" % (feature, f, delta)] = ("super", feature, delta, fmt)
    return names


CASES = _names()


def group_of(name):
    """The test a case runs in: its feature; the reload files: one test per feature; the super-tile files: one per feature and
    format (the four deltas)."""
    parts = name.split("/")
    return "/".join(parts[:3]) if parts[0] == "super" else "/".join(parts[:2]) if parts[0].startswith(("reload", "super_")) else parts[0]


def is_damaged(group):
    return any(CASES[n][0] == "damaged" for n in CASES if group_of(n) == group)


GROUPS = sorted({group_of(n) for n in CASES})
BIG = 2 << 20                                     # files beyond this are not all kept: the last few are
_BUILT, _BUILT_BIG = {}, {}


def _seed(name):
    return 7000 + sum((i + 1) * c for i, c in enumerate(name.encode())) % 100000


def build(name):
    """The case as a dict: name, feature, fmt, raw (uint8, read-only), grid ("debug_records_grid" the seams are computed for),
    piece_kb (0: one piece), placements, error (None, or (kind, offset, the floor it needs)), twin (the well-formed file a
    damaged one was made from)."""
    if name in _BUILT:
        return _BUILT[name]
    if name in _BUILT_BIG:
        return _BUILT_BIG[name]
    spec = CASES[name]
    error = twin = None
    if spec[0] == "composite":
        c = _composite(spec[1], spec[2], _seed(name))
    elif spec[0] == "damaged":
        kind, fmt, twin, idx = spec[1:]
        err = DAMAGED[kind][1]
        c = dict(build(twin))
        raw, pos = _damage(c, kind, idx)
        c.update(raw=raw, feature=kind, placements=[c["placements"][idx]])
        error = (err, pos, Q if kind.startswith("qual_") else 0)
    elif spec[0] == "end":
        c = _end(spec[1], spec[2], spec[3], spec[4], _seed(name))
    elif spec[0] == "piece":
        c = _piece(spec[1], spec[2], _seed(name))
    elif spec[0] == "flat_side":
        c = _flat_side(spec[1], _seed(name))
    elif spec[0] == "uniform":
        c = _uniform(spec[1], spec[2], _seed("uniform/%d" % spec[2]))          # (one seed: the same reads in every kind)
    elif spec[0] == "reload":
        c = _reload(spec[1], spec[2], _seed(name))
    else:
        c = _super(spec[1], spec[2], spec[3], _seed(name))
    if not isinstance(c["raw"], np.ndarray):
        raw = np.frombuffer(c["raw"], np.uint8)
        raw.setflags(write=False)
        c["raw"] = raw
    c.setdefault("piece_kb", 0)
    c.setdefault("any_route", False)
    c.update(name=name, error=error, twin=twin)
    if len(c["raw"]) > BIG:
        while len(_BUILT_BIG) >= 10:
            del _BUILT_BIG[next(iter(_BUILT_BIG))]
        _BUILT_BIG[name] = c
    else:
        _BUILT[name] = c
    return c


def model_of(case, variant="plain"):
    brk, q = VARIANTS[variant]
    return model(case["raw"].tobytes(), case["fmt"], brk, q, (case["piece_kb"] << 10) or None)


_SUMMARY = {}


def summary_of(case, variant="plain"):
    """model_of without the reads (n_reads: how many), kept for every case: what the CPU tier asks more than once."""
    key = (case["name"], variant)
    if key not in _SUMMARY:
        m = model_of(case, variant)
        m["n_reads"] = len(m.pop("reads"))
        _SUMMARY[key] = m
    return _SUMMARY[key]


# ---------------------------------------------------------------------------------------------- what a seam is
def wave_ranges(consumed, grid):
    """(tiles before the limit, tiles per wavefront) as k_rec_scatter computes them."""
    n_live = -(-consumed // TILE)
    return n_live, -(-n_live // (WAVES * grid))


def seam_ok(case, p, consumed):
    """Is p's seam position what its seam says, for the tile ranges that `consumed` and the case's hook value give?"""
    pos, seam = p["seam_pos"], p["seam"]
    n_live, per_wave = wave_ranges(consumed, case["grid"])
    tile, in_tile = divmod(pos, TILE)
    slot = tile % per_wave                                        # tiles behind the range's first
    if seam == "vector":
        return pos % VEC == 0 and pos % LANE != 0
    if seam == "lane":
        return pos % LANE == 0 and in_tile != 0
    if seam == "tile":
        return in_tile == 0 and slot != 0 and tile < n_live
    if seam == "wave":
        return in_tile == 0 and slot == 0 and 0 < tile < n_live
    if seam == "reload":
        return in_tile == 0 and slot == RELOAD and tile < n_live
    if seam == "super":
        return in_tile == 0 and tile == SUPER and slot % RELOAD != 0 and tile < n_live
    if seam in ("limit_tile", "badtail_tile", "end_tile"):
        return in_tile == 0
    if seam in ("limit_lane", "badtail_lane", "end_lane"):
        return pos % LANE == 0 and in_tile != 0
    if seam == "piece":
        return pos == case["piece_kb"] << 10
    if seam == "flat_dst0":
        return in_tile == 0
    raise KeyError(seam)
