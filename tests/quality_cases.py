"""FASTQ records with low-quality bases for "min_base_quality" (include/kmm.h): with a floor Q > 0 a base whose
quality byte is below '!' + Q is a break — no k-mer that contains it is counted, the windows on either side of it are.  The
cases put low bytes where the compaction kernels can go wrong — the edges of their 4 KiB tiles (in the raw text and in flat
space), of a line, of a read, of a piece — not at the workload's size.  Pure numpy, seeded, no GPU; nothing here reads the
library's kernels.

    split_at_mask(bases, offsets, mask)     the same reads with every masked base dropped and a read boundary where it stood:
                                            what a masked base is DEFINED to be equivalent to; the oracle maps those
    surviving_windows(offsets, k, mask)     brute force: the windows inside one read that hold no masked base
    dead_mask(case, q=None)                 the bases the case's floor (or another one) kills, the skip table's breaks included
    CASES / build(name)                     a dict: name, bases, quals, offsets, k, q, use_lut, pins, crlf
    fastq_text(bases, quals, offsets, ..)   the records as text, names padded so that chosen bytes fall on chosen raw offsets
    case_text(case)                         (text, where, layout) of a case
    index_for(k)                            the index every case of that k is mapped against (tests/ambiguous_cases.py)

tests/test_quality_cases_on_the_cpu.py holds every case to the condition it exists for.
"""
import numpy as np

from tests.ambiguous_cases import GENOME, ACGT, index_for, break_mask, is_uniform  # noqa: F401 (index_for, is_uniform: for the tests)
from kmer_mapper_amd.util import ambiguous_skip_lut

K = 31
L = 150
TILE = 4096          # bytes per tile of the records compaction kernels (REC_TB)
PIECE_KB = 16        # "debug_records_piece_kb" of the several-pieces test: tile_edges' 125 KB make eight pieces
HIGH = ord("I")      # Q40

CASES = ["tile_edges", "line_boundaries", "read_ends", "run_of_40", "pairs_k_apart", "pairs_k_apart-k12", "pairs_k_apart-k2",
         "degenerate_reads", "ragged_1_to_400", "long_read", "decoy_characters", "q1", "q93", "all_41_values", "with_skip_table"]
UNIFORM = ("tile_edges", "line_boundaries", "read_ends", "run_of_40", "pairs_k_apart", "pairs_k_apart-k12", "pairs_k_apart-k2",
           "decoy_characters", "q1", "q93", "all_41_values", "with_skip_table")
FLAT_EDGES = (0, 1023, 1024, 4095, 4096, 8191, 8192)


# ---------------------------------------------------------------------------------------------- tools of both tiers
def split_at_mask(bases, offsets, mask):
    """(bases', offsets'): the masked bases dropped, a read boundary wherever one stood (empty reads are left out: they hold
    no window)."""
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    mask = np.asarray(mask, dtype=bool)
    new_pos = np.zeros(bases.shape[0] + 1, dtype=np.int64)      # position of base p among the kept bases
    np.cumsum(~mask, out=new_pos[1:])
    bounds = np.concatenate([new_pos[offsets], new_pos[np.flatnonzero(mask) + 1], [0, new_pos[-1]]])
    return np.ascontiguousarray(bases[~mask]), np.unique(bounds).astype(np.int64)


def surviving_windows(offsets, k, mask):
    """Flat start positions of the windows of k bases inside one read that hold no masked base."""
    offsets = np.asarray(offsets, dtype=np.int64)
    total = int(offsets[-1])
    before = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(np.asarray(mask, dtype=bool), out=before[1:])
    read_of = np.repeat(np.arange(offsets.shape[0] - 1), np.diff(offsets))
    p = np.arange(total, dtype=np.int64)
    p = p[p + k <= offsets[1:][read_of]]
    return p[before[p + k] == before[p]]


def low_mask(quals, q):
    """The bases a floor of q masks: quality byte (unsigned) below '!' + q; q = 0 masks nothing."""
    return (np.asarray(quals, dtype=np.uint8) < 33 + int(q)) if q else np.zeros(len(quals), dtype=bool)


def dead_mask(case, q=None, with_lut=None):
    m = low_mask(case["quals"], case["q"] if q is None else q)
    if case["use_lut"] if with_lut is None else with_lut:
        m = m | break_mask(case["bases"], ambiguous_skip_lut())
    return m


# ---------------------------------------------------------------------------------------------- the text
def fastq_text(bases, quals, offsets, pins=(), crlf=()):
    """The records as FASTQ bytes: (text, where, layout).
    pins: (read, kind, offset, residue) — the name of that read is padded until the byte lies at a raw offset = residue mod
    4096; kind "seq" / "qual": byte `offset` of the sequence / quality line, "seq_nl": the newline that ends the sequence
    line, "plus": the '+'.  where[(read, kind, offset)] = the raw offset it got.  One pin per read.
    crlf: reads whose four lines end in "\\r\\n"; every fifth record does anyway.
    layout[i] = (raw offset of the record, of its sequence line, of its quality line, of the quality line's newline)."""
    bases = np.asarray(bases, dtype=np.uint8)
    quals = np.asarray(quals, dtype=np.uint8)
    pin_of = {}
    for read, kind, offset, residue in pins:
        assert read not in pin_of, "one pin per read"
        pin_of[int(read)] = (kind, int(offset), int(residue))
    crlf = set(int(i) for i in crlf)
    out, pos, where, layout = [], 0, {}, []
    for i in range(len(offsets) - 1):
        seq = bases[offsets[i]:offsets[i + 1]].tobytes()
        qual = quals[offsets[i]:offsets[i + 1]].tobytes()
        nl = b"\r\n" if (i % 5 == 2 or i in crlf) else b"\n"
        head = b"@r%d" % i

        def at(kind, o):
            first_seq = len(head) + len(nl)
            return {"seq": first_seq + o, "seq_nl": first_seq + len(seq) + len(nl) - 1, "plus": first_seq + len(seq) + len(nl),
                    "qual": first_seq + len(seq) + len(nl) + 1 + len(nl) + o}[kind]
        if i in pin_of:
            kind, o, residue = pin_of[i]
            pad = (residue - (pos + at(kind, o))) % TILE
            if pad:
                head += b" " + b"x" * (pad - 1)
            where[(i, kind, o)] = pos + at(kind, o)
        layout.append((pos, pos + at("seq", 0), pos + at("qual", 0), pos + at("qual", len(seq)) + len(nl) - 1))
        rec = head + nl + seq + nl + b"+" + nl + qual + nl
        out.append(rec)
        pos += len(rec)
    return b"".join(out), where, layout


def case_text(case):
    return fastq_text(case["bases"], case["quals"], case["offsets"], case["pins"], case["crlf"])


def second_piece_record(layout, piece_bytes):
    """The record a kmm_map_records call's second piece starts on: the first one that does not end inside the first piece."""
    ends = [rec[3] + 1 for rec in layout]
    return next(i for i, e in enumerate(ends) if e > piece_bytes)


# ---------------------------------------------------------------------------------------------- the cases
def _reads(lengths, seed):
    """Reads drawn from the genome without errors: every window hits the index, so every masked base shows in the counts."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lengths = np.asarray(lengths, dtype=np.int64)
    offsets = np.zeros(lengths.shape[0] + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    starts = rng.integers(0, GENOME.shape[0] - int(lengths.max()) - 64, size=lengths.shape[0])
    bases = np.empty(int(offsets[-1]), dtype=np.uint8)
    for r, (s, n) in enumerate(zip(starts, lengths)):
        bases[offsets[r]:offsets[r + 1]] = ACGT[GENOME[s:s + n]]
    return bases, offsets, rng


def _low_value(q, i):
    """A quality byte below the floor: every second one just below it (so that the floor below tells), the others further down."""
    return max(33, 33 + q - 1 - (i % 3) * 5)


def build(name):
    """The case as a dict (see the module docstring).  quals: 'I' (or the floor's own byte where that is higher) everywhere,
    the floor's own byte — NOT masked — on 3 % of the bases so that the next floor up tells, low bytes where the case wants."""
    k = 12 if name.endswith("-k12") else 2 if name.endswith("-k2") else K
    q = {"q1": 1, "q93": 93}.get(name, 20)
    use_lut, pins, crlf, low = False, [], set(), []

    def flat(read, offset):
        return int(offsets[read] + offset)

    if name == "tile_edges":
        bases, offsets, rng = _reads([L] * 400, 21)
        total = 400 * L
        low = list(FLAT_EDGES) + [total - 1, total - k]
        low += [flat(130, 40), flat(260, 75)]
        pins = [(130, "qual", 40, TILE - 1), (260, "qual", 75, 0)]       # a low byte as the last / the first byte of a tile
        crlf = {130, 260, 0, 399}
    elif name == "line_boundaries":
        bases, offsets, rng = _reads([L] * 120, 22)
        # record 30: its sequence line's newline is the last byte of a tile, so the quality line lies in the next one;
        # record 70: its quality line straddles a tile boundary (byte 70 is a tile's first), low on both sides of it
        pins = [(30, "seq_nl", 0, TILE - 1), (70, "qual", 70, 0), (100, "seq_nl", 0, TILE - 1)]
        low = [flat(30, 0), flat(30, 1), flat(30, L - 1), flat(70, 69), flat(70, 70), flat(70, 0), flat(100, 0), flat(100, 77)]
        crlf = {70, 100}
    elif name == "read_ends":
        bases, offsets, rng = _reads([L] * 300, 23)
        low = [flat(r, 0) for r in (3, 50, 27, 0, 200)] + [flat(r, L - 1) for r in (7, 120, 54, 200, 299)]
        crlf = {3, 7, 200}
    elif name == "run_of_40":
        bases, offsets, rng = _reads([L] * 300, 24)
        low = [flat(10, o) for o in range(50, 90)] + list(range(4080, 4120)) + [flat(150, o) for o in range(L - 40, L)]
        crlf = {150}
    elif name.startswith("pairs_k_apart"):
        bases, offsets, rng = _reads([L] * 200, 25)
        for read in (4, 30, 100):        # k + 1 apart: exactly one window survives between them
            low += [flat(read, 40), flat(read, 40 + k + 1)]
        for read in (9, 27, 150):        # k apart: none does
            low += [flat(read, 60), flat(read, 60 + k)]
        low += [flat(27, 45), flat(27, 46)]          # (flat 4095 and 4096)
    elif name == "degenerate_reads":
        lengths = [L] * 200
        lengths[20], lengths[21], lengths[22], lengths[120], lengths[40], lengths[199] = 20, 1, k - 1, k, 0, 0
        lengths[41], lengths[42] = 1, k
        bases, offsets, rng = _reads(lengths, 26)
        low = [flat(5, o) for o in range(L)]         # a read that is all low
        low += [flat(20, 7), flat(21, 0), flat(120, k // 2), flat(60, 75), flat(22, 0)]
        crlf = {40, 21}                              # (an empty read with "\r\n" lines)
    elif name == "ragged_1_to_400":
        rng0 = np.random.Generator(np.random.PCG64(127))
        lengths = rng0.integers(1, 401, size=260)
        lengths[3], lengths[7] = 1, 400
        bases, offsets, rng = _reads(lengths, 27)
        total = int(offsets[-1])
        low = list(np.flatnonzero(rng0.random(total) < 0.05)) + list(FLAT_EDGES) + [total - 1, total - k]
    elif name == "long_read":
        bases, offsets, rng = _reads([L] * 10 + [10_000] + [L] * 10, 28)
        pins = [(10, "seq", 0, 100)]                 # the long read's sequence starts 100 bytes into a tile
        low = [flat(10, 0), flat(10, 9_999), flat(11, 0), flat(9, L - 1)]
    elif name == "decoy_characters":
        bases, offsets, rng = _reads([L] * 60, 29)
        low = [flat(50, 70), flat(51, 0), flat(52, L - 1)]
    elif name in ("q1", "q93"):
        bases, offsets, rng = _reads([L] * 100, 30)
        low = [flat(r, o) for r, o in ((0, 0), (3, 17), (3, 18), (50, 149), (77, 60), (77, 60 + k + 1), (99, 149))]
        if name == "q93":                            # everything but '~' dies: one read keeps two stretches of it
            low = [p for p in range(int(offsets[-1])) if not (flat(40, 10) <= p < flat(40, 60) or flat(41, 100) <= p < flat(42, 50))]
    elif name == "all_41_values":
        bases, offsets, rng = _reads([L] * 200, 31)
    elif name == "with_skip_table":
        bases, offsets, rng = _reads([L] * 120, 32)
        use_lut = True
        for r, o in ((10, 50), (20, 60), (30, 70), (40, 0), (50, L - 1), (8, 33)):
            # the reads that get an N are drawn where the genome has an A there: N read as A (the default table) then hits
            # the index, and the counts tell a library that applies the floor but forgets the table
            s0 = int(rng.integers(0, GENOME.shape[0] - 2 * L - 64))
            while GENOME[s0 + o] != 0:
                s0 += 1
            bases[offsets[r]:offsets[r + 1]] = ACGT[GENOME[s0:s0 + L]]
        for r in range(1, 120, 7):                   # lower-case reads
            bases[offsets[r]:offsets[r + 1]] |= 0x20
        n_high, n_low, beside = flat(10, 50), flat(20, 60), flat(30, 70)
        bases[[n_high, n_low, beside, flat(40, 0), flat(50, L - 1)]] = ord("N")
        bases[flat(8, 33)] = ord("n")
        low = [n_low, beside + 1, flat(31, 70), flat(8, 34), flat(8, 90), flat(60, 10), flat(50, L - 2)]
    else:
        raise KeyError(name)

    total = int(offsets[-1])
    floor_byte = 33 + q
    quals = np.full(total, max(HIGH, floor_byte), dtype=np.uint8)
    quals[rng.random(total) < 0.03] = floor_byte     # exactly at the floor: alive
    if name == "all_41_values":
        # '!' .. 'I', every value; nine bases in ten from the upper half, as a sequencer's are
        quals = np.where(rng.random(total) < 0.9, rng.integers(53, 74, size=total), rng.integers(33, 74, size=total)).astype(np.uint8)
    for i, p in enumerate(sorted(set(int(p) for p in low))):
        quals[p] = _low_value(q, i)
    if name == "decoy_characters":
        # quality lines that start with '@' (Q31: alive at Q20) and with '+' (Q10: low), one made of '@' alone, "@" and "+"
        # in the middle of a line, and a line that starts with "@r" like a header
        for r in (5, 17, 33):
            quals[flat(r, 0)] = ord("@")
        for r in (6, 18, 34):
            quals[flat(r, 0)] = ord("+")
        quals[flat(40, 0):flat(41, 0)] = ord("@")
        quals[flat(41, 0):flat(41, 2)] = np.frombuffer(b"@r", np.uint8)
        quals[flat(42, 50)], quals[flat(42, 51)] = ord("+"), ord("@")
        quals[flat(43, 0):flat(43, 3)] = ord("+")
        crlf = {6, 40}
    case = dict(name=name, bases=bases, quals=quals, offsets=offsets, k=k, q=q, use_lut=use_lut, pins=pins, crlf=crlf)
    if name == "long_read":
        # low bytes at every tile boundary of the long read's quality line (the last byte of a tile and the first of the next)
        _, _, layout = case_text(case)
        q0 = layout[10][2]
        for edge in range((q0 // TILE + 1) * TILE, q0 + 10_000, TILE):
            quals[flat(10, edge - q0 - 1)] = _low_value(q, 0)
            quals[flat(10, edge - q0)] = _low_value(q, 1)
    if name == "tile_edges":
        # the several-pieces test cuts this text into pieces of PIECE_KB: the record its second piece starts on begins low
        _, _, layout = case_text(case)
        quals[flat(second_piece_record(layout, PIECE_KB << 10), 0)] = _low_value(q, 0)
    for a in (bases, quals, offsets):
        a.setflags(write=False)
    return case
