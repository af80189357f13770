"""Multi-line FASTA for the device-side unwrap (KMM_FORMAT_FASTA, include/kmm.h; csrc/kmm_records.hpp k_ml_*):
files whose features sit where the unwrap can go wrong — the seams of a lane's 16 bytes, of a 1024-byte tile, of k_ml_scan's
round of 1024 tiles (= one super-tile of the scatter's prefix: 1 MiB), of a piece of a kmm_map_records call — not at the
workload's size.  Pure numpy, seeded, no GPU; nothing here reads the library's kernels or the host parser.

    unwrap_model(raw, last)         (two-line bytes, consumed): the rule of kmm.h and of the comment above k_ml_tile_last, vectorised
    unwrap_model_bytewise(raw, last) the same rule one byte at a time (the CPU tier holds the two to each other)
    reads_of(two_line_bytes)        (bases, offsets) of strict two-line FASTA; ValueError for anything else
    pieces_model(raw, last, piece)  what a call that cuts the chunk into pieces of `piece` bytes consumes, or where it fails
    index() / GENOME                the index every case is mapped against (k = 31), and the genome the reads are cut from
    CASES / build(name)             a dict: name, raw (uint8), plus what the case needs (see each builder)
    sweep_text(s) / SWEEP_SHIFTS    shift_sweep: the file whose first header is padded to s bytes
    sweep_conditions(s)             the names of the seam conditions that shift s puts somewhere in the file
    sweep_named_shifts()            condition -> the first shift that holds it
    seam_text(d) / SEAM_SHIFTS      round_seam: the file shifted by d bytes

tests/test_multiline_cases_on_the_cpu.py holds every case to the condition it exists for.
"""
import numpy as np

from kmer_mapper_amd import synthetic
from kmer_mapper_amd.kmer_index import KmerIndex

K = 31
LANE = 16            # bytes per lane of k_ml_flags / k_ml_scatter
TILE = 1024          # bytes per tile (one wavefront)
ROUND = 1024 * TILE  # bytes per round of k_ml_scan = per super-tile of the scatter's prefix sums
NL, CR, GT = 10, 13, ord(">")
GENOME = synthetic.make_genome(60_000, seed=7301)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

CASES = ["shift_sweep", "round_seam", "n_runs", "pieces", "long_record_in_pieces"]
SWEEP_SHIFTS = range(0, 1040)
SEAM_SHIFTS = range(-17, 18)
SEAM_PAD = 17                       # the first header's padding at shift 0
PIECE_KBS = (4, 16, 64)             # "debug_records_piece_kb" of the pieces tests
LONG_PIECE_KB = 4
N_RUN_LENGTHS = (1, 30, 31, 59, 60, 61, 200)
N_RUN_WIDTH = 60


# ---------------------------------------------------------------------------------------------- the model
def _as_u8(raw):
    return np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray)) else np.asarray(raw, dtype=np.uint8)


def keep_mask(raw):
    """keep[i]: byte i survives the unwrap.  A terminator is '\\n', or a '\\r' right before one; it is dropped iff its line
    does not start with '>' and the byte after it (after the "\\r\\n" for a '\\r') exists and is not '>'."""
    raw = _as_u8(raw)
    n = raw.shape[0]
    idx = np.arange(n, dtype=np.int64)
    is_nl = raw == NL
    next_is_nl = np.zeros(n, dtype=bool)
    next_is_nl[:-1] = is_nl[1:]
    is_cr = (raw == CR) & next_is_nl
    term = is_nl | is_cr
    # start of the line byte i lies on: one past the last '\n' BEFORE i
    last_nl_incl = np.maximum.accumulate(np.where(is_nl, idx, -1))
    line_start = np.zeros(n, dtype=np.int64)
    line_start[1:] = last_nl_incl[:-1] + 1
    header = raw[line_start] == GT
    after = idx + 1 + is_cr
    padded = np.concatenate([raw, np.full(2, GT, dtype=np.uint8)])          # "does not exist" reads like '>': kept
    next_is_seq = padded[after] != GT
    return ~term | header | ~next_is_seq


def header_starts(raw):
    """Starts of the header lines: a '>' at byte 0 or right behind a '\\n'."""
    raw = _as_u8(raw)
    gt = np.flatnonzero(raw == GT)
    return gt[(gt == 0) | (raw[np.maximum(gt - 1, 0)] == NL)]


def cut_model(raw, last):
    """consumed: with `last` everything, else the start of the last header line that is not at byte 0 (0: there is none)."""
    raw = _as_u8(raw)
    if last:
        return int(raw.shape[0])
    h = header_starts(raw)
    h = h[h > 0]
    return int(h[-1]) if h.shape[0] else 0


def unwrap_model(raw, last):
    raw = _as_u8(raw)
    consumed = cut_model(raw, last)
    return raw[:consumed][keep_mask(raw)[:consumed]].tobytes(), consumed


def unwrap_model_bytewise(raw, last):
    raw = bytes(_as_u8(raw))
    n = len(raw)
    out = bytearray()
    line_start, consumed = 0, 0
    kept = []
    for i in range(n):
        c = raw[i]
        if c == GT and i == line_start and i > 0:
            consumed = i
        term = c == NL or (c == CR and i + 1 < n and raw[i + 1] == NL)
        keep = True
        if term:
            nx = i + 2 if c == CR else i + 1
            keep = raw[line_start] == GT or not (nx < n and raw[nx] != GT)
        kept.append(keep)
        if c == NL:
            line_start = i + 1
    if last:
        consumed = n
    for i in range(consumed):
        if kept[i]:
            out.append(raw[i])
    return bytes(out), consumed


def reads_of(two_line):
    """(bases, offsets) of strict two-line FASTA: every line ends in '\\n', a '>' line and one sequence line alternate, a '\\r'
    at the end of the sequence line is no base.  Anything else is a ValueError (what the library reports as an error)."""
    buf = _as_u8(two_line)
    if buf.shape[0] == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    if buf[-1] != NL:
        raise ValueError("the last line has no newline")
    nl = np.flatnonzero(buf == NL)
    if nl.shape[0] % 2:
        raise ValueError("an odd number of lines")
    start = np.concatenate([[0], nl[:-1] + 1]).astype(np.int64)
    if not np.all(buf[start[0::2]] == GT):
        raise ValueError("a record does not start with '>'")
    s, e = start[1::2], nl[1::2].astype(np.int64)
    if np.any((e > s) & (buf[np.minimum(s, buf.shape[0] - 1)] == GT)):
        raise ValueError("a header line where a sequence line belongs")
    e = e - ((e > s) & (buf[np.maximum(e - 1, 0)] == CR))
    lens = e - s
    offsets = np.zeros(lens.shape[0] + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    take = np.repeat(s - offsets[:-1], lens) + np.arange(int(offsets[-1]), dtype=np.int64)
    return np.ascontiguousarray(buf[take]), offsets


def pieces_model(raw, last, piece):
    """A call that cuts the chunk into pieces of `piece` bytes (include/kmm.h: every piece starts where the one before it
    consumed to; only the piece that ends the chunk is told `last`).  ("ok", consumed) or ("record exceeds a piece", offset of
    the piece of full size that holds no whole record)."""
    raw = _as_u8(raw)
    n, off = raw.shape[0], 0
    while off < n:
        length = min(piece, n - off)
        used = cut_model(raw[off:off + length], last and off + length == n)
        if used == 0 and length == piece:
            return "record exceeds a piece", off
        off += used
        if used == 0 or length < piece:
            break
    return "ok", off


# ---------------------------------------------------------------------------------------------- the index
_INDEX = []


def _revcomp(kmers, k):
    out = np.zeros_like(kmers)
    for j in range(k):
        out |= (np.uint64(3) - ((kmers >> np.uint64(2 * j)) & np.uint64(3))) << np.uint64(2 * (k - 1 - j))
    return out


def index():
    """Every 31-mer of GENOME (node = position mod 5000), poly-A (node 5000: what a run of N reads as under the default
    table) and the reverse complement of every third one (nodes from 5001: also_revcomp counts something else)."""
    if not _INDEX:
        n = GENOME.shape[0] - K + 1
        fwd = synthetic.pack_kmers_strided(GENOME, n, 1, K)
        rev = _revcomp(fwd[::3], K)
        kmers = np.concatenate([fwd, np.zeros(1, dtype=np.uint64), rev])
        nodes = np.concatenate([np.arange(n, dtype=np.int64) % 5000, [5000], 5001 + np.arange(rev.shape[0], dtype=np.int64) % 1000])
        _INDEX.append(KmerIndex.from_flat_kmers(kmers, nodes, synthetic.next_prime(2 * kmers.shape[0])))
    return _INDEX[0]


# ---------------------------------------------------------------------------------------------- text
def _cut(rng, n):
    """n bases cut from the genome without errors (longer than the genome: stretches of 20 000 one after the other)."""
    out = []
    while n > 0:
        m = min(n, 20_000)
        s = int(rng.integers(0, GENOME.shape[0] - m))
        out.append(ACGT[GENOME[s:s + m]])
        n -= m
    return np.concatenate(out).tobytes() if out else b""


def record(name, seq, width, nl=b"\n", blank_after=(), blank_end=False):
    """b">name" + the sequence wrapped at `width` bases a line (0: one line; an empty sequence: one empty line), every line
    ended by nl; a blank line behind the sequence lines listed in blank_after, and behind the record with blank_end."""
    lines = [seq[i:i + width] for i in range(0, len(seq), width)] if (width and seq) else [seq]
    out = [b">" + name + nl]
    for i, ln in enumerate(lines):
        out.append(ln + nl)
        if i in blank_after:
            out.append(nl)
    if blank_end:
        out.append(nl)
    return b"".join(out)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# shift_sweep ------------------------------------------------------------------------------------
_SWEEP = {}


def _sweep_parts():
    """(the first record without its name, the body): eight records after the first, about 6 KiB."""
    if not _SWEEP:
        rng = _rng(7311)
        first_seq = _cut(rng, 40)
        body = [
            record(b"w1", _cut(rng, 100), 1, b"\r\n"),
            record(b"w15", _cut(rng, 200), 15),
            record(b"w16", _cut(rng, 200), 16, b"\r\n"),
            b">h\n\n",                                                     # its only sequence line is empty: a read of length 0
            record(b"w17", _cut(rng, 200), 17, blank_end=True),            # a blank line between two records
            record(b"w60", _cut(rng, 600), 60, b"\r\n", blank_after=(3,)),  # a blank line inside a record
            record(b"one_line", _cut(rng, 3000), 0, b"\r\n"),              # a line longer than two tiles
            record(b"w1023", _cut(rng, 1500), 1023),
        ]
        _SWEEP["first_seq"], _SWEEP["body"] = first_seq, b"".join(body)
    return _SWEEP["first_seq"], _SWEEP["body"]


def sweep_text(s):
    first_seq, body = _sweep_parts()
    return record(b"x" * s, first_seq, 25) + body


SWEEP_CONDITIONS = ("cr_last_of_tile", "cr_last_of_lane", "header_first_of_tile", "last_header_at_1023", "last_header_at_0",
                    "last_header_at_1", "last_header_at_lane_start", "seq_nl_last_of_tile")


def sweep_conditions(s, raw=None):
    """Which of SWEEP_CONDITIONS the file of shift s holds, read from its bytes."""
    raw = _as_u8(sweep_text(s) if raw is None else raw)
    n = raw.shape[0]
    found = set()
    cr = np.flatnonzero(raw == CR)
    cr = cr[(cr + 1 < n)]
    cr = cr[raw[cr + 1] == NL]
    if np.any(cr % TILE == TILE - 1):
        found.add("cr_last_of_tile")           # (its '\n' is byte 0 of the next tile)
    if np.any(cr % LANE == LANE - 1):
        found.add("cr_last_of_lane")
    heads = header_starts(raw)
    if np.any((heads % TILE == 0) & (heads > 0)):
        found.add("header_first_of_tile")      # directly behind a '\n': the last byte of the tile before
    p = int(heads[-1])
    for r in (TILE - 1, 0, 1):
        if p % TILE == r:
            found.add("last_header_at_%d" % r)
    if p % LANE == 0 and p % TILE != 0:
        found.add("last_header_at_lane_start")
    # a '\n' that ends a sequence line and is followed by a sequence line (neither blank): the byte the unwrap drops
    nl = np.flatnonzero(raw == NL)
    nl = nl[(nl % TILE == TILE - 1) & (nl + 1 < n)]
    for q in nl:
        start = int(np.flatnonzero(raw[:q] == NL)[-1]) + 1 if np.any(raw[:q] == NL) else 0
        if raw[start] not in (GT, NL, CR) and raw[q - 1] != CR and raw[q + 1] not in (GT, NL, CR):
            found.add("seq_nl_last_of_tile")
    return found


_NAMED = {}


def sweep_named_shifts():
    """condition -> the first shift that holds it (every condition has one, or the CPU tier fails)."""
    if not _NAMED:
        for s in SWEEP_SHIFTS:
            for cond in sweep_conditions(s):
                _NAMED.setdefault(cond, s)
    return dict(_NAMED)


# round_seam -------------------------------------------------------------------------------------
_SEAM = {}


def _seam_parts():
    """The file without its first header.  At shift 0 the '>' of the last record is byte 2 * ROUND; the long line's own
    terminator lies 10 bytes before it, behind it a further sequence line of 8 bases of the same record."""
    if not _SEAM:
        rng = _rng(7321)
        head_len = 1 + SEAM_PAD + 1                                        # b">" + padding + b"\n"
        parts, pos, i = [_cut(rng, 500) + b"\n"], head_len + 501, 0
        while pos < 800 * TILE:
            rec = record(b"r%d" % i, _cut(rng, int(rng.integers(100, 3001))), 70, b"\r\n" if i % 3 == 1 else b"\n")
            parts.append(rec)
            pos += len(rec)
            i += 1
        parts.append(b">long\n")
        pos += 6
        long_len = 2 * ROUND - 10 - pos
        tail = _cut(rng, 8)
        parts.append(_cut(rng, long_len) + b"\n" + tail + b"\n")
        pos += long_len + 10
        assert pos == 2 * ROUND
        parts.append(record(b"last", _cut(rng, 500_000), 70))
        _SEAM.update(rest=b"".join(parts), long_start=pos - long_len - 10, long_len=long_len)
    return _SEAM


def seam_text(d):
    return b">" + b"x" * (SEAM_PAD + d) + b"\n" + _seam_parts()["rest"]


def seam_layout(d):
    """Raw offsets in the file of shift d: the '\\n' before the long line, the long line's own '\\n', the last record's '>'."""
    p = _seam_parts()
    return dict(nl_before=p["long_start"] - 1 + d, long_nl=p["long_start"] + p["long_len"] + d, last_header=2 * ROUND + d)


# n_runs -----------------------------------------------------------------------------------------
def _n_runs():
    rng = _rng(7331)
    recs, i = [], 0
    for run in N_RUN_LENGTHS:
        for col in range(N_RUN_WIDTH):          # the run starts at every column of a line, and so ends at every one
            seq = bytearray(_cut(rng, N_RUN_WIDTH + col + run + 100))
            seq[N_RUN_WIDTH + col:N_RUN_WIDTH + col + run] = b"N" * run
            recs.append(record(b"n%d_%d" % (run, col), bytes(seq), N_RUN_WIDTH, b"\r\n" if i % 4 == 3 else b"\n"))
            i += 1
    return b"".join(recs)


# pieces -----------------------------------------------------------------------------------------
def _pieces():
    rng = _rng(7341)
    recs, size, i = [], 0, 0
    while size < 300 * 1024:
        rec = record(b"p%d" % i, _cut(rng, int(rng.integers(50, 3001))), 80, b"\r\n" if rng.random() < 0.4 else b"\n")
        recs.append(rec)
        size += len(rec)
        i += 1
    return b"".join(recs)


def _long_record():
    rng = _rng(7351)
    middle = record(b"middle", _cut(rng, 10 * 1024 - 8 - 127), 80)          # 127 lines: 10 KiB with its header
    assert len(middle) == 10 * 1024
    return record(b"before", _cut(rng, 700), 80) + middle + record(b"after", _cut(rng, 900), 80, b"\r\n")


_BUILT = {}


def build(name):
    """name -> dict(name, raw): raw is the file as a read-only uint8 array (shift_sweep: of shift 0; round_seam: of shift 0)."""
    if name not in _BUILT:
        text = {"shift_sweep": lambda: sweep_text(0), "round_seam": lambda: seam_text(0), "n_runs": _n_runs, "pieces": _pieces,
                "long_record_in_pieces": _long_record}[name]()
        raw = np.frombuffer(text, dtype=np.uint8)
        _BUILT[name] = dict(name=name, raw=raw, text=text)
    return _BUILT[name]
