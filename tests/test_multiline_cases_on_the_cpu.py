"""tests/multiline_cases.py held to the conditions its cases exist for, and its model of the unwrap held to the host parser
(kmer_mapper_amd/reads_io.py: parse_fasta_block, records_cut) wherever the two are meant to agree.  No GPU: a case that no
longer contains what it is for fails here, not silently in tests/test_gpu_multiline_fasta.py."""
import numpy as np
import pytest

from tests import multiline_cases as mc
from kmer_mapper_amd import reads_io

TILE, LANE, ROUND = mc.TILE, mc.LANE, mc.ROUND


def _u8(b):
    return np.frombuffer(b, dtype=np.uint8)


def _same_reads(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _host(raw):
    batch = reads_io.parse_fasta_block(_u8(raw) if isinstance(raw, bytes) else np.ascontiguousarray(raw))
    return batch.bases, batch.offsets


def _agrees_with_host_parser(raw, what):
    """Model == host parser on the chunk `raw`, with and without "the chunk ends the file"."""
    raw = np.ascontiguousarray(raw)
    two, used = mc.unwrap_model(raw, True)
    assert used == raw.shape[0] == reads_io.records_cut(raw, "fasta_ml", True), what
    if raw[mc.header_starts(raw)[-1]:].tobytes().count(b"\n") == 1:
        # the chunk ends behind a header line: an empty read for the host parser, a record without a sequence line (an error)
        # for the model — the same reads once the empty line is written out
        with pytest.raises(ValueError):
            mc.reads_of(two)
        two += b"\n"
    assert _same_reads(mc.reads_of(two), _host(raw)), what
    two, used = mc.unwrap_model(raw, False)
    assert used == reads_io.records_cut(raw, "fasta_ml", False), what
    assert _same_reads(mc.reads_of(two), _host(raw[:used])), what


def _line_ends(raw):
    return np.flatnonzero(raw == mc.NL) + 1


# ---------------------------------------------------------------------------------------------- the model
HAND = [b">a\nAC\nGT\n>b\nA\n", b">a\r\nAC\r\nGT\r\n>b\r\nA\r\n", b">a\nAC\n\nGT\n\n>b\n\n>c\nA\n\n", b">a\n\n", b">a\nAC\rGT\nA\n>b\nC\n",
        b">a\n>b\nACGT\n", b">a\n>b\n", b">a\nAC\n>b\n", b"AC\n>a\nAC\n", b">a\nAC\nGT", b">a\nACGT\r", b"\n\n", b">", b"\r\n>a\r\n\r\nAC\r\n"]


@pytest.mark.parametrize("last", [True, False])
def test_the_vectorised_model_is_the_bytewise_one(last):
    texts = list(HAND) + [mc.sweep_text(s) for s in (0, 1, 15, 16, 500, 1023, 1039)] + [mc.build("long_record_in_pieces")["text"]]
    texts.append(mc.build("n_runs")["text"][:40_000])
    for t in texts:
        for cut in {len(t), len(t) // 2, len(t) - 1}:
            assert mc.unwrap_model(t[:cut], last) == mc.unwrap_model_bytewise(t[:cut], last), (t[:40], cut)


def test_the_rule_on_hand_written_lines():
    """The rule spelled out: terminators of sequence lines go unless a header (or nothing) follows; blank lines go; headers stay."""
    assert mc.unwrap_model(b">a\nAC\nGT\n>b\nA\n", True) == (b">a\nACGT\n>b\nA\n", 14)
    assert mc.unwrap_model(b">a\nAC\nGT\n>b\nA\n", False) == (b">a\nACGT\n", 9)
    assert mc.unwrap_model(b">a\r\nAC\r\nGT\r\n>b\r\nA\r\n", True)[0] == b">a\r\nACGT\r\n>b\r\nA\r\n"
    assert mc.unwrap_model(b">a\nAC\n\nGT\n\n>b\n\n>c\nA\n\n", True)[0] == b">a\nACGT\n>b\n\n>c\nA\n"        # blank lines are dropped ...
    bases, offsets = mc.reads_of(b">a\nACGT\n>b\n\n>c\nA\n")
    assert bases.tobytes() == b"ACGTA" and offsets.tolist() == [0, 4, 4, 5]                              # ... b is a read of length 0
    assert mc.unwrap_model(b">only\nAC\n", False) == (b"", 0)             # a header at byte 0 is no cut
    assert mc.unwrap_model(b">a\nAC\n>b", False) == (b">a\nAC\n", 6)      # an unfinished header line is one


def test_where_the_model_and_the_host_parser_differ():
    """The host parser is lenient where the device reports an error; the model hands the bytes through and reads_of refuses."""
    # a header directly followed by a header: the host parser makes the first an empty read
    assert _host(b">a\n>b\nACGT\n")[1].tolist() == [0, 0, 4]
    assert mc.unwrap_model(b">a\n>b\nACGT\n", True)[0] == b">a\n>b\nACGT\n"
    for bad in (b">a\n>b\nACGT\n", b">a\n>b\n", b">a\nAC\n>b\n", b">a\n>b\nAC\n>c\n>d\nAC\n"):
        with pytest.raises(ValueError):
            mc.reads_of(mc.unwrap_model(bad, True)[0])
    # a final line without newline: the host parser adds one (as the chunkers do at the end of a file); the model adds nothing
    assert _host(b">a\nAC\nGT")[0].tobytes() == b"ACGT"
    assert mc.unwrap_model(b">a\nAC\nGT", True)[0] == b">a\nACGT"
    with pytest.raises(ValueError):
        mc.reads_of(b">a\nACGT")
    # bytes before the first '>': both refuse, the model only in reads_of
    with pytest.raises(ValueError):
        reads_io.parse_fasta_block(_u8(b"AC\n>a\nAC\n"))
    with pytest.raises(ValueError):
        mc.reads_of(mc.unwrap_model(b"AC\n>a\nAC\n", True)[0])
    # a lone '\r' inside a sequence line is no terminator: both keep it as a (bad) base
    assert _host(b">a\nAC\rGT\n")[0].tobytes() == b"AC\rGT"
    assert mc.reads_of(mc.unwrap_model(b">a\nAC\rGT\n", True)[0])[0].tobytes() == b"AC\rGT"


@pytest.mark.parametrize("name", ["shift_sweep", "long_record_in_pieces", "n_runs", "pieces"])
def test_model_and_host_parser_agree_at_every_line_end(name):
    """The file cut at every line end, as a chunk that ends the file and as one that does not.  The two small files: every
    prefix.  The two of hundreds of KiB: the whole file, and at every line end the chunk that starts three records before it
    (a chunk starts on a record; whole records further back change nothing at the cut and would make this minutes)."""
    raw = mc.build(name)["raw"]
    ends = _line_ends(raw)
    assert ends[-1] == raw.shape[0]
    _agrees_with_host_parser(raw, (name, "whole"))
    heads = mc.header_starts(raw)
    whole_prefixes = raw.shape[0] < 32 * 1024
    for e in ends[1:]:
        h = 0 if whole_prefixes else int(heads[max(np.searchsorted(heads, e, side="left") - 3, 0)])
        if np.count_nonzero(raw[h:e] == mc.NL) > 1:
            _agrees_with_host_parser(raw[h:e], (name, h, int(e)))


def test_model_and_host_parser_agree_on_the_round_seam_file():
    """The 2.5 MiB file: the whole of it at every shift's own text for three shifts, and the prefixes at the line ends around
    its seams plus every 400th line end (every prefix of 37 000 would take an hour)."""
    for d in (-17, 0, 17):
        _agrees_with_host_parser(_u8(mc.seam_text(d)), ("round_seam", d))
    raw = mc.build("round_seam")["raw"]
    ends = _line_ends(raw)
    lay = mc.seam_layout(0)
    near = [int(i) for p in (ROUND, lay["nl_before"], lay["long_nl"], lay["last_header"], raw.shape[0])
            for i in range(np.searchsorted(ends, p) - 2, np.searchsorted(ends, p) + 3) if 1 <= i < ends.shape[0]]
    for i in sorted(set(near) | set(range(1, ends.shape[0], 400))):
        _agrees_with_host_parser(raw[:ends[i]], ("round_seam", int(ends[i])))


# ---------------------------------------------------------------------------------------------- shift_sweep
def test_shift_sweep_body():
    first_seq, body = mc._sweep_parts()
    assert 5 * 1024 < len(body) < 8 * 1024
    bases, offsets = mc.reads_of(mc.unwrap_model(body, True)[0])
    lens = np.diff(offsets).tolist()
    assert lens == [100, 200, 200, 0, 200, 600, 3000, 1500]               # eight records; ">h\n\n" is a read of length 0
    assert b">h\n\n>" in body
    # the widths, read from the bytes: the longest run without a terminator inside each record
    recs = body.split(b">")[1:]
    widths = [max(len(ln.rstrip(b"\r")) for ln in r.split(b"\n")[1:]) for r in recs]
    assert widths == [1, 15, 16, 0, 17, 60, 3000, 1023]
    assert 3000 > 2 * TILE
    crlf = [b"\r\n" in r for r in recs]
    assert sum(crlf) == 4                                                 # half the records
    assert b"\r\n\r\n" in recs[5] and not recs[5].endswith(b"\r\n\r\n")    # a blank line inside a record ...
    assert recs[4].endswith(b"\n\n")                                      # ... and one between two records
    assert set(bases.tolist()) <= set(b"ACGT")


def test_shift_sweep_reads_are_the_same_at_every_shift_and_every_residue_is_visited():
    want = mc.reads_of(mc.unwrap_model(mc.sweep_text(0), True)[0])
    assert want[1].shape[0] - 1 == 9
    starts = set()
    for s in mc.SWEEP_SHIFTS:
        text = mc.sweep_text(s)
        assert text.startswith(b">" + b"x" * s + b"\n") and (s == 0 or text[:s + 1].count(b"x") == s)
        two, used = mc.unwrap_model(text, True)
        assert used == len(text) and _same_reads(mc.reads_of(two), want), s
        body_start = text.index(b">w1\r\n")
        assert body_start == s + 2 + 42
        starts.add(body_start % TILE)
        # without the flag: everything but the last record
        two, used = mc.unwrap_model(text, False)
        assert text[used:].startswith(b">w1023\n")
        r = mc.reads_of(two)
        assert r[1].shape[0] - 1 == 8 and np.array_equal(r[1], want[1][:-1])
    assert starts == set(range(TILE))      # the body starts at every byte of a tile: each of its bytes visits every position


def test_shift_sweep_puts_every_seam_condition_somewhere():
    where = mc.sweep_named_shifts()
    assert set(where) == set(mc.SWEEP_CONDITIONS)
    for cond, s in where.items():
        assert cond in mc.sweep_conditions(s), (cond, s)
    # two of them once more by hand, from the bytes
    s = where["cr_last_of_tile"]
    raw = _u8(mc.sweep_text(s))
    assert any(raw[p] == mc.CR and raw[p + 1] == mc.NL for p in range(TILE - 1, raw.shape[0] - 1, TILE))
    s = where["last_header_at_0"]
    text = mc.sweep_text(s)
    p = text.rindex(b"\n>") + 1
    assert p % TILE == 0 and mc.cut_model(text, False) == p


# ---------------------------------------------------------------------------------------------- round_seam
def test_round_seam_layout():
    raw = mc.build("round_seam")["raw"]
    n_tiles = (raw.shape[0] + TILE - 1) // TILE
    assert 2048 < n_tiles <= 3072 and 2.3 * ROUND < raw.shape[0] < 2.7 * ROUND        # three rounds, three super-tiles
    long_nls, last_headers = set(), set()
    for d in mc.SEAM_SHIFTS:
        raw = _u8(mc.seam_text(d))
        lay = mc.seam_layout(d)
        a, b, h = lay["nl_before"], lay["long_nl"], lay["last_header"]
        assert raw[0] == mc.GT and raw[a] == mc.NL and raw[b] == mc.NL and not np.any(raw[a + 1:b] == mc.NL)
        assert b - a - 1 > 1.1 * ROUND                                    # one sequence line of 1.2 MiB ...
        assert a < ROUND <= b                                             # ... from round 0 into round 1 or 2
        assert raw[a + 1] != mc.GT and raw[a - 5:a].tobytes() == b">long"  # (a sequence line: its terminator must go)
        assert raw[b + 1] != mc.GT and raw[b + 9] == mc.NL and h == b + 10 and raw[h] == mc.GT        # a further line of 8 bases
        # nothing between the start of the terminator's round and the terminator tells k_ml_scan where the line began:
        # without the carry its tile inherits -1, the line "starts" at raw[0] == '>', and the terminator is kept
        assert not np.any(raw[(b // ROUND) * ROUND:b] == mc.NL)
        assert mc.cut_model(raw, False) == h                              # the last header of the file
        assert not mc.keep_mask(raw)[b]
        long_nls.add(b - 2 * ROUND)
        last_headers.add(h - 2 * ROUND)
    assert {-1, 0} <= long_nls and {-1, 0, 1} <= last_headers             # both cross the 2 MiB seam byte by byte
    assert min(long_nls) < -8 and max(long_nls) > 2 and min(last_headers) < -8 and max(last_headers) > 8


# ---------------------------------------------------------------------------------------------- n_runs
def test_n_runs_begin_and_end_at_every_column(oracle):
    from tests.ambiguous_cases import split_at_breaks
    from kmer_mapper_amd.util import ambiguous_skip_lut
    case = mc.build("n_runs")
    text = case["text"]
    assert all(len(ln.rstrip(b"\r")) <= mc.N_RUN_WIDTH for ln in text.split(b"\n") if not ln.startswith(b">"))
    bases, offsets = mc.reads_of(mc.unwrap_model(case["raw"], True)[0])
    seen = {}
    for i in range(offsets.shape[0] - 1):
        r = bases[offsets[i]:offsets[i + 1]]
        at = np.flatnonzero(r == ord("N"))
        assert at.shape[0] and np.array_equal(at, np.arange(at[0], at[0] + at.shape[0]))       # one run
        seen.setdefault(int(at.shape[0]), []).append((int(at[0]) % mc.N_RUN_WIDTH, int(at[-1] + 1) % mc.N_RUN_WIDTH))
    assert sorted(seen) == sorted(mc.N_RUN_LENGTHS)
    for run, cols in seen.items():
        assert {c[0] for c in cols} == set(range(mc.N_RUN_WIDTH)) and {c[1] for c in cols} == set(range(mc.N_RUN_WIDTH)), run
    # the two tables count differently: N as A finds poly-A (node 5000) in the long runs, N as a break finds nothing there
    index = mc.index()
    mx = index.max_node_id()
    as_a, n_a = oracle.map_reads(index, mx, bases, offsets, mc.K)
    sb, so = split_at_breaks(bases, offsets, ambiguous_skip_lut())
    skipped, n_s = oracle.map_reads(index, mx, sb, so, mc.K)
    assert as_a[5000] > 0 and skipped[5000] == 0 and n_s < n_a and not np.array_equal(as_a, skipped)


# ---------------------------------------------------------------------------------------------- pieces
def test_pieces_file_and_the_piecewise_cut():
    raw = mc.build("pieces")["raw"]
    text = mc.build("pieces")["text"]
    assert 300 * 1024 <= raw.shape[0] < 304 * 1024
    heads = mc.header_starts(raw)
    sizes = np.diff(np.concatenate([heads, [raw.shape[0]]]))
    assert sizes.max() < 4096                      # no record is longer than the smallest piece
    bases, offsets = mc.reads_of(mc.unwrap_model(raw, True)[0])
    lens = np.diff(offsets)
    assert lens.min() >= 50 and lens.max() <= 3000 and lens.max() > 2900
    assert text.count(b"\r\n") > 500 and text.count(b"\n") - text.count(b"\r\n") > 500
    for kb in mc.PIECE_KBS:
        for last in (True, False):
            assert mc.pieces_model(raw, last, kb << 10) == ("ok", mc.cut_model(raw, last)), (kb, last)
    assert raw.shape[0] // (4 << 10) >= 70          # tens of pieces: the stages rotate many times
    # the caller's loop of the GPU test: chunks of 10 000 bytes, raw[consumed:] carried forward
    pos, fed, n = 0, 0, 0
    while pos < raw.shape[0]:
        fed = min(raw.shape[0], max(fed, pos) + 10_000)
        two, used = mc.unwrap_model(raw[pos:fed], fed == raw.shape[0])
        assert used > 0
        n += mc.reads_of(two)[1].shape[0] - 1
        pos += used
    assert n == offsets.shape[0] - 1


def test_long_record_exceeds_a_piece():
    case = mc.build("long_record_in_pieces")
    raw, text = case["raw"], case["text"]
    heads = mc.header_starts(raw)
    assert heads.shape[0] == 3 and heads[2] - heads[1] == 10 * 1024 and heads[1] < 4096
    piece = mc.LONG_PIECE_KB << 10
    for last in (True, False):
        assert mc.pieces_model(raw, last, piece) == ("record exceeds a piece", int(heads[1]))
        assert mc.pieces_model(raw, last, 16 << 10) == ("ok", mc.cut_model(raw, last))
    assert mc.reads_of(mc.unwrap_model(raw, True)[0])[1].shape[0] - 1 == 3
