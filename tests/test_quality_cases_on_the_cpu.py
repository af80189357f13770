"""CPU tier of "min_base_quality": the cases of tests/quality_cases.py are held to the conditions they exist for, so that
tests/test_gpu_quality.py cannot pass vacuously — the oracle on the reads split at their masked bases equals a brute-force
count of the windows without one, differs from the counts on the unsplit reads and at the neighbouring floors, and the
bytes the cases name lie where they say.  The positional identity the device code rests on is checked on
every text, and the host logic of the command line (route, argument checks) without a device."""
import numpy as np
import pytest

from tests import quality_cases as qc
from kmer_mapper_amd import synthetic
from kmer_mapper_amd.util import ambiguous_skip_lut


@pytest.fixture(scope="module", params=qc.CASES)
def case(request, oracle):
    c = dict(qc.build(request.param))
    c["index"] = qc.index_for(c["k"])
    c["mx"] = c["index"].max_node_id()
    c["dead"] = qc.dead_mask(c)
    c["sb"], c["so"] = qc.split_at_mask(c["bases"], c["offsets"], c["dead"])
    c["split"], c["n_windows"] = oracle.map_reads(c["index"], c["mx"], c["sb"], c["so"], c["k"])
    return c


def _counts_at(case, oracle, q, with_lut=None):
    sb, so = qc.split_at_mask(case["bases"], case["offsets"], qc.dead_mask(case, q, with_lut))
    return oracle.map_reads(case["index"], case["mx"], sb, so, case["k"])


def test_split_reads_equal_the_brute_force_count_of_windows_without_a_masked_base(case, oracle):
    win = qc.surviving_windows(case["offsets"], case["k"], case["dead"])
    assert win.shape[0] == case["n_windows"]
    codes = (ambiguous_skip_lut()[case["bases"]] & 3).astype(np.uint8)
    kmers = synthetic.pack_kmers_at(codes, win, case["k"])
    assert np.array_equal(oracle.map_kmers(case["index"], case["mx"], kmers), case["split"])
    # no base but the masked ones is lost, and none is reordered
    assert np.array_equal(case["sb"], case["bases"][~case["dead"]])
    assert case["so"][0] == 0 and case["so"][-1] == case["sb"].shape[0]


def test_every_case_tells_the_floor_from_none_and_from_its_neighbours(case, oracle):
    q = case["q"]
    unsplit, n_all = _counts_at(case, oracle, 0, with_lut=False) if not case["use_lut"] else _counts_at(case, oracle, 0)
    assert not np.array_equal(unsplit, case["split"])
    assert 0 < case["n_windows"] < n_all and case["split"].sum() > 0
    for other in (q - 1, q + 1):
        if 0 <= other <= 93:
            counts, n = _counts_at(case, oracle, other)
            assert not np.array_equal(counts, case["split"]), (case["name"], other)
            assert (n > case["n_windows"]) if other < q else (n < case["n_windows"])
    if case["use_lut"]:                  # both rules kill: each alone leaves more
        for counts, n in (_counts_at(case, oracle, 0), _counts_at(case, oracle, q, with_lut=False)):
            assert n > case["n_windows"] and not np.array_equal(counts, case["split"])
    assert qc.is_uniform(case["offsets"]) == (case["name"] in qc.UNIFORM)
    assert 0 < qc.low_mask(case["quals"], q).sum() < case["quals"].shape[0]


def _line_phase(text):
    """Per byte: (newlines before it) mod 4, and whether it is a line terminator ('\\n', '\\r')."""
    raw = np.frombuffer(text, np.uint8)
    nl = raw == 10
    before = np.cumsum(nl) - nl
    return raw, before & 3, nl | (raw == 13)


def test_positional_identity_the_jth_quality_byte_is_the_jth_base(case):
    """What the quality variant of k_rec_scatter rests on: in every text the rank of a quality byte among the quality bytes
    equals the rank of its base among the sequence bytes, and at every newline that ends a quality line both counts agree."""
    text, where, layout = qc.case_text(case)
    raw, phase, term = _line_phase(text)
    seq_at, qual_at = np.flatnonzero((phase == 1) & ~term), np.flatnonzero((phase == 3) & ~term)
    assert np.array_equal(raw[seq_at], case["bases"]) and np.array_equal(raw[qual_at], case["quals"])
    n_seq, n_qual = np.cumsum((phase == 1) & ~term), np.cumsum((phase == 3) & ~term)
    ends = np.flatnonzero((raw == 10) & (phase == 3))
    assert ends.shape[0] == len(case["offsets"]) - 1 and np.array_equal(n_seq[ends], n_qual[ends])
    assert np.array_equal(n_seq[ends], case["offsets"][1:])
    for i, (rec, seq0, qual0, qual_nl) in enumerate(layout):
        assert text[rec:rec + 1] == b"@" and text[qual_nl:qual_nl + 1] == b"\n"
        n = int(case["offsets"][i + 1] - case["offsets"][i])
        assert text[seq0:seq0 + n] == case["bases"][case["offsets"][i]:case["offsets"][i + 1]].tobytes()
        assert text[qual0:qual0 + n] == case["quals"][case["offsets"][i]:case["offsets"][i + 1]].tobytes()
    assert any(text[rec[3] - 1:rec[3]] == b"\r" for rec in layout[2::5])       # every fifth record: "\r\n"


def _low_at(case, p):
    return bool(qc.low_mask(case["quals"], case["q"])[p])


def test_the_low_bytes_stand_where_the_cases_say():
    c = qc.build("tile_edges")
    total, k = c["bases"].shape[0], c["k"]
    for p in qc.FLAT_EDGES + (total - 1, total - k):
        assert _low_at(c, p)
    text, where, layout = qc.case_text(c)
    last, first = where[(130, "qual", 40)], where[(260, "qual", 75)]
    assert last % qc.TILE == qc.TILE - 1 and first % qc.TILE == 0
    assert text[last] < 33 + c["q"] and text[first] < 33 + c["q"]
    assert text[last] == c["quals"][130 * qc.L + 40] and text[first] == c["quals"][260 * qc.L + 75]
    # pieces of PIECE_KB: at least three, and the second starts on a record whose first base is low
    piece = qc.PIECE_KB << 10
    assert len(text) > 3 * piece
    r = qc.second_piece_record(layout, piece)
    assert layout[r][0] <= piece < layout[r][3] + 1 and r > 0 and _low_at(c, r * qc.L)

    c = qc.build("line_boundaries")
    text, where, layout = qc.case_text(c)
    for r in (30, 100):
        at = where[(r, "seq_nl", 0)]
        assert at % qc.TILE == qc.TILE - 1 and text[at:at + 1] == b"\n"
        assert layout[r][2] // qc.TILE == at // qc.TILE + 1 and layout[r][1] // qc.TILE <= at // qc.TILE   # quality line: the next tile
        assert _low_at(c, r * qc.L)
    at = where[(70, "qual", 70)]
    assert at % qc.TILE == 0 and layout[70][2] < at < layout[70][3]               # the quality line straddles the edge
    assert _low_at(c, 70 * qc.L + 69) and _low_at(c, 70 * qc.L + 70)
    assert text[layout[100][3] - 1:layout[100][3]] == b"\r"

    c = qc.build("read_ends")
    low = qc.low_mask(c["quals"], c["q"])
    assert low[200 * qc.L] and low[201 * qc.L - 1] and low[3 * qc.L] and low[8 * qc.L - 1] and low[300 * qc.L - 1] and low[0]

    c = qc.build("run_of_40")
    low = qc.low_mask(c["quals"], c["q"])
    assert low[10 * qc.L + 50:10 * qc.L + 90].all() and low[4080:4120].all() and low[151 * qc.L - 40:151 * qc.L].all()

    for name in ("pairs_k_apart", "pairs_k_apart-k12", "pairs_k_apart-k2"):
        c = qc.build(name)
        k = c["k"]
        low = qc.low_mask(c["quals"], c["q"])
        win = qc.surviving_windows(c["offsets"], k, low)
        for read in (4, 30, 100):
            assert low[read * qc.L + 40] and low[read * qc.L + 41 + k]
            assert read * qc.L + 41 in win and read * qc.L + 40 not in win and read * qc.L + 42 not in win   # exactly one
        for read in (9, 27, 150):
            assert not ((win > read * qc.L + 60 - k) & (win <= read * qc.L + 60 + k)).any()                   # none

    c = qc.build("degenerate_reads")
    lens = np.diff(c["offsets"])
    low = qc.low_mask(c["quals"], c["q"])
    assert low[c["offsets"][5]:c["offsets"][6]].all()
    assert {0, 1, c["k"] - 1, c["k"]} <= set(lens.tolist()) and lens[-1] == 0
    text, _, layout = qc.case_text(c)
    assert text[layout[40][1]:layout[40][1] + 2] == b"\r\n" and text.endswith(b"@r199\n\n+\n\n")            # two empty lines

    c = qc.build("ragged_1_to_400")
    low = qc.low_mask(c["quals"], c["q"])
    assert 0.04 < low.mean() < 0.06 and set(np.diff(c["offsets"]).tolist()) >= {1, 400}
    assert all(low[p] for p in qc.FLAT_EDGES)

    c = qc.build("long_read")
    text, where, layout = qc.case_text(c)
    rec, seq0, qual0, qual_nl = layout[10]
    assert qual_nl - qual0 == 10_000 and seq0 % qc.TILE == 100
    assert qual_nl // qc.TILE - qual0 // qc.TILE == 2 and qual0 // qc.TILE - seq0 // qc.TILE == 2       # spans three tiles, two behind
    edges = list(range((qual0 // qc.TILE + 1) * qc.TILE, qual_nl, qc.TILE))
    assert len(edges) == 2
    for e in edges:
        assert text[e - 1] < 33 + c["q"] and text[e] < 33 + c["q"]
    assert text[qual0] < 33 + c["q"] and text[qual_nl - 1] < 33 + c["q"]

    c = qc.build("decoy_characters")
    text, _, layout = qc.case_text(c)
    assert text[layout[5][2]:layout[5][2] + 1] == b"@" and text[layout[6][2]:layout[6][2] + 1] == b"+"
    assert text[layout[40][2]:layout[40][3] - 1] == b"@" * qc.L and text[layout[40][3] - 1:layout[40][3]] == b"\r"
    assert text[layout[41][2]:layout[41][2] + 2] == b"@r" and text[layout[43][2] - 2:layout[43][2] + 4] == b"+\n+++" + bytes([text[layout[43][2] + 3]])
    low = qc.low_mask(c["quals"], c["q"])
    assert low[6 * qc.L] and not low[5 * qc.L] and not low[40 * qc.L:41 * qc.L].any()                      # '+' is Q10, '@' Q31

    c = qc.build("q1")
    assert set(c["quals"][qc.low_mask(c["quals"], 1)].tolist()) == {33} and (c["quals"] == 34).any()
    c = qc.build("q93")
    low = qc.low_mask(c["quals"], 93)
    assert set(c["quals"][~low].tolist()) == {126} and 0.9 < low.mean() < 1
    c = qc.build("all_41_values")
    assert set(c["quals"].tolist()) == set(range(33, 74))

    c = qc.build("with_skip_table")
    low, brk = qc.low_mask(c["quals"], c["q"]), qc.break_mask(c["bases"], ambiguous_skip_lut())
    assert brk[10 * qc.L + 50] and not low[10 * qc.L + 50]                        # an N under a high quality
    assert brk[20 * qc.L + 60] and low[20 * qc.L + 60]                            # ... under a low one
    assert brk[30 * qc.L + 70] and low[30 * qc.L + 71] and not brk[30 * qc.L + 71]   # a low base next to an N
    assert (c["bases"][8 * qc.L:9 * qc.L] & 0x20).all() and low[8 * qc.L + 34] and brk[8 * qc.L + 33]


@pytest.mark.parametrize("q", [1, 20, 93])
def test_choose_route_never_hands_a_quality_floor_to_the_host_packer(q):
    import itertools
    from kmer_mapper_amd.command_line_interface import choose_route
    from kmer_mapper_amd.reads_io import probe_input  # noqa: F401 (the probe's fields are what choose_route reads)
    import types
    seen = set()
    for fmt, container, world, threads, has_device, lut in itertools.product(
            ("fastq", "fasta", "fasta_ml"), (None, "bgzf", "gzip"), (1, 2), (1, 16), (False, True), (None, ambiguous_skip_lut())):
        probe = types.SimpleNamespace(inflate=container is not None, container=container, fmt=fmt, two_line=True)
        for env in ({}, {"KMM_CLI_GPU_GUNZIP": "1"}, {"KMM_CLI_NO_PREFETCH": "1"}):
            route, populate, steer = choose_route(fmt, probe, world, threads, has_device, env=env, lut=lut, min_base_quality=q)
            assert route != "mmap" and not populate and not steer
            seen.add(route)
            if lut is None:              # the floor off: the routes of today, "mmap" among them
                off = choose_route(fmt, probe, world, threads, has_device, env=env)
                assert off == choose_route(fmt, probe, world, threads, has_device, env=env, min_base_quality=0)
                assert (route, populate, steer) == (("raw", False, False) if off[0] == "mmap" else off)
    assert seen == {"raw", "prefetch", "bgzf", "gzip"}
    plain = types.SimpleNamespace(inflate=False, container=None, fmt="fastq", two_line=True)
    assert choose_route("fastq", plain, 1, 16, True, env={})[0] == "mmap"


def test_the_argument_parser_takes_the_flag_and_refuses_what_it_cannot_mean(capsys):
    from kmer_mapper_amd import command_line_interface as cli
    base = ["map", "-i", "no_such_index.npz", "-f", "no_such_reads.fq", "-o", "out"]
    args = cli.build_argument_parser().parse_args(base)
    assert args.min_base_quality == 0
    args = cli.build_argument_parser().parse_args(base + ["--min-base-quality", "20"])
    assert args.min_base_quality == 20
    for extra, word in ((["--min-base-quality", "94"], "0 .. 93"), (["--min-base-quality", "-1"], "0 .. 93"),
                        (["--min-base-quality", "20", "-k", "1"], "-k 2"), (["--min-base-quality", "x"], "invalid int")):
        with pytest.raises(SystemExit) as exc:      # (before the index file, which does not exist, is opened)
            cli.run_argument_parser(base + extra)
        assert exc.value.code == 2 and word in capsys.readouterr().err, extra
    # the checks behind the parser, without a device
    assert cli.check_min_base_quality(0, 1, "sam") == 0 and cli.check_min_base_quality(20, 31, "fastq") == 20
    assert cli.check_min_base_quality(20, 31, "fasta") == 0 and cli.check_min_base_quality(20, 31, "fasta_ml") == 0
    for fmt, host_parser, word in (("sam", False, "SAM"), ("bam", False, "BAM"), ("fastq", True, "--host-parser")):
        with pytest.raises(ValueError, match=word):
            cli.check_min_base_quality(20, 31, fmt, host_parser)
    with pytest.raises(ValueError, match="-k 2"):
        cli.check_min_base_quality(20, 1, "fastq")
