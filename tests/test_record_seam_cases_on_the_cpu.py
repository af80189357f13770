"""tests/record_seam_cases.py held to its conditions, without a GPU: every (feature, seam, delta) of the table below has a case,
every placed byte lies where the builder says and its seam is what its name says, the line model agrees with a second, naive
formulation on every case, well-formed cases are accepted and damaged ones refused for the stated reason at the stated byte."""
import os
import re

import numpy as np
import pytest

from tests import record_seam_cases as rc

# ---------------------------------------------------------------------------------------------- the coverage table
# Written out here, not derived from the builder's lists: a case that is dropped there fails here.
IN_BOTH_FORMATS = ("nl_header", "nl_seq", "crlf", "lone_cr", "first_header", "break", "empty_seq", "long_seq", "long_header")
IN_FASTQ_ONLY = ("nl_plus", "nl_qual", "first_plus", "low_qual", "low_run", "qual_at", "qual_plus")
DAMAGED_IN_BOTH = ("bad_header", "bad_base")
DAMAGED_IN_FASTQ_ONLY = ("bad_plus", "qual_short", "qual_long")
SMALL_SEAMS = ("vector", "lane", "wave", "tile")
DELTAS = (-2, -1, 0, 1)
BIG_SEAMS = ("reload", "super")
END_SEAMS = ("limit_tile", "limit_lane", "badtail_tile", "badtail_lane", "end_tile", "end_lane", "piece")


def _table():
    t = set()
    for fmt in ("fastq", "fasta2"):
        features = IN_BOTH_FORMATS + DAMAGED_IN_BOTH + ((IN_FASTQ_ONLY + DAMAGED_IN_FASTQ_ONLY) if fmt == "fastq" else ())
        t |= {(fmt, f, s, d) for f in features for s in SMALL_SEAMS + BIG_SEAMS for d in DELTAS}
        t |= {(fmt, "record_end", s, d) for s in END_SEAMS for d in DELTAS}
        t |= {(fmt, "flat_side", "flat_dst0", v) for v in range(16)}
    return t


UNIFORM_CASES = {"one_length": True, "one_length_lone_cr": False, "alternating": False, "length_15": False, "two_pieces": False}


def test_every_feature_seam_and_delta_of_the_table_has_a_case():
    have = set()
    for name in rc.CASES:
        c = rc.build(name)
        have |= {(rc.FMT_NAME[c["fmt"]], c["feature"], p["seam"], p["delta"]) for p in c["placements"]}
    want = _table()
    assert have == want, (sorted(want - have)[:10], sorted(have - want)[:10])
    # 16 + 9 features and 5 + 2 kinds of damage at six seams and four deltas; seven record-end seams; 16 values of dst0 & 15
    assert len(want) == (16 + 9 + 5 + 2) * 6 * 4 + 2 * 7 * 4 + 2 * 16
    assert {n for n in rc.CASES if n.startswith("uniform_")} == {"uniform_%s/%s" % (k, f) for k in UNIFORM_CASES for f in ("fastq", "fasta2")}


def test_the_geometry_constants_are_the_kernels():
    """The constants are stated once in the case file with the functions they are read from; here: those functions exist and
    the tile is what the kernel file calls REC_TB.  (What the constants mean for the results, the GPU tier shows.)"""
    src = open(os.path.join(os.path.dirname(__file__), "..", "kmer_mapper_amd", "csrc", "kmm_records.hpp")).read()
    assert re.search(r"\bREC_TB\s*=\s*%d\b" % rc.TILE, src)
    for name in ("rec_load16", "rec_load64", "k_rec_count2", "k_rec_scatter", "k_rec_uniform"):
        assert re.search(r"\b%s\b" % name, src), name
    assert rc.VEC * 4 == rc.LANE and rc.LANE * 64 == rc.TILE


# ---------------------------------------------------------------------------------------------- the placements
EXPECT_BYTE = {"nl_header": b"\n", "nl_seq": b"\n", "nl_plus": b"\n", "nl_qual": b"\n", "crlf": b"\n", "lone_cr": b"\r", "first_plus": b"+",
               "break": b"N", "low_qual": bytes([rc.JUST_LOW]), "low_run": bytes([rc.JUST_LOW]), "empty_seq": b"\n", "long_seq": b"\n",
               "long_header": b"\r", "qual_at": b"@", "qual_plus": b"+", "record_end": b"\n", "bad_header": b"x", "bad_plus": b"-",
               "bad_base": b"X", "qual_short": b"\n", "qual_long": b"\n", "flat_side": b"x"}

GROUPS = rc.GROUPS


def _group(g):
    return [n for n in rc.CASES if rc.group_of(n) == g]


@pytest.mark.parametrize("group", GROUPS)
def test_the_placed_byte_is_where_the_builder_says(group):
    for name in _group(group):
        c = rc.build(name)
        raw, fmt = c["raw"].tobytes(), c["fmt"]
        m = rc.summary_of(c, _variants(c)[0])                     # (consumed is the same in every variant of a well-formed file)
        assert c["placements"] or c["feature"] == "uniform", name
        for p in c["placements"]:
            what = (name, p["seam"], p["delta"])
            if c["feature"] == "flat_side":
                assert p["pos"] == p["seam_pos"] and raw[p["pos"]:p["pos"] + 1] == b"x", what
            else:
                assert p["pos"] == p["seam_pos"] + p["delta"], what
                want = (b"@" if fmt == rc.FASTQ else b">") if c["feature"] == "first_header" else EXPECT_BYTE[c["feature"]]
                assert raw[p["pos"]:p["pos"] + 1] == want, what
            assert rc.seam_ok(c, p, m["consumed"]), what
            # what surrounds the byte
            pos, f = p["pos"], c["feature"]
            if f == "crlf":
                assert raw[pos - 1] == rc.CR, what
            if f == "lone_cr":
                assert raw[pos + 1] != rc.NL and raw[pos - 1] in b"ACGT" and raw[pos + 1] in b"ACGT", what
            if f in ("first_header", "first_plus", "qual_at", "qual_plus", "bad_header", "bad_plus"):
                assert raw[pos - 1] == rc.NL, what
            if f == "empty_seq":
                assert raw[pos - 1] == rc.NL, what
            if f == "long_seq":
                assert rc.NL not in raw[pos - 9000:pos] and 9000 > 2 * rc.TILE, what
            if f == "long_header":
                assert raw[pos - 1:pos + 5] == b"x\r@+>x" and rc.NL not in raw[pos - 2501:pos + 2505], what
            if f == "low_run":
                run = raw[pos - 35:pos + 35]
                assert max(run) < 33 + rc.Q and raw[pos - 36] >= 33 + rc.Q and raw[pos + 35] >= 33 + rc.Q and len(run) > rc.LANE, what
            if f in ("break", "low_qual"):
                assert rc.NL not in raw[pos - 29:pos + 29], what
        if len(c["placements"]) > 1:
            assert all(a["pos"] < b["pos"] for a, b in zip(c["placements"], c["placements"][1:])), name


def test_the_wave_ranges_of_the_big_cases():
    """Reload: the 64th tile of every wavefront's range; super-tile: tile 1024 inside the last wavefront's range."""
    c = rc.build("reload/nl_seq/fastq")
    n_live, per_wave = rc.wave_ranges(rc.model_of(c)["consumed"], 1)
    assert (n_live, per_wave) == (280, 70) and per_wave > rc.RELOAD
    assert [p["seam_pos"] // rc.TILE for p in c["placements"]] == [64, 134, 204, 274]
    c = rc.build("super/nl_seq/fastq/-1")
    n_live, per_wave = rc.wave_ranges(rc.model_of(c)["consumed"], 1)
    assert (n_live, per_wave) == (1040, 260) and 3 * per_wave < rc.SUPER < n_live and (rc.SUPER - 3 * per_wave) % rc.RELOAD
    # the small composite files: two tiles per wavefront with the hook at 2, four with it at 1: the in-register carries
    c = rc.build("nl_seq/fastq")
    assert rc.wave_ranges(rc.model_of(c)["consumed"], 2) == (16, 2) and rc.wave_ranges(rc.model_of(c)["consumed"], 1) == (16, 4)
    assert len(c["raw"]) <= 64 << 10


@pytest.mark.parametrize("fmt", ["fastq", "fasta2"])
def test_the_pieces_start_unaligned_and_the_limit_leaves_a_tail(fmt):
    starts = []
    for d in DELTAS:
        c = rc.build("piece/%s/%d" % (fmt, d))
        m = rc.model_of(c)
        assert len(m["pieces"]) == 3 and m["consumed"] == len(c["raw"]), d
        # delta -1: the record is the first piece's last byte; delta 0 and 1: it opens the second piece
        assert (m["pieces"][1][0] == c["placements"][0]["pos"] + 1) == (d < 0), d
        starts += m["pieces"][1:]
    assert any(raw0 % 16 and flat % 32 and flat % 16 for raw0, flat in starts), starts
    for seam in ("tile", "lane"):
        for d in DELTAS:
            c = rc.build("limit_%s/%s/%d" % (seam, fmt, d))
            m = rc.model_of(c)
            assert m["consumed"] == c["placements"][0]["pos"] + 1 == len(c["raw"]) - len(rc.TAIL[c["fmt"]]), (seam, d)
            assert m["error"] is None and rc.wave_ranges(m["consumed"], 1)[1] == 3     # (three tiles per wavefront with the hook at 1)
            c = rc.build("badtail_%s/%s/%d" % (seam, fmt, d))
            m, tail = rc.model_of(c), rc.TAIL_BAD[c["fmt"]]
            assert m["consumed"] == c["placements"][0]["pos"] + 1 == len(c["raw"]) - len(tail) and m["error"] is None, (seam, d)
            assert c["any_route"] and 0xFF in rc.table(False)[np.frombuffer(tail.split(b"\n")[1], np.uint8)], (seam, d)
            assert c["fmt"] == rc.FASTA2 or tail.split(b"\n")[2][:1] != b"+", (seam, d)
            c = rc.build("end_%s/%s/%d" % (seam, fmt, d))
            assert rc.model_of(c)["consumed"] == len(c["raw"]) == c["placements"][0]["pos"] + 1, (seam, d)


@pytest.mark.parametrize("fmt", [rc.FASTQ, rc.FASTA2])
def test_the_flat_side(fmt):
    """dst0 & 15 takes each of the 16 values at a tile start; an N and a low quality byte sit at flat positions 31 mod 32; a
    16-byte vector of bases starts at a flat position that is no multiple of 16 (the run crosses a code word); the flat reads
    end with low bases."""
    c = rc.build("flat_side/%s" % rc.FMT_NAME[fmt])
    raw = c["raw"].tobytes()
    a = c["raw"]
    line = np.cumsum(a == rc.NL) - (a == rc.NL)
    base = ((line % fmt) == 1) & (a != rc.NL) & (a != rc.CR)
    before = np.concatenate([[0], np.cumsum(base)])
    assert [int(before[p["pos"]]) & 15 for p in c["placements"]] == list(range(16))
    at31 = [p for p in c["placements"] if p["flat31"] >= 0]
    assert any(p["flat31_is_n"] for p in at31) and not all(p["flat31_is_n"] for p in at31)
    flat_pos = np.flatnonzero(base)
    for p in at31:
        assert p["flat31"] % 32 == 31 and (raw[flat_pos[p["flat31"]]] == ord("N")) == p["flat31_is_n"]
    vec = np.flatnonzero(base[:len(a) // 16 * 16].reshape(-1, 16).all(axis=1))
    assert any(before[v * 16] % 16 for v in vec)
    assert rc.model_of(c)["total"] == int(before[-1]) and int(before[-1]) % 32 == 0
    if fmt == rc.FASTQ:
        assert raw.endswith(bytes([rc.LOW]) * 3 + b"\n")
        assert rc.model_of(c, "qual")["n_masked"] > rc.model_of(c, "plain")["n_masked"] == 0


# ---------------------------------------------------------------------------------------------- the model
def _variants(c):
    if len(c["raw"]) > (600 << 10):                               # the files of 1 MiB and more: the fullest variant
        return (rc.variants_of(c)[-1],)
    if c["error"]:
        return ("plain", "qual") if c["error"][2] else ("plain", "brk")
    return rc.variants_of(c)


_PREFIX_MODEL = {}


def _prefix_model(fmt, v):
    """The model of the records that every super-tile file starts with, which the naive formulation agrees with (once)."""
    if (fmt, v) not in _PREFIX_MODEL:
        brk, q = rc.VARIANTS[v]
        pre = rc.super_prefix(fmt)
        a = rc.model(pre, fmt, brk, q)
        b = rc.model(pre, fmt, brk, q, piece=rc.naive_piece)
        assert a == b and a["consumed"] == len(pre) and a["error"] is None
        _PREFIX_MODEL[fmt, v] = a
    return _PREFIX_MODEL[fmt, v]


@pytest.mark.parametrize("group", GROUPS)
def test_the_model_agrees_with_the_naive_formulation(group):
    """(The super-tile files: the naive formulation runs over the shared first 1012 tiles once, and over the rest of every file;
    the model of the whole file must be the two put together — records do not reach into each other.)"""
    for name in _group(group):
        c = rc.build(name)
        for v in _variants(c):
            brk, q = rc.VARIANTS[v]
            pm = (c["piece_kb"] << 10) or None
            raw, skip = c["raw"].tobytes(), 0
            if name.startswith("super"):
                pre, whole = _prefix_model(c["fmt"], v), rc.model(raw, c["fmt"], brk, q)
                skip = pre["consumed"]
                assert raw[:skip] == rc.super_prefix(c["fmt"]), name
                raw = raw[skip:]
                rest = rc.model(raw, c["fmt"], brk, q)
                for key in ("consumed", "n_records", "total") + (() if whole["error"] else ("n_masked", "reads")):
                    assert whole[key] == pre[key] + rest[key], (name, v, key)
                assert whole["error"] == (rest["error"] and (rest["error"][0], rest["error"][1] + skip, 0)) and not whole["uniform"], (name, v)
            a = rc.model(raw, c["fmt"], brk, q, pm)
            b = rc.model(raw, c["fmt"], brk, q, pm, piece=rc.naive_piece)
            # (behind a quality line of the wrong length the two pair bases and quality bytes differently: the file is refused)
            for key in ("consumed", "n_records", "error", "pieces") if a["error"] else a:
                assert a[key] == b[key], (name, v, key)


@pytest.mark.parametrize("group", GROUPS)
def test_well_formed_cases_are_accepted_and_damaged_ones_refused_for_their_reason(group):
    for name in _group(group):
        c = rc.build(name)
        for v in rc.variants_of(c) if len(c["raw"]) <= rc.BIG else _variants(c):
            m = rc.summary_of(c, v)
            if c["error"] and rc.VARIANTS[v][1] >= c["error"][2]:
                kind, pos, _ = c["error"]
                assert m["error"] == (kind, pos, 0), (name, v)
                twin = rc.build(c["twin"])
                assert rc.summary_of(twin, v)["error"] is None and len(twin["raw"]) == len(c["raw"]), (name, v)
                assert rc.summary_of(twin, v)["consumed"] == m["consumed"], (name, v)
            else:
                assert m["error"] is None, (name, v)
                assert m["n_records"] > 0 and m["consumed"] > 0 and m["n_reads"], (name, v)
            if c["error"] and c["error"][2] and not rc.VARIANTS[v][1]:      # a quality line's length is checked with a floor only
                assert rc.model_of(c, v)["reads"] == rc.model_of(rc.build(c["twin"]), v)["reads"], (name, v)


def test_the_variants_differ_where_a_feature_says_so():
    """An N splits under the break table only, a low quality byte under the floor only, a lone '\\r' always."""
    def n_reads(name, v):
        return len(rc.model_of(rc.build(name), v)["reads"])
    for fmt in ("fastq", "fasta2"):
        quiet = rc.model_of(rc.build("uniform_one_length/" + fmt))
        cr = rc.model_of(rc.build("uniform_one_length_lone_cr/" + fmt))
        assert len(cr["reads"]) == len(quiet["reads"]) + 1 == quiet["n_records"] + 1
        assert b"".join(cr["reads"]) == b"".join(quiet["reads"])          # (the '\\r' is dropped, no base is)
    assert n_reads("break/fastq", "brk") > n_reads("break/fastq", "plain")
    assert n_reads("low_qual/fastq", "qual") > n_reads("low_qual/fastq", "plain")
    assert n_reads("low_qual/fastq", "brk_qual") > max(n_reads("low_qual/fastq", "qual"), n_reads("low_qual/fastq", "brk"))
    assert rc.model_of(rc.build("qual_plus/fastq"), "qual")["n_masked"] >= 16          # ('+' is Q10; '@', Q31, is alive)


@pytest.mark.parametrize("fmt", ["fastq", "fasta2"])
def test_the_uniform_cases(fmt):
    for kind, uniform in UNIFORM_CASES.items():
        c = rc.build("uniform_%s/%s" % (kind, fmt))
        for v in rc.variants_of(c):
            m = rc.model_of(c, v)
            assert m["uniform"] == uniform and m["error"] is None, (kind, v)
        m = rc.model_of(c)
        lengths = {len(r) for r in m["reads"]}
        if kind == "one_length":
            assert lengths == {rc.UNIFORM_L} and rc.UNIFORM_L >= 16
        if kind == "alternating":
            assert lengths == {rc.UNIFORM_L - 1, rc.UNIFORM_L + 1} and m["total"] == m["n_records"] * rc.UNIFORM_L
        if kind == "length_15":
            assert lengths == {15}
        if kind == "two_pieces":
            assert len(m["pieces"]) == 2 and m["pieces"][1][0] == 1024 and lengths == {rc.UNIFORM_L, rc.UNIFORM_L + 4}
            for s, e in ((0, 1024), (1024, len(c["raw"]))):           # each piece by itself has one length
                assert rc.model(c["raw"].tobytes()[s:e], c["fmt"])["uniform"]


# ---------------------------------------------------------------------------------------------- the library's side
def test_the_hook_and_the_lone_cr_rule_are_in_kmm_h():
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "kmm.h")).read()
    assert '"debug_records_grid"' in text
    assert re.search(r"'\\r' inside a sequence line that no '\\n' follows is dropped and breaks the read", text)
