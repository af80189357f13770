"""CPU tier of mates kept together in SAM output (include/kmm.h "record_sam_mates"): the catalogue of
tests/sam_mates_cases.py held to its own conditions — the whole-text model against the window-by-window one under every cutting,
the kinds of seams, decisions, names and cuts it must reach, and how often pairing changes the bytes at all; the source the
kernels share (csrc/kmm_sam.hpp: the spans by entry, the mate check, the pair flags, the pair copy, the waiting line) compiled by
itself with g++ (tests/sam_mates_cpu_driver.hpp) and run with 1 and 64 lanes into queues of exactly the model's size, filled with
0x00 and with 0xFF; the mate check against brute force; the same driver as an executable under ASan + UBSan; the command line's
parsing and refusals up to the first look at the index."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import sam_mates_cases as sm
from tests import sam_records_cases as sr
from tests.test_sam_records_on_the_cpu import tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
U64, I64, U32 = ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32
CASES = sm.all_cases()
IDS = [c.name for c in CASES]
PAIR_RULE = {sm.ANY: 0, sm.BOTH: 1}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam_mates")
    src = tmp / "shim.cpp"
    src.write_text('#include "sam_mates_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.sam_mates_cpu.argtypes = [ctypes.c_char_p, U64, ctypes.c_void_p, ctypes.c_int, U32, ctypes.c_int, ctypes.c_int, U32, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, U32, ctypes.c_void_p, ctypes.c_void_p, U64,
                                  ctypes.c_void_p, ctypes.c_int, U64, ctypes.c_void_p, U64, ctypes.c_void_p]
    lib.sam_mates_names_sweep.argtypes, lib.sam_mates_names_sweep.restype = [U32, U32], U64
    return lib


def _entries(case, text):
    """One entry per selected record of the stream: the model's, an odd last one included"""
    single = sr.model(case, text)
    return np.ascontiguousarray(single.hits), np.ascontiguousarray(single.windows)


def _run(lib, case, text, want_out, cuts=(), lanes=1, fill=0, tail0=0):
    """(rc, kept bytes, stats) of the driver; the queue holds exactly tail0 + len(want_out) bytes."""
    cuts = sorted(set([c for c in cuts if 0 < c < len(text)] + [len(text)]))
    rules, iv, names, offs = tables(case.sel)
    c = (U64 * len(cuts))(*cuts)
    r = (U64 * 4)(*rules)
    ivs = (I64 * (3 * len(iv) + 1))(*[x for t in iv for x in t])
    off = (U32 * len(offs))(*offs)
    hits, windows = _entries(case, sr.with_final_newline(text))
    rule4 = (U32 * 4)(case.min_hits, case.min_permille, int(case.invert), PAIR_RULE[case.pair_rule])
    out = np.zeros(len(want_out) + 1, np.uint8)
    st = (U64 * 9)()
    rc = lib.sam_mates_cpu(text, len(text), c, len(cuts), case.excl, case.mode, int(case.orig), lanes, r, ivs, b"".join(names), off, len(names),
                           hits.ctypes.data, windows.ctypes.data, hits.shape[0], rule4, fill, tail0, out.ctypes.data, len(want_out), st)
    return rc, out[:len(want_out)].tobytes(), list(st)


# ---------------------------------------------------------------------------------------------- the catalogue itself
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_model_against_itself_under_every_cutting(case):
    """The expected bytes, entries and windows are the uncut ones however the text is cut into windows"""
    e = sm.expected(case)
    cut_sets = dict(sm.cut_sets(case), none=[], every_byte_of_the_first_400=list(range(1, 400)), tiles=list(range(1024, len(case.text), 1024)))
    for kind, cuts in cut_sets.items():
        try:
            out, per_window = sm.model_stream(case, case.text, cuts)
        except sm.Strangers as s:
            assert s.pair == e.stranger, kind
            continue
        except sm.Unpaired:
            assert case.last and e.odd, kind
            continue
        assert e.stranger is None and not (case.last and e.odd), kind
        assert out == e.out, kind
        assert sum(per_window) == 2 * e.n_pairs and all(n % 2 == 0 for n in per_window), kind


def test_pairing_changes_the_bytes_in_at_least_half_of_the_good_cases():
    """Otherwise "record_sam" alone would pass: the unpaired expectation of the same text and rule differs"""
    good = sm.good_cases()
    differ = [c.name for c in good if sm.expected(c).out != sm.expected(c).unpaired_out]
    assert len(good) >= 15 and 2 * len(differ) >= len(good), (len(differ), len(good))
    for c in sm.block_cases():
        if sm.expected(c).stranger is None:
            assert sm.expected(c).out != sm.expected(c).unpaired_out


def test_every_kind_named_occurs_in_a_case():
    every = CASES + sm.block_cases()
    seams = set().union(*[sm.seam_kinds(c) for c in every])
    assert seams >= {"mate2_at_tile_first_byte", "mate2_at_tile_last_byte", "mate2_tiles_on_behind_a_long_line", "span_block_straddled",
                     "tile_block_straddled"}
    decisions = set().union(*[sm.decision_kinds(c) for c in CASES])
    for m1 in (False, True):
        for m2 in (False, True):
            for rule in (sm.ANY, sm.BOTH):
                for inv in (False, True):
                    assert (m1, m2, rule, inv) in decisions
    assert "permille_between_the_mates" in decisions
    names = set().union(*[sm.name_kinds(c) for c in every])
    assert names >= {"equal_1", "equal_63", "equal_64", "equal_65", "equal_254", "star_twice", "differ_in_the_last_byte",
                     "one_a_prefix_of_the_other", "differ"}
    between = set().union(*[sm.between_kinds(c) for c in CASES])
    assert between >= {"supplementary", "mapq_floor", "region", "header_mode_1", "header_mode_2"}
    cuts = set().union(*[set(sm.cut_sets(c)) for c in CASES])
    assert cuts >= {"between_the_mates", "inside_mate_2s_name", "inside_mate_2s_seq", "inside_a_header_between_the_mates",
                    "a_window_of_unselected_lines_behind_a_waiting_mate"}
    e = {c.name: sm.expected(c) for c in every}
    assert e["strangers_first_pair"].stranger == 0 and e["strangers_last_byte"].stranger == 2
    assert e["blocks_dense_k1_strangers_in_block_2"].stranger > 1024
    assert e["odd_count"].odd and e["odd_count_last"].odd and e["none_selected"].n_records == 0 and e["none_selected"].out.count(b"\n") == 5
    crlf = sm.by_name("crlf").text
    assert crlf.count(b"\r\n") == crlf.count(b"\n")
    assert not sm.by_name("unterminated_last_line").text.endswith(b"\n")
    # a reverse-strand mate that hits in read orientation alone, with also_revcomp off: the pair's fate turns on it
    assert e["read_orientation"].out != e["as_stored"].out and e["read_orientation"].n_kept > e["as_stored"].n_kept


def test_a_header_line_between_two_mates_comes_out_in_front_of_the_pair():
    e = sm.expected(sm.by_name("header_between"))
    lines = e.out.split(b"\n")
    at = lines.index(b"@CO\tbetween the mates of a kept pair")
    assert lines[at + 1].startswith(b"h0\t67\t") and lines[at + 2].startswith(b"h0\t131\t")
    assert b"@CO\tbetween the mates of a dropped pair" in lines and not any(ln.startswith(b"h1\t") for ln in lines)
    assert e.out.endswith(b"@CO\tat the end\n")


# ---------------------------------------------------------------------------------------------- the shared source on the CPU
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_with_1_and_64_lanes_into_queues_of_exactly_the_models_size(lib, case):
    e = sm.model(case, sr.with_final_newline(case.text))                # (the driver ends the stream as the stream routes do)
    for lanes in (1, 64):
        for fill in (0x00, 0xFF):
            rc, out, st = _run(lib, case, case.text, e.out, lanes=lanes, fill=fill)
            if e.stranger is not None:
                assert rc == -8 and st[7] == e.stranger, (lanes, fill, rc, st)
                continue
            assert rc == 0 and out == e.out, (lanes, fill, rc)
            assert st[:7] == [e.n_records, e.n_excluded, e.n_headers, len(e.out), e.n_kept, 2 * e.n_pairs, int(e.odd)], st


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_streams_in_windows_with_a_waiting_mate_and_tails_at_every_residue(lib, case):
    e = sm.model(case, sr.with_final_newline(case.text))
    cut_sets = dict(sm.cut_sets(case), tiles=list(range(1024, len(case.text), 1024)), odd_places=[1, 2, 3, 1000, 1023, 1024, 1025, 2047, 2048])
    for kind, cuts in cut_sets.items():
        for tail0 in (0, 1, 15, 16, 33):
            rc, out, st = _run(lib, case, case.text, e.out, cuts, lanes=64, fill=0xFF, tail0=tail0)
            if e.stranger is not None:
                assert rc == -8 and st[7] == e.stranger, (kind, tail0, rc, st)
                continue
            assert rc == 0 and out == e.out, (kind, tail0, rc)
            assert st[4:7] == [e.n_kept, 2 * e.n_pairs, int(e.odd)], (kind, st)


@pytest.mark.parametrize("case", sm.block_cases(), ids=[c.name for c in sm.block_cases()])
def test_more_than_one_block_of_spans_and_of_tiles(lib, case):
    e = sm.expected(case)
    for cuts in ((), (len(case.text) // 3, 2 * len(case.text) // 3)):
        rc, out, st = _run(lib, case, case.text, e.out, cuts, lanes=64, fill=0xFF, tail0=7)
        if e.stranger is not None:
            assert rc == -8 and st[7] == e.stranger
            continue
        assert rc == 0 and out == e.out
        assert st[:7] == [e.n_records, e.n_excluded, e.n_headers, len(e.out), e.n_kept, 2 * e.n_pairs, int(e.odd)]


def test_a_queue_one_byte_short_is_noticed_before_anything_is_copied(lib):
    case = sm.by_name("patterns_any")
    e = sm.expected(case)
    assert _run(lib, case, case.text, e.out[:-1])[0] == -5


def test_the_mate_check_against_brute_force(lib):
    """All pairs of name lengths up to 70 with a difference at every position of the shorter name, lines without a TAB, with 1,
    16 and 64 lanes: equal in length and content, or strangers"""
    for lanes in (1, 16, 64):
        assert lib.sam_mates_names_sweep(lanes, 70) == 0


# ---------------------------------------------------------------------------------------------- under the sanitizers
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def sanitizers(tmp_path_factory):
    """Asked up front, with a program of one line: does this machine's g++ link the sanitizers' runtimes?"""
    tmp = tmp_path_factory.mktemp("san_probe")
    src = tmp / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", *SAN_FLAGS, str(src), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ does not link the sanitizers' runtimes here: " + probe.stderr[-200:])


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, sanitizers):
    """The same driver as an executable with ASan + UBSan (tests/sam_mates_san_main.cpp; host code, nothing sanitized is loaded
    into Python): the input, the entries, the tables, the waiting line and the queue live in heap buffers of exactly their size."""
    exe = str(tmp_path / "sam_mates_san")
    src = os.path.join(ROOT, "tests", "sam_mates_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", *SAN_FLAGS, "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    for lanes in (1, 64):
        run = subprocess.run([exe, "names", str(lanes), "40"], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.split() == ["0"], run.stderr[-2000:]
    inp, outp, jobp = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "job.bin"
    runs = [("patterns_both_inverted", 1, 0x00, 0, []), ("tile_seams", 64, 0xFF, 5, ["2048", "4095"]), ("tiles_on", 64, 0x00, 15, ["1500", "4000"]),
            ("between_supplementary_mapq_region", 1, 0xFF, 16, [str(c) for c in range(300, 4000, 411)]), ("header_between", 64, 0xFF, 1, ["560"]),
            ("names", 64, 0x00, 3, ["333"]), ("strangers_last_byte", 64, 0xFF, 0, []), ("odd_count", 1, 0x00, 9, ["2999"]),
            ("none_selected", 64, 0xFF, 2, ["100"]), ("crlf", 64, 0x00, 0, ["700"]), ("unterminated_last_line", 64, 0xFF, 4, []),
            ("read_orientation", 64, 0x00, 0, []), ("blocks_dense_k1", 64, 0xFF, 11, ["30000"]),
            ("blocks_big_inverted_no_header", 64, 0x00, 5, ["1048570"])]
    for name, lanes, fill, tail0, cuts in runs:
        case = sm.by_name(name)
        text = sr.with_final_newline(case.text)
        e = sm.model(case, text)
        hits, windows = _entries(case, text)
        rules, iv, names, offs = tables(case.sel)
        inp.write_bytes(case.text)
        jobp.write_bytes(struct.pack("<9I", case.excl, case.mode, int(case.orig), lanes, case.min_hits, case.min_permille, int(case.invert),
                                     PAIR_RULE[case.pair_rule], fill) +
                         struct.pack("<3Q", tail0, len(e.out), hits.shape[0]) + hits.astype("<u4").tobytes() + windows.astype("<u4").tobytes() +
                         struct.pack("<4Q", *rules) + b"".join(struct.pack("<3q", *t) for t in iv) +
                         struct.pack("<I", len(names)) + struct.pack("<%dI" % len(offs), *offs) + b"".join(names))
        run = subprocess.run([exe, "run", str(inp), str(outp), str(jobp)] + cuts, capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stderr[-3000:])
        got = [int(v) for v in run.stdout.split()]
        if e.stranger is not None:
            assert got[0] == -8 and got[8] == e.stranger, (name, got)
            continue
        assert got[:8] == [0, e.n_records, e.n_excluded, e.n_headers, len(e.out), e.n_kept, 2 * e.n_pairs, int(e.odd)], (name, got)
        assert outp.read_bytes() == e.out, name


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    from tests import record_hits_cases as rh
    bases, offsets = rh.reads_arrays([sr.hit_read(60, 0), sr.miss_read(60)])
    batch = ReadBatch(bases, offsets)
    paths = {ext: str(tmp_path / ("r." + ext)) for ext in ("bam", "sam", "fq")}
    paths["sam.gz"] = str(tmp_path / "r.sam.gz")
    reads_io.write_bam(paths["bam"], batch)
    reads_io.write_sam(paths["sam"], batch)
    reads_io.write_sam(paths["sam.gz"], batch, bgzf=True)
    reads_io.write_fastq(paths["fq"], batch)
    return paths


def test_the_command_line_refuses_before_the_index_is_read(tmp_path, monkeypatch):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.sam")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out]      # (the index does not exist)
    for ext in ("sam", "sam.gz", "fq", "bam"):
        with pytest.raises(ValueError, match="--sam-mates goes with --sam-out"):
            run_argument_parser(common + ["-f", paths[ext], "--sam-mates"])
    for ext in ("fq", "bam"):
        with pytest.raises(ValueError, match="--sam-out applies to SAM input only"):
            run_argument_parser(common + ["-f", paths[ext], "--sam-out", "--sam-mates"])
    # what --sam-out refuses stays refused in its words with --sam-mates beside it
    for option in (["--keep-mates"], ["--bam-pairs"], ["--interleaved"], ["--mate-suffix"]):
        with pytest.raises(ValueError, match="--sam-out does not go with %s" % option[0]):
            run_argument_parser(common + ["-f", paths["sam"], "--sam-out", "--sam-mates"] + option)
    # --pair-rule without a pairing option stays refused as before
    with pytest.raises(ValueError, match="--pair-rule goes with --interleaved or -f2"):
        run_argument_parser(common + ["-f", paths["sam"], "--sam-out", "--pair-rule", "both"])
    with pytest.raises(ValueError, match="--sam-out does not go with --min-base-quality"):
        run_argument_parser(common + ["-f", paths["sam"], "--sam-out", "--sam-mates", "--min-base-quality", "20"])
    assert not os.path.exists(out)


def test_with_the_switch_a_sam_file_passes_the_checks_up_to_the_index(tmp_path, monkeypatch):
    """--sam-out --sam-mates with every option that goes with it: the first thing that fails is the index file that does not exist."""
    from kmer_mapper_amd import command_line_interface as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.sam")
    args = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out, "--sam-out", "--sam-mates", "--pair-rule", "both", "--no-header",
            "--bgzf", "--min-hits", "2", "--min-hit-permille", "10", "--invert", "--hits-output", str(tmp_path / "h"), "--exclude-flags", "0x4",
            "--include-flags", "1", "--min-mapq", "20", "--regions", "chr1:1-500"]
    for ext in ("sam", "sam.gz"):
        with pytest.raises(Exception) as info:
            cli.run_argument_parser(args + ["-f", paths[ext]])
        assert "none.npz" in str(info.value) or isinstance(info.value, (FileNotFoundError, OSError)), info.value
    assert not os.path.exists(out)
    parsed = cli.build_argument_parser().parse_args(args + ["-f", paths["sam"]])
    assert parsed.sam_mates is True and parsed.pair_rule == "both"
    plain = cli.build_argument_parser().parse_args(["select-reads", "-i", "i.npz", "-f", paths["sam"], "-o", out, "--sam-out"])
    assert "sam_mates" not in vars(plain)                                          # (a call without it parses as it did before)
    cli.check_select_reads_sam_mates(True, True)
    sink = cli.RecordKeepSink(None, sam_out=True, sam_mates=True, pair_rule="both")
    assert sink.sam_mates and not cli.RecordKeepSink(None, sam_mates=True).sam_mates
