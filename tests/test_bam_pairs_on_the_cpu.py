"""CPU tier of keeping the mates of a name-collated BAM file together (include/kmm.h "record_names_pairs").  The
catalogue of tests/bam_pairs_cases.py is held to the conditions that keep it from being vacuous and to itself (the text of a case
through the pair model against a per-record derivation); the plain-C++ arithmetic of the mate check (csrc/kmm_record_keep.hpp:
rk_name_trim, rk_names_equal, rk_mate2_line) is compiled with g++ and run against the Python restatement over every case and over
all small strings, and once more as a stand-alone executable under ASan + UBSan; the command line's new refusals come before the
index is read, and a call without --bam-pairs parses as before."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import bam_fastq_cases as bc
from tests import bam_pairs_cases as bp
from tests import record_pairs_cases as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
GOOD, BAD = bp.good_cases(), bp.error_cases()
P, I64, U32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint32


# ---------------------------------------------------------------------------------------------- the catalogue
def test_the_catalogue_holds_what_the_issue_lists():
    names = {c.name for c in bp.all_cases()}
    assert len(names) == len(bp.all_cases())
    assert {c.error[0] for c in BAD} == {"strangers", "unpaired"}
    assert all(c.min_hits == 1 for c in bp.all_cases())
    assert max(len(bc.read_bam(c.base.payload)[1]) for c in bp.all_cases()) <= 400          # (small files)


@pytest.mark.parametrize("case", GOOD, ids=lambda c: c.name)
def test_every_good_case_keeps_a_pair_and_drops_a_pair(case):
    e = bp.expected(case)
    assert 0 < e.n_kept < e.n_pairs, (e.n_kept, e.n_pairs)
    assert bp.error_of(case.base) is None


@pytest.mark.parametrize("case", GOOD, ids=lambda c: c.name)
def test_the_model_against_itself(case):
    """The kept bytes of the pair model are the texts of the kept pairs' records, the entries those of the record-wise model of
    tests/bam_fastq_cases.py, and the keep flags the pair rule over them."""
    e = bp.expected(case)
    d = bc.decoded(case.base)
    _, _, _, hits, windows = bc.expected(bc.BCase("pairs_cpu_" + case.name, case.base, 1, 0, False))
    assert np.array_equal(e.hits, hits) and np.array_equal(e.windows, windows)
    keep = [rp.pair_keep(int(hits[2 * p]), int(windows[2 * p]), int(hits[2 * p + 1]), int(windows[2 * p + 1]), case.min_hits,
                         case.min_permille, case.invert, case.pair_rule) for p in range(len(hits) // 2)]
    assert keep == e.keep.tolist()
    assert e.text1 == b"".join(d.texts[2 * p] + d.texts[2 * p + 1] for p, kp in enumerate(keep) if kp)
    assert len(e.text1) % 2 == 0                                         # (why the kept span ends at even residues only)


def test_every_feature_occurs_in_a_kept_and_in_a_dropped_pair():
    seen = {f: [False, False] for f in bp.FEATURES}
    for case in GOOD:
        for f_set, kept in zip(bp.features(case), bp.expected(case).keep.tolist()):
            for f in f_set:
                seen[f][int(kept)] = True
    assert {f: v for f, v in seen.items() if v != [True, True]} == {}


def test_the_four_hit_patterns_and_a_threshold_between_the_mates():
    for name, permille in (("patterns__", 0), ("permille_150__", 150)):
        e = bp.expected(bp.by_name(name + "any"))
        match = [(int(h) >= 1 and 1000 * int(h) >= permille * int(w)) for h, w in zip(e.hits, e.windows)]
        assert {(match[i], match[i + 1]) for i in range(0, len(match), 2)} == set(itertools.product((True, False), repeat=2))
        kept = {tag: bp.expected(bp.by_name(name + tag)).keep.tolist() for tag in ("any", "any_invert", "both", "both_invert")}
        assert kept["any"] != kept["both"] and kept["any_invert"] == [not k for k in kept["any"]]
        assert kept["both_invert"] == [not k for k in kept["both"]]


def test_the_kept_span_ends_at_the_residues_the_docstring_names():
    case = bp.by_name("residues__any")
    e, d = bp.expected(case), bc.decoded(case.base)
    at, ends = 0, []
    for p, kp in enumerate(e.keep.tolist()):
        if kp:
            at += len(d.texts[2 * p]) + len(d.texts[2 * p + 1])
            ends.append(at % 16)
    assert ends == [14, 0, 2] * 3


def test_the_windows_end_inside_every_part_of_either_mate_and_the_carries_are_not_empty():
    kinds = set()
    for name in ("windows_every_97__any", "windows_every_301__any"):
        kinds |= {(mate, kind, carried) for mate, kind, carried, _ in bp.boundary_kinds(bp.by_name(name))}
    for part in ("head", "name", "seq", "qual"):
        assert (1, part, False) in kinds and (2, part, True) in kinds, part         # (inside mate 2: mate 1 is the text carry)
    # the carry that lives through a window without a selected record and one without a complete record
    k = bp.boundary_kinds(bp.by_name("carry_over_empty_windows__any"))
    assert [(mate, carried, new) for mate, _, carried, new in k] == [(None, True, 3), (None, True, 0), (2, True, 0)]
    assert k[2][1] in ("head", "name", "seq")
    # a long record: windows that hold no complete record at all, in either mate
    k = bp.boundary_kinds(bp.by_name("lengths_in_windows__any"))
    assert any(new == 0 and carried for _, _, carried, new in k) and any(new == 0 and not carried for _, _, carried, new in k)
    # the pair astride the carry is the stranger of its case
    case = bp.by_name("astride_the_carry")
    assert case.error == ("strangers", 7) and bp.selected_done(case)[0] == 15 and bp.window_of(case) == 1
    marks = bp.straddle_base()[1]
    for kind, goal, len1, len2 in marks:
        tile = -(-goal // bp.TILE) * bp.TILE
        inside = tile - goal
        assert {"mate1": 0 < inside < len1, "between": inside == len1, "mate2": len1 < inside < len1 + len2}[kind]


@pytest.mark.parametrize("case", BAD, ids=lambda c: c.name)
def test_the_error_cases_fail_where_the_docstrings_say(case):
    want = {"last_byte_at_pair_0": ("strangers", 0), "first_byte_in_the_middle": ("strangers", 9), "prefix_in_the_last_pair": ("strangers", 19),
            "longer_in_the_middle": ("strangers", 10), "astride_the_carry": ("strangers", 7), "suffix_does_not_hide_it": ("strangers", 3),
            "coordinate_sorted": ("strangers", 0), "trio_with_0x900_not_excluded": ("strangers", 3), "odd_count": ("unpaired", 13),
            "odd_count_in_windows": ("unpaired", 13), "a_selection_that_removes_one_mate": ("unpaired", 7)}
    assert case.error == want[case.name]
    assert 0 <= bp.window_of(case) < len(bp.window_ends(case))


def test_windowed_files_inflate_to_the_payload_and_their_windows_end_at_members():
    for name in ("windows_every_97__any", "carry_over_empty_windows__any", "odd_count_in_windows"):
        case = bp.by_name(name)
        comp, windows = bp.windowed_file(case)
        assert bc.inflate(comp) == case.base.payload
        assert windows[0][0] == 0 and windows[-1][1] == len(comp) and all(a[1] == b[0] for a, b in zip(windows, windows[1:]))
        _, _, hdr = bc.read_bam(case.base.payload)
        for (lo, hi), end in zip(windows, bp.window_ends(case)):
            assert len(bc.inflate(comp[:hi])) == hdr + end and comp[lo:lo + 4] == b"\x1f\x8b\x08\x04"


# ---------------------------------------------------------------------------------------------- the plain-C++ arithmetic
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_pairs")
    src = tmp / "shim.cpp"
    src.write_text('#include "bam_pairs_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.bam_pairs_names_equal_cpu.argtypes = [ctypes.c_char_p, U32, ctypes.c_char_p, U32, U32]
    lib.bam_pairs_name_trim_cpu.argtypes = [ctypes.c_char_p, U32, U32]
    lib.bam_pairs_name_trim_cpu.restype = U32
    lib.bam_pairs_mate2_line_cpu.argtypes = [I64, I64, I64]
    lib.bam_pairs_mate2_line_cpu.restype = I64
    lib.bam_pairs_check_cpu.argtypes = [P, I64, U32, P]
    lib.bam_pairs_check_cpu.restype = I64
    return lib


def _trimmed(name, suffix):
    return name[:-2] if suffix and len(name) >= 2 and name[-2:] in (b"/1", b"/2") else name


def test_name_comparison_over_all_small_strings(lib):
    alphabet = b"/12a"
    strings = [bytes(t) for n in range(5) for t in itertools.product(alphabet, repeat=n)]
    assert len(strings) == 341
    for suffix in (0, 1):
        for a in strings:
            assert lib.bam_pairs_name_trim_cpu(a, len(a), suffix) == len(_trimmed(a, suffix))
            for b in strings:
                want = _trimmed(a, suffix) == _trimmed(b, suffix)
                assert lib.bam_pairs_names_equal_cpu(a, len(a), b, len(b), suffix) == int(want), (a, b, suffix)


def test_mate_2_line_arithmetic_over_small_records(lib):
    for n_name, l_seq, at in itertools.product(range(0, 5), range(0, 5), (0, 7)):
        rec = b"@" + b"n" * n_name + b"\n" + b"A" * l_seq + b"\n+\n" + b"I" * l_seq + b"\n"
        text = b"x" * at + rec + b"@"
        e0 = text.index(b"\n", at)
        e1 = text.index(b"\n", e0 + 1)
        assert lib.bam_pairs_mate2_line_cpu(at, e0, e1) == at + len(rec)


@pytest.mark.parametrize("case", bp.all_cases(), ids=lambda c: c.name)
def test_the_check_agrees_with_the_restatement_on_every_case(lib, case):
    d = bc.decoded(case.base)
    n_pairs = len(d.texts) // 2
    text = np.frombuffer(b"".join(d.texts[:2 * n_pairs]) or b"\n", dtype=np.uint8)
    stats = np.zeros(2, dtype=np.int64)
    got = lib.bam_pairs_check_cpu(text.ctypes.data, text.shape[0] if n_pairs else 0, int(case.base.suffix), stats.ctypes.data)
    want = bp.first_stranger(d.texts, case.base.suffix)
    assert got == (-1 if want is None else want) and stats[0] == n_pairs
    if case.error and case.error[0] == "strangers":
        assert want == case.error[1]


def test_arithmetic_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/bam_pairs_san_main.cpp; host code, nothing sanitized is loaded into
    Python): the text lives in a heap buffer of exactly its size."""
    exe = str(tmp_path / "bam_pairs_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "bam_pairs_san_main.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    path, ran = str(tmp_path / "text.bin"), 0
    for case in bp.all_cases():
        d = bc.decoded(case.base)
        n_pairs = len(d.texts) // 2
        if not n_pairs:
            continue
        open(path, "wb").write(b"".join(d.texts[:2 * n_pairs]))
        r = subprocess.run([exe, path, str(int(case.base.suffix))], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (case.name, r.stdout, r.stderr[-2000:])
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        want = bp.first_stranger(d.texts, case.base.suffix)
        assert r.stdout.split()[:4] == ["ok", str(sum(len(t) for t in d.texts[:2 * n_pairs])), str(n_pairs), str(-1 if want is None else want)]
        ran += 1
    assert ran == len(bp.all_cases())


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    batch = ReadBatch.from_strings(["ACGTACGTAC", "GGGTTTAAAC"])
    paths = {name: str(tmp_path / name) for name in ("r.sam", "r.bam", "r.fq", "r2.fq")}
    reads_io.write_sam(paths["r.sam"], batch)
    reads_io.write_bam(paths["r.bam"], batch)
    reads_io.write_fastq(paths["r.fq"], batch)
    reads_io.write_fastq(paths["r2.fq"], batch)
    return paths


def test_bam_pairs_refusals_come_before_the_index_is_read(tmp_path, monkeypatch):
    """Refused with ValueError before the index file is read (there is none), and before -o is created."""
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    f = _files(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out, out2 = str(tmp_path / "kept.fq"), str(tmp_path / "kept2.fq")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out]
    refused = [(["-f", f["r.bam"], "--bam-pairs"], "--bam-pairs goes with --bam-to-fastq"),
               (["-f", f["r.fq"], "--bam-pairs"], "--bam-pairs applies to BAM input only"),
               (["-f", f["r.fq"], "--bam-pairs", "--interleaved"], "--bam-pairs applies to BAM input only"),
               (["-f", f["r.sam"], "--bam-pairs", "--bam-to-fastq"], "--bam-pairs applies to BAM input only"),
               (["-f", f["r.bam"], "--bam-to-fastq", "--bam-pairs", "--interleaved"], "--bam-pairs does not go with --interleaved"),
               (["-f", f["r.bam"], "--bam-to-fastq", "--bam-pairs", "-f2", f["r2.fq"], "-o2", out2], "--bam-pairs does not go with -f2"),
               (["-f", f["r.bam"], "--bam-to-fastq", "--bam-pairs", "-o2", out2], "--bam-pairs does not go with -o2"),
               (["-f", f["r.bam"], "--bam-to-fastq", "--pair-rule", "both"], "--pair-rule goes with"),
               (["-f", f["r.bam"], "--bam-to-fastq", "--interleaved"], "BAM.*out of scope")]
    before = {name: open(path, "rb").read() for name, path in f.items()}
    for more, message in refused:
        with pytest.raises(ValueError, match=message):
            run_argument_parser(common + more)
    # accepted up to the index, which is not there: --pair-rule goes with --bam-pairs
    with pytest.raises((FileNotFoundError, OSError)):
        run_argument_parser(common + ["-f", f["r.bam"], "--bam-to-fastq", "--bam-pairs", "--pair-rule", "both", "--mate-suffix", "--bgzf"])
    assert {name: open(path, "rb").read() for name, path in f.items()} == before
    assert not os.path.exists(out) and not os.path.exists(out2)


def test_the_option_parses_and_a_call_without_it_parses_as_before():
    from kmer_mapper_amd.command_line_interface import build_argument_parser, select_reads_file
    parser = build_argument_parser()
    a = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.bam", "-o", "kept.fq", "--bam-to-fastq"])
    assert "bam_pairs" not in vars(a) and a.bam_to_fastq is True and a.func is select_reads_file
    b = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.bam", "-o", "kept.fq", "--bam-to-fastq", "--bam-pairs", "--pair-rule", "both"])
    assert b.bam_pairs is True and b.pair_rule == "both"
    assert set(vars(b)) - set(vars(a)) == {"bam_pairs", "pair_rule"}
    c = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.fq", "-o", "kept.fq"])
    assert not {"bam_pairs", "bam_to_fastq", "pair_rule"} & set(vars(c))
