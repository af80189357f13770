"""CPU tier of keeping mates together (include/kmm.h KEEPING MATES TOGETHER).  The catalogue's model
(tests/record_pairs_cases.py) against a second route — every record's sequence line through the oracle's extract -> in_index —
and the conditions that keep the catalogue from being vacuous; the pair rule, the pair form of the lane mask and the line
search of the cut (csrc/kmm_record_keep.hpp, csrc/kmm_line_search.hpp) compiled with g++ against brute force on every case
(once more under ASan + UBSan as a stand-alone executable), also on lane masks that no text produces; the command line's
refusals, which need no GPU, and the unchanged parsing of the commands without the new options."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests import record_pairs_cases as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = rp.all_cases()
IDS = [c.name for c in CASES]
SMALL = [c for c in CASES if c.text1.shape[0] < 100_000]
I64, U32, P = ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("case", [c for c in SMALL if c.lut is None], ids=lambda c: c.name)
def test_model_agrees_with_the_oracle(case, oracle):
    want = rp.expected(case)
    m1, m2 = rp.mates_of(case)
    keep = []
    for a, b in zip(m1, m2):
        match = []
        for _, seq in (a, b):
            n = max(len(seq) - case.k + 1, 0)
            hits = 0
            if n:
                kmers = oracle.extract(np.frombuffer(seq, dtype=np.uint8), np.array([0, len(seq)], dtype=np.int64), case.k)
                hits = int(oracle.in_index(case.index, kmers).sum())
            match.append(hits >= case.min_hits and 1000 * hits >= case.min_permille * n)
        pair = (match[0] or match[1]) if case.pair_rule == rp.ANY else (match[0] and match[1])
        keep.append(pair != case.invert)
    assert keep == want.keep.tolist()
    if case.text2 is None:
        assert want.text1 == b"".join(a[0] + b[0] for a, b, kp in zip(m1, m2, keep) if kp)
    else:
        assert want.text1 == b"".join(a[0] for a, kp in zip(m1, keep) if kp)
        assert want.text2 == b"".join(b[0] for b, kp in zip(m2, keep) if kp)


def test_every_case_keeps_some_and_drops_some():
    for c in CASES:
        e = rp.expected(c)
        if c.name.startswith("empty_"):
            assert e.n_pairs == 0 and e.n_kept == 0 and (e.consumed1, e.consumed2) == (0, 0)
        else:
            assert 0 < e.n_kept < e.n_pairs, c.name
            assert e.hits.shape == (2 * e.n_pairs,) and len(e.text1) > 0


def test_the_catalogue_holds_what_the_issue_lists():
    by = rp.by_name
    # the four hit patterns, told apart by the four rules
    e = {r: rp.expected(by("patterns_fastq_interleaved__" + r)) for r in ("any", "both", "any_invert", "both_invert")}
    match = [(h > 0) for h in e["any"].hits.tolist()]
    assert [tuple(match[i:i + 2]) for i in range(0, 10, 2)] == [(True, False), (False, True), (True, True), (False, False), (True, False)]
    assert e["any"].keep.tolist() == [True, True, True, False, True] and e["both"].keep.tolist() == [False, False, True, False, False]
    assert (e["any_invert"].keep == ~e["any"].keep).all() and (e["both_invert"].keep == ~e["both"].keep).all()
    # a per-mille threshold one mate passes and the other fails, in either order
    e = rp.expected(by("permille_fastq_two_files__150_any"))
    h, w = e.hits.tolist(), e.windows.tolist()
    passes = [1000 * a >= 150 * b and a >= 1 for a, b in zip(h, w)]
    assert passes[:4] == [True, False, False, True] and h[0] == h[1] > 0 and w[0] < w[1]
    assert e.keep.tolist() != rp.expected(by("permille_fastq_two_files__150_both")).keep.tolist()
    # a break table that empties one mate's windows
    e = rp.expected(by("breaks_fastq_interleaved__min_hits_0_permille_200_both"))
    assert e.windows[0] == 0 and e.windows[1] > 0 and e.windows[3] == 0 and e.keep.tolist() == [True, True, True, False, False]
    # the seams: a mate 1 that ends exactly at a lane, tile and group boundary, a mate 2 one before, at and one behind a tile's
    text, marks = rp.seam_text(rh.FASTQ)
    ends = np.cumsum([len(r[0]) for r in rp.records(text, rh.FASTQ)]).tolist()
    for what, at in marks:
        i = ends.index(at)
        assert i % 2 == (1 if what.startswith("mate2") else 0), what
    assert [at % rp.LINE for _, at in marks[:3]] == [0, 0, 0] and marks[0][1] % rp.TILE and marks[1][1] % rp.TILE == 0
    assert marks[1][1] % rp.GROUP and marks[2][1] % rp.GROUP == 0 and [at % rp.TILE for _, at in marks[3:]] == [rp.TILE - 1, 0, 1]
    kept = rp.expected(by("seams_fastq_interleaved__any")).keep
    assert all(kept[ends.index(at) // 2] for _, at in marks)
    big = by("super_seam_fastq_interleaved__any")
    ends = np.cumsum([len(r[0]) for r in rp.records(big.text1, rh.FASTQ)]).tolist()
    i = ends.index(rp.SUPER)
    assert i % 2 == 0 and rp.expected(big).keep[i // 2] and not rp.expected(big).keep[i // 2 - 1]
    # kept runs that end at 15, 16 and 17 modulo 16 of the output: of the one queue, and of both
    e = rp.expected(by("residues_fasta_interleaved__any"))
    m1, m2 = rp.mates_of(by("residues_fasta_interleaved__any"))
    run = np.cumsum([len(a[0]) + len(b[0]) for a, b, kp in zip(m1, m2, e.keep) if kp])
    assert [int(x) % 16 for x in run] == [15, 0, 1] * 3
    c = by("residues_fasta_two_files__any")
    e = rp.expected(c)
    for mates in rp.mates_of(c):
        run = np.cumsum([len(a[0]) for a, kp in zip(mates, e.keep) if kp])
        assert [int(x) % 16 for x in run] == [15, 0, 1] * 3
    assert len(e.text1) != len(e.text2)
    # piece cuts: every piece's byte limit falls inside a mate 2 whose mate 1 lies in front of it
    c = by("pieces_fastq_interleaved__any")
    spans = np.cumsum([0] + [len(r[0]) for r in rp.records(c.text1, c.fmt)]).tolist()
    start = 0
    while start + 1024 < c.text1.shape[0]:
        limit = start + 1024
        i = next(i for i in range(len(spans) - 1) if spans[i] < limit < spans[i + 1])
        assert i % 2 == 1 and spans[i - 1] >= start                  # inside a mate 2: the unpaired cut would keep its mate 1
        start = spans[i - 1]                                         # the pair-aligned cut: in front of that mate 1
    # odd record counts; surplus records of one and of many; cuts around a tile boundary and the super-tile seam
    c = by("odd_fastq_interleaved__any")
    assert len(rp.records(c.text1, c.fmt)) == 2 * rp.expected(c).n_pairs + 1 and rp.expected(c).consumed1 < c.text1.shape[0]
    for name, d1, d2 in (("first_one_more", 1, 0), ("first_many_more", 7, 0), ("second_one_more", 0, 1), ("second_many_more", 0, 8)):
        c = by("surplus_%s_two_files__both" % name)
        m = rp.expected(c).n_pairs
        assert (len(rp.records(c.text1, c.fmt)), len(rp.records(c.text2, c.fmt))) == (m + d1, m + d2)
    for d in (-1, 0, 1):
        for name, seam in (("cut_at_tile_%+d_two_files__any", 3 * rp.TILE), ("cut_at_super_tile_%+d_two_files__any", rp.SUPER)):
            c = by(name % d)
            assert rp.expected(c).consumed1 == seam + d and len(rp.records(c.text1, c.fmt)) == rp.expected(c).n_pairs + 3
    c = by("lengths_150_100_two_files__any")
    assert {len(s) for _, s in rp.records(c.text1, c.fmt)} == {150} and {len(s) for _, s in rp.records(c.text2, c.fmt)} == {100}


def test_interleave_and_deinterleave_are_inverse():
    c = rp.by_name("lengths_150_100_two_files__any")
    both = rp.interleave(c.text1, c.text2, c.fmt)
    assert rp.deinterleave(both, c.fmt) == (c.text1.tobytes(), c.text2.tobytes())


# ---------------------------------------------------------------------------------------------- the plain-C++ helpers
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_pairs")
    src = tmp / "shim.cpp"
    src.write_text('#include "record_pairs_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.record_pairs_rule_cpu.argtypes = [U32] * 8
    lib.record_pairs_cpu.argtypes = [P, I64, I64, U32, U32, P, P, I64, U32, U32, U32, U32, I64, P, I64, P]
    lib.record_pairs_lane_cpu.argtypes = [U32, U32, U32, U32, I64, I64, P, P, I64, U32, U32, U32, U32, P]
    lib.record_pairs_cut_cpu.argtypes = lib.record_pairs_cut_brute.argtypes = [P, I64, U32]
    lib.record_pairs_cut_cpu.restype = lib.record_pairs_cut_brute.restype = I64
    return lib


def test_the_pair_rule_over_all_sixteen_combinations_and_the_64_bit_edge(lib):
    passing, failing = (5, 10), (0, 10)
    for m1, m2, both, invert in itertools.product((True, False), repeat=4):
        a, b = (passing if m1 else failing), (passing if m2 else failing)
        want = ((m1 and m2) if both else (m1 or m2)) != invert
        assert lib.record_pairs_rule_cpu(a[0], a[1], b[0], b[1], 1, 100, int(invert), int(both)) == int(want), (m1, m2, both, invert)
        assert rp.pair_keep(a[0], a[1], b[0], b[1], 1, 100, invert, rp.BOTH if both else rp.ANY) == want
    # 1000 * hits and min_permille * windows beyond 2^32: no wrap in either mate
    top = 2 ** 32 - 1
    for h1, w1, h2, w2, permille in ((top, top, 5_000_000, top, 1000), (5_000_000, top, top, top - 1, 1000), (5_000_000, top, 4_294_968, top, 1),
                                     (4_294_967, top, 4_294_967, top, 1), (top, top, top, top, 1000)):
        for rule in (0, 1):
            want = rp.pair_keep(h1, w1, h2, w2, 0, permille, False, (rp.ANY, rp.BOTH)[rule])
            assert lib.record_pairs_rule_cpu(h1, w1, h2, w2, 0, permille, 0, rule) == int(want), (h1, w1, h2, w2, permille, rule)
    assert lib.record_pairs_rule_cpu(top, top, 5_000_000, top, 0, 1000, 0, 0) == 1 and lib.record_pairs_rule_cpu(top, top, 5_000_000, top, 0, 1000, 0, 1) == 0


def _pieces(case):
    """(text of one buffer from a pair boundary on, pair_shift, the entries of its pairs, expected kept text) — the whole
    buffers, and for interleaved text pieces that start at later pairs (other offsets of the lanes against the records)."""
    e = rp.expected(case)
    m1, m2 = rp.mates_of(case)
    n = e.n_pairs
    if case.text2 is None:
        starts = np.cumsum([0] + [len(a[0]) + len(b[0]) for a, b in zip(m1, m2)]).tolist()
        for first in sorted({0, 1, n // 2, n - 1} & set(range(n))):
            want = b"".join(a[0] + b[0] for a, b, kp in list(zip(m1, m2, e.keep))[first:] if kp)
            yield case.text1[starts[first]:], 1, e.hits[2 * first:], e.windows[2 * first:], n - first, want
    else:
        yield case.text1, 0, e.hits, e.windows, n, e.text1
        yield case.text2, 0, e.hits, e.windows, n, e.text2


@pytest.mark.parametrize("case", [c for c in CASES if rp.expected(c).n_pairs], ids=lambda c: c.name)
def test_helpers_agree_with_the_model(lib, case):
    shift = rh.PERIOD[case.fmt].bit_length() - 1
    for text, pair_shift, hits, windows, n_pairs, want in _pieces(case):
        text, hits, windows = np.ascontiguousarray(text), np.ascontiguousarray(hits), np.ascontiguousarray(windows)
        n_records = n_pairs << pair_shift
        consumed = int(np.nonzero(text == 10)[0][n_records * rh.PERIOD[case.fmt] - 1]) + 1
        for tail in ((0, 15, 4097) if text.shape[0] < 100_000 else (5,)):
            out = np.full(tail + len(want) + 64, 0xEE, dtype=np.uint8)
            stats = np.zeros(5, dtype=np.int64)
            lib.record_pairs_cpu(text.ctypes.data, text.shape[0], consumed, shift, pair_shift, hits.ctypes.data, windows.ctypes.data,
                                 n_records, case.min_hits, case.min_permille, int(case.invert), int(case.pair_rule == rp.BOTH), tail,
                                 out.ctypes.data, out.shape[0], stats.ctypes.data)
            n_kept = want.count(b"\n") // rh.PERIOD[case.fmt]
            assert stats.tolist() == [len(want), n_kept, 0, 0, 0], (tail, stats)
            assert out[tail:tail + len(want)].tobytes() == want
            assert (out[:tail] == 0xEE).all() and (out[tail + len(want):] == 0xEE).all()


@pytest.mark.parametrize("name", ["patterns_fastq_interleaved__any", "patterns_fasta_two_files__both_invert",
                                  "permille_fastq_interleaved__150_both", "seams_fasta_interleaved__any_invert"])
def test_the_pair_lane_mask_on_masks_no_text_produces(lib, name):
    case = rp.by_name(name)
    e = rp.expected(case)
    shift, pair_shift = rh.PERIOD[case.fmt].bit_length() - 1, 1 if case.text2 is None else 0
    n_records = e.n_pairs << pair_shift
    hits, windows = np.ascontiguousarray(e.hits), np.ascontiguousarray(e.windows)
    rng = np.random.default_rng(7)
    out = np.zeros(3, dtype=np.uint32)
    differ = 0
    for i in range(3000):
        nl = int(rng.integers(0, 1 << 16)) if i % 4 else (0xFFFF, 0, 0x8001, 0x5555)[(i // 4) % 4]
        line0 = int(rng.integers(0, (n_records << shift) + 3))
        p0 = 16 * int(rng.integers(0, 64))
        end = p0 + int(rng.integers(-12, 30))
        lib.record_pairs_lane_cpu(line0, nl, shift, pair_shift, p0, end, hits.ctypes.data, windows.ctypes.data, n_records, case.min_hits,
                                  case.min_permille, int(case.invert), int(case.pair_rule == rp.BOTH), out.ctypes.data)
        assert out[0] == out[1], (i, line0, hex(nl), p0, end, hex(out[0]), hex(out[1]))
        differ += out[0] not in (0, 0xFFFF)
    assert differ > 100                                                # (masks that change inside the lane)


@pytest.mark.parametrize("name", ["patterns_fasta_interleaved__any", "seams_fastq_interleaved__any", "cut_at_tile_+0_two_files__any",
                                  "cut_at_super_tile_-1_two_files__any", "cut_at_super_tile_+0_two_files__any",
                                  "cut_at_super_tile_+1_two_files__any", "super_seam_fastq_interleaved__any"])
def test_the_line_search_of_the_cut(lib, name):
    case = rp.by_name(name)
    text = case.text1
    n_lines = int((text == 10).sum())
    period = rh.PERIOD[case.fmt]
    targets = set(range(0, min(n_lines, 40) + 1)) | set(range(max(n_lines - 40, 0), n_lines + 3)) | set(range(period, n_lines, 37 * period))
    m = rp.expected(case).n_pairs
    targets |= {m * period, 2 * m * period}
    ends = np.nonzero(text == 10)[0] + 1
    for target in sorted(t for t in targets if t >= 0):
        want = int(ends[target - 1]) if 1 <= target <= n_lines else -1
        assert lib.record_pairs_cut_brute(text.ctypes.data, text.shape[0], target) == want
        assert lib.record_pairs_cut_cpu(text.ctypes.data, text.shape[0], target) == want, target
    if case.text2 is not None and m:                                   # where the two-file call cuts this buffer
        assert lib.record_pairs_cut_cpu(text.ctypes.data, text.shape[0], m * period) == rp.expected(case).consumed1


def test_helpers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/record_pairs_san_main.cpp; host code, nothing sanitized is
    loaded into Python): text, entries and the output live in heap buffers of exactly their size."""
    exe = str(tmp_path / "record_pairs_san")
    src = os.path.join(ROOT, "tests", "record_pairs_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    t_path, e_path = str(tmp_path / "text.bin"), str(tmp_path / "entries.bin")
    ran = 0
    for case in CASES:
        if not rp.expected(case).n_pairs or (case.text1.shape[0] > 100_000 and "+0" not in case.name and "super_seam" not in case.name):
            continue
        shift = str(rh.PERIOD[case.fmt].bit_length() - 1)
        rule = [str(case.min_hits), str(case.min_permille), str(int(case.invert)), str(int(case.pair_rule == rp.BOTH))]
        for text, pair_shift, hits, windows, n_pairs, want in _pieces(case):
            np.ascontiguousarray(text).tofile(t_path)
            np.concatenate([hits, windows]).astype(np.uint32).tofile(e_path)
            r = subprocess.run([exe, t_path, e_path, shift, str(pair_shift)] + rule + ["13"], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (case.name, r.stdout, r.stderr[-2000:])
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            got = r.stdout.split()
            assert got[0] == "ok" and got[5:8] == ["0", "0", "0"], (case.name, r.stdout)
            assert got[1] == str(text.shape[0]) and got[3] == str(len(want)) and int(got[9]) > 3
            ran += 1
    assert ran > 60


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    batch = ReadBatch.from_strings(["ACGTACGTAC", "GGGTTTAAAC"])
    paths = {name: str(tmp_path / name) for name in ("r.sam", "r.bam", "r1.fq", "r2.fq", "r.fa", "wrapped.fa")}
    reads_io.write_sam(paths["r.sam"], batch)
    reads_io.write_bam(paths["r.bam"], batch)
    reads_io.write_fastq(paths["r1.fq"], batch)
    reads_io.write_fastq(paths["r2.fq"], batch)
    reads_io.write_fasta(paths["r.fa"], batch)
    reads_io.write_fasta(paths["wrapped.fa"], batch, line_width=4)
    return paths


def test_pair_refusals_come_before_the_index_is_read(tmp_path, monkeypatch):
    """Refused with ValueError before the index file is read (there is none), and before -o / -o2 are created."""
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    f = _files(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out, out2 = str(tmp_path / "kept1.fq"), str(tmp_path / "kept2.fq")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5"]
    refused = [
        (["-f", f["r1.fq"], "-o", out, "--interleaved", "-f2", f["r2.fq"], "-o2", out2], "--interleaved.*-f2"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["r2.fq"]], "-f2/--reads2 needs -o2"),
        (["-f", f["r1.fq"], "-o", out, "-o2", out2], "-o2/--output2 goes with -f2"),
        (["-f", f["r1.fq"], "-o", out, "--pair-rule", "both"], "--pair-rule goes with"),
        (["-f", f["wrapped.fa"], "-o", out, "--interleaved"], "multi-line FASTA.*out of scope"),
        (["-f", f["r.sam"], "-o", out, "--interleaved"], "SAM.*out of scope"),
        (["-f", f["r.bam"], "-o", out, "--interleaved", "--bam-to-fastq"], "BAM.*out of scope"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["r.bam"], "-o2", out2], "BAM.*out of scope"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["wrapped.fa"], "-o2", out2], "multi-line FASTA.*out of scope"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["r.fa"], "-o2", out2], "differ in format"),
        (["-f", f["r1.fq"], "-o", f["r2.fq"], "-f2", f["r2.fq"], "-o2", out2], "-o .* is the input file \\(-f2\\)"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["r2.fq"], "-o2", f["r1.fq"]], "-o2 .* is the input file \\(-f\\)"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["r2.fq"], "-o2", os.path.join(str(tmp_path), ".", "r2.fq")], "-o2 .* is the input file \\(-f2\\)"),
        (["-f", f["r1.fq"], "-o", out, "-f2", f["r2.fq"], "-o2", out], "-o and -o2 name the same file"),
        (["-f", f["r1.fq"], "-o", f["r1.fq"], "--interleaved"], "is the input file"),
    ]
    before = {name: open(path, "rb").read() for name, path in f.items()}
    for more, message in refused:
        with pytest.raises(ValueError, match=message):
            run_argument_parser(common + more)
    with pytest.raises(SystemExit):                                     # (argparse: not one of the choices)
        run_argument_parser(common + ["-f", f["r1.fq"], "-o", out, "--interleaved", "--pair-rule", "either"])
    assert {name: open(path, "rb").read() for name, path in f.items()} == before
    assert not os.path.exists(out) and not os.path.exists(out2)


def test_the_pair_options_parse_and_a_call_without_them_parses_as_before():
    from kmer_mapper_amd.command_line_interface import build_argument_parser, select_reads_file
    parser = build_argument_parser()
    a = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.fq.gz", "-o", "kept.fq"])
    assert not {"interleaved", "reads2", "output2", "pair_rule"} & set(vars(a)) and a.func is select_reads_file
    b = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r1.fq", "-f2", "r2.fq", "-o", "k1.fq", "-o2", "k2.fq", "--pair-rule", "both"])
    assert (b.reads, b.reads2, b.output_file, b.output2, b.pair_rule) == ("r1.fq", "r2.fq", "k1.fq", "k2.fq", "both")
    c = parser.parse_args(["select-reads", "-i", "x.npz", "--reads", "r.fq", "--reads2", "s.fq", "-o", "a", "--output2", "b"])
    assert (c.reads, c.reads2, c.output2) == ("r.fq", "s.fq", "b") and "pair_rule" not in vars(c)
    d = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.fq", "-o", "a", "--interleaved"])
    assert d.interleaved is True and "reads2" not in vars(d)
