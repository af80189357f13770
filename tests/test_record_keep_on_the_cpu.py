"""CPU tier of the record-keep mode (include/kmm.h).  The catalogue's model (tests/record_keep_cases.py) against a
second route — records grouped from a plain split at '\\n', every record's reads through the oracle's extract -> in_index — and
the conditions that keep the catalogue from being vacuous; the line -> record, keep-rule, clipping and destination arithmetic
of csrc/kmm_record_keep.hpp compiled with g++ against brute force on every case (once more under ASan + UBSan as a stand-alone
executable), also on masks that no text produces; the command line's refusals and the unchanged parsing of `map` / `read-hits`."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh
from tests import record_keep_cases as rk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = rk.all_cases()
IDS = [c.name for c in CASES]
I64, U32, P = ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p
PLAIN = [c for c in CASES if c.base.lut is None and c.base.max_freq == rc.NO_FILTER]


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("case", PLAIN, ids=[c.name for c in PLAIN])
def test_model_agrees_with_split_lines_and_the_oracle(case, oracle):
    base = case.base
    period = rh.PERIOD[base.fmt]
    lines = base.text.tobytes().split(b"\n")[:-1]                      # (what follows the last '\n' is no line)
    want = []
    for r in range(len(lines) // period):
        rec = lines[r * period:(r + 1) * period]
        seq = rec[1][:-1] if rec[1].endswith(b"\r") else rec[1]
        bases = np.frombuffer(seq, dtype=np.uint8)
        n = max(len(seq) - base.k + 1, 0)
        hits = 0
        if n:
            kmers = oracle.extract(bases, np.array([0, len(seq)], dtype=np.int64), base.k)
            inside = oracle.in_index(base.index, kmers)
            if base.revcomp:
                inside = inside | oracle.in_index(base.index, oracle.revcomp(kmers, base.k))
            hits = int(inside.sum())
        match = hits >= case.min_hits and 1000 * hits >= case.min_permille * n
        if match != case.invert:
            want.append(b"".join(x + b"\n" for x in rec))
    text, n_kept = rk.expected(case)[:2]
    assert text == b"".join(want) and n_kept == len(want)


def test_the_catalogue_is_not_vacuous():
    by_name = {c.name: c for c in CASES}
    mixed = [c for c in CASES if 0 < rk.expected(c)[1] < rk.expected(c)[6]]
    everything = [c for c in CASES if rk.expected(c)[1] == rk.expected(c)[6] > 1]
    nothing = [c for c in CASES if rk.expected(c)[1] == 0 and rk.expected(c)[6] > 1]
    assert mixed and everything and nothing
    for c in everything:                                               # all kept: the consumed bytes, verbatim
        assert rk.expected(c)[0] == c.base.text.tobytes()[:rk.expected(c)[5]]
    for c in nothing:
        assert rk.expected(c)[0] == b""
    default = lambda name: rk.expected(by_name[name + "__default"])[0]
    # invert, the permille rule and min_hits each change an output
    assert rk.expected(by_name["crlf_fasta_k16__invert"])[0] != default("crlf_fasta_k16")
    assert rk.expected(by_name["rk_permille_fastq_k31__permille_200"])[0] != default("rk_permille_fastq_k31")
    assert rk.expected(by_name["short_and_empty_fastq_k16__min_hits_0"])[0] != default("short_and_empty_fastq_k16")
    assert rk.expected(by_name["short_and_empty_fastq_k16__above_the_largest"])[0] != default("short_and_empty_fastq_k16")
    # kept and dropped together are every record once
    for name in ("crlf_fasta_k16", "rk_tile_ends_fastq_k31"):
        a, b = rk.expected(by_name[name + "__default"]), rk.expected(by_name[name + "__invert"])
        assert a[1] + b[1] == a[6] and not (a[2] & b[2]).any() and len(a[0]) + len(b[0]) == a[5]


def test_the_catalogue_holds_what_the_scatter_needs():
    by_name = {c.name: c for c in CASES}
    # kept runs that end at 15, 16 and 17 modulo 16 of the output; records alternately kept and dropped
    c = by_name["rk_output_residues_fasta_k31__default"]
    text, n_kept, keep = rk.expected(c)[:3]
    assert keep.tolist() == [True, False] * 9
    spans = rk.record_spans(c.base.text.tobytes(), c.base.fmt)
    ends = np.cumsum([b - a for (a, b), kp in zip(spans, keep) if kp])
    assert [int(e) % 16 for e in ends] == [15, 0, 1] * 3 and int(ends[-1]) == len(text)
    assert len({a % 16 for (a, b), kp in zip(spans, keep) if kp}) > 3  # (input and output out of step)
    # kept records that end one before, at and one behind a tile boundary of the input
    c = by_name["rk_tile_ends_fastq_k31__default"]
    keep = rk.expected(c)[2]
    spans = rk.record_spans(c.base.text.tobytes(), c.base.fmt)
    assert keep.tolist() == [False, True] * 3 + [False]
    assert [b % rk.TILE for (a, b), kp in zip(spans, keep) if kp] == [rk.TILE - 1, 0, 1]
    # a kept record across the super-tile seam, with dropped neighbours
    c = by_name["super_tile_fastq_k31__seam_record"]
    keep = rk.expected(c)[2]
    s = rk.seam_record(c.base)
    assert keep[s] and not keep[s - 1] and not keep[s + 1] and 0 < keep.sum() < keep.shape[0]
    # first dropped / last dropped / only the last kept
    assert rk.expected(by_name["rk_first_and_last_dropped_fastq_k31__default"])[2].tolist() == [False, True, False, True, False]
    assert rk.expected(by_name["rk_only_the_last_kept_fasta_k31__default"])[2].tolist() == [False, False, False, True]
    assert rk.expected(by_name["rk_first_kept_last_dropped_fasta_k31__default"])[2].tolist() == [True, True, False]
    # a single kept record shorter than 16 bytes
    assert rk.expected(by_name["rk_single_short_record_k1__invert"])[:2] == (b">\nA\n", 1)
    assert rk.expected(by_name["rk_single_short_record_k1__default"])[:2] == (b"", 0)
    assert rk.expected(by_name["rk_short_records_k1__default"])[:2] == (b">\nC\n", 1)
    # two records with equal hits and different windows, told apart by the permille rule alone
    c = by_name["rk_permille_fastq_k31__permille_200"]
    _, _, keep, hits, windows = rk.expected(c)[:5]
    assert hits[0] == hits[1] > 0 and windows[0] < windows[1] and keep.tolist() == [True, False, False]
    assert rk.expected(by_name["rk_permille_fastq_k31__default"])[2].tolist() == [True, True, False]
    # a break table that empties a read's windows: it matches at min_hits 0 only
    hits, windows = rk.expected(by_name["breaks_fastq_k16__default"])[3:5]
    no_windows = np.nonzero(windows == 0)[0]
    assert no_windows.size and not rk.expected(by_name["breaks_fastq_k16__default"])[2][no_windows].any()
    assert rk.expected(by_name["breaks_fastq_k16__min_hits_0"])[2][no_windows].all()
    assert rk.expected(by_name["short_and_empty_fastq_k16__permille_1000"])[2][rk.expected(by_name["short_and_empty_fastq_k16__default"])[4] == 0].all()
    # CRLF, a 3000-byte header, quality lines that start with '@' and '+', an incomplete last record: kept from the catalogue
    assert b"\r\n" in rk.expected(by_name["crlf_fastq_k31__default"])[0]
    assert b"x" * 3000 in rk.expected(by_name["long_header_fastq_k31__default"])[0]
    look = rk.expected(by_name["quality_lines_start_with_at_and_plus_k16__default"])[0].split(b"\n")
    assert {ln[:1] for ln in look[3::4] if ln} >= {b"@", b"+"}
    for name in ("incomplete_fastq_k31", "incomplete_fasta_k31"):
        c = by_name[name + "__default"]
        assert 0 < rk.expected(c)[5] < c.base.text.shape[0] and c.base.text.tobytes()[rk.expected(c)[5]:] not in rk.expected(c)[0]


def test_the_rule_in_64_bit_arithmetic():
    big = np.array([2 ** 32 - 1, 2 ** 32 - 1, 5_000_000], dtype=np.uint32)
    win = np.array([2 ** 32 - 1, 2 ** 32 - 2, 2 ** 32 - 1], dtype=np.uint32)
    assert rk.keep_rule(big, win, 2 ** 32 - 1, 1000).tolist() == [True, True, False]
    assert rk.keep_rule(big, win, 0, 1).tolist() == [True, True, True]
    assert rk.keep_rule(big, win, 0, 2).tolist() == [True, True, False]


# ---------------------------------------------------------------------------------------------- the plain-C++ helpers
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_keep")
    src = tmp / "shim.cpp"
    src.write_text('#include "record_keep_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.record_keep_cpu.argtypes = [P, I64, I64, U32, P, P, I64, U32, U32, U32, I64, P, I64, P]
    lib.record_keep_scatter_cpu.argtypes = [P, I64, P, I64, P, I64, P]
    return lib


def _run(lib, case, tail):
    text, n_kept, _, hits, windows, consumed, n_records = rk.expected(case)
    raw = case.base.text
    out = np.full(tail + len(text) + 64, 0xEE, dtype=np.uint8)
    stats = np.zeros(5, dtype=np.int64)
    hits, windows = np.ascontiguousarray(hits), np.ascontiguousarray(windows)
    lib.record_keep_cpu(raw.ctypes.data, raw.shape[0], consumed, rh.PERIOD[case.base.fmt].bit_length() - 1, hits.ctypes.data,
                        windows.ctypes.data, n_records, case.min_hits, case.min_permille, int(case.invert), tail, out.ctypes.data,
                        out.shape[0], stats.ctypes.data)
    return out, stats


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_helpers_agree_with_the_model(lib, case):
    text, n_kept = rk.expected(case)[:2]
    for tail in ((0, 1, 15, 16, 4097) if case.base.text.shape[0] < 100_000 else (5,)):
        out, stats = _run(lib, case, tail)
        assert stats.tolist() == [len(text), n_kept, 0, 0, 0], (tail, stats)
        assert out[tail:tail + len(text)].tobytes() == text
        assert (out[:tail] == 0xEE).all() and (out[tail + len(text):] == 0xEE).all()


def _random_lane_masks(n, seed):
    rng = np.random.default_rng(seed)
    masks = rng.integers(0, 1 << 16, size=(n + 15) // 16, dtype=np.uint16)
    masks[rng.integers(0, 4, size=masks.shape[0]) == 0] = 0           # (whole lanes without a kept byte, and full ones)
    masks[rng.integers(0, 8, size=masks.shape[0]) == 0] = 0xFFFF
    if n % 16:
        masks[-1] &= np.uint16((1 << (n % 16)) - 1)
    return masks


@pytest.mark.parametrize("case", [c for c in CASES if c.name.endswith("__default") and c.base.text.shape[0] < 100_000],
                         ids=lambda c: c.name)
def test_scatter_on_masks_no_text_produces(lib, case):
    raw = case.base.text
    n = raw.shape[0]
    for seed, tail in ((1, 0), (2, 7), (3, 16), (4, 1025)):
        masks = _random_lane_masks(n, seed)
        bits = ((masks[:, None] >> np.arange(16, dtype=np.uint16)) & 1).astype(bool).reshape(-1)[:n]
        want = raw[bits]
        out = np.full(tail + want.shape[0] + 64, 0xEE, dtype=np.uint8)
        stats = np.zeros(5, dtype=np.int64)
        lib.record_keep_scatter_cpu(raw.ctypes.data, n, masks.ctypes.data, tail, out.ctypes.data, out.shape[0], stats.ctypes.data)
        assert stats.tolist() == [want.shape[0], 0, 0, 0, 0], (seed, stats)     # (no destination outside [0, kept_total))
        assert np.array_equal(out[tail:tail + want.shape[0]], want)
        assert (out[:tail] == 0xEE).all() and (out[tail + want.shape[0]:] == 0xEE).all()


def test_helpers_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/record_keep_san_main.cpp; host code, nothing sanitized is
    loaded into Python): text, entries, masks and the output live in heap buffers of exactly their size."""
    exe = str(tmp_path / "record_keep_san")
    src = os.path.join(ROOT, "tests", "record_keep_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    t_path, e_path, m_path = str(tmp_path / "text.bin"), str(tmp_path / "entries.bin"), str(tmp_path / "masks.bin")
    for case in CASES:
        text, n_kept, _, hits, windows, consumed, _ = rk.expected(case)
        case.base.text.tofile(t_path)
        np.concatenate([hits, windows]).astype(np.uint32).tofile(e_path)
        shift = str(rh.PERIOD[case.base.fmt].bit_length() - 1)
        rule = [str(case.min_hits), str(case.min_permille), str(int(case.invert))]
        runs = [([], tail) for tail in ((0, 13) if case.base.text.shape[0] < 100_000 else (3,))]
        if case.name.endswith("__default"):
            _random_lane_masks(case.base.text.shape[0], 5).tofile(m_path)
            runs.append(([m_path], 9))
        for extra, tail in runs:
            r = subprocess.run([exe, t_path, e_path, shift] + rule + [str(tail)] + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (case.name, r.stdout, r.stderr[-2000:])
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            got = r.stdout.split()
            assert got[0] == "ok" and got[5:] == ["0", "0", "0"], (case.name, r.stdout)
            if not extra:
                assert got[1:5] == [str(case.base.text.shape[0]), str(consumed), str(len(text)), str(n_kept)]


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    batch = ReadBatch.from_strings(["ACGTACGTAC", "GGGTTTAAAC"])
    sam, bam, fq = str(tmp_path / "r.sam"), str(tmp_path / "r.bam"), str(tmp_path / "r.fq")
    reads_io.write_sam(sam, batch)
    reads_io.write_bam(bam, batch)
    reads_io.write_fastq(fq, batch)
    return sam, bam, fq


def test_select_reads_refusals_come_before_the_index_is_read(tmp_path, monkeypatch):
    """Refused with ValueError before the index file is read (there is none), and before -o is created."""
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    sam, bam, fq = _files(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = str(tmp_path / "kept.fq")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5"]
    for path, what in ((sam, "SAM"), (bam, "BAM")):
        with pytest.raises(ValueError, match="select-reads does not read %s files.*name" % what):
            run_argument_parser(common + ["-f", path, "-o", out])
    before = open(fq, "rb").read()
    for same in (fq, os.path.join(str(tmp_path), ".", "r.fq")):
        with pytest.raises(ValueError, match="is the input file"):
            run_argument_parser(common + ["-f", fq, "-o", same])
    assert open(fq, "rb").read() == before
    for bad in (["--min-hit-permille", "1001"], ["--min-hit-permille", "-1"], ["--min-hits", "-1"]):
        with pytest.raises(ValueError, match="min-hit"):
            run_argument_parser(common + ["-f", fq, "-o", out] + bad)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
        run_argument_parser(common + ["-f", fq, "-o", out])
    assert not os.path.exists(out)


def test_select_reads_defaults_and_the_other_commands_parse_as_before():
    from kmer_mapper_amd.command_line_interface import build_argument_parser, map_bnp, read_hits_file, select_reads_file
    parser = build_argument_parser()
    a = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.fq.gz", "-o", "kept.fq"])
    assert vars(a) == dict(kmer_index="x.npz", index_bundle=None, reads="r.fq.gz", kmer_size=31, chunk_size=2500000, output_file="kept.fq",
                           min_hits=1, min_hit_permille=0, invert=False, max_hits_per_kmer=1000, map_reverse_complements=False,
                           ambiguous_bases="a", hits_output=None, device=0, debug=None, func=select_reads_file)
    b = parser.parse_args(["select-reads", "-i", "x.npz", "-f", "r.fq", "-k", "31", "-o", "kept.fq", "--min-hits", "3", "--min-hit-permille",
                           "250", "--invert", "-r", "True", "-I", "1000", "--ambiguous-bases", "skip", "--hits-output", "out"])
    assert (b.min_hits, b.min_hit_permille, b.invert, b.map_reverse_complements, b.ambiguous_bases, b.hits_output) == \
        (3, 250, True, True, "skip", "out")
    new = {"min_hit_permille", "invert", "hits_output"}
    r = parser.parse_args(["read-hits", "-i", "x.npz", "-f", "r.fq", "-o", "o"])
    assert r.func is read_hits_file and not new & set(vars(r))
    assert vars(r) == dict(kmer_index="x.npz", index_bundle=None, reads="r.fq", kmer_size=31, chunk_size=2500000, output_file="o",
                           max_hits_per_kmer=1000, map_reverse_complements=False, ambiguous_bases="a", windows=False, min_hits=1, device=0,
                           debug=None, func=read_hits_file, device_parser=False, exclude_flags=0, include_flags=0, min_mapq=0,
                           regions=None, regions_file=None, original_strand=False)
    m = parser.parse_args(["map", "-i", "x.npz", "-f", "r.fq", "-o", "o"])
    assert m.func is map_bnp and not (new | {"min_hits"}) & set(vars(m))
    assert (m.kmer_size, m.n_threads, m.chunk_size, m.max_hits_per_kmer, m.map_reverse_complements, m.ambiguous_bases, m.host_parser) == \
        (31, 16, 2500000, 1000, False, "a", False)
