"""CPU tier of the record-hits mode (include/kmm.h).  The catalogue's parser + model (tests/record_hits_cases.py)
against a second route — the oracle's extract -> in_index -> per-read sum, on reads cut out of the text by line arithmetic —
and the conditions that keep the catalogue from being vacuous; the line -> record and run-folding arithmetic of
csrc/kmm_read_hits.hpp compiled with g++ against brute force on every case's bytes (once more under ASan + UBSan as a
stand-alone executable); the command line's new refusals and its unchanged defaults."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = rh.all_cases()
IDS = [c.name for c in CASES]
I64 = ctypes.c_int64


# ---------------------------------------------------------------------------------------------- parser + model
def _reads_by_line_arithmetic(case):
    """The second route to the reads: numpy over the bytes — a byte is a base iff its line number mod the period is 1 and it is
    no terminator — independent of the parser's string splitting."""
    text = case.text
    period = rh.PERIOD[case.fmt]
    nl = text == 10
    n_lines = int(nl.sum())
    n_records = n_lines // period
    if n_records == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64), 0, 0
    consumed = int(np.nonzero(nl)[0][n_records * period - 1]) + 1
    line = np.concatenate([[0], np.cumsum(nl)[:-1]])[:consumed]
    head = text[:consumed]
    base = ((line % period) == 1) & (head != 10) & (head != 13)
    lens = np.bincount((line // period)[base], minlength=n_records)
    return head[base], np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), consumed, n_records


def _per_read(values, offsets, k):
    n = np.maximum(np.diff(offsets) - k + 1, 0)
    ends = np.cumsum(n)
    cs = np.concatenate([[0], np.cumsum(values.astype(np.int64))])
    return (cs[ends] - cs[ends - n]).astype(np.uint32), n.astype(np.uint32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_parser_agrees_with_line_arithmetic(case):
    reads, consumed, n_records = rh.parse(case.text, case.fmt)
    bases, offsets, want_consumed, want_records = _reads_by_line_arithmetic(case)
    got_bases, got_offsets = rh.reads_arrays(reads)
    assert (consumed, n_records) == (want_consumed, want_records) and n_records > 0
    assert np.array_equal(got_offsets, offsets) and np.array_equal(got_bases, bases)
    if case.name.startswith("incomplete_"):
        assert 0 < consumed < case.text.shape[0]
    else:
        assert consumed == case.text.shape[0]


@pytest.mark.parametrize("case", [c for c in CASES if c.lut is None], ids=[c.name for c in CASES if c.lut is None])
def test_parser_and_model_agree_with_extract_then_in_index(case, oracle):
    plain = case._replace(max_freq=rc.NO_FILTER, revcomp=False)
    hits, windows = rh.run_model(plain)
    bases, offsets, _, _ = _reads_by_line_arithmetic(case)
    kmers = oracle.extract(bases, offsets, case.k)
    want_hits, want_windows = _per_read(oracle.in_index(case.index, kmers), offsets, case.k)
    assert np.array_equal(windows, want_windows) and np.array_equal(hits, want_hits)
    if case.revcomp:
        hits, windows = rh.run_model(case._replace(max_freq=rc.NO_FILTER))
        either = oracle.in_index(case.index, kmers) | oracle.in_index(case.index, oracle.revcomp(kmers, case.k))
        want_hits, _ = _per_read(either, offsets, case.k)
        assert np.array_equal(hits, want_hits) and np.array_equal(windows, want_windows)


@pytest.mark.parametrize("case", [c for c in CASES if c.rule is not None], ids=[c.name for c in CASES if c.rule is not None])
def test_every_rule_changes_something(case):
    hits, windows = rh.expected(case)[:2]
    plain = case._replace(max_freq=rc.NO_FILTER if case.rule == "filter" else case.max_freq,
                          revcomp=False if case.rule == "revcomp" else case.revcomp, lut=None if case.rule == "break" else case.lut)
    h0, w0 = rh.run_model(plain)
    assert not (np.array_equal(h0, hits) and np.array_equal(w0, windows))
    if case.rule == "break":
        assert (windows < w0).any() and (windows <= w0).all()
    elif case.rule == "revcomp":
        assert (hits[(h0 == 0)] > 0).any(), "a read that hits only in the other orientation"
        if case.k == 16:
            assert (b"ACGT" * 12) in case.text.tobytes(), "the palindrome"


def test_the_catalogue_is_not_vacuous():
    some, none, no_windows, two_records = 0, 0, 0, 0
    for case in CASES:
        hits, windows = rh.expected(case)[:2]
        assert (hits <= windows).all()
        some += int(((hits > 0) & (hits < windows)).sum())
        none += int(((hits == 0) & (windows > 0)).sum())
        no_windows += int((windows == 0).sum())
        two_records += rh.lanes_that_hold_two_records(case)
    assert some > 0, "a read with 0 < hits < windows"
    assert none > 0, "a read with hits == 0 < windows"
    assert no_windows > 0, "a read with windows == 0"
    assert two_records > 0, "a lane that holds two records"


def test_the_catalogue_holds_what_the_seams_need():
    by_name = {c.name: c for c in CASES}
    for fmt, k in ((rh.FASTQ, 31), (rh.FASTA, 31)):
        text, ends = rh.seam_text(fmt, k)
        assert {(u, d) for u, d, _ in ends} == {(u, d) for u in rh.SEAM_UNITS for d in (-1, 0, 1)}
        for unit, d, e in ends:
            assert text[e:e + 1] == b"\n" and (e - d) % unit == 0
        lines = text.split(b"\n")
        seq_ends = set(np.cumsum([len(x) + 1 for x in lines[:-1]])[1::rh.PERIOD[fmt]] - 1)
        assert {e for _, _, e in ends} == seq_ends                   # every one of them ends a sequence line
        assert by_name["seams_%s_k%d" % (fmt, k)].text.tobytes().startswith(text)
    big = by_name["super_tile_fastq_k31"]
    assert rh.SUPER < big.text.shape[0] < rh.SUPER + (1 << 15)
    assert big.text[rh.SUPER + 1] == 10 and not (big.text[rh.SUPER + 1 - 200:rh.SUPER + 1] == 10).any()
    line = int((big.text[:rh.SUPER + 1] == 10).sum())
    assert line % 4 == 1                                             # ... of a sequence line that crosses the super-tile seam
    assert max(c.text.shape[0] for c in CASES if c is not big) < 8192
    tiny = by_name["tiny_fasta_k1"].text.tobytes()
    assert tiny.startswith(b">\nA\n>\nC\n>\n\n>\nCC\n")
    assert b"x" * 3000 in by_name["long_header_fastq_k31"].text.tobytes()
    look = by_name["quality_lines_start_with_at_and_plus_k16"].text.tobytes().split(b"\n")
    assert {ln[:1] for ln in look[3::4] if ln} >= {b"@", b"+"}
    assert b"\r\n" in by_name["crlf_fastq_k31"].text.tobytes() and b"\r\n\r\n" in by_name["crlf_fasta_k16"].text.tobytes()
    brk = by_name["breaks_fastq_k16"].text
    at = np.nonzero((brk == ord("N")) | (brk == ord("n")))[0]
    assert any(p % rh.TILE == rh.TILE - 1 for p in at) and any(p % rh.TILE == 1 for p in at)


# ---------------------------------------------------------------------------------------------- line -> record, run folding
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_hits")
    src = tmp / "shim.cpp"
    src.write_text('#include "record_hits_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.record_hits_fold_cpu.argtypes = [ctypes.c_void_p, I64, ctypes.c_void_p, ctypes.c_uint32, I64, I64, ctypes.c_void_p, ctypes.c_void_p]
    lib.record_hits_fold_cpu.restype = I64
    return lib


def _window_masks(case, consumed, seed):
    """Two mask sets over the consumed bytes (bit 0 a window, bit 1 a hit): the windows the records really have, with random
    hits; and windows at random bytes of any line — runs of two and more records inside one lane, which no well-formed text
    produces at this lane length."""
    text = case.text[:consumed]
    period = rh.PERIOD[case.fmt]
    line = np.concatenate([[0], np.cumsum(text == 10)[:-1]])
    base = ((line % period) == 1) & (text != 10) & (text != 13)
    gaps = np.cumsum(~base)
    real = np.zeros(consumed, dtype=np.uint8)
    n = consumed - case.k + 1
    if n > 0:
        real[:n] = base[:n] & (gaps[case.k - 1:] == gaps[:n])
    rng = np.random.default_rng(seed)
    real |= (rng.integers(0, 2, size=consumed, dtype=np.uint8) << 1)
    anywhere = rng.integers(0, 4, size=consumed, dtype=np.uint8)
    return real, anywhere


def _brute(text, masks, period, n_records):
    rec = np.concatenate([[0], np.cumsum(text == 10)[:-1]]) // period
    win = (masks & 1).astype(bool)
    hit = win & ((masks >> 1) & 1).astype(bool)
    return (np.bincount(rec[hit], minlength=n_records).astype(np.uint32), np.bincount(rec[win], minlength=n_records).astype(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fold_agrees_with_brute_force(lib, case):
    _, _, consumed, n_records = rh.expected(case)
    period = rh.PERIOD[case.fmt]
    text = np.ascontiguousarray(case.text[:consumed])
    for i, masks in enumerate(_window_masks(case, consumed, 7)):
        want_h, want_w = _brute(text, masks, period, n_records)
        assert want_w.any()
        for lane in ((4, 1, 16) if consumed < 100_000 else (4,)):
            hits, windows = np.zeros(n_records, np.uint32), np.zeros(n_records, np.uint32)
            outside = lib.record_hits_fold_cpu(text.ctypes.data, consumed, masks.ctypes.data, period.bit_length() - 1, lane, n_records,
                                               hits.ctypes.data, windows.ctypes.data)
            assert outside == 0
            assert np.array_equal(windows, want_w) and np.array_equal(hits, want_h), (i, lane)


def test_fold_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/record_hits_san_main.cpp; host code, nothing sanitized is
    loaded into Python): text, masks and entries live in heap buffers of exactly their size."""
    exe = str(tmp_path / "record_hits_san")
    src = os.path.join(ROOT, "tests", "record_hits_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    t_path, m_path = str(tmp_path / "text.bin"), str(tmp_path / "masks.bin")
    for case in CASES:
        _, _, consumed, n_records = rh.expected(case)
        case.text[:consumed].tofile(t_path)
        for masks in _window_masks(case, consumed, 11):
            masks.tofile(m_path)
            for lane in ((4, 1) if consumed < 100_000 else (4,)):
                r = subprocess.run([exe, t_path, m_path, str(rh.PERIOD[case.fmt].bit_length() - 1), str(lane)], capture_output=True,
                                   text=True, timeout=300)
                assert r.returncode == 0, (case.name, r.stdout, r.stderr[-2000:])
                assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
                assert r.stdout.split() == ["ok", str(consumed), str(n_records), "0", "0"]


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


SELECTION = (["--exclude-flags", "0x900"], ["--include-flags", "4"], ["--min-mapq", "20"], ["--regions", "chr1:1-100"],
             ["--regions-file", "regions.bed"], ["--original-strand"])


def test_selection_options_need_the_device_parser_and_sam_or_bam(tmp_path, monkeypatch):
    """Refused with ValueError before the index file is read (there is none)."""
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    sam, bam, fq = _files(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    common = ["read-hits", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", str(tmp_path / "o")]
    for option in SELECTION:
        for path in (sam, bam, fq):
            with pytest.raises(ValueError, match="%s needs --device-parser" % option[0]):
                run_argument_parser(common + ["-f", path] + option)
        with pytest.raises(ValueError, match="%s applies to SAM and BAM input only" % option[0]):
            run_argument_parser(common + ["-f", fq, "--device-parser"] + option)
    assert not os.path.exists(str(tmp_path / "o.npy"))


def test_several_ranks_stay_refused_with_and_without_the_flag(tmp_path, monkeypatch):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    sam, bam, fq = _files(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    for path in (fq, bam):
        for flag in ([], ["--device-parser"]):
            if path == bam and not flag:
                continue                                               # (refused as BAM first: the existing test pins that wording)
            with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
                run_argument_parser(["read-hits", "-i", str(tmp_path / "none.npz"), "-f", path, "-k", "5", "-o", str(tmp_path / "o")] + flag)


def test_read_hits_without_the_flag_parses_to_the_same_defaults():
    from kmer_mapper_amd.command_line_interface import build_argument_parser, read_hits_file
    a = build_argument_parser().parse_args(["read-hits", "-i", "x.npz", "-f", "r.fq", "-o", "o"])
    before = dict(kmer_index="x.npz", index_bundle=None, reads="r.fq", kmer_size=31, chunk_size=2500000, output_file="o",
                  max_hits_per_kmer=1000, map_reverse_complements=False, ambiguous_bases="a", windows=False, min_hits=1, device=0,
                  debug=None, func=read_hits_file)
    new = dict(device_parser=False, exclude_flags=0, include_flags=0, min_mapq=0, regions=None, regions_file=None, original_strand=False)
    assert vars(a) == {**before, **new}
    b = build_argument_parser().parse_args(["read-hits", "-i", "x.npz", "-f", "r.bam", "-o", "o", "--device-parser", "--include-flags", "4",
                                            "--min-mapq", "3", "--regions", "chr1", "--original-strand", "--exclude-flags", "0x900"])
    assert (b.device_parser, b.include_flags, b.min_mapq, b.regions, b.original_strand, b.exclude_flags) == (True, 4, 3, ["chr1"], True, 0x900)
