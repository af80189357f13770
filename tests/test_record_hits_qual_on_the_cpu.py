"""CPU tier of the base-quality floor of the record-hits mode: tests/record_hits_qual_cases.py held to the
conditions its cases exist for; the plain-C++ arithmetic of csrc/kmm_rh_qual.hpp — compiled by itself with g++ — against the
Python model on the catalogue's texts (once more under ASan + UBSan, as a program of its own); the command line up to the first
HIP call."""
import ctypes
import logging
import os
import subprocess

import numpy as np
import pytest

from tests import quality_cases as qc
from tests import read_hits_cases as rc
from tests import record_hits_qual_cases as qh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = qh.all_cases()
IDS = [c.name for c in CASES]
I64 = ctypes.c_int64


# ---------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_case_differs_from_the_floor_off_model(case):
    on, off = qh.expected(case), qh.expected(case, 0)
    assert (on.consumed, on.n_records) == (off.consumed, off.n_records) == (case.text.shape[0], len(on.recs))
    assert on.masked > 0 and off.masked == 0
    assert (on.windows != off.windows).any() and (on.windows <= off.windows).all() and (on.hits <= off.hits).all()
    assert (on.hits < off.hits).any()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_model_counts_the_surviving_windows(case):
    """The windows of the model (a low base as a break byte) are quality_cases.surviving_windows under the same mask."""
    e = qh.expected(case)
    bases, offsets, mask = qh.reads_under_floor([r.seq for r in e.recs], [r.qual for r in e.recs], case.q)
    if case.lut is not None:
        mask = mask | (np.asarray(case.lut)[bases] == rc.LUT_BREAK)
    alive = qc.surviving_windows(offsets, case.k, mask)
    want = np.bincount(np.searchsorted(offsets, alive, side="right") - 1, minlength=offsets.shape[0] - 1)
    assert np.array_equal(e.windows, want.astype(np.uint32))


def test_seam_cases_have_the_quality_byte_and_the_base_in_different_units():
    seen = set()
    for case in CASES:
        for base_at, qual_at, unit in case.marks:
            assert base_at // unit != qual_at // unit, (case.name, base_at, qual_at, unit)
            assert case.text[qual_at] < 33 + case.q and chr(case.text[base_at]) in "ACGT"
            recs = [r for r in qh.expected(case).recs if r.seq_at <= base_at < r.seq_at + len(r.seq)]
            assert len(recs) == 1 and base_at - recs[0].seq_at == qual_at - recs[0].qual_at
            if "base_last" in case.name or case.name == "super_tile":
                seen.add((unit, "base_last", base_at % unit == unit - 1))
            if "qual_first" in case.name:
                seen.add((unit, "qual_first", qual_at % unit == 0))
    for unit in qh.SEAM_UNITS:
        assert (unit, "base_last", True) in seen and (unit, "qual_first", True) in seen
    assert (qh.SUPER, "base_last", True) in seen
    big = qh.by_name("super_tile")
    assert qh.SUPER < big.text.shape[0] < qh.SUPER + 8192                           # one text just over 1 MiB, the rest a few KB
    assert all(c.text.shape[0] < 64 << 10 for c in CASES if c is not big)
    for case in CASES:                                                              # the pair shifted by a long '+' line and a long header
        if case.name.startswith("seam_"):
            gaps = sorted(q - b for b, q, _ in case.marks)
            assert gaps[0] == qh.L + 3 and gaps[-1] > qh.L + 300 and any(r.seq_at - r.start > 2000 for r in qh.expected(case).recs)


def test_masked_base_cases_have_windows_on_both_sides():
    case = qh.by_name("positions")
    e = qh.expected(case)
    k = case.k
    both = 0
    for r, w in zip(e.recs, e.windows):
        low = np.flatnonzero(np.frombuffer(r.qual, dtype=np.uint8) < 33 + case.q)
        for p in low:
            left = p >= k and not ((low >= p - k) & (low < p)).any()
            right = p + k < len(r.seq) and not ((low > p) & (low <= p + k)).any()
            both += bool(left and right)
    assert both >= 3
    lows = [set(np.flatnonzero(np.frombuffer(r.qual, dtype=np.uint8) < 53)) for r in e.recs]
    assert any(0 in s for s in lows) and any(qh.L - 1 in s for s in lows) and any(k - 1 in s for s in lows)
    assert any(qh.L - k in s for s in lows) and any(set(range(50, 90)) <= s for s in lows)
    assert any({40, 40 + k} <= s for s in lows) and any({40, 40 + k + 1} <= s for s in lows)
    assert any(0 < len(r.seq) < k for r in e.recs) and any(len(r.seq) == 0 for r in e.recs)
    for q in (1, 20, 93):                                                           # 33 + Q - 1 and 33 + Q side by side
        text = qh.by_name("values_q%d" % q).text.tobytes()
        assert bytes([33 + q - 1, 33 + q]) in text and bytes([33 + q, 33 + q - 1]) in text
    odd = next(r for r in qh.expected(qh.by_name("values_q20")).recs if 0x80 in r.qual)
    assert 0x20 in odd.qual and 0xFF in odd.qual and qc.low_mask(np.frombuffer(odd.qual, np.uint8), 20)[[40, 75, 76, 110]].tolist() == \
        [True, False, False, True]
    crlf = qh.expected(qh.by_name("crlf_lookalikes")).recs
    assert b"\r\n" in qh.by_name("crlf_lookalikes").text.tobytes() and {r.qual[:1] for r in crlf} == {b"@", b"+"}
    starts = qh.piece_starts(qh.by_name("pieces").text.tobytes())
    recs = qh.expected(qh.by_name("pieces")).recs
    assert len(starts) >= 5 and all(recs[i].qual[0] < 53 for i in starts)


@pytest.mark.parametrize("name", ["keep_min_hits", "keep_min_permille", "pairs_any", "pairs_both"])
def test_keep_cases_keep_some_and_differ_from_the_floor_off_set(name):
    case = qh.by_name(name)
    on, text = qh.kept(case)
    off, _ = qh.kept(case, 0)
    assert 0 < on.sum() < on.shape[0] and (on != off).any()
    assert len(text) == sum(r.end - r.start for r, k in zip(qh.expected(case).recs, on) if k)


def test_the_bam_case_would_lose_hits_if_absent_qualities_were_masked():
    recs = qh.bam_records()
    h, w, masked, no_qual, texts = qh.bam_expected(recs, 20)
    names, seqs, named_quals, exempt = qh.bam_reads(recs, absent=b'"')
    h_masked, w_masked, _ = qh.model(rc.genome_index(qh.K), qh.K, seqs, named_quals, 20)          # no exemption
    assert no_qual == len(exempt) == 3 and h[exempt].sum() > 0 and h_masked[exempt].sum() == 0 and w_masked[exempt].sum() == 0
    assert any(r.flag & 0x10 for r in recs) and any(r.flag & 0x400 for r in recs) and any(len(r.seq) == 0 for r in recs)
    assert len(names) == len(recs) - 2 and masked > 0
    text, seqs, quals, exempt = qh.sam_case()
    assert len(exempt) == 2 and text.tobytes().count(b"\t*\n") == 2


def test_the_malformed_cases_name_the_quality_lines_newline():
    for case, at in qh.malformed_cases():
        recs, _ = qh.parse_q(case.text)
        assert qh.first_malformed(recs) == at and case.text[at] == 10
        bad = next(r for r in recs if len(r.seq) != len(r.qual))
        assert abs(len(bad.seq) - len(bad.qual)) == 1 and bad.qual_nl == at


# ---------------------------------------------------------------------------------------------- the arithmetic of the mark pass
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("record_hits_qual")
    src = tmp / "shim.cpp"
    src.write_text('#include "record_hits_qual_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.rq_mark_cpu.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    lib.rq_mark_cpu.restype = None
    return lib


def _mark(lib, text, limit, n_records, q, exempt=None):
    text = np.ascontiguousarray(text)
    line_start = np.zeros(max(4 * n_records, 1), dtype=np.uint32)
    dead = np.zeros((limit + 31) // 32 + 1, dtype=np.uint32)
    out = np.zeros(4, dtype=np.int64)
    lib.rq_mark_cpu(text.ctypes.data, limit, 4 * n_records, 33 + q, None if exempt is None else exempt.ctypes.data, 0,
                    line_start.ctypes.data, dead.ctypes.data, dead.shape[0], out.ctypes.data)
    bits = np.flatnonzero(np.unpackbits(dead.view(np.uint8), bitorder="little"))
    return bits, out, line_start


def _dead_offsets(recs, q, exempt=()):
    want = []
    for i, r in enumerate(recs):
        if i not in exempt:
            want += [r.seq_at + int(j) for j in np.flatnonzero(np.frombuffer(r.qual, dtype=np.uint8) < 33 + q) if j < len(r.seq)]
    return np.array(sorted(want), dtype=np.int64)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_mark_pass_agrees_with_the_model(lib, case):
    e = qh.expected(case)
    bits, out, line_start = _mark(lib, case.text, e.consumed, e.n_records, case.q)
    assert out.tolist() == [e.masked, -1, 0, 0]
    assert np.array_equal(bits, _dead_offsets(e.recs, case.q))
    assert np.array_equal(line_start[3::4], [r.qual_at for r in e.recs]) and np.array_equal(line_start[1::4], [r.seq_at for r in e.recs])
    cut = e.recs[len(e.recs) // 2].qual_at + 5                                      # a chunk that ends inside a quality line
    recs, consumed = qh.parse_q(case.text[:cut])
    bits, out, _ = _mark(lib, case.text[:cut], consumed, len(recs), case.q)
    assert out[1:].tolist() == [-1, 0, 0] and np.array_equal(bits, _dead_offsets(recs, case.q))


def test_mark_pass_reports_the_length_rule_and_honours_the_exemption(lib):
    for case, at in qh.malformed_cases():
        recs, consumed = qh.parse_q(case.text)
        _, out, _ = _mark(lib, case.text, consumed, len(recs), case.q)
        assert out[1] == at and out[2] == 0 and out[3] == 0
    bam = qh.bam_records()
    h, w, masked, no_qual, texts = qh.bam_expected(bam, 20)
    exempt_recs = qh.bam_reads(bam)[3]
    text = np.frombuffer(b"".join(texts), dtype=np.uint8)
    recs, consumed = qh.parse_q(text)
    flags = np.zeros(consumed // 32 + 2, dtype=np.uint32)
    for i in exempt_recs:
        flags[recs[i].qual_at >> 5] |= np.uint32(1 << (recs[i].qual_at & 31))
    bits, out, _ = _mark(lib, text, consumed, len(recs), 20, flags)
    assert out.tolist() == [masked, -1, 0, 0] and np.array_equal(bits, _dead_offsets(recs, 20, exempt_recs))
    bits, out, _ = _mark(lib, text, consumed, len(recs), 20)                        # without the flags '"' is below the floor
    assert out[0] == masked + sum(len(recs[i].seq) for i in exempt_recs)


def test_mark_pass_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/record_hits_qual_san_main.cpp; host code, nothing sanitized is
    loaded into Python): the text, the line starts and the bitset live in heap buffers of exactly their size."""
    exe = str(tmp_path / "record_hits_qual_san")
    src = os.path.join(ROOT, "tests", "record_hits_qual_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    path = str(tmp_path / "text.bin")
    runs = [(c, qh.expected(c).consumed, qh.expected(c).n_records, qh.expected(c).masked, -1) for c in CASES]
    for case, at in qh.malformed_cases():
        recs, consumed = qh.parse_q(case.text)
        runs.append((case, consumed, len(recs), None, at))
    for case, consumed, n_records, masked, at in runs:
        case.text.tofile(path)
        for limit, lines in ((consumed, 4 * n_records), (consumed, 4 * n_records - 4)):   # (fewer lines than the text holds: no entry read)
            r = subprocess.run([exe, path, str(limit), str(max(lines, 0)), str(33 + case.q)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (case.name, r.stdout, r.stderr[-2000:])
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            got = r.stdout.split()
            assert got[0] == "ok" and got[3:5] == ["0", "0"]
            if lines == 4 * n_records:
                assert int(got[2]) == at and (masked is None or (int(got[1]), int(got[5])) == (masked, masked))


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    batch = ReadBatch.from_strings(["ACGTACGTAC", "GGGTTTAAAC"])
    sam, bam, fq, fa = (str(tmp_path / n) for n in ("r.sam", "r.bam", "r.fq", "r.fa"))
    reads_io.write_sam(sam, batch)
    reads_io.write_bam(bam, batch)
    reads_io.write_fastq(fq, batch)
    reads_io.write_fasta(fa, batch)
    return sam, bam, fq, fa


def test_the_flags_parse():
    from kmer_mapper_amd.command_line_interface import build_argument_parser
    p = build_argument_parser()
    a = p.parse_args(["read-hits", "-i", "x.npz", "-f", "r.fq", "-o", "o", "--min-base-quality", "20", "--use-record-qual"])
    assert (a.min_base_quality, a.use_record_qual) == (20, True)
    b = p.parse_args(["select-reads", "-i", "x.npz", "-f", "r.bam", "-o", "o", "--bam-to-fastq", "--min-base-quality", "7", "--use-record-qual"])
    assert (b.min_base_quality, b.use_record_qual) == (7, True)
    for sub in ("read-hits", "select-reads"):                                       # without them: the defaults of before
        c = p.parse_args([sub, "-i", "x.npz", "-f", "r.fq", "-o", "o"])
        assert not hasattr(c, "min_base_quality") and not hasattr(c, "use_record_qual")


def test_the_refusals_fire_before_the_index_is_read(tmp_path, monkeypatch, capsys):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    sam, bam, fq, fa = _files(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    none, out = str(tmp_path / "none.npz"), str(tmp_path / "o")
    for sub, more in (("read-hits", []), ("select-reads", [])):
        with pytest.raises(SystemExit):                                             # k = 1: the parser's error, as `map`
            run_argument_parser([sub, "-i", none, "-f", fq, "-o", out, "-k", "1", "--min-base-quality", "20"] + more)
        assert "--min-base-quality needs -k 2 or more" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            run_argument_parser([sub, "-i", none, "-f", fq, "-o", out, "-k", "5", "--min-base-quality", "94"])
        assert "--min-base-quality must lie in 0 .. 93" in capsys.readouterr().err
        with pytest.raises(ValueError, match="--use-record-qual applies to SAM and BAM input only"):
            run_argument_parser([sub, "-i", none, "-f", fq, "-o", out, "-k", "5", "--min-base-quality", "20", "--use-record-qual"])
    for path in (sam, bam):                                                         # SAM / BAM need the second flag
        with pytest.raises(ValueError, match="--min-base-quality applies to FASTQ input.*--use-record-qual"):
            run_argument_parser(["read-hits", "-i", none, "-f", path, "-o", out, "-k", "5", "--min-base-quality", "20"])
    with pytest.raises(ValueError, match="--min-base-quality applies to FASTQ input.*--use-record-qual"):
        run_argument_parser(["select-reads", "-i", none, "-f", bam, "-o", out, "-k", "5", "--bam-to-fastq", "--min-base-quality", "20"])
    for extra in ([], ["--use-record-qual"]):
        with pytest.raises(ValueError, match="--sam-out does not go with --min-base-quality"):
            run_argument_parser(["select-reads", "-i", none, "-f", sam, "-o", out, "-k", "5", "--sam-out", "--min-base-quality", "20"] + extra)
    assert not os.path.exists(out) and not os.path.exists(out + ".npy")


@pytest.mark.parametrize("sub", ["read-hits", "select-reads"])
def test_fasta_is_warned_about_and_served(tmp_path, monkeypatch, caplog, sub):
    """FASTA has no qualities: one warning, then the command goes on — here to the index file, which does not exist."""
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    fa = _files(tmp_path)[3]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with caplog.at_level(logging.INFO):
        with pytest.raises(Exception) as exc:
            run_argument_parser([sub, "-i", str(tmp_path / "none.npz"), "-f", fa, "-o", str(tmp_path / "o"), "-k", "5",
                                 "--min-base-quality", "20"])
    assert "min-base-quality" not in str(exc.value) and not isinstance(exc.value, SystemExit)
    assert "--min-base-quality 20 has no effect on FASTA input" in caplog.text
    if sub == "read-hits":
        assert "--min-base-quality implies --device-parser" in caplog.text
