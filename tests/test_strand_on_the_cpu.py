"""CPU tier of "original_strand" (include/kmm.h): the decode of csrc/kmm_bam.hpp and the write pass of
csrc/kmm_sam.hpp, plain and quality variants, compiled by themselves with g++ (tests/strand_cpu_driver.hpp) and driven in windows
with a carry.  The records are made in read orientation and stored the way an aligner stores them (tests/strand_cases.py): with
the switch on the text has to be the reads', with it off the stored text, byte for byte; the per-record functions run with 1 and
with 64 lanes; once more under AddressSanitizer + UndefinedBehaviorSanitizer with every output in an exact-size heap buffer.
Also: the command line's --original-strand up to the first HIP call."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import strand_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
VARIANTS = list(itertools.product((0, 1), (0, 1), (1, 64)))      # (quality variant, switch, lanes)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("strand")
    src = tmp / "shim.cpp"
    src.write_text('#include "strand_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    for fn in (lib.strand_bam_cpu, lib.strand_sam_cpu):
        fn.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, ctypes.c_int,
                       ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    for fn in (lib.strand_comp_letter, lib.strand_comp_code_letter):
        fn.argtypes, fn.restype = [ctypes.c_uint32], ctypes.c_uint32
    return lib


def _run(fn, data, cuts=(), excl=0, qual=0, orig=0, lanes=1):
    """(rc, text, records, excluded, records without qualities, records flipped)"""
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out = np.zeros(3 * len(data) + 64, np.uint8)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 6)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = fn(data, len(data), c, len(cuts), excl, qual, orig, lanes, out.ctypes.data, len(out), ctypes.byref(on), st)
    return rc, out[:on.value].tobytes(), st[0], st[1], st[3], st[4]


def _both(lib, records, cuts_bam=((),), cuts_sam=((),), excl=0, crlf=False, variants=VARIANTS, bam_upper=True):
    """Every variant on the records as BAM and as SAM: byte-exact text, records, flips."""
    bam, sam = sc.bam_payload(records), sc.sam_bytes(records, crlf=crlf)
    kept = sum(1 for f, _, _ in records if not f & excl)
    for qual, orig, lanes in variants:
        n_flip = sc.n_flipped(records, excl) if orig else 0
        for fn, data, all_cuts, upper in ((lib.strand_bam_cpu, bam, cuts_bam, bam_upper), (lib.strand_sam_cpu, sam, cuts_sam, False)):
            want = sc.text(records, orig, qual, excl, upper)
            for cuts in all_cuts:
                rc, out, recs, excluded, _, flipped = _run(fn, data, cuts, excl, qual, orig, lanes)
                assert rc == 0 and out == want, (upper, qual, orig, lanes, cuts[:4])
                assert (recs, excluded, flipped) == (kept, len(records) - kept, n_flip), (upper, qual, orig, lanes)
    return bam, sam


# ---------------------------------------------------------------------------------------------- the tables
def test_the_complement_tables():
    """strand_cases' own table against the issue's letters, and reads_io.stored_form against it."""
    from kmer_mapper_amd import reads_io
    assert sc.revcomp(sc.BAM_LETTERS) == sc.BAM_COMPLEMENT[::-1]
    assert sc.revcomp(b"GGACGTT") == b"AACGTCC"
    assert sc.revcomp(b"acgtNn=.UuWwSs*") == b"*sSwWuU.=nNacgt"
    for i, c in enumerate(sc.BAM_LETTERS):                    # the complement of a BAM code is the code with its four bits reversed
        assert sc.BAM_COMPLEMENT[i] == sc.BAM_LETTERS[int("{:04b}".format(i)[::-1], 2)], chr(c)
    every = bytes(range(256))
    assert sc.revcomp(sc.revcomp(every)) == every
    assert reads_io.stored_form(every, every, reverse=True) == (sc.revcomp(every), every[::-1])
    assert reads_io.stored_form(b"ACGTN", b"ABCDE") == (b"ACGTN", b"ABCDE")
    assert reads_io.stored_form(b"ACGTN", None, reverse=True) == (b"NACGT", None)


def test_the_library_complements_like_the_tables(lib):
    for c in range(256):
        assert lib.strand_comp_letter(c) == sc.revcomp(bytes([c]))[0], c
    assert bytes(lib.strand_comp_code_letter(i) for i in range(16)) == sc.BAM_COMPLEMENT
    assert bytes(lib.strand_comp_letter(c) for c in sc.BAM_LETTERS) == sc.BAM_COMPLEMENT          # BAM and upper-case SAM agree


# ---------------------------------------------------------------------------------------------- byte-exact text
def test_every_length_forward_and_reversed_interleaved(lib):
    records = sc.length_sweep(71, absent={2, 9, 21})
    assert [len(s) for _, s, _ in records[::2]] == list(sc.LENGTHS) and sc.n_flipped(records) == len(sc.LENGTHS) - 1
    assert sc.text(records, 1, 0) != sc.text(records, 0, 0) and sc.text(records, 1, 1) != sc.text(records, 0, 1)
    bam = sc.bam_payload(records)
    _both(lib, records, cuts_bam=((), (100, 700, 701, 3000), tuple(range(50, len(bam), 997))),
          cuts_sam=((), (5, 1000, 1001, 4000), tuple(range(100, 12_000, 1024))))


def test_a_reversed_record_of_40000_bases_between_ordinary_ones(lib):
    """Longer than a 16 KiB BAM tile and many 1 KiB SAM tiles; its neighbours are of the other strand."""
    rng = np.random.default_rng(72)
    records = [(0 if i % 2 else 16, sc.random_read(rng, n), sc.random_qual(rng, n)) for i, n in enumerate(rng.integers(10, 200, size=20))]
    records.insert(10, (16, sc.random_read(rng, 40_000), sc.random_qual(rng, 40_000)))
    records.insert(11, (0, sc.random_read(rng, 40_001), None))
    bam, _ = _both(lib, records, cuts_bam=((), tuple(range(10_000, 140_000, 10_000))), cuts_sam=((), tuple(range(10_000, 170_000, 10_000))),
                   variants=[(0, 1, 64), (1, 1, 64), (1, 1, 1), (0, 0, 1)])
    assert len(bam) > 4 * 16384


def test_all_16_bam_codes_in_one_reversed_record_and_bam_equals_upper_case_sam(lib):
    records = [(0, b"ACGT", b"IIII"), (16, sc.BAM_LETTERS, bytes(range(40, 56))), (16, sc.BAM_LETTERS[:15], bytes(range(60, 75))),
               (0, sc.BAM_LETTERS, None)]
    bam = sc.bam_payload(records)
    sam = sc.sam_bytes(records, upper=True)
    for qual, orig, lanes in VARIANTS:
        a = _run(lib.strand_bam_cpu, bam, qual=qual, orig=orig, lanes=lanes)
        b = _run(lib.strand_sam_cpu, sam, qual=qual, orig=orig, lanes=lanes)
        assert a == b and a[0] == 0 and a[1] == sc.text(records, orig, qual, upper=True), (qual, orig, lanes)
    assert _run(lib.strand_bam_cpu, bam, orig=1)[1].split(b"\n")[3] == sc.BAM_LETTERS


def test_sam_lower_case_other_bytes_star_and_crlf(lib):
    """Lower case is kept, '=', '.', U and digits are left as they are, SEQ "*" and QUAL "*" have nothing to flip / stay absent,
    a one-base read, CRLF line ends; the same set through the BAM decode (upper case)."""
    records = [(16, b"acgtnACGTNmkryvbhdwsMKRYVBHDWS", b"0123456789ABCDEFGHIJabcdefghij"), (16, b"AC=.UuG", b"IJKLMNO"), (16, b"", None),
               (16, b"ACGTT", None), (16, b"A", b"#"), (0, b"c", b"I"), (16 | 4, b"GATTACA", b"ABCDEFG"), (16, b"N", None)]
    for crlf in (False, True):
        sam = sc.sam_bytes(records, crlf=crlf)
        for qual, orig, lanes in VARIANTS:
            rc, out, recs, _, no_qual, flipped = _run(lib.strand_sam_cpu, sam, (40, 200), qual=qual, orig=orig, lanes=lanes)
            assert rc == 0 and out == sc.text(records, orig, qual), (crlf, qual, orig, lanes)
            assert recs == 8 and flipped == (6 if orig else 0) and no_qual == (2 if qual else 0)
    assert _run(lib.strand_sam_cpu, sc.sam_bytes(records), orig=1)[1].startswith(b">\nacgtnACGTNmkryvbhdwsMKRYVBHDWS\n>\nAC=.UuG\n>\n\n>\nACGTT\n")
    only_bam = [r for r in records if b"." not in r[1] and b"U" not in r[1]]
    _both(lib, only_bam)


def test_flag_values_and_the_filter(lib):
    """16, 16 | 4, 16 | 1 | 64 are flipped; 16 | 0x100 is dropped by excl 0x900 — not looked at, not counted — and flipped without
    the filter; 0 is left alone."""
    rng = np.random.default_rng(73)
    flags = [16, 16 | 4, 16 | 1 | 64, 16 | 0x100, 0, 0x800, 16 | 0x800 | 0x100, 16]
    records = [(f, sc.random_read(rng, 33 + i, b"ACGTN"), sc.random_qual(rng, 33 + i)) for i, f in enumerate(flags)]
    assert sc.n_flipped(records, 0x900) == 4 and sc.n_flipped(records) == 6
    for excl in (0, 0x900, 16):
        _both(lib, records, excl=excl)
    assert sc.n_flipped(records, 16) == 0


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/strand_san_main.cpp; host code, nothing sanitized is loaded into
    Python): every call's output lives in a heap buffer of exactly the totals' size, so a byte written in front of out[0] or behind
    the last record is reported.  (The padding nibble of an odd reversed l_seq would land on out[1], the newline inside the buffer:
    that one is caught by the byte-exact compare, here and in the tests above.)"""
    exe = str(tmp_path / "strand_san")
    src = os.path.join(ROOT, "tests", "strand_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    rng = np.random.default_rng(74)
    records = sc.length_sweep(75, absent={5, 12})
    records.insert(7, (16, sc.random_read(rng, 40_000, b"ACGTN"), sc.random_qual(rng, 40_000)))
    records += [(16 | 0x100, b"ACGTA", b"IIIII"), (16, b"", None), (16, b"G", b"5")]
    # the first kept record of the stream is reversed and odd: its first base is the buffer's byte 2, its padding nibble has no place
    records.insert(0, (16, b"ACG", b"ABC"))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    bam, sam = sc.bam_payload(records), sc.sam_bytes(records, crlf=True)
    kept = sum(1 for f, _, _ in records if not f & 0x900)
    for kind, data, upper in (("bam", bam, True), ("sam", sam, False)):
        inp.write_bytes(data)
        for (qual, orig, lanes), cuts in itertools.product(VARIANTS, ([], [str(c) for c in range(7, len(data), 4567)])):
            r = subprocess.run([exe, kind, str(inp), str(outp), "0x900", str(qual), str(orig), str(lanes), *cuts], capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            assert r.stdout.split()[:2] == ["0", str(kept)], r.stdout
            assert int(r.stdout.split()[4]) == (sc.n_flipped(records, 0x900) if orig else 0)
            assert outp.read_bytes() == sc.text(records, orig, qual, 0x900, upper), (kind, qual, orig, lanes, cuts[:3])


# ---------------------------------------------------------------------------------------------- the command line
def test_check_original_strand():
    from kmer_mapper_amd import command_line_interface as cli
    assert cli.check_original_strand(True, "bam") and cli.check_original_strand(True, "sam")
    for fmt in ("fastq", "fasta", "fasta_ml", "bam", "sam"):
        assert cli.check_original_strand(False, fmt) is False
    for fmt in ("fastq", "fasta", "fasta_ml"):
        with pytest.raises(ValueError, match="--original-strand applies to SAM and BAM input only"):
            cli.check_original_strand(True, fmt)


def test_cli_flag_up_to_its_first_hip_call(tmp_path, monkeypatch, caplog):
    """--original-strand is parsed and reaches map_gpu_raw for SAM and BAM; on FASTQ and FASTA it is refused before the index
    file is read; --host-parser stays refused on SAM / BAM; without 0x900 in the flag filter one info line says so."""
    import logging
    from kmer_mapper_amd import reads_io, synthetic
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.util import ReadBatch
    parser = cli.build_argument_parser()
    assert parser.parse_args(["map", "-f", "x.bam", "-o", "y", "--original-strand"]).original_strand is True
    assert parser.parse_args(["map", "-f", "x.sam", "-o", "y", "--original-strand"]).original_strand is True
    assert parser.parse_args(["map", "-f", "x.sam", "-o", "y"]).original_strand is False
    index, _ = synthetic.make_index(200, seed=3)
    b = ReadBatch.from_strings(["ACGT" * 10])
    reads_io.write_sam(str(tmp_path / "r.sam"), b)
    reads_io.write_bam(str(tmp_path / "r.bam"), b)
    reads_io.write_fastq(str(tmp_path / "r.fq"), b)
    reads_io.write_fasta(str(tmp_path / "r.fa"), b)
    index_reads = []

    def fake_index(a):
        index_reads.append(a.reads)
        return index
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", fake_index)
    seen = {}

    def fake_raw(index, path, chunk_size, fmt, k, *a, **kw):
        seen.clear()
        seen.update(fmt=fmt, **kw)
        return np.zeros(3, np.uint32)
    monkeypatch.setattr(cli, "map_gpu_raw", fake_raw)

    def args(name, *extra):
        return ["map", "-i", "idx.npz", "-f", str(tmp_path / name), "-o", str(tmp_path / "out"), *extra]
    for name, fmt in (("r.sam", "sam"), ("r.bam", "bam")):
        cli.run_argument_parser(args(name, "--original-strand", "--exclude-flags", "0x900"))
        assert seen["fmt"] == fmt and seen["original_strand"] is True and seen["exclude_flags"] == 0x900
        cli.run_argument_parser(args(name))
        assert seen["original_strand"] is False
        with pytest.raises(ValueError, match="--host-parser does not read %s" % fmt.upper()):
            cli.run_argument_parser(args(name, "--original-strand", "--host-parser"))
    for name in ("r.fq", "r.fa"):
        index_reads.clear()
        for extra in ([], ["--host-parser"]):
            with pytest.raises(ValueError, match="--original-strand applies to SAM and BAM input only"):
                cli.run_argument_parser(args(name, "--original-strand", *extra))
        assert index_reads == []                                        # refused before the index file is read
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--original-strand applies to SAM and BAM input only"):
        cli.map_gpu_raw(index, str(tmp_path / "r.fq"), 1 << 20, "fastq", 31, original_strand=True)
    for excl, n in ((0, 1), (0x100, 1), (0x900, 0), (0xF00, 0)):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            cli._log_original_strand_filter(excl)
        assert caplog.text.count("samtools fastq") == n and caplog.text.count("secondary and supplementary") == n
