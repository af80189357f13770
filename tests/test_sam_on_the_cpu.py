"""CPU tier of KMM_FORMAT_SAM: csrc/kmm_sam.hpp — the per-tile line walk the GPU runs (line starts, the lanes' TAB / newline
masks and their prefix, the line classification, the two-line FASTA output) — compiled by itself with g++ and driven in windows
with a carry, against an independent pure-Python SAM reader written from the SAM specification (below); once more under
AddressSanitizer + UndefinedBehaviorSanitizer.  Also: reads_io tells SAM by content, the SAM cut and multi-rank rules, and the
CLI's SAM route and its refusals up to the first HIP call."""
import ctypes
import gzip
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")


class SamError(ValueError):
    def __init__(self, offset, why):
        super().__init__("%s at byte %d" % (why, offset))
        self.offset, self.why = offset, why


def read_sam(data):
    """The independent reader (SAM specification 1.4, section 1.4): SAM bytes -> (records, header lines); a record = (flag, SEQ
    as stored, b"" for "*").  A line starting with '@' is a header line; every other line needs 11 TAB-separated fields and a
    decimal FLAG in [0, 65535]; an empty line is an error.  A last line without its newline counts."""
    recs, headers, pos = [], 0, 0
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for line in lines:
        start, pos = pos, pos + len(line) + 1
        body = line[:-1] if line.endswith(b"\r") else line
        if not body:
            raise SamError(start, "empty")
        if body[:1] == b"@":
            headers += 1
            continue
        f = body.split(b"\t")
        if len(f) < 11:
            raise SamError(start, "fields")
        if not (f[1].isdigit() and int(f[1]) <= 0xFFFF):
            raise SamError(start, "flag")
        recs.append((int(f[1]), b"" if f[9] == b"*" else f[9]))
    return recs, headers


def fasta2(recs, excl=0):
    return b"".join(b">\n" + s + b"\n" for f, s in recs if not f & excl)


def _build(tmp_path, name, extra=()):
    src = tmp_path / (name + ".cpp")
    src.write_text('#include "sam_cpu_driver.hpp"\n')
    so = str(tmp_path / (name + ".so"))
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", *extra, "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                           str(src), "-o", so])
    return so


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = ctypes.CDLL(_build(tmp_path_factory.mktemp("sam"), "shim"))
    lib.sam_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _run(lib, data, cuts=(), excl=0):
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out = np.zeros(len(data) + 16, np.uint8)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 5)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = lib.sam_cpu(data, len(data), c, len(cuts), excl, out.ctypes.data, len(out), ctypes.byref(on), st)
    return rc, out[:on.value].tobytes(), list(st)


def _reads(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, size=n)
    return [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(L), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for L in lens]


def random_sam(rng, reads, crlf=False, flags=None, tags=True, headers_inside=True):
    """SAM text with everything the parser must get right: header lines in front and between records, '*' SEQ, optional tags,
    aligned-looking fields, CRLF line ends."""
    nl = b"\r\n" if crlf else b"\n"
    out = [b"@HD\tVN:1.6\tSO:unsorted" + nl, b"@SQ\tSN:chr1\tLN:1000" + nl, b"@PG\tID:x\tPN:y\tCL:a b\tc" + nl]
    for i, r in enumerate(reads):
        flag = int(flags[i]) if flags is not None else int(rng.choice([0, 4, 16, 256, 2048, 0x900, 1 | 2 | 64]))
        seq = r if r else b"*"
        qual = b"I" * len(r) if r and i % 3 else b"*"
        tag = b"\tNM:i:0\tMD:Z:%d\tRG:Z:g\t\tXX:Z:\t\t" % len(r) if tags and i % 2 else b""
        out.append(b"q%d:%d/1\t%d\tchr1\t%d\t60\t%dM\t=\t0\t-%d\t%s\t%s%s" % (i, i * 7, flag, i + 1, max(len(r), 1), i, seq, qual, tag) + nl)
        if headers_inside and i % 97 == 50:
            out.append(b"@CO\tcomment\twith\ttabs\tand more\t\t\t\t\t\t\t" + nl)
    return b"".join(out)


def test_ragged_reads_in_windows_like_the_python_reader(lib):
    rng = np.random.default_rng(21)
    reads = _reads(rng, 3000, 0, 300)
    for crlf in (False, True):
        data = random_sam(rng, reads, crlf=crlf)
        recs, hdr = read_sam(data)
        for cuts in ((), (5, 1000, 1001, 70_000), tuple(range(777, len(data), 33_333)), tuple(range(100, len(data), 1024))):
            rc, out, st = _run(lib, data, cuts)
            assert rc == 0 and out == fasta2(recs), (crlf, cuts[:4])
            assert st[0] == len(reads) and st[2] == hdr


def test_flag_filter_and_star_seq(lib):
    rng = np.random.default_rng(22)
    reads = _reads(rng, 800, 0, 150)
    flags = [int(f) for f in rng.choice([0, 4, 16, 256, 2048, 256 | 16, 65535], size=len(reads))]
    data = random_sam(rng, reads, flags=flags)
    recs, _ = read_sam(data)
    for excl in (0, 0x900, 4):
        rc, out, st = _run(lib, data, (10_000, 20_000), excl)
        assert rc == 0 and out == fasta2(recs, excl)
        assert st[1] == sum(1 for f in flags if f & excl) and st[0] == len(reads) - st[1]
    assert b">\n\n" in fasta2(recs)                          # '*' reads are empty reads


def test_long_lines_span_many_tiles(lib):
    rng = np.random.default_rng(23)
    reads = _reads(rng, 4, 100_000, 210_000) + _reads(rng, 60, 0, 40)
    rng.shuffle(reads)
    data = random_sam(rng, reads)
    recs, _ = read_sam(data)
    for cuts in ((), tuple(range(100_000, len(data), 100_000)), (len(data) - 1,), tuple(range(1, len(data), 50_001))):
        rc, out, st = _run(lib, data, cuts)
        assert rc == 0 and out == fasta2(recs), cuts[:3]


def test_last_line_without_newline_and_header_only(lib):
    data = b"@HD\tVN:1.6\nr\t0\t*\t0\t0\t*\t*\t0\t0\tACGTA\tIIIII"
    rc, out, st = _run(lib, data, (20,))
    assert rc == 0 and out == b">\nACGTA\n" and st[0] == 1 and st[2] == 1
    rc, out, st = _run(lib, b"@HD\tVN:1.6\n@SQ\tSN:c\tLN:5\n")
    assert rc == 0 and out == b"" and st[0] == 0 and st[2] == 2


@pytest.mark.parametrize("bad,why", [
    (b"r\t0\t*\t0\t0\t*\t*\t0\t0\tACGT\n", "fields"),            # 10 fields
    (b"r\t70000\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n", "flag"),
    (b"r\t1a\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n", "flag"),
    (b"r\t\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n", "flag"),
    (b"r\t-4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n", "flag"),
    (b"\n", "empty"),
    (b"\r\n", "empty"),
])
def test_refusals_name_the_first_bad_line(lib, bad, why):
    rng = np.random.default_rng(24)
    good = random_sam(rng, _reads(rng, 300, 10, 100))
    cut = good.index(b"\n", len(good) // 2) + 1
    data = good[:cut] + bad + good[cut:] + bad
    with pytest.raises(SamError) as e:
        read_sam(data)
    assert e.value.offset == cut and e.value.why == why
    code = {"fields": 1, "flag": 2, "empty": 3}[why]
    for cuts in ((), (cut - 5, cut + 3), (cut + 1,)):
        rc, _, st = _run(lib, data, cuts)
        assert rc == -3 and st[4] == cut << 2 | code, cuts


def test_sniff_format_tells_sam_by_content(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    b = ReadBatch.from_strings(["ACGTACGT", "", "GGGA"])
    for hdr in (b"@HD\tVN:1.6\n", b""):
        for name, kw in (("x.sam", {}), ("x.sam.gz", {"bgzf": True}), ("y.sam.gz", {"gz": True}), ("noext.txt", {})):
            p = str(tmp_path / name)
            reads_io.write_sam(p, b, header=hdr, **kw)
            assert reads_io.sniff_format(p) == ("sam", True), (hdr, name)
            raw = open(p, "rb").read()
            recs, _ = read_sam(gzip.decompress(raw) if kw else raw)
            assert [s for _, s in recs] == [b"ACGTACGT", b"", b"GGGA"]
    # a FASTQ whose first header reads like a SAM header line stays FASTQ, whatever its name
    (tmp_path / "hd.sam").write_bytes(b"@HD\tVN:1.6\nACGT\n+\nIIII\n@r2\nGG\n+\nII\n")
    assert reads_io.sniff_format(str(tmp_path / "hd.sam"))[0] == "fastq"
    reads_io.write_fastq(str(tmp_path / "a.fq"), b)
    reads_io.write_fasta(str(tmp_path / "a.fa"), b)
    reads_io.write_fastq(str(tmp_path / "a.fq.gz"), b, gz=True)
    reads_io.write_bam(str(tmp_path / "a.bam"), b)
    assert reads_io.sniff_format(str(tmp_path / "a.fq")) == ("fastq", True)
    assert reads_io.sniff_format(str(tmp_path / "a.fa"))[0] == "fasta"
    assert reads_io.sniff_format(str(tmp_path / "a.fq.gz")) == ("fastq", True)
    assert reads_io.sniff_format(str(tmp_path / "a.bam")) == ("bam", True)


def _rank_file(rng, tmp_path):
    """A SAM file whose header is a third of it and that holds a 100 kb line near a rank boundary."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    reads = [r.decode() for r in _reads(rng, 400, 0, 200)]
    reads[200] = "ACGT" * 25_000
    header = b"".join(b"@SQ\tSN:chr%d\tLN:%d\n" % (i, 1000 + i) for i in range(6000))
    b = ReadBatch.from_strings(reads)
    return b, header


def test_records_cut_and_rank_byte_ranges_partition_the_records(tmp_path):
    from kmer_mapper_amd import reads_io
    rng = np.random.default_rng(25)
    b, header = _rank_file(rng, tmp_path)
    p = str(tmp_path / "r.sam")
    reads_io.write_sam(p, b, header=header)
    data = open(p, "rb").read()
    recs, hdr = read_sam(data)
    for cut_at in (0, 10, len(header) - 3, len(data) // 2, len(data) - 1):
        buf = np.frombuffer(data[:cut_at], np.uint8)
        c = reads_io.records_cut(buf, "sam")
        assert c == (data.rindex(b"\n", 0, cut_at) + 1 if b"\n" in data[:cut_at] else 0)
    for w in (2, 3, 5):
        ranges = [reads_io.rank_byte_range(p, "sam", r, w) for r in range(w)]
        assert ranges[0][0] == 0 and ranges[-1][1] == len(data)
        assert all(ranges[i][1] == ranges[i + 1][0] for i in range(w - 1))
        assert all(lo == 0 or data[lo - 1:lo] == b"\n" for lo, _ in ranges)
        got, got_hdr = [], 0
        for lo, hi in ranges:
            r, h = read_sam(data[lo:hi])
            got += r
            got_hdr += h
        assert got == recs and got_hdr == hdr, w
    assert any(lo < len(header) for lo, _ in [reads_io.rank_byte_range(p, "sam", 1, 5)])  # (a boundary inside the header)


def test_rank_member_ranges_partition_the_records(tmp_path):
    from kmer_mapper_amd import bgzf_ranges, reads_io
    rng = np.random.default_rng(26)
    b, header = _rank_file(rng, tmp_path)
    p = str(tmp_path / "r.sam.gz")
    reads_io.write_sam(p, b, header=header, bgzf=True, block=8000)
    buf = open(p, "rb").read()
    data = gzip.decompress(buf)
    recs, hdr = read_sam(data)
    for w in (2, 3, 5):
        got, got_hdr = [], 0
        for r in range(w):
            lo, s0, hi, s1 = bgzf_ranges.rank_member_range(buf, "sam", r, w)
            parts, m = [], lo
            while m < hi:
                e = bgzf_ranges.member_end(buf, m)
                parts.append(bgzf_ranges.inflate_member(buf, m, e))
                m = e
            mine = b"".join(parts)[s0:]
            if s1:
                mine += bgzf_ranges.inflate_member(buf, hi, bgzf_ranges.member_end(buf, hi))[:s1]
            if mine:
                assert mine.endswith(b"\n")
            rr, hh = read_sam(mine)
            got += rr
            got_hdr += hh
        assert got == recs and got_hdr == hdr, w


def test_cli_sam_route_up_to_its_first_hip_call_and_its_refusals(tmp_path, monkeypatch):
    """`kmer_mapper map -f r.sam` sniffs SAM and takes the GPU route with the flag filter (also with several ranks); --host-parser
    with SAM is refused, --exclude-flags on a FASTQ still is; the route fails loudly at its first HIP call without a GPU."""
    from kmer_mapper_amd import _lib, reads_io, synthetic
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.util import ReadBatch
    index, _ = synthetic.make_index(200, seed=3)
    reads_io.write_sam(str(tmp_path / "r.sam"), ReadBatch.from_strings(["ACGT" * 10]))
    reads_io.write_fastq(str(tmp_path / "r.fq"), ReadBatch.from_strings(["ACGT" * 10]))
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", lambda a: index)
    seen = {}

    def fake_raw(index, path, chunk_size, fmt, k, *a, **kw):
        seen.update(fmt=fmt, path=path, **kw)
        return np.zeros(3, np.uint32)

    monkeypatch.setattr(cli, "map_gpu_raw", fake_raw)
    args = ["map", "-i", "idx.npz", "-f", str(tmp_path / "r.sam"), "-o", str(tmp_path / "out")]
    cli.run_argument_parser(args + ["--exclude-flags", "0x900"])
    assert seen["fmt"] == "sam" and seen["exclude_flags"] == 0x900
    with pytest.raises(ValueError, match="--host-parser does not read SAM"):
        cli.run_argument_parser(args + ["--host-parser"])
    with pytest.raises(ValueError, match="BAM input only"):
        cli.run_argument_parser(["map", "-i", "idx.npz", "-f", str(tmp_path / "r.fq"), "-o", str(tmp_path / "o"), "--exclude-flags", "4"])
    monkeypatch.undo()
    cli._check_bam_route("sam", 4, 0x900)                    # several ranks and the filter: not refused for SAM
    if _lib.device_count() == 0:
        with pytest.raises(Exception):                        # the index upload: the route's first HIP call
            cli.map_gpu_raw(index, str(tmp_path / "r.sam"), 1 << 20, "sam", 31, exclude_flags=0x900)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same walk and driver built as an executable with ASan + UBSan (tests/sam_san_main.cpp; host code): ragged, long,
    CRLF and filtered records in windows, a malformed line — the Python reader's bytes, and no report."""
    exe = str(tmp_path / "sam_san")
    src = os.path.join(ROOT, "tests", "sam_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr
    rng = np.random.default_rng(27)
    reads = _reads(rng, 400, 0, 300) + _reads(rng, 2, 100_000, 120_000)
    rng.shuffle(reads)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    for crlf in (False, True):
        data = random_sam(rng, reads, crlf=crlf)
        recs, _ = read_sam(data)
        inp.write_bytes(data)
        for cuts in ([], [str(c) for c in range(7, len(data), 45_678)]):
            r = subprocess.run([exe, str(inp), str(outp), "0x900", *cuts], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            assert r.stdout.split()[0] == "0" and outp.read_bytes() == fasta2(recs, 0x900), cuts
    inp.write_bytes(data[:data.index(b"\n", 5000) + 1] + b"r\t99999\t*\t0\t0\t*\t*\t0\t0\tA\tI\n")
    r = subprocess.run([exe, str(inp), str(outp), "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "-3", r.stderr[-2000:]
