"""CPU tier of "use_record_qual" (include/kmm.h): the quality variants of csrc/kmm_bam.hpp and csrc/kmm_sam.hpp — the
walks the GPU runs, with every kept record written as four-line FASTQ ("@\\n" SEQ "\\n+\\n" QUAL "\\n") — compiled by themselves with
g++ (tests/record_qual_cpu_driver.hpp) and driven in windows with a carry, against independent pure-Python readers of BAM and SAM
that keep QUAL (below); once more under AddressSanitizer + UndefinedBehaviorSanitizer.  Also: the test-data writers' quals=, and
the command line's --use-record-qual up to the first HIP call."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
_NIB = b"=ACMGRSVTWYHKDBN"


# ---------------------------------------------------------------------------------------------- the independent readers
def read_bam_qual(data):
    """Inflated BAM bytes (SAM/BAM specification 4.2) -> [(flag, SEQ letters, raw Phred bytes)]."""
    assert data[:4] == b"BAM\1"
    (l_text,) = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, p)
        p += 4 + l_name + 4
    recs = []
    while p < len(data):
        (bs,) = struct.unpack_from("<i", data, p)
        _, _, l_name, _, _, n_cig, flag, l_seq, _, _, _ = struct.unpack_from("<iiBBHHHiiii", data, p + 4)
        s = p + 36 + l_name + 4 * n_cig
        packed = data[s:s + (l_seq + 1) // 2]
        seq = bytes(_NIB[(packed[j // 2] >> (4 if j % 2 == 0 else 0)) & 15] for j in range(l_seq))
        recs.append((flag, seq, data[s + (l_seq + 1) // 2:s + (l_seq + 1) // 2 + l_seq]))
        p += 4 + bs
    return recs


class SamQualError(ValueError):
    def __init__(self, offset):
        super().__init__("QUAL and SEQ differ in length at byte %d" % offset)
        self.offset = offset


def read_sam_qual(data):
    """SAM bytes (specification 1.4) -> [(flag, SEQ, QUAL or None)]: SEQ "*" is b"", a QUAL that is exactly "*" is None (absent,
    for a one-base read too, as htslib reads it); any other QUAL must be as long as SEQ."""
    recs, pos = [], 0
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for line in lines:
        start, pos = pos, pos + len(line) + 1
        body = line[:-1] if line.endswith(b"\r") else line
        if body[:1] == b"@":
            continue
        f = body.split(b"\t")
        seq = b"" if f[9] == b"*" else f[9]
        qual = None if f[10] == b"*" else f[10]
        if qual is not None and len(qual) != len(seq):
            raise SamQualError(start)
        recs.append((int(f[1]), seq, qual))
    return recs


def fastq4_bam(recs, excl=0):
    """What the BAM quality variant writes: raw Phred + 33, clipped at '~' (0xFF, absent, becomes '~')."""
    return b"".join(b"@\n" + s + b"\n+\n" + bytes(min(q + 33, 126) for q in qual) + b"\n" for f, s, qual in recs if not f & excl)


def fastq4_sam(recs, excl=0):
    return b"".join(b"@\n" + s + b"\n+\n" + (b"~" * len(s) if qual is None else qual) + b"\n" for f, s, qual in recs if not f & excl)


# ---------------------------------------------------------------------------------------------- the driver
def _build(tmp_path, name, extra=()):
    src = tmp_path / (name + ".cpp")
    src.write_text('#include "record_qual_cpu_driver.hpp"\n')
    so = str(tmp_path / (name + ".so"))
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", *extra, "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                           str(src), "-o", so])
    return so


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = ctypes.CDLL(_build(tmp_path_factory.mktemp("record_qual"), "shim"))
    for fn in (lib.bam_qual_cpu, lib.sam_qual_cpu):
        fn.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                       ctypes.c_void_p, ctypes.c_void_p]
    lib.bam_walk_qual.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint32,
                                  ctypes.c_void_p]
    lib.bam_walk_qual.restype = None
    lib.bam_max_tile_out.restype = ctypes.c_uint64
    return lib


def _run(fn, data, cuts=(), excl=0):
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out = np.zeros(3 * len(data) + 64, np.uint8)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 8)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = fn(data, len(data), c, len(cuts), excl, out.ctypes.data, len(out), ctypes.byref(on), st)
    return rc, out[:on.value].tobytes(), list(st)


def _reads(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, size=n)
    return [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(L), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for L in lens]


def _bam_payload(rng, reads, flags=None, absent=()):
    """Records with names, CIGARs and tags of varying length; raw qualities 0 .. 93 and a few above (up to 254); `absent`: 0xFF."""
    from kmer_mapper_amd import reads_io
    recs = []
    for i, r in enumerate(reads):
        qual = None if i in absent else bytes(rng.choice(np.r_[0:94, 94, 127, 200, 254], size=len(r)).astype(np.uint8))
        recs.append(reads_io.bam_record(r, b"read%d" % i + b"x" * (i % 7), flags[i] if flags else 4, qual=qual,
                                        cigar=(len(r) << 4,) * (i % 3), aux=b"NMC\x00" * (i % 4)))
    return reads_io.bam_header((), b"@HD\tVN:1.6\n") + b"".join(recs)


def _sam_text(rng, reads, flags=None, absent=(), crlf=False, tags=True):
    """Records with header lines in front and between, aligned-looking fields, optional tags behind QUAL, SEQ "*" for an empty
    read (its QUAL is "*": the only QUAL the specification allows it)."""
    nl = b"\r\n" if crlf else b"\n"
    out = [b"@HD\tVN:1.6\tSO:unsorted" + nl, b"@CO\ta\tcomment\twith\tmany\ttabs\t\t\t\t\t\t\t\t" + nl]
    for i, r in enumerate(reads):
        flag = int(flags[i]) if flags is not None else 4
        qual = bytes(rng.integers(33, 127, size=len(r)).astype(np.uint8))
        if qual == b"*":
            qual = b"I"                                       # (a one-base QUAL that reads "*" IS absent)
        if i in absent or not r:
            qual = b"*"
        tag = b"\tNM:i:0\tRG:Z:g\t\tXX:Z:\t" if tags and i % 2 else b""
        out.append(b"q%d\t%d\tchr1\t%d\t60\t%dM\t=\t0\t0\t%s\t%s%s" % (i, flag, i + 1, max(len(r), 1), r or b"*", qual, tag) + nl)
        if i % 97 == 50:
            out.append(b"@CO\tinside" + nl)
    return b"".join(out)


# ---------------------------------------------------------------------------------------------- BAM
def test_bam_ragged_reads_in_windows_decode_like_the_python_reader(lib):
    rng = np.random.default_rng(41)
    reads = _reads(rng, 2500, 0, 300)
    absent = set(int(i) for i in rng.choice(len(reads), 300, replace=False))
    data = _bam_payload(rng, reads, absent=absent)
    recs = read_bam_qual(data)
    want = fastq4_bam(recs)
    assert b"\xff" not in want and want.count(b"~") > 300
    n_absent = sum(1 for i in absent if reads[i])             # (a record without bases has no qualities to miss)
    for cuts in ((), (100, 20_000, 20_001, 300_000), tuple(range(5_000, len(data), 16_384)), tuple(range(777, len(data), 33_333))):
        rc, out, st = _run(lib.bam_qual_cpu, data, cuts)
        assert rc == 0 and out == want, cuts[:4]
        assert st[0] == len(reads) and st[7] == n_absent


def test_bam_a_record_of_40000_bases_spans_four_tiles(lib):
    rng = np.random.default_rng(42)
    reads = _reads(rng, 20, 10, 200) + _reads(rng, 1, 40_000, 40_000) + _reads(rng, 20, 10, 200)
    data = _bam_payload(rng, reads, absent={3})
    want = fastq4_bam(read_bam_qual(data))
    assert len(data) > 4 * 16384
    for cuts in ((), tuple(range(10_000, len(data), 10_000)), (len(data) - 1,), tuple(range(1, len(data), 16_385))):
        rc, out, st = _run(lib.bam_qual_cpu, data, cuts)
        assert rc == 0 and out == want and st[7] == 1, cuts[:3]


def test_bam_flag_filter_leaves_out_the_record_and_its_qualities(lib):
    rng = np.random.default_rng(43)
    reads = _reads(rng, 600, 1, 150)
    flags = [int(f) for f in rng.choice([0, 4, 16, 256, 2048, 256 | 16], size=len(reads))]
    absent = set(range(0, 600, 5))
    data = _bam_payload(rng, reads, flags=flags, absent=absent)
    recs = read_bam_qual(data)
    for excl in (0, 0x900, 4):
        rc, out, st = _run(lib.bam_qual_cpu, data, (30_000,), excl)
        assert rc == 0 and out == fastq4_bam(recs, excl)
        assert st[1] == sum(1 for f in flags if f & excl)
        assert st[7] == sum(1 for i in absent if not flags[i] & excl)


def test_bam_the_uint32_output_byte_bound(lib):
    """Walk::bytes / Tile::bytes are uint32: the worst tile — small records up to its last bytes, then one of the largest
    block_size, every one with the longest SEQ its block_size allows — stays below 2^32, and below the bound kmm_bam.hpp states.
    (The buffer is 2 GiB of address space, never touched but for the record heads.)"""
    assert lib.bam_max_tile_out() < 1 << 32
    tile, big = 16384, (1 << 31) - 1
    n = tile + 4 + big + 64
    import mmap
    mem = mmap.mmap(-1, n, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000))
    d = np.frombuffer(mem, np.uint8)                          # (address space only: pages are made when written)
    p, total, recs = 0, 0, 0

    def put(p, bs):
        l_seq = ((bs - 34) * 2) // 3                          # 32 + l_name (2) + (l_seq + 1) / 2 + l_seq <= bs
        while 34 + (l_seq + 1) // 2 + l_seq > bs:
            l_seq -= 1
        d[p:p + 36] = np.frombuffer(struct.pack("<IiiBBHHHiiii", bs, -1, -1, 2, 0, 0, 0, 4, l_seq, -1, -1, 0), np.uint8)
        d[p + 36] = ord("r")
        return l_seq

    while p + 4 + 40 < tile - 1:
        total += 2 * put(p, 36) + 6
        p += 40
        recs += 1
    total += 2 * put(p, big) + 6
    recs += 1
    assert p < tile and total > 1 << 31
    out = (ctypes.c_uint64 * 5)()
    lib.bam_walk_qual(d.ctypes.data, n, 0, tile, 0, 0, out)
    assert list(out) == [p + 4 + big, recs, 0, total, 0]
    assert total <= lib.bam_max_tile_out()


# ---------------------------------------------------------------------------------------------- SAM
def test_sam_ragged_reads_in_windows_like_the_python_reader(lib):
    rng = np.random.default_rng(44)
    reads = _reads(rng, 2500, 0, 300)
    absent = set(int(i) for i in rng.choice(len(reads), 300, replace=False))
    for crlf in (False, True):
        data = _sam_text(rng, reads, absent=absent, crlf=crlf)
        recs = read_sam_qual(data)
        want = fastq4_sam(recs)
        n_absent = sum(1 for _, s, q in recs if q is None and s)
        assert n_absent >= sum(1 for i in absent if reads[i]) > 0 and b"@\n\n+\n\n" in want        # (SEQ "*": an empty record)
        for cuts in ((), (5, 1000, 1001, 70_000), tuple(range(777, len(data), 33_333)), tuple(range(100, len(data), 1024))):
            rc, out, st = _run(lib.sam_qual_cpu, data, cuts)
            assert rc == 0 and out == want, (crlf, cuts[:4])
            assert st[0] == len(reads) and st[5] == n_absent


def test_sam_absent_qual_makes_the_output_longer_than_the_line(lib):
    """QUAL "*" on reads longer than their other fields: 2 |SEQ| + 6 output bytes from a line of |SEQ| + 30 — the output of a
    window is larger than the window, and sized from the totals."""
    rng = np.random.default_rng(45)
    reads = _reads(rng, 200, 100, 400)
    data = _sam_text(rng, reads, absent=set(range(200)), tags=False)
    want = fastq4_sam(read_sam_qual(data))
    assert len(want) > len(data) + 16
    rc, out, st = _run(lib.sam_qual_cpu, data, (10_000,))
    assert rc == 0 and out == want and st[5] == 200
    one = b"r\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n"                   # a one-base read whose QUAL is "*": absent, not Phred 9
    rc, out, st = _run(lib.sam_qual_cpu, one)
    assert rc == 0 and out == b"@\nA\n+\n~\n" and st[5] == 1


def test_sam_a_record_of_40000_bases(lib):
    rng = np.random.default_rng(46)
    reads = _reads(rng, 20, 10, 200) + _reads(rng, 1, 40_000, 40_000) + _reads(rng, 20, 10, 200)
    data = _sam_text(rng, reads)
    want = fastq4_sam(read_sam_qual(data))
    for cuts in ((), tuple(range(10_000, len(data), 10_000)), (len(data) - 1,)):
        rc, out, st = _run(lib.sam_qual_cpu, data, cuts)
        assert rc == 0 and out == want, cuts[:3]


@pytest.mark.parametrize("bad", [
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIII\n",                    # one byte short
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIIII\n",                  # one byte long
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIII\tNM:i:0\n",            # short, tags behind it
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIIII\r\n",
    b"r\t4\t*\t0\t0\t*\t*\t0\t0\t*\tI\n",                         # SEQ "*" counts as length 0
    b"r\t256\t*\t0\t0\t*\t*\t0\t0\tACGT\t**\n",                   # (only a QUAL that is exactly "*" is absent)
])
def test_sam_a_qual_of_another_length_is_refused_with_its_line_offset(lib, bad):
    rng = np.random.default_rng(47)
    good = _sam_text(rng, _reads(rng, 300, 10, 100))
    cut = good.index(b"\n", len(good) // 2) + 1
    data = good[:cut] + bad + good[cut:]
    with pytest.raises(SamQualError) as e:
        read_sam_qual(data)
    assert e.value.offset == cut
    for cuts in ((), (cut - 5, cut + 3), (cut + 1,)):
        rc, _, st = _run(lib.sam_qual_cpu, data, cuts)
        assert rc == -3 and st[4] == cut << 2 | 0, cuts
    rc, _, st = _run(lib.sam_qual_cpu, good[:cut] + b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\n" + good[cut:])    # the older reasons stay
    assert rc == -3 and st[4] == cut << 2 | 1


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same walks and driver built as an executable with ASan + UBSan (tests/record_qual_san_main.cpp; host code): the
    output buffers are exactly as large as the totals say."""
    exe = str(tmp_path / "record_qual_san")
    src = os.path.join(ROOT, "tests", "record_qual_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr
    rng = np.random.default_rng(48)
    reads = _reads(rng, 400, 0, 300) + _reads(rng, 1, 40_000, 40_000)
    rng.shuffle(reads)
    flags = [int(f) for f in rng.choice([4, 256, 2048], size=len(reads))]
    absent = set(range(0, len(reads), 3))
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    bam = _bam_payload(rng, reads, flags=flags, absent=absent)
    sam = _sam_text(rng, reads, flags=flags, absent=absent, crlf=True)
    for kind, data, want in (("bam", bam, fastq4_bam(read_bam_qual(bam), 0x900)), ("sam", sam, fastq4_sam(read_sam_qual(sam), 0x900))):
        inp.write_bytes(data)
        for cuts in ([], [str(c) for c in range(7, len(data), 45_678)]):
            r = subprocess.run([exe, kind, str(inp), str(outp), "0x900", *cuts], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            assert r.stdout.split()[0] == "0" and outp.read_bytes() == want, (kind, cuts)
    inp.write_bytes(sam + b"r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\tIII\n")
    r = subprocess.run([exe, "sam", str(inp), str(outp), "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "-3" and int(r.stdout.split()[4]) == len(sam) << 2, r.stderr[-2000:]


# ---------------------------------------------------------------------------------------------- Python and the command line
def test_the_writers_take_quals(tmp_path):
    import gzip
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    b = ReadBatch.from_strings(["ACGTACGT", "", "GGGA", "T"])
    sam_q = [b"IIII##II", b"", None, b"*"]
    text = reads_io.sam_text(b, quals=sam_q)
    assert [(s, q) for _, s, q in read_sam_qual(text)] == [(b"ACGTACGT", b"IIII##II"), (b"", None), (b"GGGA", None), (b"T", None)]
    assert reads_io.sam_text(b) == reads_io.sam_text(b, quals=[b"I" * 8, b"", b"IIII", b"I"])           # None: 'I' as before
    bam_q = [bytes([40, 40, 2, 2, 93, 0, 40, 40]), b"", None, bytes([7])]
    p = str(tmp_path / "a.bam")
    reads_io.write_bam(p, b, quals=bam_q)
    recs = read_bam_qual(gzip.decompress(open(p, "rb").read()))
    assert [q for _, _, q in recs] == [bam_q[0], b"", b"\xff" * 4, bytes([7])]
    reads_io.write_bam(p, b)
    assert [q for _, _, q in read_bam_qual(gzip.decompress(open(p, "rb").read()))] == [b"\x28" * 8, b"", b"\x28" * 4, b"\x28"]
    reads_io.write_sam(str(tmp_path / "a.sam.gz"), b, bgzf=True, quals=sam_q)
    assert gzip.decompress(open(str(tmp_path / "a.sam.gz"), "rb").read()) == text
    with pytest.raises(ValueError, match="quality bytes"):
        reads_io.sam_text(b, quals=[b"III", b"", None, b"I"])


def test_check_min_base_quality_with_use_record_qual():
    from kmer_mapper_amd import command_line_interface as cli
    for fmt in ("sam", "bam"):
        assert cli.check_min_base_quality(20, 31, fmt, use_record_qual=True) == 20
        assert cli.check_min_base_quality(0, 31, fmt, use_record_qual=True) == 0
        with pytest.raises(ValueError, match=r"QUAL column of %s.*--use-record-qual" % fmt.upper()):
            cli.check_min_base_quality(20, 31, fmt)
        with pytest.raises(ValueError, match="needs -k 2"):
            cli.check_min_base_quality(20, 1, fmt, use_record_qual=True)
        with pytest.raises(ValueError, match="drop --host-parser"):
            cli.check_min_base_quality(20, 31, fmt, host_parser=True, use_record_qual=True)
    assert cli.check_min_base_quality(20, 31, "fastq", use_record_qual=True) == 20
    assert cli.check_use_record_qual(True, "bam", 20) and cli.check_use_record_qual(True, "sam", 1)
    assert not cli.check_use_record_qual(False, "fastq", 20)
    for fmt in ("fastq", "fasta", "fasta_ml"):
        with pytest.raises(ValueError, match="--use-record-qual applies to SAM and BAM input only"):
            cli.check_use_record_qual(True, fmt, 20)


def test_cli_flag_up_to_its_first_hip_call(tmp_path, monkeypatch, caplog):
    """--use-record-qual is parsed and reaches map_gpu_raw for SAM and BAM (SAM also with several ranks, BAM not); on a FASTQ it
    is refused; without --min-base-quality it warns once and changes nothing; --host-parser stays refused."""
    import logging
    from kmer_mapper_amd import reads_io, synthetic
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.util import ReadBatch
    assert cli.build_argument_parser().parse_args(["map", "-f", "x", "-o", "y", "--use-record-qual"]).use_record_qual is True
    assert cli.build_argument_parser().parse_args(["map", "-f", "x", "-o", "y"]).use_record_qual is False
    index, _ = synthetic.make_index(200, seed=3)
    b = ReadBatch.from_strings(["ACGT" * 10])
    reads_io.write_sam(str(tmp_path / "r.sam"), b)
    reads_io.write_bam(str(tmp_path / "r.bam"), b)
    reads_io.write_fastq(str(tmp_path / "r.fq"), b)
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", lambda a: index)
    seen = {}

    def fake_raw(index, path, chunk_size, fmt, k, *a, **kw):
        seen.clear()
        seen.update(fmt=fmt, **kw)
        return np.zeros(3, np.uint32)

    monkeypatch.setattr(cli, "map_gpu_raw", fake_raw)

    def args(name, *extra):
        return ["map", "-i", "idx.npz", "-f", str(tmp_path / name), "-o", str(tmp_path / "out"), *extra]
    for name, fmt in (("r.sam", "sam"), ("r.bam", "bam")):
        cli.run_argument_parser(args(name, "--min-base-quality", "20", "--use-record-qual"))
        assert seen["fmt"] == fmt and seen["min_base_quality"] == 20 and seen["use_record_qual"] is True
        with pytest.raises(ValueError, match="QUAL column of %s" % fmt.upper()):
            cli.run_argument_parser(args(name, "--min-base-quality", "20"))
        with pytest.raises(ValueError, match="--host-parser"):
            cli.run_argument_parser(args(name, "--min-base-quality", "20", "--use-record-qual", "--host-parser"))
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            cli.run_argument_parser(args(name, "--use-record-qual"))
        assert caplog.text.count("--use-record-qual has no effect without --min-base-quality") == 1
        assert seen["min_base_quality"] == 0 and seen["use_record_qual"] is False
    for extra in (["--min-base-quality", "20"], []):
        with pytest.raises(ValueError, match="--use-record-qual applies to SAM and BAM input only"):
            cli.run_argument_parser(args("r.fq", "--use-record-qual", *extra))
    monkeypatch.undo()
    cli._check_bam_route("sam", 2, 0)                                   # several ranks: every SAM line is a record
    with pytest.raises(ValueError, match="BAM input is mapped by one rank"):
        cli._check_bam_route("bam", 2, 0)
