"""CPU tier of kmm_map_bam: csrc/kmm_bam.hpp — the speculative record walk the GPU runs (spec, link check and fix, totals,
decode) — compiled by itself with g++ and driven through the very same orchestration (run_call) on the CPU, against an
independent pure-Python BAM reader (gzip + struct, below); once more under AddressSanitizer + UndefinedBehaviorSanitizer.
Also: reads_io recognises BAM by content, and the CLI's BAM route and its refusals up to the first HIP call."""
import ctypes
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")

_NIB = b"=ACMGRSVTWYHKDBN"


def read_bam_payload(data):
    """The independent reader (SAM/BAM specification 4.2): inflated BAM bytes -> (records, header length); a record =
    (flag, seq bytes as letters).  Raises ValueError on anything malformed."""
    if data[:4] != b"BAM\1":
        raise ValueError("magic")
    (l_text,) = struct.unpack_from("<i", data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from("<i", data, p)
    p += 4
    for _ in range(n_ref):
        (l_name,) = struct.unpack_from("<i", data, p)
        p += 4 + l_name + 4
    hdr = p
    recs = []
    while p < len(data):
        if p + 4 > len(data):
            raise ValueError("truncated")
        (bs,) = struct.unpack_from("<i", data, p)
        if p + 4 + bs > len(data):
            raise ValueError("truncated")
        ref, pos, l_name, mapq, bin_, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from("<iiBBHHHiiii", data, p + 4)
        s = p + 36 + l_name + 4 * n_cig
        if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
            raise ValueError("block_size")
        packed = data[s:s + (l_seq + 1) // 2]
        seq = bytes(_NIB[(packed[j // 2] >> (4 if j % 2 == 0 else 0)) & 15] for j in range(l_seq))
        recs.append((flag, seq))
        p += 4 + bs
    return recs, hdr


def read_bam(path_or_bytes):
    raw = path_or_bytes if isinstance(path_or_bytes, bytes) else open(path_or_bytes, "rb").read()
    return read_bam_payload(gzip.decompress(raw))


def fasta2(recs, excl=0):
    return b"".join(b">\n" + s + b"\n" for f, s in recs if not f & excl)


def _build(tmp_path, name, extra=()):
    src = tmp_path / (name + ".cpp")
    src.write_text('#include "bam_cpu_driver.hpp"\n')
    so = str(tmp_path / (name + ".so"))
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", *extra, "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                           str(src), "-o", so])
    return so


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    lib = ctypes.CDLL(_build(tmp_path_factory.mktemp("bam"), "shim"))
    lib.bam_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p,
                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _run(lib, data, cuts=(), excl=0):
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out = np.zeros(len(data) + 16, np.uint8)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 7)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = lib.bam_cpu(data, len(data), c, len(cuts), excl, out.ctypes.data, len(out), ctypes.byref(on), st)
    return rc, out[:on.value].tobytes(), list(st)


def _reads(rng, n, lo, hi):
    lens = rng.integers(lo, hi + 1, size=n)
    return [bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), size=int(L), p=[0.24, 0.24, 0.24, 0.24, 0.04])) for L in lens]


def _payload(reads, refs=(), text=b"", names=None, flags=None, quals=None, auxs=None, cigars=None):
    from kmer_mapper_amd import reads_io
    recs = []
    for i, r in enumerate(reads):
        recs.append(reads_io.bam_record(r, names[i] if names else b"read%d" % i, flags[i] if flags else 4,
                                        cigar=cigars[i] if cigars else (), qual=quals[i] if quals else None,
                                        aux=auxs[i] if auxs else b""))
    return reads_io.bam_header(refs, text) + b"".join(recs)


def test_ragged_reads_in_windows_decode_like_the_python_reader(lib):
    rng = np.random.default_rng(11)
    reads = _reads(rng, 3000, 0, 300)
    data = _payload(reads, refs=[(b"chr%d" % i, 1000) for i in range(5)], text=b"@HD\tVN:1.6\n")
    recs, hdr = read_bam_payload(data)
    want = fasta2(recs)
    for cuts in ((), (hdr - 3, hdr + 17, 70_000, 70_001, 300_000), tuple(range(5000, len(data), 33_333)), (5,)):
        rc, out, st = _run(lib, data, cuts)
        assert rc == 0 and out == want, cuts
        assert st[0] == len(reads) and st[5] == hdr


def test_false_starts_are_found_and_rejected(lib):
    """Names, qualities and aux crafted to look like records (a copy of a real record inside them): the walk still finds the
    true chain, and the link check had to reject speculative starts."""
    rng = np.random.default_rng(12)
    reads = _reads(rng, 1500, 20, 200)
    decoy = _payload([b"ACGT" * 5])[12:]                      # a whole record (header of 12 bytes with no references)
    decoy = decoy * 5                                         # ... and a chain of them
    quals = [decoy[:len(r)] + b"\x28" * max(0, len(r) - len(decoy)) for r in reads]
    auxs = [b"ZZZ" + decoy if i % 3 == 0 else b"" for i in range(len(reads))]
    data = _payload(reads, quals=quals, auxs=auxs)
    recs, _ = read_bam_payload(data)
    rc, out, st = _run(lib, data, (40_000, 90_000))
    assert rc == 0 and out == fasta2(recs)
    assert st[2] > 0 and st[3] > 0


def test_long_reads_span_many_tiles(lib):
    rng = np.random.default_rng(13)
    reads = _reads(rng, 6, 150_000, 260_000) + _reads(rng, 50, 0, 40)
    rng.shuffle(reads)
    data = _payload(reads, cigars=[(150 << 4,)] * len(reads))
    recs, _ = read_bam_payload(data)
    for cuts in ((), tuple(range(100_000, len(data), 100_000)), (len(data) - 1,)):
        rc, out, st = _run(lib, data, cuts)
        assert rc == 0 and out == fasta2(recs), cuts


def test_flag_filter(lib):
    rng = np.random.default_rng(14)
    reads = _reads(rng, 800, 30, 150)
    flags = [int(f) for f in rng.choice([0, 4, 16, 256, 2048, 256 | 16], size=len(reads))]
    data = _payload(reads, flags=flags)
    recs, _ = read_bam_payload(data)
    rc, out, st = _run(lib, data, (), excl=0x900)
    assert rc == 0 and out == fasta2(recs, 0x900)
    assert st[1] == sum(1 for f in flags if f & 0x900)


def test_refusals(lib):
    rng = np.random.default_rng(15)
    data = _payload(_reads(rng, 200, 10, 100))
    assert _run(lib, b"BAN\1" + data[4:])[0] == -1              # magic
    assert _run(lib, data[:7])[0] == -2                         # ends inside the header
    assert _run(lib, data[:-5])[0] == -4                        # ends inside a record
    _, hdr = read_bam_payload(data)
    bad = bytearray(data)
    p = hdr
    for _ in range(50):                                         # record 50: block_size too small for its fields
        p += 4 + struct.unpack_from("<i", bad, p)[0]
    struct.pack_into("<i", bad, p, 34)
    rc, _, st = _run(lib, bytes(bad), (p + 1000,))
    assert rc == -3 and st[6] == p


def test_sniff_format_tells_bam_by_content(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    b = ReadBatch.from_strings(["ACGTACGT", "GGGA"])
    for name in ("x.bam", "reads.fq.gz", "noext"):
        reads_io.write_bam(str(tmp_path / name), b)
        assert reads_io.sniff_format(str(tmp_path / name)) == ("bam", True)
        recs, _ = read_bam(str(tmp_path / name))
        assert [s for _, s in recs] == [b"ACGTACGT", b"GGGA"]
    reads_io.write_fastq(str(tmp_path / "y.fq.gz"), b, gz=True)
    assert reads_io.sniff_format(str(tmp_path / "y.fq.gz"))[0] == "fastq"


def test_cli_bam_route_up_to_its_first_hip_call_and_its_refusals(tmp_path, monkeypatch):
    """`kmer_mapper map -f r.bam` sniffs BAM and takes the GPU route with the flag filter; that route fails loudly at its first
    HIP call without a GPU.  Several ranks, --host-parser with BAM, and --exclude-flags on a FASTQ are refused before that."""
    from kmer_mapper_amd import _lib, reads_io, synthetic
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.util import ReadBatch
    index, _ = synthetic.make_index(200, seed=3)
    reads_io.write_bam(str(tmp_path / "r.bam"), ReadBatch.from_strings(["ACGT" * 10]))
    reads_io.write_fastq(str(tmp_path / "r.fq"), ReadBatch.from_strings(["ACGT" * 10]))
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", lambda a: index)
    seen = {}

    def fake_raw(index, path, chunk_size, fmt, k, *a, **kw):
        seen.update(fmt=fmt, path=path, **kw)
        return np.zeros(3, np.uint32)

    monkeypatch.setattr(cli, "map_gpu_raw", fake_raw)
    args = ["map", "-i", "idx.npz", "-f", str(tmp_path / "r.bam"), "-o", str(tmp_path / "out")]
    cli.run_argument_parser(args + ["--exclude-flags", "0x900"])
    assert seen["fmt"] == "bam" and seen["exclude_flags"] == 0x900
    with pytest.raises(ValueError, match="--host-parser"):
        cli.run_argument_parser(args + ["--host-parser"])
    with pytest.raises(ValueError, match="BAM input only"):
        cli.run_argument_parser(["map", "-i", "idx.npz", "-f", str(tmp_path / "r.fq"), "-o", str(tmp_path / "o"), "--exclude-flags", "4"])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="one rank"):
        cli.map_gpu_raw(index, str(tmp_path / "r.bam"), 1 << 20, "bam", 31, world_size=2)
    if _lib.device_count() == 0:
        with pytest.raises(Exception):                        # the index upload: the route's first HIP call
            cli.map_gpu_raw(index, str(tmp_path / "r.bam"), 1 << 20, "bam", 31, exclude_flags=0x900)
    else:
        assert cli.map_gpu_raw(index, str(tmp_path / "r.bam"), 1 << 20, "bam", 31).shape == (index.max_node_id() + 1,)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same walk and driver built as an executable with ASan + UBSan (tests/bam_san_main.cpp; host code): ragged, long and
    decoy-laden records in windows, a malformed record — the Python reader's bytes, and no report."""
    exe = str(tmp_path / "bam_san")
    src = os.path.join(ROOT, "tests", "bam_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr
    rng = np.random.default_rng(16)
    reads = _reads(rng, 400, 0, 300) + _reads(rng, 2, 100_000, 120_000)
    rng.shuffle(reads)
    decoy = _payload([b"ACGT" * 5])[12:] * 4
    data = _payload(reads, auxs=[decoy if i % 4 == 0 else b"" for i in range(len(reads))], refs=[(b"c", 10)])
    recs, _ = read_bam_payload(data)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(data)
    for cuts in ([], [str(c) for c in range(7, len(data), 45_678)]):
        r = subprocess.run([exe, str(inp), str(outp), "0", *cuts], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        assert r.stdout.split()[0] == "0" and outp.read_bytes() == fasta2(recs), cuts
    inp.write_bytes(data[:-3])
    r = subprocess.run([exe, str(inp), str(outp), "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split()[0] == "-4", r.stderr[-2000:]
