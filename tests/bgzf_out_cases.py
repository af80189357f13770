"""The catalogue of the BGZF writer's tests: texts built from fixed numpy.random.RandomState seeds, each at most
200 KB; the check of an output against zlib; the g++ build of csrc/kmm_bgzf_out.hpp (tests/bgzf_out_cpu_driver.hpp) and the
generator of tests/golden/bgzf_out_expected.json, which ties the GPU kernel to that build:

    python -m tests.bgzf_out_cases --write
"""
import ctypes
import functools
import gzip
import hashlib
import json
import os
import struct
import subprocess
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bgzf_out_expected.json")
BLOCK = 0xFF00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SEAMS = (0, 1, 3, 254, 255, 256, 510, 65279, 65280, 65281, 2 * 65280 + 1)
FIB = [1, 1]
while len(FIB) < 22:
    FIB.append(FIB[-1] + FIB[-2])


def bound(n):
    return n + 31 * ((n + BLOCK - 1) // BLOCK)


def fastq_text(n_records, seed, quals):
    """150-base reads, Illumina-style names that share a prefix, qualities drawn from `quals` = (values, probabilities)."""
    rs = np.random.RandomState(seed)
    out = []
    values = np.asarray(quals[0], dtype=np.uint8) + 33
    for r in range(n_records):
        name = "@A00123:45:HXXXXXXXX:1:%d:%d:%d 1:N:0:ACGTACGT" % (1101 + r // 100, 1000 + int(rs.randint(0, 30000)), 1000 + 7 * r)
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, 150)].tobytes()
        qual = values[rs.choice(len(values), 150, p=quals[1])].tobytes()
        out.append(name.encode() + b"\n" + seq + b"\n+\n" + qual + b"\n")
    return b"".join(out)


SKEWED = ((2, 11, 25, 37), (0.02, 0.08, 0.2, 0.7))
UNIFORM41 = (tuple(range(41)), (1.0 / 41,) * 41)


def printable(rs, n):
    return rs.randint(32, 127, n).astype(np.uint8).tobytes()


def no_repeat_text(seed, n=3000, letters=16):
    """Compressible (16 letters) and without a repeated 4-byte string: no match can be found, no distance code is used."""
    rs = np.random.RandomState(seed)
    seen, out = set(), [0, 1, 2]
    while len(out) < n:
        for c in rs.permutation(letters):
            gram = (out[-3], out[-2], out[-1], int(c))
            if gram not in seen:
                seen.add(gram)
                out.append(int(c))
                break
        else:
            raise AssertionError("the walk is stuck")
    return bytes(97 + c for c in out)


def repeat_text(seed, length, at):
    """Random printable filler with `length` bytes of it repeated once, the copy starting at byte `at`; what follows the copy
    differs from what follows the original, so the repeat is exactly `length` long."""
    rs = np.random.RandomState(seed)
    text = bytearray(printable(rs, at + length + 500))
    text[at:at + length] = text[100:100 + length]
    if text[at + length] == text[100 + length]:
        text[at + length] = 32 + (text[at + length] - 31) % 95
    return bytes(text)


def limited_text(seed):
    """A text whose LITERALS keep Fibonacci frequencies although the end-of-block symbol joins them: 20 letters with the
    frequencies F(2) .. F(21) — the end-of-block symbol is the chain's F(1) — every one followed by a letter of a second, uniform
    alphabet of 16, so that the four-byte repeats are short and cheaper as literals.  The literal / length code is deeper than 15
    before the limit."""
    rs = np.random.RandomState(seed)
    letters = np.repeat(np.arange(20, dtype=np.uint8) + 200, FIB[1:21])
    rs.shuffle(letters)
    text = np.empty(2 * len(letters), dtype=np.uint8)
    text[0::2] = letters
    text[1::2] = rs.randint(48, 64, len(letters))
    return text.tobytes()


@functools.lru_cache(maxsize=None)
def all_cases():
    """name -> text, in a fixed order."""
    cases = {}
    seam_src = fastq_text(400, 11, SKEWED)
    for n in SEAMS:
        cases["seam_%d" % n] = seam_src[:n]
    cases["fastq_skewed_quals"] = fastq_text(420, 1, SKEWED)
    cases["fastq_uniform_41_quals"] = fastq_text(420, 2, UNIFORM41)
    rs = np.random.RandomState(3)
    lines = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, (1300, 101))].copy()
    lines[:, 100] = 10
    cases["random_acgt_lines"] = lines.tobytes()
    record = fastq_text(1, 4, SKEWED)
    cases["one_record_repeated"] = (record * (BLOCK // len(record) + 1))[:BLOCK]
    cases["poly_a"] = b"A" * 70000
    cases["one_distinct_byte_1"] = b"G"
    cases["one_distinct_byte_65280"] = b"G" * BLOCK
    cases["no_repeated_4_bytes"] = no_repeat_text(5)
    cases["random_bytes"] = np.random.RandomState(6).randint(0, 256, 150000).astype(np.uint8).tobytes()
    letters = np.repeat(np.arange(22, dtype=np.uint8) + 97, FIB)
    np.random.RandomState(7).shuffle(letters)
    cases["fibonacci_frequencies"] = letters.tobytes()
    cases["fibonacci_literals_beside_the_end_of_block"] = limited_text(12)
    head = printable(np.random.RandomState(8), 32768)
    cases["window_edge_32768"] = head + head[:64]
    cases["window_edge_32769"] = head + b"\x01" + head[:64]
    for length in (258, 300):
        cases["repeat_%d_at_a_segment_start" % length] = repeat_text(9, length, 255 * 8)
        cases["repeat_%d_across_a_segment_end" % length] = repeat_text(10, length, 255 * 8 + 100)
    assert all(len(t) <= 200000 for t in cases.values())
    return cases


def members_of(data):
    """[(member bytes, deflate bytes, crc, isize)] of a BGZF stream, by its BSIZE fields; the headers are checked."""
    out, p = [], 0
    while p < len(data):
        head = data[p:p + 18]
        assert head[:16] == bytes.fromhex("1f8b08040000000000ff0600") + b"BC\x02\x00", "member header at %d: %r" % (p, head)
        size = struct.unpack("<H", head[16:18])[0] + 1
        member = data[p:p + size]
        assert len(member) == size and size >= 26
        crc, isize = struct.unpack("<II", member[-8:])
        out.append((member, member[18:-8], crc, isize))
        p += size
    return out


def check_stream(data, text):
    """`data` (members, no EOF block) is the BGZF form of `text`: the layout, every member by itself against zlib, the whole
    through gzip.  Returns the member sizes."""
    members = members_of(data)
    assert len(members) == (len(text) + BLOCK - 1) // BLOCK
    for i, (member, deflate, crc, isize) in enumerate(members):
        piece = text[i * BLOCK:(i + 1) * BLOCK]
        d = zlib.decompressobj(-15)
        got = d.decompress(deflate)
        assert d.eof and d.unused_data == b"" and got == piece, "member %d does not inflate to its piece" % i
        assert crc == zlib.crc32(piece) and isize == len(piece)
        assert len(member) <= len(piece) + 31
        first = deflate[0] & 7                                          # BFINAL, BTYPE of the member's only block
        assert first in (1, 5), "member %d: a final stored or dynamic block is expected, got %d" % (i, first)
        if first == 1:
            assert len(member) == len(piece) + 31
    assert gzip.decompress(data + EOF_BLOCK) == text
    return [len(m[0]) for m in members]


def build_cpu_lib(tmp_dir):
    """The g++ build of csrc/kmm_bgzf_out.hpp with the driver's C entry points, as a ctypes library."""
    src = os.path.join(str(tmp_dir), "bgzf_out_shim.cpp")
    with open(src, "w") as f:
        f.write('#include "bgzf_out_cpu_driver.hpp"\n')
    so = os.path.join(str(tmp_dir), "bgzf_out_shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), src, "-o", so])
    lib = ctypes.CDLL(so)
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    lib.bgzf_out_bound_cpu.restype = I64
    lib.bgzf_out_bound_cpu.argtypes = [I64]
    lib.bgzf_out_compress_cpu.restype = I64
    lib.bgzf_out_compress_cpu.argtypes = [P, I64, P, I64, P, P]
    return lib


def cpu_compress(lib, text, capacity=None):
    """(members, sizes, (deepest code, limited members, stored members)) of the CPU build; None when it refuses the capacity."""
    n = len(text)
    cap = bound(n) if capacity is None else capacity
    src = np.frombuffer(text, dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8)
    out = np.full(max(cap, 1), 0x5A, dtype=np.uint8)
    sizes = np.zeros(max((n + BLOCK - 1) // BLOCK, 1), dtype=np.uint32)
    stats = np.zeros(3, dtype=np.uint32)
    got = lib.bgzf_out_compress_cpu(src.ctypes.data, n, out.ctypes.data, cap, sizes.ctypes.data, stats.ctypes.data)
    if got < 0:
        return None
    return out[:got].tobytes(), sizes[:(n + BLOCK - 1) // BLOCK].tolist(), tuple(int(x) for x in stats)


def golden_of(lib):
    return {name: {"sizes": cpu_compress(lib, text)[1], "sha256": hashlib.sha256(cpu_compress(lib, text)[0]).hexdigest()}
            for name, text in all_cases().items()}


def read_golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        fresh = golden_of(build_cpu_lib(tmp))
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(fresh, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", GOLDEN)
    else:
        print("golden file is", "current" if fresh == read_golden() else "STALE")
