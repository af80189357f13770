"""CPU tier of the BGZF writer (include/kmm.h COMPRESSED OUTPUT): csrc/kmm_bgzf_out.hpp compiled with g++ -Wall
-Wextra -Werror and driven the way the kernel walks a member (tests/bgzf_out_cpu_driver.hpp).  Every case of
tests/bgzf_out_cases.py round-trips through zlib — member by member (zlib.decompressobj(-15) consumes exactly the deflate
bytes; BSIZE, CRC32, ISIZE) and whole (gzip) — and keeps the conditions derived in the issue: no member above n + 31, random
A/C/G/T lines at or below 0.30, a repeated record at or below 0.05, random bytes stored.  Once more under ASan + UBSan as a
stand-alone executable.  tests/golden/bgzf_out_expected.json, which ties the GPU kernel to this build, must be current.

The code-length limit.  The case with byte frequencies F(1) .. F(22) has an unlimited BYTE code 21 deep, but a deflate block never
codes the bytes alone: the end-of-block symbol is a 23rd leaf of frequency 1, and with three leaves of frequency 1 two chains grow
side by side — the Huffman code of F(1) .. F(22) and one more 1 is 12 deep (test_the_fibonacci_cases_and_the_code_length_limit
builds both codes with heapq).  No deflater that writes one block per member reaches the 15-bit limit on that text, with or
without matches; this one reports 14 and no limiter (the parse takes repeats: two of the 22 letters are 62 % of the text).  The
text stays in the catalogue and round-trips like the others.  The limiter is reached where it can be: by build_code on the 22
frequencies themselves (21 deep, limited, Kraft sum exactly 1) and, inside a member, by a text built so that the end-of-block
symbol is the chain's first link (tests/bgzf_out_cases.limited_text: deeper than 15, limited, round trip, in the golden file for
the GPU) — the driver's report is asserted on both texts.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import bgzf_out_cases as bc

ROOT = bc.ROOT
CASES = bc.all_cases()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return bc.build_cpu_lib(tmp_path_factory.mktemp("bgzf_out"))


@pytest.fixture(scope="module")
def results(lib):
    """name -> (members, sizes, stats) of the CPU build, computed once."""
    return {name: bc.cpu_compress(lib, text) for name, text in CASES.items()}


def test_the_catalogue_holds_what_the_issue_lists():
    assert [len(CASES["seam_%d" % n]) for n in bc.SEAMS] == list(bc.SEAMS)
    assert len(CASES["fibonacci_frequencies"]) == 46367
    counts = np.bincount(np.frombuffer(CASES["fibonacci_frequencies"], dtype=np.uint8))
    assert sorted(counts[counts > 0].tolist()) == sorted(bc.FIB)
    text = CASES["no_repeated_4_bytes"]
    grams = {text[i:i + 4] for i in range(len(text) - 3)}
    assert len(grams) == len(text) - 3 and len(set(text)) == 16
    head = CASES["window_edge_32768"]
    assert head[32768:] == head[:64] and CASES["window_edge_32769"][32769:] == head[:64]
    assert set(CASES["one_distinct_byte_65280"]) == {ord("G")} and len(CASES["poly_a"]) == 70000
    assert len(set(CASES["fastq_uniform_41_quals"].split(b"\n")[3])) > 30
    for length in (258, 300):
        for where, at in (("at_a_segment_start", 255 * 8), ("across_a_segment_end", 255 * 8 + 100)):
            t = CASES["repeat_%d_%s" % (length, where)]
            assert t[at:at + length] == t[100:100 + length] and t[at + length] != t[100 + length]


@pytest.mark.parametrize("name", list(CASES))
def test_cases_round_trip_through_zlib(results, name):
    data, sizes, _ = results[name]
    text = CASES[name]
    assert bc.check_stream(data, text) == sizes
    assert len(data) <= bc.bound(len(text))


def test_bound_and_capacity(lib):
    assert [lib.bgzf_out_bound_cpu(n) for n in (-1, 0, 1, 65280, 65281)] == [-1, 0, 32, 65311, 65343]
    text = CASES["seam_65281"]
    assert bc.cpu_compress(lib, text, capacity=bc.bound(len(text)) - 1) is None
    assert bc.cpu_compress(lib, b"")[0] == b""


def test_derived_conditions(results):
    ratio = lambda name: len(results[name][0]) / len(CASES[name])
    # {A, C, G, T, '\n', end-of-block}: code lengths 2, 2, 2, 3, 4, 4 -> 2.26 bits a byte, 0.283 with the header; a parser
    # that takes four-byte matches blindly is above 0.30
    assert ratio("random_acgt_lines") <= 0.30
    # one match token of about 3 bytes per 255-byte segment: 0.012 plus the header; a match finder that finds nothing is above
    assert ratio("one_record_repeated") <= 0.05
    data, sizes, stats = results["random_bytes"]
    n = len(CASES["random_bytes"])
    assert stats[2] == len(sizes) == 3 and sizes == [65280 + 31, 65280 + 31, n - 2 * 65280 + 31]
    # the matches are found and are long: poly-A and the single byte are a few hundred bytes a member
    assert ratio("poly_a") <= 0.02 and ratio("one_distinct_byte_65280") <= 0.02
    # the repeat at distance 32768 is taken, the one at 32769 cannot be: the second text is one byte longer and costs more than that
    assert len(results["window_edge_32769"][0]) - len(results["window_edge_32768"][0]) > 8
    assert results["no_repeated_4_bytes"][2][2] == 0                               # (dynamic, not stored)


def _huffman_depth(freq):
    """The deepest leaf of a Huffman code of these frequencies (heapq; ties merge the shallower trees first)."""
    import heapq
    heap = [(f, 0) for f in freq]
    heapq.heapify(heap)
    while len(heap) > 1:
        (fa, da), (fb, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (fa + fb, max(da, db) + 1))
    return heap[0][1]


def test_the_fibonacci_cases_and_the_code_length_limit(results):
    """The driver reports the deepest unlimited literal / length code and whether the limiter ran.  On the text with byte
    frequencies F(1) .. F(22) the bytes alone would be 21 deep, but beside the end-of-block symbol they are 12 deep: the limit
    cannot be reached there, and the report must say so.  On the text whose chain starts at the end-of-block symbol the code is
    deeper than 15 and the limiter ran, so the limiter cannot go untested."""
    assert _huffman_depth(bc.FIB) == 21 and _huffman_depth(bc.FIB + [1]) == 12
    deepest, limited, stored = results["fibonacci_frequencies"][2]
    print("fibonacci_frequencies: deepest unlimited code %d, members limited %d, stored %d" % (deepest, limited, stored))
    assert stored == 0 and 1 <= deepest <= 285 and limited == (1 if deepest > 15 else 0)
    assert _huffman_depth(bc.FIB[:21]) == 20                                       # F(2) .. F(21) and the end-of-block symbol
    text = CASES["fibonacci_literals_beside_the_end_of_block"]
    assert len(text) <= bc.BLOCK
    deepest, limited, stored = results["fibonacci_literals_beside_the_end_of_block"][2]
    print("fibonacci_literals_beside_the_end_of_block: deepest unlimited code %d, members limited %d" % (deepest, limited))
    assert deepest > 15 and limited == 1 and stored == 0


def test_the_limiter_on_fibonacci_frequencies(tmp_path):
    """build_code on the frequencies F(1) .. F(22) themselves, in rising and in falling symbol order: 21 deep before the
    limit, every length at most 15 behind it, the code complete (Kraft sum exactly 1), rarer symbols never shorter, and
    canonical: zlib inflates a block written with it."""
    src = tmp_path / "code.cpp"
    src.write_text('#include "bgzf_out_cpu_driver.hpp"\n'
                   'extern "C" uint32_t code_lengths(const uint32_t *freq, uint32_t n, uint32_t max_bits, uint8_t *len, uint16_t *code,\n'
                   '                                 uint32_t *stats)\n'
                   '{\n'
                   '    std::vector<uint32_t> sorted(n), scr(6 * (size_t)n + 64);\n'
                   '    for (uint32_t s = 0; s < n; ++s)\n'
                   '        kmm_bz::rank_symbol(freq, n, s, sorted.data());\n'
                   '    return kmm_bz::build_code(freq, n, kmm_bz::count_nonzero(freq, n), sorted.data(), max_bits, scr.data(), len, code,\n'
                   '                              stats[0], stats[1]);\n'
                   '}\n')
    so = str(tmp_path / "code.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + bc.CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.code_lengths.restype = ctypes.c_uint32
    lib.code_lengths.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    for fib, want_depth in ((bc.FIB, 21), (bc.FIB[::-1], 21)):
        freq = np.array(fib + [0, 0], dtype=np.uint32)
        n = len(freq)
        lens, codes, stats = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint16), np.zeros(2, dtype=np.uint32)
        last = lib.code_lengths(freq.ctypes.data, n, 15, lens.ctypes.data, codes.ctypes.data, stats.ctypes.data)
        used = lens[freq > 0].astype(int)
        assert last == n - 2 and not lens[freq == 0].any()
        assert stats.tolist() == [want_depth, 1] and used.max() == 15 and used.min() >= 1
        assert sum(2 ** (15 - l) for l in used) == 2 ** 15
        order = np.lexsort((np.arange(n), freq))
        by_rarity = lens[order][freq[order] > 0].astype(int)
        assert (np.diff(by_rarity) <= 0).all()
        # canonical, bit-reversed: consecutive codes within a length, in symbol order
        plain = [int(format(int(c), "0%db" % l)[::-1], 2) for c, l in zip(codes, lens) if l]
        nxt, code = {}, 0
        counts = np.bincount(lens, minlength=17)
        counts[0] = 0
        for bits in range(1, 16):
            code = (code + counts[bits - 1]) << 1
            nxt[bits] = code
        for c, l in zip(plain, [int(l) for l in lens if l]):
            assert c == nxt[l]
            nxt[l] += 1
    # without a limit to reach nothing is limited and the depth is the code's
    freq = np.array([5, 9, 12, 13, 16, 45], dtype=np.uint32)
    lens, codes, stats = np.zeros(6, dtype=np.uint8), np.zeros(6, dtype=np.uint16), np.zeros(2, dtype=np.uint32)
    lib.code_lengths(freq.ctypes.data, 6, 15, lens.ctypes.data, codes.ctypes.data, stats.ctypes.data)
    assert lens.tolist() == [4, 4, 3, 3, 3, 1] and stats.tolist() == [4, 0]


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, results):
    """The same driver as an executable with ASan + UBSan (tests/bgzf_out_san_main.cpp; host code, nothing sanitized is loaded
    into Python): every member's bytes, the workgroup state, the candidates and the slots in heap blocks of exactly their size.
    Its output is the shared library's."""
    exe = str(tmp_path / "bgzf_out_san")
    src = os.path.join(ROOT, "tests", "bgzf_out_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + bc.CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("the sanitizer runtimes are not installed")
    assert build.returncode == 0, build.stderr
    t_path, o_path = str(tmp_path / "text.bin"), str(tmp_path / "out.bin")
    for name, text in CASES.items():
        open(t_path, "wb").write(text)
        run = subprocess.run([exe, t_path, o_path], capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stdout, run.stderr)
        data, sizes, stats = results[name]
        assert run.stdout.split() == ["ok", str(len(text)), str(len(data)), str(len(sizes))] + [str(x) for x in stats]
        assert open(o_path, "rb").read() == data


def test_the_golden_file_is_current(results):
    """tests/golden/bgzf_out_expected.json is what this build gives (python -m tests.bgzf_out_cases --write renews it)."""
    golden = bc.read_golden()
    assert sorted(golden) == sorted(CASES)
    for name, (data, sizes, _) in results.items():
        assert golden[name] == {"sizes": sizes, "sha256": hashlib.sha256(data).hexdigest()}, name


def test_the_command_line_knows_the_flag():
    from kmer_mapper_amd.command_line_interface import build_argument_parser
    common = ["select-reads", "-i", "x.npz", "-f", "r.fq", "-o", "kept.fq.gz", "-k", "31"]
    assert build_argument_parser().parse_args(common + ["--bgzf"]).bgzf is True
    assert not hasattr(build_argument_parser().parse_args(common), "bgzf")         # (a name that ends in .gz still gets text)
    from kmer_mapper_amd import gz_io
    assert gz_io.BGZF_EOF == bc.EOF_BLOCK and len(gz_io.BGZF_EOF) == 28
