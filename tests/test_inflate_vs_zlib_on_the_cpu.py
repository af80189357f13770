"""The deflate decoders against zlib on hand-forged streams (tests/deflate_forge.py), on the CPU.

zlib's own encoder never emits literal-only blocks, deep codes, HCLEN = 4 or repeat codes across the HLIT -> HDIST boundary;
other encoders do.  Every decoder of the project sees the same forged streams: the GPU inflater's decoder
(csrc/kmm_gpu_inflate.hpp, compiled with g++; also under ASan / UBSan), the plain-gzip pipeline (csrc/kmm_gpu_gunzip.hpp
through tests/gunzip_cpu_driver.hpp) and the host reader (csrc/kmm_inflate.hpp in libkmm_io, through a .gz file).

The rule: each decoder's outcome equals zlib's — the very same bytes with nothing written behind them, or a refusal where zlib
refuses.  A refusal of the GPU decoder is an error code, never a stray access.  Incomplete codes follow zlib's rule: a
literal / length or distance code may be ONE code of length 1, and a distance code may be empty (a literal-only block);
every other incomplete code is refused.
"""
import ctypes
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from tests import deflate_forge as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
SEEDS = [int(x) for x in os.environ.get("KMM_FUZZ_SEEDS", "1,2").split(",")]

SHIM = ('#include "kmm_gpu_inflate.hpp"\n#include <vector>\n'
        'extern "C" int gz_stream(const uint8_t *in, uint32_t n_in, uint8_t *out, uint32_t n_out) {\n'
        '    std::vector<uint16_t> prim(kmm_gz::PRIM_WORDS), sec(kmm_gz::SEC_WORDS); std::vector<uint64_t> list(kmm_gz::LIST_ALLOC);\n'
        '    return kmm_gz::inflate_stream(in, n_in, out, n_out, prim.data(), sec.data(), list.data()); }\n'
        'extern "C" int gz_const(int which) {\n'
        '    const int v[4] = {kmm_gz::LIT_PB, kmm_gz::DIST_PB, kmm_gz::SEC_LIT, kmm_gz::SEC_DIST}; return v[which]; }\n')


@pytest.fixture(scope="module")
def gz(tmp_path_factory):
    d = tmp_path_factory.mktemp("forge")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = str(d / "shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.gz_stream.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
    return lib


@pytest.fixture(scope="module")
def gunzip(tmp_path_factory):
    from tests.test_gpu_gunzip_on_the_cpu import _build, _load
    return _load(_build(tmp_path_factory.mktemp("forge_gunzip"), "shim"))


@pytest.fixture(scope="module")
def cat():
    return {name: (F.stream(blocks, tail), blocks) for name, (blocks, tail) in F.catalogue().items()}


def zlib_raw(raw):
    """zlib's bytes for a raw deflate stream, or None: refused, or the stream ends before its final block."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(raw)
    except zlib.error:
        return None
    return out if d.eof else None


def zlib_gzip(blob):
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(blob)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data else None


def claimed_size(expect, blocks):
    """The output size the decoder is told: zlib's when zlib inflates the stream, else what the symbols spell out (so that a
    decoder which wrongly accepts the stream cannot hide behind a size mismatch)."""
    if expect is not None:
        return len(expect)
    e = F.expand(blocks)
    return len(e) if e is not None else 1000


def check_gpu_decoder(gz, raw, blocks, what):
    expect = zlib_raw(raw)
    n = claimed_size(expect, blocks)
    out = np.full(n + 16, 0xA5, np.uint8)
    rc = gz.gz_stream(raw, len(raw), out.ctypes.data, n)
    assert (out[n:] == 0xA5).all(), ("a byte written behind the output", what)
    if expect is None:
        assert rc != 0, ("accepted a stream zlib refuses", what)
        assert 1 <= rc <= 11, (what, rc)
    else:
        assert rc == 0, ("refused a stream zlib inflates", what, rc)
        assert out[:n].tobytes() == expect, ("bytes differ from zlib's", what)
    return expect


NAMED = ["literal_only_hdist1", "literal_only_hdist30", "one_dist_code_len1", "one_dist_code_len1_symbol9",
         "one_dist_code_len2", "one_dist_code_len15", "two_dist_codes_len3", "one_lit_code_eob_len2",
         "dist_1040_issue_0", "dist_1040_issue_1", "dist_1040_search_0", "lit_404_0", "lit_404_1", "hclen4", "hclen19",
         "rle18_crosses", "rle17_crosses", "rle16_crosses", "rle18_overshoots", "rle16_overshoots", "rle16_first",
         "len258_sym285", "sym284_extra31", "dist32768_at_32k", "dist32768_at_32k_minus1", "dist_before_start",
         "fixed_lit286", "fixed_lit287", "fixed_dist30", "fixed_dist31", "stored_nlen_mismatch", "stored_beyond_input",
         "empty_dynamic_eob_only", "empty_dynamic_two_codes", "empty_fixed_then_stored_empty", "blocks_reach_back_greedy",
         "blocks_reach_back_maxdist", "bytes_after_final", "no_final_block", "reserved_btype"]

# what zlib says about the named shapes (pins the forge: each case really is the shape its name says)
ZLIB_ACCEPTS = {"literal_only_hdist1", "literal_only_hdist30", "one_dist_code_len1", "one_dist_code_len1_symbol9",
                "dist_1040_issue_0", "dist_1040_issue_1", "dist_1040_search_0", "lit_404_0", "lit_404_1", "hclen19",
                "rle18_crosses", "rle17_crosses", "rle16_crosses", "len258_sym285", "sym284_extra31", "dist32768_at_32k",
                "empty_dynamic_eob_only", "empty_dynamic_two_codes", "empty_fixed_then_stored_empty", "blocks_reach_back_greedy",
                "blocks_reach_back_maxdist", "bytes_after_final"}


@pytest.mark.parametrize("name", NAMED)
def test_named_shape_inflates_like_zlib(gz, cat, name):
    raw, blocks = cat[name]
    expect = check_gpu_decoder(gz, raw, blocks, name)
    assert (expect is not None) == (name in ZLIB_ACCEPTS), name
    if expect is not None:
        assert expect == F.expand(blocks)


def test_whole_catalogue_inflates_like_zlib(gz, cat):
    """Every shape of the catalogue (overlaps at distance 1 .. 16, stored blocks of 0 and 65 535 bytes at every bit offset,
    the worst subtable shapes in three symbol orders, ...)."""
    for name, (raw, blocks) in cat.items():
        check_gpu_decoder(gz, raw, blocks, name)
    for off in range(8):
        for n in (0, 65535):
            assert zlib_raw(cat["stored%d_bitoff%d" % (n, off)][0]) is not None


@pytest.mark.parametrize("seed", SEEDS)
def test_random_valid_streams_inflate_like_zlib(gz, seed):
    """A few thousand random valid streams per seed (KMM_FUZZ_SEEDS): random parses and block splits, random complete codes
    weighted towards depth 12-15 and the worst subtable shapes."""
    rng = random.Random(9000 + seed)
    src = bytes(rng.choice(b"ACGTN\n@+FFFF:,#") for _ in range(6000)) + bytes(rng.randrange(256) for _ in range(2000))
    n_deep = 0
    for i in range(1500):
        a = rng.randrange(len(src))
        data = (src[a:] + src)[:rng.choice([0, 1, 17, 300, 2000, 8000])]
        raw, blocks = F.random_stream(rng, data)
        assert zlib_raw(raw) == data, i
        check_gpu_decoder(gz, raw, blocks, (seed, i))
        n_deep += any(b.kind == "dynamic" and max(b.lit_lens + b.dist_lens) >= 12 for b in blocks)
    assert n_deep > 300


def test_refusals_under_damage_of_forged_streams(gz, cat):
    """Damaged forged streams: a refusal where zlib refuses, zlib's bytes where it does not."""
    rng = random.Random(77)
    names = sorted(n for n in cat if n in ZLIB_ACCEPTS)
    for trial in range(600):
        raw, blocks = cat[names[trial % len(names)]]
        b = bytearray(raw)
        if len(b) < 2:
            continue
        p = rng.randrange(len(b))
        if trial % 3 == 0:
            b[p] ^= 1 << rng.randrange(8)
        elif trial % 3 == 1:
            del b[p:]
        else:
            b[p:p + 4] = bytes(rng.randrange(256) for _ in range(len(b[p:p + 4])))
        expect = zlib_raw(bytes(b))
        n = len(expect) if expect is not None else len(F.expand(blocks) or b"")
        out = np.full(n + 16, 0xA5, np.uint8)
        rc = gz.gz_stream(bytes(b), len(b), out.ctypes.data, n)
        assert (out[n:] == 0xA5).all(), trial
        if rc == 0:
            assert expect is not None and out[:n].tobytes() == expect, ("accepted what zlib refuses / other bytes", trial)


def _gzip_cases(cat, rng, n_random):
    cases = []
    for name, (raw, blocks) in sorted(cat.items()):
        if name in ("bytes_after_final", "no_final_block"):
            continue                                  # (in a gzip member: the trailer would not follow the final block)
        e = F.expand(blocks)
        cases.append((name, F.gzip_member(raw, e if e is not None else b"")))
    src = bytes(rng.choice(b"ACGT\n@+F:#") for _ in range(20000))
    for i in range(n_random):
        data = src[rng.randrange(5000):][:rng.choice([100, 3000, 15000])]
        raw, _ = F.random_stream(rng, data)
        cases.append(("random%d" % i, F.gzip_member(raw, data, fname=b"r.fq" if i % 3 == 0 else None)))
    return cases


def test_gzip_pipeline_on_forged_members(gunzip, cat):
    """The plain-gzip pipeline (csrc/kmm_gpu_gunzip.hpp: speculative chunk starts, markers, windows): every forged shape as a
    gzip member, cut into windows at varied points and decoded in chunks of varied size; and all valid ones as ONE file of
    concatenated members."""
    from tests.test_gpu_gunzip_on_the_cpu import _run
    rng = random.Random(5)
    good = []
    for name, blob in _gzip_cases(cat, rng, 60):
        expect = zlib_gzip(blob)
        for chunk in (1024, 4096, 65536):
            cuts = sorted(rng.randrange(1, len(blob)) for _ in range(rng.randint(0, 3))) if len(blob) > 2 else []
            rc, out, _ = _run(gunzip, blob, cuts=cuts, chunk=chunk)
            if expect is None:
                assert rc != 0, ("accepted a member zlib refuses", name, chunk)
            else:
                assert rc == 0 and out == expect, (name, chunk, rc)
        if expect is not None:
            good.append((blob, expect))
    blob = b"".join(g[0] for g in good)
    rc, out, st = _run(gunzip, blob, cuts=[len(blob) // 3, len(blob) // 2], chunk=2048)
    assert rc == 0 and out == b"".join(g[1] for g in good) and st[3] == len(good)


def test_host_reader_on_forged_members(cat, tmp_path, monkeypatch):
    """The host reader (libkmm_io: csrc/kmm_inflate.hpp's speculative many-thread decoder) on every forged shape as a .gz file."""
    from kmer_mapper_amd import _io
    _io.build()
    monkeypatch.setenv("KMM_IO_GZIP_CHUNK", "1024")
    rng = random.Random(6)
    path = str(tmp_path / "f.gz")
    for name, blob in _gzip_cases(cat, rng, 30):
        expect = zlib_gzip(blob)
        open(path, "wb").write(blob)
        for n_threads in (4, 1):
            try:
                with _io.NativeStream(path, n_threads) as s:
                    got = bytearray()
                    while True:
                        piece = s.read(1 << 20)
                        if not piece:
                            break
                        got += piece
            except (ValueError, EOFError):
                assert expect is None, ("the host reader refused a member zlib inflates", name, n_threads)
                continue
            assert expect is not None and bytes(got) == expect, ("the host reader's bytes differ from zlib's", name, n_threads)


def test_forged_streams_under_the_sanitizers(tmp_path, cat):
    """The GPU decoder on every catalogue shape and on random valid and damaged streams, built with ASan + UBSan
    (tests/gz_cases_san_main.cpp: exact-size heap buffers, the output's slack checked): zlib's outcome, no report."""
    exe = str(tmp_path / "gz_cases")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I" + CSRC,
           os.path.join(ROOT, "tests", "gz_cases_san_main.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    rng = random.Random(11)
    cases = [(raw, blocks) for raw, blocks in cat.values()]
    src = bytes(rng.choice(b"ACGT\n@+F:#") for _ in range(9000))
    for i in range(300):
        raw, blocks = F.random_stream(rng, src[rng.randrange(3000):][:rng.choice([0, 50, 4000])])
        if i % 2:
            b = bytearray(raw)
            if b:
                b[rng.randrange(len(b))] ^= 1 << rng.randrange(8)
            raw = bytes(b)
        cases.append((raw, blocks))
    expects = [zlib_raw(raw) for raw, _ in cases]
    sizes = [claimed_size(e, blocks) for e, (_, blocks) in zip(expects, cases)]
    with open(tmp_path / "cases.bin", "wb") as f:
        for (raw, _), n in zip(cases, sizes):
            f.write(np.array([len(raw), n], np.uint32).tobytes() + raw)
    run = subprocess.run([exe, str(tmp_path / "cases.bin"), str(tmp_path / "res.bin")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "ERROR" not in run.stderr, (run.stdout + run.stderr)[-3000:]
    res = open(tmp_path / "res.bin", "rb").read()
    p = 0
    for i, (e, n) in enumerate(zip(expects, sizes)):
        rc, n2 = np.frombuffer(res[p:p + 8], np.int32)[0], int(np.frombuffer(res[p + 4:p + 8], np.uint32)[0])
        out = res[p + 8:p + 8 + n2]
        p += 8 + n2
        assert n2 == n
        if e is None:
            assert rc != 0 or i >= len(cat), ("accepted a stream zlib refuses", i)
        else:
            assert rc == 0 and out == e, ("differs from zlib", i, rc)
    assert p == len(res)


# ---------------------------------------------------------------- the subtables' bounds
def _all_complete_counts(n_max, maxlen=15):
    """Every complete code of at most n_max symbols as counts per length 1..maxlen (brute force)."""
    out = []

    def rec(l, left, syms, counts):
        if l > maxlen:
            return
        for c in range(0, min(left, syms) + 1):
            cc = counts + [c]
            if c == left:
                out.append(cc + [0] * (maxlen - l))
            elif 2 * (left - c) <= syms - c:
                rec(l + 1, 2 * (left - c), syms - c, cc)

    rec(1, 2, n_max, [])
    return out


def test_bound_search_matches_brute_force():
    """The memoized search (deflate_forge.worst_code) against every complete code of up to 9 symbols enumerated outright, at
    several primary widths: the same maximum."""
    for n in (2, 5, 9):
        codes = _all_complete_counts(n)
        for root in (1, 2, 3, 5):
            brute = max(F.subtable_entries(F.lengths_from_counts(c, sum(c), list(range(sum(c)))), root) for c in codes)
            assert F.worst_code(n, root)[0] == brute, (n, root)


def test_subtables_cover_the_proven_bounds(gz):
    """Every valid distance code (at most 30 symbols, 1..15 bits, and the incomplete ones the decoder accepts: one code of
    length 1, or none) and literal / length code (at most 286 symbols; the fixed code has 288 but needs no subtable at 8
    primary bits) needs at most worst_code() subtable entries — 1040 behind a 5-bit and 404 behind an 8-bit primary table.
    The decoder's SEC_DIST / SEC_LIT must hold them, and the link's 11-bit offset / 4-bit width must address them."""
    lit_pb, dist_pb, sec_lit, sec_dist = (gz.gz_const(i) for i in range(4))
    lit_bound, lit_counts = F.worst_code(286, lit_pb)
    dist_bound, dist_counts = F.worst_code(30, dist_pb)
    assert (lit_pb, dist_pb) != (8, 5) or (lit_bound, dist_bound) == (404, 1040)
    assert F.subtable_entries(F.lengths_from_counts(lit_counts, 286, list(range(286))), lit_pb) == lit_bound
    assert F.subtable_entries(F.lengths_from_counts(dist_counts, 30, list(range(30))), dist_pb) == dist_bound
    assert F.subtable_entries(F.lengths_from_counts(F.WORST_DIST_COUNTS, 30, list(range(30))), 5) == 1040
    assert F.subtable_entries(F.FIXED_LIT, lit_pb) <= lit_bound and F.subtable_entries(F.FIXED_DIST, dist_pb) <= dist_bound
    assert sec_lit >= lit_bound, (sec_lit, lit_bound)
    assert sec_dist >= dist_bound, (sec_dist, dist_bound)
    assert max(lit_bound, dist_bound) <= 2048 and 15 - min(lit_pb, dist_pb) <= 15
