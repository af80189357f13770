"""CPU tier of kmm_map_gzip: csrc/kmm_gpu_gunzip.hpp — the speculative plain-gzip inflater the GPU runs (find, decode with
markers, accept / continue, the window chain, resolve, CRC32 / ISIZE) — compiled by itself with g++ and driven through the
very same orchestration (run_call) on the CPU, against zlib's bytes; damaged streams end in an error code; once more under
AddressSanitizer + UndefinedBehaviorSanitizer with buffers of exactly the right size."""
import ctypes
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")

SHIM = '#include "gunzip_cpu_driver.hpp"\n'   # (the driver: tests/gunzip_cpu_driver.hpp, shared with gunzip_san_main.cpp)


def _build(tmp_path, name, extra=()):
    src = tmp_path / (name + ".cpp")
    src.write_text(SHIM)
    so = str(tmp_path / (name + ".so"))
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", *extra, "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                           str(src), "-o", so])
    return so


def _load(so):
    lib = ctypes.CDLL(so)
    lib.gunzip_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint64,
                               ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    return lib


def _run(lib, comp, cuts=None, chunk=32768, cap=None, call_cap=1 << 40):
    cuts = sorted(set([c for c in (cuts or []) if 0 < c < len(comp)] + [len(comp)]))
    cap = cap if cap is not None else 64 << 20
    out = np.zeros(cap + 1, np.uint8)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 6)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = lib.gunzip_cpu(comp, len(comp), c, len(cuts), chunk, call_cap, out.ctypes.data, cap, ctypes.byref(on), st)
    return rc, out[:on.value].tobytes(), list(st)


def _fastq(n, rng, names=None):
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    qual = np.frombuffer(b"FFFFFF:,#", dtype=np.uint8)
    return b"".join(b"@" + (names[i] if names else b"SRR1.%d %d/1" % (i, i)) + b"\n" + bytes(rng.choice(acgt, size=150)) + b"\n+\n" +
                    bytes(rng.choice(qual, size=150)) + b"\n" for i in range(n))


def _gzip(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    return c.compress(data) + c.flush()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return _load(_build(tmp_path_factory.mktemp("gunzip"), "shim"))


@pytest.fixture(scope="module")
def data():
    return _fastq(4000, np.random.default_rng(51))


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED])
@pytest.mark.parametrize("mem", [1, 8, 9])
def test_levels_strategies_and_memlevels_inflate_like_zlib(lib, data, level, strategy, mem):
    comp = _gzip(data, level, strategy, mem)
    for chunk in (1024, 65536):
        rc, out, st = _run(lib, comp, chunk=chunk)
        assert rc == 0 and out == data, (chunk, rc)
        assert st[3] == 1


def test_chunk_spacings_and_windows(lib, data):
    comp = _gzip(data * 3, 6)
    rng = np.random.default_rng(52)
    for chunk in (1024, 2048, 4096, 16384, 32768, 65536):
        rc, out, st = _run(lib, comp, chunk=chunk)
        assert rc == 0 and out == data * 3, chunk
        if chunk == 1024:
            assert st[0] > 20                                   # (one chunk per deflate block, roughly)
    for n_win in (3, 7, 20):
        cuts = [int(x) for x in rng.integers(1, len(comp), size=n_win - 1)]
        rc, out, _ = _run(lib, comp, cuts=cuts, chunk=2048)
        assert rc == 0 and out == data * 3, n_win


def test_concatenated_members_with_header_fields_and_padding(lib, data):
    parts = [data[:100_000], data[100_000:100_001], data[100_001:700_000], data[700_000:]]
    hdr = b"\x1f\x8b\x08\x1e\x00\x00\x00\x00\x00\x03" + b"\x06\x00AB\x02\x00xy" + b"reads.fq\x00" + b"comment\x00"
    m2 = hdr + (zlib.crc32(hdr) & 0xFFFF).to_bytes(2, "little") + _gzip(parts[2], 9)[10:]
    comp = gzip.compress(parts[0], 1) + gzip.compress(parts[1], 6) + m2 + gzip.compress(parts[3], 0) + b"\x00" * 50
    for chunk in (1024, 32768):
        rc, out, st = _run(lib, comp, chunk=chunk)
        assert rc == 0 and out == data and st[3] == 4, chunk
    rc, out, st = _run(lib, comp, cuts=[len(comp) // 3, len(comp) // 2, len(comp) - 60], chunk=1024)
    assert rc == 0 and out == data and st[3] == 4
    many = b"".join(gzip.compress(data[i:i + 3000], 6) for i in range(0, 120_000, 3000))   # more members than a piece records
    rc, out, st = _run(lib, many, chunk=65536)
    assert rc == 0 and out == data[:120_000] and st[3] == 40


def test_stored_only_members_and_empty_ones(lib, data):
    for comp in (gzip.compress(data, 0), gzip.compress(b"", 6), gzip.compress(b"", 6) + gzip.compress(data[:5000], 0)):
        expect = zlib.decompress(comp, 31) if len(comp) > 30 and comp[3] == 0 and comp.count(b"\x1f\x8b") == 1 else None
        rc, out, _ = _run(lib, comp, chunk=1024)
        assert rc == 0
        assert out == gzip.decompress(comp) if expect is None else out == expect


def _false_start_data(rng):
    blobs, seed = [], 0
    while len(blobs) < 8:
        seed += 1
        r = np.random.default_rng(seed)
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        b = c.compress(bytes(r.choice(np.frombuffer(b"ACGTacgt:#", dtype=np.uint8), size=4000))) + c.flush(zlib.Z_FULL_FLUSH)
        b = b[:160]
        if b"\n" not in b and (b[0] & 7) == 4:
            blobs.append(b)
    return _fastq(1500, rng, [b"r%d " % i + blobs[i % 8] for i in range(1500)])


def test_a_false_start_is_rejected(lib):
    """A level-0 member whose FASTQ header lines carry the raw bytes of real dynamic blocks: the search finds them, the
    predecessor check rejects every one."""
    raw = _false_start_data(np.random.default_rng(53))
    comp = gzip.compress(raw, 0)
    rc, out, st = _run(lib, comp, chunk=1024)
    assert rc == 0 and out == raw
    assert st[1] >= 1


def test_slots_that_run_full_are_continued(lib):
    rec = b"@same\n" + b"ACGT" * 40 + b"\n+\n" + b"F" * 160 + b"\n"
    raw = rec * 40000
    rc, out, st = _run(lib, _gzip(raw, 9), cap=len(raw) + 16)
    assert rc == 0 and out == raw and st[2] >= 1


def test_damage_ends_in_an_error_code(lib, data):
    comp = _gzip(data, 6)
    rng = np.random.default_rng(54)
    assert _run(lib, comp[:-100])[0] != 0                       # truncated
    assert _run(lib, comp[:-3])[0] != 0                         # truncated trailer
    assert _run(lib, comp + b"garbage")[0] != 0                 # trailing bytes that are no member
    bad = bytearray(comp)
    bad[-8] ^= 1
    assert _run(lib, bytes(bad))[0] == 11                       # CRC32
    bad = bytearray(comp)
    bad[-4] ^= 1
    assert _run(lib, bytes(bad))[0] == 10                       # ISIZE
    bad = bytearray(comp)
    bad[0] ^= 1
    assert _run(lib, bytes(bad))[0] != 0                        # header
    for _ in range(60):                                         # bit flips anywhere: an error code, or (never) wrong bytes
        bad = bytearray(comp)
        bad[int(rng.integers(10, len(comp) - 8))] ^= 1 << int(rng.integers(0, 8))
        rc, out, _ = _run(lib, bytes(bad), chunk=int(rng.choice([1024, 32768])))
        assert rc != 0 or out == data


def test_calls_stop_at_their_size_limit(lib, data):
    """A per-call cap of a few chunks' output: every call ends in front of the chunk that would pass it (or, when the first
    chunk alone does, where its pieces stopped), the next call goes on there — the same bytes in many more calls."""
    comp = _gzip(data * 2, 6)
    rc0, out0, st0 = _run(lib, comp, chunk=1024)
    assert rc0 == 0 and out0 == data * 2 and st0[5] == 0
    for call_cap in (300_000, 70_000, 5_000):
        for cuts in (None, [len(comp) // 3, 2 * len(comp) // 3]):
            rc, out, st = _run(lib, comp, cuts=cuts, chunk=1024, call_cap=call_cap)
            assert rc == 0 and out == data * 2, (call_cap, cuts, rc)
            assert st[5] >= 1 and st[4] > st0[4] + 1, (call_cap, st)   # (more calls; one chunk per call at the smallest cap)
    rec = b"@same\n" + b"ACGT" * 40 + b"\n+\n" + b"F" * 160 + b"\n"
    raw = rec * 100000                                            # blocks of ~4 MB, continued in pieces, cut at the cap
    rc, out, st = _run(lib, _gzip(raw, 9), call_cap=1_000_000, cap=len(raw) + 16)
    assert rc == 0 and out == raw and st[5] >= 1 and st[2] >= 1


def test_many_empty_members(lib):
    """Hundreds of empty members (each one fills the event list of a piece without output) and data behind them."""
    comp = gzip.compress(b"", 6) * 300 + gzip.compress(b"@r\nACGT\n+\nFFFF\n", 6)
    rc, out, st = _run(lib, comp, chunk=1024)
    assert rc == 0 and out == b"@r\nACGT\n+\nFFFF\n" and st[3] == 301


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same pipeline and driver built as an executable with ASan + UBSan (tests/gunzip_san_main.cpp; host code): zlib's
    streams of every level and strategy, concatenated members, false starts, small per-call caps, windows cut anywhere in
    exact-size buffers, damaged streams — exact bytes or an error code, no stray access, nothing reported."""
    exe = str(tmp_path / "gunzip_san")
    src = os.path.join(ROOT, "tests", "gunzip_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe, "-lz"]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=900)
    out = run.stdout + run.stderr
    assert run.returncode == 0 and "40 rounds" in run.stdout, out[-3000:]
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr, out[-3000:]
