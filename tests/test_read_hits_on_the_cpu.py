"""CPU tier of kmm_read_hits (include/kmm.h).  The catalogue's model (tests/read_hits_cases.py) against a second,
independent route — the oracle's extract -> in_index -> per-read sum, and for the reverse complement the OR over q and
oracle.revcomp(q) — the conditions that keep every case from being vacuous, the position -> read search of
csrc/kmm_read_hits.hpp compiled with g++ against brute force (once more under ASan + UBSan as a stand-alone executable), and the
command line's refusals."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import read_hits_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = rc.all_cases()
IDS = [c.name for c in CASES]
I64 = ctypes.c_int64


def _per_read(values, offsets, k):
    """values: one per k-mer, in (read, offset) order -> the sum per read"""
    n = np.maximum(np.diff(offsets) - k + 1, 0)
    ends = np.cumsum(n)
    cs = np.concatenate([[0], np.cumsum(values.astype(np.int64))])
    return (cs[ends] - cs[ends - n]).astype(np.uint32), n.astype(np.uint32)


@pytest.mark.parametrize("case", [c for c in CASES if c.lut is None], ids=[c.name for c in CASES if c.lut is None])
def test_model_agrees_with_extract_then_in_index(case, oracle):
    plain = case._replace(max_freq=rc.NO_FILTER, revcomp=False)
    hits, windows = rc.run_model(plain)
    kmers = oracle.extract(case.bases, case.offsets, case.k)
    want_hits, want_windows = _per_read(oracle.in_index(case.index, kmers), case.offsets, case.k)
    assert np.array_equal(windows, want_windows)
    assert np.array_equal(hits, want_hits)
    assert (hits <= windows).all()


@pytest.mark.parametrize("case", [c for c in CASES if c.rule == "revcomp"], ids=[c.name for c in CASES if c.rule == "revcomp"])
def test_model_agrees_with_the_or_over_both_orientations(case, oracle):
    hits, windows = rc.run_model(case)
    kmers = oracle.extract(case.bases, case.offsets, case.k)
    either = oracle.in_index(case.index, kmers) | oracle.in_index(case.index, oracle.revcomp(kmers, case.k))
    want_hits, want_windows = _per_read(either, case.offsets, case.k)
    assert np.array_equal(hits, want_hits) and np.array_equal(windows, want_windows)
    # every kind of window is there: only q, only the reverse complement, both
    fwd = oracle.in_index(case.index, kmers).astype(bool)
    rev = oracle.in_index(case.index, oracle.revcomp(kmers, case.k)).astype(bool)
    assert (fwd & ~rev).any() and (~fwd & rev).any() and (fwd & rev).any()
    if case.k % 2 == 0:
        assert (oracle.revcomp(kmers, case.k) == kmers)[fwd].any(), "a palindrome that is in the index"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_no_case_is_vacuous(case):
    hits, windows = rc.expected(case)
    assert (hits <= windows).all()
    assert rc.conditions(case, hits, windows) == []
    if case.rule is not None:
        h0, w0 = rc.run_model(rc.without_rule(case))
        assert not (np.array_equal(h0, hits) and np.array_equal(w0, windows)), "the rule changes nothing"
        if case.rule == "break":
            assert (windows < w0).any() and (windows <= w0).all()
        else:
            assert np.array_equal(windows, w0)


def test_the_catalogue_holds_what_the_seams_need():
    by_name = {c.name: c for c in CASES}
    ends = set(by_name["seams_k31"].offsets.tolist())
    for seam in (rc.LANE, rc.WAVE, rc.TILE, 2 * rc.TILE):
        assert {seam - 1, seam, seam + 1} <= ends
    lens = np.diff(by_name["seams_k31"].offsets)
    assert 3000 in lens and lens.max() > 2 * rc.TILE
    empty = np.diff(by_name["empty_reads_k31"].offsets) == 0
    assert empty[0] and empty[-1] and empty[1:-1].any()
    run = np.diff(np.nonzero(np.diff(np.concatenate([[0], empty.astype(np.int8), [0]])))[0])[::2].max()
    assert run >= 2000 > rc.TILE
    assert {rc.uniform_length(c) for c in CASES if c.name.startswith("uniform_")} == {15, 16, 150, 151, 1024, 1025}
    tiny = by_name["tiny_reads_k2"]
    assert (np.diff(tiny.offsets)[:700] <= 4).all()               # four reads and more inside one lane's positions
    large = by_name["large_uniform_40000x150_k31"]
    assert large.offsets.shape[0] == 40_001 and rc.uniform_length(large) == 150
    assert max(c.bases.shape[0] for c in CASES if c is not large) < 400_000


# ---------------------------------------------------------------------------------------------- the position -> read search
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("read_hits")
    src = tmp / "shim.cpp"
    src.write_text('#include "read_hits_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.read_hits_search_cpu.argtypes = [ctypes.c_void_p, I64, I64, I64, I64, ctypes.c_void_p]
    lib.read_hits_search_cpu.restype = I64
    return lib


def _brute(offsets, total):
    return np.minimum(np.searchsorted(offsets, np.arange(total), side="right") - 1, offsets.shape[0] - 2)


def _offset_sets():
    seen = {}
    for c in CASES:
        if c.bases.shape[0]:
            seen.setdefault(c.offsets.tobytes(), (c.name, c.offsets))
    return list(seen.values())


@pytest.mark.parametrize("name,offsets", _offset_sets(), ids=[n for n, _ in _offset_sets()])
def test_search_agrees_with_brute_force(lib, name, offsets):
    total, n_reads = int(offsets[-1]), offsets.shape[0] - 1
    want = _brute(offsets, total)
    for tile, lane in ((rc.TILE, rc.LANE), (8, 4), (4, 1)) if total < 100_000 else ((rc.TILE, rc.LANE),):
        got = np.full(total, -1, dtype=np.int64)
        outside = lib.read_hits_search_cpu(offsets.ctypes.data, n_reads, total, tile, lane, got.ctypes.data)
        assert outside == 0
        assert np.array_equal(got, want), (tile, lane, int(np.nonzero(got != want)[0][0]))


def test_search_stays_in_bounds_on_offsets_that_are_not_sorted(lib):
    """Decreasing offsets are refused after the kernels have run: every read id they produce must still be a valid index."""
    rng = np.random.default_rng(5)
    for n_reads in (1, 2, 7, 300):
        offsets = rng.integers(-50, 5000, size=n_reads + 1).astype(np.int64)
        offsets[0], offsets[-1] = 0, 3000
        got = np.full(3000, -1, dtype=np.int64)
        assert lib.read_hits_search_cpu(offsets.ctypes.data, n_reads, 3000, rc.TILE, rc.LANE, got.ctypes.data) == 0
        assert got.min() >= 0 and got.max() < n_reads


def test_search_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/read_hits_san_main.cpp; host code, nothing sanitized is loaded
    into Python): offsets and results live in heap buffers of exactly their size."""
    exe = str(tmp_path / "read_hits_san")
    src = os.path.join(ROOT, "tests", "read_hits_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    path = tmp_path / "offsets.bin"
    for name, offsets in _offset_sets():
        offsets.tofile(str(path))
        for tile, lane in ((rc.TILE, rc.LANE), (4, 1)):
            r = subprocess.run([exe, str(path), str(tile), str(lane)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            assert r.stdout.split() == ["ok", str(int(offsets[-1])), "0", "0"]


# ---------------------------------------------------------------------------------------------- the command line
def test_read_hits_refuses_sam_bam_and_several_ranks(tmp_path, monkeypatch):
    """Refused with a message that says so, before the index file is read (there is none)."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    batch = ReadBatch.from_strings(["ACGTACGTAC", "GGGTTTAAAC"])
    sam, bam, fq = str(tmp_path / "r.sam"), str(tmp_path / "r.bam"), str(tmp_path / "r.fq")
    reads_io.write_sam(sam, batch)
    reads_io.write_bam(bam, batch)
    reads_io.write_fastq(fq, batch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for path, word in ((sam, "SAM"), (bam, "BAM")):
        with pytest.raises(ValueError, match="read-hits does not read %s files.*out of scope" % word):
            run_argument_parser(["read-hits", "-i", str(tmp_path / "none.npz"), "-f", path, "-k", "5", "-o", str(tmp_path / "o")])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
        run_argument_parser(["read-hits", "-i", str(tmp_path / "none.npz"), "-f", fq, "-k", "5", "-o", str(tmp_path / "o")])
    assert not os.path.exists(str(tmp_path / "o.npy"))


def test_map_keeps_its_arguments():
    """`kmer_mapper map` is untouched by the new subcommand: same options, same defaults."""
    from kmer_mapper_amd.command_line_interface import build_argument_parser, map_bnp, read_hits_file
    p = build_argument_parser()
    a = p.parse_args(["map", "-i", "x.npz", "-f", "r.fq", "-o", "o"])
    assert a.func is map_bnp and a.max_hits_per_kmer == 1000 and a.kmer_size == 31 and not hasattr(a, "min_hits")
    b = p.parse_args(["read-hits", "-i", "x.npz", "-f", "r.fq", "-o", "o", "--windows", "--min-hits", "3", "-I", "7", "-r", "True"])
    assert b.func is read_hits_file and b.windows and b.min_hits == 3 and b.max_hits_per_kmer == 7 and b.map_reverse_complements
