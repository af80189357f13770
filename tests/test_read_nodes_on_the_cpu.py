"""CPU tier of kmm_read_nodes (include/kmm.h).  The catalogue's model (tests/read_nodes_cases.py) against the
oracle's map_reads called read by read — a break-free segment of a read is a read — the conditions that keep the catalogue from
being vacuous, the arithmetic of csrc/kmm_read_nodes_plan.hpp compiled with g++ against brute force (once more under ASan +
UBSan as a stand-alone executable), the command line's refusals and its assignment rule."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from kmer_mapper_amd.util import LUT_BREAK, default_lut
from tests import read_nodes_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = nc.all_cases()
IDS = [c.name for c in CASES]
I64, U32, U64 = ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
_P = ctypes.c_void_p


# ---------------------------------------------------------------------------------------------- the model against the oracle
def _segments(case, r):
    """The break-free segments of read r as (bases, offsets) of a batch of their own"""
    read = case.bases[case.offsets[r]:case.offsets[r + 1]]
    lut = default_lut() if case.lut is None else case.lut
    parts = np.split(read, np.nonzero(lut[read] == LUT_BREAK)[0])
    parts = [p if i == 0 else p[1:] for i, p in enumerate(parts)]
    return nc.rc.batch(parts)


def _reads_to_check(case):
    n = case.offsets.shape[0] - 1
    if n <= 200:
        return range(n)
    lens = np.diff(case.offsets)
    picked = set(np.nonzero(lens > 0)[0][:60].tolist()) | set(range(0, n, max(n // 60, 1)))
    return sorted(picked)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_model_agrees_with_the_oracle_read_by_read(case, oracle):
    """total_votes and the whole vote vector: what map_reads adds to the node counts when it is given the read alone."""
    mx = case.index.max_node_id()
    tallies = nc.tallies(case)
    want = nc.expected(case)
    some = False
    for r in _reads_to_check(case):
        bases, offsets = _segments(case, r)
        counts, _ = oracle.map_reads(case.index, mx, bases, offsets, case.k, case.max_freq, case.revcomp)
        votes, windows = tallies[r]
        vector = np.zeros(mx + 1, dtype=np.uint32)
        for node, v in votes.items():
            vector[node] = v
        assert np.array_equal(counts, vector), r
        assert int(counts.sum()) == int(want.total_votes[r]) and int((counts > 0).sum()) == int(want.n_nodes[r])
        if counts.any():
            top = int(counts.max())
            assert int(want.best_votes[r]) == top and int(want.best_node[r]) == int(np.nonzero(counts == top)[0][0])
            rest = np.delete(counts, want.best_node[r])
            assert int(want.second_votes[r]) == (int(rest.max()) if rest.shape[0] else 0)
            some = True
        else:
            assert want.best_node[r] == -1 and want.best_votes[r] == 0 and want.second_votes[r] == 0
    assert some


# ---------------------------------------------------------------------------------------------- non-vacuity
def test_the_catalogue_is_not_vacuous():
    exp = {c.name: nc.expected(c) for c in CASES}
    ties = [n for n, e in exp.items() if ((e.best_votes == e.second_votes) & (e.best_votes > 0)).any()]
    assert "ties_k31" in ties and "three_nodes_k31" in ties
    assert any((e.second_votes > 0).any() for e in exp.values())
    # the smaller id is met second and wins the tie; ids above 16 bits occur
    tie = nc.case("ties_k31")
    assert nc.first_node_met(tie, 0) == nc.BIG > 0xFFFF and exp["ties_k31"].best_node[0] == nc.SMALL
    assert nc.tallies(tie)[0][0] == {nc.BIG: 3, nc.SMALL: 3}
    assert nc.tallies(tie)[2][0] == {nc.MID: 2, nc.BIG: 2, nc.SMALL: 2} and exp["ties_k31"].n_nodes[2] == 3
    # some read has no vote although it has windows
    assert any(e.best_node[r] == -1 and w > 0 for c in CASES for e in [exp[c.name]] for r, (_, w) in enumerate(nc.tallies(c)))
    # a read without hits between reads with hits
    e = exp["ties_k31"]
    assert e.best_node[0] >= 0 and e.best_node[1] == -1 and e.best_node[2] >= 0
    # one k-mer under three nodes; the filter between two entries of one k-mer
    assert nc.tallies(nc.case("three_nodes_k31"))[0][0] == {5: 1, 6: 1, 7: 1}
    filt = nc.case("filter_k31")
    assert nc.answer(nc.tally_read(filt.index, filt.bases[:80], 31)[0])[:3] == (20, 3, 2)         # without the filter
    assert tuple(int(a[0]) for a in exp["filter_k31"][:3]) == (30, 2, 0)                           # the filtered node loses
    # 120 windows on 120 nodes
    many = exp["many_nodes_k31"]
    assert many.n_nodes[0] == 120 and many.best_votes[0] == 1 and many.best_node[0] == 1000
    # one cell with many adders, many cells on one node, many nodes
    assert exp["long_read_one_node_k31"].best_votes[0] == 20_000 - 30 and exp["long_read_one_node_k31"].n_nodes[0] == 1
    assert (exp["one_node_3000x150_k31"].best_node == 12_345).all()
    mixed = exp["mixed_3000x150_k31"]
    assert np.unique(mixed.best_node[mixed.best_node >= 0]).shape[0] == 50 and (mixed.n_nodes == 2).any() and (mixed.best_node == -1).any()
    assert int(exp["oversize_read_k31"].total_votes[1]) > nc.MIN_TABLE_BYTES // 32
    assert int(mixed.total_votes.sum()) > 3 * (nc.MIN_TABLE_BYTES // 32)


def test_the_seam_case_is_won_behind_the_seam():
    """Node B wins the part of the read in front of the seam, node A wins the read: no per-tile or per-wavefront winner gives it."""
    case = nc.case("seam_winner_k31")
    want = nc.expected(case)
    for r, seam in nc.SEAM_READS.items():
        read = case.bases[case.offsets[r]:case.offsets[r + 1]]
        assert (int(case.offsets[r]) + seam) % nc.WAVE == 0
        front = nc.answer(nc.tally_read(case.index, read[:seam + case.k - 1], case.k)[0])           # the windows that start in front of it
        behind = nc.answer(nc.tally_read(case.index, read[seam:], case.k)[0])
        assert front[:3] == (nc.SMALL, 5, 3) and behind[:3] == (nc.BIG, 3, 0)
        assert (int(want.best_node[r]), int(want.best_votes[r]), int(want.second_votes[r])) == (nc.BIG, 6, 5)
        assert want.best_node[r] != front[0]
    assert (int(case.offsets[3]) + nc.SEAM_READS[3]) % nc.TILE == 0


def test_the_catalogue_holds_what_the_seams_need():
    by_name = {c.name: c for c in CASES}
    ends = set(by_name["seams_k31"].offsets.tolist())
    for seam in (nc.LANE, nc.WAVE, nc.TILE, 2 * nc.TILE):
        assert {seam - 1, seam, seam + 1} <= ends
    empty = np.diff(by_name["empty_reads_k31"].offsets) == 0
    assert empty[0] and empty[-1]
    run = np.diff(np.nonzero(np.diff(np.concatenate([[0], empty.astype(np.int8), [0]])))[0])[::2].max()
    assert run >= 2000 > nc.TILE
    assert (np.diff(by_name["short_reads_k31"].offsets)[:120] <= 33).all()
    brk = by_name["breaks_k31"]
    is_break = brk.lut[brk.bases] == LUT_BREAK
    assert is_break[0] and is_break[nc.TILE - 1] and is_break[nc.TILE] and is_break[int(brk.offsets[3]) - 1]
    pal = by_name["revcomp_k16"]
    only_rc = nc.tally_read(pal.index, pal.bases[pal.offsets[1]:pal.offsets[2]], 16)[0]
    assert only_rc == {} and nc.expected(pal).best_node[1] == 2                                   # votes in the other orientation only
    assert nc.expected(pal).best_votes[4] == 2 * 9                                                 # the palindrome votes twice per window
    assert {int(c.index._modulo) for c in CASES if c.name.startswith("modulo_")} == {257, 3}
    assert max(c.bases.shape[0] for c in CASES) <= 3000 * 150


# ---------------------------------------------------------------------------------------------- the arithmetic
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("read_nodes")
    src = tmp / "shim.cpp"
    src.write_text('#include "read_nodes_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    for name in ("read_nodes_round_votes", "read_nodes_table_slots"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [I64], I64
    for name in ("read_nodes_rounds_cpu", "read_nodes_rounds_brute"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [_P, I64, I64, _P], I64
    lib.read_nodes_table_cpu.argtypes, lib.read_nodes_table_cpu.restype = [_P, _P, I64, I64, _P, _P], I64
    lib.read_nodes_reduce_cpu.argtypes, lib.read_nodes_reduce_cpu.restype = [_P, _P, I64, I64, _P, _P, _P], None
    lib.read_nodes_best_node.argtypes, lib.read_nodes_best_node.restype = [U64], ctypes.c_int32
    lib.read_nodes_best_votes.argtypes, lib.read_nodes_best_votes.restype = [U64], U32
    lib.read_nodes_best_word.argtypes, lib.read_nodes_best_word.restype = [U32, U32], U64
    lib.read_nodes_key.argtypes, lib.read_nodes_key.restype = [U32, U32], U64
    return lib


def test_table_sizes(lib):
    assert lib.read_nodes_round_votes(0) == (4 << 30) // 32
    assert lib.read_nodes_round_votes(1) == lib.read_nodes_round_votes(nc.MIN_TABLE_BYTES) == nc.MIN_TABLE_BYTES // 32 == 2048
    assert lib.read_nodes_round_votes(1 << 20) == (1 << 20) // 32
    assert lib.read_nodes_round_votes(1 << 62) == 2 ** 31 - 1
    for votes in (0, 1, 31, 32, 33, 2048, 10 ** 6, 2 ** 31 - 1):
        slots = lib.read_nodes_table_slots(votes)
        assert slots >= 2 * votes and slots >= 64 and slots < 2 ** 32
        assert slots == max(2 * votes, 64)


def _vote_totals():
    rng = np.random.default_rng(3)
    yield "mixed", nc.expected(nc.case("mixed_3000x150_k31")).total_votes
    yield "oversize", nc.expected(nc.case("oversize_read_k31")).total_votes
    yield "empty", nc.expected(nc.case("empty_reads_k31")).total_votes
    yield "zeros", np.zeros(700, np.uint32)
    yield "one", np.array([5], np.uint32)
    yield "random", rng.integers(0, 3000, size=5000).astype(np.uint32)
    yield "all_oversize", np.full(40, 5000, np.uint32)


@pytest.mark.parametrize("name,totals", list(_vote_totals()), ids=[n for n, _ in _vote_totals()])
def test_rounds_agree_with_brute_force(lib, name, totals):
    n = totals.shape[0]
    for cap in (1, 100, 2048, 2049, 10 ** 9):
        got, want = np.zeros(n, np.int64), np.zeros(n, np.int64)
        n_got = lib.read_nodes_rounds_cpu(totals.ctypes.data, n, cap, got.ctypes.data)
        n_want = lib.read_nodes_rounds_brute(totals.ctypes.data, n, cap, want.ctypes.data)
        assert n_got == n_want and np.array_equal(got[:n_got], want[:n_want]), cap
        ends = got[:n_got]
        assert ends[-1] == n and (np.diff(np.concatenate([[0], ends])) >= 1).all()              # whole reads, at least one
        prefix = np.concatenate([[0], np.cumsum(totals.astype(np.int64))])
        per_round = np.diff(prefix[np.concatenate([[0], ends])])
        lone = np.diff(np.concatenate([[0], ends])) == 1
        assert (per_round[~lone] <= cap).all()                                                  # only a read alone may exceed the cap
    if name == "mixed":
        assert lib.read_nodes_rounds_cpu(totals.ctypes.data, n, 2048, got.ctypes.data) >= 3


def _votes_of(case, reads):
    """(rel_read, node) per vote of the given reads, in read order"""
    rel, node = [], []
    for i, r in enumerate(reads):
        for nd, v in nc.tallies(case)[r][0].items():
            rel += [i] * v
            node += [nd] * v
    return np.array(rel, np.uint32), np.array(node, np.uint32)


@pytest.mark.parametrize("name", ["ties_k31", "many_nodes_k31", "seam_winner_k31", "one_node_3000x150_k31", "mixed_3000x150_k31",
                                  "long_read_one_node_k31", "seams_k31"])
def test_table_and_reduction_agree_with_the_model(lib, name):
    """Votes in a shuffled order through the table's walk and the max / add reduction give the model's five outputs."""
    case = nc.case(name)
    n_reads = case.offsets.shape[0] - 1
    rel, node = _votes_of(case, range(n_reads))
    order = np.random.default_rng(1).permutation(rel.shape[0])
    rel, node = np.ascontiguousarray(rel[order]), np.ascontiguousarray(node[order])
    slots = lib.read_nodes_table_slots(rel.shape[0])
    keys, counts = np.zeros(slots, np.uint64), np.zeros(slots, np.uint32)
    longest = lib.read_nodes_table_cpu(rel.ctypes.data, node.ctypes.data, rel.shape[0], slots, keys.ctypes.data, counts.ctypes.data)
    assert 1 <= longest <= 64, "a walk that long says the home slots cluster"
    used = keys != np.uint64(2 ** 64 - 1)
    assert int(used.sum()) == int(nc.expected(case).n_nodes.sum()) and int(counts.sum()) == rel.shape[0]
    best, nn, second = np.zeros(n_reads, np.uint64), np.zeros(n_reads, np.uint32), np.zeros(n_reads, np.uint32)
    lib.read_nodes_reduce_cpu(keys.ctypes.data, counts.ctypes.data, slots, n_reads, best.ctypes.data, nn.ctypes.data, second.ctypes.data)
    want = nc.expected(case)
    assert [lib.read_nodes_best_node(int(w)) for w in best] == want.best_node.tolist()
    assert [lib.read_nodes_best_votes(int(w)) for w in best] == want.best_votes.tolist()
    assert np.array_equal(nn, want.n_nodes) and np.array_equal(second, want.second_votes)


def test_key_and_best_word(lib):
    rng = np.random.default_rng(2)
    for rel, node in zip(rng.integers(0, 2 ** 31, 200).tolist() + [0, 2 ** 31 - 1], rng.integers(0, 2 ** 31, 200).tolist() + [0, 2 ** 31 - 1]):
        key = lib.read_nodes_key(rel, node)
        assert key == (rel << 32) | node and key != 2 ** 64 - 1
    assert lib.read_nodes_best_node(0) == -1 and lib.read_nodes_best_votes(0) == 0
    words = [(v, n, lib.read_nodes_best_word(v, n)) for v in (1, 2, 3, 2 ** 31, 2 ** 32 - 1) for n in (0, 9, 70_001, 2 ** 31 - 1)]
    for v, n, w in words:
        assert (lib.read_nodes_best_node(w), lib.read_nodes_best_votes(w)) == (n, v) and w > 0
    # the order of the words is the rule: more votes first, then the smaller node
    ranked = sorted(words, key=lambda t: t[2], reverse=True)
    assert [(v, n) for v, n, _ in ranked] == sorted([(v, n) for v, n, _ in words], key=lambda t: (-t[0], t[1]))


def test_arithmetic_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/read_nodes_san_main.cpp; host code, nothing sanitized is loaded
    into Python): votes, tables and results live in heap buffers of exactly their size."""
    exe = str(tmp_path / "read_nodes_san")
    src = os.path.join(ROOT, "tests", "read_nodes_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    probe = tmp_path / "probe.cpp"                                                  # is there a sanitizer runtime to link against?
    probe.write_text("int main() { return 0; }\n")
    found = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if found.returncode != 0:
        pytest.skip("no sanitizer runtime on this box: " + found.stderr[-200:])
    build = subprocess.run(cmd, capture_output=True, text=True)                     # (a failure from here on is the code's)
    assert build.returncode == 0, build.stderr
    path = tmp_path / "votes.bin"
    for name in ("mixed_3000x150_k31", "oversize_read_k31", "many_nodes_k31", "empty_reads_k31"):
        case = nc.case(name)
        n_reads = case.offsets.shape[0] - 1
        rel, node = _votes_of(case, range(n_reads))
        np.stack([rel, node], axis=1).astype(np.uint32).tofile(str(path))
        for cap in (1, 2048, 10 ** 9):
            r = subprocess.run([exe, str(path), str(cap)], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (name, cap, r.stdout, r.stderr[-2000:])
            assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
            words = r.stdout.split()
            assert words[0] == "ok" and int(words[1]) == int(rel[-1]) + 1 and words[3] == "0" and 1 <= int(words[4]) <= 64


# ---------------------------------------------------------------------------------------------- the command line
def test_assign_reads_refusals(tmp_path, monkeypatch):
    """Refused with a message that says what to do, before the index file is read (there is none)."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    batch = ReadBatch.from_strings(["ACGTACGTAC", "GGGTTTAAAC"])
    sam, bam, fq = str(tmp_path / "r.sam"), str(tmp_path / "r.bam"), str(tmp_path / "r.fq")
    reads_io.write_sam(sam, batch)
    reads_io.write_bam(bam, batch)
    reads_io.write_fastq(fq, batch)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["assign-reads", "-i", str(tmp_path / "none.npz"), "-o", str(tmp_path / "o"), "-k", "5"]
    for path, word in ((sam, "SAM"), (bam, "BAM")):
        with pytest.raises(ValueError, match="assign-reads does not read %s files.*out of scope" % word):
            run_argument_parser(base + ["-f", path])
    with pytest.raises(ValueError, match="--ambiguous-bases skip needs -k 2"):
        run_argument_parser(base[:-1] + ["1", "-f", fq, "--ambiguous-bases", "skip"])
    with pytest.raises(ValueError, match="--min-votes -1 is negative"):
        run_argument_parser(base + ["-f", fq, "--min-votes", "-1"])
    with pytest.raises(ValueError, match="--min-margin -2 is negative"):
        run_argument_parser(base + ["-f", fq, "--min-margin", "-2"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
        run_argument_parser(base + ["-f", fq])
    assert not os.path.exists(str(tmp_path / "o.npy"))


def test_a_names_file_with_fewer_lines_than_nodes_is_refused(tmp_path, monkeypatch):
    """Needs the node count, so it comes behind the index file and before any device work (this test has no device)."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import read_node_names, run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    fq, npz, names = str(tmp_path / "r.fq"), str(tmp_path / "index.npz"), tmp_path / "names.txt"
    reads_io.write_fastq(fq, ReadBatch.from_strings(["ACGTACGTAC"]))
    nc.filter_index().to_file(npz)                                                  # nodes 20 and 30: 31 nodes
    names.write_text("".join("n%d\n" % i for i in range(30)))
    with pytest.raises(ValueError, match="has 30 lines and the index has 31 nodes.*--names-output"):
        run_argument_parser(["assign-reads", "-i", npz, "-f", fq, "-o", str(tmp_path / "o"), "--names", str(names)])
    names.write_text("".join("n%d\n" % i for i in range(31)))
    assert read_node_names(str(names), 31)[30] == "n30"


def test_the_assignment_rule_on_arrays(tmp_path):
    from kmer_mapper_amd.command_line_interface import assign_rule, write_assign_summary
    best_node = np.array([4, 4, 7, -1, 0, 70_001], np.int32)
    best = np.array([10, 3, 5, 0, 1, 4_000_000_000], np.uint32)
    second = np.array([2, 3, 4, 0, 0, 3_999_999_999], np.uint32)
    assert assign_rule(best_node, best, second).tolist() == [4, 4, 7, -1, 0, 70_001] and assign_rule(best_node, best, second).dtype == np.int32
    assert assign_rule(best_node, best, second, min_votes=4).tolist() == [4, -1, 7, -1, -1, 70_001]
    assert assign_rule(best_node, best, second, min_margin=1).tolist() == [4, -1, 7, -1, 0, 70_001]    # a tie is no margin
    assert assign_rule(best_node, best, second, min_margin=2).tolist() == [4, -1, -1, -1, -1, -1]
    assert assign_rule(best_node, best, second, min_votes=0).tolist() == [4, 4, 7, -1, 0, 70_001]       # no vote stays -1
    out = tmp_path / "s.tsv"
    write_assign_summary(str(out), np.array([1, 1, -1, 0], np.int32), 3, ["a", "b c", "d"])
    assert out.read_text().splitlines() == ["node\tname\treads\tshare", "0\ta\t1\t0.250000", "1\tb c\t2\t0.500000", "2\td\t0\t0.000000",
                                            "-1\tunassigned\t1\t0.250000"]


def test_the_other_subcommands_keep_their_arguments():
    from kmer_mapper_amd.command_line_interface import assign_reads_file, build_argument_parser, read_hits_file
    p = build_argument_parser()
    a = p.parse_args(["read-hits", "-i", "x.npz", "-f", "r.fq", "-o", "o"])
    assert a.func is read_hits_file and not hasattr(a, "min_votes")
    b = p.parse_args(["assign-reads", "-i", "x.npz", "-f", "r.fq", "-o", "o", "--min-votes", "3", "--min-margin", "2", "-I", "7",
                      "-r", "True", "--names", "n.txt", "--summary", "s.tsv", "-c", "1000", "--device", "1"])
    assert b.func is assign_reads_file and (b.min_votes, b.min_margin, b.max_hits_per_kmer, b.chunk_size, b.device) == (3, 2, 7, 1000, 1)
    assert b.map_reverse_complements and b.names == "n.txt" and b.summary == "s.tsv" and b.ambiguous_bases == "a" and b.kmer_size == 31
