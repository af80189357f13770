"""CPU tier of the sequence index builder (kmm_seq_index_build): the catalogue of tests/seq_index_cases.py is held
to its claims; its model to the C oracle where the oracle speaks (extraction on break-free cases, the index of D, reverse
complements) and to the arrays written out by hand; reads_io.parse_fasta_named to a line-by-line reader; the plain-C++
arithmetic of csrc/kmm_seqindex_plan.hpp, compiled by itself with g++ (tests/seq_index_cpu_driver.hpp), to trial division and
to its limits, as a library and as an ASan + UBSan executable; the command line's refusals that need no device.  The GPU tier
is tests/test_gpu_seq_index.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import ambiguous_cases as ac
from tests import seq_index_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
FIELDS = ("hashes_to_index", "n_kmers", "kmers", "nodes", "frequencies")


# --------------------------------------------------------------------------------------------------- the catalogue
@pytest.mark.parametrize("name", sc.CASES)
def test_every_case_reaches_the_seam_it_names(name):
    case, m = sc.build(name), sc.model(name)
    assert case.seam
    case.check(case, m)
    assert m.n_pairs == m.n_windows * (2 if case.both else 1) and m.n_entries <= m.n_pairs
    assert m.index.n_kmers.shape[0] == m.modulo and int(m.index.n_kmers.sum()) == m.n_entries


def test_the_catalogue_covers_the_paths_of_the_driver():
    cases = [sc.build(n) for n in sc.CASES]
    assert any(c.both for c in cases) and any(c.nodes is not None for c in cases) and any(c.lut is not None for c in cases)
    assert any(c.flags & sc.DEBUG_SHORT_ROUNDS for c in cases) and any(c.modulo for c in cases)
    assert any(c.offsets.shape[0] == 1 for c in cases)


def test_the_hand_case_equals_its_written_out_arrays():
    m = sc.model("hand")
    assert (m.modulo, m.n_windows, m.n_pairs, m.n_entries) == (sc.HAND.modulo, sc.HAND.n_windows, sc.HAND.n_pairs, sc.HAND.n_entries)
    for f in FIELDS:
        got, want = getattr(m.index, f), getattr(sc.HAND, f)
        assert got.dtype == want.dtype and np.array_equal(got, want), f
    assert m.d_kmers.tolist() == [36, 57, 14, 36, 0] and m.d_nodes.tolist() == [0, 0, 0, 1, 2]     # D, in order of first occurrence


# ------------------------------------------------------------------------------------------ the model and the oracle
@pytest.mark.parametrize("name", [n for n in sc.BREAK_FREE if n not in ("round_seam", "super_tile")])
def test_the_models_windows_are_the_oracles_kmers_on_break_free_cases(oracle, name):
    case = sc.build(name)
    _, kmers, _ = sc.pairs_of(case)
    want = oracle.extract(case.bases, case.offsets, case.k) if case.offsets.shape[0] > 1 else np.zeros(0, dtype=np.uint64)
    assert np.array_equal(kmers[::2] if case.both else kmers, want)


@pytest.mark.parametrize("name", ["hand", "shared", "palindromes", "contention_k5", "modulo_13", "n_runs", "all_shorter_than_k"])
def test_the_models_index_is_the_oracles_index_of_d(oracle, name):
    m = sc.model(name)
    want = oracle.build_index(m.d_kmers, m.d_nodes.astype(np.int64), m.modulo)
    for f, w in zip(FIELDS, (want._hashes_to_index, want._n_kmers, want._kmers, want._nodes, want._frequencies)):
        assert np.array_equal(getattr(m.index, f), w), (name, f)


def test_the_models_reverse_complements_are_the_oracles(oracle):
    for name in ("palindromes", "ac_repeat-both"):
        case = sc.build(name)
        _, kmers, nodes = sc.pairs_of(case)
        assert np.array_equal(kmers[1::2][:500], oracle.revcomp(kmers[0::2][:500], case.k))
        assert np.array_equal(nodes[0::2], nodes[1::2])


def test_first_occurrence_order_on_a_list_with_known_answer():
    km = np.array([9, 3, 9, 3, 7, 9, 3], dtype=np.uint64)
    nd = np.array([1, 1, 1, 2, 0, 1, 1], dtype=np.int32)
    assert sc.distinct_first(km, nd).tolist() == [0, 1, 3, 4]


# ---------------------------------------------------------------------------------------------------- parse_fasta_named
FASTA_TEXTS = {
    "wrapped": b">chr1 the first\nACGTAC\nGTAC\nGT\n>chr2\nTTTT\nAA\n",
    "crlf": b">a desc\r\nACGT\r\nAC\r\n>b\r\nGG\r\n",
    "lower_case": b">low\nacgtn\nNNac\n>UP\tx\nACGT\n",
    "no_final_newline": b">x 1\nACGT\nAC\n>y\nGGA",
    "empty_sequences": b">e1\n>e2 nothing\n\n>full\nACG\n>e3\n",
    "blank_name": b"> spaced\nAC\n>\nGT\n",
}


@pytest.mark.parametrize("which", sorted(FASTA_TEXTS))
def test_parse_fasta_named_against_a_line_by_line_reader(which):
    from kmer_mapper_amd import reads_io
    text = FASTA_TEXTS[which]
    names, seqs = sc.read_fasta_by_lines(text)
    batch, got_names = reads_io.parse_fasta_named(np.frombuffer(text, dtype=np.uint8))
    assert got_names == names
    assert bytes(batch.bases) == b"".join(seqs)
    assert np.asarray(batch.offsets).tolist() == np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).tolist()
    plain = reads_io.parse_fasta_block(np.frombuffer(text, dtype=np.uint8))            # parse_fasta_block is left alone
    assert bytes(plain.bases) == bytes(batch.bases) and np.array_equal(plain.offsets, batch.offsets)


def test_parse_fasta_named_on_nothing():
    from kmer_mapper_amd import reads_io
    batch, names = reads_io.parse_fasta_named(np.zeros(0, dtype=np.uint8))
    assert names == [] and np.asarray(batch.offsets).tolist() == [0]


# ------------------------------------------------------------------------------------------- csrc/kmm_seqindex_plan.hpp
@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("seq_index")
    src = tmp / "shim.cpp"
    src.write_text('#include "seq_index_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), str(src),
                           "-o", so])
    lib = ctypes.CDLL(so)
    i64, u64, i32, P = ctypes.c_int64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p
    for name, res, args in (("si_cpu_max_pairs", i64, []), ("si_cpu_pairs", i64, [i64, ctypes.c_int]), ("si_cpu_table_slots", i64, [i64]),
                            ("si_cpu_modulo", u64, [i64]), ("si_cpu_is_prime", ctypes.c_int, [u64]),
                            ("si_cpu_round_tiles", i64, [ctypes.c_int]), ("si_cpu_mix", u64, [u64, i32]),
                            ("si_cpu_dedup", i64, [P, P, i64, P, i64, P])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def test_the_table_has_at_least_two_slots_per_pair_and_a_power_of_two_of_them(plan):
    for n in list(range(0, 70)) + [511, 512, 513, 65535, 65536, 65537, (1 << 30) - 1, 1 << 30]:
        s = plan.si_cpu_table_slots(n)
        assert s >= 2 * n and s & (s - 1) == 0 and s <= 1 << 31, (n, s)
        assert s == 1024 or s // 2 < 2 * n, (n, s)                 # the smallest such power of two


def test_the_pair_limit_arithmetic_at_its_edge_without_overflow(plan):
    lim = plan.si_cpu_max_pairs()
    assert lim >= 1 << 30
    assert [plan.si_cpu_pairs(lim + d, 0) for d in (-1, 0, 1)] == [lim - 1, lim, -1]
    assert [plan.si_cpu_pairs(lim // 2 + d, 1) for d in (-1, 0, 1)] == [lim - 2, lim, -1]
    assert plan.si_cpu_pairs(2 ** 63 - 1, 1) == -1 and plan.si_cpu_pairs(2 ** 63 - 1, 0) == -1 and plan.si_cpu_pairs(-5, 0) == -1
    assert plan.si_cpu_pairs(0, 1) == 0
    assert plan.si_cpu_round_tiles(1) * sc.TILE == sc.ROUND_DEBUG and plan.si_cpu_round_tiles(0) == 1 << 20


def test_the_modulo_is_the_smallest_prime_by_trial_division(plan):
    for n in range(0, 2001):
        assert plan.si_cpu_modulo(n) == sc.model_modulo(n), n
    assert plan.si_cpu_modulo(-3) == 3
    assert plan.si_cpu_modulo(1 << 30) == sc.smallest_prime_at_least((1 << 31) + 1)
    assert plan.si_cpu_is_prime((1 << 31) - 1) == 1 and plan.si_cpu_is_prime((1 << 31) + 1) == 0


@pytest.mark.parametrize("name", ["poly_a-both", "palindromes", "contention_k5", "shared-one_node"])
def test_the_pair_index_set_keeps_the_first_of_every_pair(plan, name):
    """The probe rule of the kernels, run one pair after the other: the kept pairs are the model's D."""
    case = sc.build(name)
    _, kmers, nodes = sc.pairs_of(case)
    n = kmers.shape[0]
    slots = plan.si_cpu_table_slots(n)
    table = np.zeros(slots, dtype=np.uint32)
    keep = np.full(n, 2, dtype=np.uint8)
    used = plan.si_cpu_dedup(kmers.ctypes.data, nodes.ctypes.data, n, table.ctypes.data, slots, keep.ctypes.data)
    m = sc.model(name)
    assert used == m.n_entries
    assert np.array_equal(np.flatnonzero(keep), sc.distinct_first(kmers, nodes))
    assert np.array_equal(kmers[keep == 1], m.d_kmers) and np.array_equal(nodes[keep == 1], m.d_nodes)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver built as an executable with ASan + UBSan (host code; nothing is loaded into Python)."""
    exe = str(tmp_path / "seq_index_san")
    src = os.path.join(ROOT, "tests", "seq_index_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
    assert run.stdout.split()[0] == "ok" and int(run.stdout.split()[1]) == 2002


# ------------------------------------------------------------------------------------------------------ the command line
def test_the_command_line_refuses_before_a_device_is_opened(tmp_path, monkeypatch):
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd import engine

    def no_device(*a, **kw):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(engine, "index_from_sequences", no_device)
    fq = tmp_path / "reads.fq"
    fq.write_bytes(b"@r1\nACGTACGT\n+\nIIIIIIII\n")
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">s\nACGTACGTACGT\n")
    out = str(tmp_path / "o.npz")
    with pytest.raises(ValueError, match="FASTQ.*FASTA"):
        cli.run_argument_parser(["index", "-f", str(fq), "-k", "5", "-o", out])
    with pytest.raises(SystemExit):                                                   # -o is required
        cli.run_argument_parser(["index", "-f", str(fa), "-k", "5"])
    with pytest.raises(ValueError, match="--modulo 1 "):
        cli.run_argument_parser(["index", "-f", str(fa), "-k", "5", "-o", out, "--modulo", "1"])
    with pytest.raises(ValueError, match="-k 32"):
        cli.run_argument_parser(["index", "-f", str(fa), "-k", "32", "-o", out])
    with pytest.raises(ValueError, match="skip needs -k 2"):
        cli.run_argument_parser(["index", "-f", str(fa), "-k", "1", "-o", out])
    assert not os.path.exists(out)


def test_the_index_command_defaults_to_skip_and_says_that_map_does_not():
    from kmer_mapper_amd import command_line_interface as cli
    parser = cli.build_argument_parser()
    args = parser.parse_args(["index", "-f", "x.fa", "-o", "y.npz"])
    assert args.ambiguous_bases == "skip" and args.kmer_size == 31 and args.modulo == 0 and not args.both_strands
    assert parser.parse_args(["map", "-f", "x.fa", "-i", "y.npz", "-o", "z"]).ambiguous_bases == "a"
    sub = [a for a in parser._subparsers._group_actions[0].choices["index"]._actions if a.dest == "ambiguous_bases"][0]
    assert "map" in sub.help and "other way" in sub.help
