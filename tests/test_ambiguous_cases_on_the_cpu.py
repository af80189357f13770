"""CPU tier of the break code (KMM_LUT_BREAK): the cases of tests/ambiguous_cases.py are held to the conditions they exist
for, so that tests/test_gpu_ambiguous.py cannot pass vacuously — the oracle on the reads split at their break bytes equals
a brute-force count of the windows without one, differs from what N read as A gives, and hits the index."""
import numpy as np
import pytest

from tests import ambiguous_cases as ac
from kmer_mapper_amd.util import LUT_BREAK, ambiguous_skip_lut


@pytest.fixture(scope="module")
def lut():
    return ambiguous_skip_lut()


@pytest.fixture(scope="module", params=ac.CASES)
def case(request, oracle, lut):
    name, bases, offsets, k = ac.build(request.param)
    index = ac.index_for(k)
    mx = index.max_node_id()
    sb, so = ac.split_at_breaks(bases, offsets, lut)
    split, n_windows = oracle.map_reads(index, mx, sb, so, k)
    return dict(name=name, bases=bases, offsets=offsets, k=k, index=index, mx=mx, sb=sb, so=so, split=split, n_windows=n_windows)


def test_split_reads_equal_the_brute_force_count_of_windows_without_a_break(case, oracle, lut):
    kmers = ac.surviving_kmers(case["bases"], case["offsets"], case["k"], lut)
    assert kmers.shape[0] == case["n_windows"]
    assert np.array_equal(oracle.map_kmers(case["index"], case["mx"], kmers), case["split"])
    assert not ac.break_mask(case["sb"], lut).any() and case["so"][0] == 0 and case["so"][-1] == case["sb"].shape[0]
    # no byte but the breaks is lost, and none is reordered
    assert np.array_equal(case["sb"], case["bases"][~ac.break_mask(case["bases"], lut)])


def test_every_case_tells_skipping_from_n_read_as_a_and_hits_the_index(case, oracle, lut):
    n_to_a, n_all = oracle.map_reads(case["index"], case["mx"], ac.n_to_a_bytes(case["bases"], lut), case["offsets"], case["k"])
    assert not np.array_equal(n_to_a, case["split"])
    as_g, _ = oracle.map_reads(case["index"], case["mx"], ac.code2_bytes(case["bases"], lut), case["offsets"], case["k"])
    assert not np.array_equal(as_g, case["split"])      # (0xFE read as code 2: a library without the break code)
    assert case["split"].sum() > 0
    assert 0 < case["n_windows"] < n_all
    if case["name"] == ac.RANDOM_CASE:       # 1 % breaks, k = 31: 1 - 0.99^31 = 26.8 % of the windows hold one
        assert 0.15 <= 1 - case["n_windows"] / n_all <= 0.40
    assert ac.is_uniform(case["offsets"]) == (case["name"] in ac.UNIFORM)


def test_the_breaks_stand_where_the_case_says(lut):
    """The positions the kernels can go wrong at hold a break byte."""
    _, bases, offsets, k = ac.build("tile_edges")
    total = bases.shape[0]
    brk = ac.break_mask(bases, lut)
    assert np.array_equal(np.flatnonzero(brk), sorted({0, 30, 31, 32, 1023, 1024, 4095, 4096, 8191, 8192, total - 1, total - k}))
    _, bases, offsets, k = ac.build("run_of_40")
    brk = ac.break_mask(bases, lut)
    assert brk[10 * ac.L + 50:10 * ac.L + 90].all() and brk[4080:4120].all() and brk[151 * ac.L - 40:151 * ac.L].all()
    _, bases, offsets, k = ac.build("all_n_and_short_reads")
    brk = ac.break_mask(bases, lut)
    lens = np.diff(offsets)
    assert brk[offsets[5]:offsets[6]].all() and lens[20] < k and brk[offsets[20]:offsets[21]].any()
    _, bases, offsets, k = ac.build("pairs_k_apart")
    at = np.flatnonzero(ac.break_mask(bases, lut))
    assert (np.diff(at) == k + 1).sum() == 3 and (np.diff(at) == k).sum() == 3
    win = ac.surviving_windows(bases, offsets, k, lut)
    assert 4 * ac.L + 41 in win and 4 * ac.L + 40 not in win and 4 * ac.L + 42 not in win      # exactly one between the pair
    assert not ((win > 9 * ac.L + 60 - k) & (win <= 9 * ac.L + 60 + k)).any()
    _, bases, offsets, k = ac.build("lower_case_and_iupac")
    seen = set(bases[ac.break_mask(bases, lut)].tobytes())
    assert seen == set(b"NRYKMSWBDHVnrykmswbdhv") and (bases & 0x20).any()


@pytest.mark.parametrize("name", ac.CASES)
@pytest.mark.parametrize("fmt", [4, 2])
def test_records_text_holds_the_same_reads_and_puts_breaks_on_tile_edges(name, fmt, lut):
    from kmer_mapper_amd import reads_io
    _, bases, offsets, k = ac.build(name)
    text, last, first = ac.records_text(bases, offsets, lut, fmt)
    batch = (reads_io.parse_fastq_block if fmt == 4 else reads_io.parse_fasta_block)(np.frombuffer(text, np.uint8))
    assert np.array_equal(batch.bases, bases) and np.array_equal(batch.offsets, offsets)
    assert last is not None and first is not None
    assert last % ac.TILE == ac.TILE - 1 and lut[text[last]] == LUT_BREAK
    assert first % ac.TILE == 0 and lut[text[first]] == LUT_BREAK
    # a "\r\n" line that holds a break; where a read ends with one, the break stands right before the "\r"
    lines = text.split(b"\n")[1::fmt]
    assert any(ln.endswith(b"\r") and ac.break_mask(np.frombuffer(ln[:-1], np.uint8), lut).any() for ln in lines)
    if name == "read_ends":
        assert b"N\r\n" in text and b"\r\nN" in text


def test_skip_table_differs_from_the_default_in_the_22_letters(oracle, lut):
    from kmer_mapper_amd.util import default_lut
    ref = oracle.default_lut()
    assert np.array_equal(default_lut(), ref)
    changed = np.flatnonzero(lut != ref)
    assert sorted(changed) == sorted(b"NRYKMSWBDHVnrykmswbdhv") and len(changed) == 22
    assert (lut[changed] == LUT_BREAK).all() and LUT_BREAK == 0xFE


def test_cli_option():
    from kmer_mapper_amd.command_line_interface import build_argument_parser
    base = ["map", "-i", "x.npz", "-f", "r.fq", "-o", "out"]
    parser = build_argument_parser()
    assert parser.parse_args(base).ambiguous_bases == "a"
    assert parser.parse_args(base + ["--ambiguous-bases", "skip"]).ambiguous_bases == "skip"
    assert parser.parse_args(base + ["--ambiguous-bases", "a"]).ambiguous_bases == "a"
    with pytest.raises(SystemExit):
        parser.parse_args(base + ["--ambiguous-bases", "c"])


def test_a_table_of_the_callers_never_takes_the_host_packers_route():
    from kmer_mapper_amd.command_line_interface import choose_route
    from kmer_mapper_amd.reads_io import InputProbe
    fields = InputProbe._fields
    plain = InputProbe(**{f: {"fmt": "fastq", "inflate": False, "container": None, "two_line": True}.get(f) for f in fields})
    assert choose_route("fastq", plain, 1, 16, True, env={})[0] == "mmap"
    assert choose_route("fastq", plain, 1, 16, True, env={}, lut=ambiguous_skip_lut())[0] == "raw"
