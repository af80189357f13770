"""CPU tier of SAM lines kept as SAM lines (include/kmm.h "record_sam"): the source the kernels share —
csrc/kmm_sam.hpp's span sink on the write walk, the keep predicate, the destinations and a lane's share of a copy — compiled by
itself with g++ (tests/sam_records_cpu_driver.hpp) and run with 1 and 64 lanes into queues of exactly the model's size, filled
with 0x00 and with 0xFF, against the independent model of tests/sam_records_cases.py; every residue of source and destination
modulo 16 with every byte written exactly once; the same driver as an executable under ASan + UBSan; the conditions that keep the
catalogue from being vacuous; the command line's refusals up to the first look at the index."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import sam_records_cases as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
U64, I64, U32 = ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32
CASES = sr.all_cases()
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sam_records")
    src = tmp / "shim.cpp"
    src.write_text('#include "sam_records_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.sam_raw_cpu.argtypes = [ctypes.c_char_p, U64, ctypes.c_void_p, ctypes.c_int, U32, ctypes.c_int, ctypes.c_int, U32, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, U32, ctypes.c_void_p, ctypes.c_void_p, U64,
                                ctypes.c_void_p, ctypes.c_int, U64, ctypes.c_void_p, U64, ctypes.c_void_p, U64, ctypes.c_void_p]
    lib.sam_raw_copy_sweep.argtypes, lib.sam_raw_copy_sweep.restype = [U32, U32], U64
    return lib


def tables(sel):
    """The selection as the SAM front end takes it: (rules[4], intervals by name index, names, offsets)"""
    incl, min_mapq, regions, keep_unplaced = sel
    names = sorted({bytes(n) for n, _, _ in regions or []})
    iv = [(names.index(bytes(n)), beg, end) for n, beg, end in regions or []]
    offs = [0]
    for nm in names:
        offs.append(offs[-1] + len(nm))
    return [incl, min_mapq, int(keep_unplaced), len(iv)], iv, names, offs


def _run(lib, case, text, want, cuts=(), lanes=1, fill=0, tail0=0):
    """(rc, kept bytes, stats, FASTA text) of the driver; the queue holds exactly tail0 + len(want.out) bytes."""
    cuts = sorted(set([c for c in cuts if 0 < c < len(text)] + [len(text)]))
    rules, iv, names, offs = tables(case.sel)
    c = (U64 * len(cuts))(*cuts)
    r = (U64 * 4)(*rules)
    ivs = (I64 * (3 * len(iv) + 1))(*[x for t in iv for x in t])
    off = (U32 * len(offs))(*offs)
    hits, windows = np.ascontiguousarray(want.hits), np.ascontiguousarray(want.windows)
    rule3 = (U32 * 3)(case.min_hits, case.min_permille, int(case.invert))
    out = np.zeros(len(want.out) + 1, np.uint8)
    fasta = np.zeros(len(text) + 16, np.uint8)
    st = (U64 * 9)()
    rc = lib.sam_raw_cpu(text, len(text), c, len(cuts), case.excl, case.mode, int(case.orig), lanes, r, ivs, b"".join(names), off, len(names),
                         hits.ctypes.data, windows.ctypes.data, hits.shape[0], rule3, fill, tail0, out.ctypes.data, len(want.out),
                         fasta.ctypes.data, fasta.shape[0], st)
    return rc, out[:len(want.out)].tobytes(), list(st), fasta[:st[5]].tobytes()


# ---------------------------------------------------------------------------------------------- the catalogue itself
def test_the_identity_of_the_model():
    """min_hits 0, no exclusion, header lines on: what comes out is what went in, up to the last newline."""
    for name in ("mixed_all_kept", "dense_k1_all", "header_only"):
        c = sr.by_name(name)
        assert sr.expected(c).out == c.text
    c = sr.by_name("unterminated_last_line")
    whole = sr.model(c._replace(min_hits=0), sr.with_final_newline(c.text))
    assert whole.out == c.text + b"\n" and whole.n_kept == whole.n_records == sr.expected(c).n_records + 1


def test_no_case_is_vacuous():
    e = {c.name: sr.expected(c) for c in CASES}
    mixed = e["mixed"]
    assert mixed.keep.any() and not mixed.keep.all()
    flips = np.count_nonzero(mixed.keep[1:] != mixed.keep[:-1])
    assert flips >= len(mixed.keep) // 3                                           # kept and dropped records alternate
    assert e["mixed_none_kept"].n_kept == 0 and e["mixed_none_kept"].out.count(b"\n") == mixed.n_headers
    assert e["mixed_all_kept"].n_kept == mixed.n_records and (mixed.windows == 0).any()
    assert not (e["mixed_inverted"].keep == mixed.keep).any()
    assert 0 < e["mixed_permille"].n_kept < mixed.n_kept
    assert len(e["mixed_no_header"].out) < len(mixed.out) and mixed.out.startswith(b"@HD") and not e["mixed_no_header"].out.startswith(b"@")
    ex = e["mixed_excluded_between"]
    assert ex.n_excluded > 5 and 0 < ex.n_kept < ex.n_records
    for name in ("mixed_selection", "mixed_selection_no_header"):
        assert 5 < e[name].n_records < mixed.n_records - 5 and 0 < e[name].n_kept < e[name].n_records
    # a reverse-strand record that hits in read orientation alone, with also_revcomp off
    assert e["read_orientation"].hits[1] > 0 and e["as_stored"].hits[1] == 0 and e["as_stored_both_orientations"].hits[1] > 0
    assert e["read_orientation"].out != e["as_stored"].out
    crlf = sr.by_name("crlf").text
    assert crlf.count(b"\r\n") == crlf.count(b"\n")
    seqs = [ln.split(b"\t")[9] for ln in crlf.split(b"\r\n") if ln and not ln.startswith(b"@")]
    assert any(s.islower() and len(s) > 31 for s in seqs) and any(s.isupper() for s in seqs)   # lower-case SEQ goes through untouched
    dense = sr.by_name("dense_k1")
    per_tile = np.bincount(np.array([s for s, _ in sr.lines_of(dense.text)]) // sr.TILE)
    assert per_tile.max() >= 40
    assert e["no_complete_line"].consumed == 0 and e["no_complete_line"].out == b""
    assert e["header_only"].n_records == 0 and e["header_only_no_header"].out == b""


# ---------------------------------------------------------------------------------------------- the shared source on the CPU
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cases_with_1_and_64_lanes_into_queues_of_exactly_the_models_size(lib, case):
    want = sr.expected(case)
    for lanes in (1, 64):
        for fill in (0x00, 0xFF):
            rc, out, st, fasta = _run(lib, case, case.text[:want.consumed], want, lanes=lanes, fill=fill)
            assert rc == 0 and out == want.out, (lanes, fill, rc)
            assert st[:5] == [want.n_records, want.n_excluded, want.n_headers, len(want.out), want.n_kept], st
            assert fasta == want.fasta and st[7] == want.n_records


@pytest.mark.parametrize("name", ["mixed", "mixed_selection", "long_lines", "tile_edges", "crlf", "unterminated_last_line", "dense_k1"])
def test_streams_in_windows_cut_inside_lines_and_tails_at_every_residue(lib, name):
    """The carry: windows that end inside lines give the one-shot result; the queue's tail moves from window to window, so every
    window's first span lands on another residue; a final line without its newline gets one."""
    case = sr.by_name(name)
    want = sr.model(case, sr.with_final_newline(case.text))
    for cuts in ((), tuple(range(777, len(case.text), 777)), (1, 2, 3, 1000, 1023, 1024, 1025, 2047, 2048)):
        for tail0 in (0, 1, 15, 16, 33):
            rc, out, st, fasta = _run(lib, case, case.text, want, cuts, lanes=64, fill=0xFF, tail0=tail0)
            assert rc == 0 and out == want.out and fasta == want.fasta, (cuts[:3], tail0, rc)
            assert st[4] == want.n_kept and st[7] == want.n_records


@pytest.mark.parametrize("case", sr.block_cases(), ids=[c.name for c in sr.block_cases()])
def test_more_than_one_block_of_spans_and_of_tiles(lib, case):
    """The catalogue's block cases (more than 1024 spans; more than 1024 tiles with records and header lines on both sides of tile
    1024) through the CPU driver, whose loops restate the two levels of both prefixes — raw_tile_pre and raw_span_dest add them as
    the kernels do.  The kernels' own second level runs in tests/test_gpu_sam_records.py, on the same cases."""
    want = sr.expected(case)
    rc, out, st, fasta = _run(lib, case, case.text, want, lanes=64, fill=0xFF, tail0=7)
    assert rc == 0 and out == want.out and fasta == want.fasta
    assert st[:5] == [want.n_records, want.n_excluded, want.n_headers, len(want.out), want.n_kept]


def test_a_queue_one_byte_short_is_noticed_before_anything_is_copied(lib):
    case = sr.by_name("mixed")
    want = sr.expected(case)
    short = want._replace(out=want.out[:-1])
    assert _run(lib, case, case.text, short)[0] == -5


def test_every_residue_of_source_and_destination_every_byte_written_once(lib):
    """16 x 16 residues of the source start and the destination start modulo 16, lengths 1 to 80 — where rk_span's head, middle
    and tail meet — with 1 and 64 lanes: the bytes arrive, nothing in front is touched, every byte is written exactly once."""
    for lanes in (1, 64):
        assert lib.sam_raw_copy_sweep(lanes, 80) == 0


# ---------------------------------------------------------------------------------------------- under the sanitizers
SAN_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


@pytest.fixture(scope="module")
def sanitizers(tmp_path_factory):
    """Asked up front, with a program of one line: does this machine's g++ link the sanitizers' runtimes?  The driver's own build
    below is then held to succeed."""
    tmp = tmp_path_factory.mktemp("san_probe")
    src = tmp / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    probe = subprocess.run(["g++", *SAN_FLAGS, str(src), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("g++ does not link the sanitizers' runtimes here: " + probe.stderr[-200:])


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path, sanitizers):
    """The same driver as an executable with ASan + UBSan (tests/sam_records_san_main.cpp; host code, nothing sanitized is loaded
    into Python): the input, the entries, the tables, the text and the queue live in heap buffers of exactly their size."""
    exe = str(tmp_path / "sam_records_san")
    src = os.path.join(ROOT, "tests", "sam_records_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", *SAN_FLAGS, "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    for lanes in (1, 64):
        run = subprocess.run([exe, "sweep", str(lanes), "80"], capture_output=True, text=True)
        assert run.returncode == 0 and run.stdout.split() == ["0"], run.stderr[-2000:]
    inp, outp, jobp = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "job.bin"
    runs = [("mixed", 1, 0x00, 0, []), ("mixed_selection_no_header", 64, 0xFF, 5, [str(c) for c in range(500, 11_000, 1_313)]),
            ("long_lines", 64, 0x00, 15, ["1024", "4000"]), ("tile_edges", 1, 0xFF, 16, []), ("dense_k1_inverted_no_header", 64, 0xFF, 1, ["23"]),
            ("crlf", 64, 0x00, 3, []), ("read_orientation", 64, 0xFF, 0, []), ("unterminated_last_line", 1, 0x00, 9, ["2999"]),
            ("header_only", 64, 0xFF, 2, []), ("no_complete_line", 1, 0x00, 0, []),
            ("blocks_dense_k1", 64, 0xFF, 11, ["30000"]), ("blocks_big_excluded_no_header", 64, 0x00, 5, ["1048570"])]
    for name, lanes, fill, tail0, cuts in runs:
        case = sr.by_name(name)
        want = sr.model(case, sr.with_final_newline(case.text))
        rules, iv, names, offs = tables(case.sel)
        inp.write_bytes(case.text)
        jobp.write_bytes(struct.pack("<8I", case.excl, case.mode, int(case.orig), lanes, case.min_hits, case.min_permille, int(case.invert), fill) +
                         struct.pack("<4Q", tail0, len(want.out), want.hits.shape[0], 1) + want.hits.astype("<u4").tobytes() +
                         want.windows.astype("<u4").tobytes() + struct.pack("<4Q", *rules) + b"".join(struct.pack("<3q", *t) for t in iv) +
                         struct.pack("<I", len(names)) + struct.pack("<%dI" % len(offs), *offs) + b"".join(names))
        run = subprocess.run([exe, "run", str(inp), str(outp), str(jobp)] + cuts, capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stderr[-3000:])
        got = [int(v) for v in run.stdout.split()]
        assert got[:6] == [0, want.n_records, want.n_excluded, want.n_headers, len(want.out), want.n_kept], (name, got)
        assert got[6] == len(want.fasta) and got[8] == want.n_records
        assert outp.read_bytes() == want.out, name


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    from tests import record_hits_cases as rh
    bases, offsets = rh.reads_arrays([sr.hit_read(60, 0), sr.miss_read(60)])
    batch = ReadBatch(bases, offsets)
    paths = {ext: str(tmp_path / ("r." + ext)) for ext in ("bam", "sam", "fq")}
    paths["sam.gz"] = str(tmp_path / "r.sam.gz")
    reads_io.write_bam(paths["bam"], batch)
    reads_io.write_sam(paths["sam"], batch)
    reads_io.write_sam(paths["sam.gz"], batch, bgzf=True)
    reads_io.write_fastq(paths["fq"], batch)
    return paths


def test_the_command_line_refuses_before_the_index_is_read(tmp_path, monkeypatch):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.sam")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out]      # (the index does not exist)
    for ext in ("fq", "bam"):
        with pytest.raises(ValueError, match="--sam-out applies to SAM input only"):
            run_argument_parser(common + ["-f", paths[ext], "--sam-out"])
    for option in (["--bam-to-fastq"], ["--bam-out"], ["--as-stored"], ["--mate-suffix"], ["--bam-pairs"], ["--keep-mates"], ["--interleaved"],
                   ["-f2", paths["fq"]], ["-o2", str(tmp_path / "kept2.sam")], ["-f2", paths["sam"], "-o2", str(tmp_path / "kept2.sam")]):
        for ext in ("sam", "sam.gz"):
            with pytest.raises(ValueError, match="--sam-out does not go with %s" % option[0]):
                run_argument_parser(common + ["-f", paths[ext], "--sam-out"] + option)
    for ext in ("sam", "fq", "bam"):
        with pytest.raises(ValueError, match="--no-header goes with --sam-out"):
            run_argument_parser(common + ["-f", paths[ext], "--no-header"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
        run_argument_parser(common + ["-f", paths["sam"], "--sam-out"])
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="is the input file"):
        run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-f", paths["sam"], "-o", paths["sam"], "--sam-out"])
    # without the switch SAM stays refused in its words, now with a hint; the selection options stay BAM's
    with pytest.raises(ValueError, match="select-reads does not read SAM files.*name.*--sam-out"):
        run_argument_parser(common + ["-f", paths["sam"]])
    with pytest.raises(ValueError, match="select-reads does not read SAM files.*name"):
        run_argument_parser(common + ["-f", paths["sam"], "--min-mapq", "3"])
    with pytest.raises(ValueError, match="--min-mapq applies to BAM input only"):
        run_argument_parser(common + ["-f", paths["fq"], "--min-mapq", "3"])
    # values the library would refuse are refused here, with the switch too
    with pytest.raises(ValueError, match="--min-mapq outside"):
        run_argument_parser(common + ["-f", paths["sam"], "--sam-out", "--min-mapq", "300"])
    assert not os.path.exists(out)


def test_with_the_switch_a_sam_file_passes_the_checks_up_to_the_index(tmp_path, monkeypatch):
    """--sam-out with every option that goes with it: the first thing that fails is the index file that does not exist."""
    from kmer_mapper_amd import command_line_interface as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.sam")
    args = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out, "--sam-out", "--no-header", "--bgzf", "--min-hits", "2",
            "--min-hit-permille", "10", "--invert", "--hits-output", str(tmp_path / "h"), "--exclude-flags", "0x900", "--include-flags", "1",
            "--min-mapq", "20", "--regions", "chr1:1-500"]
    for ext in ("sam", "sam.gz"):
        with pytest.raises(Exception) as info:
            cli.run_argument_parser(args + ["-f", paths[ext]])
        assert "none.npz" in str(info.value) or isinstance(info.value, (FileNotFoundError, OSError)), info.value
    assert not os.path.exists(out)
    plain = cli.build_argument_parser().parse_args(["select-reads", "-i", "i.npz", "-f", paths["sam"], "-o", out])
    assert not {"sam_out", "no_header"} & set(vars(plain))                         # (a call without them parses as it did before)
    cli.check_select_reads_input("sam", 1, paths["sam"], out, sam_out=True)
