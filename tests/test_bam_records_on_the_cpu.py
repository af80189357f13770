"""CPU tier of the raw form of the BAM keep (include/kmm.h "record_bam"): csrc/kmm_bam.hpp compiled by itself with g++
and driven through run_call and CpuBackend's raw_count() + raw_copy() (tests/bam_records_cpu_driver.hpp) — the plain C++ the
kernels run — with 1 and 64 lanes, against the independent model of tests/bam_records_cases.py; once more as an executable under
AddressSanitizer + UndefinedBehaviorSanitizer (tests/bam_records_san_main.cpp: host code with its own main).  Also: the
conditions that keep the catalogue from being vacuous, and `select-reads --bam-out` up to the point where the index is read."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import bam_records_cases as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = br.all_cases() + [br.identity_case()]
IDS = [c.name for c in CASES]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_records")
    src = tmp / "shim.cpp"
    src.write_text('#include "bam_records_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), str(src),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.bam_records_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                    ctypes.c_void_p, ctypes.c_void_p]
    lib.bam_records_copy_writes.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    return lib


def _run(lib, case, lanes, cuts=(), fill=0, cap=None, tail0=0, windows=True, payload=None):
    base = case.base
    data = base.payload if payload is None else payload
    want, _, _, hits, wins = br.expected(case)
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    cap = tail0 + len(want) if cap is None else cap                               # (exactly the model's size: no slack to hide in)
    out = np.full(max(cap, 1), fill ^ 0x5A, np.uint8)
    sel = base.sel
    regions = sel.regions or []
    opt = (ctypes.c_uint32 * 10)(sel.excl, sel.incl, sel.min_mapq, len(regions), int(sel.keep_unplaced), lanes, case.min_hits,
                                 case.min_permille, int(case.invert), fill)
    reg = (ctypes.c_int64 * max(3 * len(regions), 1))(*[v for r in regions for v in r])
    h = np.ascontiguousarray(hits, dtype=np.uint32)
    w = np.ascontiguousarray(wins, dtype=np.uint32)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 6)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = lib.bam_records_cpu(data, len(data), c, len(cuts), opt, reg, h.ctypes.data, w.ctypes.data if windows else None, len(h),
                             out.ctypes.data, cap, tail0, ctypes.byref(on), st)
    return rc, out[:cap].tobytes(), on.value, list(st)


def _cuts(base):
    """Windows that end inside the header, inside a block_size word, inside a record's head and inside its last bytes; a comb."""
    d = br.decoded(base)
    mid = d.all_records[len(d.all_records) // 2]
    return [(), (d.hdr - 3, d.hdr + 2, mid.start + 1, mid.start + 20, mid.start + mid.size - 2), tuple(range(777, len(base.payload), 20_011))]


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_queue_bytes_are_the_models(lib, case, lanes):
    want, n_kept, keep, _, _ = br.expected(case)
    d = br.decoded(case.base)
    for cuts in _cuts(case.base)[:1 if case.base.name == "big" else 3]:
        # two fills into a buffer of exactly the model's size: a byte the copy did not write differs between the runs
        rc0, out0, n0, st0 = _run(lib, case, lanes, cuts, fill=0x00)
        rc1, out1, n1, st1 = _run(lib, case, lanes, cuts, fill=0xFF)
        assert rc0 == 0 and rc1 == 0, (cuts, rc0, rc1)
        assert n0 == n1 == len(want) and out0 == want and out1 == want, cuts
        assert st0[:3] == [len(d.records), d.excluded, n_kept] and st0 == st1


@pytest.mark.parametrize("lanes", [1, 64])
def test_a_tail_that_is_not_aligned_and_what_lies_in_front_of_it_stays(lib, lanes):
    """The queue holds bytes already: the copy starts at every residue modulo 16 and leaves the bytes in front alone."""
    case = next(c for c in CASES if c.name == "sizes__default")
    want = br.expected(case)[0]
    for tail0 in (1, 5, 15, 16, 33):
        for fill in (0x00, 0xFF):
            rc, out, n, _ = _run(lib, case, lanes, fill=fill, tail0=tail0)
            assert rc == 0 and n == len(want)
            assert out[:tail0] == bytes([fill]) * tail0 and out[tail0:] == want


@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_every_output_byte_is_written_exactly_once(lib, lanes):
    """Lane by lane, into bytes that were 0x00 and into bytes that were 0xFF, at all 16 x 16 residues of source and destination:
    the lanes' stores partition the record's bytes, none falls outside them, and every byte is the source's."""
    for length in list(range(1, 50)) + [63, 64, 65, 100, 1023, 1024, 1025, 1040, 16 * 64, 16 * 64 + 17, 60_000]:
        writes = np.zeros(length, np.uint32)
        for sa in range(16):
            for da in range(16):
                if length > 2000 and (sa * 16 + da) % 37:                        # (the long ones at a sample of the residues)
                    continue
                assert lib.bam_records_copy_writes(length, sa, da, lanes, writes.ctypes.data) == 0, (length, sa, da)
                assert (writes == 1).all(), (length, sa, da, np.nonzero(writes != 1)[0][:8])


def test_a_short_queue_a_malformed_record_and_entries_without_windows(lib):
    case = next(c for c in CASES if c.name == "aux__default")
    want = br.expected(case)[0]
    assert _run(lib, case, 64, cap=len(want) - 1)[0] == -5
    recs = br.decoded(case.base).all_records
    bad = bytearray(case.base.payload)
    bad[recs[7].start + 36 + len(recs[7].name)] = 1                              # the name's terminating NUL
    rc, _, n, st = _run(lib, case, 64, payload=bytes(bad))
    assert rc == -3 and st[5] == recs[7].start and n == 0
    rc, out, n, _ = _run(lib, case, 64, windows=False)                           # (mode 1: the rule reads 0 windows)
    assert rc == 0 and out == want


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver built as an executable with ASan + UBSan (host code; nothing is loaded into Python): every base but the
    largest, whole and in windows, into a queue of exactly the model's size — the model's bytes, and no report."""
    exe = str(tmp_path / "bam_records_san")
    src = os.path.join(ROOT, "tests", "bam_records_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr
    for case in CASES:
        base = case.base
        if base.name == "big":
            continue
        want, n_kept, _, hits, wins = br.expected(case)
        d = br.decoded(base)
        inp, ent, outp = tmp_path / (case.name + ".bin"), tmp_path / (case.name + ".ent"), tmp_path / (case.name + ".out")
        inp.write_bytes(base.payload)
        ent.write_bytes(np.asarray(hits, np.uint32).tobytes() + np.asarray(wins, np.uint32).tobytes())
        sel = base.sel
        regions = [str(v) for r in (sel.regions or []) for v in r]
        for lanes in (1, 64):
            for cuts in _cuts(base)[:2]:
                args = [exe, str(inp), str(ent), str(outp), str(len(want)), str(sel.excl), str(sel.incl), str(sel.min_mapq),
                        str(int(sel.keep_unplaced)), str(lanes), str(case.min_hits), str(case.min_permille), str(int(case.invert)),
                        str(len(regions) // 3)] + regions + [str(c) for c in cuts if 0 < c < len(base.payload)]
                run = subprocess.run(args, capture_output=True, text=True)
                assert run.returncode == 0 and not run.stderr, (run.returncode, run.stderr[-2000:])
                assert run.stdout.split() == [str(v) for v in (0, len(d.records), d.excluded, n_kept)]
                assert outp.read_bytes() == want


# ---------------------------------------------------------------------------------------------- the catalogue is not vacuous
def test_the_identity_no_selection_and_min_hits_0_keeps_the_file():
    for name in br.bases():
        case = br.identity_case(name)
        d = br.decoded(case.base)
        assert br.expected(case)[0] == case.base.payload[d.hdr:] and br.expected_file(case) == case.base.payload
        assert br.inflate(br.bam_file(case.base, block=997)) == case.base.payload


def test_the_model_reads_the_files_it_is_given():
    base = br.bases()["aux"]
    recs = br.decoded(base).all_records
    assert [r.name for r in recs] == [b"aux%d_%d" % (n, j) for n in br.AUX_SIZES for j in range(2)]
    assert [(r.ref, r.pos, r.mapq) for r in recs] == [(0, 100 * i, 30 + i) for i in range(len(br.AUX_SIZES)) for _ in range(2)]
    assert b"".join(base.payload[r.start:r.start + r.size] for r in recs) == base.payload[br.decoded(base).hdr:]
    rev = next(r for r in recs if r.flag & 0x10)
    assert br.fasta_of(rev, True) == b">\n" + br.bc.revcomp(rev.seq) + b"\n" and br.fasta_of(rev, False) == b">\n" + rev.seq + b"\n"


def test_every_feature_has_a_kept_and_a_dropped_record():
    kept = {f: 0 for f in br.FEATURES + br.FEATURES_KEPT}
    dropped = dict(kept)
    for case in br.all_cases():
        if (case.min_hits, case.min_permille, case.invert) != (1, 0, False):
            continue
        keep = br.expected(case)[2]
        assert 0 < keep.sum() < len(keep), case.name                              # every base under min_hits 1 keeps some, drops some
        for kp, feats in zip(keep, br.features(case.base)):
            for f in feats:
                (kept if kp else dropped)[f] += 1
    assert all(kept.values()), kept
    assert all(dropped[f] for f in br.FEATURES), dropped


def test_the_seams_the_cases_are_named_for():
    b = br.bases()
    by_name = {c.name: c for c in br.all_cases()}
    # sizes: 37 to 100 consecutively, each kept and dropped (37 and 38 hold no base: kept by min_hits 0 and by invert alone)
    sizes = br.decoded(b["sizes"])
    keep = br.expected(by_name["sizes__default"])[2]
    assert {r.size for r in sizes.records} == set(br.SIZES) and min(br.SIZES) == 37
    assert {r.size for r, kp in zip(sizes.records, keep) if kp} == set(range(39, 101))
    assert {r.size for r, kp in zip(sizes.records, keep) if not kp} == set(br.SIZES)
    for name in ("sizes__min_hits_0", "sizes__invert"):
        assert {37, 38} <= {r.size for r, kp in zip(sizes.records, br.expected(by_name[name])[2]) if kp}
    small = next(r for r in sizes.records if r.size == 37)
    assert small.name == b"" and small.seq == b""
    assert len(br.residues(by_name["sizes__default"])) == 256                     # all 16 x 16 residues of source and destination
    # records across tile boundaries, as they are named
    base, across = br.straddle_base()
    by_start = {r.start: r for r in br.decoded(base).all_records}
    for kind, start, size in across:
        r = by_start[start]
        assert r.size == size
        lo, hi = {"word1": (0, 4), "word2": (0, 4), "word3": (0, 4), "head": (4, 36), "aux": (size - 200, size)}[kind]
        assert (start + lo) // br.TILE + 1 == (start + hi - 1) // br.TILE, kind
        if kind.startswith("word"):
            assert br.TILE - start % br.TILE == int(kind[4])
    # long reads: whole tiles without a record start, a kept record right behind a kept and behind a dropped one
    long_ = br.decoded(b["long"])
    keep = br.expected(by_name["long__default"])[2]
    starts = {r.start // br.TILE for r in long_.all_records}
    outcomes = set()
    for i, r in enumerate(long_.records):
        if len(r.seq) in br.LONG:
            assert any(t not in starts for t in range(r.start // br.TILE + 1, (r.start + r.size) // br.TILE))
            assert keep[i + 1]
            outcomes.add((len(r.seq), bool(keep[i])))
    assert outcomes == {(n, kp) for n in br.LONG for kp in (True, False)}
    # the selection skips records between selected ones, each rule on its own
    sel = br.decoded(b["selection"])
    picked = [br.selected(r, b["selection"].sel) for r in sel.all_records]
    assert any(not picked[i] and picked[i - 1] and picked[i + 1] for i in range(1, len(picked) - 1)) and sel.excluded > 0
    for rule in ("excl", "incl", "min_mapq", "regions"):
        rest = b["selection"].sel._replace(**{rule: {"excl": 0, "incl": 0, "min_mapq": 0, "regions": None}[rule]})
        assert sum(br.selected(r, rest) for r in sel.all_records) > len(sel.records), rule
    assert any(r.pos < 1000 for r in sel.records)                                 # (a region reached through the CIGAR only)
    # tiles: one record alone, none selected, all kept
    base, (alone, none, all_kept, _) = br.tiles_base()
    d = br.decoded(base)
    keep = dict(zip((r.start for r in d.records), br.expected(by_name["tiles__default"])[2]))
    in_tile = lambda t: [r for r in d.all_records if r.start // br.TILE == t]
    assert len(in_tile(alone)) == 1 and keep[in_tile(alone)[0].start]
    assert len(in_tile(none)) > 10 and not any(r.start in keep for r in in_tile(none))
    assert len(in_tile(all_kept)) > 10 and all(keep[r.start] for r in in_tile(all_kept))
    # big: the kept bytes exceed 1 MiB
    assert len(br.decoded(b["big"]).records) == 4500 and len(br.expected(by_name["big__default"])[0]) > 1 << 20
    rules = {(c.min_hits > 1, c.min_hits == 0, c.min_permille > 0, c.invert) for c in br.all_cases()}
    assert len(rules) >= 5


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    from tests import record_hits_cases as rh
    bases, offsets = rh.reads_arrays([br.hit(60, 0), br.miss(60, 1)])
    batch = ReadBatch(bases, offsets)
    paths = {ext: str(tmp_path / ("r." + ext)) for ext in ("bam", "sam", "fq")}
    reads_io.write_bam(paths["bam"], batch)
    reads_io.write_sam(paths["sam"], batch)
    reads_io.write_fastq(paths["fq"], batch)
    return paths


def test_the_command_line_refuses_before_the_index_is_read(tmp_path, monkeypatch):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.bam")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out, "--bam-out"]   # (the index does not exist)
    for ext in ("fq", "sam"):
        with pytest.raises(ValueError, match="--bam-out applies to BAM input only"):
            run_argument_parser(common + ["-f", paths[ext]])
    for more, named in ((["--bam-to-fastq"], "--bam-to-fastq"), (["--as-stored"], "--as-stored"), (["--mate-suffix"], "--mate-suffix"),
                        (["--bam-pairs"], "--bam-pairs"), (["--bam-to-fastq", "--bam-pairs"], "--bam-to-fastq"),
                        (["--interleaved"], "--interleaved"), (["-f2", paths["bam"], "-o2", str(tmp_path / "o2")], "-f2/--reads2"),
                        (["-o2", str(tmp_path / "o2")], "-o2/--output2")):
        with pytest.raises(ValueError, match="--bam-out does not go with %s" % named):
            run_argument_parser(common + ["-f", paths["bam"]] + more)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
        run_argument_parser(common + ["-f", paths["bam"]])
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="is the input file"):
        run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-f", paths["bam"], "-o", paths["bam"], "--bam-out"])
    # a BAM file given with neither switch: the refusal of before, word for word, with a closing hint
    with pytest.raises(ValueError, match="select-reads does not read BAM files.*name.*--bam-to-fastq.*--bam-out"):
        run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out, "-f", paths["bam"]])
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "o2"))


def test_the_switch_passes_the_check_and_the_options_parse(tmp_path, monkeypatch):
    from kmer_mapper_amd import command_line_interface as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.bam")
    cli.check_select_reads_input("bam", 1, paths["bam"], out, False, ["--bam-out", "--regions"], True)
    cli.check_select_reads_bam_out("bam", [])
    args = cli.build_argument_parser().parse_args(
        ["select-reads", "-i", "i.npz", "-f", paths["bam"], "-o", out, "--bam-out", "--exclude-flags", "0x900", "--include-flags", "4",
         "--min-mapq", "7", "--regions", "c:1-5", "--regions", "d", "--regions-file", "r.bed", "--min-hits", "3", "--min-hit-permille", "20",
         "--invert", "--hits-output", "h"])
    assert (args.bam_out, args.exclude_flags, args.include_flags, args.min_mapq, args.regions, args.regions_file) == \
           (True, 0x900, 4, 7, ["c:1-5", "d"], "r.bed")
    assert (args.min_hits, args.min_hit_permille, args.invert, args.hits_output) == (3, 20, True, "h")
    plain = cli.build_argument_parser().parse_args(["select-reads", "-i", "i.npz", "-f", paths["bam"], "-o", out])
    assert "bam_out" not in vars(plain)                                           # (a call without it parses as it did before)
    # with the switch the call gets as far as the index file, which does not exist: every refusal lies in front of that
    seen = []
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", lambda a: seen.append(a) or (_ for _ in ()).throw(FileNotFoundError("index")))
    with pytest.raises(FileNotFoundError):
        cli.run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-f", paths["bam"], "-o", out, "--bam-out",
                                 "--exclude-flags", "0x900", "--invert"])
    assert len(seen) == 1 and not os.path.exists(out)


def test_the_sink_writes_the_header_once_then_the_members_then_the_end_of_file_block(monkeypatch):
    import io
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.gz_io import BGZF_EOF

    class Dev:
        device = 0

        def __init__(self):
            self.calls, self.header_ready, self.pending = [], False, 0

        def record_hits(self, on, windows=False):
            self.calls.append(("hits", on, windows))

        def record_keep(self, on, **rule):
            self.calls.append(("keep", on, rule))

        def record_bam(self, on):
            self.calls.append(("bam", on))

        def get_param(self, name):
            return {"record_hits_pending": 0}[name]

        def bam_header(self):
            if not self.header_ready:
                raise ValueError("no BAM stream with a header was started")
            return b"BAM\1header"

        def take_kept_bgzf(self, mate):
            n, self.pending = self.pending, 0
            return np.frombuffer(b"M" * n, np.uint8), 10 * n, n

    compressed = []
    import kmer_mapper_amd.util as util
    monkeypatch.setattr(util, "bgzf_compress", lambda data, device=0: compressed.append(bytes(data)) or np.frombuffer(b"<H>", np.uint8))
    dev, out = Dev(), io.BytesIO()
    sink = cli.RecordKeepSink(out, min_hits=2, bam_out=True)
    assert sink.bgzf and not sink.names
    sink.open(dev)
    assert dev.calls == [("hits", True, True), ("keep", True, dict(min_hits=2, min_permille=0, invert=False)), ("bam", True)]
    sink.drain(dev)                                                               # a first window inside the header: nothing yet
    assert out.getvalue() == b""
    dev.header_ready, dev.pending = True, 3
    sink.drain(dev)
    dev.pending = 2
    sink.drain(dev)
    sink.close()
    assert out.getvalue() == b"<H>MMMMM" + BGZF_EOF and compressed == [b"BAM\1header"]
    assert (sink.kept, sink.kept_bytes, sink.written) == (5, 50, 8 + len(BGZF_EOF))
    never = cli.RecordKeepSink(io.BytesIO(), bam_out=True)
    with pytest.raises(RuntimeError, match="header was never read"):
        never.close()
