"""CPU tier of the named FASTQ form of the BAM decode (include/kmm.h "record_names"): csrc/kmm_bam.hpp compiled by
itself with g++ and driven through run_call with CpuBackend's `named` switch on (tests/bam_fastq_cpu_driver.hpp), with 1 and 64
lanes, against the independent model of tests/bam_fastq_cases.py; once more as an executable under AddressSanitizer +
UndefinedBehaviorSanitizer (tests/bam_fastq_san_main.cpp: host code with its own main).  Also: the conditions that keep the
catalogue from being vacuous, and `select-reads --bam-to-fastq` up to the point where the index is read."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import bam_fastq_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
BASES = list(bc.bases().values())
BASE_IDS = [b.name for b in BASES]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_fastq")
    src = tmp / "shim.cpp"
    src.write_text('#include "bam_fastq_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), str(src),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.bam_fastq_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.bam_fastq_record_writes.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_void_p, ctypes.c_uint64]
    lib.bam_fastq_record_writes.restype = ctypes.c_int64
    return lib


def _options(base, lanes):
    sel = base.sel
    regions = sel.regions or []
    opt = (ctypes.c_uint32 * 8)(sel.excl, sel.incl, sel.min_mapq, len(regions), int(sel.keep_unplaced), int(base.orig), int(base.suffix),
                                lanes)
    reg = (ctypes.c_int64 * max(3 * len(regions), 1))(*[v for r in regions for v in r])
    return opt, reg


def _run(lib, base, lanes, cuts=(), fill=0, cap=None):
    data = base.payload
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    cap = len(bc.decoded(base).text) if cap is None else cap                     # (exactly the model's size: no slack to hide in)
    out = np.full(cap, fill, np.uint8)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 10)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    opt, reg = _options(base, lanes)
    rc = lib.bam_fastq_cpu(data, len(data), c, len(cuts), opt, reg, out.ctypes.data, cap, ctypes.byref(on), st)
    return rc, out[:on.value].tobytes(), list(st)


def _cuts(base):
    """Windows that end inside the header, inside a record's head, inside a name and inside its qualities, and a regular comb."""
    _, recs, hdr = bc.read_bam(base.payload)
    mid = recs[len(recs) // 2]
    return [(), (hdr - 3, hdr + 17, mid.start + 20, mid.start + 36 + max(len(mid.name) // 2, 1), mid.start + mid.size - 2),
            tuple(range(777, len(base.payload), 20_011))]


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("base", BASES, ids=BASE_IDS)
def test_the_decoded_text_is_the_models(lib, base, lanes):
    d = bc.decoded(base)
    for cuts in _cuts(base):
        # two fills: a byte decode() did not write differs between the runs, so equal outputs mean every byte was written
        rc0, out0, st0 = _run(lib, base, lanes, cuts, fill=0x00)
        rc1, out1, st1 = _run(lib, base, lanes, cuts, fill=0xFF)
        assert rc0 == 0 and rc1 == 0, (cuts, rc0, rc1)
        assert out0 == d.text and out1 == d.text, cuts                          # (out_bytes == the text's length: both have it)
        assert st0[:2] == [len(d.records), d.excluded] and st0 == st1
        assert st0[7:10] == [d.no_qual, d.reversed, d.replaced], cuts


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("base", [b for b in BASES if b.name != "big"], ids=[n for n in BASE_IDS if n != "big"])
def test_every_output_byte_is_written_exactly_once(lib, base, lanes):
    """Lane by lane, into bytes that were 0x00 and into bytes that were 0xFF: the lanes' writes partition the record's bytes."""
    d = bc.decoded(base)
    for r, text in zip(d.records, d.texts):
        rec = base.payload[r.start:r.start + r.size]
        writes = np.zeros(len(text), np.uint32)
        n = lib.bam_fastq_record_writes(rec, len(rec), lanes, int(base.suffix), int(base.orig), writes.ctypes.data, len(text))
        assert n == len(text), (r.name, n)
        assert (writes == 1).all(), (r.name, np.nonzero(writes != 1)[0][:8])


def test_a_short_output_buffer_and_a_malformed_record(lib):
    base = bc.bases()["names"]
    assert _run(lib, base, 64, cap=len(bc.decoded(base).text) - 1)[0] == -5
    _, recs, _ = bc.read_bam(base.payload)
    bad = bytearray(base.payload)
    at = recs[7].start
    bad[at + 36 + len(recs[7].name)] = 1                                        # the name's terminating NUL
    rc, _, st = _run(lib, base._replace(name="names_bad", payload=bytes(bad)), 64, cap=1 << 16)
    assert rc == -3 and st[6] == at


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver built as an executable with ASan + UBSan (host code; nothing is loaded into Python): every base but the
    largest, whole and in windows, into an output buffer of exactly the model's size — the model's bytes, and no report."""
    exe = str(tmp_path / "bam_fastq_san")
    src = os.path.join(ROOT, "tests", "bam_fastq_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr
    for base in BASES:
        if base.name == "big":
            continue
        d = bc.decoded(base)
        inp, outp = tmp_path / (base.name + ".bin"), tmp_path / (base.name + ".out")
        inp.write_bytes(base.payload)
        sel = base.sel
        regions = [str(v) for r in (sel.regions or []) for v in r]
        for lanes in (1, 64):
            for cuts in _cuts(base)[:2]:
                args = [exe, str(inp), str(outp), str(len(d.text)), str(sel.excl), str(sel.incl), str(sel.min_mapq), str(int(sel.keep_unplaced)),
                        str(int(base.orig)), str(int(base.suffix)), str(lanes), str(len(regions) // 3)] + regions + \
                       [str(c) for c in cuts if 0 < c < len(base.payload)]
                run = subprocess.run(args, capture_output=True, text=True)
                assert run.returncode == 0 and not run.stderr, run.stderr[-2000:]
                assert run.stdout.split() == [str(v) for v in (0, len(d.records), d.excluded, d.no_qual, d.reversed, d.replaced)]
                assert outp.read_bytes() == d.text


# ---------------------------------------------------------------------------------------------- the catalogue is not vacuous
def test_the_model_reads_the_files_it_is_given():
    """The model's reader against the writer's own arguments, through a BGZF file: names, flags, letters and raw qualities."""
    base = bc.bases()["names"]
    assert bc.inflate(bc.bam_file(base, block=997)) == base.payload
    _, recs, _ = bc.read_bam(base.payload)
    names = [bc.name_of(n, n) for n in bc.NAME_LENGTHS] + [b"*"] + list(bc.BAD_NAMES)
    assert [r.name for r in recs] == [nm for nm in names for _ in range(2)]
    assert all(r.flag == 4 and r.qual == bc.ramp(len(r.seq)) and set(r.seq) <= set(b"ACGT") for r in recs)
    text, replaced, rev, absent = bc.fastq_of(recs[2 * len(bc.NAME_LENGTHS) + 2])           # b"tab\there"
    assert text.startswith(b"@tab?here\n") and (replaced, rev, absent) == (1, False, False)
    # the sixteen codes reversed and complemented, written out by hand (= and N are their own complements)
    assert bc.decoded(bc.bases()["all_codes"]).texts[1].split(b"\n")[1] == b"T" + b"NVHMDRWABSYCKGT=" * 4


def test_every_feature_has_a_kept_and_a_dropped_record():
    kept = {f: 0 for f in bc.FEATURES}
    dropped = dict(kept)
    for case in bc.gpu_cases():
        if (case.min_hits, case.min_permille, case.invert) != (1, 0, False):
            continue
        keep = bc.expected(case)[2]
        assert 0 < keep.sum() < len(keep), case.name                              # every base under min_hits 1 keeps some, drops some
        for kp, feats in zip(keep, bc.features(case.base)):
            for f in feats:
                (kept if kp else dropped)[f] += 1
    assert all(kept.values()) and all(dropped.values()), (kept, dropped)


def test_the_seams_the_cases_are_named_for():
    b = bc.bases()
    _, recs, _ = bc.read_bam(b["names"].payload)
    assert {len(r.name) for r in recs} >= set(bc.NAME_LENGTHS) and b"*" in {r.name for r in recs}
    assert bc.decoded(b["names"]).replaced == sum(1 for nm in bc.BAD_NAMES for c in nm if not 0x21 <= c <= 0x7E) * 2 > 0
    _, recs, _ = bc.read_bam(b["lengths"].payload)
    assert {len(r.seq) for r in recs} >= set(bc.SEQ_LENGTHS) and max(r.size for r in recs) > 3 * bc.TILE
    base, across = bc.straddle_base()
    _, recs, _ = bc.read_bam(base.payload)
    by_start = {r.start: r for r in recs}
    for kind, start, size in across:
        r = by_start[start]
        lo, hi = {"head": (0, 36), "name": (36, 36 + len(r.name)), "qual": (r.size - len(r.seq), r.size)}[kind]
        assert (start + lo) // bc.TILE + 1 == (start + hi - 1) // bc.TILE, kind     # the part itself lies across the boundary
    _, recs, _ = bc.read_bam(b["quals"].payload)
    assert {r.qual[0] for r in recs if r.seq} >= {0xFF, 0, 92, 93, 254}
    flags = {r.flag & 0xC0 for r in bc.read_bam(b["mates_suffix"].payload)[1]}
    assert flags == {0, 0x40, 0x80, 0xC0}
    sel = bc.decoded(b["selection"])
    _, recs, _ = bc.read_bam(b["selection"].payload)
    picked = [bc.selected(r, bc.SELECTION) for r in recs]
    assert any(not picked[i] and picked[i - 1] and picked[i + 1] for i in range(1, len(recs) - 1)) and sel.excluded > 0
    for rule in ("excl", "incl", "min_mapq", "regions"):                            # every rule drops a record the others let through
        rest = bc.SELECTION._replace(**{rule: {"excl": 0, "incl": 0, "min_mapq": 0, "regions": None}[rule]})
        assert sum(bc.selected(r, rest) for r in recs) > len(sel.records), rule
    big = bc.decoded(b["big"])
    assert len(big.text) > 1 << 20
    keep = bc.expected(next(c for c in bc.all_cases() if c.name == "big__default"))[2]
    ends = np.cumsum([len(t) for t in big.texts])
    assert keep[ends <= 1 << 20].any() and keep[ends > (1 << 20) + 400].any()       # kept text from both sides of the super-tile seam
    rules = {(c.min_hits > 1, c.min_hits == 0, c.min_permille > 0, c.invert) for c in bc.all_cases()}
    assert len(rules) >= 5


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    from tests import record_hits_cases as rh
    bases, offsets = rh.reads_arrays([bc.hit(60, 0), bc.miss(60, 1)])
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
    out = str(tmp_path / "kept.fq")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out]      # (the index does not exist)
    with pytest.raises(ValueError, match="select-reads does not read BAM files.*name.*--bam-to-fastq"):
        run_argument_parser(common + ["-f", paths["bam"]])
    for more in ([], ["--bam-to-fastq"]):
        with pytest.raises(ValueError, match="select-reads does not read SAM files.*name"):
            run_argument_parser(common + ["-f", paths["sam"]] + more)
    for option in (["--bam-to-fastq"], ["--exclude-flags", "0x900"], ["--include-flags", "4"], ["--min-mapq", "3"], ["--regions", "c:1-5"],
                   ["--regions-file", str(tmp_path / "r.bed")], ["--as-stored"], ["--mate-suffix"]):
        with pytest.raises(ValueError, match="%s applies to BAM input only" % option[0]):
            run_argument_parser(common + ["-f", paths["fq"]] + option)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE=2.*out of scope"):
        run_argument_parser(common + ["-f", paths["bam"], "--bam-to-fastq"])
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="is the input file"):
        run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-f", paths["bam"], "-o", paths["bam"],
                             "--bam-to-fastq"])
    assert not os.path.exists(out)


def test_a_bam_file_with_the_switch_passes_the_check_and_the_options_parse(tmp_path, monkeypatch):
    from kmer_mapper_amd import command_line_interface as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.fq")
    cli.check_select_reads_input("bam", 1, paths["bam"], out, True, ["--bam-to-fastq", "--regions"])
    cli.check_select_reads_input("fastq", 1, paths["fq"], out)                             # as before the switch existed
    args = cli.build_argument_parser().parse_args(
        ["select-reads", "-i", "i.npz", "-f", paths["bam"], "-o", out, "--bam-to-fastq", "--exclude-flags", "0x900", "--include-flags", "4",
         "--min-mapq", "7", "--regions", "c:1-5", "--regions", "d", "--regions-file", "r.bed", "--as-stored", "--mate-suffix", "--min-hits",
         "3", "--min-hit-permille", "20", "--invert", "--hits-output", "h"])
    assert (args.bam_to_fastq, args.exclude_flags, args.include_flags, args.min_mapq, args.regions, args.regions_file, args.as_stored,
            args.mate_suffix) == (True, 0x900, 4, 7, ["c:1-5", "d"], "r.bed", True, True)
    assert (args.min_hits, args.min_hit_permille, args.invert, args.hits_output) == (3, 20, True, "h")
    plain = cli.build_argument_parser().parse_args(["select-reads", "-i", "i.npz", "-f", paths["bam"], "-o", out])
    new = {"bam_to_fastq", "exclude_flags", "include_flags", "min_mapq", "regions", "regions_file", "as_stored", "mate_suffix"}
    assert not new & set(vars(plain))                                             # (a call without them parses as it did before)
    # with the switch the call gets as far as the index file, which does not exist: every refusal lies in front of that
    seen = []
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", lambda a: seen.append(a) or (_ for _ in ()).throw(FileNotFoundError("index")))
    with pytest.raises(FileNotFoundError):
        cli.run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-f", paths["bam"], "-o", out, "--bam-to-fastq",
                                 "--exclude-flags", "0x900", "--mate-suffix"])
    assert len(seen) == 1


def test_the_sink_switches_the_names_on_and_reads_the_counters():
    from kmer_mapper_amd.command_line_interface import RecordKeepSink

    class Dev:
        def __init__(self):
            self.calls = []

        def record_hits(self, on, windows=False):
            self.calls.append(("hits", on, windows))

        def record_keep(self, on, **rule):
            self.calls.append(("keep", on, rule))

        def record_names(self, on, mate_suffix=False):
            self.calls.append(("names", on, mate_suffix))

        def get_param(self, name):
            return {"records_reversed": 3, "records_without_qual": 0, "record_name_bytes_replaced": 2}[name]

    dev = Dev()
    sink = RecordKeepSink(None, min_hits=2, names=True, mate_suffix=True)
    sink.open(dev)
    sink.finish(dev)
    assert dev.calls == [("hits", True, True), ("keep", True, dict(min_hits=2, min_permille=0, invert=False)), ("names", True, True)]
    assert sink.counters == {"records_reversed": 3, "records_without_qual": 0, "record_name_bytes_replaced": 2}
    dev = Dev()
    sink = RecordKeepSink(None)
    sink.open(dev)
    sink.finish(dev)
    assert [c[0] for c in dev.calls] == ["hits", "keep"] and sink.counters == {}
