"""CPU tier of mates kept together in BAM output (include/kmm.h "record_bam_mates"): csrc/kmm_bam.hpp compiled by
itself with g++ and driven through run_call and CpuBackend's raw_count_pairs() + raw_pair_names() + raw_carry_copy() +
raw_copy_pairs() (tests/bam_mates_cpu_driver.hpp) — the plain C++ the kernels run — with 1 and 64 lanes, against the independent
model of tests/bam_mates_cases.py; once more as an executable under AddressSanitizer + UndefinedBehaviorSanitizer
(tests/bam_mates_san_main.cpp: host code with its own main).  Also: the conditions that keep the catalogue from being vacuous,
and `select-reads --bam-out --keep-mates` up to the point where the index is read."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import bam_mates_cases as bm
from tests import bam_records_cases as br
from tests import record_pairs_cases as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
CASES = bm.all_cases()
GOOD, BAD = bm.good_cases(), bm.error_cases()
PAIR_RULE = {rp.ANY: 0, rp.BOTH: 1}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bam_mates")
    src = tmp / "shim.cpp"
    src.write_text('#include "bam_mates_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), str(src),
                           "-o", so])
    lib = ctypes.CDLL(so)
    lib.bam_mates_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                  ctypes.c_void_p, ctypes.c_void_p]
    lib.bam_mates_names_differ.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
    return lib


def _cuts(case, whole=False):
    """The windows of the case as offsets into the payload (the driver's cuts), the payload's end last."""
    hdr = br.decoded(case.base).hdr
    return [len(case.base.payload)] if whole else [hdr + w for w in bm.window_ends(case)]


def _want(case):
    """What the stream leaves in the queue: every kept pair — for an error case the pairs of the windows before the failing one."""
    if case.error is None:
        return bm.expected(case)
    i = bm.window_of(case)
    done = bm.selected_done(case)
    return bm.expected(case, done[i - 1] // 2 if i else 0)


def _run(lib, case, lanes, fill=0, whole=False, tail0=0, cap=None):
    base = case.base
    data = base.payload
    want = bm.expected(case, 0) if whole and case.error is not None else _want(case)
    hits, wins = bm.entries(base)
    cuts = _cuts(case, whole)
    cap = tail0 + len(want.raw) if cap is None else cap                           # (exactly the model's size: no slack to hide in)
    out = np.full(max(cap, 1), fill ^ 0x5A, np.uint8)
    sel = base.sel
    regions = sel.regions or []
    opt = (ctypes.c_uint32 * 11)(sel.excl, sel.incl, sel.min_mapq, len(regions), int(sel.keep_unplaced), lanes, case.min_hits,
                                 case.min_permille, int(case.invert), fill, PAIR_RULE[case.pair_rule])
    reg = (ctypes.c_int64 * max(3 * len(regions), 1))(*[v for r in regions for v in r])
    h = np.ascontiguousarray(hits, dtype=np.uint32)
    w = np.ascontiguousarray(wins, dtype=np.uint32)
    on = ctypes.c_uint64(0)
    st = (ctypes.c_uint64 * 8)()
    c = (ctypes.c_uint64 * len(cuts))(*cuts)
    rc = lib.bam_mates_cpu(data, len(data), c, len(cuts), opt, reg, h.ctypes.data, w.ctypes.data, len(h), out.ctypes.data, cap, tail0,
                           ctypes.byref(on), st)
    return rc, out[:cap].tobytes(), on.value, list(st)


# ---------------------------------------------------------------------------------------------- the shared C++ against the model
@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("case", GOOD, ids=[c.name for c in GOOD])
def test_the_queue_bytes_are_the_models(lib, case, lanes):
    want = bm.expected(case)
    d = br.decoded(case.base)
    for whole in ((True,) if not case.cuts else (True, False)):
        # two fills into a buffer of exactly the model's size: a byte the copy did not write differs between the runs
        rc0, out0, n0, st0 = _run(lib, case, lanes, fill=0x00, whole=whole)
        rc1, out1, n1, st1 = _run(lib, case, lanes, fill=0xFF, whole=whole)
        assert rc0 == 0 and rc1 == 0, (whole, rc0, rc1)
        assert n0 == n1 == len(want.raw) and out0 == want.raw and out1 == want.raw, whole
        assert st0[:3] == [len(d.records), d.excluded, want.n_records] and st0 == st1


@pytest.mark.parametrize("lanes", [1, 64])
@pytest.mark.parametrize("case", BAD, ids=[c.name for c in BAD])
def test_strangers_and_unpaired_ends_fail_the_window_that_completes_them(lib, case, lanes):
    kind, number = case.error
    for whole in ((True,) if not case.cuts else (True, False)):
        rc, out, n, st = _run(lib, case, lanes, whole=whole)
        assert rc == {"strangers": -10, "unpaired": -11}[kind] and st[6] == number, (whole, rc, st)
        if whole:
            assert n == 0                                                         # (one call: it appends nothing)
        else:
            assert st[7] == bm.window_of(case)
            assert n == len(_want(case).raw) and out == _want(case).raw           # (what the windows before it appended stays)


@pytest.mark.parametrize("lanes", [1, 64])
def test_a_tail_that_is_not_aligned_and_what_lies_in_front_of_it_stays(lib, lanes):
    for name in ("residues__any", "kept_carry_at_a_filled_queue__any"):
        case = bm.by_name(name)
        want = bm.expected(case).raw
        for tail0 in (1, 5, 15, 16, 33):
            for fill in (0x00, 0xFF):
                rc, out, n, _ = _run(lib, case, lanes, fill=fill, tail0=tail0)
                assert rc == 0 and n == len(want)
                assert out[:tail0] == bytes([fill]) * tail0 and out[tail0:] == want
    assert _run(lib, bm.by_name("patterns__any"), 64, cap=len(bm.expected(bm.by_name("patterns__any")).raw) - 1)[0] == -5


NAME_CASES = [(b"abc", b"abc", False), (b"", b"", False), (b"x" * 254, b"x" * 254, False),
              (b"Abc", b"abc", True), (b"abc", b"abd", True), (b"abc", b"ab", True), (b"ab", b"abc", True), (b"", b"a", True)] + \
             [(bytes(100), bytes(i) + b"\x01" + bytes(99 - i), True) for i in (0, 62, 63, 64, 65, 99)] + \
             [(b"q" * 254, b"q" * 253 + b"r", True), (b"q" * 254, b"r" + b"q" * 253, True), (b"own/1", b"own/2", True), (b"own", b"own/2", True)]


@pytest.mark.parametrize("lanes", [1, 3, 64])
def test_the_name_comparison(lib, lanes):
    """read_name as it stands, the NUL included: equal l_read_name and equal bytes, nothing trimmed."""
    for a, b, differ in NAME_CASES:
        assert (a != b) == differ
        assert lib.bam_mates_names_differ(a + b"\0", len(a) + 1, b + b"\0", len(b) + 1, lanes) == int(differ), (a, b)
    for case in CASES:                                                            # and on every pair of every case
        recs = bm.selected_records(case.base)
        for p in range(len(recs) // 2):
            a, b = bytes(recs[2 * p].name), bytes(recs[2 * p + 1].name)
            assert lib.bam_mates_names_differ(a + b"\0", len(a) + 1, b + b"\0", len(b) + 1, lanes) == int(a != b)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver built as an executable with ASan + UBSan (host code; nothing is loaded into Python): every case in its
    windows, into a queue of exactly the model's size — the model's bytes, the model's error, and no report."""
    exe = str(tmp_path / "bam_mates_san")
    src = os.path.join(ROOT, "tests", "bam_mates_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    probe = tmp_path / "probe.cpp"                                               # is there a sanitizer runtime to link against at all?
    probe.write_text("int main() { return 0; }\n")
    linked = subprocess.run(["g++", "-fsanitize=address,undefined", str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if linked.returncode != 0:
        pytest.skip("no sanitizer runtime on this box: " + linked.stderr[-200:])
    build = subprocess.run(cmd, capture_output=True, text=True)                  # (with one, a failing build is a failure)
    assert build.returncode == 0, build.stderr
    for case in CASES:
        base = case.base
        want = _want(case)
        hits, wins = bm.entries(base)
        d = br.decoded(base)
        inp, ent, outp = tmp_path / (case.name + ".bin"), tmp_path / (case.name + ".ent"), tmp_path / (case.name + ".out")
        inp.write_bytes(base.payload)
        ent.write_bytes(np.asarray(hits, np.uint32).tobytes() + np.asarray(wins, np.uint32).tobytes())
        sel = base.sel
        regions = [str(v) for r in (sel.regions or []) for v in r]
        for lanes in (1, 64):
            args = [exe, str(inp), str(ent), str(outp), str(len(want.raw)), str(sel.excl), str(sel.incl), str(sel.min_mapq),
                    str(int(sel.keep_unplaced)), str(lanes), str(case.min_hits), str(case.min_permille), str(int(case.invert)),
                    str(PAIR_RULE[case.pair_rule]), str(len(regions) // 3)] + regions + [str(c) for c in _cuts(case)[:-1]]
            run = subprocess.run(args, capture_output=True, text=True)
            assert run.returncode == 0 and not run.stderr, (case.name, run.returncode, run.stderr[-2000:])
            got = run.stdout.split()
            if case.error is None:
                assert got[:4] == [str(v) for v in (0, len(d.records), d.excluded, want.n_records)], case.name
            else:
                assert got[0] == {"strangers": "-10", "unpaired": "-11"}[case.error[0]] and got[4] == str(case.error[1]), case.name
                assert got[5] == str(bm.window_of(case))
            assert outp.read_bytes() == want.raw, case.name


# ---------------------------------------------------------------------------------------------- the catalogue is not vacuous
def test_every_seam_kind_occurs():
    seen = {}
    for case in GOOD:
        for kind in bm.seam_kinds(case):
            seen.setdefault(kind, case.name)
    assert set(bm.SEAM_KINDS) <= set(seen), sorted(set(bm.SEAM_KINDS) - set(seen))
    # the unselected runs occur under a selection that is not flags only too (the walk then asks the whole predicate)
    mapq = set().union(*(bm.seam_kinds(c) for c in GOOD if not _flags_only(c.base.sel)))
    assert {"one unselected record between the mates", "an unselected run across a tile boundary",
            "an unselected run longer than a tile", "unselected records behind the last pair"} <= mapq
    long_pairs = bm.seam_kinds(bm.by_name("lengths__any"))
    assert {"mate 2 several tiles on", "a tile without a record start between the mates"} <= long_pairs


def _flags_only(sel):
    return not sel.incl and not sel.min_mapq and not sel.regions


def test_the_four_decision_kinds_occur_under_both_rules_with_and_without_invert_and_per_mille():
    every = {"only mate 1", "only mate 2", "both", "neither"}
    for pair_rule, invert in bm.RULES:
        for permille in (0, 150):
            cases = [c for c in GOOD if (c.pair_rule, c.invert) == (pair_rule, invert) and c.min_permille == permille and c.min_hits == 1]
            assert cases and every <= set().union(*(bm.decision_kinds(c) for c in cases)), (pair_rule, invert, permille)
    # under ANY a pair with one matching mate is kept, under BOTH it is dropped: the rules differ on the catalogue's pairs
    a, b = bm.expected(bm.by_name("patterns__any")).keep, bm.expected(bm.by_name("patterns__both")).keep
    assert a.tolist() == [True, True, True, False, True] and b.tolist() == [False, False, True, False, False]
    pa, pb = bm.expected(bm.by_name("permille_150__any")).keep, bm.expected(bm.by_name("permille_150__both")).keep
    assert pa.any() and not pa.all() and pb.any() and (pa != pb).any()
    assert (bm.expected(bm.by_name("patterns__any_invert")).keep == ~a).all()
    nothing, everything = bm.expected(bm.by_name("patterns__nothing_kept")), bm.expected(bm.by_name("patterns__everything_kept"))
    assert nothing.n_records == 0 and nothing.raw == b""
    base = bm.by_name("patterns__everything_kept").base
    assert everything.keep.all() and everything.raw == base.payload[br.decoded(base).hdr:]


def test_all_sixteen_destination_residues_for_either_mate_at_changing_source_residues():
    first, second = bm.residues(bm.by_name("residues__any"))
    for got in (first, second):
        assert {dst for _, dst in got} == set(range(16))
        assert len({(src - dst) % 16 for src, dst in got}) >= 8                   # (the source moves against the destination)
    keep = bm.expected(bm.by_name("residues__any")).keep
    assert keep.tolist() == [True, False] * 20                                    # (kept pairs behind dropped ones)


def test_every_window_kind_occurs():
    seen = {}
    for case in CASES:
        for kind in bm.window_kinds(case):
            seen.setdefault(kind, case.name)
    assert set(bm.WINDOW_KINDS) <= set(seen), sorted(set(bm.WINDOW_KINDS) - set(seen))
    assert "three windows in a row that end odd" in bm.window_kinds(bm.by_name("three_windows_end_odd__any"))
    assert "a window whose only selected record is the carry's mate" in bm.window_kinds(bm.by_name("only_the_carrys_mate__any"))
    assert "a kept carried pair at a queue residue of not 0" in bm.window_kinds(bm.by_name("kept_carry_at_a_filled_queue__any"))
    assert "a dropped carried pair" in bm.window_kinds(bm.by_name("dropped_carry__any"))
    assert "a window with no selected record while a carry waits" in bm.window_kinds(bm.by_name("carry_over_empty_windows__any"))


def test_the_name_kinds_and_the_errors_the_cases_are_named_for():
    names = bm.selected_records(bm.by_name("names__any").base)
    assert {len(r.name) for r in names} == {0, 1, 63, 64, 65, 254}
    keep = bm.expected(bm.by_name("names__any")).keep
    assert keep.tolist() == [True, False] * 6
    errors = {c.name: c.error for c in BAD}
    assert errors["coordinate_sorted"] == ("strangers", 0)
    assert errors["last_byte_at_pair_0"] == ("strangers", 0) and errors["first_byte_in_the_middle"] == ("strangers", 9)
    assert errors["prefix_in_the_last_pair"] == ("strangers", 19) and errors["longer_in_the_middle"] == ("strangers", 10)
    for at in (63, 64, 65):
        case = bm.by_name("strangers_differ_at_byte_%d" % at)
        assert case.error == ("strangers", 5)
        a, b = bm.selected_records(case.base)[10:12]
        assert len(a.name) == len(b.name) == 100 and [i for i in range(100) if a.name[i] != b.name[i]] == [at]
    astride = bm.by_name("astride_the_carry")                                     # strangers whose mate 1 is the carry
    assert astride.error == ("strangers", 7) and bm.selected_done(astride)[bm.window_of(astride) - 1] == 15
    assert bm.by_name("strangers_in_windows").error == ("strangers", 11) and bm.window_of(bm.by_name("strangers_in_windows")) > 0
    assert errors["odd_count"] == ("unpaired", 13) and errors["odd_count_in_windows"] == ("unpaired", 13)
    assert bm.by_name("odd_count_in_windows").cuts and errors["a_selection_that_removes_one_mate"][0] == "unpaired"
    assert errors["trio_with_0x900_not_excluded"][0] == "strangers"
    # an error case whose failing call finds a mate 1 waiting: tests/test_gpu_bam_mates.py then looks at the carry behind the
    # failure (for an unpaired end it does so behind a last call that brings no member)
    waiting = [c.name for c in BAD if bm.window_of(c) and bm.selected_done(c)[bm.window_of(c) - 1] % 2]
    assert "astride_the_carry" in waiting, waiting


def test_the_model_reads_the_files_it_is_given():
    case = bm.by_name("patterns__any")
    d = br.decoded(case.base)
    assert [r.name for r in d.records] == [b"p%d" % (i // 2) for i in range(10)]
    want = bm.expected(case)
    p = case.base.payload
    assert want.raw == b"".join(p[r.start:r.start + r.size] for i, r in enumerate(d.records) if i // 2 != 3)
    assert bm.expected_file(case) == p[:d.hdr] + want.raw and want.n_records == 8
    assert br.inflate(br.bam_file(case.base, block=97)) == p
    data, windows = bm.windowed_file(bm.by_name("three_windows_end_odd__any"))
    assert br.inflate(data) == p and len(windows) == 4


# ---------------------------------------------------------------------------------------------- the command line
def _files(tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    from tests import record_hits_cases as rh
    bases, offsets = rh.reads_arrays([br.hit(60, 0), br.miss(60, 1)])
    batch = ReadBatch(bases, offsets)
    paths = {ext: str(tmp_path / ("r." + ext)) for ext in ("bam", "fq")}
    reads_io.write_bam(paths["bam"], batch)
    reads_io.write_fastq(paths["fq"], batch)
    return paths


def test_the_command_line_refuses_before_the_index_is_read(tmp_path, monkeypatch):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.bam")
    common = ["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-o", out]                   # (the index does not exist)
    for more in ([], ["--bam-to-fastq"], ["--bam-to-fastq", "--bam-pairs"], ["--pair-rule", "both"]):
        with pytest.raises(ValueError, match="--keep-mates goes with --bam-out.*--bam-to-fastq --bam-pairs.*--interleaved"):
            run_argument_parser(common + ["-f", paths["bam"], "--keep-mates"] + more)
    with pytest.raises(ValueError, match="--keep-mates goes with --bam-out"):
        run_argument_parser(common + ["-f", paths["fq"], "--keep-mates"])
    with pytest.raises(ValueError, match="--bam-out applies to BAM input only"):
        run_argument_parser(common + ["-f", paths["fq"], "--bam-out", "--keep-mates"])
    # what --bam-out refuses stays refused with --keep-mates, word for word
    for more, named in ((["--bam-pairs"], "--bam-pairs"), (["--interleaved"], "--interleaved"),
                        (["-f2", paths["bam"], "-o2", str(tmp_path / "o2")], "-f2/--reads2"), (["-o2", str(tmp_path / "o2")], "-o2/--output2")):
        with pytest.raises(ValueError, match="--bam-out does not go with %s: mates are not kept together in BAM output" % named):
            run_argument_parser(common + ["-f", paths["bam"], "--bam-out", "--keep-mates"] + more)
    # --pair-rule without a pair form stays refused
    with pytest.raises(ValueError, match="--pair-rule goes with --interleaved or -f2/--reads2"):
        run_argument_parser(common + ["-f", paths["bam"], "--bam-out", "--pair-rule", "both"])
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "o2"))


def test_the_switch_passes_the_checks_and_the_options_parse(tmp_path, monkeypatch):
    from kmer_mapper_amd import command_line_interface as cli
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    paths = _files(tmp_path)
    out = str(tmp_path / "kept.bam")
    cli.check_select_reads_keep_mates(True, True)
    cli.check_select_reads_keep_mates(False, False)
    args = cli.build_argument_parser().parse_args(
        ["select-reads", "-i", "i.npz", "-f", paths["bam"], "-o", out, "--bam-out", "--keep-mates", "--pair-rule", "both", "--exclude-flags",
         "0x400", "--include-flags", "1", "--min-mapq", "7", "--regions", "c:1-5", "--regions-file", "r.bed", "--min-hits", "3",
         "--min-hit-permille", "20", "--invert", "--hits-output", "h"])
    assert (args.bam_out, args.keep_mates, args.pair_rule, args.exclude_flags, args.include_flags, args.min_mapq, args.regions,
            args.regions_file) == (True, True, "both", 0x400, 1, 7, ["c:1-5"], "r.bed")
    assert (args.min_hits, args.min_hit_permille, args.invert, args.hits_output) == (3, 20, True, "h")
    plain = cli.build_argument_parser().parse_args(["select-reads", "-i", "i.npz", "-f", paths["bam"], "-o", out, "--bam-out"])
    assert "keep_mates" not in vars(plain)                                        # (a call without it parses as it did before)
    # with the switch the call gets as far as the index file, which does not exist; 0x900 is ORed into the exclude mask before
    seen, routes = [], []
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", lambda a: seen.append(a) or (_ for _ in ()).throw(FileNotFoundError("index")))
    check = cli._check_bam_route
    monkeypatch.setattr(cli, "_check_bam_route", lambda fmt, world, excl: routes.append(excl) or check(fmt, world, excl))
    with pytest.raises(FileNotFoundError):
        cli.run_argument_parser(["select-reads", "-i", str(tmp_path / "none.npz"), "-k", "5", "-f", paths["bam"], "-o", out, "--bam-out",
                                 "--keep-mates", "--pair-rule", "both", "--exclude-flags", "0x400"])
    assert len(seen) == 1 and routes == [0xD00] and not os.path.exists(out)


def test_the_sink_turns_the_mates_on_with_the_pair_rule():
    import io
    from kmer_mapper_amd import command_line_interface as cli

    class Dev:
        device = 0

        def __init__(self):
            self.calls = []

        def record_hits(self, on, windows=False):
            self.calls.append(("hits", on, windows))

        def record_keep(self, on, **rule):
            self.calls.append(("keep", on, rule))

        def record_bam(self, on, mates=False):
            self.calls.append(("bam", on, mates))

        def record_pairs(self, on, rule="any"):
            self.calls.append(("pairs", on, rule))

    dev = Dev()
    sink = cli.RecordKeepSink(io.BytesIO(), min_hits=2, bam_out=True, bam_mates=True, pair_rule="both")
    assert sink.bgzf and sink.bam_mates and not sink.names
    sink.open(dev)
    assert dev.calls == [("hits", True, True), ("keep", True, dict(min_hits=2, min_permille=0, invert=False)), ("bam", True, True),
                         ("pairs", False, "both")]
    assert not cli.RecordKeepSink(io.BytesIO(), bam_mates=True).bam_mates          # (without BAM out there is nothing to pair)
