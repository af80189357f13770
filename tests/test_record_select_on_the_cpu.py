"""CPU tier of the SAM / BAM record selection (include/kmm.h RECORD SELECTION): the walk and decode of
csrc/kmm_bam.hpp and the count and write passes of csrc/kmm_sam.hpp under a selection, compiled by themselves with g++
(tests/select_cpu_driver.hpp) and driven in windows with a carry.  What they write and count has to be what the catalogue's own
keep() (tests/select_cases.py) says, byte for byte, for the two-line FASTA, quality and original-strand variants, with 1 and 64
lanes; once more under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone executable.  Also: the interval merge
against brute force, util.parse_regions / read_bed_regions, reads_io.bam_references, and the command line up to its first HIP
call."""
import ctypes
import itertools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import select_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
VARIANTS = list(itertools.product((0, 1), (0, 1), (1, 64)))      # (quality variant, original strand, lanes)
U64, I64, U32 = ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("select")
    src = tmp / "shim.cpp"
    src.write_text('#include "select_cpu_driver.hpp"\n')
    so = str(tmp / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    common = [ctypes.c_char_p, U64, ctypes.c_void_p, ctypes.c_int, U32, ctypes.c_int, ctypes.c_int, U32, ctypes.c_void_p, U64,
              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.select_bam_cpu.argtypes = common
    lib.select_sam_cpu.argtypes = common + [ctypes.c_char_p, ctypes.c_void_p, U32]
    lib.select_merge.argtypes, lib.select_merge.restype = [ctypes.c_void_p, U64], U64
    lib.select_overlaps.argtypes = [ctypes.c_void_p, U64, I64, I64, I64]
    return lib


def _tables(sel, refs):
    """ctypes forms of sc.tables: (rules for BAM, iv for BAM, rules for SAM, iv for SAM, names blob, offsets, n names)"""
    by_id, names, by_name = sc.tables(sel, refs)

    def pack(iv):
        return (U64 * 4)(sel.incl, sel.min_mapq, int(sel.keep_unplaced), len(iv)), (I64 * (3 * len(iv) + 1))(*[x for t in iv for x in t])
    offs = [0]
    for nm in names:
        offs.append(offs[-1] + len(nm))
    return pack(by_id) + pack(by_name) + (b"".join(names), (U32 * len(offs))(*offs), len(names))


def _run(lib, kind, data, sel, refs, cuts=(), qual=0, orig=0, lanes=1):
    """(rc, text, records, excluded, without qualities, flipped, error position, error code)"""
    cuts = sorted(set([c for c in cuts if 0 < c < len(data)] + [len(data)]))
    out = np.zeros(3 * len(data) + 64, np.uint8)
    on, st = U64(0), (U64 * 7)()
    c = (U64 * len(cuts))(*cuts)
    rb, ib, rs, is_, blob, offs, n_names = _tables(sel, refs)
    if kind == "bam":
        rc = lib.select_bam_cpu(data, len(data), c, len(cuts), sel.excl, qual, orig, lanes, out.ctypes.data, len(out), ctypes.byref(on), st, rb, ib)
    else:
        rc = lib.select_sam_cpu(data, len(data), c, len(cuts), sel.excl, qual, orig, lanes, out.ctypes.data, len(out), ctypes.byref(on), st,
                                rs, is_, blob, offs, n_names)
    return rc, out[:on.value].tobytes(), st[0], st[1], st[3], st[4], st[5], st[6]


def _check(lib, case, cuts_bam=((),), cuts_sam=((),), variants=VARIANTS, crlf=False, names=None, selections=None):
    """Every variant on the case as BAM and as SAM, under the case's selection, each rule alone, and none."""
    bam, sam = sc.bam_payload(case.records, case.refs), sc.sam_bytes(case.records, case.refs, crlf=crlf, names=names)
    for sel in selections or ([case.sel, sc.NO_SEL._replace(excl=case.sel.excl)] + [s for _, s in sc.alone(case.sel)]):
        for qual, orig, lanes in variants:
            kept, excluded, flipped, no_qual = sc.counts(case.records, sel, orig)
            for kind, data, all_cuts in (("bam", bam, cuts_bam), ("sam", sam, cuts_sam)):
                want = sc.text(case.records, sel, qual, orig, upper=kind == "bam")
                for cuts in all_cuts:
                    rc, out, recs, excl, nq, flips = _run(lib, kind, data, sel, case.refs, cuts, qual, orig, lanes)[:6]
                    assert rc == 0, (kind, rc, sel[:3])
                    assert out == want, (kind, qual, orig, lanes, cuts[:4], sel[:3])
                    assert (recs, excl, flips) == (kept, excluded, flipped), (kind, qual, orig, lanes, sel[:3])
                    assert nq == (no_qual if qual else 0), (kind, qual, nq, no_qual)
    return bam, sam


# ---------------------------------------------------------------------------------------------- the catalogue itself
@pytest.mark.parametrize("name", list(sc.CASES) + ["sam_seams"])
def test_no_case_is_vacuous(name):
    """Each rule alone removes and keeps at least one record; the combined selection keeps 5 % .. 95 %."""
    case = sc.sam_seams()[0] if name == "sam_seams" else sc.CASES[name]()
    sc.check_not_vacuous(case)


def test_keep_on_hand_written_records():
    R = sc.Rec
    sel = sc.Sel(0x400, 0x2, 30, [(0, 100, 200)], True)
    assert sc.keep(R(0x2, 0, 150, 30, [(10, "M")], b"A", None), sel)
    assert not sc.keep(R(0x402, 0, 150, 30, [(10, "M")], b"A", None), sel)
    assert not sc.keep(R(0x1, 0, 150, 30, [(10, "M")], b"A", None), sel)
    assert not sc.keep(R(0x2, 0, 150, 29, [(10, "M")], b"A", None), sel)
    assert sc.keep(R(0x2, 0, 90, 255, [(5, "M"), (6, "D")], b"A", None), sel) and not sc.keep(R(0x2, 0, 90, 255, [(5, "M"), (5, "D")], b"A", None), sel)
    assert not sc.keep(R(0x2, 0, 90, 255, [(5, "M"), (60, "I"), (60, "S")], b"A", None), sel)
    assert sc.keep(R(0x2, -1, -1, 255, None, b"A", None), sel) and not sc.keep(R(0x2, -1, -1, 255, None, b"A", None), sel._replace(keep_unplaced=False))
    assert not sc.keep(R(0x2, 1, 150, 255, [(10, "M")], b"A", None), sel) and not sc.keep(R(0x2, 0, 200, 255, [(10, "M")], b"A", None), sel)
    assert sc.keep(R(0x6, 0, 199, 255, [(10, "M")], b"A", None), sel) and not sc.keep(R(0x6, 0, 99, 255, [(10, "M")], b"A", None), sel)


# ---------------------------------------------------------------------------------------------- byte-exact text
def test_the_mixed_case_in_awkward_windows(lib):
    case = sc.mixed()
    bam = sc.bam_payload(case.records, case.refs)
    _check(lib, case, cuts_bam=((), tuple(range(777, len(bam), 16384 + 333))), cuts_sam=((), tuple(range(1000, 900_000, 50_001))),
           variants=[(0, 0, 1), (1, 1, 64), (0, 1, 64), (1, 0, 1)])
    assert len(bam) > 20 * 16384


def test_every_region_boundary(lib):
    case = sc.boundaries()
    want = [0, 1, 1, 0, 1, 1, 0, 0, 0, 0, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0]
    assert [int(sc.keep(r, case.sel)) for r in case.records] == want          # (the catalogue's comments, checked)
    _check(lib, case, cuts_bam=((), (100, 900, 901)), cuts_sam=((), (300, 1500)))
    _check(lib, case, crlf=True, variants=[(0, 0, 64), (1, 1, 1)])


def test_cigars_of_63_64_65_128_and_5000_operations(lib):
    case = sc.long_cigars()
    assert [int(sc.keep(r, case.sel)) for r in case.records] == [1, 0] * 10 + [0, 0]
    _check(lib, case, cuts_bam=((), (5_000, 30_000)), cuts_sam=((), (3_000, 20_000)))


@pytest.mark.parametrize("name", ["long_records", "straddling_cigar"])
def test_records_longer_than_a_tile(lib, name):
    case = sc.CASES[name]()
    bam, _ = _check(lib, case, cuts_bam=((), tuple(range(10_000, 250_000, 10_000))), cuts_sam=((), tuple(range(9_999, 300_000, 20_000))),
                    variants=[(0, 0, 64), (1, 1, 1), (1, 0, 64)])
    assert len(bam) > 8 * 16384


def test_sam_names_are_compared_exactly_and_whole(lib):
    case = sc.sam_names()
    assert sc.counts(case.records, case.sel)[0] == 6
    _check(lib, case, crlf=False)
    _check(lib, case, crlf=True, variants=[(1, 0, 64)])


def test_sam_pos_and_mapq_extremes(lib):
    case = sc.sam_extremes()
    assert [int(sc.keep(r, case.sel)) for r in case.records] == [1, 1, 0, 0, 0, 0, 0]
    _check(lib, case)
    _check(lib, case, crlf=True, variants=[(0, 1, 1)])


def test_sam_fields_across_block_and_window_edges(lib):
    """TABs 3 to 6 and the digits of POS and MAPQ on every place of a 16-byte block and on both sides of the 1 KiB window edge
    (asserted on the text itself, with the chunk 16-byte aligned, which a heap buffer of this size is), CIGAR texts over 1 KiB."""
    case, names = sc.sam_seams()
    sam = sc.sam_bytes(case.records, case.refs, names=names)
    seen_block, seen_win = {k: set() for k in range(3, 7)}, {k: set() for k in range(3, 7)}
    for s in sc.sam_line_starts(sam):
        line = sam[s:sam.index(b"\n", s)]
        if line.startswith(b"@"):
            continue
        tabs = [s + i for i, c in enumerate(line) if c == 9]
        for k in range(3, 7):
            seen_block[k].add(tabs[k - 1] % 16)
            seen_win[k].add((tabs[k - 1] - (s - s % 16)) % 1024)
    for k in range(3, 7):
        assert seen_block[k] == set(range(16)), k
        assert {1021, 1022, 1023, 0, 1, 2} <= seen_win[k], k
    assert max(len(b"".join(b"%d%s" % (n, o.encode()) for n, o in r.cigar)) for r in case.records) > 1024
    _check(lib, case, names=names, cuts_sam=((), tuple(range(500, len(sam), 1531))), variants=[(0, 0, 1), (1, 1, 64)])
    _check(lib, case, names=names, crlf=True, variants=[(0, 0, 64)])


@pytest.mark.parametrize("field,value,code,rule", sc.MALFORMED)
def test_a_malformed_field_fails_the_call_only_while_its_rule_reads_it(lib, field, value, code, rule):
    data, at = sc.malformed_sam(field, value)
    for qual, lanes, cuts in ((0, 1, ()), (1, 64, (1000, 2500))):
        rc, _, _, _, _, _, pos, got = _run(lib, "sam", data, sc.MALFORMED_SEL[rule], sc.REFS3, cuts, qual=qual, lanes=lanes)
        assert (rc, pos, got) == (-3, at, code), (field, value)
    other = sc.MALFORMED_SEL["mapq" if rule == "regions" else "regions"]
    if field == "mapq":
        other = other._replace(regions=[(1, 0, 10)])          # (regions that name another reference: POS and CIGAR are not read either)
    for sel in (sc.NO_SEL, sc.NO_SEL._replace(incl=1), other if field != "mapq" else sc.NO_SEL._replace(regions=[(0, 0, 1000)])):
        rc, out, recs, excl = _run(lib, "sam", data, sel, sc.REFS3)[:4]
        assert rc == 0 and recs + excl == 45, (field, value, sel)
    # a record that an earlier rule drops is not looked at further: the same line with FLAG 0 under an include mask
    f = data[at:].split(b"\t")
    f[1] = b"0"
    rc, _, recs, excl = _run(lib, "sam", data[:at] + b"\t".join(f), sc.MALFORMED_SEL[rule]._replace(incl=1), sc.REFS3)[:4]
    assert (rc, recs, excl) == (0, 44, 1)


def test_leading_zeros_are_numbers(lib):
    data, _ = sc.malformed_sam("cigar", b"0005M0000000000001D")
    data2, _ = sc.malformed_sam("mapq", b"0060")
    data3, _ = sc.malformed_sam("pos", b"000141")
    sel = sc.Sel(0, 0, 60, [(0, 0, 1000)], False)
    for d in (data, data2, data3):
        rc, _, recs, excl = _run(lib, "sam", d, sel, sc.REFS3)[:4]
        assert (rc, recs, excl) == (0, 45, 0)


# ---------------------------------------------------------------------------------------------- under the sanitizers
def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/select_san_main.cpp; host code, nothing sanitized is loaded into
    Python): inputs, tables and every call's output live in heap buffers of exactly their size."""
    exe = str(tmp_path / "select_san")
    src = os.path.join(ROOT, "tests", "select_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    inp, outp, tbp = tmp_path / "in.bin", tmp_path / "out.bin", tmp_path / "tables.bin"
    seams, seam_names = sc.sam_seams()
    runs = [(sc.mixed(n=600), None, [(0, 0, 1), (1, 1, 64)]), (sc.boundaries(), None, [(0, 1, 64)]), (sc.long_cigars(), None, [(0, 0, 64), (1, 0, 1)]),
            (sc.straddling_cigar(), None, [(1, 1, 64)]), (sc.sam_names(), None, [(0, 0, 1)]), (seams, seam_names, [(1, 0, 64)])]
    for case, names, variants in runs:
        by_id, table_names, by_name = sc.tables(case.sel, case.refs)
        for kind, data, iv, upper in (("bam", sc.bam_payload(case.records, case.refs), by_id, True),
                                      ("sam", sc.sam_bytes(case.records, case.refs, crlf=True, names=names), by_name, False)):
            if names is not None and kind == "bam":
                continue
            inp.write_bytes(data)
            offs = [0]
            for nm in table_names:
                offs.append(offs[-1] + len(nm))
            tbp.write_bytes(struct.pack("<4Q", case.sel.incl, case.sel.min_mapq, int(case.sel.keep_unplaced), len(iv)) +
                            b"".join(struct.pack("<3q", *t) for t in iv) + struct.pack("<I", len(table_names)) +
                            struct.pack("<%dI" % len(offs), *offs) + b"".join(table_names))
            for (qual, orig, lanes), cuts in itertools.product(variants, ([], [str(c) for c in range(7, len(data), 45_677)])):
                r = subprocess.run([exe, kind, str(inp), str(outp), str(tbp), hex(case.sel.excl), str(qual), str(orig), str(lanes), *cuts],
                                   capture_output=True, text=True, timeout=300)
                assert r.returncode == 0, r.stderr[-2000:]
                assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
                kept, excluded, flipped, _ = sc.counts(case.records, case.sel, orig)
                got = r.stdout.split()
                assert got[:3] == ["0", str(kept), str(excluded)] and int(got[4]) == flipped, r.stdout
                assert outp.read_bytes() == sc.text(case.records, case.sel, qual, orig, upper), (kind, qual, orig, lanes, cuts[:3])


# ---------------------------------------------------------------------------------------------- the interval list
def test_sort_and_merge_against_brute_force(lib):
    rng = np.random.default_rng(21)
    for trial in range(60):
        n = int(rng.integers(1, 40))
        iv = [(int(rng.integers(0, 4)), b, b + int(rng.integers(1, 30))) for b in rng.integers(0, 200, size=n)]
        if trial % 5 == 0:
            iv += [(r, e, e + 3) for r, _, e in iv[:5]]                                # abutting intervals
        arr = (I64 * (3 * len(iv)))(*[x for t in iv for x in t])
        m = lib.select_merge(arr, len(iv))
        merged = [tuple(arr[3 * i:3 * i + 3]) for i in range(m)]
        assert merged == sorted(merged)
        for a, b in zip(merged, merged[1:]):
            assert a[0] < b[0] or a[2] < b[1], (a, b)                                  # disjoint and not abutting
        for ref in range(-1, 5):
            covered = {p for r, b, e in iv if r == ref for p in range(b, e)}
            assert covered == {p for r, b, e in merged if r == ref for p in range(b, e)}
            for rb in range(-2, 240, 3):
                for ln in (1, 2, 7, 40):
                    brute = any(r == ref and b < rb + ln and rb < e for r, b, e in iv)
                    assert bool(lib.select_overlaps(arr, m, ref, rb, rb + ln)) == brute, (ref, rb, ln)
    assert lib.select_overlaps(arr, 0, 0, 0, 10) == 0


# ---------------------------------------------------------------------------------------------- regions as text
def test_parse_regions():
    from kmer_mapper_amd.util import REGION_END_MAX as E, parse_regions
    refs = [("chr6", 171_000_000), (b"chr1", 1000), ("HLA:A", 50), ("chr1:5", 9), ("chr1:5-6", 9)]
    assert parse_regions("chr6:28,000,000-34,000,000", refs) == ([("chr6", 0, 27_999_999, 34_000_000)], False)
    assert parse_regions("chr6:5,chr6:5-,chr6,*", refs) == ([("chr6", 0, 4, E), ("chr6", 0, 4, E), ("chr6", 0, 0, E)], True)
    assert parse_regions(["chr1:1-1", "chr1:1,000"], refs) == ([("chr1", 1, 0, 1), ("chr1", 1, 999, E)], False)
    assert parse_regions("chr6:1,000-2,000,chr1:7-9", refs) == ([("chr6", 0, 999, 2000), ("chr1", 1, 6, 9)], False)
    # a name that contains ':' — the whole string is tried as a name first, as htslib does
    assert parse_regions(["HLA:A", "HLA:A:3-7", "chr1:5", "chr1:5-6", "chr1:5:2-3"], refs)[0] == [
        ("HLA:A", 2, 0, E), ("HLA:A", 2, 2, 7), ("chr1:5", 3, 0, E), ("chr1:5-6", 4, 0, E), ("chr1:5", 3, 1, 3)]
    # without references (SAM): names as they stand, ids -1
    assert parse_regions("chrX:10-20,weird:name,*") == ([("chrX", -1, 9, 20), ("weird:name", -1, 0, E)], True)
    assert parse_regions(b"chr1") == ([("chr1", -1, 0, E)], False)
    for bad, msg in (("chr7", "no reference named 'chr7'"), ("chr7:1-5", "no reference named 'chr7'"), ("chr6:9-3", "end lies before"),
                     ("chr6,,chr1", "empty region"), ("", "empty region"), ("chr6:a-b", "no reference named 'chr6:a-b'")):
        with pytest.raises(ValueError, match=msg):
            parse_regions(bad, refs)
    with pytest.raises(ValueError, match="end lies before"):
        parse_regions("c:9-3")


def test_read_bed_regions(tmp_path):
    from kmer_mapper_amd.util import read_bed_regions
    bed = tmp_path / "r.bed"
    bed.write_text("# a comment\ntrack name=x\nbrowser position chr1:1-2\nchr1\t0\t10\tname\t0\t+\n\nchr2\t5\t6\nchr1 7 9\n")
    assert read_bed_regions(str(bed)) == [("chr1", -1, 0, 10), ("chr2", -1, 5, 6), ("chr1", -1, 7, 9)]
    assert read_bed_regions(str(bed), [("chr2", 9), ("chr1", 99)]) == [("chr1", 1, 0, 10), ("chr2", 0, 5, 6), ("chr1", 1, 7, 9)]
    with pytest.raises(ValueError, match="no reference named 'chr2'"):
        read_bed_regions(str(bed), [("chr1", 99)])
    for text, msg in (("chr1\t5\n", "three columns"), ("chr1\tx\t9\n", "three columns"), ("chr1\t9\t9\n", "at or before the start")):
        with pytest.raises(ValueError, match=msg):
            read_bed_regions([text])


def test_bam_references_on_a_header_that_spans_several_members(tmp_path):
    from kmer_mapper_amd import reads_io
    refs = [(b"chr%d" % i + b"_a_long_name" * (i % 4), 1000 + i) for i in range(300)]
    want = [(n.decode(), ln) for n, ln in refs]
    head = reads_io.bam_header(refs, b"@HD\tVN:1.6\n" + b"@CO\tpadding\n" * 500)
    data = reads_io.bgzf_members(head + reads_io.bam_record(b"ACGT"), block=700) + reads_io.BGZF_EOF
    assert len(head) > 10 * 700
    assert reads_io.bam_references(data) == want
    path = tmp_path / "r.bam"
    path.write_bytes(data)
    assert reads_io.bam_references(str(path)) == want
    assert reads_io.bam_references(reads_io.bgzf_members(reads_io.bam_header()) + reads_io.BGZF_EOF) == []
    with pytest.raises(ValueError, match="ends inside its header"):
        reads_io.bam_references(reads_io.bgzf_members(head, block=700)[:3000].rsplit(b"\x1f\x8b\x08\x04", 1)[0])
    with pytest.raises(ValueError, match="not a BAM file"):
        reads_io.bam_references(reads_io.bgzf_members(b"@HD\tVN:1.6\nr\t4\t*\t0\t0\t*\t*\t0\t0\tA\tI\n"))
    with pytest.raises(ValueError, match="not a BAM file"):
        reads_io.bam_references(b"plain text, no BGZF member" * 3)


# ---------------------------------------------------------------------------------------------- the command line
def test_check_record_select():
    from kmer_mapper_amd import command_line_interface as cli
    for fmt in ("fastq", "fasta", "fasta_ml", "bam", "sam"):
        assert cli.check_record_select(fmt) is None and cli.check_record_select(fmt, 0, 0, [], None) is None
    assert cli.check_record_select("bam", 2, 30, ["chr1"], "x.bed") == dict(include_flags=2, min_mapq=30, regions=["chr1"], regions_file="x.bed")
    for fmt in ("fastq", "fasta", "fasta_ml"):
        for kw, flag in ((dict(include_flags=2), "--include-flags"), (dict(min_mapq=1), "--min-mapq"), (dict(regions=["c"]), "--regions"),
                         (dict(regions_file="x.bed"), "--regions-file")):
            with pytest.raises(ValueError, match="%s applies to SAM and BAM input only" % flag):
                cli.check_record_select(fmt, **kw)
    for kw in (dict(regions=["*"]), dict(regions=["*,*", " * "])):
        with pytest.raises(ValueError, match="'\\*' alone selects nothing"):
            cli.check_record_select("bam", **kw)
    assert cli.check_record_select("sam", regions=["*", "chr1"])["regions"] == ["*", "chr1"]
    assert cli.check_record_select("sam", regions=["*"], regions_file="x.bed")["regions"] == ["*"]
    for kw in (dict(include_flags=0x10000), dict(include_flags=-1), dict(min_mapq=256), dict(min_mapq=-1)):
        with pytest.raises(ValueError, match="outside"):
            cli.check_record_select("sam", **kw)


def test_cli_flags_up_to_their_first_hip_call(tmp_path, monkeypatch):
    """The new flags are parsed and reach map_gpu_raw for SAM and BAM; on FASTQ and FASTA they are refused before the index file
    is read; without them map_gpu_raw gets no selection; the regions resolve against the BAM header, by name for SAM."""
    from kmer_mapper_amd import reads_io, synthetic
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.util import REGION_END_MAX, ReadBatch
    parser = cli.build_argument_parser()
    a = parser.parse_args(["map", "-f", "x.bam", "-o", "y", "--include-flags", "0x2", "--min-mapq", "30", "--regions", "chr1:5-9,chr2",
                           "--regions", "*", "--regions-file", "t.bed"])
    assert (a.include_flags, a.min_mapq, a.regions, a.regions_file) == (2, 30, ["chr1:5-9,chr2", "*"], "t.bed")
    a = parser.parse_args(["map", "-f", "x.bam", "-o", "y"])
    assert (a.include_flags, a.min_mapq, a.regions, a.regions_file) == (0, 0, None, None)
    index, _ = synthetic.make_index(200, seed=3)
    b = ReadBatch.from_strings(["ACGT" * 10])
    reads_io.write_sam(str(tmp_path / "r.sam"), b)
    reads_io.write_bam(str(tmp_path / "r.bam"), b, refs=((b"chr1", 500), (b"chr2", 600)))
    reads_io.write_fastq(str(tmp_path / "r.fq"), b)
    reads_io.write_fasta(str(tmp_path / "r.fa"), b)
    (tmp_path / "t.bed").write_text("chr2\t10\t20\n")
    index_reads = []

    def fake_index(a):
        index_reads.append(a.reads)
        return index
    monkeypatch.setattr(cli, "_get_kmer_index_from_args", fake_index)
    seen = {}

    def fake_raw(index, path, chunk_size, fmt, k, *a, **kw):
        seen.clear()
        seen.update(fmt=fmt, **kw)
        return np.zeros(3, np.uint32)
    monkeypatch.setattr(cli, "map_gpu_raw", fake_raw)

    def args(name, *extra):
        return ["map", "-i", "idx.npz", "-f", str(tmp_path / name), "-o", str(tmp_path / "out"), *extra]
    every = ["--include-flags", "3", "--min-mapq", "20", "--regions", "chr1:5-9,*", "--regions-file", str(tmp_path / "t.bed")]
    for name, fmt in (("r.sam", "sam"), ("r.bam", "bam")):
        cli.run_argument_parser(args(name, *every, "--exclude-flags", "0x900", "--original-strand"))
        assert seen["fmt"] == fmt and seen["exclude_flags"] == 0x900 and seen["original_strand"] is True
        assert seen["record_select"] == dict(include_flags=3, min_mapq=20, regions=["chr1:5-9,*"], regions_file=str(tmp_path / "t.bed"))
        ids = (0, 1) if fmt == "bam" else (-1, -1)
        assert cli.resolve_record_regions(str(tmp_path / name), fmt, seen["record_select"]) == (
            [("chr1", ids[0], 4, 9), ("chr2", ids[1], 10, 20)], True)
        cli.run_argument_parser(args(name))
        assert "record_select" not in seen                              # (none of the flags: no new argument, no new call)
    with pytest.raises(ValueError, match="no reference named 'chr3'"):
        cli.resolve_record_regions(str(tmp_path / "r.bam"), "bam", dict(regions=["chr3:1-2"], regions_file=None))
    assert cli.resolve_record_regions(str(tmp_path / "r.sam"), "sam", dict(regions=["chr3"], regions_file=None)) == (
        [("chr3", -1, 0, REGION_END_MAX)], False)
    for name in ("r.fq", "r.fa"):
        for i in range(0, len(every), 2):
            index_reads.clear()
            with pytest.raises(ValueError, match="%s applies to SAM and BAM input only" % every[i]):
                cli.run_argument_parser(args(name, every[i], every[i + 1]))
            assert index_reads == []                                    # refused before the index file is read
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--min-mapq applies to SAM and BAM input only"):
        cli.map_gpu_raw(index, str(tmp_path / "r.fq"), 1 << 20, "fastq", 31, record_select=dict(min_mapq=3))
