"""GPU tests of the SAM / BAM record selection (include/kmm.h RECORD SELECTION): "bam_include_flags",
"bam_min_mapq" and kmm_set_record_regions on kmm_map_bam and KMM_FORMAT_SAM.  For every case of tests/select_cases.py the node
counts equal the oracle's (oracle.map_reads) over the SEQs the catalogue's own keep() keeps, bit for bit, and *n_records and the
excluded counters match — as a BAM file, as SAM text with LF and with CRLF line ends, as BGZF SAM and as plain-gzip SAM; with records carried between calls,
with "original_strand" and "use_record_qual", over two shares of one BAM file; the rules hold across streams until cleared; the
refusals map nothing."""
import gzip

import numpy as np
import pytest

from tests import quality_cases as qc
from tests import select_cases as sc

pytestmark = pytest.mark.gpu

SAM, FASTQ = 8, 4
K = 31
COUNTERS = ("bam_records", "bam_records_excluded", "sam_records", "sam_records_excluded", "records_reversed", "records_without_qual")


@pytest.fixture(scope="module")
def base(oracle):
    """One small index, its genome as ASCII and one handle: shared by the tests of this module."""
    from kmer_mapper_amd import _lib, synthetic as syn
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    index, genome = syn.make_index(5000, seed=911)
    mx = index.max_node_id()
    dev = engine.DeviceIndex.from_index(index, mx)
    yield dict(index=index, mx=mx, genome=np.frombuffer(b"ACGT", np.uint8)[genome].tobytes(), dev=dev, oracle=oracle)
    dev.close()


@pytest.fixture(scope="module")
def cases(base):
    """The catalogue with SEQs from the genome, each case with its files; built once."""
    from kmer_mapper_amd import reads_io
    made = {}

    def get(name):
        if name not in made:
            names = None
            if name == "sam_seams":
                case, names = sc.sam_seams()
            else:
                case = sc.CASES[name]()
            case = sc.with_genome(case, base["genome"])
            text = sc.sam_bytes(case.records, case.refs, names=names)
            made[name] = (case, dict(
                bam=np.frombuffer(reads_io.bgzf_members(sc.bam_payload(case.records, case.refs), 0x1000) + reads_io.BGZF_EOF, np.uint8),
                sam=np.frombuffer(text, np.uint8),
                crlf=np.frombuffer(sc.sam_bytes(case.records, case.refs, crlf=True, names=names), np.uint8),
                bgzf=np.frombuffer(reads_io.bgzf_members(text, 0x1000) + reads_io.BGZF_EOF, np.uint8),
                gzip=np.frombuffer(gzip.compress(text, 6), np.uint8)))
        return made[name]
    return get


def _flat(reads):
    offsets = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    return np.frombuffer(b"".join(reads), np.uint8), offsets


def _expect(base, records, sel, orig=False, q=0):
    """(counts, lookups, masked bases) of the oracle over the records keep() keeps, flipped / masked by the restatements the
    original-strand and record-quality tests use."""
    kept = [sc.shown(r, orig) for r in records if sc.keep(r, sel)]
    bases, offsets = _flat([s for s, _ in kept])
    n_masked = 0
    if q:
        quals = np.frombuffer(b"".join(b"~" * len(s) if ql is None else ql for s, ql in kept), np.uint8)
        mask = qc.low_mask(quals, q)
        n_masked = int(mask.sum())
        bases, offsets = qc.split_at_mask(bases, offsets, mask)
    counts, n = base["oracle"].map_reads(base["index"], base["mx"], bases, offsets, K)
    return counts, n, n_masked


def _regions(sel, refs):
    return [(bytes(refs[ref][0]), ref, beg, end) for ref, beg, end in (sel.regions or [])]


def _set(dev, sel, refs):
    dev.set_param("bam_exclude_flags", sel.excl)
    dev.set_param("bam_include_flags", sel.incl)
    dev.set_param("bam_min_mapq", sel.min_mapq)
    dev.set_record_regions(_regions(sel, refs), sel.keep_unplaced)


def _clear(dev):
    _set(dev, sc.NO_SEL, ())
    for name in ("original_strand", "use_record_qual", "min_base_quality", "debug_records_piece_kb", "debug_bgzf_call_cap_kb", "path"):
        dev.set_param(name, 0)


def _stream(dev, entry, comp, **kw):
    """A compressed stream mapped to its end, call by call: (bytes used, records, calls that left a carry)"""
    pos = n = carried = 0
    while pos < len(comp):
        used, n_rec = entry(comp[pos:], first=pos == 0, last=True, **kw)
        assert used > 0
        pos, n = pos + used, n + n_rec
        carried += dev.get_param("bgzf_carry_bytes") > 0
    return pos, n, carried


def _routes(dev, files):
    return (("bam", "bam", lambda: _stream(dev, dev.map_bam, files["bam"], k=K)[:2], len(files["bam"])),
            ("sam", "sam", lambda: dev.map_records(files["sam"], fmt=SAM, k=K), len(files["sam"])),
            ("sam, crlf", "sam", lambda: dev.map_records(files["crlf"], fmt=SAM, k=K), len(files["crlf"])),
            ("sam, bgzf", "sam", lambda: _stream(dev, dev.map_bgzf, files["bgzf"], fmt=SAM, k=K)[:2], len(files["bgzf"])),
            ("sam, gzip", "sam", lambda: _stream(dev, dev.map_gzip, files["gzip"], fmt=SAM, k=K)[:2], len(files["gzip"])))


def _run(dev, call):
    """(counts, lookups, what the call returned, the counters' growth) on cleared counts"""
    dev.reset()
    dev.get_stats(reset=True)
    before = {c: dev.get_param(c) for c in COUNTERS}
    ret = call()
    counts = dev.get_node_counts().copy()
    return counts, dev.get_stats()[0], ret, {c: dev.get_param(c) - before[c] for c in COUNTERS}


def _check_routes(base, case, files, sel, routes=None, orig=False, q=0):
    dev = base["dev"]
    want = _expect(base, case.records, sel, orig, q)
    kept, excluded, flipped, no_qual = sc.counts(case.records, sel, orig)
    for what, kind, call, n_bytes in _routes(dev, files):
        if routes and what not in routes:
            continue
        counts, lookups, ret, grown = _run(dev, call)
        assert np.array_equal(counts, want[0]) and lookups == want[1], (what, sel[:3])
        assert ret == (n_bytes, kept), (what, ret, kept)
        assert (grown[kind + "_records"], grown[kind + "_records_excluded"]) == (kept, excluded), (what, grown)
        assert grown["records_reversed"] == flipped and grown["records_without_qual"] == (no_qual if q else 0), (what, grown)
        if q:
            assert dev.get_param("quality_masked_bases") == want[2], what
    return want


# ---------------------------------------------------------------------------------------------- the parameters
def test_the_parameters(base):
    dev = base["dev"]
    for name, top in (("bam_include_flags", 0xFFFF), ("bam_min_mapq", 255)):
        assert dev.get_param(name) == 0
        for bad in (-1, top + 1):
            with pytest.raises(ValueError, match=name + " outside"):
                dev.set_param(name, bad)
        dev.set_param(name, top)
        assert dev.get_param(name) == top
        dev.set_param(name, 0)
    assert dev.get_param("record_regions") == 0
    dev.set_record_regions([("chr1", 0, 10, 20), ("chr1", 0, 20, 30), ("chr1", 0, 5, 12), ("chr2", 1, 0, 5), ("chr1", 0, 40, 50)])
    assert dev.get_param("record_regions") == 3                             # [5, 30) and [40, 50) on chr1, [0, 5) on chr2
    dev.set_record_regions([])
    assert dev.get_param("record_regions") == 0
    with pytest.raises(ValueError, match="record_regions|unknown"):
        dev.set_param("record_regions", 1)                                  # read-only


# ---------------------------------------------------------------------------------------------- the catalogue, four routes
@pytest.mark.parametrize("name", list(sc.CASES) + ["sam_seams"])
def test_every_case_on_every_route(base, cases, name):
    case, files = cases(name)
    dev = base["dev"]
    try:
        _set(dev, case.sel, case.refs)
        want = _check_routes(base, case, files, case.sel, routes=("sam", "sam, crlf", "sam, bgzf", "sam, gzip") if name == "sam_seams" else None)
        _clear(dev)
        dev.set_param("bam_exclude_flags", case.sel.excl)
        plain = _check_routes(base, case, files, sc.NO_SEL._replace(excl=case.sel.excl), routes=("bam", "sam") if name != "sam_seams" else ("sam",))
        assert not np.array_equal(want[0], plain[0])                        # (the selection shows in the counts)
    finally:
        _clear(dev)


def test_each_rule_alone_on_the_mixed_case(base, cases):
    case, files = cases("mixed")
    dev = base["dev"]
    try:
        for _, sel in sc.alone(case.sel):
            _set(dev, sel, case.refs)
            _check_routes(base, case, files, sel, routes=("bam", "sam"))
    finally:
        _clear(dev)


def test_records_carried_between_calls_are_judged_once(base, cases):
    """kmm_map_bam under a call cap of 4 KiB (calls end inside records: the carry is used), SAM text cut into pieces of 4 KiB."""
    case, files = cases("mixed")
    dev = base["dev"]
    want = _expect(base, case.records, case.sel)
    kept, excluded = sc.counts(case.records, case.sel)[:2]
    try:
        _set(dev, case.sel, case.refs)
        dev.set_param("debug_bgzf_call_cap_kb", 4)
        dev.set_param("debug_records_piece_kb", 4)
        counts, lookups, ret, grown = _run(dev, lambda: _stream(dev, dev.map_bam, files["bam"], k=K))
        assert np.array_equal(counts, want[0]) and lookups == want[1]
        assert ret[:2] == (len(files["bam"]), kept) and ret[2] > 3 and (grown["bam_records"], grown["bam_records_excluded"]) == (kept, excluded)
        counts, lookups, ret, grown = _run(dev, lambda: dev.map_records(files["sam"], fmt=SAM, k=K))
        assert np.array_equal(counts, want[0]) and lookups == want[1]
        assert ret == (len(files["sam"]), kept) and (grown["sam_records"], grown["sam_records_excluded"]) == (kept, excluded)
        assert len(files["sam"]) > 20 * 4096
    finally:
        _clear(dev)


@pytest.mark.parametrize("name", ["mixed", "long_records"])
def test_with_original_strand_and_with_record_qualities(base, cases, name):
    """"original_strand" 1: the kept records flipped back; "use_record_qual" 1 with a floor of 20: their QUAL applied; both
    together.  "records_reversed" and "records_without_qual" count kept records only."""
    case, files = cases(name)
    dev = base["dev"]
    sel = case.sel._replace(incl=0) if name == "mixed" else case.sel        # (mixed: FLAG 16 alone has no 0x1; 0x93 has both)
    assert sc.counts(case.records, sel, True)[2] > 0 or name != "mixed"
    try:
        for orig, q in ((1, 0), (0, 20), (1, 20)):
            _set(dev, sel, case.refs)
            dev.set_param("original_strand", orig)
            dev.set_param("use_record_qual", 1 if q else 0)
            dev.set_param("min_base_quality", q)
            _check_routes(base, case, files, sel, routes=("bam", "sam", "sam, bgzf"), orig=bool(orig), q=q)
        all_flips = sc.counts(case.records, sc.NO_SEL, True)[2]
        assert name != "mixed" or all_flips > sc.counts(case.records, sel, True)[2] > 0
    finally:
        _clear(dev)


def test_two_shares_of_one_bam_file_sum_to_the_whole(base, cases):
    from tests.test_gpu_bam_shard import _map_sharded
    case, files = cases("mixed")
    dev = base["dev"]
    want = _expect(base, case.records, case.sel)
    kept, excluded = sc.counts(case.records, case.sel)[:2]
    try:
        _set(dev, case.sel, case.refs)
        dev.reset()
        before = dev.get_param("bam_records_excluded")
        n, shares = _map_sharded(dev, files["bam"].tobytes(), 2, k=K)
        assert n == kept and dev.get_param("bam_records_excluded") - before == excluded
        assert np.array_equal(dev.get_node_counts(), want[0])
        assert shares[1][0:2] > (0, 0)                                      # (the second share starts behind the header)
    finally:
        _clear(dev)


def test_rules_hold_across_streams_until_cleared(base, cases):
    case, files = cases("boundaries")
    dev = base["dev"]
    sel = case.sel
    with_rules, without = _expect(base, case.records, sel), _expect(base, case.records, sc.NO_SEL)
    assert not np.array_equal(with_rules[0], without[0])
    try:
        _set(dev, sel, case.refs)
        for what, _, call, _ in _routes(dev, files)[:4] * 2:                  # every stream inherits the rules
            assert np.array_equal(_run(dev, call)[0], with_rules[0]), what
        _set(dev, sc.NO_SEL, ())                                            # n_regions 0, masks 0
        assert dev.get_param("record_regions") == 0
        for what, kind, call, _ in _routes(dev, files)[:2]:
            counts, _, ret, grown = _run(dev, call)
            assert np.array_equal(counts, without[0]) and ret[1] == len(case.records) and grown[kind + "_records_excluded"] == 0, what
        dev.set_record_regions([], keep_unplaced=True)                      # keep_unplaced without a list has no effect
        assert np.array_equal(_run(dev, _routes(dev, files)[0][2])[0], without[0])
    finally:
        _clear(dev)


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals_map_nothing(base, cases):
    import ctypes
    from kmer_mapper_amd import _lib
    case, files = cases("boundaries")
    dev = base["dev"]
    try:
        dev.reset()
        for bad, msg in (([("chr1", 0, 5, 5)], "end <= beg"), ([("chr1", 0, 9, 3)], "end <= beg"), ([("chr1", 0, -1, 3)], "beg < 0"),
                         ([("chr1", 0, 0, 1)] * 4097, "at most 4096"), ([("r%d" % i, i, 0, 1) for i in range(257)], "at most 256"),
                         ([("*", 0, 0, 1)], "ref_name"), ([(None, -1, 0, 1)], "every region needs"), ([("n" * 256, 0, 0, 1)], "ref_name")):
            with pytest.raises(ValueError, match=msg):
                dev.set_record_regions(bad)
        assert dev.get_param("record_regions") == 0
        dev.set_record_regions([("chr1", 0, 0, 1)] * 4096)                  # the limits themselves are taken
        dev.set_record_regions([("r%d" % i, i, 0, 1) for i in range(256)])
        assert dev.get_param("record_regions") == 256
        # a ref_id beyond the stream's n_ref (3): from the map call, nothing mapped; the C ABI gives KMM_ERR_INVALID_ARG
        dev.set_record_regions([("chr1", 0, 0, 10), ("chrX", 3, 0, 10)])
        with pytest.raises(ValueError, match="ref_id 3, the stream has 3 references"):
            dev.map_bam(files["bam"], first=True, last=True, k=K)
        used, n_rec = ctypes.c_int64(0), ctypes.c_int64(0)
        rc = _lib.lib().kmm_map_bam(dev._h, files["bam"].ctypes.data_as(ctypes.c_void_p), len(files["bam"]),
                                    _lib.FORMAT_NEW_STREAM | _lib.FORMAT_LAST_CHUNK, K, 1000, 0, None, ctypes.byref(used), ctypes.byref(n_rec))
        assert rc == _lib.KMM_ERR_INVALID_ARG and n_rec.value == 0
        dev.set_record_regions([(None, 0, 0, 10)])                          # ids alone serve BAM, not SAM
        with pytest.raises(ValueError, match="without ref_name"):
            dev.map_records(files["sam"], fmt=SAM, k=K)
        dev.set_record_regions([("chr1", None, 0, 10)])                     # names alone serve SAM, not BAM
        with pytest.raises(ValueError, match="without ref_id"):
            dev.map_bam(files["bam"], first=True, last=True, k=K)
        assert dev.map_records(files["sam"], fmt=SAM, k=K)[0] == len(files["sam"])
        dev.reset()
        assert not dev.get_node_counts().any()
        # each malformed SAM field: the byte offset in the message, nothing mapped; accepted while its rule is off
        for field, value, _, rule in sc.MALFORMED:
            data, at = sc.malformed_sam(field, value, genome=base["genome"])
            text = np.frombuffer(data, np.uint8)
            _set(dev, sc.MALFORMED_SEL[rule], sc.REFS3)
            with pytest.raises(ValueError, match="SAM line at byte %d of the chunk: %s" % (at, {"mapq": "MAPQ", "pos": "POS", "cigar": "CIGAR"}[field])):
                dev.map_records(text, fmt=SAM, k=K)
            assert not dev.get_node_counts().any(), (field, value)
            _set(dev, sc.NO_SEL._replace(incl=1), ())
            assert dev.map_records(text, fmt=SAM, k=K) == (len(text), 45), (field, value)
            assert dev.get_node_counts().any()
            dev.reset()
    finally:
        _clear(dev)


def test_a_selection_does_not_touch_fastq(base, cases):
    case, _ = cases("boundaries")
    dev = base["dev"]
    reads = [r.seq for r in case.records]
    fq = np.frombuffer(b"".join(b"@r\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in reads), np.uint8)
    bases, offsets = _flat(reads)
    want = base["oracle"].map_reads(base["index"], base["mx"], bases, offsets, K)[0]
    try:
        _set(dev, sc.Sel(0xFFFF, 0xFFFF, 255, [(0, 0, 1)], False), case.refs)
        counts, _, ret, _ = _run(dev, lambda: dev.map_records(fq, fmt=FASTQ, k=K))
        assert np.array_equal(counts, want) and ret == (len(fq), len(reads))
    finally:
        _clear(dev)


# ---------------------------------------------------------------------------------------------- the command line
def test_cli_end_to_end(base, cases, tmp_path, caplog):
    """`kmer_mapper map` on a small BAM and a small SAM with --regions, --regions-file, --min-mapq, --include-flags and
    --exclude-flags: the .npy holds the oracle's counts over the records keep() keeps; one line names the rules, one the totals."""
    import logging
    from kmer_mapper_amd import command_line_interface as cli
    case, files = cases("boundaries")
    sel = case.sel
    idx = str(tmp_path / "idx.npz")
    base["index"].to_file(idx)
    bam, sam, bed = str(tmp_path / "r.bam"), str(tmp_path / "r.sam"), str(tmp_path / "r.bed")
    files["bam"].tofile(bam)
    files["sam"].tofile(sam)
    name = lambda ref: case.refs[ref][0].decode()
    on_chr1 = ",".join("%s:%s-%s" % (name(ref), format(beg + 1, ","), format(end, ",")) for ref, beg, end in sel.regions if ref == 0)
    with open(bed, "w") as f:
        f.write("# the chr2 regions\ntrack name=t\n" + "".join("%s\t%d\t%d\n" % (name(ref), beg, end) for ref, beg, end in sel.regions if ref != 0))
    want = _expect(base, case.records, sel)[0]
    kept, excluded = sc.counts(case.records, sel)[:2]
    for path in (bam, sam):
        out = str(tmp_path / "out")
        caplog.clear()
        with caplog.at_level(logging.INFO):
            cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out, "--regions", on_chr1, "--regions", "*", "--regions-file", bed,
                                     "--min-mapq", str(sel.min_mapq), "--include-flags", hex(sel.incl), "--exclude-flags", hex(sel.excl)])
        assert np.array_equal(np.load(out + ".npy"), want), path
        assert "Records are selected on the GPU: exclude flags 0x400, include flags 0x1, MAPQ >= 30, 5 region(s) (3 after merging)" in caplog.text
        assert "Record selection: %d records kept and mapped, %d excluded" % (kept, excluded) in caplog.text
        caplog.clear()
        with caplog.at_level(logging.INFO):
            cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out])
        assert not np.array_equal(np.load(out + ".npy"), want) and "selected" not in caplog.text and "selection" not in caplog.text
    with pytest.raises(ValueError, match="no reference named 'chr9'"):
        cli.run_argument_parser(["map", "-i", idx, "-f", bam, "-o", str(tmp_path / "out"), "--regions", "chr9:1-5"])
