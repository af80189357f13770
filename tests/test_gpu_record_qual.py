"""GPU tests of "use_record_qual" (include/kmm.h): with the switch set and a floor Q > 0, kmm_map_bam and
KMM_FORMAT_SAM decode every record's QUAL beside its SEQ and no k-mer over a base below the floor is counted.  The cases are
the FASTQ ones of tests/quality_cases.py written as BAM (raw Phred bytes) and as SAM (Phred+33): the node counts equal the
oracle's on the reads split at their masked bases, kmm_get_stats' lookups the windows that survive, "quality_masked_bases" the
numpy count, and "records_without_qual" the records written with QUAL "*" / 0xFF."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from tests import quality_cases as qc

pytestmark = pytest.mark.gpu

SAM = 8                      # KMM_FORMAT_SAM
CAP_KB = 4                   # "debug_bgzf_call_cap_kb" of the several-calls test: a call takes one 4 KiB member behind its carry


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def lut():
    from kmer_mapper_amd.util import ambiguous_skip_lut
    return ambiguous_skip_lut()


def _sam_quals(quals, offsets, absent=()):
    return [None if i in absent else quals[offsets[i]:offsets[i + 1]].tobytes() for i in range(len(offsets) - 1)]


def _bam_quals(quals, offsets, absent=()):
    return [None if i in absent else (quals[offsets[i]:offsets[i + 1]] - 33).astype(np.uint8).tobytes() for i in range(len(offsets) - 1)]


def _bam_file(bases, quals, offsets, absent=(), flags=None, block=0x1000):
    """(the file, its inflated bytes): members of `block` inflated bytes, so that records straddle members and 16 KiB tiles."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    payload = reads_io.bam_header() + reads_io.bam_records(ReadBatch(bases, offsets), flags=flags, quals=_bam_quals(quals, offsets, absent))
    return np.frombuffer(reads_io.bgzf_members(payload, block) + reads_io.BGZF_EOF, np.uint8), payload


def _sam_bytes(bases, quals, offsets, absent=(), flags=None):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    return reads_io.sam_text(ReadBatch(bases, offsets), flags=flags, quals=_sam_quals(quals, offsets, absent))


def _answers(oracle, index, mx, bases, offsets, k, mask):
    sb, so = qc.split_at_mask(bases, offsets, mask)
    fwd, n = oracle.map_reads(index, mx, sb, so, k)
    rc, _ = oracle.map_reads(index, mx, sb, so, k, also_revcomp=True)
    fwd.setflags(write=False)
    rc.setflags(write=False)
    return fwd, rc, n


_EXPECT = {}


@pytest.fixture(scope="module")
def expect(oracle):
    """name -> the case, its BAM file and SAM text, its index and the oracle's answers (computed once, never changed)."""
    def get(name):
        if name not in _EXPECT:
            c = dict(qc.build(name))
            assert c["quals"].min() >= 33 and c["quals"].max() <= 126
            index = qc.index_for(c["k"])
            mx = index.max_node_id()
            c["split"], c["split_rc"], c["n_windows"] = _answers(oracle, index, mx, c["bases"], c["offsets"], c["k"], qc.dead_mask(c))
            c["unsplit"], _, c["n_all"] = _answers(oracle, index, mx, c["bases"], c["offsets"], c["k"], qc.dead_mask(c, q=0))
            c["n_masked"] = int(qc.low_mask(c["quals"], c["q"]).sum())
            bam, payload = _bam_file(c["bases"], c["quals"], c["offsets"])
            sam = _sam_bytes(c["bases"], c["quals"], c["offsets"])
            c.update(index=index, mx=mx, bam=bam, payload=payload, sam=np.frombuffer(sam, np.uint8), sam_text=sam,
                     n_reads=len(c["offsets"]) - 1)
            _EXPECT[name] = c
        return _EXPECT[name]
    return get


@pytest.fixture(scope="module")
def devs(kmm):
    """One handle per k, shared by the tests of this module."""
    open_ = {}

    def get(case):
        if case["k"] not in open_:
            open_[case["k"]] = kmm.DeviceIndex.from_index(case["index"], case["mx"])
            assert open_[case["k"]].get_param("radix_available")
        return open_[case["k"]]
    yield get
    for d in open_.values():
        d.close()


def _run(dev, q, call, use=1, path=0, piece_kb=0, cap_kb=0, excl=0):
    """(node counts, lookups, masked bases, records without QUAL, what the call returned) of map call(s) on a clean handle."""
    dev.reset()
    dev.get_stats(reset=True)
    dev.set_param("min_base_quality", q)
    dev.set_param("use_record_qual", use)
    dev.set_param("path", path)
    dev.set_param("debug_records_piece_kb", piece_kb)
    dev.set_param("debug_bgzf_call_cap_kb", cap_kb)
    dev.set_param("bam_exclude_flags", excl)
    try:
        ret = call()
        return (dev.get_node_counts().copy(), dev.get_stats()[0], dev.get_param("quality_masked_bases"),
                dev.get_param("records_without_qual"), ret)
    finally:
        dev.set_param("min_base_quality", 0)
        dev.set_param("use_record_qual", 0)
        dev.set_param("path", 0)
        dev.set_param("debug_records_piece_kb", 0)
        dev.set_param("debug_bgzf_call_cap_kb", 0)
        dev.set_param("bam_exclude_flags", 0)


def _check(dev, case, lut, call, what, n_ret=None, want=None, n_no_qual=0, **kw):
    """call(lut, also_revcomp) against the oracle on the split reads, forward and with reverse complements."""
    table = lut if case["use_lut"] else None
    want = want or (case["split"], case["split_rc"], case["n_windows"], case["n_masked"])
    for rc in (False, True):
        got, lookups, masked, no_qual, ret = _run(dev, case["q"], lambda: call(table, rc), **kw)
        assert np.array_equal(got, want[1 if rc else 0]), (case["name"], what, rc)
        assert lookups == (2 if rc else 1) * want[2], (case["name"], what, rc, "lookups")
        assert masked == want[3], (case["name"], what, rc, "quality_masked_bases")
        assert no_qual == n_no_qual, (case["name"], what, rc, "records_without_qual")
        if n_ret is not None:
            assert ret == n_ret, (case["name"], what, rc)


def _bam_in_calls(dev, bam, k, table, rc):
    """kmm_map_bam's caller when a call takes less than it is given (the call cap): go on at bam[used:]; (bytes, records, whether
    a call ended inside a record and left a carry)."""
    pos = n = 0
    carried = False
    while pos < len(bam):
        used, n_rec = dev.map_bam(bam[pos:], first=pos == 0, last=True, k=k, also_revcomp=rc, lut=table)
        assert used > 0
        pos += used
        n += n_rec
        carried = carried or dev.get_param("bgzf_carry_bytes") > 0
    return pos, n, carried


@pytest.mark.parametrize("name", qc.CASES)
def test_every_case_as_bam(kmm, expect, devs, lut, name):
    """One call from a host buffer; "path" 1 and 2 (both end on the radix path, as on the FASTQ routes); several calls under a
    call cap of 4 KiB (16 for long_read, whose record of 15 KB has to fit a call), so that calls end inside records and the
    carry is used."""
    case = expect(name)
    dev = devs(case)
    k, bam = case["k"], case["bam"]
    done = (len(bam), case["n_reads"])
    _check(dev, case, lut, lambda t, rc: dev.map_bam(bam, first=True, last=True, k=k, also_revcomp=rc, lut=t), "one call", done)
    for path in (1, 2):
        radix, direct = dev.get_param("radix_batches"), dev.get_param("direct_batches")
        _check(dev, case, lut, lambda t, rc: dev.map_bam(bam, first=True, last=True, k=k, also_revcomp=rc, lut=t), "path %d" % path, done,
               path=path)
        assert dev.get_param("radix_batches") == radix + 2 and dev.get_param("direct_batches") == direct
    cap_kb, n_calls = (16, 2) if name == "long_read" else (CAP_KB, 3)
    assert len(case["payload"]) > n_calls * (cap_kb << 10) or name == "long_read"
    calls = dev.get_param("bam_calls")
    _check(dev, case, lut, lambda t, rc: _bam_in_calls(dev, bam, k, t, rc), "several calls", done + (True,), cap_kb=cap_kb)
    assert dev.get_param("bam_calls") >= calls + 2 * n_calls


def _gzip_two_windows(dev, gz, k, table, rc):
    pos, total, end = 0, 0, len(gz) // 2
    while pos < len(gz):
        used, n_rec = dev.map_gzip(gz[pos:end], fmt=SAM, k=k, first=pos == 0, last=end == len(gz), also_revcomp=rc, lut=table)
        total += n_rec
        pos += used
        if used == 0 or end < len(gz):
            assert end < len(gz)
            end = len(gz)
    return total


@pytest.mark.parametrize("name", qc.CASES)
def test_every_case_as_sam(kmm, expect, devs, lut, name):
    """kmm_map_records from host and from device memory (tile_edges also in pieces of 16 KiB), BGZF members of 4 KiB through
    kmm_map_bgzf, plain gzip in two windows through kmm_map_gzip."""
    import torch
    from kmer_mapper_amd import reads_io
    case = expect(name)
    dev = devs(case)
    k, sam, text = case["k"], case["sam"], case["sam_text"]
    d_sam = torch.from_numpy(sam.copy()).cuda()
    done = (len(sam), case["n_reads"])
    _check(dev, case, lut, lambda t, rc: dev.map_records(sam, fmt=SAM, k=k, also_revcomp=rc, lut=t), "host", done)
    _check(dev, case, lut, lambda t, rc: dev.map_records(d_sam, fmt=SAM, k=k, also_revcomp=rc, lut=t), "device", done)
    if name == "tile_edges":
        assert len(sam) >= 3 * (qc.PIECE_KB << 10)
        for src, what in ((sam, "pieces, host"), (d_sam, "pieces, device")):
            _check(dev, case, lut, lambda t, rc: dev.map_records(src, fmt=SAM, k=k, also_revcomp=rc, lut=t), what, done, piece_kb=qc.PIECE_KB)
    bgzf = np.frombuffer(reads_io.bgzf_members(text, 0x1000) + reads_io.BGZF_EOF, np.uint8)
    _check(dev, case, lut, lambda t, rc: dev.map_bgzf(bgzf, fmt=SAM, k=k, first=True, last=True, also_revcomp=rc, lut=t), "bgzf",
           (len(bgzf), case["n_reads"]))
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    third = len(text) // 3
    gz = np.frombuffer(c.compress(text[:third]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[third:]) + c.flush(), np.uint8)
    _check(dev, case, lut, lambda t, rc: _gzip_two_windows(dev, gz, k, t, rc), "gzip", case["n_reads"])


def test_a_read_of_40000_bases_between_ordinary_ones(kmm, expect, devs, oracle):
    """Its BAM record covers four 16 KiB tiles, its SAM line forty of 1 KiB; low bases at its ends, around the flat edges of
    the compaction tiles, and on both sides of every 16 KiB boundary of the inflated BAM bytes inside its qualities."""
    from kmer_mapper_amd import reads_io
    base = expect("read_ends")
    dev = devs(base)
    k, index, mx = base["k"], base["index"], base["mx"]
    rng = np.random.Generator(np.random.PCG64(61))
    G = qc.GENOME
    pieces = [qc.ACGT[G[100 * i:100 * i + qc.L]] for i in range(10)]
    pieces.append(np.concatenate([qc.ACGT[G[100:20_100]], qc.ACGT[G[15_000:35_000]]]))
    pieces += [qc.ACGT[G[2000 + 100 * i:2000 + 100 * i + qc.L]] for i in range(10)]
    offsets = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([len(p) for p in pieces], out=offsets[1:])
    bases = np.concatenate(pieces)
    quals = np.full(len(bases), qc.HIGH, np.uint8)
    quals[rng.random(len(bases)) < 0.03] = 33 + 20
    lo, hi = int(offsets[10]), int(offsets[11])
    assert hi - lo == 40_000
    low = [lo, hi - 1, lo - 1, hi] + [p for e in range(4096, len(bases), 4096) for p in (e - 1, e)]
    _, payload = _bam_file(bases, quals, offsets)
    marker = (quals[lo:hi] - 33).astype(np.uint8).tobytes()
    q0 = payload.index(marker)                               # where the long record's qualities lie in the inflated bytes
    edges = list(range((q0 // 16384 + 1) * 16384, q0 + 40_000, 16384))
    assert len(edges) >= 2
    low += [lo + e - q0 + d for e in edges for d in (-1, 0)]
    quals[low] = 33 + 20 - 1
    mask = qc.low_mask(quals, 20)
    want = _answers(oracle, index, mx, bases, offsets, k, mask) + (int(mask.sum()),)
    case = dict(name="read of 40000", q=20, use_lut=False)
    bam, payload = _bam_file(bases, quals, offsets)
    assert (q0 + 40_000 - 1) // 16384 - (q0 - 20_000 - 40) // 16384 == 3           # the long record lies in four tiles
    sam = np.frombuffer(_sam_bytes(bases, quals, offsets), np.uint8)
    _check(dev, case, None, lambda t, rc: dev.map_bam(bam, first=True, last=True, k=k, also_revcomp=rc), "bam", (len(bam), 21), want=want)
    _check(dev, case, None, lambda t, rc: dev.map_records(sam, fmt=SAM, k=k, also_revcomp=rc), "sam", (len(sam), 21), want=want)
    bgzf = np.frombuffer(reads_io.bgzf_members(sam.tobytes(), 0x1000) + reads_io.BGZF_EOF, np.uint8)
    _check(dev, case, None, lambda t, rc: dev.map_bgzf(bgzf, fmt=SAM, k=k, first=True, last=True, also_revcomp=rc), "sam, bgzf",
           (len(bgzf), 21), want=want)


def test_absent_qualities_pass_the_floor_and_are_counted(kmm, expect, devs, oracle):
    """Half the records of read_ends with QUAL "*" / 0xFF: the counts of a mask that is cleared on those reads,
    "records_without_qual" their number, "quality_masked_bases" the low bytes of the others."""
    case = expect("read_ends")
    dev = devs(case)
    k, offsets = case["k"], case["offsets"]
    absent = set(range(0, case["n_reads"], 2))
    mask = np.array(qc.dead_mask(case))
    for i in absent:
        mask[offsets[i]:offsets[i + 1]] = False
    assert 0 < mask.sum() < case["n_masked"]
    want = _answers(oracle, case["index"], case["mx"], case["bases"], offsets, k, mask) + (int(mask.sum()),)
    assert not np.array_equal(want[0], case["split"]) and not np.array_equal(want[0], case["unsplit"])
    bam, _ = _bam_file(case["bases"], case["quals"], offsets, absent)
    sam = np.frombuffer(_sam_bytes(case["bases"], case["quals"], offsets, absent), np.uint8)
    _check(dev, case, None, lambda t, rc: dev.map_bam(bam, first=True, last=True, k=k, also_revcomp=rc), "bam", (len(bam), 300), want=want,
           n_no_qual=len(absent))
    _check(dev, case, None, lambda t, rc: dev.map_records(sam, fmt=SAM, k=k, also_revcomp=rc), "sam", (len(sam), 300), want=want,
           n_no_qual=len(absent))
    _check(dev, case, None, lambda t, rc: dev.map_records(sam, fmt=SAM, k=k, also_revcomp=rc), "sam, pieces", (len(sam), 300), want=want,
           n_no_qual=len(absent), piece_kb=qc.PIECE_KB)
    # (with the floor off nothing is counted: QUAL is not read)
    got = _run(dev, 0, lambda: dev.map_bam(bam, first=True, last=True, k=k))
    assert np.array_equal(got[0], case["unsplit"]) and got[2] == 0 and got[3] == 0


def test_excluded_records_contribute_neither_counts_nor_masked_bases(kmm, expect, devs, oracle):
    """"bam_exclude_flags" 0x900 with the floor: half the records are secondary or supplementary, a few of them without
    qualities."""
    case = expect("tile_edges")
    dev = devs(case)
    k, offsets, n = case["k"], case["offsets"], case["n_reads"]
    flags = [256 if i % 3 == 1 else 2048 | 16 if i % 6 == 2 else 4 for i in range(n)]
    kept = np.array([not f & 0x900 for f in flags])
    absent = {1, 4, 6, 9}                                    # two of them excluded (1, 4), two kept (6, 9)
    assert not kept[1] and not kept[4] and kept[6] and kept[9]
    read_of = np.repeat(np.arange(n), np.diff(offsets))
    sel = kept[read_of]
    k_off = np.zeros(int(kept.sum()) + 1, np.int64)
    np.cumsum(np.diff(offsets)[kept], out=k_off[1:])
    mask = np.array(qc.dead_mask(case))
    for i in absent:
        mask[offsets[i]:offsets[i + 1]] = False
    want = _answers(oracle, case["index"], case["mx"], case["bases"][sel], k_off, k, mask[sel]) + (int(mask[sel].sum()),)
    assert 0 < want[3] < case["n_masked"]
    bam, _ = _bam_file(case["bases"], case["quals"], offsets, absent, flags)
    sam = np.frombuffer(_sam_bytes(case["bases"], case["quals"], offsets, absent, flags), np.uint8)
    n_kept = int(kept.sum())
    before = dev.get_param("bam_records_excluded"), dev.get_param("sam_records_excluded")
    _check(dev, case, None, lambda t, rc: dev.map_bam(bam, first=True, last=True, k=k, also_revcomp=rc), "bam", (len(bam), n_kept),
           want=want, n_no_qual=2, excl=0x900)
    assert dev.get_param("bam_records_excluded") == before[0] + 2 * (n - n_kept)         # (two calls: forward, reverse complement)
    _check(dev, case, None, lambda t, rc: dev.map_records(sam, fmt=SAM, k=k, also_revcomp=rc), "sam", (len(sam), n_kept), want=want,
           n_no_qual=2, excl=0x900)
    assert dev.get_param("sam_records_excluded") == before[1] + 2 * (n - n_kept)


def _sam_with_qual(case, record, delta):
    """The case's SAM text with the QUAL of `record` one byte longer (delta 1) or shorter (-1); the offset of that line."""
    text = case["sam_text"]
    lines = text.split(b"\n")
    n_header = sum(1 for ln in lines if ln[:1] == b"@")
    i = n_header + record
    at = sum(len(ln) + 1 for ln in lines[:i])
    assert lines[i].startswith(b"r%d\t" % record)
    lines[i] = lines[i] + b"I" if delta > 0 else lines[i][:-1]
    return np.frombuffer(b"\n".join(lines), np.uint8), at


@pytest.mark.parametrize("record", [0, 299])
@pytest.mark.parametrize("delta", [-1, 1])
def test_a_sam_qual_of_another_length_is_malformed(kmm, expect, devs, record, delta):
    """One byte short and one byte long, in the first record and in the last (a later piece, when the call is cut in pieces):
    KMM_ERR_MALFORMED with the line's offset, nothing of the call counted, and the handle works again after reset(); with the
    switch's floor off the line is not looked at."""
    from kmer_mapper_amd import reads_io
    case = expect("read_ends")
    dev = devs(case)
    k = case["k"]
    raw, at = _sam_with_qual(case, record, delta)
    assert len(raw) == len(case["sam"]) + delta
    bgzf = np.frombuffer(reads_io.bgzf_members(raw.tobytes(), 0x1000) + reads_io.BGZF_EOF, np.uint8)
    for what, call, kw in (("one piece", lambda: dev.map_records(raw, fmt=SAM, k=k), {}),
                           ("pieces", lambda: dev.map_records(raw, fmt=SAM, k=k), dict(piece_kb=qc.PIECE_KB)),
                           ("bgzf", lambda: dev.map_bgzf(bgzf, fmt=SAM, k=k, first=True, last=True), {})):
        records = dev.get_param("sam_records")
        with pytest.raises(ValueError, match=r"SAM line at byte %d of the chunk: QUAL is not .* as long as SEQ" % at):
            _run(dev, 20, call, **kw)
        assert not dev.get_node_counts().any() and dev.get_stats()[0] == 0, what
        assert dev.get_param("sam_records") == records, what
        dev.reset()
    got = _run(dev, 20, lambda: dev.map_records(case["sam"], fmt=SAM, k=k))
    assert np.array_equal(got[0], case["split"]) and got[2] == case["n_masked"]
    got = _run(dev, 0, lambda: dev.map_records(raw, fmt=SAM, k=k))
    assert np.array_equal(got[0], case["unsplit"]) and got[1] == case["n_all"]


def test_refusals_and_identities(kmm, expect, devs):
    """k = 1; an index without a radix view (the FASTQ hand-off needs the radix path: refused, as kmm.h states); a switch value
    of 2; the switch with Q = 0 is the library without it, counters included; without the switch Q = 20 still refuses."""
    import types
    case = expect("tile_edges")
    dev = devs(case)
    k, bam, sam = case["k"], case["bam"], case["sam"]
    for bad in (2, -1):
        with pytest.raises(ValueError, match="use_record_qual takes 0 or 1"):
            dev.set_param("use_record_qual", bad)
    assert dev.get_param("use_record_qual") == 0
    with pytest.raises(ValueError, match="k = 1 with min_base_quality"):
        _run(dev, 20, lambda: dev.map_bam(bam, first=True, last=True, k=1))
    with pytest.raises(ValueError, match="k = 1 with min_base_quality"):
        _run(dev, 20, lambda: dev.map_records(sam, fmt=SAM, k=1))
    with pytest.raises(ValueError, match="SAM / BAM records are mapped without their QUAL.*use_record_qual"):
        _run(dev, 20, lambda: dev.map_bam(bam, first=True, last=True, k=k), use=0)
    dev.reset()

    counters = ("bam_calls", "bam_records", "bam_records_excluded", "bam_header_bytes", "bam_false_starts", "bam_continuations",
                "sam_calls", "sam_records", "sam_records_excluded", "sam_header_lines", "flat_uniform_batches", "radix_batches",
                "direct_batches")

    def deltas(call, use, path):
        before = [dev.get_param(c) for c in counters]
        got = _run(dev, 0, call, use=use, path=path)
        return got, [dev.get_param(c) - b for c, b in zip(counters, before)]
    for call in (lambda: dev.map_bam(bam, first=True, last=True, k=k), lambda: dev.map_records(sam, fmt=SAM, k=k)):
        for path in (0, 2):
            off, d_off = deltas(call, 0, path)
            on, d_on = deltas(call, 1, path)
            assert np.array_equal(on[0], off[0]) and np.array_equal(on[0], case["unsplit"])
            assert on[1:] == off[1:] and on[1] == case["n_all"] and on[2] == 0 and on[3] == 0
            assert d_on == d_off

    index = case["index"]
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo)
    with kmm.DeviceIndex.from_index(dup, case["mx"]) as other:
        assert other.get_param("radix_available") == 0
        for call in (lambda: other.map_bam(bam, first=True, last=True, k=k), lambda: other.map_records(sam, fmt=SAM, k=k)):
            with pytest.raises(ValueError, match="min_base_quality needs the radix path"):
                _run(other, 20, call)
            assert not other.get_node_counts().any()
            got = _run(other, 0, call)
            assert np.array_equal(got[0], case["unsplit"])


def test_cli_end_to_end(kmm, expect, lut, oracle, tmp_path, caplog):
    """`kmer_mapper map --min-base-quality 20 --use-record-qual` on the 400 reads of tile_edges as .bam, .sam and BGZF .sam.gz:
    each writes the oracle's vector and logs the masked bases; a BAM with a few N under --ambiguous-bases skip; a few records
    without qualities are logged; the flag on a .fq is refused."""
    import logging
    from kmer_mapper_amd import command_line_interface as cli, reads_io
    from kmer_mapper_amd.util import ReadBatch
    case = expect("tile_edges")
    assert case["n_reads"] == 400
    offsets, quals = case["offsets"], case["quals"]
    idx = str(tmp_path / "idx.npz")
    case["index"].to_file(idx)
    batch = ReadBatch(case["bases"], offsets)
    bam, sam, samgz = str(tmp_path / "reads.bam"), str(tmp_path / "reads.sam"), str(tmp_path / "reads.sam.gz")
    reads_io.write_bam(bam, batch, quals=_bam_quals(quals, offsets), block=0x1000)
    reads_io.write_sam(sam, batch, quals=_sam_quals(quals, offsets))
    reads_io.write_sam(samgz, batch, quals=_sam_quals(quals, offsets), bgzf=True, block=0x1000)
    bases = np.array(case["bases"])
    bases[[150 * 5 + 70, 150 * 9, 150 * 300 + 149]] = ord("N")
    both = dict(case, bases=bases, use_lut=True)
    want_both = _answers(oracle, case["index"], case["mx"], bases, offsets, case["k"], qc.dead_mask(both))[0]
    assert not np.array_equal(want_both, case["split"])
    bam_n = str(tmp_path / "reads_n.bam")
    reads_io.write_bam(bam_n, ReadBatch(bases, offsets), quals=_bam_quals(quals, offsets), block=0x1000)
    out = str(tmp_path / "out")
    for path, extra, want in ((bam, [], case["split"]), (sam, [], case["split"]), (samgz, [], case["split"]),
                              (bam_n, ["--ambiguous-bases", "skip"], want_both), (sam, ["-t", "1"], case["split"])):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out, "--min-base-quality", "20", "--use-record-qual"] + extra)
        got = np.load(out + ".npy")
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any(), (path, extra)
        assert "quality_masked_bases: %d bases" % case["n_masked"] in caplog.text, (path, extra)
        assert "records_without_qual" not in caplog.text
    # three records without qualities: logged, and their low bases alive
    absent = {0, 130, 399}
    mask = np.array(qc.dead_mask(case))
    for i in absent:
        mask[offsets[i]:offsets[i + 1]] = False
    want = _answers(oracle, case["index"], case["mx"], case["bases"], offsets, case["k"], mask)[0]
    reads_io.write_bam(bam, batch, quals=_bam_quals(quals, offsets, absent), block=0x1000)
    caplog.clear()
    with caplog.at_level(logging.INFO):
        cli.run_argument_parser(["map", "-i", idx, "-f", bam, "-o", out, "--min-base-quality", "20", "--use-record-qual"])
    assert np.array_equal(np.load(out + ".npy")[:len(want)], want)
    assert "quality_masked_bases: %d bases" % int(mask.sum()) in caplog.text and "records_without_qual: 3 records" in caplog.text
    # without --min-base-quality the flag warns once and the file is mapped as before
    caplog.clear()
    with caplog.at_level(logging.INFO):
        cli.run_argument_parser(["map", "-i", idx, "-f", sam, "-o", out, "--use-record-qual"])
    assert caplog.text.count("--use-record-qual has no effect without --min-base-quality") == 1
    assert np.array_equal(np.load(out + ".npy")[:len(case["unsplit"])], case["unsplit"])
    fq = str(tmp_path / "reads.fq")
    with open(fq, "wb") as f:
        f.write(qc.case_text(case)[0])
    caplog.clear()
    with caplog.at_level(logging.INFO), pytest.raises(ValueError, match="--use-record-qual applies to SAM and BAM input only"):
        cli.run_argument_parser(["map", "-i", idx, "-f", fq, "-o", out, "--min-base-quality", "20", "--use-record-qual"])
    assert "Index resident in HBM" not in caplog.text      # refused before the index went up


def test_two_rank_gloo_rehearsal_with_the_floor(tmp_path):
    """Two ranks on the box's one GPU (the reduce over gloo), each process under its own time limit, mapping SAM with
    --min-base-quality 20 --use-record-qual: a plain file split by byte ranges, a BGZF one by member ranges, a gzip one by chunk
    round-robin — the oracle's counts on the reads split at their low bases (tools/sam_two_rank_rehearsal.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tools", "sam_two_rank_rehearsal.py")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, script, "--prepare", str(tmp_path), "20"], cwd=root,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    env = dict(os.environ, KMM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29673", WORLD_SIZE="2")
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, script, str(tmp_path)], cwd=root,
                              env=dict(env, RANK=str(i), LOCAL_RANK=str(i)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for i in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    assert outs[0].count("SAME AS ONE RANK") == 3 and "DIFFERS" not in outs[0], outs[0][-2000:]
    assert "quality_masked_bases" in outs[0] and "records_without_qual" in outs[0]
