"""GPU tests of "min_base_quality" (include/kmm.h): with a floor Q > 0 no k-mer over a FASTQ base whose quality
byte is below '!' + Q is counted, on every call that parses FASTQ records.  The node counts equal the oracle's on the reads
split at their masked bases, kmm_get_stats' lookups the windows that survive, and "quality_masked_bases" the numpy count
(tests/quality_cases.py, held to their conditions by tests/test_quality_cases_on_the_cpu.py)."""
import gzip
import zlib

import numpy as np
import pytest

from tests import quality_cases as qc

pytestmark = pytest.mark.gpu


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


_EXPECT = {}


@pytest.fixture(scope="module")
def expect(oracle):
    """name -> the case, its text, its index and the oracle's answers (computed once, never changed)."""
    def get(name):
        if name not in _EXPECT:
            c = dict(qc.build(name))
            index = qc.index_for(c["k"])
            mx = index.max_node_id()
            sb, so = qc.split_at_mask(c["bases"], c["offsets"], qc.dead_mask(c))
            c["split"], c["n_windows"] = oracle.map_reads(index, mx, sb, so, c["k"])
            c["split_rc"], _ = oracle.map_reads(index, mx, sb, so, c["k"], also_revcomp=True)
            sb, so = qc.split_at_mask(c["bases"], c["offsets"], qc.dead_mask(c, q=0))
            c["unsplit"], c["n_all"] = oracle.map_reads(index, mx, sb, so, c["k"])
            c["n_masked"] = int(qc.low_mask(c["quals"], c["q"]).sum())
            text, _, layout = qc.case_text(c)
            c.update(index=index, mx=mx, text=text, layout=layout, raw=np.frombuffer(text, np.uint8), n_reads=len(c["offsets"]) - 1)
            for a in (c["split"], c["split_rc"], c["unsplit"]):
                a.setflags(write=False)
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


def _run(dev, q, call, path=0, piece_kb=0):
    """(node counts, lookups, masked bases, what the call returned) of map call(s) on a clean handle with the floor q."""
    dev.reset()
    dev.get_stats(reset=True)
    dev.set_param("min_base_quality", q)
    dev.set_param("path", path)
    dev.set_param("debug_records_piece_kb", piece_kb)
    try:
        ret = call()
        return dev.get_node_counts().copy(), dev.get_stats()[0], dev.get_param("quality_masked_bases"), ret
    finally:
        dev.set_param("min_base_quality", 0)
        dev.set_param("path", 0)
        dev.set_param("debug_records_piece_kb", 0)


def _check(dev, case, lut, call, what, n_ret=None, **kw):
    """call(lut, also_revcomp) against the oracle on the split reads, forward and with reverse complements."""
    table = lut if case["use_lut"] else None
    for rc, want in ((False, case["split"]), (True, case["split_rc"])):
        got, lookups, masked, ret = _run(dev, case["q"], lambda: call(table, rc), **kw)
        assert np.array_equal(got, want), (case["name"], what, rc)
        assert lookups == (2 if rc else 1) * case["n_windows"], (case["name"], what, rc, "lookups")
        assert masked == case["n_masked"], (case["name"], what, rc, "quality_masked_bases")
        if n_ret is not None:
            assert ret == n_ret, (case["name"], what, rc)


@pytest.mark.parametrize("name", qc.CASES)
def test_map_records_from_host_device_and_an_odd_address(kmm, expect, devs, lut, name):
    """kmm_map_records on the FASTQ text, from a host buffer, a device buffer, and a device buffer shifted by one byte (the
    unaligned 16-byte loads); "path" 1 and 2 give the same and both take the radix path."""
    import torch
    case = expect(name)
    dev = devs(case)
    k, raw = case["k"], case["raw"]
    d_raw = torch.from_numpy(raw.copy()).cuda()
    shifted = torch.empty(raw.shape[0] + 1, dtype=torch.uint8, device="cuda")
    shifted[1:] = d_raw
    done = (len(case["text"]), case["n_reads"])
    _check(dev, case, lut, lambda t, rc: dev.map_records(raw, fmt=4, k=k, also_revcomp=rc, lut=t), "host", done)
    _check(dev, case, lut, lambda t, rc: dev.map_records(d_raw, fmt=4, k=k, also_revcomp=rc, lut=t), "device", done)
    _check(dev, case, lut, lambda t, rc: dev.map_records(shifted[1:], fmt=4, k=k, also_revcomp=rc, lut=t), "odd address", done)
    for path in (1, 2):                  # the parameter is ignored: compaction + the radix path whatever it says
        radix, direct = dev.get_param("radix_batches"), dev.get_param("direct_batches")
        _check(dev, case, lut, lambda t, rc: dev.map_records(d_raw, fmt=4, k=k, also_revcomp=rc, lut=t), "path %d" % path, done,
               path=path)
        assert dev.get_param("radix_batches") == radix + 2 and dev.get_param("direct_batches") == direct


@pytest.mark.parametrize("name", qc.CASES)
def test_several_pieces_and_chunked_calls(kmm, expect, devs, lut, name):
    """The text cut into pieces of a few KiB inside one call ("debug_records_piece_kb": the quality base of a later piece is
    its flat_base), and fed in chunks that end mid-record, the caller re-feeding raw[consumed:]."""
    import torch
    case = expect(name)
    dev = devs(case)
    k, raw = case["k"], case["raw"]
    d_raw = torch.from_numpy(raw.copy()).cuda()
    done = (len(case["text"]), case["n_reads"])
    piece_kb = qc.PIECE_KB if len(raw) > (3 * qc.PIECE_KB << 10) else max(1, len(raw) // 4096)      # at least three pieces
    if name != "long_read":              # (its record of 10 000 bases needs a piece of 24 KiB, and the text has 30)
        assert len(raw) >= 3 * (piece_kb << 10)
        _check(dev, case, lut, lambda t, rc: dev.map_records(raw, fmt=4, k=k, also_revcomp=rc, lut=t), "pieces, host", done, piece_kb=piece_kb)
        _check(dev, case, lut, lambda t, rc: dev.map_records(d_raw, fmt=4, k=k, also_revcomp=rc, lut=t), "pieces, device", done,
               piece_kb=piece_kb)

    def chunked(source, step):
        def call(t, rc):
            pos = n = 0
            while pos < len(raw):
                used, n_rec = dev.map_records(source[pos:pos + step], fmt=4, k=k, also_revcomp=rc, lut=t)
                assert used > 0
                pos += used
                n += n_rec
            return pos, n
        return call
    step = 25_001 if name == "long_read" else 7_001
    assert any(lay[0] < step < lay[3] for lay in case["layout"])        # the first chunk ends inside a record
    _check(dev, case, lut, chunked(raw, step), "chunks, host", done)
    _check(dev, case, lut, chunked(d_raw, step), "chunks, device", done)
    if name == "tile_edges":             # the second piece starts on a record whose first base is low
        r = qc.second_piece_record(case["layout"], qc.PIECE_KB << 10)
        assert case["quals"][case["offsets"][r]] < 33 + case["q"]


def _gzip_two_windows(dev, gz, k, table, rc):
    """kmm_map_gzip's caller: a first window that ends inside the stream, then the rest; each call goes on where the one before
    could verify a block boundary."""
    pos, total, end = 0, 0, len(gz) // 2
    while pos < len(gz):
        used, n_rec = dev.map_gzip(gz[pos:end], fmt=4, k=k, first=pos == 0, last=end == len(gz), also_revcomp=rc, lut=table)
        total += n_rec
        pos += used
        if used == 0 or end < len(gz):
            assert end < len(gz)
            end = len(gz)
    return total


@pytest.mark.parametrize("name", ["tile_edges", "ragged_1_to_400", "with_skip_table", "long_read"])
def test_compressed_routes(kmm, expect, devs, lut, name):
    """BGZF members of 32 KiB through kmm_map_bgzf; plain gzip (a full flush in the middle, so that the first of two windows
    ends behind a block boundary) through kmm_map_gzip."""
    from kmer_mapper_amd import reads_io
    case = expect(name)
    dev = devs(case)
    k, text = case["k"], case["text"]
    bgzf = np.frombuffer(reads_io.bgzf_members(text, 0x8000) + reads_io.BGZF_EOF, np.uint8)
    _check(dev, case, lut, lambda t, rc: dev.map_bgzf(bgzf, fmt=4, k=k, first=True, last=True, also_revcomp=rc, lut=t), "bgzf",
           (len(bgzf), case["n_reads"]))
    if name in ("tile_edges", "ragged_1_to_400"):
        c = zlib.compressobj(6, zlib.DEFLATED, 31)
        half = len(text) // 3
        gz = np.frombuffer(c.compress(text[:half]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[half:]) + c.flush(), np.uint8)
        _check(dev, case, lut, lambda t, rc: _gzip_two_windows(dev, gz, k, t, rc), "gzip", case["n_reads"])


def test_floor_off_after_on_is_bit_for_bit_the_library_without_it(kmm, expect, devs):
    """Q = 0 after Q = 20 on the same handle: the oracle's counts on the unsplit reads, and reads of one length take the
    uniform front end of pass 1 again (with the floor they take the ragged one: more starts than records)."""
    import torch
    case = expect("tile_edges")
    dev = devs(case)
    d_raw = torch.from_numpy(case["raw"].copy()).cuda()
    call = lambda: dev.map_records(d_raw, fmt=4, k=case["k"])          # noqa: E731
    before = dev.get_param("flat_uniform_batches")
    got, lookups, masked, _ = _run(dev, 20, call, path=2)
    assert np.array_equal(got, case["split"]) and masked == case["n_masked"]
    assert dev.get_param("flat_uniform_batches") == before
    got, lookups, masked, _ = _run(dev, 0, call, path=2)
    assert np.array_equal(got, case["unsplit"]) and lookups == case["n_all"] and masked == 0
    assert dev.get_param("flat_uniform_batches") == before + 1
    assert dev.get_param("min_base_quality") == 0


def test_the_host_packer_is_bypassed(kmm, expect):
    """host_pack_threads 16 and a chunk that qualifies for the packer: it packs with the floor off and is not used with it on."""
    case = expect("tile_edges")
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.set_param("host_pack_threads", 16)
        dev.set_param("radix_min_units", 1)
        call = lambda: dev.map_records(case["raw"], fmt=4, k=case["k"])  # noqa: E731
        before = dev.get_param("host_packed_record_calls")
        got, _, masked, _ = _run(dev, 20, call)
        assert np.array_equal(got, case["split"]) and masked == case["n_masked"]
        assert dev.get_param("host_packed_record_calls") == before
        got, _, masked, _ = _run(dev, 0, call)
        assert np.array_equal(got, case["unsplit"]) and masked == 0
        assert dev.get_param("host_packed_record_calls") == before + 1


def test_with_the_skip_table_a_base_is_dead_if_either_rule_kills_it(kmm, expect, devs, lut, oracle):
    """Q = 20 plus util.ambiguous_skip_lut(): the oracle on the reads split at the union of both masks — and each rule alone
    gives something else (the floor alone reads N as A)."""
    case = expect("with_skip_table")
    dev = devs(case)
    call = lambda t: (lambda: dev.map_records(case["raw"], fmt=4, k=case["k"], lut=t))       # noqa: E731
    both, n_both, _, _ = _run(dev, 20, call(lut))
    assert np.array_equal(both, case["split"]) and n_both == case["n_windows"]
    for q, table in ((20, None), (0, lut)):
        sb, so = qc.split_at_mask(case["bases"], case["offsets"], qc.dead_mask(case, q=q, with_lut=table is not None))
        want, n = oracle.map_reads(case["index"], case["mx"], sb, so, case["k"])
        got, lookups, _, _ = _run(dev, q, call(table))
        assert np.array_equal(got, want) and lookups == n and n > n_both and not np.array_equal(want, both)


def _with_quality_line(case, record, delta):
    """The case's text with the quality line of `record` one byte longer (delta 1) or shorter (-1); the raw offset of that
    line's newline in the new text."""
    text, (_, _, qual0, qual_nl) = case["text"], case["layout"][record]
    assert text[qual_nl - 1:qual_nl] != b"\r"
    new = text[:qual_nl] + b"I" + text[qual_nl:] if delta > 0 else text[:qual_nl - 1] + text[qual_nl:]
    return np.frombuffer(new, np.uint8), qual_nl + delta


@pytest.mark.parametrize("record", [0, 30])
@pytest.mark.parametrize("delta", [-1, 1])
def test_a_quality_line_of_another_length_is_malformed(kmm, expect, devs, record, delta):
    """One byte short and one byte long, in the first record and in one past the first tile: KMM_ERR_MALFORMED at the next
    synchronising call, with the offset of the quality line's newline; the handle works again after reset(); with the floor
    off nothing is checked."""
    case = expect("read_ends")
    dev = devs(case)
    raw, at = _with_quality_line(case, record, delta)
    assert (case["layout"][30][2] > qc.TILE) and len(raw) == len(case["raw"]) + delta
    dev.reset()
    dev.set_param("min_base_quality", 20)
    try:
        dev.map_records(raw, fmt=4, k=case["k"])
        with pytest.raises(ValueError, match="byte offset %d of a mapped chunk .*quality line" % at):
            dev.get_node_counts()
    finally:
        dev.reset()
        dev.set_param("min_base_quality", 0)
    got, _, masked, _ = _run(dev, 20, lambda: dev.map_records(case["raw"], fmt=4, k=case["k"]))
    assert np.array_equal(got, case["split"]) and masked == case["n_masked"]
    got, lookups, _, _ = _run(dev, 0, lambda: dev.map_records(raw, fmt=4, k=case["k"]))
    assert np.array_equal(got, case["unsplit"]) and lookups == case["n_all"]


def test_quality_lines_far_longer_than_their_reads_leave_no_mark_outside_the_bitset(kmm, expect, devs):
    """Every quality line 300 low bytes long on reads of 4 bases: the quality bytes outnumber the bases seventy-five times, so
    their flat positions run far beyond the flat reads — malformed, reported, and the handle and its neighbours in HBM are
    unharmed (the same text maps cleanly with the floor off, and a good text after reset())."""
    case = expect("read_ends")
    dev = devs(case)
    bad = np.frombuffer(b"".join(b"@r%d\nACGT\n+\n" % i + b"#" * 300 + b"\n" for i in range(400)), np.uint8)
    dev.reset()
    dev.set_param("min_base_quality", 20)
    try:
        dev.map_records(bad, fmt=4, k=case["k"])
        with pytest.raises(ValueError, match="byte offset %d of a mapped chunk .*quality line" % (bad.tobytes().index(b"#\n") + 1)):
            dev.get_node_counts()
    finally:
        dev.reset()
        dev.set_param("min_base_quality", 0)
    got, _, masked, _ = _run(dev, 20, lambda: dev.map_records(case["raw"], fmt=4, k=case["k"]))
    assert np.array_equal(got, case["split"]) and masked == case["n_masked"]


def test_refusals(kmm, expect, devs, oracle):
    """KMM_ERR_INVALID_ARG with a message: SAM, BAM, k = 1, a floor outside 0 .. 93, an index without a radix view."""
    import types
    from kmer_mapper_amd import reads_io, _lib
    from kmer_mapper_amd.util import ReadBatch
    case = expect("read_ends")
    dev = devs(case)
    reads = [case["bases"][case["offsets"][i]:case["offsets"][i + 1]].tobytes() for i in range(20)]
    sam = np.frombuffer(reads_io.sam_text(ReadBatch.from_strings([r.decode() for r in reads])), np.uint8)
    bam = np.frombuffer(reads_io.bgzf_members(reads_io.bam_header()) +
                        reads_io.bgzf_members(b"".join(reads_io.bam_record(r, b"r%d" % i) for i, r in enumerate(reads))) +
                        reads_io.BGZF_EOF, np.uint8)
    sam_bgzf = np.frombuffer(reads_io.bgzf_members(sam.tobytes()) + reads_io.BGZF_EOF, np.uint8)
    dev.reset()
    for bad in (94, -1, 1000):
        with pytest.raises(ValueError, match="min_base_quality outside"):
            dev.set_param("min_base_quality", bad)
    assert dev.get_param("min_base_quality") == 0
    dev.set_param("min_base_quality", 20)
    try:
        with pytest.raises(ValueError, match="SAM / BAM records are mapped without their QUAL"):
            dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=case["k"])
        with pytest.raises(ValueError, match="SAM / BAM records are mapped without their QUAL"):
            dev.map_bgzf(sam_bgzf, fmt=_lib.FORMAT_SAM, k=case["k"], first=True, last=True)
        with pytest.raises(ValueError, match="SAM / BAM records are mapped without their QUAL"):
            dev.map_bam(bam, first=True, last=True, k=case["k"])
        with pytest.raises(ValueError, match="k = 1 with min_base_quality"):
            dev.map_records(case["raw"], fmt=4, k=1)
        assert not dev.get_node_counts().any()
    finally:
        dev.set_param("min_base_quality", 0)
    # with the floor off all three are served
    assert dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=case["k"]) == (len(sam), 20)
    assert dev.map_bam(bam, first=True, last=True, k=case["k"]) == (len(bam), 20)
    dev.reset()
    # an index without a radix view (two buckets share entries): the floor has no route
    index = case["index"]
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo)
    with kmm.DeviceIndex.from_index(dup, case["mx"]) as other:
        assert other.get_param("radix_available") == 0
        other.set_param("min_base_quality", 20)
        with pytest.raises(ValueError, match="min_base_quality needs the radix path"):
            other.map_records(case["raw"], fmt=4, k=case["k"])
        other.set_param("min_base_quality", 0)
        other.map_records(case["raw"], fmt=4, k=case["k"])
        assert np.array_equal(other.get_node_counts(), case["unsplit"])


def test_fasta_is_unaffected(kmm, expect, devs):
    """Two-line FASTA has no qualities: Q = 20 gives what Q = 0 gives."""
    case = expect("read_ends")
    dev = devs(case)
    fa = np.frombuffer(b"".join(b">r%d\n" % i + case["bases"][case["offsets"][i]:case["offsets"][i + 1]].tobytes() + b"\n"
                                for i in range(case["n_reads"])), np.uint8)
    for path in (0, 2):
        off = _run(dev, 0, lambda: dev.map_records(fa, fmt=2, k=case["k"]), path=path)
        on = _run(dev, 20, lambda: dev.map_records(fa, fmt=2, k=case["k"]), path=path)
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[0], case["unsplit"]) and on[1:] == off[1:] and on[2] == 0


def test_cli_end_to_end(kmm, expect, lut, oracle, tmp_path, caplog):
    """`kmer_mapper map --min-base-quality 20` on a 400-read file: plain, BGZF and plain gzip (inflated by the host) write the
    oracle's vector, also together with --ambiguous-bases skip; a FASTA input warns and maps; a SAM input is refused."""
    import logging
    from kmer_mapper_amd import command_line_interface as cli, reads_io
    from kmer_mapper_amd.gz_io import write_bgzf
    from kmer_mapper_amd.util import ReadBatch
    case = expect("tile_edges")
    assert case["n_reads"] == 400
    idx = str(tmp_path / "idx.npz")
    case["index"].to_file(idx)
    fq, bgz, gz = str(tmp_path / "reads.fq"), str(tmp_path / "reads.bgzf.fq.gz"), str(tmp_path / "reads.plain.fq.gz")
    with open(fq, "wb") as f:
        f.write(case["text"])
    write_bgzf(bgz, case["text"])
    with open(gz, "wb") as f:
        f.write(gzip.compress(case["text"], 6))
    # the same reads with a few N: the floor and the table together
    bases = np.array(case["bases"])
    bases[[150 * 5 + 70, 150 * 9, 150 * 300 + 149]] = ord("N")
    both = dict(case, bases=bases, use_lut=True)
    sb, so = qc.split_at_mask(bases, case["offsets"], qc.dead_mask(both))
    want_both, _ = oracle.map_reads(case["index"], case["mx"], sb, so, case["k"])
    assert not np.array_equal(want_both, case["split"])
    fq_n = str(tmp_path / "reads_n.fq")
    with open(fq_n, "wb") as f:
        f.write(qc.case_text(both)[0])
    out = str(tmp_path / "out")
    for path, extra, want in ((fq, [], case["split"]), (bgz, [], case["split"]), (gz, [], case["split"]),
                              (fq_n, ["--ambiguous-bases", "skip"], want_both), (fq, ["-t", "1"], case["split"])):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out, "--min-base-quality", "20"] + extra)
        got = np.load(out + ".npy")
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any(), (path, extra)
        assert "quality_masked_bases: %d bases" % case["n_masked"] in caplog.text, (path, extra)
    fa = str(tmp_path / "reads.fa")
    with open(fa, "wb") as f:
        f.write(b"".join(b">r%d\n" % i + case["bases"][150 * i:150 * i + 150].tobytes() + b"\n" for i in range(400)))
    caplog.clear()
    with caplog.at_level(logging.INFO):
        cli.run_argument_parser(["map", "-i", idx, "-f", fa, "-o", out, "--min-base-quality", "20"])
    assert caplog.text.count("has no effect on FASTA input") == 1
    assert np.array_equal(np.load(out + ".npy")[:len(case["unsplit"])], case["unsplit"])
    sam = str(tmp_path / "reads.sam")
    reads = [case["bases"][150 * i:150 * i + 150].tobytes().decode() for i in range(20)]
    with open(sam, "wb") as f:
        f.write(reads_io.sam_text(ReadBatch.from_strings(reads)))
    caplog.clear()
    with caplog.at_level(logging.INFO), pytest.raises(ValueError, match="QUAL column of SAM"):
        cli.run_argument_parser(["map", "-i", idx, "-f", sam, "-o", out, "--min-base-quality", "20"])
    assert "Index resident in HBM" not in caplog.text      # refused before the index went up
