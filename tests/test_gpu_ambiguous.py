"""GPU tests of the break code of the lookup table (KMM_LUT_BREAK, include/kmm.h): with
util.ambiguous_skip_lut() no k-mer over N or an IUPAC letter is counted, on every front end and on both paths; the node
counts and the number of lookups equal the oracle's on the reads split at their break bytes (tests/ambiguous_cases.py,
held to their conditions by tests/test_ambiguous_cases_on_the_cpu.py), and lut=None still gives N read as A."""
import gzip

import numpy as np
import pytest

from tests import ambiguous_cases as ac
from tests.skew_cases import numpy_entry_counts

pytestmark = pytest.mark.gpu

DIRECT, RADIX = 1, 2


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
def expect(oracle, lut):
    """name -> the case, its index and the oracle's answers (computed once, never changed)."""
    def get(name):
        if name not in _EXPECT:
            _, bases, offsets, k = ac.build(name)
            index = ac.index_for(k)
            mx = index.max_node_id()
            sb, so = ac.split_at_breaks(bases, offsets, lut)
            split, n_windows = oracle.map_reads(index, mx, sb, so, k)
            split_rc, _ = oracle.map_reads(index, mx, sb, so, k, also_revcomp=True)
            n_to_a, n_all = oracle.map_reads(index, mx, ac.n_to_a_bytes(bases, lut), offsets, k)
            for a in (split, split_rc, n_to_a, bases, offsets):
                a.setflags(write=False)
            _EXPECT[name] = dict(name=name, bases=bases, offsets=offsets, k=k, index=index, mx=mx, split=split, n_windows=n_windows,
                                 split_rc=split_rc, n_to_a=n_to_a, n_all=n_all, n_reads=len(offsets) - 1)
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


def _run(dev, path, call):
    """(node counts, lookups) of one map call on a clean handle with the path forced."""
    dev.reset()
    dev.get_stats(reset=True)
    dev.set_param("path", path)
    try:
        ret = call()
        return dev.get_node_counts().copy(), dev.get_stats()[0], ret
    finally:
        dev.set_param("path", 0)


def _check(dev, path, case, lut, call, what, n_ret=None):
    """call(lut, also_revcomp) through the three expectations: skip, skip with reverse complements, the default table."""
    got, lookups, ret = _run(dev, path, lambda: call(lut, False))
    assert np.array_equal(got, case["split"]), (case["name"], what, "skip")
    assert lookups == case["n_windows"], (case["name"], what, "lookups")
    if n_ret is not None:
        assert ret == n_ret, (case["name"], what)
    got, lookups, _ = _run(dev, path, lambda: call(lut, True))
    assert np.array_equal(got, case["split_rc"]), (case["name"], what, "skip, reverse complements")
    assert lookups == 2 * case["n_windows"], (case["name"], what, "lookups, reverse complements")
    if set(case["bases"].tobytes()) <= set(b"ACGTNacgtn"):        # (the default table reads no IUPAC letter)
        got, lookups, _ = _run(dev, path, lambda: call(None, False))
        assert np.array_equal(got, case["n_to_a"]), (case["name"], what, "default table")
        assert lookups == case["n_all"], (case["name"], what, "default table, lookups")


@pytest.mark.parametrize("path", [DIRECT, RADIX])
@pytest.mark.parametrize("name", ac.CASES)
def test_flat_reads(kmm, expect, devs, lut, name, path):
    """kmm_map_reads with host and device pointers (the table too), kmm_map_reads_uniform on the reads of one length."""
    import torch
    case = expect(name)
    dev = devs(case)
    k, bases, offsets = case["k"], case["bases"], case["offsets"]
    d_bases, d_offsets = torch.from_numpy(np.array(bases)).cuda(), torch.from_numpy(np.array(offsets)).cuda()
    d_lut = torch.from_numpy(lut).cuda()
    _check(dev, path, case, lut, lambda t, rc: dev.map_reads(bases, offsets, k, also_revcomp=rc, lut=t), "map_reads, host")
    _check(dev, path, case, lut, lambda t, rc: dev.map_reads(d_bases, d_offsets, k, also_revcomp=rc, lut=t), "map_reads, device")
    _check(dev, path, case, lut, lambda t, rc: dev.map_reads(d_bases, d_offsets, k, also_revcomp=rc, lut=None if t is None else d_lut),
           "map_reads, device, table in HBM")
    # a base pointer that is not 16-byte aligned: the pre-pass loads unaligned vectors
    shifted = torch.empty(bases.shape[0] + 1, dtype=torch.uint8, device="cuda")
    shifted[1:] = d_bases
    _check(dev, path, case, lut, lambda t, rc: dev.map_reads(shifted[1:], d_offsets, k, also_revcomp=rc, lut=t), "map_reads, odd address")
    if name in ac.UNIFORM:
        n, L = case["n_reads"], int(offsets[1])
        _check(dev, path, case, lut, lambda t, rc: dev.map_reads_uniform(bases, n, L, k, also_revcomp=rc, lut=t), "uniform, host")
        _check(dev, path, case, lut, lambda t, rc: dev.map_reads_uniform(d_bases, n, L, k, also_revcomp=rc, lut=t), "uniform, device")
        before = dev.get_param("flat_uniform_batches")
        _run(dev, path, lambda: dev.map_reads_uniform(bases, n, L, k, lut=lut))
        _run(dev, path, lambda: dev.map_reads_uniform(d_bases, n, L, k, lut=lut))
        assert dev.get_param("flat_uniform_batches") == before     # (a break table: the ragged front end)


@pytest.mark.parametrize("path", [DIRECT, RADIX])
@pytest.mark.parametrize("fmt", [4, 2])
@pytest.mark.parametrize("name", ac.CASES)
def test_raw_records(kmm, expect, devs, lut, name, fmt, path):
    """kmm_map_records on FASTQ and two-line FASTA text of the same reads, host and device bytes; a break on the last byte
    of a 4 KiB compaction tile and on the first byte of the next, "\\r\\n" lines next to breaks."""
    import torch
    case = expect(name)
    dev = devs(case)
    k = case["k"]
    text, _, _ = ac.records_text(case["bases"], case["offsets"], lut, fmt)
    raw = np.frombuffer(text, np.uint8)
    d_raw = torch.from_numpy(raw.copy()).cuda()
    done = (len(text), case["n_reads"])
    _check(dev, path, case, lut, lambda t, rc: dev.map_records(raw, fmt=fmt, k=k, also_revcomp=rc, lut=t), "records, host", done)
    _check(dev, path, case, lut, lambda t, rc: dev.map_records(d_raw, fmt=fmt, k=k, also_revcomp=rc, lut=t), "records, device", done)
    if path == RADIX and name in ac.UNIFORM:
        # reads of one length: the default table takes the uniform front end of pass 1, a table with breaks in the data does not
        before = dev.get_param("flat_uniform_batches")
        if set(case["bases"].tobytes()) <= set(b"ACGTNacgtn"):
            _run(dev, path, lambda: dev.map_records(d_raw, fmt=fmt, k=k))
            assert dev.get_param("flat_uniform_batches") == before + 1
            before += 1
        _run(dev, path, lambda: dev.map_records(d_raw, fmt=fmt, k=k, lut=lut))
        assert dev.get_param("flat_uniform_batches") == before


def test_per_kmer_mode(kmm, expect, lut):
    case = expect("random_1_percent")
    want = numpy_entry_counts(np.asarray(case["index"]._kmers, dtype=np.uint64),
                              ac.surviving_kmers(case["bases"], case["offsets"], case["k"], lut))
    assert want.sum() > 0
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.count_kmers_mode()
        dev.map_reads(case["bases"], case["offsets"], case["k"], lut=lut)
        assert np.array_equal(dev.get_kmer_counts(), want)
        assert np.array_equal(dev.get_node_counts(), case["split"])


def _upper(case, oracle, lut):
    """The case as BAM stores it (no lower case): (reads, oracle's counts on the split reads, windows)."""
    bases = np.where((case["bases"] >= ord("a")) & (case["bases"] <= ord("z")), case["bases"] - 32, case["bases"]).astype(np.uint8)
    sb, so = ac.split_at_breaks(bases, case["offsets"], lut)
    counts, n = oracle.map_reads(case["index"], case["mx"], sb, so, case["k"])
    return [bases[case["offsets"][i]:case["offsets"][i + 1]].tobytes() for i in range(case["n_reads"])], counts, n


def _gzip_whole(dev, gz, k, table):
    """The caller's loop of kmm_map_gzip over one window that is the whole file: each call goes on where the one before
    stopped; the records mapped."""
    pos, total = 0, 0
    while pos < len(gz):
        used, n_rec = dev.map_gzip(gz[pos:], fmt=4, k=k, first=pos == 0, last=True, lut=table)
        assert used > 0
        pos += used
        total += n_rec
    return total


def test_compressed_and_alignment_formats(kmm, expect, devs, oracle, lut):
    """One case each through BGZF FASTQ, plain gzip FASTQ, SAM text (IUPAC letters in SEQ) and BAM (code 15 and the IUPAC
    codes); '=' is still not a nucleotide."""
    from kmer_mapper_amd import reads_io, _lib
    from kmer_mapper_amd.util import ReadBatch
    case = expect("tile_edges")
    dev = devs(case)
    k = case["k"]
    text, _, _ = ac.records_text(case["bases"], case["offsets"], lut, 4)
    bgzf = np.frombuffer(reads_io.bgzf_members(text, 0x8000) + reads_io.BGZF_EOF, np.uint8)
    for path in (DIRECT, RADIX):
        for table, want, n in ((lut, case["split"], case["n_windows"]), (None, case["n_to_a"], case["n_all"])):
            got, lookups, ret = _run(dev, path, lambda: dev.map_bgzf(bgzf, fmt=4, k=k, first=True, last=True, lut=table))
            assert ret == (len(bgzf), case["n_reads"])
            assert np.array_equal(got, want) and lookups == n, ("bgzf", path, table is None)
        gz = np.frombuffer(gzip.compress(text, 6), np.uint8)
        for table, want, n in ((lut, case["split"], case["n_windows"]), (None, case["n_to_a"], case["n_all"])):
            got, lookups, ret = _run(dev, path, lambda: _gzip_whole(dev, gz, k, table))
            assert ret == case["n_reads"]
            assert np.array_equal(got, want) and lookups == n, ("gzip", path, table is None)
    case = expect("lower_case_and_iupac")
    dev = devs(case)
    reads = [case["bases"][case["offsets"][i]:case["offsets"][i + 1]].tobytes() for i in range(case["n_reads"])]
    sam = np.frombuffer(reads_io.sam_text(ReadBatch.from_strings([r.decode() for r in reads])), np.uint8)
    up_reads, up_counts, up_n = _upper(case, oracle, lut)
    bam = np.frombuffer(reads_io.bgzf_members(reads_io.bam_header()) +
                        reads_io.bgzf_members(b"".join(reads_io.bam_record(r, b"r%d" % i) for i, r in enumerate(up_reads))) +
                        reads_io.BGZF_EOF, np.uint8)
    assert any(c in b"".join(up_reads) for c in b"MRSVWYHKDBN")
    for path in (DIRECT, RADIX):
        got, lookups, ret = _run(dev, path, lambda: dev.map_records(sam, fmt=_lib.FORMAT_SAM, k=k, lut=lut))
        assert ret == (len(sam), case["n_reads"])
        assert np.array_equal(got, case["split"]) and lookups == case["n_windows"], ("sam", path)
        got, lookups, ret = _run(dev, path, lambda: dev.map_bam(bam, first=True, last=True, k=k, lut=lut))
        assert ret == (len(bam), case["n_reads"])
        assert np.array_equal(got, up_counts) and lookups == up_n, ("bam", path)
    # the default table still refuses the IUPAC letters, and the skip table still refuses '='
    dev.reset()
    dev.map_bam(bam, first=True, last=True, k=k)
    with pytest.raises(ValueError, match="not a nucleotide"):
        dev.get_node_counts()
    dev.reset()
    bad = np.frombuffer(reads_io.bgzf_members(reads_io.bam_header()) +
                        reads_io.bgzf_members(reads_io.bam_record(b"ACGT" * 10 + b"N=" + b"ACGT" * 10)) + reads_io.BGZF_EOF, np.uint8)
    dev.map_bam(bad, first=True, last=True, k=k, lut=lut)
    with pytest.raises(ValueError, match="not a nucleotide"):
        dev.get_node_counts()
    dev.reset()


def test_refusals(kmm, expect, devs, lut):
    """k = 1 with a break table and kmm_extract_kmers with one are KMM_ERR_INVALID_ARG; the handle stays usable."""
    import torch
    case = expect("read_ends")
    dev = devs(case)
    bases, offsets = case["bases"], case["offsets"]
    text, _, _ = ac.records_text(bases, offsets, lut, 4)
    dev.reset()
    for table in (lut, torch.from_numpy(lut).cuda()):
        with pytest.raises(ValueError, match="k = 1"):
            dev.map_reads(bases, offsets, 1, lut=table)
        with pytest.raises(ValueError, match="k = 1"):
            dev.map_reads_uniform(bases, case["n_reads"], ac.L, 1, lut=table)
        with pytest.raises(ValueError, match="k = 1"):
            dev.map_records(np.frombuffer(text, np.uint8), fmt=4, k=1, lut=table)
        with pytest.raises(ValueError, match="break entry"):
            kmm.extract_kmers(bases, offsets, case["k"], lut=table)
    assert not dev.get_node_counts().any()
    no_break = lut.copy()
    no_break[no_break == 0xFE] = 0
    dev.map_reads(bases, offsets, 1, lut=no_break)                    # (k = 1 itself is fine)
    dev.reset()
    got, lookups, _ = _run(dev, 0, lambda: dev.map_reads(bases, offsets, case["k"], lut=lut))
    assert np.array_equal(got, case["split"]) and lookups == case["n_windows"]


@pytest.mark.parametrize("path", [DIRECT, RADIX])
def test_a_byte_outside_the_table_next_to_a_break_is_still_reported_with_its_offset(kmm, expect, devs, lut, path):
    case = expect("tile_edges")
    dev = devs(case)
    bases = np.array(case["bases"])
    at = 4097                                                          # (4096 holds a break)
    assert lut[bases[at - 1]] == 0xFE
    bases[at] = ord("!")
    dev.reset()
    dev.set_param("path", path)
    try:
        dev.map_reads(bases, case["offsets"], case["k"], lut=lut)
        with pytest.raises(ValueError, match="offset %d of a mapped chunk is not a nucleotide" % at):
            dev.get_node_counts()
        dev.reset()
        dev.map_reads_uniform(bases, case["n_reads"], ac.L, case["k"], lut=lut)
        with pytest.raises(ValueError, match="offset %d of a mapped chunk is not a nucleotide" % at):
            dev.get_node_counts()
        dev.reset()
        text, _, _ = ac.records_text(bases, case["offsets"], lut, 4)
        dev.map_records(np.frombuffer(text, np.uint8), fmt=4, k=case["k"], lut=lut)
        with pytest.raises(ValueError, match="offset %d of a mapped chunk is not a nucleotide" % text.index(b"!")):
            dev.get_node_counts()
    finally:
        dev.reset()
        dev.set_param("path", 0)


def test_cli_skips_ambiguous_bases(kmm, expect, lut, tmp_path):
    """`kmer_mapper map --ambiguous-bases skip` on a small FASTQ, and on its BGZF, writes the oracle's .npy; without the
    option the same file gives N read as A."""
    from kmer_mapper_amd import command_line_interface as cli
    from kmer_mapper_amd.gz_io import write_bgzf
    case = expect("random_1_percent")
    text, _, _ = ac.records_text(case["bases"], case["offsets"], lut, 4)
    fq, gz, idx = str(tmp_path / "reads.fq"), str(tmp_path / "reads.fq.gz"), str(tmp_path / "idx.npz")
    with open(fq, "wb") as f:
        f.write(text)
    write_bgzf(gz, text)
    case["index"].to_file(idx)
    for path, extra, want in ((fq, ["--ambiguous-bases", "skip"], case["split"]), (gz, ["--ambiguous-bases", "skip"], case["split"]),
                              (fq, [], case["n_to_a"]), (fq, ["--ambiguous-bases", "skip", "--host-parser"], case["split"])):
        out = str(tmp_path / "out")
        cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out] + extra)
        got = np.load(out + ".npy")
        assert np.array_equal(got[:len(want)], want) and not got[len(want):].any(), (path, extra)
