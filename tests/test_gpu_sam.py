"""GPU tests of KMM_FORMAT_SAM (csrc/kmm_sam.hpp): SAM text — what `bnp.open(args.reads)` reads at the reference's
command_line_interface.py:102,109 — its lines parsed on the GPU and the SEQ column mapped, plain (kmm_map_records), BGZF
(kmm_map_bgzf) and gzip (kmm_map_gzip).  The node counts equal the oracle's (oracle.map_reads) on the SEQ an independent
pure-Python reader (tests/test_sam_on_the_cpu.py) takes from the same bytes, bit for bit; malformed files are refused with
nothing mapped."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_sam_on_the_cpu import random_sam, read_sam

pytestmark = pytest.mark.gpu

SAM = 8


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    assert _lib.FORMAT_SAM == SAM
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def syn():
    from kmer_mapper_amd import synthetic
    return synthetic


def _expect(oracle, index, mx, data, k=31, excl=0, also_revcomp=False):
    """The oracle's counts on the SEQ the Python reader finds in the SAM bytes `data` (records with flag & excl left out)."""
    recs, _ = read_sam(data)
    seqs = [s for f, s in recs if not f & excl]
    offs = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    return oracle.map_reads(index, mx, bases, offs, k, also_revcomp=also_revcomp, n_threads=4)[0], len(seqs)


def _feed(dev, data, chunk=1 << 40, k=31, also_revcomp=False):
    """The CLI's loop over a plain file (map_gpu_raw): chunks of `chunk` bytes, the bytes behind a chunk's last newline carried
    into the next one, a last line without newline given one."""
    pos, total = 0, 0
    while pos < len(data):
        end = min(pos + chunk, len(data))
        win = data[pos:end]
        if end == len(data) and not win.endswith(b"\n"):
            win += b"\n"
        used, n = dev.map_records(np.frombuffer(win, np.uint8), fmt=SAM, k=k, also_revcomp=also_revcomp)
        if used == 0:
            assert end < len(data)
            chunk *= 2                              # a line longer than the chunk
            continue
        pos += used
        total += n
    return total


def _sam(reads, **kw):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    return reads_io.sam_text(ReadBatch.from_strings([r.decode() for r in reads]), **kw)


def _split(bases, offs):
    return [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]


def test_known_answer(kmm, oracle):
    """k = 4: read 1 "ACGTNAC" (N -> A: ACGT CGTA GTAA TAAC), read 2 "*", read 3 "GGACGTT" (GGAC GACG ACGT CGTT), one record
    excluded by nothing, header lines in front and between.  Index: ACGT -> 1, GTAA -> 2, CGTT -> 3, TTTT -> 4.  By hand:
    node 1 twice, nodes 2 and 3 once, node 4 never."""
    words = [b"ACGT", b"GTAA", b"CGTT", b"TTTT"]
    km = np.array([int(oracle.extract(np.frombuffer(w, np.uint8), np.array([0, 4], np.int64), 4)[0]) for w in words], np.uint64)
    index = oracle.build_index(km, np.array([1, 2, 3, 4], np.int64), 13)
    data = (b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100\n"
            b"read1\t0\tchr1\t5\t60\t7M\t*\t0\t0\tACGTNAC\tIIIIIII\tNM:i:1\tMD:Z:4A2\n"
            b"read2\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
            b"@CO\ta comment between records\n"
            b"read3\t16\tchr1\t20\t60\t7M\t*\t0\t0\tGGACGTT\t*\r\n")
    assert [s for _, s in read_sam(data)[0]] == [b"ACGTNAC", b"", b"GGACGTT"]
    with kmm.DeviceIndex.from_index(index, 4) as dev:
        for path in (0, 1):
            dev.set_param("path", path)
            dev.reset()
            used, n = dev.map_records(np.frombuffer(data, np.uint8), fmt=SAM, k=4)
            assert used == len(data) and n == 3
            assert dev.get_node_counts().tolist() == [0, 2, 1, 1, 0]
        assert dev.get_param("sam_header_lines") == 6 and dev.get_param("sam_records") == 6
        assert dev.get_param("sam_calls") == 2


@pytest.mark.parametrize("k", [5, 16, 31])
def test_ragged_and_uniform_reads(kmm, syn, oracle, k):
    index, genome = syn.make_index(20000, k=k, seed=901)
    mx = index.max_node_id()
    ragged = _split(*syn.make_ragged_reads(genome, 6000, 0, 300, seed=902))
    ragged[:40] = [r[:k - 1] for r in ragged[:40]]                      # shorter than k
    uniform = _split(*syn.make_reads(genome, 8000, 150, seed=903))
    rng = np.random.default_rng(904)
    for reads in (ragged, uniform):
        data = random_sam(rng, reads, flags=[0] * len(reads), crlf=reads is uniform)
        for revcomp in (False, True):
            expect, n = _expect(oracle, index, mx, data, k, also_revcomp=revcomp)
            with kmm.DeviceIndex.from_index(index, mx) as dev:
                for path in (0, 1, 2):
                    if path == 2 and not dev.get_param("radix_available"):
                        continue
                    dev.set_param("path", path)
                    dev.reset()
                    assert _feed(dev, data, k=k, also_revcomp=revcomp) == n
                    assert np.array_equal(dev.get_node_counts(), expect), (path, revcomp)


def test_per_kmer_mode(kmm, syn, oracle):
    """Per-k-mer counting ("count_kmers"): the index entries' counts from SAM equal those of the same reads as FASTA."""
    index, genome = syn.make_index(20000, seed=911)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 4000, 0, 250, seed=912))
    data = _sam(reads)
    expect, _ = _expect(oracle, index, mx, data)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.count_kmers_mode(True)
        _feed(dev, data, chunk=50_000)
        got_k = dev.get_kmer_counts().copy()
        assert np.array_equal(dev.get_node_counts(), expect)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.count_kmers_mode(True)
        raw = np.frombuffer(b"".join(b">\n" + r + b"\n" for r in reads), np.uint8)
        dev.map_records(raw, len(raw), 2 | 0x100, 31)
        assert got_k.any() and np.array_equal(got_k, dev.get_kmer_counts())


def test_small_chunks_cut_mid_line_and_a_200kb_seq(kmm, syn, oracle):
    index, genome = syn.make_index(20000, seed=921)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 3000, 0, 200, seed=922))
    long_read = b"".join(_split(*syn.make_reads(genome, 1400, 150, seed=923)))[:200_000]
    reads = reads[:1500] + [long_read] + reads[1500:]
    data = random_sam(np.random.default_rng(924), reads)
    data = data[:-1]                                                    # a last line without its newline
    expect, n = _expect(oracle, index, mx, data)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        for chunk in (3000, 7777, 1 << 20, 1 << 40):
            dev.reset()
            assert _feed(dev, data, chunk=chunk) == n
            assert np.array_equal(dev.get_node_counts(), expect), chunk


def test_a_chunk_for_the_radix_path(kmm, syn, oracle):
    index, genome = syn.make_index(50000, seed=931)
    mx = index.max_node_id()
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        if not dev.get_param("radix_available"):
            pytest.skip("no radix path on this device")
        n_reads = int(dev.get_param("radix_min_units") * 1.5 / 150) + 1000
        bases, offs = syn.make_reads(genome, n_reads, 150, seed=932)
        data = _sam(_split(bases, offs))
        expect = oracle.map_reads(index, mx, bases, offs, 31, n_threads=8)[0]
        r0 = dev.get_param("radix_batches")
        used, n = dev.map_records(np.frombuffer(data, np.uint8), fmt=SAM)
        assert used == len(data) and n == n_reads
        assert dev.get_param("radix_batches") > r0
        assert np.array_equal(dev.get_node_counts(), expect)


def test_same_reads_as_bam_and_as_sam(kmm, syn, oracle, tmp_path):
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    index, genome = syn.make_index(20000, seed=941)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 5000, 0, 300, seed=942))
    batch = ReadBatch.from_strings([r.decode() for r in reads])
    flags = [0x900 if i % 7 == 0 else 4 for i in range(len(reads))]
    reads_io.write_bam(str(tmp_path / "x.bam"), batch, flags=flags)
    reads_io.write_sam(str(tmp_path / "x.sam"), batch, flags=flags)
    comp = np.fromfile(str(tmp_path / "x.bam"), np.uint8)
    data = open(str(tmp_path / "x.sam"), "rb").read()
    for excl in (0, 0x900):
        with kmm.DeviceIndex.from_index(index, mx) as dev:
            dev.set_param("bam_exclude_flags", excl)
            _, n_bam = dev.map_bam(comp, first=True, last=True)
            c_bam = dev.get_node_counts().copy()
            dev.reset()
            n_sam = _feed(dev, data)
            assert n_sam == n_bam and np.array_equal(dev.get_node_counts(), c_bam), excl
            assert np.array_equal(c_bam, _expect(oracle, index, mx, data, excl=excl)[0])


def test_bgzf_sam_with_a_small_call_cap_and_hints(kmm, syn, oracle):
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(20000, seed=951)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 20000, 0, 300, seed=952))
    data = random_sam(np.random.default_rng(953), reads)
    comp = reads_io.bgzf_members(data, block=20000) + reads_io.BGZF_EOF
    expect, n = _expect(oracle, index, mx, data)
    buf = np.frombuffer(comp, np.uint8)
    size = len(buf)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        for cap_kb, step in ((0, 1 << 40), (300, 1 << 40), (200, 150_000)):
            dev.reset()
            dev.set_param("debug_bgzf_call_cap_kb", cap_kb)
            pos, total, end = 0, 0, min(step, size)
            while pos < size:                                    # (the CLI's loop: windows end at fixed places, hinted)
                nxt = min(end + step, size)
                used, n_rec = dev.map_bgzf(buf[pos:end], fmt=SAM, first=pos == 0, last=end == size,
                                           next_chunk=buf[end:nxt] if nxt > end else None)
                assert used > 0
                pos += used
                total += n_rec
                if pos < end and end == size:
                    continue
                end = nxt
            assert total == n and np.array_equal(dev.get_node_counts(), expect), cap_kb
        dev.set_param("debug_bgzf_call_cap_kb", 0)


def test_plain_gzip_sam(kmm, syn, oracle):
    index, genome = syn.make_index(20000, seed=961)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 12000, 0, 300, seed=962))
    data = random_sam(np.random.default_rng(963), reads)[:-1]       # (no final newline)
    comp = np.frombuffer(gzip.compress(data, 6), np.uint8)
    expect, n = _expect(oracle, index, mx, data)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.set_param("debug_gzip_chunk_kb", 2)
        pos, total = 0, 0
        while pos < len(comp):
            used, n_rec = dev.map_gzip(comp[pos:], fmt=SAM, first=pos == 0, last=True)
            assert used > 0
            pos += used
            total += n_rec
        assert total == n and np.array_equal(dev.get_node_counts(), expect)


def test_flag_filter_and_counters(kmm, syn, oracle):
    index, genome = syn.make_index(20000, seed=971)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 4000, 0, 250, seed=972))
    rng = np.random.default_rng(973)
    flags = [int(f) for f in rng.choice([0, 4, 16, 256, 2048, 256 | 16, 1 | 64], size=len(reads))]
    data = random_sam(rng, reads, flags=flags)
    _, hdr = read_sam(data)
    expect, n = _expect(oracle, index, mx, data, excl=0x900)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.set_param("bam_exclude_flags", 0x900)
        assert _feed(dev, data, chunk=40_000) == n
        assert np.array_equal(dev.get_node_counts(), expect)
        assert dev.get_param("sam_records") == n
        assert dev.get_param("sam_records_excluded") == sum(1 for f in flags if f & 0x900) == len(reads) - n
        assert dev.get_param("sam_header_lines") == hdr and dev.get_param("sam_calls") >= 2


def test_refusals_leave_nothing_mapped_and_the_handle_usable(kmm, syn, oracle):
    index, genome = syn.make_index(8000, seed=981)
    mx = index.max_node_id()
    reads = _split(*syn.make_reads(genome, 3000, 150, seed=982))
    good = _sam(reads)
    expect, n = _expect(oracle, index, mx, good)
    mid = good.index(b"\n", len(good) // 2) + 1
    cases = {
        "fields": b"r\t0\t*\t0\t0\t*\t*\t0\t0\tACGT\n",
        "flag": b"r\t65536\t*\t0\t0\t*\t*\t0\t0\tACGT\tIIII\n",
        "empty": b"\n",
    }
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        for name, bad in cases.items():
            dev.reset()
            data = good[:mid] + bad + good[mid:]
            with pytest.raises(ValueError, match="SAM line at byte %d" % mid):
                dev.map_records(np.frombuffer(data, np.uint8), fmt=SAM)
            assert not dev.get_node_counts().any(), name
            assert _feed(dev, good, 100_000) == n
            assert np.array_equal(dev.get_node_counts(), expect), name
        dev.reset()
        data = good[:mid] + b"r\t0\t*\t0\t0\t*\t*\t0\t0\tACG=T\tIIIII\n" + good[mid:]
        dev.map_records(np.frombuffer(data, np.uint8), fmt=SAM)
        with pytest.raises(ValueError, match="not a nucleotide"):
            dev.get_node_counts()
        dev.reset()
        assert _feed(dev, good) == n
        assert np.array_equal(dev.get_node_counts(), expect)


def test_header_only_file(kmm, syn):
    index, _ = syn.make_index(2000, seed=991)
    data = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:c%d\tLN:100\n" % i for i in range(5000))
    with kmm.DeviceIndex.from_index(index, index.max_node_id()) as dev:
        assert _feed(dev, data, chunk=30_000) == 0
        assert not dev.get_node_counts().any()
        assert dev.get_param("sam_records") == 0 and dev.get_param("sam_header_lines") == 5001


def _cli_npy(tmp_path, idx, path, name, extra=()):
    from kmer_mapper_amd import command_line_interface as cli
    out = str(tmp_path / name)
    cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out, "-c", "200000", *extra])
    return np.load(out + ".npy")


def test_cli_writes_the_oracles_npy(kmm, syn, oracle, tmp_path, monkeypatch):
    """`kmer_mapper map -f x.sam | x.sam.gz` (plain, BGZF, gzip on the host and on the GPU), --exclude-flags 0x900: the oracle's
    counts; the same reads as FASTQ and BAM give the same .npy."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.util import ReadBatch
    index, genome = syn.make_index(20000, seed=1001)
    mx = index.max_node_id()
    reads = _split(*syn.make_ragged_reads(genome, 20000, 0, 300, seed=1002))
    batch = ReadBatch.from_strings([r.decode() for r in reads])
    flags = [0x100 if i % 5 == 0 else 4 for i in range(len(reads))]
    idx = str(tmp_path / "idx.npz")
    index.to_file(idx)
    p = {"sam": str(tmp_path / "x.sam"), "bgzf": str(tmp_path / "b.sam.gz"), "gz": str(tmp_path / "g.sam.gz")}
    reads_io.write_sam(p["sam"], batch, flags=flags)
    reads_io.write_sam(p["bgzf"], batch, flags=flags, bgzf=True)
    reads_io.write_sam(p["gz"], batch, flags=flags, gz=True)
    reads_io.write_fastq(str(tmp_path / "x.fq"), batch)
    reads_io.write_bam(str(tmp_path / "x.bam"), batch)
    data = open(p["sam"], "rb").read()
    expect, _ = _expect(oracle, index, mx, data)
    expect_x, _ = _expect(oracle, index, mx, data, excl=0x900)
    fq = _cli_npy(tmp_path, idx, str(tmp_path / "x.fq"), "o_fq")
    bam = _cli_npy(tmp_path, idx, str(tmp_path / "x.bam"), "o_bam")
    assert np.array_equal(fq[:len(expect)], expect) and np.array_equal(fq, bam)
    for name, path in p.items():
        assert np.array_equal(_cli_npy(tmp_path, idx, path, "o_" + name), fq), name
        got = _cli_npy(tmp_path, idx, path, "x_" + name, ("--exclude-flags", "0x900"))
        assert np.array_equal(got[:len(expect_x)], expect_x) and not got[len(expect_x):].any(), name
    monkeypatch.setenv("KMM_CLI_GPU_GUNZIP", "1")
    assert np.array_equal(_cli_npy(tmp_path, idx, p["gz"], "o_gpugz"), fq)


def test_two_rank_gloo_rehearsal(tmp_path):
    """Two ranks on the box's one GPU (the reduce over gloo), each process under its own time limit: a plain SAM file split by
    byte ranges, a BGZF one by member ranges, a gzip one by chunk round-robin — the one-rank counts (tools/sam_two_rank_rehearsal.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tools", "sam_two_rank_rehearsal.py")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, script, "--prepare", str(tmp_path)], cwd=root,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    env = dict(os.environ, KMM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", WORLD_SIZE="2")
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, script, str(tmp_path)], cwd=root,
                              env=dict(env, RANK=str(i), LOCAL_RANK=str(i)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for i in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    assert outs[0].count("SAME AS ONE RANK") == 3 and "DIFFERS" not in outs[0], outs[0][-2000:]
