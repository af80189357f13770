"""GPU tests of kmm_map_bam (csrc/kmm_bam.hpp): BAM files — what `bnp.open(args.reads)` reads at the reference's
command_line_interface.py:102,109 — inflated on the GPU, their records found and decoded there; the node counts equal the
oracle's (oracle.map_reads) on the SEQ an independent pure-Python reader (gzip + struct, tests/test_bam_walk_on_the_cpu.py)
takes from the same bytes, bit for bit, and damaged files are refused with nothing mapped."""
import struct

import numpy as np
import pytest

from tests.test_bam_walk_on_the_cpu import read_bam

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def syn():
    from kmer_mapper_amd import synthetic
    return synthetic


def _bam(payload_header, records, block=0xFF00, level=6, eof=True):
    from kmer_mapper_amd import reads_io
    return (reads_io.bgzf_members(payload_header, block, level) + reads_io.bgzf_members(b"".join(records), block, level) +
            (reads_io.BGZF_EOF if eof else b""))


def _records(reads, flags=None, quals=None, auxs=None, names=None, ref_ids=None):
    from kmer_mapper_amd import reads_io
    return [reads_io.bam_record(r, names[i] if names else b"r%d" % i, flags[i] if flags else 4,
                                ref_id=ref_ids[i] if ref_ids else -1, qual=quals[i] if quals else None,
                                aux=auxs[i] if auxs else b"") for i, r in enumerate(reads)]


def _expect(oracle, index, mx, comp, k=31, excl=0, also_revcomp=False):
    """The oracle's counts on the SEQ the Python reader finds in `comp` (records with flag & excl left out)."""
    recs, _ = read_bam(comp)
    seqs = [s for f, s in recs if not f & excl]
    offs = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=offs[1:])
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    return oracle.map_reads(index, mx, bases, offs, k, also_revcomp=also_revcomp, n_threads=4)[0], len(seqs)


def _feed(dev, comp, step=1 << 40, hinted=False, k=31, also_revcomp=False):
    """The CLI's loop (command_line_interface._map_compressed_file): windows that END at fixed places (anywhere in a member), each
    call told which bytes follow when hinted; a first window inside the header is made longer."""
    buf = np.frombuffer(comp, dtype=np.uint8)
    size, pos, total = len(comp), 0, 0
    end = min(step, size)
    while pos < size:
        nxt = min(end + step, size)
        used, n_rec = dev.map_bam(buf[pos:end], first=pos == 0, last=end == size, k=k, also_revcomp=also_revcomp,
                                  next_chunk=buf[end:nxt] if (hinted and nxt > end) else None)
        if used == 0 and pos == 0 and end < size:
            end = nxt
            continue
        assert used > 0 or end < size
        pos += used
        total += n_rec
        if pos < end and end == size:
            continue
        end = nxt
    return total


def _known_answer_bam():
    """Three records laid out byte by byte (SAM/BAM specification 4.2), behind a header with one reference."""
    text = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100\n"
    header = b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", 1) + struct.pack("<I", 5) + b"chr1\x00" + \
        struct.pack("<I", 100)

    def rec(ref, pos, name, flag, cigar, l_seq, seq_bytes, qual, aux):
        body = struct.pack("<i", ref) + struct.pack("<i", pos) + bytes([len(name) + 1, 60]) + struct.pack("<H", 4680) + \
            struct.pack("<H", len(cigar)) + struct.pack("<H", flag) + struct.pack("<i", l_seq) + struct.pack("<iii", -1, -1, 0) + \
            name + b"\x00" + b"".join(struct.pack("<I", c) for c in cigar) + seq_bytes + qual + aux
        return struct.pack("<I", len(body)) + body
    # "ACGTNAC": A=1 C=2 G=4 T=8 N=15, high nibble first, the odd last base padded with 0
    r1 = rec(0, 10, b"first", 0, [(7 << 4) | 0], 7, bytes([0x12, 0x48, 0xF1, 0x20]), b"IIIIIII", b"NMC\x01XZZhello\x00")
    r2 = rec(-1, -1, b"empty", 4, [], 0, b"", b"", b"")                                    # SEQ "*"
    # "GGACGTT" on the reverse strand (flag 16): taken as stored
    r3 = rec(0, 20, b"third", 16, [(3 << 4) | 0, (1 << 4) | 1, (3 << 4) | 0], 7, bytes([0x44, 0x12, 0x48, 0x80]), b"\xff" * 7,
             b"RGZgrp1\x00")
    return header, [r1, r2, r3]


def test_known_answer(kmm, oracle):
    """k = 4: read 1 "ACGTNAC" (N -> A: ACGT CGTA GTAA TAAC), read 2 empty, read 3 "GGACGTT" (GGAC GACG ACGT CGTT).  Index:
    ACGT -> node 1, GTAA -> node 2, CGTT -> node 3, TTTT -> node 4.  By hand: node 1 twice, nodes 2 and 3 once, node 4 never."""
    words = [b"ACGT", b"GTAA", b"CGTT", b"TTTT"]
    km = np.array([int(oracle.extract(np.frombuffer(w, np.uint8), np.array([0, 4], np.int64), 4)[0]) for w in words], np.uint64)
    index = oracle.build_index(km, np.array([1, 2, 3, 4], np.int64), 13)
    header, recs = _known_answer_bam()
    comp = _bam(header, recs)
    assert [s for _, s in read_bam(comp)[0]] == [b"ACGTNAC", b"", b"GGACGTT"]
    with kmm.DeviceIndex.from_index(index, 4) as dev:
        for path in (0, 1):
            dev.set_param("path", path)
            dev.reset()
            used, n = dev.map_bam(np.frombuffer(comp, np.uint8), first=True, last=True, k=4)
            assert used == len(comp) and n == 3
            assert dev.get_node_counts().tolist() == [0, 2, 1, 1, 0]
        assert dev.get_param("bam_header_bytes") > 0


@pytest.mark.parametrize("k", [5, 16, 31])
def test_ragged_short_and_uniform_reads(kmm, syn, oracle, k):
    index, genome = syn.make_index(20000, k=k, seed=801)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 6000, 0, 300, seed=802)
    ragged = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    ragged[:40] = [r[:k - 1] for r in ragged[:40]]                      # shorter than k
    bases, offs = syn.make_reads(genome, 8000, 150, seed=803)
    uniform = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    from kmer_mapper_amd import reads_io
    for reads in (ragged, uniform):
        comp = _bam(reads_io.bam_header(), _records(reads))
        for revcomp in (False, True):
            expect, n = _expect(oracle, index, mx, comp, k, also_revcomp=revcomp)
            with kmm.DeviceIndex.from_index(index, mx) as dev:
                for path in (0, 1, 2):
                    if path == 2 and not dev.get_param("radix_available"):
                        continue
                    dev.set_param("path", path)
                    dev.reset()
                    u0 = dev.get_param("flat_uniform_batches")
                    assert _feed(dev, comp, k=k, also_revcomp=revcomp) == n
                    assert np.array_equal(dev.get_node_counts(), expect), (path, revcomp)
                    if path == 2:
                        assert (dev.get_param("flat_uniform_batches") > u0) == (reads is uniform)


def test_per_kmer_mode(kmm, syn, oracle):
    """Per-k-mer counting ("count_kmers"): the index entries' counts from kmm_map_bam equal those of the same reads as FASTA."""
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(20000, seed=811)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 4000, 0, 250, seed=812)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    comp = _bam(reads_io.bam_header(), _records(reads))
    expect, _ = _expect(oracle, index, mx, comp)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.count_kmers_mode(True)
        _feed(dev, comp, step=50_000)
        got_k = dev.get_kmer_counts().copy()
        assert np.array_equal(dev.get_node_counts(), expect)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.count_kmers_mode(True)
        raw = np.frombuffer(b"".join(b">\n" + r + b"\n" for r in reads), np.uint8)
        dev.map_records(raw, len(raw), 2 | 0x100, 31)
        assert got_k.any() and np.array_equal(got_k, dev.get_kmer_counts())


def test_stream_cutting_long_headers_long_reads_and_hints(kmm, syn, oracle):
    """A header of > 64 KiB (5000 references) over several members, reads of > 200 kb over many members and tiles, short
    reads between them; windows that end anywhere (records and the header straddle calls), announced ahead or not, small
    members: the oracle's counts, every record once, nothing carried at the end."""
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(100000, seed=821)
    mx = index.max_node_id()
    rng = np.random.default_rng(822)
    bases, offs = syn.make_ragged_reads(genome, 3000, 0, 300, seed=823)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    for j, L in enumerate((210_000, 260_000, 330_000)):
        long_read = syn.make_reads(genome, 1, L, seed=824 + j)[0].tobytes()
        reads.insert(int(rng.integers(0, len(reads))), long_read)
    refs = [(b"contig_%05d_with_a_long_name" % i, 1000 + i) for i in range(5000)]
    header = reads_io.bam_header(refs, b"@HD\tVN:1.6\n" + b"@CO\tpadding\n" * 200)
    assert len(header) > 65536
    ref_ids = [int(x) for x in rng.integers(-1, 5000, size=len(reads))]
    for block in (0xFF00, 7000):
        comp = _bam(header, _records(reads, ref_ids=ref_ids), block=block)
        expect, n = _expect(oracle, index, mx, comp)
        with kmm.DeviceIndex.from_index(index, mx) as dev:
            for step, hinted in ((1 << 40, False), (150_001, False), (150_001, True), (40_000, True), (65_537, False)):
                dev.reset()
                before = dev.get_param("bgzf_prestaged_calls")
                assert _feed(dev, comp, step, hinted) == n, (block, step, hinted)
                assert np.array_equal(dev.get_node_counts(), expect), (block, step, hinted)
                assert dev.get_param("bgzf_carry_bytes") == 0
                if hinted:
                    assert dev.get_param("bgzf_prestaged_calls") > before


def test_false_starts(kmm, syn, oracle):
    """Read names, qualities and aux fields that hold whole records (chains of them): speculative starts are found there,
    rejected by the link check, and the counts stay exact."""
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(20000, seed=831)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 5000, 20, 250, seed=832)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    decoy = reads_io.bam_record(b"ACGTACGTAC" * 3, b"decoy", 0) * 5
    quals = [(decoy * 3)[:len(r)] for r in reads]
    auxs = [b"ZZZ" + decoy + b"\x00" if i % 2 == 0 else b"" for i in range(len(reads))]
    names = [b"n" + decoy[:200].replace(b"\x00", b"\x01") if i % 5 == 0 else b"r%d" % i for i in range(len(reads))]
    comp = _bam(reads_io.bam_header(), _records(reads, quals=quals, auxs=auxs, names=names))
    expect, n = _expect(oracle, index, mx, comp)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        assert _feed(dev, comp, 100_000) == n
        assert np.array_equal(dev.get_node_counts(), expect)
        assert dev.get_param("bam_false_starts") > 0 and dev.get_param("bam_continuations") > 0


def test_flag_filter(kmm, syn, oracle):
    """"bam_exclude_flags" = 0x900 drops exactly the secondary and supplementary records; the default maps every record."""
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(20000, seed=841)
    mx = index.max_node_id()
    bases, offs = syn.make_reads(genome, 6000, 150, seed=842)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    rng = np.random.default_rng(843)
    flags = [int(f) for f in rng.choice([0, 16, 99, 147, 256, 272, 2048, 2064, 4], size=len(reads))]
    comp = _bam(reads_io.bam_header([(b"chr1", 10 ** 6)]), _records(reads, flags=flags, ref_ids=[0] * len(reads)))
    all_, n_all = _expect(oracle, index, mx, comp)
    prim, n_prim = _expect(oracle, index, mx, comp, excl=0x900)
    assert n_prim < n_all
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        assert dev.get_param("bam_exclude_flags") == 0
        assert _feed(dev, comp, 200_000) == n_all
        assert np.array_equal(dev.get_node_counts(), all_)
        dev.reset()
        dev.set_param("bam_exclude_flags", 0x900)
        assert _feed(dev, comp, 200_000) == n_prim
        assert np.array_equal(dev.get_node_counts(), prim)
        assert dev.get_param("bam_records_excluded") == n_all - n_prim


def test_refusals_leave_nothing_mapped_and_the_handle_usable(kmm, syn, oracle):
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(8000, seed=851)
    mx = index.max_node_id()
    bases, offs = syn.make_reads(genome, 3000, 150, seed=852)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    hdr = reads_io.bam_header()
    recs = _records(reads)
    good = _bam(hdr, recs)
    expect, n = _expect(oracle, index, mx, good)
    bad_size = list(recs)
    bad_size[1500] = struct.pack("<I", 40) + bad_size[1500][4:]              # block_size too small for its fields
    cut = b"".join(recs)
    comp_damaged = bytearray(_bam(hdr, recs))
    comp_damaged[len(comp_damaged) // 2] ^= 0x55                             # inside a member: Huffman data or CRC32
    cases = {
        "magic": _bam(b"BAM\x02" + hdr[4:], recs),
        "block_size": _bam(hdr, bad_size),
        "ends inside a record": reads_io.bgzf_members(hdr) + reads_io.bgzf_members(cut[:-100]) + reads_io.BGZF_EOF,
        "ends inside a member": _bam(hdr, recs, eof=False)[:-30],
        "damaged member": bytes(comp_damaged),
    }
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        for name, comp in cases.items():
            dev.reset()
            with pytest.raises(ValueError):
                _feed(dev, comp, step=1 << 40)
            assert not dev.get_node_counts().any(), name
            assert _feed(dev, good, 100_000) == n
            assert np.array_equal(dev.get_node_counts(), expect), name


def test_invalid_base(kmm, syn):
    """An IUPAC code in SEQ (R) is KMM_ERR_INVALID_BASE, as the same letter in a FASTQ."""
    from kmer_mapper_amd import reads_io
    index, _ = syn.make_index(2000, seed=861)
    comp = _bam(reads_io.bam_header(), _records([b"ACGT" * 20, b"ACGTRACGT" * 5, b"ACGT" * 10]))
    with kmm.DeviceIndex.from_index(index, index.max_node_id()) as dev:
        dev.map_bam(np.frombuffer(comp, np.uint8), first=True, last=True)
        with pytest.raises(ValueError, match="not a nucleotide"):
            dev.get_node_counts()


def test_cli_writes_the_oracles_npy(kmm, syn, oracle, tmp_path):
    """`kmer_mapper map -i idx.npz -f x.bam -o out` (x.bam written by reads_io.write_bam) saves the oracle's counts."""
    from kmer_mapper_amd import command_line_interface as cli, reads_io
    from kmer_mapper_amd.util import ReadBatch
    index, genome = syn.make_index(20000, seed=871)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 20000, 0, 300, seed=872)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    path = str(tmp_path / "x.bam")
    reads_io.write_bam(path, ReadBatch.from_strings([r.decode() for r in reads]))
    expect, _ = _expect(oracle, index, mx, open(path, "rb").read())
    index.to_file(str(tmp_path / "idx.npz"))
    cli.run_argument_parser(["map", "-i", str(tmp_path / "idx.npz"), "-f", path, "-o", str(tmp_path / "out")])
    got = np.load(str(tmp_path / "out.npy"))
    assert np.array_equal(got[:len(expect)], expect) and not got[len(expect):].any()


def _feed_cuts(dev, comp, cuts, bam, fmt=None):
    """Windows that end at `cuts` (the last one = the file's end), each call told the next window's bytes (the CLI's loop)."""
    buf = np.frombuffer(comp, np.uint8)
    size, pos, total, i = len(buf), 0, 0, 0
    while pos < size:
        end = cuts[i]
        nxt = cuts[i + 1] if i + 1 < len(cuts) else end
        kw = dict(first=pos == 0, last=end == size, next_chunk=buf[end:nxt] if nxt > end else None)
        used, n_rec = dev.map_bam(buf[pos:end], **kw) if bam else dev.map_bgzf(buf[pos:end], fmt=fmt, **kw)
        assert used > 0
        pos += used
        total += n_rec
        if i + 1 < len(cuts):        # (as the CLI: the next window ends at the next cut, and starts where this call stopped)
            i += 1
    return total


def test_prestaged_window_at_the_call_cap_then_a_prestaged_last_window(kmm, syn, oracle):
    """A window staged ahead whose member chain reaches the (lowered) call cap, then small windows staged ahead, the last one
    included: the last call keeps its KMM_FORMAT_LAST_CHUNK handling (a FASTQ whose last line has no newline keeps its last
    read, a truncated BAM is refused) — the cap of an earlier staged window is not taken over by the later ones."""
    from kmer_mapper_amd import _lib, reads_io
    index, genome = syn.make_index(20000, seed=881)
    mx = index.max_node_id()
    bases, offs = syn.make_reads(genome, 6000, 150, seed=882)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    fq = b"".join(b"@r\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for r in reads)[:-1]       # no final newline
    expect_fq = oracle.map_reads(index, mx, bases, offs, 31, n_threads=4)[0]
    comp_fq = reads_io.bgzf_members(fq, 16000) + reads_io.BGZF_EOF
    comp_bam = _bam(reads_io.bam_header(), _records(reads), block=16000)
    expect_bam, n_bam = _expect(oracle, index, mx, comp_bam)
    trunc = reads_io.bgzf_members(reads_io.bam_header(), 16000) + reads_io.bgzf_members(b"".join(_records(reads))[:-50], 16000)

    def cuts(size):        # a large window (its chain cut at the cap when it is staged), then windows far below the cap
        return [20_000, size // 2] + list(range(size // 2 + 8_000, size, 8_000)) + [size]

    with kmm.DeviceIndex.from_index(index, mx) as dev:
        dev.set_param("debug_bgzf_call_cap_kb", 128)
        before = dev.get_param("bgzf_prestaged_calls")
        assert _feed_cuts(dev, comp_fq, cuts(len(comp_fq)), False, _lib.FORMAT_FASTQ) == len(reads)
        assert np.array_equal(dev.get_node_counts(), expect_fq)
        assert dev.get_param("bgzf_prestaged_calls") - before >= 5
        dev.reset()
        assert _feed_cuts(dev, comp_bam, cuts(len(comp_bam)), True) == n_bam
        assert np.array_equal(dev.get_node_counts(), expect_bam)
        dev.reset()
        with pytest.raises(ValueError):
            _feed_cuts(dev, trunc, cuts(len(trunc)), True)
        dev.set_param("debug_bgzf_call_cap_kb", 0)


def test_a_gigabyte_of_bam(kmm, syn, oracle):
    """~1 GB of inflated BAM (150 bp reads, names, qualities) in windows of 96 MB announced ahead: several calls and the carry
    between them; the counts are the oracle's on one block of reads times the repetitions."""
    from concurrent.futures import ThreadPoolExecutor
    from kmer_mapper_amd import reads_io
    index, genome = syn.make_index(200000, seed=891)
    mx = index.max_node_id()
    bases, offs = syn.make_reads(genome, 20000, 150, seed=892)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    block = b"".join(reads_io.bam_record(r, b"SRR000001.%d" % i, 4, qual=bytes(np.random.default_rng(i).integers(33, 74, len(r), np.uint8)))
                     for i, r in enumerate(reads))
    reps = (1 << 30) // len(block) + 1
    payload = memoryview(reads_io.bam_header() + block * reps)
    with ThreadPoolExecutor(16) as pool:                          # (zlib releases the GIL)
        comp = b"".join(pool.map(lambda p: reads_io.bgzf_members(bytes(payload[p:p + 0xFF00]), 0xFF00, 1),
                                 range(0, len(payload), 0xFF00))) + reads_io.BGZF_EOF
    one = oracle.map_reads(index, mx, bases, offs, 31, n_threads=8)[0]
    expect = ((one.astype(np.uint64) * reps) % (1 << 32)).astype(np.uint32)
    with kmm.DeviceIndex.from_index(index, mx) as dev:
        assert _feed(dev, comp, 96 << 20, hinted=True) == reps * len(reads)
        assert np.array_equal(dev.get_node_counts(), expect)
        assert dev.get_param("bam_calls") >= 3
