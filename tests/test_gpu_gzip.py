"""GPU tests of kmm_map_gzip (csrc/kmm_gpu_gunzip.hpp): PLAIN gzip streams — what `gzip reads.fq` writes, the most common
form of the .fq.gz the reference's Readme.md:11 names — inflated on the GPU from speculative block starts and parsed there;
the node counts equal the oracle's on the reads, and damaged streams are refused with nothing mapped."""
import gzip
import logging
import os
import subprocess
import zlib

import numpy as np
import pytest

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


def _fastq(reads, rng, names=None):
    return b"".join(b"@" + (names[i] if names else b"read%d some text" % i) + b"\n" + r + b"\n+\n" +
                    bytes(rng.choice(np.frombuffer(b"FFFF:,#@+I", dtype=np.uint8), size=len(r))) + b"\n" for i, r in enumerate(reads))


def _gzip(data, level=6, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem, strategy)
    return c.compress(data) + c.flush()


def _feed(dev, comp, fmt=4, k=31, cuts=None, revcomp=False):
    """The caller's loop: windows that end at `cuts` (None: one window), each call going on where the one before stopped."""
    from kmer_mapper_amd import _lib
    buf = np.frombuffer(comp, dtype=np.uint8)
    size = len(comp)
    ends = sorted(set([c for c in (cuts or []) if 0 < c < size] + [size]))
    pos, total = 0, 0
    for end in ends:
        while pos < end:
            used, n_rec = dev.map_gzip(buf[pos:end], fmt=fmt, k=k, first=pos == 0, last=end == size, also_revcomp=revcomp)
            total += n_rec
            assert 0 <= used <= end - pos
            pos += used
            if used == 0 or end < size:
                break
    assert pos == size
    return total


@pytest.fixture(scope="module")
def case(syn, oracle):
    index, genome = syn.make_index(20000, seed=901)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 12000, 30, 260, seed=902)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    expect, _ = oracle.map_reads(index, mx, bases, offs, 31, n_threads=4)
    expect_rc, _ = oracle.map_reads(index, mx, bases, offs, 31, also_revcomp=True, n_threads=4)
    raw = _fastq(reads, np.random.default_rng(903))
    return dict(index=index, mx=mx, reads=reads, expect=expect, expect_rc=expect_rc, raw=raw, bases=bases, offs=offs)


@pytest.mark.parametrize("level", [1, 6, 9])
def test_plain_gzip_inflated_on_the_gpu_gives_the_oracles_counts(kmm, case, level):
    """FASTQ as `gzip -<level>` writes it, fed whole and with the chunk search every 1 KiB (hundreds of chunks): the oracle's
    counts, the record count, one member; with -r the oracle's reverse-complement counts."""
    comp = _gzip(case["raw"], level)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        assert _feed(dev, comp) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect"])
        assert dev.get_param("gzip_members") == 1
        dev.reset()
        dev.set_param("debug_gzip_chunk_kb", 1)
        c0 = dev.get_param("gzip_chunks")
        assert _feed(dev, comp) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect"])
        assert dev.get_param("gzip_chunks") - c0 > 40                    # (about one chunk per deflate block)
        dev.reset()
        assert _feed(dev, comp, revcomp=True) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect_rc"])


def test_per_kmer_mode(kmm, case):
    """Per-k-mer counting ("count_kmers"): the index entries' counts from kmm_map_gzip equal those from the raw bytes mapped
    by kmm_map_records, and the node counts the oracle's."""
    comp = _gzip(case["raw"], 6)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.count_kmers_mode(True)
        dev.set_param("debug_gzip_chunk_kb", 2)
        assert _feed(dev, comp) == len(case["reads"])
        got_k = dev.get_kmer_counts().copy()
        got_n = dev.get_node_counts().copy()
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.count_kmers_mode(True)
        raw = np.frombuffer(case["raw"], dtype=np.uint8)
        dev.map_records(raw, len(raw), 4 | 0x100, 31)
        assert got_k.any() and np.array_equal(got_k, dev.get_kmer_counts())
    assert np.array_equal(got_n, case["expect"])


def test_hundreds_of_chunks(kmm, case):
    """A few MB of FASTQ with the search every KiB: more than a hundred speculative chunks, the same counts."""
    raw = case["raw"] * 3
    comp = _gzip(raw, 6, strategy=zlib.Z_FILTERED)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.set_param("debug_gzip_chunk_kb", 1)
        assert _feed(dev, comp) == 3 * len(case["reads"])
        assert dev.get_param("gzip_chunks") > 100
        assert np.array_equal(dev.get_node_counts(), 3 * case["expect"].astype(np.int64))


def test_two_line_fasta_and_a_last_line_without_newline(kmm, case, oracle):
    raw = b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(case["reads"]))[:-1]
    comp = _gzip(raw, 6)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        assert _feed(dev, comp, fmt=2) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect"])
        dev.reset()
        raw_q = case["raw"][:-1]                              # FASTQ whose quality line has no newline
        assert _feed(dev, _gzip(raw_q, 9)) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect"])


def test_concatenated_members_with_header_fields(kmm, case):
    """`cat a.gz b.gz c.gz`: members of different levels, FNAME / FCOMMENT / FEXTRA / FHCRC headers, cut inside records."""
    raw = case["raw"]
    cuts = [0, len(raw) // 5 + 17, len(raw) // 2 + 3, len(raw)]
    parts = [raw[cuts[i]:cuts[i + 1]] for i in range(3)]
    m0 = gzip.compress(parts[0], 1)
    body = _gzip(parts[1], 9)[10:]                           # member with FEXTRA + FNAME + FCOMMENT + FHCRC
    hdr = b"\x1f\x8b\x08\x1e\x00\x00\x00\x00\x00\x03" + b"\x04\x00AB\x00\x00" + b"name.fq\x00" + b"a comment\x00"
    m1 = hdr + (zlib.crc32(hdr) & 0xFFFF).to_bytes(2, "little") + body
    m2 = gzip.compress(parts[2], 6)
    comp = m0 + m1 + m2 + b"\x00" * 100
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.set_param("debug_gzip_chunk_kb", 2)
        assert _feed(dev, comp) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect"])
        assert dev.get_param("gzip_members") == 3


def test_windows_cut_anywhere_give_the_same_counts(kmm, case):
    """The same file in 1, 3 and 7 windows cut at arbitrary bytes: every call consumes up to a verified block boundary."""
    comp = _gzip(case["raw"] * 2, 6)
    rng = np.random.default_rng(905)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.set_param("debug_gzip_chunk_kb", 4)
        for n_win in (1, 3, 7):
            cuts = sorted(int(x) for x in rng.integers(1, len(comp), size=n_win - 1))
            dev.reset()
            assert _feed(dev, comp, cuts=cuts) == 2 * len(case["reads"])
            assert np.array_equal(dev.get_node_counts(), 2 * case["expect"].astype(np.int64)), n_win


def _false_start_fastq(reads, rng):
    """FASTQ whose header lines carry the raw bytes of a real non-final dynamic-Huffman block (no newline among them)."""
    blobs = []
    seed = 0
    while len(blobs) < 8:
        seed += 1
        r = np.random.default_rng(seed)
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        b = c.compress(bytes(r.choice(np.frombuffer(b"ACGTacgt:#", dtype=np.uint8), size=4000))) + c.flush(zlib.Z_FULL_FLUSH)
        b = b[:160]
        if b"\n" not in b and (b[0] & 7) == 4:
            blobs.append(b)
    names = [b"r%d " % i + blobs[i % len(blobs)] for i in range(len(reads))]
    return _fastq(reads, rng, names)


def test_a_false_start_is_rejected(kmm, case):
    """A level-0 (stored) gzip file whose FASTQ headers hold real dynamic block headers: the search finds them, the
    predecessor check rejects them, and the counts are exact."""
    raw = _false_start_fastq(case["reads"][:3000], np.random.default_rng(907))
    comp = gzip.compress(raw, 0)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.set_param("debug_gzip_chunk_kb", 1)
        assert _feed(dev, comp) == 3000
        assert dev.get_param("gzip_false_starts") >= 1
        got = dev.get_node_counts()
        dev.reset()
        dev.map_records(np.frombuffer(raw, dtype=np.uint8), len(raw), 4 | 0x100, 31)
        assert np.array_equal(got, dev.get_node_counts())


def test_full_slots_are_continued(kmm, case):
    """Tens of MB of one repeated record (ratio ~1000): the first slots run full and the lanes go on in new pieces."""
    rec = b"@same\n" + case["reads"][0] + b"\n+\n" + b"F" * len(case["reads"][0]) + b"\n"
    n = (24 << 20) // len(rec)
    comp = _gzip(rec * n, 9)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        assert _feed(dev, comp) == n
        assert dev.get_param("gzip_continuations") >= 1
        got = dev.get_node_counts()
        dev.reset()
        raw = np.frombuffer(rec * n, dtype=np.uint8)
        dev.map_records(raw, len(raw), 4 | 0x100, 31)
        assert np.array_equal(got, dev.get_node_counts())


def _corruptions(comp):
    mid = len(comp) // 2
    flip = bytearray(comp)
    flip[mid] ^= 0x10
    crc = bytearray(comp)
    crc[-8] ^= 1
    isz = bytearray(comp)
    isz[-4] ^= 1
    return {"bit flip": bytes(flip), "crc": bytes(crc), "isize": bytes(isz), "truncated": comp[:-100],
            "trailing garbage": comp + b"garbage!", "truncated trailer": comp[:-3]}


def test_damaged_streams_are_refused(kmm, case):
    comp = _gzip(case["raw"], 6)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        for what, bad in _corruptions(comp).items():
            dev.reset()
            with pytest.raises(ValueError):
                _feed(dev, bad)
            assert not dev.get_node_counts().any(), what
        dev.reset()
        assert _feed(dev, comp) == len(case["reads"])                # (the handle is usable afterwards)
        assert np.array_equal(dev.get_node_counts(), case["expect"])


def test_cli_plain_gzip_on_the_gpu_route(kmm, syn, oracle, tmp_path, caplog, monkeypatch):
    """`kmer_mapper map -f reads.fq.gz` with the GPU inflater switched on: the route line is logged and the output equals the
    oracle's; KMM_CLI_NO_GPU_INFLATE=1 keeps the host inflater with the same output."""
    from kmer_mapper_amd import reads_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    index, genome = syn.make_index(5000, seed=911)
    bases, offs = syn.make_ragged_reads(genome, 3000, 20, 200, seed=912)
    idx_path = str(tmp_path / "index.npz")
    index.to_file(idx_path)
    reads_path = str(tmp_path / "reads.fq.gz")
    reads_io.write_fastq(reads_path, ReadBatch(bases, offs), gz=True)
    expect, _ = oracle.map_reads(index, index.max_node_id(), bases, offs, 31, n_threads=4)
    monkeypatch.setenv("KMM_CLI_GPU_GUNZIP", "1")
    with caplog.at_level(logging.INFO):
        run_argument_parser(["map", "-i", idx_path, "-f", reads_path, "-o", str(tmp_path / "a"), "-k", "31"])
    assert "gzip stream inflated on the GPU" in caplog.text
    assert np.array_equal(np.load(str(tmp_path / "a.npy")), expect)
    caplog.clear()
    monkeypatch.setenv("KMM_CLI_NO_GPU_INFLATE", "1")
    with caplog.at_level(logging.INFO):
        run_argument_parser(["map", "-i", idx_path, "-f", reads_path, "-o", str(tmp_path / "b"), "-k", "31"])
    assert "gzip stream inflated on the GPU" not in caplog.text
    assert np.array_equal(np.load(str(tmp_path / "b.npy")), expect)


def test_a_gigabyte_of_fastq_as_plain_gzip(kmm, syn, tmp_path):
    """>= 1 GB of FASTQ written by `gzip -1` maps exactly like its raw bytes (kmm_map_records on the same bytes)."""
    index, genome = syn.make_index(20000, seed=921)
    bases, offs = syn.make_reads(genome, 20000, 150, seed=922)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    block = _fastq(reads, np.random.default_rng(923))
    reps = (1 << 30) // len(block) + 1
    path = tmp_path / "big.fq"
    with open(path, "wb") as f:
        for _ in range(reps):
            f.write(block)
    subprocess.check_call(["gzip", "-1", "-k", str(path)])
    comp = np.fromfile(str(path) + ".gz", dtype=np.uint8)
    with kmm.DeviceIndex.from_index(index, index.max_node_id()) as dev:
        assert _feed(dev, comp.tobytes()) == reps * len(reads)
        got = dev.get_node_counts()
        dev.reset()
        raw = np.frombuffer(block, dtype=np.uint8)
        dev.map_records(raw, len(raw), 4 | 0x100, 31)
        one = dev.get_node_counts().astype(np.int64)
    assert np.array_equal(got.astype(np.int64), reps * one)
    os.unlink(path)
