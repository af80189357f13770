"""GPU tests of "original_strand" (include/kmm.h): with the switch on, kmm_map_bam and KMM_FORMAT_SAM hand every kept
record whose FLAG has 0x10 to the mapper in read orientation.  The reads are made in READ ORIENTATION and written the way an
aligner stores them (tests/strand_cases.py: a chosen set R reverse-complemented, qualities reversed, FLAG | 0x10): with the switch
on, counts, lookups and "quality_masked_bases" equal the oracle's on the untouched reads; with it off, on the stored text; every
case asserts that the two answers differ."""
import numpy as np
import pytest

from tests import quality_cases as qc
from tests import strand_cases as sc

pytestmark = pytest.mark.gpu

SAM, FASTQ, FASTA2 = 8, 4, 2
REPEATS = 10                 # the length list, this many times: 40 KB of BAM records in members of 4 KiB, three 16 KiB tiles


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


@pytest.fixture(scope="module")
def devs(kmm):
    """One handle per k, shared by the tests of this module."""
    open_ = {}

    def get(k):
        if k not in open_:
            index = qc.index_for(k)
            open_[k] = (kmm.DeviceIndex.from_index(index, index.max_node_id()), index, index.max_node_id())
        return open_[k]
    yield get
    for d, _, _ in open_.values():
        d.close()


def _genome_read(rng, n):
    s = int(rng.integers(0, qc.GENOME.shape[0] - n - 64))
    return qc.ACGT[qc.GENOME[s:s + n]].tobytes()


def _sweep(seed, repeats=REPEATS):
    """The CPU tier's lengths, `repeats` times, drawn from the genome; R = every second record."""
    rng = np.random.Generator(np.random.PCG64(seed))
    recs = []
    for n in sc.LENGTHS * repeats:
        recs.append((sc.REVERSE if len(recs) % 2 else 0, _genome_read(rng, n), b"I" * n))
    return recs


def _flat(reads):
    offsets = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offsets[1:])
    return np.frombuffer(b"".join(reads), np.uint8), offsets


def _oracle(oracle, index, mx, reads, k, rc=False, mask=None, table=None):
    """(counts, lookups) of the oracle on the reads, split at the masked bases and at the table's break letters."""
    bases, offsets = _flat(reads)
    if table is not None:
        brk = np.asarray(table, np.uint8)[bases] == 0xFE
        mask = brk if mask is None else (mask | brk)
    if mask is not None:
        bases, offsets = qc.split_at_mask(bases, offsets, mask)
    counts, n = oracle.map_reads(index, mx, bases, offsets, k, also_revcomp=rc)
    return counts, (2 if rc else 1) * n


def _files(records, block=0x1000):
    from kmer_mapper_amd import reads_io
    bam = np.frombuffer(reads_io.bgzf_members(sc.bam_payload(records), block) + reads_io.BGZF_EOF, np.uint8)
    text = sc.sam_bytes(records)
    bgzf = np.frombuffer(reads_io.bgzf_members(text, block) + reads_io.BGZF_EOF, np.uint8)
    return bam, np.frombuffer(text, np.uint8), bgzf


def _run(dev, call, orig, path=0, q=0, use=0, piece_kb=0, cap_kb=0, excl=0):
    """(counts, lookups, records_reversed, quality_masked_bases, records_without_qual, what the call returned), clean handle."""
    dev.reset()
    dev.get_stats(reset=True)
    for name, v in (("original_strand", orig), ("path", path), ("min_base_quality", q), ("use_record_qual", use),
                    ("debug_records_piece_kb", piece_kb), ("debug_bgzf_call_cap_kb", cap_kb), ("bam_exclude_flags", excl)):
        dev.set_param(name, v)
    try:
        ret = call()
        return (dev.get_node_counts().copy(), dev.get_stats()[0], dev.get_param("records_reversed"), dev.get_param("quality_masked_bases"),
                dev.get_param("records_without_qual"), ret)
    finally:
        for name in ("original_strand", "path", "min_base_quality", "use_record_qual", "debug_records_piece_kb", "debug_bgzf_call_cap_kb",
                     "bam_exclude_flags"):
            dev.set_param(name, 0)


def _routes(dev, files, k, rc=False, table=None):
    bam, sam, bgzf = files
    return (("bam", lambda: dev.map_bam(bam, first=True, last=True, k=k, also_revcomp=rc, lut=table), len(bam)),
            ("sam", lambda: dev.map_records(sam, fmt=SAM, k=k, also_revcomp=rc, lut=table), len(sam)),
            ("sam, bgzf", lambda: dev.map_bgzf(bgzf, fmt=SAM, k=k, first=True, last=True, also_revcomp=rc, lut=table), len(bgzf)))


def _check_on_and_off(oracle, devs, records, k, paths=(0, 1), rc=False, table=None, excl=0):
    """Every route, switch on and off: the oracle on the untouched reads / on the stored text; the two differ."""
    dev, index, mx = devs(k)
    kept = [r for r in records if not r[0] & excl]
    on = _oracle(oracle, index, mx, [s for _, s, _ in kept], k, rc, table=table)
    off = _oracle(oracle, index, mx, [s for _, s, _ in sc.stored(kept)], k, rc, table=table)
    assert not np.array_equal(on[0], off[0])
    files = _files(records)
    for what, call, n_bytes in _routes(dev, files, k, rc, table):
        for path in paths:
            for orig, want in ((1, on), (0, off)):
                got = _run(dev, call, orig, path=path, excl=excl)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], (what, path, orig)
                assert got[2] == (sc.n_flipped(records, excl) if orig else 0), (what, path, orig, "records_reversed")
                assert got[5] == (n_bytes, len(kept)), (what, path, orig)
    return files, on, off


# ---------------------------------------------------------------------------------------------- known answer
def test_known_answer_by_hand(kmm, oracle):
    """The three records of tests/test_gpu_bam.py::test_known_answer, k = 4, index ACGT -> 1, GTAA -> 2, CGTT -> 3, TTTT -> 4.
    Record 1 "ACGTNAC" (N -> A: ACGT CGTA GTAA TAAC), record 2 empty, record 3 "GGACGTT" with FLAG 16.  Off: GGAC GACG ACGT CGTT,
    counts [0, 2, 1, 1, 0].  On: the read is "AACGTCC" (AACG ACGT CGTC GTCC): node 3 is not hit, [0, 2, 1, 0, 0].  8 lookups both."""
    import struct
    from kmer_mapper_amd import reads_io
    words = [b"ACGT", b"GTAA", b"CGTT", b"TTTT"]
    km = np.array([int(oracle.extract(np.frombuffer(w, np.uint8), np.array([0, 4], np.int64), 4)[0]) for w in words], np.uint64)
    index = oracle.build_index(km, np.array([1, 2, 3, 4], np.int64), 13)
    text = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:100\n"
    header = b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<II", 1, 5) + b"chr1\x00" + struct.pack("<I", 100)

    def rec(ref, pos, name, flag, cigar, l_seq, seq_bytes, qual, aux):
        body = struct.pack("<iiBBHHHiiii", ref, pos, len(name) + 1, 60, 4680, len(cigar), flag, l_seq, -1, -1, 0) + name + b"\x00" + \
            b"".join(struct.pack("<I", c) for c in cigar) + seq_bytes + qual + aux
        return struct.pack("<I", len(body)) + body
    r1 = rec(0, 10, b"first", 0, [(7 << 4) | 0], 7, bytes([0x12, 0x48, 0xF1, 0x20]), b"IIIIIII", b"NMC\x01XZZhello\x00")
    r2 = rec(-1, -1, b"empty", 4, [], 0, b"", b"", b"")
    r3 = rec(0, 20, b"third", 16, [(3 << 4) | 0, (1 << 4) | 1, (3 << 4) | 0], 7, bytes([0x44, 0x12, 0x48, 0x80]), b"\xff" * 7, b"RGZgrp1\x00")
    comp = np.frombuffer(reads_io.bgzf_members(header) + reads_io.bgzf_members(r1 + r2 + r3) + reads_io.BGZF_EOF, np.uint8)
    with kmm.DeviceIndex.from_index(index, 4) as dev:
        for path in (0, 1):
            for orig, want in ((0, [0, 2, 1, 1, 0]), (1, [0, 2, 1, 0, 0])):
                got = _run(dev, lambda: dev.map_bam(comp, first=True, last=True, k=4), orig, path=path)
                assert got[0].tolist() == want and got[1] == 8 and got[2] == orig and got[5] == (len(comp), 3), (path, orig)


# ---------------------------------------------------------------------------------------------- lengths, calls, symmetry
@pytest.mark.parametrize("k", [31, 4])
def test_every_length_forward_and_reversed(kmm, oracle, devs, k):
    """0 .. 257 bases, every second record reversed: BAM in members of 4 KiB (records straddle members and 16 KiB tiles), the
    same reads as SAM text through kmm_map_records and as BGZF through kmm_map_bgzf; "path" 0 and 1."""
    records = _sweep(81)
    files, _, _ = _check_on_and_off(oracle, devs, records, k)
    assert len(sc.bam_payload(records)) > 2 * 16384 and len(files[0]) > 8 * 1024


def test_several_calls_flip_a_carried_record_once(kmm, oracle, devs):
    """kmm_map_bam under a call cap of 4 KiB (calls end inside records, the carry is used); SAM through kmm_map_records fed in
    pieces of 6 000 bytes cut at *consumed, the library cutting those into pieces of 4 KiB: the totals of the one-call run."""
    k = 31
    dev, index, mx = devs(k)
    records = _sweep(82)
    bam, sam, _ = _files(records)
    reads = [s for _, s, _ in records]
    on = _oracle(oracle, index, mx, reads, k)
    off = _oracle(oracle, index, mx, [s for _, s, _ in sc.stored(records)], k)
    assert not np.array_equal(on[0], off[0])

    def bam_in_calls():
        pos = n = 0
        carried = False
        while pos < len(bam):
            used, n_rec = dev.map_bam(bam[pos:], first=pos == 0, last=True, k=k)
            assert used > 0
            pos, n = pos + used, n + n_rec
            carried = carried or dev.get_param("bgzf_carry_bytes") > 0
        return pos, n, carried

    def sam_in_pieces():
        pos = n = calls = 0
        while pos < len(sam):
            used, n_rec = dev.map_records(sam[pos:pos + 6_000], fmt=SAM, k=k)
            assert used > 0
            pos, n, calls = pos + used, n + n_rec, calls + 1
        return pos, n, calls > 3

    for what, call, size in (("bam", bam_in_calls, len(bam)), ("sam", sam_in_pieces, len(sam))):
        for path in (0, 1):
            for orig, want in ((1, on), (0, off)):
                got = _run(dev, call, orig, path=path, cap_kb=4, piece_kb=4)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], (what, path, orig)
                assert got[2] == (sc.n_flipped(records) if orig else 0) and got[5] == (size, len(records), True), (what, path, orig)


def test_symmetry_under_also_revcomp(kmm, oracle, devs):
    """With also_revcomp the k-mers of a read and of its reverse complement are the same set: the switch changes nothing (reads
    without N); without also_revcomp it does."""
    k = 31
    dev, index, mx = devs(k)
    records = _sweep(83, repeats=2)
    want = _oracle(oracle, index, mx, [s for _, s, _ in records], k, rc=True)[0]
    for path in (0, 1):
        for what, call, _ in _routes(dev, _files(records), k, rc=True):
            on, off = _run(dev, call, 1, path=path), _run(dev, call, 0, path=path)
            assert np.array_equal(on[0], off[0]) and on[1] == off[1] and on[0].any(), (what, path)
            assert np.array_equal(on[0], want), (what, path)
            assert on[2] == sc.n_flipped(records) and off[2] == 0, (what, path)
        for what, call, _ in _routes(dev, _files(records), k, rc=False):
            assert not np.array_equal(_run(dev, call, 1, path=path)[0], _run(dev, call, 0, path=path)[0]), (what, path)


# ---------------------------------------------------------------------------------------------- the table after the flip
def test_break_letters_break_at_their_mirrored_positions(kmm, oracle, devs, lut):
    """ambiguous_skip_lut(): reversed records with N and IUPAC letters (R <-> Y, K <-> M, ... swap under the flip, all are breaks)
    at positions that are not their own mirror: the oracle on the untouched reads split at those letters.  The default table turns
    the flipped read's N into A.  '=' in a reversed record is KMM_ERR_INVALID_BASE at the next synchronising call, as forward."""
    k = 31
    dev, index, mx = devs(k)
    rng = np.random.Generator(np.random.PCG64(84))
    records = []
    for i in range(40):
        read = bytearray(_genome_read(rng, 150))
        for j, letter in enumerate(b"NRYKMSWBDHV"[i % 11:][:3]):
            read[(7 + 11 * i + 37 * j) % 150] = letter
        if i % 5 == 0:
            read[0], read[148] = ord("N"), ord("R")
        records.append((sc.REVERSE if i % 3 else 0, bytes(read), b"I" * 150))
    _check_on_and_off(oracle, devs, records, k, table=lut)
    only_n = [(f, bytes(ord("N") if c not in b"ACGT" else c for c in s), q) for f, s, q in records]
    _check_on_and_off(oracle, devs, only_n, k)                                            # (the oracle reads N as A too)
    bad = list(records)
    bad[4] = (sc.REVERSE, bad[4][1][:70] + b"=" + bad[4][1][71:], bad[4][2])
    bad_fwd = list(records)
    bad_fwd[4] = (0,) + bad[4][1:]
    for recs in (bad, bad_fwd):
        files = _files(recs)
        for what, call, _ in _routes(dev, files, k, table=lut):
            for path in (0, 1):
                with pytest.raises(ValueError, match="is not a nucleotide"):
                    _run(dev, call, 1, path=path)
                dev.reset()


# ---------------------------------------------------------------------------------------------- the quality floor
def test_the_floor_masks_the_base_the_sequencer_called_badly(kmm, oracle, devs):
    """"use_record_qual" 1, Q = 20: reversed records of 150 and of 151 bases (the padding nibble of an odd l_seq beside qualities)
    with one low base at read position 2 — stored position l_seq - 3 — and a few elsewhere; "path" 0 and 1; counts and "quality_masked_bases" equal the untouched reads'.  With the switch off the same files give the answer
    on the stored text with the stored qualities.  A reversed record without qualities is counted and still flipped."""
    k, q = 31, 20
    dev, index, mx = devs(k)
    rng = np.random.Generator(np.random.PCG64(85))
    records = []
    for i in range(60):
        n = 151 if i % 4 in (0, 3) else 150                              # (odd lengths forward, i % 4 == 0, and reversed, == 3)
        qual = bytearray(b"I" * n)
        qual[2] = 33 + q - 1
        if i % 7 == 0:
            qual[40], qual[n - 1] = 33 + 3, 33 + q - 1
        records.append((sc.REVERSE if i % 2 else 0, _genome_read(rng, n), None if i in (5, 6) else bytes(qual)))

    def answer(recs):
        quals = np.frombuffer(b"".join(b"~" * len(s) if ql is None else ql for _, s, ql in recs), np.uint8)
        mask = qc.low_mask(quals, q)
        return _oracle(oracle, index, mx, [s for _, s, _ in recs], k, mask=mask) + (int(mask.sum()),)
    on, off = answer(records), answer(sc.stored(records))
    assert not np.array_equal(on[0], off[0]) and on[2] == off[2] > 60
    assert sum(1 for f, s, _ in records if f & sc.REVERSE and len(s) % 2) == 15
    for what, call, n_bytes in _routes(dev, _files(records), k):
        for path in (0, 1):
            for orig, want in ((1, on), (0, off)):
                got = _run(dev, call, orig, path=path, q=q, use=1)
                assert np.array_equal(got[0], want[0]) and got[1] == want[1], (what, path, orig)
                assert got[3] == want[2] and got[4] == 2, (what, path, orig, "quality_masked_bases / records_without_qual")
                assert got[2] == (30 if orig else 0) and got[5] == (n_bytes, 60), (what, path, orig)
            with pytest.raises(ValueError, match="SAM / BAM records are mapped without their QUAL.*use_record_qual"):
                _run(dev, call, 1, path=path, q=q, use=0)                # refused as without the switch
            dev.reset()


# ---------------------------------------------------------------------------------------------- refusals and no-ops
def test_refusals_and_no_ops(kmm, oracle, devs):
    """2 and -1 are KMM_ERR_INVALID_ARG; the switch changes nothing on FASTQ, two-line FASTA and flat reads; records dropped by the
    flag filter are neither flipped nor counted."""
    k = 31
    dev, index, mx = devs(k)
    for bad in (2, -1):
        with pytest.raises(ValueError, match="original_strand takes 0 or 1"):
            dev.set_param("original_strand", bad)
    assert dev.get_param("original_strand") == 0
    dev.set_param("original_strand", 1)
    assert dev.get_param("original_strand") == 1
    dev.set_param("original_strand", 0)
    records = _sweep(86, repeats=1)
    reads = [s for _, s, _ in sc.stored(records)]
    bases, offsets = _flat(reads)
    fq = np.frombuffer(b"".join(b"@r 16\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for s in reads), np.uint8)
    fa = np.frombuffer(b"".join(b">r 16\n" + s + b"\n" for s in reads), np.uint8)
    want = _oracle(oracle, index, mx, reads, k)
    for what, call in (("fastq", lambda: dev.map_records(fq, fmt=FASTQ, k=k)), ("fasta", lambda: dev.map_records(fa, fmt=FASTA2, k=k)),
                       ("flat", lambda: dev.map_reads(bases, offsets, k=k))):
        for path in (0, 1):
            on, off = _run(dev, call, 1, path=path), _run(dev, call, 0, path=path)
            assert np.array_equal(on[0], off[0]) and np.array_equal(on[0], want[0]), (what, path)
            assert on[1:5] == off[1:5] == (want[1], 0, 0, 0), (what, path)
    flagged = [(f | (0x100 if i % 4 == 1 else 0x800 if i % 4 == 3 else 0), s, ql) for i, (f, s, ql) in enumerate(records)]
    assert sc.n_flipped(flagged, 0x900) == 0 and sc.n_flipped(flagged) > 0
    dropped = [r for r in flagged if not r[0] & 0x900]
    want = _oracle(oracle, index, mx, [s for _, s, _ in dropped], k)
    for what, call, n_bytes in _routes(dev, _files(flagged), k):
        for path in (0, 1):
            got = _run(dev, call, 1, path=path, excl=0x900)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == 0, (what, path)
            assert got[5] == (n_bytes, len(dropped)), (what, path)
    _check_on_and_off(oracle, devs, flagged, k)


# ---------------------------------------------------------------------------------------------- the command line
def test_cli_end_to_end(kmm, oracle, devs, tmp_path, caplog):
    """One read set as FASTQ and as aligned-style BAM and SAM with every second record reversed: `kmer_mapper map` (no -r) writes
    identical .npy files for the FASTQ and for the BAM and SAM with --original-strand, different ones without it; with
    --min-base-quality 20 --use-record-qual they are identical as well."""
    import logging
    from kmer_mapper_amd import command_line_interface as cli, reads_io
    k = 31
    _, index, _ = devs(k)
    rng = np.random.Generator(np.random.PCG64(87))
    records = []
    for i in range(300):
        qual = bytearray(b"I" * 150)
        for p in rng.integers(0, 150, size=3):
            qual[int(p)] = 33 + 7
        records.append((sc.REVERSE if i % 2 else 0, _genome_read(rng, 150), bytes(qual)))
    idx = str(tmp_path / "idx.npz")
    index.to_file(idx)
    fq, bam, sam = str(tmp_path / "r.fq"), str(tmp_path / "r.bam"), str(tmp_path / "r.sam")
    with open(fq, "wb") as f:
        f.write(b"".join(b"@r%d\n" % i + s + b"\n+\n" + ql + b"\n" for i, (_, s, ql) in enumerate(records)))
    with open(bam, "wb") as f:
        f.write(reads_io.bgzf_members(sc.bam_payload(records), 0x1000) + reads_io.BGZF_EOF)
    with open(sam, "wb") as f:
        f.write(sc.sam_bytes(records))

    def run(path, *extra):
        out = str(tmp_path / "out")
        caplog.clear()
        with caplog.at_level(logging.INFO):
            cli.run_argument_parser(["map", "-i", idx, "-f", path, "-o", out, *extra])
        return np.load(out + ".npy"), caplog.text
    for floor in ([], ["--min-base-quality", "20"]):
        want, _ = run(fq, *floor)
        assert want.any()
        rq = ["--use-record-qual"] if floor else []
        for path in (bam, sam):
            got, log = run(path, "--original-strand", "--exclude-flags", "0x900", *floor, *rq)
            assert np.array_equal(got, want), (path, floor)
            assert "records_reversed: 150 records" in log and "samtools fastq" not in log
            got, log = run(path, *floor, *rq)
            assert not np.array_equal(got, want) and "records_reversed" not in log, (path, floor)
    _, log = run(bam, "--original-strand")
    assert log.count("samtools fastq") == 1
    caplog.clear()
    with caplog.at_level(logging.INFO), pytest.raises(ValueError, match="--original-strand applies to SAM and BAM input only"):
        cli.run_argument_parser(["map", "-i", idx, "-f", fq, "-o", str(tmp_path / "out"), "--original-strand"])
    assert "Index resident in HBM" not in caplog.text
