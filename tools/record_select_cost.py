#!/usr/bin/env python3
"""What a record selection costs: one set of aligned reads as a BAM file and as SAM text, mapped through
DeviceIndex.map_bam / map_records with no rule, a MAPQ floor alone, a region list that keeps everything and one that keeps about
a tenth; and a long-read BAM file whose records carry thousands of CIGAR operations, with no rule and with a region list that
every record starts outside of — the case in which the walking lane of spec / fix reads every CIGAR.
    python tools/record_select_cost.py [n_reads=4000000] [n_index=10000000] [out_dir=/tmp/kmm_select] [reps=5] [legs=all|none|long|names]
Prints per leg the median / min / max wall time of the map calls up to kmm_synchronize over `reps` repetitions after one warm-up,
and the records kept.  legs=none: the no-rule legs alone (an A/B against another build: KMM_LIB_PATH=...).  The files are kept in
out_dir and reused by the next run with the same sizes.  legs=long: the long-read file alone, with no rule and with the region no
record starts in (under `rocprofv3 --kernel-trace --stats`: k_bam_spec / k_bam_decode against k_bam_spec_sel, whose walking lane
reads every CIGAR).  legs=names: the SAM text with no rule, with one name in the list and with 256 names in it (the RNAME lookup)."""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import reads_io, synthetic as syn          # noqa: E402

L = 150
POS0, POS_SPAN = 100_000_000, 100_000_000                       # 9-digit positions on one reference of 250 Mb
REFS = ((b"chr1", 250_000_000),)
_NIB = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _NIB[_c] = _NIB[ord(chr(_c).lower())] = _i


def bgzf_file(path, raw, threads=16):
    view = memoryview(raw)
    with ThreadPoolExecutor(threads) as pool, open(path, "wb") as f:
        for part in pool.map(lambda p: reads_io.bgzf_members(bytes(view[p:p + (64 << 20)]), 0xFF00, 6), range(0, len(raw), 64 << 20)):
            f.write(part)
        f.write(reads_io.BGZF_EOF)


def _digits(values, width):
    out = np.zeros((values.shape[0], width), np.uint8)
    v = values.astype(np.int64).copy()
    for j in range(width - 1, -1, -1):
        out[:, j] = 48 + v % 10
        v //= 10
    return out


def short_reads(bases, n, pos, mapq):
    """(BAM payload, SAM text) of n reads of L bases: FLAG 0, chr1, the given positions and MAPQs, CIGAR <L>M, qualities 'I'."""
    seq = np.ascontiguousarray(bases.reshape(n, L))
    seq = np.where(seq >= 97, seq - 32, seq).astype(np.uint8)
    name = np.concatenate([np.full((n, 1), ord("r"), np.uint8), _digits(np.arange(n), 8)], axis=1)
    ln = name.shape[1] + 1
    size = 36 + ln + 4 + (L + 1) // 2 + L
    out = np.zeros((n, size), np.uint8)
    out[:, 0:4] = np.frombuffer(np.array([size - 4], "<i4").tobytes(), np.uint8)
    out[:, 8:12] = pos.astype("<i4").view(np.uint8).reshape(n, 4)
    out[:, 12] = ln
    out[:, 13] = mapq
    out[:, 14:16] = np.frombuffer(np.array([4680], "<u2").tobytes(), np.uint8)
    out[:, 16:18] = np.frombuffer(np.array([1], "<u2").tobytes(), np.uint8)
    out[:, 20:24] = np.frombuffer(np.array([L], "<i4").tobytes(), np.uint8)
    out[:, 24:32] = 0xFF                                                     # next_refID, next_pos = -1
    out[:, 36:36 + ln - 1] = name
    out[:, 36 + ln:40 + ln] = np.frombuffer(np.array([L << 4], "<u4").tobytes(), np.uint8)
    codes = _NIB[seq]
    s = 40 + ln
    out[:, s:s + L // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    out[:, s + (L + 1) // 2:] = 40
    bam = reads_io.bam_header(REFS, b"@HD\tVN:1.6\tSO:unsorted\n") + out.tobytes()
    tab = np.full((n, 1), 9, np.uint8)
    lit = lambda t: np.tile(np.frombuffer(t, np.uint8), (n, 1))
    sam = np.concatenate([name, lit(b"\t0\tchr1\t"), _digits(pos + 1, 9), tab, _digits(mapq, 2), lit(b"\t%dM\t*\t0\t0\t" % L), seq, tab,
                          np.full((n, L), ord("I"), np.uint8), np.full((n, 1), 10, np.uint8)], axis=1)
    return bam, b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:250000000\n" + sam.tobytes()


def long_reads(genome_ascii, n, length, n_ops, seed=5):
    """A BAM payload of n reads of `length` bases whose CIGARs have n_ops operations (M and D alternating)."""
    rng = np.random.default_rng(seed)
    m = length // ((n_ops + 1) // 2)
    cigar = []
    left = length
    for j in range(n_ops):
        if j % 2 == 0:
            k = m if j + 2 < n_ops else left
            cigar.append(k << 4)
            left -= k
        else:
            cigar.append(1 << 4 | 2)
    cigar = tuple(cigar)
    out = [reads_io.bam_header(REFS, b"@HD\tVN:1.6\tSO:unsorted\n")]
    for i in range(n):
        at = int(rng.integers(0, len(genome_ascii) - length))
        out.append(reads_io.bam_record(genome_ascii[at:at + length], b"long%06d" % i, 0, ref_id=0, pos=int(rng.integers(POS0, POS0 + POS_SPAN)),
                                       cigar=cigar, qual=b"\x28" * length, mapq=60))
    return b"".join(out)


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    out_dir = sys.argv[3] if len(sys.argv) > 3 else "/tmp/kmm_select"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    legs = sys.argv[5] if len(sys.argv) > 5 else "all"
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    tag = "%d_%d" % (n_reads, n_index)
    paths = {k: os.path.join(out_dir, "%s_%s" % (tag, k)) for k in ("short.bam", "short.sam", "long.bam")}
    n_long, long_len, long_ops = max(n_reads // 2000, 100), 20_000, 4_001
    if not all(os.path.exists(p) for p in paths.values()):
        bases, _ = syn.make_reads(genome, n_reads, L, seed=2, n_rate=0.0)
        rng = np.random.default_rng(3)
        bam, sam = short_reads(bases, n_reads, rng.integers(POS0, POS0 + POS_SPAN, size=n_reads), rng.integers(10, 70, size=n_reads))
        bgzf_file(paths["short.bam"], bam)
        with open(paths["short.sam"], "wb") as f:
            f.write(sam)
        bgzf_file(paths["long.bam"], long_reads(np.frombuffer(b"ACGT", np.uint8)[genome[:4_000_000]].tobytes(), n_long, long_len, long_ops))
    files = {k: np.fromfile(p, np.uint8) for k, p in paths.items()}
    print("setup %.1f s: %d reads of %d bp (BAM %.2f GB, SAM %.2f GB), %d long reads of %d bp with %d CIGAR operations (BAM %.2f GB), "
          "%d-entry index" % (time.time() - t0, n_reads, L, files["short.bam"].size / 1e9, files["short.sam"].size / 1e9, n_long, long_len,
                              long_ops, files["long.bam"].size / 1e9, len(index._kmers)), flush=True)
    from kmer_mapper_amd.engine import DeviceIndex
    dev = DeviceIndex.from_index(index, index.max_node_id())
    has_select = os.environ.get("KMM_LIB_PATH") is None or legs != "none"

    def map_bam(comp):
        pos = n = 0
        while pos < len(comp):
            used, n_rec = dev.map_bam(comp[pos:], first=pos == 0, last=True)
            pos, n = pos + used, n + n_rec
        return n

    def map_sam(text):
        pos = n = 0
        while pos < len(text):
            used, n_rec = dev.map_records(text[pos:pos + (512 << 20)], fmt=8)
            pos, n = pos + used, n + n_rec
        return n

    def leg(what, call, data, min_mapq=0, regions=()):
        if has_select:
            dev.set_param("bam_min_mapq", min_mapq)
            dev.set_record_regions(regions)
        times, kept = [], 0
        for rep in range(reps + 1):
            dev.reset()
            dev.synchronize()
            t = time.perf_counter()
            kept = call(data)
            dev.synchronize()
            times.append(time.perf_counter() - t)
        t = np.array(times[1:]) * 1e3
        print("%-44s median %8.2f ms  min %8.2f  max %8.2f  (%d runs, %d records kept)" % (what, np.median(t), t.min(), t.max(), reps, kept),
              flush=True)

    everything, tenth = [("chr1", 0, 0, (1 << 31) - 1)], [("chr1", 0, POS0, POS0 + POS_SPAN // 10)]
    outside = [("chr1", 0, 240_000_000, 240_000_001)]               # every long read starts in front of it: its CIGAR is read
    if legs == "names":
        many = [("zz%03d" % i, None, 0, 10) for i in range(255)]
        leg("SAM, no rule", map_sam, files["short.sam"])
        leg("SAM, everything, 1 name in the list", map_sam, files["short.sam"], regions=[("chr1", None, 0, (1 << 31) - 1)])
        leg("SAM, everything, 256 names in the list", map_sam, files["short.sam"], regions=many + [("chr1", None, 0, (1 << 31) - 1)])
        leg("SAM, nothing, 255 other names in the list", map_sam, files["short.sam"], regions=many)
        dev.close()
        return
    for name, call, key in (("BAM", map_bam, "short.bam"), ("SAM", map_sam, "short.sam")):
        if legs == "long":
            break
        leg(name + ", no rule", call, files[key])
        if legs == "all":
            leg(name + ", MAPQ >= 40", call, files[key], min_mapq=40)
            leg(name + ", a region that keeps everything", call, files[key], regions=everything)
            leg(name + ", a region that keeps a tenth", call, files[key], regions=tenth)
    leg("long-read BAM, no rule", map_bam, files["long.bam"])
    if legs == "long":
        leg("long-read BAM, a region no record starts in", map_bam, files["long.bam"], regions=outside)
    if legs == "all":
        leg("long-read BAM, MAPQ >= 40", map_bam, files["long.bam"], min_mapq=40)
        leg("long-read BAM, a region no record starts in", map_bam, files["long.bam"], regions=outside)
        leg("long-read BAM, a region that keeps everything", map_bam, files["long.bam"], regions=everything)
    dev.close()


if __name__ == "__main__":
    main()
