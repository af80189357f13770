#!/usr/bin/env python3
"""`kmer_mapper map` on the same synthetic reads written once as BGZF FASTQ (.fq.gz) and once as unaligned BAM, both at zlib
level 6 in members of 0xFF00 inflated bytes; the two CLI routes alternated in one job.
    python tools/bam_e2e.py [n_reads=10000000] [n_index=100000000] [out_dir=/tmp/kmm_bam] [reps=3] [min_q=0]
The FASTQ is tools/bgzf_e2e.py's (names SRR0000001.<i>, binned qualities); the BAM holds the same names, bases and qualities
(Phred values, FLAG 4).  Prints per repetition the CLI's map phase on either route (its "hashing and counting" line) and the
end-to-end time; KMM_VERBOSE=1 in the environment adds the library's per-call split.  The count vectors must be equal.
min_q > 0 adds both routes once more with --min-base-quality min_q (the BAM with --use-record-qual), alternated with
the floor-off runs: "<route>@Q"; their count vectors must be equal too."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import reads_io, synthetic as syn          # noqa: E402
from tools.bgzf_e2e import make_fastq                            # noqa: E402

_NIB = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    _NIB[_c] = _NIB[ord(chr(_c).lower())] = _i                   # (soft-masked bases: BAM stores the upper-case code)


def bgzf_file(path, raw, threads=16):
    view = memoryview(raw)
    with ThreadPoolExecutor(threads) as pool, open(path, "wb") as f:      # (zlib releases the GIL)
        for part in pool.map(lambda p: reads_io.bgzf_members(bytes(view[p:p + (64 << 20)]), 0xFF00, 6), range(0, len(raw), 64 << 20)):
            f.write(part)
        f.write(reads_io.BGZF_EOF)


def bam_payload(fastq, n_reads, L):
    """The records of the FASTQ written by make_fastq (fixed-size lines) as BAM records, built column by column."""
    rec = np.frombuffer(fastq, np.uint8).reshape(n_reads, -1)
    W = rec.shape[1] - (2 * L + 4)                       # "@" + name + "\n"
    name = rec[:, 1:W - 1]
    ln = name.shape[1] + 1
    size = 36 + ln + (L + 1) // 2 + L
    out = np.zeros((n_reads, size), np.uint8)
    fixed = np.frombuffer(np.array([size - 4, -1, -1], "<i4").tobytes() + bytes([ln, 255]) + np.array([4680, 0, 4], "<u2").tobytes() +
                          np.array([L, -1, -1, 0], "<i4").tobytes(), np.uint8)
    out[:, :36] = fixed
    out[:, 36:36 + ln - 1] = name
    codes = _NIB[rec[:, W:W + L]]
    if L % 2:
        codes = np.concatenate([codes, np.zeros((n_reads, 1), np.uint8)], axis=1)
    s = 36 + ln
    out[:, s:s + (L + 1) // 2] = (codes[:, 0::2] << 4) | codes[:, 1::2]
    out[:, s + (L + 1) // 2:] = rec[:, W + L + 3:W + 2 * L + 3] - 33
    return reads_io.bam_header(text=b"@HD\tVN:1.6\tSO:unsorted\n") + out.tobytes()


def main():
    import logging
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    out_dir = sys.argv[3] if len(sys.argv) > 3 else "/tmp/kmm_bam"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    min_q = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    L = 150
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    fq = os.path.join(out_dir, "reads.fq")
    make_fastq(fq, bases, n_reads, L)
    raw = open(fq, "rb").read()
    os.remove(fq)
    paths = {"fastq.gz": os.path.join(out_dir, "reads.fq.gz"), "bam": os.path.join(out_dir, "reads.bam")}
    bgzf_file(paths["fastq.gz"], raw)
    payload = bam_payload(raw, n_reads, L)
    bgzf_file(paths["bam"], payload)
    print("setup %.1f s: %d reads; FASTQ %.2f GB -> %.2f GB BGZF; BAM %.2f GB inflated -> %.2f GB; %d-entry index"
          % (time.time() - t0, n_reads, len(raw) / 1e9, os.path.getsize(paths["fastq.gz"]) / 1e9, len(payload) / 1e9,
             os.path.getsize(paths["bam"]) / 1e9, len(index._kmers)), flush=True)
    del raw, payload
    from kmer_mapper_amd.command_line_interface import map_bnp

    def cli(kind):
        route, floor = kind.split("@")[0], kind.endswith("@Q")
        ns = argparse.Namespace(kmer_index=index, index_bundle=None, reads=paths[route], kmer_size=31, n_threads=16, chunk_size=2_500_000,
                                output_file=None, debug=None, max_hits_per_kmer=1000, gpu=True, gpu_hash_map_size=0,
                                map_reverse_complements=False, apply_max_hits_per_kmer=False, host_parser=False, device=0,
                                exclude_flags=0, min_base_quality=min_q if floor else 0, use_record_qual=floor and route == "bam")
        time.sleep(4)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        c = map_bnp(ns)
        return c, time.perf_counter() - t

    kinds = ["fastq.gz", "bam"] + (["fastq.gz@Q", "bam@Q"] if min_q > 0 else [])
    outs, times = {}, {k: [] for k in kinds}
    for rep in range(reps):
        for kind in kinds:
            c, dt = cli(kind)
            outs[kind] = c
            times[kind].append(dt)
            print("CLI rep %d, %s: %.3f s end to end" % (rep, kind, dt), flush=True)
    for kind, t in times.items():
        t = np.array(t)
        print("CLI %s: median %.3f s end to end, min %.3f, max %.3f over %d runs" % (kind, np.median(t), t.min(), t.max(), len(t)),
              flush=True)
    same = np.array_equal(outs["fastq.gz"], outs["bam"])
    print("counts: BGZF FASTQ route == BAM route: %s" % same, flush=True)
    if min_q > 0:
        same_q = np.array_equal(outs["fastq.gz@Q"], outs["bam@Q"])
        print("counts at Q%d: BGZF FASTQ route == BAM route: %s" % (min_q, same_q), flush=True)
        same = same and same_q
    for p in paths.values():
        os.remove(p)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
