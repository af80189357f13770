#!/usr/bin/env python3
"""`kmer_mapper map` on the same synthetic reads written as BGZF FASTQ (.fq.gz), unaligned BAM, BGZF SAM (.sam.gz) and plain SAM
(.sam); the four CLI routes alternated in one job.
    python tools/sam_e2e.py [n_reads=4000000] [n_index=10000000] [out_dir=/tmp/kmm_sam] [reps=3] [min_q=0]
The FASTQ is tools/bgzf_e2e.py's (names SRR0000001.<i>, binned qualities), the BAM tools/bam_e2e.py's; the SAM files hold the same
names, bases and qualities (FLAG 4, no header but @HD), compressed files at zlib level 6 in members of 0xFF00 inflated bytes.
Prints per repetition the CLI's map phase on every route (its "hashing and counting" line) and the end-to-end time;
KMM_VERBOSE=1 in the environment adds the library's per-call split.  The count vectors must be equal.
min_q > 0 adds every route once more with --min-base-quality min_q (SAM and BAM with --use-record-qual), alternated
with the floor-off runs: "<route>@Q".  Their count vectors must be equal too — the BGZF FASTQ at the same floor is the yardstick,
the route the records' text hand-off ends in (KMM_E2E_QUAL=full41 draws the qualities from all 41 values)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import synthetic as syn                     # noqa: E402
from tools.bam_e2e import bam_payload, bgzf_file                 # noqa: E402
from tools.bgzf_e2e import make_fastq                            # noqa: E402

_MID = b"\t4\t*\t0\t0\t*\t*\t0\t0\t"


def sam_payload(fastq, n_reads, L):
    """The records of the FASTQ written by make_fastq (fixed-size lines) as SAM lines, built column by column."""
    rec = np.frombuffer(fastq, np.uint8).reshape(n_reads, -1)
    W = rec.shape[1] - (2 * L + 4)                       # "@" + name + "\n"
    name = rec[:, 1:W - 1]
    nl = name.shape[1]
    out = np.empty((n_reads, nl + len(_MID) + 2 * L + 2), np.uint8)
    out[:, :nl] = name
    out[:, nl:nl + len(_MID)] = np.frombuffer(_MID, np.uint8)
    s = nl + len(_MID)
    out[:, s:s + L] = rec[:, W:W + L]
    out[:, s + L] = 9
    out[:, s + L + 1:s + 2 * L + 1] = rec[:, W + L + 3:W + 2 * L + 3]
    out[:, -1] = 10
    return b"@HD\tVN:1.6\tSO:unsorted\n" + out.tobytes()


def main():
    import logging
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    out_dir = sys.argv[3] if len(sys.argv) > 3 else "/tmp/kmm_sam"
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
    paths = {"fastq.gz": os.path.join(out_dir, "reads.fq.gz"), "bam": os.path.join(out_dir, "reads.bam"),
             "sam.gz": os.path.join(out_dir, "reads.sam.gz"), "sam": os.path.join(out_dir, "reads.sam")}
    bgzf_file(paths["fastq.gz"], raw)
    bgzf_file(paths["bam"], bam_payload(raw, n_reads, L))
    sam = sam_payload(raw, n_reads, L)
    bgzf_file(paths["sam.gz"], sam)
    with open(paths["sam"], "wb") as f:
        f.write(sam)
    print("setup %.1f s: %d reads; FASTQ %.2f GB; SAM %.2f GB -> %.2f GB BGZF; %d-entry index"
          % (time.time() - t0, n_reads, len(raw) / 1e9, len(sam) / 1e9, os.path.getsize(paths["sam.gz"]) / 1e9, len(index._kmers)),
          flush=True)
    del raw, sam
    from kmer_mapper_amd.command_line_interface import map_bnp

    def cli(kind):
        route, floor = kind.split("@")[0], kind.endswith("@Q")
        ns = argparse.Namespace(kmer_index=index, index_bundle=None, reads=paths[route], kmer_size=31, n_threads=16, chunk_size=2_500_000,
                                output_file=None, debug=None, max_hits_per_kmer=1000, gpu=True, gpu_hash_map_size=0,
                                map_reverse_complements=False, apply_max_hits_per_kmer=False, host_parser=False, device=0,
                                exclude_flags=0, min_base_quality=min_q if floor else 0,
                                use_record_qual=floor and route != "fastq.gz")
        time.sleep(4)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        c = map_bnp(ns)
        return c, time.perf_counter() - t

    kinds = list(paths) + ([k + "@Q" for k in paths] if min_q > 0 else [])
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
    same = all(np.array_equal(outs["fastq.gz"], outs[k]) for k in paths)
    print("counts: BGZF FASTQ route == BAM route == BGZF SAM route == plain SAM route: %s" % same, flush=True)
    if min_q > 0:
        same_q = all(np.array_equal(outs["fastq.gz@Q"], outs[k + "@Q"]) for k in paths)
        print("counts at Q%d: BGZF FASTQ route == BAM route == BGZF SAM route == plain SAM route: %s; they differ from the floor-off "
              "counts: %s" % (min_q, same_q, not np.array_equal(outs["fastq.gz"], outs["fastq.gz@Q"])), flush=True)
        same = same and same_q
    for p in paths.values():
        os.remove(p)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
