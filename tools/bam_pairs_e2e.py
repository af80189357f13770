#!/usr/bin/env python3
"""`select-reads --bam-to-fastq --bam-pairs` next to the routes it is priced against, on the reads of
tools/bam_fastq_e2e.py built as pairs: 150 bases, records 2p and 2p + 1 named SRR0000001.<p>, both mates of every second pair
random bases (half of the pairs have a hit), written once as unaligned BAM and once as interleaved BGZF FASTQ.
    python tools/bam_pairs_e2e.py setup DIR [n_reads=4000000] [n_index=10000000]     writes DIR/index.npz, reads.bam, reads.fq.gz
    python tools/bam_pairs_e2e.py run WHAT DIR [reps=3]                              WHAT: select-bam | select-bam-pairs | select-interleaved
select-bam: `select-reads --bam-to-fastq` (every record by itself); select-bam-pairs: the same with --bam-pairs;
select-interleaved: `select-reads --interleaved` on the BGZF FASTQ.  Prints per repetition the CLI's map phase and the end-to-end
time.  One process per library under comparison (KMM_LIB_PATH names another build's libkmm.so); a profiler goes around `run`."""
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(out_dir, n_reads, n_index):
    from kmer_mapper_amd import synthetic as syn
    from tools.bam_e2e import bam_payload, bgzf_file
    from tools.bgzf_e2e import make_fastq
    L = 150
    assert n_reads % 4 == 0
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    pairs = np.asarray(bases).reshape(n_reads // 2, 2, L)
    rng = np.random.Generator(np.random.PCG64(3))
    pairs[1::2] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n_reads // 4, 2, L), dtype=np.uint8)]   # no hit in either mate
    fq = os.path.join(out_dir, "reads.fq")
    width = make_fastq(fq, pairs.reshape(-1), n_reads, L)
    rec = np.fromfile(fq, dtype=np.uint8).reshape(n_reads, width)
    os.remove(fq)
    hdr = len(b"@SRR0000001.")
    pair = np.arange(n_reads, dtype=np.int64) // 2                     # the name's number: the pair's, in both mates
    for d in range(9):
        rec[:, hdr + 8 - d] = (pair // 10 ** d % 10 + 48).astype(np.uint8)
    raw = rec.tobytes()
    bgzf_file(os.path.join(out_dir, "reads.fq.gz"), raw)
    payload = bam_payload(raw, n_reads, L)
    bgzf_file(os.path.join(out_dir, "reads.bam"), payload)
    index.to_file(os.path.join(out_dir, "index.npz"))
    print("setup %.1f s: %d reads in %d pairs; FASTQ %.2f GB -> %.2f GB BGZF; BAM %.2f GB inflated -> %.2f GB; %d-entry index"
          % (time.time() - t0, n_reads, n_reads // 2, len(raw) / 1e9, os.path.getsize(os.path.join(out_dir, "reads.fq.gz")) / 1e9,
             len(payload) / 1e9, os.path.getsize(os.path.join(out_dir, "reads.bam")) / 1e9, len(index._kmers)), flush=True)


def run(what, out_dir, reps):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from tools.bam_fastq_e2e import _MapPhase
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    npz, bam, fq = (os.path.join(out_dir, n) for n in ("index.npz", "reads.bam", "reads.fq.gz"))
    out = os.path.join(out_dir, "out_" + what)
    common = ["-i", npz, "-k", "31", "-o", out]
    args = {"select-bam": ["select-reads", "-f", bam, "--bam-to-fastq"] + common,
            "select-bam-pairs": ["select-reads", "-f", bam, "--bam-to-fastq", "--bam-pairs"] + common,
            "select-interleaved": ["select-reads", "-f", fq, "--interleaved"] + common}[what]
    lib = os.environ.get("KMM_LIB_PATH", "this build")
    times, sizes = [], set()
    for rep in range(reps):
        watch = _MapPhase()
        logging.getLogger().addHandler(watch)
        time.sleep(2)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        run_argument_parser(args)
        dt = time.perf_counter() - t
        logging.getLogger().removeHandler(watch)
        times.append(watch.seconds)
        sizes.add(os.path.getsize(out))
        print("%s [%s] rep %d: map phase %.4f s, %.3f s end to end; %s" % (what, lib, rep, watch.seconds, dt, " | ".join(watch.lines)),
              flush=True)
    t = np.array(times)
    print("%s [%s]: map phase median %.4f s, min %.4f, max %.4f over %d runs; output bytes %s" % (what, lib, np.median(t), t.min(), t.max(),
                                                                                                 len(t), sorted(sizes)), flush=True)
    if os.path.exists(out):
        os.remove(out)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "setup":
        setup(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4_000_000, int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000)
    elif len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
