#!/usr/bin/env python3
"""`kmer_mapper map` on a PLAIN gzip FASTQ (`gzip -6`: one deflate stream), inflated on the GPU (kmm_map_gzip) against the
host inflater, the two routes alternated in one job.
    python tools/gzip_e2e.py [n_reads=10000000] [n_index=100000000] [out_dir=/tmp/kmm_gzip] [reps=3]
The FASTQ is tools/bgzf_e2e.py's (KMM_E2E_QUAL=full41 for the 41-value qualities).  Prints the library loop's time and,
per repetition, the CLI's end-to-end time on either route (KMM_CLI_GPU_GUNZIP=1 / KMM_CLI_NO_GPU_INFLATE=1); the count
vectors must be equal."""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import synthetic as syn                     # noqa: E402
from tools.bgzf_e2e import make_fastq                           # noqa: E402


def main():
    import logging
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 100_000_000
    out_dir = sys.argv[3] if len(sys.argv) > 3 else "/tmp/kmm_gzip"
    reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, 150, seed=2)
    fq = os.path.join(out_dir, "reads.fq")
    make_fastq(fq, bases, n_reads, 150)
    size = os.path.getsize(fq)
    gz = fq + ".gz"
    if os.path.exists(gz):
        os.remove(gz)
    subprocess.check_call(["gzip", "-6", "-k", fq])
    csize = os.path.getsize(gz)
    print("setup %.1f s: %d reads, FASTQ %.2f GB -> gzip -6 %.2f GB (ratio %.2f), %d-entry index"
          % (time.time() - t0, n_reads, size / 1e9, csize / 1e9, size / csize, len(index._kmers)), flush=True)
    from kmer_mapper_amd import _lib
    from kmer_mapper_amd.engine import DeviceIndex
    comp = np.memmap(gz, dtype=np.uint8, mode="r")
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        for rep in range(2):
            dev.reset()
            t = time.perf_counter()
            pos, recs, end = 0, 0, csize
            while pos < csize:
                used, n = dev.map_gzip(comp[pos:end], fmt=_lib.FORMAT_FASTQ, k=31, first=pos == 0, last=True)
                pos += used
                recs += n
            lib_counts = dev.get_node_counts()
            dt = time.perf_counter() - t
            assert recs == n_reads
            print("library loop (rep %d): %.3f s, %.2f GB/s of FASTQ, %d chunks, %d false starts, %d continuations"
                  % (rep, dt, size / dt / 1e9, dev.get_param("gzip_chunks"), dev.get_param("gzip_false_starts"),
                     dev.get_param("gzip_continuations")), flush=True)
    del comp
    from kmer_mapper_amd.command_line_interface import map_bnp

    def cli(gpu):
        os.environ.pop("KMM_CLI_NO_GPU_INFLATE", None)
        os.environ["KMM_CLI_GPU_GUNZIP"] = "1"
        if not gpu:
            os.environ["KMM_CLI_NO_GPU_INFLATE"] = "1"
        ns = argparse.Namespace(kmer_index=index, index_bundle=None, reads=gz, kmer_size=31, n_threads=16, chunk_size=2_500_000,
                                output_file=None, debug=None, max_hits_per_kmer=1000, gpu=True, gpu_hash_map_size=0,
                                map_reverse_complements=False, apply_max_hits_per_kmer=False, host_parser=False, device=0)
        time.sleep(4)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        c = map_bnp(ns)
        return c, time.perf_counter() - t

    times = {True: [], False: []}
    outs = {}
    for rep in range(reps):
        for gpu in (True, False):
            c, dt = cli(gpu)
            times[gpu].append(dt)
            outs[gpu] = c
            print("CLI rep %d, %s: %.3f s end to end, %.2f GB/s of FASTQ" % (rep, "GPU inflater" if gpu else "host inflater", dt,
                                                                             size / dt / 1e9), flush=True)
    for gpu in (True, False):
        t = np.array(times[gpu])
        print("CLI %s: median %.3f s, min %.3f, max %.3f over %d runs" % ("GPU inflater" if gpu else "host inflater", np.median(t),
                                                                          t.min(), t.max(), len(t)), flush=True)
    same = np.array_equal(lib_counts, outs[True]) and np.array_equal(outs[True], outs[False])
    print("counts: library loop == CLI (GPU inflater) == CLI (host inflater): %s" % same, flush=True)
    os.remove(fq)
    os.remove(gz)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
