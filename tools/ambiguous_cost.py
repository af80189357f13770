#!/usr/bin/env python3
"""What a lookup table with a break entry (KMM_LUT_BREAK, `--ambiguous-bases skip`) costs.

Kernels: BASELINE configs[2]'s index (100 M k-mers) and ONE batch of 20 M reads of 150 bp resident in HBM, mapped with
kmm_map_reads_uniform in one of three ways (--variant):
    default      the default table, no N in the data: packed tiles in pass 1, nothing new launched
    skip_clean   util.ambiguous_skip_lut(), no N in the data: the pre-pass (k_mark_uniform_starts + k_mark_breaks) and
                 pass 1 on position-based tiles with the read-start bitset
    skip_n       the same table, 0.1 % N in the data
Per-kernel times come from a run of its own under the profiler, one variant per run (no counters in that run):
    rocprofv3 --kernel-trace --stats -d OUT -o skip_n -- python tools/ambiguous_cost.py --variant skip_n
Without the profiler the tool prints the whole step (wall clock between synchronisations) and pass 1 .. flush from the
library's own event timers:
    python tools/ambiguous_cost.py --variant all

CLI (--cli N_READS): `kmer_mapper map` on a plain FASTQ of N_READS reads (10 M = 3 GB) with the default table (host
packer) against --ambiguous-bases skip (device route: the raw bytes cross PCIe), and on its BGZF (both on the device),
the map phase of each ("hashing and counting") alternated --reps times.
Not part of the product."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import synthetic as syn                     # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex                    # noqa: E402
from kmer_mapper_amd.util import ambiguous_skip_lut               # noqa: E402

VARIANTS = {"default": (False, 0.0), "skip_clean": (True, 0.0), "skip_n": (True, 0.001)}


def kernels(args):
    import torch
    index, g_ascii = syn.make_index_torch(args.index_kmers, k=31, seed=1)
    lut = torch.from_numpy(ambiguous_skip_lut()).cuda()
    names = list(VARIANTS) if args.variant == "all" else [args.variant]
    R, L = args.reads, 150
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        batches = {}
        for name in names:
            n_rate = VARIANTS[name][1]
            if n_rate not in batches:
                batches[n_rate] = syn.make_reads_torch(g_ascii, R, L, seed=1001, n_rate=n_rate, lower_frac=0.0)
        torch.cuda.synchronize()
        for name in names:
            skip, n_rate = VARIANTS[name]
            bases = batches[n_rate]
            table = lut if skip else None
            for _ in range(args.warmup):
                dev.map_reads_uniform(bases, R, L, 31, lut=table)
            dev.synchronize()
            dev.reset()
            dev.get_stats(reset=True)
            dev.set_timing(True)
            dev.get_timing()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                dev.map_reads_uniform(bases, R, L, 31, lut=table)
            dev.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            timers = {k: round(ms / max(n, 1), 3) for k, (ms, n) in dev.get_timing().items() if n}
            dev.set_timing(False)
            lookups, hits = dev.get_stats()
            print(json.dumps({"variant": name, "reads": R, "n_fraction": n_rate, "step_ms": round(dt * 1e3, 3),
                              "M_kmers_per_s": round(lookups / args.steps / dt / 1e6, 1), "lookups_per_step": lookups // args.steps,
                              "hits_per_step": hits // args.steps, "ms_per_launch": timers,
                              "radix_batches": dev.get_param("radix_batches"), "flat_uniform_batches": dev.get_param("flat_uniform_batches")}),
                  flush=True)


def cli(args):
    import logging
    import re
    import io
    from kmer_mapper_amd.command_line_interface import map_bnp
    from tools.bam_e2e import bgzf_file
    from tools.cli_e2e import write_fastq_fast
    n_reads, L = args.cli, 150
    os.makedirs(args.out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(args.index_kmers, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    fq, gz = os.path.join(args.out_dir, "reads.fq"), os.path.join(args.out_dir, "reads.fq.gz")
    write_fastq_fast(fq, bases, n_reads, L)
    n_gz = min(n_reads, args.bgzf_reads)
    with open(fq, "rb") as f:
        bgzf_file(gz, f.read(n_gz * (2 * L + 7)))
    print("setup %.1f s: FASTQ of %.2f GB (%d reads), BGZF of %.2f GB (%d reads)"
          % (time.time() - t0, os.path.getsize(fq) / 1e9, n_reads, os.path.getsize(gz) / 1e9, n_gz), flush=True)
    log = io.StringIO()
    handler = logging.StreamHandler(log)
    logging.getLogger().addHandler(handler)
    logging.getLogger().setLevel(logging.INFO)

    def run(path, mode):
        ns = argparse.Namespace(kmer_index=index, index_bundle=None, reads=path, kmer_size=31, n_threads=16, chunk_size=2_500_000,
                                output_file=None, debug=None, max_hits_per_kmer=1000, gpu=True, gpu_hash_map_size=0,
                                map_reverse_complements=False, apply_max_hits_per_kmer=False, host_parser=False, device=0,
                                ambiguous_bases=mode)
        log.seek(0)
        log.truncate()
        t = time.perf_counter()
        counts = map_bnp(ns)
        e2e = time.perf_counter() - t
        phase = float(re.findall(r"hashing and counting hashes: ([0-9.]+)", log.getvalue())[-1])
        return counts, phase, e2e

    runs = [("plain FASTQ, default (host packer)", fq, "a"), ("plain FASTQ, skip (raw bytes over PCIe)", fq, "skip"),
            ("BGZF, default", gz, "a"), ("BGZF, skip", gz, "skip")]
    for what, path, mode in runs:                                # warm: page cache, library, upload path
        run(path, mode)
    for rep in range(args.reps):
        for what, path, mode in runs:
            counts, phase, e2e = run(path, mode)
            print("rep %d  %-42s map phase %.3f s, end to end %.2f s, %d counts" % (rep, what, phase, e2e, int(counts.sum())), flush=True)
    os.remove(fq)
    os.remove(gz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=list(VARIANTS) + ["all"], default="all")
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--index-kmers", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cli", type=int, default=0, metavar="N_READS")
    ap.add_argument("--bgzf-reads", type=int, default=4_000_000, help="reads of the FASTQ that are also written as BGZF")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out-dir", default="/tmp/kmm_ambiguous")
    args = ap.parse_args()
    if args.cli:
        cli(args)
    else:
        kernels(args)


if __name__ == "__main__":
    main()
