#!/usr/bin/env python3
"""What a base-quality floor ("min_base_quality", `--min-base-quality`) costs.

--mode compaction (default): census + compaction of 1 GiB of FASTQ resident in HBM, per kmm_map_records call (wall clock
between synchronisations, "debug_records_copy_stream" = the compaction kernels alone, nothing mapped), with the floor off
and with Q = 20, on two synthetic files: qualities that take all 41 values '!' .. 'I' (nine in ten from the upper half) and
four binned values.  On a build without the parameter (the parent: KMM_LIB_PATH=build_ab/libkmm_parent.so) the floor-off
rows alone are measured.
--mode step: BASELINE configs[2]'s index (100 M k-mers) and ONE batch of 20 M reads of 150 bp as FASTQ resident in HBM,
the whole step (compaction plus the three passes) with the floor off and on.
Per-kernel times come from a run of its own under the profiler (no counters in that run):
    rocprofv3 --kernel-trace --stats -d OUT -o q20 -- python tools/quality_cost.py --mode step
Not part of the product."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import synthetic as syn                     # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex                    # noqa: E402

L = 150
HEAD = b"@read/0000000001\n"


def fastq_on_device(n_reads, qualities, seed, g_ascii=None):
    """n_reads records of 150 bases as one uint8 tensor in HBM; qualities: "41" or "binned".  g_ascii: draw the reads from
    this genome (ASCII, on the device) instead of at random."""
    import torch
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rec_len = len(HEAD) + L + 3 + L + 1
    rec = torch.empty((n_reads, rec_len), dtype=torch.uint8, device="cuda")
    rec[:, :len(HEAD)] = torch.frombuffer(bytearray(HEAD), dtype=torch.uint8).cuda()
    s0 = len(HEAD)
    acgt = torch.frombuffer(bytearray(b"ACGT"), dtype=torch.uint8).cuda()
    rec[:, s0 + L:s0 + L + 3] = torch.frombuffer(bytearray(b"\n+\n"), dtype=torch.uint8).cuda()
    rec[:, -1] = 10
    for a in range(0, n_reads, 2_000_000):                        # (blocks: the intermediates are 64-bit)
        n = min(n_reads, a + 2_000_000) - a
        if g_ascii is None:
            seq = acgt[torch.randint(0, 4, (n, L), device="cuda", generator=gen)]
        else:
            starts = torch.randint(0, g_ascii.shape[0] - L, (n, 1), device="cuda", generator=gen)
            seq = g_ascii[starts + torch.arange(L, device="cuda")]
        rec[a:a + n, s0:s0 + L] = seq
        p = torch.rand((n, L), device="cuda", generator=gen)
        if qualities == "41":
            low = torch.randint(33, 74, (n, L), device="cuda", generator=gen)
            high = torch.randint(53, 74, (n, L), device="cuda", generator=gen)
            q = torch.where(p < 0.9, high, low)
        else:                                                     # '#' 3 %, '-' 7 %, '8' 20 %, 'F' 70 %
            q = torch.where(p < 0.03, 35, torch.where(p < 0.10, 45, torch.where(p < 0.30, 56, 70)))
        rec[a:a + n, s0 + L + 3:s0 + 2 * L + 3] = q.to(torch.uint8)
    return rec.reshape(-1)


def has_floor(dev):
    try:
        dev.get_param("min_base_quality")
        return True
    except ValueError:
        return False


def timed(dev, raw, q, steps, warmup):
    if q:
        dev.set_param("min_base_quality", q)
    for _ in range(warmup):
        dev.map_records(raw, fmt=4, k=31)
    dev.synchronize()
    dev.reset()
    dev.get_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        used, n_rec = dev.map_records(raw, fmt=4, k=31)
    dev.synchronize()
    dt = (time.perf_counter() - t0) / steps
    lookups, _ = dev.get_stats()
    masked = dev.get_param("quality_masked_bases") // steps if q else 0
    if q:
        dev.set_param("min_base_quality", 0)
    assert used == raw.shape[0], (used, raw.shape[0])
    return dt, n_rec, lookups // steps, masked


def compaction(args):
    import torch
    index, _ = syn.make_index_torch(1_000_000, k=31, seed=1)
    n_reads = (1 << 30) // (len(HEAD) + 2 * L + 4)
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        floors = (0, 20) if has_floor(dev) else (0,)
        dev.set_param("path", 2)
        dev.set_param("debug_records_copy_stream", 1)             # compaction alone: the passes are not launched
        for qualities in ("41", "binned"):
            raw = fastq_on_device(n_reads, qualities, seed=7)
            torch.cuda.synchronize()
            for q in floors:
                dt, n_rec, _, masked = timed(dev, raw, q, args.steps, args.warmup)
                print(json.dumps({"mode": "compaction", "qualities": qualities, "min_base_quality": q, "bytes": raw.shape[0], "reads": n_rec,
                                  "ms_per_call": round(dt * 1e3, 3), "ms_per_GiB": round(dt * 1e3 * (1 << 30) / raw.shape[0], 3),
                                  "masked_fraction": round(masked / (n_rec * L), 4)}), flush=True)
            del raw


def step(args):
    import torch
    index, g_ascii = syn.make_index_torch(args.index_kmers, k=31, seed=1)
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        floors = (0, 20) if has_floor(dev) else (0,)
        raw = fastq_on_device(args.reads, "41", seed=9, g_ascii=g_ascii)
        torch.cuda.synchronize()
        for q in floors:
            dt, n_rec, lookups, masked = timed(dev, raw, q, args.steps, args.warmup)
            print(json.dumps({"mode": "step", "min_base_quality": q, "reads": n_rec, "bytes": raw.shape[0], "step_ms": round(dt * 1e3, 3),
                              "lookups_per_step": lookups, "M_kmers_per_s": round(lookups / dt / 1e6, 1),
                              "masked_fraction": round(masked / (n_rec * L), 4), "radix_batches": dev.get_param("radix_batches"),
                              "flat_uniform_batches": dev.get_param("flat_uniform_batches")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("compaction", "step"), default="compaction")
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--index-kmers", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=None, help="timed calls (default: 200 compaction calls, 20 whole steps)")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if args.steps is None:
        args.steps = 200 if args.mode == "compaction" else 20
    (compaction if args.mode == "compaction" else step)(args)


if __name__ == "__main__":
    main()
