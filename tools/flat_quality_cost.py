#!/usr/bin/env python3
"""What a base-quality floor costs flat reads held in memory (kmm_map_reads_qual).

--mode prepass: ONE batch of 20 M reads of 150 bp resident in HBM, mapped with kmm_map_reads_uniform against a small index
(the pre-pass does not depend on the index) in one of four ways (--variant), for a run of its own under the profiler, one
variant per run, no counters:
    rocprofv3 --kernel-trace --stats -d OUT -o qual_41 -- python tools/flat_quality_cost.py --mode prepass --variant qual_41
    breaks_clean   util.ambiguous_skip_lut(), no N in the reads, the floor off: k_mark_breaks, the yardstick
    qual_41        default table, Q = 20, qualities that take all 41 values '!' .. 'I' (nine in ten from the upper half)
    qual_binned    default table, Q = 20, four binned values ('#' 3 %, '-' 7 %, '8' 20 %, 'F' 70 %)
    qual_high      default table, Q = 20, every byte 'I': the loads and the compare alone, no word of the bitset is written
Without the profiler it prints the whole call (wall clock between synchronisations) and the fraction masked.
--summarise DIR: the k_mark_* rows of every *kernel_stats*.csv under DIR, as ms and TB/s of the bytes the kernel reads.

--mode step: BASELINE configs[2]'s index (100 M k-mers) and one batch of 20 M reads of 150 bp, the whole step (wall clock
between synchronisations) with the floor off, at Q = 20 on qualities of 41 values (most windows die: fewer lookups) and at
Q = 20 on qualities that are all 'I' (every window survives: the price of the route alone), reads and qualities in HBM (--where hbm) or in pageable host
memory (--where host: with the floor off the host packer takes the bases; at Q = 20 both byte streams cross PCIe whole).
Not part of the product."""
import argparse
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L = 150
VARIANTS = ("breaks_clean", "qual_41", "qual_binned", "qual_high")


def qualities_on_device(n_reads, kind, seed):
    """uint8[n_reads * L] in HBM: "41" or "binned" (the distributions of tools/quality_cost.py), or "high": 'I' everywhere."""
    import torch
    if kind == "high":
        return torch.full((n_reads * L,), ord("I"), dtype=torch.uint8, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(seed)
    out = torch.empty((n_reads, L), dtype=torch.uint8, device="cuda")
    for a in range(0, n_reads, 2_000_000):                        # (blocks: the intermediates are 64-bit)
        n = min(n_reads, a + 2_000_000) - a
        p = torch.rand((n, L), device="cuda", generator=gen)
        if kind == "41":
            low = torch.randint(33, 74, (n, L), device="cuda", generator=gen)
            high = torch.randint(53, 74, (n, L), device="cuda", generator=gen)
            q = torch.where(p < 0.9, high, low)
        else:
            q = torch.where(p < 0.03, 35, torch.where(p < 0.10, 45, torch.where(p < 0.30, 56, 70)))
        out[a:a + n] = q.to(torch.uint8)
    return out.reshape(-1)


def timed(dev, call, q, steps, warmup):
    dev.set_param("min_base_quality", q)
    for _ in range(warmup):
        call()
    dev.synchronize()
    dev.reset()
    dev.get_stats(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    dev.synchronize()
    dt = (time.perf_counter() - t0) / steps
    lookups, _ = dev.get_stats()
    masked = dev.get_param("quality_masked_bases") // steps
    dev.set_param("min_base_quality", 0)
    return dt, lookups // steps, masked


def prepass(args):
    import torch
    from kmer_mapper_amd import synthetic as syn
    from kmer_mapper_amd.engine import DeviceIndex
    from kmer_mapper_amd.util import ambiguous_skip_lut
    index, g_ascii = syn.make_index_torch(args.prepass_index_kmers, k=31, seed=1)
    R = args.reads
    bases = syn.make_reads_torch(g_ascii, R, L, seed=1001, n_rate=0.0, lower_frac=0.0)
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        dev.set_param("path", 2)
        if args.variant == "breaks_clean":
            lut = torch.from_numpy(ambiguous_skip_lut()).cuda()
            call, q = (lambda: dev.map_reads_uniform(bases, R, L, 31, lut=lut)), 0
        else:
            quals = qualities_on_device(R, args.variant[5:], seed=7)
            call, q = (lambda: dev.map_reads_uniform(bases, R, L, 31, qualities=quals)), 20
        torch.cuda.synchronize()
        dt, lookups, masked = timed(dev, call, q, args.steps, args.warmup)
        print(json.dumps({"mode": "prepass", "variant": args.variant, "reads": R, "bases": R * L, "min_base_quality": q,
                          "call_ms": round(dt * 1e3, 3), "lookups_per_call": lookups, "masked_fraction": round(masked / (R * L), 4),
                          "flat_uniform_batches": dev.get_param("flat_uniform_batches")}), flush=True)


def summarise(args):
    for path in sorted(glob.glob(os.path.join(args.summarise, "**", "*kernel_stats*.csv"), recursive=True)):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "k_mark_" not in row["Name"]:
                    continue
                name = row["Name"].split("k_mark_")[1].split("(")[0]
                ms = float(row["AverageNs"]) / 1e6
                rate = "" if "starts" in name else ", %.2f TB/s of the %d bytes it reads" % (args.reads * L / ms / 1e9, args.reads * L)
                print("%-40s k_mark_%-16s %3d launches, average %.3f ms (min %.3f, max %.3f)%s"
                      % (os.path.basename(path), name, int(row["Calls"]), ms, float(row["MinNs"]) / 1e6, float(row["MaxNs"]) / 1e6, rate))


def step(args):
    import torch
    from kmer_mapper_amd import synthetic as syn
    from kmer_mapper_amd.engine import DeviceIndex
    index, g_ascii = syn.make_index_torch(args.index_kmers, k=31, seed=1)
    R = args.reads
    bases = syn.make_reads_torch(g_ascii, R, L, seed=1001, n_rate=0.0, lower_frac=0.0)
    quals, high = qualities_on_device(R, "41", seed=7), qualities_on_device(R, "high", seed=7)
    torch.cuda.synchronize()
    if args.where == "host":
        bases, quals, high = bases.cpu().numpy(), quals.cpu().numpy(), high.cpu().numpy()
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        for what, q, qu in (("kmm_map_reads_uniform", 0, None), ("kmm_map_reads_qual", 0, quals), ("kmm_map_reads_qual, 41 values", 20, quals),
                             ("kmm_map_reads_qual, all 'I'", 20, high)):
            before = dev.get_param("host_packed_calls"), dev.get_param("flat_uniform_batches")
            dt, lookups, masked = timed(dev, lambda: dev.map_reads_uniform(bases, R, L, 31, qualities=qu), q, args.steps, args.warmup)
            packed = dev.get_param("host_packed_calls") - before[0]
            print(json.dumps({"mode": "step", "where": args.where, "call": what, "min_base_quality": q, "reads": R,
                              "step_ms": round(dt * 1e3, 3), "lookups_per_step": lookups, "M_kmers_per_s": round(lookups / dt / 1e6, 1),
                              "masked_fraction": round(masked / (R * L), 4),
                              "bytes_over_pcie_per_step": 0 if args.where == "hbm" else 2 * R * L if q else R * L // 4 if packed else R * L,
                              "host_packed_calls": packed,
                              "flat_uniform_batches": dev.get_param("flat_uniform_batches") - before[1]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("prepass", "step"), default="prepass")
    ap.add_argument("--variant", choices=VARIANTS, default="qual_41")
    ap.add_argument("--where", choices=("hbm", "host"), default="hbm")
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--index-kmers", type=int, default=100_000_000)
    ap.add_argument("--prepass-index-kmers", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--summarise", metavar="DIR", help="print the k_mark_* rows of the profiler's *kernel_stats*.csv under DIR")
    args = ap.parse_args()
    if args.summarise:
        summarise(args)
    else:
        (prepass if args.mode == "prepass" else step)(args)


if __name__ == "__main__":
    main()
