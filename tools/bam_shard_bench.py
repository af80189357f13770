#!/usr/bin/env python3
"""What sharding a BAM file costs a rank before it maps, and that the single-rank BAM route has not moved (DESIGN 4.14,
profiles/bam_shard/).
    python tools/bam_shard_bench.py [n_reads=4000000] [n_index=10000000] [out_dir=/tmp/kmm_bam_shard] [other_tree]
The set-up is tools/bam_e2e.py's (the same reads as unaligned BAM, level 6, members of 0xFF00 bytes).  Then:
  * with other_tree (a check-out of another commit, built): `kmer_mapper map -f reads.bam` from that tree and from this one,
    alternated three times, a fresh process each — the CLI's map phase ("hashing and counting"), the time in kmm_map_bam, the
    index upload; the two count vectors must be equal;
  * kmm_bam_find_record_start at the default window (1 MiB of compressed bytes from the middle of the file), six calls, wall
    time each (KMM_VERBOSE=1 adds the library's split: copy + inflate + CRC, resync kernel);
  * bgzf_ranges.rank_member_range_bam for ranks of 2 and of 8: the header and both boundaries, wall time."""
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from kmer_mapper_amd import bgzf_ranges, synthetic as syn       # noqa: E402
from tools.bam_e2e import bam_payload, bgzf_file                # noqa: E402
from tools.bgzf_e2e import make_fastq                            # noqa: E402

_ONCE = ("import sys; sys.path.insert(0, sys.argv[1]); "
         "from kmer_mapper_amd.command_line_interface import run_argument_parser; "
         "run_argument_parser(['map', '-i', sys.argv[2], '-f', sys.argv[3], '-o', sys.argv[4]])")


def cli_once(tree, idx, bam, out, tag):
    time.sleep(4)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, "-c", _ONCE, tree, idx, bam, out], capture_output=True, text=True,
                       cwd=tree)
    if r.returncode != 0:
        print(r.stdout[-3000:], r.stderr[-3000:], flush=True)
        sys.exit(3)
    phase = float(re.search(r"Time spent only on hashing and counting hashes: ([0-9.]+)", r.stdout).group(1)) * 1e3
    print("CLI %s: map phase %.1f ms; %s ms in kmm_map_bam; index resident after %s s" % (
        tag, phase, re.search(r"([0-9.]+) ms in kmm_map_bam", r.stdout).group(1),
        re.search(r"Index resident in HBM after ([0-9.]+) sec", r.stdout).group(1)), flush=True)
    return phase


def main():
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 4_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    d = sys.argv[3] if len(sys.argv) > 3 else "/tmp/kmm_bam_shard"
    other = sys.argv[4] if len(sys.argv) > 4 else None
    L = 150
    os.makedirs(d, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    fq = os.path.join(d, "reads.fq")
    make_fastq(fq, bases, n_reads, L)
    raw = open(fq, "rb").read()
    os.remove(fq)
    bam, idx = os.path.join(d, "reads.bam"), os.path.join(d, "index.npz")
    payload = bam_payload(raw, n_reads, L)
    bgzf_file(bam, payload)
    index.to_file(idx)
    print("setup %.1f s: BAM %.2f GB inflated -> %.2f GB" % (time.time() - t0, len(payload) / 1e9, os.path.getsize(bam) / 1e9), flush=True)
    del raw, payload, bases
    same = True
    if other:
        times = {"other": [], "this": []}
        for _ in range(3):
            times["other"].append(cli_once(other, idx, bam, os.path.join(d, "out_other"), "other"))
            times["this"].append(cli_once(ROOT, idx, bam, os.path.join(d, "out_this"), "this"))
        for k, t in times.items():
            print("CLI BAM route, %s tree: map phase ms %s, median %.1f, min %.1f, max %.1f" % (k, ["%.1f" % x for x in t], np.median(t),
                                                                                              min(t), max(t)), flush=True)
        same = bool(np.array_equal(np.load(os.path.join(d, "out_other.npy")), np.load(os.path.join(d, "out_this.npy"))))
        print("counts other == this:", same, flush=True)
    from kmer_mapper_amd.engine import DeviceIndex
    small, _ = syn.make_index(20000, seed=3)
    comp = np.fromfile(bam, np.uint8)
    raw_b = comp.tobytes()
    with DeviceIndex.from_index(small, small.max_node_id()) as dev:
        n_ref, member, skip = dev.bam_header(comp[:1 << 20])
        print("header: n_ref %d, first record at member %d + %d" % (n_ref, member, skip), flush=True)
        m, _ = bgzf_ranges.member_at_or_after(raw_b, len(raw_b) // 2)
        for i in range(6):
            t = time.perf_counter()
            ans = dev.bam_find_record_start(comp[m:m + (1 << 20)], n_ref)
            print("kmm_bam_find_record_start, 1 MiB window, call %d: %.2f ms -> %s" % (i, (time.perf_counter() - t) * 1e3, ans), flush=True)
        for world in (2, 8):
            for r in (1, world - 1):
                t = time.perf_counter()
                share = bgzf_ranges.rank_member_range_bam(dev, raw_b, r, world)
                print("rank_member_range_bam, rank %d of %d: %.1f ms -> %s" % (r, world, (time.perf_counter() - t) * 1e3, share), flush=True)
    os.remove(bam)
    os.remove(idx)
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
