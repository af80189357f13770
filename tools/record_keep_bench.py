#!/usr/bin/env python3
"""What the record-keep mode costs: the 10 M-k-mer index of BASELINE configs[1] and 1 M reads of 150 bases as one
raw FASTQ chunk resident in HBM; every second read is random bases, so about half the reads have a hit.  Legs on that chunk:
  (a)  kmm_map_records with "record_hits" 2, kmm_take_record_hits into device arrays: the call there was before — run it at the
       parent commit too (KMM_LIB_PATH=<its build>, legs=a);
  (b)  the same with "record_keep" 1 and kmm_take_kept_records into a device buffer, under three rules: min_hits 1 (about
       half kept), min_hits 0 (all kept), min_hits 2^32 - 1 (none kept).  (b) - (a) is the price of the feature;
  (c)  the floor: a device-to-device copy of as many bytes as rule "half" kept, plus one read of the chunk (a sum over it as
       64-bit words), by device events;
  (d)  with legs containing "d": the command line — `select-reads` on the chunk as a .fq file against `read-hits --device-parser`
       on the same file, each a run of run_argument_parser in this process with its own index load and upload.
    python tools/record_keep_bench.py [n_reads=1000000] [n_index=10000000] [reps=9] [legs=abc]
One warm-up round, then `reps` rounds with the legs alternated inside every round; prints median / min / max per leg.  The
kernels alone (k_rk_flags, k_rec_scan1, k_super_scan, k_rk_scatter, k_rk_advance): run legs=b under
`rocprofv3 --kernel-trace --stats -- python tools/record_keep_bench.py ... 3 b`."""
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import _lib, synthetic as syn                  # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex                      # noqa: E402
from tools.record_hits_bench import K, L, fastq_chunk, report, run_rounds   # noqa: E402

RULES = (("half", 1), ("all", 0), ("none", (1 << 32) - 1))


def main():
    import torch
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    legs = sys.argv[4] if len(sys.argv) > 4 else "abc"
    has_keep = hasattr(_lib.lib(), "kmm_take_kept_records")
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2).cpu().numpy().reshape(n_reads, L).copy()
    rng = np.random.default_rng(3)
    bases[1::2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=bases[1::2].shape)]
    chunk = fastq_chunk(bases.reshape(-1), n_reads)
    d_chunk = torch.from_numpy(chunk).cuda()
    n_kmers = n_reads * (L - K + 1)
    dev = DeviceIndex.from_index(index, index.max_node_id())
    dt = getattr(torch, "uint32", torch.int32)
    d_hits = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_windows = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_text = torch.zeros(chunk.shape[0], dtype=torch.uint8, device="cuda")
    taken = {}

    def mode(min_hits):
        dev.record_hits(True, windows=True)
        if min_hits is not None:
            dev.record_keep(True, min_hits=min_hits)
        used, n = dev.map_records(d_chunk, fmt=_lib.FORMAT_FASTQ, k=K)
        assert (used, n) == (chunk.shape[0], n_reads)
        assert dev.take_record_hits(out=(d_hits, d_windows)) == n_reads
        if min_hits is not None:
            taken[min_hits] = dev.take_kept_records(out=d_text)
            dev.record_keep(False)
        dev.record_hits(False)

    named = []
    if "a" in legs:
        named.append(("a  map_records, record_hits 2, take hits", lambda: mode(None)))
    if "b" in legs and has_keep:
        named += [("b  ... + record_keep 1, %s kept, take text" % name, (lambda m: lambda: mode(m))(m)) for name, m in RULES]
    print("library: %s" % _lib.SO_PATH)
    print("%d reads of %d bases as FASTQ (%d bytes, %d k-mers), index of %d k-mers, k = %d, %d rounds after one warm-up"
          % (n_reads, L, chunk.shape[0], n_kmers, n_index, K, reps))
    if named:
        report(named, run_rounds(named, reps, torch.cuda.synchronize), n_kmers)
    if "b" in legs and has_keep:
        for name, m in RULES:
            print("  rule %-5s kept %d bytes of %d records" % ((name,) + taken[m]))
        mode(1)
        hits = d_hits.cpu().numpy().view(np.uint32)
        keep = hits >= 1
        want = chunk.reshape(n_reads, -1)[keep].reshape(-1)
        assert taken[1] == (want.shape[0], int(keep.sum())) and np.array_equal(d_text[:want.shape[0]].cpu().numpy(), want)
        print("  checked: the kept text equals the rows of the chunk whose entry has a hit; reads with a hit: %.1f %%" % (100.0 * keep.mean()))
    if "c" in legs and has_keep and 1 in taken:
        n_kept = taken[1][0]
        src, dst = d_chunk[:n_kept], torch.empty(n_kept, dtype=torch.uint8, device="cuda")
        words = d_chunk[:chunk.shape[0] // 8 * 8].view(torch.int64)
        ms = {"copy": [], "read": []}
        for rnd in range(reps + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            words.sum()
            ev[2].record()
            torch.cuda.synchronize()
            if rnd:
                ms["copy"].append(ev[0].elapsed_time(ev[1]))
                ms["read"].append(ev[1].elapsed_time(ev[2]))
        print("  c  floor: device-to-device copy of %d bytes: median %.3f ms; one read of the chunk (%d bytes): median %.3f ms"
              % (n_kept, float(np.median(ms["copy"])), chunk.shape[0], float(np.median(ms["read"]))))
    dev.close()
    if "d" in legs and has_keep:
        command_line(index, chunk, n_kmers, max(3, reps // 3))


def command_line(index, chunk, n_kmers, reps):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    import logging
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        npz, fq, out, kept = (os.path.join(tmp, n) for n in ("index.npz", "reads.fq", "out", "kept.fq"))
        (index.to_host() if hasattr(index, "to_host") else index).to_file(npz)
        chunk.tofile(fq)
        common = ["-i", npz, "-k", str(K), "-f", fq]
        named = [("d  read-hits --device-parser on .fq", lambda: run_argument_parser(["read-hits"] + common + ["-o", out, "--device-parser"])),
                 ("d  select-reads on .fq", lambda: run_argument_parser(["select-reads"] + common + ["-o", kept]))]
        logging.disable(logging.INFO)
        times = run_rounds(named, reps, torch.cuda.synchronize)
        logging.disable(logging.NOTSET)
        print("command line on %d bytes, index load and upload included, %d rounds after one warm-up; kept.fq: %d bytes"
              % (chunk.shape[0], reps, os.path.getsize(kept)))
        report(named, times, n_kmers)


if __name__ == "__main__":
    main()
