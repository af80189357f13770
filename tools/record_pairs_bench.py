#!/usr/bin/env python3
"""What keeping mates together costs: the 10 M-k-mer index of BASELINE configs[1] and 1 M reads of 150 bases —
500 k pairs, the mates of every second pair random bases, so about half the pairs have a hit — resident in HBM as one interleaved
FASTQ chunk and as its two de-interleaved halves.  Legs, every one with its takes into device buffers:
  (a)  the interleaved chunk through kmm_map_records with "record_keep" 1, every record by itself: the call there was before —
       run it at the parent commit too (KMM_LIB_PATH=<its build>, legs=ac);
  (b)  the same chunk with "record_pairs" 1;
  (c)  the two halves as two unpaired calls (parent and this build);
  (d)  the two halves through kmm_map_record_pairs;
  (e)  (d) with one record more in the first half, so that the call cuts it (k_rec_cut and its second synchronisation).
    python tools/record_pairs_bench.py [n_reads=1000000] [n_index=10000000] [reps=9] [legs=abcde]
One warm-up round, then `reps` rounds with the legs alternated inside every round; prints median / min / max per leg.  The kernels
alone: `rocprofv3 --kernel-trace --stats -- python tools/record_pairs_bench.py ... 3 bd`."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import _lib, synthetic as syn                  # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex                      # noqa: E402
from tools.record_hits_bench import K, L, fastq_chunk, report, run_rounds   # noqa: E402


def main():
    import torch
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    legs = sys.argv[4] if len(sys.argv) > 4 else "abcde"
    has_pairs = hasattr(_lib.lib(), "kmm_map_record_pairs")
    n_reads -= n_reads % 4
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2).cpu().numpy().reshape(n_reads, L).copy()
    rng = np.random.default_rng(3)
    for lane in (2, 3):                                             # pairs 1, 3, 5, ...: both mates random bases
        bases[lane::4] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=bases[lane::4].shape)]
    chunk = fastq_chunk(bases.reshape(-1), n_reads)
    rows = chunk.reshape(n_reads, -1)
    half = [np.ascontiguousarray(rows[0::2]).reshape(-1), np.ascontiguousarray(rows[1::2]).reshape(-1)]
    longer = np.concatenate([half[0], rows[0]])
    d_chunk = torch.from_numpy(chunk).cuda()
    d_half = [torch.from_numpy(h).cuda() for h in half]
    d_longer = torch.from_numpy(longer).cuda()
    n_kmers = n_reads * (L - K + 1)
    dev = DeviceIndex.from_index(index, index.max_node_id())
    dt = getattr(torch, "uint32", torch.int32)
    d_hits = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_windows = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_text = torch.zeros(chunk.shape[0], dtype=torch.uint8, device="cuda")
    d_text2 = torch.zeros(chunk.shape[0], dtype=torch.uint8, device="cuda")
    taken = {}

    def one_file(pairs):
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        if pairs:
            dev.record_pairs(True)
        used, n = dev.map_records(d_chunk, fmt=_lib.FORMAT_FASTQ, k=K)
        assert (used, n) == (chunk.shape[0], n_reads)
        assert dev.take_record_hits(out=(d_hits, d_windows)) == n_reads
        taken["b" if pairs else "a"] = dev.take_kept_records(out=d_text)
        if pairs:
            dev.record_pairs(False)
        dev.record_keep(False)
        dev.record_hits(False)

    def two_calls():
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        for i, (d, out) in enumerate(zip(d_half, (d_text, d_text2))):
            used, n = dev.map_records(d, fmt=_lib.FORMAT_FASTQ, k=K)
            assert (used, n) == (half[i].shape[0], n_reads // 2)
            assert dev.take_record_hits(out=(d_hits, d_windows)) == n_reads // 2
            taken["c%d" % i] = dev.take_kept_records(out=out)
        dev.record_keep(False)
        dev.record_hits(False)

    def two_files(first, leg):
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        assert dev.map_record_pairs(first, d_half[1], fmt=_lib.FORMAT_FASTQ, k=K) == (half[0].shape[0], half[1].shape[0], n_reads // 2)
        assert dev.take_record_hits(out=(d_hits, d_windows)) == n_reads
        taken[leg] = (dev.take_kept_mates(0, out=d_text), dev.take_kept_mates(1, out=d_text2))
        dev.record_keep(False)
        dev.record_hits(False)

    named = []
    if "a" in legs:
        named.append(("a  interleaved, record_keep 1, every record by itself", lambda: one_file(False)))
    if "b" in legs and has_pairs:
        named.append(("b  interleaved, record_pairs 1", lambda: one_file(True)))
    if "c" in legs:
        named.append(("c  two halves, two unpaired calls", two_calls))
    if "d" in legs and has_pairs:
        named.append(("d  two halves, kmm_map_record_pairs", lambda: two_files(d_half[0], "d")))
    if "e" in legs and has_pairs:
        named.append(("e  ... the first half one record longer (cut)", lambda: two_files(d_longer, "e")))
    print("library: %s" % _lib.SO_PATH)
    print("%d reads of %d bases as FASTQ (%d bytes, %d k-mers), index of %d k-mers, k = %d, %d rounds after one warm-up"
          % (n_reads, L, chunk.shape[0], n_kmers, n_index, K, reps))
    report(named, run_rounds(named, reps, torch.cuda.synchronize), n_kmers)
    for leg, what in sorted(taken.items()):
        print("  leg %-2s kept (bytes, records): %s" % (leg, what))
    if "b" in taken:                                                # the kept text: the rows of the pairs with a hit in either mate
        one_file(True)
        hits = d_hits.cpu().numpy().view(np.uint32)
        keep = np.repeat((hits[0::2] >= 1) | (hits[1::2] >= 1), 2)
        want = rows[keep].reshape(-1)
        assert taken["b"] == (want.shape[0], int(keep.sum())) and np.array_equal(d_text[:want.shape[0]].cpu().numpy(), want)
        print("  checked: leg b kept the rows of the pairs with a hit in either mate: %.1f %% of the pairs" % (100.0 * keep.mean()))
    if "d" in taken:
        two_files(d_half[0], "d")
        hits = d_hits.cpu().numpy().view(np.uint32)
        keep = (hits[0::2] >= 1) | (hits[1::2] >= 1)
        for i, d in enumerate((d_text, d_text2)):
            want = rows[i::2][keep].reshape(-1)
            assert taken["d"][i] == (want.shape[0], int(keep.sum())) and np.array_equal(d[:want.shape[0]].cpu().numpy(), want)
        print("  checked: leg d kept the same pairs in both queues")
    dev.close()


if __name__ == "__main__":
    main()
