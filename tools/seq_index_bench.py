#!/usr/bin/env python3
"""What kmm_seq_index_build costs against the route a caller could compose before it existed, on two inputs:
  random   `n_bases` of random sequence in `n_seqs` sequences;
  repeat   the same with a tenth of it (one stretch) replaced by one repeated 5-base motif.
Legs, host arrays in and host arrays out, every sequence node 0 (the --single-node index of select-reads: the composed route
has no node per k-mer to offer), one strand, k = 31:
  new        engine.index_from_sequences
  composed   engine.extract_kmers -> np.unique(return_index) on the host, first indices sorted -> engine.build_index with the
             modulo the new route chose
    python tools/seq_index_bench.py [n_bases=100000000] [n_seqs=1000] [reps=3] [legs=new,composed] [inputs=random,repeat]
One warm-up build of a small input, then `reps` rounds with the legs alternated inside every round; prints the median / min /
max wall time per leg and input, and fails unless both legs give the same five arrays.  Under rocprofv3 run one input and
legs=new: the kernel stats then belong to that input."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import engine           # noqa: E402

K = 31


def make_input(which, n_bases, n_seqs, seed=5):
    rng = np.random.default_rng(seed)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n_bases, dtype=np.uint8)]
    if which == "repeat":
        a, n = n_bases // 3, n_bases // 10
        bases[a:a + n] = np.resize(np.frombuffer(b"ACGTT", dtype=np.uint8), n)
    cuts = np.sort(rng.integers(1, n_bases, size=n_seqs - 1))
    offsets = np.concatenate([[0], cuts, [n_bases]]).astype(np.int64)
    return np.ascontiguousarray(bases), offsets


def leg_new(bases, offsets, nodes):
    return engine.index_from_sequences(bases, offsets, k=K, nodes=nodes)


def leg_composed(bases, offsets, modulo):
    kmers = engine.extract_kmers(bases, offsets, K)
    _, first = np.unique(kmers, return_index=True)
    first.sort()
    d = kmers[first]
    return engine.build_index(d, np.zeros(d.shape[0], dtype=np.int32), modulo) + (modulo,)


def main():
    arg = lambda i, d: sys.argv[i] if len(sys.argv) > i else d
    n_bases, n_seqs, reps = int(arg(1, 100_000_000)), int(arg(2, 1000)), int(arg(3, 3))
    legs, inputs = arg(4, "new,composed").split(","), arg(5, "random,repeat").split(",")
    wb, wo = make_input("random", 200_000, 10)
    warm = leg_new(wb, wo, np.zeros(10, dtype=np.int32))
    if "composed" in legs:
        leg_composed(wb, wo, warm[5])
    for which in inputs:
        bases, offsets = make_input(which, n_bases, n_seqs)
        nodes = np.zeros(n_seqs, dtype=np.int32)
        times = {leg: [] for leg in legs}
        last = {}
        modulo = None
        for _ in range(reps):
            for leg in legs:
                if leg == "composed" and modulo is None:
                    modulo = leg_new(bases, offsets, nodes)[5]
                t0 = time.perf_counter()
                last[leg] = leg_new(bases, offsets, nodes) if leg == "new" else leg_composed(bases, offsets, modulo)
                times[leg].append(time.perf_counter() - t0)
                if leg == "new":
                    modulo = last[leg][5]
        info = {}
        engine.index_from_sequences(bases, offsets, k=K, nodes=nodes, info=info)
        print("%s: %d bases in %d sequences, %d windows, %d entries, modulo %d" % (which, n_bases, n_seqs, info["n_windows"],
                                                                                  info["n_entries"], info["modulo"]), flush=True)
        for leg in legs:
            t = sorted(times[leg])
            print("  %-9s median %.3f s  min %.3f  max %.3f  (%d runs)" % (leg, t[len(t) // 2], t[0], t[-1], len(t)), flush=True)
        if len(legs) == 2:
            same = all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(last["new"], last["composed"]))
            print("  the two legs give the same arrays: %s; new / composed = %.3f" % (same, sorted(times["new"])[len(times["new"]) // 2]
                                                                                     / sorted(times["composed"])[len(times["composed"]) // 2]), flush=True)
            if not same:
                sys.exit("seq_index_bench: the legs differ on input %s" % which)


if __name__ == "__main__":
    main()
