#!/usr/bin/env python3
"""What kmm_read_hits costs: the 10 M-k-mer index of BASELINE configs[1] and 1 M reads of 150 bases resident
in HBM, three legs on the same batch:
  (a)  kmm_read_hits — through the uniform entry (read ids by division) and through the ragged entry (the same reads with
       their offsets: read ids by the search), hits alone and hits + windows;
  (b)  kmm_map_reads_uniform with "path" 1 up to kmm_synchronize: the same gathers, node counts instead of per-read sums;
  (c)  what a caller could do before the call existed: kmm_extract_kmers -> kmm_in_index -> a per-read sum on the host.
    python tools/read_hits_bench.py [n_reads=1000000] [n_index=10000000] [reps=9] [legs=abc|a]
One warm-up round, then `reps` rounds with the legs alternated inside every round; prints the median / min / max wall time per
leg and the ratios.  legs=a: kmm_read_hits alone — for a diagnostic build (KMM_LIB_PATH=... built with -DKMM_RH_STUB_SEARCH or
-DKMM_RH_STUB_REDUCE, whose outputs are wrong and are not checked)."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import _lib, synthetic as syn                  # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex, extract_kmers       # noqa: E402

L, K = 150, 31
_P = ctypes.c_void_p


def main():
    import torch
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    legs = sys.argv[4] if len(sys.argv) > 4 else "abc"
    stub = bool(os.environ.get("KMM_LIB_PATH"))
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2)
    offsets = torch.arange(n_reads + 1, dtype=torch.int64, device=bases.device) * L
    n_kmers = n_reads * (L - K + 1)
    dev = DeviceIndex.from_index(index, index.max_node_id())
    dev.set_param("path", 1)
    lib = _lib.lib()
    hits = torch.zeros(n_reads, dtype=torch.int32, device=bases.device)
    windows = torch.zeros(n_reads, dtype=torch.int32, device=bases.device)
    kmers = torch.zeros(n_kmers, dtype=torch.int64, device=bases.device)
    ptr = lambda t: _P(t.data_ptr())

    def read_hits(ragged, with_windows):
        _lib.check(lib.kmm_read_hits(dev._h, ptr(bases), ptr(offsets) if ragged else None, n_reads, L, K, 1000, 0, None, ptr(hits),
                                     ptr(windows) if with_windows else None))

    def map_reads():
        dev.map_reads_uniform(bases, n_reads, L, K)
        dev.synchronize()

    composed = {}

    def compose():
        extract_kmers(bases, offsets, K, out=kmers)
        present = dev.in_index(kmers)                               # uint8 per k-mer, on the host
        composed["hits"] = present.reshape(n_reads, L - K + 1).sum(axis=1, dtype=np.uint32)

    named = [("a  read_hits, uniform entry, hits", lambda: read_hits(False, False)),
             ("a  read_hits, uniform entry, hits + windows", lambda: read_hits(False, True)),
             ("a  read_hits, ragged entry, hits", lambda: read_hits(True, False)),
             ("a  read_hits, ragged entry, hits + windows", lambda: read_hits(True, True))]
    if "b" in legs:
        named.append(("b  map_reads_uniform, path 1", map_reads))
    if "c" in legs:
        named.append(("c  extract_kmers -> in_index -> host sum", compose))
    times = {name: [] for name, _ in named}
    for rnd in range(reps + 1):
        for name, fn in (named if rnd % 2 == 0 else named[::-1]):    # alternated: no leg always runs behind the same one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("library: %s%s" % (_lib.SO_PATH, "  (diagnostic build: outputs not checked)" if stub else ""))
    print("%d reads of %d bases (%d k-mers), index of %d k-mers, k = %d, %d rounds after one warm-up" % (n_reads, L, n_kmers, n_index, K, reps))
    med = {}
    for name, _ in named:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        print("  %-48s median %9.3f ms   min %9.3f   max %9.3f   (%.2f G k-mers/s)" % (name, med[name], t.min(), t.max(),
                                                                                       n_kmers / med[name] / 1e6))
    a = med[named[0][0]]
    if "b" in legs:
        print("  (a) / (b) = %.3f  (uniform entry, hits)   %.3f  (ragged entry, hits + windows)" %
              (a / med[named[4][0]], med[named[3][0]] / med[named[4][0]]))
    if "c" in legs:
        print("  (c) / (a) = %.1f" % (med[named[-1][0]] / a))
    if not stub:
        read_hits(True, True)
        h = hits.cpu().numpy().view(np.uint32)
        w = windows.cpu().numpy().view(np.uint32)
        assert (w == L - K + 1).all() and (h <= w).all()
        read_hits(False, False)
        assert np.array_equal(hits.cpu().numpy().view(np.uint32), h)
        if "c" in legs:                                              # the filter can only take hits away
            assert (h <= composed["hits"]).all() and int(composed["hits"].sum()) > 0
            read = lambda: _lib.check(lib.kmm_read_hits(dev._h, ptr(bases), None, n_reads, L, K, 65535, 0, None, ptr(hits), None))
            read()
            assert np.array_equal(hits.cpu().numpy().view(np.uint32), composed["hits"])
        print("  checked: uniform and ragged entries agree; hits at max frequency 65535 equal the composed route's; "
              "reads with a hit: %.1f %%" % (100.0 * (h > 0).mean()))
    dev.close()


if __name__ == "__main__":
    main()
