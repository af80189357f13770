#!/usr/bin/env python3
"""What kmm_read_nodes costs: the 10 M-k-mer index of BASELINE configs[1] and 1 M reads of 150 bases resident in
HBM, on the same batch:
  (h)  kmm_read_hits, uniform entry, hits alone — the yardstick: one walk, no table.  With KMM_LIB_PATH set to a library built
       at the parent commit and legs=h, the same leg measures that build on the same box;
  (n)  kmm_read_nodes, uniform and ragged entry, all five outputs and best_node alone — against three node maps over the same
       k-mers: the index as it is (every k-mer its own node: ~30 cells per read); one node per stretch of 150 genome bases, with
       a batch of reads cut at the stretch boundaries, so that every read sits on one node; and every entry under node 0 (all
       reads share one node);
    python tools/read_nodes_bench.py [n_reads=1000000] [n_index=10000000] [reps=9] [legs=hn|h|n]
One warm-up round, then `reps` rounds with the legs alternated inside every round; prints the median / min / max wall time per
leg and the ratios to (h)."""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import _lib, synthetic as syn                  # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex                      # noqa: E402

L, K = 150, 31
_P = ctypes.c_void_p


def main():
    import torch
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    legs = sys.argv[4] if len(sys.argv) > 4 else "hn"
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2)
    offsets = torch.arange(n_reads + 1, dtype=torch.int64, device=bases.device) * L
    n_kmers = n_reads * (L - K + 1)
    lib = _lib.lib()
    ptr = lambda t: None if t is None else _P(t.data_ptr())
    i32 = lambda: torch.zeros(n_reads, dtype=torch.int32, device=bases.device)
    hits, outs = i32(), [i32() for _ in range(5)]
    rounds = ctypes.c_int64(0)

    def with_nodes(nodes, max_node):
        return syn.DeviceSyntheticIndex(index._hashes_to_index, index._n_kmers, index._kmers, nodes, index._frequencies, index._modulo,
                                        max_node)

    # (node i of the synthetic index is the k-mer at genome position 4 i; the few planted duplicates keep their random nodes,
    # so a read of the stretch batch may see a second node now and then: the check below prints how often)
    maps = [("own node per k-mer", index)]
    if "n" in legs:
        maps += [("one node per read", with_nodes(((index._nodes.long() * 4) // L).int(), (index.max_node_id() * 4) // L)),
                 ("one node", with_nodes(torch.zeros_like(index._nodes), 0))]
    devs = [(name, DeviceIndex.from_index(ix, ix.max_node_id())) for name, ix in maps]
    # reads cut at the stretch boundaries, unaltered: all windows of a read lie in one stretch
    g = torch.Generator(device=bases.device)
    g.manual_seed(3)
    starts = torch.randint(0, (genome.shape[0] - L) // L, (n_reads,), generator=g, device=bases.device) * L
    stretch_bases = genome[starts[:, None] + torch.arange(L, device=bases.device)[None, :]].reshape(-1).contiguous()
    batch_of = {"one node per read": stretch_bases}

    def read_hits(dev):
        _lib.check(lib.kmm_read_hits(dev._h, ptr(bases), None, n_reads, L, K, 1000, 0, None, ptr(hits), None))

    def read_nodes(dev, ragged, all_outputs, batch=None):
        want = outs if all_outputs else [outs[0], None, None, None, None]
        _lib.check(lib.kmm_read_nodes(dev._h, ptr(bases if batch is None else batch), ptr(offsets) if ragged else None, n_reads, L, K, 1000, 0, None, 0,
                                      *[ptr(t) for t in want], ctypes.byref(rounds)))

    named = []
    if "h" in legs:
        named.append(("h  read_hits, uniform entry, hits", lambda: read_hits(devs[0][1])))
    if "n" in legs:
        for name, dev in devs:
            named.append(("n  read_nodes, uniform, 5 outputs, %s" % name,
                          lambda dev=dev, name=name: read_nodes(dev, False, True, batch_of.get(name))))
        named.append(("n  read_nodes, uniform, best_node alone, %s" % devs[0][0], lambda: read_nodes(devs[0][1], False, False)))
        named.append(("n  read_nodes, ragged, 5 outputs, %s" % devs[0][0], lambda: read_nodes(devs[0][1], True, True)))
    times = {name: [] for name, _ in named}
    for rnd in range(reps + 1):
        for name, fn in (named if rnd % 2 == 0 else named[::-1]):    # alternated: no leg always runs behind the same one
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print("library: %s" % _lib.SO_PATH)
    print("%d reads of %d bases (%d k-mers), index of %d k-mers, k = %d, %d rounds after one warm-up" % (n_reads, L, n_kmers, n_index, K, reps))
    med = {}
    for name, _ in named:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        print("  %-58s median %9.3f ms   min %9.3f   max %9.3f" % (name, med[name], t.min(), t.max()))
    if "h" in legs and "n" in legs:
        for name, _ in named[1:]:
            print("  %-58s / (h) = %.2f" % (name, med[name] / med[named[0][0]]))
    if "n" in legs:                                                  # the answers, against each other and against read_hits
        for name, dev in devs:
            read_nodes(dev, False, True, batch_of.get(name))
            best_node, best, second, total, nn = (t.cpu().numpy() for t in outs)
            n_rounds = rounds.value
            read_nodes(dev, True, True, batch_of.get(name))
            assert all(np.array_equal(a, t.cpu().numpy()) for a, t in zip((best_node, best, second, total, nn), outs))
            assert ((best_node >= 0) == (total > 0)).all() and (second <= best).all() and (best <= total).all() and (nn <= total).all()
            if name == "one node per read":
                assert (nn[total > 0] == 1).mean() > 0.9 and (best_node[nn == 1] == (starts.cpu().numpy() // L)[nn == 1]).all()
            if name == "one node":
                assert (best_node <= 0).all() and (best == total).all() and (nn <= 1).all()
            print("  %-20s rounds %d, votes %d, reads with a vote %.1f %%, mean distinct nodes %.2f, reads with a tie %.2f %%" %
                  (name, n_rounds, int(total.astype(np.int64).sum()), 100.0 * (total > 0).mean(), nn[total > 0].mean(),
                   100.0 * ((best == second) & (best > 0)).mean()))
    for _, dev in devs:
        dev.close()


if __name__ == "__main__":
    main()
