#!/usr/bin/env python3
"""What the base-quality floor of the record-hits mode costs: the workload of profiles/record_hits/README.md — the
10 M-k-mer index and 1 M reads of 150 bases as one raw FASTQ chunk in HBM, "record_hits" 2 — in three configurations:
  parent   a build of the parent commit (KMM_LIB_PATH of a worker process; it has no floor)
  q0       this build, "record_hits_min_base_quality" 0: the kernels of the parent are launched, and nothing else
  q20      this build, the floor at 20: line starts + mark pass + the quality variant of the hit kernel
each as the hits mode alone (map_records + take_record_hits into device arrays) and with the keep mode on (half of the reads
are random bases and hit nothing: "record_keep" with min_hits 1 keeps the other half; the kept text is taken into a device
buffer).  The quality lines are a sequencer's in shape: every read is 'I' up to a tail whose length is drawn per read, and the
tail is '#' (Q2) — LOW_SHARE of all bases, stated in the output with the share measured on the chunk.

A library is loaded once per process, so every configuration runs in worker processes of its own: `rounds` rounds, the
libraries alternated inside every round, every worker with one warm-up pass and `reps` timed passes per leg, timed with device
events around calls that end in a synchronise.  The parent's legs give the run-to-run spread that q0 is held to.
    python tools/record_hits_qual_bench.py [--parent-lib PATH] [n_reads=1000000] [n_index=10000000] [reps=7] [rounds=2]
Without --parent-lib the parent's legs are reported as not measured."""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

L, K, Q = 150, 31, 20
LOW_SHARE = 0.08


def fastq_chunk(bases, n_reads, seed=3):
    """One row of 307 bytes per record: '@r', the bases, '+', 150 quality bytes; returns (chunk, share of low bytes)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    row = np.empty((n_reads, 3 + L + 3 + L + 1), dtype=np.uint8)
    row[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    row[:, 3:3 + L] = bases.reshape(n_reads, L)
    row[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    tail = np.minimum(rng.geometric(1.0 / (LOW_SHARE * L), size=n_reads) - 1, L)      # low bases at the end of the read
    qual = np.where(np.arange(L)[None, :] >= (L - tail)[:, None], ord("#"), ord("I")).astype(np.uint8)
    row[:, 6 + L:6 + 2 * L] = qual
    row[:, -1] = 10
    return row.reshape(-1), float((qual < 33 + Q).mean())


def worker(n_reads, n_index, reps):
    import torch
    from kmer_mapper_amd import _lib, synthetic as syn
    from kmer_mapper_amd.engine import DeviceIndex
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2).cpu().numpy().reshape(n_reads, L).copy()
    rng = np.random.Generator(np.random.PCG64(5))
    bases[1::2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=bases[1::2].shape)]   # every second read hits nothing
    chunk, share = fastq_chunk(bases.reshape(-1), n_reads)
    d_chunk = torch.from_numpy(chunk).cuda()
    dev = DeviceIndex.from_index(index, index.max_node_id())
    dt = getattr(torch, "uint32", torch.int32)
    d_hits = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_windows = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_text = torch.zeros(chunk.shape[0], dtype=torch.uint8, device="cuda")
    try:
        dev.get_param("record_hits_min_base_quality")
        floors = (0, Q)
    except ValueError:
        floors = (None,)                                                            # a build of the parent commit
    out = {"library": _lib.SO_PATH, "low_share": share, "legs": {}}

    def one(q, keep):
        if q is not None:
            dev.set_param("record_hits_min_base_quality", q)
        dev.set_param("record_hits", 2)
        if keep:
            dev.record_keep(True, min_hits=1)
        used, n = dev.map_records(d_chunk, fmt=_lib.FORMAT_FASTQ, k=K)
        assert (used, n) == (chunk.shape[0], n_reads)
        assert dev.take_record_hits(out=(d_hits, d_windows)) == n_reads
        kept = dev.take_kept_records(out=d_text)[1] if keep else None
        if keep:
            dev.record_keep(False)
        dev.set_param("record_hits", 0)
        return kept

    legs = [(q, keep) for keep in (False, True) for q in floors]
    times = {leg: [] for leg in legs}
    info = {}
    for rnd in range(reps + 1):
        for leg in (legs if rnd % 2 == 0 else legs[::-1]):
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            kept = one(*leg)                                                        # (ends in the takes' synchronise)
            t1.record()
            t1.synchronize()
            if rnd:
                times[leg].append(t0.elapsed_time(t1))
            info[leg] = (kept, int(d_windows.sum().item()), int(d_hits.sum().item()))
    for (q, keep), t in times.items():
        name = "%s%s" % ("parent" if q is None else "q%d" % q, " + keep" if keep else "")
        out["legs"][name] = {"ms": t, "kept": info[(q, keep)][0], "windows": info[(q, keep)][1], "hits": info[(q, keep)][2]}
    if floors != (None,):
        dev.set_timing(True)
        dev.get_stats(reset=True)
        one(Q, False)
        out["mark_pass_ms"] = dev.get_timing(_lib.KERNEL_RH_QUAL_MARK)[0]
        out["masked_bases"] = dev.get_param("quality_masked_bases")
    dev.close()
    print("__RESULT__" + json.dumps(out))


def main():
    args = sys.argv[1:]
    if args and args[0] == "--worker":
        return worker(*(int(a) for a in args[1:4]))
    parent = None
    if args and args[0] == "--parent-lib":
        parent, args = args[1], args[2:]
    n_reads, n_index, reps, rounds = (int(args[i]) if len(args) > i else d for i, d in enumerate((1_000_000, 10_000_000, 7, 2)))
    merged, meta = {}, {}
    libs = [parent, None] if parent is not None else [None]
    for rnd in range(rounds):
        for lib in (libs if rnd % 2 == 0 else libs[::-1]):                           # alternated: no library always runs first
            env = dict(os.environ)
            env.pop("KMM_LIB_PATH", None)
            if lib is not None:
                env["KMM_LIB_PATH"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", str(n_reads), str(n_index), str(reps)],
                               env=env, capture_output=True, text=True, timeout=900)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")), None)
            if p.returncode != 0 or line is None:
                print(p.stdout[-2000:], p.stderr[-4000:])
                raise SystemExit("worker failed (%d)" % p.returncode)
            res = json.loads(line[len("__RESULT__"):])
            for name, leg in res["legs"].items():
                merged.setdefault(name, dict(leg, ms=[]))["ms"] += leg["ms"]
            meta.update({k: v for k, v in res.items() if k != "legs"})
    print("%d reads of %d bases as FASTQ in HBM, index of %d k-mers, k = %d; quality bytes below Q%d: %.2f %% (planned %.0f %%)"
          % (n_reads, L, n_index, K, Q, 100 * meta["low_share"], 100 * LOW_SHARE))
    print("%d rounds x %d timed passes per leg, device events around calls that end in a synchronise" % (rounds, reps))
    for name in ("parent", "q0", "q%d" % Q, "parent + keep", "q0 + keep", "q%d + keep" % Q):
        if name not in merged:
            print("  %-14s not measured" % name)
            continue
        t = np.array(merged[name]["ms"])
        print("  %-14s median %8.3f ms   min %8.3f   max %8.3f   (n %d)   windows %d hits %d%s"
              % (name, np.median(t), t.min(), t.max(), t.shape[0], merged[name]["windows"], merged[name]["hits"],
                 "" if merged[name]["kept"] is None else "   kept %d" % merged[name]["kept"]))
    if "mark_pass_ms" in meta:
        print("  KMM_KERNEL_RH_QUAL_MARK (line starts + mark pass, one call with timing on): %.3f ms; quality_masked_bases %d"
              % (meta["mark_pass_ms"], meta["masked_bases"]))


if __name__ == "__main__":
    main()
