#!/usr/bin/env python3
"""Rehearsal of the multi-rank CLI flow on SAM input, on a 1-GPU box (tests/test_gpu_sam.py runs it):
   python tools/sam_two_rank_rehearsal.py --prepare DIR [Q]        writes the index, the reads as plain / BGZF / gzip SAM and
                                                                   the one-rank counts (the oracle's) into DIR; Q > 0: the reads
                                                                   get qualities of all 41 values, the counts are those of a
                                                                   floor Q, and the ranks map with --min-base-quality Q
                                                                   --use-record-qual
   RANK=r WORLD_SIZE=N MASTER_ADDR=127.0.0.1 MASTER_PORT=p KMM_DIST_BACKEND=gloo python tools/sam_two_rank_rehearsal.py DIR
                                                                   one rank: the CLI on each file, rank 0 compares
A plain SAM file is split by byte ranges (reads_io.rank_byte_range), a BGZF one by member ranges (bgzf_ranges.rank_member_range),
a plain gzip one by chunk round-robin cut with records_cut("sam"); the counts are summed over gloo."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import reads_io, synthetic as syn                      # noqa: E402
from kmer_mapper_amd.util import ReadBatch                                  # noqa: E402

FILES = ("reads.sam", "reads_bgzf.sam.gz", "reads_gz.sam.gz")


def split_at_low(bases, offs, low):
    """The reads with every base of `low` dropped and a read boundary where it stood: what a masked base is defined to be."""
    new_pos = np.zeros(len(bases) + 1, np.int64)
    np.cumsum(~low, out=new_pos[1:])
    bounds = np.concatenate([new_pos[offs], new_pos[np.flatnonzero(low) + 1], [0, new_pos[-1]]])
    return np.ascontiguousarray(bases[~low]), np.unique(bounds).astype(np.int64)


def prepare(d, min_q=0):
    index, genome = syn.make_index(20000, seed=7)
    bases, offs = syn.make_ragged_reads(genome, 6000 if min_q else 30000, 0, 220, seed=8)
    batch = ReadBatch(bases, offs)
    header = b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:c%d\tLN:1000\n" % i for i in range(2000))
    index.to_file(os.path.join(d, "index.npz"))
    quals = None
    if min_q:
        q = np.random.default_rng(9).integers(33, 74, size=len(bases)).astype(np.uint8)
        q[np.random.default_rng(10).random(len(bases)) < 0.9] = ord("I")
        quals = [q[offs[i]:offs[i + 1]].tobytes() if i % 50 else None for i in range(len(offs) - 1)]     # (every 50th: QUAL "*")
        low = q < 33 + min_q
        for i in range(0, len(offs) - 1, 50):
            low[offs[i]:offs[i + 1]] = False
        bases, offs = split_at_low(bases, offs, low)
    reads_io.write_sam(os.path.join(d, FILES[0]), batch, header=header, quals=quals)
    reads_io.write_sam(os.path.join(d, FILES[1]), batch, header=header, bgzf=True, block=23456, quals=quals)
    reads_io.write_sam(os.path.join(d, FILES[2]), batch, header=header, gz=True, quals=quals)
    from oracle import oracle
    expect, _ = oracle.map_reads(index, index.max_node_id(), bases, offs, 31, n_threads=4)
    np.save(os.path.join(d, "expect.npy"), expect)
    with open(os.path.join(d, "min_q.txt"), "w") as f:
        f.write("%d\n" % min_q)


def rank_run(d):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    expect = np.load(os.path.join(d, "expect.npy"))
    min_q = int(open(os.path.join(d, "min_q.txt")).read())
    floor = ["--min-base-quality", str(min_q), "--use-record-qual"] if min_q else []
    ok = True
    for name in FILES:
        out = os.path.join(d, "out_" + name.replace(".", "_"))
        run_argument_parser(["map", "-i", os.path.join(d, "index.npz"), "-f", os.path.join(d, name), "-o", out, "-c", "300000"] + floor)
        dist.barrier()
        if rank == 0:
            got = np.load(out + ".npy")
            same = bool(np.array_equal(got[:len(expect)], expect) and not got[len(expect):].any())
            ok = ok and same
            print("%d-rank CLI rehearsal on %s: %s" % (world, name, "SAME AS ONE RANK" if same else "DIFFERS"), flush=True)
    dist.destroy_process_group()
    return ok


if __name__ == "__main__":
    if sys.argv[1] == "--prepare":
        prepare(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 0)
    elif not rank_run(sys.argv[1]):
        sys.exit(1)
