#!/usr/bin/env python3
"""Rehearsal of `kmer_mapper map --shard-bam` with several ranks on a 1-GPU box (tests/test_gpu_bam_shard.py runs it):
   python tools/bam_shard_rehearsal.py --prepare DIR      writes the index, the reads as one BAM file (members of 0x1F00 bytes,
                                                          records that span them, flags of both strands, secondary and
                                                          supplementary ones) and the one-rank counts (the oracle's), plain and
                                                          with --exclude-flags 0x900 --original-strand, into DIR
   RANK=r WORLD_SIZE=N MASTER_ADDR=127.0.0.1 MASTER_PORT=p KMM_DIST_BACKEND=gloo python tools/bam_shard_rehearsal.py DIR
                                                          one rank: the CLI on the file, rank 0 compares
Every rank finds its member range on the GPU (bgzf_ranges.rank_member_range_bam); the counts are summed over gloo."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import reads_io, synthetic as syn                      # noqa: E402
from kmer_mapper_amd.util import ReadBatch                                  # noqa: E402

RUNS = (("plain", []), ("filtered", ["--exclude-flags", "0x900", "--original-strand"]))
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def prepare(d):
    index, genome = syn.make_index(20000, seed=17)
    bases, offs = syn.make_ragged_reads(genome, 20000, 0, 300, seed=18)
    flags = np.random.default_rng(19).choice([0, 16, 99, 147, 256, 272, 2048, 4], size=len(offs) - 1)
    index.to_file(os.path.join(d, "index.npz"))
    reads_io.write_bam(os.path.join(d, "reads.bam"), ReadBatch(bases, offs), flags=flags, block=0x1F00)
    from oracle import oracle
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    for name, _ in RUNS:
        if name == "filtered":      # primary records, the reverse-strand ones flipped back
            reads = [(r.translate(_COMP)[::-1] if f & 16 else r) for r, f in zip(reads, flags) if not f & 0x900]
        b = np.frombuffer(b"".join(reads), np.uint8)
        o = np.zeros(len(reads) + 1, np.int64)
        np.cumsum([len(r) for r in reads], out=o[1:])
        np.save(os.path.join(d, "expect_%s.npy" % name), oracle.map_reads(index, index.max_node_id(), b, o, 31, n_threads=4)[0])


def rank_run(d):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    import torch.distributed as dist
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    ok = True
    for name, switches in RUNS:
        expect = np.load(os.path.join(d, "expect_%s.npy" % name))
        out = os.path.join(d, "out_" + name)
        run_argument_parser(["map", "-i", os.path.join(d, "index.npz"), "-f", os.path.join(d, "reads.bam"), "-o", out, "--shard-bam"]
                            + switches)
        dist.barrier()
        if rank == 0:
            got = np.load(out + ".npy")
            same = bool(np.array_equal(got[:len(expect)], expect) and not got[len(expect):].any())
            ok = ok and same
            print("%d-rank --shard-bam rehearsal, %s: %s" % (world, name, "SAME AS ONE RANK" if same else "DIFFERS"), flush=True)
    dist.destroy_process_group()
    return ok


if __name__ == "__main__":
    if sys.argv[1] == "--prepare":
        prepare(sys.argv[2])
    elif not rank_run(sys.argv[1]):
        sys.exit(1)
