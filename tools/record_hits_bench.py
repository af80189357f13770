#!/usr/bin/env python3
"""What the record-hits mode costs: the 10 M-k-mer index of BASELINE configs[1] and 1 M reads of 150 bases as one
raw FASTQ chunk, legs on the same chunk:
  (a)  the chunk in HBM through the mode: kmm_map_records with "record_hits" 2, then kmm_take_record_hits into device arrays
       (and with "record_hits" 1: hits alone);
  (b)  kmm_map_records on the same chunk in HBM with the mode off and "path" 1, up to kmm_synchronize: the same front end and
       the same gathers, node counts instead of per-record sums — run it at the parent commit too (KMM_LIB_PATH=<its build>,
       legs=b): the out-parameter of tile_kmers must cost this leg nothing;
  (c)  the route there was before: the chunk in host memory parsed by the host (reads_io.parse_fastq_block), then kmm_read_hits
       on the flat reads.
  (d)  with legs containing "d": the command line — `read-hits --device-parser` on the reads as BGZF FASTQ and as BAM against
       `read-hits` (host-parsed) on the same reads as .fq.gz, each a run of run_argument_parser in this process with its own
       index load and upload (the files and the index are written to a temporary directory first; level-1 deflate).
    python tools/record_hits_bench.py [n_reads=1000000] [n_index=10000000] [reps=9] [legs=abc]
One warm-up round, then `reps` rounds with the legs alternated inside every round; prints median / min / max wall time per leg."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import _lib, reads_io, synthetic as syn        # noqa: E402
from kmer_mapper_amd.engine import DeviceIndex                      # noqa: E402

L, K = 150, 31


def fastq_chunk(bases, n_reads):
    """The reads as FASTQ text, one row of 307 bytes per record: '@r', the bases, '+', 150 quality bytes."""
    row = np.empty((n_reads, 3 + L + 3 + L + 1), dtype=np.uint8)
    row[:, :3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    row[:, 3:3 + L] = bases.reshape(n_reads, L)
    row[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    row[:, 6 + L:6 + 2 * L] = ord("I")
    row[:, -1] = 10
    return row.reshape(-1)


def report(named, times, n_kmers):
    med = {}
    for name, _ in named:
        t = np.array(times[name])
        med[name] = float(np.median(t))
        print("  %-58s median %9.3f ms   min %9.3f   max %9.3f   (%.2f G k-mers/s)" % (name, med[name], t.min(), t.max(),
                                                                                       n_kmers / med[name] / 1e6))
    return med


def run_rounds(named, reps, sync):
    times = {name: [] for name, _ in named}
    for rnd in range(reps + 1):
        for name, fn in (named if rnd % 2 == 0 else named[::-1]):    # alternated: no leg always runs behind the same one
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    import torch
    n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    n_index = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 9
    legs = sys.argv[4] if len(sys.argv) > 4 else "abc"
    has_mode = hasattr(_lib.lib(), "kmm_take_record_hits")
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2).cpu().numpy()
    chunk = fastq_chunk(bases, n_reads)
    d_chunk = torch.from_numpy(chunk).cuda()
    n_kmers = n_reads * (L - K + 1)
    dev = DeviceIndex.from_index(index, index.max_node_id())
    dt = getattr(torch, "uint32", torch.int32)
    d_hits = torch.zeros(n_reads, dtype=dt, device="cuda")
    d_windows = torch.zeros(n_reads, dtype=dt, device="cuda")
    kept = {}

    def mode(windows):
        dev.record_hits(True, windows=windows)
        used, n = dev.map_records(d_chunk, fmt=_lib.FORMAT_FASTQ, k=K)
        assert (used, n) == (chunk.shape[0], n_reads)
        assert dev.take_record_hits(out=(d_hits, d_windows if windows else None)) == n_reads
        dev.record_hits(False)

    def map_direct():
        dev.set_param("path", 1)
        dev.map_records(d_chunk, fmt=_lib.FORMAT_FASTQ, k=K)
        dev.synchronize()
        dev.set_param("path", 0)

    def host_route():
        batch = reads_io.parse_fastq_block(chunk)
        kept["hits"] = dev.read_hits(batch.bases, n_reads=len(batch), read_len=L, k=K)

    named = []
    if "a" in legs and has_mode:
        named += [("a  map_records in HBM, record_hits 2, take to device", lambda: mode(True)),
                  ("a  map_records in HBM, record_hits 1, take to device", lambda: mode(False))]
    if "b" in legs:
        named.append(("b  map_records in HBM, mode off, path 1, synchronize", map_direct))
    if "c" in legs:
        named.append(("c  host parse + kmm_read_hits (host arrays)", host_route))
    print("library: %s" % _lib.SO_PATH)
    print("%d reads of %d bases as FASTQ (%d bytes, %d k-mers), index of %d k-mers, k = %d, %d rounds after one warm-up"
          % (n_reads, L, chunk.shape[0], n_kmers, n_index, K, reps))
    if named:
        report(named, run_rounds(named, reps, torch.cuda.synchronize), n_kmers)
    if "a" in legs and "c" in legs and has_mode:
        mode(True)
        h, w = d_hits.cpu().numpy().view(np.uint32), d_windows.cpu().numpy().view(np.uint32)
        assert (w == L - K + 1).all() and np.array_equal(h, kept["hits"])
        print("  checked: the mode's hits equal kmm_read_hits' on the host-parsed reads; reads with a hit: %.1f %%" % (100.0 * (h > 0).mean()))
    dev.close()
    if "d" in legs:
        command_line(index, bases, chunk, n_reads, n_kmers, max(3, reps // 3), has_mode)


def command_line(index, bases, chunk, n_reads, n_kmers, reps, has_mode):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.util import ReadBatch
    import logging
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        npz, fqgz, bam, out = (os.path.join(tmp, n) for n in ("index.npz", "reads.fq.gz", "reads.bam", "out"))
        (index.to_host() if hasattr(index, "to_host") else index).to_file(npz)
        print("index written; writing the read files ...", flush=True)
        with open(fqgz, "wb") as f:
            f.write(reads_io.bgzf_members(chunk.tobytes(), level=1) + reads_io.BGZF_EOF)
        reads_io.write_bam(bam, ReadBatch(bases, np.arange(n_reads + 1, dtype=np.int64) * L), level=1)
        print("files: %s %d bytes, %s %d bytes" % (os.path.basename(fqgz), os.path.getsize(fqgz), os.path.basename(bam), os.path.getsize(bam)))
        common = ["read-hits", "-i", npz, "-k", str(K), "-o", out]
        run = lambda extra: (lambda: run_argument_parser(common + extra))
        named = [("d  read-hits on .fq.gz (host-parsed)", run(["-f", fqgz]))]
        if has_mode:
            named += [("d  read-hits --device-parser on .fq.gz (BGZF)", run(["-f", fqgz, "--device-parser"])),
                      ("d  read-hits --device-parser on .bam", run(["-f", bam, "--device-parser"]))]
        logging.disable(logging.INFO)
        times = run_rounds(named, reps, torch.cuda.synchronize)
        logging.disable(logging.NOTSET)
        print("command line, index load and upload included, %d rounds after one warm-up" % reps)
        report(named, times, n_kmers)
        if has_mode:
            ref = np.load(out + ".npy")
            for _, fn in named:
                fn()
                assert np.array_equal(np.load(out + ".npy"), ref)
            print("  checked: the three routes write the same hits")


if __name__ == "__main__":
    main()
