#!/usr/bin/env python3
"""`select-reads --sam-out` next to the routes it is priced against, on the reads of tools/sam_e2e.py — 4 M reads of
150 bases, names SRR0000001.<i>, FLAG 4 — with every second read replaced by random bases, so that half of them are kept; written
as plain SAM, as BGZF SAM (zlib level 6, members of 0xFF00 inflated bytes) and, for context, as unaligned BAM.
    python tools/sam_out_e2e.py setup DIR [n_reads=4000000] [n_index=10000000]   writes DIR/index.npz, reads.sam, reads.sam.gz, reads.bam
    python tools/sam_out_e2e.py run WHAT DIR [reps=3]
WHAT: read-hits-sam | read-hits-samgz (`read-hits --device-parser`: the hits alone, what the keep is priced against), sam-out |
sam-out-gz (`select-reads --sam-out` on the plain / the BGZF file, plain text out), sam-out-gz-bgzf (BGZF in and out), bam-out
(`select-reads --bam-out` on the BAM).  Prints per repetition the CLI's map phase (its "hashing and counting" line) and the
end-to-end time.  One process per library under comparison (KMM_LIB_PATH names another build's libkmm.so, which serves the
read-hits and bam-out routes); a profiler goes around `run`.
    python tools/sam_out_e2e.py timing DIR [mb=1024]    the first mb MiB of reads.sam through DeviceIndex.map_records with timing on:
                                                        the KMM_KERNEL_SAM_RAW slot, the kept bytes, and the output checked
                                                        against a host filter of the same lines"""
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(out_dir, n_reads, n_index):
    from kmer_mapper_amd import synthetic as syn
    from tools.bam_e2e import bam_payload, bgzf_file
    from tools.bgzf_e2e import make_fastq
    from tools.sam_e2e import sam_payload
    L = 150
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    reads = np.asarray(bases).reshape(n_reads, L)
    rng = np.random.Generator(np.random.PCG64(3))
    reads[1::2] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n_reads // 2, L), dtype=np.uint8)]   # no hit
    fq = os.path.join(out_dir, "reads.fq")
    make_fastq(fq, reads.reshape(-1), n_reads, L)
    raw = open(fq, "rb").read()
    os.remove(fq)
    sam = sam_payload(raw, n_reads, L)
    with open(os.path.join(out_dir, "reads.sam"), "wb") as f:
        f.write(sam)
    bgzf_file(os.path.join(out_dir, "reads.sam.gz"), sam)
    bgzf_file(os.path.join(out_dir, "reads.bam"), bam_payload(raw, n_reads, L))
    index.to_file(os.path.join(out_dir, "index.npz"))
    print("setup %.1f s: %d reads; SAM %.2f GB -> %.2f GB BGZF; BAM %.2f GB; %d-entry index"
          % (time.time() - t0, n_reads, len(sam) / 1e9, os.path.getsize(os.path.join(out_dir, "reads.sam.gz")) / 1e9,
             os.path.getsize(os.path.join(out_dir, "reads.bam")) / 1e9, len(index._kmers)), flush=True)


def run(what, out_dir, reps):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from tools.bam_fastq_e2e import _MapPhase
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    npz, sam, samgz, bam = (os.path.join(out_dir, n) for n in ("index.npz", "reads.sam", "reads.sam.gz", "reads.bam"))
    out = os.path.join(out_dir, "out_" + what)
    common = ["-i", npz, "-k", "31", "-o", out]
    args = {"read-hits-sam": ["read-hits", "-f", sam, "--device-parser", "--windows", "--original-strand"] + common,
            "read-hits-samgz": ["read-hits", "-f", samgz, "--device-parser", "--windows", "--original-strand"] + common,
            "sam-out": ["select-reads", "-f", sam, "--sam-out"] + common,
            "sam-out-gz": ["select-reads", "-f", samgz, "--sam-out"] + common,
            "sam-out-gz-bgzf": ["select-reads", "-f", samgz, "--sam-out", "--bgzf"] + common,
            "bam-out": ["select-reads", "-f", bam, "--bam-out"] + common}[what]
    lib = os.environ.get("KMM_LIB_PATH", "this build")
    times = []
    for rep in range(reps):
        watch = _MapPhase()
        logging.getLogger().addHandler(watch)
        time.sleep(2)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        run_argument_parser(args)
        dt = time.perf_counter() - t
        logging.getLogger().removeHandler(watch)
        times.append(watch.seconds)
        size = os.path.getsize(out) if os.path.exists(out) else 0
        print("%s [%s] rep %d: map phase %.4f s, %.3f s end to end, %d bytes written; %s"
              % (what, lib, rep, watch.seconds, dt, size, " | ".join(watch.lines)), flush=True)
    t = np.array(times)
    print("%s [%s]: map phase median %.4f s, min %.4f, max %.4f over %d runs" % (what, lib, np.median(t), t.min(), t.max(), len(t)),
          flush=True)
    for name in (out, out + ".npy", out + ".windows.npy"):
        if os.path.exists(name):
            os.remove(name)


def timing(out_dir, mb):
    """One piece of the plain SAM file through the library with timing on: what the KMM_KERNEL_SAM_RAW slot holds."""
    from kmer_mapper_amd import _lib
    from kmer_mapper_amd.engine import DeviceIndex
    from kmer_mapper_amd.kmer_index import KmerIndex
    index = KmerIndex.from_file(os.path.join(out_dir, "index.npz"))
    data = np.fromfile(os.path.join(out_dir, "reads.sam"), dtype=np.uint8, count=mb << 20)
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        dev.set_param("original_strand", 1)
        for rep in range(4):
            for mode in ("hits", "sam-out"):
                dev.record_hits(True, windows=True)
                dev.record_keep(mode == "sam-out")
                dev.record_sam(mode == "sam-out")
                dev.set_timing(True)
                dev.get_timing()
                t = time.perf_counter()
                used, n = dev.map_records(data, fmt=_lib.FORMAT_SAM, k=31)
                t_call = time.perf_counter() - t
                dev.synchronize()
                dt = time.perf_counter() - t
                ms, launches = dev.get_timing(_lib.KERNEL_SAM_RAW)
                hits, _ = dev.take_record_hits()
                kept = dev.get_param("record_keep_pending_bytes")
                text = dev.take_kept_records()[0] if mode == "sam-out" else None
                print("timing rep %d %s: %d bytes, %d records, call %.2f ms, with the sync %.2f ms; KMM_KERNEL_SAM_RAW %.3f ms in %d "
                      "intervals; %d bytes kept" % (rep, mode, used, n, t_call * 1e3, dt * 1e3, ms, launches, kept), flush=True)
                if text is not None and rep == 0:
                    lines = data[:used].tobytes().split(b"\n")[:-1]
                    n_head = sum(1 for ln in lines if ln.startswith(b"@"))
                    want = b"".join(ln + b"\n" for i, ln in enumerate(lines) if i < n_head or hits[i - n_head] >= 1)
                    print("timing: output equals the host filter of the same lines: %s" % (text.tobytes() == want), flush=True)


def main():
    if len(sys.argv) >= 3 and sys.argv[1] == "setup":
        setup(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 4_000_000, int(sys.argv[4]) if len(sys.argv) > 4 else 10_000_000)
    elif len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    elif len(sys.argv) >= 3 and sys.argv[1] == "timing":
        timing(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1024)
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
