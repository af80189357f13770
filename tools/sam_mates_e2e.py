#!/usr/bin/env python3
"""`select-reads --sam-out --sam-mates` next to `--sam-out` alone, on the reads of tools/sam_e2e.py — 4 M reads of 150
bases, FLAG 4 — built as 2 M pairs: read 2p + 1 carries the name of read 2p, and both reads of every second pair are replaced by
random bases, so that half of the pairs are kept; written as plain SAM and as BGZF SAM (zlib level 6, members of 0xFF00 bytes).
    python tools/sam_mates_e2e.py setup DIR [n_reads=4000000] [n_index=10000000]   writes DIR/index.npz, reads.sam, reads.sam.gz
    python tools/sam_mates_e2e.py run WHAT DIR [reps=3]
WHAT: sam-out | sam-mates (`select-reads --sam-out [--sam-mates]` on the plain file), sam-out-gz | sam-mates-gz (on the BGZF file).
Prints per repetition the CLI's map phase (its "hashing and counting" line) and the end-to-end time.  The files carry the names
tools/sam_out_e2e.py reads, so another build's checkout runs its own `sam_out_e2e.py run sam-out DIR` on them: one process per
build and switch under comparison, alternated by the caller.
    python tools/sam_mates_e2e.py timing DIR [mb=1024]   the first mb MiB of reads.sam through DeviceIndex.map_records with timing
                                                         on, the switch off and on: the KMM_KERNEL_SAM_RAW and
                                                         KMM_KERNEL_SAM_RAW_MATES slots, the kept bytes, and the pair form's
                                                         output checked against a host filter of the same lines"""
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def setup(out_dir, n_reads, n_index):
    from kmer_mapper_amd import synthetic as syn
    from tools.bam_e2e import bgzf_file
    from tools.bgzf_e2e import make_fastq
    from tools.sam_e2e import sam_payload
    L = 150
    n_reads -= n_reads % 4
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    reads = np.asarray(bases).reshape(n_reads, L)
    rng = np.random.Generator(np.random.PCG64(3))
    random = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=(n_reads // 2, L), dtype=np.uint8)]         # no hit
    reads[2::4], reads[3::4] = random[0::2], random[1::2]              # both mates of every second pair
    fq = os.path.join(out_dir, "reads.fq")
    make_fastq(fq, reads.reshape(-1), n_reads, L)
    rec = np.fromfile(fq, dtype=np.uint8).reshape(n_reads, -1)
    os.remove(fq)
    W = rec.shape[1] - (2 * L + 4)
    rec[1::2, 1:W - 1] = rec[0::2, 1:W - 1]                            # mate 2 carries mate 1's name
    sam = sam_payload(rec.tobytes(), n_reads, L)
    with open(os.path.join(out_dir, "reads.sam"), "wb") as f:
        f.write(sam)
    bgzf_file(os.path.join(out_dir, "reads.sam.gz"), sam)
    index.to_file(os.path.join(out_dir, "index.npz"))
    print("setup %.1f s: %d reads in %d pairs; SAM %.2f GB -> %.2f GB BGZF; %d-entry index"
          % (time.time() - t0, n_reads, n_reads // 2, len(sam) / 1e9, os.path.getsize(os.path.join(out_dir, "reads.sam.gz")) / 1e9,
             len(index._kmers)), flush=True)


def run(what, out_dir, reps):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from tools.bam_fastq_e2e import _MapPhase
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    npz, sam, samgz = (os.path.join(out_dir, n) for n in ("index.npz", "reads.sam", "reads.sam.gz"))
    out = os.path.join(out_dir, "out_" + what)
    common = ["-i", npz, "-k", "31", "-o", out]
    args = {"sam-out": ["select-reads", "-f", sam, "--sam-out"] + common,
            "sam-mates": ["select-reads", "-f", sam, "--sam-out", "--sam-mates"] + common,
            "sam-out-gz": ["select-reads", "-f", samgz, "--sam-out"] + common,
            "sam-mates-gz": ["select-reads", "-f", samgz, "--sam-out", "--sam-mates"] + common}[what]
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
        print("%s rep %d: map phase %.4f s, %.3f s end to end, %d bytes written; %s"
              % (what, rep, watch.seconds, dt, size, " | ".join(watch.lines)), flush=True)
    t = np.array(times)
    print("%s: map phase median %.4f s, min %.4f, max %.4f over %d runs" % (what, np.median(t), t.min(), t.max(), len(t)), flush=True)
    if os.path.exists(out):
        os.remove(out)


def timing(out_dir, mb):
    """One piece of the plain SAM file through the library with timing on, the switch off and on."""
    from kmer_mapper_amd import _lib
    from kmer_mapper_amd.engine import DeviceIndex
    from kmer_mapper_amd.kmer_index import KmerIndex
    index = KmerIndex.from_file(os.path.join(out_dir, "index.npz"))
    data = np.fromfile(os.path.join(out_dir, "reads.sam"), dtype=np.uint8, count=mb << 20)
    with DeviceIndex.from_index(index, index.max_node_id()) as dev:
        dev.set_param("original_strand", 1)
        dev.record_hits(True, windows=True)
        dev.record_keep(True)
        for rep in range(4):
            for mates in (False, True):
                dev.record_sam(True, mates=mates)
                dev.set_timing(True)
                dev.get_timing()
                t = time.perf_counter()
                used, n = dev.map_records(data, fmt=_lib.FORMAT_SAM, k=31)
                t_call = time.perf_counter() - t
                dev.synchronize()
                dt = time.perf_counter() - t
                ms, launches = dev.get_timing(_lib.KERNEL_SAM_RAW_MATES if mates else _lib.KERNEL_SAM_RAW)
                other = dev.get_timing(_lib.KERNEL_SAM_RAW if mates else _lib.KERNEL_SAM_RAW_MATES)[1]
                hits, _ = dev.take_record_hits()
                kept = dev.get_param("record_keep_pending_bytes")
                text = dev.take_kept_records()[0]
                dev.reset()
                print("timing rep %d %s: %d bytes, %d entries, call %.2f ms, with the sync %.2f ms; %s %.3f ms in %d intervals (the other "
                      "slot: %d); %d bytes kept" % (rep, "sam-mates" if mates else "sam-out", used, n, t_call * 1e3, dt * 1e3,
                                                    "KMM_KERNEL_SAM_RAW_MATES" if mates else "KMM_KERNEL_SAM_RAW", ms, launches, other, kept),
                      flush=True)
                if mates and rep == 0:
                    lines = data[:used].tobytes().split(b"\n")[:-1]
                    n_head = sum(1 for ln in lines if ln.startswith(b"@"))
                    recs = lines[n_head:]
                    want = [ln + b"\n" for ln in lines[:n_head]]
                    for p in range(len(hits) // 2):
                        if hits[2 * p] >= 1 or hits[2 * p + 1] >= 1:
                            want += [recs[2 * p] + b"\n", recs[2 * p + 1] + b"\n"]
                    print("timing: the pair form's output equals the host filter of the same lines: %s" % (text.tobytes() == b"".join(want)),
                          flush=True)


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
