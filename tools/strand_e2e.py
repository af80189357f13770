#!/usr/bin/env python3
"""`kmer_mapper map` with and without --original-strand on synthetic reads written as an aligned-style BAM and as
plain SAM text: a fraction of the records stored reverse-complemented, qualities reversed, FLAG 16; the two settings alternated
in one job.
    python tools/strand_e2e.py [n_reads=4000000] [n_index=10000000] [out_dir=/tmp/kmm_strand] [reps=3] [fraction=0.5] [routes=bam,sam]
The reads are tools/bam_e2e.py's (names SRR0000001.<i>, binned qualities).  Prints per repetition the end-to-end time of the CLI
(its own log has the map phase: "hashing and counting"), then the medians.  Checked: with the switch on, the count vector of
either file equals the one of the FASTQ the reads came from; with it off it does not.  KMM_STRAND_ONLY=on|off runs one setting
alone (a profiler run of its own)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from kmer_mapper_amd import reads_io, synthetic as syn          # noqa: E402
from tools.bgzf_e2e import make_fastq                            # noqa: E402
from tools.bam_e2e import bam_payload, bgzf_file                 # noqa: E402

_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    _COMP[_a] = _b


def stored_fastq(raw, n_reads, L, reverse):
    """The FASTQ of make_fastq (fixed-size records) with the sequence lines of the reads in `reverse` reverse-complemented and
    their quality lines reversed: the text whose records are what an aligner stores."""
    rec = np.frombuffer(raw, np.uint8).reshape(n_reads, -1).copy()
    W = rec.shape[1] - (2 * L + 4)
    rec[reverse, W:W + L] = _COMP[rec[reverse, W:W + L]][:, ::-1]
    rec[reverse, W + L + 3:W + 2 * L + 3] = rec[reverse, W + L + 3:W + 2 * L + 3][:, ::-1]
    return rec


def sam_text(rec, L, flags):
    """The fixed-size FASTQ records as SAM lines (FLAG 16 / 0 are two digits / one: two shapes of line)."""
    n = rec.shape[0]
    W = rec.shape[1] - (2 * L + 4)
    out = []
    for flag in (0, 16):
        sel = np.flatnonzero(flags == flag)
        mid = np.frombuffer(b"\t%d\tchr1\t1\t60\t%dM\t*\t0\t0\t" % (flag, L), np.uint8)
        line = np.empty((len(sel), (W - 2) + len(mid) + L + 1 + L + 1), np.uint8)
        line[:, :W - 2] = rec[sel, 1:W - 1]
        p = W - 2
        line[:, p:p + len(mid)] = mid
        p += len(mid)
        line[:, p:p + L] = rec[sel, W:W + L]
        line[:, p + L] = 9
        line[:, p + L + 1:p + 2 * L + 1] = rec[sel, W + L + 3:W + 2 * L + 3]
        line[:, -1] = 10
        out.append((sel, line))
    # (the order of the records does not matter to the counts: forward records first, reversed behind them)
    return b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr1\tLN:1000000\n" + out[0][1].tobytes() + out[1][1].tobytes(), n


def main():
    import logging
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    a = sys.argv
    n_reads = int(a[1]) if len(a) > 1 else 4_000_000
    n_index = int(a[2]) if len(a) > 2 else 10_000_000
    out_dir = a[3] if len(a) > 3 else "/tmp/kmm_strand"
    reps = int(a[4]) if len(a) > 4 else 3
    fraction = float(a[5]) if len(a) > 5 else 0.5
    routes = (a[6] if len(a) > 6 else "bam,sam").split(",")
    only = os.environ.get("KMM_STRAND_ONLY")
    L = 150
    os.makedirs(out_dir, exist_ok=True)
    t0 = time.time()
    index, genome = syn.make_index(n_index, seed=1, gpu_builder=True)
    bases, _ = syn.make_reads(genome, n_reads, L, seed=2)
    paths = {"fastq": os.path.join(out_dir, "reads.fq"), "bam": os.path.join(out_dir, "reads.bam"), "sam": os.path.join(out_dir, "reads.sam")}
    make_fastq(paths["fastq"], bases, n_reads, L)
    raw = open(paths["fastq"], "rb").read()
    reverse = np.random.Generator(np.random.PCG64(3)).random(n_reads) < fraction
    flags = np.where(reverse, 16, 0)
    rec = stored_fastq(raw, n_reads, L, reverse)
    if "bam" in routes:
        payload = bytearray(bam_payload(rec.tobytes(), n_reads, L))
        hdr = len(reads_io.bam_header(text=b"@HD\tVN:1.6\tSO:unsorted\n"))
        body = np.frombuffer(payload, np.uint8)[hdr:].reshape(n_reads, -1)
        body[:, 18:20] = np.frombuffer(flags.astype("<u2").tobytes(), np.uint8).reshape(n_reads, 2)      # FLAG: bytes 18, 19 of a record
        bgzf_file(paths["bam"], bytes(payload))
        del payload, body
    if "sam" in routes:
        text, _ = sam_text(rec, L, flags)
        with open(paths["sam"], "wb") as f:
            f.write(text)
        del text
    print("setup %.1f s: %d reads of %d bases, %d stored reversed (fraction %.2f); %d-entry index"
          % (time.time() - t0, n_reads, L, int(reverse.sum()), fraction, len(index._kmers)), flush=True)
    del raw, rec
    from kmer_mapper_amd.command_line_interface import map_bnp

    def cli(route, on):
        ns = argparse.Namespace(kmer_index=index, index_bundle=None, reads=paths[route], kmer_size=31, n_threads=16, chunk_size=2_500_000,
                                output_file=None, debug=None, max_hits_per_kmer=1000, gpu=True, gpu_hash_map_size=0,
                                map_reverse_complements=False, apply_max_hits_per_kmer=False, host_parser=False, device=0,
                                exclude_flags=0x900 if route != "fastq" else 0, min_base_quality=0, use_record_qual=False,
                                original_strand=on)
        time.sleep(4)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        c = map_bnp(ns)
        return c, time.perf_counter() - t

    want, _ = cli("fastq", False)
    kinds = [(r, on) for r in routes for on in (False, True) if only is None or on == (only == "on")]
    outs, times = {}, {k: [] for k in kinds}
    for rep in range(reps):
        for kind in kinds:
            outs[kind], dt = cli(*kind)
            times[kind].append(dt)
            print("CLI rep %d, %s, original_strand %s: %.3f s end to end" % (rep, kind[0], "on" if kind[1] else "off", dt), flush=True)
    ok = True
    for kind, t in times.items():
        t = np.array(t)
        same = np.array_equal(outs[kind], want)
        ok = ok and same == kind[1]
        print("CLI %s, original_strand %s: median %.3f s end to end, min %.3f, max %.3f over %d runs; counts == the FASTQ's: %s"
              % (kind[0], "on" if kind[1] else "off", np.median(t), t.min(), t.max(), len(t), same), flush=True)
    for p in paths.values():
        if os.path.exists(p):
            os.remove(p)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
