#!/usr/bin/env python3
"""`select-reads --bam-out --keep-mates` next to `select-reads --bam-out`, on the paired files of
tools/bam_pairs_e2e.py (4 M reads of 150 bases as 2 M pairs in an unaligned BAM, both mates of every second pair random bases, a
10 M-k-mer index).
    python tools/bam_pairs_e2e.py setup DIR                       writes DIR/index.npz, reads.bam (and reads.fq.gz)
    python tools/bam_mates_e2e.py run WHAT DIR [reps=3]           WHAT: bam-out | bam-out-mates
bam-out: `select-reads --bam-out` on the BAM (every record by itself); bam-out-mates: the same with --keep-mates.  Prints per
repetition the CLI's map phase (its "hashing and counting" line), the end-to-end time and the output's size.  One process per
build under comparison; an older commit is measured from a check-out of its own with its tools/bam_out_e2e.py (this tree's Python
sets "record_bam_mates", which an older libkmm.so named by KMM_LIB_PATH does not know); a profiler goes around `run`.
    python tools/bam_mates_e2e.py check DIR                       bam-out-mates once; the output read back on the host with zlib:
                                                                  header equal, the kept records a subsequence of the input's,
                                                                  an even number, every two neighbours with one name."""
import logging
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _args(what, out_dir, out):
    npz, bam = os.path.join(out_dir, "index.npz"), os.path.join(out_dir, "reads.bam")
    common = ["select-reads", "-f", bam, "-i", npz, "-k", "31", "-o", out, "--bam-out"]
    return common + {"bam-out": [], "bam-out-mates": ["--keep-mates"]}[what]


def run(what, out_dir, reps):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from tools.bam_fastq_e2e import _MapPhase
    logging.basicConfig(stream=sys.stdout, level=logging.INFO, format='%(asctime)s %(levelname)s: %(message)s')
    out = os.path.join(out_dir, "out_" + what)
    lib = "this build"
    times = []
    for rep in range(reps):
        watch = _MapPhase()
        logging.getLogger().addHandler(watch)
        time.sleep(2)  # (a handle just closed leaves the driver VRAM to wipe: see tools/bgzf_e2e.py)
        t = time.perf_counter()
        run_argument_parser(_args(what, out_dir, out))
        dt = time.perf_counter() - t
        logging.getLogger().removeHandler(watch)
        times.append(watch.seconds)
        print("%s [%s] rep %d: map phase %.4f s, %.3f s end to end, %d bytes written; %s"
              % (what, lib, rep, watch.seconds, dt, os.path.getsize(out), " | ".join(watch.lines)), flush=True)
    t = np.array(times)
    print("%s [%s]: map phase median %.4f s, min %.4f, max %.4f over %d runs" % (what, lib, np.median(t), t.min(), t.max(), len(t)),
          flush=True)
    os.remove(out)


def check(out_dir):
    """The output of one run against the input, both inflated with zlib (host)."""
    import zlib
    from kmer_mapper_amd.command_line_interface import run_argument_parser

    def inflate(path):
        data, out, p = open(path, "rb").read(), [], 0
        while p < len(data):
            size = int.from_bytes(data[p + 16:p + 18], "little") + 1
            out.append(zlib.decompress(data[p + 18:p + size - 8], -15))
            p += size
        return b"".join(out)

    def records(raw):
        p = 8 + int.from_bytes(raw[4:8], "little")
        n_ref = int.from_bytes(raw[p:p + 4], "little")
        p += 4
        for _ in range(n_ref):
            p += 8 + int.from_bytes(raw[p:p + 4], "little")
        hdr, out = p, []
        while p < len(raw):
            size = 4 + int.from_bytes(raw[p:p + 4], "little")
            out.append(raw[p:p + size])
            p += size
        assert p == len(raw)
        return raw[:hdr], out

    def name(rec):
        return rec[36:36 + rec[12]]

    out = os.path.join(out_dir, "out_check.bam")
    seen, kept = run_argument_parser(_args("bam-out-mates", out_dir, out))
    head_in, recs_in = records(inflate(os.path.join(out_dir, "reads.bam")))
    head_out, recs_out = records(inflate(out))
    assert head_in == head_out and len(recs_in) == seen and len(recs_out) == kept and kept % 2 == 0
    it = iter(recs_in)
    assert all(any(r == s for s in it) for r in recs_out), "the kept records are no subsequence of the input's"
    assert all(name(recs_out[i]) == name(recs_out[i + 1]) for i in range(0, kept, 2)), "two neighbours of the output are no mates"
    print("check: %d of %d records kept in %d pairs, header of %d bytes verbatim, every kept record byte-equal and in file order, "
          "every two neighbours with one name" % (kept, seen, kept // 2, len(head_in)), flush=True)
    os.remove(out)


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    elif len(sys.argv) >= 3 and sys.argv[1] == "check":
        check(sys.argv[2])
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
