#!/usr/bin/env python3
"""What the BGZF writer costs and gives (profiles/bgzf_out/README.md).

  ratio   (no GPU) the g++ build of csrc/kmm_bgzf_out.hpp against per-block zlib at levels 1 and 6 (what gz_io.write_bgzf
          does) on FASTQ-like text: 150-base reads, Illumina-style names, a skewed or a uniform quality alphabet
              python tools/bgzf_out_bench.py ratio [megabytes=30]
  take    the case of profiles/record_keep: the 10 M-k-mer index, 1 M reads of 150 bases as one FASTQ chunk in HBM, every second
          read random.  kmm_map_records + kmm_take_record_hits, then the kept text taken (p) plain into host memory, (z) as BGZF
          into host memory, (pd) / (zd) the same into device memory; the new kernels' kmm_get_timing; the host pass the feature
          replaces — per-block zlib level 1 on 16 threads over the plain text
              python tools/bgzf_out_bench.py take [n_reads=1000000] [n_index=10000000] [reps=7]
  text    kmm_bgzf_compress, device to device, on `megabytes` of the FASTQ-like text of `ratio` (names and qualities that do not
          compress to nothing): GB/s of text by device events around the call
              python tools/bgzf_out_bench.py text [megabytes=30] [reps=7]
"""
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BLOCK = 0xFF00


def fastq_like(n_records, seed, uniform_quals=False):
    """Vectorised: '@A00123:45:HXXXXXXXX:1:TTTT:XXXXX:YYYYY 1:N:0:ACGTACGT', 150 bases, '+', 150 qualities."""
    rs = np.random.RandomState(seed)
    tile = 1101 + np.arange(n_records) // 2000
    x, y = rs.randint(1000, 32000, n_records), 1000 + (np.arange(n_records) * 7) % 30000
    names = np.array(["@A00123:45:HXXXXXXXX:1:%04d:%05d:%05d 1:N:0:ACGTACGT\n" % t for t in zip(tile, x, y)], dtype="S55")
    row = np.empty((n_records, 55 + 151 + 2 + 151), dtype=np.uint8)
    row[:, :55] = names.view(np.uint8).reshape(n_records, 55)
    row[:, 55:205] = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, (n_records, 150))]
    row[:, 205:208] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    if uniform_quals:
        row[:, 208:358] = 33 + rs.randint(0, 41, (n_records, 150))
    else:
        row[:, 208:358] = 33 + np.array([2, 11, 25, 37], dtype=np.uint8)[rs.choice(4, (n_records, 150), p=(0.02, 0.08, 0.2, 0.7))]
    row[:, 358] = 10
    return row.reshape(-1)


def zlib_member(piece, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return 26 + len(c.compress(piece) + c.flush())


def zlib_bgzf_size(data, level, threads=16):
    """(bytes, seconds) of per-block zlib on `threads` threads (zlib releases the interpreter lock)."""
    view = memoryview(data)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as pool:
        total = sum(pool.map(lambda p: zlib_member(view[p:p + BLOCK], level), range(0, len(view), BLOCK)))
    return total, time.perf_counter() - t0


def ratio(megabytes):
    import tempfile
    from tests import bgzf_out_cases as bc
    with tempfile.TemporaryDirectory() as tmp:
        lib = bc.build_cpu_lib(tmp)
        for name, uniform in (("skewed qualities (4 values)", False), ("uniform qualities (41 values)", True)):
            text = fastq_like(int(megabytes * 1e6) // 359, 21, uniform).tobytes()
            t0 = time.perf_counter()
            data, sizes, stats = bc.cpu_compress(lib, text)
            t_cpu = time.perf_counter() - t0
            z1, _ = zlib_bgzf_size(text, 1)
            z6, _ = zlib_bgzf_size(text, 6)
            print("%-30s %10d bytes: this %10d (%.4f)   zlib -1 %10d (%.4f)   zlib -6 %10d (%.4f)   this / zlib -1 %.3f, / zlib -6 %.3f"
                  "   [%d members, %d stored, %d limited; CPU model %.1f s]"
                  % (name, len(text), len(data), len(data) / len(text), z1, z1 / len(text), z6, z6 / len(text), len(data) / z1,
                     len(data) / z6, len(sizes), stats[2], stats[1], t_cpu))


def take(n_reads, n_index, reps):
    import torch
    from kmer_mapper_amd import _lib, synthetic as syn
    from kmer_mapper_amd.engine import DeviceIndex
    from tools.record_hits_bench import K, L, fastq_chunk, run_rounds
    index, genome = syn.make_index_torch(n_index, k=K, seed=1)
    bases = syn.make_reads_torch(genome, n_reads, L, seed=2).cpu().numpy().reshape(n_reads, L).copy()
    rng = np.random.default_rng(3)
    bases[1::2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=bases[1::2].shape)]
    chunk = fastq_chunk(bases.reshape(-1), n_reads)
    d_chunk = torch.from_numpy(chunk).cuda()
    dev = DeviceIndex.from_index(index, index.max_node_id())
    dt = getattr(torch, "uint32", torch.int32)
    d_hits, d_windows = (torch.zeros(n_reads, dtype=dt, device="cuda") for _ in range(2))
    cap = int(_lib.lib().kmm_bgzf_bound(chunk.shape[0]))
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    h_out = np.zeros(cap, dtype=np.uint8)
    h_pin = _lib.pinned_array(cap, np.uint8)
    got = {}

    def leg(kind, out):
        dev.record_hits(True, windows=True)
        dev.record_keep(True, min_hits=1)
        assert dev.map_records(d_chunk, fmt=_lib.FORMAT_FASTQ, k=K) == (chunk.shape[0], n_reads)
        assert dev.take_record_hits(out=(d_hits, d_windows)) == n_reads
        got[kind] = dev.take_kept_bgzf(out=out) if kind.startswith("z") else dev.take_kept_records(out=out)
        dev.record_keep(False)
        dev.record_hits(False)

    named = [("p   take_kept_records -> host (pageable)", lambda: leg("p", h_out)),
             ("pp  take_kept_records -> host (page-locked)", lambda: leg("pp", h_pin)),
             ("z   take_kept_bgzf    -> host (pageable)", lambda: leg("z", h_out)),
             ("zp  take_kept_bgzf    -> host (page-locked)", lambda: leg("zp", h_pin)),
             ("pd  take_kept_records -> device", lambda: leg("pd", d_out)),
             ("zd  take_kept_bgzf    -> device", lambda: leg("zd", d_out))]
    print("library: %s" % _lib.SO_PATH)
    print("%d reads of %d bases as FASTQ (%d bytes), index of %d k-mers, k = %d, %d rounds after one warm-up"
          % (n_reads, L, chunk.shape[0], n_index, K, reps))
    times = run_rounds(named, reps, torch.cuda.synchronize)
    for name, _ in named:
        t = np.array(times[name])
        print("  %-46s median %9.3f ms   min %9.3f   max %9.3f" % (name, np.median(t), t.min(), t.max()))
    n_comp, n_text, n_records = got["z"]
    print("  kept %d bytes of %d records -> %d bytes of members (%.4f)" % (n_text, n_records, n_comp, n_comp / n_text))
    dev.set_timing(True)
    for _ in range(3):
        leg("zd", d_out)
        a, b = dev.get_timing(_lib.KERNEL_BGZF_DEFLATE), dev.get_timing(_lib.KERNEL_BGZF_GATHER)
        print("  kmm_get_timing: k_bz_deflate %.3f ms in %d launches (%.1f GB/s of text), k_bz_offsets + k_bz_gather %.3f ms in %d"
              % (a[0], a[1], n_text / a[0] / 1e6, b[0], b[1]))
    dev.set_timing(False)
    leg("p", h_out)
    plain = h_out[:got["p"][0]].copy()
    leg("z", h_out)
    import gzip
    from kmer_mapper_amd.gz_io import BGZF_EOF
    assert gzip.decompress(h_out[:got["z"][0]].tobytes() + BGZF_EOF) == plain.tobytes()
    print("  checked: the members inflate (gzip) to the plain take's bytes")
    for level in (1, 6):
        size, sec = min(zlib_bgzf_size(plain, level) for _ in range(3))
        print("  host pass: per-block zlib -%d on 16 threads over the plain text: %d bytes (%.4f), best of 3 %.1f ms"
              % (level, size, size / len(plain), sec * 1e3))
    dev.close()


def text(megabytes, reps):
    import torch
    from kmer_mapper_amd import _lib
    import ctypes
    for name, uniform in (("skewed qualities", False), ("uniform qualities", True)):
        data = fastq_like(int(megabytes * 1e6) // 359, 21, uniform)
        d_in = torch.from_numpy(data).cuda()
        cap = int(_lib.lib().kmm_bgzf_bound(data.shape[0]))
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        n_out = ctypes.c_int64(0)
        ms = []
        for rnd in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _lib.check(_lib.lib().kmm_bgzf_compress(0, ctypes.c_void_p(d_in.data_ptr()), data.shape[0], ctypes.c_void_p(d_out.data_ptr()),
                                                    cap, ctypes.byref(n_out)))
            if rnd:
                ms.append((time.perf_counter() - t0) * 1e3)
        z1, s1 = zlib_bgzf_size(data, 1)
        print("%-18s %10d bytes -> %10d (%.4f); kmm_bgzf_compress device to device (scratch allocated inside the call): median %.2f ms, "
              "min %.2f (%.1f GB/s of text); zlib -1 on 16 threads: %d bytes, %.1f ms"
              % (name, data.shape[0], n_out.value, n_out.value / data.shape[0], np.median(ms), min(ms), data.shape[0] / min(ms) / 1e6,
                 z1, s1 * 1e3))


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "ratio"
    args = [float(a) for a in sys.argv[2:]]
    if what == "ratio":
        ratio(*(args or [30]))
    elif what == "take":
        take(*[int(a) for a in (args + [1_000_000, 10_000_000, 7][len(args):])])
    else:
        text(*((args + [30, 7][len(args):])[:1]), int((args + [30, 7][len(args):])[1]))
