"""`kmer_mapper map …` — the reference's CLI surface (kmer_mapper/command_line_interface.py:155-192)
on the MI355X engine.  Same flags, defaults and output file; the work runs in libkmm.so.

Differences that follow from replacing the engine (all documented in DESIGN.md):
  * there is one engine, the GPU: `-g/--gpu` is accepted and ignored; `-s/--gpu-hash-map-size` is ignored (the
    index's own modulo is the hash table);
  * `-t/--n-threads` keeps its meaning — how many host cores work on the read bytes (the reference: a pool of `-t`
    processes that encode and hash every chunk, :124-130,168) — but the cores do less: they read / inflate the file
    and pack the sequence lines to 2 bits per base (libkmm's host packer, kmm_set_param "host_pack_threads"), so that
    a quarter of the bases' bytes cross PCIe; everything after that happens on the GPU.  Capped by the CPUs the
    process may actually use (affinity mask, cgroup quota);
  * results follow the reference's CPU path (uint32 node counts with the frequency filter of
    mapper.pyx:64-66).  The reference parses `-I/--max-hits-per-kmer` but never forwards it
    (command_line_interface.py:51 passes 3 arguments), so its effective filter is always 1000; the same
    holds here unless `--apply-max-hits-per-kmer` is given;
  * `-r` works (the reference only supports it in its experimental GPU mode, :107);
  * `-b/--index-bundle`, Minimal/Counter index variants (util.py:52-66) are out of scope -> error.
  * launched under torchrun (WORLD_SIZE > 1) every rank maps its own BYTE RANGE of the read file (both ends
    re-synchronised to record starts, reads_io.rank_byte_range: no rank reads or scans another rank's bytes);
    ranks sharing one .gz stream (not seekable) take chunk i mod WORLD_SIZE and cut the chunks they skip by the
    record parser's own rule (newline count, reads_io.records_cut); the count vectors are summed with one RCCL reduce; rank 0 writes the output.
    A BAM file is shared only with `--shard-bam` (extension): each rank maps a member range whose ends it finds on the GPU
    (bgzf_ranges.rank_member_range_bam).
  * `--ambiguous-bases skip` (extension; default `a` = the reference, N counted as A and every other letter an error): a
    k-mer that contains N or an IUPAC ambiguity letter is not counted, the windows on either side of it are
    (util.ambiguous_skip_lut, KMM_LUT_BREAK).  Such a table takes the device routes: the raw bytes of a plain file cross
    PCIe as they are, the host threads do not pack them.
  * `--min-base-quality Q` (extension; default 0 = off): a FASTQ base whose quality byte is below '!' + Q is treated like such
    a break — no k-mer over it is counted (kmm_set_param "min_base_quality").  The qualities are read on the
    GPU, so the flag takes the device routes as a table does (plain, BGZF, gzip); it combines with `--ambiguous-bases
    skip`.  SAM / BAM input and `--host-parser` hand the library reads without qualities and are refused; FASTA has none:
    one warning, mapped as before.
  * `--include-flags`, `--min-mapq`, `--regions`, `--regions-file` (extensions, SAM and BAM input only, beside `--exclude-flags`):
    which records are mapped — `samtools view -f / -q / regions / -L` without the pipe: the rule is applied on the GPU inside
    the record the decode kernels hold (kmm_set_param "bam_include_flags" / "bam_min_mapq", kmm_set_record_regions; DESIGN
    4.15).  Regions take samtools syntax (1-based, inclusive; `*` = the records without a reference), the file is BED.  For BAM
    the names are resolved against the file's header; SAM needs none.  They combine with `--exclude-flags`,
    `--use-record-qual`, `--original-strand`, `--shard-bam` and several ranks on SAM.
"""
import argparse
import logging
import os
import sys
import time

import numpy as np

from .distributed import chunk_owner
from .engine import DeviceIndex
from .kmer_index import KmerIndex
from . import _lib
from .reads_io import (MmapChunker, RawChunker, PrefetchingRawChunker, prefetch, probe_input, rank_byte_range, read_chunks,
                       records_cut)


def main():
    run_argument_parser(sys.argv[1:])


def _get_kmer_index_from_args(args):
    """util.py:38-68, restricted to plain KmerIndex (.npz) or an in-memory index object."""
    if args.kmer_index is None:
        if getattr(args, "index_bundle", None) is None:
            logging.error("Either a kmer index (-i) or an index bundle (-b) needs to be specified")
            sys.exit(1)
        logging.error("Index bundles (-b) are not supported by this build: pass the kmer index with -i")
        sys.exit(1)
    if not isinstance(args.kmer_index, (str, os.PathLike)):
        kmer_index = args.kmer_index          # already an index object (util.py:40-44), duck-typed
    else:
        if "minimal" in os.path.basename(str(args.kmer_index)):
            logging.error("MinimalKmerIndex files are not supported by this build")
            sys.exit(1)
        kmer_index = KmerIndex.from_file(args.kmer_index)
    if hasattr(kmer_index, "convert_to_int32"):
        kmer_index.convert_to_int32()
    if hasattr(kmer_index, "remove_ref_offsets"):
        kmer_index.remove_ref_offsets()
    return kmer_index


def map_cpu(args, kmer_index, chunk_sequence):
    """Per-chunk mapper with the reference's name and return value (command_line_interface.py:32-56):
    a fresh uint32 node-count vector for ONE chunk.  `chunk_sequence` is a ReadBatch (the reference
    passes a shared-memory name of the chunk; there is no process pool here).  N->A (:41), k-mer
    extraction (:42) and lookup (:51, default frequency filter 1000) all happen in the fused kernel."""
    from .mapper import _device_index
    from .util import as_read_batch
    k = args["kmer_size"] if isinstance(args, dict) else args.kmer_size
    batch = as_read_batch(chunk_sequence)
    max_node_id = kmer_index.max_node_id() if hasattr(kmer_index, "max_node_id") else int(np.max(kmer_index._nodes))
    dev = _device_index(kmer_index, max_node_id)
    dev.reset()
    dev.map_reads(batch.bases, batch.offsets, k)
    return dev.get_node_counts()


def host_threads(n_threads, world_size=1):
    """`-t` as the number of host threads that work on the read bytes of THIS rank: at most the cores the process may keep
    busy (affinity mask, cgroup quota), shared between the ranks of a node."""
    from . import _io
    return max(1, min(int(n_threads), _io.cpu_budget() // max(int(world_size), 1)))


def map_gpu(index, chunks, k, hash_map_size=0, map_reverse_complements=False,
            max_index_lookup_frequency=1000, device=0, rank=0, world_size=1, before_fetch=None, n_threads=16, lut=None):
    """command_line_interface.py:59-79 on the HIP engine: chunks -> fused kmm_map_reads calls.
    lut: the lookup table of every call (None: the default; util.ambiguous_skip_lut() for --ambiguous-bases skip).
    before_fetch(dev): called with the open handle after the last chunk and before the counts are copied to the
    host (the multi-rank reduce runs there, on the device)."""
    max_node_id = index.max_node_id() if hasattr(index, "max_node_id") else int(np.max(index._nodes))
    dev = DeviceIndex.from_index(index, max_node_id, device=device)
    dev.set_param("host_pack_threads", host_threads(n_threads, world_size) if n_threads > 1 else 0)
    t_start = time.perf_counter()
    n_kmers = 0
    try:
        for i, chunk in enumerate(chunks):
            if chunk is None:          # a chunk of a shared .gz stream that another rank maps
                continue
            t0 = time.perf_counter()
            L = chunk.uniform_length
            if L is not None:
                dev.map_reads_uniform(chunk.bases, len(chunk), L, k, max_index_lookup_frequency,
                                      also_revcomp=map_reverse_complements, lut=lut)
            else:
                dev.map_reads(chunk.bases, chunk.offsets, k, max_index_lookup_frequency,
                              also_revcomp=map_reverse_complements, lut=lut)
            n_kmers += chunk.n_kmers(k)
            logging.debug("GPU: chunk %d (%d reads) submitted in %.5f sec", i, len(chunk),
                          time.perf_counter() - t0)
        if before_fetch is not None:
            before_fetch(dev)
        node_counts = dev.get_node_counts()
    finally:
        dev.close()
    dt = time.perf_counter() - t_start
    logging.info("Time spent only on hashing and counting hashes: %.5f" % dt)
    logging.info("Mapped %d k-mers (%.1f M k-mers/s)" % (n_kmers, n_kmers / max(dt, 1e-9) / 1e6))
    return node_counts


def choose_route(fmt, probe, world_size, n_threads, has_device, env=os.environ, lut=None, min_base_quality=0, record_hits=False):
    """How map_gpu_raw reads the file: (route, populate, steer).  fmt: the GPU's record format ("fasta_ml" = wrapped FASTA);
    probe: reads_io.probe_input of the file; env: where the KMM_CLI_* switches of A/B runs are read.

    route "bam" / "bgzf" / "gzip": the compressed bytes go to the GPU as they lie in the file mapping and are inflated there
    (_map_compressed_file).  BGZF (.gz written by bgzip / htslib: independent members of <= 64 KiB): one GPU thread inflates one
    member — the host's inflater (10.8 GB/s of FASTQ on 16 cores) is out of the way; several ranks each take the members that
    start in their share of the compressed bytes (bgzf_ranges.py).  Plain gzip (`gzip reads.fq`: one deflate stream, no member
    sizes), one rank: speculative block starts, one lane per ~32 KiB of compressed bytes (kmm_map_gzip); opt-in
    (KMM_CLI_GPU_GUNZIP=1) until it beats the host inflater's route on the same box (profiles/gzip_gpu/).  BAM is
    told by its content, whatever its name.
    route "mmap": a plain FASTQ / two-line FASTA with host packing is mapped into memory and its chunks handed to the packer
    threads as views of the page cache (MmapChunker: no copy, nothing pinned).  populate: helper threads map its pages ahead
    (MADV_POPULATE_READ) while the index goes up — the 16 packer threads otherwise take a page fault per 64 KiB of a fresh
    mapping, all in one address space (profiles/r05/cli_populate_ab.txt); steer: the packer threads run next to the file's
    page-cache pages.
    route "prefetch": any other input the host inflates: two pinned buffers and a reader thread, the next batch is inflated
    while the GPU works on this one (BGZF 5.7 -> 6.5 GB/s end to end); plain files are read at memory speed and the second
    pinned buffer costs more than the overlap returns (3 GB FASTQ: 0.30 s with one buffer, 0.37 s with two), so they take
    route "raw": one pinned buffer (RawChunker).
    lut: a caller's lookup table (--ambiguous-bases skip) is never taken by the host packer, so route "mmap", which counts
    on it (pageable views of the page cache), gives way to "raw": the bytes cross PCIe from a pinned buffer.
    min_base_quality > 0: the same — the packer drops the quality lines the GPU is to read.
    record_hits: the same — the record-hits mode never takes the host packer."""
    gpu_inflate = probe.inflate and fmt in ("fastq", "fasta", "sam") and not env.get("KMM_CLI_NO_GPU_INFLATE")
    if fmt == "bam":
        return "bam", False, False
    if gpu_inflate and probe.container == "bgzf":
        return "bgzf", False, False
    if gpu_inflate and probe.container == "gzip" and world_size == 1 and env.get("KMM_CLI_GPU_GUNZIP", "") not in ("", "0"):
        return "gzip", False, False
    if probe.inflate:
        return ("raw" if env.get("KMM_CLI_NO_PREFETCH") else "prefetch"), False, False
    if (fmt in ("fastq", "fasta") and n_threads > 1 and has_device and lut is None and not min_base_quality
            and not record_hits and not env.get("KMM_CLI_NO_MMAP")):
        return "mmap", not env.get("KMM_CLI_NO_POPULATE"), not env.get("KMM_CLI_NO_PACKER_STEERING")
    return "raw", False, False


def map_gpu_raw(index, path, chunk_size, fmt, k, map_reverse_complements=False,
                max_index_lookup_frequency=1000, device=0, rank=0, world_size=1, before_fetch=None, n_threads=16,
                exclude_flags=0, probe=None, lut=None, min_base_quality=0, use_record_qual=False, original_strand=False,
                shard_bam=False, record_select=None, record_hits=None):
    """Same job as map_gpu, but the FASTQ / two-line FASTA records are parsed ON THE GPU
    (kmm_map_records): the host only reads (and for .gz inflates) raw bytes.  fmt "bam": a BAM file, inflated and decoded
    on the GPU (kmm_map_bam; exclude_flags = its "bam_exclude_flags").  fmt "sam": SAM text, plain, BGZF or gzip, its SEQ column
    extracted on the GPU (KMM_FORMAT_SAM on the routes of a FASTQ; exclude_flags filters it too).  probe: reads_io.probe_input
    of the file, if the caller has it.  lut: the lookup table of every call, on every route (None: the default).
    min_base_quality: the handle's "min_base_quality", set before the first map call on every route (FASTQ has qualities;
    SAM / BAM are refused before the index goes up unless use_record_qual is given; FASTA is mapped as before with a warning).
    use_record_qual: the handle's "use_record_qual" — the QUAL of SAM / BAM records is decoded on the GPU and the floor applied
    (DESIGN 4.12); records that store no qualities pass unmasked and are counted ("records_without_qual").
    original_strand: the handle's "original_strand", SAM / BAM alone — the kept records whose FLAG has 0x10 are mapped in read
    orientation (SEQ reverse-complemented back, QUAL reversed: DESIGN 4.13) and counted ("records_reversed").
    shard_bam: several ranks on one BAM file each map their member range, its ends trimmed to record starts found on the GPU
    (bgzf_ranges.rank_member_range_bam); without it several ranks on a BAM file are refused.
    record_select: check_record_select's dict (include flags, MAPQ floor, regions; SAM / BAM alone) or None: no
    selection, and no call that sets one.
    record_hits: RecordHitsSink or None — the handle's record-hits mode is switched on before the first map call, and the sink
    takes the pending entries after every map call, on every route (the queue stays chunk-sized); the node counts returned are
    then all zero; min_base_quality is then the MODE's floor ("record_hits_min_base_quality"), which the sink sets
    with the mode: "min_base_quality" with the mode on is refused by the library."""
    _check_bam_route(fmt, world_size, exclude_flags, shard_bam=shard_bam)
    record_select = check_record_select(fmt, **(record_select or {}))
    original_strand = check_original_strand(original_strand, fmt)
    use_record_qual = check_use_record_qual(use_record_qual, fmt, min_base_quality)
    min_base_quality = check_min_base_quality(min_base_quality, k, fmt, use_record_qual=use_record_qual)
    t_index = time.perf_counter()
    probe = probe_input(path) if probe is None else probe
    has_device = _lib.device_count() > 0
    # (decided BEFORE anything is made: the prefetching chunker starts a reader thread and page-locks two batch buffers —
    # making and freeing those cost the BGZF route 100 ms of its map phase until it was noticed)
    route, populate, steer = choose_route(fmt, probe, world_size, n_threads, has_device, lut=lut, min_base_quality=min_base_quality,
                                          record_hits=record_hits is not None)
    seekable = not probe.inflate
    # page-locked memory is slow to make (~50 ms per GB): the staging buffers of the host packer are made by a helper thread
    # WHILE the index is uploaded and repacked, not inside the map phase.  (The count vector needs none: kmm_get_node_counts
    # brings a large vector to ordinary memory through the handle's page-locked ring at the link's rate.)
    import threading
    prepared = {}

    def prepare_host_memory():
        try:
            size = os.stat(path).st_size
            _lib.check(_lib.lib().kmm_host_reserve(min(size // max(world_size, 1) + (1 << 20), 2 << 30)))
        except Exception as exc:                         # noqa: BLE001 - an optimisation: the map calls allocate what is missing
            logging.debug("host memory was not prepared ahead: %s", exc)

    helper = threading.Thread(target=prepare_host_memory, daemon=True)
    # (.gz input needs 128 MB of it, made in 7 ms by the first call that wants it; behind a helper thread the same allocation
    # came back 100 ms after the index upload it was meant to hide behind: profiles/r05/bgzf_e2e_v6_*.txt)
    if has_device and n_threads > 1 and seekable and lut is None and not min_base_quality and record_hits is None:  # (the packer's buffers: no packer
                                                                                             # with a table or a quality floor)
        helper.start()
    byte_range = rank_byte_range(path, fmt, rank, world_size) if (world_size > 1 and seekable) else None
    # the file mapping of route "mmap" is made HERE, and its pages populated, while the index goes up
    chunker = None
    if route == "mmap":
        chunker = MmapChunker(path, int(chunk_size), byte_range, pinned=True)
        if populate:
            chunker.populate(n_threads=max(1, min(4, host_threads(n_threads, world_size) // 2)))
    # (the scan for the largest node id — 30 ms on one thread for 10^8 entries — runs with the helpers above already at work)
    max_node_id = index.max_node_id() if hasattr(index, "max_node_id") else int(np.max(index._nodes))
    dev = DeviceIndex.from_index(index, max_node_id, device=device)
    logging.info("Index resident in HBM after %.3f sec (max_node_id scan + upload + repack)", time.perf_counter() - t_index)
    # -t: the host cores' share of the work (reference: command_line_interface.py:124-130,168) — reader / inflate threads
    # and the threads that pack the sequence lines to 2 bits per base inside kmm_map_records; -t 1 = no host packing,
    # the raw bytes cross PCIe and the GPU parses them
    n_host = host_threads(n_threads, world_size)
    dev.set_param("host_pack_threads", n_host if n_threads > 1 else 0)
    if min_base_quality and record_hits is None:
        dev.set_param("min_base_quality", min_base_quality)
    if record_hits is not None:
        record_hits.min_base_quality = min_base_quality      # (the checked floor: 0 for FASTA)
    if use_record_qual:
        dev.set_param("use_record_qual", 1)
    if original_strand:
        dev.set_param("original_strand", 1)
        _log_original_strand_filter(exclude_flags)
    if record_hits is not None:
        record_hits.open(dev)
        logging.info("Route: %s, records parsed on the GPU with the handle's record-hits mode", route)
    from . import _io
    _io.set_default_threads(n_host)
    logging.info("%d host thread(s) read and pack the read bytes (-t %d, CPU budget %d)", n_host, n_threads, _io.cpu_budget())
    if byte_range is not None:
        logging.info("Rank %d of %d maps bytes [%d, %d) of %s", rank, world_size, byte_range[0], byte_range[1], path)
    # GPU batches: the reference maps chunk by chunk (-c bytes, command_line_interface.py:109-111,169); here the chunks
    # of a large file are accumulated until one map call holds enough positions for the radix path to run well (a raw
    # FASTQ piece takes it from 2 x radix_min_units bytes on: its sequence lines are compacted into flat reads on the
    # device first, kmm_map_records), at most 2 GiB per call.
    batch_bytes = int(chunk_size)
    try:
        n_file = os.stat(path).st_size * (6.5 if not seekable else 1)
    except OSError:
        n_file = 0
    # (the record-hits mode never takes the radix path: its chunks stay -c bytes, and so does its queue)
    if dev.get_param("radix_available") and not os.environ.get("KMM_CLI_NO_BATCHING") and record_hits is None:
        # (radix_min_units is where the radix path BREAKS EVEN with the direct kernel, in base positions ~ half the
        # FASTQ bytes; a batch twelve times that runs within 20 % of the path's large-batch rate.  Larger batches would
        # run the GPU closer to its large-batch rate, but end to end the host is the bound — reading the file into pinned
        # memory at 8-11 GB/s — and several batches per file let that overlap the copies and kernels: a 3 GB FASTQ took
        # 0.27 s in five batches of 615 MB and 0.62 s as ONE batch, profiles/r04/cli_e2e_large_fastq.txt.)
        want = min(max(int(12 * dev.get_param("radix_min_units")), 256 << 20), 2 << 30)
        share = n_file / max(world_size, 1)
        if share >= want > batch_bytes:
            # equal batches, none below the threshold (a small last batch would take the direct path)
            batch_bytes = min(int(share / int(share // want)) + (1 << 20), 2 << 30) if seekable else want
            logging.info("Chunks of %d bytes are accumulated into GPU batches of %d bytes (radix path)", chunk_size, batch_bytes)
        elif seekable and share > batch_bytes and share >= 2.5 * dev.get_param("radix_min_units"):
            # a file (or a rank's share of one) between the radix path's break-even and the batch size above: ONE call.  Chunk
            # by chunk it is 271 direct-path calls for 675 MB — 39-42 ms of map calls against 7.5 + 4.4 ms of GPU tail as one
            # call packed by the host threads (profiles/r05/cli_mid_sized_file.txt)
            batch_bytes = min(int(share) + (1 << 20), 2 << 30)
            logging.info("Chunks of %d bytes are accumulated into ONE GPU batch of %d bytes (radix path)", chunk_size, batch_bytes)
    if route in ("prefetch", "raw"):
        chunker = (PrefetchingRawChunker if route == "prefetch" else RawChunker)(path, batch_bytes, byte_range, pinned=True)
    elif route == "mmap":
        chunker.chunk_size = batch_bytes
    steered_from = None
    if steer:
        # the packer threads are made by the first map call and inherit this thread's CPUs: next to the file's pages
        from .distributed import packer_cpus_near
        try:
            where = chunker.page_nodes()
            near = packer_cpus_near(where)
            if near is not None:
                steered_from = os.sched_getaffinity(0)
                os.sched_setaffinity(0, near[1])
                logging.info("The read file's page-cache pages lie on NUMA node %d (%s): its packer threads run there (%d CPUs), "
                             "the packed stream crosses to the GPU's node", near[0], where, len(near[1]))
        except (OSError, AttributeError) as exc:
            logging.debug("packer threads stay on the GPU's node: %s", exc)
    owns = (lambda i: True) if (world_size == 1 or seekable) else (lambda i: chunk_owner(i, world_size) == rank)
    # FASTQ and two-line FASTA are parsed as they are; FASTA with wrapped sequence lines is unwrapped on the GPU first
    kfmt = {"fastq": _lib.FORMAT_FASTQ, "fasta": _lib.FORMAT_FASTA2, "fasta_ml": _lib.FORMAT_FASTA, "bam": 0, "sam": _lib.FORMAT_SAM}[fmt]
    # SAM: lines parsed on the GPU, the SEQ column written as two-line FASTA there; BAM: records decoded there
    if fmt in ("sam", "bam"):
        dev.set_param("bam_exclude_flags", int(exclude_flags))
    if record_select:
        apply_record_select(dev, path, fmt, record_select, exclude_flags)
    t_start = time.perf_counter()
    n_reads = n_bytes = 0
    if route in ("bam", "bgzf", "gzip"):
        if helper.ident is not None:
            helper.join()
        return _map_compressed_file(dev, path, route, kfmt, k, max_index_lookup_frequency,
                                    map_reverse_complements, before_fetch, t_start, counts_out=prepared.get("counts"), rank=rank,
                                    world_size=world_size, fmt=fmt, lut=lut, min_base_quality=min_base_quality,
                                    use_record_qual=use_record_qual, original_strand=original_strand, shard_bam=shard_bam,
                                    record_select=bool(record_select), record_hits=record_hits)
    # (mates kept together in SAM output, DESIGN 4.28: the file's last chunk says so, and an unpaired last record fails it)
    sam_mates, said_last = fmt == "sam" and bool(getattr(record_hits, "sam_mates", False)), False
    try:
        i = 0
        while True:
            buf = chunker.next_chunk()
            if buf is None:
                break
            last = _lib.FORMAT_LAST_CHUNK if ((fmt == "fasta_ml" or sam_mates) and chunker.eof) else 0
            said_last = said_last or bool(last)
            if owns(i):
                used, n_rec = dev.map_records(buf, buf.shape[0], kfmt | last, k, max_index_lookup_frequency,
                                              also_revcomp=map_reverse_complements, lut=lut)
                if record_hits is not None:
                    record_hits.drain(dev)
            else:   # a chunk of a shared .gz stream that another rank maps: only its record boundary is needed,
                    # cut by the SAME rule as the GPU parser's `consumed` (newline count), at end of input too
                used, n_rec = records_cut(buf, fmt, chunker.eof), 0
            if used == 0:
                if chunker.eof:
                    raise ValueError("trailing bytes at end of %s do not form a complete record" % path)
                chunker.chunk_size *= 2          # a record longer than the chunk: read more
                continue
            n_reads += n_rec
            n_bytes += used
            chunker.consumed(used)
            i += 1
        if sam_mates and not said_last:              # (the reader met the end of the file behind its last chunk)
            dev.map_records(np.zeros(0, dtype=np.uint8), 0, kfmt | _lib.FORMAT_LAST_CHUNK, k, max_index_lookup_frequency,
                            also_revcomp=map_reverse_complements, lut=lut)
        t_calls = time.perf_counter()
        n_lookups, n_hits = dev.get_stats()
        n_radix, n_direct = dev.get_param("radix_batches"), dev.get_param("direct_batches")
        n_host_packed = dev.get_param("host_packed_record_calls")
        n_masked = dev.get_param("quality_masked_bases") if min_base_quality else None
        n_no_qual = dev.get_param("records_without_qual") if (min_base_quality and use_record_qual) else 0
        n_reversed = dev.get_param("records_reversed") if original_strand else None
        n_selected = (dev.get_param("sam_records"), dev.get_param("sam_records_excluded")) if record_select else None
        if before_fetch is not None:
            before_fetch(dev)
        if helper.is_alive() or helper.ident is not None:
            helper.join()
        t_fetch = time.perf_counter()
        node_counts = dev.get_node_counts(out=prepared.get("counts"))
        # (the reference's timer stops before its get_node_counts, command_line_interface.py:78-79; ours runs on through
        # the fetch, and says what the fetch was)
        if getattr(chunker, "populate_t1", None) is not None:
            logging.info("The file mapping's pages were populated in %.1f ms, done %.1f ms %s the first map call",
                         (chunker.populate_t1 - chunker.populate_t0) * 1e3, abs(t_start - chunker.populate_t1) * 1e3,
                         "before" if chunker.populate_t1 <= t_start else "AFTER")
        logging.info("%.1f ms in the map calls, %.1f ms until the GPU had finished them (= %.1f M k-mers/s up to where the "
                     "reference stops its timer), %.1f ms more until the node counts were on the host",
                     (t_calls - t_start) * 1e3, (t_fetch - t_calls) * 1e3, n_lookups / max(t_fetch - t_start, 1e-9) / 1e6,
                     (time.perf_counter() - t_fetch) * 1e3)
    finally:
        dt = time.perf_counter() - t_start
        chunker.close()
        dev.close()
        if steered_from is not None:                     # (this thread goes back to the GPU's node)
            try:
                os.sched_setaffinity(0, steered_from)
            except OSError:
                pass
    logging.info("Time spent only on hashing and counting hashes: %.5f" % dt)
    logging.info("Mapped %d reads from %d bytes (%.1f MB/s, GPU record parser): %d k-mer lookups "
                 "(%.1f M/s), %d index hits" % (n_reads, n_bytes, n_bytes / max(dt, 1e-9) / 1e6, n_lookups,
                                                  n_lookups / max(dt, 1e-9) / 1e6, n_hits))
    _log_quality_masked(min_base_quality, n_masked, n_no_qual)
    _log_records_reversed(n_reversed)
    _log_records_selected(n_selected)
    _log_path_taken(n_radix, n_direct, n_host_packed, record_hits)
    return node_counts


def check_record_select(fmt, include_flags=0, min_mapq=0, regions=None, regions_file=None):
    """--include-flags / --min-mapq / --regions / --regions-file as one dict, or None when none of them is given; on input that
    is neither SAM nor BAM they are refused, as --exclude-flags is; values the library would refuse are refused here."""
    include_flags, min_mapq = int(include_flags or 0), int(min_mapq or 0)
    regions = [r for r in (regions or []) if r]
    given = [name for name, v in (("--include-flags", include_flags), ("--min-mapq", min_mapq), ("--regions", regions),
                                  ("--regions-file", regions_file)) if v]
    if not given:
        return None
    if fmt not in ("bam", "sam"):
        raise ValueError("%s applies to SAM and BAM input only (the reads are %s)" % (given[0], fmt))
    if not 0 <= include_flags <= 0xFFFF:
        raise ValueError("--include-flags outside [0, 0xFFFF]")
    if not 0 <= min_mapq <= 255:
        raise ValueError("--min-mapq outside [0, 255]")
    if regions and not regions_file and all(t.strip() == "*" for r in regions for t in str(r).split(",")):
        # (a list of no regions is no list — kmm_set_record_regions clears it — so '*' has nothing to add the unplaced records to)
        raise ValueError("--regions '*' alone selects nothing: it adds the records without a reference to a region list; give "
                         "--include-flags 4 for the unmapped records, or a region beside it")
    return dict(include_flags=include_flags, min_mapq=min_mapq, regions=regions, regions_file=regions_file)


def resolve_record_regions(path, fmt, select):
    """The regions of --regions and --regions-file as ([(ref_name, ref_id, beg, end)], keep_unplaced): for BAM against the
    references of the file's header (an unknown name is an error that names it), for SAM by name alone."""
    from . import reads_io, util
    references = reads_io.bam_references(path) if fmt == "bam" else None
    regions, keep_unplaced = [], False
    for text in select["regions"]:
        got, unplaced = util.parse_regions(text, references)
        regions += got
        keep_unplaced = keep_unplaced or unplaced
    if select["regions_file"]:
        regions += util.read_bed_regions(select["regions_file"], references)
    return regions, keep_unplaced


def apply_record_select(dev, path, fmt, select, exclude_flags=0):
    """The selection set on the handle, and one line that says which rules are in force."""
    if select["include_flags"]:
        dev.set_param("bam_include_flags", select["include_flags"])
    if select["min_mapq"]:
        dev.set_param("bam_min_mapq", select["min_mapq"])
    regions, keep_unplaced = resolve_record_regions(path, fmt, select)
    if regions:
        dev.set_record_regions(regions, keep_unplaced)
    elif keep_unplaced:                    # (an empty --regions-file beside '*': check_record_select has refused '*' alone)
        raise ValueError("--regions '*' with no region beside it selects nothing: give --include-flags 4 for the unmapped records")
    logging.info("Records are selected on the GPU: exclude flags 0x%x, include flags 0x%x, MAPQ >= %d, %s", int(exclude_flags),
                 select["include_flags"], select["min_mapq"],
                 "%d region(s) (%d after merging)%s" % (len(regions), dev.get_param("record_regions"),
                                                       ", and the records without a reference" if keep_unplaced else "")
                 if regions else "no region list")


def _log_records_selected(n_selected):
    if n_selected is not None:
        logging.info("Record selection: %d records kept and mapped, %d excluded" % tuple(n_selected))


def _log_quality_masked(min_base_quality, n_masked, n_no_qual=0):
    if min_base_quality:
        logging.info("quality_masked_bases: %d bases below Q%d, no k-mer over them counted", n_masked, min_base_quality)
        if n_no_qual:
            logging.info("records_without_qual: %d records store no qualities (QUAL '*' / 0xFF): they passed Q%d unmasked",
                         n_no_qual, min_base_quality)


def _log_records_reversed(n_reversed):
    if n_reversed is not None:
        logging.info("records_reversed: %d records with FLAG 0x10 were mapped in read orientation (--original-strand)", n_reversed)


def _log_original_strand_filter(exclude_flags):
    """--original-strand asks for the reads as sequenced: one line when the flag filter lets partial or repeated ones through."""
    if int(exclude_flags) & 0x900 != 0x900:
        logging.info("--original-strand without --exclude-flags 0x900: secondary and supplementary records hold partial or repeated "
                     "reads, and `samtools fastq` leaves them out")


def check_original_strand(original_strand, fmt):
    """--original-strand against what it cannot go with; returns whether it applies."""
    if not original_strand:
        return False
    if fmt not in ("sam", "bam"):
        raise ValueError("--original-strand applies to SAM and BAM input only (the reads are %s)" % fmt)
    return True


def check_use_record_qual(use_record_qual, fmt, min_base_quality):
    """--use-record-qual against what it cannot go with; returns whether it applies (not without a floor: one warning)."""
    if not use_record_qual:
        return False
    if fmt not in ("sam", "bam"):
        raise ValueError("--use-record-qual applies to SAM and BAM input only (the reads are %s)" % fmt)
    if not int(min_base_quality or 0):
        logging.warning("--use-record-qual has no effect without --min-base-quality: QUAL is not read")
        return False
    return True


def check_min_base_quality(min_base_quality, k, fmt=None, host_parser=False, use_record_qual=False):
    """--min-base-quality against what it cannot go with, before anything is uploaded; returns the floor that applies (0 for
    FASTA, which has no qualities, after one warning).  fmt None: the format is not known yet (the argument parser).
    use_record_qual: SAM and BAM are served — their QUAL is decoded on the GPU (--use-record-qual)."""
    q = int(min_base_quality or 0)
    if not 0 <= q <= 93:
        raise ValueError("--min-base-quality must lie in 0 .. 93 (Phred+33 qualities are '!' .. '~')")
    if q == 0:
        return 0
    if k < 2:
        raise ValueError("--min-base-quality needs -k 2 or more")
    if fmt in ("sam", "bam") and not use_record_qual:
        raise ValueError("--min-base-quality applies to FASTQ input: the QUAL column of %s records is not carried to the GPU "
                         "(convert to FASTQ, or drop the option; or pass --use-record-qual to have it decoded there: records "
                         "that store no qualities then pass the floor unmasked)" % fmt.upper())
    if host_parser:
        raise ValueError("--min-base-quality reads the qualities on the GPU: the host parser hands it reads without them "
                         "(drop --host-parser)")
    if fmt in ("fasta", "fasta_ml"):
        logging.warning("--min-base-quality %d has no effect on FASTA input: it has no qualities", q)
        return 0
    return q


def _log_path_taken(n_radix, n_direct, n_host_packed=0, record_hits=None):
    if record_hits is not None:
        logging.info("path_taken: direct records front end, record-hits mode (no node was counted: %d entries taken)",
                     sum(len(h) for h in record_hits.hits))
        return
    logging.info("path_taken: %s (%d batches on the radix path, %d on the direct path; %d batches packed to 2 bits per base "
                 "by the host threads)"
                 % ("radix" if n_radix and not n_direct else "direct" if n_direct and not n_radix else "mixed", n_radix, n_direct,
                    n_host_packed))


_GZIP_CALL_INFLATED = 3 << 30      # inflated bytes a kmm_map_gzip window is sized for (a call takes at most 3.5 GiB)
_BGZF_CALL_INFLATED = 3150 << 20   # inflated bytes per kmm_map_bgzf call: under what a call takes (3.5 GiB; 3.25 GiB for a window staged ahead)

# per route: the counters its summary line reports, and that line
_COMPRESSED_ROUTES = {
    "gzip": (("gzip_members", "gzip_chunks"),
             "Mapped %d reads from %d compressed bytes (%.1f MB/s compressed; gzip stream inflated on the GPU: %d members, "
             "%d chunks): %d k-mer lookups (%.1f M/s), %d index hits"),
    "bgzf": (("bgzf_members",),
             "Mapped %d reads from %d compressed bytes (%.1f MB/s compressed; %d BGZF members inflated on the GPU): %d k-mer "
             "lookups (%.1f M/s), %d index hits"),
    "bam": (("bgzf_members", "bam_records_excluded", "bam_false_starts"),
            "Mapped %d BAM records from %d compressed bytes (%.1f MB/s compressed; %d BGZF members inflated and the records "
            "decoded on the GPU; %d records excluded by flag, %d false record starts): %d k-mer lookups (%.1f M/s), %d index "
            "hits"),
}


def _map_compressed_file(dev, path, route, kfmt, k, max_freq, revcomp, before_fetch, t_start, counts_out=None, rank=0,
                         world_size=1, fmt="fastq", lut=None, min_base_quality=0, use_record_qual=False, original_strand=False,
                         shard_bam=False, record_select=False, record_hits=None):
    """`kmer_mapper map -f reads.fq.gz | reads.bam` with the GPU inflater: windows of the file mapping -> kmm_map_<route>.

    route "gzip" (PLAIN gzip, kmm_map_gzip): each call goes on where the one before could verify a deflate block boundary.
    route "bgzf" / "bam" (kmm_map_bgzf / kmm_map_bam): each window starts at a member boundary; members are inflated and the
    records parsed (BAM: found and their SEQ decoded) on the GPU, and the handle carries the bytes behind a window's last
    complete record to the next one.  BGZF with several ranks: each maps its member range (bgzf_ranges.rank_member_range),
    the first member's head and the last member's tail trimmed to the record boundaries the ranks agree on.  BAM with several
    ranks (shard_bam): the same, the boundaries found on the GPU (bgzf_ranges.rank_member_range_bam); the ranks behind the
    first start their stream behind the header (mid_stream), and a rank whose share is empty makes no map call.
    record_hits: as map_gpu_raw's — the sink takes the pending entries after every map call."""
    import mmap
    counters, summary = _COMPRESSED_ROUTES[route]
    n_reads = lo = size = 0
    if route == "gzip":
        logging.info("Route: gzip stream inflated on the GPU (kmm_map_gzip)")
    try:
        with open(path, "rb") as f:
            file_size = os.fstat(f.fileno()).st_size
            mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
            try:
                lo, size, head_skip, tail_stop, mid_stream = 0, file_size, 0, None, False
                if world_size > 1:                       # (BGZF text, and BAM with shard_bam: gzip is mapped by one rank)
                    from . import bgzf_ranges
                    if route == "bam":
                        t_range = time.perf_counter()
                        lo, s0, hi, s1, n_ref = bgzf_ranges.rank_member_range_bam(dev, mm, rank, world_size)
                        mid_stream = (lo, s0) > (0, 0)
                        if mid_stream:
                            dev.set_param("bam_n_ref", n_ref)
                        logging.info("Rank %d of %d found its BAM record boundaries on the GPU in %.1f ms (n_ref %d)", rank, world_size,
                                     (time.perf_counter() - t_range) * 1e3, n_ref)
                    else:
                        lo, s0, hi, s1 = bgzf_ranges.rank_member_range(mm, fmt, rank, world_size)
                    size = bgzf_ranges.member_end(mm, hi) if s1 > 0 else hi
                    head_skip, tail_stop = s0, (s1 if s1 > 0 else None)
                    if route == "bam" and (hi, s1) <= (lo, s0):   # an empty share: no map call, the rank still joins the reduce
                        size = lo
                    logging.info("Rank %d of %d maps the BGZF members in compressed bytes [%d, %d) of %d: %d inflated bytes of the "
                                 "first member skipped, %s of the last one taken", rank, world_size, lo, size, file_size, s0,
                                 "all" if tail_stop is None else "%d bytes" % s1)
                if hasattr(mm, "madvise") and hasattr(mmap, "MADV_SEQUENTIAL"):
                    mm.madvise(mmap.MADV_SEQUENTIAL)
                whole = np.frombuffer(mm, dtype=np.uint8)
                if route == "gzip":
                    # windows of ~3 GiB INFLATED: the first from a typical FASTQ ratio, every later one from the ratio of what
                    # the calls before inflated (the trailer's ISIZE is the size mod 2^32: no guide for the large files)
                    inflated0 = dev.get_param("gzip_inflated_bytes")
                    window = int(_GZIP_CALL_INFLATED / 4.5)
                    pos = 0
                    t_calls = time.perf_counter()
                    while pos < size:
                        end = min(pos + window, size)
                        if size - end < window // 4:     # (no short tail call: a call's time is its slowest lane's)
                            end = size
                        used, n_rec = dev.map_gzip(whole[pos:end], fmt=kfmt, k=k, max_index_lookup_frequency=max_freq,
                                                   also_revcomp=revcomp, first=pos == 0, last=end == size, lut=lut)
                        if record_hits is not None:
                            record_hits.drain(dev)
                        n_reads += n_rec
                        if used == 0:
                            if end == size:
                                raise ValueError("trailing bytes of %s are no complete gzip member" % path)
                            window *= 2                  # no whole deflate block in the window: a longer one
                            continue
                        pos += used
                        ratio = max((dev.get_param("gzip_inflated_bytes") - inflated0) / pos, 1.0)
                        window = min(max(int(_GZIP_CALL_INFLATED / ratio), 1 << 20), 2 << 30)
                else:
                    # equal windows, none small: one GPU thread inflates one member, a call's time is one member's (~tens of
                    # milliseconds) whatever its size — so as FEW calls as their inflated size allows: the compressed bytes of
                    # a call follow from the file's own ratio (its first members' ISIZE against their sizes; FASTQ with binned
                    # qualities 3.3, with forty quality values 2.1 — one call instead of two for 1.5 GB of it)
                    from . import bgzf_ranges as _br
                    per_call = int(_BGZF_CALL_INFLATED / max(1.0, _br.inflation_ratio(mm, lo, size)))
                    n_calls = max(1, -(-(size - lo) // per_call))
                    pos, window = lo, (size - lo) // n_calls + (1 << 16)
                    t_calls = time.perf_counter()
                    end = min(lo + window, size)         # windows END at fixed places; a window starts where the one before
                    while pos < size:                    # it ran out of whole members (at most 64 KiB in front of that end)
                        nxt = min(end + window, size)
                        # each window is announced to the call before it (next_chunk: staged under that call's inflate kernel)
                        common = dict(first=pos == lo, last=end == size, k=k, max_index_lookup_frequency=max_freq,
                                      also_revcomp=revcomp, next_chunk=whole[end:nxt] if nxt > end else None, lut=lut)
                        if route == "bam":
                            used, n_rec = dev.map_bam(whole[pos:end], mid_stream=mid_stream and pos == lo,
                                                      head_skip=head_skip if pos == lo else 0,
                                                      tail_stop=tail_stop if end == size else None, **common)
                            if record_hits is not None:
                                record_hits.drain(dev)
                            if used == 0 and end == size:
                                raise ValueError("%s: the BAM header or the trailing bytes are no complete BGZF member" % path)
                            if used == 0 and pos == lo:  # a header longer than the window: a longer one
                                end = nxt
                                continue
                        else:
                            used, n_rec = dev.map_bgzf(whole[pos:end], fmt=kfmt, head_skip=head_skip if pos == lo else 0,
                                                       tail_stop=tail_stop if end == size else None, **common)
                            if record_hits is not None:
                                record_hits.drain(dev)
                            if used == 0 and end == size:
                                raise ValueError("trailing bytes of %s are no complete BGZF member" % path)
                        pos += used
                        n_reads += n_rec
                        if pos < end and end == size:    # the last window held more than one call takes: go on
                            continue
                        end = nxt
                del whole
            finally:
                try:
                    mm.close()
                except BufferError:
                    pass
        n_lookups, n_hits = dev.get_stats()
        counts = [dev.get_param(c) for c in counters]
        n_masked = dev.get_param("quality_masked_bases") if min_base_quality else None
        n_no_qual = dev.get_param("records_without_qual") if (min_base_quality and use_record_qual) else 0
        n_reversed = dev.get_param("records_reversed") if original_strand else None
        n_selected = None
        if record_select:
            which = "bam" if route == "bam" else "sam"
            n_selected = (dev.get_param(which + "_records"), dev.get_param(which + "_records_excluded"))
        n_radix, n_direct = dev.get_param("radix_batches"), dev.get_param("direct_batches")
        if before_fetch is not None:
            before_fetch(dev)
        t_fetch = time.perf_counter()
        node_counts = dev.get_node_counts(out=counts_out)
        logging.info("%.0f ms in kmm_map_%s, %.0f ms more until the node counts were on the host",
                     (t_fetch - t_calls) * 1e3, route, (time.perf_counter() - t_fetch) * 1e3)
    finally:
        dt = time.perf_counter() - t_start
        dev.close()
    logging.info("Time spent only on hashing and counting hashes: %.5f" % dt)
    logging.info(summary % (n_reads, size - lo, (size - lo) / max(dt, 1e-9) / 1e6, *counts, n_lookups,
                            n_lookups / max(dt, 1e-9) / 1e6, n_hits))
    _log_quality_masked(min_base_quality, n_masked, n_no_qual)
    _log_records_reversed(n_reversed)
    _log_records_selected(n_selected)
    _log_path_taken(n_radix, n_direct, record_hits=record_hits)
    return node_counts


def _check_bam_route(fmt, world_size, exclude_flags, shard_bam=False):
    """What the BAM route does only when asked (shard_bam): several ranks on one file; and the flag filter is for SAM and BAM alone."""
    if fmt == "bam" and world_size > 1 and not shard_bam:
        raise ValueError("BAM input is mapped by one rank: sharding a BAM file over %d ranks needs the ranks to resynchronise "
                         "to its records, which is not implemented (run without torchrun, WORLD_SIZE=1)" % world_size +
                         "; or pass --shard-bam: the ranks then find their record boundaries on the GPU")
    if exclude_flags and fmt not in ("bam", "sam"):
        raise ValueError("--exclude-flags applies to SAM and BAM input only (the reads are %s)" % fmt)


def map_bnp(args):
    if args.debug:
        logging.info("Will print debug log")
        logging.getLogger().setLevel(logging.DEBUG)

    k = args.kmer_size
    start_time = time.perf_counter()
    if getattr(args, "original_strand", False):    # (refused here: before the index file is read)
        check_original_strand(True, probe_input(args.reads).fmt)
    select_args = dict(include_flags=getattr(args, "include_flags", 0), min_mapq=getattr(args, "min_mapq", 0),
                       regions=getattr(args, "regions", None), regions_file=getattr(args, "regions_file", None))
    if any(select_args.values()):                  # (likewise)
        check_record_select(probe_input(args.reads).fmt, **select_args)
    kmer_index = _get_kmer_index_from_args(args)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    max_freq = args.max_hits_per_kmer if getattr(args, "apply_max_hits_per_kmer", False) else 1000

    device = local_rank if world > 1 else getattr(args, "device", 0)
    backend = os.environ.get("KMM_DIST_BACKEND", "nccl")      # "gloo": rehearsal of the N>1 flow on one GPU
    if world > 1 and backend == "gloo":
        device = local_rank % max(_lib.device_count(), 1)
    before_fetch = None
    if world > 1:
        import torch
        import torch.distributed as dist
        from .distributed import init_rccl_comm, reduce_node_counts
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if backend == "nccl" and torch.cuda.is_available():
                torch.cuda.set_device(local_rank)
                dist.init_process_group("nccl")
            else:
                dist.init_process_group("gloo")
        if dist.get_backend() == "nccl":
            # the additive reduce of command_line_interface.py:124-130 as ONE RCCL sum on the device, in place on the
            # handle's count vector (kmm_comm_reduce_counts); torch.distributed only carries the 128-byte communicator id
            def before_fetch(dev):
                t0 = time.perf_counter()
                init_rccl_comm(dev)
                dev.comm_reduce_counts(root=0)
                logging.info("Rank %d: RCCL reduce of the node counts on the device: %.5f sec", rank, time.perf_counter() - t0)
    # the process next to its GPU: reader / packing threads and their page-locked buffers on that NUMA node (16 threads pack
    # 172 GB/s of FASTQ from the GPU's own node, 132 spread over both sockets: profiles/r05/hostpack_rate.txt)
    from .distributed import bind_to_gpu_numa_node
    logging.info("Rank %d: host side bound to its GPU's NUMA node: %s", rank, bind_to_gpu_numa_node(device))
    # (the read file is opened first HERE, on the GPU's NUMA node — but for --original-strand, whose check above has read its
    # first bytes already, to refuse before the index file is read)
    probe = probe_input(args.reads)
    n_bytes = os.stat(args.reads).st_size
    if probe.inflate:
        n_bytes *= 6.5  # rough estimate for gzipped to give a progress (reference :92-93)
    logging.info("N bytes of reads: %d" % n_bytes)
    logging.info("Approx number of chunks of %d bytes: %d" % (args.chunk_size, int(n_bytes / args.chunk_size)))
    revcomp = bool(getattr(args, "map_reverse_complements", False))
    fmt = probe.fmt
    exclude_flags = int(getattr(args, "exclude_flags", 0) or 0)
    shard_bam = bool(getattr(args, "shard_bam", False))
    _check_bam_route(fmt, world, exclude_flags, shard_bam=shard_bam)
    lut = None
    if getattr(args, "ambiguous_bases", "a") == "skip":
        from .util import ambiguous_skip_lut
        lut = ambiguous_skip_lut()
        if k < 2:
            raise ValueError("--ambiguous-bases skip needs -k 2 or more")
    use_qual = check_use_record_qual(bool(getattr(args, "use_record_qual", False)), fmt, getattr(args, "min_base_quality", 0))
    min_q = check_min_base_quality(getattr(args, "min_base_quality", 0), k, fmt, bool(getattr(args, "host_parser", False)),
                                   use_record_qual=use_qual)
    original_strand = check_original_strand(bool(getattr(args, "original_strand", False)), fmt)
    record_select = check_record_select(fmt, **select_args)
    if fmt == "bam" and getattr(args, "host_parser", False):
        raise ValueError("--host-parser does not read BAM: its records are decoded on the GPU (drop --host-parser)")
    if fmt == "sam" and getattr(args, "host_parser", False):
        raise ValueError("--host-parser does not read SAM: its SEQ column is extracted on the GPU (drop --host-parser)")
    if not getattr(args, "host_parser", False):
        if fmt == "fasta" and not probe.two_line:
            fmt = "fasta_ml"           # wrapped sequence lines: unwrapped on the GPU (KMM_FORMAT_FASTA)
        node_counts = map_gpu_raw(kmer_index, args.reads, args.chunk_size, fmt, k, revcomp, max_freq,
                                  device=device, rank=rank, world_size=world, before_fetch=before_fetch,
                                  n_threads=args.n_threads, exclude_flags=exclude_flags, probe=probe, lut=lut,
                                  min_base_quality=min_q, use_record_qual=use_qual, original_strand=original_strand,
                                  shard_bam=shard_bam, **({"record_select": record_select} if record_select else {}))
    else:
        logging.info("Using the host FASTA/FASTQ parser")
        if world > 1 and not probe.inflate:
            chunks = read_chunks(args.reads, min_chunk_size=args.chunk_size,
                                 byte_range=rank_byte_range(args.reads, fmt, rank, world))
        elif world > 1:
            chunks = read_chunks(args.reads, min_chunk_size=args.chunk_size,
                                 owned=lambda i: chunk_owner(i, world) == rank)
        else:
            chunks = read_chunks(args.reads, min_chunk_size=args.chunk_size)
        chunks = prefetch(chunks)
        node_counts = map_gpu(kmer_index, chunks, k, getattr(args, "gpu_hash_map_size", 0), revcomp,
                              max_freq, device=device, rank=rank, world_size=world, before_fetch=before_fetch,
                              n_threads=args.n_threads, lut=lut)

    if world > 1:
        if before_fetch is None:        # gloo rehearsal on a 1-GPU box: the sum runs on the host copies
            t = torch.from_numpy(node_counts.view(np.int32).copy())
            reduce_node_counts(t, dst=0)
            node_counts = t.numpy().view(np.uint32)
        if rank != 0:
            return node_counts

    if args.output_file is None:
        return node_counts

    np.save(args.output_file, node_counts)
    logging.info("Saved node counts to %s.npy" % args.output_file)
    logging.info("Spent %.3f sec in total mapping kmers using %d threads"
                 % (time.perf_counter() - start_time, args.n_threads))
    return node_counts


class RecordHitsSink:
    """The per-call hook of the shared drivers (map_gpu_raw, _map_compressed_file) for the record-hits mode:
    open(dev) switches the mode on, drain(dev) takes what is pending after a map call; result() is the whole file's (hits,
    windows), in file order."""

    def __init__(self, windows=True, min_base_quality=0):
        self.windows = bool(windows)
        self.min_base_quality = int(min_base_quality or 0)   # the mode's floor, set with the mode
        self.hits, self.wins = [], []

    def open(self, dev):
        dev.record_hits(True, windows=self.windows, **({"min_base_quality": self.min_base_quality} if self.min_base_quality else {}))

    def drain(self, dev):
        if dev.get_param("record_hits_pending"):
            got = dev.take_record_hits()
            self.hits.append(got[0] if self.windows else got)
            if self.windows:
                self.wins.append(got[1])

    def result(self):
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, np.uint32)
        return cat(self.hits), (cat(self.wins) if self.windows else None)


_READ_HITS_SELECTION = (("--exclude-flags", "exclude_flags"), ("--include-flags", "include_flags"), ("--min-mapq", "min_mapq"),
                        ("--regions", "regions"), ("--regions-file", "regions_file"), ("--original-strand", "original_strand"))


def check_read_hits_input(fmt, world_size, device_parser=False, selection=()):
    """`kmer_mapper read-hits` takes FASTA / FASTQ in one process — with --device-parser also SAM and BAM, and the options
    that select their records (selection: the names of those given); everything else is refused before the index is read."""
    if selection and not device_parser:
        raise ValueError("%s needs --device-parser: records are selected where they are parsed, on the GPU" % selection[0])
    if selection and fmt not in ("sam", "bam"):
        raise ValueError("%s applies to SAM and BAM input only (the reads are %s)" % (selection[0], fmt))
    if fmt in ("sam", "bam") and not device_parser:
        raise ValueError("read-hits does not read %s files: per-read hits are implemented for FASTA and FASTQ (plain or .gz) "
                         "only; SAM and BAM input is out of scope" % fmt.upper())
    if world_size > 1:
        raise ValueError("read-hits runs in one process: WORLD_SIZE=%d (torchrun) is out of scope, run it without torchrun"
                         % world_size)


def read_hits_file(args):
    """`kmer_mapper read-hits`: per read of a FASTA / FASTQ file, in file order, the number of its k-mers that are in the
    index (kmm_read_hits) -> <out>.npy (uint32), with --windows also the number of windows looked up -> <out>.windows.npy.
    With --device-parser the records are parsed on the GPU (read_hits_file_device), and SAM and BAM are read too."""
    k = args.kmer_size
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device_parser = bool(getattr(args, "device_parser", False))
    if int(getattr(args, "min_base_quality", 0) or 0) and not device_parser:
        # (the floor lives in the library's record-hits mode, DESIGN 4.27: flat reads carry no qualities to kmm_read_hits)
        logging.info("read-hits: --min-base-quality implies --device-parser: the qualities are read where the records are parsed, "
                     "on the GPU")
        device_parser = True
    selection = [opt for opt, name in _READ_HITS_SELECTION if getattr(args, name, None)]
    probe = probe_input(args.reads)
    check_read_hits_input(probe.fmt, world, device_parser, selection)
    if device_parser:
        return read_hits_file_device(args, probe)
    lut = None
    if args.ambiguous_bases == "skip":
        from .util import ambiguous_skip_lut
        lut = ambiguous_skip_lut()
        if k < 2:
            raise ValueError("--ambiguous-bases skip needs -k 2 or more")
    kmer_index = _get_kmer_index_from_args(args)
    max_node_id = kmer_index.max_node_id() if hasattr(kmer_index, "max_node_id") else int(np.max(kmer_index._nodes))
    revcomp = bool(args.map_reverse_complements)
    hits, wins = [], []
    dev = DeviceIndex.from_index(kmer_index, max_node_id, device=args.device)
    try:
        for chunk in prefetch(read_chunks(args.reads, min_chunk_size=args.chunk_size)):
            L = chunk.uniform_length
            if L is not None:
                res = dev.read_hits(chunk.bases, n_reads=len(chunk), read_len=L, k=k, max_index_lookup_frequency=args.max_hits_per_kmer,
                                    also_revcomp=revcomp, lut=lut, windows=True)
            else:
                res = dev.read_hits(chunk.bases, chunk.offsets, k=k, max_index_lookup_frequency=args.max_hits_per_kmer,
                                    also_revcomp=revcomp, lut=lut, windows=True)
            hits.append(res[0])
            wins.append(res[1])
    finally:
        dev.close()
    hits = np.concatenate(hits) if hits else np.zeros(0, np.uint32)
    wins = np.concatenate(wins) if wins else np.zeros(0, np.uint32)
    return _save_read_hits(args, hits, wins)


def read_hits_file_device(args, probe):
    """`kmer_mapper read-hits --device-parser`: the file goes down the route `map` would choose for it in one process
    (choose_route: raw records, BGZF, gzip, SAM, BAM — parsed, inflated and selected on the GPU) with the handle's record-hits
    mode on; the pending entries are taken after every map call."""
    k = args.kmer_size
    fmt = probe.fmt
    select = check_record_select(fmt, include_flags=args.include_flags, min_mapq=args.min_mapq, regions=args.regions,
                                 regions_file=args.regions_file)
    original_strand = check_original_strand(bool(args.original_strand), fmt)
    _check_bam_route(fmt, 1, int(args.exclude_flags or 0))
    # (the checks of `map`, before the index is read: k >= 2, SAM / BAM with --use-record-qual, FASTA warned about and served)
    use_qual = check_use_record_qual(bool(getattr(args, "use_record_qual", False)), fmt, getattr(args, "min_base_quality", 0))
    min_q = check_min_base_quality(getattr(args, "min_base_quality", 0), k, fmt, use_record_qual=use_qual)
    lut = None
    if args.ambiguous_bases == "skip":
        from .util import ambiguous_skip_lut
        lut = ambiguous_skip_lut()
        if k < 2:
            raise ValueError("--ambiguous-bases skip needs -k 2 or more")
    kmer_index = _get_kmer_index_from_args(args)
    if fmt == "fasta" and not probe.two_line:
        fmt = "fasta_ml"
    sink = RecordHitsSink(windows=True)
    logging.info("read-hits: records parsed on the GPU, record-hits mode (--device-parser)")
    map_gpu_raw(kmer_index, args.reads, args.chunk_size, fmt, k, bool(args.map_reverse_complements), args.max_hits_per_kmer,
                device=args.device, n_threads=16, exclude_flags=int(args.exclude_flags or 0), probe=probe, lut=lut,
                original_strand=original_strand, record_hits=sink, min_base_quality=min_q, use_record_qual=use_qual,
                **({"record_select": select} if select else {}))
    hits, wins = sink.result()
    return _save_read_hits(args, hits, wins)


def _save_read_hits(args, hits, wins):
    n_reads, n_sel = hits.shape[0], int((hits >= args.min_hits).sum())
    logging.info("%d reads; %d (%.2f %%) have at least %d k-mer%s in the index", n_reads, n_sel,
                 100.0 * n_sel / max(n_reads, 1), args.min_hits, "" if args.min_hits == 1 else "s")
    if args.output_file is not None:
        np.save(args.output_file, hits)
        logging.info("Saved per-read hits to %s.npy" % args.output_file)
        if args.windows:
            np.save(str(args.output_file) + ".windows", wins)
            logging.info("Saved per-read windows to %s.windows.npy" % args.output_file)
    return (hits, wins) if args.windows else hits


def check_assign_reads_input(fmt, world_size, k, ambiguous_bases, min_votes, min_margin):
    """`kmer_mapper assign-reads` takes FASTA / FASTQ (plain or .gz) in one process; what it does not serve is refused before
    the index is read, with what to do instead."""
    if fmt in ("sam", "bam"):
        raise ValueError("assign-reads does not read %s files: per-read node assignment is implemented for FASTA and FASTQ "
                         "(plain or .gz) only; SAM and BAM input is out of scope (convert the reads to FASTQ first, e.g. with "
                         "`kmer_mapper select-reads --bam-to-fastq`)" % fmt.upper())
    if world_size > 1:
        raise ValueError("assign-reads runs in one process: WORLD_SIZE=%d (torchrun) is out of scope, run it without torchrun"
                         % world_size)
    if ambiguous_bases == "skip" and k < 2:
        raise ValueError("--ambiguous-bases skip needs -k 2 or more")
    if min_votes < 0:
        raise ValueError("--min-votes %d is negative: give 0 or more (1, the default, assigns every read with a vote)" % min_votes)
    if min_margin < 0:
        raise ValueError("--min-margin %d is negative: give 0 or more (0, the default, lets a tie go to the smallest node id)"
                         % min_margin)


def assign_rule(best_node, best_votes, second_votes, min_votes=1, min_margin=0):
    """The node a read is assigned to: its best node, or -1 when best_votes < min_votes or best_votes - second_votes <
    min_margin (a read without a vote has best_node -1 already) -> int32."""
    best_votes, second_votes = np.asarray(best_votes, dtype=np.int64), np.asarray(second_votes, dtype=np.int64)
    ok = (best_votes >= min_votes) & (best_votes - second_votes >= min_margin)
    return np.where(ok, np.asarray(best_node, dtype=np.int32), np.int32(-1)).astype(np.int32)


def read_node_names(path, n_nodes=None):
    """Line i of `path` names node i (the file `kmer_mapper index --names-output` wrote); fewer lines than nodes are refused
    (n_nodes None: the lines are read, check_node_names compares them once the node count is known)."""
    with open(path) as f:
        names = [line.rstrip("\n") for line in f]
    return names if n_nodes is None else check_node_names(path, names, n_nodes)


def check_node_names(path, names, n_nodes):
    if len(names) < n_nodes:
        raise ValueError("--names %s has %d lines and the index has %d nodes: line i names node i; give the file that "
                         "`kmer_mapper index --names-output` wrote for this index" % (path, len(names), n_nodes))
    return names


def write_assign_summary(path, assigned, n_nodes, names=None):
    """One line per node and one for the unassigned reads: node id, name, reads assigned, share of all reads."""
    assigned = np.asarray(assigned)
    counts = np.bincount(assigned[assigned >= 0], minlength=n_nodes)
    n = max(assigned.shape[0], 1)
    with open(path, "w") as f:
        f.write("node\tname\treads\tshare\n")
        for v in range(counts.shape[0]):
            f.write("%d\t%s\t%d\t%.6f\n" % (v, names[v] if names is not None and v < len(names) else "", counts[v], counts[v] / n))
        rest = int((assigned < 0).sum())
        f.write("-1\tunassigned\t%d\t%.6f\n" % (rest, rest / n))


def assign_reads_file(args):
    """`kmer_mapper assign-reads`: per read of a FASTA / FASTQ file, in file order, the node most of its k-mers map to
    (kmm_read_nodes) -> <out>.npy (int32, -1: unassigned), <out>.best_votes.npy, <out>.second_votes.npy, <out>.total_votes.npy
    (uint32), and with --summary a table of reads per node.  The file is read through the host reader in chunks, as
    `read-hits` without --device-parser reads it."""
    k = args.kmer_size
    world = int(os.environ.get("WORLD_SIZE", "1"))
    probe = probe_input(args.reads)
    check_assign_reads_input(probe.fmt, world, k, args.ambiguous_bases, args.min_votes, args.min_margin)
    lut = None
    if args.ambiguous_bases == "skip":
        from .util import ambiguous_skip_lut
        lut = ambiguous_skip_lut()
    names = read_node_names(args.names) if args.names else None            # (read before the index: a missing file fails here)
    kmer_index = _get_kmer_index_from_args(args)
    max_node_id = kmer_index.max_node_id() if hasattr(kmer_index, "max_node_id") else int(np.max(kmer_index._nodes))
    n_nodes = max_node_id + 1
    if names is not None:                                                   # (the node count comes from the index: before the GPU)
        check_node_names(args.names, names, n_nodes)
    revcomp = bool(args.map_reverse_complements)
    parts = [[], [], [], []]
    dev = DeviceIndex.from_index(kmer_index, max_node_id, device=args.device)
    try:
        for chunk in prefetch(read_chunks(args.reads, min_chunk_size=args.chunk_size)):
            L = chunk.uniform_length
            if L is not None:
                res = dev.read_nodes(chunk.bases, n_reads=len(chunk), read_len=L, k=k, max_index_lookup_frequency=args.max_hits_per_kmer,
                                     also_revcomp=revcomp, lut=lut)
            else:
                res = dev.read_nodes(chunk.bases, chunk.offsets, k=k, max_index_lookup_frequency=args.max_hits_per_kmer,
                                     also_revcomp=revcomp, lut=lut)
            for part, got in zip(parts, (res.best_node, res.best_votes, res.second_votes, res.total_votes)):
                part.append(got)
    finally:
        dev.close()
    cat = lambda part, dt: np.concatenate(part) if part else np.zeros(0, dt)
    best_node, best_votes, second_votes, total_votes = (cat(p, dt) for p, dt in zip(parts, (np.int32, np.uint32, np.uint32, np.uint32)))
    assigned = assign_rule(best_node, best_votes, second_votes, args.min_votes, args.min_margin)
    n_reads, n_assigned, n_none = assigned.shape[0], int((assigned >= 0).sum()), int((best_node < 0).sum())
    n_margin = int(((best_votes.astype(np.int64) >= max(args.min_votes, 1)) &
                    (best_votes.astype(np.int64) - second_votes < args.min_margin)).sum())
    logging.info("%d reads; %d (%.2f %%) assigned to a node, %d ambiguous (margin below %d), %d without a vote", n_reads, n_assigned,
                 100.0 * n_assigned / max(n_reads, 1), n_margin, args.min_margin, n_none)
    if args.output_file is not None:
        out = str(args.output_file)
        np.save(out, assigned)
        np.save(out + ".best_votes", best_votes)
        np.save(out + ".second_votes", second_votes)
        np.save(out + ".total_votes", total_votes)
        logging.info("Saved per-read nodes to %s.npy (votes: .best_votes.npy, .second_votes.npy, .total_votes.npy)" % out)
    if args.summary:
        write_assign_summary(args.summary, assigned, n_nodes, names)
        logging.info("Saved the per-node summary to %s" % args.summary)
    return assigned


class RecordKeepSink(RecordHitsSink):
    """The same hook for `select-reads`: open(dev) sets record-hits mode 2 and the keep rule, drain(dev) takes
    both queues after every map call — so both stay chunk-sized — and appends the kept records' bytes to `out`, a binary file
    object; seen / kept count the records.  bgzf: the kept text is deflated on the GPU and `out` (and out2) get
    BGZF members — every drain ends its last member; close() writes the end-of-file block; kept_bytes still counts text."""

    def __init__(self, out, min_hits=1, min_permille=0, invert=False, names=False, mate_suffix=False, pairs=False, pair_rule="any",
                 out2=None, bgzf=False, bam_pairs=False, bam_out=False, bam_mates=False, sam_out=False, sam_header=True,
                 min_base_quality=0, sam_mates=False):
        super().__init__(windows=True, min_base_quality=min_base_quality)
        self.out = out
        self.rule = dict(min_hits=int(min_hits), min_permille=int(min_permille), invert=bool(invert))
        self.seen = self.kept = self.kept_bytes = 0
        # BAM input: the decode carries QNAME and QUAL — four-line FASTQ — with "/1" / "/2" on request
        self.names, self.mate_suffix = bool(names), bool(mate_suffix)
        self.counters = {}
        # mates kept together: pairs: the stream is interleaved ("record_pairs"); out2: the file of the mate-2
        # texts of map_record_pairs, whose queue is drained with the other two
        self.pairs, self.pair_rule, self.out2 = bool(pairs), pair_rule, out2
        # the mates of a name-collated BAM file: the named decode's records are mates in file order
        self.bam_pairs = bool(bam_pairs)
        # BAM out: the kept records as they stand in the file ("record_bam"), always BGZF, behind the input's header —
        # written once, as members of its own, in front of the first take
        self.bam_out = bool(bam_out)
        # mates kept together in BAM out: the selected records are mates in file order ("record_bam_mates")
        self.bam_mates = bool(bam_mates) and self.bam_out
        # SAM out: the kept records' own lines ("record_sam"), behind the header lines unless sam_header is off
        self.sam_out, self.sam_header = bool(sam_out), bool(sam_header)
        # mates kept together in SAM out: the selected records are mates in file order ("record_sam_mates")
        self.sam_mates = bool(sam_mates) and self.sam_out
        self.header_written = False
        self.bgzf = bool(bgzf) or self.bam_out
        self.written = 0                     # bytes written to out and out2 (the members' with bgzf, else the text's)

    def open(self, dev):
        super().open(dev)
        dev.record_keep(True, **self.rule)
        if self.names:
            dev.record_names(True, mate_suffix=self.mate_suffix, **({"pairs": True} if self.bam_pairs else {}))
        if self.bam_mates:
            dev.record_bam(True, mates=True)
        elif self.bam_out:
            dev.record_bam(True)
        if self.sam_out:
            dev.record_sam(True, header=self.sam_header, **({"mates": True} if self.sam_mates else {}))
        if self.bam_pairs or self.bam_mates or self.sam_mates:
            dev.record_pairs(False, rule=self.pair_rule)
        if self.pairs or self.out2 is not None:
            dev.record_pairs(self.pairs, rule=self.pair_rule)

    def finish(self, dev):
        """The named decode's counters, read once behind the last map call (the drivers' before_fetch hook)."""
        if self.names:
            self.counters = {name: dev.get_param(name)
                             for name in ("records_reversed", "records_without_qual", "record_name_bytes_replaced")}

    def drain(self, dev):
        if dev.get_param("record_hits_pending"):
            got = dev.take_record_hits()
            self.hits.append(got[0])
            self.wins.append(got[1])
            self.seen += int(got[0].shape[0])
        if self.bam_out and not self.header_written:
            self._write_header(dev)
        n = self._take(dev, 0, self.out)
        if self.out2 is not None:
            n2 = self._take(dev, 1, self.out2)
            if n2 != n:
                raise RuntimeError("select-reads: %d mate-1 and %d mate-2 records kept by one call" % (n, n2))

    def _write_header(self, dev):
        """The input's header, verbatim, as BGZF members of its own — once the stream's first windows have brought all of it."""
        from .util import bgzf_compress
        try:
            header = dev.bam_header()
        except ValueError:                   # (the windows so far ended inside the header: no record was mapped either)
            return
        members = bgzf_compress(header, device=getattr(dev, "device", 0))
        self.out.write(memoryview(members))
        self.written += int(members.shape[0])
        self.header_written = True

    def _take(self, dev, mate, out):
        """One queue into its file; returns the records taken."""
        if self.bgzf:
            data, n_text, n = dev.take_kept_bgzf(mate)
        else:
            data, n = dev.take_kept_mates(mate)
            n_text = int(data.shape[0])
        if data.shape[0]:
            out.write(memoryview(data))
        self.written += int(data.shape[0])
        self.kept += int(n)
        self.kept_bytes += int(n_text)
        return n

    def close(self):
        """Behind the last drain: the block that ends a BGZF file."""
        if self.bam_out and not self.header_written:
            raise RuntimeError("select-reads --bam-out: the input's header was never read: nothing to write in front of the records")
        if self.bgzf:
            from .gz_io import BGZF_EOF
            for out in (self.out, self.out2):
                if out is not None:
                    out.write(BGZF_EOF)
                    self.written += len(BGZF_EOF)


_SELECT_READS_BAM_ONLY = (("--bam-to-fastq", "bam_to_fastq"), ("--exclude-flags", "exclude_flags"), ("--include-flags", "include_flags"),
                          ("--min-mapq", "min_mapq"), ("--regions", "regions"), ("--regions-file", "regions_file"),
                          ("--as-stored", "as_stored"), ("--mate-suffix", "mate_suffix"), ("--bam-out", "bam_out"))


def check_select_reads_input(fmt, world_size, reads, output, bam_to_fastq=False, bam_options=(), bam_out=False, sam_out=False):
    """`kmer_mapper select-reads` takes FASTA / FASTQ (plain or .gz) — and with --bam-to-fastq a BAM file, whose kept records
    come out as FASTQ, with --bam-out a BAM file whose kept records come out as BAM records — in one
    process and never writes over its input; everything else is refused before the index is read.  bam_options: the names of
    the options given that go with BAM input alone.  sam_out: --sam-out reads SAM text and writes the kept lines back."""
    if fmt == "bam" and not bam_to_fastq and not bam_out:
        raise ValueError("select-reads does not read %s files: their records are decoded on the GPU without the read's name, so "
                         "the selected text would be useless; SAM and BAM input is out of scope — unless --bam-to-fastq asks for "
                         "a BAM file's kept records as FASTQ, with their names and qualities (or --bam-out for the kept records "
                         "as a BAM file)" % fmt.upper())
    if fmt == "sam" and not sam_out:
        raise ValueError("select-reads does not read %s files: their records are decoded on the GPU without the read's name, so "
                         "the selected text would be useless; SAM and BAM input is out of scope (--bam-to-fastq reads BAM, not "
                         "SAM text: `samtools view -b` makes one of the other) — unless --sam-out asks for the kept records as "
                         "SAM lines, untouched" % fmt.upper())
    if bam_options and fmt != "bam":
        raise ValueError("%s applies to BAM input only (the reads are %s)" % (bam_options[0], fmt))
    if world_size > 1:
        raise ValueError("select-reads runs in one process: WORLD_SIZE=%d (torchrun) is out of scope, run it without torchrun"
                         % world_size)
    if os.path.abspath(str(output)) == os.path.abspath(str(reads)) or (os.path.exists(str(output)) and os.path.samefile(str(output), str(reads))):
        raise ValueError("select-reads: -o %s is the input file (-f): the output would overwrite the reads" % output)


def check_select_reads_bam_out(fmt, given):
    """--bam-out of `kmer_mapper select-reads`: a BAM file in, the kept records out as a BAM file, untouched and in
    file order.  given: the names of the other options given that change the form of the output or pair the reads — none goes
    with it.  Refused before the index is read and before -o is created."""
    if fmt != "bam":
        raise ValueError("--bam-out applies to BAM input only (the reads are %s): BAM records are written from BAM records" % fmt)
    for opt in given:
        why = {"--bam-to-fastq": "the kept records leave as FASTQ text or as BAM records, not both",
               "--as-stored": "the records are written as they stand in the file in any case; the strand matters to the hits alone, "
                              "which are counted in read orientation",
               "--mate-suffix": "the names are not rewritten"}.get(opt, "mates are not kept together in BAM output, which has one "
                                                                        "input file (-f) and one output file (-o)")
        raise ValueError("select-reads: --bam-out does not go with %s: %s" % (opt, why))


_SELECT_READS_NOT_WITH_SAM_OUT = (("--bam-to-fastq", "bam_to_fastq"), ("--bam-out", "bam_out"), ("--as-stored", "as_stored"),
                                  ("--mate-suffix", "mate_suffix"), ("--bam-pairs", "bam_pairs"), ("--keep-mates", "keep_mates"),
                                  ("--interleaved", "interleaved"), ("-f2/--reads2", "reads2"), ("-o2/--output2", "output2"))


def check_select_reads_sam_out(fmt, sam_out, no_header=False, given=()):
    """--sam-out of `kmer_mapper select-reads`: SAM text in (plain, BGZF or gzip), the kept records out as SAM
    lines, untouched and in file order, behind the header lines (--no-header: without them).  given: the names of the other
    options given that change the form of the output or pair the reads — none goes with it.  Refused before the index is read
    and before -o is created."""
    if no_header and not sam_out:
        raise ValueError("select-reads: --no-header goes with --sam-out: it leaves the header lines out of SAM output")
    if not sam_out:
        return
    if fmt != "sam":
        raise ValueError("--sam-out applies to SAM input only (the reads are %s): SAM lines are written from SAM lines%s"
                         % (fmt, "; a BAM file has --bam-out" if fmt == "bam" else ""))
    for opt in given:
        why = {"--bam-to-fastq": "it reads BAM, and the kept records leave as SAM lines, not as FASTQ",
               "--bam-out": "BAM records are written from BAM records: `samtools view -b` makes a BAM file of the output",
               "--as-stored": "the lines are written as they stand in the file in any case; the strand matters to the hits alone, "
                              "which are counted in read orientation",
               "--mate-suffix": "the names are not rewritten"}.get(opt, "mates are not kept together in SAM output, which has one "
                                                                        "input file (-f) and one output file (-o)")
        raise ValueError("select-reads: --sam-out does not go with %s: %s" % (opt, why))


def check_select_reads_sam_mates(sam_mates, sam_out):
    """--sam-mates of `kmer_mapper select-reads`: with --sam-out, the mates of SAM text grouped by name — an
    aligner's own output — are kept or dropped together and leave as SAM lines.  Without --sam-out it is refused before the index
    is read and before -o is created."""
    if sam_mates and not sam_out:
        raise ValueError("select-reads: --sam-mates goes with --sam-out: the kept mates are written as SAM lines; a BAM file's mates "
                         "have --bam-out --keep-mates, and interleaved FASTQ / FASTA input has --interleaved")


def check_select_reads_keep_mates(keep_mates, bam_out):
    """--keep-mates of `kmer_mapper select-reads`: with --bam-out, the mates of a name-collated BAM file are kept or
    dropped together and leave as BAM records.  Without --bam-out it is refused before the index is read."""
    if keep_mates and not bam_out:
        raise ValueError("select-reads: --keep-mates goes with --bam-out: the kept mates are written as BAM records; for FASTQ output "
                         "a BAM file's mates have --bam-to-fastq --bam-pairs, and interleaved FASTQ / FASTA input has --interleaved")


def check_select_reads_bam_pairs(fmt, bam_to_fastq=False, interleaved=False, reads2=None, output2=None):
    """--bam-pairs of `kmer_mapper select-reads`: a name-collated BAM file whose mates are kept together.  What
    does not go with it is refused before the index is read and before -o is created."""
    if fmt != "bam":
        raise ValueError("--bam-pairs applies to BAM input only (the reads are %s; interleaved FASTQ has --interleaved)" % fmt)
    if not bam_to_fastq:
        raise ValueError("select-reads: --bam-pairs goes with --bam-to-fastq: the kept mates are written as interleaved FASTQ")
    for given, opt in ((interleaved, "--interleaved"), (reads2 is not None, "-f2/--reads2"), (output2 is not None, "-o2/--output2")):
        if given:
            raise ValueError("select-reads: --bam-pairs does not go with %s: the mates lie in one BAM file (-f) and leave as one "
                             "interleaved FASTQ file (-o)" % opt)


def _same_file(a, b):
    a, b = str(a), str(b)
    return os.path.abspath(a) == os.path.abspath(b) or (os.path.exists(a) and os.path.exists(b) and os.path.samefile(a, b))


def check_select_reads_pairs(probe, reads, output, interleaved=False, reads2=None, output2=None, pair_rule=None):
    """The pair forms of `kmer_mapper select-reads`: --interleaved (-f holds mates in turn) or -f2 with -o2 (two
    files in, two out), FASTQ or two-line FASTA, plain or .gz.  What does not go together is refused before the index is read.
    Returns the probe of -f2 (None without it)."""
    if interleaved and reads2 is not None:
        raise ValueError("select-reads: --interleaved says that -f holds both mates; it does not go with -f2/--reads2")
    if reads2 is not None and output2 is None:
        raise ValueError("select-reads: -f2/--reads2 needs -o2/--output2, the file of the kept mate-2 reads")
    if output2 is not None and reads2 is None:
        raise ValueError("select-reads: -o2/--output2 goes with -f2/--reads2")
    if pair_rule is not None and not interleaved and reads2 is None:
        raise ValueError("select-reads: --pair-rule goes with --interleaved or -f2/--reads2")
    if not interleaved and reads2 is None:
        return None

    def pairable(p, path):
        if p.fmt in ("sam", "bam") or (p.fmt == "fasta" and not p.two_line):
            raise ValueError("select-reads: mates are kept together in FASTQ and two-line FASTA files; %s is %s, which is out of scope "
                             "for --interleaved and -f2 (a BAM file's mates: `samtools fastq` first)"
                             % (path, "multi-line FASTA" if p.fmt == "fasta" else p.fmt.upper()))

    pairable(probe, reads)
    probe2 = None
    if reads2 is not None:
        probe2 = probe_input(reads2)
        pairable(probe2, reads2)
        if probe2.fmt != probe.fmt:
            raise ValueError("select-reads: -f %s is %s and -f2 %s is %s: the two inputs differ in format" % (reads, probe.fmt, reads2, probe2.fmt))
    inputs = [("-f", reads)] + ([("-f2", reads2)] if reads2 is not None else [])
    outputs = [("-o", output)] + ([("-o2", output2)] if output2 is not None else [])
    for o_opt, o in outputs:
        for i_opt, i in inputs:
            if _same_file(o, i):
                raise ValueError("select-reads: %s %s is the input file (%s): the output would overwrite the reads" % (o_opt, o, i_opt))
    if output2 is not None and _same_file(output, output2):
        raise ValueError("select-reads: -o and -o2 name the same file %s" % output)
    if reads2 is not None and _same_file(reads, reads2):
        raise ValueError("select-reads: -f and -f2 name the same file %s" % reads)
    return probe2


def _records_left(chunker, period):
    """The whole records a chunker still holds or can read (the error path at the end of paired input)."""
    n_lines = 0
    while True:
        buf = chunker.next_chunk()
        if buf is None:
            break
        n_lines += int(np.count_nonzero(buf == 10))
        chunker.consumed(buf.shape[0])
    return n_lines // period


def select_read_pairs_files(index, reads1, reads2, chunk_size, fmt, k, sink, map_reverse_complements=False,
                            max_index_lookup_frequency=1000, device=0, lut=None):
    """Two files in step: record i of reads1 and record i of reads2 are mates.  Both files are read by the host
    readers (RawChunker: plain text as it lies, .gz inflated by gz_io.open_gz), the unconsumed tail of each is carried into its
    next chunk, every pair of chunks goes through DeviceIndex.map_record_pairs and the sink drains the three queues after every
    call.  Returns the number of pairs; files of different record counts are an error that names both counts."""
    period = {"fastq": 4, "fasta": 2}[fmt]
    kfmt = {"fastq": _lib.FORMAT_FASTQ, "fasta": _lib.FORMAT_FASTA2}[fmt]
    max_node_id = index.max_node_id() if hasattr(index, "max_node_id") else int(np.max(index._nodes))
    dev = DeviceIndex.from_index(index, max_node_id, device=device)
    chunkers = []
    n_pairs = 0
    try:
        sink.open(dev)
        chunkers = [RawChunker(path, int(chunk_size), pinned=True) for path in (reads1, reads2)]
        while True:
            bufs = [c.next_chunk() for c in chunkers]
            if bufs[0] is None or bufs[1] is None:
                break
            used1, used2, m = dev.map_record_pairs(bufs[0], bufs[1], fmt=kfmt, k=k, max_index_lookup_frequency=max_index_lookup_frequency,
                                                   also_revcomp=map_reverse_complements, lut=lut)
            sink.drain(dev)
            if m == 0:
                if all(c.eof for c in chunkers):
                    break
                for c in chunkers:                   # a record longer than the chunk: read more
                    if not c.eof:
                        c.chunk_size *= 2
                continue
            n_pairs += m
            chunkers[0].consumed(used1)
            chunkers[1].consumed(used2)
        left = [_records_left(c, period) for c in chunkers]
        if left[0] or left[1]:
            raise ValueError("select-reads: %s holds %d records and %s holds %d: the files are not mates of each other (%d pairs were "
                             "written)" % (reads1, n_pairs + left[0], reads2, n_pairs + left[1], n_pairs))
    finally:
        for c in chunkers:
            c.close()
        dev.close()
    return n_pairs


def select_reads_file(args):
    """`kmer_mapper select-reads`: the reads of a FASTA / FASTQ file that pass the keep rule, written to -o as uncompressed
    text — with --bgzf as a BGZF file, deflated on the GPU — in file order.  The file goes down the route `map` would choose for it in one process (choose_route: raw records,
    BGZF, gzip — parsed and inflated on the GPU) with the handle's record-hits mode 2 and record-keep mode on; both queues are
    taken after every map call.  Wrapped FASTA comes out unwrapped (two-line).
    --interleaved / -f2 with -o2: paired-end reads, whose mates are kept or dropped together."""
    k = args.kmer_size
    world = int(os.environ.get("WORLD_SIZE", "1"))
    probe = probe_input(args.reads)
    interleaved, reads2, output2 = bool(getattr(args, "interleaved", False)), getattr(args, "reads2", None), getattr(args, "output2", None)
    pair_rule = getattr(args, "pair_rule", None)
    bam_pairs = bool(getattr(args, "bam_pairs", False))
    bam_out = bool(getattr(args, "bam_out", False))
    keep_mates = bool(getattr(args, "keep_mates", False))
    sam_out = bool(getattr(args, "sam_out", False))
    sam_mates = bool(getattr(args, "sam_mates", False))
    check_select_reads_sam_mates(sam_mates, sam_out)
    check_select_reads_sam_out(probe.fmt, sam_out, bool(getattr(args, "no_header", False)),
                               [opt for opt, name in _SELECT_READS_NOT_WITH_SAM_OUT if getattr(args, name, None)])
    check_select_reads_keep_mates(keep_mates, bam_out)
    if bam_out:
        check_select_reads_bam_out(probe.fmt, [opt for opt, name in (("--bam-to-fastq", "bam_to_fastq"), ("--as-stored", "as_stored"),
                                                                     ("--mate-suffix", "mate_suffix"), ("--bam-pairs", "bam_pairs"),
                                                                     ("--interleaved", "interleaved"), ("-f2/--reads2", "reads2"),
                                                                     ("-o2/--output2", "output2")) if getattr(args, name, None)])
    if bam_pairs:
        check_select_reads_bam_pairs(probe.fmt, bool(getattr(args, "bam_to_fastq", False)), interleaved, reads2, output2)
    check_select_reads_pairs(probe, args.reads, args.output_file, interleaved, reads2, output2,
                             None if bam_pairs or keep_mates or sam_mates else pair_rule)
    # (with --sam-out the options that select records apply to SAM too; those that change the output's form were refused above)
    bam_options = [opt for opt, name in _SELECT_READS_BAM_ONLY if getattr(args, name, None) and not sam_out]
    check_select_reads_input(probe.fmt, world, args.reads, args.output_file, bool(getattr(args, "bam_to_fastq", False)), bam_options,
                             bam_out, sam_out)
    # (the floor of the record-hits mode, DESIGN 4.27, under the checks of `map`, before the index is read: k >= 2, BAM with
    # --use-record-qual, FASTA warned about and served; SAM lines kept as SAM lines are mapped without their QUAL column)
    if sam_out and int(getattr(args, "min_base_quality", 0) or 0):
        raise ValueError("select-reads: --sam-out does not go with --min-base-quality: SAM lines kept as SAM lines are mapped without "
                         "their QUAL column (a BAM file has --bam-to-fastq and --bam-out with --use-record-qual)")
    use_qual = check_use_record_qual(bool(getattr(args, "use_record_qual", False)), probe.fmt, getattr(args, "min_base_quality", 0))
    min_q = check_min_base_quality(getattr(args, "min_base_quality", 0), k, probe.fmt, use_record_qual=use_qual)
    more_floor = dict(min_base_quality=min_q, use_record_qual=use_qual) if min_q else {}
    if not 0 <= args.min_hit_permille <= 1000:
        raise ValueError("--min-hit-permille outside [0, 1000]")
    if args.min_hits < 0:
        raise ValueError("--min-hits negative")
    fmt = probe.fmt
    bam = fmt == "bam"
    more = {}
    if sam_out:
        # (the route `read-hits --device-parser` takes for SAM — plain, BGZF or gzip — with the hits counted in read orientation,
        # as --bam-out counts them; the lines leave as they stand)
        opt = lambda name, default=None: getattr(args, name, default)
        select = check_record_select(fmt, include_flags=opt("include_flags", 0), min_mapq=opt("min_mapq", 0), regions=opt("regions"),
                                     regions_file=opt("regions_file"))
        exclude_flags = int(opt("exclude_flags", 0) or 0)
        if sam_mates:
            # (a secondary or supplementary line between two mates would be taken for one of them: DESIGN 4.28)
            logging.info("select-reads --sam-mates: secondary and supplementary records are excluded (--exclude-flags 0x%x | 0x900 "
                         "= 0x%x)", exclude_flags, exclude_flags | 0x900)
            exclude_flags |= 0x900
        more = dict(exclude_flags=exclude_flags, original_strand=check_original_strand(True, fmt),
                    **({"record_select": select} if select else {}))
    if bam:
        # (the route `read-hits --device-parser` takes for BAM, with the names on; reverse-strand records in read orientation
        # unless --as-stored: a FASTQ of reverse-complemented reads is not what anyone wants from a BAM file)
        opt = lambda name, default=None: getattr(args, name, default)
        select = check_record_select(fmt, include_flags=opt("include_flags", 0), min_mapq=opt("min_mapq", 0), regions=opt("regions"),
                                     regions_file=opt("regions_file"))
        exclude_flags = int(opt("exclude_flags", 0) or 0)
        if bam_pairs:
            # (a secondary or supplementary record between two mates would be taken for one of them: DESIGN 4.23)
            logging.info("select-reads --bam-pairs: secondary and supplementary records are excluded (--exclude-flags 0x%x | 0x900 "
                         "= 0x%x)", exclude_flags, exclude_flags | 0x900)
            exclude_flags |= 0x900
        if keep_mates:
            logging.info("select-reads --keep-mates: secondary and supplementary records are excluded (--exclude-flags 0x%x | 0x900 "
                         "= 0x%x)", exclude_flags, exclude_flags | 0x900)
            exclude_flags |= 0x900
        _check_bam_route(fmt, 1, exclude_flags)
        more = dict(exclude_flags=exclude_flags, original_strand=check_original_strand(not opt("as_stored", False), fmt),
                    **({"record_select": select} if select else {}))
    lut = None
    if args.ambiguous_bases == "skip":
        from .util import ambiguous_skip_lut
        lut = ambiguous_skip_lut()
        if k < 2:
            raise ValueError("--ambiguous-bases skip needs -k 2 or more")
    kmer_index = _get_kmer_index_from_args(args)
    if fmt == "fasta" and not probe.two_line:
        fmt = "fasta_ml"
    logging.info("select-reads: records parsed on the GPU, record-hits and record-keep modes%s%s",
                 "; the kept BAM records written as they stand, behind the input's header (--bam-out)" if bam_out else
                 "; the kept SAM lines written as they stand, %s the header lines (--sam-out)"
                 % ("without" if getattr(args, "no_header", False) else "behind") if sam_out else
                 "; BAM records decoded to FASTQ with their names (--bam-to-fastq)" if bam else "",
                 "; neighbouring records are mates, kept together, pair rule '%s' (--bam-pairs)" % (pair_rule or "any") if bam_pairs else
                 "; neighbouring selected records are mates, kept together, pair rule '%s' (--sam-mates)" % (pair_rule or "any")
                 if sam_mates else "")
    rule = dict(min_hits=args.min_hits, min_permille=args.min_hit_permille, invert=args.invert,
                bgzf=bool(getattr(args, "bgzf", False)))
    if reads2 is not None:
        logging.info("select-reads: -f and -f2 are read in step by the host readers (two compressed streams are not inflated on the "
                     "GPU in step); mates are kept together, pair rule '%s'", pair_rule or "any")
        with open(args.output_file, "wb") as out, open(output2, "wb") as out2:
            sink = RecordKeepSink(out, pair_rule=pair_rule or "any", out2=out2, min_base_quality=min_q, **rule)
            select_read_pairs_files(kmer_index, args.reads, reads2, args.chunk_size, fmt, k, sink, bool(args.map_reverse_complements),
                                    args.max_hits_per_kmer, device=args.device, lut=lut)
            sink.close()
    else:
        with open(args.output_file, "wb") as out:
            sink = RecordKeepSink(out, names=bam and not bam_out, mate_suffix=bam and bool(getattr(args, "mate_suffix", False)),
                                  pairs=interleaved, pair_rule=pair_rule or "any", bam_pairs=bam_pairs, bam_out=bam_out,
                                  **({"bam_mates": True} if keep_mates else {}),
                                  **({"sam_out": True, "sam_header": not getattr(args, "no_header", False)} if sam_out else {}),
                                  **({"sam_mates": True} if sam_mates else {}), **rule)
            try:
                map_gpu_raw(kmer_index, args.reads, args.chunk_size, fmt, k, bool(args.map_reverse_complements), args.max_hits_per_kmer,
                            device=args.device, n_threads=16, probe=probe, lut=lut, record_hits=sink, before_fetch=sink.finish, **more,
                            **more_floor)
            except ValueError as exc:
                if keep_mates and ("are not mates" in str(exc) or "unpaired record" in str(exc)):
                    # (a BAM file that stops in the middle looks like one that does not — -o is removed)
                    out.close()
                    os.remove(args.output_file)
                    raise ValueError("select-reads --bam-out --keep-mates: %s (%s was removed)" % (exc, args.output_file)) from exc
                if sam_mates and ("are not mates" in str(exc) or "unpaired record" in str(exc)):
                    # (a SAM file that stops in the middle looks like one that does not — -o is removed)
                    out.close()
                    os.remove(args.output_file)
                    raise ValueError("select-reads --sam-out --sam-mates: %s (%s was removed)" % (exc, args.output_file)) from exc
                if not interleaved or not ("unpaired record" in str(exc) or "do not form a complete record" in str(exc)):
                    raise
                # (the error path alone: the file's lines counted once more on the host, to name both sides)
                counter = RawChunker(args.reads, 1 << 22)
                try:
                    n_whole = _records_left(counter, {"fastq": 4, "fasta": 2}[fmt])
                finally:
                    counter.close()
                raise ValueError("select-reads --interleaved: %s does not end with a whole pair: it holds %d whole records, %d mate-1 "
                                 "and %d mate-2%s (%s)" % (args.reads, n_whole, (n_whole + 1) // 2, n_whole // 2, "" if n_whole % 2 else
                                                           ", and an incomplete record behind them", exc)) from exc
            sink.close()
    hits, wins = sink.result()
    logging.info("%d reads seen, %d (%.2f %%) kept: %d bytes %s %s%s", sink.seen, sink.kept,
                 100.0 * sink.kept / max(sink.seen, 1), sink.kept_bytes,
                 "written as %d bytes of BGZF to" % sink.written if sink.bgzf else "written to", args.output_file,
                 "".join("; %s %d" % (name, v) for name, v in sink.counters.items() if v))
    if args.hits_output is not None:
        np.save(args.hits_output, hits)
        np.save(str(args.hits_output) + ".windows", wins)
        logging.info("Saved per-read hits to %s.npy and windows to %s.windows.npy", args.hits_output, args.hits_output)
    return sink.seen, sink.kept


def check_index_args(kmer_size, modulo, ambiguous_bases):
    """The refusals of `kmer_mapper index` that need neither the file nor a device."""
    if not 1 <= kmer_size <= 31:
        raise ValueError("index: -k %d outside [1, 31]" % kmer_size)
    if modulo != 0 and not 2 <= modulo <= 2 ** 31 - 1:
        raise ValueError("index: --modulo %d outside [2, 2^31 - 1] (0, the default: the smallest prime >= 2 entries + 1)" % modulo)
    if ambiguous_bases == "skip" and kmer_size < 2:
        raise ValueError("--ambiguous-bases skip needs -k 2 or more")


def index_file(args):
    """`kmer_mapper index`: a Kmer Index (.npz) from the sequences of a FASTA file, built on the GPU: what
    `map`, `read-hits` and `select-reads` take with -i.  Node i is the i-th sequence (--single-node: all are node 0)."""
    from . import mapper
    check_index_args(args.kmer_size, args.modulo, args.ambiguous_bases)
    t0 = time.perf_counter()
    index, names, info = mapper.index_from_fasta(args.fasta, k=args.kmer_size, both_strands=args.both_strands,
                                                 single_node=args.single_node, modulo=args.modulo,
                                                 ambiguous_bases=args.ambiguous_bases, device=args.device)
    skipped = info["n_full_windows"] - info["n_windows"]
    logging.info("index: %d sequences, %d bases, %d windows of %d bases (%d skipped at ambiguous bases: %.3f %%), %d pairs%s, "
                 "%d entries, modulo %d, %.2f s", info["n_seqs"], info["n_bases"], info["n_windows"], args.kmer_size, skipped,
                 100.0 * skipped / max(info["n_full_windows"], 1), info["n_pairs"], " (both strands)" if args.both_strands else "",
                 info["n_entries"], info["modulo"], time.perf_counter() - t0)
    if info["n_entries"] == 0:
        raise ValueError("index: %s gives an index without entries (no sequence holds a window of %d bases clear of ambiguous "
                         "bases): lower -k or check the file" % (args.fasta, args.kmer_size))
    index.to_file(args.output_file)
    if args.names_output:
        with open(args.names_output, "w") as f:
            for name in names:
                f.write(name + "\n")
        logging.info("index: %d names written to %s (line i names node i%s)", len(names), args.names_output,
                     "; with --single-node every sequence is node 0" if args.single_node else "")
    logging.info("index: written to %s", args.output_file if str(args.output_file).endswith(".npz") else str(args.output_file) + ".npz")
    return index


def build_argument_parser():
    parser = argparse.ArgumentParser(
        description='Kmer Mapper',
        prog='kmer_mapper',
        formatter_class=lambda prog: argparse.HelpFormatter(prog, max_help_position=50, width=100))

    subparsers = parser.add_subparsers()
    subparser = subparsers.add_parser("map", help="Map reads to a kmer index")
    subparser.add_argument("-i", "--kmer-index", required=False)
    subparser.add_argument("-b", "--index-bundle", required=False)
    subparser.add_argument("-f", "--reads", required=True, help="Reads in .fa, .fq, .fa.gz, fq.gz, SAM (.sam, .sam.gz) or BAM format")
    subparser.add_argument("-k", "--kmer-size", required=False, default=31, type=int)
    subparser.add_argument("-t", "--n-threads", required=False, default=16, type=int,
                           help="Host threads that read / inflate the reads and pack them to 2 bits per base before they "
                                "cross PCIe (1: none, the raw bytes cross). Default 16.")
    subparser.add_argument("-c", "--chunk-size", required=False, type=int, default=2500000,
                           help="N bytes to process in each chunk")
    subparser.add_argument("-o", "--output-file", required=True)
    subparser.add_argument("-d", "--debug", required=False, help="Set to True to print debug log")
    subparser.add_argument("-I", "--max-hits-per-kmer", required=False, default=1000, type=int,
                           help="Ignore kmers that have more than this amount of hits in index")
    subparser.add_argument("-g", "--gpu", default=False, type=bool,
                           help="Accepted for compatibility: this build always maps on the GPU.")
    subparser.add_argument("-s", "--gpu-hash-map-size", default=0, type=int,
                           help="Accepted for compatibility; the index's own modulo is used.")
    subparser.add_argument("-r", "--map-reverse-complements", default=False, type=bool,
                           help="Also count kmers in reverse complement of reads. "
                                "Default False. Not necessary if index contains reverse complements.")
    subparser.add_argument("--apply-max-hits-per-kmer", action="store_true",
                           help="Extension: actually apply -I (the reference parses it but always uses 1000).")
    subparser.add_argument("--host-parser", action="store_true",
                           help="Extension: parse records on the host instead of on the GPU (kmm_map_records; wrapped FASTA is "
                                "unwrapped on the GPU too).")
    subparser.add_argument("--device", default=0, type=int, help="Extension: GPU ordinal (single process).")
    subparser.add_argument("--exclude-flags", default=0, type=lambda v: int(v, 0),
                           help="Extension, SAM and BAM input only: leave out records whose FLAG has any of these bits (samtools view -F; "
                                "e.g. 0x900 = secondary and supplementary alignments). Default 0: every record, as the reference.")
    subparser.add_argument("--include-flags", default=0, type=lambda v: int(v, 0),
                           help="Extension, SAM and BAM input only: map only records whose FLAG has all of these bits (samtools view "
                                "-f; e.g. 0x2 = proper pairs, 4 = unmapped reads). Default 0: every record.")
    subparser.add_argument("--min-mapq", default=0, type=int, metavar="Q",
                           help="Extension, SAM and BAM input only: map only records with MAPQ >= Q (samtools view -q; 0 .. 255). "
                                "Default 0: MAPQ is not read.")
    subparser.add_argument("--regions", action="append", default=None, metavar="REGIONS",
                           help="Extension, SAM and BAM input only: map only records that overlap one of these regions, decided on "
                                "the GPU from RNAME / POS / CIGAR. Comma-separated, repeatable, samtools syntax: chr6:28,000,000-"
                                "34,000,000 (1-based, inclusive), chr6:5, chr6, '*' = also the records without a reference ('*' "
                                "alone is refused: it adds to a list; --include-flags 4 gives the unmapped records). In one "
                                "string a comma in front of exactly three digits is a thousands separator: chr1:5,100 is "
                                "chr1:5100, and a reference named by three digits needs a --regions of its own.")
    subparser.add_argument("--regions-file", default=None, metavar="BED",
                           help="Extension, SAM and BAM input only: regions from a BED file (three columns, 0-based half-open; "
                                "'#', 'track' and 'browser' lines are skipped); adds to --regions.")
    subparser.add_argument("--ambiguous-bases", choices=("a", "skip"), default="a",
                           help="a (default): N is counted as A and any other letter is an error, as the reference. skip "
                                "(extension): no k-mer that contains N or an IUPAC ambiguity letter is counted; the k-mers on "
                                "either side of it are.")
    subparser.add_argument("--min-base-quality", default=0, type=int, metavar="Q",
                           help="Extension, FASTQ input (SAM / BAM with --use-record-qual): a base whose Phred+33 quality is below Q (0 .. 93) is skipped like an "
                                "ambiguous base under --ambiguous-bases skip: no k-mer that contains it is counted. Default 0: "
                                "qualities are not read.")
    subparser.add_argument("--use-record-qual", action="store_true",
                           help="Extension, SAM and BAM input only, with --min-base-quality: decode every record's QUAL on the GPU "
                                "and apply the floor to it. Records that store no qualities (QUAL '*', 0xFF in BAM) pass unmasked "
                                "and are counted in the log. Without it, --min-base-quality is refused on SAM and BAM.")
    subparser.add_argument("--original-strand", action="store_true",
                           help="Extension, SAM and BAM input only: map every record whose FLAG has 0x10 (stored reverse-complemented "
                                "by the aligner) in read orientation, SEQ flipped back and QUAL reversed on the GPU, as `samtools "
                                "fastq` writes it; with --exclude-flags 0x900 the counts are those of the FASTQ the file was made "
                                "from. Default: SEQ as stored, as the reference.")
    subparser.add_argument("--shard-bam", action="store_true",
                           help="Extension, BAM input under torchrun (WORLD_SIZE > 1): every rank maps its own member range of the "
                                "file, trimmed at both ends to record starts that the ranks find on the GPU; a boundary guessed "
                                "wrongly is an error, never a wrong count. Default: several ranks on one BAM file are refused.")
    subparser.set_defaults(func=map_bnp)

    sub = subparsers.add_parser("read-hits", help="Extension: per read, the number of its k-mers that are in a kmer index")
    sub.add_argument("-i", "--kmer-index", required=False)
    sub.add_argument("-b", "--index-bundle", required=False)
    sub.add_argument("-f", "--reads", required=True, help="Reads in .fa, .fq, .fa.gz or .fq.gz format (SAM, .sam.gz and BAM with --device-parser only)")
    sub.add_argument("-k", "--kmer-size", required=False, default=31, type=int)
    sub.add_argument("-c", "--chunk-size", required=False, type=int, default=2500000, help="N bytes to process in each chunk")
    sub.add_argument("-o", "--output-file", required=True,
                     help="<out>.npy: uint32, one value per read in file order; with --windows also <out>.windows.npy")
    sub.add_argument("-I", "--max-hits-per-kmer", required=False, default=1000, type=int,
                     help="A k-mer whose index entries all have a frequency above this is no hit. Applied as given.")
    sub.add_argument("-r", "--map-reverse-complements", default=False, type=bool,
                     help="A window also hits when the reverse complement of its k-mer is in the index. Default False.")
    sub.add_argument("--ambiguous-bases", choices=("a", "skip"), default="a",
                     help="a (default): N is looked up as A and any other letter is an error. skip: no window that contains N "
                          "or an IUPAC ambiguity letter is looked up (it is not counted in --windows either).")
    sub.add_argument("--windows", action="store_true", help="Also write the number of windows looked up per read.")
    sub.add_argument("--min-hits", default=1, type=int, metavar="N",
                     help="The log reports how many reads have at least N hits. Default 1.")
    sub.add_argument("--device", default=0, type=int, help="GPU ordinal.")
    sub.add_argument("-d", "--debug", required=False, help="Set to True to print debug log")
    sub.add_argument("--device-parser", action="store_true",
                     help="Parse the records on the GPU, on the route `map` takes for the file (.gz inflated there), with the "
                          "library's record-hits mode. Also reads SAM (.sam, .sam.gz) and BAM.")
    sub.add_argument("--exclude-flags", default=0, type=lambda v: int(v, 0),
                     help="With --device-parser, SAM and BAM input only: leave out records whose FLAG has any of these bits.")
    sub.add_argument("--include-flags", default=0, type=lambda v: int(v, 0),
                     help="With --device-parser, SAM and BAM input only: only records whose FLAG has all of these bits "
                          "(4 = unmapped reads).")
    sub.add_argument("--min-mapq", default=0, type=int, metavar="Q",
                     help="With --device-parser, SAM and BAM input only: only records with MAPQ >= Q.")
    sub.add_argument("--regions", action="append", default=None, metavar="REGIONS",
                     help="With --device-parser, SAM and BAM input only: only records that overlap one of these regions "
                          "(syntax as `map --regions`).")
    sub.add_argument("--regions-file", default=None, metavar="BED",
                     help="With --device-parser, SAM and BAM input only: regions from a BED file; adds to --regions.")
    sub.add_argument("--original-strand", action="store_true",
                     help="With --device-parser, SAM and BAM input only: records whose FLAG has 0x10 are looked up in read "
                          "orientation.")
    sub.add_argument("--min-base-quality", default=argparse.SUPPRESS, type=int, metavar="Q",
                     help="FASTQ input (SAM / BAM with --use-record-qual): a base whose Phred+33 quality is below Q (0 .. 93) is a "
                          "break: no k-mer over it is looked up, and it counts in neither hits nor windows. Implies --device-parser. "
                          "FASTA has no qualities (a warning). Needs -k 2 or more. Default 0: off.")
    sub.add_argument("--use-record-qual", action="store_true", default=argparse.SUPPRESS,
                     help="SAM and BAM input only, with --min-base-quality: decode every record's QUAL on the GPU and apply the "
                          "floor to it. Records that store no qualities pass unmasked and are counted in the log.")
    sub.set_defaults(func=read_hits_file)

    sub = subparsers.add_parser("assign-reads", help="Extension: per read, the node (sequence) that most of its k-mers map to")
    sub.add_argument("-i", "--kmer-index", required=False)
    sub.add_argument("-b", "--index-bundle", required=False)
    sub.add_argument("-f", "--reads", required=True, help="Reads in .fa, .fq, .fa.gz or .fq.gz format")
    sub.add_argument("-k", "--kmer-size", required=False, default=31, type=int)
    sub.add_argument("-c", "--chunk-size", required=False, type=int, default=2500000, help="N bytes to process in each chunk")
    sub.add_argument("-o", "--output-file", required=True,
                     help="<out>.npy: int32, one node id per read in file order, -1: unassigned; also <out>.best_votes.npy, "
                          "<out>.second_votes.npy and <out>.total_votes.npy (uint32)")
    sub.add_argument("-I", "--max-hits-per-kmer", required=False, default=1000, type=int,
                     help="An index entry with a frequency above this gives no vote. Applied as given.")
    sub.add_argument("-r", "--map-reverse-complements", default=False, type=bool,
                     help="The reverse complement of every k-mer votes too, as `map -r True` counts it. Default False.")
    sub.add_argument("--ambiguous-bases", choices=("a", "skip"), default="a",
                     help="a (default): N is looked up as A and any other letter is an error. skip: no window that contains N "
                          "or an IUPAC ambiguity letter votes.")
    sub.add_argument("--min-votes", default=1, type=int, metavar="N",
                     help="A read whose best node has fewer than N votes is unassigned (-1). Default 1.")
    sub.add_argument("--min-margin", default=0, type=int, metavar="M",
                     help="A read whose best node leads the runner-up by fewer than M votes is unassigned (-1). Default 0: a tie "
                          "goes to the smallest node id.")
    sub.add_argument("--names", default=None, metavar="FILE",
                     help="Node names for --summary, line i names node i: the file `kmer_mapper index --names-output` wrote.")
    sub.add_argument("--summary", default=None, metavar="TSV",
                     help="Write one line per node and one for the unassigned reads: node id, name, reads assigned, share.")
    sub.add_argument("--device", default=0, type=int, help="GPU ordinal.")
    sub.add_argument("-d", "--debug", required=False, help="Set to True to print debug log")
    sub.set_defaults(func=assign_reads_file)

    sub = subparsers.add_parser("select-reads", help="Extension: write the reads whose k-mers hit a kmer index back out")
    sub.add_argument("-i", "--kmer-index", required=False)
    sub.add_argument("-b", "--index-bundle", required=False)
    sub.add_argument("-f", "--reads", required=True, help="Reads in .fa, .fq, .fa.gz or .fq.gz format (BAM with --bam-to-fastq or --bam-out, SAM text with --sam-out)")
    sub.add_argument("-k", "--kmer-size", required=False, default=31, type=int)
    sub.add_argument("-c", "--chunk-size", required=False, type=int, default=2500000, help="N bytes to process in each chunk")
    sub.add_argument("-o", "--output-file", required=True,
                     help="The kept reads as uncompressed text, in file order, every record as it stands in the (inflated) input; "
                          "wrapped FASTA comes out unwrapped")
    sub.add_argument("--min-hits", default=1, type=int, metavar="N", help="Keep a read with at least N k-mers in the index. Default 1.")
    sub.add_argument("--min-hit-permille", default=0, type=int, metavar="P",
                     help="... and with at least P per mille of its windows in the index (0 .. 1000). Default 0.")
    sub.add_argument("--invert", action="store_true", help="Keep the reads the rule does not match instead (depletion).")
    sub.add_argument("-I", "--max-hits-per-kmer", required=False, default=1000, type=int,
                     help="A k-mer whose index entries all have a frequency above this is no hit. Applied as given.")
    sub.add_argument("-r", "--map-reverse-complements", default=False, type=bool,
                     help="A window also hits when the reverse complement of its k-mer is in the index. Default False.")
    sub.add_argument("--ambiguous-bases", choices=("a", "skip"), default="a",
                     help="a (default): N is looked up as A and any other letter is an error. skip: no window that contains N "
                          "or an IUPAC ambiguity letter is looked up.")
    sub.add_argument("--hits-output", default=None, metavar="OUT",
                     help="Also write the per-read hits of ALL reads to <OUT>.npy and their windows to <OUT>.windows.npy.")
    # (the BAM options are absent from the namespace unless given: a call without them parses as it did before they existed)
    sub.add_argument("--bam-to-fastq", action="store_true", default=argparse.SUPPRESS,
                     help="Read a BAM file: its records are inflated, selected and decoded on the GPU, and the kept ones are "
                          "written as four-line FASTQ with their names and qualities (absent qualities as '\"'; name bytes outside "
                          "'!' .. '~' as '?'). Records with FLAG 0x10 come out in read orientation.")
    sub.add_argument("--exclude-flags", default=argparse.SUPPRESS, type=lambda v: int(v, 0),
                     help="BAM input only: leave out records whose FLAG has any of these bits (0x900: secondary and supplementary).")
    sub.add_argument("--include-flags", default=argparse.SUPPRESS, type=lambda v: int(v, 0),
                     help="BAM input only: only records whose FLAG has all of these bits (4 = unmapped reads).")
    sub.add_argument("--min-mapq", default=argparse.SUPPRESS, type=int, metavar="Q", help="BAM input only: only records with MAPQ >= Q.")
    sub.add_argument("--regions", action="append", default=argparse.SUPPRESS, metavar="REGIONS",
                     help="BAM input only: only records that overlap one of these regions (syntax as `map --regions`).")
    sub.add_argument("--regions-file", default=argparse.SUPPRESS, metavar="BED",
                     help="BAM input only: regions from a BED file; adds to --regions.")
    sub.add_argument("--as-stored", action="store_true", default=argparse.SUPPRESS,
                     help="BAM input only: write records with FLAG 0x10 as the file stores them (reverse-complemented), not in read "
                          "orientation.")
    sub.add_argument("--mate-suffix", action="store_true", default=argparse.SUPPRESS,
                     help="BAM input only: /1 behind the name of a first mate (FLAG 0x40 and not 0x80), /2 behind a second "
                          "(0x80 and not 0x40), as `samtools fastq` without -n.")
    # (the pair options too)
    sub.add_argument("--interleaved", action="store_true", default=argparse.SUPPRESS,
                     help="Paired-end reads in one file: -f holds mates in turn (records 2i and 2i + 1), FASTQ or two-line FASTA, "
                          "plain or .gz (inflated on the GPU as for `map`). Both mates of a pair are kept or both dropped.")
    sub.add_argument("-f2", "--reads2", default=argparse.SUPPRESS, metavar="FILE",
                     help="Paired-end reads in two files: record i of -f and record i of FILE are mates (by position; names are "
                          "not compared). Needs -o2. Both files are read, and .gz inflated, by the host readers: two compressed "
                          "streams are not inflated on the GPU in step.")
    sub.add_argument("-o2", "--output2", default=argparse.SUPPRESS, metavar="FILE",
                     help="The kept mate-2 reads (of -f2); -o then holds the kept mate-1 reads, record for record in step.")
    sub.add_argument("--pair-rule", choices=("any", "both"), default=argparse.SUPPRESS,
                     help="With --interleaved or -f2: a pair matches when any of its mates passes --min-hits / --min-hit-permille "
                          "(default), or only when both do; --invert then flips the pair's outcome.")
    sub.add_argument("--bam-pairs", action="store_true", default=argparse.SUPPRESS,
                     help="With --bam-to-fastq: the BAM file is grouped by name (as it leaves the sequencer or an aligner, or after "
                          "`samtools collate`): neighbouring records are mates, both kept or both dropped (--pair-rule), and -o is "
                          "interleaved FASTQ. Secondary and supplementary records (0x900) are excluded; the names of every pair are "
                          "compared on the GPU, and neighbours that are no mates (a coordinate-sorted file) or a last record without "
                          "its mate are an error.")
    sub.add_argument("--bam-out", action="store_true", default=argparse.SUPPRESS,
                     help="Read a BAM file and write the kept records back out as a BAM file: every kept record as it stands in the "
                          "input (RNAME, POS, MAPQ, CIGAR, mate fields and aux tags included), in file order, behind the input's header "
                          "(verbatim: no @PG line; no index is written). -o is always BGZF, deflated on the GPU. Takes --min-hits, "
                          "--min-hit-permille, --invert, --hits-output and the BAM selection options; the hits of records with FLAG "
                          "0x10 are counted in read orientation. Does not go with --bam-to-fastq, --as-stored, --mate-suffix, "
                          "--bam-pairs, --interleaved or -f2 / -o2.")
    sub.add_argument("--keep-mates", action="store_true", default=argparse.SUPPRESS,
                     help="With --bam-out: the BAM file is grouped by name (unaligned BAM, an aligner's unsorted output, or after "
                          "`samtools collate`): neighbouring selected records are mates, both kept or both dropped (--pair-rule), "
                          "and both leave as BAM records, mate 1 directly in front of mate 2. Secondary and supplementary records "
                          "(0x900) are excluded; the read names of every pair are compared on the GPU, and neighbours that are no "
                          "mates (a coordinate-sorted file) or a last record without its mate are an error, after which -o is removed "
                          "(--hits-output is written behind a complete run alone: such an error leaves none).")
    sub.add_argument("--sam-out", action="store_true", default=argparse.SUPPRESS,
                     help="Read SAM text (plain, BGZF or gzip; inflated and parsed on the GPU) and write the kept records back out as "
                          "SAM lines: every kept record's whole line as it stands in the input (RNAME, POS, CIGAR and every tag "
                          "included), in file order, behind the header lines (verbatim: no @PG line). Plain text, or BGZF with "
                          "--bgzf (htslib reads it as .sam.gz). Takes --min-hits, --min-hit-permille, --invert, --hits-output, "
                          "--exclude-flags, --include-flags, --min-mapq, --regions and --regions-file; the hits of records with "
                          "FLAG 0x10 are counted in read orientation. Does not go with --bam-to-fastq, --bam-out, --as-stored, "
                          "--mate-suffix, --bam-pairs, --keep-mates, --interleaved or -f2 / -o2.")
    sub.add_argument("--sam-mates", action="store_true", default=argparse.SUPPRESS,
                     help="With --sam-out: the SAM text is grouped by name (as bwa mem, minimap2 -a and bowtie2 write it): "
                          "neighbouring selected records are mates, and both lines are kept or both dropped (--pair-rule), mate 1 "
                          "directly in front of mate 2. Secondary and supplementary records (0x900) are excluded; the QNAME bytes "
                          "of every pair are compared on the GPU as they stand. Neighbours that are not mates (a coordinate-sorted "
                          "file) or a last record without its mate are an error, after which -o is removed and no --hits-output "
                          "is written.")
    sub.add_argument("--no-header", action="store_true", default=argparse.SUPPRESS,
                     help="With --sam-out: leave the header lines out (`samtools view` without -h), for shares that are concatenated.")
    sub.add_argument("--bgzf", action="store_true", default=argparse.SUPPRESS,
                     help="Write -o (and -o2) as BGZF files: the kept text is deflated on the GPU, one member per 65280 bytes, and "
                          "only the members are copied to the host. Without it the output is plain text, whatever -o is called.")
    sub.add_argument("--min-base-quality", default=argparse.SUPPRESS, type=int, metavar="Q",
                     help="FASTQ input (BAM with --use-record-qual): a base whose Phred+33 quality is below Q (0 .. 93) is a break "
                          "for the keep rule: no k-mer over it is looked up, and it counts in neither hits nor windows. The reads "
                          "are written as they stand. FASTA has no qualities (a warning). Needs -k 2 or more; does not go with "
                          "--sam-out. Default 0: off.")
    sub.add_argument("--use-record-qual", action="store_true", default=argparse.SUPPRESS,
                     help="BAM input only, with --min-base-quality: apply the floor to every record's QUAL, decoded on the GPU. "
                          "Records that store no qualities pass unmasked and are counted in the log.")
    sub.add_argument("--device", default=0, type=int, help="GPU ordinal.")
    sub.add_argument("-d", "--debug", required=False, help="Set to True to print debug log")
    sub.set_defaults(func=select_reads_file)

    sub = subparsers.add_parser("index", help="Extension: build a kmer index from the sequences of a FASTA file, on the GPU")
    sub.add_argument("-f", "--fasta", required=True, help="Sequences in FASTA format (.fa, .fa.gz; wrapped lines are fine). The "
                     "file is read whole; FASTQ, SAM and BAM are refused.")
    sub.add_argument("-k", "--kmer-size", required=False, default=31, type=int)
    sub.add_argument("-o", "--output-file", required=True, help="The kmer index (.npz) that map, read-hits and select-reads take with -i")
    sub.add_argument("--both-strands", action="store_true",
                     help="Also enter the reverse complement of every k-mer, under the same node: reads of either strand hit "
                          "without -r.")
    sub.add_argument("--single-node", action="store_true",
                     help="Every sequence is node 0 (default: sequence i is node i): the smallest index, for select-reads.")
    sub.add_argument("--modulo", default=0, type=int,
                     help="The index's hash modulo, 2 .. 2^31 - 1. Default 0: the smallest prime >= 2 x entries + 1.")
    sub.add_argument("--ambiguous-bases", choices=("skip", "a"), default="skip",
                     help="skip (the default HERE): no k-mer over N or an IUPAC ambiguity letter enters the index, so an N run of "
                          "a reference does not become a poly-A entry. a: N is A and every other letter is an error. Note that "
                          "`map`, `read-hits` and `select-reads` default the other way (a), for the reference's sake.")
    sub.add_argument("--names-output", required=False, help="Write the sequence names here, one per line: line i names node i.")
    sub.add_argument("--device", default=0, type=int, help="GPU ordinal.")
    sub.add_argument("-d", "--debug", required=False, help="Set to True to print debug log")
    sub.set_defaults(func=index_file)
    return parser


def run_argument_parser(args):
    logging.basicConfig(stream=sys.stdout, level=logging.INFO,
                        format='%(asctime)s %(levelname)s: %(message)s')
    parser = build_argument_parser()

    if len(args) == 0:
        parser.print_help()
        sys.exit(1)

    args = parser.parse_args(args)
    if getattr(args, "min_base_quality", 0):     # (refused here: before the index file is read)
        try:
            check_min_base_quality(args.min_base_quality, args.kmer_size)
        except ValueError as exc:
            parser.error(str(exc))
    return args.func(args)


if __name__ == "__main__":
    main()
