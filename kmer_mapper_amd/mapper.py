"""Drop-in for kmer_mapper/mapper.pyx — same names, arguments, return dtypes and shapes,
executed by the HIP kernels behind include/kmm.h (never on the CPU).

  map_kmers_to_graph_index(index, max_node_id, kmers, max_index_lookup_frequency=1000)
      -> np.uint32[max_node_id+1]                       mapper.pyx:19-72
  in_graph_index(index, kmers, max_index_lookup_frequency=1000) -> np.uint8[len(kmers)]
                                                        mapper.pyx:81-130
  in_graph_index_no_memory_maps(...)                    mapper.pyx:137-190 (same result)

`index` is duck-typed exactly like the reference: only _hashes_to_index, _n_kmers, _nodes, _kmers,
_frequencies, _modulo are read (mapper.pyx:22-29); wrong dtypes raise ValueError like Cython's
typed memoryviews do.  The HBM copy of an index is cached per index object so that repeated
calls (one per chunk in map_cpu, command_line_interface.py:51) do not re-upload it.
"""
import numpy as np

from .engine import DeviceIndex

_CACHE = {}      # key -> (DeviceIndex, strong refs to the arrays so ids stay valid)
_CACHE_MAX = 4


def _device_index(index, max_node_id, device=0):
    arrays = (index._hashes_to_index, index._n_kmers, index._nodes, index._kmers,
              index._frequencies)
    key = (tuple(id(a) for a in arrays), int(index._modulo), int(max_node_id), int(device))
    hit = _CACHE.get(key)
    if hit is not None:
        return hit[0]
    dev = DeviceIndex(index._hashes_to_index, index._n_kmers, index._modulo, index._kmers,
                      index._nodes, index._frequencies, max_node_id, device=device)
    while len(_CACHE) >= _CACHE_MAX:
        _, (old, _) = _CACHE.popitem()
        old.close()
    _CACHE[key] = (dev, arrays)
    return dev


def clear_cache():
    while _CACHE:
        _, (old, _) = _CACHE.popitem()
        old.close()


def _check_kmers(kmers):
    kmers = np.asarray(kmers) if not hasattr(kmers, "data_ptr") else kmers
    if isinstance(kmers, np.ndarray):
        if kmers.dtype != np.uint64:
            raise ValueError("Buffer dtype mismatch, expected 'uint64_t' but got '%s'" % kmers.dtype)
        if kmers.ndim != 1:
            raise ValueError("Buffer has wrong number of dimensions (expected 1, got %d)" % kmers.ndim)
        if not kmers.flags.c_contiguous:
            raise ValueError("ndarray is not C-contiguous")
    return kmers


class NodeCountAccumulator:
    """The SUM of many map_kmers_to_graph_index calls without the per-call traffic.  The reference's callers add the
    per-chunk vectors up (command_line_interface.py:51,124-130: one `np.zeros(max_node_id + 1)` per chunk, mapper.pyx:37,
    summed by the pool); reproduced call for call that is a reset, a map and a copy of 4 (max_node_id + 1) bytes to the host
    PER CHUNK — 400 MB at the 100 M index for a 2.5 MB chunk.  An accumulator keeps ONE count vector in HBM:

        with NodeCountAccumulator(index, max_node_id) as acc:
            for kmers in chunks:
                map_kmers_to_graph_index(index, max_node_id, kmers, accumulate_into=acc)     # returns None: nothing moves
            counts = acc.node_counts()                                                       # fetched once

    Bit-identical to summing the per-call results (uint32 additions wrap like the reference's, mapper.pyx:37,68)."""

    def __init__(self, index, max_node_id, device=0):
        self._dev = _device_index(index, max_node_id, device)
        self._dev.reset()

    def map_kmers(self, kmers, max_index_lookup_frequency=1000):
        self._dev.map_kmers(_check_kmers(kmers), max_index_lookup_frequency)

    def node_counts(self):
        return self._dev.get_node_counts()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def map_kmers_to_graph_index(index, max_node_id, kmers, max_index_lookup_frequency=1000, accumulate_into=None):
    """mapper.pyx:19-72.  accumulate_into (extension): a NodeCountAccumulator of the same index — the call adds to its
    vector in HBM and returns None instead of a fresh host array."""
    kmers = _check_kmers(kmers)
    dev = _device_index(index, max_node_id)
    if accumulate_into is not None:
        if accumulate_into._dev is not dev:
            raise ValueError("accumulate_into belongs to another index / max_node_id")
        dev.map_kmers(kmers, max_index_lookup_frequency)
        return None
    dev.reset()                      # mapper.pyx:37 — a fresh zeroed vector per call
    dev.map_kmers(kmers, max_index_lookup_frequency)
    return dev.get_node_counts()


def in_graph_index(index, kmers, max_index_lookup_frequency=1000):
    kmers = _check_kmers(kmers)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    return _device_index(index, max_node_id).in_index(kmers)


in_graph_index_no_memory_maps = in_graph_index


def read_hits(index, reads, k=31, max_index_lookup_frequency=1000, also_revcomp=False, lut=None, windows=False, device=0):
    """Extension (no counterpart in mapper.pyx, whose in_graph_index answers per k-mer): per read, how many of its k-mers
    are in the index -> np.uint32[n_reads]; windows=True: (hits, windows looked up).  `reads`: what util.as_read_batch
    takes (a ReadBatch, a (bases, offsets) pair or a list of reads).  DeviceIndex.read_hits on the cached handle."""
    from .util import as_read_batch
    batch = as_read_batch(reads)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    return _device_index(index, max_node_id, device).read_hits(batch.bases, batch.offsets, k=k,
                                                               max_index_lookup_frequency=max_index_lookup_frequency,
                                                               also_revcomp=also_revcomp, lut=lut, windows=windows)


def read_nodes(index, reads, k=31, max_index_lookup_frequency=1000, also_revcomp=False, lut=None, table_bytes=0, device=0):
    """Extension: per read, the node that most of its k-mers map to -> engine.ReadNodes (best_node, best_votes, second_votes,
    total_votes, n_nodes, n_rounds; DeviceIndex.read_nodes).  `reads`: what util.as_read_batch takes.  Opens a handle for the
    call and closes it: nothing of the index stays on the device."""
    from .util import as_read_batch
    batch = as_read_batch(reads)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    with DeviceIndex.from_index(index, max_node_id, device=device) as dev:
        return dev.read_nodes(batch.bases, batch.offsets, k=k, max_index_lookup_frequency=max_index_lookup_frequency,
                              also_revcomp=also_revcomp, lut=lut, table_bytes=table_bytes)


def _floor_on(dev, windows, min_base_quality, use_record_qual):
    """The record-hits mode with its floor on a cached handle; returns what _floor_off puts back."""
    before = dev.get_param("use_record_qual")
    dev.record_hits(True, windows=windows, min_base_quality=min_base_quality)
    if min_base_quality:
        dev.set_param("use_record_qual", int(bool(use_record_qual)))
    return before


def _floor_off(dev, before):
    dev.record_hits(False)
    dev.set_param("use_record_qual", before)


def record_hits(index, raw, fmt="fastq", k=31, max_index_lookup_frequency=1000, also_revcomp=False, lut=None, windows=False, device=0,
                min_base_quality=0, use_record_qual=False):
    """Extension: read_hits for reads that are still records — `raw` is a chunk of FASTQ (fmt "fastq"), two-line FASTA ("fasta")
    or SAM ("sam") text (bytes, a uint8 array or a torch tensor, host or device), parsed on the GPU with the cached handle's
    record-hits mode (DeviceIndex.record_hits / take_record_hits).  Returns (hits, consumed) — with windows=True
    (hits, windows, consumed): one entry per whole record of the chunk, in order; raw[consumed:] is the incomplete last record,
    to be put in front of the next chunk.  The handle's node counts do not move, and the mode is off again afterwards.
    min_base_quality: a base whose quality byte is below '!' + Q is a break — no window over it is looked up, and it counts in
    neither hits nor windows; FASTA has no qualities and is served unchanged; SAM needs use_record_qual=True (its
    QUAL column is decoded on the GPU; a QUAL of "*" passes unmasked)."""
    from . import _lib
    kfmt = {"fastq": _lib.FORMAT_FASTQ, "fasta": _lib.FORMAT_FASTA2, "sam": _lib.FORMAT_SAM}[fmt]
    if isinstance(raw, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    dev = _device_index(index, max_node_id, device)
    if dev.get_param("record_hits_pending"):
        raise ValueError("the cached handle has record hits pending: take them first (DeviceIndex.take_record_hits)")
    before = _floor_on(dev, windows, min_base_quality, use_record_qual)
    try:
        consumed, _ = dev.map_records(raw, fmt=kfmt, k=k, max_index_lookup_frequency=max_index_lookup_frequency,
                                      also_revcomp=also_revcomp, lut=lut)
        got = dev.take_record_hits()
    finally:
        _floor_off(dev, before)
    return (got[0], got[1], consumed) if windows else (got, consumed)


def select_records(index, raw, fmt="fastq", k=31, max_index_lookup_frequency=1000, also_revcomp=False, lut=None, min_hits=1,
                   min_permille=0, invert=False, device=0, exclude_flags=0, original_strand=False, mate_suffix=False, compress=False, pairs=False,
                   pair_rule="any", output="fastq", keep_mates=False, header=True, min_base_quality=0, use_record_qual=False,
                   sam_mates=False):
    """Extension: record_hits that also hands back the reads it selects — `raw` as in record_hits (fmt "fastq" or "fasta"; SAM
    text does not carry the read's name through the device-side decode and is refused).  A record is kept iff
    (hits >= min_hits and 1000 * hits >= min_permille * windows) != invert.  Returns (text, hits, windows): the kept records'
    bytes as the parser saw them, in order and contiguous, and one entry per whole record of the chunk, kept or not
    (DeviceIndex.record_keep / take_kept_records).  The mode is off again afterwards.
    fmt "bam": `raw` is a WHOLE BAM file held as bytes; its records — those whose FLAG has none of exclude_flags — are decoded on
    the GPU into four-line FASTQ that carries QNAME and QUAL (DeviceIndex.record_names), and the text returned is
    that FASTQ.  original_strand: records with FLAG 0x10 in read orientation; mate_suffix: "/1" / "/2" behind the names.
    compress: the text comes back as a BGZF file's bytes — deflated on the GPU (DeviceIndex.take_kept_bgzf), the
    end-of-file block appended.
    pairs (fmt "bam"): the file is name-collated — its selected records are mates in file order, 2p and 2p + 1 — and
    mates are kept or dropped together: a pair matches when pair_rule "any" mate does, or only when "both" do.  The text is
    interleaved FASTQ, the entries lie in pair order.  Neighbours whose names differ, or an unpaired last record, raise
    ValueError with the library's hint (collate by name; exclude secondary and supplementary records, 0x900).
    output "bam" (fmt "bam"): the kept records come back AS BAM RECORDS, untouched — RNAME, POS, MAPQ, CIGAR, mate
    fields and aux tags included — and the text returned is the bytes of a complete BAM file: the input's header, verbatim, as BGZF
    members of its own, the kept records' members (deflated on the GPU), the end-of-file block.  original_strand then applies
    to the hits alone; mate_suffix, pairs and compress do not go with it.
    keep_mates (output "bam"): the file is name-collated and mates are kept or dropped together under pair_rule, as
    with `pairs`, but as BAM records: both records of every kept pair, untouched, mate 1 directly in front of mate 2.  The mate
    check compares the read_name bytes as they stand; strangers or an unpaired last record raise ValueError with the hint.
    output "sam" (fmt "sam"): `raw` is SAM text and the text returned is SAM text — every kept record's whole line,
    untouched, in file order, behind (header=True) every header line at its place; header=False drops the header lines.
    Records whose FLAG has any of exclude_flags are not written; original_strand applies to the hits alone; compress: a complete
    BGZF file (htslib reads it as .sam.gz).  The bytes behind the last newline are not looked at (len(text) tells with
    min_hits=0).  mate_suffix, pairs and keep_mates do not go with it.
    sam_mates (output "sam"): the text is grouped by name, as aligners write it — its selected records are mates in
    file order — and both lines of a pair are kept or dropped together under pair_rule, mate 1 directly in front of mate 2; the
    entries lie in pair order.  Neighbours whose QNAME bytes differ, or an unpaired last record, raise ValueError with the
    library's hint (group by name; exclude secondary and supplementary records, 0x900).
    min_base_quality: the floor of record_hits — it changes which records pass the rule, never the text that comes
    back; fmt "bam" needs use_record_qual=True (records that store no qualities pass unmasked); output "sam" does not go with it."""
    from . import _lib
    if sam_mates and output != "sam":
        raise ValueError("sam_mates goes with output=\"sam\": mates kept together as SAM lines (BAM out: keep_mates=True)")
    if output == "sam" and min_base_quality:
        raise ValueError("output=\"sam\" does not go with min_base_quality: SAM lines kept as SAM lines are mapped without their QUAL "
                         "column")
    if output == "sam":
        if fmt != "sam":
            raise ValueError("output=\"sam\" goes with fmt=\"sam\": SAM lines are written from SAM lines")
        if mate_suffix or pairs or keep_mates:
            raise ValueError("output=\"sam\" does not go with mate_suffix, pairs or keep_mates: the lines are written as they stand, in "
                             "file order")
        if pair_rule not in ("any", "both"):
            raise ValueError("pair_rule must be 'any' or 'both', not %r" % (pair_rule,))
        return _select_sam_lines(index, raw, k, max_index_lookup_frequency, also_revcomp, lut, min_hits, min_permille, invert, device,
                                 exclude_flags, original_strand, compress, header, sam_mates, pair_rule)
    if keep_mates and output != "bam":
        raise ValueError("keep_mates goes with output=\"bam\": mates kept together as BAM records (FASTQ out: pairs=True)")
    if output not in ("fastq", "bam"):
        raise ValueError("output must be 'fastq', 'bam' or 'sam', not %r" % (output,))
    if output == "bam" and fmt != "bam":
        raise ValueError("output=\"bam\" goes with fmt=\"bam\": BAM records are written from BAM records")
    if output == "bam" and (mate_suffix or pairs or compress):
        raise ValueError("output=\"bam\" does not go with mate_suffix, pairs or compress: the records are written as they stand, in "
                         "file order, and a BAM file is always BGZF")
    if fmt != "bam" and (exclude_flags or original_strand or mate_suffix):
        raise ValueError("exclude_flags, original_strand and mate_suffix go with fmt=\"bam\"")
    if pairs and fmt != "bam":
        raise ValueError("pairs goes with fmt=\"bam\" (interleaved FASTQ / FASTA text: select_record_pairs)")
    if pair_rule not in ("any", "both"):
        raise ValueError("pair_rule must be 'any' or 'both', not %r" % (pair_rule,))
    kfmt = {"fastq": _lib.FORMAT_FASTQ, "fasta": _lib.FORMAT_FASTA2, "sam": _lib.FORMAT_SAM, "bam": 0}[fmt]
    if isinstance(raw, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    dev = _device_index(index, max_node_id, device)
    if dev.get_param("record_hits_pending") or dev.get_param("record_keep_pending_bytes"):
        raise ValueError("the cached handle has record hits or kept records pending: take them first")
    before_qual = _floor_on(dev, True, min_base_quality, use_record_qual)
    dev.record_keep(True, min_hits=min_hits, min_permille=min_permille, invert=invert)
    before = None
    try:
        if fmt == "bam":
            before = (dev.get_param("bam_exclude_flags"), dev.get_param("original_strand"), dev.get_param("record_pairs_rule"))
            dev.set_param("bam_exclude_flags", int(exclude_flags))
            dev.set_param("original_strand", int(bool(original_strand)))
            if pairs or keep_mates:
                dev.set_param("record_pairs_rule", dev.PAIR_RULES[pair_rule])
            if output == "bam":
                dev.record_bam(True, mates=keep_mates)
            else:
                dev.record_names(True, mate_suffix=mate_suffix, pairs=pairs)
            dev.map_bam(raw, first=True, last=True, k=k, max_index_lookup_frequency=max_index_lookup_frequency,
                        also_revcomp=also_revcomp, lut=lut)
        else:
            dev.map_records(raw, fmt=kfmt, k=k, max_index_lookup_frequency=max_index_lookup_frequency, also_revcomp=also_revcomp, lut=lut)
        hits, windows = dev.take_record_hits()
        if output == "bam":
            from .gz_io import BGZF_EOF
            from .util import bgzf_compress
            text = bgzf_compress(dev.bam_header(), device=device).tobytes() + dev.take_kept_bgzf()[0].tobytes() + BGZF_EOF
        elif compress:
            from .gz_io import BGZF_EOF
            text = dev.take_kept_bgzf()[0].tobytes() + BGZF_EOF
        else:
            text = dev.take_kept_records()[0].tobytes()
    finally:
        if before is not None:                                                      # (the handle is cached: as it was found)
            if output == "bam":
                if dev.get_param("record_keep_pending_bytes"):                      # (a take that failed: raw records never meet text)
                    dev.take_kept_records()
                if keep_mates and dev.get_param("record_hits_pending"):             # (a take that failed: the switch stays with its entries)
                    dev.take_record_hits()
                dev.record_bam(False)
            elif pairs and dev.get_param("record_hits_pending"):                    # (a take that failed: the switch stays with its entries)
                dev.set_param("record_names", 0)
            else:
                dev.record_names(False)
            dev.set_param("bam_exclude_flags", before[0])
            dev.set_param("original_strand", before[1])
            dev.set_param("record_pairs_rule", before[2])
        dev.record_keep(False)
        _floor_off(dev, before_qual)
    return text, hits, windows


def _select_sam_lines(index, raw, k, max_index_lookup_frequency, also_revcomp, lut, min_hits, min_permille, invert, device, exclude_flags,
                      original_strand, compress, header, mates=False, pair_rule="any"):
    """select_records(fmt="sam", output="sam"): DeviceIndex.record_sam around one map_records call; the cached handle is left as it
    was found.  mates: the pair form — `raw` is the whole stream, an unpaired last record fails the call."""
    from . import _lib
    if isinstance(raw, (bytes, bytearray, memoryview)):
        raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    dev = _device_index(index, max_node_id, device)
    if dev.get_param("record_hits_pending") or dev.get_param("record_keep_pending_bytes"):
        raise ValueError("the cached handle has record hits or kept records pending: take them first")
    before = (dev.get_param("bam_exclude_flags"), dev.get_param("original_strand"), dev.get_param("record_pairs_rule"))
    dev.record_hits(True, windows=True)
    dev.record_keep(True, min_hits=min_hits, min_permille=min_permille, invert=invert)
    dev.record_sam(True, header=header, mates=mates)
    try:
        dev.set_param("bam_exclude_flags", int(exclude_flags))
        dev.set_param("original_strand", int(bool(original_strand)))
        if mates:
            dev.set_param("record_pairs_rule", dev.PAIR_RULES[pair_rule])
        dev.map_records(raw, fmt=_lib.FORMAT_SAM | (_lib.FORMAT_LAST_CHUNK if mates else 0), k=k, max_index_lookup_frequency=max_index_lookup_frequency, also_revcomp=also_revcomp,
                        lut=lut)
        hits, windows = dev.take_record_hits()
        if compress:
            from .gz_io import BGZF_EOF
            text = dev.take_kept_bgzf()[0].tobytes() + BGZF_EOF
        else:
            text = dev.take_kept_records()[0].tobytes()
    finally:
        if dev.get_param("record_keep_pending_bytes"):                              # (a take that failed: raw lines never meet text)
            dev.take_kept_records()
        if mates and dev.get_param("record_hits_pending"):                          # (a take that failed: the switch stays with its entries)
            dev.take_record_hits()
        dev.record_sam(False)
        dev.set_param("bam_exclude_flags", before[0])
        dev.set_param("original_strand", before[1])
        dev.set_param("record_pairs_rule", before[2])
        dev.record_keep(False)
        dev.record_hits(False)
    return text, hits, windows


def select_record_pairs(index, raw1, raw2=None, fmt="fastq", k=31, max_index_lookup_frequency=1000, also_revcomp=False, lut=None,
                        min_hits=1, min_permille=0, invert=False, pair_rule="any", device=0, compress=False, min_base_quality=0,
                        use_record_qual=False):
    """Extension: select_records for paired-end reads, whose mates are kept or dropped together.  raw2 None: `raw1`
    holds the mates interleaved, records 2i and 2i + 1; else record i of raw1 and record i of raw2 are mates (fmt "fastq" or
    "fasta", two-line, the same for both; each of bytes, a uint8 array or a torch tensor, host or device).  Per mate, match is
    hits >= min_hits and 1000 * hits >= min_permille * windows; a pair matches when pair_rule "any" mate does, or only when
    "both" do, and is kept iff match != invert.  Returns (text1, text2, hits, windows): the kept records of raw1 and of raw2 in
    order — text2 None for interleaved input, whose kept pairs are text1 — and one entry per record of every whole pair, in pair
    order (mate 1, mate 2).  Records behind the last whole pair are not looked at.  The cached handle is left as it was found.
    compress: text1, and text2 where there is one, are the bytes of BGZF files — deflated on the GPU.
    min_base_quality: the floor of record_hits, on both mates; use_record_qual is taken for symmetry with
    select_records: FASTQ and FASTA text never need it."""
    from . import _lib
    kfmt = {"fastq": _lib.FORMAT_FASTQ, "fasta": _lib.FORMAT_FASTA2}[fmt]
    as_array = lambda raw: np.frombuffer(bytes(raw), dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else raw
    raw1, raw2 = as_array(raw1), None if raw2 is None else as_array(raw2)
    max_node_id = int(np.max(index._nodes)) if len(index._nodes) else 0
    dev = _device_index(index, max_node_id, device)
    if (dev.get_param("record_hits_pending") or dev.get_param("record_keep_pending_bytes")
            or dev.get_param("record_keep_pending_bytes_mate2")):
        raise ValueError("the cached handle has record hits or kept records pending: take them first")
    before = (dev.get_param("record_pairs"), dev.get_param("record_pairs_rule"))
    before_qual = _floor_on(dev, True, min_base_quality, use_record_qual)
    dev.record_keep(True, min_hits=min_hits, min_permille=min_permille, invert=invert)
    try:
        dev.record_pairs(raw2 is None, rule=pair_rule)
        common = dict(fmt=kfmt, k=k, max_index_lookup_frequency=max_index_lookup_frequency, also_revcomp=also_revcomp, lut=lut)
        text2 = None
        if raw2 is None:
            dev.map_records(raw1, **common)
        else:
            dev.map_record_pairs(raw1, raw2, **common)
        hits, windows = dev.take_record_hits()
        if compress:
            from .gz_io import BGZF_EOF
            take = lambda mate: dev.take_kept_bgzf(mate)[0].tobytes() + BGZF_EOF
        else:
            take = lambda mate: dev.take_kept_mates(mate)[0].tobytes()
        text1 = take(0)
        if raw2 is not None:
            text2 = take(1)
    finally:
        dev.record_keep(False)
        _floor_off(dev, before_qual)
        dev.set_param("record_pairs_rule", before[1])
        if not dev.get_param("record_hits_pending"):                                   # (a failing call appended nothing)
            dev.set_param("record_pairs", before[0])
    return text1, text2, hits, windows


def index_from_fasta(path, k=31, both_strands=False, single_node=False, modulo=0, ambiguous_bases="skip", device=0):
    """A Kmer Index from the sequences of a FASTA file (plain or .gz, wrapped or not): the file is read whole by the host reader,
    the index is built on the GPU (engine.index_from_sequences).  Node i is the i-th sequence; single_node: every
    sequence is node 0.  ambiguous_bases "skip" (the default HERE, unlike `map`): no k-mer over N or an IUPAC letter — an N run
    of a reference must not become a poly-A entry; "a": the reference's table, N counted as A.
    Returns (KmerIndex, names, info): names[i] names node i; info holds n_seqs, n_bases, n_windows, n_pairs, n_entries, modulo
    and n_full_windows (the windows there would be without breaks)."""
    from . import reads_io
    from .kmer_index import KmerIndex
    from .util import ambiguous_skip_lut
    if ambiguous_bases not in ("skip", "a"):
        raise ValueError("ambiguous_bases must be 'skip' or 'a'")
    k = int(k)
    lut = ambiguous_skip_lut() if ambiguous_bases == "skip" else None
    if lut is not None and k < 2:
        raise ValueError("--ambiguous-bases skip needs -k 2 or more")
    probe = reads_io.probe_input(path)
    if probe.fmt != "fasta":
        raise ValueError("index: %s holds %s records, an index is built from FASTA sequences (convert it, e.g. "
                         "`samtools fasta` / `seqtk seq -A`, or pass the reference the reads were aligned to)"
                         % (path, probe.fmt.upper()))
    with reads_io._open(path) as f:
        parts = []
        while True:
            piece = f.read(1 << 26)
            if not piece:
                break
            parts.append(bytes(piece))
    buf = np.frombuffer(b"".join(parts), dtype=np.uint8)
    batch, names = reads_io.parse_fasta_named(buf)
    offsets = np.ascontiguousarray(batch.offsets, dtype=np.int64)
    n_seqs = offsets.shape[0] - 1
    full = int(np.maximum(np.diff(offsets) - k + 1, 0).sum())
    from . import _lib
    # (without breaks every window is a pair: refused before the file's bytes cross to the device; with breaks the library counts)
    if full * (2 if both_strands else 1) > _lib.SEQIDX_MAX_PAIRS and lut is None:
        raise ValueError("index: %s holds %d windows of %d bases%s, one build takes at most %d (k-mer, node) pairs: split the "
                         "FASTA file and build one index per part" % (path, full, k, ", twice that on both strands" if both_strands
                                                                      else "", _lib.SEQIDX_MAX_PAIRS))
    nodes = np.zeros(n_seqs, dtype=np.int32) if single_node else None
    info = {}
    try:
        index = KmerIndex.from_sequences_gpu(np.ascontiguousarray(batch.bases), offsets, k=k, nodes=nodes, lut=lut,
                                             both_strands=both_strands, modulo=modulo, device=device, info=info)
    except ValueError as exc:
        if "KMM_SEQIDX_MAX_PAIRS" in str(exc):
            raise ValueError("index: %s is above the limit of one build (%s): split the FASTA file and build one index per part"
                             % (path, exc)) from None
        raise
    info.update(n_seqs=n_seqs, n_bases=int(offsets[-1]), n_full_windows=full)
    return index, names, info
