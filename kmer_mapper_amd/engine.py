"""DeviceIndex — a Kmer Index resident in HBM plus its uint32 node-count vector.

Thin object wrapper over the C ABI (include/kmm.h).  Everything the reference does per chunk in
map_cpu (kmer_mapper/command_line_interface.py:32-56) happens inside `map_reads`; the
operator-level `map_kmers` is the drop-in for mapper.pyx:19-72.
"""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib

_P = ctypes.c_void_p

# what DeviceIndex.read_nodes returns (kmm_read_nodes, include/kmm.h)
ReadNodes = namedtuple("ReadNodes", "best_node best_votes second_votes total_votes n_nodes n_rounds")


def _is_torch_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "data_ptr")


def _n_bytes(b, n_bytes):
    """The bytes of `b` a call takes: all of them, or the first n_bytes."""
    n = b.n if n_bytes is None else int(n_bytes)
    if n > b.n:
        raise ValueError("n_bytes exceeds the buffer")
    return n


class _Arg:
    """A borrowed pointer for one C call: numpy array (host) or torch tensor (host or device)."""

    def __init__(self, x, dtype, name):
        self.keep = None
        if x is None:
            self.ptr, self.n = None, 0
            return
        if _is_torch_tensor(x):
            import torch
            want = {np.uint8: torch.uint8, np.int64: torch.int64, np.int32: torch.int32,
                    np.uint64: getattr(torch, "uint64", None), np.uint16: getattr(torch, "uint16", None),
                    np.uint32: getattr(torch, "uint32", None)}[dtype]
            if x.dtype != want and not (dtype is np.uint64 and x.dtype == torch.int64) \
                    and not (dtype is np.uint32 and x.dtype == torch.int32):
                raise ValueError("Buffer dtype mismatch for %s: expected %s got %s"
                                 % (name, np.dtype(dtype), x.dtype))
            if not x.is_contiguous():
                raise ValueError("%s: ndarray is not C-contiguous" % name)
            self.keep, self.ptr, self.n = x, _P(x.data_ptr()), x.numel()
            return
        a = np.asarray(x)
        if a.dtype != np.dtype(dtype):
            # the reference's typed memoryviews reject other dtypes (mapper.pyx:19,22-28)
            raise ValueError("Buffer dtype mismatch for %s: expected '%s' but got '%s'"
                             % (name, np.dtype(dtype), a.dtype))
        if not a.flags.c_contiguous:
            raise ValueError("%s: ndarray is not C-contiguous" % name)
        self.keep, self.ptr, self.n = a, a.ctypes.data_as(_P), a.size


class DeviceIndex:
    """The five index arrays of graph_kmer_index.KmerIndex (mapper.pyx:22-29) repacked in HBM."""

    def __init__(self, hashes_to_index, n_kmers, modulo, kmers, nodes, frequencies, max_node_id,
                 device=0):
        L = _lib.lib()
        h2i = _Arg(hashes_to_index, np.int32, "hashes_to_index")
        nk = _Arg(n_kmers, np.int32, "n_kmers")
        km = _Arg(kmers, np.uint64, "kmers")
        nd = _Arg(nodes, np.int32, "nodes")
        fr = _Arg(frequencies, np.uint16, "frequencies")
        modulo = int(modulo)
        if h2i.n != modulo or nk.n != modulo:
            raise ValueError("hashes_to_index / n_kmers must have `modulo`=%d entries (got %d, %d)"
                             % (modulo, h2i.n, nk.n))
        if not (km.n == nd.n == fr.n):
            raise ValueError("kmers / nodes / frequencies differ in length")
        self._h = _P()
        self.max_node_id = int(max_node_id)
        self.modulo = modulo
        self.n_entries = km.n
        self.device = int(device)
        _lib.check(L.kmm_index_create(h2i.ptr, nk.ptr, modulo, km.ptr, nd.ptr, fr.ptr, km.n,
                                      self.max_node_id, self.device, ctypes.byref(self._h)))
        self._bound = None

    @classmethod
    def from_index(cls, index, max_node_id=None, device=0):
        """From any object with the attributes mapper.pyx:22-29 reads (duck-typed, like the reference)."""
        if max_node_id is None:
            max_node_id = index.max_node_id()
        return cls(index._hashes_to_index, index._n_kmers, index._modulo, index._kmers,
                   index._nodes, index._frequencies, max_node_id, device=device)

    # -- lifetime --------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().kmm_index_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- counts ----------------------------------------------------------------------------------
    def reset(self):
        _lib.check(_lib.lib().kmm_reset_counts(self._h))

    def bind_counts(self, tensor):
        """Accumulate into a caller-owned device tensor of max_node_id+1 32-bit ints (for RCCL)."""
        if tensor is None:
            _lib.check(_lib.lib().kmm_bind_counts(self._h, None))
            self._bound = None
            return
        if tensor.numel() != self.max_node_id + 1 or tensor.element_size() != 4:
            raise ValueError("bind_counts needs %d 32-bit elements" % (self.max_node_id + 1))
        _lib.check(_lib.lib().kmm_bind_counts(self._h, _P(tensor.data_ptr())))
        self._bound = tensor

    def synchronize(self):
        _lib.check(_lib.lib().kmm_synchronize(self._h))

    def get_node_counts(self, out=None, pinned=False):
        """The count vector on the host.  pinned: into a fresh page-locked array (freed with it) — the copy of a large
        vector then runs at the link's rate."""
        if out is None:
            out = (_lib.pinned_array(self.max_node_id + 1, np.uint32) if pinned
                   else np.empty(self.max_node_id + 1, dtype=np.uint32))
        _lib.check(_lib.lib().kmm_get_node_counts(self._h, out.ctypes.data_as(_P)))
        return out

    def count_kmers_mode(self, on=True):
        """Per-k-mer counting mode (gpu_counter.py:23-37, command_line_interface.py:46-49): every batch takes the
        radix path, hits are kept per index entry (get_kmer_counts) and summed into the node counts."""
        self.set_param("count_kmers", int(bool(on)))

    def get_kmer_counts(self, out=None):
        """uint32[n_entries]: how many mapped k-mers matched each index entry, in the entry order given to the
        constructor (needs count_kmers_mode() before mapping)."""
        if out is None:
            out = np.empty(self.n_entries, dtype=np.uint32)
        dst = _Arg(out, np.uint32, "out") if not _is_torch_tensor(out) else None
        ptr = dst.ptr if dst is not None else _P(out.data_ptr())
        _lib.check(_lib.lib().kmm_get_kmer_counts(self._h, ptr))
        return out

    # -- multi-GPU: one process per GPU, RCCL behind the C ABI -------------------------------------
    @staticmethod
    def comm_unique_id():
        """128 bytes created on rank 0 (kmm_comm_get_unique_id); hand them to every rank."""
        buf = (ctypes.c_uint8 * 128)()
        _lib.check(_lib.lib().kmm_comm_get_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, n_ranks, rank):
        """Collective: join the communicator of the job with this handle."""
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _lib.check(_lib.lib().kmm_comm_init_rank(self._h, buf, int(n_ranks), int(rank)))

    def comm_reduce_counts(self, root=0):
        """Collective: sum of the ranks' count vectors, in place (root = -1: on every rank).  Replaces the additive
        reduce of command_line_interface.py:124-130."""
        _lib.check(_lib.lib().kmm_comm_reduce_counts(self._h, int(root)))

    # -- the hot path ----------------------------------------------------------------------------
    def map_kmers(self, kmers, max_index_lookup_frequency=1000, also_revcomp=False, k=31):
        a = _Arg(kmers, np.uint64, "kmers")
        _lib.check(_lib.lib().kmm_map_kmers(self._h, a.ptr, a.n, int(max_index_lookup_frequency),
                                            int(bool(also_revcomp)), int(k)))

    def _map_reads_qual(self, b, qualities, qual_base, o, n_reads, read_len, k, max_index_lookup_frequency, also_revcomp, t):
        """kmm_map_reads_qual: the reads of map_reads (o given) / map_reads_uniform (o None) with one quality byte per base."""
        q = _Arg(qualities, np.uint8, "qualities")
        if q.n != b.n:
            raise ValueError("qualities holds %d bytes, bases %d: one quality byte per base" % (q.n, b.n))
        _lib.check(_lib.lib().kmm_map_reads_qual(self._h, b.ptr, q.ptr, int(qual_base), o.ptr if o is not None else None,
                                                 int(n_reads), int(read_len), int(k), int(max_index_lookup_frequency),
                                                 int(bool(also_revcomp)), t.ptr))

    def map_reads(self, bases, read_offsets, k=31, max_index_lookup_frequency=1000,
                  also_revcomp=False, lut=None, qualities=None, qual_base=33):
        """qualities: one quality byte per base (what `bases` takes, host or device) — with set_param("min_base_quality", Q)
        a base whose byte is below qual_base + Q is a break (kmm_map_reads_qual; qual_base 33 = Phred+33 text, 0 = raw
        Phred as BAM stores it).  None: kmm_map_reads, which knows no floor."""
        b = _Arg(bases, np.uint8, "bases")
        o = _Arg(read_offsets, np.int64, "read_offsets")
        t = _Arg(lut, np.uint8, "lut")
        if lut is not None and t.n != 256:
            raise ValueError("lut must have 256 entries")
        if o.n < 1:
            raise ValueError("read_offsets needs n_reads+1 entries")
        if qualities is not None:
            return self._map_reads_qual(b, qualities, qual_base, o, o.n - 1, 0, k, max_index_lookup_frequency, also_revcomp, t)
        _lib.check(_lib.lib().kmm_map_reads(self._h, b.ptr, o.ptr, o.n - 1, int(k),
                                            int(max_index_lookup_frequency),
                                            int(bool(also_revcomp)), t.ptr))

    def map_reads_uniform(self, bases, n_reads, read_len, k=31, max_index_lookup_frequency=1000,
                          also_revcomp=False, lut=None, qualities=None, qual_base=33):
        """qualities / qual_base: as map_reads."""
        b = _Arg(bases, np.uint8, "bases")
        t = _Arg(lut, np.uint8, "lut")
        if b.n < int(n_reads) * int(read_len):
            raise ValueError("bases holds %d bytes, need n_reads*read_len=%d"
                             % (b.n, int(n_reads) * int(read_len)))
        if qualities is not None:
            return self._map_reads_qual(b, qualities, qual_base, None, n_reads, read_len, k, max_index_lookup_frequency,
                                        also_revcomp, t)
        _lib.check(_lib.lib().kmm_map_reads_uniform(self._h, b.ptr, int(n_reads), int(read_len),
                                                    int(k), int(max_index_lookup_frequency),
                                                    int(bool(also_revcomp)), t.ptr))

    def map_records(self, raw, n_bytes=None, fmt=_lib.FORMAT_FASTQ, k=31, max_index_lookup_frequency=1000,
                    also_revcomp=False, lut=None):
        """Map a raw FASTQ (fmt=4) / two-line FASTA (fmt=2) / SAM (fmt=8; "bam_exclude_flags" filters it) chunk parsed on
        the GPU.
        Returns (consumed_bytes, n_records); the caller carries raw[consumed:] to the next chunk.
        A base-quality floor is a parameter of the handle: set_param("min_base_quality", Q) makes every FASTQ base whose
        quality byte is below '!' + Q a break, on this call and on map_bgzf / map_gzip (no effect on FASTA; SAM and map_bam
        are refused while it is set, unless set_param("use_record_qual", 1) has their QUAL decoded beside SEQ:
        get_param("records_without_qual") then counts the records that store none and passed unmasked), and get_param("quality_masked_bases") counts the bases it masked since the last
        get_stats(reset=True).  Reads already held as arrays bring their quality bytes to map_reads / map_reads_uniform
        (qualities=...), which apply the same floor."""
        b = _Arg(raw, np.uint8, "raw")
        t = _Arg(lut, np.uint8, "lut")
        n = _n_bytes(b, n_bytes)
        consumed = ctypes.c_int64(0)
        n_rec = ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_map_records(self._h, b.ptr, n, int(fmt), int(k),
                                              int(max_index_lookup_frequency), int(bool(also_revcomp)),
                                              t.ptr, ctypes.byref(consumed), ctypes.byref(n_rec)))
        return consumed.value, n_rec.value

    def _hint_next(self, next_chunk):
        if next_chunk is not None and len(next_chunk):
            # the bytes that follow `comp` in the caller's memory (a view of the same file mapping): staged under this chunk's
            # inflate kernel (kmm_map_bgzf_hint_next); the next call passes comp[used:] + next_chunk as one view
            nx = _Arg(next_chunk, np.uint8, "next_chunk")
            _lib.check(_lib.lib().kmm_map_bgzf_hint_next(self._h, nx.ptr, nx.n))

    def _map_stream(self, entry, comp, n_bytes, fmt, first, last, k, max_index_lookup_frequency, also_revcomp, lut, more_flags=0):
        """One call of a compressed stream's entry point (kmm_map_bgzf / kmm_map_gzip / kmm_map_bam): (used, n_records)."""
        b = _Arg(comp, np.uint8, "comp")
        t = _Arg(lut, np.uint8, "lut")
        n = _n_bytes(b, n_bytes)
        used = ctypes.c_int64(0)
        n_rec = ctypes.c_int64(0)
        flags = (_lib.FORMAT_NEW_STREAM if first else 0) | (_lib.FORMAT_LAST_CHUNK if last else 0) | more_flags
        _lib.check(getattr(_lib.lib(), entry)(self._h, b.ptr, n, int(fmt) | flags, int(k), int(max_index_lookup_frequency),
                                              int(bool(also_revcomp)), t.ptr, ctypes.byref(used), ctypes.byref(n_rec)))
        return used.value, n_rec.value

    def map_bgzf(self, comp, n_bytes=None, fmt=_lib.FORMAT_FASTQ, k=31, max_index_lookup_frequency=1000, also_revcomp=False,
                 lut=None, first=False, last=False, head_skip=0, tail_stop=None, next_chunk=None):
        """Map a chunk of a BGZF-compressed FASTQ (fmt=4) / two-line FASTA (fmt=2) / SAM (fmt=8) file, inflated on the GPU
        (kmm_map_bgzf).
        `comp` starts at a member boundary; returns (compressed bytes used, records mapped): continue at comp[used:].  The
        handle carries the inflated bytes behind the last complete record to the next call; first / last mark the file's
        first / last chunk.  A rank's share of a file (bgzf_ranges.rank_member_range): head_skip = inflated bytes of the
        FIRST chunk's first member that belong to the rank before; tail_stop = how many inflated bytes of the LAST chunk's
        last member are this rank's (None: all).  next_chunk: see below."""
        self._hint_next(next_chunk)
        if head_skip:
            self.set_param("bgzf_head_skip", int(head_skip))
        if tail_stop is not None:
            self.set_param("bgzf_tail_stop", int(tail_stop))
        return self._map_stream("kmm_map_bgzf", comp, n_bytes, fmt, first, last, k, max_index_lookup_frequency, also_revcomp, lut)

    def map_gzip(self, comp, n_bytes=None, fmt=_lib.FORMAT_FASTQ, k=31, max_index_lookup_frequency=1000, also_revcomp=False,
                 lut=None, first=False, last=False):
        """Map a window of a PLAIN gzip-compressed FASTQ (fmt=4) / two-line FASTA (fmt=2) / SAM (fmt=8) file, inflated on the GPU
        (kmm_map_gzip).  `comp` is any prefix of the rest of the file; returns (compressed bytes used, records mapped):
        continue at comp[used:].  first / last mark the file's first / last window (per call: nothing is kept for later)."""
        return self._map_stream("kmm_map_gzip", comp, n_bytes, fmt, first, last, k, max_index_lookup_frequency, also_revcomp, lut)

    def map_bam(self, comp, first, last, next_chunk=None, n_bytes=None, k=31, max_index_lookup_frequency=1000, also_revcomp=False,
                lut=None, mid_stream=False, head_skip=0, tail_stop=None):
        """Map a window of a BAM file (kmm_map_bam): BGZF members inflated, records found and their SEQ decoded on the GPU.
        `comp` starts at a member boundary; returns (compressed bytes used, records mapped): continue at comp[used:].  first /
        last mark the file's first / last window (the header is read on the first; a first window that ends inside the header
        uses nothing: bring a longer one).  next_chunk: the bytes that follow `comp` in the caller's memory, staged under this
        window's inflate kernel (as map_bgzf).
        A rank's share of a file (bgzf_ranges.rank_member_range_bam): mid_stream = the stream begins behind the header — its
        first call (first=True) expects no header, takes n_ref from set_param("bam_n_ref", ...) and starts at the record
        head_skip inflated bytes into the first member; tail_stop = how many inflated bytes of the LAST window's last member
        are this rank's (None: all).  Both are written on every first / last call, so a stream that failed leaves no stale
        value for the next file."""
        self._hint_next(next_chunk)
        if first:
            self.set_param("bgzf_head_skip", int(head_skip))
        if last:
            self.set_param("bgzf_tail_stop", -1 if tail_stop is None else int(tail_stop))
        return self._map_stream("kmm_map_bam", comp, n_bytes, 0, first, last, k, max_index_lookup_frequency, also_revcomp, lut,
                                more_flags=_lib.FORMAT_MID_STREAM if mid_stream else 0)

    def bam_header(self, comp=None, n_bytes=None):
        """kmm_bam_header: `comp` starts at a BAM file's first member.  Returns (n_ref, hdr_member, hdr_skip): the reference count
        and where the first record lies (compressed offset of its member, offset in the member's inflated bytes); n_ref = -1:
        the window ends inside the header — bring a longer one.
        Without `comp` — kmm_bam_stream_header: the header of the last stream that map_bam started on this handle
        with first=True, as bytes, from the magic through the last reference; ValueError when there is none (no stream, a first
        window that ended inside the header, or a mid-stream share)."""
        if comp is None:
            n = ctypes.c_int64(0)
            if _lib.lib().kmm_bam_stream_header(self._h, None, 0, ctypes.byref(n)) != _lib.KMM_OK and n.value == 0:
                _lib.check(_lib.KMM_ERR_INVALID_ARG)                  # (no header: the library's message)
            buf = np.empty(max(n.value, 1), dtype=np.uint8)
            _lib.check(_lib.lib().kmm_bam_stream_header(self._h, buf.ctypes.data_as(_P), n.value, ctypes.byref(n)))
            return buf[:n.value].tobytes()
        b = _Arg(comp, np.uint8, "comp")
        n_ref, member, skip = ctypes.c_int32(-1), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_bam_header(self._h, b.ptr, _n_bytes(b, n_bytes), ctypes.byref(n_ref), ctypes.byref(member),
                                             ctypes.byref(skip)))
        return n_ref.value, member.value, skip.value

    def bam_find_record_start(self, comp, n_ref, n_bytes=None):
        """kmm_bam_find_record_start: `comp` starts at a member boundary of a BAM file with n_ref references.  Returns
        (member, skip): the first position from which a chain of records holds to the end of the window's whole members, as
        the compressed offset (relative to comp) of the member that holds it and the offset in that member's inflated bytes;
        (len, 0): comp ends the file and no record starts in it; member = -1: no chain holds — bring a longer window."""
        b = _Arg(comp, np.uint8, "comp")
        member, skip = ctypes.c_int64(-1), ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_bam_find_record_start(self._h, b.ptr, _n_bytes(b, n_bytes), int(n_ref), ctypes.byref(member),
                                                        ctypes.byref(skip)))
        return member.value, skip.value

    def map_packed(self, codes, n_bases, n_reads, read_len=0, read_starts=None, k=31, max_index_lookup_frequency=1000,
                   also_revcomp=False):
        """Reads held as 2-bit codes (uint32 words, 16 codes per word, first base lowest): kmm_map_packed.  read_len > 0:
        n_reads reads of one length; else `read_starts` = uint32 bitset over the base positions."""
        c = _Arg(codes, np.uint32, "codes")
        st = _Arg(read_starts, np.uint32, "read_starts")
        if c.n < (int(n_bases) + 15) // 16:
            raise ValueError("codes holds %d words, need %d" % (c.n, (int(n_bases) + 15) // 16))
        if not read_len and st.n < int(n_bases) // 32 + 1:
            raise ValueError("read_starts needs n_bases / 32 + 1 words")
        _lib.check(_lib.lib().kmm_map_packed(self._h, c.ptr, int(n_bases), int(n_reads), int(read_len), st.ptr, int(k),
                                             int(max_index_lookup_frequency), int(bool(also_revcomp))))

    def in_index(self, kmers):
        a = _Arg(kmers, np.uint64, "kmers")
        out = np.zeros(a.n, dtype=np.uint8)
        _lib.check(_lib.lib().kmm_in_index(self._h, a.ptr, a.n, out.ctypes.data_as(_P)))
        return out

    def read_hits(self, bases, read_offsets=None, n_reads=None, read_len=None, k=31, max_index_lookup_frequency=1000,
                  also_revcomp=False, lut=None, windows=False):
        """kmm_read_hits: per read, how many of its k-mers are in the index (a window is a hit once, whatever the number of
        entries or orientations that match; entries above max_index_lookup_frequency do not count).  read_offsets given:
        ragged reads; else n_reads reads of read_len bytes.  A pure query: the counts of the handle do not move.
        numpy in -> numpy uint32[n_reads] out; torch device tensors in -> torch device tensors out.  windows=True returns
        (hits, windows): windows[r] = the windows of read r that were looked up (those over a break byte are not)."""
        b = _Arg(bases, np.uint8, "bases")
        t = _Arg(lut, np.uint8, "lut")
        if lut is not None and t.n != 256:
            raise ValueError("lut must have 256 entries")
        if read_offsets is not None:
            o = _Arg(read_offsets, np.int64, "read_offsets")
            if o.n < 1:
                raise ValueError("read_offsets needs n_reads+1 entries")
            n, L, optr = o.n - 1, 0, o.ptr
        else:
            if n_reads is None or read_len is None:
                raise ValueError("read_hits needs read_offsets, or n_reads and read_len")
            n, L, optr = int(n_reads), int(read_len), None
            if n < 0 or L < 0:
                raise ValueError("n_reads / read_len negative")
            if b.n < n * L:
                raise ValueError("bases holds %d bytes, need n_reads*read_len=%d" % (b.n, n * L))
        if _is_torch_tensor(bases) and bases.is_cuda:
            import torch
            dt = getattr(torch, "uint32", torch.int32)
            hits = torch.zeros(n, dtype=dt, device=bases.device)
            win = torch.zeros(n, dtype=dt, device=bases.device) if windows else None
            hp, wp = _P(hits.data_ptr()), (_P(win.data_ptr()) if windows else None)
        else:
            hits = np.zeros(n, dtype=np.uint32)
            win = np.zeros(n, dtype=np.uint32) if windows else None
            hp, wp = hits.ctypes.data_as(_P), (win.ctypes.data_as(_P) if windows else None)
        _lib.check(_lib.lib().kmm_read_hits(self._h, b.ptr, optr, n, L, int(k), int(max_index_lookup_frequency),
                                            int(bool(also_revcomp)), t.ptr, hp, wp))
        return (hits, win) if windows else hits

    def read_nodes(self, bases, read_offsets=None, n_reads=None, read_len=None, k=31, max_index_lookup_frequency=1000,
                   also_revcomp=False, lut=None, table_bytes=0):
        """kmm_read_nodes: per read, the node that most of its k-mers map to.  A vote is what map_reads would add to a node
        count for the read alone (one per matching entry, both orientations with also_revcomp, entries above
        max_index_lookup_frequency left out).  Reads as in read_hits.  Returns ReadNodes(best_node int32, best_votes,
        second_votes, total_votes, n_nodes uint32, n_rounds int): best_node is the node with the most votes, the smallest id
        among equals, -1 without a vote; second_votes the most votes among the other nodes.  table_bytes: the target size
        of a round's vote table (0: the library's default); the answer does not depend on it.  A pure query.
        numpy in -> numpy out; torch device tensors in -> torch device tensors out."""
        b = _Arg(bases, np.uint8, "bases")
        t = _Arg(lut, np.uint8, "lut")
        if lut is not None and t.n != 256:
            raise ValueError("lut must have 256 entries")
        if read_offsets is not None:
            o = _Arg(read_offsets, np.int64, "read_offsets")
            if o.n < 1:
                raise ValueError("read_offsets needs n_reads+1 entries")
            n, L, optr = o.n - 1, 0, o.ptr
        else:
            if n_reads is None or read_len is None:
                raise ValueError("read_nodes needs read_offsets, or n_reads and read_len")
            n, L, optr = int(n_reads), int(read_len), None
            if n < 0 or L < 0:
                raise ValueError("n_reads / read_len negative")
            if b.n < n * L:
                raise ValueError("bases holds %d bytes, need n_reads*read_len=%d" % (b.n, n * L))
        if _is_torch_tensor(bases) and bases.is_cuda:
            import torch
            dt = getattr(torch, "uint32", torch.int32)
            outs = [torch.full((n,), -1, dtype=torch.int32, device=bases.device)]
            outs += [torch.zeros(n, dtype=dt, device=bases.device) for _ in range(4)]
            ptrs = [_P(x.data_ptr()) for x in outs]
        else:
            outs = [np.full(n, -1, dtype=np.int32)] + [np.zeros(n, dtype=np.uint32) for _ in range(4)]
            ptrs = [x.ctypes.data_as(_P) for x in outs]
        rounds = ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_read_nodes(self._h, b.ptr, optr, n, L, int(k), int(max_index_lookup_frequency),
                                             int(bool(also_revcomp)), t.ptr, int(table_bytes), *ptrs, ctypes.byref(rounds)))
        return ReadNodes(*outs, rounds.value)

    def record_hits(self, on=True, windows=False, min_base_quality=0):
        """The record-hits mode (include/kmm.h): while it is on, map_records / map_bgzf / map_gzip / map_bam
        append one entry per record — its index hits, with windows=True also its windows, as read_hits defines them — to a
        queue of the handle instead of counting nodes; take_record_hits() fetches them.  on=False: the calls count nodes
        again; entries still pending stay takeable.
        min_base_quality: the mode's own floor, "record_hits_min_base_quality" (DESIGN 4.27): a FASTQ base whose quality byte is
        below '!' + Q is a break for hits and windows alike, the kept text is never altered; SAM / BAM records need
        set_param("use_record_qual", 1), and those that store no qualities pass unmasked.  0, and on=False: no floor."""
        self.set_param("record_hits_min_base_quality", int(min_base_quality) if on else 0)
        self.set_param("record_hits", (2 if windows else 1) if on else 0)

    def take_record_hits(self, capacity=None, out=None):
        """kmm_take_record_hits: the oldest pending entries (all of them, or at most `capacity`), in stream order, as numpy
        uint32 arrays: hits — or (hits, windows) when the entries were appended with windows=True.  They leave the queue.
        out: (hits, windows-or-None) arrays or torch tensors to write into instead (host or device, uint32 / int32; their
        length is the capacity); then the number of entries taken is returned."""
        with_windows = self.get_param("record_hits_pending_mode") == 2 if out is None else out[1] is not None
        taken = ctypes.c_int64(0)
        if out is not None:
            h, w = _Arg(out[0], np.uint32, "hits"), _Arg(out[1], np.uint32, "windows")
            cap = h.n if capacity is None else min(int(capacity), h.n)
            if with_windows and w.n < cap:
                raise ValueError("windows holds %d entries, hits %d" % (w.n, cap))
            _lib.check(_lib.lib().kmm_take_record_hits(self._h, h.ptr, w.ptr, cap, ctypes.byref(taken)))
            return taken.value
        pending = self.get_param("record_hits_pending")
        cap = pending if capacity is None else min(int(capacity), pending)
        hits = np.zeros(cap, dtype=np.uint32)
        win = np.zeros(cap, dtype=np.uint32) if with_windows else None
        _lib.check(_lib.lib().kmm_take_record_hits(self._h, hits.ctypes.data_as(_P),
                                                   win.ctypes.data_as(_P) if with_windows else None, cap, ctypes.byref(taken)))
        hits = hits[:taken.value]
        return (hits, win[:taken.value]) if with_windows else hits

    def record_keep(self, on=True, min_hits=1, min_permille=0, invert=False):
        """The record-keep mode (include/kmm.h), on top of record_hits(): the record calls also append the TEXT of
        every record whose entry passes the keep rule — hits >= min_hits and 1000 * hits >= min_permille * windows, the
        outcome flipped by invert — to a byte queue of the handle; take_kept_records() fetches it.  min_permille > 0 needs
        record_hits(windows=True).  on=False: nothing more is appended; bytes still pending stay takeable."""
        self.set_param("record_keep_min_hits", int(min_hits))
        self.set_param("record_keep_min_permille", int(min_permille))
        self.set_param("record_keep_invert", int(bool(invert)))
        self.set_param("record_keep", int(bool(on)))

    def record_names(self, on=True, mate_suffix=False, pairs=False):
        """The named form of the BAM decode (include/kmm.h), on top of record_hits(): map_bam decodes every selected
        record into four-line FASTQ that carries the read's name and qualities ('@' NAME '\\n' SEQ '\\n' "+\\n" QUAL '\\n') instead
        of ">\\n" SEQ — the text record_keep() appends for BAM input.  Name bytes outside '!' .. '~' are written as '?'
        (get_param("record_name_bytes_replaced")); records without qualities get '"' per base.  mate_suffix: "/1" behind the
        name of a record whose FLAG has 0x40 and not 0x80, "/2" for 0x80 and not 0x40.  The text routes never read it.
        pairs (with record_keep()): the selected records of a map_bam stream are mates in file order — 2p and 2p + 1,
        as in a name-collated file — kept or dropped together under record_pairs()'s rule; their names are compared on the GPU
        and a pair of strangers, or an unpaired last record, fails the call.  Refused while hit entries are pending."""
        self.set_param("record_names_pairs", int(bool(on and pairs)))
        self.set_param("record_names_mate_suffix", int(bool(mate_suffix)))
        self.set_param("record_names", int(bool(on)))

    def record_bam(self, on=True, mates=False):
        """The raw form of the keep (include/kmm.h), on top of record_hits() and record_keep(): map_bam maps the
        selected records as without the switch and appends every kept record AS IT STANDS IN THE FILE — its block_size word and
        the block_size bytes behind it — to the queue of take_kept_records() / take_kept_bgzf(); bam_header() has the header that
        goes in front.  The text routes never read it.  Refused while kept bytes are pending.
        mates: the selected records of a map_bam stream are mates in file order — 2p and 2p + 1, as in a
        name-collated file — kept or dropped together under record_pairs()'s rule; their read_name bytes are compared on the GPU
        and a pair of strangers, or an unpaired last record, fails the call.  Refused while hit entries or kept bytes are pending."""
        if not (on and mates):
            self.set_param("record_bam_mates", 0)
        self.set_param("record_bam", int(bool(on)))
        if on and mates:
            self.set_param("record_bam_mates", 1)

    def record_sam(self, on=True, header=True, mates=False):
        """SAM lines kept as SAM lines (include/kmm.h), on top of record_hits() and record_keep(): a SAM call
        (map_records, map_bgzf, map_gzip with FORMAT_SAM) maps the selected records as without the switch and appends every kept
        record's WHOLE LINE, untouched, to the queue of take_kept_records() / take_kept_bgzf(); header=True: every header line
        too, at its place in the stream; False: none (shares that are concatenated).  The other formats never read it.  Refused
        while kept bytes are pending.
        mates: the selected records of the stream are mates in file order — 2p and 2p + 1, as an aligner writes
        them — kept or dropped together under record_pairs()'s rule, mate 1 directly in front of mate 2; their QNAME bytes are
        compared on the GPU and a pair of strangers, or (with FORMAT_LAST_CHUNK / last=True) an unpaired last record, fails the
        call.  get_param("record_sam_mate_waiting") tells whether a mate 1 waits for the next call.  Refused while hit entries
        or kept bytes are pending."""
        if not (on and mates):
            self.set_param("record_sam_mates", 0)
        self.set_param("record_sam", (1 if header else 2) if on else 0)
        if on and mates:
            self.set_param("record_sam_mates", 1)

    def take_kept_records(self, out=None):
        """kmm_take_kept_records: ALL pending bytes — the kept records, whole, in stream order — as (np.uint8 array, n_records);
        they leave the queue.  out: a uint8 array or torch tensor (host or device) to write into instead, at least as long as
        the pending bytes; then (n_bytes, n_records) is returned."""
        n_bytes, n_records = ctypes.c_int64(0), ctypes.c_int64(0)
        if out is not None:
            o = _Arg(out, np.uint8, "out")
            _lib.check(_lib.lib().kmm_take_kept_records(self._h, o.ptr, o.n, ctypes.byref(n_bytes), ctypes.byref(n_records)))
            return n_bytes.value, n_records.value
        pending = self.get_param("record_keep_pending_bytes")
        buf = np.empty(pending, dtype=np.uint8)
        _lib.check(_lib.lib().kmm_take_kept_records(self._h, buf.ctypes.data_as(_P) if pending else None, pending,
                                                    ctypes.byref(n_bytes), ctypes.byref(n_records)))
        return buf[:n_bytes.value], n_records.value

    PAIR_RULES = {"any": 0, "both": 1}

    def record_pairs(self, on=True, rule="any"):
        """Keeping mates together (include/kmm.h), on top of record_keep(): the records of a stream are interleaved —
        2i and 2i + 1 are mates — and both are kept or both dropped: a pair matches when `rule` "any" of its mates passes the
        keep rule (without its inversion), or only when "both" do, and invert flips the pair's outcome.  map_records (FASTQ,
        two-line FASTA), map_bgzf and map_gzip then take whole pairs only.  rule is also the rule of map_record_pairs, which
        does not read `on`.  Refused while hit entries are pending."""
        if rule not in self.PAIR_RULES:
            raise ValueError("rule must be 'any' or 'both', not %r" % (rule,))
        self.set_param("record_pairs_rule", self.PAIR_RULES[rule])
        self.set_param("record_pairs", int(bool(on)))

    def map_record_pairs(self, raw1, raw2, fmt=_lib.FORMAT_FASTQ, k=31, max_index_lookup_frequency=1000, also_revcomp=False,
                         lut=None, n_bytes1=None, n_bytes2=None):
        """kmm_map_record_pairs: record i of raw1 and record i of raw2 (FASTQ or two-line FASTA chunks, each in host or device
        memory) are mates, kept or dropped together under record_keep()'s rule and record_pairs()'s pair rule.  The hits queue
        gains two entries per pair (mate 1, mate 2); the kept mate-1 text goes to the queue of take_kept_records(), the kept
        mate-2 text to take_kept_mates(1).  Returns (consumed1, consumed2, n_pairs): only whole pairs are taken, the caller
        carries raw1[consumed1:] and raw2[consumed2:] to the next chunks."""
        a, b = _Arg(raw1, np.uint8, "raw1"), _Arg(raw2, np.uint8, "raw2")
        t = _Arg(lut, np.uint8, "lut")
        c1, c2, n_pairs = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_map_record_pairs(self._h, a.ptr, _n_bytes(a, n_bytes1), b.ptr, _n_bytes(b, n_bytes2), int(fmt), int(k),
                                                   int(max_index_lookup_frequency), int(bool(also_revcomp)), t.ptr,
                                                   ctypes.byref(c1), ctypes.byref(c2), ctypes.byref(n_pairs)))
        return c1.value, c2.value, n_pairs.value

    def take_kept_mates(self, mate, out=None):
        """kmm_take_kept_mates: take_kept_records() on the queue of mate 0 (the same queue) or mate 1 (the mate-2 texts of
        map_record_pairs)."""
        n_bytes, n_records = ctypes.c_int64(0), ctypes.c_int64(0)
        if out is not None:
            o = _Arg(out, np.uint8, "out")
            _lib.check(_lib.lib().kmm_take_kept_mates(self._h, int(mate), o.ptr, o.n, ctypes.byref(n_bytes), ctypes.byref(n_records)))
            return n_bytes.value, n_records.value
        pending = self.get_param("record_keep_pending_bytes_mate2" if int(mate) == 1 else "record_keep_pending_bytes")
        buf = np.empty(pending, dtype=np.uint8)
        _lib.check(_lib.lib().kmm_take_kept_mates(self._h, int(mate), buf.ctypes.data_as(_P) if pending else None, pending,
                                                  ctypes.byref(n_bytes), ctypes.byref(n_records)))
        return buf[:n_bytes.value], n_records.value

    def take_kept_bgzf(self, mate=0, out=None):
        """kmm_take_kept_bgzf: take_kept_mates() with the queue's text compressed on the device — BGZF members of at
        most 65280 bytes of text each, no end-of-file block — so that only the members cross the link.  Returns (np.uint8
        array of members, n_text_bytes, n_records); with out (a uint8 array or torch tensor, host or device, at least
        kmm_bgzf_bound(pending bytes) long) the members are written there and (n_member_bytes, n_text_bytes, n_records) is
        returned."""
        n_comp, n_bytes, n_records = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        refs = (ctypes.byref(n_comp), ctypes.byref(n_bytes), ctypes.byref(n_records))
        if out is not None:
            o = _Arg(out, np.uint8, "out")
            _lib.check(_lib.lib().kmm_take_kept_bgzf(self._h, int(mate), o.ptr, o.n, *refs))
            return n_comp.value, n_bytes.value, n_records.value
        pending = self.get_param("record_keep_pending_bytes_mate2" if int(mate) == 1 else "record_keep_pending_bytes")
        cap = int(_lib.lib().kmm_bgzf_bound(pending))
        buf = np.empty(cap, dtype=np.uint8)
        _lib.check(_lib.lib().kmm_take_kept_bgzf(self._h, int(mate), buf.ctypes.data_as(_P) if cap else None, cap, *refs))
        return buf[:n_comp.value], n_bytes.value, n_records.value

    # -- measurement -----------------------------------------------------------------------------
    def set_timing(self, on=True):
        _lib.check(_lib.lib().kmm_set_timing(self._h, int(bool(on))))

    def get_timing(self, kernel_id=None):
        """(milliseconds, launches) of one kernel id since the last call, or a dict over all ids."""
        if kernel_id is None:
            return {name: self.get_timing(i) for i, name in enumerate(_lib.KERNEL_NAMES)}
        ms = ctypes.c_double(0.0)
        n = ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_get_timing(self._h, int(kernel_id), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def get_stats(self, reset=False):
        """(k-mer lookups performed, count increments) since creation / the last reset."""
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(_lib.lib().kmm_get_stats(self._h, int(bool(reset)), ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_param(self, name, value):
        """kmm_set_param: the names, the values they take and what they do are documented in include/kmm.h (the list above
        kmm_set_param, and the sections of the calls that read them)."""
        _lib.check(_lib.lib().kmm_set_param(self._h, name.encode(), int(value)))

    def set_record_regions(self, regions, keep_unplaced=False):
        """kmm_set_record_regions: only SAM / BAM records that overlap one of `regions` are mapped (beside "bam_exclude_flags",
        "bam_include_flags" and "bam_min_mapq"; include/kmm.h RECORD SELECTION).  regions: [(ref_name, ref_id, beg, end)],
        0-based half-open, as util.parse_regions / util.read_bed_regions give them — ref_name (str / bytes, or None) selects SAM
        records, ref_id (an index into the BAM header's references, or None / -1) BAM records.  keep_unplaced: the records
        without a reference pass.  An empty list clears the selection.  get_param("record_regions"): intervals after merging."""
        regions = list(regions or ())
        arr = (_lib.Region * max(len(regions), 1))()
        for i, (name, ref_id, beg, end) in enumerate(regions):
            arr[i].ref_name = None if name is None else (name if isinstance(name, bytes) else str(name).encode())
            arr[i].ref_id = -1 if ref_id is None else int(ref_id)
            arr[i].beg, arr[i].end = int(beg), int(end)
        _lib.check(_lib.lib().kmm_set_record_regions(self._h, arr, len(regions), int(bool(keep_unplaced))))

    def get_param(self, name):
        v = ctypes.c_int64(0)
        _lib.check(_lib.lib().kmm_get_param(self._h, name.encode(), ctypes.byref(v)))
        return v.value


def extract_kmers(bases, read_offsets, k, lut=None, device=0, out=None):
    """Operator form of util.py:71-75 on the GPU: flat uint64 k-mers in (read, offset) order.
    bases / read_offsets may be numpy arrays or torch tensors (host or device).  With `out` (a
    uint64 numpy array or an int64/uint64 torch tensor of the right length, host or device) the k-mers
    are written there; otherwise a numpy array is returned."""
    b = _Arg(bases, np.uint8, "bases")
    o = _Arg(read_offsets if _is_torch_tensor(read_offsets)
             else np.ascontiguousarray(np.asarray(read_offsets, dtype=np.int64)), np.int64, "read_offsets")
    t = _Arg(lut, np.uint8, "lut")
    if out is None:
        offs = o.keep.cpu().numpy() if _is_torch_tensor(o.keep) else o.keep
        n_out = int(np.maximum(np.diff(offs) - int(k) + 1, 0).sum())
        out = np.empty(n_out, dtype=np.uint64)
    dst = _Arg(out, np.uint64, "out")
    _lib.check(_lib.lib().kmm_extract_kmers(int(device), b.ptr, o.ptr, o.n - 1, int(k), t.ptr, dst.ptr, dst.n))
    return out


def build_index_device(kmers, nodes, modulo, device=0):
    """kmm_build_index on torch DEVICE tensors (kmers int64/uint64 bit patterns, nodes int32), outputs left on the
    device: (hashes_to_index int32[M], n_kmers int32[M], kmers int64[n], nodes int32[n], frequencies uint16[n]).
    For indexes too large to round-trip through host memory quickly (a 10^9-k-mer index is 30 GB of arrays)."""
    import torch
    n, M = kmers.numel(), int(modulo)
    assert kmers.is_cuda and nodes.is_cuda and nodes.dtype == torch.int32 and kmers.element_size() == 8
    dev = kmers.device
    h2i = torch.empty(M, dtype=torch.int32, device=dev)
    nk = torch.empty(M, dtype=torch.int32, device=dev)
    ko = torch.empty(n, dtype=torch.int64, device=dev)
    no = torch.empty(n, dtype=torch.int32, device=dev)
    fo = torch.empty(n, dtype=torch.uint16, device=dev)
    p = lambda t: _P(t.data_ptr())
    _lib.check(_lib.lib().kmm_build_index(int(device), p(kmers), p(nodes), n, M, p(h2i), p(nk), p(ko), p(no), p(fo)))
    return h2i, nk, ko, no, fo


def build_index(kmers, nodes, modulo, device=0):
    """GPU counterpart of graph_kmer_index's KmerIndex.from_flat_kmers (tests/test_mapping.py:36-38):
    returns (hashes_to_index int32[M], n_kmers int32[M], kmers uint64[n], nodes int32[n],
    frequencies uint16[n]) — bit-identical to the stable-sort numpy construction."""
    km = np.ascontiguousarray(np.asarray(kmers, dtype=np.uint64))
    nd_in = np.asarray(nodes)
    if nd_in.size and (nd_in.min() < 0 or nd_in.max() > 2 ** 31 - 1):
        raise ValueError("node ids must fit int32")
    nd = np.ascontiguousarray(nd_in, dtype=np.int32)
    if km.shape != nd.shape or km.ndim != 1:
        raise ValueError("kmers and nodes must be 1-D arrays of the same length")
    M, n = int(modulo), km.shape[0]
    h2i = np.empty(M, dtype=np.int32)
    nk = np.empty(M, dtype=np.int32)
    ko = np.empty(n, dtype=np.uint64)
    no = np.empty(n, dtype=np.int32)
    fo = np.empty(n, dtype=np.uint16)
    p = lambda a: a.ctypes.data_as(_P)
    _lib.check(_lib.lib().kmm_build_index(int(device), p(km), p(nd), n, M, p(h2i), p(nk), p(ko), p(no), p(fo)))
    return h2i, nk, ko, no, fo


def index_from_sequences(bases, seq_offsets, k=31, nodes=None, lut=None, both_strands=False, modulo=0, device=0, info=None,
                         _flags=0):
    """kmm_seq_index_build: sequences -> distinct (k-mer, node) pairs in order of first occurrence -> the five
    index arrays, on the GPU.  bases uint8 flat, seq_offsets int64[n + 1]; nodes int32[n] or None (sequence i is node i);
    modulo 0: the smallest prime >= 2 entries + 1.  Returns (hashes_to_index, n_kmers, kmers, nodes, frequencies, modulo) in
    the order of build_index: numpy arrays for host input, torch tensors on the device of `bases` for a device tensor.
    info: a dict that receives n_entries, modulo, n_windows and n_pairs."""
    L = _lib.lib()
    on_device = _is_torch_tensor(bases) and bases.is_cuda
    b = _Arg(bases, np.uint8, "bases")
    o = _Arg(seq_offsets if _is_torch_tensor(seq_offsets)
             else np.ascontiguousarray(np.asarray(seq_offsets, dtype=np.int64)), np.int64, "seq_offsets")
    if o.n < 1:
        raise ValueError("seq_offsets needs n_seqs + 1 entries (got none)")
    if nodes is not None and not _is_torch_tensor(nodes):
        nd_in = np.asarray(nodes)
        if nd_in.size and (nd_in.min() < -2 ** 31 or nd_in.max() > 2 ** 31 - 1):
            raise ValueError("node ids must fit int32")
        nodes = np.ascontiguousarray(nd_in, dtype=np.int32)
    nd = _Arg(nodes, np.int32, "nodes")
    if nodes is not None and nd.n != o.n - 1:
        raise ValueError("nodes has %d entries for %d sequences" % (nd.n, o.n - 1))
    t = _Arg(lut, np.uint8, "lut")
    if lut is not None and t.n != 256:
        raise ValueError("lut must have 256 entries")
    flags = (_lib.SEQIDX_BOTH_STRANDS if both_strands else 0) | int(_flags)
    h = _P()
    _lib.check(L.kmm_seq_index_build(int(device), b.ptr, o.ptr, o.n - 1, nd.ptr, int(k), t.ptr, flags, int(modulo), ctypes.byref(h)))
    try:
        n, M, nw, npairs = ctypes.c_int64(0), ctypes.c_uint64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(L.kmm_seq_index_info(h, ctypes.byref(n), ctypes.byref(M), ctypes.byref(nw), ctypes.byref(npairs)))
        n, M = n.value, M.value
        if info is not None:
            info.update(n_entries=n, modulo=M, n_windows=nw.value, n_pairs=npairs.value)
        if on_device:
            import torch
            dev = bases.device
            h2i = torch.empty(M, dtype=torch.int32, device=dev)
            nk = torch.empty(M, dtype=torch.int32, device=dev)
            ko = torch.empty(n, dtype=torch.int64, device=dev)
            no = torch.empty(n, dtype=torch.int32, device=dev)
            fo = torch.empty(n, dtype=torch.uint16, device=dev)
            p = lambda x: _P(x.data_ptr()) if x.numel() else None
        else:
            h2i = np.empty(M, dtype=np.int32)
            nk = np.empty(M, dtype=np.int32)
            ko = np.empty(n, dtype=np.uint64)
            no = np.empty(n, dtype=np.int32)
            fo = np.empty(n, dtype=np.uint16)
            p = lambda a: a.ctypes.data_as(_P) if a.size else None
        _lib.check(L.kmm_seq_index_fetch(h, p(h2i), p(nk), p(ko), p(no), p(fo)))
    finally:
        L.kmm_seq_index_destroy(h)
    return h2i, nk, ko, no, fo, M


def seq_index_modulo(n_entries):
    """What modulo=0 chooses for n_entries entries (kmm_seq_index_modulo: pure, needs no GPU)."""
    return int(_lib.lib().kmm_seq_index_modulo(int(n_entries)))
