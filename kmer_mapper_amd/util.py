"""Drop-in for the hot-path half of kmer_mapper/util.py.

get_kmer_hashes_from_chunk_sequence(chunk_sequence, kmer_size) -> np.uint64[n]  (util.py:71-75)

The reference receives a bionumpy EncodedRaggedArray; bionumpy is not a dependency here, so a
chunk is the pair the ragged array is made of: flat ASCII bytes + row offsets (`ReadBatch`).
"""
import numpy as np

from .engine import extract_kmers

LUT_BREAK = 0xFE      # KMM_LUT_BREAK (include/kmm.h): a base that no k-mer may contain
AMBIGUOUS_LETTERS = "NRYKMSWBDHV"   # N and the ten IUPAC ambiguity codes


def default_lut():
    """The table behind lut=None: A C G T -> 0 1 2 3 in both cases, N -> A (command_line_interface.py:41), every other
    byte 0xFF (not a nucleotide)."""
    lut = np.full(256, 0xFF, dtype=np.uint8)
    for code, letter in enumerate("ACGT"):
        lut[ord(letter)] = lut[ord(letter.lower())] = code
    lut[ord("N")] = lut[ord("n")] = 0
    return lut


def ambiguous_skip_lut():
    """The default table with N and the IUPAC ambiguity letters R Y K M S W B D H V, both cases, set to the break code: a
    k-mer that contains one of them is not counted, the windows on either side are (`--ambiguous-bases skip`)."""
    lut = default_lut()
    for letter in AMBIGUOUS_LETTERS:
        lut[ord(letter)] = lut[ord(letter.lower())] = LUT_BREAK
    return lut


def bgzf_compress(data, device=0):
    """kmm_bgzf_compress: the BGZF members of `data` (bytes, a uint8 numpy array or a torch tensor, host or
    device), deflated on the GPU — one member per 65280 bytes, no end-of-file block (gz_io.BGZF_EOF ends a file).  Returns a
    np.uint8 array; the bytes are a pure function of the data."""
    import ctypes
    from . import _lib
    from .engine import _Arg
    if isinstance(data, (bytes, bytearray, memoryview)):
        data = np.frombuffer(data, dtype=np.uint8)
    src = _Arg(data, np.uint8, "data")
    cap = int(_lib.lib().kmm_bgzf_bound(src.n))
    out = np.empty(cap, dtype=np.uint8)
    n_out = ctypes.c_int64(0)
    _lib.check(_lib.lib().kmm_bgzf_compress(int(device), src.ptr, src.n, out.ctypes.data_as(ctypes.c_void_p) if cap else None, cap,
                                            ctypes.byref(n_out)))
    return out[:n_out.value]


class ReadBatch:
    """A chunk of reads: `bases` uint8[sum(len)] (ASCII), `offsets` int64[n_reads+1].

    Stands in for bionumpy's `chunk.sequence` (command_line_interface.py:110,
    util.py:72): flat data + row boundaries, reads in file order."""

    def __init__(self, bases, offsets):
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if self.offsets.ndim != 1 or self.offsets.size < 1 or self.offsets[0] != 0:
            raise ValueError("offsets must be int64[n_reads+1] starting at 0")
        if self.offsets[-1] != self.bases.size:
            raise ValueError("offsets[-1] (%d) != len(bases) (%d)" % (self.offsets[-1], self.bases.size))

    def __len__(self):
        return self.offsets.size - 1

    def n_kmers(self, k):
        """Number of k-mer windows in the batch: sum over reads of max(len - k + 1, 0)."""
        return int(np.maximum(np.diff(self.offsets) - k + 1, 0).sum())

    @property
    def uniform_length(self):
        """Read length if every read has the same length, else None."""
        n = len(self)
        if n == 0:
            return None
        L = int(self.offsets[1])
        if self.offsets[-1] == n * L and (n < 3 or np.array_equal(
                self.offsets, np.arange(n + 1, dtype=np.int64) * L)):
            return L
        return None

    @classmethod
    def from_strings(cls, reads):
        enc = [r.encode() if isinstance(r, str) else bytes(r) for r in reads]
        offsets = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum([len(e) for e in enc], out=offsets[1:])
        return cls(np.frombuffer(b"".join(enc), dtype=np.uint8), offsets)


def as_read_batch(chunk_sequence):
    if isinstance(chunk_sequence, ReadBatch):
        return chunk_sequence
    if isinstance(chunk_sequence, tuple) and len(chunk_sequence) == 2:
        return ReadBatch(*chunk_sequence)
    if isinstance(chunk_sequence, (list,)):
        return ReadBatch.from_strings(chunk_sequence)
    raise TypeError("chunk_sequence must be a ReadBatch, a (bases, offsets) pair or a list of reads")


def get_kmer_hashes_from_chunk_sequence(chunk_sequence, kmer_size, lut=None, device=0):
    batch = as_read_batch(chunk_sequence)
    return extract_kmers(batch.bases, batch.offsets, kmer_size, lut=lut, device=device)


REGION_END_MAX = (1 << 31) - 1     # "to the end of the reference": behind every position a record can have


def _reference_ids(references):
    return None if references is None else {(n.decode() if isinstance(n, bytes) else str(n)): i for i, (n, _) in enumerate(references)}


def _parse_interval(text, spec):
    """`5`, `5-`, `5-9`, commas allowed: 1-based inclusive -> (beg, end) 0-based half-open; None: `text` is no interval."""
    t = text.replace(",", "")
    first, dash, last = t.partition("-")
    if not first.isdigit() or (last and not last.isdigit()):
        return None
    beg = max(int(first) - 1, 0)
    end = int(last) if last else REGION_END_MAX
    if end <= beg:
        raise ValueError("region %r: the end lies before the start" % spec)
    return beg, end


def parse_regions(text_or_list, references=None):
    """Regions in samtools syntax -> ([(ref_name, ref_id, beg, end)], keep_unplaced), 0-based half-open, for
    DeviceIndex.set_record_regions.  `text_or_list`: one string of comma-separated regions — a comma in front of exactly three digits is
    a thousands separator, so a reference named by three digits goes into a list — or a list of region strings.  A region: `chr6:28,000,000-34,000,000` (1-based, inclusive), `chr6:5` or
    `chr6:5-` (from base 5 to the end), a bare reference name (all of it), or `*`: the records without a reference.
    references: the file's [(name, length)] (reads_io.bam_references) — names become ids, an unknown name is an error that names
    it, and a name that itself contains ':' is found as htslib finds it: the whole string is tried as a name first.  None (SAM
    needs no header): the ids are -1, and a string is split at its last ':' when what follows reads as an interval."""
    import re
    if isinstance(text_or_list, (str, bytes)):
        text = text_or_list.decode() if isinstance(text_or_list, bytes) else text_or_list
        specs = [t for t in re.split(r",(?!\d{3}(?:\D|$))", text)]          # (a comma in front of three digits separates thousands)
    else:
        specs = [t.decode() if isinstance(t, bytes) else str(t) for t in text_or_list]
    ids = _reference_ids(references)
    regions, keep_unplaced = [], False
    for spec in (t.strip() for t in specs):
        if not spec:
            raise ValueError("an empty region in %r" % (text_or_list,))
        if spec == "*":
            keep_unplaced = True
            continue
        name, interval = spec, (0, REGION_END_MAX)
        if ids is None or spec not in ids:                                  # (htslib: the whole string as a name first)
            head, colon, tail = spec.rpartition(":")
            got = _parse_interval(tail, spec) if colon and head else None
            if got is not None:
                name, interval = head, got
            elif ids is not None:
                raise ValueError("region %r: the file has no reference named %r" % (spec, spec))
        if ids is not None and name not in ids:
            raise ValueError("region %r: the file has no reference named %r" % (spec, name))
        if name == "*" or len(name.encode()) > 255:
            raise ValueError("region %r: %r cannot be a reference name" % (spec, name))
        regions.append((name, -1 if ids is None else ids[name], interval[0], interval[1]))
    return regions, keep_unplaced


def read_bed_regions(path_or_lines, references=None):
    """The regions of a BED file -> [(ref_name, ref_id, beg, end)]: three columns (more are ignored), 0-based half-open as they
    stand; empty lines and lines that start with '#', 'track' or 'browser' are skipped.  references: as parse_regions."""
    if isinstance(path_or_lines, (str, bytes)):
        with open(path_or_lines, "r") as f:
            lines = f.read().splitlines()
    else:
        lines = [t.decode() if isinstance(t, bytes) else t for t in path_or_lines]
    ids = _reference_ids(references)
    regions = []
    for no, line in enumerate(lines, 1):
        if not line.strip() or line.startswith("#") or line.split()[0] in ("track", "browser"):
            continue
        cols = line.rstrip("\r\n").split("\t") if "\t" in line else line.split()
        if len(cols) < 3 or not cols[1].isdigit() or not cols[2].isdigit():
            raise ValueError("BED line %d: three columns (name, start, end) are needed: %r" % (no, line))
        name, beg, end = cols[0], int(cols[1]), int(cols[2])
        if end <= beg:
            raise ValueError("BED line %d: the end lies at or before the start: %r" % (no, line))
        if ids is not None and name not in ids:
            raise ValueError("BED line %d: the file has no reference named %r" % (no, name))
        regions.append((name, -1 if ids is None else ids[name], beg, end))
    return regions
