"""Reads with ambiguous bases for the break code of the lookup table (KMM_LUT_BREAK, include/kmm.h): a k-mer that contains N
or an IUPAC ambiguity letter is not counted, the windows on either side of it are.  The cases put breaks where the kernels
can go wrong — the edges of the direct tile (1024 positions), of pass 1's half-tile and block (4096, 8192), of the chunk and
of a read — not at the workload's size.  Pure numpy, seeded, no GPU; nothing here reads the library's kernels.

    split_at_breaks(bases, offsets, lut)    the same reads with every break byte dropped and a read boundary where it stood:
                                            what the break code is DEFINED to be equivalent to; the oracle maps those
    surviving_kmers(bases, offsets, k, lut) brute force: the packed k-mers of the windows that hold no break byte
    n_to_a_bytes(bases, lut)                the bytes today's default table can read: every break letter as N (-> A)
    CASES / build(name)                     (name, bases, offsets, k)
    index_for(k)                            the index every case of that k is mapped against
    records_text(bases, offsets, lut, fmt)  the reads as FASTQ / two-line FASTA text, names padded so that one break is the
                                            last byte of a 4 KiB compaction tile and another the first byte of a tile, with
                                            "\\r\\n" lines next to breaks

tests/test_ambiguous_cases_on_the_cpu.py holds every case to the condition it exists for.
"""
import numpy as np

from kmer_mapper_amd import synthetic
from kmer_mapper_amd.kmer_index import KmerIndex
from kmer_mapper_amd.util import LUT_BREAK, ambiguous_skip_lut

K = 31
L = 150
GENOME = synthetic.make_genome(40_000, seed=4401)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
IUPAC = b"RYKMSWBDHV"
N = ord("N")

CASES = ["tile_edges", "read_ends", "run_of_40", "all_n_and_short_reads", "pairs_k_apart", "pairs_k_apart-k12",
         "lower_case_and_iupac", "random_1_percent", "ragged_1_to_400", "k2"]
UNIFORM = ("tile_edges", "read_ends", "run_of_40", "pairs_k_apart", "pairs_k_apart-k12", "lower_case_and_iupac",
           "random_1_percent", "k2")
RANDOM_CASE = "random_1_percent"


# ---------------------------------------------------------------------------------------------- tools of both tiers
def break_mask(bases, lut):
    return np.asarray(lut, dtype=np.uint8)[np.asarray(bases, dtype=np.uint8)] == LUT_BREAK


def split_at_breaks(bases, offsets, lut):
    """(bases', offsets'): the break bytes dropped, a read boundary wherever one stood (empty reads are left out: they hold
    no window)."""
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    brk = break_mask(bases, lut)
    new_pos = np.zeros(bases.shape[0] + 1, dtype=np.int64)      # position of byte p among the kept bytes
    np.cumsum(~brk, out=new_pos[1:])
    bounds = np.concatenate([new_pos[offsets], new_pos[np.flatnonzero(brk) + 1], [0, new_pos[-1]]])
    return np.ascontiguousarray(bases[~brk]), np.unique(bounds).astype(np.int64)


def surviving_windows(bases, offsets, k, lut):
    """Flat start positions of the windows of k bases inside one read that hold no break byte."""
    bases = np.asarray(bases, dtype=np.uint8)
    offsets = np.asarray(offsets, dtype=np.int64)
    total = bases.shape[0]
    before = np.zeros(total + 1, dtype=np.int64)                # break bytes before position p
    np.cumsum(break_mask(bases, lut), out=before[1:])
    read_of = np.repeat(np.arange(offsets.shape[0] - 1), np.diff(offsets))
    p = np.arange(total, dtype=np.int64)
    inside = p + k <= offsets[1:][read_of]
    p = p[inside]
    return p[before[p + k] == before[p]]


def surviving_kmers(bases, offsets, k, lut):
    codes = (np.asarray(lut, dtype=np.uint8)[np.asarray(bases, dtype=np.uint8)] & 3).astype(np.uint8)
    return synthetic.pack_kmers_at(codes, surviving_windows(bases, offsets, k, lut), k)


def n_to_a_bytes(bases, lut):
    out = np.array(bases, dtype=np.uint8)
    out[break_mask(out, lut)] = N
    return out


def code2_bytes(bases, lut):
    """What a library without the break code makes of the table: the entry's low two bits, 0xFE & 3 = 2 = G."""
    out = np.array(bases, dtype=np.uint8)
    out[break_mask(out, lut)] = ord("G")
    return out


def is_uniform(offsets):
    offsets = np.asarray(offsets)
    n = offsets.shape[0] - 1
    return n > 0 and np.array_equal(offsets, np.arange(n + 1, dtype=np.int64) * int(offsets[1]))


def _revcomp(kmers, k):
    """Reverse complements of packed k-mers (first base in the lowest two bits; the complement of code c is 3 - c)."""
    out = np.zeros(kmers.shape[0], dtype=np.uint64)
    for j in range(k):
        out |= (np.uint64(3) - ((kmers >> np.uint64(2 * j)) & np.uint64(3))) << np.uint64(2 * (k - 1 - j))
    return out


_INDEXES = {}


def index_for(k):
    """k >= 8: every k-mer of the genome the reads are drawn from (node = position mod 5000), poly-A (node 5000) and the
    reverse complement of every third one (nodes from 5001).
    Smaller k: each of the 4^k k-mers once (a genome would hold each beyond the frequency filter)."""
    if k not in _INDEXES:
        if k < 8:
            kmers = np.arange(4 ** k, dtype=np.uint64)
            nodes = np.arange(4 ** k, dtype=np.int64)
        else:
            n = GENOME.shape[0] - k + 1
            fwd = synthetic.pack_kmers_strided(GENOME, n, 1, k)
            rev = _revcomp(fwd[::3], k)          # (so that mapping with reverse complements counts something else)
            kmers = np.concatenate([fwd, np.zeros(1, dtype=np.uint64), rev])
            nodes = np.concatenate([np.arange(n, dtype=np.int64) % 5000, [5000], 5001 + np.arange(rev.shape[0], dtype=np.int64) % 1000])
        _INDEXES[k] = KmerIndex.from_flat_kmers(kmers, nodes, synthetic.next_prime(2 * kmers.shape[0]))
    return _INDEXES[k]


# ---------------------------------------------------------------------------------------------- the cases
class _Reads:
    """Reads drawn from the genome without errors.  put(read, offset, letter) writes a break there and first moves the
    read along the genome until the base it replaces is an A: every window over it then hits the index when N is read
    as A, and none does when the windows are skipped — the difference the case exists for.  Every second read is moved to
    a G instead: a library that knows no break code reads the entry 0xFE as code 2 (its low two bits), and its counts
    must differ as well."""

    def __init__(self, lengths, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.lengths = np.asarray(lengths, dtype=np.int64)
        self.offsets = np.zeros(self.lengths.shape[0] + 1, dtype=np.int64)
        np.cumsum(self.lengths, out=self.offsets[1:])
        self.starts = self.rng.integers(0, GENOME.shape[0] - 2 * int(self.lengths.max()) - 64, size=self.lengths.shape[0])
        self.marks = []                                          # (read, offset, letter)
        self.pinned = set()

    def put(self, read, offset, letter=N):
        read, offset = int(read), int(offset)
        assert 0 <= offset < self.lengths[read]
        if read not in self.pinned:
            want = 0 if len(self.pinned) % 2 == 0 else 2         # A, G, A, ... (the reads in the order they are first marked)
            while GENOME[self.starts[read] + offset] != want:
                self.starts[read] += 1
            self.pinned.add(read)
        self.marks.append((read, offset, letter))

    def put_flat(self, p, letter=N):
        p = int(p)
        read = int(np.searchsorted(self.offsets, p, side="right") - 1)
        self.put(read, p - self.offsets[read], letter)

    def finish(self, lower_every=0):
        bases = np.empty(int(self.offsets[-1]), dtype=np.uint8)
        for r, (s, n) in enumerate(zip(self.starts, self.lengths)):
            row = ACGT[GENOME[s:s + n]]
            if lower_every and r % lower_every == 1:
                row = row | 0x20
            bases[self.offsets[r]:self.offsets[r + 1]] = row
        for r, o, letter in self.marks:
            bases[self.offsets[r] + o] = letter
        return bases, self.offsets.copy()


def build(name):
    """(name, bases, offsets, k)"""
    k = 12 if name.endswith("-k12") else 2 if name == "k2" else K
    if name == "tile_edges":             # the direct tile's T = 256 * 4, pass 1's half-tile and block, the chunk's ends
        r = _Reads([L] * 400, 11)
        total = 400 * L
        for p in (0, 30, 31, 32, 1023, 1024, 4095, 4096, 8191, 8192, total - 1, total - k):
            r.put_flat(p)
    elif name == "read_ends":            # the first and the last base of a read, and both
        r = _Reads([L] * 300, 12)
        for read in (3, 50, 27):
            r.put(read, 0)
        for read in (7, 120, 54):
            r.put(read, L - 1)
        r.put(200, 0)
        r.put(200, L - 1)
        r.put(299, L - 1)
        r.put(0, 0)
    elif name == "run_of_40":
        r = _Reads([L] * 300, 13)
        for o in range(50, 90):
            r.put(10, o)
        for p in range(4080, 4120):      # across pass 1's half-tile
            r.put_flat(p)
        for o in range(L - 40, L):       # a tail of 40 N: ten poly-A 31-mers when N is read as A
            r.put(150, o)
    elif name == "all_n_and_short_reads":
        lengths = [L] * 200
        lengths[20], lengths[21], lengths[22], lengths[120] = 20, 1, k - 1, k
        r = _Reads(lengths, 14)
        for o in range(L):
            r.put(5, o)                  # a read that is all N
        r.put(20, 7)                     # shorter than k, with an N
        r.put(21, 0)                     # a read that is one N
        r.put(120, k // 2)               # exactly one window, killed
        r.put(60, 75)
    elif name.startswith("pairs_k_apart"):
        r = _Reads([L] * 200, 15)
        for read in (4, 30, 100):        # k + 1 apart: exactly one window survives between them
            r.put(read, 40)
            r.put(read, 40 + k + 1)
        for read in (9, 27, 150):        # k apart: none does
            r.put(read, 60)
            r.put(read, 60 + k)
        r.put(27, 45)                    # (flat 4095 = read 27, offset 45)
        r.put(27, 46)
    elif name == "lower_case_and_iupac":
        r = _Reads([L] * 200, 16)
        letters = list(IUPAC + IUPAC.lower() + b"Nn")
        for i, letter in enumerate(letters):
            r.put(1 + 9 * i, 35 + 4 * i, letter)
    elif name == RANDOM_CASE:
        r = _Reads([L] * 400, 17)
        for p in np.flatnonzero(r.rng.random(400 * L) < 0.01):
            r.marks.append((int(p // L), int(p % L), N))
    elif name == "ragged_1_to_400":
        rng = np.random.Generator(np.random.PCG64(18))
        r = _Reads(rng.integers(1, 401, size=260), 18)
        total = int(r.offsets[-1])
        for p in np.flatnonzero(rng.random(total) < 0.004):
            r.put_flat(p, int(rng.choice(list(IUPAC + b"N"))))
        for p in (0, 1023, 1024, 4095, 4096, 8191, 8192, total - 1):
            r.put_flat(p)
    elif name == "k2":                   # the smallest k the bitset rule can express: neighbours, ends, pairs
        r = _Reads([L] * 200, 19)
        for read, o in ((0, 0), (0, 1), (0, 3), (6, 149), (6, 147), (6, 148), (27, 45), (27, 46), (54, 91), (100, 75)):
            r.put(read, o)
    else:
        raise KeyError(name)
    bases, offsets = r.finish(lower_every=7 if name in ("lower_case_and_iupac", "ragged_1_to_400") else 0)
    return name, bases, offsets, k


# ---------------------------------------------------------------------------------------------- the same reads as text
TILE = 4096       # bytes per tile of the records compaction kernels (REC_TB)


def records_text(bases, offsets, lut, fmt):
    """The reads as FASTQ (fmt 4) or two-line FASTA (fmt 2) bytes.  Returns (text, last, first): `last` / `first` are the
    byte offsets of a break that is the last byte of a 4 KiB tile / the first byte of one (None where the case has no read
    to spare for it).  Every second read that holds a break, the reads that start or end with one, and every fifth read
    have "\\r\\n" line ends."""
    bases = np.asarray(bases, dtype=np.uint8)
    brk = break_mask(bases, lut)
    n = len(offsets) - 1
    with_break = [i for i in range(n) if brk[offsets[i]:offsets[i + 1]].any()]
    target = {}
    if len(with_break) >= 3:
        target[with_break[len(with_break) // 3]] = TILE - 1
        target[with_break[2 * len(with_break) // 3]] = 0
    crlf = set(with_break[::2])
    out, pos, where = [], 0, {}
    for i in range(n):
        seq = bases[offsets[i]:offsets[i + 1]].tobytes()
        b = brk[offsets[i]:offsets[i + 1]]
        nl = b"\r\n" if (i % 5 == 2 or i in crlf or (len(seq) and (b[0] or b[-1]))) else b"\n"
        head = (b"@" if fmt == 4 else b">") + b"r%d" % i
        if i in target:
            o = int(np.flatnonzero(b)[0])
            pad = (target[i] - (pos + len(head) + len(nl) + o)) % TILE
            head += b" " + b"x" * (pad - 1) if pad else b""
            where[target[i]] = pos + len(head) + len(nl) + o
        rec = head + nl + seq + nl
        if fmt == 4:
            rec += b"+" + nl + b"I" * len(seq) + nl
        out.append(rec)
        pos += len(rec)
    return b"".join(out), where.get(TILE - 1), where.get(0)
