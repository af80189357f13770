"""Flat reads with their quality bytes as a second array, for kmm_map_reads_qual (include/kmm.h): the cases of
tests/quality_cases.py — which already holds bases, quals and offsets as flat arrays — plus the ones the geometry of
k_mark_low_quals needs: a lane takes 16 positions, two lanes make a 32-position word, a workgroup takes 256 x 16 x 4 = 16384
positions per round, the last vector of a batch is loaded byte-wise, and bit `total` of the bitset is the last mark there is.
Pure numpy, seeded, no GPU; reads drawn from the genome of tests/ambiguous_cases.py, so every masked base shows in the counts.

    CASES / NEW / build(name)     a dict: name, bases, quals, offsets, k, q, qual_base, use_lut (+ what quality_cases gives)
    low_mask(case, q=None)        the bases the floor masks: quals < qual_base + q as unsigned bytes; q = 0: none
    dead_mask(case, q=None)       ... the skip table's breaks included where the case uses the table
    with_n(case, positions)       the case with 'N' at those flat positions and the skip table

tests/test_flat_quality_cases_on_the_cpu.py holds every new case to the condition it exists for.
"""
import numpy as np

from tests import quality_cases as qc
from kmer_mapper_amd.util import ambiguous_skip_lut

L = qc.L
SPAN = 256 * 16 * 4      # positions a workgroup of k_mark_low_quals takes per round
SPAN_EDGES = (0, 15, 16, 31, 32, SPAN - 1, SPAN, 2 * SPAN - 1, 2 * SPAN)
SPAN_PAIR = (3 * SPAN - 16, 3 * SPAN - 16 + qc.K + 1)       # k + 1 apart, one on either side of a workgroup's seam
ODD_TOTALS = {"odd_total-1": 3041, "odd_total-17": 3057, "odd_total-31": 3039, "odd_total-32": 3040}
ABSENT_STRETCH = (40, 90)    # raw_phred-absent: these bases of every sixth read carry 0xFF

NEW = ["span_edges"] + list(ODD_TOTALS) + ["tiny-middle", "tiny-short", "tiny-all_low", "raw_phred", "raw_phred-absent"]
CASES = list(qc.CASES) + NEW
UNIFORM = tuple(qc.UNIFORM) + ("span_edges",)


def low_mask(case, q=None):
    q = case["q"] if q is None else int(q)
    quals = np.asarray(case["quals"], dtype=np.uint8)
    return (quals.astype(np.int64) < case["qual_base"] + q) if q else np.zeros(quals.shape[0], dtype=bool)


def dead_mask(case, q=None):
    m = low_mask(case, q)
    if case["use_lut"]:
        m = m | qc.break_mask(case["bases"], ambiguous_skip_lut())
    return m


def with_n(case, positions):
    bases = np.array(case["bases"])
    bases[np.asarray(positions, dtype=np.int64)] = ord("N")
    bases.setflags(write=False)
    return dict(case, bases=bases, use_lut=True, name=case["name"] + "+N")


def _quals_with_low(total, rng, q, low):
    """'I' everywhere, the floor's own byte (alive) on 3 % of the bases, low bytes at `low` (as quality_cases.build)."""
    quals = np.full(total, max(qc.HIGH, 33 + q), dtype=np.uint8)
    quals[rng.random(total) < 0.03] = 33 + q
    for i, p in enumerate(sorted(set(int(p) for p in low))):
        quals[p] = qc._low_value(q, i)
    return quals


def build(name):
    if name in qc.CASES:
        return dict(qc.build(name), qual_base=33)
    k, q, qual_base = qc.K, 20, 33
    if name == "span_edges":
        # 16383 and 16384 are low themselves, so no window between a pair around THAT seam could survive: the pair k + 1
        # apart straddles the next seam of the same kind that is free, 3 * 16384
        bases, offsets, rng = qc._reads([L] * 400, 41)
        total = 400 * L
        quals = _quals_with_low(total, rng, q, SPAN_EDGES + SPAN_PAIR + (total - 1, total - k))
    elif name in ODD_TOTALS:
        total = ODD_TOTALS[name]
        bases, offsets, rng = qc._reads([L] * 20 + [total - 20 * L], 42 + total % 32)
        quals = _quals_with_low(total, rng, q, (total - 1, 7, 3 * L + 75, 1024))
    elif name == "tiny-middle":
        bases, offsets, rng = qc._reads([k], 51)
        quals = _quals_with_low(k, rng, q, (k // 2,))
    elif name == "tiny-short":           # 15 bases in all: the byte-wise tail alone; k = 12 so that the read holds windows
        k = 12
        bases, offsets, rng = qc._reads([15], 52)
        quals = _quals_with_low(15, rng, q, (0,))
    elif name == "tiny-all_low":
        bases, offsets, rng = qc._reads([k], 53)
        quals = _quals_with_low(k, rng, q, range(k))
    elif name in ("raw_phred", "raw_phred-absent"):
        c = qc.build("all_41_values")
        bases, offsets = c["bases"], c["offsets"]
        quals, qual_base = (c["quals"] - 33).astype(np.uint8), 0
        if name == "raw_phred-absent":   # 0xFF ("absent" in BAM) in stretches, 5.6 % of the bytes: alive at every floor
            q = 93
            for r in range(0, len(offsets) - 1, 6):
                quals[offsets[r] + ABSENT_STRETCH[0]:offsets[r] + ABSENT_STRETCH[1]] = 0xFF
    else:
        raise KeyError(name)
    case = dict(name=name, bases=bases, quals=quals, offsets=offsets, k=k, q=q, qual_base=qual_base, use_lut=False, pins=[], crlf=set())
    for a in (bases, quals, offsets):
        a.setflags(write=False)
    return case
