"""Catalogue of cases for the record-keep mode (include/kmm.h): raw FASTQ / two-line FASTA text whose kept
records' bytes come back, compacted.

A case is a text + index + k of tests/record_hits_cases.py (imported unchanged, with its parser and hit model) and one keep
rule.  Expected values never come from the library: the model is the per-record (hits, windows) of that catalogue, then
keep_rule, then b"".join of the kept records' bytes, cut out of the text by record_spans.  tests/test_record_keep_on_the_cpu.py
holds the model to a second route and to the conditions that keep the catalogue from being vacuous.

The scatter's seams: a lane takes 16 bytes of the text, a tile 1024, a workgroup four tiles, a super-tile 1 MiB; the output
leaves as aligned 16-byte lines with a ragged head and tail per workgroup.
"""
from collections import namedtuple

import numpy as np

from tests import read_hits_cases as rc
from tests import record_hits_cases as rh

KCase = namedtuple("KCase", "name base min_hits min_permille invert")
LINE, TILE, SUPER = 16, rh.TILE, rh.SUPER


# ------------------------------------------------------------------------------------------------ the model
def record_spans(text, fmt):
    """[(start, end)] of the whole records of `text`: from the first byte of the header line to behind the '\\n' of the last."""
    ends = np.nonzero(np.frombuffer(bytes(text), dtype=np.uint8) == 10)[0][rh.PERIOD[fmt] - 1::rh.PERIOD[fmt]] + 1
    starts = np.concatenate([[0], ends[:-1]])
    return [(int(a), int(b)) for a, b in zip(starts, ends)]


def keep_rule(hits, windows, min_hits=1, min_permille=0, invert=False):
    """The keep rule of include/kmm.h over arrays of entries, in Python integers (no width to overflow)."""
    out = np.zeros(len(hits), dtype=bool)
    for i, (h, w) in enumerate(zip(hits.tolist(), windows.tolist())):
        match = h >= min_hits and 1000 * h >= min_permille * w
        out[i] = match != bool(invert)
    return out


_EXPECT = {}


def expected(case):
    """(kept text as bytes, n_kept, keep mask, hits, windows, consumed, n_records) of the case, computed once (read-only)."""
    if case.name not in _EXPECT:
        hits, windows, consumed, n_records = rh.expected(case.base)
        keep = keep_rule(hits, windows, case.min_hits, case.min_permille, case.invert)
        raw = case.base.text.tobytes()
        spans = record_spans(raw[:consumed], case.base.fmt)
        assert len(spans) == n_records
        text = b"".join(raw[a:b] for (a, b), kp in zip(spans, keep) if kp)
        keep.setflags(write=False)
        _EXPECT[case.name] = (text, int(keep.sum()), keep, hits, windows, consumed, n_records)
    return _EXPECT[case.name]


# ------------------------------------------------------------------------------------------------ texts chosen for the scatter
K = 31


def hit_read(n, at):
    return rc.gslice(at % 15_000, n).tobytes()


def miss_read(n):
    return b"T" * n                                                   # (no window of it is in genome_index(31))


def _padded(fmt, seq, total, seed):
    """A record of exactly `total` bytes: the header takes what the other lines leave."""
    bare = len(rh.record(fmt, seq, b"", seed=seed))
    assert total >= bare, (total, bare)
    rec = rh.record(fmt, seq, b"p" * (total - bare), seed=seed)
    assert len(rec) == total
    return rec


def output_residue_text():
    """Two-line FASTA, records alternately kept and dropped; the kept ones end at 15, 16 and 17 modulo 16 of the OUTPUT, three
    times over; the dropped ones have lengths that move the input out of step with the output."""
    parts, out_len = [], 0
    for i, residue in enumerate((15, 16, 17) * 3):
        n = 40 + i
        bare = len(rh.record(rh.FASTA, hit_read(n, 100 * i), b""))
        total = bare + (residue - (out_len + bare)) % LINE
        parts.append(_padded(rh.FASTA, hit_read(n, 100 * i), total, i))
        out_len += total
        assert out_len % LINE == residue % LINE
        parts.append(rh.record(rh.FASTA, miss_read(35 + 3 * i), b"d%d" % i))
    return b"".join(parts)


def tile_end_text():
    """FASTQ, records alternately dropped and kept; kept records end (the byte behind their last '\\n') one byte before, at and
    one byte behind a 1024-byte tile boundary of the INPUT."""
    parts, at = [], 0
    for i, d in enumerate((-1, 0, 1)):
        drop = rh.record(rh.FASTQ, miss_read(50 + i), b"d%d" % i, seed=i)
        parts.append(drop)
        at += len(drop)
        seq = hit_read(120 + i, 700 * i)
        bare = len(rh.record(rh.FASTQ, seq, b"", seed=i))
        end = -(-(at + bare + 1) // TILE) * TILE + d
        parts.append(_padded(rh.FASTQ, seq, end - at, i))
        at = end
    parts.append(rh.record(rh.FASTQ, miss_read(60), b"last", seed=9))
    return b"".join(parts)


def order_texts():
    hit = [hit_read(70 + i, 300 * i) for i in range(4)]
    miss = [miss_read(60 + i) for i in range(4)]
    return {"first_and_last_dropped": rh.text_of(rh.FASTQ, [miss[0], hit[0], miss[1], hit[1], miss[2]]),
            "only_the_last_kept": rh.text_of(rh.FASTA, [miss[0], miss[1], miss[2], hit[0]]),
            "first_kept_last_dropped": rh.text_of(rh.FASTA, [hit[0], hit[1], miss[0]])}


def permille_text():
    """Two records with the same hits and different windows: the second has 60 bases without a hit behind the same 60 bases."""
    a = hit_read(60, 2000)
    return rh.text_of(rh.FASTQ, [a, a + miss_read(60), miss_read(80)])


def _new_bases():
    g = rc.genome_index(K)
    out = [rh.make("rk_output_residues_fasta_k31", g, K, rh.FASTA, output_residue_text()),
           rh.make("rk_tile_ends_fastq_k31", g, K, rh.FASTQ, tile_end_text()),
           rh.make("rk_permille_fastq_k31", g, K, rh.FASTQ, permille_text()),
           rh.make("rk_single_short_record_k1", rc.genome_index(1), 1, rh.FASTA, b">\nA\n"),
           rh.make("rk_short_records_k1", rc.genome_index(1), 1, rh.FASTA, b">\n\n>\nC\n>\nA\n")]
    for name, text in order_texts().items():
        fmt = rh.FASTQ if text[:1] == b"@" else rh.FASTA
        out.append(rh.make("rk_%s_%s_k31" % (name, fmt), g, K, fmt, text))
    return out


_ALL = None


def all_cases():
    global _ALL
    if _ALL is not None:
        return _ALL
    out = []
    bases = {c.name: c for c in rh.all_cases() + _new_bases()}
    for name, base in bases.items():                                 # every text under the default rule
        out.append(KCase(name + "__default", base, 1, 0, False))
    top = lambda name: int(rh.expected(bases[name])[0].max())
    for name in ("short_and_empty_fastq_k16", "rk_output_residues_fasta_k31", "crlf_fasta_k16"):
        out.append(KCase(name + "__min_hits_0", bases[name], 0, 0, False))                       # all kept
        out.append(KCase(name + "__above_the_largest", bases[name], top(name) + 1, 0, False))    # none kept
        out.append(KCase(name + "__invert", bases[name], 1, 0, True))
    # (genome_index(1) holds C alone: ">\nA\n" is kept as a record without a hit)
    out.append(KCase("rk_single_short_record_k1__invert", bases["rk_single_short_record_k1"], 1, 0, True))
    out.append(KCase("rk_tile_ends_fastq_k31__invert", bases["rk_tile_ends_fastq_k31"], 1, 0, True))
    out.append(KCase("rk_permille_fastq_k31__permille_200", bases["rk_permille_fastq_k31"], 1, 200, False))
    out.append(KCase("rk_permille_fastq_k31__permille_200_invert", bases["rk_permille_fastq_k31"], 1, 200, True))
    out.append(KCase("breaks_fastq_k16__min_hits_0", bases["breaks_fastq_k16"], 0, 0, False))
    out.append(KCase("short_and_empty_fastq_k16__permille_1000", bases["short_and_empty_fastq_k16"], 0, 1000, False))
    # the record across the super-tile seam kept, its neighbours (fewer windows, so fewer hits) dropped
    big = bases["super_tile_fastq_k31"]
    out.append(KCase("super_tile_fastq_k31__seam_record", big, int(rh.expected(big)[0][seam_record(big)]), 0, False))
    out.append(KCase("super_tile_fastq_k31__invert", big, 1, 0, True))
    _ALL = out
    return _ALL


def seam_record(case):
    """The record of `case` that holds byte SUPER (the first byte of the second super-tile)."""
    spans = record_spans(case.text.tobytes(), case.fmt)
    return next(i for i, (a, b) in enumerate(spans) if a < SUPER < b)
