"""Catalogue of cases for keeping the mates of a name-collated BAM file together (include/kmm.h "record_names_pairs"; DESIGN
4.23): BAM files whose selected records are mates in file order, 2p and 2p + 1, whose kept pairs come back as interleaved FASTQ.

Nothing here reads the library.  The model is the chain of two models the test tree already has, and a restated name check:
    bam_fastq_cases.decoded      the text of the selected records (its own BAM reader; selection, names, suffix, strand, qualities)
    record_pairs_cases.expected  that text as interleaved FASTQ: lines split at '\\n', the numpy hit model, the pair rule in integers
    first_stranger               the mate check: the name lines 8p and 8p + 4 behind '@', a trailing "/1" or "/2" left out with the
                                 suffix on; equal means equal length and equal bytes
A case that is no error case expects the kept pairs' bytes and one entry per record in pair order; an error case expects the call
that completes the offending pair to fail — `window_of` says which one.  tests/test_bam_pairs_on_the_cpu.py holds the catalogue
to the conditions that keep it from being vacuous.

Windows: a case's stream is cut at inflated offsets (`cuts`, relative to the payload); every window ends at a member boundary, so
a call consumes its whole window and what it carries is what the cut leaves: the bytes of an incomplete record (the stream's
carry) and, with an odd number of selected records complete so far, the text of a mate 1 (the text carry of DESIGN 4.23).

The length of a pair's text is even — both names are equally long, or differ by a two-byte suffix — so the kept span ends at even
residues of the 16-byte output lines only: the catalogue places them at 14, 0 and 2 (the issue's 15, 16 and 17 cannot occur at the
end of a pair; inside the span every residue occurs, as the scatter groups cut it every 4096 input bytes)."""
from collections import namedtuple

from tests import bam_fastq_cases as bc
from tests import record_hits_cases as rh
from tests import record_pairs_cases as rp
from tests import select_cases as sc

K = bc.K
TILE = bc.TILE
LONG = 39_770
F1, F2 = 0x4D, 0x8D                                                   # paired, unmapped, mate unmapped, first / last
X900 = sc.NO_SEL._replace(excl=0x900)

# base: bam_fastq_cases.Base; cuts: inflated payload offsets where windows end (None: one window); error: None, ("strangers", p)
# or ("unpaired", n_selected); piece_kb: the case is ALSO run under "debug_records_piece_kb" (0: its pairs do not fit one)
PCase = namedtuple("PCase", "name base cuts min_hits min_permille invert pair_rule error piece_kb")


# ------------------------------------------------------------------------------------------------ the model
def name_of_record(text, suffix):
    """What the mate check compares of a record's text: the name line behind '@', without a trailing /1 or /2 with the suffix on."""
    line = text[1:text.index(b"\n")]
    if suffix and len(line) >= 2 and line[-2:] in (b"/1", b"/2"):
        line = line[:-2]
    return line


def first_stranger(texts, suffix):
    """The first pair p whose records 2p and 2p + 1 are no mates (None: all are)."""
    for p in range(len(texts) // 2):
        if name_of_record(texts[2 * p], suffix) != name_of_record(texts[2 * p + 1], suffix):
            return p
    return None


def error_of(base):
    """What a stream of `base` has to fail with: strangers come first (they lie in front of an unpaired end)."""
    d = bc.decoded(base)
    p = first_stranger(d.texts, base.suffix)
    if p is not None:
        return ("strangers", p)
    if len(d.texts) % 2:
        return ("unpaired", len(d.texts))
    return None


def pairs_case(case):
    """The case as tests/record_pairs_cases.py takes it: the decoded text as interleaved FASTQ."""
    return rp._mk("bam_pairs_" + case.name, rh.FASTQ, bc.decoded(case.base).text, min_hits=case.min_hits, min_permille=case.min_permille,
                  invert=case.invert, pair_rule=case.pair_rule)


def expected(case):
    """record_pairs_cases.Expect of the case: text1 the kept bytes, n_kept PAIRS, keep per pair, hits / windows per record."""
    assert case.error is None
    e = rp.expected(pairs_case(case))
    d = bc.decoded(case.base)
    assert e.consumed1 == len(d.text) and 2 * e.n_pairs == len(d.records)
    return e


def window_ends(case):
    """The inflated payload offsets at which the case's windows end, the last one the payload's end."""
    _, _, hdr = bc.read_bam(case.base.payload)
    size = len(case.base.payload) - hdr
    cuts = sorted(set(c for c in (case.cuts or ()) if 0 < c < size))
    return cuts + [size]


def selected_done(case):
    """Per window: the selected records complete at its end, counted from the stream's start."""
    _, recs, hdr = bc.read_bam(case.base.payload)
    ends = [r.start + r.size - hdr for r in recs if bc.selected(r, case.base.sel)]
    return [sum(1 for e in ends if e <= w) for w in window_ends(case)]


def window_of(case):
    """The window whose call has to fail: the one that completes mate 2 of the strangers; the last one for an unpaired end."""
    done = selected_done(case)
    if case.error[0] == "unpaired":
        return len(done) - 1
    return next(i for i, n in enumerate(done) if n >= 2 * case.error[1] + 2)


def boundary_kinds(case):
    """Per window end that lies inside a record: (which mate holds it — 1, 2, or 0 for a record not selected —, 'head' / 'name' /
    'seq' / 'qual', text carry non-empty, selected records completed by this window)."""
    _, recs, hdr = bc.read_bam(case.base.payload)
    done = selected_done(case)
    out = []
    for i, w in enumerate(window_ends(case)[:-1]):
        at = w + hdr
        inside = [r for r in recs if r.start < at < r.start + r.size]
        new = done[i] - (done[i - 1] if i else 0)
        if not inside:
            out.append((None, "between", done[i] % 2 == 1, new))
            continue
        r = inside[0]
        off = at - r.start
        name_end = 36 + len(r.name) + 1
        qual_at = name_end + 4 * len(r.cigar) + (len(r.seq) + 1) // 2
        kind = "head" if off < 36 else "name" if off < name_end else "seq" if off < qual_at else "qual"
        mate = 0 if not bc.selected(r, case.base.sel) else 1 + done[i] % 2
        out.append((mate, kind, done[i] % 2 == 1, new))
    return out


def windowed_file(case, block=301, level=6):
    """(the BAM file's bytes, [(start, end)] of the windows in them): the header's member goes with the first window, every
    window's payload in members of at most `block` inflated bytes, the end-of-file block with the last."""
    from kmer_mapper_amd import reads_io
    payload = case.base.payload
    _, _, hdr = bc.read_bam(payload)
    parts, windows, at, lo = [reads_io.bgzf_members(payload[:hdr], 0xFF00, level)], [], 0, 0
    ends = window_ends(case)
    for i, w in enumerate(ends):
        parts.append(reads_io.bgzf_members(payload[hdr + lo:hdr + w], block, level))
        if i == len(ends) - 1:
            parts.append(reads_io.BGZF_EOF)
        size = sum(len(p) for p in parts)
        windows.append((at, size))
        at, lo = size, w
    return b"".join(parts), windows


# ------------------------------------------------------------------------------------------------ writing pairs
def mates(seq1, seq2, name, flags=(F1, F2), name2=None, **kw):
    return [bc._rec(seq1, name, flags[0], **kw), bc._rec(seq2, name if name2 is None else name2, flags[1], **kw)]


def _base(name, records, sel=X900, orig=False, suffix=False):
    return bc.Base("pairs_" + name, bc._payload([r for pair in records for r in (pair if isinstance(pair, list) else [pair])]), sel,
                   orig, suffix, False)


def pattern_records(tag=b"p"):
    """Mate 1 only, mate 2 only, both, neither, and the first once more; mates of different lengths."""
    h, m = bc.hit, bc.miss
    shapes = [(h(100, 0), m(90, 1)), (m(80, 2), h(120, 500)), (h(70, 900), h(75, 1300)), (m(60, 3), m(65, 4)), (h(150, 2000), m(100, 5))]
    return [mates(a, b, tag + b"%d" % i) for i, (a, b) in enumerate(shapes)]


def permille_records():
    """a: a genome slice; b = a + 60 bases without a hit: the same hits over three times the windows — 150 per mille lies between."""
    a = bc.hit(60, 2000)
    b = a + bc.miss(60, 11)
    shapes = [(a, b), (b, a), (a, a), (b, b), (bc.miss(80, 12), bc.miss(70, 13))]
    return [mates(x, y, b"pm%d" % i) for i, (x, y) in enumerate(shapes)]


NAME_LENGTHS = (1, 63, 64, 65, 254)
# stored differently, equal once the bytes outside '!' .. '~' are written as '?'
REPLACED = ((b"tab\there", b"tab here"), (b"hi\x80gh\xff", b"hi\x7fgh\x01"))


def names_records():
    recs = []
    for i, n in enumerate(NAME_LENGTHS):
        recs.append(mates(bc.hit(70 + i, 300 * i), bc.miss(60 + i, 20 + i), bc.name_of(n, n)))
        recs.append(mates(bc.miss(71 + i, 30 + i), bc.miss(61 + i, 40 + i), bc.name_of(n, n + 1)))
    for i, (n1, n2) in enumerate(REPLACED):
        recs.append(mates(bc.miss(50 + i, 50 + i), bc.hit(80 + i, 700 * i), n1, name2=n2))
        recs.append(mates(bc.miss(52 + i, 52 + i), bc.miss(82 + i, 54 + i), n2, name2=n1))
    return recs


def suffix_records():
    """0x40 / 0x80 in both stored orders, neither bit, and the edge of include/kmm.h: a QNAME that itself ends in /1 or /2 while
    FLAG carries no mate bit is trimmed like a written suffix."""
    recs = []
    for i, flags in enumerate(((0x41, 0x81), (0x81, 0x41), (0x1, 0x1), (0xC1, 0xC1))):
        recs.append(mates(bc.hit(64 + i, 400 * i), bc.miss(66 + i, 60 + i), b"sfx%d" % i, flags))
        recs.append(mates(bc.miss(65 + i, 64 + i), bc.miss(67 + i, 68 + i), b"sfd%d" % i, flags))
    recs.append(mates(bc.hit(90, 100), bc.miss(91, 72), b"own/1", (0x1, 0x1), name2=b"own/2"))
    recs.append(mates(bc.miss(92, 73), bc.miss(93, 74), b"own", (0x1, 0x1), name2=b"own/2"))
    return recs


def strand_records():
    """A mate stored reverse-complemented (FLAG 0x10): with original_strand the text is the read's, and it hits as such."""
    h = bc.hit(110, 1234)
    return [mates(bc.miss(100, 80), h, b"fwd"),
            [bc._rec(bc.miss(100, 81), b"flip2", F1), bc._rec(bc.revcomp(h), b"flip2", F2 | 0x10)],
            [bc._rec(bc.revcomp(bc.hit(95, 4000)), b"flip1", F1 | 0x10), bc._rec(bc.miss(90, 82), b"flip1", F2)],
            [bc._rec(bc.revcomp(bc.miss(95, 83)), b"flipd", F1 | 0x10), bc._rec(bc.miss(90, 84), b"flipd", F2 | 0x10)]]


def lengths_records():
    """l_seq 0, 1 and 39 770 as either mate, each in a kept and in a dropped pair; absent qualities."""
    recs = []
    for i, n in enumerate((0, 1)):
        short = b"ACGT"[:n]
        recs.append(mates(short, bc.hit(80 + i, 100 * i), b"s%d_first_kept" % n))
        recs.append(mates(short, bc.miss(81 + i, 90 + i), b"s%d_first_dropped" % n))
        recs.append(mates(bc.hit(82 + i, 600 + i), short, b"s%d_second_kept" % n))
        recs.append(mates(bc.miss(83 + i, 92 + i), short, b"s%d_second_dropped" % n))
    recs.append(mates(b"", b"", b"both_empty"))
    recs.append(mates(bc.hit(LONG, 9), bc.miss(70, 94), b"long_first_kept"))
    recs.append(mates(bc.miss(LONG, 95), bc.miss(71, 96), b"long_first_dropped"))
    recs.append(mates(bc.miss(72, 97), bc.hit(LONG, 3000), b"long_second_kept"))
    recs.append(mates(bc.miss(73, 98), bc.miss(LONG, 99), b"long_second_dropped"))
    recs.append([bc._rec(bc.hit(88, 5000), b"noqual_kept", F1, qual=None), bc._rec(bc.miss(77, 100), b"noqual_kept", F2, qual=None)])
    recs.append([bc._rec(bc.miss(89, 101), b"noqual_dropped", F1, qual=None), bc._rec(bc.miss(78, 102), b"noqual_dropped", F2)])
    return recs


def excluded_records():
    """Secondary and supplementary records between two mates and between two pairs: the selection (0x900) takes them out."""
    recs = []
    for i in range(4):
        a, b = (bc.hit(75 + i, 800 * i), bc.miss(70 + i, 110 + i)) if i % 2 == 0 else (bc.miss(76 + i, 120 + i), bc.miss(71 + i, 130 + i))
        name = b"ex%d" % i
        recs.append([bc._rec(a, name, F1), bc._rec(bc.hit(40, 50 * i), name, 0x800 | 0x41), bc._rec(bc.hit(41, 60 * i), name, 0x100 | 0x41),
                     bc._rec(b, name, F2), bc._rec(bc.hit(42, 70 * i), name, 0x900 | 0x81)])
    return recs


def _filler_to(parts, at, goal):
    """An excluded record (0x900 is set on it) that ends where `goal` says."""
    bare = len(bc._rec(bc.miss(40, 900), b"fill", 0x800))
    assert goal - at >= bare, (goal, at, bare)
    parts.append(bc._rec(bc.miss(40, 900), b"fill", 0x800, aux=b"Z" * (goal - at - bare)))


def straddle_base():
    """Pairs astride a 16 KiB boundary of the inflated stream: the boundary inside mate 1, between the mates, and inside mate 2, each
    once kept and once dropped; excluded fillers put them there."""
    from kmer_mapper_amd import reads_io
    parts = [reads_io.bam_header((), b"@HD\tVN:1.6\tSO:unsorted\tGO:query\n")]
    at, m, marks = len(parts[0]), 1, []
    for kind in ("mate1", "between", "mate2"):
        for j in range(2):
            a, b = (bc.hit(150, 700 * m), bc.miss(140, 140 + m)) if j == 0 else (bc.miss(150, 150 + m), bc.miss(140, 160 + m))
            pair = mates(a, b, b"%s_%d" % (kind.encode(), j))
            inside = {"mate1": 100, "between": len(pair[0]), "mate2": len(pair[0]) + 90}[kind]
            goal = m * TILE - inside
            _filler_to(parts, at, goal)
            parts.extend(pair)
            marks.append((kind, goal, len(pair[0]), len(pair[1])))
            at = goal + len(pair[0]) + len(pair[1])
            m += 1
    return bc.Base("pairs_straddle", b"".join(parts), X900, False, False, False), marks


def residue_records():
    """Kept (hit, hit) and dropped (miss, miss) pairs in turn; the kept text ends 14, 0 and 2 bytes into a 16-byte line, three times."""
    recs, out_len = [], 0
    for i, residue in enumerate((14, 16, 18) * 3):
        a, b = bc.hit(40 + i, 100 * i), bc.hit(47 + 2 * i, 100 * i + 50)
        bare = 2 * len(a) + 2 * len(b) + 12
        pad = ((residue - (out_len + bare)) % 16) // 2 or 8               # bytes of name, each counted twice
        recs.append(mates(a, b, b"k" * pad))
        out_len += bare + 2 * pad
        assert out_len % 16 == residue % 16
        recs.append(mates(bc.miss(35 + 3 * i, 170 + i), bc.miss(36 + 3 * i, 180 + i), b"d%d" % i))
    return recs


def window_records():
    """Twenty pairs of about 300 bytes, kept and dropped in turn, names of 12 to 31 bytes."""
    recs = []
    for i in range(20):
        a = bc.hit(60 + i, 350 * i) if i % 2 == 0 else bc.miss(60 + i, 200 + i)
        b = bc.hit(50 + i, 350 * i + 80) if i % 4 == 0 else bc.miss(50 + i, 230 + i)
        recs.append(mates(a, b, bc.name_of(12 + i, i)))
    return recs


def carry_base():
    """(base, cuts): mate 1 of pair 1 ends a window; the next window holds two excluded records and nothing else; the next one the
    first 50 bytes of mate 2 (no complete record); the next one the rest.  The text carry lives through both."""
    pairs = pattern_records(b"c")
    extra = [bc._rec(bc.hit(45, 10), b"c1", 0x800 | 0x41), bc._rec(bc.hit(46, 20), b"c1", 0x100 | 0x81)]
    records = pairs[0] + [pairs[1][0]] + extra + [pairs[1][1]] + [r for p in pairs[2:] for r in p]
    base = bc.Base("pairs_carry", bc._payload(records), X900, False, False, False)
    a = len(pairs[0][0]) + len(pairs[0][1]) + len(pairs[1][0])
    b = a + len(extra[0]) + len(extra[1])
    return base, [a, b, b + 50]


# ------------------------------------------------------------------------------------------------ strangers, unpaired ends
def _renamed(records, p, mate, name):
    """`records` (pairs) with the name of one mate of pair p replaced."""
    _, recs, _ = bc.read_bam(bc._payload(records[p]))
    r = recs[mate]
    out = [list(pair) for pair in records]
    out[p][mate] = bc._rec(r.seq, name, r.flag)
    return out


def stranger_bases():
    """{name: (base, cuts)} — names that differ in the last byte, in the first byte and in length only, at pair 0, in the middle, at
    the pair astride the text carry and in the last pair; a coordinate-sorted toy; a trio with 0x900 not excluded."""
    w = window_records()
    name = lambda p: bc.name_of(12 + p, p)
    out = {}
    out["last_byte_at_pair_0"] = (_base("strangers_last_byte", _renamed(w, 0, 1, name(0)[:-1] + b"~")), None)
    out["first_byte_in_the_middle"] = (_base("strangers_first_byte", _renamed(w, 9, 0, b"~" + name(9)[1:])), None)
    out["prefix_in_the_last_pair"] = (_base("strangers_prefix", _renamed(w, 19, 1, name(19)[:-1])), None)
    out["longer_in_the_middle"] = (_base("strangers_longer", _renamed(w, 10, 1, name(10) + b"x")), None)
    # the pair astride the text carry: the window ends behind mate 1 of pair 7, whose mate 2 has another name
    astride = _renamed(w, 7, 1, name(7)[:-1] + b"!")
    cut = sum(len(r) for pair in astride[:7] for r in pair) + len(astride[7][0])
    out["astride_the_carry"] = (_base("strangers_astride", astride), [cut, cut + 2000])
    out["suffix_does_not_hide_it"] = (_base("strangers_suffix", _renamed(w, 3, 1, name(3)[:-1] + b"2"), suffix=True), None)
    # sorted by coordinate: the mates of three pairs lie apart (mate 1s first), as `samtools sort` leaves a small region
    srt = [bc._rec(bc.hit(80, 100 * i), b"frag%d" % i, 0x63, ref_id=0, pos=100 + 10 * i, cigar=(80 << 4,)) for i in range(3)] + \
          [bc._rec(bc.hit(80, 100 * i + 300), b"frag%d" % i, 0x93, ref_id=0, pos=400 + 10 * i, cigar=(80 << 4,)) for i in range(3)]
    out["coordinate_sorted"] = (bc.Base("pairs_strangers_sorted", bc._payload(srt, sc.REFS3), X900, False, False, False), None)
    trio = pattern_records(b"t")[:2] + [[bc._rec(bc.hit(70, 1), b"trio", 0x41), bc._rec(bc.hit(30, 90), b"trio", 0x841),
                                         bc._rec(bc.miss(70, 2), b"trio", 0x81)]] + [mates(bc.hit(60, 7), bc.miss(61, 8), b"after")[0]]
    out["trio_with_0x900_not_excluded"] = (_base("strangers_trio", trio, sel=sc.NO_SEL), None)
    return out


def unpaired_bases():
    w = window_records()
    odd = w[:6] + [[w[6][0]]]
    cut = sum(len(r) for pair in odd[:5] for r in pair) + 40
    return {"odd_count": (_base("unpaired_odd", odd), None),
            "odd_count_in_windows": (_base("unpaired_odd_windows", odd), [cut, cut + 300]),
            "a_selection_that_removes_one_mate": (_base("unpaired_selected", w[:3] + [[w[3][0], bc._rec(bc.miss(50, 1), bc.name_of(15, 3), 0x400 | F2)]],
                                                        sel=sc.NO_SEL._replace(excl=0xD00)), None)}


# ------------------------------------------------------------------------------------------------ the cases
RULES = [(rp.ANY, False), (rp.ANY, True), (rp.BOTH, False), (rp.BOTH, True)]
_ALL = None


def _mk(name, base, cuts=None, min_hits=1, min_permille=0, invert=False, pair_rule=rp.ANY, piece_kb=1):
    return PCase(name, base, cuts, min_hits, min_permille, invert, pair_rule, error_of(base), piece_kb)


def _every(base, step):
    _, _, hdr = bc.read_bam(base.payload)
    return list(range(step, len(base.payload) - hdr, step))


def all_cases():
    global _ALL
    if _ALL is not None:
        return _ALL
    out = []
    patterns, permille = _base("patterns", pattern_records()), _base("permille", permille_records())
    for pair_rule, invert in RULES:                                   # 1. the four hit patterns, inside one 16 KiB tile
        tag = pair_rule + ("_invert" if invert else "")
        out.append(_mk("patterns__" + tag, patterns, pair_rule=pair_rule, invert=invert))
        out.append(_mk("permille_150__" + tag, permille, min_permille=150, pair_rule=pair_rule, invert=invert))
    out.append(_mk("names__any", _base("names", names_records())))   # 2. what the decode and the check see
    out.append(_mk("suffix_on__any", _base("suffix_on", suffix_records(), suffix=True)))
    out.append(_mk("suffix_off__any_invert", _base("suffix_off", suffix_records()[:-2], suffix=False), invert=True))
    out.append(_mk("strand__any", _base("strand", strand_records(), orig=True)))
    lengths = _base("lengths", lengths_records())
    out.append(_mk("lengths__any", lengths, piece_kb=0))
    out.append(_mk("lengths_in_windows__any", lengths._replace(name="pairs_lengths_windows"), cuts=_every(lengths, 25_000), piece_kb=0))
    out.append(_mk("excluded_between__any", _base("excluded", excluded_records())))
    out.append(_mk("straddle__any", straddle_base()[0]))
    out.append(_mk("residues__any", _base("residues", residue_records())))
    windows = _base("windows", window_records())                      # 3. windows: the two carries
    for step in (97, 301, 1000):
        out.append(_mk("windows_every_%d__any" % step, windows._replace(name="pairs_windows_%d" % step), cuts=_every(windows, step)))
    base, cuts = carry_base()
    out.append(_mk("carry_over_empty_windows__any", base, cuts=cuts))
    out.append(_mk("carry_over_empty_windows__both", base._replace(name="pairs_carry_both"), cuts=cuts, pair_rule=rp.BOTH))
    for name, (base, cuts) in list(stranger_bases().items()) + list(unpaired_bases().items()):          # 4. what has to fail
        out.append(_mk(name, base, cuts=cuts))
    _ALL = out
    return _ALL


def good_cases():
    return [c for c in all_cases() if c.error is None]


def error_cases():
    return [c for c in all_cases() if c.error is not None]


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ------------------------------------------------------------------------------------------------ what keeps it from being vacuous
FEATURES = ("name of 1", "name of 63", "name of 64", "name of 65", "name of 254", "replaced name byte", "suffix, first then last",
            "suffix, last then first", "suffix on, no mate bit", "flipped mate", "l_seq 0 first", "l_seq 0 second", "l_seq 1 first",
            "l_seq 1 second", "l_seq 39770 first", "l_seq 39770 second", "absent qualities", "excluded between the mates",
            "excluded between pairs", "across a tile boundary")


def features(case):
    """Per pair of the case, the set of the features it has."""
    base = case.base
    _, recs, _ = bc.read_bam(base.payload)
    sel = [i for i, r in enumerate(recs) if bc.selected(r, base.sel)]
    out = []
    for p in range(len(sel) // 2):
        i, j = sel[2 * p], sel[2 * p + 1]
        a, b = recs[i], recs[j]
        f = set()
        if len(a.name) in NAME_LENGTHS:
            f.add("name of %d" % len(a.name))
        if any(not 0x21 <= c <= 0x7E for c in a.name + b.name):
            f.add("replaced name byte")
        if base.suffix:
            s = (bc.mate_suffix(a.flag, True), bc.mate_suffix(b.flag, True))
            f.add({(b"/1", b"/2"): "suffix, first then last", (b"/2", b"/1"): "suffix, last then first"}.get(s, "suffix on, no mate bit"))
        if base.orig and (a.flag | b.flag) & 0x10:
            f.add("flipped mate")
        for n in (0, 1, LONG):
            if len(a.seq) == n:
                f.add("l_seq %d first" % n)
            if len(b.seq) == n:
                f.add("l_seq %d second" % n)
        if any(r.seq and r.qual[0] == 0xFF for r in (a, b)):
            f.add("absent qualities")
        if j > i + 1:
            f.add("excluded between the mates")
        if p and i > sel[2 * p - 1] + 1:
            f.add("excluded between pairs")
        if a.start // TILE != (b.start + b.size - 1) // TILE:
            f.add("across a tile boundary")
        out.append(f)
    return out
