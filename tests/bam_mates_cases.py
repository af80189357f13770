"""Catalogue of cases for keeping the mates of a name-collated BAM file together IN BAM OUTPUT (include/kmm.h "record_bam_mates";
DESIGN 4.25): BAM files whose selected records are mates in file order, 2p and 2p + 1, whose kept pairs come back as the two
records' own bytes, mate 1 directly in front of mate 2.

Nothing here reads the library.  The model is
    bam_fastq_cases.read_bam / selected   that module's own BAM reader and the selection's rule; BRec.start / BRec.size locate a
                                          record's raw bytes, BRec.name is its read_name without the NUL
    bam_records_cases.fasta_of + expected the two-line FASTA of the selected records and, through the record-keep catalogue's model,
                                          hits and windows per record
    record_pairs_cases.pair_keep_entries  the pair rule in Python integers
    first_stranger                        the mate check: the two names compared as Python bytes, nothing trimmed
so a good case expects b"".join(payload[r.start:r.start + r.size]) over both mates of every kept pair, one entry per record in
pair order, and a file that inflates to payload[:hdr] + those bytes; an error case expects ("strangers", p) or ("unpaired", n) from
the call bam_pairs_cases.window_of names.  Windows are bam_pairs_cases' (cuts at inflated offsets, windowed_file): its functions
read case.base.payload, case.base.sel, case.cuts and case.error, which the cases here have too.
tests/test_bam_mates_on_the_cpu.py holds the catalogue to the conditions that keep it from being vacuous."""
from collections import namedtuple

from tests import bam_fastq_cases as bc
from tests import bam_pairs_cases as bp
from tests import bam_records_cases as br
from tests import record_pairs_cases as rp

K = br.K
TILE = br.TILE
LONG = bp.LONG
X900 = bp.X900
MAPQ20 = X900._replace(min_mapq=20)                                   # (not flags only: the walk asks the whole predicate)

# base: bam_records_cases.RBase (name payload sel orig k); cuts: inflated payload offsets where windows end (None: one window);
# error: None, ("strangers", p) or ("unpaired", n_selected)
MCase = namedtuple("MCase", "name base cuts min_hits min_permille invert pair_rule error")


# ------------------------------------------------------------------------------------------------ the model
def selected_records(base):
    return br.decoded(base).records


def first_stranger(records):
    """The first pair p whose records 2p and 2p + 1 have different read_name bytes (None: all are mates)."""
    for p in range(len(records) // 2):
        if bytes(records[2 * p].name) != bytes(records[2 * p + 1].name):
            return p
    return None


def error_of(base):
    """What a stream of `base` has to fail with: strangers come first (they lie in front of an unpaired end)."""
    recs = selected_records(base)
    p = first_stranger(recs)
    if p is not None:
        return ("strangers", p)
    if len(recs) % 2:
        return ("unpaired", len(recs))
    return None


def entries(base):
    """(hits, windows) per selected record of `base`, in file order: the record-keep catalogue's model over the FASTA text."""
    e = br.expected(br.RCase(base.name + "__entries", base, 1, 0, False))
    return e[3], e[4]


def rule_of(case):
    return dict(min_hits=case.min_hits, min_permille=case.min_permille, invert=case.invert, pair_rule=case.pair_rule)


Expect = namedtuple("Expect", "raw n_records keep hits windows")
_EXPECT = {}


def expected(case, n_pairs=None):
    """The first n_pairs pairs of the case (None: all whole pairs): the kept pairs' raw bytes, the kept RECORDS, the keep flag per
    pair, and the entries per record in pair order."""
    key = (case.name, n_pairs)
    if key not in _EXPECT:
        recs = selected_records(case.base)
        n = len(recs) // 2 if n_pairs is None else n_pairs
        hits, windows = entries(case.base)
        hits, windows = hits[:2 * n], windows[:2 * n]
        keep = rp.pair_keep_entries(hits, windows, **rule_of(case))
        p = case.base.payload
        raw = b"".join(p[r.start:r.start + r.size] for i in range(n) if keep[i] for r in recs[2 * i:2 * i + 2])
        _EXPECT[key] = Expect(raw, 2 * int(keep.sum()), keep, hits, windows)
    return _EXPECT[key]


def expected_file(case):
    """What the output file inflates to: the input's header, verbatim, and both records of every kept pair."""
    return case.base.payload[:br.decoded(case.base).hdr] + expected(case).raw


window_ends, selected_done, window_of, windowed_file, boundary_kinds = (bp.window_ends, bp.selected_done, bp.window_of, bp.windowed_file,
                                                                        bp.boundary_kinds)


# ------------------------------------------------------------------------------------------------ the bases
def _flat(records):
    return [r for pair in records for r in (pair if isinstance(pair, list) else [pair])]


def _base(name, records, sel=X900, orig=False, k=K, refs=()):
    return br.RBase("mates_" + name, bc._payload(_flat(records), refs), sel, orig, k)


def _of(b, name=None, sel=None):
    """A bam_fastq_cases.Base (bam_pairs_cases builds those) as a base of this catalogue."""
    return br.RBase("mates_" + (name or b.name), b.payload, b.sel if sel is None else sel, b.orig, K)


def good_names_records():
    """Equal names of 1, 63, 64, 65 and 254 bytes and empty ones (l_read_name 1), each on a kept and on a dropped pair."""
    recs = []
    for i, n in enumerate((0, 1, 63, 64, 65, 254)):
        recs.append(bp.mates(bc.hit(70 + i, 300 * i), bc.miss(60 + i, 20 + i), bc.name_of(n, n)))
        recs.append(bp.mates(bc.miss(71 + i, 30 + i), bc.miss(61 + i, 40 + i), bc.name_of(n, n + 1)))
    return recs


def runs_records(mapq):
    """Unselected records between two mates: one; a run that crosses a 16 KiB boundary; a run longer than a tile; and unselected
    records behind the last pair.  mapq: the fillers are unselected by turns through 0x800 and through MAPQ 0 (the mates have MAPQ
    30) — else through 0x800 alone."""
    kw = dict(mapq=30)
    n = [0]

    def filler(size):
        n[0] += 1
        low = mapq and n[0] % 2 == 0
        bare = len(bc._rec(bc.hit(40, 11 * n[0]), b"fill", 0x41 if low else 0x841, mapq=0 if low else 30))
        return bc._rec(bc.hit(40, 11 * n[0]), b"fill", 0x41 if low else 0x841, mapq=0 if low else 30, aux=b"Z" * (size - bare))

    def pair(i, kept):
        a, b = (bc.hit(80 + i, 500 * i), bc.miss(70 + i, 300 + i)) if kept else (bc.miss(81 + i, 310 + i), bc.miss(71 + i, 320 + i))
        return bp.mates(a, b, b"run%d" % i, **kw)

    out = []
    for i, sizes in enumerate(((200,), (200,), (6000, 6000, 6000), (6000, 6000, 6000), (5000,) * 5, (5000,) * 5)):
        m1, m2 = pair(i, i % 2 == 0)
        out += [m1] + [filler(s) for s in sizes] + [m2]
    out += [filler(300), filler(9000), filler(9000)]
    return out


def residues_records():
    """Kept pairs of 49 + 64 bytes (113 = 1 modulo 16: the destination of both mates moves on by one residue per kept pair) and
    dropped pairs of 49 + 49 in between (the source moves on by two against it): all 16 destination residues for either mate, at
    changing source residues.  Empty names; genome_index(1), as bam_records_cases.sizes_base."""
    recs = []
    for i in range(20):
        recs.append([br._sized(49, True, 3 * i), br._sized(64, True, 3 * i + 1)])
        recs.append([br._sized(49, False, 3 * i + 2), br._sized(49, False, 3 * i)])
    return recs


def _sizes(records):
    return [len(r) for r in _flat(records)]


def _ends(records):
    out, at = [], 0
    for s in _sizes(records):
        at += s
        out.append(at)
    return out


# ------------------------------------------------------------------------------------------------ the cases
RULES = bp.RULES
_ALL = None


def _mk(name, base, cuts=None, min_hits=1, min_permille=0, invert=False, pair_rule=rp.ANY):
    return MCase(name, base, cuts, min_hits, min_permille, invert, pair_rule, error_of(base))


def _every(base, step):
    hdr = br.decoded(base).hdr
    return list(range(step, len(base.payload) - hdr, step))


def all_cases():
    global _ALL
    if _ALL is not None:
        return _ALL
    out = []
    patterns, permille = _base("patterns", bp.pattern_records()), _base("permille", bp.permille_records())
    for pair_rule, invert in RULES:                                   # 1. decisions
        tag = pair_rule + ("_invert" if invert else "")
        out.append(_mk("patterns__" + tag, patterns, pair_rule=pair_rule, invert=invert))
        out.append(_mk("permille_150__" + tag, permille, min_permille=150, pair_rule=pair_rule, invert=invert))
    out.append(_mk("patterns__nothing_kept", patterns, min_hits=1_000_000))
    out.append(_mk("patterns__everything_kept", patterns, min_hits=0))
    out.append(_mk("names__any", _base("names", good_names_records())))    # 2. names, tiles, runs, destinations
    out.append(_mk("straddle__any", _of(bp.straddle_base()[0])))
    lengths = _base("lengths", bp.lengths_records())
    out.append(_mk("lengths__any", lengths))
    out.append(_mk("lengths_in_windows__both", lengths, cuts=_every(lengths, 25_000), pair_rule=rp.BOTH))
    out.append(_mk("excluded_between__any", _base("excluded", bp.excluded_records())))
    runs = _base("runs", runs_records(False))
    out.append(_mk("runs__any", runs))
    out.append(_mk("runs_in_windows__any", runs, cuts=_every(runs, 7001)))
    runs_q = _base("runs_mapq", runs_records(True), sel=MAPQ20)
    out.append(_mk("runs_mapq__any", runs_q))
    out.append(_mk("runs_mapq_in_windows__any_invert", runs_q, cuts=_every(runs_q, 4999), invert=True))
    out.append(_mk("selection__any", _of(bc.selection_base(), "selection")))
    residues = _base("residues", residues_records(), k=1)
    out.append(_mk("residues__any", residues))
    out.append(_mk("residues_in_windows__any", residues, cuts=_every(residues, 61)))
    windows = _base("windows", bp.window_records())                    # 3. windows: the two carries
    for step in (97, 301, 1000):
        out.append(_mk("windows_every_%d__any" % step, windows, cuts=_every(windows, step)))
    ends = _ends(bp.pattern_records())
    out.append(_mk("cut_between_the_mates__any", patterns, cuts=[ends[0], ends[6]]))
    out.append(_mk("three_windows_end_odd__any", patterns, cuts=[ends[0], ends[2], ends[4]]))
    out.append(_mk("only_the_carrys_mate__any", patterns, cuts=[ends[2], ends[3]]))
    out.append(_mk("kept_carry_at_a_filled_queue__any", patterns, cuts=[ends[2]]))
    out.append(_mk("dropped_carry__any", patterns, cuts=[ends[6]]))
    base, cuts = bp.carry_base()
    out.append(_mk("carry_over_empty_windows__any", _of(base), cuts=cuts))
    out.append(_mk("carry_over_empty_windows__both", _of(base), cuts=cuts, pair_rule=rp.BOTH))
    for name, (base, cuts) in list(bp.stranger_bases().items()) + list(bp.unpaired_bases().items()):     # 4. what has to fail
        out.append(_mk(name, _of(base), cuts=cuts))
    w = bp.window_records()
    long_name = lambda tag: bc.name_of(100, tag)
    named = [bp.mates(bc.hit(60 + i, 350 * i), bc.miss(50 + i, 230 + i), long_name(i)) for i in range(8)]
    for at in (63, 64, 65):
        other = bytearray(long_name(5))
        other[at] ^= 1
        out.append(_mk("strangers_differ_at_byte_%d" % at, _base("strangers_at_%d" % at, bp._renamed(named, 5, 1, bytes(other)))))
    out.append(_mk("strangers_in_windows", _base("strangers_windows", bp._renamed(w, 11, 0, b"~" + bc.name_of(23, 11)[1:])),
                   cuts=_every(windows, 301)))
    _ALL = out
    return _ALL


def good_cases():
    return [c for c in all_cases() if c.error is None]


def error_cases():
    return [c for c in all_cases() if c.error is not None]


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


# ------------------------------------------------------------------------------------------------ what keeps it from being vacuous
def _all_and_selected(base):
    d = br.decoded(base)
    chosen = {r.start for r in d.records}
    return d.all_records, [i for i, r in enumerate(d.all_records) if r.start in chosen]


def seam_kinds(case):
    """The kinds of tile seam and of unselected run the pairs of the case show."""
    recs, sel = _all_and_selected(case.base)
    starts = {r.start // TILE for r in recs}
    out = set()
    for p in range(len(sel) // 2):
        i, j = sel[2 * p], sel[2 * p + 1]
        a, b = recs[i], recs[j]
        ta, tb = a.start // TILE, b.start // TILE
        if ta == tb:
            out.add("both mates in one tile")
        if tb == ta + 1 and recs[j - 1].start // TILE == ta and not any(r.start // TILE == ta for r in recs[i + 1:j]) and j == i + 1:
            out.add("mate 1 last of its tile, mate 2 first of the next")
        if tb - ta >= 3 and j == i + 1:
            out.add("mate 2 several tiles on")
        if any(t not in starts for t in range(ta + 1, tb)):
            out.add("a tile without a record start between the mates")
        between = recs[i + 1:j]
        if len(between) == 1:
            out.add("one unselected record between the mates")
        if between and between[0].start // TILE != (between[-1].start + between[-1].size - 1) // TILE:
            out.add("an unselected run across a tile boundary")
        if between and between[-1].start + between[-1].size - between[0].start > TILE:
            out.add("an unselected run longer than a tile")
    if sel and sel[-1] < len(recs) - 1 and len(sel) % 2 == 0:
        out.add("unselected records behind the last pair")
    return out


SEAM_KINDS = ("both mates in one tile", "mate 1 last of its tile, mate 2 first of the next", "mate 2 several tiles on",
              "a tile without a record start between the mates", "one unselected record between the mates",
              "an unselected run across a tile boundary", "an unselected run longer than a tile", "unselected records behind the last pair")


def decision_kinds(case):
    """{'only mate 1', 'only mate 2', 'both', 'neither'}: which mates of the case's pairs match the rule (before the pair rule)."""
    hits, windows = entries(case.base)
    h, w = hits.tolist(), windows.tolist()
    m = [h[i] >= case.min_hits and 1000 * h[i] >= case.min_permille * w[i] for i in range(len(h) - len(h) % 2)]
    names = {(True, False): "only mate 1", (False, True): "only mate 2", (True, True): "both", (False, False): "neither"}
    return {names[(m[i], m[i + 1])] for i in range(0, len(m), 2)}


def residues(case):
    """({(source % 16, destination % 16)} of the kept mate 1s, the same of the kept mate 2s), the queue's tail at 0."""
    recs = selected_records(case.base)
    out, dst = (set(), set()), 0
    for p, kp in enumerate(expected(case).keep):
        if kp:
            for m in (0, 1):
                r = recs[2 * p + m]
                out[m].add((r.start % 16, dst % 16))
                dst += r.size
    return out


def window_kinds(case):
    """What the windows of the case show: cuts by the record they lie in, and the states of the carry."""
    out = set()
    if not case.cuts:
        return out
    done = selected_done(case)
    for mate, kind, waiting, new in boundary_kinds(case):
        if mate is None:
            out.add("a cut between the mates" if waiting else "a cut between two pairs")
        else:
            out.add("a cut inside %s%s" % ({0: "an unselected record", 1: "mate 1", 2: "mate 2"}[mate],
                                          "" if mate != 2 else "'s " + {"head": "fixed head", "name": "name", "seq": "SEQ", "qual": "QUAL or aux"}[kind]))
            if mate == 0 and waiting:
                out.add("a cut inside an unselected record between the mates")
    prev, odd_run = 0, 0
    for i, n in enumerate(done):
        new = n - prev
        if prev % 2 == 1 and new == 0 and i < len(done) - 1:
            out.add("a window with no selected record while a carry waits")
        if prev % 2 == 1 and new == 1:
            out.add("a window whose only selected record is the carry's mate")
        odd_run = odd_run + 1 if n % 2 == 1 and new > 0 else 0
        if odd_run >= 3:
            out.add("three windows in a row that end odd")
        if case.error is None and prev % 2 == 1 and new >= 1:
            e = expected(case)
            p = prev // 2
            if e.keep[p]:
                filled = len(expected(case, p).raw)
                out.add("a kept carried pair at a queue residue of %s" % ("0" if filled % 16 == 0 else "not 0"))
            else:
                out.add("a dropped carried pair")
        prev = n
    return out


WINDOW_KINDS = ("a cut between the mates", "a cut inside mate 2's fixed head", "a cut inside mate 2's name", "a cut inside mate 2's SEQ",
                "a cut inside mate 2's QUAL or aux", "a cut inside mate 1", "a cut inside an unselected record between the mates",
                "a window with no selected record while a carry waits", "a window whose only selected record is the carry's mate",
                "three windows in a row that end odd", "a kept carried pair at a queue residue of not 0", "a dropped carried pair")
