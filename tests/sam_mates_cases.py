"""Catalogue of cases for mates kept together in SAM output (include/kmm.h "record_sam_mates"), and an independent
model.  Nothing here reads the library.

A case is a SAM text with a selection, a keep rule, a pair rule and the mode (1: header lines kept, 2: dropped).  The model is pure
Python: the text is split at '\\n'; what is selected comes from tests/sam_records_cases.selected, the per-record (hits, windows)
from the numpy model behind sam_records_cases.model over the model's own FASTA, the pair rule in Python integers from
tests/record_pairs_cases.pair_keep; names are compared as Python bytes (everything in front of the first TAB).  The selected records
of the stream, in file order, are mates 2p and 2p + 1; the expected bytes are line slices: a header line where it stands (mode 1),
both lines of a kept pair where mate 2 stands — so a header line between two mates comes out in front of the pair.

model_stream restates the same rule window by window with a waiting mate, as a caller that cuts the text anywhere would see it;
tests/test_sam_mates_on_the_cpu.py holds the two formulations to each other under every cutting.

The kernels' seams: the walk's tiles are 1024 bytes; both prefixes are two-level, over blocks of 1024 spans and of 1024 tiles; the
mate check compares 64 bytes a round.
"""
from collections import namedtuple

import numpy as np

from tests import record_pairs_cases as rp
from tests import sam_records_cases as sr
from tests import strand_cases

K = sr.K
TILE, BLOCK = 1024, 1024
ANY, BOTH = rp.ANY, rp.BOTH
NO_SEL = sr.NO_SEL
MCase = namedtuple("MCase", "name text k excl sel orig revcomp min_hits min_permille invert mode pair_rule last")
# stranger: the stream-wide ordinal of the first pair whose names differ (None: none; out then holds what precedes nothing: the
# call fails); odd: a selected record is left without a mate (with `last` the stream's end is an error)
Expected = namedtuple("Expected", "out n_kept keep hits windows consumed n_records n_excluded n_headers n_pairs odd stranger unpaired_out")


def case(name, text, k=K, excl=0, sel=NO_SEL, orig=False, revcomp=False, min_hits=1, min_permille=0, invert=False, mode=1, pair_rule=ANY,
         last=False):
    return MCase(name, bytes(text), k, excl, sel, orig, revcomp, min_hits, min_permille, invert, mode, pair_rule, last)


# ------------------------------------------------------------------------------------------------ the model
def name_of(line):
    """The bytes in front of the first TAB (the whole line when it has none)"""
    return line.split(b"\t", 1)[0]


def classify(c, text):
    """[(start, length, kind)] of the lines that have their newline: kind None a header line, True selected, False not"""
    out = []
    for start, length in sr.lines_of(text):
        body = text[start:start + length - 1]
        if body.endswith(b"\r"):
            body = body[:-1]
        if body[:1] == b"@":
            out.append((start, length, None))
        else:
            out.append((start, length, bool(sr.selected(body.split(b"\t"), c.excl, c.sel))))
    return out


def rule_of(c):
    return dict(min_hits=c.min_hits, min_permille=c.min_permille, invert=c.invert, pair_rule=c.pair_rule)


def model(c, text=None):
    """Expected of the case over the whole text at once (text: another text under the case's rules)."""
    text = c.text if text is None else bytes(text)
    single = sr.model(c, text)                                         # entries per selected record, counters, the unpaired keep
    kinds = classify(c, text)
    sel_lines = [(s, n) for s, n, kind in kinds if kind]
    assert len(sel_lines) == single.n_records
    n_pairs = len(sel_lines) // 2
    hits, windows = single.hits[:2 * n_pairs].copy(), single.windows[:2 * n_pairs].copy()
    keep = rp.pair_keep_entries(hits, windows, **rule_of(c)) if n_pairs else np.zeros(0, dtype=bool)
    stranger = None
    for p in range(n_pairs):
        (s1, n1), (s2, n2) = sel_lines[2 * p], sel_lines[2 * p + 1]
        if name_of(text[s1:s1 + n1]) != name_of(text[s2:s2 + n2]):
            stranger = p
            break
    out, g = [], 0
    for s, n, kind in kinds:
        if kind is None:
            if c.mode == 1:
                out.append(text[s:s + n])
        elif kind:
            if g % 2 == 1 and keep[g // 2]:
                s1, n1 = sel_lines[g - 1]
                out.append(text[s1:s1 + n1] + text[s:s + n])
            g += 1
    for a in (hits, windows, keep):
        a.setflags(write=False)
    return Expected(b"".join(out), 2 * int(keep.sum()), keep, hits, windows, single.consumed, single.n_records, single.n_excluded,
                    single.n_headers, n_pairs, len(sel_lines) % 2 == 1, stranger, single.out)


_EXPECT = {}


def expected(c):
    if c.name not in _EXPECT:
        _EXPECT[c.name] = model(c)
    return _EXPECT[c.name]


class Strangers(Exception):
    def __init__(self, pair):
        super().__init__("pair %d" % pair)
        self.pair = pair


class Unpaired(Exception):
    pass


def model_stream(c, text, cuts, entries=None):
    """The same rule as a caller sees it who hands the text over in windows that end at `cuts` (and at the end), the bytes behind a
    window's last newline carried to the next: per window the kept bytes and the entries appended; a selected record without its
    mate waits.  entries: (hits, windows) per selected record of the stream (default: the model's own).  Returns
    (out, n_entries per window); raises Strangers(stream-wide pair) from the window that completes such a pair — nothing of that
    window is appended — and Unpaired at the end of a `last` stream that leaves a record waiting."""
    text = bytes(text)
    if entries is None:
        single = sr.model(c, text)
        entries = (single.hits, single.windows)
    h, w = entries[0].tolist(), entries[1].tolist()
    rule = rule_of(c)
    ends = sorted(set([x for x in cuts if 0 < x < len(text)] + [len(text)]))
    out, per_window, waiting, done, pos, carry = [], [], None, 0, 0, b""
    for end in ends:
        win = carry + text[pos:end]
        pos = end
        cut = win.rfind(b"\n") + 1
        carry, win = win[cut:], win[:cut]
        got, mate, n = [], waiting, 0
        for s, ln, kind in classify(c, win):
            line = win[s:s + ln]
            if kind is None:
                if c.mode == 1:
                    got.append(line)
            elif kind:
                if mate is None:
                    mate = line
                    continue
                p = done + n // 2
                if name_of(mate) != name_of(line):
                    raise Strangers(p)
                if rp.pair_keep(h[2 * p], w[2 * p], h[2 * p + 1], w[2 * p + 1], **rule):
                    got.append(mate + line)
                mate = None
                n += 2
        waiting, done = mate, done + n // 2
        out.append(b"".join(got))
        per_window.append(n)
    if c.last and waiting is not None:
        raise Unpaired()
    return b"".join(out), per_window


# ------------------------------------------------------------------------------------------------ writing lines
HEAD = sr.HEAD
hit_read, miss_read = sr.hit_read, sr.miss_read


def half_read(n, at):
    """A read whose first half hits and whose second half cannot: some 40 % of its windows"""
    return hit_read(n // 2, at) + miss_read(n - n // 2)


def mline(name, flag, seq, total=None, **kw):
    """sam_records_cases.line; total: the line is padded to exactly that many bytes by a tag (the name stays what it is)"""
    tags = kw.pop("tags", b"")
    bare = sr.line(name, flag, seq, tags=tags, **kw)
    if total is None:
        return bare
    need = total - len(bare)
    assert need >= 6, (total, len(bare))
    out = sr.line(name, flag, seq, tags=tags + b"\tXP:Z:" + b"p" * (need - 6), **kw)
    assert len(out) == total
    return out


def pair(name, seq1, seq2, flag1=0x43, flag2=0x83, name2=None, **kw):
    return mline(name, flag1, seq1, **kw) + mline(name if name2 is None else name2, flag2, seq2, **kw)


H, M = (lambda i: hit_read(120, 300 * i + 11)), (lambda i: miss_read(110))


def patterns_text():
    """The four hit patterns of a pair, twice over, then a pair whose mates lie on both sides of a per-mille threshold"""
    out = [HEAD]
    for i, (a, b) in enumerate([(H, H), (H, M), (M, H), (M, M), (M, H), (H, H), (M, M), (H, M)]):
        out.append(pair(b"pat%d" % i, a(2 * i), b(2 * i + 1)))
    out.append(pair(b"permille", hit_read(150, 4000), half_read(200, 5000)))
    out.append(pair(b"permille_r", half_read(180, 6000), hit_read(90, 7000)))
    return b"".join(out)


def tile_seam_text():
    """Mate 1 the last line of a tile, mate 2 at the next tile's first byte; then a mate 1 that ends one byte short of a tile's end,
    so that mate 2 STARTS at the tile's last byte; every pair kept or dropped by its own reads."""
    parts = [HEAD, pair(b"s0", H(0), M(1))]
    at = sum(len(p) for p in parts)
    parts.append(mline(b"edge_a", 0x43, H(2), total=2 * TILE - at))                # ends at 2048
    parts.append(mline(b"edge_a", 0x83, M(3)))                                      # starts at 2048
    at = sum(len(p) for p in parts)
    parts.append(pair(b"mid", M(4), M(5)))
    at = sum(len(p) for p in parts)
    parts.append(mline(b"edge_b", 0x43, M(6), total=4 * TILE - 1 - at))            # ends at 4095
    parts.append(mline(b"edge_b", 0x83, H(7)))                                      # starts at 4095, the tile's last byte
    parts.append(pair(b"tail", H(8), H(9)))
    text = b"".join(parts)
    starts = [s for s, _ in sr.lines_of(text)]
    assert 2 * TILE in starts and 4 * TILE - 1 in starts
    return text


def tiles_on_text():
    """Mate 2 several tiles behind mate 1: a supplementary line longer than two tiles (not selected) and a header line of a tile
    and a half lie between them"""
    return (HEAD + pair(b"a", H(0), H(1)) + mline(b"far", 0x43, H(2)) + mline(b"far", 0x843, miss_read(2300)) +
            b"@CO\t" + b"c" * 1500 + b"\n" + mline(b"far", 0x83, M(3)) + pair(b"z", M(4), M(5)) + pair(b"zz", M(6), H(7)))


def between_text():
    """Lines that are not selected between two mates: a supplementary one (0x800), one under the MAPQ floor, one outside the
    regions; and a record of another name that is not selected either"""
    out = [HEAD]
    for i in range(6):
        out.append(mline(b"b%d" % i, 0x43, (H, M)[i % 2](2 * i), pos=1000 + 10 * i))
        out.append(mline(b"b%d" % i, 0x843, hit_read(60, 40 * i), pos=1000))       # supplementary
        out.append(mline(b"other%d" % i, 0x0, H(50 + i), mapq=3, pos=1000))          # under the floor
        out.append(mline(b"b%d" % i, 0x43, H(70 + i), pos=90_000))                   # outside the regions
        out.append(mline(b"b%d" % i, 0x83, (M, H, M)[i % 3](2 * i + 1), pos=1200 + 10 * i))
    return b"".join(out)


BETWEEN_SEL = (0, 20, [(b"chr1", 0, 50_000)], False)


def header_between_text():
    """Header lines in front, between the two mates of a kept and of a dropped pair, between pairs and at the end"""
    return (HEAD + mline(b"h0", 0x43, H(0)) + b"@CO\tbetween the mates of a kept pair\n" + mline(b"h0", 0x83, M(1)) +
            b"@CO\tbetween two pairs\n" + mline(b"h1", 0x43, M(2)) + b"@CO\tbetween the mates of a dropped pair\n" +
            b"@CO\tand another\n" + mline(b"h1", 0x83, M(3)) + pair(b"h2", H(4), H(5)) + b"@CO\tat the end\n")


NAME_LENGTHS = (1, 2, 31, 63, 64, 65, 127, 128, 129, 254)


def names_text():
    """Mates whose names have 1, 63, 64, 65 and 254 bytes, and QNAME '*' twice: all mates of each other"""
    out = [HEAD]
    for i, n in enumerate(NAME_LENGTHS):
        name = (b"%03d" % n + b"n" * 300)[:n] if n >= 3 else b"nq"[:n]
        out.append(pair(name, (H, M)[i % 2](2 * i), (M, H, H)[i % 3](2 * i + 1)))
    out.append(pair(b"*", H(40), M(41)))
    return b"".join(out)


def strangers_text(kind):
    good = [pair(b"g%d" % i, (H, M)[i % 2](2 * i), H(2 * i + 1)) for i in range(4)]
    if kind == "last_byte":
        bad = pair(b"x" * 64 + b"a", H(20), H(21), name2=b"x" * 64 + b"b")
    elif kind == "prefix":
        bad = pair(b"read7", H(20), H(21), name2=b"read77")
    elif kind == "prefix_reversed":
        bad = pair(b"read77", H(20), H(21), name2=b"read7")
    elif kind == "first_byte":
        bad = pair(b"aread", H(20), H(21), name2=b"bread")
    else:
        raise ValueError(kind)
    return HEAD + b"".join(good[:2]) + bad + b"".join(good[2:])


def dense_pairs_text(n=2700, bad_at=None):
    """Minimal 22-byte records named 'q' — all mates of each other — SEQ 'C' (a hit at k = 1), 'A' (a window, no hit), '*' (none),
    a header line every 500: more than two blocks of spans; with the header lines kept, record 1022 is span 1023 and its mate span
    1024.  bad_at: that record is named 'r' (a stranger to its mate)."""
    recs = [(b"r" if i == bad_at else b"q") + b"\t4\t*\t0\t0\t*\t*\t0\t0\t" + (b"C", b"A", b"*", b"A", b"C", b"A", b"A")[i % 7] + b"\t*\n"
            for i in range(n)]
    parts = []
    for i in range(0, n, 500):
        parts += [b"@CO\tbefore record %d\n" % i] + recs[i:i + 500]
    return b"".join(parts)


def big_pairs_text(size=1_400_000, seed=11):
    """More than 1024 tiles of pairs with supplementary lines between some mates and a header line now and then; one mate 1 ends
    at the last byte of tile 1023, so that its mate 2 starts at the first byte of tile 1024"""
    rng = np.random.default_rng(seed)
    edge = BLOCK * TILE
    parts, at, i, placed = [HEAD], len(HEAD), 0, False
    while at < size:
        ln = int(rng.integers(120, 260))
        s1 = (hit_read(ln, 53 * i), miss_read(ln), hit_read(ln, 29 * i + 7))[i % 3]
        s2 = (miss_read(ln), hit_read(ln, 31 * i + 3))[i % 2]
        name = b"b%d" % i
        m1, m2 = mline(name, 0x63, s1, pos=1 + 17 * i), mline(name, 0x93, s2, pos=1 + 17 * i)
        mid = b""
        if i % 5 == 2:
            mid = mline(name, 0x863, hit_read(40, i), pos=5)
        if i % 150 == 75:
            mid += b"@CO\tbehind record %d\n" % i
        if not placed and at + 4000 > edge:
            m1, mid, placed = mline(name, 0x63, s1, pos=1 + 17 * i, total=edge - at), b"", True
        rec = m1 + mid + m2
        parts.append(rec)
        at += len(rec)
        i += 1
    text = b"".join(parts)
    assert placed and edge in [s for s, _ in sr.lines_of(text)] and text[edge - 1:edge] == b"\n"
    return text


def orientation_text():
    g = hit_read
    rc_ = strand_cases.revcomp
    return (HEAD + pair(b"o0", g(100, 400), rc_(g(100, 1200)), flag1=0x63, flag2=0x93) + pair(b"o1", miss_read(80), rc_(g(151, 5000)), flag1=0x63, flag2=0x93) +
            pair(b"o2", miss_read(80), g(90, 7000), flag1=0x63, flag2=0x93) + pair(b"o3", rc_(g(77, 9000)), miss_read(60), flag1=0x53, flag2=0xA3))


def crlf_text():
    return b"".join([HEAD.replace(b"\n", b"\r\n")] + [mline(b"c%d" % i, 0x43, (H, M)[i % 2](i), eol=b"\r\n") + mline(b"c%d" % i, 0x83, (M, M, H)[i % 3](i + 9), eol=b"\r\n")
                                                       for i in range(7)])


def none_selected_text():
    return HEAD + b"".join(mline(b"u%d" % i, 0x904, H(i)) for i in range(5)) + b"@CO\tnothing is selected\n"


def _build():
    pats = patterns_text()
    out = []
    for rule in (ANY, BOTH):
        for inv in (False, True):
            out.append(case("patterns_%s%s" % (rule, "_inverted" if inv else ""), pats, pair_rule=rule, invert=inv, last=True))
            out.append(case("permille_%s%s" % (rule, "_inverted" if inv else ""), pats, pair_rule=rule, invert=inv, min_hits=2, min_permille=200,
                            last=True))
    names = names_text()
    out += [
        case("tile_seams", tile_seam_text(), last=True),
        case("tile_seams_both_no_header", tile_seam_text(), pair_rule=BOTH, mode=2, last=True),
        case("tiles_on", tiles_on_text(), excl=0x900, last=True),
        case("tiles_on_no_header", tiles_on_text(), excl=0x900, mode=2, last=True),
        case("between_supplementary_mapq_region", between_text(), excl=0x900, sel=BETWEEN_SEL, last=True),
        case("header_between", header_between_text(), last=True),
        case("header_between_no_header", header_between_text(), mode=2, last=True),
        case("names", names, last=True),
        case("names_both_inverted", names, pair_rule=BOTH, invert=True, last=True),
        case("strangers_last_byte", strangers_text("last_byte"), last=True),
        case("strangers_prefix", strangers_text("prefix"), last=True),
        case("strangers_prefix_reversed", strangers_text("prefix_reversed"), last=True),
        case("strangers_first_pair", pair(b"one", H(0), H(1), name2=b"two") + pair(b"g", H(2), H(3)), last=True),
        case("odd_count", patterns_text() + mline(b"lonely", 0x43, H(90))),
        case("odd_count_last", patterns_text() + mline(b"lonely", 0x43, H(90)), last=True),
        case("none_selected", none_selected_text(), excl=0x900, last=True),
        case("none_selected_no_header", none_selected_text(), excl=0x900, mode=2, last=True),
        case("crlf", crlf_text(), last=True),
        case("unterminated_last_line", patterns_text() + pair(b"tail", M(60), H(61))[:-1], last=True),
        case("read_orientation", orientation_text(), orig=True, last=True),
        case("as_stored", orientation_text(), orig=False, last=True),
    ]
    assert len({c.name for c in out}) == len(out)
    return out


_ALL = None
_BLOCKS = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = _build()
    return _ALL


def block_cases():
    """More than one block of 1024 spans and of 1024 tiles; strangers in a later block of spans"""
    global _BLOCKS
    if _BLOCKS is None:
        dense, big = dense_pairs_text(), big_pairs_text()
        _BLOCKS = [case("blocks_dense_k1", dense, k=1, last=True), case("blocks_dense_k1_both_no_header", dense, k=1, pair_rule=BOTH, mode=2, last=True),
                   case("blocks_dense_k1_strangers_in_block_2", dense_pairs_text(bad_at=2301), k=1, last=True),
                   case("blocks_big", big, excl=0x900, last=True), case("blocks_big_inverted_no_header", big, excl=0x900, invert=True, mode=2, last=True)]
    return _BLOCKS


def by_name(name):
    return next(c for c in all_cases() + (_BLOCKS or []) if c.name == name)


def good_cases():
    return [c for c in all_cases() if expected(c).stranger is None and not (c.last and expected(c).odd)]


# ------------------------------------------------------------------------------------------------ what the cases reach
def _selected_lines(c, text=None):
    text = c.text if text is None else text
    return [(s, n) for s, n, kind in classify(c, text) if kind]


def seam_kinds(c):
    """Where the two mates of a pair lie relative to the kernels' seams"""
    kinds, sel = set(), _selected_lines(c)
    all_lines = classify(c, c.text)
    span_of = {}
    i = 0
    for s, n, kind in all_lines:
        if kind or (kind is None and c.mode == 1):
            span_of[s] = i
            i += 1
    for p in range(len(sel) // 2):
        (s1, n1), (s2, n2) = sel[2 * p], sel[2 * p + 1]
        if (s1 + n1) % TILE == 0 and s2 == s1 + n1:
            kinds.add("mate2_at_tile_first_byte")
        if s2 % TILE == TILE - 1 and s2 == s1 + n1:
            kinds.add("mate2_at_tile_last_byte")
        if s2 // TILE - s1 // TILE >= 3 and any(n > 2 * TILE and s1 < s < s2 for s, n, _ in all_lines):
            kinds.add("mate2_tiles_on_behind_a_long_line")
        if span_of[s1] // BLOCK != span_of[s2] // BLOCK:
            kinds.add("span_block_straddled")
        if (s1 // TILE) // BLOCK != (s2 // TILE) // BLOCK:
            kinds.add("tile_block_straddled")
    return kinds


def decision_kinds(c):
    """(mate 1 matches, mate 2 matches, pair rule, invert) of every pair, and whether a per-mille threshold parts two mates"""
    e, kinds = expected(c), set()
    h, w = e.hits.tolist(), e.windows.tolist()
    for p in range(e.n_pairs):
        m = [h[2 * p + j] >= c.min_hits and 1000 * h[2 * p + j] >= c.min_permille * w[2 * p + j] for j in (0, 1)]
        kinds.add((m[0], m[1], c.pair_rule, bool(c.invert)))
        if c.min_permille and m[0] != m[1] and min(h[2 * p], h[2 * p + 1]) >= c.min_hits:
            kinds.add("permille_between_the_mates")
    return kinds


def name_kinds(c):
    kinds, sel = set(), _selected_lines(c)
    for p in range(len(sel) // 2):
        a, b = (name_of(c.text[s:s + n]) for s, n in (sel[2 * p], sel[2 * p + 1]))
        if a == b:
            kinds.add("equal_%d" % len(a))
            if a == b"*":
                kinds.add("star_twice")
        elif a[:-1] == b[:-1] and len(a) == len(b):
            kinds.add("differ_in_the_last_byte")
        elif b.startswith(a) or a.startswith(b):
            kinds.add("one_a_prefix_of_the_other")
        else:
            kinds.add("differ")
    return kinds


def between_kinds(c):
    """What lies between the two mates of a pair"""
    kinds, sel = set(), _selected_lines(c)
    all_lines = classify(c, c.text)
    for p in range(len(sel) // 2):
        s1, s2 = sel[2 * p][0], sel[2 * p + 1][0]
        for s, n, kind in all_lines:
            if not s1 < s < s2:
                continue
            if kind is None:
                kinds.add("header_mode_%d" % c.mode)
                continue
            f = c.text[s:s + n].split(b"\t")
            if int(f[1]) & c.excl & 0x800:
                kinds.add("supplementary")
            elif int(f[4]) < c.sel[1]:
                kinds.add("mapq_floor")
            elif c.sel[2] is not None:
                kinds.add("region")
    return kinds


def cut_sets(c):
    """kind -> the offsets at which the text is cut into windows or chunks for that kind (only the kinds the case can reach)"""
    text, sel = c.text, _selected_lines(c)
    all_lines = classify(c, text)
    out = {}
    if len(sel) >= 2:
        s1, n1 = sel[0]
        s2, n2 = sel[1]
        name = name_of(text[s2:s2 + n2])
        f = text[s2:s2 + n2].split(b"\t")
        seq_at = s2 + sum(len(x) + 1 for x in f[:9])
        out["between_the_mates"] = [s2]
        if len(name) >= 2:
            out["inside_mate_2s_name"] = [s2 + len(name) // 2]
        if len(f[9]) >= 4:
            out["inside_mate_2s_seq"] = [seq_at + len(f[9]) // 2]
        out["every_777"] = list(range(777, len(text), 777))
    for p in range(len(sel) // 2):
        s1, s2 = sel[2 * p][0], sel[2 * p + 1][0]
        mid = [(s, n, kind) for s, n, kind in all_lines if s1 < s < s2]
        hdr = [(s, n) for s, n, kind in mid if kind is None]
        if hdr and "inside_a_header_between_the_mates" not in out:
            out["inside_a_header_between_the_mates"] = [hdr[0][0] + hdr[0][1] // 2]
        uns = [(s, n) for s, n, kind in mid if kind is False]
        if uns and "a_window_of_unselected_lines_behind_a_waiting_mate" not in out:
            out["a_window_of_unselected_lines_behind_a_waiting_mate"] = [uns[0][0], uns[-1][0] + uns[-1][1]]
    return out
