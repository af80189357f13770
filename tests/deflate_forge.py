"""A deflate stream forge for the inflater tests (RFC 1951 / 1952, restated; pure Python, test-only).

zlib's encoder emits only a few of the stream shapes a decoder must take: never a literal-only dynamic block, never a code
of depth 15 under a narrow prefix, never HCLEN = 4, never a repeat code that runs from the literal / length lengths into the
distance lengths.  Other encoders do.  Here the caller controls every field:

- ``Block``: block type, BFINAL, HLIT / HDIST / HCLEN, the code-length code, the literal / length and distance code lengths
  (unused symbols included), how the lengths are run-length coded (16 / 17 / 18, across the HLIT -> HDIST boundary or not,
  or an explicit list), and the exact symbol sequence (literals, EOB, matches, or a length / distance symbol with chosen
  extra bits).  Nothing is validated: invalid symbols are written as asked (symbol mode).
- ``payload_stream``: target bytes and a parse policy -> a stream that inflates to them (payload mode).
- ``gzip_member`` / ``bgzf_member`` / ``bgzf_file``: the containers.
- ``random_stream``: a seeded generator of valid streams, weighted towards deep codes and the worst-case subtable shapes.

Symbols in ``Block.symbols``: an int 0..255 is a literal, 256 the end-of-block code (added at the end unless ``eob=False``);
``("M", length, distance)`` a match in its standard encoding; ``("L", sym, extra)`` a literal / length symbol with the given
value of its extra bits; ``("D", sym, extra)`` a distance symbol with the given value of its extra bits.
"""
import bisect
import heapq
import struct
import zlib

# RFC 1951 3.2.5
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [i // 2 for i in range(2, 28)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8   # 288 codes
FIXED_DIST = [5] * 32                                    # 32 codes (30 and 31 are invalid symbols)

# The deepest shapes: counts of codes per length 1..15 that need the most subtable entries behind an 8-bit (literal /
# length, 286 symbols) and a 5-bit (distance, 30 symbols) primary table — see worst_code() / subtable_entries().
WORST_DIST_COUNTS = [0, 3, 0, 0, 0, 13, 5, 1, 1, 1, 1, 1, 1, 1, 2]


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):               # n bits, least significant first
        assert 0 <= value < (1 << n) or n == 0, (value, n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):           # a Huffman code: most significant bit first
        self.bits(int(format(code, "0%db" % length)[::-1], 2) if length else 0, length)

    @property
    def bit_pos(self):
        return len(self.out) * 8 + self.n

    def align(self, pad_value=0):           # to the next byte boundary, the padding bits = pad_value
        k = (8 - self.n) % 8
        self.bits(pad_value & ((1 << k) - 1), k)
        return k

    def getvalue(self, tail_value=0):
        if self.n:
            return bytes(self.out) + bytes([(self.acc | (tail_value << self.n)) & 0xFF])
        return bytes(self.out)


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the code of every symbol (None for length 0).  Over-subscribed lengths give codes that collide."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l] & ((1 << l) - 1))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft_left(lengths):
    """Code space left free, in units of 2^-15: 0 complete, > 0 incomplete, < 0 over-subscribed."""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


def limited_lengths(freqs, max_bits):
    """Length-limited Huffman code lengths (package-merge); symbols of frequency 0 get no code; one used symbol gets length 1."""
    syms = sorted((f, i) for i, f in enumerate(freqs) if f > 0)
    lengths = [0] * len(freqs)
    if not syms:
        return lengths
    if len(syms) == 1:
        lengths[syms[0][1]] = 1
        return lengths
    assert len(syms) <= (1 << max_bits)
    leaves = [(f, (i,)) for f, i in syms]
    cur = leaves
    for _ in range(max_bits - 1):
        pk = [(cur[j][0] + cur[j + 1][0], cur[j][1] + cur[j + 1][1]) for j in range(0, len(cur) - 1, 2)]
        cur = list(heapq.merge(leaves, pk, key=lambda x: x[0]))
    for _, members in cur[:2 * len(syms) - 2]:
        for i in members:
            lengths[i] += 1
    return lengths


def lengths_from_counts(counts, n_syms, order):
    """Code lengths for n_syms symbols with counts[l - 1] codes of length l, handed out in the order of `order` (a list of
    symbols; the rest get no code)."""
    lens = [0] * n_syms
    k = 0
    for l, c in enumerate(counts, start=1):
        for _ in range(c):
            lens[order[k]] = l
            k += 1
    return lens


def rle_lengths(lens, how="cross"):
    """The code-length symbols of a lengths sequence: a list of (sym, extra).  how: "plain" (no repeats), "greedy" (16 / 17 / 18
    wherever they fit), or a list of split points (each piece coded on its own: [hlit] is what zlib does)."""
    if how == "plain":
        return [(l, 0) for l in lens]
    pieces = [lens] if how in ("cross", "greedy") else [lens[a:b] for a, b in zip([0] + list(how), list(how) + [len(lens)])]
    out = []
    for piece in pieces:
        i = 0
        while i < len(piece):
            l = piece[i]
            run = 1
            while i + run < len(piece) and piece[i + run] == l:
                run += 1
            if l == 0 and run >= 3:
                r = min(run, 138)
                out.append((18, r - 11) if r >= 11 else (17, r - 3))
                i += r
                continue
            out.append((l, 0))
            i += 1
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                i += r
                run -= r
        # (a leftover run of 1 or 2 goes round the loop as plain lengths)
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}


class Block:
    """One deflate block.  kind: "stored", "fixed", "dynamic" or "reserved" (BTYPE 3).  For a dynamic block: lit_lens (HLIT = len), dist_lens
    (HDIST = len); optional overrides hlit / hdist / hclen (the field values written, +257 / +1 / +4 included), cl_lens (19
    code-length code lengths, by symbol), rle ("cross", "greedy", "plain", split points, or an explicit list of (sym, extra)).
    For a stored block: data, and pad_value (the padding bits' value); nlen overrides NLEN."""

    def __init__(self, kind, symbols=(), final=False, lit_lens=None, dist_lens=None, hlit=None, hdist=None, hclen=None,
                 cl_lens=None, rle=None, eob=True, data=b"", pad_value=0, nlen=None, length=None):
        self.kind, self.symbols, self.final, self.eob = kind, list(symbols), final, eob
        self.lit_lens, self.dist_lens = lit_lens, dist_lens
        self.hlit, self.hdist, self.hclen, self.cl_lens, self.rle = hlit, hdist, hclen, cl_lens, rle
        self.data, self.pad_value, self.nlen, self.length = data, pad_value, nlen, length

    def write(self, w):
        w.bits(1 if self.final else 0, 1)
        if self.kind == "reserved":        # BTYPE 3
            w.bits(3, 2)
            return
        if self.kind == "stored":
            w.bits(0, 2)
            w.align(self.pad_value)
            n = len(self.data) if self.length is None else self.length
            w.bits(n, 16)
            w.bits((n ^ 0xFFFF) if self.nlen is None else self.nlen, 16)
            for c in self.data:
                w.bits(c, 8)
            return
        if self.kind == "fixed":
            w.bits(1, 2)
            lit, dist = FIXED_LIT, FIXED_DIST
        else:
            w.bits(2, 2)
            lit, dist = self.lit_lens, self.dist_lens
            self._write_header(w, lit, dist)
        lc, dc = canonical_codes(lit), canonical_codes(dist)

        def put(codes, lens, s):
            if s >= len(codes) or codes[s] is None:
                raise ValueError("symbol %d has no code" % s)
            w.code(codes[s], lens[s])

        syms = self.symbols + ([256] if self.eob else [])
        for s in syms:
            if isinstance(s, int):
                put(lc, lit, s)
            elif s[0] == "M":
                _, length, distance = s
                ls, le = len_symbol(length)
                ds, de = dist_symbol(distance)
                put(lc, lit, ls)
                w.bits(le, LEN_EXTRA[ls - 257])
                put(dc, dist, ds)
                w.bits(de, DIST_EXTRA[ds])
            elif s[0] == "L":
                put(lc, lit, s[1])
                if 257 <= s[1] <= 285:
                    w.bits(s[2], LEN_EXTRA[s[1] - 257])
            elif s[0] == "D":
                put(dc, dist, s[1])
                if s[1] < 30:
                    w.bits(s[2], DIST_EXTRA[s[1]])
            else:
                raise ValueError(s)

    def _write_header(self, w, lit, dist):
        hlit = len(lit) if self.hlit is None else self.hlit
        hdist = len(dist) if self.hdist is None else self.hdist
        if isinstance(self.rle, list) and self.rle and isinstance(self.rle[0], tuple):
            cl_syms = self.rle
        else:
            how = self.rle or "greedy"
            cl_syms = rle_lengths(list(lit) + list(dist), how if how != "split" else [len(lit)])
        cl_lens = self.cl_lens
        if cl_lens is None:
            freq = [0] * 19
            for s, _ in cl_syms:
                freq[s] += 1
            if sum(1 for f in freq if f) == 1:       # (a one-code code-length code is incomplete: zlib refuses it)
                freq[0 if cl_syms[0][0] else 1] += 1
            cl_lens = limited_lengths(freq, 7)
        hclen = self.hclen
        if hclen is None:
            hclen = 19
            while hclen > 4 and cl_lens[CL_ORDER[hclen - 1]] == 0:
                hclen -= 1
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for i in range(hclen):
            w.bits(cl_lens[CL_ORDER[i]], 3)
        cc = canonical_codes(cl_lens)
        for s, extra in cl_syms:
            if cc[s] is None:
                raise ValueError("code-length symbol %d has no code" % s)
            w.code(cc[s], cl_lens[s])
            if s >= 16:
                w.bits(extra, CL_EXTRA[s])


def len_symbol(length):
    assert 3 <= length <= 258
    if length == 258:
        return 285, 0
    for i in range(27, -1, -1):
        if LEN_BASE[i] <= length:
            return 257 + i, length - LEN_BASE[i]


def dist_symbol(distance):
    assert 1 <= distance <= 32768
    for i in range(29, -1, -1):
        if DIST_BASE[i] <= distance:
            return i, distance - DIST_BASE[i]


def stream(blocks, tail=b"", tail_bits=0):
    """The blocks as one raw deflate stream; tail: bytes behind the final block; tail_bits: the value of the last byte's
    unused high bits."""
    w = BitWriter()
    for b in blocks:
        b.write(w)
    return w.getvalue(tail_bits) + tail


def expand(blocks):
    """The bytes the blocks decode to as far as their symbols are well-formed (distances in range, no symbol 286 / 287 /
    distance 30 / 31); code shapes are not checked.  None if a symbol is not well-formed."""
    out = bytearray()
    for b in blocks:
        if b.kind == "stored":
            out += b.data
            continue
        pend = None
        for s in b.symbols:
            if isinstance(s, int):
                if s > 256:
                    return None
                out.append(s)
                continue
            if s[0] == "M":
                length, distance = s[1], s[2]
            elif s[0] == "L":
                if not 257 <= s[1] <= 285:
                    return None
                pend = LEN_BASE[s[1] - 257] + s[2]
                continue
            else:
                if s[1] >= 30 or pend is None:
                    return None
                length, distance, pend = pend, DIST_BASE[s[1]] + s[2], None
            if distance > len(out):
                return None
            for _ in range(length):
                out.append(out[-distance])
    return bytes(out)


# ---------------------------------------------------------------- payload mode
def parse(data, policy="greedy", start=0, window=32768, chain=16):
    """data[start:] as tokens (int literal, or ("M", length, distance)) with data[:start] as history.  policy: "literals",
    "greedy", "runs258" (distance-1 runs of up to 258 wherever the byte repeats, greedy elsewhere), "maxdist" (the farthest
    match of at least 3 bytes within the window)."""
    toks = []
    if policy == "literals":
        return list(data[start:])
    heads = {}
    n = len(data)

    def insert(p):
        if p + 3 <= n:
            heads.setdefault(data[p:p + 3], []).append(p)

    for p in range(max(0, start - window), start):
        insert(p)
    i = start
    while i < n:
        best_l, best_d = 0, 0
        if policy == "runs258" and i > 0 and data[i] == data[i - 1]:
            l = 0
            while i + l < n and l < 258 and data[i + l] == data[i - 1]:
                l += 1
            if l >= 3:
                best_l, best_d = l, 1
        if not best_l and i + 3 <= n:
            cands = heads.get(data[i:i + 3], [])
            if policy == "maxdist":              # the farthest candidates first
                k = bisect.bisect_left(cands, i - window)
                cands = cands[k:k + chain]
            else:                                # the nearest first
                cands = [c for c in reversed(cands[-chain:]) if i - c <= window]
            for c in cands:
                l = 0
                while i + l < n and l < 258 and data[c + l] == data[i + l]:
                    l += 1
                if l > best_l or (policy == "maxdist" and l >= 3 and best_l < 3):
                    best_l, best_d = l, i - c
                if policy == "maxdist" and best_l >= 3:
                    break
        if best_l >= 3:
            toks.append(("M", best_l, best_d))
            for p in range(i, i + best_l):
                insert(p)
            i += best_l
        else:
            toks.append(data[i])
            insert(i)
            i += 1
    return toks


def tok_len(t):
    return 1 if isinstance(t, int) else t[1]


def code_for(toks, kind, rng=None, max_bits=15, deep=False):
    """(lit_lens, dist_lens) for a dynamic block of these tokens: length-limited Huffman of their frequencies, or (deep) a
    random deep complete code over every symbol (rng)."""
    lf, df = [0] * 286, [0] * 30
    lf[256] = 1
    for t in toks:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[len_symbol(t[1])[0]] += 1
            df[dist_symbol(t[2])[0]] += 1
    if deep:
        return random_code(rng, 286, lf), random_code(rng, 30, df, dist=True)
    lit = limited_lengths(lf, max_bits)
    dist = limited_lengths(df, max_bits)
    hlit = max(257, max(i for i, l in enumerate(lit) if l) + 1)
    used_d = [i for i, l in enumerate(dist) if l]
    hdist = max(used_d) + 1 if used_d else 1
    return lit[:hlit], dist[:hdist]


def payload_stream(data, policy="greedy", splits=None, kinds=None, rng=None, deep=False, tail=b""):
    """A stream that inflates to `data`.  The whole input is parsed once (matches reach back across block boundaries and into
    stored blocks); splits: byte offsets where blocks end (the token boundary at or after each); kinds: the type of each
    block ("dynamic", "fixed", "stored"; default dynamic).  Returns (stream bytes, blocks)."""
    toks = parse(data, policy)
    cuts = sorted(set(splits or []))
    groups, cur, pos = [], [], 0
    for t in toks:
        cur.append(t)
        pos += tok_len(t)
        while cuts and cuts[0] <= pos:
            cuts.pop(0)
            groups.append(cur)
            cur = []
    groups.append(cur)
    blocks, pos = [], 0
    for gi, g in enumerate(groups):
        kind = (kinds[gi % len(kinds)] if kinds else "dynamic")
        n = sum(tok_len(t) for t in g)
        if kind == "stored":
            chunk = data[pos:pos + n]
            pieces = [chunk[j:j + 65535] for j in range(0, len(chunk), 65535)] or [b""]
            blocks += [Block("stored", data=p) for p in pieces]
        elif kind == "fixed":
            blocks.append(Block("fixed", g))
        else:
            lit, dist = code_for(g, kind, rng=rng, deep=deep)
            blocks.append(Block("dynamic", g, lit_lens=lit, dist_lens=dist,
                                rle=(rng.choice(["greedy", "split", "plain"]) if rng is not None else "greedy")))
        pos += n
    blocks[-1].final = True
    return stream(blocks, tail), blocks


# ---------------------------------------------------------------- random valid codes and streams
def random_code(rng, n, freq, dist=False):
    """A random complete code over n symbols that gives every symbol with freq > 0 a code: deep (lengths up to 15) with a fair
    chance, or the worst-case subtable shape."""
    used = [i for i in range(n) if freq[i]]
    r = rng.random()
    if dist and r < 0.25:
        order = list(range(n))
        rng.shuffle(order)
        return lengths_from_counts(WORST_DIST_COUNTS, n, order)
    if not dist and r < 0.2:
        counts = worst_code(286, 8)[1]
        if len(used) <= sum(counts):
            return _fill(counts, n, used, rng)
    if len(used) <= 1 and rng.random() < 0.5:     # a single code of length 1, or none (distances)
        lens = [0] * n
        if used:
            lens[used[0]] = 1
        return lens
    extra = [i for i in range(n) if not freq[i] and rng.random() < 0.5]
    syms = sorted(set(used + extra)) if len(used) + len(extra) >= 2 else list(range(n))
    weights = [0] * n
    depth = rng.choice([4, 8, 12, 20, 40])
    for s in syms:
        weights[s] = max(1, int(2 ** (rng.random() * depth)))
    return limited_lengths(weights, 15)


def _fill(counts, n, used, rng):
    order = used + [i for i in range(n) if i not in used]
    rest = order[len(used):]
    rng.shuffle(rest)
    head = order[:len(used)]
    rng.shuffle(head)
    return lengths_from_counts(counts, n, head + rest)


def random_stream(rng, data, max_blocks=6):
    """A random valid stream of `data` (random.Random rng): random parse policy, block splits and types, random codes (deep
    ones and the worst subtable shapes among them).  Returns (stream bytes, blocks)."""
    policy = rng.choice(["literals", "greedy", "greedy", "runs258", "maxdist"])
    nb = rng.randint(1, max_blocks)
    splits = sorted(rng.randrange(0, len(data) + 1) for _ in range(nb - 1))
    kinds = [rng.choice(["dynamic", "dynamic", "dynamic", "fixed", "stored"]) for _ in range(nb)]
    return payload_stream(data, policy, splits, kinds, rng=rng, deep=rng.random() < 0.7)


# ---------------------------------------------------------------- the exact subtable bounds
def _worst(n, root, maxlen=15):
    import functools

    @functools.lru_cache(maxsize=None)
    def f(l, syms, left):
        # codes of length l .. maxlen fill `left` free codes of length l; the long codes lie in canonical order, so the root
        # slot being filled is the one `left` ends inside: it is (-left) mod S full, S = 2^(l - root) codes of length l.  A
        # slot that fills up at length l needs a subtable of S entries.  Returns (entries, counts per length l..) or None.
        S = 1 << (l - root)
        fill = (-left) % S
        best = None
        lo = max(0, 2 * left - syms) if l < maxlen else left
        for c in range(lo, min(left, syms) + 1):
            cost = (fill + c) // S * S
            if c == left:
                cand = (cost, (c,))
            else:
                r = f(l + 1, syms - c, 2 * (left - c))
                cand = None if r is None else (cost + r[0], (c,) + r[1])
            if cand is not None and (best is None or cand[0] > best[0]):
                best = cand
        return best

    best = (0, None)
    for left in range(1, (1 << root) + 1):
        used = (1 << root) - left          # code space of the short codes, in codes of length root: the fewest codes
        short = [(used >> (root - l)) & 1 for l in range(1, root + 1)]
        syms = n - sum(short)
        if syms < 0 or 2 * left > syms:
            continue
        r = f(root + 1, syms, 2 * left)
        if r is not None and r[0] > best[0]:
            best = (r[0], short + list(r[1]) + [0] * (maxlen - root - len(r[1])))
    return best


_WORST = {}


def worst_code(n, root):
    """(entries, counts per length 1..15): the complete code of at most n symbols with the most subtable entries behind a
    root-bit primary table (the method of zlib's examples/enough.c, restated as a memoized search).  Incomplete codes that a
    decoder accepts (one code of length 1, or none) need no subtable."""
    if (n, root) not in _WORST:
        _WORST[(n, root)] = _worst(n, root)
    return _WORST[(n, root)]


def subtable_entries(lengths, root):
    """Subtable entries a table builder that sizes each subtable by the longest code under its root index needs."""
    codes = canonical_codes(lengths)
    longest = {}
    for c, l in zip(codes, lengths):
        if l > root:
            p = c >> (l - root)
            longest[p] = max(longest.get(p, 0), l)
    return sum(1 << (l - root) for l in longest.values())


# ---------------------------------------------------------------- containers
def gzip_member(raw, data, mtime=0, fname=None, comment=None, extra=None, fhcrc=False, xfl=0, os_=255):
    """A gzip member around the raw deflate stream `raw` whose output is `data` (for CRC32 / ISIZE)."""
    flg = (4 if extra is not None else 0) | (8 if fname is not None else 0) | (16 if comment is not None else 0) | (2 if fhcrc else 0)
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + bytes([xfl, os_]))
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if fname is not None:
        h += fname + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if fhcrc:
        h += struct.pack("<H", zlib.crc32(bytes(h)) & 0xFFFF)
    return bytes(h) + raw + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data) & 0xFFFFFFFF)


def bgzf_member(raw, data):
    """A BGZF member (the BC subfield with BSIZE) around `raw`; at most 64 KiB in and out."""
    bsize = 18 + len(raw) + 8
    assert bsize <= 65536 and len(data) <= 65536, (bsize, len(data))
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + raw +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_file(members, eof=True):
    return b"".join(members) + (BGZF_EOF if eof else b"")


# ---------------------------------------------------------------- the catalogue of named shapes
def _dyn(toks, lit=None, dist=None, final=True, **kw):
    if lit is None or dist is None:
        l2, d2 = code_for(toks, "dynamic")
        lit = l2 if lit is None else lit
        dist = d2 if dist is None else dist
    return Block("dynamic", toks, final=final, lit_lens=lit, dist_lens=dist, **kw)


def _lits(data):
    return list(data)


def _every_dist_symbol(rng):
    """Tokens whose matches use all 30 distance symbols (history: 32 KiB of text first)."""
    hist = bytes(rng.choice(b"ACGT\n@+F:#") for _ in range(32768))
    toks = list(hist)
    for ds in range(30):
        extra = rng.randrange(1 << DIST_EXTRA[ds]) if DIST_EXTRA[ds] else 0
        toks.append(("M", rng.randint(3, 258), DIST_BASE[ds] + extra))
    return toks


def catalogue(seed=0):
    """{name: (blocks, tail)}: every shape the tests name.  Inflate with stream(blocks, tail)."""
    import random
    rng = random.Random(seed)
    text = bytes(rng.choice(b"ACGTN\n@+FFF:,#") for _ in range(3000))
    C = {}
    # literal-only dynamic blocks: HDIST = 1 with length 0, and 30 zero lengths
    C["literal_only_hdist1"] = ([_dyn(_lits(text[:500]), dist=[0])], b"")
    C["literal_only_hdist30"] = ([_dyn(_lits(text[:500]), dist=[0] * 30)], b"")
    # a single distance code of length 1 (accepted), of length 2 and 15, two codes of length 3 (refused: zlib's rule)
    runs = [65, ("M", 200, 1), 66, ("M", 100, 1)]
    C["one_dist_code_len1"] = ([_dyn(runs, dist=[1])], b"")
    C["one_dist_code_len1_symbol9"] = ([_dyn(list(text[:100]) + [("M", 40, 30)], dist=[0] * 9 + [1])], b"")
    C["one_dist_code_len2"] = ([_dyn(runs, dist=[2])], b"")
    C["one_dist_code_len15"] = ([_dyn(runs, dist=[15])], b"")
    C["two_dist_codes_len3"] = ([_dyn(runs + [("M", 5, 2)], dist=[3, 3])], b"")
    C["one_lit_code_eob_len2"] = ([_dyn([], lit=[0] * 256 + [2], dist=[0])], b"")
    # the worst subtable shapes: the 1040-entry distance codes, the 404-entry literal / length code
    toks = _every_dist_symbol(rng)
    for name, counts in (("dist_1040_issue", WORST_DIST_COUNTS), ("dist_1040_search", worst_code(30, 5)[1])):
        for k in range(3):
            order = list(range(30))
            if k:
                rng.shuffle(order)
            C["%s_%d" % (name, k)] = ([_dyn(toks, dist=lengths_from_counts(counts, 30, order))], b"")
    lc = worst_code(286, 8)[1]
    for k in range(3):
        order = list(range(286))
        if k:
            rng.shuffle(order)
        lit = lengths_from_counts(lc, 286, order)
        C["lit_404_%d" % k] = ([_dyn(list(range(256)) * 2 + [("M", 3 + j, 1 + j) for j in range(256)], lit=lit)], b"")
    # HCLEN = 4 (only 16 17 18 0: no length can be nonzero, so no end-of-block code: refused), and HCLEN = 19 padded with zeros
    C["hclen4"] = ([Block("dynamic", [], final=True, lit_lens=[0] * 257, dist_lens=[0], hclen=4,
                          cl_lens=[1] + [0] * 16 + [0, 1], rle=[(18, 127), (18, 127), (0, 0), (0, 0), (0, 0), (0, 0)], eob=False)], b"")
    C["hclen19"] = ([_dyn(list(text[:300]), hclen=19)], b"")
    # repeat codes that run from the literal / length lengths into the distance lengths, and ones that overshoot
    lit16 = [9] * 48 + [8] * 232 + [0] * 6                                  # 280 codes: 48 x 9 + 232 x 8 bits, complete
    t16 = list(text[:400]) + [("M", 10, 17), ("M", 20, 200), ("M", 7, 40)]
    C["rle18_crosses"] = ([_dyn(t16, lit=lit16, dist=[0] * 8 + [4] * 16)], b"")            # 6 + 8 zeros: an 18
    C["rle17_crosses"] = ([_dyn([x for x in t16 if x != ("M", 10, 17)] + [("M", 9, 5)], lit=lit16, dist=[0] * 2 + [4] * 16)], b"")
    lit_d = [9] * 60 + [8] * 226                                            # 226 x 8 + 60 x 9 bits, complete, ends in 8s
    C["rle16_crosses"] = ([_dyn(list(text[:300]) + [("M", 5, 1), ("M", 6, 3), ("M", 3, 8)], lit=lit_d,
                                dist=[8, 8, 8, 8, 1, 2, 3, 4, 5, 6])], b"")
    C["rle_split_like_zlib"] = ([_dyn(t16, lit=lit16, dist=[0] * 8 + [4] * 16, rle="split")], b"")
    C["rle_plain"] = ([_dyn(t16, lit=lit16, dist=[0] * 8 + [4] * 16, rle="plain")], b"")
    over = rle_lengths(lit16 + [0] * 8 + [4] * 16)
    C["rle18_overshoots"] = ([_dyn(t16, lit=lit16, dist=[0] * 8 + [4] * 16, rle=over[:-1] + [(18, 20)])], b"")
    C["rle16_overshoots"] = ([_dyn(t16, lit=lit16, dist=[0] * 8 + [4] * 16,
                                   rle=rle_lengths(lit16 + [0] * 8 + [4] * 14) + [(4, 0), (16, 3)])], b"")   # 5 too many
    C["rle16_first"] = ([_dyn(t16, lit=lit16, dist=[0] * 8 + [4] * 16, rle=[(16, 0)] + over)], b"")
    # lengths: 258 via symbol 285, symbol 284 with extra bits 31
    C["len258_sym285"] = ([_dyn([ord("A")] + [("M", 258, 1)] * 40 + list(text[:50]) + [("M", 258, 50)])], b"")
    C["sym284_extra31"] = ([_dyn([ord("A"), ord("C")] + [("L", 284, 31), ("D", 1, 0)] * 3 + [("L", 284, 30), ("D", 0, 0)],
                                 lit=[8] * 253 + [0] * 3 + [8] + [0] * 27 + [8, 8], dist=[1, 1])], b"")
    # overlapping copies at distance 1 .. 16
    for d in range(1, 17):
        C["overlap_d%d" % d] = ([_dyn(list(text[:d]) + [("M", 3 + 17 * d % 256, d), ("M", 258, d), ("M", 3, d)])], b"")
    # distance 32768 at exactly 32 KiB of output, and one byte short of that (refused)
    big = bytes(rng.randrange(256) for _ in range(32768))
    C["dist32768_at_32k"] = ([Block("stored", data=big), Block("fixed", [("M", 258, 32768), ("M", 3, 32768)], final=True)], b"")
    C["dist32768_at_32k_minus1"] = ([Block("stored", data=big[:-1]), Block("fixed", [("M", 258, 32768)], final=True)], b"")
    C["dist_before_start"] = ([_dyn(list(text[:10]) + [("M", 5, 11)])], b"")
    # the fixed code's symbols that do not exist: literal / length 286 / 287, distance 30 / 31
    for s in (286, 287):
        C["fixed_lit%d" % s] = ([Block("fixed", list(text[:20]) + [("L", s, 0)], final=True)], b"")
    for s in (30, 31):
        C["fixed_dist%d" % s] = ([Block("fixed", list(text[:20]) + [("L", 257, 0), ("D", s, 0)], final=True)], b"")
    # stored blocks of length 0 and 65535 at every bit offset, a NLEN mismatch
    for off in range(8):
        for n in (0, 65535):
            data = bytes(rng.randrange(256) for _ in range(n)) if n else b""
            pre = Block("fixed", [200] * ((off - 2) % 8) + list(text[:3]))   # (3 + 9 m + 8 * 3 + 7 bits: offset 2 + m)
            C["stored%d_bitoff%d" % (n, off)] = ([pre, Block("stored", data=data, pad_value=0x55 >> (off % 2)),
                                                  Block("fixed", [("M", 20, min(n, 32768))] if n else [1], final=True)], b"")
    C["stored_nlen_mismatch"] = ([Block("stored", data=text[:100], nlen=(100 ^ 0xFFFF) ^ 0x0100, final=True)], b"")
    C["stored_beyond_input"] = ([Block("stored", data=text[:100], length=200, final=True)], b"")
    # empty blocks
    C["empty_dynamic_eob_only"] = ([_dyn([], lit=[0] * 256 + [1], dist=[0])], b"")
    C["empty_dynamic_two_codes"] = ([_dyn([], lit=[0] * 65 + [1] + [0] * 190 + [1], dist=[0])], b"")
    C["empty_fixed_then_stored_empty"] = ([Block("fixed", []), Block("stored", final=True)], b"")
    # several blocks whose matches reach back into earlier blocks (stored ones too)
    data = (text * 4)[:9000]
    for pol in ("greedy", "runs258", "maxdist", "literals"):
        s, blocks = payload_stream(data, pol, splits=[700, 2500, 2600, 5000, 7000],
                                   kinds=["dynamic", "stored", "fixed", "dynamic", "stored", "dynamic"])
        C["blocks_reach_back_%s" % pol] = (blocks, b"")
    # bytes after the final block
    C["bytes_after_final"] = ([_dyn(list(text[:200]))], b"\x00\xffgarbage")
    C["no_final_block"] = ([_dyn(list(text[:200]), final=False)], b"")
    C["reserved_btype"] = ([Block("fixed", list(text[:10])), Block("reserved", final=True)], b"\x00" * 4)
    return C
