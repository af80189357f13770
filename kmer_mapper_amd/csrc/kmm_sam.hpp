// kmm_sam.hpp — part of libkmm: SAM text records (SAM/BAM specification 1.4) turned into two-line FASTA ON THE GPU
// (KMM_FORMAT_SAM; included by kmm.hip — the host side is kmm_sam_host.hpp —, compiled by itself with g++ in tests/test_sam_on_the_cpu.py, where the same per-line
// steps run on the CPU).
//
// The QNAME grammar [!-?A-~]{1,254} cannot start with '@', so every line of a SAM stream is either a header line (first byte
// '@') or one whole record: every newline is an exact record boundary.  A chunk in HBM (at most 2^30 bytes: one piece of
// kmm_map_records) is cut into tiles of TILE bytes; the tile in which a line STARTS owns it, however long it is:
//   1. count   one wavefront per tile finds its first line start (the first newline at or after the tile's start), then
//              walks its lines: per line, 64 lanes read 16 bytes each per step (a 1 KiB window, aligned 16-byte loads) and
//              find the newline and TABs 1, 2, 9 and 10 with ballots and a lane prefix sum.  From those: header / record,
//              FLAG, the SEQ range, the flag filter, the output length; the first malformed line of the tile;
//   2. totals  the tiles' output offsets (an exclusive scan), records, exclusions, header lines, the end of the last complete
//              line (= *consumed) and the first error;
//   3. write   the same walk again, every kept record written as ">\n" SEQ "\n" (SEQ "*": an empty line), 64 lanes per SEQ.
// kmm_map_records then maps that text as two-line FASTA: the LUT, the invalid-base rule and the radix / direct choice are the
// ones every other input takes.  Every read is bounds-checked against n.
// The quality variant (<true> / k_sam_*_q; "use_record_qual" with a floor) also finds TAB 11, checks that QUAL is
// "*" or as long as SEQ, and writes every kept record as four-line FASTQ ("@\n" SEQ "\n+\n" QUAL "\n"; QUAL "*": '~' per base),
// 2 |SEQ| + 6 bytes per record, which the library maps as KMM_FORMAT_FASTQ, where "min_base_quality" is applied.
// "original_strand"  has the write pass emit the kept records whose FLAG has 0x10 in read orientation: SEQ reversed
// and complemented letter by letter, QUAL reversed.  The output lengths are the same: the count pass does not know of the switch.
// Record selection (kmm_select.hpp has the rule): with an include mask, a MAPQ floor or a region list set, the count
// and write passes run as their <.., true> / k_sam_*_sel forms: the line scan also finds TABs 3 to 6, and classify_sel reads, of
// the records that pass the flag masks, MAPQ (with a floor) and RNAME, POS and CIGAR (with regions; RNAME looked up in the
// handle's name table, POS and CIGAR read only of records on a listed reference).  A field that is read and malformed fails the
// call (ERR_MAPQ, ERR_POS, ERR_CIGAR); a field no rule needs is not looked at.
// The raw form ("record_sam"): the write pass also leaves one span per line it considers (walk_tile<.., H = true> with
// a SpanSink: the k_sam_write_spans* kernels); behind the inner records call k_sam_raw_flags asks the keep rule of every span's
// entry and k_sam_raw_copy moves the kept lines, untouched, behind the keep queue's tail.  No further walk over the lines.
#pragma once

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "kmm_bam.hpp" // (the raw form: the keep rule rk_keep, and raw_copy_part, a lane's share of a copy into the keep queue)
#include "kmm_select.hpp"

#if defined(__HIPCC__)
#define KMM_SAM_HD __host__ __device__ __forceinline__
#else
#define KMM_SAM_HD inline
#endif

namespace kmm_sam {

constexpr uint64_t NONE = ~0ull;
constexpr uint32_t TILE = 1024;       // bytes per tile (the lines that start in it are its own)
constexpr uint32_t WIN = 1024;        // bytes one wavefront reads per step of a line: 64 lanes x 16 bytes
enum Err : uint32_t { ERR_QUAL = 0, ERR_FIELDS = 1, ERR_FLAG = 2, ERR_EMPTY = 3, ERR_MAPQ = 4, ERR_POS = 5, ERR_CIGAR = 6 };
// an error word = line start << 2 | code; with a selection (S: codes up to 6) line start << 3 | code
// (ERR_QUAL: the quality variant only — QUAL is not "*" and not as long as SEQ.  With a selection only: ERR_MAPQ — MAPQ is not a
// decimal integer in [0, 255]; ERR_POS — POS is not one in [0, 2^31 - 1]; ERR_CIGAR — CIGAR is neither "*" nor
// ([0-9]+[MIDNSHP=X])+ with every length in [0, 2^28 - 1])
using kmm_sel::Sel;
template <bool S>
KMM_SAM_HD uint32_t err_shift() { return S ? 3u : 2u; }
enum Kind : uint32_t { K_KEPT = 0, K_EXCLUDED = 1, K_HEADER = 2, K_BAD = 3 };

// One tile's lines: records kept / excluded, header lines, output bytes, the end of its last complete line (0: none), the
// first malformed line (NONE: none).  bytes is uint32: a piece holds at most 2^30 bytes, the SEQs of the lines that start in one
// tile lie in it one behind the other, and at most TILE lines start there: at most 2 * 2^30 + 6 * TILE output bytes, four-line
// FASTQ included.
struct Tile {
    uint32_t recs, excluded, headers, bytes;
    uint64_t last_end, err;
};

struct Totals {
    unsigned long long recs, excluded, headers, out_bytes, consumed, err;
};

// Where a line's fields lie: its newline (NONE: no newline before n), TABs 1, 2, 9 and 10 (NONE: the line has fewer); the
// quality variant (NT = 5) also looks for TAB 11, behind QUAL
template <int NT>
struct LineT {
    uint64_t end;
    uint64_t tab[NT];
};
typedef LineT<4> Line;
typedef LineT<5> LineQ;
// NT 4 / 5: TABs 1, 2, 9, 10, 11; with a selection (NT 8 / 9): 1 to 6, 9, 10, 11
template <int NT>
KMM_SAM_HD uint32_t want_tab(int w)
{
    if (NT >= 8)
        return w < 6 ? (uint32_t)w + 1u : (uint32_t)w + 3u;
    return w < 2 ? (uint32_t)w + 1u : (uint32_t)w + 7u;
}

struct LineInfo {
    uint32_t kind, err;
    uint64_t seq, seq_len; // SEQ of a record ("*": length 0)
    bool rev;              // FLAG has 0x10: the record is stored reverse-complemented
    uint32_t flag;         // FLAG of a record
};
struct LineInfoQ : LineInfo {
    uint64_t qual; // QUAL of a record: seq_len bytes at d[qual], or
    bool absent;   // "*": the record stores no qualities
};

// TAB / newline masks of one lane's 16 bytes d[a + 16 lane, +16), restricted to [s, n).  d + a is 16-byte aligned; on the
// device a block wholly inside [0, n) is one 16-byte load, anything else (the chunk's ends) is read byte by byte.
KMM_SAM_HD void lane_masks(const uint8_t *d, uint64_t n, uint64_t s, int64_t a, uint32_t lane, uint32_t &tab, uint32_t &nl)
{
    const int64_t p = a + 16 * (int64_t)lane;
    tab = nl = 0;
#if defined(__HIP_DEVICE_COMPILE__)
    if (p >= 0 && p + 16 <= (int64_t)n) {
        typedef uint32_t v4 __attribute__((ext_vector_type(4)));
        const v4 x = *reinterpret_cast<const v4 *>(d + p);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const uint32_t c = (x[i] >> (8 * b)) & 255u;
                tab |= (c == 9u ? 1u : 0u) << (4 * i + b);
                nl |= (c == 10u ? 1u : 0u) << (4 * i + b);
            }
        const int64_t lo = (int64_t)s - p; // bytes of the block before s
        if (lo > 0) {
            const uint32_t keep = lo >= 16 ? 0u : ~((1u << lo) - 1u);
            tab &= keep;
            nl &= keep;
        }
        return;
    }
#endif
    for (int i = 0; i < 16; ++i) {
        const int64_t q = p + i;
        if (q < (int64_t)s || q < 0 || q >= (int64_t)n)
            continue;
        const uint32_t c = d[q];
        tab |= (c == 9u ? 1u : 0u) << i;
        nl |= (c == 10u ? 1u : 0u) << i;
    }
}

// position (0..15) of the k-th (1-based) set bit of m; m has at least k set bits
KMM_SAM_HD uint32_t nth_bit(uint32_t m, uint32_t k)
{
    for (uint32_t i = 1; i < k; ++i)
        m &= m - 1u;
    uint32_t b = 0;
    while (!((m >> b) & 1u))
        ++b;
    return b;
}

// The first window of a line that starts at s: its start is s rounded down to the 16-byte alignment of the address d + s.
KMM_SAM_HD int64_t first_window(const uint8_t *d, uint64_t s)
{
    return (int64_t)s - (int64_t)(((uintptr_t)d + s) & 15u);
}

// What the line [s, L.end) is.  L.end != NONE.
KMM_SAM_HD void classify(const uint8_t *d, uint64_t s, const Line &L, uint32_t excl, LineInfo &o)
{
    o.kind = K_BAD;
    o.err = 0;
    o.seq = o.seq_len = 0;
    o.rev = false;
    o.flag = 0;
    const uint64_t e = L.end;
    if (e == s || (e == s + 1 && d[s] == 13u)) {
        o.err = ERR_EMPTY;
        return;
    }
    if (d[s] == (uint8_t)'@') {
        o.kind = K_HEADER;
        return;
    }
    if (L.tab[3] == NONE) { // (fewer than 10 TABs before the newline)
        o.err = ERR_FIELDS;
        return;
    }
    const uint64_t f0 = L.tab[0] + 1, f1 = L.tab[1];
    uint32_t flag = 0;
    bool ok = f1 > f0;
    for (uint64_t q = f0; q < f1 && ok; ++q) {
        const uint32_t c = d[q];
        ok = c >= (uint32_t)'0' && c <= (uint32_t)'9';
        flag = flag * 10u + (c - (uint32_t)'0');
        ok = ok && flag <= 0xFFFFu;
    }
    if (!ok) {
        o.err = ERR_FLAG;
        return;
    }
    o.seq = L.tab[2] + 1;
    o.seq_len = L.tab[3] - o.seq;
    if (o.seq_len == 1 && d[o.seq] == (uint8_t)'*')
        o.seq_len = 0;
    o.kind = (flag & excl) ? K_EXCLUDED : K_KEPT;
    o.rev = (flag & 0x10u) != 0u;
    o.flag = flag;
}

// The quality variant: what the line is, and its QUAL — the bytes between TAB 10 and TAB 11 (or the line's end, without a CR in
// front of the newline).  A QUAL that is exactly "*" is absent, for a one-base read too (as htslib reads it); any other QUAL has
// to be as long as SEQ.
KMM_SAM_HD void classify(const uint8_t *d, uint64_t s, const LineQ &L, uint32_t excl, LineInfoQ &o)
{
    Line l4;
    l4.end = L.end;
    for (int w = 0; w < 4; ++w)
        l4.tab[w] = L.tab[w];
    classify(d, s, l4, excl, o);
    o.qual = 0;
    o.absent = false;
    if (o.kind != K_KEPT && o.kind != K_EXCLUDED)
        return;
    const uint64_t qs = L.tab[3] + 1;
    uint64_t qe = L.tab[4];
    if (qe == NONE) {
        qe = L.end;
        if (qe > qs && d[qe - 1] == 13u)
            --qe;
    }
    o.qual = qs;
    o.absent = qe - qs == 1 && d[qs] == (uint8_t)'*';
    if (!o.absent && qe - qs != o.seq_len) {
        o.kind = K_BAD;
        o.err = ERR_QUAL;
    }
}

// ---- record selection ----

// The decimal field d[b, e): false when it is empty, holds anything but digits, or exceeds max.
KMM_SAM_HD bool parse_decimal(const uint8_t *d, uint64_t b, uint64_t e, uint64_t max, uint64_t &v)
{
    v = 0;
    bool ok = e > b;
    for (uint64_t q = b; q < e && ok; ++q) {
        const uint32_t c = d[q];
        ok = c >= (uint32_t)'0' && c <= (uint32_t)'9';
        v = v * 10u + (c - (uint32_t)'0');
        ok = ok && v <= max;
    }
    return ok;
}

KMM_SAM_HD bool is_digit(uint32_t c) { return c >= (uint32_t)'0' && c <= (uint32_t)'9'; }

// The BAM code (0..8) of a CIGAR operation letter, 15: none
KMM_SAM_HD uint32_t cigar_op(uint32_t c)
{
    switch (c) {
    case 'M': return 0u;
    case 'I': return 1u;
    case 'D': return 2u;
    case 'N': return 3u;
    case 'S': return 4u;
    case 'H': return 5u;
    case 'P': return 6u;
    case '=': return 7u;
    case 'X': return 8u;
    default: return 15u;
    }
}

// The CIGAR text d[b, e) (not "*", not empty), the share of lane `lane` of `lanes`: the bytes b + lane, b + lane + lanes, ...
// Every byte is judged where it stands, so the lanes need nothing of each other: a digit needs a byte behind it; an operation
// letter needs the digits in front of it, which it reads (its length; M, D, N, = and X add it to span); any other byte is
// malformed.  Together the lanes accept exactly ([0-9]+[MIDNSHP=X])+ with every length <= 2^28 - 1.
KMM_SAM_HD bool cigar_text_part(const uint8_t *d, uint64_t b, uint64_t e, uint32_t lane, uint32_t lanes, uint64_t &span)
{
    bool ok = true;
    for (uint64_t i = b + lane; i < e; i += lanes) {
        const uint32_t c = d[i];
        if (is_digit(c)) {
            ok = ok && i + 1 < e;
            continue;
        }
        const uint32_t op = cigar_op(c);
        uint64_t q = i;
        while (q > b && is_digit(d[q - 1]))
            --q;
        uint64_t v = 0;
        for (uint64_t r = q; r < i; ++r) {
            v = v * 10u + (d[r] - (uint32_t)'0');
            if (v > kmm_sel::MAX_CIGAR_LEN)
                v = kmm_sel::MAX_CIGAR_LEN + 1ull; // (too long, however many digits follow)
        }
        ok = ok && op != 15u && q < i && v <= kmm_sel::MAX_CIGAR_LEN;
        if (op != 15u && kmm_sel::consumes_ref(op))
            span += v;
    }
    return ok;
}

// The index of the name d[b, e) in the selection's name table, -1: not there (compared exactly and whole)
KMM_SAM_HD int64_t find_name(const Sel &sel, const uint8_t *d, uint64_t b, uint64_t e)
{
    for (uint32_t i = 0; i < sel.n_names; ++i) {
        const uint32_t o = sel.name_off[i], len = sel.name_off[i + 1] - o;
        if ((uint64_t)len != e - b)
            continue;
        bool same = true;
        for (uint32_t j = 0; j < len && same; ++j)
            same = sel.names[o + j] == d[b + j];
        if (same)
            return (int64_t)i;
    }
    return -1;
}

// What the line is under a selection.  L holds TABs 1 to 6, 9, 10 (and 11: the quality variant).  The line's class, FLAG, SEQ and
// (quality variant) QUAL are judged as without a selection; then, of a record, the rules in turn — each field read only when its
// rule is set and the rules before it passed.  scan.cigar(b, e, span): the CIGAR text, read by the scanner's lanes together.
template <int NT, class Info, class Scan>
KMM_SAM_HD void classify_sel(const uint8_t *d, uint64_t s, const LineT<NT> &L, const Sel &sel, Scan &scan, Info &o)
{
    LineT<NT - 4> l;
    l.end = L.end;
    l.tab[0] = L.tab[0];
    l.tab[1] = L.tab[1];
    for (int w = 2; w < NT - 4; ++w)
        l.tab[w] = L.tab[w + 4];
    classify(d, s, l, 0u, o);
    if (o.kind != K_KEPT)
        return;
    o.kind = K_EXCLUDED;
    if (!kmm_sel::flags_pass(o.flag, sel))
        return;
    uint64_t v = 0;
    if (sel.min_mapq > 0) {
        if (!parse_decimal(d, L.tab[3] + 1, L.tab[4], 255u, v)) {
            o.kind = K_BAD;
            o.err = ERR_MAPQ;
            return;
        }
        if (v < sel.min_mapq)
            return;
    }
    if (sel.n_iv > 0) {
        const uint64_t nb = L.tab[1] + 1, ne = L.tab[2];
        if (ne - nb == 1 && d[nb] == (uint8_t)'*') {
            if (sel.keep_unplaced)
                o.kind = K_KEPT;
            return;
        }
        const int64_t ref = find_name(sel, d, nb, ne);
        if (ref < 0)
            return;
        if (!parse_decimal(d, L.tab[2] + 1, L.tab[3], 0x7FFFFFFFu, v)) {
            o.kind = K_BAD;
            o.err = ERR_POS;
            return;
        }
        const uint64_t cb = L.tab[4] + 1, ce = L.tab[5];
        uint64_t span = 0;
        if (!(ce - cb == 1 && d[cb] == (uint8_t)'*') && (ce == cb || !scan.cigar(cb, ce, span))) {
            o.kind = K_BAD;
            o.err = ERR_CIGAR;
            return;
        }
        if (!kmm_sel::region_pass(sel, ref, (int64_t)v - 1, o.flag, span))
            return;
    }
    o.kind = K_KEPT;
}

template <bool Q>
KMM_SAM_HD uint32_t out_len(uint64_t seq_len)
{
    return Q ? 2u * (uint32_t)seq_len + 6u : (uint32_t)seq_len + 3u;
}

// The complement of a SEQ letter ("original_strand"): A <-> T, C <-> G, M <-> K, R <-> Y, V <-> B, H <-> D, each case kept; W, S, N
// and every other byte ('=', '.', U, ...) as they are.  On the 16 BAM letters it agrees with kmm_bam.hpp's comp_code.
KMM_SAM_HD uint8_t comp_letter(uint8_t c)
{
    const uint32_t u = c & 0xDFu; // (a letter's upper case)
    if (u < (uint32_t)'A' || u > (uint32_t)'Z')
        return c;
    return (uint8_t)((uint32_t)"TVGHEFCDIJMLKNOPQYSAUBWXRZ"[u - (uint32_t)'A'] | (c & 0x20u));
}

// Is the record one the switch flips?  (0x10 and at least one base.)
KMM_SAM_HD bool flipped(const LineInfo &li, bool orig) { return orig && li.rev && li.seq_len > 0; }

// The quality variant of emit: "@\n" + SEQ + "\n+\n" + QUAL + "\n" at out[0]; an absent QUAL is written as '~' per base, which no
// floor masks.  rev: in read orientation — output byte j is the complement of SEQ's byte seq_len - 1 - j, and QUAL's byte
// seq_len - 1 - j as it is (the stores ascend, the loads descend).
KMM_SAM_HD void emit(const uint8_t *d, const LineInfoQ &li, uint8_t *out, uint32_t lane, uint32_t lanes, bool rev = false)
{
    uint8_t *oq = out + 5 + li.seq_len;
    if (lane == 0) {
        out[0] = '@';
        out[1] = '\n';
        out[2 + li.seq_len] = '\n';
        out[3 + li.seq_len] = '+';
        out[4 + li.seq_len] = '\n';
        oq[li.seq_len] = '\n';
    }
    if (rev) {
        for (uint64_t j = lane; j < li.seq_len; j += lanes) {
            const uint64_t m = li.seq_len - 1 - j;
            out[2 + j] = comp_letter(d[li.seq + m]);
            oq[j] = li.absent ? (uint8_t)'~' : d[li.qual + m];
        }
        return;
    }
    for (uint64_t j = lane; j < li.seq_len; j += lanes) {
        out[2 + j] = d[li.seq + j];
        oq[j] = li.absent ? (uint8_t)'~' : d[li.qual + j];
    }
}

// One kept record's output (lane `lane` of `lanes`): ">\n" + SEQ + "\n" at out[0]; rev: in read orientation, as above
KMM_SAM_HD void emit(const uint8_t *d, const LineInfo &li, uint8_t *out, uint32_t lane, uint32_t lanes, bool rev = false)
{
    if (lane == 0) {
        out[0] = '>';
        out[1] = '\n';
        out[2 + li.seq_len] = '\n';
    }
    if (rev) {
        for (uint64_t j = lane; j < li.seq_len; j += lanes)
            out[2 + j] = comp_letter(d[li.seq + li.seq_len - 1 - j]);
        return;
    }
    for (uint64_t j = lane; j < li.seq_len; j += lanes)
        out[2 + j] = d[li.seq + j];
}

// The line that starts at s, scanned window by window as the wavefront does, one lane after the other (the CPU form of
// scan_line_wave below: the same masks, the same prefix over the lanes).  tabs: false = the newline only; windows that start
// at or past `stop` are not read (L.end NONE).
template <int NT>
inline void scan_line_lanes(const uint8_t *d, uint64_t n, uint64_t s, bool tabs, uint64_t stop, LineT<NT> &L)
{
    L.end = NONE;
    for (int w = 0; w < NT; ++w)
        L.tab[w] = NONE;
    uint32_t seen = 0; // TABs of the line before the window
    for (int64_t a = first_window(d, s); a < (int64_t)n && a < (int64_t)stop; a += WIN) {
        for (uint32_t lane = 0; lane < 64; ++lane) {
            uint32_t tm, nm;
            lane_masks(d, n, s, a, lane, tm, nm);
            if (nm)
                tm &= (nm & (0u - nm)) - 1u; // (TABs behind the newline are another line's)
            const uint32_t cnt = tabs ? (uint32_t)__builtin_popcount(tm) : 0u;
            for (int w = 0; w < NT && tabs; ++w) {
                const uint32_t k = want_tab<NT>(w);
                if (L.tab[w] == NONE && seen < k && k <= seen + cnt)
                    L.tab[w] = (uint64_t)(a + 16 * (int64_t)lane + nth_bit(tm, k - seen));
            }
            seen += cnt;
            if (nm) {
                L.end = (uint64_t)(a + 16 * (int64_t)lane + __builtin_ctz(nm));
                return;
            }
        }
    }
}

template <bool Q>
struct InfoOf {
    typedef LineInfo type;
};
template <>
struct InfoOf<true> {
    typedef LineInfoQ type;
};

KMM_SAM_HD uint64_t tile_end(uint64_t t, uint64_t n) { return (t + 1) * TILE < n ? (t + 1) * TILE : n; }

// The walk over tile t's lines, written once against a scanner (scan(s, tabs, stop, Line &)) and a sink for the kept records
// (sink(LineInfo, offset of its output inside the tile's)).  The tile's first line starts at its first byte when the byte
// before is a newline (or the tile is the first), else behind the first newline inside the tile — looked for inside the tile
// only, so that a long line costs its own tiles one window each.
// H (the raw form): the sink is also told of every header line and every kept record as a line,
// sink.line(start, length with the newline, header?); without it the walk is what it was.
template <bool Q = false, bool S = false, bool H = false, class Scan, class Sink>
KMM_SAM_HD void walk_tile(const uint8_t *d, uint64_t n, uint64_t t, uint32_t excl, Scan &scan, Sink &sink, Tile &o, const Sel &sel = Sel())
{
    o.recs = o.excluded = o.headers = o.bytes = 0;
    o.last_end = 0;
    o.err = NONE;
    const uint64_t ts = t * TILE, te = tile_end(t, n);
    uint64_t s = ts;
    LineT<(Q ? 5 : 4) + (S ? 4 : 0)> L;
    if (ts > 0 && d[ts - 1] != 10u) {
        scan(ts, false, te, L); // (the line in progress at the tile's start belongs to a tile before)
        if (L.end == NONE)
            return;
        s = L.end + 1;
    }
    while (s < te) {
        scan(s, true, n, L);
        if (L.end == NONE)
            return; // (no newline before the chunk ends: the line waits for the next call)
        typename InfoOf<Q>::type li;
        if constexpr (S)
            classify_sel(d, s, L, sel, scan, li);
        else
            classify(d, s, L, excl, li);
        if (li.kind == K_BAD) {
            o.err = s << err_shift<S>() | li.err;
            return;
        }
        if (li.kind == K_HEADER) {
            if constexpr (H)
                sink.line(s, L.end + 1 - s, true);
            ++o.headers;
        } else if (li.kind == K_EXCLUDED)
            ++o.excluded;
        else {
            sink(li, o.bytes);
            if constexpr (H)
                sink.line(s, L.end + 1 - s, false);
            ++o.recs;
            o.bytes += out_len<Q>(li.seq_len);
        }
        o.last_end = L.end + 1;
        s = L.end + 1;
    }
}

// ---- the raw form ("record_sam"): the kept lines as they stand, behind the record-hits mode.
// One span per line the keep step considers, left by the write walk in file order: the selected records, and with "record_sam" 1
// the header lines between them.  entry: the record's ordinal among the piece's selected records (the inner call's entries, in
// file order), RAW_HEADER for a header line, which no rule drops.
struct RawSpan {
    uint64_t start; // of the line in the piece
    uint32_t len;   // with its newline (a line lies inside a piece: below 2^30)
    uint32_t entry;
};
constexpr uint32_t RAW_HEADER = 0xFFFFFFFFu;
constexpr uint32_t RAW_BLOCK = 1024; // spans per block of k_sam_raw_flags: the kept bytes are summed per block, then over the blocks

// The sink of the write walk with spans: the records go to the inner sink as they did; every line the walk reports becomes span
// n of the tile's share spans[0, cap) (cap: what the count pass found — the two passes ask one predicate, so the share is never
// passed; bounds all the same).  entry0: the selected records of the tiles in front.  lead: the lane that stores (the walk is
// wave-uniform).
template <class Inner>
struct SpanSink {
    Inner in;
    RawSpan *spans;
    uint32_t cap, entry0;
    bool headers, lead;
    uint32_t n = 0, recs = 0;
    template <class Info>
    KMM_SAM_HD void operator()(const Info &li, uint32_t at) { in(li, at); }
    KMM_SAM_HD void line(uint64_t start, uint64_t len, bool header)
    {
        if (header && !headers)
            return;
        if (n < cap && lead) {
            RawSpan sp;
            sp.start = start;
            sp.len = (uint32_t)len;
            sp.entry = header ? RAW_HEADER : entry0 + recs;
            spans[n] = sp;
        }
        ++n;
        recs += header ? 0u : 1u;
    }
};

// A tile's share of the spans, from the two-level scan of Tile::recs and Tile::headers: {records, header lines} of the tiles in
// front = those of the blocks of RAW_BLOCK tiles in front (block) + those of the block's tiles in front (in_block).
KMM_SAM_HD uint32_t raw_tile_spans(const Tile &c, bool headers) { return c.recs + (headers ? c.headers : 0u); }
KMM_SAM_HD void raw_tile_pre(const uint32_t *in_block, const uint32_t *block, uint32_t (&pre)[2])
{
    pre[0] = in_block[0] + block[0];
    pre[1] = in_block[1] + block[1];
}
KMM_SAM_HD uint64_t raw_tile_first(const uint32_t (&pre)[2], bool headers) { return (uint64_t)pre[0] + (headers ? pre[1] : 0u); }

// The bytes a span adds to the queue: its line when it is a header line or its entry passes the rule, else 0.  A span that does
// not lie inside the piece's consumed bytes, or whose entry the piece does not have, adds nothing (a slot the walk did not fill
// reads as length 0).  hits / windows: the piece's n_entries entries (windows null: mode 1).
KMM_SAM_HD uint32_t raw_kept_len(const RawSpan &sp, uint64_t consumed, const uint32_t *hits, const uint32_t *windows, uint64_t n_entries,
                                 const RkRule &rule)
{
    if (sp.len == 0 || sp.start >= consumed || (uint64_t)sp.len > consumed - sp.start)
        return 0u;
    if (sp.entry == RAW_HEADER)
        return sp.len;
    if ((uint64_t)sp.entry >= n_entries)
        return 0u;
    return rk_keep(hits[sp.entry], windows ? windows[sp.entry] : 0u, rule) ? sp.len : 0u;
}

// Where a kept span goes: the queue's tail, the kept bytes of the blocks in front, those of the block's spans in front
KMM_SAM_HD uint64_t raw_span_dest(uint64_t tail, uint32_t block_pre, uint32_t pre) { return tail + block_pre + pre; }

// The share of lane `lane` of `lanes` in moving kept span sp to the queue (kmm_bam::raw_copy_part: rk_span's split — the
// destination's aligned middle as 16-byte stores from 16-byte loads at the source's alignment, head and tail byte by byte; no
// byte of the queue is read, none outside [dst, dst + len) written, none outside the span read).
KMM_SAM_HD void raw_copy_span(const uint8_t *d, const RawSpan &sp, uint8_t *queue, uint64_t dst, uint32_t lane, uint32_t lanes)
{
    kmm_bam::raw_copy_part(d + sp.start, queue, dst, sp.len, lane, lanes);
}

// ---- mates kept together in the raw form ("record_sam_mates"): the selected records of the stream are mates in file
// order, 2p and 2p + 1; their lines are kept or dropped together, mate 1 directly in front of mate 2.  A piece's entries are those
// of its whole pairs, n_entries = 2P of them; a mate 1 that the piece or call before left over is entry 0 (`carried` = 1: its line
// waits in a buffer of the handle), so selected record i of the piece has entry carried + i.  The record whose entry would be 2P is
// the odd last one: it waits for the next piece.  span_of[i]: the span of selected record i (MATE_NONE where the walk left none).
constexpr uint32_t MATE_NONE = 0xFFFFFFFFu;

// One line of a pair: where its bytes are and how many (p null: there is no such line).
struct MateLine {
    const uint8_t *p;
    uint32_t len;
};

// A span as the keep step may read it: filled by the walk and inside the piece's consumed bytes.
KMM_SAM_HD bool raw_span_ok(const RawSpan &sp, uint64_t consumed)
{
    return sp.len != 0 && sp.start < consumed && (uint64_t)sp.len <= consumed - sp.start;
}

// The spans by entry: span i of the walk is that of selected record sp.entry (header lines and empty slots have none).
KMM_SAM_HD void raw_span_of_store(const RawSpan &sp, uint64_t i, uint64_t n_recs, uint32_t *span_of)
{
    if (sp.len != 0 && sp.entry != RAW_HEADER && (uint64_t)sp.entry < n_recs)
        span_of[sp.entry] = (uint32_t)i;
}

// What a piece of the pair form reads: its bytes and spans, the spans by entry, the waiting line.
struct MatePiece {
    const uint8_t *d;
    uint64_t consumed;
    const RawSpan *spans;
    uint64_t n_spans;
    const uint32_t *span_of;
    uint64_t n_recs; // the piece's selected records
    uint32_t carried;
    const uint8_t *carry;
    uint32_t carry_len;
};

// The line of entry g of the piece: the waiting one for entry 0 of a piece with a carry, else the span of record g - carried.
KMM_SAM_HD MateLine raw_mate_line(const MatePiece &m, uint64_t g)
{
    if (m.carried && g == 0)
        return MateLine{m.carry_len ? m.carry : nullptr, m.carry_len};
    const uint64_t e = g - m.carried;
    if (e >= m.n_recs)
        return MateLine{nullptr, 0u};
    const uint32_t i = m.span_of[e];
    if ((uint64_t)i >= m.n_spans)
        return MateLine{nullptr, 0u};
    const RawSpan sp = m.spans[i];
    if (!raw_span_ok(sp, m.consumed) || sp.entry != (uint32_t)e)
        return MateLine{nullptr, 0u};
    return MateLine{m.d + sp.start, sp.len};
}

// The share of lane `lane` of `lanes` in comparing two lines' names over bytes [j0, j1) (both lines hold j1 bytes): the lowest
// position of its share where the lines differ or hold a TAB, as position << 1 | (they differ), MATE_NONE when there is none.
// The lowest such position over all lanes decides: two TABs there end two equal names, anything else parts two strangers.
KMM_SAM_HD uint32_t raw_names_part(const uint8_t *a, const uint8_t *b, uint32_t j0, uint32_t j1, uint32_t lane, uint32_t lanes)
{
    for (uint32_t j = j0 + lane; j < j1; j += lanes) {
        const uint8_t x = a[j], y = b[j];
        if (x != y || x == (uint8_t)'\t')
            return j << 1 | (x != y ? 1u : 0u);
    }
    return MATE_NONE;
}

// Are two lines no mates?  Their bytes up to the first TAB must agree in length and content; a line without a TAB inside its span
// is a stranger to every other.  `lanes` bytes a round; lowest(f): the minimum of f(lane) over the lanes, the same for all of them.
template <class Lowest>
KMM_SAM_HD bool raw_pair_strangers(const MateLine &a, const MateLine &b, uint32_t lanes, Lowest &&lowest)
{
    if (!a.p || !b.p)
        return true;
    const uint32_t m = a.len < b.len ? a.len : b.len;
    for (uint32_t j0 = 0; j0 < m; j0 += lanes) {
        const uint32_t j1 = m - j0 < lanes ? m : j0 + lanes;
        const uint32_t c = lowest([&](uint32_t lane) { return raw_names_part(a.p, b.p, j0, j1, lane, lanes); });
        if (c != MATE_NONE)
            return (c & 1u) != 0u;
    }
    return true;
}

// The bytes a span adds to the queue in the pair form: a header line its own length; a mate 1 nothing at its own place; a mate 2
// both lines' lengths when the pair is kept (rk_pair_keep over its two entries), so that mate 1 comes out directly in front of it
// wherever a cut falls.  recs: the records it adds (2 for a kept pair).  odd: the span is the odd last record, which is neither
// counted nor copied here.
KMM_SAM_HD uint32_t raw_pair_kept_len(const MatePiece &m, const RawSpan &sp, const uint32_t *hits, const uint32_t *windows, uint64_t n_entries,
                                      const RkPairRule &rule, uint32_t &recs, bool &odd)
{
    recs = 0u;
    odd = false;
    if (!raw_span_ok(sp, m.consumed))
        return 0u;
    if (sp.entry == RAW_HEADER)
        return sp.len;
    const uint64_t g = (uint64_t)sp.entry + m.carried;
    if (g >= n_entries) {
        odd = g == n_entries;
        return 0u;
    }
    if ((g & 1ull) == 0ull || !kmm_bam::raw_pair_kept(hits, windows, n_entries, g, rule))
        return 0u;
    const MateLine first = raw_mate_line(m, g - 1);
    if (!first.p)
        return 0u;
    recs = 2u;
    return first.len + sp.len;
}

// The share of lane `lane` of `lanes` in moving a kept span of the pair form to the queue: a header line as it stands, a mate 2
// behind its mate 1's line (from the piece, or from the waiting buffer).  kept: what raw_pair_kept_len gave for the span — the
// copy writes exactly those bytes or none.
KMM_SAM_HD void raw_pair_copy_span(const MatePiece &m, const RawSpan &sp, uint32_t kept, uint8_t *queue, uint64_t dst, uint32_t lane,
                                   uint32_t lanes)
{
    if (sp.entry == RAW_HEADER) {
        if (kept == sp.len)
            kmm_bam::raw_copy_part(m.d + sp.start, queue, dst, sp.len, lane, lanes);
        return;
    }
    const uint64_t g = (uint64_t)sp.entry + m.carried;
    if (g == 0)
        return;
    const MateLine first = raw_mate_line(m, g - 1);
    if (!first.p || (uint64_t)first.len + sp.len != (uint64_t)kept)
        return;
    kmm_bam::raw_copy_part(first.p, queue, dst, first.len, lane, lanes);
    kmm_bam::raw_copy_part(m.d + sp.start, queue, dst + first.len, sp.len, lane, lanes);
}

// ---- the CPU form (the tests): the same walk, the lanes one after the other ----
struct CpuScan {
    const uint8_t *d;
    uint64_t n;
    uint32_t lanes = 64; // lanes cigar() reads a CIGAR text with, one after the other
    template <int NT>
    void operator()(uint64_t s, bool tabs, uint64_t stop, LineT<NT> &L)
    {
        scan_line_lanes(d, n, s, tabs, stop, L);
    }
    bool cigar(uint64_t b, uint64_t e, uint64_t &span)
    {
        bool ok = true;
        for (uint32_t lane = 0; lane < lanes; ++lane)
            ok = cigar_text_part(d, b, e, lane, lanes, span) && ok;
        return ok;
    }
};
struct CpuSink {
    const uint8_t *d;
    uint8_t *out; // null: the count pass
    uint64_t no_qual = 0; // (the quality variant) kept records with bases whose QUAL is absent
    bool orig = false;     // "original_strand": the kept records with FLAG 0x10 are written in read orientation
    uint32_t lanes = 1;    // lanes emit is called with, one after the other
    uint64_t reversed = 0; // the records written flipped
    void operator()(const LineInfo &li, uint32_t at)
    {
        if (out) {
            for (uint32_t lane = 0; lane < lanes; ++lane)
                emit(d, li, out + at, lane, lanes, flipped(li, orig));
            reversed += flipped(li, orig) ? 1u : 0u;
        }
    }
    void operator()(const LineInfoQ &li, uint32_t at)
    {
        if (out) {
            for (uint32_t lane = 0; lane < lanes; ++lane)
                emit(d, li, out + at, lane, lanes, flipped(li, orig));
            no_qual += li.absent && li.seq_len > 0 ? 1u : 0u;
            reversed += flipped(li, orig) ? 1u : 0u;
        }
    }
};

// One chunk on the CPU: the count pass, the totals, the write pass (out: at least tot.out_bytes; null = count only).
// Q: the quality variant (four-line FASTQ out; *no_qual: the kept records whose QUAL is absent, counted by the write pass).
// orig: "original_strand" (*reversed: the records the write pass flipped); lanes: what emit is called with.
// sel: the selection beyond excl (its own excl is not read); null or flags only: none.  With one, tot.err is line start << 3 | code.
template <bool Q = false>
inline void cpu_chunk(const uint8_t *d, uint64_t n, uint32_t excl, uint8_t *out, Totals &tot, uint64_t *no_qual = nullptr,
                      bool orig = false, uint64_t *reversed = nullptr, uint32_t lanes = 1, const Sel *sel = nullptr)
{
    tot = Totals{0, 0, 0, 0, 0, NONE};
    const uint64_t n_tiles = (n + TILE - 1) / TILE;
    std::vector<uint64_t> base(n_tiles);
    CpuScan sc{d, n};
    sc.lanes = lanes;
    CpuSink count{d, nullptr};
    const bool selected = sel && !sel->flags_only();
    Sel eff = selected ? *sel : Sel();
    eff.excl = excl;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        Tile o;
        if (selected)
            walk_tile<Q, true>(d, n, t, excl, sc, count, o, eff);
        else
            walk_tile<Q>(d, n, t, excl, sc, count, o);
        base[t] = tot.out_bytes;
        tot.recs += o.recs;
        tot.excluded += o.excluded;
        tot.headers += o.headers;
        tot.out_bytes += o.bytes;
        if (o.last_end > tot.consumed)
            tot.consumed = o.last_end;
        if (o.err < tot.err)
            tot.err = o.err;
    }
    if (!out || tot.err != NONE)
        return;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        CpuSink write{d, out + base[t]};
        write.orig = orig;
        write.lanes = lanes;
        Tile o;
        if (selected)
            walk_tile<Q, true>(d, n, t, excl, sc, write, o, eff);
        else
            walk_tile<Q>(d, n, t, excl, sc, write, o);
        if (no_qual)
            *no_qual += write.no_qual;
        if (reversed)
            *reversed += write.reversed;
    }
}

// The raw form of one chunk on the CPU, as the library runs it: the count pass, the scan of the tiles, the write walk with spans
// (text: the two-line FASTA it writes as before, at least tot.out_bytes), then — the caller maps the text and hands the entries
// over — cpu_raw_keep.  mode: "record_sam" 1 or 2.
struct CpuRaw {
    Totals tot;
    std::vector<RawSpan> spans;
    uint64_t reversed = 0;
};
inline void cpu_raw_spans(const uint8_t *d, uint64_t n, uint32_t excl, int mode, uint8_t *text, CpuRaw &r, bool orig = false,
                          uint32_t lanes = 1, const Sel *sel = nullptr)
{
    cpu_chunk<false>(d, n, excl, nullptr, r.tot, nullptr, orig, nullptr, lanes, sel);
    r.spans.clear();
    if (r.tot.err != NONE)
        return;
    const bool headers = mode == 1, selected = sel && !sel->flags_only();
    Sel eff = selected ? *sel : Sel();
    eff.excl = excl;
    const uint64_t n_tiles = (n + TILE - 1) / TILE;
    std::vector<Tile> tiles(n_tiles);
    std::vector<uint64_t> base(n_tiles);
    std::vector<uint32_t> in_block(2 * n_tiles), block(2 * ((n_tiles + RAW_BLOCK - 1) / RAW_BLOCK) + 2, 0u);
    CpuScan sc{d, n};
    sc.lanes = lanes;
    CpuSink count{d, nullptr};
    uint64_t bytes = 0;
    uint32_t recs = 0, hdrs = 0;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        if (selected)
            walk_tile<false, true>(d, n, t, excl, sc, count, tiles[t], eff);
        else
            walk_tile<false>(d, n, t, excl, sc, count, tiles[t]);
        base[t] = bytes;
        if (t % RAW_BLOCK == 0) { // (the blocks' scan, then the scan inside the block: as k_sam_raw_scan and k_sam_raw_tiles)
            block[2 * (t / RAW_BLOCK)] = recs;
            block[2 * (t / RAW_BLOCK) + 1] = hdrs;
        }
        in_block[2 * t] = recs - block[2 * (t / RAW_BLOCK)];
        in_block[2 * t + 1] = hdrs - block[2 * (t / RAW_BLOCK) + 1];
        bytes += tiles[t].bytes;
        recs += tiles[t].recs;
        hdrs += tiles[t].headers;
    }
    r.spans.assign((size_t)recs + (headers ? hdrs : 0u), RawSpan{0, 0, 0});
    for (uint64_t t = 0; t < n_tiles; ++t) {
        const uint32_t cap = raw_tile_spans(tiles[t], headers);
        if (cap == 0)
            continue;
        CpuSink write{d, text + base[t]};
        write.orig = orig;
        write.lanes = lanes;
        uint32_t pre[2];
        raw_tile_pre(&in_block[2 * t], &block[2 * (t / RAW_BLOCK)], pre);
        SpanSink<CpuSink> sink{write, r.spans.data() + raw_tile_first(pre, headers), cap, pre[0], headers, true};
        Tile o;
        if (selected)
            walk_tile<false, true, true>(d, n, t, excl, sc, sink, o, eff);
        else
            walk_tile<false, false, true>(d, n, t, excl, sc, sink, o);
        r.reversed += sink.in.reversed;
    }
}

// The keep step on the CPU: the flags, the two-level prefix (inside blocks of RAW_BLOCK spans, then over the blocks), the copy
// with `lanes` lanes one after the other.  queue: 16-byte aligned, room behind tail for the kept bytes; returns them, *kept_recs
// the kept records (header lines are not counted).
inline uint64_t cpu_raw_keep(const uint8_t *d, const CpuRaw &r, const uint32_t *hits, const uint32_t *windows, uint64_t n_entries,
                             const RkRule &rule, uint8_t *queue, uint64_t tail, uint32_t lanes, uint64_t *kept_recs)
{
    const size_t m = r.spans.size(), n_blocks = (m + RAW_BLOCK - 1) / RAW_BLOCK;
    std::vector<uint32_t> kept(m), pre(m), block_pre(n_blocks + 1, 0u);
    uint64_t recs = 0;
    for (size_t b = 0; b < n_blocks; ++b) {
        uint32_t sum = 0;
        for (size_t i = b * RAW_BLOCK; i < m && i < (b + 1) * RAW_BLOCK; ++i) {
            kept[i] = raw_kept_len(r.spans[i], r.tot.consumed, hits, windows, n_entries, rule);
            pre[i] = sum;
            sum += kept[i];
            recs += kept[i] && r.spans[i].entry != RAW_HEADER ? 1u : 0u;
        }
        block_pre[b + 1] = block_pre[b] + sum;
    }
    for (size_t i = 0; i < m; ++i)
        if (kept[i])
            for (uint32_t lane = 0; lane < lanes; ++lane)
                raw_copy_span(d, r.spans[i], queue, raw_span_dest(tail, block_pre[i / RAW_BLOCK], pre[i]), lane, lanes);
    *kept_recs = recs;
    return block_pre[n_blocks];
}

// The keep step of the pair form on the CPU ("record_sam_mates"), as the library runs it over one piece: the spans by entry, the
// mate check (`lanes` bytes a round), the pair flags, the two-level prefix, the pair copy with `lanes` lanes one after the other.
// carry[0, carry_len): the waiting mate 1's line (carried = 1) — entry 0.  hits / windows: the n_entries entries of the piece's
// whole pairs.  Returns the kept bytes; *kept_recs the kept records; *stranger the lowest pair of the piece whose lines are no
// mates (MATE_NONE: none; nothing is copied then); *odd_span the span of the odd last record (MATE_NONE: none).
struct CpuMates {
    uint64_t kept_recs = 0;
    uint32_t stranger = MATE_NONE, odd_span = MATE_NONE;
};
inline uint64_t cpu_raw_mates_keep(const uint8_t *d, const CpuRaw &r, uint32_t carried, const uint8_t *carry, uint32_t carry_len,
                                   const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const RkPairRule &rule, uint8_t *queue,
                                   uint64_t tail, uint32_t lanes, CpuMates &o)
{
    const size_t m = r.spans.size(), n_blocks = (m + RAW_BLOCK - 1) / RAW_BLOCK;
    std::vector<uint32_t> span_of((size_t)r.tot.recs + 1, MATE_NONE);
    for (size_t i = 0; i < m; ++i)
        raw_span_of_store(r.spans[i], i, r.tot.recs, span_of.data());
    const MatePiece mp{d, r.tot.consumed, r.spans.data(), m, span_of.data(), r.tot.recs, carried, carry, carry_len};
    o = CpuMates();
    for (uint64_t p = 0; p < n_entries / 2; ++p) {
        const bool bad = raw_pair_strangers(raw_mate_line(mp, 2 * p), raw_mate_line(mp, 2 * p + 1), lanes, [&](auto f) {
            uint32_t low = MATE_NONE;
            for (uint32_t lane = 0; lane < lanes; ++lane) {
                const uint32_t c = f(lane);
                low = c < low ? c : low;
            }
            return low;
        });
        if (bad && (uint32_t)p < o.stranger)
            o.stranger = (uint32_t)p;
    }
    std::vector<uint32_t> kept(m), pre(m), block_pre(n_blocks + 1, 0u);
    for (size_t b = 0; b < n_blocks; ++b) {
        uint32_t sum = 0;
        for (size_t i = b * RAW_BLOCK; i < m && i < (b + 1) * RAW_BLOCK; ++i) {
            uint32_t recs = 0;
            bool odd = false;
            kept[i] = raw_pair_kept_len(mp, r.spans[i], hits, windows, n_entries, rule, recs, odd);
            pre[i] = sum;
            sum += kept[i];
            o.kept_recs += recs;
            if (odd)
                o.odd_span = (uint32_t)i;
        }
        block_pre[b + 1] = block_pre[b] + sum;
    }
    if (o.stranger != MATE_NONE)
        return 0;
    for (size_t i = 0; i < m; ++i)
        if (kept[i])
            for (uint32_t lane = 0; lane < lanes; ++lane)
                raw_pair_copy_span(mp, r.spans[i], kept[i], queue, raw_span_dest(tail, block_pre[i / RAW_BLOCK], pre[i]), lane, lanes);
    return block_pre[n_blocks];
}

#if defined(__HIPCC__)
// The line that starts at s, one wavefront: 64 lanes x 16 bytes per window; the newline is the first lane (ballot) with one,
// TAB k lies in the lane whose prefix of TAB counts passes k.  Wave-uniform result.
template <int NT>
__device__ __forceinline__ void scan_line_wave(const uint8_t *__restrict__ d, uint64_t n, uint64_t s, bool tabs, uint64_t stop,
                                               LineT<NT> &L)
{
    const uint32_t lane = threadIdx.x & 63u;
    L.end = NONE;
#pragma unroll
    for (int w = 0; w < NT; ++w)
        L.tab[w] = NONE;
    uint32_t seen = 0;
    for (int64_t a = first_window(d, s); a < (int64_t)n && a < (int64_t)stop; a += WIN) {
        uint32_t tm, nm;
        lane_masks(d, n, s, a, lane, tm, nm);
        const unsigned long long nb = __ballot(nm != 0);
        const uint32_t cut = nb ? (uint32_t)__ffsll((long long)nb) - 1u : 64u;
        if (lane == cut)
            tm &= (nm & (0u - nm)) - 1u;
        else if (lane > cut)
            tm = 0;
        if (tabs && L.tab[NT - 1] == NONE) {
            const uint32_t cnt = (uint32_t)__popc(tm);
            uint32_t incl = cnt;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o);
                if ((int)lane >= o)
                    incl += v;
            }
            const uint32_t before = seen + incl - cnt;
#pragma unroll
            for (int w = 0; w < NT; ++w) {
                const uint32_t k = want_tab<NT>(w);
                const bool mine = L.tab[w] == NONE && before < k && k <= before + cnt;
                const unsigned long long m = __ballot(mine);
                if (m) {
                    const int src = __ffsll((long long)m) - 1;
                    const uint32_t bit = __shfl(mine ? nth_bit(tm, k - before) : 0u, src);
                    L.tab[w] = (uint64_t)(a + 16 * (int64_t)src + bit);
                }
            }
            seen += __shfl(incl, 63);
        }
        if (nb) {
            const uint32_t bit = (uint32_t)__shfl((int)(nm ? __builtin_ctz(nm) : 0), (int)cut);
            L.end = (uint64_t)(a + 16 * (int64_t)cut + bit);
            return;
        }
    }
}

struct WaveScan {
    const uint8_t *d;
    uint64_t n;
    template <int NT>
    __device__ void operator()(uint64_t s, bool tabs, uint64_t stop, LineT<NT> &L)
    {
        scan_line_wave(d, n, s, tabs, stop, L);
    }
    // (with a selection) the CIGAR text d[b, e): 64 bytes per step, one per lane; the verdict and the span are wave-uniform
    __device__ bool cigar(uint64_t b, uint64_t e, uint64_t &span)
    {
        uint64_t part = 0;
        const bool ok = cigar_text_part(d, b, e, threadIdx.x & 63u, 64u, part);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)part, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(part >> 32), o);
            part += (uint64_t)hi << 32 | lo;
        }
        span += part;
        return __ballot(!ok) == 0ull;
    }
};
struct NoSink {
    __device__ void operator()(const LineInfo &, uint32_t) {}
};
struct WaveSink {
    const uint8_t *d;
    uint8_t *out;
    __device__ void operator()(const LineInfo &li, uint32_t at) { emit(d, li, out + at, threadIdx.x & 63u, 64u); }
};
struct WaveSinkQ {
    const uint8_t *d;
    uint8_t *out;
    uint32_t no_qual; // kept records with bases whose QUAL is absent (wave-uniform)
    __device__ void operator()(const LineInfoQ &li, uint32_t at)
    {
        emit(d, li, out + at, threadIdx.x & 63u, 64u);
        no_qual += li.absent && li.seq_len > 0 ? 1u : 0u;
    }
};

// ("original_strand": the kept records with FLAG 0x10 and bases are written in read orientation, a wave-uniform choice per
// record, and counted)
struct WaveSinkRev {
    const uint8_t *d;
    uint8_t *out;
    uint32_t reversed; // records written flipped (wave-uniform)
    __device__ void operator()(const LineInfo &li, uint32_t at)
    {
        const bool rev = flipped(li, true);
        emit(d, li, out + at, threadIdx.x & 63u, 64u, rev);
        reversed += rev ? 1u : 0u;
    }
};
struct WaveSinkQRev {
    const uint8_t *d;
    uint8_t *out;
    uint32_t no_qual;  // kept records with bases whose QUAL is absent (wave-uniform)
    uint32_t reversed; // records written flipped (wave-uniform)
    __device__ void operator()(const LineInfoQ &li, uint32_t at)
    {
        const bool rev = flipped(li, true);
        emit(d, li, out + at, threadIdx.x & 63u, 64u, rev);
        no_qual += li.absent && li.seq_len > 0 ? 1u : 0u;
        reversed += rev ? 1u : 0u;
    }
};

// count: one wavefront per tile (grid-stride)
__global__ void __launch_bounds__(256) k_sam_count(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                   Tile *__restrict__ tiles)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    NoSink none;
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        Tile o;
        walk_tile(d, n, t, excl, sc, none, o);
        if ((threadIdx.x & 63u) == 0)
            tiles[t] = o;
    }
}

// count, the quality variant (TAB 11 found, QUAL checked against SEQ, four-line FASTQ lengths)
__global__ void __launch_bounds__(256) k_sam_count_q(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                     Tile *__restrict__ tiles)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    NoSink none;
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        Tile o;
        walk_tile<true>(d, n, t, excl, sc, none, o);
        if ((threadIdx.x & 63u) == 0)
            tiles[t] = o;
    }
}

// totals: one workgroup of 1024 threads, each over a run of consecutive tiles: the exclusive scan of the tiles' output bytes
// (base) and the sums / extremes
__global__ void __launch_bounds__(1024) k_sam_totals(const Tile *__restrict__ in, uint64_t n_tiles, unsigned long long *__restrict__ base,
                                                     Totals *__restrict__ tot)
{
    __shared__ unsigned long long s[1024];
    const uint32_t i = threadIdx.x;
    const uint64_t per = (n_tiles + 1023) / 1024, t0 = (uint64_t)i * per < n_tiles ? (uint64_t)i * per : n_tiles,
                   t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    unsigned long long v[6] = {0, 0, 0, 0, 0, NONE}; // out bytes, recs, excluded, headers, consumed (max), err (min)
    for (uint64_t t = t0; t < t1; ++t) {
        const Tile c = in[t];
        v[0] += c.bytes;
        v[1] += c.recs;
        v[2] += c.excluded;
        v[3] += c.headers;
        v[4] = c.last_end > v[4] ? c.last_end : v[4];
        v[5] = c.err < v[5] ? c.err : v[5];
    }
    s[i] = v[0];
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) { // inclusive scan (Hillis-Steele)
        const unsigned long long x = i >= off ? s[i - off] : 0ull;
        __syncthreads();
        s[i] += x;
        __syncthreads();
    }
    unsigned long long b = s[i] - v[0];
    for (uint64_t t = t0; t < t1; ++t) {
        base[t] = b;
        b += in[t].bytes;
    }
    if (i == 1023)
        tot->out_bytes = s[1023];
#pragma unroll
    for (int f = 1; f < 6; ++f) {
        __syncthreads();
        s[i] = v[f];
        __syncthreads();
        for (uint32_t h = 512; h > 0; h >>= 1) {
            if (i < h) {
                const unsigned long long x = s[i + h];
                s[i] = f == 4 ? (x > s[i] ? x : s[i]) : f == 5 ? (x < s[i] ? x : s[i]) : s[i] + x;
            }
            __syncthreads();
        }
        if (i == 0) {
            if (f == 1)
                tot->recs = s[0];
            else if (f == 2)
                tot->excluded = s[0];
            else if (f == 3)
                tot->headers = s[0];
            else if (f == 4)
                tot->consumed = s[0];
            else
                tot->err = s[0];
        }
    }
}

// write: one wavefront per tile (grid-stride), the same walk; every kept record at base[t] + its offset in the tile
__global__ void __launch_bounds__(256) k_sam_write(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                   const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                   uint8_t *__restrict__ out)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSink sink{d, out + base[t]};
        Tile o;
        walk_tile(d, n, t, excl, sc, sink, o);
    }
}

// write, the quality variant: four-line FASTQ per kept record; the kept records whose QUAL is absent are counted per tile and
// added to *no_qual (one atomic per tile that has any)
__global__ void __launch_bounds__(256) k_sam_write_q(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                     const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                     uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSinkQ sink{d, out + base[t], 0u};
        Tile o;
        walk_tile<true>(d, n, t, excl, sc, sink, o);
        if ((threadIdx.x & 63u) == 0 && sink.no_qual)
            atomicAdd(no_qual, (unsigned long long)sink.no_qual);
    }
}

// write with "original_strand" on: k_sam_write and k_sam_write_q with the kept records whose FLAG has 0x10 written in read
// orientation and counted per tile into *reversed (one atomic per tile that has any).  Kernels of their own: the two above are
// what runs while the switch is off.
__global__ void __launch_bounds__(256) k_sam_write_rev(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                       const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                       uint8_t *__restrict__ out, unsigned long long *__restrict__ reversed)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSinkRev sink{d, out + base[t], 0u};
        Tile o;
        walk_tile(d, n, t, excl, sc, sink, o);
        if ((threadIdx.x & 63u) == 0 && sink.reversed)
            atomicAdd(reversed, (unsigned long long)sink.reversed);
    }
}

__global__ void __launch_bounds__(256) k_sam_write_q_rev(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                         const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                         uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual,
                                                         unsigned long long *__restrict__ reversed)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSinkQRev sink{d, out + base[t], 0u, 0u};
        Tile o;
        walk_tile<true>(d, n, t, excl, sc, sink, o);
        if ((threadIdx.x & 63u) == 0 && sink.no_qual)
            atomicAdd(no_qual, (unsigned long long)sink.no_qual);
        if ((threadIdx.x & 63u) == 0 && sink.reversed)
            atomicAdd(reversed, (unsigned long long)sink.reversed);
    }
}

// ---- with a selection set: the passes above as <.., true>; kernels of their own — the ones above are what runs
// without one.  sel.excl is the exclude mask.
template <bool Q>
__device__ __forceinline__ void sam_count_sel_tiles(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, const Sel &sel,
                                                    Tile *__restrict__ tiles)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    WaveScan sc{d, n};
    NoSink none;
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        Tile o;
        walk_tile<Q, true>(d, n, t, sel.excl, sc, none, o, sel);
        if ((threadIdx.x & 63u) == 0)
            tiles[t] = o;
    }
}
__global__ void __launch_bounds__(256) k_sam_count_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                       Tile *__restrict__ tiles)
{
    sam_count_sel_tiles<false>(d, n, n_tiles, sel, tiles);
}
__global__ void __launch_bounds__(256) k_sam_count_q_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                         Tile *__restrict__ tiles)
{
    sam_count_sel_tiles<true>(d, n, n_tiles, sel, tiles);
}

// A sink that stops at the end of the tile's share of the output (what the count pass gave it): the two passes ask one
// predicate, so it never does; bounds all the same.
template <class Inner>
struct BoundedSink {
    Inner in;
    uint32_t cap;
    __device__ void operator()(const LineInfo &li, uint32_t at)
    {
        if ((uint64_t)at + li.seq_len + 3u <= (uint64_t)cap)
            in(li, at);
    }
    __device__ void operator()(const LineInfoQ &li, uint32_t at)
    {
        if ((uint64_t)at + 2u * li.seq_len + 6u <= (uint64_t)cap)
            in(li, at);
    }
};

template <bool Q, class Inner>
__device__ __forceinline__ void sam_write_sel_tile(const uint8_t *__restrict__ d, uint64_t n, uint64_t t, const Sel &sel, uint32_t cap,
                                                   Inner &inner)
{
    WaveScan sc{d, n};
    BoundedSink<Inner> sink{inner, cap};
    Tile o;
    walk_tile<Q, true>(d, n, t, sel.excl, sc, sink, o, sel);
    inner = sink.in;
}

__global__ void __launch_bounds__(256) k_sam_write_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                       const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                       uint8_t *__restrict__ out)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSink sink{d, out + base[t]};
        sam_write_sel_tile<false>(d, n, t, sel, tiles[t].bytes, sink);
    }
}
__global__ void __launch_bounds__(256) k_sam_write_q_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                         const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                         uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSinkQ sink{d, out + base[t], 0u};
        sam_write_sel_tile<true>(d, n, t, sel, tiles[t].bytes, sink);
        if ((threadIdx.x & 63u) == 0 && sink.no_qual)
            atomicAdd(no_qual, (unsigned long long)sink.no_qual);
    }
}
__global__ void __launch_bounds__(256) k_sam_write_rev_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                           const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                           uint8_t *__restrict__ out, unsigned long long *__restrict__ reversed)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSinkRev sink{d, out + base[t], 0u};
        sam_write_sel_tile<false>(d, n, t, sel, tiles[t].bytes, sink);
        if ((threadIdx.x & 63u) == 0 && sink.reversed)
            atomicAdd(reversed, (unsigned long long)sink.reversed);
    }
}
__global__ void __launch_bounds__(256) k_sam_write_q_rev_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                             const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                             uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual,
                                                             unsigned long long *__restrict__ reversed)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        if (tiles[t].recs == 0)
            continue;
        WaveSinkQRev sink{d, out + base[t], 0u, 0u};
        sam_write_sel_tile<true>(d, n, t, sel, tiles[t].bytes, sink);
        if ((threadIdx.x & 63u) == 0 && sink.no_qual)
            atomicAdd(no_qual, (unsigned long long)sink.no_qual);
        if ((threadIdx.x & 63u) == 0 && sink.reversed)
            atomicAdd(reversed, (unsigned long long)sink.reversed);
    }
}

// ---- the raw form ("record_sam") ----
// scan: the second level of both prefixes, over the sums of blocks of RAW_BLOCK items — the blocks of k_sam_raw_tiles (records and
// header lines: the entry base and the span base of every tile) and the blocks of k_sam_raw_flags (kept bytes and kept records: the
// destinations and the queue's advance).  One workgroup of 1024 threads, each over a run of consecutive blocks (the shape of
// kmm_bam.hpp k_bam_raw_scan), two columns at once: pre[2 i] and pre[2 i + 1] = the sums of a[u] and b[u] over u < i (32-bit: both
// columns count lines or bytes of one piece, below 2^31); total, where given, gets the two sums over all blocks.  (A piece of
// 2^30 bytes has 1024 blocks of tiles: one per thread.  The first level is not this kernel's: over a million tiles, a thousand one
// after the other per thread, it took 3.6 ms: profiles/sam_out/README.md.)
__global__ void __launch_bounds__(1024) k_sam_raw_scan(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint64_t n_items,
                                                       uint32_t *__restrict__ pre, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s[1024];
    const uint32_t i = threadIdx.x;
    const uint64_t per = (n_items + 1023) / 1024, t0 = (uint64_t)i * per < n_items ? (uint64_t)i * per : n_items,
                   t1 = t0 + per < n_items ? t0 + per : n_items;
    unsigned long long sum = 0; // (the two columns side by side: neither reaches 2^32, no carry crosses)
    for (uint64_t t = t0; t < t1; ++t)
        sum += (unsigned long long)a[t] | (unsigned long long)b[t] << 32;
    s[i] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) { // inclusive scan (Hillis-Steele)
        const unsigned long long x = i >= off ? s[i - off] : 0ull;
        __syncthreads();
        s[i] += x;
        __syncthreads();
    }
    unsigned long long run = s[i] - sum;
    for (uint64_t t = t0; t < t1; ++t) {
        pre[2 * t] = (uint32_t)run;
        pre[2 * t + 1] = (uint32_t)(run >> 32);
        run += (unsigned long long)a[t] | (unsigned long long)b[t] << 32;
    }
    if (total && i == 1023) {
        total[0] = s[1023] & 0xFFFFFFFFull;
        total[1] = s[1023] >> 32;
    }
}

// The scan inside a workgroup of RAW_BLOCK threads over two columns side by side in 64 bits (neither reaches 2^32): returns the
// thread's inclusive prefix, all = the workgroup's sum.  s: 16 words of LDS.
__device__ __forceinline__ unsigned long long raw_block_scan(unsigned long long v, unsigned long long *s, unsigned long long &all)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), o);
        if ((int)lane >= o)
            incl += (unsigned long long)hi << 32 | lo;
    }
    if (lane == 63)
        s[wave] = incl;
    __syncthreads();
    unsigned long long before = 0;
    all = 0;
#pragma unroll
    for (uint32_t w = 0; w < 16; ++w) {
        before += w < wave ? s[w] : 0ull;
        all += s[w];
    }
    return before + incl;
}

// tiles: one thread per tile, RAW_BLOCK tiles per workgroup: pre[2 t] and pre[2 t + 1] = the selected records and the header lines
// of the block's tiles in front of tile t, block_recs / block_headers the block's sums (k_sam_raw_scan over them gives the blocks'
// bases: raw_tile_pre adds the two levels).
__global__ void __launch_bounds__(1024) k_sam_raw_tiles(const Tile *__restrict__ tiles, uint64_t n_tiles, uint32_t *__restrict__ pre,
                                                        uint32_t *__restrict__ block_recs, uint32_t *__restrict__ block_headers)
{
    static_assert(RAW_BLOCK == 1024, "one tile per thread of a 1024-thread workgroup");
    __shared__ unsigned long long s[16];
    const uint64_t t = (uint64_t)blockIdx.x * RAW_BLOCK + threadIdx.x;
    unsigned long long v = 0, all;
    if (t < n_tiles)
        v = (unsigned long long)tiles[t].recs | (unsigned long long)tiles[t].headers << 32;
    const unsigned long long excl = raw_block_scan(v, s, all) - v;
    if (t < n_tiles) {
        pre[2 * t] = (uint32_t)excl;
        pre[2 * t + 1] = (uint32_t)(excl >> 32);
    }
    if (threadIdx.x == 0) {
        block_recs[blockIdx.x] = (uint32_t)all;
        block_headers[blockIdx.x] = (uint32_t)(all >> 32);
    }
}

// write with spans: the write walk of k_sam_write / _sel / _rev / _rev_sel, its sink wrapped in a SpanSink — the FASTA text as
// before, and span first + i for line i of the tile's share (tile_pre, block_pre: k_sam_raw_tiles and k_sam_raw_scan over its
// blocks; headers: "record_sam" 1).
// A tile that holds header lines alone is walked too.  Kernels of their own: the four above are what runs while "record_sam" is 0.
template <bool S, bool REV>
__device__ __forceinline__ void sam_write_spans_tiles(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, const Sel &sel,
                                                      const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                      uint8_t *__restrict__ out, unsigned long long *__restrict__ reversed,
                                                      const uint32_t *__restrict__ tile_pre, const uint32_t *__restrict__ block_pre,
                                                      bool headers, RawSpan *__restrict__ spans, uint64_t n_spans)
{
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    const bool lead = (threadIdx.x & 63u) == 0;
    WaveScan sc{d, n};
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const Tile c = tiles[t];
        const uint32_t cap = raw_tile_spans(c, headers);
        uint32_t pre[2];
        raw_tile_pre(tile_pre + 2 * t, block_pre + 2 * (t / RAW_BLOCK), pre);
        const uint64_t first = raw_tile_first(pre, headers);
        if (cap == 0 || first + cap > n_spans)
            continue;
        typename std::conditional<REV, WaveSinkRev, WaveSink>::type inner{d, out + base[t]};
        Tile o;
        uint32_t flips = 0;
        if constexpr (S) {
            SpanSink<BoundedSink<decltype(inner)>> sink{{inner, c.bytes}, spans + first, cap, pre[0], headers, lead};
            walk_tile<false, true, true>(d, n, t, sel.excl, sc, sink, o, sel);
            if constexpr (REV)
                flips = sink.in.in.reversed;
        } else {
            SpanSink<decltype(inner)> sink{inner, spans + first, cap, pre[0], headers, lead};
            walk_tile<false, false, true>(d, n, t, sel.excl, sc, sink, o);
            if constexpr (REV)
                flips = sink.in.reversed;
        }
        if (REV && lead && flips)
            atomicAdd(reversed, (unsigned long long)flips);
    }
}
__global__ void __launch_bounds__(256) k_sam_write_spans(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                         const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                         uint8_t *__restrict__ out, const uint32_t *__restrict__ tile_pre,
                                                         const uint32_t *__restrict__ block_pre, uint32_t headers,
                                                         RawSpan *__restrict__ spans, uint64_t n_spans)
{
    Sel sel;
    sel.excl = excl;
    sam_write_spans_tiles<false, false>(d, n, n_tiles, sel, tiles, base, out, nullptr, tile_pre, block_pre, headers != 0u, spans, n_spans);
}
__global__ void __launch_bounds__(256) k_sam_write_spans_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                             const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                             uint8_t *__restrict__ out, const uint32_t *__restrict__ tile_pre,
                                                             const uint32_t *__restrict__ block_pre, uint32_t headers,
                                                             RawSpan *__restrict__ spans, uint64_t n_spans)
{
    sam_write_spans_tiles<true, false>(d, n, n_tiles, sel, tiles, base, out, nullptr, tile_pre, block_pre, headers != 0u, spans, n_spans);
}
__global__ void __launch_bounds__(256) k_sam_write_spans_rev(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint32_t excl,
                                                             const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                             uint8_t *__restrict__ out, unsigned long long *__restrict__ reversed,
                                                             const uint32_t *__restrict__ tile_pre, const uint32_t *__restrict__ block_pre,
                                                             uint32_t headers, RawSpan *__restrict__ spans, uint64_t n_spans)
{
    Sel sel;
    sel.excl = excl;
    sam_write_spans_tiles<false, true>(d, n, n_tiles, sel, tiles, base, out, reversed, tile_pre, block_pre, headers != 0u, spans, n_spans);
}
__global__ void __launch_bounds__(256) k_sam_write_spans_rev_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, Sel sel,
                                                                 const Tile *__restrict__ tiles, const unsigned long long *__restrict__ base,
                                                                 uint8_t *__restrict__ out, unsigned long long *__restrict__ reversed,
                                                                 const uint32_t *__restrict__ tile_pre, const uint32_t *__restrict__ block_pre,
                                                                 uint32_t headers, RawSpan *__restrict__ spans, uint64_t n_spans)
{
    sam_write_spans_tiles<true, true>(d, n, n_tiles, sel, tiles, base, out, reversed, tile_pre, block_pre, headers != 0u, spans, n_spans);
}

// flags: one thread per span, RAW_BLOCK spans per workgroup: kept[i] = the span's kept length or 0 (raw_kept_len), pre[i] = the kept
// bytes of the block's spans in front, block_bytes / block_recs = the block's kept bytes and kept records (header lines are not
// records).  hits / windows: the inner call's n_entries entries, complete behind its k_read_hits.
__global__ void __launch_bounds__(1024) k_sam_raw_flags(const RawSpan *__restrict__ spans, uint64_t n_spans, uint64_t consumed,
                                                        const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                                        uint64_t n_entries, RkRule rule, uint32_t *__restrict__ kept,
                                                        uint32_t *__restrict__ pre, uint32_t *__restrict__ block_bytes,
                                                        uint32_t *__restrict__ block_recs)
{
    static_assert(RAW_BLOCK == 1024, "one span per thread of a 1024-thread workgroup");
    __shared__ unsigned long long s[16];
    const uint64_t i = (uint64_t)blockIdx.x * RAW_BLOCK + threadIdx.x;
    uint32_t len = 0, rec = 0;
    if (i < n_spans) {
        const RawSpan sp = spans[i];
        len = raw_kept_len(sp, consumed, hits, windows, n_entries, rule);
        rec = len && sp.entry != RAW_HEADER ? 1u : 0u;
    }
    // (bytes and records side by side: a block's kept bytes lie below 2^31)
    unsigned long long all;
    const unsigned long long incl = raw_block_scan((unsigned long long)len | (unsigned long long)rec << 32, s, all);
    if (i < n_spans) {
        kept[i] = len;
        pre[i] = (uint32_t)incl - len;
    }
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = (uint32_t)all;
        block_recs[blockIdx.x] = (uint32_t)(all >> 32);
    }
}

// copy: one wavefront per kept span (grid-stride), its 64 lanes over the line's bytes (raw_copy_span), written behind the queue's
// tail (read from the device: {bytes, records}, as k_rk_scatter reads it) at the block's base (block_pre[2 b]: k_sam_raw_scan over
// the blocks) plus the span's prefix.  kept[i] is the span's own length or 0: the span was checked against `consumed` by flags.
__global__ void __launch_bounds__(256) k_sam_raw_copy(const uint8_t *__restrict__ d, const RawSpan *__restrict__ spans, uint64_t n_spans,
                                                      const uint32_t *__restrict__ kept, const uint32_t *__restrict__ pre,
                                                      const uint32_t *__restrict__ block_pre, const unsigned long long *__restrict__ tail,
                                                      uint8_t *__restrict__ queue)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    const uint64_t tail0 = tail[0];
    for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; i < n_spans; i += waves) {
        if (kept[i] == 0)
            continue;
        const RawSpan sp = spans[i];
        raw_copy_span(d, sp, queue, raw_span_dest(tail0, block_pre[2 * (i / RAW_BLOCK)], pre[i]), lane, 64u);
    }
}

// ---- mates kept together in the raw form ("record_sam_mates"): kernels of their own, so that the unpaired forms
// above stay as they are.  ctl: three control words of the piece — [0] the lowest pair of the piece whose lines are no mates, [1]
// and [2] the start and the length of the odd last record's line — all ~0 before the launches.

// span_of: one thread per span (grid-stride): the spans by entry (span_of is filled with MATE_NONE first).
__global__ void __launch_bounds__(256) k_sam_raw_span_of(const RawSpan *__restrict__ spans, uint64_t n_spans, uint64_t n_recs,
                                                         uint32_t *__restrict__ span_of)
{
    const uint64_t threads = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_spans; i += threads)
        raw_span_of_store(spans[i], i, n_recs, span_of);
}

// The minimum of v over the wavefront's 64 lanes, in all of them.
__device__ __forceinline__ uint32_t wave_lowest(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t x = (uint32_t)__shfl_xor((int)v, o);
        v = x < v ? x : v;
    }
    return v;
}

// names: one wavefront per pair of the piece (grid-stride), 64 bytes of both lines a round (raw_pair_strangers: names are at most
// 254 bytes and mostly under 40 — one round); every read lies inside a span the flags would accept, or inside the waiting line.
// The lowest pair of strangers goes to ctl[0].
__global__ void __launch_bounds__(256) k_sam_raw_pair_names(MatePiece m, uint64_t n_entries, unsigned long long *__restrict__ ctl)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u), n_pairs = n_entries / 2;
    for (uint64_t pr = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; pr < n_pairs; pr += waves) {
        const bool strangers = raw_pair_strangers(raw_mate_line(m, 2 * pr), raw_mate_line(m, 2 * pr + 1), 64u,
                                                  [&](auto f) { return wave_lowest(f(lane)); });
        if (lane == 0 && strangers)
            atomicMin(ctl, (unsigned long long)pr);
    }
}

// flags, the pair form: as k_sam_raw_flags with raw_pair_kept_len; the thread that meets the odd last record reports its line.
__global__ void __launch_bounds__(1024) k_sam_raw_pair_flags(MatePiece m, const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                                             uint64_t n_entries, RkPairRule rule, uint32_t *__restrict__ kept,
                                                             uint32_t *__restrict__ pre, uint32_t *__restrict__ block_bytes,
                                                             uint32_t *__restrict__ block_recs, unsigned long long *__restrict__ ctl)
{
    static_assert(RAW_BLOCK == 1024, "one span per thread of a 1024-thread workgroup");
    __shared__ unsigned long long s[16];
    const uint64_t i = (uint64_t)blockIdx.x * RAW_BLOCK + threadIdx.x;
    uint32_t len = 0, rec = 0;
    if (i < m.n_spans) {
        const RawSpan sp = m.spans[i];
        bool odd;
        len = raw_pair_kept_len(m, sp, hits, windows, n_entries, rule, rec, odd);
        if (odd) {
            ctl[1] = sp.start;
            ctl[2] = sp.len;
        }
    }
    unsigned long long all;
    const unsigned long long incl = raw_block_scan((unsigned long long)len | (unsigned long long)rec << 32, s, all);
    if (i < m.n_spans) {
        kept[i] = len;
        pre[i] = (uint32_t)incl - len;
    }
    if (threadIdx.x == 0) {
        block_bytes[blockIdx.x] = (uint32_t)all;
        block_recs[blockIdx.x] = (uint32_t)(all >> 32);
    }
}

// copy, the pair form: one wavefront per kept span (grid-stride): a header line as k_sam_raw_copy moves it, a mate 2 behind its
// mate 1's line (raw_pair_copy_span).
__global__ void __launch_bounds__(256) k_sam_raw_pair_copy(MatePiece m, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ pre,
                                                           const uint32_t *__restrict__ block_pre, const unsigned long long *__restrict__ tail,
                                                           uint8_t *__restrict__ queue)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    const uint64_t tail0 = tail[0];
    for (uint64_t i = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; i < m.n_spans; i += waves) {
        const uint32_t k = kept[i];
        if (k == 0)
            continue;
        raw_pair_copy_span(m, m.spans[i], k, queue, raw_span_dest(tail0, block_pre[2 * (i / RAW_BLOCK)], pre[i]), lane, 64u);
    }
}
#endif

} // namespace kmm_sam
