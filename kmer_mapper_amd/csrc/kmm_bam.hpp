// kmm_bam.hpp — part of libkmm: BAM records (SAM/BAM specification 4.2) found and decoded ON THE GPU (kmm_map_bam; included by
// kmm.hip — the host side is kmm_bam_host.hpp —, compiled by itself with g++ in tests/test_bam_walk_on_the_cpu.py, where the very same orchestration runs on the CPU).
//
// A BAM file is a BGZF stream (kmm_gpu_inflate.hpp inflates it) holding a header and then records, each one prefixed by its
// length: where a record starts is known only by walking the chain from the first one — a serial chain.  It is cut the way
// kmm_gpu_gunzip.hpp cuts a deflate stream:
//   1. spec     the inflated bytes are cut into tiles of TILE bytes; one wavefront per tile tests 64 byte positions at a time
//               for a plausible record start (fields consistent with block_size, the name NUL-terminated, -1 <= refID,
//               next_refID < n_ref, and CHAIN such records in a row) and one lane walks the chain from the first one to the
//               first start at or past the tile's end: the tile's claim (entry, exit, records).  Tile 0 starts where it is
//               known to (behind the header, or at the bytes carried over from the call before).  A tile with no plausible
//               start claims to lie inside one record (long reads) — the exit passes through it;
//   2. link     a tile's claim stands iff it agrees with the exit of the tiles before it (check); the claims that do not are
//               walked again from that exit (fix) — follow-up launches until every claim agrees.  A fix from an exit that is
//               itself verified (the first disagreeing tile) is exact: a malformed record met there is an error of the file;
//   3. totals   records, excluded records (the flag filter), the output offset of every tile (an exclusive scan), the exit;
//   4. decode   one wavefront per tile walks its records again and writes every kept record as two-line FASTA (">\n" SEQ
//               "\n": the 4-bit codes =ACMGRSVTWYHKDBN as letters), 64 lanes over a record's bases.  The library maps that with
//               kmm_map_records: the LUT, the invalid-base rule, the radix / direct choice and the uniform-length path are
//               the ones every other input takes.
// The quality variant (<true> / k_bam_*_q; "use_record_qual" with a floor) writes every kept record as four-line
// FASTQ instead ("@\n" SEQ "\n+\n" QUAL "\n", the raw Phred bytes as Phred+33 clipped at '~'): 2 l_seq + 6 bytes per record, which
// the library maps as KMM_FORMAT_FASTQ, where "min_base_quality" is applied.
// The named form ("record_names"; k_bam_*_named) writes every selected record as four-line FASTQ WITH its identity:
// '@' NAME [ "/1" | "/2" ] '\n' SEQ '\n' "+\n" QUAL '\n' — the name's bytes outside '!' .. '~' as '?', absent qualities as '"' — the
// text the record-keep mode appends for BAM input.  Its length comes from the record's head too, so it is a third output form of
// spec, link and totals (FORM_NAMED), not a mechanism of its own.
// "original_strand"  has decode write the kept records whose FLAG has 0x10 in read orientation: SEQ reversed and
// complemented, QUAL reversed.  The output lengths are the same: spec, link and totals do not know of the switch.
// Record selection (kmm_select.hpp has the rule): with an include mask, a MAPQ floor or a region list set, spec, fix,
// decode and the CPU backend run as their <.., true> / k_bam_*_sel forms, which ask ONE predicate, kept(), about every record:
// counting and writing can never disagree.  Without one, the forms above run, as they did before the selection existed.
// The raw form ("record_bam"; k_bam_raw_*): behind the record-hits mode's decode and mapping, the selected records whose
// entry passes the keep rule are appended to the keep queue AS THEY STAND — block_size word and all — by a walk of the verified
// claims with the same predicate: a scan of the tiles' record counts, a count, a scan of the kept bytes, a copy, the tail's advance.
// Mates kept together in the raw form ("record_bam_mates"; k_bam_raw_*_pairs, k_bam_raw_pair_names, k_bam_raw_carry): the
// selected records are mates in file order; the count walk decides per pair, leaves every selected record's start by entry and
// reports an odd last record, the mate check compares the read_name bytes of every pair from those starts, and the mate 1 that a
// window left over goes to the queue from a buffer of the handle, in front of the next window's records.
// Exactness never depends on the plausibility test: a wrong guess only costs a fix.  Every read is bounds-checked against n.
// resync (kmm_bam_find_record_start) is the other use of the plausibility test: in inflated bytes that begin anywhere
// in the stream — a rank's share of a file — k_bam_resync finds the lowest position from which the chain of records holds to the
// end of the bytes.  There a wrong guess is caught by the share in front of it, whose last record it cuts.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "kmm_record_keep.hpp" // (the keep rule rk_keep and the store split rk_span of the raw form below)
#include "kmm_select.hpp"

#if defined(__HIPCC__)
#define KMM_BAM_HD __host__ __device__ __forceinline__
#else
#define KMM_BAM_HD inline
#endif

namespace kmm_bam {

constexpr uint64_t NONE = ~0ull;        // claim: no record starts in the tile (the exit of the tiles before passes through)
constexpr uint64_t INVALID = ~0ull - 1; // claim: the walk from the tile's start met a malformed record (never agrees)
constexpr uint32_t TILE = 16384;
constexpr int CHAIN = 4;
enum Rec { REC_OK = 0, REC_SHORT = 1, REC_BAD = 2 };

// One tile's claim: records starting in [entry, exit) (entry NONE / INVALID: see above); bytes = its kept records' output.
struct Tile {
    uint64_t entry, exit;
    uint32_t recs, excluded, bytes, spec; // spec: the claim comes from the speculative pass
};

// Host <-> device control words of the link passes (one struct, read back after every check).
struct Ctl {
    unsigned long long n_bad;        // claims that disagree, this pass
    unsigned long long first_bad;    // the first of them (its predecessors are verified)
    unsigned long long err_pos;      // a malformed record met from a verified start (NONE: none)
    unsigned long long false_starts; // speculative starts found to be wrong
};

struct Totals {
    unsigned long long recs, excluded, out_bytes, exit;
};

KMM_BAM_HD uint32_t rd32(const uint8_t *p)
{
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

KMM_BAM_HD uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }

struct RecHead {
    uint32_t bs, l_name, n_cigar, flag, l_seq;
};

// The record at d[p]: REC_OK (h filled), REC_SHORT (it does not end inside d[0, n)), REC_BAD (its fields cannot be a record's).
KMM_BAM_HD int record_at(const uint8_t *d, uint64_t n, uint64_t p, int32_t n_ref, RecHead &h)
{
    if (p > n || n - p < 4) // (overflow-safe: p may be any claim)
        return REC_SHORT;
    const uint32_t bs = rd32(d + p);
    if (bs < 32u || bs >= 0x80000000u)
        return REC_BAD;
    if (n - p - 4 < bs)
        return REC_SHORT;
    const int32_t ref = (int32_t)rd32(d + p + 4), next_ref = (int32_t)rd32(d + p + 24);
    const uint32_t l_name = d[p + 12], n_cigar = rd16(d + p + 16), flag = rd16(d + p + 18), l_seq = rd32(d + p + 20);
    if (ref < -1 || ref >= n_ref || next_ref < -1 || next_ref >= n_ref || l_name == 0 || l_seq >= 0x80000000u)
        return REC_BAD;
    if (32ull + l_name + 4ull * n_cigar + (l_seq + 1ull) / 2 + l_seq > (uint64_t)bs)
        return REC_BAD;
    if (d[p + 35 + l_name] != 0) // (read_name[l_read_name - 1]; inside the record: 32 + l_name <= bs)
        return REC_BAD;
    h.bs = bs;
    h.l_name = l_name;
    h.n_cigar = n_cigar;
    h.flag = flag;
    h.l_seq = l_seq;
    return REC_OK;
}

KMM_BAM_HD uint64_t seq_offset(const RecHead &h) { return 36ull + h.l_name + 4ull * h.n_cigar; }

// Could a record start at d[c]?  It is whole and consistent, and so are the CHAIN - 1 behind it (or the data ends there).
KMM_BAM_HD bool plausible(const uint8_t *d, uint64_t n, uint64_t c, int32_t n_ref)
{
    uint64_t p = c;
    for (int i = 0; i < CHAIN; ++i) {
        RecHead h;
        const int r = record_at(d, n, p, n_ref, h);
        if (r == REC_BAD)
            return false;
        if (r == REC_SHORT)
            return i > 0;
        p += 4ull + h.bs;
    }
    return true;
}

// ---- record selection: refID, pos, MAPQ and the CIGAR words lie in front of SEQ, inside the bounds record_at checked
using kmm_sel::Sel;

// The reference span of the record's CIGAR, the share of lane `lane` of `lanes` (operations lane, lane + lanes, ...): the lengths
// of M, D, N, = and X summed in 64 bits.  I, S, H and P never count; the long-CIGAR placeholder <l_seq>S<n>N counts its N.
KMM_BAM_HD uint64_t cigar_span_part(const uint8_t *rec, const RecHead &h, uint32_t lane, uint32_t lanes)
{
    const uint8_t *c = rec + 36ull + h.l_name;
    uint64_t span = 0;
    for (uint32_t j = lane; j < h.n_cigar; j += lanes) {
        const uint32_t w = rd32(c + 4ull * j);
        if (kmm_sel::consumes_ref(w))
            span += w >> 4;
    }
    return span;
}

// Rules 1 to 3 of the record at rec (flag masks, MAPQ) and what rule 4 says without the CIGAR: 1 kept, 0 not kept, -1 the
// CIGAR's span decides (the record starts outside every region and may reach into one).
KMM_BAM_HD int kept_without_cigar(const uint8_t *rec, const RecHead &h, const Sel &s)
{
    if (!kmm_sel::flags_pass(h.flag, s) || (uint32_t)rec[13] < s.min_mapq)
        return 0;
    if (s.n_iv == 0)
        return 1;
    const int32_t ref = (int32_t)rd32(rec + 4), pos = (int32_t)rd32(rec + 8);
    if (ref < 0)
        return s.keep_unplaced ? 1 : 0;
    if (kmm_sel::region_pass(s, ref, pos, h.flag, 0)) // (its first base lies in a region: no span can change that)
        return 1;
    return pos < 0 || (h.flag & kmm_sel::FLAG_UNMAPPED) || h.n_cigar == 0 ? 0 : -1;
}

// THE predicate: is the record at rec mapped?  S false: the exclude mask alone, as before the selection existed.  lanes > 1: the
// callers' lanes walk the CIGAR together, one after the other here (the CPU form of kept_wave below).
template <bool S>
KMM_BAM_HD bool kept(const uint8_t *rec, const RecHead &h, uint32_t excl, const Sel &s, uint32_t lanes = 1)
{
    if (!S)
        return !(h.flag & excl);
    const int r = kept_without_cigar(rec, h, s);
    if (r >= 0)
        return r != 0;
    uint64_t span = 0;
    for (uint32_t lane = 0; lane < lanes; ++lane)
        span += cigar_span_part(rec, h, lane, lanes);
    return kmm_sel::region_pass(s, (int32_t)rd32(rec + 4), (int32_t)rd32(rec + 8), h.flag, span);
}

struct Walk {
    uint64_t exit;
    uint32_t recs, excluded, bytes;
    bool bad;
};

// The output forms of a kept record: two-line FASTA, four-line FASTQ without a name (the quality variant), and the NAMED form
// ("record_names"): four-line FASTQ that carries QNAME and, when asked for, the mate suffix.  The templates below take
// the form as an int (their callers from before the named form pass false / true: 0 / 1).
constexpr int FORM_FASTA = 0, FORM_FASTQ = 1, FORM_NAMED = 2;

// Output bytes of one kept record: two-line FASTA, or (Q) four-line FASTQ.
template <int Q>
KMM_BAM_HD uint32_t out_len(uint32_t l_seq)
{
    return Q ? 2u * l_seq + 6u : l_seq + 3u;
}

// The mate suffix of the named form: 1 ("/1") iff FLAG has 0x40 and not 0x80, 2 ("/2") iff 0x80 and not 0x40, else 0 (none) — the
// rule of `samtools fastq` without -n.  on: "record_names_mate_suffix".
KMM_BAM_HD uint32_t mate_of(uint32_t flag, bool on)
{
    const uint32_t m = flag & 0xC0u;
    return !on ? 0u : m == 0x40u ? 1u : m == 0x80u ? 2u : 0u;
}

// Output bytes of one kept record in the named form: '@' NAME [/1 | /2] '\n' SEQ '\n' "+\n" QUAL '\n' — from the record's head
// alone, as the other forms' (l_name >= 1: record_at).
KMM_BAM_HD uint32_t out_len_named(const RecHead &h, bool sfx)
{
    return (h.l_name - 1u) + (mate_of(h.flag, sfx) ? 2u : 0u) + 2u * h.l_seq + 6u;
}

template <int Q>
KMM_BAM_HD uint32_t rec_out_len(const RecHead &h, bool sfx)
{
    return Q == FORM_NAMED ? out_len_named(h, sfx) : out_len<Q>(h.l_seq);
}

// Walk::bytes and Tile::bytes are uint32.  The records that start in one tile, all but the last, end before the next one starts,
// i.e. inside the tile: their 4 + block_size sum to less than TILE, there are at most TILE / 36 of them (block_size >= 32), and
// l_seq + (l_seq + 1) / 2 <= block_size bounds every l_seq by 2/3 block_size.  The last one has block_size < 2^31.  So a tile's
// quality output is below 2 * (2/3) * (TILE + 2^31) + 6 * (TILE / 36 + 1) (the FASTA output is smaller still).  The named form
// adds a record's name and mate suffix: l_name - 1 <= 254 and 2 more bytes, at most 256 per record:
constexpr uint64_t MAX_TILE_OUT = 4ull * ((uint64_t)TILE + 0x80000000ull) / 3 + (6ull + 256ull) * (TILE / 36 + 1);
static_assert(MAX_TILE_OUT < 0x100000000ull, "a tile's output bytes fit uint32");
// The raw form ("record_bam") keeps a record as its own 4 + block_size bytes: by the same argument the kept raw bytes of
// a tile are below TILE (the records that end inside it) plus 4 + (2^31 - 1) (the last one):
constexpr uint64_t MAX_TILE_RAW = (uint64_t)TILE + 4ull + 0x7FFFFFFFull;
static_assert(MAX_TILE_RAW < 0x100000000ull, "a tile's kept raw bytes fit uint32");

// The chain from p (a record start) to the first start at or past te; it stops early at a record that does not end inside
// d[0, n) (exit = its start) or at a malformed one (bad, exit = its start).
template <int Q = 0, bool S = false>
KMM_BAM_HD void walk(const uint8_t *d, uint64_t n, uint64_t p, uint64_t te, int32_t n_ref, uint32_t excl, Walk &w, const Sel &sel = Sel(),
                     bool sfx = false)
{
    w.recs = w.excluded = w.bytes = 0;
    w.bad = false;
    while (p < te) {
        RecHead h;
        const int r = record_at(d, n, p, n_ref, h);
        if (r == REC_SHORT)
            break;
        if (r == REC_BAD) {
            w.bad = true;
            break;
        }
        if (!kept<S>(d + p, h, excl, sel))
            ++w.excluded;
        else {
            ++w.recs;
            w.bytes += rec_out_len<Q>(h, sfx);
        }
        p += 4ull + h.bs;
    }
    w.exit = p;
}

KMM_BAM_HD uint64_t tile_end(uint64_t t, uint64_t n) { return (t + 1) * TILE < n ? (t + 1) * TILE : n; }

// The claim of tile t once its start is known (entry = a record start) or guessed.
template <int Q = 0, bool S = false>
KMM_BAM_HD void claim_from(const uint8_t *d, uint64_t n, uint64_t t, uint64_t entry, int32_t n_ref, uint32_t excl, uint32_t spec,
                           Tile &o, const Sel &sel = Sel(), bool sfx = false)
{
    o.spec = spec;
    if (entry == NONE) {
        o.entry = o.exit = NONE;
        o.recs = o.excluded = o.bytes = 0;
        return;
    }
    Walk w;
    walk<Q, S>(d, n, entry, tile_end(t, n), n_ref, excl, w, sel, sfx);
    o.entry = w.bad ? INVALID : entry;
    o.exit = w.bad ? INVALID : w.exit;
    o.recs = w.recs;
    o.excluded = w.excluded;
    o.bytes = w.bytes;
}

// The exit of the tiles before t, as the claims `in` say (start0 in front of tile 0).
KMM_BAM_HD uint64_t prev_exit(const Tile *in, uint64_t t, uint64_t start0)
{
    while (t > 0) {
        --t;
        if (in[t].entry != NONE)
            return in[t].exit;
    }
    return start0;
}

// Does tile t's claim agree with the exit `prev` of the tiles before it?
KMM_BAM_HD bool agrees(const uint8_t *d, uint64_t n, uint64_t t, const Tile &c, uint64_t prev, int32_t n_ref)
{
    if (c.entry != NONE)
        return c.entry == prev;
    if (prev >= tile_end(t, n))
        return true;
    RecHead h;
    return record_at(d, n, prev, n_ref, h) == REC_SHORT; // (the data end inside the record that starts at prev)
}

// ---- the per-tile steps, shared by the kernels and the CPU backend ----

// spec, one tile (scalar form: the kernel tests 64 positions at a time, with the same `plausible`)
template <int Q = 0, bool S = false>
inline void spec_tile_scalar(const uint8_t *d, uint64_t n, uint64_t t, uint64_t start0, int32_t n_ref, uint32_t excl, Tile &o,
                             const Sel &sel = Sel(), bool sfx = false)
{
    uint64_t entry = NONE;
    if (t == 0)
        entry = start0;
    else
        for (uint64_t c = t * TILE, e = tile_end(t, n); c < e && entry == NONE; ++c)
            if (plausible(d, n, c, n_ref))
                entry = c;
    claim_from<Q, S>(d, n, t, entry, n_ref, excl, 1u, o, sel, sfx);
}

// fix, one tile: its claim is walked again from the exit before it.  verified: that exit is exact (t is the first tile
// that disagrees), so a malformed record met on the way is an error of the file (returns its position, else NONE).
template <int Q = 0, bool S = false>
KMM_BAM_HD uint64_t fix_tile(const uint8_t *d, uint64_t n, uint64_t t, uint64_t prev, bool verified, int32_t n_ref, uint32_t excl,
                             Tile &o, const Sel &sel = Sel(), bool sfx = false)
{
    Walk w;
    walk<Q, S>(d, n, prev, tile_end(t, n), n_ref, excl, w, sel, sfx);
    o.spec = 0;
    o.recs = w.recs;
    o.excluded = w.excluded;
    o.bytes = w.bytes;
    if (w.bad) {
        o.entry = o.exit = INVALID;
        return verified ? w.exit : NONE;
    }
    o.entry = prev;
    o.exit = w.exit;
    return NONE;
}

// ---- resync (kmm_bam_find_record_start): where does the first record start in inflated bytes d[0, n) that begin
// somewhere in the stream?  The smallest position from which the chain of records holds to the end of d.

// Does the chain from p hold?  Every record is REC_OK until one is REC_SHORT at the end of the bytes, at least one is whole,
// and at the end of the file (at_eof) the chain ends exactly at n.  A true record start always holds.
KMM_BAM_HD bool chain_holds(const uint8_t *d, uint64_t n, uint64_t p, int32_t n_ref, bool at_eof)
{
    bool whole = false;
    for (;;) { // (p grows by at least 36 per round)
        RecHead h;
        const int r = record_at(d, n, p, n_ref, h);
        if (r == REC_BAD)
            return false;
        if (r == REC_SHORT)
            return whole && (!at_eof || p == n);
        whole = true;
        p += 4ull + h.bs;
    }
}

// resync, one tile (scalar form: the kernel tests 64 positions at a time, with the same `plausible` — which every holding
// position passes — and walks the survivors in ascending order): the tile's lowest holding position, or NONE
inline uint64_t resync_tile_scalar(const uint8_t *d, uint64_t n, uint64_t t, int32_t n_ref, bool at_eof)
{
    for (uint64_t c = t * TILE, e = tile_end(t, n); c < e; ++c)
        if (plausible(d, n, c, n_ref) && chain_holds(d, n, c, n_ref, at_eof))
            return c;
    return NONE;
}

// resync, all tiles (the CPU form of k_bam_resync): the lowest holding position of d[0, n), or NONE
inline uint64_t resync_scalar(const uint8_t *d, uint64_t n, int32_t n_ref, bool at_eof)
{
    for (uint64_t t = 0, n_tiles = (n + TILE - 1) / TILE; t < n_tiles; ++t) {
        const uint64_t p = resync_tile_scalar(d, n, t, n_ref, at_eof);
        if (p != NONE)
            return p;
    }
    return NONE;
}

// The inflated position p as (member, offset inside it): the member that HOLDS byte p, i.e. the first one that ends behind p
// (empty members hold nothing).  m_off / o_off: where the n_members members start in the compressed / inflated bytes
// (n_members + 1 entries each).  p at or behind the last member's end: (m_off[n_members], 0).
inline void locate(const unsigned long long *m_off, const unsigned long long *o_off, uint64_t n_members, uint64_t p, int64_t *member,
                   int64_t *skip)
{
    uint64_t lo = 0, hi = n_members; // the first j with o_off[j + 1] > p
    while (lo < hi) {
        const uint64_t mid = (lo + hi) / 2;
        if (o_off[mid + 1] > p)
            hi = mid;
        else
            lo = mid + 1;
    }
    *member = (int64_t)m_off[lo];
    *skip = lo < n_members ? (int64_t)(p - o_off[lo]) : 0;
}

// The bytes a resync examines of a window whose whole members inflate to n_total bytes: all of them, or `cap` (the test hook;
// 0: none).  *at_eof: the window's whole members end where the window does (whole) and every byte is examined — the caller
// brought the rest of the file.
inline uint64_t resync_extent(uint64_t n_total, uint64_t cap, bool whole, bool *at_eof)
{
    const uint64_t n = cap && cap < n_total ? cap : n_total;
    *at_eof = whole && n == n_total;
    return n;
}

// What kmm_bam_find_record_start answers: `best` = the lowest holding position (NONE: no chain holds) as (member, skip); at the
// end of the file, with no record start in the bytes, (m_off[n_members], 0) — they end a record that began in front of them,
// or are empty; else member -1: a longer window is needed.
inline void resync_answer(const unsigned long long *m_off, const unsigned long long *o_off, uint64_t n_members, uint64_t best, bool at_eof,
                          int64_t *member, int64_t *skip)
{
    *member = -1;
    *skip = 0;
    if (best != NONE)
        locate(m_off, o_off, n_members, best, member, skip);
    else if (at_eof)
        *member = (int64_t)m_off[n_members];
}

// "=ACMGRSVTWYHKDBN": the letters of the 4-bit base codes (SAM/BAM specification 4.2.3)
KMM_BAM_HD uint8_t base_letter(uint32_t code)
{
    return (uint8_t)"=ACMGRSVTWYHKDBN"[code & 15u];
}

// decode, one record's output (lane `lane` of `lanes`): ">\n" + letters + "\n" at out[o]
KMM_BAM_HD void decode_record(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes)
{
    const uint8_t *seq = rec + seq_offset(h);
    const uint32_t n_bytes = (h.l_seq + 1u) / 2u;
    if (lane == 0) {
        out[0] = '>';
        out[1] = '\n';
        out[2 + h.l_seq] = '\n';
    }
    for (uint32_t j = lane; j < n_bytes; j += lanes) {
        const uint32_t b = seq[j];
        out[2 + 2 * j] = base_letter(b >> 4);
        if (2 * j + 1 < h.l_seq)
            out[3 + 2 * j] = base_letter(b);
    }
}

// The quality bytes of a record (l_seq raw Phred values behind the packed bases; inside block_size: record_at)
KMM_BAM_HD const uint8_t *qual_of(const uint8_t *rec, const RecHead &h) { return rec + seq_offset(h) + (h.l_seq + 1u) / 2u; }

// Are the record's qualities absent?  (0xFF bytes; as htslib, the first one decides.)  A record without bases has none to miss.
KMM_BAM_HD bool qual_absent(const uint8_t *rec, const RecHead &h) { return h.l_seq > 0 && qual_of(rec, h)[0] == 0xFFu; }

// A raw Phred byte as Phred+33 text, clipped at '~': 0xFF (absent) and every byte >= 93 become '~', which no floor <= 93 masks.
KMM_BAM_HD uint8_t qual_letter(uint32_t q) { return (uint8_t)(q >= 93u ? 126u : q + 33u); }

// decode, the quality variant: "@\n" + letters + "\n+\n" + qualities + "\n" at out[0] (2 l_seq + 6 bytes)
KMM_BAM_HD void decode_record_q(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes)
{
    const uint8_t *seq = rec + seq_offset(h), *qual = qual_of(rec, h);
    const uint32_t n_bytes = (h.l_seq + 1u) / 2u;
    uint8_t *oq = out + 5ull + h.l_seq;
    if (lane == 0) {
        out[0] = '@';
        out[1] = '\n';
        out[2ull + h.l_seq] = '\n';
        out[3ull + h.l_seq] = '+';
        out[4ull + h.l_seq] = '\n';
        oq[h.l_seq] = '\n';
    }
    for (uint32_t j = lane; j < n_bytes; j += lanes) {
        const uint32_t b = seq[j];
        out[2ull + 2ull * j] = base_letter(b >> 4);
        oq[2ull * j] = qual_letter(qual[2ull * j]);
        if (2 * j + 1 < h.l_seq) {
            out[3ull + 2ull * j] = base_letter(b);
            oq[2ull * j + 1] = qual_letter(qual[2ull * j + 1]);
        }
    }
}

// ---- "original_strand" (DESIGN 4.13): a kept record whose FLAG has 0x10 is stored reverse-complemented; the reversed forms
// below write it in read orientation.  The output lengths are the forward forms', so nothing but decode knows of the switch.
constexpr uint32_t FLAG_REVERSE = 0x10u;

// The complement of a 4-bit base code is the code with its four bits reversed (A 1 <-> T 8, C 2 <-> G 4, M 3 <-> K 12, ...;
// '=' 0 and N 15 are their own): "=TGKCYSBAWRDMHVN", htslib's table.
KMM_BAM_HD uint32_t comp_code(uint32_t code)
{
    return ((code & 1u) << 3) | ((code & 2u) << 1) | ((code & 4u) >> 1) | ((code & 8u) >> 3);
}

// Is the record one the switch flips?  (0x10 and at least one base; wave-uniform: it depends on the record's head alone.)
KMM_BAM_HD bool flipped(const RecHead &h, bool orig) { return orig && (h.flag & FLAG_REVERSE) != 0u && h.l_seq > 0u; }

// decode, reversed: base i of the stored SEQ goes to position l_seq - 1 - i as its complement.  Byte j holds bases 2j (high
// nibble) and 2j + 1 (low), which land side by side at l_seq - 2 - 2j and l_seq - 1 - 2j: the lanes of a wavefront store one
// contiguous run, descending.  The low nibble of the last byte of an odd l_seq is padding: it would land on out[1], in front of
// the sequence, and is not written.
KMM_BAM_HD void decode_record_rev(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes)
{
    const uint8_t *seq = rec + seq_offset(h);
    const uint32_t n_bytes = (h.l_seq + 1u) / 2u;
    if (lane == 0) {
        out[0] = '>';
        out[1] = '\n';
        out[2ull + h.l_seq] = '\n';
    }
    uint8_t *last = out + 1ull + h.l_seq; // the sequence's last byte
    for (uint32_t j = lane; j < n_bytes; j += lanes) {
        const uint32_t b = seq[j];
        last[-2ll * j] = base_letter(comp_code(b >> 4));
        if (2 * j + 1 < h.l_seq)
            last[-2ll * j - 1] = base_letter(comp_code(b & 15u));
    }
}

// decode, the quality variant, reversed: the letters as above, qual[i] at oq[l_seq - 1 - i] (reversed, not complemented)
KMM_BAM_HD void decode_record_q_rev(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes)
{
    const uint8_t *seq = rec + seq_offset(h), *qual = qual_of(rec, h);
    const uint32_t n_bytes = (h.l_seq + 1u) / 2u;
    uint8_t *oq = out + 5ull + h.l_seq;
    if (lane == 0) {
        out[0] = '@';
        out[1] = '\n';
        out[2ull + h.l_seq] = '\n';
        out[3ull + h.l_seq] = '+';
        out[4ull + h.l_seq] = '\n';
        oq[h.l_seq] = '\n';
    }
    uint8_t *last = out + 1ull + h.l_seq, *qlast = oq + h.l_seq - 1ull; // (l_seq 0: n_bytes 0, neither is used)
    for (uint32_t j = lane; j < n_bytes; j += lanes) {
        const uint32_t b = seq[j];
        last[-2ll * j] = base_letter(comp_code(b >> 4));
        qlast[-2ll * j] = qual_letter(qual[2ull * j]);
        if (2 * j + 1 < h.l_seq) {
            last[-2ll * j - 1] = base_letter(comp_code(b & 15u));
            qlast[-2ll * j - 1] = qual_letter(qual[2ull * j + 1]);
        }
    }
}

// ---- the named form ("record_names"): '@' NAME [/1 | /2] '\n' SEQ '\n' "+\n" QUAL '\n'
// A name byte as text: the bytes outside 0x21 .. 0x7E ('!' .. '~') become '?' — a NUL in the middle, a tab or a newline in a
// damaged file cannot break the line arithmetic of the records front end.
KMM_BAM_HD uint8_t name_letter(uint32_t c) { return (uint8_t)(c - 0x21u <= 0x5Du ? c : (uint32_t)'?'); }

// The quality letter every base of a record without qualities gets: '"' (Phred 1), the default of `samtools fastq -v 1` — not the
// '~' of the floor variant, which passes a floor but would claim the best quality in a file that is kept.
constexpr uint8_t QUAL_ABSENT_LETTER = 0x22u;

// The head of a named record, the share of lane `lane` of `lanes`: '@', the name (bytes lane, lane + lanes, ...), the suffix and
// the three line ends around SEQ and QUAL.  Returns how many of ITS name bytes the lane replaced, and *body = where SEQ starts.
KMM_BAM_HD uint32_t named_head(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes, bool sfx, uint8_t **body)
{
    const uint8_t *name = rec + 36;
    const uint32_t nl = h.l_name - 1u, mate = mate_of(h.flag, sfx);
    uint8_t *seq = out + 1ull + nl + (mate ? 2u : 0u) + 1ull;
    uint32_t replaced = 0;
    for (uint32_t j = lane; j < nl; j += lanes) {
        const uint32_t c = name[j];
        const uint8_t t = name_letter(c);
        out[1ull + j] = t;
        replaced += t != c ? 1u : 0u;
    }
    if (lane == 0) {
        out[0] = '@';
        if (mate) {
            out[1ull + nl] = '/';
            out[2ull + nl] = (uint8_t)('0' + mate);
        }
        seq[-1] = '\n';
        seq[h.l_seq] = '\n';
        seq[1ull + h.l_seq] = '+';
        seq[2ull + h.l_seq] = '\n';
        seq[3ull + 2ull * h.l_seq] = '\n';
    }
    *body = seq;
    return replaced;
}

// decode, the named form (lane `lane` of `lanes`): out_len_named bytes at out[0]; returns the lane's replaced name bytes.  The
// letters are decode_record's, the qualities qual_letter's — or QUAL_ABSENT_LETTER throughout when the record stores none.
KMM_BAM_HD uint32_t decode_record_named(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes, bool sfx)
{
    uint8_t *os;
    const uint32_t replaced = named_head(rec, h, out, lane, lanes, sfx, &os);
    const uint8_t *seq = rec + seq_offset(h), *qual = qual_of(rec, h);
    const uint32_t n_bytes = (h.l_seq + 1u) / 2u;
    const bool absent = qual_absent(rec, h);
    uint8_t *oq = os + 3ull + h.l_seq;
    for (uint32_t j = lane; j < n_bytes; j += lanes) {
        const uint32_t b = seq[j];
        os[2ull * j] = base_letter(b >> 4);
        oq[2ull * j] = absent ? QUAL_ABSENT_LETTER : qual_letter(qual[2ull * j]);
        if (2 * j + 1 < h.l_seq) {
            os[2ull * j + 1] = base_letter(b);
            oq[2ull * j + 1] = absent ? QUAL_ABSENT_LETTER : qual_letter(qual[2ull * j + 1]);
        }
    }
    return replaced;
}

// decode, the named form, reversed (a record flipped() accepts: l_seq > 0): SEQ complemented and reversed, QUAL reversed, as
// decode_record_q_rev writes them; the name is not touched by the strand.
KMM_BAM_HD uint32_t decode_record_named_rev(const uint8_t *rec, const RecHead &h, uint8_t *out, uint32_t lane, uint32_t lanes, bool sfx)
{
    uint8_t *os;
    const uint32_t replaced = named_head(rec, h, out, lane, lanes, sfx, &os);
    const uint8_t *seq = rec + seq_offset(h), *qual = qual_of(rec, h);
    const uint32_t n_bytes = (h.l_seq + 1u) / 2u;
    const bool absent = qual_absent(rec, h);
    uint8_t *last = os + h.l_seq - 1ull, *qlast = os + 2ull + 2ull * h.l_seq; // the last letter, the last quality
    for (uint32_t j = lane; j < n_bytes; j += lanes) {
        const uint32_t b = seq[j];
        last[-2ll * j] = base_letter(comp_code(b >> 4));
        qlast[-2ll * j] = absent ? QUAL_ABSENT_LETTER : qual_letter(qual[2ull * j]);
        if (2 * j + 1 < h.l_seq) {
            last[-2ll * j - 1] = base_letter(comp_code(b & 15u));
            qlast[-2ll * j - 1] = absent ? QUAL_ABSENT_LETTER : qual_letter(qual[2ull * j + 1]);
        }
    }
    return replaced;
}

// ---- the raw form ("record_bam"): behind the record-hits mode, the selected records whose entry passes the keep rule
// are appended to the keep queue as they stand in the file — d[p, p + 4 + block_size), untouched.  Selected record i of tile t
// (in file order) has entry first + rec_base[t] + i of the call's entries, rec_base = the exclusive scan of Tile::recs.
KMM_BAM_HD uint32_t raw_len(const RecHead &h) { return 4u + h.bs; } // (block_size < 2^31: record_at)

// The walk of one verified tile: every selected record (is_selected: the predicate spec, fix and decode asked) meets its entry;
// visit(p, len, off) is called for the kept ones, in file order — off = the raw bytes of the tile's kept records in front of it.
// Every read of d is bounded by record_at, every entry index by n_entries and by the tile's own count.  Returns the tile's kept
// raw bytes; *kept_recs its kept records.
template <class Selected, class Visit>
KMM_BAM_HD uint32_t raw_walk_tile(const uint8_t *d, uint64_t n, int32_t n_ref, const Tile &c, uint64_t entry0, const uint32_t *hits,
                                  const uint32_t *windows, uint64_t n_entries, const RkRule &rule, uint32_t *kept_recs,
                                  Selected &&is_selected, Visit &&visit)
{
    uint32_t bytes = 0, recs = 0;
    if (c.entry != NONE && c.entry != INVALID && c.recs != 0) {
        uint64_t p = c.entry, e = entry0;
        const uint64_t e_end = entry0 + c.recs;
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (is_selected(d + p, h)) {
                if (e >= e_end || e >= n_entries) // (cannot happen: the walk that counted and this one ask one predicate)
                    break;
                if (rk_keep(hits[e], windows ? windows[e] : 0u, rule)) {
                    visit(p, raw_len(h), bytes);
                    bytes += raw_len(h);
                    ++recs;
                }
                ++e;
            }
            p += 4ull + h.bs;
        }
    }
    *kept_recs = recs;
    return bytes;
}

// Where a kept record goes: the queue's tail, the kept raw bytes of the tiles in front, those of the tile's kept records in front.
KMM_BAM_HD uint64_t raw_dest(uint64_t tail, uint64_t tile_base, uint32_t off) { return tail + tile_base + off; }

// The share of lane `lane` of `lanes` in copying the len bytes at src to queue[dst, dst + len) (queue: 16-byte aligned).  rk_span
// states the split: the ragged head and tail of the destination byte by byte, its aligned middle as 16-byte lines — one store
// each, from one 16-byte load at whatever alignment the source has.  Nothing outside [dst, dst + len) is written, nothing of
// the queue is read, nothing outside src[0, len) is read.
KMM_BAM_HD void raw_copy_part(const uint8_t *src, uint8_t *queue, uint64_t dst, uint32_t len, uint32_t lane, uint32_t lanes)
{
    const uint32_t a = (uint32_t)(dst & 15u);
    uint8_t *g = queue + (dst - a); // (the 16-byte line the record starts in: g[i] takes src[i - a])
    const RkSpan sp = rk_span(a, len);
    for (uint32_t i = a + lane; i < sp.head_end; i += lanes)
        g[i] = src[i - a];
    for (uint32_t i = sp.full_begin + 16u * lane; i < sp.full_end; i += 16u * lanes) {
        uint32_t x[4];
        __builtin_memcpy(x, src + (i - a), 16);
        __builtin_memcpy(__builtin_assume_aligned(g + i, 16), x, 16);
    }
    for (uint32_t i = sp.tail_begin + lane; i < a + len; i += lanes)
        g[i] = src[i - a];
}

// ---- mates kept together in the raw form ("record_bam_mates"): the selected records of the stream are mates in file
// order, 2p and 2p + 1, kept or dropped together.  A call's entries are those of its whole pairs, n_entries = 2P of them; a mate 1
// that the window before left over is entry 0 (`carried` = 1: its raw bytes wait in a buffer of the handle), so selected record i
// of the call has entry carried + i.  The record whose entry would be 2P is the odd last one: it waits for the next call.

// The two entries of the pair that entry e belongs to.
KMM_BAM_HD uint64_t pair_first(uint64_t e) { return e & ~1ull; }
KMM_BAM_HD uint64_t pair_second(uint64_t e) { return e | 1ull; }

// Is the pair of entry e kept?  Both indices are bounded by the call's entry count.
KMM_BAM_HD bool raw_pair_kept(const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, uint64_t e, const RkPairRule &rule)
{
    const uint64_t a = pair_first(e), b = pair_second(e);
    if (b >= n_entries)
        return false;
    return rk_pair_keep(hits[a], windows ? windows[a] : 0u, hits[b], windows ? windows[b] : 0u, rule.rule, rule.pair_rule);
}

// The bytes the carried mate 1 takes in front of the tiles' records: its length when its pair (entries 0 and 1) is kept.
KMM_BAM_HD uint64_t raw_carry_shift(const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const RkPairRule &rule, uint32_t carried,
                                    uint32_t carry_len)
{
    return carried && raw_pair_kept(hits, windows, n_entries, 0, rule) ? carry_len : 0u;
}

// The pair form of raw_walk_tile: entry0 = carried + the record base of the tile.  at(e, p) for every selected record that has an
// entry (the mate check reads the starts by entry); visit(p, len, off) for every record of a kept pair; odd(p, len) for the odd
// last record, which is neither counted nor visited (no selected record lies behind it).
template <class Selected, class At, class Visit, class Odd>
KMM_BAM_HD uint32_t raw_walk_tile_pairs(const uint8_t *d, uint64_t n, int32_t n_ref, const Tile &c, uint64_t entry0, const uint32_t *hits,
                                        const uint32_t *windows, uint64_t n_entries, const RkPairRule &rule, uint32_t *kept_recs,
                                        Selected &&is_selected, At &&at, Visit &&visit, Odd &&odd)
{
    uint32_t bytes = 0, recs = 0;
    if (c.entry != NONE && c.entry != INVALID && c.recs != 0) {
        uint64_t p = c.entry, e = entry0;
        const uint64_t e_end = entry0 + c.recs;
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (is_selected(d + p, h)) {
                if (e >= e_end) // (cannot happen: the walk that counted and this one ask one predicate)
                    break;
                if (e >= n_entries) {
                    if (e == n_entries)
                        odd(p, raw_len(h));
                    break;
                }
                at(e, p);
                if (raw_pair_kept(hits, windows, n_entries, e, rule)) {
                    visit(p, raw_len(h), bytes);
                    bytes += raw_len(h);
                    ++recs;
                }
                ++e;
            }
            p += 4ull + h.bs;
        }
    }
    *kept_recs = recs;
    return bytes;
}

// The mate check compares read_name as it stands: l bytes (l_read_name, the NUL included) at na and nb; the share of lane `lane`
// of `lanes` — true iff one of its bytes differs.  The callers have compared the two lengths.
KMM_BAM_HD bool names_differ_part(const uint8_t *na, const uint8_t *nb, uint32_t l, uint32_t lane, uint32_t lanes)
{
    bool diff = false;
#if defined(__HIPCC__)
#pragma unroll 1
#endif
    for (uint32_t i = lane; i < l; i += lanes)
        diff |= na[i] != nb[i];
    return diff;
}

// The mate check of one pair: the records of entries 2P and 2P + 1 start at pos_a and pos_b of d[0, consumed) — the count walk left
// the starts there, NONE where it left none — or, for the mate 1 that was carried in (a_carry: carry[0, carry_len) holds its raw
// bytes), in the carry buffer.  Mates have equal l_read_name and equal read_name bytes; differ(na, nb, l) says whether any lane
// found a difference.  Every read is bounded: the fixed head and the name lie in front of `consumed` (of carry_len).  True iff
// the two are no mates; a pair whose starts are not both known is none.
template <class Differ>
KMM_BAM_HD bool raw_names_pair(const uint8_t *d, uint64_t consumed, uint64_t pos_a, uint64_t pos_b, bool a_carry, const uint8_t *carry,
                               uint32_t carry_len, Differ &&differ)
{
    const uint8_t *a = a_carry ? carry : d + pos_a;
    const uint64_t a_room = a_carry ? (uint64_t)carry_len : (pos_a < consumed ? consumed - pos_a : 0ull);
    const uint64_t b_room = pos_b < consumed ? consumed - pos_b : 0ull;
    if ((a_carry ? carry == nullptr : pos_a == NONE) || pos_b == NONE || a_room < 37 || b_room < 37)
        return true;
    const uint8_t *b = d + pos_b;
    const uint32_t la = a[12], lb = b[12];
    if (36ull + la > a_room || 36ull + lb > b_room)
        return true;
    return la != lb || differ(a + 36, b + 36, la);
}

// ---- the header (host side: the library reads it back once per stream) ----

// d[0, n) = the stream's first inflated bytes.  0: the header ends at *hdr_end and names *n_ref references; 1: it goes on
// behind n; -1: it is no BAM header (magic, or a length no header can have).
inline int parse_header(const uint8_t *d, uint64_t n, uint64_t *hdr_end, int32_t *n_ref)
{
    static const uint8_t magic[4] = {'B', 'A', 'M', 1};
    if (memcmp(d, magic, n < 4 ? (size_t)n : 4) != 0)
        return -1;
    if (n < 8)
        return 1;
    const uint32_t l_text = rd32(d + 4);
    if (l_text >= 0x80000000u)
        return -1;
    uint64_t p = 8ull + l_text;
    if (p + 4 > n)
        return 1;
    const uint32_t nr = rd32(d + p);
    if (nr >= 0x80000000u)
        return -1;
    p += 4;
    for (uint32_t i = 0; i < nr; ++i) {
        if (p + 4 > n)
            return 1;
        const uint32_t l_name = rd32(d + p);
        if (l_name == 0 || l_name >= 0x80000000u)
            return -1;
        p += 4ull + l_name + 4ull;
        if (p > n)
            return 1;
    }
    *hdr_end = p;
    *n_ref = (int32_t)nr;
    return 0;
}

// ---- the orchestration, written once against a backend (GPU: BamGpuBackend, kmm_bam_host.hpp; CPU: CpuBackend below) ----
//   be.spec(n_tiles, start0)                 the speculative claims into the current buffer
//   be.check(n_tiles, start0, Ctl &)         counts the claims that disagree (synchronises: the control words come back)
//   be.fix(n_tiles, start0)                  the disagreeing claims walked again, into the other buffer; swaps the buffers
//   be.totals(n_tiles, start0, Totals &)     output offsets of the tiles + totals (synchronises)
struct CallOut {
    uint64_t consumed = 0;           // where the last complete record ends (the bytes behind it are carried over)
    uint64_t recs = 0, excluded = 0, out_bytes = 0;
    uint64_t false_starts = 0, continuations = 0;
    uint64_t err_pos = NONE;         // a malformed record (nothing of the call may be mapped)
};

template <class B>
int run_call(B &be, uint64_t n, uint64_t start0, CallOut &co)
{
    co = CallOut();
    if (start0 >= n) {
        co.consumed = start0 < n ? start0 : n;
        return 0;
    }
    const uint64_t n_tiles = (n + TILE - 1) / TILE;
    int rc = be.spec(n_tiles, start0);
    for (int pass = 0; rc == 0; ++pass) {
        Ctl c;
        if ((rc = be.check(n_tiles, start0, c)) != 0)
            break;
        co.false_starts = c.false_starts;
        if (c.err_pos != NONE) {
            co.err_pos = c.err_pos;
            return 0;
        }
        if (c.n_bad == 0)
            break;
        co.continuations += c.n_bad;
        rc = be.fix(n_tiles, start0);
    }
    if (rc != 0)
        return rc;
    Totals t;
    if ((rc = be.totals(n_tiles, start0, t)) != 0)
        return rc;
    co.recs = t.recs;
    co.excluded = t.excluded;
    co.out_bytes = t.out_bytes;
    co.consumed = t.exit;
    return 0;
}

// The CPU backend (the tests): the same per-tile steps in loops; decode() writes the two-line FASTA of the call (or its four-line
// FASTQ: `qual`, `named`).
struct CpuBackend {
    const uint8_t *d = nullptr;
    uint64_t n = 0;
    int32_t n_ref = 0;
    uint32_t excl = 0;
    bool qual = false;     // the quality variant: decode() writes four-line FASTQ
    uint64_t no_qual = 0;  // kept records whose qualities are absent (counted by decode() of the quality variant)
    bool orig = false;     // "original_strand": decode() writes the kept records with FLAG 0x10 in read orientation
    uint64_t reversed = 0; // the records decode() flipped
    uint32_t lanes = 1;    // lanes decode() gives the per-record functions (the tests: 1 and 64), one after the other
    Sel sel;               // the selection beyond excl (its own excl is not read: eff()); default: flags only
    bool named = false;    // the named form ("record_names"): decode() writes four-line FASTQ with QNAME; `qual` is not read
    bool mate_suffix = false; // the named form: "/1" / "/2" behind the name ("record_names_mate_suffix")
    uint64_t replaced = 0; // the named form: name bytes outside '!' .. '~' that decode() wrote as '?'
    std::vector<Tile> cur, nxt;
    std::vector<uint64_t> base;
    uint64_t false_starts = 0;

    Sel eff() const
    {
        Sel s = sel;
        s.excl = excl;
        return s;
    }
    bool is_kept(uint64_t p, const RecHead &h) const
    {
        return sel.flags_only() && !named ? kept<false>(d + p, h, excl, sel) : kept<true>(d + p, h, excl, eff(), lanes);
    }
    int spec(uint64_t n_tiles, uint64_t start0)
    {
        cur.assign(n_tiles, Tile());
        nxt.assign(n_tiles, Tile());
        false_starts = 0;
        first_bad = err_pos = NONE;
        const bool s = !sel.flags_only();
        for (uint64_t t = 0; t < n_tiles; ++t)
            if (named) // (one form for every selection, as the kernels: kept<true> with no selection set is the exclude mask)
                spec_tile_scalar<FORM_NAMED, true>(d, n, t, start0, n_ref, excl, cur[t], eff(), mate_suffix);
            else if (qual && s)
                spec_tile_scalar<true, true>(d, n, t, start0, n_ref, excl, cur[t], eff());
            else if (s)
                spec_tile_scalar<false, true>(d, n, t, start0, n_ref, excl, cur[t], eff());
            else if (qual)
                spec_tile_scalar<true>(d, n, t, start0, n_ref, excl, cur[t]);
            else
                spec_tile_scalar(d, n, t, start0, n_ref, excl, cur[t]);
        return 0;
    }
    uint64_t first_bad = NONE, err_pos = NONE;
    int check(uint64_t n_tiles, uint64_t start0, Ctl &c)
    {
        c.n_bad = 0;
        c.first_bad = NONE;
        c.err_pos = err_pos;
        for (uint64_t t = 0; t < n_tiles; ++t)
            if (!agrees(d, n, t, cur[t], prev_exit(cur.data(), t, start0), n_ref)) {
                ++c.n_bad;
                if (c.first_bad == NONE)
                    c.first_bad = t;
            }
        first_bad = c.first_bad;
        c.false_starts = false_starts;
        return 0;
    }
    int fix(uint64_t n_tiles, uint64_t start0)
    {
        for (uint64_t t = 0; t < n_tiles; ++t) {
            const uint64_t prev = prev_exit(cur.data(), t, start0);
            if (agrees(d, n, t, cur[t], prev, n_ref)) {
                nxt[t] = cur[t];
                continue;
            }
            if (cur[t].spec && cur[t].entry != NONE)
                ++false_starts;
            const bool s = !sel.flags_only();
            const uint64_t e = named     ? fix_tile<FORM_NAMED, true>(d, n, t, prev, t == first_bad, n_ref, excl, nxt[t], eff(), mate_suffix)
                               : qual && s ? fix_tile<true, true>(d, n, t, prev, t == first_bad, n_ref, excl, nxt[t], eff())
                               : s       ? fix_tile<false, true>(d, n, t, prev, t == first_bad, n_ref, excl, nxt[t], eff())
                               : qual    ? fix_tile<true>(d, n, t, prev, t == first_bad, n_ref, excl, nxt[t])
                                         : fix_tile(d, n, t, prev, t == first_bad, n_ref, excl, nxt[t]);
            if (e != NONE && (err_pos == NONE || e < err_pos))
                err_pos = e;
        }
        cur.swap(nxt);
        return 0;
    }
    int totals(uint64_t n_tiles, uint64_t start0, Totals &o)
    {
        o.recs = o.excluded = o.out_bytes = 0;
        base.assign(n_tiles, 0);
        for (uint64_t t = 0; t < n_tiles; ++t) {
            base[t] = o.out_bytes;
            o.recs += cur[t].recs;
            o.excluded += cur[t].excluded;
            o.out_bytes += cur[t].bytes;
        }
        o.exit = prev_exit(cur.data(), n_tiles, start0);
        return 0;
    }
    void decode(uint8_t *out)
    {
        for (uint64_t t = 0; t < cur.size(); ++t) {
            const Tile &c = cur[t];
            if (c.entry == NONE || c.recs == 0)
                continue;
            uint64_t p = c.entry, o = base[t];
            while (p < c.exit) {
                RecHead h;
                if (record_at(d, n, p, n_ref, h) != REC_OK)
                    break;
                const bool rev = flipped(h, orig), keep = is_kept(p, h);
                if (keep)
                    reversed += rev ? 1u : 0u;
                if (keep && named) {
                    for (uint32_t lane = 0; lane < lanes; ++lane)
                        replaced += rev ? decode_record_named_rev(d + p, h, out + o, lane, lanes, mate_suffix)
                                        : decode_record_named(d + p, h, out + o, lane, lanes, mate_suffix);
                    o += out_len_named(h, mate_suffix);
                    no_qual += qual_absent(d + p, h) ? 1u : 0u;
                } else if (keep && qual) {
                    for (uint32_t lane = 0; lane < lanes; ++lane)
                        rev ? decode_record_q_rev(d + p, h, out + o, lane, lanes) : decode_record_q(d + p, h, out + o, lane, lanes);
                    o += 2ull * h.l_seq + 6ull;
                    no_qual += qual_absent(d + p, h) ? 1u : 0u;
                } else if (keep) {
                    for (uint32_t lane = 0; lane < lanes; ++lane)
                        rev ? decode_record_rev(d + p, h, out + o, lane, lanes) : decode_record(d + p, h, out + o, lane, lanes);
                    o += h.l_seq + 3ull;
                }
                p += 4ull + h.bs;
            }
        }
    }
    // The raw form ("record_bam"), behind totals(): the call's selected records have the entries hits / windows
    // [0, n_entries) (windows null: none kept).  raw_count(): the record base, the kept raw bytes per tile and their scan, as the
    // kernels make them; returns the call's kept bytes.  raw_copy(): the records that pass `rule` copied to queue[tail, ...) with
    // `lanes` lanes one after the other (queue: 16-byte aligned, room for tail + the counted bytes).
    std::vector<uint64_t> raw_rec_base, raw_byte_base;
    std::vector<uint32_t> raw_kept_bytes;
    uint64_t raw_count(const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const RkRule &rule, uint64_t *kept_recs)
    {
        const auto is_sel = [&](const uint8_t *rec, const RecHead &h) { return is_kept((uint64_t)(rec - d), h); };
        raw_rec_base.assign(cur.size(), 0);
        raw_byte_base.assign(cur.size(), 0);
        raw_kept_bytes.assign(cur.size(), 0);
        uint64_t recs = 0, bytes = 0, kept = 0;
        for (uint64_t t = 0; t < cur.size(); ++t) { // (a) the record base, (b) the count
            raw_rec_base[t] = recs;
            recs += cur[t].recs;
            uint32_t kr = 0;
            raw_kept_bytes[t] = raw_walk_tile(d, n, n_ref, cur[t], raw_rec_base[t], hits, windows, n_entries, rule, &kr, is_sel,
                                              [](uint64_t, uint32_t, uint32_t) {});
            kept += kr;
        }
        for (uint64_t t = 0; t < cur.size(); ++t) { // (c) the scan
            raw_byte_base[t] = bytes;
            bytes += raw_kept_bytes[t];
        }
        *kept_recs = kept;
        return bytes;
    }
    void raw_copy(const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const RkRule &rule, uint8_t *queue, uint64_t tail)
    {
        const auto is_sel = [&](const uint8_t *rec, const RecHead &h) { return is_kept((uint64_t)(rec - d), h); };
        for (uint64_t t = 0; t < cur.size(); ++t) { // (d) the copy
            uint32_t kr = 0;
            raw_walk_tile(d, n, n_ref, cur[t], raw_rec_base[t], hits, windows, n_entries, rule, &kr, is_sel,
                          [&](uint64_t p, uint32_t len, uint32_t off) {
                              if ((uint64_t)off + len > raw_kept_bytes[t]) // (the tile's share, as the kernel checks it)
                                  return;
                              for (uint32_t lane = 0; lane < lanes; ++lane)
                                  raw_copy_part(d + p, queue, raw_dest(tail, raw_byte_base[t], off), len, lane, lanes);
                          });
        }
    }
    // Mates kept together ("record_bam_mates"): the pair forms of the two steps above, over the n_entries = 2P entries of
    // the call's whole pairs (carried: a mate 1 was carried in and is entry 0).  raw_count_pairs() also reports the odd last record
    // (*odd_pos NONE: there is none).  raw_pair_names(): the lowest pair ordinal of the call whose two records are no mates (NONE:
    // all are), over the records in front of `consumed`.  raw_carry_copy(): the carried mate 1 to queue[tail, tail + len).
    std::vector<uint64_t> raw_pos; // the start of the selected record of every entry (NONE: the carried one's, or none left)
    uint64_t raw_count_pairs(const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const RkPairRule &rule, uint32_t carried,
                             uint64_t *kept_recs, uint64_t *odd_pos, uint32_t *odd_len)
    {
        raw_pos.assign(n_entries, NONE);
        const auto is_sel = [&](const uint8_t *rec, const RecHead &h) { return is_kept((uint64_t)(rec - d), h); };
        raw_rec_base.assign(cur.size(), 0);
        raw_byte_base.assign(cur.size(), 0);
        raw_kept_bytes.assign(cur.size(), 0);
        uint64_t recs = 0, bytes = 0, kept = 0;
        *odd_pos = NONE;
        *odd_len = 0;
        for (uint64_t t = 0; t < cur.size(); ++t) {
            raw_rec_base[t] = recs;
            recs += cur[t].recs;
            uint32_t kr = 0;
            raw_kept_bytes[t] = raw_walk_tile_pairs(d, n, n_ref, cur[t], carried + raw_rec_base[t], hits, windows, n_entries, rule, &kr, is_sel,
                                                    [&](uint64_t e, uint64_t p) { raw_pos[e] = p; },
                                                    [](uint64_t, uint32_t, uint32_t) {},
                                                    [&](uint64_t p, uint32_t len) {
                                                        *odd_pos = p;
                                                        *odd_len = len;
                                                    });
            kept += kr;
        }
        for (uint64_t t = 0; t < cur.size(); ++t) {
            raw_byte_base[t] = bytes;
            bytes += raw_kept_bytes[t];
        }
        *kept_recs = kept;
        return bytes;
    }
    void raw_copy_pairs(const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const RkPairRule &rule, uint32_t carried,
                        uint8_t *queue, uint64_t tail)
    {
        const auto is_sel = [&](const uint8_t *rec, const RecHead &h) { return is_kept((uint64_t)(rec - d), h); };
        for (uint64_t t = 0; t < cur.size(); ++t) {
            uint32_t kr = 0;
            raw_walk_tile_pairs(d, n, n_ref, cur[t], carried + raw_rec_base[t], hits, windows, n_entries, rule, &kr, is_sel,
                                [](uint64_t, uint64_t) {},
                                [&](uint64_t p, uint32_t len, uint32_t off) {
                                    if ((uint64_t)off + len > raw_kept_bytes[t])
                                        return;
                                    for (uint32_t lane = 0; lane < lanes; ++lane)
                                        raw_copy_part(d + p, queue, raw_dest(tail, raw_byte_base[t], off), len, lane, lanes);
                                },
                                [](uint64_t, uint32_t) {});
        }
    }
    uint64_t raw_pair_names(uint64_t consumed, uint64_t n_entries, uint32_t carried, const uint8_t *carry, uint32_t carry_len)
    {
        for (uint64_t pr = 0; 2 * pr + 1 < n_entries && 2 * pr + 1 < raw_pos.size(); ++pr)
            if (raw_names_pair(d, consumed, raw_pos[2 * pr], raw_pos[2 * pr + 1], carried && pr == 0, carry, carry_len,
                               [&](const uint8_t *na, const uint8_t *nb, uint32_t l) {
                                   bool diff = false;
                                   for (uint32_t lane = 0; lane < lanes; ++lane)
                                       diff |= names_differ_part(na, nb, l, lane, lanes);
                                   return diff;
                               }))
                return pr;
        return NONE;
    }
    void raw_carry_copy(const uint8_t *carry, uint32_t len, uint8_t *queue, uint64_t tail) const
    {
        for (uint32_t lane = 0; lane < lanes; ++lane)
            raw_copy_part(carry, queue, tail, len, lane, lanes);
    }
};

#if defined(__HIPCC__)
// spec: one wavefront per tile (grid-stride); lanes test 64 consecutive positions, the lowest plausible one is the start;
// lane 0 walks the chain from it.
template <int Q, bool S = false>
__device__ __forceinline__ void bam_spec_tiles(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                               int32_t n_ref, uint32_t excl, Tile *__restrict__ out, const Sel &sel = Sel(),
                                               bool sfx = false)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        uint64_t entry = NONE;
        if (t == 0)
            entry = start0;
        else
            for (uint64_t c0 = t * TILE, e = tile_end(t, n); c0 < e && entry == NONE; c0 += 64u) {
                const uint64_t c = c0 + lane;
                const unsigned long long m = __ballot(c < e && plausible(d, n, c, n_ref));
                if (m)
                    entry = c0 + (uint64_t)(__ffsll((long long)m) - 1);
            }
        if (lane == 0) {
            Walk w;
            if (entry != NONE)
                walk<Q, S>(d, n, entry, tile_end(t, n), n_ref, excl, w, sel, sfx);
            const bool none = entry == NONE, bad = !none && w.bad;
            out[t].entry = bad ? INVALID : entry;
            out[t].exit = none ? NONE : bad ? INVALID : w.exit;
            out[t].recs = none ? 0u : w.recs;
            out[t].excluded = none ? 0u : w.excluded;
            out[t].bytes = none ? 0u : w.bytes;
            out[t].spec = 1u;
        }
    }
}

__global__ void __launch_bounds__(256) k_bam_spec(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                  int32_t n_ref, uint32_t excl, Tile *__restrict__ out)
{
    bam_spec_tiles<false>(d, n, n_tiles, start0, n_ref, excl, out);
}
__global__ void __launch_bounds__(256) k_bam_spec_q(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                    int32_t n_ref, uint32_t excl, Tile *__restrict__ out)
{
    bam_spec_tiles<true>(d, n, n_tiles, start0, n_ref, excl, out);
}
// spec with a selection set: the walking lane asks kept<true> — rules 1 to 3 from the record's head; a record that
// starts outside every region has its CIGAR read by that one lane.  Kernels of their own: the two above run without a selection.
__global__ void __launch_bounds__(256) k_bam_spec_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                      int32_t n_ref, Sel sel, Tile *__restrict__ out)
{
    bam_spec_tiles<false, true>(d, n, n_tiles, start0, n_ref, sel.excl, out, sel);
}
__global__ void __launch_bounds__(256) k_bam_spec_q_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                        int32_t n_ref, Sel sel, Tile *__restrict__ out)
{
    bam_spec_tiles<true, true>(d, n, n_tiles, start0, n_ref, sel.excl, out, sel);
}

// spec, the named form ("record_names"): ONE kernel for every selection — kept<true> with no selection set is the
// exclude mask — with the mate-suffix switch as a wave-uniform argument (it changes a record's output length by 0 or 2).
__global__ void __launch_bounds__(256) k_bam_spec_named(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                        int32_t n_ref, Sel sel, uint32_t sfx, Tile *__restrict__ out)
{
    bam_spec_tiles<FORM_NAMED, true>(d, n, n_tiles, start0, n_ref, sel.excl, out, sel, sfx != 0u);
}

// check: one lane per tile; bad[t] = its claim disagrees with the exit before it
__global__ void __launch_bounds__(256) k_bam_check(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                   int32_t n_ref, const Tile *__restrict__ in, uint8_t *__restrict__ bad,
                                                   Ctl *__restrict__ ctl)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tiles; t += (uint64_t)gridDim.x * blockDim.x) {
        const bool b = !agrees(d, n, t, in[t], prev_exit(in, t, start0), n_ref);
        bad[t] = b ? 1 : 0;
        if (b) {
            atomicAdd(&ctl->n_bad, 1ull);
            atomicMin(&ctl->first_bad, (unsigned long long)t);
        }
    }
}

// fix: one lane per tile; claims that agree are copied, the others walked again from the exit before them
template <int Q, bool S = false>
__device__ __forceinline__ void bam_fix_tiles(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                              int32_t n_ref, uint32_t excl, const Tile *__restrict__ in, const uint8_t *__restrict__ bad,
                                              Tile *__restrict__ out, Ctl *__restrict__ ctl, const Sel &sel = Sel(), bool sfx = false)
{
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_tiles; t += (uint64_t)gridDim.x * blockDim.x) {
        const Tile c = in[t];
        if (!bad[t]) {
            out[t] = c;
            continue;
        }
        if (c.spec && c.entry != NONE)
            atomicAdd(&ctl->false_starts, 1ull);
        Tile o;
        const uint64_t e = fix_tile<Q, S>(d, n, t, prev_exit(in, t, start0), t == ctl->first_bad, n_ref, excl, o, sel, sfx);
        out[t] = o;
        if (e != NONE)
            atomicMin(&ctl->err_pos, (unsigned long long)e);
    }
}

__global__ void __launch_bounds__(256) k_bam_fix(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                 int32_t n_ref, uint32_t excl, const Tile *__restrict__ in, const uint8_t *__restrict__ bad,
                                                 Tile *__restrict__ out, Ctl *__restrict__ ctl)
{
    bam_fix_tiles<false>(d, n, n_tiles, start0, n_ref, excl, in, bad, out, ctl);
}
__global__ void __launch_bounds__(256) k_bam_fix_q(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                   int32_t n_ref, uint32_t excl, const Tile *__restrict__ in,
                                                   const uint8_t *__restrict__ bad, Tile *__restrict__ out, Ctl *__restrict__ ctl)
{
    bam_fix_tiles<true>(d, n, n_tiles, start0, n_ref, excl, in, bad, out, ctl);
}
__global__ void __launch_bounds__(256) k_bam_fix_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                     int32_t n_ref, Sel sel, const Tile *__restrict__ in, const uint8_t *__restrict__ bad,
                                                     Tile *__restrict__ out, Ctl *__restrict__ ctl)
{
    bam_fix_tiles<false, true>(d, n, n_tiles, start0, n_ref, sel.excl, in, bad, out, ctl, sel);
}
__global__ void __launch_bounds__(256) k_bam_fix_q_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                       int32_t n_ref, Sel sel, const Tile *__restrict__ in,
                                                       const uint8_t *__restrict__ bad, Tile *__restrict__ out, Ctl *__restrict__ ctl)
{
    bam_fix_tiles<true, true>(d, n, n_tiles, start0, n_ref, sel.excl, in, bad, out, ctl, sel);
}

__global__ void __launch_bounds__(256) k_bam_fix_named(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, uint64_t start0,
                                                       int32_t n_ref, Sel sel, uint32_t sfx, const Tile *__restrict__ in,
                                                       const uint8_t *__restrict__ bad, Tile *__restrict__ out, Ctl *__restrict__ ctl)
{
    bam_fix_tiles<FORM_NAMED, true>(d, n, n_tiles, start0, n_ref, sel.excl, in, bad, out, ctl, sel, sfx != 0u);
}

// totals: one workgroup of 1024 threads, each over a run of consecutive tiles: the exclusive scan of the tiles' output bytes
// (base), the sums, the exit of the last tile
__global__ void __launch_bounds__(1024) k_bam_totals(const Tile *__restrict__ in, uint64_t n_tiles, uint64_t start0,
                                                     unsigned long long *__restrict__ base, Totals *__restrict__ tot)
{
    __shared__ unsigned long long s[1024];
    const uint32_t i = threadIdx.x;
    const uint64_t per = (n_tiles + 1023) / 1024, t0 = (uint64_t)i * per < n_tiles ? (uint64_t)i * per : n_tiles,
                   t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    unsigned long long sum = 0, recs = 0, excl = 0;
    for (uint64_t t = t0; t < t1; ++t) {
        sum += in[t].bytes;
        recs += in[t].recs;
        excl += in[t].excluded;
    }
    s[i] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) { // inclusive scan (Hillis-Steele)
        const unsigned long long v = i >= off ? s[i - off] : 0ull;
        __syncthreads();
        s[i] += v;
        __syncthreads();
    }
    unsigned long long b = s[i] - sum;
    for (uint64_t t = t0; t < t1; ++t) {
        base[t] = b;
        b += in[t].bytes;
    }
    if (i == 1023)
        tot->out_bytes = s[1023];
    __syncthreads();
    s[i] = recs;
    __syncthreads();
    for (uint32_t h = 512; h > 0; h >>= 1) {
        if (i < h)
            s[i] += s[i + h];
        __syncthreads();
    }
    if (i == 0)
        tot->recs = s[0];
    __syncthreads();
    s[i] = excl;
    __syncthreads();
    for (uint32_t h = 512; h > 0; h >>= 1) {
        if (i < h)
            s[i] += s[i + h];
        __syncthreads();
    }
    if (i == 0) {
        tot->excluded = s[0];
        tot->exit = prev_exit(in, n_tiles, start0);
    }
}

// decode: one wavefront per tile (grid-stride); its records in order, 64 lanes over every kept record's bases
__global__ void __launch_bounds__(256) k_bam_decode(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                    uint32_t excl, const Tile *__restrict__ in, const unsigned long long *__restrict__ base,
                                                    uint8_t *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const Tile c = in[t];
        if (c.entry == NONE || c.recs == 0)
            continue;
        uint64_t p = c.entry, o = base[t];
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (!(h.flag & excl)) {
                decode_record(d + p, h, out + o, lane, 64u);
                o += h.l_seq + 3ull;
            }
            p += 4ull + h.bs;
        }
    }
}

// decode, the quality variant: the same walk, four-line FASTQ per kept record; the kept records whose qualities are absent are
// counted per tile and added to *no_qual (one atomic per tile that has any).
__global__ void __launch_bounds__(256) k_bam_decode_q(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                      uint32_t excl, const Tile *__restrict__ in,
                                                      const unsigned long long *__restrict__ base, uint8_t *__restrict__ out,
                                                      unsigned long long *__restrict__ no_qual)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const Tile c = in[t];
        if (c.entry == NONE || c.recs == 0)
            continue;
        uint64_t p = c.entry, o = base[t];
        uint32_t absent = 0;
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (!(h.flag & excl)) {
                decode_record_q(d + p, h, out + o, lane, 64u);
                o += 2ull * h.l_seq + 6ull;
                absent += qual_absent(d + p, h) ? 1u : 0u;
            }
            p += 4ull + h.bs;
        }
        if (lane == 0 && absent)
            atomicAdd(no_qual, (unsigned long long)absent);
    }
}

// decode with "original_strand" on: the walks of k_bam_decode (Q false) and k_bam_decode_q (Q true), with every kept record whose
// FLAG has 0x10 and that has bases written in read orientation — a wave-uniform choice per record — and counted per tile into
// *reversed (one atomic per tile that has any).  Kernels of their own: the two above are what runs while the switch is off.
template <bool Q>
__device__ __forceinline__ void bam_decode_rev_tiles(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                     uint32_t excl, const Tile *__restrict__ in, const unsigned long long *__restrict__ base,
                                                     uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual,
                                                     unsigned long long *__restrict__ reversed)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const Tile c = in[t];
        if (c.entry == NONE || c.recs == 0)
            continue;
        uint64_t p = c.entry, o = base[t];
        uint32_t absent = 0, flips = 0;
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (!(h.flag & excl)) {
                const bool rev = flipped(h, true);
                if constexpr (Q) {
                    if (rev)
                        decode_record_q_rev(d + p, h, out + o, lane, 64u);
                    else
                        decode_record_q(d + p, h, out + o, lane, 64u);
                    o += 2ull * h.l_seq + 6ull;
                    absent += qual_absent(d + p, h) ? 1u : 0u;
                } else {
                    if (rev)
                        decode_record_rev(d + p, h, out + o, lane, 64u);
                    else
                        decode_record(d + p, h, out + o, lane, 64u);
                    o += h.l_seq + 3ull;
                }
                flips += rev ? 1u : 0u;
            }
            p += 4ull + h.bs;
        }
        if (Q && lane == 0 && absent)
            atomicAdd(no_qual, (unsigned long long)absent);
        if (lane == 0 && flips)
            atomicAdd(reversed, (unsigned long long)flips);
    }
}

__global__ void __launch_bounds__(256) k_bam_decode_rev(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                        uint32_t excl, const Tile *__restrict__ in,
                                                        const unsigned long long *__restrict__ base, uint8_t *__restrict__ out,
                                                        unsigned long long *__restrict__ reversed)
{
    bam_decode_rev_tiles<false>(d, n, n_tiles, n_ref, excl, in, base, out, nullptr, reversed);
}
__global__ void __launch_bounds__(256) k_bam_decode_q_rev(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                          uint32_t excl, const Tile *__restrict__ in,
                                                          const unsigned long long *__restrict__ base, uint8_t *__restrict__ out,
                                                          unsigned long long *__restrict__ no_qual,
                                                          unsigned long long *__restrict__ reversed)
{
    bam_decode_rev_tiles<true>(d, n, n_tiles, n_ref, excl, in, base, out, no_qual, reversed);
}

// decode with a selection set: the walk of the kernels above with kept() as the whole wavefront asks it — the same
// rules 1 to 3, the same shortcut for a record that starts inside a region, and where the CIGAR decides, 64 operations per step,
// one per lane, summed over the wavefront: the very sum the walking lane of spec / fix made, so the two agree on every record.
__device__ __forceinline__ bool kept_wave(const uint8_t *rec, const RecHead &h, const Sel &s)
{
    const int r = kept_without_cigar(rec, h, s); // (wave-uniform: the record's head)
    if (r >= 0)
        return r != 0;
    uint64_t span = cigar_span_part(rec, h, threadIdx.x & 63u, 64u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)span, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(span >> 32), o);
        span += (uint64_t)hi << 32 | lo;
    }
    return kmm_sel::region_pass(s, (int32_t)rd32(rec + 4), (int32_t)rd32(rec + 8), h.flag, span);
}

// Q: four-line FASTQ (no_qual counted); R: "original_strand" (reversed counted).  Both count kept records only.
template <bool Q, bool R>
__device__ __forceinline__ void bam_decode_sel_tiles(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                     const Sel &sel, const Tile *__restrict__ in, const unsigned long long *__restrict__ base,
                                                     uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual,
                                                     unsigned long long *__restrict__ reversed)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const Tile c = in[t];
        if (c.entry == NONE || c.recs == 0)
            continue;
        uint64_t p = c.entry, o = base[t];
        const uint64_t o_end = o + c.bytes; // (the tile's share of `out`: what its walk counted)
        uint32_t absent = 0, flips = 0;
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (kept_wave(d + p, h, sel)) {
                if (o + out_len<Q>(h.l_seq) > o_end) // (cannot happen: the walk and this pass ask one predicate; bounds all the same)
                    break;
                const bool rev = flipped(h, R);
                if constexpr (Q) {
                    if (rev)
                        decode_record_q_rev(d + p, h, out + o, lane, 64u);
                    else
                        decode_record_q(d + p, h, out + o, lane, 64u);
                    absent += qual_absent(d + p, h) ? 1u : 0u;
                } else {
                    if (rev)
                        decode_record_rev(d + p, h, out + o, lane, 64u);
                    else
                        decode_record(d + p, h, out + o, lane, 64u);
                }
                o += out_len<Q>(h.l_seq);
                flips += rev ? 1u : 0u;
            }
            p += 4ull + h.bs;
        }
        if (Q && lane == 0 && absent)
            atomicAdd(no_qual, (unsigned long long)absent);
        if (R && lane == 0 && flips)
            atomicAdd(reversed, (unsigned long long)flips);
    }
}

__global__ void __launch_bounds__(256) k_bam_decode_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref, Sel sel,
                                                        const Tile *__restrict__ in, const unsigned long long *__restrict__ base,
                                                        uint8_t *__restrict__ out)
{
    bam_decode_sel_tiles<false, false>(d, n, n_tiles, n_ref, sel, in, base, out, nullptr, nullptr);
}
__global__ void __launch_bounds__(256) k_bam_decode_q_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                          Sel sel, const Tile *__restrict__ in, const unsigned long long *__restrict__ base,
                                                          uint8_t *__restrict__ out, unsigned long long *__restrict__ no_qual)
{
    bam_decode_sel_tiles<true, false>(d, n, n_tiles, n_ref, sel, in, base, out, no_qual, nullptr);
}
__global__ void __launch_bounds__(256) k_bam_decode_rev_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                            Sel sel, const Tile *__restrict__ in,
                                                            const unsigned long long *__restrict__ base, uint8_t *__restrict__ out,
                                                            unsigned long long *__restrict__ reversed)
{
    bam_decode_sel_tiles<false, true>(d, n, n_tiles, n_ref, sel, in, base, out, nullptr, reversed);
}
__global__ void __launch_bounds__(256) k_bam_decode_q_rev_sel(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                              Sel sel, const Tile *__restrict__ in,
                                                              const unsigned long long *__restrict__ base, uint8_t *__restrict__ out,
                                                              unsigned long long *__restrict__ no_qual,
                                                              unsigned long long *__restrict__ reversed)
{
    bam_decode_sel_tiles<true, true>(d, n, n_tiles, n_ref, sel, in, base, out, no_qual, reversed);
}

// decode, the named form ("record_names"): the walk of bam_decode_sel_tiles — kept_wave is the predicate of
// k_bam_spec_named / k_bam_fix_named — with the strand switch (orig) and the mate suffix (sfx) as wave-uniform arguments: one
// kernel for every combination.  64 lanes over a kept record's name bytes, then over its bases; byte stores into disjoint
// ranges.  Per tile: the kept records without qualities, the flipped ones and the replaced name bytes (the lanes' shares summed
// over the wavefront), each added with one atomic per tile that has any.
// exempt (null: none): a bitset over the bytes of the text that `out` is part of, out[0] at its byte exempt_base,
// zeroed by the caller — the bit of a kept record's first quality byte is set when the record stores no qualities: its '"'
// letters are below every floor of 2 or more, and the mark pass of the record-hits mode lets such a record pass unmasked.
__global__ void __launch_bounds__(256) k_bam_decode_named(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref, Sel sel,
                                                          uint32_t orig, uint32_t sfx, const Tile *__restrict__ in,
                                                          const unsigned long long *__restrict__ base, uint8_t *__restrict__ out,
                                                          unsigned long long *__restrict__ no_qual, unsigned long long *__restrict__ reversed,
                                                          unsigned long long *__restrict__ replaced, uint32_t *__restrict__ exempt,
                                                          uint64_t exempt_base)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const Tile c = in[t];
        if (c.entry == NONE || c.recs == 0)
            continue;
        uint64_t p = c.entry, o = base[t];
        const uint64_t o_end = o + c.bytes; // (the tile's share of `out`: what its walk counted)
        uint32_t absent = 0, flips = 0, repl = 0;
        while (p < c.exit) {
            RecHead h;
            if (record_at(d, n, p, n_ref, h) != REC_OK) // (cannot happen on a verified chain; bounds all the same)
                break;
            if (kept_wave(d + p, h, sel)) {
                const uint32_t len = out_len_named(h, sfx != 0u);
                if (o + len > o_end) // (cannot happen: the walk and this pass ask one predicate; bounds all the same)
                    break;
                const bool rev = flipped(h, orig != 0u);
                repl += rev ? decode_record_named_rev(d + p, h, out + o, lane, 64u, sfx != 0u)
                            : decode_record_named(d + p, h, out + o, lane, 64u, sfx != 0u);
                if (exempt && lane == 0 && qual_absent(d + p, h)) { // (the quality line: the record's last l_seq bytes and a '\n')
                    const uint64_t q = exempt_base + o + len - 1u - h.l_seq;
                    atomicOr(&exempt[q >> 5], 1u << (q & 31u));
                }
                o += len;
                absent += qual_absent(d + p, h) ? 1u : 0u;
                flips += rev ? 1u : 0u;
            }
            p += 4ull + h.bs;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1)
            repl += (uint32_t)__shfl_xor((int)repl, s);
        if (lane == 0 && absent)
            atomicAdd(no_qual, (unsigned long long)absent);
        if (lane == 0 && flips)
            atomicAdd(reversed, (unsigned long long)flips);
        if (lane == 0 && repl)
            atomicAdd(replaced, (unsigned long long)repl);
    }
}

// ---- the raw form ("record_bam"): the kept records' own bytes into the keep queue, behind the inner records call.
// scan: one workgroup of 1024 threads, each over a run of consecutive tiles, as k_bam_totals: base[t] = the sum of v[stride * u]
// over u < t (64-bit; base null: the total alone), *total = the sum over all tiles.  It serves Tile::recs (the record base), the
// kept bytes (the destinations) and the kept records (their total).
__global__ void __launch_bounds__(1024) k_bam_raw_scan(const uint32_t *__restrict__ v, uint32_t stride, uint64_t n_tiles,
                                                       unsigned long long *__restrict__ base, unsigned long long *__restrict__ total)
{
    __shared__ unsigned long long s[1024];
    const uint32_t i = threadIdx.x;
    const uint64_t per = (n_tiles + 1023) / 1024, t0 = (uint64_t)i * per < n_tiles ? (uint64_t)i * per : n_tiles,
                   t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    unsigned long long sum = 0;
    for (uint64_t t = t0; t < t1; ++t)
        sum += v[t * stride];
    s[i] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) { // inclusive scan (Hillis-Steele)
        const unsigned long long x = i >= off ? s[i - off] : 0ull;
        __syncthreads();
        s[i] += x;
        __syncthreads();
    }
    if (base) {
        unsigned long long b = s[i] - sum;
        for (uint64_t t = t0; t < t1; ++t) {
            base[t] = b;
            b += v[t * stride];
        }
    }
    if (i == 1023)
        *total = s[1023];
}

// count: one wavefront per tile (grid-stride) walks its records with the predicate of spec, fix and decode (S: kept_wave, the
// CIGAR walked by the whole wavefront; else the exclude mask) and looks every selected one's entry up: the tile's kept raw
// bytes and kept records.  Every lane walks the same records: the loads are one address per wavefront.
template <bool S>
__global__ void __launch_bounds__(256) k_bam_raw_count(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref, Sel sel,
                                                       const Tile *__restrict__ in, const unsigned long long *__restrict__ rec_base,
                                                       const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                                       uint64_t n_entries, RkRule rule, uint32_t *__restrict__ kept_bytes,
                                                       uint32_t *__restrict__ kept_recs)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        uint32_t recs = 0;
        const uint32_t bytes = raw_walk_tile(
            d, n, n_ref, in[t], rec_base[t], hits, windows, n_entries, rule, &recs,
            [&](const uint8_t *rec, const RecHead &h) { return S ? kept_wave(rec, h, sel) : !(h.flag & sel.excl); },
            [](uint64_t, uint32_t, uint32_t) {});
        if (lane == 0) {
            kept_bytes[t] = bytes;
            kept_recs[t] = recs;
        }
    }
}

// copy: the same walk; 64 lanes over every kept record's 4 + block_size bytes (raw_copy_part), written behind the queue's tail
// (read from the device: {bytes, records}, as k_rk_scatter reads it) at the tile's base plus the kept bytes in front inside the
// tile.  A record is copied by the wavefront that owns its start, however many tiles it spans.  A record that would pass the
// tile's share (what count found) is not written: the same predicate and the same entries make that impossible.
template <bool S>
__global__ void __launch_bounds__(256) k_bam_raw_copy(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref, Sel sel,
                                                      const Tile *__restrict__ in, const unsigned long long *__restrict__ rec_base,
                                                      const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                                      uint64_t n_entries, RkRule rule, const uint32_t *__restrict__ kept_bytes,
                                                      const unsigned long long *__restrict__ byte_base,
                                                      const unsigned long long *__restrict__ tail, uint8_t *__restrict__ queue)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    const uint64_t tail0 = tail[0];
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const uint32_t share = kept_bytes[t];
        if (share == 0)
            continue;
        const uint64_t base = byte_base[t];
        uint32_t recs = 0;
        raw_walk_tile(
            d, n, n_ref, in[t], rec_base[t], hits, windows, n_entries, rule, &recs,
            [&](const uint8_t *rec, const RecHead &h) { return S ? kept_wave(rec, h, sel) : !(h.flag & sel.excl); },
            [&](uint64_t p, uint32_t len, uint32_t off) {
                if ((uint64_t)off + len <= share)
                    raw_copy_part(d + p, queue, raw_dest(tail0, base, off), len, lane, 64u);
            });
    }
}

// advance: the queue's tail {bytes, records} moves behind the call's kept bytes and records (k_rk_advance with 64-bit totals)
__global__ void k_bam_raw_advance(unsigned long long *tail, const unsigned long long *__restrict__ total)
{
    if (threadIdx.x < 2 && blockIdx.x == 0)
        tail[threadIdx.x] += total[threadIdx.x];
}

// ---- mates kept together in the raw form ("record_bam_mates"): kernels of their own, so that the unpaired forms above
// stay as they are.  ctl: three control words of the call — [0] the lowest pair ordinal whose records are no mates, [1] and [2]
// the start and the length of the odd last record — all NONE before the launches.

// count, the pair form: as k_bam_raw_count with raw_walk_tile_pairs; the wavefront that meets the odd last record reports it.
template <bool S>
__global__ void __launch_bounds__(256) k_bam_raw_count_pairs(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref, Sel sel,
                                                             const Tile *__restrict__ in, const unsigned long long *__restrict__ rec_base,
                                                             const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                                             uint64_t n_entries, RkPairRule rule, uint32_t carried,
                                                             uint32_t *__restrict__ kept_bytes, uint32_t *__restrict__ kept_recs,
                                                             unsigned long long *__restrict__ pos, unsigned long long *__restrict__ ctl)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        uint32_t recs = 0;
        const uint32_t bytes = raw_walk_tile_pairs(
            d, n, n_ref, in[t], carried + rec_base[t], hits, windows, n_entries, rule, &recs,
            [&](const uint8_t *rec, const RecHead &h) { return S ? kept_wave(rec, h, sel) : !(h.flag & sel.excl); },
            [&](uint64_t e, uint64_t p) {
                if (lane == 0)
                    pos[e] = p;
            },
            [](uint64_t, uint32_t, uint32_t) {},
            [&](uint64_t p, uint32_t len) {
                if (lane == 0) {
                    ctl[1] = p;
                    ctl[2] = len;
                }
            });
        if (lane == 0) {
            kept_bytes[t] = bytes;
            kept_recs[t] = recs;
        }
    }
}

// names: one wavefront per pair of the call (grid-stride) — raw_names_pair over the starts that the count walk left by entry; two
// names are compared 64 bytes a round, a ballot says whether a lane found a difference.  The lowest ordinal of a pair of
// strangers goes to ctl[0].  No chain is walked here: records that are not selected between two mates cost nothing.
__global__ void __launch_bounds__(256) k_bam_raw_pair_names(const uint8_t *__restrict__ d, uint64_t consumed,
                                                            const unsigned long long *__restrict__ pos, uint64_t n_entries, uint32_t carried,
                                                            const uint8_t *__restrict__ carry, uint32_t carry_len,
                                                            unsigned long long *__restrict__ ctl)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u), n_pairs = n_entries / 2;
    for (uint64_t pr = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; pr < n_pairs; pr += waves) {
        const bool strangers = raw_names_pair(
            d, consumed, pos[2 * pr], pos[2 * pr + 1], carried && pr == 0, carry, carry_len,
            [&](const uint8_t *na, const uint8_t *nb, uint32_t l) { return __ballot(names_differ_part(na, nb, l, lane, 64u)) != 0ull; });
        if (lane == 0 && strangers)
            atomicMin(ctl, (unsigned long long)pr);
    }
}

// carry: the carried mate 1 goes to the queue's tail when its pair is kept — every thread of the grid a share of raw_copy_part.
__global__ void __launch_bounds__(256) k_bam_raw_carry(const uint8_t *__restrict__ carry, uint32_t carry_len, const uint32_t *__restrict__ hits,
                                                       const uint32_t *__restrict__ windows, uint64_t n_entries, RkPairRule rule,
                                                       const unsigned long long *__restrict__ tail, uint8_t *__restrict__ queue)
{
    if (raw_carry_shift(hits, windows, n_entries, rule, 1u, carry_len) == 0)
        return;
    raw_copy_part(carry, queue, tail[0], carry_len, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// copy, the pair form: as k_bam_raw_copy; the tiles' bytes lie behind the carried mate 1 where that one is kept.
template <bool S>
__global__ void __launch_bounds__(256) k_bam_raw_copy_pairs(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref, Sel sel,
                                                            const Tile *__restrict__ in, const unsigned long long *__restrict__ rec_base,
                                                            const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                                            uint64_t n_entries, RkPairRule rule, uint32_t carried, uint32_t carry_len,
                                                            const uint32_t *__restrict__ kept_bytes,
                                                            const unsigned long long *__restrict__ byte_base,
                                                            const unsigned long long *__restrict__ tail, uint8_t *__restrict__ queue)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    const uint64_t tail0 = tail[0] + raw_carry_shift(hits, windows, n_entries, rule, carried, carry_len);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        const uint32_t share = kept_bytes[t];
        if (share == 0)
            continue;
        const uint64_t base = byte_base[t];
        uint32_t recs = 0;
        raw_walk_tile_pairs(
            d, n, n_ref, in[t], carried + rec_base[t], hits, windows, n_entries, rule, &recs,
            [&](const uint8_t *rec, const RecHead &h) { return S ? kept_wave(rec, h, sel) : !(h.flag & sel.excl); },
            [](uint64_t, uint64_t) {},
            [&](uint64_t p, uint32_t len, uint32_t off) {
                if ((uint64_t)off + len <= share)
                    raw_copy_part(d + p, queue, raw_dest(tail0, base, off), len, lane, 64u);
            },
            [](uint64_t, uint32_t) {});
    }
}

// advance, the pair form: the tiles' totals and the carried mate 1 where it is kept
__global__ void k_bam_raw_advance_pairs(unsigned long long *tail, const unsigned long long *__restrict__ total, const uint32_t *__restrict__ hits,
                                        const uint32_t *__restrict__ windows, uint64_t n_entries, RkPairRule rule, uint32_t carried,
                                        uint32_t carry_len)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const uint64_t shift = raw_carry_shift(hits, windows, n_entries, rule, carried, carry_len);
        tail[0] += total[0] + shift;
        tail[1] += total[1] + (shift ? 1ull : 0ull);
    }
}

// resync: one wavefront per tile (grid-stride), the shape of spec; lanes test 64 consecutive positions, the survivors are
// walked to the end of the bytes in ascending order — the same walk in every lane: the position comes from a ballot, so the
// loads are one address per wavefront and nothing diverges — and the tile's lowest holding position goes to *best (a 64-bit
// minimum, NONE before the launch).  A wavefront stops where a lower position is known to hold.  No scratch: a claim is a word.
__global__ void __launch_bounds__(256) k_bam_resync(const uint8_t *__restrict__ d, uint64_t n, uint64_t n_tiles, int32_t n_ref,
                                                    uint32_t at_eof, unsigned long long *__restrict__ best)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x / 64u);
    for (uint64_t t = (uint64_t)blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; t < n_tiles; t += waves) {
        uint64_t found = NONE;
        for (uint64_t c0 = t * TILE, e = tile_end(t, n); c0 < e && found == NONE; c0 += 64u) {
            // (a lower position holds already: nothing from here on can be the minimum; the ballot keeps the wavefront together)
            if (__ballot(__hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= c0))
                break;
            const uint64_t c = c0 + lane;
            unsigned long long m = __ballot(c < e && plausible(d, n, c, n_ref));
            while (m && found == NONE) {
                const uint64_t s = c0 + (uint64_t)(__ffsll((long long)m) - 1);
                m &= m - 1;
                if (chain_holds(d, n, s, n_ref, at_eof != 0u))
                    found = s;
            }
        }
        if (found != NONE && lane == 0)
            atomicMin(best, (unsigned long long)found);
    }
}
#endif

} // namespace kmm_bam
