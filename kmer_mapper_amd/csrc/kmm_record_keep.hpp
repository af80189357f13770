// kmm_record_keep.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace.
// The record-keep mode: behind k_read_hits in records mode, the TEXT of every record whose entry passes the keep
// rule is appended to a byte queue of the handle.  The record of a byte is arithmetic on its line number (the newline census
// of the records front end), its keep flag a look at the entry k_read_hits has just written:
//   k_rk_flags     keep flags -> kept bytes and kept records per 1024-byte tile
//   (k_rec_scan1 + k_super_scan: prefix sums of the byte counts; the same pair sums the record counts)
//   k_rk_scatter   the kept bytes of four tiles, compacted in LDS, written as one contiguous span of the queue
//   k_rk_advance   the queue's tail moves behind the piece's bytes and records
// Mates kept together: k_rk_flags and k_rk_scatter are templates over PAIR — 0 is the code above, 1 and 2 ask the
// pair rule of the two entries of a record's pair — and k_rk_zip puts the entries of two buffers into the queue in pair order.
// The mates of a BAM stream: k_rk_pair_names compares the two name lines of every pair of the named decode's text.
// The arithmetic is plain C++ (KMM_RH_HD): the CPU tier compiles this header with g++.
#pragma once

#include "kmm_read_hits.hpp"

// The keep rule (include/kmm.h): hits and windows of a record's entry; windows is 0 where the mode keeps none (min_permille
// is 0 there).
struct RkRule {
    uint32_t min_hits, min_permille, invert;
};

KMM_RH_HD bool rk_keep(uint32_t hits, uint32_t windows, const RkRule &rule)
{
    const bool match = hits >= rule.min_hits && 1000ull * (uint64_t)hits >= (uint64_t)rule.min_permille * (uint64_t)windows;
    return match != (rule.invert != 0u);
}

// The pair rule: mates are kept or dropped together.  `match` of a mate is the rule above without its inversion;
// the pair matches when ANY mate does, or only when BOTH do, and the inversion is applied to the pair.
enum : uint32_t { RK_PAIR_ANY = 0u, RK_PAIR_BOTH = 1u };

struct RkPairRule {
    RkRule rule;
    uint32_t pair_rule;
};

KMM_RH_HD bool rk_match(uint32_t hits, uint32_t windows, const RkRule &rule)
{
    return hits >= rule.min_hits && 1000ull * (uint64_t)hits >= (uint64_t)rule.min_permille * (uint64_t)windows;
}

KMM_RH_HD bool rk_pair_keep(uint32_t h1, uint32_t w1, uint32_t h2, uint32_t w2, const RkRule &rule, uint32_t pair_rule)
{
    const bool m1 = rk_match(h1, w1, rule), m2 = rk_match(h2, w2, rule);
    const bool pair_match = pair_rule == RK_PAIR_ANY ? (m1 || m2) : (m1 && m2);
    return pair_match != (rule.invert != 0u);
}

// The pair forms of the kernels below, PAIR: 0 none (one record, one entry); 1: record r of the buffer is pair r (the two-file
// call: the buffer holds one mate of every pair); 2: records 2p and 2p + 1 are pair p (interleaved).  The entries of pair p
// are 2p and 2p + 1 in every form.
template <int PAIR> struct RkRuleOf { typedef RkPairRule type; };
template <> struct RkRuleOf<0> { typedef RkRule type; };

KMM_RH_HD uint32_t rk_pair_of_record(uint32_t record, uint32_t pair_shift)
{
    return record >> pair_shift;
}

// Keep mask of a lane's LANE bytes at piece positions p0 .. p0 + LANE - 1: bit j = byte j lies before `consumed` and belongs to
// a kept record.  line0: the line of the lane's first byte; nl: bit j = byte j is '\n' (it belongs to the line it ends).
// keep_of(record) is asked once per record the lane touches, never for a byte at or behind `consumed`.
template <int LANE, typename KeepOf>
KMM_RH_HD uint32_t rk_lane_mask(uint32_t line0, uint32_t nl, uint32_t period_shift, int64_t p0, int64_t consumed, KeepOf &&keep_of)
{
    if (p0 >= consumed)
        return 0u;
    uint32_t mask = 0, line = line0, rec = rh_record_of_line(line0, period_shift);
    bool keep = keep_of(rec);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < LANE; ++j) {
        const bool inside = p0 + j < consumed;
        const uint32_t r = rh_record_of_line(line, period_shift);
        if (inside && r != rec) {
            rec = r;
            keep = keep_of(rec);
        }
        mask |= (keep && inside ? 1u : 0u) << j;
        line += (nl >> j) & 1u;
    }
    return mask;
}

// Kept records that END inside the lane: kept newlines on the last line of a record.
template <int LANE>
KMM_RH_HD uint32_t rk_lane_records(uint32_t line0, uint32_t nl, uint32_t period_mask, uint32_t mask)
{
    uint32_t n = 0, ends = nl & mask;
    while (ends) {
        const int j = __builtin_ctz(ends);
        ends &= ends - 1u;
        n += (rh_line_of_byte(line0, nl, j) & period_mask) == period_mask ? 1u : 0u;
    }
    return n;
}

// Destination of a lane's first kept byte: the queue's tail, the kept bytes of the super-tiles and tiles in front (exclusive
// prefixes, 32-bit inside a piece) and of the lanes in front inside the tile.
KMM_RH_HD int64_t rk_dest(int64_t tail, uint32_t super_pre, uint32_t tile_pre, uint32_t rank)
{
    return tail + (int64_t)super_pre + (int64_t)tile_pre + (int64_t)rank;
}

// How a span of `len` bytes that starts `a` (0 .. 15) bytes behind a 16-byte line is written: bytes [a, head_end) and
// [tail_begin, a + len) one by one, [full_begin, full_end) as whole 16-byte lines.  Nothing outside [a, a + len) is named.
struct RkSpan {
    uint32_t head_end, full_begin, full_end, tail_begin;
};

KMM_RH_HD RkSpan rk_span(uint32_t a, uint32_t len)
{
    RkSpan s;
    const uint32_t hi = a + len;
    s.full_begin = (a + 15u) & ~15u;
    s.full_end = hi & ~15u;
    s.head_end = s.full_begin < hi ? s.full_begin : hi;
    s.tail_begin = s.full_end > s.head_end ? s.full_end : s.head_end;
    if (s.full_end < s.full_begin)
        s.full_end = s.full_begin; // (a span inside one line: no whole line)
    return s;
}

// The mate check: the two name lines of a pair of the named BAM decode's text, lines 8p and 8p + 4.
// A name is what stands behind '@'; with the mate suffix on, a trailing "/1" or "/2" is left out of the comparison (so is one
// that the QNAME itself ends in while FLAG carries no mate bit: include/kmm.h).
KMM_RH_HD uint32_t rk_name_trim(const uint8_t *name, uint32_t len, bool mate_suffix)
{
    if (mate_suffix && len >= 2u && name[len - 2u] == (uint8_t)'/' && (name[len - 1u] == (uint8_t)'1' || name[len - 1u] == (uint8_t)'2'))
        return len - 2u;
    return len;
}

// Equal: equal length and equal bytes, behind the trim.
KMM_RH_HD bool rk_names_equal(const uint8_t *a, uint32_t len_a, const uint8_t *b, uint32_t len_b, bool mate_suffix)
{
    const uint32_t la = rk_name_trim(a, len_a, mate_suffix), lb = rk_name_trim(b, len_b, mate_suffix);
    if (la != lb)
        return false;
    for (uint32_t i = 0; i < la; ++i)
        if (a[i] != b[i])
            return false;
    return true;
}

// Where mate 2's name line starts, from mate 1's alone: at: its '@'; name_end, seq_end: the newlines that end its name line and
// its SEQ line.  The decode writes SEQ and QUAL of one length, so no newline behind seq_end has to be looked for:
// '@' name '\n' | SEQ '\n' | "+\n" | QUAL '\n' | '@' of mate 2.
KMM_RH_HD int64_t rk_mate2_line(int64_t at, int64_t name_end, int64_t seq_end)
{
    const int64_t name = name_end - at, l_seq = seq_end - name_end - 1;
    return at + name + 1 + 2 * (l_seq + 1) + 2;
}

#if defined(__HIPCC__)

typedef uint32_t u32x2 __attribute__((ext_vector_type(2))); // (the two entries of a pair: one 8-byte load)

// What both per-byte kernels know of a lane: its 16 bytes, their newlines, its keep mask and the line of its first byte.
struct RkLane {
    uint32_t w[4];
    uint32_t nl, mask, line0;
};

// One wavefront per tile; called with all 64 lanes active (a tile behind the piece: no bytes, no mask).  hits / windows: the
// piece's entries (n_records of them), complete; windows null: mode 1.
// PAIR != 0: hits / windows are the entries of the piece's pairs, two per pair, 8-byte aligned; n_records counts the records of
// `raw` (PAIR 1: as many as pairs; PAIR 2: twice as many).
template <int PAIR>
__device__ __forceinline__ void rk_lane_front(const uint8_t *__restrict__ raw, int64_t n, int64_t consumed, int64_t n_tiles, int64_t tile,
                                              int lane, const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ super_nl,
                                              uint32_t period_mask, const uint32_t *__restrict__ hits, const uint32_t *__restrict__ windows,
                                              int64_t n_records, const typename RkRuleOf<PAIR>::type &rule, RkLane &L)
{
    const int64_t p = tile * 1024 + lane * 16;
    L.w[0] = L.w[1] = L.w[2] = L.w[3] = 0u;
    if (tile < n_tiles && p + 16 <= n) {
        u32x4 x; // (a piece starts at any byte offset: one 16-byte load, aligned or not, as rec_load16)
        __builtin_memcpy(&x, raw + p, 16);
        L.w[0] = x[0]; L.w[1] = x[1]; L.w[2] = x[2]; L.w[3] = x[3];
    } else if (tile < n_tiles) {
#pragma unroll
        for (int j = 0; j < 16; ++j) // (the piece's last bytes; what lies behind them reads as zero)
            if (p + j < n)
                L.w[j >> 2] |= (uint32_t)raw[p + j] << (8 * (j & 3));
    }
    uint32_t cr;
    rec_masks(L.w, L.nl, cr);
    const uint32_t cnt = (uint32_t)__popc(L.nl);
    const uint32_t incl = wave_scan_incl(cnt);
    uint32_t base = 0;
    if (tile < n_tiles)
        base = super_nl[tile >> 10] + tile_nl[tile];
    L.line0 = base + incl - cnt;
    const int64_t end = tile < n_tiles ? consumed : 0;
    L.mask = rk_lane_mask<16>(L.line0, L.nl, (uint32_t)__popc(period_mask), p, end, [&](uint32_t r) {
        if ((int64_t)r >= n_records)
            return false;
        if constexpr (PAIR == 0) {
            return rk_keep(hits[r], windows ? windows[r] : 0u, rule);
        } else {
            const size_t e = 2 * (size_t)rk_pair_of_record(r, (uint32_t)(PAIR - 1)); // (both entries exist: n_records is whole pairs)
            const u32x2 h = *reinterpret_cast<const u32x2 *>(hits + e);
            u32x2 w = {0u, 0u};
            if (windows)
                w = *reinterpret_cast<const u32x2 *>(windows + e);
            return rk_pair_keep(h[0], w[0], h[1], w[1], rule.rule, rule.pair_rule);
        }
    });
}

// (The record counts go through an array and the scans, not through an atomic on the tail: one atomic per tile on one address
// added 3.9 ms to a chunk of 300 000 tiles, eight times what the whole mode costs now: profiles/record_keep/README.md.)
template <int PAIR>
__global__ void __launch_bounds__(256) k_rk_flags(const uint8_t *__restrict__ raw, int64_t n, int64_t consumed, int64_t n_tiles,
                                                  const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ super_nl,
                                                  uint32_t period_mask, const uint32_t *__restrict__ hits,
                                                  const uint32_t *__restrict__ windows, int64_t n_records, typename RkRuleOf<PAIR>::type rule,
                                                  uint32_t *__restrict__ tile_cnt, uint32_t *__restrict__ tile_rec)
{
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles)
        return;
    RkLane L;
    rk_lane_front<PAIR>(raw, n, consumed, n_tiles, tile, lane, tile_nl, super_nl, period_mask, hits, windows, n_records, rule, L);
    const uint32_t kept = wave_sum((uint32_t)__popc(L.mask));
    const uint32_t recs = wave_sum(rk_lane_records<16>(L.line0, L.nl, period_mask, L.mask));
    if (lane == 0) {
        tile_cnt[tile] = kept;
        tile_rec[tile] = recs;
    }
}

// One workgroup per four tiles (one super-tile holds 256 such groups: a group never straddles two).  The kept bytes of the four
// tiles go to LDS in order, shifted so that LDS byte i and queue byte (dst - a + i) share their place inside a 16-byte line;
// the span [a, a + len) then leaves as whole 16-byte lines, its ragged head and tail byte by byte.  The neighbouring groups
// write the other bytes of the first and the last line: no byte outside the span is written, none of the queue is read.
template <int PAIR>
__global__ void __launch_bounds__(256) k_rk_scatter(const uint8_t *__restrict__ raw, int64_t n, int64_t consumed, int64_t n_tiles,
                                                    const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ super_nl,
                                                    uint32_t period_mask, const uint32_t *__restrict__ hits,
                                                    const uint32_t *__restrict__ windows, int64_t n_records, typename RkRuleOf<PAIR>::type rule,
                                                    const uint32_t *__restrict__ tile_pre, const uint32_t *__restrict__ super_pre,
                                                    const unsigned long long *__restrict__ tail, uint8_t *__restrict__ queue)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_buf[4096 + 16];
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t tile0 = (int64_t)blockIdx.x * 4, tile = tile0 + wave;
    RkLane L;
    rk_lane_front<PAIR>(raw, n, consumed, n_tiles, tile, lane, tile_nl, super_nl, period_mask, hits, windows, n_records, rule, L);
    const uint32_t kept = (uint32_t)__popc(L.mask);
    const uint32_t incl = wave_scan_incl(kept);
    if (lane == 63)
        s_cnt[wave] = incl;
    __syncthreads();
    uint32_t before = 0, len = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = s_cnt[i];
        before += i < wave ? c : 0u;
        len += c;
    }
    if (len == 0) // (the same for the whole group)
        return;
    const int64_t dst = rk_dest((int64_t)tail[0], super_pre[tile0 >> 10], tile_pre[tile0], 0u);
    const uint32_t a = (uint32_t)dst & 15u;
    uint32_t o = a + before + (incl - kept);
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if ((L.mask >> j) & 1u)
            s_buf[o++] = (uint8_t)(L.w[j >> 2] >> (8 * (j & 3)));
    __syncthreads();
    uint8_t *g = queue + (dst - (int64_t)a); // (the 16-byte line the span starts in)
    const RkSpan sp = rk_span(a, len);
    const uint32_t t = threadIdx.x;
    if (a + t < sp.head_end)
        g[a + t] = s_buf[a + t];
    for (uint32_t i = sp.full_begin + 16u * t; i + 16u <= sp.full_end; i += 16u * 256u)
        *reinterpret_cast<u32x4 *>(g + i) = *reinterpret_cast<const u32x4 *>(s_buf + i);
    if (sp.tail_begin + t < a + len)
        g[sp.tail_begin + t] = s_buf[sp.tail_begin + t];
}

// tail: {bytes, records} of the queue; total: {kept bytes, kept records} of the piece.
__global__ void k_rk_advance(unsigned long long *tail, const uint32_t *__restrict__ total)
{
    if (threadIdx.x < 2 && blockIdx.x == 0)
        tail[threadIdx.x] += (unsigned long long)total[threadIdx.x];
}

// The entries of the two buffers of kmm_map_record_pairs (m each, in record order) in pair order: out[2i] = mate1[i],
// out[2i + 1] = mate2[i], as the interleaved file would have appended them.  out is 8-byte aligned.
__global__ void __launch_bounds__(256) k_rk_zip(const uint32_t *__restrict__ mate1, const uint32_t *__restrict__ mate2, int64_t m,
                                                uint32_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        u32x2 e;
        e[0] = mate1[i];
        e[1] = mate2[i];
        *reinterpret_cast<u32x2 *>(out + 2 * i) = e;
    }
}

// ---- the mate check: are records 2p and 2p + 1 of the named BAM decode's text mates — do their names agree?
// A lane's 16 bytes at piece position p; what lies at or behind `limit` reads as zero (and is not read).
__device__ __forceinline__ void rk_load16(const uint8_t *__restrict__ raw, int64_t p, int64_t limit, uint32_t (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (p + 16 <= limit) {
        u32x4 x;
        __builtin_memcpy(&x, raw + p, 16);
        w[0] = x[0]; w[1] = x[1]; w[2] = x[2]; w[3] = x[3];
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if (p + j < limit)
                w[j >> 2] |= (uint32_t)raw[p + j] << (8 * (j & 3));
    }
}

// The whole wavefront looks for the first `want` (1 or 2) newlines at or behind `from` and before `limit`, 1024 bytes a round:
// e[t] is newline t's position in every lane, -1 where the bytes end first.  from, limit and want are the same in all lanes.
__device__ __forceinline__ void rk_wave_newlines(const uint8_t *__restrict__ raw, int64_t from, int64_t limit, int lane, uint32_t want,
                                                 int64_t (&e)[2])
{
    e[0] = e[1] = -1;
    uint32_t seen = 0;
    for (int64_t base = from; base < limit && seen < want; base += 1024) {
        uint32_t w[4], nl, cr;
        rk_load16(raw, base + lane * 16, limit, w);
        rec_masks(w, nl, cr);
        const uint32_t cnt = (uint32_t)__popc(nl), incl = wave_scan_incl(cnt), before = seen + incl - cnt;
#pragma unroll
        for (uint32_t t = 0; t < 2u; ++t) {
            const bool mine = t < want && before <= t && t < before + cnt; // (newline t of the search is one of this lane's)
            const unsigned long long who = __ballot(mine);
            if (who) {
                uint32_t m = nl;
                for (uint32_t i = before; mine && i < t; ++i)
                    m &= m - 1u;
                const int off = lane * 16 + (mine ? __builtin_ctz(m) : 0);
                e[t] = base + __shfl(off, __builtin_ctzll(who));
            }
        }
        seen += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
}

// One wavefront per 1024-byte tile of the piece's consumed bytes, as the keep kernels; tile_nl / super_nl: the newline census
// (the line of every byte).  Every '@' that starts a line 8p inside the tile is a pair's: the wavefront finds the ends of mate 1's
// name and SEQ lines, steps to mate 2's name line by arithmetic (rk_mate2_line), finds its end, and compares the names 64 bytes a
// round.  Nothing at or behind `consumed` is read: the pairs in front of it are whole.  first_bad: the piece's first pair
// (ordinal inside the piece) whose names differ — or whose text is not what the decode writes — else 0xFFFFFFFF as it was set.
__global__ void __launch_bounds__(256) k_rk_pair_names(const uint8_t *__restrict__ raw, int64_t consumed, int64_t n_tiles,
                                                       const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ super_nl,
                                                       uint32_t mate_suffix, uint32_t *__restrict__ first_bad)
{
    const int lane = threadIdx.x & 63;
    const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= n_tiles)
        return;
    const int64_t p = tile * 1024 + lane * 16;
    uint32_t w[4], nl, cr;
    rk_load16(raw, p, consumed, w);
    rec_masks(w, nl, cr);
    const uint32_t cnt = (uint32_t)__popc(nl);
    const uint32_t line0 = super_nl[tile >> 10] + tile_nl[tile] + wave_scan_incl(cnt) - cnt;
    // a line's first byte: behind a newline, or the piece's first
    uint32_t prev = (uint32_t)__shfl_up((int)(nl >> 15), 1) & 1u;
    if (lane == 0)
        prev = tile == 0 || raw[p - 1] == (uint8_t)'\n' ? 1u : 0u;
    const uint32_t starts = ((nl << 1) | prev) & 0xFFFFu;
    uint32_t first = 0; // ... of those the first bytes of the lines 8p
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (((starts >> j) & 1u) && p + j < consumed && (rh_line_of_byte(line0, nl, j) & 7u) == 0u)
            first |= 1u << j;
    for (;;) {
        const unsigned long long who = __ballot(first != 0u);
        if (!who)
            break;
        const int src = __builtin_ctzll(who);
        const int j_own = first ? __builtin_ctz(first) : 0;
        const int j = __shfl(j_own, src);
        const uint32_t pair = (uint32_t)__shfl((int)rh_line_of_byte(line0, nl, j_own), src) >> 3;
        if (lane == src)
            first &= first - 1u;
        const int64_t at = tile * 1024 + src * 16 + j;
        int64_t e[2], f[2];
        rk_wave_newlines(raw, at, consumed, lane, 2u, e);
        bool bad = raw[at] != (uint8_t)'@' || e[1] < 0;
        int64_t at2 = 0;
        if (!bad) {
            at2 = rk_mate2_line(at, e[0], e[1]);
            bad = at2 >= consumed || raw[at2 - 1] != (uint8_t)'\n' || raw[at2] != (uint8_t)'@';
        }
        if (!bad) {
            rk_wave_newlines(raw, at2, consumed, lane, 1u, f);
            bad = f[0] < 0;
        }
        if (!bad) {
            const uint8_t *a = raw + at + 1, *b = raw + at2 + 1;
            const uint32_t la = rk_name_trim(a, (uint32_t)(e[0] - at - 1), mate_suffix != 0u);
            const uint32_t lb = rk_name_trim(b, (uint32_t)(f[0] - at2 - 1), mate_suffix != 0u);
            bool differ = la != lb;
            for (uint32_t i = (uint32_t)lane; !differ && i < la; i += 64u)
                differ = a[i] != b[i];
            bad = __ballot(differ) != 0ull;
        }
        if (bad && lane == 0)
            atomicMin(first_bad, pair);
    }
}

#endif // __HIPCC__
