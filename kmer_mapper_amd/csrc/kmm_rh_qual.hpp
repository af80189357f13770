// kmm_rh_qual.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace.
// The base-quality floor of the record-hits mode: a mark pass over a piece of raw FASTQ text, in front of
// k_read_hits, that fills a bitset in RAW space — bit p: the sequence byte at offset p of the piece has a quality byte below
// the floor — which the quality variants of the records front end (MODE_RECORDS_QUAL, MODE_RECORDS_BRK_QUAL, kmm_tile.hpp) AND
// into their sequence bytes.  The text itself is never touched: the keep kernels read the bytes they read without a floor.
// The arithmetic of a lane is plain C++ (KMM_RH_HD, kmm_read_hits.hpp): the CPU tier compiles this header with g++.
#pragma once

#include "kmm_read_hits.hpp"

// Quality lines are the fourth lines of their records (line numbers count the newlines in front of a byte).
KMM_RH_HD bool rq_is_qual_line(uint32_t line)
{
    return (line & 3u) == 3u;
}

// The lane's bytes [a, n_in) start on one line: the first byte behind that line's share of the lane — the position of its
// '\n' when the lane holds it (nl: bit i = byte i is '\n', no bit at or behind n_in), else n_in.
KMM_RH_HD uint32_t rq_seg_end(uint32_t nl, uint32_t a, uint32_t n_in)
{
    const uint32_t m = nl >> a;
    return m ? a + (uint32_t)__builtin_ctz(m) : n_in;
}

// The bytes of a line in front of its '\n', without the '\r' of a CRLF end: what the length rule compares.
KMM_RH_HD uint32_t rq_line_len(uint32_t start, uint32_t nl_pos, bool cr_before_nl)
{
    const uint32_t len = nl_pos - start;
    return len > 0 && cr_before_nl ? len - 1u : len;
}

// Up to 16 flags of quality bytes (bit i: the byte at offset o + i of its quality line is low) as words of the bitset: byte
// o + i of the quality line belongs to byte o + i of the sequence line, which starts at s_start and whose '\n' is at s_nl —
// a flag at or behind that '\n' marks no base (the record fails the length rule).
struct RqMark {
    uint32_t word, w0, w1;
};

KMM_RH_HD RqMark rq_mark(uint32_t bits, uint32_t o, uint32_t s_start, uint32_t s_nl)
{
    const uint32_t target = s_start + o;
    const uint32_t room = s_nl > target ? s_nl - target : 0u;
    if (room < 16u)
        bits &= (1u << room) - 1u;
    const uint64_t v = (uint64_t)bits << (target & 31u);
    RqMark m;
    m.word = target >> 5;
    m.w0 = (uint32_t)v;
    m.w1 = (uint32_t)(v >> 32);
    return m;
}

// Is the record whose quality line starts at text offset q exempt (a BAM record that stores no qualities, named form)?
KMM_RH_HD bool rq_exempt(const uint32_t *exempt, uint64_t q)
{
    return exempt && ((exempt[q >> 5] >> (q & 31u)) & 1u);
}

// One lane of the mark pass: its n_in <= 16 bytes at offset p of the piece, in front of the piece's last complete record's
// end.  nl / cr / low: bit i = byte i is '\n' / '\r' / below the floor (taken as unsigned); line: the line of byte 0;
// line_start[L], L < n_lines: where line L starts (n_lines = 4 x the piece's records: every line the front end reads).
// The lane's share of every quality line it touches is OR-ed into the bitset as whole words — low bases come in runs — through
// or_word(word, bits); the lane that holds a quality line's '\n' checks the length rule and reports that '\n' through bad(p).
// exempt / text_base: the records that pass unmasked, by the offset of their quality line in the text the piece is cut from.
// Returns the lane's low quality bytes.  Nothing at or behind p + n_in is read, and no word behind the lane's own byte is set.
template <typename Or, typename Bad>
KMM_RH_HD uint32_t rq_lane(const uint8_t *raw, uint32_t p, uint32_t n_in, uint32_t nl, uint32_t cr, uint32_t low, uint32_t line,
                           uint32_t n_lines, const uint32_t *line_start, const uint32_t *exempt, uint64_t text_base, Or &&or_word,
                           Bad &&bad)
{
    uint32_t n_low = 0;
    const uint32_t inside = n_in >= 16u ? 0xFFFFu : (1u << n_in) - 1u;
    nl &= inside;
    low &= inside & ~(nl | cr);
    for (uint32_t a = 0; a < n_in; ++line) {
        const uint32_t e = rq_seg_end(nl, a, n_in);
        const bool ends = e < n_in; // (byte e is the line's '\n')
        if (rq_is_qual_line(line) && line < n_lines) {
            const uint32_t seg = e - a >= 16u ? 0xFFFFu : (1u << (e - a)) - 1u;
            uint32_t bits = (low >> a) & seg;
            if (bits || ends) {
                const uint32_t q_start = line_start[line], s_start = line_start[line - 2u], s_nl = line_start[line - 1u] - 1u;
                if (bits && rq_exempt(exempt, text_base + q_start))
                    bits = 0;
                if (bits) {
                    const RqMark m = rq_mark(bits, p + a - q_start, s_start, s_nl);
                    if (m.w0)
                        or_word(m.word, m.w0);
                    if (m.w1)
                        or_word(m.word + 1u, m.w1);
                    n_low += (uint32_t)__builtin_popcount(bits);
                }
                if (ends && rq_line_len(q_start, p + e, raw[p + e - 1u] == 13u) != rq_line_len(s_start, s_nl, raw[s_nl - 1u] == 13u))
                    bad(p + e);
            }
        }
        a = e + 1u;
    }
    return n_low;
}

#if defined(__HIPCC__)

// Where every line of the piece starts: line_start[0] = 0, line_start[L + 1] = the byte behind the L-th newline, written by
// the lane that holds it, for the lines in front of `limit` (the end of the piece's last complete record) — n_lines entries.
// One wavefront per 1024-byte tile of the census (tile_nl / super_nl: k_rec_count .. k_rec_scan2), 16 bytes per lane.
__global__ void __launch_bounds__(256) k_rq_line_starts(const uint8_t *__restrict__ raw, uint32_t limit, uint32_t n_tiles,
                                                        const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ super_nl,
                                                        uint32_t n_lines, uint32_t *__restrict__ line_start)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles)
        return;
    const uint32_t p = tile * 1024u + lane * 16u;
    uint32_t w[4], nl, cr;
    rec_load16(raw, limit, p, w);
    rec_masks(w, nl, cr);
    if (p + 16u > limit)
        nl &= p < limit ? (1u << (limit - p)) - 1u : 0u;
    const uint32_t c = (uint32_t)__popc(nl);
    const uint32_t line = super_nl[tile >> 10] + tile_nl[tile] + (wave_scan_incl(c) - c);
    if (p == 0 && n_lines > 0)
        line_start[0] = 0u;
    uint32_t m = nl;
    while (m) {
        const uint32_t i = (uint32_t)__builtin_ctz(m);
        m &= m - 1u;
        const uint32_t next = line + (uint32_t)__popc(nl & ((1u << i) - 1u)) + 1u;
        if (next < n_lines)
            line_start[next] = p + i + 1u;
    }
}

// The mark pass (rq_lane): the same geometry, behind k_rq_line_starts.  dead: the bitset, zeroed on the stream; thresh = 33 + Q;
// first_bad[1]: the smallest offset of a quality line's '\n' that fails the length rule (the deferred KMM_ERR_MALFORMED of the
// record calls); masked: the handle's statistics block, the low quality bytes added to one shard per tile.
__global__ void __launch_bounds__(256) k_rq_mark(const uint8_t *__restrict__ raw, uint32_t limit, uint32_t n_tiles,
                                                 const uint32_t *__restrict__ tile_nl, const uint32_t *__restrict__ super_nl,
                                                 uint32_t n_lines, const uint32_t *__restrict__ line_start, uint32_t thresh,
                                                 const uint32_t *__restrict__ exempt, uint64_t text_base, uint32_t *__restrict__ dead,
                                                 unsigned long long *__restrict__ first_bad, unsigned long long *__restrict__ masked)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (tile >= n_tiles)
        return;
    const uint32_t p = tile * 1024u + lane * 16u;
    uint32_t w[4], nl, cr, low = 0;
    rec_load16(raw, limit, p, w);
    rec_masks(w, nl, cr);
#pragma unroll
    for (int i = 0; i < 4; ++i)
        low |= flags_to_bits(bytes_below(w[i], thresh)) << (4 * i);
    const uint32_t n_in = p >= limit ? 0u : (limit - p < 16u ? limit - p : 16u);
    if (n_in < 16u)
        nl &= (1u << n_in) - 1u;
    const uint32_t c = (uint32_t)__popc(nl);
    const uint32_t line = super_nl[tile >> 10] + tile_nl[tile] + (wave_scan_incl(c) - c);
    const uint32_t n_low = rq_lane(raw, p, n_in, nl, cr, low, line, n_lines, line_start, exempt, text_base,
                                   [&](uint32_t word, uint32_t bits) { atomicOr(&dead[word], bits); },
                                   [&](uint32_t at) { atomicMin(&first_bad[1], (unsigned long long)at); });
    const uint32_t tile_low = wave_sum(n_low);
    if (lane == 0 && tile_low)
        atomicAdd(&masked[(size_t)(tile % (uint32_t)KMM_STAT_SHARDS) * KMM_STAT_STRIDE + KMM_STAT_QUAL_MASKED],
                  (unsigned long long)tile_low);
}

// bits [from, from + n_bits) of src -> bits [0, n_bits) of dst (whole words of dst are written, the bits behind n_bits as 0):
// the exemption flags of the text that a kmm_map_bam window leaves for the next one ("record_names_pairs": the waiting mate 1).
__global__ void __launch_bounds__(256) k_rq_bits_move(const uint32_t *__restrict__ src, uint64_t from, uint64_t n_bits,
                                                      uint32_t *__restrict__ dst)
{
    const uint64_t n_words = (n_bits + 31) / 32;
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_words; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = from + 32 * j;
        const uint32_t sh = (uint32_t)(b & 31u);
        uint32_t v = src[b >> 5] >> sh;
        if (sh)
            v |= src[(b >> 5) + 1] << (32u - sh);
        const uint64_t left = n_bits - 32 * j;
        dst[j] = left < 32 ? v & ((1u << left) - 1u) : v;
    }
}

#endif // __HIPCC__
