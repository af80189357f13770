// kmm_bgzf_out.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip.
// The BGZF writer: text that lies in HBM — the keep queue of the record-keep mode — leaves the device as BGZF
// members.  The input is cut every BLOCK = 0xFF00 bytes (as bgzip and gz_io.write_bgzf cut it); every piece becomes one member:
// the 18-byte header, ONE final deflate block, CRC32, ISIZE.  The block is dynamic Huffman over LZ77 tokens, or stored whenever
// the dynamic form would not be smaller than n + 5 bytes: a member is never larger than n + 31 bytes.
//
// One 256-thread workgroup per member; thread t owns the SEG = 255 bytes [255 t, 255 t + 255) (256 x 255 = BLOCK):
//   crc      every thread sums its segment (crc_register) and moves the register forward by the bytes behind it (crc_shift);
//            the exclusive-or over the workgroup is the member's register (kmm_gpu_inflate.hpp: one CRC in the library)
//   costs    byte histogram -> what a literal of every byte value costs, in quarter bits (bz_ilog2q)
//   fill     the hash table (4 bytes -> the last position seen, LDS) is filled FILL positions at a time: look the phase's
//            positions up (cand[i], HBM scratch of the workgroup), barrier, insert them with atomicMax, barrier.  A candidate
//            therefore lies in front of its phase — never behind the position — and is the same whatever order the lanes ran in
//   parse    greedy, per thread inside its segment, matches cut at the segment's end (one token more per 255 bytes, no walk over
//            the member); a candidate is verified byte by byte and taken only when the literals it replaces cost more than
//            the match (on A/C/G/T text a four-byte repeat is everywhere and dearer than four 2-bit literals); the tokens stay
//            in cand[] (cand[i]: where the match lies, cand[i + 1]: its length), the histograms of both alphabets in LDS
//   codes    leaves sorted by rank (all threads), then ONE lane per alphabet: Huffman tree from two queues, depths, the 15-bit
//            limit (overflow moved down the length counts as zlib's gen_bitlen does), canonical codes; the code lengths go out
//            through the code-length alphabet WITHOUT the run-length symbols 16-18
//   emit     bits per thread, a workgroup prefix sum, bits or-ed into the zeroed slot at the thread's bit offset
// Everything above is plain C++ under KMM_HD, written once as a sequence of phases (deflate_member); `each` of the executor
// runs a phase for the 256 threads — on the GPU the threads of the workgroup and a barrier, on the CPU a loop (the CPU tier
// compiles this header with g++).  The updates between two barriers are order-independent (max, add, or, xor), so the bytes
// are a pure function of the input: the kernel and the g++ build give identical members.
// Restated from RFC 1951 / RFC 1952 and the BGZF section of the SAM specification; no code taken.
#pragma once

#include "kmm_gpu_inflate.hpp"

namespace kmm_bz {

constexpr uint32_t BLOCK = 0xFF00u, SEG = 255u, THREADS = 256u;
constexpr uint32_t SLOT = 65312u;         // a member's slot: >= BLOCK + 31, a multiple of 32 bytes
constexpr uint32_t OVERHEAD = 31u;        // header 18 + stored block 5 + trailer 8
constexpr uint32_t HASH_BITS = 13u, TABLE = 1u << HASH_BITS;
constexpr uint32_t FILL = 512u;           // positions per fill phase (two per thread)
constexpr uint32_t CAND_STRIDE = 65536u;  // uint16 per workgroup (BLOCK and the slack a chunked read of the last positions needs)
constexpr uint32_t MIN_MATCH = 4u, MAX_MATCH = 258u, WINDOW = 32768u;
constexpr uint32_t NLIT = 286u, NDIST = 30u, NCL = 19u, EOB = 256u;
#ifndef KMM_BZ_MATCH_BITS
#define KMM_BZ_MATCH_BITS 14
#endif
constexpr uint32_t MATCH_BASE_QBITS = 4u * KMM_BZ_MATCH_BITS; // what a match is taken to cost before its extra bits: 14 bits for its two symbols

static_assert(SEG * THREADS == BLOCK, "the threads' segments tile a member");
static_assert(SLOT >= BLOCK + OVERHEAD && SLOT % 32u == 0u, "slot");
static_assert(kmm_gz::CRC_TABLE_WORDS <= (int)TABLE, "the CRC tables borrow the hash table");

#if defined(__HIP_DEVICE_COMPILE__)
#define KMM_BZ_ADD(p, v) atomicAdd((p), (v))
#define KMM_BZ_MAX(p, v) atomicMax((p), (v))
#define KMM_BZ_OR(p, v) atomicOr((p), (v))
#define KMM_BZ_XOR(p, v) atomicXor((p), (v))
#else
#define KMM_BZ_ADD(p, v) (void)(*(p) += (v))
#define KMM_BZ_MAX(p, v) (void)(*(p) = *(p) > (v) ? *(p) : (v))
#define KMM_BZ_OR(p, v) (void)(*(p) |= (v))
#define KMM_BZ_XOR(p, v) (void)(*(p) ^= (v))
#endif

// n + 31 * ceil(n / BLOCK)
KMM_HD inline int64_t bound(int64_t n)
{
    return n < 0 ? -1 : n + (int64_t)OVERHEAD * ((n + (int64_t)BLOCK - 1) / (int64_t)BLOCK);
}

KMM_HD inline int64_t member_count(int64_t n)
{
    return (n + (int64_t)BLOCK - 1) / (int64_t)BLOCK;
}

KMM_HD inline uint32_t bz_ilog2(uint32_t v) // v >= 1
{
    return 31u - (uint32_t)__builtin_clz(v);
}

// 4 log2(v), v >= 1: the exponent and the two bits behind the leading one
KMM_HD inline uint32_t bz_ilog2q(uint32_t v)
{
    const uint32_t e = bz_ilog2(v);
    const uint32_t f = e >= 2u ? (v >> (e - 2u)) & 3u : (v << (2u - e)) & 3u;
    return 4u * e + f;
}

// length 3 .. 258 -> symbol 257 .. 285, its extra bits and their value
KMM_HD inline void len_code(uint32_t len, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    const uint32_t l = len - 3u;
    if (len == 258u) {
        sym = 285u; eb = 0u; ev = 0u;
    } else if (l < 8u) {
        sym = 257u + l; eb = 0u; ev = 0u;
    } else {
        eb = bz_ilog2(l) - 2u;
        sym = 261u + 4u * eb + ((l >> eb) & 3u);
        ev = l & ((1u << eb) - 1u);
    }
}

// distance 1 .. 32768 -> symbol 0 .. 29, its extra bits and their value
KMM_HD inline void dist_code(uint32_t dist, uint32_t &sym, uint32_t &eb, uint32_t &ev)
{
    const uint32_t d = dist - 1u;
    if (d < 4u) {
        sym = d; eb = 0u; ev = 0u;
    } else {
        const uint32_t k = bz_ilog2(d);
        eb = k - 1u;
        sym = 2u * k + ((d >> eb) & 1u);
        ev = d & ((1u << eb) - 1u);
    }
}

KMM_HD inline uint32_t load32u(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}

KMM_HD inline uint32_t hash4(const uint8_t *p)
{
    return (load32u(p) * 2654435761u) >> (32u - HASH_BITS);
}

// how many of the first `max` bytes at a and b agree (both readable for `max` bytes)
KMM_HD inline uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t max)
{
    uint32_t k = 0;
    for (; k + 8u <= max; k += 8u) {
        uint64_t x, y;
        memcpy(&x, a + k, 8);
        memcpy(&y, b + k, 8);
        if (x != y)
            return k + ((uint32_t)__builtin_ctzll(x ^ y) >> 3);
    }
    for (; k < max && a[k] == b[k]; ++k) {
    }
    return k;
}

#if defined(__HIPCC__)
#define KMM_BZ_UNROLL _Pragma("unroll")
#else
#define KMM_BZ_UNROLL
#endif

// the `count` (8 or 16) bytes at in[at ...) in one request; what lies behind in[n) reads as zero
KMM_HD inline void load_clipped(const uint8_t *in, uint32_t n, uint32_t at, uint64_t *v, uint32_t count)
{
    if (at + count <= n) {
        memcpy(v, in + at, count);
        return;
    }
    v[0] = 0;
    if (count > 8u)
        v[1] = 0;
    for (uint32_t j = 0; j < count && at + j < n; ++j)
        v[j >> 3] |= (uint64_t)in[at + j] << (8u * (j & 7u));
}

// A thread walks its segment CHUNK positions at a time: their candidates (and bytes) arrive in one request each and are then
// picked out of registers — a walk that asks memory for every position pays a trip to L2 per position, 255 in a row.
constexpr uint32_t CHUNK = 8u;

KMM_HD inline uint32_t chunk_cand(const uint64_t *c, int k)
{
    return (uint32_t)(c[k >> 2] >> (16 * (k & 3))) & 0xFFFFu;
}

// the 8 bytes at place k of a chunk's 16 bytes
KMM_HD inline uint64_t chunk_bytes8(const uint64_t *own, int k)
{
    return k ? (own[0] >> (8 * k)) | (own[1] << (64 - 8 * k)) : own[0];
}

// The tokens of the segment [s, e) as the parse left them in cand[]: lit(position, byte), match(position, length, distance).
template <typename L, typename M>
KMM_HD inline void walk_tokens(const uint8_t *in, uint32_t n, const uint16_t *cand, uint32_t s, uint32_t e, L &&lit, M &&match)
{
    uint32_t i = s;
    for (uint32_t b = s; b < e; b += CHUNK) {
        if (i >= b + CHUNK)
            continue; // (a match covers the chunk)
        uint64_t own, c[2];
        load_clipped(in, n, b, &own, 8u);
        memcpy(c, cand + b, 16); // (the scratch has CHUNK entries of slack behind a member's last position)
        KMM_BZ_UNROLL
        for (int k = 0; k < (int)CHUNK; ++k) {
            const uint32_t pos = b + (uint32_t)k;
            if (pos != i || pos >= e)
                continue;
            const uint32_t cd = chunk_cand(c, k);
            if (cd) {
                const uint32_t len = cand[pos + 1u];
                match(pos, len, pos - (cd - 1u));
                i += len;
            } else {
                lit(pos, (uint32_t)(own >> (8 * k)) & 0xFFu);
                ++i;
            }
        }
    }
}

// A workgroup's state for the member at work: LDS on the GPU.
struct Wg {
    uint32_t table[TABLE];   // the CRC tables, then the hash table (position + 1; 0: none), then the tree builders' scratch
    uint32_t bfreq[256];     // byte histogram
    uint8_t lcost[256];      // a literal's cost in quarter bits
    uint32_t lfreq[288], dfreq[32], clfreq[32];
    uint16_t lcode[288], dcode[32], clcode[32]; // codes, bit-reversed: ready for the stream
    uint8_t llen[288], dlen[32], cllen[32];
    uint32_t scan[2][THREADS]; // per thread: header bits << 20 | token bits; prefix sums (ping-pong)
    uint32_t own[THREADS];
    uint32_t crc, hlit, hdist, hclen, stored, body, words;
    uint32_t stat_depth, stat_limited; // the literal / length alphabet: its deepest code before the limit; whether the limiter ran
};

constexpr uint32_t SCR_LIT = 0u, SCR_DIST = 4096u, SCR_CL = 4096u + 512u; // (words of Wg::table)

// Code lengths of one alphabet by ONE lane.  freq[0, n): at least two are non-zero; sorted[0, m): the symbols of non-zero
// frequency by (frequency, symbol) ascending; scr: 6 m + 64 words (LDS on the GPU: the length counts are indexed by data).
// Lengths at most max_bits; codes bit-reversed.  stat_depth: raised to the deepest leaf before the limit; stat_limited: set
// when the limiter ran.
// Returns the last symbol with a code, plus one.
KMM_HD inline uint32_t build_code(const uint32_t *freq, uint32_t n, uint32_t m, const uint32_t *sorted, uint32_t max_bits, uint32_t *scr,
                                  uint8_t *len, uint16_t *code, uint32_t &stat_depth, uint32_t &stat_limited)
{
    uint32_t *wt = scr, *parent = scr + 2u * m, *depth = scr + 4u * m, *count = scr + 6u * m, *next = count + 32;
    for (uint32_t k = 0; k < m; ++k)
        wt[k] = freq[sorted[k]];
    // two queues: the leaves in order, the inner nodes in the order they were made (their weights never decrease)
    uint32_t a = 0, b = m, nxt = m;
    while (nxt < 2u * m - 1u) {
        uint32_t pick[2];
        for (int j = 0; j < 2; ++j) {
            if (a < m && (b >= nxt || wt[a] <= wt[b]))
                pick[j] = a++;
            else
                pick[j] = b++;
        }
        wt[nxt] = wt[pick[0]] + wt[pick[1]];
        parent[pick[0]] = parent[pick[1]] = nxt;
        ++nxt;
    }
    for (uint32_t k = 0; k < 32u; ++k)
        count[k] = 0;
    // depths from the root down; a node that would lie below the limit is put AT the limit and counted, inner nodes too, and
    // its children hang from there (zlib's gen_bitlen): `over` such nodes leave a code that is over-subscribed by over / 2 codes
    // of max_bits.  The depth without the limit, for the statistics, goes where the weights were.
    const uint32_t root = 2u * m - 2u;
    uint32_t *true_depth = wt;
    depth[root] = true_depth[root] = 0;
    uint32_t deepest = 0, overflow = 0;
    for (uint32_t k = root; k-- > 0;) {
        uint32_t d = depth[parent[k]] + 1u;
        const uint32_t td = true_depth[parent[k]] + 1u;
        if (d > max_bits) {
            d = max_bits;
            ++overflow;
        }
        depth[k] = d;
        true_depth[k] = td;
        if (k < m) {
            deepest = td > deepest ? td : deepest;
            ++count[d];
        }
    }
    if (deepest > stat_depth)
        stat_depth = deepest;
    if (overflow) {
        stat_limited = 1u;
        // (a leaf one level up makes room for two at the bottom: the overflowing leaves come up pair by pair)
        int32_t over = (int32_t)overflow;
        do {
            uint32_t bits = max_bits - 1u;
            while (count[bits] == 0u)
                --bits;
            --count[bits];
            count[bits + 1u] += 2u;
            --count[max_bits];
            over -= 2;
        } while (over > 0);
    }
    for (uint32_t s = 0; s < n; ++s)
        len[s] = 0;
    uint32_t k = 0; // (the rarest leaves get the longest codes)
    for (uint32_t bits = max_bits; bits >= 1u; --bits)
        for (uint32_t c = count[bits]; c > 0u; --c)
            len[sorted[k++]] = (uint8_t)bits;
    uint32_t c = 0;
    next[0] = 0;
    count[0] = 0;
    for (uint32_t bits = 1; bits <= max_bits; ++bits) {
        c = (c + count[bits - 1u]) << 1;
        next[bits] = c;
    }
    uint32_t last = 0;
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = len[s];
        code[s] = 0;
        if (l) {
            code[s] = (uint16_t)kmm_gz::rev_bits(next[l]++, (int)l);
            last = s + 1u;
        }
    }
    return last;
}

// value's low nbits (nbits <= 32) into the zeroed stream at bit position `pos`
KMM_HD inline void put_bits(uint32_t *slot, uint32_t pos, uint32_t value, uint32_t nbits)
{
    if (!nbits)
        return;
    const uint32_t w = pos >> 5, sh = pos & 31u;
    KMM_BZ_OR(slot + w, value << sh);
    if (sh + nbits > 32u)
        KMM_BZ_OR(slot + w + 1u, value >> (32u - sh));
}

// A thread's bits: gathered in a 64-bit window that starts at a word of the slot, whole words or-ed out.
struct BitOut {
    uint32_t *slot;
    uint32_t word, fill;
    uint64_t acc;
    KMM_HD BitOut(uint32_t *s, uint32_t pos) : slot(s), word(pos >> 5), fill(pos & 31u), acc(0) {}
    KMM_HD void put(uint32_t value, uint32_t nbits) // nbits <= 32
    {
        acc |= (uint64_t)value << fill;
        fill += nbits;
        if (fill >= 32u) {
            KMM_BZ_OR(slot + word, (uint32_t)acc);
            ++word;
            acc >>= 32;
            fill -= 32u;
        }
    }
    KMM_HD void flush()
    {
        if (fill)
            KMM_BZ_OR(slot + word, (uint32_t)acc);
    }
};

KMM_HD inline uint32_t cl_order(uint32_t i)
{
    // (a table in the code, not in memory: 19 five-bit fields)
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12u ? lo >> (5u * i) : hi >> (5u * (i - 12u))) & 31u);
}

// The symbols of non-zero frequency of freq[0, n) in (frequency, symbol) order -> sorted; symbol s by the thread that owns it.
KMM_HD inline void rank_symbol(const uint32_t *freq, uint32_t n, uint32_t s, uint32_t *sorted)
{
    if (s >= n || !freq[s])
        return;
    const uint32_t f = freq[s];
    uint32_t r = 0;
    for (uint32_t u = 0; u < n; ++u) {
        const uint32_t g = freq[u];
        r += g && (g < f || (g == f && u < s)) ? 1u : 0u;
    }
    sorted[r] = s;
}

KMM_HD inline uint32_t count_nonzero(const uint32_t *freq, uint32_t n)
{
    uint32_t m = 0;
    for (uint32_t u = 0; u < n; ++u)
        m += freq[u] ? 1u : 0u;
    return m;
}

// One member: in[0, n), 1 <= n <= BLOCK -> slot (SLOT bytes, 4-byte aligned); *size: the member's bytes.  crcT: the CRC tables
// of kmm_gpu_inflate.hpp (CRC_TABLE_WORDS); cand: CAND_STRIDE uint16 of scratch.  x.each(f) runs f(t) for t = 0 .. 255 and
// separates it from what follows.
template <typename X>
KMM_HD inline void deflate_member(const X &x, Wg &w, const uint32_t *crcT, const uint8_t *in, uint32_t n, uint16_t *cand, uint32_t *slot,
                                  uint32_t *size)
{
    // crc: the tables borrow the hash table
    x.each([&](uint32_t t) {
        for (uint32_t i = t; i < (uint32_t)kmm_gz::CRC_TABLE_WORDS; i += THREADS)
            w.table[i] = crcT[i];
        w.bfreq[t] = 0;
        if (t == 0) {
            w.crc = 0;
            w.stat_depth = w.stat_limited = 0;
        }
    });
    x.each([&](uint32_t t) {
        const uint32_t s = t * SEG;
        if (s >= n)
            return;
        const uint32_t e = s + SEG < n ? s + SEG : n;
        const uint32_t c = kmm_gz::crc_register(w.table, in + s, e - s, t ? 0u : 0xFFFFFFFFu);
        KMM_BZ_XOR(&w.crc, kmm_gz::crc_shift(w.table + 8 * 256, c, n - e));
        for (uint32_t i = s; i < e; ++i)
            KMM_BZ_ADD(&w.bfreq[in[i]], 1u);
    });
    // costs; the table and the histograms empty
    x.each([&](uint32_t t) {
        for (uint32_t i = t; i < TABLE; i += THREADS)
            w.table[i] = 0;
        const uint32_t f = w.bfreq[t];
        uint32_t q = 60u;
        if (f) {
            q = bz_ilog2q(n) - bz_ilog2q(f); // (f <= n, and bz_ilog2q does not decrease)
            q = q < 4u ? 4u : q > 60u ? 60u : q;
        }
        w.lcost[t] = (uint8_t)q;
        w.lfreq[t] = 0;
        if (t < 32u) {
            w.lfreq[256u + t] = t == 0u ? 1u : 0u; // (one end-of-block)
            w.dfreq[t] = 0;
            w.clfreq[t] = 0;
        }
    });
    // fill
    for (uint32_t p0 = 0; p0 < n; p0 += FILL) {
        x.each([&](uint32_t t) {
            for (uint32_t i = p0 + t; i < p0 + FILL && i < n; i += THREADS)
                cand[i] = i + 4u <= n ? (uint16_t)w.table[hash4(in + i)] : (uint16_t)0;
        });
        if (p0 + FILL >= n)
            break; // (nothing looks the last phase's positions up)
        x.each([&](uint32_t t) {
            for (uint32_t i = p0 + t; i < p0 + FILL && i + 4u <= n; i += THREADS)
                KMM_BZ_MAX(&w.table[hash4(in + i)], i + 1u);
        });
    }
    // parse
    x.each([&](uint32_t t) {
        const uint32_t s = t * SEG;
        if (s >= n)
            return;
        const uint32_t e = s + SEG < n ? s + SEG : n;
        uint32_t i = s;
        for (uint32_t b = s; b < e; b += CHUNK) {
            if (i >= b + CHUNK)
                continue; // (a match covers the chunk)
            // the chunk's bytes with the 8 behind them, its candidates, and the 8 bytes at every candidate: three requests in a
            // row instead of three per position
            uint64_t own[2], c[2], far[CHUNK];
            load_clipped(in, n, b, own, 16u);
            memcpy(c, cand + b, 16);
            uint32_t fast = 0;
            KMM_BZ_UNROLL
            for (int k = 0; k < (int)CHUNK; ++k) {
                const uint32_t pos = b + (uint32_t)k, cd = chunk_cand(c, k);
                far[k] = 0;
                if (pos >= i && pos < e && cd && cd <= pos && cd + 7u <= n) {
                    memcpy(&far[k], in + (cd - 1u), 8);
                    fast |= 1u << k;
                }
            }
            KMM_BZ_UNROLL
            for (int k = 0; k < (int)CHUNK; ++k) {
                const uint32_t pos = b + (uint32_t)k;
                if (pos != i || pos >= e)
                    continue;
                const uint32_t cd = chunk_cand(c, k);
                uint32_t len = 0, dist = 0;
                if (cd && cd <= pos && pos - (cd - 1u) <= WINDOW && e - pos >= MIN_MATCH) {
                    dist = pos - (cd - 1u);
                    const uint32_t room = e - pos < MAX_MATCH ? e - pos : MAX_MATCH;
                    if ((fast >> k) & 1u) {
                        const uint64_t x = chunk_bytes8(own, k) ^ far[k];
                        const uint32_t m = x ? (uint32_t)__builtin_ctzll(x) >> 3 : 8u;
                        if (m >= 8u && room > 8u)
                            len = 8u + match_len(in + pos + 8u, in + (cd - 1u) + 8u, room - 8u);
                        else
                            len = m < room ? m : room;
                    } else {
                        len = match_len(in + pos, in + (cd - 1u), room);
                    }
                    if (len >= MIN_MATCH) {
                        uint32_t ls, leb, lev, ds, deb, dev;
                        len_code(len, ls, leb, lev);
                        dist_code(dist, ds, deb, dev);
                        const uint32_t cost = MATCH_BASE_QBITS + 4u * (leb + deb);
                        uint32_t lits = 0;
                        for (uint32_t j = 0; j < len && lits <= cost; j += 8u) {
                            uint64_t v;
                            load_clipped(in, n, pos + j, &v, 8u);
                            for (uint32_t q = 0; q < 8u && j + q < len; ++q)
                                lits += w.lcost[(v >> (8u * q)) & 0xFFu];
                        }
                        if (lits > cost) {
                            KMM_BZ_ADD(&w.lfreq[ls], 1u);
                            KMM_BZ_ADD(&w.dfreq[ds], 1u);
                        } else {
                            len = 0;
                        }
                    } else {
                        len = 0;
                    }
                }
                if (len) {
                    cand[pos + 1u] = (uint16_t)len; // (len >= 4: pos + 1 lies inside the match and inside the segment)
                    i += len;
                } else {
                    cand[pos] = 0;
                    KMM_BZ_ADD(&w.lfreq[(uint32_t)(own[0] >> (8 * k)) & 0xFFu], 1u);
                    ++i;
                }
            }
        }
    });
    // codes: no distance used -> two codes of one bit, as zlib sends them (every inflater takes a complete code)
    x.each([&](uint32_t t) {
        if (t == 0) {
            const uint32_t m = count_nonzero(w.dfreq, NDIST);
            if (m < 2u) {
                const uint32_t extra = w.dfreq[0] ? 1u : 0u;
                w.dfreq[extra] = 1u;
                if (m == 0u)
                    w.dfreq[1] = 1u;
            }
        }
    });
    x.each([&](uint32_t t) {
        rank_symbol(w.lfreq, NLIT, t, w.table + SCR_LIT);
        if (t + 256u < NLIT)
            rank_symbol(w.lfreq, NLIT, t + 256u, w.table + SCR_LIT);
        if (t < NDIST)
            rank_symbol(w.dfreq, NDIST, t, w.table + SCR_DIST);
    });
    x.each([&](uint32_t t) {
        if (t == 0) {
            const uint32_t m = count_nonzero(w.lfreq, NLIT); // (>= 2: the member's first byte is a literal, and the end-of-block)
            const uint32_t last = build_code(w.lfreq, NLIT, m, w.table + SCR_LIT, 15u, w.table + SCR_LIT + 288u, w.llen, w.lcode,
                                             w.stat_depth, w.stat_limited);
            w.hlit = last < 257u ? 257u : last;
        } else if (t == 64u) {
            uint32_t depth = 0, limited = 0;
            const uint32_t m = count_nonzero(w.dfreq, NDIST);
            w.hdist = build_code(w.dfreq, NDIST, m, w.table + SCR_DIST, 15u, w.table + SCR_DIST + 32u, w.dlen, w.dcode, depth, limited);
        }
    });
    x.each([&](uint32_t t) {
        if (t < w.hlit)
            KMM_BZ_ADD(&w.clfreq[w.llen[t]], 1u);
        if (t + 256u < w.hlit)
            KMM_BZ_ADD(&w.clfreq[w.llen[t + 256u]], 1u);
        if (t < w.hdist)
            KMM_BZ_ADD(&w.clfreq[w.dlen[t]], 1u);
    });
    x.each([&](uint32_t t) {
        if (t == 0) {
            // (the lengths sent are >= 2 different values or one value many times; a second symbol keeps the code complete)
            if (count_nonzero(w.clfreq, NCL) < 2u)
                w.clfreq[w.clfreq[0] ? 1u : 0u] = 1u;
        }
    });
    x.each([&](uint32_t t) {
        if (t < NCL)
            rank_symbol(w.clfreq, NCL, t, w.table + SCR_CL);
    });
    x.each([&](uint32_t t) {
        if (t == 0) {
            uint32_t depth = 0, limited = 0;
            const uint32_t m = count_nonzero(w.clfreq, NCL);
            build_code(w.clfreq, NCL, m, w.table + SCR_CL, 7u, w.table + SCR_CL + 32u, w.cllen, w.clcode, depth, limited);
            uint32_t h = NCL;
            while (h > 4u && w.cllen[cl_order(h - 1u)] == 0)
                --h;
            w.hclen = h;
        }
    });
    // bits per thread: the code lengths at places 2 t and 2 t + 1 of the header, the thread's tokens
    x.each([&](uint32_t t) {
        uint32_t hb = 0, tb = 0;
        for (uint32_t p = 2u * t; p < 2u * t + 2u; ++p)
            if (p < w.hlit + w.hdist)
                hb += w.cllen[p < w.hlit ? w.llen[p] : w.dlen[p - w.hlit]];
        const uint32_t s = t * SEG;
        const uint32_t e = s + SEG < n ? s + SEG : n;
        if (s < e)
            walk_tokens(in, n, cand, s, e, [&](uint32_t, uint32_t byte) { tb += w.llen[byte]; },
                        [&](uint32_t, uint32_t len, uint32_t dist) {
                            uint32_t ls, leb, lev, ds, deb, dev;
                            len_code(len, ls, leb, lev);
                            dist_code(dist, ds, deb, dev);
                            tb += w.llen[ls] + leb + w.dlen[ds] + deb;
                        });
        w.own[t] = w.scan[0][t] = hb << 20 | tb; // (the tokens of a member are fewer than 2^20 bits: 15 bits a byte at most)
    });
    for (uint32_t d = 1, r = 0; d < THREADS; d <<= 1, r ^= 1u)
        x.each([&](uint32_t t) { w.scan[r ^ 1u][t] = w.scan[r][t] + (t >= d ? w.scan[r][t - d] : 0u); });
    // (eight rounds: the inclusive sums are in scan[0])
    x.each([&](uint32_t t) {
        if (t == 0) {
            const uint32_t tot = w.scan[0][THREADS - 1u];
            const uint32_t bits = 17u + 3u * w.hclen + (tot >> 20) + (tot & 0xFFFFFu) + w.llen[EOB];
            const uint32_t bytes = (bits + 7u) >> 3;
            w.stored = bytes >= n + 5u ? 1u : 0u;
            w.body = w.stored ? n + 5u : bytes;
            w.words = (18u + w.body + 8u + 3u) >> 2;
        }
    });
    x.each([&](uint32_t t) {
        for (uint32_t i = t; i < w.words; i += THREADS)
            slot[i] = 0;
    });
    x.each([&](uint32_t t) {
        const uint32_t body = w.body, total = 18u + body + 8u;
        if (t == 0) {
            put_bits(slot, 0u, 0x04088B1Fu, 32u);          // ID1 ID2 CM FLG.FEXTRA
            put_bits(slot, 64u, 0x0006FF00u, 32u);         // XFL 0, OS ff, XLEN 6
            put_bits(slot, 96u, 0x00024342u, 32u);         // 'B' 'C' 2
            put_bits(slot, 128u, total - 1u, 16u);         // BSIZE
            put_bits(slot, 8u * (18u + body), ~w.crc, 32u);
            put_bits(slot, 8u * (18u + body) + 32u, n, 32u);
            *size = total;
        }
        const uint32_t s = t * SEG;
        const uint32_t e = s + SEG < n ? s + SEG : n;
        if (w.stored) {
            if (t == 0) {
                put_bits(slot, 144u, 1u, 8u); // BFINAL 1, BTYPE 0, the bits to the byte's end
                put_bits(slot, 152u, n | (~n << 16), 32u);
            }
            uint8_t *o = reinterpret_cast<uint8_t *>(slot) + 23u;
            for (uint32_t i = s; i < e; ++i)
                o[i] = in[i];
            return;
        }
        const uint32_t base0 = 144u + 17u + 3u * w.hclen;
        const uint32_t excl = w.scan[0][t] - w.own[t], tot = w.scan[0][THREADS - 1u];
        if (t == 0) {
            BitOut h(slot, 144u);
            h.put(1u | 2u << 1, 3u); // BFINAL 1, BTYPE 2
            h.put(w.hlit - 257u, 5u);
            h.put(w.hdist - 1u, 5u);
            h.put(w.hclen - 4u, 4u);
            for (uint32_t i = 0; i < w.hclen; ++i)
                h.put(w.cllen[cl_order(i)], 3u);
            h.flush();
            put_bits(slot, base0 + (tot >> 20) + (tot & 0xFFFFFu), w.lcode[EOB], w.llen[EOB]);
        }
        {
            BitOut h(slot, base0 + (excl >> 20));
            for (uint32_t p = 2u * t; p < 2u * t + 2u; ++p)
                if (p < w.hlit + w.hdist) {
                    const uint32_t l = p < w.hlit ? w.llen[p] : w.dlen[p - w.hlit];
                    h.put(w.clcode[l], w.cllen[l]);
                }
            h.flush();
        }
        BitOut o(slot, base0 + (tot >> 20) + (excl & 0xFFFFFu));
        if (s < e)
            walk_tokens(in, n, cand, s, e, [&](uint32_t, uint32_t byte) { o.put(w.lcode[byte], w.llen[byte]); },
                        [&](uint32_t, uint32_t len, uint32_t dist) {
                            uint32_t ls, leb, lev, ds, deb, dev;
                            len_code(len, ls, leb, lev);
                            dist_code(dist, ds, deb, dev);
                            o.put(w.lcode[ls] | lev << w.llen[ls], w.llen[ls] + leb);
                            o.put(w.dcode[ds] | dev << w.dlen[ds], w.dlen[ds] + deb);
                        });
        o.flush();
    });
}

// where the members of a batch start in the output: sizes[0, n) -> offs[0, n] (offs[n]: the batch's bytes)
KMM_HD inline void member_offsets(const uint32_t *sizes, uint32_t n, unsigned long long *offs)
{
    unsigned long long at = 0;
    for (uint32_t m = 0; m < n; ++m) {
        offs[m] = at;
        at += sizes[m];
    }
    offs[n] = at;
}

#if defined(__HIPCC__)

struct GpuExec {
    template <typename F>
    __device__ __forceinline__ void each(F &&f) const
    {
        f(threadIdx.x);
        __syncthreads();
    }
};

// Persistent workgroups: member m of the batch is in[m * BLOCK ...) of the batch's n bytes; its slot slots + m * SLOT.
// cand: CAND_STRIDE uint16 per workgroup of the grid.
__global__ void __launch_bounds__(256) k_bz_deflate(const uint8_t *__restrict__ in, int64_t n, uint32_t n_members,
                                                    const uint32_t *__restrict__ crcT, uint16_t *__restrict__ cand,
                                                    uint8_t *__restrict__ slots, uint32_t *__restrict__ sizes)
{
    __shared__ Wg w;
    uint16_t *my_cand = cand + (size_t)blockIdx.x * CAND_STRIDE;
    for (uint32_t m = blockIdx.x; m < n_members; m += gridDim.x) {
        const int64_t off = (int64_t)m * BLOCK;
        const uint32_t len = n - off < (int64_t)BLOCK ? (uint32_t)(n - off) : BLOCK;
        deflate_member(GpuExec{}, w, crcT, in + off, len, my_cand, reinterpret_cast<uint32_t *>(slots + (size_t)m * SLOT), sizes + m);
    }
}

// offs[0, n] from sizes[0, n): one workgroup, a span of members per thread
__global__ void __launch_bounds__(1024) k_bz_offsets(const uint32_t *__restrict__ sizes, uint32_t n, unsigned long long *__restrict__ offs)
{
    __shared__ unsigned long long s_sum[1024];
    const uint32_t t = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t a = t * per < n ? t * per : n, b = a + per < n ? a + per : n;
    unsigned long long sum = 0;
    for (uint32_t m = a; m < b; ++m)
        sum += sizes[m];
    s_sum[t] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long at = 0;
        for (uint32_t i = 0; i < 1024u; ++i) {
            const unsigned long long v = s_sum[i];
            s_sum[i] = at;
            at += v;
        }
        offs[n] = at;
    }
    __syncthreads();
    unsigned long long at = s_sum[t];
    for (uint32_t m = a; m < b; ++m) {
        offs[m] = at;
        at += sizes[m];
    }
}

// the members out of their slots, one behind the other: one workgroup per member
__global__ void __launch_bounds__(256) k_bz_gather(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ sizes,
                                                   const unsigned long long *__restrict__ offs, uint8_t *__restrict__ out)
{
    const uint32_t m = blockIdx.x, size = sizes[m];
    const uint8_t *src = slots + (size_t)m * SLOT;
    uint8_t *dst = out + offs[m];
    // (the destination's 4-byte words whole, its ragged head and tail byte by byte)
    const uint32_t head = (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u);
    const uint32_t h = head < size ? head : size, words = (size - h) >> 2;
    if (threadIdx.x < h)
        dst[threadIdx.x] = src[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < words; i += 256u) {
        uint32_t v;
        memcpy(&v, src + h + 4u * i, 4);
        *reinterpret_cast<uint32_t *>(dst + h + 4u * i) = v;
    }
    const uint32_t done = h + 4u * words;
    if (done + threadIdx.x < size)
        dst[done + threadIdx.x] = src[done + threadIdx.x];
}

#endif // __HIPCC__

} // namespace kmm_bz
