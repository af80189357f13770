// kmm_gpu_gunzip.hpp — part of libkmm: a PLAIN gzip stream (what `gzip reads.fq` writes: one deflate stream, or several
// members back to back, no sizes anywhere) inflated ON THE GPU (kmm_map_gzip; included by kmm.hip, compiled by itself with
// g++ in tests/test_gpu_gunzip_on_the_cpu.py, where the very same pipeline runs on the CPU against zlib).
//
// Why.  BGZF members carry their sizes and are independent: one lane per member (kmm_gpu_inflate.hpp).  A plain gzip file has
// neither, and the host reader inflates it at ~3 GB/s on 16 threads (kmm_inflate.hpp: speculative block starts with markers for
// the unknown 32 KiB of history — the pugz / rapidgzip idea).  Here that same idea is laid out for the GPU:
//   1. find     candidate bit positions every S bytes of the window; for each one a WAVEFRONT tests 64 consecutive bit
//               positions at a time (13-bit prefilter, the Kraft sum of the code-length code, then the full block header:
//               kmm_gz::block_header) — the first non-final dynamic-Huffman header at or after the candidate is a chunk start;
//   2. decode   one LANE per chunk, from its start to the first block boundary at or after the next chunk's start, into
//               16-bit symbols (0..255 a byte, MARK + i = byte i of the unknown window) behind a prefix of WIN markers;
//               a lane that sees BFINAL notes the trailer's position, parses the next member's header and goes on with
//               an empty history (a back-reference before the member's start is an error);
//   3. accept   chunk j stands iff chunk j-1 ended exactly at j's start, at a block boundary; otherwise j is dropped and
//               j-1 is continued to the next start — follow-up launches over the lanes that need it (run_call below), as
//               for an output slot that ran full (the lane goes on in a new piece whose prefix is its last WIN symbols);
//   4. windows  chunk j's window = the last WIN resolved bytes before it: a serial chain, composed hierarchically — the
//               32 K-entry maps of G chunks inside a group (one workgroup per group, in LDS), then over the groups (one
//               workgroup), then every chunk's window from its group's (k_gz_compose / k_gz_chain / k_gz_fix);
//   5. resolve  every symbol -> byte in one parallel pass, which also checks that no marker reaches before the member's real
//               history;
//   6. CRC32 / ISIZE per member: CRC registers of 64 KiB parts on the device, folded on the host with the x^(8n) shift
//               (kmm_gz::crc_shift) — before anything is mapped.
// Everything a lane reads or writes is bounds-checked against the window and its slot: a damaged stream ends in an error code.
// The orchestration (run_call) is written once, against a backend: the GPU one lives in kmm.hip, the CPU one below.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

#include "kmm_gpu_inflate.hpp"

namespace kmm_gunzip {

using kmm_gz::Bits;

constexpr uint32_t WIN = 32768;
constexpr uint16_t MARK = 0x8000;  // symbol MARK + i = byte i of the chunk's unknown window
constexpr int MAX_EVENTS = 8;      // member ends one piece records (more: the piece stops, a new one goes on)
constexpr uint64_t NPOS = ~0ull;

enum Status { ST_DONE = 1, ST_FULL = 2, ST_END = 3, ST_STREAM_END = 4, ST_FAIL = 5 };
//   DONE        stopped at a block boundary at or after the target
//   FULL        the slot (or the event list) ran full: stopped at the last boundary, to be continued in a new piece
//   END         the window ended: stopped at the last boundary (the next call goes on there)
//   STREAM_END  behind the last member there is nothing, or only zero bytes: the whole window is used
//   FAIL        the data cannot be a deflate stream from this start (a real error only where the start is verified)
enum Mode { M_BLOCK = 0, M_HEADER = 1 }; // what begins at a boundary: a deflate block / a gzip member header

// One lane's job.  slot: WIN + cap (+ 16) symbols; the prefix is WIN markers (prev == nullptr) or prev[prev_n, prev_n + WIN)
// — the last WIN symbols of the piece before, whose output is prev[WIN, WIN + prev_n).
struct Work {
    uint64_t bit;       // where to start: a block boundary (mode M_BLOCK) or a member header (M_HEADER, byte aligned)
    uint64_t target;    // stop at the first block boundary >= target
    uint16_t *slot;
    const uint16_t *prev;
    uint32_t prev_n, cap, mode, mbase; // mbase: slot position of the member's start (0: before the prefix, markers allowed)
};

struct Result {
    uint64_t end_bit;   // the last boundary reached
    uint32_t n_out;     // output symbols at that boundary
    uint32_t status, end_mode, mbase, err, n_events;
    uint32_t ev_off[MAX_EVENTS];  // output offset (in the piece) where a member ended
    uint64_t ev_pos[MAX_EVENTS];  // byte of its trailer in the window
};

// ---- the gzip member header (RFC 1952 2.3) at in[at, n): its length, 0 if it needs bytes behind n, -1 if it is none
KMM_HD inline int64_t member_header_len(const uint8_t *in, uint64_t at, uint64_t n)
{
    if (at + 10 > n)
        return (at < n && in[at] != 0x1f) || (at + 1 < n && in[at + 1] != 0x8b) || (at + 2 < n && in[at + 2] != 8) ? -1 : 0;
    if (in[at] != 0x1f || in[at + 1] != 0x8b || in[at + 2] != 8 || (in[at + 3] & 0xE0))
        return -1;
    const uint32_t flg = in[at + 3];
    uint64_t p = at + 10;
    if (flg & 4) { // FEXTRA
        if (p + 2 > n)
            return 0;
        p += 2 + kmm_gz::rd16(in + p);
    }
    for (uint32_t f = 8; f <= 16; f <<= 1) // FNAME, FCOMMENT: zero-terminated
        if (flg & f) {
            while (p < n && in[p])
                ++p;
            if (p >= n)
                return 0;
            ++p;
        }
    if (flg & 2) // FHCRC
        p += 2;
    return p > n ? 0 : (int64_t)(p - at);
}

KMM_HD inline uint64_t bit_pos(const Bits &b) { return (uint64_t)(b.pos - 16u - 4u * (uint32_t)b.fw) * 8u - (uint64_t)b.cnt; }

KMM_HD inline void seek_bit(Bits &b, uint64_t bit)
{
    kmm_gz::bits_start(b, (uint32_t)(bit >> 3));
    kmm_gz::bits_take(b, (int)(bit & 7u));
}

// ---- one lane: decode w.bit .. the first block boundary >= w.target into w.slot (see Work).  in[0, n_pad) readable, the
// window's own bytes are in[0, n) (n_pad >= 16, n <= n_pad).  prim: kmm_gz::PRIM_WORDS (stride kmm_gz::PS; LDS on the GPU),
// sec: kmm_gz::SEC_WORDS of scratch.
KMM_HD inline void decode_lane(const uint8_t *in, uint32_t n_pad, uint64_t n, const Work &w, Result &r, uint16_t *prim, uint16_t *sec)
{
    using namespace kmm_gz;
    const uint64_t nbits = n * 8u;
    uint16_t *slot = w.slot;
    if (w.prev) {
        for (uint32_t i = 0; i < WIN; ++i)
            slot[i] = w.prev[w.prev_n + i];
    } else {
        for (uint32_t i = 0; i < WIN; ++i)
            slot[i] = (uint16_t)(MARK + i);
    }
    const uint32_t lim = WIN + w.cap;
    uint32_t o = WIN, mbase = w.mbase, mode = w.mode, n_ev = 0;
    uint64_t bit = w.bit;
    // the last boundary
    uint64_t l_bit = bit;
    uint32_t l_o = o, l_mode = mode, l_mbase = mbase, l_ev = 0;
    uint32_t status = 0, err = 0;
    Bits b;
    b.in = in;
    b.n = n_pad;
    const uint16_t *lit = prim, *dst = prim + PRIM_LIT * PS;
    const uint16_t *lit2 = sec, *dst2 = sec + SEC_LIT;
    if (mode == M_BLOCK) {
        if (bit >= nbits)
            status = ST_END;
        else
            seek_bit(b, bit);
    }
    while (!status) {
        if (mode == M_HEADER) {
            const uint64_t at = bit >> 3;
            if (at >= n) {
                status = ST_STREAM_END;
                break;
            }
            if (in[at] == 0) { // zero padding behind the last member, to the end of the window — or trailing garbage
                uint64_t q = at;
                while (q < n && in[q] == 0)
                    ++q;
                status = q == n ? ST_STREAM_END : ST_FAIL;
                err = E_HEADER;
                break;
            }
            const int64_t hl = member_header_len(in, at, n);
            if (hl <= 0) {
                status = hl == 0 ? ST_END : ST_FAIL;
                err = E_HEADER;
                break;
            }
            bit = (at + (uint64_t)hl) * 8u;
            mode = M_BLOCK;
            mbase = o;
            if (bit >= nbits) {
                status = ST_END;
                break;
            }
            seek_bit(b, bit);
            l_bit = bit, l_o = o, l_mode = mode, l_mbase = mbase, l_ev = n_ev;
            if (bit >= w.target) {
                status = ST_DONE;
                break;
            }
        }
        // ---- a block
        bits_refill(b);
        const uint32_t h3 = (uint32_t)b.buf & 7u, final = h3 & 1u, type = h3 >> 1;
        int rc = OK;
        if (type == 0u) {
            bits_take(b, 3);
            bits_take(b, b.cnt & 7);
            bits_refill(b);
            const uint32_t slen = bits_take(b, 16);
            bits_refill(b);
            const uint32_t nlen = bits_take(b, 16);
            const uint32_t at = bits_consumed_bytes(b);
            if ((uint64_t)at > n) {
                status = ST_END;
                break;
            } else if ((slen ^ nlen) != 0xFFFFu) {
                rc = E_STORED;
            } else if ((uint64_t)at + slen > n) {
                status = ST_END;
                break;
            } else if (o + slen > lim) {
                status = ST_FULL;
                break;
            } else {
                for (uint32_t j = 0; j < slen; ++j)
                    slot[o + j] = in[at + j];
                o += slen;
                bits_start(b, at + slen);
            }
        } else {
            uint32_t fin2 = 0, dummy_o = 0;
            bool stored = false;
            rc = block_header(b, n_pad, nullptr, 0, dummy_o, prim, sec, &fin2, &stored);
            while (rc == OK) {
                if (bit_pos(b) > nbits)
                    break;
                bits_refill(b);
                uint32_t e = lit[((uint32_t)b.buf & (uint32_t)(PRIM_LIT - 1)) * PS];
                if (e & LINK) {
                    e = lit2[((e >> 4) & 0x7FFu) + (((uint32_t)b.buf >> LIT_PB) & ((1u << (e & 15u)) - 1u))];
                    bits_take(b, LIT_PB);
                }
                const uint32_t l = e & 15u, sym = e >> 4;
                if (!l) {
                    rc = E_SYMBOL;
                    break;
                }
                bits_take(b, (int)l);
                if (sym < 256u) {
                    if (o >= lim) {
                        status = ST_FULL;
                        break;
                    }
                    slot[o++] = (uint16_t)sym;
                    continue;
                }
                if (sym == 256u)
                    break;
                if (sym > 285u) {
                    rc = E_SYMBOL;
                    break;
                }
                const uint32_t ls = sym - 257u;
                const uint32_t len = len_base_of(ls) + bits_take(b, (int)len_extra_bits(ls));
                bits_refill(b);
                uint32_t d = dst[((uint32_t)b.buf & (uint32_t)(PRIM_DIST - 1)) * PS];
                if (d & LINK) {
                    d = dst2[((d >> 4) & 0x7FFu) + (((uint32_t)b.buf >> DIST_PB) & ((1u << (d & 15u)) - 1u))];
                    bits_take(b, DIST_PB);
                }
                const uint32_t dl = d & 15u, dcode = d >> 4;
                if (!dl || dcode > 29u) {
                    rc = E_SYMBOL;
                    break;
                }
                bits_take(b, (int)dl);
                const uint32_t dist = dist_base_of(dcode) + bits_take(b, (int)dist_extra_bits(dcode));
                if (dist > o - mbase) { // (before the member's start; with mbase = 0 every distance <= WIN <= o is fine)
                    rc = E_DISTANCE;
                    break;
                }
                if (o + len > lim) {
                    status = ST_FULL;
                    break;
                }
                if (dist >= 8u) { // eight symbols per request: the source block ends in front of its destination
                    for (uint32_t j = 0; j < len; j += 8u) { // (up to 7 symbols behind the match: the slot has 16 to spare)
                        uint64_t lo, hi;
                        load16u(reinterpret_cast<const uint8_t *>(slot + o - dist + j), lo, hi);
                        memcpy(slot + o + j, &lo, 8);
                        memcpy(slot + o + j + 4u, &hi, 8);
                    }
                } else {
                    for (uint32_t j = 0; j < len; ++j)
                        slot[o + j] = slot[o - dist + j];
                }
                o += len;
            }
            if (status)
                break;
        }
        const uint64_t here = bit_pos(b);
        if (here > nbits || (rc != OK && here + 64u > nbits)) { // the window ended inside the block
            status = ST_END;
            break;
        }
        if (rc != OK) {
            status = ST_FAIL;
            err = (uint32_t)rc;
            break;
        }
        bit = here;
        if (final) { // the member's last block: its trailer, then a member header
            bits_take(b, b.cnt & 7);
            const uint32_t at = bits_consumed_bytes(b);
            if ((uint64_t)at + 8u > n) {
                status = ST_END;
                break;
            }
            if (n_ev == (uint32_t)MAX_EVENTS) {
                status = ST_FULL;
                break;
            }
            r.ev_off[n_ev] = o - WIN;
            r.ev_pos[n_ev] = at;
            ++n_ev;
            bit = ((uint64_t)at + 8u) * 8u;
            mode = M_HEADER;
            mbase = o;
            l_bit = bit, l_o = o, l_mode = mode, l_mbase = mbase, l_ev = n_ev;
            continue;
        }
        l_bit = bit, l_o = o, l_mode = mode, l_mbase = mbase, l_ev = n_ev;
        if (bit >= w.target)
            status = ST_DONE;
    }
    if (status == ST_STREAM_END) { // (everything behind the last member is used)
        l_bit = nbits;
        l_o = o;
        l_mode = M_HEADER;
        l_ev = n_ev;
    }
    r.end_bit = l_bit;
    r.n_out = l_o - WIN;
    r.status = status;
    r.end_mode = l_mode;
    r.mbase = l_mbase;
    r.err = err;
    r.n_events = l_ev;
}

// ---- find: is there a non-final dynamic-Huffman block header at bit `at`?  (in[0, n) the window, n_pad as in decode_lane)
KMM_HD inline bool header_at(const uint8_t *in, uint32_t n_pad, uint64_t n, uint64_t at, uint16_t *prim, uint16_t *sec)
{
    using namespace kmm_gz;
    const uint64_t byte = at >> 3;
    if (byte + 16u > n)
        return false;
    uint64_t lo, hi;
    load16u(in + byte, lo, hi);
    const uint32_t s = (uint32_t)(at & 7u);
    const uint64_t w0 = s ? (lo >> s) | (hi << (64u - s)) : lo, w1 = hi >> s;
    // BFINAL = 0, BTYPE = 2 (bits 100, LSB first), HLIT <= 29, HDIST <= 29
    if ((w0 & 7u) != 4u || ((w0 >> 3) & 31u) > 29u || ((w0 >> 8) & 31u) > 29u)
        return false;
    // the code-length code must be complete: Kraft sum of its lengths (3 bits each from bit 17 on)
    const uint32_t hclen = (uint32_t)((w0 >> 13) & 15u) + 4u;
    uint32_t kraft = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        const uint32_t p = 17u + 3u * i;
        const uint32_t v = (uint32_t)((p < 64u ? (w0 >> p) | (p > 61u ? w1 << (64u - p) : 0ull) : w1 >> (p - 64u)) & 7u);
        kraft += v ? 1u << (7u - v) : 0u;
    }
    if (kraft != 128u)
        return false;
    Bits b;
    b.in = in;
    b.n = n_pad;
    seek_bit(b, at);
    uint32_t final = 0, dummy_o = 0;
    bool stored = false;
    const int rc = block_header(b, n_pad, nullptr, 0, dummy_o, prim, sec, &final, &stored);
    return rc == OK && !final && !stored && bit_pos(b) <= n * 8u;
}

// ---- the window chain: entry x of a 32 K map (or of a symbol stream) through the window bytes w
KMM_HD inline uint8_t resolve_sym(uint16_t s, const uint8_t *w) { return s < 256u ? (uint8_t)s : w[s & 0x7FFFu]; }
KMM_HD inline uint16_t compose_sym(uint16_t s, const uint16_t *m) { return s < 256u ? s : m[s & 0x7FFFu]; }

// What the window kernels need of a chunk: its out-map = slot[n + i], i < WIN, of its last piece.
struct MapRef {
    const uint16_t *map;
};

// One resolve job: a piece's output symbols -> out[off, off + n); markers below `floor` reach before the member's history.
struct PieceRef {
    const uint16_t *sym; // the piece's output (slot + WIN)
    uint64_t off;
    uint32_t n, chunk, floor, pad;
};

struct Part {        // a CRC part: out[off, off + len), len <= CRC_PART
    uint64_t off;
    uint32_t len, pad;
};
constexpr uint32_t CRC_PART = 65536;

#if defined(__HIPCC__)
// find: one wavefront per candidate c (grid-stride), bits [c * S8, (c + 1) * S8) of the window; starts[c] = the first bit whose
// header parses, NPOS if none.  tabs: SEC_WORDS uint16 per thread of the grid.
__global__ void __launch_bounds__(64) k_gz_find(const uint8_t *__restrict__ in, uint32_t n_pad, uint64_t n, uint64_t S8, uint32_t c0,
                                                uint32_t n_cand, uint16_t *__restrict__ tabs, unsigned long long *__restrict__ starts)
{
    __shared__ uint16_t s_prim[64 * kmm_gz::PRIM_WORDS];
    uint16_t *prim = s_prim + threadIdx.x;
    uint16_t *sec = tabs + (size_t)(blockIdx.x * 64u + threadIdx.x) * kmm_gz::SEC_WORDS;
    for (uint32_t c = blockIdx.x; c < n_cand; c += gridDim.x) {
        const uint64_t a = (uint64_t)(c0 + c) * S8, e = a + S8 < n * 8u ? a + S8 : n * 8u;
        unsigned long long found = NPOS;
        for (uint64_t base = a; base < e && found == NPOS; base += 64u) {
            const uint64_t at = base + threadIdx.x;
            const bool hit = at < e && header_at(in, n_pad, n, at, prim, sec);
            const unsigned long long m = __ballot(hit);
            if (m)
                found = base + (uint64_t)(__ffsll((long long)m) - 1);
        }
        if (threadIdx.x == 0)
            starts[c] = found;
    }
}

// decode: one lane per job (grid-stride); tabs: SEC_WORDS uint16 per thread of the grid
__global__ void __launch_bounds__(64) k_gz_decode(const uint8_t *__restrict__ in, uint32_t n_pad, uint64_t n, const Work *__restrict__ work,
                                                  Result *__restrict__ res, uint32_t n_work, uint16_t *__restrict__ tabs)
{
    __shared__ uint16_t s_prim[64 * kmm_gz::PRIM_WORDS];
    uint16_t *prim = s_prim + threadIdx.x;
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    uint16_t *sec = tabs + (size_t)t * kmm_gz::SEC_WORDS;
    for (uint32_t i = t; i < n_work; i += gridDim.x * 64u) {
        const Work w = work[i];
        Result r;
        decode_lane(in, n_pad, n, w, r, prim, sec);
        res[i] = r;
    }
}

constexpr uint32_t WT = 1024, WPT = WIN / WT; // window kernels: threads, entries per thread

// a group's chunks [g G, min(g G + G, n)): the composition of their maps, in terms of the group's first window
__global__ void __launch_bounds__(1024) k_gz_compose(const MapRef *__restrict__ maps, uint32_t n, uint32_t G, uint16_t *__restrict__ gmaps)
{
    __shared__ uint16_t cur[WIN];
    const uint32_t g = blockIdx.x, j0 = g * G, j1 = j0 + G < n ? j0 + G : n;
    for (uint32_t r = 0; r < WPT; ++r)
        cur[threadIdx.x + r * WT] = maps[j0].map[threadIdx.x + r * WT];
    for (uint32_t j = j0 + 1; j < j1; ++j) {
        uint16_t v[WPT];
        __syncthreads();
        for (uint32_t r = 0; r < WPT; ++r)
            v[r] = compose_sym(maps[j].map[threadIdx.x + r * WT], cur);
        __syncthreads();
        for (uint32_t r = 0; r < WPT; ++r)
            cur[threadIdx.x + r * WT] = v[r];
    }
    __syncthreads();
    for (uint32_t r = 0; r < WPT; ++r)
        gmaps[(size_t)g * WIN + threadIdx.x + r * WT] = cur[threadIdx.x + r * WT];
}

// over the groups (one workgroup): gwin[g] = the window in front of group g, from w0 (the stream's window before the call)
__global__ void __launch_bounds__(1024) k_gz_chain(const uint16_t *__restrict__ gmaps, uint32_t n_groups, const uint8_t *__restrict__ w0,
                                                   uint8_t *__restrict__ gwin)
{
    __shared__ uint8_t w[WIN];
    for (uint32_t r = 0; r < WPT; ++r)
        w[threadIdx.x + r * WT] = w0[threadIdx.x + r * WT];
    for (uint32_t g = 0; g < n_groups; ++g) {
        uint8_t v[WPT];
        __syncthreads();
        for (uint32_t r = 0; r < WPT; ++r) {
            gwin[(size_t)g * WIN + threadIdx.x + r * WT] = w[threadIdx.x + r * WT];
            v[r] = resolve_sym(gmaps[(size_t)g * WIN + threadIdx.x + r * WT], w);
        }
        __syncthreads();
        for (uint32_t r = 0; r < WPT; ++r)
            w[threadIdx.x + r * WT] = v[r];
    }
}

// every chunk's window from its group's; the last group also writes the window behind the last chunk to w_after
__global__ void __launch_bounds__(1024) k_gz_fix(const MapRef *__restrict__ maps, uint32_t n, uint32_t G, const uint8_t *__restrict__ gwin,
                                                 uint8_t *__restrict__ win, uint8_t *__restrict__ w_after)
{
    __shared__ uint8_t w[WIN];
    const uint32_t g = blockIdx.x, j0 = g * G, j1 = j0 + G < n ? j0 + G : n;
    for (uint32_t r = 0; r < WPT; ++r)
        w[threadIdx.x + r * WT] = gwin[(size_t)g * WIN + threadIdx.x + r * WT];
    for (uint32_t j = j0; j < j1; ++j) {
        uint8_t v[WPT];
        __syncthreads();
        for (uint32_t r = 0; r < WPT; ++r) {
            win[(size_t)j * WIN + threadIdx.x + r * WT] = w[threadIdx.x + r * WT];
            v[r] = resolve_sym(maps[j].map[threadIdx.x + r * WT], w);
        }
        __syncthreads();
        for (uint32_t r = 0; r < WPT; ++r)
            w[threadIdx.x + r * WT] = v[r];
    }
    if (j1 == n)
        for (uint32_t r = 0; r < WPT; ++r)
            w_after[threadIdx.x + r * WT] = w[threadIdx.x + r * WT];
}

// symbols -> bytes, one workgroup per piece (grid-stride); err[0] += markers below the piece's floor
__global__ void __launch_bounds__(256) k_gz_resolve(const PieceRef *__restrict__ pieces, uint32_t n_pieces, const uint8_t *__restrict__ win,
                                                    uint8_t *__restrict__ out, unsigned int *__restrict__ err)
{
    __shared__ uint8_t w[WIN];
    for (uint32_t p = blockIdx.x; p < n_pieces; p += gridDim.x) {
        const PieceRef pr = pieces[p];
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < WIN; i += 256u)
            w[i] = win[(size_t)pr.chunk * WIN + i];
        __syncthreads();
        uint32_t bad = 0;
        for (uint32_t i = threadIdx.x; i < pr.n; i += 256u) {
            const uint16_t s = pr.sym[i];
            bad += s >= 256u && (s & 0x7FFFu) < pr.floor;
            out[pr.off + i] = resolve_sym(s, w);
        }
        if (bad)
            atomicAdd(err, bad);
    }
}

// the CRC register of every part, from a zero register (crcT: the 8 x 256 slicing tables)
__global__ void __launch_bounds__(256) k_gz_crc(const uint8_t *__restrict__ out, const Part *__restrict__ parts, uint32_t n_parts,
                                                const uint32_t *__restrict__ crcT, uint32_t *__restrict__ regs)
{
    __shared__ uint32_t T[8 * 256];
    for (uint32_t i = threadIdx.x; i < 8u * 256u; i += 256u)
        T[i] = crcT[i];
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_parts)
        regs[i] = kmm_gz::crc_register(T, out + parts[i].off, parts[i].len, 0u);
}
#endif

// ---- the orchestration of one call (host code, for either backend)

// what a stream keeps from one call to the next
struct StreamState {
    uint32_t bit = 0;          // bit offset inside the first byte of the next window
    uint32_t mode = M_HEADER;  // what starts there
    uint32_t hist = 0;         // real bytes of the member's history at the end of the window (<= WIN)
    uint32_t crc = 0xFFFFFFFFu, isize = 0; // the member in progress: CRC register and length so far
};

struct CallStats {
    uint64_t chunks = 0, false_starts = 0, continuations = 0, members = 0;
};

struct CallOut {
    uint64_t consumed = 0;   // compressed bytes used (the next window starts there, at StreamState::bit)
    uint64_t n_out = 0;      // inflated bytes written
    bool stream_end = false; // nothing but zero bytes behind the last member
    bool hit_cap = false;    // stopped at the size limit
    int err = 0;             // 0, or an kmm_gz::Err (the call's output is not to be used)
    uint64_t err_at = 0;     // compressed byte near the error
};

struct ChunkPlan {
    uint64_t start;
    uint32_t mode;
    bool live = true, link_ok = false, cont = false;
    uint64_t target = NPOS;
    uint32_t base_cap = 0;
    std::vector<int> pieces; // indexes into the call's piece list
};

struct PieceInfo {
    uint16_t *slot;
    uint64_t bit; // where the piece started
    uint32_t cap;
    Result r;
};

// Backend B:  uint16_t *alloc_syms(size_t n)  (valid until the call ends; nullptr: out of memory)
//             bool find(const uint8_t *comp, uint64_t n, uint64_t S8, uint32_t c0, uint32_t n_cand, uint64_t *starts)
//             bool decode(const Work *w, Result *r, size_t n)
//             bool windows(const MapRef *maps, uint32_t n_chunks, uint32_t G)   (the stream's window -> every chunk's; the
//                                                                               window behind the last chunk becomes the stream's)
//             bool resolve(const PieceRef *p, size_t n, uint64_t *bad)          (into the call's output)
//             bool crc(const Part *p, size_t n, uint32_t *regs)
// A backend error (false) is returned as -1.
template <class B>
int run_call(B &be, const uint8_t *comp, uint64_t n, bool last, uint64_t S, uint64_t out_cap, StreamState &st, CallOut &co, CallStats &cs)
{
    using namespace kmm_gz;
    co = CallOut();
    // 1. chunk starts
    std::vector<ChunkPlan> ch;
    ch.push_back(ChunkPlan());
    ch[0].start = st.bit;
    ch[0].mode = st.mode;
    const uint64_t S8 = S * 8u;
    const uint32_t n_cand = n > S ? (uint32_t)((n - 1) / S) : 0u; // candidates 1 .. n_cand: bits [c S8, (c + 1) S8)
    if (n_cand) {
        std::vector<uint64_t> starts(n_cand);
        if (!be.find(comp, n, S8, 1u, n_cand, starts.data()))
            return -1;
        for (uint32_t c = 0; c < n_cand; ++c)
            if (starts[c] != NPOS) {
                ChunkPlan p;
                p.start = starts[c];
                p.mode = M_BLOCK;
                ch.push_back(p);
            }
    }
    cs.chunks += ch.size();
    // slot size: the chunk's compressed span times the stream's ratio so far (the caller's estimate), with room to spare
    std::vector<PieceInfo> pcs;
    std::vector<Work> work;
    std::vector<int> work_chunk;
    auto add_work = [&](int j, uint64_t bit, uint32_t mode, uint32_t cap, const PieceInfo *prev) -> bool {
        uint16_t *slot = be.alloc_syms((size_t)WIN + cap + 16u);
        if (!slot)
            return false;
        Work w;
        w.bit = bit;
        w.target = ch[j].target;
        w.slot = slot;
        w.prev = prev ? prev->slot : nullptr;
        w.prev_n = prev ? prev->r.n_out : 0u;
        w.cap = cap;
        w.mode = mode;
        w.mbase = prev ? (prev->r.mbase > prev->r.n_out ? prev->r.mbase - prev->r.n_out : 0u) : 0u;
        work.push_back(w);
        work_chunk.push_back(j);
        PieceInfo pi;
        pi.slot = slot;
        pi.bit = bit;
        pi.cap = cap;
        memset(&pi.r, 0, sizeof pi.r);
        ch[j].pieces.push_back((int)pcs.size());
        pcs.push_back(pi);
        return true;
    };
    auto launch = [&]() -> bool {
        std::vector<Result> res(work.size());
        if (!be.decode(work.data(), res.data(), work.size()))
            return false;
        for (size_t i = 0; i < work.size(); ++i)
            pcs[(size_t)ch[(size_t)work_chunk[i]].pieces.back()].r = res[i];
        work.clear();
        work_chunk.clear();
        return true;
    };
    for (size_t j = 0; j < ch.size(); ++j) {
        ch[j].target = j + 1 < ch.size() ? ch[j + 1].start : NPOS;
        const uint64_t span = (j + 1 < ch.size() ? ch[j + 1].start / 8 : n) - ch[j].start / 8 + 1;
        const double want = (double)span * be.ratio * 1.25 + 4096.0;
        ch[j].base_cap = want > (double)(1u << 26) ? (1u << 26) : (uint32_t)want;
        if (!add_work((int)j, ch[j].start, ch[j].mode, ch[j].base_cap, nullptr))
            return -1;
    }
    if (!launch())
        return -1;
    // 2. accept / continue, round after round.  Walking the live chunks in order, the OWNER is the chunk whose end decides
    // the next link.  A link judged against an owner that will be continued (or that failed, or ran full) waits for a later
    // round; "verified": every link from chunk 0 to the owner stands (a failure there is the stream's, not a false start's).
    for (;;) {
        size_t owner = 0;
        bool owner_in_ok = true, verified = true;
        uint64_t total = 0; // output of the verified chunks in front of the owner
        auto out_of = [&](const ChunkPlan &c) {
            uint64_t t = 0;
            for (int pi : c.pieces)
                t += pcs[(size_t)pi].r.n_out;
            return t;
        };
        auto cut_behind = [&](size_t j) { // the call has its fill: what lies behind chunk j waits for the next call
            for (size_t q = j + 1; q < ch.size(); ++q)
                ch[q].live = false;
            co.hit_cap = true;
        };
        for (size_t j = 1; j <= ch.size(); ++j) {
            if (j < ch.size() && !ch[j].live)
                continue;
            ChunkPlan &o = ch[owner];
            const Result &r = pcs[(size_t)o.pieces.back()].r;
            if (verified && r.status == ST_FAIL) {
                co.err = r.err ? (int)r.err : E_SYMBOL;
                co.err_at = r.end_bit / 8;
                return 0;
            }
            if (verified && r.status == ST_FULL && total + out_of(o) >= out_cap) {
                cut_behind(owner);
                break;
            }
            if (j == ch.size()) { // the last live chunk: it goes on to the end of the window
                if ((r.status == ST_FULL && verified) || r.status == ST_DONE)
                    o.cont = true;
                break;
            }
            if (o.cont) { // pending: the link is judged when the owner has gone on
                verified = false;
                owner = j;
                owner_in_ok = false;
            } else if (r.status == ST_DONE) {
                if (r.end_bit == ch[j].start && r.end_mode == M_BLOCK) {
                    if (verified)
                        total += out_of(o);
                    ch[j].link_ok = true;
                    owner = j;
                    owner_in_ok = true;
                } else if (r.end_bit >= ch[j].start) {
                    ch[j].live = false; // a false start (or one behind one): the owner's end lies past it
                    ++cs.false_starts;
                } else {
                    o.cont = true; // the owner stopped at a start dropped before: it goes on to this one
                    verified = false;
                    owner = j;
                    owner_in_ok = false;
                }
            } else if (r.status == ST_FULL || r.status == ST_FAIL) {
                if (r.status == ST_FULL && owner_in_ok)
                    o.cont = true;
                verified = false;
                owner = j;
                owner_in_ok = false;
            } else { // END / STREAM_END: nothing behind the owner can be reached
                ch[j].live = false;
                ++cs.false_starts;
            }
        }
        // targets follow the live chunks
        int prev_live = -1;
        for (size_t j = 0; j < ch.size(); ++j)
            if (ch[j].live) {
                if (prev_live >= 0)
                    ch[(size_t)prev_live].target = ch[j].start;
                prev_live = (int)j;
            }
        if (prev_live >= 0)
            ch[(size_t)prev_live].target = NPOS;
        for (size_t j = 0; j < ch.size(); ++j) {
            if (!ch[j].live || !ch[j].cont)
                continue;
            ch[j].cont = false;
            const PieceInfo last_p = pcs[(size_t)ch[j].pieces.back()];
            const Result &r = last_p.r;
            if (r.status != ST_DONE && r.status != ST_FULL)
                continue;
            if (r.status == ST_DONE && r.end_bit >= ch[j].target) // (the target moved back: nothing to do)
                continue;
            uint32_t cap = ch[j].base_cap;
            if (r.status == ST_FULL) {
                // no progress at all (not even past member ends, which fill the event list without output): a block larger
                // than the slot — four times the room; else twice (a stream of high ratio gets geometric pieces)
                const bool stuck = r.n_out == 0 && r.end_bit == last_p.bit;
                const uint64_t grow = stuck ? (uint64_t)last_p.cap * 4u : r.n_out == 0 ? (uint64_t)last_p.cap : (uint64_t)last_p.cap * 2u;
                cap = grow > (1u << 28) ? (1u << 28) : (uint32_t)grow;
                if (stuck && last_p.cap >= (1u << 28)) { // a block larger than any slot: not a deflate stream
                    co.err = E_OUTPUT;
                    co.err_at = r.end_bit / 8;
                    return 0;
                }
            }
            ++cs.continuations;
            if (!add_work((int)j, r.end_bit, r.end_mode, cap, &last_p))
                return -1;
        }
        if (work.empty())
            break;
        if (!launch())
            return -1;
    }
    // 3. the chunks that stand, in order: the call's output, its end, every chunk's floor.  At most out_cap bytes: the call
    // ends in front of the chunk that would pass it (each live chunk's predecessor ended exactly at its start), unless that is
    // the first chunk (its pieces stopped growing at the cap above)
    std::vector<int> live;
    {
        uint64_t total = 0;
        for (size_t j = 0; j < ch.size(); ++j) {
            if (!ch[j].live)
                continue;
            uint64_t t = 0;
            for (int pi : ch[j].pieces)
                t += pcs[(size_t)pi].r.n_out;
            if (!live.empty() && total + t > out_cap) {
                for (size_t q = j; q < ch.size(); ++q)
                    ch[q].live = false;
                co.hit_cap = true;
                break;
            }
            total += t;
            live.push_back((int)j);
        }
    }
    const Result &fin = pcs[(size_t)ch[(size_t)live.back()].pieces.back()].r;
    std::vector<MapRef> maps;
    std::vector<PieceRef> prefs;
    struct Seg { uint64_t off; uint32_t len; int ev_piece; int ev; };
    uint32_t hist = st.mode == M_HEADER ? 0u : st.hist;
    uint64_t off = 0;
    std::vector<uint64_t> ends;     // output offsets where members end (with their trailer positions)
    std::vector<uint64_t> trailers;
    for (size_t li = 0; li < live.size(); ++li) {
        const ChunkPlan &c = ch[(size_t)live[li]];
        const uint32_t floor = WIN - (hist < WIN ? hist : WIN);
        uint64_t chunk_n = 0, last_start = c.mode == M_HEADER ? 0u : NPOS;
        for (int pi : c.pieces) {
            const PieceInfo &p = pcs[(size_t)pi];
            PieceRef pr;
            pr.sym = p.slot + WIN;
            pr.off = off + chunk_n;
            pr.n = p.r.n_out;
            pr.chunk = (uint32_t)maps.size();
            pr.floor = floor;
            pr.pad = 0;
            if (pr.n)
                prefs.push_back(pr);
            for (uint32_t e = 0; e < p.r.n_events; ++e) {
                ends.push_back(off + chunk_n + p.r.ev_off[e]);
                trailers.push_back(p.r.ev_pos[e]);
                last_start = chunk_n + p.r.ev_off[e];
            }
            chunk_n += p.r.n_out;
        }
        const PieceInfo &lp = pcs[(size_t)c.pieces.back()];
        MapRef m;
        m.map = lp.slot + lp.r.n_out;
        maps.push_back(m);
        if (last_start != NPOS)
            hist = (uint32_t)((chunk_n - last_start) < WIN ? chunk_n - last_start : WIN);
        else
            hist = (uint32_t)((uint64_t)hist + chunk_n < WIN ? hist + chunk_n : WIN);
        off += chunk_n;
    }
    co.n_out = off;
    if (fin.status == ST_STREAM_END) {
        co.consumed = n;
        co.stream_end = true;
    } else {
        co.consumed = fin.end_bit >> 3;
    }
    if (last && !co.hit_cap && fin.status != ST_STREAM_END) {
        co.err = E_INPUT; // the file ends inside a member
        co.err_at = fin.end_bit / 8;
        return 0;
    }
    // 4. windows, 5. resolve
    const uint32_t n_chunks = (uint32_t)maps.size();
    uint32_t G = 1;
    while ((uint64_t)G * G < n_chunks)
        ++G;
    if (!be.windows(maps.data(), n_chunks, G))
        return -1;
    uint64_t bad = 0;
    if (!be.resolve(prefs.data(), prefs.size(), &bad))
        return -1;
    if (bad) {
        co.err = E_DISTANCE; // a back-reference before the start of the member
        co.err_at = ch[0].start / 8;
        return 0;
    }
    // 6. CRC32 and ISIZE of every member that ends in the call; the one in progress goes on in the stream state
    std::vector<Part> parts;
    std::vector<int> part_member; // index into ends (or -1: the member in progress)
    {
        uint64_t a = 0;
        for (size_t m = 0; m <= ends.size(); ++m) {
            const uint64_t b = m < ends.size() ? ends[m] : off;
            for (uint64_t x = a; x < b; x += CRC_PART) {
                Part p;
                p.off = x;
                p.len = (uint32_t)(b - x < CRC_PART ? b - x : CRC_PART);
                p.pad = 0;
                parts.push_back(p);
                part_member.push_back((int)m);
            }
            a = b;
        }
    }
    std::vector<uint32_t> regs(parts.size());
    if (!parts.empty() && !be.crc(parts.data(), parts.size(), regs.data()))
        return -1;
    uint32_t X[CRC_SHIFT_WORDS];
    for (int k2 = 0; k2 < CRC_SHIFT_WORDS; ++k2)
        X[k2] = crc_shift_table_entry(k2);
    const uint32_t part_shift = crc_shift(X, 0x80000000u, CRC_PART); // x^(8 CRC_PART) (bit 31 = x^0): one product per whole part
    uint32_t reg = st.crc, isz = st.isize;
    size_t pi = 0;
    for (size_t m = 0; m <= ends.size(); ++m) {
        for (; pi < parts.size() && part_member[pi] == (int)m; ++pi) {
            reg = (parts[pi].len == CRC_PART ? gf2_mul(part_shift, reg) : crc_shift(X, reg, parts[pi].len)) ^ regs[pi];
            isz += parts[pi].len;
        }
        if (m == ends.size())
            break;
        const uint8_t *t = comp + trailers[m];
        if (~reg != rd32(t)) {
            co.err = E_CRC;
            co.err_at = trailers[m];
            return 0;
        }
        if (isz != rd32(t + 4)) {
            co.err = E_ISIZE;
            co.err_at = trailers[m];
            return 0;
        }
        reg = 0xFFFFFFFFu;
        isz = 0;
        ++cs.members;
    }
    st.crc = reg;
    st.isize = isz;
    st.hist = hist;
    if (co.stream_end) {
        st.bit = 0;
        st.mode = M_HEADER;
    } else {
        st.bit = (uint32_t)(fin.end_bit & 7u);
        st.mode = fin.end_mode;
    }
    return 0;
}

// ---- the CPU backend (tests; the same lane functions, one after the other)
struct CpuBackend {
    double ratio = 4.0;
    const uint8_t *in = nullptr; // the window, padded
    uint32_t n_pad = 0;
    uint64_t n = 0;
    std::vector<std::vector<uint16_t>> arena;
    std::vector<uint8_t> window = std::vector<uint8_t>(WIN, 0); // the stream's window (the last `hist` bytes are real)
    std::vector<uint8_t> win, out;
    std::vector<uint16_t> prim = std::vector<uint16_t>(kmm_gz::PRIM_WORDS), sec = std::vector<uint16_t>(kmm_gz::SEC_WORDS);

    uint16_t *alloc_syms(size_t k)
    {
        arena.emplace_back(k, (uint16_t)0);
        return arena.back().data();
    }
    bool find(const uint8_t *, uint64_t, uint64_t S8, uint32_t c0, uint32_t n_cand, uint64_t *starts)
    {
        for (uint32_t c = 0; c < n_cand; ++c) {
            const uint64_t a = (uint64_t)(c0 + c) * S8, e = a + S8 < n * 8u ? a + S8 : n * 8u;
            starts[c] = NPOS;
            for (uint64_t at = a; at < e; ++at)
                if (header_at(in, n_pad, n, at, prim.data(), sec.data())) {
                    starts[c] = at;
                    break;
                }
        }
        return true;
    }
    bool decode(const Work *w, Result *r, size_t k)
    {
        for (size_t i = 0; i < k; ++i)
            decode_lane(in, n_pad, n, w[i], r[i], prim.data(), sec.data());
        return true;
    }
    bool windows(const MapRef *maps, uint32_t n_chunks, uint32_t G)
    {
        const uint32_t n_groups = (n_chunks + G - 1) / G;
        std::vector<uint16_t> gmaps((size_t)n_groups * WIN), cur(WIN), v(WIN);
        for (uint32_t g = 0; g < n_groups; ++g) { // k_gz_compose
            const uint32_t j0 = g * G, j1 = j0 + G < n_chunks ? j0 + G : n_chunks;
            memcpy(cur.data(), maps[j0].map, WIN * 2);
            for (uint32_t j = j0 + 1; j < j1; ++j) {
                for (uint32_t i = 0; i < WIN; ++i)
                    v[i] = compose_sym(maps[j].map[i], cur.data());
                cur.swap(v);
            }
            memcpy(&gmaps[(size_t)g * WIN], cur.data(), WIN * 2);
        }
        std::vector<uint8_t> gwin((size_t)n_groups * WIN), w(window), wv(WIN);
        for (uint32_t g = 0; g < n_groups; ++g) { // k_gz_chain
            memcpy(&gwin[(size_t)g * WIN], w.data(), WIN);
            for (uint32_t i = 0; i < WIN; ++i)
                wv[i] = resolve_sym(gmaps[(size_t)g * WIN + i], w.data());
            w.swap(wv);
        }
        win.assign((size_t)n_chunks * WIN, 0);
        for (uint32_t g = 0; g < n_groups; ++g) { // k_gz_fix
            const uint32_t j0 = g * G, j1 = j0 + G < n_chunks ? j0 + G : n_chunks;
            memcpy(w.data(), &gwin[(size_t)g * WIN], WIN);
            for (uint32_t j = j0; j < j1; ++j) {
                memcpy(&win[(size_t)j * WIN], w.data(), WIN);
                for (uint32_t i = 0; i < WIN; ++i)
                    wv[i] = resolve_sym(maps[j].map[i], w.data());
                w.swap(wv);
            }
            if (j1 == n_chunks)
                window = w;
        }
        return true;
    }
    bool resolve(const PieceRef *p, size_t k, uint64_t *bad)
    {
        uint64_t need = 0;
        for (size_t i = 0; i < k; ++i)
            need = p[i].off + p[i].n > need ? p[i].off + p[i].n : need;
        out.assign(need, 0);
        *bad = 0;
        for (size_t i = 0; i < k; ++i)
            for (uint32_t x = 0; x < p[i].n; ++x) {
                const uint16_t s = p[i].sym[x];
                *bad += s >= 256u && (s & 0x7FFFu) < p[i].floor;
                out[p[i].off + x] = resolve_sym(s, &win[(size_t)p[i].chunk * WIN]);
            }
        return true;
    }
    bool crc(const Part *p, size_t k, uint32_t *regs)
    {
        static std::vector<uint32_t> T;
        if (T.empty()) {
            T.resize(8 * 256);
            for (int kk = 0; kk < 8; ++kk)
                for (uint32_t bb = 0; bb < 256u; ++bb)
                    T[(size_t)kk * 256 + bb] = kmm_gz::crc_table_entry(kk, bb);
        }
        for (size_t i = 0; i < k; ++i)
            regs[i] = kmm_gz::crc_register(T.data(), out.data() + p[i].off, p[i].len, 0u);
        return true;
    }
};

} // namespace kmm_gunzip
