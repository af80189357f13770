// kmm_radix_plan.hpp — part of libkmm (MI355X / gfx950); included by kmm_radix.hpp.
// The decisions of the radix path that are plain integer arithmetic, each stated once: the fan-out of an index (RxGeometry),
// the scratch layout of a sub-batch (RxScratch), the split of a batch into sub-batches, which pass-3 kernel runs
// (RxP3Variant), the bytes of the radix view, the batch size where the radix path takes over, and the bit a k-mer tests in
// pass 2's slot filter (rx_filter_slot: host, kernels and tests share the one definition), the fingerprint byte pass 3 keeps of
// every LDS-resident entry and the test of a bucket's bytes against it (rx_p3_fp, rx_p3_candidates).  Standard C++17: no HIP
// header, no kmm_index — tests/test_radix_plan_on_the_cpu.py, tests/test_radix_filter_slots_on_the_cpu.py and
// tests/test_radix_p3_fp_on_the_cpu.py compile it by themselves with g++.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>

constexpr int RX_B = 8192;            // positions per pass-1 block = k-mer capacity of a block area / item: each
                                      // 256-thread half of the workgroup owns 4096 of them (flat reads: one tile of
                                      // 16 windows per lane; records mode: four tiles of 4 windows per lane)
constexpr int RX_MAXF = 512;          // largest fan-out of one pass (512 x 512 slices of 8192 buckets = every modulo < 2^32)
#ifndef RX_CHV
#define RX_CHV 256
#endif
constexpr int RX_CH = RX_CHV;            // blocks per chunk of the directory scan
constexpr int RX_IC = 1024;           // pass-2 items per pass-3 work item
constexpr int RX_ECAP = 4096;         // entries of a fine partition kept in LDS (keys + counters)
constexpr int RX_ECAP_BIG = 8192;     // slices of 8192 buckets (modulo 452 930 477): 140 KB of LDS, one workgroup of pass 3 per CU
constexpr int RX_ECAP_MID = 4608;     // 8192-bucket slices at load factor 0.5 (4096 +- 64 entries): 16-bit directory, 1024-piece
                                      // list, 77 KB of LDS: two workgroups per CU (the 1 B-k-mer index)
constexpr int P2F_KMAX = 64;             // most items per work unit (rx.p2f_k: chosen per batch, rx_view_of)
constexpr int P2F_LOGBITS = 19;          // buckets per coarse partition the LDS bitmap covers: 2^19 (64 KB)
constexpr int P2F_SLOT_WORDS = 3 << (P2F_LOGBITS - 6); // 32-bit words of the slot filter of one coarse partition: 3 bits per
                                         // bucket PAIR, 3 x 2^18 bits = 96 KB (rx_filter_slot)
constexpr int P2F_SLOTS = 5888;          // k-mers k_rx_p2f's sort buffer holds beside the slot filter (even; an item with more
                                         // survivors than that — 72 % of its k-mers — is placed and copied out in rounds).
                                         // 96 KB + 46 KB + 17.3 KB of tables (fan-outs beyond 128: with the scan's table of
                                         // bases) = 163 120 of the 163 840 bytes a workgroup may declare; 6144 would not fit

// Pass 2's slot filter, for coarse partitions of exactly 2^P2F_LOGBITS buckets at one bit per bucket (RxGeometry::slot_filter).
// The bucket bitmap spends 2 bits per entry at load factor 0.5 and passes 1 - e^-0.5 = 39.3 % of the absent k-mers.  Keyed by
// the k-mer as well it does better with the same kind of test: every pair of buckets shares 3 bits, an entry sets the one
// its (bucket parity, quotient) selects, and an absent k-mer passes only where an entry of its bucket pair chose the same
// bit: 1 - e^-1/3 = 28.3 %.  No false negatives: an entry and a k-mer equal to it have the same bucket and quotient.
//   b: bucket inside the coarse partition (sh = w + f2 bits); quot: the quotient part of the packed form (x >> sh; any
//   64-bit value).  Returns the bit index in [0, 3 x 2^(sh - 1)).
// Full-rate operations only (a 32-bit multiply is quarter rate, and pass 2 is as much bound by its vector ALUs as by anything):
// the quotient folded to 24 bits, the parity xored into bit 23, a 24-bit multiplicative mix (v_mul_u32_u24) whose bits
// [16, 32) — every one of the 24 input bits reaches the upper ones — are mapped to 0 .. 2 with a second 24-bit multiply.
// Nine vector instructions per k-mer in k_rx_p2f, where sh is a constant and the quotient has 45 bits.
constexpr uint32_t rx_filter_slot(uint32_t b, uint64_t quot)
{
    const uint32_t v = ((uint32_t)quot ^ (uint32_t)(quot >> 24) ^ (uint32_t)(quot >> 48)) + (b << 23); // (+: one v_lshl_add_u32;
                                                                       // below bit 24 it is the xor: b << 23 has no lower bits)
    const uint32_t h16 = ((v & 0xFFFFFFu) * 0x9E3779u) >> 16;
    return 3u * (b >> 1) + ((h16 * 3u) >> 16);
}

// Pass 3's fingerprints.  Beside the 8-byte key of every LDS-resident entry k_rx_p3 keeps ONE byte of it, and a probe reads
// the bytes of its bucket's first five entries (two aligned 32-bit words) instead of their keys: only entries whose byte equals
// the k-mer's are compared in full, so an absent k-mer — more than half of what reaches pass 3 — reads a key once in 256
// entries, and the wavefront's trips over the entries follow the candidates, not the longest bucket.
//   quot: the quotient part of the packed form (x >> (w + f2)): the bits below are the bucket (constant inside a slice) and
//   the fine partition.  The same 24-bit fold as rx_filter_slot, another odd multiplier, bits [16, 24) of the 24-bit
//   product: full-rate operations, and independent of the bit the slot filter tested (every k-mer that reaches pass 3 passed
//   that test; tests/test_radix_p3_fp_on_the_cpu.py holds the false-candidate rate to 1/256).
// The kernel works on the byte in all four bytes of a word (rx_p3_fp4) and on masks with one bit per BYTE (rx_p3_match4,
// rx_p3_match_entry4); rx_p3_candidates states the same test with one bit per entry, for the tests.  On the device the
// multiply is spelled v_mul_u32_u24 — of a product whose bits [16, 24) alone are used the compiler drops the 24-bit mask and
// then takes the quarter-rate 32-bit multiply — and the byte is spread with one v_perm_b32.
#if defined(__HIPCC__)
#define RX_PLAN_HD __host__ __device__
#else
#define RX_PLAN_HD
#endif
constexpr int RX_P3_FP_ENTRIES = 5; // entries of a bucket tested by fingerprint; the ones behind them are walked key by key

RX_PLAN_HD inline uint32_t rx_p3_fp4(uint64_t quot)
{
    const uint32_t v = (uint32_t)quot ^ (uint32_t)(quot >> 24) ^ (uint32_t)(quot >> 48);
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t h = __umul24(v, 0xB5297Bu);
    return __builtin_amdgcn_perm(h, h, 0x02020202u); // byte 2 of the product in every byte
#else
    return (((v & 0xFFFFFFu) * 0xB5297Bu >> 16) & 0xFFu) * 0x01010101u;
#endif
}
RX_PLAN_HD inline uint32_t rx_p3_fp(uint64_t quot) { return rx_p3_fp4(quot) & 0xFFu; }

// lo: the fingerprint bytes of the bucket's entries 0 .. 3 (byte j = entry j); fp4: the k-mer's, in every byte; cn: entries
// of the bucket.  Returns bit 8 j for every entry j < min(cn, 4) whose byte equals the k-mer's.  The key compare stays the
// arbiter: a spurious bit costs one compare, a MISSING bit would be a wrong count.  The SWAR zero-byte test
// (x - 0x01..01) & ~x & 0x80..80 marks every zero byte; it may also mark a byte 0x01 above a marked one (the borrow), never
// drop one.  (The width of the last step is at most 31: bit 24, entry 3, lies below it.)
RX_PLAN_HD inline uint32_t rx_p3_match4(uint32_t lo, uint32_t fp4, uint32_t cn)
{
    const uint32_t x = lo ^ fp4;
    const uint32_t z = ((x - 0x01010101u) & ~x & 0x80808080u) >> 7;
    const uint32_t width = 8u * cn < 31u ? 8u * cn : 31u;
    return z & ((1u << width) - 1u);
}
// hi: the word whose byte 0 belongs to entry 4.  Bit 31 if the bucket has that entry and its byte equals the k-mer's.
// ((x - 1) & ~x: the bits below the lowest set one; bit 7 is among them iff byte 0 is zero.)
RX_PLAN_HD inline uint32_t rx_p3_match_entry4(uint32_t hi, uint32_t fp4, uint32_t cn)
{
    const uint32_t x = hi ^ fp4;
    return cn >= (uint32_t)RX_P3_FP_ENTRIES ? ((x - 1u) & ~x & 0x80u) << 24 : 0u;
}
// The entry the lowest bit of such a mask (not 0) stands for: bits 0, 8, 16, 24, 31 -> 0 .. 4.
RX_PLAN_HD inline uint32_t rx_p3_first_entry(uint32_t m) { return ((uint32_t)__builtin_ctz(m) + 1u) >> 3; }

// f: the 64-bit window of fingerprint bytes that starts at the bucket's first entry (byte j = entry j); fp: the k-mer's;
// cn: entries of the bucket.  Returns the mask (bit j = entry j) of the entries below min(cn, 5) whose byte equals fp.
RX_PLAN_HD inline uint32_t rx_p3_candidates(uint64_t f, uint32_t fp, uint32_t cn)
{
    const uint32_t fp4 = fp * 0x01010101u;
    uint32_t m = rx_p3_match4((uint32_t)f, fp4, cn) | rx_p3_match_entry4((uint32_t)(f >> 32), fp4, cn), out = 0;
    for (; m; m &= m - 1u)
        out |= 1u << rx_p3_first_entry(m);
    return out;
}

// ------------------------------------------------------------------------------------------------
// Geometry: 2^w buckets per fine partition, F2 = 2^f2 fine partitions per coarse one, F1 coarse partitions
// ------------------------------------------------------------------------------------------------
struct RxGeometry {
    int w = 12, f2 = 0;      // log2 buckets per fine partition, log2 fine partitions per coarse one
    int occ_shift = 0;       // k_rx_p2f folds 2^occ_shift buckets into one bit of its LDS bitmap
    bool slot_filter = false; // coarse partitions of 2^P2F_LOGBITS buckets at one bit per bucket: the slot filter applies
    uint32_t PF = 1, F1 = 1, F2 = 1;
};

// Fan-out of the radix path for 2^w buckets per fine partition: F1 coarse x F2 fine partitions, each at most `maxf`
// (<= RX_MAXF = 512: 512 x 512 slices of 8192 buckets cover every modulo the index format's int32 tables allow,
// mapper.pyx:22-23,31-32).  S: entries of the index (0: unknown, load factor 0.5 assumed); filter: the fan-out is chosen for
// pass 2's empty-bucket filter; f2_force >= 0 (experiments, KMM_RX_F2 / "fine_bits"): that many fine-partition bits.
// No value: the configuration is refused.
inline std::optional<RxGeometry> rx_geometry(uint64_t modulo, uint64_t S, bool filter, int w, int maxf = RX_MAXF, int f2_force = -1)
{
    if (w < 0 || w > 13 || modulo == 0 || modulo >= (1ull << 31)) // (pass 1 divides with a 32-bit remainder)
        return std::nullopt;
    const uint64_t PF = (modulo + (1ull << w) - 1) >> w;
    if (PF > (uint64_t)maxf * maxf)
        return std::nullopt;
    int lg = 0;
    while ((1ull << lg) < PF)
        ++lg;
    int f2 = (lg + 1) / 2;
    bool for_filter = false;
    // pass 2's empty-bucket filter has 2^19 bits of LDS per coarse partition: take fewer fine-partition bits — more,
    // smaller coarse partitions — when pass 1's fan-out stays within 512; tables too large for that at one bit per
    // bucket get one bit per 2 or 4 buckets (sparse tables such as modulo 452 930 477 with 1e8 entries still lose
    // half of their k-mers there; at load factor 0.5 a bit per 4 buckets would pass 86 %: not taken)
    if (filter && w + f2 > P2F_LOGBITS) {
        const double load = S ? (double)S / (double)modulo : 0.5;
        for (int gs = 0; gs <= 2 && !for_filter; ++gs) {
            const int fb = P2F_LOGBITS + gs - w;
            if (fb < 0 || load * (double)(1 << gs) > 0.75)
                continue;
            if (((PF + (1ull << fb) - 1) >> fb) <= (uint64_t)RX_MAXF && fb <= 9) {
                f2 = fb;
                for_filter = true;
            }
        }
    }
    if (f2_force >= 0)
        f2 = f2_force;
    // the packed form (kmm_radix.hpp) keeps floor(q / modulo) above w + f2 hash bits: it must fit for EVERY
    // 64-bit q (callers may hand over arbitrary uint64 values), else give the quotient more room
    const uint64_t max_quo = ~0ull / modulo;
    auto fits = [&](int sh) { return sh == 0 || (sh < 64 && (max_quo >> (64 - sh)) == 0); };
    while (f2 > 0 && !fits(w + f2))
        --f2;
    if (!fits(w + f2))
        return std::nullopt;
    const uint64_t F2 = 1ull << f2, F1 = (PF + F2 - 1) / F2;
    if (F2 > (uint64_t)maxf || F1 > (uint64_t)(for_filter ? RX_MAXF : maxf))
        return std::nullopt;
    RxGeometry g;
    g.w = w;
    g.f2 = f2;
    g.occ_shift = w + f2 > P2F_LOGBITS ? w + f2 - P2F_LOGBITS : 0; // (the filter's bits never outnumber its LDS;
                                                                   // rx_filter_active refuses more than 2)
    g.slot_filter = w + f2 == P2F_LOGBITS; // (then occ_shift = 0)
    g.PF = (uint32_t)PF;
    g.F1 = (uint32_t)F1;
    g.F2 = (uint32_t)F2;
    return g;
}

// The geometry an index gets at creation.  2^w buckets per fine partition: as many as keep a slice's entries (load
// factor x 2^w) well inside the LDS key capacity; fewer when the table is dense.  w_force with a value / f2_force >= 0
// (experiments / tests, KMM_RX_W / KMM_RX_F2): the slice width, taken as it is and refused if no kernel serves it / the
// fine-partition bits.
// Fan-out, in order of preference (runs between the passes get shorter, then pass 3 loses its second workgroup
// per CU): up to 256 x 256 slices of 2^w buckets; 256 x 256 slices of 8192 buckets whose entries fit 4096 keys
// (16-bit LDS directory, two workgroups of pass 3 per CU); up to 512 x 512 slices of 4096 buckets; slices of 8192
// buckets with up to 8192 keys (one workgroup of pass 3 per CU), 256 x 256, then 512 x 512: every modulo below
// 2^31 is covered as long as the load factor lets a slice's entries fit LDS.
inline std::optional<RxGeometry> rx_choose_geometry(uint64_t modulo, uint64_t S, bool filter, std::optional<int> w_force = std::nullopt,
                                                    int f2_force = -1)
{
    const bool w_forced = w_force.has_value();
    const double load = (double)S / (double)modulo;
    int w = 12;
    if (w_forced)
        w = *w_force;
    else
        while (w > 0 && (load * (double)(1u << w) * 1.3 + 64.0 > (double)RX_ECAP || (1ull << w) > modulo))
            --w;
    const bool fits13_small = load * 8192.0 * 1.3 + 64.0 <= (double)RX_ECAP;
    const bool fits13 = load * 8192.0 * 1.3 + 64.0 <= (double)RX_ECAP_BIG;
    auto conf = [&](int w_, int maxf) { return rx_geometry(modulo, S, filter, w_, maxf); };
    std::optional<RxGeometry> g = rx_geometry(modulo, S, filter, w, f2_force >= 0 ? RX_MAXF : 256, f2_force);
    if (!g && w == 12 && !w_forced) {
        if (fits13_small)
            g = conf(13, 256);
        if (!g)
            g = conf(12, RX_MAXF);
        if (!g && fits13 && !(g = conf(13, 256)))
            g = conf(13, RX_MAXF);
    } else if (!g) {
        g = conf(w, RX_MAXF);
    }
    return g;
}

// ------------------------------------------------------------------------------------------------
// Scratch of one sub-batch of NB pass-1 blocks: where every table of RxView lies in the handle's meta buffer, and how
// large the two k-mer buffers are.  Every table grows with NB (or not at all), so the layout of the largest sub-batch
// sizes the buffers for all of them.
// ------------------------------------------------------------------------------------------------
struct RxScratch {
    uint32_t chunks;    // directory-scan chunks of RX_CH blocks
    size_t max_items;   // pass-2 items: at most one partly filled item per coarse partition beside the full ones
    size_t start1, P1T, S1T, csum, T1, item_base, work_base, item_desc, start2, start2T, ctrl, queue; // byte offsets, 256-aligned
    size_t meta_bytes;  // all of the above; [ctrl, meta_bytes) is cleared before every sub-batch
    size_t buf1_bytes, buf2_bytes; // pass 1's block areas, pass 2's items
};

constexpr size_t rx_align256(size_t x) { return (x + 255) & ~(size_t)255; }

inline RxScratch rx_scratch(uint32_t NB, uint32_t F1, uint32_t F2)
{
    RxScratch s;
    s.chunks = (NB + RX_CH - 1) / RX_CH;
    s.max_items = (size_t)NB + F1 + 1;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += rx_align256(bytes); return o; };
    s.start1 = carve((size_t)NB * (F1 + 1) * 2);            // uint16 [NB][F1 + 1]
    s.P1T = carve((size_t)F1 * ((size_t)NB + 1) * 4);       // uint32 [F1][NB + 1] (k_rx_p2 only: unused in front of k_rx_p2f)
    s.S1T = carve((size_t)F1 * NB * 2);                     // uint16 [F1][NB]
    s.csum = carve((size_t)s.chunks * F1 * 4);              // uint32 [chunks][F1]
    s.T1 = carve((size_t)F1 * 4);                           // uint32 [F1]
    s.item_base = carve((size_t)(F1 + 1) * 4);              // uint32 [F1 + 1]
    s.work_base = carve((size_t)(F1 + 1) * 4);              // uint32 [F1 + 1]
    s.item_desc = carve(s.max_items * 8);                   // uint2  [max_items]
    s.start2 = carve(s.max_items * (F2 + 1) * 2);           // uint16 [max_items][F2 + 1]
    s.start2T = carve(s.max_items * (F2 + 1) * 2 + 256);    // uint16 [F2 + 1][max_items] (+ k_rx_tr2's last tile)
    s.ctrl = carve(64);                                     // uint32 [3]
    s.queue = carve(2048);                                  // 2 x 8 work counters, 128 bytes apart
    s.meta_bytes = off;
    s.buf1_bytes = (size_t)NB * RX_B * 8;
    s.buf2_bytes = s.max_items * RX_B * 8;
    return s;
}

// ------------------------------------------------------------------------------------------------
// Sub-batches.  Every sub-batch streams the index slices once (pass 3) and pays the per-work-item costs once, so they
// are as large as the 32-bit prefixes allow: a coarse partition's k-mers are numbered with 32 bits and in the worst
// case (one k-mer repeated) ALL of a sub-batch's k-mers fall into one coarse partition, hence fewer than 2^32 k-mer
// slots per sub-batch (r03: 2^31; the 1 B-k-mer index streamed its 14 GB of slices twice per 28 M-read batch).  Every
// other offset is 64-bit or relative (to a table's first block, to a work item's first item).
// ------------------------------------------------------------------------------------------------
constexpr int64_t RX_SUB_CAP_MAX = ((int64_t)1 << 32) - 2 * RX_B; // k-mer slots per sub-batch ("radix_sub_batch_kmers")
constexpr int64_t RX_SUB_CAP_FLOOR = (int64_t)1 << 28;            // an out-of-memory call shrinks its sub-batches down to this
constexpr int RX_SUB_CAP_AGE = 16; // calls after which a handle that settled on a smaller size tries the caller's cap again

struct RxSplit {
    int64_t n_sub, max_src; // sub-batches of equal size (no small last one): source blocks of each
};

// n_src_total source blocks, X output blocks per source block (2 with reverse complements), at most `cap` k-mer slots.
inline RxSplit rx_split(int64_t n_src_total, uint32_t X, int64_t cap)
{
    const int64_t cap_src = (cap / RX_B) / X > 0 ? (cap / RX_B) / X : 1;
    RxSplit s;
    s.n_sub = (n_src_total + cap_src - 1) / cap_src;
    s.max_src = s.n_sub ? (n_src_total + s.n_sub - 1) / s.n_sub : cap_src;
    return s;
}

// The next size that really is smaller than an attempt with n_sub sub-batches: one sub-batch more, not below the floor.
inline int64_t rx_next_smaller_cap(int64_t n_src_total, uint32_t X, int64_t n_sub)
{
    const int64_t next_src = (n_src_total + n_sub) / (n_sub + 1);
    const int64_t cap = next_src * RX_B * X;
    return cap < RX_SUB_CAP_FLOOR ? RX_SUB_CAP_FLOOR : cap;
}

// ------------------------------------------------------------------------------------------------
// Pass 3: which instantiation of k_rx_p3 runs
// ------------------------------------------------------------------------------------------------
enum class RxP3Variant {
    W12_DIR16,       // slices of up to 4096 buckets (the usual case): 16-bit directory loaded as it is
    W12,             // ... without the 16-bit directory (a slice beyond 65535 entries, or no HBM for it)
    W13_SMALL_DIR16, // 8192-bucket slices whose entries all fit 4096 keys: 16-bit directory, two workgroups per CU
    W13_SMALL,
    W13_MID_DIR16,   // ... at most 4608 keys (load factor 0.5): the same with a shorter piece list
    W13_MID,
    W13_BIG,         // 8192 keys, 32-bit LDS directory, one workgroup per CU
};
struct RxP3Shape {
    int keys_in_lds;   // entries of a slice kept in LDS (the rest is walked in HBM)
    int wg_per_cu;
    bool dir16;        // the slice's directory is loaded from RxView::pstart16
    bool fingerprints = false; // the kernel has the fingerprint form of the probe (rx_p3_fp): only where one byte per key more
                               // still leaves LDS for two workgroups per CU — 71 776 + 4 104 B; W12 (79 968 B) and the
                               // 8192-bucket variants do not fit and keep the plain entry loop
};
constexpr RxP3Shape RX_P3_SHAPES[] = {
    {RX_ECAP, 2, true, true}, {RX_ECAP, 2, false},   // W12_DIR16, W12
    {RX_ECAP, 2, true}, {RX_ECAP, 2, false},         // W13_SMALL_DIR16, W13_SMALL
    {RX_ECAP_MID, 2, true}, {RX_ECAP_MID, 2, false}, // W13_MID_DIR16, W13_MID
    {RX_ECAP_BIG, 1, false},                         // W13_BIG
};
constexpr const RxP3Shape &rx_p3_shape(RxP3Variant v) { return RX_P3_SHAPES[(int)v]; }
constexpr int rx_p3_fp_shapes()
{
    int n = 0;
    for (const RxP3Shape &s : RX_P3_SHAPES)
        n += s.fingerprints ? 1 : 0;
    return n;
}

// fits_small / fits_mid: all but one slice in 1000 hold at most RX_ECAP / RX_ECAP_MID entries; p16: the 16-bit directory
// exists (implies max_slice <= 65535); no_mid (experiments, KMM_RX_NO_MID): the 4608-key variants are not used.
inline RxP3Variant rx_choose_p3(int w, bool fits_small, bool fits_mid, bool p16, uint32_t max_slice, bool no_mid)
{
    if (w <= 12)
        return p16 ? RxP3Variant::W12_DIR16 : RxP3Variant::W12;
    const bool lds16 = p16 || max_slice <= 65535u; // a 16-bit LDS directory holds every slice
    if (fits_small && lds16)
        return p16 ? RxP3Variant::W13_SMALL_DIR16 : RxP3Variant::W13_SMALL;
    if (fits_mid && lds16 && !no_mid)
        return p16 ? RxP3Variant::W13_MID_DIR16 : RxP3Variant::W13_MID;
    return RxP3Variant::W13_BIG;
}

// ------------------------------------------------------------------------------------------------
// The radix view of the index (rx_build): bytes per entry of each of its arrays, and their sum
// ------------------------------------------------------------------------------------------------
struct RxViewBytes {
    enum : size_t { pstart = 4, pkeys = 8, pkeys_raw = 8, pfreq = 2, pnodes = 4, porig = 4, ecnt = 4, norder = 4, nnode = 4 };
};
// ("radix_view_bytes": the bucket directory + the arrays of max(S, 1) entries; node_order: with the node-ordered entry list)
constexpr size_t rx_view_bytes(uint64_t modulo, uint64_t S, bool node_order)
{
    return (size_t)(modulo + 1) * RxViewBytes::pstart +
           (size_t)(S ? S : 1) * (RxViewBytes::pkeys + RxViewBytes::pkeys_raw + RxViewBytes::pfreq + RxViewBytes::pnodes +
                                  RxViewBytes::porig + RxViewBytes::ecnt + (node_order ? RxViewBytes::norder + RxViewBytes::nnode : 0));
}

// auto: the radix path streams the whole directory + key arrays once per batch (4 B x modulo + 14 B x entries) and
// then costs ~6.5 ps per k-mer (10 ps at the 1 B-k-mer index: shorter runs); the direct kernel has no fixed cost and
// runs at ~60 G k-mers/s below ~1 GB of index, ~38 G above.  The batch size where the two meet
// (profiles/r03/path_crossover.txt: 16-20 M positions at the 10 M index, ~52 M at the 100 M index; units are
// base positions, 1.25 per k-mer at 150 bp); at least 2^22.
inline int64_t rx_min_units(uint64_t modulo, uint64_t S)
{
    const double bytes = (double)modulo * 4.0 + (double)S * 14.0;
    const double fixed = 50e-6 + bytes / 2.6e12;
    const double per_kmer_radix = 6.5e-12 * (1.0 + bytes / 40e9);
    const double per_kmer_direct = 1.0 / (bytes < 1e9 ? 60e9 : 38e9);
    const int64_t units = (int64_t)(1.25 * fixed / (per_kmer_direct - per_kmer_radix));
    return units < ((int64_t)1 << 22) ? (int64_t)1 << 22 : units;
}
