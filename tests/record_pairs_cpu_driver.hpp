// CPU driver of the plain-C++ arithmetic of keeping mates together (tests/test_record_pairs_on_the_cpu.py,
// tests/record_pairs_san_main.cpp): csrc/kmm_record_keep.hpp and csrc/kmm_line_search.hpp compiled by themselves with g++ and
// walked the way the pair forms of the kernels walk a piece.  Stage A is the pair form of k_rk_flags — a lane takes 16
// consecutive bytes, its keep mask comes from rk_lane_mask with the keep_of of rk_lane_front<PAIR>: the two entries of pair
// record >> pair_shift under rk_pair_keep; stage B is the scatter of tests/record_keep_cpu_driver.hpp, unchanged (tiles, groups
// of four, rk_span stores, every store checked).  The cut search walks super-tiles, tiles and bytes as k_rec_cut does.
#pragma once
#include "record_keep_cpu_driver.hpp"

#include "kmm_line_search.hpp"

// The keep_of of rk_lane_front<PAIR>: pair_shift = PAIR - 1; hits / windows: two entries per pair; n_records: records of the
// buffer (whole pairs only).
struct PairKeepOf {
    const uint32_t *hits, *windows;
    int64_t n_records;
    uint32_t pair_shift;
    RkPairRule rule;
    int64_t *asked_behind;
    bool operator()(uint32_t r) const
    {
        if ((int64_t)r >= n_records) {
            ++*asked_behind;
            return false;
        }
        const size_t e = 2 * (size_t)rk_pair_of_record(r, pair_shift);
        return rk_pair_keep(hits[e], windows ? windows[e] : 0u, hits[e + 1], windows ? windows[e + 1] : 0u, rule.rule, rule.pair_rule);
    }
};

extern "C" int record_pairs_rule_cpu(uint32_t h1, uint32_t w1, uint32_t h2, uint32_t w2, uint32_t min_hits, uint32_t min_permille,
                                     uint32_t invert, uint32_t pair_rule)
{
    const RkRule rule = {min_hits, min_permille, invert};
    return rk_pair_keep(h1, w1, h2, w2, rule, pair_rule) ? 1 : 0;
}

// The whole piece: text[0, n) starts at a pair's first record (pair_shift 1) or is one mate's buffer (pair_shift 0).
// stats: {kept_bytes, kept_records, outside, twice-or-missed, asked_behind}.
extern "C" int record_pairs_cpu(const uint8_t *text, int64_t n, int64_t consumed, uint32_t period_shift, uint32_t pair_shift,
                                const uint32_t *hits, const uint32_t *windows, int64_t n_records, uint32_t min_hits, uint32_t min_permille,
                                uint32_t invert, uint32_t pair_rule, int64_t tail, uint8_t *out, int64_t cap, int64_t *stats)
{
    RecordKeepStats st = {0, 0, 0, 0, 0};
    const PairKeepOf keep_of = {hits, windows, n_records, pair_shift, {{min_hits, min_permille, invert}, pair_rule}, &st.asked_behind};
    const uint32_t period_mask = (1u << period_shift) - 1u;
    const int64_t n_lanes = (n + 15) / 16;
    std::vector<uint16_t> masks((size_t)n_lanes, 0);
    uint32_t line0 = 0;
    for (int64_t l = 0; l < n_lanes; ++l) {
        const int64_t p0 = l * 16;
        uint32_t nl = 0;
        for (int j = 0; j < 16 && p0 + j < n; ++j)
            nl |= (text[p0 + j] == 10 ? 1u : 0u) << j;
        const uint32_t mask = rk_lane_mask<16>(line0, nl, period_shift, p0, consumed, keep_of);
        masks[(size_t)l] = (uint16_t)mask;
        st.kept_records += rk_lane_records<16>(line0, nl, period_mask, mask);
        line0 = rh_line_of_byte(line0, nl, 16);
    }
    std::vector<uint8_t> written((size_t)cap, 0);
    record_keep_scatter(text, n, masks, tail, out, cap, written, st);
    st.twice += record_keep_check(written, tail, st.kept_bytes);
    stats[0] = st.kept_bytes; stats[1] = st.kept_records; stats[2] = st.outside; stats[3] = st.twice; stats[4] = st.asked_behind;
    return 0;
}

// The brute force: every byte by itself, its record from the newlines in front of it, the pair rule spelled out.
extern "C" int64_t record_pairs_brute(const uint8_t *text, int64_t consumed, uint32_t period_shift, uint32_t pair_shift, const uint32_t *hits,
                                      const uint32_t *windows, uint32_t min_hits, uint32_t min_permille, uint32_t invert, uint32_t pair_rule,
                                      uint8_t *out, int64_t *kept_records)
{
    int64_t line = 0, at = 0;
    *kept_records = 0;
    for (int64_t p = 0; p < consumed; ++p) {
        const int64_t e = 2 * ((line >> period_shift) >> pair_shift);
        bool m[2];
        for (int i = 0; i < 2; ++i) {
            const unsigned long long h = hits[e + i], w = windows ? windows[e + i] : 0;
            m[i] = h >= min_hits && 1000ull * h >= (unsigned long long)min_permille * w;
        }
        const bool match = pair_rule == 0 ? (m[0] || m[1]) : (m[0] && m[1]);
        if (match != (invert != 0)) {
            out[at++] = text[p];
            if (text[p] == 10 && ((line + 1) & ((1 << period_shift) - 1)) == 0)
                ++*kept_records;
        }
        line += text[p] == 10;
    }
    return at;
}

// One lane by itself, on a newline mask that no text need produce: the mask of rk_lane_mask<16> under the pair keep_of, and
// the same bit by bit.  Returns the two masks in out[0], out[1]; out[2]: keep_of asked for a record behind n_records.
extern "C" int record_pairs_lane_cpu(uint32_t line0, uint32_t nl, uint32_t period_shift, uint32_t pair_shift, int64_t p0, int64_t consumed,
                                     const uint32_t *hits, const uint32_t *windows, int64_t n_records, uint32_t min_hits,
                                     uint32_t min_permille, uint32_t invert, uint32_t pair_rule, uint32_t *out)
{
    int64_t asked = 0;
    const PairKeepOf keep_of = {hits, windows, n_records, pair_shift, {{min_hits, min_permille, invert}, pair_rule}, &asked};
    out[0] = rk_lane_mask<16>(line0, nl, period_shift, p0, consumed, keep_of);
    uint32_t brute = 0;
    for (int j = 0; j < 16; ++j) {
        if (p0 + j >= consumed)
            continue;
        const uint32_t line = line0 + (uint32_t)__builtin_popcount(nl & ((1u << j) - 1u));
        const int64_t rec = line >> period_shift, e = 2 * (rec >> pair_shift);
        if (rec >= n_records)
            continue;
        bool m[2];
        for (int i = 0; i < 2; ++i) {
            const unsigned long long h = hits[e + i], w = windows ? windows[e + i] : 0;
            m[i] = h >= min_hits && 1000ull * h >= (unsigned long long)min_permille * w;
        }
        const bool match = pair_rule == 0 ? (m[0] || m[1]) : (m[0] && m[1]);
        brute |= (match != (invert != 0) ? 1u : 0u) << j;
    }
    out[1] = brute;
    out[2] = (uint32_t)asked;
    return 0;
}

// k_rec_cut as plain C++: the newline census per 1024-byte tile and per super-tile of 1024 tiles (exclusive prefixes, as
// k_rec_scan1 and k_rec_scan2 leave them), then the search of the byte behind the target-th newline through ls_slot_holds on
// the three levels, every slot tested by itself as every thread tests its own.  -1 where no slot holds the target.
extern "C" int64_t record_pairs_cut_cpu(const uint8_t *text, int64_t n, uint32_t target)
{
    const int64_t n_tiles = (n + 1023) / 1024, n_super = (n_tiles + 1023) / 1024;
    std::vector<uint32_t> tile_pre((size_t)n_super * 1024, 0), super_pre((size_t)n_super, 0);
    for (int64_t p = 0; p < n; ++p)
        tile_pre[(size_t)(p / 1024)] += text[p] == 10;
    uint32_t total = 0;
    for (int64_t s = 0; s < n_super; ++s) {
        super_pre[(size_t)s] = total;
        uint32_t run = 0;
        for (int t = 0; t < 1024; ++t) {
            const uint32_t c = tile_pre[(size_t)s * 1024 + t];
            tile_pre[(size_t)s * 1024 + t] = run;
            run += c;
        }
        total += run;
    }
    int64_t sup = -1, tile = -1, cut = -1, found = 0;
    uint32_t rem = 0, super_cnt = 0;
    for (int64_t s = 0; s < n_super; ++s) {
        const uint32_t pre = super_pre[(size_t)s], nxt = s + 1 < n_super ? super_pre[(size_t)s + 1] : total;
        if (ls_slot_holds(pre, nxt, target)) {
            sup = s;
            rem = ls_rank_in_slot(pre, target);
            super_cnt = nxt - pre;
            ++found;
        }
    }
    if (sup < 0)
        return -1;
    for (int t = 0; t < 1024; ++t) {
        const uint32_t pre = tile_pre[(size_t)sup * 1024 + t], nxt = t < 1023 ? tile_pre[(size_t)sup * 1024 + t + 1] : super_cnt;
        if (ls_slot_holds(pre, nxt, rem)) {
            tile = sup * 1024 + t;
            ++found;
        }
    }
    if (tile < 0)
        return -1;
    const uint32_t r = ls_rank_in_slot(tile_pre[(size_t)tile], rem);
    uint32_t seen = 0;
    for (int t = 0; t < 1024; ++t) {
        const int64_t pos = tile * 1024 + t;
        const bool is_nl = pos < n && text[pos] == 10;
        seen += is_nl;
        if (is_nl && seen == r) {
            cut = pos + 1;
            ++found;
        }
    }
    return found == 3 ? cut : -2; // (exactly one slot per level)
}

extern "C" int64_t record_pairs_cut_brute(const uint8_t *text, int64_t n, uint32_t target)
{
    uint32_t seen = 0;
    if (target == 0)
        return -1;
    for (int64_t p = 0; p < n; ++p)
        if (text[p] == 10 && ++seen == target)
            return p + 1;
    return -1;
}
