// CPU driver of the plain-C++ arithmetic of csrc/kmm_record_keep.hpp (tests/test_record_keep_on_the_cpu.py,
// tests/record_keep_san_main.cpp): the header compiled by itself with g++ and walked the way its kernels walk a piece — a lane
// takes 16 consecutive bytes, a tile is 64 lanes, a group four tiles.  Stage A (k_rk_flags): line of every lane from the
// newlines in front, the lane's keep mask from the per-record rule, kept bytes per tile, kept records.  Stage B
// (k_rk_scatter): exclusive prefixes, the group's kept bytes compacted into a staging buffer shifted by the destination's
// offset inside a 16-byte line, the span written as head bytes, whole lines and tail bytes.  Every store is checked: inside
// [tail, tail + kept_total), and no byte twice.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "kmm_record_keep.hpp"

struct RecordKeepStats {
    int64_t kept_bytes, kept_records, outside, twice, asked_behind;
};

// Stage A.  hits / windows: n_records entries.  masks: one 16-bit mask per lane (n_lanes = ceil(n / 16)).
static void record_keep_flags(const uint8_t *text, int64_t n, int64_t consumed, uint32_t period_shift, const uint32_t *hits,
                              const uint32_t *windows, int64_t n_records, const RkRule &rule, std::vector<uint16_t> &masks,
                              RecordKeepStats &st)
{
    const uint32_t period_mask = (1u << period_shift) - 1u;
    const int64_t n_lanes = (n + 15) / 16;
    masks.assign((size_t)n_lanes, 0);
    uint32_t line0 = 0;
    for (int64_t l = 0; l < n_lanes; ++l) {
        const int64_t p0 = l * 16;
        uint32_t nl = 0;
        for (int j = 0; j < 16 && p0 + j < n; ++j)
            nl |= (text[p0 + j] == 10 ? 1u : 0u) << j;
        const uint32_t mask = rk_lane_mask<16>(line0, nl, period_shift, p0, consumed, [&](uint32_t r) {
            if ((int64_t)r >= n_records) {
                ++st.asked_behind; // (a byte before `consumed` lies in a whole record)
                return false;
            }
            return rk_keep(hits[r], windows ? windows[r] : 0u, rule);
        });
        masks[(size_t)l] = (uint16_t)mask;
        st.kept_records += rk_lane_records<16>(line0, nl, period_mask, mask);
        line0 = rh_line_of_byte(line0, nl, 16);
    }
}

// Stage B.  out: cap bytes, the queue; tail: where the piece's bytes start.  written: one counter per byte of out.
static void record_keep_scatter(const uint8_t *text, int64_t n, const std::vector<uint16_t> &masks, int64_t tail, uint8_t *out,
                                int64_t cap, std::vector<uint8_t> &written, RecordKeepStats &st)
{
    const int64_t n_lanes = (int64_t)masks.size(), n_tiles = (n_lanes + 63) / 64, n_super = (n_tiles + 1023) / 1024;
    std::vector<uint32_t> tile_cnt((size_t)n_super * 1024, 0), super_pre((size_t)n_super, 0);
    for (int64_t l = 0; l < n_lanes; ++l)
        tile_cnt[(size_t)(l / 64)] += (uint32_t)__builtin_popcount(masks[(size_t)l]);
    uint32_t total = 0;
    for (int64_t s = 0; s < n_super; ++s) { // (k_rec_scan1 + k_super_scan: exclusive prefixes, per super-tile and over them)
        super_pre[(size_t)s] = total;
        uint32_t run = 0;
        for (int t = 0; t < 1024; ++t) {
            const uint32_t c = tile_cnt[(size_t)s * 1024 + t];
            tile_cnt[(size_t)s * 1024 + t] = run;
            run += c;
        }
        total += run;
    }
    st.kept_bytes = total;
    auto store = [&](int64_t at, uint8_t v) {
        if (at < tail || at >= tail + (int64_t)total || at >= cap) {
            ++st.outside;
            return;
        }
        if (written[(size_t)at]++)
            ++st.twice;
        out[at] = v;
    };
    std::vector<uint8_t> buf(4096 + 16);
    for (int64_t tile0 = 0; tile0 < n_tiles; tile0 += 4) {
        const int64_t dst = rk_dest(tail, super_pre[(size_t)(tile0 >> 10)], tile_cnt[(size_t)tile0], 0u);
        const uint32_t a = (uint32_t)dst & 15u;
        uint32_t o = a;
        for (int64_t l = tile0 * 64; l < (tile0 + 4) * 64 && l < n_lanes; ++l)
            for (int j = 0; j < 16; ++j)
                if ((masks[(size_t)l] >> j) & 1u) {
                    if (o >= buf.size() || l * 16 + j >= n) {
                        ++st.outside;
                        continue;
                    }
                    buf[o++] = text[l * 16 + j];
                }
        const uint32_t len = o - a;
        if (len == 0)
            continue;
        const int64_t g = dst - (int64_t)a;
        const RkSpan sp = rk_span(a, len);
        for (uint32_t i = a; i < sp.head_end; ++i)
            store(g + i, buf[i]);
        for (uint32_t i = sp.full_begin; i + 16u <= sp.full_end; i += 16u) {
            if ((g + i) % 16 != 0)
                ++st.outside; // (a whole line starts at a multiple of 16)
            for (uint32_t b = 0; b < 16u; ++b)
                store(g + i + b, buf[i + b]);
        }
        for (uint32_t i = sp.tail_begin; i < a + len; ++i)
            store(g + i, buf[i]);
    }
}

static int64_t record_keep_check(const std::vector<uint8_t> &written, int64_t tail, int64_t total)
{
    int64_t bad = 0;
    for (int64_t i = 0; i < (int64_t)written.size(); ++i)
        bad += written[(size_t)i] != (i >= tail && i < tail + total ? 1 : 0);
    return bad;
}

// The whole piece.  out: cap bytes, filled from `tail`.  stats: {kept_bytes, kept_records, outside, twice-or-missed, asked_behind}.
extern "C" int record_keep_cpu(const uint8_t *text, int64_t n, int64_t consumed, uint32_t period_shift, const uint32_t *hits,
                               const uint32_t *windows, int64_t n_records, uint32_t min_hits, uint32_t min_permille, uint32_t invert,
                               int64_t tail, uint8_t *out, int64_t cap, int64_t *stats)
{
    const RkRule rule = {min_hits, min_permille, invert};
    RecordKeepStats st = {0, 0, 0, 0, 0};
    std::vector<uint16_t> masks;
    record_keep_flags(text, n, consumed, period_shift, hits, windows, n_records, rule, masks, st);
    std::vector<uint8_t> written((size_t)cap, 0);
    record_keep_scatter(text, n, masks, tail, out, cap, written, st);
    st.twice += record_keep_check(written, tail, st.kept_bytes);
    stats[0] = st.kept_bytes; stats[1] = st.kept_records; stats[2] = st.outside; stats[3] = st.twice; stats[4] = st.asked_behind;
    return 0;
}

// Stage B alone, on lane masks that no text produces (any bits of the bytes before n).
extern "C" int record_keep_scatter_cpu(const uint8_t *text, int64_t n, const uint16_t *lane_masks, int64_t tail, uint8_t *out,
                                       int64_t cap, int64_t *stats)
{
    RecordKeepStats st = {0, 0, 0, 0, 0};
    const std::vector<uint16_t> masks(lane_masks, lane_masks + (n + 15) / 16);
    std::vector<uint8_t> written((size_t)cap, 0);
    record_keep_scatter(text, n, masks, tail, out, cap, written, st);
    st.twice += record_keep_check(written, tail, st.kept_bytes);
    stats[0] = st.kept_bytes; stats[1] = st.kept_records; stats[2] = st.outside; stats[3] = st.twice; stats[4] = st.asked_behind;
    return 0;
}

// The brute force: every byte by itself, its record from the newlines in front of it, the rule spelled out.  Returns the
// kept bytes; *kept_records: the kept records.
extern "C" int64_t record_keep_brute(const uint8_t *text, int64_t consumed, uint32_t period_shift, const uint32_t *hits,
                                     const uint32_t *windows, uint32_t min_hits, uint32_t min_permille, uint32_t invert, uint8_t *out,
                                     int64_t *kept_records)
{
    int64_t line = 0, at = 0;
    *kept_records = 0;
    for (int64_t p = 0; p < consumed; ++p) {
        const int64_t r = line >> period_shift;
        const unsigned long long h = hits[r], w = windows ? windows[r] : 0;
        const bool match = h >= min_hits && 1000ull * h >= (unsigned long long)min_permille * w;
        if (match != (invert != 0)) {
            out[at++] = text[p];
            if (text[p] == 10 && ((line + 1) & ((1 << period_shift) - 1)) == 0)
                ++*kept_records;
        }
        line += text[p] == 10;
    }
    return at;
}
