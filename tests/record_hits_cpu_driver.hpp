// CPU driver of the records arithmetic of csrc/kmm_read_hits.hpp (tests/test_record_hits_on_the_cpu.py,
// tests/record_hits_san_main.cpp): the header compiled by itself with g++, walked the way k_read_hits walks raw records — a
// lane takes LANE consecutive bytes, knows the line of its first byte and the newline mask of its bytes (what the tile front
// end hands it), folds its windows into runs of one record and adds every run to that record's entry.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kmm_read_hits.hpp"

struct RecordHitsOut {
    uint32_t *hits, *windows;
    int64_t n_records, outside;
    void add(uint32_t r, uint32_t h, uint32_t w)
    {
        if (h == 0 && w == 0)
            return; // (the kernel issues no atomic for a run of nothing)
        if ((int64_t)r >= n_records) {
            ++outside;
            return;
        }
        hits[r] += h;
        windows[r] += w;
    }
};

template <int LANE>
static void record_hits_fold_lanes(const uint8_t *text, int64_t n, const uint8_t *masks, uint32_t period_shift, RecordHitsOut &out)
{
    uint32_t line0 = 0;
    for (int64_t p0 = 0; p0 < n; p0 += LANE) {
        uint32_t nl = 0, valid = 0, hit = 0;
        for (int j = 0; j < LANE && p0 + j < n; ++j) {
            nl |= (text[p0 + j] == 10 ? 1u : 0u) << j;
            valid |= (uint32_t)(masks[p0 + j] & 1u) << j;
            hit |= (uint32_t)((masks[p0 + j] >> 1) & masks[p0 + j] & 1u) << j;
        }
        RhRun run;
        rh_fold_records<LANE>(line0, nl, period_shift, valid, hit, run, [&](uint32_t r, uint32_t h, uint32_t w) { out.add(r, h, w); });
        out.add(run.r, run.h, run.w); // (the kernel: the reduction across the wavefront)
        line0 = rh_line_of_byte(line0, nl, LANE);
    }
}

// text[0, n): the consumed bytes of a chunk; masks[p]: bit 0 = a window starts at p, bit 1 = it is a hit; the records have
// 1 << period_shift lines.  hits / windows: uint32[n_records], zeroed by the caller.  Returns the number of runs that named a
// record outside [0, n_records) (must be 0), or -1 for a lane length the driver does not have.
extern "C" int64_t record_hits_fold_cpu(const uint8_t *text, int64_t n, const uint8_t *masks, uint32_t period_shift, int64_t lane,
                                        int64_t n_records, uint32_t *hits, uint32_t *windows)
{
    RecordHitsOut out{hits, windows, n_records, 0};
    switch (lane) {
    case 1: record_hits_fold_lanes<1>(text, n, masks, period_shift, out); break;
    case 2: record_hits_fold_lanes<2>(text, n, masks, period_shift, out); break;
    case 4: record_hits_fold_lanes<4>(text, n, masks, period_shift, out); break;
    case 8: record_hits_fold_lanes<8>(text, n, masks, period_shift, out); break;
    case 16: record_hits_fold_lanes<16>(text, n, masks, period_shift, out); break;
    default: return -1;
    }
    return out.outside;
}

// The brute force: every position by itself, its record from the newlines in front of it.
extern "C" void record_hits_fold_brute(const uint8_t *text, int64_t n, const uint8_t *masks, uint32_t period_shift, uint32_t *hits,
                                       uint32_t *windows)
{
    uint32_t line = 0;
    for (int64_t p = 0; p < n; ++p) {
        const uint32_t r = line >> period_shift;
        if (masks[p] & 1u) {
            windows[r] += 1u;
            hits[r] += (masks[p] >> 1) & 1u;
        }
        line += text[p] == 10;
    }
}
