// CPU driver of the position -> read search of csrc/kmm_read_hits.hpp (tests/test_read_hits_on_the_cpu.py,
// tests/read_hits_san_main.cpp): the header compiled by itself with g++, walked the way k_read_hits walks it — the first
// read of every tile, a cursor per lane at its first position, then forward over the lane's positions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kmm_read_hits.hpp"

// out[p] = the read the kernel would give position p, for every p in [0, total).  n_reads >= 1, total >= 1, offs[n_reads] == total.
// Returns the number of offsets reads that fell outside [0, n_reads] (must be 0: the driver checks every index it passes on).
extern "C" int64_t read_hits_search_cpu(const int64_t *offs, int64_t n_reads, int64_t total, int64_t tile_len, int64_t lane_len,
                                               int64_t *out)
{
    const int64_t n_tiles = (total + tile_len - 1) / tile_len;
    std::vector<int64_t> first((size_t)n_tiles + 1);
    int64_t outside = 0;
    for (int64_t t = 0; t <= n_tiles; ++t) {
        first[(size_t)t] = rh_tile_first_read(offs, n_reads, total, t, tile_len);
        if (first[(size_t)t] < 0 || first[(size_t)t] >= n_reads)
            ++outside;
    }
    for (int64_t t = 0; t < n_tiles; ++t)
        for (int64_t p0 = t * tile_len; p0 < (t + 1) * tile_len && p0 < total; p0 += lane_len) {
            RhCursor c = rh_cursor_at(offs, first[(size_t)t], first[(size_t)t + 1], p0);
            for (int64_t j = 0; j < lane_len && p0 + j < total && p0 + j < (t + 1) * tile_len; ++j) {
                rh_cursor_advance(offs, c, p0 + j);
                if (c.r < 0 || c.r >= n_reads)
                    ++outside;
                out[p0 + j] = c.r;
            }
        }
    return outside;
}

// The brute force: the largest r with offs[r] <= p, by a walk from the front.
extern "C" void read_hits_search_brute(const int64_t *offs, int64_t n_reads, int64_t total, int64_t *out)
{
    int64_t r = 0;
    for (int64_t p = 0; p < total; ++p) {
        while (r + 1 < n_reads && offs[r + 1] <= p)
            ++r;
        out[p] = r;
    }
}
