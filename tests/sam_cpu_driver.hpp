// The CPU driver of kmm_sam.hpp for the tests (tests/test_sam_on_the_cpu.py builds it as a shared library, tests/sam_san_main.cpp
// as a sanitized executable): a SAM stream through the per-tile line walk in windows, the bytes behind each window's last newline
// carried into the next one, a final line without newline given one — the loop of kmm_map_bgzf on SAM without the inflater.
#pragma once

#include "kmm_sam.hpp"

#include <cstddef>
#include <vector>

// Windows end at cuts[0 .. n_cuts) (the last one = n); every window is copied into a buffer of exactly its size.  out: the
// two-line FASTA of the kept records.  stats: records, excluded, header lines, calls, the malformed line's stream offset << 2 |
// its error code.  Returns 0; -3 a malformed line; -5 out_cap too small.
extern "C" int sam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, uint8_t *out,
                       uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    uint64_t pos = 0, w = 0, base = 0; // base: stream offset of the window's first byte
    for (int i = 0; i < 5; ++i)
        stats[i] = 0;
    std::vector<uint8_t> carry;
    for (int i = 0; i < n_cuts; ++i) {
        const uint64_t end = cuts[i];
        if (end < pos)
            continue;
        const bool last = end == n;
        std::vector<uint8_t> win(carry);
        win.insert(win.end(), data + pos, data + end);
        if (last && !win.empty() && win.back() != 10)
            win.push_back(10);
        kmm_sam::Totals t;
        kmm_sam::cpu_chunk(win.data(), win.size(), excl, nullptr, t);
        ++stats[3];
        if (t.err != kmm_sam::NONE) {
            stats[4] = (base + (t.err >> 2)) << 2 | (t.err & 3);
            return -3;
        }
        if (w + t.out_bytes > out_cap)
            return -5;
        kmm_sam::cpu_chunk(win.data(), win.size(), excl, out + w, t);
        w += t.out_bytes;
        stats[0] += t.recs;
        stats[1] += t.excluded;
        stats[2] += t.headers;
        carry.assign(win.begin() + (std::ptrdiff_t)t.consumed, win.end());
        base += t.consumed;
        pos = end;
    }
    *out_n = w;
    return 0;
}
