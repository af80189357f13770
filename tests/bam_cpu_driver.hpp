// The CPU driver of kmm_bam.hpp's pipeline for the tests (tests/test_bam_walk_on_the_cpu.py builds it as a shared library,
// tests/bam_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in windows, with the
// bytes behind each window's last complete record carried into the next one — kmm_map_bam's loop without the inflater.
#pragma once

#include "kmm_bam.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

// Windows end at cuts[0 .. n_cuts) (the last one = n).  The first window starts with the header; every window is copied into
// a buffer of exactly its size (carry + new bytes).  out: the two-line FASTA of the kept records.  stats: records,
// excluded, false starts, continuations, calls, header bytes.  Returns 0; -1 the header is malformed; -2 the stream ends
// inside the header; -3 a malformed record (stats[6] = its offset in the stream); -4 the stream ends inside a record;
// -5 out_cap too small.
extern "C" int bam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, uint8_t *out,
                       uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    uint64_t pos = 0, w = 0, base = 0; // base: stream offset of the window's first byte
    int32_t n_ref = -1;
    uint64_t start0 = 0;
    for (int i = 0; i <= 6; ++i)
        stats[i] = 0;
    std::vector<uint8_t> carry;
    for (int i = 0; i < n_cuts; ++i) {
        const uint64_t end = cuts[i];
        if (end < pos)
            continue;
        const bool last = end == n;
        std::vector<uint8_t> win(carry);
        win.insert(win.end(), data + pos, data + end);
        if (n_ref < 0) {
            uint64_t hdr_end = 0;
            int32_t nr = 0;
            const int r = kmm_bam::parse_header(win.data(), win.size(), &hdr_end, &nr);
            if (r < 0)
                return -1;
            if (r > 0) {
                if (last)
                    return -2;
                continue; // (a first window inside the header uses nothing: the next one starts at the same place)
            }
            n_ref = nr;
            start0 = hdr_end;
            stats[5] = hdr_end;
        }
        kmm_bam::CpuBackend be;
        be.d = win.data();
        be.n = win.size();
        be.n_ref = n_ref;
        be.excl = excl;
        kmm_bam::CallOut co;
        if (kmm_bam::run_call(be, win.size(), start0, co) != 0)
            return -6;
        ++stats[4];
        stats[2] += co.false_starts;
        stats[3] += co.continuations;
        if (co.err_pos != kmm_bam::NONE) {
            stats[6] = base + co.err_pos;
            return -3;
        }
        if (last && co.consumed != win.size())
            return -4;
        if (w + co.out_bytes > out_cap)
            return -5;
        if (co.recs)
            be.decode(out + w);
        w += co.out_bytes;
        stats[0] += co.recs;
        stats[1] += co.excluded;
        carry.assign(win.begin() + (std::ptrdiff_t)co.consumed, win.end());
        base += co.consumed;
        pos = end;
        start0 = 0;
    }
    *out_n = w;
    return 0;
}
