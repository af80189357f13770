// The CPU driver of "original_strand"  for the tests (tests/test_strand_on_the_cpu.py builds it as a shared library,
// tests/strand_san_main.cpp as a sanitized executable): the window loops of bam_cpu_driver.hpp and sam_cpu_driver.hpp with the
// switch, the plain or the quality variant, and the lane count the per-record functions are called with as arguments.
#pragma once

#include "bam_windows_cpu.hpp"
#include "kmm_sam.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

// As bam_cpu (bam_cpu_driver.hpp).  qual: four-line FASTQ instead of two-line FASTA; orig: the switch; lanes: 1 or 64.
// stats: [0] records, [1] excluded, [2] calls, [3] records without qualities, [4] records flipped, [5] error position.
extern "C" int strand_bam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, int qual, int orig,
                              uint32_t lanes, uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    for (int i = 0; i < 6; ++i)
        stats[i] = 0;
    uint64_t w = 0;
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{2, 5},
        [&](kmm_bam::CpuBackend &be) {
            be.excl = excl;
            be.qual = qual != 0;
            be.orig = orig != 0;
            be.lanes = lanes;
        },
        [&](kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, const std::vector<uint8_t> &, uint64_t, bool) {
            const int r = bam_windows::decode_to(be, co, out, out_cap, &w, true);
            if (r != 0)
                return r;
            stats[3] += be.no_qual;
            stats[4] += be.reversed;
            return 0;
        });
    if (rc == 0)
        *out_n = w;
    return rc;
}

template <bool Q>
static int strand_sam_windows(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, bool orig, uint32_t lanes,
                              uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    uint64_t pos = 0, w = 0, base = 0;
    for (int i = 0; i < 6; ++i)
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
        kmm_sam::cpu_chunk<Q>(win.data(), win.size(), excl, nullptr, t);
        ++stats[2];
        if (t.err != kmm_sam::NONE) {
            stats[5] = (base + (t.err >> 2)) << 2 | (t.err & 3);
            return -3;
        }
        if (w + t.out_bytes > out_cap)
            return -5;
        if (t.out_bytes) {
            std::vector<uint8_t> exact(t.out_bytes); // (see strand_bam_cpu)
            kmm_sam::cpu_chunk<Q>(win.data(), win.size(), excl, exact.data(), t, &stats[3], orig, &stats[4], lanes);
            memcpy(out + w, exact.data(), exact.size());
        }
        w += t.out_bytes;
        stats[0] += t.recs;
        stats[1] += t.excluded;
        carry.assign(win.begin() + (std::ptrdiff_t)t.consumed, win.end());
        base += t.consumed;
        pos = end;
    }
    *out_n = w;
    return 0;
}

// As sam_cpu (sam_cpu_driver.hpp), with the arguments and statistics of strand_bam_cpu.
extern "C" int strand_sam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, int qual, int orig,
                              uint32_t lanes, uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    return qual ? strand_sam_windows<true>(data, n, cuts, n_cuts, excl, orig != 0, lanes, out, out_cap, out_n, stats)
                : strand_sam_windows<false>(data, n, cuts, n_cuts, excl, orig != 0, lanes, out, out_cap, out_n, stats);
}

// The two complements: of a SAM letter, and of a BAM code as the letter it decodes to
extern "C" uint32_t strand_comp_letter(uint32_t c) { return kmm_sam::comp_letter((uint8_t)c); }
extern "C" uint32_t strand_comp_code_letter(uint32_t code) { return kmm_bam::base_letter(kmm_bam::comp_code(code)); }
