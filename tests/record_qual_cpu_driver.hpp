// The CPU driver of the quality variants of kmm_bam.hpp and kmm_sam.hpp ("use_record_qual") for the tests
// (tests/test_record_qual_on_the_cpu.py builds it as a shared library, tests/record_qual_san_main.cpp as a sanitized executable):
// the window loops of bam_cpu_driver.hpp and sam_cpu_driver.hpp, with the four-line FASTQ output in place of the two-line FASTA.
#pragma once

#include "bam_windows_cpu.hpp"
#include "kmm_sam.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

// As bam_cpu (bam_cpu_driver.hpp); out: the four-line FASTQ of the kept records; stats[7]: kept records whose qualities are absent.
extern "C" int bam_qual_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, uint8_t *out,
                            uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    for (int i = 0; i <= 7; ++i)
        stats[i] = 0;
    uint64_t w = 0;
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{4, 6, 5, 2, 3},
        [&](kmm_bam::CpuBackend &be) {
            be.excl = excl;
            be.qual = true;
        },
        [&](kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, const std::vector<uint8_t> &, uint64_t, bool) {
            const int r = bam_windows::decode_to(be, co, out, out_cap, &w, true);
            if (r != 0)
                return r;
            stats[7] += be.no_qual;
            return 0;
        });
    if (rc == 0)
        *out_n = w;
    return rc;
}

// As sam_cpu (sam_cpu_driver.hpp); out: the four-line FASTQ of the kept records; stats[5]: kept records with bases whose QUAL is
// absent.  The error code 0 in stats[4] is a QUAL that is not "*" and not as long as SEQ.
extern "C" int sam_qual_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, uint8_t *out,
                            uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
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
        kmm_sam::cpu_chunk<true>(win.data(), win.size(), excl, nullptr, t);
        ++stats[3];
        if (t.err != kmm_sam::NONE) {
            stats[4] = (base + (t.err >> 2)) << 2 | (t.err & 3);
            return -3;
        }
        if (w + t.out_bytes > out_cap)
            return -5;
        if (t.out_bytes) {
            std::vector<uint8_t> exact(t.out_bytes); // (exactly the totals' size: longer than the window when QUAL is "*")
            kmm_sam::cpu_chunk<true>(win.data(), win.size(), excl, exact.data(), t, &stats[5]);
            memcpy(out + w, exact.data(), exact.size());
        }
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

// kmm_bam::walk<true> from p to te over d[0, n): out = exit, records, excluded, output bytes (the uint32 of Walk), bad
extern "C" void bam_walk_qual(const uint8_t *d, uint64_t n, uint64_t p, uint64_t te, int32_t n_ref, uint32_t excl, uint64_t *out)
{
    kmm_bam::Walk w;
    kmm_bam::walk<true>(d, n, p, te, n_ref, excl, w);
    out[0] = w.exit;
    out[1] = w.recs;
    out[2] = w.excluded;
    out[3] = w.bytes;
    out[4] = w.bad ? 1 : 0;
}

extern "C" uint64_t bam_max_tile_out() { return kmm_bam::MAX_TILE_OUT; }
