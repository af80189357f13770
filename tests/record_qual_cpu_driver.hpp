// The CPU driver of the quality variants of kmm_bam.hpp and kmm_sam.hpp ("use_record_qual") for the tests
// (tests/test_record_qual_on_the_cpu.py builds it as a shared library, tests/record_qual_san_main.cpp as a sanitized executable):
// the window loops of bam_cpu_driver.hpp and sam_cpu_driver.hpp, with the four-line FASTQ output in place of the two-line FASTA.
#pragma once

#include "kmm_bam.hpp"
#include "kmm_sam.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

// As bam_cpu (bam_cpu_driver.hpp); out: the four-line FASTQ of the kept records; stats[7]: kept records whose qualities are absent.
extern "C" int bam_qual_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, uint8_t *out,
                            uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    uint64_t pos = 0, w = 0, base = 0;
    int32_t n_ref = -1;
    uint64_t start0 = 0;
    for (int i = 0; i <= 7; ++i)
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
                continue;
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
        be.qual = true;
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
        if (co.recs) {
            std::vector<uint8_t> exact(co.out_bytes); // (exactly the totals' size: a write past it is caught by the sanitizer)
            be.decode(exact.data());
            memcpy(out + w, exact.data(), exact.size());
        }
        w += co.out_bytes;
        stats[0] += co.recs;
        stats[1] += co.excluded;
        stats[7] += be.no_qual;
        carry.assign(win.begin() + (std::ptrdiff_t)co.consumed, win.end());
        base += co.consumed;
        pos = end;
        start0 = 0;
    }
    *out_n = w;
    return 0;
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
