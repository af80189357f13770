// The CPU driver of kmm_bam.hpp's resync for the tests (tests/test_bam_resync_on_the_cpu.py builds it as a shared library,
// tests/bam_resync_san_main.cpp as a sanitized executable): what kmm_bam_find_record_start does behind its inflater — the
// examined extent, the per-tile step over all tiles, the answer as (member, skip) — on inflated bytes the caller holds.
#pragma once

#include "kmm_bam.hpp"

#include <cstddef>
#include <vector>

// d[0, n): the inflated bytes of a window's whole members, which start at m_off / o_off (n_members + 1 entries each;
// o_off[n_members] == n).  whole: the members end where the window does.  cap: examined bytes at most (0: all).
// *member / *skip: the answer; *pos: the lowest holding position (kmm_bam::NONE: none).  Returns 0.
extern "C" int bam_resync_cpu(const uint8_t *d, uint64_t n, const unsigned long long *m_off, const unsigned long long *o_off,
                              uint64_t n_members, int whole, uint64_t cap, int32_t n_ref, int64_t *member, int64_t *skip, uint64_t *pos)
{
    bool at_eof = false;
    const uint64_t n_ex = kmm_bam::resync_extent(n, cap, whole != 0, &at_eof);
    *pos = n_ex ? kmm_bam::resync_scalar(d, n_ex, n_ref, at_eof) : kmm_bam::NONE;
    kmm_bam::resync_answer(m_off, o_off, n_members, *pos, at_eof, member, skip);
    return 0;
}

// Every boundary byte b in [from, n) of ONE payload: out[b - from] = the lowest holding position of the window d[b, b + len)
// (len 0: to the end of the payload, which ends the file), relative to d; kmm_bam::NONE where no chain holds.
extern "C" void bam_resync_every_byte(const uint8_t *d, uint64_t n, uint64_t from, uint64_t len, int32_t n_ref, uint64_t *out)
{
    for (uint64_t b = from; b < n; ++b) {
        const uint64_t w = len && len < n - b ? len : n - b;
        const uint64_t p = kmm_bam::resync_scalar(d + b, w, n_ref, w == n - b);
        out[b - from] = p == kmm_bam::NONE ? p : b + p;
    }
}
