// The CPU driver of kmm_bam.hpp's RAW form for the tests (tests/test_bam_records_on_the_cpu.py builds it as a shared library,
// tests/bam_records_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in windows, as
// tests/bam_fastq_cpu_driver.hpp feeds it, and behind every window CpuBackend's raw_count() + raw_copy() — the plain C++ the
// kernels of "record_bam" run: the selected records whose entry passes the keep rule, copied as they stand.
#pragma once

#include "bam_windows_cpu.hpp"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

// opt: excl, incl, min_mapq, n_regions, keep_unplaced, lanes, min_hits, min_permille, invert, fill.  regions: n_regions x (refID,
// beg, end), merged here as the library merges them.  Windows end at cuts[0 .. n_cuts) (the last one = n).  hits / windows: one
// entry per selected record of the stream, in file order (n_entries of them).  out[0, out_cap): the queue as the caller sees it;
// the driver's own queue is 16-byte aligned, filled with `fill`, starts with tail0 bytes that are not the stream's, and is
// copied to out at the end: a byte that still holds `fill` was not written.  stats: selected records, excluded, kept records,
// calls, header bytes, [5] the offset of a malformed record.  Returns 0; -1 the header is malformed; -2 the stream ends inside
// the header; -3 a malformed record; -4 the stream ends inside a record; -5 out_cap too small; -8 more selected records than
// entries.
extern "C" int bam_records_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, const uint32_t *opt,
                               const int64_t *regions, const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, uint8_t *out,
                               uint64_t out_cap, uint64_t tail0, uint64_t *out_n, uint64_t *stats)
{
    uint64_t w = tail0, done = 0; // done: entries used
    for (int i = 0; i <= 5; ++i)
        stats[i] = 0;
    *out_n = 0;
    if (tail0 > out_cap)
        return -5;
    std::vector<kmm_sel::Interval> iv;
    for (uint32_t i = 0; i < opt[3]; ++i)
        iv.push_back(kmm_sel::Interval{regions[3 * i], regions[3 * i + 1], regions[3 * i + 2]});
    kmm_sel::merge_intervals(iv);
    const RkRule rule = {opt[6], opt[7], opt[8]};
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, out_cap ? (size_t)out_cap : 1) != 0) // (exactly out_cap bytes: a store behind them is the sanitizer's)
        return -9;
    uint8_t *queue = (uint8_t *)mem;
    memset(queue, (int)opt[9], (size_t)out_cap);
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{3, 5, 4},
        [&](kmm_bam::CpuBackend &be) {
            be.excl = opt[0];
            be.sel.incl = opt[1];
            be.sel.min_mapq = opt[2];
            be.sel.n_iv = (uint32_t)iv.size();
            be.sel.keep_unplaced = opt[4];
            be.sel.iv = iv.data();
            be.lanes = opt[5];
        },
        [&](kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, const std::vector<uint8_t> &, uint64_t, bool) {
            if (done + co.recs > n_entries)
                return -8;
            uint64_t kept_recs = 0;
            const uint64_t kept = be.raw_count(hits + done, windows ? windows + done : nullptr, co.recs, rule, &kept_recs);
            if (w + kept > out_cap)
                return -5;
            be.raw_copy(hits + done, windows ? windows + done : nullptr, co.recs, rule, queue, w);
            w += kept;
            done += co.recs;
            stats[2] += kept_recs;
            return 0;
        });
    memcpy(out, queue, (size_t)out_cap);
    free(mem);
    if (rc == 0)
        *out_n = w - tail0;
    return rc;
}

// One copy of len bytes from a source that starts src_a bytes behind a 16-byte line to a destination that starts dst_a bytes
// behind one, by every lane of `lanes` on its own, twice — into bytes that were 0x00 and into bytes that were 0xFF: a byte the
// lane wrote is the same in both.  writes[i] = how many lanes wrote byte i of the len bytes (the caller asserts 1 throughout).
// Returns 0; -2: a lane wrote outside the destination (32 guard bytes on either side); -3: a written byte is not the source's.
extern "C" int bam_records_copy_writes(uint32_t len, uint32_t src_a, uint32_t dst_a, uint32_t lanes, uint32_t *writes)
{
    void *ms = nullptr, *ma = nullptr, *mb = nullptr;
    const size_t cap = 32 + 16 + (size_t)len + 32;
    if (posix_memalign(&ms, 16, 16 + (size_t)len + 1) != 0 || posix_memalign(&ma, 16, cap) != 0 || posix_memalign(&mb, 16, cap) != 0)
        return -9;
    uint8_t *src = (uint8_t *)ms + src_a, *a = (uint8_t *)ma, *b = (uint8_t *)mb;
    for (uint32_t i = 0; i < len; ++i) {
        src[i] = (uint8_t)(1u + i % 251u);
        writes[i] = 0;
    }
    const uint64_t dst = 32 + dst_a;
    int rc = 0;
    for (uint32_t lane = 0; lane < lanes && rc == 0; ++lane) {
        memset(a, 0x00, cap);
        memset(b, 0xFF, cap);
        kmm_bam::raw_copy_part(src, a, dst, len, lane, lanes);
        kmm_bam::raw_copy_part(src, b, dst, len, lane, lanes);
        for (size_t i = 0; i < cap; ++i) {
            const bool inside = i >= dst && i < dst + len, wrote = a[i] == b[i];
            if (!inside && (a[i] != 0x00 || b[i] != 0xFF))
                rc = -2;
            if (inside && wrote && a[i] != src[i - dst])
                rc = -3;
            if (inside && wrote)
                ++writes[i - dst];
        }
    }
    free(ms);
    free(ma);
    free(mb);
    return rc;
}
