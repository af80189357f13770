// The CPU driver of kmm_bam.hpp's RAW form WITH MATES KEPT TOGETHER for the tests (tests/test_bam_mates_on_the_cpu.py builds it as a
// shared library, tests/bam_mates_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in
// windows, as tests/bam_records_cpu_driver.hpp feeds it, and behind every window what kmm_map_bam does under "record_bam_mates"
//  with the plain C++ its kernels run — CpuBackend's raw_count_pairs(), raw_pair_names(), raw_carry_copy() and
// raw_copy_pairs() — and the hand-over of an odd last record's raw bytes to the next window.
#pragma once

#include "bam_windows_cpu.hpp"

#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

// opt: excl, incl, min_mapq, n_regions, keep_unplaced, lanes, min_hits, min_permille, invert, fill, pair_rule.  regions, cuts, out,
// out_cap, tail0, out_n: as bam_records_cpu.  hits / windows: one entry per selected record of the stream in file order, which is
// pair order (n_entries of them; an odd last one is never read).  stats: selected records, excluded, kept records, calls, header
// bytes, [5] the offset of a malformed record, [6] the pair ordinal of the first strangers or the count of selected records of an
// unpaired end, [7] the window (its index in cuts) whose call failed.  Returns 0; -1 .. -9 as bam_records_cpu; -10 strangers;
// -11 the stream ends with an unpaired record.  A failing window appends nothing: *out_n is what the windows before it appended.
extern "C" int bam_mates_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, const uint32_t *opt, const int64_t *regions,
                             const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, uint8_t *out, uint64_t out_cap, uint64_t tail0,
                             uint64_t *out_n, uint64_t *stats)
{
    uint64_t w = tail0, done = 0; // done: entries used (even)
    for (int i = 0; i <= 7; ++i)
        stats[i] = 0;
    *out_n = 0;
    if (tail0 > out_cap)
        return -5;
    std::vector<kmm_sel::Interval> iv;
    for (uint32_t i = 0; i < opt[3]; ++i)
        iv.push_back(kmm_sel::Interval{regions[3 * i], regions[3 * i + 1], regions[3 * i + 2]});
    kmm_sel::merge_intervals(iv);
    const RkPairRule rule = {{opt[6], opt[7], opt[8]}, opt[10]};
    void *mem = nullptr;
    if (posix_memalign(&mem, 16, out_cap ? (size_t)out_cap : 1) != 0) // (exactly out_cap bytes: a store behind them is the sanitizer's)
        return -9;
    uint8_t *queue = (uint8_t *)mem;
    memset(queue, (int)opt[9], (size_t)out_cap);
    std::vector<uint8_t> mate; // the raw bytes of a waiting mate 1
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{3, 5, 4, -1, -1, 7},
        [&](kmm_bam::CpuBackend &be) {
            be.excl = opt[0];
            be.sel.incl = opt[1];
            be.sel.min_mapq = opt[2];
            be.sel.n_iv = (uint32_t)iv.size();
            be.sel.keep_unplaced = opt[4];
            be.sel.iv = iv.data();
            be.lanes = opt[5];
        },
        [&](kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, const std::vector<uint8_t> &win, uint64_t, bool last) {
            const uint32_t carried = mate.empty() ? 0u : 1u;
            if (co.recs == 0) { // (no selected record: a waiting mate 1 goes on waiting, unless the stream ends here)
                if (last && carried) {
                    stats[6] = done + 1;
                    return -11;
                }
                return 0;
            }
            const uint64_t n_rec = co.recs + carried, n_call = n_rec & ~1ull; // the call's entries: those of its whole pairs
            if (done + n_call > n_entries)
                return -8;
            const uint32_t *h = hits + done, *wn = windows ? windows + done : nullptr;
            uint64_t kept_recs = 0, odd_pos = kmm_bam::NONE;
            uint32_t odd_len = 0;
            const uint64_t kept = be.raw_count_pairs(h, wn, n_call, rule, carried, &kept_recs, &odd_pos, &odd_len);
            const uint64_t bad = be.raw_pair_names(co.consumed, n_call, carried, mate.data(), (uint32_t)mate.size());
            if (bad != kmm_bam::NONE) {
                stats[6] = done / 2 + bad;
                return -10;
            }
            if ((n_rec & 1) != (odd_pos != kmm_bam::NONE ? 1u : 0u))
                return -12;
            if (last && (n_rec & 1)) {
                stats[6] = done + n_call + 1;
                return -11;
            }
            const uint64_t shift = kmm_bam::raw_carry_shift(h, wn, n_call, rule, carried, (uint32_t)mate.size());
            if (w + shift + kept > out_cap)
                return -5;
            if (shift)
                be.raw_carry_copy(mate.data(), (uint32_t)mate.size(), queue, w);
            be.raw_copy_pairs(h, wn, n_call, rule, carried, queue, w + shift);
            w += shift + kept;
            done += n_call;
            stats[2] += kept_recs + (shift ? 1u : 0u);
            if (odd_pos != kmm_bam::NONE)
                mate.assign(win.begin() + (std::ptrdiff_t)odd_pos, win.begin() + (std::ptrdiff_t)(odd_pos + odd_len));
            else
                mate.clear();
            return 0;
        });
    memcpy(out, queue, (size_t)out_cap);
    free(mem);
    *out_n = w - tail0;
    return rc;
}

// The mate check's comparison by itself: 1 iff the names (la and lb bytes, the NUL included) are no mates' — the lengths, then
// names_differ_part by every lane of `lanes`.  The names are copied into buffers of exactly their size: a read past them is the
// sanitizer's.
extern "C" int bam_mates_names_differ(const uint8_t *a, uint32_t la, const uint8_t *b, uint32_t lb, uint32_t lanes)
{
    if (la != lb)
        return 1;
    std::vector<uint8_t> x(a, a + la), y(b, b + lb);
    bool diff = false;
    for (uint32_t lane = 0; lane < lanes; ++lane)
        diff |= kmm_bam::names_differ_part(x.data(), y.data(), la, lane, lanes);
    return diff ? 1 : 0;
}
