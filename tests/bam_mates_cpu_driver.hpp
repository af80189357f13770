// The CPU driver of kmm_bam.hpp's RAW form WITH MATES KEPT TOGETHER for the tests (tests/test_bam_mates_on_the_cpu.py builds it as a
// shared library, tests/bam_mates_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in
// windows, as tests/bam_records_cpu_driver.hpp feeds it, and behind every window what kmm_map_bam does under "record_bam_mates"
//  with the plain C++ its kernels run — CpuBackend's raw_count_pairs(), raw_pair_names(), raw_carry_copy() and
// raw_copy_pairs() — and the hand-over of an odd last record's raw bytes to the next window.
#pragma once

#include "kmm_bam.hpp"

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
    uint64_t pos = 0, w = tail0, base = 0, done = 0; // done: entries used (even)
    int32_t n_ref = -1;
    uint64_t start0 = 0;
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
    int rc = 0;
    std::vector<uint8_t> carry, mate; // carry: the bytes behind the last whole record; mate: the raw bytes of a waiting mate 1
    for (int i = 0; i < n_cuts && rc == 0; ++i) {
        const uint64_t end = cuts[i];
        if (end < pos)
            continue;
        const bool last = end == n;
        stats[7] = (uint64_t)i;
        std::vector<uint8_t> win(carry);
        win.insert(win.end(), data + pos, data + end);
        if (n_ref < 0) {
            uint64_t hdr_end = 0;
            int32_t nr = 0;
            const int r = kmm_bam::parse_header(win.data(), win.size(), &hdr_end, &nr);
            if (r < 0) {
                rc = -1;
                break;
            }
            if (r > 0) {
                if (last)
                    rc = -2;
                continue;
            }
            n_ref = nr;
            start0 = hdr_end;
            stats[4] = hdr_end;
        }
        kmm_bam::CpuBackend be;
        be.d = win.data();
        be.n = win.size();
        be.n_ref = n_ref;
        be.excl = opt[0];
        be.sel.incl = opt[1];
        be.sel.min_mapq = opt[2];
        be.sel.n_iv = (uint32_t)iv.size();
        be.sel.keep_unplaced = opt[4];
        be.sel.iv = iv.data();
        be.lanes = opt[5];
        kmm_bam::CallOut co;
        if (kmm_bam::run_call(be, win.size(), start0, co) != 0) {
            rc = -6;
            break;
        }
        ++stats[3];
        if (co.err_pos != kmm_bam::NONE) {
            stats[5] = base + co.err_pos;
            rc = -3;
            break;
        }
        if (last && co.consumed != win.size()) {
            rc = -4;
            break;
        }
        const uint32_t carried = mate.empty() ? 0u : 1u;
        if (co.recs == 0) { // (no selected record: a waiting mate 1 goes on waiting, unless the stream ends here)
            if (last && carried) {
                stats[6] = done + 1;
                rc = -11;
                break;
            }
            stats[1] += co.excluded;
            carry.assign(win.begin() + (std::ptrdiff_t)co.consumed, win.end());
            base += co.consumed;
            pos = end;
            start0 = 0;
            continue;
        }
        const uint64_t n_rec = co.recs + carried, n_call = n_rec & ~1ull; // the call's entries: those of its whole pairs
        if (done + n_call > n_entries) {
            rc = -8;
            break;
        }
        const uint32_t *h = hits + done, *wn = windows ? windows + done : nullptr;
        uint64_t kept_recs = 0, odd_pos = kmm_bam::NONE;
        uint32_t odd_len = 0;
        const uint64_t kept = be.raw_count_pairs(h, wn, n_call, rule, carried, &kept_recs, &odd_pos, &odd_len);
        const uint64_t bad = be.raw_pair_names(co.consumed, n_call, carried, mate.data(), (uint32_t)mate.size());
        if (bad != kmm_bam::NONE) {
            stats[6] = done / 2 + bad;
            rc = -10;
            break;
        }
        if ((n_rec & 1) != (odd_pos != kmm_bam::NONE ? 1u : 0u)) {
            rc = -12;
            break;
        }
        if (last && (n_rec & 1)) {
            stats[6] = done + n_call + 1;
            rc = -11;
            break;
        }
        const uint64_t shift = kmm_bam::raw_carry_shift(h, wn, n_call, rule, carried, (uint32_t)mate.size());
        if (w + shift + kept > out_cap) {
            rc = -5;
            break;
        }
        if (shift)
            be.raw_carry_copy(mate.data(), (uint32_t)mate.size(), queue, w);
        be.raw_copy_pairs(h, wn, n_call, rule, carried, queue, w + shift);
        w += shift + kept;
        done += n_call;
        stats[0] += co.recs;
        stats[1] += co.excluded;
        stats[2] += kept_recs + (shift ? 1u : 0u);
        if (co.recs > 0) { // (a window without a selected record leaves a waiting mate 1 where it is)
            if (odd_pos != kmm_bam::NONE)
                mate.assign(win.begin() + (std::ptrdiff_t)odd_pos, win.begin() + (std::ptrdiff_t)(odd_pos + odd_len));
            else
                mate.clear();
        }
        carry.assign(win.begin() + (std::ptrdiff_t)co.consumed, win.end());
        base += co.consumed;
        pos = end;
        start0 = 0;
    }
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
