// The CPU driver of the record selection for the tests (tests/test_record_select_on_the_cpu.py builds it as a shared
// library, tests/select_san_main.cpp as a sanitized executable): the window loops of strand_cpu_driver.hpp with a selection —
// include mask, MAPQ floor, region list — handed to kmm_bam::CpuBackend and kmm_sam::cpu_chunk.  The region list is sorted and
// merged here by kmm_sel::merge_intervals, as the library does before it uploads one.
#pragma once

#include "bam_windows_cpu.hpp"
#include "kmm_sam.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

// rules: [0] include mask, [1] MAPQ floor, [2] keep_unplaced, [3] n intervals; iv: n x (ref, beg, end), unmerged
struct SelectTables {
    std::vector<kmm_sel::Interval> iv;
    kmm_sel::Sel sel;
    SelectTables(const uint64_t *rules, const int64_t *iv3, const uint8_t *names, const uint32_t *name_off, uint32_t n_names)
    {
        for (uint64_t i = 0; i < rules[3]; ++i)
            iv.push_back(kmm_sel::Interval{iv3[3 * i], iv3[3 * i + 1], iv3[3 * i + 2]});
        kmm_sel::merge_intervals(iv);
        sel.incl = (uint32_t)rules[0];
        sel.min_mapq = (uint32_t)rules[1];
        sel.keep_unplaced = rules[3] ? (uint32_t)rules[2] : 0u;
        sel.n_iv = (uint32_t)iv.size();
        sel.iv = iv.data();
        sel.names = names;
        sel.name_off = name_off;
        sel.n_names = n_names;
    }
};

// As strand_bam_cpu.  stats: [0] records, [1] excluded, [2] calls, [3] records without qualities, [4] records flipped, [5] error
// position, [6] error code (SAM).
extern "C" int select_bam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, int qual, int orig,
                              uint32_t lanes, uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats, const uint64_t *rules,
                              const int64_t *iv3)
{
    SelectTables tb(rules, iv3, nullptr, nullptr, 0);
    for (int i = 0; i < 7; ++i)
        stats[i] = 0;
    uint64_t w = 0;
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{2, 5},
        [&](kmm_bam::CpuBackend &be) {
            be.excl = excl;
            be.qual = qual != 0;
            be.orig = orig != 0;
            be.lanes = lanes;
            be.sel = tb.sel;
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
static int select_sam_windows(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, bool orig, uint32_t lanes,
                              uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats, const kmm_sel::Sel &sel)
{
    uint64_t pos = 0, w = 0, base = 0;
    for (int i = 0; i < 7; ++i)
        stats[i] = 0;
    const unsigned shift = sel.flags_only() ? 2u : 3u;
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
        kmm_sam::cpu_chunk<Q>(win.data(), win.size(), excl, nullptr, t, nullptr, false, nullptr, lanes, &sel);
        ++stats[2];
        if (t.err != kmm_sam::NONE) {
            stats[5] = base + (t.err >> shift);
            stats[6] = t.err & ((1u << shift) - 1u);
            return -3;
        }
        if (w + t.out_bytes > out_cap)
            return -5;
        if (t.out_bytes) {
            std::vector<uint8_t> exact(t.out_bytes);
            kmm_sam::cpu_chunk<Q>(win.data(), win.size(), excl, exact.data(), t, &stats[3], orig, &stats[4], lanes, &sel);
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

// As strand_sam_cpu; names / name_off / n_names: the name table the intervals' refs index.
extern "C" int select_sam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, int qual, int orig,
                              uint32_t lanes, uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats, const uint64_t *rules,
                              const int64_t *iv3, const uint8_t *names, const uint32_t *name_off, uint32_t n_names)
{
    SelectTables tb(rules, iv3, names, name_off, n_names);
    return qual ? select_sam_windows<true>(data, n, cuts, n_cuts, excl, orig != 0, lanes, out, out_cap, out_n, stats, tb.sel)
                : select_sam_windows<false>(data, n, cuts, n_cuts, excl, orig != 0, lanes, out, out_cap, out_n, stats, tb.sel);
}

// merge_intervals in place: iv3 = n x (ref, beg, end); returns the number of intervals left
extern "C" uint64_t select_merge(int64_t *iv3, uint64_t n)
{
    std::vector<kmm_sel::Interval> v;
    for (uint64_t i = 0; i < n; ++i)
        v.push_back(kmm_sel::Interval{iv3[3 * i], iv3[3 * i + 1], iv3[3 * i + 2]});
    kmm_sel::merge_intervals(v);
    for (size_t i = 0; i < v.size(); ++i) {
        iv3[3 * i] = v[i].ref;
        iv3[3 * i + 1] = v[i].beg;
        iv3[3 * i + 2] = v[i].end;
    }
    return v.size();
}

// overlaps() on a merged list
extern "C" int select_overlaps(const int64_t *iv3, uint64_t n, int64_t ref, int64_t rb, int64_t re)
{
    std::vector<kmm_sel::Interval> v;
    for (uint64_t i = 0; i < n; ++i)
        v.push_back(kmm_sel::Interval{iv3[3 * i], iv3[3 * i + 1], iv3[3 * i + 2]});
    return kmm_sel::overlaps(v.data(), (uint32_t)v.size(), ref, rb, re) ? 1 : 0;
}
