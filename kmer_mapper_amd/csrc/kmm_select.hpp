// kmm_select.hpp — part of libkmm: which SAM / BAM records are mapped (kmm_set_record_regions, "bam_include_flags",
// "bam_min_mapq").  The rule is one for both front ends; this file holds what they share: the interval list
// (sorted by reference and start, overlapping and abutting intervals merged — on the host, merge_intervals) and its lookup
// (overlaps: a binary search, on the device and in the CPU tests).  kmm_bam.hpp and kmm_sam.hpp read a record's fields and ask
// here.  Compiled by itself with g++ in tests/test_record_select_on_the_cpu.py.
//
// A record is KEPT iff (FLAG & exclude) == 0, (FLAG & include) == include, MAPQ >= min_mapq and, with a region list set, it
// overlaps a region on its reference (htslib's rule): positions 0-based, half-open; rec_beg = pos; rec_end = rec_beg + the summed
// lengths of the CIGAR operations M, D, N, = and X — or rec_beg + 1 when FLAG has 0x4, there is no CIGAR, or the sum is 0;
// overlap: beg < rec_end && rec_beg < end.  A record without a reference is kept iff keep_unplaced; one with a reference and no
// position (pos < 0) overlaps nothing.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define KMM_SEL_HD __host__ __device__ __forceinline__
#else
#define KMM_SEL_HD inline
#endif

namespace kmm_sel {

// (the limits on a region list — regions, distinct references, name bytes — are the C ABI's: include/kmm.h)
constexpr uint32_t FLAG_UNMAPPED = 0x4u;
constexpr uint32_t MAX_CIGAR_LEN = (1u << 28) - 1u; // an operation's length (BAM stores it in 28 bits)

// ref: the BAM refID, or (SAM) the index of the reference's name in the handle's name table
struct Interval {
    int64_t ref, beg, end;
};

// The selection beyond the exclude mask.  The default-constructed value means "flags only": nothing but excl applies.
struct Sel {
    uint32_t excl = 0, incl = 0, min_mapq = 0;
    uint32_t n_iv = 0;          // > 0: a region list is set (iv: n_iv merged intervals, sorted by (ref, beg))
    uint32_t keep_unplaced = 0; // records without a reference pass the region rule
    uint32_t n_names = 0;       // SAM: names[name_off[i], name_off[i + 1]) is the name of reference i
    const Interval *iv = nullptr;
    const uint32_t *name_off = nullptr;
    const uint8_t *names = nullptr;
    bool flags_only() const { return incl == 0 && min_mapq == 0 && n_iv == 0; }
};

// Rules 1 and 2: the two flag masks
KMM_SEL_HD bool flags_pass(uint32_t flag, const Sel &s) { return (flag & s.excl) == 0u && (flag & s.incl) == s.incl; }

// Does [rb, re) overlap an interval on `ref`?  The intervals are disjoint and sorted by (ref, beg), so their ends ascend with
// their starts: the last one that starts before re is the only candidate.
KMM_SEL_HD bool overlaps(const Interval *iv, uint32_t n, int64_t ref, int64_t rb, int64_t re)
{
    uint32_t lo = 0, hi = n; // the first interval with (ref, beg) >= (ref, re)
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2;
        if (iv[mid].ref < ref || (iv[mid].ref == ref && iv[mid].beg < re))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo > 0 && iv[lo - 1].ref == ref && iv[lo - 1].end > rb;
}

// Rule 4 for a record with a reference: flag, position and the CIGAR's reference span (0: none).
KMM_SEL_HD bool region_pass(const Sel &s, int64_t ref, int64_t pos, uint32_t flag, uint64_t span)
{
    if (pos < 0)
        return false;
    const uint64_t len = (flag & FLAG_UNMAPPED) || span == 0 ? 1ull : span;
    return overlaps(s.iv, s.n_iv, ref, pos, pos + (int64_t)len);
}

// Does a CIGAR operation consume reference?  BAM codes MIDNSHP=X = 0..8: M 0, D 2, N 3, = 7, X 8.
KMM_SEL_HD bool consumes_ref(uint32_t op) { return ((0x18Du >> (op & 15u)) & 1u) != 0u; }

// Sort by (ref, beg) and merge the intervals that overlap or abut (host side; the kernels search the result).
inline void merge_intervals(std::vector<Interval> &v)
{
    std::sort(v.begin(), v.end(), [](const Interval &a, const Interval &b) { return a.ref != b.ref ? a.ref < b.ref : a.beg < b.beg; });
    size_t w = 0;
    for (size_t i = 0; i < v.size(); ++i) {
        if (w > 0 && v[w - 1].ref == v[i].ref && v[i].beg <= v[w - 1].end) {
            if (v[i].end > v[w - 1].end)
                v[w - 1].end = v[i].end;
        } else
            v[w++] = v[i];
    }
    v.resize(w);
}

} // namespace kmm_sel
