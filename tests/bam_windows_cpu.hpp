// The window loop of the tests' CPU drivers of kmm_bam.hpp (bam_cpu_driver.hpp, bam_fastq_cpu_driver.hpp,
// bam_records_cpu_driver.hpp, bam_mates_cpu_driver.hpp and the BAM halves of strand_cpu_driver.hpp, record_qual_cpu_driver.hpp and
// select_cpu_driver.hpp): a stream of inflated BAM bytes through run_call in windows, with the bytes behind each window's last
// complete record carried into the next one — kmm_map_bam's loop without the inflater.  A driver is this loop plus what it sets
// in the backend and what it does with a window's records.
#pragma once

#include "kmm_bam.hpp"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace bam_windows {

// Where a driver's stats array keeps the loop's own figures (-1: nowhere): the calls, the stream offset of a malformed record,
// the header's bytes, the walk's false starts and continuations, the window (its index in cuts) at work.  Slots 0 and 1 are the
// selected and the excluded records in every driver.
struct Slots {
    int calls, err_pos, header = -1, false_starts = -1, continuations = -1, window = -1;
};

// Windows end at cuts[0 .. n_cuts) (the last one = n).  The first window starts with the header, and one that ends inside the
// header uses nothing: the next starts at the same place.  Every window is copied into a buffer of exactly its size (carry + new
// bytes).  setup(be): the driver's switches, behind d, n and n_ref.  body(be, co, win, base, last) runs behind a good run_call
// (base: the stream offset of the window's first byte) and returns 0 or the driver's own error; the window's records are counted
// behind it.  Returns 0; -1 the header is malformed; -2 the stream ends inside the header; -3 a malformed record; -4 the stream
// ends inside a record; -6 run_call failed; or what body returned.
template <typename Setup, typename Body>
int run(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint64_t *stats, const Slots &s, Setup &&setup, Body &&body)
{
    uint64_t pos = 0, base = 0, start0 = 0;
    int32_t n_ref = -1;
    std::vector<uint8_t> carry;
    for (int i = 0; i < n_cuts; ++i) {
        const uint64_t end = cuts[i];
        if (end < pos)
            continue;
        const bool last = end == n;
        if (s.window >= 0)
            stats[s.window] = (uint64_t)i;
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
            if (s.header >= 0)
                stats[s.header] = hdr_end;
        }
        kmm_bam::CpuBackend be;
        be.d = win.data();
        be.n = win.size();
        be.n_ref = n_ref;
        setup(be);
        kmm_bam::CallOut co;
        if (kmm_bam::run_call(be, win.size(), start0, co) != 0)
            return -6;
        ++stats[s.calls];
        if (s.false_starts >= 0)
            stats[s.false_starts] += co.false_starts;
        if (s.continuations >= 0)
            stats[s.continuations] += co.continuations;
        if (co.err_pos != kmm_bam::NONE) {
            stats[s.err_pos] = base + co.err_pos;
            return -3;
        }
        if (last && co.consumed != win.size())
            return -4;
        const int rc = body(be, co, win, base, last);
        if (rc != 0)
            return rc;
        stats[0] += co.recs;
        stats[1] += co.excluded;
        carry.assign(win.begin() + (std::ptrdiff_t)co.consumed, win.end());
        base += co.consumed;
        pos = end;
        start0 = 0;
    }
    return 0;
}

// The body of the drivers that decode: the window's text behind out[*w].  exact: through a buffer of exactly the totals' size on
// the heap — a write in front of it or behind its last byte is the sanitizer's.  -5: out_cap too small.
inline int decode_to(kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, uint8_t *out, uint64_t out_cap, uint64_t *w, bool exact)
{
    if (*w + co.out_bytes > out_cap)
        return -5;
    if (co.recs && exact) {
        std::vector<uint8_t> buf(co.out_bytes);
        be.decode(buf.data());
        memcpy(out + *w, buf.data(), buf.size());
    } else if (co.recs) {
        be.decode(out + *w);
    }
    *w += co.out_bytes;
    return 0;
}

} // namespace bam_windows
