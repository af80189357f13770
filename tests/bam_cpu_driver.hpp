// The CPU driver of kmm_bam.hpp's pipeline for the tests (tests/test_bam_walk_on_the_cpu.py builds it as a shared library,
// tests/bam_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in windows, with the
// bytes behind each window's last complete record carried into the next one — kmm_map_bam's loop without the inflater.
#pragma once

#include "bam_windows_cpu.hpp"

// Windows end at cuts[0 .. n_cuts) (the last one = n), as bam_windows::run takes them.  out: the two-line FASTA of the kept records.  stats: records,
// excluded, false starts, continuations, calls, header bytes.  Returns 0; -1 the header is malformed; -2 the stream ends
// inside the header; -3 a malformed record (stats[6] = its offset in the stream); -4 the stream ends inside a record;
// -5 out_cap too small.
extern "C" int bam_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, uint8_t *out,
                       uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    for (int i = 0; i <= 6; ++i)
        stats[i] = 0;
    uint64_t w = 0;
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{4, 6, 5, 2, 3}, [&](kmm_bam::CpuBackend &be) { be.excl = excl; },
        [&](kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, const std::vector<uint8_t> &, uint64_t, bool) {
            return bam_windows::decode_to(be, co, out, out_cap, &w, false);
        });
    if (rc == 0)
        *out_n = w;
    return rc;
}
