// The CPU driver of kmm_bam.hpp's NAMED form for the tests (tests/test_bam_fastq_on_the_cpu.py builds it as a shared library,
// tests/bam_fastq_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in windows, as
// tests/bam_cpu_driver.hpp feeds it, with CpuBackend's `named` switch on — decode() writes '@' NAME [/1 | /2] '\n' SEQ '\n' "+\n"
// QUAL '\n' per selected record.
#pragma once

#include "bam_windows_cpu.hpp"

#include <algorithm>

// opt: excl, incl, min_mapq, n_regions, keep_unplaced, original_strand, mate_suffix, lanes.  regions: n_regions x (refID, beg,
// end), merged here as the library merges them.  Windows end at cuts[0 .. n_cuts) (the last one = n).  out: the named FASTQ of
// the selected records; its bytes are written by decode() alone — the caller fills it first and sees what was not written.
// stats: records, excluded, false starts, continuations, calls, header bytes, [6] the offset of a malformed record, no_qual,
// reversed, replaced.  Returns 0; -1 the header is malformed; -2 the stream ends inside the header; -3 a malformed record; -4 the
// stream ends inside a record; -5 out_cap too small; -7 the bytes run_call counted are not the bytes of the records' heads.
extern "C" int bam_fastq_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, const uint32_t *opt,
                             const int64_t *regions, uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    for (int i = 0; i <= 9; ++i)
        stats[i] = 0;
    std::vector<kmm_sel::Interval> iv;
    for (uint32_t i = 0; i < opt[3]; ++i)
        iv.push_back(kmm_sel::Interval{regions[3 * i], regions[3 * i + 1], regions[3 * i + 2]});
    kmm_sel::merge_intervals(iv);
    uint64_t w = 0;
    const int rc = bam_windows::run(
        data, n, cuts, n_cuts, stats, bam_windows::Slots{4, 6, 5, 2, 3},
        [&](kmm_bam::CpuBackend &be) {
            be.excl = opt[0];
            be.sel.incl = opt[1];
            be.sel.min_mapq = opt[2];
            be.sel.n_iv = (uint32_t)iv.size();
            be.sel.keep_unplaced = opt[4];
            be.sel.iv = iv.data();
            be.orig = opt[5] != 0;
            be.named = true;
            be.mate_suffix = opt[6] != 0;
            be.lanes = opt[7];
        },
        [&](kmm_bam::CpuBackend &be, const kmm_bam::CallOut &co, const std::vector<uint8_t> &, uint64_t, bool) {
            const int r = bam_windows::decode_to(be, co, out, out_cap, &w, false);
            if (r != 0)
                return r;
            stats[7] += be.no_qual;
            stats[8] += be.reversed;
            stats[9] += be.replaced;
            return 0;
        });
    if (rc == 0)
        *out_n = w;
    return rc;
}

// One record (rec[0, n): block_size and all) decoded by every lane of `lanes` on its own, twice — into bytes that were 0x00 and
// into bytes that were 0xFF: a byte the lane wrote is the same in both.  writes[i] = how many lanes wrote byte i of the record's
// out_len_named bytes (the caller asserts 1 throughout).  Returns that length, or -1 when rec is no whole record.
extern "C" int64_t bam_fastq_record_writes(const uint8_t *rec, uint64_t n, uint32_t lanes, uint32_t mate_suffix, uint32_t orig,
                                           uint32_t *writes, uint64_t cap)
{
    kmm_bam::RecHead h;
    if (kmm_bam::record_at(rec, n, 0, 0x7FFFFFFF, h) != kmm_bam::REC_OK)
        return -1;
    const uint32_t len = kmm_bam::out_len_named(h, mate_suffix != 0);
    if (len > cap)
        return -1;
    const bool rev = kmm_bam::flipped(h, orig != 0);
    std::vector<uint8_t> a(len + 16ull), b(len + 16ull); // (8 guard bytes on either side)
    for (uint32_t i = 0; i < len; ++i)
        writes[i] = 0;
    for (uint32_t lane = 0; lane < lanes; ++lane) {
        std::fill(a.begin(), a.end(), (uint8_t)0x00);
        std::fill(b.begin(), b.end(), (uint8_t)0xFF);
        if (rev) {
            kmm_bam::decode_record_named_rev(rec, h, a.data() + 8, lane, lanes, mate_suffix != 0);
            kmm_bam::decode_record_named_rev(rec, h, b.data() + 8, lane, lanes, mate_suffix != 0);
        } else {
            kmm_bam::decode_record_named(rec, h, a.data() + 8, lane, lanes, mate_suffix != 0);
            kmm_bam::decode_record_named(rec, h, b.data() + 8, lane, lanes, mate_suffix != 0);
        }
        for (uint32_t i = 0; i < 8; ++i)
            if (a[i] != 0x00 || b[i] != 0xFF || a[len + 8ull + i] != 0x00 || b[len + 8ull + i] != 0xFF)
                return -2; // a store outside the record's bytes
        for (uint32_t i = 0; i < len; ++i)
            writes[i] += a[8ull + i] == b[8ull + i] ? 1u : 0u;
    }
    return (int64_t)len;
}
