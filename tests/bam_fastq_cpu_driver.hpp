// The CPU driver of kmm_bam.hpp's NAMED form for the tests (tests/test_bam_fastq_on_the_cpu.py builds it as a shared library,
// tests/bam_fastq_san_main.cpp as a sanitized executable): a stream of inflated BAM bytes through run_call in windows, as
// tests/bam_cpu_driver.hpp feeds it, with CpuBackend's `named` switch on — decode() writes '@' NAME [/1 | /2] '\n' SEQ '\n' "+\n"
// QUAL '\n' per selected record.
#pragma once

#include "kmm_bam.hpp"

#include <cstddef>
#include <cstring>
#include <vector>

// opt: excl, incl, min_mapq, n_regions, keep_unplaced, original_strand, mate_suffix, lanes.  regions: n_regions x (refID, beg,
// end), merged here as the library merges them.  Windows end at cuts[0 .. n_cuts) (the last one = n).  out: the named FASTQ of
// the selected records; its bytes are written by decode() alone — the caller fills it first and sees what was not written.
// stats: records, excluded, false starts, continuations, calls, header bytes, [6] the offset of a malformed record, no_qual,
// reversed, replaced.  Returns 0; -1 the header is malformed; -2 the stream ends inside the header; -3 a malformed record; -4 the
// stream ends inside a record; -5 out_cap too small; -7 the bytes run_call counted are not the bytes of the records' heads.
extern "C" int bam_fastq_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, const uint32_t *opt,
                             const int64_t *regions, uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    uint64_t pos = 0, w = 0, base = 0; // base: stream offset of the window's first byte
    int32_t n_ref = -1;
    uint64_t start0 = 0;
    for (int i = 0; i <= 9; ++i)
        stats[i] = 0;
    std::vector<kmm_sel::Interval> iv;
    for (uint32_t i = 0; i < opt[3]; ++i)
        iv.push_back(kmm_sel::Interval{regions[3 * i], regions[3 * i + 1], regions[3 * i + 2]});
    kmm_sel::merge_intervals(iv);
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
                continue; // (a first window inside the header uses nothing: the next one starts at the same place)
            }
            n_ref = nr;
            start0 = hdr_end;
            stats[5] = hdr_end;
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
        be.orig = opt[5] != 0;
        be.named = true;
        be.mate_suffix = opt[6] != 0;
        be.lanes = opt[7];
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
        if (co.recs)
            be.decode(out + w);
        w += co.out_bytes;
        stats[0] += co.recs;
        stats[1] += co.excluded;
        stats[7] += be.no_qual;
        stats[8] += be.reversed;
        stats[9] += be.replaced;
        carry.assign(win.begin() + (std::ptrdiff_t)co.consumed, win.end());
        base += co.consumed;
        pos = end;
        start0 = 0;
    }
    *out_n = w;
    return 0;
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
