// CPU driver of the plain-C++ arithmetic of the mate check (tests/test_bam_pairs_on_the_cpu.py,
// tests/bam_pairs_san_main.cpp): csrc/kmm_record_keep.hpp compiled by itself with g++ and walked pair by pair the way
// k_rk_pair_names walks a piece — the ends of mate 1's name and SEQ lines, the step to mate 2's name line by rk_mate2_line, the
// end of that line, rk_names_equal — beside a brute-force walk that counts newlines.  No byte at or behind `consumed` is read.
#pragma once
#include <cstdint>
#include <cstring>

#include "kmm_record_keep.hpp"

// The first newline at or behind `from` and before `limit` (-1: none).
static int64_t bam_pairs_newline(const uint8_t *text, int64_t from, int64_t limit)
{
    for (int64_t p = from; p < limit; ++p)
        if (text[p] == 10)
            return p;
    return -1;
}

extern "C" int bam_pairs_names_equal_cpu(const uint8_t *a, uint32_t len_a, const uint8_t *b, uint32_t len_b, uint32_t mate_suffix)
{
    return rk_names_equal(a, len_a, b, len_b, mate_suffix != 0u) ? 1 : 0;
}

extern "C" uint32_t bam_pairs_name_trim_cpu(const uint8_t *name, uint32_t len, uint32_t mate_suffix)
{
    return rk_name_trim(name, len, mate_suffix != 0u);
}

extern "C" int64_t bam_pairs_mate2_line_cpu(int64_t at, int64_t name_end, int64_t seq_end)
{
    return rk_mate2_line(at, name_end, seq_end);
}

// text[0, consumed): whole pairs of four-line FASTQ.  Returns the first pair whose names differ, -1 when all agree, -2 when
// rk_mate2_line does not land on the line that a count of newlines finds (stats[0]: pairs walked; stats[1]: bytes compared).
extern "C" int64_t bam_pairs_check_cpu(const uint8_t *text, int64_t consumed, uint32_t mate_suffix, int64_t *stats)
{
    int64_t at = 0, pair = 0, first = -1;
    stats[0] = stats[1] = 0;
    while (at < consumed) {
        const int64_t e0 = bam_pairs_newline(text, at, consumed), e1 = e0 < 0 ? -1 : bam_pairs_newline(text, e0 + 1, consumed);
        if (text[at] != '@' || e1 < 0)
            return -2;
        const int64_t at2 = rk_mate2_line(at, e0, e1);
        int64_t brute = e1; // the newline that ends line 3 of the record, by counting
        for (int i = 0; i < 2 && brute >= 0; ++i)
            brute = bam_pairs_newline(text, brute + 1, consumed);
        if (brute < 0 || at2 != brute + 1 || at2 >= consumed || text[at2] != '@')
            return -2;
        const int64_t f0 = bam_pairs_newline(text, at2, consumed);
        if (f0 < 0)
            return -2;
        const uint32_t la = (uint32_t)(e0 - at - 1), lb = (uint32_t)(f0 - at2 - 1);
        if (!rk_names_equal(text + at + 1, la, text + at2 + 1, lb, mate_suffix != 0u) && first < 0)
            first = pair;
        stats[1] += la < lb ? la : lb;
        int64_t end = f0; // behind mate 2: three more lines
        for (int i = 0; i < 3 && end >= 0; ++i)
            end = bam_pairs_newline(text, end + 1, consumed);
        if (end < 0)
            return -2;
        at = end + 1;
        ++pair;
    }
    stats[0] = pair;
    return first;
}
