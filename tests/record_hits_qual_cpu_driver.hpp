// CPU driver of the mark pass of csrc/kmm_rh_qual.hpp (tests/test_record_hits_qual_on_the_cpu.py,
// tests/record_hits_qual_san_main.cpp): the header compiled by itself with g++ and walked the way k_rq_line_starts and k_rq_mark
// walk a piece of FASTQ text — 16 bytes per lane, the line of a lane's first byte and the masks of its bytes formed here the
// way the kernels form them from the census — over the bytes in front of `limit`, the end of the last whole record.
#pragma once
#include <cstddef>
#include <cstdint>

#include "kmm_rh_qual.hpp"

// line_start: uint32[n_lines], filled here; dead: uint32[dead_words], zeroed by the caller; exempt: a bitset over the text's
// bytes or null.  out[0] = the low quality bytes, out[1] = the smallest offset reported as malformed (-1: none), out[2] = words
// set outside [0, dead_words) (must be 0), out[3] = line_start entries never written (must be 0).
extern "C" void rq_mark_cpu(const uint8_t *text, uint32_t limit, uint32_t n_lines, uint32_t thresh, const uint32_t *exempt,
                            uint64_t text_base, uint32_t *line_start, uint32_t *dead, uint32_t dead_words, int64_t *out)
{
    out[0] = 0, out[1] = -1, out[2] = 0, out[3] = 0;
    for (uint32_t i = 0; i < n_lines; ++i)
        line_start[i] = 0xFFFFFFFFu;
    if (n_lines)
        line_start[0] = 0;
    uint32_t line = 0;
    for (uint32_t p = 0; p < limit; ++p)
        if (text[p] == 10 && ++line < n_lines)
            line_start[line] = p + 1;
    for (uint32_t i = 0; i < n_lines; ++i)
        out[3] += line_start[i] == 0xFFFFFFFFu;
    line = 0;
    for (uint32_t p = 0; p < limit; p += 16) {
        const uint32_t n_in = limit - p < 16u ? limit - p : 16u;
        uint32_t nl = 0, cr = 0, low = 0;
        for (uint32_t j = 0; j < 16; ++j) { // (the kernels' loads stage the bytes behind the limit as 0: "low" until rq_lane masks them)
            const uint32_t c = j < n_in ? text[p + j] : 0u;
            nl |= (c == 10 ? 1u : 0u) << j;
            cr |= (c == 13 ? 1u : 0u) << j;
            low |= (c < thresh ? 1u : 0u) << j;
        }
        out[0] += rq_lane(text, p, n_in, nl, cr, low, line, n_lines, line_start, exempt, text_base,
                          [&](uint32_t word, uint32_t bits) {
                              if (word < dead_words)
                                  dead[word] |= bits;
                              else
                                  ++out[2];
                          },
                          [&](uint32_t at) {
                              if (out[1] < 0 || (int64_t)at < out[1])
                                  out[1] = (int64_t)at;
                          });
        line += (uint32_t)__builtin_popcount(nl & (n_in >= 16u ? 0xFFFFu : (1u << n_in) - 1u));
    }
}
