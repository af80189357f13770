// tests/test_record_hits_qual_on_the_cpu.py: the mark pass of csrc/kmm_rh_qual.hpp under ASan + UBSan, as a program of its own
// (host code; nothing sanitized is loaded into Python).  argv: text file, limit, n_lines, thresh.  The text, the line starts and
// the bitset live in heap buffers of exactly their size.  Prints "ok <low bytes> <malformed offset> <outside> <unwritten>
// <set bits>".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "record_hits_qual_cpu_driver.hpp"

int main(int argc, char **argv)
{
    if (argc != 5)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> all;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
        all.insert(all.end(), buf, buf + n);
    fclose(f);
    const uint32_t limit = (uint32_t)strtoul(argv[2], nullptr, 10), n_lines = (uint32_t)strtoul(argv[3], nullptr, 10),
                   thresh = (uint32_t)strtoul(argv[4], nullptr, 10);
    if (limit > all.size())
        return 2;
    uint8_t *text = (uint8_t *)malloc(limit ? limit : 1);
    for (uint32_t i = 0; i < limit; ++i)
        text[i] = all[i];
    const uint32_t dead_words = (limit + 31) / 32;
    uint32_t *line_start = (uint32_t *)malloc((n_lines ? n_lines : 1) * sizeof(uint32_t));
    uint32_t *dead = (uint32_t *)calloc(dead_words ? dead_words : 1, sizeof(uint32_t));
    int64_t out[4];
    rq_mark_cpu(text, limit, n_lines, thresh, nullptr, 0, line_start, dead, dead_words, out);
    long long bits = 0;
    for (uint32_t i = 0; i < dead_words; ++i)
        bits += __builtin_popcount(dead[i]);
    printf("ok %lld %lld %lld %lld %lld\n", (long long)out[0], (long long)out[1], (long long)out[2], (long long)out[3], bits);
    free(text);
    free(line_start);
    free(dead);
    return 0;
}
