// The pair rule, the pair form of the lane mask and the line search of the cut (csrc/kmm_record_keep.hpp,
// csrc/kmm_line_search.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone executable
// (tests/test_record_pairs_on_the_cpu.py builds and runs it; nothing sanitized is loaded into Python).
// usage: record_pairs_san TEXT.bin ENTRIES.bin PERIOD_SHIFT PAIR_SHIFT MIN_HITS MIN_PERMILLE INVERT PAIR_RULE TAIL
// TEXT.bin: a piece that starts at a pair's first record (PAIR_SHIFT 1: interleaved) or one mate's buffer (PAIR_SHIFT 0), its
// end may hold records without a whole pair; ENTRIES.bin: uint32 hits of its pairs, two per pair, then their windows; TAIL:
// where the queue's pending bytes end.  Every buffer on the heap, exactly its size.
// Prints "ok <bytes> <consumed> <kept bytes> <kept records> <mismatches> <outside> <twice or missed> <lanes tried> <cuts tried>".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "record_pairs_cpu_driver.hpp"

static std::unique_ptr<uint8_t[]> slurp(const char *path, int64_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return nullptr;
    fseek(f, 0, SEEK_END);
    *n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<uint8_t[]> exact(new uint8_t[(size_t)(*n > 0 ? *n : 1)]);
    const bool ok = fread(exact.get(), 1, (size_t)*n, f) == (size_t)*n;
    fclose(f);
    if (!ok)
        return nullptr;
    return exact;
}

int main(int argc, char **argv)
{
    if (argc != 10)
        return 2;
    int64_t n = 0, n_entries = 0;
    std::unique_ptr<uint8_t[]> text = slurp(argv[1], &n), entries = slurp(argv[2], &n_entries);
    if (!text || !entries || n < 1)
        return 2;
    const uint32_t shift = (uint32_t)atoi(argv[3]), pair_shift = (uint32_t)atoi(argv[4]), min_hits = (uint32_t)strtoul(argv[5], nullptr, 10),
                   min_permille = (uint32_t)atoi(argv[6]), invert = (uint32_t)atoi(argv[7]), pair_rule = (uint32_t)atoi(argv[8]);
    const int64_t tail = atoll(argv[9]);
    if (n_entries % 16 != 0 || tail < 0 || pair_shift > 1)
        return 2;
    const int64_t n_pairs = n_entries / 16, n_records = n_pairs << pair_shift; // (records of this text that belong to whole pairs)
    int64_t lines = 0, consumed = 0, total_lines = 0;
    for (int64_t p = 0; p < n; ++p)
        if (text[(size_t)p] == 10) {
            ++total_lines;
            if (lines < (n_records << shift) && ++lines == (n_records << shift))
                consumed = p + 1;
        }
    if (lines != (n_records << shift))
        return 2;
    std::unique_ptr<uint32_t[]> hw(new uint32_t[(size_t)(4 * n_pairs + 1)]);
    memcpy(hw.get(), entries.get(), (size_t)n_entries);
    const uint32_t *hits = hw.get(), *windows = hw.get() + 2 * n_pairs;
    int64_t stats[5] = {0, 0, 0, 0, 0}, want_records = 0, bad = 0;
    std::unique_ptr<uint8_t[]> brute(new uint8_t[(size_t)(consumed > 0 ? consumed : 1)]);
    const int64_t want = record_pairs_brute(text.get(), consumed, shift, pair_shift, hits, windows, min_hits, min_permille, invert, pair_rule,
                                            brute.get(), &want_records);
    const int64_t cap = tail + want; // (exactly what is needed: a store behind it is a heap overflow)
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(cap > 0 ? cap : 1)]());
    record_pairs_cpu(text.get(), n, consumed, shift, pair_shift, hits, windows, n_records, min_hits, min_permille, invert, pair_rule, tail,
                     out.get(), cap, stats);
    bad += stats[0] != want || stats[1] != want_records || stats[4] != 0;
    for (int64_t i = 0; i < want && stats[0] == want; ++i)
        bad += out[(size_t)(tail + i)] != brute[(size_t)i];
    // lanes with newline masks no text produces, at lines and piece positions around the end of the whole pairs
    int64_t lanes = 0;
    uint32_t x = 12345u;
    const uint32_t n_lines = (uint32_t)(n_records << shift);
    for (int i = 0; i < 2000 && n_pairs > 0; ++i) {
        x = x * 1664525u + 1013904223u;
        uint32_t nl = (x >> 8) & 0xFFFFu;
        if (i % 5 == 0)
            nl = i % 10 ? 0xFFFFu : 0u;
        x = x * 1664525u + 1013904223u;
        const uint32_t line0 = (x >> 4) % (n_lines + 3);
        x = x * 1664525u + 1013904223u;
        const int64_t p0 = 16 * (int64_t)((x >> 4) % 64), end = p0 + (int64_t)((x >> 12) % 40) - 12;
        uint32_t got[3] = {0, 0, 0};
        record_pairs_lane_cpu(line0, nl, shift, pair_shift, p0, end, hits, windows, n_records, min_hits, min_permille, invert, pair_rule, got);
        bad += got[0] != got[1];
        ++lanes;
    }
    // the cut behind every line that ends a record, and the targets no slot holds
    int64_t cuts = 0;
    for (uint32_t target = 0; target <= (uint32_t)total_lines + 2; target += (target < 64 || target + 64 > (uint32_t)total_lines ? 1 : 37)) {
        bad += record_pairs_cut_cpu(text.get(), n, target) != record_pairs_cut_brute(text.get(), n, target);
        ++cuts;
    }
    printf("ok %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)n, (long long)consumed, (long long)stats[0], (long long)stats[1],
           (long long)bad, (long long)stats[2], (long long)stats[3], (long long)lanes, (long long)cuts);
    return bad || stats[2] || stats[3] ? 1 : 0;
}
