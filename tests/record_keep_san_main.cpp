// The line -> record, keep-rule, clipping and destination arithmetic of csrc/kmm_record_keep.hpp under AddressSanitizer +
// UndefinedBehaviorSanitizer, as a stand-alone executable (tests/test_record_keep_on_the_cpu.py builds and runs it; nothing
// sanitized is loaded into Python).
// usage: record_keep_san TEXT.bin ENTRIES.bin PERIOD_SHIFT MIN_HITS MIN_PERMILLE INVERT TAIL [LANE_MASKS.bin]
// TEXT.bin: a chunk (its last record may be incomplete); ENTRIES.bin: uint32 hits of its whole records, then their windows;
// TAIL: where the queue's pending bytes end.  LANE_MASKS.bin (uint16 per 16 bytes): the scatter alone, on these masks instead
// of the rule's.  Every buffer on the heap, exactly its size.
// Prints "ok <bytes> <consumed> <kept bytes> <kept records> <mismatches> <outside> <twice or missed>".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "record_keep_cpu_driver.hpp"

static std::unique_ptr<uint8_t[]> slurp(const char *path, int64_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return nullptr;
    fseek(f, 0, SEEK_END);
    *n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)*n + 1]); // (+1: an empty file still gets an array)
    const bool ok = fread(buf.get(), 1, (size_t)*n, f) == (size_t)*n;
    fclose(f);
    if (!ok)
        return nullptr;
    std::unique_ptr<uint8_t[]> exact(new uint8_t[(size_t)(*n > 0 ? *n : 1)]);
    for (int64_t i = 0; i < *n; ++i)
        exact[(size_t)i] = buf[(size_t)i];
    return exact;
}

int main(int argc, char **argv)
{
    if (argc != 8 && argc != 9)
        return 2;
    int64_t n = 0, n_entries = 0, n_masks = 0;
    std::unique_ptr<uint8_t[]> text = slurp(argv[1], &n), entries = slurp(argv[2], &n_entries), lane_masks;
    if (!text || !entries || n < 1)
        return 2;
    const uint32_t shift = (uint32_t)atoi(argv[3]), min_hits = (uint32_t)strtoul(argv[4], nullptr, 10),
                   min_permille = (uint32_t)atoi(argv[5]), invert = (uint32_t)atoi(argv[6]);
    const int64_t tail = atoll(argv[7]);
    int64_t lines = 0, consumed = 0;
    for (int64_t p = 0; p < n; ++p)
        if (text[(size_t)p] == 10 && (++lines & ((1 << shift) - 1)) == 0)
            consumed = p + 1;
    const int64_t n_records = lines >> shift;
    if (n_entries != n_records * 8 || tail < 0)
        return 2;
    std::unique_ptr<uint32_t[]> hw(new uint32_t[(size_t)(2 * n_records + 1)]);
    memcpy(hw.get(), entries.get(), (size_t)n_entries);
    const uint32_t *hits = hw.get(), *windows = hw.get() + n_records;
    int64_t stats[5] = {0, 0, 0, 0, 0}, want_records = 0, want = 0, bad = 0;
    if (argc == 9) {
        lane_masks = slurp(argv[8], &n_masks);
        if (!lane_masks || n_masks != (n + 15) / 16 * 2)
            return 2;
        std::unique_ptr<uint16_t[]> m(new uint16_t[(size_t)(n_masks / 2)]);
        memcpy(m.get(), lane_masks.get(), (size_t)n_masks);
        std::unique_ptr<uint8_t[]> brute(new uint8_t[(size_t)n]);
        for (int64_t p = 0; p < n; ++p)
            if ((m[(size_t)(p / 16)] >> (p % 16)) & 1u)
                brute[(size_t)want++] = text[(size_t)p];
        const int64_t cap = tail + want; // (exactly what is needed: a store behind it is a heap overflow)
        std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(cap > 0 ? cap : 1)]());
        record_keep_scatter_cpu(text.get(), n, m.get(), tail, out.get(), cap, stats);
        bad += stats[0] != want;
        for (int64_t i = 0; i < want && stats[0] == want; ++i)
            bad += out[(size_t)(tail + i)] != brute[(size_t)i];
    } else {
        std::unique_ptr<uint8_t[]> brute(new uint8_t[(size_t)(consumed > 0 ? consumed : 1)]);
        want = record_keep_brute(text.get(), consumed, shift, hits, windows, min_hits, min_permille, invert, brute.get(), &want_records);
        const int64_t cap = tail + want;
        std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(cap > 0 ? cap : 1)]());
        record_keep_cpu(text.get(), n, consumed, shift, hits, windows, n_records, min_hits, min_permille, invert, tail, out.get(), cap,
                        stats);
        bad += stats[0] != want || stats[1] != want_records || stats[4] != 0;
        for (int64_t i = 0; i < want && stats[0] == want; ++i)
            bad += out[(size_t)(tail + i)] != brute[(size_t)i];
    }
    printf("ok %lld %lld %lld %lld %lld %lld %lld\n", (long long)n, (long long)consumed, (long long)stats[0], (long long)stats[1],
           (long long)bad, (long long)stats[2], (long long)stats[3]);
    return bad || stats[2] || stats[3] ? 1 : 0;
}
