// The line -> record and run-folding arithmetic of csrc/kmm_read_hits.hpp under AddressSanitizer + UndefinedBehaviorSanitizer, as
// a stand-alone executable (tests/test_record_hits_on_the_cpu.py builds and runs it; nothing sanitized is loaded into Python).
// usage: record_hits_san TEXT.bin MASKS.bin PERIOD_SHIFT LANE   — TEXT.bin: the consumed bytes of a chunk, MASKS.bin: one byte
// per position (bit 0 a window, bit 1 a hit); every buffer on the heap, exactly its size.
// Prints "ok <bytes> <records> <mismatches> <outside>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "record_hits_cpu_driver.hpp"

static std::unique_ptr<uint8_t[]> slurp(const char *path, int64_t *n)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return nullptr;
    fseek(f, 0, SEEK_END);
    *n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[(size_t)*n]);
    const bool ok = fread(buf.get(), 1, (size_t)*n, f) == (size_t)*n;
    fclose(f);
    return ok ? std::move(buf) : nullptr;
}

int main(int argc, char **argv)
{
    if (argc != 5)
        return 2;
    int64_t n = 0, n_masks = 0;
    std::unique_ptr<uint8_t[]> text = slurp(argv[1], &n), masks = slurp(argv[2], &n_masks);
    if (!text || !masks || n != n_masks || n < 1)
        return 2;
    const uint32_t shift = (uint32_t)atoi(argv[3]);
    const int64_t lane = atoll(argv[4]);
    int64_t lines = 0;
    for (int64_t p = 0; p < n; ++p)
        lines += text[(size_t)p] == 10;
    const int64_t n_records = lines >> shift;
    if (n_records < 1 || (n_records << shift) != lines || text[(size_t)n - 1] != 10)
        return 2; // (the consumed bytes end with the newline of a whole record)
    std::unique_ptr<uint32_t[]> gh(new uint32_t[(size_t)n_records]()), gw(new uint32_t[(size_t)n_records]()),
        wh(new uint32_t[(size_t)n_records]()), ww(new uint32_t[(size_t)n_records]());
    const int64_t outside = record_hits_fold_cpu(text.get(), n, masks.get(), shift, lane, n_records, gh.get(), gw.get());
    record_hits_fold_brute(text.get(), n, masks.get(), shift, wh.get(), ww.get());
    int64_t bad = 0;
    for (int64_t r = 0; r < n_records; ++r)
        bad += gh[(size_t)r] != wh[(size_t)r] || gw[(size_t)r] != ww[(size_t)r];
    printf("ok %lld %lld %lld %lld\n", (long long)n, (long long)n_records, (long long)bad, (long long)outside);
    return bad || outside ? 1 : 0;
}
