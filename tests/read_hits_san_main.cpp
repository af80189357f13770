// The position -> read search of csrc/kmm_read_hits.hpp under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone
// executable (tests/test_read_hits_on_the_cpu.py builds and runs it; nothing sanitized is loaded into Python).
// usage: read_hits_san OFFSETS.bin TILE_LEN LANE_LEN   — OFFSETS.bin: int64[n_reads + 1]; every buffer on the heap, exactly
// its size.  Prints "ok <positions> <mismatches> <outside>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "read_hits_cpu_driver.hpp"

int main(int argc, char **argv)
{
    if (argc != 4)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const int64_t n = bytes / 8;
    std::unique_ptr<int64_t[]> offs(new int64_t[(size_t)n]);
    if (fread(offs.get(), 8, (size_t)n, f) != (size_t)n)
        return 2;
    fclose(f);
    const int64_t n_reads = n - 1, total = offs[(size_t)n_reads];
    if (n_reads < 1 || total < 1)
        return 2;
    const int64_t tile_len = atoll(argv[2]), lane_len = atoll(argv[3]);
    std::unique_ptr<int64_t[]> got(new int64_t[(size_t)total]), want(new int64_t[(size_t)total]);
    const int64_t outside = read_hits_search_cpu(offs.get(), n_reads, total, tile_len, lane_len, got.get());
    read_hits_search_brute(offs.get(), n_reads, total, want.get());
    int64_t bad = 0;
    for (int64_t p = 0; p < total; ++p)
        bad += got[(size_t)p] != want[(size_t)p];
    printf("ok %lld %lld %lld\n", (long long)total, (long long)bad, (long long)outside);
    return bad || outside ? 1 : 0;
}
