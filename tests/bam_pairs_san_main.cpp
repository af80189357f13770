// The mate check's plain-C++ arithmetic (csrc/kmm_record_keep.hpp: rk_name_trim, rk_names_equal, rk_mate2_line) under
// AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone executable (tests/test_bam_pairs_on_the_cpu.py builds and runs
// it; nothing sanitized is loaded into Python).
// usage: bam_pairs_san TEXT.bin MATE_SUFFIX
// TEXT.bin: whole pairs of four-line FASTQ, on the heap in a buffer of exactly its size — a read behind the text is caught.
// Prints "ok <bytes> <pairs> <first stranger or -1> <bytes compared>".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "bam_pairs_cpu_driver.hpp"

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    fseek(f, 0, SEEK_END);
    const int64_t n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::unique_ptr<uint8_t[]> text(new uint8_t[(size_t)(n > 0 ? n : 1)]);
    const bool ok = fread(text.get(), 1, (size_t)n, f) == (size_t)n;
    fclose(f);
    if (!ok)
        return 2;
    int64_t stats[2] = {0, 0};
    const int64_t first = bam_pairs_check_cpu(text.get(), n, (uint32_t)atoi(argv[2]), stats);
    if (first == -2)
        return 1;
    // names at the very end of a heap block: the trim looks two bytes back, never ahead
    for (uint32_t len = 0; len < 6; ++len) {
        std::unique_ptr<uint8_t[]> a(new uint8_t[len ? len : 1]), b(new uint8_t[len ? len : 1]);
        for (uint32_t i = 0; i < len; ++i)
            a[i] = b[i] = (uint8_t)(i + 1 == len ? '1' : '/');
        if (!rk_names_equal(a.get(), len, b.get(), len, true) || rk_name_trim(a.get(), len, true) != (len >= 2 ? len - 2 : len))
            return 1;
    }
    printf("ok %lld %lld %lld %lld\n", (long long)n, (long long)stats[0], (long long)first, (long long)stats[1]);
    return 0;
}
