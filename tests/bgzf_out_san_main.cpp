// csrc/kmm_bgzf_out.hpp under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone executable
// (tests/test_bgzf_out_on_the_cpu.py builds and runs it; nothing sanitized is loaded into Python).
// usage: bgzf_out_san TEXT.bin OUT.bin
// TEXT.bin: the text; OUT.bin: its BGZF members (no EOF block).  Every buffer on the heap, exactly its size.
// Prints "ok <bytes in> <bytes out> <members> <deepest code> <limited> <stored>".
#include <cstdio>
#include <cstdlib>

#include "bgzf_out_cpu_driver.hpp"

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
    const int64_t cap = kmm_bz::bound(n), n_members = kmm_bz::member_count(n);
    std::unique_ptr<uint8_t[]> out(new uint8_t[(size_t)(cap > 0 ? cap : 1)]);
    std::unique_ptr<uint32_t[]> sizes(new uint32_t[(size_t)(n_members > 0 ? n_members : 1)]);
    uint32_t stats[3];
    if (n > 0 && bgzf_out_compress(text.get(), n, out.get(), cap - 1, sizes.get(), stats) != -1)
        return 3; // (one byte short of the bound is refused)
    const int64_t got = bgzf_out_compress(text.get(), n, out.get(), cap, sizes.get(), stats);
    if (got < 0 || got > cap)
        return 3;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.get(), 1, (size_t)got, f) != (size_t)got)
        return 2;
    fclose(f);
    printf("ok %lld %lld %lld %u %u %u\n", (long long)n, (long long)got, (long long)n_members, stats[0], stats[1], stats[2]);
    return 0;
}
