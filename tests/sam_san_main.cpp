// tests/sam_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_sam_on_the_cpu.py):
//   sam_san <SAM bytes> <output> <exclude flags> [cut ...]
// writes the two-line FASTA of the kept records to <output> and prints "rc records excluded header_lines calls error".
#include "sam_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 4)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> data;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0)
        data.insert(data.end(), buf, buf + got);
    fclose(f);
    std::vector<uint64_t> cuts;
    for (int i = 4; i < argc; ++i)
        cuts.push_back(strtoull(argv[i], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> out(data.size() + 16);
    uint64_t out_n = 0, st[5];
    const int rc = sam_cpu(data.data(), data.size(), cuts.data(), (int)cuts.size(), (uint32_t)strtoul(argv[3], nullptr, 0), out.data(),
                           out.size(), &out_n, st);
    FILE *o = fopen(argv[2], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, out_n, o);
    fclose(o);
    printf("%d %llu %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
           (unsigned long long)st[3], (unsigned long long)st[4]);
    return 0;
}
