// tests/strand_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_strand_on_the_cpu.py):
//   strand_san bam|sam <input bytes> <output> <exclude flags> <qual 0|1> <original_strand 0|1> <lanes> [cut ...]
// writes the text of the kept records to <output> and prints "rc records excluded without_qual reversed".
#include "strand_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 8)
        return 2;
    const bool bam = !strcmp(argv[1], "bam");
    FILE *f = fopen(argv[2], "rb");
    if (!f)
        return 2;
    std::vector<uint8_t> data;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0)
        data.insert(data.end(), buf, buf + got);
    fclose(f);
    std::vector<uint64_t> cuts;
    for (int i = 8; i < argc; ++i)
        cuts.push_back(strtoull(argv[i], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> exact(data); // (exactly the stream's size: a read past its end is caught)
    std::vector<uint8_t> out(3 * data.size() + 64);
    uint64_t out_n = 0, st[6] = {0, 0, 0, 0, 0, 0};
    const uint32_t excl = (uint32_t)strtoul(argv[4], nullptr, 0), lanes = (uint32_t)strtoul(argv[7], nullptr, 10);
    const int qual = atoi(argv[5]), orig = atoi(argv[6]);
    const int rc = (bam ? strand_bam_cpu : strand_sam_cpu)(exact.data(), exact.size(), cuts.data(), (int)cuts.size(), excl, qual, orig,
                                                          lanes, out.data(), out.size(), &out_n, st);
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, out_n, o);
    fclose(o);
    printf("%d %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[3],
           (unsigned long long)st[4]);
    return 0;
}
