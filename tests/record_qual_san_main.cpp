// tests/record_qual_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_record_qual_on_the_cpu.py):
//   record_qual_san bam|sam <input bytes> <output> <exclude flags> [cut ...]
// writes the four-line FASTQ of the kept records to <output> and prints "rc records excluded without_qual error".
#include "record_qual_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 5)
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
    for (int i = 5; i < argc; ++i)
        cuts.push_back(strtoull(argv[i], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> exact(data); // (exactly the stream's size: a read past its end is caught)
    std::vector<uint8_t> out(3 * data.size() + 64);
    uint64_t out_n = 0, st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint32_t excl = (uint32_t)strtoul(argv[4], nullptr, 0);
    const int rc = bam ? bam_qual_cpu(exact.data(), exact.size(), cuts.data(), (int)cuts.size(), excl, out.data(), out.size(), &out_n, st)
                       : sam_qual_cpu(exact.data(), exact.size(), cuts.data(), (int)cuts.size(), excl, out.data(), out.size(), &out_n, st);
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, out_n, o);
    fclose(o);
    printf("%d %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[bam ? 7 : 5],
           (unsigned long long)st[bam ? 6 : 4]);
    return 0;
}
