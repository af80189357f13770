// tests/bam_fastq_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_bam_fastq_on_the_cpu.py):
//   bam_fastq_san <inflated BAM bytes> <output> <out bytes expected> <excl> <incl> <min_mapq> <keep_unplaced> <orig> <suffix> <lanes>
//                 <n_regions> [ref beg end ...] [cut ...]
// writes the named FASTQ of the selected records to <output> — a buffer of exactly the expected size: a store past it is caught —
// and prints "rc records excluded no_qual reversed replaced".
#include "bam_fastq_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 12)
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
    const uint64_t want = strtoull(argv[3], nullptr, 10);
    uint32_t opt[8] = {(uint32_t)strtoul(argv[4], nullptr, 0), (uint32_t)strtoul(argv[5], nullptr, 0), (uint32_t)strtoul(argv[6], nullptr, 0),
                       (uint32_t)strtoul(argv[11], nullptr, 0), (uint32_t)strtoul(argv[7], nullptr, 0), (uint32_t)strtoul(argv[8], nullptr, 0),
                       (uint32_t)strtoul(argv[9], nullptr, 0), (uint32_t)strtoul(argv[10], nullptr, 0)};
    int at = 12;
    std::vector<int64_t> regions;
    for (uint32_t i = 0; i < 3 * opt[3] && at < argc; ++i)
        regions.push_back(strtoll(argv[at++], nullptr, 10));
    if (regions.size() != 3ull * opt[3])
        return 2;
    std::vector<uint64_t> cuts;
    for (; at < argc; ++at)
        cuts.push_back(strtoull(argv[at], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> exact(data); // (exactly the stream's size: a read past its end is caught)
    std::vector<uint8_t> out(want);
    uint64_t out_n = 0, st[10];
    const int rc = bam_fastq_cpu(exact.data(), exact.size(), cuts.data(), (int)cuts.size(), opt, regions.data(), out.data(), out.size(),
                                 &out_n, st);
    FILE *o = fopen(argv[2], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, rc == 0 ? out_n : 0, o);
    fclose(o);
    printf("%d %llu %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[7],
           (unsigned long long)st[8], (unsigned long long)st[9]);
    return 0;
}
