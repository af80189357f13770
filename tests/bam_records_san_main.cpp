// tests/bam_records_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_bam_records_on_the_cpu.py):
//   bam_records_san <inflated BAM bytes> <entries: n x uint32 hits, then n x uint32 windows> <output> <out bytes expected> <excl> <incl>
//                   <min_mapq> <keep_unplaced> <lanes> <min_hits> <min_permille> <invert> <n_regions> [ref beg end ...] [cut ...]
// writes the kept records' raw bytes to <output> — the driver's queue has exactly the expected size: a store past it is caught —
// and prints "rc selected excluded kept_records"; then every copy of 1 .. 40 bytes at every source and destination residue.
#include "bam_records_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool slurp(const char *path, std::vector<uint8_t> &data)
{
    FILE *f = fopen(path, "rb");
    if (!f)
        return false;
    uint8_t buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0)
        data.insert(data.end(), buf, buf + got);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc < 14)
        return 2;
    std::vector<uint8_t> data, ent;
    if (!slurp(argv[1], data) || !slurp(argv[2], ent) || ent.size() % 8 != 0)
        return 2;
    const uint64_t n_entries = ent.size() / 8;
    std::vector<uint32_t> hits(n_entries + 1), windows(n_entries + 1); // (+ 1: never an empty vector's null data())
    if (n_entries) {
        memcpy(hits.data(), ent.data(), n_entries * 4);
        memcpy(windows.data(), ent.data() + n_entries * 4, n_entries * 4);
    }
    hits.resize(n_entries ? n_entries : 1);
    windows.resize(n_entries ? n_entries : 1);
    const uint64_t want = strtoull(argv[4], nullptr, 10);
    uint32_t opt[10] = {(uint32_t)strtoul(argv[5], nullptr, 0),  (uint32_t)strtoul(argv[6], nullptr, 0),  (uint32_t)strtoul(argv[7], nullptr, 0),
                        (uint32_t)strtoul(argv[13], nullptr, 0), (uint32_t)strtoul(argv[8], nullptr, 0),  (uint32_t)strtoul(argv[9], nullptr, 0),
                        (uint32_t)strtoul(argv[10], nullptr, 0), (uint32_t)strtoul(argv[11], nullptr, 0), (uint32_t)strtoul(argv[12], nullptr, 0),
                        0xA5u};
    int at = 14;
    std::vector<int64_t> regions;
    for (uint32_t i = 0; i < 3 * opt[3] && at < argc; ++i)
        regions.push_back(strtoll(argv[at++], nullptr, 10));
    if (regions.size() != 3ull * opt[3])
        return 2;
    regions.push_back(0);
    std::vector<uint64_t> cuts;
    for (; at < argc; ++at)
        cuts.push_back(strtoull(argv[at], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> exact(data); // (exactly the stream's size: a read past its end is caught)
    std::vector<uint8_t> out(want + 1);
    uint64_t out_n = 0, st[6];
    const int rc = bam_records_cpu(exact.data(), exact.size(), cuts.data(), (int)cuts.size(), opt, regions.data(), hits.data(), windows.data(),
                                   n_entries, out.data(), want, 0, &out_n, st);
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, rc == 0 ? out_n : 0, o);
    fclose(o);
    printf("%d %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2]);
    std::vector<uint32_t> writes(64);
    for (uint32_t len = 1; len <= 40; ++len)
        for (uint32_t sa = 0; sa < 16; ++sa)
            for (uint32_t da = 0; da < 16; ++da) {
                if (bam_records_copy_writes(len, sa, da, opt[5], writes.data()) != 0)
                    return 3;
                for (uint32_t i = 0; i < len; ++i)
                    if (writes[i] != 1)
                        return 4;
            }
    return 0;
}
