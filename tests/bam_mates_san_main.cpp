// tests/bam_mates_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_bam_mates_on_the_cpu.py):
//   bam_mates_san <inflated BAM bytes> <entries: n x uint32 hits, then n x uint32 windows> <output> <out bytes expected> <excl> <incl>
//                 <min_mapq> <keep_unplaced> <lanes> <min_hits> <min_permille> <invert> <pair_rule> <n_regions> [ref beg end ...] [cut ...]
// runs the walk, the name check and the carry copy over the stream in its windows, writes the kept pairs' raw bytes to <output> —
// the driver's queue has exactly the expected size: a store past it is caught — and prints "rc selected excluded kept_records
// ordinal window"; then the name comparison at every length up to 255 with a difference at every byte.
#include "bam_mates_cpu_driver.hpp"

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
    if (argc < 15)
        return 2;
    std::vector<uint8_t> data, ent;
    if (!slurp(argv[1], data) || !slurp(argv[2], ent) || ent.size() % 8 != 0)
        return 2;
    const uint64_t n_entries = ent.size() / 8;
    std::vector<uint32_t> hits(n_entries ? n_entries : 1), windows(n_entries ? n_entries : 1);
    if (n_entries) {
        memcpy(hits.data(), ent.data(), n_entries * 4);
        memcpy(windows.data(), ent.data() + n_entries * 4, n_entries * 4);
    }
    const uint64_t want = strtoull(argv[4], nullptr, 10);
    auto u = [&](int i) { return (uint32_t)strtoul(argv[i], nullptr, 0); };
    uint32_t opt[11] = {u(5), u(6), u(7), u(14), u(8), u(9), u(10), u(11), u(12), 0xA5u, u(13)};
    int at = 15;
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
    uint64_t out_n = 0, st[8];
    const int rc = bam_mates_cpu(exact.data(), exact.size(), cuts.data(), (int)cuts.size(), opt, regions.data(), hits.data(), windows.data(),
                                 n_entries, out.data(), want, 0, &out_n, st);
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, out_n <= want ? out_n : 0, o);
    fclose(o);
    printf("%d %llu %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
           (unsigned long long)st[6], (unsigned long long)st[7]);
    for (uint32_t l = 1; l <= 255; ++l) {
        std::vector<uint8_t> a(l), b;
        for (uint32_t i = 0; i + 1 < l; ++i)
            a[i] = (uint8_t)(33 + i % 90);
        b = a;
        if (bam_mates_names_differ(a.data(), l, b.data(), l, opt[5]) != 0)
            return 3;
        for (uint32_t i = 0; i + 1 < l; ++i) {
            b[i] ^= 1;
            if (bam_mates_names_differ(a.data(), l, b.data(), l, opt[5]) != 1)
                return 4;
            b[i] ^= 1;
        }
        if (l > 1 && bam_mates_names_differ(a.data(), l, a.data() + 1, l - 1, opt[5]) != 1)
            return 5;
    }
    return 0;
}
