// tests/select_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_record_select_on_the_cpu.py):
//   select_san bam|sam <input bytes> <output> <tables> <exclude flags> <qual 0|1> <original_strand 0|1> <lanes> [cut ...]
// <tables>: a binary file — uint64 rules[4] (include mask, MAPQ floor, keep_unplaced, n intervals), int64 iv[3 n], uint32 n_names,
// uint32 name_off[n_names + 1], the name bytes.  Writes the text of the kept records to <output> and prints
// "rc records excluded without_qual reversed".
#include "select_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (argc < 9)
        return 2;
    const bool bam = !strcmp(argv[1], "bam");
    std::vector<uint8_t> data, tb;
    if (!slurp(argv[2], data) || !slurp(argv[4], tb) || tb.size() < 36)
        return 2;
    uint64_t rules[4];
    memcpy(rules, tb.data(), 32);
    std::vector<int64_t> iv(3 * rules[3] + 1);
    if (tb.size() < 36 + 24 * rules[3])
        return 2;
    memcpy(iv.data(), tb.data() + 32, 24 * rules[3]);
    uint32_t n_names = 0;
    size_t at = 32 + 24 * rules[3];
    memcpy(&n_names, tb.data() + at, 4);
    at += 4;
    std::vector<uint32_t> off(n_names + 1);
    if (tb.size() < at + 4 * off.size())
        return 2;
    memcpy(off.data(), tb.data() + at, 4 * off.size());
    at += 4 * off.size();
    std::vector<uint8_t> names(tb.begin() + (std::ptrdiff_t)at, tb.end()); // (exactly the names' size)
    if (names.size() != off[n_names])
        return 2;
    std::vector<uint64_t> cuts;
    for (int i = 9; i < argc; ++i)
        cuts.push_back(strtoull(argv[i], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> out(3 * data.size() + 64);
    uint64_t out_n = 0, st[7] = {0, 0, 0, 0, 0, 0, 0};
    const uint32_t excl = (uint32_t)strtoul(argv[5], nullptr, 0), lanes = (uint32_t)strtoul(argv[8], nullptr, 10);
    const int qual = atoi(argv[6]), orig = atoi(argv[7]);
    const int rc = bam ? select_bam_cpu(data.data(), data.size(), cuts.data(), (int)cuts.size(), excl, qual, orig, lanes, out.data(),
                                        out.size(), &out_n, st, rules, iv.data())
                       : select_sam_cpu(data.data(), data.size(), cuts.data(), (int)cuts.size(), excl, qual, orig, lanes, out.data(),
                                        out.size(), &out_n, st, rules, iv.data(), names.data(), off.data(), n_names);
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    fwrite(out.data(), 1, out_n, o);
    fclose(o);
    printf("%d %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[3],
           (unsigned long long)st[4]);
    return 0;
}
