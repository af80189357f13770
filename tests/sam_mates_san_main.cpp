// tests/sam_mates_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_sam_mates_on_the_cpu.py; host code only):
//   sam_mates_san run <input bytes> <output> <job> [cut ...]
//   sam_mates_san names <lanes> <max length>
// <job>: a binary file — uint32 exclude flags, mode, original_strand, lanes, min_hits, min_permille, invert, pair rule, fill;
// uint64 tail0, kept bytes expected, n entries; uint32 hits[n]; uint32 windows[n]; then the tables of select_san_main.cpp: uint64
// rules[4], int64 iv[3 n], uint32 n_names, uint32 name_off[n_names + 1], the name bytes.
// run writes the kept bytes to <output> and prints "rc records excluded headers kept_bytes kept_records entries waiting
// stranger_pair"; names prints the number of verdicts that failed.  Every buffer has exactly its size.
#include "sam_mates_cpu_driver.hpp"

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

template <class T>
static bool take(const std::vector<uint8_t> &b, size_t &at, size_t n, std::vector<T> &out)
{
    if (b.size() < at + n * sizeof(T))
        return false;
    out.resize(n);
    if (n)
        memcpy(out.data(), b.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return true;
}

int main(int argc, char **argv)
{
    if (argc == 4 && !strcmp(argv[1], "names")) {
        printf("%llu\n", (unsigned long long)sam_mates_names_sweep((uint32_t)strtoul(argv[2], nullptr, 10), (uint32_t)strtoul(argv[3], nullptr, 10)));
        return 0;
    }
    if (argc < 5 || strcmp(argv[1], "run"))
        return 2;
    std::vector<uint8_t> data, job;
    if (!slurp(argv[2], data) || !slurp(argv[4], job))
        return 2;
    size_t at = 0;
    std::vector<uint32_t> head, hits, windows, n_names, off;
    std::vector<uint64_t> sizes, rules;
    std::vector<int64_t> iv;
    if (!take(job, at, 9, head) || !take(job, at, 3, sizes) || !take(job, at, (size_t)sizes[2], hits) || !take(job, at, (size_t)sizes[2], windows) ||
        !take(job, at, 4, rules) || !take(job, at, 3 * (size_t)rules[3], iv) || !take(job, at, 1, n_names) ||
        !take(job, at, (size_t)n_names[0] + 1, off))
        return 2;
    std::vector<uint8_t> names(job.begin() + (std::ptrdiff_t)at, job.end()); // (exactly the names' size)
    if (names.size() != off[n_names[0]])
        return 2;
    iv.push_back(0); // (never a null pointer)
    if (hits.empty()) {
        hits.push_back(0);
        windows.push_back(0);
    }
    std::vector<uint64_t> cuts;
    for (int i = 5; i < argc; ++i)
        cuts.push_back(strtoull(argv[i], nullptr, 10));
    cuts.push_back(data.size());
    std::vector<uint8_t> out((size_t)sizes[1] + 1);
    uint64_t st[9];
    const int rc = sam_mates_cpu(data.data(), data.size(), cuts.data(), (int)cuts.size(), head[0], (int)head[1], (int)head[2], head[3], rules.data(),
                                 iv.data(), names.data(), off.data(), n_names[0], hits.data(), windows.data(), sizes[2], &head[4], (int)head[8],
                                 sizes[0], out.data(), sizes[1], st);
    FILE *o = fopen(argv[3], "wb");
    if (!o)
        return 2;
    if (rc == 0 && sizes[1])
        fwrite(out.data(), 1, (size_t)sizes[1], o);
    fclose(o);
    printf("%d %llu %llu %llu %llu %llu %llu %llu %llu\n", rc, (unsigned long long)st[0], (unsigned long long)st[1], (unsigned long long)st[2],
           (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)st[6], (unsigned long long)st[7]);
    return 0;
}
