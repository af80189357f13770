// tests/bam_resync_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer
// (tests/test_bam_resync_on_the_cpu.py):
//   bam_resync_san every <inflated bytes> <from> <len> <n_ref> <output>     the lowest holding position for every boundary byte
//                                                                           (uint64 each, little endian) into <output>
//   bam_resync_san one <inflated bytes> <whole> <cap> <n_ref> <member size>  one window cut into members of that many inflated
//                                                                           bytes (compressed offsets = 10 x the inflated ones);
//                                                                           prints "member skip pos"
// The bytes are held in a buffer of exactly their size: a read past the end is caught.
#include "bam_resync_cpu_driver.hpp"

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
    if (argc < 7)
        return 2;
    std::vector<uint8_t> in;
    if (!slurp(argv[2], in))
        return 2;
    std::vector<uint8_t> data(in.begin(), in.end()); // (capacity == size)
    if (!strcmp(argv[1], "every")) {
        const uint64_t from = strtoull(argv[3], nullptr, 10), len = strtoull(argv[4], nullptr, 10);
        if (from > data.size())
            return 2;
        std::vector<uint64_t> out(data.size() - from);
        bam_resync_every_byte(data.data(), data.size(), from, len, (int32_t)atoi(argv[5]), out.data());
        FILE *o = fopen(argv[6], "wb");
        if (!o)
            return 2;
        fwrite(out.data(), 8, out.size(), o);
        fclose(o);
        return 0;
    }
    const uint64_t msize = strtoull(argv[6], nullptr, 10);
    if (!msize)
        return 2;
    std::vector<unsigned long long> m_off{0ull}, o_off{0ull};
    while (o_off.back() < data.size()) {
        const unsigned long long e = o_off.back() + msize < data.size() ? o_off.back() + msize : data.size();
        o_off.push_back(e);
        m_off.push_back(10ull * e);
    }
    int64_t member = 0, skip = 0;
    uint64_t pos = 0;
    bam_resync_cpu(data.data(), data.size(), m_off.data(), o_off.data(), m_off.size() - 1, atoi(argv[3]), strtoull(argv[4], nullptr, 10),
                   (int32_t)atoi(argv[5]), &member, &skip, &pos);
    printf("%lld %lld %llu\n", (long long)member, (long long)skip, (unsigned long long)pos);
    return 0;
}
