// Sanitizer run of the plain-gzip pipeline the GPU runs (csrc/kmm_gpu_gunzip.hpp) on the CPU: tests/test_gpu_gunzip_on_the_cpu.py
// builds this with -fsanitize=address,undefined.  gzip streams made by zlib (FASTQ-like data; levels, strategies, concatenated
// members, stored members whose bytes hold real dynamic block headers — false starts) go through the same run_call in windows
// cut anywhere, with a small per-call cap now and then; every window lies in a heap buffer of exactly its size.  Intact
// streams must come out byte for byte; damaged ones (a bit flipped, truncated, garbage behind) must end in an error code or
// in the right bytes — and in no case may anything touch memory outside its buffers.
#include "gunzip_cpu_driver.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include <zlib.h>

static std::vector<uint8_t> gzip_member(const std::vector<uint8_t> &in, int level, int strategy, int wbits = 31)
{
    z_stream z{};
    if (deflateInit2(&z, level, Z_DEFLATED, wbits, 8, strategy) != Z_OK)
        exit(3);
    std::vector<uint8_t> out(deflateBound(&z, (uLong)in.size()) + 64);
    z.next_in = const_cast<Bytef *>(in.data());
    z.avail_in = (uInt)in.size();
    z.next_out = out.data();
    z.avail_out = (uInt)out.size();
    if (deflate(&z, Z_FINISH) != Z_STREAM_END)
        exit(3);
    out.resize(z.total_out);
    deflateEnd(&z);
    return out;
}

// FASTQ-like records; `blob`: bytes to put into every header line (a real dynamic block header: a false start for the search)
static std::vector<uint8_t> fastq(std::mt19937_64 &rng, int n, const std::vector<uint8_t> &blob)
{
    std::vector<uint8_t> v;
    const char *acgt = "ACGT", *q = "FFFFFF:,#";
    for (int i = 0; i < n; ++i) {
        char h[32];
        const int hl = snprintf(h, sizeof h, "@r%d ", i);
        v.insert(v.end(), h, h + hl);
        v.insert(v.end(), blob.begin(), blob.end());
        v.push_back('\n');
        const int len = 50 + (int)(rng() % 150);
        for (int j = 0; j < len; ++j)
            v.push_back((uint8_t)acgt[rng() % 4]);
        v.push_back('\n');
        v.push_back('+');
        v.push_back('\n');
        for (int j = 0; j < len; ++j)
            v.push_back((uint8_t)q[rng() % 9]);
        v.push_back('\n');
    }
    return v;
}

// the first bytes of a non-final dynamic block with no newline among them
static std::vector<uint8_t> dynamic_block_blob()
{
    for (uint32_t seed = 1;; ++seed) {
        std::mt19937_64 r(seed);
        std::vector<uint8_t> d(4000);
        for (auto &c : d)
            c = (uint8_t)"ACGTacgt:#"[r() % 10];
        z_stream z{};
        deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        std::vector<uint8_t> out(8192);
        z.next_in = d.data();
        z.avail_in = (uInt)d.size();
        z.next_out = out.data();
        z.avail_out = (uInt)out.size();
        deflate(&z, Z_FULL_FLUSH);
        deflateEnd(&z);
        out.resize(160);
        bool nl = false;
        for (uint8_t c : out)
            nl = nl || c == '\n';
        if (!nl && (out[0] & 7) == 4)
            return out;
    }
}

static int run(const std::vector<uint8_t> &comp, std::vector<uint64_t> cuts, uint32_t chunk, uint64_t call_cap, std::vector<uint8_t> &out,
               uint64_t *st)
{
    cuts.push_back(comp.size());
    std::vector<uint64_t> c;
    for (uint64_t x : cuts)
        if (x > 0 && x <= comp.size() && (c.empty() || x > c.back()))
            c.push_back(x);
    out.assign(comp.size() * 1100 + 1024, 0);
    uint64_t n_out = 0;
    // (the stream itself in an exact-size buffer too)
    uint8_t *exact = (uint8_t *)malloc(comp.size() ? comp.size() : 1);
    if (comp.size())
        memcpy(exact, comp.data(), comp.size());
    const int rc = gunzip_cpu(exact, comp.size(), c.data(), (int)c.size(), chunk, call_cap, out.data(), out.size(), &n_out, st);
    free(exact);
    out.resize(n_out);
    return rc;
}

int main(int argc, char **argv)
{
    const int rounds = argc > 1 ? atoi(argv[1]) : 40;
    std::mt19937_64 rng(777);
    const std::vector<uint8_t> blob = dynamic_block_blob();
    const int levels[] = {0, 1, 6, 9}, strategies[] = {Z_DEFAULT_STRATEGY, Z_FILTERED, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED};
    long intact = 0, refused = 0, wrong = 0, false_starts = 0, capped = 0;
    for (int r = 0; r < rounds; ++r) {
        const bool fs = r % 4 == 3;
        const std::vector<uint8_t> data = fastq(rng, 300 + (int)(rng() % 1500), fs ? blob : std::vector<uint8_t>());
        // one to three members
        std::vector<uint8_t> comp;
        const int n_mem = 1 + (int)(rng() % 3);
        size_t a = 0;
        for (int m = 0; m < n_mem; ++m) {
            const size_t b = m + 1 == n_mem ? data.size() : a + (size_t)(rng() % (data.size() - a + 1));
            const std::vector<uint8_t> part(data.begin() + (long)a, data.begin() + (long)b);
            const std::vector<uint8_t> g = gzip_member(part, fs ? 0 : levels[rng() % 4], strategies[rng() % 5]);
            comp.insert(comp.end(), g.begin(), g.end());
            a = b;
        }
        const uint32_t chunk = (uint32_t)1024 << (rng() % 6);
        std::vector<uint64_t> cuts;
        for (int k = (int)(rng() % 5); k > 0; --k)
            cuts.push_back(rng() % (comp.size() + 1));
        std::sort(cuts.begin(), cuts.end());
        const uint64_t call_cap = r % 3 == 1 ? 20000 + rng() % 60000 : (1ull << 40);
        std::vector<uint8_t> out;
        uint64_t st[6] = {0, 0, 0, 0, 0, 0};
        int rc = run(comp, cuts, chunk, call_cap, out, st);
        if (rc != 0 || out != data) {
            fprintf(stderr, "ERROR round %d: an intact stream gave rc %d, %zu of %zu bytes\n", r, rc, out.size(), data.size());
            return 1;
        }
        ++intact;
        false_starts += (long)st[1];
        capped += (long)st[5];
        // damaged versions
        for (int d = 0; d < 6; ++d) {
            std::vector<uint8_t> bad = comp;
            if (d < 3) {
                bad[rng() % bad.size()] ^= (uint8_t)(1u << (rng() % 8));
            } else if (d == 3) {
                bad.resize(rng() % bad.size());
            } else if (d == 4) {
                for (int k = 0; k < 8; ++k)
                    bad[rng() % bad.size()] = (uint8_t)rng();
            } else {
                bad.push_back('x');
            }
            rc = run(bad, cuts, chunk, call_cap, out, st);
            // (a cut exactly behind a member leaves a valid, shorter stream)
            if (rc == 0 && out != data && !(d == 3 && out.size() < data.size() && std::equal(out.begin(), out.end(), data.begin())))
                ++wrong;
            refused += rc != 0;
        }
    }
    if (wrong || !false_starts || !capped) {
        fprintf(stderr, "ERROR: %ld damaged streams gave wrong bytes without an error; %ld false starts, %ld capped calls\n", wrong,
                false_starts, capped);
        return 1;
    }
    printf("%d rounds: %ld intact streams exact, %ld damaged ones refused, %ld false starts rejected, %ld calls at their cap\n", rounds,
           intact, refused, false_starts, capped);
    return 0;
}
