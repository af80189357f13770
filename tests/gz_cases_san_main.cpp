// Sanitizer run of the GPU inflater's decoder on forged streams (tests/test_inflate_vs_zlib_on_the_cpu.py writes the cases with
// tests/deflate_forge.py and builds this with -fsanitize=address,undefined): every case in exact-size heap buffers — the input
// with no byte behind it, the output with the decoder's 16 bytes of slack, which must stay untouched.
//   argv[1]  cases: repeated [u32 n_in][u32 n_out][n_in bytes]
//   argv[2]  results: per case [i32 rc][u32 n_out][n_out bytes of output]
// Exit 0; 1 when a case wrote into the slack; 2 on a malformed case file.
#include "kmm_gpu_inflate.hpp"

#include <cstdio>
#include <vector>

int main(int argc, char **argv)
{
    if (argc < 3)
        return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g)
        return 2;
    long n_cases = 0;
    for (;;) {
        uint32_t hdr[2];
        const size_t got = fread(hdr, 4, 2, f);
        if (got == 0)
            break;
        if (got != 2)
            return 2;
        std::vector<uint8_t> in(hdr[0]);            // exactly n_in bytes on the heap
        if (hdr[0] && fread(in.data(), 1, hdr[0], f) != hdr[0])
            return 2;
        std::vector<uint8_t> out((size_t)hdr[1] + 16, 0xA5);
        std::vector<uint16_t> prim(kmm_gz::PRIM_WORDS), sec(kmm_gz::SEC_WORDS);
        std::vector<uint64_t> list(kmm_gz::LIST_ALLOC);
        const int32_t rc = kmm_gz::inflate_stream(in.data(), hdr[0], out.data(), hdr[1], prim.data(), sec.data(), list.data());
        for (int k = 0; k < 16; ++k)
            if (out[(size_t)hdr[1] + (size_t)k] != 0xA5) {
                fprintf(stderr, "case %ld: a byte written behind the output\n", n_cases);
                return 1;
            }
        fwrite(&rc, 4, 1, g);
        fwrite(&hdr[1], 4, 1, g);
        fwrite(out.data(), 1, hdr[1], g);
        ++n_cases;
    }
    fclose(f);
    fclose(g);
    printf("%ld cases\n", n_cases);
    return 0;
}
