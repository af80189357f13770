// CPU driver of csrc/kmm_bgzf_out.hpp (tests/test_bgzf_out_on_the_cpu.py, tests/bgzf_out_san_main.cpp): the header compiled
// by itself with g++ and walked the way k_bz_deflate, k_bz_offsets and k_bz_gather walk a text — one member per BLOCK bytes,
// every phase of deflate_member run for the 256 threads of a workgroup in turn (CpuExec), each member into a slot of SLOT
// bytes, the members then put one behind the other at the offsets the scan gives.  The workgroup's state, its candidate
// scratch and the slot live on the heap, exactly their size.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "kmm_bgzf_out.hpp"

struct BgzfOutCpuExec {
    template <typename F>
    void each(F &&f) const
    {
        for (uint32_t t = 0; t < kmm_bz::THREADS; ++t)
            f(t);
    }
};

// in[0, n) -> out (capacity bytes).  sizes: room for kmm_bz::member_count(n) member sizes.  stats[0]: the deepest literal /
// length code before the limit, over the members; stats[1]: members whose limiter ran; stats[2]: members that came out stored.
// Returns the bytes written, or -1 when capacity is below kmm_bz::bound(n).
static int64_t bgzf_out_compress(const uint8_t *in, int64_t n, uint8_t *out, int64_t capacity, uint32_t *sizes, uint32_t *stats)
{
    if (n < 0 || capacity < kmm_bz::bound(n))
        return -1;
    stats[0] = stats[1] = stats[2] = 0;
    const uint32_t n_members = (uint32_t)kmm_bz::member_count(n);
    std::vector<uint32_t> crcT((size_t)kmm_gz::CRC_TABLE_WORDS);
    for (int k = 0; k < 8; ++k)
        for (uint32_t b = 0; b < 256u; ++b)
            crcT[(size_t)k * 256 + b] = kmm_gz::crc_table_entry(k, b);
    for (int k = 0; k < kmm_gz::CRC_SHIFT_WORDS; ++k)
        crcT[8 * 256 + (size_t)k] = kmm_gz::crc_shift_table_entry(k);
    std::unique_ptr<kmm_bz::Wg> w(new kmm_bz::Wg);
    std::unique_ptr<uint16_t[]> cand(new uint16_t[kmm_bz::CAND_STRIDE]()); // (a chunked read takes entries behind the member's last)
    std::vector<std::unique_ptr<uint32_t[]>> slots;
    for (uint32_t m = 0; m < n_members; ++m) {
        const int64_t off = (int64_t)m * kmm_bz::BLOCK;
        const uint32_t len = n - off < (int64_t)kmm_bz::BLOCK ? (uint32_t)(n - off) : kmm_bz::BLOCK;
        // (the member's bytes in a buffer of their own: a read behind them is a read behind the heap block)
        std::unique_ptr<uint8_t[]> piece(new uint8_t[len]);
        memcpy(piece.get(), in + off, len);
        slots.emplace_back(new uint32_t[kmm_bz::SLOT / 4]);
        memset(slots.back().get(), 0xA5, kmm_bz::SLOT); // (the kernel's slots are not zeroed either)
        kmm_bz::deflate_member(BgzfOutCpuExec{}, *w, crcT.data(), piece.get(), len, cand.get(), slots.back().get(), sizes + m);
        stats[0] = w->stat_depth > stats[0] ? w->stat_depth : stats[0];
        stats[1] += w->stat_limited;
        stats[2] += w->stored;
    }
    std::vector<unsigned long long> offs((size_t)n_members + 1);
    kmm_bz::member_offsets(sizes, n_members, offs.data());
    for (uint32_t m = 0; m < n_members; ++m)
        memcpy(out + offs[m], slots[m].get(), sizes[m]);
    return (int64_t)offs[n_members];
}

extern "C" int64_t bgzf_out_bound_cpu(int64_t n)
{
    return kmm_bz::bound(n);
}

extern "C" int64_t bgzf_out_compress_cpu(const uint8_t *in, int64_t n, uint8_t *out, int64_t capacity, uint32_t *sizes, uint32_t *stats)
{
    return bgzf_out_compress(in, n, out, capacity, sizes, stats);
}
