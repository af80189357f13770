// kmm_seqindex_plan.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip in front of the namespace the kernels live in.
// The decisions of kmm_seq_index_build that are plain integer arithmetic, each stated once: the pair limit, the
// number of pairs a call makes, the slots of the de-duplication table, the home slot of a pair, the rounds of the emit pass and
// the modulo that `modulo == 0` chooses.  Standard C++17: no HIP header — tests/test_seq_index_on_the_cpu.py compiles it by
// itself with g++ (tests/seq_index_cpu_driver.hpp).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KMM_SI_HD __host__ __device__ __forceinline__
#else
#define KMM_SI_HD inline
#endif

constexpr int64_t SI_MAX_PAIRS = (int64_t)1 << 30;      // = KMM_SEQIDX_MAX_PAIRS (kmm.h): the table stores pair index + 1 in 32 bits
                                                        // and has 2 |P| slots, 2^31 at the limit
constexpr int64_t SI_MIN_SLOTS = 1024;
constexpr int64_t SI_ROUND_TILES = (int64_t)1 << 20;    // tiles per emit round: 1024 super-tiles of 1024 tiles (k_super_scan's reach)
constexpr int64_t SI_DEBUG_ROUND_TILES = 2 * 1024;      // KMM_SEQIDX_DEBUG_SHORT_ROUNDS: two super-tiles
constexpr uint64_t SI_MAX_MODULO = 0x7FFFFFFFull;       // kmm_build_index: the int32 arrays of the index format

// Pairs of n_windows windows: one each, two with both strands.  -1: more than SI_MAX_PAIRS (judged without overflow: n_windows
// is any int64).
constexpr int64_t si_pairs(int64_t n_windows, bool both_strands)
{
    if (n_windows < 0)
        return -1;
    const int64_t lim = both_strands ? SI_MAX_PAIRS / 2 : SI_MAX_PAIRS;
    return n_windows > lim ? -1 : (both_strands ? 2 * n_windows : n_windows);
}

// Slots of the de-duplication table: the smallest power of two >= max(2 n_pairs, SI_MIN_SLOTS); n_pairs in [0, SI_MAX_PAIRS].
// At least half of the slots stay empty whatever the input, so every probe sequence ends.
constexpr int64_t si_table_slots(int64_t n_pairs)
{
    int64_t s = SI_MIN_SLOTS;
    while (s < 2 * n_pairs)
        s <<= 1;
    return s;
}

// The home slot's hash: splitmix64's finalizer over the k-mer with the node folded in by an odd multiplier.  Poly-A and (AC)n
// k-mers, which differ from their neighbours in a few low or high bits, land far apart; kmer % slots would put the 4^j k-mers
// that share their low bases into one run of slots.
KMM_SI_HD uint64_t si_mix(uint64_t kmer, int32_t node)
{
    uint64_t x = kmer ^ ((uint64_t)(uint32_t)node * 0x9E3779B97F4A7C15ull);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

constexpr int64_t si_round_tiles(bool debug_short_rounds)
{
    return debug_short_rounds ? SI_DEBUG_ROUND_TILES : SI_ROUND_TILES;
}

constexpr bool si_is_prime(uint64_t n)
{
    if (n < 2)
        return false;
    if (n < 4)
        return true;
    if (n % 2 == 0 || n % 3 == 0)
        return false;
    for (uint64_t d = 5; d * d <= n; d += 6)
        if (n % d == 0 || n % (d + 2) == 0)
            return false;
    return true;
}

// What modulo == 0 chooses: the smallest prime >= max(2 n_entries + 1, 3) — load factor below one half, and a prime, so that
// k-mers with a common stride do not share buckets.  Pure; n_entries < 0 counts as 0.  The value may exceed SI_MAX_MODULO
// (n_entries >= 2^30 - 1 or so): the build then refuses and asks for a modulo.
constexpr uint64_t si_modulo(int64_t n_entries)
{
    uint64_t m = n_entries > 0 ? 2 * (uint64_t)n_entries + 1 : 3;
    if (m < 3)
        m = 3;
    while (!si_is_prime(m))
        ++m;
    return m;
}
