// kmm_read_nodes_plan.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip in front of the namespace the kernels live in.
// The decisions of kmm_read_nodes that are plain integer arithmetic, each stated once: the cell key and the best
// word with their tie rule, the slots of a round's vote table, the home slot of a key, and where the rounds are cut over the
// prefix of the reads' vote totals.  Standard C++17: no HIP header — tests/test_read_nodes_on_the_cpu.py compiles it by itself
// with g++ (tests/read_nodes_cpu_driver.hpp).
#pragma once
#include <cstdint>

#include "kmm_seqindex_plan.hpp" // si_mix: splitmix64's finalizer

#if defined(__HIPCC__)
#define KMM_RN_HD __host__ __device__ __forceinline__
#else
#define KMM_RN_HD inline
#endif

constexpr uint64_t RN_EMPTY_KEY = ~0ull;                      // node ids are below 2^31: no key has all bits set
constexpr int64_t RN_CELL_BYTES = 16;                         // {key 8, count 4, pad 4}: key and count share one 16-byte line piece
constexpr int64_t RN_MIN_SLOTS = 64;
constexpr int64_t RN_MIN_TABLE_BYTES = (int64_t)64 << 10;     // smaller targets are raised to this: 2048 votes per round
constexpr int64_t RN_DEFAULT_TABLE_BYTES = (int64_t)4 << 30;  // table_bytes == 0: 2^27 votes per round
constexpr int64_t RN_MAX_ROUND_VOTES = ((int64_t)1 << 31) - 1; // slots stay below 2^32 (rn_home), per-cell counts below 2^31
constexpr int64_t RN_MAX_ROUND_READS = (int64_t)1 << 31;      // the read of a key is relative to the round's first: 31 bits

// ---- the cell key: (read - the round's first read) << 32 | node
KMM_RN_HD uint64_t rn_key(uint32_t rel_read, uint32_t node)
{
    return ((uint64_t)rel_read << 32) | node;
}
KMM_RN_HD uint32_t rn_key_read(uint64_t key) { return (uint32_t)(key >> 32); }
KMM_RN_HD uint32_t rn_key_node(uint64_t key) { return (uint32_t)key; }

// ---- the best word of a read: votes << 32 | (0x7FFFFFFF - node).  The largest word is the largest vote count, and among
// equal counts the smallest node id.  0: the read has no vote (a cell holds at least one).
KMM_RN_HD uint64_t rn_best_word(uint32_t votes, uint32_t node)
{
    return ((uint64_t)votes << 32) | (0x7FFFFFFFu - node);
}
KMM_RN_HD int32_t rn_best_node(uint64_t word) { return word ? (int32_t)(0x7FFFFFFFu - (uint32_t)word) : -1; }
KMM_RN_HD uint32_t rn_best_votes(uint64_t word) { return (uint32_t)(word >> 32); }

// ---- the table of a round
// Votes a table of table_bytes may hold: half of its slots.  table_bytes >= 0 (0: the default).
constexpr int64_t rn_round_votes(int64_t table_bytes)
{
    if (table_bytes == 0)
        table_bytes = RN_DEFAULT_TABLE_BYTES;
    if (table_bytes < RN_MIN_TABLE_BYTES)
        table_bytes = RN_MIN_TABLE_BYTES;
    const int64_t v = table_bytes / RN_CELL_BYTES / 2;
    return v > RN_MAX_ROUND_VOTES ? RN_MAX_ROUND_VOTES : v;
}

// Slots for a round of `votes` votes (0 .. RN_MAX_ROUND_VOTES): twice the votes — the distinct (read, node) pairs are no more than
// the votes, so at least half of the slots stay empty and every probe sequence ends.
constexpr int64_t rn_table_slots(int64_t votes)
{
    return 2 * votes < RN_MIN_SLOTS ? RN_MIN_SLOTS : 2 * votes;
}

// The home slot: the high half of the mixed key scaled into [0, slots), slots < 2^32 — not the key's low bits, which are the
// node: reads that sit on one node would start in one slot.
KMM_RN_HD uint64_t rn_home(uint64_t key, uint64_t slots)
{
    return ((si_mix(key, 0) >> 32) * slots) >> 32;
}

// ---- rounds.  prefix[r] = the votes of reads [0, r), r = 0 .. n_reads (non-decreasing).  The round that starts at read r0 <
// n_reads ends in front of the returned read: the largest r1 with prefix[r1] - prefix[r0] <= cap_votes and r1 - r0 <=
// RN_MAX_ROUND_READS, and r0 + 1 when read r0 alone has more votes than cap_votes (a round holds whole reads and at least one).
KMM_RN_HD int64_t rn_round_end(const int64_t *prefix, int64_t n_reads, int64_t r0, int64_t cap_votes)
{
    int64_t lo = r0 + 1, hi = n_reads - r0 > RN_MAX_ROUND_READS ? r0 + RN_MAX_ROUND_READS : n_reads;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2; // in (lo, hi]
        if (prefix[mid] - prefix[r0] <= cap_votes)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
