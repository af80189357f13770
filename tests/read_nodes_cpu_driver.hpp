// CPU driver of csrc/kmm_read_nodes_plan.hpp (tests/test_read_nodes_on_the_cpu.py, tests/read_nodes_san_main.cpp): the header
// compiled by itself with g++ and used the way the host driver and the kernels of kmm_read_nodes use it — the rounds cut over
// the prefix of the reads' vote totals, votes added to an open-addressing table through rn_home and a linear walk, the best
// word raised by max — next to brute-force versions of the same.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "kmm_read_nodes_plan.hpp"

extern "C" int64_t read_nodes_round_votes(int64_t table_bytes) { return rn_round_votes(table_bytes); }
extern "C" int64_t read_nodes_table_slots(int64_t votes) { return rn_table_slots(votes); }

// ends[i] = the read in front of which round i ends; returns the number of rounds.  ends holds n_reads entries.
extern "C" int64_t read_nodes_rounds_cpu(const uint32_t *totals, int64_t n_reads, int64_t cap_votes, int64_t *ends)
{
    std::vector<int64_t> prefix((size_t)n_reads + 1);
    prefix[0] = 0;
    for (int64_t r = 0; r < n_reads; ++r)
        prefix[(size_t)r + 1] = prefix[(size_t)r] + totals[(size_t)r];
    int64_t rounds = 0;
    for (int64_t r0 = 0; r0 < n_reads; ++rounds) {
        const int64_t r1 = rn_round_end(prefix.data(), n_reads, r0, cap_votes);
        ends[(size_t)rounds] = r1;
        r0 = r1;
    }
    return rounds;
}

// The brute force: reads are added to the round one by one while they fit.
extern "C" int64_t read_nodes_rounds_brute(const uint32_t *totals, int64_t n_reads, int64_t cap_votes, int64_t *ends)
{
    int64_t rounds = 0;
    for (int64_t r = 0; r < n_reads; ++rounds) {
        int64_t votes = totals[(size_t)r++];
        while (r < n_reads && votes + totals[(size_t)r] <= cap_votes)
            votes += totals[(size_t)r++];
        ends[(size_t)rounds] = r;
    }
    return rounds;
}

// n votes, vote i for (rel[i], node[i]), into a table of `slots` cells (keys: RN_EMPTY_KEY where free; counts) as
// rn_table_add walks it.  Returns the longest walk (slots looked at for one vote), or -1 when a vote found no slot.
extern "C" int64_t read_nodes_table_cpu(const uint32_t *rel, const uint32_t *node, int64_t n, int64_t slots, uint64_t *keys,
                                        uint32_t *counts)
{
    for (int64_t s = 0; s < slots; ++s) {
        keys[(size_t)s] = RN_EMPTY_KEY;
        counts[(size_t)s] = 0;
    }
    int64_t longest = 0;
    for (int64_t i = 0; i < n; ++i) {
        const uint64_t key = rn_key(rel[(size_t)i], node[(size_t)i]);
        uint64_t s = rn_home(key, (uint64_t)slots);
        if (s >= (uint64_t)slots)
            return -1;
        int64_t tries = 0;
        for (; tries < slots; ++tries) {
            if (keys[s] == RN_EMPTY_KEY || keys[s] == key) {
                keys[s] = key;
                counts[s] += 1;
                break;
            }
            if (++s == (uint64_t)slots)
                s = 0;
        }
        if (tries == slots)
            return -1;
        if (tries + 1 > longest)
            longest = tries + 1;
    }
    return longest;
}

// The cells of a table -> per read (n_reads of them): best word, distinct nodes, and second votes, as k_rn_best and k_rn_second.
extern "C" void read_nodes_reduce_cpu(const uint64_t *keys, const uint32_t *counts, int64_t slots, int64_t n_reads, uint64_t *best,
                                      uint32_t *n_nodes, uint32_t *second)
{
    for (int64_t r = 0; r < n_reads; ++r) {
        best[(size_t)r] = 0;
        n_nodes[(size_t)r] = second[(size_t)r] = 0;
    }
    for (int64_t s = 0; s < slots; ++s) {
        if (keys[(size_t)s] == RN_EMPTY_KEY)
            continue;
        const uint32_t r = rn_key_read(keys[(size_t)s]);
        const uint64_t w = rn_best_word(counts[(size_t)s], rn_key_node(keys[(size_t)s]));
        if (w > best[r])
            best[r] = w;
        n_nodes[r] += 1;
    }
    for (int64_t s = 0; s < slots; ++s) {
        if (keys[(size_t)s] == RN_EMPTY_KEY)
            continue;
        const uint32_t r = rn_key_read(keys[(size_t)s]);
        if ((int32_t)rn_key_node(keys[(size_t)s]) != rn_best_node(best[r]) && counts[(size_t)s] > second[r])
            second[r] = counts[(size_t)s];
    }
}

extern "C" int32_t read_nodes_best_node(uint64_t word) { return rn_best_node(word); }
extern "C" uint32_t read_nodes_best_votes(uint64_t word) { return rn_best_votes(word); }
extern "C" uint64_t read_nodes_best_word(uint32_t votes, uint32_t node) { return rn_best_word(votes, node); }
extern "C" uint64_t read_nodes_key(uint32_t rel, uint32_t node) { return rn_key(rel, node); }
