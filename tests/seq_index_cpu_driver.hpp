// seq_index_cpu_driver.hpp — the plain-C++ arithmetic of kmm_seq_index_build (csrc/kmm_seqindex_plan.hpp) behind C entry
// points, for tests/test_seq_index_on_the_cpu.py (a shared library through ctypes) and tests/seq_index_san_main.cpp (an
// executable under ASan + UBSan).  No HIP header.
#pragma once
#include <cstdint>

#include "kmm_seqindex_plan.hpp"

extern "C" {

int64_t si_cpu_max_pairs() { return SI_MAX_PAIRS; }
int64_t si_cpu_pairs(int64_t n_windows, int both) { return si_pairs(n_windows, both != 0); }
int64_t si_cpu_table_slots(int64_t n_pairs) { return si_table_slots(n_pairs); }
uint64_t si_cpu_modulo(int64_t n_entries) { return si_modulo(n_entries); }
int si_cpu_is_prime(uint64_t n) { return si_is_prime(n) ? 1 : 0; }
int64_t si_cpu_round_tiles(int debug) { return si_round_tiles(debug != 0); }
uint64_t si_cpu_mix(uint64_t kmer, int32_t node) { return si_mix(kmer, node); }

// The set of pair indices as the kernels keep it (k_si_insert, k_si_keep), one pair after the other: keep[i] = 1 iff pair i is
// the first of its kind.  table: si_table_slots(n) zeroed words.  Returns the number of occupied slots, -1 if a probe ran
// around the whole table.
int64_t si_cpu_dedup(const uint64_t *kmers, const int32_t *nodes, int64_t n, uint32_t *table, int64_t slots, uint8_t *keep)
{
    const uint32_t mask = (uint32_t)(slots - 1);
    int64_t used = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint32_t h = (uint32_t)si_mix(kmers[i], nodes[i]) & mask;
        int64_t steps = 0;
        for (;; h = (h + 1u) & mask) {
            if (++steps > slots)
                return -1;
            if (table[h] == 0u) {
                table[h] = (uint32_t)i + 1u;
                ++used;
                break;
            }
            const uint32_t j = table[h] - 1u;
            if (kmers[j] == kmers[i] && nodes[j] == nodes[i]) {
                if (j > (uint32_t)i)
                    table[h] = (uint32_t)i + 1u;
                break;
            }
        }
    }
    for (int64_t i = 0; i < n; ++i) {
        uint32_t h = (uint32_t)si_mix(kmers[i], nodes[i]) & mask;
        keep[i] = 0;
        for (;; h = (h + 1u) & mask) {
            if (table[h] == 0u)
                return -1;
            const uint32_t j = table[h] - 1u;
            if (j == (uint32_t)i) {
                keep[i] = 1;
                break;
            }
            if (kmers[j] == kmers[i] && nodes[j] == nodes[i])
                break;
        }
    }
    return used;
}

} // extern "C"
