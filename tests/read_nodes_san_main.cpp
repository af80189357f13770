// The arithmetic of csrc/kmm_read_nodes_plan.hpp under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone executable
// (tests/test_read_nodes_on_the_cpu.py builds and runs it; nothing sanitized is loaded into Python).
// usage: read_nodes_san VOTES.bin CAP_VOTES   — VOTES.bin: one uint32 pair (read, node) per vote, reads in non-decreasing
// order (a read's total is the number of its pairs; the last pair names the last read).  Every buffer on the heap, exactly its size.
// Cuts the rounds with rn_round_end and with the brute force, then runs every round's votes through a table of
// rn_table_slots cells and reduces it.  Prints "ok <reads> <rounds> <mismatches> <longest walk>".
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "read_nodes_cpu_driver.hpp"

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    const int64_t n = bytes / 8;
    if (n < 1)
        return 2;
    std::unique_ptr<uint32_t[]> raw(new uint32_t[(size_t)(2 * n)]);
    if (fread(raw.get(), 8, (size_t)n, f) != (size_t)n)
        return 2;
    fclose(f);
    const int64_t cap = atoll(argv[2]);
    std::unique_ptr<uint32_t[]> rel(new uint32_t[(size_t)n]), node(new uint32_t[(size_t)n]);
    for (int64_t i = 0; i < n; ++i) {
        rel[(size_t)i] = raw[(size_t)(2 * i)];
        node[(size_t)i] = raw[(size_t)(2 * i + 1)];
    }
    const int64_t n_reads = (int64_t)rel[(size_t)(n - 1)] + 1;
    std::unique_ptr<uint32_t[]> totals(new uint32_t[(size_t)n_reads]());
    std::unique_ptr<int64_t[]> first(new int64_t[(size_t)n_reads + 1]()); // first vote of every read
    for (int64_t i = 0; i < n; ++i)
        totals[rel[(size_t)i]] += 1;
    for (int64_t r = 0; r < n_reads; ++r)
        first[(size_t)r + 1] = first[(size_t)r] + totals[(size_t)r];
    std::unique_ptr<int64_t[]> ends(new int64_t[(size_t)n_reads]), want(new int64_t[(size_t)n_reads]);
    const int64_t rounds = read_nodes_rounds_cpu(totals.get(), n_reads, cap, ends.get());
    int64_t bad = rounds != read_nodes_rounds_brute(totals.get(), n_reads, cap, want.get());
    for (int64_t i = 0; i < rounds && !bad; ++i)
        bad += ends[(size_t)i] != want[(size_t)i];
    int64_t longest = 0;
    for (int64_t i = 0, r0 = 0; i < rounds && !bad; r0 = ends[(size_t)i++]) {
        const int64_t r1 = ends[(size_t)i], v0 = first[(size_t)r0], votes = first[(size_t)r1] - v0, nr = r1 - r0;
        const int64_t slots = read_nodes_table_slots(votes);
        std::unique_ptr<uint64_t[]> keys(new uint64_t[(size_t)slots]), best(new uint64_t[(size_t)nr]);
        std::unique_ptr<uint32_t[]> counts(new uint32_t[(size_t)slots]), nn(new uint32_t[(size_t)nr]), second(new uint32_t[(size_t)nr]);
        std::unique_ptr<uint32_t[]> rr(new uint32_t[(size_t)(votes ? votes : 1)]);
        for (int64_t v = 0; v < votes; ++v)
            rr[(size_t)v] = rel[(size_t)(v0 + v)] - (uint32_t)r0;
        const int64_t walk = read_nodes_table_cpu(rr.get(), node.get() + v0, votes, slots, keys.get(), counts.get());
        if (walk < 0)
            ++bad;
        if (walk > longest)
            longest = walk;
        read_nodes_reduce_cpu(keys.get(), counts.get(), slots, nr, best.get(), nn.get(), second.get());
        for (int64_t r = 0; r < nr; ++r) // every vote is in some cell: a read with votes has a best node with votes
            bad += (totals[(size_t)(r0 + r)] > 0) != (read_nodes_best_node(best[(size_t)r]) >= 0) ||
                   read_nodes_best_votes(best[(size_t)r]) > totals[(size_t)(r0 + r)] || second[(size_t)r] > read_nodes_best_votes(best[(size_t)r]);
    }
    printf("ok %lld %lld %lld %lld\n", (long long)n_reads, (long long)rounds, (long long)bad, (long long)longest);
    return bad ? 1 : 0;
}
