// seq_index_san_main.cpp — tests/seq_index_cpu_driver.hpp as a stand-alone program, built with -fsanitize=address,undefined by
// tests/test_seq_index_on_the_cpu.py: the limit arithmetic at its edges, the prime search against trial division, and the
// pair-index set on pairs that repeat, in an exactly sized table.  Prints "ok <primes checked> <pairs kept>"; exit status 1 and
// a line on stderr for the first claim that does not hold.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "seq_index_cpu_driver.hpp"

static int fail(const char *what, long long a, long long b)
{
    fprintf(stderr, "seq_index_san: %s (%lld, %lld)\n", what, a, b);
    return 1;
}

static bool trial_prime(uint64_t n)
{
    if (n < 2)
        return false;
    for (uint64_t d = 2; d * d <= n; ++d)
        if (n % d == 0)
            return false;
    return true;
}

int main()
{
    const int64_t lim = si_cpu_max_pairs();
    if (lim < ((int64_t)1 << 30))
        return fail("the limit is below 2^30", lim, 0);
    if (si_cpu_pairs(lim, 0) != lim || si_cpu_pairs(lim + 1, 0) != -1 || si_cpu_pairs(lim - 1, 0) != lim - 1)
        return fail("pairs at the limit, one strand", si_cpu_pairs(lim, 0), si_cpu_pairs(lim + 1, 0));
    if (si_cpu_pairs(lim / 2, 1) != lim || si_cpu_pairs(lim / 2 + 1, 1) != -1 || si_cpu_pairs(INT64_MAX, 1) != -1 ||
        si_cpu_pairs(INT64_MAX, 0) != -1 || si_cpu_pairs(-1, 0) != -1)
        return fail("pairs at the limit, both strands", si_cpu_pairs(lim / 2, 1), si_cpu_pairs(INT64_MAX, 1));
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)511, (int64_t)512, (int64_t)513, lim - 1, lim}) {
        const int64_t s = si_cpu_table_slots(n);
        if (s < 2 * n || (s & (s - 1)) != 0 || s > ((int64_t)1 << 31))
            return fail("table slots", n, s);
    }
    int64_t primes = 0;
    for (int64_t n = 0; n <= 2000; ++n) {
        uint64_t want = 2 * (uint64_t)n + 1 < 3 ? 3 : 2 * (uint64_t)n + 1;
        while (!trial_prime(want))
            ++want;
        if (si_cpu_modulo(n) != want)
            return fail("modulo", n, (long long)si_cpu_modulo(n));
        ++primes;
    }
    {
        uint64_t want = 2 * ((uint64_t)1 << 30) + 1;
        while (!trial_prime(want))
            ++want;
        if (si_cpu_modulo((int64_t)1 << 30) != want)
            return fail("modulo at 2^30", (long long)want, (long long)si_cpu_modulo((int64_t)1 << 30));
        ++primes;
    }
    // pairs that repeat: 5000 pairs over 37 k-mers and 3 nodes, then 600 distinct ones
    std::vector<uint64_t> km;
    std::vector<int32_t> nd;
    uint64_t x = 88172645463325252ull;
    for (int i = 0; i < 5600; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        km.push_back(i < 5000 ? (x % 37) * 0x0101010101010101ull : x);
        nd.push_back(i < 5000 ? (int32_t)((x >> 40) % 3) : (int32_t)(x >> 40 & 0x7FFFFFFF));
    }
    const int64_t n = (int64_t)km.size(), slots = si_cpu_table_slots(n);
    std::vector<uint32_t> table((size_t)slots, 0u);
    std::vector<uint8_t> keep((size_t)n, 2);
    const int64_t used = si_cpu_dedup(km.data(), nd.data(), n, table.data(), slots, keep.data());
    int64_t kept = 0;
    for (int64_t i = 0; i < n; ++i) {
        bool first = true;
        for (int64_t j = 0; j < i && first; ++j)
            first = !(km[(size_t)j] == km[(size_t)i] && nd[(size_t)j] == nd[(size_t)i]);
        if ((keep[(size_t)i] == 1) != first)
            return fail("keep flag", i, keep[(size_t)i]);
        kept += first ? 1 : 0;
    }
    if (used != kept)
        return fail("occupied slots", used, kept);
    printf("ok %lld %lld\n", (long long)primes, (long long)kept);
    return 0;
}
