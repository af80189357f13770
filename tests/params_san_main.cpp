// tests/params_cpu_driver.hpp as an executable for AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_params_on_the_cpu.py):
//   params_san <value> ...
// Sets every row of the plain table, by its name and by its alias, to every value given and reads it back; prints one line per
// (name, value): "name value set_rc get_rc read-back-or-message".
#include "params_cpu_driver.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    ParamsHandle *h = params_new();
    params_bump_counters(h);
    for (int i = 0; i < params_n_rows(); ++i)
        for (const char *name : {params_row_name(i), params_row_alias(i)}) {
            if (!name)
                continue;
            for (int a = 1; a < argc; ++a) {
                const int64_t value = strtoll(argv[a], nullptr, 10);
                char err[256] = "";
                int64_t got = 0;
                const int set_rc = params_set(h, name, value, err, sizeof err);
                const int get_rc = params_get(h, name, &got, err, sizeof err);
                if (get_rc == 0)
                    printf("%s %lld %d %d %lld\n", name, (long long)value, set_rc, get_rc, (long long)got);
                else
                    printf("%s %lld %d %d %s\n", name, (long long)value, set_rc, get_rc, err);
            }
        }
    params_free(h);
    return 0;
}
