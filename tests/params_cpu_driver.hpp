// C entry points over csrc/kmm_params.hpp for tests/test_params_on_the_cpu.py (g++, no HIP): the plain half of the parameter
// table on a handle that is nothing but the two structs, put together the way kmm_set_param / kmm_get_param do it.
#include "kmm_params.hpp"

struct ParamsHandle : KmmKnobs, KmmCounters {};

extern "C" {

ParamsHandle *params_new() { return new ParamsHandle; }
void params_free(ParamsHandle *h) { delete h; }

int params_n_rows() { return (int)(sizeof kmm_params::ROWS / sizeof kmm_params::ROWS[0]); }
const char *params_row_name(int i) { return kmm_params::ROWS[i].name; }
const char *params_row_alias(int i) { return kmm_params::ROWS[i].alias; }
int params_row_has_hook(int i) { return kmm_params::ROWS[i].set || kmm_params::ROWS[i].get; }

// 0, or -1 (KMM_ERR_INVALID_ARG) with the message in err
int params_set(ParamsHandle *h, const char *name, int64_t value, char *err, int n)
{
    const kmm_params::Row *row = kmm_params::find(kmm_params::ROWS, name);
    if (kmm_params::set_refused(row, name, value, err, (size_t)n))
        return -1;
    kmm_params::store(*row, *h, value);
    return 0;
}

int params_get(ParamsHandle *h, const char *name, int64_t *value, char *err, int n)
{
    const kmm_params::Row *row = kmm_params::find(kmm_params::ROWS, name);
    if (kmm_params::get_refused(row, name, err, (size_t)n))
        return -1;
    *value = kmm_params::load(*row, *h, *h);
    return 0;
}

// a counter moves (what the map calls do): so that a get of a counter row is seen to read its own field
void params_bump_counters(ParamsHandle *h)
{
    int64_t v = 100;
    for (const kmm_params::Row &r : kmm_params::ROWS) {
        if (r.at.type == kmm_params::Member::COUNTER_I64)
            h->*r.at.cl = v++;
        else if (r.at.type == kmm_params::Member::COUNTER_U64)
            h->*r.at.cu = (uint64_t)v++;
    }
}

} // extern "C"
