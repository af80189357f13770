// C entry points over csrc/kmm_radix_plan.hpp for tests/test_radix_plan_on_the_cpu.py (g++, no HIP).
#include "kmm_radix_plan.hpp"

static int put_geometry(const std::optional<RxGeometry> &g, int64_t *out)
{
    if (!g)
        return 0;
    out[0] = g->w; out[1] = g->f2; out[2] = g->occ_shift; out[3] = g->PF; out[4] = g->F1; out[5] = g->F2;
    return 1;
}

extern "C" {

// out: w, f2, occ_shift, PF, F1, F2; returns 0 when the configuration is refused
int plan_geometry(uint64_t modulo, uint64_t S, int filter, int w, int maxf, int f2_force, int64_t *out)
{
    return put_geometry(rx_geometry(modulo, S, filter != 0, w, maxf, f2_force), out);
}

// w_forced: whether w_force counts (KMM_RX_W set)
int plan_choose_geometry(uint64_t modulo, uint64_t S, int filter, int w_forced, int w_force, int f2_force, int64_t *out)
{
    return put_geometry(rx_choose_geometry(modulo, S, filter != 0, w_forced ? std::optional<int>(w_force) : std::nullopt, f2_force),
                        out);
}

// out: the 12 table offsets in the order of RxScratch, meta_bytes, buf1_bytes, buf2_bytes, chunks, max_items
void plan_scratch(uint32_t NB, uint32_t F1, uint32_t F2, uint64_t *out)
{
    const RxScratch s = rx_scratch(NB, F1, F2);
    const size_t v[17] = {s.start1, s.P1T, s.S1T, s.csum, s.T1, s.item_base, s.work_base, s.item_desc, s.start2, s.start2T,
                          s.ctrl, s.queue, s.meta_bytes, s.buf1_bytes, s.buf2_bytes, s.chunks, s.max_items};
    for (int i = 0; i < 17; ++i)
        out[i] = v[i];
}

void plan_split(int64_t n_src_total, uint32_t X, int64_t cap, int64_t *out)
{
    const RxSplit s = rx_split(n_src_total, X, cap);
    out[0] = s.n_sub;
    out[1] = s.max_src;
}

int64_t plan_next_smaller_cap(int64_t n_src_total, uint32_t X, int64_t n_sub) { return rx_next_smaller_cap(n_src_total, X, n_sub); }

// returns the variant's number; out: keys in LDS, workgroups per CU, 16-bit directory
int plan_p3(int w, int fits_small, int fits_mid, int p16, uint32_t max_slice, int no_mid, int *out)
{
    const RxP3Variant v = rx_choose_p3(w, fits_small != 0, fits_mid != 0, p16 != 0, max_slice, no_mid != 0);
    const RxP3Shape &s = rx_p3_shape(v);
    out[0] = s.keys_in_lds; out[1] = s.wg_per_cu; out[2] = s.dir16 ? 1 : 0;
    return (int)v;
}

uint64_t plan_view_bytes(uint64_t modulo, uint64_t S, int node_order) { return rx_view_bytes(modulo, S, node_order != 0); }
int64_t plan_min_units(uint64_t modulo, uint64_t S) { return rx_min_units(modulo, S); }

// RX_B, RX_CH, RX_MAXF, RX_IC, RX_ECAP, RX_ECAP_MID, RX_ECAP_BIG, P2F_LOGBITS, P2F_KMAX, RX_SUB_CAP_FLOOR, RX_SUB_CAP_MAX, RX_SUB_CAP_AGE
void plan_constants(int64_t *out)
{
    const int64_t v[12] = {RX_B, RX_CH, RX_MAXF, RX_IC, RX_ECAP, RX_ECAP_MID, RX_ECAP_BIG, P2F_LOGBITS, P2F_KMAX,
                           RX_SUB_CAP_FLOOR, RX_SUB_CAP_MAX, RX_SUB_CAP_AGE};
    for (int i = 0; i < 12; ++i)
        out[i] = v[i];
}

} // extern "C"
