// kmm_read_nodes_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace, behind the
// flat-reads helpers of kmm_read_hits (FlatReads, flat_reads_*), view_of, with_probe_flavour, grid_for and ensure.  The host
// driver of kmm_read_nodes (kernels: kmm_read_nodes.hpp, arithmetic: kmm_read_nodes_plan.hpp).
#pragma once

// A round's table stays with the handle between calls while it is no larger than this (a chunk loop does not allocate per
// chunk); a larger one goes back to the device when the call ends.
constexpr size_t RN_KEEP_TABLE_BYTES = (size_t)256 << 20;

template <int MODE>
int launch_rn_count(kmm_index *ix, const FlatReads &fr, int k, int max_freq, int also_rc, uint32_t *total_votes, unsigned long long *grand)
{
    const IndexView iv = view_of(ix);
    const dim3 grid((unsigned)grid_for_tiles(ix, fr.n_tiles));
    with_probe_flavour(iv, [&](auto probe) {
        hipLaunchKernelGGL((k_rn_count<TILE_S, MODE, decltype(probe)::value>), grid, dim3(256), 0, ix->stream, fr.rv, iv, k, max_freq,
                           also_rc, fr.n_tiles, fr.tile_first, total_votes, grand);
    });
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

template <int MODE>
int launch_rn_vote(kmm_index *ix, const FlatReads &fr, int k, int max_freq, int also_rc, int64_t tile_lo, int64_t tile_hi, int64_t r0,
                   int64_t n_round, RnCell *cells, uint64_t slots, unsigned long long *err)
{
    const IndexView iv = view_of(ix);
    const dim3 grid((unsigned)grid_for_tiles(ix, tile_hi - tile_lo));
    with_probe_flavour(iv, [&](auto probe) {
        hipLaunchKernelGGL((k_rn_vote<TILE_S, MODE, decltype(probe)::value>), grid, dim3(256), 0, ix->stream, fr.rv, iv, k, max_freq,
                           also_rc, tile_lo, tile_hi, fr.tile_first, r0, n_round, cells, slots, err);
    });
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

// The five per-read outputs: the caller's array where it lies in device memory, else a slice of the stage's aux buffer that
// is copied out at the end (`user` == null: the output is not wanted; total_votes gets a slice all the same).
struct RnOut {
    void *user = nullptr;
    bool dev = false;
    void *d = nullptr;
};

struct RnArgs {
    int k, max_freq, also_rc;
    int64_t n_reads, read_len, table_bytes;
    const int64_t *read_offsets;
    int64_t *n_rounds;
};

// One round: the votes of reads [r0, r1) — `votes` of them, at positions [p_lo, p_hi) — into a cleared table, then the table
// into best / n_nodes / second_votes.
int rn_round(kmm_index *ix, const FlatReads &fr, const RnArgs &a, int64_t r0, int64_t r1, int64_t votes, int64_t p_lo, int64_t p_hi,
             unsigned long long *d_best, uint32_t *d_nn, uint32_t *d_second, unsigned long long *d_err)
{
    if (votes == 0)
        return KMM_OK; // (no cell would be in use)
    if (votes > RN_MAX_ROUND_VOTES)
        return fail(KMM_ERR_INVALID_ARG, "kmm_read_nodes: read %lld alone has %lld votes, more than one round's table holds (%lld)",
                    (long long)r0, (long long)votes, (long long)RN_MAX_ROUND_VOTES);
    const uint64_t slots = (uint64_t)rn_table_slots(votes);
    KMMCHK(ensure(ix->rn_table, (size_t)slots * RN_CELL_BYTES));
    RnCell *cells = (RnCell *)ix->rn_table.p;
    const dim3 sgrid((unsigned)grid_for(ix, (int64_t)((slots + 255) / 256), 32));
    hipLaunchKernelGGL(k_rn_clear, sgrid, dim3(256), 0, ix->stream, cells, slots);
    HIPCHK(hipGetLastError());
    const int64_t tile_lo = p_lo / TILE_T, tile_hi = (p_hi + TILE_T - 1) / TILE_T;
    if (fr.uniform_kernel)
        KMMCHK(launch_rn_vote<MODE_UNIFORM>(ix, fr, a.k, a.max_freq, a.also_rc, tile_lo, tile_hi, r0, r1 - r0, cells, slots, d_err));
    else
        KMMCHK(launch_rn_vote<MODE_GENERAL>(ix, fr, a.k, a.max_freq, a.also_rc, tile_lo, tile_hi, r0, r1 - r0, cells, slots, d_err));
    hipLaunchKernelGGL(k_rn_best, sgrid, dim3(256), 0, ix->stream, cells, slots, r0, d_best, d_nn);
    if (d_second)
        hipLaunchKernelGGL(k_rn_second, sgrid, dim3(256), 0, ix->stream, cells, slots, r0, d_best, d_second);
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

// Behind the count pass (grand: all votes of the call): cut the reads into rounds and run them.  One round when everything fits
// the target table — nothing but the grand total has then left the device; else the per-read totals (and offsets that lie in
// device memory) are fetched and the cuts made over their 64-bit prefix (rn_round_end).
int rn_rounds(kmm_index *ix, const FlatReads &fr, const RnArgs &a, unsigned long long grand, const uint32_t *d_total,
              unsigned long long *d_best, uint32_t *d_nn, uint32_t *d_second, unsigned long long *d_err)
{
    const int64_t cap = rn_round_votes(a.table_bytes), n = a.n_reads;
    int64_t rounds = 0;
    if (grand <= (unsigned long long)cap && n <= RN_MAX_ROUND_READS) {
        KMMCHK(rn_round(ix, fr, a, 0, n, (int64_t)grand, 0, fr.total, d_best, d_nn, d_second, d_err));
        rounds = 1;
    } else {
        std::vector<uint32_t> tv((size_t)n);
        HIPCHK(hipMemcpyAsync(tv.data(), d_total, (size_t)n * 4, hipMemcpyDeviceToHost, ix->stream));
        std::vector<int64_t> offs_copy;
        const int64_t *offs = a.read_offsets;
        if (offs && is_device_ptr(offs)) {
            offs_copy.resize((size_t)n + 1);
            HIPCHK(hipMemcpyAsync(offs_copy.data(), offs, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, ix->stream));
            offs = offs_copy.data();
        }
        HIPCHK(hipStreamSynchronize(ix->stream));
        std::vector<int64_t> prefix((size_t)n + 1);
        prefix[0] = 0;
        for (int64_t r = 0; r < n; ++r)
            prefix[(size_t)r + 1] = prefix[(size_t)r] + tv[(size_t)r];
        for (int64_t r0 = 0; r0 < n; ++rounds) {
            const int64_t r1 = rn_round_end(prefix.data(), n, r0, cap);
            const int64_t p_lo = offs ? offs[r0] : r0 * a.read_len, p_hi = offs ? offs[r1] : r1 * a.read_len;
            KMMCHK(rn_round(ix, fr, a, r0, r1, prefix[(size_t)r1] - prefix[(size_t)r0], p_lo, p_hi, d_best, d_nn, d_second, d_err));
            r0 = r1;
        }
    }
    if (a.n_rounds)
        *a.n_rounds = rounds;
    return KMM_OK;
}

int read_nodes_impl(kmm_index *ix, const uint8_t *bases, const uint8_t *lut, const RnArgs &a, int32_t *best_node, uint32_t *best_votes,
                    uint32_t *second_votes, uint32_t *total_votes, uint32_t *n_nodes)
{
    HIPCHK(hipSetDevice(ix->device));
    int64_t total = 0;
    KMMCHK(flat_reads_total("kmm_read_nodes", bases, a.read_offsets, a.n_reads, a.read_len, &total));
    const size_t out_bytes = (size_t)a.n_reads * 4, out_slot = (out_bytes + 255) & ~(size_t)255;
    RnOut out[5]; // best_node, best_votes, second_votes, total_votes, n_nodes
    void *const users[5] = {best_node, best_votes, second_votes, total_votes, n_nodes};
    for (int i = 0; i < 5; ++i) {
        out[i].user = users[i];
        out[i].dev = users[i] && is_device_ptr(users[i]);
    }
    if (a.n_rounds)
        *a.n_rounds = 0;
    if (total == 0) { // nothing to look up: the outputs are written in full all the same (-1 / 0)
        hipError_t e = hipSuccess;
        for (int i = 0; i < 5 && e == hipSuccess; ++i) {
            if (!out[i].user)
                continue;
            const int fill = i == 0 ? 0xFF : 0;
            e = out[i].dev ? hipMemsetAsync(out[i].user, fill, out_bytes, ix->stream) : (memset(out[i].user, fill, out_bytes), hipSuccess);
        }
        if (e == hipSuccess)
            e = hipStreamSynchronize(ix->stream);
        if (e != hipSuccess)
            return fail(KMM_ERR_HIP, "kmm_read_nodes: %s", hipGetErrorString(e));
        return KMM_OK;
    }
    // aux behind the error words: [0, 256) the grand total and the table-full flag; the best words; the five output slices
    const size_t best_bytes = ((size_t)a.n_reads * 8 + 255) & ~(size_t)255;
    FlatReads fr;
    KMMCHK(flat_reads_stage(ix, bases, a.read_offsets, a.n_reads, a.read_len, total, lut, 256 + best_bytes + 5 * out_slot, fr));
    uint8_t *aux = (uint8_t *)fr.d_bad + 256;
    unsigned long long *d_ctl = (unsigned long long *)aux; // [0] all votes of the call, [1] a vote found no slot
    unsigned long long *d_best = (unsigned long long *)(aux + 256);
    for (int i = 0; i < 5; ++i)
        out[i].d = out[i].dev ? out[i].user : (out[i].user || i == 3) ? (void *)(aux + 256 + best_bytes + (size_t)i * out_slot) : nullptr;
    uint32_t *d_total = (uint32_t *)out[3].d, *d_second = (uint32_t *)out[2].d, *d_nn = (uint32_t *)out[4].d;
    HIPCHK(hipMemsetAsync(d_ctl, 0, 16, ix->stream));
    HIPCHK(hipMemsetAsync(d_best, 0, (size_t)a.n_reads * 8, ix->stream));
    for (int i = 2; i < 5; ++i)
        if (out[i].d)
            HIPCHK(hipMemsetAsync(out[i].d, 0, out_bytes, ix->stream));
    KMMCHK(flat_reads_mark(ix, fr));
    if (fr.uniform_kernel)
        KMMCHK(launch_rn_count<MODE_UNIFORM>(ix, fr, a.k, a.max_freq, a.also_rc, d_total, &d_ctl[0]));
    else
        KMMCHK(launch_rn_count<MODE_GENERAL>(ix, fr, a.k, a.max_freq, a.also_rc, d_total, &d_ctl[0]));
    unsigned long long bad[3] = {NO_BAD, NO_BAD, NO_BAD}, ctl[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(bad, fr.d_bad, sizeof bad, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipMemcpyAsync(ctl, d_ctl, 8, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    // (bad offsets or bytes: the totals mean nothing, no round is run)
    int rc = flat_reads_errors("kmm_read_nodes", bad);
    if (rc == KMM_OK)
        rc = rn_rounds(ix, fr, a, ctl[0], d_total, d_best, d_nn, d_second, &d_ctl[1]);
    hipError_t e = hipSuccess;
    if (rc == KMM_OK) {
        hipLaunchKernelGGL(k_rn_unpack, dim3(grid_for(ix, (a.n_reads + 255) / 256, 16)), dim3(256), 0, ix->stream, d_best, a.n_reads,
                           (int32_t *)out[0].d, (uint32_t *)out[1].d);
        e = hipGetLastError();
        for (int i = 0; i < 5 && e == hipSuccess; ++i)
            if (out[i].user && !out[i].dev)
                e = hipMemcpyAsync(out[i].user, out[i].d, out_bytes, hipMemcpyDeviceToHost, ix->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(&ctl[1], &d_ctl[1], 8, hipMemcpyDeviceToHost, ix->stream);
    }
    const hipError_t es = hipStreamSynchronize(ix->stream);
    if (e == hipSuccess)
        e = es;
    if (ix->rn_table.cap > RN_KEEP_TABLE_BYTES)
        (void)ix->rn_table.reset();
    if (e != hipSuccess)
        return rc != KMM_OK ? rc : fail(KMM_ERR_HIP, "kmm_read_nodes: %s", hipGetErrorString(e));
    const std::string why = g_err; // (of rc; stage_release may write its own)
    const int released = stage_release(ix, *fr.s, fr.staged);
    if (rc != KMM_OK) {
        g_err = why;
        return rc;
    }
    KMMCHK(released);
    if (ctl[1])
        return fail(KMM_ERR_INTERNAL, "kmm_read_nodes: a vote found no free slot: the count pass and the vote pass disagree");
    return KMM_OK;
}
