// kmm_seqindex_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace, behind
// scan_exclusive and bi_build_device.  The host driver of kmm_seq_index_build (kernels: kmm_seqindex.hpp,
// arithmetic: kmm_seqindex_plan.hpp): validate, emit the pair list P in rounds, de-duplicate it to D, choose the modulo and
// run the index build on D — all on one private stream, nothing but counts and error words crossing to the host.
#pragma once

inline unsigned si_grid(int64_t n, int per_block = 256)
{
    int64_t g = (n + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : (g > 65536 ? 65536 : g));
}

// |D| == 0: the two tables of `modulo` zeros, no entries.
int si_empty(kmm_seq_index &s, uint64_t modulo, hipStream_t st)
{
    const uint64_t M = modulo ? modulo : si_modulo(0);
    KMMCHK(ensure(s.h2i, (size_t)M * 4));
    KMMCHK(ensure(s.nk, (size_t)M * 4));
    HIPCHK(hipMemsetAsync(s.h2i.p, 0, (size_t)M * 4, st));
    HIPCHK(hipMemsetAsync(s.nk.p, 0, (size_t)M * 4, st));
    HIPCHK(hipStreamSynchronize(st));
    s.modulo = M;
    s.n_entries = 0;
    return KMM_OK;
}

int seq_index_build_impl(int device, const uint8_t *bases, const int64_t *seq_offsets, int64_t n_seqs, const int32_t *seq_nodes,
                         int k, const uint8_t *lut, int flags, uint64_t modulo, kmm_seq_index &s)
{
    KMMCHK(check_k(k));
    if (n_seqs < 0)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: n_seqs=%lld is negative", (long long)n_seqs);
    if (flags & ~(KMM_SEQIDX_BOTH_STRANDS | KMM_SEQIDX_DEBUG_SHORT_ROUNDS))
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: flags=0x%x has bits this version does not know", (unsigned)flags);
    if (modulo > SI_MAX_MODULO)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: modulo=%llu exceeds the int32 arrays of the index format (at most %llu)",
                    (unsigned long long)modulo, (unsigned long long)SI_MAX_MODULO);
    if (n_seqs > 0 && !seq_offsets)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: seq_offsets is NULL for n_seqs=%lld", (long long)n_seqs);
    if (n_seqs > 0x7FFFFFFFll)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: n_seqs=%lld exceeds the int32 nodes of the index format", (long long)n_seqs);
    const bool both = (flags & KMM_SEQIDX_BOTH_STRANDS) != 0;
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(KMM_ERR_HIP, "no HIP device available: libkmm has no CPU fallback");
    }
    HIPCHK(hipSetDevice(device));
    s.device = device;
    Stream st; // a stream of its own: other handles' work on this device is not stalled (destroyed after the buffers)
    DevBuf d_bases, d_offs, d_nodes, d_lut, d_bad, d_bits, d_first, d_cnt, d_sup, d_pk, d_pn, d_table, d_keep, d_pos, d_dk, d_dn;
    BiScratch bis;
    HIPCHK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking));

    uint8_t lutbuf[256];
    if (!lut)
        default_lut(lutbuf);
    else if (is_device_ptr(lut))
        HIPCHK(hipMemcpy(lutbuf, lut, 256, hipMemcpyDeviceToHost));
    else
        memcpy(lutbuf, lut, 256);
    const bool has_break = memchr(lutbuf, KMM_LUT_BREAK, 256) != nullptr;
    if (has_break && k == 1)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: k=1 with a break entry in the lookup table (a break is a one-base read: k >= 2)");

    unsigned long long bad[3] = {NO_BAD, NO_BAD, NO_BAD}; // [0] byte without a code, [1] negative node, [2] decreasing offsets
    KMMCHK(ensure(d_bad, sizeof bad));
    HIPCHK(hipMemsetAsync(d_bad.p, 0xFF, sizeof bad, st));
    unsigned long long *p_bad = (unsigned long long *)d_bad.p;

    // offsets and nodes: judged where they lie
    int64_t total = 0;
    const int64_t *p_offs = seq_offsets;
    const int32_t *p_nodes = seq_nodes;
    if (n_seqs > 0) {
        const bool offs_dev = is_device_ptr(seq_offsets);
        int64_t ends[2];
        if (offs_dev) {
            HIPCHK(hipMemcpy(&ends[0], seq_offsets, 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(&ends[1], seq_offsets + n_seqs, 8, hipMemcpyDeviceToHost));
        } else {
            ends[0] = seq_offsets[0];
            ends[1] = seq_offsets[n_seqs];
        }
        if (ends[0] != 0)
            return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: seq_offsets[0] must be 0 (got %lld)", (long long)ends[0]);
        if (offs_dev) {
            hipLaunchKernelGGL(k_check_offsets, dim3(si_grid(n_seqs)), dim3(256), 0, st, seq_offsets, n_seqs, p_bad);
            HIPCHK(hipGetLastError());
        } else {
            for (int64_t r = 0; r < n_seqs; ++r)
                if (seq_offsets[r + 1] < seq_offsets[r])
                    return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: seq_offsets is not non-decreasing at sequence %lld", (long long)r);
        }
        if (seq_nodes) {
            if (is_device_ptr(seq_nodes)) {
                hipLaunchKernelGGL(k_si_check_nodes, dim3(si_grid(n_seqs)), dim3(256), 0, st, seq_nodes, n_seqs, p_bad);
                HIPCHK(hipGetLastError());
            } else {
                for (int64_t r = 0; r < n_seqs; ++r)
                    if (seq_nodes[r] < 0)
                        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: seq_nodes[%lld]=%d is negative", (long long)r, (int)seq_nodes[r]);
            }
        }
        if (offs_dev || (seq_nodes && is_device_ptr(seq_nodes))) {
            HIPCHK(hipStreamSynchronize(st));
            HIPCHK(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
            if (bad[2] != NO_BAD)
                return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: seq_offsets is not non-decreasing at sequence %llu", bad[2]);
            if (bad[1] != NO_BAD)
                return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: seq_nodes[%llu] is negative", bad[1]);
        }
        total = ends[1]; // (>= 0: the offsets start at 0 and do not decrease)
    }
    if (total > 0 && !bases)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: bases is NULL for %lld bases", (long long)total);
    s.n_windows = s.n_pairs = 0;
    if (total == 0)
        return si_empty(s, modulo, st);

    // ---- the tile front end's view: bases, offsets, table, the read-start bitset with the breaks
    ReadsView rv;
    memset(&rv, 0, sizeof rv);
    rv.total = total;
    rv.n_reads = n_seqs;
    if (is_device_ptr(bases)) {
        rv.bases = bases;
    } else {
        KMMCHK(ensure(d_bases, (size_t)total));
        HIPCHK(hipMemcpyAsync(d_bases.p, bases, (size_t)total, hipMemcpyHostToDevice, st));
        rv.bases = (const uint8_t *)d_bases.p;
    }
    if (!is_device_ptr(seq_offsets)) {
        KMMCHK(ensure(d_offs, (size_t)(n_seqs + 1) * 8));
        HIPCHK(hipMemcpyAsync(d_offs.p, seq_offsets, (size_t)(n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
        p_offs = (const int64_t *)d_offs.p;
    }
    rv.offsets = p_offs;
    if (seq_nodes && !is_device_ptr(seq_nodes)) {
        KMMCHK(ensure(d_nodes, (size_t)n_seqs * 4));
        HIPCHK(hipMemcpyAsync(d_nodes.p, seq_nodes, (size_t)n_seqs * 4, hipMemcpyHostToDevice, st));
        p_nodes = (const int32_t *)d_nodes.p;
    }
    KMMCHK(ensure(d_lut, 256));
    HIPCHK(hipMemcpyAsync(d_lut.p, lutbuf, 256, hipMemcpyHostToDevice, st));
    rv.lut = (const uint8_t *)d_lut.p;
    rv.first_bad = p_bad;
    const int64_t n_words = total / 32 + 2;
    const int64_t n_tiles = (total + TILE_T - 1) / TILE_T;
    KMMCHK(ensure(d_bits, (size_t)n_words * 4));
    KMMCHK(ensure(d_first, (size_t)(n_tiles + 1) * 8));
    HIPCHK(hipMemsetAsync(d_bits.p, 0, (size_t)n_words * 4, st));
    rv.start_bits = (const uint32_t *)d_bits.p;
    rv.n_start_words = n_words;
    hipLaunchKernelGGL(k_mark_starts, dim3(si_grid(n_seqs + 1)), dim3(256), 0, st, p_offs, n_seqs, total, (uint32_t *)d_bits.p);
    if (has_break) // every break byte: a one-base read
        hipLaunchKernelGGL(k_mark_breaks, dim3(si_grid(total, 256 * 16 * MARK_U)), dim3(256), 0, st, rv.bases, total, rv.lut,
                           (uint32_t *)d_bits.p);
    hipLaunchKernelGGL(k_rh_tile_reads, dim3(si_grid(n_tiles + 1)), dim3(256), 0, st, p_offs, n_seqs, total, n_tiles, (int64_t)TILE_T,
                       (int64_t *)d_first.p);
    HIPCHK(hipGetLastError());

    // ---- emit, count: per round the tiles' window counts, scanned inside their super-tile, and the super-tiles' scanned totals
    // (the round's own total behind them).  All rounds keep their counts: the write pass runs once |P| is known and judged.
    const int64_t round_tiles = si_round_tiles((flags & KMM_SEQIDX_DEBUG_SHORT_ROUNDS) != 0);
    const int64_t n_rounds = (n_tiles + round_tiles - 1) / round_tiles;
    std::vector<int64_t> cnt_off((size_t)n_rounds + 1, 0), sup_off((size_t)n_rounds + 1, 0);
    for (int64_t r = 0; r < n_rounds; ++r) {
        const int64_t t0 = r * round_tiles, t1 = t0 + round_tiles < n_tiles ? t0 + round_tiles : n_tiles;
        const int64_t n_super = (t1 - t0 + 1023) / 1024;
        cnt_off[(size_t)r + 1] = cnt_off[(size_t)r] + n_super * 1024;
        sup_off[(size_t)r + 1] = sup_off[(size_t)r] + n_super + 1;
    }
    KMMCHK(ensure(d_cnt, (size_t)cnt_off[(size_t)n_rounds] * 4));
    KMMCHK(ensure(d_sup, (size_t)sup_off[(size_t)n_rounds] * 4));
    HIPCHK(hipMemsetAsync(d_cnt.p, 0, (size_t)cnt_off[(size_t)n_rounds] * 4, st));
    for (int64_t r = 0; r < n_rounds; ++r) {
        const int64_t t0 = r * round_tiles, t1 = t0 + round_tiles < n_tiles ? t0 + round_tiles : n_tiles;
        const int n_super = (int)((t1 - t0 + 1023) / 1024);
        uint32_t *tile_cnt = (uint32_t *)d_cnt.p + cnt_off[(size_t)r], *super_tot = (uint32_t *)d_sup.p + sup_off[(size_t)r];
        hipLaunchKernelGGL((k_extract_count<TILE_S, MODE_GENERAL>), dim3(si_grid(t1 - t0, 1)), dim3(256), 0, st, rv, k, t0, t1, tile_cnt);
        hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, st, tile_cnt, super_tot);
        hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, st, super_tot, n_super, super_tot + n_super);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(bad, d_bad.p, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != NO_BAD)
        return fail(KMM_ERR_INVALID_BASE, "kmm_seq_index_build: sequence byte at offset %llu is not a nucleotide under the lookup table "
                    "(the reference's DNA encoder raises here)", bad[0]);
    std::vector<int64_t> round_base((size_t)n_rounds + 1, 0);
    for (int64_t r = 0; r < n_rounds; ++r) {
        uint32_t tot = 0;
        HIPCHK(hipMemcpy(&tot, (uint32_t *)d_sup.p + sup_off[(size_t)r + 1] - 1, 4, hipMemcpyDeviceToHost));
        round_base[(size_t)r + 1] = round_base[(size_t)r] + (int64_t)tot;
    }
    const int64_t n_windows = round_base[(size_t)n_rounds];
    const int64_t n_pairs = si_pairs(n_windows, both);
    if (n_pairs < 0)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: %lld windows%s make more than KMM_SEQIDX_MAX_PAIRS=%lld pairs; "
                    "build the index from fewer sequences per call", (long long)n_windows, both ? " on both strands" : "",
                    (long long)SI_MAX_PAIRS);
    s.n_windows = n_windows;
    s.n_pairs = n_pairs;
    if (n_pairs == 0)
        return si_empty(s, modulo, st);

    // ---- emit, write: P
    const int mult = both ? 2 : 1;
    KMMCHK(ensure(d_pk, (size_t)n_pairs * 8));
    KMMCHK(ensure(d_pn, (size_t)n_pairs * 4));
    for (int64_t r = 0; r < n_rounds; ++r) {
        if (round_base[(size_t)r + 1] == round_base[(size_t)r])
            continue;
        const int64_t t0 = r * round_tiles, t1 = t0 + round_tiles < n_tiles ? t0 + round_tiles : n_tiles;
        const uint32_t *tile_pre = (const uint32_t *)d_cnt.p + cnt_off[(size_t)r], *super_pre = (const uint32_t *)d_sup.p + sup_off[(size_t)r];
        hipLaunchKernelGGL((k_si_write<TILE_S>), dim3(si_grid(t1 - t0, 1)), dim3(256), 0, st, rv, k, both ? 1 : 0, t0, t1, tile_pre, super_pre,
                           (const int64_t *)d_first.p, p_nodes, (uint64_t *)d_pk.p + round_base[(size_t)r] * mult,
                           (int32_t *)d_pn.p + round_base[(size_t)r] * mult);
    }
    HIPCHK(hipGetLastError());

    // ---- de-duplicate: D = the pairs that are the first of their kind, in order
    const int64_t slots = si_table_slots(n_pairs);
    const uint32_t mask = (uint32_t)(slots - 1);
    KMMCHK(ensure(d_table, (size_t)slots * 4));
    KMMCHK(ensure(d_keep, (size_t)n_pairs * 4));
    KMMCHK(ensure(d_pos, (size_t)n_pairs * 4));
    HIPCHK(hipMemsetAsync(d_table.p, 0, (size_t)slots * 4, st));
    hipLaunchKernelGGL(k_si_insert, dim3(si_grid(n_pairs)), dim3(256), 0, st, (const uint64_t *)d_pk.p, (const int32_t *)d_pn.p, n_pairs,
                       (uint32_t *)d_table.p, mask);
    hipLaunchKernelGGL(k_si_keep, dim3(si_grid(n_pairs)), dim3(256), 0, st, (const uint64_t *)d_pk.p, (const int32_t *)d_pn.p, n_pairs,
                       (const uint32_t *)d_table.p, mask, (uint32_t *)d_keep.p);
    HIPCHK(hipGetLastError());
    KMMCHK(scan_exclusive((const uint32_t *)d_keep.p, (uint32_t *)d_pos.p, (uint64_t)n_pairs, bis.scan, 0, st));
    HIPCHK(hipStreamSynchronize(st));
    uint32_t last[2] = {0, 0};
    HIPCHK(hipMemcpy(&last[0], (uint32_t *)d_pos.p + (n_pairs - 1), 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&last[1], (uint32_t *)d_keep.p + (n_pairs - 1), 4, hipMemcpyDeviceToHost));
    const int64_t n_entries = (int64_t)last[0] + (int64_t)last[1];
    if (n_entries < 1 || n_entries > n_pairs)
        return fail(KMM_ERR_INTERNAL, "kmm_seq_index_build: %lld distinct pairs of %lld", (long long)n_entries, (long long)n_pairs);
    HIPCHK(d_table.reset());
    const uint64_t M = modulo ? modulo : si_modulo(n_entries);
    if (M > SI_MAX_MODULO)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: %lld entries ask for modulo %llu, beyond the int32 arrays of the index format "
                    "(at most %llu): give a modulo", (long long)n_entries, (unsigned long long)M, (unsigned long long)SI_MAX_MODULO);
    KMMCHK(ensure(d_dk, (size_t)n_entries * 8));
    KMMCHK(ensure(d_dn, (size_t)n_entries * 4));
    hipLaunchKernelGGL(k_si_compact, dim3(si_grid(n_pairs)), dim3(256), 0, st, (const uint64_t *)d_pk.p, (const int32_t *)d_pn.p, n_pairs,
                       (const uint32_t *)d_keep.p, (const uint32_t *)d_pos.p, (uint64_t *)d_dk.p, (int32_t *)d_dn.p);
    HIPCHK(hipGetLastError());

    // ---- the index of D, without a trip to the host
    KMMCHK(ensure(s.h2i, (size_t)M * 4));
    KMMCHK(ensure(s.nk, (size_t)M * 4));
    KMMCHK(ensure(s.kmers, (size_t)n_entries * 8));
    KMMCHK(ensure(s.nodes, (size_t)n_entries * 4));
    KMMCHK(ensure(s.freqs, (size_t)n_entries * 2));
    KMMCHK(bi_build_device(st, (const uint64_t *)d_dk.p, (const int32_t *)d_dn.p, n_entries, M, (uint32_t *)s.nk.p, (uint32_t *)s.h2i.p,
                           (uint64_t *)s.kmers.p, (int32_t *)s.nodes.p, (uint16_t *)s.freqs.p, bis));
    HIPCHK(hipStreamSynchronize(st));
    s.modulo = M;
    s.n_entries = n_entries;
    return KMM_OK;
}

int seq_index_fetch_impl(kmm_seq_index &s, int32_t *hashes_to_index, int32_t *n_kmers, uint64_t *kmers, int32_t *nodes,
                         uint16_t *frequencies)
{
    if (!hashes_to_index || !n_kmers)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_fetch: hashes_to_index / n_kmers is NULL (int32[%llu] each)",
                    (unsigned long long)s.modulo);
    if (s.n_entries > 0 && (!kmers || !nodes || !frequencies))
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_fetch: kmers / nodes / frequencies is NULL for %lld entries", (long long)s.n_entries);
    HIPCHK(hipSetDevice(s.device));
    auto down = [&](void *dst, const void *src, size_t bytes) -> hipError_t {
        if (bytes == 0)
            return hipSuccess;
        return hipMemcpy(dst, src, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost);
    };
    HIPCHK(down(hashes_to_index, s.h2i.p, (size_t)s.modulo * 4));
    HIPCHK(down(n_kmers, s.nk.p, (size_t)s.modulo * 4));
    HIPCHK(down(kmers, s.kmers.p, (size_t)s.n_entries * 8));
    HIPCHK(down(nodes, s.nodes.p, (size_t)s.n_entries * 4));
    HIPCHK(down(frequencies, s.freqs.p, (size_t)s.n_entries * 2));
    return KMM_OK;
}
