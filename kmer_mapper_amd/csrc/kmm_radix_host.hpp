// kmm_radix_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace, once kmm_index
// and its helpers (view_of, ScopedTimer, ensure, grid_for, scan_exclusive) are defined.
// Host side of the radix path: the handle's geometry, the launches of a sub-batch, the flush, the self-check and the build
// of the radix view.  What is plain arithmetic (fan-out, scratch layout, sub-batch split, choice of the pass-3 kernel) is in
// kmm_radix_plan.hpp.
#pragma once

// Self-check of the radix path at every synchronising call: every k-mer pass 1 emitted must have been gathered by
// pass 2 and probed by pass 3 (or dropped by pass 2's empty-bucket filter).  The three passes count independently
// (per-lane registers -> one sharded atomic per wavefront at kernel end), so a work item that is handed out twice, skipped, or
// seen differently by the wavefronts of one workgroup (the round-2 race) shows up here instead of as
// silently wrong counts.  Called with both streams drained.
int rx_check_conservation(kmm_index *ix)
{
    if (!ix->rx_unchecked)
        return KMM_OK;
    ix->rx_unchecked = false;
    static thread_local std::vector<unsigned long long> st;
    st.resize(KMM_STAT_BYTES / 8);
    HIPCHK(hipMemcpy(st.data(), ix->stats, KMM_STAT_BYTES, hipMemcpyDeviceToHost));
    unsigned long long p1 = 0, p2 = 0, p3 = 0, dropped = 0;
    for (int i = 0; i < KMM_STAT_SHARDS; ++i) {
        const unsigned long long *sh = st.data() + (size_t)i * KMM_STAT_STRIDE;
        p1 += sh[KMM_STAT_RX_P1];
        p2 += sh[2];
        p3 += sh[3];
        dropped += sh[KMM_STAT_RX_DROPPED];
    }
    if (p1 == p2 && p2 == p3 + dropped)
        return KMM_OK;
    const int rc = fail(KMM_ERR_INTERNAL, "radix path self-check failed: pass 1 emitted %llu k-mers, pass 2 gathered %llu, "
                        "pass 3 probed %llu (+ %llu dropped as absent) since the counters were last reset: the node counts "
                        "are invalid until kmm_reset_counts [latest map call #%llu on this handle]",
                        p1, p2, p3, dropped, (unsigned long long)ix->map_calls);
    ix->sticky_rc = rc;
    ix->sticky_msg = g_err;
    return rc;
}

// Pass 2 filters k-mers of empty buckets (k_rx_p2f) when a coarse partition's bitmap fits its 64 KB of LDS and its
// first bucket starts a bitmap word.
bool rx_filter_active(const kmm_index *ix)
{
    const RxGeometry &g = ix->rx_geo;
    return ix->rx_filter && ix->rx_occ && g.w + g.f2 - g.occ_shift >= 5 && g.occ_shift <= 2;
}

// ... with the slot filter (rx_filter_slot) where the coarse partitions have exactly 2^19 buckets and the array is there
bool rx_slots_active(const kmm_index *ix)
{
    return rx_filter_active(ix) && ix->rx_geo.slot_filter && ix->rx_filter_slots && ix->rx_slots;
}

bool use_radix(const kmm_index *ix, int64_t units)
{
    if (!ix->rx_ok || ix->path == 1)
        return false;
    return ix->path == 2 || ix->rx_ecnt_acc || units >= ix->rx_min_units;
}

RxP3Variant rx_p3_variant(const kmm_index *ix)
{
    return rx_choose_p3(ix->rx_geo.w, ix->rx_fits_small, ix->rx_fits_mid, ix->rx_pstart16 != nullptr, ix->rx_max_slice,
                        ix->rx_no_mid);
}

// Pass 3 probes through fingerprint bytes: the variant has that form and "radix_p3_fingerprints" asks for it
bool rx_p3_fp_active(const kmm_index *ix)
{
    return ix->rx_p3_fp && rx_p3_shape(rx_p3_variant(ix)).fingerprints;
}

// The kernels' view of a sub-batch of NB blocks whose tables lie in rx_meta as `sc` says.
RxView rx_view_of(const kmm_index *ix, const RxScratch &sc, uint32_t NB)
{
    const RxGeometry &g = ix->rx_geo;
    RxView rx;
    memset(&rx, 0, sizeof rx);
    rx.pstart = ix->rx_pstart; rx.pkeys = ix->rx_pkeys; rx.pfreq = ix->rx_pfreq; rx.ecnt = ix->rx_ecnt;
    rx.pstart16 = ix->rx_pstart16; rx.slice_e0 = ix->rx_slice_e0; rx.slice_fmax = ix->rx_slice_fmax;
    rx.occ = ix->rx_occ;
    rx.slots = rx_slots_active(ix) ? (const uint32_t *)ix->rx_slots : nullptr;
    rx.p2f_cap = ix->dbg_p2f_cap;
    rx.occ_shift = rx_filter_active(ix) ? g.occ_shift : 3; // (3: k_rx_p2f without its filter)
    rx.p2f_k = NB / 2048u < 4u ? 4u : (NB / 2048u > (uint32_t)P2F_KMAX ? (uint32_t)P2F_KMAX : NB / 2048u);
    rx.w = g.w; rx.f2 = g.f2; rx.PF = g.PF; rx.F1 = g.F1; rx.F2 = g.F2;
    rx.NB = NB; rx.max_items = (uint32_t)sc.max_items;
    uint8_t *m = (uint8_t *)ix->rx_meta.p;
    rx.start1 = (uint16_t *)(m + sc.start1); rx.P1T = (uint32_t *)(m + sc.P1T); rx.S1T = (uint16_t *)(m + sc.S1T);
    rx.csum = (uint32_t *)(m + sc.csum); rx.T1 = (uint32_t *)(m + sc.T1); rx.item_base = (uint32_t *)(m + sc.item_base);
    rx.work_base = (uint32_t *)(m + sc.work_base); rx.item_desc = (uint2 *)(m + sc.item_desc);
    rx.start2 = (uint16_t *)(m + sc.start2); rx.start2T = (uint16_t *)(m + sc.start2T);
    rx.ctrl = (uint32_t *)(m + sc.ctrl);
    rx.queue = (unsigned long long *)(m + sc.queue);
    rx.buf1 = (uint64_t *)ix->rx_buf1.p;
    rx.buf2 = (uint64_t *)ix->rx_buf2.p;
#if RX_PROBE_ANY
    rx.probe = (uint64_t *)ix->rx_probe.p;
#endif
    return rx;
}

// Pass 1 of n_src source blocks: with or without reverse complements, from bytes or from 2-bit codes.
template <int MODE>
int rx_launch_p1(kmm_index *ix, const ReadsView &rv, const uint64_t *src_kmers, int64_t n_kmers, const IndexView &iv,
                 const RxView &rx, int k, int64_t tile0, uint32_t n_src, int also_rc)
{
    static const int p1_per_cu = getenv("KMM_RX_P1_GRID_PER_CU") ? atoi(getenv("KMM_RX_P1_GRID_PER_CU")) : 8; // (experiments)
    const int64_t g1cap = (int64_t)ix->n_cu * (p1_per_cu > 0 ? p1_per_cu : 8);
    const dim3 g1((unsigned)(n_src < g1cap ? n_src : g1cap));
    constexpr bool CAN_C2 = MODE == MODE_PACKED || MODE == MODE_UNIFORM || MODE == MODE_GENERAL;
    if (rv.codes2 && !CAN_C2)
        return fail(KMM_ERR_INTERNAL, "2-bit code input reaches pass 1 through the flat-read modes only");
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, g1, dim3(RX_NT), 0, ix->stream, rv, src_kmers, n_kmers, iv, rx, k, tile0, n_src);
    };
    if constexpr (CAN_C2) {
        if (rv.codes2) {
            if (also_rc)
                go(k_rx_p1<MODE, true, true>);
            else
                go(k_rx_p1<MODE, false, true>);
            return KMM_OK;
        }
    }
    if (also_rc)
        go(k_rx_p1<MODE, true>);
    else
        go(k_rx_p1<MODE, false>);
    return KMM_OK;
}

void rx_launch_p2(kmm_index *ix, const IndexView &iv, const RxView &rx)
{
    if (!ix->rx_filter) { // the round-2 form ("radix_filter" = 0)
        hipLaunchKernelGGL(k_rx_p2, dim3(ix->n_cu * ix->rx_grid_per_cu), dim3(RX_NT), 0, ix->stream, iv, rx);
        return;
    }
    // gather by k-mer; where a coarse partition's occupancy bitmap fits LDS (one bit per 1, 2 or 4 buckets) the k-mers of
    // empty buckets are dropped here; with the slot filter also those whose bucket pair holds no entry that chose their bit
    const bool flt = rx_filter_active(ix), small = rx.F2 <= 128;
    auto kern = rx.slots ? (small ? k_rx_p2f<P2F_SLOT, true> : k_rx_p2f<P2F_SLOT, false>)
                : flt    ? (small ? k_rx_p2f<P2F_BITMAP, true> : k_rx_p2f<P2F_BITMAP, false>)
                         : (small ? k_rx_p2f<P2F_NONE, true> : k_rx_p2f<P2F_NONE, false>);
    hipLaunchKernelGGL(kern, dim3(ix->n_cu), dim3(P2F_NT), 0, ix->stream, iv, rx);
}

// (the only place that names instantiations of k_rx_p3: one per RxP3Variant, and the fingerprint form of those whose shape
// has one)
void rx_launch_p3(kmm_index *ix, const IndexView &iv, const RxView &rx, int max_freq)
{
    const RxP3Variant v = rx_p3_variant(ix);
    const dim3 grid(ix->n_cu * (rx_p3_shape(v).wg_per_cu > 1 ? ix->rx_grid_per_cu : 1));
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(RX_NT), 0, ix->stream, iv, rx, max_freq); };
    static_assert(rx_p3_shape(RxP3Variant::W12_DIR16).fingerprints && rx_p3_fp_shapes() == 1,
                  "RX_P3_SHAPES promises the fingerprint form exactly where an instantiation is named below");
    switch (v) {
    case RxP3Variant::W12_DIR16:
        if (rx_p3_fp_active(ix))
            go(k_rx_p3<RX_WMAX, RX_ECAP, 4, uint16_t, RX_SUBCAP3, true, true>);
        else
            go(k_rx_p3<RX_WMAX, RX_ECAP, 4, uint16_t, RX_SUBCAP3, true>);
        break;
    case RxP3Variant::W12:             go(k_rx_p3<RX_WMAX, RX_ECAP, 4, uint32_t>); break;
    case RxP3Variant::W13_SMALL_DIR16: go(k_rx_p3<RX_WMAX_BIG, RX_ECAP, 4, uint16_t, RX_SUBCAP3, true>); break;
    case RxP3Variant::W13_SMALL:       go(k_rx_p3<RX_WMAX_BIG, RX_ECAP, 4, uint16_t>); break;
    case RxP3Variant::W13_MID_DIR16:   go(k_rx_p3<RX_WMAX_BIG, RX_ECAP_MID, 4, uint16_t, 1024, true>); break;
    case RxP3Variant::W13_MID:         go(k_rx_p3<RX_WMAX_BIG, RX_ECAP_MID, 4, uint16_t, 1024>); break;
    case RxP3Variant::W13_BIG:         go(k_rx_p3<RX_WMAX_BIG, RX_ECAP_BIG, 2, uint32_t>); break;
    }
}

// One batch on the radix path, in sub-batches (kmm_radix_plan.hpp): pass 1 (reads or k-mers -> blocks sorted by coarse
// partition), the directory scan, pass 2 (items sorted by fine partition), pass 3 (LDS probe).  Hits land in rx_ecnt.
template <int MODE>
int launch_rx(kmm_index *ix, const ReadsView &rv, const uint64_t *kmers_in, int64_t n_in, int k, int max_freq,
              int also_rc)
{
    const IndexView iv = view_of(ix);
    const int64_t units = MODE == MODE_KMERS ? n_in : rv.total;
    // blocks of pass 1: 8192 positions, or (packed tiles) the reads of two tiles
    const int64_t n_src_total = MODE == MODE_PACKED ? (rv.n_reads + 2 * (int64_t)rv.pk_rpt - 1) / (2 * (int64_t)rv.pk_rpt)
                                                    : (units + RX_B - 1) / RX_B;
    const uint32_t X = also_rc ? 2u : 1u;
    const uint32_t F1 = ix->rx_geo.F1, F2 = ix->rx_geo.F2;
    // The buffers are sized for the largest sub-batch.  Without the HBM for the buffers of that size the call takes one
    // sub-batch more, and again, down to 2^28 slots per sub-batch; the handle remembers the size that fitted
    // ("radix_sub_batch_kmers_effective") for its next 15 calls and then tries the caller's cap again — an allocation that
    // failed because something else held the memory for a moment does not shrink the handle's sub-batches for good (round 4
    // halved "radix_sub_batch_kmers" itself: four failing rounds for a 2^29-slot batch, for ever).
    RxSplit split;
    static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
    const auto t_0 = std::chrono::steady_clock::now();
    if (ix->rx_sub_cap_eff > 0 && ++ix->rx_sub_cap_eff_age >= RX_SUB_CAP_AGE)
        ix->rx_sub_cap_eff = 0;
    int64_t cap = ix->rx_sub_cap_eff > 0 && ix->rx_sub_cap_eff < ix->rx_sub_cap ? ix->rx_sub_cap_eff : ix->rx_sub_cap;
    for (;;) {
        split = rx_split(n_src_total, X, cap);
        const RxScratch sm = rx_scratch((uint32_t)(split.max_src * X), F1, F2);
        int rc = ix->dbg_rx_buf_limit && sm.buf1_bytes > (size_t)ix->dbg_rx_buf_limit ? (int)KMM_ERR_NOMEM // (test hook)
                                                                                      : ensure(ix->rx_meta, sm.meta_bytes);
        if (rc == KMM_OK)
            rc = ensure(ix->rx_buf1, sm.buf1_bytes);
        if (rc == KMM_OK)
            rc = ensure(ix->rx_buf2, sm.buf2_bytes);
#if RX_PROBE_ANY
        if (rc == KMM_OK)
            rc = ensure(ix->rx_probe, sm.buf2_bytes);
#endif
        if (rc == KMM_OK)
            break;
        if (rc != KMM_ERR_NOMEM || cap <= RX_SUB_CAP_FLOOR || n_src_total <= 1)
            return rc;
        (void)hipGetLastError();
        (void)ix->rx_buf1.reset();
        (void)ix->rx_buf2.reset();
        cap = rx_next_smaller_cap(n_src_total, X, split.n_sub);
        ix->rx_sub_cap_eff = cap;
        ix->rx_sub_cap_eff_age = 0;
    }
    ix->rx_sub_cap_last = cap;
    const double ms_buffers = ms_since(t_0);
    const int64_t max_src = split.max_src;
    for (int64_t s0 = 0; s0 < n_src_total; s0 += max_src) {
        const uint32_t n_src = (uint32_t)(n_src_total - s0 < max_src ? n_src_total - s0 : max_src);
        const uint32_t NB = n_src * X;
        const RxScratch sc = rx_scratch(NB, F1, F2);
        // (growing a buffer here would free it under the previous sub-batch's kernels)
        bool grew = sc.meta_bytes > ix->rx_meta.cap || sc.buf1_bytes > ix->rx_buf1.cap || sc.buf2_bytes > ix->rx_buf2.cap;
#if RX_PROBE_ANY
        grew = grew || sc.buf2_bytes > ix->rx_probe.cap;
#endif
        if (grew)
            return fail(KMM_ERR_INTERNAL, "radix path: a sub-batch of %u blocks needs more scratch than the largest one was given", NB);
        const RxView rx = rx_view_of(ix, sc, NB);
        ix->dbg_T1 = rx.T1; ix->dbg_item_base = rx.item_base; ix->dbg_start1 = rx.start1; ix->dbg_F1 = F1; ix->dbg_NB = NB;
        HIPCHK(hipMemsetAsync(rx.ctrl, 0, sc.meta_bytes - sc.ctrl, ix->stream)); // ctrl and the work counters behind it
        ScopedTimer tm;
        KMMCHK(tm.begin(ix, KMM_KERNEL_RX_P1));
        const int64_t tile0 = s0 * (RX_B / (MODE == MODE_RECORDS ? 1024 : 4096));
        KMMCHK(rx_launch_p1<MODE>(ix, rv, kmers_in ? kmers_in + s0 * RX_B : nullptr, n_in - s0 * RX_B, iv, rx, k, tile0, n_src,
                                  also_rc));
        HIPCHK(hipGetLastError());
        KMMCHK(tm.end());
        KMMCHK(tm.begin(ix, KMM_KERNEL_RX_SCAN));
        // (the scan's form follows the pass 2 rx_launch_p2 is about to choose: k_rx_p2 reads the absolute run starts P1T,
        // k_rx_p2f rebuilds them from the run lengths and item_desc.y, and the scan then leaves the P1T area alone)
        const bool with_p = !ix->rx_filter;
        auto chunkscan = with_p ? k_rx_chunkscan<true> : k_rx_chunkscan<false>;
        auto colscan = with_p ? k_rx_colscan<true> : k_rx_colscan<false>;
        hipLaunchKernelGGL(k_rx_colsum, dim3(sc.chunks), dim3(256), 0, ix->stream, rx);
        hipLaunchKernelGGL(chunkscan, dim3(F1), dim3(256), 0, ix->stream, rx, sc.chunks);
        hipLaunchKernelGGL(k_rx_tables, dim3(1), dim3(512), 0, ix->stream, rx);
        hipLaunchKernelGGL(colscan, dim3(sc.chunks, (F1 + 255) / 256), dim3(256), 0, ix->stream, rx);
        HIPCHK(hipGetLastError());
        KMMCHK(tm.end());
        KMMCHK(tm.begin(ix, KMM_KERNEL_RX_P2));
        rx_launch_p2(ix, iv, rx);
        HIPCHK(hipGetLastError());
        KMMCHK(tm.end());
        KMMCHK(tm.begin(ix, KMM_KERNEL_RX_SCAN));
        hipLaunchKernelGGL(k_rx_tr2, dim3((unsigned)((sc.max_items + RX_TR2 - 1) / RX_TR2)), dim3(256), 0, ix->stream, rx);
        HIPCHK(hipGetLastError());
        KMMCHK(tm.end());
        KMMCHK(tm.begin(ix, KMM_KERNEL_RX_P3));
        rx_launch_p3(ix, iv, rx, max_freq);
        HIPCHK(hipGetLastError());
        KMMCHK(tm.end());
        ix->ecnt_dirty = true;
        ix->rx_unchecked = true;
    }
    ix->n_radix_batches++;
    if (verbose && ms_since(t_0) > 20.0)
        fprintf(stderr, "libkmm: radix passes of %lld positions: %.2f ms for the batch buffers (%zu + %zu + %zu bytes), %.2f ms to issue %lld "
                "sub-batch(es)\n", (long long)units, ms_buffers, ix->rx_meta.cap, ix->rx_buf1.cap, ix->rx_buf2.cap, ms_since(t_0) - ms_buffers,
                (long long)split.n_sub);
    return KMM_OK;
}

// Per-entry hits of the radix path -> node counts (mapper.pyx:68 summed per entry first).  Asynchronous.
int rx_flush(kmm_index *ix)
{
    if (!ix->ecnt_dirty)
        return KMM_OK;
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_RX_FLUSH));
    if (ix->rx_norder && !ix->rx_ecnt_acc && ix->rx_flush_sorted) {
        // entries in node order: a gather of the counts + atomics that walk the count vector front to back
        hipLaunchKernelGGL(k_rx_flush_sorted, dim3(ix->n_cu * 8), dim3(256), 0, ix->stream, view_of(ix), ix->rx_ecnt,
                           ix->rx_norder, ix->rx_nnode, ix->rx_S);
        HIPCHK(hipMemsetAsync(ix->rx_ecnt, 0, (size_t)ix->rx_S * 4, ix->stream));
    } else {
        hipLaunchKernelGGL(k_rx_flush, dim3(ix->n_cu * 8), dim3(256), 0, ix->stream, view_of(ix), ix->rx_ecnt,
                           ix->rx_pnodes, ix->rx_S, ix->rx_ecnt_acc);
    }
    HIPCHK(hipGetLastError());
    KMMCHK(tm.end());
    ix->ecnt_dirty = false;
    return KMM_OK;
}

// Pass 2's slot filter for the current (w, f2), from the packed keys: built where the geometry has one and "radix_filter_slots"
// asks for it, dropped otherwise.  Optional: without the HBM for it (96 KB per coarse partition) the bucket bitmap serves.
// Synchronous.
int rx_build_slots(kmm_index *ix)
{
    static_cast<RxSlotFilter &>(*ix) = RxSlotFilter();
    if (!ix->rx_filter || !ix->rx_geo.slot_filter || !ix->rx_filter_slots || !ix->rx_occ)
        return KMM_OK;
    const size_t bytes = (size_t)ix->rx_geo.F1 * P2F_SLOT_WORDS * 4;
    if (hipMalloc(ix->rx_slots.put(), bytes) != hipSuccess) {
        (void)hipGetLastError();
        static_cast<RxSlotFilter &>(*ix) = RxSlotFilter();
        return KMM_OK;
    }
    HIPCHK(hipMemsetAsync(ix->rx_slots, 0, bytes, ix->stream));
    hipLaunchKernelGGL(k_rx_build_slots, dim3(grid_for(ix, (int64_t)((ix->modulo + 255) / 256), 16)), dim3(256), 0, ix->stream,
                       ix->rx_pstart, ix->rx_pkeys, ix->modulo, ix->rx_geo.w + ix->rx_geo.f2, ix->rx_slots);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ix->stream));
    return KMM_OK;
}

// The entry k-mers in the packed form of the current (w, f2) (kmm_radix.hpp), and what else depends on the geometry: the
// 16-bit directory, the slot filter; synchronous.
int rx_repack_keys(kmm_index *ix)
{
    if (ix->rx_S)
        hipLaunchKernelGGL(k_rx_pack_keys, dim3(grid_for(ix, (int64_t)((ix->rx_S + 255) / 256), 16)), dim3(256), 0,
                           ix->stream, ix->rx_pkeys_raw, ix->rx_S, view_of(ix), ix->rx_geo.w + ix->rx_geo.f2, ix->rx_pkeys);
    HIPCHK(hipGetLastError());
    // most entries of one slice: decides whether pass 3 may keep a 16-bit directory (ix->queue serves as the cell)
    HIPCHK(hipMemsetAsync(ix->queue, 0, 3 * sizeof(unsigned long long), ix->stream));
    hipLaunchKernelGGL(k_rx_max_slice, dim3(grid_for(ix, (int64_t)((ix->rx_geo.PF + 255) / 256), 16)), dim3(256), 0, ix->stream,
                       ix->rx_pstart, ix->modulo, ix->rx_geo.w, ix->rx_geo.PF, ix->queue);
    HIPCHK(hipGetLastError());
    unsigned long long mx[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(mx, ix->queue, sizeof mx, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    ix->rx_max_slice = (uint32_t)mx[0];
    // a slice with more entries than pass 3 keeps in LDS has the buckets behind them walked in HBM: fine for the odd
    // slice (a k-mer stored under 1500 nodes), not as the rule — at most one slice in a thousand (or one slice)
    const unsigned long long odd = ix->rx_geo.PF / 1000 > 1 ? ix->rx_geo.PF / 1000 : 1;
    ix->rx_fits_small = mx[1] <= odd;
    ix->rx_fits_mid = mx[2] <= odd;
    // 16-bit slice-relative directory: pass 3 loads 2 B per bucket instead of 4 (optional: 2 B x modulo of HBM)
    static_cast<RxDir16 &>(*ix) = RxDir16();
    if (ix->rx_max_slice <= 65535u && !getenv("KMM_RX_NO_P16")) {
        const size_t n16 = ((size_t)ix->rx_geo.PF << ix->rx_geo.w) + 8;
        if (hipMalloc(ix->rx_pstart16.put(), n16 * 2) == hipSuccess &&
            hipMalloc(ix->rx_slice_e0.put(), ((size_t)ix->rx_geo.PF + 2) * 4) == hipSuccess &&
            hipMalloc(ix->rx_slice_fmax.put(), ((size_t)ix->rx_geo.PF + 2) * 2) == hipSuccess) {
            hipLaunchKernelGGL(k_rx_pstart16, dim3(grid_for(ix, (int64_t)((n16 + 255) / 256), 16)), dim3(256), 0, ix->stream,
                               ix->rx_pstart, ix->modulo, ix->rx_geo.w, ix->rx_geo.PF, ix->rx_pstart16, ix->rx_slice_e0);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_rx_slice_fmax, dim3(grid_for(ix, (int64_t)((ix->rx_geo.PF + 3) / 4), 16)), dim3(256), 0, ix->stream,
                               ix->rx_slice_e0, ix->rx_pfreq, ix->rx_geo.PF, ix->rx_slice_fmax);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(ix->stream));
        } else {
            (void)hipGetLastError();
            static_cast<RxDir16 &>(*ix) = RxDir16();
        }
    }
    return rx_build_slots(ix);
}

// Radix-path view of the index (kmm_radix.hpp): entries regrouped in bucket order (whatever order the caller's
// hashes_to_index uses) + the exclusive prefix of the bucket sizes, which serves as the bucket directory of any
// 2^w-bucket slice.  Built from the raw arrays while they are still in HBM.
int rx_build(kmm_index *ix, const int32_t *h2i, const int32_t *nk, const uint64_t *kmers, const int32_t *nodes,
             const uint16_t *freqs)
{
    const uint64_t M = ix->modulo;
    if (const char *env = getenv("KMM_RX_FILTER")) // experiments: 0 = plain pass 2 and the fan-out chosen without the filter
        ix->rx_filter = atoi(env) != 0;
    if (const char *env = getenv("KMM_RX_FILTER_SLOTS")) // experiments: 0 = the bucket bitmap where the slot filter would serve
        ix->rx_filter_slots = atoi(env) != 0;
    if (const char *env = getenv("KMM_RX_P3_FP")) // experiments: 0 = pass 3's plain entry loop where the fingerprint form would serve
        ix->rx_p3_fp = atoi(env) != 0;
    ix->rx_why_not = 1;
    if (M >= (1ull << 31))
        return KMM_OK; // beyond the index format's int32 tables: no radix path; the direct path serves every batch
    DevBuf sizes;
    std::vector<DevBuf> scratch(2 * SCAN_MAX_LEVELS);
    int rc = KMM_OK;
    hipError_t e = hipSuccess;
    bool overlap = false;
    do {
        if ((rc = ensure(sizes, (size_t)(M + 1) * 4))) break;
        if ((e = hipMalloc(ix->rx_pstart.put(), (size_t)(M + 1) * RxViewBytes::pstart))) break;
        hipLaunchKernelGGL(k_rx_bucket_sizes, dim3(grid_for(ix, (int64_t)((M + 256) / 256), 16)), dim3(256), 0,
                           ix->stream, h2i, nk, M, ix->n_entries, (uint32_t *)sizes.p);
        // an index whose buckets overlap (sum of the bucket sizes > n_entries: legal for the reference's loop, which only
        // follows (start, count) per bucket) has no bucket-ordered copy of bounded size, and a 32-bit prefix could
        // wrap: such an index is served by the direct path alone
        unsigned long long sum64 = 0;
        if ((e = hipMemsetAsync(ix->queue, 0, sizeof(unsigned long long), ix->stream))) break;
        hipLaunchKernelGGL(k_sum_u32, dim3(grid_for(ix, (int64_t)((M + 256) / 256), 8)), dim3(256), 0, ix->stream,
                           (const uint32_t *)sizes.p, M + 1, ix->queue);
        if ((e = hipMemcpyAsync(&sum64, ix->queue, 8, hipMemcpyDeviceToHost, ix->stream))) break;
        if ((e = hipStreamSynchronize(ix->stream))) break;
        if (sum64 > (unsigned long long)ix->n_entries) {
            overlap = true;
            break;
        }
        if ((rc = scan_exclusive((const uint32_t *)sizes.p, ix->rx_pstart, M + 1, scratch, 0, ix->stream))) break;
        uint32_t total = 0;
        if ((e = hipMemcpyAsync(&total, ix->rx_pstart + M, 4, hipMemcpyDeviceToHost, ix->stream))) break;
        if ((e = hipStreamSynchronize(ix->stream))) break;
        ix->rx_S = total; // = sum64 <= n_entries < 2^31
        {   // occupancy bitmap for pass 2's empty-bucket filter, padded by one coarse partition's worth of words
            // (k_rx_p2f loads whole partitions); optional: without the memory for it the plain pass 2 runs
            const size_t occ_words = (size_t)((M + 31) / 32) + ((size_t)1 << (P2F_LOGBITS + 2 - 5)); // (up to 4 buckets per LDS bit)
            if (hipMalloc(ix->rx_occ.put(), occ_words * 4) == hipSuccess) {
                if ((e = hipMemsetAsync(ix->rx_occ, 0, occ_words * 4, ix->stream))) break;
                hipLaunchKernelGGL(k_rx_build_occ, dim3(grid_for(ix, (int64_t)((M / 32 + 256) / 256), 16)), dim3(256), 0, ix->stream,
                                   ix->rx_pstart, M, ix->rx_occ);
            } else {
                (void)hipGetLastError();
            }
        }
        const size_t S = total ? total : 1;
        if ((e = hipMalloc(ix->rx_pkeys.put(), S * RxViewBytes::pkeys))) break;
        if ((e = hipMalloc(ix->rx_pkeys_raw.put(), S * RxViewBytes::pkeys_raw))) break;
        if ((e = hipMalloc(ix->rx_pfreq.put(), S * RxViewBytes::pfreq))) break;
        if ((e = hipMalloc(ix->rx_pnodes.put(), S * RxViewBytes::pnodes))) break;
        if ((e = hipMalloc(ix->rx_porig.put(), S * RxViewBytes::porig))) break;
        if ((e = hipMalloc(ix->rx_ecnt.put(), S * RxViewBytes::ecnt))) break;
        if ((e = hipMemsetAsync(ix->rx_ecnt, 0, S * RxViewBytes::ecnt, ix->stream))) break;
        hipLaunchKernelGGL(k_rx_pack, dim3(grid_for(ix, (int64_t)((M + 255) / 256), 16)), dim3(256), 0, ix->stream, h2i,
                           kmers, nodes, freqs, M, ix->max_node_id, ix->rx_pstart, ix->rx_pkeys_raw, ix->rx_pfreq,
                           ix->rx_pnodes, ix->rx_porig);
        if ((e = hipGetLastError())) break;
        if ((e = hipStreamSynchronize(ix->stream))) break;
        // the entries once more in NODE order, for the flush (k_rx_flush_sorted): counting sort by node.  Optional:
        // without the memory for it the flush walks the entries in bucket order (k_rx_flush).
        // (few nodes with many entries each — a graph with 1000 hot nodes — aggregate in the bucket-order kernel's
        // LDS table instead: 1.1 ms against 2.3 ms per flush at 10^8 entries / 1000 nodes; 4.0 against 2.0 ms when
        // every entry has its own node)
        if (total) {
            const uint64_t n_nodes = (uint64_t)ix->max_node_id + 1;
            DevBuf hist, cursor;
            if (n_nodes + 1 < 0xFFFFFFFFull && (uint64_t)total / n_nodes < 8 && ensure(hist, (size_t)(n_nodes + 1) * 4) == KMM_OK &&
                ensure(cursor, (size_t)(n_nodes + 1) * 4) == KMM_OK &&
                hipMalloc(ix->rx_norder.put(), S * RxViewBytes::norder) == hipSuccess &&
                hipMalloc(ix->rx_nnode.put(), S * RxViewBytes::nnode) == hipSuccess) {
                bool ok = hipMemsetAsync(hist.p, 0, (size_t)(n_nodes + 1) * 4, ix->stream) == hipSuccess;
                hipLaunchKernelGGL(k_rx_node_hist, dim3(grid_for(ix, (int64_t)((S + 255) / 256), 16)), dim3(256), 0,
                                   ix->stream, ix->rx_pnodes, (uint64_t)total, (uint32_t *)hist.p);
                ok = ok && scan_exclusive((const uint32_t *)hist.p, (uint32_t *)cursor.p, n_nodes + 1, scratch, 0,
                                          ix->stream) == KMM_OK;
                hipLaunchKernelGGL(k_rx_node_scatter, dim3(grid_for(ix, (int64_t)((S + 255) / 256), 16)), dim3(256), 0,
                                   ix->stream, ix->rx_pnodes, (uint64_t)total, (uint32_t *)cursor.p, ix->rx_norder,
                                   ix->rx_nnode);
                ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(ix->stream) == hipSuccess;
                if (!ok) {
                    (void)ix->rx_norder.reset();
                    (void)ix->rx_nnode.reset();
                }
            } else {
                (void)hipGetLastError();
                (void)ix->rx_norder.reset();
                (void)ix->rx_nnode.reset();
            }
        }
    } while (0);
    (void)sizes.reset(); // (here, not at the end: the repack below allocates the optional 16-bit directory)
    scratch.clear();
    if (rc != KMM_OK || e != hipSuccess || overlap) {
        // the radix view is optional: without the memory for it (or for an index with overlapping buckets) the
        // direct path serves every batch; any other failure is an error
        const bool nomem = rc == KMM_ERR_NOMEM || e == hipErrorOutOfMemory;
        (void)hipGetLastError();
        static_cast<RxArrays &>(*ix) = RxArrays();
        ix->rx_ok = false;
        if (overlap || nomem) {
            ix->rx_why_not = overlap ? 4 : 3;
            if (getenv("KMM_VERBOSE"))
                fprintf(stderr, "libkmm: radix view not built (%s): every batch takes the direct path\n",
                        overlap ? "the buckets of the index overlap" : "out of HBM");
            return KMM_OK;
        }
        if (rc != KMM_OK)
            return rc;
        return fail(KMM_ERR_HIP, "radix index build: %s", hipGetErrorString(e));
    }
    // slice width and fan-out (rx_choose_geometry); experiments / tests force the slice width and the fine-partition bits
    std::optional<int> w_force;
    if (const char *env = getenv("KMM_RX_W"))
        w_force = atoi(env);
    const int f2_force = getenv("KMM_RX_F2") ? atoi(getenv("KMM_RX_F2")) : -1;
    ix->rx_no_mid = getenv("KMM_RX_NO_MID") != nullptr;
    const std::optional<RxGeometry> geo = rx_choose_geometry(M, ix->rx_S, ix->rx_filter, w_force, f2_force);
    ix->rx_ok = geo.has_value();
    if (geo)
        ix->rx_geo = *geo;
    ix->rx_why_not = ix->rx_ok ? 0 : 2;
    if (getenv("KMM_VERBOSE"))
        fprintf(stderr, "libkmm: modulo %llu, %llu entries: radix path %s (2^%d buckets per slice, %u x %u partitions)\n",
                (unsigned long long)M, (unsigned long long)ix->rx_S, ix->rx_ok ? "available" : "NOT available: slices too "
                "dense for LDS or more than 512 x 512 of them", ix->rx_geo.w, ix->rx_geo.F1, ix->rx_geo.F2);
    if (ix->rx_ok)
        KMMCHK(rx_repack_keys(ix));
    ix->rx_min_units = rx_min_units(M, ix->rx_S); // auto: where the radix path overtakes the direct one
    if (const char *env = getenv("KMM_RX_MIN_UNITS"))
        ix->rx_min_units = strtoll(env, nullptr, 10);
    return KMM_OK;
}

// "part_shift", "radix_filter", "fine_bits" (kmm_set_param): a new geometry for the index, 2^w buckets per slice and, with
// f2_force >= 0, that many fine-partition bits.  RX_REFUSED: the handle stays as it was.  Else nothing of the old layout
// stays pending and the view that is there is repacked; set_ok: the radix path is available iff there is a view.
constexpr int RX_REFUSED = 1;
int rx_reconfigure(kmm_index *ix, int w, int f2_force, bool set_ok)
{
    const std::optional<RxGeometry> geo = rx_geometry(ix->modulo, ix->rx_S, ix->rx_filter, w, RX_MAXF, f2_force);
    if (!geo)
        return RX_REFUSED;
    ix->rx_geo = *geo;
    if (set_ok)
        ix->rx_ok = ix->rx_pstart != nullptr;
    if (ix->rx_pstart) {
        KMMCHK(rx_flush(ix));
        KMMCHK(rx_repack_keys(ix));
    }
    return KMM_OK;
}
