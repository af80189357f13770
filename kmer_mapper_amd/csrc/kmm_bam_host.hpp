// kmm_bam_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside an anonymous namespace, once StreamCall,
// selection_of, ensure_crc_tables and the keep queue's helpers (rkq_*, rk_snap_restore, keep_entries_last, rk_rule, RkCallMode,
// with_selected) are defined.  Host side of kmm_map_bam behind the inflater: the backend of run_call, bam_map_inflated, the forms
// that keep mates together or the records' own bytes (bam_map_mates, bam_raw_keep, bam_map_raw_mates), and the inflater of
// kmm_bam_header / kmm_bam_find_record_start (rs_*).  The kernels and run_call, which the CPU tests share, are in kmm_bam.hpp.
#pragma once

// The backend of run_call: the handle's bam_* buffers, kernels on its stream.
struct BamGpuBackend {
    kmm_index_t *ix;
    const uint8_t *d;
    uint64_t n;
    int32_t n_ref;
    uint32_t excl;
    bool qual = false; // the quality variant: four-line FASTQ, 2 l_seq + 6 bytes per kept record
    bool orig = false; // "original_strand": decode writes the kept records with FLAG 0x10 in read orientation
    bool selected = false; // a selection beyond excl is set (sel): the k_bam_*_sel kernels run
    kmm_bam::Sel sel;
    int cur = 0;
    bool named = false; // the named form ("record_names"): the k_bam_*_named kernels run, whatever the selection
    bool sfx = false;   // ... with "/1" / "/2" behind the name
    uint32_t *exempt = nullptr; // the named form under a floor: decode flags the records without qualities here, the
    uint64_t exempt_base = 0;   // bit of their quality line's offset in the inner call's text, which decode's `out` starts at this byte of

    kmm_bam::Tile *tiles(int i) { return (kmm_bam::Tile *)ix->bam_tiles[i].p; }
    kmm_bam::Ctl *ctl() { return (kmm_bam::Ctl *)ix->bam_ctl.p; }
    dim3 wave_grid(uint64_t n_tiles) { return dim3((unsigned)grid_for(ix, (int64_t)((n_tiles + 3) / 4), 16)); } // 4 waves per block
    dim3 lane_grid(uint64_t n_tiles) { return dim3((unsigned)grid_for(ix, (int64_t)((n_tiles + 255) / 256), 16)); }

    int spec(uint64_t n_tiles, uint64_t start0)
    {
        for (DevBuf &b : ix->bam_tiles)
            KMMCHK(ensure(b, (size_t)n_tiles * sizeof(kmm_bam::Tile) + 64));
        KMMCHK(ensure(ix->bam_bad, (size_t)n_tiles + 64));
        KMMCHK(ensure(ix->bam_base, (size_t)n_tiles * 8 + 64));
        KMMCHK(ensure(ix->bam_ctl, 256));
        cur = 0;
        HIPCHK(hipMemsetAsync(ctl(), 0, sizeof(kmm_bam::Ctl), ix->stream));
        HIPCHK(hipMemsetAsync(&ctl()->err_pos, 0xFF, 8, ix->stream)); // (no error)
        if (named)
            hipLaunchKernelGGL(kmm_bam::k_bam_spec_named, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, sel,
                               sfx ? 1u : 0u, tiles(0));
        else if (selected && qual)
            hipLaunchKernelGGL(kmm_bam::k_bam_spec_q_sel, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, sel, tiles(0));
        else if (selected)
            hipLaunchKernelGGL(kmm_bam::k_bam_spec_sel, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, sel, tiles(0));
        else if (qual)
            hipLaunchKernelGGL(kmm_bam::k_bam_spec_q, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, excl, tiles(0));
        else
            hipLaunchKernelGGL(kmm_bam::k_bam_spec, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, excl, tiles(0));
        HIPCHK(hipGetLastError());
        return KMM_OK;
    }
    int check(uint64_t n_tiles, uint64_t start0, kmm_bam::Ctl &h)
    {
        HIPCHK(hipMemsetAsync(&ctl()->n_bad, 0, 8, ix->stream));
        HIPCHK(hipMemsetAsync(&ctl()->first_bad, 0xFF, 8, ix->stream));
        hipLaunchKernelGGL(kmm_bam::k_bam_check, lane_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref,
                           (const kmm_bam::Tile *)tiles(cur), (uint8_t *)ix->bam_bad.p, ctl());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h, ctl(), sizeof h, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        return KMM_OK;
    }
    int fix(uint64_t n_tiles, uint64_t start0)
    {
        const kmm_bam::Tile *from = tiles(cur);
        kmm_bam::Tile *to = tiles(cur ^ 1);
        const uint8_t *bad = (const uint8_t *)ix->bam_bad.p;
        if (named)
            hipLaunchKernelGGL(kmm_bam::k_bam_fix_named, lane_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, sel,
                               sfx ? 1u : 0u, from, bad, to, ctl());
        else if (selected && qual)
            hipLaunchKernelGGL(kmm_bam::k_bam_fix_q_sel, lane_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, sel, from, bad, to, ctl());
        else if (selected)
            hipLaunchKernelGGL(kmm_bam::k_bam_fix_sel, lane_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, sel, from, bad, to, ctl());
        else if (qual)
            hipLaunchKernelGGL(kmm_bam::k_bam_fix_q, lane_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, excl, from, bad, to, ctl());
        else
            hipLaunchKernelGGL(kmm_bam::k_bam_fix, lane_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, start0, n_ref, excl, from, bad, to, ctl());
        HIPCHK(hipGetLastError());
        cur ^= 1;
        return KMM_OK;
    }
    int totals(uint64_t n_tiles, uint64_t start0, kmm_bam::Totals &h)
    {
        kmm_bam::Totals *d_tot = (kmm_bam::Totals *)((uint8_t *)ix->bam_ctl.p + 128);
        hipLaunchKernelGGL(kmm_bam::k_bam_totals, dim3(1), dim3(1024), 0, ix->stream, (const kmm_bam::Tile *)tiles(cur), n_tiles, start0,
                           (unsigned long long *)ix->bam_base.p, d_tot);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&h, d_tot, sizeof h, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        return KMM_OK;
    }
    int decode(uint64_t n_tiles, uint8_t *out)
    {
        const kmm_bam::Tile *tl = (const kmm_bam::Tile *)tiles(cur);
        const unsigned long long *bs = (const unsigned long long *)ix->bam_base.p;
        if (named)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_named, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, sel,
                               orig ? 1u : 0u, sfx ? 1u : 0u, tl, bs, out, ix->stats + KMM_STAT_REC_NO_QUAL,
                               ix->stats + KMM_STAT_REC_REVERSED, ix->stats + KMM_STAT_REC_NAME_REPLACED, exempt, exempt_base);
        else if (selected && qual && orig)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_q_rev_sel, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, sel, tl, bs,
                               out, ix->stats + KMM_STAT_REC_NO_QUAL, ix->stats + KMM_STAT_REC_REVERSED);
        else if (selected && qual)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_q_sel, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, sel, tl, bs,
                               out, ix->stats + KMM_STAT_REC_NO_QUAL);
        else if (selected && orig)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_rev_sel, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, sel, tl, bs,
                               out, ix->stats + KMM_STAT_REC_REVERSED);
        else if (selected)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_sel, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, sel, tl, bs, out);
        else if (qual && orig)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_q_rev, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, excl, tl, bs,
                               out, ix->stats + KMM_STAT_REC_NO_QUAL, ix->stats + KMM_STAT_REC_REVERSED);
        else if (qual)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_q, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, excl, tl, bs,
                               out, ix->stats + KMM_STAT_REC_NO_QUAL);
        else if (orig)
            hipLaunchKernelGGL(kmm_bam::k_bam_decode_rev, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, excl, tl, bs,
                               out, ix->stats + KMM_STAT_REC_REVERSED);
        else
            hipLaunchKernelGGL(kmm_bam::k_bam_decode, wave_grid(n_tiles), dim3(256), 0, ix->stream, d, n, n_tiles, n_ref, excl, tl, bs, out);
        HIPCHK(hipGetLastError());
        return KMM_OK;
    }
};

// The named form under the floor of the record-hits mode, in front of decode: the handle's exemption bitset over
// the n_text bytes of the inner records call's text, zeroed, the flags of the waiting mate 1's `carry` bytes at its start; decode
// then writes behind them.  Any other form: nothing.  While the guard lives, the mark pass of the inner call reads the bitset.
struct RqExemptCall {
    kmm_index_t *ix;
    ~RqExemptCall() { ix->rq_exempt = nullptr, ix->rq_text_off = 0; }
};

int bam_exempt_begin(kmm_index_t *ix, BamGpuBackend &be, int64_t n_text, int64_t carry)
{
    if (!be.named || !be.qual)
        return KMM_OK;
    const size_t bytes = ((size_t)n_text / 32 + 2) * 4, carried = ((size_t)carry + 31) / 32 * 4;
    KMMCHK(ensure(ix->rq_exempt_buf, bytes));
    HIPCHK(hipMemsetAsync(ix->rq_exempt_buf.p, 0, bytes, ix->stream));
    if (carry > 0 && ix->bam_mate_exempt_len == carry)
        HIPCHK(hipMemcpyAsync(ix->rq_exempt_buf.p, ix->bam_mate_exempt.p, carried, hipMemcpyDeviceToDevice, ix->stream));
    be.exempt = (uint32_t *)ix->rq_exempt_buf.p;
    be.exempt_base = (uint64_t)carry;
    ix->rq_exempt = be.exempt;
    return KMM_OK;
}

// "The stream ends with an unpaired record" (DESIGN 4.23): a mate 1 is left when the stream's last call has nothing more for it.
// param: the parameter that pairs the records, "record_names_pairs" or "record_bam_mates" (4.25).
int bam_unpaired_end(const char *param, int64_t n_selected)
{
    return fail(KMM_ERR_MALFORMED, "kmm_map_bam: \"%s\" is 1 and the stream ends with an unpaired record: it holds %lld "
                "selected records, the last one has no mate (a selection that removes one mate of a pair is an error here; nothing of "
                "the call is appended)", param, (long long)n_selected);
}

// What a kmm_map_bam window has added to the handle, taken back on every way out while `armed` (a path clears it once nothing
// more of the window can fail); the failure's message stays.  Always: the call and record counters, the pair ordinal and what the
// inner records call appended (rk_snap; after an inner call that put its own entries back, the same values once more).  walk (the
// mate paths; plain "record_bam" passes false): also the walk's false starts and continuations and the decode's three
// device counters, neighbours in the first shard of the statistics (d_counters: their copy from before the decode, null while none).
struct BamWindowUndo {
    kmm_index_t *ix;
    const kmm_bam::CallOut &co;
    bool walk;
    int64_t pairs0;
    bool armed = true;
    unsigned long long *d_counters = nullptr;

    ~BamWindowUndo()
    {
        if (!armed)
            return;
        const std::string msg = g_err;
        ix->bam_pairs_done = pairs0;
        ix->bam_calls--;
        ix->bam_records -= (int64_t)co.recs;
        ix->bam_excluded -= (int64_t)co.excluded;
        if (walk) {
            ix->bam_false_starts -= (int64_t)co.false_starts;
            ix->bam_continuations -= (int64_t)co.continuations;
            if (d_counters && hipMemcpyAsync(ix->stats + KMM_STAT_REC_NO_QUAL, d_counters, 24, hipMemcpyDeviceToDevice, ix->stream) != hipSuccess)
                (void)hipGetLastError();
        }
        rk_snap_restore(ix);
        g_err = msg;
    }
};

// The front half of the two mate paths, for a window with selected records: the three device counters saved (undo.d_counters),
// the waiting mate's text copied in front of bam_out, the window's records decoded behind it, the inner records call over both in
// the pair form (fmt: the text's format; raw: under rk_raw_call too), and the check that it took whole pairs and no more.
// *taken / *recs: the inner call's (0 when fewer than two records stand there).
int bam_mates_front(kmm_index_t *ix, const StreamCall &c, BamGpuBackend &be, const kmm_bam::CallOut &co, int64_t n_raw, int fmt, bool raw,
                    BamWindowUndo &undo, int64_t *taken, int64_t *recs)
{
    static_assert(KMM_STAT_REC_REVERSED == KMM_STAT_REC_NO_QUAL + 1 && KMM_STAT_REC_NAME_REPLACED == KMM_STAT_REC_NO_QUAL + 2, "one copy");
    const int64_t carry = ix->bam_mate_len, n_rec = (int64_t)co.recs + (carry > 0 ? 1 : 0), n_text = carry + (int64_t)co.out_bytes;
    KMMCHK(ensure(ix->rk_names_ctl, 64));
    KMMCHK(ensure(ix->bam_out, (size_t)n_text + 64));
    undo.d_counters = (unsigned long long *)((uint8_t *)ix->rk_names_ctl.p + 16);
    HIPCHK(hipMemcpyAsync(undo.d_counters, ix->stats + KMM_STAT_REC_NO_QUAL, 24, hipMemcpyDeviceToDevice, ix->stream));
    if (carry > 0)
        HIPCHK(hipMemcpyAsync(ix->bam_out.p, ix->bam_mate.p, (size_t)carry, hipMemcpyDeviceToDevice, ix->stream));
    const RqExemptCall exempting{ix};
    KMMCHK(bam_exempt_begin(ix, be, n_text, carry));
    KMMCHK(be.decode(((uint64_t)n_raw + kmm_bam::TILE - 1) / kmm_bam::TILE, (uint8_t *)ix->bam_out.p + carry));
    if (n_rec >= 2) {
        const RkCallMode mode(ix, true, raw);
        KMMCHK(kmm_map_records(ix, (const uint8_t *)ix->bam_out.p, n_text, fmt, c.k, c.max_freq, c.also_revcomp, c.lut, taken, recs));
        if (*recs != (n_rec & ~(int64_t)1) || ((n_rec & 1) == 0 && *taken != n_text) || *taken > n_text)
            return fail(KMM_ERR_INTERNAL, "kmm_map_bam: %lld of %lld decoded bytes, %lld of %lld records mapped as pairs", (long long)*taken,
                        (long long)n_text, (long long)*recs, (long long)n_rec);
    }
    return KMM_OK;
}

// The selected records of a kmm_map_bam window as mates ("record_names_pairs"), behind run_call: the window's
// records are decoded BEHIND the text of the mate 1 that the window before left over, and the inner records call takes carry +
// decoded text in the interleaved pair form (rk_mates_call: whole pairs only, the names of every pair compared).  An odd last
// record's text stays unconsumed and becomes the next carry.  A failing call leaves carry, ordinals, queues and counters as they were.
int bam_map_mates(kmm_index_t *ix, const StreamCall &c, BamGpuBackend &be, const kmm_bam::CallOut &co, int64_t n_raw)
{
    const int64_t carry = ix->bam_mate_len, n_text = carry + (int64_t)co.out_bytes;
    const bool decoded = co.recs > 0;
    BamWindowUndo undo{ix, co, true, ix->bam_pairs_done};
    ix->rk_snap.valid = false;
    int64_t taken = 0, recs = 0;
    if (decoded)
        KMMCHK(bam_mates_front(ix, c, be, co, n_raw, KMM_FORMAT_FASTQ, false, undo, &taken, &recs));
    const int64_t left = decoded ? n_text - taken : carry; // the text of a mate 1 whose mate has not come
    if (c.last_chunk && left > 0)
        return bam_unpaired_end("record_names_pairs", 2 * ix->bam_pairs_done + 1);
    undo.armed = false;
    if (decoded && left > 0) {
        KMMCHK(ensure(ix->bam_mate, (size_t)left + 64)); // (may free and reallocate: a device-wide sync, rare)
        HIPCHK(hipMemcpyAsync(ix->bam_mate.p, (const uint8_t *)ix->bam_out.p + taken, (size_t)left, hipMemcpyDeviceToDevice, ix->stream));
        if (be.exempt) { // (the waiting mate's exemption flag goes with its text)
            KMMCHK(ensure(ix->bam_mate_exempt, ((size_t)left + 31) / 32 * 4 + 64));
            hipLaunchKernelGGL(k_rq_bits_move, dim3((unsigned)grid_for(ix, (left / 32 + 256) / 256, 8)), dim3(256), 0, ix->stream,
                               (const uint32_t *)be.exempt, (uint64_t)taken, (uint64_t)left, (uint32_t *)ix->bam_mate_exempt.p);
            HIPCHK(hipGetLastError());
        }
    }
    if (decoded) {
        ix->bam_mate_len = left;
        ix->bam_mate_exempt_len = be.exempt ? left : 0;
    }
    if (c.n_records)
        *c.n_records = recs;
    return KMM_OK;
}

// The scratch of the raw walk in the handle's bam_raw, both forms: per tile the record base and the kept bytes' base (8 bytes
// each), then the kept bytes and the kept records (4 each); behind them, 16-aligned, tot: the window's kept bytes, its kept
// records and, in tot[2], its selected records.  The walk's first step scans the tiles themselves:
// k_bam_raw_scan((const uint32_t *)tiles + 4, 8u, ...) reads Tile::recs as word 4 of 8.
static_assert(sizeof(kmm_bam::Tile) == 32 && offsetof(kmm_bam::Tile, recs) == 16, "k_bam_raw_scan reads Tile::recs as word 4 of 8");
struct BamRawScratch { unsigned long long *rec_base, *byte_base, *tot; uint32_t *kept_bytes, *kept_recs; };

int bam_raw_scratch(kmm_index_t *ix, uint64_t n_tiles, BamRawScratch &w)
{
    const size_t off_kept = 2 * (size_t)n_tiles * 8, off_tot = (off_kept + 2 * (size_t)n_tiles * 4 + 15) & ~(size_t)15;
    KMMCHK(ensure(ix->bam_raw, off_tot + 64));
    uint8_t *p = (uint8_t *)ix->bam_raw.p;
    unsigned long long *rec_base = (unsigned long long *)p;
    uint32_t *kept_bytes = (uint32_t *)(p + off_kept);
    w = {rec_base, rec_base + n_tiles, (unsigned long long *)(p + off_tot), kept_bytes, kept_bytes + n_tiles};
    return KMM_OK;
}

// The kept records of a kmm_map_bam window as they stand in the file ("record_bam"), behind the inner records call:
// its co.recs entries are the last ones of the entry queue, one per selected record in file order.  Five steps on the handle's
// stream, no read-back: the record base of every tile (a scan of Tile::recs), the kept raw bytes and records per tile, their
// scans, the copy behind the queue's tail, the tail's advance.  The queue holds room for the window's consumed bytes first.
int bam_raw_keep(kmm_index_t *ix, BamGpuBackend &be, const kmm_bam::CallOut &co, int64_t n_raw)
{
    const uint64_t n_tiles = ((uint64_t)n_raw + kmm_bam::TILE - 1) / kmm_bam::TILE;
    kmm_index::RkQueue &q = ix->rkq[0];
    BamRawScratch w;
    KMMCHK(bam_raw_scratch(ix, n_tiles, w));
    KMMCHK(rkq_reserve(ix, q, (int64_t)co.consumed));
    KeepEntries e; // (the inner call's entries)
    if (!keep_entries_last(ix, co.recs, e))
        return fail(KMM_ERR_INTERNAL, "kmm_map_bam: %llu selected records and %lld entries pending", co.recs, (long long)ix->rhq_pending);
    const RkRule rule = rk_rule(ix);
    const kmm_bam::Tile *tl = be.tiles(be.cur);
    unsigned long long *tail = (unsigned long long *)q.ctl.p;
    const kmm_bam::Sel sel = be.sel; // (its excl is the exclude mask, which the form without a selection reads from here)
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_BAM_RAW));
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_scan, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)tl + 4, 8u, n_tiles, w.rec_base, w.tot + 2);
    with_selected(be.selected, [&](auto S) {
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_count<decltype(S)::value>, be.wave_grid(n_tiles), dim3(256), 0, ix->stream, be.d, be.n, n_tiles,
                           be.n_ref, sel, tl, (const unsigned long long *)w.rec_base, e.hits, e.windows, e.n, rule, w.kept_bytes, w.kept_recs);
    });
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_scan, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)w.kept_bytes, 1u, n_tiles, w.byte_base, w.tot);
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_scan, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)w.kept_recs, 1u, n_tiles,
                       (unsigned long long *)nullptr, w.tot + 1);
    with_selected(be.selected, [&](auto S) {
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_copy<decltype(S)::value>, be.wave_grid(n_tiles), dim3(256), 0, ix->stream, be.d, be.n, n_tiles,
                           be.n_ref, sel, tl, (const unsigned long long *)w.rec_base, e.hits, e.windows, e.n, rule, (const uint32_t *)w.kept_bytes,
                           (const unsigned long long *)w.byte_base, (const unsigned long long *)tail, (uint8_t *)q.text.p);
    });
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_advance, dim3(1), dim3(64), 0, ix->stream, tail, (const unsigned long long *)w.tot);
    KMMCHK(tm.end());
    HIPCHK(hipGetLastError());
    q.bound += (int64_t)co.consumed;
    return KMM_OK;
}

// The selected records of a kmm_map_bam window as mates whose own bytes are kept ("record_bam_mates"), behind run_call.
// As bam_map_mates: the window's records are decoded behind the FASTA text of the mate 1 that the window before left over, and the
// inner records call takes carry + decoded text in the pair form — whole pairs of entries, no text appended, no name lines
// compared.  Then the raw walk in its pair form: record base, count (which reports the odd last record), the mate check over the
// records' own read_name bytes, ONE read-back (strangers, the odd record), scans, the carried mate 1 to the queue's tail, the
// tiles' records behind it, the tail's advance.  The odd last record's text and raw bytes become the next carry.  A call that fails
// leaves the carries, the ordinal, the queues and the counters as it found them.
int bam_map_raw_mates(kmm_index_t *ix, const StreamCall &c, BamGpuBackend &be, const kmm_bam::CallOut &co, int64_t n_raw, bool qual)
{
    const int64_t carry = ix->bam_mate_len, pairs0 = ix->bam_pairs_done, raw_carry = ix->bam_raw_mate_len;
    const uint32_t carried = carry > 0 ? 1u : 0u;
    const int64_t n_rec = (int64_t)co.recs + carried, n_text = carry + (int64_t)co.out_bytes;
    BamWindowUndo undo{ix, co, true, pairs0};
    ix->rk_snap.valid = false;
    if (carried && (raw_carry < 37 || raw_carry > 0x7FFFFFFFll + 4))
        return fail(KMM_ERR_INTERNAL, "kmm_map_bam: a mate 1 waits with %lld bytes of text and %lld raw bytes", (long long)carry, (long long)raw_carry);
    if (co.recs == 0) { // (nothing selected: a mate 1 goes on waiting, unless the stream ends here)
        if (c.last_chunk && carried)
            return bam_unpaired_end("record_bam_mates", 2 * pairs0 + 1);
        undo.armed = false;
        return KMM_OK;
    }
    int64_t taken = 0, recs = 0;
    unsigned long long h_ctl[3] = {kmm_bam::NONE, kmm_bam::NONE, kmm_bam::NONE};
    KMMCHK(ensure(ix->bam_raw_ctl, 64));
    KMMCHK(bam_mates_front(ix, c, be, co, n_raw, qual ? KMM_FORMAT_FASTQ : KMM_FORMAT_FASTA2, true, undo, &taken, &recs));
    // the raw walk, pair form
    const uint64_t n_tiles = ((uint64_t)n_raw + kmm_bam::TILE - 1) / kmm_bam::TILE;
    kmm_index::RkQueue &q = ix->rkq[0];
    BamRawScratch w;
    KMMCHK(bam_raw_scratch(ix, n_tiles, w));
    unsigned long long *ctl = (unsigned long long *)ix->bam_raw_ctl.p;
    const uint64_t n_entries = (uint64_t)recs;
    KMMCHK(ensure(ix->bam_raw_pos, (size_t)n_entries * 8 + 64)); // (the start of every selected record that has an entry)
    unsigned long long *pos = (unsigned long long *)ix->bam_raw_pos.p;
    KeepEntries e; // (the inner call's entries; none: the kernels read none — e >= n_entries comes first — and the pointers are null)
    if (!keep_entries_last(ix, n_entries, e))
        return fail(KMM_ERR_INTERNAL, "kmm_map_bam: %lld entries of the call and %lld entries pending", (long long)recs, (long long)ix->rhq_pending);
    const RkPairRule rule = rk_pair_rule(ix);
    const kmm_bam::Tile *tl = be.tiles(be.cur);
    const uint8_t *d_carry = carried ? (const uint8_t *)ix->bam_raw_mate.p : nullptr;
    const uint32_t carry_len = carried ? (uint32_t)raw_carry : 0u;
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_BAM_RAW_MATES));
    HIPCHK(hipMemsetAsync(ctl, 0xFF, 24, ix->stream));
    if (n_entries > 0)
        HIPCHK(hipMemsetAsync(pos, 0xFF, (size_t)n_entries * 8, ix->stream));
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_scan, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)tl + 4, 8u, n_tiles, w.rec_base, w.tot + 2);
    with_selected(be.selected, [&](auto S) {
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_count_pairs<decltype(S)::value>, be.wave_grid(n_tiles), dim3(256), 0, ix->stream, be.d, be.n,
                           n_tiles, be.n_ref, be.sel, tl, (const unsigned long long *)w.rec_base, e.hits, e.windows, n_entries, rule, carried,
                           w.kept_bytes, w.kept_recs, pos, ctl);
    });
    if (n_entries > 0)
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_pair_names, be.wave_grid(n_entries / 2), dim3(256), 0, ix->stream, be.d,
                           co.consumed, (const unsigned long long *)pos, n_entries, carried, d_carry, carry_len, ctl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_ctl, ctl, 24, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    if (h_ctl[0] != kmm_bam::NONE) {
        (void)tm.end();
        const long long p = (long long)(pairs0 + (int64_t)h_ctl[0]);
        return fail(KMM_ERR_MALFORMED, "kmm_map_bam: \"record_bam_mates\" is 1 and pair %lld of the stream is none: records %lld and %lld "
                    "are not mates (their read_name bytes differ): collate the file by name (`samtools collate`) and exclude secondary "
                    "and supplementary records (0x900) (nothing of the call is appended)", p, 2 * p, 2 * p + 1);
    }
    const bool odd = (n_rec & 1) != 0;
    if (odd != (h_ctl[1] != kmm_bam::NONE) || (odd && (h_ctl[1] >= co.consumed || h_ctl[2] > co.consumed - h_ctl[1]))) {
        (void)tm.end();
        return fail(KMM_ERR_INTERNAL, "kmm_map_bam: %lld selected records with the carry, the odd last one reported at %llu (%llu bytes)",
                    (long long)n_rec, h_ctl[1], h_ctl[2]);
    }
    if (c.last_chunk && odd) {
        (void)tm.end();
        return bam_unpaired_end("record_bam_mates", 2 * ix->bam_pairs_done + 1);
    }
    if (odd) {
        // the odd last record's text (what the inner call left) and raw bytes go to the SPARE carry buffers, before anything is
        // appended: a failure here still leaves the queues and the waiting mate as the call found them
        const int64_t left = n_text - taken;
        KMMCHK(ensure(ix->bam_mate_next, (size_t)left + 64)); // (may free and reallocate: a device-wide sync, rare)
        KMMCHK(ensure(ix->bam_raw_mate_next, (size_t)h_ctl[2] + 64));
        HIPCHK(hipMemcpyAsync(ix->bam_mate_next.p, (const uint8_t *)ix->bam_out.p + taken, (size_t)left, hipMemcpyDeviceToDevice, ix->stream));
        HIPCHK(hipMemcpyAsync(ix->bam_raw_mate_next.p, be.d + h_ctl[1], (size_t)h_ctl[2], hipMemcpyDeviceToDevice, ix->stream));
    }
    if (n_entries > 0) {
        KMMCHK(rkq_reserve(ix, q, (int64_t)co.consumed + (int64_t)carry_len));
        unsigned long long *tail = (unsigned long long *)q.ctl.p;
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_scan, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)w.kept_bytes, 1u, n_tiles, w.byte_base, w.tot);
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_scan, dim3(1), dim3(1024), 0, ix->stream, (const uint32_t *)w.kept_recs, 1u, n_tiles,
                           (unsigned long long *)nullptr, w.tot + 1);
        if (carried) {
            const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)carry_len + 4095) / 4096, 64);
            hipLaunchKernelGGL(kmm_bam::k_bam_raw_carry, dim3(blocks), dim3(256), 0, ix->stream, d_carry, carry_len, e.hits, e.windows, n_entries,
                               rule, (const unsigned long long *)tail, (uint8_t *)q.text.p);
        }
        with_selected(be.selected, [&](auto S) {
            hipLaunchKernelGGL(kmm_bam::k_bam_raw_copy_pairs<decltype(S)::value>, be.wave_grid(n_tiles), dim3(256), 0, ix->stream, be.d, be.n,
                               n_tiles, be.n_ref, be.sel, tl, (const unsigned long long *)w.rec_base, e.hits, e.windows, n_entries, rule, carried,
                               carry_len, (const uint32_t *)w.kept_bytes, (const unsigned long long *)w.byte_base,
                               (const unsigned long long *)tail, (uint8_t *)q.text.p);
        });
        hipLaunchKernelGGL(kmm_bam::k_bam_raw_advance_pairs, dim3(1), dim3(64), 0, ix->stream, tail, (const unsigned long long *)w.tot, e.hits,
                           e.windows, n_entries, rule, carried, carry_len);
        HIPCHK(hipGetLastError());
        q.bound += (int64_t)co.consumed + (int64_t)carry_len;
    }
    KMMCHK(tm.end());
    undo.armed = false;
    ix->rk_snap.valid = false;
    // the next carry: what went into the spare buffers becomes the waiting mate (the kernels that read the old one are queued
    // in front of whatever writes that buffer next); nothing here can fail
    if ((n_rec & 1) != 0) {
        std::swap(ix->bam_mate, ix->bam_mate_next);
        std::swap(ix->bam_raw_mate, ix->bam_raw_mate_next);
        ix->bam_mate_len = n_text - taken;
        ix->bam_raw_mate_len = (int64_t)h_ctl[2];
    } else {
        ix->bam_mate_len = 0;
        ix->bam_raw_mate_len = 0;
    }
    if (c.n_records)
        *c.n_records = recs;
    return KMM_OK;
}

// The inflated bytes of a kmm_map_bam call (d_raw[0, n_raw): the carry of the call before in front): the header on a stream's
// first call, then the records up to the last complete one (*used), decoded into two-line FASTA in HBM and mapped by
// kmm_map_records.  *short_header: a first window that ends inside the header (nothing is used).
int bam_map_inflated(kmm_index_t *ix, const StreamCall &c, uint8_t *d_raw, int64_t head, int64_t tail_stop, int64_t n_raw, int64_t *used,
                     bool *short_header)
{
    *used = 0;
    *short_header = false;
    uint64_t start0 = 0;
    if (c.mid_stream) {
        // a rank's share: no header — n_ref is the caller's ("bam_n_ref"), the first record starts `head` bytes
        // into the stream's first member ("bgzf_head_skip"), where kmm_bam_find_record_start found it
        ix->bam_n_ref = (int32_t)ix->bam_n_ref_param;
        ix->bam_hdr_valid = false; // (kmm_bam_stream_header: a share has no header)
        start0 = (uint64_t)head;
    } else if (c.new_stream) {
        // the header (magic, l_text, text, n_ref, the references) is read back in growing prefixes: its length is only known by
        // walking it, and it is read once per stream
        ix->bam_n_ref = -1;
        ix->bam_hdr_valid = false;
        std::vector<uint8_t> h;
        uint64_t want = n_raw < (1 << 16) ? (uint64_t)n_raw : 1u << 16, hdr_end = 0;
        int32_t n_ref = 0;
        for (;;) {
            h.resize(want);
            if (want)
                HIPCHK(hipMemcpyAsync(h.data(), d_raw, want, hipMemcpyDeviceToHost, ix->stream));
            HIPCHK(hipStreamSynchronize(ix->stream));
            const int r = kmm_bam::parse_header(h.data(), want, &hdr_end, &n_ref);
            if (r < 0)
                return fail(KMM_ERR_MALFORMED, "kmm_map_bam: the stream does not start with a BAM header (magic \"BAM\\1\", lengths)");
            if (r == 0)
                break;
            if (want == (uint64_t)n_raw) {
                if (c.last_chunk)
                    return fail(KMM_ERR_MALFORMED, "kmm_map_bam: the file ends inside the BAM header (%lld bytes)", (long long)n_raw);
                *short_header = true;
                return KMM_OK;
            }
            want = want * 4 < (uint64_t)n_raw ? want * 4 : (uint64_t)n_raw;
        }
        ix->bam_n_ref = n_ref;
        ix->bam_hdr.assign(h.begin(), h.begin() + (std::ptrdiff_t)hdr_end); // (kmm_bam_stream_header: magic through the last reference)
        ix->bam_hdr_valid = true;
        ix->bam_header_bytes += (int64_t)hdr_end;
        start0 = hdr_end;
    } else if (ix->bam_n_ref < 0) {
        return fail(KMM_ERR_INVALID_ARG, "kmm_map_bam: no BAM stream was started on this handle (KMM_FORMAT_NEW_STREAM)");
    }
    const bool qual = record_quality(ix) > 0;
    BamGpuBackend be{ix, d_raw, (uint64_t)n_raw, ix->bam_n_ref, ix->bam_excl, qual, ix->original_strand != 0};
    KMMCHK(selection_of(ix, "kmm_map_bam", false, ix->bam_n_ref, be.sel));
    be.selected = !be.sel.flags_only();
    // (the named form: its text goes to the records front end as FASTQ whatever `qual` says; under the floor of the record-hits
    // mode — `qual` — decode also flags the records without qualities for the mark pass)
    be.named = ix->record_names != 0;
    be.sfx = ix->record_names_mate_suffix != 0;
    kmm_bam::CallOut co;
    KMMCHK(kmm_bam::run_call(be, (uint64_t)n_raw, start0, co));
    ix->bam_false_starts += (int64_t)co.false_starts;
    ix->bam_continuations += (int64_t)co.continuations;
    if (co.err_pos != kmm_bam::NONE)
        return fail(KMM_ERR_MALFORMED, "kmm_map_bam: the record at inflated byte %llu of the call does not fit its block_size (or its "
                    "refID / next_refID / read_name are not a record's)", co.err_pos);
    if (c.last_chunk && co.consumed != (uint64_t)n_raw && tail_stop >= 0)
        return fail(KMM_ERR_MALFORMED, "kmm_map_bam: the file ends inside a record (%lld bytes behind the last complete one): "
                    "\"bgzf_tail_stop\" cut the last member after %lld inflated bytes, which is no record boundary (a share boundary "
                    "guessed by kmm_bam_find_record_start lay inside a record: map the file with one rank)",
                    (long long)(n_raw - (int64_t)co.consumed), (long long)tail_stop);
    if (c.last_chunk && co.consumed != (uint64_t)n_raw)
        return fail(KMM_ERR_MALFORMED, "kmm_map_bam: the file ends inside a record (%lld bytes behind the last complete one)",
                    (long long)(n_raw - (int64_t)co.consumed));
    ix->bam_calls++;
    ix->bam_records += (int64_t)co.recs;
    ix->bam_excluded += (int64_t)co.excluded;
    *used = (int64_t)co.consumed;
    if (bam_mates_on(ix))
        return bam_map_mates(ix, c, be, co, n_raw);
    if (bam_raw_mates_on(ix))
        return bam_map_raw_mates(ix, c, be, co, n_raw, qual);
    if (co.recs == 0)
        return KMM_OK;
    KMMCHK(ensure(ix->bam_out, (size_t)co.out_bytes + 64));
    const RqExemptCall exempting{ix};
    KMMCHK(bam_exempt_begin(ix, be, (int64_t)co.out_bytes, 0));
    KMMCHK(be.decode((n_raw + kmm_bam::TILE - 1) / kmm_bam::TILE, (uint8_t *)ix->bam_out.p));
    int64_t taken = 0, recs = 0;
    // ("record_bam", DESIGN 4.24: the inner call appends the entries and leaves the keep queue to bam_raw_keep below)
    const bool raw = ix->record_bam && ix->record_hits && ix->record_keep;
    {
        // (the quality variant's text is FASTQ: compaction and the radix path, where "min_base_quality" is applied)
        const RkCallMode mode(ix, false, raw);
        KMMCHK(kmm_map_records(ix, (const uint8_t *)ix->bam_out.p, (int64_t)co.out_bytes, qual || be.named ? KMM_FORMAT_FASTQ : KMM_FORMAT_FASTA2,
                               c.k, c.max_freq, c.also_revcomp, c.lut, &taken, &recs));
    }
    // (the raw form: a failing call appends nothing to either queue, what the inner call found is put back)
    BamWindowUndo undo{ix, co, false, ix->bam_pairs_done, raw};
    if (taken != (int64_t)co.out_bytes || recs != (int64_t)co.recs)
        return fail(KMM_ERR_INTERNAL, "kmm_map_bam: %lld of %llu decoded bytes, %lld of %llu records mapped", (long long)taken, co.out_bytes,
                    (long long)recs, co.recs);
    if (raw) {
        KMMCHK(bam_raw_keep(ix, be, co, n_raw));
        ix->rk_snap.valid = false;
    }
    undo.armed = false;
    if (c.n_records)
        *c.n_records = recs;
    return KMM_OK;
}

// ---- kmm_bam_header, kmm_bam_find_record_start: where a rank's share of a BAM file begins.  Both inflate whole
// members of the caller's window into buffers of their own (rs_*) on the handle's stream and leave its stream state alone.

// The chain of whole members at the head of comp[0, n_comp): m_off / o_off as k_inflate_bgzf takes them, p = where it ends.
struct RsChain {
    std::vector<unsigned long long> m_off{0ull}, o_off{0ull};
    uint64_t p = 0;
    uint32_t n_members() const { return (uint32_t)(m_off.size() - 1); }
};

// Walks the chain on from c.p until it holds at least out_want inflated bytes, or to the last whole member of the window (an
// incomplete one ends the chain: the caller brings it again in a longer window).
int rs_scan(const char *who, const uint8_t *comp, int64_t n_comp, unsigned long long out_want, RsChain &c)
{
    const uint64_t limit = (uint64_t)n_comp;
    while (c.o_off.back() < out_want && c.p + 18 <= limit && c.m_off.size() < 0x7FFFFFFFu) {
        const uint64_t p = c.p;
        const uint32_t ms = kmm_gz::bgzf_member_size(comp + p, limit - p);
        if (!ms) {
            const uint32_t xlen = (uint32_t)comp[p + 10] | ((uint32_t)comp[p + 11] << 8);
            if (comp[p] == 0x1f && comp[p + 1] == 0x8b && comp[p + 2] == 8 && (comp[p + 3] & 4) && p + 12 + xlen + 8 > limit)
                break; // (a header that runs past the window)
            return fail(KMM_ERR_MALFORMED, "%s: no BGZF member at compressed byte %llu of the window", who, (unsigned long long)p);
        }
        if (p + ms > limit)
            break;
        const uint32_t isize = kmm_gz::rd32(comp + p + ms - 4);
        if ((uint64_t)isize > (uint64_t)ms * 1032ull + 64ull)
            return fail(KMM_ERR_MALFORMED, "%s: member at compressed byte %llu claims %u inflated bytes for %u compressed ones", who,
                        (unsigned long long)p, isize, ms);
        c.p = p + ms;
        c.m_off.push_back(c.p);
        c.o_off.push_back(c.o_off.back() + isize);
    }
    return KMM_OK;
}

// Inflates the chain's members into rs_raw and checks their CRC32s (k_inflate_bgzf, k_crc_bgzf, as bgzf_inflate launches
// them); synchronises.  A corrupt member is KMM_ERR_MALFORMED.
int rs_inflate(kmm_index_t *ix, const char *who, const uint8_t *comp, const RsChain &c)
{
    const uint32_t n_members = c.n_members();
    KMMCHK(ensure(ix->rs_comp, (size_t)c.p + 64));
    KMMCHK(ensure(ix->rs_raw, (size_t)c.o_off.back() + 4096));
    KMMCHK(ensure(ix->rs_meta, (size_t)(n_members + 1) * 16 + 64));
    KMMCHK(ensure(ix->rs_err, 64));
    KMMCHK(ensure(ix->rs_status, (size_t)n_members + 64));
    KMMCHK(ensure_crc_tables(ix));
    const uint32_t grid_threads = ((n_members < 65536u ? n_members : 65536u) + 63u) / 64u * 64u;
    KMMCHK(ensure(ix->bgzf_tabs, (size_t)grid_threads * kmm_gz::SCRATCH_BYTES)); // (scratch of the inflater: the stream orders its users)
    uint8_t *d_comp = (uint8_t *)ix->rs_comp.p, *d_raw = (uint8_t *)ix->rs_raw.p;
    unsigned long long *d_moff = (unsigned long long *)ix->rs_meta.p, *d_ooff = d_moff + (n_members + 1);
    const unsigned int err0[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
    HIPCHK(hipMemcpyAsync(d_comp, comp, (size_t)c.p, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(d_moff, c.m_off.data(), (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(d_ooff, c.o_off.data(), (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemcpyAsync(ix->rs_err.p, err0, sizeof err0, hipMemcpyHostToDevice, ix->stream));
    HIPCHK(hipMemsetAsync(ix->rs_status.p, 0, n_members, ix->stream));
    hipLaunchKernelGGL(kmm_gz::k_inflate_bgzf, dim3(grid_threads / 64u), dim3(64), 0, ix->stream, d_comp, d_moff, d_ooff, d_raw, n_members,
                       (uint8_t *)ix->bgzf_tabs.p, (const uint32_t *)nullptr, (unsigned int *)ix->rs_err.p, (unsigned long long *)nullptr,
                       (uint8_t *)ix->rs_status.p);
    hipLaunchKernelGGL(kmm_gz::k_crc_bgzf, dim3((n_members + 63u) / 64u), dim3(256), 0, ix->stream, d_comp, d_moff, d_ooff,
                       (const uint8_t *)d_raw, n_members, (const uint32_t *)ix->bgzf_crc.p, (unsigned int *)ix->rs_err.p,
                       (const uint8_t *)ix->rs_status.p);
    HIPCHK(hipGetLastError());
    unsigned int err[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(err, ix->rs_err.p, sizeof err, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    if (err[0])
        return fail(KMM_ERR_MALFORMED, "%s: %u corrupt BGZF member(s); the first starts at compressed byte %llu of the window (inflater code %u)",
                    who, err[0], err[1] < n_members ? c.m_off[err[1]] : 0ull, err[2]);
    return KMM_OK;
}

int rs_args(kmm_index_t *ix, const char *who, const uint8_t *comp, int64_t n_comp)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    if (n_comp < 0 || (n_comp > 0 && !comp))
        return fail(KMM_ERR_INVALID_ARG, "comp NULL or n_comp negative");
    if (n_comp > 0 && is_device_ptr(comp))
        return fail(KMM_ERR_INVALID_ARG, "%s takes the compressed bytes from host memory (the member chain is read there)", who);
    HIPCHK(hipSetDevice(ix->device));
    return KMM_OK;
}
