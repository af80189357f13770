// kmm_sam_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside an anonymous namespace, once the stages,
// map_records_piece, map_records_radix_call, selection_of and the keep queue's helpers (rkq_reserve, keep_entries_last, rk_rule,
// RkCallMode) are defined.  Host side of the SAM front end of kmm_map_records: one piece counted, checked, written as text and
// mapped (map_sam_piece), and its raw form that keeps the records' own lines (sam_raw_piece).  The kernels are in kmm_sam.hpp.
#pragma once

// The raw form of one counted and checked SAM piece ("record_sam"), in place of map_sam_piece's plain write and map:
// the write walk also leaves one span per selected record (and, with 1, per header line); the inner piece call appends the records'
// entries and none of their FASTA text; the keep step then asks the rule of every span's entry and copies the kept lines behind
// the queue's tail (both prefixes — the tiles' records and header lines, the spans' kept bytes — are two-level scans over blocks of
// 1024).  No walk over the lines beyond the one write; no read-back: the queue holds room for the piece's consumed
// bytes before anything is launched.  A piece of header lines alone is served too.  The caller's kmm_map_records puts both queues
// back when anything here fails.
int sam_raw_piece(kmm_index_t *ix, Stage &s, const uint8_t *d_raw, int64_t n_bytes, uint64_t n_tiles, dim3 gw, const kmm_sam::Totals &h,
                  bool selected, const kmm_sel::Sel &sel, int k, int max_freq, int also_revcomp, const uint8_t *lut, int64_t *n_records)
{
    using kmm_sam::RawSpan;
    static_assert(sizeof(RawSpan) == 16, "a span is one 16-byte store");
    const bool headers = ix->record_sam == 1;
    const uint64_t n_spans = h.recs + (headers ? h.headers : 0ull);
    if (n_spans == 0)
        return KMM_OK;
    kmm_index::RkQueue &q = ix->rkq[0];
    const uint64_t n_blocks = (n_spans + kmm_sam::RAW_BLOCK - 1) / kmm_sam::RAW_BLOCK;    // of spans (k_sam_raw_flags)
    const uint64_t n_tblocks = (n_tiles + kmm_sam::RAW_BLOCK - 1) / kmm_sam::RAW_BLOCK;   // of tiles (k_sam_raw_tiles)
    // spans | tile_pre (2 per tile) | kept, pre (1 per span) | per block of spans, then per block of tiles: sums (2), bases (2) | totals
    const size_t off_tile = (size_t)n_spans * 16, off_kept = off_tile + (size_t)n_tiles * 8, off_blk = off_kept + (size_t)n_spans * 8,
                 off_tblk = off_blk + (size_t)n_blocks * 16, off_tot = (off_tblk + (size_t)n_tblocks * 16 + 15) & ~(size_t)15;
    KMMCHK(ensure(ix->sam_raw, off_tot + 64));
    KMMCHK(rkq_reserve(ix, q, (int64_t)h.consumed));
    uint8_t *w = (uint8_t *)ix->sam_raw.p;
    RawSpan *spans = (RawSpan *)w;
    uint32_t *tile_pre = (uint32_t *)(w + off_tile), *kept = (uint32_t *)(w + off_kept), *pre = kept + n_spans;
    uint32_t *blk_bytes = (uint32_t *)(w + off_blk), *blk_recs = blk_bytes + n_blocks, *blk_pre = blk_recs + n_blocks;
    uint32_t *tblk_recs = (uint32_t *)(w + off_tblk), *tblk_hdrs = tblk_recs + n_tblocks, *tblk_pre = tblk_hdrs + n_tblocks;
    unsigned long long *tot = (unsigned long long *)(w + off_tot); // the kept bytes and the kept records of the piece
    const kmm_sam::Tile *tiles = (const kmm_sam::Tile *)ix->sam_tiles.p;
    const unsigned long long *base = (const unsigned long long *)ix->sam_base.p;
    uint8_t *out = (uint8_t *)s.kmers.p;
    hipStream_t cs = ix->stream;
    const uint64_t nb = (uint64_t)n_bytes;
    {
        ScopedTimer tm;
        KMMCHK(tm.begin(ix, KMM_KERNEL_SAM_RAW));
        HIPCHK(hipMemsetAsync(spans, 0, (size_t)n_spans * 16, cs)); // (a slot no walk fills has length 0: it is never copied)
        hipLaunchKernelGGL(kmm_sam::k_sam_raw_tiles, dim3((unsigned)n_tblocks), dim3(1024), 0, cs, tiles, n_tiles, tile_pre, tblk_recs, tblk_hdrs);
        hipLaunchKernelGGL(kmm_sam::k_sam_raw_scan, dim3(1), dim3(1024), 0, cs, (const uint32_t *)tblk_recs, (const uint32_t *)tblk_hdrs,
                           n_tblocks, tblk_pre, (unsigned long long *)nullptr);
        KMMCHK(tm.end());
    }
    const uint32_t hd = headers ? 1u : 0u;
    if (selected && ix->original_strand)
        hipLaunchKernelGGL(kmm_sam::k_sam_write_spans_rev_sel, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, sel, tiles, base, out,
                           ix->stats + KMM_STAT_REC_REVERSED, (const uint32_t *)tile_pre, (const uint32_t *)tblk_pre, hd, spans, n_spans);
    else if (selected)
        hipLaunchKernelGGL(kmm_sam::k_sam_write_spans_sel, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, sel, tiles, base, out,
                           (const uint32_t *)tile_pre, (const uint32_t *)tblk_pre, hd, spans, n_spans);
    else if (ix->original_strand)
        hipLaunchKernelGGL(kmm_sam::k_sam_write_spans_rev, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, (uint32_t)ix->bam_excl, tiles, base, out,
                           ix->stats + KMM_STAT_REC_REVERSED, (const uint32_t *)tile_pre, (const uint32_t *)tblk_pre, hd, spans, n_spans);
    else
        hipLaunchKernelGGL(kmm_sam::k_sam_write_spans, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, (uint32_t)ix->bam_excl, tiles, base, out,
                           (const uint32_t *)tile_pre, (const uint32_t *)tblk_pre, hd, spans, n_spans);
    HIPCHK(hipGetLastError());
    if (h.recs > 0) {
        // the records as two-line FASTA, as without the raw form; the inner call appends the entries and leaves the keep queue alone
        int64_t used = 0;
        const RkCallMode mode(ix, false, true);
        KMMCHK(map_records_piece(ix, out, (int64_t)h.out_bytes, KMM_FORMAT_FASTA2, k, max_freq, also_revcomp, lut, &used, n_records));
        if (used != (int64_t)h.out_bytes || *n_records != (int64_t)h.recs)
            return fail(KMM_ERR_INTERNAL, "SAM chunk: %lld of %llu written bytes, %lld of %llu records mapped", (long long)used, h.out_bytes,
                        (long long)*n_records, h.recs);
    }
    KeepEntries e; // (the inner call's entries)
    if (!keep_entries_last(ix, h.recs, e))
        return fail(KMM_ERR_INTERNAL, "kmm_map_records: %llu selected SAM records and %lld entries pending", h.recs, (long long)ix->rhq_pending);
    const RkRule rule = rk_rule(ix);
    unsigned long long *tail = (unsigned long long *)q.ctl.p;
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_SAM_RAW));
    hipLaunchKernelGGL(kmm_sam::k_sam_raw_flags, dim3((unsigned)n_blocks), dim3(1024), 0, cs, (const RawSpan *)spans, n_spans, h.consumed, e.hits,
                       e.windows, e.n, rule, kept, pre, blk_bytes, blk_recs);
    hipLaunchKernelGGL(kmm_sam::k_sam_raw_scan, dim3(1), dim3(1024), 0, cs, (const uint32_t *)blk_bytes, (const uint32_t *)blk_recs,
                       n_blocks, blk_pre, tot);
    hipLaunchKernelGGL(kmm_sam::k_sam_raw_copy, dim3((unsigned)grid_for(ix, (int64_t)((n_spans + 3) / 4), 16)), dim3(256), 0, cs, d_raw,
                       (const RawSpan *)spans, n_spans, (const uint32_t *)kept, (const uint32_t *)pre, (const uint32_t *)blk_pre,
                       (const unsigned long long *)tail, (uint8_t *)q.text.p);
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_advance, dim3(1), dim3(64), 0, cs, tail, (const unsigned long long *)tot);
    KMMCHK(tm.end());
    HIPCHK(hipGetLastError());
    q.bound += (int64_t)h.consumed;
    return KMM_OK;
}

// One piece of a SAM chunk (kmm_sam.hpp): its lines counted and checked on the device, the SEQ of every kept record written as
// two-line FASTA into the stage's second buffer, which map_records_piece then maps.  Only complete lines are taken (*consumed:
// the byte after the piece's last newline).  dry: the count and the checks only (a chunk of several pieces is checked whole
// before any of it is mapped).  at: the piece's offset in the caller's chunk (for the error message).
int map_sam_piece(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int64_t at, bool dry, int k, int max_freq, int also_revcomp,
                  const uint8_t *lut, int64_t *consumed, int64_t *n_records)
{
    *consumed = 0;
    *n_records = 0;
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    bool staged = false;
    const uint8_t *d_raw = nullptr;
    KMMCHK(stage_in<uint8_t>(ix, s.bases, raw, (size_t)n_bytes, &d_raw, &staged));
    const uint64_t n_tiles = ((uint64_t)n_bytes + kmm_sam::TILE - 1) / kmm_sam::TILE;
    KMMCHK(ensure(ix->sam_tiles, (size_t)n_tiles * sizeof(kmm_sam::Tile) + 64));
    KMMCHK(ensure(ix->sam_base, (size_t)n_tiles * 8 + 64));
    KMMCHK(ensure(ix->sam_ctl, 256));
    const bool qual = record_quality(ix) > 0; // the quality variant: four-line FASTQ, mapped with the floor
    if (!dry && !qual)
        KMMCHK(ensure(s.kmers, (size_t)n_bytes + 16)); // (a record's output is never longer than its line)
    kmm_sam::Tile *tiles = (kmm_sam::Tile *)ix->sam_tiles.p;
    unsigned long long *base = (unsigned long long *)ix->sam_base.p;
    kmm_sam::Totals *d_tot = (kmm_sam::Totals *)ix->sam_ctl.p;
    const uint32_t excl = ix->bam_excl;
    kmm_sel::Sel sel; // a selection beyond excl: the k_sam_*_sel kernels run
    const int src = selection_of(ix, "kmm_map_records (KMM_FORMAT_SAM)", true, 0, sel);
    if (src != KMM_OK) {
        (void)stage_release(ix, s, false);
        return src;
    }
    const bool selected = !sel.flags_only();
    KMMCHK(stage_copies_done(ix));
    hipStream_t cs = ix->stream; // (kernels run on the handle's stream only: see rec_compact_piece)
    const dim3 gw((unsigned)grid_for(ix, (int64_t)((n_tiles + 3) / 4), 16)); // one wavefront per tile, 4 per block, grid-stride
    if (selected && qual)
        hipLaunchKernelGGL(kmm_sam::k_sam_count_q_sel, gw, dim3(256), 0, cs, d_raw, (uint64_t)n_bytes, n_tiles, sel, tiles);
    else if (selected)
        hipLaunchKernelGGL(kmm_sam::k_sam_count_sel, gw, dim3(256), 0, cs, d_raw, (uint64_t)n_bytes, n_tiles, sel, tiles);
    else if (qual)
        hipLaunchKernelGGL(kmm_sam::k_sam_count_q, gw, dim3(256), 0, cs, d_raw, (uint64_t)n_bytes, n_tiles, excl, tiles);
    else
        hipLaunchKernelGGL(kmm_sam::k_sam_count, gw, dim3(256), 0, cs, d_raw, (uint64_t)n_bytes, n_tiles, excl, tiles);
    hipLaunchKernelGGL(kmm_sam::k_sam_totals, dim3(1), dim3(1024), 0, cs, (const kmm_sam::Tile *)tiles, n_tiles, base, d_tot);
    HIPCHK(hipGetLastError());
    kmm_sam::Totals h;
    HIPCHK(hipMemcpyAsync(&h, d_tot, sizeof h, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs)); // (the borrowed host buffer is free from here on)
    if (h.err != kmm_sam::NONE) {
        static const char *why[8] = {"QUAL is not \"*\" and not as long as SEQ", "fewer than 11 TAB-separated fields",
                                     "FLAG is not a decimal integer in [0, 65535]", "an empty line",
                                     "MAPQ is not a decimal integer in [0, 255] (\"bam_min_mapq\" reads it)",
                                     "POS is not a decimal integer in [0, 2^31 - 1] (the region list reads it)",
                                     "CIGAR is neither \"*\" nor ([0-9]+[MIDNSHP=X])+ with lengths up to 2^28 - 1 (the region list reads it)",
                                     "?"};
        const unsigned shift = selected ? 3u : 2u; // (kmm_sam::err_shift)
        (void)stage_release(ix, s, false);
        return fail(KMM_ERR_MALFORMED, "kmm_map_records: SAM line at byte %llu of the chunk: %s (nothing of the call is mapped)",
                    (unsigned long long)at + (h.err >> shift), why[h.err & ((1u << shift) - 1u)]);
    }
    *consumed = (int64_t)h.consumed;
    const uint64_t nb = (uint64_t)n_bytes;
    int rc = KMM_OK;
    if (!dry) {
        ix->sam_records += (int64_t)h.recs;
        ix->sam_excluded += (int64_t)h.excluded;
        ix->sam_header_lines += (int64_t)h.headers;
        if (h.recs > 0 && qual) {
            // (with QUAL "*" a record's four-line FASTQ is longer than its line: the buffer is sized from the totals)
            rc = ensure(s.kmers, (size_t)h.out_bytes + 16);
            if (rc == KMM_OK) {
                uint8_t *out = (uint8_t *)s.kmers.p;
                unsigned long long *no_qual = ix->stats + KMM_STAT_REC_NO_QUAL;
                if (selected && ix->original_strand)
                    hipLaunchKernelGGL(kmm_sam::k_sam_write_q_rev_sel, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, sel, tiles, base, out, no_qual,
                                       ix->stats + KMM_STAT_REC_REVERSED);
                else if (selected)
                    hipLaunchKernelGGL(kmm_sam::k_sam_write_q_sel, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, sel, tiles, base, out, no_qual);
                else if (ix->original_strand)
                    hipLaunchKernelGGL(kmm_sam::k_sam_write_q_rev, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, excl, tiles, base, out, no_qual,
                                       ix->stats + KMM_STAT_REC_REVERSED);
                else
                    hipLaunchKernelGGL(kmm_sam::k_sam_write_q, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, excl, tiles, base, out, no_qual);
                const hipError_t e = hipGetLastError();
                if (e != hipSuccess)
                    rc = fail(KMM_ERR_HIP, "kmm_map_records: k_sam_write_q: %s", hipGetErrorString(e));
            }
            // the records as FASTQ, from HBM, through compaction and the radix path, where the floor is applied — in the
            // record-hits mode through the direct records route, piece by piece, under that mode's floor
            int64_t used = 0;
            if (rc == KMM_OK && ix->record_hits)
                rc = map_records_entry(ix, (const uint8_t *)s.kmers.p, (int64_t)h.out_bytes, KMM_FORMAT_FASTQ, k, max_freq, also_revcomp, lut,
                                       &used, n_records);
            else if (rc == KMM_OK)
                rc = map_records_radix_call(ix, (const uint8_t *)s.kmers.p, (int64_t)h.out_bytes, KMM_FORMAT_FASTQ, k, max_freq,
                                            also_revcomp, lut, &used, n_records);
            if (rc == KMM_OK && (used != (int64_t)h.out_bytes || *n_records != (int64_t)h.recs))
                rc = fail(KMM_ERR_INTERNAL, "SAM chunk: %lld of %llu written bytes, %lld of %llu records mapped", (long long)used,
                          h.out_bytes, (long long)*n_records, h.recs);
        } else if (sam_raw_on(ix)) {
            rc = sam_raw_piece(ix, s, d_raw, n_bytes, n_tiles, gw, h, selected, sel, k, max_freq, also_revcomp, lut, n_records);
        } else if (h.recs > 0) {
            uint8_t *out = (uint8_t *)s.kmers.p;
            unsigned long long *reversed = ix->stats + KMM_STAT_REC_REVERSED;
            if (selected && ix->original_strand)
                hipLaunchKernelGGL(kmm_sam::k_sam_write_rev_sel, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, sel, tiles, base, out, reversed);
            else if (selected)
                hipLaunchKernelGGL(kmm_sam::k_sam_write_sel, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, sel, tiles, base, out);
            else if (ix->original_strand)
                hipLaunchKernelGGL(kmm_sam::k_sam_write_rev, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, excl, tiles, base, out, reversed);
            else
                hipLaunchKernelGGL(kmm_sam::k_sam_write, gw, dim3(256), 0, cs, d_raw, nb, n_tiles, excl, tiles, base, out);
            HIPCHK(hipGetLastError());
            // the records as two-line FASTA, from HBM, through the two-line parser (its kernels wait for the copy stream)
            int64_t used = 0;
            rc = map_records_piece(ix, out, (int64_t)h.out_bytes, KMM_FORMAT_FASTA2, k, max_freq, also_revcomp, lut, &used, n_records);
            if (rc == KMM_OK && (used != (int64_t)h.out_bytes || *n_records != (int64_t)h.recs))
                rc = fail(KMM_ERR_INTERNAL, "SAM chunk: %lld of %llu written bytes, %lld of %llu records mapped", (long long)used,
                          h.out_bytes, (long long)*n_records, h.recs);
        }
    }
    const int rel = stage_release(ix, s, false); // (after the inner call's kernels: they read this stage's buffer)
    return rc != KMM_OK ? rc : rel;
}
