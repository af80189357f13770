// kmm_sam_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside an anonymous namespace, once the stages,
// map_records_piece, map_records_radix_call, selection_of and the keep queue's helpers (rkq_reserve, keep_entries_last, rk_rule,
// RkCallMode) are defined.  Host side of the SAM front end of kmm_map_records: one piece counted, checked, written as text and
// mapped (map_sam_piece), its raw form that keeps the records' own lines (sam_raw_piece) and the pair form of that
// (sam_raw_mates_piece, SamMatesUndo).  The kernels are in kmm_sam.hpp.
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

// "The stream ends with an unpaired record" (DESIGN 4.28): a mate 1 waits when the stream's last call has nothing more for it.
int sam_unpaired_end(const char *who, int64_t n_selected)
{
    return fail(KMM_ERR_MALFORMED, "%s: \"record_sam_mates\" is 1 and the stream ends with an unpaired record: it holds %lld selected "
                "records, the last one has no mate (a selection that removes one mate of a pair is an error here; nothing of the call "
                "is appended)", who, (long long)n_selected);
}

// What a KMM_FORMAT_SAM call of the pair form has changed in the handle beyond the queues, taken back on every way out while
// `armed`: the SAM counters, the pair ordinal, and the waiting mate, which the first piece that replaces it moves to the *_call0
// buffers.  The failure's message stays.
struct SamMatesUndo {
    kmm_index_t *ix;
    bool on;
    int64_t records0, excluded0, headers0, pairs0;
    bool armed = true;

    explicit SamMatesUndo(kmm_index_t *ix_, bool on_)
        : ix(ix_), on(on_), records0(ix_->sam_records), excluded0(ix_->sam_excluded), headers0(ix_->sam_header_lines), pairs0(ix_->sam_pairs_done)
    {
        if (on)
            ix->sam_mate_saved = false;
    }
    ~SamMatesUndo()
    {
        if (!on)
            return;
        if (armed) {
            ix->sam_records = records0;
            ix->sam_excluded = excluded0;
            ix->sam_header_lines = headers0;
            ix->sam_pairs_done = pairs0;
            if (ix->sam_mate_saved) {
                std::swap(ix->sam_mate, ix->sam_mate_call0);
                std::swap(ix->sam_mate_line, ix->sam_mate_line_call0);
                ix->sam_mate_len = ix->sam_mate_len_call0;
                ix->sam_mate_line_len = ix->sam_mate_line_len_call0;
            }
        }
        ix->sam_mate_saved = false;
    }
};

// The pair form of sam_raw_piece ("record_sam_mates"): the selected records of the stream are mates 2p and 2p + 1.
// The write walk puts the piece's FASTA text BEHIND the text of the mate 1 that the piece or call before left over, and the inner
// piece call takes both in the pair form — whole pairs of entries, no text appended (rk_mates_call with rk_raw_call, as
// bam_map_raw_mates).  Then, over the spans the write walk left: the spans by entry, the mate check on the lines' own QNAME bytes,
// the pair flags (which report the odd last record), ONE read-back (strangers, the odd record), the block scan, the pair copy, the
// tail's advance.  The odd last record's text and line go to the spare buffers and become the waiting mate once nothing of the
// piece can fail any more.  A piece without a selected record leaves the waiting mate alone and still writes its header lines.
int sam_raw_mates_piece(kmm_index_t *ix, Stage &s, const uint8_t *d_raw, int64_t n_bytes, uint64_t n_tiles, dim3 gw, const kmm_sam::Totals &h,
                        bool selected, const kmm_sel::Sel &sel, int k, int max_freq, int also_revcomp, const uint8_t *lut, int64_t *n_records)
{
    using kmm_sam::RawSpan;
    const bool headers = ix->record_sam == 1;
    const uint64_t n_spans = h.recs + (headers ? h.headers : 0ull);
    if (n_spans == 0)
        return KMM_OK;
    const int64_t carry = ix->sam_mate_len, line_carry = ix->sam_mate_line_len, pairs0 = ix->sam_pairs_done;
    const uint32_t carried = carry > 0 ? 1u : 0u;
    if (carried && (line_carry < 1 || line_carry > 0x7FFFFFFFll))
        return fail(KMM_ERR_INTERNAL, "kmm_map_records: a mate 1 waits with %lld bytes of text and a line of %lld bytes", (long long)carry,
                    (long long)line_carry);
    const uint32_t carry_len = carried ? (uint32_t)line_carry : 0u;
    const int64_t n_rec = (int64_t)h.recs + carried, n_text = carry + (int64_t)h.out_bytes;
    const uint64_t n_entries = h.recs > 0 ? (uint64_t)(n_rec & ~(int64_t)1) : 0ull; // (no selected record: the waiting mate stays)
    const bool odd = h.recs > 0 && (n_rec & 1) != 0;
    kmm_index::RkQueue &q = ix->rkq[0];
    const uint64_t n_blocks = (n_spans + kmm_sam::RAW_BLOCK - 1) / kmm_sam::RAW_BLOCK;
    const uint64_t n_tblocks = (n_tiles + kmm_sam::RAW_BLOCK - 1) / kmm_sam::RAW_BLOCK;
    // (the layout of sam_raw_piece)
    const size_t off_tile = (size_t)n_spans * 16, off_kept = off_tile + (size_t)n_tiles * 8, off_blk = off_kept + (size_t)n_spans * 8,
                 off_tblk = off_blk + (size_t)n_blocks * 16, off_tot = (off_tblk + (size_t)n_tblocks * 16 + 15) & ~(size_t)15;
    KMMCHK(ensure(ix->sam_raw, off_tot + 64));
    KMMCHK(ensure(ix->sam_span_of, ((size_t)h.recs + 1) * 4 + 64));
    KMMCHK(ensure(ix->sam_mates_ctl, 64));
    KMMCHK(ensure(s.kmers, (size_t)n_bytes + (size_t)carry + 16)); // (the piece's text behind the waiting mate's)
    KMMCHK(rkq_reserve(ix, q, (int64_t)h.consumed + (int64_t)carry_len));
    uint8_t *w = (uint8_t *)ix->sam_raw.p;
    RawSpan *spans = (RawSpan *)w;
    uint32_t *tile_pre = (uint32_t *)(w + off_tile), *kept = (uint32_t *)(w + off_kept), *pre = kept + n_spans;
    uint32_t *blk_bytes = (uint32_t *)(w + off_blk), *blk_recs = blk_bytes + n_blocks, *blk_pre = blk_recs + n_blocks;
    uint32_t *tblk_recs = (uint32_t *)(w + off_tblk), *tblk_hdrs = tblk_recs + n_tblocks, *tblk_pre = tblk_hdrs + n_tblocks;
    unsigned long long *tot = (unsigned long long *)(w + off_tot);
    uint32_t *span_of = (uint32_t *)ix->sam_span_of.p;
    unsigned long long *ctl = (unsigned long long *)ix->sam_mates_ctl.p;
    const kmm_sam::Tile *tiles = (const kmm_sam::Tile *)ix->sam_tiles.p;
    const unsigned long long *base = (const unsigned long long *)ix->sam_base.p;
    uint8_t *text = (uint8_t *)s.kmers.p, *out = text + carry;
    hipStream_t cs = ix->stream;
    const uint64_t nb = (uint64_t)n_bytes;
    const kmm_sam::MatePiece mp{d_raw, h.consumed, spans, n_spans, span_of, h.recs, carried,
                                carried ? (const uint8_t *)ix->sam_mate_line.p : nullptr, carry_len};
    {
        ScopedTimer tm;
        KMMCHK(tm.begin(ix, KMM_KERNEL_SAM_RAW_MATES));
        HIPCHK(hipMemsetAsync(spans, 0, (size_t)n_spans * 16, cs));
        HIPCHK(hipMemsetAsync(span_of, 0xFF, ((size_t)h.recs + 1) * 4, cs));
        HIPCHK(hipMemsetAsync(ctl, 0xFF, 24, cs));
        hipLaunchKernelGGL(kmm_sam::k_sam_raw_tiles, dim3((unsigned)n_tblocks), dim3(1024), 0, cs, tiles, n_tiles, tile_pre, tblk_recs, tblk_hdrs);
        hipLaunchKernelGGL(kmm_sam::k_sam_raw_scan, dim3(1), dim3(1024), 0, cs, (const uint32_t *)tblk_recs, (const uint32_t *)tblk_hdrs,
                           n_tblocks, tblk_pre, (unsigned long long *)nullptr);
        KMMCHK(tm.end());
    }
    if (carried)
        HIPCHK(hipMemcpyAsync(text, ix->sam_mate.p, (size_t)carry, hipMemcpyDeviceToDevice, cs));
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
    {
        ScopedTimer tm;
        KMMCHK(tm.begin(ix, KMM_KERNEL_SAM_RAW_MATES));
        hipLaunchKernelGGL(kmm_sam::k_sam_raw_span_of, dim3((unsigned)grid_for(ix, (int64_t)((n_spans + 255) / 256), 16)), dim3(256), 0, cs,
                           (const RawSpan *)spans, n_spans, h.recs, span_of);
        if (n_entries > 0)
            hipLaunchKernelGGL(kmm_sam::k_sam_raw_pair_names, dim3((unsigned)grid_for(ix, (int64_t)((n_entries / 2 + 3) / 4), 16)), dim3(256), 0,
                               cs, mp, n_entries, ctl);
        KMMCHK(tm.end());
        HIPCHK(hipGetLastError());
    }
    int64_t taken = 0;
    if (n_entries > 0) {
        // carry + piece as two-line FASTA in the pair form: whole pairs of entries, no text appended, no name lines compared (the
        // pair ordinal that form advances is kmm_map_bam's: it is put back, this stream has its own)
        const int64_t bam_pairs0 = ix->bam_pairs_done;
        int rc;
        {
            const RkCallMode mode(ix, true, true);
            rc = map_records_piece(ix, text, n_text, KMM_FORMAT_FASTA2, k, max_freq, also_revcomp, lut, &taken, n_records);
        }
        ix->bam_pairs_done = bam_pairs0;
        KMMCHK(rc);
        if (*n_records != (int64_t)n_entries || (!odd && taken != n_text) || taken > n_text)
            return fail(KMM_ERR_INTERNAL, "SAM chunk: %lld of %lld written bytes, %lld of %lld records mapped as pairs", (long long)taken,
                        (long long)n_text, (long long)*n_records, (long long)n_rec);
    }
    KeepEntries e; // (the inner call's entries; none: the kernels read none — the entry bound comes first — and the pointers are null)
    if (!keep_entries_last(ix, n_entries, e))
        return fail(KMM_ERR_INTERNAL, "kmm_map_records: %llu entries of the SAM piece and %lld entries pending", (unsigned long long)n_entries,
                    (long long)ix->rhq_pending);
    const RkPairRule rule = rk_pair_rule(ix);
    unsigned long long *tail = (unsigned long long *)q.ctl.p;
    unsigned long long h_ctl[3] = {~0ull, ~0ull, ~0ull};
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_SAM_RAW_MATES));
    hipLaunchKernelGGL(kmm_sam::k_sam_raw_pair_flags, dim3((unsigned)n_blocks), dim3(1024), 0, cs, mp, e.hits, e.windows, n_entries, rule, kept,
                       pre, blk_bytes, blk_recs, ctl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_ctl, ctl, 24, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs));
    if (h_ctl[0] != ~0ull) {
        (void)tm.end();
        const long long p = (long long)(pairs0 + (int64_t)h_ctl[0]);
        return fail(KMM_ERR_MALFORMED, "kmm_map_records: \"record_sam_mates\" is 1 and pair %lld of the stream is none: selected records "
                    "%lld and %lld are not mates (their QNAME bytes differ): group the file by name (an aligner's own output, or "
                    "`samtools collate`) and exclude secondary and supplementary records (0x900) (nothing of the call is appended)", p,
                    2 * p, 2 * p + 1);
    }
    if (odd != (h_ctl[1] != ~0ull) || (odd && (h_ctl[1] >= h.consumed || h_ctl[2] == 0 || h_ctl[2] > h.consumed - h_ctl[1]))) {
        (void)tm.end();
        return fail(KMM_ERR_INTERNAL, "kmm_map_records: %lld selected SAM records with the waiting one, the odd last one reported at %llu "
                    "(%llu bytes)", (long long)n_rec, h_ctl[1], h_ctl[2]);
    }
    const int64_t left = odd ? n_text - taken : 0;
    if (odd) {
        // the odd last record's text (what the inner call left) and line go to the SPARE buffers, before anything is appended
        if (left <= 0) {
            (void)tm.end();
            return fail(KMM_ERR_INTERNAL, "kmm_map_records: the odd last SAM record left %lld bytes of text", (long long)left);
        }
        KMMCHK(ensure(ix->sam_mate_next, (size_t)left + 64)); // (may free and reallocate: a device-wide sync, rare)
        KMMCHK(ensure(ix->sam_mate_line_next, (size_t)h_ctl[2] + 64));
        HIPCHK(hipMemcpyAsync(ix->sam_mate_next.p, text + taken, (size_t)left, hipMemcpyDeviceToDevice, cs));
        HIPCHK(hipMemcpyAsync(ix->sam_mate_line_next.p, d_raw + h_ctl[1], (size_t)h_ctl[2], hipMemcpyDeviceToDevice, cs));
    }
    hipLaunchKernelGGL(kmm_sam::k_sam_raw_scan, dim3(1), dim3(1024), 0, cs, (const uint32_t *)blk_bytes, (const uint32_t *)blk_recs,
                       n_blocks, blk_pre, tot);
    hipLaunchKernelGGL(kmm_sam::k_sam_raw_pair_copy, dim3((unsigned)grid_for(ix, (int64_t)((n_spans + 3) / 4), 16)), dim3(256), 0, cs, mp,
                       (const uint32_t *)kept, (const uint32_t *)pre, (const uint32_t *)blk_pre, (const unsigned long long *)tail,
                       (uint8_t *)q.text.p);
    hipLaunchKernelGGL(kmm_bam::k_bam_raw_advance, dim3(1), dim3(64), 0, cs, tail, (const unsigned long long *)tot);
    KMMCHK(tm.end());
    HIPCHK(hipGetLastError());
    q.bound += (int64_t)h.consumed + (int64_t)carry_len;
    ix->sam_pairs_done = pairs0 + (int64_t)n_entries / 2;
    // the next waiting mate: nothing from here on can fail.  The one the call found goes to the *_call0 buffers first (the kernels
    // that read it are queued in front of whatever writes a buffer next); a call that fails later swaps it back.
    if (h.recs > 0) {
        if (!ix->sam_mate_saved) {
            std::swap(ix->sam_mate, ix->sam_mate_call0);
            std::swap(ix->sam_mate_line, ix->sam_mate_line_call0);
            ix->sam_mate_len_call0 = carry;
            ix->sam_mate_line_len_call0 = line_carry;
            ix->sam_mate_saved = true;
        }
        if (odd) {
            std::swap(ix->sam_mate, ix->sam_mate_next);
            std::swap(ix->sam_mate_line, ix->sam_mate_line_next);
        }
        ix->sam_mate_len = left;
        ix->sam_mate_line_len = odd ? (int64_t)h_ctl[2] : 0;
    }
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
        } else if (sam_raw_mates_on(ix)) {
            rc = sam_raw_mates_piece(ix, s, d_raw, n_bytes, n_tiles, gw, h, selected, sel, k, max_freq, also_revcomp, lut, n_records);
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
