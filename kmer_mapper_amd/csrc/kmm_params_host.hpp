// kmm_params_host.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip in front of kmm_set_param / kmm_get_param.
// The rows of the parameter table (kmm_params.hpp) that need the handle, and the functions they name: the setters with an action
// behind the store, the one guard of the record-form switches, the values derived from the handle's state, and the counters
// that live on the device (the statistics block, the tails of the keep queues, the directory of the latest radix sub-batch).
// find_param looks a name up in both halves of the table.

using kmm_params::Row;

// ---- setters with an action ----

int set_path(kmm_index *ix, const Row &row, int64_t value)
{
    if (value == 2 && !ix->rx_ok)
        return fail(KMM_ERR_INVALID_ARG, "the radix path is not available for this index (modulo %llu: needs modulo < 2^31 "
                    "and slices whose entries fit LDS)", (unsigned long long)ix->modulo);
    kmm_params::store(row, *ix, value);
    return KMM_OK;
}

int set_part_shift(kmm_index *ix, const Row &, int64_t value)
{
    const int rc = rx_reconfigure(ix, (int)value, -1, true);
    if (rc == RX_REFUSED)
        return fail(KMM_ERR_INVALID_ARG, "part_shift %lld: needs 0 <= shift <= 13, at most 512 x 512 fine partitions "
                    "and 2^shift small enough for the quotient of a 64-bit k-mer by the modulo to fit beside "
                    "the hash bits", (long long)value);
    return rc;
}

// experiments: split the current slice width's fan-out as F2 = 2^value fine partitions per coarse partition
int set_fine_bits(kmm_index *ix, const Row &, int64_t value)
{
    const int rc = value < 0 || value > 9 ? RX_REFUSED : rx_reconfigure(ix, ix->rx_geo.w, (int)value, true);
    if (rc == RX_REFUSED)
        return fail(KMM_ERR_INVALID_ARG, "fine_bits %lld: both fan-outs must stay within 512", (long long)value);
    return rc;
}

// 1 (default): pass 2 drops the k-mers of empty buckets where a coarse partition's bitmap fits LDS (the fan-out is chosen for
// it); 0: the plain pass 2
int set_radix_filter(kmm_index *ix, const Row &row, int64_t value)
{
    kmm_params::store(row, *ix, value);
    if (ix->rx_pstart) { // (the fan-out is derived anew: a forced "fine_bits" is dropped; refused: the old one stays)
        const int rc = rx_reconfigure(ix, ix->rx_geo.w, -1, false);
        if (rc != RX_REFUSED)
            KMMCHK(rc);
    }
    return KMM_OK;
}

// 1 (default): coarse partitions of 2^19 buckets are filtered with 3 bits per bucket pair keyed by bucket and quotient
// (rx_filter_slot); 0: with the bucket bitmap, as every other geometry
int set_radix_filter_slots(kmm_index *ix, const Row &row, int64_t value)
{
    kmm_params::store(row, *ix, value);
    if (ix->rx_pstart && ix->rx_ok)
        KMMCHK(rx_build_slots(ix));
    return KMM_OK;
}

// k-mer slots per sub-batch of the radix path: at most 2^32 - 2 blocks (launch_rx), at least a few blocks
int set_radix_sub_batch_kmers(kmm_index *ix, const Row &row, int64_t value)
{
    kmm_params::store(row, *ix, value);
    ix->rx_sub_cap_eff = 0;
    return KMM_OK;
}

// kmm_comm_reduce_counts: node ranges whose flush runs under the previous range's reduce (1: flush, then one reduce)
int set_comm_overlap_slices(kmm_index *ix, const Row &row, int64_t value)
{
    kmm_params::store(row, *ix, value);
    ix->flush_cuts.clear();
    return KMM_OK;
}

// per-k-mer counting mode (GpuCounter semantics, gpu_counter.py:23-37): every batch takes the radix path and the per-entry hit
// counts are kept (kmm_get_kmer_counts) besides being summed into the node counts
int set_count_kmers(kmm_index *ix, const Row &, int64_t value)
{
    if (value && !ix->rx_ok)
        return fail(KMM_ERR_INVALID_ARG, "count_kmers needs the radix path, which is not available for this index");
    KMMCHK(rx_flush(ix));
    HIPCHK(hipStreamSynchronize(ix->stream));
    if (value && !ix->rx_ecnt_acc) {
        const size_t S = ix->rx_S ? ix->rx_S : 1;
        HIPCHK(hipMalloc(ix->rx_ecnt_acc.put(), S * 4));
        HIPCHK(hipMemset(ix->rx_ecnt_acc, 0, S * 4));
    } else if (!value && ix->rx_ecnt_acc) {
        HIPCHK(ix->rx_ecnt_acc.reset());
    }
    return KMM_OK;
}

// 1 / 2: the record calls append per-record index hits (2: and windows) to the handle's queue instead of counting nodes
// (kmm_take_record_hits); 0: off, entries still pending stay takeable
int set_record_hits(kmm_index *ix, const Row &row, int64_t value)
{
    if (value != 0 && ix->rhq_pending > 0 && ix->rhq_mode != (int)value)
        return fail(KMM_ERR_INVALID_ARG, "record_hits %lld with %lld entries of mode %d pending: take them (kmm_take_record_hits) "
                    "or empty the queue (kmm_reset_counts) first", (long long)value, (long long)ix->rhq_pending, ix->rhq_mode);
    kmm_params::store(row, *ix, value);
    if (value != 0)
        ix->rhq_mode = (int)value;
    return KMM_OK;
}

// test hook of the conservation self-check: adds `value` to the device-side "gathered by pass 2" counter, as a doubly
// processed work item would; the next synchronising call must fail with KMM_ERR_INTERNAL
int set_debug_skew_p2_counter(kmm_index *ix, const Row &, int64_t value)
{
    unsigned long long v = 0;
    HIPCHK(hipMemcpy(&v, ix->stats + 2, 8, hipMemcpyDeviceToHost));
    v += (unsigned long long)value;
    HIPCHK(hipMemcpy(ix->stats + 2, &v, 8, hipMemcpyHostToDevice));
    ix->rx_unchecked = true;
    return KMM_OK;
}

// ---- the record-form switches ----
// Each changes what the record calls append — whether the hit entries come in pairs, whether the kept bytes are text or the
// records' own — so it does not move while what was appended under its other setting is pending: the row says which of the two
// queues hold it (the entries are looked at first) and what waiting mate a move drops.
enum : int {
    HELD_BY_ENTRIES = 1,  // hit entries pending (kmm_take_record_hits)
    HELD_BY_BYTES = 2,    // kept bytes pending in rkq[0] (kmm_take_kept_records, kmm_take_kept_bgzf): the true tail is the device's
    DROPS_BAM_MATE = 4,   // a mate 1 that waits under one form or pair mode is no carry of the other's
    DROPS_SAM_MATE = 8,   // ... DESIGN 4.28
};

int set_record_form(kmm_index *ix, const Row &row, int64_t value)
{
    const int was = (int)kmm_params::load(row, *ix, *ix);
    if ((int)value != was) {
        if ((row.arg & HELD_BY_ENTRIES) && ix->rhq_pending > 0)
            return fail(KMM_ERR_INVALID_ARG, "%s %lld with %lld entries pending that were appended under %s %d: take them "
                        "(kmm_take_record_hits) or empty the queue (kmm_reset_counts) first", row.name, (long long)value,
                        (long long)ix->rhq_pending, row.name, was);
        if ((row.arg & HELD_BY_BYTES) && ix->rkq[0].ctl.p) {
            KMMCHK(drain(ix));
            unsigned long long tail[2];
            KMMCHK(rkq_tail(ix->rkq[0], tail));
            if (tail[0] > 0)
                return fail(KMM_ERR_INVALID_ARG, "%s %lld with %llu kept bytes pending that were appended under %s %d: take them "
                            "(kmm_take_kept_records, kmm_take_kept_bgzf) or empty the queue (kmm_reset_counts) first", row.name,
                            (long long)value, tail[0], row.name, was);
        }
        if (row.arg & DROPS_BAM_MATE)
            ix->bam_mate_len = ix->bam_raw_mate_len = 0;
        if (row.arg & DROPS_SAM_MATE)
            sam_mates_drop(ix);
    }
    kmm_params::store(row, *ix, value);
    return KMM_OK;
}

int set_record_sam_mates(kmm_index *ix, const Row &row, int64_t value)
{
    if (value == 1 && !ix->record_sam)
        return fail(KMM_ERR_INVALID_ARG, "record_sam_mates 1 with \"record_sam\" 0: mates are kept together in the raw form of the keep, "
                    "set \"record_sam\" to 1 or 2 first (with \"record_hits\" and \"record_keep\")");
    return set_record_form(ix, row, value);
}

// ---- counters on the device ----

// One counter of the statistics block, summed over its shards, since the last kmm_get_stats(reset).  Slots 2 and 3 are the
// conservation check of the radix path: the k-mers gathered by pass 2 / probed by pass 3, both equal to the lookups pass 1
// emitted.  name: what the caller asked for ("stats_slot_<n>" may ask for a slot the block does not have).
int get_stat_slot(kmm_index *ix, int slot, const char *name, int64_t *value)
{
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix));
    std::vector<unsigned long long> st(KMM_STAT_BYTES / 8);
    HIPCHK(hipMemcpy(st.data(), ix->stats, KMM_STAT_BYTES, hipMemcpyDeviceToHost));
    if (slot < 0 || slot >= KMM_STAT_STRIDE)
        return fail(KMM_ERR_INVALID_ARG, "unknown parameter '%s'", name);
    unsigned long long t = 0;
    for (int i = 0; i < KMM_STAT_SHARDS; ++i)
        t += st[(size_t)i * KMM_STAT_STRIDE + slot];
    *value = (int64_t)t;
    return KMM_OK;
}

int get_stat(kmm_index *ix, const Row &row, int64_t *value) { return get_stat_slot(ix, row.arg, row.name, value); }

// The true tail of a queue of kept records lives on the device: behind a synchronisation, as the statistics.  arg: 2 x queue +
// (0 bytes, 1 records)
int get_keep_tail(kmm_index *ix, const Row &row, int64_t *value)
{
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix));
    unsigned long long tail[2];
    KMMCHK(rkq_tail(ix->rkq[row.arg >> 1], tail));
    *value = (int64_t)tail[row.arg & 1];
    return KMM_OK;
}

// Diagnostics of the latest radix sub-batch (both streams drained first): the k-mers its directory accounts for — by coarse
// partition (T1), by pass-1 block (last entry of every start1 row) — and its items
enum : int { RX_DIAG_T1_SUM, RX_DIAG_START1_SUM, RX_DIAG_ITEMS };

int get_rx_diag(kmm_index *ix, const Row &row, int64_t *value)
{
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipStreamSynchronize(ix->copy_stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    if (!ix->dbg_T1)
        return fail(KMM_ERR_INVALID_ARG, "no radix batch has run on this handle");
    uint64_t sum = 0;
    if (row.arg == RX_DIAG_T1_SUM) {
        std::vector<uint32_t> t(ix->dbg_F1);
        HIPCHK(hipMemcpy(t.data(), ix->dbg_T1, t.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t v : t)
            sum += v;
    } else if (row.arg == RX_DIAG_ITEMS) {
        uint32_t v = 0;
        HIPCHK(hipMemcpy(&v, ix->dbg_item_base + ix->dbg_F1, 4, hipMemcpyDeviceToHost));
        sum = v;
    } else {
        const size_t ld = (size_t)ix->dbg_F1 + 1;
        std::vector<uint16_t> r((size_t)ix->dbg_NB * ld);
        HIPCHK(hipMemcpy(r.data(), ix->dbg_start1, r.size() * 2, hipMemcpyDeviceToHost));
        for (size_t b = 0; b < ix->dbg_NB; ++b)
            sum += r[b * ld + ld - 1];
    }
    *value = (int64_t)sum;
    return KMM_OK;
}

// ---- the rows ----

// A value derived from the handle's state: the expression over `ix`, as a function of the row.
#define KMM_DERIVED(expr) [](kmm_index *ix, const Row &, int64_t *value) -> int { *value = (expr); return KMM_OK; }

constexpr Row derived(const char *name, kmm_params::GetHook f) { return Row(name).read_only().on_get(f); }
constexpr Row stat_row(const char *name, int slot) { return Row(name).read_only().on_get(get_stat, slot); }

static_assert(RK_PAIR_ANY == 0u && RK_PAIR_BOTH == 1u, "\"record_pairs_rule\" (kmm_params.hpp) takes 0 or 1");

const Row HOST_ROWS[] = {
    // path selection and the radix path's configuration; what is read back is what is in force, not what was stored
    Row("path", &KmmKnobs::path).within(0, 2).saying("path must be 0 (auto), 1 (direct) or 2 (radix)").on_set(set_path),
    Row("part_shift").on_set(set_part_shift).on_get(KMM_DERIVED(ix->rx_geo.w)),
    Row("fine_bits").write_only().on_set(set_fine_bits),
    Row("radix_filter", &KmmKnobs::rx_filter).any_non_zero().on_set(set_radix_filter)
        .on_get(KMM_DERIVED((ix->rx_ok && rx_filter_active(ix)) ? 1 : 0)),
    Row("radix_filter_slots", &KmmKnobs::rx_filter_slots).any_non_zero().on_set(set_radix_filter_slots)
        .on_get(KMM_DERIVED((ix->rx_ok && rx_slots_active(ix)) ? 1 : 0)), // 1: pass 2 filters with the slot filter
    // 1 (default): the pass-3 variants that have the fingerprint form of the probe (rx_p3_shape) run it; 0: the plain entry loop
    Row("radix_p3_fingerprints", &KmmKnobs::rx_p3_fp).any_non_zero()
        .on_get(KMM_DERIVED((ix->rx_ok && rx_p3_fp_active(ix)) ? 1 : 0)), // 1: pass 3 probes through fingerprint bytes
    Row("radix_sorted_flush", &KmmKnobs::rx_flush_sorted).any_non_zero().on_get(KMM_DERIVED((ix->rx_flush_sorted && ix->rx_norder) ? 1 : 0)),
    Row("radix_sub_batch_kmers", &KmmKnobs::rx_sub_cap).within(4 * RX_B, ((int64_t)1 << 32) - 2 * RX_B)
        .saying("radix_sub_batch_kmers outside [32768, 2^32 - 16384]").on_set(set_radix_sub_batch_kmers),
    Row("comm_overlap_slices", &KmmKnobs::comm_slices).within(1, 64).on_set(set_comm_overlap_slices),
    Row("count_kmers").on_set(set_count_kmers).on_get(KMM_DERIVED(ix->rx_ecnt_acc ? 1 : 0)),
    Row("occupancy_filter", &KmmKnobs::use_occ).any_non_zero().on_get(KMM_DERIVED((ix->use_occ && ix->occ) ? 1 : 0)),
    Row("debug_skew_p2_counter").write_only().on_set(set_debug_skew_p2_counter),
    derived("radix_available", KMM_DERIVED(ix->rx_ok ? 1 : 0)),
    derived("radix_unavailable_reason", KMM_DERIVED(ix->rx_ok ? 0 : ix->rx_why_not)), // 0 available, 1 modulo >= 2^31, 2 slices, 3 memory, 4 overlapping buckets
    derived("direct_view_resident", KMM_DERIVED(ix->buckets ? 1 : 0)),
    derived("direct_view_bytes", KMM_DERIVED((int64_t)ix->direct_bytes)),
    derived("radix_view_bytes", KMM_DERIVED(ix->rx_pstart ? (int64_t)rx_view_bytes(ix->modulo, ix->rx_S, ix->rx_norder != nullptr) : 0)),
    // entries of a slice pass 3 keeps in LDS (the rest is walked in HBM)
    derived("radix_p3_keys_in_lds", KMM_DERIVED(ix->rx_ok ? rx_p3_shape(rx_p3_variant(ix)).keys_in_lds : 0)),
    derived("radix_filter_buckets_per_bit", KMM_DERIVED((ix->rx_ok && rx_filter_active(ix)) ? (1 << ix->rx_geo.occ_shift) : 0)), // 1, 2 or 4 (0: no filter)
    // filter bits of one coarse partition in LDS (0: no filter)
    derived("radix_filter_bits_per_partition", KMM_DERIVED(!(ix->rx_ok && rx_filter_active(ix)) ? 0
                                                           : rx_slots_active(ix)                ? (int64_t)P2F_SLOT_WORDS * 32
                                                                                                : (int64_t)1 << (ix->rx_geo.w + ix->rx_geo.f2 - ix->rx_geo.occ_shift))),
    derived("n_fine_per_coarse", KMM_DERIVED(ix->rx_ok ? ix->rx_geo.F2 : 0)),
    derived("n_coarse_partitions", KMM_DERIVED(ix->rx_ok ? ix->rx_geo.F1 : 0)),
    derived("n_partitions", KMM_DERIVED(ix->rx_ok ? ix->rx_geo.PF : 0)),
    derived("bloom_filter_bytes", KMM_DERIVED((ix->use_occ && ix->occ) ? (int64_t)ix->bloom_words * 4 : 0)),
    derived("occupancy_bits_per_bucket", KMM_DERIVED((ix->use_occ && ix->occ && !ix->bloom_words) ? (1 << ix->occ_shift) : 0)),
    derived("wide_buckets", KMM_DERIVED(ix->wide ? 1 : 0)),
    derived("host_cpu_budget", KMM_DERIVED(kmm_hostpack::cpu_budget())), // cores the process may keep busy (affinity mask, cgroup quota)
    derived("bgzf_carry_bytes", KMM_DERIVED(ix->bgzf_carry_len)), // inflated bytes behind the last complete record, waiting for the next call
    Row("debug_rx_t1_sum").read_only().on_get(get_rx_diag, RX_DIAG_T1_SUM),
    Row("debug_rx_start1_sum").read_only().on_get(get_rx_diag, RX_DIAG_START1_SUM),
    Row("debug_rx_items").read_only().on_get(get_rx_diag, RX_DIAG_ITEMS),
    // the record-hits queue and the record-form switches (what each stands for: KmmKnobs).  The pair switches make the calls append even
    // counts, which the pending entries of the other setting need not be; text and raw records never share the keep queue
    Row("record_hits", &KmmKnobs::record_hits).within(0, 2).saying("record_hits takes 0 (off), 1 (hits) or 2 (hits and windows)")
        .on_set(set_record_hits),
    derived("record_hits_pending", KMM_DERIVED(ix->rhq_pending)),   // entries waiting for kmm_take_record_hits
    derived("record_hits_pending_mode", KMM_DERIVED(ix->rhq_mode)), // the mode the pending entries were appended in (2: they have windows)
    Row("record_pairs", &KmmKnobs::record_pairs).flag().on_set(set_record_form, HELD_BY_ENTRIES),
    Row("record_names_pairs", &KmmKnobs::record_names_pairs).flag().on_set(set_record_form, HELD_BY_ENTRIES),
    Row("record_bam", &KmmKnobs::record_bam).flag().on_set(set_record_form, HELD_BY_BYTES | DROPS_BAM_MATE),
    Row("record_sam", &KmmKnobs::record_sam).within(0, 2).saying("record_sam takes 0, 1 (header lines kept) or 2 (header lines dropped)")
        .on_set(set_record_form, HELD_BY_BYTES | DROPS_SAM_MATE),
    Row("record_bam_mates", &KmmKnobs::record_bam_mates).flag().on_set(set_record_form, HELD_BY_ENTRIES | HELD_BY_BYTES | DROPS_BAM_MATE),
    Row("record_sam_mates", &KmmKnobs::record_sam_mates).flag().on_set(set_record_sam_mates, HELD_BY_ENTRIES | HELD_BY_BYTES | DROPS_SAM_MATE),
    derived("record_sam_mate_waiting", KMM_DERIVED(ix->sam_mate_len > 0 ? 1 : 0)), // a selected SAM record waits for its mate
    // intervals of kmm_set_record_regions after merging (by ref_id; by name where no id was given)
    derived("record_regions", KMM_DERIVED((int64_t)(ix->sel_iv_id.empty() ? ix->sel_iv_name.size() : ix->sel_iv_id.size()))),
    Row("record_keep_pending_bytes").read_only_said().on_get(get_keep_tail, 0),
    Row("record_keep_pending_records").read_only_said().on_get(get_keep_tail, 1),
    Row("record_keep_pending_bytes_mate2").read_only_said().on_get(get_keep_tail, 2),
    Row("record_keep_pending_records_mate2").read_only_said().on_get(get_keep_tail, 3),
    // the statistics block ("stats_slot_<n>", the one prefix form, reads raw counter n: kmm_get_param)
    stat_row("radix_p2_kmers", 2),
    stat_row("radix_p3_kmers", 3),
    stat_row("radix_p2_dropped", KMM_STAT_RX_DROPPED),
    stat_row("radix_p2_multi_round_items", KMM_STAT_RX_MULTI),
    stat_row("quality_masked_bases", KMM_STAT_QUAL_MASKED),            // FASTQ bases whose quality byte was below "min_base_quality"
    stat_row("records_without_qual", KMM_STAT_REC_NO_QUAL),            // SAM / BAM records with bases and no qualities that were mapped with a floor
    stat_row("records_reversed", KMM_STAT_REC_REVERSED),               // SAM / BAM records with FLAG 0x10 and bases written in read orientation ("original_strand")
    stat_row("record_name_bytes_replaced", KMM_STAT_REC_NAME_REPLACED), // QNAME bytes outside '!' .. '~' written as '?' by the named BAM decode ("record_names")
    stat_row("debug_p3_key_reads", KMM_STAT_RX_P3_KEYS),               // 8-byte key reads of pass 3's probes; counted by -DRX_P3_FP_STATS builds only, else 0
};
#undef KMM_DERIVED

const Row *find_param(const char *name)
{
    const Row *row = kmm_params::find(kmm_params::ROWS, name);
    return row ? row : kmm_params::find(HOST_ROWS, name);
}
