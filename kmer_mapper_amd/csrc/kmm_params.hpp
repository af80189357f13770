// kmm_params.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip.
// The parameters of kmm_set_param / kmm_get_param (include/kmm.h), each stated once: the fields that are nothing but a stored
// parameter value (KmmKnobs) and the host-side counters that are only read (KmmCounters) — both bases of kmm_index, so the
// fields keep their names in the handle — and one row per name (Row): the field it stores to or loads from, who may set and who
// may read it, the values it takes, the text of the refusal and how an accepted value is stored.  ROWS holds the rows that need
// nothing but the two structs; the rows that need the handle (an action behind the store, a derived value, a counter on the
// device) are of the same type and live in kmm_params_host.hpp.  Standard C++17: no HIP header, no kmm_index —
// tests/test_params_on_the_cpu.py compiles it by itself with g++ and replays tests/golden/param_contract.json on it.
//
// A new plain parameter is one field and one row.  The messages are behaviour (tests match on them, the CLI prints them):
// "%s takes 0 or 1" and "%s outside [lo, hi]" with decimal bounds are made from the row, every other wording rides in it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "kmm_radix_plan.hpp" // RX_SUB_CAP_MAX, P2F_SLOTS: two defaults

struct kmm_index; // (the rows of kmm_params_host.hpp name functions over the handle)

// The fields that are a stored parameter value and nothing else; the name in quotes is the parameter's.
struct KmmKnobs {
    bool use_occ = true;                 // "occupancy_filter"
    bool dynamic_schedule = true;
    int dyn_chunk = 16;                  // tiles per grab
    // path selection / radix path (kmm_radix.hpp)
    int path = 0;         // 0 auto, 1 direct, 2 radix
    int grid_per_cu = 64; // upper bound on workgroups per CU of the grid-stride fused kernel
    bool rx_flush_sorted = true; // "radix_sorted_flush": use the node-ordered entry list for the flush
    int rx_grid_per_cu = 2;   // persistent workgroups of passes 2 and 3 per CU (1: leave room for another stream's kernels)
    int64_t rx_min_units = 0; // auto: batches of at least this many positions / k-mers take the radix path
    int64_t rx_sub_cap = RX_SUB_CAP_MAX; // k-mer slots per sub-batch of the radix path ("radix_sub_batch_kmers")
    bool rx_filter = true;        // "radix_filter": use the filtering pass 2 whenever a coarse partition's bitmap fits LDS
    bool rx_filter_slots = true;  // "radix_filter_slots": where the geometry allows it the filter is the slot filter (0: the bucket bitmap)
    bool rx_p3_fp = true;         // "radix_p3_fingerprints": pass 3 probes through fingerprint bytes where its variant has that form
    uint32_t dbg_p2f_cap = P2F_SLOTS; // test hook ("debug_p2f_round_slots"): sort-buffer slots k_rx_p2f uses beside the slot filter
    bool rx_packed = true;        // "radix_packed_tiles": pass 1 on reads of one length takes tiles of whole reads
    int64_t dbg_rx_buf_limit = 0; // test hook ("debug_rx_buffer_limit"): a pass-1 buffer beyond this many bytes counts as out of memory
    int comm_slices = 8;          // "comm_overlap_slices": flush of node range s under the reduce of node range s - 1 (kmm_comm_reduce_counts)
    int host_pack_threads = 0;     // "host_pack_threads": reads / raw records in host memory are packed to 2 bits per base by that
                                   // many host threads before they cross PCIe (default: min(16, the process's CPU budget))
    int64_t host_pack_slice_kb = 0; // "host_pack_slice_kb": raw bytes per slice of the records packer (0: its default)
    int64_t bgzf_head_skip = 0;  // "bgzf_head_skip": inflated bytes of the next NEW_STREAM call's first member that belong to someone else
    int64_t bgzf_tail_stop = -1; // "bgzf_tail_stop": >= 0: of the next LAST_CHUNK call's last member only this many inflated bytes are taken
    int dbg_bgzf_slot_kb = 0;     // test hook ("debug_bgzf_ring_slot_kb"): slot size of kmm_map_bgzf's staging ring (a power of two, >= 4)
    int64_t dbg_bgzf_call_cap_kb = 0; // test hook ("debug_bgzf_call_cap_kb"): inflated bytes a kmm_map_bgzf / kmm_map_bam call
                                      // takes at most, KiB (0: 3.5 GiB)
    int dbg_gzip_chunk_kb = 0;    // test hook ("debug_gzip_chunk_kb"): spacing of the chunk search, KiB (0: 32)
    uint32_t bam_excl = 0;        // "bam_exclude_flags": records with flag & mask are not mapped (samtools view -F)
    uint32_t bam_incl = 0, bam_min_mapq = 0; // record selection (kmm_select.hpp): "bam_include_flags", "bam_min_mapq"
    int64_t bam_n_ref_param = -1;     // "bam_n_ref": n_ref of a KMM_FORMAT_MID_STREAM stream (-1: not set)
    int64_t dbg_bam_resync_kb = 0;    // test hook ("debug_bam_resync_kb"): inflated bytes kmm_bam_find_record_start examines at most, KiB (0: all)
    int dbg_rec_copy_stream = 0; // experiments (tools/records_overlap_bisect.py): compaction kernels on the copy stream again, beside the
                                 // previous call's passes, WITHOUT mapping the call's reads
    int dbg_rec_skip = 0;        // and which of them to leave out (1 count2, 2 scans, 4 scatter, 8 uniform, 16 the large memsets)
    int64_t dbg_rec_piece_kb = 0; // test hook ("debug_records_piece_kb"): bytes per piece of kmm_map_records, KiB (0: 2^30 bytes)
    int dbg_rec_grid = 0;         // test hook ("debug_records_grid"): workgroups of the compaction's per-tile kernels (0: grid_for)
    int min_base_quality = 0;    // "min_base_quality": > 0: a FASTQ base whose quality byte is below 33 + this is a break (flat reads: 4.11)
    // "record_hits_min_base_quality": the floor of the record calls while "record_hits" is 1 or 2 — a parameter of
    // its own: "min_base_quality" with the mode on stays refused.  Entries may be pending: an entry holds what its record had under the
    // floor of its own call
    int rh_min_base_quality = 0;
    int use_record_qual = 0;     // "use_record_qual": 1: with a floor set, SAM / BAM records are mapped with their QUAL
    int original_strand = 0;     // "original_strand": 1: kept SAM / BAM records with FLAG 0x10 are mapped in read orientation
    // the record-hits mode: while "record_hits" is 1 or 2 the record calls append one entry per record to the handle's
    // queue instead of counting nodes
    int record_hits = 0;
    // the record-keep mode: with "record_keep" 1 the record calls also append the text of every record whose entry
    // passes the keep rule ("record_keep_min_hits", "record_keep_min_permille", "record_keep_invert") to rkq[0]
    int record_keep = 0, rk_invert = 0, rk_min_permille = 0;
    int64_t rk_min_hits = 1;
    // the named form of the BAM decode: with "record_names" 1 kmm_map_bam, in the record-hits mode, decodes the selected
    // records into four-line FASTQ that carries QNAME and QUAL (k_bam_*_named) — the text "record_keep" appends;
    // "record_names_mate_suffix" 1: "/1" / "/2" behind the name
    int record_names = 0, record_names_mate_suffix = 0;
    // keeping mates together: "record_pairs" 1: the records of a stream are interleaved, 2i and 2i + 1 are mates,
    // and the keep rule is rk_pair_keep over their two entries ("record_pairs_rule": RK_PAIR_ANY / RK_PAIR_BOTH); both are read
    // only while "record_keep" is 1
    int record_pairs = 0, rk_pair_rule = 0;
    // the mates of a name-collated BAM file: "record_names_pairs" 1: the selected records of a kmm_map_bam stream
    // are mates in file order, 2p and 2p + 1
    int record_names_pairs = 0;
    // the raw form: "record_bam" 1: kmm_map_bam with "record_hits" and "record_keep" maps the selected records in the
    // two-line FASTA form and appends the kept records' own bytes (block_size word and all) to rkq[0]
    int record_bam = 0;
    // mates kept together in the raw form: "record_bam_mates" 1: the selected records of a kmm_map_bam stream are mates
    // in file order and their own bytes are kept or dropped together
    int record_bam_mates = 0;
    // SAM lines kept as SAM lines: "record_sam" 1 / 2: a KMM_FORMAT_SAM call with "record_hits" and "record_keep" maps
    // the selected records in the two-line FASTA form and appends the kept records' own lines to rkq[0]; 1: the header lines as well
    int record_sam = 0;
    // mates kept together in SAM output: "record_sam_mates" 1: the selected records of a SAM stream are mates in file
    // order and their lines are kept or dropped together
    int record_sam_mates = 0;
};

// The host-side counters that are only read; each is the parameter of (nearly) the same name.
struct KmmCounters {
    int64_t host_packed_calls = 0;        // map calls whose flat reads crossed PCIe as 2-bit codes
    int64_t host_packed_record_calls = 0; // kmm_map_records calls whose sequence lines were packed on the host
    int64_t bgzf_prestaged_calls = 0;     // kmm_map_bgzf calls that staged the chunk behind them under their own kernel
    int64_t bgzf_members = 0;             // BGZF members inflated on the GPU by kmm_map_bgzf
    int64_t gzip_calls = 0;               // kmm_map_gzip calls
    int64_t gzip_members = 0;             // gzip members whose CRC32 / ISIZE kmm_map_gzip checked
    int64_t gzip_chunks = 0;              // speculative starts decoded by kmm_map_gzip (the first chunk of every call included)
    int64_t gzip_false_starts = 0;        // starts rejected by the predecessor check
    int64_t gzip_continuations = 0;       // lanes re-run past a rejected start or a full output slot
    int64_t gzip_inflated = 0;            // "gzip_inflated_bytes": bytes kmm_map_gzip inflated (callers size their next window from it)
    int64_t bam_calls = 0;                // kmm_map_bam calls that mapped their records (a window inside the header not counted)
    int64_t bam_records = 0;              // BAM records mapped
    int64_t bam_excluded = 0;             // "bam_records_excluded": BAM records left out by "bam_exclude_flags"
    int64_t bam_header_bytes = 0;         // inflated bytes of the BAM headers read
    int64_t bam_false_starts = 0;         // speculative record starts found wrong by the link check
    int64_t bam_continuations = 0;        // tiles walked again from the exit before them
    int64_t sam_calls = 0;                // kmm_map_records calls (direct, or on the inflated bytes of kmm_map_bgzf / _gzip) on SAM
    int64_t sam_records = 0;              // SAM records mapped
    int64_t sam_excluded = 0;             // "sam_records_excluded": SAM records left out by "bam_exclude_flags"
    int64_t sam_header_lines = 0;         // SAM lines starting with '@', skipped
    int64_t flat_uniform_batches = 0;     // flat reads of one length mapped by the uniform / packed front ends of the radix path (rec_launch_flat)
    int64_t read_hits_calls = 0;          // kmm_read_hits calls that were accepted (a pure query: no other counter moves)
    int64_t rx_sub_cap_last = 0;          // "radix_sub_batch_kmers_effective": the size the last radix call ran with
    int64_t comm_sliced_reduces = 0;      // kmm_comm_reduce_counts calls that issued one reduce per node range
    uint64_t n_radix_batches = 0, n_direct_batches = 0; // which path the batches took ("radix_batches" / "direct_batches")
};

namespace kmm_params {

// The field of a row, with its width.
struct Member {
    enum Type : uint8_t { NONE, KNOB_BOOL, KNOB_INT, KNOB_U32, KNOB_I64, COUNTER_I64, COUNTER_U64 } type = NONE;
    union {
        bool KmmKnobs::*kb;
        int KmmKnobs::*ki;
        uint32_t KmmKnobs::*ku;
        int64_t KmmKnobs::*kl;
        int64_t KmmCounters::*cl;
        uint64_t KmmCounters::*cu;
    };
    constexpr Member() : kb(nullptr) {}
    constexpr Member(bool KmmKnobs::*p) : type(KNOB_BOOL), kb(p) {}
    constexpr Member(int KmmKnobs::*p) : type(KNOB_INT), ki(p) {}
    constexpr Member(uint32_t KmmKnobs::*p) : type(KNOB_U32), ku(p) {}
    constexpr Member(int64_t KmmKnobs::*p) : type(KNOB_I64), kl(p) {}
    constexpr Member(int64_t KmmCounters::*p) : type(COUNTER_I64), cl(p) {}
    constexpr Member(uint64_t KmmCounters::*p) : type(COUNTER_U64), cu(p) {}
};

enum Access : uint8_t {
    READ_WRITE,
    WRITE_ONLY,     // a get does not know the name
    READ_ONLY,      // a set does not know the name
    READ_ONLY_SAID, // a set answers "%s is read-only"
};
enum Accept : uint8_t { ANY_VALUE, ZERO_OR_ONE, RANGE };
enum Store : uint8_t {
    AS_GIVEN,               // converted to the field's type
    NON_ZERO,               // value != 0: the switch takes ANY non-zero value for "on" and has no refusal
    NEGATIVE_AS_MINUS_ONE,  // "bgzf_tail_stop": every negative value means "not set"
};

struct Row;
using SetHook = int (*)(kmm_index *, const Row &, int64_t value);  // behind the checks of the row; the store is the hook's
using GetHook = int (*)(kmm_index *, const Row &, int64_t *value);

struct Row {
    const char *name = nullptr, *alias = nullptr;
    Member at;
    Access access = READ_WRITE;
    Accept accept = ANY_VALUE;
    int64_t lo = 0, hi = 0;            // RANGE
    bool (*also)(int64_t) = nullptr;   // a rule beyond the range (even, a power of two)
    const char *refusal = nullptr;     // the text of the refusal where it is not one of the two made from the row
    Store store = AS_GIVEN;
    bool no_sync = false;              // kmm_set_param does not synchronise the stream first (the "debug_records_*" switches of the
                                       // overlap experiment are set between two calls in flight)
    SetHook set = nullptr;             // kmm_params_host.hpp
    GetHook get = nullptr;
    int arg = 0;                       // what the hook's rows differ in (a statistics slot, a queue, the guards of a switch)

    constexpr Row(const char *n, Member m = Member()) : name(n), at(m) {}
    constexpr Row flag() const { Row r = *this; r.accept = ZERO_OR_ONE; return r; }
    constexpr Row within(int64_t l, int64_t h) const { Row r = *this; r.accept = RANGE; r.lo = l; r.hi = h; return r; }
    constexpr Row and_is(bool (*rule)(int64_t)) const { Row r = *this; r.also = rule; return r; }
    constexpr Row saying(const char *text) const { Row r = *this; r.refusal = text; return r; }
    constexpr Row any_non_zero() const { Row r = *this; r.store = NON_ZERO; return r; }
    constexpr Row negative_as_minus_one() const { Row r = *this; r.store = NEGATIVE_AS_MINUS_ONE; return r; }
    constexpr Row aka(const char *other) const { Row r = *this; r.alias = other; return r; }
    constexpr Row write_only() const { Row r = *this; r.access = WRITE_ONLY; return r; }
    constexpr Row read_only() const { Row r = *this; r.access = READ_ONLY; return r; }
    constexpr Row read_only_said() const { Row r = *this; r.access = READ_ONLY_SAID; return r; }
    constexpr Row unsynchronised() const { Row r = *this; r.no_sync = true; return r; }
    constexpr Row on_set(SetHook f, int a = 0) const { Row r = *this; r.set = f; r.arg = a; return r; }
    constexpr Row on_get(GetHook f, int a = 0) const { Row r = *this; r.get = f; r.arg = a; return r; }
};
constexpr Row counter(const char *name, Member m) { return Row(name, m).read_only(); }

constexpr bool even(int64_t v) { return (v & 1) == 0; }
constexpr bool zero_or_a_power_of_two_from_4(int64_t v) { return v == 0 || (v >= 4 && (v & (v - 1)) == 0); }
static_assert(P2F_SLOTS == 5888 && RX_B == 8192, "the bounds spelled out in the texts of debug_p2f_round_slots and radix_sub_batch_kmers");

// The rows that need nothing but KmmKnobs and KmmCounters.
constexpr Row ROWS[] = {
    // the radix path and the schedule of the fused kernel
    Row("radix_packed_tiles", &KmmKnobs::rx_packed).any_non_zero(),
    Row("debug_p2f_round_slots", &KmmKnobs::dbg_p2f_cap).within(512, P2F_SLOTS).and_is(even)
        .saying("debug_p2f_round_slots must be even and in [512, 5888]"),
    Row("radix_min_units", &KmmKnobs::rx_min_units),
    Row("radix_grid_per_cu", &KmmKnobs::rx_grid_per_cu).within(1, 2).saying("radix_grid_per_cu must be 1 or 2"),
    Row("grid_per_cu", &KmmKnobs::grid_per_cu).within(1, 1024),
    Row("dynamic_schedule", &KmmKnobs::dynamic_schedule).any_non_zero(),
    Row("dyn_chunk", &KmmKnobs::dyn_chunk).within(1, 4096).write_only(),
    Row("debug_rx_buffer_limit", &KmmKnobs::dbg_rx_buf_limit).write_only(),
    // host packing (kmm_hostpack.hpp)
    Row("host_pack_threads", &KmmKnobs::host_pack_threads).within(0, 256),
    Row("host_pack_slice_kb", &KmmKnobs::host_pack_slice_kb).within(0, 65536),
    // compressed streams
    Row("bgzf_head_skip", &KmmKnobs::bgzf_head_skip).within(0, INT64_MAX).saying("bgzf_head_skip negative").write_only(),
    Row("bgzf_tail_stop", &KmmKnobs::bgzf_tail_stop).negative_as_minus_one().write_only(),
    Row("debug_bgzf_ring_slot_kb", &KmmKnobs::dbg_bgzf_slot_kb).aka("debug_ring_slot_kb").within(0, 1 << 20)
        .and_is(zero_or_a_power_of_two_from_4).saying("debug_ring_slot_kb: 0 or a power of two in [4, 2^20]").write_only(),
    Row("debug_bgzf_call_cap_kb", &KmmKnobs::dbg_bgzf_call_cap_kb).within(0, 7ll << 19)
        .saying("debug_bgzf_call_cap_kb outside [0, 3.5 GiB / 1 KiB]"),
    Row("debug_gzip_chunk_kb", &KmmKnobs::dbg_gzip_chunk_kb).within(0, 1 << 20).saying("debug_gzip_chunk_kb outside [0, 2^20]"),
    // SAM / BAM records: selection, the stream's reference count, strand and qualities
    Row("bam_exclude_flags", &KmmKnobs::bam_excl).within(0, 0xFFFF).saying("bam_exclude_flags outside [0, 0xFFFF]"),
    Row("bam_include_flags", &KmmKnobs::bam_incl).within(0, 0xFFFF).saying("bam_include_flags outside [0, 0xFFFF]"),
    Row("bam_min_mapq", &KmmKnobs::bam_min_mapq).within(0, 255),
    Row("bam_n_ref", &KmmKnobs::bam_n_ref_param).within(-1, 0x7FFFFFFFll).saying("bam_n_ref outside [-1, 2^31)"),
    Row("debug_bam_resync_kb", &KmmKnobs::dbg_bam_resync_kb).within(0, 1ll << 32).saying("debug_bam_resync_kb outside [0, 2^32]"),
    Row("use_record_qual", &KmmKnobs::use_record_qual).flag(),
    Row("original_strand", &KmmKnobs::original_strand).flag(),
    Row("min_base_quality", &KmmKnobs::min_base_quality).within(0, 93),
    Row("record_hits_min_base_quality", &KmmKnobs::rh_min_base_quality).within(0, 93),
    Row("record_keep", &KmmKnobs::record_keep).flag(),
    Row("record_keep_min_hits", &KmmKnobs::rk_min_hits).within(0, 0xFFFFFFFFll).saying("record_keep_min_hits outside [0, 2^32 - 1]"),
    Row("record_keep_min_permille", &KmmKnobs::rk_min_permille).within(0, 1000),
    Row("record_keep_invert", &KmmKnobs::rk_invert).flag(),
    Row("record_pairs_rule", &KmmKnobs::rk_pair_rule).flag()
        .saying("record_pairs_rule takes 0 (a pair matches when any mate does) or 1 (when both do)"),
    Row("record_names", &KmmKnobs::record_names).flag(),
    Row("record_names_mate_suffix", &KmmKnobs::record_names_mate_suffix).flag(),
    // kmm_map_records' test hooks and the overlap experiment, set between two calls in flight
    Row("debug_records_copy_stream", &KmmKnobs::dbg_rec_copy_stream).any_non_zero().write_only().unsynchronised(),
    Row("debug_records_skip", &KmmKnobs::dbg_rec_skip).write_only().unsynchronised(),
    Row("debug_records_piece_kb", &KmmKnobs::dbg_rec_piece_kb).within(0, 1 << 20).saying("debug_records_piece_kb outside [0, 2^20]")
        .unsynchronised(),
    Row("debug_records_grid", &KmmKnobs::dbg_rec_grid).within(0, 65536).unsynchronised(),
    // the counters
    counter("host_packed_calls", &KmmCounters::host_packed_calls),
    counter("host_packed_record_calls", &KmmCounters::host_packed_record_calls),
    counter("bgzf_prestaged_calls", &KmmCounters::bgzf_prestaged_calls),
    counter("bgzf_members", &KmmCounters::bgzf_members),
    counter("gzip_calls", &KmmCounters::gzip_calls),
    counter("gzip_members", &KmmCounters::gzip_members),
    counter("gzip_chunks", &KmmCounters::gzip_chunks),
    counter("gzip_false_starts", &KmmCounters::gzip_false_starts),
    counter("gzip_continuations", &KmmCounters::gzip_continuations),
    counter("gzip_inflated_bytes", &KmmCounters::gzip_inflated),
    counter("bam_calls", &KmmCounters::bam_calls),
    counter("bam_records", &KmmCounters::bam_records),
    counter("bam_records_excluded", &KmmCounters::bam_excluded),
    counter("bam_header_bytes", &KmmCounters::bam_header_bytes),
    counter("bam_false_starts", &KmmCounters::bam_false_starts),
    counter("bam_continuations", &KmmCounters::bam_continuations),
    counter("sam_calls", &KmmCounters::sam_calls),
    counter("sam_records", &KmmCounters::sam_records),
    counter("sam_records_excluded", &KmmCounters::sam_excluded),
    counter("sam_header_lines", &KmmCounters::sam_header_lines),
    counter("flat_uniform_batches", &KmmCounters::flat_uniform_batches),
    counter("read_hits_calls", &KmmCounters::read_hits_calls),
    counter("radix_sub_batch_kmers_effective", &KmmCounters::rx_sub_cap_last),
    counter("comm_sliced_reduces", &KmmCounters::comm_sliced_reduces),
    counter("radix_batches", &KmmCounters::n_radix_batches),
    counter("direct_batches", &KmmCounters::n_direct_batches),
};

template <size_t N>
inline const Row *find(const Row (&rows)[N], const char *name)
{
    for (const Row &r : rows)
        if (!strcmp(name, r.name) || (r.alias && !strcmp(name, r.alias)))
            return &r;
    return nullptr;
}

// Why a set of `name` to `value` is refused, written to err: the name is not one a set knows (row: what find gave, or null), it
// is read-only, or the value is none the row takes.  False: accepted, store it.
inline bool set_refused(const Row *row, const char *name, int64_t value, char *err, size_t n)
{
    if (!row || row->access == READ_ONLY)
        return snprintf(err, n, "unknown parameter '%s'", name), true;
    if (row->access == READ_ONLY_SAID)
        return snprintf(err, n, "%s is read-only", name), true;
    const bool ok = (row->accept == ANY_VALUE || (row->accept == ZERO_OR_ONE ? value == 0 || value == 1 : value >= row->lo && value <= row->hi)) &&
                    (!row->also || row->also(value));
    if (ok)
        return false;
    if (row->refusal)
        snprintf(err, n, "%s", row->refusal);
    else if (row->accept == ZERO_OR_ONE)
        snprintf(err, n, "%s takes 0 or 1", name);
    else
        snprintf(err, n, "%s outside [%lld, %lld]", name, (long long)row->lo, (long long)row->hi);
    return true;
}

inline bool get_refused(const Row *row, const char *name, char *err, size_t n)
{
    if (row && row->access != WRITE_ONLY)
        return false;
    return snprintf(err, n, "unknown parameter '%s'", name), true;
}

inline void store(const Row &row, KmmKnobs &k, int64_t value)
{
    const int64_t v = row.store == NON_ZERO ? value != 0 : row.store == NEGATIVE_AS_MINUS_ONE && value < 0 ? -1 : value;
    switch (row.at.type) {
    case Member::KNOB_BOOL: k.*row.at.kb = v != 0; break;
    case Member::KNOB_INT: k.*row.at.ki = (int)v; break;
    case Member::KNOB_U32: k.*row.at.ku = (uint32_t)v; break;
    case Member::KNOB_I64: k.*row.at.kl = v; break;
    default: break; // (counters are not stored to; a row without a field has a hook)
    }
}

inline int64_t load(const Row &row, const KmmKnobs &k, const KmmCounters &c)
{
    switch (row.at.type) {
    case Member::KNOB_BOOL: return k.*row.at.kb ? 1 : 0;
    case Member::KNOB_INT: return k.*row.at.ki;
    case Member::KNOB_U32: return k.*row.at.ku;
    case Member::KNOB_I64: return k.*row.at.kl;
    case Member::COUNTER_I64: return c.*row.at.cl;
    case Member::COUNTER_U64: return (int64_t)(c.*row.at.cu);
    default: return 0;
    }
}

} // namespace kmm_params
