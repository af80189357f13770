// kmm.hip — MI355X (gfx950 / CDNA4) kernels and C-ABI host code for kmer_mapper's hot path:
// reads -> 2-bit codes -> rolling k-mer pack -> modulo hash -> bucket gather -> compare/filter ->
// per-node atomic counts.  See include/kmm.h for the boundary and DESIGN.md for the layout.
//
// Reference semantics restated (never copied): kmer_mapper/mapper.pyx:53-69 (lookup),
// kmer_mapper/util.py:71-75 (extraction), kmer_mapper/command_line_interface.py:41 (N->A).
//
// Integer / gather work: no MFMA.  The bound is random HBM accesses, so the kernels are built for
// memory-level parallelism (U independent bucket gathers in flight per lane, then U independent
// first-entry gathers) at high occupancy; reads are staged through LDS as packed 2-bit codes so
// each byte is fetched from HBM exactly once with 16-byte coalesced loads.
//
// File map.  Here: the handle, its helpers, the C entry points, StreamCall and the drivers of the compressed streams.  Kernels:
// kmm_*.hpp.  Host code included further down, inside an anonymous namespace, behind the helpers it uses: kmm_radix_host.hpp (the
// radix path), kmm_sam_host.hpp (the SAM pieces of kmm_map_records), kmm_bam_host.hpp (kmm_map_bam behind the inflater; rs_*).
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "kmm.h"
#include "kmm_radix_plan.hpp" // (plain C++ with standard headers of its own: before the namespace the kernels live in)
#include "kmm_params.hpp"     // (the same: KmmKnobs, KmmCounters and the parameter table)
#include "kmm_seqindex_plan.hpp" // (the same: the limits, the table size and the prime search of kmm_seq_index_build)
#include "kmm_read_nodes_plan.hpp" // (the same: keys, best words, table slots and round cuts of kmm_read_nodes)

namespace {

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// Nothing C++ throws may cross the C ABI (std::vector / std::function allocate; a thread may fail to start): the entry points
// that run host-side machinery go through this.
template <typename F>
static int guarded(const char *what, F body)
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(KMM_ERR_NOMEM, "%s: out of host memory", what);
    } catch (const std::exception &e) {
        return fail(KMM_ERR_INTERNAL, "%s: %s", what, e.what());
    } catch (...) {
        return fail(KMM_ERR_INTERNAL, "%s: unexpected exception", what);
    }
}

static double ms_since(std::chrono::steady_clock::time_point a)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(KMM_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #expr,                 \
                        hipGetErrorString(e_));                                                    \
    } while (0)

#define KMMCHK(expr)                                                                               \
    do {                                                                                           \
        int r_ = (expr);                                                                           \
        if (r_ != KMM_OK)                                                                          \
            return r_;                                                                             \
    } while (0)

#include "kmm_probe.hpp"
#include "kmm_tile.hpp"
#include "kmm_records.hpp"
#include "kmm_kernels.hpp"
#include "kmm_read_hits.hpp"
#include "kmm_rh_qual.hpp"
#include "kmm_record_keep.hpp"
#include "kmm_radix.hpp"
#include "kmm_build.hpp"
#include "kmm_seqindex.hpp"
#include "kmm_read_nodes.hpp"

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// Move-only owners of what the host side allocates.  HipOwned holds one HIP handle (a device array, an event, a stream) and
// gives it back when it is reset, replaced or destroyed; put() hands the creating call (hipMalloc, hipEventCreate*,
// hipStreamCreate*) the slot to fill.  hipFree waits for the whole device: a reset() in the middle of a call is a
// synchronisation point.
template <typename H, hipError_t (*Free)(H)>
struct HipOwned {
    H h = nullptr;
    HipOwned() = default;
    HipOwned(HipOwned &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    HipOwned &operator=(HipOwned &&o) noexcept { if (this != &o) { (void)reset(); h = std::exchange(o.h, nullptr); } return *this; }
    ~HipOwned() { (void)reset(); }
    hipError_t reset() { H x = std::exchange(h, nullptr); return x ? Free(x) : hipSuccess; }
    H *put() { (void)reset(); return &h; }
    operator H() const { return h; }
};
template <typename T>
hipError_t free_device(T *p) { return hipFree(p); }
template <typename T>
using DevPtr = HipOwned<T *, free_device<T>>;
using Event = HipOwned<hipEvent_t, hipEventDestroy>;
using Stream = HipOwned<hipStream_t, hipStreamDestroy>;

// A device buffer that only grows (ensure).
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { (void)reset(); p = std::exchange(o.p, nullptr); cap = std::exchange(o.cap, 0); } return *this; }
    ~DevBuf() { (void)reset(); }
    hipError_t reset() { cap = 0; void *q = std::exchange(p, nullptr); return q ? hipFree(q) : hipSuccess; }
};

int ensure(DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap && b.p)
        return KMM_OK;
    HIPCHK(b.reset()); // blocks until the device is idle: safe w.r.t. in-flight kernels
    size_t want = bytes < 256 ? 256 : bytes;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        return fail(e == hipErrorOutOfMemory ? KMM_ERR_NOMEM : KMM_ERR_HIP,
                    "hipMalloc(%zu bytes) -> %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return KMM_OK;
}

bool is_device_ptr(const void *p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError(); // unregistered host memory: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

uint64_t magic_for(uint64_t m)
{
    if (m <= 1)
        return ~0ull;
    return (uint64_t)(((unsigned __int128)1 << 64) / m);
}

void default_lut(uint8_t lut[256])
{
    memset(lut, 0xFF, 256);
    lut['A'] = lut['a'] = 0;
    lut['C'] = lut['c'] = 1;
    lut['G'] = lut['g'] = 2;
    lut['T'] = lut['t'] = 3;
    lut['N'] = lut['n'] = 0; // command_line_interface.py:41
}

struct Stage {
    DevBuf bases, quals, offsets, tile_first, start_bits, kmers, lut, aux;
    Event done; // the last kernel that read this stage has finished
    bool used = false;
};

constexpr unsigned long long NO_BAD = ~0ull;

} // namespace

#include "kmm_comm.hpp"
#include "kmm_hostpack.hpp"
#include "kmm_gpu_inflate.hpp"
#include "kmm_gpu_gunzip.hpp"
#include "kmm_bgzf_out.hpp"
#include "kmm_bam.hpp"
#include "kmm_sam.hpp"

// What the BGZF writer (kmm_bgzf_out.hpp) keeps between calls: the workgroups' candidate scratch, the member slots of
// one round, their sizes and offsets, and the members one behind the other where they leave for host memory.
struct BzScratch {
    DevBuf cand, slots, sizes, offs, comp;
};

// Page-locked buffers are expensive to make (hipHostMalloc: ~50 ms per GB) and cheap to keep: the ones a handle gives up go
// to a process-wide shelf (at most 8 GiB), and kmm_host_reserve puts buffers there ahead of time — from another thread,
// while the index is uploaded — so that a one-shot `kmer_mapper map` does not pay for them inside its map phase.
struct PinnedShelf {
    std::mutex m;
    std::vector<std::pair<uint8_t *, size_t>> free_list;
    size_t bytes = 0;
    uint8_t *take(size_t want, size_t *got)
    {
        std::lock_guard<std::mutex> g(m);
        size_t best = free_list.size();
        for (size_t i = 0; i < free_list.size(); ++i)
            if (free_list[i].second >= want && (best == free_list.size() || free_list[i].second < free_list[best].second))
                best = i;
        if (best == free_list.size())
            return nullptr;
        uint8_t *p = free_list[best].first;
        *got = free_list[best].second;
        bytes -= *got;
        free_list.erase(free_list.begin() + (long)best);
        return p;
    }
    void give(uint8_t *p, size_t n)
    {
        if (!p)
            return;
        {
            std::lock_guard<std::mutex> g(m);
            if (bytes + n <= ((size_t)8 << 30)) {
                free_list.emplace_back(p, n);
                bytes += n;
                return;
            }
        }
        (void)hipHostFree(p);
    }
};
static PinnedShelf g_shelf;

// A page-locked buffer of the handle, given back to the shelf when it is reset or destroyed.
struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { reset(); }
    void reset() { g_shelf.give(std::exchange(p, nullptr), std::exchange(bytes, 0)); }
};
constexpr size_t RING_SLOT = (size_t)16 << 20;
#ifndef KMM_RING_SLOTS
#define KMM_RING_SLOTS 8 // (A/B builds: a ring the size of a batch never makes the packing threads wait)
#endif
constexpr int RING_SLOTS = KMM_RING_SLOTS;


struct TimedEvent {
    Event start, stop;
    int kernel_id = 0;
};

// What kmm_map_bgzf knows about a chunk of compressed bytes once they are on their way to HBM: the member chain.
struct BgzfStaged {
    std::vector<unsigned long long> m_off, o_rel; // member starts in the chunk; inflated offsets from the chunk's first member (o_rel[0] = 0)
    uint64_t p = 0;                               // bytes of whole members
    int chain_err = 0;                            // 1: no member at p, 2: implausible ISIZE
    uint32_t bad_isize = 0, bad_ms = 0;
    bool hit_cap = false;                         // the chain was cut at the size limit of a call
    bool staged = false;                          // the bytes went through the page-locked ring (else: not copied at all yet)
    double ms_scan_inside = 0;
};

// The handle's streams: a base of kmm_index, so that they are destroyed after everything else in it.
struct IndexStreams {
    Stream stream;      // kernels
    Stream copy_stream; // host -> HBM staging, overlaps the previous kernel
};

// The radix path's view of the index (rx_build), a base of kmm_index: the view (or its 16-bit directory alone) is dropped
// with one assignment, and the arrays keep their rx_* names in the handle.
struct RxDir16 {
    DevPtr<uint16_t> rx_pstart16;   // slice-relative 16-bit directory + first entry of every slice (for the current
    DevPtr<uint32_t> rx_slice_e0;   // part_shift; null when a slice holds more than 65535 entries or HBM is short)
    DevPtr<uint16_t> rx_slice_fmax; // largest frequency of every slice (with the two above)
};
struct RxSlotFilter {
    DevPtr<uint32_t> rx_slots;      // [F1][P2F_SLOT_WORDS] pass 2's slot filter (rx_filter_slot) for the current (w, f2); null where
};                                  // the geometry has none (RxGeometry::slot_filter), it is switched off, or HBM is short
struct RxArrays : RxDir16, RxSlotFilter {
    uint64_t rx_S = 0;        // entries in bucket order
    DevPtr<uint32_t> rx_pstart;
    DevPtr<uint64_t> rx_pkeys;     // packed form for the current (w, f2)
    DevPtr<uint64_t> rx_pkeys_raw; // the k-mers themselves (re-packed when part_shift changes)
    DevPtr<uint16_t> rx_pfreq;
    DevPtr<uint32_t> rx_pnodes, rx_porig, rx_ecnt, rx_ecnt_acc;
    DevPtr<uint32_t> rx_norder, rx_nnode; // entries in node order (k_rx_flush_sorted); absent if memory is short
    DevPtr<uint32_t> rx_occ;   // bit h = bucket h holds an entry: pass 2's empty-bucket filter (k_rx_p2f); optional
};

struct kmm_index : IndexStreams, RxArrays, KmmKnobs, KmmCounters { // (the stored parameter values and the counters: kmm_params.hpp)
    int device = 0;
    Event copied;
    DevPtr<uint4> buckets;
    DevPtr<uint4> entries;
    DevPtr<uint32_t> occ;              // occupancy bitmap, only for indexes small enough (see occ_max_bytes)
    int occ_shift = 0;                 // log2(bitmap bits per bucket)
    uint32_t bloom_words = 0;          // != 0: occ is a word-blocked Bloom filter
    bool wide = false;                 // 32-byte buckets (chosen when the index is too large for the bitmap)
    bool direct_deferred = false;      // the direct view (buckets, entries) is packed from the radix view on first use
    size_t direct_bytes = 0;           // HBM bytes of the direct view (resident or not yet)
    size_t occ_bytes_plan = 0;         // size of the direct view's pre-filter (0: none)
    int rx_why_not = 0;                // why the radix path is unavailable: 0 it is available, 1 modulo >= 2^31, 2 more
                                       // than 512 x 512 slices / slices too dense for LDS, 3 out of memory, 4 the
                                       // buckets of the index overlap (sum of bucket sizes > n_entries)
    uint32_t *counts = nullptr;          // own_counts_buf or the caller's buffer (kmm_bind_counts)
    DevPtr<uint32_t> own_counts_buf;
    DevPtr<uint8_t> lut_default;
    DevPtr<uint8_t> lut_codes;           // codes 0..3 map to themselves: flat reads compacted from raw records (k_rec_scatter)
    DevPtr<unsigned long long> first_bad;
    DevPtr<unsigned long long> stats;
    DevPtr<unsigned long long> queue;    // tile counter of the dynamic schedule
    uint64_t modulo = 0, magic = 0;
    int64_t n_entries = 0, max_node_id = 0;
    Stage stage[2];
    int cur = 0;
    int n_cu = 256;
    // radix path state (kmm_radix.hpp)
    bool rx_ok = false;   // the index fits the radix path's fan-out (<= 512 x 512 fine partitions)
    RxGeometry rx_geo;    // slice width and fan-out (kmm_radix_plan.hpp); assigned whole, a refused configuration leaves it as it was
    bool rx_no_mid = false; // experiments (KMM_RX_NO_MID, read at creation): pass 3 without its 4608-key variants
    uint32_t rx_max_slice = 0; // most entries in one fine partition's slice (for the current part_shift)
    bool rx_fits_small = false, rx_fits_mid = false; // all but one slice in 1000 hold at most RX_ECAP / RX_ECAP_MID entries
    int64_t rx_sub_cap_eff = 0;  // > 0: the smaller size an out-of-memory call settled on, tried first by the next calls
    int rx_sub_cap_eff_age = 0;  // calls since then (at 16 the caller's cap is tried again)
    const uint32_t *dbg_T1 = nullptr, *dbg_item_base = nullptr; // the latest sub-batch's tables (debug_rx_* parameters)
    const uint16_t *dbg_start1 = nullptr;
    uint32_t dbg_F1 = 0, dbg_NB = 0;
    std::unique_ptr<kmm_hostpack::Workers> pack_pool; // the packing threads ("host_pack_threads"), asleep between calls
    PinnedBuf pack_pinned;          // page-locked home of a packed records batch (kmm_hostpack.hpp)
    PinnedBuf ring[RING_SLOTS];     // the page-locked staging ring (ensure_ring)
    PinnedBuf pack_bits_pinned;     // ... and of the read-start bitset of packed raw records
    // kmm_map_bgzf: BGZF members inflated on the GPU (kmm_gpu_inflate.hpp).  Two sets of buffers in turn (the copy of call
    // i + 1 runs under the kernels of call i); the uncompressed bytes behind a call's last complete record wait in `carry`
    // for the next call.
    DevBuf bgzf_comp[2], bgzf_raw[2], bgzf_meta[2], bgzf_tabs, bgzf_err, bgzf_carry, bgzf_crc, bgzf_status;
    Event bgzf_done[2];
    Event bgzf_slot_ev[RING_SLOTS]; // copies out of / into the slots of the staging ring
    bool bgzf_used[2] = {false, false};
    int bgzf_cur = 0;
    int64_t bgzf_carry_len = 0;
    BgzfStaged bgzf_pre;         // the NEXT chunk, staged and walked under this chunk's inflate kernel (kmm_map_bgzf_hint_next)
    bool bgzf_pre_valid = false;
    const uint8_t *bgzf_pre_from = nullptr, *bgzf_hint_ptr = nullptr;
    int64_t bgzf_pre_n = 0, bgzf_hint_n = 0;
    int bgzf_pre_buf = 0;
    int64_t bgzf_calls = 0;
    // kmm_map_gzip: a plain gzip stream inflated on the GPU (kmm_gpu_gunzip.hpp).  The symbol slots come from an arena of
    // large blocks kept from call to call (a bump pointer per call); the stream's state (bit offset, mode, history length,
    // CRC register and length of the member in progress) and its last 32 KiB of output (gz_window) carry over.
    DevBuf gz_comp, gz_raw, gz_carry, gz_window, gz_tabs, gz_meta, gz_res, gz_win, gz_gmaps, gz_gwin, gz_err;
    std::vector<DevBuf> gz_arena; // (kept while a stream lasts, released when it ends: ~2.5 bytes per inflated byte of a call
                                  // plus 64 KiB per chunk — 10 GB for a call of 3.3 GB)
    kmm_gunzip::StreamState gz_state;
    int64_t gz_carry_len = 0;
    double gz_ratio = 4.0;        // inflated / compressed bytes of the stream so far (the slots' size)
    // kmm_map_bam: the BGZF members of a BAM file inflated as for kmm_map_bgzf, the records found and decoded on the GPU
    // (kmm_bam.hpp): the tiles' claims (two buffers: the link passes read one and write the other), the control words, the
    // tiles' output offsets and the two-line FASTA the records become.  The stream's reference count (from its header)
    // validates refID / next_refID of every record.
    DevBuf bam_tiles[2], bam_bad, bam_base, bam_ctl, bam_out;
    int32_t bam_n_ref = -1;       // -1: no BAM stream started on this handle
    // kmm_bam_header / kmm_bam_find_record_start (a rank's share of a BAM file): buffers of their own — the compressed
    // window, its inflated bytes, the member offsets, the inflater's error words and status bytes — so that a stream in
    // progress on the handle is not touched
    DevBuf rs_comp, rs_raw, rs_meta, rs_err, rs_status;
    // KMM_FORMAT_SAM (kmm_sam.hpp): the tiles' line counts, their output offsets, the totals; the filter is bam_excl
    DevBuf sam_tiles, sam_base, sam_ctl;
    // record selection (kmm_select.hpp): "bam_include_flags", "bam_min_mapq" and the region list of
    // kmm_set_record_regions, merged twice — by refID for kmm_map_bam (sel_iv_id; empty when a region came without an id) and by
    // name for KMM_FORMAT_SAM (sel_iv_name, the names in sel_names; empty when one came without a name) — and held in one small
    // device buffer: the two interval lists, the name offsets, the name bytes
    int sel_n_regions = 0, sel_keep_unplaced = 0; // regions as given (0: no list)
    std::vector<kmm_sel::Interval> sel_iv_id, sel_iv_name;
    std::vector<std::string> sel_names;
    DevBuf sel_buf;
    size_t sel_off_name_iv = 0, sel_off_name_off = 0, sel_off_names = 0;
    // the floor of the record-hits mode ("record_hits_min_base_quality").  rq_exempt / rq_text_off: set around the inner
    // records call of kmm_map_bam's named form — the records that pass unmasked (no stored qualities), by the offset of their quality
    // line in the inner call's text, and where the piece at work starts in that text.  bam_mate_exempt: the flags of the waiting mate 1.
    const uint32_t *rq_exempt = nullptr;
    int64_t rq_text_off = 0;
    DevBuf rq_exempt_buf, bam_mate_exempt;
    int64_t bam_mate_exempt_len = 0; // the bytes of waiting text that bam_mate_exempt holds flags for (0: none)
    bool ecnt_dirty = false;  // rx_ecnt holds hits that are not in `counts` yet
    bool rx_unchecked = false; // radix passes have run since the conservation counters were last compared (drain)
    DevBuf rx_buf1, rx_buf2, rx_meta, rx_probe; // (rx_probe: scratch of the marginal-byte probe builds, kmm_radix.hpp)
    // deferred device-side error, sticky until kmm_reset_counts
    int sticky_rc = KMM_OK;
    std::string sticky_msg;
    uint64_t map_calls = 0;   // sequence number of map calls on this handle (error reports name the call)
    // the record-hits mode: while "record_hits" is 1 or 2 the record calls append one entry per record to this
    // queue instead of counting nodes.  Entries [rhq_head, rhq_head + rhq_pending) of both arrays wait for
    // kmm_take_record_hits; rhq_mode: the last non-zero "record_hits" (whether the pending entries have their windows)
    int rhq_mode = 0;
    DevBuf rhq_hits, rhq_win;
    int64_t rhq_head = 0, rhq_pending = 0, rhq_cap = 0;
    DevBuf rn_table; // kmm_read_nodes: a round's vote table, kept between calls up to RN_KEEP_TABLE_BYTES
    // the record-keep mode: with "record_keep" 1 the record calls also append the text of every record whose entry
    // passes the keep rule to rkq[0].  ctl (device): {bytes, records} of the queue's true tail, advanced by the kernels; the same
    // pair as a call found it (put back when the call fails); the kept bytes and records of the piece at work.  bound: what
    // the host knows, an upper bound of the pending bytes (the consumed bytes of the pieces since the last take), which the queue
    // holds room for before a piece's kernels are launched.  rk_tile / rk_super: kept bytes, and behind them kept records, per
    // tile and super-tile of that piece.
    // [0]: the queue of kept text; [1]: the mate-2 texts of kmm_map_record_pairs, whose mate-1 texts go to [0]
    struct RkQueue {
        DevBuf text, ctl;
        int64_t bound = 0, cap = 0;
    } rkq[2];
    DevBuf rk_tile, rk_super;
    // keeping mates together: "record_pairs" 1: the records of a stream are interleaved, 2i and 2i + 1 are mates,
    // and the keep rule is rk_pair_keep over their two entries ("record_pairs_rule": RK_PAIR_ANY / RK_PAIR_BOTH); both are read
    // only while "record_keep" is 1.  rk_snap: what the last kmm_map_records found (entries pending, the bound of rkq[0]; the
    // tail is kept on the device), which a stream call whose last chunk ends with an unpaired record puts back.
    // rk_pair_entries: the per-buffer entries of kmm_map_record_pairs before they are zipped into the queue.
    struct { int64_t pending = 0, bound = 0; bool valid = false; } rk_snap;
    DevBuf rk_pair_entries;
    // the mates of a name-collated BAM file: "record_names_pairs" 1: the selected records of a kmm_map_bam stream
    // are mates in file order, 2p and 2p + 1.  bam_mate: the text of a window's odd last selected record, which the next window's
    // decode writes behind (bam_mate_len bytes; 0: none); bam_pairs_done: pairs of the stream handed over so far (the ordinals
    // of the error reports).  rk_mates_call: set around kmm_map_bam's inner kmm_map_records alone — that call then takes the
    // interleaved pair form without "record_pairs", and every piece has its pairs' names compared (k_rk_pair_names), the first
    // differing pair read back through rk_names_ctl (behind it: the decode's three counters as the call found them).
    bool rk_mates_call = false;
    DevBuf bam_mate, rk_names_ctl;
    int64_t bam_mate_len = 0, bam_pairs_done = 0;
    // the raw form: "record_bam" 1: kmm_map_bam with "record_hits" and "record_keep" maps the selected records in the
    // two-line FASTA form and appends the kept records' own bytes (block_size word and all) to rkq[0].  rk_raw_call: set around
    // that call's inner kmm_map_records alone, which then appends its entries but none of the FASTA text.  bam_raw: the record
    // base, the kept bytes' base, the kept bytes and records per tile, the totals.  bam_hdr: the header of the last stream
    // started with KMM_FORMAT_NEW_STREAM, magic through the last reference (kmm_bam_stream_header); bam_hdr_valid: there is one.
    bool rk_raw_call = false, bam_hdr_valid = false;
    DevBuf bam_raw;
    std::vector<uint8_t> bam_hdr;
    // mates kept together in the raw form: "record_bam_mates" 1: the selected records of a kmm_map_bam stream are mates
    // in file order and their own bytes are kept or dropped together.  The inner records call runs with rk_mates_call AND
    // rk_raw_call: whole pairs, no text, no name lines to compare.  A window's odd last selected record waits twice: its FASTA text
    // in bam_mate (bam_mate_len, as DESIGN 4.23), its raw bytes in bam_raw_mate (bam_raw_mate_len).  bam_raw_ctl: the call's three
    // control words (kmm_bam.hpp k_bam_raw_count_pairs), read back once per window.  bam_raw_pos: where the selected record of
    // every entry of the call starts, left by the count walk for the mate check.
    DevBuf bam_raw_mate, bam_raw_ctl, bam_raw_pos;
    DevBuf bam_mate_next, bam_raw_mate_next; // the spare carry buffers: a call fills them before it appends and swaps them in when it is done
    int64_t bam_raw_mate_len = 0;
    // SAM lines kept as SAM lines: "record_sam" 1 / 2: a KMM_FORMAT_SAM call with "record_hits" and "record_keep" maps
    // the selected records in the two-line FASTA form (the inner piece call under rk_raw_call: entries, no text) and appends the
    // kept records' own lines to rkq[0]; 1: the header lines as well.  sam_raw: per piece, the tiles' {records, header lines} in
    // front, the spans of the write walk, their kept lengths and prefixes, the blocks' sums and bases, the totals.
    DevBuf sam_raw;
    // mates kept together in SAM output: "record_sam_mates" 1: the selected records of a SAM stream are mates in file
    // order and their lines are kept or dropped together.  The inner piece call runs with rk_mates_call AND rk_raw_call, as under
    // "record_bam_mates".  A piece's odd last selected record waits twice: its FASTA text in sam_mate (sam_mate_len), its line in
    // sam_mate_line (sam_mate_line_len); sam_pairs_done: pairs of the stream handed over so far.  *_next: the spare buffers a piece
    // fills before it appends and swaps in when it is done; *_call0: the waiting mate as the call found it (sam_mate_saved: it was
    // moved there by a piece of the call), put back by a call that fails.  sam_mates_ctl: a piece's three control words;
    // sam_span_of: its spans by entry.
    DevBuf sam_mate, sam_mate_line, sam_mate_next, sam_mate_line_next, sam_mate_call0, sam_mate_line_call0, sam_mates_ctl, sam_span_of;
    int64_t sam_mate_len = 0, sam_mate_line_len = 0, sam_pairs_done = 0, sam_mate_len_call0 = 0, sam_mate_line_len_call0 = 0;
    bool sam_mate_saved = false;
    BzScratch bz; // kmm_take_kept_bgzf
    ncclComm_t comm = nullptr; // multi-process communicator of this handle (kmm_comm_init_rank)
    int comm_rank = -1, comm_size = 0;
    Stream comm_stream;
    std::vector<Event> comm_events;
    std::vector<uint64_t> flush_cuts; // entry (node order) where node range s begins, for comm_slices ranges; [slices + 1]
    // timing
    bool timing = false;
    std::vector<TimedEvent> ev_used;
    std::vector<TimedEvent> ev_free;
    double ms_total[KMM_N_KERNELS] = {0};
    int64_t launches[KMM_N_KERNELS] = {0};
};

// What kmm_seq_index_build returns: the five arrays in device memory, each in an owner of its own.
struct kmm_seq_index {
    int device = 0;
    DevBuf h2i, nk, kmers, nodes, freqs;
    int64_t n_entries = 0, n_windows = 0, n_pairs = 0;
    uint64_t modulo = 0;
};

namespace {

IndexView view_of(const kmm_index *ix)
{
    IndexView v;
    v.buckets = ix->buckets;
    v.entries = ix->entries;
    v.occ = ix->use_occ ? ix->occ : nullptr;
    v.occ_shift = ix->occ_shift;
    v.bloom_words = ix->bloom_words;
    v.wide = ix->wide ? 1 : 0;
    v.counts = ix->counts;
    v.stats = ix->stats;
    v.modulo = ix->modulo;
    v.magic = ix->magic;
    return v;
}

struct ScopedTimer {
    kmm_index *ix;
    TimedEvent ev{};
    bool active = false;
    int begin(kmm_index *ix_, int kernel_id)
    {
        ix = ix_;
        if (!ix->timing)
            return KMM_OK;
        if (!ix->ev_free.empty()) {
            ev = std::move(ix->ev_free.back());
            ix->ev_free.pop_back();
        } else {
            HIPCHK(hipEventCreate(ev.start.put()));
            HIPCHK(hipEventCreate(ev.stop.put()));
        }
        ev.kernel_id = kernel_id;
        HIPCHK(hipEventRecord(ev.start, ix->stream));
        active = true;
        return KMM_OK;
    }
    int end()
    {
        if (!active)
            return KMM_OK;
        HIPCHK(hipEventRecord(ev.stop, ix->stream));
        ix->ev_used.push_back(std::move(ev));
        active = false;
        return KMM_OK;
    }
};

int rx_flush(kmm_index *ix); // (kmm_radix_host.hpp)
int rx_build_slots(kmm_index *ix);
bool rx_slots_active(const kmm_index *ix);
int rx_check_conservation(kmm_index *ix);
int ensure_direct(kmm_index *ix);
constexpr size_t KMM_STAT_BYTES = (size_t)KMM_STAT_SHARDS * KMM_STAT_STRIDE * 8;

// Drain the streams and surface deferred device-side errors (invalid bases, malformed records, bad offsets).
// The reference raises before any count of the offending chunk is added (bionumpy's encoder, util.py:72); here
// the chunk's valid windows have already been counted when the error is seen, so the error stays on the handle:
// every later synchronising call fails with the same code until kmm_reset_counts clears counts and error together.
int drain(kmm_index *ix)
{
    KMMCHK(rx_flush(ix));
    HIPCHK(hipStreamSynchronize(ix->copy_stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    if (ix->sticky_rc != KMM_OK)
        return fail(ix->sticky_rc, "%s", ix->sticky_msg.c_str());
    KMMCHK(rx_check_conservation(ix));
    unsigned long long bad[3] = {NO_BAD, NO_BAD, NO_BAD};
    HIPCHK(hipMemcpy(bad, ix->first_bad, sizeof bad, hipMemcpyDeviceToHost));
    if (bad[0] != NO_BAD || bad[1] != NO_BAD || bad[2] != NO_BAD) {
        unsigned long long reset[3] = {NO_BAD, NO_BAD, NO_BAD};
        HIPCHK(hipMemcpy(ix->first_bad, reset, sizeof reset, hipMemcpyHostToDevice));
        char where[160];
        snprintf(where, sizeof where, " [one of the map calls since the last synchronising call; the latest was call "
                 "#%llu on this handle; counts are invalid until kmm_reset_counts]", (unsigned long long)ix->map_calls);
        int rc;
        if (bad[2] != NO_BAD)
            rc = fail(KMM_ERR_INVALID_ARG, "read_offsets of a mapped chunk is not non-decreasing at read %llu%s",
                      bad[2], where);
        else if (bad[1] != NO_BAD)
            rc = fail(KMM_ERR_MALFORMED,
                      "record structure violated at byte offset %llu of a mapped chunk (a record line "
                      "does not start with '@' / '+' / '>'%s): multi-line FASTA/FASTQ is not supported by "
                      "the GPU reader%s", bad[1],
                      ix->min_base_quality > 0 ? ", or a quality line that ends there is not as long as its sequence line "
                                                 "(checked with min_base_quality set)"
                      : ix->rh_min_base_quality > 0 ? ", or a quality line that ends there is not as long as its sequence line "
                                                      "(checked with record_hits_min_base_quality set)" : "", where);
        else
            rc = fail(KMM_ERR_INVALID_BASE,
                      "read byte at offset %llu of a mapped chunk is not a nucleotide under the "
                      "lookup table (the reference's DNA encoder raises here)%s", bad[0], where);
        ix->sticky_rc = rc;
        ix->sticky_msg = g_err;
        return rc;
    }
    return KMM_OK;
}

int grid_for(const kmm_index *ix, int64_t work_items, int per_cu)
{
    int64_t cap = (int64_t)ix->n_cu * per_cu;
    int64_t g = work_items < cap ? work_items : cap;
    return (int)(g < 1 ? 1 : g);
}

// Grid of the fused kernel.  Every workgroup pays a LUT load, an aggregation-table init and a flush, so
// small batches want several tiles per workgroup (>= 4 once all CU slots are taken), while large batches
// run ~15 % faster with many more workgroups than CU slots (measured: 8 / 16 / 64 per CU = 23.1 / 21.0 /
// 20.2 ms per 1.2e9 k-mers).
int grid_for_tiles(const kmm_index *ix, int64_t n_tiles)
{
    const int64_t slots = (int64_t)ix->n_cu * 8;
    const int64_t cap = (int64_t)ix->n_cu * ix->grid_per_cu;
    int64_t g = n_tiles <= slots ? n_tiles : n_tiles / 4;
    if (n_tiles > slots && g < slots)
        g = slots;
    if (g > cap)
        g = cap;
    return (int)(g < 1 ? 1 : g);
}

// The schedule of a direct launch over n_units tiles or spans (device side: for_owned_units, kmm_kernels.hpp).  Large
// launches: persistent workgroups, one per CU slot, and the dynamic unit queue, zeroed here; small ones: the static
// schedule, queue == null.
struct DirectSchedule {
    dim3 grid;
    unsigned long long *queue;
};

int direct_schedule(kmm_index *ix, int64_t n_units, DirectSchedule *sched)
{
    const int64_t slots = (int64_t)ix->n_cu * 8;
    const bool dynamic = ix->dynamic_schedule && n_units >= slots * 4 * ix->dyn_chunk;
    if (dynamic)
        HIPCHK(hipMemsetAsync(ix->queue, 0, 3 * sizeof(unsigned long long), ix->stream));
    sched->grid = dim3(dynamic ? (unsigned)slots : (unsigned)grid_for_tiles(ix, n_units));
    sched->queue = dynamic ? ix->queue : nullptr;
    return KMM_OK;
}

// The probe flavour of an index view (kmm_probe.hpp) as a compile-time constant: f(std::integral_constant<int, PROBE_...>).
template <typename F>
void with_probe_flavour(const IndexView &iv, F &&f)
{
    if (iv.occ && iv.wide)
        f(std::integral_constant<int, PROBE_WIDE_FILTER>{});
    else if (iv.occ)
        f(std::integral_constant<int, PROBE_BITMAP>{});
    else if (iv.wide)
        f(std::integral_constant<int, PROBE_WIDE>{});
    else
        f(std::integral_constant<int, PROBE_NARROW>{});
}

// Whether a selection beyond the exclude mask is set, as a compile-time constant for the k_bam_raw_*<SELECTED> kernels: f(S).
template <typename F>
void with_selected(bool selected, F &&f)
{
    if (selected)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// Stage a host array into the given device buffer on the copy stream; device arrays pass through.
template <typename TT>
int stage_in(kmm_index *ix, DevBuf &buf, const TT *src, size_t count, const TT **dev, bool *staged)
{
    if (count == 0) {
        KMMCHK(ensure(buf, 256));
        *dev = static_cast<const TT *>(buf.p);
        return KMM_OK;
    }
    if (is_device_ptr(src)) {
        *dev = src;
        return KMM_OK;
    }
    KMMCHK(ensure(buf, count * sizeof(TT)));
    HIPCHK(hipMemcpyAsync(buf.p, src, count * sizeof(TT), hipMemcpyHostToDevice, ix->copy_stream));
    *dev = static_cast<const TT *>(buf.p);
    *staged = true;
    return KMM_OK;
}

Stage &next_stage(kmm_index *ix)
{
    Stage &s = ix->stage[ix->cur];
    ix->cur ^= 1;
    return s;
}

// Every map call: (1) the stage's buffers may be overwritten once the kernels of the call that
// last used them are done; (2) kernels may start once the copies are in; (3) borrowed host buffers
// are free again once the copies are done.
int stage_acquire(kmm_index *ix, Stage &s)
{
    if (s.used)
        HIPCHK(hipStreamWaitEvent(ix->copy_stream, s.done, 0));
    return KMM_OK;
}

int stage_copies_done(kmm_index *ix)
{
    HIPCHK(hipEventRecord(ix->copied, ix->copy_stream));
    HIPCHK(hipStreamWaitEvent(ix->stream, ix->copied, 0));
    return KMM_OK;
}

int stage_release(kmm_index *ix, Stage &s, bool staged)
{
    HIPCHK(hipEventRecord(s.done, ix->stream));
    s.used = true;
    if (staged)
        HIPCHK(hipEventSynchronize(ix->copied));
    return KMM_OK;
}

// Does the caller's lookup table have a break entry (KMM_LUT_BREAK)?  A table in HBM is copied back (256 bytes).
int lut_has_break(const uint8_t *lut, bool *has_break)
{
    *has_break = false;
    if (!lut)
        return KMM_OK; // (the default table: N -> A, no breaks)
    uint8_t copy[256];
    if (is_device_ptr(lut)) {
        HIPCHK(hipMemcpy(copy, lut, 256, hipMemcpyDeviceToHost));
        lut = copy;
    }
    *has_break = memchr(lut, KMM_LUT_BREAK, 256) != nullptr;
    return KMM_OK;
}

// has_break: whether the table has a break entry — the call then marks the break bytes as one-base reads in its
// read-start bitset (k_mark_breaks, k_rec_scatter<true>, MODE_RECORDS_BRK) and takes the ragged front ends.
int resolve_lut(kmm_index *ix, Stage &s, const uint8_t *lut, const uint8_t **dev, bool *staged, bool *has_break)
{
    KMMCHK(lut_has_break(lut, has_break));
    if (!lut) {
        *dev = ix->lut_default;
        return KMM_OK;
    }
    return stage_in<uint8_t>(ix, s.lut, lut, 256, dev, staged);
}

// k == 1 with a break table: "no read start inside (p, p + k - 1]" is an empty condition — the break's own window
// could not be killed.  Refused by every entry point that takes a table.
int check_k_lut(int k, const uint8_t *lut)
{
    if (k != 1 || !lut)
        return KMM_OK;
    bool has_break = false;
    KMMCHK(lut_has_break(lut, &has_break));
    if (has_break)
        return fail(KMM_ERR_INVALID_ARG, "k = 1 with a lookup table that has a break entry (KMM_LUT_BREAK): needs k >= 2");
    return KMM_OK;
}

// Layout choice by index size (profiles/r01/partitioned_path_ablation.md, ms per 1.2e9 k-mers, same box):
//   16-byte buckets + L2 bitmap vs 32-byte buckets without: 10 M entries 20.2 / 24.4, 15 M 21.4 / 26.3,
//   20 M 23.6 / 27.9, 40 M (10 MB bitmap) 28.7 / 30.3, 100 M (25 MB bitmap) 34.0 / 31.7.
// (with fingerprints: 55 M entries 28.1 bitmap / 30.9 wide, 70 M 29.2 / 31.2, 100 M 30.6 / 31.7, 200 M 32.4 / 27.9)
constexpr size_t KMM_OCC_MAX_BYTES = (size_t)20 << 20;  // 168 M buckets at one bit per bucket
constexpr size_t KMM_BLOOM_MAX_BYTES = (size_t)4 << 20;  // Bloom filter size cap (L2 of one XCD)
constexpr int64_t KMM_BLOOM_MAX_ENTRIES = 20000000;     // beyond: fewer than ~2.5 bits per key, no better than the bitmap
constexpr size_t KMM_OCC_SWEET_BYTES = (size_t)5 << 20; // bitmap size that still lives in the 4 MiB L2s + MALL
constexpr int TILE_S = 4;
constexpr int TILE_T = 256 * TILE_S;

// Exclusive scan of n uint32 values on the device (in -> out): 1024-wide block scans, recursing on the
// block totals (n < 2^32 needs at most 4 levels).  All launches go to `stream`; ensure() may hipFree (device-wide sync).  `scratch` holds one DevBuf pair per level and is sized
// by the caller ONCE — it must not reallocate while outer levels hold references into it.
constexpr size_t SCAN_MAX_LEVELS = 8;
int scan_exclusive(const uint32_t *in, uint32_t *out, uint64_t n, std::vector<DevBuf> &scratch,
                   size_t level, hipStream_t stream)
{
    const uint64_t n_blocks = (n + 1023) / 1024;
    if (level >= SCAN_MAX_LEVELS || scratch.size() < 2 * SCAN_MAX_LEVELS)
        return fail(KMM_ERR_INVALID_ARG, "scan_exclusive: level %zu out of range", level);
    DevBuf &sums = scratch[2 * level], &pre = scratch[2 * level + 1];
    KMMCHK(ensure(sums, (size_t)n_blocks * 4));
    hipLaunchKernelGGL(k_scan_blocks, dim3((unsigned)n_blocks), dim3(1024), 0, stream, in, out, (uint32_t *)sums.p, n);
    HIPCHK(hipGetLastError());
    if (n_blocks == 1)
        return KMM_OK;
    KMMCHK(ensure(pre, (size_t)n_blocks * 4));
    KMMCHK(scan_exclusive((const uint32_t *)sums.p, (uint32_t *)pre.p, n_blocks, scratch, level + 1, stream));
    uint64_t g = (n + 255) / 256;
    if (g > 65536)
        g = 65536;
    hipLaunchKernelGGL(k_scan_add, dim3((unsigned)g), dim3(256), 0, stream, out, (const uint32_t *)pre.p, n);
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

// kmm_build_index on device arrays and a stream (kmm_build.hpp): kmers / nodes [n] -> the five arrays, all device memory, all
// launches on `st`, nothing waited for.  Shared by kmm_build_index and kmm_seq_index_build (kmm_seqindex_host.hpp).
struct BiScratch {
    DevBuf cur, src, list, ksort;
    std::vector<DevBuf> scan{2 * SCAN_MAX_LEVELS};
};

int bi_build_device(hipStream_t st, const uint64_t *kmers, const int32_t *nodes, int64_t n, uint64_t M, uint32_t *w_nk, uint32_t *w_h2i,
                    uint64_t *w_ko, int32_t *w_no, uint16_t *w_fo, BiScratch &s)
{
    const uint64_t magic = magic_for(M);
    KMMCHK(ensure(s.cur, (size_t)M * 4));
    HIPCHK(hipMemsetAsync(w_nk, 0, (size_t)M * 4, st));
    HIPCHK(hipMemsetAsync(s.cur.p, 0, (size_t)M * 4, st));
    int64_t g = (n + 255) / 256;
    if (g > 65536) g = 65536;
    if (g < 1) g = 1;
    uint64_t gm = (M + 255) / 256;
    if (gm > 65536) gm = 65536;
    if (n > 0)
        hipLaunchKernelGGL(k_bi_hist, dim3((unsigned)g), dim3(256), 0, st, kmers, n, M, magic, w_nk);
    KMMCHK(scan_exclusive(w_nk, w_h2i, M, s.scan, 0, st));
    if (n > 0) {
        KMMCHK(ensure(s.src, (size_t)n * 4));
        hipLaunchKernelGGL(k_bi_scatter, dim3((unsigned)g), dim3(256), 0, st, kmers, n, M, magic, w_h2i, (uint32_t *)s.cur.p,
                           (uint32_t *)s.src.p);
        hipLaunchKernelGGL(k_bi_place, dim3((unsigned)g), dim3(256), 0, st, kmers, nodes, n, M, magic, w_h2i, w_nk,
                           (const uint32_t *)s.src.p, w_ko, w_no, w_fo);
        // buckets with more than BI_BIG entries: listed, then ordered by one workgroup each
        const size_t list_cap = (size_t)n / BI_BIG + 2;
        KMMCHK(ensure(s.list, (list_cap + 1) * 4));
        KMMCHK(ensure(s.ksort, (size_t)n * 8));
        uint32_t *d_count = (uint32_t *)s.list.p + list_cap;
        HIPCHK(hipMemsetAsync(d_count, 0, 4, st));
        hipLaunchKernelGGL(k_bi_list_big, dim3((unsigned)gm), dim3(256), 0, st, w_nk, M, (uint32_t *)s.list.p, d_count);
        hipLaunchKernelGGL(k_bi_big, dim3(1024), dim3(1024), 0, st, kmers, nodes, w_h2i, w_nk, (const uint32_t *)s.list.p, d_count,
                           (uint32_t *)s.src.p, (uint64_t *)s.ksort.p, w_ko, w_no, w_fo);
    }
    // the format leaves hashes_to_index = 0 for empty buckets (upstream fills only the used ones)
    hipLaunchKernelGGL(k_bi_zero_empty, dim3((unsigned)gm), dim3(256), 0, st, w_h2i, w_nk, M);
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

#include "kmm_radix_host.hpp"

template <int MODE>
int launch_map_reads(kmm_index *ix, const ReadsView &rv, int k, int max_freq, int also_rc)
{
    const int64_t n_tiles = (rv.total + TILE_T - 1) / TILE_T;
    // raw records reach this function only for the direct path: on the radix path they are compacted into flat reads
    // first (map_records_piece_radix)
    const bool radix = mode_is_records(MODE) ? false : use_radix(ix, rv.total);
    if (!radix) {
        KMMCHK(ensure_direct(ix));
        ix->n_direct_batches++;
        const IndexView iv = view_of(ix); // (the direct view may have been packed just now)
        ScopedTimer tm;
        KMMCHK(tm.begin(ix, KMM_KERNEL_MAP_READS));
        DirectSchedule sched;
        KMMCHK(direct_schedule(ix, n_tiles, &sched));
        with_probe_flavour(iv, [&](auto probe) {
            hipLaunchKernelGGL((k_map_reads<TILE_S, MODE, decltype(probe)::value>), sched.grid, dim3(256), 0, ix->stream, rv, iv,
                               k, max_freq, also_rc, (int64_t)0, n_tiles, sched.queue, ix->dyn_chunk);
        });
        HIPCHK(hipGetLastError());
        return tm.end();
    }
    if constexpr (mode_is_records(MODE)) {
        return fail(KMM_ERR_INTERNAL, "raw records reach the radix path as flat reads only");
    } else {
        if (MODE == MODE_UNIFORM && rv.pk_rpt) // reads of one length: tiles of whole reads, every computed window a real k-mer
            return launch_rx<MODE_PACKED>(ix, rv, nullptr, 0, k, max_freq, also_rc);
        return launch_rx<MODE>(ix, rv, nullptr, 0, k, max_freq, also_rc);
    }
}


// The direct view (kmm_probe.hpp): bucket records + 16-byte entries (+ the L2 pre-filter for small indexes), packed
// from the caller's arrays at creation or from the radix view's bucket-ordered copy later.  Synchronous.
template <typename Src>
int direct_build(kmm_index *ix, const Src &src, int64_t n_entries, size_t occ_bytes, uint32_t *d_err)
{
    const uint64_t M = ix->modulo;
    const size_t nb = sizeof(uint4) * (size_t)M * (ix->wide ? 2 : 1), ne = sizeof(uint4) * (size_t)(n_entries > 0 ? n_entries : 1);
    hipError_t e = hipMalloc(ix->buckets.put(), nb);
    if (e == hipSuccess) e = hipMalloc(ix->entries.put(), ne);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        (void)ix->buckets.reset();
        return fail(e == hipErrorOutOfMemory ? KMM_ERR_NOMEM : KMM_ERR_HIP, "direct view of the index (%zu + %zu bytes): %s",
                    nb, ne, hipGetErrorString(e));
    }
    if (ix->wide)
        hipLaunchKernelGGL((k_pack_buckets_wide<Src>), dim3(grid_for(ix, (int64_t)((M + 255) / 256), 16)), dim3(256), 0,
                           ix->stream, src, M, n_entries, ix->max_node_id, ix->buckets, d_err);
    else
        hipLaunchKernelGGL((k_pack_buckets<Src>), dim3(grid_for(ix, (int64_t)((M + 255) / 256), 16)), dim3(256), 0,
                           ix->stream, src, M, n_entries, ix->max_node_id, ix->buckets, d_err);
    if (n_entries > 0)
        hipLaunchKernelGGL((k_pack_entries<Src>), dim3(grid_for(ix, (n_entries + 255) / 256, 16)), dim3(256), 0, ix->stream,
                           src, n_entries, ix->max_node_id, ix->entries, d_err);
    e = hipGetLastError();
    // occupancy bitmap / Bloom filter (16-byte layout only), built from the k-mers while they are here
    if (e == hipSuccess && occ_bytes) {
        e = hipMalloc(ix->occ.put(), occ_bytes);
        if (e == hipSuccess) e = hipMemsetAsync(ix->occ, 0, occ_bytes, ix->stream);
        if (e == hipSuccess && n_entries > 0) {
            if (ix->bloom_words)
                hipLaunchKernelGGL(k_build_bloom, dim3(grid_for(ix, (n_entries + 255) / 256, 16)), dim3(256), 0, ix->stream,
                                   src.kmers, n_entries, ix->bloom_words, ix->occ);
            else
                hipLaunchKernelGGL(k_build_occ, dim3(grid_for(ix, (n_entries + 255) / 256, 16)), dim3(256), 0, ix->stream,
                                   src.kmers, n_entries, M, ix->magic, ix->occ_shift, ix->occ);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess)
        return fail(KMM_ERR_HIP, "index repack: %s", hipGetErrorString(e));
    return KMM_OK;
}

// Called by every entry point that needs the direct view (small batches, kmm_in_index).
int ensure_direct(kmm_index *ix)
{
    if (ix->buckets || !ix->direct_deferred)
        return KMM_OK;
    DevBuf d_err;
    KMMCHK(ensure(d_err, 4));
    HIPCHK(hipMemsetAsync(d_err.p, 0, 4, ix->stream));
    IdxRx src;
    src.pstart = ix->rx_pstart; src.kmers = ix->rx_pkeys_raw; src.nodes = ix->rx_pnodes; src.freqs = ix->rx_pfreq;
    const int rc = direct_build(ix, src, (int64_t)ix->rx_S, ix->occ_bytes_plan, (uint32_t *)d_err.p);
    if (rc == KMM_OK)
        ix->direct_deferred = false;
    return rc;
}

int check_k(int k)
{
    if (k < 1 || k > KMM_MAX_K)
        return fail(KMM_ERR_INVALID_ARG, "k=%d outside [1, %d]", k, KMM_MAX_K);
    return KMM_OK;
}

#include "kmm_seqindex_host.hpp" // kmm_seq_index_build behind bi_build_device and check_k

template <int MODE>
int launch_read_hits(kmm_index *ix, const ReadsView &rv, int k, int max_freq, int also_rc, const int64_t *tile_first_read,
                     uint32_t *hits, uint32_t *windows)
{
    const int64_t n_tiles = (rv.total + TILE_T - 1) / TILE_T;
    const IndexView iv = view_of(ix);
    const dim3 grid((unsigned)grid_for_tiles(ix, n_tiles));
    with_probe_flavour(iv, [&](auto probe) {
        hipLaunchKernelGGL((k_read_hits<TILE_S, MODE, decltype(probe)::value>), grid, dim3(256), 0, ix->stream, rv, iv, k,
                           max_freq, also_rc, n_tiles, tile_first_read, hits, windows);
    });
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

// Flat reads in front of k_read_hits's front end: what kmm_read_hits and kmm_read_nodes (kmm_read_nodes_host.hpp) share.
// The ReadsView is prepared as map_reads_common prepares it (staging, lookup table, the uniform front end for reads of 16
// bases and more without breaks, else the read-start bitset and k_mark_breaks), with two differences: the bad-byte and
// bad-offset words are the call's own (in the stage's aux buffer, never ix->first_bad), and reads of one length that take
// the ragged front end get no offsets array: their starts and their read ids are arithmetic.
struct FlatReads {
    Stage *s = nullptr;
    ReadsView rv;
    bool uniform = false, uniform_kernel = false, has_break = false, staged = false;
    int64_t total = 0, n_tiles = 0;
    unsigned long long *d_bad = nullptr;  // aux [0, 256): the call's three error words
    const int64_t *tile_first = nullptr;  // ragged reads: the first read of every tile (k_rh_tile_reads)
};

// The number of base bytes, and what is wrong with the arguments that say it.
int flat_reads_total(const char *who, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len,
                     int64_t *out)
{
    int64_t total = 0;
    if (!read_offsets) {
        if (read_len > 0 && n_reads > INT64_MAX / read_len)
            return fail(KMM_ERR_INVALID_ARG, "%s: n_reads * read_len overflows", who);
        total = n_reads * read_len;
    } else {
        int64_t ends[2] = {0, 0};
        if (is_device_ptr(read_offsets)) {
            HIPCHK(hipMemcpy(&ends[0], read_offsets, 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(&ends[1], read_offsets + n_reads, 8, hipMemcpyDeviceToHost));
        } else {
            ends[0] = read_offsets[0];
            ends[1] = read_offsets[n_reads];
        }
        if (ends[0] != 0)
            return fail(KMM_ERR_INVALID_ARG, "%s: read_offsets[0] must be 0 (got %lld)", who, (long long)ends[0]);
        if (ends[1] < 0)
            return fail(KMM_ERR_INVALID_ARG, "%s: read_offsets[n_reads] negative", who);
        total = ends[1];
    }
    if (total > 0 && !bases)
        return fail(KMM_ERR_INVALID_ARG, "%s: bases is NULL", who);
    *out = total;
    return KMM_OK;
}

// total > 0.  Takes the next stage, stages what lies in host memory, builds the view and makes room: aux holds the error words
// and aux_bytes more behind them (at (uint8_t *)fr.d_bad + 256: the caller's).  On return the copies are ordered before the
// handle's stream and the error words are NO_BAD there.
int flat_reads_stage(kmm_index *ix, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len,
                     int64_t total, const uint8_t *lut, size_t aux_bytes, FlatReads &fr)
{
    fr.uniform = read_offsets == nullptr;
    fr.total = total;
    KMMCHK(ensure_direct(ix));
    Stage &s = next_stage(ix);
    fr.s = &s;
    KMMCHK(stage_acquire(ix, s));
    ReadsView &rv = fr.rv;
    memset(&rv, 0, sizeof rv);
    KMMCHK(stage_in<uint8_t>(ix, s.bases, bases, (size_t)total, &rv.bases, &fr.staged));
    KMMCHK(resolve_lut(ix, s, lut, &rv.lut, &fr.staged, &fr.has_break));
    if (!fr.uniform)
        KMMCHK(stage_in<int64_t>(ix, s.offsets, read_offsets, (size_t)(n_reads + 1), &rv.offsets, &fr.staged));
    rv.total = total;
    rv.n_reads = n_reads;
    if (fr.uniform) {
        rv.read_len = (uint64_t)read_len;
        rv.read_len_magic = magic_for((uint64_t)read_len);
    }
    fr.n_tiles = (total + TILE_T - 1) / TILE_T;
    KMMCHK(ensure(s.aux, 256 + aux_bytes));
    fr.d_bad = (unsigned long long *)s.aux.p;
    rv.first_bad = fr.d_bad;
    fr.uniform_kernel = fr.uniform && read_len >= 16 && !fr.has_break;
    if (!fr.uniform_kernel) {
        rv.n_start_words = total / 32 + 2;
        KMMCHK(ensure(s.start_bits, (size_t)rv.n_start_words * 4));
        rv.start_bits = (const uint32_t *)s.start_bits.p;
    }
    if (!fr.uniform) {
        KMMCHK(ensure(s.tile_first, (size_t)(fr.n_tiles + 1) * 8));
        fr.tile_first = (const int64_t *)s.tile_first.p;
    }
    KMMCHK(stage_copies_done(ix));
    HIPCHK(hipMemsetAsync(fr.d_bad, 0xFF, 3 * sizeof(unsigned long long), ix->stream));
    return KMM_OK;
}

// What the ragged front end reads (nothing for fr.uniform_kernel): read starts and break bytes into the bitset, the offsets
// checked, the first read of every tile.
int flat_reads_mark(kmm_index *ix, const FlatReads &fr)
{
    if (fr.uniform_kernel)
        return KMM_OK;
    const ReadsView &rv = fr.rv;
    uint32_t *bits = (uint32_t *)fr.s->start_bits.p;
    HIPCHK(hipMemsetAsync(bits, 0, (size_t)rv.n_start_words * 4, ix->stream));
    if (fr.uniform)
        hipLaunchKernelGGL(k_mark_uniform_starts, dim3(grid_for(ix, (rv.n_reads + 256) / 256, 8)), dim3(256), 0, ix->stream,
                           rv.n_reads, (int64_t)rv.read_len, bits);
    else
        hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(ix, (rv.n_reads + 256) / 256, 8)), dim3(256), 0, ix->stream,
                           rv.offsets, rv.n_reads, fr.total, bits);
    if (fr.has_break) // every break byte: a one-base read
        hipLaunchKernelGGL(k_mark_breaks, dim3(grid_for(ix, (fr.total + 256 * 16 * MARK_U - 1) / (256 * 16 * MARK_U), 8)), dim3(256), 0,
                           ix->stream, rv.bases, fr.total, rv.lut, bits);
    if (!fr.uniform) {
        hipLaunchKernelGGL(k_check_offsets, dim3(grid_for(ix, (rv.n_reads + 255) / 256, 8)), dim3(256), 0, ix->stream,
                           rv.offsets, rv.n_reads, fr.d_bad);
        hipLaunchKernelGGL(k_rh_tile_reads, dim3(grid_for(ix, (fr.n_tiles + 256) / 256, 8)), dim3(256), 0, ix->stream,
                           rv.offsets, rv.n_reads, fr.total, fr.n_tiles, (int64_t)TILE_T, (int64_t *)fr.s->tile_first.p);
    }
    HIPCHK(hipGetLastError());
    return KMM_OK;
}

// errors of this call are this call's: nothing is left on the handle
int flat_reads_errors(const char *who, const unsigned long long (&bad)[3])
{
    if (bad[2] != NO_BAD)
        return fail(KMM_ERR_INVALID_ARG, "%s: read_offsets is not non-decreasing at read %llu", who, bad[2]);
    if (bad[0] != NO_BAD)
        return fail(KMM_ERR_INVALID_BASE, "%s: read byte at offset %llu is not a nucleotide under the lookup table "
                    "(the reference's DNA encoder raises here)", who, bad[0]);
    return KMM_OK;
}

int read_hits_impl(kmm_index *ix, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len, int k,
                   int max_freq, int also_revcomp, const uint8_t *lut, uint32_t *hits, uint32_t *windows)
{
    HIPCHK(hipSetDevice(ix->device));
    int64_t total = 0;
    KMMCHK(flat_reads_total("kmm_read_hits", bases, read_offsets, n_reads, read_len, &total));
    const bool hits_dev = is_device_ptr(hits), win_dev = windows && is_device_ptr(windows);
    const size_t out_bytes = (size_t)n_reads * 4;
    if (total == 0) { // nothing to look up: the outputs are written in full all the same
        hipError_t e = hits_dev ? hipMemsetAsync(hits, 0, out_bytes, ix->stream) : (memset(hits, 0, out_bytes), hipSuccess);
        if (e == hipSuccess && windows)
            e = win_dev ? hipMemsetAsync(windows, 0, out_bytes, ix->stream) : (memset(windows, 0, out_bytes), hipSuccess);
        if (e == hipSuccess)
            e = hipStreamSynchronize(ix->stream);
        if (e != hipSuccess)
            return fail(KMM_ERR_HIP, "kmm_read_hits: %s", hipGetErrorString(e));
        ix->read_hits_calls++;
        return KMM_OK;
    }
    // aux behind the error words: the outputs of a caller that gave host arrays
    const size_t out_slot = (out_bytes + 255) & ~(size_t)255;
    FlatReads fr;
    KMMCHK(flat_reads_stage(ix, bases, read_offsets, n_reads, read_len, total, lut, 2 * out_slot, fr));
    uint8_t *aux = (uint8_t *)fr.d_bad + 256;
    uint32_t *d_hits = hits_dev ? hits : (uint32_t *)aux;
    uint32_t *d_win = !windows ? nullptr : (win_dev ? windows : (uint32_t *)(aux + out_slot));
    HIPCHK(hipMemsetAsync(d_hits, 0, out_bytes, ix->stream));
    if (d_win)
        HIPCHK(hipMemsetAsync(d_win, 0, out_bytes, ix->stream));
    const int rc_flag = also_revcomp ? 1 : 0;
    KMMCHK(flat_reads_mark(ix, fr));
    if (fr.uniform_kernel)
        KMMCHK(launch_read_hits<MODE_UNIFORM>(ix, fr.rv, k, max_freq, rc_flag, nullptr, d_hits, d_win));
    else
        KMMCHK(launch_read_hits<MODE_GENERAL>(ix, fr.rv, k, max_freq, rc_flag, fr.tile_first, d_hits, d_win));
    unsigned long long bad[3] = {NO_BAD, NO_BAD, NO_BAD};
    hipError_t e = hipMemcpyAsync(bad, fr.d_bad, sizeof bad, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess && !hits_dev)
        e = hipMemcpyAsync(hits, d_hits, out_bytes, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess && windows && !win_dev)
        e = hipMemcpyAsync(windows, d_win, out_bytes, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess)
        return fail(KMM_ERR_HIP, "kmm_read_hits: %s", hipGetErrorString(e));
    KMMCHK(stage_release(ix, *fr.s, fr.staged));
    KMMCHK(flat_reads_errors("kmm_read_hits", bad));
    ix->read_hits_calls++;
    return KMM_OK;
}

#include "kmm_read_nodes_host.hpp" // kmm_read_nodes behind the flat-reads helpers

// ---- the record-hits queue
// Room for n more entries behind the pending ones, zeroed on the handle's stream; *hits / *windows: the first new entry.  The
// arrays grow here, before the probe kernel is launched (a piece's record count is known from its census): a new pair, the
// pending entries copied to its start.  The caller adds n to rhq_pending once its kernel is launched.
// even (the pair forms of the keep kernels load a pair's two entries as 8 bytes): the first new entry lies at an even index
// of the arrays — where a take of an odd number of entries has left it at an odd one, the pending entries move.
int rhq_reserve(kmm_index *ix, int64_t n, uint32_t **hits, uint32_t **windows, bool even = false)
{
    if (ix->rhq_pending == 0)
        ix->rhq_head = 0;
    const bool odd = even && ((ix->rhq_head + ix->rhq_pending) & 1) != 0;
    if (odd || ix->rhq_head + ix->rhq_pending + n > ix->rhq_cap) {
        int64_t cap = 2 * (ix->rhq_pending + n) + 2;
        if (cap < (1 << 16))
            cap = 1 << 16;
        const int64_t head = even ? (ix->rhq_pending & 1) : 0;
        DevBuf nh, nw;
        KMMCHK(ensure(nh, (size_t)cap * 4));
        KMMCHK(ensure(nw, (size_t)cap * 4));
        if (ix->rhq_pending > 0) {
            const size_t bytes = (size_t)ix->rhq_pending * 4;
            HIPCHK(hipMemcpyAsync((uint32_t *)nh.p + head, (const uint32_t *)ix->rhq_hits.p + ix->rhq_head, bytes, hipMemcpyDeviceToDevice,
                                  ix->stream));
            HIPCHK(hipMemcpyAsync((uint32_t *)nw.p + head, (const uint32_t *)ix->rhq_win.p + ix->rhq_head, bytes, hipMemcpyDeviceToDevice,
                                  ix->stream));
        }
        HIPCHK(hipStreamSynchronize(ix->stream)); // (the old pair is freed below)
        ix->rhq_hits = std::move(nh);
        ix->rhq_win = std::move(nw);
        ix->rhq_head = head;
        ix->rhq_cap = cap;
    }
    *hits = (uint32_t *)ix->rhq_hits.p + ix->rhq_head + ix->rhq_pending;
    *windows = (uint32_t *)ix->rhq_win.p + ix->rhq_head + ix->rhq_pending;
    if (n > 0) {
        HIPCHK(hipMemsetAsync(*hits, 0, (size_t)n * 4, ix->stream));
        HIPCHK(hipMemsetAsync(*windows, 0, (size_t)n * 4, ix->stream));
    }
    return KMM_OK;
}

// The map calls without records have kmm_read_hits: refused while the mode is on, nothing mapped.
int refuse_in_record_hits(const kmm_index *ix, const char *who)
{
    if (ix && ix->record_hits)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_hits\" is %d: the mode serves the record calls (kmm_map_records, kmm_map_bgzf, "
                    "kmm_map_gzip, kmm_map_bam); reads held as flat arrays have kmm_read_hits (nothing is mapped)", who, ix->record_hits);
    return KMM_OK;
}

// A record call while the mode is on and "min_base_quality" is set: refused, nothing mapped (that mask lives in the
// compaction and the radix front end, which the mode never takes; the mode's own floor is "record_hits_min_base_quality",
// call_floor).
int refuse_quality_in_record_hits(const kmm_index *ix, const char *who)
{
    if (ix && ix->record_hits && ix->min_base_quality > 0)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_hits\" is %d and min_base_quality is %d: the record-hits mode applies no "
                    "quality floor (nothing is mapped)", who, ix->record_hits, ix->min_base_quality);
    return KMM_OK;
}

// ---- the record-keep queue
// What a record call is refused for while "record_keep" is 1 (nothing is mapped, nothing appended).  sam_or_bam: the call decodes
// SAM or BAM records, whose text on the device is ">\n" SEQ: the read's name is not carried — unless the call is kmm_map_bam with
// "record_names" 1 (named), whose decode carries it.
// multiline: the call unwraps multi-line FASTA.  With "record_pairs" 1 as well only the routes whose pieces can
// end behind a mate 2 are served: FASTQ and two-line FASTA text.
int refuse_record_keep(const kmm_index *ix, const char *who, bool sam_or_bam, bool named = false, bool multiline = false)
{
    if (!ix || !ix->record_keep)
        return KMM_OK;
    if (!ix->record_hits)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_keep\" is 1 and \"record_hits\" is 0: the keep rule reads the entries of the "
                    "record-hits mode, set it to 1 or 2 (nothing is mapped)", who);
    if (ix->rk_min_permille > 0 && ix->record_hits != 2)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_keep_min_permille\" is %d and \"record_hits\" is 1: the rule needs the windows, "
                    "which mode 2 keeps (nothing is mapped)", who, ix->rk_min_permille);
    if (sam_or_bam && !named)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_keep\" is 1: SAM and BAM records are decoded to \">\\n\" SEQ without the read's "
                    "name (QNAME is not carried), their text would be useless (nothing is mapped)", who);
    if (ix->record_pairs && sam_or_bam)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_keep\" and \"record_pairs\" are 1: the decode of SAM and BAM records hands over "
                    "whole windows, not pair-aligned ones; mates are kept together on FASTQ and two-line FASTA text only (nothing is "
                    "mapped)", who);
    if (ix->record_pairs && multiline)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_keep\" and \"record_pairs\" are 1: the unwrap of multi-line FASTA cuts at header "
                    "lines, not behind a mate 2; mates are kept together on FASTQ and two-line FASTA text only (nothing is mapped)", who);
    return KMM_OK;
}

// What a KMM_FORMAT_SAM call is refused for while "record_sam" is 1 or 2 (nothing is mapped, nothing appended).  A
// call that passes is `named` to refuse_record_keep: what it appends is the records' own lines, QNAME and all.
int refuse_record_sam(const kmm_index *ix, const char *who)
{
    if (!ix->record_hits || !ix->record_keep)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_sam\" is %d and \"%s\" is 0: the kept records' own lines are appended under the "
                    "keep rule, which reads the entries of the record-hits mode; set \"record_hits\" to 1 or 2 and \"record_keep\" to 1, "
                    "or \"record_sam\" to 0 (nothing is mapped)", who, ix->record_sam, ix->record_hits ? "record_keep" : "record_hits");
    if (ix->record_pairs)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_sam\" is %d and \"record_pairs\" is 1: mates are not kept together in SAM output; "
                    "set one of them to 0 (nothing is mapped)", who, ix->record_sam);
    return KMM_OK;
}

// "record_sam" under the floor of the record-hits mode: refused, nothing mapped — the span-leaving decode of that
// form has no quality variant, so there are no quality lines for the mark pass to read.
int refuse_floor_with_record_sam(const kmm_index *ix, const char *who)
{
    if (ix->record_hits && ix->rh_min_base_quality > 0)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_sam\" is %d and record_hits_min_base_quality is %d: SAM lines kept as SAM lines are "
                    "mapped without their QUAL column; set the floor to 0, or \"record_sam\" to 0 (nothing is mapped)", who,
                    ix->record_sam, ix->rh_min_base_quality);
    return KMM_OK;
}

// Does a KMM_FORMAT_SAM call append the kept records' own lines ("record_sam")?
bool sam_raw_on(const kmm_index *ix)
{
    return ix->record_sam && ix->record_hits && ix->record_keep;
}

// Are the selected records of a SAM stream taken as mates whose lines are kept together ("record_sam_mates")?
bool sam_raw_mates_on(const kmm_index *ix)
{
    return ix->record_sam_mates && sam_raw_on(ix);
}

// The waiting mate 1 of a SAM stream and the stream's pair ordinal are dropped (a new stream, emptied queues, a changed form).
void sam_mates_drop(kmm_index *ix)
{
    ix->sam_mate_len = ix->sam_mate_line_len = ix->sam_pairs_done = 0;
    ix->sam_mate_saved = false;
}

// Are the records of a FASTQ / two-line FASTA stream taken as interleaved mates?
bool record_pairs_on(const kmm_index *ix)
{
    return ix->record_hits && ix->record_keep && (ix->record_pairs || ix->rk_mates_call);
}

// Are the selected records of a kmm_map_bam stream taken as mates ("record_names_pairs")?
bool bam_mates_on(const kmm_index *ix)
{
    return ix->record_names_pairs && ix->record_names && ix->record_hits && ix->record_keep;
}

// Are they taken as mates whose own bytes are kept ("record_bam_mates")?
bool bam_raw_mates_on(const kmm_index *ix)
{
    return ix->record_bam_mates && ix->record_bam && ix->record_hits && ix->record_keep;
}

// The mate check of one piece of kmm_map_bam's inner records call: *bad is the first pair of the piece (its ordinal inside the
// piece) whose two names differ, 0xFFFFFFFF when all agree.  One small read-back per piece, behind everything the piece queued.
int pair_names_piece(kmm_index *ix, const ReadsView &rv, int64_t consumed, uint32_t *bad)
{
    const int64_t n_tiles = (consumed + 1023) / 1024;
    KMMCHK(ensure(ix->rk_names_ctl, 64));
    uint32_t *d_bad = (uint32_t *)ix->rk_names_ctl.p;
    HIPCHK(hipMemsetAsync(d_bad, 0xFF, 4, ix->stream));
    hipLaunchKernelGGL(k_rk_pair_names, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, ix->stream, rv.bases, consumed, n_tiles,
                       (const uint32_t *)rv.tile_nl, (const uint32_t *)rv.super_nl, ix->record_names_mate_suffix ? 1u : 0u, d_bad);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(bad, d_bad, 4, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream));
    return KMM_OK;
}

// Room for n more bytes behind q.bound pending ones, made before a piece's kernels are launched (n: its consumed bytes, more
// than it can keep); the control words on first use.  A new queue gets the pending bytes on the handle's stream.
int rkq_reserve(kmm_index *ix, kmm_index::RkQueue &q, int64_t n)
{
    if (!q.ctl.p) {
        KMMCHK(ensure(q.ctl, 64));
        HIPCHK(hipMemsetAsync(q.ctl.p, 0, 64, ix->stream));
    }
    if (q.bound + n > q.cap) {
        int64_t cap = 2 * (q.bound + n);
        if (cap < (1 << 20))
            cap = 1 << 20;
        DevBuf nb;
        KMMCHK(ensure(nb, (size_t)cap + 16));
        if (q.bound > 0)
            HIPCHK(hipMemcpyAsync(nb.p, q.text.p, (size_t)q.bound, hipMemcpyDeviceToDevice, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream)); // (the old queue is freed below)
        q.text = std::move(nb);
        q.cap = cap;
    }
    return KMM_OK;
}

// A queue's tail as a call finds it, kept on the device behind the tail itself, and put back by a call that fails.
int rkq_mark(kmm_index *ix, kmm_index::RkQueue &q)
{
    KMMCHK(rkq_reserve(ix, q, 0));
    HIPCHK(hipMemcpyAsync((uint8_t *)q.ctl.p + 16, q.ctl.p, 16, hipMemcpyDeviceToDevice, ix->stream));
    return KMM_OK;
}

void rkq_rollback(kmm_index *ix, kmm_index::RkQueue &q, int64_t bound0)
{
    const std::string msg = g_err; // (the failure's message, not the copy's)
    if (q.ctl.p && hipMemcpyAsync(q.ctl.p, (const uint8_t *)q.ctl.p + 16, 16, hipMemcpyDeviceToDevice, ix->stream) != hipSuccess)
        (void)hipGetLastError();
    q.bound = bound0;
    g_err = msg;
}

// Both queues back to what the last kmm_map_records found (rk_snap), once: for an outer call that fails behind a good inner one.
void rk_snap_restore(kmm_index *ix)
{
    if (ix->rk_snap.valid) {
        ix->rhq_pending = ix->rk_snap.pending;
        rkq_rollback(ix, ix->rkq[0], ix->rk_snap.bound);
    }
    ix->rk_snap.valid = false;
}

// rk_mates_call / rk_raw_call around one inner records call of kmm_map_bam or of a SAM piece: cleared on every way out.
struct RkCallMode {
    kmm_index *ix;
    RkCallMode(kmm_index *ix_, bool mates, bool raw) : ix(ix_) { ix->rk_mates_call = mates, ix->rk_raw_call = raw; }
    ~RkCallMode() { ix->rk_mates_call = ix->rk_raw_call = false; }
};

// The keep rule of the handle, for single records and for pairs.
RkRule rk_rule(const kmm_index *ix) { return {(uint32_t)ix->rk_min_hits, (uint32_t)ix->rk_min_permille, (uint32_t)ix->rk_invert}; }
RkPairRule rk_pair_rule(const kmm_index *ix) { return {rk_rule(ix), (uint32_t)ix->rk_pair_rule}; }

// The entries an inner records call has just appended: the last n of the entry queue.  Null pointers when n is 0 (the kernels
// then read none), a null `windows` in mode 1.  false: fewer than n entries are pending (the caller's internal error).
struct KeepEntries { const uint32_t *hits = nullptr, *windows = nullptr; uint64_t n = 0; };

bool keep_entries_last(const kmm_index *ix, uint64_t n, KeepEntries &e)
{
    const int64_t first = ix->rhq_head + ix->rhq_pending - (int64_t)n;
    if (first < 0)
        return false;
    e.n = n;
    e.hits = n ? (const uint32_t *)ix->rhq_hits.p + first : nullptr;
    e.windows = n && ix->record_hits == 2 ? (const uint32_t *)ix->rhq_win.p + first : nullptr;
    return true;
}

// The kept records of one piece, behind its k_read_hits (the entries are sums of atomics over that whole grid: complete only
// when it has ended).  hits / windows: the piece's n_records entries (windows null in mode 1); consumed: where its last whole
// record ends.
// PAIR (kmm_record_keep.hpp): 0: one entry per record; else the entries are those of the piece's pairs, two per pair, the first
// at an even index of the queue's arrays; 1: record r of this buffer is pair r (kmm_map_record_pairs), 2: records 2p and
// 2p + 1 are pair p (interleaved).  q: the queue the text goes to.
template <int PAIR>
int record_keep_piece(kmm_index *ix, kmm_index::RkQueue &q, const ReadsView &rv, int64_t n_bytes, int64_t consumed, int64_t n_records,
                      const uint32_t *hits, const uint32_t *windows)
{
    const int64_t n_tiles = (consumed + 1023) / 1024;
    const int n_super = (int)((n_tiles + 1023) / 1024);
    KMMCHK(ensure(ix->rk_tile, (size_t)n_super * 1024 * 8));
    KMMCHK(ensure(ix->rk_super, (size_t)n_super * 8 + 64));
    KMMCHK(rkq_reserve(ix, q, consumed));
    // (kept bytes per tile and super-tile, and behind them the kept records)
    uint32_t *tile_cnt = (uint32_t *)ix->rk_tile.p, *super_tot = (uint32_t *)ix->rk_super.p;
    uint32_t *tile_rec = tile_cnt + (size_t)n_super * 1024, *super_rec = super_tot + n_super;
    unsigned long long *tail = (unsigned long long *)q.ctl.p;
    uint32_t *d_total = (uint32_t *)((uint8_t *)q.ctl.p + 32);
    typename RkRuleOf<PAIR>::type rule;
    if constexpr (PAIR == 0)
        rule = rk_rule(ix);
    else
        rule = rk_pair_rule(ix);
    const dim3 g4((unsigned)((n_tiles + 3) / 4));
    HIPCHK(hipMemsetAsync(tile_cnt, 0, (size_t)n_super * 1024 * 8, ix->stream));
    hipLaunchKernelGGL(k_rk_flags<PAIR>, g4, dim3(256), 0, ix->stream, rv.bases, n_bytes, consumed, n_tiles, rv.tile_nl, rv.super_nl,
                       rv.period_mask, hits, windows, n_records, rule, tile_cnt, tile_rec);
    hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, ix->stream, tile_cnt, super_tot);
    hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, ix->stream, super_tot, n_super, d_total);
    hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, ix->stream, tile_rec, super_rec);
    hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, ix->stream, super_rec, n_super, d_total + 1);
    hipLaunchKernelGGL(k_rk_scatter<PAIR>, g4, dim3(256), 0, ix->stream, rv.bases, n_bytes, consumed, n_tiles, rv.tile_nl, rv.super_nl,
                       rv.period_mask, hits, windows, n_records, rule, (const uint32_t *)tile_cnt, (const uint32_t *)super_tot,
                       (const unsigned long long *)tail, (uint8_t *)q.text.p);
    hipLaunchKernelGGL(k_rk_advance, dim3(1), dim3(64), 0, ix->stream, tail, (const uint32_t *)d_total);
    HIPCHK(hipGetLastError());
    q.bound += consumed;
    return KMM_OK;
}

// The queue's true tail {bytes, records}, behind the caller's synchronisation.
int rkq_tail(const kmm_index::RkQueue &q, unsigned long long (&tail)[2])
{
    tail[0] = tail[1] = 0;
    if (q.ctl.p)
        HIPCHK(hipMemcpy(tail, q.ctl.p, 16, hipMemcpyDeviceToHost));
    return KMM_OK;
}

} // namespace

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

const char *kmm_version(void) { return "kmm 0.3.0 (gfx950)"; }

const char *kmm_last_error(void) { return g_err.c_str(); }

int kmm_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0)
        return fail(KMM_ERR_INVALID_ARG, "out is NULL or bytes is 0");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *out = nullptr;
        return fail(e == hipErrorOutOfMemory ? KMM_ERR_NOMEM : KMM_ERR_HIP, "hipHostMalloc(%zu bytes) -> %s", bytes,
                    hipGetErrorString(e));
    }
    return KMM_OK;
}

int kmm_host_reserve(int64_t raw_batch_bytes)
{
    if (raw_batch_bytes < 0)
        return fail(KMM_ERR_INVALID_ARG, "raw_batch_bytes negative");
    // the two page-locked buffers a host-packed batch of that many raw bytes needs (map_records_host_packed / map_reads_host_packed)
    const size_t n = (size_t)raw_batch_bytes;
    const size_t want[2] = {(n / 4 + 1024 + 63) & ~(size_t)63, (n / 8 + 256 + 63) & ~(size_t)63};
    for (size_t w : want) {
        uint8_t *p = nullptr;
        const size_t take = w + w / 8;
        if (hipHostMalloc(reinterpret_cast<void **>(&p), take, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return fail(KMM_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed", take);
        }
        g_shelf.give(p, take);
    }
    return KMM_OK;
}

int kmm_host_reserve_buffer(int64_t bytes)
{
    if (bytes < 0)
        return fail(KMM_ERR_INVALID_ARG, "bytes negative");
    if (bytes == 0)
        return KMM_OK;
    uint8_t *p = nullptr;
    const size_t take = ((size_t)bytes + 4095) & ~(size_t)4095;
    if (hipHostMalloc(reinterpret_cast<void **>(&p), take, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KMM_ERR_NOMEM, "hipHostMalloc(%zu bytes) failed", take);
    }
    g_shelf.give(p, take);
    return KMM_OK;
}

int kmm_host_free(void *p)
{
    if (p)
        HIPCHK(hipHostFree(p));
    return KMM_OK;
}

int kmm_device_count(int *n_devices)
{
    if (!n_devices)
        return fail(KMM_ERR_INVALID_ARG, "n_devices is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        n = 0;
    }
    *n_devices = n;
    return KMM_OK;
}

int kmm_device_pci_bus_id(int device, char *out, int out_bytes)
{
    if (!out || out_bytes < 16)
        return fail(KMM_ERR_INVALID_ARG, "out is NULL or shorter than 16 bytes");
    out[0] = 0;
    HIPCHK(hipDeviceGetPCIBusId(out, out_bytes, device));
    return KMM_OK;
}

void kmm_index_destroy(kmm_index_t *ix)
{
    if (!ix)
        return;
    (void)hipSetDevice(ix->device);
    if (ix->stream)
        (void)hipStreamSynchronize(ix->stream);
    if (ix->copy_stream)
        (void)hipStreamSynchronize(ix->copy_stream);
    ix->pack_pool.reset(); // (its threads are joined before their page-locked buffers go back to the shelf)
    if (ix->comm && g_rccl.lib)
        (void)g_rccl.CommDestroy(ix->comm);
    delete ix; // every buffer, event and stream of the handle frees itself; the streams go last
}


static bool ensure_ring(kmm_index_t *ix);

static int index_create_impl(kmm_index *ix, const int32_t *h2i, const int32_t *nk,
                             const uint64_t *kmers, const int32_t *nodes, const uint16_t *freqs)
{
    const uint64_t M = ix->modulo;
    const int64_t N = ix->n_entries;
    HIPCHK(hipSetDevice(ix->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ix->device));
    ix->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIPCHK(hipStreamCreateWithFlags(ix->stream.put(), hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(ix->copy_stream.put(), hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(ix->copied.put(), hipEventDisableTiming));
    for (Stage &s : ix->stage)
        HIPCHK(hipEventCreateWithFlags(s.done.put(), hipEventDisableTiming));

    // layout: small indexes get 16-byte buckets + the L2 occupancy bitmap, larger ones 32-byte buckets
    size_t occ_max = KMM_OCC_MAX_BYTES;
    if (const char *env = getenv("KMM_OCC_MAX_BYTES")) // experiments: threshold of the bitmap prefilter
        occ_max = (size_t)strtoull(env, nullptr, 10);
    // bits per bucket: as many (1, 2, 4 or 8) as keep the bitmap within KMM_OCC_SWEET_BYTES — an entry sets
    // the bit chosen by its k-mer's fingerprint, so every doubling halves the false-positive passes of
    // single-entry buckets (10 M-k-mer index: 1 bit 19.7 ms, 2 bits 18.1 ms, 4 bits (10 MB) 21.5 ms per step)
    // (2.5 M: 4 bits/2.5 MB 14.5 ms, 8 bits/5 MB 15.3 ms; 5 M: 2 bits 16.1, 4 bits/5 MB 16.3, 8 bits/10 MB 20.6;
    //  15 M: 1 bit/3.75 MB 20.4, 2 bits/7.5 MB 21.3): the second bit is worth up to 5 MiB, further bits 3 MiB
    int occ_shift = 0;
    while (occ_shift < 3 &&
           ((M << (occ_shift + 1)) + 7) / 8 <= (occ_shift == 0 ? KMM_OCC_SWEET_BYTES : KMM_OCC_SWEET_BYTES * 3 / 5))
        occ_shift++;
    if (const char *env = getenv("KMM_OCC_SHIFT")) // experiments: force 2^shift bitmap bits per bucket
        occ_shift = atoi(env) < 0 ? 0 : (atoi(env) > 3 ? 3 : atoi(env));
    size_t occ_bytes = (size_t)(((M << occ_shift) + 31) / 32) * 4;
    const bool with_occ = (size_t)((M + 31) / 32) * 4 <= occ_max || occ_bytes <= occ_max;
    // Up to ~13 M entries a word-blocked Bloom filter (two bits per key inside one 32-bit word, chosen by a
    // hash of the k-mer alone) of at most 4 MiB beats the per-bucket bitmap: 10 M entries, ms per step:
    // bitmap 2 bits/bucket (5 MB) 18.0; Bloom 2.5 MB 19.6, 4 MB 16.7, 5 MB 17.0, 6.5 MB 18.1.  13 M: Bloom 4 MiB 18.3,
    // bitmap 19.5; 16 M: Bloom 6 MiB 19.9, bitmap 20.5; 20 M and 30 M: equal.
    int64_t bloom_max_entries = KMM_BLOOM_MAX_ENTRIES;
    if (const char *env = getenv("KMM_BLOOM_MAX_ENTRIES")) // experiments
        bloom_max_entries = strtoll(env, nullptr, 10);
    if (with_occ && N <= bloom_max_entries) {
        size_t bb = (size_t)N * 2;             // 16 bits per key is plenty
        const size_t cap = N <= 13000000 ? KMM_BLOOM_MAX_BYTES : KMM_BLOOM_MAX_BYTES * 3 / 2; // 13-20 M: 6 MiB
        if (bb > cap) bb = cap;
        if (bb < 64) bb = 64;
        if (const char *env = getenv("KMM_BLOOM_BYTES")) // experiments: filter size; 0 = per-bucket bitmap
            bb = (size_t)strtoull(env, nullptr, 10);
        if (bb >= 4) {
            ix->bloom_words = (uint32_t)(bb / 4);
            occ_bytes = (size_t)ix->bloom_words * 4;
        }
    }
    ix->occ_shift = occ_shift;
    ix->wide = !with_occ;
    if (const char *env = getenv("KMM_WIDE_BUCKETS")) // experiments: force the bucket layout (0 / 1)
        ix->wide = atoi(env) != 0;
    HIPCHK(hipMalloc(ix->own_counts_buf.put(), sizeof(uint32_t) * (size_t)(ix->max_node_id + 1)));
    ix->counts = ix->own_counts_buf;
    HIPCHK(hipMemsetAsync(ix->counts, 0, sizeof(uint32_t) * (size_t)(ix->max_node_id + 1), ix->stream));
    HIPCHK(hipMalloc(ix->lut_default.put(), 256));
    HIPCHK(hipMalloc(ix->first_bad.put(), 3 * sizeof(unsigned long long)));
    HIPCHK(hipMalloc(ix->queue.put(), 4 * sizeof(unsigned long long))); // (a tile queue head; also the result cells of small reductions)
    HIPCHK(hipMalloc(ix->stats.put(), KMM_STAT_BYTES));
    HIPCHK(hipMemset(ix->stats, 0, KMM_STAT_BYTES));
    uint8_t lut[256];
    default_lut(lut);
    HIPCHK(hipMemcpy(ix->lut_default, lut, 256, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(ix->lut_codes.put(), 256));
    memset(lut, 0xFF, sizeof lut);
    lut[0] = 0; lut[1] = 1; lut[2] = 2; lut[3] = 3;
    HIPCHK(hipMemcpy(ix->lut_codes, lut, 256, hipMemcpyHostToDevice));
    unsigned long long nb[3] = {NO_BAD, NO_BAD, NO_BAD};
    HIPCHK(hipMemcpy(ix->first_bad, nb, sizeof nb, hipMemcpyHostToDevice));
    {   // host packing of reads that arrive in host memory: on by default with the reference CLI's worker count
        // (-t 16, command_line_interface.py:168) where the process has the cores for it — with fewer than 8 the plain
        // copy over PCIe is the faster way
        const int budget = kmm_hostpack::cpu_budget();
        ix->host_pack_threads = budget >= 8 ? (budget < 16 ? budget : 16) : 0;
        if (const char *env = getenv("KMM_HOST_PACK_THREADS")) {
            const int v = atoi(env);
            ix->host_pack_threads = v < 0 ? 0 : (v > 256 ? 256 : v);
        }
    }

    // The page-locked staging ring (8 x 16 MiB: 7-10 ms to make) is made HERE for an index whose count vector will leave
    // through it (kmm_get_node_counts -> pageable memory; flat reads and BGZF windows come in through it): a one-shot
    // `kmer_mapper map` otherwise makes it inside its first fetch — 18 ms instead of 8 for configs[2]'s 400 MB vector
    // (profiles/r05/cli_populate_ab.txt).  Best effort: without it the first user makes it.
    if (ix->host_pack_threads > 0 && (size_t)(ix->max_node_id + 1) * 4 >= ((size_t)64 << 20))
        (void)ensure_ring(ix);

    // raw arrays -> HBM (temporary); validate, build the radix view, and the direct view now or on first use
    DevBuf d_h2i, d_nk, d_km, d_nd, d_fr, d_err;
    bool staged = false;
    const int32_t *p_h2i = nullptr, *p_nk = nullptr, *p_nd = nullptr;
    const uint64_t *p_km = nullptr;
    const uint16_t *p_fr = nullptr;
    int rc = KMM_OK;
    do {
        if ((rc = stage_in<int32_t>(ix, d_h2i, h2i, (size_t)M, &p_h2i, &staged))) break;
        if ((rc = stage_in<int32_t>(ix, d_nk, nk, (size_t)M, &p_nk, &staged))) break;
        if ((rc = stage_in<uint64_t>(ix, d_km, kmers, (size_t)N, &p_km, &staged))) break;
        if ((rc = stage_in<int32_t>(ix, d_nd, nodes, (size_t)N, &p_nd, &staged))) break;
        if ((rc = stage_in<uint16_t>(ix, d_fr, freqs, (size_t)N, &p_fr, &staged))) break;
        if ((rc = ensure(d_err, 4))) break;
    } while (0);
    if (rc == KMM_OK) {
        hipError_t e = hipMemsetAsync(d_err.p, 0, 4, ix->copy_stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ix->copy_stream);
        if (e != hipSuccess)
            rc = fail(KMM_ERR_HIP, "index upload: %s", hipGetErrorString(e));
    }
    uint32_t err = 0;
    if (rc == KMM_OK) { // what the reference never checks (mapper.pyx:17 disables bounds checks)
        hipLaunchKernelGGL(k_validate_index, dim3(grid_for(ix, (int64_t)((M + 255) / 256), 16)), dim3(256), 0, ix->stream,
                           p_h2i, p_nk, p_nd, M, N, ix->max_node_id, (uint32_t *)d_err.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(ix->stream);
        if (e == hipSuccess) e = hipMemcpy(&err, d_err.p, 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            rc = fail(KMM_ERR_HIP, "index validation: %s", hipGetErrorString(e));
    }
    if (rc == KMM_OK && !err)
        rc = rx_build(ix, p_h2i, p_nk, p_km, p_nd, p_fr);
    // HBM budget: an index whose direct view is large (a 10^9-k-mer index: 64 GB of wide buckets + 16 GB of entries
    // beside the 46 GB radix view) keeps only the radix view resident; the direct view is packed from it when the
    // first small batch (or kmm_in_index) needs it.  Small indexes pack both now.
    size_t eager_max = (size_t)16 << 30;
    if (const char *env = getenv("KMM_DIRECT_EAGER_BYTES")) // tests / experiments
        eager_max = (size_t)strtoull(env, nullptr, 10);
    ix->direct_bytes = sizeof(uint4) * ((size_t)M * (ix->wide ? 2 : 1) + (size_t)(N > 0 ? N : 1));
    if (rc == KMM_OK && !err) {
        ix->occ_bytes_plan = with_occ ? occ_bytes : 0;
        if (ix->rx_ok && ix->direct_bytes > eager_max) {
            ix->direct_deferred = true;
        } else {
            IdxRaw src;
            src.h2i = p_h2i; src.nk = p_nk; src.kmers = p_km; src.nodes = p_nd; src.freqs = p_fr;
            rc = direct_build(ix, src, N, with_occ ? occ_bytes : 0, (uint32_t *)d_err.p);
        }
    }
    if (rc != KMM_OK)
        return rc;
    if (err & 1u)
        return fail(KMM_ERR_INDEX, "index inconsistent: a non-empty bucket "
                    "(hashes_to_index[h], n_kmers[h]) reaches outside [0, n_entries=%lld)",
                    (long long)N);
    if (err & 2u)
        return fail(KMM_ERR_INDEX, "index inconsistent: a node id lies outside [0, max_node_id=%lld]",
                    (long long)ix->max_node_id);
    return KMM_OK;
}

int kmm_index_create(const int32_t *hashes_to_index, const int32_t *n_kmers, uint64_t modulo,
                     const uint64_t *kmers, const int32_t *nodes, const uint16_t *frequencies,
                     int64_t n_entries, int64_t max_node_id, int device, kmm_index_t **out)
{
    if (!out)
        return fail(KMM_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!hashes_to_index || !n_kmers)
        return fail(KMM_ERR_INVALID_ARG, "hashes_to_index / n_kmers is NULL");
    if (modulo < 1)
        return fail(KMM_ERR_INVALID_ARG, "modulo must be >= 1");
    if (n_entries < 0 || max_node_id < 0)
        return fail(KMM_ERR_INVALID_ARG, "n_entries=%lld / max_node_id=%lld negative",
                    (long long)n_entries, (long long)max_node_id);
    if (n_entries > 0 && (!kmers || !nodes || !frequencies))
        return fail(KMM_ERR_INVALID_ARG, "kmers / nodes / frequencies is NULL");
    if (n_entries > 0x7FFFFFFFll)
        return fail(KMM_ERR_INVALID_ARG, "n_entries exceeds the int32 bucket offsets of the index format");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(KMM_ERR_HIP, "no HIP device available (%s): libkmm has no CPU fallback",
                    e != hipSuccess ? hipGetErrorString(e) : "0 devices");
    }
    if (device < 0 || device >= ndev)
        return fail(KMM_ERR_INVALID_ARG, "device %d outside [0, %d)", device, ndev);
    kmm_index *ix = new kmm_index();
    ix->device = device;
    ix->modulo = modulo;
    ix->magic = magic_for(modulo);
    ix->n_entries = n_entries;
    ix->max_node_id = max_node_id;
    int rc = index_create_impl(ix, hashes_to_index, n_kmers, kmers, nodes, frequencies);
    if (rc != KMM_OK) {
        std::string keep = g_err;
        kmm_index_destroy(ix);
        g_err = keep;
        return rc;
    }
    *out = ix;
    return KMM_OK;
}

int kmm_reset_counts(kmm_index_t *ix)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipMemsetAsync(ix->counts, 0, sizeof(uint32_t) * (size_t)(ix->max_node_id + 1), ix->stream));
    if (ix->rx_ecnt && ix->ecnt_dirty)
        HIPCHK(hipMemsetAsync(ix->rx_ecnt, 0, sizeof(uint32_t) * (size_t)(ix->rx_S ? ix->rx_S : 1), ix->stream));
    if (ix->rx_ecnt_acc)
        HIPCHK(hipMemsetAsync(ix->rx_ecnt_acc, 0, sizeof(uint32_t) * (size_t)(ix->rx_S ? ix->rx_S : 1), ix->stream));
    ix->ecnt_dirty = false;
    ix->rhq_head = ix->rhq_pending = 0; // (the record-hits queue is emptied with the counts; its arrays stay)
    for (auto &q : ix->rkq) { // (and the queues of kept records)
        if (q.ctl.p)
            HIPCHK(hipMemsetAsync(q.ctl.p, 0, 16, ix->stream));
        q.bound = 0;
    }
    ix->rk_snap.valid = false;
    ix->bam_mate_len = ix->bam_pairs_done = 0; // (a mate 1 that waits for its mate belongs to the entries just dropped: DESIGN 4.23)
    ix->bam_raw_mate_len = 0;                  // (and so do its raw bytes: DESIGN 4.25)
    sam_mates_drop(ix);                        // (and the waiting mate 1 of a SAM stream: DESIGN 4.28)
    // ("record_name_bytes_replaced" counts bytes of the text that queue held: it restarts with it.  The named decode adds to the
    // first shard alone; the other statistics stay, as before, until kmm_get_stats(reset).)
    HIPCHK(hipMemsetAsync(ix->stats + KMM_STAT_REC_NAME_REPLACED, 0, sizeof(unsigned long long), ix->stream));
    // an error that the kernels of an earlier map call have found, or will find, and no synchronising call has reported yet
    // goes with that call's counts: left in place it would be reported against the counts of the calls AFTER this reset
    HIPCHK(hipMemsetAsync(ix->first_bad, 0xFF, 3 * sizeof(unsigned long long), ix->stream));
    if (ix->sticky_rc != KMM_OK) { // the error of a mapped chunk goes away together with its partial counts
        unsigned long long nb[3] = {NO_BAD, NO_BAD, NO_BAD};
        HIPCHK(hipStreamSynchronize(ix->stream));
        HIPCHK(hipMemcpy(ix->first_bad, nb, sizeof nb, hipMemcpyHostToDevice));
        if (ix->sticky_rc == KMM_ERR_INTERNAL) // the conservation counters restart with the counts
            HIPCHK(hipMemset(ix->stats, 0, KMM_STAT_BYTES));
        ix->sticky_rc = KMM_OK;
        ix->sticky_msg.clear();
    }
    return KMM_OK;
}

int kmm_bind_counts(kmm_index_t *ix, uint32_t *device_counts)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(rx_flush(ix)); // hits mapped so far belong to the buffer that was bound when they were mapped
    HIPCHK(hipStreamSynchronize(ix->stream));
    if (!device_counts) {
        ix->counts = ix->own_counts_buf;
        return KMM_OK;
    }
    if (!is_device_ptr(device_counts))
        return fail(KMM_ERR_INVALID_ARG, "kmm_bind_counts needs a device pointer");
    ix->counts = device_counts;
    return KMM_OK;
}

int kmm_counts_device_ptr(kmm_index_t *ix, uint32_t **out)
{
    if (!ix || !out)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    *out = ix->counts;
    return KMM_OK;
}

int kmm_synchronize(kmm_index_t *ix)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    HIPCHK(hipSetDevice(ix->device));
    return drain(ix);
}

static bool ensure_pack_pool(kmm_index_t *ix);
static bool ensure_pinned(PinnedBuf &b, size_t want);

// The staging ring: RING_SLOTS page-locked buffers of RING_SLOT bytes, each an allocation of its own.  Host threads fill a
// slot, a copy engine empties it (or the other way round), and a slot is touched by one side at a time.  Why a ring and not
// one buffer the size of the batch: 128 MB are made in 7 ms, a 750 MB batch buffer in 40 — as long as the map phase of a
// whole file.  (It does not make the threads faster: 16 threads pack 300 GB/s into page-locked memory with no copy in
// flight and 200 GB/s with one, whether the copies read the buffer being filled, slots of a ring of 8 or of a ring of 64
// that never makes anyone wait — profiles/r05/pack_without_copies.txt, host_membw_dma.txt; at 200 GB/s the packing of a
// batch takes as long as its 2-bit stream needs to cross PCIe, which is what bounds the leg.)
static bool ensure_ring(kmm_index_t *ix)
{
    for (int i = 0; i < RING_SLOTS; ++i) {
        if (ix->ring[i].p)
            continue;
        size_t got = 0;
        uint8_t *p = g_shelf.take(RING_SLOT, &got);
        if (p && got != RING_SLOT) { // (a larger buffer someone reserved: not for a slot)
            g_shelf.give(p, got);
            p = nullptr;
        }
        if (!p && hipHostMalloc(reinterpret_cast<void **>(&p), RING_SLOT, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        ix->ring[i].p = p;
        ix->ring[i].bytes = RING_SLOT;
    }
    for (int i = 0; i < RING_SLOTS; ++i)
        if (!ix->bgzf_slot_ev[i] && hipEventCreateWithFlags(ix->bgzf_slot_ev[i].put(), hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
    return true;
}

// HBM -> PAGEABLE host memory (a fresh numpy array: what get_node_counts hands to the reference's caller).  The runtime's own
// path for pageable memory moves ~10 GB/s and a page-locked landing buffer costs ~50 ms per GB to make — either way tens of
// milliseconds for configs[2]'s 400 MB vector, as long as the whole map phase of a 3 GB FASTQ.  So: through the handle's
// page-locked ring (8 slots of 16 MiB, the one kmm_map_bgzf stages through), the packing threads copying a slot out —
// and taking the destination's first-touch page faults — while the next slots are in flight: PCIe rate.
static int fetch_to_pageable(kmm_index_t *ix, uint8_t *dst, const uint8_t *src, size_t bytes, bool *done)
{
    *done = false;
    constexpr size_t SLOT = RING_SLOT;
    constexpr int SLOTS = RING_SLOTS;
    if (bytes < 4 * SLOT || !ensure_pack_pool(ix) || !ensure_ring(ix))
        return KMM_OK;
    const size_t n_slots = (bytes + SLOT - 1) / SLOT;
    auto issue = [&](size_t c) -> int {
        const size_t b0 = c * SLOT, len = bytes - b0 < SLOT ? bytes - b0 : SLOT;
        HIPCHK(hipMemcpyAsync(ix->ring[c % SLOTS].p, src + b0, len, hipMemcpyDeviceToHost, ix->copy_stream));
        HIPCHK(hipEventRecord(ix->bgzf_slot_ev[c % SLOTS], ix->copy_stream));
        return KMM_OK;
    };
    for (size_t c = 0; c < n_slots && c < (size_t)SLOTS; ++c)
        KMMCHK(issue(c));
    const int T = ix->pack_pool->size();
    for (size_t c = 0; c < n_slots; ++c) {
        HIPCHK(hipEventSynchronize(ix->bgzf_slot_ev[c % SLOTS]));
        const size_t b0 = c * SLOT, len = bytes - b0 < SLOT ? bytes - b0 : SLOT;
        const uint8_t *from = ix->ring[c % SLOTS].p;
        const size_t per = ((len + (size_t)T - 1) / (size_t)T + 63) & ~(size_t)63;
        ix->pack_pool->start([=](int w) {
            const size_t a = (size_t)w * per;
            if (a < len)
                memcpy(dst + b0 + a, from + a, len - a < per ? len - a : per);
        });
        ix->pack_pool->wait();
        if (c + SLOTS < n_slots)
            KMMCHK(issue(c + SLOTS));
    }
    *done = true;
    return KMM_OK;
}

int kmm_get_node_counts(kmm_index_t *ix, uint32_t *out)
{
    if (!ix || !out)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix));
    const size_t bytes = sizeof(uint32_t) * (size_t)(ix->max_node_id + 1);
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    const bool known = hipPointerGetAttributes(&a, out) == hipSuccess;
    if (!known)
        (void)hipGetLastError(); // (ordinary host memory the runtime has never seen)
    const bool on_device = known && (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged);
    const bool page_locked = known && a.type == hipMemoryTypeHost;
    if (!on_device && !page_locked) {
        bool done = false;
        KMMCHK(guarded("kmm_get_node_counts", [&] {
            return fetch_to_pageable(ix, reinterpret_cast<uint8_t *>(out), reinterpret_cast<const uint8_t *>(ix->counts), bytes, &done);
        }));
        if (done)
            return KMM_OK;
    }
    HIPCHK(hipMemcpy(out, ix->counts, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return KMM_OK;
}

int kmm_comm_get_unique_id(uint8_t id[KMM_COMM_ID_BYTES])
{
    if (!id)
        return fail(KMM_ERR_INVALID_ARG, "id is NULL");
    static_assert(KMM_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "kmm.h and rccl.h disagree on the id size");
    KMMCHK(rccl_load());
    ncclUniqueId u;
    RCCLCHK(g_rccl.GetUniqueId(&u));
    memcpy(id, u.internal, KMM_COMM_ID_BYTES);
    return KMM_OK;
}

int kmm_comm_init_rank(kmm_index_t *ix, const uint8_t id[KMM_COMM_ID_BYTES], int n_ranks, int rank)
{
    if (!ix || !id)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    if (n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return fail(KMM_ERR_INVALID_ARG, "rank %d outside [0, %d)", rank, n_ranks);
    KMMCHK(rccl_load());
    HIPCHK(hipSetDevice(ix->device));
    if (ix->comm) {
        RCCLCHK(g_rccl.CommDestroy(ix->comm));
        ix->comm = nullptr;
    }
    ncclUniqueId u;
    memcpy(u.internal, id, KMM_COMM_ID_BYTES);
    RCCLCHK(g_rccl.CommInitRank(&ix->comm, n_ranks, u, rank));
    ix->comm_rank = rank;
    ix->comm_size = n_ranks;
    return KMM_OK;
}

int kmm_comm_reduce_counts(kmm_index_t *ix, int root)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    if (!ix->comm)
        return fail(KMM_ERR_INVALID_ARG, "kmm_comm_init_rank has not been called on this handle");
    if (root < -1 || root >= ix->comm_size)
        return fail(KMM_ERR_INVALID_ARG, "root %d outside [-1, %d)", root, ix->comm_size);
    HIPCHK(hipSetDevice(ix->device));
    const size_t n = (size_t)ix->max_node_id + 1;
    auto reduce = [&](size_t first, size_t count, hipStream_t st) {
        // uint32 addition wraps modulo 2^32 like mapper.pyx:37,68, whatever the order of the reduction
        return root < 0 ? g_rccl.AllReduce(ix->counts + first, ix->counts + first, count, ncclUint32, ncclSum, ix->comm, st)
                        : g_rccl.Reduce(ix->counts + first, ix->counts + first, count, ncclUint32, ncclSum, root, ix->comm, st);
    };
    // The tail of a multi-GPU job is flush (per-entry hits -> node counts: 2 ms at the 100 M index, 25 ms at 10^9 entries)
    // + the reduce of 4 (max_node_id + 1) bytes.  With the entries listed in node order the flush of one node RANGE only
    // writes that range of the count vector, so range s is flushed while range s - 1 travels: the ranges' reduces go to
    // a second stream, each behind the event of its flush.  Every rank issues the same sequence of reduces.
    const int S = ix->comm_slices;
    // How many collectives a rank issues must not depend on anything rank-local — what THIS rank has mapped, whether ITS
    // node-ordered entry list could be allocated ("absent if memory is short", rx_build), per-handle modes: a rank that
    // issued one reduce of n elements against its peers' S reduces of n / S would hang the job or corrupt the counts.
    // Only the vector's length and "comm_overlap_slices" (the same on every rank: a parameter of the job) decide; a rank
    // that cannot flush by node range flushes everything first and then issues the same S range reduces.
    if (S > 1 && n >= (size_t)S * 1024) {
        const bool by_range = ix->rx_norder && !ix->rx_ecnt_acc && ix->rx_flush_sorted;
        ix->comm_sliced_reduces++;
        if (!ix->comm_stream)
            HIPCHK(hipStreamCreateWithFlags(ix->comm_stream.put(), hipStreamNonBlocking));
        while ((int)ix->comm_events.size() < S + 1) {
            Event e;
            HIPCHK(hipEventCreateWithFlags(e.put(), hipEventDisableTiming));
            ix->comm_events.push_back(std::move(e));
        }
        if (!by_range)
            KMMCHK(rx_flush(ix)); // (every hit is in `counts`; the ranges below then only travel)
        if (by_range && (int)ix->flush_cuts.size() != S + 1) { // once per handle: where the node ranges begin in the node-ordered list
            std::vector<uint32_t> bounds(S + 1);
            for (int t = 0; t <= S; ++t)
                bounds[t] = (uint32_t)(n * (size_t)t / (size_t)S);
            DevBuf d_b, d_c;
            KMMCHK(ensure(d_b, (S + 1) * 4));
            KMMCHK(ensure(d_c, (S + 1) * 8));
            HIPCHK(hipMemcpyAsync(d_b.p, bounds.data(), (S + 1) * 4, hipMemcpyHostToDevice, ix->stream));
            hipLaunchKernelGGL(k_rx_node_cuts, dim3(1), dim3(64), 0, ix->stream, ix->rx_nnode, ix->rx_S, (const uint32_t *)d_b.p, S + 1,
                               (unsigned long long *)d_c.p);
            HIPCHK(hipGetLastError());
            ix->flush_cuts.assign(S + 1, 0);
            HIPCHK(hipMemcpyAsync(ix->flush_cuts.data(), d_c.p, (S + 1) * 8, hipMemcpyDeviceToHost, ix->stream));
            HIPCHK(hipStreamSynchronize(ix->stream));
            ix->flush_cuts[0] = 0;
            ix->flush_cuts[S] = ix->rx_S;
        }
        ScopedTimer tm;
        KMMCHK(tm.begin(ix, KMM_KERNEL_RX_FLUSH));
        for (int t = 0; t < S; ++t) {
            if (by_range && ix->ecnt_dirty) {
                const uint64_t j0 = ix->flush_cuts[t], j1 = ix->flush_cuts[t + 1];
                if (j1 > j0)
                    hipLaunchKernelGGL(k_rx_flush_sorted, dim3(grid_for(ix, (int64_t)((j1 - j0 + 1023) / 1024), 8)), dim3(256), 0, ix->stream,
                                       view_of(ix), ix->rx_ecnt, ix->rx_norder + j0, ix->rx_nnode + j0, j1 - j0);
                HIPCHK(hipGetLastError());
            }
            HIPCHK(hipEventRecord(ix->comm_events[t], ix->stream));
            HIPCHK(hipStreamWaitEvent(ix->comm_stream, ix->comm_events[t], 0));
            const size_t first = n * (size_t)t / (size_t)S, end = n * (size_t)(t + 1) / (size_t)S;
            RCCLCHK(reduce(first, end - first, ix->comm_stream));
        }
        if (by_range && ix->ecnt_dirty)
            HIPCHK(hipMemsetAsync(ix->rx_ecnt, 0, (size_t)ix->rx_S * 4, ix->stream));
        KMMCHK(tm.end());
        ix->ecnt_dirty = false;
        HIPCHK(hipEventRecord(ix->comm_events[S], ix->comm_stream));
        HIPCHK(hipStreamWaitEvent(ix->stream, ix->comm_events[S], 0));
        return drain(ix);
    }
    KMMCHK(rx_flush(ix)); // every hit mapped so far is in `counts` before it travels
    RCCLCHK(reduce(0, n, ix->stream));
    return drain(ix);
}

int kmm_comm_destroy(kmm_index_t *ix)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    if (ix->comm) {
        HIPCHK(hipSetDevice(ix->device));
        HIPCHK(hipStreamSynchronize(ix->stream));
        RCCLCHK(g_rccl.CommDestroy(ix->comm));
        ix->comm = nullptr;
        ix->comm_rank = -1;
        ix->comm_size = 0;
    }
    return KMM_OK;
}

int kmm_reduce_counts(kmm_index_t **per_gpu, int n_gpus, int root)
{
    if (!per_gpu || n_gpus < 1)
        return fail(KMM_ERR_INVALID_ARG, "per_gpu is NULL or n_gpus < 1");
    if (root < -1 || root >= n_gpus)
        return fail(KMM_ERR_INVALID_ARG, "root %d outside [-1, %d)", root, n_gpus);
    std::vector<int> devs(n_gpus);
    for (int i = 0; i < n_gpus; ++i) {
        if (!per_gpu[i])
            return fail(KMM_ERR_INVALID_ARG, "per_gpu[%d] is NULL", i);
        if (per_gpu[i]->max_node_id != per_gpu[0]->max_node_id)
            return fail(KMM_ERR_INVALID_ARG, "handles disagree on max_node_id");
        devs[i] = per_gpu[i]->device;
        for (int j = 0; j < i; ++j)
            if (devs[j] == devs[i])
                return fail(KMM_ERR_INVALID_ARG, "handles %d and %d share device %d: one handle per GPU", j, i, devs[i]);
    }
    if (n_gpus == 1) {
        HIPCHK(hipSetDevice(per_gpu[0]->device));
        return drain(per_gpu[0]);
    }
    KMMCHK(rccl_load());
    std::vector<ncclComm_t> comms(n_gpus);
    RCCLCHK(g_rccl.CommInitAll(comms.data(), n_gpus, devs.data()));
    int rc = KMM_OK;
    const size_t n = (size_t)per_gpu[0]->max_node_id + 1;
    for (int i = 0; i < n_gpus && rc == KMM_OK; ++i) {
        if (hipSetDevice(devs[i]) != hipSuccess)
            rc = fail(KMM_ERR_HIP, "hipSetDevice(%d) failed", devs[i]);
        else
            rc = rx_flush(per_gpu[i]);
    }
    if (rc == KMM_OK) {
        ncclResult_t r = g_rccl.GroupStart();
        for (int i = 0; i < n_gpus && r == ncclSuccess; ++i) {
            kmm_index *ix = per_gpu[i];
            r = root < 0 ? g_rccl.AllReduce(ix->counts, ix->counts, n, ncclUint32, ncclSum, comms[i], ix->stream)
                         : g_rccl.Reduce(ix->counts, ix->counts, n, ncclUint32, ncclSum, root, comms[i], ix->stream);
        }
        const ncclResult_t r2 = g_rccl.GroupEnd();
        if (r == ncclSuccess)
            r = r2;
        if (r != ncclSuccess)
            rc = fail(KMM_ERR_HIP, "RCCL reduce of the node counts: %s", g_rccl.GetErrorString(r));
    }
    for (int i = 0; i < n_gpus; ++i) {
        (void)hipSetDevice(devs[i]);
        const int d = drain(per_gpu[i]);
        if (rc == KMM_OK)
            rc = d;
        (void)g_rccl.CommDestroy(comms[i]);
    }
    return rc;
}

int kmm_get_kmer_counts(kmm_index_t *ix, uint32_t *out)
{
    if (!ix || !out)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    if (!ix->rx_ecnt_acc)
        return fail(KMM_ERR_INVALID_ARG, "per-k-mer counts are only kept in count_kmers mode "
                    "(kmm_set_param(idx, \"count_kmers\", 1) before mapping)");
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix));
    const size_t n = (size_t)ix->n_entries;
    if (n == 0)
        return KMM_OK;
    const bool out_dev = is_device_ptr(out);
    DevBuf tmp;
    uint32_t *d_out = out;
    if (!out_dev) {
        KMMCHK(ensure(tmp, n * 4));
        d_out = (uint32_t *)tmp.p;
    }
    hipError_t e = hipMemsetAsync(d_out, 0, n * 4, ix->stream); // entries that no bucket references stay 0
    if (e == hipSuccess && ix->rx_S) {
        hipLaunchKernelGGL(k_rx_entry_counts, dim3(grid_for(ix, (int64_t)((ix->rx_S + 255) / 256), 16)), dim3(256), 0,
                           ix->stream, ix->rx_ecnt_acc, ix->rx_porig, ix->rx_S, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess && !out_dev)
        e = hipMemcpyAsync(out, d_out, n * 4, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess)
        return fail(KMM_ERR_HIP, "kmm_get_kmer_counts: %s", hipGetErrorString(e));
    return KMM_OK;
}

int kmm_map_kmers(kmm_index_t *ix, const uint64_t *kmers, int64_t n, int max_freq, int also_revcomp,
                  int k)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(refuse_in_record_hits(ix, "kmm_map_kmers"));
    if (n < 0 || (n > 0 && !kmers))
        return fail(KMM_ERR_INVALID_ARG, "kmers NULL or n negative");
    if (also_revcomp)
        KMMCHK(check_k(k));
    if (n == 0)
        return KMM_OK;
    HIPCHK(hipSetDevice(ix->device));
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    bool staged = false;
    const uint64_t *d_kmers = nullptr;
    KMMCHK(stage_in<uint64_t>(ix, s.kmers, kmers, (size_t)n, &d_kmers, &staged));
    KMMCHK(stage_copies_done(ix));
    ix->map_calls++;
    if (use_radix(ix, n)) {
        ReadsView rv;
        memset(&rv, 0, sizeof rv);
        rv.first_bad = ix->first_bad;
        KMMCHK(launch_rx<MODE_KMERS>(ix, rv, d_kmers, n, k, max_freq, also_revcomp ? 1 : 0));
        return stage_release(ix, s, staged);
    }
    constexpr int U = 8;
    KMMCHK(ensure_direct(ix));
    ix->n_direct_batches++;
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_MAP_KMERS));
    {
        const IndexView iv = view_of(ix);
        const int64_t n_spans = (n + 256 * U - 1) / (256 * U);
        DirectSchedule sched;
        KMMCHK(direct_schedule(ix, n_spans, &sched));
        with_probe_flavour(iv, [&](auto probe) {
            hipLaunchKernelGGL((k_map_kmers<U, decltype(probe)::value>), sched.grid, dim3(256), 0, ix->stream, d_kmers, n, iv,
                               max_freq, also_revcomp ? 1 : 0, k, sched.queue, ix->dyn_chunk);
        });
    }
    HIPCHK(hipGetLastError());
    KMMCHK(tm.end());
    return stage_release(ix, s, staged);
}

// Reads of one length: the uniform front end's constants and, where they apply, the packed tiles of the radix path's
// pass 1 (kmm_tile.hpp): pk_lpr lanes per read, pk_S windows each.
static void set_uniform_geometry(const kmm_index_t *ix, ReadsView &rv, int64_t read_len, int k)
{
    rv.read_len = (uint64_t)read_len;
    rv.read_len_magic = magic_for((uint64_t)read_len);
    if (ix->rx_packed && read_len >= k && read_len - k + 1 <= 4096) {
        const uint32_t W = (uint32_t)(read_len - k + 1), lpr = (W + 15u) / 16u, rpt = 256u / lpr;
        if (rpt >= 1u && (uint64_t)rpt * (uint64_t)read_len <= 8176u) {
            rv.pk_rpt = rpt;
            rv.pk_lpr = lpr;
            rv.pk_S = (W + lpr - 1u) / lpr;
            rv.pk_W = W;
            rv.pk_inv = (65536u + lpr - 1u) / lpr;
        }
    }
}

static int rec_launch_flat(kmm_index_t *ix, const uint32_t *flat, int64_t total, int64_t n_reads, const uint32_t *start_bits,
                           int64_t n_words, int64_t uniform_len, int k, int max_freq, int also_revcomp);

// The handle's packing threads ("host_pack_threads"), created at first use and kept asleep between calls.  false: no
// threads to be had (the caller takes the ordinary route) — nothing thrown by the thread library crosses the C ABI.
static bool ensure_pack_pool(kmm_index_t *ix)
{
    if (ix->host_pack_threads < 1)
        return false;
    if (ix->pack_pool && ix->pack_pool->size() == ix->host_pack_threads)
        return true;
    try {
        ix->pack_pool.reset();
        ix->pack_pool.reset(new kmm_hostpack::Workers(ix->host_pack_threads));
    } catch (...) {
        ix->pack_pool.reset();
        return false;
    }
    return true;
}

// page-locked home of a packed batch: grown, never shrunk; false = none to be had
static bool ensure_pinned(PinnedBuf &b, size_t want)
{
    if (b.bytes >= want)
        return true;
    b.reset();
    if ((b.p = g_shelf.take(want, &b.bytes)))
        return true;
    const size_t take = want + want / 8;
    if (hipHostMalloc(reinterpret_cast<void **>(&b.p), take, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return false;
    }
    b.bytes = take;
    return true;
}

// Flat reads in HOST memory, default lookup table, a batch of radix size, "host_pack_threads" > 0: packed to 2 bits
// per base by that many host threads into a page-locked buffer, chunk by chunk, each chunk copied to HBM as soon as it is
// packed (copy stream: under the previous call's kernels and under the packing of the next chunks), then mapped like the
// flat reads the records compaction makes (pass 1 on 2-bit codes).  *done = false: a byte outside the table — the caller
// takes the ordinary route, whose kernels report the byte's offset (mapper semantics unchanged: nothing was mapped here).
static int map_reads_host_packed(kmm_index_t *ix, const uint8_t *bases, const int64_t *read_offsets, int64_t total_bases,
                                 int64_t n_reads, int64_t read_len, int k, int max_freq, int also_revcomp, bool *done)
{
    *done = false;
    const size_t total = (size_t)total_bases;
    const size_t packed_total = (total + 3) / 4, code_bytes = (packed_total + 256 + 63) & ~(size_t)63;
    if (!ensure_pack_pool(ix) || !ensure_ring(ix))
        return KMM_OK; // (no threads / no page-locked memory to be had: the ordinary route)
    static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
    const auto t_0 = std::chrono::steady_clock::now();
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    KMMCHK(ensure(s.kmers, code_bytes));
    const double ms_stage = ms_since(t_0);
    const auto t_1 = std::chrono::steady_clock::now();
    // Tasks of 4 Mi bases (1 MiB packed) handed out in order; 16 of them fill a slot of the staging ring, a full slot leaves
    // for HBM (copy stream: under the previous call's kernels and under the packing of the next slots) and is written again
    // when its copy has landed.
    // ("debug_ring_slot_kb": tests wrap the ring many times with a small batch)
    const size_t SLOT_BYTES = ix->dbg_bgzf_slot_kb > 0 && ((size_t)ix->dbg_bgzf_slot_kb << 10) < RING_SLOT ? (size_t)ix->dbg_bgzf_slot_kb << 10 : RING_SLOT;
    const size_t CHUNK = 4 * (SLOT_BYTES < ((size_t)1 << 20) ? SLOT_BYTES : (size_t)1 << 20), PER_SLOT = SLOT_BYTES / (CHUNK / 4);
    constexpr int SLOTS = RING_SLOTS;
    const size_t n_chunks = (total + CHUNK - 1) / CHUNK, n_slots = (n_chunks + PER_SLOT - 1) / PER_SLOT;
    std::vector<std::atomic<uint32_t>> filled(n_slots);
    for (auto &f : filled)
        f.store(0, std::memory_order_relaxed);
    std::atomic<size_t> next{0}, slots_free{(size_t)SLOTS};
    std::atomic<bool> stop{false}, bad{false};
    const PinnedBuf *ring = ix->ring;
    ix->pack_pool->start([&](int) {
        for (;;) {
            const size_t c = next.fetch_add(1);
            if (c >= n_chunks)
                return;
            const size_t piece = c / PER_SLOT;
            int spins = 0;
            while (piece >= slots_free.load(std::memory_order_acquire) && !stop.load(std::memory_order_relaxed)) {
                if (++spins < 4000) {
#if defined(__x86_64__)
                    __builtin_ia32_pause();
#endif
                } else {
                    std::this_thread::sleep_for(std::chrono::microseconds(50));
                }
            }
            if (stop.load(std::memory_order_relaxed))
                return;
            const size_t b0 = c * CHUNK, len = total - b0 < CHUNK ? total - b0 : CHUNK;
            if (!bad.load(std::memory_order_relaxed) && !kmm_hostpack::pack2(bases + b0, len, ring[piece % SLOTS].p + (c % PER_SLOT) * (CHUNK / 4)))
                bad.store(true);
            filled[piece].fetch_add(1, std::memory_order_release);
        }
    });
    int rc = KMM_OK;
    size_t landed = 0; // slot-sized pieces whose copy to HBM is known to have finished
    double ms_in_copy_calls = 0;
    // (every second slot on a second copy stream: 141 against 146 G k-mers/s, profiles/r05/h2d_two_copy_streams.txt — one stream)
    for (size_t c = 0; c < n_slots && rc == KMM_OK && !bad.load(); ++c) {
        const size_t first = c * PER_SLOT, want = n_chunks - first < PER_SLOT ? n_chunks - first : PER_SLOT;
        int idle = 0;
        while (filled[c].load(std::memory_order_acquire) < (uint32_t)want) {
            bool did = false;
            while (landed + SLOTS < n_slots && landed < c) { // slots whose copies have landed go back to the threads
                if (hipEventQuery(ix->bgzf_slot_ev[landed % SLOTS]) != hipSuccess) {
                    (void)hipGetLastError(); // ("not ready" is no error to keep)
                    break;
                }
                ++landed;
                slots_free.store(landed + SLOTS, std::memory_order_release);
                did = true;
            }
            if (!did) {
                if (++idle < 2000) {
#if defined(__x86_64__)
                    __builtin_ia32_pause();
#endif
                } else {
                    std::this_thread::sleep_for(std::chrono::microseconds(20));
                }
            }
        }
        if (bad.load())
            break;
        const size_t b0 = c * SLOT_BYTES, len = packed_total - b0 < SLOT_BYTES ? packed_total - b0 : SLOT_BYTES;
        const auto t_c = std::chrono::steady_clock::now();
#ifdef KMM_EXPERIMENT_PACK_WITHOUT_COPIES // (tools/ab_build.sh only: how fast do the threads pack when nothing is copied? results are garbage)
        (void)b0; (void)len;
        if (hipEventRecord(ix->bgzf_slot_ev[c % SLOTS], ix->copy_stream) != hipSuccess)
            rc = fail(KMM_ERR_HIP, "hipEventRecord: %s", hipGetErrorString(hipGetLastError()));
#else
        hipStream_t cs = ix->copy_stream;
        if (hipMemcpyAsync((uint8_t *)s.kmers.p + b0, ring[c % SLOTS].p, len, hipMemcpyHostToDevice, cs) != hipSuccess ||
            hipEventRecord(ix->bgzf_slot_ev[c % SLOTS], cs) != hipSuccess)
            rc = fail(KMM_ERR_HIP, "copy of packed reads: %s", hipGetErrorString(hipGetLastError()));
#endif
        if (verbose)
            ms_in_copy_calls += ms_since(t_c);
        while (rc == KMM_OK && landed + SLOTS < n_slots && landed + SLOTS <= c + 1) { // the ring is full: the oldest copy is waited for
            if (hipEventSynchronize(ix->bgzf_slot_ev[landed % SLOTS]) != hipSuccess) {
                rc = fail(KMM_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(hipGetLastError()));
                break;
            }
            ++landed;
            slots_free.store(landed + SLOTS, std::memory_order_release);
        }
    }
    if (rc != KMM_OK || bad.load())
        stop.store(true);
    ix->pack_pool->wait();
    if (verbose)
        fprintf(stderr, "libkmm: host flat packer: %zu bases, waited %.2f ms for the stage, pack + copies issued %.2f ms (%.1f GB/s; %.2f ms of it "
                "inside the %zu copy calls), %d threads\n", total, ms_stage, ms_since(t_1), (double)total / 1e6 / ms_since(t_1),
                ms_in_copy_calls, n_slots, ix->host_pack_threads);
    if (rc != KMM_OK || bad.load()) {
        // nothing was launched on the handle's stream; the copies issued so far only touched this stage's own buffer
        HIPCHK(hipEventRecord(ix->copied, ix->copy_stream));
        HIPCHK(hipEventSynchronize(ix->copied));
        ix->cur ^= 1; // (hand the stage back: the ordinary route takes it again)
        return rc;
    }
    // (the halo words pass 1 loads behind the last read)
    HIPCHK(hipMemsetAsync((uint8_t *)s.kmers.p + packed_total, 0, code_bytes - packed_total, ix->copy_stream));
    ix->map_calls++;
    ix->host_packed_calls++;
    const uint32_t *start_bits = nullptr;
    int64_t n_words = 0;
    if (read_offsets) { // ragged reads: where they start, as a bitset over the flat bases (what pass 1's flat front end reads)
        bool staged = false;
        const int64_t *d_offs = nullptr;
        KMMCHK(stage_in<int64_t>(ix, s.offsets, read_offsets, (size_t)(n_reads + 1), &d_offs, &staged));
        n_words = (int64_t)total / 32 + 2;
        KMMCHK(ensure(s.start_bits, (size_t)n_words * 4));
        KMMCHK(stage_copies_done(ix));
        HIPCHK(hipMemsetAsync(s.start_bits.p, 0, (size_t)n_words * 4, ix->stream));
        hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(ix, (n_reads + 256) / 256, 8)), dim3(256), 0, ix->stream, d_offs, n_reads,
                           (int64_t)total, (uint32_t *)s.start_bits.p);
        hipLaunchKernelGGL(k_check_offsets, dim3(grid_for(ix, (n_reads + 255) / 256, 8)), dim3(256), 0, ix->stream, d_offs, n_reads,
                           ix->first_bad);
        HIPCHK(hipGetLastError());
        start_bits = (const uint32_t *)s.start_bits.p;
    }
    KMMCHK(rec_launch_flat(ix, (const uint32_t *)s.kmers.p, (int64_t)total, n_reads, start_bits, n_words, read_offsets ? 0 : read_len, k,
                           max_freq, also_revcomp));
    *done = true;
    return stage_release(ix, s, true);
}

// Raw FASTQ / two-line FASTA records in HOST memory (the file mapping, the inflater's output: no page-locked copy of the raw
// bytes is made), default lookup table, a chunk of radix size, "host_pack_threads" > 0: the host threads put the bases
// of the sequence lines straight into the 2-bit stream and the read starts into the bitset (kmm_hostpack::RecordsJob: the
// rules of the device-side compaction, kmm_records.hpp), the stream crosses PCIe while the rest is still being packed,
// and pass 1 runs on it as on the compaction's output.  This is what the reference's `-t` workers do with a chunk
// (bnp parser + encoder, command_line_interface.py:102-111,124-130), minus the k-mer hashing.  *done = false: a byte without
// a code or a malformed record line — the ordinary route maps the chunk and reports the byte's offset.
static int map_records_host_packed(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int format, int k, int max_freq,
                                   int also_revcomp, int64_t *consumed, int64_t *n_records, bool *done)
{
    *done = false;
    const size_t n = (size_t)n_bytes;
    const size_t code_bytes = (n / 4 + 1024 + 63) & ~(size_t)63, bits_bytes = (n / 8 + 256 + 63) & ~(size_t)63;
    static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
    const auto t_0 = std::chrono::steady_clock::now();
    if (!ensure_pack_pool(ix) || !ensure_pinned(ix->pack_pinned, code_bytes) || !ensure_pinned(ix->pack_bits_pinned, bits_bytes))
        return KMM_OK;
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    KMMCHK(ensure(s.kmers, code_bytes));
    const double ms_alloc = ms_since(t_0);
    const auto t_1 = std::chrono::steady_clock::now();
    kmm_hostpack::RecordsJob job;
    const size_t slice = ix->host_pack_slice_kb > 0 ? (size_t)ix->host_pack_slice_kb << 10 : kmm_hostpack::RecordsJob::slice_bytes();
    job.prepare(raw, n, format == KMM_FORMAT_FASTQ ? 4 : 2, reinterpret_cast<uint64_t *>(ix->pack_pinned.p),
                reinterpret_cast<uint32_t *>(ix->pack_bits_pinned.p), slice);
    ix->pack_pool->start([&job](int) { job.run(); });
    // groups of slices (32 MiB of raw bytes): the words of the stream that lie wholly below the group's end are final
    const size_t GROUP = std::max<size_t>(1, ((size_t)32 << 20) / slice);
    int rc = KMM_OK;
    uint64_t copied_w = 0;
    for (size_t g1 = GROUP; g1 < job.n_slices() && rc == KMM_OK; g1 += GROUP) {
        const uint64_t upto_w = job.wait_packed_prefix(g1) >> 5;
        if (upto_w > copied_w) {
            if (hipMemcpyAsync((uint8_t *)s.kmers.p + copied_w * 8, ix->pack_pinned.p + copied_w * 8, (size_t)(upto_w - copied_w) * 8,
                               hipMemcpyHostToDevice, ix->copy_stream) != hipSuccess)
                rc = fail(KMM_ERR_HIP, "hipMemcpyAsync of packed records: %s", hipGetErrorString(hipGetLastError()));
            copied_w = upto_w;
        }
    }
    ix->pack_pool->wait();
    const kmm_hostpack::RecordsResult r = job.finish();
    if (verbose)
        fprintf(stderr, "libkmm: host records packer: %zu bytes, buffers %.2f ms, pack %.2f ms (%.1f GB/s), %d threads, %s\n", n, ms_alloc,
                ms_since(t_1), (double)n / 1e6 / ms_since(t_1), ix->host_pack_threads, r.ok ? "ok" : "refused");
    if (rc != KMM_OK || !r.ok) {
        HIPCHK(hipEventRecord(ix->copied, ix->copy_stream));
        HIPCHK(hipEventSynchronize(ix->copied));
        ix->cur ^= 1; // (hand the stage back: the ordinary route takes it again)
        return rc;
    }
    ix->map_calls++;
    ix->host_packed_record_calls++;
    if (consumed)
        *consumed = r.consumed;
    if (n_records)
        *n_records = r.n_records;
    *done = true;
    if (r.n_bases <= 0)
        return stage_release(ix, s, copied_w != 0);
    {   // the rest of the stream: from the word that holds the last base's neighbourhood (finish() cleaned it) to the zero
        // words behind it
        const uint64_t end_w = ((uint64_t)r.n_bases >> 5) + 40, from_w = copied_w < ((uint64_t)r.n_bases >> 5) ? copied_w : ((uint64_t)r.n_bases >> 5);
        HIPCHK(hipMemcpyAsync((uint8_t *)s.kmers.p + from_w * 8, ix->pack_pinned.p + from_w * 8, (size_t)(end_w - from_w) * 8,
                              hipMemcpyHostToDevice, ix->copy_stream));
    }
    const bool uniform = r.uniform_len >= 16;
    const uint32_t *start_bits = nullptr;
    int64_t n_words = 0;
    if (!uniform) { // ragged reads: the read-start bitset crosses too (1 bit per base)
        n_words = r.n_bases / 32 + 2;
        KMMCHK(ensure(s.start_bits, (size_t)n_words * 4));
        HIPCHK(hipMemcpyAsync(s.start_bits.p, ix->pack_bits_pinned.p, (size_t)n_words * 4, hipMemcpyHostToDevice, ix->copy_stream));
        start_bits = (const uint32_t *)s.start_bits.p;
    }
    KMMCHK(rec_launch_flat(ix, (const uint32_t *)s.kmers.p, r.n_bases, r.n_records, start_bits, n_words, uniform ? r.uniform_len : 0, k,
                           max_freq, also_revcomp));
    return stage_release(ix, s, true);
}

// quals != NULL (kmm_map_reads_qual with a floor set): quals[p] < qual_thresh makes base p a break (k_mark_low_quals); like a
// table with a break entry that means the ragged front end, and never the host packer, which knows no breaks.
static int map_reads_common(kmm_index_t *ix, const uint8_t *bases, const int64_t *read_offsets,
                            int64_t n_reads, int64_t read_len, int k, int max_freq,
                            int also_revcomp, const uint8_t *lut, const uint8_t *quals = nullptr, uint32_t qual_thresh = 0)
{
    const bool uniform = (read_offsets == nullptr);
    HIPCHK(hipSetDevice(ix->device));
    int64_t total = 0;
    const bool offs_on_device = !uniform && is_device_ptr(read_offsets);
    if (uniform) {
        total = n_reads * read_len;
    } else {
        int64_t ends[2] = {0, 0};
        if (offs_on_device) {
            HIPCHK(hipMemcpy(&ends[0], read_offsets, 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(&ends[1], read_offsets + n_reads, 8, hipMemcpyDeviceToHost));
        } else {
            ends[0] = read_offsets[0];
            ends[1] = read_offsets[n_reads];
        }
        if (ends[0] != 0)
            return fail(KMM_ERR_INVALID_ARG, "read_offsets[0] must be 0 (got %lld)", (long long)ends[0]);
        if (ends[1] < 0)
            return fail(KMM_ERR_INVALID_ARG, "read_offsets[n_reads] negative");
        total = ends[1];
    }
    if (total == 0)
        return KMM_OK;
    if (!bases)
        return fail(KMM_ERR_INVALID_ARG, "bases is NULL");
    if (ix->host_pack_threads > 0 && (uniform ? read_len >= 16 : !offs_on_device) && !lut && !quals && use_radix(ix, total) &&
        !is_device_ptr(bases)) {
        bool done = false;
        KMMCHK(map_reads_host_packed(ix, bases, uniform ? nullptr : read_offsets, total, n_reads, read_len, k, max_freq, also_revcomp,
                                     &done));
        if (done)
            return KMM_OK;
    }

    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    ix->map_calls++;
    bool staged = false;
    ReadsView rv;
    memset(&rv, 0, sizeof rv);
    KMMCHK(stage_in<uint8_t>(ix, s.bases, bases, (size_t)total, &rv.bases, &staged));
    const uint8_t *d_quals = nullptr;
    if (quals)
        KMMCHK(stage_in<uint8_t>(ix, s.quals, quals, (size_t)total, &d_quals, &staged));
    bool has_break = false;
    KMMCHK(resolve_lut(ix, s, lut, &rv.lut, &staged, &has_break));
    rv.total = total;
    rv.n_reads = n_reads;
    rv.first_bad = ix->first_bad;
    const int64_t n_tiles = (total + TILE_T - 1) / TILE_T;
    // the uniform kernel's wrap-around handles one read boundary per lane: needs read_len >= S.  A table with a break
    // entry or a quality floor: the breaks are read boundaries only the bitset can hold — the ragged front end
    const bool uniform_kernel = uniform && read_len >= 16 && !has_break && !quals;
    if (uniform_kernel) {
        set_uniform_geometry(ix, rv, read_len, k);
        KMMCHK(stage_copies_done(ix));
        KMMCHK(launch_map_reads<MODE_UNIFORM>(ix, rv, k, max_freq, also_revcomp ? 1 : 0));
    } else {
        const bool arithmetic_starts = uniform && (has_break || quals); // (no offsets array: nothing on this route reads one)
        if (uniform && !arithmetic_starts) {
            KMMCHK(ensure(s.offsets, (size_t)(n_reads + 1) * 8));
            hipLaunchKernelGGL(k_iota_offsets, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256),
                               0, ix->stream, (int64_t *)s.offsets.p, n_reads, read_len);
            HIPCHK(hipGetLastError());
            rv.offsets = (const int64_t *)s.offsets.p;
        } else if (!uniform) {
            KMMCHK(stage_in<int64_t>(ix, s.offsets, read_offsets, (size_t)(n_reads + 1), &rv.offsets,
                                     &staged));
        }
        const int64_t n_words = total / 32 + 2;
        KMMCHK(ensure(s.start_bits, (size_t)n_words * 4));
        rv.start_bits = (const uint32_t *)s.start_bits.p;
        rv.n_start_words = n_words;
        KMMCHK(stage_copies_done(ix));
        HIPCHK(hipMemsetAsync(s.start_bits.p, 0, (size_t)n_words * 4, ix->stream));
        if (arithmetic_starts)
            hipLaunchKernelGGL(k_mark_uniform_starts, dim3(grid_for(ix, (n_reads + 256) / 256, 8)), dim3(256), 0, ix->stream,
                               n_reads, read_len, (uint32_t *)s.start_bits.p);
        else
            hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(ix, (n_reads + 256) / 256, 8)), dim3(256), 0, ix->stream,
                               rv.offsets, n_reads, total, (uint32_t *)s.start_bits.p);
        if (has_break) // every break byte: a one-base read
            hipLaunchKernelGGL(k_mark_breaks, dim3(grid_for(ix, (total + 256 * 16 * MARK_U - 1) / (256 * 16 * MARK_U), 8)), dim3(256), 0,
                               ix->stream, rv.bases, total, rv.lut, (uint32_t *)s.start_bits.p);
        if (quals) // every quality byte below the floor: a one-base read, too
            hipLaunchKernelGGL(k_mark_low_quals, dim3(grid_for(ix, (total + 256 * 16 * MARK_U - 1) / (256 * 16 * MARK_U), 8)), dim3(256), 0,
                               ix->stream, d_quals, total, qual_thresh, (uint32_t *)s.start_bits.p, (unsigned long long *)ix->stats);
        if (!uniform)
            hipLaunchKernelGGL(k_check_offsets, dim3(grid_for(ix, (n_reads + 255) / 256, 8)), dim3(256), 0,
                               ix->stream, rv.offsets, n_reads, ix->first_bad);
        HIPCHK(hipGetLastError());
        KMMCHK(launch_map_reads<MODE_GENERAL>(ix, rv, k, max_freq, also_revcomp ? 1 : 0));
    }
    return stage_release(ix, s, staged);
}

int kmm_map_reads(kmm_index_t *ix, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads,
                  int k, int max_freq, int also_revcomp, const uint8_t *lut)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(refuse_in_record_hits(ix, "kmm_map_reads"));
    KMMCHK(check_k(k));
    if (n_reads < 0)
        return fail(KMM_ERR_INVALID_ARG, "n_reads negative");
    if (n_reads == 0)
        return KMM_OK;
    if (!read_offsets)
        return fail(KMM_ERR_INVALID_ARG, "read_offsets is NULL");
    KMMCHK(check_k_lut(k, lut));
    return guarded("kmm_map_reads", [&] { return map_reads_common(ix, bases, read_offsets, n_reads, 0, k, max_freq, also_revcomp, lut); });
}

int kmm_map_reads_uniform(kmm_index_t *ix, const uint8_t *bases, int64_t n_reads, int64_t read_len,
                          int k, int max_freq, int also_revcomp, const uint8_t *lut)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(refuse_in_record_hits(ix, "kmm_map_reads_uniform"));
    KMMCHK(check_k(k));
    if (n_reads < 0 || read_len < 0)
        return fail(KMM_ERR_INVALID_ARG, "n_reads / read_len negative");
    if (n_reads == 0 || read_len == 0)
        return KMM_OK;
    KMMCHK(check_k_lut(k, lut));
    return guarded("kmm_map_reads_uniform", [&] { return map_reads_common(ix, bases, nullptr, n_reads, read_len, k, max_freq, also_revcomp, lut); });
}

// Raw records on the radix path: should a piece of n_bytes raw bytes take it?  (Same rule as for flat reads, on the
// bases the piece holds at most: half of a FASTQ piece's bytes, all of a FASTA piece's.)
static bool records_take_radix(const kmm_index_t *ix, int64_t n_bytes, int format)
{
    return use_radix(ix, format == KMM_FORMAT_FASTQ ? n_bytes / 2 : n_bytes);
}

// Bytes per piece of a kmm_map_records call ("debug_records_piece_kb": tests cut a small file into several pieces).
static int64_t records_piece_max(const kmm_index_t *ix)
{
    return ix->dbg_rec_piece_kb > 0 ? ix->dbg_rec_piece_kb << 10 : (int64_t)1 << 30;
}

// The quality floor of a record call, by mode: "record_hits_min_base_quality" while "record_hits" is 1 or 2 (where
// "min_base_quality" > 0 is refused), else "min_base_quality".
static int call_floor(const kmm_index_t *ix)
{
    return ix->record_hits ? ix->rh_min_base_quality : ix->min_base_quality;
}
static const char *call_floor_name(const kmm_index_t *ix)
{
    return ix->record_hits ? "record_hits_min_base_quality" : "min_base_quality";
}

// The quality floor that applies to records of this format: the call's for FASTQ, none for the formats without quality lines.
static int records_quality(const kmm_index_t *ix, int format)
{
    return format == KMM_FORMAT_FASTQ ? call_floor(ix) : 0;
}

// The quality floor that applies to SAM / BAM records: the call's once "use_record_qual" is set (the decoders then
// write four-line FASTQ), else none — QUAL is not read at all, not even its length.
static int record_quality(const kmm_index_t *ix)
{
    return ix->use_record_qual ? call_floor(ix) : 0;
}

// "min_base_quality" > 0 and what it cannot go with: k = 1 (the masked base's own window could not be killed: check_k_lut)
// and the formats whose writers emit two-line FASTA, without QUAL (sam: KMM_FORMAT_SAM or kmm_map_bam), unless
// "use_record_qual" asks for their quality variants — whose FASTQ text is mapped by the radix path alone.
static int check_quality(const kmm_index_t *ix, const char *who, int k, bool sam)
{
    const int q = call_floor(ix);
    const char *name = call_floor_name(ix);
    if (q <= 0)
        return KMM_OK;
    if (sam && !ix->use_record_qual)
        return fail(KMM_ERR_INVALID_ARG, "%s: %s %d is set, and SAM / BAM records are mapped without their QUAL "
                    "column: set it to 0 for this input, or set \"use_record_qual\" to 1 (records that store no qualities then "
                    "pass the floor unmasked: \"records_without_qual\")", who, name, q);
    // (the record-hits mode marks the low bases in front of the direct front end, kmm_rh_qual.hpp: no radix path, no compaction)
    if (sam && !ix->record_hits && !ix->rx_ok)
        return fail(KMM_ERR_INVALID_ARG, "%s: min_base_quality needs the radix path, which is not available for this "
                    "index (kmm_get_param \"radix_unavailable_reason\")", who);
    if (sam && !ix->record_hits && ix->dbg_rec_skip)
        return fail(KMM_ERR_INVALID_ARG, "%s: min_base_quality does not go with debug_records_skip", who);
    if (k == 1)
        return fail(KMM_ERR_INVALID_ARG, "%s: k = 1 with %s %d: needs k >= 2", who, name, q);
    return KMM_OK;
}

// Flat reads with their quality bytes: kmm_map_reads (read_offsets given) or kmm_map_reads_uniform (NULL) with
// "min_base_quality" applied to quals[p] < qual_base + Q.  With the floor off the call is one of those two, quals unread.
int kmm_map_reads_qual(kmm_index_t *ix, const uint8_t *bases, const uint8_t *quals, int qual_base, const int64_t *read_offsets,
                       int64_t n_reads, int64_t read_len, int k, int max_freq, int also_revcomp, const uint8_t *lut)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(refuse_in_record_hits(ix, "kmm_map_reads_qual"));
    KMMCHK(check_k(k));
    if (qual_base != 0 && qual_base != 33)
        return fail(KMM_ERR_INVALID_ARG, "kmm_map_reads_qual: qual_base %d: 33 (Phred+33 text) or 0 (raw Phred)", qual_base);
    if (n_reads < 0 || (!read_offsets && read_len < 0))
        return fail(KMM_ERR_INVALID_ARG, "n_reads / read_len negative");
    if (n_reads == 0 || (!read_offsets && read_len == 0))
        return KMM_OK;
    KMMCHK(check_k_lut(k, lut));
    KMMCHK(check_quality(ix, "kmm_map_reads_qual", k, false));
    const int q = ix->min_base_quality;
    if (q > 0 && !quals)
        return fail(KMM_ERR_INVALID_ARG, "kmm_map_reads_qual: quals is NULL with min_base_quality %d", q);
    return guarded("kmm_map_reads_qual", [&] {
        return map_reads_common(ix, bases, read_offsets, n_reads, read_offsets ? 0 : read_len, k, max_freq, also_revcomp, lut,
                                q > 0 ? quals : nullptr, (uint32_t)(qual_base + q));
    });
}

// Raw records on the radix path (r04): census -> the sequence bytes compacted into flat reads of 2-bit codes (one per
// byte) + the read-start bitset (kmm_records.hpp, k_rec_count2 .. k_rec_uniform), all on the copy stream, i.e. under
// the previous call's map kernels; then pass 1 runs on flat reads — on packed tiles when the reads have one length —
// instead of pushing every raw byte through the records front end (22.3 ms per 10 M reads in round 3).
//
// rec_compact_piece: one piece of at most 2^30 raw bytes (the census is a two-level scan over 1024 x 1024 tiles of 1024
// bytes), appended to the flat reads at flat position `flat_base`.  Synchronises the copy stream (the caller's host
// buffer is free afterwards) and returns where the piece's last complete record ends, its records, the flat length
// after it, and whether its reads have one length.
// qual: the quality floor of a FASTQ piece (0: none) — a second prefix, over the quality bytes, gives k_rec_scatter's quality
// variant the flat position of every tile's first quality byte; n_bit_words: the words of start_bits.
static int rec_compact_piece(kmm_index_t *ix, Stage &s, const uint8_t *d_raw, int64_t n_bytes, int format, const uint8_t *d_lut,
                             bool has_break, int qual, size_t n_bit_words, int64_t flat_base, uint32_t *flat, uint32_t *start_bits,
                             int64_t *consumed, int64_t *n_records, int64_t *flat_end, int64_t *uniform_len)
{
    const int64_t n_tiles = (n_bytes + REC_TB - 1) / REC_TB; // 4 KiB tiles: one wavefront, 64 bytes per lane
    const int n_super = (int)((n_tiles + 1023) / 1024);
    const size_t n_pad = (size_t)n_super * 1024;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_nl = carve(n_pad * 4), o_seq = carve(n_pad * 8), o_pre = carve(n_pad * 4), o_snl = carve((size_t)n_super * 4 + 64),
                 o_sseq = carve((size_t)n_super * 4 + 64), o_info = carve(256), o_out = carve(256);
    const size_t o_qpre = qual ? carve(n_pad * 4) : 0, o_sq = qual ? carve((size_t)n_super * 4 + 64) : 0;
    KMMCHK(ensure(s.aux, off));
    uint8_t *a = (uint8_t *)s.aux.p;
    uint32_t *tile_nl = (uint32_t *)(a + o_nl), *tile_pre = (uint32_t *)(a + o_pre), *super_nl = (uint32_t *)(a + o_snl),
             *super_seq = (uint32_t *)(a + o_sseq);
    unsigned long long *tile_seq = (unsigned long long *)(a + o_seq), *d_out = (unsigned long long *)(a + o_out);
    int64_t *d_info = (int64_t *)(a + o_info);
    // The compaction kernels run on the handle's OWN stream, behind the previous call's passes — not on the copy stream
    // beside them: beside them they gain nothing (both fill the CUs: 64.7 against 65.2 ms per two 10 M-read calls).
    // (Running them there is how round 4 found a race in pass 1 that round 3 had left behind — foreign wavefronts on
    // pass 1's SIMDs delayed a counter clear past another wavefront's next ranking atomic, rx_sort_emit; fixed there,
    // profiles/r04/records_overlap_fault.txt — and tools/records_overlap_bisect.py still can: debug_records_copy_stream.)
    // Host -> HBM copies stay on the copy stream; every kernel of a handle runs on the handle's stream.
    hipStream_t cs = ix->dbg_rec_copy_stream ? ix->copy_stream : ix->stream;
    const int skip = ix->dbg_rec_skip;
    const uint32_t pm = (uint32_t)format - 1u, hc = format == KMM_FORMAT_FASTQ ? (uint32_t)'@' : (uint32_t)'>';
    // persistent wavefronts: tiles t, t + waves, ... ("debug_records_grid": a few wavefronts give a small file the long tile
    // ranges per wavefront that only a piece beyond 32 MiB has otherwise)
    const dim3 g4((unsigned)(ix->dbg_rec_grid > 0 ? ix->dbg_rec_grid : grid_for(ix, (n_tiles + 3) / 4, 8)));
    HIPCHK(hipMemsetAsync(tile_nl, 0, n_pad * 4, cs));
    HIPCHK(hipMemsetAsync(tile_seq, 0, n_pad * 8, cs));
    HIPCHK(hipMemsetAsync(d_info, 0, 512, cs)); // (info and out_info: neighbours)
    if (!(skip & 1))
        hipLaunchKernelGGL(k_rec_count2, g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_nl, tile_seq);
    if (!(skip & 2)) {
        hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, cs, tile_nl, super_nl);
        hipLaunchKernelGGL(k_rec_scan2, dim3(1), dim3(1024), 0, cs, d_raw, n_bytes, n_super, tile_nl, super_nl, (uint32_t)format, d_info,
                           (int)REC_TB);
        hipLaunchKernelGGL(k_rec_seq_scan, dim3(n_super), dim3(1024), 0, cs, tile_seq, tile_nl, super_nl, n_tiles, pm, 1u, tile_pre, super_seq);
        hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, cs, super_seq, n_super, (uint32_t *)(d_out + 8));
    }
    if (qual) { // (never with "debug_records_skip": map_records_entry)
        RecQual q;
        uint32_t *tile_q = (uint32_t *)(a + o_qpre), *super_q = (uint32_t *)(a + o_sq);
        hipLaunchKernelGGL(k_rec_seq_scan, dim3(n_super), dim3(1024), 0, cs, tile_seq, tile_nl, super_nl, n_tiles, pm, 3u, tile_q, super_q);
        hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, cs, super_q, n_super, (uint32_t *)(d_out + 9));
        q.tile_pre = tile_q;
        q.super_pre = super_q;
        q.masked = ix->stats;
        q.thresh = 33u + (uint32_t)qual;
        q.n_words = (uint32_t)n_bit_words; // (a call holds fewer than 2^37 bytes)
        if (has_break)
            hipLaunchKernelGGL((k_rec_scatter<true, true>), g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_nl, super_nl, tile_pre, super_seq,
                               d_info, d_lut, pm, hc, flat, (uint64_t)flat_base, start_bits, ix->first_bad, d_out, q);
        else
            hipLaunchKernelGGL((k_rec_scatter<false, true>), g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_nl, super_nl, tile_pre, super_seq,
                               d_info, d_lut, pm, hc, flat, (uint64_t)flat_base, start_bits, ix->first_bad, d_out, q);
    } else if (!(skip & 4) && has_break) // (break bytes become one-base reads: k_rec_uniform then finds more starts than records)
        hipLaunchKernelGGL(k_rec_scatter<true>, g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_nl, super_nl, tile_pre, super_seq,
                           d_info, d_lut, pm, hc, flat, (uint64_t)flat_base, start_bits, ix->first_bad, d_out);
    else if (!(skip & 4))
        hipLaunchKernelGGL(k_rec_scatter<false>, g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_nl, super_nl, tile_pre, super_seq,
                           d_info, d_lut, pm, hc, flat, (uint64_t)flat_base, start_bits, ix->first_bad, d_out);
    if (!(skip & 8))
        hipLaunchKernelGGL(k_rec_uniform, dim3(grid_for(ix, (n_bytes / 32 + 256) / 256, 4)), dim3(256), 0, cs, start_bits,
                           (uint64_t)flat_base, d_info, d_out);
    HIPCHK(hipGetLastError());
    struct { int64_t info[8]; unsigned long long out[8]; } h;
    memset(&h, 0, sizeof h);
    HIPCHK(hipMemcpyAsync(h.info, d_info, 64, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipMemcpyAsync(h.out, d_out, 64, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs)); // (it waited for the copy: the borrowed host buffer is free from here on)
    *consumed = h.info[0];
    *n_records = h.info[1];
    *flat_end = h.info[0] > 0 ? (int64_t)h.out[0] : flat_base;
    const int64_t piece = *flat_end - flat_base, recs = h.info[1];
    const int64_t L = recs > 0 ? piece / recs : 0;
    *uniform_len = (recs > 0 && L * recs == piece && h.out[1] == (unsigned long long)recs && h.out[2] == 0) ? L : 0;
    return KMM_OK;
}

// The flat reads (codes, one per byte) through the radix path.
static int rec_launch_flat(kmm_index_t *ix, const uint32_t *flat, int64_t total, int64_t n_reads, const uint32_t *start_bits,
                           int64_t n_words, int64_t uniform_len, int k, int max_freq, int also_revcomp)
{
    ReadsView rv;
    memset(&rv, 0, sizeof rv);
    rv.bases = reinterpret_cast<const uint8_t *>(flat);
    rv.codes2 = 1;           // 16 two-bit codes per word: pass 1 stages the words as they are
    rv.total = total;
    rv.n_reads = n_reads;
    rv.lut = ix->lut_codes;
    rv.first_bad = ix->first_bad;
    KMMCHK(stage_copies_done(ix));
    if (uniform_len >= 16 && uniform_len * n_reads == total) {
        set_uniform_geometry(ix, rv, uniform_len, k);
        ix->flat_uniform_batches++;
        if (rv.pk_rpt)
            return launch_rx<MODE_PACKED>(ix, rv, nullptr, 0, k, max_freq, also_revcomp ? 1 : 0);
        return launch_rx<MODE_UNIFORM>(ix, rv, nullptr, 0, k, max_freq, also_revcomp ? 1 : 0);
    }
    rv.start_bits = start_bits;
    rv.n_start_words = n_words;
    return launch_rx<MODE_GENERAL>(ix, rv, nullptr, 0, k, max_freq, also_revcomp ? 1 : 0);
}

// One piece, compacted and mapped by itself (the unwrapped pieces of multi-line FASTA come this way).
static int map_records_piece_radix(kmm_index_t *ix, Stage &s, const uint8_t *d_raw, int64_t n_bytes, int format, int k,
                                   int max_freq, int also_revcomp, const uint8_t *d_lut, bool has_break, int64_t *consumed,
                                   int64_t *n_records)
{
    const size_t n_words = (size_t)n_bytes / 32 + 2, code_bytes = ((size_t)n_bytes / 4 + 256) & ~(size_t)15;
    KMMCHK(ensure(s.start_bits, n_words * 4));
    KMMCHK(ensure(s.kmers, code_bytes));
    KMMCHK(stage_copies_done(ix)); // (a host buffer staged by the caller: the kernels below wait for the copy)
    HIPCHK(hipMemsetAsync(s.start_bits.p, 0, n_words * 4, ix->stream));
    HIPCHK(hipMemsetAsync(s.kmers.p, 0, code_bytes, ix->stream));
    int64_t flat_end = 0, L = 0;
    // (no quality floor here: a FASTQ call with one is map_records_radix_call's, whatever its size)
    KMMCHK(rec_compact_piece(ix, s, d_raw, n_bytes, format, d_lut, has_break, 0, n_words, 0, (uint32_t *)s.kmers.p,
                             (uint32_t *)s.start_bits.p, consumed, n_records, &flat_end, &L));
    if (*consumed <= 0 || flat_end <= 0)
        return KMM_OK;
    return rec_launch_flat(ix, (const uint32_t *)s.kmers.p, flat_end, *n_records, (const uint32_t *)s.start_bits.p, (int64_t)n_words,
                           L, k, max_freq, also_revcomp);
}

// A whole kmm_map_records call on the radix path: the pieces (at most 2^30 raw bytes each, every one starting where the
// previous one's last complete record ended) are compacted one after the other into ONE array of flat reads, which then
// takes the radix path as one batch — the passes' fixed costs per batch (0.85 ms at the 100 M index) are paid once per
// call, not once per GiB of FASTQ.
static int map_records_radix_call(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int format, int k, int max_freq,
                                  int also_revcomp, const uint8_t *lut, int64_t *consumed, int64_t *n_records)
{
    static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
    const auto t_0 = std::chrono::steady_clock::now();
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    const double ms_acquire = ms_since(t_0);
    ix->map_calls++;
    bool staged = false;
    const uint8_t *d_lut = nullptr;
    bool has_break = false;
    KMMCHK(resolve_lut(ix, s, lut, &d_lut, &staged, &has_break));
    if (staged)
        KMMCHK(stage_copies_done(ix)); // (a caller's lookup table staged from the host)
    const bool on_device = is_device_ptr(raw);
    const size_t n_words = (size_t)n_bytes / 32 + 2, code_bytes = ((size_t)n_bytes / 4 + 256) & ~(size_t)15;
    KMMCHK(ensure(s.start_bits, n_words * 4));
    KMMCHK(ensure(s.kmers, code_bytes));
    if (!(ix->dbg_rec_skip & 16)) {
        hipStream_t ms = ix->dbg_rec_copy_stream ? ix->copy_stream : ix->stream;
        HIPCHK(hipMemsetAsync(s.start_bits.p, 0, n_words * 4, ms));
        HIPCHK(hipMemsetAsync(s.kmers.p, 0, code_bytes, ms));
    }
    const int64_t piece_max = records_piece_max(ix);
    const int qual = records_quality(ix, format);
    int64_t off = 0, recs = 0, flat = 0, L = -1;
    while (off < n_bytes) {
        const int64_t len = n_bytes - off < piece_max ? n_bytes - off : piece_max;
        const uint8_t *d_raw = raw + off;
        if (!on_device) {
            KMMCHK(ensure(s.bases, (size_t)len));
            HIPCHK(hipMemcpyAsync(s.bases.p, raw + off, (size_t)len, hipMemcpyHostToDevice, ix->copy_stream));
            KMMCHK(stage_copies_done(ix)); // the compaction kernels (handle's stream) wait for the copy
            d_raw = (const uint8_t *)s.bases.p;
        }
        int64_t used = 0, nr = 0, flat_end = flat, Lp = 0;
        KMMCHK(rec_compact_piece(ix, s, d_raw, len, format, d_lut, has_break, qual, n_words, flat, (uint32_t *)s.kmers.p,
                                 (uint32_t *)s.start_bits.p, &used, &nr, &flat_end, &Lp));
        if (used > 0) {
            L = (L == -1 || L == Lp) ? Lp : 0; // one length over all pieces, or none
            flat = flat_end;
        }
        off += used;
        recs += nr;
        if (used == 0 || len < piece_max)
            break; // no complete record left in reach / the last piece
    }
    if (consumed)
        *consumed = off;
    if (n_records)
        *n_records = recs;
    const double ms_compact = ms_since(t_0) - ms_acquire;
    if (flat > 0 && !ix->dbg_rec_skip && !ix->dbg_rec_copy_stream)
        KMMCHK(rec_launch_flat(ix, (const uint32_t *)s.kmers.p, flat, recs, (const uint32_t *)s.start_bits.p, (int64_t)n_words,
                               L > 0 ? L : 0, k, max_freq, also_revcomp));
    if (verbose)
        fprintf(stderr, "libkmm: records on the radix path: %lld bytes %s: waited %.2f ms for the stage, census + compaction issued %.2f ms, "
                "passes issued %.2f ms\n", (long long)n_bytes, on_device ? "in HBM" : "in host memory", ms_acquire, ms_compact,
                ms_since(t_0) - ms_acquire - ms_compact);
    return stage_release(ix, s, false);
}

// The floor of the record-hits mode on one FASTQ piece (kmm_rh_qual.hpp), between the census and the hit kernel:
// rv as the hit kernel takes it (total: the end of the piece's last complete record; the census arrays).  The bitset of the
// low bases (one bit per raw byte, the halo of the last tile included) lies in the stage's start_bits, the line starts of the
// piece's n_records records in its aux: neither is used by the direct records route.  Sets rv.dead; no host round trip.
static int rq_mark_piece(kmm_index_t *ix, Stage &s, ReadsView &rv, int64_t n_records, int qual)
{
    const uint32_t n_tiles = (uint32_t)((rv.total + 1023) / 1024), n_lines = (uint32_t)(4 * n_records); // (a piece: at most 2^30 bytes)
    const size_t dead_bytes = (size_t)n_tiles * 128 + 64;
    KMMCHK(ensure(s.start_bits, dead_bytes));
    KMMCHK(ensure(s.aux, (size_t)n_lines * 4 + 64));
    ScopedTimer tm;
    KMMCHK(tm.begin(ix, KMM_KERNEL_RH_QUAL_MARK));
    HIPCHK(hipMemsetAsync(s.start_bits.p, 0, dead_bytes, ix->stream));
    const dim3 grid((n_tiles + 3) / 4);
    hipLaunchKernelGGL(k_rq_line_starts, grid, dim3(256), 0, ix->stream, rv.bases, (uint32_t)rv.total, n_tiles, rv.tile_nl, rv.super_nl,
                       n_lines, (uint32_t *)s.aux.p);
    hipLaunchKernelGGL(k_rq_mark, grid, dim3(256), 0, ix->stream, rv.bases, (uint32_t)rv.total, n_tiles, rv.tile_nl, rv.super_nl, n_lines,
                       (const uint32_t *)s.aux.p, 33u + (uint32_t)qual, ix->rq_exempt, (uint64_t)ix->rq_text_off, (uint32_t *)s.start_bits.p,
                       ix->first_bad, ix->stats);
    HIPCHK(hipGetLastError());
    KMMCHK(tm.end());
    rv.dead = (const uint32_t *)s.start_bits.p;
    return KMM_OK;
}

// The hit kernel of a piece of records: the variant for the table (a break entry) and the floor (rv.dead set: rq_mark_piece).
static int launch_record_hits(kmm_index_t *ix, const ReadsView &rv, bool has_break, int k, int max_freq, int also_rc, uint32_t *hits,
                              uint32_t *windows)
{
    if (rv.dead && has_break)
        return launch_read_hits<MODE_RECORDS_BRK_QUAL>(ix, rv, k, max_freq, also_rc, nullptr, hits, windows);
    if (rv.dead)
        return launch_read_hits<MODE_RECORDS_QUAL>(ix, rv, k, max_freq, also_rc, nullptr, hits, windows);
    if (has_break)
        return launch_read_hits<MODE_RECORDS_BRK>(ix, rv, k, max_freq, also_rc, nullptr, hits, windows);
    return launch_read_hits<MODE_RECORDS>(ix, rv, k, max_freq, also_rc, nullptr, hits, windows);
}

// One piece of at most 2^30 bytes (the newline census is a two-level scan over 1024 x 1024 tiles of 1024 bytes).
static int map_records_piece(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int format, int k,
                             int max_freq, int also_revcomp, const uint8_t *lut, int64_t *consumed,
                             int64_t *n_records)
{
    static_assert(TILE_T == 1024, "records mode counts newlines per 1024-byte tile");
    *consumed = 0;
    *n_records = 0;
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    ix->map_calls++;
    bool staged = false;
    ReadsView rv;
    memset(&rv, 0, sizeof rv);
    KMMCHK(stage_in<uint8_t>(ix, s.bases, raw, (size_t)n_bytes, &rv.bases, &staged));
    bool has_break = false;
    KMMCHK(resolve_lut(ix, s, lut, &rv.lut, &staged, &has_break));
    if (!ix->record_hits && records_take_radix(ix, n_bytes, format)) {
        KMMCHK(map_records_piece_radix(ix, s, rv.bases, n_bytes, format, k, max_freq, also_revcomp, rv.lut, has_break, consumed,
                                       n_records));
        return stage_release(ix, s, false);
    }
    const int64_t n_tiles = (n_bytes + TILE_T - 1) / TILE_T;
    const int n_super = (int)((n_tiles + 1023) / 1024);
    KMMCHK(ensure(s.tile_first, (size_t)n_super * 1024 * 4));
    KMMCHK(ensure(s.offsets, (size_t)n_super * 4 + 64));
    uint32_t *tile_cnt = (uint32_t *)s.tile_first.p;
    uint32_t *super_tot = (uint32_t *)s.offsets.p;
    int64_t *d_out = (int64_t *)((uint8_t *)s.offsets.p + (((size_t)n_super * 4 + 15) & ~(size_t)15));
    // (kernels run on the handle's stream only — the copy stream carries copies: see rec_compact_piece)
    KMMCHK(stage_copies_done(ix));
    HIPCHK(hipMemsetAsync(tile_cnt, 0, (size_t)n_super * 1024 * 4, ix->stream));
    hipLaunchKernelGGL(k_rec_count, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, ix->stream,
                       rv.bases, n_bytes, n_tiles, tile_cnt);
    hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, ix->stream, tile_cnt, super_tot);
    // ("record_pairs", DESIGN 4.21: the piece ends behind a mate 2 — the census counts pairs, records of twice the lines)
    const bool pairs = record_pairs_on(ix);
    hipLaunchKernelGGL(k_rec_scan2, dim3(1), dim3(1024), 0, ix->stream, rv.bases, n_bytes, n_super,
                       tile_cnt, super_tot, (uint32_t)format * (pairs ? 2u : 1u), d_out, 1024);
    HIPCHK(hipGetLastError());
    int64_t out[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream)); // (it waited for the copy: the borrowed host buffer is free from here on)
    if (pairs)
        out[1] *= 2;
    *consumed = out[0];
    *n_records = out[1];
    if (out[0] > 0) {
        rv.total = out[0];
        rv.first_bad = ix->first_bad;
        rv.tile_nl = tile_cnt;
        rv.super_nl = super_tot;
        rv.period_mask = (uint32_t)format - 1u;
        rv.header_char = format == KMM_FORMAT_FASTQ ? (uint32_t)'@' : (uint32_t)'>';
        KMMCHK(stage_copies_done(ix));
        if (ix->record_hits) {
            // the record-hits mode: one zeroed entry per record of the piece behind the pending ones, then the
            // membership kernel on the same front end; the node counts, the per-k-mer counts and the statistics stay untouched
            uint32_t *q_hits = nullptr, *q_win = nullptr;
            KMMCHK(ensure_direct(ix));
            KMMCHK(rhq_reserve(ix, out[1], &q_hits, &q_win, pairs));
            if (ix->record_hits != 2)
                q_win = nullptr;
            if (const int qual = records_quality(ix, format))
                KMMCHK(rq_mark_piece(ix, s, rv, out[1], qual));
            KMMCHK(launch_record_hits(ix, rv, has_break, k, max_freq, also_revcomp ? 1 : 0, q_hits, q_win));
            ix->rhq_pending += out[1];
            if (pairs && ix->rk_raw_call) // ("record_bam_mates", DESIGN 4.25: whole pairs of entries; the bytes and the mate check are
                ix->bam_pairs_done += out[1] / 2; // kmm_map_bam's, over the records themselves — this text has no names)
            else if (pairs)
                KMMCHK(record_keep_piece<2>(ix, ix->rkq[0], rv, n_bytes, out[0], out[1], q_hits, q_win));
            else if (ix->record_keep && !ix->rk_raw_call) // ("record_bam", DESIGN 4.24: kmm_map_bam appends the records' own bytes)
                KMMCHK(record_keep_piece<0>(ix, ix->rkq[0], rv, n_bytes, out[0], out[1], q_hits, q_win));
            if (pairs && ix->rk_mates_call && !ix->rk_raw_call) {
                // (the text is kmm_map_bam's — neighbours that are no mates fail the call, which puts back what
                // its pieces appended)
                uint32_t bad = 0xFFFFFFFFu;
                KMMCHK(pair_names_piece(ix, rv, out[0], &bad));
                if (bad != 0xFFFFFFFFu) {
                    const long long p = (long long)(ix->bam_pairs_done + (int64_t)bad);
                    (void)stage_release(ix, s, false);
                    return fail(KMM_ERR_MALFORMED, "kmm_map_bam: \"record_names_pairs\" is 1 and pair %lld of the stream is none: records "
                                "%lld and %lld are not mates: collate the file by name (`samtools collate`) and exclude secondary and "
                                "supplementary records (0x900) (nothing of the call is appended)", p, 2 * p, 2 * p + 1);
                }
                ix->bam_pairs_done += out[1] / 2;
            }
        } else if (has_break) // (a break byte on a sequence line: a break like the bytes outside the sequence lines)
            KMMCHK(launch_map_reads<MODE_RECORDS_BRK>(ix, rv, k, max_freq, also_revcomp ? 1 : 0));
        else
            KMMCHK(launch_map_reads<MODE_RECORDS>(ix, rv, k, max_freq, also_revcomp ? 1 : 0));
    }
    return stage_release(ix, s, false);
}

// One piece of a multi-line FASTA chunk: unwrapped on the device into two-line FASTA (kmm_records.hpp k_ml_*), then
// mapped like one.  Only whole records are taken: up to the start of the chunk's last header line, or all of it when
// the caller says the chunk ends the file.
static int map_multiline_piece(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, bool last, int k, int max_freq,
                               int also_revcomp, const uint8_t *lut, int64_t *consumed, int64_t *n_records)
{
    *consumed = 0;
    *n_records = 0;
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    bool staged = false;
    const uint8_t *d_raw = nullptr;
    KMMCHK(stage_in<uint8_t>(ix, s.bases, raw, (size_t)n_bytes, &d_raw, &staged));
    const int64_t n_tiles = (n_bytes + 1023) / 1024;
    const int n_super = (int)((n_tiles + 1023) / 1024);
    KMMCHK(ensure(s.tile_first, (size_t)n_super * 1024 * 4));
    KMMCHK(ensure(s.offsets, (size_t)n_super * 4 + 64));
    KMMCHK(ensure(s.start_bits, (size_t)n_tiles * 8 + 64));
    KMMCHK(ensure(s.kmers, (size_t)n_bytes + 16));
    uint32_t *tile_cnt = (uint32_t *)s.tile_first.p;
    uint32_t *super_tot = (uint32_t *)s.offsets.p;
    uint8_t *cells = (uint8_t *)s.offsets.p + (((size_t)n_super * 4 + 15) & ~(size_t)15);
    uint32_t *d_total = (uint32_t *)cells;                       // kept bytes of the whole chunk
    int *d_lone_cr = (int *)(cells + 4);                         // first '\r' of a sequence line without '\n' (0x7F7F7F7F: none)
    int *d_last_header = (int *)(cells + 8);                     // start of the last header line (-1: none)
    unsigned long long *d_out_len = (unsigned long long *)(cells + 16);
    int32_t *tile_last = (int32_t *)s.start_bits.p, *tile_prev = tile_last + n_tiles;
    uint8_t *unwrapped = (uint8_t *)s.kmers.p;
    KMMCHK(stage_copies_done(ix));
    hipStream_t cs = ix->stream; // (kernels run on the handle's stream only: see rec_compact_piece)
    HIPCHK(hipMemsetAsync(tile_cnt, 0, (size_t)n_super * 1024 * 4, cs));
    HIPCHK(hipMemsetAsync(d_last_header, 0xFF, 4, cs));
    HIPCHK(hipMemsetAsync(d_lone_cr, 0x7F, 4, cs)); // (beyond every position of a piece: pieces have at most 2^30 bytes)
    const dim3 g4((unsigned)((n_tiles + 3) / 4));
    hipLaunchKernelGGL(k_ml_tile_last, g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_last);
    hipLaunchKernelGGL(k_ml_scan, dim3(1), dim3(1024), 0, cs, tile_last, n_tiles, tile_prev);
    hipLaunchKernelGGL(k_ml_flags, g4, dim3(256), 0, cs, d_raw, n_bytes, n_tiles, tile_prev, tile_cnt, d_last_header,
                       d_lone_cr);
    hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, cs, tile_cnt, super_tot);
    hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, cs, super_tot, n_super, d_total);
    HIPCHK(hipGetLastError());
    struct { uint32_t total; int lone_cr; int last_header; } h = {0, 0x7F7F7F7F, -1};
    HIPCHK(hipMemcpyAsync(&h, cells, 12, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipStreamSynchronize(cs)); // (the borrowed host buffer is free from here on)
    const int64_t limit = last ? n_bytes : (h.last_header > 0 ? (int64_t)h.last_header : 0);
    if ((int64_t)h.lone_cr < limit) {
        (void)stage_release(ix, s, false);
        return fail(KMM_ERR_MALFORMED, "multi-line FASTA chunk: the '\\r' at byte %d of the piece is not followed by '\\n' (nothing of "
                    "the piece is mapped)", h.lone_cr);
    }
    int64_t out_len = 0;
    if (limit > 0) {
        unsigned long long ol = h.total;
        if (limit < n_bytes) {
            HIPCHK(hipMemsetAsync(d_out_len, 0, 8, cs));
        }
        hipLaunchKernelGGL(k_ml_scatter, g4, dim3(256), 0, cs, d_raw, n_bytes, limit, n_tiles, tile_prev, tile_cnt, super_tot,
                           unwrapped, d_out_len);
        HIPCHK(hipGetLastError());
        if (limit < n_bytes) {
            HIPCHK(hipMemcpyAsync(&ol, d_out_len, 8, hipMemcpyDeviceToHost, cs));
            HIPCHK(hipStreamSynchronize(cs));
        }
        out_len = (int64_t)ol;
    }
    int rc = KMM_OK;
    if (out_len > 0) {
        // the unwrapped records, from HBM, through the two-line parser (its kernels wait for the copy stream)
        int64_t used = 0;
        rc = map_records_piece(ix, unwrapped, out_len, KMM_FORMAT_FASTA2, k, max_freq, also_revcomp, lut, &used, n_records);
        if (rc == KMM_OK && used != out_len)
            rc = fail(KMM_ERR_MALFORMED, "multi-line FASTA chunk: %lld of %lld unwrapped bytes form whole records (a record "
                      "without a sequence line, or bytes before the first '>')", (long long)used, (long long)out_len);
        if (rc == KMM_OK)
            *consumed = limit;
    }
    const int rel = stage_release(ix, s, false); // (after the inner call's kernels: they read this stage's buffer)
    return rc != KMM_OK ? rc : rel;
}

// The selection a SAM (by_name) / BAM call runs under: the masks, the floor and — with a region list set — the interval list of
// that front end in the handle's device buffer.  A list that cannot serve the front end is refused here, before anything is
// mapped: regions without a name for SAM; for BAM, regions without an id, or an id outside [0, n_ref) of the stream.
static int selection_of(const kmm_index_t *ix, const char *who, bool by_name, int32_t n_ref, kmm_sel::Sel &sel)
{
    sel = kmm_sel::Sel();
    sel.excl = ix->bam_excl;
    sel.incl = ix->bam_incl;
    sel.min_mapq = ix->bam_min_mapq;
    if (ix->sel_n_regions == 0)
        return KMM_OK;
    const std::vector<kmm_sel::Interval> &iv = by_name ? ix->sel_iv_name : ix->sel_iv_id;
    if (iv.empty())
        return fail(KMM_ERR_INVALID_ARG, by_name ? "%s: the region list of kmm_set_record_regions has a region without ref_name, which SAM "
                                                   "records are selected by (nothing is mapped)"
                                                 : "%s: the region list of kmm_set_record_regions has a region without ref_id (negative), which "
                                                   "BAM records are selected by (nothing is mapped)", who);
    if (!by_name && iv.back().ref >= (int64_t)n_ref)
        return fail(KMM_ERR_INVALID_ARG, "%s: the region list names ref_id %lld, the stream has %d references (nothing is mapped)", who,
                    (long long)iv.back().ref, (int)n_ref);
    const uint8_t *b = (const uint8_t *)ix->sel_buf.p;
    sel.n_iv = (uint32_t)iv.size();
    sel.keep_unplaced = ix->sel_keep_unplaced ? 1u : 0u;
    sel.iv = (const kmm_sel::Interval *)(by_name ? b + ix->sel_off_name_iv : b);
    if (by_name) {
        sel.n_names = (uint32_t)ix->sel_names.size();
        sel.name_off = (const uint32_t *)(b + ix->sel_off_name_off);
        sel.names = b + ix->sel_off_names;
    }
    return KMM_OK;
}

static int map_records_entry(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int format, int k, int max_freq, int also_revcomp,
                             const uint8_t *lut, int64_t *consumed, int64_t *n_records);

namespace {
#include "kmm_sam_host.hpp" // map_sam_piece, sam_raw_piece: behind the stages and map_records_piece, in front of kmm_map_records
} // namespace

int kmm_map_records(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int format, int k,
                    int max_freq, int also_revcomp, const uint8_t *lut, int64_t *consumed,
                    int64_t *n_records)
{
    return guarded("kmm_map_records", [&] {
        const int64_t pending0 = ix ? ix->rhq_pending : 0, bound0 = ix ? ix->rkq[0].bound : 0;
        const bool keep = ix && ix->record_keep && ix->record_hits;
        if (ix)
            ix->rk_snap.valid = false;
        if (keep) { // the queue's tail as the call finds it, kept on the device: a call that fails puts it back
            HIPCHK(hipSetDevice(ix->device));
            KMMCHK(rkq_mark(ix, ix->rkq[0]));
            ix->rk_snap.pending = pending0;
            ix->rk_snap.bound = bound0;
            ix->rk_snap.valid = true; // (a stream call that finds its last chunk ending with an unpaired record: keep_carry)
        }
        const int rc = map_records_entry(ix, raw, n_bytes, format, k, max_freq, also_revcomp, lut, consumed, n_records);
        if (rc != KMM_OK && ix)
            ix->rhq_pending = pending0; // (record-hits mode: a call that fails reports no record and appends no entry)
        if (rc != KMM_OK && keep)
            rkq_rollback(ix, ix->rkq[0], bound0);
        return rc;
    });
}

static int map_records_entry(kmm_index_t *ix, const uint8_t *raw, int64_t n_bytes, int format, int k, int max_freq, int also_revcomp,
                             const uint8_t *lut, int64_t *consumed, int64_t *n_records)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(check_k(k));
    const bool last_chunk = (format & KMM_FORMAT_LAST_CHUNK) != 0;
    format &= ~KMM_FORMAT_LAST_CHUNK;
    if (format != KMM_FORMAT_FASTQ && format != KMM_FORMAT_FASTA2 && format != KMM_FORMAT_FASTA && format != KMM_FORMAT_SAM)
        return fail(KMM_ERR_INVALID_ARG, "format must be KMM_FORMAT_FASTQ (4), KMM_FORMAT_FASTA2 (2), KMM_FORMAT_FASTA (1) or "
                    "KMM_FORMAT_SAM (8)");
    if (n_bytes < 0)
        return fail(KMM_ERR_INVALID_ARG, "n_bytes negative");
    if (consumed)
        *consumed = 0;
    if (n_records)
        *n_records = 0;
    // ("record_sam_mates", DESIGN 4.28: a last call that brings no byte can still leave a mate 1 alone)
    const bool sam_mates = format == KMM_FORMAT_SAM && sam_raw_mates_on(ix);
    if (n_bytes == 0 && last_chunk && sam_mates && ix->sam_mate_len > 0)
        return sam_unpaired_end("kmm_map_records", 2 * ix->sam_pairs_done + 1);
    if (n_bytes == 0)
        return KMM_OK;
    if (!raw)
        return fail(KMM_ERR_INVALID_ARG, "raw is NULL");
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(check_k_lut(k, lut));
    KMMCHK(refuse_quality_in_record_hits(ix, "kmm_map_records"));
    const bool sam_lines = format == KMM_FORMAT_SAM && ix->record_sam != 0; // ("record_sam", DESIGN 4.26: read by SAM calls alone)
    if (sam_lines)
        KMMCHK(refuse_record_sam(ix, "kmm_map_records"));
    if (sam_lines)
        KMMCHK(refuse_floor_with_record_sam(ix, "kmm_map_records"));
    KMMCHK(refuse_record_keep(ix, "kmm_map_records", format == KMM_FORMAT_SAM, sam_lines, format == KMM_FORMAT_FASTA));
    KMMCHK(check_quality(ix, "kmm_map_records", k, format == KMM_FORMAT_SAM));
    // A quality floor on FASTQ: always compaction + the radix path, whatever the batch size and "path" say (as kmm_map_packed) —
    // the records front end of the direct path has no flat positions to put a quality mark on — and never the host packer,
    // whose parser skips the quality lines.
    // (SAM with "use_record_qual" comes back here as FASTQ text, piece by piece: map_sam_piece)
    // (the record-hits mode keeps the direct front end under its own floor: rq_mark_piece)
    if (!ix->record_hits && records_quality(ix, format) > 0) {
        if (!ix->rx_ok)
            return fail(KMM_ERR_INVALID_ARG, "kmm_map_records: min_base_quality needs the radix path, which is not available for this "
                        "index (kmm_get_param \"radix_unavailable_reason\")");
        if (ix->dbg_rec_skip)
            return fail(KMM_ERR_INVALID_ARG, "kmm_map_records: min_base_quality does not go with debug_records_skip");
        return map_records_radix_call(ix, raw, n_bytes, format, k, max_freq, also_revcomp, lut, consumed, n_records);
    }
    // chunks beyond 2^30 bytes are mapped piece by piece: every piece starts where the previous one's last complete
    // record ended, so the pieces cut the chunk exactly as one census over all of it would
    // (multi-line FASTA and SAM are turned into two-line FASTA on the device first: never the host packer, whose parser knows
    // FASTQ and two-line FASTA only)
    // (the record-hits mode takes the direct records front end at every size: neither the radix path nor the host packer)
    if (!ix->record_hits && format != KMM_FORMAT_FASTA && format != KMM_FORMAT_SAM && records_take_radix(ix, n_bytes, format)) {
        // raw bytes in host memory: the host threads pack the sequence lines to 2 bits per base before they cross PCIe
        if (ix->host_pack_threads > 0 && !lut && !ix->dbg_rec_skip && !ix->dbg_rec_copy_stream && !is_device_ptr(raw)) {
            bool done = false;
            KMMCHK(map_records_host_packed(ix, raw, n_bytes, format, k, max_freq, also_revcomp, consumed, n_records, &done));
            if (done)
                return KMM_OK;
        }
        return map_records_radix_call(ix, raw, n_bytes, format, k, max_freq, also_revcomp, lut, consumed, n_records);
    }
    const int64_t piece_max = records_piece_max(ix);
    int64_t off = 0, recs = 0;
    SamMatesUndo sam_undo(ix, sam_mates); // (the pair form of "record_sam": a failing call leaves the waiting mate and the counters alone)
    if (format == KMM_FORMAT_SAM && n_bytes > piece_max) {
        // a SAM chunk of several pieces is checked whole first: a malformed line in a later piece maps nothing of the call
        while (off < n_bytes) {
            const int64_t len = n_bytes - off < piece_max ? n_bytes - off : piece_max;
            int64_t used = 0, nr = 0;
            KMMCHK(map_sam_piece(ix, raw + off, len, off, true, k, max_freq, also_revcomp, lut, &used, &nr));
            off += used;
            if (used == 0 || len < piece_max)
                break;
        }
        off = 0;
    }
    while (off < n_bytes) {
        const int64_t len = n_bytes - off < piece_max ? n_bytes - off : piece_max;
        int64_t used = 0, nr = 0;
        if (format == KMM_FORMAT_SAM)
            KMMCHK(map_sam_piece(ix, raw + off, len, off, false, k, max_freq, also_revcomp, lut, &used, &nr));
        else if (format == KMM_FORMAT_FASTA)
            KMMCHK(map_multiline_piece(ix, raw + off, len, last_chunk && off + len == n_bytes, k, max_freq, also_revcomp, lut,
                                       &used, &nr));
        else {
            ix->rq_text_off = off; // (read by rq_mark_piece while kmm_map_bam's named form has set rq_exempt)
            KMMCHK(map_records_piece(ix, raw + off, len, format, k, max_freq, also_revcomp, lut, &used, &nr));
        }
        // a multi-line FASTA record that fills a whole piece: no later piece, no longer chunk and no further call can ever
        // complete it, and with KMM_FORMAT_LAST_CHUNK the rest of the file would be dropped behind a KMM_OK
        if (format == KMM_FORMAT_FASTA && used == 0 && len == piece_max)
            return fail(KMM_ERR_MALFORMED, "kmm_map_records: multi-line FASTA: the piece at byte %lld of the chunk holds no whole "
                        "record: one record exceeds a piece of %lld bytes (the pieces before it are already counted)",
                        (long long)off, (long long)piece_max);
        off += used;
        recs += nr;
        if (used == 0 || len < piece_max)
            break; // no complete record left in reach / the last piece
    }
    // (a mate 1 that waits behind the stream's last line has no mate; a line longer than a piece, which ends the call in front of
    // it, is brought again: the stream goes on)
    if (sam_mates && last_chunk && ix->sam_mate_len > 0 && n_bytes - off < piece_max)
        return sam_unpaired_end("kmm_map_records", 2 * ix->sam_pairs_done + 1);
    sam_undo.armed = false;
    if (format == KMM_FORMAT_SAM)
        ix->sam_calls++;
    if (consumed)
        *consumed = off;
    if (n_records)
        *n_records = recs;
    return KMM_OK;
}

// ---- kmm_map_record_pairs: the mates of a pair in two buffers, record i of one beside record i of the other.
// One buffer's piece of a piece pair: its stage, its census (as map_records_piece takes it) and where it is cut.
struct PairSide {
    Stage *s = nullptr;
    ReadsView rv;
    int64_t len = 0, cut = 0;
    int n_super = 0;
    uint32_t *tile_cnt = nullptr, *super_tot = nullptr;
    int64_t *d_out = nullptr; // {consumed, n_records, n_lines} of k_rec_scan2, {cut} of k_rec_cut
    int64_t out[4] = {0, 0, 0, 0};
};

static int pair_side_census(kmm_index_t *ix, PairSide &p, const uint8_t *raw, int64_t len, int format)
{
    memset(&p.rv, 0, sizeof p.rv);
    p.len = len;
    if (len == 0)
        return KMM_OK;
    bool staged = false;
    KMMCHK(stage_in<uint8_t>(ix, p.s->bases, raw, (size_t)len, &p.rv.bases, &staged));
    const int64_t n_tiles = (len + TILE_T - 1) / TILE_T;
    p.n_super = (int)((n_tiles + 1023) / 1024);
    KMMCHK(ensure(p.s->tile_first, (size_t)p.n_super * 1024 * 4));
    KMMCHK(ensure(p.s->offsets, (size_t)p.n_super * 4 + 64));
    p.tile_cnt = (uint32_t *)p.s->tile_first.p;
    p.super_tot = (uint32_t *)p.s->offsets.p;
    p.d_out = (int64_t *)((uint8_t *)p.s->offsets.p + (((size_t)p.n_super * 4 + 15) & ~(size_t)15));
    KMMCHK(stage_copies_done(ix));
    HIPCHK(hipMemsetAsync(p.tile_cnt, 0, (size_t)p.n_super * 1024 * 4, ix->stream));
    hipLaunchKernelGGL(k_rec_count, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, ix->stream, p.rv.bases, len, n_tiles, p.tile_cnt);
    hipLaunchKernelGGL(k_rec_scan1, dim3(p.n_super), dim3(1024), 0, ix->stream, p.tile_cnt, p.super_tot);
    hipLaunchKernelGGL(k_rec_scan2, dim3(1), dim3(1024), 0, ix->stream, p.rv.bases, len, p.n_super, p.tile_cnt, p.super_tot,
                       (uint32_t)format, p.d_out, 1024);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(p.out, p.d_out, 24, hipMemcpyDeviceToHost, ix->stream));
    return KMM_OK;
}

// One piece pair: both censuses, the cut of the buffer that holds more whole records than the other, the hit kernel once per
// buffer, the entries zipped into the queue in pair order, the pair forms of the keep kernels once per buffer.
static int map_record_pairs_piece(kmm_index_t *ix, const uint8_t *raw1, int64_t len1, const uint8_t *raw2, int64_t len2, int format, int k,
                                  int max_freq, int also_revcomp, const uint8_t *lut, int64_t *used1, int64_t *used2, int64_t *n_pairs)
{
    *used1 = *used2 = *n_pairs = 0;
    PairSide side[2];
    side[0].s = &next_stage(ix);
    side[1].s = &next_stage(ix);
    KMMCHK(stage_acquire(ix, *side[0].s));
    KMMCHK(stage_acquire(ix, *side[1].s));
    ix->map_calls++;
    bool staged = false, has_break = false;
    const uint8_t *d_lut = nullptr;
    KMMCHK(resolve_lut(ix, *side[0].s, lut, &d_lut, &staged, &has_break));
    KMMCHK(pair_side_census(ix, side[0], raw1, len1, format));
    KMMCHK(pair_side_census(ix, side[1], raw2, len2, format));
    HIPCHK(hipStreamSynchronize(ix->stream)); // (it waited for the copies: the borrowed host buffers are free from here on)
    const int64_t m = side[0].out[1] < side[1].out[1] ? side[0].out[1] : side[1].out[1];
    bool cuts = false;
    for (PairSide &p : side) {
        p.cut = p.out[0];
        if (m == 0 || p.out[1] == m)
            continue;
        // more whole records than the other buffer: the byte behind record m, line m * format of the census
        hipLaunchKernelGGL(k_rec_cut, dim3(1), dim3(1024), 0, ix->stream, p.rv.bases, p.len, p.n_super, (const uint32_t *)p.tile_cnt,
                           (const uint32_t *)p.super_tot, (const int64_t *)p.d_out, (uint32_t)(m * format), p.d_out + 3);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&p.cut, p.d_out + 3, 8, hipMemcpyDeviceToHost, ix->stream));
        cuts = true;
    }
    if (cuts)
        HIPCHK(hipStreamSynchronize(ix->stream));
    if (m > 0) {
        for (const PairSide &p : side)
            if (p.cut <= 0 || p.cut > p.out[0])
                return fail(KMM_ERR_INTERNAL, "kmm_map_record_pairs: record %lld of a buffer with %lld whole records in %lld bytes ends "
                            "at byte %lld", (long long)m, (long long)p.out[1], (long long)p.out[0], (long long)p.cut);
        uint32_t *q_hits = nullptr, *q_win = nullptr;
        KMMCHK(ensure_direct(ix));
        KMMCHK(rhq_reserve(ix, 2 * m, &q_hits, &q_win, true));
        if (ix->record_hits != 2)
            q_win = nullptr;
        // (the entries of each buffer by themselves first — sums of atomics, zeroed — then zipped: entry 2i is mate 1 of pair i)
        const size_t stride = ((size_t)m + 63) & ~(size_t)63;
        KMMCHK(ensure(ix->rk_pair_entries, stride * 16));
        uint32_t *e = (uint32_t *)ix->rk_pair_entries.p;
        HIPCHK(hipMemsetAsync(e, 0, stride * 16, ix->stream));
        KMMCHK(stage_copies_done(ix)); // (a lookup table staged from the host)
        for (int i = 0; i < 2; ++i) {
            PairSide &p = side[i];
            p.rv.total = p.cut;
            p.rv.lut = d_lut;
            p.rv.first_bad = ix->first_bad;
            p.rv.tile_nl = p.tile_cnt;
            p.rv.super_nl = p.super_tot;
            p.rv.period_mask = (uint32_t)format - 1u;
            p.rv.header_char = format == KMM_FORMAT_FASTQ ? (uint32_t)'@' : (uint32_t)'>';
            uint32_t *h = e + (size_t)i * stride, *w = q_win ? e + (size_t)(2 + i) * stride : nullptr;
            if (const int qual = records_quality(ix, format))
                KMMCHK(rq_mark_piece(ix, *p.s, p.rv, m, qual));
            KMMCHK(launch_record_hits(ix, p.rv, has_break, k, max_freq, also_revcomp ? 1 : 0, h, w));
        }
        const dim3 gz((unsigned)grid_for(ix, (m + 255) / 256, 8));
        hipLaunchKernelGGL(k_rk_zip, gz, dim3(256), 0, ix->stream, (const uint32_t *)e, (const uint32_t *)(e + stride), m, q_hits);
        if (q_win)
            hipLaunchKernelGGL(k_rk_zip, gz, dim3(256), 0, ix->stream, (const uint32_t *)(e + 2 * stride), (const uint32_t *)(e + 3 * stride), m,
                               q_win);
        HIPCHK(hipGetLastError());
        ix->rhq_pending += 2 * m;
        for (int i = 0; i < 2; ++i)
            KMMCHK(record_keep_piece<1>(ix, ix->rkq[i], side[i].rv, side[i].len, side[i].cut, m, q_hits, q_win));
        *used1 = side[0].cut;
        *used2 = side[1].cut;
        *n_pairs = m;
    }
    KMMCHK(stage_release(ix, *side[0].s, false));
    return stage_release(ix, *side[1].s, false);
}

static int map_record_pairs_entry(kmm_index_t *ix, const uint8_t *raw1, int64_t n1, const uint8_t *raw2, int64_t n2, int format, int k,
                                  int max_freq, int also_revcomp, const uint8_t *lut, int64_t *consumed1, int64_t *consumed2,
                                  int64_t *n_pairs)
{
    const char *who = "kmm_map_record_pairs";
    KMMCHK(check_k(k));
    if (format != KMM_FORMAT_FASTQ && format != KMM_FORMAT_FASTA2)
        return fail(KMM_ERR_INVALID_ARG, "%s: format must be KMM_FORMAT_FASTQ (4) or KMM_FORMAT_FASTA2 (2), the same for both buffers "
                    "(nothing is mapped)", who);
    if (n1 < 0 || n2 < 0)
        return fail(KMM_ERR_INVALID_ARG, "%s: n1 or n2 negative", who);
    if ((n1 > 0 && !raw1) || (n2 > 0 && !raw2))
        return fail(KMM_ERR_INVALID_ARG, "%s: raw1 or raw2 is NULL", who);
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(check_k_lut(k, lut));
    KMMCHK(refuse_quality_in_record_hits(ix, who));
    if (!ix->record_hits || !ix->record_keep)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_hits\" is %d and \"record_keep\" is %d: the call appends the entries and the kept "
                    "text of both mates, set \"record_hits\" to 1 or 2 and \"record_keep\" to 1 (nothing is mapped)", who, ix->record_hits,
                    ix->record_keep);
    if (ix->rk_min_permille > 0 && ix->record_hits != 2)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_keep_min_permille\" is %d and \"record_hits\" is 1: the rule needs the windows, "
                    "which mode 2 keeps (nothing is mapped)", who, ix->rk_min_permille);
    const int64_t piece_max = records_piece_max(ix);
    int64_t off1 = 0, off2 = 0, pairs = 0;
    while (off1 < n1 && off2 < n2) {
        const int64_t len1 = n1 - off1 < piece_max ? n1 - off1 : piece_max, len2 = n2 - off2 < piece_max ? n2 - off2 : piece_max;
        int64_t used1 = 0, used2 = 0, m = 0;
        KMMCHK(map_record_pairs_piece(ix, raw1 + off1, len1, raw2 + off2, len2, format, k, max_freq, also_revcomp, lut, &used1, &used2, &m));
        off1 += used1;
        off2 += used2;
        pairs += m;
        if (m == 0 || (len1 < piece_max && len2 < piece_max))
            break; // no complete pair left in reach / the last piece pair
    }
    *consumed1 = off1;
    *consumed2 = off2;
    *n_pairs = pairs;
    return KMM_OK;
}

int kmm_map_record_pairs(kmm_index_t *ix, const uint8_t *raw1, int64_t n1, const uint8_t *raw2, int64_t n2, int format, int k,
                         int max_freq, int also_revcomp, const uint8_t *lut, int64_t *consumed1, int64_t *consumed2, int64_t *n_pairs)
{
    return guarded("kmm_map_record_pairs", [&] {
        if (!ix || !consumed1 || !consumed2 || !n_pairs)
            return fail(KMM_ERR_INVALID_ARG, "NULL argument");
        *consumed1 = *consumed2 = *n_pairs = 0;
        const int64_t pending0 = ix->rhq_pending, bound0[2] = {ix->rkq[0].bound, ix->rkq[1].bound};
        const bool keep = ix->record_keep && ix->record_hits;
        ix->rk_snap.valid = false;
        if (keep) { // both queues' tails as the call finds them, kept on the device: a call that fails puts them back
            HIPCHK(hipSetDevice(ix->device));
            KMMCHK(rkq_mark(ix, ix->rkq[0]));
            KMMCHK(rkq_mark(ix, ix->rkq[1]));
        }
        const int rc = map_record_pairs_entry(ix, raw1, n1, raw2, n2, format, k, max_freq, also_revcomp, lut, consumed1, consumed2, n_pairs);
        if (rc != KMM_OK) {
            ix->rhq_pending = pending0;
            *consumed1 = *consumed2 = *n_pairs = 0;
            if (keep) {
                rkq_rollback(ix, ix->rkq[0], bound0[0]);
                rkq_rollback(ix, ix->rkq[1], bound0[1]);
            }
        }
        return rc;
    });
}

int kmm_map_packed(kmm_index_t *ix, const uint32_t *codes, int64_t n_bases, int64_t n_reads, int64_t read_len,
                   const uint32_t *read_starts, int k, int max_freq, int also_revcomp)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(refuse_in_record_hits(ix, "kmm_map_packed"));
    KMMCHK(check_k(k));
    if (n_bases < 0 || n_reads < 0 || read_len < 0)
        return fail(KMM_ERR_INVALID_ARG, "n_bases / n_reads / read_len negative");
    if (n_bases == 0)
        return KMM_OK;
    if (!codes)
        return fail(KMM_ERR_INVALID_ARG, "codes is NULL");
    if (read_len > 0 ? n_reads * read_len != n_bases : !read_starts)
        return fail(KMM_ERR_INVALID_ARG, read_len > 0 ? "n_reads * read_len != n_bases" : "read_starts is NULL and read_len is 0");
    if (!ix->rx_ok)
        return fail(KMM_ERR_INVALID_ARG, "packed reads are mapped by the radix path, which is not available for this index "
                    "(kmm_get_param \"radix_unavailable_reason\")");
    HIPCHK(hipSetDevice(ix->device));
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    ix->map_calls++;
    bool staged = false;
    const uint32_t *d_codes = nullptr, *d_starts = nullptr;
    KMMCHK(stage_in<uint32_t>(ix, s.kmers, codes, (size_t)((n_bases + 15) / 16), &d_codes, &staged));
    int64_t n_words = 0;
    if (read_len == 0) {
        n_words = n_bases / 32 + 1;
        KMMCHK(stage_in<uint32_t>(ix, s.start_bits, read_starts, (size_t)n_words, &d_starts, &staged));
    } else if (read_len < 16) { // (the uniform front ends need reads of at least 16 bases: shorter ones go as ragged reads)
        n_words = n_bases / 32 + 2;
        KMMCHK(ensure(s.offsets, (size_t)(n_reads + 1) * 8));
        KMMCHK(ensure(s.start_bits, (size_t)n_words * 4));
        HIPCHK(hipMemsetAsync(s.start_bits.p, 0, (size_t)n_words * 4, ix->stream));
        hipLaunchKernelGGL(k_iota_offsets, dim3((unsigned)((n_reads + 1 + 255) / 256)), dim3(256), 0, ix->stream, (int64_t *)s.offsets.p,
                           n_reads, read_len);
        hipLaunchKernelGGL(k_mark_starts, dim3(grid_for(ix, (n_reads + 256) / 256, 8)), dim3(256), 0, ix->stream,
                           (const int64_t *)s.offsets.p, n_reads, n_bases, (uint32_t *)s.start_bits.p);
        HIPCHK(hipGetLastError());
        d_starts = (const uint32_t *)s.start_bits.p;
    }
    KMMCHK(rec_launch_flat(ix, d_codes, n_bases, n_reads, d_starts, n_words, read_len >= 16 ? read_len : 0, k, max_freq, also_revcomp));
    return stage_release(ix, s, staged);
}


// Stages comp[pre, n_comp) to d_comp + pre through the page-locked ring (comp[0, pre) is there already: a member's head left
// over from the chunk before) and walks the member chain of comp[0, n_comp) behind the copying threads.  cap: inflated bytes
// the chain may hold.  all: n_comp is where the chunk ends (an incomplete last member ends the chain).
static int bgzf_stage_and_scan(kmm_index_t *ix, const uint8_t *comp, int64_t pre, int64_t n_comp, uint8_t *d_comp, unsigned long long out_cap,
                               BgzfStaged &st, bool walk = true)
{
    std::vector<unsigned long long> &m_off = st.m_off, &o_off = st.o_rel;
    m_off.assign(1, 0ull);
    o_off.assign(1, 0ull); // (offsets relative to the chunk: the caller adds what it carries over)
    uint64_t &p = st.p;
    p = 0;
    bool chain_end = false;
    int &chain_err = st.chain_err;
    uint32_t &bad_isize = st.bad_isize, &bad_ms = st.bad_ms;
    chain_err = 0;
    bad_isize = bad_ms = 0;
    st.hit_cap = false; // (st may be the handle's prestaged chunk of an earlier call: nothing of that call's chain holds here)
    // walks the chain through comp[0, limit); all = the limit is the end of the chunk
    auto scan_upto = [&](uint64_t limit, bool all) {
        if (!walk) // (kmm_map_gzip: the ring only — a plain gzip stream has no member chain to walk)
            return;
        while (!chain_end && p + 18 <= limit) {
            const uint32_t ms = kmm_gz::bgzf_member_size(comp + p, limit - p);
            if (!ms) {
                // (a header that needs more bytes than are in reach: wait for them, or — at the end of the chunk — an
                // incomplete member that the caller brings again)
                const uint32_t xlen = (uint32_t)comp[p + 10] | ((uint32_t)comp[p + 11] << 8);
                if (comp[p] == 0x1f && comp[p + 1] == 0x8b && comp[p + 2] == 8 && (comp[p + 3] & 4) && p + 12 + xlen + 8 > limit) {
                    chain_end = all;
                    return;
                }
                chain_err = 1;
                chain_end = true;
                return;
            }
            if (p + ms > limit) {
                chain_end = all; // (an incomplete member at the end of the chunk)
                return;
            }
            const uint32_t isize = kmm_gz::rd32(comp + p + ms - 4);
            if ((uint64_t)isize > (uint64_t)ms * 1032ull + 64ull) {
                chain_err = 2;
                bad_isize = isize;
                bad_ms = ms;
                chain_end = true;
                return;
            }
            if (o_off.back() + isize > out_cap && m_off.size() > 1) {
                st.hit_cap = true; // (the call stops at its own size limit: the caller continues with the same flags)
                chain_end = true;
                return;
            }
            p += ms;
            m_off.push_back(p);
            o_off.push_back(o_off.back() + isize);
        }
        if (all)
            chain_end = true;
    };
    bool &staged = st.staged;
    double &ms_scan_inside = st.ms_scan_inside;
    staged = false;
    ms_scan_inside = 0;
    // ("debug_bgzf_ring_slot_kb": tests wrap the ring many times with a small input)
    const size_t SLOT = ix->dbg_bgzf_slot_kb > 0 && ((size_t)ix->dbg_bgzf_slot_kb << 10) < RING_SLOT ? (size_t)ix->dbg_bgzf_slot_kb << 10 : RING_SLOT;
    const size_t SUB = SLOT < ((size_t)1 << 20) ? SLOT : (size_t)1 << 20;
    constexpr int SLOTS = RING_SLOTS;
    if (n_comp > pre && ensure_pack_pool(ix) && ensure_ring(ix)) {
        const size_t n_stage = (size_t)(n_comp - pre); // bytes to copy: [pre, n_comp)
        const size_t n_slots = (n_stage + SLOT - 1) / SLOT, n_sub = (n_stage + SUB - 1) / SUB;
        std::vector<std::atomic<uint32_t>> filled(n_slots); // 1 MiB pieces copied, per slot-sized piece
        for (auto &f : filled)
            f.store(0, std::memory_order_relaxed);
        std::atomic<size_t> next{0}, slots_free{(size_t)SLOTS}; // slot-sized pieces [0, slots_free) may be written
        std::atomic<bool> stop{false};
        const PinnedBuf *ring = ix->ring;
        ix->pack_pool->start([&](int) {
            for (;;) {
                const size_t c = next.fetch_add(1);
                if (c >= n_sub)
                    return;
                const size_t piece = c / (SLOT / SUB);
                int spins = 0;
                while (piece >= slots_free.load(std::memory_order_acquire) && !stop.load(std::memory_order_relaxed)) {
                    if (++spins < 2000) {
#if defined(__x86_64__)
                        __builtin_ia32_pause();
#endif
                    } else
                        std::this_thread::sleep_for(std::chrono::microseconds(50));
                }
                if (stop.load(std::memory_order_relaxed))
                    return;
                const size_t b0 = c * SUB, len = n_stage - b0 < SUB ? n_stage - b0 : SUB;
                memcpy(ring[piece % SLOTS].p + (b0 - piece * SLOT), comp + pre + b0, len);
                filled[piece].fetch_add(1, std::memory_order_release);
            }
        });
        int rc = KMM_OK;
        size_t landed = 0; // slot-sized pieces whose copy to HBM is known to have finished
        for (size_t c = 0; c < n_slots && rc == KMM_OK; ++c) {
            const size_t b0 = c * SLOT, len = n_stage - b0 < SLOT ? n_stage - b0 : SLOT;
            const uint32_t want = (uint32_t)((len + SUB - 1) / SUB);
            while (filled[c].load(std::memory_order_acquire) < want) {
                // meanwhile: slots whose copies have landed are handed back, the chain is walked through what is there
                bool did = false;
                while (landed + SLOTS < n_slots && landed < c) {
                    if (hipEventQuery(ix->bgzf_slot_ev[landed % SLOTS]) != hipSuccess) {
                        (void)hipGetLastError(); // ("not ready" is no error to keep)
                        break;
                    }
                    ++landed;
                    slots_free.store(landed + SLOTS, std::memory_order_release);
                    did = true;
                }
                if (!chain_end && !chain_err && c > 0) {
                    const auto t_s = std::chrono::steady_clock::now();
                    const uint64_t before = p;
                    scan_upto((uint64_t)pre + (uint64_t)b0, false);
                    ms_scan_inside += ms_since(t_s);
                    did = did || p != before;
                }
                if (!did)
                    std::this_thread::sleep_for(std::chrono::microseconds(20));
            }
            if (hipMemcpyAsync(d_comp + pre + b0, ring[c % SLOTS].p, len, hipMemcpyHostToDevice, ix->copy_stream) != hipSuccess ||
                hipEventRecord(ix->bgzf_slot_ev[c % SLOTS], ix->copy_stream) != hipSuccess)
                rc = fail(KMM_ERR_HIP, "copy of compressed bytes: %s", hipGetErrorString(hipGetLastError()));
            // a slot is written again only when its copy has landed: the oldest one is waited for when the ring is full
            while (rc == KMM_OK && landed + SLOTS < n_slots && landed + SLOTS <= c + 1) {
                if (hipEventSynchronize(ix->bgzf_slot_ev[landed % SLOTS]) != hipSuccess) {
                    rc = fail(KMM_ERR_HIP, "hipEventSynchronize: %s", hipGetErrorString(hipGetLastError()));
                    break;
                }
                ++landed;
                slots_free.store(landed + SLOTS, std::memory_order_release);
            }
        }
        if (rc != KMM_OK)
            stop.store(true);
        ix->pack_pool->wait();
        if (rc != KMM_OK) {
            (void)hipStreamSynchronize(ix->copy_stream);
            return rc;
        }
        staged = true;
    }
    scan_upto((uint64_t)n_comp, true);
    return KMM_OK;
}

int kmm_map_bgzf_hint_next(kmm_index_t *ix, const uint8_t *comp_next, int64_t n_next)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    ix->bgzf_hint_ptr = n_next > 0 ? comp_next : nullptr;
    ix->bgzf_hint_n = n_next > 0 ? n_next : 0;
    return KMM_OK;
}

// ---- Compressed read streams (kmm_map_bgzf, kmm_map_gzip, kmm_map_bam): one stream per handle, started by KMM_FORMAT_NEW_STREAM
// and ended by KMM_FORMAT_LAST_CHUNK; the inflated bytes behind a call's last complete record are carried to the next call.
struct StreamCall {
    const char *who;
    int k, max_freq, also_revcomp;
    const uint8_t *lut;
    int64_t *consumed_comp, *n_records;
    int fmt = 0; // the format without the stream flags (stream_call_start)
    bool new_stream = false, last_chunk = false;
    bool mid_stream = false; // KMM_FORMAT_MID_STREAM (kmm_map_bam): the stream begins behind the header, at "bgzf_head_skip"
};

// text: FASTQ, two-line FASTA or SAM (else BAM: the flags alone); chain: a BGZF member chain is walked in the caller's bytes
static int stream_call_start(kmm_index_t *ix, StreamCall &c, const uint8_t *comp, int64_t n_comp, int format, bool text, bool chain)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(check_k(c.k));
    KMMCHK(check_k_lut(c.k, c.lut));
    c.last_chunk = (format & KMM_FORMAT_LAST_CHUNK) != 0;
    c.new_stream = (format & KMM_FORMAT_NEW_STREAM) != 0;
    c.fmt = format & ~(KMM_FORMAT_LAST_CHUNK | KMM_FORMAT_NEW_STREAM);
    if (!text && (c.fmt & KMM_FORMAT_MID_STREAM)) { // (a text format keeps the bit and is refused below)
        c.mid_stream = true;
        c.fmt &= ~KMM_FORMAT_MID_STREAM;
    }
    if (text ? c.fmt != KMM_FORMAT_FASTQ && c.fmt != KMM_FORMAT_FASTA2 && c.fmt != KMM_FORMAT_SAM : c.fmt != 0)
        return fail(KMM_ERR_INVALID_ARG, text ? "%s: format must be KMM_FORMAT_FASTQ (4), KMM_FORMAT_FASTA2 (2) or KMM_FORMAT_SAM (8)"
                                              : "%s: flags take KMM_FORMAT_NEW_STREAM, KMM_FORMAT_LAST_CHUNK and KMM_FORMAT_MID_STREAM only", c.who);
    if (c.mid_stream && !c.new_stream)
        return fail(KMM_ERR_INVALID_ARG, "%s: KMM_FORMAT_MID_STREAM goes with KMM_FORMAT_NEW_STREAM, on a stream's first call", c.who);
    if (c.mid_stream && ix->bam_n_ref_param < 0)
        return fail(KMM_ERR_INVALID_ARG, "%s: KMM_FORMAT_MID_STREAM needs \"bam_n_ref\" (kmm_set_param): a stream that begins behind "
                                         "the header does not say how many references the file has", c.who);
    KMMCHK(refuse_quality_in_record_hits(ix, c.who));
    // ("record_names", DESIGN 4.20: kmm_map_bam alone — the text routes never read it, SAM text stays refused)
    if (!text && ix->record_names && !ix->record_hits)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_names\" is 1 and \"record_hits\" is 0: the named FASTQ form of the decode serves "
                    "the record-hits mode (and \"record_keep\"), set \"record_hits\" to 1 or 2, or \"record_names\" to 0 (nothing is mapped)",
                    c.who);
    // ("record_bam", DESIGN 4.24: kmm_map_bam alone, as "record_names" — one output form per queue, whole streams, no mates)
    if (!text && ix->record_bam) {
        if (!ix->record_hits || !ix->record_keep)
            return fail(KMM_ERR_INVALID_ARG, "%s: \"record_bam\" is 1 and \"%s\" is 0: the kept records' own bytes are appended under the "
                        "keep rule, which reads the entries of the record-hits mode; set \"record_hits\" to 1 or 2 and \"record_keep\" to 1, "
                        "or \"record_bam\" to 0 (nothing is mapped)", c.who, ix->record_hits ? "record_keep" : "record_hits");
        if (ix->record_names)
            return fail(KMM_ERR_INVALID_ARG, "%s: \"record_bam\" and \"record_names\" are 1: the queue of kept records takes one form, the "
                        "records' own bytes or their named FASTQ text; set one of them to 0 (nothing is mapped)", c.who);
        if (ix->record_names_pairs || ix->record_pairs)
            return fail(KMM_ERR_INVALID_ARG, "%s: \"record_bam\" and \"%s\" are 1: mates are not kept together in BAM output; set one of "
                        "them to 0 (nothing is mapped)", c.who, ix->record_names_pairs ? "record_names_pairs" : "record_pairs");
        if (c.mid_stream)
            return fail(KMM_ERR_INVALID_ARG, "%s: \"record_bam\" is 1 and the stream begins behind the header (KMM_FORMAT_MID_STREAM): a "
                        "rank's share of a file has no header to write in front of its records; map the file with one rank (nothing is "
                        "mapped)", c.who);
    }
    // ("record_bam_mates", DESIGN 4.25: read by kmm_map_bam alone, behind everything "record_bam" refuses)
    if (!text && ix->record_bam_mates && !ix->record_bam)
        return fail(KMM_ERR_INVALID_ARG, "%s: \"record_bam_mates\" is 1 and \"record_bam\" is 0: mates are kept together in the raw form "
                    "of the keep, set \"record_bam\" to 1 (with \"record_hits\" and \"record_keep\"), or \"record_bam_mates\" to 0; for "
                    "FASTQ output there is \"record_names_pairs\" (nothing is mapped)", c.who);
    // ("record_sam", DESIGN 4.26: read by the SAM text routes alone)
    const bool sam_lines = text && c.fmt == KMM_FORMAT_SAM && ix->record_sam != 0;
    if (sam_lines)
        KMMCHK(refuse_record_sam(ix, c.who));
    if (sam_lines)
        KMMCHK(refuse_floor_with_record_sam(ix, c.who));
    KMMCHK(refuse_record_keep(ix, c.who, !text || c.fmt == KMM_FORMAT_SAM,
                              sam_lines || (!text && (ix->record_names != 0 || ix->record_bam != 0))));
    KMMCHK(check_quality(ix, c.who, c.k, !text || c.fmt == KMM_FORMAT_SAM));
    if (n_comp < 0 || (n_comp > 0 && !comp))
        return fail(KMM_ERR_INVALID_ARG, "comp NULL or n_comp negative");
    if (c.consumed_comp)
        *c.consumed_comp = 0;
    if (c.n_records)
        *c.n_records = 0;
    if (n_comp > 0 && is_device_ptr(comp))
        return fail(KMM_ERR_INVALID_ARG, "%s takes the compressed bytes from host memory%s", c.who,
                    chain ? " (the member chain is read there)" : "");
    HIPCHK(hipSetDevice(ix->device));
    if (text && c.new_stream && c.fmt == KMM_FORMAT_SAM)
        sam_mates_drop(ix); // ("record_sam_mates", DESIGN 4.28: a mate 1 left over belongs to the stream before)
    return KMM_OK;
}

// A text stream's last call that has no inflated byte to map: under "record_sam_mates" a mate 1 that still waits has no mate.
static int sam_mates_empty_end(kmm_index_t *ix, const StreamCall &c)
{
    if (c.last_chunk && c.fmt == KMM_FORMAT_SAM && sam_raw_mates_on(ix) && ix->sam_mate_len > 0)
        return kmm_map_records(ix, nullptr, 0, c.fmt | KMM_FORMAT_LAST_CHUNK, c.k, c.max_freq, c.also_revcomp, c.lut, nullptr, nullptr);
    return KMM_OK;
}

static int ensure_crc_tables(kmm_index_t *ix) // the CRC32 tables (slicing by 8), once per handle
{
    if (ix->bgzf_crc.p)
        return KMM_OK;
    std::vector<uint32_t> t(kmm_gz::CRC_TABLE_WORDS);
    for (int kk = 0; kk < 8; ++kk)
        for (uint32_t bb = 0; bb < 256u; ++bb)
            t[(size_t)kk * 256 + bb] = kmm_gz::crc_table_entry(kk, bb);
    for (int kk = 0; kk < kmm_gz::CRC_SHIFT_WORDS; ++kk) // (x^(8 * 2^kk): a part's register moved forward by the bytes behind it)
        t[8 * 256 + kk] = kmm_gz::crc_shift_table_entry(kk);
    KMMCHK(ensure(ix->bgzf_crc, t.size() * 4));
    HIPCHK(hipMemcpy(ix->bgzf_crc.p, t.data(), t.size() * 4, hipMemcpyHostToDevice));
    return KMM_OK;
}

// The bytes behind a call's last complete record, d_raw[used, n_raw), are carried to the next call (none on the last one).
static int keep_carry(kmm_index_t *ix, const StreamCall &c, const uint8_t *d_raw, int64_t used, int64_t n_raw, DevBuf &carry,
                      int64_t &carry_len)
{
    const int64_t tail = n_raw - used;
    if (c.last_chunk && tail > 0 && record_pairs_on(ix)) {
        // ("record_pairs": a complete record behind the last whole pair stays unconsumed like an incomplete one; nothing of the
        // call stays in the queues — the pairs in front of it were appended by the call's kmm_map_records, which succeeded)
        carry_len = 0;
        rk_snap_restore(ix);
        return fail(KMM_ERR_MALFORMED, "%s: \"record_pairs\" is 1 and the stream ends with an unpaired record: the last %lld bytes "
                    "form no complete pair of records (nothing of the call is appended)", c.who, (long long)tail);
    }
    if (c.last_chunk && tail > 0) {
        carry_len = 0;
        return fail(KMM_ERR_MALFORMED, "%s: the stream ends with %lld bytes that form no complete record", c.who, (long long)tail);
    }
    if (tail > 0) {
        KMMCHK(ensure(carry, (size_t)tail + 64)); // (may free and reallocate: a device-wide sync, rare)
        HIPCHK(hipMemcpyAsync(carry.p, d_raw + used, (size_t)tail, hipMemcpyDeviceToDevice, ix->stream));
    }
    carry_len = tail;
    return KMM_OK;
}

// The verified inflated bytes d_raw[head, n_raw) of a text stream call (kmm_map_bgzf, kmm_map_gzip): on LAST_CHUNK a last line
// without its newline gets one (last_byte = d_raw[n_raw - 1]), then the records are mapped; *used: where the last complete one ends.
static int map_text_inflated(kmm_index_t *ix, const StreamCall &c, uint8_t *d_raw, int64_t head, int64_t &n_raw, size_t cap,
                             uint8_t last_byte, int64_t *used)
{
    if (c.last_chunk && n_raw > head && last_byte != 10) { // a last line without its newline gets one (as the file readers do)
        if (cap < (size_t)n_raw + 1)
            return fail(KMM_ERR_INTERNAL, "%s: no room for the final newline", c.who);
        HIPCHK(hipMemsetAsync(d_raw + n_raw, 10, 1, ix->stream));
        ++n_raw;
    }
    int64_t recs = 0;
    *used = 0;
    ix->rk_snap.valid = false; // (what keep_carry may put back is this call's, never an earlier one's)
    // ("record_sam_mates", DESIGN 4.28: the stream's last call says so — a mate 1 that still waits then has no mate)
    const int last = c.last_chunk && c.fmt == KMM_FORMAT_SAM && sam_raw_mates_on(ix) ? KMM_FORMAT_LAST_CHUNK : 0;
    if (n_raw > head || last)
        KMMCHK(kmm_map_records(ix, d_raw + head, n_raw - head, c.fmt | last, c.k, c.max_freq, c.also_revcomp, c.lut, used, &recs));
    *used += head;
    if (c.n_records)
        *c.n_records = recs;
    return KMM_OK;
}

// What bgzf_inflate returns: the verified inflated bytes d_raw[head, n_raw) (the carry in front) in the buffer pair `cur`;
// d_raw stays NULL when there is no member and no carry to finish (the call is over).
struct BgzfCall {
    BgzfStaged st;
    int cur = 0;
    uint8_t *d_raw = nullptr;
    int64_t head = 0, n_raw = 0;
    int64_t tail_stop = -1; // >= 0: "bgzf_tail_stop" cut the last member there (bgzf_rank_share)
    uint8_t last_byte = 10; // d_raw[n_raw - 1] on LAST_CHUNK
    uint32_t n_members = 0;
    bool from_pre = false;
    std::chrono::steady_clock::time_point t_0;
    double ms_stage = 0, ms_scan = 0, ms_inflate = 0;
};

// kmm_map_bgzf and kmm_map_bam up to their verified inflated bytes: the chunk is staged and its member chain walked (or both were
// done under the call before), the members are inflated behind the carried bytes and their CRC32s checked by kernels on the
// handle's stream, and the chunk announced behind this one is staged meanwhile.  narrow (kmm_map_bgzf: a rank's share of a
// file) may set b.head and b.n_raw while the kernels run.
static int bgzf_inflate(kmm_index_t *ix, StreamCall &c, const uint8_t *comp, int64_t n_comp, BgzfCall &b,
                        int (*narrow)(kmm_index_t *, const StreamCall &, BgzfCall &))
{
    const char *who = c.who;
    if (c.new_stream)
        ix->bgzf_carry_len = 0;
    const auto t_0 = b.t_0 = std::chrono::steady_clock::now();
    // The compressed bytes go through a RING of page-locked memory (8 slots of 16 MiB; from a file mapping — pageable memory —
    // the runtime's own staging is slow, and a page-locked buffer the size of the window costs ~50 ms per GB to make, more
    // than the whole call): the packing threads copy 1 MiB pieces into the slots, a slot leaves for HBM as soon as it is full
    // and is refilled when its copy has landed.  The member chain is read from the caller's bytes BEHIND the threads — what
    // they have copied is mapped into the process, so the walk (two cache lines per member) pays no page fault — and at the
    // same time: the calling thread has nothing else to do while the threads copy.
    const int cur = b.cur = ix->bgzf_cur;
    ix->bgzf_cur ^= 1;
    if (!ix->bgzf_done[cur])
        HIPCHK(hipEventCreateWithFlags(ix->bgzf_done[cur].put(), hipEventDisableTiming));
    const int64_t carry = ix->bgzf_carry_len;
    // 3.5 GiB per call; what a prestaged chain leaves for a carry ("debug_bgzf_call_cap_kb": a small file reaches the cap)
    const unsigned long long CALL_CAP = ix->dbg_bgzf_call_cap_kb > 0 ? (unsigned long long)ix->dbg_bgzf_call_cap_kb << 10 : 7ull << 29,
                             PRE_CARRY = ix->dbg_bgzf_call_cap_kb > 0 ? CALL_CAP / 4 : 256ull << 20;
    BgzfStaged &st = b.st;
    if (ix->bgzf_pre_valid && ix->bgzf_pre_from == comp && ix->bgzf_pre_n == n_comp && ix->bgzf_pre_buf == cur &&
        (unsigned long long)carry <= PRE_CARRY) {
        st = std::move(ix->bgzf_pre); // staged and walked while the chunk before this one was being inflated
        st.ms_scan_inside = 0;
        b.from_pre = true;
    }
    ix->bgzf_pre_valid = false;
    if (!b.from_pre) {
        if (ix->bgzf_used[cur])
            HIPCHK(hipStreamWaitEvent(ix->copy_stream, ix->bgzf_done[cur], 0)); // the kernels that last read these buffers are done
        KMMCHK(ensure(ix->bgzf_comp[cur], (size_t)n_comp + 64));
        KMMCHK(bgzf_stage_and_scan(ix, comp, 0, n_comp, (uint8_t *)ix->bgzf_comp[cur].p, CALL_CAP - (unsigned long long)carry, st));
    }
    uint8_t *d_comp = (uint8_t *)ix->bgzf_comp[cur].p;
    const bool staged = st.staged;
    if (st.hit_cap)
        c.last_chunk = false; // (the call stops at its own size limit: the caller continues with the same flags)
    const double ms_stage = b.ms_stage = ms_since(t_0) - st.ms_scan_inside;
    const uint64_t p = st.p;
    if (st.chain_err) {
        (void)hipStreamSynchronize(ix->copy_stream); // (the page-locked ring is free again)
        if (st.chain_err == 1)
            return fail(KMM_ERR_MALFORMED, "%s: no BGZF member at compressed byte %llu of the chunk (a gzip file that bgzip did "
                        "not write has no member sizes in its headers: inflate it on the host)", who, (unsigned long long)p);
        return fail(KMM_ERR_MALFORMED, "%s: member at compressed byte %llu claims %u inflated bytes for %u compressed ones",
                    who, (unsigned long long)p, st.bad_isize, st.bad_ms);
    }
    std::vector<unsigned long long> &m_off = st.m_off, &o_off = st.o_rel;
    for (unsigned long long &o : o_off) // (the inflated bytes carried over from the call before lie in front)
        o += (unsigned long long)carry;
    const uint32_t n_members = b.n_members = (uint32_t)(m_off.size() - 1);
    const int64_t n_used = (int64_t)p, n_total = (int64_t)o_off.back();
    if (c.consumed_comp)
        *c.consumed_comp = n_used;
    if (c.last_chunk && n_used != n_comp) {
        (void)hipStreamSynchronize(ix->copy_stream);
        return fail(KMM_ERR_MALFORMED, "%s: the file ends inside a BGZF member (%lld bytes behind the last whole member)", who,
                    (long long)(n_comp - n_used));
    }
    if (n_members == 0 && !(c.last_chunk && carry > 0)) {
        HIPCHK(hipStreamSynchronize(ix->copy_stream)); // (the page-locked buffer is free again)
        return KMM_OK;
    }
    b.ms_scan = ms_since(t_0) - ms_stage;
    KMMCHK(ensure(ix->bgzf_raw[cur], (size_t)n_total + 4096));
    KMMCHK(ensure(ix->bgzf_meta[cur], (size_t)(n_members + 1) * 16 + 64));
    KMMCHK(ensure(ix->bgzf_err, 64));
    KMMCHK(ensure_crc_tables(ix));
    const uint32_t grid_threads = ((n_members < 65536u ? n_members : 65536u) + 63u) / 64u * 64u;
    if (n_members) {
        KMMCHK(ensure(ix->bgzf_tabs, (size_t)grid_threads * kmm_gz::SCRATCH_BYTES));
        KMMCHK(ensure(ix->bgzf_status, (size_t)n_members + 64));
    }
    uint8_t *d_raw = b.d_raw = (uint8_t *)ix->bgzf_raw[cur].p;
    unsigned long long *d_moff = (unsigned long long *)ix->bgzf_meta[cur].p, *d_ooff = d_moff + (n_members + 1);
    if (n_members) {
        if (!staged)
            HIPCHK(hipMemcpyAsync(d_comp, comp, (size_t)n_used, hipMemcpyHostToDevice, ix->copy_stream));
        HIPCHK(hipMemcpyAsync(d_moff, m_off.data(), (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, ix->copy_stream));
        HIPCHK(hipMemcpyAsync(d_ooff, o_off.data(), (size_t)(n_members + 1) * 8, hipMemcpyHostToDevice, ix->copy_stream));
    }
    const unsigned int err0[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
    HIPCHK(hipMemcpyAsync(ix->bgzf_err.p, err0, sizeof err0, hipMemcpyHostToDevice, ix->copy_stream));
    KMMCHK(stage_copies_done(ix)); // (the handle's stream waits for the copies; the page-locked buffer is free after the sync below)
    if (carry > 0)
        HIPCHK(hipMemcpyAsync(d_raw, ix->bgzf_carry.p, (size_t)carry, hipMemcpyDeviceToDevice, ix->stream));
    if (n_members) {
        // members refused by the inflater are marked; the CRC32s are checked by a kernel of its own behind it (there nothing holds
        // the occupancy down: 2-3 ms of the inflater's 24 per wavefront become a fraction of a millisecond)
        HIPCHK(hipMemsetAsync(ix->bgzf_status.p, 0, n_members, ix->stream));
        hipLaunchKernelGGL(kmm_gz::k_inflate_bgzf, dim3(grid_threads / 64u), dim3(64), 0, ix->stream, d_comp, d_moff, d_ooff, d_raw, n_members,
                           (uint8_t *)ix->bgzf_tabs.p, (const uint32_t *)nullptr, (unsigned int *)ix->bgzf_err.p,
                           (unsigned long long *)nullptr, (uint8_t *)ix->bgzf_status.p);
        hipLaunchKernelGGL(kmm_gz::k_crc_bgzf, dim3((n_members + 63u) / 64u), dim3(256), 0, ix->stream, d_comp, d_moff, d_ooff,
                           (const uint8_t *)d_raw, n_members, (const uint32_t *)ix->bgzf_crc.p, (unsigned int *)ix->bgzf_err.p,
                           (const uint8_t *)ix->bgzf_status.p);
        HIPCHK(hipGetLastError());
    }
    // The chunk BEHIND this one (kmm_map_bgzf_hint_next: the caller's bytes go on where this chunk ends) is staged and walked NOW,
    // under this chunk's inflate kernel: its 20 ms over PCIe would otherwise stand in front of its own 46 ms of kernel.  The next
    // call starts where this call's whole members end — the head of a member that this chunk cut off is copied in front.
    if (ix->bgzf_hint_ptr && ix->bgzf_hint_ptr == comp + n_comp && ix->bgzf_hint_n > 0 && n_members > 0 && n_used <= n_comp) {
        const int nxt = cur ^ 1;
        const int64_t head_len = n_comp - n_used, total = head_len + ix->bgzf_hint_n;
        bool ok = hipStreamSynchronize(ix->copy_stream) == hipSuccess; // (this chunk's copies have landed: the ring is free)
        if (ok && ix->bgzf_used[nxt])
            ok = hipStreamWaitEvent(ix->copy_stream, ix->bgzf_done[nxt], 0) == hipSuccess;
        if (ok && ix->bgzf_comp[nxt].cap < (size_t)total + 64) // (growing it frees it first: a device-wide wait, once)
            ok = ensure(ix->bgzf_comp[nxt], (size_t)total + 64) == KMM_OK;
        if (ok && head_len > 0)
            ok = hipMemcpyAsync(ix->bgzf_comp[nxt].p, d_comp + n_used, (size_t)head_len, hipMemcpyDeviceToDevice, ix->copy_stream) == hipSuccess;
        if (ok && bgzf_stage_and_scan(ix, comp + n_used, head_len, total, (uint8_t *)ix->bgzf_comp[nxt].p, CALL_CAP - PRE_CARRY, ix->bgzf_pre) == KMM_OK &&
            ix->bgzf_pre.staged && !ix->bgzf_pre.chain_err) {
            ix->bgzf_pre_valid = true;
            ix->bgzf_pre_from = comp + n_used;
            ix->bgzf_pre_n = total;
            ix->bgzf_pre_buf = nxt;
            ix->bgzf_prestaged_calls++;
        } else {
            (void)hipGetLastError();
        }
        (void)hipStreamSynchronize(ix->copy_stream); // (between calls the ring is free: its last slots have landed, ~2 ms)
    }
    ix->bgzf_hint_ptr = nullptr;
    ix->bgzf_hint_n = 0;
    b.n_raw = n_total;
    if (narrow)
        KMMCHK(narrow(ix, c, b));
    unsigned int err[4] = {0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(err, ix->bgzf_err.p, sizeof err, hipMemcpyDeviceToHost, ix->stream));
    if (c.last_chunk && b.n_raw > b.head)
        HIPCHK(hipMemcpyAsync(&b.last_byte, d_raw + b.n_raw - 1, 1, hipMemcpyDeviceToHost, ix->stream));
    HIPCHK(hipStreamSynchronize(ix->stream)); // (CRC32 / ISIZE of every member are checked before a byte is mapped)
    b.ms_inflate = ms_since(t_0) - b.ms_scan - ms_stage;
    ix->bgzf_calls++;
    ix->bgzf_members += n_members;
    if (err[0]) {
        static const char *why[] = {"", "header", "reserved block type", "stored block", "code lengths", "Huffman code", "invalid symbol",
                                    "distance too far back", "more data than ISIZE", "compressed data ended early", "less data than ISIZE",
                                    "CRC32 mismatch"};
        ix->bgzf_carry_len = 0;
        return fail(KMM_ERR_MALFORMED, "%s: %u corrupt BGZF member(s); the first starts at compressed byte %llu of the chunk: %s",
                    who, err[0], err[1] < n_members ? m_off[err[1]] : 0ull, err[2] < 12 ? why[err[2]] : "?");
    }
    return KMM_OK;
}

// The end of a kmm_map_bgzf / kmm_map_bam call whose records are mapped up to d_raw[used]: the rest is carried, and the buffers
// `cur` are free again once the handle's stream has passed what the call queued.
static int bgzf_finish(kmm_index_t *ix, const StreamCall &c, const BgzfCall &b, int64_t used)
{
    static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
    if (verbose)
        fprintf(stderr, "libkmm: %s: %u members, %lld -> %lld bytes: member scan %.2f ms, buffers + staging + copy %.2f ms%s, "
                "copy tail + inflate kernel%s %.2f ms, records %.2f ms\n", c.who, b.n_members, (long long)b.st.p, (long long)b.st.o_rel.back(),
                b.ms_scan, b.ms_stage, b.from_pre ? " (staged and walked under the call before)" : "",
                ix->bgzf_pre_valid ? " + the next chunk's staging" : "", b.ms_inflate, ms_since(b.t_0) - b.ms_scan - b.ms_stage - b.ms_inflate);
    KMMCHK(keep_carry(ix, c, b.d_raw, used, b.n_raw, ix->bgzf_carry, ix->bgzf_carry_len));
    HIPCHK(hipEventRecord(ix->bgzf_done[b.cur], ix->stream));
    ix->bgzf_used[b.cur] = true;
    return KMM_OK;
}

// A RANK'S SHARE of a file (kmer_mapper map with several ranks, bgzf_ranges.py; kmm_map_bgzf and kmm_map_bam): its first member starts inside a record
// that belongs to the rank before it — "bgzf_head_skip" bytes of the stream's first member are passed over — and its last
// member holds the start of the next rank's first record — only "bgzf_tail_stop" bytes of the last member are taken.
static int bgzf_rank_share(kmm_index_t *ix, const StreamCall &c, BgzfCall &b)
{
    const uint32_t n_members = b.n_members;
    const std::vector<unsigned long long> &o_off = b.st.o_rel;
    if (c.new_stream) {
        b.head = ix->bgzf_head_skip;
        ix->bgzf_head_skip = 0;
    }
    if (c.last_chunk && ix->bgzf_tail_stop >= 0) {
        if (n_members == 0 || (unsigned long long)ix->bgzf_tail_stop > o_off[n_members] - o_off[n_members - 1]) {
            (void)hipStreamSynchronize(ix->stream);
            return fail(KMM_ERR_INVALID_ARG, "%s: bgzf_tail_stop %lld lies beyond the last member's %llu bytes", c.who,
                        (long long)ix->bgzf_tail_stop, n_members ? o_off[n_members] - o_off[n_members - 1] : 0ull);
        }
        b.n_raw = (int64_t)o_off[n_members - 1] + ix->bgzf_tail_stop;
        b.tail_stop = ix->bgzf_tail_stop;
        ix->bgzf_tail_stop = -1;
    }
    if (b.head > b.n_raw) {
        (void)hipStreamSynchronize(ix->stream);
        return fail(KMM_ERR_INVALID_ARG, "%s: bgzf_head_skip %lld lies beyond the %lld bytes of the call", c.who, (long long)b.head,
                    (long long)b.n_raw);
    }
    return KMM_OK;
}

int kmm_map_bgzf(kmm_index_t *ix, const uint8_t *comp, int64_t n_comp, int format, int k, int max_freq, int also_revcomp,
                 const uint8_t *lut, int64_t *consumed_comp, int64_t *n_records)
{
    StreamCall c{"kmm_map_bgzf", k, max_freq, also_revcomp, lut, consumed_comp, n_records};
    return guarded(c.who, [&] {
        KMMCHK(stream_call_start(ix, c, comp, n_comp, format, true, true));
        BgzfCall b;
        KMMCHK(bgzf_inflate(ix, c, comp, n_comp, b, bgzf_rank_share));
        if (!b.d_raw)
            return sam_mates_empty_end(ix, c);
        int64_t used = 0;
        KMMCHK(map_text_inflated(ix, c, b.d_raw, b.head, b.n_raw, ix->bgzf_raw[b.cur].cap, b.last_byte, &used));
        return bgzf_finish(ix, c, b, used);
    });
}

namespace {
#include "kmm_bam_host.hpp" // bam_map_inflated and what it runs, rs_*: behind StreamCall and bgzf_inflate, in front of kmm_map_bam
} // namespace

int kmm_map_bam(kmm_index_t *ix, const uint8_t *comp, int64_t n_comp, int flags, int k, int max_freq, int also_revcomp,
                const uint8_t *lut, int64_t *consumed_comp, int64_t *n_records)
{
    StreamCall c{"kmm_map_bam", k, max_freq, also_revcomp, lut, consumed_comp, n_records};
    return guarded(c.who, [&] {
        KMMCHK(stream_call_start(ix, c, comp, n_comp, flags, false, true));
        // ("record_names_pairs", DESIGN 4.23: read here alone)
        if (ix->record_names_pairs && (!ix->record_names || !ix->record_keep))
            return fail(KMM_ERR_INVALID_ARG, "kmm_map_bam: \"record_names_pairs\" is 1 and \"%s\" is 0: mates are kept together in the "
                        "named FASTQ form of the decode under the keep rule, set \"record_names\" and \"record_keep\" to 1, or "
                        "\"record_names_pairs\" to 0 (nothing is mapped)", ix->record_names ? "record_keep" : "record_names");
        if (ix->record_names_pairs && ix->record_pairs)
            return fail(KMM_ERR_INVALID_ARG, "kmm_map_bam: \"record_names_pairs\" and \"record_pairs\" are 1: the first pairs the records "
                        "of a BAM stream, the second those of FASTQ and two-line FASTA text; set one of them to 0 (nothing is mapped)");
        if (c.new_stream)
            ix->bam_mate_len = ix->bam_pairs_done = ix->bam_raw_mate_len = 0; // (a mate 1 left over belongs to the stream before)
        BgzfCall b;
        KMMCHK(bgzf_inflate(ix, c, comp, n_comp, b, bgzf_rank_share));
        if (!b.d_raw) { // (no member and no carried byte: a last call that brings nothing can still leave a mate 1 alone)
            if (c.last_chunk && ix->bam_mate_len > 0 && (bam_mates_on(ix) || bam_raw_mates_on(ix)))
                return bam_unpaired_end(bam_mates_on(ix) ? "record_names_pairs" : "record_bam_mates", 2 * ix->bam_pairs_done + 1);
            return KMM_OK;
        }
        int64_t used = 0;
        bool short_header = false;
        const int rc = bam_map_inflated(ix, c, b.d_raw, b.head, b.tail_stop, b.n_raw, &used, &short_header);
        if (rc != KMM_OK || short_header) { // (an error, or a first window that ends inside the header: nothing used, nothing kept)
            ix->bgzf_carry_len = 0;
            ix->bgzf_pre_valid = false;
            if (c.consumed_comp)
                *c.consumed_comp = 0;
            HIPCHK(hipEventRecord(ix->bgzf_done[b.cur], ix->stream));
            ix->bgzf_used[b.cur] = true;
            return rc;
        }
        return bgzf_finish(ix, c, b, used);
    });
}

int kmm_bam_stream_header(kmm_index_t *ix, uint8_t *out, int64_t capacity, int64_t *n_bytes)
{
    return guarded("kmm_bam_stream_header", [&] {
        if (!ix)
            return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
        if (n_bytes)
            *n_bytes = 0;
        if (!ix->bam_hdr_valid)
            return fail(KMM_ERR_INVALID_ARG, "kmm_bam_stream_header: no BAM stream with a header was started on this handle (kmm_map_bam with "
                        "KMM_FORMAT_NEW_STREAM; a KMM_FORMAT_MID_STREAM share has none)");
        const int64_t n = (int64_t)ix->bam_hdr.size();
        if (n_bytes)
            *n_bytes = n;
        if (capacity < n || !out)
            return fail(KMM_ERR_INVALID_ARG, "kmm_bam_stream_header: the header has %lld bytes, capacity is %lld", (long long)n,
                        (long long)(out ? capacity : 0));
        memcpy(out, ix->bam_hdr.data(), (size_t)n);
        return KMM_OK;
    });
}


int kmm_bam_header(kmm_index_t *ix, const uint8_t *comp, int64_t n_comp, int32_t *n_ref, int64_t *hdr_member, int64_t *hdr_skip)
{
    const char *who = "kmm_bam_header";
    return guarded(who, [&] {
        KMMCHK(rs_args(ix, who, comp, n_comp));
        if (!n_ref || !hdr_member || !hdr_skip)
            return fail(KMM_ERR_INVALID_ARG, "%s: n_ref, hdr_member or hdr_skip is NULL", who);
        *n_ref = -1;
        *hdr_member = *hdr_skip = 0;
        // growing prefixes of the window's members are inflated and read back: the header's length is only known by walking it
        RsChain c;
        std::vector<uint8_t> h;
        uint64_t hdr_end = 0;
        for (unsigned long long want = 1ull << 16;; want *= 4) {
            const uint64_t p_before = c.p;
            KMMCHK(rs_scan(who, comp, n_comp, want, c));
            if (c.p != p_before)
                KMMCHK(rs_inflate(ix, who, comp, c));
            h.resize((size_t)c.o_off.back());
            if (!h.empty()) {
                HIPCHK(hipMemcpyAsync(h.data(), ix->rs_raw.p, h.size(), hipMemcpyDeviceToHost, ix->stream));
                HIPCHK(hipStreamSynchronize(ix->stream));
            }
            int32_t nr = 0;
            const int r = h.empty() ? 1 : kmm_bam::parse_header(h.data(), h.size(), &hdr_end, &nr);
            if (r < 0)
                return fail(KMM_ERR_MALFORMED, "%s: the file does not start with a BAM header (magic \"BAM\\1\", lengths)", who);
            if (r == 0) {
                *n_ref = nr;
                break;
            }
            if (c.o_off.back() < want) // (the window's whole members are all in: it ends inside the header)
                return KMM_OK;
        }
        // the first byte behind the header: in the member that holds it — behind the inflated prefix, the next member that
        // holds a byte at all (the chain goes on over empty members; at the window's end: there, skip 0)
        while (hdr_end >= c.o_off.back()) {
            const uint64_t p_before = c.p;
            KMMCHK(rs_scan(who, comp, n_comp, c.o_off.back() + 1, c));
            if (c.p == p_before)
                break;
        }
        kmm_bam::locate(c.m_off.data(), c.o_off.data(), c.n_members(), hdr_end, hdr_member, hdr_skip);
        return KMM_OK;
    });
}

int kmm_bam_find_record_start(kmm_index_t *ix, const uint8_t *comp, int64_t n_comp, int32_t n_ref, int64_t *member, int64_t *skip)
{
    const char *who = "kmm_bam_find_record_start";
    return guarded(who, [&] {
        KMMCHK(rs_args(ix, who, comp, n_comp));
        if (!member || !skip)
            return fail(KMM_ERR_INVALID_ARG, "%s: member or skip is NULL", who);
        if (n_ref < 0)
            return fail(KMM_ERR_INVALID_ARG, "%s: n_ref negative (kmm_bam_header returns it)", who);
        *member = -1;
        *skip = 0;
        const auto t_0 = std::chrono::steady_clock::now();
        // ("debug_bam_resync_kb": the examined bytes end at the cap, as if the window did)
        const unsigned long long cap = ix->dbg_bam_resync_kb > 0 ? (unsigned long long)ix->dbg_bam_resync_kb << 10 : ~0ull;
        RsChain c;
        KMMCHK(rs_scan(who, comp, n_comp, cap, c));
        bool at_eof = false;
        const uint64_t n = kmm_bam::resync_extent(c.o_off.back(), ix->dbg_bam_resync_kb > 0 ? cap : 0, c.p == (uint64_t)n_comp, &at_eof);
        if (n == 0) { // (no whole member, or only empty ones)
            kmm_bam::resync_answer(c.m_off.data(), c.o_off.data(), c.n_members(), kmm_bam::NONE, at_eof, member, skip);
            return KMM_OK;
        }
        KMMCHK(rs_inflate(ix, who, comp, c));
        const double ms_inflate = ms_since(t_0);
        unsigned long long *d_best = (unsigned long long *)((uint8_t *)ix->rs_err.p + 32), best = kmm_bam::NONE;
        const uint64_t n_tiles = (n + kmm_bam::TILE - 1) / kmm_bam::TILE;
        HIPCHK(hipMemsetAsync(d_best, 0xFF, 8, ix->stream));
        hipLaunchKernelGGL(kmm_bam::k_bam_resync, dim3((unsigned)grid_for(ix, (int64_t)((n_tiles + 3) / 4), 16)), dim3(256), 0, ix->stream,
                           (const uint8_t *)ix->rs_raw.p, n, n_tiles, n_ref, at_eof ? 1u : 0u, d_best);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&best, d_best, 8, hipMemcpyDeviceToHost, ix->stream));
        HIPCHK(hipStreamSynchronize(ix->stream));
        static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
        if (verbose)
            fprintf(stderr, "libkmm: %s: %u members, %lld -> %llu bytes examined%s: copy + inflate + CRC %.2f ms, resync kernel %.2f ms\n", who,
                    c.n_members(), (long long)c.p, (unsigned long long)n, at_eof ? " (to the end of the file)" : "", ms_inflate,
                    ms_since(t_0) - ms_inflate);
        kmm_bam::resync_answer(c.m_off.data(), c.o_off.data(), c.n_members(), best, at_eof, member, skip);
        return KMM_OK;
    });
}

// ---- kmm_map_gzip: a plain gzip stream inflated on the GPU (kmm_gpu_gunzip.hpp; the orchestration there, run_call, is shared
// with the CPU tests).  The backend: buffers of the handle, kernels on its stream, a bump allocator over gz_arena for the slots.
struct GzGpuBackend {
    kmm_index_t *ix;
    double ratio = 4.0;
    const uint8_t *d_in = nullptr;
    uint32_t n_pad = 0;
    uint64_t n = 0;
    int64_t carry = 0;        // inflated bytes carried over from the call before: they lie in front in gz_raw
    uint8_t *d_out = nullptr; // where the call's inflated bytes go: gz_raw behind the carried bytes
    size_t blk = 0, used = 0; // arena block in use, bytes used in it
    int rc = KMM_OK;
    uint32_t n_chunks = 0;
    double ms_find = 0, ms_decode = 0, ms_windows = 0, ms_resolve = 0, ms_crc = 0;
    int launches = 0;

    bool hip(hipError_t e, const char *what)
    {
        if (e == hipSuccess)
            return true;
        rc = fail(KMM_ERR_HIP, "kmm_map_gzip: %s: %s", what, hipGetErrorString(e));
        return false;
    }
    bool sync() { return hip(hipStreamSynchronize(ix->stream), "hipStreamSynchronize"); }
    bool upload(DevBuf &b, const void *p, size_t bytes)
    {
        if ((rc = ensure(b, bytes + 64)) != KMM_OK)
            return false;
        return hip(hipMemcpyAsync(b.p, p, bytes, hipMemcpyHostToDevice, ix->stream), "upload");
    }
    uint16_t *alloc_syms(size_t k)
    {
        const size_t bytes = (k * 2 + 255) & ~(size_t)255, BLOCK = (size_t)1 << 30;
        while (blk < ix->gz_arena.size() && used + bytes > ix->gz_arena[blk].cap) {
            ++blk;
            used = 0;
        }
        if (blk == ix->gz_arena.size()) {
            ix->gz_arena.emplace_back();
            if ((rc = ensure(ix->gz_arena.back(), bytes > BLOCK ? bytes : BLOCK)) != KMM_OK) {
                ix->gz_arena.pop_back();
                return nullptr;
            }
            used = 0;
        }
        uint16_t *p = (uint16_t *)((uint8_t *)ix->gz_arena[blk].p + used);
        used += bytes;
        return p;
    }
    bool tabs(uint32_t threads)
    {
        return (rc = ensure(ix->gz_tabs, (size_t)threads * kmm_gz::SEC_WORDS * 2)) == KMM_OK;
    }
    bool find(const uint8_t *, uint64_t, uint64_t S8, uint32_t c0, uint32_t n_cand, uint64_t *starts)
    {
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t grid = n_cand < 1024u ? n_cand : 1024u;
        if (!tabs(grid * 64u) || (rc = ensure(ix->gz_res, (size_t)n_cand * 8 + 64)) != KMM_OK)
            return false;
        hipLaunchKernelGGL(kmm_gunzip::k_gz_find, dim3(grid), dim3(64), 0, ix->stream, d_in, n_pad, n, S8, c0, n_cand, (uint16_t *)ix->gz_tabs.p,
                           (unsigned long long *)ix->gz_res.p);
        ++launches;
        if (!hip(hipGetLastError(), "k_gz_find") ||
            !hip(hipMemcpyAsync(starts, ix->gz_res.p, (size_t)n_cand * 8, hipMemcpyDeviceToHost, ix->stream), "starts") || !sync())
            return false;
        ms_find += ms_since(t0);
        return true;
    }
    bool decode(const kmm_gunzip::Work *w, kmm_gunzip::Result *r, size_t k)
    {
        const auto t0 = std::chrono::steady_clock::now();
        const uint32_t threads = (uint32_t)((k < 65536 ? k : 65536) + 63) / 64u * 64u;
        if (!tabs(threads) || !upload(ix->gz_meta, w, k * sizeof *w) || (rc = ensure(ix->gz_res, k * sizeof(kmm_gunzip::Result) + 64)) != KMM_OK)
            return false;
        hipLaunchKernelGGL(kmm_gunzip::k_gz_decode, dim3(threads / 64u), dim3(64), 0, ix->stream, d_in, n_pad, n,
                           (const kmm_gunzip::Work *)ix->gz_meta.p, (kmm_gunzip::Result *)ix->gz_res.p, (uint32_t)k, (uint16_t *)ix->gz_tabs.p);
        ++launches;
        if (!hip(hipGetLastError(), "k_gz_decode") ||
            !hip(hipMemcpyAsync(r, ix->gz_res.p, k * sizeof(kmm_gunzip::Result), hipMemcpyDeviceToHost, ix->stream), "results") || !sync())
            return false;
        ms_decode += ms_since(t0);
        return true;
    }
    bool windows(const kmm_gunzip::MapRef *maps, uint32_t nc, uint32_t G)
    {
        const auto t0 = std::chrono::steady_clock::now();
        using kmm_gunzip::WIN;
        const uint32_t n_groups = (nc + G - 1) / G;
        n_chunks = nc;
        if (!upload(ix->gz_meta, maps, nc * sizeof *maps) || (rc = ensure(ix->gz_gmaps, (size_t)n_groups * WIN * 2)) != KMM_OK ||
            (rc = ensure(ix->gz_gwin, (size_t)n_groups * WIN)) != KMM_OK || (rc = ensure(ix->gz_win, (size_t)nc * WIN)) != KMM_OK)
            return false;
        const kmm_gunzip::MapRef *d_maps = (const kmm_gunzip::MapRef *)ix->gz_meta.p;
        hipLaunchKernelGGL(kmm_gunzip::k_gz_compose, dim3(n_groups), dim3(kmm_gunzip::WT), 0, ix->stream, d_maps, nc, G, (uint16_t *)ix->gz_gmaps.p);
        hipLaunchKernelGGL(kmm_gunzip::k_gz_chain, dim3(1), dim3(kmm_gunzip::WT), 0, ix->stream, (const uint16_t *)ix->gz_gmaps.p, n_groups,
                           (const uint8_t *)ix->gz_window.p, (uint8_t *)ix->gz_gwin.p);
        hipLaunchKernelGGL(kmm_gunzip::k_gz_fix, dim3(n_groups), dim3(kmm_gunzip::WT), 0, ix->stream, d_maps, nc, G, (const uint8_t *)ix->gz_gwin.p,
                           (uint8_t *)ix->gz_win.p, (uint8_t *)ix->gz_window.p);
        launches += 3;
        if (!hip(hipGetLastError(), "window kernels") || !sync())
            return false;
        ms_windows += ms_since(t0);
        return true;
    }
    bool resolve(const kmm_gunzip::PieceRef *p, size_t k, uint64_t *bad)
    {
        uint64_t need = 0;
        for (size_t i = 0; i < k; ++i)
            need = p[i].off + p[i].n > need ? p[i].off + p[i].n : need;
        DevBuf &raw = ix->gz_raw;
        if (raw.cap < (size_t)carry + need + 4096) { // (the carried bytes move along)
            DevBuf nb;
            if ((rc = ensure(nb, (size_t)carry + need + need / 8 + 4096)) != KMM_OK)
                return false;
            if (carry > 0 && !hip(hipMemcpyAsync(nb.p, ix->gz_carry.p, (size_t)carry, hipMemcpyDeviceToDevice, ix->stream), "carry"))
                return false;
            if (!sync())
                return false;
            (void)raw.reset();
            raw = std::move(nb);
        } else if (carry > 0 && !hip(hipMemcpyAsync(raw.p, ix->gz_carry.p, (size_t)carry, hipMemcpyDeviceToDevice, ix->stream), "carry")) {
            return false;
        }
        d_out = (uint8_t *)raw.p + carry;
        const auto t0 = std::chrono::steady_clock::now();
        *bad = 0;
        if (!k)
            return true;
        if (!upload(ix->gz_meta, p, k * sizeof *p) || (rc = ensure(ix->gz_err, 64)) != KMM_OK ||
            !hip(hipMemsetAsync(ix->gz_err.p, 0, 4, ix->stream), "memset"))
            return false;
        const uint32_t grid = k < 65535 ? (uint32_t)k : 65535u;
        hipLaunchKernelGGL(kmm_gunzip::k_gz_resolve, dim3(grid), dim3(256), 0, ix->stream, (const kmm_gunzip::PieceRef *)ix->gz_meta.p, (uint32_t)k,
                           (const uint8_t *)ix->gz_win.p, d_out, (unsigned int *)ix->gz_err.p);
        ++launches;
        unsigned int e = 0;
        if (!hip(hipGetLastError(), "k_gz_resolve") || !hip(hipMemcpyAsync(&e, ix->gz_err.p, 4, hipMemcpyDeviceToHost, ix->stream), "err") ||
            !sync())
            return false;
        *bad = e;
        ms_resolve += ms_since(t0);
        return true;
    }
    bool crc(const kmm_gunzip::Part *p, size_t k, uint32_t *regs)
    {
        const auto t0 = std::chrono::steady_clock::now();
        if (!upload(ix->gz_meta, p, k * sizeof *p) || (rc = ensure(ix->gz_res, k * 4 + 64)) != KMM_OK)
            return false;
        hipLaunchKernelGGL(kmm_gunzip::k_gz_crc, dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, ix->stream, (const uint8_t *)d_out,
                           (const kmm_gunzip::Part *)ix->gz_meta.p, (uint32_t)k, (const uint32_t *)ix->bgzf_crc.p, (uint32_t *)ix->gz_res.p);
        ++launches;
        if (!hip(hipGetLastError(), "k_gz_crc") || !hip(hipMemcpyAsync(regs, ix->gz_res.p, k * 4, hipMemcpyDeviceToHost, ix->stream), "regs") ||
            !sync())
            return false;
        ms_crc += ms_since(t0);
        return true;
    }
};

int kmm_map_gzip(kmm_index_t *ix, const uint8_t *comp, int64_t n_comp, int format, int k, int max_freq, int also_revcomp,
                 const uint8_t *lut, int64_t *consumed_comp, int64_t *n_records)
{
    StreamCall c{"kmm_map_gzip", k, max_freq, also_revcomp, lut, consumed_comp, n_records};
    return guarded(c.who, [&] {
        KMMCHK(stream_call_start(ix, c, comp, n_comp, format, true, false));
        static const bool verbose = getenv("KMM_VERBOSE") != nullptr;
        const auto t_0 = std::chrono::steady_clock::now();
        constexpr int64_t MAX_WINDOW = (int64_t)1 << 31;   // compressed bytes one call looks at (the lanes' byte positions are 32-bit)
        constexpr unsigned long long CALL_CAP = 7ull << 29; // 3.5 GiB of inflated bytes per call, as kmm_map_bgzf
        bool window_cut = false;
        if (n_comp > MAX_WINDOW) {
            n_comp = MAX_WINDOW;
            window_cut = true;
        }
        if (c.new_stream) {
            ix->gz_carry_len = 0;
            ix->gz_state = kmm_gunzip::StreamState();
            ix->gz_ratio = 4.0;
        }
        KMMCHK(ensure(ix->gz_window, kmm_gunzip::WIN));
        if (c.new_stream)
            HIPCHK(hipMemsetAsync(ix->gz_window.p, 0, kmm_gunzip::WIN, ix->stream));
        KMMCHK(ensure_crc_tables(ix));
        // the compressed bytes reach HBM through the page-locked staging ring of kmm_map_bgzf (no member chain to walk)
        const uint32_t n_pad = (uint32_t)(n_comp < 16 ? 16 : n_comp) + 64u;
        KMMCHK(ensure(ix->gz_comp, n_pad));
        HIPCHK(hipStreamSynchronize(ix->stream)); // (the kernels of the call before have let go of gz_comp)
        uint8_t *d_comp = (uint8_t *)ix->gz_comp.p;
        HIPCHK(hipMemsetAsync(d_comp + n_comp, 0, n_pad - (uint32_t)n_comp, ix->copy_stream));
        if (n_comp > 0) {
            BgzfStaged st;
            KMMCHK(bgzf_stage_and_scan(ix, comp, 0, n_comp, d_comp, 0, st, false));
            if (!st.staged)
                HIPCHK(hipMemcpyAsync(d_comp, comp, (size_t)n_comp, hipMemcpyHostToDevice, ix->copy_stream));
        }
        KMMCHK(stage_copies_done(ix));
        HIPCHK(hipStreamSynchronize(ix->copy_stream));
        const double ms_stage = ms_since(t_0);
        // inflate
        const int64_t carry = ix->gz_carry_len;
        // the output: the call inflates into gz_raw behind the carried bytes; its size is known once the chunks stand, so the
        // buffer is made large enough for the window at the stream's ratio and grown (before any byte lands) if it must be
        const uint64_t S = ix->dbg_gzip_chunk_kb > 0 ? (uint64_t)ix->dbg_gzip_chunk_kb << 10 : (uint64_t)32 << 10;
        kmm_gunzip::StreamState state = ix->gz_state;
        kmm_gunzip::CallOut co;
        kmm_gunzip::CallStats cs;
        GzGpuBackend be{ix, ix->gz_ratio, d_comp, n_pad, (uint64_t)n_comp, carry};
        if (carry == 0 && ix->gz_raw.p == nullptr)
            KMMCHK(ensure(ix->gz_raw, 4096));
        const int rr = kmm_gunzip::run_call(be, comp, (uint64_t)n_comp, c.last_chunk && !window_cut, S, CALL_CAP - (unsigned long long)carry, state, co, cs);
        if (rr != 0)
            return be.rc != KMM_OK ? be.rc : fail(KMM_ERR_INTERNAL, "kmm_map_gzip: backend failure");
        ix->gzip_calls++;
        ix->gzip_chunks += (int64_t)cs.chunks;
        ix->gzip_false_starts += (int64_t)cs.false_starts;
        ix->gzip_continuations += (int64_t)cs.continuations;
        if (co.err) {
            static const char *why[] = {"", "header", "reserved block type", "stored block", "code lengths", "Huffman code", "invalid symbol",
                                        "distance too far back", "more data than a block can hold", "compressed data ended early",
                                        "ISIZE mismatch", "CRC32 mismatch"};
            ix->gz_carry_len = 0;
            ix->gz_arena.clear(); // the stream cannot go on: its symbol slots go back to the device
            return fail(KMM_ERR_MALFORMED, "kmm_map_gzip: corrupt gzip stream near compressed byte %llu of the chunk: %s",
                        (unsigned long long)co.err_at, co.err < 12 ? why[co.err] : "?");
        }
        if (co.hit_cap || window_cut)
            c.last_chunk = false; // (the call stops at its own size limit: the caller continues with the same flags)
        ix->gzip_members += (int64_t)cs.members;
        ix->gzip_inflated += (int64_t)co.n_out;
        ix->gz_state = state;
        if (co.consumed > 0 && co.n_out > 0) {
            const double r = (double)co.n_out / (double)co.consumed;
            ix->gz_ratio = r < 1.0 ? 1.0 : r > 1032.0 ? 1032.0 : r;
        }
        if (c.consumed_comp)
            *c.consumed_comp = (int64_t)co.consumed;
        const double ms_inflate = ms_since(t_0) - ms_stage;
        uint8_t *d_raw = (uint8_t *)ix->gz_raw.p;
        int64_t n_raw = carry + (int64_t)co.n_out;
        if (n_raw > 0) {
            uint8_t last_byte = 10;
            if (c.last_chunk) {
                HIPCHK(hipMemcpyAsync(&last_byte, d_raw + n_raw - 1, 1, hipMemcpyDeviceToHost, ix->stream));
                HIPCHK(hipStreamSynchronize(ix->stream));
            }
            int64_t used = 0;
            KMMCHK(map_text_inflated(ix, c, d_raw, 0, n_raw, ix->gz_raw.cap, last_byte, &used));
            if (verbose)
                fprintf(stderr, "libkmm: kmm_map_gzip: %lld -> %llu bytes, %llu chunks (%llu false starts, %llu continuations), %d launches: "
                        "staging %.2f ms, inflate %.2f ms (find %.2f, decode %.2f, windows %.2f, resolve %.2f, crc %.2f), records %.2f ms\n",
                        (long long)co.consumed, (unsigned long long)co.n_out, (unsigned long long)cs.chunks, (unsigned long long)cs.false_starts,
                        (unsigned long long)cs.continuations, be.launches, ms_stage, ms_inflate, be.ms_find, be.ms_decode, be.ms_windows,
                        be.ms_resolve, be.ms_crc, ms_since(t_0) - ms_stage - ms_inflate);
            KMMCHK(keep_carry(ix, c, d_raw, used, n_raw, ix->gz_carry, ix->gz_carry_len));
            HIPCHK(hipStreamSynchronize(ix->stream));
        } else
            KMMCHK(sam_mates_empty_end(ix, c));
        if (c.last_chunk)
            ix->gz_arena.clear(); // the stream has ended: its symbol slots go back to the device
        return KMM_OK;
    });
}

int kmm_in_index(kmm_index_t *ix, const uint64_t *kmers, int64_t n, uint8_t *out)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    if (n < 0 || (n > 0 && (!kmers || !out)))
        return fail(KMM_ERR_INVALID_ARG, "NULL argument or n negative");
    if (n == 0)
        return KMM_OK;
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(ensure_direct(ix));
    Stage &s = next_stage(ix);
    KMMCHK(stage_acquire(ix, s));
    bool staged = false;
    const uint64_t *d_kmers = nullptr;
    KMMCHK(stage_in<uint64_t>(ix, s.kmers, kmers, (size_t)n, &d_kmers, &staged));
    KMMCHK(stage_copies_done(ix));
    const bool out_dev = is_device_ptr(out);
    DevBuf tmp;
    uint8_t *d_out = out;
    if (!out_dev) {
        KMMCHK(ensure(tmp, (size_t)n));
        d_out = (uint8_t *)tmp.p;
    }
    hipLaunchKernelGGL(k_in_index, dim3(grid_for(ix, (n + 255) / 256, 32)), dim3(256), 0, ix->stream,
                       d_kmers, n, view_of(ix), d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && !out_dev)
        e = hipMemcpyAsync(out, d_out, (size_t)n, hipMemcpyDeviceToHost, ix->stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(ix->stream);
    if (e != hipSuccess)
        return fail(KMM_ERR_HIP, "kmm_in_index: %s", hipGetErrorString(e));
    return stage_release(ix, s, staged);
}

int kmm_read_hits(kmm_index_t *ix, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len, int k,
                  int max_freq, int also_revcomp, const uint8_t *lut, uint32_t *hits, uint32_t *windows)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(check_k(k));
    if (n_reads < 0 || (!read_offsets && read_len < 0))
        return fail(KMM_ERR_INVALID_ARG, "kmm_read_hits: n_reads / read_len negative");
    if (n_reads == 0)
        return KMM_OK;
    if (!hits)
        return fail(KMM_ERR_INVALID_ARG, "kmm_read_hits: hits is NULL");
    KMMCHK(check_k_lut(k, lut));
    return guarded("kmm_read_hits", [&] {
        return read_hits_impl(ix, bases, read_offsets, n_reads, read_len, k, max_freq, also_revcomp, lut, hits, windows);
    });
}

int kmm_read_nodes(kmm_index_t *ix, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len, int k,
                   int max_freq, int also_revcomp, const uint8_t *lut, int64_t table_bytes, int32_t *best_node, uint32_t *best_votes,
                   uint32_t *second_votes, uint32_t *total_votes, uint32_t *n_nodes, int64_t *n_rounds)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    KMMCHK(check_k(k));
    if (n_reads < 0 || (!read_offsets && read_len < 0))
        return fail(KMM_ERR_INVALID_ARG, "kmm_read_nodes: n_reads / read_len negative");
    if (table_bytes < 0)
        return fail(KMM_ERR_INVALID_ARG, "kmm_read_nodes: table_bytes negative (0: the default, %lld)", (long long)RN_DEFAULT_TABLE_BYTES);
    if (n_rounds)
        *n_rounds = 0;
    if (n_reads == 0)
        return KMM_OK;
    if (!best_node)
        return fail(KMM_ERR_INVALID_ARG, "kmm_read_nodes: best_node is NULL");
    KMMCHK(check_k_lut(k, lut));
    return guarded("kmm_read_nodes", [&] {
        const RnArgs a{k, max_freq, also_revcomp ? 1 : 0, n_reads, read_len, table_bytes, read_offsets, n_rounds};
        return read_nodes_impl(ix, bases, lut, a, best_node, best_votes, second_votes, total_votes, n_nodes);
    });
}

int kmm_take_record_hits(kmm_index_t *ix, uint32_t *hits, uint32_t *windows, int64_t capacity, int64_t *n_taken)
{
    if (!ix || !n_taken)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    *n_taken = 0;
    if (capacity < 0 || (capacity > 0 && !hits))
        return fail(KMM_ERR_INVALID_ARG, "kmm_take_record_hits: capacity negative, or hits is NULL");
    if (windows && ix->rhq_mode != 2)
        return fail(KMM_ERR_INVALID_ARG, "kmm_take_record_hits: windows given, and the entries were appended with \"record_hits\" %d: "
                    "windows are kept in mode 2 only (nothing is taken)", ix->rhq_mode);
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix)); // (a sticky or deferred device error: returned, nothing taken)
    const int64_t n = capacity < ix->rhq_pending ? capacity : ix->rhq_pending;
    if (n > 0) {
        const size_t bytes = (size_t)n * 4;
        HIPCHK(hipMemcpy(hits, (const uint32_t *)ix->rhq_hits.p + ix->rhq_head, bytes,
                         is_device_ptr(hits) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        if (windows)
            HIPCHK(hipMemcpy(windows, (const uint32_t *)ix->rhq_win.p + ix->rhq_head, bytes,
                             is_device_ptr(windows) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    }
    ix->rhq_head += n;
    ix->rhq_pending -= n;
    if (ix->rhq_pending == 0)
        ix->rhq_head = 0;
    *n_taken = n;
    return KMM_OK;
}

static int take_kept(kmm_index_t *ix, const char *who, int mate, uint8_t *out, int64_t capacity, int64_t *n_bytes, int64_t *n_records)
{
    if (!ix || !n_bytes || !n_records)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    *n_bytes = *n_records = 0;
    if (capacity < 0 || (capacity > 0 && !out))
        return fail(KMM_ERR_INVALID_ARG, "%s: capacity negative, or out is NULL", who);
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix)); // (a sticky or deferred device error: returned, nothing taken)
    kmm_index::RkQueue &q = ix->rkq[mate];
    unsigned long long tail[2];
    KMMCHK(rkq_tail(q, tail));
    if ((unsigned long long)capacity < tail[0])
        return fail(KMM_ERR_INVALID_ARG, "%s: %llu bytes of %llu records are pending and capacity is %lld: the queue is "
                    "taken whole (nothing is taken)", who, tail[0], tail[1], (long long)capacity);
    if (tail[0] > 0) {
        HIPCHK(hipMemcpy(out, q.text.p, (size_t)tail[0], is_device_ptr(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
        HIPCHK(hipMemset(q.ctl.p, 0, 16));
    }
    q.bound = 0;
    *n_bytes = (int64_t)tail[0];
    *n_records = (int64_t)tail[1];
    return KMM_OK;
}

int kmm_take_kept_records(kmm_index_t *ix, uint8_t *out, int64_t capacity, int64_t *n_bytes, int64_t *n_records)
{
    return take_kept(ix, "kmm_take_kept_records", 0, out, capacity, n_bytes, n_records);
}

int kmm_take_kept_mates(kmm_index_t *ix, int mate, uint8_t *out, int64_t capacity, int64_t *n_bytes, int64_t *n_records)
{
    if (mate != 0 && mate != 1)
        return fail(KMM_ERR_INVALID_ARG, "kmm_take_kept_mates: mate is %d: 0 (the queue of kmm_take_kept_records) or 1 (the mate-2 "
                    "texts of kmm_map_record_pairs)", mate);
    return take_kept(ix, "kmm_take_kept_mates", mate, out, capacity, n_bytes, n_records);
}

// d_in[0, n) (device memory) -> its BGZF members in out (host or device memory; at least kmm_bz::bound(n) bytes), on stream st,
// BZ_ROUND members at a time: deflate into slots, offsets, gather; a round's bytes are known to the host before the next begins.
// timed: the handle whose timing the kernels go to (st is its stream), or null.
constexpr uint32_t BZ_ROUND = 2048; // (128 MiB of slots)

static int bz_compress(hipStream_t st, int n_cu, BzScratch &s, const uint32_t *d_crcT, const uint8_t *d_in, int64_t n, uint8_t *out,
                       int64_t *n_out, kmm_index *timed)
{
    *n_out = 0;
    const int64_t n_members = kmm_bz::member_count(n);
    if (n_members == 0)
        return KMM_OK;
    const bool out_dev = is_device_ptr(out);
    const uint32_t round = (uint32_t)(n_members < (int64_t)BZ_ROUND ? n_members : (int64_t)BZ_ROUND);
    const uint32_t grid_max = (uint32_t)n_cu * 4u; // (persistent workgroups: three to four fit a CU)
    const uint32_t grid = round < grid_max ? round : grid_max;
    KMMCHK(ensure(s.cand, (size_t)grid * kmm_bz::CAND_STRIDE * 2));
    KMMCHK(ensure(s.slots, (size_t)round * kmm_bz::SLOT));
    KMMCHK(ensure(s.sizes, (size_t)round * 4));
    KMMCHK(ensure(s.offs, ((size_t)round + 1) * 8));
    if (!out_dev)
        KMMCHK(ensure(s.comp, (size_t)round * kmm_bz::SLOT));
    int64_t written = 0;
    for (int64_t m0 = 0; m0 < n_members; m0 += round) {
        const uint32_t nm = (uint32_t)(n_members - m0 < (int64_t)round ? n_members - m0 : (int64_t)round);
        const int64_t first = m0 * (int64_t)kmm_bz::BLOCK;
        const int64_t bytes = n - first < (int64_t)nm * kmm_bz::BLOCK ? n - first : (int64_t)nm * kmm_bz::BLOCK;
        uint8_t *dst = out_dev ? out + written : (uint8_t *)s.comp.p;
        ScopedTimer tm;
        if (timed)
            KMMCHK(tm.begin(timed, KMM_KERNEL_BGZF_DEFLATE));
        hipLaunchKernelGGL(kmm_bz::k_bz_deflate, dim3(nm < grid ? nm : grid), dim3(256), 0, st, d_in + first, bytes, nm, d_crcT,
                           (uint16_t *)s.cand.p, (uint8_t *)s.slots.p, (uint32_t *)s.sizes.p);
        KMMCHK(tm.end());
        if (timed)
            KMMCHK(tm.begin(timed, KMM_KERNEL_BGZF_GATHER));
        hipLaunchKernelGGL(kmm_bz::k_bz_offsets, dim3(1), dim3(1024), 0, st, (const uint32_t *)s.sizes.p, nm, (unsigned long long *)s.offs.p);
        hipLaunchKernelGGL(kmm_bz::k_bz_gather, dim3(nm), dim3(256), 0, st, (const uint8_t *)s.slots.p, (const uint32_t *)s.sizes.p,
                           (const unsigned long long *)s.offs.p, dst);
        KMMCHK(tm.end());
        HIPCHK(hipGetLastError());
        unsigned long long total = 0;
        HIPCHK(hipMemcpyAsync(&total, (const unsigned long long *)s.offs.p + nm, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if ((int64_t)total > kmm_bz::bound(bytes))
            return fail(KMM_ERR_INTERNAL, "BGZF writer: %llu bytes of members for %lld bytes of text", total, (long long)bytes);
        if (!out_dev) {
            HIPCHK(hipMemcpyAsync(out + written, s.comp.p, (size_t)total, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        written += (int64_t)total;
    }
    *n_out = written;
    return KMM_OK;
}

int64_t kmm_bgzf_bound(int64_t n)
{
    return kmm_bz::bound(n);
}

int kmm_take_kept_bgzf(kmm_index_t *ix, int mate, uint8_t *out, int64_t capacity, int64_t *n_comp, int64_t *n_bytes, int64_t *n_records)
{
    if (!ix || !n_comp || !n_bytes || !n_records)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    *n_comp = *n_bytes = *n_records = 0;
    if (mate != 0 && mate != 1)
        return fail(KMM_ERR_INVALID_ARG, "kmm_take_kept_bgzf: mate is %d: 0 (the queue of kmm_take_kept_records) or 1 (the mate-2 "
                    "texts of kmm_map_record_pairs)", mate);
    if (capacity < 0 || (capacity > 0 && !out))
        return fail(KMM_ERR_INVALID_ARG, "kmm_take_kept_bgzf: capacity negative, or out is NULL");
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix)); // (a sticky or deferred device error: returned, nothing taken)
    kmm_index::RkQueue &q = ix->rkq[mate];
    unsigned long long tail[2];
    KMMCHK(rkq_tail(q, tail));
    const int64_t need = kmm_bz::bound((int64_t)tail[0]);
    if (capacity < need)
        return fail(KMM_ERR_INVALID_ARG, "kmm_take_kept_bgzf: %llu bytes of %llu records are pending, their members can need %lld "
                    "bytes (kmm_bgzf_bound) and capacity is %lld: the queue is taken whole (nothing is taken)", tail[0], tail[1],
                    (long long)need, (long long)capacity);
    if (tail[0] > 0) {
        KMMCHK(ensure_crc_tables(ix));
        KMMCHK(bz_compress(ix->stream, ix->n_cu, ix->bz, (const uint32_t *)ix->bgzf_crc.p, (const uint8_t *)q.text.p, (int64_t)tail[0], out,
                           n_comp, ix));
        HIPCHK(hipMemset(q.ctl.p, 0, 16));
    }
    q.bound = 0;
    *n_bytes = (int64_t)tail[0];
    *n_records = (int64_t)tail[1];
    return KMM_OK;
}

int kmm_bgzf_compress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t capacity, int64_t *n_out)
{
    if (!n_out)
        return fail(KMM_ERR_INVALID_ARG, "kmm_bgzf_compress: n_out is NULL");
    *n_out = 0;
    if (n < 0 || capacity < 0)
        return fail(KMM_ERR_INVALID_ARG, "kmm_bgzf_compress: negative size");
    if (capacity < kmm_bz::bound(n))
        return fail(KMM_ERR_INVALID_ARG, "kmm_bgzf_compress: the members of %lld bytes can need %lld bytes (kmm_bgzf_bound) and "
                    "capacity is %lld (nothing is written)", (long long)n, (long long)kmm_bz::bound(n), (long long)capacity);
    if (n == 0)
        return KMM_OK;
    if (!in || !out)
        return fail(KMM_ERR_INVALID_ARG, "kmm_bgzf_compress: in / out is NULL");
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(KMM_ERR_HIP, "no HIP device available: libkmm has no CPU fallback");
    }
    HIPCHK(hipSetDevice(device));
    int n_cu = 0;
    HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device));
    Stream st; // (destroyed after the buffers)
    BzScratch s;
    DevBuf d_in, d_crc;
    HIPCHK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking));
    std::vector<uint32_t> t(kmm_gz::CRC_TABLE_WORDS);
    for (int kk = 0; kk < 8; ++kk)
        for (uint32_t bb = 0; bb < 256u; ++bb)
            t[(size_t)kk * 256 + bb] = kmm_gz::crc_table_entry(kk, bb);
    for (int kk = 0; kk < kmm_gz::CRC_SHIFT_WORDS; ++kk)
        t[8 * 256 + kk] = kmm_gz::crc_shift_table_entry(kk);
    KMMCHK(ensure(d_crc, t.size() * 4));
    HIPCHK(hipMemcpyAsync(d_crc.p, t.data(), t.size() * 4, hipMemcpyHostToDevice, st));
    const uint8_t *p_in = in;
    if (!is_device_ptr(in)) {
        KMMCHK(ensure(d_in, (size_t)n));
        HIPCHK(hipMemcpyAsync(d_in.p, in, (size_t)n, hipMemcpyHostToDevice, st));
        p_in = (const uint8_t *)d_in.p;
    }
    HIPCHK(hipStreamSynchronize(st));
    const int rc = bz_compress(st, n_cu > 0 ? n_cu : 256, s, (const uint32_t *)d_crc.p, p_in, n, out, n_out, nullptr);
    (void)hipStreamSynchronize(st);
    return rc;
}

int kmm_extract_kmers(int device, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads,
                      int k, const uint8_t *lut, uint64_t *out, int64_t n_out)
{
    KMMCHK(check_k(k));
    if (n_reads < 0 || n_out < 0)
        return fail(KMM_ERR_INVALID_ARG, "negative size");
    if (n_reads == 0)
        return n_out == 0 ? KMM_OK : fail(KMM_ERR_INVALID_ARG, "n_out != 0 for zero reads");
    if (!read_offsets)
        return fail(KMM_ERR_INVALID_ARG, "read_offsets is NULL");
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(KMM_ERR_HIP, "no HIP device available: libkmm has no CPU fallback");
    }
    HIPCHK(hipSetDevice(device));
    const bool offs_dev = is_device_ptr(read_offsets);
    int64_t ends[2];
    if (offs_dev) {
        HIPCHK(hipMemcpy(&ends[0], read_offsets, 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(&ends[1], read_offsets + n_reads, 8, hipMemcpyDeviceToHost));
    } else {
        ends[0] = read_offsets[0];
        ends[1] = read_offsets[n_reads];
        for (int64_t r = 0; r < n_reads; ++r)
            if (read_offsets[r + 1] < read_offsets[r])
                return fail(KMM_ERR_INVALID_ARG, "read_offsets not non-decreasing at read %lld", (long long)r);
    }
    if (ends[0] != 0)
        return fail(KMM_ERR_INVALID_ARG, "read_offsets[0] must be 0");
    const int64_t total = ends[1];
    if (total < 0)
        return fail(KMM_ERR_INVALID_ARG, "read_offsets[n_reads] negative");
    if (total == 0)
        return n_out == 0 ? KMM_OK : fail(KMM_ERR_INVALID_ARG, "n_out != 0 but the reads are empty");
    if (!bases || (n_out > 0 && !out))
        return fail(KMM_ERR_INVALID_ARG, "bases / out is NULL");

    Stream st; // a stream of its own: other handles' work on this device is not stalled (destroyed after the buffers)
    DevBuf d_bases, d_offs, d_lut, d_out, d_bad, d_tf, d_cnt, d_sup;
    int rc = KMM_OK;
    hipError_t e = hipSuccess;
    HIPCHK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking));
    auto copy = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind kind) -> hipError_t {
        hipError_t x = hipMemcpyAsync(dst, src, bytes, kind, st);
        return x == hipSuccess ? hipStreamSynchronize(st) : x;
    };
    const bool out_dev = n_out == 0 || is_device_ptr(out);
    uint8_t lutbuf[256];
    if (lut) {
        if (is_device_ptr(lut))
            e = copy(lutbuf, lut, 256, hipMemcpyDeviceToHost);
        else
            memcpy(lutbuf, lut, 256);
    } else {
        default_lut(lutbuf);
    }
    if (e == hipSuccess && memchr(lutbuf, KMM_LUT_BREAK, 256))
        return fail(KMM_ERR_INVALID_ARG, "kmm_extract_kmers: the lookup table has a break entry (KMM_LUT_BREAK); n_out is "
                    "defined per read, which a break would split");
    unsigned long long bad[2] = {NO_BAD, NO_BAD};
    int64_t produced = 0;
    const int64_t n_tiles = (total + TILE_T - 1) / TILE_T;
    const int64_t sub_tiles = (int64_t)1 << 20; // 1024 super-tiles of 1024 tiles per round
    do {
        if (e != hipSuccess) break;
        ReadsView rv;
        memset(&rv, 0, sizeof rv);
        rv.total = total;
        rv.n_reads = n_reads;
        if (is_device_ptr(bases)) {
            rv.bases = bases;
        } else {
            if ((rc = ensure(d_bases, (size_t)total))) break;
            if ((e = copy(d_bases.p, bases, (size_t)total, hipMemcpyHostToDevice))) break;
            rv.bases = (const uint8_t *)d_bases.p;
        }
        if (offs_dev) {
            rv.offsets = read_offsets;
        } else {
            if ((rc = ensure(d_offs, (size_t)(n_reads + 1) * 8))) break;
            if ((e = copy(d_offs.p, read_offsets, (size_t)(n_reads + 1) * 8, hipMemcpyHostToDevice))) break;
            rv.offsets = (const int64_t *)d_offs.p;
        }
        uint64_t *p_out = out;
        if (!out_dev) {
            if ((rc = ensure(d_out, (size_t)n_out * 8))) break;
            p_out = (uint64_t *)d_out.p;
        }
        const int64_t max_tiles = n_tiles < sub_tiles ? n_tiles : sub_tiles;
        const int max_super = (int)((max_tiles + 1023) / 1024);
        if ((rc = ensure(d_lut, 256))) break;
        if ((rc = ensure(d_bad, 16))) break;
        if ((rc = ensure(d_tf, (size_t)(total / 32 + 2) * 4))) break; // read-start bitset
        if ((rc = ensure(d_cnt, (size_t)max_super * 1024 * 4))) break;
        if ((rc = ensure(d_sup, (size_t)max_super * 4 + 16))) break;
        if ((e = copy(d_lut.p, lutbuf, 256, hipMemcpyHostToDevice))) break;
        if ((e = copy(d_bad.p, bad, 16, hipMemcpyHostToDevice))) break;
        rv.lut = (const uint8_t *)d_lut.p;
        rv.first_bad = (unsigned long long *)d_bad.p;
        rv.start_bits = (const uint32_t *)d_tf.p;
        rv.n_start_words = total / 32 + 2;
        if ((e = hipMemsetAsync(d_tf.p, 0, (size_t)rv.n_start_words * 4, st))) break;
        hipLaunchKernelGGL(k_mark_starts, dim3((unsigned)((n_reads + 256) / 256 < 65536 ? (n_reads + 256) / 256 : 65536)),
                           dim3(256), 0, st, rv.offsets, n_reads, total, (uint32_t *)d_tf.p);
        uint32_t *tile_cnt = (uint32_t *)d_cnt.p;
        uint32_t *super_tot = (uint32_t *)d_sup.p;
        uint32_t *d_total = super_tot + max_super;
        for (int64_t t0 = 0; t0 < n_tiles && rc == KMM_OK; t0 += sub_tiles) {
            const int64_t t1 = t0 + sub_tiles < n_tiles ? t0 + sub_tiles : n_tiles;
            const int n_super = (int)((t1 - t0 + 1023) / 1024);
            int64_t g = t1 - t0;
            if (g > 65536) g = 65536;
            if ((e = hipMemsetAsync(tile_cnt, 0, (size_t)n_super * 1024 * 4, st))) break;
            hipLaunchKernelGGL((k_extract_count<TILE_S, MODE_GENERAL>), dim3((unsigned)g), dim3(256), 0, st, rv,
                               k, t0, t1, tile_cnt);
            hipLaunchKernelGGL(k_rec_scan1, dim3(n_super), dim3(1024), 0, st, tile_cnt, super_tot);
            hipLaunchKernelGGL(k_super_scan, dim3(1), dim3(1024), 0, st, super_tot, n_super, d_total);
            uint32_t sub_total = 0;
            if ((e = hipGetLastError())) break;
            if ((e = copy(&sub_total, d_total, 4, hipMemcpyDeviceToHost))) break;
            if (produced + (int64_t)sub_total > n_out) { // never write past the caller's buffer
                rc = fail(KMM_ERR_INVALID_ARG, "n_out=%lld but the reads hold more k-mers", (long long)n_out);
                break;
            }
            if (sub_total)
                hipLaunchKernelGGL((k_extract_write<TILE_S, MODE_GENERAL>), dim3((unsigned)g), dim3(256), 0, st,
                                   rv, k, t0, t1, tile_cnt, super_tot, p_out + produced);
            produced += sub_total;
        }
        if (rc != KMM_OK || e != hipSuccess) break;
        if ((e = hipGetLastError())) break;
        if ((e = hipStreamSynchronize(st))) break;
        if ((e = copy(bad, d_bad.p, 16, hipMemcpyDeviceToHost))) break;
        if (produced != n_out) {
            rc = fail(KMM_ERR_INVALID_ARG, "n_out=%lld but the reads hold %lld k-mers", (long long)n_out,
                      (long long)produced);
            break;
        }
        if (!out_dev && n_out)
            if ((e = copy(out, d_out.p, (size_t)n_out * 8, hipMemcpyDeviceToHost))) break;
    } while (0);
    (void)hipStreamSynchronize(st);
    if (rc != KMM_OK)
        return rc;
    if (e != hipSuccess)
        return fail(KMM_ERR_HIP, "kmm_extract_kmers: %s", hipGetErrorString(e));
    if (bad[0] != NO_BAD)
        return fail(KMM_ERR_INVALID_BASE, "read byte at offset %llu is not a nucleotide under the "
                    "lookup table (the reference's DNA encoder raises here)", bad[0]);
    return KMM_OK;
}

int kmm_build_index(int device, const uint64_t *kmers, const int32_t *nodes, int64_t n, uint64_t modulo,
                    int32_t *hashes_to_index, int32_t *n_kmers, uint64_t *kmers_out, int32_t *nodes_out,
                    uint16_t *frequencies_out)
{
    if (n < 0 || modulo < 1)
        return fail(KMM_ERR_INVALID_ARG, "n negative or modulo < 1");
    if (n > 0x7FFFFFFFll || modulo > 0x7FFFFFFFull)
        return fail(KMM_ERR_INVALID_ARG, "n / modulo exceed the int32 arrays of the index format");
    if (!hashes_to_index || !n_kmers || (n > 0 && (!kmers || !nodes || !kmers_out || !nodes_out || !frequencies_out)))
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    int ndev = 0;
    hipError_t e0 = hipGetDeviceCount(&ndev);
    if (e0 != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(KMM_ERR_HIP, "no HIP device available: libkmm has no CPU fallback");
    }
    HIPCHK(hipSetDevice(device));
    const uint64_t M = modulo;
    Stream st; // a stream of its own: other handles' work on this device is not stalled (destroyed after the buffers)
    DevBuf d_km, d_nd, d_nk, d_h2i, d_ko, d_no, d_fo;
    BiScratch scratch;
    int rc = KMM_OK;
    hipError_t e = hipSuccess;
    HIPCHK(hipStreamCreateWithFlags(st.put(), hipStreamNonBlocking));
    auto up = [&](DevBuf &b, const void *src, size_t bytes, const void **dev) -> bool {
        if (bytes == 0 || is_device_ptr(src)) {
            *dev = src;
            return true;
        }
        if ((rc = ensure(b, bytes)))
            return false;
        if ((e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st)))
            return false;
        *dev = b.p;
        return true;
    };
    auto down = [&](void *dst, const void *dev, size_t bytes) -> bool {
        if (bytes == 0 || dst == dev)
            return true;
        e = hipMemcpyAsync(dst, dev, bytes, is_device_ptr(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        return e == hipSuccess;
    };
    do {
        const void *p_km = nullptr, *p_nd = nullptr;
        if (!up(d_km, kmers, (size_t)n * 8, &p_km)) break;
        if (!up(d_nd, nodes, (size_t)n * 4, &p_nd)) break;
        // outputs: work in place when the caller's arrays are already on the device
        uint32_t *w_nk = is_device_ptr(n_kmers) ? (uint32_t *)n_kmers : nullptr;
        uint32_t *w_h2i = is_device_ptr(hashes_to_index) ? (uint32_t *)hashes_to_index : nullptr;
        if (!w_nk) { if ((rc = ensure(d_nk, (size_t)M * 4))) break; w_nk = (uint32_t *)d_nk.p; }
        if (!w_h2i) { if ((rc = ensure(d_h2i, (size_t)M * 4))) break; w_h2i = (uint32_t *)d_h2i.p; }
        uint64_t *w_ko = nullptr;
        int32_t *w_no = nullptr;
        uint16_t *w_fo = nullptr;
        if (n > 0) {
            w_ko = is_device_ptr(kmers_out) ? kmers_out : nullptr;
            w_no = is_device_ptr(nodes_out) ? nodes_out : nullptr;
            w_fo = is_device_ptr(frequencies_out) ? frequencies_out : nullptr;
            if (!w_ko) { if ((rc = ensure(d_ko, (size_t)n * 8))) break; w_ko = (uint64_t *)d_ko.p; }
            if (!w_no) { if ((rc = ensure(d_no, (size_t)n * 4))) break; w_no = (int32_t *)d_no.p; }
            if (!w_fo) { if ((rc = ensure(d_fo, (size_t)n * 2))) break; w_fo = (uint16_t *)d_fo.p; }
        }
        if ((rc = bi_build_device(st, (const uint64_t *)p_km, (const int32_t *)p_nd, n, M, w_nk, w_h2i, w_ko, w_no, w_fo, scratch))) break;
        if ((e = hipStreamSynchronize(st))) break;
        if (n > 0) {
            if (!down(kmers_out, w_ko, (size_t)n * 8)) break;
            if (!down(nodes_out, w_no, (size_t)n * 4)) break;
            if (!down(frequencies_out, w_fo, (size_t)n * 2)) break;
        }
        if (!down(n_kmers, w_nk, (size_t)M * 4)) break;
        if (!down(hashes_to_index, w_h2i, (size_t)M * 4)) break;
    } while (0);
    (void)hipStreamSynchronize(st);
    if (rc != KMM_OK)
        return rc;
    if (e != hipSuccess)
        return fail(KMM_ERR_HIP, "kmm_build_index: %s", hipGetErrorString(e));
    return KMM_OK;
}

int kmm_seq_index_build(int device, const uint8_t *bases, const int64_t *seq_offsets, int64_t n_seqs, const int32_t *seq_nodes, int k,
                        const uint8_t *lut, int flags, uint64_t modulo, kmm_seq_index_t **out)
{
    if (!out)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_build: out is NULL");
    *out = nullptr;
    return guarded("kmm_seq_index_build", [&]() -> int {
        std::unique_ptr<kmm_seq_index> s(new kmm_seq_index);
        const int rc = seq_index_build_impl(device, bases, seq_offsets, n_seqs, seq_nodes, k, lut, flags, modulo, *s);
        if (rc != KMM_OK) {
            s.reset(); // (its arrays freed; hipFree leaves no error of ours behind)
            (void)hipGetLastError();
            return rc;
        }
        *out = s.release();
        return KMM_OK;
    });
}

int kmm_seq_index_info(const kmm_seq_index_t *s, int64_t *n_entries, uint64_t *modulo, int64_t *n_windows, int64_t *n_pairs)
{
    if (!s)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_info: the object is NULL");
    if (n_entries)
        *n_entries = s->n_entries;
    if (modulo)
        *modulo = s->modulo;
    if (n_windows)
        *n_windows = s->n_windows;
    if (n_pairs)
        *n_pairs = s->n_pairs;
    return KMM_OK;
}

int kmm_seq_index_fetch(kmm_seq_index_t *s, int32_t *hashes_to_index, int32_t *n_kmers, uint64_t *kmers, int32_t *nodes,
                        uint16_t *frequencies)
{
    if (!s)
        return fail(KMM_ERR_INVALID_ARG, "kmm_seq_index_fetch: the object is NULL");
    return seq_index_fetch_impl(*s, hashes_to_index, n_kmers, kmers, nodes, frequencies);
}

void kmm_seq_index_destroy(kmm_seq_index_t *s)
{
    if (!s)
        return;
    (void)hipSetDevice(s->device);
    delete s;
}

uint64_t kmm_seq_index_modulo(int64_t n_entries)
{
    return si_modulo(n_entries);
}

int kmm_get_stats(kmm_index_t *ix, int reset, uint64_t *n_lookups, uint64_t *n_hits)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    HIPCHK(hipSetDevice(ix->device));
    KMMCHK(drain(ix));
    std::vector<unsigned long long> st(KMM_STAT_BYTES / 8);
    HIPCHK(hipMemcpy(st.data(), ix->stats, KMM_STAT_BYTES, hipMemcpyDeviceToHost));
    unsigned long long tot[2] = {0, 0};
    for (int i = 0; i < KMM_STAT_SHARDS; ++i) {
        tot[0] += st[(size_t)i * KMM_STAT_STRIDE];
        tot[1] += st[(size_t)i * KMM_STAT_STRIDE + 1];
    }
    if (n_lookups)
        *n_lookups = tot[0];
    if (n_hits)
        *n_hits = tot[1];
    if (reset)
        HIPCHK(hipMemset(ix->stats, 0, KMM_STAT_BYTES));
    return KMM_OK;
}

int kmm_set_timing(kmm_index_t *ix, int enabled)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    ix->timing = enabled != 0;
    return KMM_OK;
}

int kmm_get_timing(kmm_index_t *ix, int kernel_id, double *kernel_ms, int64_t *n_launches)
{
    if (!ix)
        return fail(KMM_ERR_INVALID_ARG, "idx is NULL");
    if (kernel_id < 0 || kernel_id >= KMM_N_KERNELS)
        return fail(KMM_ERR_INVALID_ARG, "kernel_id %d outside [0, %d)", kernel_id, KMM_N_KERNELS);
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipStreamSynchronize(ix->stream));
    for (auto &ev : ix->ev_used) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ev.start, ev.stop));
        ix->ms_total[ev.kernel_id] += ms;
        ix->launches[ev.kernel_id] += 1;
        ix->ev_free.push_back(std::move(ev));
    }
    ix->ev_used.clear();
    if (kernel_ms)
        *kernel_ms = ix->ms_total[kernel_id];
    if (n_launches)
        *n_launches = ix->launches[kernel_id];
    ix->ms_total[kernel_id] = 0.0;
    ix->launches[kernel_id] = 0;
    return KMM_OK;
}

int kmm_set_record_regions(kmm_index_t *ix, const kmm_region_t *regions, int n_regions, int keep_unplaced)
{
    return guarded("kmm_set_record_regions", [&]() -> int {
        if (!ix || n_regions < 0 || (n_regions > 0 && !regions))
            return fail(KMM_ERR_INVALID_ARG, "kmm_set_record_regions: NULL argument or n_regions negative");
        if (n_regions > KMM_MAX_RECORD_REGIONS)
            return fail(KMM_ERR_INVALID_ARG, "kmm_set_record_regions: %d regions, at most %d are taken", n_regions, KMM_MAX_RECORD_REGIONS);
        // the list is judged whole before the handle changes: by id and by name, each usable only when every region has one
        std::vector<kmm_sel::Interval> by_id, by_name;
        std::vector<std::string> names;
        bool ids = true, named = true;
        for (int i = 0; i < n_regions; ++i) {
            const kmm_region_t &r = regions[i];
            if (r.beg < 0 || r.end <= r.beg)
                return fail(KMM_ERR_INVALID_ARG, "kmm_set_record_regions: region %d is [%lld, %lld): beg < 0 or end <= beg", i,
                            (long long)r.beg, (long long)r.end);
            if (r.ref_name && (r.ref_name[0] == 0 || strlen(r.ref_name) > (size_t)KMM_MAX_REGION_NAME_BYTES || !strcmp(r.ref_name, "*")))
                return fail(KMM_ERR_INVALID_ARG, "kmm_set_record_regions: region %d: ref_name is empty, \"*\" or longer than %d bytes", i,
                            KMM_MAX_REGION_NAME_BYTES);
            ids = ids && r.ref_id >= 0;
            named = named && r.ref_name != nullptr;
            if (r.ref_name)
                names.push_back(r.ref_name);
        }
        if (n_regions > 0 && !ids && !named)
            return fail(KMM_ERR_INVALID_ARG, "kmm_set_record_regions: every region needs a ref_id (>= 0; BAM) or every region a ref_name (SAM)");
        std::sort(names.begin(), names.end());
        names.erase(std::unique(names.begin(), names.end()), names.end());
        if (!named)
            names.clear();
        for (int i = 0; i < n_regions; ++i) {
            const kmm_region_t &r = regions[i];
            if (ids)
                by_id.push_back(kmm_sel::Interval{(int64_t)r.ref_id, r.beg, r.end});
            if (named)
                by_name.push_back(kmm_sel::Interval{(int64_t)(std::lower_bound(names.begin(), names.end(), std::string(r.ref_name)) - names.begin()),
                                                    r.beg, r.end});
        }
        kmm_sel::merge_intervals(by_id);
        kmm_sel::merge_intervals(by_name);
        std::vector<int64_t> refs;
        for (const kmm_sel::Interval &v : by_id)
            if (refs.empty() || refs.back() != v.ref)
                refs.push_back(v.ref);
        if (refs.size() > (size_t)KMM_MAX_REGION_REFERENCES || names.size() > (size_t)KMM_MAX_REGION_REFERENCES)
            return fail(KMM_ERR_INVALID_ARG, "kmm_set_record_regions: regions on %zu distinct references, at most %d are taken",
                        std::max(refs.size(), names.size()), KMM_MAX_REGION_REFERENCES);
        // the device buffer: [intervals by id][intervals by name][name offsets][name bytes]
        const size_t off_name_iv = by_id.size() * sizeof(kmm_sel::Interval), off_name_off = off_name_iv + by_name.size() * sizeof(kmm_sel::Interval),
                     off_names = off_name_off + (names.size() + 1) * 4;
        std::vector<uint8_t> h(off_names);
        if (!by_id.empty())
            memcpy(h.data(), by_id.data(), off_name_iv);
        if (!by_name.empty())
            memcpy(h.data() + off_name_iv, by_name.data(), off_name_off - off_name_iv);
        uint32_t at = 0;
        for (size_t i = 0; i <= names.size(); ++i) {
            memcpy(h.data() + off_name_off + 4 * i, &at, 4);
            if (i < names.size()) {
                h.insert(h.end(), names[i].begin(), names[i].end());
                at += (uint32_t)names[i].size();
            }
        }
        HIPCHK(hipSetDevice(ix->device));
        HIPCHK(hipStreamSynchronize(ix->stream)); // (kernels of a call before may read the list in place)
        if (n_regions > 0) {
            KMMCHK(ensure(ix->sel_buf, h.size() + 64));
            HIPCHK(hipMemcpy(ix->sel_buf.p, h.data(), h.size(), hipMemcpyHostToDevice));
        }
        ix->sel_n_regions = n_regions;
        ix->sel_keep_unplaced = n_regions > 0 && keep_unplaced ? 1 : 0;
        ix->sel_iv_id.swap(by_id);
        ix->sel_iv_name.swap(by_name);
        ix->sel_names.swap(names);
        ix->sel_off_name_iv = off_name_iv;
        ix->sel_off_name_off = off_name_off;
        ix->sel_off_names = off_names;
        return KMM_OK;
    });
}

} // extern "C"

namespace {
#include "kmm_params_host.hpp" // the rows of the parameter table that need the handle, find_param: behind everything they call
} // namespace

extern "C" {

int kmm_set_param(kmm_index_t *ix, const char *name, int64_t value)
{
    if (!ix || !name)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    HIPCHK(hipSetDevice(ix->device));
    const kmm_params::Row *row = find_param(name);
    if (!(row && row->no_sync))
        HIPCHK(hipStreamSynchronize(ix->stream)); // scratch layouts depend on the knobs
    char why[256];
    if (kmm_params::set_refused(row, name, value, why, sizeof why))
        return fail(KMM_ERR_INVALID_ARG, "%s", why);
    if (row->set)
        return row->set(ix, *row, value);
    kmm_params::store(*row, *ix, value);
    return KMM_OK;
}

int kmm_get_param(kmm_index_t *ix, const char *name, int64_t *value)
{
    if (!ix || !name || !value)
        return fail(KMM_ERR_INVALID_ARG, "NULL argument");
    const kmm_params::Row *row = find_param(name);
    if (!row && !strncmp(name, "stats_slot_", 11)) // raw counter <n> of the statistics block; slots 4.. are only written by diagnostic builds
        return get_stat_slot(ix, atoi(name + 11), name, value);
    char why[256];
    if (kmm_params::get_refused(row, name, why, sizeof why))
        return fail(KMM_ERR_INVALID_ARG, "%s", why);
    if (row->get)
        return row->get(ix, *row, value);
    *value = kmm_params::load(*row, *ix, *ix);
    return KMM_OK;
}

} // extern "C"
