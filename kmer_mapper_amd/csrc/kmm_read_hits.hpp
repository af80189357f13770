// kmm_read_hits.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace.
// kmm_read_hits: per-read counts of index hits and of windows looked up.  The tile front end (kmm_tile.hpp)
// and the membership probe (kmm_probe.hpp, member_batch) joined, with the read id of every window carried to the output.
// The position -> read search is plain C++ (KMM_RH_HD): the CPU tier compiles this header with g++.
#pragma once

#if defined(__HIPCC__)
#define KMM_RH_HD __host__ __device__ __forceinline__
#else
#include <cstdint>
#define KMM_RH_HD inline
#endif

// The read of flat position p is the largest r with offsets[r] <= p: empty reads (offsets[r] == offsets[r + 1]) are
// skipped, whatever their number.  Searched inside [lo, hi]: returns the largest r in [lo, hi] with offs[r] <= p, or lo
// when there is none.  Every index read lies inside [lo, hi], whatever the offsets hold (they need not be sorted for the
// search to end and to stay in bounds; the result then means nothing).
KMM_RH_HD int64_t rh_read_of_pos(const int64_t *offs, int64_t lo, int64_t hi, int64_t p)
{
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2; // in (lo, hi]
        if (offs[mid] <= p)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// First read of tile t (tile_len positions per tile), t = 0 .. n_tiles: the read of position t * tile_len, clamped to the
// last read for positions at or behind `total` (the entry behind the last tile).  n_reads >= 1.
KMM_RH_HD int64_t rh_tile_first_read(const int64_t *offs, int64_t n_reads, int64_t total, int64_t t, int64_t tile_len)
{
    int64_t p = t * tile_len;
    if (p >= total)
        p = total - 1;
    return rh_read_of_pos(offs, 0, n_reads - 1, p);
}

// A lane's cursor over the reads while it walks forward over its positions: `r` is the read of the position it was
// last moved to, `next` = offs[r + 1] (the first position behind read r; INT64_MAX at the last read), `hi` the last read
// a position of the lane's tile can belong to.
struct RhCursor {
    int64_t r, next, hi;
};

KMM_RH_HD void rh_cursor_load(const int64_t *offs, RhCursor &c)
{
    c.next = c.r < c.hi ? offs[c.r + 1] : INT64_MAX;
}

KMM_RH_HD RhCursor rh_cursor_at(const int64_t *offs, int64_t lo, int64_t hi, int64_t p)
{
    RhCursor c;
    c.hi = hi < lo ? lo : hi;
    c.r = rh_read_of_pos(offs, lo, c.hi, p);
    rh_cursor_load(offs, c);
    return c;
}

// Move to position p (not before the position of the last move).  One compare in registers while p stays inside the
// read; a search, not a walk, when it leaves it: a run of empty reads costs its logarithm.
KMM_RH_HD void rh_cursor_advance(const int64_t *offs, RhCursor &c, int64_t p)
{
    if (p < c.next)
        return;
    c.r = rh_read_of_pos(offs, c.r + 1, c.hi, p);
    rh_cursor_load(offs, c);
}

// ---- records mode: the reads are the records of raw two-line FASTA / FASTQ text, and the read of a position
// is arithmetic on its line number (the newlines before it): lines_per_record = 1 << period_shift, 2 or 4.
KMM_RH_HD uint32_t rh_record_of_line(uint32_t line, uint32_t period_shift)
{
    return line >> period_shift;
}

// The line of byte j of a lane whose first byte lies on line `line0`; nl: bit i = the lane's byte i is '\n' (a newline
// belongs to the line it ends).
KMM_RH_HD uint32_t rh_line_of_byte(uint32_t line0, uint32_t nl, int j)
{
    return line0 + (uint32_t)__builtin_popcount(nl & ((1u << j) - 1u));
}

// One run of a read's windows inside a lane.
struct RhRun {
    uint32_t r, h, w;
};

// Fold the lane's S windows (valid / hit: bit j = window j exists / is in the index) into runs of one record each.  A run
// that ends inside the lane goes to flush(r, h, w) — a lane's first byte often lies in the record before its window's
// ("\nC\n>" of ">\nA\n>\nC\n>\nG\n" at k = 1), and nothing here counts on a lane's windows sharing one record — and the last
// one stays in `run` for the reduction across the wavefront.  A lane without windows leaves the record of its first byte
// with sums of zero; flush may be called with sums of zero.
template <int S, typename Flush>
KMM_RH_HD void rh_fold_records(uint32_t line0, uint32_t nl, uint32_t period_shift, uint32_t valid, uint32_t hit, RhRun &run,
                               Flush &&flush)
{
    run.r = rh_record_of_line(line0, period_shift);
    run.h = run.w = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < S; ++j) {
        if (!((valid >> j) & 1u))
            continue;
        const uint32_t r = rh_record_of_line(rh_line_of_byte(line0, nl, j), period_shift);
        if (r != run.r) {
            flush(run.r, run.h, run.w);
            run.r = r;
            run.h = run.w = 0;
        }
        run.h += (hit >> j) & 1u;
        run.w += 1u;
    }
}

#if defined(__HIPCC__)

// tile_first_read[t] for t = 0 .. n_tiles (rh_tile_first_read): one search over all offsets per tile boundary, so that the
// lanes of the main kernel search only among the reads of their own tile.
__global__ void __launch_bounds__(256) k_rh_tile_reads(const int64_t *__restrict__ offs, int64_t n_reads, int64_t total,
                                                       int64_t n_tiles, int64_t tile_len, int64_t *__restrict__ tile_first_read)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t <= n_tiles; t += (int64_t)gridDim.x * blockDim.x)
        tile_first_read[t] = rh_tile_first_read(offs, n_reads, total, t, tile_len);
}

// One run of a read's windows: flushed with one atomic per output that has something to add.
__device__ __forceinline__ void rh_emit(uint32_t *__restrict__ hits, uint32_t *__restrict__ windows, int64_t r, uint32_t h,
                                        uint32_t w)
{
    if (h)
        atomicAdd(&hits[r], h);
    if (windows && w)
        atomicAdd(&windows[r], w);
}

// The reduction.  Every lane brings the last run of its positions: the read `key` and the packed sums v = hits | windows
// << 16 (a wavefront looks up at most 64 S windows: both halves stay far below 2^15, bit 31 is free).  Lanes are in
// position order, so the keys do not decrease along the wavefront and the lanes of one read are neighbours: a segment.
// A suffix scan segmented by key — six ds_bpermute steps; bit 31 marks a lane whose sum already reaches its segment's
// tail — leaves every segment's total in its head lane, which issues the atomics: one per read and wavefront instead of
// one per window.  Call with all 64 lanes active.
__device__ __forceinline__ void rh_wave_reduce(uint32_t *__restrict__ hits, uint32_t *__restrict__ windows, int64_t key,
                                               uint32_t v)
{
#ifdef KMM_RH_STUB_REDUCE // diagnostic build (tools/read_hits_bench.py): no scan, no atomics; the sums stay live, the outputs are wrong
    if (v == 0xFFFFFFFFu)
        rh_emit(hits, windows, key, v, v);
    return;
#endif
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t klo = (uint32_t)key, khi = (uint32_t)((uint64_t)key >> 32);
    // (every shuffle on its own line, outside || and ?: — a shuffle that a lane skips reads nothing from that lane)
    const uint32_t plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
    const bool head = lane == 0 || plo != klo || phi != khi;
    const uint32_t next_head = __shfl_down((uint32_t)head, 1);
    const bool tail = lane == 63 || next_head != 0u;
    uint32_t x = v | (tail ? 0x80000000u : 0u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_down(x, d);
        if (lane + d < 64 && !(x >> 31))
            x += y; // (y's bit 31 comes along: closed once the lanes added so far reach the tail)
    }
    if (head)
        rh_emit(hits, windows, key, x & 0xFFFFu, (x >> 16) & 0x7FFFu);
}

// MODE_UNIFORM: reads of rv.read_len bytes, the read of position p is p / read_len.  MODE_GENERAL: ragged reads through
// rv.offsets and tile_first_read — or, for reads of one length that took the ragged front end (shorter than 16 bases, or a
// table with breaks), rv.offsets == null and the division again.  The read id never comes from the read-start bitset:
// breaks set bits there too.
// MODE_RECORDS, MODE_RECORDS_BRK: raw two-line FASTA / FASTQ text; the reads are its records and the read id
// comes from the line number that stage 1 of the records front end forms (TileLines).  hits / windows point at the piece's
// first entry, zeroed on the stream before the launch: a record without a window keeps its zeros.
template <int S, int MODE, int PROBE>
__global__ void __launch_bounds__(256) k_read_hits(ReadsView rv, IndexView iv, int k, int max_freq, int also_rc,
                                                   int64_t n_tiles, const int64_t *__restrict__ tile_first_read,
                                                   uint32_t *__restrict__ hits, uint32_t *__restrict__ windows)
{
    __shared__ TileSmem<S> sm;
    constexpr int T = TileSmem<S>::T;
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    const TileConst tc = tile_const(rv, k);
    const bool by_offsets = MODE == MODE_GENERAL && rv.offsets != nullptr;
    [[maybe_unused]] TileLines tl;
    if constexpr (mode_is_records(MODE)) {
        __shared__ uint32_t line_stage[2 * TileSmem<S>::NV];
        tl.stage = line_stage;
    }
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint64_t q[S];
        uint32_t valid;
        if constexpr (mode_is_records(MODE))
            valid = tile_kmers<S, MODE>(rv, tc, tile, k, sm, q, (int)threadIdx.x, &tl);
        else
            valid = tile_kmers<S, MODE>(rv, tc, tile, k, sm, q);
        uint32_t hit = 0;
        if (__builtin_amdgcn_ballot_w64(valid != 0)) {
            hit = member_batch<S, PROBE>(iv, q, valid, max_freq);
            const uint32_t miss = valid & ~hit;
            if (also_rc && __builtin_amdgcn_ballot_w64(miss != 0)) { // the other orientation of the windows that missed
#pragma unroll
                for (int j = 0; j < S; ++j)
                    q[j] = revcomp(q[j], k);
                hit |= member_batch<S, PROBE>(iv, q, miss, max_freq);
            }
        }
        if constexpr (mode_is_records(MODE)) {
            RhRun run;
            rh_fold_records<S>(tl.line, tl.nl, (uint32_t)__popc(rv.period_mask), valid, hit, run,
                               [&](uint32_t r, uint32_t h, uint32_t w) { rh_emit(hits, windows, (int64_t)r, h, w); });
            rh_wave_reduce(hits, windows, (int64_t)run.r, run.h | (run.w << 16));
            continue;
        }
        // fold the lane's windows into runs of (read, hits, windows); a run that ends inside the lane goes out at once
        int64_t p0 = tile * T + (int64_t)threadIdx.x * S;
        if (p0 >= rv.total)
            p0 = rv.total - 1; // (a lane behind the chunk: no windows, the key of the last position)
        int64_t run_r;
        uint32_t run_h = 0, run_w = 0;
#ifdef KMM_RH_STUB_SEARCH // diagnostic build (tools/read_hits_bench.py): a read id that costs nothing; the outputs are wrong
        if (by_offsets) {
            run_r = (p0 >> 7) < rv.n_reads ? (p0 >> 7) : rv.n_reads - 1;
            run_h = (uint32_t)__popc(hit);
            run_w = (uint32_t)__popc(valid);
        } else
#endif
        if (by_offsets) {
            RhCursor c = rh_cursor_at(rv.offsets, tile_first_read[tile], tile_first_read[tile + 1], p0);
            run_r = c.r;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (!((valid >> j) & 1u))
                    continue;
                rh_cursor_advance(rv.offsets, c, p0 + j);
                if (c.r != run_r) {
                    rh_emit(hits, windows, run_r, run_h, run_w);
                    run_r = c.r;
                    run_h = run_w = 0;
                }
                run_h += (hit >> j) & 1u;
                run_w += 1u;
            }
        } else {
            uint64_t o;
            uint64_t r = fastdiv((uint64_t)p0, rv.read_len, rv.read_len_magic, &o);
            run_r = (int64_t)r;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (j > 0 && ++o == rv.read_len) {
                    o = 0;
                    ++r;
                }
                if (!((valid >> j) & 1u))
                    continue;
                if ((int64_t)r != run_r) {
                    rh_emit(hits, windows, run_r, run_h, run_w);
                    run_r = (int64_t)r;
                    run_h = run_w = 0;
                }
                run_h += (hit >> j) & 1u;
                run_w += 1u;
            }
        }
        rh_wave_reduce(hits, windows, run_r, run_h | (run_w << 16));
    }
}

#endif // __HIPCC__
