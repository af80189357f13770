// kmm_read_nodes.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace.
// kmm_read_nodes: per read, the node that most of its k-mers map to.  Two walks over k_read_hits's front end
// (kmm_tile.hpp, kmm_probe.hpp, the read search of kmm_read_hits.hpp) with sinks that count every matching entry, as
// CountSink does: k_rn_count sums the votes per read (they size the table and cut the rounds), k_rn_vote adds every vote to
// the (read, node) cell of an open-addressing table in HBM.  k_rn_best / k_rn_second / k_rn_unpack then reduce the cells to
// the per-read answers with max and add, which commute: the outputs do not depend on the order the threads ran in.
// The arithmetic (keys, best words, slots, rounds) is kmm_read_nodes_plan.hpp.
#pragma once

struct RnCell {
    unsigned long long key; // rn_key, RN_EMPTY_KEY while free
    uint32_t count, pad;
};
static_assert(sizeof(RnCell) == RN_CELL_BYTES, "one 16-byte cell");

// Suffix sums along the wavefront segmented by `key`: lanes whose keys equal their neighbours' form a segment, `head` is set in
// the first lane of each, and that lane gets the segment's sum.  rh_wave_reduce's scan with the value and the "reached the
// tail" mark in words of their own: vote counts do not fit its packed halves.  Call with all 64 lanes active.
__device__ __forceinline__ uint32_t rn_wave_segments(uint64_t key, uint32_t v, bool &head)
{
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t klo = (uint32_t)key, khi = (uint32_t)(key >> 32);
    // (every shuffle on its own line, outside || and ?: — a shuffle that a lane skips reads nothing from that lane)
    const uint32_t plo = __shfl_up(klo, 1), phi = __shfl_up(khi, 1);
    head = lane == 0 || plo != klo || phi != khi;
    const uint32_t next_head = __shfl_down((uint32_t)head, 1);
    uint32_t closed = (lane == 63 || next_head != 0u) ? 1u : 0u;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_down(x, d);
        const uint32_t yc = __shfl_down(closed, d);
        if (lane + d < 64 && !closed) {
            x += y;
            closed = yc;
        }
    }
    return x;
}

// The read of each of the lane's S windows (p0: the lane's first position, clamped into the chunk), as k_read_hits finds it:
// through the offsets and the tile's first read, or by division for reads of one length.  rid[j] of a window that is not
// valid is the read of the last valid one before it (of p0 when there is none).
template <int S, int MODE>
__device__ __forceinline__ void rn_window_reads(const ReadsView &rv, const int64_t *__restrict__ tile_first_read, int64_t tile,
                                                int64_t p0, uint32_t valid, int64_t (&rid)[S])
{
    if (MODE == MODE_GENERAL && rv.offsets != nullptr) {
        RhCursor c = rh_cursor_at(rv.offsets, tile_first_read[tile], tile_first_read[tile + 1], p0);
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if ((valid >> j) & 1u)
                rh_cursor_advance(rv.offsets, c, p0 + j);
            rid[j] = c.r;
        }
    } else {
        uint64_t o;
        uint64_t r = fastdiv((uint64_t)p0, rv.read_len, rv.read_len_magic, &o);
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (j > 0 && ++o == rv.read_len) {
                o = 0;
                ++r;
            }
            rid[j] = (int64_t)r;
        }
    }
}

// One vote per matching entry (mapper.pyx:60-68, CountSink's rule), counted per window.
template <int S>
struct RnCountSink {
    static constexpr bool FIRST_ENDS = false;
    uint32_t c[S];
    __device__ __forceinline__ void match(int u, uint32_t) { ++c[u]; }
};

// total_votes[r] += the votes of read r, for every read of the chunk; grand[0] += all of them.  total_votes is zeroed before
// the launch.  Modes as k_read_hits (MODE_UNIFORM, MODE_GENERAL with or without offsets).
template <int S, int MODE, int PROBE>
__global__ void __launch_bounds__(256) k_rn_count(ReadsView rv, IndexView iv, int k, int max_freq, int also_rc, int64_t n_tiles,
                                                  const int64_t *__restrict__ tile_first_read, uint32_t *__restrict__ total_votes,
                                                  unsigned long long *__restrict__ grand)
{
    __shared__ TileSmem<S> sm;
    constexpr int T = TileSmem<S>::T;
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    const TileConst tc = tile_const(rv, k);
    unsigned long long mine = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint64_t q[S];
        const uint32_t valid = tile_kmers<S, MODE>(rv, tc, tile, k, sm, q);
        RnCountSink<S> sink;
#pragma unroll
        for (int j = 0; j < S; ++j)
            sink.c[j] = 0;
        if (__builtin_amdgcn_ballot_w64(valid != 0)) {
            walk_batch<S, PROBE>(iv, q, valid, max_freq, sink);
            if (also_rc) { // both orientations of every window, as map_one_tile
#pragma unroll
                for (int j = 0; j < S; ++j)
                    q[j] = revcomp(q[j], k);
                walk_batch<S, PROBE>(iv, q, valid, max_freq, sink);
            }
        }
        int64_t p0 = tile * T + (int64_t)threadIdx.x * S;
        if (p0 >= rv.total)
            p0 = rv.total - 1; // (a lane behind the chunk: no windows, the key of the last position)
        int64_t rid[S];
        rn_window_reads<S, MODE>(rv, tile_first_read, tile, p0, valid, rid);
        // fold the lane's windows into runs of one read; a run that ends inside the lane goes out at once
        int64_t run_r = rid[0];
        uint32_t run_v = 0;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            if (!((valid >> j) & 1u))
                continue;
            if (rid[j] != run_r) {
                if (run_v)
                    atomicAdd(&total_votes[run_r], run_v);
                run_r = rid[j];
                run_v = 0;
            }
            run_v += sink.c[j];
            mine += sink.c[j];
        }
        bool head;
        const uint32_t sum = rn_wave_segments((uint64_t)run_r, run_v, head);
        if (head && sum)
            atomicAdd(&total_votes[run_r], sum);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        mine += __shfl_xor(mine, d);
    if ((threadIdx.x & 63u) == 0 && mine)
        atomicAdd(grand, mine);
}

// cells[slot of key].count += inc: the key is claimed with a 64-bit compare-and-swap, acting on the value it returns (free, or
// already this key: ours; another key: the next slot), the count added beside it.  The table has at least twice as many slots
// as the round has votes, so a free slot is met; the walk is bounded by `slots` all the same, and a walk that finds none
// (the two passes disagreed: a bug) raises err[0] instead of spinning.
__device__ __forceinline__ void rn_table_add(RnCell *__restrict__ cells, uint64_t slots, uint64_t key, uint32_t inc,
                                             unsigned long long *__restrict__ err)
{
    uint64_t s = rn_home(key, slots);
    for (uint64_t tries = 0; tries < slots; ++tries) {
        const unsigned long long prev = atomicCAS(&cells[s].key, (unsigned long long)RN_EMPTY_KEY, (unsigned long long)key);
        if (prev == RN_EMPTY_KEY || prev == key) {
            atomicAdd(&cells[s].count, inc);
            return;
        }
        if (++s == slots)
            s = 0;
    }
    atomicMax(err, 1ull);
}

// (window, node) per matching entry -> votes of (read, node).  Equal pairs that follow each other in the lane's walk are folded
// in registers (pend_*) before they go to memory: a read that sits on one node sends one add per lane and walk, not one per
// window.  rel[u]: the read of window u relative to the round's first.
template <int S>
struct RnVoteSink {
    static constexpr bool FIRST_ENDS = false;
    RnCell *cells;
    uint64_t slots;
    unsigned long long *err;
    uint32_t rel[S];
    uint64_t pend_key = RN_EMPTY_KEY;
    uint32_t pend_n = 0;
    __device__ __forceinline__ void flush()
    {
        if (pend_n)
            rn_table_add(cells, slots, pend_key, pend_n, err);
    }
    __device__ __forceinline__ void match(int u, uint32_t node)
    {
        const uint64_t key = rn_key(rel[u], node);
        if (key == pend_key) {
            ++pend_n;
        } else {
            flush();
            pend_key = key;
            pend_n = 1;
        }
    }
};

// The votes of reads [r0, r0 + n_round) — the windows of tiles [tile_lo, tile_hi), which cover those reads' positions; windows
// of other reads in the two end tiles are not looked up — into `cells` (cleared before the launch).  What is left in a lane's
// registers after its walks is summed over equal neighbouring lanes first (rn_wave_segments): a 150-base read on one node
// reaches the table with one or two adds per wavefront.
template <int S, int MODE, int PROBE>
__global__ void __launch_bounds__(256) k_rn_vote(ReadsView rv, IndexView iv, int k, int max_freq, int also_rc, int64_t tile_lo,
                                                 int64_t tile_hi, const int64_t *__restrict__ tile_first_read, int64_t r0,
                                                 int64_t n_round, RnCell *__restrict__ cells, uint64_t slots,
                                                 unsigned long long *__restrict__ err)
{
    __shared__ TileSmem<S> sm;
    constexpr int T = TileSmem<S>::T;
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    const TileConst tc = tile_const(rv, k);
    for (int64_t tile = tile_lo + blockIdx.x; tile < tile_hi; tile += gridDim.x) {
        uint64_t q[S];
        uint32_t valid = tile_kmers<S, MODE>(rv, tc, tile, k, sm, q);
        int64_t p0 = tile * T + (int64_t)threadIdx.x * S;
        if (p0 >= rv.total)
            p0 = rv.total - 1;
        int64_t rid[S];
        rn_window_reads<S, MODE>(rv, tile_first_read, tile, p0, valid, rid);
        RnVoteSink<S> sink{cells, slots, err, {}};
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const int64_t d = rid[j] - r0;
            if (d < 0 || d >= n_round)
                valid &= ~(1u << j);
            sink.rel[j] = (uint32_t)d;
        }
        if (__builtin_amdgcn_ballot_w64(valid != 0)) {
            walk_batch<S, PROBE>(iv, q, valid, max_freq, sink);
            if (also_rc) {
#pragma unroll
                for (int j = 0; j < S; ++j)
                    q[j] = revcomp(q[j], k);
                walk_batch<S, PROBE>(iv, q, valid, max_freq, sink);
            }
        }
        bool head;
        const uint32_t sum = rn_wave_segments(sink.pend_key, sink.pend_n, head);
        if (head && sum)
            rn_table_add(cells, slots, sink.pend_key, sum, err);
    }
}

__global__ void __launch_bounds__(256) k_rn_clear(RnCell *__restrict__ cells, uint64_t slots)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x)
        reinterpret_cast<uint4 *>(cells)[i] = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
}

// One thread per slot: a cell in use raises its read's best word (rn_best_word: ties go to the smaller node) and counts one
// distinct node.  n_nodes may be null.
__global__ void __launch_bounds__(256) k_rn_best(const RnCell *__restrict__ cells, uint64_t slots, int64_t r0,
                                                 unsigned long long *__restrict__ best, uint32_t *__restrict__ n_nodes)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 c = reinterpret_cast<const uint4 *>(cells)[i];
        const uint64_t key = (uint64_t)c.x | ((uint64_t)c.y << 32);
        if (key == RN_EMPTY_KEY)
            continue;
        const int64_t r = r0 + rn_key_read(key);
        atomicMax(&best[r], (unsigned long long)rn_best_word(c.z, rn_key_node(key)));
        if (n_nodes)
            atomicAdd(&n_nodes[r], 1u);
    }
}

// Behind k_rn_best: the cells of every node but the read's best raise second_votes.
__global__ void __launch_bounds__(256) k_rn_second(const RnCell *__restrict__ cells, uint64_t slots, int64_t r0,
                                                   const unsigned long long *__restrict__ best, uint32_t *__restrict__ second_votes)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < slots; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 c = reinterpret_cast<const uint4 *>(cells)[i];
        const uint64_t key = (uint64_t)c.x | ((uint64_t)c.y << 32);
        if (key == RN_EMPTY_KEY)
            continue;
        const int64_t r = r0 + rn_key_read(key);
        if ((int32_t)rn_key_node(key) != rn_best_node(best[r]))
            atomicMax(&second_votes[r], c.z);
    }
}

// best word -> best_node (-1 without a vote) and best_votes (may be null).
__global__ void __launch_bounds__(256) k_rn_unpack(const unsigned long long *__restrict__ best, int64_t n_reads,
                                                   int32_t *__restrict__ best_node, uint32_t *__restrict__ best_votes)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t w = best[r];
        best_node[r] = rn_best_node(w);
        if (best_votes)
            best_votes[r] = rn_best_votes(w);
    }
}
