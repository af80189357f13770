// kmm_seqindex.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace.
// kmm_seq_index_build: sequences -> distinct (k-mer, node) pairs in order of first occurrence.  The arithmetic
// that needs no device is kmm_seqindex_plan.hpp; the host driver is kmm_seqindex_host.hpp.
//   emit          k_extract_count (kmm_kernels.hpp) counts the windows of every tile under the read-start bitset — sequence
//                 starts and, through k_mark_breaks, break bytes — the two-level scan of the records front end turns the
//                 counts into bases, and k_si_write regenerates the k-mers and writes each beside the node of its sequence,
//                 with both strands directly followed by its reverse complement: the pair list P.
//   de-duplicate  a set of pair INDICES in an open-addressing table of 32-bit slots (0 = empty, else index + 1): k_si_insert
//                 leaves in the slot of every distinct pair the smallest index that holds it, k_si_keep marks exactly those
//                 indices, a scan and k_si_compact write them out in order: D.
// Work per pair does not depend on how often the pair repeats: a repeat costs the probe to its pair's slot, one compare and —
// only while the slot still holds a larger index — one atomicMin.
#pragma once

// Negative nodes: the first sequence that has one -> first_bad[1].
__global__ void k_si_check_nodes(const int32_t *__restrict__ seq_nodes, int64_t n_seqs, unsigned long long *first_bad)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_seqs; r += (int64_t)gridDim.x * blockDim.x)
        if (seq_nodes[r] < 0)
            atomicMin(&first_bad[1], (unsigned long long)r);
}

// k_extract_write with the node of every window and, with `both`, its reverse complement.  The sequence of a window is that
// of its first position, searched among the sequences of the lane's own tile (tile_first_seq: k_rh_tile_reads) and then
// walked (RhCursor), as k_read_hits does under a break table: the read-start bitset also holds the breaks and cannot say.
// out_kmers / out_nodes point at the round's first pair; tile_pre / super_pre are the round's scanned WINDOW counts.
template <int S>
__global__ void __launch_bounds__(256) k_si_write(ReadsView rv, int k, int both, int64_t tile_begin, int64_t tile_end,
                                                  const uint32_t *__restrict__ tile_pre, const uint32_t *__restrict__ super_pre,
                                                  const int64_t *__restrict__ tile_first_seq, const int32_t *__restrict__ seq_nodes,
                                                  uint64_t *__restrict__ out_kmers, int32_t *__restrict__ out_nodes)
{
    __shared__ TileSmem<S> sm;
    __shared__ uint32_t s_wave[4];
    constexpr int T = TileSmem<S>::T;
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    const TileConst tc = tile_const(rv, k);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = tile_begin + blockIdx.x; tile < tile_end; tile += gridDim.x) {
        uint64_t q[S];
        const uint32_t valid = tile_kmers<S, MODE_GENERAL>(rv, tc, tile, k, sm, q);
        const uint32_t c = (uint32_t)__popc(valid);
        const uint32_t inc = wave_scan_incl(c);
        if (lane == 63)
            s_wave[wave] = inc;
        __syncthreads();
        uint32_t base = inc - c;
        for (int w = 0; w < wave; ++w)
            base += s_wave[w];
        const int64_t lt = tile - tile_begin;
        uint64_t slot = (uint64_t)super_pre[lt >> 10] + tile_pre[lt] + base;
        if (valid) {
            const int64_t p0 = tile * T + (int64_t)threadIdx.x * S; // (a lane with a window lies inside the chunk)
            RhCursor cur = rh_cursor_at(rv.offsets, tile_first_seq[tile], tile_first_seq[tile + 1], p0);
#pragma unroll
            for (int j = 0; j < S; ++j) {
                if (!((valid >> j) & 1u))
                    continue;
                rh_cursor_advance(rv.offsets, cur, p0 + j);
                const int32_t node = seq_nodes ? seq_nodes[cur.r] : (int32_t)cur.r;
                if (both) {
                    out_kmers[2 * slot] = q[j];
                    out_kmers[2 * slot + 1] = revcomp(q[j], k);
                    out_nodes[2 * slot] = node;
                    out_nodes[2 * slot + 1] = node;
                } else {
                    out_kmers[slot] = q[j];
                    out_nodes[slot] = node;
                }
                ++slot;
            }
        }
        __syncthreads(); // s_wave is rewritten by the next tile
    }
}

// Pair i into the set.  Slots never empty again and never change the pair they stand for (an index is only ever replaced by a
// smaller index of an EQUAL pair), so a load that returns an old value still names the slot's pair, and all copies of a pair
// end their probe in the one slot the first of them claimed: it ends holding their smallest index + 1.  At most half of the
// slots are ever taken (si_table_slots): every probe ends.
__global__ void __launch_bounds__(256) k_si_insert(const uint64_t *__restrict__ kmers, const int32_t *__restrict__ nodes, int64_t n,
                                                   uint32_t *table, uint32_t mask)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t km = kmers[i];
        const int32_t nd = nodes[i];
        const uint32_t me = (uint32_t)i + 1u;
        uint32_t h = (uint32_t)si_mix(km, nd) & mask;
        for (;;) {
            uint32_t v = __hip_atomic_load(&table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (v == 0u) {
                v = atomicCAS(&table[h], 0u, me); // (act on what the slot held, not on the load)
                if (v == 0u)
                    break;
            }
            const uint32_t j = v - 1u;
            if (kmers[j] == km && nodes[j] == nd) {
                if (j > (uint32_t)i)
                    atomicMin(&table[h], me);
                break;
            }
            h = (h + 1u) & mask;
        }
    }
}

// Behind ALL inserts (the next launch on the stream): keep[i] = 1 iff the slot of pair i holds i + 1, i.e. i is the first
// occurrence of its pair.  Read-only on the table.
__global__ void __launch_bounds__(256) k_si_keep(const uint64_t *__restrict__ kmers, const int32_t *__restrict__ nodes, int64_t n,
                                                 const uint32_t *__restrict__ table, uint32_t mask, uint32_t *__restrict__ keep)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t km = kmers[i];
        const int32_t nd = nodes[i];
        uint32_t h = (uint32_t)si_mix(km, nd) & mask;
        uint32_t k = 0u;
        for (;;) {
            const uint32_t v = table[h];
            if (v == 0u)
                break; // (cannot happen behind the inserts: the pair has a slot; ends the probe whatever the table holds)
            const uint32_t j = v - 1u;
            if (j == (uint32_t)i) {
                k = 1u;
                break;
            }
            if (j < (uint64_t)n && kmers[j] == km && nodes[j] == nd)
                break;
            h = (h + 1u) & mask;
        }
        keep[i] = k;
    }
}

// pos = exclusive scan of keep: the kept pairs, in order.
__global__ void __launch_bounds__(256) k_si_compact(const uint64_t *__restrict__ kmers, const int32_t *__restrict__ nodes, int64_t n,
                                                    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ pos,
                                                    uint64_t *__restrict__ out_kmers, int32_t *__restrict__ out_nodes)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (keep[i]) {
            out_kmers[pos[i]] = kmers[i];
            out_nodes[pos[i]] = nodes[i];
        }
}
