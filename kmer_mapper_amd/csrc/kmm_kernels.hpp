// kmm_kernels.hpp — part of libkmm (MI355X / gfx950); included by kmm.hip inside its anonymous namespace.
// Direct-path kernels (k_map_reads, k_map_kmers), operator facades, index repack.
#pragma once

// ------------------------------------------------------------------------------------------------
// K1 (direct path): fused reads -> counts, every probe goes to HBM.  Used for small batches and for
// indexes whose hash space cannot be cut into L2-sized partitions.
// ------------------------------------------------------------------------------------------------

template <int S, int MODE, int PROBE>
__device__ __forceinline__ void map_one_tile(const ReadsView &rv, const IndexView &iv, const TileConst &tc,
                                             int64_t tile, int k, int max_freq, int also_rc, TileSmem<S> &sm,
                                             NodeAgg &agg, LaneStats &st)
{
    uint64_t q[S];
    const uint32_t valid = tile_kmers<S, MODE>(rv, tc, tile, k, sm, q);
    if (__builtin_amdgcn_ballot_w64(valid != 0)) {
        probe_batch<S, PROBE>(iv, agg, st, q, valid, max_freq);
        if (also_rc) {
#pragma unroll
            for (int j = 0; j < S; ++j)
                q[j] = revcomp(q[j], k);
            probe_batch<S, PROBE>(iv, agg, st, q, valid, max_freq);
        }
    }
}

// The schedule of a direct launch (host side: direct_schedule, kmm.hip): body(unit) for every unit of [begin, end) that
// this workgroup owns.  `queue` == null: static grid-stride schedule.  Otherwise the workgroups are persistent (one per CU
// slot) and pull chunks of `chunk` consecutive units from a device-side counter, so that the last round of a large launch
// does not leave CU slots idle while a few workgroups finish their fixed share.  Call with the whole workgroup.
template <typename Body>
__device__ __forceinline__ void for_owned_units(int64_t begin, int64_t end, unsigned long long *queue, int chunk, Body &&body)
{
    __shared__ unsigned long long s_next;
    if (!queue) {
        for (int64_t unit = begin + blockIdx.x; unit < end; unit += gridDim.x)
            body(unit);
        return;
    }
    for (;;) {
        if (threadIdx.x == 0)
            s_next = atomicAdd(queue, (unsigned long long)chunk);
        __syncthreads();
        // (one value for the whole workgroup: read through the scalar unit, the chunk's bounds then live in SGPRs like the
        // static schedule's)
        const uint64_t grabbed = s_next;
        const int64_t first = begin + (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(grabbed >> 32)) << 32) |
                                                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)grabbed));
        __syncthreads(); // s_next may be rewritten only after everyone has read it
        if (first >= end)
            break;
        const int64_t last = first + chunk < end ? first + chunk : end;
        for (int64_t unit = first; unit < last; ++unit)
            body(unit);
    }
}

// The units are tiles.
template <int S, int MODE, int PROBE>
__global__ void __launch_bounds__(256) k_map_reads(ReadsView rv, IndexView iv, int k, int max_freq,
                                                   int also_rc, int64_t tile_begin, int64_t tile_end,
                                                   unsigned long long *queue, int chunk)
{
    __shared__ TileSmem<S> sm;
    __shared__ NodeAgg agg;
    LaneStats st;
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    agg_init(agg); // ordered before the first agg_add by the barriers inside tile_kmers
    const TileConst tc = tile_const(rv, k);
    for_owned_units(tile_begin, tile_end, queue, chunk, [&](int64_t tile) {
        map_one_tile<S, MODE, PROBE>(rv, iv, tc, tile, k, max_freq, also_rc, sm, agg, st);
    });
    stats_reduce(agg, st);
    __syncthreads();
    agg_flush(iv, agg);
}

// ------------------------------------------------------------------------------------------------
// K2: operator-level lookup, uint64 k-mers already in HBM (drop-in for map_kmers_to_graph_index).
// ------------------------------------------------------------------------------------------------
template <int U, int PROBE>
__device__ __forceinline__ void map_kmer_span(const uint64_t *__restrict__ kmers, int64_t n, int64_t base,
                                              const IndexView &iv, int max_freq, int also_rc, int k,
                                              NodeAgg &agg, LaneStats &st)
{
    uint64_t q[U];
    uint32_t valid = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        int64_t i = base + (int64_t)u * 256 + threadIdx.x;
        q[u] = 0;
        if (i < n) {
            q[u] = __builtin_nontemporal_load(&kmers[i]);
            valid |= 1u << u;
        }
    }
    probe_batch<U, PROBE>(iv, agg, st, q, valid, max_freq);
    if (also_rc) {
#pragma unroll
        for (int u = 0; u < U; ++u)
            q[u] = revcomp(q[u], k);
        probe_batch<U, PROBE>(iv, agg, st, q, valid, max_freq);
    }
}

// The units are spans of 256*U k-mers.
template <int U, int PROBE>
__global__ void __launch_bounds__(256) k_map_kmers(const uint64_t *__restrict__ kmers, int64_t n,
                                                   IndexView iv, int max_freq, int also_rc, int k,
                                                   unsigned long long *queue, int chunk)
{
    __shared__ NodeAgg agg;
    LaneStats st;
    agg_init(agg);
    __syncthreads();
    constexpr int64_t span = (int64_t)256 * U;
    const int64_t n_spans = (n + span - 1) / span;
    for_owned_units(0, n_spans, queue, chunk, [&](int64_t s) {
        map_kmer_span<U, PROBE>(kmers, n, s * span, iv, max_freq, also_rc, k, agg, st);
    });
    stats_reduce(agg, st);
    __syncthreads();
    agg_flush(iv, agg);
}

// General path helper: the read-start bitset of the chunk, bit p set iff some read starts at base position p
// (offsets[r] for r = 0..n_reads; offsets[n_reads] = total marks the end).  The words are cleared by the caller.
__global__ void k_mark_starts(const int64_t *__restrict__ offs, int64_t n_reads, int64_t total, uint32_t *__restrict__ bits)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = offs[r];
        if (o >= 0 && o <= total) // (out-of-range offsets are reported by k_check_offsets / the host checks)
            atomicOr(&bits[o >> 5], 1u << (o & 31));
    }
}

// Reads of one length whose lookup table has a break entry take the ragged front end: their arithmetic starts
// r * read_len, r = 0 .. n_reads, into the same bitset (no offsets array is made for them).
__global__ void k_mark_uniform_starts(int64_t n_reads, int64_t read_len, uint32_t *__restrict__ bits)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_reads; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = r * read_len;
        atomicOr(&bits[o >> 5], 1u << (o & 31));
    }
}

// The marking stream of k_mark_breaks and k_mark_low_quals: one byte per base position in, one bit per position (touched
// only where something is marked) out.  A marked position b is a one-base read: bits b and b + 1 of the read-start bitset.
// With "no read start inside (p, p + k - 1]" (k >= 2) the window that starts at b dies of bit b + 1 and every earlier window
// that contains b of bit b; the windows behind b live.  So the mapping kernels need no notion of a break or of a quality.
// Per round a workgroup takes 16 KiB: MARK_U 16-byte loads per lane, all issued before the first is consumed;
// classify(four words) turns a lane's 16 bytes into a 16-position mask, two neighbouring lanes make one 32-position word,
// and the even lane ORs word | word << 1 into the bitset — one atomic per word that holds a mark, plus one for bit 31's
// carry into the next word.  The marks may be DENSE (low qualities: at a few per cent of low bases most 32-position words
// hold one).  The word is still written with a no-return atomic OR by the even lane that formed it: the alternative — the
// incoming carry by shuffle and a plain load / OR / store of the word, atomics only at the wave's seam — puts a dependent
// load between the compare and the store and has two write forms to keep right, while the atomic is issued and forgotten
// and the L2 does the same read-modify-write either way (measured: the plain form takes 3.3 times as long,
// profiles/flat_quality/README.md); the words are 1/8 of the bytes read.
// Bytes past the end are staged as 0, which the classifier may mark: positions at or past `total` are cleared before
// anything else, so the highest mark is bit `total`: word total / 32 of the total / 32 + 2 the bitset has, whatever the
// bytes hold.  Returns the number of positions this lane marked (before the << 1).
constexpr int MARK_U = 4;
template <typename Classify>
__device__ __forceinline__ uint32_t mark_stream(const uint8_t *__restrict__ bytes, int64_t total, uint32_t *__restrict__ bits,
                                                Classify classify)
{
    const bool aligned = (((uintptr_t)bytes) & 15u) == 0;
    constexpr int64_t SPAN = (int64_t)256 * 16 * MARK_U;
    uint32_t n_marked = 0;
    for (int64_t base = (int64_t)blockIdx.x * SPAN; base < total; base += (int64_t)gridDim.x * SPAN) {
        uint32_t w[MARK_U][4];
#pragma unroll
        for (int u = 0; u < MARK_U; ++u) {
            const int64_t p = base + ((int64_t)u * 256 + threadIdx.x) * 16;
            if (p + 16 <= total) {
                u32x4 x;
                if (aligned)
                    x = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(bytes + p));
                else
                    __builtin_memcpy(&x, bytes + p, 16); // (one unaligned 16-byte load: rec_load16)
                w[u][0] = x[0]; w[u][1] = x[1]; w[u][2] = x[2]; w[u][3] = x[3];
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    w[u][i] = p < total ? tile_load_bytes4(bytes, total, p + 4 * i) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < MARK_U; ++u) {
            const int64_t p = base + ((int64_t)u * 256 + threadIdx.x) * 16;
            uint32_t m = classify(w[u]);
            const int64_t left = total - p;
            if (left < 16)
                m &= left > 0 ? (1u << left) - 1u : 0u;
            n_marked += (uint32_t)__popc(m);
            const uint32_t hi = (uint32_t)__shfl_xor((int)m, 1);
            if (!(threadIdx.x & 1u)) {
                const uint32_t word = m | (hi << 16);
                if (word) {
                    const int64_t wi = p >> 5; // (p is a multiple of 32 for even lanes)
                    atomicOr(&bits[wi], word | (word << 1));
                    if (word >> 31)
                        atomicOr(&bits[wi + 1], 1u);
                }
            }
        }
    }
    return n_marked;
}

// Break bytes (lookup table entry KMM_LUT_BREAK: N, IUPAC letters) -> the read-start bitset.  This pre-pass runs only for
// calls whose table has a break entry.  Each byte goes through an LDS copy of the table (1 = break).
__global__ void __launch_bounds__(256) k_mark_breaks(const uint8_t *__restrict__ bases, int64_t total,
                                                     const uint8_t *__restrict__ lut, uint32_t *__restrict__ bits)
{
    __shared__ uint32_t s_brk[256];
    s_brk[threadIdx.x] = lut[threadIdx.x] == KMM_LUT_BREAK ? 1u : 0u;
    __syncthreads();
    mark_stream(bases, total, bits, [&](const uint32_t (&w)[4]) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            m |= s_brk[(w[i >> 2] >> (8 * (i & 3))) & 0xFFu] << i;
        return m;
    });
}

// Quality bytes of flat reads (kmm_map_reads_qual with "min_base_quality" > 0) -> the read-start bitset:
// quals[p] < thresh (unsigned; thresh = qual_base + Q, 1 .. 126) marks base p; runs behind k_mark_starts / k_mark_breaks in
// stream order, on the same words.  The test is a compare, four bytes per operation (bytes_below, kmm_records.hpp), so
// there is no LDS table.  The low bytes each lane marked are summed over the wave and the workgroup, and added once per
// workgroup to statistics slot KMM_STAT_QUAL_MASKED.
__global__ void __launch_bounds__(256) k_mark_low_quals(const uint8_t *__restrict__ quals, int64_t total, uint32_t thresh,
                                                        uint32_t *__restrict__ bits, unsigned long long *__restrict__ stats)
{
    __shared__ uint32_t s_wave[4];
    uint32_t n_low = mark_stream(quals, total, bits, [&](const uint32_t (&w)[4]) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            m |= flags_to_bits(bytes_below(w[i], thresh)) << (4 * i);
        return m;
    });
    n_low = wave_sum(n_low);
    if ((threadIdx.x & 63) == 0)
        s_wave[threadIdx.x >> 6] = n_low;
    __syncthreads();
    const uint32_t n_wg = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    if (threadIdx.x == 0 && n_wg)
        atomicAdd(&stats[(size_t)(blockIdx.x % KMM_STAT_SHARDS) * KMM_STAT_STRIDE + KMM_STAT_QUAL_MASKED], (unsigned long long)n_wg);
}

// read_offsets must be non-decreasing; checked here (off the host's critical path) and reported at the
// next synchronising call.  A violation cannot make the map kernels touch memory out of bounds.
__global__ void k_check_offsets(const int64_t *__restrict__ offs, int64_t n_reads, unsigned long long *first_bad)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * blockDim.x)
        if (offs[r + 1] < offs[r])
            atomicMin(&first_bad[2], (unsigned long long)r);
}

__global__ void k_iota_offsets(int64_t *out, int64_t n_reads, int64_t read_len)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n_reads)
        out[i] = i * read_len;
}

// ------------------------------------------------------------------------------------------------
// Operator façade kernels (not on the fused path).
// ------------------------------------------------------------------------------------------------
// get_kmer_hashes_from_chunk_sequence (util.py:71-75) as an operator: the k-mers of all reads,
// flattened in (read, offset) order, i.e. in increasing base position.  The output slot of a window is
// therefore the number of valid windows before it: pass 1 counts the valid windows per tile, a
// two-level scan turns the counts into tile bases, pass 2 regenerates the k-mers (cheaper than storing
// them) and writes each lane's run of up to S k-mers contiguously.
template <int S, int MODE>
__global__ void __launch_bounds__(256) k_extract_count(ReadsView rv, int k, int64_t tile_begin,
                                                       int64_t tile_end, uint32_t *__restrict__ tile_cnt)
{
    __shared__ TileSmem<S> sm;
    __shared__ uint32_t s_wave[4];
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    const TileConst tc = tile_const(rv, k);
    for (int64_t tile = tile_begin + blockIdx.x; tile < tile_end; tile += gridDim.x) {
        uint64_t q[S];
        uint32_t c = (uint32_t)__popc(tile_kmers<S, MODE>(rv, tc, tile, k, sm, q));
#pragma unroll
        for (int d = 32; d > 0; d >>= 1)
            c += __shfl_xor(c, d);
        if ((threadIdx.x & 63) == 0)
            s_wave[threadIdx.x >> 6] = c;
        __syncthreads();
        if (threadIdx.x == 0)
            tile_cnt[tile - tile_begin] = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    }
}

// Exclusive scan of the (<= 1024) super-tile totals, in place; total -> *total_out.
__global__ void __launch_bounds__(1024) k_super_scan(uint32_t *super_tot, int n_super, uint32_t *total_out)
{
    __shared__ uint32_t s_a[1024];
    const int t = threadIdx.x;
    const uint32_t c = t < n_super ? super_tot[t] : 0u;
    s_a[t] = c;
    __syncthreads();
    block_scan_1024(s_a);
    if (t < n_super)
        super_tot[t] = s_a[t] - c;
    if (t == 1023)
        *total_out = s_a[t];
}

template <int S, int MODE>
__global__ void __launch_bounds__(256) k_extract_write(ReadsView rv, int k, int64_t tile_begin,
                                                       int64_t tile_end, const uint32_t *__restrict__ tile_pre,
                                                       const uint32_t *__restrict__ super_pre,
                                                       uint64_t *__restrict__ out)
{
    __shared__ TileSmem<S> sm;
    __shared__ uint32_t s_wave[4];
    sm.lut[threadIdx.x] = rv.lut[threadIdx.x];
    const TileConst tc = tile_const(rv, k);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = tile_begin + blockIdx.x; tile < tile_end; tile += gridDim.x) {
        uint64_t q[S];
        const uint32_t valid = tile_kmers<S, MODE>(rv, tc, tile, k, sm, q);
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
#pragma unroll
        for (int j = 0; j < S; ++j)
            if ((valid >> j) & 1u)
                out[slot++] = q[j];
        __syncthreads(); // s_wave is rewritten by the next tile
    }
}

// in_graph_index (mapper.pyx:112-127): first match wins, no frequency filter.  The membership walk of one k-mer with the
// largest bound there is: stored frequencies are 16-bit, so every entry passes.
__global__ void k_in_index(const uint64_t *__restrict__ kmers, int64_t n, IndexView iv,
                           uint8_t *__restrict__ out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t q[1] = {kmers[i]};
        MemberSink sink;
        if (iv.wide)
            walk_wide<1, false>(iv, q, 1u, INT_MAX, sink);
        else
            walk_narrow<1, false>(iv, q, 1u, INT_MAX, sink);
        out[i] = (uint8_t)sink.bits;
    }
}

// ------------------------------------------------------------------------------------------------
// Index repack (on the GPU, at load).  Also the validation the reference does not do.
// err bit 0: bucket outside [0, n_entries); bit 1: node outside [0, max_node_id].
// The direct view is packed either from the caller's arrays (IdxRaw: at kmm_index_create, small indexes) or later,
// on the first batch that takes the direct path, from the radix view's bucket-ordered copy (IdxRx: large indexes
// keep ONE view resident until the other is needed — HBM budget).
// ------------------------------------------------------------------------------------------------
struct IdxRaw {
    const int32_t *h2i, *nk;
    const uint64_t *kmers;
    const int32_t *nodes;
    const uint16_t *freqs;
    __device__ __forceinline__ int64_t count(uint64_t h) const { return nk[h]; }
    __device__ __forceinline__ int64_t start(uint64_t h) const { return h2i[h]; }
    __device__ __forceinline__ int64_t node(int64_t l) const { return nodes[l]; }
};

struct IdxRx { // entries in bucket order: validated and clamped when the radix view was built
    const uint32_t *pstart;
    const uint64_t *kmers;
    const uint32_t *nodes;
    const uint16_t *freqs;
    __device__ __forceinline__ int64_t count(uint64_t h) const { return (int64_t)(pstart[h + 1] - pstart[h]); }
    __device__ __forceinline__ int64_t start(uint64_t h) const { return pstart[h]; }
    __device__ __forceinline__ int64_t node(int64_t l) const { return nodes[l]; }
};

// validation only (the direct view of a large index is packed later, the errors are reported at creation)
__global__ void k_validate_index(const int32_t *__restrict__ h2i, const int32_t *__restrict__ nk,
                                 const int32_t *__restrict__ nodes, uint64_t modulo, int64_t n_entries,
                                 int64_t max_node_id, uint32_t *err)
{
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (uint64_t)gridDim.x * blockDim.x;
    uint32_t e = 0;
    for (uint64_t h = gid; h < modulo; h += stride) {
        const int32_t c = nk[h], s = h2i[h];
        if (c > 0 && (s < 0 || (int64_t)s + c > n_entries))
            e |= 1u;
    }
    for (uint64_t l = gid; l < (uint64_t)n_entries; l += stride) {
        const int32_t nd = nodes[l];
        if (nd < 0 || (int64_t)nd > max_node_id)
            e |= 2u;
    }
    if (e)
        atomicOr(err, e);
}

template <typename Src>
__global__ void k_pack_buckets(Src src, uint64_t modulo, int64_t n_entries, int64_t max_node_id,
                               uint4 *__restrict__ buckets, uint32_t *err)
{
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < modulo;
         h += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t c = src.count(h), s = src.start(h);
        uint4 b = make_uint4(0u, 0u, 0u, 0u);
        if (c > 0) { // c <= 0: `for j in range(n_local_hits)` runs zero times (mapper.pyx:58)
            if (s < 0 || s + c > n_entries) {
                atomicOr(err, 1u);
            } else if (c == 1) {
                const uint64_t km = src.kmers[s];
                int64_t nd = src.node(s);
                if (nd < 0 || nd > max_node_id)
                    nd = 0; // reported by k_pack_entries / k_validate_index
                b = make_uint4((uint32_t)km, (uint32_t)(km >> 32), (uint32_t)nd,
                               ((uint32_t)src.freqs[s] << 16) | 1u);
            } else if (c <= 3) {
                const uint32_t f0 = kmer_fp16(src.kmers[s]), f1 = kmer_fp16(src.kmers[s + 1]);
                const uint32_t f2 = c > 2 ? kmer_fp16(src.kmers[s + 2]) : 0u;
                b = make_uint4((uint32_t)s, (uint32_t)c, f0 | (f1 << 16), (f2 << 16) | 4u | 2u);
            } else {
                b = make_uint4((uint32_t)s, (uint32_t)c, 0u, 2u);
            }
        }
        buckets[h] = b;
    }
}

// Wide layout: 32-byte bucket = halves A (2h) and B (2h+1), up to two entries inline.
template <typename Src>
__global__ void k_pack_buckets_wide(Src src, uint64_t modulo, int64_t n_entries, int64_t max_node_id,
                                    uint4 *__restrict__ buckets, uint32_t *err)
{
    for (uint64_t h = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; h < modulo;
         h += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t c = src.count(h), s = src.start(h);
        uint4 a = make_uint4(0u, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
        if (c > 0) {
            if (s < 0 || s + c > n_entries) {
                atomicOr(err, 1u);
            } else if (c <= 2) {
                for (int j = 0; j < (int)c; ++j) {
                    const uint64_t km = src.kmers[s + j];
                    int64_t nd = src.node(s + j);
                    if (nd < 0 || nd > max_node_id)
                        nd = 0; // reported by k_pack_entries / k_validate_index
                    const uint4 e = make_uint4((uint32_t)km, (uint32_t)(km >> 32), (uint32_t)nd,
                                               ((uint32_t)src.freqs[s + j] << 16) | (uint32_t)c);
                    if (j == 0)
                        a = e;
                    else
                        b = e;
                }
            } else {
                a = make_uint4((uint32_t)s, (uint32_t)c, 0u, 3u);
            }
        }
        buckets[2 * h] = a;
        buckets[2 * h + 1] = b;
    }
}

template <typename Src>
__global__ void k_pack_entries(Src src, int64_t n, int64_t max_node_id, uint4 *__restrict__ entries, uint32_t *err)
{
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < n;
         l += (int64_t)gridDim.x * blockDim.x) {
        uint64_t km = src.kmers[l];
        int64_t nd = src.node(l);
        if (nd < 0 || nd > max_node_id) {
            atomicOr(err, 2u);
            nd = 0;
        }
        entries[l] = make_uint4((uint32_t)km, (uint32_t)(km >> 32), (uint32_t)nd, (uint32_t)src.freqs[l]);
    }
}

// Word-blocked Bloom filter over the index k-mers: two bits inside one 32-bit word per key.
__global__ void k_build_bloom(const uint64_t *__restrict__ kmers, int64_t n, uint32_t n_words,
                              uint32_t *__restrict__ occ)
{
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < n; l += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t hs = kmers[l] * 0x9E3779B97F4A7C15ull;
        const uint32_t wi = (uint32_t)(((hs >> 32) * (uint64_t)n_words) >> 32);
        atomicOr(&occ[wi], (1u << ((hs >> 7) & 31u)) | (1u << ((hs >> 12) & 31u)));
    }
}

// Occupancy bitmap with 2^shift bits per bucket: every index entry sets bit (h << shift) | (fingerprint of
// its k-mer & (2^shift - 1)).  The bitmap must be zeroed first.
__global__ void k_build_occ(const uint64_t *__restrict__ kmers, int64_t n, uint64_t modulo, uint64_t magic,
                            int shift, uint32_t *__restrict__ occ)
{
    const uint32_t sub = (1u << shift) - 1u;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < n; l += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t km = kmers[l];
        const uint64_t bit = (fastmod(km, modulo, magic) << shift) | (kmer_fp16(km) & sub);
        atomicOr(&occ[bit >> 5], 1u << (bit & 31u));
    }
}
