/*
 * kmm.h — C ABI of libkmm.so: the MI355X (gfx950) implementation of kmer_mapper's
 * k-mer extraction + Kmer-Index lookup + per-node count accumulation hot path.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; nothing here knows about
 * numpy, torch or Python.  Every entry point names the reference interface it replaces
 * (paths relative to the ivargr/kmer_mapper tree).  INTEGRATION.md shows the ctypes binding a
 * reference maintainer would add.
 *
 * Conventions
 *   - All functions return KMM_OK (0) or a negative KMM_ERR_* code and never throw across the
 *     ABI; kmm_last_error() returns a thread-local human-readable message for the last failure.
 *   - Input pointers are BORROWED for the duration of the call.  Every data pointer may be a
 *     host pointer or a device (HBM) pointer on the handle's device; the library detects which
 *     (hipPointerGetAttributes).  Host inputs are staged to HBM by the call (the host buffer is free
 *     again when the call returns); device inputs are used in place by kernels that run after the
 *     call returns: they must already be complete (produced on another stream -> synchronise that
 *     stream first) and must stay valid and unmodified until the next synchronising call.
 *   - One handle = one device + one HIP stream + one uint32 node-count vector in HBM.
 *     map calls are asynchronous on the handle's stream and ACCUMULATE into the count vector
 *     (the reference sums per-chunk vectors, command_line_interface.py:124-130);
 *     kmm_get_node_counts / kmm_synchronize are the synchronisation points.  Calls on one
 *     handle must be serialised by the caller; different handles are independent.
 *   - Errors found by the kernels of a map call (a byte that is not a nucleotide, a malformed record,
 *     decreasing read offsets) are reported by the next synchronising call and then STAY on the handle:
 *     the chunk's valid windows are already counted by then (the reference raises before counting anything
 *     of that chunk), so every later synchronising call fails with the same code until kmm_reset_counts
 *     clears the counts and the error together — an error of the calls before it that no synchronising call
 *     has reported yet included: it is never reported against the counts of the calls after the reset.  A
 *     caller-owned buffer (kmm_bind_counts) must be zeroed by the caller as well.
 *   - Counts are uint32 and wrap modulo 2^32 exactly like the reference (mapper.pyx:37,68).
 */
#ifndef KMM_H
#define KMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMM_OK 0
#define KMM_ERR_INVALID_ARG (-1)   /* NULL pointer, k out of range, negative size ...            */
#define KMM_ERR_HIP (-2)           /* a HIP runtime call failed (message has file:line)          */
#define KMM_ERR_INDEX (-3)         /* index arrays inconsistent (bucket out of range, bad node)  */
#define KMM_ERR_INVALID_BASE (-4)  /* a read byte is not a nucleotide under the lookup table     */
#define KMM_ERR_NOMEM (-5)
#define KMM_ERR_MALFORMED (-6)     /* raw FASTA/FASTQ chunk does not have the expected line structure */
#define KMM_ERR_INTERNAL (-7)      /* self-check of the radix path failed (k-mers emitted by pass 1 != gathered by
                                      pass 2 != probed by pass 3): counts are NOT returned; sticky until
                                      kmm_reset_counts */

#define KMM_MAX_K 31               /* a k-mer is packed 2 bits/base into a uint64; bionumpy's
                                      get_kmers (util.py:72) is used with k <= 31                */

/*
 * The `lut` argument of every entry point is uint8[256] with three kinds of entries: 0..3 = the base's 2-bit code, 0xFF = not
 * a nucleotide (KMM_ERR_INVALID_BASE), and KMM_LUT_BREAK = a BREAK: a byte that is a base of its read but has no code (N, the
 * IUPAC ambiguity letters).  No k-mer that contains a break byte is looked up, forward or reverse complement, and it raises no
 * error; the windows on either side that do not contain it are mapped as before (what jellyfish, KMC and others do with N).
 *   - A break inside a read is equivalent to ending the read before it and starting a new one behind it; the library
 *     represents it that way (two bits of the read-start bitset), so the mapping kernels are the ragged ones.
 *   - *n_records is unaffected (the record is still one record); kmm_get_stats' n_lookups counts only the surviving windows.
 *   - k == 1 with a table that has a break entry is KMM_ERR_INVALID_ARG (the bitset rule "no read start inside (p, p+k-1]"
 *     cannot kill a window of one base; refused rather than silently counted).
 *   - kmm_extract_kmers with a break entry is KMM_ERR_INVALID_ARG: its n_out contract is per read.
 *   - kmm_map_packed takes no table: its caller expresses breaks through read_starts.
 *   - lut == NULL stays the reference's table (N -> A, every other letter an error): nothing changes without a break entry.
 *   - Tables with a break entry take the device routes only (the host packer, "host_pack_threads", serves lut == NULL), and
 *     reads of one length with such a table take the ragged front end (they do not count in "flat_uniform_batches").
 */
#define KMM_LUT_BREAK 0xFE

typedef struct kmm_index kmm_index_t;

/* Library / device probes. */
const char *kmm_version(void);
const char *kmm_last_error(void);
int kmm_device_count(int *n_devices);
/* "0000:5a:00.0" of HIP device `device` (hipDeviceGetPCIBusId): /sys/bus/pci/devices/<id>/numa_node and local_cpulist
 * name the host cores and memory next to that GPU — where a rank's packing threads and page-locked buffers belong
 * (kmer_mapper_amd/distributed.py bind_to_gpu_numa_node; the reference leaves its workers unbound). */
int kmm_device_pci_bus_id(int device, char *out, int out_bytes);

/*
 * kmm_index_create — replaces the typed-memoryview binding of the five index arrays at
 * mapper.pyx:22-29 and the cucounter table construction at gpu_counter.py:13-16.
 * Arrays are the attributes of graph_kmer_index.KmerIndex after convert_to_int32()
 * (util.py:60-62): hashes_to_index int32[modulo], n_kmers int32[modulo], kmers uint64[n_entries],
 * nodes int32[n_entries], frequencies uint16[n_entries].  They are copied to HBM and repacked on the
 * GPU (16-byte bucket records with the single entry of a bucket stored inline, 16-byte {kmer,node,freq}
 * entries, and for small and medium indexes an L2-resident Bloom filter / occupancy bitmap that rejects
 * most absent k-mers without an HBM access; large indexes get 32-byte buckets).  Unlike the
 * reference (no bounds checks, mapper.pyx:17) the arrays are validated: every non-empty bucket
 * must lie inside [0, n_entries) and every node inside [0, max_node_id], else KMM_ERR_INDEX.
 * Environment knobs for experiments, read here: KMM_OCC_MAX_BYTES (largest occupancy bitmap that is still
 * built; 0 forces the wide 32-byte bucket layout), KMM_WIDE_BUCKETS=0 (16-byte buckets without filter),
 * KMM_BLOOM_BYTES (Bloom filter size; 0 = per-bucket bitmap), KMM_BLOOM_MAX_ENTRIES, KMM_OCC_SHIFT.
 */
int kmm_index_create(const int32_t *hashes_to_index, const int32_t *n_kmers, uint64_t modulo,
                     const uint64_t *kmers, const int32_t *nodes, const uint16_t *frequencies,
                     int64_t n_entries, int64_t max_node_id, int device, kmm_index_t **out);
void kmm_index_destroy(kmm_index_t *idx);

/*
 * Node-count vector management (mapper.pyx:37 allocates it per call; gpu_counter.py keeps it
 * inside the counter).  kmm_bind_counts makes the handle accumulate into a caller-owned device
 * buffer of max_node_id+1 uint32 (e.g. a torch tensor that is then reduced with RCCL); the
 * buffer is NOT zeroed by the bind.  kmm_counts_device_ptr returns the current device buffer.
 */
int kmm_reset_counts(kmm_index_t *idx);
int kmm_bind_counts(kmm_index_t *idx, uint32_t *device_counts);
int kmm_counts_device_ptr(kmm_index_t *idx, uint32_t **out);
/* Copies the max_node_id+1 counts to `out` after draining the stream.  out: host memory of any kind (or device memory).  Into
 * ORDINARY (pageable) memory a vector of 64 MiB and more travels through the handle's page-locked staging ring, the
 * "host_pack_threads" threads copying the slots out: the link's rate without a page-locked destination (which costs ~50 ms
 * per GB to make — as much as a whole map phase; configs[2]'s 400 MB vector: ~10 ms instead of 30-40). */
int kmm_get_node_counts(kmm_index_t *idx, uint32_t *out);
int kmm_synchronize(kmm_index_t *idx);

/*
 * The one exchange step of the path: the sum of the per-GPU node-count vectors over RCCL / xGMI.  Replaces the
 * additive reduce of per-chunk vectors, command_line_interface.py:124-130 (shared_memory_wrapper's
 * additative_shared_array_map_reduce).  uint32 addition wraps modulo 2^32 like mapper.pyx:37,68, so the result
 * is bit-exact whatever the reduction order.  RCCL is loaded at first use (dlopen), not linked.
 *
 * One process, several GPUs (one handle per GPU, same index on each):
 *   kmm_reduce_counts(handles, n_gpus, root)  root >= 0: handles[root]'s count vector becomes the sum (the others are
 *                                             unspecified afterwards); root = -1: every vector becomes the sum.
 * One process per GPU (what bench.py and the CLI use under torchrun):
 *   kmm_comm_get_unique_id(id)                on rank 0; the caller hands the 128 bytes to the other ranks by any
 *                                             means (a file, MPI, torch.distributed's store, ...)
 *   kmm_comm_init_rank(idx, id, n_ranks, rank)  collective: every rank joins with its own handle
 *   kmm_comm_reduce_counts(idx, root)         collective, in place on the handle's (library-owned or bound) count
 *                                             vector; root as above
 *   kmm_comm_destroy(idx)                     (kmm_index_destroy does it too)
 * All of them synchronise like kmm_get_node_counts (pending per-entry hits of the radix path are flushed first,
 * deferred device-side errors are reported).
 */
#define KMM_COMM_ID_BYTES 128
int kmm_reduce_counts(kmm_index_t **per_gpu, int n_gpus, int root);
int kmm_comm_get_unique_id(uint8_t id[KMM_COMM_ID_BYTES]);
int kmm_comm_init_rank(kmm_index_t *idx, const uint8_t id[KMM_COMM_ID_BYTES], int n_ranks, int rank);
int kmm_comm_reduce_counts(kmm_index_t *idx, int root);
int kmm_comm_destroy(kmm_index_t *idx);

/*
 * kmm_map_kmers — replaces map_kmers_to_graph_index (mapper.pyx:19-72, loop :53-69) and
 * GpuCounter.count (gpu_counter.py:23-24): for each of the n packed k-mers q,
 * h = q % modulo, scan bucket h, and for every entry with kmer == q and
 * frequency <= max_index_lookup_frequency add 1 to counts[node].  If also_revcomp != 0 the
 * reverse complement of q (k bases) is looked up as well (`-r`,
 * command_line_interface.py:74,180-182).  k is only used for also_revcomp.
 */
int kmm_map_kmers(kmm_index_t *idx, const uint64_t *kmers, int64_t n,
                  int max_index_lookup_frequency, int also_revcomp, int k);

/*
 * kmm_map_reads — the fused path: replaces map_cpu's three steps
 * (command_line_interface.py:41 N->A, :42 get_kmer_hashes_from_chunk_sequence = util.py:71-75,
 * :51 map_kmers_to_graph_index) without materialising the k-mer array.
 * bases: the chunk's flat ASCII read bytes; read_offsets: int64[n_reads+1], read r is
 * bases[read_offsets[r] : read_offsets[r+1]] (read_offsets[0] must be 0; the offsets must be
 * non-decreasing, which is checked on the GPU and reported by the next synchronising call as
 * KMM_ERR_INVALID_ARG).  Every window of k
 * bases inside one read is packed first-base-lowest, 2 bits/base through `lut`
 * (uint8[256]: 0..3 = code, 0xFF = not a nucleotide, KMM_LUT_BREAK = a base no k-mer may contain;
 * NULL = A,C,G,T->0,1,2,3 case-insensitive with N->A) and looked up as in kmm_map_kmers.  A byte with lut 0xFF makes the NEXT
 * synchronising call fail with KMM_ERR_INVALID_BASE (the reference's encoder raises).
 */
int kmm_map_reads(kmm_index_t *idx, const uint8_t *bases, const int64_t *read_offsets,
                  int64_t n_reads, int k, int max_index_lookup_frequency, int also_revcomp,
                  const uint8_t *lut);
/* Same for n_reads reads of identical length read_len stored back to back (no offsets array;
 * the 150 bp short-read case of the reference's Readme.md:11-13). */
int kmm_map_reads_uniform(kmm_index_t *idx, const uint8_t *bases, int64_t n_reads,
                          int64_t read_len, int k, int max_index_lookup_frequency,
                          int also_revcomp, const uint8_t *lut);
/*
 * kmm_map_reads_qual — flat reads with their quality bytes as a second array (a bionumpy chunk's .sequence + .quality,
 * pysam / htslib records, a basecaller's output in HBM): "min_base_quality" (kmm_set_param) for callers that hold no FASTQ
 * text.  read_offsets != NULL: ragged reads as in kmm_map_reads, read_len is ignored; read_offsets == NULL: n_reads reads of
 * read_len back to back as in kmm_map_reads_uniform.  quals[p] is the quality byte of bases[p] (the same total length);
 * bases, quals and read_offsets are each host or device memory, independently.  qual_base: 33 (Phred+33 text, as in FASTQ)
 * or 0 (raw Phred, as BAM stores it); anything else KMM_ERR_INVALID_ARG.
 * With the handle's floor Q > 0 a base is masked iff the unsigned byte has quals[p] < qual_base + Q — with qual_base 33 a
 * byte below '!' is masked, as on the FASTQ routes; with qual_base 0 BAM's 0xFF ("absent") never is, at any Q.  A masked
 * base is a break exactly as a KMM_LUT_BREAK byte: no window that contains it is looked up, forward or reverse complement,
 * the windows on either side are, and kmm_get_stats' n_lookups counts the surviving windows.  A table with break entries
 * combines with it (a base is dead if either rule kills it); "quality_masked_bases" counts the bases whose byte was below
 * the floor, whether or not the table breaks them too; a byte with lut 0xFF stays KMM_ERR_INVALID_BASE at the next
 * synchronising call, whatever its quality.  quals == NULL and k = 1 are KMM_ERR_INVALID_ARG.  The host packer is never
 * used, reads of one length take the ragged front end (they do not count in "flat_uniform_batches"), and the path is
 * chosen as for any flat batch, by size and "path": an index with "radix_available" 0 is served by the direct path.
 * With Q = 0 the call IS kmm_map_reads / kmm_map_reads_uniform: quals is not read and may be NULL, the same routes and
 * counters.
 */
int kmm_map_reads_qual(kmm_index_t *idx, const uint8_t *bases, const uint8_t *quals, int qual_base,
                       const int64_t *read_offsets, int64_t n_reads, int64_t read_len, int k,
                       int max_index_lookup_frequency, int also_revcomp, const uint8_t *lut);

/*
 * kmm_map_records — maps a RAW chunk of a FASTQ (format = 4 lines per record) or two-line FASTA
 * (format = 2) file: replaces `bnp.open(reads).read_chunks(...)` + the per-chunk map
 * (command_line_interface.py:102-103,109-111 and :32-56) — record parsing happens on the GPU, the host
 * only reads (and, for .gz, inflates) bytes.  `raw` must start at the first byte of a record.  The
 * library finds the end of the last COMPLETE record inside the chunk, maps every base of the sequence
 * lines up to there exactly like kmm_map_reads, and returns in *consumed how many bytes it used (the
 * caller prepends the remaining raw[consumed:] to the next chunk; at end of file the last line must end
 * with a newline) and in *n_records the number of reads mapped.  '\r' before '\n' is tolerated.
 * A '\r' inside a sequence line that no '\n' follows is dropped and breaks the read — no window spans it, the windows on
 * either side of it are mapped — on every route (the direct path, the device-side compaction, the host packer); multi-line
 * FASTA keeps its own rule (below).
 * The call returns once the chunk is staged and scanned (so *consumed is valid and the host buffer is
 * free); the mapping kernels run asynchronously like every other map call.  Chunks of any size: beyond 2^30
 * bytes the library scans the chunk piece by piece (each piece starts at the end of the previous one's last
 * complete record).  A chunk large enough for the radix path (FASTQ: 2 x kmm_get_param("radix_min_units") bytes) is
 * first compacted on the device — only the bytes of its sequence lines survive, as 2-bit codes — and mapped as ONE
 * batch of flat reads; kmer_mapper map accumulates file chunks to such sizes.
 * A line that should start a record ('@' / '>') or the FASTQ '+' line but does not (e.g. multi-line
 * FASTA) makes the next synchronising call fail with KMM_ERR_MALFORMED.
 */
#define KMM_FORMAT_FASTA2 2
#define KMM_FORMAT_FASTQ 4
/* Multi-line FASTA (sequences wrapped over several lines; `bnp.open` reads those too): the chunk is unwrapped into
 * two-line FASTA on the GPU first.  A record is only known to be complete once the NEXT header line has been seen, so
 * *consumed stops at the start of the chunk's last header line — unless the caller ORs KMM_FORMAT_LAST_CHUNK into
 * `format` (the chunk ends the file: everything is consumed).
 *   - a line terminator ('\n', or a '\r' right before one) is dropped iff its line does not start with '>' and the byte
 *     behind it exists and is not '>': blank lines are dropped, inside a record and between two;
 *   - a header line followed by an empty line (">h\n\n") is a read of length 0 that counts in *n_records;
 *   - a header line directly followed by a header line (or by the end of the chunk), and bytes before the first '>', are
 *     errors: KMM_ERR_MALFORMED from the call, or KMM_ERR_MALFORMED / KMM_ERR_INVALID_BASE at the next synchronising call,
 *     as for two-line FASTA; a '\r' on a sequence line that no '\n' follows is KMM_ERR_MALFORMED from the call, nothing
 *     of its piece mapped (the last byte of a chunk that does not end the file is not looked at: it lies in the record
 *     that is not consumed);
 *   - at the end of the file the last line must end with a newline, as for the other formats: a final line without one is
 *     KMM_ERR_MALFORMED with KMM_FORMAT_LAST_CHUNK (the records before it are already counted);
 *   - the call cuts a chunk into pieces (of 2^30 bytes) that each end where a header line starts; only the piece that ends
 *     the chunk is told that the file ends.  A piece of full size that holds no whole record — one record exceeds a piece —
 *     is KMM_ERR_MALFORMED, with and without KMM_FORMAT_LAST_CHUNK, the message naming the piece's offset: the call never
 *     returns KMM_OK with part of a last chunk unconsumed.  The pieces before it are already counted (the rule for every
 *     error the device finds). */
#define KMM_FORMAT_FASTA 1
#define KMM_FORMAT_LAST_CHUNK 0x100
/* SAM text (SAM/BAM specification 1.4; what `samtools view`, aligners and simulators write; `bnp.open` reads it and the
 * reference maps chunk.sequence, command_line_interface.py:102,109).  Also a format of kmm_map_bgzf (BGZF .sam.gz, as htslib
 * writes it) and kmm_map_gzip.  The chunk's lines are parsed on the GPU (csrc/kmm_sam.hpp) into two-line FASTA
 * in HBM, which is then mapped like any other:
 *   - a line whose first byte is '@' is a header line, skipped wherever it appears (concatenated files), counted in
 *     "sam_header_lines";
 *   - every other line is one record with at least 11 TAB-separated fields; field 10 (SEQ) is mapped AS STORED (reverse-
 *     strand records are not flipped, as in kmm_map_bam) unless "original_strand" (kmm_set_param) is 1 — a kept record
 *     whose FLAG has 0x10 is then reverse-complemented back letter by letter, its QUAL reversed — through the same lookup
 *     table as every other entry point (lut NULL: ACGT -> 0123, N -> A): "=" and the IUPAC codes are
 *     KMM_ERR_INVALID_BASE at the next synchronising call; optional fields behind QUAL are ignored.  SEQ "*" is a read without k-mers that counts in *n_records (as l_seq = 0 in BAM);
 *   - "bam_exclude_flags" (kmm_set_param) leaves out records with FLAG & mask; "bam_include_flags", "bam_min_mapq" and
 *     kmm_set_record_regions select further (RECORD SELECTION below: FLAG, MAPQ, RNAME, POS and CIGAR, fields 2 to 6, are read
 *     on the GPU, each only while a rule needs it; a needed field that is malformed is one more KMM_ERR_MALFORMED of the list);
 *   - *consumed = the byte after the chunk's last '\n' (a record never spans a newline); '\r' before '\n' is tolerated;
 *   - refused with KMM_ERR_MALFORMED, nothing of the call mapped, the message naming the first bad line's byte offset: a
 *     record line with fewer than 10 TABs, a FLAG that is no decimal integer in [0, 65535], an empty line;
 *   - refused with KMM_ERR_INVALID_ARG while "min_base_quality" (kmm_set_param) is above 0, on every entry point that takes
 *     the format: the writer emits two-line FASTA, the QUAL column is not carried to the mapper — unless "use_record_qual"
 *     (kmm_set_param) is 1: field 11 (QUAL, Phred+33) is then written beside SEQ and the floor applied to it.  A QUAL that
 *     is not "*" and not as long as SEQ (SEQ "*": length 0) is one more KMM_ERR_MALFORMED of the list above.
 * Counters (kmm_get_param): "sam_calls", "sam_records", "sam_records_excluded", "sam_header_lines". */
#define KMM_FORMAT_SAM 8
int kmm_map_records(kmm_index_t *idx, const uint8_t *raw, int64_t n_bytes, int format, int k,
                    int max_index_lookup_frequency, int also_revcomp, const uint8_t *lut,
                    int64_t *consumed, int64_t *n_records);

/*
 * kmm_map_bgzf — reads from a BGZF-compressed FASTQ / two-line FASTA file (what bgzip / htslib write: a chain of independent
 * gzip members of at most 64 KiB of data, each with its size in the header), INFLATED ON THE GPU: replaces
 * `bnp.open("reads.fq.gz").read_chunks(...)` + the per-chunk map (command_line_interface.py:102-111; ".fa.gz, or fq.gz",
 * Readme.md:11; the igzip reader of util.py:78-101) without a host-side inflater — the compressed bytes cross PCIe (about a
 * quarter of the raw ones), one GPU thread inflates one member (thousands per chunk; stored, fixed and dynamic blocks;
 * every member's ISIZE and CRC32 checked on the device), and the raw records go to the device-side parser as in
 * kmm_map_records.  The bytes reach HBM through the handle's page-locked staging ring (eight slots of 16 MiB, filled by the
 * "host_pack_threads" threads, emptied by a copy engine); the member chain is walked in the caller's bytes meanwhile.
 * comp: n_comp compressed bytes in HOST memory (a file mapping will do) that start at a member boundary;
 * the call uses the whole members inside (at most 3.5 GiB of inflated bytes) and returns in *consumed_comp how many
 * compressed bytes that was — the caller continues there.  Records do not end where members end: the handle keeps the
 * inflated bytes behind the call's last complete record and puts them in front of the next call's (a STREAM per handle:
 * calls in file order; OR KMM_FORMAT_NEW_STREAM into `format` for the first chunk of a file, KMM_FORMAT_LAST_CHUNK for the
 * last: a final line without newline gets one, and bytes that then still form no record — or compressed bytes behind the
 * last whole member — are KMM_ERR_MALFORMED; a call that stops at its own size limit ignores the flag: the caller comes
 * back with the rest and the same flag).
 * format: KMM_FORMAT_FASTQ, KMM_FORMAT_FASTA2 or KMM_FORMAT_SAM.  A corrupt member (header, Huffman code, distance, ISIZE, CRC32) makes the
 * call fail with KMM_ERR_MALFORMED before anything of the chunk is mapped.  A plain gzip file (no member sizes: `gzip`, not
 * `bgzip`) is refused the same way — kmm_map_gzip below inflates those on the GPU.  *n_records: reads mapped by this call.
 */
#define KMM_FORMAT_NEW_STREAM 0x400
/* Optional, before a kmm_map_bgzf call whose chunk is followed in the caller's memory by more of the file (a file mapping):
 * comp_next = comp + n_comp of that call, n_next = how many more bytes the NEXT call will bring (the next call then passes
 * comp + *consumed_comp, n_comp - *consumed_comp + n_next).  The library stages and walks those bytes while this chunk's
 * members are being inflated — a chunk's 20 ms over PCIe then no longer stand in front of its 46 ms of kernel.  A hint that
 * the next call does not keep to costs nothing but the copy.  "bgzf_prestaged_calls" (read-only) counts the hints used. */
int kmm_map_bgzf_hint_next(kmm_index_t *idx, const uint8_t *comp_next, int64_t n_next);
int kmm_map_bgzf(kmm_index_t *idx, const uint8_t *comp, int64_t n_comp, int format, int k, int max_index_lookup_frequency,
                 int also_revcomp, const uint8_t *lut, int64_t *consumed_comp, int64_t *n_records);

/*
 * kmm_map_gzip — reads from a PLAIN gzip-compressed FASTQ / two-line FASTA file (what `gzip reads.fq` writes: one deflate
 * stream, or several members back to back, any header flags), INFLATED ON THE GPU and mapped like kmm_map_bgzf's output.
 * The deflate stream is cut at speculative block starts (one every ~32 KiB of compressed bytes), one GPU lane decodes each
 * piece with markers for its unknown 32 KiB of history, a start is kept only where the piece before it ended exactly
 * there, and the history is resolved afterwards (csrc/kmm_gpu_gunzip.hpp).  The same stream-per-handle contract
 * as kmm_map_bgzf: format KMM_FORMAT_FASTQ / KMM_FORMAT_FASTA2 / KMM_FORMAT_SAM, OR KMM_FORMAT_NEW_STREAM for a file's first window and
 * KMM_FORMAT_LAST_CHUNK for its last; comp lies in HOST memory (a file mapping will do) and reaches HBM through the handle's
 * staging ring; the inflated bytes behind the last complete record are carried to the next call.
 * comp may be ANY prefix of the rest of the file (at most 2 GiB of it are looked at): the call maps everything up to the
 * last deflate block boundary it could verify (at most 3.5 GiB of inflated bytes; a call stopped by that limit ignores
 * KMM_FORMAT_LAST_CHUNK) and returns that point's byte in *consumed_comp — the caller continues there (the bit offset inside
 * that byte, the last 32 KiB of output and the member's running CRC32 / ISIZE stay in the handle).  A window too short to
 * hold a whole block consumes nothing: bring a longer one.  KMM_ERR_MALFORMED, with nothing of the window mapped: a bad
 * header, Huffman code or distance, a distance before the start of the member, a CRC32 or ISIZE mismatch, a file that ends
 * inside a member (or inside a record) on KMM_FORMAT_LAST_CHUNK, bytes behind a member that are neither zeros nor a member.
 * Counters: "gzip_calls", "gzip_members", "gzip_chunks", "gzip_false_starts", "gzip_continuations", "gzip_inflated_bytes"
 * (see kmm_set_param).  The handle keeps the device memory of its symbol slots while a stream lasts and releases it at the
 * end of the stream (a KMM_FORMAT_LAST_CHUNK call that used the whole file, or an error).
 */
int kmm_map_gzip(kmm_index_t *idx, const uint8_t *comp, int64_t n_comp, int format, int k, int max_index_lookup_frequency,
                 int also_revcomp, const uint8_t *lut, int64_t *consumed_comp, int64_t *n_records);

/*
 * kmm_map_bam — reads from a BAM file (SAM/BAM specification 4.2; aligned or unaligned), INFLATED AND DECODED ON THE GPU:
 * replaces `bnp.open(args.reads)` on a .bam + the map of `chunk.sequence` (command_line_interface.py:102,109; bionumpy >= 0.2.7,
 * pinned by setup.py, opens .bam through its BAM buffer and yields every record's SEQ [UPSTREAM-UNVERIFIED: bionumpy is not
 * vendored here]).  The same stream-per-handle contract as kmm_map_bgzf: comp lies in HOST memory and starts at a member
 * boundary; flags = KMM_FORMAT_NEW_STREAM for a file's first window, KMM_FORMAT_LAST_CHUNK for its last (no format value);
 * the call uses whole members up to 3.5 GiB of inflated bytes and returns *consumed_comp; the inflated bytes behind its last
 * complete record are carried to the next call; kmm_map_bgzf_hint_next prestages BAM windows too.  On KMM_FORMAT_NEW_STREAM
 * the header is checked (magic "BAM\1") and skipped (l_text, text, n_ref, the references; it may span many members — a first
 * window that ends inside it consumes nothing and maps nothing: bring a longer one); n_ref stays in the handle.  Record
 * starts are found speculatively per 16 KiB tile and verified by a link pass (csrc/kmm_bam.hpp); each record's
 * SEQ, AS STORED (reverse-strand records are not flipped, as bionumpy does not flip them) unless "original_strand"
 * (kmm_set_param) is 1 — a kept record whose FLAG has 0x10 is then decoded in read orientation — goes through the same
 * 256-byte
 * lookup table as every other entry point (lut NULL: ACGT -> 0123, N -> A, command_line_interface.py:41): "=" and the IUPAC
 * codes are KMM_ERR_INVALID_BASE at the next synchronising call, exactly as the same letter in a FASTQ.  A record with
 * l_seq = 0 is a read without k-mers; no k-mer spans two records.  Refused with KMM_ERR_MALFORMED, with nothing of the call
 * mapped: a bad magic, a header that overruns its lengths, a record whose fields do not fit its block_size (or whose refID /
 * next_refID lie outside [-1, n_ref), or whose read_name is not NUL-terminated), a corrupt member, a file that ends inside a
 * member or a record on KMM_FORMAT_LAST_CHUNK.  The handle then takes a new stream.  Extension (default off):
 * "bam_exclude_flags" drops records with flag & mask (samtools view -F).  *n_records: records mapped by this call.
 * Counters (kmm_get_param): "bam_calls", "bam_records", "bam_records_excluded", "bam_header_bytes", "bam_false_starts",
 * "bam_continuations".  SAM text is read by kmm_map_bgzf / kmm_map_gzip / kmm_map_records (KMM_FORMAT_SAM); CRAM is not read.
 * While "min_base_quality" (kmm_set_param) is above 0 the call is refused with KMM_ERR_INVALID_ARG: the records' qual bytes
 * are not decoded, and ignoring the floor silently is not an option — unless "use_record_qual" (kmm_set_param) is 1: the
 * qual bytes (raw Phred) are then decoded beside SEQ and the floor applied to them.
 */
int kmm_map_bam(kmm_index_t *idx, const uint8_t *comp, int64_t n_comp, int flags, int k, int max_index_lookup_frequency,
                int also_revcomp, const uint8_t *lut, int64_t *consumed_comp, int64_t *n_records);

/*
 * A RANK'S SHARE of a BAM file (several processes on one file; kmer_mapper_amd/bgzf_ranges.py rank_member_range_bam).
 * KMM_FORMAT_MID_STREAM, OR-ed with KMM_FORMAT_NEW_STREAM into the flags of kmm_map_bam (anything else: KMM_ERR_INVALID_ARG):
 * the stream does not begin with the file's header.  n_ref is the caller's — kmm_set_param "bam_n_ref", >= 0, else
 * KMM_ERR_INVALID_ARG — and the first record starts "bgzf_head_skip" inflated bytes into the call's first member.  On every
 * kmm_map_bam stream "bgzf_tail_stop" cuts the last call's last member as it does for kmm_map_bgzf ("bgzf_head_skip" is passed
 * over by a stream that begins with the header).  A cut that is no record boundary is "the file ends inside a record",
 * KMM_ERR_MALFORMED with nothing of the call mapped: the net under a wrongly guessed boundary.
 *
 * kmm_bam_header — comp (host memory) starts at the file's first member: growing prefixes of its members are inflated on the
 * GPU until the header is walked.  *n_ref: its reference count; *hdr_member / *hdr_skip: where the first record lies — the
 * compressed offset of the member that holds the first byte behind the header, and that byte's offset in the member's inflated
 * bytes (a header that ends with a member: the next member that holds a byte, skip 0).  A window that ends inside the header:
 * KMM_OK with *n_ref = -1 — bring a longer one.  A bad magic or lengths no header can have, or a corrupt member:
 * KMM_ERR_MALFORMED.  Maps nothing and leaves a stream in progress on the handle alone.
 *
 * kmm_bam_find_record_start — comp (host memory) starts at a member boundary anywhere in the file.  Its whole members are
 * inflated and checked (CRC32, ISIZE), and a kernel finds the smallest inflated offset from which a chain of records HOLDS to
 * the end of those bytes: every record's fields fit its block_size and [-1, n_ref) until one runs past the end, at least one
 * record is whole, and when comp ends the file (its whole members end exactly at n_comp) the chain ends at the last byte.
 * The first true record start always holds; a position in front of it holds only if the bytes there chain on like records
 * to the window's end — kmm_map_bam's tail stop turns such a guess into an error of the share in front of it.
 * *member: the compressed offset, relative to comp, of the member that holds the offset; *skip: the offset inside it.
 * (n_comp, 0): comp ends the file and no record starts in it (empty members, or the tail of a record that began in front).
 * *member = -1 with KMM_OK: no chain holds — a record is longer than the window's bytes: bring a longer window.  A corrupt
 * member: KMM_ERR_MALFORMED.  Maps nothing and leaves a stream in progress on the handle alone.  n_ref: from kmm_bam_header.
 */
#define KMM_FORMAT_MID_STREAM 0x200
int kmm_bam_header(kmm_index_t *idx, const uint8_t *comp, int64_t n_comp, int32_t *n_ref, int64_t *hdr_member, int64_t *hdr_skip);
int kmm_bam_find_record_start(kmm_index_t *idx, const uint8_t *comp, int64_t n_comp, int32_t n_ref, int64_t *member, int64_t *skip);

/*
 * RECORD SELECTION — which SAM / BAM records are mapped, decided on the GPU inside the record the decode kernels hold (DESIGN
 * 4.15).  One rule for kmm_map_bam and KMM_FORMAT_SAM: the same records written either way give the same counts.  A record is
 * KEPT iff all of
 *   1. (FLAG & "bam_exclude_flags") == 0                         (samtools view -F)
 *   2. (FLAG & "bam_include_flags") == "bam_include_flags"       (samtools view -f; 0 .. 0xFFFF, default 0)
 *   3. MAPQ >= "bam_min_mapq"                                    (samtools view -q; 0 .. 255, default 0; numeric, 255 included)
 *   4. with a region list set (kmm_set_record_regions): the record overlaps a region on its reference, by htslib's rule.
 *      Positions are 0-based, half-open.  rec_beg = pos (SAM: POS - 1); rec_end = rec_beg + the summed lengths of the CIGAR
 *      operations M, D, N, = and X (64-bit; I, S, H and P never count; the long-CIGAR placeholder <l_seq>S<n>N counts its N) —
 *      or rec_beg + 1 when FLAG has 0x4, there is no CIGAR (BAM n_cigar_op 0, SAM "*") or the sum is 0.  Overlap: beg < rec_end
 *      && rec_beg < end.  A record without a reference (BAM refID -1, SAM RNAME "*") is kept iff keep_unplaced; one with a
 *      reference and no position (BAM pos < 0, SAM POS 0) overlaps nothing.
 * A record that is not kept is not looked at further (no SEQ / QUAL decode, no strand flip), counts in "bam_records_excluded" /
 * "sam_records_excluded" whatever the reason, and not in *n_records, "bam_records", "sam_records", "records_reversed" or
 * "records_without_qual".  With nothing set the library runs the kernels it ran before the selection existed, bit for bit.
 *
 * kmm_set_record_regions — the region list: regions[i] = reference (ref_id for kmm_map_bam, ref_name for KMM_FORMAT_SAM; give
 * both to serve both), [beg, end) 0-based half-open.  beg < 0 or end <= beg: KMM_ERR_INVALID_ARG.  n_regions == 0 clears the
 * list (keep_unplaced then has no effect: "the unplaced records alone" is no region list — the unmapped records are
 * "bam_include_flags" 4).  The library sorts the list by (reference, beg), merges overlapping and abutting
 * intervals, and keeps it in a small device buffer of the handle, where the kernels binary-search it; "record_regions"
 * (kmm_get_param, read-only) is the number of intervals after merging.  Limits: KMM_MAX_RECORD_REGIONS regions over
 * KMM_MAX_REGION_REFERENCES distinct references, names of at most KMM_MAX_REGION_NAME_BYTES bytes (not empty, not "*"); more:
 * KMM_ERR_INVALID_ARG, the list in force unchanged.  kmm_map_bam uses ref_id: a list with a negative one, or one outside
 * [0, n_ref) of the stream, is KMM_ERR_INVALID_ARG from the map call, with nothing mapped.  KMM_FORMAT_SAM uses ref_name, compared
 * with RNAME exactly and whole ("chr1" does not select "chr10"); a list with a NULL one is KMM_ERR_INVALID_ARG from the map call.
 * No @SQ header is needed.  The selection holds until changed, across streams and calls, like "bam_exclude_flags"; a record
 * carried between two calls is judged once, by the call that maps it.  Formats other than SAM / BAM are not affected.
 *
 * KMM_FORMAT_SAM reads a field only when a rule that needs it is set, of the records that passed the rules before it: MAPQ with
 * a floor above 0; RNAME with a region list, and POS and CIGAR of the records whose RNAME the list names.  A field that is read
 * and malformed — MAPQ or POS empty or not decimal, MAPQ above 255, POS above 2^31 - 1, a CIGAR that is neither "*" nor
 * ([0-9]+[MIDNSHP=X])+ or has an operation longer than 2^28 - 1 — is KMM_ERR_MALFORMED with the line's byte offset and nothing
 * of the call mapped.  With no rule set such a field stays as unnoticed as it was.
 */
#define KMM_MAX_RECORD_REGIONS 4096
#define KMM_MAX_REGION_REFERENCES 256
#define KMM_MAX_REGION_NAME_BYTES 255
typedef struct {
    const char *ref_name; /* KMM_FORMAT_SAM: the reference's name (NULL: the list serves kmm_map_bam only) */
    int32_t ref_id;       /* kmm_map_bam: its index in the file's header (negative: the list serves KMM_FORMAT_SAM only) */
    int64_t beg, end;     /* 0-based, half-open */
} kmm_region_t;
int kmm_set_record_regions(kmm_index_t *idx, const kmm_region_t *regions, int n_regions, int keep_unplaced);

/*
 * kmm_map_packed — reads the caller already holds as 2-BIT CODES (its own encoder, a .2bit-style store, the output of a
 * host-side packer): the same mapping as kmm_map_reads without the byte -> code step, and a quarter of the bytes over
 * PCIe.  This is the form the library's own host packer produces when kmm_map_reads* / kmm_map_records are handed host
 * memory ("host_pack_threads" below) — the work the reference spends its `-t` worker processes on
 * (bnp.as_encoded_array in util.py:71-72, command_line_interface.py:124-130,168).
 * codes: uint32 words, 16 codes per word, base p of the flat read stream in bits [2 (p & 15), 2 (p & 15) + 2) of word
 * p >> 4 (first base lowest; A,C,G,T = 0,1,2,3 — the packing of util.py:72-73), (n_bases + 15) / 16 words, host or device.
 * read_len > 0: n_reads reads of that length back to back (n_reads * read_len == n_bases), read_starts ignored.
 * read_len == 0: ragged reads; read_starts = bitset over the base positions, bit p & 31 of word p >> 5 set iff a read
 * starts at base p (n_bases / 32 + 1 words, host or device): no k-mer spans a set bit (util.py:72).
 * Served by the radix path at every batch size (KMM_ERR_INVALID_ARG when the index has none: "radix_available").
 */
int kmm_map_packed(kmm_index_t *idx, const uint32_t *codes, int64_t n_bases, int64_t n_reads, int64_t read_len,
                   const uint32_t *read_starts, int k, int max_index_lookup_frequency, int also_revcomp);

/*
 * kmm_host_alloc / kmm_host_free — page-locked host memory (hipHostMalloc) for the caller's read buffers: the
 * staging copy of a map call then runs at the PCIe link's rate (~50 GB/s) instead of the pageable path's.  The
 * reference keeps its chunks in POSIX shared memory (command_line_interface.py:110); this is the GPU counterpart.
 */
int kmm_host_alloc(size_t bytes, void **out);
int kmm_host_free(void *p);
/* Prepares the page-locked staging buffers the library needs for host-resident batches of raw_batch_bytes raw bytes
 * ("host_pack_threads": the packed stream + the read-start bitset) and shelves them for the next handle that asks.  A
 * page-locked allocation costs ~50 ms per GB: a caller that knows its batch size calls this from another thread while
 * the index is created (kmer_mapper map does), and the first map call finds the buffers ready.  Optional. */
int kmm_host_reserve(int64_t raw_batch_bytes);
/* The same for ONE page-locked buffer of `bytes` bytes, for callers that know what the next handle will ask for. */
int kmm_host_reserve_buffer(int64_t bytes);

/*
 * kmm_extract_kmers — replaces get_kmer_hashes_from_chunk_sequence (util.py:71-75) as an
 * operator: writes the packed k-mers of all reads, flattened in (read, offset) order, to `out`
 * (host or device, n_out = sum(max(len_r-k+1,0)) uint64).  Not used by the fused path.
 */
int kmm_extract_kmers(int device, const uint8_t *bases, const int64_t *read_offsets,
                      int64_t n_reads, int k, const uint8_t *lut, uint64_t *out, int64_t n_out);

/*
 * kmm_in_index — replaces in_graph_index / in_graph_index_no_memory_maps
 * (mapper.pyx:81-130,137-190): out[i] = 1 iff some entry of bucket kmers[i] % modulo equals
 * kmers[i] (no frequency filter).  out: uint8[n], host or device.
 */
int kmm_in_index(kmm_index_t *idx, const uint64_t *kmers, int64_t n, uint8_t *out);

/*
 * kmm_read_hits — per read, how many of its k-mers are in the index.  A fused kernel: read bytes -> k-mers
 * -> one gather per k-mer -> per-read sums; no k-mer is written to memory.
 * Reads as in kmm_map_reads_qual: read_offsets != NULL: ragged reads (int64[n_reads + 1], read_offsets[0] == 0,
 * non-decreasing), read_len ignored; read_offsets == NULL: n_reads reads of read_len bytes back to back.  bases and
 * read_offsets may each be host or device memory.  lut as everywhere (NULL: the reference's table; KMM_LUT_BREAK entries
 * are breaks; k == 1 with a break table is KMM_ERR_INVALID_ARG).
 *   - hits[r]: the number of windows of read r that are hits.  A window with k-mer q is a hit iff some entry l of bucket
 *     q % modulo has kmers[l] == q and frequencies[l] <= max_index_lookup_frequency; with also_revcomp, iff that holds for
 *     q or for the reverse complement of q.  A window counts once, however many entries or orientations match (a k-mer
 *     under five nodes, a palindrome: one hit).  With max_index_lookup_frequency >= 65535 and also_revcomp == 0, hits[r] is
 *     the sum of kmm_in_index over the read's k-mers.
 *   - windows[r] (windows may be NULL): the number of windows of read r that were looked up: max(len_r - k + 1, 0) minus
 *     the windows that contain a break byte.  hits[r] <= windows[r].
 *   - both are uint32[n_reads], host or device, written in full (a read without windows gets 0); counts wrap modulo 2^32.
 * A pure query: node counts, per-k-mer counts, kmm_get_stats, the handle's stream state (BGZF, gzip, BAM carry) and any
 * sticky error are left as they were.  Synchronous like kmm_in_index: runs on the handle's stream and returns when the
 * outputs are complete.  Served by the direct view on every index ("radix_available" 0 included); "read_hits_calls"
 * (kmm_get_param, read-only) counts the calls.
 * Errors come from the call itself and are never left on the handle: a byte with table entry 0xFF is
 * KMM_ERR_INVALID_BASE, the message naming its flat position; decreasing offsets, read_offsets[0] != 0, hits == NULL with
 * n_reads > 0 and k out of range are KMM_ERR_INVALID_ARG.  After an error the outputs are unspecified.  n_reads == 0 or no
 * bases at all is KMM_OK, the outputs zeroed where they exist.
 */
int kmm_read_hits(kmm_index_t *idx, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len,
                  int k, int max_index_lookup_frequency, int also_revcomp, const uint8_t *lut, uint32_t *hits,
                  uint32_t *windows);

/*
 * kmm_read_nodes — per read, the node that most of its k-mers map to.  Fused from read bytes to the answer:
 * one walk of kmm_read_hits's kernel counts the votes of every read, a second adds each vote to the (read, node) cell of a
 * hash table in device memory, and the cells are reduced to the per-read outputs.  No k-mer is written to memory.
 * Reads (read_offsets / n_reads / read_len), bases, lut, host-or-device pointers, errors and synchronisation are exactly
 * those of kmm_read_hits: ragged or uniform reads, KMM_LUT_BREAK entries are breaks, k == 1 with a break table is
 * KMM_ERR_INVALID_ARG.
 * Votes: votes[r][v] is what kmm_map_reads with the same k, max_index_lookup_frequency, also_revcomp and lut adds to
 * node_counts[v] when it is given read r alone: one vote per entry l of bucket q % modulo with kmers[l] == q and
 * frequencies[l] <= max_index_lookup_frequency (a k-mer under three nodes gives each node one vote; the filter applies
 * per entry); with also_revcomp the same again for the reverse complement of q (a palindrome in the index votes twice, as
 * map counts it twice); windows over a break give nothing.
 * Outputs, each an array of n_reads entries in host or device memory (independently), written in full; all but best_node
 * may be NULL:
 *   - best_node[r] (int32): the node with the most votes, the smallest node id among equals, -1 when the read has no vote;
 *   - best_votes[r]: that node's votes (0 with -1);
 *   - second_votes[r]: the largest vote count among the other nodes, 0 if there is none (best_votes - second_votes is the
 *     margin; 0: a tie);
 *   - total_votes[r]: the sum over all nodes;
 *   - n_nodes[r]: the number of distinct nodes with at least one vote.
 * Counts are taken modulo 2^32.  The outputs do not depend on the order the GPU's threads ran in: the same call gives the
 * same bytes.
 * Rounds: the reads are served in rounds of whole reads (at least one), cut so that the votes of a round fit a table of
 * table_bytes: 16 bytes per slot, two slots per vote.  table_bytes == 0: 4 GiB; values below 64 KiB count as 64 KiB; negative:
 * KMM_ERR_INVALID_ARG.  The table is allocated at the size the round needs, never at the target; a single read whose
 * votes need more than the target gets the table it needs (at most 2^31 - 1 votes: beyond, KMM_ERR_INVALID_ARG).  A table of
 * up to 256 MiB stays with the handle for the next call; a larger one is freed when the call returns.  *n_rounds (may be
 * NULL): the rounds the reads were cut into (0 when there was nothing to look up); rounds whose reads have no vote launch
 * nothing and are counted all the same.  The answer does not depend on the rounds.
 * A pure query like kmm_read_hits: node counts, per-k-mer counts, kmm_get_stats, the record-hits and keep queues, the
 * compressed readers' stream state, every counter of kmm_get_param and any sticky error are left as they were.  Served by
 * the direct view on every index ("radix_available" 0 included).
 * Errors come from the call itself and are never left on the handle: a byte with table entry 0xFF is
 * KMM_ERR_INVALID_BASE, the message naming its flat position; decreasing offsets, read_offsets[0] != 0, best_node == NULL
 * with n_reads > 0, k out of range and negative table_bytes are KMM_ERR_INVALID_ARG.  After an error the outputs are
 * unspecified.  n_reads == 0 or no bases at all is KMM_OK, the outputs that exist filled with -1 (best_node) and 0.
 */
int kmm_read_nodes(kmm_index_t *idx, const uint8_t *bases, const int64_t *read_offsets, int64_t n_reads, int64_t read_len,
                   int k, int max_index_lookup_frequency, int also_revcomp, const uint8_t *lut, int64_t table_bytes,
                   int32_t *best_node, uint32_t *best_votes, uint32_t *second_votes, uint32_t *total_votes,
                   uint32_t *n_nodes, int64_t *n_rounds);

/*
 * The record-hits mode: kmm_read_hits for reads that are still records.  kmm_set_param(idx, "record_hits", v):
 * 0 off (default), 1 hits, 2 hits and windows; any other value is KMM_ERR_INVALID_ARG; kmm_get_param returns it.  While the mode
 * is on:
 *   - kmm_map_records (FASTQ, two-line and multi-line FASTA, SAM), kmm_map_bgzf, kmm_map_gzip and kmm_map_bam keep parsing as
 *     they do: the carry between stream calls, *consumed, *n_records, the record counters, record selection,
 *     "original_strand", break tables and the error rules (device-found errors deferred and sticky, a KMM_ERR_MALFORMED call
 *     maps nothing) are unchanged.  They no longer touch the node counts, the per-k-mer counts or kmm_get_stats.  Instead every
 *     record that counts in *n_records appends one entry to a queue of the handle, in stream order: the sum of *n_records over
 *     the calls is the number of entries appended.  A record that selection drops gets no entry; SEQ "*", l_seq = 0 and an empty
 *     sequence line give an entry of 0 / 0; a call that fails appends nothing.
 *   - hits and windows of an entry mean what they mean in kmm_read_hits: a window counts once whatever entries or orientations
 *     match, max_index_lookup_frequency applies as given, with also_revcomp a hit is the OR over both orientations, break bytes
 *     remove windows, hits <= windows.
 *   - the calls take the direct records front end and the direct index view at every chunk size — never the radix path, never
 *     the host packer — so an index with "radix_available" 0 is served.
 *   - a record call with "min_base_quality" > 0 is KMM_ERR_INVALID_ARG, nothing mapped: that mask lives in the compaction
 *     and the radix front end; the mode has a floor of its own, "record_hits_min_base_quality" (below).  kmm_map_reads, kmm_map_reads_uniform,
 *     kmm_map_reads_qual, kmm_map_packed and kmm_map_kmers are KMM_ERR_INVALID_ARG too: flat reads have kmm_read_hits.
 * With the mode off every call runs exactly what it runs without this feature; entries still pending stay takeable.
 * The queue is device memory of the library and grows as needed (before the probe kernel is launched; pending entries are kept).
 * "record_hits_pending" (read-only) is the number of entries waiting, "record_hits_pending_mode" (read-only) the last non-zero
 * mode, in which they were appended; kmm_reset_counts empties the queue.  Switching between
 * modes 1 and 2 while entries are pending is KMM_ERR_INVALID_ARG (the pending entries have no windows, or have them).
 *
 * kmm_take_record_hits synchronises like kmm_get_node_counts — a sticky or deferred device error is returned and nothing is
 * taken — then copies the oldest min(capacity, pending) entries to hits, and to windows when that is non-NULL (entries
 * appended in mode 2 only: windows non-NULL otherwise is KMM_ERR_INVALID_ARG).  hits and windows are uint32 arrays in host or
 * device memory, independently.  *n_taken: the entries copied; they leave the queue, the rest keep their order.
 *
 * THE FLOOR OF THE MODE.  "record_hits_min_base_quality" Q, 0 .. 93, default 0 (anything else
 * KMM_ERR_INVALID_ARG; kmm_set_param / kmm_get_param): the base-quality floor of the record calls WHILE "record_hits" IS 1 OR 2.
 * No other call reads it; "min_base_quality" keeps its meaning for the node-count routes and stays refused with the mode on,
 * which is why the mode's floor is a parameter of its own.  With Q = 0 every call launches exactly what it launches without
 * the parameter.  With Q > 0:
 *   - FASTQ text (kmm_map_records, kmm_map_bgzf, kmm_map_gzip, kmm_map_record_pairs; interleaved "record_pairs" included): byte i
 *     of a record's quality line belongs to byte i of its sequence line, counted from the line starts.  A sequence base whose
 *     quality byte, taken as unsigned, is < 33 + Q is a break exactly as a KMM_LUT_BREAK byte: no window that contains it is
 *     looked up in either orientation, the windows on either side are, and it counts in neither hits nor windows.  A byte below
 *     '!' is masked, a byte >= 0x80 is not.  *n_records does not change and the queue keeps one entry per record.  A break table
 *     combines with the floor (a base is dead if either rule kills it); a 0xFF table entry stays KMM_ERR_INVALID_BASE whatever
 *     the quality.  A record whose quality line is not as long as its sequence line (the bytes in front of the '\n', without the
 *     '\r' of a CRLF end) is KMM_ERR_MALFORMED, deferred and sticky as with "min_base_quality"; the message names the raw offset
 *     of the quality line's '\n' in its piece.
 *   - THE KEPT TEXT IS NEVER ALTERED: the keep queue, kmm_take_kept_bgzf, both mate queues and the raw BAM form hold exactly the
 *     bytes they hold without a floor; only which records pass the rule changes.
 *   - two-line and multi-line FASTA have no qualities: the calls are served and the floor has no effect.
 *   - kmm_map_bam (plain hits, "record_names" with and without "record_names_pairs", "record_bam", "record_bam_mates") and
 *     KMM_FORMAT_SAM in the hits mode without keep need "use_record_qual" 1, else KMM_ERR_INVALID_ARG with nothing mapped.  The
 *     decode's quality variants hand four-line FASTQ to the records call; QUAL is reversed under "original_strand".  A record
 *     that stores no qualities (BAM: first byte 0xFF; SAM: "*") passes UNMASKED and counts in "records_without_qual", in every
 *     form — in the named form its text still shows '"' for every base: the decode tells the mark pass which records are exempt.
 *   - "record_sam" 1 / 2 with Q > 0 is KMM_ERR_INVALID_ARG, nothing mapped (that form's decode reads no QUAL); so is k = 1.
 *   - "quality_masked_bases" counts the masked sequence bases of the records that count in *n_records.
 *   - an index with "radix_available" 0 is served; Q may change while entries are pending (an entry keeps its call's floor).
 * With timing on, the line-start and mark kernels in front of the hit kernel are timed as KMM_KERNEL_RH_QUAL_MARK.  Out of
 * scope: a floor for flat kmm_read_hits, "record_sam", the host packer.
 */
int kmm_take_record_hits(kmm_index_t *idx, uint32_t *hits, uint32_t *windows, int64_t capacity, int64_t *n_taken);

/*
 * The record-keep mode: the reads that the record-hits mode counted, written back out.  It extends that mode:
 * with "record_keep" 0 (default) every call runs the kernels it runs without this feature.  kmm_set_param / kmm_get_param:
 *   "record_keep"               0 / 1 (anything else KMM_ERR_INVALID_ARG): the record calls also append the TEXT of every kept
 *                               record to a byte queue of the handle
 *   "record_keep_min_hits"      0 .. 2^32 - 1, default 1
 *   "record_keep_min_permille"  0 .. 1000, default 0
 *   "record_keep_invert"        0 / 1, default 0
 *   "record_keep_pending_bytes", "record_keep_pending_records"  read-only; they synchronise like "quality_masked_bases"
 * The keep rule of a record with entry (hits, windows), in 64-bit arithmetic:
 *   match = hits >= min_hits && 1000 * hits >= min_permille * windows;   keep = match != invert
 * so a record without windows matches iff min_hits is 0.
 * Refused with KMM_ERR_INVALID_ARG, nothing mapped and nothing appended to either queue, while "record_keep" is 1:
 *   - a record call with "record_hits" 0 (the rule reads that mode's entries);
 *   - a record call with "record_keep_min_permille" > 0 and "record_hits" 1 (the rule needs windows, which mode 2 keeps);
 *   - kmm_map_bam with "record_names" 0, and KMM_FORMAT_SAM on every entry point that takes it whatever "record_names" says:
 *     their records are decoded to ">\n" SEQ on the device and the read's name (QNAME) is not carried, so the text would be
 *     useless.  kmm_map_bam with "record_names" 1 carries it (below); SAM text is out of scope;
 *   - whatever the record-hits mode refuses ("min_base_quality" > 0, the flat-read calls).
 * Appended by kmm_map_records (KMM_FORMAT_FASTQ, KMM_FORMAT_FASTA2, KMM_FORMAT_FASTA), kmm_map_bgzf, kmm_map_gzip and, with
 * "record_names" 1, kmm_map_bam (the records' named FASTQ text: THE NAMED FORM below): exactly
 * the records that count in *n_records, each at most once (a record carried between two stream calls is judged by the call that
 * maps it), in stream order, contiguously, nothing between them.
 *   - FASTQ and two-line FASTA: the record's bytes as the parser sees them, from the first byte of its header line through the
 *     '\n' that ends its last line; header, '+' line, qualities and '\r' untouched.  For kmm_map_records on well-formed input
 *     these are the caller's bytes verbatim.
 *   - the stream routes: the inflated bytes; a final line without a newline has got one on KMM_FORMAT_LAST_CHUNK.
 *   - multi-line FASTA: the record as UNWRAPPED two-line text (header line, then the sequence on one line), which is what the
 *     device-side unwrap hands to the parser — not the caller's line breaks.
 * The hits queue is unaffected: one entry per record, kept or not, so the keep rule over the taken entries names exactly the
 * kept records.  A call that fails appends nothing to either queue (pieces before a failing piece included).  Node counts,
 * per-k-mer counts, kmm_get_stats and the compressed streams' carry stay as in the record-hits mode.
 * The queue is device memory of the library; it grows before a piece's kernels are launched (pending bytes are kept), and its
 * tail lives on the device, so a map call gains no host round trip.  Changing the rule or "record_keep" while bytes are pending
 * is allowed: they stay takeable.  kmm_reset_counts empties the queue.
 *
 * THE NAMED FORM of the BAM decode.  "record_names" 0 / 1 (default 0; anything else KMM_ERR_INVALID_ARG): while it
 * is 1 and "record_hits" is 1 or 2, kmm_map_bam decodes every record that passes the selection (exclude / include flags, MAPQ
 * floor, regions) into four-line FASTQ that carries the read's name and qualities, and hands that text to the records front
 * end as KMM_FORMAT_FASTQ — one (hits, windows) entry per record as in the record-hits mode, and with "record_keep" 1 the text of
 * the kept records goes to the byte queue:
 *     '@' NAME [ "/1" | "/2" ] '\n'  SEQ '\n'  "+\n"  QUAL '\n'           (l_read_name - 1) + suffix + 2 * l_seq + 6 bytes
 *   NAME   the l_read_name - 1 bytes in front of the terminating NUL; every byte outside 0x21 .. 0x7E is written as '?' (a NUL in
 *          the middle, a tab or a newline of a damaged file cannot break a line).  Read-only "record_name_bytes_replaced": the
 *          bytes so replaced since the statistics were last reset (kmm_get_stats(reset)) or kmm_reset_counts emptied the queue;
 *          synchronises like "quality_masked_bases"
 *   suffix only with "record_names_mate_suffix" 1 (0 / 1, default 0): "/1" iff FLAG has 0x40 and not 0x80, "/2" iff 0x80 and not
 *          0x40, else nothing — the rule of `samtools fastq` without -n
 *   SEQ    the letters =ACMGRSVTWYHKDBN as stored; with "original_strand" 1 a record with FLAG 0x10 and at least one base is
 *          written in read orientation (SEQ complemented and reversed, QUAL reversed) and counted in "records_reversed"
 *   QUAL   Phred + 33, clipped at '~'; a record whose qualities are absent (first byte 0xFF) gets '"' (0x22) for every base, the
 *          default of `samtools fastq -v 1`, and is counted in "records_without_qual"
 * A record without bases gives "@NAME\n\n+\n\n".  With "record_names" 0 every call launches the kernels it launched without the
 * parameter.  Refused with KMM_ERR_INVALID_ARG, nothing mapped: kmm_map_bam with "record_names" 1 and "record_hits" 0.  The
 * parameter is not read by any other call: the FASTA / FASTQ routes are unaffected, KMM_FORMAT_SAM with "record_keep" 1 stays
 * refused, and so does "min_base_quality" in the record-hits mode (its own floor, "record_hits_min_base_quality", is served).
 *
 * kmm_take_kept_records synchronises like kmm_take_record_hits — a sticky or deferred device error is returned and nothing is
 * taken.  If capacity is at least the pending bytes, ALL of them are copied to out (host or device memory), *n_bytes and
 * *n_records are set and the queue is emptied; otherwise KMM_ERR_INVALID_ARG, the message names the bytes needed, and nothing is
 * taken: whole queue or nothing, records are never split.  out == NULL with capacity 0 on an empty queue is KMM_OK with zeros.
 */
int kmm_take_kept_records(kmm_index_t *idx, uint8_t *out, int64_t capacity, int64_t *n_bytes, int64_t *n_records);

/*
 * KEEPING MATES TOGETHER.  The keep rule above sees one record; paired-end reads need both mates kept or both
 * dropped.  Per mate, match = hits >= min_hits && 1000 * hits >= min_permille * windows (the rule without its inversion), and
 *   pair_match = "record_pairs_rule" 0 (any, default): match1 || match2;  1 (both): match1 && match2
 *   keep       = pair_match != "record_keep_invert", for both mates alike.
 *
 * INTERLEAVED INPUT: "record_pairs" 0 (default) / 1 (anything else, and any "record_pairs_rule" but 0 / 1, is
 * KMM_ERR_INVALID_ARG).  With 1, and only while "record_keep" is 1 (with "record_keep" 0 neither parameter changes anything),
 * records 2i and 2i + 1 of a stream are mates: kmm_map_records with KMM_FORMAT_FASTQ / KMM_FORMAT_FASTA2, kmm_map_bgzf and
 * kmm_map_gzip take whole pairs only — *n_records is even and *consumed ends a pair, for every piece of a chunk beyond the piece
 * limit as well — and a complete record behind the last whole pair stays unconsumed like an incomplete one: on the stream routes
 * the KMM_FORMAT_LAST_CHUNK call is then KMM_ERR_MALFORMED ("ends with an unpaired record") and appends nothing.  The hits queue
 * is as without pairs: one entry per record, in order.  Refused with KMM_ERR_INVALID_ARG while "record_keep" and "record_pairs"
 * are both 1, nothing mapped, nothing appended: KMM_FORMAT_FASTA (multi-line), KMM_FORMAT_SAM, and kmm_map_bam with or without
 * "record_names".  Changing "record_pairs" while hit entries are pending is refused, like a change of the record-hits mode.
 *
 * TWO BUFFERS: kmm_map_record_pairs maps record i of raw1 and record i of raw2 as mates, by position (names are not compared).
 * format is KMM_FORMAT_FASTQ or KMM_FORMAT_FASTA2, the same for both; each buffer lies in host or in device memory,
 * independently.  The call needs "record_hits" 1 or 2 and "record_keep" 1 (else KMM_ERR_INVALID_ARG); "record_pairs" is not
 * read.  Only whole pairs are taken: m = min(whole records of raw1, of raw2) per piece pair ("debug_records_piece_kb" applies to
 * both buffers), *n_pairs is their sum, *consumed1 / *consumed2 the bytes used of each buffer — the byte behind its last taken
 * record.  The hits queue gains 2 * *n_pairs entries in pair order (entry 2i mate 1, entry 2i + 1 mate 2: what the interleaved
 * file would have appended); the kept mate-1 text goes to the queue of kmm_take_kept_records, the kept mate-2 text to a second
 * queue of the handle.  A failing call restores the hits queue and both text queues; kmm_reset_counts empties both.  After any
 * successful sequence of calls the two text queues of a handle that is fed through this call alone hold equally many records.
 *
 * kmm_take_kept_mates: mate 0 is kmm_take_kept_records, mate 1 the same contract on the second queue, anything else
 * KMM_ERR_INVALID_ARG.  Read-only "record_keep_pending_bytes_mate2", "record_keep_pending_records_mate2".
 *
 * THE MATES OF A BAM STREAM: "record_names_pairs" 0 (default) / 1 (anything else KMM_ERR_INVALID_ARG), read by
 * kmm_map_bam alone.  With 1 — and "record_names" 1, "record_hits" 1 or 2, "record_keep" 1 — the SELECTED records of a stream, in
 * file order, are mates: kept records 2p and 2p + 1 are pair p, as in a file grouped by name (unaligned BAM, an aligner's unsorted
 * output, `samtools collate`).  The keep rule is the pair rule above over their two entries ("record_pairs_rule",
 * "record_keep_invert" as there); the hits queue gains one entry per record in pair order, the first of a call at an even index;
 * the kept text, interleaved four-line FASTQ in stored order, goes to the queue of kmm_take_kept_records / kmm_take_kept_bgzf.
 * Windows need not hold whole pairs: the text of an odd last selected record waits on the handle for its mate in the next call,
 * through windows without a selected or without a complete record; *n_records counts the records appended, an even number.
 *   THE MATE CHECK: the names of every pair are compared on the device — what the decode wrote behind '@', after the '?'
 *   replacement, equal in length and in bytes; with "record_names_mate_suffix" 1 a trailing "/1" or "/2" is left out of the
 *   comparison.  (The one edge: a QNAME that itself ends in "/1" or "/2" while FLAG carries no mate bit loses those two bytes in
 *   the comparison too — "x/1" and "x" then count as mates.)  The first pair whose names differ fails the call that decoded its
 *   second record with KMM_ERR_MALFORMED; the message names the pair's ordinal in the stream and what to do: collate the file by
 *   name and exclude secondary and supplementary records (0x900).  A coordinate-sorted file fails at its first pair of strangers.
 *   A stream whose KMM_FORMAT_LAST_CHUNK call leaves a record without its mate fails with KMM_ERR_MALFORMED ("the stream ends
 *   with an unpaired record", with the count of selected records).  A failing call leaves the hits queue, the text queues, the
 *   waiting mate, the node counts, the statistics and the decode's counters as it found them; the stream cannot be continued.
 *   kmm_reset_counts and KMM_FORMAT_NEW_STREAM drop a waiting mate.
 * Refused with KMM_ERR_INVALID_ARG, nothing mapped, nothing appended: kmm_map_bam with "record_names_pairs" 1 while "record_names"
 * or "record_keep" is 0, or together with "record_pairs" 1 (which stays refused on BAM input as above); a change of
 * "record_names_pairs" while hit entries are pending.  With 0 every call launches exactly what it launched without the parameter.
 *
 * THE RAW FORM: BAM RECORDS KEPT AS BAM RECORDS.  "record_bam" 0 (default) / 1 (anything else KMM_ERR_INVALID_ARG),
 * read by kmm_map_bam alone; the text routes and KMM_FORMAT_SAM never read it.  With 1 — and "record_hits" 1 or 2, "record_keep" 1 —
 * the selected records of a call are decoded in the two-line FASTA form ("original_strand" honoured, as in the record-hits mode
 * without the switch) and mapped; the hits queue gains one entry per selected record in file order, exactly the entries the
 * record-hits mode appends with the switch off.  Behind that, every selected record whose entry passes the keep rule
 * ("record_keep_min_hits", "record_keep_min_permille", "record_keep_invert") is appended to the queue of kmm_take_kept_records /
 * kmm_take_kept_bgzf AS IT STANDS IN THE FILE: its block_size word and the block_size bytes behind it, untouched — RNAME, POS, MAPQ,
 * CIGAR, the mate fields and every aux tag included — in file order.  "record_keep_pending_records" counts records as it does for
 * text.  The queue's tail stays on the device; the call makes no host round trip beyond those of the record-hits mode.
 * *n_records, "bam_records", "bam_records_excluded", the carry between windows, the node counts and kmm_get_stats behave as in the
 * record-hits mode.  A failing call (a malformed record behind good ones, a failure of the inner records call) appends nothing
 * to either queue.  A kept record that spans many 16 KiB tiles (a long read) is copied by one wavefront.
 *   The bytes taken are headerless: a BAM file is kmm_bam_stream_header's bytes and the taken bytes, BGZF-compressed, and the
 *   28-byte end-of-file member.  kmm_bam_stream_header(idx, out, capacity, n_bytes): the header of the last stream started on the
 *   handle with KMM_FORMAT_NEW_STREAM, from the magic through the last reference, copied to out (host memory); *n_bytes its
 *   length.  capacity below it: KMM_ERR_INVALID_ARG, the message and *n_bytes name the size.  No stream started, a first window
 *   that ended inside the header, or a KMM_FORMAT_MID_STREAM share: KMM_ERR_INVALID_ARG.  (kmm_bam_header, DESIGN 4.14, is the
 *   other call: it finds where the header of a file ENDS, for a rank's share.)
 * Refused with KMM_ERR_INVALID_ARG, nothing mapped, nothing appended: kmm_map_bam with "record_bam" 1 while "record_hits" or
 * "record_keep" is 0; with "record_names" 1 (one output form per queue); with "record_names_pairs" 1 or "record_pairs" 1; with
 * KMM_FORMAT_MID_STREAM; a change of "record_bam" while "record_keep_pending_bytes" > 0 (text and raw records never share a
 * queue).  With 0 every call launches exactly what it launched without the parameter.  With timing on the kernels of the raw
 * form are timed together as KMM_KERNEL_BAM_RAW.  Out of scope: a rank's share, SAM text in or out, @PG lines and .bai / .csi
 * indices, uncompressed BAM, edited records.  (Mates kept together: "record_bam_mates", below.)
 *
 * MATES KEPT TOGETHER IN THE RAW FORM.  "record_bam_mates" 0 (default) / 1 (anything else KMM_ERR_INVALID_ARG), read
 * by kmm_map_bam alone; it applies with "record_bam" 1, "record_hits" 1 or 2 and "record_keep" 1.  The selected records of the
 * stream, in file order from KMM_FORMAT_NEW_STREAM, are mates: 2p and 2p + 1.  The keep decision is the pair rule of DESIGN 4.21
 * over the two records' entries (the keep rule's parameters and "record_pairs_rule"; "original_strand" is honoured for the hits).
 * For every kept pair the raw bytes of both records (4 + block_size each, untouched) are appended to the queue of
 * kmm_take_kept_records / kmm_take_kept_bgzf in file order, mate 1 directly in front of mate 2; records that are not selected and
 * lie between two mates are dropped like any record that is not selected.  "record_keep_pending_records" counts records, two per
 * kept pair.  The hits queue gets one entry per record in pair order, whole pairs per call: windows need not hold whole pairs —
 * the entry and the raw bytes of an odd last selected record wait on the handle for the call that brings its mate, through windows
 * without a selected or a complete record; *n_records counts the entries appended, an even number.  One small read-back per window.
 *   THE MATE CHECK: the read_name bytes of records 2p and 2p + 1 are compared on the device as they stand — equal l_read_name and
 *   equal bytes, nothing trimmed.  The first pair of strangers fails the call that completes it with KMM_ERR_MALFORMED; the message
 *   names the pair's ordinal in the stream and what to do: collate the file by name, exclude 0x900.  A KMM_FORMAT_LAST_CHUNK call
 *   that leaves a mate 1 alone — also one that brings no member — fails with KMM_ERR_MALFORMED ("the stream ends with an unpaired
 *   record", with the count of selected records).  Strangers come before an unpaired end.  A failing call appends nothing to either
 *   queue, restores the pair ordinal, the BAM counters of the call and the decode's device counters and leaves the waiting mate as
 *   it found it: a later call that brings its mate completes the pair.  (The bytes of an incomplete record that the stream carried
 *   are dropped by a failed call that brought members, as on every route: the next call begins at a record start.)
 *   kmm_reset_counts, KMM_FORMAT_NEW_STREAM and a change of "record_bam" or "record_bam_mates" drop a waiting mate.
 * Refused with KMM_ERR_INVALID_ARG, nothing mapped: everything "record_bam" refuses, in its wording and first; kmm_map_bam with
 * "record_bam_mates" 1 and "record_bam" 0; a change of "record_bam_mates" while hit entries or kept bytes are pending.  With 0
 * every call launches exactly what it launched without the parameter.  With timing on the kernels are timed together as
 * KMM_KERNEL_BAM_RAW_MATES.  Out of scope: coordinate-sorted input (the check reports it), singletons diverted, a rank's share,
 * a requirement that FLAG has 0x1, 0x40 or 0x80.
 *
 * SAM LINES KEPT AS SAM LINES.  "record_sam" 0 (default) / 1 / 2 (anything else KMM_ERR_INVALID_ARG), read by
 * KMM_FORMAT_SAM calls alone: kmm_map_records, and kmm_map_bgzf / kmm_map_gzip on their inflated bytes; FASTQ, FASTA and BAM calls
 * never read it.  With 1 or 2 — and "record_hits" 1 or 2, "record_keep" 1 — the call's selected records are decoded to two-line
 * FASTA and mapped as in the record-hits mode ("original_strand" honoured for the hits); the hits queue gains one entry per
 * selected record in file order and none of the FASTA text is appended.  Behind that, every selected record whose entry passes
 * the keep rule is appended to the queue of kmm_take_kept_records / kmm_take_kept_bgzf as its WHOLE LINE, from its first byte
 * through its newline, untouched — a '\r' before the newline, lower-case SEQ and every tag come out as they went in — in file
 * order.  With 1 every header line ('@' first) is appended too, verbatim, at its place in the stream; 2 drops the header lines
 * (`samtools view` without -h: shares that are concatenated).  Records excluded by "bam_exclude_flags" or by the selection are not
 * written.  "record_keep_pending_records" counts records, not header lines.  The one byte that is not input is the newline that
 * KMM_FORMAT_LAST_CHUNK supplies for a final unterminated line on the stream routes.  "sam_records", "sam_records_excluded",
 * "sam_header_lines", *consumed, *n_records, the node counts and kmm_get_stats are what the record-hits mode reports.  The queue's
 * tail stays on the device; the call makes no host round trip beyond those of the record-hits mode, and no walk over the lines
 * beyond the count and one write.  A failing call (a malformed line anywhere in the chunk, a failure of the inner call or behind
 * it) appends nothing to either queue.
 * Refused with KMM_ERR_INVALID_ARG, nothing mapped, nothing appended: a SAM call with "record_sam" non-zero while "record_hits" or
 * "record_keep" is 0, or with "record_pairs" 1; a change of "record_sam" while "record_keep_pending_bytes" > 0 (raw lines and text
 * never share a queue).  With 0 every call launches exactly what it launched without the parameter, and SAM stays refused in the
 * keep mode with its text.  With timing on the kernels of the keep step are timed together as KMM_KERNEL_SAM_RAW.  Out of scope:
 * mates kept together, SAM to FASTQ with names, SAM in with BAM out (or BAM in with SAM out), a rank's share, an @PG line, a
 * quality floor (the record-hits mode refuses one).  (Mates kept together: "record_sam_mates", below.)
 *
 * SAM MATES KEPT TOGETHER.  "record_sam_mates" 0 (default) / 1 (anything else, or 1 while "record_sam" is 0,
 * KMM_ERR_INVALID_ARG), read by KMM_FORMAT_SAM calls alone — kmm_map_records, and kmm_map_bgzf / kmm_map_gzip on their inflated
 * bytes — and only while "record_sam" is 1 or 2, "record_hits" 1 or 2 and "record_keep" 1.  The selected records of the stream (what
 * passes "bam_exclude_flags" and the selection), in file order, are mates: 2p and 2p + 1, as bwa mem, minimap2 -a and bowtie2 write
 * them once 0x900 is excluded.  The stream runs from KMM_FORMAT_NEW_STREAM on the stream routes; on kmm_map_records from the moment
 * the parameter is set, or from kmm_reset_counts.  Header lines and lines that are not selected never take part in the pairing.
 * The keep decision is the pair rule of DESIGN 4.21 over the two records' entries (the keep rule's parameters and
 * "record_pairs_rule"): both mates are kept or both are dropped.  Both lines of a kept pair are appended as they stand, newlines
 * included, mate 1 directly in front of mate 2, where mate 2 stands in the file; with "record_sam" 1 every header line is appended
 * once, at its place relative to the pairs — a header line between the two mates of a pair comes out in front of the pair.  Lines
 * that are not selected and lie between two mates are dropped like any others.  The kept bytes are a function of the text and the
 * rules alone, however the text is cut into pieces, chunks or windows.  "record_keep_pending_records" counts records, two per kept
 * pair.  The hits queue gets one entry per record in pair order, whole pairs per call, and *n_records — an even number — counts
 * them; "sam_records", "sam_records_excluded", "sam_header_lines" and *consumed are what they are without the switch.
 *   THE WAITING MATE: a selected record whose mate the call has not brought waits on the handle — its line and its FASTA text — for
 *   the piece or call that brings the mate, through pieces and windows without a selected record; its entry arrives with its
 *   mate's call.  Read-only "record_sam_mate_waiting" is 1 while one waits.  *consumed is never shortened for it.  One small
 *   read-back per piece.
 *   THE MATE CHECK: the bytes of both lines up to their first TAB are compared on the device as they stand — equal in length and
 *   content, nothing trimmed, no "/1", no case folding.  Strangers fail the call that completes the pair with KMM_ERR_MALFORMED;
 *   the message names the lowest such pair's ordinal in the stream and its records 2p and 2p + 1, says "are not mates", and what
 *   to do: group the file by name, exclude 0x900.  A KMM_FORMAT_LAST_CHUNK call that leaves a mate 1 waiting — also one that
 *   brings no byte; kmm_map_records reads the flag for SAM under this switch alone — fails with KMM_ERR_MALFORMED ("the stream ends
 *   with an unpaired record", with the count of selected records).  Strangers come first.  A failing call appends nothing to
 *   either queue, restores the pair ordinal and the SAM counters and leaves the waiting mate as it found it: a later call that
 *   brings its mate completes the pair.  kmm_reset_counts, KMM_FORMAT_NEW_STREAM and a change of "record_sam" or "record_sam_mates"
 *   drop a waiting mate.
 * Refused with KMM_ERR_INVALID_ARG: everything "record_sam" refuses, in its wording ("record_pairs" 1 and the floor of the
 * record-hits mode among it); a change of "record_sam_mates" while hit entries or kept bytes are pending.  With 0 every call
 * launches exactly what it launched without the parameter.  With timing on the kernels are timed together as
 * KMM_KERNEL_SAM_RAW_MATES, and KMM_KERNEL_SAM_RAW counts none.  Out of scope: coordinate-sorted input (the check reports it),
 * singletons diverted, a requirement that FLAG has 0x1, 0x40 or 0x80, SAM to FASTQ, SAM in with BAM out, a quality floor, several
 * ranks, an @PG line.
 */
int kmm_bam_stream_header(kmm_index_t *idx, uint8_t *out, int64_t capacity, int64_t *n_bytes);
int kmm_map_record_pairs(kmm_index_t *idx, const uint8_t *raw1, int64_t n1, const uint8_t *raw2, int64_t n2, int format, int k,
                         int max_freq, int also_revcomp, const uint8_t *lut, int64_t *consumed1, int64_t *consumed2, int64_t *n_pairs);
int kmm_take_kept_mates(kmm_index_t *idx, int mate, uint8_t *out, int64_t capacity, int64_t *n_bytes, int64_t *n_records);

/*
 * COMPRESSED OUTPUT.  Text that lies in device memory leaves it as BGZF: the input is cut every 65280 (0xFF00)
 * bytes, as bgzip cuts it, and every piece becomes one member — the 18-byte header (1f 8b 08 04, MTIME 0, XFL 0, OS ff, XLEN 6,
 * 'B' 'C' 2, BSIZE = member size - 1), one final deflate block, the CRC32 of the piece, ISIZE.  The block is dynamic Huffman
 * over LZ77 tokens, or stored whenever the dynamic form would not be smaller than the piece + 5 bytes: a member of n bytes of
 * text is never larger than n + 31 bytes.  Zero bytes give zero members; NO end-of-file block is appended — the caller writes
 * the 28-byte empty member once, at the end of a file.  The bytes are a pure function of the text: two calls, two devices and
 * the g++ build of csrc/kmm_bgzf_out.hpp give identical members.
 *
 * kmm_bgzf_bound(n): what n bytes of text can need, n + 31 * ceil(n / 65280); 0 for n == 0; -1 for n < 0.
 *
 * kmm_bgzf_compress — an operator like kmm_extract_kmers (no handle; a stream of its own): in[0, n) -> out, *n_out the bytes
 * written.  in and out may each be host or device memory.  capacity < kmm_bgzf_bound(n) is KMM_ERR_INVALID_ARG, the message
 * names the bound, and nothing is written.
 *
 * kmm_take_kept_bgzf — kmm_take_kept_mates with the queue's text compressed on the device, so that only the members cross the
 * link: mate 0 is the queue of kmm_take_kept_records, mate 1 the mate-2 queue of kmm_map_record_pairs, anything else
 * KMM_ERR_INVALID_ARG.  It synchronises first — a sticky or deferred device error is returned and nothing is taken.  capacity is
 * judged against kmm_bgzf_bound(pending bytes): if it is at least that, ALL pending text is compressed, the members are copied
 * to out (host or device memory), *n_comp is their bytes, *n_bytes the text they hold, *n_records its records, and the queue is
 * emptied; otherwise KMM_ERR_INVALID_ARG, the message names the bound, nothing is taken and the queue stays takeable by either
 * kind of take.  out == NULL with capacity 0 on an empty queue is KMM_OK with zeros.  Every take ends its last member:
 * concatenated takes are a valid BGZF stream (short last members are the price).  The plain takes are untouched; the two kinds
 * may be mixed on one handle.  With timing on the kernels are timed as KMM_KERNEL_BGZF_DEFLATE and KMM_KERNEL_BGZF_GATHER.
 */
int64_t kmm_bgzf_bound(int64_t n);
int kmm_bgzf_compress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t capacity, int64_t *n_out);
int kmm_take_kept_bgzf(kmm_index_t *idx, int mate, uint8_t *out, int64_t capacity, int64_t *n_comp, int64_t *n_bytes,
                       int64_t *n_records);

/*
 * kmm_build_index — builds the Kmer Index arrays on the GPU from flat (k-mer, node) pairs: replaces
 * graph_kmer_index's KmerIndex.from_flat_kmers(flat_kmers, modulo) (reference call site
 * tests/test_mapping.py:36-38; gpu_counter.py:16 builds its table from the same pairs).  Entries are
 * ordered by kmer % modulo, ties by original position (a stable sort, reproducible bit for bit);
 * hashes_to_index[h] = first entry of bucket h (0 for empty buckets),
 * frequencies[l] = number of entries holding the same k-mer as entry l, clipped to 65535.
 * Outputs: hashes_to_index int32[modulo], n_kmers int32[modulo], kmers_out uint64[n], nodes_out int32[n],
 * frequencies_out uint16[n]; every pointer may be host or device memory.  n, modulo < 2^31.
 */
int kmm_build_index(int device, const uint64_t *kmers, const int32_t *nodes, int64_t n, uint64_t modulo,
                    int32_t *hashes_to_index, int32_t *n_kmers, uint64_t *kmers_out, int32_t *nodes_out,
                    uint16_t *frequencies_out);

/*
 * kmm_seq_index_build — a Kmer Index from sequences: the step in front of kmm_build_index that the callers of
 * that function had to do themselves.  bases uint8 flat, seq_offsets int64[n_seqs + 1] (seq_offsets[0] == 0, non-decreasing),
 * seq_nodes int32[n_seqs], all >= 0, or NULL: the node of sequence i is i.  lut as everywhere (NULL: the reference's table, N is
 * A; 0xFF entries are KMM_ERR_INVALID_BASE; KMM_LUT_BREAK entries are breaks; k == 1 with a break table is
 * KMM_ERR_INVALID_ARG, as in kmm_read_hits).  Every pointer may be host or device memory.
 *   1. windows: all windows of k bases that lie inside one sequence and contain no break byte, in flat order; their packed
 *      k-mers are what kmm_extract_kmers gives for break-free input.
 *   2. pair list P: per window (k-mer, node of its sequence); with KMM_SEQIDX_BOTH_STRANDS directly followed by (reverse
 *      complement of the k-mer, same node).
 *   3. D: the distinct pairs of P in order of first occurrence in P.  A k-mer that occurs 10^6 times in one sequence is one
 *      entry, the same k-mer under three nodes is three entries of frequency 3, a palindrome under both strands is one.
 *   4. modulo: the caller's, or with modulo == 0 kmm_seq_index_modulo(|D|): the smallest prime >= max(2 |D| + 1, 3).  Limits as
 *      in kmm_build_index (< 2^31).
 *   5. the index: exactly what kmm_build_index(D.kmers, D.nodes, |D|, modulo) returns.
 * The five arrays are a pure function of the input: two builds give the same bytes.  |D| == 0 (no sequences, all shorter than
 * k) is KMM_OK: no entries, the two tables zeroed.  KMM_ERR_INVALID_ARG, the message naming the number: more than
 * KMM_SEQIDX_MAX_PAIRS pairs in P, decreasing offsets, seq_offsets[0] != 0, a negative node, k outside [1, KMM_MAX_K], a flag
 * bit not listed here, NULL where data is needed.  After an error *out is NULL, nothing stays allocated and the next call
 * works.  Runs on a stream of its own, like kmm_build_index, and returns when the object is complete.  Device memory while it
 * runs: about 40 bytes per pair of P beside the input.
 *
 * kmm_seq_index_info — the entries |D|, the modulo, the windows of step 1 and the pairs |P| (each pointer may be NULL).
 * kmm_seq_index_fetch — copies the five arrays out: hashes_to_index int32[modulo], n_kmers int32[modulo], kmers
 * uint64[n_entries], nodes int32[n_entries], frequencies uint16[n_entries], each host or device memory.  A NULL table, or a
 * NULL per-entry array while n_entries > 0, is KMM_ERR_INVALID_ARG and nothing is copied.  May be called again.
 * kmm_seq_index_destroy — frees the object (NULL: nothing).
 * kmm_seq_index_modulo — pure, no device: what modulo == 0 chooses for n_entries entries.
 */
typedef struct kmm_seq_index kmm_seq_index_t;
#define KMM_SEQIDX_BOTH_STRANDS 1
#define KMM_SEQIDX_DEBUG_SHORT_ROUNDS 0x40000000 /* TEST ONLY: an emit round is two super-tiles (2 Mi bases) instead of 2^20
                                                  * tiles, so that a 3 Mi-base input crosses a round seam; the result is the same */
#define KMM_SEQIDX_MAX_PAIRS (1ll << 30)         /* pairs of P one call takes (the de-duplication table keeps 32-bit indices) */
int kmm_seq_index_build(int device, const uint8_t *bases, const int64_t *seq_offsets, int64_t n_seqs,
                        const int32_t *seq_nodes, int k, const uint8_t *lut, int flags, uint64_t modulo,
                        kmm_seq_index_t **out);
int kmm_seq_index_info(const kmm_seq_index_t *s, int64_t *n_entries, uint64_t *modulo, int64_t *n_windows, int64_t *n_pairs);
int kmm_seq_index_fetch(kmm_seq_index_t *s, int32_t *hashes_to_index, int32_t *n_kmers, uint64_t *kmers, int32_t *nodes,
                        uint16_t *frequencies);
void kmm_seq_index_destroy(kmm_seq_index_t *s);
uint64_t kmm_seq_index_modulo(int64_t n_entries);

/*
 * Measurement hooks (the reference only logs perf_counter deltas,
 * command_line_interface.py:67-78).  With timing on, every launch of a hot-path kernel is
 * bracketed by HIP events on the handle's stream; kmm_get_timing drains the stream and returns,
 * for one kernel id, the summed milliseconds and the number of launches since the last call for
 * that id, then clears them.
 */
#define KMM_KERNEL_MAP_READS 0    /* fused direct kernel (reads -> counts)                    */
#define KMM_KERNEL_MAP_KMERS 1    /* operator kernel (uint64 k-mers -> counts)                */
#define KMM_KERNEL_RX_P1 2        /* radix path, pass 1: reads -> blocks sorted by coarse hash range   */
#define KMM_KERNEL_RX_SCAN 3      /* radix path: directory column scan between pass 1 and pass 2       */
#define KMM_KERNEL_RX_P2 4        /* radix path, pass 2: items sorted by fine hash range               */
#define KMM_KERNEL_RX_P3 5        /* radix path, pass 3: probe of LDS-resident index slices + counting */
#define KMM_KERNEL_RX_FLUSH 6     /* radix path: per-entry hit counts -> node counts                   */
#define KMM_KERNEL_BGZF_DEFLATE 7 /* BGZF writer: text -> one member per 65280 bytes, in slots             */
#define KMM_KERNEL_BGZF_GATHER 8  /* BGZF writer: member offsets + the members one behind the other       */
#define KMM_KERNEL_BAM_RAW 9      /* "record_bam": record base, count, scans, copy and advance of the kept BAM records */
#define KMM_KERNEL_BAM_RAW_MATES 10 /* "record_bam_mates": the pair forms of the above, the mate check and the carried mate 1 */
#define KMM_KERNEL_SAM_RAW 11     /* "record_sam": the tiles' scan, flags, block scan, copy and advance of the kept SAM lines */
#define KMM_KERNEL_RH_QUAL_MARK 12 /* "record_hits_min_base_quality": line starts and the mark pass in front of the hit kernel */
#define KMM_KERNEL_SAM_RAW_MATES 13 /* "record_sam_mates": the pair forms of the above, the spans by entry and the mate check */
#define KMM_N_KERNELS 14
int kmm_set_timing(kmm_index_t *idx, int enabled);
/* Work done by the map calls of this handle since creation (or the last call with reset != 0):
 * k-mer lookups performed (windows, doubled with also_revcomp) and count increments (index hits that
 * passed the frequency filter) — the numbers the reference logs per chunk
 * (command_line_interface.py:53, util.py:74).  Synchronises like kmm_get_node_counts. */
int kmm_get_stats(kmm_index_t *idx, int reset, uint64_t *n_lookups, uint64_t *n_hits);
int kmm_get_timing(kmm_index_t *idx, int kernel_id, double *kernel_ms, int64_t *n_launches);

/*
 * kmm_get_kmer_counts — per-k-mer counting mode: replaces the table lookup of GpuCounter.get_node_counts
 * (gpu_counter.py:29-34, `counter[index_kmers]`) and the CounterKmerIndex branch of the CLI
 * (command_line_interface.py:46-49,133-138): out[l] = number of mapped k-mers that matched index entry l
 * (entry order of the arrays given to kmm_index_create; the frequency filter of every map call applied) since
 * the mode was switched on or the last kmm_reset_counts.  Needs kmm_set_param(idx, "count_kmers", 1) BEFORE the
 * map calls; the node counts are still maintained (they are the segmented sum of these counts over
 * nodes[l], which is how the reference's GPU counter derives them, gpu_counter.py:37).  out: uint32[n_entries],
 * host or device.  Synchronises.
 */
int kmm_get_kmer_counts(kmm_index_t *idx, uint32_t *out);

/*
 * Tuning knobs, for experiments and benchmarks (defaults are chosen at index creation):
 *   "path"             0 = auto (by batch size), 1 = direct fused kernel (one HBM gather per k-mer),
 *                      2 = radix path (two partition passes by hash range + probe of LDS-resident index
 *                      slices)
 *   "part_shift"       log2 of the number of hash buckets per fine partition of the radix path (0..13)
 *   "radix_min_units"  auto: smallest batch (positions / k-mers) that takes the radix path; default: where the two
 *                      paths break even under a cost model fitted to measurements (~0.38 M reads of 150 bp at a
 *                      100 M-k-mer index)
 *   "radix_grid_per_cu" persistent workgroups per CU of passes 2 and 3 (1 or 2; 2 by default)
 *   "radix_sorted_flush" 1 (default) = per-entry counts are added to the node counts through the node-ordered entry
 *                      list (built when an index has fewer than 8 entries per node on average); 0 = in bucket order
 *   "count_kmers"      1 = per-k-mer counting mode (see kmm_get_kmer_counts)
 *   "radix_filter"     1 (default) = pass 2 drops the k-mers whose bucket is empty (they cannot match: mapper.pyx:55-58)
 *                      wherever a coarse partition's occupancy bitmap fits 64 KB of LDS, at one bit per bucket or — sparse
 *                      tables — per 2 or 4 buckets ("radix_filter_buckets_per_bit", read-only); the fan-out is chosen for it
 *   "radix_filter_slots" 1 (default) = where the coarse partitions have exactly 2^19 buckets at one bit per bucket (the
 *                      fan-out chosen for the filter: the 10 M- and 100 M-k-mer indexes) the filter spends 3 bits per PAIR
 *                      of buckets, keyed by bucket and by the k-mer's quotient (96 KB of LDS; an array of 96 KB per coarse
 *                      partition in HBM, optional like the bitmap): 28 % of the absent k-mers pass instead of 39 % at
 *                      load factor 0.5, the counts are the same.  0 = the bucket bitmap there too (also: environment
 *                      variable KMM_RX_FILTER_SLOTS=0 at creation).  "radix_filter_bits_per_partition" (read-only): the
 *                      filter bits of one coarse partition in LDS — 786432, or 524288 and fewer with the bitmap, 0
 *                      without a filter.  The sort buffer beside the slot filter holds 5888 k-mers: an item with more
 *                      survivors is placed and copied out in rounds ("radix_p2_multi_round_items", read-only, counts
 *                      them since the statistics were last reset)
 *   "radix_p3_fingerprints" 1 (default) = pass 3 keeps one fingerprint byte per LDS-resident entry and reads the 8-byte keys
 *                      of the entries whose byte equals the k-mer's only (the variant for slices of up to 4096 buckets with
 *                      the 16-bit directory: the 10 M- and 100 M-k-mer indexes; reads 1 only where that variant runs);
 *                      0 = every entry of a bucket is compared (also: KMM_RX_P3_FP=0 at creation).  The counts are the same
 *   "radix_packed_tiles" 1 (default) = pass 1 on reads of one length works on tiles of whole reads (no windows across
 *                      read boundaries are computed)
 *   "fine_bits"        experiments: log2 fine partitions per coarse partition of the radix path
 *   "radix_sub_batch_kmers" k-mer slots per sub-batch of the radix path: a larger map call is cut into equal sub-batches,
 *                      each a full run of the passes (the index slices are streamed once per sub-batch); default and
 *                      maximum 2^32 - 2 * 8192 (a coarse partition's k-mers are numbered with 32 bits).  When the batch
 *                      buffers of that size do not fit the free HBM a call takes one sub-batch more, and again (down to
 *                      2^28 slots); the size it ran with is "radix_sub_batch_kmers_effective" (read-only), kept for the
 *                      handle's next 15 calls, after which the caller's value is tried again
 *   "host_pack_threads" the host cores' share of the read bytes — the reference's `-t` (command_line_interface.py:168).  > 0: reads
 *                      that arrive in HOST memory (kmm_map_reads_uniform; kmm_map_reads with host offsets; kmm_map_records
 *                      with FASTQ / two-line FASTA bytes — a file mapping or an inflater's output, pinned or not; default
 *                      lookup table, a batch large enough for the radix path) are packed to 2 bits per base by that many
 *                      threads of a per-handle pool inside the call and cross PCIe at a quarter of their size
 *                      (csrc/kmm_hostpack.hpp: AVX-512 VBMI / AVX2 / scalar; for records the sequence lines go straight
 *                      from the raw bytes to the 2-bit stream + read-start bitset, by the rules of the device parser); a
 *                      byte outside the table or a malformed record sends the call down the ordinary route, which reports
 *                      it with its offset.  The packer knows no breaks (KMM_LUT_BREAK): a table with a break entry is a
                      caller's table like any other and takes the device routes — the raw bytes cross PCIe as they are
                      (the price on plain FASTQ: profiles/ambiguous/README.md).  0: the bytes cross as they are.  Default: min(16, "host_cpu_budget") when that
 *                      budget — the CPUs of the affinity mask but one, cut by the cgroup's CPU quota — is at least 8, else
 *                      0; environment KMM_HOST_PACK_THREADS overrides it at index creation.
 *                      "host_packed_calls" / "host_packed_record_calls" (read-only) count the calls that took the route;
 *                      "host_pack_slice_kb": raw bytes per slice the records packer hands its threads (0 = default, 1024)
 *   "bgzf_head_skip" / "bgzf_tail_stop"  a RANK'S SHARE of a BGZF file (several processes on one file, kmm_map_bgzf; kmm_map_bam with
 *                      KMM_FORMAT_MID_STREAM takes the head skip, every kmm_map_bam stream the tail stop): the next
 *                      call with KMM_FORMAT_NEW_STREAM passes over that many inflated bytes of its first member (they end a
 *                      record of the rank before), the next call with KMM_FORMAT_LAST_CHUNK takes only that many inflated
 *                      bytes of its last member (the rest starts the next rank's first record); each is used once
 *                      (tail: -1 = all, the default).  The boundaries are the caller's business
 *                      (kmer_mapper_amd/bgzf_ranges.py: record-structure resynchronisation on the members around a boundary)
 *   "bam_n_ref"        n_ref of the next kmm_map_bam stream started with KMM_FORMAT_MID_STREAM (kmm_bam_header returns it): -1
 *                      (default: not set) or 0 .. 2^31 - 1; read/write
 *   "debug_bam_resync_kb" test hook of kmm_bam_find_record_start: inflated bytes it examines at most, in KiB — the bytes end at the
 *                      cap as if the window did, so a small file shows the "longer window" answer and a forged chain can reach
 *                      the end; not for callers, no effect at 0
 *   "debug_gzip_chunk_kb" test hook of kmm_map_gzip: spacing of the chunk search in KiB (0 = the default, 32; a test file of a
 *                      few MB then has hundreds of chunks).  Read-only: "gzip_calls", "gzip_members" (members whose CRC32 and
 *                      ISIZE were checked), "gzip_chunks" (speculative starts decoded, every call's first chunk included),
 *                      "gzip_false_starts" (starts rejected by the predecessor check), "gzip_continuations" (lanes re-run past
 *                      a rejected start or a full output slot), "gzip_inflated_bytes" (inflated so far: a caller's ratio for
 *                      sizing its next window)
 *   "bam_exclude_flags" kmm_map_bam and KMM_FORMAT_SAM: records whose FLAG has any of these bits are not mapped (0 = the
 *                      default: every record, as the reference; 0x900 = no secondary and supplementary alignments).  Read-only: "bam_calls",
 *                      "bam_records" (mapped), "bam_records_excluded", "bam_header_bytes", "bam_false_starts" (speculative
 *                      starts the link check rejected), "bam_continuations" (tiles walked again from the exit before them)
 *   "bam_include_flags" kmm_map_bam and KMM_FORMAT_SAM: only records whose FLAG has ALL of these bits are mapped (0 .. 0xFFFF,
 *                      default 0: every record; samtools view -f; RECORD SELECTION above)
 *   "bam_min_mapq"     kmm_map_bam and KMM_FORMAT_SAM: only records with MAPQ >= this are mapped (0 .. 255, default 0: MAPQ is not
 *                      read; samtools view -q).  Read-only: "record_regions" (intervals of kmm_set_record_regions after merging)
 *   "min_base_quality" a base-quality floor Q for FASTQ, 0 .. 93 (default 0 = off: nothing changes, bit for bit; anything else
 *                      KMM_ERR_INVALID_ARG).  With Q > 0, on every call that parses KMM_FORMAT_FASTQ records (kmm_map_records,
 *                      kmm_map_bgzf, kmm_map_gzip), a base whose quality byte q (Phred+33, unsigned — a byte below '!'
 *                      included) has q < 33 + Q is a break at that base exactly as a KMM_LUT_BREAK byte is: no window that
 *                      contains it is looked up, forward or reverse complement, the windows on either side are, *n_records
 *                      is unaffected and kmm_get_stats' n_lookups counts the surviving windows.  A table with break entries
 *                      combines with it: a base is dead if either rule kills it.  k = 1 is KMM_ERR_INVALID_ARG (as for a
 *                      break table).  KMM_FORMAT_FASTA2 / KMM_FORMAT_FASTA have no qualities: no effect.  KMM_FORMAT_SAM and
 *                      kmm_map_bam are refused with KMM_ERR_INVALID_ARG while Q > 0, unless "use_record_qual" is 1.  The FASTQ piece always takes
 *                      compaction + the radix path, at every batch size and whatever "path" says (as kmm_map_packed; an
 *                      index with "radix_available" 0: KMM_ERR_INVALID_ARG), and never the host packer
 *                      ("host_packed_record_calls" does not move).  A record whose quality line does not have as many
 *                      non-terminator bytes as its sequence line is KMM_ERR_MALFORMED at the next synchronising call, with
 *                      the raw byte offset of the quality line's '\n' (with Q = 0 nothing new is checked).  Read-only
 *                      "quality_masked_bases": sequence bases whose quality byte was below the floor since the statistics
 *                      were last reset (kmm_get_stats(reset)); synchronises like kmm_get_stats.  Flat reads
 *                      (kmm_map_reads, kmm_map_reads_uniform) carry no qualities and are unaffected; kmm_map_reads_qual
 *                      takes them as a second array and applies the same floor (its own rules are at its declaration)
 *   "use_record_qual"  0 (default) or 1; anything else KMM_ERR_INVALID_ARG.  0: the library as it is without the parameter, bit
 *                      for bit, the refusals above included.  1 and "min_base_quality" Q > 0: kmm_map_bam, and
 *                      kmm_map_records / kmm_map_bgzf / kmm_map_gzip with KMM_FORMAT_SAM, are served: every kept record's
 *                      QUAL is decoded beside its SEQ (csrc/kmm_bam.hpp, csrc/kmm_sam.hpp) and the floor applied
 *                      with the rules of "min_base_quality".  BAM qual bytes are raw Phred: a base is masked iff its byte
 *                      is < Q (0xFF and every other byte >= 93 are never masked); SAM QUAL bytes are Phred+33: masked iff
 *                      the unsigned byte is < 33 + Q.  A SAM QUAL that is exactly "*" (a one-base read's too, as htslib reads
 *                      it) and BAM qual bytes that start with 0xFF mean that the record stores no qualities: every base of
 *                      it survives — the caller who sets the switch accepts that — and the record is counted.  Records
 *                      dropped by "bam_exclude_flags" are not looked at.  *n_records, "sam_records" / "bam_records" are
 *                      unaffected; "quality_masked_bases" counts the low bytes of the kept records.  The records reach the
 *                      mapper as four-line FASTQ text in HBM, so what holds for KMM_FORMAT_FASTQ with a floor holds here:
 *                      compaction + the radix path whatever "path" says, and an index with "radix_available" 0 is refused
 *                      with KMM_ERR_INVALID_ARG ("min_base_quality needs the radix path"); k = 1 is KMM_ERR_INVALID_ARG.  A
 *                      SAM record whose QUAL is not "*" and not as long as its SEQ is KMM_ERR_MALFORMED, nothing of the call
 *                      mapped, the message naming the line's byte offset in the chunk (BAM: block_size already holds l_seq
 *                      qual bytes).  1 and Q = 0: QUAL is not read, not even its length — the calls are the ones without the
 *                      switch.  No effect on FASTQ, FASTA or flat reads.  Read-only "records_without_qual": kept SAM / BAM
 *                      records with at least one base that store no qualities, counted while the floor is applied, since
 *                      the statistics were last reset (kmm_get_stats(reset)); synchronises like "quality_masked_bases"
 *   "original_strand"  0 (default) or 1; anything else KMM_ERR_INVALID_ARG.  0: the library as it is without the parameter, bit
 *                      for bit: SEQ as stored.  1: on kmm_map_bam, and on kmm_map_records / kmm_map_bgzf / kmm_map_gzip with
 *                      KMM_FORMAT_SAM, every KEPT record whose FLAG has 0x10 — stored reverse-complemented by the aligner —
 *                      is handed to the mapper in read orientation, as `samtools fastq` writes it (csrc/kmm_bam.hpp,
 *                      csrc/kmm_sam.hpp).  SEQ is reversed and complemented: BAM by reversing the four bits of
 *                      the base code, =ACMGRSVTWYHKDBN -> =TGKCYSBAWRDMHVN (htslib's table); SAM text by A<->T, C<->G,
 *                      M<->K, R<->Y, V<->B, H<->D with upper and lower case each kept, W, S, N and every other byte ('=',
 *                      '.', U, ...) left as it is — the same records as BAM and as upper-case SAM give the same text.  The
 *                      lookup table is applied AFTER the flip, as for any other input: a KMM_LUT_BREAK letter breaks at its
 *                      mirrored position, a 0xFF letter is KMM_ERR_INVALID_BASE at the next synchronising call, the default
 *                      table turns the flipped read's N into A.  QUAL, where it is decoded ("use_record_qual" 1 and
 *                      "min_base_quality" Q > 0), is reversed and not complemented, so the masked base is the one the
 *                      sequencer called badly; absent qualities stay absent; "records_without_qual" and
 *                      "quality_masked_bases" keep their meaning; with "use_record_qual" 0 and Q > 0 the calls are refused
 *                      as without the switch.  A record with SEQ "*" / l_seq 0 has nothing to flip; records dropped by
 *                      "bam_exclude_flags" are not looked at (0x900 drops the partial and repeated records that `samtools
 *                      fastq` drops).  SEQ is flipped whole: clipping is not looked at.  *n_records, "bam_records",
 *                      "sam_records", *consumed and the carry between calls are unaffected (a record carried over is
 *                      flipped once, by the call that maps it).  No effect on FASTQ, FASTA, flat or packed reads.  Read-only
 *                      "records_reversed": kept records with 0x10 and at least one base that were flipped since the
 *                      statistics were last reset (kmm_get_stats(reset)); 0 while the switch is 0; synchronises like
 *                      "quality_masked_bases"
 *   "record_hits"      0 (default) / 1 / 2: the record-hits mode — the record calls append per-record index hits (2: and windows)
 *                      to a queue of the handle instead of counting nodes; see kmm_take_record_hits.  Read-only
 *                      "record_hits_pending", "record_hits_pending_mode"
 *   "record_keep"      0 (default) / 1: in the record-hits mode the record calls also append the text of the records that pass
 *                      the keep rule ("record_keep_min_hits", "record_keep_min_permille", "record_keep_invert") to a byte queue
 *                      of the handle; see kmm_take_kept_records.  Read-only "record_keep_pending_bytes",
 *                      "record_keep_pending_records"
 *   "record_pairs"     0 (default) / 1: while "record_keep" is 1 the records of a stream are interleaved mates, kept or dropped
 *                      together; "record_pairs_rule" 0 (default: any mate matches) / 1 (both do).  See kmm_map_record_pairs,
 *                      KEEPING MATES TOGETHER.  Read-only "record_keep_pending_bytes_mate2", "record_keep_pending_records_mate2"
 *   "record_names"     0 (default) / 1: in the record-hits mode kmm_map_bam decodes the selected records into four-line FASTQ with
 *                      their names and qualities — the text "record_keep" appends for BAM input; "record_names_mate_suffix"
 *                      0 (default) / 1: "/1" / "/2" behind the names.  Read-only "record_name_bytes_replaced".  See
 *                      kmm_take_kept_records, THE NAMED FORM.  "record_names_pairs" 0 (default) / 1: with "record_names" and
 *                      "record_keep", the selected records of a kmm_map_bam stream are mates in file order (2p, 2p + 1), their
 *                      names are compared on the device and they are kept or dropped together; see THE MATES OF A BAM STREAM
 *   "record_bam"       0 (default) / 1: kmm_map_bam with "record_hits" and "record_keep" appends the kept records' own bytes
 *                      (block_size word and all) to the keep queue instead of text; see THE RAW FORM, kmm_bam_stream_header
 *   "record_sam"       0 (default) / 1 / 2: a KMM_FORMAT_SAM call with "record_hits" and "record_keep" appends the kept records'
 *                      own lines to the keep queue, 1 with the header lines, 2 without; see SAM LINES KEPT AS SAM LINES
 *   "record_sam_mates" 0 (default) / 1: with "record_sam", the selected records of a SAM stream are mates in file order (2p,
 *                      2p + 1), their QNAME bytes are compared on the device and their lines are kept or dropped together;
 *                      read-only "record_sam_mate_waiting"; see SAM MATES KEPT TOGETHER
 *   "debug_records_piece_kb" test hook of kmm_map_records: bytes per piece in KiB (0 = the default, 2^30 bytes) — a file of a
 *                      few hundred KB then has several pieces; not for callers, no effect at 0
 *   "debug_records_grid" test hook of kmm_map_records: workgroups (four wavefronts each) of the two per-tile kernels of the
 *                      device-side compaction, 0 .. 65536 (anything else KMM_ERR_INVALID_ARG; 0 = the default, chosen from the
 *                      piece's size and the device's CUs) — with 1 a file of a few KB gives every wavefront the range of
 *                      consecutive 4 KiB tiles that only a piece beyond 32 MiB has otherwise; not for callers, no effect at 0
 *   "debug_bgzf_call_cap_kb" test hook of kmm_map_bgzf / kmm_map_bam: inflated bytes one call takes at most, in KiB (0 = the
 *                      default, 3.5 GiB) — a small file then reaches the cap.  Read-only "flat_uniform_batches": flat reads
 *                      of one length that took the uniform / packed front ends of the radix path
 *   "comm_overlap_slices" kmm_comm_reduce_counts: node ranges whose flush (per-entry hits -> node counts) runs under the
 *                      previous range's RCCL reduce on a second stream (default 8; 1 = flush, then one reduce).  A
 *                      parameter of the JOB: every rank must use the same value — it alone (with the vector's length)
 *                      decides how many collectives a rank issues; a rank that cannot flush by node range (no node-ordered
 *                      entry list for lack of HBM, "count_kmers" mode, "radix_sorted_flush" 0) flushes everything first and
 *                      issues the same reduces.  "comm_sliced_reduces" (read-only) counts the calls that issued them
 *   "debug_records_copy_stream" / "debug_records_skip" / "debug_rx_*"  test hooks of tools/records_overlap_bisect.py (run
 *                      the compaction kernels of kmm_map_records on the copy stream, next to the radix passes; skip one
 *                      of them; directory sums of pass 1) and of the tests ("debug_rx_buffer_limit": a pass-1 buffer
 *                      beyond that many bytes counts as out of memory: the call takes more sub-batches;
 *                      "debug_p2f_round_slots": slots of pass 2's sort buffer in use beside the slot filter, even, in
 *                      [512, 5888] — ordinary batches then take several rounds per item;
 *                      "debug_p3_key_reads" (read-only): 8-byte key reads of pass 3's probes, -DRX_P3_FP_STATS builds;
 *                      "debug_skew_p2_counter": trips the conservation check; "debug_ring_slot_kb": slot size of the
 *                      page-locked staging ring): not for callers, no effect at 0
 * Read-only (kmm_get_param): "radix_available", "radix_unavailable_reason" (0 available, 1 modulo >= 2^31, 2 slices too
 *   dense for LDS, 3 out of memory, 4 the index's buckets overlap), "n_partitions", "n_coarse_partitions",
 *   "n_fine_per_coarse", "radix_p2_kmers" / "radix_p3_kmers" / "radix_p2_dropped" (the conservation counters every
 *   synchronising call compares: KMM_ERR_INTERNAL), "radix_batches" / "direct_batches" (which path the map calls took),
 *   "radix_view_bytes" / "direct_view_bytes" / "direct_view_resident" (HBM budget: the direct view of an index beyond
 *   16 GiB of it is packed on first use), "radix_p3_keys_in_lds" (entries of a slice pass 3 keeps in LDS: 4096, 4608 or
 *   8192; buckets behind them are walked in HBM), "wide_buckets", "occupancy_filter", "bloom_filter_bytes".
 * Unknown names return KMM_ERR_INVALID_ARG.
 */
int kmm_set_param(kmm_index_t *idx, const char *name, int64_t value);
int kmm_get_param(kmm_index_t *idx, const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* KMM_H */
