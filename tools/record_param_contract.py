"""Record what kmm_set_param / kmm_get_param answer, name by name and value by value, into tests/golden/param_contract.json.

The recording is the contract tests/test_gpu_param_contract.py (every name, on the GPU) and tests/test_params_on_the_cpu.py (the
plain rows of csrc/kmm_params.hpp, without one) replay: run it once against a build of the commit whose behaviour is to be
kept, commit the fixture, and any later change of a return code, a message or a value read back shows up as a failed triple.

    python -m tools.record_param_contract --commit <hash> [--out tests/golden/param_contract.json]

NAMES is typed by hand from the two if-chains of commit b37f09b (csrc/kmm.hip), in the order of the chains: every name
kmm_set_param knew, then every name only kmm_get_param knew.  It is not derived from the table that replaced the chains, so a
row lost from the table is a failed test and not a shorter walk."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SET_NAMES = (
    "path", "part_shift", "radix_packed_tiles", "radix_filter", "radix_filter_slots", "radix_p3_fingerprints",
    "debug_p2f_round_slots", "fine_bits", "radix_min_units", "radix_sub_batch_kmers", "comm_overlap_slices", "radix_sorted_flush",
    "radix_grid_per_cu", "count_kmers", "grid_per_cu", "dynamic_schedule", "dyn_chunk", "occupancy_filter",
    "debug_records_copy_stream", "host_pack_threads", "host_pack_slice_kb", "bgzf_head_skip", "bgzf_tail_stop",
    "debug_bgzf_ring_slot_kb", "debug_ring_slot_kb", "bam_exclude_flags", "bam_include_flags", "bam_min_mapq", "bam_n_ref",
    "debug_bam_resync_kb", "debug_bgzf_call_cap_kb", "debug_gzip_chunk_kb", "debug_rx_buffer_limit", "debug_records_skip",
    "min_base_quality", "record_hits_min_base_quality", "record_hits", "record_keep", "record_keep_min_hits",
    "record_keep_min_permille", "record_keep_invert", "record_pairs", "record_names_pairs", "record_pairs_rule",
    "record_keep_pending_bytes", "record_keep_pending_records", "record_keep_pending_bytes_mate2",
    "record_keep_pending_records_mate2", "use_record_qual", "record_names", "record_names_mate_suffix", "record_bam", "record_sam",
    "record_sam_mates", "record_bam_mates", "original_strand", "debug_records_piece_kb", "debug_records_grid",
    "debug_skew_p2_counter",
)
GET_ONLY_NAMES = (
    "host_packed_calls", "host_packed_record_calls", "bgzf_prestaged_calls", "gzip_calls", "gzip_members", "gzip_chunks",
    "gzip_false_starts", "gzip_continuations", "gzip_inflated_bytes", "record_hits_pending", "record_hits_pending_mode",
    "record_sam_mate_waiting", "read_hits_calls", "bam_calls", "bam_records", "bam_records_excluded", "bam_header_bytes",
    "bam_false_starts", "bam_continuations", "record_regions", "sam_calls", "sam_records", "sam_records_excluded",
    "sam_header_lines", "flat_uniform_batches", "bgzf_members", "bgzf_carry_bytes", "host_cpu_budget",
    "radix_sub_batch_kmers_effective", "comm_sliced_reduces", "debug_rx_t1_sum", "debug_rx_start1_sum", "debug_rx_items",
    "radix_available", "radix_batches", "direct_batches", "radix_unavailable_reason", "direct_view_resident", "direct_view_bytes",
    "radix_view_bytes", "radix_p3_keys_in_lds", "radix_filter_buckets_per_bit", "radix_filter_bits_per_partition",
    "n_fine_per_coarse", "n_coarse_partitions", "radix_p2_kmers", "radix_p3_kmers", "radix_p2_dropped",
    "radix_p2_multi_round_items", "quality_masked_bases", "records_without_qual", "records_reversed",
    "record_name_bytes_replaced", "debug_p3_key_reads",
    # the one prefix form, "stats_slot_<n>": both ends of the block, one past either, and what atoi makes of no digits
    "stats_slot_0", "stats_slot_2", "stats_slot_3", "stats_slot_31", "stats_slot_32", "stats_slot_-1", "stats_slot_", "stats_slot_x",
    "bloom_filter_bytes", "occupancy_bits_per_bucket", "wide_buckets", "n_partitions",
)
NAMES = SET_NAMES + GET_ONLY_NAMES

PROBES = (-2, -1, 0, 1, 2, 3, 4, 9, 10, 13, 14, 64, 65, 93, 94, 255, 256, 511, 512, 1000, 1001, 1024, 1025, 4096, 4097, 65535,
          65536, 2 ** 20, 2 ** 20 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 62)

ZERO_ONLY = ("debug_skew_p2_counter",)   # it exists to make the next synchronising call fail: no value walk, probed with 0 alone
CODE_ONLY = ("host_cpu_budget",)         # its value is the machine's: the return code alone


def probes_of(name):
    return (0,) if name in ZERO_ONLY else PROBES


def n_triples():
    return sum(len(probes_of(n)) for n in NAMES)


def _get(L, h, name):
    """[return code, the value — or the message where the get failed]"""
    import ctypes
    v = ctypes.c_int64(0)
    rc = L.kmm_get_param(h, name.encode(), ctypes.byref(v))
    if rc != 0:
        return [rc, L.kmm_last_error().decode("utf-8", "replace")]
    return [rc, None if name in CODE_ONLY else v.value]


def _set(L, h, name, value):
    """[return code, the message of a refusal or None]"""
    rc = L.kmm_set_param(h, name.encode(), int(value))
    return [rc, L.kmm_last_error().decode("utf-8", "replace") if rc != 0 else None]


def walk(make_handle):
    """The whole walk on the library under test.  make_handle(): a context manager that yields a fresh DeviceIndex over the
    index of smoke().  Returns {"defaults": {name: get}, "walk": {name: [[value, set, get], ...]}}."""
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    out = {"defaults": {}, "walk": {}}
    with make_handle() as dev:
        for name in NAMES:
            out["defaults"][name] = _get(L, dev._h, name)
    for name in NAMES:
        with make_handle() as dev:
            out["walk"][name] = [[v, _set(L, dev._h, name, v), _get(L, dev._h, name)] for v in probes_of(name)]
    return out


def smoke_handles():
    """make_handle for walk(): fresh handles on the 1000-entry synthetic index of smoke(), where the radix path is available."""
    from kmer_mapper_amd import synthetic
    from kmer_mapper_amd.engine import DeviceIndex
    index, _ = synthetic.make_index(1000, seed=1)
    mx = index.max_node_id()
    return lambda: DeviceIndex.from_index(index, mx, device=0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="the commit the library under test was built from (noted in the fixture)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "param_contract.json"))
    a = ap.parse_args()
    rec = walk(smoke_handles())
    doc = {"recorded_from": a.commit, "names": list(NAMES), "probes": list(PROBES), "zero_only": list(ZERO_ONLY),
           "code_only": list(CODE_ONLY), "defaults": rec["defaults"], "walk": rec["walk"]}
    # one name per line: a changed triple is a one-line diff
    with open(a.out, "w") as f:
        f.write("{\n")
        for key in ("recorded_from", "names", "probes", "zero_only", "code_only", "defaults"):
            f.write(" %s: %s,\n" % (json.dumps(key), json.dumps(doc[key], separators=(",", ":"))))
        f.write(' "walk": {\n')
        f.write(",\n".join("  %s: %s" % (json.dumps(n), json.dumps(doc["walk"][n], separators=(",", ":"))) for n in NAMES))
        f.write("\n }\n}\n")
    print("recorded %d names, %d triples from %s -> %s" % (len(NAMES), n_triples(), a.commit, a.out))


if __name__ == "__main__":
    main()
