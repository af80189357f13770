"""GPU tests of pass 2's slot filter (k_rx_p2f<P2F_SLOT, ...>, csrc/kmm_radix.hpp; rx_filter_slot, csrc/kmm_radix_plan.hpp):
coarse partitions of exactly 2^19 buckets are filtered with 3 bits per bucket pair keyed by bucket and quotient, and the sort
buffer beside the filter holds fewer slots than an item has k-mers, so an item with many survivors is placed and copied
out in rounds.  Everything against the oracle, on an index of six coarse partitions of 2^19 buckets (the last one partial)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P2F_SLOTS = 5888          # kmm_radix_plan.hpp: slots of the sort buffer beside the filter
SLOT_BITS = 3 << 18       # filter bits per coarse partition; the bucket bitmap has 1 << 19


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def syn():
    from kmer_mapper_amd import synthetic
    return synthetic


@pytest.fixture(scope="module")
def case(syn, oracle):
    """The index, a ragged batch and the oracle's counts for it (computed once, never modified)."""
    index, genome = syn.make_index(300000, seed=351, modulo=3000017)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 40000, 0, 260, seed=352)
    expect, n = oracle.map_reads(index, mx, bases, offs, 31, also_revcomp=True, n_threads=4)
    expect.setflags(write=False)
    return dict(index=index, genome=genome, mx=mx, bases=bases, offs=offs, expect=expect, n=n)


def open_index(kmm, case, part_shift=12, fine_bits=7):
    dev = kmm.DeviceIndex.from_index(case["index"], case["mx"])
    dev.set_param("part_shift", part_shift)
    dev.set_param("fine_bits", fine_bits)
    dev.set_param("path", 2)
    return dev


def map_and_check(dev, case):
    """Maps the batch on a handle whose counters are clear; returns (dropped, items that took several rounds)."""
    dev.map_reads(case["bases"], case["offs"], 31, also_revcomp=True)
    assert np.array_equal(dev.get_node_counts(), case["expect"])
    dropped = dev.get_param("radix_p2_dropped")
    assert dev.get_param("radix_p2_kmers") == 2 * case["n"]
    assert dev.get_param("radix_p3_kmers") + dropped == 2 * case["n"]
    multi = dev.get_param("radix_p2_multi_round_items")
    assert dev.get_stats(reset=True)[0] == 2 * case["n"]
    dev.reset()
    return dropped, multi


def test_slot_filter_against_the_bucket_bitmap(kmm, case):
    """(a) "radix_filter_slots" 1 then 0 on one handle: the counts are the oracle's both times, the slot filter drops more."""
    with open_index(kmm, case) as dev:
        assert dev.get_param("n_coarse_partitions") == 6 and dev.get_param("n_fine_per_coarse") == 128
        assert dev.get_param("radix_filter_slots") == 1
        assert dev.get_param("radix_filter_bits_per_partition") == SLOT_BITS == 786432
        assert dev.get_param("radix_filter_buckets_per_bit") == 1
        dropped_slots, multi = map_and_check(dev, case)
        assert multi == 0
        dev.set_param("radix_filter_slots", 0)
        assert dev.get_param("radix_filter_slots") == 0
        assert dev.get_param("radix_filter_bits_per_partition") == 524288
        dropped_bitmap, multi = map_and_check(dev, case)
        assert multi == 0
        print("dropped of %d: slot filter %d, bucket bitmap %d" % (2 * case["n"], dropped_slots, dropped_bitmap))
        assert dropped_slots > dropped_bitmap > 0
        dev.set_param("radix_filter_slots", 1)
        assert dev.get_param("radix_filter_bits_per_partition") == SLOT_BITS
        assert map_and_check(dev, case) == (dropped_slots, 0)


@pytest.mark.parametrize("part_shift, fine_bits", [(12, 7), (11, 8)])
@pytest.mark.parametrize("round_slots", [1024, 514])
def test_forced_rounds(kmm, case, part_shift, fine_bits, round_slots):
    """(b) "debug_p2f_round_slots": the ordinary batch (8192 k-mers per full item, a tenth of them hits, some 1200 survivors)
    takes 2-3 rounds per item.  Both scans of the sort place in rounds: fan-out 128 takes the per-wavefront scan
    (k_rx_p2f<P2F_SLOT, true>), fan-out 256 — part_shift 11 with 8 fine-partition bits, the same 2^19 buckets per coarse
    partition — the table of bases (k_rx_p2f<P2F_SLOT, false>).  (fine_bits 8 at part_shift 12 would leave the slot filter:
    2 buckets per bit.)"""
    with open_index(kmm, case, part_shift, fine_bits) as dev:
        assert dev.get_param("n_fine_per_coarse") == 1 << fine_bits
        assert dev.get_param("radix_filter_bits_per_partition") == SLOT_BITS
        dropped, multi = map_and_check(dev, case)
        assert multi == 0
        dev.set_param("debug_p2f_round_slots", round_slots)
        assert dev.get_param("debug_p2f_round_slots") == round_slots
        dropped_r, multi = map_and_check(dev, case)
        assert dropped_r == dropped
        assert multi > 0
        dev.set_param("debug_p2f_round_slots", P2F_SLOTS)
        assert map_and_check(dev, case) == (dropped, 0)


def test_rounds_without_the_hook_when_every_kmer_survives(kmm, syn, oracle, case):
    """(c) 200 000 reads of 31 bases, each spelling a k-mer of the index (drawn with repeats): every k-mer survives the
    filter, so every full item (8192 k-mers) has more survivors than the sort buffer has slots and takes two rounds."""
    rng = np.random.default_rng(353)
    genome, index, mx = case["genome"], case["index"], case["mx"]
    at = 4 * rng.integers(0, 300000, size=200000, dtype=np.int64)            # make_index: the k-mers at every 4th position
    bases = np.ascontiguousarray(syn.ACGT[genome[at[:, None] + np.arange(31, dtype=np.int64)[None, :]]]).reshape(-1)
    offs = 31 * np.arange(200001, dtype=np.int64)
    expect, n = oracle.map_reads(index, mx, bases, offs, 31, n_threads=4)
    assert n == 200000 and int(expect.sum()) >= n
    with open_index(kmm, case) as dev:
        dev.map_reads(bases, offs, 31)
        assert np.array_equal(dev.get_node_counts(), expect)
        assert dev.get_param("radix_p2_dropped") == 0
        assert dev.get_param("radix_p3_kmers") == n
        # six coarse partitions of ~33 000 k-mers: four full items each
        assert dev.get_param("radix_p2_multi_round_items") >= 6 * 3


def test_round_slots_refuses_bad_values(kmm, case):
    """(d) odd, beyond the sort buffer, 0 (and below 512): an error, and the handle keeps its value."""
    with open_index(kmm, case) as dev:
        for bad in (1025, P2F_SLOTS + 2, 0, 510, -2):
            with pytest.raises(ValueError):
                dev.set_param("debug_p2f_round_slots", bad)
            assert dev.get_param("debug_p2f_round_slots") == P2F_SLOTS
        dev.set_param("debug_p2f_round_slots", 512)
        with pytest.raises(ValueError):
            dev.set_param("debug_p2f_round_slots", 8192)
        assert dev.get_param("debug_p2f_round_slots") == 512
        assert map_and_check(dev, case)[1] > 0


def test_reconfiguring_rebuilds_or_drops_the_filter(kmm, case):
    """(e) fine_bits 8 (2 buckets per bit: the bitmap, folded) and back to 7 on one handle."""
    with open_index(kmm, case) as dev:
        first = map_and_check(dev, case)
        dev.set_param("fine_bits", 8)
        assert dev.get_param("radix_filter_slots") == 0
        assert dev.get_param("radix_filter_buckets_per_bit") == 2
        assert dev.get_param("radix_filter_bits_per_partition") == 524288
        folded = map_and_check(dev, case)
        assert 0 < folded[0] < first[0]
        dev.set_param("fine_bits", 7)
        assert dev.get_param("radix_filter_slots") == 1
        assert dev.get_param("radix_filter_buckets_per_bit") == 1
        assert dev.get_param("radix_filter_bits_per_partition") == SLOT_BITS
        assert map_and_check(dev, case) == first
        dev.set_param("part_shift", 11)      # (the fan-out is derived anew: 2^18 buckets per coarse partition or fewer)
        dev.set_param("fine_bits", 8)
        assert dev.get_param("radix_filter_slots") == 1
        assert map_and_check(dev, case)[0] == first[0]      # same buckets, same quotients: the same k-mers are dropped
        dev.set_param("radix_filter", 0)
        assert dev.get_param("radix_filter_bits_per_partition") == 0
        assert map_and_check(dev, case) == (0, 0)
