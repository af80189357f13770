"""GPU tests of pass 3's fingerprint form (k_rx_p3<..., FP = true>, csrc/kmm_radix.hpp; rx_p3_fp and rx_p3_candidates,
csrc/kmm_radix_plan.hpp): a probe tests one byte per entry of its bucket's first five entries and reads the 8-byte keys of the
candidates only; entries 5 and up are walked key by key; buckets beyond the slice's LDS copy are walked in HBM.  Everything
against the oracle, on a dense index: modulo 65 537 under 60 593 entries — 17 slices of 4096 buckets, 20 buckets of 6 or
more entries, 1 593 entries that are k-mers under several nodes, one planted bucket of 1 501 entries in a slice of 5 163
(beyond the 4 096 kept in LDS)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 65537
FP_ENTRIES = 5


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


def fp_mirror(quot):
    """rx_p3_fp in Python integers (held to the header by tests/test_radix_p3_fp_on_the_cpu.py)."""
    v = (quot ^ (quot >> 24) ^ (quot >> 48)) & 0xFFFFFF
    return ((v * 0xB5297B) >> 16) & 0xFF


def reads_of(syn, kmers):
    """One 31-base read per k-mer (first base in the lowest two bits)."""
    q = np.asarray(kmers, dtype=np.uint64)
    codes = ((q[:, None] >> (2 * np.arange(31, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)
    return np.ascontiguousarray(syn.ACGT[codes]).reshape(-1), 31 * np.arange(q.shape[0] + 1, dtype=np.int64)


@pytest.fixture(scope="module")
def case(syn, oracle):
    """The index, the two batches and the oracle's counts for them (computed once, never modified)."""
    index, genome = syn.make_index(59000, seed=411, modulo=M)
    mx = index.max_node_id()
    h2i, nk, km = (np.asarray(a) for a in (index._hashes_to_index, index._n_kmers, index._kmers))
    assert km.shape[0] == 60593 and int(nk.sum()) == 60593 and int(nk.max()) == 1501 and int((nk >= 6).sum()) == 20
    pstart = np.concatenate([[0], np.cumsum(nk, dtype=np.int64)])
    slice_entries = [int(pstart[min(M, s + 4096)] - pstart[s]) for s in range(0, M, 4096)]
    assert max(slice_entries) == 5163 and sorted(slice_entries)[-2] <= 4096          # one slice takes the HBM walk
    # (a) ragged reads from the genome
    bases, offs = syn.make_ragged_reads(genome, 20000, 0, 260, seed=412)
    expect, n = oracle.map_reads(index, mx, bases, offs, 31, also_revcomp=True, n_threads=4)
    expect_f1, n_f1 = oracle.map_reads(index, mx, bases, offs, 31, max_index_lookup_frequency=1, also_revcomp=True, n_threads=4)
    assert n_f1 == n and 0 < int(expect_f1.sum()) < int(expect.sum())
    # (b) hand-built k-mers: buckets of 6 and more entries (not the planted one), of 1, 2 and 5, and one whose first entry
    # sits at each alignment inside its slice; of each the stored k-mers and absent k-mers b + t M whose fingerprint is that
    # of entry 0, of entry 4 (the last one tested by fingerprint) and of entry 5 (the first one walked)
    st = pstart[:-1] - pstart[np.arange(M) & ~4095]                                  # first entry, relative to the slice
    buckets = [int(b) for b in np.flatnonzero((nk >= 6) & (nk < 1000))]
    assert len(buckets) == 19
    for want in (1, 2, 5):
        buckets.append(int(np.flatnonzero(nk == want)[3]))
    for al in range(4):
        buckets.append(int(np.flatnonzero((nk >= 3) & ((st & 3) == al))[5]))
    assert sorted(set(int(st[b]) & 3 for b in buckets)) == [0, 1, 2, 3]
    hand, n_absent = [], 0
    for b in buckets:
        stored = [int(km[h2i[b] + j]) for j in range(int(nk[b]))]
        assert all(q % M == b for q in stored)
        hand += stored
        for j in (0, 4, 5):
            if j >= len(stored):
                continue
            target, found, t = fp_mirror(stored[j] // M), 0, 1 + 7919 * j
            while found < 3:
                t += 1
                if fp_mirror(t) == target and b + t * M not in stored:
                    hand.append(b + t * M)
                    found += 1
                    n_absent += 1
    assert n_absent >= 3 * (19 * 3 + 4)
    hand = np.array(hand, dtype=np.uint64)
    assert int(hand.max()) < 1 << 62
    hbases, hoffs = reads_of(syn, hand)
    hexpect, hn = oracle.map_reads(index, mx, hbases, hoffs, 31, n_threads=4)
    assert hn == hand.shape[0] and int(hexpect.sum()) >= hand.shape[0] - n_absent
    for a in (expect, expect_f1, hexpect):
        a.setflags(write=False)
    return dict(index=index, mx=mx, bases=bases, offs=offs, expect=expect, expect_f1=expect_f1, n=n,
                hbases=hbases, hoffs=hoffs, hexpect=hexpect, hn=hn)


def open_index(kmm, case, part_shift=12):
    dev = kmm.DeviceIndex.from_index(case["index"], case["mx"])
    dev.set_param("part_shift", part_shift)
    dev.set_param("path", 2)
    return dev


def check_conservation(dev, n):
    assert dev.get_param("radix_p2_kmers") == n
    assert dev.get_param("radix_p3_kmers") + dev.get_param("radix_p2_dropped") == n
    assert dev.get_stats(reset=True)[0] == n
    dev.reset()


def map_ragged(dev, case, max_freq=1000):
    dev.map_reads(case["bases"], case["offs"], 31, max_index_lookup_frequency=max_freq, also_revcomp=True)
    assert np.array_equal(dev.get_node_counts(), case["expect"] if max_freq == 1000 else case["expect_f1"])
    check_conservation(dev, 2 * case["n"])


def map_hand(dev, case):
    dev.map_reads(case["hbases"], case["hoffs"], 31)
    assert np.array_equal(dev.get_node_counts(), case["hexpect"])
    check_conservation(dev, case["hn"])


def test_ragged_reads(kmm, case):
    """(a) 20 000 ragged reads and their reverse complements: the oracle's counts, every k-mer accounted for."""
    with open_index(kmm, case) as dev:
        assert dev.get_param("radix_p3_fingerprints") == 1
        assert dev.get_param("radix_p3_keys_in_lds") == 4096 and dev.get_param("n_partitions") == 17
        map_ragged(dev, case)


def test_hand_built_kmers_on_long_buckets(kmm, case):
    """(b) stored k-mers of the long buckets and absent k-mers that share the fingerprint of entry 0, 4 and 5."""
    with open_index(kmm, case) as dev:
        assert dev.get_param("radix_p3_fingerprints") == 1
        map_hand(dev, case)


def test_frequency_filter(kmm, case):
    """(c) max_index_lookup_frequency = 1: flagged entries take the add and are ignored by the flush."""
    with open_index(kmm, case) as dev:
        assert dev.get_param("radix_p3_fingerprints") == 1
        map_ragged(dev, case, max_freq=1)
        map_hand(dev, case)


def test_switch_off_and_on(kmm, case):
    """(d) "radix_p3_fingerprints" 0, then 1 again, on one handle: the same counts, and the getter follows."""
    with open_index(kmm, case) as dev:
        for value in (1, 0, 1):
            dev.set_param("radix_p3_fingerprints", value)
            assert dev.get_param("radix_p3_fingerprints") == value
            map_ragged(dev, case)
            map_hand(dev, case)


def test_another_variant_has_no_fingerprints(kmm, case):
    """(e) slices of 8192 buckets (7 500 entries: the variant with 8192 keys in LDS): the getter says 0, the counts hold."""
    with open_index(kmm, case, part_shift=13) as dev:
        assert dev.get_param("radix_p3_keys_in_lds") == 8192
        assert dev.get_param("radix_p3_fingerprints") == 0
        dev.set_param("radix_p3_fingerprints", 1)
        assert dev.get_param("radix_p3_fingerprints") == 0
        map_ragged(dev, case)
        map_hand(dev, case)
        dev.set_param("part_shift", 12)
        assert dev.get_param("radix_p3_fingerprints") == 1
        map_hand(dev, case)
