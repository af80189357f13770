"""The three users of the bucket walk (kmm_probe.hpp: walk_narrow / walk_wide) against each other on bucket shapes:
kmm_in_index (membership, no frequency bound), kmm_map_kmers on the direct path (counting, every entry) and kmm_read_hits
(membership under the bound), under the six index layouts of test_gpu_read_hits.LAYOUTS.  One hand-built index holds every
bucket length the walks distinguish and the entries that catch a walk which stops too early or too late; what is expected
comes from the CPU oracle and from the read-hits model, never from the library."""
import types

import numpy as np
import pytest

from oracle import oracle
from tests import read_hits_cases as rc
from tests.test_gpu_read_hits import LAYOUTS

pytestmark = pytest.mark.gpu

K = 31
M = 601                                   # buckets
BOUND = 100                               # splits FREQS
FREQS = np.array([1, 5, 100, 101, 1000, 3000], dtype=np.uint16)
LENGTHS = (0, 1, 2, 3, 4, 6, 1, 0, 2, 7, 3, 1, 5, 9)      # entries per bucket, repeated over the hashes
# buckets rebuilt by hand (hash: what it holds), all of them at hashes whose length in LENGTHS is replaced
SEVERAL_NODES, TRAP_4, TRAP_6, INLINE_HIGH, INLINE_TOP, MULTI_TOP = 2, 4, 5, 1, 6, 3


def _keys(rng, h, count):
    """`count` distinct k-mers of hash h below 4^K."""
    t = np.unique(rng.integers(0, ((1 << (2 * K)) - M) // M, size=count, dtype=np.uint64))
    assert t.shape[0] == count
    return np.uint64(h) + np.uint64(M) * rng.permutation(t)


def _build():
    rng = np.random.Generator(np.random.PCG64(2024))
    kmers, freqs, h2i, nk = [], [], np.zeros(M, np.int32), np.zeros(M, np.int32)
    for h in range(M):
        c = LENGTHS[h % len(LENGTHS)]
        km = _keys(rng, h, c)
        fr = FREQS[rng.integers(0, FREQS.shape[0], size=c)]
        if h == SEVERAL_NODES:            # X under two nodes, both entries under the bound, and a stranger
            x, y = _keys(rng, h, 2)
            km, fr = np.array([x, y, x], np.uint64), np.array([5, 1, 100], np.uint16)
        elif h == TRAP_4:                 # the first three entries are X above the bound, the last is X below it
            x = _keys(rng, h, 1)[0]
            km, fr = np.array([x] * 4, np.uint64), np.array([3000, 1000, 101, 100], np.uint16)
        elif h == TRAP_6:                 # the same with strangers around the entry that counts
            x, y, z = _keys(rng, h, 3)
            km, fr = np.array([x, x, x, y, x, z], np.uint64), np.array([101, 5000, 3000, 1, 50, 1000], np.uint16)
        elif h == INLINE_HIGH:            # a single entry above the bound
            fr = np.array([3000], np.uint16)
        elif h == INLINE_TOP:             # the largest frequency the format has, alone in its bucket
            fr = np.array([65535], np.uint16)
        elif h == MULTI_TOP:              # and among others
            fr = np.array([1, 65535, 1000], np.uint16)
        assert len(km) == len(fr) and (km % np.uint64(M) == np.uint64(h)).all()
        h2i[h], nk[h] = sum(len(a) for a in kmers), len(km)
        kmers.append(km)
        freqs.append(fr)
    kmers, freqs = np.concatenate(kmers).astype(np.uint64), np.concatenate(freqs).astype(np.uint16)
    nodes = rng.integers(0, 50, size=kmers.shape[0]).astype(np.int32)
    nodes[h2i[SEVERAL_NODES]], nodes[h2i[SEVERAL_NODES] + 2] = 7, 8
    index = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=nodes, _kmers=kmers, _frequencies=freqs, _modulo=M,
                                  max_node_id=lambda: 49)

    # ---- the queries: every stored k-mer, an absent k-mer of every bucket's hash, more of them in the empty buckets
    stored = np.unique(kmers)
    empty = np.flatnonzero(nk == 0)
    absent = np.concatenate([_keys(rng, h, 1) for h in range(M)] + [_keys(rng, h, 4) for h in empty])
    assert not np.isin(absent, stored).any()
    queries = rng.permutation(np.concatenate([stored, absent]))
    assert 2000 <= queries.shape[0] <= 5000 and int(queries.max()) < 1 << (2 * K)

    # ---- what the index is claimed to hold
    assert {0, 1, 2, 3, 4}.issubset(set(nk.tolist())) and nk.max() >= 6
    assert (kmers % np.uint64(M) == np.repeat(np.arange(M, dtype=np.uint64), nk)).all()
    bucket_of = np.repeat(np.arange(M), nk)
    place = np.arange(kmers.shape[0]) - h2i[bucket_of]                              # place of an entry inside its bucket
    uniq, first, n_copies = np.unique(kmers, return_index=True, return_counts=True)
    assert (n_copies > 1).any() and len({int(n) for n in nodes[kmers == kmers[h2i[SEVERAL_NODES]]]}) == 2
    last = (place == nk[bucket_of] - 1) & (nk[bucket_of] >= 4)
    assert (last & np.isin(kmers, uniq[n_copies == 1])).any()                       # a match that is a long bucket's last entry
    for h, n in ((TRAP_4, 4), (TRAP_6, 6)):
        sl = slice(h2i[h], h2i[h] + nk[h])
        x = kmers[sl][0]
        assert nk[h] == n and (kmers[sl][:3] == x).all() and (freqs[sl][:3] > BOUND).all()
        assert ((kmers[sl][3:] == x) & (freqs[sl][3:] <= BOUND)).any()
    assert nk[INLINE_HIGH] == 1 and freqs[h2i[INLINE_HIGH]] > BOUND
    assert nk[INLINE_TOP] == 1 and freqs[h2i[INLINE_TOP]] == 65535 and (freqs[bucket_of == MULTI_TOP] == 65535).any()
    assert (freqs <= BOUND).any() and (freqs > BOUND).any()
    return index, queries


@pytest.fixture(scope="module")
def world():
    """The index, the queries, the reads that spell them (one of K bases per query) and the expectations, computed once."""
    index, queries = _build()
    kmers, freqs, nodes = index._kmers, index._frequencies, index._nodes
    codes = ((queries[:, None] >> (np.uint64(2) * np.arange(K, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.int64)
    bases = np.ascontiguousarray(rc.ACGT[codes].reshape(-1))
    offsets = np.arange(queries.shape[0] + 1, dtype=np.int64) * K
    w = types.SimpleNamespace(index=index, queries=queries, bases=bases, offsets=offsets)
    w.present = oracle.in_index(index, queries)
    assert w.present[np.isin(queries, kmers[freqs == 65535])].all() and 0 < w.present.sum() < queries.shape[0]
    w.counts, w.hits, w.once, w.once_counts = {}, {}, {}, {}
    for bound in (BOUND, rc.NO_FILTER):
        w.counts[bound] = oracle.map_kmers(index, 49, queries, max_index_lookup_frequency=bound)
        hits, windows = rc.model(rc.index_arrays(index), bases, offsets, K, bound)
        assert (windows == 1).all()
        # "some entry of that k-mer has a frequency of at most the bound"
        assert np.array_equal(hits.astype(bool), np.isin(queries, kmers[freqs <= bound]))
        w.hits[bound] = hits
        # k-mers stored exactly once, under the bound: the three users agree on them
        uniq, n_copies = np.unique(kmers, return_counts=True)
        once = np.isin(queries, uniq[n_copies == 1]) & np.isin(queries, kmers[freqs <= bound])
        assert once.sum() > 100
        entry = np.flatnonzero(np.isin(kmers, queries[once]))
        w.once[bound] = once
        w.once_counts[bound] = np.bincount(nodes[entry], minlength=50).astype(np.uint32)
    assert w.hits[BOUND].sum() < w.hits[rc.NO_FILTER].sum() == w.present.sum()
    assert w.counts[BOUND].sum() < w.counts[rc.NO_FILTER].sum() == index._kmers.shape[0]      # every entry counts once
    return w


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.mark.parametrize("bound", [BOUND, rc.NO_FILTER], ids=["bound_100", "filter_off"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_the_three_users_agree_on_bucket_shapes(kmm, monkeypatch, world, layout, bound):
    env, wide, occ = LAYOUTS[layout]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    w = world
    n = w.queries.shape[0]
    with kmm.DeviceIndex.from_index(w.index, 49) as dev:
        assert (dev.get_param("wide_buckets"), dev.get_param("occupancy_filter")) == (wide, occ)
        dev.set_param("path", 1)
        # membership without a bound: the k-mers of frequency 65535 and those above BOUND are present
        present = dev.in_index(w.queries)
        assert np.array_equal(present, w.present), int(np.flatnonzero(present != w.present)[0])
        # counting: a k-mer under several nodes adds to each of them
        dev.map_kmers(w.queries, bound)
        counts = dev.get_node_counts()
        assert np.array_equal(counts, w.counts[bound]), int(np.flatnonzero(counts != w.counts[bound])[0])
        assert dev.get_stats() == (n, int(w.counts[bound].sum()))
        # membership under the bound: one read of K bases per query, ragged and through the uniform entry
        hits = dev.read_hits(w.bases, w.offsets, k=K, max_index_lookup_frequency=bound)
        assert np.array_equal(hits, w.hits[bound]), int(np.flatnonzero(hits != w.hits[bound])[0])
        u_hits = dev.read_hits(w.bases, n_reads=n, read_len=K, k=K, max_index_lookup_frequency=bound)
        assert np.array_equal(u_hits, w.hits[bound]), int(np.flatnonzero(u_hits != w.hits[bound])[0])
        # stored once, under the bound: present, a hit, and one count each
        once = w.once[bound]
        assert present[once].all() and (hits[once] == 1).all()
        dev.reset()
        dev.map_kmers(w.queries[once], bound)
        assert np.array_equal(dev.get_node_counts(), w.once_counts[bound]) and int(w.once_counts[bound].sum()) == int(once.sum())
