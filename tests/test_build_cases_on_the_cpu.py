"""CPU tier of the index-builder suite (tests/build_cases.py): every case of the catalogue is deterministic, is what its
name claims (by its own check, on the model's arrays), and has one answer on which three builders written differently agree
array for array and dtype for dtype: build_cases.model (argsort / bincount / cumsum / unique), the C oracle's
oracle_build_index (counting sort; quadratic counts up to 64 entries, a sorted copy with two binary searches beyond — its
long-bucket branch runs here at 65, 66, 129 ... 65 537 + 170 entries) and the package's KmerIndex.from_flat_kmers.  A case
that does not reach its seam fails here, before a GPU sees it.

Measured on an 8-core CPU-only machine: the whole module 35 s, of which long_input (16.8 M entries) 26 s — 11 s in the model,
10 s in from_flat_kmers, 1 s in the oracle, the rest building the case twice."""
import functools

import numpy as np
import pytest

from tests import build_cases as bc

FIELDS = ("_hashes_to_index", "_n_kmers", "_kmers", "_nodes", "_frequencies")
DTYPES = (np.int32, np.int32, np.uint64, np.int32, np.uint16)


@functools.lru_cache(maxsize=None)
def _model(name):
    c = bc.build(name)
    return bc.model(c.kmers, c.nodes, c.modulo)


def test_model_on_a_hand_worked_example():
    """Modulo 5: hashes 2 2 0 2 4 0 2 -> bucket 0 = entries 2, 5; bucket 2 = entries 0, 1, 3, 6; bucket 4 = entry 4."""
    kmers = np.array([7, 2, 10, 7, 2 ** 64 - 2, 5, 12], dtype=np.uint64)          # 2^64 - 2 = 4 (mod 5)
    nodes = np.array([70, 20, 100, 71, 2 ** 31 - 1, 50, 120])
    m = bc.model(kmers, nodes, 5)
    assert m.n_kmers.tolist() == [2, 0, 4, 0, 1] and m.hashes_to_index.tolist() == [0, 0, 2, 0, 6]
    assert m.kmers.tolist() == [10, 5, 7, 2, 7, 12, 2 ** 64 - 2] and m.nodes.tolist() == [100, 50, 70, 20, 71, 120, 2 ** 31 - 1]
    assert m.frequencies.tolist() == [1, 1, 2, 1, 2, 1, 1]
    assert tuple(a.dtype for a in m) == (np.int32, np.int32, np.uint64, np.int32, np.uint16)
    m = bc.model(np.full(70_000, 9, dtype=np.uint64), np.arange(70_000), 4)
    assert m.frequencies.tolist() == [65_535] * 70_000 and m.nodes.tolist() == list(range(70_000))


def test_the_catalogue_holds_every_required_case():
    assert len(set(bc.CASES)) == len(bc.CASES)
    for name in ("threshold", "clip", "many_big", "one_bucket-65", "one_bucket-70001", "long_input", "high_bits-100003"):
        assert name in bc.CASES
    for M in (1, 2, 1023, 1024, 1025, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1025):
        assert "scan_seams-%d" % M in bc.CASES
    for M in (2 ** 24 + 1, 2 ** 24 + 1025):
        assert "wide_modulo-%d" % M in bc.CASES
    assert sum(n.startswith("empty-") for n in bc.CASES) >= 3 and sum(n.startswith("single-") for n in bc.CASES) >= 3
    assert sum(n.startswith("high_bits-") for n in bc.CASES) == 2
    assert set(bc.THRESHOLD_LENGTHS) == {1, 2, 3, 4, 62, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047,
                                         2048, 2049, 3000, 4097}
    assert set(bc.LARGE_BUCKET_CASES) <= set(bc.CASES) and set(bc.OVER_A_MILLION) <= set(bc.CASES)


@pytest.mark.parametrize("name", bc.CASES)
def test_case_is_deterministic_shuffled_and_what_it_claims(name):
    c, again = bc.build(name), bc.build.__wrapped__(name)
    assert c.name == name and c.kmers.dtype == np.uint64 and c.nodes.dtype == np.int64 and c.kmers.shape == c.nodes.shape
    assert np.array_equal(c.kmers, again.kmers) and np.array_equal(c.nodes, again.nodes) and c.modulo == again.modulo
    assert not c.kmers.flags.writeable and not c.nodes.flags.writeable
    m = _model(name)
    c.check(c, m)
    n = c.kmers.shape[0]
    if n:
        assert int((c.kmers >> np.uint64(63)).sum()) > 0                      # k-mers with bit 63 set
        assert int(c.nodes.min()) >= 0 and int(c.nodes.max()) == 2 ** 31 - 1
    if n >= 2:
        assert int(c.nodes.min()) == 0 and int((c.kmers >> np.uint64(62) & np.uint64(1)).sum()) > 0
    if n > 100:
        # input order is no order the builder could reach by sorting: neither the k-mers nor the hashes ascend, and inside
        # the buckets the k-mers do not ascend either (so "stable by original position" differs from "sorted by k-mer")
        h = c.kmers % np.uint64(c.modulo)
        assert (np.diff(h.astype(np.int64)) < 0).any() or c.modulo == 1
        assert (c.kmers[1:] < c.kmers[:-1]).any()
        if name in bc.LARGE_BUCKET_CASES:
            same_bucket = np.diff(np.repeat(np.arange(c.modulo), m.n_kmers)) == 0
            assert (same_bucket & (m.kmers[1:] < m.kmers[:-1])).any()
    assert name in bc.OVER_A_MILLION or max(n, c.modulo) <= 1_200_000


def test_threshold_lengths_sit_at_adjacent_hashes():
    c, m = bc.build("threshold"), _model("threshold")
    first = bc.THRESHOLD_FIRST_HASH
    assert m.n_kmers[first:first + len(bc.THRESHOLD_LENGTHS)].tolist() == list(bc.THRESHOLD_LENGTHS)
    for x in (64, 128, 256, 1024, 2048):                    # c - 1, c, c + 1 side by side
        at = first + bc.THRESHOLD_LENGTHS.index(x)
        assert m.n_kmers[at - 1:at + 2].tolist() == [x - 1, x, x + 1]
    assert m.n_kmers[first - 1] == 0 and m.n_kmers[first + len(bc.THRESHOLD_LENGTHS)] == 0
    assert int((m.n_kmers > bc.BIG).sum()) == sum(x > bc.BIG for x in bc.THRESHOLD_LENGTHS) + 1      # + bucket 0 (65)


def test_clip_frequencies():
    c, m = bc.build("clip"), _model("clip")
    heavy = sorted(v for v in c.expected.values() if v[1] > 1000)
    assert heavy == [(65_534, 65_534), (65_535, 65_535), (65_535, 65_536), (65_535, 65_537)]
    assert sum(v == (70, 70) for v in c.expected.values()) == 4 and sum(v == (1, 1) for v in c.expected.values()) == 400
    assert np.bincount(m.frequencies)[[1, 70, 65_534, 65_535]].tolist() == [400, 280, 65_534, 65_535 + 65_536 + 65_537]


def test_many_big_needs_a_second_trip_and_long_input_too():
    m = _model("many_big")
    assert int((m.n_kmers > bc.BIG).sum()) >= 1100 > 1024
    assert bc.build("long_input").kmers.shape[0] == 65_536 * 256 + 300
    assert all(bc.build(n).modulo > 65_536 * 256 for n in bc.CASES if n.startswith("wide_modulo-"))


@pytest.mark.parametrize("name", bc.CASES)
def test_model_oracle_and_numpy_builder_agree(oracle, name):
    from kmer_mapper_amd.kmer_index import KmerIndex
    c, m = bc.build(name), _model(name)
    assert tuple(a.dtype for a in m) == DTYPES
    for who, ix in (("oracle_build_index", oracle.build_index(c.kmers, c.nodes, c.modulo)),
                    ("KmerIndex.from_flat_kmers", KmerIndex.from_flat_kmers(c.kmers, c.nodes, c.modulo))):
        got = bc.Index(ix._hashes_to_index, ix._n_kmers, ix._kmers, ix._nodes, ix._frequencies)
        assert tuple(a.dtype for a in got) == DTYPES, who
        assert bc.first_difference(c, got, m) is None, who
        assert all(np.array_equal(x, y) for x, y in zip(got, m)), who


def test_first_difference_names_the_bucket():
    c, m = bc.build("threshold"), _model("threshold")
    assert bc.first_difference(c, m, m) is None
    h = bc.THRESHOLD_FIRST_HASH + bc.THRESHOLD_LENGTHS.index(65)
    wrong = m.frequencies.copy()
    wrong[m.hashes_to_index[h] + 3] ^= 1
    msg = bc.first_difference(c, m._replace(frequencies=wrong), m)
    assert "frequencies" in msg and "bucket %d:" % h in msg and "length 65, above" in msg
    wrong = m.nodes.copy()
    wrong[m.hashes_to_index[h - 1]] ^= 1
    msg = bc.first_difference(c, m._replace(nodes=wrong), m)
    assert "nodes" in msg and "bucket %d:" % (h - 1) in msg and "length 64, at or below" in msg
    wrong = m.hashes_to_index.copy()
    wrong[5] = 9
    assert "hashes_to_index" in bc.first_difference(c, m._replace(hashes_to_index=wrong), m)
    assert "dtype" in bc.first_difference(c, m._replace(nodes=m.nodes.astype(np.int64)), m)
