"""GPU tier of the index-builder suite: kmm_build_index (csrc/kmm_build.hpp, driver in csrc/kmm.hip) on the catalogue of
tests/build_cases.py — the small / large bucket hand-over at 64, the any-n bitonic network at 2^m - 1, 2^m, 2^m + 1 and at one
and two strides of its workgroup, more large buckets than workgroups, the uint16 clip at 65 534 .. 65 537, k-mers with bits 62
and 63 set, the second trip of every grid-stride loop (over the entries and over the modulo), carries on the scan's block
boundaries, one bucket for everything — against build_cases.model, which shares no structure with the builder or the C
oracle (tests/test_build_cases_on_the_cpu.py holds the catalogue to its claims and the oracle to the model).

Routes: host arrays through engine.build_index; device tensors through engine.build_index_device and through the raw entry
point with buffers this test owns, pre-filled with 0xA5 bytes and followed by 64 guard bytes (an entry no kernel wrote is then
a certain mismatch, and a write past the end shows); inputs and outputs on different sides.  Every case runs on every route;
nothing is left out.  The built index is then used: DeviceIndex.from_index on the GPU-built arrays must map like the oracle
on the model's.  Bit-exact: this is integer work."""
import ctypes
import functools
import time

import numpy as np
import pytest

from tests import build_cases as bc

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 64
ITEMSIZE = (4, 4, 8, 4, 2)                                   # hashes_to_index, n_kmers, kmers, nodes, frequencies
DTYPES = (np.int32, np.int32, np.uint64, np.int32, np.uint16)
NODE_MASK = 0xFFF        # the lookups count into 4096 nodes: a count vector over the catalogue's 2^31 node ids is 8.6 GB


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@functools.lru_cache(maxsize=None)
def _model(name):
    c = bc.build(name)
    return bc.model(c.kmers, c.nodes, c.modulo)


_host = {}


def _host_route(kmm, name):
    """engine.build_index on the case, once per module; (arrays, seconds of the GPU call with its copies)."""
    if name not in _host:
        c = bc.build(name)
        t0 = time.perf_counter()
        got = bc.Index(*kmm.build_index(c.kmers, c.nodes, c.modulo))
        _host[name] = (got, time.perf_counter() - t0)
    return _host[name]


def _same(case, got, want, what):
    got = bc.Index(*got)
    assert tuple(a.dtype for a in got) == DTYPES, (what, [a.dtype for a in got])
    msg = bc.first_difference(case, got, want)
    assert msg is None, "%s: %s" % (what, msg)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)), what


# ------------------------------------------------------------------------------------- buffers this test owns
class _Out:
    """The five output arrays on one side each ("d" device, "h" host), filled with 0xA5 and followed by guard bytes."""

    def __init__(self, n, M, sides):
        import torch
        self.sizes = [M * 4, M * 4, n * 8, n * 4, n * 2]
        self.bufs = []
        for nbytes, side in zip(self.sizes, sides):
            if side == "d":
                self.bufs.append(torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda"))
            else:
                self.bufs.append(np.full(nbytes + GUARD, SENTINEL, dtype=np.uint8))
        torch.cuda.synchronize()

    def pointers(self):
        return [ctypes.c_void_p(b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()) for b in self.bufs]

    def arrays(self):
        """The outputs on the host; the guard bytes behind every one of them must be untouched."""
        out = []
        for b, nbytes, dt in zip(self.bufs, self.sizes, DTYPES):
            raw = b if isinstance(b, np.ndarray) else b.cpu().numpy()
            assert (raw[nbytes:] == SENTINEL).all(), "bytes behind an output array were written"
            out.append(raw[:nbytes].copy().view(dt))
        return bc.Index(*out)


def _raw_build(case, in_sides, out_sides):
    """kmm_build_index through the C entry point, every pointer on the side asked for; returns (rc, _Out)."""
    import torch
    from kmer_mapper_amd import _lib
    km, nd = case.kmers, np.ascontiguousarray(case.nodes, dtype=np.int32)
    keep = []
    ptrs = []
    for a, side in zip((km.view(np.int64), nd), in_sides):
        if side == "d":
            t = torch.from_numpy(a.copy()).cuda()
            keep.append(t)
            ptrs.append(ctypes.c_void_p(t.data_ptr()))
        else:
            keep.append(a)
            ptrs.append(ctypes.c_void_p(a.ctypes.data))
    out = _Out(km.shape[0], case.modulo, out_sides)
    torch.cuda.synchronize()
    rc = _lib.lib().kmm_build_index(0, ptrs[0], ptrs[1], km.shape[0], case.modulo, *out.pointers())
    return rc, out


# ------------------------------------------------------------------------------------- the routes
@pytest.mark.parametrize("name", bc.CASES)
def test_host_route_equals_model(kmm, name):
    """engine.build_index == build_cases.model, all five arrays, values and dtypes; a failure names the first differing
    bucket, its length and its side of the hand-over at 64.

    Wall time of the cases above 10^6 elements on an MI355X, GPU call (engine.build_index with its host copies) / whole
    test with the numpy model: long_input 0.040 s / 4.07 s; wide_modulo-16777217 0.010 s / 0.081 s; wide_modulo-16778241
    0.010 s / 0.080 s; high_bits-67108859 0.035 s / 0.34 s.  Every other case: GPU call at most 0.03 s but the first of
    the process (0.15 s).  (Run with -s for the figures.)"""
    t0 = time.perf_counter()
    c, want = bc.build(name), _model(name)
    got, seconds = _host_route(kmm, name)
    _same(c, got, want, "host route")
    print("\n%-24s n %d modulo %d: GPU call %.3f s, whole test %.3f s" % (name, c.kmers.shape[0], c.modulo, seconds, time.perf_counter() - t0))


@pytest.mark.parametrize("name", bc.CASES)
def test_device_route_equals_host_route(kmm, name):
    """The same inputs as device tensors: engine.build_index_device (five in-place device outputs, no staging, nothing
    copied down by the library), and the raw entry point writing into 0xA5-filled device buffers of this test's.  Both
    identical to the host route — every case, long_input and the largest high_bits modulo included."""
    import torch
    c = bc.build(name)
    host, _ = _host_route(kmm, name)
    km = torch.from_numpy(c.kmers.view(np.int64).copy()).cuda()
    nd = torch.from_numpy(c.nodes.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    h2i, nk, ko, no, fo = kmm.build_index_device(km, nd, c.modulo)
    torch.cuda.synchronize()
    assert all(t.is_cuda for t in (h2i, nk, ko, no, fo))
    assert (h2i.dtype, nk.dtype, ko.dtype, no.dtype, fo.dtype) == (torch.int32, torch.int32, torch.int64, torch.int32, torch.uint16)
    got = (h2i.cpu().numpy(), nk.cpu().numpy(), ko.cpu().numpy().view(np.uint64), no.cpu().numpy(), fo.cpu().numpy())
    _same(c, got, host, "build_index_device")
    assert np.array_equal(km.cpu().numpy(), c.kmers.view(np.int64)) and np.array_equal(nd.cpu().numpy(), c.nodes)    # inputs intact
    del h2i, nk, ko, no, fo, km, nd
    rc, out = _raw_build(c, "dd", "ddddd")
    assert rc == 0
    _same(c, out.arrays(), host, "device inputs, sentinel-filled device outputs")


@pytest.mark.parametrize("in_sides, out_sides", [("dd", "hhhhh"), ("hh", "ddddd"), ("hd", "dhdhd"), ("dh", "hdhdh")])
def test_mixed_residency(kmm, in_sides, out_sides):
    """Some of the ten pointers on the host, some on the device (threshold): the staged and the in-place halves of the
    driver in one call.  All outputs pre-filled with 0xA5."""
    c = bc.build("threshold")
    rc, out = _raw_build(c, in_sides, out_sides)
    assert rc == 0
    _same(c, out.arrays(), _model("threshold"), "inputs %s, outputs %s" % (in_sides, out_sides))


# ------------------------------------------------------------------------------------- the index is usable
@pytest.mark.parametrize("name", ["threshold", "clip", "many_big", "high_bits-100003"])
def test_gpu_built_index_maps_like_the_models(kmm, oracle, name):
    """DeviceIndex.from_index on the GPU-built arrays; every distinct key once, plus key + 1 and key - 1 (wrapping), through
    map_kmers at max_index_lookup_frequency 64, 65 534 and 65 535 on the direct path and, where the index has one, the radix
    path, and through in_index — equal to the oracle's lookups on the MODEL's index.  Node ids are folded into 0 .. 4095 on
    both sides, each from its own nodes array (which the route tests compare in full).  A heavy key is queried once: its
    bucket is walked per query on the direct path."""
    c = bc.build(name)
    got, _ = _host_route(kmm, name)
    built, modelled = bc.as_index(got, NODE_MASK), bc.as_index(_model(name), NODE_MASK)
    keys = np.unique(c.kmers)
    q = np.concatenate([keys, keys + np.uint64(1), keys - np.uint64(1)])
    q = q[np.random.default_rng(7).permutation(q.shape[0])]
    expect_in = oracle.in_index(modelled, q)
    assert expect_in.sum() >= keys.shape[0]
    with kmm.DeviceIndex.from_index(built, NODE_MASK) as dev:
        paths = (1, 2) if dev.get_param("radix_available") == 1 else (1,)
        print("\n%-24s %d queries, paths %s (radix_unavailable_reason %d)" % (name, q.shape[0], paths, dev.get_param("radix_unavailable_reason")))
        for mf in (64, 65_534, 65_535):
            expect = oracle.map_kmers(modelled, NODE_MASK, q, mf)
            for path in paths:
                dev.set_param("path", path)
                dev.reset()
                before = dev.get_param("radix_batches")
                dev.map_kmers(q, mf)
                assert np.array_equal(dev.get_node_counts(), expect), (name, mf, path)
                assert (dev.get_param("radix_batches") > before) == (path == 2), (name, mf, path)
        dev.set_param("path", 1)
        assert np.array_equal(dev.in_index(q), expect_in)
    if name == "clip":      # the filter sees the clip: 65 534 lets exactly the 65 534-run through, 65 535 all four
        heavy = np.array([k for k, (f, n) in c.expected.items() if n > 1000], dtype=np.uint64)
        counts = [int(oracle.map_kmers(modelled, NODE_MASK, heavy, mf).sum()) for mf in (64, 65_534, 65_535)]
        assert counts == [0, 65_534, 65_534 + 65_535 + 65_536 + 65_537]


# ------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_builder_usable(kmm):
    """n = -1, modulo 0, modulo 2^31 and a NULL hashes_to_index return KMM_ERR_INVALID_ARG from the entry point; node ids
    outside int32 and arrays of different lengths raise in engine.build_index; a correct build succeeds after each."""
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    c = bc.build("one_bucket-65")
    want = _model("one_bucket-65")
    km, nd = c.kmers, c.nodes.astype(np.int32)
    n = km.shape[0]
    p = lambda a: ctypes.c_void_p(a.ctypes.data)

    def good():
        _same(c, kmm.build_index(c.kmers, c.nodes, c.modulo), want, "after a refusal")

    def outputs(M):
        return [np.full(max(M, 1), -1, dtype=np.int32), np.full(max(M, 1), -1, dtype=np.int32), np.zeros(n, np.uint64), np.zeros(n, np.int32),
                np.zeros(n, np.uint16)]

    for bad_n, bad_M in ((-1, 1), (n, 0), (n, 2 ** 31)):
        out = outputs(1)          # (never written: the refusal comes before any work)
        assert L.kmm_build_index(0, p(km), p(nd), bad_n, bad_M, *[p(a) for a in out]) == _lib.KMM_ERR_INVALID_ARG, (bad_n, bad_M)
        assert out[0].tolist() == [-1] and out[1].tolist() == [-1] and not out[2].any()
        assert L.kmm_last_error()
        good()
    out = outputs(1)
    assert L.kmm_build_index(0, p(km), p(nd), n, 1, None, *[p(a) for a in out[1:]]) == _lib.KMM_ERR_INVALID_ARG
    assert out[1].tolist() == [-1]
    good()
    with pytest.raises(ValueError):
        _lib.check(L.kmm_build_index(0, p(km), p(nd), n, 0, *[p(a) for a in outputs(1)]))
    for nodes in (np.where(np.arange(n) == 3, -1, c.nodes), np.where(np.arange(n) == 3, 2 ** 31, c.nodes)):
        with pytest.raises(ValueError, match="int32"):
            kmm.build_index(c.kmers, nodes, c.modulo)
        good()
    for kmers, nodes in ((c.kmers, c.nodes[:-1]), (c.kmers[:-1], c.nodes), (c.kmers.reshape(5, 13), c.nodes.reshape(5, 13))):
        with pytest.raises(ValueError, match="same length"):
            kmm.build_index(kmers, nodes, c.modulo)
        good()


# ------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("name", ["many_big", "clip"])
def test_two_builds_are_identical(kmm, name):
    """The scatter fills a bucket in arrival order (atomic cursors), which differs from run to run; only the ranking by
    original position makes the result reproducible.  Two more builds equal the first, array for array."""
    c = bc.build(name)
    first, _ = _host_route(kmm, name)
    for i in range(2):
        _same(c, kmm.build_index(c.kmers, c.nodes, c.modulo), first, "build %d" % (i + 2))
