"""GPU tests of kmm_map_reads_qual (include/kmm.h): flat reads with their quality bytes as a second array, the
floor "min_base_quality" applied to quals[p] < qual_base + Q.  The node counts equal the oracle's on the reads split at their
masked bases, kmm_get_stats' lookups the windows that survive, and "quality_masked_bases" the numpy count
(tests/flat_quality_cases.py, held to their conditions by tests/test_flat_quality_cases_on_the_cpu.py)."""
import types

import numpy as np
import pytest

from tests import flat_quality_cases as fq
from tests import quality_cases as qc

pytestmark = pytest.mark.gpu

BOTH_DOORS = ("span_edges", "tile_edges", "ragged_1_to_400", "degenerate_reads", "all_41_values")


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def lut():
    from kmer_mapper_amd.util import ambiguous_skip_lut
    return ambiguous_skip_lut()


def _answers(oracle, c, q=None):
    """The oracle on the case's reads split at the bases the floor q (default: the case's own) and the table kill."""
    index, mx = qc.index_for(c["k"]), qc.index_for(c["k"]).max_node_id()
    sb, so = qc.split_at_mask(c["bases"], c["offsets"], fq.dead_mask(c, q))
    split, n = oracle.map_reads(index, mx, sb, so, c["k"])
    split_rc, _ = oracle.map_reads(index, mx, sb, so, c["k"], also_revcomp=True)
    for a in (split, split_rc):
        a.setflags(write=False)
    return dict(split=split, split_rc=split_rc, n_windows=n, n_masked=int(fq.low_mask(c, q).sum()))


_EXPECT = {}


@pytest.fixture(scope="module")
def expect(oracle):
    """name -> the case, its index and the oracle's answers (computed once, never changed)."""
    def get(name):
        if name not in _EXPECT:
            c = dict(fq.build(name))
            c.update(_answers(oracle, c), index=qc.index_for(c["k"]), n_reads=len(c["offsets"]) - 1)
            c["mx"] = c["index"].max_node_id()
            off = _answers(oracle, c, q=0)
            c["unsplit"], c["unsplit_rc"], c["n_all"] = off["split"], off["split_rc"], off["n_windows"]
            _EXPECT[name] = c
        return _EXPECT[name]
    return get


@pytest.fixture(scope="module")
def devs(kmm):
    """One handle per k, shared by the tests of this module."""
    open_ = {}

    def get(case):
        if case["k"] not in open_:
            open_[case["k"]] = kmm.DeviceIndex.from_index(case["index"], case["mx"])
            assert open_[case["k"]].get_param("radix_available")
        return open_[case["k"]]
    yield get
    for d in open_.values():
        d.close()


def _run(dev, q, call, path=0):
    """(node counts, lookups, masked bases) of map call(s) on a clean handle with the floor q."""
    dev.reset()
    dev.get_stats(reset=True)
    dev.set_param("min_base_quality", q)
    dev.set_param("path", path)
    try:
        call()
        return dev.get_node_counts().copy(), dev.get_stats()[0], dev.get_param("quality_masked_bases")
    finally:
        dev.set_param("min_base_quality", 0)
        dev.set_param("path", 0)


def _check(dev, case, lut, call, what, want=None, q=None, **kw):
    """call(lut, also_revcomp) against the oracle on the split reads (`want`: other answers than the case's own), forward
    and with reverse complements."""
    table = lut if case["use_lut"] else None
    want = case if want is None else want
    for rc in (False, True):
        got, lookups, masked = _run(dev, case["q"] if q is None else q, lambda: call(table, rc), **kw)
        assert np.array_equal(got, want["split_rc" if rc else "split"]), (case["name"], what, rc)
        assert lookups == (2 if rc else 1) * want["n_windows"], (case["name"], what, rc, "lookups")
        assert masked == want["n_masked"], (case["name"], what, rc, "quality_masked_bases")


def _shifted(t, by):
    """The tensor's bytes again, in HBM at an address that is `by` bytes past a 16-byte boundary."""
    import torch
    buf = torch.empty(t.shape[0] + 16 + by, dtype=torch.uint8, device="cuda")
    start = (-buf.data_ptr()) % 16 + by
    out = buf[start:start + t.shape[0]]
    out.copy_(t)
    assert out.data_ptr() % 16 == by
    return out


def _ragged(dev, case, b, qu, o):
    return lambda t, rc: dev.map_reads(b, o, case["k"], also_revcomp=rc, lut=t, qualities=qu, qual_base=case["qual_base"])


def _uniform(dev, case, b, qu):
    n, length = case["n_reads"], int(case["offsets"][1])
    return lambda t, rc: dev.map_reads_uniform(b, n, length, case["k"], also_revcomp=rc, lut=t, qualities=qu,
                                               qual_base=case["qual_base"])


@pytest.mark.parametrize("name", fq.CASES)
def test_ragged_call(kmm, expect, devs, lut, name):
    """kmm_map_reads_qual with offsets: from host arrays, device tensors, device tensors at odd addresses (bases one byte past
    a 16-byte boundary, quals three: the unaligned loads of two kernels), one array on the host and the other on the device,
    and with the path forced either way — each batch counted on the path asked for."""
    import torch
    case = expect(name)
    dev = devs(case)
    bases, quals, offsets = case["bases"], case["quals"], case["offsets"]
    d_bases, d_quals, d_offsets = (torch.from_numpy(np.array(a)).cuda() for a in (bases, quals, offsets))
    _check(dev, case, lut, _ragged(dev, case, bases, quals, offsets), "host")
    _check(dev, case, lut, _ragged(dev, case, d_bases, d_quals, d_offsets), "device")
    _check(dev, case, lut, _ragged(dev, case, _shifted(d_bases, 1), _shifted(d_quals, 3), d_offsets), "odd addresses")
    _check(dev, case, lut, _ragged(dev, case, bases, d_quals, offsets), "quals on the device")
    _check(dev, case, lut, _ragged(dev, case, d_bases, quals, d_offsets), "bases on the device")
    for path, moves, stays in ((1, "direct_batches", "radix_batches"), (2, "radix_batches", "direct_batches")):
        before = dev.get_param(moves), dev.get_param(stays)
        _check(dev, case, lut, _ragged(dev, case, d_bases, d_quals, d_offsets), "path %d" % path, path=path)
        assert (dev.get_param(moves), dev.get_param(stays)) == (before[0] + 2, before[1]), (name, path)


@pytest.mark.parametrize("name", list(qc.UNIFORM) + ["span_edges"])
def test_uniform_call(kmm, expect, devs, lut, name):
    """read_offsets NULL: the counts of the ragged call, on both paths, and no batch takes the uniform front end while Q > 0."""
    import torch
    case = expect(name)
    dev = devs(case)
    assert qc.is_uniform(case["offsets"])
    d_bases, d_quals = (torch.from_numpy(np.array(a)).cuda() for a in (case["bases"], case["quals"]))
    before = dev.get_param("flat_uniform_batches")
    _check(dev, case, lut, _uniform(dev, case, case["bases"], case["quals"]), "uniform, host")
    _check(dev, case, lut, _uniform(dev, case, d_bases, d_quals), "uniform, device")
    _check(dev, case, lut, _uniform(dev, case, _shifted(d_bases, 1), _shifted(d_quals, 3)), "uniform, odd addresses")
    for path in (1, 2):
        _check(dev, case, lut, _uniform(dev, case, d_bases, d_quals), "uniform, path %d" % path, path=path)
    assert dev.get_param("flat_uniform_batches") == before


@pytest.mark.parametrize("name", BOTH_DOORS)
def test_the_same_reads_through_both_doors(kmm, expect, devs, lut, oracle, name):
    """kmm_map_records on the FASTQ text and kmm_map_reads_qual on the arrays: identical counts, lookups and masked bases, at
    the case's floor and at the next one up (the cases plant bytes exactly at the floor: they die there)."""
    case = expect(name)
    dev = devs(case)
    k = case["k"]
    text = np.frombuffer(qc.fastq_text(case["bases"], case["quals"], case["offsets"])[0], np.uint8)
    for q in (case["q"], case["q"] + 1):
        want = case if q == case["q"] else _answers(oracle, case, q)
        for rc in (False, True):
            records = _run(dev, q, lambda: dev.map_records(text, fmt=4, k=k, also_revcomp=rc))
            flat = _run(dev, q, lambda: dev.map_reads(case["bases"], case["offsets"], k, also_revcomp=rc, qualities=case["quals"]))
            assert np.array_equal(records[0], flat[0]) and records[1:] == flat[1:], (name, q, rc)
            assert np.array_equal(flat[0], want["split_rc" if rc else "split"]) and flat[2] == want["n_masked"], (name, q, rc)
        assert (want["n_masked"] > case["n_masked"]) == (q > case["q"])


def test_raw_phred(kmm, expect, devs, lut):
    """qual_base 0: the same reads with quals - 33 give what Phred+33 gives; BAM's 0xFF is alive at every floor."""
    ref, raw, absent = expect("all_41_values"), expect("raw_phred"), expect("raw_phred-absent")
    assert np.array_equal(raw["split"], ref["split"]) and raw["n_masked"] == ref["n_masked"] and raw["n_windows"] == ref["n_windows"]
    dev = devs(raw)
    _check(dev, raw, lut, _ragged(dev, raw, raw["bases"], raw["quals"], raw["offsets"]), "raw phred", want=ref)
    n_absent = int((absent["quals"] == 0xFF).sum())
    assert absent["q"] == 93 and absent["n_masked"] == absent["quals"].shape[0] - n_absent and absent["n_windows"] > 0
    _check(dev, absent, lut, _ragged(dev, absent, absent["bases"], absent["quals"], absent["offsets"]), "0xFF at Q93")
    # the same bytes read as Phred+33 text at Q = 8: every byte below '!' + 8 = 41 is masked, 0xFF is above every floor
    got, _, masked = _run(dev, 8, lambda: dev.map_reads(absent["bases"], absent["offsets"], absent["k"], qualities=absent["quals"]))
    assert masked == absent["n_masked"] and np.array_equal(got, absent["split"])


@pytest.mark.parametrize("name", ["tile_edges", "ragged_1_to_400"])
def test_floor_off_is_map_reads(kmm, expect, devs, name):
    """Q = 0: qualities=None and any qualities give the oracle's counts on the unsplit reads, nothing is masked, and the
    handle's counters move as under map_reads / map_reads_uniform on the same input."""
    import torch
    case = expect(name)
    dev = devs(case)
    k, bases, offsets, quals = case["k"], case["bases"], case["offsets"], case["quals"]
    d_bases = torch.from_numpy(np.array(bases)).cuda()
    names = ("direct_batches", "radix_batches", "flat_uniform_batches", "host_packed_calls")

    def moved(call, path):
        before = [dev.get_param(n) for n in names]
        got = _run(dev, 0, call, path=path)
        return got, [dev.get_param(n) - b for n, b in zip(names, before)]
    garbage = np.zeros_like(quals)                                   # all low at any floor: not read at Q = 0
    for path in (1, 2):
        for rc in (False, True):
            want = case["unsplit_rc" if rc else "unsplit"]
            plain, d_plain = moved(lambda: dev.map_reads(bases, offsets, k, also_revcomp=rc), path)
            for qu in (quals, garbage):
                (got, lookups, masked), d = moved(lambda: dev.map_reads(bases, offsets, k, also_revcomp=rc, qualities=qu), path)
                assert np.array_equal(got, want) and lookups == (2 if rc else 1) * case["n_all"] and masked == 0
                assert np.array_equal(got, plain[0]) and lookups == plain[1] and d == d_plain, (name, path, rc)
        if name in qc.UNIFORM:
            n = case["n_reads"]
            plain, d_plain = moved(lambda: dev.map_reads_uniform(d_bases, n, qc.L, k), path)
            (got, lookups, masked), d = moved(lambda: dev.map_reads_uniform(d_bases, n, qc.L, k, qualities=garbage), path)
            assert np.array_equal(got, case["unsplit"]) and lookups == case["n_all"] and masked == 0 and d == d_plain
            (got, _, masked), d = moved(lambda: dev.map_reads_uniform(d_bases, n, qc.L, k, qualities=quals), path)
            assert np.array_equal(got, case["unsplit"]) and masked == 0 and d == d_plain


def test_the_host_packer_serves_q0_and_is_bypassed_above(kmm, expect):
    """host_pack_threads 16 and a host-resident batch that qualifies for the packer: it packs with the floor off — with or
    without qualities, as under map_reads, reads of one length on the uniform front end ("flat_uniform_batches") — and is not
    used with it on, where reads of one length take the ragged front end."""
    case = expect("tile_edges")
    k, bases, offsets, quals, n = case["k"], case["bases"], case["offsets"], case["quals"], case["n_reads"]
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.set_param("host_pack_threads", 16)
        dev.set_param("radix_min_units", 1)
        for uniform, call in ((0, lambda qu: dev.map_reads(bases, offsets, k, qualities=qu)),
                              (1, lambda qu: dev.map_reads_uniform(bases, n, qc.L, k, qualities=qu))):
            before, before_uniform = dev.get_param("host_packed_calls"), dev.get_param("flat_uniform_batches")
            got, _, masked = _run(dev, 0, lambda: call(None))
            assert np.array_equal(got, case["unsplit"]) and dev.get_param("host_packed_calls") == before + 1
            got, _, masked = _run(dev, 0, lambda: call(quals))
            assert np.array_equal(got, case["unsplit"]) and masked == 0 and dev.get_param("host_packed_calls") == before + 2
            got, lookups, masked = _run(dev, 20, lambda: call(quals))
            assert np.array_equal(got, case["split"]) and masked == case["n_masked"] and lookups == case["n_windows"]
            assert dev.get_param("host_packed_calls") == before + 2
            assert dev.get_param("flat_uniform_batches") == before_uniform + 2 * uniform


@pytest.mark.parametrize("name", ["span_edges", "ragged_1_to_400", "with_skip_table"])
def test_two_calls_on_the_halves_equal_one(kmm, expect, devs, lut, name):
    """The batch cut at a read boundary (not a multiple of 32 positions): the counts, lookups and masked bases add up."""
    case = expect(name)
    dev = devs(case)
    bases, quals, offsets = case["bases"], case["quals"], case["offsets"]
    r = case["n_reads"] // 2 + 1
    cut = int(offsets[r])
    assert 0 < cut < offsets[-1] and cut % 32

    def halves(t, rc):
        dev.map_reads(bases[:cut], offsets[:r + 1], case["k"], also_revcomp=rc, lut=t, qualities=quals[:cut])
        dev.map_reads(bases[cut:], offsets[r:] - cut, case["k"], also_revcomp=rc, lut=t, qualities=quals[cut:])
    _check(dev, case, lut, halves, "two halves")
    for path in (1, 2):
        _check(dev, case, lut, halves, "two halves, path %d" % path, path=path)


@pytest.mark.parametrize("name", ["with_skip_table", "span_edges"])
def test_with_the_skip_table_a_base_is_dead_if_either_rule_kills_it(kmm, expect, devs, lut, oracle, name):
    """N under low bases and next to them: the oracle on the reads split at the union of both masks; the counter counts the
    low bases, those that are N too; each rule alone gives something else."""
    import torch
    base_case = expect(name)
    low = np.flatnonzero(fq.low_mask(base_case))
    spots = [int(low[1]), int(low[5]), int(low[3]) + 1, int(low[-2]) - 1, 16384 - 31 if name == "span_edges" else 77]
    case = fq.with_n(base_case, spots)
    assert fq.low_mask(case)[spots[:2]].all() and not fq.low_mask(case)[spots[2:]].all()
    want = _answers(oracle, case)
    assert want["n_masked"] == base_case["n_masked"] and want["n_windows"] < base_case["n_windows"]
    dev = devs(case)
    d_bases, d_quals, d_offsets = (torch.from_numpy(np.array(a)).cuda() for a in (case["bases"], case["quals"], case["offsets"]))
    _check(dev, case, lut, _ragged(dev, case, case["bases"], case["quals"], case["offsets"]), "table + floor, host", want=want)
    for path in (1, 2):
        _check(dev, case, lut, _ragged(dev, case, d_bases, d_quals, d_offsets), "table + floor, path %d" % path, want=want, path=path)
        if qc.is_uniform(case["offsets"]):
            _check(dev, case, lut, _uniform(dev, case, d_bases, d_quals), "table + floor, uniform, path %d" % path, want=want, path=path)
    # the table alone (Q = 0, nothing counted as masked), and the floor alone (N read as A)
    table_only = _answers(oracle, case, q=0)
    _check(dev, case, lut, _ragged(dev, case, d_bases, d_quals, d_offsets), "table alone", want=table_only, q=0)
    floor_only = _answers(oracle, dict(case, use_lut=False))
    _check(dev, dict(case, use_lut=False), lut, _ragged(dev, case, d_bases, d_quals, d_offsets), "floor alone", want=floor_only)
    assert table_only["n_windows"] > want["n_windows"] < floor_only["n_windows"] and table_only["n_masked"] == 0


def test_refusals_and_errors(kmm, expect, devs, lut):
    """KMM_ERR_INVALID_ARG with a message: no qualities under a floor, k = 1, a qual_base other than 0 and 33, arrays of
    different lengths (in Python, before the call); an invalid base under a low quality is reported at the synchronising call
    as under map_reads, and the handle maps a good batch after reset()."""
    import ctypes
    from kmer_mapper_amd import _lib
    case = expect("read_ends")
    dev = devs(case)
    k, bases, quals, offsets = case["k"], case["bases"], case["quals"], case["offsets"]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    n = case["n_reads"]
    dev.reset()
    dev.set_param("min_base_quality", 20)
    try:
        for offs_ptr, read_len in ((p(offsets), 0), (None, qc.L)):
            rc = _lib.lib().kmm_map_reads_qual(dev._h, p(bases), None, 33, offs_ptr, n, read_len, k, 1000, 0, None)
            assert rc == _lib.KMM_ERR_INVALID_ARG and b"quals is NULL" in _lib.lib().kmm_last_error()
        with pytest.raises(ValueError, match="k = 1 with min_base_quality 20"):
            dev.map_reads(bases, offsets, 1, qualities=quals)
        with pytest.raises(ValueError, match="k = 1 with min_base_quality 20"):
            dev.map_reads_uniform(bases, n, qc.L, 1, qualities=quals)
        for bad in (1, 64):
            with pytest.raises(ValueError, match="qual_base %d" % bad):
                dev.map_reads(bases, offsets, k, qualities=quals, qual_base=bad)
        with pytest.raises(ValueError, match="one quality byte per base"):
            dev.map_reads(bases, offsets, k, qualities=quals[:-1])
        with pytest.raises(ValueError, match="one quality byte per base"):
            dev.map_reads_uniform(bases, n, qc.L, k, qualities=np.concatenate([quals, quals[:1]]))
        assert not dev.get_node_counts().any()
    finally:
        dev.set_param("min_base_quality", 0)
    for bad in (1, 64):                                              # ... with the floor off as well
        with pytest.raises(ValueError, match="qual_base %d" % bad):
            dev.map_reads(bases, offsets, k, qualities=quals, qual_base=bad)
    dev.map_reads(bases, offsets, 1, qualities=quals)                # (k = 1 itself is fine without a floor)
    dev.reset()

    broken = np.array(bases)
    at = int(np.flatnonzero(fq.low_mask(case))[3])
    broken[at] = ord("X")
    for path in (1, 2):
        for table in (None, lut):
            dev.reset()
            dev.set_param("min_base_quality", 20)
            dev.set_param("path", path)
            try:
                dev.map_reads(broken, offsets, k, qualities=quals, lut=table)
                with pytest.raises(ValueError, match="offset %d of a mapped chunk is not a nucleotide" % at):
                    dev.get_node_counts()
                with pytest.raises(ValueError, match="offset %d of a mapped chunk is not a nucleotide" % at):
                    dev.get_node_counts()                             # (sticky until reset)
            finally:
                dev.reset()
                dev.set_param("min_base_quality", 0)
                dev.set_param("path", 0)
            _check(dev, case, lut, _ragged(dev, case, bases, quals, offsets), "after reset", path=path)


def test_an_index_without_a_radix_view_is_served_by_the_direct_path(kmm, expect, lut):
    """Two buckets share entries: "radix_available" 0.  kmm_map_records has no route for the floor there; flat reads have
    flat positions on both paths, so kmm_map_reads_qual maps them on the direct one."""
    case = expect("span_edges")
    index = case["index"]
    h2i, nk = index._hashes_to_index.copy(), index._n_kmers.copy()
    empty, full = np.flatnonzero(nk == 0)[:200], np.flatnonzero(nk > 0)[:200]
    h2i[empty], nk[empty] = h2i[full], nk[full]
    dup = types.SimpleNamespace(_hashes_to_index=h2i, _n_kmers=nk, _nodes=index._nodes, _kmers=index._kmers,
                                _frequencies=index._frequencies, _modulo=index._modulo)
    with kmm.DeviceIndex.from_index(dup, case["mx"]) as other:
        assert other.get_param("radix_available") == 0
        before = other.get_param("direct_batches")
        _check(other, case, lut, _ragged(other, case, case["bases"], case["quals"], case["offsets"]), "no radix view")
        _check(other, case, lut, _uniform(other, case, case["bases"], case["quals"]), "no radix view, uniform")
        assert other.get_param("direct_batches") == before + 4 and other.get_param("radix_batches") == 0
