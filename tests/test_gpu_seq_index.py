"""GPU tier of the sequence index builder: kmm_seq_index_build (csrc/kmm_seqindex.hpp, driver in csrc/kmm_seqindex_host.hpp) on
the catalogue of tests/seq_index_cases.py against its model, which shares no structure with the kernels
(tests/test_seq_index_on_the_cpu.py holds the catalogue to its claims and the model to the oracle).

Routes: host arrays through engine.index_from_sequences; device tensors through the same; the raw entry points with buffers
this test owns, pre-filled with 0xA5 bytes and followed by 64 guard bytes, inputs and outputs on different sides.  Every case
runs on every route; nothing is left out.  The built index is then used (read_hits, map), the errors carry the contract's code
and number, and `kmer_mapper index` feeds `select-reads` end to end.  Bit-exact: this is integer work."""
import ctypes
import gzip
import os

import numpy as np
import pytest

from tests import ambiguous_cases as ac
from tests import build_cases as bc
from tests import seq_index_cases as sc

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 64
DTYPES = (np.int32, np.int32, np.uint64, np.int32, np.uint16)
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def _as_index(got):
    """The five arrays of a route, on the host, in the order of the model."""
    out = []
    for a, dt in zip(got[:5], DTYPES):
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        out.append(a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize and a.dtype != dt else a)
    return bc.Index(*out)


def _same(name, got, m, what):
    got = _as_index(got)
    assert tuple(a.dtype for a in got) == tuple(np.dtype(d) for d in DTYPES), (what, [a.dtype for a in got])
    for f, g, w in zip(bc.Index._fields, got, m.index):
        assert g.shape == w.shape, (name, what, f, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = int(np.flatnonzero(g != w)[0])
            raise AssertionError("%s, %s: %s differs first at %d: got %r, the model has %r" % (name, what, f, at, g[at], w[at]))


def _build(kmm, case, device=False, **more):
    info = {}
    bases, offsets, nodes, lut = case.bases, case.offsets, case.nodes, case.lut
    if device:
        import torch
        bases = torch.from_numpy(np.array(bases)).cuda()
        offsets = torch.from_numpy(np.array(offsets)).cuda()
        nodes = None if nodes is None else torch.from_numpy(np.array(nodes)).cuda()
        lut = None if lut is None else torch.from_numpy(np.array(lut)).cuda()
    got = kmm.index_from_sequences(bases, offsets, k=case.k, nodes=nodes, lut=lut, both_strands=case.both, modulo=case.modulo,
                                   info=info, _flags=case.flags, **more)
    return got, info


# ------------------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize("name", sc.CASES)
def test_host_arrays_give_the_models_index(kmm, name):
    case, m = sc.build(name), sc.model(name)
    got, info = _build(kmm, case)
    assert all(isinstance(a, np.ndarray) for a in got[:5])
    assert (got[5], info["modulo"]) == (m.modulo, m.modulo)
    assert (info["n_windows"], info["n_pairs"], info["n_entries"]) == (m.n_windows, m.n_pairs, m.n_entries)
    _same(name, got, m, "host arrays")
    if case.modulo == 0:
        assert got[5] == kmm.seq_index_modulo(m.n_entries)


@pytest.mark.parametrize("name", sc.CASES)
def test_device_tensors_give_the_models_index(kmm, name):
    case, m = sc.build(name), sc.model(name)
    got, info = _build(kmm, case, device=True)
    assert all(a.is_cuda for a in got[:5]) and got[5] == m.modulo
    assert (info["n_windows"], info["n_pairs"], info["n_entries"]) == (m.n_windows, m.n_pairs, m.n_entries)
    _same(name, got, m, "device tensors")


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
        return [P(b.ctypes.data if isinstance(b, np.ndarray) else b.data_ptr()) for b in self.bufs]

    def arrays(self):
        out = []
        for b, nbytes, dt in zip(self.bufs, self.sizes, DTYPES):
            raw = b if isinstance(b, np.ndarray) else b.cpu().numpy()
            assert (raw[nbytes:] == SENTINEL).all(), "bytes behind an output array were written"
            out.append(raw[:nbytes].copy().view(dt))
        return out


def _raw(case, in_sides="hhhh", bases=None, offsets=None, nodes="case", k=None, lut="case"):
    """kmm_seq_index_build through the C entry point, every input on the side asked for (bases, offsets, nodes, lut).  Returns
    (rc, message, handle or None, what must stay alive)."""
    import torch
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    bases = case.bases if bases is None else bases
    offsets = case.offsets if offsets is None else offsets
    nodes = case.nodes if isinstance(nodes, str) else nodes
    lut = case.lut if isinstance(lut, str) else lut
    keep, ptrs = [], []
    for a, side in zip((bases, offsets, nodes, lut), in_sides):
        if a is None or a.size == 0:
            keep.append(None)
            ptrs.append(None if a is None else P(np.zeros(1, dtype=a.dtype).ctypes.data))
            continue
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a.copy()).cuda() if side == "d" else a
        keep.append(t)
        ptrs.append(P(t.data_ptr() if side == "d" else t.ctypes.data))
    torch.cuda.synchronize()
    h = P()
    flags = (1 if case.both else 0) | case.flags
    rc = L.kmm_seq_index_build(0, ptrs[0], ptrs[1], offsets.shape[0] - 1, ptrs[2], case.k if k is None else k, ptrs[3], flags,
                               case.modulo, ctypes.byref(h))
    msg = L.kmm_last_error().decode() if rc else ""
    assert (h.value is not None) == (rc == 0), "an object exists exactly when the build succeeded"
    return rc, msg, (h if rc == 0 else None), keep


@pytest.mark.parametrize("name", sc.CASES)
def test_the_raw_entry_points_write_exactly_their_arrays(kmm, name):
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    case, m = sc.build(name), sc.model(name)
    i = sc.CASES.index(name)
    in_sides = "".join("dh"[(i >> b) & 1] for b in range(4))
    out_sides = "".join("hd"[(i + b) & 1] for b in range(5))
    rc, msg, h, keep = _raw(case, in_sides)
    assert rc == 0, msg
    try:
        n, M, nw, npairs = ctypes.c_int64(-1), ctypes.c_uint64(0), ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert L.kmm_seq_index_info(h, ctypes.byref(n), ctypes.byref(M), ctypes.byref(nw), ctypes.byref(npairs)) == 0
        assert (n.value, M.value, nw.value, npairs.value) == (m.n_entries, m.modulo, m.n_windows, m.n_pairs)
        out = _Out(m.n_entries, m.modulo, out_sides)
        assert L.kmm_seq_index_fetch(h, *out.pointers()) == 0, L.kmm_last_error()
        _same(name, out.arrays(), m, "raw, inputs %s outputs %s" % (in_sides, out_sides))
        again = _Out(m.n_entries, m.modulo, out_sides[::-1])             # a second fetch gives the same
        assert L.kmm_seq_index_fetch(h, *again.pointers()) == 0
        _same(name, again.arrays(), m, "raw, second fetch")
    finally:
        L.kmm_seq_index_destroy(h)


@pytest.mark.parametrize("name", sc.DETERMINISM)
def test_three_builds_give_the_same_bytes(kmm, name):
    case = sc.build(name)
    runs = [[np.asarray(a).tobytes() for a in _build(kmm, case)[0][:5]] for _ in range(3)]
    assert runs[0] == runs[1] == runs[2]


# ---------------------------------------------------------------------------------------------------- the index is used
def _reads_from(case, rng, n, length):
    """n reads of `length` bases cut from the sequences, clear of breaks and of sequence ends; (bases, offsets)."""
    brk = ac.break_mask(case.bases, sc.table_of(case))
    reads = []
    lens = np.diff(case.offsets)
    seqs = np.flatnonzero(lens >= length)
    while len(reads) < n:
        s = int(rng.choice(seqs))
        a = int(case.offsets[s] + rng.integers(0, lens[s] - length + 1))
        if not brk[a:a + length].any():
            reads.append(np.array(case.bases[a:a + length]))
    return np.concatenate(reads), np.arange(n + 1, dtype=np.int64) * length


def _revcomp_reads(bases, n, length):
    comp = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
        comp[a] = b
    return np.ascontiguousarray(comp[bases.reshape(n, length)[:, ::-1]].reshape(-1))


def _index_object(got):
    from kmer_mapper_amd.kmer_index import KmerIndex
    h2i, nk, ko, no, fo, M = got
    return KmerIndex(h2i, nk, no, ko, M, fo)


@pytest.mark.parametrize("name", ["n_runs", "shared", "explicit_nodes", "seq_ends_at_tile_edge", "iupac"])
def test_reads_cut_from_the_sequences_hit_with_every_window(kmm, name):
    case = sc.build(name)
    rng = np.random.default_rng(11)
    n, length = 64, case.k + 17
    bases, offs = _reads_from(case, rng, n, length)
    with kmm.DeviceIndex.from_index(_index_object(_build(kmm, case)[0])) as dev:
        hits, wins = dev.read_hits(bases, offs, k=case.k, max_index_lookup_frequency=65535, lut=case.lut, windows=True)
    assert np.array_equal(wins, np.full(n, length - case.k + 1, dtype=np.uint32)) and np.array_equal(hits, wins)


def test_reverse_complements_hit_without_r_exactly_when_both_strands_were_built(kmm):
    case = sc.build("no_contention_k31")
    rng = np.random.default_rng(12)
    n, length = 64, 80
    bases, offs = _reads_from(case, rng, n, length)
    rc = _revcomp_reads(bases, n, length)
    for both in (False, True):
        got = kmm.index_from_sequences(case.bases, case.offsets, k=case.k, both_strands=both)
        with kmm.DeviceIndex.from_index(_index_object(got)) as dev:
            fwd, wins = dev.read_hits(bases, offs, k=case.k, max_index_lookup_frequency=65535, windows=True)
            rev = dev.read_hits(rc, offs, k=case.k, max_index_lookup_frequency=65535)
            rev_r = dev.read_hits(rc, offs, k=case.k, max_index_lookup_frequency=65535, also_revcomp=True)
        assert np.array_equal(fwd, wins) and np.array_equal(rev_r, wins)
        assert np.array_equal(rev, wins) == both and (both or not rev.any())


@pytest.mark.parametrize("name", ["explicit_nodes", "shared", "palindromes"])
def test_random_reads_hit_and_map_as_the_oracle_says_on_the_models_arrays(kmm, oracle, name):
    case, m = sc.build(name), sc.model(name)
    rng = np.random.default_rng(13)
    n, length = 96, 70
    bases = sc.ACGT[rng.integers(0, 4, size=n * length)]
    cut, _ = _reads_from(case, rng, n // 2, 40)
    bases.reshape(n, length)[: n // 2, 10:50] = cut.reshape(n // 2, 40)            # half of the reads carry a piece of a sequence
    offs = np.arange(n + 1, dtype=np.int64) * length
    model_index = bc.as_index(m.index)
    member = oracle.in_index(model_index, oracle.extract(bases, offs, case.k))
    want_hits = member.reshape(n, length - case.k + 1).sum(axis=1).astype(np.uint32)
    assert 0 < want_hits.sum() < member.shape[0]
    max_node = int(m.index.nodes.max())
    want_counts, _ = oracle.map_reads(model_index, max_node, bases, offs, case.k)
    with kmm.DeviceIndex.from_index(_index_object(_build(kmm, case)[0]), max_node) as dev:
        hits = dev.read_hits(bases, offs, k=case.k, max_index_lookup_frequency=65535)
        dev.map_reads(bases, offs, case.k)
        counts = dev.get_node_counts()
    assert np.array_equal(hits, want_hits)
    assert np.array_equal(counts, want_counts)


# -------------------------------------------------------------------------------------------------------------- errors
def _then_a_correct_build_succeeds(kmm):
    case, m = sc.build("hand"), sc.model("hand")
    got, info = _build(kmm, case)
    _same("hand", got, m, "a build after an error")
    for f in bc.Index._fields:
        assert np.array_equal(getattr(_as_index(got), f), getattr(sc.HAND, f)), f


def test_the_hand_case_gives_the_arrays_written_out_by_hand(kmm):
    _then_a_correct_build_succeeds(kmm)


def test_errors_carry_the_code_and_the_number_and_leave_nothing_behind(kmm):
    from kmer_mapper_amd import _lib
    case = sc.build("short_sequences")
    INVALID_ARG, INVALID_BASE = _lib.KMM_ERR_INVALID_ARG, _lib.KMM_ERR_INVALID_BASE
    bad_base = np.array(case.bases)
    bad_base[777] = ord("X")                                   # table entry 0xFF
    down = np.array(case.offsets)
    down[5], down[6] = down[6], down[5] - 1                    # offsets[6] < offsets[5]
    assert down[6] < down[5]
    neg = np.arange(case.offsets.shape[0] - 1, dtype=np.int32)
    neg[9] = -4
    not_zero = np.array(case.offsets)
    not_zero[0] = 3
    for sides in ("hhhh", "dddd"):
        for kwargs, code, words in ((dict(bases=bad_base), INVALID_BASE, ("offset 777",)),
                                    (dict(offsets=down), INVALID_ARG, ("non-decreasing", "sequence 5")),
                                    (dict(nodes=neg), INVALID_ARG, ("seq_nodes[9]", "negative")),
                                    (dict(offsets=not_zero), INVALID_ARG, ("seq_offsets[0]", "got 3")),
                                    (dict(k=0), INVALID_ARG, ("k=0",)),
                                    (dict(k=32), INVALID_ARG, ("k=32",)),
                                    (dict(k=1, lut=sc.SKIP), INVALID_ARG, ("k=1", "break"))):
            rc, msg, h, _ = _raw(case, sides, **kwargs)
            assert rc == code and h is None, (sides, kwargs.keys(), rc, msg)
            assert all(w in msg for w in words), (sides, msg)
            _then_a_correct_build_succeeds(kmm)
    with pytest.raises(ValueError, match="offset 777"):
        kmm.index_from_sequences(bad_base, case.offsets, k=case.k)


def test_a_null_output_in_fetch_is_refused_and_the_object_stays_usable(kmm):
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    case, m = sc.build("explicit_nodes"), sc.model("explicit_nodes")
    rc, msg, h, keep = _raw(case)
    assert rc == 0, msg
    try:
        out = _Out(m.n_entries, m.modulo, "hhhhh")
        for missing in range(5):
            ptrs = out.pointers()
            ptrs[missing] = None
            assert L.kmm_seq_index_fetch(h, *ptrs) == _lib.KMM_ERR_INVALID_ARG
            assert "NULL" in L.kmm_last_error().decode() and str(m.modulo if missing < 2 else m.n_entries) in L.kmm_last_error().decode()
        assert all((b == SENTINEL).all() for b in out.bufs), "a refused fetch wrote"
        assert L.kmm_seq_index_fetch(h, *out.pointers()) == 0
        _same("explicit_nodes", out.arrays(), m, "fetch after refusals")
        assert L.kmm_seq_index_info(None, None, None, None, None) == _lib.KMM_ERR_INVALID_ARG
    finally:
        L.kmm_seq_index_destroy(h)
    L.kmm_seq_index_destroy(None)
    _then_a_correct_build_succeeds(kmm)


# ---------------------------------------------------------------------------------------------------------- end to end
def _wrap(seq, width, eol):
    return eol.join(seq[i:i + width] for i in range(0, len(seq), width)) + eol


def test_kmer_mapper_index_then_select_reads(kmm, tmp_path):
    """A PhiX-sized reference as a wrapped, CRLF, partly lower-case, gzip-compressed FASTA with N runs -> `kmer_mapper index` ->
    `select-reads -i`: of a FASTQ whose reads are half drawn from it (either strand) and half random, exactly the drawn ones come out."""
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    from kmer_mapper_amd.kmer_index import KmerIndex
    rng = np.random.default_rng(14)
    seqs = [bytearray(sc.ACGT[rng.integers(0, 4, size=n)].tobytes()) for n in (5386, 3100, 2200)]
    seqs[2][400:900] = seqs[0][1000:1500]                                 # a segment two sequences share
    seqs[0][2000:2150] = b"N" * 150
    seqs[1][0:40] = b"N" * 40
    seqs[1][1500] = ord("n")
    seqs[0][3000:3300] = bytes(seqs[0][3000:3300]).lower()
    names = ["phiX_like", "second|seq", "third"]
    text = b"".join(b">" + nm.encode() + (b" description %d" % i) + b"\r\n" + _wrap(bytes(s), 70, b"\r\n")
                    for i, (nm, s) in enumerate(zip(names, seqs)))
    fa = str(tmp_path / "ref.fa.gz")
    with gzip.open(fa, "wb") as f:
        f.write(text)
    n_reads, length = 200, 100
    drawn = np.zeros(n_reads, dtype=bool)
    drawn[rng.permutation(n_reads)[: n_reads // 2]] = True
    records = []
    for i in range(n_reads):
        if drawn[i]:
            while True:
                s = seqs[int(rng.integers(0, 3))]
                a = int(rng.integers(0, len(s) - length + 1))
                read = bytes(s[a:a + length]).upper()
                if b"N" not in read:
                    break
            if i % 4 == 0:
                read = bytes(_revcomp_reads(np.frombuffer(read, dtype=np.uint8), 1, length))
        else:
            read = sc.ACGT[rng.integers(0, 4, size=length)].tobytes()
        records.append(b"@read%d\n%s\n+\n%s\n" % (i, read, b"I" * length))
    fq = str(tmp_path / "reads.fq")
    open(fq, "wb").write(b"".join(records))
    want = b"".join(r for r, d in zip(records, drawn) if d)

    npz, names_out = str(tmp_path / "ref.npz"), str(tmp_path / "names.txt")
    run_argument_parser(["index", "-f", fa, "-k", "31", "-o", npz, "--both-strands", "--names-output", names_out])
    assert open(names_out).read().split("\n") == names + [""]
    index = KmerIndex.from_file(npz)
    assert sorted(set(index._nodes.tolist())) == [0, 1, 2] and int(index._frequencies.max()) == 2
    assert 0 not in index._kmers.tolist()                                     # the N runs did not become poly-A
    out = str(tmp_path / "kept.fq")
    seen, kept = run_argument_parser(["select-reads", "-i", npz, "-f", fq, "-k", "31", "-o", out])
    assert (seen, kept) == (n_reads, n_reads // 2)
    assert open(out, "rb").read() == want

    npz1, out1 = str(tmp_path / "ref1.npz"), str(tmp_path / "kept1.fq")
    run_argument_parser(["index", "-f", fa, "-k", "31", "-o", npz1, "--both-strands", "--single-node"])
    single = KmerIndex.from_file(npz1)
    assert set(single._nodes.tolist()) == {0} and single._kmers.shape[0] < index._kmers.shape[0]
    assert os.path.getsize(npz1) < os.path.getsize(npz)
    assert run_argument_parser(["select-reads", "-i", npz1, "-f", fq, "-k", "31", "-o", out1]) == (n_reads, n_reads // 2)
    assert open(out1, "rb").read() == want


def test_an_index_without_entries_is_refused_by_the_command(kmm, tmp_path):
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    fa = tmp_path / "short.fa"
    fa.write_bytes(b">a\nACGTACGT\n>b\nNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNN\n")
    out = str(tmp_path / "o.npz")
    with pytest.raises(ValueError, match="without entries"):
        run_argument_parser(["index", "-f", str(fa), "-k", "31", "-o", out])
    assert not os.path.exists(out)
