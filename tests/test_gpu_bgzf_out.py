"""GPU tests of the BGZF writer (include/kmm.h COMPRESSED OUTPUT).  The operator kmm_bgzf_compress on every
case of tests/bgzf_out_cases.py, from host and from device bytes: the output inflates with zlib, member by member and whole, and
is byte for byte what the g++ build of the same header gave (tests/golden/bgzf_out_expected.json; the CPU tier keeps that file
current), also on a second call.  kmm_take_kept_bgzf against kmm_take_kept_records / kmm_take_kept_mates on a second handle fed
the same calls (the texts of tests/record_keep_cases.py).  The command line with --bgzf against the same command without it, and
the writer's output read back by the library's own inflater."""
import ctypes
import gzip
import hashlib

import numpy as np
import pytest

from tests import bgzf_out_cases as bc
from tests import record_keep_cases as rk
from tests.test_gpu_record_keep import _case, _keep_on, _map, _open, _rule

pytestmark = pytest.mark.gpu

CASES = bc.all_cases()
EOF_BLOCK = bc.EOF_BLOCK


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def golden():
    return bc.read_golden()


def _compress(src, n, out, cap):
    """kmm_bgzf_compress on raw pointers -> (return code, n_out)."""
    from kmer_mapper_amd import _lib
    n_out = ctypes.c_int64(-1)
    rc = _lib.lib().kmm_bgzf_compress(0, ctypes.c_void_p(src), n, ctypes.c_void_p(out), cap, ctypes.byref(n_out))
    return rc, n_out.value


# ---------------------------------------------------------------------------------------------- the operator
@pytest.mark.parametrize("name", list(CASES))
def test_operator_against_zlib_and_the_cpu_build(kmm, golden, name):
    import torch
    from kmer_mapper_amd import _lib, util
    text = CASES[name]
    n, cap = len(text), bc.bound(len(text))
    assert _lib.lib().kmm_bgzf_bound(n) == cap
    host = util.bgzf_compress(text).tobytes()                                       # host -> host
    sizes = bc.check_stream(host, text)
    assert sizes == golden[name]["sizes"]
    assert hashlib.sha256(host).hexdigest() == golden[name]["sha256"]
    assert util.bgzf_compress(text).tobytes() == host                               # a second call
    src = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda() if n else torch.zeros(1, dtype=torch.uint8, device="cuda")
    assert util.bgzf_compress(src[:n]).tobytes() == host                            # device -> host
    out = torch.full((cap + 5,), 0xEE, dtype=torch.uint8, device="cuda")            # device -> device
    rc, n_out = _compress(src.data_ptr(), n, out.data_ptr(), cap)
    assert (rc, n_out) == (_lib.KMM_OK, len(host))
    got = out.cpu().numpy()
    assert got[:n_out].tobytes() == host and (got[n_out:] == 0xEE).all()
    if n:                                                                           # one byte below the bound: refused, nothing written
        out.fill_(0xEE)
        rc, n_out = _compress(src.data_ptr(), n, out.data_ptr(), cap - 1)
        assert (rc, n_out) == (_lib.KMM_ERR_INVALID_ARG, 0)
        assert ("can need %d bytes" % cap) in _lib.lib().kmm_last_error().decode()
        assert (out.cpu().numpy() == 0xEE).all()


def test_bound_and_refusals(kmm):
    from kmer_mapper_amd import _lib
    L = _lib.lib()
    assert [L.kmm_bgzf_bound(n) for n in (-1, 0, 1, 65280, 65281, 2 * 65280)] == [-1, 0, 32, 65311, 65343, 2 * 65311]
    buf = np.zeros(64, dtype=np.uint8)
    assert _compress(buf.ctypes.data, -1, buf.ctypes.data, 64)[0] == _lib.KMM_ERR_INVALID_ARG
    assert _compress(None, 0, None, 0) == (_lib.KMM_OK, 0)


# ---------------------------------------------------------------------------------------------- the take
TAKE_CASES = ["rk_output_residues_fasta_k31__default", "rk_tile_ends_fastq_k31__default", "crlf_fastq_k31__default",
              "super_tile_fastq_k31__default"]


def _inflate(members):
    data = members.tobytes() if isinstance(members, np.ndarray) else members
    return gzip.decompress(data + EOF_BLOCK)


@pytest.mark.parametrize("name", TAKE_CASES)
def test_take_against_the_plain_take_on_a_second_handle(kmm, monkeypatch, name):
    case = _case(name)
    with _open(kmm, case.base.index, monkeypatch) as dev, _open(kmm, case.base.index, monkeypatch) as ref:
        for d in (dev, ref):
            _keep_on(d, case)
        # one call, then a take; two calls, then a take: the takes concatenated are one BGZF stream
        stream, plain = b"", b""
        for calls in (1, 2):
            for d in (dev, ref):
                for _ in range(calls):
                    _map(d, case.base)
            want, want_records = ref.take_kept_records()
            pending = dev.get_param("record_keep_pending_bytes")
            assert pending == len(want)
            members, n_text, n_records = dev.take_kept_bgzf()
            assert (n_text, n_records) == (len(want), want_records)
            assert len(members) <= bc.bound(len(want))
            bc.check_stream(members.tobytes(), want.tobytes())
            assert dev.get_param("record_keep_pending_bytes") == 0 and dev.get_param("record_keep_pending_records") == 0
            stream += members.tobytes()
            plain += want.tobytes()
        assert len(plain) > 0 and _inflate(stream) == plain
        # an empty queue gives zeros
        members, n_text, n_records = dev.take_kept_bgzf()
        assert (len(members), n_text, n_records) == (0, 0, 0)
        # the two kinds of take mixed on one handle
        _map(dev, case.base)
        got, n = dev.take_kept_records()
        assert got.tobytes() == rk.expected(case)[0] and n == rk.expected(case)[1]
        _map(dev, case.base)
        assert _inflate(dev.take_kept_bgzf()[0]) == rk.expected(case)[0]


def test_take_into_a_device_buffer_too_small_capacity_and_reset(kmm, monkeypatch):
    import torch
    from kmer_mapper_amd import _lib
    case = _case("rk_tile_ends_fastq_k31__default")
    text, n_kept = rk.expected(case)[:2]
    with _open(kmm, case.base.index, monkeypatch) as dev:
        _keep_on(dev, case)
        _map(dev, case.base)
        _map(dev, case.base)
        need = bc.bound(2 * len(text))
        short = torch.full((need - 1,), 0xEE, dtype=torch.uint8, device="cuda")
        with pytest.raises(ValueError, match="can need %d bytes" % need):
            dev.take_kept_bgzf(out=short)
        assert (short.cpu().numpy() == 0xEE).all()                                  # nothing taken: the queue as it was,
        assert dev.get_param("record_keep_pending_bytes") == 2 * len(text)
        got, n = dev.take_kept_records()                                           # takeable by the plain take
        assert got.tobytes() == text * 2 and n == 2 * n_kept
        _map(dev, case.base)
        with pytest.raises(ValueError, match="can need"):
            dev.take_kept_bgzf(out=short[:10])
        out = torch.full((need,), 0xEE, dtype=torch.uint8, device="cuda")            # and by the compressed one, into device memory
        n_comp, n_text, n_records = dev.take_kept_bgzf(out=out)
        assert (n_text, n_records) == (len(text), n_kept) and 0 < n_comp <= bc.bound(len(text))
        host = out.cpu().numpy()
        assert _inflate(host[:n_comp]) == text and (host[n_comp:] == 0xEE).all()
        with pytest.raises(ValueError, match="mate is 2"):
            dev.take_kept_bgzf(mate=2)
        _map(dev, case.base)                                                        # kmm_reset_counts empties the queue
        dev.reset()
        assert dev.take_kept_bgzf()[1:] == (0, 0)
        nc, nb, nr = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert _lib.lib().kmm_take_kept_bgzf(dev._h, 0, None, 0, ctypes.byref(nc), ctypes.byref(nb), ctypes.byref(nr)) == _lib.KMM_OK
        assert (nc.value, nb.value, nr.value) == (0, 0, 0)


def test_take_of_both_mates_after_record_pairs(kmm, monkeypatch):
    case = _case("rk_tile_ends_fastq_k31__default")
    base = case.base
    from tests.test_gpu_record_keep import _kfmt
    with _open(kmm, base.index, monkeypatch) as dev, _open(kmm, base.index, monkeypatch) as ref:
        for d in (dev, ref):
            _keep_on(d, case)
            d.map_record_pairs(base.text, base.text, fmt=_kfmt(base), k=base.k, max_index_lookup_frequency=base.max_freq,
                               also_revcomp=base.revcomp, lut=base.lut)
        for mate in (1, 0):
            want, want_records = ref.take_kept_mates(mate)
            members, n_text, n_records = dev.take_kept_bgzf(mate=mate)
            assert len(want) > 0 and (n_text, n_records) == (len(want), want_records)
            bc.check_stream(members.tobytes(), want.tobytes())


def test_timing_ids_of_the_writer(kmm, monkeypatch):
    from kmer_mapper_amd import _lib
    case = _case("rk_tile_ends_fastq_k31__default")
    with _open(kmm, case.base.index, monkeypatch) as dev:
        _keep_on(dev, case)
        dev.set_timing(True)
        _map(dev, case.base)
        dev.take_kept_bgzf()
        ms, launches = dev.get_timing(_lib.KERNEL_BGZF_DEFLATE)
        assert launches == 1 and ms > 0
        assert dev.get_timing(_lib.KERNEL_BGZF_GATHER)[1] == 1


# ---------------------------------------------------------------------------------------------- the façade and the command line
def _cli_inputs(tmp_path):
    from tests import read_hits_cases as rc
    from tests import record_hits_cases as rh
    from tests.test_gpu_record_keep import K, _route_reads
    index = rc.genome_index(K)
    text = rh.text_of(rh.FASTQ, _route_reads() * 3)                                  # (an even number of records: mates in turn)
    reads, npz = str(tmp_path / "reads.fq"), str(tmp_path / "index.npz")
    open(reads, "wb").write(text)
    index.to_file(npz)
    common = ["select-reads", "-i", npz, "-k", str(K), "-c", "1500", "-I", str(rc.NO_FILTER), "--min-hits", "3"]
    return index, text, reads, common


def test_facade_compress(kmm):
    from kmer_mapper_amd import gz_io, mapper
    from tests import read_hits_cases as rc
    from tests import record_hits_cases as rh
    from tests.test_gpu_record_keep import K, _route_reads
    index = rc.genome_index(K)
    text = rh.text_of(rh.FASTQ, _route_reads() * 2)
    rule = dict(k=K, max_index_lookup_frequency=rc.NO_FILTER, min_hits=3)
    plain, hits, windows = mapper.select_records(index, text, **rule)
    packed, hits2, windows2 = mapper.select_records(index, text, compress=True, **rule)
    assert 0 < len(plain) < len(text) and packed.endswith(gz_io.BGZF_EOF) and gzip.decompress(packed) == plain
    assert np.array_equal(hits, hits2) and np.array_equal(windows, windows2)
    for raw2 in (None, text):
        a = mapper.select_record_pairs(index, text, raw2, **rule)
        b = mapper.select_record_pairs(index, text, raw2, compress=True, **rule)
        assert len(a[0]) > 0 and gzip.decompress(b[0]) == a[0]
        assert (a[1] is None and b[1] is None) or gzip.decompress(b[1]) == a[1]
        assert np.array_equal(a[2], b[2])


@pytest.mark.parametrize("form", ["single", "interleaved", "two_files"])
def test_command_line_bgzf_against_plain(kmm, tmp_path, form):
    from kmer_mapper_amd import gz_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    index, text, reads, common = _cli_inputs(tmp_path)
    outs = [str(tmp_path / "kept_1"), str(tmp_path / "kept_2")][:2 if form == "two_files" else 1]
    mates = str(tmp_path / "mates.fq")                                               # (the same records once more: mates by position)
    open(mates, "wb").write(text)
    more = {"single": [], "interleaved": ["--interleaved"], "two_files": ["-f2", mates]}[form]

    def run(suffix, flags):
        names = [o + suffix for o in outs]
        args = common + ["-f", reads, "-o", names[0]] + more + (["-o2", names[1]] if len(names) == 2 else []) + flags
        return run_argument_parser(args), [open(n, "rb").read() for n in names]

    counts, plain = run(".fq", [])
    counts_z, packed = run(".fq.gz", ["--bgzf"])
    assert counts == counts_z and 0 < counts[1] < counts[0]
    for p, z in zip(plain, packed):
        assert len(p) > 0 and z.endswith(gz_io.BGZF_EOF) and gz_io.container(z[:1 << 16]) == "bgzf"
        assert gzip.decompress(z) == p
        bc.members_of(z)                                                             # (every member, the last one included, is BGZF)


def test_the_library_reads_what_it_writes(kmm, tmp_path):
    """select-reads --bgzf, its output fed back as -f with --min-hits 0: the library's GPU inflater (the BGZF route) reads what its
    deflater wrote, and the second output holds the same text."""
    from kmer_mapper_amd import gz_io
    from kmer_mapper_amd.command_line_interface import run_argument_parser
    index, text, reads, common = _cli_inputs(tmp_path)
    first, second, everything = str(tmp_path / "kept.fq.gz"), str(tmp_path / "again.fq.gz"), str(tmp_path / "all.fq.gz")
    run_argument_parser(common + ["-f", reads, "-o", first, "--bgzf"])
    assert gz_io.is_bgzf(first)
    kept = gzip.decompress(open(first, "rb").read())
    assert 0 < len(kept) < len(text)
    again = common[:-2] + ["--min-hits", "0"]
    seen, n = run_argument_parser(again + ["-f", first, "-o", second, "--bgzf"])
    assert seen == n == kept.count(b"\n") // 4
    assert gzip.decompress(open(second, "rb").read()) == kept
    # the whole text (several members per drain with a large chunk) through the same loop
    big = ["1000000" if i and again[i - 1] == "-c" else a for i, a in enumerate(again)]
    run_argument_parser(big + ["-f", reads, "-o", everything, "--bgzf"])
    assert gzip.decompress(open(everything, "rb").read()) == text
