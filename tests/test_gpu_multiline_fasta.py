"""GPU tests of the multi-line FASTA unwrap (KMM_FORMAT_FASTA, include/kmm.h; csrc/kmm_records.hpp k_ml_*, map_multiline_piece
and the piece loop of kmm_map_records) at the seams of its lanes, tiles, scan rounds and pieces.  Every check compares three
things on a clean handle: the node counts with the oracle's on the reads the model unwraps (tests/multiline_cases.py, held to
its conditions by tests/test_multiline_cases_on_the_cpu.py), kmm_get_stats' lookups with the oracle's window count — the one
number that moves for every byte wrongly kept or dropped, hit or no hit — and (consumed, n_records) with the model.  Exact:
no tolerance is involved."""
import ctypes

import numpy as np
import pytest

from tests import multiline_cases as mc

pytestmark = pytest.mark.gpu

K = mc.K
FASTA, LAST = 1, 0x100          # KMM_FORMAT_FASTA, KMM_FORMAT_LAST_CHUNK
KMM_OK, KMM_ERR_INVALID_BASE, KMM_ERR_MALFORMED = 0, -4, -6


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    assert (_lib.FORMAT_FASTA, _lib.FORMAT_LAST_CHUNK) == (FASTA, LAST)
    assert (_lib.KMM_ERR_INVALID_BASE, _lib.KMM_ERR_MALFORMED) == (KMM_ERR_INVALID_BASE, KMM_ERR_MALFORMED)
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def dev(kmm):
    """The one handle of this module."""
    index = mc.index()
    d = kmm.DeviceIndex.from_index(index, index.max_node_id())
    assert d.get_param("radix_available")
    yield d
    d.close()


_ANSWERS = {}


@pytest.fixture(scope="module")
def answers(oracle):
    """name -> the model's reads of the case and the oracle's answers on them (computed once, never changed):
    counts / windows of all reads, *_rc with reverse complements, *_head of all reads but the last."""
    def get(name, lut=None):
        key = (name, lut is not None)
        if key not in _ANSWERS:
            from tests.ambiguous_cases import split_at_breaks
            index = mc.index()
            mx = index.max_node_id()
            raw = mc.build(name)["raw"]
            two, used = mc.unwrap_model(raw, True)
            bases, offsets = mc.reads_of(two)
            a = dict(raw=raw, n_reads=offsets.shape[0] - 1, cut=mc.cut_model(raw, False))

            def ask(b, o, rc=False):
                if lut is not None:          # a break is DEFINED as a read boundary in its place (tests/ambiguous_cases.py)
                    b, o = split_at_breaks(b, o, lut)
                counts, n = oracle.map_reads(index, mx, b, o, K, also_revcomp=rc)
                counts.setflags(write=False)
                return counts, int(n)
            a["counts"], a["windows"] = ask(bases, offsets)
            a["counts_rc"], _ = ask(bases, offsets, rc=True)
            a["counts_head"], a["windows_head"] = ask(bases[:offsets[-2]], offsets[:-1])
            assert a["windows"] > 0 and a["counts"].sum() > 0.3 * a["windows"]          # the reads come from the index's genome
            _ANSWERS[key] = a
        return _ANSWERS[key]
    return get


def _measure(dev, call):
    """(what the call returned, node counts, lookups) of map call(s) on a clean handle."""
    dev.reset()
    dev.get_stats(reset=True)
    ret = call()
    return ret, dev.get_node_counts(), dev.get_stats()[0]


class _params:
    def __init__(self, dev, **kw):
        self.dev, self.kw = dev, kw

    def __enter__(self):
        for name, v in self.kw.items():
            self.dev.set_param(name, v)

    def __exit__(self, *exc):
        for name in self.kw:
            self.dev.set_param(name, 0)


def _whole(dev, raw, a, what, rc=False, lut=None):
    """One call with the last-chunk flag: everything consumed, every record, the oracle's counts and windows."""
    ret, counts, lookups = _measure(dev, lambda: dev.map_records(raw, fmt=FASTA | LAST, k=K, also_revcomp=rc, lut=lut))
    assert ret == (raw.shape[0], a["n_reads"]), (what, "consumed, n_records", ret)
    assert lookups == (2 if rc else 1) * a["windows"], (what, "lookups", lookups)
    assert np.array_equal(counts, a["counts_rc" if rc else "counts"]), (what, "counts")


def _in_two_calls(dev, raw, a, cut, what):
    """Without the flag the call stops at the start of the last header line; the remainder, with the flag, completes it."""
    ret, counts, lookups = _measure(dev, lambda: dev.map_records(raw, fmt=FASTA, k=K))
    assert ret == (cut, a["n_reads"] - 1), (what, "consumed, n_records", ret)
    assert lookups == a["windows_head"] and np.array_equal(counts, a["counts_head"]), (what, "all records but the last")
    rest = raw[cut:]
    assert dev.map_records(rest, fmt=FASTA | LAST, k=K) == (rest.shape[0], 1), (what, "the remainder")
    assert dev.get_stats()[0] == a["windows"] and np.array_equal(dev.get_node_counts(), a["counts"]), (what, "both calls")


def _first_wrong(dev, check, shifts, what):
    """Runs check(shift) for every shift and reports the first that fails by number (and how many did)."""
    wrong = []
    for s in shifts:
        try:
            check(s)
        except (AssertionError, ValueError, RuntimeError) as e:           # (a device-found error surfaces as ValueError)
            wrong.append((s, repr(e)[:300]))
            dev.reset()
    assert not wrong, "%s: first wrong shift %d of %d wrong: %s" % (what, wrong[0][0], len(wrong), wrong[0][1])


# ---------------------------------------------------------------------------------------------- shift_sweep
def test_shift_sweep_every_byte_at_every_position_of_a_lane_and_a_tile(dev, answers):
    """All 1040 shifts, one call with the flag each: the reads and so the answer are the same at every shift."""
    a = answers("shift_sweep")
    _first_wrong(dev, lambda s: _whole(dev, np.frombuffer(mc.sweep_text(s), np.uint8), a, s), mc.SWEEP_SHIFTS, "shift_sweep")


def test_shift_sweep_without_the_flag_stops_at_the_last_header(dev, answers):
    """Every 7th shift and the shifts that put the last header on a tile start, one byte either side of it and on a lane start
    (the branch `tile * 1024 > limit` of k_ml_scatter), and the other named seams."""
    a = answers("shift_sweep")
    named = mc.sweep_named_shifts()
    assert set(named) == set(mc.SWEEP_CONDITIONS)

    def check(s):
        raw = np.frombuffer(mc.sweep_text(s), np.uint8)
        _in_two_calls(dev, raw, a, mc.cut_model(raw, False), s)
    _first_wrong(dev, check, sorted(set(range(0, 1040, 7)) | set(named.values())), "shift_sweep, two calls")


# ---------------------------------------------------------------------------------------------- round_seam
def test_round_seam_the_carry_of_the_scan_and_the_second_super_tile(dev, answers):
    """Three rounds of k_ml_scan, three super-tiles: a sequence line of 1.2 MiB whose terminator, and the last header behind
    it, cross the 2 MiB seam byte by byte over the 35 shifts."""
    a = answers("round_seam")
    _first_wrong(dev, lambda d: _whole(dev, np.frombuffer(mc.seam_text(d), np.uint8), a, d), mc.SEAM_SHIFTS, "round_seam")

    def check(d):
        raw = np.frombuffer(mc.seam_text(d), np.uint8)
        _in_two_calls(dev, raw, a, mc.seam_layout(d)["last_header"], d)
    _first_wrong(dev, check, (-1, 0, 1), "round_seam, two calls")


def test_round_seam_paths_reverse_complements_and_device_buffers(dev, answers):
    """Shift 0 on the direct and the radix path, with reverse complements, and from a device buffer that starts at an odd
    byte offset of a larger allocation."""
    import torch
    a = answers("round_seam")
    raw = a["raw"]
    for path, counter in ((1, "direct_batches"), (2, "radix_batches")):
        before = dev.get_param(counter)
        with _params(dev, path=path):
            _whole(dev, raw, a, "path %d" % path)
            _whole(dev, raw, a, "path %d, revcomp" % path, rc=True)
        assert dev.get_param(counter) > before, path
    _whole(dev, raw, a, "revcomp", rc=True)
    for shift in (0, 1, 3, 13):
        buf = torch.zeros(raw.shape[0] + 64, dtype=torch.uint8, device="cuda")
        buf[shift:shift + raw.shape[0]] = torch.from_numpy(raw.copy()).cuda()
        view = buf[shift:shift + raw.shape[0]]
        torch.cuda.synchronize()          # (torch's copy runs on torch's stream, the map call on the handle's)
        _whole(dev, view, a, "device buffer + %d" % shift)
        _in_two_calls(dev, view, a, a["cut"], "device buffer + %d" % shift)


# ---------------------------------------------------------------------------------------------- n_runs
@pytest.mark.parametrize("skip", [False, True], ids=["n_as_a", "n_as_break"])
def test_runs_of_n_across_the_line_breaks(dev, answers, skip):
    """Runs of N that begin and end at every column of the wrapped lines: read as A by the default table (a run of 31 and
    more finds poly-A), a break under the skip table — the run is ONE break once the line ends inside it are gone."""
    from kmer_mapper_amd.util import ambiguous_skip_lut
    lut = ambiguous_skip_lut() if skip else None
    a = answers("n_runs", lut)
    for path in (1, 2):
        with _params(dev, path=path):
            for rc in (False, True):
                _whole(dev, a["raw"], a, "path %d revcomp %d" % (path, rc), rc=rc, lut=lut)


# ---------------------------------------------------------------------------------------------- pieces
@pytest.mark.parametrize("path", [0, 2])
def test_pieces_equal_the_unpieced_call(dev, answers, path):
    """The chunk cut into pieces of 4, 16 and 64 KiB inside one call (tens of pieces, each unwrapped into one stage's buffer
    and mapped from it through the next): only the piece that ends the chunk may be told that the file ends."""
    a = answers("pieces")
    raw = a["raw"]
    for kb in (0,) + mc.PIECE_KBS:
        with _params(dev, path=path, debug_records_piece_kb=kb):
            _whole(dev, raw, a, "pieces of %d KiB" % kb)
            _in_two_calls(dev, raw, a, a["cut"], "pieces of %d KiB" % kb)


def test_chunks_of_10000_bytes_with_the_tail_carried(dev, answers):
    """The caller's loop: chunks of 10 000 new bytes, raw[consumed:] carried forward, the flag on the chunk that ends the file."""
    a = answers("pieces")
    raw = a["raw"]

    def feed():
        pos = fed = n = 0
        while pos < raw.shape[0]:
            fed = min(raw.shape[0], max(fed, pos) + 10_000)
            chunk = raw[pos:fed]
            used, n_rec = dev.map_records(chunk, fmt=FASTA | (LAST if fed == raw.shape[0] else 0), k=K)
            assert (used, n_rec + (fed != raw.shape[0])) == (mc.cut_model(chunk, fed == raw.shape[0]), len(mc.header_starts(chunk))), pos
            pos += used
            n += n_rec
        return pos, n
    # a chunk that ends between the '\\r' and the '\\n' of a line: that '\\r' is no lone one, it lies in the record that stays
    cr = int(np.flatnonzero(raw[20_000:] == mc.CR)[0]) + 20_000
    heads = mc.header_starts(raw)
    chunk = raw[int(heads[heads < cr][-3]):cr + 1]
    assert chunk[-1] == mc.CR and len(mc.header_starts(chunk)) == 3
    dev.reset()
    assert dev.map_records(chunk, fmt=FASTA, k=K) == (mc.cut_model(chunk, False), 2)
    dev.synchronize()
    for kb in (0, 4):
        with _params(dev, debug_records_piece_kb=kb):
            ret, counts, lookups = _measure(dev, feed)
        assert ret == (raw.shape[0], a["n_reads"]) and lookups == a["windows"] and np.array_equal(counts, a["counts"]), kb


# ---------------------------------------------------------------------------------------------- a record longer than a piece
def _abi_call(dev, raw, fmt):
    """kmm_map_records through the C ABI: (return code, *consumed, *n_records, kmm_last_error) — the Python binding turns the
    codes into exceptions and drops them."""
    from kmer_mapper_amd import _lib
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    used, n_rec = ctypes.c_int64(-1), ctypes.c_int64(-1)
    rc = _lib.lib().kmm_map_records(dev._h, raw.ctypes.data_as(ctypes.c_void_p), raw.shape[0], fmt, K, 1000, 0, None,
                                    ctypes.byref(used), ctypes.byref(n_rec))
    return rc, used.value, n_rec.value, _lib.lib().kmm_last_error().decode("utf-8", "replace") if rc else ""


def _abi_synchronize(dev):
    from kmer_mapper_amd import _lib
    return _lib.lib().kmm_synchronize(dev._h)


@pytest.mark.parametrize("flag", [LAST, 0], ids=["last_chunk", "more_to_come"])
def test_a_record_longer_than_a_piece_is_an_error_never_a_silent_stop(dev, answers, oracle, flag):
    """Three records, the middle one 10 KiB, pieces of 4 KiB: the second piece starts on the long record and holds no other
    header.  With KMM_FORMAT_LAST_CHUNK kmm.h promises that everything is consumed: the call must do that or fail — never
    return KMM_OK with fewer bytes (what it did before: the rest of the file dropped without a word).  It fails, with and
    without the flag (include/kmm.h), naming the piece; the piece before it is already counted."""
    a = answers("long_record_in_pieces")
    raw = a["raw"]
    second = int(mc.header_starts(raw)[1])
    assert mc.pieces_model(raw, bool(flag), mc.LONG_PIECE_KB << 10) == ("record exceeds a piece", second)
    dev.reset()
    dev.get_stats(reset=True)
    with _params(dev, debug_records_piece_kb=mc.LONG_PIECE_KB):
        rc, used, n_rec, message = _abi_call(dev, raw, FASTA | flag)
    if rc == KMM_OK and flag:
        assert used == raw.shape[0] and np.array_equal(dev.get_node_counts(), a["counts"]), "KMM_OK with %d of %d bytes" % (used, raw.shape[0])
    assert rc == KMM_ERR_MALFORMED, (rc, used, message)
    assert "exceeds a piece" in message and "byte %d " % second in message, message
    index = mc.index()
    first = mc.reads_of(mc.unwrap_model(raw[:second], True)[0])
    want, windows = oracle.map_reads(index, index.max_node_id(), first[0], first[1], K)
    assert np.array_equal(dev.get_node_counts(), want) and dev.get_stats()[0] == windows          # the first piece is counted
    # a piece that holds the record: all of it
    with _params(dev, debug_records_piece_kb=16):
        _whole(dev, raw, a, "pieces of 16 KiB")


# ---------------------------------------------------------------------------------------------- odd input
_SEQ = mc.ACGT[mc.GENOME[100:140]].tobytes()
ODD = {
    "bytes_before_the_first_header": _SEQ + b"\n>a\n" + _SEQ + b"\n",
    "header_then_header": b">a\n>b\n" + _SEQ + b"\n",
    "only_headers": b">a\n>b\n",
    "header_pairs": b">a\n>b\n" + _SEQ + b"\n>c\n>d\n" + _SEQ + b"\n",
    "lone_cr_in_a_sequence_line": b">a\n" + _SEQ[:20] + b"\r" + _SEQ[20:] + b"\n" + _SEQ + b"\n>b\n" + _SEQ + b"\n",
}


@pytest.mark.parametrize("name", sorted(ODD))
def test_odd_input_is_an_error_and_the_handle_recovers(dev, answers, name):
    """What is no multi-line FASTA fails at the call or at the next synchronising call, with KMM_ERR_MALFORMED or
    KMM_ERR_INVALID_BASE; after kmm_reset_counts the handle maps as before."""
    raw = np.frombuffer(ODD[name], np.uint8)
    if name != "lone_cr_in_a_sequence_line":      # (that one is two-line FASTA after the unwrap, with a byte that is no base)
        with pytest.raises(ValueError):
            mc.reads_of(mc.unwrap_model(raw, True)[0])
    dev.reset()
    rc, used, n_rec, message = _abi_call(dev, raw, FASTA | LAST)
    if rc == KMM_OK:
        rc = _abi_synchronize(dev)
    assert rc in (KMM_ERR_MALFORMED, KMM_ERR_INVALID_BASE), (name, rc, used, n_rec, message)
    dev.reset()
    a = answers("shift_sweep")
    _whole(dev, a["raw"], a, "after " + name)


def test_a_final_line_without_newline_is_malformed(dev, answers):
    """include/kmm.h: at the end of the file the last line must end with a newline, with KMM_FORMAT_LAST_CHUNK too (the file
    readers of the package add one).  The same bytes with the newline are two records."""
    text = b">a\n" + _SEQ + b"\n" + _SEQ + b"\n>b\n" + _SEQ + b"\n" + _SEQ
    dev.reset()
    rc, used, n_rec, message = _abi_call(dev, np.frombuffer(text, np.uint8), FASTA | LAST)
    assert rc == KMM_ERR_MALFORMED, (rc, used, n_rec, message)
    dev.reset()
    assert dev.map_records(np.frombuffer(text + b"\n", np.uint8), fmt=FASTA | LAST, k=K) == (len(text) + 1, 2)
    dev.synchronize()
    dev.reset()
    a = answers("shift_sweep")
    _whole(dev, a["raw"], a, "after the line without newline")
