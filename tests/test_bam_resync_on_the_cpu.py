"""CPU tier of kmm_bam_find_record_start and of the ownership rule of a sharded BAM file: the per-tile resync step of
csrc/kmm_bam.hpp — the code k_bam_resync runs 64 positions at a time — compiled by itself with g++ (tests/bam_resync_cpu_driver.hpp)
against record offsets an independent pure-Python walk takes from the same bytes; once more under AddressSanitizer +
UndefinedBehaviorSanitizer as an executable of its own; bgzf_ranges.rank_member_range_bam against a fake device that answers from
the Python reader; and the CLI's switch."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_bam_walk_on_the_cpu import _payload, _reads, read_bam_payload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
NONE = (1 << 64) - 1


def record_starts(data):
    """Offsets of the records of inflated BAM bytes (the block_size chain behind the header), and the header's length."""
    recs, hdr = read_bam_payload(data)
    starts, p = [], hdr
    for _ in recs:
        starts.append(p)
        p += 4 + struct.unpack_from("<i", data, p)[0]
    assert p == len(data)
    return np.asarray(starts, np.int64), hdr


def first_start_at_or_after(starts, lo, hi):
    """For every byte b in [lo, hi): the first record start >= b (NONE if there is none)."""
    b = np.arange(lo, hi)
    i = np.searchsorted(starts, b)
    return np.where(i < len(starts), starts[np.minimum(i, len(starts) - 1)], NONE).astype(np.uint64)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("bam_resync")
    src = d / "shim.cpp"
    src.write_text('#include "bam_resync_cpu_driver.hpp"\n')
    so = str(d / "shim.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-shared", "-fPIC", "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"),
                           str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.bam_resync_cpu.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                   ctypes.c_uint64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.bam_resync_every_byte.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32,
                                          ctypes.c_void_p]
    lib.bam_resync_every_byte.restype = None
    return lib


def _members(n, msize):
    """A window of n inflated bytes cut into members of msize (compressed offsets: 10 x the inflated ones)."""
    o = list(range(0, n, msize)) + [n]
    if n == 0:
        o = [0]
    return np.asarray([10 * x for x in o], np.uint64), np.asarray(o, np.uint64)


def _one(lib, window, whole, cap=0, n_ref=0, msize=1000):
    m_off, o_off = _members(len(window), msize)
    member, skip, pos = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_uint64(0)
    assert lib.bam_resync_cpu(window, len(window), m_off.ctypes.data, o_off.ctypes.data, len(m_off) - 1, int(whole), cap, n_ref,
                              ctypes.byref(member), ctypes.byref(skip), ctypes.byref(pos)) == 0
    return member.value, skip.value, pos.value


def _every_byte(lib, data, start, length, n_ref):
    out = np.zeros(len(data) - start, np.uint64)
    lib.bam_resync_every_byte(data, len(data), start, length, n_ref, out.ctypes.data)
    return out


def _ragged_payload(seed, n=300, n_ref=0):
    rng = np.random.default_rng(seed)
    reads = _reads(rng, n, 0, 400)
    refs = [(b"chr%d" % i, 1000) for i in range(n_ref)]
    return _payload(reads, refs=refs, text=b"@HD\tVN:1.6\n")


@pytest.mark.parametrize("n_ref", [0, 3])
def test_every_boundary_byte_finds_the_first_true_record_start(lib, n_ref):
    """A window that begins at ANY byte behind the header and runs to the end of the file: the lowest holding position is the
    first true record start at or after it — never an earlier one, for these bytes — and a window cut off behind 3000 bytes
    (longer than any record here) gives the same wherever a whole record still fits."""
    data = _ragged_payload(21 + n_ref, n_ref=n_ref)
    starts, hdr = record_starts(data)
    want = first_start_at_or_after(starts, hdr, len(data))
    got = _every_byte(lib, data, hdr, 0, n_ref)
    assert np.array_equal(got, want)
    assert want[-1] == NONE and want[0] == hdr                     # (behind the last start: no chain; at the header's end: there)
    got = _every_byte(lib, data, hdr, 3000, n_ref)
    fits = np.arange(hdr, len(data)) + 3000 <= len(data)            # windows that do not reach the file's end
    sizes = np.diff(np.append(starts, len(data)))
    i = np.minimum(np.searchsorted(starts, np.arange(hdr, len(data))), len(starts) - 1)
    whole = starts[i] + sizes[i] <= np.arange(hdr, len(data)) + 3000
    assert np.array_equal(got[fits & whole], want[fits & whole])
    assert sizes.max() < 3000 and (fits & whole).sum() > 50_000


def _decoy_payload():
    """Records around one whose aux field holds a forged chain of 120 small records (and 8 zero bytes behind it, inside the
    same field: the forged chain does not run on into the next true record).  Returns (payload, offset of the forged chain,
    its length, true record starts)."""
    rng = np.random.default_rng(31)
    reads = _reads(rng, 60, 50, 300)
    forged = _payload([b"ACGT" * 5])[12:] * 120
    auxs = [b""] * len(reads)
    auxs[30] = b"ZZZ" + forged + b"\0" * 8
    data = _payload(reads, auxs=auxs)
    starts, _ = record_starts(data)
    at = data.index(forged)
    assert starts[30] < at < starts[31] and at + len(forged) + 8 == starts[31]
    return data, at, len(forged), starts


def test_a_forged_chain_shorter_than_the_window_is_rejected(lib):
    data, at, n_forged, starts = _decoy_payload()
    window = data[at - 10:]                                         # (a member that begins 10 bytes in front of the forgery)
    member, skip, pos = _one(lib, window, whole=True)
    assert pos == starts[31] - (at - 10)                            # the next TRUE record start
    assert (member, skip) == (10 * (pos // 1000 * 1000), pos % 1000)
    # ... not at the end of the file either: the window stops inside a later record
    member, skip, pos2 = _one(lib, window[:n_forged + 3000], whole=False)
    assert pos2 == pos


def test_a_forged_chain_that_reaches_the_capped_window_is_accepted(lib):
    """The documented limit: with the examined bytes capped inside the forgery nothing tells it from records — the answer lies
    inside a record, and kmm_map_bam's tail stop is what catches it (tests/test_gpu_bam_shard.py)."""
    data, at, n_forged, starts = _decoy_payload()
    window = data[at - 10:]
    member, skip, pos = _one(lib, window, whole=True, cap=n_forged // 2)
    assert pos == 10 and (member, skip) == (0, 10)
    assert _one(lib, window, whole=True, cap=n_forged + 4000)[2] == starts[31] - (at - 10)   # (a cap behind it: rejected)


def test_a_window_shorter_than_one_record_asks_for_a_longer_one(lib):
    rng = np.random.default_rng(41)
    data = _payload(_reads(rng, 3, 5000, 6000) + _reads(rng, 20, 50, 100))
    starts, hdr = record_starts(data)
    window = data[hdr + 100:]                                       # begins inside the first long record
    assert _one(lib, window[:2000], whole=False)[0] == -1           # no record start in it
    assert _one(lib, window[:starts[1] - hdr - 100 + 1000], whole=False)[0] == -1          # a start, no whole record behind it
    assert _one(lib, window, whole=True, cap=2000)[0] == -1         # the cap cuts the same way, at the file's end too
    member, skip, pos = _one(lib, window[:starts[2] - hdr - 100 + 50], whole=False)       # one whole record: its start
    assert pos == starts[1] - hdr - 100 and member == 10 * (pos // 1000 * 1000)


def test_the_end_of_the_file(lib):
    """An empty tail (no member, or only empty ones) gives (n, 0); so do last bytes in which no record starts; a chain must end
    exactly at the file's last byte; a position at a member's end belongs to the member behind it."""
    rng = np.random.default_rng(51)
    data = _payload(_reads(rng, 10, 100, 200))
    starts, hdr = record_starts(data)
    assert _one(lib, b"", whole=True)[:2] == (0, 0)
    assert _one(lib, b"", whole=False)[0] == -1
    tail = data[starts[-1] + 7:]                                    # the last record's tail: no record starts in it
    assert _one(lib, tail, whole=True, msize=50)[:2] == (10 * len(tail), 0)
    assert _one(lib, tail, whole=False)[0] == -1
    member, skip, pos = _one(lib, data[starts[5] - 3:-1], whole=True)                      # truncated file: no chain ends at its end
    assert (member, skip, pos) == (10 * (len(data) - 1 - starts[5] + 3), 0, NONE)
    size = int(starts[6] - starts[5])                              # members that end on record boundaries: skip 0 of the next
    member, skip, pos = _one(lib, data[starts[5] - size + 1:], whole=True, msize=size)
    assert pos == size - 1 and (member, skip) == (0, size - 1)
    member, skip, pos = _one(lib, data[starts[4] + 1:starts[5]] + data[starts[5]:], whole=True, msize=int(starts[5] - starts[4] - 1))
    assert (member, skip) == (10 * pos, 0)


def test_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """The same cases as an executable of its own with ASan + UBSan (tests/bam_resync_san_main.cpp; host code): every boundary
    byte of a ragged payload, the forged chain rejected and — capped — accepted, the window shorter than a record, the empty
    tail: the Python reader's offsets, and no report."""
    exe = str(tmp_path / "bam_resync_san")
    src = os.path.join(ROOT, "tests", "bam_resync_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and ("asan" in build.stderr or "ubsan" in build.stderr or "sanitize" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])
    assert build.returncode == 0, build.stderr

    def run(*args):
        r = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
        return r.stdout

    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    data = _ragged_payload(61, n=120, n_ref=2)
    starts, hdr = record_starts(data)
    inp.write_bytes(data)
    run("every", inp, hdr, 0, 2, outp)
    assert np.array_equal(np.fromfile(str(outp), np.uint64), first_start_at_or_after(starts, hdr, len(data)))
    data, at, n_forged, starts = _decoy_payload()
    inp.write_bytes(data[at - 10:])
    true_next = int(starts[31]) - (at - 10)
    assert run("one", inp, 1, 0, 0, 1000).split() == [str(10 * (true_next // 1000 * 1000)), str(true_next % 1000), str(true_next)]
    assert run("one", inp, 1, n_forged // 2, 0, 1000).split() == ["0", "10", "10"]
    inp.write_bytes(data[starts[3] + 5:starts[3] + 40])
    assert run("one", inp, 0, 0, 0, 1000).split()[0] == "-1"
    assert run("one", inp, 1, 0, 0, 10).split()[:2] == ["350", "0"]
    inp.write_bytes(b"")
    assert run("one", inp, 1, 0, 0, 10).split()[:2] == ["0", "0"]


# ---- the ownership rule against a fake device that answers from the Python reader ----

class FakeDev:
    """bam_header / bam_find_record_start answered from zlib + the record offsets: the TRUE first record start at or after a
    window's first member, as (member, skip)."""

    def __init__(self, comp):
        from kmer_mapper_amd import bgzf_ranges
        self.comp = comp
        self.base = np.frombuffer(comp, np.uint8).ctypes.data
        self.m_off = bgzf_ranges.member_chain(comp)
        parts = [bgzf_ranges.inflate_member(comp, int(a), int(b)) for a, b in zip(self.m_off[:-1], self.m_off[1:])]
        self.o_off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        self.data = b"".join(parts)
        self.starts, self.hdr = record_starts(self.data)
        self.n_ref = struct.unpack_from("<i", self.data, 8 + struct.unpack_from("<i", self.data, 4)[0])[0]
        self.calls = 0

    def get_param(self, name):
        return 0

    def position(self, p):
        """Inflated offset p as (member, skip): the member that holds byte p."""
        j = int(np.searchsorted(self.o_off, p, side="right")) - 1
        while j < len(self.m_off) - 1 and self.o_off[j + 1] <= p:
            j += 1
        return (int(self.m_off[j]), int(p - self.o_off[j])) if j < len(self.m_off) - 1 else (len(self.comp), 0)

    def bam_header(self, a):
        return (self.n_ref, *self.position(self.hdr))

    def bam_find_record_start(self, a, n_ref):
        assert n_ref == self.n_ref
        self.calls += 1
        m = a.ctypes.data - self.base
        j = int(np.searchsorted(self.m_off, m))
        assert self.m_off[j] == m                                   # the window starts at a member boundary
        i = int(np.searchsorted(self.starts, self.o_off[j]))
        if i == len(self.starts):
            return len(a), 0
        member, skip = self.position(int(self.starts[i]))
        return member - m, skip


def _bam_file(reads, block, n_ref=0, text=b"@HD\tVN:1.6\n", on_boundaries=False):
    from kmer_mapper_amd import reads_io
    header = reads_io.bam_header([(b"chr%d" % i, 1000) for i in range(n_ref)], text)
    recs = [reads_io.bam_record(r, b"r%d" % i) for i, r in enumerate(reads)]
    if on_boundaries:                                               # members that end on record boundaries, as htslib writes them
        body, group = [], b""
        for rec in recs:
            if group and len(group) + len(rec) > block:
                body.append(reads_io.bgzf_members(group, 0xFF00))
                group = b""
            group += rec
        body.append(reads_io.bgzf_members(group, 0xFF00))
        return reads_io.bgzf_members(header, block) + b"".join(body) + reads_io.BGZF_EOF
    return reads_io.bgzf_members(header, block) + reads_io.bgzf_members(b"".join(recs), block) + reads_io.BGZF_EOF


def _shares_as_record_ranges(fake, world):
    """Every rank's share through rank_member_range_bam, as [first record, end record) by the true starts."""
    from kmer_mapper_amd import bgzf_ranges
    pos = [fake.position(int(s)) for s in fake.starts]
    out = []
    for r in range(world):
        lo, s0, hi, s1, n_ref = bgzf_ranges.rank_member_range_bam(fake, fake.comp, r, world)
        assert n_ref == fake.n_ref
        if r == 0:
            assert (lo, s0) == (0, 0)
            a = 0
        else:
            assert (lo, s0) in pos or (lo, s0) == (len(fake.comp), 0)
            a = pos.index((lo, s0)) if (lo, s0) in pos else len(pos)
        b = pos.index((hi, s1)) if (hi, s1) in pos else len(pos)
        assert (hi, s1) in pos or (hi, s1) == (len(fake.comp), 0)
        out.append((a, b))
    return out


@pytest.mark.parametrize("block,on_boundaries", [(0x400, False), (0x1F00, False), (0x1F00, True)])
def test_shares_partition_the_records_exactly(block, on_boundaries):
    rng = np.random.default_rng(71)
    reads = _reads(rng, 400, 0, 400)
    fake = FakeDev(_bam_file(reads, block, n_ref=3, on_boundaries=on_boundaries))
    assert len(fake.starts) == len(reads)
    n_members = len(fake.m_off) - 1
    for world in (2, 3, 5, 8, n_members + 7):
        shares = _shares_as_record_ranges(fake, world)
        assert shares[0][0] == 0 and shares[-1][1] == len(reads)
        assert all(a <= b for a, b in shares)
        assert all(shares[r][1] == shares[r + 1][0] for r in range(world - 1)), world
    assert fake.calls > 0
    if on_boundaries:                                               # every share boundary is the first byte of a member
        from kmer_mapper_amd import bgzf_ranges
        assert all(bgzf_ranges.rank_member_range_bam(fake, fake.comp, r, 5)[1] == 0 for r in range(1, 5))


def test_boundaries_inside_the_header_collapse_to_the_first_record():
    """A header of many members: the ranks whose byte boundary falls inside it all start at the first record — empty shares
    for all of them but the last — and rank 0 keeps the header."""
    from kmer_mapper_amd import bgzf_ranges
    rng = np.random.default_rng(81)
    reads = _reads(rng, 40, 10, 60)
    text = b"@HD\tVN:1.6\n" + b"".join(b"@CO\t%d %s\n" % (i, bytes(rng.integers(65, 91, 40, np.uint8))) for i in range(3000))
    fake = FakeDev(_bam_file(reads, 0x1F00, n_ref=2, text=text))
    first = fake.position(fake.hdr)
    assert first[0] > len(fake.comp) * 3 // 4                       # (the header is most of the file)
    for r in (1, 2, 3):
        lo, s0, hi, s1, _ = bgzf_ranges.rank_member_range_bam(fake, fake.comp, r, 5)
        assert (lo, s0) == first and ((hi, s1) == first or r == 3)
    lo, s0, hi, s1, _ = bgzf_ranges.rank_member_range_bam(fake, fake.comp, 0, 5)
    assert (lo, s0, hi, s1) == (0, 0, *first)
    assert _shares_as_record_ranges(fake, 5)[-1][1] == len(reads)


def test_boundaries_out_of_order_are_refused():
    """A device whose guess for the later boundary lies in front of the earlier one (a wrong guess): ValueError, no share."""
    from kmer_mapper_amd import bgzf_ranges
    rng = np.random.default_rng(91)
    fake = FakeDev(_bam_file(_reads(rng, 400, 0, 400), 0x1F00))
    true_find = fake.bam_find_record_start
    calls = []

    def lying(a, n_ref):
        calls.append(a.ctypes.data - fake.base)
        if len(calls) == 1:                                         # B(2): a position near the end of the file
            return int(fake.m_off[-3]) - calls[-1], 1
        return true_find(a, n_ref)                                  # B(3): the truth, in front of it

    fake.bam_find_record_start = lying
    with pytest.raises(ValueError, match="out of order"):
        bgzf_ranges.rank_member_range_bam(fake, fake.comp, 2, 5)
    assert len(calls) == 2


def test_a_record_longer_than_every_window_is_refused(monkeypatch):
    from kmer_mapper_amd import bgzf_ranges
    rng = np.random.default_rng(92)
    fake = FakeDev(_bam_file(_reads(rng, 400, 0, 400), 0x1F00))
    windows = []

    def never(a, n_ref):
        windows.append(len(a))
        return -1, 0

    fake.bam_find_record_start = never
    monkeypatch.setattr(bgzf_ranges, "_BAM_WINDOW", 1 << 10)
    monkeypatch.setattr(bgzf_ranges, "_BAM_WINDOW_MAX", 1 << 13)
    with pytest.raises(ValueError, match="one rank"):
        bgzf_ranges.rank_member_range_bam(fake, fake.comp, 1, 2)
    assert windows == [1 << 10, 1 << 11, 1 << 12, 1 << 13]         # doubled up to the limit


def test_the_cli_switch():
    from kmer_mapper_amd import command_line_interface as cli
    cli._check_bam_route("bam", 2, 0, shard_bam=True)
    cli._check_bam_route("bam", 1, 0)
    with pytest.raises(ValueError, match="one rank"):
        cli._check_bam_route("bam", 2, 0)
    with pytest.raises(ValueError, match="--shard-bam"):
        cli._check_bam_route("bam", 2, 0, shard_bam=False)
    args = cli.build_argument_parser().parse_args(["map", "-f", "x.bam", "-o", "o", "--shard-bam"])
    assert args.shard_bam is True
    assert cli.build_argument_parser().parse_args(["map", "-f", "x.bam", "-o", "o"]).shard_bam is False


def test_the_binding_lists_the_new_entry_points():
    from kmer_mapper_amd import _lib
    assert _lib.FORMAT_MID_STREAM == 0x200
    assert "kmm_bam_header" in _lib.SIGNATURES and "kmm_bam_find_record_start" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "kmm.h")).read()
    assert "#define KMM_FORMAT_MID_STREAM 0x200" in header
