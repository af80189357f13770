"""GPU tests of a BAM file shared between ranks: kmm_bam_header, kmm_bam_find_record_start (k_bam_resync),
KMM_FORMAT_MID_STREAM and the rank share of kmm_map_bam, bgzf_ranges.rank_member_range_bam, `kmer_mapper map --shard-bam`.
Every share of a file is mapped in turn on one handle: the summed node counts are those of the whole-file call and of the
oracle (oracle.map_reads) on the SEQ an independent pure-Python reader takes from the same bytes, bit for bit; a boundary
guessed inside a record is an error of the share in front of it, with nothing mapped."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_bam_resync_on_the_cpu import FakeDev, _bam_file
from tests.test_gpu_bam import _bam, _expect, _records

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


@pytest.fixture(scope="module")
def base(oracle):
    """One index, ~2 000 ragged reads of 30-400 bp and the oracle's counts on them: shared, never changed."""
    from kmer_mapper_amd import synthetic as syn
    index, genome = syn.make_index(20000, seed=901)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 2000, 30, 400, seed=902)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    expect = oracle.map_reads(index, mx, bases, offs, 31, n_threads=4)[0]
    return dict(index=index, mx=mx, genome=genome, reads=reads, expect=expect)


def _map_share(dev, comp, share, **kw):
    """One rank's share (lo, head_skip, hi, tail_stop, n_ref) in one call, the way the CLI cuts it; returns the records mapped."""
    from kmer_mapper_amd import bgzf_ranges
    lo, s0, hi, s1, n_ref = share
    if (hi, s1) <= (lo, s0):
        return 0                                                    # an empty share: no map call
    buf = np.frombuffer(comp, np.uint8)
    end = bgzf_ranges.member_end(comp, hi) if s1 > 0 else hi
    mid = (lo, s0) > (0, 0)
    if mid:
        dev.set_param("bam_n_ref", n_ref)
    used, n = dev.map_bam(buf[lo:end], first=True, last=True, mid_stream=mid, head_skip=s0, tail_stop=s1 if s1 > 0 else None, **kw)
    assert used == end - lo
    return n


def _map_sharded(dev, comp, world, **kw):
    from kmer_mapper_amd import bgzf_ranges
    shares = [bgzf_ranges.rank_member_range_bam(dev, comp, r, world) for r in range(world)]
    assert all(shares[r][2:4] == shares[r + 1][0:2] for r in range(world - 1))      # neighbours agree
    return sum(_map_share(dev, comp, s, **kw) for s in shares), shares


def _map_whole(dev, comp, **kw):
    used, n = dev.map_bam(np.frombuffer(comp, np.uint8), first=True, last=True, **kw)
    assert used == len(comp)
    return n


@pytest.mark.parametrize("block,n_ref,on_boundaries", [(0x400, 0, False), (0x1F00, 3, False), (0xFF00, 0, False), (0x1F00, 3, True)])
def test_the_shares_partition_the_file_exactly(kmm, base, block, n_ref, on_boundaries):
    """Members of 0x400 bytes (a record spans many), 0x1F00 and 0xFF00, and members that end on record boundaries (skip 0, what
    htslib writes): for 2, 3 and 8 ranks the shares' counts sum to the whole file's and the oracle's, every record once."""
    reads = base["reads"]
    comp = _bam_file(reads, block, n_ref=n_ref, on_boundaries=on_boundaries)
    with kmm.DeviceIndex.from_index(base["index"], base["mx"]) as dev:
        assert _map_whole(dev, comp) == len(reads)
        assert np.array_equal(dev.get_node_counts(), base["expect"])
        truth = FakeDev(comp)                                       # the Python reader's record positions
        true_positions = {truth.position(int(p)) for p in truth.starts} | {(len(comp), 0)}
        for world in (2, 3, 8):
            dev.reset()
            r0 = dev.get_param("bam_records")
            n, shares = _map_sharded(dev, comp, world)
            assert n == len(reads), world
            assert dev.get_param("bam_records") - r0 == len(reads)
            assert np.array_equal(dev.get_node_counts(), base["expect"]), world
            assert all((lo, s0) in true_positions for lo, s0, *_ in shares[1:])             # true record starts, all of them
            if on_boundaries:
                assert all(s[1] == 0 for s in shares)
        assert dev.get_param("bgzf_carry_bytes") == 0


def test_long_records_take_the_doubling_path(kmm, base, oracle):
    """Three reads of 100-300 kb between short ones, and the examined bytes capped at 64 KiB: the first window of a boundary
    inside a long record holds no chain, the range finder doubles it (and the cap with it) until one does.  Counts exact."""
    from kmer_mapper_amd import reads_io
    joined = b"".join(base["reads"])                                # (~430 kb: the long reads are runs of it)
    reads = []
    for j, (a, L) in enumerate(((0, 100_000), (50_000, 300_000), (200_000, 180_000))):
        reads += [joined[a:a + L]] + base["reads"][20 * j:20 * j + 20]
    assert [len(r) for r in reads[::21]] == [100_000, 300_000, 180_000]
    comp = _bam(reads_io.bam_header(), _records(reads))
    expect, n_all = _expect(oracle, base["index"], base["mx"], comp)
    with kmm.DeviceIndex.from_index(base["index"], base["mx"]) as dev:
        dev.set_param("debug_bam_resync_kb", 64)
        answers = []
        find = dev.bam_find_record_start
        dev.bam_find_record_start = lambda a, n_ref: answers.append(find(a, n_ref)) or answers[-1]
        for world in (2, 4):
            dev.reset()
            n, _ = _map_sharded(dev, comp, world)
            assert n == n_all and np.array_equal(dev.get_node_counts(), expect), world
        assert any(m < 0 for m, _ in answers) and any(m >= 0 for m, _ in answers)     # "longer window", then a chain
        assert dev.get_param("debug_bam_resync_kb") == 64           # (the hook is put back)


@pytest.mark.parametrize("case", ["exclude_flags", "record_qual", "original_strand"])
def test_the_switches_of_the_route_compose(kmm, base, case):
    """The flag filter, the quality floor on QUAL and the read orientation apply to a share as to a file: three shares give the
    single-rank result with the same switch."""
    from kmer_mapper_amd import reads_io
    rng = np.random.default_rng(920)
    reads = base["reads"][:900]
    flags = [int(f) for f in rng.choice([0, 16, 99, 147, 256, 272, 2048, 2064, 4], size=len(reads))]
    quals = [bytes(rng.integers(2, 41, len(r), np.uint8)) if i % 7 else None for i, r in enumerate(reads)]
    comp = _bam(reads_io.bam_header([(b"chr1", 10 ** 6)]), _records(reads, flags=flags, quals=quals, ref_ids=[0] * len(reads)),
                block=0x1F00)
    with kmm.DeviceIndex.from_index(base["index"], base["mx"]) as dev:
        plain = (_map_whole(dev, comp), dev.get_node_counts().copy())
        if case == "exclude_flags":
            dev.set_param("bam_exclude_flags", 0x900)
        elif case == "record_qual":
            dev.set_param("use_record_qual", 1)
            dev.set_param("min_base_quality", 20)
        else:
            dev.set_param("original_strand", 1)
        dev.reset()
        n_one = _map_whole(dev, comp)
        one = dev.get_node_counts().copy()
        masked_one = dev.get_param("quality_masked_bases")
        dev.get_stats(reset=True)
        assert not np.array_equal(one, plain[1])                    # (the switch does something on this file)
        dev.reset()
        n, _ = _map_sharded(dev, comp, 3)
        assert n == n_one and np.array_equal(dev.get_node_counts(), one)
        assert dev.get_param("quality_masked_bases") == masked_one
        assert (n < plain[0]) == (case == "exclude_flags")


def test_a_wrong_guess_fails_the_share_in_front_of_it(kmm, base, oracle):
    """A forged chain of 600 records in a record's aux field, the member behind cut 10 bytes in front of it and the examined
    bytes capped inside it: kmm_bam_find_record_start answers the forgery's start — the documented limit.  The share in front
    of it then ends inside a record: KMM_ERR_MALFORMED, nothing mapped, the handle usable.  Without the cap the forgery is
    rejected and the two shares are exact."""
    from kmer_mapper_amd import _lib, bgzf_ranges, reads_io
    reads = base["reads"][:300]
    forged = reads_io.bam_record(b"ACGT" * 5, b"decoy", 0) * 600
    auxs = [b""] * len(reads)
    auxs[150] = b"ZZZ" + forged + b"\0" * 8
    payload = reads_io.bam_header() + b"".join(_records(reads, auxs=auxs))
    at = payload.index(forged) - 10
    front = reads_io.bgzf_members(payload[:at])
    comp = front + reads_io.bgzf_members(payload[at:]) + reads_io.BGZF_EOF
    expect, n_all = _expect(oracle, base["index"], base["mx"], comp)
    buf, m = np.frombuffer(comp, np.uint8), len(front)
    with kmm.DeviceIndex.from_index(base["index"], base["mx"]) as dev:
        dev.set_param("debug_bam_resync_kb", 16)
        assert dev.bam_find_record_start(buf[m:], 0) == (0, 10)
        end = bgzf_ranges.member_end(comp, m)
        used, n_rec = ctypes.c_int64(0), ctypes.c_int64(0)
        dev.set_param("bgzf_head_skip", 0)
        dev.set_param("bgzf_tail_stop", 10)
        rc = _lib.lib().kmm_map_bam(dev._h, buf.ctypes.data_as(ctypes.c_void_p), end, _lib.FORMAT_NEW_STREAM | _lib.FORMAT_LAST_CHUNK, 31,
                                    1000, 0, None, ctypes.byref(used), ctypes.byref(n_rec))
        assert rc == _lib.KMM_ERR_MALFORMED and (used.value, n_rec.value) == (0, 0)
        msg = _lib.lib().kmm_last_error().decode()
        assert "ends inside a record" in msg and "bgzf_tail_stop" in msg
        with pytest.raises(ValueError, match="ends inside a record"):
            dev.map_bam(buf[:end], first=True, last=True, tail_stop=10)
        assert not dev.get_node_counts().any()
        dev.set_param("debug_bam_resync_kb", 0)
        member, skip = dev.bam_find_record_start(buf[m:], 0)        # uncapped: the next true record start
        share0, share1 = (0, 0, m + member, skip, 0), (m + member, skip, len(comp), 0, 0)
        assert _map_share(dev, comp, share0) + _map_share(dev, comp, share1) == n_all
        assert np.array_equal(dev.get_node_counts(), expect)


def test_refusals(kmm, base):
    """KMM_FORMAT_MID_STREAM without "bam_n_ref", and without KMM_FORMAT_NEW_STREAM, are KMM_ERR_INVALID_ARG; so is the flag
    on a text stream.  Nothing is mapped."""
    from kmer_mapper_amd import _lib
    comp = _bam_file(base["reads"][:200], 0x1F00)
    buf = np.frombuffer(comp, np.uint8)
    L = _lib.lib()
    with kmm.DeviceIndex.from_index(base["index"], base["mx"]) as dev:
        def call(entry, flags):
            used, n_rec = ctypes.c_int64(0), ctypes.c_int64(0)
            return getattr(L, entry)(dev._h, buf.ctypes.data_as(ctypes.c_void_p), len(buf), flags, 31, 1000, 0, None, ctypes.byref(used),
                                     ctypes.byref(n_rec))
        assert dev.get_param("bam_n_ref") == -1
        assert call("kmm_map_bam", _lib.FORMAT_MID_STREAM | _lib.FORMAT_NEW_STREAM | _lib.FORMAT_LAST_CHUNK) == _lib.KMM_ERR_INVALID_ARG
        assert "bam_n_ref" in L.kmm_last_error().decode()
        dev.set_param("bam_n_ref", 0)
        assert dev.get_param("bam_n_ref") == 0
        assert call("kmm_map_bam", _lib.FORMAT_MID_STREAM | _lib.FORMAT_LAST_CHUNK) == _lib.KMM_ERR_INVALID_ARG
        assert "KMM_FORMAT_NEW_STREAM" in L.kmm_last_error().decode()
        assert call("kmm_map_bgzf", _lib.FORMAT_FASTQ | _lib.FORMAT_MID_STREAM | _lib.FORMAT_NEW_STREAM) == _lib.KMM_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            dev.set_param("bam_n_ref", -2)
        with pytest.raises(ValueError):
            dev.bam_find_record_start(buf, -1)
        assert not dev.get_node_counts().any()
        assert dev.map_bam(buf, first=True, last=True)[1] == 200    # (the handle is usable)


def test_the_header_is_found_over_several_members(kmm, base):
    """5 000 references in members of 0x1F00 bytes: n_ref and the first record's position are the Python reader's; a window that
    ends inside the header asks for a longer one; a header that ends with its member puts the first record at the next
    member, skip 0; a bad magic and a damaged member are refused; a stream in progress is not disturbed."""
    from kmer_mapper_amd import reads_io
    reads = base["reads"][:300]
    refs = [(b"contig_%05d_with_a_long_name" % i, 1000 + i) for i in range(5000)]
    header = reads_io.bam_header(refs, b"@HD\tVN:1.6\n" + b"@CO\tpadding\n" * 200)
    payload = header + b"".join(_records(reads))
    comp = reads_io.bgzf_members(payload, 0x1F00) + reads_io.BGZF_EOF       # the header ends inside a member
    truth = FakeDev(comp)
    buf = np.frombuffer(comp, np.uint8)
    with kmm.DeviceIndex.from_index(base["index"], base["mx"]) as dev:
        assert len(header) > 20 * 0x1F00 and truth.position(truth.hdr)[1] > 0
        assert dev.bam_header(buf) == (5000, *truth.position(truth.hdr))
        assert dev.bam_header(buf[:truth.position(truth.hdr)[0] - 1]) == (-1, 0, 0)
        assert dev.bam_header(buf[:30]) == (-1, 0, 0)
        split = _bam(header, _records(reads), block=0x1F00)         # the header in members of its own
        assert dev.bam_header(np.frombuffer(split, np.uint8)) == (5000, len(reads_io.bgzf_members(header, 0x1F00)), 0)
        with pytest.raises(ValueError, match="BAM header"):
            dev.bam_header(np.frombuffer(_bam(b"BAM\2" + header[4:], []), np.uint8))
        damaged = bytearray(comp)
        damaged[3000] ^= 0x55
        with pytest.raises(ValueError):
            dev.bam_header(np.frombuffer(bytes(damaged), np.uint8))
        # between two calls of a stream: the carry and n_ref of the stream stay
        half = truth.position(int(truth.starts[150]))[0]            # a member boundary in the middle of the records
        used, n0 = dev.map_bam(buf[:half], first=True, last=False)
        carry = dev.get_param("bgzf_carry_bytes")
        assert used == half and 0 < n0 < len(reads) and carry > 0
        assert dev.bam_header(buf)[0] == 5000 and dev.bam_find_record_start(buf[half:], 5000)[0] >= 0
        assert dev.get_param("bgzf_carry_bytes") == carry
        _, n1 = dev.map_bam(buf[used:], first=False, last=True)
        assert n0 + n1 == len(reads)


def test_cli_two_ranks_shard_one_bam_file(tmp_path):
    """Two ranks on the box's one GPU (the reduce over gloo), each process under its own time limit: `kmer_mapper map
    --shard-bam` on one BAM file, plain and with --exclude-flags 0x900 --original-strand; rank 0's .npy is the one-rank run's
    (tools/bam_shard_rehearsal.py)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tools", "bam_shard_rehearsal.py")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, script, "--prepare", str(tmp_path)], cwd=root,
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    env = dict(os.environ, KMM_DIST_BACKEND="gloo", MASTER_ADDR="127.0.0.1", MASTER_PORT="29673", WORLD_SIZE="2")
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, script, str(tmp_path)], cwd=root,
                              env=dict(env, RANK=str(i), LOCAL_RANK=str(i)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                              text=True) for i in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-1500:] for o in outs)
    assert outs[0].count("SAME AS ONE RANK") == 2 and "DIFFERS" not in outs[0], outs[0][-2000:]
    assert all("found its BAM record boundaries on the GPU" in o for o in outs)
