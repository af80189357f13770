"""GPU tier of the forged-stream tests (tests/deflate_forge.py; CPU tier: test_inflate_vs_zlib_on_the_cpu.py): FASTQ from
`synthetic`, forged into BGZF members of every shape the CPU tier names — literal-only blocks, the worst subtable shapes,
deep random codes, repeat codes across HLIT -> HDIST, runs of 258, far distances, stored and fixed blocks — several hundred
members per file, mapped by kmm_map_bgzf, as one plain gzip stream by kmm_map_gzip, and as a BAM by kmm_map_bam, on both
lookup paths: the counts equal the oracle's over zlib's bytes.  A refused member raises and leaves nothing mapped."""
import random
import zlib

import numpy as np
import pytest

from tests import deflate_forge as F

pytestmark = pytest.mark.gpu

SHAPES = ["random", "literal_only", "dist_1040", "lit_404", "runs258", "maxdist", "rle_plain", "hclen19", "stored_mix",
          "random", "random"]


@pytest.fixture(scope="module")
def kmm():
    from kmer_mapper_amd import _lib
    assert _lib.device_count() >= 1, "GPU tests need a HIP device"
    import kmer_mapper_amd.engine as engine
    return engine


def forge_blocks(rng, piece, shape):
    """Blocks that inflate to `piece`, in the given shape."""
    if shape == "random":
        return F.random_stream(rng, piece)[1]
    if shape == "literal_only":
        return F.payload_stream(piece, "literals")[1]
    if shape in ("runs258", "maxdist"):
        return F.payload_stream(piece, shape, splits=[len(piece) // 2], kinds=["dynamic", "fixed"])[1]
    if shape == "stored_mix":
        return F.payload_stream(piece, "greedy", splits=sorted(rng.randrange(len(piece) + 1) for _ in range(3)),
                                kinds=["dynamic", "stored", "fixed", "stored"])[1]
    toks = F.parse(piece, "greedy")
    lit, dist = F.code_for(toks, "dynamic")
    kw = {}
    if shape == "dist_1040":
        order = list(range(30))
        rng.shuffle(order)
        dist = F.lengths_from_counts(F.WORST_DIST_COUNTS if rng.random() < 0.5 else F.worst_code(30, 5)[1], 30, order)
    elif shape == "lit_404":
        lf = [0] * 286
        for t in toks:
            lf[t if isinstance(t, int) else F.len_symbol(t[1])[0]] += 1
        lf[256] = 1
        lit = F._fill(F.worst_code(286, 8)[1], 286, [i for i in range(286) if lf[i]], rng)
    elif shape == "rle_plain":
        kw["rle"] = "plain"
    elif shape == "hclen19":
        kw["hclen"] = 19
    return [F.Block("dynamic", toks, final=True, lit_lens=lit, dist_lens=dist, **kw)]


def forged_members(rng, raw, max_piece=9000):
    """raw cut into pieces, each forged into a BGZF member (its shape in turn from SHAPES): (members, blocks per member)."""
    members, blocks, p, i = [], [], 0, 0
    while p < len(raw):
        n = rng.randint(1, max_piece)
        piece = raw[p:p + n]
        b = forge_blocks(rng, piece, SHAPES[i % len(SHAPES)])
        s = F.stream(b)
        assert zlib.decompress(s, -15) == piece
        members.append(F.bgzf_member(s, piece))
        blocks.append(b)
        p += n
        i += 1
    return members, blocks


def _fastq(reads, rng):
    qual = np.frombuffer(b"FFFF:,#@+I", dtype=np.uint8)
    return b"".join(b"@read%d forged\n" % i + r + b"\n+\n" + bytes(rng.choice(qual, size=len(r))) + b"\n" for i, r in enumerate(reads))


@pytest.fixture(scope="module")
def case(oracle):
    from kmer_mapper_amd import synthetic as syn
    index, genome = syn.make_index(20000, seed=951)
    mx = index.max_node_id()
    bases, offs = syn.make_ragged_reads(genome, 6000, 0, 260, seed=952)
    reads = [bases[offs[i]:offs[i + 1]].tobytes() for i in range(len(offs) - 1)]
    expect, _ = oracle.map_reads(index, mx, bases, offs, 31, n_threads=4)
    raw = _fastq(reads, np.random.default_rng(953))
    rng = random.Random(954)
    members, blocks = forged_members(rng, raw)
    return dict(index=index, mx=mx, reads=reads, expect=expect, raw=raw, members=members, blocks=blocks, rng=rng)


@pytest.fixture(scope="module")
def cat():
    return F.catalogue()


def test_forged_bgzf_members_give_the_oracles_counts(kmm, case):
    from kmer_mapper_amd import _lib
    from tests.test_gpu_bgzf import _feed
    comp = F.bgzf_file(case["members"])
    assert len(case["members"]) >= 200
    got = bytearray()
    rest = comp
    while rest:
        d = zlib.decompressobj(31)
        got += d.decompress(rest)
        rest = d.unused_data
    assert bytes(got) == case["raw"]
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        for path in (2, 0):
            dev.set_param("path", path)
            for step in (1 << 30, 100_003):
                dev.reset()
                assert _feed(dev, comp, _lib.FORMAT_FASTQ, 31, step) == len(case["reads"])
                assert np.array_equal(dev.get_node_counts(), case["expect"]), (path, step)


def test_forged_plain_gzip_gives_the_oracles_counts(kmm, case):
    """The same blocks as ONE deflate stream in one gzip member, and as concatenated gzip members (kmm_map_gzip)."""
    from tests.test_gpu_gzip import _feed
    all_blocks = []
    for b in case["blocks"]:
        for x in b:
            x.final = False
        all_blocks += b
    all_blocks[-1].final = True
    one = F.gzip_member(F.stream(all_blocks), case["raw"], fname=b"reads.fq")
    for b in case["blocks"]:
        b[-1].final = True
    many = b"".join(F.gzip_member(F.stream(b), F.expand(b)) for b in case["blocks"])
    assert zlib.decompress(one, 31) == case["raw"]
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        for path in (2, 0):
            dev.set_param("path", path)
            for cuts in (None, [len(one) // 3, 2 * len(one) // 3]):
                dev.reset()
                assert _feed(dev, one, cuts=cuts) == len(case["reads"])
                assert np.array_equal(dev.get_node_counts(), case["expect"]), (path, cuts)
            dev.reset()
            assert _feed(dev, many, cuts=[len(many) // 2]) == len(case["reads"])
            assert np.array_equal(dev.get_node_counts(), case["expect"]), (path, "members")


REFUSED = ["one_dist_code_len2", "two_dist_codes_len3", "rle18_overshoots", "fixed_dist30", "dist32768_at_32k_minus1"]


@pytest.mark.parametrize("name", REFUSED)
def test_a_refused_member_raises_and_leaves_nothing_mapped(kmm, case, cat, name):
    """One member of a refused shape among the forged ones: ValueError, counts still zero, and the handle maps the good file."""
    from kmer_mapper_amd import _lib
    from tests import test_gpu_bgzf, test_gpu_gzip
    blocks, tail = cat[name]
    raw = F.stream(blocks, tail)
    with pytest.raises(zlib.error):
        zlib.decompress(raw, -15)
    data = F.expand(blocks) or b""
    good = F.bgzf_file(case["members"])
    k = len(case["members"]) // 2
    bad = F.bgzf_file(case["members"][:k] + [F.bgzf_member(raw, data)] + case["members"][k:])
    bad_gz = b"".join(F.gzip_member(F.stream(b), F.expand(b)) for b in case["blocks"][:20]) + F.gzip_member(raw, data)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        dev.reset()
        with pytest.raises(ValueError):
            test_gpu_bgzf._feed(dev, bad, _lib.FORMAT_FASTQ, 31, 1 << 30)
        assert not dev.get_node_counts().any()
        dev.reset()
        with pytest.raises(ValueError):
            test_gpu_gzip._feed(dev, bad_gz)
        assert not dev.get_node_counts().any()
        dev.reset()
        assert test_gpu_bgzf._feed(dev, good, _lib.FORMAT_FASTQ, 31, 1 << 30) == len(case["reads"])
        assert np.array_equal(dev.get_node_counts(), case["expect"])


def test_forged_bam_members(kmm, case, oracle):
    """A BAM whose BGZF members are forged in every shape (kmm_map_bam)."""
    from kmer_mapper_amd import reads_io
    from tests.test_gpu_bam import _expect, _feed
    recs = [reads_io.bam_record(r, b"r%d" % i, 4) for i, r in enumerate(case["reads"][:3000])]
    body = reads_io.bam_header() + b"".join(recs)
    members, _ = forged_members(random.Random(961), body)
    comp = F.bgzf_file(members)
    expect, n = _expect(oracle, case["index"], case["mx"], comp)
    with kmm.DeviceIndex.from_index(case["index"], case["mx"]) as dev:
        for path in (2, 0):
            dev.set_param("path", path)
            for step in (1 << 40, 77_777):
                dev.reset()
                assert _feed(dev, comp, step) == n
                assert np.array_equal(dev.get_node_counts(), expect), (path, step)
