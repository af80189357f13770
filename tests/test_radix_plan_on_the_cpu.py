"""CPU tier of the radix path's host decisions: csrc/kmm_radix_plan.hpp — the fan-out of an index, the scratch layout of a
sub-batch, the split of a batch into sub-batches, the choice of the pass-3 kernel — compiled by itself with g++ (it includes
no HIP header) and checked against values worked out by hand, against an independent statement of every table's size
(RxView's comments in csrc/kmm_radix.hpp) and against the size formula launch_rx used before the layout had one home."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
u32, u64, i64, cint = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("radix_plan")
    src = d / "shim.cpp"
    src.write_text('#include "radix_plan_cpu_driver.hpp"\n')
    so = str(d / "shim.so")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.plan_geometry.argtypes = [u64, u64, cint, cint, cint, cint, ctypes.POINTER(i64)]
    lib.plan_choose_geometry.argtypes = [u64, u64, cint, cint, cint, cint, ctypes.POINTER(i64)]
    lib.plan_scratch.argtypes = [u32, u32, u32, ctypes.POINTER(u64)]
    lib.plan_split.argtypes = [i64, u32, i64, ctypes.POINTER(i64)]
    lib.plan_next_smaller_cap.argtypes = [i64, u32, i64]
    lib.plan_next_smaller_cap.restype = i64
    lib.plan_p3.argtypes = [cint, cint, cint, cint, u32, cint, ctypes.POINTER(cint)]
    lib.plan_view_bytes.argtypes = [u64, u64, cint]
    lib.plan_view_bytes.restype = u64
    lib.plan_min_units.argtypes = [u64, u64]
    lib.plan_min_units.restype = i64
    lib.plan_constants.argtypes = [ctypes.POINTER(i64)]
    return lib


GEO = ("w", "f2", "occ_shift", "PF", "F1", "F2")


def geometry(plan, modulo, S, filt, w, maxf=512, f2_force=-1):
    out = (i64 * 6)()
    return dict(zip(GEO, out)) if plan.plan_geometry(modulo, S, int(filt), w, maxf, f2_force, out) else None


def choose(plan, modulo, S, filt, w_force=None, f2_force=-1):
    out = (i64 * 6)()
    forced = w_force is not None
    return dict(zip(GEO, out)) if plan.plan_choose_geometry(modulo, S, int(filt), forced, w_force if forced else 0, f2_force, out) else None


TABLES = ("start1", "P1T", "S1T", "csum", "T1", "item_base", "work_base", "item_desc", "start2", "start2T", "ctrl", "queue")


def scratch(plan, NB, F1, F2):
    out = (u64 * 17)()
    plan.plan_scratch(NB, F1, F2, out)
    return dict(zip(TABLES + ("meta_bytes", "buf1_bytes", "buf2_bytes", "chunks", "max_items"), out))


def split(plan, n, X, cap):
    out = (i64 * 2)()
    plan.plan_split(n, X, cap, out)
    return out[0], out[1]


def p3(plan, w, fits_small, fits_mid, p16, max_slice, no_mid=False):
    out = (cint * 3)()
    v = plan.plan_p3(w, int(fits_small), int(fits_mid), int(p16), max_slice, int(no_mid), out)
    return v, out[0], out[1], bool(out[2])


def consts(plan):
    out = (i64 * 12)()
    plan.plan_constants(out)
    return dict(zip(("RX_B", "RX_CH", "RX_MAXF", "RX_IC", "RX_ECAP", "RX_ECAP_MID", "RX_ECAP_BIG", "P2F_LOGBITS", "P2F_KMAX",
                     "FLOOR", "CAP_MAX", "AGE"), out))


def test_constants(plan):
    """What the kernels, the tests' batch sizes and "radix_sub_batch_kmers" rely on."""
    assert consts(plan) == dict(RX_B=8192, RX_CH=256, RX_MAXF=512, RX_IC=1024, RX_ECAP=4096, RX_ECAP_MID=4608, RX_ECAP_BIG=8192,
                                P2F_LOGBITS=19, P2F_KMAX=64, FLOOR=2 ** 28, CAP_MAX=2 ** 32 - 2 * 8192, AGE=16)


@pytest.mark.parametrize("filt", [True, False])
def test_geometry_of_the_skew_cases(plan, filt):
    """Modulo 100 003, part_shift 4, fine_bits 4 (tests/skew_cases.py, _force in test_gpu_radix_skew.py): 6251 slices of 16
    buckets, 391 coarse partitions of 16 — with the filter and without it."""
    g = geometry(plan, 100003, 60000, filt, 4, 512, 4)
    assert g == dict(w=4, f2=4, occ_shift=0, PF=6251, F1=391, F2=16)
    assert geometry(plan, 100003, 0, filt, 4, 512, 4) == g           # (the entry count only matters beyond 2^19 buckets per coarse partition)


def test_geometry_of_a_large_index(plan):
    """Modulo 200 000 033 with 10^8 entries at 4096 buckets per slice, fan-outs up to 256: ceil(modulo / 4096) = 48 829
    slices, 16 bits of them -> 8 fine-partition bits, 2^20 buckets per coarse partition: one more than the filter's 2^19 bits
    of LDS, so with the filter one bit fewer (load factor 0.5 <= 0.75: one bit per bucket): 128 fine x 382 coarse partitions
    (382 > 256 is allowed for the filter's sake, up to 512); without it 256 x 191."""
    on = geometry(plan, 200000033, 10 ** 8, True, 12, 256)
    assert on == dict(w=12, f2=7, occ_shift=0, PF=48829, F1=382, F2=128)
    off = geometry(plan, 200000033, 10 ** 8, False, 12, 256)
    assert off == dict(w=12, f2=8, occ_shift=1, PF=48829, F1=191, F2=256)
    # the same index as kmm_index_create configures it: load factor 0.5 -> 2^11 buckets keep 1.3 x 1024 + 64 <= 4096 keys and
    # so do 2^12 (2727); 2^12 is where the search starts
    assert choose(plan, 200000033, 10 ** 8, True) == on
    assert choose(plan, 200000033, 10 ** 8, False) == off


def test_geometry_refusals(plan):
    assert geometry(plan, 2 ** 31, 1000, True, 12) is None             # pass 1 divides with a 32-bit remainder
    assert geometry(plan, 2 ** 31 - 1, 1000, True, 13) is not None
    assert geometry(plan, 2 ** 31 - 1, 1000, True, 12) is None         # 524 288 slices > 512 x 512
    assert geometry(plan, 100003, 1000, True, 14) is None
    assert geometry(plan, 100003, 1000, True, -1) is None
    assert geometry(plan, 100003, 1000, True, 13) is not None
    assert geometry(plan, 200000033, 10 ** 8, False, 12, 128) is None  # 48 829 slices > 128 x 128
    assert choose(plan, 2 ** 31, 1000, True) is None


def test_forced_fine_bits_stay_within_512(plan):
    """A forced f2 ("fine_bits", KMM_RX_F2): both fan-outs are at most 512 or the configuration is refused; whatever is
    configured covers every bucket and leaves the quotient of any 64-bit k-mer room above the w + f2 hash bits."""
    for modulo, w, f2, filt in itertools.product((2, 1009, 40009, 100003, 12011, 10 ** 7 + 19, 200000033, 452930477, 2 ** 31 - 1),
                                                 range(0, 14), range(0, 12), (True, False)):
        g = geometry(plan, modulo, modulo // 2, filt, w, 512, f2)
        if g is None:
            continue
        assert g["F1"] <= 512 and g["F2"] <= 512, (modulo, w, f2, g)
        assert g["w"] == w and g["f2"] <= f2 and g["F2"] == 1 << g["f2"]
        assert g["PF"] == -(-modulo // (1 << w)) and g["F1"] * g["F2"] >= g["PF"] > (g["F1"] - 1) * g["F2"]
        assert ((2 ** 64 - 1) // modulo) << (g["w"] + g["f2"]) < 2 ** 64
        assert g["occ_shift"] == max(0, g["w"] + g["f2"] - 19)
    assert geometry(plan, 200000033, 10 ** 8, True, 12, 512, 3) is None   # 6104 coarse partitions
    assert geometry(plan, 200000033, 10 ** 8, True, 12, 512, 10) is None  # 1024 fine partitions


def test_order_of_preference(plan):
    """kmm_index_create: <= 256 x 256 slices of 2^w buckets; 256 x 256 slices of 8192 buckets when their entries fit 4096
    keys; 512 x 512 slices of 4096 buckets; slices of 8192 buckets with up to 8192 keys, 256 x 256, then 512 x 512."""
    assert choose(plan, 40009, 3000, True)["w"] == 12
    assert choose(plan, 12011, 6000, True)["w"] == 12                  # load 0.5: 2^12 buckets hold 2727 keys
    assert choose(plan, 12011, 12011, True)["w"] == 11                 # load 1: 2^11
    sparse = choose(plan, 452930477, 10 ** 8, True)                    # 110 579 slices of 4096 > 256 x 256; load 0.22: 8192 x .22 x 1.3 fit
    assert (sparse["w"], sparse["PF"]) == (13, 55290) and sparse["F1"] <= 512 and sparse["F2"] <= 256
    dense = choose(plan, 452930477, 2 * 10 ** 8, True)                 # load 0.44: 4757 keys > 4096 -> 512 x 512 slices of 4096
    assert (dense["w"], dense["PF"]) == (12, 110579) and dense["F1"] <= 512 and dense["F2"] <= 512
    big = choose(plan, 2 ** 31 - 1, 10 ** 9, True)                     # 524 288 slices of 4096 > 512 x 512; load 0.47: 8192-key slices
    assert (big["w"], big["PF"]) == (13, 262144)
    assert choose(plan, 2 ** 31 - 1, 2 ** 31 - 1, True) is None        # load 1: 2^9 buckets per slice, far too many slices
    forced = choose(plan, 100003, 60000, True, w_force=4, f2_force=4)  # KMM_RX_W / KMM_RX_F2
    assert forced == dict(w=4, f2=4, occ_shift=0, PF=6251, F1=391, F2=16)
    assert choose(plan, 100003, 60000, True, w_force=14) is None       # a forced width is not replaced by another
    assert choose(plan, 100003, 60000, True, w_force=-1) is None       # ... nor a negative one taken as "not forced"


def _table_bytes(NB, F1, F2):
    """Bytes of every table, from RxView's comments (csrc/kmm_radix.hpp), in the order of TABLES."""
    chunks, items = -(-NB // 256), NB + F1 + 1
    return ((NB * (F1 + 1)) * 2, (F1 * (NB + 1)) * 4, (F1 * NB) * 2, (chunks * F1) * 4, F1 * 4, (F1 + 1) * 4, (F1 + 1) * 4,
            items * 8, (items * (F2 + 1)) * 2, ((F2 + 1) * items) * 2, 3 * 4, 2 * 8 * 128)


def _old_size_formula(NB, F1, F2):
    """launch_rx's size of the meta buffer before RxScratch: it took three tables of F1 + 1 words where the carve had one of F1
    words and two of F1 + 1 — exact unless 4 F1 is a multiple of 256, 256 bytes too many when it is."""
    a = lambda x: (x + 255) & ~255
    chunks, items = -(-NB // 256), NB + F1 + 1
    return (a(NB * (F1 + 1) * 2) + a(F1 * (NB + 1) * 4) + a(F1 * NB * 2) + a(chunks * F1 * 4) + 3 * a((F1 + 1) * 4) + a(items * 8) +
            a(items * (F2 + 1) * 2) + a(items * (F2 + 1) * 2 + 256) + a(64) + a(2048))


def test_scratch_layout(plan):
    NBs = (1, 2, 3, 255, 256, 257, 1000, 4096, 45777, 2 ** 19 - 2)
    Fs = (1, 2, 16, 63, 64, 65, 128, 191, 382, 391, 511, 512)
    for F1, F2 in itertools.product(Fs, (1, 16, 128, 256, 512)):
        prev = None
        for NB in NBs:
            s = scratch(plan, NB, F1, F2)
            offs = [s[t] for t in TABLES] + [s["meta_bytes"]]
            assert all(o % 256 == 0 for o in offs), (NB, F1, F2)
            assert offs[0] == 0
            for t, o, nxt, need in zip(TABLES, offs, offs[1:], _table_bytes(NB, F1, F2)):
                assert nxt - o >= need, (t, NB, F1, F2)                          # no table reaches into the next
            assert s["meta_bytes"] - s["ctrl"] == 256 + 2048                       # what launch_rx clears before a sub-batch
            assert s["chunks"] == -(-NB // 256) and s["max_items"] == NB + F1 + 1
            assert s["buf1_bytes"] == NB * 8192 * 8 and s["buf2_bytes"] == (NB + F1 + 1) * 8192 * 8
            old = _old_size_formula(NB, F1, F2)
            assert s["meta_bytes"] == (old if F1 % 64 else old - 256), (NB, F1, F2)
            if prev:                                                               # the largest sub-batch sizes the buffers for all
                assert all(s[k] >= prev[k] for k in ("meta_bytes", "buf1_bytes", "buf2_bytes")), (NB, F1, F2)
            prev = s
    for NB in range(1, 600):                                                       # ... step by step
        a, b = scratch(plan, NB, 391, 16), scratch(plan, NB + 1, 391, 16)
        assert b["meta_bytes"] >= a["meta_bytes"] and b["buf2_bytes"] > a["buf2_bytes"]


def test_sub_batches(plan):
    B = 8192
    for n, X, cap in itertools.product((0, 1, 2, 5, 1000, 32768, 32769, 45777, 524286, 524287, 10 ** 6, 3 * 10 ** 6), (1, 2),
                                       (1, B, 4 * B, 5 * B + 1, 10 ** 6, 2 ** 28, 2 ** 28 + 1, 187506688, 2 ** 31, 2 ** 32 - 2 * B)):
        n_sub, max_src = split(plan, n, X, cap)
        assert n_sub * max_src >= n, (n, X, cap)
        assert max_src >= 1 and (n_sub >= 1 or n == 0)
        if cap >= B * X:                                                           # the cap holds at least one block
            assert max_src * X * B <= cap, (n, X, cap)
            assert n == 0 or (n_sub - 1) * (cap // B // X) < n                     # and no more sub-batches than it takes
        # the next attempt of a call that ran out of memory: one sub-batch more.  ceil(n / (n_sub + 1)) blocks are fewer than
        # the cap's while the cap holds more blocks than there are sub-batches (n <= n_sub x cap_src): always, above the floor
        # of 32 768 blocks, for batches below 2^41 positions
        if n >= 2 and cap > 2 ** 28 and cap // B // X > n_sub:
            nxt = plan.plan_next_smaller_cap(n, X, n_sub)
            assert 2 ** 28 <= nxt < cap, (n, X, cap)
            assert nxt == max(2 ** 28, -(-n // (n_sub + 1)) * B * X)
            assert nxt == 2 ** 28 or split(plan, n, X, nxt)[0] == n_sub + 1


def test_sub_batches_at_the_floor(plan):
    """test_gpu_configs.py's out-of-memory route: 2.5 M reads of 150 bases = 45 777 blocks; one sub-batch needs 3.0 GB for
    pass 1 where the test hook allows 1.6 GB; the next smaller size, 22 889 blocks, lies below the floor of 2^28 slots, so the
    floor it is: two sub-batches of 22 889 blocks (1.5 GB).  With 100 MB allowed nothing at the floor fits: the call fails."""
    n, limit = -(-2_500_000 * 150 // 8192), 1_600_000_000
    assert n == 45777
    cap = 2 ** 32 - 2 * 8192
    n_sub, max_src = split(plan, n, 1, cap)
    assert (n_sub, max_src) == (1, 45777) and scratch(plan, max_src, 16, 16)["buf1_bytes"] > limit
    cap = plan.plan_next_smaller_cap(n, 1, n_sub)
    assert cap == 2 ** 28
    n_sub, max_src = split(plan, n, 1, cap)
    assert (n_sub, max_src) == (2, 22889) and 100_000_000 < scratch(plan, max_src, 16, 16)["buf1_bytes"] <= limit
    assert plan.plan_next_smaller_cap(n, 1, n_sub) == 2 ** 28                      # not below the floor: launch_rx gives up there


def test_pass_3_variants(plan):
    # the shapes of test_gpu_radix.py::test_slices_of_8192_buckets (modulo 40 009, part_shift 13: 5 slices)
    assert p3(plan, 13, True, True, True, 700)[1:] == (4096, 2, True)              # 3000 entries: every slice fits 4096 keys
    assert p3(plan, 13, False, True, True, 4500)[1:] == (4608, 2, True)            # 21 500 entries: load factor 0.54
    assert p3(plan, 13, False, False, True, 6300)[1:] == (8192, 1, False)          # 30 000 entries
    assert p3(plan, 13, False, True, True, 4500, no_mid=True)[1:] == (8192, 1, False)  # KMM_RX_NO_MID
    assert p3(plan, 13, True, True, True, 700, no_mid=True)[1:] == (4096, 2, True)
    # without the 16-bit directory in HBM (no memory for it): the 16-bit LDS directory needs max_slice <= 65535
    assert p3(plan, 13, True, True, False, 700)[1:] == (4096, 2, False)
    assert p3(plan, 13, False, True, False, 4500)[1:] == (4608, 2, False)
    assert p3(plan, 13, True, True, False, 70000)[1:] == (8192, 1, False)          # one heavy slice among sparse ones
    assert p3(plan, 13, False, True, False, 70000)[1:] == (8192, 1, False)
    for w, fs, fm, p16, nm in itertools.product(range(0, 13), (False, True), (False, True), (False, True), (False, True)):
        for mx in ((100, 65535) if p16 else (100, 65535, 65536, 10 ** 6)):
            assert p3(plan, w, fs, fm, p16, mx, nm)[1:] == (4096, 2, p16)          # up to 4096 buckets: always 4096 keys
    seen = {p3(plan, w, fs, fm, p16, mx, nm)[0] for w, fs, fm, p16, mx, nm in
            itertools.product((12, 13), (False, True), (False, True), (False, True), (100, 70000), (False, True)) if not (p16 and mx > 65535)}
    assert seen == set(range(7))                                                   # every variant is reachable, none beyond the table


def test_view_bytes_and_crossover(plan):
    """"radix_view_bytes": 4 bytes per bucket (+ 1) and 30 per entry (keys packed and raw, frequency, node, original position,
    hit count), 38 with the node-ordered list; an empty index still has one entry's worth.  The crossover never lies below 2^22."""
    assert plan.plan_view_bytes(12011, 6000, 0) == 12012 * 4 + 6000 * 30
    assert plan.plan_view_bytes(12011, 6000, 1) == 12012 * 4 + 6000 * 38
    assert plan.plan_view_bytes(7, 0, 1) == 8 * 4 + 38
    # a tiny index: 50 us of fixed cost against 1 / 60e9 - 6.5e-12 s saved per k-mer, 1.25 positions per k-mer: 6.15 M positions
    assert 6_100_000 <= plan.plan_min_units(12011, 6000) <= 6_200_000
    # profiles/r03/path_crossover.txt: 16-20 M positions at the 10 M-entry index, ~52 M at the 100 M-entry index
    assert 16_000_000 <= plan.plan_min_units(20000003, 10 ** 7) <= 20_000_000
    assert 45_000_000 <= plan.plan_min_units(200000033, 10 ** 8) <= 65_000_000
    assert all(plan.plan_min_units(m, s) >= 2 ** 22 for m, s in ((2, 0), (2, 1), (1009, 10 ** 9), (2 ** 31 - 1, 2 ** 31 - 1)))
