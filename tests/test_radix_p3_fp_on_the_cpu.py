"""CPU tier of pass 3's fingerprints: rx_p3_fp and rx_p3_candidates of csrc/kmm_radix_plan.hpp, compiled by themselves with
g++ (the header includes no HIP header).

k_rx_p3 keeps one byte of every LDS-resident key and a probe tests the bytes of its bucket's first five entries instead of
reading their keys; the key compare stays the arbiter.  So

  * rx_p3_candidates must never miss an entry whose byte equals the k-mer's (a missing bit is a wrong count) and never name an
    entry at or beyond min(cn, 5) (that byte belongs to another bucket, or is not there); a spurious bit below that costs
    one key compare, and
  * the byte must be independent of the bit rx_filter_slot tested — every k-mer that reaches pass 3 passed that test — and
    uniform: an absent k-mer then matches an entry it is compared with once in 256.  Held to 1/256 +- 20 % on more than
    10^6 compares (sampling error below 2 %; a fingerprint correlated with the slot would be off several-fold), on the
    flagship's shape: coarse partitions of 2^19 buckets at load factor 0.5, 19.6 % of the k-mers present.

The model also prints what the kernel's comments and profiles/p3_fingerprints/README.md quote: 8-byte key reads per probe and
trips of the entry loop per 256 probes (a wavefront's 64 lanes x 4 k-mers), today and with the fingerprint test."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
SH = 19            # buckets of a coarse partition: the slot filter's geometry
FP_ENTRIES = 5

SHIM = r"""
#include "kmm_radix_plan.hpp"
static_assert(RX_P3_FP_ENTRIES == 5, "five bytes of the two aligned words are always there");
static_assert(rx_p3_shape(RxP3Variant::W12_DIR16).fingerprints && rx_p3_fp_shapes() == 1, "one variant has the form");
extern "C" void fp_of(const uint64_t *quot, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i)
        out[i] = rx_p3_fp(quot[i]);
}
extern "C" void candidates(const uint64_t *f, const uint8_t *fp, const uint32_t *cn, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i)
        out[i] = rx_p3_candidates(f[i], fp[i], cn[i]);
}
extern "C" void slots_of(const uint32_t *b, const uint64_t *quot, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i)
        out[i] = rx_filter_slot(b[i], quot[i]);
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("radix_p3_fp")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = str(d / "shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, str(src),
                           "-o", so])
    L = ctypes.CDLL(so)
    L.fp_of.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.candidates.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.slots_of.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    return L


def fp_of(lib, quot):
    quot = np.ascontiguousarray(quot, dtype=np.uint64)
    out = np.empty(quot.shape[0], dtype=np.uint32)
    lib.fp_of(quot.ctypes.data, quot.shape[0], out.ctypes.data)
    assert out.max(initial=0) < 256
    return out.astype(np.uint8)


def candidates(lib, f, fp, cn):
    f = np.ascontiguousarray(f, dtype=np.uint64)
    fp = np.ascontiguousarray(fp, dtype=np.uint8)
    cn = np.ascontiguousarray(cn, dtype=np.uint32)
    out = np.empty(f.shape[0], dtype=np.uint32)
    lib.candidates(f.ctypes.data, fp.ctypes.data, cn.ctypes.data, f.shape[0], out.ctypes.data)
    return out


def slots_of(lib, b, quot):
    b = np.ascontiguousarray(b, dtype=np.uint32)
    quot = np.ascontiguousarray(quot, dtype=np.uint64)
    out = np.empty(b.shape[0], dtype=np.uint32)
    lib.slots_of(b.ctypes.data, quot.ctypes.data, b.shape[0], out.ctypes.data)
    return out


def fp_mirror(quot):
    """rx_p3_fp in Python integers (tests/test_gpu_radix_p3_fingerprints.py scans quotients with the same mirror)."""
    v = (quot ^ (quot >> 24) ^ (quot >> 48)) & 0xFFFFFF
    return ((v * 0xB5297B) >> 16) & 0xFF


def windows(byte_array, st):
    """The kernel's window: two aligned 32-bit words from byte st & ~3 on, shifted down by 8 (st & 3) bits each."""
    w32 = byte_array.view(np.uint32)
    w0, w1 = w32[st >> 2].astype(np.uint64), w32[(st >> 2) + 1].astype(np.uint64)
    by = (8 * (st & 3)).astype(np.uint64)
    lo = ((w0 | (w1 << np.uint64(32))) >> by) & np.uint64(0xFFFFFFFF)
    return lo | ((w1 >> by) << np.uint64(32))


def popcount5(m):
    return sum(((m >> j) & 1) for j in range(FP_ENTRIES)).astype(np.int64)


def test_fp_is_the_documented_function(lib):
    rng = np.random.default_rng(4201)
    quot = np.concatenate([rng.integers(0, 1 << 35, size=2000, dtype=np.uint64),
                           rng.integers(1 << 40, 1 << 63, size=2000, dtype=np.uint64) * np.uint64(2) + np.uint64(1),
                           np.array([0, 1, (1 << 24) - 1, 1 << 24, (1 << 48) | 5, (1 << 64) - 1], dtype=np.uint64)])
    got = fp_of(lib, quot)
    assert [int(g) for g in got] == [fp_mirror(int(q)) for q in quot]
    # uniform over the 256 values (10^6 quotients below 2^35: sigma of a share 6e-5)
    share = np.bincount(fp_of(lib, rng.integers(0, 1 << 35, size=10 ** 6, dtype=np.uint64)), minlength=256) / 1e6
    assert np.abs(share - 1 / 256).max() < 0.0005, (share.min(), share.max())


def test_candidates_against_a_byte_by_byte_loop(lib):
    """(a) random byte strings, every alignment of the bucket's first entry, 0 .. 8 entries, the fingerprints 0x00, 0x80 and
    0xFF (and 0x01 / 0x7F, the SWAR test's neighbours) among the values, byte strings of few distinct values so that
    equal bytes and runs of them are common."""
    rng = np.random.default_rng(4202)
    special = np.array([0x00, 0x80, 0xFF, 0x01, 0x7F, 0x81, 0xFE], dtype=np.uint8)
    n = 400000
    n_missing = n_beyond = n_spurious = n_exact = 0
    for alphabet in (special, np.arange(256, dtype=np.uint8), special[:3], np.array([0, 1], dtype=np.uint8)):
        store = alphabet[rng.integers(0, alphabet.shape[0], size=n + 16)]
        store = np.ascontiguousarray(store[:(n + 16) // 4 * 4])
        st = rng.integers(0, n, size=n, dtype=np.int64)
        st[:4000] = np.arange(4000) % 4 + 4 * rng.integers(0, n // 4, size=4000)       # every alignment, for sure
        cn = rng.integers(0, 9, size=n).astype(np.uint32)
        fp = alphabet[rng.integers(0, alphabet.shape[0], size=n)]
        f = windows(store, st)
        for j in range(FP_ENTRIES):                                              # the window is the bytes st .. st + 4
            assert np.array_equal((f >> np.uint64(8 * j)) & np.uint64(0xFF), store[st + j].astype(np.uint64))
        got = candidates(lib, f, fp, cn)
        lim = np.minimum(cn, FP_ENTRIES)
        want = np.zeros(n, dtype=np.uint32)
        for j in range(FP_ENTRIES):
            want |= ((store[st + j] == fp) & (j < lim)).astype(np.uint32) << np.uint32(j)
        n_missing += int(np.count_nonzero(want & ~got))
        n_beyond += int(np.count_nonzero(got >> lim))
        n_spurious += int(np.count_nonzero(got & ~want))
        n_exact += int(popcount5(want).sum())
    print("rx_p3_candidates: %d exact matches, %d spurious bits, %d missing, %d at or beyond min(cn, 5)"
          % (n_exact, n_spurious, n_missing, n_beyond))
    assert n_exact > 100000
    assert n_missing == 0
    assert n_beyond == 0


def test_false_candidates_once_in_256_after_the_slot_filter(lib):
    """(b) the model of the flagship's pass 3 with the committed functions: 2^21 buckets (four coarse partitions of 2^19) at
    load factor 0.5; absent k-mers that pass rx_filter_slot; 19.6 % of the k-mers present."""
    rng = np.random.default_rng(4203)
    n_buckets, n_entries = 1 << (SH + 2), 1 << (SH + 1)
    eb = np.sort(rng.integers(0, n_buckets, size=n_entries, dtype=np.int64))          # entries in bucket order
    eq = rng.integers(0, 1 << 35, size=n_entries, dtype=np.uint64)                    # 62-bit k-mers over a 28-bit modulo
    pstart = np.zeros(n_buckets + 1, dtype=np.int64)
    np.cumsum(np.bincount(eb, minlength=n_buckets), out=pstart[1:])
    fps = np.zeros((n_entries + 8 + 3) // 4 * 4, dtype=np.uint8)
    fps[:n_entries] = fp_of(lib, eq)
    slot_bits = np.zeros((n_buckets >> SH) * (3 << (SH - 1)), dtype=bool)
    part = lambda b: (b >> SH) * (3 << (SH - 1))
    slot_bits[part(eb) + slots_of(lib, eb & ((1 << SH) - 1), eq)] = True
    # absent k-mers: random bucket and quotient; those the slot filter passes reach pass 3
    n_absent = 6 * 10 ** 6
    ab = rng.integers(0, n_buckets, size=n_absent, dtype=np.int64)
    aq = rng.integers(0, 1 << 35, size=n_absent, dtype=np.uint64)
    passed = slot_bits[part(ab) + slots_of(lib, ab & ((1 << SH) - 1), aq)]
    assert abs(passed.mean() - 0.283) < 0.01
    ab, aq = ab[passed], aq[passed]
    st, cn = pstart[ab], (pstart[ab + 1] - pstart[ab]).astype(np.uint32)
    m_abs = candidates(lib, windows(fps, st), fp_of(lib, aq), cn)
    compared = int(np.minimum(cn, FP_ENTRIES).sum())
    equal_keys = 0
    for j in range(FP_ENTRIES):                      # (an absent k-mer that happens to equal an entry: none at 2^35 quotients)
        ok = j < cn
        equal_keys += int(np.count_nonzero(eq[np.where(ok, st + j, 0)][ok] == aq[ok]))
    matches = int(popcount5(m_abs).sum()) - equal_keys
    rate = matches / (compared - equal_keys)
    print("absent k-mers behind the slot filter: %d fingerprint matches in %d compares with unequal entries: 1 / %.1f"
          % (matches, compared - equal_keys, 1 / rate))
    assert compared >= 10 ** 6
    assert abs(rate - 1 / 256) <= 0.2 / 256
    # present k-mers: 0.196 of what pass 1 emits; the absent ones are 0.804 x the pass rate
    n_hit = int(round(ab.shape[0] * 0.196 / (0.804 * passed.mean())))
    he = rng.integers(0, n_entries, size=n_hit, dtype=np.int64)
    hb = eb[he]
    hst, hcn = pstart[hb], (pstart[hb + 1] - pstart[hb]).astype(np.uint32)
    m_hit = candidates(lib, windows(fps, hst), fps[he], hcn)
    own = he - hst
    assert np.all((own >= FP_ENTRIES) | (((m_hit >> np.minimum(own, 31).astype(np.uint32)) & 1) == 1))   # no false negative
    masks = np.concatenate([m_abs, m_hit])
    cns = np.concatenate([cn, hcn]).astype(np.int64)
    order = rng.permutation(masks.shape[0])
    masks, cns = masks[order], cns[order]
    cand = popcount5(masks)
    tail = np.maximum(cns - FP_ENTRIES, 0)
    n_grp = masks.shape[0] // 256
    grp = lambda a: a[:n_grp * 256].reshape(n_grp, 256)
    print("pass 3, %d probes (%.1f %% present): key reads per probe %.3f -> %.3f; trips per 256 probes %.2f -> %.2f; "
          "candidates per probe %.3f; probes with more than 5 entries %.4f %%"
          % (masks.shape[0], 100.0 * n_hit / masks.shape[0], cns.mean(), (cand + tail).mean(), grp(cns).max(axis=1).mean(),
             (grp(cand).max(axis=1) + grp(tail).max(axis=1)).mean(), cand.mean(), 100.0 * (cns > FP_ENTRIES).mean()))
    assert (cand + tail).mean() < 0.55 and cns.mean() > 1.1
