"""CPU tier of pass 2's slot filter: rx_filter_slot of csrc/kmm_radix_plan.hpp, compiled by itself with g++ (the header
includes no HIP header), on random tables at load factor 0.5 — the shape of the flagship's coarse partitions: 2^19 buckets,
2^18 entries.  Every pair of buckets shares 3 bits and an entry sets the one its (bucket parity, quotient) selects, so

  * an entry's own bit is always set (no false negative: the node counts cannot change), and
  * an absent k-mer passes with probability 1 - e^-1/3 = 0.283: its bucket pair holds Poisson(1) entries, each of which chose
    the k-mer's bit with probability 1/3.  The bucket bitmap on the same table passes 1 - e^-1/2 = 0.393.

The pass rate is held to 0.283 +- 0.01 on 10^6 absent keys (the standard deviation of the estimate is 0.0005; the 2^18
entries of the table itself move it by ~0.001) for three kinds of quotients: random below 2^35 (the flagship: 62-bit k-mers
over a 28-bit modulo), quotients that share their low 16 bits, and quotients of 2^40 and more — callers may hand over any
uint64 value."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
SH = 19

SHIM = r"""
#include "kmm_radix_plan.hpp"
static_assert(rx_filter_slot(0u, 0ull) < 3u, "usable in constant expressions");
static_assert(P2F_SLOT_WORDS * 32 == 3 << (P2F_LOGBITS - 1), "3 bits per bucket pair");
static_assert(P2F_SLOTS % 2 == 0 && P2F_SLOTS >= 5632 && P2F_SLOTS <= 6144, "sort-buffer slots beside the filter");
extern "C" void slots_of(const uint32_t *b, const uint64_t *quot, int64_t n, uint32_t *out)
{
    for (int64_t i = 0; i < n; ++i)
        out[i] = rx_filter_slot(b[i], quot[i]);
}
extern "C" void slot_constants(int64_t *out)
{
    out[0] = P2F_LOGBITS;
    out[1] = P2F_SLOT_WORDS;
    out[2] = P2F_SLOTS;
}
extern "C" int geometry_has_slot_filter(uint64_t modulo, uint64_t S, int w, int f2_force)
{
    const auto g = rx_geometry(modulo, S, true, w, RX_MAXF, f2_force);
    return g ? (g->slot_filter ? 1 : 0) | (g->occ_shift << 1) : -1;
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("radix_filter_slots")
    src = d / "shim.cpp"
    src.write_text(SHIM)
    so = str(d / "shim.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC, str(src),
                           "-o", so])
    L = ctypes.CDLL(so)
    L.slots_of.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.slot_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    L.geometry_has_slot_filter.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]
    return L


def slots_of(lib, b, quot):
    b = np.ascontiguousarray(b, dtype=np.uint32)
    quot = np.ascontiguousarray(quot, dtype=np.uint64)
    out = np.empty(b.shape[0], dtype=np.uint32)
    lib.slots_of(b.ctypes.data, quot.ctypes.data, b.shape[0], out.ctypes.data)
    return out


def quotients(kind, rng, n):
    if kind == "below 2^35":
        return rng.integers(0, 1 << 35, size=n, dtype=np.uint64)
    if kind == "same low 16 bits":
        return (rng.integers(0, 1 << 19, size=n, dtype=np.uint64) << np.uint64(16)) | np.uint64(0xBEEF)
    assert kind == "2^40 and more"
    return rng.integers(1 << 40, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)


def test_constants(lib):
    out = (ctypes.c_int64 * 3)()
    lib.slot_constants(out)
    logbits, words, slots = out
    assert logbits == SH and words * 32 == 786432 and words * 4 == 96 * 1024
    # the kernel's LDS: filter + sort buffer + 17 712 bytes of tables (fan-outs beyond 128) within a workgroup's 160 KB
    assert words * 4 + slots * 8 + 17712 <= 163840


@pytest.mark.parametrize("kind", ["below 2^35", "same low 16 bits", "2^40 and more"])
def test_no_false_negatives_and_the_derived_pass_rate(lib, kind):
    rng = np.random.default_rng(4100 + len(kind))
    n_buckets, n_entries, n_absent = 1 << SH, 1 << (SH - 1), 10 ** 6
    eb = rng.integers(0, n_buckets, size=n_entries, dtype=np.uint32)
    eq = quotients(kind, rng, n_entries)
    es = slots_of(lib, eb, eq)
    assert es.max() < 3 << (SH - 1)
    assert np.array_equal(es // 3, eb >> 1)                     # slot = 3 (b >> 1) + r, r in 0 .. 2
    bits = np.zeros(3 << (SH - 1), dtype=bool)
    bits[es] = True
    assert bits[slots_of(lib, eb, eq)].all()                    # an entry's own bit: no false negative
    # r is well mixed: the three bits of a pair are chosen equally often (sigma of a share: 0.0009)
    share = np.bincount(es % 3, minlength=3) / n_entries
    assert np.abs(share - 1 / 3).max() < 0.005, share
    # absent keys: random buckets, quotients of the same kind (a key that happens to equal an entry passes, as it should;
    # at most 10^6 x 2^18 / (2^19 x 2^19) = one in a million of them)
    ab = rng.integers(0, n_buckets, size=n_absent, dtype=np.uint32)
    aq = quotients(kind, rng, n_absent)
    rate = bits[slots_of(lib, ab, aq)].mean()
    occupied = np.zeros(n_buckets, dtype=bool)
    occupied[eb] = True
    rate_bitmap = occupied[ab].mean()
    print("%s: slot filter passes %.4f (derived %.4f), bucket bitmap %.4f (derived %.4f)"
          % (kind, rate, 1 - math.exp(-1 / 3), rate_bitmap, 1 - math.exp(-0.5)))
    assert abs(rate - 0.283) <= 0.01
    assert abs(rate_bitmap - 0.393) <= 0.01


def test_which_geometries_get_the_slot_filter(lib):
    """Coarse partitions of exactly 2^19 buckets at one bit per bucket — the flagship (modulo 200 000 033, 10^8 entries),
    configs[1] — and nothing else: smaller partitions and tables at one bit per 2 or 4 buckets keep the bitmap."""
    g = lib.geometry_has_slot_filter
    assert g(200000033, 100000000, 12, -1) == 1                 # for_filter: f2 = 7
    assert g(20000003, 10000000, 12, -1) == 1
    assert g(3000017, 300000, 12, 7) == 1
    assert g(3000017, 300000, 11, 8) == 1
    assert g(3000017, 300000, 12, 8) == 0 | (1 << 1)            # 2 buckets per bit
    assert g(3000017, 300000, 12, 9) == 0 | (2 << 1)            # 4
    assert g(3000017, 300000, 12, 6) == 0                       # 2^18 buckets per coarse partition
    assert g(40009, 3000, 12, -1) == 0
