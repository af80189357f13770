"""CPU tier of the parameter table: csrc/kmm_params.hpp — the fields that are a stored parameter value (KmmKnobs), the counters
that are only read (KmmCounters) and the rows over them — compiled by itself with g++ (it includes no HIP header) and replayed
against tests/golden/param_contract.json, the answers of kmm_set_param / kmm_get_param recorded from the commit that still had
them as two if-chains (tools/record_param_contract.py): for every plain row, the same return code, the same message and the same
value read back, value by value.  The rows that need the handle are replayed on the GPU (test_gpu_param_contract.py)."""
import ctypes
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kmer_mapper_amd", "csrc")
i64, cint = ctypes.c_int64, ctypes.c_int


@pytest.fixture(scope="module")
def params(tmp_path_factory):
    d = tmp_path_factory.mktemp("params")
    alone = d / "alone.cpp"
    alone.write_text('#include "kmm_params.hpp"\n')                                    # the header by itself, before anything else
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + CSRC, str(alone)])
    src = d / "shim.cpp"
    src.write_text('#include "params_cpu_driver.hpp"\n')
    so = str(d / "shim.so")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "tests"), str(src), "-o", so])
    lib = ctypes.CDLL(so)
    lib.params_new.restype = ctypes.c_void_p
    lib.params_free.argtypes = [ctypes.c_void_p]
    lib.params_row_name.argtypes = lib.params_row_alias.argtypes = lib.params_row_has_hook.argtypes = [cint]
    lib.params_row_name.restype = lib.params_row_alias.restype = ctypes.c_char_p
    lib.params_set.argtypes = [ctypes.c_void_p, ctypes.c_char_p, i64, ctypes.c_char_p, cint]
    lib.params_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(i64), ctypes.c_char_p, cint]
    lib.params_bump_counters.argtypes = [ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def contract():
    with open(os.path.join(ROOT, "tests", "golden", "param_contract.json")) as f:
        return json.load(f)


class Handle:
    """A bare KmmKnobs + KmmCounters; set / get answer as the fixture records them: [code, message or None], [code, value or message]."""

    def __init__(self, lib):
        self.lib, self.h, self.err = lib, lib.params_new(), ctypes.create_string_buffer(256)

    def close(self):
        self.lib.params_free(self.h)

    def set(self, name, value):
        rc = self.lib.params_set(self.h, name.encode(), value, self.err, 256)
        return [rc, self.err.value.decode() if rc else None]

    def get(self, name):
        v = i64(0)
        rc = self.lib.params_get(self.h, name.encode(), ctypes.byref(v), self.err, 256)
        return [rc, self.err.value.decode() if rc else v.value]


def _names(lib):
    rows = [(lib.params_row_name(i).decode(), lib.params_row_alias(i)) for i in range(lib.params_n_rows())]
    return [n for n, _ in rows] + [a.decode() for _, a in rows if a]


def test_names_and_aliases_are_unique(params, contract):
    names = _names(params)
    assert len(names) == len(set(names))
    assert len(names) > 50 and "debug_ring_slot_kb" in names and "debug_bgzf_ring_slot_kb" in names
    assert set(names) <= set(contract["names"])                                        # no name the chains did not know
    assert not any(params.params_row_has_hook(i) for i in range(params.params_n_rows()))  # plain: nothing here needs the handle


def test_plain_rows_answer_as_recorded(params, contract):
    """Every plain row's part of the recorded walk.  A refused value leaves the field as it was; an accepted one reads back as
    recorded (a write-only name: the recorded refusal of the get)."""
    compared = 0
    for name in _names(params):
        h = Handle(params)
        try:
            for value, want_set, want_get in contract["walk"][name]:
                before = h.get(name)
                assert h.set(name, value) == want_set, (name, value)
                got = h.get(name)
                if want_set[0] != 0:
                    assert got == before, (name, value)
                if want_set[0] == 0 or want_get[0] != 0:                             # (a default the handle's creation sets — "host_pack_threads",
                    assert got == want_get, (name, value)                              # "radix_min_units" — is not the bare struct's)
                compared += 1
        finally:
            h.close()
    assert compared == len(_names(params)) * len(contract["probes"])


def test_defaults_of_the_bare_structs(params, contract):
    """What a get on an untouched handle gave, but for the two fields kmm_index_create computes."""
    h = Handle(params)
    try:
        for name in _names(params):
            if name not in ("host_pack_threads", "radix_min_units"):
                assert h.get(name) == contract["defaults"][name], name
        assert h.get("host_pack_threads") == [0, 0] and h.get("radix_min_units") == [0, 0]
    finally:
        h.close()


def test_counters_read_their_own_field_and_take_no_set(params):
    h = Handle(params)
    try:
        params.params_bump_counters(h.h)
        seen = [h.get(n)[1] for n in _names(params) if h.set(n, 0) == [-1, "unknown parameter '%s'" % n]]
        assert len(seen) == 26 and sorted(seen) == list(range(100, 126))               # 26 counters, each its own field
    finally:
        h.close()


def test_under_address_and_undefined_behaviour_sanitizers(params, contract, tmp_path):
    """The same driver as an executable with ASan + UBSan (tests/params_san_main.cpp; host code, nothing sanitized is loaded into
    Python): every row, by name and alias, over the whole probe list — the conversions to the fields' widths included — answers
    as the shared library does."""
    exe = str(tmp_path / "params_san")
    src = os.path.join(ROOT, "tests", "params_san_main.cpp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I" + CSRC, "-I" + os.path.join(ROOT, "tests"), src, "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True)
    if build.returncode != 0 and "cannot find" in build.stderr and ("asan" in build.stderr or "ubsan" in build.stderr):
        pytest.skip("no sanitizer runtime on this box: " + build.stderr[-200:])         # (the linker misses libasan / libubsan)
    assert build.returncode == 0, build.stderr
    probes = [str(v) for v in contract["probes"]]
    run = subprocess.run([exe] + probes, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    h = Handle(params)
    try:
        params.params_bump_counters(h.h)
        want = []
        for name in [n for i in range(params.params_n_rows()) for n in (params.params_row_name(i), params.params_row_alias(i)) if n]:
            for v in contract["probes"]:
                s, g = h.set(name.decode(), v), h.get(name.decode())
                want.append("%s %d %d %d %s" % (name.decode(), v, s[0], g[0], g[1]))
    finally:
        h.close()
    assert run.stdout.splitlines() == want
