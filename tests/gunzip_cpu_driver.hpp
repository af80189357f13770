// The CPU driver of kmm_gpu_gunzip.hpp's pipeline for the tests (tests/test_gpu_gunzip_on_the_cpu.py builds it as a shared
// library, tests/gunzip_san_main.cpp as a sanitized executable): a whole stream through run_call in windows, the caller's loop
// of kmm_map_gzip.
#pragma once

#include "kmm_gpu_gunzip.hpp"

#include <cstring>
#include <vector>

// Windows end at cuts[0 .. n_cuts) (the last one = n).  Each call sees exactly comp[pos, end) (padded to 16 bytes only when
// shorter) and inflates at most call_cap bytes; the next call starts where it stopped, and the last window is called again
// while a call stopped at its size limit.  stats: chunks, false starts, continuations, members, calls, calls that hit the
// cap.  Returns 0, a kmm_gz::Err, -1 (backend), -2 (output larger than out_cap), -3 (a call went backwards).
extern "C" int gunzip_cpu(const uint8_t *comp, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t chunk_bytes, uint64_t call_cap,
                          uint8_t *out, uint64_t out_cap, uint64_t *out_n, uint64_t *stats)
{
    kmm_gunzip::CpuBackend be;
    kmm_gunzip::StreamState st;
    kmm_gunzip::CallStats cs;
    uint64_t pos = 0, w = 0, calls = 0, capped = 0;
    for (int i = 0; i < n_cuts; ++i) {
        const uint64_t end = cuts[i];
        const bool last = end == n;
        for (;;) {
            if (end <= pos && !last)
                break;
            const uint64_t len = end - pos;
            std::vector<uint8_t> win(len < 16 ? 16 : len, 0);
            if (len)
                memcpy(win.data(), comp + pos, len);
            be.in = win.data();
            be.n_pad = (uint32_t)win.size();
            be.n = len;
            kmm_gunzip::CallOut co;
            ++calls;
            if (kmm_gunzip::run_call(be, win.data(), len, last, chunk_bytes, call_cap, st, co, cs) != 0)
                return -1;
            if (co.err)
                return co.err;
            if (co.consumed > len)
                return -3;
            capped += co.hit_cap;
            if (w + co.n_out > out_cap)
                return -2;
            if (co.n_out)
                memcpy(out + w, be.out.data(), co.n_out);
            w += co.n_out;
            pos += co.consumed;
            be.arena.clear();
            if (!last || pos == n || (co.consumed == 0 && !co.hit_cap))
                break;
        }
        if (last)
            break;
    }
    *out_n = w;
    stats[0] = cs.chunks;
    stats[1] = cs.false_starts;
    stats[2] = cs.continuations;
    stats[3] = cs.members;
    stats[4] = calls;
    stats[5] = capped;
    return pos == n ? 0 : kmm_gz::E_INPUT;
}
