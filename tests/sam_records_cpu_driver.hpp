// The CPU driver of the raw form of the SAM keep ("record_sam") for the tests (tests/test_sam_records_on_the_cpu.py
// builds it as a shared library, tests/sam_records_san_main.cpp as a sanitized executable): a SAM stream in windows with a carry,
// as sam_cpu_driver.hpp feeds one; per window the shared source of kmm_sam.hpp — the write walk with its span sink
// (cpu_raw_spans), the keep predicate, the destinations and every lane's share of the copy (cpu_raw_keep) — into a keep queue
// of exactly the size the caller expects, whose tail moves from window to window.  The entries (hits, windows) are the caller's:
// one per selected record of the stream, in file order.
#pragma once

#include "select_cpu_driver.hpp" // (SelectTables: the selection as the front ends take it)

#include <cstddef>
#include <cstring>
#include <new>
#include <vector>

// A buffer of exactly n bytes at a 16-byte aligned address: what lies behind it is the sanitizer's.
struct AlignedBytes {
    uint8_t *p;
    size_t n;
    AlignedBytes(size_t n_, int fill) : p((uint8_t *)::operator new(n_ ? n_ : 1, std::align_val_t(16))), n(n_) { memset(p, fill, n_ ? n_ : 1); }
    ~AlignedBytes() { ::operator delete(p, std::align_val_t(16)); }
    AlignedBytes(const AlignedBytes &) = delete;
    AlignedBytes &operator=(const AlignedBytes &) = delete;
};

// Windows end at cuts[0 .. n_cuts) (the last one = n), each copied into a buffer of exactly its size; a final line without its
// newline gets one.  mode: "record_sam" 1 / 2.  rules .. n_names: SelectTables.  hits / windows: n_entries entries (windows null:
// mode 1 of the record-hits mode); rule3: min_hits, min_permille, invert.  The queue holds tail0 + out_n bytes, all `fill`; out
// gets its last out_n bytes.  text: the two-line FASTA of the selected records (text_cap bytes at least).
// stats: [0] records, [1] excluded, [2] header lines, [3] kept bytes, [4] kept records, [5] text bytes, [6] records flipped,
// [7] entries used, [8] calls.
// Returns 0; -3 a malformed line; -4 more selected records than entries; -5 the kept bytes pass out_n (nothing is copied then) or
// the text passes text_cap; -7 a byte in front of tail0 was written.
extern "C" int sam_raw_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, int mode, int orig,
                           uint32_t lanes, const uint64_t *rules, const int64_t *iv3, const uint8_t *names, const uint32_t *name_off,
                           uint32_t n_names, const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const uint32_t *rule3,
                           int fill, uint64_t tail0, uint8_t *out, uint64_t out_n, uint8_t *text, uint64_t text_cap, uint64_t *stats)
{
    SelectTables tb(rules, iv3, names, name_off, n_names);
    const RkRule rule = {rule3[0], rule3[1], rule3[2]};
    for (int i = 0; i < 9; ++i)
        stats[i] = 0;
    AlignedBytes queue((size_t)(tail0 + out_n), fill);
    uint64_t pos = 0, tail = tail0, entry = 0, w = 0;
    std::vector<uint8_t> carry;
    for (int i = 0; i < n_cuts; ++i) {
        const uint64_t end = cuts[i];
        if (end < pos)
            continue;
        const bool last = end == n;
        std::vector<uint8_t> win(carry);
        win.insert(win.end(), data + pos, data + end);
        if (last && !win.empty() && win.back() != 10)
            win.push_back(10);
        kmm_sam::Totals t;
        kmm_sam::cpu_chunk<false>(win.data(), win.size(), excl, nullptr, t, nullptr, false, nullptr, lanes, &tb.sel);
        ++stats[8];
        if (t.err != kmm_sam::NONE)
            return -3;
        if (entry + t.recs > n_entries)
            return -4;
        if (w + t.out_bytes > text_cap)
            return -5;
        std::vector<uint8_t> exact(t.out_bytes); // (exactly the totals' size)
        kmm_sam::CpuRaw r;
        kmm_sam::cpu_raw_spans(win.data(), win.size(), excl, mode, exact.data(), r, orig != 0, lanes, &tb.sel);
        if (t.out_bytes)
            memcpy(text + w, exact.data(), exact.size());
        w += t.out_bytes;
        const uint32_t *h = hits ? hits + entry : nullptr, *wn = windows ? windows + entry : nullptr;
        uint64_t sum = 0;
        for (const kmm_sam::RawSpan &sp : r.spans)
            sum += kmm_sam::raw_kept_len(sp, r.tot.consumed, h, wn, t.recs, rule);
        if (tail + sum > tail0 + out_n)
            return -5;
        uint64_t kept_recs = 0;
        const uint64_t kept = kmm_sam::cpu_raw_keep(win.data(), r, h, wn, t.recs, rule, queue.p, tail, lanes, &kept_recs);
        tail += kept;
        entry += t.recs;
        stats[0] += t.recs;
        stats[1] += t.excluded;
        stats[2] += t.headers;
        stats[3] += kept;
        stats[4] += kept_recs;
        stats[6] += r.reversed;
        carry.assign(win.begin() + (std::ptrdiff_t)t.consumed, win.end());
        pos = end;
    }
    stats[5] = w;
    stats[7] = entry;
    for (uint64_t i = 0; i < tail0; ++i)
        if (queue.p[i] != (uint8_t)fill)
            return -7;
    if (out_n)
        memcpy(out, queue.p + tail0, (size_t)out_n);
    return 0;
}

// Where rk_span's head, middle and tail meet: every residue of the source start and of the destination start modulo 16, lengths
// 1 .. max_len, `lanes` lanes one after the other (raw_copy_span).  The source lies in a buffer of exactly its size, the queue in
// one that ends with the span.  Per span: the queue filled with 0x00 and with 0xFF equals the source inside and the fill in
// front; and every byte is written exactly once — each lane's share goes into a zeroed queue of its own, the bytes it made
// non-zero are counted (no source byte is zero), and every count inside the span must be 1.  Returns the number of spans that
// fail any of it.
extern "C" uint64_t sam_raw_copy_sweep(uint32_t lanes, uint32_t max_len)
{
    uint64_t bad = 0;
    for (uint32_t a = 0; a < 16; ++a)
        for (uint32_t b = 0; b < 16; ++b)
            for (uint32_t len = 1; len <= max_len; ++len) {
                AlignedBytes src(a + len, 0);
                for (uint32_t i = 0; i < a + len; ++i)
                    src.p[i] = (uint8_t)(1u + (i * 7u + a + 3u * b + len) % 255u);
                kmm_sam::RawSpan sp;
                sp.start = a;
                sp.len = len;
                sp.entry = 0;
                bool ok = true;
                for (int fill = 0; fill <= 0xFF; fill += 0xFF) {
                    AlignedBytes q(b + len, fill);
                    for (uint32_t lane = 0; lane < lanes; ++lane)
                        kmm_sam::raw_copy_span(src.p, sp, q.p, b, lane, lanes);
                    ok = ok && memcmp(q.p + b, src.p + a, len) == 0;
                    for (uint32_t i = 0; i < b; ++i)
                        ok = ok && q.p[i] == (uint8_t)fill;
                }
                std::vector<uint32_t> count(b + len, 0u);
                for (uint32_t lane = 0; lane < lanes; ++lane) {
                    AlignedBytes q(b + len, 0);
                    kmm_sam::raw_copy_span(src.p, sp, q.p, b, lane, lanes);
                    for (uint32_t i = 0; i < b + len; ++i)
                        count[i] += q.p[i] != 0 ? 1u : 0u;
                }
                for (uint32_t i = 0; i < b + len; ++i)
                    ok = ok && count[i] == (i < b ? 0u : 1u);
                bad += ok ? 0u : 1u;
            }
    return bad;
}
