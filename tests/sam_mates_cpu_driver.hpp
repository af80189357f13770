// The CPU driver of mates kept together in SAM output ("record_sam_mates") for the tests
// (tests/test_sam_mates_on_the_cpu.py builds it as a shared library, tests/sam_mates_san_main.cpp as a sanitized executable): a
// SAM stream in windows with a carry of bytes and a waiting mate 1, as the library's calls see one; per window the shared source
// of kmm_sam.hpp — the write walk with its span sink (cpu_raw_spans), the spans by entry, the mate check, the pair flags, the
// destinations and every lane's share of the pair copy (cpu_raw_mates_keep) — into a keep queue of exactly the size the caller
// expects, whose tail moves from window to window.  The entries (hits, windows) are the caller's: one per selected record of the
// stream, in file order.
#pragma once

#include "sam_records_cpu_driver.hpp" // (AlignedBytes, SelectTables)

// Windows end at cuts[0 .. n_cuts) (the last one = n), each copied into a buffer of exactly its size behind the carried bytes; a
// final line without its newline gets one.  mode: "record_sam" 1 / 2.  rules .. n_names: SelectTables.  hits / windows: n_entries
// entries, one per selected record of the stream; rule4: min_hits, min_permille, invert, pair rule (0 any, 1 both).  The queue
// holds tail0 + out_n bytes, all `fill`; out gets its last out_n bytes.
// stats: [0] records, [1] excluded, [2] header lines, [3] kept bytes, [4] kept records, [5] entries used (whole pairs), [6] a mate
// waits at the end, [7] the stream-wide pair of strangers (with -8), [8] calls.
// Returns 0; -3 a malformed line; -4 more selected records than entries; -5 the kept bytes pass out_n (nothing of the window is
// copied); -7 a byte in front of tail0 was written; -8 strangers (nothing of the window is copied).
extern "C" int sam_mates_cpu(const uint8_t *data, uint64_t n, const uint64_t *cuts, int n_cuts, uint32_t excl, int mode, int orig,
                             uint32_t lanes, const uint64_t *rules, const int64_t *iv3, const uint8_t *names, const uint32_t *name_off,
                             uint32_t n_names, const uint32_t *hits, const uint32_t *windows, uint64_t n_entries, const uint32_t *rule4,
                             int fill, uint64_t tail0, uint8_t *out, uint64_t out_n, uint64_t *stats)
{
    SelectTables tb(rules, iv3, names, name_off, n_names);
    const RkPairRule rule = {{rule4[0], rule4[1], rule4[2]}, rule4[3]};
    for (int i = 0; i < 9; ++i)
        stats[i] = 0;
    AlignedBytes queue((size_t)(tail0 + out_n), fill);
    uint64_t pos = 0, tail = tail0, pairs_done = 0;
    std::vector<uint8_t> carry, waiting;
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
        std::vector<uint8_t> text(t.out_bytes); // (exactly the totals' size)
        kmm_sam::CpuRaw r;
        kmm_sam::cpu_raw_spans(win.data(), win.size(), excl, mode, text.data(), r, orig != 0, lanes, &tb.sel);
        const uint32_t carried = waiting.empty() ? 0u : 1u;
        const uint64_t n_rec = t.recs + carried, entries = t.recs > 0 ? (n_rec & ~1ull) : 0ull, entry0 = 2 * pairs_done;
        if (entry0 + entries > n_entries)
            return -4;
        const uint32_t *h = hits + entry0, *wn = windows ? windows + entry0 : nullptr;
        // the waiting line in a buffer of exactly its size
        std::vector<uint8_t> held(waiting);
        // what the window keeps, summed before anything is copied (the queue is exactly as long as the model says)
        {
            std::vector<uint32_t> span_of((size_t)t.recs + 1, kmm_sam::MATE_NONE);
            for (size_t s = 0; s < r.spans.size(); ++s)
                kmm_sam::raw_span_of_store(r.spans[s], s, t.recs, span_of.data());
            const kmm_sam::MatePiece mp{win.data(), r.tot.consumed, r.spans.data(), r.spans.size(), span_of.data(), t.recs, carried,
                                        held.data(), (uint32_t)held.size()};
            uint64_t sum = 0;
            for (const kmm_sam::RawSpan &sp : r.spans) {
                uint32_t recs;
                bool odd;
                sum += kmm_sam::raw_pair_kept_len(mp, sp, h, wn, entries, rule, recs, odd);
            }
            if (tail + sum > tail0 + out_n)
                return -5;
        }
        kmm_sam::CpuMates o;
        const uint64_t kept = kmm_sam::cpu_raw_mates_keep(win.data(), r, carried, held.data(), (uint32_t)held.size(), h, wn, entries, rule,
                                                          queue.p, tail, lanes, o);
        if (o.stranger != kmm_sam::MATE_NONE) {
            stats[7] = pairs_done + o.stranger;
            return -8;
        }
        if ((o.odd_span != kmm_sam::MATE_NONE) != (t.recs > 0 && (n_rec & 1)))
            return -9;
        tail += kept;
        pairs_done += entries / 2;
        stats[0] += t.recs;
        stats[1] += t.excluded;
        stats[2] += t.headers;
        stats[3] += kept;
        stats[4] += o.kept_recs;
        if (t.recs > 0) {
            waiting.clear();
            if (o.odd_span != kmm_sam::MATE_NONE) {
                const kmm_sam::RawSpan &sp = r.spans[o.odd_span];
                waiting.assign(win.begin() + (std::ptrdiff_t)sp.start, win.begin() + (std::ptrdiff_t)(sp.start + sp.len));
            }
        }
        carry.assign(win.begin() + (std::ptrdiff_t)t.consumed, win.end());
        pos = end;
    }
    stats[5] = 2 * pairs_done;
    stats[6] = waiting.empty() ? 0 : 1;
    for (uint64_t i = 0; i < tail0; ++i)
        if (queue.p[i] != (uint8_t)fill)
            return -7;
    if (out_n)
        memcpy(out, queue.p + tail0, (size_t)out_n);
    return 0;
}

// The mate check against brute force: two lines whose names have la and lb bytes (0 .. max_len), equal, or different at exactly
// one position d of the shorter name, each followed by a TAB and a rest — and each once more without any TAB (a stranger to
// everything).  Every line lies in a heap buffer of exactly its size.  Returns the number of verdicts that disagree with
// "the names are equal in length and content".
extern "C" uint64_t sam_mates_names_sweep(uint32_t lanes, uint32_t max_len)
{
    uint64_t bad = 0;
    const auto lowest = [&](auto f) {
        uint32_t low = kmm_sam::MATE_NONE;
        for (uint32_t lane = 0; lane < lanes; ++lane) {
            const uint32_t c = f(lane);
            low = c < low ? c : low;
        }
        return low;
    };
    const auto make = [](uint32_t len, uint32_t differ_at, bool tab, uint32_t rest) {
        std::vector<uint8_t> v;
        for (uint32_t i = 0; i < len; ++i)
            v.push_back((uint8_t)('a' + (i * 7u) % 23u + (i == differ_at ? 1u : 0u)));
        if (tab)
            v.push_back((uint8_t)'\t');
        for (uint32_t i = 0; i < rest; ++i)
            v.push_back((uint8_t)(i % 3u == 2u ? '\t' : 'z' - i % 5u)); // (what follows the name never decides)
        v.push_back((uint8_t)'\n');
        return v;
    };
    for (uint32_t la = 0; la <= max_len; ++la)
        for (uint32_t lb = 0; lb <= max_len; ++lb) {
            const uint32_t m = la < lb ? la : lb;
            for (uint32_t d = 0; d <= m; ++d) { // (d == m: no difference inside the shorter name)
                const uint32_t at = d < m ? d : 0xFFFFFFFFu;
                const std::vector<uint8_t> a = make(la, 0xFFFFFFFFu, true, la % 7u), b = make(lb, at, true, (lb + d) % 9u);
                const bool want = la != lb || d < m;
                const bool got = kmm_sam::raw_pair_strangers(kmm_sam::MateLine{a.data(), (uint32_t)a.size()},
                                                             kmm_sam::MateLine{b.data(), (uint32_t)b.size()}, lanes, lowest);
                bad += got != want ? 1u : 0u;
            }
            // no TAB in one of the lines: strangers, and no byte behind either line is read
            const std::vector<uint8_t> a = make(la, 0xFFFFFFFFu, false, 0), b = make(lb, 0xFFFFFFFFu, true, 3);
            bad += kmm_sam::raw_pair_strangers(kmm_sam::MateLine{a.data(), (uint32_t)a.size()}, kmm_sam::MateLine{b.data(), (uint32_t)b.size()},
                                               lanes, lowest) ? 0u : 1u;
            bad += kmm_sam::raw_pair_strangers(kmm_sam::MateLine{b.data(), (uint32_t)b.size()}, kmm_sam::MateLine{a.data(), (uint32_t)a.size()},
                                               lanes, lowest) ? 0u : 1u;
        }
    // a line that is missing altogether
    const std::vector<uint8_t> a = make(5, 0xFFFFFFFFu, true, 2);
    bad += kmm_sam::raw_pair_strangers(kmm_sam::MateLine{nullptr, 0u}, kmm_sam::MateLine{a.data(), (uint32_t)a.size()}, lanes, lowest) ? 0u : 1u;
    return bad;
}
