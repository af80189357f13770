// kmm_line_search.hpp — part of libkmm (MI355X / gfx950); included by kmm_records.hpp.
// Where the target-th item (1-based) of a sequence lies, searched through exclusive prefix sums of item counts: the test every
// thread of k_rec_cut makes for its own slot, on each of the three levels (super-tiles, the tiles of one, the bytes of one).
// Plain C++: the CPU tier compiles this header with g++.
#pragma once

#if defined(__HIPCC__)
#define KMM_LS_HD __host__ __device__ __forceinline__
#else
#include <cstdint>
#define KMM_LS_HD inline
#endif

// Slot with `pre` items in front of it and `next` items in front of its successor (the total behind the last slot): does it
// hold item `target`?  Exactly one slot does for 1 <= target <= total, none for target 0 or beyond the total; a slot without
// items (pre == next) never does.
KMM_LS_HD bool ls_slot_holds(uint32_t pre, uint32_t next, uint32_t target)
{
    return pre < target && target <= next;
}

// The rank of `target` inside the slot that holds it (1-based).
KMM_LS_HD uint32_t ls_rank_in_slot(uint32_t pre, uint32_t target)
{
    return target - pre;
}
