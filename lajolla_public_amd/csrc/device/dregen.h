// Camera-sample bookkeeping of one k_mega wave (mega.hip): the wave's open range off the grid counter and its stash of generated samples.
//
// A wave generates camera samples 64 at a time with ALL its lanes into a per-wave stash (LDS); lanes whose path has ended pick a finished
// sample up from there.  Everything here is wave-uniform arithmetic — the ballots, the counter atomic and the LDS accesses stay in the
// kernel — so that g++ compiles the very same decisions for the host model of a persistent grid (tests/twin_regen), which checks them
// before a wrong end condition can hang a GPU.
//
//   [w_next, w_end)   samples the wave has taken off the counter and not generated yet
//   stash slot i      holds sample st_base + i; slots [st_read, st_fill) are generated and not handed to a lane yet
//
// Invariants: st_read <= st_fill <= kRegenSlots; a refill happens only when st_read == st_fill (no unread slot is overwritten) and takes
// its samples from the wave's own open range only (nothing is generated that the wave may not finish); w_next <= w_end.
#pragma once
#include "dtypes.h"

namespace ljd {

constexpr uint32_t kRegenSlots = 64;

struct RegenState { uint32_t w_next, w_end, st_base, st_fill, st_read; bool exhausted; };

LJ_HD void regen_init(RegenState &rg) { rg.w_next = rg.w_end = rg.st_base = rg.st_fill = rg.st_read = 0u; rg.exhausted = false; }

// `n_dead` lanes want a sample: the first `return value` of them (by rank) take slots first, first + 1, ... of the stash.
LJ_HD uint32_t regen_take(RegenState &rg, uint32_t n_dead, uint32_t &first) {
    const uint32_t have = rg.st_fill - rg.st_read, take = n_dead < have ? n_dead : have;
    first = rg.st_read;
    rg.st_read += take;
    return take;
}

// Lanes are still without a sample after regen_take (so the stash is empty): does the wave have to go to the grid counter first?
LJ_HD bool regen_needs_grab(const RegenState &rg) { return rg.w_next == rg.w_end && !rg.exhausted; }

// The counter returned `b` for an add of `grab`: the wave owns [b, min(b + grab, n_samples)), or the frame has run out.
LJ_HD void regen_grabbed(RegenState &rg, uint32_t b, uint32_t n_samples, uint32_t grab) {
    if (b >= n_samples) rg.exhausted = true;
    else { rg.w_next = b; rg.w_end = (n_samples - b < grab) ? n_samples : b + grab; }
}

// Refill of the EMPTY stash from the open range: lanes [0, return value) generate sample st_base + lane into slot lane.  0: the range is empty.
LJ_HD uint32_t regen_refill(RegenState &rg) {
    const uint32_t left = rg.w_end - rg.w_next, n_gen = left < kRegenSlots ? left : kRegenSlots;
    if (n_gen == 0u || rg.st_read != rg.st_fill) return 0u;
    rg.st_base = rg.w_next; rg.st_fill = n_gen; rg.st_read = 0u;
    rg.w_next += n_gen;
    return n_gen;
}

// No lane of the wave is live: may it end?  Only with the counter exhausted, nothing left in its range and nothing left in the stash.
LJ_HD bool regen_done(const RegenState &rg) { return rg.exhausted && rg.w_next == rg.w_end && rg.st_read == rg.st_fill; }

} // namespace ljd
