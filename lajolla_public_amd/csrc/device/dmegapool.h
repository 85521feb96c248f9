// Pass arithmetic of the candidate pool of a tiny scene's leaf scan (mega.hip: scan_trace).
//
// After the box scan every lane holds two masks: ms (leaf boxes its shadow ray's segment overlaps) and me (those of its extension ray).
// The (ray, leaf) candidates of the whole wave are listed in a per-wave LDS pool of `cap` 16-bit items and then tested 64 at a time by
// whichever lane is free.  The list is written LANE-MAJOR: one wave prefix sum over the lanes' candidate counts gives every lane the
// index of its first item, and each lane writes its own items there.  When the wave has more candidates than the pool holds, the
// pass lists the first `cap` of them in lane order — a lane's candidates may be split between two passes — and the rest waits.
//
// Everything here is plain integer arithmetic that g++ compiles as well as hipcc: the prefix sum (DPP), the LDS accesses and the
// wavefront barriers stay in mega.hip, so that the host model (tests/twin_pool) runs the very decisions of a pass — with the prefix sum
// as a plain loop — and checks that every candidate is listed exactly once, that no index reaches items[cap] and that the pass loop
// ends, before a mistake in them can hang a GPU.
//
//   c      candidates a lane has left: c_s + c_e = popc(ms) + popc(me)
//   excl   candidates left in lower lanes (exclusive prefix sum of c); total: those of the whole wave
//   a pass lists items [0, min(total, cap)); the lane writes its share (pool_share) of them at excl, excl + 1, ...
//   the pass loop ends when total == 0; a pass with total > 0 lists at least one item for any cap >= 1 (the lowest lane with c > 0 has
//   excl == 0 < cap), so total falls by min(total, cap) >= 1 per pass: ceil(total / cap) passes.
#pragma once
#include "dtypes.h"

namespace ljd {

// A lane's candidates are numbered by their bit in the 64-bit word ms | me << 32: bit b < 32 is bit b of ms, bit 32 + b is bit b of me.  They are
// taken lowest bit first, so the shadow ray's candidates come first.  The kernel never forms the word: it keeps the two masks apart (32-bit
// registers and instructions) and lists a lane's share in two loops, first from ms, then from me.
constexpr uint32_t kPoolExtBit = 32u;

// Item: lane | bit << 6 (12 bits).  bit >> 5 = 1: the lane's extension ray, 0: its shadow ray; bit b of a mask stands for leaf n_used - 1 - b
// (the scan shifts the boxes' bits in from below).  The subtraction is done where an item is read, once per 64 items, not where it is written.
LJ_HD uint32_t pool_item(uint32_t lane, uint32_t bit) { return lane | (bit << 6); }
LJ_HD uint32_t pool_item_lane(uint32_t it) { return it & 63u; }
LJ_HD uint32_t pool_item_ext(uint32_t it) { return it >> 11; }
LJ_HD uint32_t pool_item_leaf(uint32_t it, uint32_t n_used) { return n_used - 1u - ((it >> 6) & 31u); }

// Items the lane lists in this pass — n_s from ms, then n_e from me: what the pool still holds above the lower lanes' items (excl of them), and
// no more than the lane has (c_s + c_e).  excl + n_s + n_e <= cap.
LJ_HD void pool_share(uint32_t c_s, uint32_t c_e, uint32_t excl, uint32_t cap, uint32_t &n_s, uint32_t &n_e) {
    const uint32_t room = cap - (excl < cap ? excl : cap);
    n_s = c_s < room ? c_s : room;
    n_e = c_e < room - n_s ? c_e : room - n_s;
}
// Items of the pass, over all lanes
LJ_HD uint32_t pool_pass_items(uint32_t total, uint32_t cap) { return total < cap ? total : cap; }

// Was that the last pass?  It listed min(total, cap) of the wave's `total` candidates: none is left exactly when total <= cap, and the next
// prefix sum would come to 0 — the end condition, without computing that sum.
LJ_HD bool pool_last_pass(uint32_t total, uint32_t cap) { return total <= cap; }

// The next candidate of a mask (m != 0): its bit, cleared from the mask
LJ_HD uint32_t pool_pop(uint32_t &m) {
    const uint32_t bit = (uint32_t)__builtin_ctz(m);
    m &= m - 1u;
    return bit;
}

// ---- the short last test round of a pass, split by primitive
//
// The test loop walks the pass's items 64 at a time, every lane the `count` primitives of its item's leaf one after the other.  The last round
// holds m = n_items - r items; when that is few enough, several lanes share an item.  With M the largest `count` of the leaf table rounded up
// to a power of two (a scene constant, wave-uniform), a round of m * M <= 64 items runs ONE primitive per lane: lane l takes primitive l % M
// of item r + l / M, and is idle when that item does not exist or its leaf has no such primitive.  M = 1 never splits: there is nothing to
// share out.  A table whose largest leaf is an exception (cbox: seventeen leaves of two triangles and one of four, so M = 4) would split
// only below 64 / M items; so a round too long for M lanes per item takes the widest power of two W < M with m * W <= 64 instead: lane l
// then walks primitives l % W, l % W + W, ... of item r + l / W.  W = M is the case above, W = 1 the unsplit round.  The order of the tests
// cannot change a result (closest hit: a minimum over a total order; occlusion: an OR).

// M of a leaf table whose largest leaf holds max_count primitives (1 for an empty table)
LJ_HD uint32_t pool_split_width(uint32_t max_count) {
    uint32_t m = 1u;
    while (m < max_count) m <<= 1;
    return m;
}
// Does a round of m >= 1 items run one primitive per lane (M lanes per item)?  Wave-uniform, as everything about a round's shape.
LJ_HD bool pool_round_splits(uint32_t m, uint32_t M) { return M > 1u && m * M <= 64u; }
// log2 of W, the lanes per item of a round of m >= 1 items: the widest power of two W <= M with m * W <= 64 (0: one lane per item — every
// round of more than 32 items, so every round but a pass's last).  pool_round_splits(m, M) exactly when this comes to log2 M > 0.
LJ_HD uint32_t pool_round_shift(uint32_t m, uint32_t M) {
    uint32_t shift = 0u;
    while ((2u << shift) <= M && m * (2u << shift) <= 64u) shift++;
    return shift;
}
// The lane's item of the round that starts at item r (to be held against n_items by the caller) ...
LJ_HD uint32_t pool_round_item(uint32_t r, uint32_t lane, uint32_t shift) { return r + (lane >> shift); }
// ... and the first primitive of that item's leaf it tests; the next ones follow in steps of W = 1 << shift, below the leaf's `count`
LJ_HD uint32_t pool_round_prim(uint32_t lane, uint32_t shift) { return lane & ((1u << shift) - 1u); }

} // namespace ljd
