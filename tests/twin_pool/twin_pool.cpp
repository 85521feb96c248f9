// TEST INFRASTRUCTURE — host model of the candidate pool of one k_mega wave, built from the kernel's own pass arithmetic
// (device/dmegapool.h) with g++.
//
// A wave of 64 lanes with given candidate masks (ms: shadow ray, me: extension ray) runs the pass loop of scan_trace (mega.hip) until
// it ends: the prefix sum over the lanes' counts as a plain loop, every lane's write loop, the end test.  The items of every pass are
// handed back decoded, with what a wrong pass logic would break: indices outside the pass, slots written twice or not at all, a pass
// loop that does not end.  Built only by the test suite (lajolla_public_amd/build.py build_twin_pool), never loaded by the product.
#include "../../lajolla_public_amd/csrc/device/dmegapool.h"
#include <cstdint>
#include <vector>

using namespace ljd;

extern "C" {

// Returns the number of passes run, or -1 if the loop was still running after `pass_limit` passes (the model's stand-in for a hang).
//   ms[64], me[64]   the lanes' masks; n_used: leaves in the table (bit b of a mask is leaf n_used - 1 - b)
//   listed           out: per item over all passes, in pass and index order: lane | kind << 8 | leaf << 16 | pass << 32 (kind 1: shadow ray);
//                    at most `listed_cap` are stored, *n_listed counts all of them
//   pass_items       out: n_items of each pass (at most `pass_limit` stored)
//   faults[4]        out: writes at an index >= n_items or >= cap | slots of [0, n_items) written more than once | slots of [0, n_items)
//                    never written | passes after which pool_last_pass disagreed with "no candidate is left"
int twin_pool_run(const uint32_t *ms, const uint32_t *me, uint32_t n_used, uint32_t cap, uint32_t pass_limit, uint64_t *listed, uint64_t listed_cap,
                  uint64_t *n_listed, uint32_t *pass_items, uint64_t *faults) {
    uint32_t ws[64], we[64];   // the lanes' masks as the pass loop consumes them
    for (int l = 0; l < 64; l++) { ws[l] = ms[l]; we[l] = me[l]; }
    for (int k = 0; k < 4; k++) faults[k] = 0;
    *n_listed = 0;
    std::vector<uint32_t> items(cap), written(cap);
    uint32_t passes = 0;
    for (;;) {
        // the prefix sum (mega.hip: wave_prefix_incl and the readlane of lane 63)
        uint32_t cs[64], c[64], incl[64], run = 0;
        for (int l = 0; l < 64; l++) { cs[l] = (uint32_t)__builtin_popcount(ws[l]); c[l] = cs[l] + (uint32_t)__builtin_popcount(we[l]); run += c[l]; incl[l] = run; }
        const uint32_t total = incl[63];
        if (total == 0u) break;
        if (passes == pass_limit) return -1;
        const uint32_t n_items = pool_pass_items(total, cap);
        for (uint32_t i = 0; i < cap; i++) written[i] = 0;
        // the write loop of every lane
        for (uint32_t l = 0; l < 64; l++) {
            auto store = [&](uint32_t idx, uint32_t it) {   // (a 16-bit store)
                if (idx >= n_items || idx >= cap) faults[0]++; else { items[idx] = it & 0xffffu; written[idx]++; }
            };
            uint32_t n_s, n_e, idx = incl[l] - c[l];
            pool_share(cs[l], c[l] - cs[l], idx, cap, n_s, n_e);
            for (const uint32_t end = idx + n_s; idx != end; idx++) store(idx, pool_item(l, pool_pop(ws[l])));
            for (const uint32_t end = idx + n_e; idx != end; idx++) store(idx, pool_item(l, kPoolExtBit + pool_pop(we[l])));
        }
        // the read side: what the test loop decodes from slots [0, n_items)
        for (uint32_t i = 0; i < n_items; i++) {
            if (written[i] > 1) faults[1]++;
            if (written[i] == 0) { faults[2]++; continue; }
            const uint32_t it = items[i], kind = 1u - pool_item_ext(it);
            if (*n_listed < listed_cap) listed[*n_listed] = pool_item_lane(it) | (kind << 8) | (pool_item_leaf(it, n_used) << 16) | ((uint64_t)passes << 32);
            (*n_listed)++;
        }
        if (passes < pass_limit) pass_items[passes] = n_items;
        passes++;
        bool left = false;
        for (int l = 0; l < 64; l++) left = left || (ws[l] | we[l]) != 0u;
        const bool last = pool_last_pass(total, cap);
        if (last == left) faults[3]++;
        if (last) break;
    }
    return (int)passes;
}

}  // extern "C"
