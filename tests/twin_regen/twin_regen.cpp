// TEST INFRASTRUCTURE — host model of one persistent k_mega grid, built from the kernel's own bookkeeping (device/dregen.h) with g++.
//
// `waves` waves of 64 lanes drain one shared sample counter exactly as the loop of k_mega does — a step of every live path, dead lanes
// served from the wave's stash, a grab off the counter, a 64-wide refill, a second serve, the end test — with the ballots replaced by
// loops over a lane array, the atomic by a plain add (the waves are interleaved at iteration granularity by a seeded scheduler) and a
// path by its length in steps.  It records what a wrong bookkeeping would break: which samples were handed out and how often, refills
// that overwrite an unread slot, samples served from slots that were never filled, and how many iterations each wave ran.
// Built only by the test suite (lajolla_public_amd/build.py build_twin_regen), never loaded by the product.
#include "../../lajolla_public_amd/csrc/device/dregen.h"
#include <cstdint>
#include <vector>

using namespace ljd;

namespace {

struct Rng {   // splitmix64: the scheduler's and the path lengths' own stream, nothing to do with the renderer's pcg32
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ULL); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL; z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL; return z ^ (z >> 31); }
};

struct Wave {
    RegenState rg;
    bool live[64]; uint32_t left[64];          // per lane: a path is under way, and the steps it still takes
    bool unread[kRegenSlots];                  // per stash slot: generated and not handed out yet
    bool ended = false;
    uint32_t iters = 0; uint64_t steps = 0;
};

}  // namespace

extern "C" {

// Returns 0, or -1 if a wave was still running after `iter_cap` iterations (the model's stand-in for a hang).
//   path_len[n]   steps of each sample's path (>= 1)
//   handed[n]     out: times each sample id was started on a lane
//   wave_iters[waves], wave_steps[waves], wave_samples_steps[waves]   out: loop iterations, path steps executed, and the summed path
//                 lengths of the samples the wave started
//   faults[4]     out: refills over an unread slot | serves from a slot that holds nothing | sample ids >= n handed out |
//                 iterations that left no lane live without ending the wave
int twin_regen_run(uint32_t n, uint32_t grab, uint32_t waves, uint64_t seed, const uint32_t *path_len, uint64_t iter_cap, uint32_t *handed,
                   uint64_t *wave_iters, uint64_t *wave_steps, uint64_t *wave_samples_steps, uint64_t *faults) {
    std::vector<Wave> W(waves);
    for (auto &w : W) { regen_init(w.rg); for (int l = 0; l < 64; l++) { w.live[l] = false; w.left[l] = 0; } for (auto &u : w.unread) u = false; }
    for (uint32_t i = 0; i < n; i++) handed[i] = 0;
    for (uint32_t i = 0; i < waves; i++) wave_iters[i] = wave_steps[i] = wave_samples_steps[i] = 0;
    for (int k = 0; k < 4; k++) faults[k] = 0;
    uint64_t counter = 0;   // the grid counter (64 bits here so that the model itself cannot wrap; the kernel's is zeroed per pass)
    Rng sched{seed};
    uint32_t running = waves;

    auto serve = [&](Wave &w, uint32_t wi, uint32_t take, uint32_t first) {
        // the first `take` lanes without a path, in lane order (the kernel's rank among the dead), take slots first, first + 1, ...
        uint32_t served = 0;
        for (int l = 0; l < 64 && served < take; l++) {
            if (w.live[l]) continue;
            const uint32_t slot = first + served, id = w.rg.st_base + slot;
            if (slot >= kRegenSlots || !w.unread[slot]) faults[1]++; else w.unread[slot] = false;
            if (id >= n) { faults[2]++; w.left[l] = 1; }
            else { handed[id]++; w.left[l] = path_len[id]; wave_samples_steps[wi] += path_len[id]; }
            w.live[l] = true; served++;
        }
    };

    while (running) {
        // the scheduler: any wave that has not ended runs its next iteration
        uint32_t pick = (uint32_t)(sched.next() % running), wi = 0;
        for (;; wi++) if (!W[wi].ended) { if (pick == 0) break; pick--; }
        Wave &w = W[wi];
        if (++w.iters > iter_cap) return -1;
        // ---- the step of every path under way
        for (int l = 0; l < 64; l++) if (w.live[l]) { w.steps++; if (--w.left[l] == 0) w.live[l] = false; }
        // ---- regeneration, in the kernel's order
        uint32_t n_dead = 0;
        for (int l = 0; l < 64; l++) n_dead += w.live[l] ? 0u : 1u;
        if (n_dead != 0u) {
            uint32_t first;
            uint32_t take = regen_take(w.rg, n_dead, first);
            serve(w, wi, take, first);
            n_dead -= take;
            if (n_dead != 0u) {
                if (regen_needs_grab(w.rg)) {
                    const uint64_t b = counter; counter += grab;
                    regen_grabbed(w.rg, b > 0xffffffffull ? 0xffffffffu : (uint32_t)b, n, grab);
                }
                const uint32_t n_gen = regen_refill(w.rg);
                if (n_gen != 0u) {   // a refill restarts the stash: whatever slot is still unread now is lost
                    for (uint32_t s = 0; s < kRegenSlots; s++) if (w.unread[s]) faults[0]++;
                    for (uint32_t s = 0; s < n_gen; s++) w.unread[s] = true;
                    take = regen_take(w.rg, n_dead, first);
                    serve(w, wi, take, first);
                }
            }
        }
        bool any = false;
        for (int l = 0; l < 64; l++) any = any || w.live[l];
        if (!any) {
            if (regen_done(w.rg)) { w.ended = true; running--; }
            else faults[3]++;
        }
    }
    for (uint32_t i = 0; i < waves; i++) { wave_iters[i] = W[i].iters; wave_steps[i] = W[i].steps; }
    // what a wave leaves behind when it ends: nothing unread
    for (auto &w : W) for (auto u : w.unread) if (u) faults[1]++;
    return 0;
}

}  // extern "C"
