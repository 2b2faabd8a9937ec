// leaf_wg_queue.hpp -- what the seven workgroup-per-block kernels share: the task queue in LDS, its protocol and the spectrum-row load.
// Included by every unit (through leaf_fft_wg.hpp): templates, device functions, constexpr sizes (gfx950 only).
//
// The kernels (forward: leaf_fft_wg, _wg4k, _wgg, _wgg4k; backward: leaf_fft_wg_bwd, _wgg_bwd, _wgg4k_bwd) give a workgroup a list of
// blocks ("sets"), keep the spectra of two of them in a ring in LDS and hand (block, filter) tasks to their waves through one queue,
// without barriers.  Everything the waves tell each other goes through the kWgQueueInts ints described here.
#pragma once
#include "leaf_fft.hpp"

namespace {

// ---- the queue's ints ---------------------------------------------------------------------------------------------------------
// `slot` = set & 1 is the ring slot of a block, `gen` = set >> 1 counts the slot's occupants.  Every counter only grows.
//   field            ints    meaning                                                            written / waited for by
//   kWgQNext         0       task cursor                                                        wg_pull: all seven
//   kWgQSpectrum     1..2    spectra published in the slot, ever                                wg_publish / wg_acquire_block: all seven
//   kWgQReaders      3..4    filter tasks that are done with the slot's spectrum, ever          wg_reader_done (band tasks included): all seven;
//                                                                                               the forward transforms of the FORWARD kernels wait for it
//   kWgQCoords       5..8    {clip, block in the clip} of the slot's occupant                   wg_publish / wg_acquire_block: all seven
//   kWgQReleased     9..10   generations of the slot that every reader has left                 the three BACKWARD kernels, at their task ends (their
//                                                                                               forward transforms wait for it instead of kWgQReaders)
//   kWgQStreamOut    11..12  blocks finalized per slot parity                                   the STREAM instances of leaf_fft_wg_kernel only
//   kWgQDxTicket     11..12  filters added to the slot's dL/dx sum G, ever (filter order)       leaf_fft_wg_bwd / leaf_fft_wgg_bwd with DX, and their
//                                                                                               band tasks (leaf_band_bwd.hpp)
//   kWgQTapTicket    13..14  filters added to the slot's unpaired-tap sums, ever                leaf_fft_wgg_bwd with DX, even windows
// kWgQStreamOut and kWgQDxTicket SHARE ints 11..12.  That is safe because no kernel uses both: the first belongs to a forward kernel,
// the second to backward kernels, and a launch's queue belongs to one kernel.  (leaf_fft_wgg4k_bwd keeps its dL/dx tickets behind its
// sums, not here.)  Int 15 is unused.
constexpr int kWgQueueInts = 16;
enum WgQueueField : int {
    kWgQNext = 0,
    kWgQSpectrum = 1,
    kWgQReaders = 3,
    kWgQCoords = 5,
    kWgQReleased = 9,
    kWgQStreamOut = 11,
    kWgQDxTicket = 11,
    kWgQTapTicket = 13,
    kWgQEnd = 15
};
static_assert(kWgQEnd <= kWgQueueInts, "the queue's fields fit its LDS");
// (&q[field + slot], the form the kernels had written out: the compiler folds the field into the LDS instruction's offset)
__device__ __forceinline__ int* wgq_next(int* q) { return &q[kWgQNext]; }
__device__ __forceinline__ int* wgq_spectrum_cnt(int* q, int slot) { return &q[kWgQSpectrum + slot]; }
__device__ __forceinline__ int* wgq_readers_cnt(int* q, int slot) { return &q[kWgQReaders + slot]; }
__device__ __forceinline__ int* wgq_clip(int* q, int slot) { return &q[kWgQCoords + 2 * slot]; }
__device__ __forceinline__ int* wgq_block_in_clip(int* q, int slot) { return &q[kWgQCoords + 1 + 2 * slot]; }
__device__ __forceinline__ int* wgq_released_cnt(int* q, int slot) { return &q[kWgQReleased + slot]; }
__device__ __forceinline__ int* wgq_stream_out_cnt(int* q, int parity) { return &q[kWgQStreamOut + parity]; }
__device__ __forceinline__ int* wgq_dx_ticket(int* q, int slot) { return &q[kWgQDxTicket + slot]; }
__device__ __forceinline__ int* wgq_tap_ticket(int* q, int slot) { return &q[kWgQTapTicket + slot]; }

// ---- the protocol ---------------------------------------------------------------------------------------------------------------
// Data (ring slots, block coordinates, shared sums) is written with plain LDS stores, then a counter moves (relaxed atomic add by lane
// 0) and the readers spin on it (relaxed atomic loads).  The ordering is carried by FENCES restricted to the LDS address space: release
// before the counter moves, acquire after the spin.  On gfx950 the release fence is the s_waitcnt lgkmcnt(0) these sites issued by hand
// in round 2 and the acquire fence emits no instruction (a wave's LDS operations execute in order) -- the generated code is unchanged --
// but the compiler now KNOWS it may not move LDS accesses across them; the unrestricted fences would also wait for the global loads in
// flight (table prefetches), which the protocol does not need.
__device__ __forceinline__ int wg_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void wg_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local"); }
__device__ __forceinline__ void wg_wait_ge(const int* p, int need) {
    while (wg_ld(p) < need) __builtin_amdgcn_s_sleep(1);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// lane 0 adds one to a counter
__device__ __forceinline__ void wg_bump(int* cnt, int lane) {
    if (lane == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// ... and every lane gets the old value (wave-uniform)
__device__ __forceinline__ int wg_count(int* cnt, int lane) {
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __builtin_amdgcn_readfirstlane(old);
}
// the next task id (lane0: the wave's lane index as the compiler knows it, not an opaque copy)
__device__ __forceinline__ int wg_pull(int* q, int lane0) { return wg_count(wgq_next(q), lane0); }
// The hand-over of a spectrum that the caller has stored in ring slot `slot`: the block's coordinates for its readers, the release
// fence, the counter.
__device__ __forceinline__ void wg_publish(int* q, int slot, int b, int c, int lane) {
    if (lane == 0) { *wgq_clip(q, slot) = b; *wgq_block_in_clip(q, slot) = c; }
    wg_release();
    wg_bump(wgq_spectrum_cnt(q, slot), lane);
}
// A wave's first filter of a block: once the spectrum of generation `gen` is in the slot it stays until every filter is done.
__device__ __forceinline__ void wg_acquire_block(int* q, int slot, int gen, int& b, int& c) {
    wg_wait_ge(wgq_spectrum_cnt(q, slot), gen + 1);
    b = __builtin_amdgcn_readfirstlane(wg_ld(wgq_clip(q, slot)));
    c = __builtin_amdgcn_readfirstlane(wg_ld(wgq_block_in_clip(q, slot)));
}
// This task has read the slot's spectrum for the last time: release fence + count (forward kernels, band tasks).
__device__ __forceinline__ void wg_reader_done(int* q, int slot, int lane) {
    wg_release();
    wg_bump(wgq_readers_cnt(q, slot), lane);
}
// (The backward kernels count their readers the same way but need the old value: the reader that finds gen NT + NT - 1 before it is the
// block's last one and bumps kWgQReleased, which their forward transforms wait for.  That sequence is written out at their task ends:
// as a function of this header it changed the register allocation of leaf_fft_wg_bwd_kernel, which then measured 0.2 % slower with dL/dx.)

// Task ids over a DENSE grid of F + 1 slots per set: task 0 = fwd(0); task 1 + i (F + 1) + r = slot r of set i, slot 0 being
// fwd(i + 1) and slots 1..F the set's filters.  u / (F + 1) by multiply-high with M = ceil(2^32 / (F + 1)) -- exact while
// u (M (F + 1) - 2^32) < 2^32, i.e. u < 2^32 / (F + 1); a plain division beyond that (`exact` = false).  (A power-of-two grid
// decoded by shifts left 23 of 64 slots empty at F = 40 -- 63 of 128 at F = 64 -- each costing a queue pull and a wasted
// spectrum-row prefetch: tools/trace_wg.py.)
struct WgTaskGrid {
    unsigned n, magic;
    bool exact;
};
__device__ __forceinline__ WgTaskGrid wg_task_grid(int F, int nset) {
    WgTaskGrid g;
    g.n = (unsigned)F + 1u;
    g.magic = (unsigned)((0x100000000ull + g.n - 1u) / g.n);
    g.exact = (unsigned long long)(nset > 0 ? nset : 1) * g.n * g.n < 0x80000000ull;
    return g;
}
__device__ __forceinline__ void wg_task_decode(const WgTaskGrid& g, int t, int& set, int& role) {
    if (t == 0) { set = 0; role = 0; return; }
    const unsigned u = (unsigned)(t - 1);
    const unsigned qv = g.exact ? __umulhi(u, g.magic) : u / g.n;
    set = (int)qv;
    role = (int)(u - qv * g.n);
    if (role == 0) set += 1;                                              // the NEXT set's spectrum, ahead of this set's filters
}
// A wave's view of the queue: `nset` sets of NT filter tasks each.  next(): pull a task and, when there is one (has(t)), decode it into
// (set, role) -- role 0 = forward transform of set `set`, role 1..NT = filter task role - 1 of set `set`; past the last task `set` is
// left as it was and role = 0 (no filter: the callers that prefetch the next task's table row take row 0).  Returns the task id.
struct WgTaskCursor {
    int* q;
    int lane0;
    WgTaskGrid grid;
    int ntasks;
    __device__ __forceinline__ bool has(int t) const { return t < ntasks; }
    __device__ __forceinline__ int next(int& set, int& role) const {
        const int t = wg_pull(q, lane0);
        if (t < ntasks) wg_task_decode(grid, t, set, role);
        else role = 0;
        return t;
    }
};
__device__ __forceinline__ WgTaskCursor wg_task_cursor(int* q, int lane0, int NT, int nset) {
    return WgTaskCursor{q, lane0, wg_task_grid(NT, nset), nset > 0 ? 1 + nset * (NT + 1) : 0};
}

// ---- a filter's spectrum row: rq[k] = R[row][64 k + lane] of the [..][2048] float table H, the 32 loads issued together ----------------
__device__ __forceinline__ void wg_load_real_spectrum(float (&rq)[32], const void* H, int row, int lane) {
    const float* src = static_cast<const float*>(H) + (size_t)row * kFftN + lane;
    asm volatile("" ::: "memory");
#pragma unroll
    for (int k = 0; k < 32; ++k) rq[k] = src[64 * k];
    asm volatile("" ::: "memory");
}

}  // namespace
