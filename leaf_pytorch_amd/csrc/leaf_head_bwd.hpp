// leaf_head_bwd.hpp -- the head-only backward: the gradients of pool_b and of the four PCEN vectors from pooled_raw and grad_out,
// one launch.  What a Leaf with a frozen filterbank (Gabor kernel and pooling width) needs: no waveform, no tables, no transforms.
// Included by inst_head_bwd.hip only: the kernel and the split of its grid (gfx950 only).
//
// Grid (F, S), four waves per workgroup.  Workgroup (f, s) walks the rows b in [s L, min(B, (s + 1) L)) of filter f, one wave per
// row (pcen_bwd_scan_row, leaf_pcen_scan.hpp, without its per-frame stores: neither g_pre nor the rows' sums reach memory), and
// adds the rows' five numbers in a fixed order: each wave its rows b = s L + wave, + 4, ... ascending, then the four waves in wave
// order.  The sum over the batch happens in the same launch, without floating-point atomics: the workgroup writes its five sums as
// one RECORD into the workspace and takes a ticket for its filter (an integer fetch_add); the workgroup that draws the last ticket
// adds the S records in the order s = 0 .. S - 1 and writes the outputs.  Nobody waits for anybody, and the result does not depend
// on who finishes last: bit-identical from run to run.
// The hand-over is an agent-scope release in every workgroup and one agent-scope acquire in the reducer:
//     record stores -> s_waitcnt vmcnt(0) -> barrier -> one lane: release fence, s_waitcnt vmcnt(0), ticket add
//     reducer: one lane's acquire fence -> s_waitcnt vmcnt(0) -> barrier -> vector loads of the records (staged through LDS)
// The records are reached through a plain pointer (no const __restrict__) at lane-dependent addresses: vector loads behind the
// acquire, never the scalar cache.  The host zeroes the tickets with a memset node in front of every launch; nothing else is
// assumed about the workspace.
#pragma once
#include "leaf_pcen_scan.hpp"

namespace {

constexpr int kHeadThreads = 64 * kHeadWaves;          // (kHeadWaves, kHeadRecFloats: leaf_params.hpp -- they size the workspace)
constexpr int kHeadSliceRows = 8;        // the shortest slice of the batch a workgroup takes: two rows per wave
constexpr int kHeadWgPerCu = 4;          // workgroups per CU the split aims at
constexpr int kHeadStage = 128;          // records the reducer brings into LDS at a time

// S slices of L rows (L a multiple of the waves; the last slice holds the rest, at least one row): from B, F and the CU count alone
struct HeadPlan {
    int S, L;
};
inline HeadPlan head_plan(int B, int F, int cus) {
    const int cap = std::max(1, kHeadWgPerCu * cus / std::max(F, 1));
    const int s0 = std::max(1, std::min((B + kHeadSliceRows - 1) / kHeadSliceRows, cap));
    const int L = ((B + s0 - 1) / s0 + kHeadWaves - 1) / kHeadWaves * kHeadWaves;
    return HeadPlan{L > 0 ? (B + L - 1) / L : 0, L};
}

__global__ __launch_bounds__(kHeadThreads) void leaf_head_bwd_kernel(const HeadBwdParams p) {
    // the one LDS array: the waves' sums in rows 0 .. 3, word [0][7] the ticket this workgroup drew; in the reducer the records
    __shared__ float sm[kHeadStage][kHeadRecFloats];
    const int f = blockIdx.x, s = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int TP = p.TP, S = p.S;
    const int b_hi = min(p.B, (s + 1) * p.L);
    float* M = p.ema ? p.ema + ((size_t)(f * S + s) * kHeadWaves + wave) * TP : nullptr;
    float a_a = 0.f, a_d = 0.f, a_rho = 0.f, a_w = 0.f, a_g = 0.f;
    for (int b = s * p.L + wave; b < b_hi; b += kHeadWaves) {
        const size_t r0 = ((size_t)b * p.F + f) * TP;
        const ScanRowSums q = pcen_bwd_scan_row<false>(p.raw + r0, p.gout, r0, TP, f, p.alpha, p.delta, p.root, p.ema_w, p.floor_,
                                                       p.mode, M, nullptr, nullptr, 0, lane);
        a_a += q.a;
        a_d += q.d;
        a_rho += q.rho;
        a_w += q.w;
        a_g += q.g;
        // the wave's next row overwrites M: its loads of this row have returned before that
        if (M) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (lane < 5) sm[wave][lane] = lane == 0 ? a_a : lane == 1 ? a_d : lane == 2 ? a_rho : lane == 3 ? a_w : a_g;
    __syncthreads();
    float* recs = p.rec + (size_t)f * S * kHeadRecFloats;
    if (wave == 0 && lane < 5) {
        float t = sm[0][lane];
#pragma unroll
        for (int w = 1; w < kHeadWaves; ++w) t += sm[w][lane];
        recs[(size_t)s * kHeadRecFloats + lane] = t;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // (the fence's own wait can be dropped: keep this one, in this order)
        const unsigned ticket = __hip_atomic_fetch_add(p.tickets + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sm[0][7] = __uint_as_float(ticket);
    }
    __syncthreads();
    if (__float_as_uint(sm[0][7]) != (unsigned)(S - 1)) return;          // (the whole workgroup: the word is one value)
    // the last ticket of filter f: every record of f has been released
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // kHeadStage records at a time through LDS (every thread loads, coalesced: one memory latency per stage), added by five lanes in
    // the order s = 0 .. S - 1; the records' three padding words travel along unread
    float t = 0.0f;
    for (int i0 = 0; i0 < S; i0 += kHeadStage) {
        const int n = min(kHeadStage, S - i0);
        for (int e = threadIdx.x; e < n * kHeadRecFloats; e += kHeadThreads) (&sm[0][0])[e] = recs[(size_t)i0 * kHeadRecFloats + e];
        __syncthreads();
        if (wave == 0 && lane < 5)
            for (int i = 0; i < n; ++i) t += sm[i][lane];
        if (i0 + kHeadStage < S) __syncthreads();
    }
    if (wave == 0 && lane < 5) {
        if (lane == 4) p.g_pool_b[f] = t;
        else if (p.mode & 1) (lane == 0 ? p.g_alpha : lane == 1 ? p.g_delta : lane == 2 ? p.g_root : p.g_ema_w)[f] = t;
    }
}

}  // namespace
