// leaf_fft_wg4k.hpp -- overlap-save forward with 4096-sample blocks for the long 32 kHz window (K = 801, hop = 320)
// Included by every unit: templates, device functions, constexpr sizes (gfx950 only).
//
// Why: with 2048-sample blocks a K = 801 window leaves L = 960 valid outputs per transform (47 %); a 4096-sample block
// leaves 3200 (78 %).  A wave cannot hold a 4096-point transform (128 data registers), but it does not have to: one
// radix-2 decimation-in-frequency step splits the inverse transform into two INDEPENDENT 2048-point transforms -- the even
// output samples from zs[e] = Z[e] + Z[e + 2048], the odd ones from zd[e] = (Z[e] - Z[e + 2048]) w^e -- which the wave runs
// one after the other with the wave-level transform it already has (fft2048w).  The w^e twiddle is folded into a second
// pair of per-filter spectrum tables, so the step costs a few multiplies per bin, no extra pass:
//     zs[e] = conj(A'[e]) R[e] + A'[2048 - e] R[e + 2048]                  (A' real-input: conj(A'[e + 2048]) = A'[2048 - e])
//     zd[e] = conj(A'[e]) D_lo[e] - A'[2048 - e] D_hi[e],   D_lo = R[e] w^e,  D_hi = R[e + 2048] w^e,  w = e^{-2 pi i / 4096}
// Each half looks exactly like a 16 kHz block: 1600 valid samples at stride 2, pooled with the even / odd taps of the
// Gaussian window (401 / 400 taps, hop 160) -- the static pooling code of the 401/160 geometry, fed from de-interleaved
// pooling rows -- and both halves add into the same 13 frame accumulators.
// Round 4 (static 32 kHz kernel): (i) the odd half is computed as (conj(A'[e]) R[e] - A'[2048 - e] R[e + 2048]) w^e from the
// SAME real tables as the even half and ONE filter-independent twiddle table w^e (16 KB) -- the same eight instructions per
// bin as with the folded tables, but a task now touches 16 KB of per-filter tables instead of 48 KB: 80 filters are 1.3 MB
// instead of 3.9 MB next to a 4 MB L2 per XCD (396 MB through the fabric per launch against 102 MB algorithmic, round 3;
// the D tables are still built: the run-time-geometry and backward kernels read them); (ii) the pooling weights of a half
// live in 15 registers (the (row, frame) pairs of the 401/160 half-rate geometry share 15 distinct weight vectors,
// wg_pool_nj) instead of two wave-private LDS rows and a DMA per task: -160 ds_read_b32 per task, -8.4 KB of LDS per wave,
// which (iii) pays for the FULL transposition scratch: half the LDS store instructions of the column-half form.
// Everything else (workgroup per block, spectrum ring in LDS, task queue) is leaf_fft_wg.hpp; the forward task builds
// A' = FFT4096(block) from two 2048-point transforms of the even / odd input samples (decimation in time, combined
// through the ring slot itself).
#pragma once
#include "leaf_fft_wg.hpp"

namespace {

constexpr int kFft4N = 4096;
#ifndef LEAF_4K_FWD_NW
#define LEAF_4K_FWD_NW 12              // waves of the static 4096-sample forward kernel (A/B: 11)
#endif
constexpr int kWg4RingFloat2 = 2056;           // bins 0..2048 of a 4096-point spectrum, padded
constexpr int kWg4RowFloats = 528;             // one half pooling row: 64 zeros + 401 taps + 63 zeros (as the 401/160 geometry)
// static forward kernel (round 4): full transposition scratch per wave, no pooling rows (the weights live in registers)
constexpr size_t fft_wg4k_lds_bytes(int NW) {
    return ((size_t)kTwFloats + 2 * (32 + 64) + 2 * 2 * kWg4RingFloat2 + kWgQueueInts + (size_t)NW * kWgScrFloats) * 4;
}
// S801: the pooling backward reads the half's parity row as 13 register vectors per lane (the forward's form) instead of
// wave-private LDS rows filled by DMA: whole backward at cfg2 5.53 -> 5.41 ms, with dL/dx 7.01 -> 6.78 ms, same box
// (profiles/r04/ab_bwd_regw.txt) -- which frees the rows' LDS: the parameter-gradient kernel
// (leaf_fft_wgg4k_bwd_kernel<12, 7, true>) runs with the forward's full transposition scratch, fft_wg4k_lds_bytes (fewer LDS
// store instructions per transform: 5.58 -> 5.49 ms, same box).
// With dL/dx (leaf_fft_wgg4k_bwd_kernel<8, 7, true, true>): half-size scratch + three folded gradient spectra and their
// tickets.  Eight waves: two per SIMD with 256 VGPRs each -- the filter's R_lo / R_hi stay in
// registers for the task (nine waves at 168 VGPRs measured 11 % slower: profiles/r04/ab_4k_dx.txt)
#ifndef LEAF_4K_BWD_NW
#define LEAF_4K_BWD_NW 12            // waves of the static 4096-sample backward without dL/dx (A/B: 8 = two per SIMD, 256 VGPRs)
#endif
#ifndef LEAF_4K_DX_NW
#define LEAF_4K_DX_NW 8
#endif
constexpr int kWg4BwdDxWaves = LEAF_4K_DX_NW;
constexpr size_t fft_wg4k_bwd_dx_lds_bytes(int NW) {
    return ((size_t)kTwFloats + 2 * (32 + 64) + 2 * 2 * kWg4RingFloat2 + kWgQueueInts +
            (size_t)NW * kWgScrHalfFloats) * 4 + (size_t)3 * kWg4RingFloat2 * 8 + 64;
}
// the filter-independent twiddle table of the odd half, w^e = e^{-2 pi i e / 4096}, e < 2048 (float2), behind the pooling rows
// (fft4k_prep_kernel still writes it and it travels in FftParams::lone, but no kernel reads it: the forward takes w^(64 k) w^lane
// from its LDS tables, which measured 1.4 % faster at cfg2.  Dropping it changes the table launch and the workspace layout.)
constexpr size_t kFft4WtFloats = 2 * 2048;
// per-filter tables of the 4096-point plan (floats): (R_lo, R_hi)[2048] f2 | (D_lo, D_hi)[2048] f4   (derivative slabs: the second part
// holds (d/dmu lo, d/dmu hi, d/dsigma lo, d/dsigma hi)[2048] in the mu slab; fft4k_prep_kernel)
constexpr size_t kFft4TabFloats = 2048 * 6;

// Rows k = 0..31 of the two ring streams a 4096-point multiply needs, eight rows at a time:
//   a[j] = A'[64 k + lane],  m[j] = A'[2048 - 64 k - lane],  k = 8 C + j.
template <int C>
__device__ __forceinline__ void wg4k_ring_chunk(v2f (&a)[8], v2f (&m)[8], unsigned a_dir, unsigned a_mir) {
    lds_rd8<512 * (8 * C + 0)>(a[0], a_dir); lds_rd8<512 * (8 * C + 1)>(a[1], a_dir); lds_rd8<512 * (8 * C + 2)>(a[2], a_dir);
    lds_rd8<512 * (8 * C + 3)>(a[3], a_dir); lds_rd8<512 * (8 * C + 4)>(a[4], a_dir); lds_rd8<512 * (8 * C + 5)>(a[5], a_dir);
    lds_rd8<512 * (8 * C + 6)>(a[6], a_dir); lds_rd8<512 * (8 * C + 7)>(a[7], a_dir);
    // mirror: byte address base + 512 (31 - k), base = &A'[2048 - 64 * 31 - lane]
    lds_rd8<512 * (31 - (8 * C + 0))>(m[0], a_mir); lds_rd8<512 * (31 - (8 * C + 1))>(m[1], a_mir);
    lds_rd8<512 * (31 - (8 * C + 2))>(m[2], a_mir); lds_rd8<512 * (31 - (8 * C + 3))>(m[3], a_mir);
    lds_rd8<512 * (31 - (8 * C + 4))>(m[4], a_mir); lds_rd8<512 * (31 - (8 * C + 5))>(m[5], a_mir);
    lds_rd8<512 * (31 - (8 * C + 6))>(m[6], a_mir); lds_rd8<512 * (31 - (8 * C + 7))>(m[7], a_mir);
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),
                   "+v"(m[0]), "+v"(m[1]), "+v"(m[2]), "+v"(m[3]), "+v"(m[4]), "+v"(m[5]), "+v"(m[6]), "+v"(m[7]));
}

// A table load as  uniform base (SGPR pair) + this lane's byte offset (one VGPR, zero-extended) + a compile-time byte offset:
// the form global_load takes without any address arithmetic in the VALU.  `voff` is what call sites make opaque to pin a group
// of loads in place (an opaque element INDEX costs ~3 VALU instructions of 64-bit arithmetic per load; opaque 64-bit pointers
// cost register pairs).
template <typename T = float>
__device__ __forceinline__ T tab_ld(const void* ubase, unsigned voff, int const_bytes) {
    return *reinterpret_cast<const T*>(static_cast<const char*>(ubase) + (size_t)voff + const_bytes);
}

// One half of a rotated 4096-sample block, the load of the three kernels of the 4096-sample plan (this one, leaf_fft_wgg4k_kernel,
// leaf_fft_wgg4k_bwd_kernel): v[r] = sample n = win.start + ((2 (64 r + lane) + odd + win.rot) & 4095) of clip win.b, zero outside
// [0, T) -- the even (odd = 0) or odd (odd = 1) samples, for the two half transforms.  One loop per sample kind, chosen once per half by
// wave-uniform branches: mixed with the partner clip (waveform mixup, leaf_common.hpp; mc = mix_clip(..), once per block) as fp32 or
// PCM16; else 16-bit (bfloat16 and PCM16 share the loop: a wave-uniform select of the conversion) or fp32.
struct Wg4kWindow {
    int b;                  // clip
    int start;              // clip sample under the block's first sample: n_c - padL
    int rot;                // the block is rotated left by this many samples: padL (static geometry) or K / 2
};
template <typename Sample>
__device__ __forceinline__ void wg4k_half_rows(const Wg4kWindow& win, int odd, int lane, float (&v)[32], Sample sample) {
#pragma unroll
    for (int r = 0; r < 32; ++r) v[r] = sample(win.start + ((2 * (64 * r + lane) + odd + win.rot) & (kFft4N - 1)));
}
__device__ __forceinline__ void wg4k_load_half(const FftParams& p, bool mixed, const MixClip& mc, const Wg4kWindow& win, int odd, int lane,
                                               float (&v)[32]) {
    const size_t row = (size_t)win.b * p.T;
    if (mixed) {
        if (p.io_bf16 == kSamplePcm16) wg4k_half_rows(win, odd, lane, v, [&](int n) { return mix_sample<kSamplePcm16>(p.x, row, mc, n, p.T); });
        else wg4k_half_rows(win, odd, lane, v, [&](int n) { return mix_sample<kSampleF32>(p.x, row, mc, n, p.T); });
    } else if (p.io_bf16) {
        const unsigned short* xh = static_cast<const unsigned short*>(p.x) + row;
        const bool pcm = p.io_bf16 == kSamplePcm16;
        wg4k_half_rows(win, odd, lane, v, [&](int n) {
            const unsigned h = xh[min(max(n, 0), p.T - 1)];
            const float w = pcm ? pcm16_widen((short)h) : __uint_as_float(h << 16);
            return (n >= 0 && n < p.T) ? w : 0.0f;
        });
    } else {
        const float* xb = static_cast<const float*>(p.x) + row;
        wg4k_half_rows(win, odd, lane, v, [&](int n) { return (n >= 0 && n < p.T) ? xb[n] : 0.0f; });
    }
}

template <int SK, int SHOP, int NW>
__global__ __launch_bounds__(NW * 64, (NW + 3) / 4) void leaf_fft_wg4k_kernel(const FftParams p) {
    static_assert(SK == 801 && SHOP == 320, "the 4096-sample plan is instantiated for the 32 kHz LEAF geometry");
    using gfp = const __attribute__((address_space(1))) float*;          // table pointers that stay `global` when made opaque
    using gf2p = const __attribute__((address_space(1))) v2f*;
    constexpr int SCRF = kWgScrFloats;                                    // full transposition scratch (round 4: no pooling rows in LDS)
    extern __shared__ __attribute__((aligned(16))) float wsm[];
    float2* twl = reinterpret_cast<float2*>(wsm);                        // [32][64]
    float2* twh = twl + 32 * 64;                                          // [32][2]
    float2* tw4a = twh + 64;                                              // w^(64 k), k < 32
    float2* tw4b = tw4a + 32;                                             // w^lane
    float2* ring = tw4b + 64;                                             // [2][kWg4RingFloat2]
    int* q = reinterpret_cast<int*>(ring + 2 * kWg4RingFloat2);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane0 = tid & 63;
    float* scr = reinterpret_cast<float*>(q + kWgQueueInts) + (size_t)wave * SCRF;
    const unsigned scr_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)scr);

    // band-limited filter tasks (leaf_band.hpp, round 5): the plan sits behind the waves' scratch
    const bool band_on = p.band.rec != nullptr;
    int* bl = reinterpret_cast<int*>(wsm + p.band.lds_off);
    if (band_on && wave == 0) band_build_plan(p.band.rec, p.band.elist, p.band.n_edge, p.F, bl, lane0, p.band.bias, p.band.smax);

    if (band_on) { if (wave > 0) fft_build_twiddles_wg(twl, twh, tid - 64, (NW - 1) * 64); }   // (wave 0 builds the plan meanwhile)
    else fft_build_twiddles_wg(twl, twh, tid, NW * 64);
    for (int i = tid; i < 96; i += NW * 64) {
        float s, c;
        sincospif(2.0f * (float)(i < 32 ? 64 * i : i - 32) / (float)kFft4N, &s, &c);
        tw4a[i] = make_float2(c, -s);                                     // (tw4b follows tw4a contiguously)
    }
    if (tid < kWgQueueInts) q[tid] = 0;
    __syncthreads();

    // full-rate geometry of the block and the half-rate geometry both halves share (= the 401 / 160 static geometry)
    constexpr int PADL = SK / 2 + SK % 2 - 1;                             // 400
    constexpr int LS = 3200;                                              // valid outputs per 4096-sample block (10 hops, 50 rows)
    constexpr int HK = (SK + 1) / 2, HHOP = SHOP / 2, HPADL = PADL / 2;   // 401, 160, 200
    constexpr int HLS = LS / 2;                                           // 1600 samples per half
    constexpr int DMIN = -((HK - 1 - HPADL) / HHOP);
    constexpr int DMAX = (HLS - 1 + HPADL) / HHOP;
    constexpr int NFR = DMAX - DMIN + 1;
    constexpr int NROW = HLS / 64;
    static_assert(NFR <= 16 && NROW == 25 && LS % SHOP == 0 && kFft4N - SK + 1 >= LS, "4096-sample plan geometry");
    // pooling weights of a half in registers: the half-rate geometry is the 401 / 160 one (wg_pool_nj: 15 vectors at stride 32)
    constexpr int PG = wg_pool_step(HHOP), PJ0 = wg_pool_jmin(HK, HHOP), NJ = wg_pool_nj(HK, HHOP);
    static_assert((HPADL - PJ0) % PG == 0, "window offsets are congruent to padL modulo gcd(64, hop)");

    // blocks dealt contiguously; clips all of whose blocks this workgroup ran are finalized in its tail (as leaf_fft_wg_kernel)
    const OwnedClips deal{p.B * p.nblk, (int)gridDim.x, p.nblk};
    const int first_gb = deal.start((int)blockIdx.x);
    const int nset = deal.count((int)blockIdx.x);
    // filter tasks per block: one per filter, or (band tasks) one per wide filter + one per four narrow-band filters
    const int NT = band_on ? __builtin_amdgcn_readfirstlane(bl[0]) : p.F;
    const int* tdesc = bl + kBandPlanHead;
    const int* bmem = tdesc + p.F + 4;
    const WgTaskCursor cur = wg_task_cursor(q, lane0, NT, nset);          // NT + 1 slots per set

    int seen_set = -1, seen_b = 0, seen_c = 0;                            // block coordinates of the set this wave last worked on
    int set = 0, role = 0;
    int t = cur.next(set, role);
    while (cur.has(t)) {
        int lane = lane0;
        asm volatile("" : "+v"(lane));
        const int slot = set & 1, gen = set >> 1;
        float2* A = ring + slot * kWg4RingFloat2;
        if (role == 0 || role > NT) {
            if (role == 0 && set < nset) {
                // ---- A' = FFT4096(rotated block), bins 0..2048, by decimation in time: Xe = FFT2048(even samples) parked in
                // the ring slot, Xo = FFT2048(odd samples), A'[e] = Xe[e] + w^e Xo[e], A'[2048] = Xe[0] - Xo[0]
                const int gb = first_gb + set;
                const int b = gb / p.nblk, c = gb - b * p.nblk;
                const int n_c = c * LS;
                // the block's two halves (wg4k_load_half, leaf_fft_wg4k.hpp); mixed: the partner clip and the weights, read once per block
                MixClip mc{};
                if (p.mix_lam) mc = mix_clip(p.mix_perm, p.mix_lam, b, p.B, p.T);
                const Wg4kWindow win{b, n_c - PADL, PADL};
                auto load_half = [&](float (&v)[32], int odd) { wg4k_load_half(p, p.mix_lam != nullptr, mc, win, odd, lane, v); };
                float xre[32], xim[32];
                load_half(xre, 0);
#pragma unroll
                for (int r = 0; r < 32; ++r) xim[r] = 0.0f;
                fft2048w<false>(xre, xim, scr, scr_lds, twl, twh, lane);
                wg_wait_ge(wgq_readers_cnt(q, slot), gen * NT);           // the slot's previous readers are done
#pragma unroll
                for (int i = 0; i < 32; ++i) A[64 * brev5(i) + lane] = make_float2(xre[i], xim[i]);
                load_half(xre, 1);
#pragma unroll
                for (int r = 0; r < 32; ++r) xim[r] = 0.0f;
                fft2048w<false>(xre, xim, scr, scr_lds, twl, twh, lane);
                const float2 wl = tw4b[lane];
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int k = brev5(i);
                    const float2 wk = tw4a[k];
                    const float wr = wk.x * wl.x - wk.y * wl.y, wi = wk.x * wl.y + wk.y * wl.x;      // w^(64 k + lane)
                    const float tr = xre[i] * wr - xim[i] * wi, ti = xre[i] * wi + xim[i] * wr;
                    const float2 xe = A[64 * k + lane];
                    A[64 * k + lane] = make_float2(xe.x + tr, xe.y + ti);
                    if (k == 0 && lane == 0) A[2048] = make_float2(xe.x - tr, xe.y - ti);
                }
                wg_publish(q, slot, b, c, lane);
            }
            t = cur.next(set, role);
            continue;
        }
        // ---- filter task of the block in ring slot `slot`.  Odd sets walk the tasks backwards: the per-filter tables (16 KB each
        // for this kernel; 1.3 MB at 80 filters, next to a 4 MB L2 per XCD) are swept once per block by every workgroup, and a
        // sweep that turns around re-reads the tables it used last while they are still resident instead of evicting them in order
        const int ti = (set & 1) ? NT - role : role - 1;
        const int tdsc = band_on ? __builtin_amdgcn_readfirstlane(tdesc[ti]) : ti << 2;   // class (0: one filter, two 2048-point halves; 2: band task) | index << 2
        const int f = tdsc >> 2;
        if (set != seen_set) {                                            // this wave's first filter of the block
            wg_acquire_block(q, slot, gen, seen_b, seen_c);
            seen_set = set;
        }
        const int b = seen_b, c = seen_c;
        const int n_c = c * LS;
        const int Lv = min(LS, p.T - n_c);
        int mlo = n_c + PADL - SK + 1;
        mlo = mlo <= 0 ? 0 : (mlo + SHOP - 1) / SHOP;
        const int mhi = min(p.TP - 1, (n_c + Lv - 1 + PADL) / SHOP);
        if (tdsc & 3) {
            // ---- band task: four narrow-band filters on 512-point transforms of their windows of the 4096-point spectrum
            // (decimation 8; leaf_band.hpp).  The filter's values for bins kb + j are R[4096 - kb - j] = R_hi[2048 - kb - j].
            const int* mem = bmem + (tdsc >> 2);
            float rq[32];
            {
                const int me1 = mem[lane / band_lpf(32)];
                const int fid = me1 & 0xffff, kb = (me1 >> 16) & 0xfff, c1 = lane & (band_lpf(32) - 1);
                const float* src = reinterpret_cast<const float*>(p.H) + (size_t)fid * kFft4TabFloats + 2 * (2048 - kb - c1) + 1;
                asm volatile("" ::: "memory");
#pragma unroll
                for (int k = 0; k < 32; ++k) rq[k] = src[-2 * (32 * (k & 15) + 16 * (k >> 4))];
                asm volatile("" ::: "memory");
            }
            int tn_b = 0, nset_b = 0, nrole_b = 0;
            auto mid = [&]() {
                tn_b = cur.next(nset_b, nrole_b);
                return 0;                                                 // no table loads for the next task
            };
            auto stamp = [&](int) {};
            auto bout = [&](int fid, int m, float v) {                    // the block's share of frame m: where the full task puts it
                const int first_block = max(0, m * SHOP - PADL) / LS;
                p.part[(((size_t)b * p.F + fid) * p.nslot + (c - first_block)) * p.TP + m] = v;
            };
            band_task<32, SK, SHOP, true>(p, rq, A, mem, bl + 4, twl, scr, scr_lds, q, slot, c, mlo, mhi, lane, mid, bout, stamp);
            t = tn_b;
            set = nset_b;
            role = nrole_b;
            continue;
        }
        const float* Rtab = reinterpret_cast<const float*>(p.H) + (size_t)f * kFft4TabFloats;   // R_lo[2048] | R_hi[2048] of this filter (wave-uniform)
        const unsigned lane4 = 4u * (unsigned)lane;
        const float* gsrc = p.Gz + (size_t)f * 2 * kWg4RowFloats + (kGPad + PJ0) + lane;   // de-interleaved pooling rows (even | odd taps)
        const unsigned a_dir = lds_addr(A + lane), a_mir = lds_addr(A + (2048 - 64 * 31) - lane);
        float zre[32], zim[32];
        // pooling of one half: sample j of the half (register i <-> j = 64 brev5(i) + lane) is output n_c + 2 j + h
        // (returns the wave-reduced frame sums of this half: after the butterfly every lane holds the total of frame
        // fi(lane); one register carried across the other half instead of sixteen accumulators)
        auto pool_half = [&](auto hh, const float (&pw)[NJ]) -> float {
            constexpr int h = decltype(hh)::value;
            float acc[16];
#pragma unroll
            for (int fi = 0; fi < 16; ++fi) acc[fi] = 0.0f;
            float er[NROW];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int r = brev5(i);
                if (r < NROW) er[r] = zre[i] * zre[i] + zim[i] * zim[i];
            }
            if (Lv < LS) {
#pragma unroll
                for (int r = 0; r < NROW; ++r) er[r] = 2 * (64 * r + lane) + h < Lv ? er[r] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < NROW; ++r) {
#pragma unroll
                for (int fi = 0; fi < NFR; ++fi) {
                    const int is = (DMIN + fi) * HHOP - HPADL;            // first half-rate sample of frame fi's window
                    if (is <= 64 * r + 63 && is + HK > 64 * r) acc[fi] = fmaf(er[r], pw[(64 * r - is - PJ0) / PG], acc[fi]);
                }
            }
            return frame_butterfly16(acc, lane);
        };
        // ---- even output samples: zs = conj(A'[e]) R_lo[e] + A'[2048 - e] R_hi[e]
        {
            auto chunk = [&](auto cc) {
                constexpr int C = decltype(cc)::value;
                float rl[8], rh[8];
                // the table offset is made opaque HERE: the loads below cannot issue before this point (a plain "memory"
                // clobber does not hold them -- they are hoisted under the previous phase and spilled one by one)
                // (the chunk's table POINTERS, in the global address space so that the loads stay global_load: its eight loads per
                // table then differ by an immediate offset only -- an opaque index cost ~3 VALU instructions of 64-bit address
                // arithmetic per load)
                unsigned vo = lane4;
                if constexpr (C > 0) asm volatile("" : "+v"(vo), "+v"(zre[8 * C - 1]), "+v"(zim[8 * C - 1]) : : "memory");
                else asm volatile("" : "+v"(vo) : : "memory");
#pragma unroll
                for (int j = 0; j < 8; ++j) { const v2f r = tab_ld<v2f>(Rtab, 2u * vo, 512 * (8 * C + j)); rl[j] = r.x; rh[j] = r.y; }
                asm volatile("" ::: "memory");
                v2f a[8], m[8];
                wg4k_ring_chunk<C>(a, m, a_dir, a_mir);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int k = 8 * C + j;
                    zre[k] = fmaf(m[j].x, rh[j], a[j].x * rl[j]);
                    zim[k] = fmaf(m[j].y, rh[j], -(a[j].y * rl[j]));
                }
                asm volatile("" : "+v"(zre[8 * C]), "+v"(zre[8 * C + 1]), "+v"(zre[8 * C + 2]), "+v"(zre[8 * C + 3]),
                                  "+v"(zre[8 * C + 4]), "+v"(zre[8 * C + 5]), "+v"(zre[8 * C + 6]), "+v"(zre[8 * C + 7]),
                                  "+v"(zim[8 * C]), "+v"(zim[8 * C + 1]), "+v"(zim[8 * C + 2]), "+v"(zim[8 * C + 3]),
                                  "+v"(zim[8 * C + 4]), "+v"(zim[8 * C + 5]), "+v"(zim[8 * C + 6]), "+v"(zim[8 * C + 7]));
            };
            chunk(std::integral_constant<int, 0>{}); chunk(std::integral_constant<int, 1>{});
            chunk(std::integral_constant<int, 2>{}); chunk(std::integral_constant<int, 3>{});
        }
        // this half's pooling weights: requested now, they land under the transform
        float pw[NJ];
        auto load_weights = [&](int h) {
            asm volatile("" ::: "memory");
#pragma unroll
            for (int k = 0; k < NJ; ++k) pw[k] = gsrc[h * kWg4RowFloats + PG * k];
            asm volatile("" ::: "memory");
        };
        load_weights(0);
        fft2048w<false>(zre, zim, scr, scr_lds, twl, twh, lane);
        pin32(zre);
        pin32(zim);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the weights have landed
        float v_even = pool_half(std::integral_constant<int, 0>{}, pw);
        // the first half's pooling is complete before the second half's table loads issue (else they are hoisted under it
        // and spilled one by one)
        asm volatile("" : "+v"(v_even) : : "memory");
        // ---- odd output samples: zd = (conj(A'[e]) R_lo[e] - A'[2048 - e] R_hi[e]) w^e
        {
            [[maybe_unused]] const float2 wl_odd = tw4b[lane];
            auto step = [&](auto cc) {                                    // four rows at a time (registers): k = 4 C4 .. 4 C4 + 3
                constexpr int C4 = decltype(cc)::value;
                unsigned vo = lane4;
                if constexpr (C4 > 0) asm volatile("" : "+v"(vo), "+v"(zre[4 * C4 - 1]), "+v"(zim[4 * C4 - 1]) : : "memory");
                else asm volatile("" : "+v"(vo) : : "memory");
                float rl[4], rh[4];
                v2f w[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const v2f r = tab_ld<v2f>(Rtab, 2u * vo, 512 * (4 * C4 + j));
                    rl[j] = r.x;
                    rh[j] = r.y;
                    const float2 wk = tw4a[4 * C4 + j];                   // w^(64 k + lane) = w^(64 k) w^lane, both in LDS
                    w[j].x = wk.x * wl_odd.x - wk.y * wl_odd.y;
                    w[j].y = wk.x * wl_odd.y + wk.y * wl_odd.x;
                }
                asm volatile("" ::: "memory");
                v2f a[4], m[4];
                lds_rd8<512 * (4 * C4 + 0)>(a[0], a_dir); lds_rd8<512 * (4 * C4 + 1)>(a[1], a_dir);
                lds_rd8<512 * (4 * C4 + 2)>(a[2], a_dir); lds_rd8<512 * (4 * C4 + 3)>(a[3], a_dir);
                lds_rd8<512 * (31 - (4 * C4 + 0))>(m[0], a_mir); lds_rd8<512 * (31 - (4 * C4 + 1))>(m[1], a_mir);
                lds_rd8<512 * (31 - (4 * C4 + 2))>(m[2], a_mir); lds_rd8<512 * (31 - (4 * C4 + 3))>(m[3], a_mir);
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(m[0]), "+v"(m[1]),
                                                      "+v"(m[2]), "+v"(m[3]));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = 4 * C4 + j;
                    // P = conj(a) rl - m rh = (ur, -ui);  zd = P w:  Re = ur w.x + ui w.y,  Im = ur w.y - ui w.x
                    const float ur = fmaf(-m[j].x, rh[j], a[j].x * rl[j]);
                    const float ui = fmaf(m[j].y, rh[j], a[j].y * rl[j]);
                    zre[k] = fmaf(ui, w[j].y, ur * w[j].x);
                    zim[k] = fmaf(ur, w[j].y, -(ui * w[j].x));
                }
                // every product of this step is complete before the next step's loads issue (VALU work may otherwise sink
                // below later volatile statements, keeping several steps' operands alive at once)
                asm volatile("" : "+v"(zre[4 * C4]), "+v"(zre[4 * C4 + 1]), "+v"(zre[4 * C4 + 2]), "+v"(zre[4 * C4 + 3]),
                                  "+v"(zim[4 * C4]), "+v"(zim[4 * C4 + 1]), "+v"(zim[4 * C4 + 2]), "+v"(zim[4 * C4 + 3]));
            };
            step(std::integral_constant<int, 0>{}); step(std::integral_constant<int, 1>{});
            step(std::integral_constant<int, 2>{}); step(std::integral_constant<int, 3>{});
            step(std::integral_constant<int, 4>{}); step(std::integral_constant<int, 5>{});
            step(std::integral_constant<int, 6>{}); step(std::integral_constant<int, 7>{});
        }
        wg_reader_done(q, slot, lane);                                    // ring reads done
        load_weights(1);                                                  // the odd taps' weights, under the second transform
        fft2048w<false>(zre, zim, scr, scr_lds, twl, twh, lane);
        pin32(zre);
        pin32(zim);
        int nset_i = 0, nrole = 0;
        const int tn = cur.next(nset_i, nrole);                                      // next task reserved under the pooling
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // the weights have landed
        const float v_odd = pool_half(std::integral_constant<int, 1>{}, pw);
        {
            const float v = v_even + v_odd;
            const int fi = ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
            const int m = n_c / SHOP + DMIN + fi;
            if ((lane & 3) == 0 && fi < NFR && m >= mlo && m <= mhi) {
                const int first_block = max(0, m * SHOP - PADL) / LS;
                p.part[(((size_t)b * p.F + f) * p.nslot + (c - first_block)) * p.TP + m] = v;
            }
        }
        t = tn;
        set = nset_i;
        role = nrole;
    }
    if (p.fin_fused)                                                      // the waves' rows are free: tile memory of the tail
        wg_tail_finalize<64>(p.fin, (first_gb + p.nblk - 1) / p.nblk, (first_gb + nset) / p.nblk,
                             reinterpret_cast<float*>(q + kWgQueueInts), tid, (int)blockDim.x);
}

}  // namespace
