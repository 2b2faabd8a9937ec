// leaf_fft_stream.hpp -- one step of a running stream in ONE launch (leaf_stream_step_f32)
// Included by every unit: templates, device functions, constexpr sizes (gfx950 only); instantiated in inst_fft_stream.hip, see leaf_inst.hpp.
//
// Why: chunked real-time inference (LeafStream) ran torch.cat -> the whole fused forward over [history | chunk] -> slice ->
// leaf_pcen_stream_f32 -> slice: two product launches and four stock ones per 10..100 ms of audio, host-bound.  The one-launch
// small-batch kernel (leaf_fft_small.hpp) already keeps a (clip, filter) row inside one workgroup from the tables to PCEN; this
// is that kernel with what a stream step needs and nothing it does not (no SPLIT form, no mixup, no second ring pass):
//
//     workgroup = (stream b, filter f), grid = (F, B), 11 waves -- the small kernel's building blocks, its phases, its LDS layout
//
//   * the clip is the VIRTUAL concatenation [hist_in[b][0..hist_len) | chunk[b][0..Tc)]: the block load resolves each sample to
//     one of the two buffers (one predicated load per sample; outside [0, hist_len + Tc) nothing is read and the sample is zero,
//     so hist_len = 0 reads no history and Tc = 0 no chunk).  `chunk` has a row stride: a slice of a recording goes in as it is.
//   * only frames first .. first + n - 1 (numbered from the virtual buffer's start) are summed, finalized and stored, compactly
//     to out[B][F][n]; only the blocks c_lo .. c_lo + nb - 1 their windows meet are transformed (nb <= kSmallRing: one pass).
//     The clip-end masking stays keyed to the virtual length: it is the reference's zero padding behind the last sample when the
//     host flushes, and touches no emitted frame otherwise (the host emits a frame only once its receptive field is complete).
//   * mode bit 0 (PCEN): the smoother's state in front of the first emitted frame is ema_state[b][f] once the stream has
//     started, else that frame's own floored pooled value (postprocessing.py:15); the state after the last emitted frame goes
//     back to ema_state[b][f].  The workgroup is that word's only reader and writer: nothing here waits for another workgroup.
//   * the workgroups with f == 0 hand the history over: samples [drop, hist_len + Tc) of the virtual buffer go to the OTHER
//     history half (hist_out), which no workgroup of this launch reads; the host flips the parity.  Plain vector loads and
//     stores in the stream's own sample type, by the waves that idle while wave 0 finalizes the row.
//   * n == 0 (a chunk too short to complete a frame): the host launches grid (1, B) and the kernel only moves history.
//
// The bank (leaf_stream_bank_step_f32, leaf_fft_stream_bank_kernel): B INDEPENDENT streams in one launch.  A workgroup is still one
// (slot b, filter f), reads only row b of the history and word (b, f) of the smoother state and waits for no other workgroup; what
// the uniform step takes from StreamParams -- where the stream stands -- it takes from slot b's record instead:
//   * the records travel BY VALUE in the kernel's parameter struct (StreamBankParams: kBankSlots packed records of 24 bytes, the
//     struct stays below 4 KB; a larger bank is several launches).  The host computes and checks every field (StreamPassRec).  blockIdx.y is wave-uniform, so a record comes in through scalar
//     loads from the argument segment: no plan buffer on the device, no copy, no readback.
//   * slot b reads history half parity_b, row b, and writes the other half, row b (the layout is leaf_stream_state_bytes').
//   * out is [B][F][n_max]: a row holds the slot's frames and zeros behind them, every element written by the row's workgroup.  An
//     idle slot's workgroups write their zeros and touch nothing else: no history, no smoother word.
//   * the dynamic LDS is sized by the launch's largest frame count (n_lds): what is laid out behind lsum sits at that offset.
//   * a stream that ENDS on a chunk that also completes frames takes two passes of the body in the same workgroup: the step's frames
//     from [history | chunk], then the frames still owed from the samples [drop, hist_len + Tc) of that buffer, numbered from `drop`
//     with the reference's zero padding behind the last sample -- the very buffer, block alignment included, a uniform stream's
//     final step would read from the history it had just been handed, so the frames are the same bits.  Nothing is handed over (the
//     stream ends); the smoother's state goes from the first pass to the second through the row's own state word, behind the
//     workgroup barrier that also separates the two passes' use of the LDS.
//
// ONE device body (leaf_fft_stream_body) and two entries: the position (StreamPos) is built from the uniform parameters or from
// the slot's record; in the uniform step its extra fields are constants (no offsets, rows of n frames) and fold away.
//
// The transform loop is the small kernel's two-trip loop through ONE copy of fft2048w, and for the same reason: the code runs
// once per launch from a cold instruction cache.
#pragma once
#include "leaf_fft_small.hpp"

namespace {

// one pass of stream b at position s; dynamic LDS: the small kernel's layout with s.n_lds frame sums.  BANK: out rows are longer
// than the pass's frames and get their zeros here (the uniform step has no such columns and carries no code for them)
template <int SK, int SHOP, bool BANK>
__device__ __forceinline__ void leaf_fft_stream_body(const StreamParams& p, const StreamPos& s, const int b, const int tid) {
    constexpr int NW = kSmallWaves;
    constexpr int SCRF = kWgScrFloats;
    constexpr int PADL = SK / 2 + SK % 2 - 1;
    constexpr int LS = fft_block_len(SK, SHOP, true);
    constexpr int DMIN = -((SK - 1 - PADL) / SHOP);
    constexpr int DMAX = (LS - 1 + PADL) / SHOP;
    constexpr int NFR = DMAX - DMIN + 1;
    constexpr int NROW = LS / 64;
    constexpr int NGRP = (NFR + 15) / 16;
    constexpr int PG = wg_pool_step(SHOP), PJ0 = wg_pool_jmin(SK, SHOP), NJ = wg_pool_nj(SK, SHOP);
    static_assert(LS % SHOP == 0 && LS % 64 == 0 && LS > 0 && NFR <= 32 && (SK & 1) && SK <= kFftN / 2 + 1, "static odd-window geometry");
    static_assert((PADL - PJ0) % PG == 0, "window offsets are congruent to padL modulo gcd(64, hop)");

    extern __shared__ __attribute__((aligned(16))) float ssm[];
    float2* twl = reinterpret_cast<float2*>(ssm);                        // [32][64]
    float2* twp = twl + 32 * 64;                                          // [2][16][2]
    float* R = reinterpret_cast<float*>(twp + 64);                        // [2048]; first the taps, conj(w)[K] as float2
    float* scr0 = R + kFftN;
    float* lsum = scr0 + (size_t)NW * SCRF;                               // [n]: the emitted frames' sums
    FinCoef* cfs = reinterpret_cast<FinCoef*>(lsum + (s.n_lds + 3) / 4 * 4);  // the row's finalize coefficients (phase 0 -> phase 3)
    float* gw = reinterpret_cast<float*>(cfs + 1);                        // [NJ][64]: the filter's pooling-weight vectors (phase 0 -> phase 2)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int lane = tid & 63;
    const int f = blockIdx.x;
    const int hl = s.hist_len, T = s.hist_len + s.Tc;                     // the virtual buffer's length
    const int TPv = T > 0 ? (T - 1) / SHOP + 1 : 0;                       // ... and its frames

    // the history hand-over (f == 0 only): virtual samples [drop, T) -> hist_out[b][0 .. T - drop), by threads t0, t0 + nt, ...
    auto move_history = [&](int t0, int nt) {
        const int drop = s.drop, tail = T - drop;
        if (p.pcm) {
            const unsigned short* hi = static_cast<const unsigned short*>(s.hist_in) + (size_t)b * p.H + s.hist_off;
            const unsigned short* ch = static_cast<const unsigned short*>(p.chunk) + (size_t)b * (size_t)p.chunk_stride + s.chunk_off;
            unsigned short* ho = static_cast<unsigned short*>(s.hist_out) + (size_t)b * p.H;
            for (int j = t0; j < tail; j += nt) {
                const int v = j + drop;
                ho[j] = v < hl ? hi[v] : ch[v - hl];
            }
        } else {
            const float* hi = static_cast<const float*>(s.hist_in) + (size_t)b * p.H + s.hist_off;
            const float* ch = static_cast<const float*>(p.chunk) + (size_t)b * (size_t)p.chunk_stride + s.chunk_off;
            float* ho = static_cast<float*>(s.hist_out) + (size_t)b * p.H;
            for (int j = t0; j < tail; j += nt) {
                const int v = j + drop;
                ho[j] = v < hl ? hi[v] : ch[v - hl];
            }
        }
    };
    // the row's columns behind its frames (the bank's out rows are n_max long; none in the uniform step), by threads t0, t0 + nt, ...
    auto zero_tail = [&](int t0, int nt) {
        if constexpr (BANK)
            for (int k = s.o_lo + s.n + t0; k < s.o_end; k += nt) fin_store(p.fin, ((size_t)b * p.F + f) * s.n_row + k, 0.0f);
    };
    if (s.n == 0) {                                                       // nothing to emit: history only (grid (1, B) when no row of out exists)
        zero_tail(tid, NW * 64);
        if (f == 0) move_history(tid, NW * 64);
        return;
    }

    float* scr = scr0 + (size_t)wave * SCRF;
    const unsigned scr_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)scr);
    // ---- phase 0 (leaf_fft_small.hpp): the filter's parameters, then tables, taps, zeroed sums, pooling weights
    const float mu = p.kernel[2 * f], sg = p.kernel[2 * f + 1], pw_raw = p.pool_w[f];
    const int row = b * p.F + f;
    float M = 0.0f;                                                       // the smoother's state (wave 0): requested here, used in phase 3
    if (wave == 0 && (p.fin.mode & 1) && s.started) M = p.ema_state[row];
    float zre[32], zim[32];             // a block wave's samples -> spectrum (kept across the barrier) -> filter outputs
    auto load_block = [&](int c, int lane_) {                             // block c of the virtual buffer, rotated left by padL samples
        const int n_c = c * LS;
        if (p.pcm) {
            const short* hi = static_cast<const short*>(s.hist_in) + (size_t)b * p.H + s.hist_off;
            const short* ch = static_cast<const short*>(p.chunk) + (size_t)b * (size_t)p.chunk_stride + s.chunk_off - hl;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = 64 * r + lane_;
                const int s = n_c - PADL + ((i + PADL) & (kFftN - 1));
                const short* src = (s < hl ? hi : ch) + s;
                zre[r] = (s >= 0 && s < T) ? pcm16_widen(*src) : 0.0f;
                zim[r] = 0.0f;
            }
        } else {
            const float* hi = static_cast<const float*>(s.hist_in) + (size_t)b * p.H + s.hist_off;
            const float* ch = static_cast<const float*>(p.chunk) + (size_t)b * (size_t)p.chunk_stride + s.chunk_off - hl;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = 64 * r + lane_;
                const int s = n_c - PADL + ((i + PADL) & (kFftN - 1));
                const float* src = (s < hl ? hi : ch) + s;
                zre[r] = (s >= 0 && s < T) ? *src : 0.0f;
                zim[r] = 0.0f;
            }
        }
    };
#pragma unroll
    for (int r = 0; r < 32; ++r) { zre[r] = 0.0f; zim[r] = 0.0f; }
    fft_build_twiddles_wg(twl, twp, tid, NW * 64);
    {
        float2* taps = reinterpret_cast<float2*>(R);
        for (int j = tid; j < SK; j += NW * 64) {
            float a, c;
            gabor_tap(mu, sg, p.bd, (float)(j - SK / 2), a, c);
            taps[j] = make_float2(a, -c);                                 // conj(w), as fft_prep_kernel
        }
    }
    for (int m = tid; m < s.n; m += NW * 64) lsum[m] = 0.0f;
    if (tid == 64) cfs[0] = fin_coef(p.fin, f);
    {
        const float half = 0.5f * (float)(SK - 1);
        const float den = pool_sigma(pw_raw, SK) * half;
        for (int t = tid; t < NJ * 64; t += NW * 64) {
            const int j = PJ0 + PG * (t >> 6) + (t & 63);
            const float q = ((float)j - half) / den;
            const float v = expf(-0.5f * (q * q));
            gw[t] = (j >= 0 && j < SK) ? v : 0.0f;
        }
    }
    __syncthreads();

    // Phases 1 and 2 through ONE copy of the wave-level transform (deliberately NOT unrolled: leaf_fft_small.hpp): trip 0 = the
    // forward transforms of the blocks and the table wave's, trip 1 = the filter tasks
#pragma nounroll
    for (int step = 0; step < 2; ++step) {
        const bool inv = step != 0;
        const bool table = !inv && wave == NW - 1;
        if (wave < s.nb || table) {
            asm volatile("" : "+v"(lane));
            const int c = s.c_lo + wave, n_c = c * LS;
            if (table) {
                const float2* taps = reinterpret_cast<const float2*>(R);
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    const int i = 64 * r + lane;
                    const int j = (i < kFftN / 2 ? i : i - kFftN) + SK / 2;
                    const float2 t = taps[min(max(j, 0), SK - 1)];
                    zre[r] = (j >= 0 && j < SK) ? t.x : 0.0f;
                    zim[r] = (j >= 0 && j < SK) ? t.y : 0.0f;
                }
            } else if (!inv) {
                load_block(c, lane);
            } else {
                // Z = conj(A') R_f, in place (leaf_fft_small.hpp: register i <-> bin 64 brev5(i) + lane)
                float rq[32];                                             // R_f[64 k + lane]
#pragma unroll
                for (int k = 0; k < 32; ++k) rq[k] = R[64 * k + lane];
#pragma unroll
                for (int k = 0; k < 32; ++k) {
                    const int j = brev5(k);
                    if (j == k) {
                        zre[k] = zre[k] * rq[k];
                        zim[k] = -(zim[k] * rq[k]);
                    } else if (j > k) {
                        const float ar = zre[k], ai = zim[k];
                        zre[k] = zre[j] * rq[k];
                        zim[k] = -(zim[j] * rq[k]);
                        zre[j] = ar * rq[j];
                        zim[j] = -(ai * rq[j]);
                    }
                }
            }
            pin32(zre);
            pin32(zim);
            fft2048w<false>(zre, zim, scr, scr_lds, twl, twp, lane);     // register i <-> element 64 brev5(i) + lane
            pin32(zre);
            pin32(zim);
            if (table) {
#pragma unroll
                for (int i = 0; i < 32; ++i) R[64 * brev5(i) + lane] = zre[i] * (1.0f / kFftN);   // imaginary parts: rounding noise
            } else if (inv) {
                const int Lv = min(LS, T - n_c);
                int mlo = n_c + PADL - SK + 1;                            // first frame whose window reaches the block
                mlo = mlo <= 0 ? 0 : (mlo + SHOP - 1) / SHOP;
                mlo = max(mlo, s.first);                                  // ... that is emitted
                const int mhi = min(min(TPv, s.first + s.n) - 1, (n_c + Lv - 1 + PADL) / SHOP);
                float er[NROW];
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int r = brev5(i);
                    if (r < NROW) er[r] = zre[i] * zre[i] + zim[i] * zim[i];
                }
                if (Lv < LS) {                                            // the virtual buffer's last block: outputs past its end
#pragma unroll
                    for (int r = 0; r < NROW; ++r) er[r] = 64 * r + lane < Lv ? er[r] : 0.0f;
                }
                float pw[NJ];                                             // the filter's weight vectors (phase 0)
#pragma unroll
                for (int k = 0; k < NJ; ++k) pw[k] = gw[64 * k + lane];
                float acc[NGRP][16];
#pragma unroll
                for (int g = 0; g < NGRP; ++g)
#pragma unroll
                    for (int fi = 0; fi < 16; ++fi) acc[g][fi] = 0.0f;
#pragma unroll
                for (int r = 0; r < NROW; ++r) {
#pragma unroll
                    for (int fi = 0; fi < NFR; ++fi) {
                        const int is = (DMIN + fi) * SHOP - PADL;
                        if (is <= 64 * r + 63 && is + SK > 64 * r)
                            acc[fi / 16][fi % 16] = fmaf(er[r], pw[(64 * r - is - PJ0) / PG], acc[fi / 16][fi % 16]);
                    }
                }
                asm volatile("" : "+v"(acc[0][0]));
#pragma unroll
                for (int g = 0; g < NGRP; ++g) {
                    const float v = frame_butterfly16(acc[g], lane);
                    const int fi = 16 * g + ((lane >> 5) & 1) * 8 + ((lane >> 4) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 2) & 1);
                    const int m = n_c / SHOP + DMIN + fi;
                    if ((lane & 3) == 0 && fi < NFR && m >= mlo && m <= mhi)
                        __hip_atomic_fetch_add(&lsum[m - s.first], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
        __syncthreads();            // R complete / sums complete
    }
    // ---- phase 3: the emitted frames of row (b, f) by wave 0, 64 at a time (leaf_fft_small.hpp: the EMA recurrence as a lane scan);
    // the other waves of the f == 0 workgroups move the history meanwhile
    if (wave == 0) {
        const FinParams& fin = p.fin;
        const int mode = fin.mode;
        const FinCoef cf = cfs[0];
        for (int m0 = 0; m0 < s.n; m0 += 64) {
            const int k = m0 + lane;
            const bool on = k < s.n;
            float x = pooled_floor(fin_pooled(lsum[on ? k : 0], 0.0f, 0.0f, 1, false, 1.0f, cf.bias));
            float Mv = 0.0f;
            if (mode & 1) {
#pragma clang fp contract(off)
                float sa = on ? cf.omw : 1.0f, sb = on ? cf.w * x : 0.0f;
                wave_affine_scan(sa, sb);
                // the state before the chunk's first frame: the stream's first frame itself (postprocessing.py:15), the state the
                // previous step left, or the previous 64 frames' last
                const float carry = (m0 == 0 && !s.started) ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))) : M;
                Mv = sa * carry + sb;
                M = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(Mv), min(64, s.n - m0) - 1));
            }
            const float o = fin_point(cf, mode, fin.floor_, x, Mv);
            if (on) fin_store(fin, (size_t)row * s.n_row + s.o_lo + k, o);
        }
        if ((mode & 1) && lane == 0) p.ema_state[row] = M;                // after the last emitted frame: the next step's carry
    } else {
        zero_tail(tid - 64, (NW - 1) * 64);
        if (f == 0) move_history(tid - 64, (NW - 1) * 64);
    }
}

// the uniform step: every stream stands where StreamParams says; dynamic LDS fft_small_lds_bytes(kSmallWaves, n)
template <int SK, int SHOP>
__global__ __launch_bounds__(kSmallWaves * 64, 3) void leaf_fft_stream_kernel(const StreamParams p) {
    const StreamPos s{p.hist_in, p.hist_out, p.hist_len, p.Tc, p.drop, p.first, p.n, p.started, p.c_lo, p.nb, 0, 0, p.n, p.n, 0, p.n};
    leaf_fft_stream_body<SK, SHOP, false>(p, s, blockIdx.y, threadIdx.x);
}

// the bank: slot blockIdx.y of this launch stands where its record says; dynamic LDS fft_small_lds_bytes(kSmallWaves, n_lds)
template <int SK, int SHOP>
__global__ __launch_bounds__(kSmallWaves * 64, 3) void leaf_fft_stream_bank_kernel(const StreamBankParams q) {
    // The arguments are read through the argument segment's own address, taken anew in every trip: what a trip loads it loads for
    // itself (scalar loads), and nothing but the record's index is carried across the body.  (Read through `q`, every argument is
    // loop-invariant, stays in scalar registers across both trips and costs the kernel scratch.)
    // Likewise the thread's index: the wave's number is kept in a scalar register and the lane's is counted anew in every trip.
    const int y = blockIdx.y, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int i = (int)((q.first[y >> 2] >> (8 * (y & 3))) & 0xff);
#pragma nounroll
    for (;;) {                                                            // one trip, or two for a stream that ends (header comment)
        const __attribute__((address_space(4))) StreamBankParams* a =
            (const __attribute__((address_space(4))) StreamBankParams*)__builtin_amdgcn_kernarg_segment_ptr();
        int yy = y, tid = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        asm volatile("" : "+s"(a), "+s"(yy), "+v"(tid));                  // (nothing derived from them is hoisted out of the loop)
        tid += 64 * wave;
        const StreamBankParams& g = *(const StreamBankParams*)a;
        const unsigned w0 = g.rec[i].w[0], w1 = g.rec[i].w[1], w2 = g.rec[i].w[2], w3 = g.rec[i].w[3], w4 = g.rec[i].w[4], w5 = g.rec[i].w[5];
        const bool par = (w5 & 2) != 0, idle = (w5 & 4) != 0;             // an idle slot: an empty pass (its zeros, nothing else)
        StreamPos s;
        s.hist_in = par ? static_cast<const void*>(g.c.hist_out) : g.c.hist_in;
        s.hist_out = par ? const_cast<void*>(g.c.hist_in) : g.c.hist_out;
        s.hist_len = idle ? 0 : (int)(w0 & 0xffff); s.Tc = idle ? 0 : (int)(w0 >> 16); s.drop = idle ? 0 : (int)(w1 & 0xffff);
        s.first = (int)(w1 >> 16); s.n = idle ? 0 : (int)(w2 & 0xffff); s.started = (int)(w5 & 1);
        s.c_lo = (int)((w2 >> 16) & 0xff); s.nb = (int)(w2 >> 24);
        s.hist_off = (int)(w3 & 0xffff); s.chunk_off = (int)(w3 >> 16);
        s.n_lds = g.n_lds; s.n_row = g.n_max;
        s.o_lo = (int)(w4 & 0xffff); s.o_end = (int)(w4 >> 16);
        leaf_fft_stream_body<SK, SHOP, true>(g.c, s, g.b0 + yy, tid);
        if (w5 & 8) break;
        ++i;
        __syncthreads();                                                  // the pass is done with the LDS; its smoother state word is visible
    }
}

}  // namespace
