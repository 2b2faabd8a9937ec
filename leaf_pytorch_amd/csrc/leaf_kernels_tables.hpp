// leaf_kernels_tables.hpp -- the table kernels: tap tables, pooling windows, filter spectra, the band tasks' tables, index maps
// Included by leaf_kernels.hip only: kernels (plain __global__ functions, and the device helpers nothing else calls).  A header
// that an inst_*.hip unit includes holds none: every kernel of the library is compiled in exactly one translation unit
// (tests/test_host_early_forward.py counts them in the built library).
#pragma once
#include "leaf_fft_wg4k.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// tap tables
// ---------------------------------------------------------------------------------------------

// Direct table, the layout convolution.py:88-90 hands to conv1d: taps[2f][j] = Re, taps[2f+1][j] = Im,
// t_j = j - K/2.
__global__ void taps_direct_kernel(const float* __restrict__ kernel, int F, int K, GaborBounds bd,
                                   float* __restrict__ taps) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * K) return;
    const int f = idx / K, j = idx - f * K;
    float re, im;
    gabor_tap(kernel[2 * f], kernel[2 * f + 1], bd, (float)(j - K / 2), re, im);
    taps[(size_t)(2 * f) * K + j] = re;
    taps[(size_t)(2 * f + 1) * K + j] = im;
}

__global__ void lowpass_window_kernel(const float* __restrict__ pool_w, int F, int K, float* __restrict__ g) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * K) return;
    const int f = idx / K, j = idx - f * K;
    const float half = 0.5f * (float)(K - 1);
    const float q = ((float)j - half) / (pool_sigma(pool_w[f], K) * half);
    g[idx] = expf(-0.5f * (q * q));
}

// One launch builds everything the fused kernel needs from the raw parameters:
//   perm[col]   filter index held by tap column col (columns are sorted by decreasing half-support so each
//               16-column MFMA tile groups filters of similar width); -1 for padding columns
//   col_of[f]   inverse map
//   tile_ks[t]  number of 4-row k-steps tile t needs = ceil((largest half-support in the tile + 1)/4)
//   W[kk][c]    c <  FP: Re tap of filter perm[c] at t=+kk;  c >= FP: Im tap of filter perm[c-FP]
//               (zero beyond that filter's own half-support, so a filter's result never depends on its tile
//               mates).  Row 0 carries hr[0]/2 because the kernel forms s_0 = x[n] + x[n].
//   G[c][j]     Gaussian pooling window of filter perm[c] (impulse_responses.py:74-80), j = 0..GJ-1, ZERO for
//               j >= K: the fused epilogue reads it with 16-byte loads and needs no window masks.
// Every block recomputes the (tiny) ordering in LDS; block 0 publishes it.
__global__ __launch_bounds__(256) void fused_prep_kernel(const float* __restrict__ kernel,
                                                         const float* __restrict__ pool_w, int F, int FP, int K, int R,
                                                         int GJ, GaborBounds bd, float* __restrict__ W,
                                                         float* __restrict__ G, float* __restrict__ Gs,
                                                         int* __restrict__ perm, int* __restrict__ col_of,
                                                         int* __restrict__ tile_ks) {
    __shared__ int s_sup[kMaxFP];        // half-support per filter slot (-1 = padding)
    __shared__ int s_perm[kMaxFP];
    const int tid = threadIdx.x;
    const int Hb = K / 2;
    for (int c = tid; c < FP; c += 256) {
        int sup = -1;
        if (c < F) {
            const float sg = fminf(fmaxf(kernel[2 * c + 1], bd.sigma_lo), bd.sigma_hi);
            sup = min(Hb, (int)ceilf(kTapCut * sg));
        }
        s_sup[c] = sup;
    }
    __syncthreads();
    for (int c = tid; c < FP; c += 256) {
        const int mine = s_sup[c];
        int rank = 0;
        for (int o = 0; o < FP; ++o) {
            const int other = s_sup[o];
            rank += (other > mine) || (other == mine && o < c);
        }
        s_perm[rank] = c;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int c = tid; c < FP; c += 256) {
            const int f = s_perm[c];
            perm[c] = f < F ? f : -1;
            if (f < F) col_of[f] = c;
            if ((c & 15) == 0) tile_ks[c >> 4] = (s_sup[f] + 1 + 3) / 4;     // sorted: first column of a tile is its widest
        }
    }
    int idx = blockIdx.x * 256 + tid;
    const int ncol = 2 * FP;
    if (idx >= R * ncol) {
        idx -= R * ncol;
        if (idx < FP * GJ) {
            const int c = idx / GJ, j = idx - c * GJ;
            const int f = s_perm[c];
            float v = 0.0f, dv = 0.0f;
            if (f < F && j < K) {
                const float half = 0.5f * (float)(K - 1);
                const float sig = pool_sigma(pool_w[f], K);
                const float q = ((float)j - half) / (sig * half);
                v = expf(-0.5f * (q * q));
                dv = v * (q * q) / sig;                  // d g / d s = g (j-c)^2 / (c^2 s^3)
            }
            G[idx] = v;
            if (Gs) Gs[idx] = dv;                        // backward only
        }
        return;
    }
    const int kk = idx / ncol, col = idx - kk * ncol;
    const bool is_im = col >= FP;
    const int f = s_perm[is_im ? col - FP : col];
    float v = 0.0f;
    if (f < F && kk <= s_sup[f]) {
        float re, im;
        gabor_tap(kernel[2 * f], kernel[2 * f + 1], bd, (float)kk, re, im);
        v = is_im ? im : re;
        if (kk == 0) v *= 0.5f;
    }
    W[idx] = v;
}

__global__ __launch_bounds__(kPrepWaves * 64) void fft_prep_kernel(const float* __restrict__ kernel,
                                                                   const float* __restrict__ pool_w, int F, int K, int GZ,
                                                                   GaborBounds bd, int real_spec, float2* __restrict__ H,
                                                                   float* __restrict__ Gz, int* __restrict__ col_of,
                                                                   float* __restrict__ lone, unsigned* __restrict__ stamps,
                                                                   int hop, int T) {
    __shared__ float2 s_twl[32 * 64];
    __shared__ float2 s_twh[64];
    __shared__ float s_scr[32 * 65];
    __shared__ float2 s_taps[kFftN / 2 + 64];            // conj(w_f), K <= N/2 + 1
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int f = blockIdx.x;
    // stamps != NULL (the table cache; grid (F, 1) only): validate or build, role 0
    unsigned* slot = stamps ? stamps + (size_t)f * kStampWords : nullptr;
    unsigned word = 0u;
    if (slot) {
        StampKey key{};
        key.kind = 1; key.F = F; key.K = K; key.hop = hop; key.T = T; key.cross = real_spec;
        if (tid < kStampWords) word = stamp_word(tid, key, kernel, pool_w, f);
        if (stamp_check(slot, word, tid)) return;
    }
    // blockIdx.y (backward tables, real-spectrum form only): 0 the taps w, 1 d w/d mu = i t w, 2 d w/d sigma =
    // (t^2/s^3 - 1/s) w (impulse_responses.py:5-16 differentiated; both stay Hermitian, so their spectra are real too)
    const int which = blockIdx.y;
    fft_prep_front(kernel, pool_w, F, K, GZ, bd, Gz, f, which, s_twl, s_twh, s_taps, nullptr, tid);
    __syncthreads();
    if (wave == 0) fft_prep_transform(F, K, real_spec, H, col_of, lone, f, which, s_twl, s_twh, s_scr, s_taps, nullptr, lane);
    if (slot) stamp_publish(slot, word, tid);
}

#include "leaf_band_phi.inc"
static_assert(kBandPhiLh == kBandLh, "leaf_band_phi.inc was generated for another filter length");

// sum over a 16-lane row (every lane of the row gets it)
__device__ __forceinline__ float band_row_sum(float v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x124, 0xf, 0xf, false));   // row_ror:4
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));   // row_ror:8
    return v;
}

// fft_prep_kernel (real-spectrum form, forward tables) + the tables of the band tasks.  Grid (F, 2 + n_edge):
//   workgroup (f, 0): the tables of fft_prep_kernel (wave 0 runs the filter's 2048-point transform), then all waves take the
//                     seven sums of the class decision from the spectrum wave 0 left in LDS;
//   workgroup (f, 1 + s): the edge table of edge entry s, both classes   } on CUs the F transform workgroups leave idle,
//   workgroup (f, 1 + n_edge): the decimated pooling windows G~ of both classes } and done before wave 0's transform is
// Sixteen lanes per table entry: the sum over the window samples within lphi of the entry's position.
// (Workgroup (0, 0) also copies the edge list to device memory for the main kernel.)
__device__ __forceinline__ void fft_prep_band_body(const float* __restrict__ kernel, const float* __restrict__ pool_w,
                                                   int F, int K, int GZ, const GaborBounds& bd, float2* __restrict__ H,
                                                   float* __restrict__ Gz, int* __restrict__ col_of, const BandTabArgs& a) {
    __shared__ float2 s_twl[32 * 64];
    __shared__ float2 s_twh[64];
    __shared__ float2 s_twp[64];
    __shared__ float s_scr[32 * 65];
    __shared__ float2 s_taps[kFftN / 2 + 64];
    __shared__ float Rs[kFftN];
    __shared__ float gs[64 * kPoolRowsMax];
    __shared__ float phis[2][kBandLh * 8 + 1];               // phi_8 | phi_4 (one half each)
    __shared__ float red[8][14];
    __shared__ int es[kBandMaxEdge][4];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, f = blockIdx.x;
    const int l16 = lane & 15;
    // one table entry per 16-lane row: value = sum over pp = lo .. hi of gs[pp + goff] phi[|p0 - pp|]
    auto entry = [&](const float* phi, int p0, int lo, int hi, int goff, const float* win) {
        float acc = 0.0f;
#pragma unroll 4
        for (int pp = lo + l16; pp <= hi; pp += 16) {
            const int u = p0 - pp;
            acc = fmaf(win[pp + goff], phi[u < 0 ? -u : u], acc);
        }
        return band_row_sum(acc);
    };
    float* gs2 = gs + 64 * kPoolRowsMax / 2;                              // (backward tables) g_f[j] (j - c)^2; K <= 640 here
    // both windows in one pass (the backward's tables: the same taps, the same phi)
    auto entry2 = [&](const float* phi, int p0, int lo, int hi, int goff, float& v2) {
        float acc = 0.0f, acc2 = 0.0f;
#pragma unroll 4
        for (int pp = lo + l16; pp <= hi; pp += 16) {
            const int u = p0 - pp;
            const float ph = phi[u < 0 ? -u : u];
            acc = fmaf(gs[pp + goff], ph, acc);
            acc2 = fmaf(gs2[pp + goff], ph, acc2);
        }
        v2 = band_row_sum(acc2);
        return band_row_sum(acc);
    };
    if (tid <= kBandLh * 8) phis[0][tid] = kBandPhi8[tid];
    else if (tid >= 128 && tid - 128 <= kBandLh * 4) phis[1][tid - 128] = kBandPhi4[tid - 128];
#pragma unroll
    for (int s = 0; s < kBandMaxEdge; ++s)
        if (tid == 256 + s) { es[s][0] = a.e[s].c; es[s][1] = a.e[s].m; es[s][2] = a.e[s].lo; es[s][3] = a.e[s].hi; }
    if (a.bwd_slabs && (int)blockIdx.y >= 2 + a.n_edge) {
        // ---- (backward) the spectrum of d w / d mu or d w / d sigma: fft_prep_kernel's workgroup (f, which)
        const int which = (int)blockIdx.y - (1 + a.n_edge);
        fft_prep_front(kernel, pool_w, F, K, GZ, bd, Gz, f, which, s_twl, s_twh, s_taps, nullptr, tid);
        __syncthreads();
        if (wave == 0) fft_prep_transform(F, K, 1, H, col_of, nullptr, f, which, s_twl, s_twh, s_scr, s_taps, nullptr, lane);
        return;
    }
    if ((LEAF_PREP_ABLATE & 1) && blockIdx.y > 0 && (int)blockIdx.y < 1 + a.n_edge) return;
    if ((LEAF_PREP_ABLATE & 2) && (int)blockIdx.y == 1 + a.n_edge) return;
    if (blockIdx.y > 0 || a.edge_only) {
        // ---- edge table W~[m] of entry s, both classes, in the register order of the class (band_task: the lane reads entry
        // k LPF + l2 of its register k): the window's samples [pa, pb) relative to the block, and the image of m D within lphi of them
        const float half = 0.5f * (float)(K - 1);
        for (int j = tid; j < K; j += kPrepWaves * 64) {                   // the pooling window: as fft_prep_front evaluates it, or
            if (a.edge_only) {                                             // (frozen-parameter tables) as it left it in the pooling row
                gs[j] = Gz[(size_t)f * GZ + kGPad + j];
            } else {
                const float q = ((float)j - half) / (pool_sigma(pool_w[f], K) * half);
                gs[j] = expf(-0.5f * (q * q));
            }
            const float tj = (float)j - half;
            gs2[j] = gs[j] * (tj * tj);
        }
        __syncthreads();
        const int grp = tid >> 4;
        if (!a.edge_only && (int)blockIdx.y == 1 + a.n_edge) {
            // ---- decimated pooling windows G~(tau) = D sum_u g[tau - u] phi_D[|u|], tau = c0min + D j, of both classes
            const int len16 = band_gz_len(K, a.hop, 16), len32 = band_gz_len(K, a.hop, 32);
            const int gzs = band_gz_floats(K, a.hop);                       // (run-time gcd loops: evaluated ONCE, not per table entry)
            float* gzf = a.gz + (size_t)f * gzs;
            float* gz2f = a.gz2 ? a.gz2 + (size_t)f * gzs : nullptr;
#pragma unroll
            for (int cls = 0; cls < 2; ++cls) {
                const int A = 16 << cls, D = band_d(A), lphi = band_lphi(A), c0 = band_c0min(K, a.hop, A), len = cls ? len32 : len16;
                for (int j = grp; j < len; j += kPrepWaves * 4) {
                    const int tau = c0 + D * j;
                    if (a.gz2) {
                        float v2;
                        const float v = entry2(phis[cls], tau, max(0, tau - lphi), min(K - 1, tau + lphi), 0, v2);
                        if (l16 == 0) {
                            gzf[(cls ? len16 : 0) + j] = (float)D * v;
                            gz2f[(cls ? len16 : 0) + j] = (float)D * v2;
                        }
                    } else {
                        const float v = entry(phis[cls], tau, max(0, tau - lphi), min(K - 1, tau + lphi), 0, gs);
                        if (l16 == 0) gzf[(cls ? len16 : 0) + j] = (float)D * v;
                    }
                }
            }
            return;
        }
        const int s = a.edge_only ? blockIdx.y : blockIdx.y - 1;
        if (f == 0 && s == 0 && tid < 4 * kBandMaxEdge) a.elist[tid] = es[tid >> 2][tid & 3];   // (edge_only: nobody else does)
        const int c = es[s][0], goff = c * a.L - (es[s][1] * a.hop - a.padL);
        const int pa = es[s][2] - c * a.L, pb = es[s][3] - c * a.L;
#pragma unroll
        for (int cls = 0; cls < 2; ++cls) {
            const int A = 16 << cls, D = band_d(A), lphi = band_lphi(A), M = band_m(A);
            float* tab = a.edge + (((size_t)f * 2 + cls) * kBandMaxEdge + s) * 512;
            for (int m = grp; m < M; m += kPrepWaves * 4) {
                int p0 = m * D;
                if (p0 - kFftN + lphi >= pa) p0 -= kFftN;
                else if (p0 + kFftN - lphi < pb) p0 += kFftN;
                const int m1 = m >> 4, m2 = m & 15;
                const int idx = cls ? brev5(m1) * 16 + m2 : (16 * (m2 >> 3) + brev4(m1)) * 8 + (m2 & 7);
                if (a.edge2) {
                    float v2;
                    const float v = entry2(phis[cls], p0, max(pa, p0 - lphi), min(pb - 1, p0 + lphi), goff, v2);
                    if (l16 == 0) { tab[idx] = (float)D * v; a.edge2[(tab - a.edge) + idx] = (float)D * v2; }
                } else {
                    const float v = entry(phis[cls], p0, max(pa, p0 - lphi), min(pb - 1, p0 + lphi), goff, gs);
                    if (l16 == 0) tab[idx] = (float)D * v;
                }
            }
        }
        return;
    }
    fft_prep_front(kernel, pool_w, F, K, GZ, bd, Gz, f, 0, s_twl, s_twh, s_taps, gs, tid);
    if (a.spec0 && tid < 64) {                                             // the half-wave twiddles in fft2048w's layout (fft_build_twiddles_wg)
        const int h = tid >> 5, e = tid & 31, j = (e >> 1) + 16 * (e & 1);
        float sn, cs;
        sincospif(2.0f * (float)j / 64.0f, &sn, &cs);
        s_twp[tid] = h ? make_float2(cs, -sn) : make_float2(1.0f, 0.0f);
    }
    __syncthreads();
    if (a.elist && f == 0 && tid >= 64 && tid < 64 + 4 * kBandMaxEdge) a.elist[tid - 64] = es[(tid - 64) >> 2][(tid - 64) & 3];
    if (wave == 0) fft_prep_transform(F, K, 1, H, col_of, nullptr, f, 0, s_twl, s_twh, s_scr, s_taps, Rs, lane);
    else if (a.spec0 && !(LEAF_PREP_ABLATE & 8)) {
        // ---- first blocks of the main kernel's workgroups, with the main kernel's own transform (fft2048w: the bits it would
        // compute itself; s_twl is the table both transforms share)
        extern __shared__ __attribute__((aligned(16))) float dyn_scr[];
        float* scr = dyn_scr + (size_t)(wave - 1) * kWgScrFloats;
        const unsigned scr_lds = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) float*)scr);
        const OwnedClips deal{a.B * a.nblk, a.G, a.nblk};
        for (int w = f * (kPrepWaves - 1) + wave - 1; w < a.G; w += F * (kPrepWaves - 1)) {
            if (deal.count(w) <= 0) continue;
            const int gb = deal.start(w), b = gb / a.nblk, c = gb - b * a.nblk, n_c = c * a.L;
            const float* xb = static_cast<const float*>(a.x) + (size_t)b * a.T;
            const unsigned short* xh = static_cast<const unsigned short*>(a.x) + (size_t)b * a.T;
            float are[32], aim[32];
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int i = 64 * r + lane;                              // block rotated left by padL samples (leaf_fft_wg_kernel)
                const int n = n_c - a.padL + ((i + a.padL) & (kFftN - 1));
                const int nc = min(max(n, 0), a.T - 1);
                const float v = a.io_bf16 ? __uint_as_float((unsigned)xh[nc] << 16) : xb[nc];
                are[r] = (n >= 0 && n < a.T) ? v : 0.0f;
                aim[r] = 0.0f;
            }
            fft2048w<false, false>(are, aim, scr, scr_lds, s_twl, s_twp, lane);
            float2* dst = a.spec0 + (size_t)w * kWgRingFwdFloat2;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int k = brev5(i);
                if (k < kWgFwdBins / 64) dst[64 * k + lane] = make_float2(are[i], aim[i]);   // bins 0..1151 (kWgFwdBins)
            }
        }
    }
    __syncthreads();
    if (LEAF_PREP_ABLATE & 4) return;
    // ---- the seven sums of the decision
    const float mu = fminf(fmaxf(kernel[2 * f], 0.0f), 3.14159274101257324f);
    const int k0 = (int)rintf(mu * (float)(kFftN / 6.283185307179586));
    float sums[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};   // tot | out2, ac(M/2), ac(3M/4) of class 1 | of class 2
    float dcs = 0.0f, mxdc = 0.0f;                                 // what every window drops at DC: bins 0, -1 .. -63 are entries 0 .. 63 (kBandAdjacentDC)
    float pmir[2] = {0.0f, 0.0f};                                  // mirrored pairs |R_k R_(2048-k)| inside a window that crosses Nyquist, 2 (k - 1024) >= 5 M / 16
    float mxo[2] = {0.0f, 0.0f};                                   // the largest dropped R^2 per class (round 6: the bias bound)
    int kbv[2];
#pragma unroll
    for (int cls = 0; cls < 2; ++cls) {
        const int M = 256 << cls;
        // bins kb .. kb + M - 1, centred on the filter.  Backward launches and LEAF_ALGO_STRICT_BAND_CLASSES keep the window inside the half
        // spectrum 1..1024 (a.cross = 0); the forward's ring holds bins 0..1151 (kWgFwdBins), so its windows may cross Nyquist -- a filter whose pass band
        // reaches beyond pi (the top one or two of the default mel bank) is then centred in its window instead of cut by it (round 6)
        const int kb = min(max(k0 - M / 2, 1), (a.cross ? kWgFwdBins : kFftN / 2 + 1) - M);
        kbv[cls] = kb;
        const int rlo = kFftN - kb - M + 1;                                // ... are entries rlo .. rlo + M - 1 of R (descending bins)
#pragma unroll
        for (int i0 = 0; i0 < kFftN; i0 += kPrepWaves * 64) {
            const int i = i0 + tid;
            const float v = Rs[i];
            if (cls == 0) {
                sums[0] += v * v;
                dcs += i < 64 ? v * v : 0.0f;
                mxdc = fmaxf(mxdc, i < 64 ? v * v : 0.0f);
            }
            const int j = i - rlo;
            const bool in = j >= 0 && j < M;
            sums[1 + 3 * cls] += in ? 0.0f : v * v;
            mxo[cls] = fmaxf(mxo[cls], in ? 0.0f : v * v);
            sums[2 + 3 * cls] += in && j + M / 2 < M ? v * Rs[min(i + M / 2, kFftN - 1)] : 0.0f;
            sums[3 + 3 * cls] += in && j + 3 * M / 4 < M ? v * Rs[min(i + 3 * M / 4, kFftN - 1)] : 0.0f;
            // entry i is bin 2048 - i: above Nyquist for i < 1024, its mirror image (bin i) is entry 2048 - i
            const int jm = kFftN - i - rlo;
            pmir[cls] += in && i < kFftN / 2 && kFftN / 2 - i >= 5 * M / 32 && jm >= 0 && jm < M ? fabsf(v * Rs[(kFftN - i) & (kFftN - 1)]) : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float w = wave_sum(sums[k]);
        if (lane == 0) red[wave][k] = w;
    }
#pragma unroll
    for (int cls = 0; cls < 2; ++cls) {
        const float w = wave_sum(pmir[cls]);
        if (lane == 0) red[wave][10 + cls] = w;
    }
    {
        const float w = wave_sum(dcs);
        float m = mxdc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) { red[wave][12] = w; red[wave][13] = m; }
    }
#pragma unroll
    for (int cls = 0; cls < 2; ++cls) {
        float m = mxo[cls];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (lane == 0) red[wave][8 + cls] = m;
    }
    __syncthreads();
    if (tid == 0) {
        int flags = 0, need = 0;
#pragma unroll
        for (int cls = 0; cls < 2; ++cls) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int col = k == 0 ? 0 : k + 3 * cls;
                float s = 0.0f;
#pragma unroll
                for (int w = 0; w < kPrepWaves; ++w) s += red[w][col];
                v[k] = s;
            }
            float pm = 0.0f;
#pragma unroll
            for (int w = 0; w < kPrepWaves; ++w) pm += red[w][10 + cls];
            float odc = 0.0f, mdc = 0.0f;
#pragma unroll
            for (int w = 0; w < kPrepWaves; ++w) { odc += red[w][12]; mdc = fmaxf(mdc, red[w][13]); }
            // (the bias-free energy bound counts what is dropped at DC kBandAdjacentDC / kBandAdjacent times too; not under round 5's rule, a.eta = kBandEta)
            const float o2 = a.eta < kBandEta ? v[1] + (kBandAdjacentDC / kBandAdjacent - 1.0f) * odc : v[1];
            bool ok = o2 <= a.eps2 * v[0] && v[2] <= a.eta * v[0] && v[3] <= a.eta * v[0] && pm <= a.eta * v[0];
            // the smallest bias that admits the class beyond the strict rule (band_need): the filter's core is 2 sigma_k around the centre bin
            const int Mc = 256 << cls;
            const float sgc = fminf(fmaxf(kernel[2 * f + 1], bd.sigma_lo), bd.sigma_hi), sk = (float)kFftN / (6.2831853f * sgc);
            const float dmin = (float)min(k0 - (kbv[cls] - 1), kbv[cls] + Mc - k0) - 2.0f * sk;
            const float spw = pool_sigma(pool_w[f], K);
            float mx = 0.0f;
#pragma unroll
            for (int w = 0; w < kPrepWaves; ++w) mx = fmaxf(mx, red[w][8 + cls]);
            int nd = band_need(v[1], mx, v[2], v[3], v[0], a.eta, fabsf(Rs[(kFftN - k0) & (kFftN - 1)]),
                               band_pool_gamma(spw, K, dmin, kFftN), spw, K, kFftN, pm, Mc, odc, mdc);
            if (a.bwd_slabs && !band_deriv_fits(k0, kbv[cls], Mc, sk)) { ok = false; nd = kBandNever; }   // (backward: see kBandDerivCore)
            if (a.force) { ok = a.force == cls + 1; nd = kBandNever; }
            flags |= ok ? 1 << cls : 0;
            need |= nd << (16 * cls);
        }
        if (a.classes) {
            const bool c1 = (flags & 1) || band_bias_admits(a.cls_bias, f, true, need), c2 = (flags & 2) || band_bias_admits(a.cls_bias, f, true, need >> 16);
            a.classes[f] = c1 ? 256 : c2 ? 512 : kFftN;
        }
        a.rec[4 * f] = flags;
        a.rec[4 * f + 1] = kbv[0];
        a.rec[4 * f + 2] = kbv[1];
        a.rec[4 * f + 3] = need;          // bmin(256) | bmin(512) << 16, fp16 codes
    }
}
// a.stamps != NULL (the table cache, leaf_forward_cached_f32; forward launches with grid (F, 2 + n_edge) only): every workgroup
// validates its stamp (leaf_fft.hpp) and returns, or builds what it builds without one and stamps it
__global__ __launch_bounds__(kPrepWaves * 64) void fft_prep_band_kernel(const float* __restrict__ kernel, const float* __restrict__ pool_w,
                                                                        int F, int K, int GZ, GaborBounds bd, float2* __restrict__ H,
                                                                        float* __restrict__ Gz, int* __restrict__ col_of, const BandTabArgs a) {
    const int tid = threadIdx.x, f = blockIdx.x, y = blockIdx.y;
    unsigned* slot = nullptr;
    unsigned word = 0u;
    if (a.stamps) {
        // role 0: workgroup (f, 0); role 1: the decimated pooling windows (f, 1 + n_edge); role 2 + s: the edge table (f, 1 + s)
        const int s = y - 1, role = y == 0 ? 0 : y == 1 + a.n_edge ? 1 : 2 + s;
        StampKey key{};
        key.kind = 2; key.F = F; key.K = K; key.hop = a.hop; key.T = a.T; key.role = role; key.n_edge = a.n_edge;
#pragma unroll
        for (int i = 0; i < kBandMaxEdge; ++i)
            if (role == 2 + i) { key.e[0] = a.e[i].c; key.e[1] = a.e[i].m; key.e[2] = a.e[i].lo; key.e[3] = a.e[i].hi; }
        key.eps2 = a.eps2; key.eta = a.eta; key.cross = a.cross; key.force = a.force; key.strict = a.strict;
        slot = a.stamps + ((size_t)role * F + f) * kStampWords;
        if (tid < kStampWords) word = stamp_word(tid, key, kernel, pool_w, f);
        if (stamp_check(slot, word, tid)) return;
    }
    fft_prep_band_body(kernel, pool_w, F, K, GZ, bd, H, Gz, col_of, a);
    if (slot) stamp_publish(slot, word, tid);
}

// ---- tables: one workgroup per filter.  z = conj(taps) in zero-phase layout over 4096 points; its spectrum through two
// 2048-point transforms (even / odd samples) and the decimation-in-time butterfly; real by the Hermitian symmetry of the
// taps about the centre (impulse_responses.py:5-16), 1 / 4096 folded in.
__global__ __launch_bounds__(kPrepWaves * 64) void fft4k_prep_kernel(const float* __restrict__ kernel, const float* __restrict__ pool_w,
                                                                     int F, int K, GaborBounds bd, float* __restrict__ tab,
                                                                     float* __restrict__ Grow, int RG, float2* __restrict__ Wt = nullptr,
                                                                     const BandTabArgs a = BandTabArgs{}) {
    __shared__ float2 s_twl[32 * 64];
    __shared__ float2 s_twh[64];
    __shared__ float s_scr[32 * 65];
    __shared__ float2 s_taps[2048 + 64];                                  // conj(w_f), K <= 2049; afterwards the spectrum R[4096] (band decision)
    __shared__ float red[kPrepWaves][7];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int f = blockIdx.x;
    // blockIdx.y (backward tables): 0 the taps w, 1 d w / d mu = i t w, 2 d w / d sigma = (t^2 / s^3 - 1 / s) w -- as
    // fft_prep_kernel; slab `which` of the table holds their spectra (the D tables matter for the taps only)
    const int which = blockIdx.y;
    tab += (size_t)which * F * kFft4TabFloats;
    const float mu = kernel[2 * f], sg = kernel[2 * f + 1];
    const float sgc = fminf(fmaxf(sg, bd.sigma_lo), bd.sigma_hi);
    for (int j = tid; j < K; j += kPrepWaves * 64) {
        float a_, b_;
        const float t = (float)(j - K / 2);
        gabor_tap(mu, sg, bd, t, a_, b_);
        if (which == 1) {
            const float a0 = a_;
            a_ = -t * b_;
            b_ = t * a0;
        } else if (which == 2) {
            const float c = t * t / (sgc * sgc * sgc) - 1.0f / sgc;
            a_ *= c;
            b_ *= c;
        }
        s_taps[j] = make_float2(a_, -b_);
    }
    if (which == 0) {   // de-interleaved pooling rows: Ge[64 + i] = g[2 i], Go[64 + i] = g[2 i + 1]  (impulse_responses.py:74-80)
        const float half = 0.5f * (float)(K - 1);
        const float sp = pool_sigma(pool_w[f], K);
        for (int jj = tid; jj < 2 * RG; jj += kPrepWaves * 64) {             // RG floats per parity row (kWg4RowFloats for K = 801)
            const int h = jj / RG, i = jj - h * RG - kGPad, j = 2 * i + h;
            float v = 0.0f;
            if (i >= 0 && j < K) {
                const float q = ((float)j - half) / (sp * half);
                v = expf(-0.5f * (q * q));
            }
            Grow[(size_t)f * 2 * RG + jj] = v;
        }
    }
    if (which == 0 && f == 0 && Wt) {                                     // w^e, e < 2048: shared by every filter (round 4)
        for (int e = tid; e < 2048; e += kPrepWaves * 64) {
            float sn, cs;
            sincospif(2.0f * (float)e / (float)kFft4N, &sn, &cs);          // the expression the D tables are built from, below
            Wt[e] = make_float2(cs, -sn);
        }
    }
    fft_build_twiddles(s_twl, s_twh, tid, kPrepWaves * 64);
    __syncthreads();
    // band-limited filter tasks of the static forward kernel (leaf_band.hpp): the class decision is taken here, from the spectrum
    const bool decide = which == 0 && a.rec != nullptr;                   // (uniform over the workgroup)
    if (wave != 0 && !decide) return;
    float* Rs = reinterpret_cast<float*>(s_taps);                         // [4096]: entry i <-> R[i] (the filter lives at entries 4096 - bin)
    if (wave == 0) {
        auto tap_at = [&](int i) {                                        // zero-phase layout: index i <-> t = i (i < 2048) or i - 4096
            const int j = (i < kFft4N / 2 ? i : i - kFft4N) + K / 2;
            return (j >= 0 && j < K) ? s_taps[j] : make_float2(0.0f, 0.0f);
        };
        // the even samples' transform first, then the odd ones' (round 5: both sets loaded up front were 128 live registers next
        // to a transform's temporaries -- 244 B of scratch per lane)
        float ere[32], eim[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const float2 te = tap_at(2 * (64 * r + lane));
            ere[r] = te.x; eim[r] = te.y;
        }
        fft2048(ere, eim, s_scr, s_twl, s_twh, lane);
        asm volatile("" : "+v"(ere[0]), "+v"(ere[31]) : : "memory");        // (the odd samples are read after it)
        float ore[32], oim[32];
#pragma unroll
        for (int r = 0; r < 32; ++r) {
            const float2 to = tap_at(2 * (64 * r + lane) + 1);
            ore[r] = to.x; oim[r] = to.y;
        }
        fft2048(ore, oim, s_scr, s_twl, s_twh, lane);
        // slab layout (kFft4TabFloats floats per filter): R2[2048] float2 = (R_lo[e], R_hi[e]) | D4[2048] float4 = (D_lo[e], D_hi[e]):
        // the values a bin needs together sit together, one 8- / 16-byte load per bin instead of two (round 4: a load instruction
        // costs these kernels more than four VALU instructions)
        float2* R2 = reinterpret_cast<float2*>(tab + (size_t)f * kFft4TabFloats);
        float4* D4 = reinterpret_cast<float4*>(tab + (size_t)f * kFft4TabFloats + 4096);
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int e = 64 * brev5(i) + lane;
            float s, c;
            sincospif(2.0f * (float)e / (float)kFft4N, &s, &c);              // w^e = (c, -s)
            const float tr = ore[i] * c + oim[i] * s;                         // Re(w^e Xo[e])
            const float rlo = (ere[i] + tr) * (1.0f / kFft4N), rhi = (ere[i] - tr) * (1.0f / kFft4N);
            if (which == 0) {
                R2[e] = make_float2(rlo, rhi);
                D4[e] = make_float4(rlo * c, -rlo * s, rhi * c, -rhi * s);
                if (decide) { Rs[e] = rlo; Rs[e + 2048] = rhi; }          // (this wave was the taps' only reader)
            } else {
                // the derivative tables' D slots carry (d/dmu lo, d/dmu hi, d/dsigma lo, d/dsigma hi) of bin e as ONE 16-byte entry
                // (in the mu slab: which = 1 writes the first half of each entry, which = 2 the second): the backward's dot products
                // take one load per bin and half instead of four (-1.4 .. -2.1 % of the backward: profiles/r04/ab_table_addressing.txt)
                float2* ms = reinterpret_cast<float2*>(tab - (size_t)(which - 1) * F * kFft4TabFloats + (size_t)f * kFft4TabFloats + 4096);
                ms[2 * e + (which - 1)] = make_float2(rlo, rhi);
            }
        }
    }
    if (!decide) return;
    __syncthreads();
    // ---- class decision (leaf_band.hpp; one class here: a 512-bin window of the 4096-point spectrum, decimation 8): the window
    // [kb, kb + 512) around the centre bin inside bins 1..2048 are entries rlo .. rlo + 511 of R (descending bins)
    constexpr int M = 512;
    const float muc = fminf(fmaxf(mu, 0.0f), 3.14159274101257324f);
    const int k0 = (int)rintf(muc * (float)(kFft4N / 6.283185307179586));
    const int kb = min(max(k0 - M / 2, 1), kFft4N / 2 + 1 - M);
    const int rlo = kFft4N - kb - M + 1;
    float sums[4] = {0.0f, 0.0f, 0.0f, 0.0f};                            // total | outside the window | |autocorrelation| at M/2, 3M/4
    float mxo = 0.0f;                                                    // the largest dropped R^2 (round 6: the bias bound, leaf_band.hpp)
    float dcs = 0.0f, mxdc = 0.0f;                                       // ... and what is dropped at DC: bins 0, -1 .. -63 = entries 0 .. 63 (kBandAdjacentDC)
#pragma unroll
    for (int i0 = 0; i0 < kFft4N; i0 += kPrepWaves * 64) {
        const int i = i0 + tid;
        const float v = Rs[i];
        const int j = i - rlo;
        const bool in = j >= 0 && j < M;
        sums[0] += v * v;
        sums[1] += in ? 0.0f : v * v;
        mxo = fmaxf(mxo, in ? 0.0f : v * v);
        dcs += i < 64 ? v * v : 0.0f;
        mxdc = fmaxf(mxdc, i < 64 ? v * v : 0.0f);
        sums[2] += in && j + M / 2 < M ? fabsf(v * Rs[min(i + M / 2, kFft4N - 1)]) : 0.0f;
        sums[3] += in && j + 3 * M / 4 < M ? fabsf(v * Rs[min(i + 3 * M / 4, kFft4N - 1)]) : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w = wave_sum(sums[k]);
        if (lane == 0) red[wave][k] = w;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mxo = fmaxf(mxo, __shfl_xor(mxo, o));
    if (lane == 0) red[wave][4] = mxo;
    {
        const float w = wave_sum(dcs);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mxdc = fmaxf(mxdc, __shfl_xor(mxdc, o));
        if (lane == 0) { red[wave][5] = w; red[wave][6] = mxdc; }
    }
    __syncthreads();
    if (tid == 0) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < kPrepWaves; ++w) s += red[w][k];
            v[k] = s;
        }
        float odc = 0.0f, mdc = 0.0f;
#pragma unroll
        for (int w = 0; w < kPrepWaves; ++w) { odc += red[w][5]; mdc = fmaxf(mdc, red[w][6]); }
        const float o2 = a.eta < kBandEta ? v[1] + (kBandAdjacentDC / kBandAdjacent - 1.0f) * odc : v[1];   // (leaf_band.hpp: what is dropped at DC)
        bool ok = o2 <= a.eps2 * v[0] && v[2] <= a.eta * v[0] && v[3] <= a.eta * v[0];
        // the smallest bias that admits the class beyond the strict rule (leaf_band.hpp: band_need, band_pool_gamma)
        const float sk = (float)kFft4N / (6.2831853f * sgc), spw = pool_sigma(pool_w[f], K);
        const float dmin = (float)min(k0 - (kb - 1), kb + M - k0) - 2.0f * sk;
        float mx = 0.0f;
#pragma unroll
        for (int w = 0; w < kPrepWaves; ++w) mx = fmaxf(mx, red[w][4]);
        int nd = band_need(v[1], mx, v[2], v[3], v[0], a.eta, fabsf(Rs[(kFft4N - k0) & (kFft4N - 1)]),
                           band_pool_gamma(spw, K, dmin, kFft4N), spw, K, kFft4N, 0.0f, M, odc, mdc);
        if (a.bwd_slabs && !band_deriv_fits(k0, kb, M, sk)) { ok = false; nd = kBandNever; }          // (backward: leaf_band.hpp, kBandDerivCore)
        if (a.force) { ok = a.force == 2; nd = kBandNever; }
        if (a.classes) a.classes[f] = (ok || band_bias_admits(a.cls_bias, f, true, nd)) ? M : kFft4N;
        a.rec[4 * f] = ok ? 2 : 0;                                        // (bit 1: the four-filters-per-task class of band_build_plan)
        a.rec[4 * f + 1] = kb;
        a.rec[4 * f + 2] = kb;
        a.rec[4 * f + 3] = kBandNever | (nd << 16);                       // bmin (fp16 codes): never the eight-per-task class | the 512-bin class
    }
}

// The tables of the band tasks on 4096-sample blocks (K = 801 / hop = 320; as the blockIdx.y > 0 workgroups of
// fft_prep_band_kernel, one class).  Grid (F, 1 + n_edge): workgroup (f, 0) the decimated pooling window G~(tau) =
// 8 sum_u g[tau - u] phi_8[|u|], tau = c0min + 8 j; workgroup (f, 1 + s) the dense table of edge entry s over the block's 512
// decimated samples, in the register order of the task (the lane reads entry 16 k + l2 of its register k).
__global__ __launch_bounds__(kPrepWaves * 64) void fft4k_band_tab_kernel(const float* __restrict__ pool_w, int F, int K, const BandTabArgs a) {
    __shared__ float gs[64 * kPoolRowsMax];
    __shared__ float gs2[64 * kPoolRowsMax];
    __shared__ float phis[kBandLh * 8 + 1];
    __shared__ int es[kBandMaxEdge][4];
    constexpr int D = 8, LPHI = kBandLh * D;
    const int tid = threadIdx.x, f = blockIdx.x, l16 = tid & 15, grp = tid >> 4;
    if (tid <= LPHI) phis[tid] = kBandPhi8[tid];
#pragma unroll
    for (int s = 0; s < kBandMaxEdge; ++s)
        if (tid == 256 + s) { es[s][0] = a.e[s].c; es[s][1] = a.e[s].m; es[s][2] = a.e[s].lo; es[s][3] = a.e[s].hi; }
    {
        const float half = 0.5f * (float)(K - 1), sp = pool_sigma(pool_w[f], K);
        for (int j = tid; j < K; j += kPrepWaves * 64) {                   // the pooling window, as fft4k_prep_kernel evaluates it
            const float q = ((float)j - half) / (sp * half);
            gs[j] = expf(-0.5f * (q * q));
            gs2[j] = gs[j] * (((float)j - half) * ((float)j - half));     // (backward tables: d pool_w, leaf_band_bwd.hpp)
        }
    }
    __syncthreads();
    auto entry = [&](int p0, int lo, int hi, int goff, const float* win) {   // sixteen lanes per table entry
        float acc = 0.0f;
#pragma unroll 4
        for (int pp = lo + l16; pp <= hi; pp += 16) {
            const int u = p0 - pp;
            acc = fmaf(win[pp + goff], phis[u < 0 ? -u : u], acc);
        }
        return band_row_sum(acc);
    };
    if (blockIdx.y == 0) {
        const int len = band_gz_len_d(K, a.hop, 32, D), c0 = band_c0min_d(K, a.hop, 32, D);
        const int gzs = band4k_gz_floats(K, a.hop);                        // (run-time gcd loops: once, not per entry)
        float* gzf = a.gz + (size_t)f * gzs;
        float* gz2f = a.gz2 ? a.gz2 + (size_t)f * gzs : nullptr;
        for (int j = grp; j < len; j += kPrepWaves * 4) {
            const int tau = c0 + D * j;
            const float v = entry(tau, max(0, tau - LPHI), min(K - 1, tau + LPHI), 0, gs);
            if (l16 == 0) gzf[j] = (float)D * v;
            if (a.gz2) {
                const float v2 = entry(tau, max(0, tau - LPHI), min(K - 1, tau + LPHI), 0, gs2);
                if (l16 == 0) gz2f[j] = (float)D * v2;
            }
        }
        if (f == 0 && tid < 4 * kBandMaxEdge) a.elist[tid] = es[tid >> 2][tid & 3];
        return;
    }
    const int s = blockIdx.y - 1;
    const int c = es[s][0], goff = c * a.L - (es[s][1] * a.hop - a.padL);
    const int pa = es[s][2] - c * a.L, pb = es[s][3] - c * a.L;
    float* tabe = a.edge + ((size_t)f * kBandMaxEdge + s) * 512;
    for (int m = grp; m < 512; m += kPrepWaves * 4) {
        int p0 = m * D;
        if (p0 - kFft4N + LPHI >= pa) p0 -= kFft4N;
        else if (p0 + kFft4N - LPHI < pb) p0 += kFft4N;
        const float v = entry(p0, max(pa, p0 - LPHI), min(pb - 1, p0 + LPHI), goff, gs);
        if (l16 == 0) tabe[brev5(m >> 4) * 16 + (m & 15)] = (float)D * v;
        if (a.edge2) {
            const float v2 = entry(p0, max(pa, p0 - LPHI), min(pb - 1, p0 + LPHI), goff, gs2);
            if (l16 == 0) a.edge2[(tabe - a.edge) + brev5(m >> 4) * 16 + (m & 15)] = (float)D * v2;
        }
    }
}

// identity filter -> column map for param_reduce_kernel (the 2048-sample tables get theirs from fft_prep_kernel)
__global__ void iota_kernel(int* __restrict__ v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}

}  // namespace
