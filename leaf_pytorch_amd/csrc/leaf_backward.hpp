// leaf_backward.hpp -- the tap-gradient MFMA GEMM of the direct-form backward (its arguments: DtapsParams, leaf_params.hpp)
// Included by every unit: templates, device functions, constexpr sizes (gfx950 only).  The backward's plain kernels -- staged
// transposes, PCEN / EMA reverse sweep, chain to (mu, sigma) -- are leaf_kernels_backward.hpp's and leaf_kernels_rows.hpp's.
#pragma once
#include "leaf_common.hpp"
#include "leaf_fused.hpp"

namespace {

// ---------------------------------------------------------------------------------------------
// fused backward, phase C: tap gradients as an fp32-MFMA GEMM.
//   dH[kk][c] = sum_{b,n} S_kk[b,n] * dY[b,n][c]   (c < FP, Re columns)      S_kk[n] = x[n+kk] + x[n-kk]
//   dH[kk][c] = sum_{b,n} D_kk[b,n] * dY[b,n][c]   (c >= FP, Im columns)     D_kk[n] = x[n+kk] - x[n-kk]
// i.e. the transpose of the forward GEMMs w.r.t. the tap table W, with the same Hermitian operands built from an
// LDS waveform window.  Rows = 16 tap rows per wave (one k-tile each), columns = the group's 16-filter tiles,
// reduction = time.  A workgroup walks 64-sample chunks (waveform window + dY tile double-buffered in LDS, next
// chunk prefetched into registers under the MFMAs) and finally writes its partial dH; a small kernel sums the
// partials and chains them to (mu, sigma).
// ---------------------------------------------------------------------------------------------

template <int RT, int NA, bool EVENK>
__device__ __forceinline__ void dtaps_ktile(f32x4 (&acc)[2 * RT], const float* xc, const float* sdy, int LD, int colre,
                                            int colim, int krow, int g, int Hf, int NS) {
    for (int nb = 0; nb < NS / 16; ++nb) {
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int rr = 16 * nb + 4 * s4 + g;
            float fw = xc[rr + krow];
            const float bw = xc[rr - krow];
            if (EVENK) fw = krow <= Hf ? fw : 0.0f;
            const float sv = fw + bw, dv = fw - bw;
            const float* row = sdy + rr * LD;
#pragma unroll
            for (int t = 0; t < NA; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv, row[colre + 16 * t], acc[t], 0, 0, 0);
                acc[RT + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv, row[colim + 16 * t], acc[RT + t], 0, 0, 0);
            }
        }
    }
}

constexpr int kDtPF = 4;      // float4 registers per thread for the dY tile prefetch
template <int RT, int TPW, bool EVENK>
__global__ __launch_bounds__(1024) void dtaps_mfma_kernel(const DtapsParams p) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int li = lane & 15, g = lane >> 4;
    const int tile_floats = p.NS * p.LD;
    const int buf_floats = (p.XSC + 3) / 4 * 4 + tile_floats;
    const int tile0 = p.tile_base + blockIdx.y * RT;
    const int colre = 16 * tile0 + li, colim = p.FP + 16 * tile0 + li;
    const int row4 = 2 * p.FP / 4;                       // float4 per dY row
    const int n4 = p.NS * row4;                          // float4 per dY tile

    // k-tile -> (wave, slot) assignment.  Column tiles are support-sorted, so low k-tiles carry more MFMAs (all column
    // tiles reach them) than high ones: a round-robin split leaves one SIMD with ~30 % more work.  Thread 0 does a
    // longest-processing-time greedy that balances the four SIMDs (waves w, w+4, .. share SIMD w & 3).
    __shared__ int s_kt[16 * 3];
    if (tid == 0) {
        int load[16], cnt[16], simd_load[4] = {0, 0, 0, 0};
        for (int w = 0; w < 16; ++w) load[w] = cnt[w] = 0;
        for (int i = 0; i < 16 * 3; ++i) s_kt[i] = -1;
        for (int kt = 0; kt < p.NKT; ++kt) {
            int work = 0;
            for (int t = 0; t < RT; ++t) work += (4 * p.tile_ks[tile0 + t] > 16 * kt) ? 1 : 0;
            if (work == 0) continue;
            int best = -1, best_key = 1 << 30;
            for (int w = 0; w < p.NW; ++w) {
                if (cnt[w] >= TPW) continue;
                const int key = simd_load[w & 3] * 64 + load[w];
                if (key < best_key) { best_key = key; best = w; }
            }
            s_kt[best * TPW + cnt[best]] = kt;
            cnt[best]++; load[best] += work; simd_load[best & 3] += work;
        }
    }
    __syncthreads();
    int na[TPW], ktile[TPW];                              // owned k-tiles and their active column tiles
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
        const int kt = __builtin_amdgcn_readfirstlane(s_kt[wave * TPW + tp]);
        ktile[tp] = kt;
        int n = 0;
        for (int t = 0; t < RT; ++t) n += (kt >= 0 && 4 * p.tile_ks[tile0 + t] > 16 * kt) ? 1 : 0;
        na[tp] = __builtin_amdgcn_readfirstlane(n);
    }
    f32x4 acc[TPW][2 * RT];
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp)
#pragma unroll
        for (int c = 0; c < 2 * RT; ++c) acc[tp][c] = f32x4{0.f, 0.f, 0.f, 0.f};

    f32x4 pre[kDtPF];
    float prex[2];
    auto load_chunk = [&](int chunk) {
        const int b = chunk / p.nch, n0 = (chunk - b * p.nch) * p.NS;
        const float* src = p.dY + ((size_t)b * p.T + n0) * (size_t)(2 * p.FP);
#pragma unroll
        for (int i = 0; i < kDtPF; ++i) {
            const int idx = tid + i * nthreads;
            pre[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < n4 && n0 + idx / row4 < p.T) pre[i] = *reinterpret_cast<const f32x4*>(src + (size_t)idx * 4);
        }
        const float* xb = p.x + (size_t)b * p.T;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * nthreads;
            const int n = n0 - p.HPc + p.xshift + idx;
            prex[i] = (idx < p.XSC && n >= 0 && n < p.T) ? xb[n] : 0.0f;
        }
    };
    auto store_chunk = [&](float* buf) {
        float* xw = buf;
        float* sdy = buf + (p.XSC + 3) / 4 * 4;
#pragma unroll
        for (int i = 0; i < kDtPF; ++i) {
            const int idx = tid + i * nthreads;
            if (idx < n4) {
                const int row = idx / row4, c4 = idx - row * row4;
                *reinterpret_cast<f32x4*>(sdy + row * p.LD + 4 * c4) = pre[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int idx = tid + i * nthreads;
            if (idx < p.XSC) xw[idx] = prex[i];
        }
    };

    int chunk = blockIdx.x;
    int cur = 0;
    if (chunk < p.total_chunks) {
        load_chunk(chunk);
        store_chunk(dsm);
    }
    __syncthreads();
    for (; chunk < p.total_chunks; chunk += gridDim.x) {
        const int next = chunk + gridDim.x;
        if (next < p.total_chunks) load_chunk(next);
        const float* buf = dsm + (size_t)cur * buf_floats;
        const float* xc = buf + p.HPc;
        const float* sdy = buf + (p.XSC + 3) / 4 * 4;
#pragma unroll
        for (int tp = 0; tp < TPW; ++tp) {
            const int krow = 16 * ktile[tp] + li;
            if (na[tp] == RT) dtaps_ktile<RT, RT, EVENK>(acc[tp], xc, sdy, p.LD, colre, colim, krow, g, p.Hf, p.NS);
            if constexpr (RT >= 2)
                if (na[tp] == RT - 1)
                    dtaps_ktile<RT, RT - 1, EVENK>(acc[tp], xc, sdy, p.LD, colre, colim, krow, g, p.Hf, p.NS);
            if constexpr (RT >= 3)
                if (na[tp] == RT - 2)
                    dtaps_ktile<RT, RT - 2, EVENK>(acc[tp], xc, sdy, p.LD, colre, colim, krow, g, p.Hf, p.NS);
        }
        if (next < p.total_chunks) store_chunk(dsm + (size_t)(cur ^ 1) * buf_floats);
        __syncthreads();
        cur ^= 1;
    }
    // partial dH of this workgroup: D layout row = 4g + r (tap row within the k-tile), col = li
    float* outp = p.dHpart + (size_t)blockIdx.x * (16 * p.NKT) * (2 * p.FP);
#pragma unroll
    for (int tp = 0; tp < TPW; ++tp) {
        const int kt = ktile[tp];
        if (kt < 0) continue;
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t rowoff = (size_t)(16 * kt + 4 * g + r) * (2 * p.FP);
                outp[rowoff + colre + 16 * t] = acc[tp][t][r];
                outp[rowoff + colim + 16 * t] = acc[tp][RT + t][r];
            }
    }
}

}  // namespace
