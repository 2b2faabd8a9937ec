// leaf_kernels_rows.hpp -- the row kernels: finalize (bias, floor, EMA, PCEN) of the direct-form path, the streaming PCEN step, the
// PCEN / EMA reverse sweeps of the backward and the per-filter parameter reduction
// Included by leaf_kernels.hip only: kernels (see leaf_kernels_tables.hpp).
#pragma once
#include "leaf_backward.hpp"
#include "leaf_fft.hpp"
#include "leaf_pcen_scan.hpp"

namespace {

// Sum the partials of every frame, add bias, floor (frontend.py:84), then the EMA recurrence and PCEN
// (postprocessing.py:13-28, 62-69).  One workgroup per (clip, group of kFinGroup filters), 128-frame chunks (a 1 s
// clip is one chunk):
//   phase 1  all threads: pooled[f][m] -> LDS (partial reads coalesced across filters)
//   phase 2  one wave per filter, lane l owns frames 2l and 2l+1: the first-order recurrence
//            M_m = w p_m + (1-w) M_{m-1} is an affine map composition -- composed in-lane for the pair, scanned
//            across the wavefront with 6 shuffle steps, with a carried state between chunks; PCEN is pointwise.
// mode bit0: PCEN, bit1: log1p (extension), bit2: bf16 output, bit3: raw (pre-floor) output, bit4: every slot valid
// Which of a frame's `noff` partial slots hold data: bit4 -> all; SlotGeom.L > 0 (overlap-save path: slot s = s-th
// block the frame's window meets) -> computed from the geometry, so the partial buffer needs no zero fill; otherwise
// (direct path) slot dd is valid when hop-block q = m + dd lies in [q_lo, q_hi].
__global__ __launch_bounds__(kFinThreads) void finalize_kernel(
    const float* __restrict__ part, int F, int FP, int TP, int noff, int q_lo, int q_hi, SlotGeom geo,
    const int* __restrict__ col_of, const float* __restrict__ bias, const float* __restrict__ alpha,
    const float* __restrict__ delta, const float* __restrict__ root, const float* __restrict__ ema_w, float floor_, int mode,
    void* __restrict__ out_, float* __restrict__ raw_out /* optional [B][F][TP]: bias + pooled sum before the floor */) {
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    float* out = static_cast<float*>(out_);
    unsigned short* outh = static_cast<unsigned short*>(out_);
    // blockIdx.y = filter group: filters [f_lo, f_lo + nf), normally one per wave
    const int per = (F + (int)gridDim.y - 1) / (int)gridDim.y;
    const int f_lo = blockIdx.y * per, nf = min(F - f_lo, per);
    if (nf <= 0) return;
    float* sv = fsm;                         // [nf][kFinStride] pooled values of the current chunk
    float* scarry = sv + per * kFinStride;   // [nf] EMA state carried across chunks
    float* s_dr = scarry + per;              // [nf] delta^(1/r)
    int* s_col = reinterpret_cast<int*>(s_dr + per);   // [nf] tap column of each filter
    const int b = blockIdx.x, tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid >> 6, lane = tid & 63;
    for (int fl = tid; fl < nf; fl += nthreads) {
        const int f = f_lo + fl;
        s_col[fl] = col_of[f];
        s_dr[fl] = (mode & 1) ? powf(delta[f], 1.0f / fmaxf(root[f], 1.0f)) : 0.0f;
    }
    __syncthreads();
    for (int m0 = 0; m0 < TP; m0 += kFinFrames) {
        const int nm = min(kFinFrames, TP - m0);
        for (int base = 0; base < nm * nf; base += nthreads * kFinPer) {
            float acc[kFinPer];
            int slot[kFinPer];
#pragma unroll
            for (int i = 0; i < kFinPer; ++i) {
                const int idx = base + i * nthreads + tid;
                acc[i] = 0.0f;
                slot[i] = -1;
                if (idx < nm * nf) {
                    const int mm = idx / nf, fl = idx - mm * nf, f = f_lo + fl;
                    const int m = m0 + mm;
                    const float* pp = part + (((size_t)b * TP + m) * noff) * FP + s_col[fl];
                    int nvalid = noff;
                    if (geo.L > 0) {
                        const int s0 = m * geo.hop - geo.padL;
                        nvalid = min(geo.T - 1, s0 + geo.K - 1) / geo.L - max(0, s0) / geo.L + 1;
                    }
                    for (int dd = 0; dd < noff; ++dd) {
                        const int q = m + dd;
                        const bool valid = geo.L > 0 ? dd < nvalid : ((mode & 16) || (q >= q_lo && q <= q_hi));
                        if (valid) acc[i] += pp[(size_t)dd * FP];
                    }
                    acc[i] += bias ? bias[f] : 0.0f;
                    slot[i] = fl * kFinStride + mm;
                }
            }
#pragma unroll
            for (int i = 0; i < kFinPer; ++i)
                if (slot[i] >= 0) {
                    sv[slot[i]] = (mode & 8) ? acc[i] : pooled_floor(acc[i]);
                    if (raw_out) {
                        const int fl = slot[i] / kFinStride, mm = slot[i] - fl * kFinStride;
                        raw_out[((size_t)b * F + f_lo + fl) * TP + m0 + mm] = acc[i];
                    }
                }
        }
        __syncthreads();
        for (int fl = wave; fl < nf; fl += nthreads / 64) {
            const int f = f_lo + fl;
            const int j0 = 2 * lane, j1 = j0 + 1;
            const float v0 = j0 < nm ? sv[fl * kFinStride + j0] : 0.0f;
            const float v1 = j1 < nm ? sv[fl * kFinStride + j1] : 0.0f;
            float r0 = v0, r1 = v1;
            if (mode & 8) {                              // backward: pre-floor pooled value
            } else if (mode & 1) {
                const float w = fminf(fmaxf(ema_w[f], 0.0f), 1.0f);
                const float A0 = j0 < nm ? 1.0f - w : 1.0f, B0 = j0 < nm ? w * v0 : 0.0f;   // M_m = A_m M_{m-1} + B_m
                const float A1 = j1 < nm ? 1.0f - w : 1.0f, B1 = j1 < nm ? w * v1 : 0.0f;
                float A = A1 * A0, Bv = fmaf(A1, B0, B1);    // the pair's map, then the inclusive scan over lanes
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float Ap = __shfl_up(A, off), Bp = __shfl_up(Bv, off);
                    if (lane >= off) {
                        Bv = fmaf(A, Bp, Bv);
                        A *= Ap;
                    }
                }
                const float carry = (m0 == 0) ? sv[fl * kFinStride] : scarry[fl];   // state starts at p_0 (postprocessing.py:15)
                const float Mend = fmaf(A, carry, Bv);       // state after this lane's second frame
                const float Mprev = __shfl_up(Mend, 1);
                const float M0 = fmaf(A0, lane ? Mprev : carry, B0);
                const float M1 = fmaf(A1, M0, B1);
                const float last = __shfl(((nm - 1) & 1) ? M1 : M0, (nm - 1) >> 1);
                if (lane == 0) scarry[fl] = last;
                const float a = fminf(alpha[f], 1.0f);
                const float inv_r = 1.0f / fmaxf(root[f], 1.0f);
                const float dl = delta[f];
                // q = p / (floor+M)^a with the hardware log2/exp2 (1 ulp each; floor+M is a normal number).  Then
                // (q+d)^(1/r) - d^(1/r) = d^(1/r) * expm1(log1p(q/d)/r) for d > 0: no cancelling subtraction, so quiet
                // frames keep full relative accuracy and the general powf (the bulk of this kernel's arithmetic) is only
                // needed for d <= 0, where the reference's own formula is followed literally (NaN/inf cases included).
                const float q0 = v0 * leaf_pow_pos(floor_ + M0, -a);
                const float q1 = v1 * leaf_pow_pos(floor_ + M1, -a);
                if (dl > 0.0f) {
                    const float inv_d = 1.0f / dl;
                    r0 = s_dr[fl] * leaf_expm1_pos(inv_r * leaf_log1p_pos(q0 * inv_d));
                    r1 = s_dr[fl] * leaf_expm1_pos(inv_r * leaf_log1p_pos(q1 * inv_d));
                } else {
                    r0 = powf(q0 + dl, inv_r) - s_dr[fl];
                    r1 = powf(q1 + dl, inv_r) - s_dr[fl];
                }
            } else if (mode & 2) {
                r0 = log1pf(v0);
                r1 = log1pf(v1);
            }
            const size_t o = ((size_t)b * F + f) * TP + m0 + j0;
            if (mode & 4) {                                  // bfloat16 features (the feature type, whatever x is): nearest even, torch's NaN
                if (j0 < nm) outh[o] = bf16_round(r0);
                if (j1 < nm) outh[o + 1] = bf16_round(r1);
            } else {
                if (j0 < nm) out[o] = r0;
                if (j1 < nm) out[o + 1] = r1;
            }
        }
        __syncthreads();
    }
}

// floor + optional log1p on an already pooled (B,F,T') tensor (staged path without PCEN)
__global__ void floor_kernel(const float* __restrict__ p, size_t n, int mode, float* __restrict__ out) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const float v = pooled_floor(p[idx]);
    out[idx] = (mode & 2) ? log1pf(v) : v;
}

// leaf_pcen_stream_f32: one lane per (stream, filter) row, the chunk's frames in order, smoother state in and out
__global__ void pcen_stream_kernel(const float* __restrict__ p, int BF, int n, FinParams q, const float* __restrict__ ema_in,
                                   float* __restrict__ ema_out) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= BF) return;
    const FinCoef c = fin_coef(q, row % q.F);
    const float* pr = p + (size_t)row * n;
    float M = ema_in ? ema_in[row] : pr[0];                     // a stream starts at its first frame (postprocessing.py:15)
    for (int m = 0; m < n; ++m) {
        const float v = pr[m];
        if (q.mode & 1) M = fin_ema_step(c, v, M);
        fin_store(q, (size_t)row * n + m, fin_point(c, q.mode, q.floor_, v, M));
    }
    if (ema_out && (q.mode & 1)) ema_out[row] = M;
}

// One lane per (b,f) row.  raw = pooled before the floor.  Forward EMA is recomputed into `ema`, then the
// reverse-time sweep produces g_pre (grad w.r.t. raw) and the row's contributions to d alpha, d delta, d root,
// d ema_w in rowsum[row][4].  mode bit0: PCEN on; bit1 (2): log1p compression behind the floor (PCEN off only: the forward's
// extension, out = log1p(max(raw, 1e-5)), so d out / d raw = 1 / (1 + raw) above the floor -- a division, not a reciprocal);
// bit2 (4): gout is bfloat16 (the feature type: LEAF_FLAG_OUT_BF16 or LEAF_FLAG_IO_BF16); bit4 (16): no pooled floor (the stand-alone PCENLayer backward).
__global__ void pcen_bwd_rows_kernel(const float* __restrict__ raw, const void* __restrict__ gout, int BF, int F, int TP,
                                     const float* __restrict__ alpha, const float* __restrict__ delta,
                                     const float* __restrict__ root, const float* __restrict__ ema_w, float floor_,
                                     int mode, float* __restrict__ ema, float* __restrict__ gpre,
                                     float* __restrict__ rowsum, const int* __restrict__ col_of, int FP,
                                     float* __restrict__ gcols) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= BF) return;
    const float* r = raw + (size_t)row * TP;
    const int gbf = (mode & 4) ? kSampleBf16 : kSampleF32;
    const size_t go0 = (size_t)row * TP;
    float* gp = gpre + (size_t)row * TP;
    const int f = row % F;
    // fused backward: also a [B][TP][FP] copy with filters in tap-column order
    float* gc = gcols ? gcols + (size_t)(row / F) * TP * FP + col_of[f] : nullptr;
    const bool nofloor = (mode & 16) != 0;          // stand-alone PCENLayer: no 1e-5 floor in front (frontend.py:84 is Leaf's)
    auto fl = [&](float v) { return nofloor ? v : fmaxf(v, kPooledFloor); };
    if (!(mode & 1)) {
        for (int m = 0; m < TP; ++m) {
            const float g = io_load(gout, go0 + m, gbf);
            const float v = (nofloor || r[m] > kPooledFloor) ? ((mode & 2) ? g / (1.0f + r[m]) : g) : 0.0f;
            gp[m] = v;
            if (gc) gc[(size_t)m * FP] = v;
        }
        return;
    }
    float* M = ema + (size_t)row * TP;
    const float w = fminf(fmaxf(ema_w[f], 0.0f), 1.0f), omw = 1.0f - w;
    const float a = fminf(alpha[f], 1.0f);
    const float reff = fmaxf(root[f], 1.0f), rho = 1.0f / reff;
    const float d = delta[f];
    const float d_rho = powf(d, rho), ln_d = logf(d);
    const bool fast = d > 1e-30f;                                         // the hardware log2 / exp2 forms (see below)
    float state = fl(r[0]);
    for (int m = 0; m < TP; ++m) {
        const float p = fl(r[m]);
        state = w * p + omw * state;
        M[m] = state;
    }
    float s_a = 0.f, s_d = 0.f, s_rho = 0.f, s_w = 0.f, gM_next = 0.f;
    const float p0 = fl(r[0]);
    for (int m = TP - 1; m >= 0; --m) {
        const float p = fl(r[m]);
        const float Mf = floor_ + M[m];
        const float u = powf(Mf, a);
        const float v = p / u + d;
        const float vr = powf(v, rho);
        const float g = io_load(gout, go0 + m, gbf);
        const float dv = rho * vr / v * g;
        s_d += dv - rho * d_rho / d * g;
        s_rho += (vr * logf(v) - d_rho * ln_d) * g;
        float dp = dv / u;
        const float du = -dv * p / (u * u);
        s_a += du * u * logf(Mf);
        const float gM = du * a * u / Mf + omw * gM_next;
        dp += w * gM;
        const float Mprev = m > 0 ? M[m - 1] : p0;
        s_w += gM * (p - Mprev);
        if (m == 0) dp += omw * gM;                 // the recurrence starts from p_0 (postprocessing.py:15)
        gM_next = gM;
        const float gv = (nofloor || r[m] > kPooledFloor) ? dp : 0.0f;
        gp[m] = gv;
        if (gc) gc[(size_t)m * FP] = gv;
    }
    const float al = alpha[f], ro = root[f], ew = ema_w[f];
    float* rs = rowsum + (size_t)row * 4;
    rs[0] = al < 1.0f ? s_a : (al == 1.0f ? 0.5f * s_a : 0.0f);
    rs[1] = s_d;
    const float g_reff = -s_rho * rho * rho;
    rs[2] = ro > 1.0f ? g_reff : (ro == 1.0f ? 0.5f * g_reff : 0.0f);
    rs[3] = (ew >= 0.0f && ew <= 1.0f) ? s_w : 0.0f;
}

// The wave-per-row form of pcen_bwd_rows_kernel: four rows per workgroup, the row's arithmetic in pcen_bwd_scan_row
// (leaf_pcen_scan.hpp, shared with the head-only backward of leaf_head_bwd.hpp), here with its per-frame stores.
__global__ __launch_bounds__(256) void pcen_bwd_scan_kernel(const float* __restrict__ raw, const void* __restrict__ gout, int BF,
                                                            int F, int TP, const float* __restrict__ alpha,
                                                            const float* __restrict__ delta, const float* __restrict__ root,
                                                            const float* __restrict__ ema_w, float floor_, int mode,
                                                            float* __restrict__ ema, float* __restrict__ gpre,
                                                            float* __restrict__ rowsum, const int* __restrict__ col_of, int FP,
                                                            float* __restrict__ gcols, float* __restrict__ grow = nullptr) {
    // grow (optional): grow[row] = sum_m g_pre[row][m], the row's share of d pool_b -- param_reduce_kernel then adds B numbers
    // per filter instead of re-reading the B x T' gradients (round 4: 22 -> 8 us at 256 x 1 s)
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= BF) return;
    const size_t go0 = (size_t)row * TP;
    const int f = row % F;
    float* gc = gcols ? gcols + (size_t)(row / F) * TP * FP + col_of[f] : nullptr;
    const ScanRowSums s = pcen_bwd_scan_row<true>(raw + go0, gout, go0, TP, f, alpha, delta, root, ema_w, floor_, mode, ema + go0,
                                                  gpre + go0, gc, FP, lane);
    if (lane == 0) {
        if (grow) grow[row] = s.g;
        if (mode & 1) {
            float* rs = rowsum + (size_t)row * 4;
            rs[0] = s.a;
            rs[1] = s.d;
            rs[2] = s.rho;
            rs[3] = s.w;
        }
    }
}

// One block per filter: d pool_b, d pool_w and the PCEN parameter sums over the batch.
constexpr int kParamRedThreads = 1024;
__global__ __launch_bounds__(kParamRedThreads) void param_reduce_kernel(const float* __restrict__ gpre, const float* __restrict__ dg,
                                    const float* __restrict__ g, const float* __restrict__ rowsum,
                                    const float* __restrict__ pool_w, int B, int F, int TP, int K, int mode,
                                    const float* __restrict__ dwpart, int dw_rows, int FP,
                                    const int* __restrict__ col_of, float* __restrict__ g_pool_w, float* __restrict__ g_pool_b, float* __restrict__ g_alpha,
                                    float* __restrict__ g_delta, float* __restrict__ g_root, float* __restrict__ g_ema,
                                    const float* __restrict__ dkpart = nullptr, int dk_blocks = 0, const float* __restrict__ kernel = nullptr,
                                    GaborBounds bd = GaborBounds{}, float* __restrict__ g_kernel = nullptr,
                                    const float* __restrict__ grow = nullptr) {
    __shared__ float red[2][kParamRedThreads / 64];
    const int f = blockIdx.x, tid = threadIdx.x;
    // sums of the block in a FIXED order (bit-reproducible): DPP / shuffle tree inside each wave, the sixteen wave sums added in wave
    // order by every thread -- two barriers per sum instead of the eleven of a shared-memory tree (round 4: this kernel is one of the
    // small launches around the main backward kernel; its seven sums were ~6 us of barriers)
    int parity = 0;
    auto block_sum = [&](float v) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        float* r = red[parity];
        parity ^= 1;                                  // two buffers: the next sum's writes cannot overtake this sum's reads
        if ((tid & 63) == 0) r[tid >> 6] = v;
        __syncthreads();
        float t = 0.0f;
#pragma unroll
        for (int w = 0; w < kParamRedThreads / 64; ++w) t += r[w];
        return t;
    };
    if (grow && dwpart) {
        // The overlap-save backwards (rows' sums from the scan kernel, per-block partials from the main kernel): every load of all
        // eight sums first, four strides of each at a time, then ONE barrier for the eight block sums -- one memory latency and one
        // barrier instead of eight of each (this kernel is a launch of a few microseconds between the main kernel and the caller).
        // Every sum adds the same numbers in the same order as the sequential form below (a lane's strided values ascending, the
        // wave's xor tree, the sixteen waves in order): the same bits.
        __shared__ float red8[kParamRedThreads / 64][8];
        const int col = col_of[f];
        const bool pc = (mode & 1) != 0;
        const int ndk = dkpart ? dk_blocks : 0;
        const int nmax = max(max(B, dw_rows), ndk);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int i0 = tid; i0 < nmax; i0 += 4 * kParamRedThreads) {
            float gr[4], dw[4];
            float4 rs[4];
            float2 dk[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * kParamRedThreads;
                gr[u] = i < B ? grow[(size_t)i * F + f] : 0.0f;
                rs[u] = (pc && i < B) ? *reinterpret_cast<const float4*>(rowsum + ((size_t)i * F + f) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                dw[u] = i < dw_rows ? dwpart[(size_t)i * FP + col] : 0.0f;
                dk[u] = i < ndk ? *reinterpret_cast<const float2*>(dkpart + ((size_t)i * F + f) * 2) : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {                     // (adding +0 for a stride past an array's end leaves the sum as it is)
                v[0] += gr[u];
                v[1] += dw[u];
                v[2] += rs[u].x;
                v[3] += rs[u].y;
                v[4] += rs[u].z;
                v[5] += rs[u].w;
                v[6] += dk[u].x;
                v[7] += dk[u].y;
            }
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[q] += __shfl_xor(v[q], off);
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) red8[tid >> 6][q] = v[q];
        }
        __syncthreads();
        if (tid == 0) {
            float t[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                t[q] = 0.0f;
#pragma unroll
                for (int w = 0; w < kParamRedThreads / 64; ++w) t[q] += red8[w][q];
            }
            const float wr0 = pool_w[f];
            if (g_pool_b) g_pool_b[f] = t[0];
            g_pool_w[f] = (wr0 >= 2.0f / (float)K && wr0 <= 0.5f) ? t[1] : 0.0f;
            if (pc) {
                g_alpha[f] = t[2];
                g_delta[f] = t[3];
                g_root[f] = t[4];
                g_ema[f] = t[5];
            }
            if (dkpart) {
                const float mu_raw = kernel[2 * f], sg_raw = kernel[2 * f + 1];
                g_kernel[2 * f] = (mu_raw >= 0.0f && mu_raw <= 3.14159274101257324f) ? t[6] : 0.0f;
                g_kernel[2 * f + 1] = (sg_raw >= bd.sigma_lo && sg_raw <= bd.sigma_hi) ? t[7] : 0.0f;
            }
        }
        return;
    }
    float acc = 0.0f;
    if (grow) {                                       // the rows' sums (pcen_bwd_scan_kernel)
        for (int b = tid; b < B; b += kParamRedThreads) acc += grow[(size_t)b * F + f];
    } else {
        for (int i = tid; i < B * TP; i += kParamRedThreads) {
            const int b = i / TP, m = i - b * TP;
            acc += gpre[((size_t)b * F + f) * TP + m];
        }
    }
    const float sb = block_sum(acc);
    // d g/d s = g * (j - c)^2 / (c^2 s^3), c = (K-1)/2   (impulse_responses.py:75-80)
    const float wr = pool_w[f];
    const float sig = pool_sigma(wr, K);
    const float c = 0.5f * (float)(K - 1);
    acc = 0.0f;
    if (dwpart) {                                     // fused backward: per-wave partial sums, tap-column order
        const int col = col_of[f];
        for (int i = tid; i < dw_rows; i += kParamRedThreads) acc += dwpart[(size_t)i * FP + col];
    } else {
        for (int j = tid; j < K; j += kParamRedThreads) {
            const float t = (float)j - c;
            acc += dg[(size_t)f * K + j] * g[(size_t)f * K + j] * (t * t) / (c * c * sig * sig * sig);
        }
    }
    const float sw = block_sum(acc);
    float sums[4] = {0.f, 0.f, 0.f, 0.f};
    if (mode & 1) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            acc = 0.0f;
            for (int b = tid; b < B; b += kParamRedThreads) acc += rowsum[((size_t)b * F + f) * 4 + q];
            sums[q] = block_sum(acc);
        }
    }
    // (overlap-save backward) the per-block (d mu, d sigma) partials of this filter and the clamp sub-gradients of
    // convolution.py:15-22 -- what fft_dkernel_reduce_kernel did in a launch of its own
    if (dkpart) {
        float a = 0.0f, c2 = 0.0f;
        for (int i = tid; i < dk_blocks; i += kParamRedThreads) {
            a += dkpart[((size_t)i * F + f) * 2];
            c2 += dkpart[((size_t)i * F + f) * 2 + 1];
        }
        const float smu = block_sum(a), ssg = block_sum(c2);
        if (tid == 0) {
            const float mu_raw = kernel[2 * f], sg_raw = kernel[2 * f + 1];
            g_kernel[2 * f] = (mu_raw >= 0.0f && mu_raw <= 3.14159274101257324f) ? smu : 0.0f;
            g_kernel[2 * f + 1] = (sg_raw >= bd.sigma_lo && sg_raw <= bd.sigma_hi) ? ssg : 0.0f;
        }
    }
    if (tid == 0) {
        if (g_pool_b) g_pool_b[f] = sb;
        g_pool_w[f] = (wr >= 2.0f / (float)K && wr <= 0.5f) ? sw : 0.0f;
        if (mode & 1) {
            g_alpha[f] = sums[0];
            g_delta[f] = sums[1];
            g_root[f] = sums[2];
            g_ema[f] = sums[3];
        }
    }
}

}  // namespace
