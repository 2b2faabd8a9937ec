// leaf_pcen_scan.hpp -- one (b, f) row of the floor + PCEN backward on one wave: the body pcen_bwd_scan_kernel (leaf_kernels_rows.hpp)
// and leaf_head_bwd_kernel (leaf_head_bwd.hpp) share.
// Included by both headers: one device function and its constants (gfx950 only).
#pragma once
#include "leaf_common.hpp"

namespace {

constexpr int kScanRegChunks = 4;

// what a row contributes to its filter's sums over the batch, the same value in every lane: d alpha, d delta, d root, d ema_w with
// the clamp sub-gradient conventions applied (zero without PCEN), and g = sum_m g_pre[m], the row's share of d pool_b
struct ScanRowSums {
    float a, d, rho, w, g;
};

// Same arithmetic as pcen_bwd_rows_kernel, one WAVE per (b,f) row instead of one lane: lane l owns frames 2l, 2l+1 of
// each 128-frame chunk.  The EMA (forward in time) and the gradient recurrence gM_m = c_m + (1-w) gM_{m+1} (backward in
// time) are first-order linear recurrences = compositions of affine maps: composed in-lane for the pair, scanned across
// the wavefront with 6 shuffle steps (up for the EMA, down for gM), with a carried state between chunks.  The serial
// kernel spends 137 us on B F = 10240 rows of 100 frames (160 waves, latency-bound); this one keeps the whole chip busy.
//   r      the row of pooled_raw (pre-floor), TP frames;   gout / go0: grad_out and the row's first element in it
//   mode   bit0 PCEN, bit1 log1p behind the floor (PCEN off only), bit2 grad_out is bfloat16 (widened in the load)
//   M      TP floats of the wave's own for the smoother's values of a row beyond kScanRegChunks x 128 frames (shorter rows: untouched)
//   STORE  the per-frame results leave the wave: gp[m] = g_pre of the row, and (gc != NULL) gc[m * FP] its tap-column copy.
//          Without it the sums are all that is computed: gp / gc are not touched.
template <bool STORE>
__device__ __forceinline__ ScanRowSums pcen_bwd_scan_row(const float* __restrict__ r, const void* __restrict__ gout, size_t go0, int TP,
                                                         int f, const float* __restrict__ alpha, const float* __restrict__ delta,
                                                         const float* __restrict__ root, const float* __restrict__ ema_w,
                                                         float floor_, int mode, float* M, float* __restrict__ gp,
                                                         float* __restrict__ gc, int FP, int lane) {
    const int gbf = (mode & 4) ? kSampleBf16 : kSampleF32;                        // grad_out is bfloat16 (widened in the load)
    if (!(mode & 1)) {
        float sg = 0.0f;
        for (int m = lane; m < TP; m += 64) {
            const float g = io_load(gout, go0 + m, gbf);
            const float v = r[m] > kPooledFloor ? ((mode & 2) ? g / (1.0f + r[m]) : g) : 0.0f;       // log1p: d log1p(p) / d p
            sg += v;
            if constexpr (STORE) {
                gp[m] = v;
                if (gc) gc[(size_t)m * FP] = v;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sg += __shfl_xor(sg, off);
        return ScanRowSums{0.0f, 0.0f, 0.0f, 0.0f, sg};
    }
    const float w = fminf(fmaxf(ema_w[f], 0.0f), 1.0f), omw = 1.0f - w;
    const float a = fminf(alpha[f], 1.0f);
    const float reff = fmaxf(root[f], 1.0f), rho = 1.0f / reff;
    const float d = delta[f];
    const float d_rho = powf(d, rho), ln_d = logf(d);
    const bool fast = d > 1e-30f;                                         // the hardware log2 / exp2 forms (see below)
    const float p0 = fmaxf(r[0], kPooledFloor);
    const int nchunk = (TP + 127) / 128;
    // rows of up to kScanRegChunks x 128 frames keep the smoother's values in registers between the two passes (the pass back in time
    // needs M_m and M_{m-1} of the lane's own two frames: a neighbour's register, not a round trip through `ema` in memory); longer
    // rows store them and read them back
    constexpr int RC = kScanRegChunks;
    const bool inreg = nchunk <= RC;
    float M0r[RC], M1r[RC];
    // ---- forward in time: M_m = w p_m + (1-w) M_{m-1}, M_{-1} = p_0 (postprocessing.py:15)
    float carry = p0;
    auto fwd_chunk = [&](int c, float& M0, float& M1, bool& ok0, bool& ok1) {
        const int j0 = 128 * c + 2 * lane, j1 = j0 + 1;
        ok0 = j0 < TP;
        ok1 = j1 < TP;
        const float q0 = ok0 ? fmaxf(r[j0], kPooledFloor) : 0.0f, q1 = ok1 ? fmaxf(r[j1], kPooledFloor) : 0.0f;
        const float A0 = ok0 ? omw : 1.0f, B0 = ok0 ? w * q0 : 0.0f, A1 = ok1 ? omw : 1.0f, B1 = ok1 ? w * q1 : 0.0f;
        float A = A1 * A0, Bv = fmaf(A1, B0, B1);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float Ap = __shfl_up(A, off), Bp = __shfl_up(Bv, off);
            if (lane >= off) {
                Bv = fmaf(A, Bp, Bv);
                A *= Ap;
            }
        }
        const float Mend = fmaf(A, carry, Bv);
        const float Mprev = __shfl_up(Mend, 1);
        M0 = fmaf(A0, lane ? Mprev : carry, B0);
        if (c == 0 && lane == 0) M0 = q0;                                  // M_0 = w p_0 + (1-w) p_0 = p_0 exactly, not to a rounding
        M1 = fmaf(A1, M0, B1);
        carry = __shfl(Mend, 63);
    };
    if (inreg) {
#pragma unroll
        for (int c = 0; c < RC; ++c) {
            M0r[c] = M1r[c] = 0.0f;
            if (c < nchunk) {
                bool ok0, ok1;
                fwd_chunk(c, M0r[c], M1r[c], ok0, ok1);
            }
        }
    } else {
        for (int c = 0; c < nchunk; ++c) {
            float M0, M1;
            bool ok0, ok1;
            fwd_chunk(c, M0, M1, ok0, ok1);
            if (ok0) M[128 * c + 2 * lane] = M0;
            if (ok1) M[128 * c + 2 * lane + 1] = M1;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");           // M is re-read below by other lanes of this wave
        __builtin_amdgcn_s_waitcnt(0);
    }
    // ---- backward in time
    float s_a = 0.f, s_d = 0.f, s_rho = 0.f, s_w = 0.f, s_g = 0.f;
    float gnext = 0.0f;                                                   // gM of the first frame of the following chunk
    // Mv0 / Mv1: M at the lane's frames j0, j0 + 1; Mb: M at j0 - 1 (p_0 in front of the row)
    // dL/dp_m = dpd_m + wm gM_m with gM_m = cm_m + (1-w) gM_{m+1}, cm_m = -dpd_m t_m, t_m = alpha p_m / (floor + M_m), wm = w (m = 0:
    // 1, the recurrence starts from p_0).  The frame's own share is taken in factored form, dpd_m (1 - wm t_m): at the first frame
    // M_0 = p_0 makes t_0 = alpha and the two terms agree to 1 - alpha (0.04 at the default) -- as a difference of two rounded products
    // a clip of ONE frame lost 25x .. 125x their rounding (tests/test_gpu_backward_edges.py); 1 - alpha (p / (floor + M)) is exact there.
    auto bwd_chunk = [&](int c, float Mv0, float Mv1, float Mb) {
        const int j0 = 128 * c + 2 * lane;
        float cm[2], dpd[2], pv[2], Mp[2], own[2];
        bool ok[2], above[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int m = j0 + k;
            ok[k] = m < TP;
            cm[k] = dpd[k] = pv[k] = Mp[k] = own[k] = 0.0f;
            above[k] = false;
            if (ok[k]) {
                const float rv = r[m];
                const float p = fmaxf(rv, kPooledFloor);
                above[k] = rv > kPooledFloor;
                // powers and logarithms on the hardware log2 / exp2 (1 ulp each; the forward's leaf_pow_pos): one log2 serves both
                // the power and the logarithm of the same argument -- 2 v_log + 2 v_exp per frame instead of two powf and two
                // logf calls (~60-100 instructions each); non-positive v gives NaN / -inf exactly where powf / logf do
                // A filter whose learned delta is <= 0 (or denormal) keeps the library powf / logf: that is the function the forward
                // evaluates there (fin_point's literal form), v = p / u + delta may be tiny or non-positive, and the raw
                // v_log_f32 / v_exp_f32 do not handle denormals like powf.  Wave-uniform: delta is per row.
                const float Mf = floor_ + (k ? Mv1 : Mv0);
                float l2M, u, v, l2v, vr;
                if (fast) {
                    l2M = __builtin_amdgcn_logf(Mf);
                    u = __builtin_amdgcn_exp2f(a * l2M);
                    v = p / u + d;
                    l2v = __builtin_amdgcn_logf(v);
                    vr = __builtin_amdgcn_exp2f(rho * l2v);
                } else {
                    l2M = logf(Mf) * 1.4426950408889634f;
                    u = powf(Mf, a);
                    v = p / u + d;
                    l2v = logf(v) * 1.4426950408889634f;
                    vr = powf(v, rho);
                }
                const float g = io_load(gout, go0 + m, gbf);
                const float dv = rho * vr / v * g;
                s_d += dv - rho * d_rho / d * g;
                s_rho += (vr * (l2v * 0.6931471805599453f) - d_rho * ln_d) * g;
                dpd[k] = dv / u;
                const float t = a * (p / Mf);
                s_a -= dpd[k] * p * (l2M * 0.6931471805599453f);          // d/d alpha: du u ln M with du = -dv p / u^2
                cm[k] = -dpd[k] * t;                                      // du alpha u / (floor + M)
                own[k] = dpd[k] * (1.0f - (m == 0 ? t : w * t));
                pv[k] = p;
                Mp[k] = k ? Mv0 : Mb;
            }
        }
        // gM_m = cm_m + beta_m gM_{m+1}: pair map, then the inclusive scan over lanes from the high end
        const float b0 = ok[0] ? omw : 1.0f, b1 = ok[1] ? omw : 1.0f;
        float A = b0 * b1, Bv = fmaf(b0, cm[1], cm[0]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float Ap = __shfl_down(A, off), Bp = __shfl_down(Bv, off);
            if (lane + off < 64) {
                Bv = fmaf(A, Bp, Bv);
                A *= Ap;
            }
        }
        const float g0 = fmaf(A, gnext, Bv);                              // gM of this lane's first frame
        const float gn = __shfl_down(g0, 1);
        const float g2 = lane < 63 ? gn : gnext;                          // gM of the frame after this lane's second
        const float g1 = fmaf(b1, g2, cm[1]);                             // gM of this lane's second frame
        gnext = __shfl(g0, 0);
        const float gM[2] = {g0, g1}, gMnext[2] = {g1, g2};              // (past the row's end: 0)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int m = j0 + k;
            if (ok[k]) {
                const float dp = fmaf(m == 0 ? omw : w * omw, gMnext[k], own[k]);
                s_w += gM[k] * (pv[k] - Mp[k]);
                const float gv = above[k] ? dp : 0.0f;
                s_g += gv;
                if constexpr (STORE) {
                    gp[m] = gv;
                    if (gc) gc[(size_t)m * FP] = gv;
                }
            }
        }
    };
    if (inreg) {
#pragma unroll
        for (int c = RC - 1; c >= 0; --c) {
            // M at j0 - 1: the previous lane's second frame; lane 0: the previous chunk's last frame (p_0 in front of the row)
            const float up = __shfl_up(M1r[c], 1);
            const float prev_chunk = c > 0 ? __shfl(M1r[c > 0 ? c - 1 : 0], 63) : p0;
            if (c < nchunk) bwd_chunk(c, M0r[c], M1r[c], lane ? up : prev_chunk);
        }
    } else {
        for (int c = nchunk - 1; c >= 0; --c) {
            const int j0 = 128 * c + 2 * lane;
            const float Mv0 = j0 < TP ? M[j0] : 0.0f, Mv1 = j0 + 1 < TP ? M[j0 + 1] : 0.0f;
            const float Mb = (j0 < TP && j0 > 0) ? M[j0 - 1] : p0;
            bwd_chunk(c, Mv0, Mv1, Mb);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        s_a += __shfl_xor(s_a, off);
        s_d += __shfl_xor(s_d, off);
        s_rho += __shfl_xor(s_rho, off);
        s_w += __shfl_xor(s_w, off);
        s_g += __shfl_xor(s_g, off);
    }
    // the clamp sub-gradients of postprocessing.py:14,63-64 (torch.clamp / torch.min / torch.max): alpha == 1 and root == 1 take half,
    // ema_w outside [0, 1] takes none
    const float al = alpha[f], ro = root[f], ew = ema_w[f];
    const float g_reff = -s_rho * rho * rho;
    return ScanRowSums{al < 1.0f ? s_a : (al == 1.0f ? 0.5f * s_a : 0.0f), s_d,
                       ro > 1.0f ? g_reff : (ro == 1.0f ? 0.5f * g_reff : 0.0f), (ew >= 0.0f && ew <= 1.0f) ? s_w : 0.0f, s_g};
}

}  // namespace
