// leaf_clip_effects.hpp -- ClipValue and the sox-style reverb of leaf_clip_effects_f32 as plain functions, for the device and for the
// host: csrc/inst_clip_effects.hip builds its kernel on them, and tools/clip_effects_check.cpp runs the sequential definition on the
// CPU with them (the host test compares it with a NumPy oracle; under -fsanitize=undefined,address it walks hostile plans).  No HIP
// header is needed.
//
// The definition is in include/leaf_hip.h (leaf_clip_effects_f32); this file IS that definition in code.  Every float32 operation
// is rounded on its own: contraction is switched off inside each function (clang: the pragma below; another compiler:
// -ffp-contract=off).  The lengths are host arithmetic in IEEE double.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEAF_FX_HD __host__ __device__
#else
#define LEAF_FX_HD
#endif
#if defined(__clang__)
#define LEAF_FX_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LEAF_FX_NO_CONTRACT
#endif
// (HIP's __fmul_rn / __fadd_rn / __fsub_rn are plain operators inside header functions compiled with contraction ON: two of them
// inline into one fused multiply-add.  The operators below stand under the pragma, which is what keeps every rounding.)
#define LEAF_FX_MUL(a, b) ((a) * (b))
#define LEAF_FX_ADD(a, b) ((a) + (b))
#define LEAF_FX_SUB(a, b) ((a) - (b))

constexpr int kFxCombs = 8, kFxAllpasses = 4;
constexpr int kFxCombTuning[kFxCombs] = {1116, 1188, 1277, 1356, 1422, 1491, 1557, 1617};     // Freeverb's lengths at 44.1 kHz
constexpr int kFxAllpassTuning[kFxAllpasses] = {225, 341, 441, 556};
constexpr int kFxLdsBudget = 64 * 1024;               // bytes of LDS one workgroup may take (the budget of the library's other kernels)
constexpr int kFxMaxClipsPerGroup = 8;                // 8 clips x 8 combs: the 64 lanes of the wave that runs the serial part

// the delay lines' lengths that depend on the call alone: cap[i] is comb i at room_scale = 100, allpass[j] all-pass j
struct FxLengths {
    int cap[kFxCombs];
    int allpass[kFxAllpasses];
};

// (int)(scale r C + 0.5) in double, the association of the header; 0 for what is no length (below 1, NaN, or beyond 2^24 samples)
inline int fx_length(double scale, double r, int tuning) {
    const double v = scale * r * (double)tuning + 0.5;
    return (v >= 1.0 && v < 16777216.0) ? (int)v : 0;
}
inline double fx_room_scale(double room_scale_percent) { return room_scale_percent / 100.0 * 0.9 + 0.1; }

// the call's lengths; false when one of them is not a length
inline bool fx_lengths(int sample_rate, FxLengths& L) {
    if (sample_rate < 1) return false;
    const double r = (double)sample_rate / 44100.0;
    bool ok = true;
    for (int i = 0; i < kFxCombs; ++i) ok = (L.cap[i] = fx_length(fx_room_scale(100.0), r, kFxCombTuning[i])) >= 1 && ok;
    for (int j = 0; j < kFxAllpasses; ++j) ok = (L.allpass[j] = fx_length(1.0, r, kFxAllpassTuning[j])) >= 1 && ok;
    return ok;
}

// Floats of LDS one clip takes: the eight comb lines at their caps, the four all-pass lines, and the staged chunk (a chunk is never
// longer than the shortest all-pass).  Clips per workgroup of `threads` lanes: as many as fit the budget, at most
// kFxMaxClipsPerGroup, and no more than leave every clip allpass[0] lanes (a whole chunk in one pass) -- but 1 where a clip fits at
// all; 0: the rate's lines do not fit.
inline long long fx_clip_floats(const FxLengths& L) {
    long long n = L.allpass[0];
    for (int i = 0; i < kFxCombs; ++i) n += L.cap[i];
    for (int j = 0; j < kFxAllpasses; ++j) n += L.allpass[j];
    return n;
}
inline int fx_clips_per_group(const FxLengths& L, int threads) {
    long long fit = (long long)(kFxLdsBudget / sizeof(float)) / fx_clip_floats(L);
    if (fit < 1) return 0;
    const long long lanes = threads / L.allpass[0];
    if (fit > lanes) fit = lanes < 1 ? 1 : lanes;
    return (int)(fit < kFxMaxClipsPerGroup ? fit : kFxMaxClipsPerGroup);
}

// a plan's comb length as the kernel uses it: clamped into [1, cap]
LEAF_FX_HD inline int fx_clamp_length(int len, int cap) { return len < 1 ? 1 : (len > cap ? cap : len); }

// ClipValue.  The bounds from the clip's exact minimum and maximum (a zero of either sign counts as +0: `+ 0.0f`), one multiply each;
// the clamp is torch.clamp's min(max(x, lo), hi) written out, so that a tie between zeros resolves the same way on every side.
LEAF_FX_HD inline void fx_clip_bounds(float mn, float mx, float factor, float& lo, float& hi) {
    LEAF_FX_NO_CONTRACT
    lo = LEAF_FX_MUL(LEAF_FX_ADD(mn, 0.0f), factor);
    hi = LEAF_FX_MUL(LEAF_FX_ADD(mx, 0.0f), factor);
}
LEAF_FX_HD inline float fx_clip(float x, float lo, float hi) {
    const float m = x < lo ? lo : x;
    return hi < m ? hi : m;
}

// One comb step: `o` is what the line holds at the write index, `store` the damping state; returns what the line takes.
LEAF_FX_HD inline float fx_comb(float o, float in, float& store, float damp, float feedback) {
    LEAF_FX_NO_CONTRACT
    store = LEAF_FX_ADD(o, LEAF_FX_MUL(LEAF_FX_SUB(store, o), damp));
    return LEAF_FX_ADD(in, LEAF_FX_MUL(store, feedback));
}
// One all-pass step: `o` is what the line holds, `out` the running sample (in: the stage's input, out: its output); returns what
// the line takes.
LEAF_FX_HD inline float fx_allpass(float o, float& out) {
    LEAF_FX_NO_CONTRACT
    const float w = LEAF_FX_ADD(out, LEAF_FX_MUL(o, 0.5f));
    out = LEAF_FX_SUB(o, out);
    return w;
}
LEAF_FX_HD inline float fx_sum(float out, float o) {
    LEAF_FX_NO_CONTRACT
    return LEAF_FX_ADD(out, o);
}
LEAF_FX_HD inline float fx_mix(float in, float out, float wet) {
    LEAF_FX_NO_CONTRACT
    return LEAF_FX_ADD(in, LEAF_FX_MUL(out, wet));
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The sequential definition for one clip, on the host: y[0, S) from x[0, S).  `lines` is the caller's scratch of
// fx_clip_floats(L) - L.allpass[0] floats (the layout the kernel keeps in LDS: combs at their caps, then the all-passes); `comb`
// NULL or comb[0] <= 0 skips the reverb, factor < 0 ClipValue.  The comb lengths are clamped as the kernel clamps them.
inline void fx_clip_sequential(const float* x, float* y, long long S, float factor, float feedback, float damp, const int* comb,
                               const FxLengths& L, float wet, float* lines) {
    float lo = 0.0f, hi = 0.0f;
    const bool clip = factor >= 0.0f && S > 0;
    if (clip) {
        float mn = x[0], mx = x[0];
        for (long long n = 1; n < S; ++n) {
            mn = x[n] < mn ? x[n] : mn;
            mx = x[n] > mx ? x[n] : mx;
        }
        fx_clip_bounds(mn, mx, factor, lo, hi);
    }
    const bool reverb = comb != nullptr && comb[0] > 0;
    float* cb[kFxCombs];
    float* ap[kFxAllpasses];
    int len[kFxCombs], p[kFxCombs] = {}, q[kFxAllpasses] = {};
    float store[kFxCombs] = {};
    if (reverb) {
        float* at = lines;
        for (int i = 0; i < kFxCombs; ++i) {
            len[i] = fx_clamp_length(comb[i], L.cap[i]);
            cb[i] = at;
            at += L.cap[i];
        }
        for (int j = 0; j < kFxAllpasses; ++j) {
            ap[j] = at;
            at += L.allpass[j];
        }
        for (float* z = lines; z < at; ++z) *z = 0.0f;
    }
    for (long long n = 0; n < S; ++n) {
        const float in = clip ? fx_clip(x[n], lo, hi) : x[n];
        if (!reverb) {
            y[n] = in;
            continue;
        }
        float out = 0.0f;
        for (int i = kFxCombs - 1; i >= 0; --i) {
            const float o = cb[i][p[i]];
            cb[i][p[i]] = fx_comb(o, in, store[i], damp, feedback);
            if (++p[i] == len[i]) p[i] = 0;
            out = fx_sum(out, o);
        }
        for (int j = kFxAllpasses - 1; j >= 0; --j) {
            const float o = ap[j][q[j]];
            ap[j][q[j]] = fx_allpass(o, out);
            if (++q[j] == L.allpass[j]) q[j] = 0;
        }
        y[n] = fx_mix(in, out, wet);
    }
}
#endif
