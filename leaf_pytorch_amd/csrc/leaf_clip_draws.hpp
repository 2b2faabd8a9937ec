// leaf_clip_draws.hpp -- the random draws of one clip's plan (leaf_draw_clip_plan) as plain functions, for the device and for the
// host: csrc/leaf_clips.hpp builds its kernel on them, and tools/clip_draws_check.cpp prints the plan they give on the CPU (the
// host test compares it with a NumPy oracle; under -fsanitize=undefined,address it walks hostile constants).  No HIP header is needed.
//
// The definition is in include/leaf_hip.h (leaf_draw_clip_plan); this file IS that definition in code.  Integers are exact on every
// side.  The floating-point part is IEEE double add / multiply / divide in the association written here -- contraction is switched
// off (clang: the pragma below; another compiler: -ffp-contract=off) -- and one double exp per gain and per SNR, the only inexact
// operation, rounded once to float32.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LEAF_DRAW_HD __host__ __device__
#else
#define LEAF_DRAW_HD
#endif
#if defined(__clang__)
#define LEAF_DRAW_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define LEAF_DRAW_NO_CONTRACT
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define LEAF_DRAW_EXP(x) exp(x)
#else
#include <cmath>
#define LEAF_DRAW_EXP(x) std::exp(x)
#endif

constexpr int kDrawMaxMasks = 32;                     // M <= 32: the masks' counters 2 .. 33 stay below the noise counter
constexpr unsigned kDrawNoiseCounter = 64u, kDrawGaussCounter = 65u;
constexpr double kDrawLn10 = 2.302585092994045684;    // ln 10, the double next to it (numpy's log(10.0))

// what the sampler is constructed with: the same for every clip and every step
struct ClipDrawConsts {
    int S, train;                 // clip size in [1, 2^31); RandomCrop (1) or CenterCrop (0)
    int mode0, mode1;             // pad modes: mode0 with probability wrap_pad_prob, else mode1
    int M;                        // time-mask spans per clip, 0 .. kDrawMaxMasks
    double wrap_pad_prob, gain_prob, gain_lo, gain_hi, time_perc;
    double noise_prob, snr_lo, snr_hi, gauss_prob, amp_lo, amp_hi;
};

// Philox4x32-10, the rounds of the Gaussian stream (csrc/leaf_clips.hpp: philox4x32_10) with the products in 64 bits
LEAF_DRAW_HD inline void draw_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        c0 = (unsigned)(p1 >> 32) ^ c1 ^ k0; c1 = (unsigned)p1; c2 = (unsigned)(p0 >> 32) ^ c3 ^ k1; c3 = (unsigned)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// P(q): key = the seed's halves, counter = (q, 1, the id's halves).  Word 1 is 1: the Gaussian stream has 0 there.
LEAF_DRAW_HD inline void draw_words(unsigned long long seed, unsigned long long id, unsigned q, unsigned (&r)[4]) {
    draw_philox(q, 1u, (unsigned)id, (unsigned)(id >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
}

// u(r) = r 2^-32 in [0, 1), exact in double
LEAF_DRAW_HD inline double draw_unit(unsigned r) { return (double)r * 0x1p-32; }

// a uniform integer in [0, n), 1 <= n <= 2^32: (r n) >> 32, integers only
LEAF_DRAW_HD inline long long draw_below(unsigned r, long long n) { return (long long)(((unsigned long long)r * (unsigned long long)n) >> 32); }

// clip b's id at `step`: stream_base + step B + b, and its place in `order`: (step B + b) mod N -- unsigned 64-bit, wrapping
LEAF_DRAW_HD inline unsigned long long draw_clip_id(unsigned long long stream_base, unsigned long long step, int B, int b) {
    return stream_base + step * (unsigned long long)B + (unsigned long long)b;
}
LEAF_DRAW_HD inline long long draw_order_place(unsigned long long step, int B, int b, long long N) {
    return (long long)((step * (unsigned long long)B + (unsigned long long)b) % (unsigned long long)N);       // N >= 1
}

// a recording index that cannot be seen, into [0, R); R >= 1
LEAF_DRAW_HD inline int draw_clamp_index(long long i, int R) { return (int)(i < 0 ? 0 : (i > (long long)R - 1 ? (long long)R - 1 : i)); }

// max(L - S, 0) for any int L (a hostile length below 0 counts as 0)
LEAF_DRAW_HD inline long long draw_span(int L, int S) {
    const long long d = (long long)L - (long long)S;
    return d > 0 ? d : 0;
}

struct ClipDraw {
    int pad_mode, start;
    float gain;
};

// P(0): pad mode, crop start, gain
LEAF_DRAW_HD inline ClipDraw draw_clip(const ClipDrawConsts& k, unsigned long long seed, unsigned long long id, int L) {
    LEAF_DRAW_NO_CONTRACT
    unsigned r[4];
    draw_words(seed, id, 0u, r);
    ClipDraw d;
    d.pad_mode = draw_unit(r[0]) < k.wrap_pad_prob ? k.mode0 : k.mode1;
    const long long span = draw_span(L, k.S);
    d.start = (int)(k.train ? draw_below(r[1], span + 1) : span / 2);
    d.gain = 1.0f;
    if (draw_unit(r[2]) < k.gain_prob) {
        const double db = k.gain_lo + (k.gain_hi - k.gain_lo) * draw_unit(r[3]);
        d.gain = (float)LEAF_DRAW_EXP(db * (kDrawLn10 / 20.0));
    }
    return d;
}

// P(1): the spans in use, 1 .. M (M >= 1)
LEAF_DRAW_HD inline int draw_masks_used(const ClipDrawConsts& k, unsigned long long seed, unsigned long long id) {
    unsigned r[4];
    draw_words(seed, id, 1u, r);
    return 1 + (int)draw_below(r[0], k.M);
}

// P(2 + m): span m as (t0, n).  n = min(S, floor((u time_perc) S)), not below 0 (a time_perc that is negative or NaN masks
// nothing); t0 = floor(u' (S - n)) in [0, S - n]
LEAF_DRAW_HD inline void draw_mask(const ClipDrawConsts& k, unsigned long long seed, unsigned long long id, int m, int used, int& t0, int& n) {
    LEAF_DRAW_NO_CONTRACT
    unsigned r[4];
    draw_words(seed, id, 2u + (unsigned)m, r);
    n = 0;
    if (m < used) {
        const double v = (draw_unit(r[0]) * k.time_perc) * (double)k.S;
        n = v >= (double)k.S ? k.S : (v > 0.0 ? (int)v : 0);
    }
    t0 = (int)(draw_unit(r[1]) * (double)(k.S - n));
}

struct NoiseDraw {
    int apply, rec;               // mixed or not; the noise recording, in [0, Rn)
    unsigned start_word;          // r3: the start is (r3 (nspan + 1)) >> 32 once the recording's length is known
    float c, cn;                  // f32(c), f32(1 - c), c = r / (1 + r), r = exp(snr ln 10 / 10)
};

// P(64): background noise; Rn >= 1
LEAF_DRAW_HD inline NoiseDraw draw_noise(const ClipDrawConsts& k, unsigned long long seed, unsigned long long id, int Rn) {
    LEAF_DRAW_NO_CONTRACT
    unsigned r[4];
    draw_words(seed, id, kDrawNoiseCounter, r);
    NoiseDraw d;
    d.apply = draw_unit(r[0]) < k.noise_prob ? 1 : 0;
    const double snr = k.snr_lo + (k.snr_hi + 1.0 - k.snr_lo) * draw_unit(r[1]);
    d.rec = (int)draw_below(r[2], Rn);
    d.start_word = r[3];
    const double ratio = LEAF_DRAW_EXP(snr * (kDrawLn10 / 10.0));
    const double c = ratio / (1.0 + ratio);
    d.c = (float)c;
    d.cn = (float)(1.0 - c);
    return d;
}

LEAF_DRAW_HD inline int draw_noise_start(const NoiseDraw& d, int Ln, int S) { return (int)draw_below(d.start_word, draw_span(Ln, S) + 1); }

// P(65): the Gaussian amplitude (0: the clip is left alone); the clip's stream is its id
LEAF_DRAW_HD inline float draw_gauss_amp(const ClipDrawConsts& k, unsigned long long seed, unsigned long long id) {
    LEAF_DRAW_NO_CONTRACT
    unsigned r[4];
    draw_words(seed, id, kDrawGaussCounter, r);
    return draw_unit(r[0]) < k.gauss_prob ? (float)(k.amp_lo + (k.amp_hi - k.amp_lo) * draw_unit(r[1])) : 0.0f;
}

// ---- the whole call: its arguments, and everything it reads and writes for clip b ----------------------------------------------------
struct DrawParams {
    const long long* offsets;     // [R] the clip store's recordings
    const int* lengths;           // [R]
    const long long* noise_offsets;   // [Rn] or null: no noise group
    const int* noise_lengths;     // [Rn]
    const long long* index;       // [B], or null with ...
    const long long* order;       // [N]: clip b is order[(step B + b) mod N]
    long long N;
    unsigned long long* state;    // the step counter
    unsigned long long seed, stream_base;
    ClipDrawConsts k;
    int B, R, Rn, advance;
    long long* rec_off;           // [B] ... the outputs, in the dtypes of the assembly entries; a null group is not drawn
    int *rec_len, *start, *pad_mode;
    float* gain;
    int* masks;                   // [B][M][2]
    int* rec;
    long long* noise_off;
    int *noise_len, *noise_start, *noise_pad_mode;
    float* noise_coeff;           // [B][2]
    float* gauss_amp;
    long long* gauss_stream;
    long long* index_out;
};

// clip b, 0 <= b < B, at `step`: reads inside offsets / lengths [0, R), noise_* [0, Rn), index [0, B) or order [0, N) only, writes
// entry b of every output that is there
LEAF_DRAW_HD inline void draw_plan_clip(const DrawParams& p, unsigned long long step, int b) {
    const unsigned long long id = draw_clip_id(p.stream_base, step, p.B, b);
    const int i = draw_clamp_index(p.index ? p.index[b] : p.order[draw_order_place(step, p.B, b, p.N)], p.R);
    const int L = p.lengths[i];
    const ClipDraw d = draw_clip(p.k, p.seed, id, L);
    p.rec_off[b] = p.offsets[i];
    p.rec_len[b] = L;
    p.start[b] = d.start;
    p.pad_mode[b] = d.pad_mode;
    if (p.gain) p.gain[b] = d.gain;
    if (p.rec) p.rec[b] = i;
    if (p.index_out) p.index_out[b] = i;
    if (p.masks) {
        const int used = draw_masks_used(p.k, p.seed, id);
        int* mb = p.masks + 2 * (size_t)b * (size_t)p.k.M;
        for (int m = 0; m < p.k.M; ++m) {
            int t0, n;
            draw_mask(p.k, p.seed, id, m, used, t0, n);
            mb[2 * m] = t0;
            mb[2 * m + 1] = n;
        }
    }
    if (p.noise_off) {
        const NoiseDraw nd = draw_noise(p.k, p.seed, id, p.Rn);
        const int Ln = p.noise_lengths[nd.rec];
        p.noise_off[b] = p.noise_offsets[nd.rec];
        p.noise_len[b] = nd.apply ? Ln : 0;
        p.noise_start[b] = nd.apply ? draw_noise_start(nd, Ln, p.k.S) : 0;
        p.noise_pad_mode[b] = 2;
        p.noise_coeff[2 * b] = nd.c;
        p.noise_coeff[2 * b + 1] = nd.cn;
    }
    if (p.gauss_amp) {
        p.gauss_amp[b] = draw_gauss_amp(p.k, p.seed, id);
        p.gauss_stream[b] = (long long)id;
    }
}
