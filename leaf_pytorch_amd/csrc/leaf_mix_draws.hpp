// leaf_mix_draws.hpp -- mixup's draws for one clip (leaf_draw_mixup): the weight lam ~ Beta(alpha, alpha) and the 64-bit key whose
// order IS the permutation, as plain functions for the device and for the host: csrc/leaf_clips.hpp builds draw_mixup_kernel on
// them, and tools/mix_draws_check.cpp prints what they give on the CPU (the host test compares it with a NumPy oracle; under
// -fsanitize=undefined,address it walks hostile constants).  No HIP header is needed.
//
// The definition is in include/leaf_hip.h (leaf_draw_mixup); this file IS that definition in code.  Philox, the clip's id and u(r)
// are leaf_clip_draws.hpp's.  The floating point is IEEE double in the association written here, contraction off, rounded once to
// float32; the only inexact operations are one pow and one cos per clip.
#pragma once
#include "leaf_clip_draws.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define LEAF_MIX_POW(x, y) pow(x, y)
#define LEAF_MIX_COS(x) cos(x)
#define LEAF_MIX_SQRT(x) sqrt(x)
#define LEAF_MIX_COPYSIGN(x, y) copysign(x, y)
#else
#include <cmath>
#define LEAF_MIX_POW(x, y) std::pow(x, y)
#define LEAF_MIX_COS(x) std::cos(x)
#define LEAF_MIX_SQRT(x) std::sqrt(x)
#define LEAF_MIX_COPYSIGN(x, y) std::copysign(x, y)
#endif

constexpr int kMixMaxBatch = 4096;                    // B <= 4096: the workgroup orders the keys in 32 KB of LDS
constexpr unsigned kMixDomain = 2u;                   // counter word 1: 0 is the Gaussian stream's, 1 the clip plan's
constexpr double kMixTwoPi = 6.283185307179586;       // the double next to 2 pi

// the clip's four words: key = the seed's halves, counter = (0, 2, the id's halves)
LEAF_DRAW_HD inline void draw_mix_words(unsigned long long seed, unsigned long long id, unsigned (&r)[4]) {
    draw_philox(0u, kMixDomain, (unsigned)id, (unsigned)(id >> 32), (unsigned)seed, (unsigned)(seed >> 32), r);
}

// lam ~ Beta(alpha, alpha) from two words, no rejection.  With T Student-t of 2 alpha degrees of freedom, 1/2 + T / (2 sqrt(2 alpha +
// T^2)) is Beta(alpha, alpha), and Bailey's polar form gives T = sqrt(2 alpha (U^(-1/alpha) - 1)) cos(2 pi V); below, the quotient is
// multiplied through by w = U^(1/alpha), so that nothing overflows for a small alpha: w may underflow to 0 and never exceeds 1.
// V = 1/4 and 3/4 give c = 0 by definition: the cos of the double next to pi / 2 is about 6e-17 with a sign that is the library's,
// and with w = 0 that sign would decide between 0 and 1.
LEAF_DRAW_HD inline float draw_mix_lam(unsigned r0, unsigned r1, double alpha) {
    LEAF_DRAW_NO_CONTRACT
    const double U = ((double)r0 + 1.0) * 0x1p-32;                        // (0, 1]
    const double V = draw_unit(r1);
    const double w = LEAF_MIX_POW(U, 1.0 / alpha);
    const double c = (r1 & 0x7FFFFFFFu) == 0x40000000u ? 0.0 : LEAF_MIX_COS(kMixTwoPi * V);
    const double n = (1.0 - w) * (c * c);
    const double d = w + n;
    const double s = d > 0.0 ? LEAF_MIX_SQRT(n / d) : 0.0;
    return (float)(0.5 + 0.5 * LEAF_MIX_COPYSIGN(s, c));
}

// the key of clip b: perm[k] is the b with the k-th smallest key.  The low word is b itself, so two keys never tie and every real key
// is below the all-ones key that pads the sort.
LEAF_DRAW_HD inline unsigned long long draw_mix_key(unsigned r2, int b) { return ((unsigned long long)r2 << 32) | (unsigned long long)(unsigned)b; }

struct MixDraw {
    float lam;
    unsigned long long key;
};

// clip b, 0 <= b < B, at `step`; r[3] is not used
LEAF_DRAW_HD inline MixDraw draw_mix_clip(unsigned long long seed, unsigned long long stream_base, unsigned long long step, int B, int b,
                                          double alpha) {
    unsigned r[4];
    draw_mix_words(seed, draw_clip_id(stream_base, step, B, b), r);
    MixDraw d;
    d.lam = draw_mix_lam(r[0], r[1], alpha);
    d.key = draw_mix_key(r[2], b);
    return d;
}
