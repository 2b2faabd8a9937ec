// leaf_common.hpp -- tuning knobs, vector types, sample loads (bfloat16 / PCM16 / mixup), Gabor tap / pooling-window formulas
// Included by every unit: templates, device functions, constexpr sizes (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include "leaf_fastmath.hpp"
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <type_traits>
#include "leaf_hip.h"
#include "leaf_params.hpp"

namespace {

using namespace leaf;                    // the launch structs (leaf_params.hpp); every csrc header reopens this one unnamed namespace

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));   // 16-byte load at 4-byte alignment

constexpr float kPooledFloor = 1e-5f;    // frontend.py:84
// frontend.py:84 is torch.maximum(pooled, 1e-5): NaN propagates (fmaxf would return the floor instead).
__device__ __forceinline__ float pooled_floor(float v) { return v < kPooledFloor ? kPooledFloor : v; }
// bfloat16 I/O (LEAF_FLAG_IO_BF16): widening is exact (the 16 bits are the float's upper half); narrowing rounds to nearest even,
// NaN to the quiet NaN torch's conversion gives.  Arithmetic stays fp32 everywhere.
__device__ __forceinline__ float bf16_widen(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned short bf16_round(float v) {
    const unsigned u = __float_as_uint(v);
    return v != v ? (unsigned short)0x7fc0u : (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
// Sample type of a waveform buffer, carried in the parameter structs' `io_bf16` field (the name predates 16-bit PCM): 0 fp32,
// 1 bfloat16 (LEAF_FLAG_IO_BF16), 2 16-bit PCM (LEAF_FLAG_X_PCM16).  A PCM sample v means v / 32768: the int -> float conversion and
// the scaling by a power of two are both exact, so the result is bit for bit what a caller's float(v) / 32768 holds.
// The FEATURE type (out of the forward, grad_out of the backward) is a second, independent type: float32 or bfloat16
// (LEAF_FLAG_OUT_BF16; LEAF_FLAG_IO_BF16 sets both), carried as bit 2 of the kernels' `mode` -- stored through io_store / bf16_round,
// read through io_load.
constexpr int kSampleF32 = 0, kSampleBf16 = 1, kSamplePcm16 = 2;
__device__ __forceinline__ float pcm16_widen(short v) { return (float)(int)v * 0x1p-15f; }
// element i of an I/O buffer of sample type `st` (one of the three codes above, nothing else: a mode bit is mapped by the caller)
__device__ __forceinline__ float io_load(const void* p, size_t i, int st) {
    if (st == kSampleBf16) return bf16_widen(static_cast<const unsigned short*>(p)[i]);
    if (st == kSamplePcm16) return pcm16_widen(static_cast<const short*>(p)[i]);
    return static_cast<const float*>(p)[i];
}
// Waveform mixup in the load (the reference's training loop, utilities/data/mixup.py: x' = x lam + x[perm] (1 - lam) per clip): a
// mixed sample is rn(rn(x[b][n] lam) + rn(x[perm[b]][n] om)) with om = rn(1 - lam), three separately rounded fp32 operations -- bit for
// bit what the torch expression gives.  The library is compiled with contraction on, so the helper switches it off for its own body
// (a fused multiply-add would round once where the definition rounds twice).  `clip` / `partner`: element offsets of the two rows in
// `x`; `st`: kSampleF32 or kSamplePcm16 (the widened sample v / 32768 is exact; bfloat16 is not mixed).
__device__ __forceinline__ float mix_load(const void* x, size_t clip, size_t partner, size_t i, float lam, float om, int st) {
#pragma clang fp contract(off)
    const float a = io_load(x, clip + i, st) * lam;
    const float b = io_load(x, partner + i, st) * om;
    return a + b;
}
// The per-clip constants of mix_load, read once per (wave, block) where the block's clip index is decoded: wave-uniform, so the
// partner's row offset and the two weights live in SGPRs.  The partner index is clamped into [0, B): a device-side `perm` with an
// out-of-range entry reads a wrong clip, never out of bounds.
struct MixClip {
    size_t partner;         // element offset of row perm[b]
    float lam, om;
};
__device__ __forceinline__ MixClip mix_clip(const int* perm, const float* lam, int b, int B, int T) {
#pragma clang fp contract(off)
    const int bu = __builtin_amdgcn_readfirstlane(b);
    const int pb = __builtin_amdgcn_readfirstlane(min(max(perm[bu], 0), B - 1));
    const float l = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(lam[bu])));
    return MixClip{(size_t)pb * T, l, 1.0f - l};
}
// The kernels' load sites: mixed sample n of the clip at element offset `clip`, zero outside [0, T) for both partners (halo and padding
// as without the mix).  Every lane loads (index clamped into the clip, value zeroed outside it): the loads of a block stay in flight
// together.  ST is a compile-time sample type: the sites branch once per block on the wave-uniform type, not per sample.
template <int ST>
__device__ __forceinline__ float mix_sample(const void* x, size_t clip, const MixClip& mc, int n, int T) {
    const float w = mix_load(x, clip, mc.partner, (size_t)min(max(n, 0), T - 1), mc.lam, mc.om, ST);
    return (n >= 0 && n < T) ? w : 0.0f;
}
__device__ __forceinline__ void io_store(void* p, size_t i, int bf16, float v) {
    if (bf16) static_cast<unsigned short*>(p)[i] = bf16_round(v);
    else static_cast<float*>(p)[i] = v;
}
// Compile-time tuning knobs (tools/ablate.py builds variants of this file with -D...; the product uses the defaults)
#ifndef LEAF_WAVES_PER_WG
#define LEAF_WAVES_PER_WG 8
#endif
#ifndef LEAF_ABLATE
#define LEAF_ABLATE 0                    // bit0 skip epilogue, bit1 skip window staging, bit2 skip partial stores
#endif
#ifndef LEAF_KLOOP_SINGLE_BUFFER_RT
#define LEAF_KLOOP_SINGLE_BUFFER_RT 4    // register tiles with >= this many filter tiles use a single-buffered k-loop
#endif
#ifndef LEAF_TRACE
#define LEAF_TRACE 0                     // tools/trace.py: per-phase s_memtime stamps of block 0 into the workspace tail
#endif
constexpr int kAblate = LEAF_ABLATE;
constexpr int kWavesPerWG = LEAF_WAVES_PER_WG;   // 8 -> 512 threads: 2 waves per SIMD
constexpr int kUB = 5;                   // 16-sample n-blocks per unit (register tile = RT x kUB MFMA tiles x2)
constexpr int kMaxLds = 160 * 1024;

// convolution.py:15-22 -- bounds are built from float32 tensors in the reference.
inline GaborBounds gabor_bounds(int K) {
    const float root = sqrtf(2.0f * logf(2.0f));
    GaborBounds b;
    b.sigma_lo = 4.0f * root / (float)M_PI;
    b.sigma_hi = (float)K * root / (float)M_PI;
    return b;
}

// impulse_responses.py:5-16 -- one complex Gabor tap at integer time t, from the UNclamped parameter.
// Same fp32 operation order as the reference: phase = fl(mu*t); env = exp(fl(1/(2 s^2)) * fl(-t^2)).
__device__ __forceinline__ void gabor_tap(float mu_raw, float sg_raw, GaborBounds bd, float t, float& re, float& im) {
    const float mu = fminf(fmaxf(mu_raw, 0.0f), 3.14159274101257324f);
    const float sg = fminf(fmaxf(sg_raw, bd.sigma_lo), bd.sigma_hi);
    const float norm = 1.0f / (2.50662827463100024f * sg);           // 1/(sqrt(2 pi) sigma)
    const float a = 1.0f / (2.0f * (sg * sg));
    const float env = expf(a * (-(t * t)));
    float s, c;
    sincosf(mu * t, &s, &c);
    re = (norm * c) * env;
    im = (norm * s) * env;
}

// impulse_responses.py:74-80
__device__ __forceinline__ float pool_sigma(float w_raw, int K) { return fminf(fmaxf(w_raw, 2.0f / (float)K), 0.5f); }

}  // namespace
