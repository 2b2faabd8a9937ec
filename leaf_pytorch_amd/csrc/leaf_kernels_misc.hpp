// leaf_kernels_misc.hpp -- kernels on the waveform itself: the stand-alone mixup, the widening copy of a 16-bit waveform
// Included by leaf_kernels.hip only: kernels (see leaf_kernels_tables.hpp).
#pragma once
#include "leaf_common.hpp"

namespace {

// The stand-alone mix (leaf_mixup_f32): out[b][n] = the mixed sample, fp32, read two rows / write one.  Grid B * tiles, tiles = ceil(T / 1024):
// a workgroup mixes 1024 samples of one clip.
__global__ __launch_bounds__(256) void mixup_kernel(const void* __restrict__ x, int st, int B, int T, int tiles, const int* __restrict__ perm,
                                                    const float* __restrict__ lam, float* __restrict__ out) {
    const int b = blockIdx.x / tiles;
    const MixClip mc = mix_clip(perm, lam, b, B, T);
    const size_t row = (size_t)b * T;
    const int n0 = (blockIdx.x - b * tiles) * 1024 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 256 * j;
        if (n < T) out[row + n] = st == kSamplePcm16 ? mix_load(x, row, mc.partner, n, mc.lam, mc.om, kSamplePcm16)
                                                     : mix_load(x, row, mc.partner, n, mc.lam, mc.om, kSampleF32);
    }
}

// 16-bit waveform (bfloat16 or PCM, `st`: kSampleBf16 / kSamplePcm16) -> fp32 copy in the workspace, for the backward families that
// read x as fp32 only (run-time-geometry 2048-sample kernels, MFMA, staged)
__global__ void x16_widen_kernel(const unsigned short* __restrict__ src, int st, size_t n, float* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = st == kSamplePcm16 ? pcm16_widen((short)src[i]) : bf16_widen(src[i]);
}

// n words <- 0: what leaf_backward_head_f32 launches in place of its hipMemsetAsync while the stream is being captured (a captured
// memset node was seen to write other bytes than zeros from the second replay of its graph on)
__global__ void zero_words_kernel(unsigned* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = 0u;
}

}  // namespace
