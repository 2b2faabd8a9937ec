// leaf_clips.hpp -- batch assembly from a packed sample store (leaf_assemble_clips_f32): per-clip pad, crop, gain, peak
// normalisation and time masks in one launch.  Included by inst_clips.hip only: kernels and their parameter structs (gfx950 only).
//
// Reference arithmetic being replaced (utilities/data/raw_transforms.py, per clip on the CPU there): PadToSize (torch: F.pad
// 'replicate' / constant signal.min(); numpy: np.pad 'wrap'), RandomCrop / CenterCrop, RandomGain, PeakNormalization
// (only_too_loud_sounds), TimeMasking -- in the order of get_raw_transforms_v2.  The contract is in include/leaf_hip.h.
//
// Shape of the kernel.  One workgroup of 1024 lanes per clip (256 clips fill the 256 CUs); a gather, a max reduction, and a min
// reduction for the clips that pad with their recording's minimum (the whole recording is then shorter than the clip).  Every
// decision that selects a path -- the store's sample type (a template argument), the pad mode, whether the min pass runs, resident
// or re-reading -- is uniform over the workgroup.  No scratch, no atomics, nothing shared between workgroups.
//
//   * The output row is walked in 16-byte chunks ALIGNED IN `out`: a row starts 4 * S * b bytes behind `out`, so its first
//     `shift` = (address / 4) mod 4 elements' worth of the first chunk belong to the row before it.  Chunk q holds the row's
//     elements 4 q - shift .. 4 q - shift + 3; whole chunks are stored as one float4, the (at most two) partial ones element-wise.
//   * A chunk whose four source samples are contiguous inside the recording is read with ONE load at element alignment (16 bytes
//     at 4-byte alignment for a float32 store, 8 bytes at 2-byte alignment for int16: `rec_off`, `start` and the left pad are
//     arbitrary, so the source cannot be aligned together with the destination; gfx950 global loads take any alignment).  Every
//     lane issues that load for every chunk of its tile, moved inside the recording where the chunk is not: straight-line code,
//     so a tile's loads are in flight together.  A chunk that touches the padded margins or the row's ends is then redone element
//     by element through the pad rule (a few lanes per clip).
//   * RESIDENT path, S <= kClipResidentMax = 8 * 4 * 1024 - 3 = 32 765 samples (two seconds at 16 kHz): the clip's chunks stay
//     in registers (eight float4 per lane; the 3 covers the worst `shift`) between the peak reduction and the store, so the store
//     is read once.  A longer clip takes the RE-READING path: one pass for the peak, a second that gathers again (from L2 where
//     the clip fits) and stores -- slower, any 1 <= S < 2^31.  Without `normalize` the first pass is skipped.
//   * One workgroup per clip also for long clips: B = 8 clips of five seconds use 8 CUs.  Splitting a clip over workgroups would
//     need a second launch for the peak and is not built.
//
// Memory safety: the plan is device memory the host never sees, so the kernel clamps it (rec_off into [0, store_len], rec_len
// into [0, store_len - rec_off], start into [0, max(L, S) - S], an unknown pad mode to 0): no plan reads outside the store or
// writes outside out[b].
//
// The noise instances (leaf_assemble_clips_noise_f32: assemble_clips_noise_kernel<PCM, NOISE, GAUSS>).  AddRandomNoise mixes a second recording, taken
// through the same pad-and-crop rule by a ClipView of its own, in front of the gain: rn(rn(c v) + rn(c' n)); AddGaussianNoise adds
// rn(a z) behind the gain, z from the counter-based stream below.  Both are per-chunk steps on the registers of the tile: a noise
// chunk, or a group of normals, is consumed into v[u] before the next one is produced, so the resident path keeps its eight chunks
// (kClipNoiseResidentMax = kClipResidentMax).  Neither may contract into an fma (clip_mix / clip_add_scaled switch contraction off
// as mix_load does).  The re-reading path computes both twice, from the same inputs by the same code: the same bits.
//
// The stream: z[b][t] is a function of (seed, stream[b], t) alone.  Philox4x32-10, key = the seed's two halves, counter =
// (t >> 2, 0, stream[b]'s two halves); its four words give the normals of row elements 4 g .. 4 g + 3 by Box-Muller in fp32
// (gauss_pair).  The chunk grid is aligned in `out`, not in the row: a chunk at shift != 0 straddles the groups q - 1 and q and
// takes its normals from two Philox calls, evaluating only the pairs it uses (the shift is uniform over the workgroup).
//
// The two plain instances keep the kernel text they had (assemble_clips_kernel below, untouched: the same instructions as before the
// noise instances existed); assemble_clips_noise_kernel restates the body over clip_view / clip_min_pass.
//
// Whole-recording evaluation (leaf_clip_peaks_f32, leaf_assemble_segments_f32) is at the end of the file: the recordings' peaks in
// wave-sized tiles, and rows cut from a recording by a window that may begin before it or end behind it, split over workgroups.
// Their clamped plan is leaf_segments_view.hpp (host and device).
//
// Waveform standardisation (leaf_clip_moments_f32, leaf_assemble_clips_std_f32, leaf_assemble_segments_std_f32): the recordings'
// mean / std / min / max, reduced in float64 in an order the recording's length fixes (at the end of the file), and instances of the
// assembly kernels that map every sample of the clip's recording to (v - mean) / (std + 1e-9f) where it leaves its load
// (clip_standardize: a subtraction and a true division, STD = true in clip_sample / clip_chunk_gather / clip_tile_load).  The plain
// and the noise instances are the STD = false instantiations of the same functions: their instructions are what they were.
//
// The plan itself (leaf_draw_clip_plan) is drawn by draw_clip_plan_kernel at the end of the file: one workgroup, a clip per lane, the
// per-clip arithmetic of leaf_clip_draws.hpp (host and device) from a counter the kernel keeps in device memory.  Mixup's permutation
// and weights (leaf_draw_mixup) are drawn the same way by draw_mixup_kernel behind it, on the arithmetic of leaf_mix_draws.hpp.
#pragma once
#include "leaf_common.hpp"
#include "leaf_segments_view.hpp"
#include "leaf_clip_draws.hpp"
#include "leaf_mix_draws.hpp"

namespace {

constexpr int kClipThreads = 1024;
constexpr int kClipChunks = 8;                                            // float4 chunks a lane keeps on the resident path
constexpr int kClipResidentMax = kClipChunks * 4 * kClipThreads - 3;     // 32 765: the cut-over to the re-reading path

constexpr int kClipNoiseChunks = 8;                                       // ... and what a noise instance keeps
constexpr int kClipNoiseResidentMax = kClipNoiseChunks * 4 * kClipThreads - 3;   // 32 765: the noise instances' cut-over

typedef short s16x4u __attribute__((ext_vector_type(4), aligned(2)));    // 8-byte load at 2-byte alignment

struct ClipParams {
    const void* store;            // float32 or int16 samples
    long long store_len;
    const long long* rec_off;     // [B]
    const int *rec_len, *start, *pad_mode;   // [B]
    const float* gain;            // [B] or null
    const int* masks;             // [B][M][2] or null
    float* out;                   // [B][S]
    int S, M, normalize;
};

// One clip's clamped plan (uniform over the workgroup).
struct ClipView {
    long long off;                // first sample in the store: of the recording, or of the cropped window when the recording is longer
    int L, left, mode;            // samples behind `off` (at most S), left pad, pad mode (0 when L == 0)
    float padv;                   // the constant outside the recording: 0, or min(r) for mode 1
    float g;
    bool has_gain;
};

// The noise transforms of leaf_assemble_clips_noise_f32 (a second kernel argument: the plain instances do not carry it)
struct ClipNoiseParams {
    const void* store;            // the noise recordings, of the clip store's sample type; null: no clip is mixed
    long long store_len;
    const long long* rec_off;     // [B]
    const int *rec_len, *start, *pad_mode;   // [B]
    const float* coeff;           // [B][2]: c, c'
    const float* amp;             // [B] Gaussian amplitudes, or null
    const long long* stream;      // [B]
    unsigned long long seed;
};

// ... and one clip's share of it (uniform over the workgroup)
struct ClipNoiseView {
    ClipView n;                   // the noise recording, clamped as the clip's; L == 0: the clip is not mixed
    float c, cn;
    float amp;                    // 0: no Gaussian noise
    unsigned k0, k1, s0, s1;      // Philox key (the seed) and counter words 2, 3 (the clip's stream)
};

template <bool PCM> __device__ __forceinline__ float clip_load(const void* store, long long i) {
    if constexpr (PCM) return pcm16_widen(static_cast<const short*>(store)[i]);
    else return static_cast<const float*>(store)[i];
}

// The standardising instances (leaf_assemble_clips_std_f32, leaf_assemble_segments_std_f32): one clip's or row's share of
// moments[R][4] (uniform over the workgroup) and the map y = (v - mean) / d, d = std + 1e-9f, applied where a sample of the
// recording leaves a load.  Two correctly rounded fp32 operations, a true division: no reciprocal, no contraction, nothing of
// leaf_fastmath.hpp -- the bits of torch's (r - mean) / (std + 1e-9) in float32.
struct ClipStd {
    float mean, d;
};

__device__ __forceinline__ float clip_standardize(float v, const ClipStd& s) {
#pragma clang fp contract(off)
    return __fdiv_rn(__fsub_rn(v, s.mean), s.d);
}

template <bool PCM, bool STD> __device__ __forceinline__ float clip_load_std(const void* store, long long i, const ClipStd* sd) {
    if constexpr (STD) return clip_standardize(clip_load<PCM>(store, i), *sd);
    else return clip_load<PCM>(store, i);
}

// max or min over the workgroup (every lane calls it; `red` is free again on return)
template <bool MIN> __device__ __forceinline__ float clip_block_reduce(float m, float* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = MIN ? fminf(m, __shfl_xor(m, off)) : fmaxf(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < kClipThreads / 64; ++w) r = MIN ? fminf(r, red[w]) : fmaxf(r, red[w]);
    __syncthreads();
    return r;
}

// element t of the padded, cropped clip (0 <= t < S) before the gain.  I: int on the resident path, long long on the other one.
// STD: the recording's samples are standardised (`padv` is not: the caller sets it in the standardised scale).
template <bool PCM, class I, bool STD = false>
__device__ __forceinline__ float clip_sample(const void* store, const ClipView& c, I t, const ClipStd* sd = nullptr) {
    const I j = t - (I)c.left;
    if (j >= 0 && j < (I)c.L) return clip_load_std<PCM, STD>(store, c.off + j, sd);
    if (c.mode == 2) return clip_load_std<PCM, STD>(store, c.off + (j < 0 ? 0 : c.L - 1), sd);
    if (c.mode == 3) {
        int m = (int)(j % (I)c.L);                                        // floor modulus: periodic over any number of periods
        if (m < 0) m += c.L;
        return clip_load_std<PCM, STD>(store, c.off + m, sd);
    }
    return c.padv;
}

// The four source samples of the chunk at row elements t0 .. t0 + 3 in ONE load, issued by every lane whether its chunk can use it or
// not (straight-line code: the loads of a tile are all in flight before the first is waited for).  The load is moved inside the
// recording (L >= 4); `exact` says whether it sits where the chunk's samples are, i.e. the chunk is whole and needs no padding.
template <bool PCM, class I> __device__ __forceinline__ bool clip_chunk_load(const void* store, const ClipView& c, int S, I t0, float (&v)[4]) {
    const I j0 = t0 - (I)c.left, top = (I)c.L - 4;
    const I jc = j0 < 0 ? 0 : (j0 > top ? top : j0);
    if constexpr (PCM) {
        const s16x4u s = *reinterpret_cast<const s16x4u*>(static_cast<const short*>(store) + (c.off + jc));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = pcm16_widen(s[e]);
    } else {
        const f32x4u s = *reinterpret_cast<const f32x4u*>(static_cast<const float*>(store) + (c.off + jc));
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = s[e];
    }
    return jc == j0 && t0 >= 0 && t0 <= (I)S - 4;
}

// ... and the chunks that load does not serve (the padded margins, the row's two ends, recordings below four samples): element by
// element through the pad rule; elements outside [0, S) come back as 0 (they leave the peak alone and are not stored)
template <bool PCM, class I, bool STD = false>
__device__ __forceinline__ void clip_chunk_gather(const void* store, const ClipView& c, int S, I t0, float (&v)[4], const ClipStd* sd = nullptr) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const I t = t0 + e;
        v[e] = (t >= 0 && t < (I)S) ? clip_sample<PCM, I, STD>(store, c, t, sd) : 0.0f;
    }
}

__device__ __forceinline__ float clip_chunk_peak(float m, const float (&v)[4]) {
    return fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
}

// one mask span as the half-open range [lo, hi) of row elements it zeroes (empty when n <= 0)
__device__ __forceinline__ void clip_mask_span(const int* masks, size_t span, int S, long long& lo, long long& hi) {
    const long long t0 = masks[2 * span], n = masks[2 * span + 1];
    lo = t0 > 0 ? t0 : 0;
    hi = n > 0 ? (t0 + n < S ? t0 + n : S) : lo;
}

template <class I> __device__ __forceinline__ void clip_chunk_store(float* ob, int S, I t0, const float (&v)[4]) {
    if (t0 >= 0 && t0 <= (I)S - 4) {
        *reinterpret_cast<f32x4*>(ob + t0) = f32x4{v[0], v[1], v[2], v[3]};   // 16-byte aligned by the chunk grid
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const I t = t0 + e;
            if (t >= 0 && t < (I)S) ob[t] = v[e];
        }
    }
}

// ---- the random stream (include/leaf_hip.h: leaf_gaussian_noise_f32) ---------------------------------------------------------------
// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped between them
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// Two normals from two words: u1 = ((ra >> 8) + 1) 2^-24 in (0, 1], u2 = (rb >> 8) 2^-24 in [0, 1) -- both exact in fp32 --
// rho = sqrt(-2 ln u1), (zc, zs) = rho (cos, sin)(2 pi u2).  The angle goes in as 2 u2 (exact) through sincospi: no rounded 2 pi u2.
// Contraction is off so that every kernel this is inlined into gives the same bits.
__device__ __forceinline__ void gauss_pair(unsigned ra, unsigned rb, float& zc, float& zs) {
#pragma clang fp contract(off)
    const float u1 = (float)((ra >> 8) + 1u) * 0x1p-24f;
    const float rho = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif((float)(rb >> 8) * 0x1p-23f, &sn, &cs);
    zc = rho * cs;
    zs = rho * sn;
}

// the four normals of the row elements 4 g .. 4 g + 3
__device__ __forceinline__ void gauss_group(unsigned k0, unsigned k1, unsigned s0, unsigned s1, unsigned g, float (&z)[4]) {
    unsigned r[4];
    philox4x32_10(g, 0u, s0, s1, k0, k1, r);
    gauss_pair(r[0], r[1], z[0], z[1]);
    gauss_pair(r[2], r[3], z[2], z[3]);
}

// rn(rn(v c) + rn(n cn)): AddRandomNoise's `coeff * x + (1.0 - coeff) * noise`, three separately rounded operations
__device__ __forceinline__ float clip_mix(float v, float c, float n, float cn) {
#pragma clang fp contract(off)
    const float a = v * c;
    const float b = n * cn;
    return a + b;
}

// rn(y + rn(a z)): AddGaussianNoise's `x + amplitude * noise`
__device__ __forceinline__ float clip_add_scaled(float y, float a, float z) {
#pragma clang fp contract(off)
    const float w = a * z;
    return y + w;
}

// The noise recording's samples of the chunk at row elements t0 .. t0 + 3, mixed into v.  (Elements outside the row: both sides are 0.)
template <bool PCM, class I> __device__ __forceinline__ void clip_chunk_mix(const void* nstore, const ClipNoiseView& a, int S, I t0, float (&v)[4]) {
    float n[4];
    bool exact = false;
    if (a.n.L >= 4) exact = clip_chunk_load<PCM, I>(nstore, a.n, S, t0, n);
    if (!exact) clip_chunk_gather<PCM, I>(nstore, a.n, S, t0, n);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = clip_mix(v[e], a.c, n[e], a.cn);
}

// The normals of chunk q (row elements 4 q - shift ..), scaled and added to v.  The chunk's elements are the entries 4 - shift ..
// 7 - shift of the eight normals of the groups q - 1 (words ra) and q (words rb).  An even shift keeps Box-Muller's pairs together
// (two evaluations); an odd one takes the sine of one pair, a whole pair and the cosine of a third.  The shift is uniform over the
// workgroup, so the words are picked by scalar conditions and the third evaluation sits in a uniform branch.  Elements outside the
// row stay as they are: zeros that must leave the peak alone.
template <class I> __device__ __forceinline__ void clip_chunk_gauss(const ClipNoiseView& a, int S, I q, int shift, float (&v)[4]) {
    unsigned ra[4] = {0u, 0u, 0u, 0u}, rb[4];
    philox4x32_10((unsigned)q, 0u, a.s0, a.s1, a.k0, a.k1, rb);
    if (shift != 0) philox4x32_10((unsigned)(q - 1), 0u, a.s0, a.s1, a.k0, a.k1, ra);   // (q == 0: its elements lie in front of the row)
    const bool s0 = shift == 0, s3 = shift == 3, odd = (shift & 1) != 0;
    float c1, n1, c2, n2, z[4];
    gauss_pair(s0 ? rb[0] : (s3 ? ra[0] : ra[2]), s0 ? rb[1] : (s3 ? ra[1] : ra[3]), c1, n1);
    gauss_pair(s0 ? rb[2] : (s3 ? ra[2] : rb[0]), s0 ? rb[3] : (s3 ? ra[3] : rb[1]), c2, n2);
    if (odd) {
        float c3, n3;
        gauss_pair(s3 ? rb[0] : rb[2], s3 ? rb[1] : rb[3], c3, n3);
        z[0] = n1; z[1] = c2; z[2] = n2; z[3] = c3;
    } else {
        z[0] = c1; z[1] = n1; z[2] = c2; z[3] = n2;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const I t = 4 * q - shift + e;
        if (t >= 0 && t < (I)S) v[e] = clip_add_scaled(v[e], a.amp, z[e]);
    }
}

// A lane's tile: the chunks q0, q0 + 1024, ... (U of them), gathered and multiplied by the gain; the lane's share of the peak comes
// back.  Chunks behind the row are zeros.  NOISE / GAUSS: the two noise steps, around the gain, chunk by chunk.  STD: the clip's
// samples are standardised as they arrive -- a whole chunk here, the others inside the pad rule; the noise recording is not.
template <bool PCM, class I, int U, bool NOISE = false, bool GAUSS = false, bool STD = false>
__device__ __forceinline__ float clip_tile_load(const void* store, const ClipView& c, int S, int shift, I q0, I nchunks, float (&v)[U][4],
                                                const void* nstore = nullptr, const ClipNoiseView* a = nullptr, const ClipStd* sd = nullptr) {
    bool exact[U];
    if (c.L >= 4) {
#pragma unroll
        for (int u = 0; u < U; ++u) exact[u] = clip_chunk_load<PCM, I>(store, c, S, 4 * (q0 + (I)u * kClipThreads) - shift, v[u]);
    } else {
#pragma unroll
        for (int u = 0; u < U; ++u) exact[u] = false;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const I q = q0 + (I)u * kClipThreads;
        if (q >= nchunks) v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0.0f;
        else if (!exact[u]) clip_chunk_gather<PCM, I, STD>(store, c, S, 4 * q - shift, v[u], sd);
        else if constexpr (STD) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = clip_standardize(v[u][e], *sd);
        }
    }
    float m = 0.0f;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if constexpr (NOISE) {
            const I q = q0 + (I)u * kClipThreads;
            if (a->n.L > 0 && q < nchunks) clip_chunk_mix<PCM, I>(nstore, *a, S, 4 * q - shift, v[u]);
        }
        if (c.has_gain) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = v[u][e] * c.g;
        }
        if constexpr (GAUSS) {
            const I q = q0 + (I)u * kClipThreads;
            if (a->amp != 0.0f && q < nchunks) clip_chunk_gauss<I>(*a, S, q, shift, v[u]);
        }
        m = clip_chunk_peak(m, v[u]);
    }
    return m;
}

// ... and its second half: the scale of the clip's peak (0 when the call does not normalise), the masks, the stores
template <class I, int U>
__device__ __forceinline__ void clip_tile_finish(const ClipParams& p, int b, int shift, I q0, I nchunks, float peak, float (&v)[U][4], float* ob) {
    const float scale = peak > 1.0f ? 1.0f / peak : 1.0f;                 // the arithmetic of peak_normalize_kernel
    if (peak > 1.0f) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) v[u][e] = v[u][e] * scale;
    }
    for (int s = 0; s < p.M; ++s) {
        long long lo, hi;
        clip_mask_span(p.masks, (size_t)b * p.M + s, p.S, lo, hi);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const I t0 = 4 * (q0 + (I)u * kClipThreads) - shift;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (t0 + e >= lo && t0 + e < hi) v[u][e] = 0.0f;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const I q = q0 + (I)u * kClipThreads;
        if (q < nchunks) clip_chunk_store<I>(ob, p.S, 4 * q - shift, v[u]);
    }
}

template <bool PCM>
__global__ __launch_bounds__(kClipThreads) void assemble_clips_kernel(const ClipParams p) {
    __shared__ float red[kClipThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, S = p.S;
    float* ob = p.out + (size_t)b * S;

    ClipView c;
    {
        const long long off = p.rec_off[b], room = p.store_len;
        c.off = off < 0 ? 0 : (off > room ? room : off);
        const long long len = p.rec_len[b], most = room - c.off;
        c.L = (int)(len < 0 ? 0 : (len > most ? most : len));
        const int st = p.start[b], mode = p.pad_mode[b];
        if (c.L > S) {                                                    // a crop: the window [start, start + S) of the recording, no padding
            c.off += st < 0 ? 0 : (st > c.L - S ? c.L - S : st);
            c.L = S;
        }                                                                 // (otherwise max(L, S) - S = 0: the only start is 0)
        c.left = (S - c.L) / 2;
        c.mode = (c.L > 0 && mode >= 0 && mode <= 3) ? mode : 0;
        c.padv = 0.0f;
        c.has_gain = p.gain != nullptr;
        c.g = c.has_gain ? p.gain[b] : 1.0f;
    }
    if (c.mode == 1 && c.L < S) {                                         // PadToSize 'constant': the recording's minimum
        float mn = INFINITY;
        for (int i = tid; i < c.L; i += kClipThreads) mn = fminf(mn, clip_load<PCM>(p.store, c.off + i));   // (L < S: i + 1024 fits)
        c.padv = clip_block_reduce<true>(mn, red);
    }
    const int shift = (int)((reinterpret_cast<uintptr_t>(ob) >> 2) & 3);  // row elements the first aligned chunk lacks

    if (S <= kClipResidentMax) {                                          // one tile per lane holds the clip
        const int nchunks = (S + shift + 3) >> 2;
        float v[kClipChunks][4];
        const float m = clip_tile_load<PCM, int, kClipChunks>(p.store, c, S, shift, tid, nchunks, v);
        const float peak = p.normalize ? clip_block_reduce<false>(m, red) : 0.0f;
        clip_tile_finish<int, kClipChunks>(p, b, shift, tid, nchunks, peak, v, ob);
        return;
    }

    constexpr int kU = 4;                                                 // chunks in flight per lane on the re-reading path
    const long long nchunks = ((long long)S + shift + 3) >> 2;
    float peak = 0.0f;
    if (p.normalize) {
        float m = 0.0f;
        for (long long q0 = tid; q0 < nchunks; q0 += kU * kClipThreads) {
            float v[kU][4];
            m = fmaxf(m, clip_tile_load<PCM, long long, kU>(p.store, c, S, shift, q0, nchunks, v));
        }
        peak = clip_block_reduce<false>(m, red);
    }
    for (long long q0 = tid; q0 < nchunks; q0 += kU * kClipThreads) {
        float v[kU][4];
        clip_tile_load<PCM, long long, kU>(p.store, c, S, shift, q0, nchunks, v);
        clip_tile_finish<long long, kU>(p, b, shift, q0, nchunks, peak, v, ob);
    }
}

// One clip's plan, clamped (the header's MEMORY SAFETY rule; the noise recording's plan goes through the same code)
__device__ __forceinline__ ClipView clip_view(const long long* rec_off, const int* rec_len, const int* start, const int* pad_mode,
                                              long long store_len, int b, int S) {
    ClipView c;
    const long long off = rec_off[b], room = store_len;
    c.off = off < 0 ? 0 : (off > room ? room : off);
    const long long len = rec_len[b], most = room - c.off;
    c.L = (int)(len < 0 ? 0 : (len > most ? most : len));
    const int st = start[b], mode = pad_mode[b];
    if (c.L > S) {                                                        // a crop: the window [start, start + S) of the recording, no padding
        c.off += st < 0 ? 0 : (st > c.L - S ? c.L - S : st);
        c.L = S;
    }                                                                     // (otherwise max(L, S) - S = 0: the only start is 0)
    c.left = (S - c.L) / 2;
    c.mode = (c.L > 0 && mode >= 0 && mode <= 3) ? mode : 0;
    c.padv = 0.0f;
    c.has_gain = false;
    c.g = 1.0f;
    return c;
}

// PadToSize 'constant': the recording's minimum, for a recording that is padded in that mode
template <bool PCM> __device__ __forceinline__ void clip_min_pass(const void* store, ClipView& c, int S, float* red) {
    if (c.mode == 1 && c.L < S) {
        float mn = INFINITY;
        for (int i = threadIdx.x; i < c.L; i += kClipThreads) mn = fminf(mn, clip_load<PCM>(store, c.off + i));   // (L < S: i + 1024 fits)
        c.padv = clip_block_reduce<true>(mn, red);
    }
}

// leaf_assemble_clips_noise_f32: the kernel above with one or both noise steps (at least one of NOISE, GAUSS is set)
template <bool PCM, bool NOISE, bool GAUSS>
__global__ __launch_bounds__(kClipThreads) void assemble_clips_noise_kernel(const ClipParams p, const ClipNoiseParams np) {
    __shared__ float red[kClipThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, S = p.S;
    float* ob = p.out + (size_t)b * S;

    ClipView c = clip_view(p.rec_off, p.rec_len, p.start, p.pad_mode, p.store_len, b, S);
    c.has_gain = p.gain != nullptr;
    c.g = c.has_gain ? p.gain[b] : 1.0f;
    clip_min_pass<PCM>(p.store, c, S, red);
    ClipNoiseView a{};
    if constexpr (NOISE) {
        a.n = clip_view(np.rec_off, np.rec_len, np.start, np.pad_mode, np.store_len, b, S);
        a.c = np.coeff[2 * b];
        a.cn = np.coeff[2 * b + 1];
        clip_min_pass<PCM>(np.store, a.n, S, red);
    }
    if constexpr (GAUSS) {
        const unsigned long long st = (unsigned long long)np.stream[b];
        a.amp = np.amp[b];
        a.k0 = (unsigned)np.seed; a.k1 = (unsigned)(np.seed >> 32);
        a.s0 = (unsigned)st; a.s1 = (unsigned)(st >> 32);
    }
    const int shift = (int)((reinterpret_cast<uintptr_t>(ob) >> 2) & 3);  // row elements the first aligned chunk lacks

    constexpr int kResident = kClipNoiseChunks;
    if (S <= kClipNoiseResidentMax) {                          // one tile per lane holds the clip
        const int nchunks = (S + shift + 3) >> 2;
        float v[kResident][4];
        const float m = clip_tile_load<PCM, int, kResident, NOISE, GAUSS>(p.store, c, S, shift, tid, nchunks, v, np.store, &a);
        const float peak = p.normalize ? clip_block_reduce<false>(m, red) : 0.0f;
        clip_tile_finish<int, kResident>(p, b, shift, tid, nchunks, peak, v, ob);
        return;
    }

    constexpr int kU = 4;                                                 // chunks in flight per lane on the re-reading path
    const long long nchunks = ((long long)S + shift + 3) >> 2;
    float peak = 0.0f;
    if (p.normalize) {
        float m = 0.0f;
        for (long long q0 = tid; q0 < nchunks; q0 += kU * kClipThreads) {
            float v[kU][4];
            m = fmaxf(m, clip_tile_load<PCM, long long, kU, NOISE, GAUSS>(p.store, c, S, shift, q0, nchunks, v, np.store, &a));
        }
        peak = clip_block_reduce<false>(m, red);
    }
    for (long long q0 = tid; q0 < nchunks; q0 += kU * kClipThreads) {
        float v[kU][4];
        clip_tile_load<PCM, long long, kU, NOISE, GAUSS>(p.store, c, S, shift, q0, nchunks, v, np.store, &a);
        clip_tile_finish<long long, kU>(p, b, shift, q0, nchunks, peak, v, ob);
    }
}

// The standardising instances (a third kernel argument: neither the plain nor the noise instances carry it)
struct ClipStdParams {
    const float* moments;         // [R][4]: mean, std, min, max of every recording of the store (leaf_clip_moments_f32)
    const int* rec;               // [B] (segments: [rows]): the clip's entry of moments, clamped into [0, R - 1]
    int R;
    int normalize;                // segments only: scale by the standardised recording's peak
};

// the clip's moments: mean and d = std + 1e-9f (one fp32 add per clip); `mo` comes back as the clip's row of moments
__device__ __forceinline__ ClipStd clip_std_view(const ClipStdParams& sp, int b, const float*& mo) {
    mo = sp.moments + 4 * (size_t)segment_peak_index(sp.rec[b], sp.R);
    ClipStd sd;
    sd.mean = mo[0];
    sd.d = __fadd_rn(mo[1], 1e-9f);
    return sd;
}

// leaf_assemble_clips_std_f32: assemble_clips_noise_kernel (any of NOISE, GAUSS, or neither) on the STANDARDISED recording:
// (v - mean_i) / d_i on every sample of the clip's recording as it is loaded, on either path; the 'min' pad value is the
// standardised minimum of the whole recording, from moments (no min pass: the map is monotone); the noise recording stays as it is.
template <bool PCM, bool NOISE, bool GAUSS>
__global__ __launch_bounds__(kClipThreads) void assemble_clips_std_kernel(const ClipParams p, const ClipNoiseParams np, const ClipStdParams sp) {
    __shared__ float red[kClipThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, S = p.S;
    float* ob = p.out + (size_t)b * S;

    ClipView c = clip_view(p.rec_off, p.rec_len, p.start, p.pad_mode, p.store_len, b, S);
    c.has_gain = p.gain != nullptr;
    c.g = c.has_gain ? p.gain[b] : 1.0f;
    const float* mo;
    const ClipStd sd = clip_std_view(sp, b, mo);
    if (c.mode == 1 && c.L < S) c.padv = clip_standardize(mo[2], sd);
    ClipNoiseView a{};
    if constexpr (NOISE) {
        a.n = clip_view(np.rec_off, np.rec_len, np.start, np.pad_mode, np.store_len, b, S);
        a.c = np.coeff[2 * b];
        a.cn = np.coeff[2 * b + 1];
        clip_min_pass<PCM>(np.store, a.n, S, red);
    }
    if constexpr (GAUSS) {
        const unsigned long long st = (unsigned long long)np.stream[b];
        a.amp = np.amp[b];
        a.k0 = (unsigned)np.seed; a.k1 = (unsigned)(np.seed >> 32);
        a.s0 = (unsigned)st; a.s1 = (unsigned)(st >> 32);
    }
    const int shift = (int)((reinterpret_cast<uintptr_t>(ob) >> 2) & 3);  // row elements the first aligned chunk lacks

    constexpr int kResident = kClipNoiseChunks;
    if (S <= kClipNoiseResidentMax) {                                     // one tile per lane holds the clip
        const int nchunks = (S + shift + 3) >> 2;
        float v[kResident][4];
        const float m = clip_tile_load<PCM, int, kResident, NOISE, GAUSS, true>(p.store, c, S, shift, tid, nchunks, v, np.store, &a, &sd);
        const float peak = p.normalize ? clip_block_reduce<false>(m, red) : 0.0f;
        clip_tile_finish<int, kResident>(p, b, shift, tid, nchunks, peak, v, ob);
        return;
    }

    constexpr int kU = 4;                                                 // chunks in flight per lane on the re-reading path
    const long long nchunks = ((long long)S + shift + 3) >> 2;
    float peak = 0.0f;
    if (p.normalize) {
        float m = 0.0f;
        for (long long q0 = tid; q0 < nchunks; q0 += kU * kClipThreads) {
            float v[kU][4];
            m = fmaxf(m, clip_tile_load<PCM, long long, kU, NOISE, GAUSS, true>(p.store, c, S, shift, q0, nchunks, v, np.store, &a, &sd));
        }
        peak = clip_block_reduce<false>(m, red);
    }
    for (long long q0 = tid; q0 < nchunks; q0 += kU * kClipThreads) {
        float v[kU][4];
        clip_tile_load<PCM, long long, kU, NOISE, GAUSS, true>(p.store, c, S, shift, q0, nchunks, v, np.store, &a, &sd);
        clip_tile_finish<long long, kU>(p, b, shift, q0, nchunks, peak, v, ob);
    }
}

// leaf_gaussian_noise_f32: z[b][t] as [B][size], one lane per group of four; grid B * tiles, tiles = ceil(ceil(size / 4) / 256)
__global__ __launch_bounds__(256) void gaussian_noise_kernel(int size, int tiles, unsigned long long seed, const long long* stream, float* out) {
    const int b = blockIdx.x / tiles;
    const unsigned g = (unsigned)(blockIdx.x % tiles) * 256u + threadIdx.x;
    const long long t0 = 4ll * g;
    if (t0 >= size) return;
    const unsigned long long st = (unsigned long long)stream[b];
    float z[4];
    gauss_group((unsigned)seed, (unsigned)(seed >> 32), (unsigned)st, (unsigned)(st >> 32), g, z);
    float* o = out + (size_t)b * size + t0;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (t0 + e < size) o[e] = z[e];
}

// ---- whole-recording evaluation (include/leaf_hip.h: leaf_clip_peaks_f32, leaf_assemble_segments_f32) -------------------------------
// test.py cuts every recording into ceil(L / S) rows of S samples after ONE peak normalisation over the whole recording and a
// 'replicate' padding split left = (P - L) / 2.  Two pieces: the recordings' peaks, once per dataset, and the rows themselves.

// leaf_clip_peaks_f32.  The work unit is a wave and a tile of kPeakTile samples of one recording: a long recording is many tiles
// (spread over the chip), a short one is one wave's reduction of 64 lanes.  Stage 1 (one workgroup) counts each clamped recording's
// tiles into the exclusive prefix `tile_start` and zeroes the peaks; stage 2 gives every wave a contiguous run of tiles -- one
// binary search, then a walk -- and folds a recording's share into peaks[i] with an INTEGER max on the bit pattern, which orders
// non-negative floats as the floats themselves (no float atomic; max is exact in any order).
constexpr int kPeakThreads = 256;
constexpr int kPeakChunks = 4;                                            // loads of four samples a lane has in flight
constexpr int kPeakTile = kPeakChunks * 4 * 64;                           // 1024 samples
constexpr int kPeakMaxBlocks = 2048;                                      // 8 workgroups per CU; the tiles beyond are walked

struct PeakParams {
    const void* store;
    long long store_len;
    const long long* rec_off;     // [R]
    const int* rec_len;           // [R]
    float* peaks;                 // [R]
    long long* tile_start;        // [R + 1] workspace
    int R;
};

__global__ __launch_bounds__(kClipThreads) void clip_peaks_plan_kernel(const PeakParams p) {
    __shared__ long long wsum[kClipThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;                                                  // tiles of the recordings before this round's
    for (long long base = 0; base < p.R; base += kClipThreads) {
        const long long i = base + tid;
        long long n = 0;
        if (i < p.R) {
            n = ((long long)recording_view(p.rec_off[i], p.rec_len[i], p.store_len).L + kPeakTile - 1) / kPeakTile;
            p.peaks[i] = 0.0f;
        }
        long long s = n;                                                  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(s, d);
            if (lane >= d) s += o;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kClipThreads / 64; ++w) {
            const long long x = wsum[w];
            if (w < wave) before += x;
            total += x;
        }
        if (i < p.R) p.tile_start[i] = carry + before + s - n;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) p.tile_start[p.R] = carry;
}

template <bool PCM>
__global__ __launch_bounds__(kPeakThreads) void clip_peaks_kernel(const PeakParams p) {
    const int lane = threadIdx.x & 63;
    const long long total = p.tile_start[p.R];
    const long long waves = (long long)gridDim.x * (kPeakThreads / 64), w = (long long)blockIdx.x * (kPeakThreads / 64) + (threadIdx.x >> 6);
    const long long per = (total + waves - 1) / waves;
    long long t = w * per;                                                // this wave's tiles: [t, end)
    const long long end = t + per < total ? t + per : total;
    if (t >= end) return;
    int i = 0;                                                            // the LAST i with tile_start[i] <= t: the recording tile t belongs to
    for (int hi = p.R; hi - i > 1;) {                                     // tile_start[i] <= t < tile_start[hi]
        const int mid = i + (hi - i) / 2;
        if (p.tile_start[mid] <= t) i = mid; else hi = mid;
    }
    while (t < end) {
        const long long first = p.tile_start[i], next = p.tile_start[i + 1];   // first <= t < next
        const long long stop = next < end ? next : end;
        const SegmentView r = recording_view(p.rec_off[i], p.rec_len[i], p.store_len);
        float m = 0.0f;
        for (; t < stop; ++t) {
            const long long j0 = (t - first) * kPeakTile + 4 * lane;
            float v[kPeakChunks][4];
#pragma unroll
            for (int u = 0; u < kPeakChunks; ++u) {
                const long long j = j0 + u * (4 * 64);
                if (j + 4 <= r.L) {                                      // one load at element alignment, as clip_chunk_load
                    if constexpr (PCM) {
                        const s16x4u s = *reinterpret_cast<const s16x4u*>(static_cast<const short*>(p.store) + (r.off + j));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[u][e] = pcm16_widen(s[e]);
                    } else {
                        const f32x4u s = *reinterpret_cast<const f32x4u*>(static_cast<const float*>(p.store) + (r.off + j));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[u][e] = s[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[u][e] = j + e < r.L ? clip_load<PCM>(p.store, r.off + j + e) : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < kPeakChunks; ++u) m = clip_chunk_peak(m, v[u]);   // (fmaxf: a NaN sample is ignored)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
        if (lane == 0 && m > 0.0f) atomicMax(reinterpret_cast<unsigned*>(p.peaks + i), __float_as_uint(m));
        if (t < end)                                                      // t == next: the following recording that has a tile
            do ++i; while (p.tile_start[i + 1] <= t);
    }
}

// leaf_assemble_segments_f32.  Nothing is reduced, so a row is split freely: grid = rows x tiles, a tile the eight chunks per lane
// of the resident path above, on the same chunk grid aligned in `out` and through the same loads.  The row is a ClipView in
// 'replicate' mode whose `left` is minus the (clamped) window start; all row indices are 64-bit.
struct SegmentParams {
    const void* store;
    long long store_len;
    const long long* rec_off;     // [rows]
    const int* rec_len;           // [rows]
    const long long* win;         // [rows]
    const float* peaks;           // [R] or null
    const int* rec;               // [rows]
    float* out;                   // [rows][S]
    int R, S, tiles;
};

template <bool PCM>
__global__ __launch_bounds__(kClipThreads) void assemble_segments_kernel(const SegmentParams p) {
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles, S = p.S;
    float* ob = p.out + (size_t)b * S;
    const SegmentView sv = segment_view(p.rec_off[b], p.rec_len[b], p.win[b], p.store_len, S);
    ClipView c;
    c.off = sv.off; c.L = sv.L; c.left = sv.left;
    c.mode = sv.L > 0 ? 2 : 0;                                            // no samples: zeros
    c.padv = 0.0f; c.has_gain = false; c.g = 1.0f;
    const float peak = p.peaks ? p.peaks[segment_peak_index(p.rec[b], p.R)] : 0.0f;   // the RECORDING's peak, not the row's
    const int shift = (int)((reinterpret_cast<uintptr_t>(ob) >> 2) & 3);  // row elements the first aligned chunk lacks
    const long long nchunks = ((long long)S + shift + 3) >> 2;
    const long long q0 = (long long)tile * (kClipChunks * kClipThreads) + threadIdx.x;
    if (q0 >= nchunks) return;                                            // (no barrier in this kernel)
    ClipParams cp{};                                                      // what clip_tile_finish reads: the row size, no masks
    cp.S = S;
    float v[kClipChunks][4];
    clip_tile_load<PCM, long long, kClipChunks>(p.store, c, S, shift, q0, nchunks, v);
    clip_tile_finish<long long, kClipChunks>(cp, b, shift, q0, nchunks, peak, v, ob);
}

// leaf_assemble_segments_std_f32: the rows of the STANDARDISED recording.  The recording's peak needs no pass over it: the map is
// monotone in fp32 (a correctly rounded subtraction, a correctly rounded division by d > 0), so max |y| is taken at min or at max.
template <bool PCM>
__global__ __launch_bounds__(kClipThreads) void assemble_segments_std_kernel(const SegmentParams p, const ClipStdParams sp) {
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles, S = p.S;
    float* ob = p.out + (size_t)b * S;
    const SegmentView sv = segment_view(p.rec_off[b], p.rec_len[b], p.win[b], p.store_len, S);
    ClipView c;
    c.off = sv.off; c.L = sv.L; c.left = sv.left;
    c.mode = sv.L > 0 ? 2 : 0;                                            // no samples: zeros
    c.padv = 0.0f; c.has_gain = false; c.g = 1.0f;
    const float* mo;
    const ClipStd sd = clip_std_view(sp, b, mo);
    const float peak = sp.normalize ? fmaxf(fabsf(clip_standardize(mo[2], sd)), fabsf(clip_standardize(mo[3], sd))) : 0.0f;
    const int shift = (int)((reinterpret_cast<uintptr_t>(ob) >> 2) & 3);  // row elements the first aligned chunk lacks
    const long long nchunks = ((long long)S + shift + 3) >> 2;
    const long long q0 = (long long)tile * (kClipChunks * kClipThreads) + threadIdx.x;
    if (q0 >= nchunks) return;                                            // (no barrier in this kernel)
    ClipParams cp{};                                                      // what clip_tile_finish reads: the row size, no masks
    cp.S = S;
    float v[kClipChunks][4];
    clip_tile_load<PCM, long long, kClipChunks, false, false, true>(p.store, c, S, shift, q0, nchunks, v, nullptr, nullptr, &sd);
    clip_tile_finish<long long, kClipChunks>(cp, b, shift, q0, nchunks, peak, v, ob);
}

// ---- the recordings' moments (include/leaf_hip.h: leaf_clip_moments_f32) -------------------------------------------------------------
// mean, std (unbiased), min and max of every recording, the reductions in float64 and in an order that the recording's length
// alone fixes.  The work unit is a wave and one SPAN of one recording (leaf_segments_view.hpp: moment_span -- up to kMomentSpans
// spans of whole 1024-sample tiles): a long recording is 32 waves' work, a short one a single tile's.  A lane adds its samples in
// index order (the tile layout of clip_peaks_kernel: four chunks of four per lane and tile), the 64 lanes are folded by a butterfly
// (a + b on both sides: the same bits in every lane), and the span's partial goes to its own slot of the workspace.  A second kernel
// folds a recording's 32 slots in slot order.  Two such passes: sum -> mean (kept in the workspace in float64), then the squared
// deviations from that mean.  No atomics; which wave takes which unit does not enter the result.
struct MomentPartial {
    double sum;                   // of the samples (pass 1), of the squared deviations (pass 2)
    float mn, mx;                 // pass 1 (NaN samples are ignored by fminf / fmaxf; the mean and the std carry them)
};

struct MomentParams {
    const void* store;
    long long store_len;
    const long long* rec_off;     // [R]
    const int* rec_len;           // [R]
    float* moments;               // [R][4]
    MomentPartial* part;          // [R][kMomentSpans] workspace
    double* mean;                 // [R] workspace: the float64 mean before its rounding
    int R;
};

template <bool PCM, bool SQ>
__global__ __launch_bounds__(kPeakThreads) void clip_moments_pass_kernel(const MomentParams p) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (kPeakThreads / 64), units = (long long)p.R * kMomentSpans;
    for (long long unit = (long long)blockIdx.x * (kPeakThreads / 64) + (threadIdx.x >> 6); unit < units; unit += waves) {
        const int i = (int)(unit / kMomentSpans), k = (int)(unit % kMomentSpans);
        const SegmentView r = recording_view(p.rec_off[i], p.rec_len[i], p.store_len);
        const MomentSpan s = moment_span(r.L, k);
        const double m = SQ ? p.mean[i] : 0.0;
        double acc = 0.0;
        float mn = INFINITY, mx = -INFINITY;
        for (long long t0 = s.begin; t0 < s.end; t0 += kMomentTile) {
            float v[kPeakChunks][4];
            int n[kPeakChunks];                                           // the chunk's samples inside the span
#pragma unroll
            for (int u = 0; u < kPeakChunks; ++u) {
                const long long j = t0 + u * (4 * 64) + 4 * lane;
                if (j + 4 <= s.end) {                                     // one load at element alignment, as clip_chunk_load
                    n[u] = 4;
                    if constexpr (PCM) {
                        const s16x4u q = *reinterpret_cast<const s16x4u*>(static_cast<const short*>(p.store) + (r.off + j));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[u][e] = pcm16_widen(q[e]);
                    } else {
                        const f32x4u q = *reinterpret_cast<const f32x4u*>(static_cast<const float*>(p.store) + (r.off + j));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[u][e] = q[e];
                    }
                } else {
                    n[u] = j < s.end ? (int)(s.end - j) : 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[u][e] = e < n[u] ? clip_load<PCM>(p.store, r.off + j + e) : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < kPeakChunks; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (e < n[u]) {
                        if constexpr (SQ) {
                            const double dv = (double)v[u][e] - m;
                            acc += dv * dv;                               // (contraction would only drop a float64 rounding; the order stays)
                        } else {
                            acc += (double)v[u][e];
                            mn = fminf(mn, v[u][e]);
                            mx = fmaxf(mx, v[u][e]);
                        }
                    }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            acc += __shfl_xor(acc, off);
            if constexpr (!SQ) {
                mn = fminf(mn, __shfl_xor(mn, off));
                mx = fmaxf(mx, __shfl_xor(mx, off));
            }
        }
        if (lane == 0) {
            p.part[unit].sum = acc;
            if constexpr (!SQ) { p.part[unit].mn = mn; p.part[unit].mx = mx; }
        }
    }
}

// ... and the fold of a recording's slots, one lane per recording.  SQ = false: mean (float64 to the workspace, rounded once to
// moments[i][0]), min, max; SQ = true: std = sqrt(sum / (L - 1)) in float64, rounded once.  L == 1: 0 / 0 = NaN, as torch's unbiased
// std; L == 0: (0, NaN, 0, 0).
template <bool SQ>
__global__ __launch_bounds__(kPeakThreads) void clip_moments_fold_kernel(const MomentParams p) {
    const long long i = (long long)blockIdx.x * kPeakThreads + threadIdx.x;
    if (i >= p.R) return;
    const int L = recording_view(p.rec_off[i], p.rec_len[i], p.store_len).L;
    const MomentPartial* part = p.part + i * kMomentSpans;
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    for (int k = 0; k < kMomentSpans; ++k) {
        sum += part[k].sum;
        if constexpr (!SQ) {
            mn = fminf(mn, part[k].mn);
            mx = fmaxf(mx, part[k].mx);
        }
    }
    float* mo = p.moments + 4 * i;
    if constexpr (SQ) {
        mo[1] = L > 0 ? (float)sqrt(sum / (double)(L - 1)) : __builtin_nanf("");
    } else {
        const double mean = L > 0 ? sum / (double)L : 0.0;
        p.mean[i] = mean;
        mo[0] = (float)mean;
        mo[2] = L > 0 ? mn : 0.0f;
        mo[3] = L > 0 ? mx : 0.0f;
    }
}

// ---- the plan (include/leaf_hip.h: leaf_draw_clip_plan) -------------------------------------------------------------------------------
// ClipSampler's draws on the device: what the assembly kernels above take as their plan, written by ONE workgroup whose lanes stride
// over the clips.  Nothing is reduced and nothing is shared but the step counter: every lane reads it, a barrier follows, and lane 0
// alone stores step + 1 behind it (one workgroup: no other reader exists).  A draw is a function of (seed, id, counter word) --
// leaf_clip_draws.hpp -- so which lane takes which clip does not enter it.  What the kernel cannot see it clamps: index / order
// entries into [0, R); the lengths it reads go out as they are (the assembly kernels clamp them) and only count as max(L - S, 0).
// The arguments (DrawParams) and one clip's reads, draws and stores (draw_plan_clip) are in leaf_clip_draws.hpp, for the host too.
constexpr int kDrawThreads = 256;

__global__ __launch_bounds__(kDrawThreads) void draw_clip_plan_kernel(const DrawParams p) {
    const unsigned long long step = p.state[0];
    __syncthreads();
    if (threadIdx.x == 0 && p.advance) p.state[0] = step + 1ull;
    for (int b = threadIdx.x; b < p.B; b += kDrawThreads) draw_plan_clip(p, step, b);
}

// ---- mixup's draws (include/leaf_hip.h: leaf_draw_mixup) -------------------------------------------------------------------------------
// The permutation and the weights of a step's mixup, by ONE workgroup and the same counter protocol.  Lanes stride over the clips:
// each computes lam[b] (leaf_mix_draws.hpp: one pow and one cos in double) and puts the clip's key into LDS.  perm is the order of the
// keys, so the workgroup sorts them: a bitonic network over N, the power of two at or above B (the host passes it), with all-ones keys
// behind the real ones -- a real key's low word is b < B, so the padding sorts last and the first B keys' low words are perm.  Every
// stage is N / 2 compare-exchanges on disjoint pairs, a barrier between stages; log2(N) (log2(N) + 1) / 2 stages, 78 at the cap.
// The workgroup is as wide as the sort, N lanes between one wave and kMixMaxThreads (mix_draw_threads): up to 64 clips are one wave's,
// and at the cap sixteen waves share the double-precision draws, four clips a lane, and hide each other's LDS round trips, two pairs
// a lane and stage (measured: 48 us at B = 4096 against 89 us with 256 lanes, 5.9 us at B = 64 either way;
// profiles/clip_device_mixup.txt).  The kernel strides by blockDim.x, so any width gives the same result.
struct MixDrawParams {
    unsigned long long* state;    // the step counter
    unsigned long long seed, stream_base;
    double alpha;
    int* perm;                    // [B]
    float* lam;                   // [B]
    int B, N, advance;            // 1 <= B <= N <= kMixMaxBatch, N a power of two
};

constexpr int kMixMaxThreads = 1024;

inline int mix_draw_threads(int N) { return N < 64 ? 64 : (N > kMixMaxThreads ? kMixMaxThreads : N); }

__global__ __launch_bounds__(kMixMaxThreads) void draw_mixup_kernel(const MixDrawParams p) {
    __shared__ unsigned long long keys[kMixMaxBatch];
    const int lane = (int)threadIdx.x, width = (int)blockDim.x;
    const unsigned long long step = p.state[0];
    __syncthreads();
    if (lane == 0 && p.advance) p.state[0] = step + 1ull;
    for (int b = lane; b < p.N; b += width) {
        unsigned long long key = ~0ull;
        if (b < p.B) {
            const MixDraw d = draw_mix_clip(p.seed, p.stream_base, step, p.B, b, p.alpha);
            p.lam[b] = d.lam;
            key = d.key;
        }
        keys[b] = key;
    }
    __syncthreads();
    for (int k = 2; k <= p.N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < (p.N >> 1); i += width) {
                const int lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;      // pair i of the stage: lo < hi < N
                const unsigned long long a = keys[lo], c = keys[hi];
                if ((a > c) == ((lo & k) == 0)) {
                    keys[lo] = c;
                    keys[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int b = lane; b < p.B; b += width) p.perm[b] = (int)(unsigned)keys[b];
}

}  // namespace
