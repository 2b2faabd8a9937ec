// inst_clip_effects.hip -- ClipValue and the sox-style reverb on a float32 batch (leaf_clip_effects_f32): the kernel and its C-ABI
// entry.  One of the translation units of libleaf_hip.so; it shares nothing with the others but the header's declarations.
//
// The arithmetic is csrc/leaf_clip_effects.hpp (host and device): this file only decides who computes which sample and where the
// delay lines lie.
//
// Shape of the kernel.  A workgroup of 256 lanes serves G consecutive clips; their delay lines live in LDS, per clip the eight comb
// lines at their caps (the lengths at room_scale = 100, so that a plan cannot index past them), the four all-pass lines and one
// staged chunk.  A clip is walked in CHUNKS of C samples, C at most every delay length of the workgroup's clips: within a chunk every
// read of a line comes before the chunk's write to the same place, so a chunk is two phases and two barriers.
//   A. elementwise, all lanes: lane (g, k) owns sample n0 + k of clip g.  It loads and clamps it (ClipValue), parks it for phase B,
//      requests its twelve line values at once, sums the eight comb outputs in the order 7 .. 0 and runs the four all-passes one
//      after another -- the running sample stays in a register, the lane reads and rewrites ITS place of each line, no other lane
//      touches it in this chunk -- and stores y.  The sample of the NEXT chunk is requested here, so its latency passes under B.
//   B. serial, one wave: lane 8 g + i carries store[i] of clip g in a register over the whole clip and runs the three-operation
//      chain over the chunk's samples in order, in whole batches of eight whose line values are requested a batch ahead of the
//      chain that consumes them; the chunk's last samples, fewer than a batch, go one by one.
// The result is bit for bit the sequential definition: every operation is the one the definition names, on the operands it names.
//
// How many clips share a workgroup: G = as many as fit kFxLdsBudget, at most 8 (8 x 8 chains fill the serial wave) and at most
// 256 / allpass[0], so that a whole chunk of every clip is ONE pass of phase A (one sample per lane).  That is 6 clips at 8 kHz, 3 at
// 16 kHz, 1 from 44.1 kHz on.  Sharing costs a clip nothing -- phase A stays one pass, phase B's chains run side by side in one
// wave's lanes -- except that the group walks in the chunk of its shortest line; it takes a third of the workgroups and of the
// LDS for a batch.  The chain is latency-bound by construction: about 3 S dependent operations per clip, whatever B is.
//
// ClipValue's minimum and maximum are a reduction over the clip in front of the first chunk (the clip's own lanes, through LDS
// that the lines take afterwards).  No workspace, no atomics, no scratch, nothing read back.
#include "leaf_common.hpp"
#include "leaf_clip_effects.hpp"

namespace {

constexpr int kFxThreads = 256;
constexpr int kFxBatch = 8;                           // line values phase B requests ahead of its chain

struct FxParams {
    const float* x;
    float* y;
    const float* factor;          // [B] or NULL
    const float* feedback;        // [B], damp [B], comb [B][8]: all three or none
    const float* damp;
    const int* comb;
    int B, S;
    int G, W;                     // clips per workgroup; lanes per clip (256 / G)
    int clip_floats;              // floats of LDS per clip
    float wet;
    FxLengths L;
};

__global__ __launch_bounds__(kFxThreads) void clip_effects_kernel(const FxParams p) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x, S = p.S;
    const int g = tid / p.W, k = tid - g * p.W;
    const long long first = (long long)blockIdx.x * p.G;                  // the workgroup's first clip
    const long long b = first + g;
    const bool mine = g < p.G && b < p.B;
    const float* xb = p.x + (mine ? b : 0) * S;
    float* yb = p.y + (mine ? b : 0) * S;

    // ClipValue: the clip's bounds
    bool clip = false;
    float lo = 0.0f, hi = 0.0f;
    if (p.factor) {
        const float f = mine ? p.factor[b] : -1.0f;
        clip = f >= 0.0f;
        float mn = xb[0], mx = mn;
        if (clip)
            for (int n = k; n < S; n += p.W) {
                const float v = xb[n];
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
        lds[tid] = mn;
        lds[kFxThreads + tid] = mx;
        __syncthreads();
        if (clip) {
            for (int j = 0; j < p.W; ++j) {
                mn = fminf(mn, lds[g * p.W + j]);
                mx = fmaxf(mx, lds[kFxThreads + g * p.W + j]);
            }
            fx_clip_bounds(mn, mx, f, lo, hi);
        }
        __syncthreads();
    }

    // the clip's reverb plan, lengths clamped into [1, cap]
    bool rev = false;
    int len[kFxCombs];
#pragma unroll
    for (int i = 0; i < kFxCombs; ++i) len[i] = 1;
    if (p.comb && mine) {
        rev = p.comb[b * kFxCombs] > 0;
#pragma unroll
        for (int i = 0; i < kFxCombs; ++i) len[i] = fx_clamp_length(p.comb[b * kFxCombs + i], p.L.cap[i]);
    }
    if (mine && !rev)                                                     // no reverb: the clamped samples, a bit copy without ClipValue
        for (int n = k; n < S; n += p.W) {
            const float v = xb[n];
            yb[n] = clip ? fx_clip(v, lo, hi) : v;
        }
    if (!p.comb) return;

    // the chunk: at most every line of every reverberated clip of the workgroup, and one sample per lane (uniform)
    int C = p.W;
#pragma unroll
    for (int j = 0; j < kFxAllpasses; ++j) C = min(C, p.L.allpass[j]);
    bool any = false;
    for (int gg = 0; gg < p.G; ++gg) {
        const long long bb = first + gg;
        if (bb >= p.B || p.comb[bb * kFxCombs] <= 0) continue;
        any = true;
#pragma unroll
        for (int i = 0; i < kFxCombs; ++i) C = min(C, fx_clamp_length(p.comb[bb * kFxCombs + i], p.L.cap[i]));
    }
    if (!any) return;

    // phase B's lane: chain iB of clip gB
    const int gB = tid >> 3, iB = tid & 7;
    const long long bB = first + gB;
    bool chain = tid < kFxCombs * p.G && bB < p.B;
    int lenB = 1, offB = 0;
    float fb = 0.0f, dp = 0.0f, store = 0.0f;
    if (chain) chain = p.comb[bB * kFxCombs] > 0;
    if (chain) {
        int capB = 1;
#pragma unroll
        for (int i = 0; i < kFxCombs; ++i) {
            if (i < iB) offB += p.L.cap[i];
            if (i == iB) capB = p.L.cap[i];
        }
        lenB = fx_clamp_length(p.comb[bB * kFxCombs + iB], capB);
        fb = p.feedback[bB];
        dp = p.damp[bB];
    }

    // LDS: per clip [comb 0 .. 7 at their caps][all-pass 0 .. 3][the staged chunk: allpass[0] floats], everything zero at sample 0
    for (int e = tid; e < p.G * p.clip_floats; e += kFxThreads) lds[e] = 0.0f;
    int comb_floats = 0;
#pragma unroll
    for (int i = 0; i < kFxCombs; ++i) comb_floats += p.L.cap[i];
    int ap_floats = 0;
#pragma unroll
    for (int j = 0; j < kFxAllpasses; ++j) ap_floats += p.L.allpass[j];
    float* lines = lds + (g < p.G ? g : 0) * p.clip_floats;
    float* parked = lines + comb_floats + ap_floats;
    float* lineB = lds + (chain ? gB : 0) * p.clip_floats + offB;
    const float* parkedB = lds + (chain ? gB : 0) * p.clip_floats + comb_floats + ap_floats;
    __syncthreads();

    int pos[kFxCombs], q[kFxAllpasses];                                   // the lines' write indices at the chunk's first sample
#pragma unroll
    for (int i = 0; i < kFxCombs; ++i) pos[i] = 0;
#pragma unroll
    for (int j = 0; j < kFxAllpasses; ++j) q[j] = 0;
    int posB = 0;
    const bool walk = mine && rev && k < C;
    float xv = (walk && k < S) ? xb[k] : 0.0f;

    for (int n0 = 0; n0 < S; n0 += C) {
        const int cnt = min(C, S - n0);
        if (walk && k < cnt) {                                            // phase A
            const float in = clip ? fx_clip(xv, lo, hi) : xv;
            if ((long long)n0 + C + k < S) xv = xb[n0 + C + k];
            parked[k] = in;
            float oc[kFxCombs], oa[kFxAllpasses];                          // every read of the chunk first: one trip to LDS
            float* wa[kFxAllpasses];
            int at = comb_floats;
#pragma unroll
            for (int i = kFxCombs - 1; i >= 0; --i) {
                at -= p.L.cap[i];
                int idx = pos[i] + k;
                if (idx >= len[i]) idx -= len[i];
                oc[i] = lines[at + idx];
            }
            at = comb_floats + ap_floats;
#pragma unroll
            for (int j = kFxAllpasses - 1; j >= 0; --j) {
                at -= p.L.allpass[j];
                int idx = q[j] + k;
                if (idx >= p.L.allpass[j]) idx -= p.L.allpass[j];
                wa[j] = lines + at + idx;
                oa[j] = *wa[j];
            }
            float out = 0.0f;
#pragma unroll
            for (int i = kFxCombs - 1; i >= 0; --i) out = fx_sum(out, oc[i]);
#pragma unroll
            for (int j = kFxAllpasses - 1; j >= 0; --j) *wa[j] = fx_allpass(oa[j], out);
            yb[n0 + k] = fx_mix(in, out, p.wet);
        }
        __syncthreads();
        if (chain) {                                                      // phase B
            // Whole batches of kFxBatch samples, the next batch's line values and samples requested before this batch's chain runs
            // (other places than this batch writes: both lie inside the chunk, and cnt <= lenB).  Sample u of a batch that begins
            // at line index `base` sits at base + u, or at base + u - lenB behind the wrap: one select per access, the u in the
            // instruction's offset.
            float o[kFxBatch], v[kFxBatch];
            int base = posB, k0 = 0;
            if (cnt >= kFxBatch) {
                const float* a = lineB + base;
                const int r = lenB - base;
#pragma unroll
                for (int u = 0; u < kFxBatch; ++u) {
                    o[u] = (u < r ? a : a - lenB)[u];
                    v[u] = parkedB[u];
                }
            }
            for (; k0 + kFxBatch <= cnt; k0 += kFxBatch) {
                const bool more = k0 + 2 * kFxBatch <= cnt;
                int next = base + kFxBatch;
                if (next >= lenB) next -= lenB;
                if (next >= lenB) next -= lenB;                           // (a line shorter than a batch cannot occur here: cnt <= lenB)
                float on[kFxBatch], vn[kFxBatch];
                if (more) {
                    const float* a = lineB + next;
                    const int r = lenB - next;
#pragma unroll
                    for (int u = 0; u < kFxBatch; ++u) {
                        on[u] = (u < r ? a : a - lenB)[u];
                        vn[u] = parkedB[k0 + kFxBatch + u];
                    }
                }
                float* w = lineB + base;
                const int r = lenB - base;
#pragma unroll
                for (int u = 0; u < kFxBatch; ++u) (u < r ? w : w - lenB)[u] = fx_comb(o[u], v[u], store, dp, fb);
                if (more) {
#pragma unroll
                    for (int u = 0; u < kFxBatch; ++u) {
                        o[u] = on[u];
                        v[u] = vn[u];
                    }
                }
                base = next;
            }
            for (; k0 < cnt; ++k0) {                                      // the chunk's last samples, fewer than a batch
                const float ov = lineB[base];
                lineB[base] = fx_comb(ov, parkedB[k0], store, dp, fb);
                if (++base == lenB) base = 0;
            }
            posB = base;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kFxCombs; ++i) {
            pos[i] += cnt;
            if (pos[i] >= len[i]) pos[i] -= len[i];
        }
#pragma unroll
        for (int j = 0; j < kFxAllpasses; ++j) {
            q[j] += cnt;
            if (q[j] >= p.L.allpass[j]) q[j] -= p.L.allpass[j];
        }
    }
}

}  // namespace

int leaf_clip_effects_f32(const float* x, float* y, int B, int S, const float* clip_factor, const float* feedback, const float* damp,
                          const int* comb, int sample_rate, float wet, void* stream) {
    if (!x || !y) return LEAF_ERR_NULL_POINTER;
    const bool reverb = feedback || damp || comb;
    if (reverb && !(feedback && damp && comb)) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || S < 1 || (long long)B * S >= (1ll << 31)) return LEAF_ERR_BAD_SHAPE;
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y), bytes = (uintptr_t)B * S * sizeof(float);
    if (xa < ya + bytes && ya < xa + bytes) return LEAF_ERR_BAD_SHAPE;    // y must not overlap x
    FxParams p{};
    if (reverb && !fx_lengths(sample_rate, p.L)) return LEAF_ERR_BAD_SHAPE;
    auto misaligned = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3u) != 0; };
    if (misaligned(x) || misaligned(y) || misaligned(clip_factor) || misaligned(feedback) || misaligned(damp) || misaligned(comb))
        return LEAF_ERR_ALIGNMENT;
    p.G = kFxMaxClipsPerGroup;
    if (reverb) {
        p.G = fx_clips_per_group(p.L, kFxThreads);
        if (p.G < 1) return LEAF_ERR_UNSUPPORTED;                         // the rate's lines do not fit the LDS budget
        p.clip_floats = (int)fx_clip_floats(p.L);
    }
    p.x = x; p.y = y; p.factor = clip_factor; p.feedback = feedback; p.damp = damp; p.comb = comb;
    p.B = B; p.S = S; p.W = kFxThreads / p.G; p.wet = wet;
    const size_t lds = sizeof(float) * std::max<size_t>((size_t)p.G * (size_t)p.clip_floats, 2 * kFxThreads);
    const dim3 grid((unsigned)((B + p.G - 1) / p.G)), block(kFxThreads);
    hipLaunchKernelGGL(clip_effects_kernel, grid, block, lds, (hipStream_t)stream, p);
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}
