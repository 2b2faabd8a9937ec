// inst_resample.hip -- windowed-sinc resampling of a packed sample store (leaf_resample_f32): the kernels and their C-ABI entries.
// One of the translation units of libleaf_hip.so; it shares nothing with the others but the header's declarations.
//
// The arithmetic is csrc/leaf_resample.hpp (host and device): this file only decides who computes which output and where the
// operands lie.
//
// Shape of the kernels.  The work unit is a TILE of kResampleTile = 1024 consecutive outputs of ONE recording and a workgroup of 256
// lanes (leaf_clip_peaks_f32's split, by outputs here): a long recording is many tiles, spread over the chip, a short one is one
// workgroup's.  Launch 1 (one workgroup) writes the exclusive prefix of the clamped records' tile counts into the workspace; launch 2
// walks the tiles, workgroup w taking tiles w, w + grid, ... -- the host does not see the plan, so the grid is sized by what
// non-overlapping records can have and a plan with more is walked by the same workgroups.  Per tile:
//   1. one binary search in the prefix finds the recording; its record is clamped (resample_record);
//   2. the tile's input window -- the recording's samples [i0 o - width, i0 o - width + wlen), i0 = j0 / n -- is staged into LDS as
//      float32, int16 converted in the load, everything outside [0, L) ZERO: that is the padding rule, and it is what keeps the
//      neighbouring recording out.  Chunks of four samples that lie inside the recording come in one load at element alignment;
//   3. lane l computes the outputs l, l + 256, l + 512, l + 768 of the tile: consecutive lanes take consecutive outputs, so their
//      window reads are o / n samples apart on average and their tap rows one (odd) stride apart.  The span k0 / cnt read from the
//      table is clamped against the window (resample_clamp_span) before it is used;
//   4. the outputs are parked in LDS and leave in 16-byte chunks aligned in `out` (four float32 or eight int16), element stores at
//      the two ends of the tile.
// Where the taps come from is a template parameter of the tile function: LDS, staged once per workgroup, when window, outputs and
// table fit kResampleLdsBudget and the table's header says so; global memory (L2-resident) otherwise.  A ratio whose window alone is
// beyond the budget (from o / n of about 15: 16 -> 1, 44100 -> 2000) reads samples and taps from global memory: correct, not fast.
// No scratch, no atomics, nothing shared between workgroups but the prefix.
#include "leaf_common.hpp"
#include "leaf_resample.hpp"

namespace {

constexpr int kResampleThreads = 256;
constexpr int kResampleMaxBlocks = 1 << 16;

typedef short s16x4v __attribute__((ext_vector_type(4), aligned(2)));    // 8-byte load at 2-byte alignment
typedef short s16x8 __attribute__((ext_vector_type(8)));                 // 16-byte store

struct ResampleParams {
    const void* store;            // float32 or int16 samples
    long long store_len;
    const long long* in_off;      // [R]
    const int* in_len;            // [R]
    const long long* out_off;     // [R]
    const int* table;             // header, k0[n], cnt[n], taps[n][stride]
    void* out;                    // float32 or int16
    long long out_total;
    long long* tile_start;        // [R + 1] workspace
    int R, o, n, width, K, stride;
    int window;                   // samples of LDS the window may take (0: the window is read from global memory)
    int taps_fit;                 // the table fits LDS beside it
};

// launch 1: the tile prefix of the clamped plan (the scan of clip_peaks_plan_kernel)
__global__ __launch_bounds__(kResampleThreads) void resample_plan_kernel(const ResampleParams p) {
    __shared__ long long wsum[kResampleThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (long long base = 0; base < p.R; base += kResampleThreads) {
        const long long i = base + tid;
        long long t = 0;
        if (i < p.R) {
            const ResampleRecord r = resample_record(p.in_off[i], p.in_len[i], p.store_len, p.out_off[i], p.out_total, p.o, p.n);
            t = (r.out_len + kResampleTile - 1) / kResampleTile;
        }
        long long s = t;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long v = __shfl_up(s, d);
            if (lane >= d) s += v;
        }
        if (lane == 63) wsum[wave] = s;
        __syncthreads();
        long long before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kResampleThreads / 64; ++w) {
            const long long x = wsum[w];
            if (w < wave) before += x;
            total += x;
        }
        if (i < p.R) p.tile_start[i] = carry + before + s - t;
        carry += total;
        __syncthreads();
    }
    if (tid == 0) p.tile_start[p.R] = carry;
}

template <bool PCM> __device__ __forceinline__ float resample_load(const void* store, long long i) {
    if constexpr (PCM) return resample_widen(static_cast<const short*>(store)[i]);
    else return static_cast<const float*>(store)[i];
}

// The tile's outputs into `outs` (LDS).  WIN: the samples come from the staged window `win`; otherwise from the store, every index
// checked against the recording.  TAPS: spans and taps come from LDS (`lk0`, `lcnt`, `ltaps`); otherwise from the table in global
// memory.  The same chain either way.
template <bool PCM, bool WIN, bool TAPS>
__device__ __forceinline__ void resample_tile(const ResampleParams& p, const ResampleRecord& r, long long i0, int p0, int count, int wlen,
                                              const float* win, const int* lk0, const int* lcnt, const float* ltaps, float* outs) {
    const int* gk0 = p.table + kResampleHeaderInts;
    const int* gcnt = gk0 + p.n;
    const float* gtaps = reinterpret_cast<const float*>(gcnt + p.n);
    for (int tj = threadIdx.x; tj < count; tj += kResampleThreads) {
        const int t = p0 + tj, di = t / p.n, ph = t - di * p.n;            // output j0 + tj = (i0 + di) n + ph
        int k0 = TAPS ? lk0[ph] : gk0[ph], cnt = TAPS ? lcnt[ph] : gcnt[ph];
        resample_clamp_span(k0, cnt, p.K, p.stride);
        const float* h = (TAPS ? ltaps : gtaps) + (size_t)ph * p.stride;
        float y;
        if constexpr (WIN) {
            const int base = di * p.o;                                    // the window begins at sample i0 o - width: tap k reads base + k
            if (base + k0 + cnt > wlen) cnt = wlen - base - k0 > 0 ? wlen - base - k0 : 0;   // (never taken: wlen covers the tile's taps)
            const float* x = win + base;
            y = resample_output(k0, cnt, [h](int i) { return h[i]; }, [x](int k) { return x[k]; });
        } else {
            const long long first = (i0 + di) * (long long)p.o - p.width;
            const void* store = p.store;
            const long long off = r.off, L = r.L;
            y = resample_output(k0, cnt, [h](int i) { return h[i]; }, [=](int k) {
                const long long s = first + k;
                return s >= 0 && s < L ? resample_load<PCM>(store, off + s) : 0.0f;
            });
        }
        outs[tj] = y;
    }
}

// `count` outputs from `outs` to out[g0, g0 + count): 16-byte chunks aligned in `out`, element stores in front of the first and
// behind the last
template <bool OUT16> __device__ __forceinline__ void resample_store(void* out, long long g0, int count, const float* outs) {
    constexpr int E = OUT16 ? 8 : 4;                                      // elements per chunk
    constexpr int ES = OUT16 ? 2 : 4;
    const int tid = threadIdx.x;
    const unsigned long long first = reinterpret_cast<uintptr_t>(out) / ES + (unsigned long long)g0;   // the element's place in memory
    int head = (int)((E - (first % E)) % E);
    if (head > count) head = count;
    const int chunks = (count - head) / E, tail0 = head + chunks * E;
    auto put = [&](int e) {
        if constexpr (OUT16) static_cast<short*>(out)[g0 + e] = resample_quantize(outs[e]);
        else static_cast<float*>(out)[g0 + e] = outs[e];
    };
    if (tid < head) put(tid);
    if (tail0 + tid < count && tid < E) put(tail0 + tid);
    for (int q = tid; q < chunks; q += kResampleThreads) {
        const float* v = outs + head + q * E;
        if constexpr (OUT16) {
            s16x8 w;
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = resample_quantize(v[e]);
            *reinterpret_cast<s16x8*>(static_cast<short*>(out) + g0 + head + (long long)q * E) = w;
        } else {
            *reinterpret_cast<f32x4*>(static_cast<float*>(out) + g0 + head + (long long)q * E) = f32x4{v[0], v[1], v[2], v[3]};
        }
    }
}

// launch 2.  LDS: [outs: kResampleTile floats][window: p.window floats][k0, cnt: 2 n ints][taps: n stride floats], the last two only
// where they fit (p.taps_fit)
template <bool PCM, bool OUT16, bool WIN>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const ResampleParams p) {
    extern __shared__ float lds[];
    float* outs = lds;
    float* win = lds + kResampleTile;
    int* lk0 = reinterpret_cast<int*>(win + p.window);
    int* lcnt = lk0 + p.n;
    float* ltaps = reinterpret_cast<float*>(lcnt + p.n);
    const int tid = threadIdx.x;
    const long long total = p.tile_start[p.R];
    if ((long long)blockIdx.x >= total) return;

    // the table's own word decides between the two tap paths (uniform: a scalar load), the host whether LDS has the room
    const bool taps_lds = WIN && p.taps_fit && p.table[5] != 0;
    if (taps_lds) {
        const int words = 2 * p.n + p.n * p.stride;                       // k0, cnt and the rows lie behind one another in both places
        const int* src = p.table + kResampleHeaderInts;
        for (int w = tid; w < words; w += kResampleThreads) lk0[w] = src[w];
    }

    for (long long tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int i = 0;                                                        // the LAST i with tile_start[i] <= tile
        for (int hi = p.R; hi - i > 1;) {
            const int mid = i + (hi - i) / 2;
            if (p.tile_start[mid] <= tile) i = mid; else hi = mid;
        }
        const ResampleRecord r = resample_record(p.in_off[i], p.in_len[i], p.store_len, p.out_off[i], p.out_total, p.o, p.n);
        const long long j0 = (tile - p.tile_start[i]) * kResampleTile;    // first output of the tile, in the recording
        const long long left = r.out_len - j0;
        if (left <= 0) continue;                                          // (a prefix that does not match the plan: nothing to do)
        const int count = (int)(left < kResampleTile ? left : kResampleTile);
        const long long i0 = j0 / p.n;
        const int p0 = (int)(j0 - i0 * p.n);
        int wlen = 0;
        __syncthreads();                                                  // the previous tile's outputs have left; the taps are staged
        if constexpr (WIN) {
            const long long need = (long long)((p0 + count - 1) / p.n) * p.o + p.K;
            wlen = (int)(need < p.window ? need : p.window);
            const long long s0 = i0 * (long long)p.o - p.width;           // the recording's sample behind window element 0
            for (int c = tid; 4 * c < wlen; c += kResampleThreads) {
                const long long s = s0 + 4ll * c;
                float v[4];
                if (s >= 0 && s + 4 <= r.L) {
                    if constexpr (PCM) {
                        const s16x4v q = *reinterpret_cast<const s16x4v*>(static_cast<const short*>(p.store) + (r.off + s));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = resample_widen(q[e]);
                    } else {
                        const f32x4u q = *reinterpret_cast<const f32x4u*>(static_cast<const float*>(p.store) + (r.off + s));
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = q[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (s + e >= 0 && s + e < r.L) ? resample_load<PCM>(p.store, r.off + s + e) : 0.0f;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (4 * c + e < wlen) win[4 * c + e] = v[e];
            }
            __syncthreads();
        }
        if (taps_lds) resample_tile<PCM, WIN, true>(p, r, i0, p0, count, wlen, win, lk0, lcnt, ltaps, outs);
        else resample_tile<PCM, WIN, false>(p, r, i0, p0, count, wlen, win, lk0, lcnt, ltaps, outs);
        __syncthreads();
        resample_store<OUT16>(p.out, r.out_off + j0, count, outs);
    }
}

}  // namespace

// include/leaf_hip.h: the output length, the table (host only, no GPU), the workspace, the call
size_t leaf_resample_length(long long L, int orig_freq, int new_freq) {
    if (orig_freq <= 0 || new_freq <= 0) return 0;
    const long long g = resample_gcd(orig_freq, new_freq);
    return (size_t)resample_length(L, orig_freq / g, new_freq / g);
}

size_t leaf_resample_table_bytes(int orig_freq, int new_freq, int lowpass_width, double rolloff) {
    if (orig_freq <= 0 || new_freq <= 0 || lowpass_width < 1 || !(rolloff > 0.0 && rolloff <= 1.0)) return 0;
    ResamplePlan q;
    if (!resample_plan(orig_freq, new_freq, lowpass_width, rolloff, q)) return 0;
    return (size_t)resample_table_shape(q).bytes;
}

int leaf_resample_table_f32(int orig_freq, int new_freq, int lowpass_width, double rolloff, void* table_host, size_t table_bytes) {
    ResamplePlan q;
    const bool valid = orig_freq > 0 && new_freq > 0 && lowpass_width >= 1 && rolloff > 0.0 && rolloff <= 1.0;
    ResampleTableShape s{};
    if (valid && (!resample_plan(orig_freq, new_freq, lowpass_width, rolloff, q) || (s = resample_table_shape(q)).bytes == 0))
        return LEAF_ERR_UNSUPPORTED;
    if (!table_host) return LEAF_ERR_NULL_POINTER;
    if (!valid || table_bytes != (size_t)s.bytes) return LEAF_ERR_BAD_SHAPE;
    if (reinterpret_cast<uintptr_t>(table_host) & 3u) return LEAF_ERR_ALIGNMENT;
    resample_table_fill(q, s, table_host);
    return LEAF_OK;
}

size_t leaf_resample_workspace_bytes(int R) { return R < 1 ? 0 : sizeof(long long) * ((size_t)R + 1); }

int leaf_resample_f32(const void* store, long long store_len, int flags, int R, const long long* in_off, const int* in_len,
                      int orig_freq, int new_freq, int lowpass_width, double rolloff, const void* table, size_t table_bytes,
                      void* out, long long out_total, const long long* out_off, void* workspace, size_t workspace_bytes, void* stream) {
    if (flags & ~(LEAF_FLAG_X_PCM16 | LEAF_FLAG_OUT_PCM16)) return LEAF_ERR_UNSUPPORTED;
    const bool valid = orig_freq > 0 && new_freq > 0 && lowpass_width >= 1 && rolloff > 0.0 && rolloff <= 1.0;
    ResamplePlan q;
    ResampleTableShape s{};
    if (valid && (!resample_plan(orig_freq, new_freq, lowpass_width, rolloff, q) || (s = resample_table_shape(q)).bytes == 0))
        return LEAF_ERR_UNSUPPORTED;
    if (!store || !in_off || !in_len || !table || !out || !out_off) return LEAF_ERR_NULL_POINTER;
    if (R < 1 || store_len < 0 || out_total < 0 || !valid || table_bytes != (size_t)s.bytes) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0, out16 = (flags & LEAF_FLAG_OUT_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(store, pcm ? 1u : 3u) || misaligned(in_off, 7u) || misaligned(in_len, 3u) || misaligned(table, 3u) ||
        misaligned(out, out16 ? 1u : 3u) || misaligned(out_off, 7u) || misaligned(workspace, 15u))
        return LEAF_ERR_ALIGNMENT;
    if (!workspace || workspace_bytes < leaf_resample_workspace_bytes(R)) return LEAF_ERR_WORKSPACE;

    bool win_lds, taps_fit;
    resample_paths(q, s, win_lds, taps_fit);
    ResampleParams p{};
    p.store = store; p.store_len = store_len; p.in_off = in_off; p.in_len = in_len; p.out_off = out_off;
    p.table = static_cast<const int*>(table); p.out = out; p.out_total = out_total;
    p.tile_start = static_cast<long long*>(workspace);
    p.R = R; p.o = q.o; p.n = q.n; p.width = q.width; p.K = q.K; p.stride = s.stride;
    p.window = win_lds ? (int)resample_window_samples(q) : 0;
    p.taps_fit = taps_fit ? 1 : 0;
    size_t lds = sizeof(float) * ((size_t)kResampleTile + (size_t)p.window);
    if (taps_fit) lds += (size_t)s.bytes - sizeof(int) * kResampleHeaderInts;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(resample_plan_kernel, dim3(1), dim3(kResampleThreads), 0, st, p);
    // the host does not see the plan: records that do not overlap in `out` have at most R + out_total / tile tiles, and a plan with
    // more is walked by the same workgroups
    const long long tiles = (long long)R + out_total / kResampleTile;
    const dim3 grid((unsigned)std::min<long long>(tiles, kResampleMaxBlocks)), block(kResampleThreads);
    switch ((pcm ? 4 : 0) | (out16 ? 2 : 0) | (win_lds ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((resample_kernel<false, false, false>), grid, block, lds, st, p); break;
        case 1: hipLaunchKernelGGL((resample_kernel<false, false, true>), grid, block, lds, st, p); break;
        case 2: hipLaunchKernelGGL((resample_kernel<false, true, false>), grid, block, lds, st, p); break;
        case 3: hipLaunchKernelGGL((resample_kernel<false, true, true>), grid, block, lds, st, p); break;
        case 4: hipLaunchKernelGGL((resample_kernel<true, false, false>), grid, block, lds, st, p); break;
        case 5: hipLaunchKernelGGL((resample_kernel<true, false, true>), grid, block, lds, st, p); break;
        case 6: hipLaunchKernelGGL((resample_kernel<true, true, false>), grid, block, lds, st, p); break;
        default: hipLaunchKernelGGL((resample_kernel<true, true, true>), grid, block, lds, st, p); break;
    }
    if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    return LEAF_OK;
}

// ======================================================================================================================================
// The chunked resampler (leaf_resample_stream_step_f32): B independent streams at a device rate, one launch per step and 128 slots.
// The position arithmetic is csrc/leaf_resample_stream.hpp; the tile function, the aligned store and the quantiser are the ones above.
//
// Shape of the kernel.  Grid (tiles of kResampleTile outputs over n_max, at least 1) x slots, 256 lanes.  Workgroup (tile, y) serves
// slot b0 + y, whose record travels BY VALUE in the kernel arguments (five words per slot, scalar loads).  It stages its tile's window
// into LDS as float32 from TWO sources -- window coordinate c is +0.0f below `shift`, history[parity][b][c - shift] below hist_len,
// chunk[b][c - shift - hist_len] below Lv, +0.0f behind that -- runs resample_tile from phase `phase` on, fills the tile behind the
// slot's n outputs with zeros and lets resample_store write the whole tile: every element of out is written.  The workgroup of tile 0
// also copies V[drop_samples, Lv) to row b of the OTHER history half.  Every workgroup reads only the old half and the chunk, so
// nothing races and no barrier crosses workgroups; an idle slot's workgroups write their zeros and touch nothing of the state.  LDS is
// that of resample_kernel (kResampleLdsBudget: a starting point that nobody measured, kept as it is).  No scratch, no atomics.
#include <vector>
#include "leaf_resample_stream.hpp"

namespace {

constexpr int kResampleBankSlots = 128;

struct ResampleSlotRec {
    // w[0] = hist_len | shift << 16     w[1] = Tc     w[2] = n     w[3] = drop_samples
    // w[4] = phase | parity << 16 | idle << 17 | end << 18
    unsigned w[5];
};
struct ResampleStreamParams {
    const void* chunk;            // [B][chunk_stride], the first Tc samples of a row; float32 or int16
    long long chunk_stride;
    char* half[2];                // the two history halves, [B][H] samples each
    const int* table;
    void* out;                    // [B][n_max], float32 or int16
    int b0;                       // the launch's first slot
    int n_max, H;
    int o, n, width, K, stride, window, taps_fit;
    ResampleSlotRec rec[kResampleBankSlots];
};
static_assert(sizeof(ResampleStreamParams) <= 4096, "the records travel in the kernel argument segment");

// LDS as in resample_kernel: [outs: kResampleTile floats][window: p.window floats][k0, cnt: 2 n ints][taps: n stride floats]
template <bool PCM, bool OUT16>
__global__ __launch_bounds__(kResampleThreads) void resample_stream_kernel(const ResampleStreamParams p) {
    extern __shared__ float lds[];
    typedef typename std::conditional<PCM, short, float>::type Sample;
    float* outs = lds;
    float* win = lds + kResampleTile;
    int* lk0 = reinterpret_cast<int*>(win + p.window);
    int* lcnt = lk0 + p.n;
    float* ltaps = reinterpret_cast<float*>(lcnt + p.n);
    const int tid = threadIdx.x, y = blockIdx.y;
    const unsigned w0 = p.rec[y].w[0], w4 = p.rec[y].w[4];
    const int hist_len = (int)(w0 & 0xffffu), shift = (int)(w0 >> 16), Tc = (int)p.rec[y].w[1], n = (int)p.rec[y].w[2];
    const int drop = (int)p.rec[y].w[3], phase = (int)(w4 & 0xffffu);
    const bool parity = (w4 >> 16) & 1u, idle = (w4 >> 17) & 1u, end = (w4 >> 18) & 1u;
    const long long b = (long long)p.b0 + y;
    const long long j0 = (long long)blockIdx.x * kResampleTile;           // first output of the tile, in the slot's row
    const int span = (int)std::min<long long>(kResampleTile, p.n_max - j0);   // elements of out this workgroup writes (n_max = 0: none)
    const int count = idle ? 0 : (int)std::max<long long>(0, std::min<long long>(span, n - j0));
    const long long Lv = (long long)hist_len + Tc;
    const Sample* hist = reinterpret_cast<const Sample*>(p.half[parity ? 1 : 0]) + b * p.H;
    const Sample* chunk = static_cast<const Sample*>(p.chunk) + b * p.chunk_stride;

    if (count > 0) {
        const bool taps_lds = p.taps_fit && p.table[5] != 0;              // the table's own word decides between the two tap paths
        if (taps_lds) {
            const int words = 2 * p.n + p.n * p.stride;
            const int* src = p.table + kResampleHeaderInts;
            for (int w = tid; w < words; w += kResampleThreads) lk0[w] = src[w];
        }
        const long long t0 = phase + j0, i0 = t0 / p.n;                   // the tile's first output is phase p0 of group i0
        const int p0 = (int)(t0 - i0 * p.n);
        const long long need = (long long)((p0 + count - 1) / p.n) * p.o + p.K;
        const int wlen = (int)(need < p.window ? need : p.window);
        const long long c0 = i0 * p.o;                                    // the window coordinate behind window element 0
        for (int c = tid; 4 * c < wlen; c += kResampleThreads) {
            const long long v = c0 + 4ll * c - shift;                     // place in V of the chunk's first sample
            float x[4];
            if (v >= hist_len && v + 4 <= Lv) {                           // four samples of the chunk: one load at element alignment
                if constexpr (PCM) {
                    const s16x4v q = *reinterpret_cast<const s16x4v*>(chunk + (v - hist_len));
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = resample_widen(q[e]);
                } else {
                    const f32x4u q = *reinterpret_cast<const f32x4u*>(chunk + (v - hist_len));
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = q[e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const long long s = resample_stream_source(c0 + 4ll * c + e, shift, hist_len, Tc);
                    float f = 0.0f;
                    if (s >= hist_len) f = resample_load<PCM>(chunk, s - hist_len);
                    else if (s >= 0) f = resample_load<PCM>(hist, s);
                    x[e] = f;
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * c + e < wlen) win[4 * c + e] = x[e];
        }
        __syncthreads();
        ResampleParams q{};                                               // what resample_tile reads with the window staged
        q.table = p.table; q.o = p.o; q.n = p.n; q.width = p.width; q.K = p.K; q.stride = p.stride;
        const ResampleRecord none{};
        if (taps_lds) resample_tile<PCM, true, true>(q, none, i0, p0, count, wlen, win, lk0, lcnt, ltaps, outs);
        else resample_tile<PCM, true, false>(q, none, i0, p0, count, wlen, win, lk0, lcnt, ltaps, outs);
    }
    for (int e = count + tid; e < span; e += kResampleThreads) outs[e] = 0.0f;   // behind the slot's outputs: zeros
    __syncthreads();
    if (span > 0) resample_store<OUT16>(p.out, b * p.n_max + j0, span, outs);

    if (blockIdx.x == 0 && !idle && !end) {                               // the hand-over: V[drop, Lv) to the other half
        Sample* next = reinterpret_cast<Sample*>(p.half[parity ? 0 : 1]) + b * p.H;
        const int keep = (int)std::min<long long>(Lv - drop, p.H);
        for (int e = tid; e < keep; e += kResampleThreads) {
            const long long v = (long long)drop + e;
            next[e] = v < hist_len ? hist[v] : chunk[v - hist_len];
        }
    }
}

struct ResampleStreamLayout { int H; size_t half, total; };
ResampleStreamLayout resample_stream_layout(int B, const ResamplePlan& q, bool pcm) {
    ResampleStreamLayout L{};
    L.H = q.K - 1;
    L.half = ((size_t)B * (size_t)L.H * (pcm ? 2 : 4) + 255) / 256 * 256;
    if (L.half == 0) L.half = 256;                                        // (o == n keeps no history: the buffer still exists)
    L.total = 2 * L.half;
    return L;
}

// the plan of a streaming call and its table's shape; LEAF_OK, or what the step answers for these parameters
int resample_stream_setup(int orig_freq, int new_freq, int W, double rolloff, int flags, ResamplePlan& q, ResampleTableShape& s, bool& valid) {
    if (flags & ~(LEAF_FLAG_X_PCM16 | LEAF_FLAG_OUT_PCM16)) return LEAF_ERR_UNSUPPORTED;
    valid = orig_freq > 0 && new_freq > 0 && W >= 1 && rolloff > 0.0 && rolloff <= 1.0;
    if (!valid) return LEAF_OK;
    if (!resample_plan(orig_freq, new_freq, W, rolloff, q) || (s = resample_table_shape(q)).bytes == 0) return LEAF_ERR_UNSUPPORTED;
    bool win_lds, taps_fit;
    resample_paths(q, s, win_lds, taps_fit);
    if (!win_lds || q.K > 65535) return LEAF_ERR_UNSUPPORTED;            // a tile's window must fit LDS (16 -> 1, 44100 -> 2000 do not)
    return LEAF_OK;
}

}  // namespace

int leaf_resample_stream_history_samples(int orig_freq, int new_freq, int lowpass_width, double rolloff) {
    ResamplePlan q;
    ResampleTableShape s{};
    bool valid = false;
    if (resample_stream_setup(orig_freq, new_freq, lowpass_width, rolloff, 0, q, s, valid) != LEAF_OK || !valid) return 0;
    return q.K - 1;
}

size_t leaf_resample_stream_state_bytes(int B, int orig_freq, int new_freq, int lowpass_width, double rolloff, int flags) {
    ResamplePlan q;
    ResampleTableShape s{};
    bool valid = false;
    if (B < 1 || resample_stream_setup(orig_freq, new_freq, lowpass_width, rolloff, flags, q, s, valid) != LEAF_OK || !valid) return 0;
    return resample_stream_layout(B, q, (flags & LEAF_FLAG_X_PCM16) != 0).total;
}

// host only: every slot's record and count from its carried position, and the positions moved -- all or none
int leaf_resample_stream_plan(int B, int orig_freq, int new_freq, int lowpass_width, double rolloff, leaf_resample_pos* pos, const int* Tc,
                              const int* end, leaf_resample_slot* slots, int* counts) {
    ResamplePlan q;
    ResampleTableShape s{};
    bool valid = false;
    const int rc = resample_stream_setup(orig_freq, new_freq, lowpass_width, rolloff, 0, q, s, valid);
    if (rc != LEAF_OK) return rc;
    if (B == 0 && valid) return LEAF_OK;
    if (!pos || !Tc || !slots || !counts) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || !valid) return LEAF_ERR_BAD_SHAPE;
    std::vector<ResampleStreamPos> next((size_t)B);
    for (int b = 0; b < B; ++b) {                                         // first pass: nothing moves
        const leaf_resample_pos& at = pos[b];
        if (Tc[b] < 0 || Tc[b] > kResampleStreamMaxChunk || (at.running & ~1) || (at.parity & ~1)) return LEAF_ERR_BAD_SHAPE;
        if (at.running && (at.hist_len < 0 || at.hist_len > q.K - 1 || at.shift < 0 || at.shift > q.width || at.phase < 0 || at.phase >= q.n))
            return LEAF_ERR_BAD_SHAPE;
        leaf_resample_slot& r = slots[b];
        r = leaf_resample_slot{};
        counts[b] = 0;
        const bool ends = end && end[b];
        if (Tc[b] == 0 && !(ends && at.running)) {                        // idle, or `end` on a slot that is not running
            r.idle = 1;
            continue;
        }
        const ResampleStreamPos from = at.running ? ResampleStreamPos{at.hist_len, at.shift, at.phase} : resample_stream_begin(q);
        const ResampleStreamMove m = resample_stream_move(q, from, Tc[b], ends);
        if (m.n > 0x7fffffffll) return LEAF_ERR_BAD_SHAPE;
        r.hist_len = from.hist_len; r.Tc = Tc[b]; r.parity = at.parity; r.shift = from.shift; r.phase = from.phase;
        r.n = (int)m.n; r.drop_samples = (int)m.drop; r.end = ends ? 1 : 0;
        counts[b] = (int)m.n;
        next[(size_t)b] = m.next;
    }
    for (int b = 0; b < B; ++b) {
        if (slots[b].idle) continue;
        const ResampleStreamPos& to = next[(size_t)b];
        pos[b].running = slots[b].end ? 0 : 1;
        pos[b].hist_len = to.hist_len; pos[b].shift = to.shift; pos[b].phase = to.phase;
        pos[b].parity ^= 1;
    }
    return LEAF_OK;
}

int leaf_resample_stream_step_f32(const void* chunk, long long chunk_stride, int B, const leaf_resample_slot* slots, int n_max, void* state,
                                  size_t state_bytes, int flags, int orig_freq, int new_freq, int lowpass_width, double rolloff,
                                  const void* table, size_t table_bytes, void* out, void* stream) {
    ResamplePlan q;
    ResampleTableShape s{};
    bool valid = false;
    const int rc = resample_stream_setup(orig_freq, new_freq, lowpass_width, rolloff, flags, q, s, valid);
    if (rc != LEAF_OK) return rc;
    if (B == 0 && valid && n_max >= 0) return LEAF_OK;
    if (!slots || !state || !table || (n_max > 0 && !out)) return LEAF_ERR_NULL_POINTER;
    int Tc_max = 0;
    for (int b = 0; b < B; ++b)
        if (!slots[b].idle) Tc_max = std::max(Tc_max, slots[b].Tc);
    if (Tc_max > 0 && !chunk) return LEAF_ERR_NULL_POINTER;
    if (B < 1 || n_max < 0 || !valid || table_bytes != (size_t)s.bytes) return LEAF_ERR_BAD_SHAPE;
    for (int b = 0; b < B; ++b) {
        if (slots[b].idle & ~1) return LEAF_ERR_BAD_SHAPE;
        if (!slots[b].idle && (slots[b].Tc < 0 || slots[b].Tc > kResampleStreamMaxChunk)) return LEAF_ERR_BAD_SHAPE;
    }
    if (Tc_max > 0 && B > 1 && chunk_stride < Tc_max) return LEAF_ERR_BAD_SHAPE;
    const bool pcm = (flags & LEAF_FLAG_X_PCM16) != 0, out16 = (flags & LEAF_FLAG_OUT_PCM16) != 0;
    auto misaligned = [](const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; };
    if (misaligned(state, 15u) || misaligned(chunk, pcm ? 1u : 3u) || misaligned(table, 3u) || misaligned(out, out16 ? 1u : 3u))
        return LEAF_ERR_ALIGNMENT;
    // the positions: everything the kernel derives an address in `state`, `chunk` or `out` from, slot by slot
    bool work = n_max > 0;
    for (int b = 0; b < B; ++b) {
        const leaf_resample_slot& r = slots[b];
        if (r.idle) continue;
        if (resample_stream_slot_bad(q, r.hist_len, r.Tc, r.parity, r.shift, r.phase, r.n, r.drop_samples, r.end, n_max)) return LEAF_ERR_BAD_SHAPE;
        work = work || (!r.end && (long long)r.hist_len + r.Tc - r.drop_samples > 0);
    }
    const ResampleStreamLayout L = resample_stream_layout(B, q, pcm);
    if (state_bytes < L.total) return LEAF_ERR_WORKSPACE;
    if (!work) return LEAF_OK;                                            // no slot emits anything or keeps anything

    bool win_lds, taps_fit;
    resample_paths(q, s, win_lds, taps_fit);
    ResampleStreamParams p{};
    p.chunk = chunk; p.chunk_stride = chunk_stride;
    p.half[0] = static_cast<char*>(state); p.half[1] = static_cast<char*>(state) + L.half;
    p.table = static_cast<const int*>(table); p.out = out;
    p.n_max = n_max; p.H = L.H;
    p.o = q.o; p.n = q.n; p.width = q.width; p.K = q.K; p.stride = s.stride;
    p.window = (int)resample_window_samples(q);
    p.taps_fit = taps_fit ? 1 : 0;
    size_t lds = sizeof(float) * ((size_t)kResampleTile + (size_t)p.window);
    if (taps_fit) lds += (size_t)s.bytes - sizeof(int) * kResampleHeaderInts;
    const unsigned tiles = (unsigned)std::max<long long>(1, ((long long)n_max + kResampleTile - 1) / kResampleTile);
    const hipStream_t st = (hipStream_t)stream;
    for (int b0 = 0; b0 < B; b0 += kResampleBankSlots) {
        const int ns = std::min(B - b0, kResampleBankSlots);
        bool keep = false;
        for (int y = 0; y < ns; ++y) {
            const leaf_resample_slot& r = slots[b0 + y];
            ResampleSlotRec& w = p.rec[y];
            if (r.idle) {
                w = ResampleSlotRec{{0, 0, 0, 0, 1u << 17}};
                continue;
            }
            w = ResampleSlotRec{{(unsigned)r.hist_len | ((unsigned)r.shift << 16), (unsigned)r.Tc, (unsigned)r.n, (unsigned)r.drop_samples,
                                 (unsigned)r.phase | ((unsigned)r.parity << 16) | ((unsigned)r.end << 18)}};
            keep = keep || (!r.end && (long long)r.hist_len + r.Tc - r.drop_samples > 0);
        }
        if (n_max == 0 && !keep) continue;                                // (a launch whose slots keep nothing has nothing to do)
        p.b0 = b0;
        const dim3 grid(tiles, (unsigned)ns), block(kResampleThreads);
        switch ((pcm ? 2 : 0) | (out16 ? 1 : 0)) {
            case 0: hipLaunchKernelGGL((resample_stream_kernel<false, false>), grid, block, lds, st, p); break;
            case 1: hipLaunchKernelGGL((resample_stream_kernel<false, true>), grid, block, lds, st, p); break;
            case 2: hipLaunchKernelGGL((resample_stream_kernel<true, false>), grid, block, lds, st, p); break;
            default: hipLaunchKernelGGL((resample_stream_kernel<true, true>), grid, block, lds, st, p); break;
        }
        if (hipGetLastError() != hipSuccess) return LEAF_ERR_LAUNCH;
    }
    return LEAF_OK;
}
